"""tools/gen_golden_rainbow_noisy_vec.py -- TEST INFRASTRUCTURE ONLY.  One `Trainer.train()` of the reference's Rainbow with `enable_noisy_dense=True`
(srl/algorithms/rainbow/model_torch.py:85-122 with `calc_target_q`, srl/algorithms/rainbow/rainbow.py:185-287; NoisyLinear: srl/rl/torch_/modules/
noisy_linear.py:8-52) on a flat Box(4) observation with 2 actions, B = 32, for the cases of tests/rainbow_noisy_recipe.py -- run by the imported reference on CPU
torch, to pin the noisy dueling MLP Q-network of libsrlx (srlx_mlpq_bind_noisy, srlx_mlpq_train_nstep) on the reference.  `torch.randn` is wrapped for the
duration of the step: every noise tensor the reference draws is recorded in call order -- the online network's pass over s_1..s_n, the target network's, then
the online network's pass over s_0 (rainbow.py:224-225, model_torch.py:103), each drawing weight then bias noise of every noisy layer in module order.

Run where the reference is importable:  PYTHONPATH=<reference root> python tools/gen_golden_rainbow_noisy_vec.py
Only data is written (tests/golden/train_step_rainbow_noisy_vec.npz), per case `<name>.`: `eps_next.<key>`, `eps_target.<key>`, `eps_s0.<key>` (the three
draws, keyed by the mu tensor they perturb), target_q [B], q0 [B][2] (online Q of s_0), loss, priorities [B], `grad.<key>` (every p.grad, the sigmas' included)
and `after.<key>` (every parameter after the Adam step).  The parameters and the batch are NOT stored: tests/rainbow_noisy_recipe.py regenerates them.
"""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rainbow_noisy_recipe as R  # noqa: E402
from gen_golden_rainbow_vec import _env_class  # noqa: E402


def run_case(case):
    import srl
    import torch
    from srl.algorithms import rainbow
    from srl.base.context import RunContext

    n = int(case["n"])
    assert n > 1
    env = srl.EnvConfig("FlatGoldenEnv").make()
    rl_config = rainbow.Config()
    rl_config.enable_noisy_dense = True
    rl_config.input_block.value.set(case["in_sizes"])
    rl_config.hidden_block.set_dueling_network(case["layer_sizes"], dueling_type=case["dueling_type"])
    rl_config.batch_size = R.B
    rl_config.memory.capacity = 1000
    rl_config.memory.warmup_size = R.B
    rl_config.enable_double_dqn = case["double_dqn"]
    rl_config.multisteps = n
    rl_config.retrace_h = case["retrace_h"]
    rl_config.set_torch()
    rl_config.setup(env)
    torch.manual_seed(0)
    parameter = rl_config.make_parameter()
    memory = rl_config.make_memory()
    trainer = rl_config.make_trainer(parameter, memory)
    trainer.setup(RunContext())
    keys_shapes = [(k, tuple(v.shape)) for k, v in parameter.q_online.state_dict().items()]
    assert keys_shapes == R.keys_shapes(case), keys_shapes
    sd_on, sd_tg = R.recipe_state_dict(case, R.SEED_ONLINE), R.recipe_state_dict(case, R.SEED_TARGET)
    parameter.q_online.load_state_dict({k: torch.tensor(v) for k, v in sd_on.items()})
    parameter.q_target.load_state_dict({k: torch.tensor(v) for k, v in sd_tg.items()})

    states, actions, rewards, terminated, weights = R.make_items(case)
    onehot = lambda a: [1.0 if k == a else 0.0 for k in range(R.A)]  # noqa: E731
    batches = []
    for b in range(R.B):  # rainbow.py:345-387: n + 1 tracked steps [state, onehot action, reward, terminated, next invalid actions]; step j carries transition j - 1
        steps = [[states[b, 0].copy(), onehot(0), 0.0, 0, []]]
        for m in range(n):
            steps.append([states[b, m + 1].copy(), onehot(actions[b, m]), float(rewards[b, m]), int(terminated[b, m]), []])
        batches.append(steps)
    rec = {}
    memory.sample = lambda *a, **k: (batches, weights.copy(), list(range(R.B)))
    memory.update = lambda update_args, priorities, step: rec.__setitem__("priorities", np.asarray(priorities).copy())
    memory.is_warmup_needed = lambda: False
    _calc = parameter.calc_target_q

    def calc(*a, **k):
        out = _calc(*a, **k)
        rec["target_q"] = np.asarray(out[0]).copy()
        return out

    parameter.calc_target_q = calc
    orig_forward = parameter.q_online.forward
    holder = {}

    def fwd(*a, **k):
        y = orig_forward(*a, **k)
        if y.requires_grad:
            holder["q"] = y.detach().clone()
        return y

    parameter.q_online.forward = fwd
    names = {id(p): k for k, p in parameter.q_online.named_parameters()}
    grads = {}
    _step = torch.optim.Adam.step

    def step(self, *a, **k):
        for g in self.param_groups:
            for p in g["params"]:
                if p.grad is not None and id(p) in names:
                    grads[names[id(p)]] = p.grad.detach().clone().numpy()
        return _step(self, *a, **k)

    torch.optim.Adam.step = step
    noise = []
    _randn = torch.randn

    def randn(*a, **k):
        t = _randn(*a, **k)
        noise.append(t.detach().clone().numpy())
        return t

    torch.randn = randn
    trainer.train_count = 1  # not a sync step
    trainer.train()
    torch.randn = _randn
    torch.optim.Adam.step = _step
    parameter.q_online.forward = orig_forward
    after = {k: v.detach().numpy().copy() for k, v in parameter.q_online.state_dict().items()}
    out = dict(target_q=rec["target_q"].astype(np.float32), q0=holder["q"].numpy(), loss=np.float32(trainer.info["loss"]),
               priorities=rec["priorities"].astype(np.float32), lr=np.float64(rl_config.lr), discount=np.float64(rl_config.discount))
    noisy = [mk for mk, sk in zip(R.mu_keys(case), R.sigma_keys(case)) if sk is not None]
    assert len(noise) == 3 * len(noisy), (len(noise), len(noisy))
    for d, label in enumerate(("eps_next", "eps_target", "eps_s0")):
        for j, mk in enumerate(noisy):
            t = noise[d * len(noisy) + j]
            assert t.shape == sd_on[mk].shape, (label, mk, t.shape)
            out[f"{label}.{mk}"] = t.astype(np.float32)
    for k, _ in keys_shapes:
        out["grad." + k] = grads[k].astype(np.float32)
        out["after." + k] = after[k].astype(np.float32)
    return out


def main():
    import torch
    from srl.base.env import registration

    torch.set_num_threads(8)
    import gen_golden_rainbow_vec as G

    G.FlatGoldenEnv = _env_class()
    registration.register("FlatGoldenEnv", entry_point="gen_golden_rainbow_vec:FlatGoldenEnv", check_duplicate=False)
    save = {}
    for name, case in R.CASES.items():
        for k, v in run_case(case).items():
            save[f"{name}.{k}"] = v
        print(f"{name}: loss={float(save[name + '.loss']):.6f} target range [{save[name + '.target_q'].min():.4f}, {save[name + '.target_q'].max():.4f}]")
    np.savez_compressed(os.path.join(OUT, "train_step_rainbow_noisy_vec.npz"), **save)


if __name__ == "__main__":
    main()
