"""tools/gen_golden_rainbow_vec.py -- TEST INFRASTRUCTURE ONLY.  One `Trainer.train()` of the reference's Rainbow (srl/algorithms/rainbow/model_torch.py:85-122
with `calc_target_q`, srl/algorithms/rainbow/rainbow.py:185-287, or rainbow_nomultisteps.py:10-43 at multisteps = 1) on a flat Box(4) observation with 2
actions, B = 32, for the cases of tests/rainbow_vec_recipe.py (dueling blocks with and without trunk layers, n = 1 / 3 / 5, double DQN on and off, retrace_h
1 and 0.5, rescale off) -- run by the imported reference on CPU torch, to pin the dueling MLP Q-network of libsrlx (srlx_mlpq_train_nstep) on the reference.

Run where the reference is importable:  PYTHONPATH=<reference root> python tools/gen_golden_rainbow_vec.py
Only data is written (tests/golden/train_step_rainbow_vec.npz), per case `<name>.`: target_q [B], q0 [B][2] (online Q of s_0), loss, priorities [B],
`grad.<key>` (every p.grad) and `after.<key>` (every parameter after the Adam step).  The weights and the batch are NOT stored: tests/rainbow_vec_recipe.py
regenerates them from seeds.
"""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))

import rainbow_vec_recipe as R  # noqa: E402


def _env_class():
    from srl.base.env.base import EnvBase
    from srl.base.spaces.box import BoxSpace
    from srl.base.spaces.discrete import DiscreteSpace

    class FlatGoldenEnv(EnvBase):
        """Box(4) float32 observations, 2 actions: only its spaces matter here (the batch is handed to the trainer directly)."""

        action_space = property(lambda self: DiscreteSpace(R.A))
        observation_space = property(lambda self: BoxSpace((R.D,), -10.0, 10.0, np.float32))
        max_episode_steps = property(lambda self: 100)
        player_num = property(lambda self: 1)

        def reset(self, **kwargs):
            return np.zeros(R.D, np.float32)

        def step(self, action):
            return np.zeros(R.D, np.float32), 1.0, False, False

    return FlatGoldenEnv


def run_case(case):
    import srl
    import torch
    from srl.algorithms import rainbow
    from srl.algorithms.rainbow import model_torch
    from srl.base.context import RunContext

    n = int(case["n"])
    env = srl.EnvConfig("FlatGoldenEnv").make()
    rl_config = rainbow.Config()
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
    for b in range(R.B):
        if n == 1:  # rainbow_nomultisteps.py:101-108: [state, n_state, onehot action, reward, undone, next invalid actions]
            batches.append([states[b, 0].copy(), states[b, 1].copy(), onehot(actions[b, 0]), float(rewards[b, 0]), int(1 - terminated[b, 0]), []])
        else:  # rainbow.py:345-387: n + 1 tracked steps [state, onehot action, reward, terminated, next invalid actions]; step j carries transition j - 1
            steps = [[states[b, 0].copy(), onehot(0), 0.0, 0, []]]
            for m in range(n):
                steps.append([states[b, m + 1].copy(), onehot(actions[b, m]), float(rewards[b, m]), int(terminated[b, m]), []])
            batches.append(steps)
    rec = {}
    memory.sample = lambda *a, **k: (batches, weights.copy(), list(range(R.B)))
    memory.update = lambda update_args, priorities, step: rec.__setitem__("priorities", np.asarray(priorities).copy())
    memory.is_warmup_needed = lambda: False
    if n == 1:
        _calc1 = model_torch.calc_target_q

        def calc1(*a, **k):
            out = _calc1(*a, **k)
            rec["target_q"] = np.asarray(out[0]).copy()
            return out

        model_torch.calc_target_q = calc1
    else:
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
    trainer.train_count = 1  # not a sync step
    trainer.train()
    torch.optim.Adam.step = _step
    parameter.q_online.forward = orig_forward
    if n == 1:
        model_torch.calc_target_q = _calc1
    after = {k: v.detach().numpy().copy() for k, v in parameter.q_online.state_dict().items()}
    out = dict(target_q=rec["target_q"].astype(np.float32), q0=holder["q"].numpy(), loss=np.float32(trainer.info["loss"]),
               priorities=rec["priorities"].astype(np.float32), lr=np.float64(rl_config.lr), discount=np.float64(rl_config.discount))
    for k, _ in keys_shapes:
        out["grad." + k] = grads[k].astype(np.float32)
        out["after." + k] = after[k].astype(np.float32)
    return out


def main():
    import torch
    from srl.base.env import registration

    torch.set_num_threads(8)
    globals()["FlatGoldenEnv"] = _env_class()
    registration.register("FlatGoldenEnv", entry_point=__name__ + ":FlatGoldenEnv", check_duplicate=False)
    save = {}
    for name, case in R.CASES.items():
        for k, v in run_case(case).items():
            save[f"{name}.{k}"] = v
        print(f"{name}: loss={float(save[name + '.loss']):.6f} target range [{save[name + '.target_q'].min():.4f}, {save[name + '.target_q'].max():.4f}]")
    np.savez_compressed(os.path.join(OUT, "train_step_rainbow_vec.npz"), **save)


if __name__ == "__main__":
    main()
