"""oracle/gen_golden_rainbow_vec.py -- TEST INFRASTRUCTURE ONLY.  One `Trainer.train()` of the reference's Rainbow (srl/algorithms/rainbow/model_torch.py:85-122
with `calc_target_q`, srl/algorithms/rainbow/rainbow.py:185-287, or rainbow_nomultisteps.py:10-43 at multisteps = 1) on a flat Box(4) observation with 2
actions, B = 32, for the cases of tests/rainbow_vec_recipe.py (dueling blocks with and without trunk layers, n = 1 / 3 / 5, double DQN on and off, retrace_h
1 and 0.5, rescale off) -- run by the imported reference on CPU torch, to pin the dueling MLP Q-network of libsrlx (srlx_mlpq_train_nstep) on the reference.

Run where the reference is ($SRL_REFERENCE):  python oracle/gen_golden_rainbow_vec.py [OUT]
Only data is written (tests/golden/train_step_rainbow_vec.npz), per case `<name>.`: target_q [B], q0 [B][2] (online Q of s_0), loss, priorities [B],
`grad.<key>` (every p.grad) and `after.<key>` (every parameter after the Adam step).  The weights and the batch are NOT stored: tests/rainbow_vec_recipe.py
regenerates them from seeds.
"""
import os

import numpy as np

import _golden_record as G
import rainbow_vec_recipe as R  # noqa: E402


def make_case(case, R, noisy=False):
    """The reference's Rainbow for one case of the recipe R, online and target network loaded with the recipe's weights."""
    import srl
    import torch
    from srl.algorithms import rainbow
    from srl.base.context import RunContext

    env = srl.EnvConfig("FlatGoldenEnv").make()
    rl_config = rainbow.Config()
    rl_config.enable_noisy_dense = noisy
    rl_config.input_block.value.set(case["in_sizes"])
    rl_config.hidden_block.set_dueling_network(case["layer_sizes"], dueling_type=case["dueling_type"])
    rl_config.batch_size = R.B
    rl_config.memory.capacity = 1000
    rl_config.memory.warmup_size = R.B
    rl_config.enable_double_dqn = case["double_dqn"]
    rl_config.multisteps = int(case["n"])
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
    return rl_config, parameter, memory, trainer, sd_on


def make_batches(case, R):
    states, actions, rewards, terminated, weights = R.make_items(case)
    n = int(case["n"])
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
    return batches, weights


def case_arrays(rl_config, parameter, trainer, rec):
    """What both flat Rainbow fixtures store of a recorded step."""
    out = dict(target_q=rec["hooked"][0].astype(np.float32), q0=rec["q"], loss=np.float32(trainer.info["loss"]), priorities=rec["priorities"].astype(np.float32),
               lr=np.float64(rl_config.lr), discount=np.float64(rl_config.discount))
    for k, v in parameter.q_online.state_dict().items():
        out["grad." + k] = rec["grads"]["q", k].astype(np.float32)
        out["after." + k] = v.detach().numpy().astype(np.float32)
    return out


def run_case(case):
    from srl.algorithms.rainbow import model_torch

    rl_config, parameter, memory, trainer, _ = make_case(case, R)
    batches, weights = make_batches(case, R)
    # at multisteps = 1 the trainer calls the module's calc_target_q (rainbow_nomultisteps.py:10-43), else the parameter's
    target = model_torch if int(case["n"]) == 1 else parameter
    rec = G.record_train_step(trainer, memory, batches, weights, dict(q=parameter.q_online), hook=(target, "calc_target_q", lambda out: out[0]),
                              q_net=parameter.q_online)
    return case_arrays(rl_config, parameter, trainer, rec)


def save_cases(path, cases, run_case):
    save = {}
    for name, case in cases.items():
        for k, v in run_case(case).items():
            save[f"{name}.{k}"] = v
        print(f"{name}: loss={float(save[name + '.loss']):.6f} target range [{save[name + '.target_q'].min():.4f}, {save[name + '.target_q'].max():.4f}]")
    np.savez_compressed(path, **save)


def main(out=G.GOLDEN):
    G.register_envs()
    save_cases(os.path.join(out, "train_step_rainbow_vec.npz"), R.CASES, run_case)


if __name__ == "__main__":
    G.run(main, __doc__)
