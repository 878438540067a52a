"""tools/gen_golden_dqn_vec.py -- TEST INFRASTRUCTURE ONLY.  One `Trainer.train()` of the reference's DQN (srl/algorithms/dqn/model_torch.py:89-131 with
`calc_target_q`, srl/algorithms/dqn/dqn.py:144-176) on a flat Box(4) observation with 2 actions, for the hidden blocks (64, 64) and (512,), with double DQN on
and off, B = 32, one terminal item -- run by the imported reference on CPU torch, to pin the MLP Q-network of libsrlx (srlx_mlpq_train_step) on the reference.

Run where the reference is importable:  PYTHONPATH=<reference root> python tools/gen_golden_dqn_vec.py
Only data is written (tests/golden/train_step_dqn_vec.npz), per case `<shape>_dd<0|1>.`: target_q [B], q0 [B][2] (online Q of s_0), loss, priorities [B],
`grad.<key>` (every p.grad) and `after.<key>` (every parameter after the Adam step).  The weights and the batch are NOT stored: tests/dqn_vec_recipe.py
regenerates them from seeds.
"""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dqn_vec_recipe as R  # noqa: E402


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


def run_case(hidden, double_dqn: bool):
    import srl
    import torch
    from srl.algorithms import dqn
    from srl.base.context import RunContext

    env = srl.EnvConfig("FlatGoldenEnv").make()
    rl_config = dqn.Config()
    rl_config.hidden_block.set(hidden)
    rl_config.batch_size = R.B
    rl_config.memory.capacity = 1000
    rl_config.memory.warmup_size = R.B
    rl_config.enable_double_dqn = double_dqn
    rl_config.set_torch()
    rl_config.setup(env)
    torch.manual_seed(0)
    parameter = rl_config.make_parameter()
    memory = rl_config.make_memory()
    trainer = rl_config.make_trainer(parameter, memory)
    trainer.setup(RunContext())
    keys_shapes = [(k, tuple(v.shape)) for k, v in parameter.q_online.state_dict().items()]
    assert keys_shapes == R.keys_shapes(hidden), keys_shapes
    sd_on, sd_tg = R.recipe_state_dict(hidden, R.SEED_ONLINE), R.recipe_state_dict(hidden, R.SEED_TARGET)
    parameter.q_online.load_state_dict({k: torch.tensor(v) for k, v in sd_on.items()})
    parameter.q_target.load_state_dict({k: torch.tensor(v) for k, v in sd_tg.items()})

    s0, s1, actions, reward, undone, weights = R.make_items()
    batches = []
    for b in range(R.B):  # the reference's item (dqn.py:234-246): [state, n_state, onehot action, reward, undone, next invalid actions]
        onehot = [1.0 if a == actions[b] else 0.0 for a in range(R.A)]
        batches.append([s0[b].copy(), s1[b].copy(), onehot, float(reward[b]), int(undone[b]), []])
    rec = {}
    memory.sample = lambda *a, **k: (batches, weights.copy(), list(range(R.B)))
    memory.update = lambda update_args, priorities, step: rec.__setitem__("priorities", np.asarray(priorities).copy())
    memory.is_warmup_needed = lambda: False
    _calc = parameter.calc_target_q

    def calc(*a, **k):
        out = _calc(*a, **k)
        rec["target_q"] = np.asarray(out).copy()
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
    for sk, hidden in R.SHAPES.items():
        for dd in R.DOUBLE:
            name = R.case_name(sk, dd)
            for k, v in run_case(hidden, dd).items():
                save[f"{name}.{k}"] = v
            print(f"{name}: loss={float(save[name + '.loss']):.6f} target range [{save[name + '.target_q'].min():.4f}, {save[name + '.target_q'].max():.4f}]")
    np.savez_compressed(os.path.join(OUT, "train_step_dqn_vec.npz"), **save)


if __name__ == "__main__":
    main()
