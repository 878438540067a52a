"""tools/gen_golden_dqn84.py -- TEST INFRASTRUCTURE ONLY.  One `Trainer.train()` of the reference's DQN (srl/algorithms/dqn/model_torch.py:89-131 with
`calc_target_q`, srl/algorithms/dqn/dqn.py:144-176) at the Atari geometry -- 84 x 84 x 4 frames, 6 actions, one dense layer of 512, double DQN, B = 16, one
terminal item -- run by the imported reference on CPU torch, to pin the device engine's plain Q head (libsrlx dueling_type 3) on the reference directly.

Run where the reference is importable:  PYTHONPATH=<reference root> python tools/gen_golden_dqn84.py
Only data is written (tests/golden/train_step_dqn84.npz):
  frames uint8 [B][5][84][84], actions [B], reward [B], undone [B], weights [B]
  outputs of the reference: target_q [B], q0 [B][6] (online Q of s_0), loss, priorities [B]
  per parameter: 2048 sampled entries of p.grad (`grad.<key>`) and of the Adam step (`upd.<key>`) at positions `pos.<key>`, float64 sums (`sum.`, `abs.`, `gsum.`)
  and the gradient's largest magnitude (`gmax.`)
The weights are NOT stored: tests/dqn84_recipe.py regenerates them from seeds.
"""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import dqn84_recipe as R  # noqa: E402


def main():
    import srl
    import torch
    from srl.algorithms import dqn
    from srl.base.context import RunContext
    from srl.base.env import registration

    import _golden_env  # noqa: F401  (oracle/_golden_env.py: a tiny image environment registered from outside the reference's tree)

    torch.set_num_threads(8)
    registration.register("TinyImageEnvGolden", entry_point="_golden_env:TinyImageEnv", check_duplicate=False)
    env = srl.EnvConfig("TinyImageEnvGolden", kwargs=dict(hw=84, actions=R.A)).make()
    rl_config = dqn.Config()
    rl_config.set_atari_config()
    rl_config.window_length = 4
    rl_config.batch_size = R.B
    rl_config.memory.capacity = 1000
    rl_config.memory.warmup_size = R.B
    rl_config.memory.compress = False
    rl_config.enable_double_dqn = True
    rl_config.set_torch()
    rl_config.setup(env)
    torch.manual_seed(0)
    parameter = rl_config.make_parameter()
    memory = rl_config.make_memory()
    trainer = rl_config.make_trainer(parameter, memory)
    trainer.setup(RunContext())
    keys_shapes = [(k, tuple(v.shape)) for k, v in parameter.q_online.state_dict().items()]
    assert keys_shapes == R.KEYS_SHAPES, keys_shapes
    sd_on, sd_tg = R.recipe_state_dict(R.SEED_ONLINE), R.recipe_state_dict(R.SEED_TARGET)
    parameter.q_online.load_state_dict({k: torch.tensor(v) for k, v in sd_on.items()})
    parameter.q_target.load_state_dict({k: torch.tensor(v) for k, v in sd_tg.items()})

    frames, actions, reward, undone, weights = R.make_items()
    batches = []
    for b in range(R.B):  # the reference's item (dqn.py:234-246): [state, n_state, onehot action, reward, undone, next invalid actions], states (84, 84, 4) float32
        st = np.stack([frames[b, c] for c in range(4)], axis=-1).astype(np.float32) / 255
        nst = np.stack([frames[b, 1 + c] for c in range(4)], axis=-1).astype(np.float32) / 255
        onehot = [1.0 if a == actions[b] else 0.0 for a in range(R.A)]
        batches.append([st, nst, onehot, float(reward[b]), int(undone[b]), []])
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

    def fwd(x):
        y = orig_forward(x)
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
    after = {k: v.detach().numpy() for k, v in parameter.q_online.state_dict().items()}
    save = dict(frames=frames, actions=actions, reward=reward, undone=undone, weights=weights, target_q=rec["target_q"].astype(np.float32), q0=holder["q"].numpy(),
                loss=np.float32(trainer.info["loss"]), priorities=rec["priorities"].astype(np.float32), lr=np.float64(rl_config.lr),
                discount=np.float64(rl_config.discount))
    prng = np.random.default_rng(99)
    for k, _ in keys_shapes:
        d = (after[k].astype(np.float64) - sd_on[k].astype(np.float64)).reshape(-1)
        pos = np.sort(prng.choice(d.size, size=min(2048, d.size), replace=False))
        save["pos." + k] = pos.astype(np.int64)
        save["upd." + k] = d[pos].astype(np.float32)
        save["sum." + k] = np.float64(d.sum())
        save["abs." + k] = np.float64(np.abs(d).sum())
        g = grads[k].astype(np.float64).reshape(-1)
        save["grad." + k] = g[pos].astype(np.float32)
        save["gmax." + k] = np.float64(np.abs(g).max())
        save["gsum." + k] = np.float64(g.sum())
    np.savez_compressed(os.path.join(OUT, "train_step_dqn84.npz"), **save)
    print(f"train_step_dqn84: loss={float(trainer.info['loss']):.6f} target range [{rec['target_q'].min():.4f}, {rec['target_q'].max():.4f}]")


if __name__ == "__main__":
    main()
