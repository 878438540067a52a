"""oracle/gen_golden_dqn84.py -- TEST INFRASTRUCTURE ONLY.  One `Trainer.train()` of the reference's DQN (srl/algorithms/dqn/model_torch.py:89-131 with
`calc_target_q`, srl/algorithms/dqn/dqn.py:144-176) at the Atari geometry -- 84 x 84 x 4 frames, 6 actions, one dense layer of 512, double DQN, B = 16, one
terminal item -- run by the imported reference on CPU torch, to pin the device engine's plain Q head (libsrlx dueling_type 3) on the reference directly.

Run where the reference is ($SRL_REFERENCE):  python oracle/gen_golden_dqn84.py [OUT]
Only data is written (tests/golden/train_step_dqn84.npz):
  frames uint8 [B][5][84][84], actions [B], reward [B], undone [B], weights [B]
  outputs of the reference: target_q [B], q0 [B][6] (online Q of s_0), loss, priorities [B]
  per parameter: 2048 sampled entries of p.grad (`grad.<key>`) and of the Adam step (`upd.<key>`) at positions `pos.<key>`, float64 sums (`sum.`, `abs.`, `gsum.`)
  and the gradient's largest magnitude (`gmax.`)
The weights are NOT stored: tests/dqn84_recipe.py regenerates them from seeds.
"""
import os

import numpy as np

import _golden_record as G
import dqn84_recipe as R  # noqa: E402


def main(out=G.GOLDEN):
    import srl
    import torch
    from srl.algorithms import dqn
    from srl.base.context import RunContext

    G.register_envs()
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
    rec = G.record_train_step(trainer, memory, batches, weights, dict(q=parameter.q_online), hook=(parameter, "calc_target_q", lambda out: out),
                              q_net=parameter.q_online)
    target_q = rec["hooked"][0]
    save = dict(frames=frames, actions=actions, reward=reward, undone=undone, weights=weights, target_q=target_q.astype(np.float32), q0=rec["q"],
                loss=np.float32(trainer.info["loss"]), priorities=rec["priorities"].astype(np.float32), lr=np.float64(rl_config.lr),
                discount=np.float64(rl_config.discount))
    prng = np.random.default_rng(99)
    for k, v in parameter.q_online.state_dict().items():
        G.sampled_entries(save, prng, k, sd_on[k], v.detach().numpy(), rec["grads"]["q", k], step_sums=True)
    np.savez_compressed(os.path.join(out, "train_step_dqn84.npz"), **save)
    print(f"train_step_dqn84: loss={float(trainer.info['loss']):.6f} target range [{target_q.min():.4f}, {target_q.max():.4f}]")


if __name__ == "__main__":
    G.run(main, __doc__)
