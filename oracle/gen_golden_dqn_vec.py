"""oracle/gen_golden_dqn_vec.py -- TEST INFRASTRUCTURE ONLY.  One `Trainer.train()` of the reference's DQN (srl/algorithms/dqn/model_torch.py:89-131 with
`calc_target_q`, srl/algorithms/dqn/dqn.py:144-176) on a flat Box(4) observation with 2 actions, for the hidden blocks (64, 64) and (512,), with double DQN on
and off, B = 32, one terminal item -- run by the imported reference on CPU torch, to pin the MLP Q-network of libsrlx (srlx_mlpq_train_step) on the reference.

Run where the reference is ($SRL_REFERENCE):  python oracle/gen_golden_dqn_vec.py [OUT]
Only data is written (tests/golden/train_step_dqn_vec.npz), per case `<shape>_dd<0|1>.`: target_q [B], q0 [B][2] (online Q of s_0), loss, priorities [B],
`grad.<key>` (every p.grad) and `after.<key>` (every parameter after the Adam step).  The weights and the batch are NOT stored: tests/dqn_vec_recipe.py
regenerates them from seeds.
"""
import os

import numpy as np

import _golden_record as G
import dqn_vec_recipe as R  # noqa: E402


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
    rec = G.record_train_step(trainer, memory, batches, weights, dict(q=parameter.q_online), hook=(parameter, "calc_target_q", lambda out: out),
                              q_net=parameter.q_online)
    out = dict(target_q=rec["hooked"][0].astype(np.float32), q0=rec["q"], loss=np.float32(trainer.info["loss"]), priorities=rec["priorities"].astype(np.float32),
               lr=np.float64(rl_config.lr), discount=np.float64(rl_config.discount))
    for k, v in parameter.q_online.state_dict().items():
        out["grad." + k] = rec["grads"]["q", k].astype(np.float32)
        out["after." + k] = v.detach().numpy().astype(np.float32)
    return out


def main(out=G.GOLDEN):
    G.register_envs()
    save = {}
    for sk, hidden in R.SHAPES.items():
        for dd in R.DOUBLE:
            name = R.case_name(sk, dd)
            for k, v in run_case(hidden, dd).items():
                save[f"{name}.{k}"] = v
            print(f"{name}: loss={float(save[name + '.loss']):.6f} target range [{save[name + '.target_q'].min():.4f}, {save[name + '.target_q'].max():.4f}]")
    np.savez_compressed(os.path.join(out, "train_step_dqn_vec.npz"), **save)


if __name__ == "__main__":
    G.run(main, __doc__)
