"""oracle/gen_golden_rainbow_noisy_vec.py -- TEST INFRASTRUCTURE ONLY.  One `Trainer.train()` of the reference's Rainbow with `enable_noisy_dense=True`
(srl/algorithms/rainbow/model_torch.py:85-122 with `calc_target_q`, srl/algorithms/rainbow/rainbow.py:185-287; NoisyLinear: srl/rl/torch_/modules/
noisy_linear.py:8-52) on a flat Box(4) observation with 2 actions, B = 32, for the cases of tests/rainbow_noisy_recipe.py -- run by the imported reference on CPU
torch, to pin the noisy dueling MLP Q-network of libsrlx (srlx_mlpq_bind_noisy, srlx_mlpq_train_nstep) on the reference.  `torch.randn` is wrapped for the
duration of the step: every noise tensor the reference draws is recorded in call order -- the online network's pass over s_1..s_n, the target network's, then
the online network's pass over s_0 (rainbow.py:224-225, model_torch.py:103), each drawing weight then bias noise of every noisy layer in module order.

Run where the reference is ($SRL_REFERENCE):  python oracle/gen_golden_rainbow_noisy_vec.py [OUT]
Only data is written (tests/golden/train_step_rainbow_noisy_vec.npz), per case `<name>.`: `eps_next.<key>`, `eps_target.<key>`, `eps_s0.<key>` (the three
draws, keyed by the mu tensor they perturb), target_q [B], q0 [B][2] (online Q of s_0), loss, priorities [B], `grad.<key>` (every p.grad, the sigmas' included)
and `after.<key>` (every parameter after the Adam step).  The parameters and the batch are NOT stored: tests/rainbow_noisy_recipe.py regenerates them.
"""
import os

import numpy as np

import _golden_record as G
import rainbow_noisy_recipe as R  # noqa: E402
from gen_golden_rainbow_vec import case_arrays, make_batches, make_case, save_cases


def run_case(case):
    import torch

    assert int(case["n"]) > 1
    rl_config, parameter, memory, trainer, sd_on = make_case(case, R, noisy=True)
    batches, weights = make_batches(case, R)
    noise = []
    _randn = torch.randn

    def randn(*a, **k):
        t = _randn(*a, **k)
        noise.append(t.detach().clone().numpy())
        return t

    torch.randn = randn
    try:
        rec = G.record_train_step(trainer, memory, batches, weights, dict(q=parameter.q_online), hook=(parameter, "calc_target_q", lambda out: out[0]),
                                  q_net=parameter.q_online)
    finally:
        torch.randn = _randn
    out = case_arrays(rl_config, parameter, trainer, rec)
    noisy = [mk for mk, sk in zip(R.mu_keys(case), R.sigma_keys(case)) if sk is not None]
    assert len(noise) == 3 * len(noisy), (len(noise), len(noisy))
    for d, label in enumerate(("eps_next", "eps_target", "eps_s0")):
        for j, mk in enumerate(noisy):
            t = noise[d * len(noisy) + j]
            assert t.shape == sd_on[mk].shape, (label, mk, t.shape)
            out[f"{label}.{mk}"] = t.astype(np.float32)
    return out


def main(out=G.GOLDEN):
    G.register_envs()
    save_cases(os.path.join(out, "train_step_rainbow_noisy_vec.npz"), R.CASES, run_case)


if __name__ == "__main__":
    G.run(main, __doc__)
