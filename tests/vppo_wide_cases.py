"""Shared by tests/test_vppo_wide_cpu.py and tests/test_vppo_wide_gpu.py: the cases of the gemm-only V-PPO handle (srlx_vppo_create_gemm) in
tests/vppo_cases.py's tuple layout, with seeded parameters and two batches per case built by vppo_cases' construction (ratios from RATIOS, Huber arguments from
HUBER_ARGS plus jitter, the first seed whose yardstick margin is >= 3e-3).  The shapes are the smallest at which k_mlp_gemm_wgrad can go wrong."""
import copy
import functools

import torch

import vppo_cases as C
from simple_distributed_rl_amd.algorithms import ppo_v

# name: B, D, head (0 categorical, 1 Normal), n_out, trunk, value block, policy block, squashed, entropy_weight, max_grad_norm, forced
CASES = {
    "one-row": (1, 1, 0, 2, (32,), (), (), False, 0.0, 10.0, False),  # a chunk with one row, element loads
    "chunk-b63": (63, 3, 0, 5, (32, 96), (32,), (), False, 0.1, 10.0, False),  # the chunk edge, a width that is no multiple of 64, non-vector state loads
    "chunk-b64": (64, 3, 0, 5, (32, 96), (32,), (), False, 0.1, 0.01, False),
    "chunk-b65": (65, 3, 0, 5, (32, 96), (32,), (), False, 0.0, 10.0, False),
    "normal-b130": (130, 1, 1, 8, (96,), (), (64, 64), True, 0.1, 10.0, False),  # both heads through kHeadCols and the kNormalLs offset
    "past-b257": (257, 256, 0, 16, (512,), (512,), (), False, 0.1, 10.0, False),  # first batch past the old envelope at the widest tiles
    "max-b4096": (4096, 4, 0, 2, (64, 64), (64,), (), False, 0.0, 0.01, False),  # the maximum, ppo_v.Config()'s blocks
}
NAMES = list(CASES)
TRAINER = {"trainer-b512": (512, 4, 0, 2, (64, 64), (64,), (), False, 0.1, 10.0, False)}  # an ordinary PPO minibatch through ppo_v.Trainer
_ALL = dict(CASES, **TRAINER)


def make_parameter(name, device="cpu"):
    """Seeded parameters of the case (vppo_cases.make_parameter's recipe: no bias is zero)."""
    B, D, head, n_out, trunk, value, policy, squashed, ew, max_norm, _ = _ALL[name]
    seed = 2000 + list(_ALL).index(name)
    torch.manual_seed(seed)
    p = ppo_v.Parameter(C.make_config(D, head, n_out, trunk, value, policy, device=device, batch_size=B, squashed_gaussian_policy=squashed, entropy_weight=ew,
                                      max_grad_norm=max_norm, lr=C.LR, discount=C.DISCOUNT, clip_range=C.CLIP, loss_align_coeff=C.ALIGN))
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for t in p.net.parameters():
            if t.dim() == 1:
                t.copy_((torch.randn(t.shape, generator=g) * 0.1).to(t.device))
    return p


def _build_batch(name, y, seed):
    """vppo_cases._build_batch for a case of this module: one batch around the forward pass of the yardstick `y` as it stands (not modified)."""
    B, D, head, n_out = _ALL[name][:4]
    K = n_out if head else 1
    g = torch.Generator().manual_seed(seed)
    state, n_state = ((0.5 * torch.randn(B, D, generator=g)).float().double() for _ in range(2))
    action = (torch.randn(B, K, generator=g) * 0.7).float().double() if head else torch.randint(0, n_out, (B,), generator=g)
    not_term = (torch.rand(B, generator=g) < 0.8).double()
    not_term[0] = 0.0
    if B > 1:
        not_term[1] = 1.0
    total_reward = torch.randn(B, generator=g).float().double()
    ratio = torch.tensor(C.RATIOS)[torch.randint(0, 4, (B, K), generator=g)].double()
    d_arg = torch.tensor(C.HUBER_ARGS)[torch.randint(0, 4, (B,), generator=g)].double() + 0.05 * torch.rand(B, generator=g).double()
    probe = copy.deepcopy(y).update(state, n_state, action, torch.zeros(B, K, dtype=torch.float64), torch.zeros(B, dtype=torch.float64), not_term, total_reward)
    old_logpi = (probe["new_logpi"] - torch.log(ratio)).float().double()
    reward = ((d_arg + probe["v"]) / ratio[:, 0] - not_term * C.DISCOUNT * probe["n_v"]).float().double()
    return dict(state=state, n_state=n_state, action=action, old_logpi=old_logpi, reward=reward, not_terminated=not_term, total_reward=total_reward)


@functools.lru_cache(maxsize=None)
def _trajectory(name):
    """The yardstick's two updates of the case, each on the first of its seeds that puts nothing within 3e-3 of a kink.  Computed once, shared, never modified."""
    y = C._yardstick(name, make_parameter(name))
    batches, outs = [], []
    for k in range(2):
        for attempt in range(200):
            b = _build_batch(name, y, 100 * (50 + list(_ALL).index(name)) + k + 7919 * attempt)
            trial = copy.deepcopy(y)
            out = trial.update(**b)
            if out["margin"] >= 3e-3:
                break
        else:
            raise AssertionError(f"{name}: no batch away from the kinks in 200 seeds")
        y = trial
        batches.append(b), outs.append(out)
    return batches, outs


def make_batches(name):
    return _trajectory(name)[0]


def reference(name):
    return _trajectory(name)[1]
