"""Float64 yardstick of the C51 update (srl/algorithms/c51/c51.py:90-135), written from the cited lines as a different program from csrc/srlx_c51_math.h: the
projection is the reference's double loop (a SCATTER; the kernels gather), and the gradient comes from torch autograd through clamp and log (the kernels use the
closed form).  A helper of tests/test_c51_*.py, not a test.  The reference's C51 is TensorFlow and cannot run here: parity with it is unpinned.

The network is DQN's plain MLP (tests/mlpq_reference.py: init_params / forward) whose out_layer has A * N rows, read as [A][N]."""
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlpq_reference as M  # noqa: E402

CLIP_LO = 1e-6  # c51.py:131


def support(v_min, v_max, N):
    """c51.py:67 (float64)."""
    return torch.from_numpy(np.linspace(float(v_min), float(v_max), int(N)))


def init_params(D, widths, A, N, seed):
    return M.init_params(D, widths, A * N, seed)


def logits(params, x, A, N, pre=None):
    return M.forward(params, x, pre).view(x.shape[0], A, N)


def expectations(lg, v_min, v_max):
    """[rows][A] means of softmax(lg) over the support; TensorFlow multiplies by float32(Z) (:93, :167)."""
    z32 = support(v_min, v_max, lg.shape[-1]).float().to(lg.dtype)
    return (torch.softmax(lg, dim=2) * z32).sum(-1)


def project(next_dists, rew, term, discount, v_min, v_max):
    """c51.py:102-121: the distributional Bellman operator and the re-binning, numpy float64, the reference's scatter loop.  One guard that the reference does not
    have: idx >= N - 1 puts the whole mass on the last atom (the reference would index target_dists[N] where rounding lifts b a hair above N - 1).
    Returns (m [B][N], indices [B][N], ratios [B][N])."""
    nd = np.asarray(next_dists, np.float64)
    B, N = nd.shape
    Z = np.linspace(float(v_min), float(v_max), N)
    delta_z = (float(v_max) - float(v_min)) / (N - 1)
    rewards = np.tile(np.reshape(np.asarray(rew, np.float64), (-1, 1)), (1, N))
    dones = np.tile(np.reshape(np.asarray(term, np.float64), (-1, 1)), (1, N))
    TZ = rewards + (1 - dones) * float(discount) * np.tile(Z, (B, 1))
    TZ = np.minimum(float(v_max), np.maximum(float(v_min), TZ))
    bj = (TZ - float(v_min)) / delta_z
    ratios, indices = np.modf(bj)
    m = np.zeros((B, N))
    for i in range(B):
        for j in range(N):
            idx, ratio = int(indices[i][j]), ratios[i][j]
            if idx >= N - 1:
                idx, ratio = N - 1, 0.0
                indices[i][j], ratios[i][j] = idx, ratio
            m[i][idx] += nd[i][j] * (1 - ratio)
            if ratio != 0:
                m[i][idx + 1] += nd[i][j] * ratio
    return torch.from_numpy(m), indices.astype(np.int64), ratios


def loss_from_logits(lg0, act, m):
    """c51.py:126-135 on logits [B][A][N] (autograd-capable): (mean loss, per-item loss, unclipped p_0 [B][N])."""
    p0 = torch.softmax(lg0, dim=2)[torch.arange(lg0.shape[0]), act]
    item = (-m * torch.log(torch.clamp(p0, CLIP_LO, 1.0))).sum(1)
    return item.mean(), item, p0


def closed_form_grad(p0, m, act, A):
    """d mean-loss / d logits [B][A][N]: with u_i = m_i where CLIP_LO <= p_i <= 1 and 0 elsewhere, (p_k * sum_i u_i - u_k) / B on a_0's atoms, 0 elsewhere."""
    B, N = p0.shape
    u = torch.where((p0 >= CLIP_LO) & (p0 <= 1.0), m, torch.zeros_like(m))
    g = torch.zeros(B, A, N, dtype=torch.float64)
    g[torch.arange(B), act] = (p0 * u.sum(1, keepdim=True) - u) / B
    return g


def targets(params, s1, rew, term, discount, A, N, v_min, v_max):
    """(m [B][N], next actions [B], means of s' [B][A]) -- c51.py:90-121."""
    with torch.no_grad():
        lg1 = logits(params, s1, A, N)
        means = expectations(lg1, v_min, v_max)
        na = means.argmax(1)
        nd = torch.softmax(lg1, dim=2)[torch.arange(s1.shape[0]), na]
    m, _, _ = project(nd.numpy(), rew.numpy(), term.numpy(), discount, v_min, v_max)
    return m, na, means


def learner_step(params, s0, s1, act, rew, term, discount, A, N, v_min, v_max, dtype=torch.float64):
    """One C51 update's quantities in float64: q0 [B][A] expectations of s_0, p0 / m [B][N], loss, item_loss [B], grads (one per parameter), grad_logits
    [B][A * N], next actions.  `dtype=torch.float32` evaluates the same program with float32 tensors (the projection stays numpy float64 and m is rounded to
    float32, as in the reference): the yardstick's own float32 - float64 distance."""
    params, s0, s1 = [p.to(dtype) for p in params], s0.to(dtype), s1.to(dtype)
    m, na, _ = targets(params, s1, rew, term, discount, A, N, v_min, v_max)
    m = m.to(dtype)
    ps = [p.clone().requires_grad_(True) for p in params]
    lg0 = logits(ps, s0, A, N)
    loss, item, p0 = loss_from_logits(lg0, act, m)
    grads = torch.autograd.grad(loss, ps + [lg0])
    return types.SimpleNamespace(q0=expectations(lg0.detach(), v_min, v_max), p0=p0.detach(), m=m, loss=float(loss.detach()), item_loss=item.detach(),
                                 grads=[g.detach() for g in grads[:-1]], grad_logits=grads[-1].detach().reshape(s0.shape[0], A * N), next_actions=na)


def interior_atom_reward(v_min, v_max, N):
    """(reward, atom j): a float32 reward that IS atom j of the support with b_j = j exactly (the ratio == 0 branch of c51.py:118-121), interior where the
    support has such an atom (nearest the middle), else atom 0 (v_min: b = 0)."""
    Z = np.linspace(float(v_min), float(v_max), N)
    dz = (float(v_max) - float(v_min)) / (N - 1)
    for j in sorted(range(1, N - 1), key=lambda j: abs(j - N // 2)):
        if float(np.float32(Z[j])) == Z[j] and np.modf((Z[j] - float(v_min)) / dz) == (0.0, float(j)):
            return float(Z[j]), j
    return float(np.float32(v_min)), 0


FORCED = 4  # the items pick_items places first: above v_max, below v_min, on an atom, non-terminated with reward 0


def pick_items(params, D, A, N, v_min, v_max, discount, seed, need):
    """`need` learner items on which a float32 evaluation takes float64's branches, out of 2 * need candidates judged by the float64 yardstick alone.

    Candidates: observations standard normal, rewards uniform in +-0.25 (v_max - v_min), one in five terminated; float32 values.  The observations live in a
    pool of rows; every fourth candidate's s_0 is the previous candidate's s_1 (the ring shares rows the same way).  Dropped, each rule by itself at most 5 % of
    the candidates (asserted):
      tie    the two best means of s' lie closer than 16 * N * 2^-24 * max(|v_min|, |v_max|), sixteen times the float32 rounding a mean of N terms can carry:
             a tie the kernel may break the other way changes the whole target;
      edge   an atom of a_0 has a probability within a factor 1 +- 1e-3 of 1e-6, the clip's edge.
    And, as tests/mlpq_reference.py:pick_items drops them (at most 10 %): a hidden pre-activation of s_0 within 1e-5 * max |pre-activation of that layer| of
    zero -- a ReLU whose float32 mask may differ moves a whole weight row's gradient.
    The first FORCED survivors get their reward and termination overwritten (neither rule reads them): terminated with reward v_max + 1 (all mass on the last
    atom, ratio 0), terminated with reward v_min - 1, terminated with a reward that is exactly an atom (`interior_atom_reward`), non-terminated with reward 0.

    Returns a namespace: rows [P][D] float64, i0 / i1 [need] (row numbers of s_0 / s_1), act int64, rew, term float64 [need], atom (the forced atom's index)."""
    pool = 2 * int(need)
    g = torch.Generator().manual_seed(int(seed))
    rows = torch.randn(2 * pool, D, generator=g, dtype=torch.float32).double()
    i0, i1 = torch.arange(pool) * 2, torch.arange(pool) * 2 + 1
    shared = torch.arange(1, pool, 4)
    i0[shared] = i1[shared - 1]
    act = torch.randint(0, A, (pool,), generator=g)
    rew = ((torch.rand(pool, generator=g, dtype=torch.float32) * 2 - 1) * np.float32(0.25 * (float(v_max) - float(v_min)))).double()
    term = (torch.rand(pool, generator=g) < 0.2).double()
    with torch.no_grad():
        pre = []
        p0 = torch.softmax(logits(params, rows[i0], A, N, pre), dim=2)[torch.arange(pool), act]
        relu = torch.zeros(pool, dtype=torch.bool)
        for z in pre:
            relu |= z.abs().min(1).values < 1e-5 * float(z.abs().max())
        top = expectations(logits(params, rows[i1], A, N), v_min, v_max).topk(2, dim=1).values
        tie = (top[:, 0] - top[:, 1]) < 16 * N * 2.0 ** -24 * max(abs(float(v_min)), abs(float(v_max)))
        edge = ((p0 > CLIP_LO * (1 - 1e-3)) & (p0 < CLIP_LO * (1 + 1e-3))).any(1)
    assert int(tie.sum()) <= pool // 20, f"tie rule: {int(tie.sum())} of {pool} candidates"
    assert int(edge.sum()) <= pool // 20, f"edge rule: {int(edge.sum())} of {pool} candidates"
    assert int(relu.sum()) <= pool // 10, f"ReLU rule: {int(relu.sum())} of {pool} candidates"
    keep = torch.nonzero(~(tie | edge | relu)).squeeze(1)
    assert len(keep) >= need, (len(keep), need)
    keep = keep[:need]
    rew, term = rew[keep].clone(), term[keep].clone()
    r_atom, atom = interior_atom_reward(v_min, v_max, N)
    forced = [(float(np.float32(float(v_max) + 1.0)), 1.0), (float(np.float32(float(v_min) - 1.0)), 1.0), (r_atom, 1.0), (0.0, 0.0)]
    for k, (r, t) in enumerate(forced[:min(FORCED, int(need))]):
        rew[k], term[k] = r, t
    return types.SimpleNamespace(rows=rows, i0=i0[keep], i1=i1[keep], act=act[keep], rew=rew, term=term, atom=atom,
                                 dropped=dict(tie=int(tie.sum()), edge=int(edge.sum()), relu=int(relu.sum()), pool=pool))
