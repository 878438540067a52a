"""A float64 yardstick for the MLP Q-network's learner step (libsrlx srlx_mlpq_train_step): the forward pass, the 1-step (double) DQN target with the optional
value rescaling, the importance-weighted Huber loss, priorities, every parameter's gradient by autograd, and torch's Adam written out -- plain torch float64 on
the CPU.  tests/test_dqn_vector_cpu.py pins it on the reference's recorded Trainer.train() (tests/golden/train_step_dqn_vec.npz) before any kernel is judged
by it.  `pick_items` draws learner batches on which float64 and float32 take the same branches (ReLU masks, the arg-max of s_1, the Huber knee).

Parameters are lists of tensors in EngineMLPQNet.kernel_parameters() order: weight [out][in] then bias of every layer, out_layer last."""
import os
import sys
import types

import numpy as np
import torch

_ORACLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle")
if _ORACLE not in sys.path:
    sys.path.insert(0, _ORACLE)
import hot_path_oracle as H  # noqa: E402  (rescaling / inverse_rescaling, pinned by tests/golden/functions.npz)

POOL = 320  # candidate items pick_items draws, whatever the batch size
KEEP = 256  # survivors it returns (the largest learner batch)


def init_params(D, widths, A, seed):
    """Every tensor uniform in +-1 / sqrt(fan_in) (biases: fan_in = their length) -- dqn_vec_recipe.recipe_state_dict's rule -- from a torch generator;
    float32 values held in float64."""
    g = torch.Generator().manual_seed(int(seed))
    out, prev = [], int(D)
    for n in list(widths) + [A]:
        for shape in ((n, prev), (n,)):
            bound = 1.0 / float(np.sqrt(shape[-1]))
            out.append(((torch.rand(shape, generator=g, dtype=torch.float32) * 2 - 1) * bound).double())
        prev = n
    return out


def forward(params, x, pre=None):
    """Linear + ReLU layers, then out_layer.  `pre` (a list) receives every hidden layer's pre-activation."""
    h = x
    n_layers = len(params) // 2
    for l in range(n_layers - 1):
        z = h @ params[2 * l].T + params[2 * l + 1]
        if pre is not None:
            pre.append(z)
        h = torch.relu(z)
    return h @ params[-2].T + params[-1]


def target_q(online, target, s1, rew, term, discount, double_dqn, rescale, sel_out=None):
    """dqn.py:144-176: the 1-step target (value from the target net at the arg-max of the online net under double DQN, of the target net otherwise)."""
    with torch.no_grad():
        qt = forward(target, s1)
        sel = forward(online, s1) if double_dqn else qt
        if sel_out is not None:
            sel_out.append(sel)
        maxq = qt.gather(1, sel.argmax(1, keepdim=True)).squeeze(1)
        if rescale:
            maxq = torch.from_numpy(H.inverse_rescaling(maxq.numpy()))
        t = rew + (1.0 - term) * discount * maxq
        if rescale:
            t = torch.from_numpy(H.rescaling(t.numpy()))
    return t


def learner_step(online, target, s0, s1, act, rew, term, w, discount, double_dqn, rescale=False):
    """dqn.py:144-176 + model_torch.py:89-131 in float64 autograd.  Returns a namespace: target [B], loss (float), priorities [B] = |target - q_a|, q0 [B][A] and
    grads (one tensor per parameter)."""
    t = target_q(online, target, s1, rew, term, discount, double_dqn, rescale)
    ps = [p.detach().clone().requires_grad_(True) for p in online]
    q = forward(ps, s0)
    qa = q.gather(1, act.view(-1, 1).long()).squeeze(1)
    loss = torch.nn.functional.huber_loss(t * w, qa * w, delta=1.0)
    grads = torch.autograd.grad(loss, ps)
    return types.SimpleNamespace(target=t, loss=float(loss.detach()), priorities=(t - qa).abs().detach(), q0=q.detach(), grads=[g.detach() for g in grads])


def adam_steps(params, grads_per_step, lr, betas=(0.9, 0.999), eps=1e-8):
    """torch.optim.Adam (no weight decay, no amsgrad) written out in float64 from zero state.  Returns, per step, the parameters after it, and the final
    exp_avg / exp_avg_sq."""
    b1, b2 = betas
    p = [x.double().clone() for x in params]
    m = [torch.zeros_like(x) for x in p]
    v = [torch.zeros_like(x) for x in p]
    after = []
    for t, grads in enumerate(grads_per_step, start=1):
        for i, g in enumerate(grads):
            g = g.double()
            m[i] = b1 * m[i] + (1 - b1) * g
            v[i] = b2 * v[i] + (1 - b2) * g * g
            denom = v[i].sqrt() / float(np.sqrt(1 - b2**t)) + eps
            p[i] = p[i] - (lr / (1 - b1**t)) * m[i] / denom
        after.append([x.clone() for x in p])
    return after, m, v


def pick_items(online, target, D, A, discount, double_dqn, rescale, seed):
    """KEEP learner items on which a float32 evaluation takes float64's branches, out of POOL candidates judged by the float64 reference alone.

    Candidates: observations standard normal, rewards uniform in [-2, 2], importance weights uniform in [0.5, 2.5], one in five terminal; all float32 values.
    The observations live in a pool of rows; every fourth candidate's s_0 is the previous candidate's s_1 (the ring shares rows the same way).  A candidate is
    discarded when a hidden pre-activation of s_0 is within 1e-5 * max |pre-activation of that layer| of zero, when the top two entries of the Q row that
    selects the action on s_1 are closer than 1e-5 * max |Q|, or when |w (target - q_a)| is within 1e-4 of the Huber knee.  The first KEEP survivors are
    returned with one terminal item, one non-terminal item and one item of each Huber branch moved to the front, so that the first B >= 4 items see all four.

    Returns a namespace: rows [P][D] float64, i0 / i1 [KEEP] (row numbers of s_0 / s_1), act int64, rew, term, w float64 [KEEP], linear bool [KEEP]."""
    g = torch.Generator().manual_seed(int(seed))
    rows = torch.randn(2 * POOL, D, generator=g, dtype=torch.float32).double()
    i0, i1 = torch.arange(POOL) * 2, torch.arange(POOL) * 2 + 1
    shared = torch.arange(1, POOL, 4)
    i0[shared] = i1[shared - 1]
    act = torch.randint(0, A, (POOL,), generator=g)
    rew = (torch.rand(POOL, generator=g, dtype=torch.float32) * 4 - 2).double()
    term = (torch.rand(POOL, generator=g) < 0.2).double()
    w = (torch.rand(POOL, generator=g, dtype=torch.float32) * 2 + 0.5).double()
    s0, s1 = rows[i0], rows[i1]
    ok = torch.ones(POOL, dtype=torch.bool)
    with torch.no_grad():
        pre = []
        q0 = forward(online, s0, pre)
        for z in pre:
            ok &= z.abs().min(1).values >= 1e-5 * float(z.abs().max())
        sel = []
        t = target_q(online, target, s1, rew, term, discount, double_dqn, rescale, sel)
        top = sel[0].topk(2, dim=1).values
        ok &= (top[:, 0] - top[:, 1]) >= 1e-5 * float(sel[0].abs().max())
        z = (w * (t - q0.gather(1, act.view(-1, 1)).squeeze(1))).abs()
        ok &= (z - 1.0).abs() >= 1e-4
    discarded = int((~ok).sum())
    assert discarded <= POOL // 10, f"{discarded} of {POOL} candidates discarded"
    keep = torch.nonzero(ok).squeeze(1)
    assert len(keep) >= KEEP, len(keep)
    keep = keep[:KEEP]
    linear, terminal = z[keep] > 1.0, term[keep] > 0
    assert int(linear.sum()) >= KEEP // 10 + 1 and int((~linear).sum()) >= KEEP // 10 + 1, int(linear.sum())
    assert bool(terminal.any()) and bool((~terminal).any())
    front = []
    for mask in (terminal, ~terminal, linear, ~linear):
        front.append(next(int(j) for j in torch.nonzero(mask).squeeze(1) if int(j) not in front))
    order = torch.tensor(front + [j for j in range(KEEP) if j not in front])
    keep = keep[order]
    return types.SimpleNamespace(rows=rows, i0=i0[keep], i1=i1[keep], act=act[keep], rew=rew[keep], term=term[keep], w=w[keep], linear=(z[keep] > 1.0))
