"""A float64 yardstick for Rainbow's learner step on flat observations (libsrlx srlx_mlpq_create_dueling / srlx_mlpq_train_nstep): the dueling forward pass,
the n-step retrace target with the optional value rescaling, the importance-weighted Huber loss, priorities, every parameter's gradient by autograd, and
torch's Adam written out -- plain torch float64 on the CPU.  tests/test_rainbow_vector_cpu.py pins it on the reference's recorded Trainer.train()
(tests/golden/train_step_rainbow_vec.npz) before any kernel is judged by it.  `pick_items` draws learner batches on which float64 and float32 take the same
branches (ReLU masks, the arg-max of every step, the Huber knee).

Parameters are lists of tensors in EngineMLPQNet.kernel_parameters() order: weight [out][in] then bias of every trunk layer, then of v_layers.0, v_layers.2,
adv_layers.0, adv_layers.2."""
import os
import sys
import types

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (_HERE, os.path.join(_HERE, "..", "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import hot_path_oracle as H  # noqa: E402  (rescaling / inverse_rescaling, pinned by tests/golden/functions.npz)
from mlpq_reference import adam_steps  # noqa: E402,F401  (torch's Adam in float64: the same for every parameter list)

import rainbow_vec_recipe as RC  # noqa: E402

POOL = 400  # candidate items pick_items draws, whatever the batch size
KEEP = 256  # survivors it returns (the largest learner batch)
GREEDY_SHARE = 0.6


# (D, trunk, H, A, dueling_type, n): the envelope shapes the GPU tests run (tests/test_rainbow_vector_gpu.py) and pick_items is checked on
ENVELOPE = [
    (1, (), 32, 2, "average", 1),
    (4, (), 512, 2, "average", 3),
    (256, (512, 512), 512, 32, "", 7),
    (3, (64,), 96, 3, "average", 2),
    (17, (96, 32), 480, 5, "", 4),
    (8, (32,), 64, 4, "average", 5),
]


def golden_inputs(name):
    """The float64 parameter lists and the items of one recorded case, in kernel_parameters() order."""
    case = RC.CASES[name]
    keys = [k for k, _ in RC.keys_shapes(case)]
    on = [torch.tensor(RC.recipe_state_dict(case, RC.SEED_ONLINE)[k]).double() for k in keys]
    tg = [torch.tensor(RC.recipe_state_dict(case, RC.SEED_TARGET)[k]).double() for k in keys]
    states, actions, rewards, terminated, weights = (torch.tensor(a) for a in RC.make_items(case))
    return case, keys, on, tg, types.SimpleNamespace(states=states, act=actions, rew=rewards, term=terminated, w=weights)


def init_params(D, trunk, units, A, seed):
    """Every tensor uniform in +-1 / sqrt(fan_in) (biases: fan_in = their length) from a torch generator; float32 values held in float64."""
    g = torch.Generator().manual_seed(int(seed))
    shapes, prev = [], int(D)
    for n in trunk:
        shapes += [(n, prev), (n,)]
        prev = n
    shapes += [(units, prev), (units,), (1, units), (1,), (units, prev), (units,), (A, units), (A,)]
    out = []
    for shape in shapes:
        bound = 1.0 / float(np.sqrt(shape[-1]))
        out.append(((torch.rand(shape, generator=g, dtype=torch.float32) * 2 - 1) * bound).double())
    return out


def forward(params, x, dueling_type, pre=None):
    """Linear + ReLU trunk layers, then the dueling head (srl/rl/torch_/blocks/dueling_network.py:41-59).  `pre` (a list) receives every hidden pre-activation:
    the trunk's, then the value branch's and the advantage branch's."""
    h = x
    n_trunk = len(params) // 2 - 4
    for l in range(n_trunk):
        z = h @ params[2 * l].T + params[2 * l + 1]
        if pre is not None:
            pre.append(z)
        h = torch.relu(z)
    vw0, vb0, vw1, vb1, aw0, ab0, aw1, ab1 = params[2 * n_trunk:]
    zv, za = h @ vw0.T + vb0, h @ aw0.T + ab0
    if pre is not None:
        pre += [zv, za]
    v, adv = torch.relu(zv) @ vw1.T + vb1, torch.relu(za) @ aw1.T + ab1
    if dueling_type == "average":
        return v + adv - adv.mean(-1, keepdim=True)
    assert dueling_type == ""
    return v + adv


def target_q(online, target, s_next, act, rew, term, discount, retrace_h, double_dqn, rescale, dueling_type, sel_out=None):
    """rainbow.py:185-287 in float64.  s_next [B][n][D] = s_1..s_n; act int64, rew, term [B][n].  `sel_out` receives the Q rows that select the actions."""
    B, n, D = s_next.shape
    with torch.no_grad():
        qon = forward(online, s_next.reshape(B * n, D), dueling_type).view(B, n, -1)
        qtg = forward(target, s_next.reshape(B * n, D), dueling_type).view(B, n, -1)
        sel = qon if double_dqn else qtg
        if sel_out is not None:
            sel_out.append(sel)
        nact = sel.argmax(-1)
        maxq = qtg.gather(2, nact.unsqueeze(-1)).squeeze(-1)
        if rescale:
            maxq = torch.from_numpy(H.inverse_rescaling(maxq.numpy()))
        gain = rew + (1.0 - term) * discount * maxq
        if rescale:
            gain = torch.from_numpy(H.rescaling(gain.numpy()))
        qsel = torch.zeros_like(gain)
        if n > 1:
            qsel[:, 1:] = qon[:, : n - 1].gather(2, act[:, 1:].long().unsqueeze(-1)).squeeze(-1)
        td = gain - qsel
        c = torch.ones_like(gain)
        for m in range(1, n):
            c[:, m] = c[:, m - 1] * retrace_h * (act[:, m].long() == nact[:, m]).double()
        disc = torch.tensor([float(discount) ** m for m in range(n)], dtype=torch.float64)
        return (td * disc * c).sum(1)


def learner_step(online, target, states, act, rew, term, w, discount, retrace_h, double_dqn, rescale, dueling_type):
    """rainbow.py:185-287 + model_torch.py:85-122 in float64 autograd.  states [B][n + 1][D].  Returns a namespace: target [B], loss (float), priorities [B] =
    |target - q_a|, q0 [B][A] and grads (one tensor per parameter)."""
    t = target_q(online, target, states[:, 1:], act, rew, term, discount, retrace_h, double_dqn, rescale, dueling_type)
    ps = [p.detach().clone().requires_grad_(True) for p in online]
    q = forward(ps, states[:, 0], dueling_type)
    qa = q.gather(1, act[:, :1].long()).squeeze(1)
    loss = torch.nn.functional.huber_loss(t * w, qa * w, delta=1.0)
    grads = torch.autograd.grad(loss, ps)
    return types.SimpleNamespace(target=t, loss=float(loss.detach()), priorities=(t - qa).abs().detach(), q0=q.detach(), grads=[g.detach() for g in grads])


def pick_items(online, target, D, A, n, dueling_type, discount, retrace_h, double_dqn, rescale, seed):
    """KEEP learner items on which a float32 evaluation takes float64's branches, out of POOL candidates judged by the float64 reference alone.

    Candidates: observations standard normal, rewards uniform in [-2, 2], importance weights uniform in [0.5, 2.5] / (1.5 * median |target - q_a| of the pool) -- the
    median Huber argument is then about 1 whatever the networks' scale and n, so both Huber branches stay populated; all float32 values.  One candidate in five
    ends its episode at a random step e: terminated is 1 from e on, and the steps behind e are padding (reward 0, the state repeated; rainbow.py:358-371).  The
    observations live in a pool of rows; every fourth candidate's s_0 is the previous candidate's s_1 (the ring shares rows the same way).  About GREEDY_SHARE
    of the taken actions at steps m >= 1 are the arg-max of the selecting Q row on s_{m+1} (rainbow.py:267), the others any other action.  A candidate is
    discarded when a hidden pre-activation of s_0 (the trunk's and both head branches') is within 1e-5 * max |pre-activation of that layer| of zero, when at
    ANY step the top two entries of the selecting Q row are closer than 1e-5 * max |Q|, or when |w (target - q_a)| is within 1e-4 of the Huber knee; at most
    15 % of the pool may go.  The first KEEP survivors are returned with one terminal item, one non-terminal item and one item of each Huber branch moved to
    the front, so that the first B >= 4 items see all four.

    Returns a namespace: rows [P][D] float64, idx [KEEP][n + 1] (row numbers of s_0..s_n), act int64 [KEEP][n], rew, term float64 [KEEP][n], w float64 [KEEP],
    linear bool [KEEP], chain int64 [KEEP] (the steps whose retrace coefficient is non-zero)."""
    g = torch.Generator().manual_seed(int(seed))
    rows = torch.randn((n + 1) * POOL, D, generator=g, dtype=torch.float32).double()
    idx = torch.arange((n + 1) * POOL).view(POOL, n + 1).clone()
    shared = torch.arange(1, POOL, 4)
    idx[shared, 0] = idx[shared - 1, 1]
    act = torch.randint(0, A, (POOL, n), generator=g)
    rew = (torch.rand(POOL, n, generator=g, dtype=torch.float32) * 4 - 2).double()
    ends = torch.rand(POOL, generator=g) < 0.2
    end_at = torch.randint(0, n, (POOL,), generator=g)
    term = torch.zeros(POOL, n, dtype=torch.float64)
    for j in torch.nonzero(ends).squeeze(1).tolist():
        e = int(end_at[j])
        term[j, e:] = 1.0
        rew[j, e + 1:] = 0.0
        idx[j, e + 2:] = idx[j, e + 1]
    w = (torch.rand(POOL, generator=g, dtype=torch.float32) * 2 + 0.5).double()
    take = torch.rand(POOL, n, generator=g) < GREEDY_SHARE
    other = torch.randint(1, A, (POOL, n), generator=g)
    states = rows[idx]  # [POOL][n + 1][D]
    ok = torch.ones(POOL, dtype=torch.bool)
    with torch.no_grad():
        sel_net = online if double_dqn else target
        greedy = forward(sel_net, states[:, 1:].reshape(POOL * n, D), dueling_type).view(POOL, n, A).argmax(-1)
        for m in range(1, n):
            act[:, m] = torch.where(take[:, m], greedy[:, m], (greedy[:, m] + other[:, m]) % A)
        pre = []
        q0 = forward(online, states[:, 0], dueling_type, pre)
        for z in pre:
            ok &= z.abs().min(1).values >= 1e-5 * float(z.abs().max())
        sel = []
        t = target_q(online, target, states[:, 1:], act, rew, term, discount, retrace_h, double_dqn, rescale, dueling_type, sel)
        top = sel[0].topk(2, dim=2).values
        ok &= ((top[..., 0] - top[..., 1]) >= 1e-5 * float(sel[0].abs().max())).all(1)
        err = (t - q0.gather(1, act[:, :1]).squeeze(1)).abs()
        w = (w / (1.5 * float(err.median()))).float().double()
        z = w * err
        ok &= (z - 1.0).abs() >= 1e-4
    discarded = int((~ok).sum())
    assert discarded <= POOL * 15 // 100, f"{discarded} of {POOL} candidates discarded"
    keep = torch.nonzero(ok).squeeze(1)
    assert len(keep) >= KEEP, len(keep)
    keep = keep[:KEEP]
    linear, terminal = z[keep] > 1.0, term[keep].sum(1) > 0
    assert int(linear.sum()) >= KEEP // 10 + 1 and int((~linear).sum()) >= KEEP // 10 + 1, int(linear.sum())
    assert bool(terminal.any()) and bool((~terminal).any())
    front = []
    for mask in (terminal, ~terminal, linear, ~linear):
        front.append(next(int(j) for j in torch.nonzero(mask).squeeze(1) if int(j) not in front))
    order = torch.tensor(front + [j for j in range(KEEP) if j not in front])
    keep = keep[order]
    chain = torch.ones(KEEP, dtype=torch.int64)
    if n > 1:
        hit = (act[keep][:, 1:] == greedy[keep][:, 1:]).long()
        chain = 1 + hit.cumprod(1).sum(1)
        assert bool((chain == n).any()) and bool((chain < n).any()), "both retrace branches must occur"
    return types.SimpleNamespace(rows=rows, idx=idx[keep], act=act[keep], rew=rew[keep], term=term[keep], w=w[keep], linear=(z[keep] > 1.0), chain=chain)
