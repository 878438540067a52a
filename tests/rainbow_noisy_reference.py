"""A float64 yardstick for Rainbow's learner step with NoisyLinear layers on flat observations (libsrlx srlx_mlpq_bind_noisy / srlx_mlpq_train_nstep on noisy
handles): tests/rainbow_vec_reference.py's forward pass, n-step target and Adam on THREE effective parameter sets -- the online network under the s_0 draw (the
pass with the gradient), the online network under the s_1..s_n draw, the target network under its own draw (rainbow.py:224-225, model_torch.py:103) -- with the
mu / sigma gradients by autograd through mu + sigma * eps of the s_0 draw.  tests/test_rainbow_noisy_vector_cpu.py pins it on the reference's recorded
Trainer.train() (tests/golden/train_step_rainbow_noisy_vec.npz) before any kernel is judged by it.

Parameter lists are in EngineMLPQNet.kernel_parameters() order; a sigma / eps list has the same length with None for the tensors of a plain layer."""
import os
import sys
import types

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)
import rainbow_noisy_recipe as NC  # noqa: E402
import rainbow_vec_reference as R  # noqa: E402

forward, target_q, adam_steps = R.forward, R.target_q, R.adam_steps
POOL, KEEP, GREEDY_SHARE = R.POOL, R.KEEP, R.GREEDY_SHARE

# (D, in_sizes (plain layers), hidden_sizes (noisy layers), H, A, dueling_type, n): the shapes the GPU tests run (tests/test_rainbow_noisy_vector_gpu.py)
ENVELOPE = [
    (1, (), (), 32, 2, "average", 1),        # every lower bound; the noisy head on the raw observation; a one-element bias
    (4, (), (), 512, 2, "average", 3),       # rainbow.Config()
    (256, (), (512, 512), 512, 32, "", 7),   # every upper bound; 12 mu + 12 sigma tensors
    (3, (), (64,), 96, 3, "average", 2),     # odd A: a Box-Muller pair's unused half
    (17, (96,), (32,), 480, 5, "", 4),       # a plain layer in front of a noisy one
    (8, (), (32,), 64, 4, "average", 5),     # two items per workgroup
]


def init_params(D, in_sizes, hidden_sizes, units, A, seed):
    """(mu, sigma): mu as rainbow_vec_reference.init_params draws it; sigma the reference's initial 0.5 / sqrt(in) (noisy_linear.py:26-33), None for the
    `in_sizes` layers' tensors."""
    trunk = tuple(in_sizes) + tuple(hidden_sizes)
    mu = R.init_params(D, trunk, units, A, seed)
    sigma = []
    for l in range(len(mu) // 2):
        if l < len(in_sizes):
            sigma += [None, None]
        else:
            s = 0.5 / float(np.sqrt(mu[2 * l].shape[1]))
            sigma += [torch.full_like(mu[2 * l], s), torch.full_like(mu[2 * l + 1], s)]
    return mu, sigma


def effective(mu, sigma, eps):
    """W = w_mu + w_sigma * eps_w, b = b_mu + b_sigma * eps_b (noisy_linear.py:50-51); plain tensors pass through."""
    return [m if s is None else m + s * e.double() for m, s, e in zip(mu, sigma, eps)]


def learner_step(mu, sigma, eps0, eff_next, eff_target, states, act, rew, term, w, discount, retrace_h, double_dqn, rescale, dueling_type):
    """rainbow.py:185-287 + model_torch.py:85-122 in float64 autograd with the three draws of one Trainer.train(): the target from `eff_next` (online network,
    s_1..s_n) and `eff_target`; the loss through mu + sigma * eps0 on s_0.  Returns a namespace: target [B], loss, priorities [B], q0 [B][A], grads (d loss / d mu
    per tensor) and sigma_grads (d loss / d sigma; None for plain tensors)."""
    t = target_q(eff_next, eff_target, states[:, 1:], act, rew, term, discount, retrace_h, double_dqn, rescale, dueling_type)
    mus = [p.detach().clone().requires_grad_(True) for p in mu]
    sigs = [None if s is None else s.detach().clone().requires_grad_(True) for s in sigma]
    q = forward(effective(mus, sigs, eps0), states[:, 0], dueling_type)
    qa = q.gather(1, act[:, :1].long()).squeeze(1)
    loss = torch.nn.functional.huber_loss(t * w, qa * w, delta=1.0)
    live = [s for s in sigs if s is not None]
    grads = torch.autograd.grad(loss, mus + live)
    gs = iter(grads[len(mus):])
    return types.SimpleNamespace(target=t, loss=float(loss.detach()), priorities=(t - qa).abs().detach(), q0=q.detach(), grads=[g.detach() for g in grads[:len(mus)]],
                                 sigma_grads=[None if s is None else next(gs).detach() for s in sigs])


def golden_inputs(name):
    """The float64 mu / sigma lists of both networks and the items of one recorded case: (case, mu keys, sigma keys, (mu, sigma) online, (mu, sigma) target,
    items)."""
    case = NC.CASES[name]
    mk, sk = NC.mu_keys(case), NC.sigma_keys(case)
    nets = []
    for seed in (NC.SEED_ONLINE, NC.SEED_TARGET):
        sd = NC.recipe_state_dict(case, seed)
        nets.append(([torch.tensor(sd[k]).double() for k in mk], [None if k is None else torch.tensor(sd[k]).double() for k in sk]))
    states, actions, rewards, terminated, weights = (torch.tensor(a) for a in NC.make_items(case))
    return case, mk, sk, nets[0], nets[1], types.SimpleNamespace(states=states, act=actions, rew=rewards, term=terminated, w=weights)


def pick_items(on0, on_next, tg, D, A, n, dueling_type, discount, retrace_h, double_dqn, rescale, seed):
    """rainbow_vec_reference.pick_items over the three effective sets of one update: the same candidates, criteria and cap (at most 15 % of the POOL = 400
    candidates discarded), with the hidden pre-activations of s_0 and q_a judged on `on0` (the s_0 draw) and the arg-max gaps of every step judged on the
    selecting next-state set (`on_next` under double DQN, `tg` otherwise).  Returns the same namespace."""
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
    states = rows[idx]
    ok = torch.ones(POOL, dtype=torch.bool)
    with torch.no_grad():
        sel_net = on_next if double_dqn else tg
        greedy = forward(sel_net, states[:, 1:].reshape(POOL * n, D), dueling_type).view(POOL, n, A).argmax(-1)
        for m in range(1, n):
            act[:, m] = torch.where(take[:, m], greedy[:, m], (greedy[:, m] + other[:, m]) % A)
        pre = []
        q0 = forward(on0, states[:, 0], dueling_type, pre)
        for z in pre:
            ok &= z.abs().min(1).values >= 1e-5 * float(z.abs().max())
        sel = []
        t = target_q(on_next, tg, states[:, 1:], act, rew, term, discount, retrace_h, double_dqn, rescale, dueling_type, sel)
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
