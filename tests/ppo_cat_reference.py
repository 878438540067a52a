"""Host-side restatement of the discrete-action PPO arithmetic (csrc/srlx_ppo_math.h: the categorical head and the self-resetting CartPole), the yardstick of
tests/test_ppo_discrete_cpu.py and tests/test_ppo_discrete_gpu.py.  Not a test module.

The categorical head, as srlx_ppo_math.h states it:
  log-softmax, float32: m = max_k logit_k; s = sum_k exp(logit_k - m), k ascending from 0; lse = log(s); logp_k = (logit_k - m) - lse.
  sample: ONE keyed uniform per row, u = u53(rng_u64(seed, counter, row)); p_k = exp(logp_k) in float32; cum += p_k for k ascending; the action is the first k with
          cum > u (compared in float64), and n - 1 when no k qualifies.
  deterministic: the first maximum of the logits.
  the taken action's log-probability is floored at log(1e-6).
  loss seeds: lp = logp_a, g_lp = d loss / d lp of compute_train_loss at K = 1 (entropy term -exp(lp) lp of the taken action only),
          d loss / d logit_k = g_lp ((k == a) - p_k).
The reference's PPO needs TensorFlow: parity UNPINNED, as for the whole PPO row."""
import math
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import hot_path_oracle as H  # noqa: E402

LOG_FLOOR = math.log(1e-6)
ACT_KEY = 0x61637400  # the engine's action stream: seed ^ ACT_KEY
RESET_KEY = 0xCA27901E


def log_softmax32(logits):
    """[rows][n] float32, summed in ascending action order."""
    x = np.asarray(logits, np.float32)
    z = x - x.max(axis=1, keepdims=True)
    s = np.zeros(x.shape[0], np.float32)
    for k in range(x.shape[1]):
        s = (s + np.exp(z[:, k])).astype(np.float32)
    return (z - np.log(s)[:, None]).astype(np.float32)


def uniforms(seed, counter, rows):
    return H.u53(H.rng_u64(seed, np.uint64(counter), np.arange(rows, dtype=np.uint64)))


def cumulative32(logits):
    p = np.exp(log_softmax32(logits)).astype(np.float32)
    cum = np.zeros_like(p)
    run = np.zeros(p.shape[0], np.float32)
    for k in range(p.shape[1]):
        run = (run + p[:, k]).astype(np.float32)
        cum[:, k] = run
    return cum


def sample(logits, seed, counter):
    """(actions int32 [rows], u float64 [rows], cum float32 [rows][n])"""
    cum = cumulative32(logits)
    u = uniforms(seed, counter, cum.shape[0])
    above = cum.astype(np.float64) > u[:, None]
    a = np.where(above.any(axis=1), above.argmax(axis=1), cum.shape[1] - 1)
    return a.astype(np.int32), u, cum


def near_boundary(u, cum, tol=1e-6):
    """rows whose uniform lies within tol of a cumulative boundary: float32 rounding of the device's exp / log may move them to the neighbouring action"""
    return (np.abs(cum.astype(np.float64) - u[:, None]) < tol).any(axis=1)


def mode(logits):
    return np.asarray(logits).argmax(axis=1).astype(np.int32)  # numpy's argmax: the first maximum


def logp_taken(logits, actions):
    lp = log_softmax32(logits)[np.arange(len(actions)), actions]
    return np.maximum(lp, np.float32(LOG_FLOOR))


def losses_and_seeds64(logits, actions, old_lp, adv, v, vt, ov, base, clip, pc, vclip, vc, vw, ew):
    """compute_train_loss (ppo.py:102-169) with a categorical head in float64, closed form: ((policy, value, entropy), d loss / d logits [B][n], d loss / d v [B])."""
    d = np.float64
    x, a = np.asarray(logits, d), np.asarray(actions)
    old_lp, adv, v, vt, ov = (np.asarray(t, d) for t in (old_lp, adv, v, vt, ov))
    B = x.shape[0]
    z = x - x.max(axis=1, keepdims=True)
    logp = z - np.log(np.exp(z).sum(axis=1, keepdims=True))
    p = np.exp(logp)
    lp = logp[np.arange(B), a]
    ad = adv - v if base else adv
    ratio = np.exp(lp - old_lp)
    if clip:
        lu, lc = ratio * ad, np.clip(ratio, 1 - pc, 1 + pc) * ad
        term, g_ratio = np.minimum(lu, lc), np.where(lu <= lc, ad, 0.0)
    else:
        term, g_ratio = ratio * ad, ad
    elp = np.exp(lp)
    ent = -elp * lp
    g_lp = -g_ratio * ratio / B + ew * (elp * lp + elp) / B
    onehot = np.zeros_like(x)
    onehot[np.arange(B), a] = 1.0
    d_logits = g_lp[:, None] * (onehot - p)
    e1 = v - vt
    if vclip:
        e2 = np.clip(v, ov - vc, ov + vc) - vt
        l1, l2 = e1 * e1, e2 * e2
        s = np.maximum(l1, l2)
        inside = (v >= ov - vc) & (v <= ov + vc)
        g = np.where(l1 >= l2, 2 * e1, np.where(inside, 2 * e2, 0.0))
    else:
        s, g = e1 * e1, 2 * e1
    d_v = vw * g / B
    return (-term.mean(), vw * s.mean(), ew * -ent.mean()), d_logits, d_v


def torch_loss(torch, logits, actions, old_lp, adv, v, vt, ov, base, clip, pc, vclip, vc, vw, ew):
    """The same loss as a torch graph through log_softmax: (policy, value, entropy) tensors."""
    lp = torch.log_softmax(logits, dim=-1).gather(1, actions.long().view(-1, 1)).squeeze(1)
    ad = adv - v.detach() if base else adv
    ratio = torch.exp(lp - old_lp)
    pol = torch.minimum(ratio * ad, torch.clamp(ratio, 1 - pc, 1 + pc) * ad) if clip else ratio * ad
    if vclip:
        v_c = torch.maximum(torch.minimum(v, ov + vc), ov - vc)
        value = torch.maximum((v - vt) ** 2, (v_c - vt) ** 2)
    else:
        value = (v - vt) ** 2
    return -pol.mean(), vw * value.mean(), ew * -(-(torch.exp(lp) * lp)).mean()


class HostCartPoleAuto:
    """E host environments (envs/cartpole.py) that start their next episode in the step that ends one, with the device's reset key."""

    def __init__(self, state, steps, episodes, max_steps, seed):
        from simple_distributed_rl_amd.envs.cartpole import CartPole

        self.envs = []
        for s, t in zip(np.asarray(state, np.float64), steps):
            e = CartPole(max_steps=max_steps)
            e.state, e.steps = s.copy(), int(t)
            self.envs.append(e)
        self.episodes, self.seed = np.asarray(episodes, np.int64).copy(), seed

    def reset_state(self, lane, episode):
        key = np.uint64((lane << 32) | (episode & 0xFFFFFFFF))
        return -0.05 + 0.1 * H.u53(H.rng_u64(self.seed ^ RESET_KEY, key, np.arange(4, dtype=np.uint64)))

    def step(self, actions):
        """-> (stepped state [E][4] BEFORE any reset, state after, terminated, truncated)"""
        E = len(self.envs)
        stepped, after, term, trunc = np.zeros((E, 4)), np.zeros((E, 4)), np.zeros(E, bool), np.zeros(E, bool)
        for i, e in enumerate(self.envs):
            _, _, te, tr = e.step(int(actions[i]))
            stepped[i], term[i], trunc[i] = e.state, te, tr
            if te or tr:
                e.state, e.steps = self.reset_state(i, int(self.episodes[i])), 0
                self.episodes[i] += 1
            after[i] = e.state
        return stepped, after, term, trunc
