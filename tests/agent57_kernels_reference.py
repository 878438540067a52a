"""Yardsticks of tests/test_agent57_kernels_gpu.py (and their own hand-worked check, tests/test_agent57_kernels_cpu.py), written as a different program from
csrc/srlx_agent57.hip and the two Agent57 kernels of csrc/srlx_ngu.hip:
  * the pointwise kernels (policy, post_step, begin_episodes, gather_inputs, pack_record, unpack_fields, priority) as whole-array float32 numpy -- bit-exact:
    the library is built with -ffp-contract=off, so `q_ext + beta * q_int` is one float32 multiply and one float32 add there as here; the keyed generator is
    rng_u64 / u53 of oracle/hot_path_oracle.py with the keys the kernels use;
  * the two learner tails as torch modules' functional forms on the CPU, float64 with autograd (the yardstick) and float32 (what float32 arithmetic costs on the
    same inputs), with the project's standing tolerance (tests/lstm_reference.py:check_tensor);
  * the UCB bank as E of the plugin's UcbMetaController (pinned to the reference's trace in tests/test_agent57_cpu.py), fed the kernel's uniforms."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
from hot_path_oracle import rng_u64, u53  # noqa: E402

F32, I32, U8 = np.float32, np.int32, np.uint8
FIELDS = 5                    # the item fields behind the frame store's 10 bytes per environment
RECORD_BYTES_PER_ENV = 10 + 4 * FIELDS


# ---- actors ----------------------------------------------------------------------------------------------------------------------------------------------------
def policy(q_ext, q_int, arm, beta_list, eps_list, test_beta, test_eps, seed, counter):
    """-> actions int32 [E], q float32 [E][A], took_random bool [E].  arm None: evaluation (test_beta / test_eps for every lane)."""
    E, A = q_ext.shape
    if arm is None:
        beta, eps = np.full(E, F32(test_beta)), np.full(E, F32(test_eps))
    else:
        beta, eps = beta_list.astype(F32)[arm], eps_list.astype(F32)[arm]
    prod = (beta[:, None] * q_int.astype(F32)).astype(F32)
    q = (q_ext.astype(F32) + prod).astype(F32)
    greedy = np.argmax(q, axis=1)  # the first maximum
    lane = np.arange(E, dtype=np.uint64)
    took_random = u53(rng_u64(seed, counter, np.uint64(2) * lane)) < eps.astype(np.float64)
    pick = np.minimum((u53(rng_u64(seed, counter, np.uint64(2) * lane + np.uint64(1))) * float(A)).astype(np.int64), A - 1)
    return np.where(took_random, pick, greedy).astype(I32), q, took_random


def post_step(s, actions, arm, rewards, reset_lane, episodic, lifelong):
    """s: dict of the four per-lane arrays (prev_action, prev_r_ext, prev_r_int, episode_reward).  -> (new s, x) with x the five item-field rows."""
    live = reset_lane == 0
    r_int = np.zeros(len(actions), F32)
    if episodic is not None:
        r_int = np.where(live, (episodic.astype(F32) * lifelong.astype(F32)).astype(F32), F32(0)).astype(F32)
    x = dict(x_r_int=r_int, x_prev_r_ext=s["prev_r_ext"].copy(), x_prev_r_int=s["prev_r_int"].copy(), x_actor=arm.astype(I32).copy(),
             x_prev_action=s["prev_action"].copy())
    new = dict(prev_action=np.where(live, actions, s["prev_action"]).astype(I32), prev_r_ext=np.where(live, rewards, s["prev_r_ext"]).astype(F32),
               prev_r_int=np.where(live, r_int, s["prev_r_int"]).astype(F32),
               episode_reward=np.where(live, (s["episode_reward"] + rewards.astype(F32)).astype(F32), s["episode_reward"]).astype(F32))
    return new, x


def begin_episodes(s, n_actions, done, seed, counter):
    """-> (new s, reset_lane uint8, live_lane uint8); done None: every lane begins an episode."""
    E = len(s["prev_action"])
    d = np.ones(E, bool) if done is None else done.astype(bool)
    first = np.minimum((u53(rng_u64(seed, counter, np.arange(E, dtype=np.uint64))) * float(n_actions)).astype(np.int64), n_actions - 1).astype(I32)
    new = dict(prev_action=np.where(d, first, s["prev_action"]).astype(I32))
    for k in ("prev_r_ext", "prev_r_int", "episode_reward"):
        new[k] = np.where(d, F32(0), s[k]).astype(F32)
    reset = np.zeros(E, U8) if done is None else d.astype(U8)
    live = np.ones(E, U8) if done is None else (~d).astype(U8)
    return new, reset, live


def gather_inputs(loc_env, loc_slot, actions, rewards, x, discount_list):
    """x: dict of the five [L][E] item-field arrays.  -> dict of the ten outputs (online rows interleaved: 2 b = what the actor saw, 2 b + 1 = one step later)."""
    at = (loc_slot, loc_env)
    B = len(loc_env)
    actor, ri = x["x_actor"][at], x["x_r_int"][at]
    o = dict(on_r_ext=np.empty(2 * B, F32), on_r_int=np.empty(2 * B, F32), on_action=np.empty(2 * B, I32), on_actor=np.empty(2 * B, I32))
    o["on_r_ext"][0::2], o["on_r_ext"][1::2] = x["x_prev_r_ext"][at], rewards
    o["on_r_int"][0::2], o["on_r_int"][1::2] = x["x_prev_r_int"][at], ri
    o["on_action"][0::2], o["on_action"][1::2] = x["x_prev_action"][at], actions
    o["on_actor"][0::2], o["on_actor"][1::2] = actor, actor
    o.update(tg_r_ext=rewards.astype(F32).copy(), tg_r_int=ri.copy(), tg_action=actions.astype(I32).copy(), tg_actor=actor.copy(),
             discount=discount_list.astype(F32)[actor], r_int=ri.copy())
    return o


def pack_record(actions, rewards, terminated, done, x):
    """One lock-step of E lanes as 30 E bytes: int32 actions, float32 rewards, E terminated bytes, E done bytes, then per lane five float32 (intrinsic reward,
    arm, previous action, previous extrinsic reward, previous intrinsic reward)."""
    f = np.stack([x["x_r_int"].astype(F32), x["x_actor"].astype(F32), x["x_prev_action"].astype(F32), x["x_prev_r_ext"].astype(F32), x["x_prev_r_int"].astype(F32)], axis=1)
    return np.concatenate([actions.astype("<i4").view(U8), rewards.astype("<f4").view(U8), terminated.astype(U8), done.astype(U8), np.ascontiguousarray(f).astype("<f4").view(U8).reshape(-1)])


def unpack_fields(records, n_records, per, stride, position, ring):
    """records: uint8 [>= n_records * stride]; ring: dict of the five [L][n_records * per] arrays, changed in place in row position mod L."""
    L = ring["x_r_int"].shape[0]
    slot = position % L  # (Python's remainder is never negative)
    for r in range(n_records):
        f = records[r * stride + 10 * per: r * stride + 30 * per].copy().view("<f4").reshape(per, FIELDS)
        cols = slice(r * per, (r + 1) * per)
        ring["x_r_int"][slot, cols] = f[:, 0]
        ring["x_actor"][slot, cols] = f[:, 1].astype(I32)
        ring["x_prev_action"][slot, cols] = f[:, 2].astype(I32)
        ring["x_prev_r_ext"][slot, cols] = f[:, 3]
        ring["x_prev_r_int"][slot, cols] = f[:, 4]
    return slot


def priority(target_ext, q_ext, target_int, q_int, actions, actor_idx, beta_list):
    """-> td_ext, td_int (None without intrinsic inputs), priorities; q_* None: target_* already hold the TD errors."""
    rows = np.arange(len(target_ext))
    te = target_ext.astype(F32) if q_ext is None else (target_ext.astype(F32) - q_ext.astype(F32)[rows, actions]).astype(F32)
    if target_int is None:
        return te, None, np.abs(te)
    ti = target_int.astype(F32) if q_int is None else (target_int.astype(F32) - q_int.astype(F32)[rows, actions]).astype(F32)
    mixed = (te + (beta_list.astype(F32)[actor_idx] * ti).astype(F32)).astype(F32)
    return te, ti, np.abs(mixed)


# ---- the learner's two tails: torch on the CPU -----------------------------------------------------------------------------------------------------------------
LN_EPS = 1e-5
EMB_NAMES = ("w1", "b1", "ln_w", "ln_b", "w2", "b2")


def _emb_tail_torch(torch, emb, actions, params, A):
    w1, b1, lw, lb, w2, b2 = params
    x = torch.cat([emb[0::2], emb[1::2]], dim=1)
    h = torch.relu(x @ w1.t() + b1)
    y = torch.nn.functional.layer_norm(h, (h.shape[1],), lw, lb, 1e-5)
    p = torch.softmax(y @ w2.t() + b2, dim=1)
    return torch.nn.functional.mse_loss(p, torch.eye(A, dtype=p.dtype)[actions.long()])


def emb_case(B, D, Hd, A, seed, zero_actions=False):
    """float32 CPU inputs of the embedding tail (the recipe of tests/test_agent57_fast_gpu.py at any shape)."""
    import torch

    g = torch.Generator().manual_seed(seed)
    emb = torch.relu(torch.randn((2 * B, D), generator=g))
    actions = torch.zeros(B, dtype=torch.int64) if zero_actions else torch.randint(0, A, (B,), generator=g)
    params = [torch.randn((Hd, 2 * D), generator=g) * 0.2, torch.randn(Hd, generator=g) * 0.1, 1 + 0.1 * torch.randn(Hd, generator=g), 0.1 * torch.randn(Hd, generator=g),
              torch.randn((A, Hd), generator=g) * 0.2, torch.randn(A, generator=g) * 0.1]
    return dict(B=B, D=D, Hd=Hd, A=A, emb=emb, actions=actions, params=params)


def emb_reference(c, dtype):
    """loss, d_emb, the six gradients (autograd in `dtype`) and the pre-activations of the hidden layer."""
    import torch

    e = c["emb"].detach().clone().to(dtype).requires_grad_(True)
    p = [t.detach().clone().to(dtype).requires_grad_(True) for t in c["params"]]
    loss = _emb_tail_torch(torch, e, c["actions"], p, c["A"])
    loss.backward()
    with torch.no_grad():
        pre = torch.cat([e[0::2], e[1::2]], dim=1) @ p[0].t() + p[1]
    return dict(loss=loss.detach(), d_emb=e.grad, grads=[t.grad for t in p], pre=pre)


def rnd_case(B, D, seed):
    import torch

    g = torch.Generator().manual_seed(seed)
    return dict(B=B, D=D, h=torch.relu(torch.randn((B, D), generator=g)), target=torch.randn((B, D), generator=g), ln_w=1 + 0.1 * torch.randn(D, generator=g),
                ln_b=0.1 * torch.randn(D, generator=g))


def rnd_reference(c, dtype):
    import torch

    h, w, b = (c[k].detach().clone().to(dtype).requires_grad_(True) for k in ("h", "ln_w", "ln_b"))
    loss = torch.nn.functional.mse_loss(c["target"].to(dtype), torch.nn.functional.layer_norm(h, (c["D"],), w, b, LN_EPS))
    loss.backward()
    return dict(loss=loss.detach(), d_h=h.grad, g_w=w.grad, g_b=b.grad)


def check_tensor(name, got, want64, ref32, where):
    """The project's standing tolerance (tests/lstm_reference.py:check_tensor): rtol 1e-5, atol 1e-5 of the tensor's largest entry, against float64; failing
    that, a tensor may be as far from float64 as twice the float32 CPU evaluation of the same function on the same inputs is -- measured from torch, never from
    the kernel, and printed."""
    import torch

    got = torch.as_tensor(got).detach().double().cpu().reshape(want64.shape)
    atol = 1e-5 * float(want64.abs().max()) if want64.numel() else 0.0
    try:
        torch.testing.assert_close(got, want64, rtol=1e-5, atol=atol)
        return
    except AssertionError as e:
        err = float((got - want64).abs().max())
        cpu32 = float((ref32.double() - want64).abs().max())
        print("A57-ESCAPE %s %s: |kernel - f64| %.3g beyond rtol 1e-5 / atol %.3g; float32 torch on the CPU is %.3g from f64; allowed %.3g" % (
            where, name, err, atol, cpu32, 2 * cpu32))
        assert err <= 2 * cpu32, f"{where} {name}: {e}"


def check_loss(got, want64, where):
    want = float(want64)
    assert abs(float(got) - want) <= 1e-5 * abs(want), f"{where} loss: {float(got)!r} against {want!r}"


# ---- the UCB bank on the host ----------------------------------------------------------------------------------------------------------------------------------
class UcbFeed:
    """The draws the kernel makes, handed to UcbMetaController through a patched `random`: random() < eps -> u0 ; randint -> floor(u1 * N)."""

    def __init__(self):
        self.u = None

    def random(self):
        return float(self.u[0])

    def randint(self, a, b):
        return min(int(self.u[1] * (b - a + 1)) + a, b)


def ucb_tie_break(u):
    def tie(vals, _u=u):
        best = max(vals)
        idx = [i for i, v in enumerate(vals) if v == best]
        return idx[min(int(_u[2] * len(idx)), len(idx) - 1)]

    return tie


class HostUcbBank:
    """E host controllers; step(done, last_reward, u) advances those whose episode ended (done None: all) on the uniforms u [E][3] and returns every arm."""

    def __init__(self, n_envs, n_arms, window, epsilon, beta):
        from simple_distributed_rl_amd.algorithms.agent57_light import UcbMetaController

        self.feeds = [UcbFeed() for _ in range(n_envs)]
        self.hosts = [UcbMetaController(n_arms, window, epsilon, beta, tie_break=None) for _ in range(n_envs)]

    def step(self, done, last, u):
        import simple_distributed_rl_amd.algorithms.agent57_light as mod

        saved = mod.random
        try:
            for e, host in enumerate(self.hosts):
                if done is not None and not done[e]:
                    continue
                self.feeds[e].u = u[e]
                mod.random = self.feeds[e]
                host.tie_break = ucb_tie_break(u[e])
                host.next_actor(float(last[e]))
        finally:
            mod.random = saved
        return np.array([h.actor_index for h in self.hosts])
