"""The bits of everything the row-blocked MLP passes (csrc/srlx_mlp_rows.h) and the update tail behind them (csrc/srlx_param_tail.h) produce, for comparing two
BUILDS of libsrlx on one box:

    SRLX_LIB=/path/to/another/libsrlx.so python tools/mlp_rows_bits.py --out a.json     # one process per build: the library is chosen at import
    python tools/mlp_rows_bits.py --out b.json                                          # the in-tree build
    python tools/mlp_rows_bits.py --compare a.json b.json --out profiles/NAME.json      # both outputs, one digest per case, and the keys that differ; exit status 1 if any does

Every case drives libsrlx's entry points (through the zero-copy handles of device/mlpq.py, sacd.py, vppo.py and notsac.py) on seeded inputs and records the
SHA-256 of every output array and, after an update, of every parameter, gradient and Adam tensor (V-PPO and NoT_SAC: one digest over each list of tensors, in
bind order).  The library is built with -ffp-contract=off and every product-sum is an explicit fma in a fixed order, so a change that only moves code must leave
every digest as it was.  The shapes are the smallest at which the shared code takes each of its paths (one tile / many tiles with a partial last one; 1, 8 and
128 row groups; idle threads; chains of 0, 1 and 2 steps; a full and a one-item workgroup; B 16 / 17, both heads, a clip that bites and one that does not)."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

DISCOUNT, RETRACE_H, LR = 0.99, 0.9, 1e-3


def digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def digest_all(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def record(out, case, **tensors):
    for k, v in tensors.items():
        for j, t in enumerate(v if isinstance(v, (list, tuple)) else [v]):
            out[f"{case}/{k}" + (f"[{j}]" if isinstance(v, (list, tuple)) else "")] = digest(t)


def mlpq_pair(net_kw, B, seed, max_nstep=7, draws=None):
    """A seeded online net with its training handle and a target net with its acting handle."""
    from simple_distributed_rl_amd.device.mlpq import EngineMLPQNet, MLPQHandle

    torch.manual_seed(seed)
    net, tgt = EngineMLPQNet(**net_kw).cuda(), EngineMLPQNet(**net_kw).cuda()
    h = MLPQHandle(net, 64, max_batch=B, lr=LR, max_nstep=max_nstep, noise_seed=seed)
    ht = MLPQHandle(tgt, 64, max_nstep=max_nstep, noise_seed=seed + 1)
    if draws:  # NoisyLinear: both builds consume the same draw ids
        h.set_next_draw(draws[0])
        ht.set_next_draw(draws[1])
    return net, h, ht


def items(B, n, D, A, seed):
    """B items of n steps on rows of their own: obs [(n + 1) B][D], offsets [B][n + 1], actions / rewards / terminated [B][n], weights [B]."""
    g = torch.Generator().manual_seed(seed)
    obs = torch.randn((n + 1) * B, D, generator=g)
    off = (torch.randperm((n + 1) * B, generator=g).view(B, n + 1) * D).to(torch.int64)
    act = torch.randint(0, A, (B, n), generator=g).int()
    rew = torch.randn(B, n, generator=g)
    term = (torch.rand(B, n, generator=g) < 0.2).float()
    w = torch.rand(B, generator=g) + 0.5
    return [t.cuda() for t in (obs, off, act, rew, term, w)]


def trained(net, h):
    sig = [t for t in h.sigmas if t is not None]
    state = dict(params=h.params, grads=[p.grad for p in h.params], exp_avg=h.exp_avg, exp_avg_sq=h.exp_avg_sq)
    if sig:
        state.update(sigmas=sig, sigma_grads=[t.grad for t in sig], sigma_exp_avg=[t for t in h.exp_avg_sigma if t is not None],
                     sigma_exp_avg_sq=[t for t in h.exp_avg_sq_sigma if t is not None])
    return state


def mlpq_td(out, case, net_kw, B, n, entry, seed, max_nstep=7, draws=None):
    """srlx_mlpq_train_step (entry "step", n = 1) or srlx_mlpq_train_nstep with Adam bound: the outputs and everything the update wrote."""
    D, A = net_kw["obs_dim"], net_kw["n_actions"]
    net, h, ht = mlpq_pair(net_kw, B, seed, max_nstep, draws)
    obs, off, act, rew, term, w = items(B, n, D, A, seed + 2)
    steps = torch.zeros(1, dtype=torch.int64, device="cuda")
    q0, target, loss, pri = (torch.zeros(s, device="cuda") for s in ((B, A), (B,), (1,), (B,)))
    if entry == "step":
        h.train_step(ht, B, obs.data_ptr(), off, act, rew, term, w, DISCOUNT, True, False, steps, q0, target, loss, pri)
    else:
        h.train_nstep(ht, B, n, obs.data_ptr(), off, act, rew, term, w, DISCOUNT, RETRACE_H, True, False, steps, q0, target, loss, pri)
    torch.cuda.synchronize()
    record(out, case, q0=q0, target=target, loss=loss, priorities=pri, **trained(net, h))


def mlpq_forward(out, case, net_kw, rows, seed):
    """srlx_mlpq_forward: Q rows and the epsilon-greedy actions, dense rows and rows through an offset table."""
    D, A = net_kw["obs_dim"], net_kw["n_actions"]
    _, _, ht = mlpq_pair(net_kw, 0, seed)
    g = torch.Generator().manual_seed(seed + 3)
    x = torch.randn(rows, D, generator=g).cuda()
    eps = torch.rand(rows, generator=g).cuda()
    perm = (torch.randperm(rows, generator=g) * D).to(torch.int64).cuda()
    counter = torch.full((1,), 5, dtype=torch.int64, device="cuda")
    for name, offsets in (("dense", None), ("table", perm)):
        q, actions = torch.zeros(rows, A, device="cuda"), torch.zeros(rows, dtype=torch.int32, device="cuda")
        ht.forward(rows, x.data_ptr(), offsets=offsets, q=q, eps=eps, seed=seed, counter=counter, actions=actions)
        torch.cuda.synchronize()
        record(out, f"{case}/{name}", q=q, actions=actions)


def mlpq_categorical(out, case, D, widths, A, atoms, B, seed):
    """srlx_mlpq_train_categorical with Adam bound."""
    from simple_distributed_rl_amd.device.mlpq import EngineMLPQNet, MLPQHandle

    torch.manual_seed(seed)
    net = EngineMLPQNet(D, (), widths, A, n_atoms=atoms).cuda()
    h = MLPQHandle(net, 64, max_batch=B, lr=LR)
    obs, off, act, rew, term, _ = items(B, 1, D, A, seed + 2)
    steps = torch.zeros(1, dtype=torch.int64, device="cuda")
    q0, p0, m, loss, item_loss = (torch.zeros(s, device="cuda") for s in ((B, A), (B, atoms), (B, atoms), (1,), (B,)))
    h.train_categorical(B, obs.data_ptr(), off, act.view(B), rew.view(B), term.view(B), DISCOUNT, steps, q0, p0, m, loss, item_loss)
    torch.cuda.synchronize()
    record(out, case, q0=q0, p0=p0, m=m, loss=loss, item_loss=item_loss, **trained(net, h))


def sacd(out, i):
    """Row i of tests/sacd_cases.py:SHAPES: srlx_sacd_forward for both targets, srlx_sacd_act with and without the offset table on both sides of
    random_until, then srlx_sacd_update (a hard sync, then a soft one)."""
    import sacd_cases as C
    from simple_distributed_rl_amd.device.sacd import NETWORKS, TRAINED, SacdUpdate

    B, D, A, pw, qw = C.SHAPES[i]
    case = "sacd/" + C.shape_id(i)
    cfg = C.make_config(D, A, pw, qw, device="cuda", lr_policy=C.LR, lr_q=C.LR, lr_alpha=C.LR, discount=C.DISCOUNT, soft_target_update_tau=C.TAU)
    p = C.make_parameter(cfg, 1000 + i)
    u = SacdUpdate(p, max_batch=B)
    b = C.make_batch(B, D, A, 3000 + i)
    state, n_state = b["state"].float().cuda(), b["n_state"].float().cuda()
    for target in (False, True):
        logits, qmin = u.forward(state, target=target)
        torch.cuda.synchronize()
        record(out, f"{case}/forward/target{int(target)}", logits=logits, qmin=qmin)
    perm = (torch.randperm(B, generator=torch.Generator().manual_seed(i)) * D).to(torch.int64).cuda()
    counter = torch.full((1,), 5, dtype=torch.int64, device="cuda")
    for name, offsets in (("dense", None), ("table", perm)):
        for random_until in (5, 6):  # the counter is 5: the policy's action, then the uniform one
            actions = torch.zeros(B, dtype=torch.int32, device="cuda")
            logits, scores = torch.zeros(B, A, device="cuda"), torch.zeros(B, A, dtype=torch.float64, device="cuda")
            u.act(B, state, offsets, 0x5ACD + i, counter, random_until, actions, logits=logits, scores=scores)
            torch.cuda.synchronize()
            record(out, f"{case}/act/{name}/until{random_until}", actions=actions, logits=logits, scores=scores)
    for k, hard in enumerate((True, False)):
        res = u.update(state, b["action"].int().cuda(), n_state, b["reward"].float().cuda(), b["done"].to(torch.uint8).cuda(), C.LR, C.LR, C.LR, hard, C.DISCOUNT,
                       C.TAU, True, -A)
        torch.cuda.synchronize()
        record(out, f"{case}/update{k}", log_alpha=p.log_alpha, grad_log_alpha=u.grad_log_alpha, alpha_exp_avg=u.alpha_exp_avg,
               alpha_exp_avg_sq=u.alpha_exp_avg_sq, **res, **{"params_" + n: u.params[n] for n in NETWORKS}, **{"grads_" + n: u.grads[n] for n in TRAINED},
               **{"exp_avg_" + n: u.exp_avg[n] for n in TRAINED}, **{"exp_avg_sq_" + n: u.exp_avg_sq[n] for n in TRAINED})


def record_update(out, case, res, u):
    """What an update returned, and one digest over each of the handle's tensor lists."""
    record(out, case, **res)
    for kind in ("raw_grads", "grads", "params", "exp_avg", "exp_avg_sq"):
        out[f"{case}/{kind}"] = digest_all(getattr(u, kind))


def vppo(out, name):
    """A case of tests/vppo_cases.py: two srlx_vppo_update, srlx_vppo_forward of the last batch, then srlx_vppo_act or srlx_vppo_act_normal of 17 rows."""
    import vppo_cases as C
    from simple_distributed_rl_amd.device.vppo import VppoUpdate

    B, D, head = C.CASES[name][:3]
    case = "vppo/" + name
    p = C.make_parameter(name, "cuda")
    cfg = p.config
    u = VppoUpdate(p, max_batch=B)
    f = lambda x: x.float().cuda()  # noqa: E731
    for k, b in enumerate(C.make_batches(name)):
        res = u.update(f(b["state"]), f(b["n_state"]), f(b["action"]) if head else b["action"].int().cuda(), f(b["old_logpi"]), f(b["reward"]),
                       f(b["not_terminated"]), f(b["total_reward"]), cfg.lr, cfg.discount, cfg.clip_range, cfg.entropy_weight, cfg.loss_align_coeff,
                       cfg.max_grad_norm, cfg.squashed_gaussian_policy)
        torch.cuda.synchronize()
        record_update(out, f"{case}/update{k}", res, u)
    v, heads = u.forward(f(b["state"]))
    torch.cuda.synchronize()
    record(out, case + "/forward", v=v, head=heads)
    n, K = 17, u.n_out
    x = torch.randn(n, D, generator=torch.Generator().manual_seed(17)).cuda()
    counter = torch.full((1,), 5, dtype=torch.int64, device="cuda")
    z32 = lambda *shape: torch.zeros(shape, device="cuda")  # noqa: E731
    if head:
        low, high = torch.full((K,), -2.0, device="cuda"), torch.full((K,), 2.0, device="cuda")
        got = dict(actions=z32(n, K), logp=z32(n, K), env_actions=z32(n, K), loc=z32(n, K), log_scale=z32(n, K), z=torch.zeros(n, K, dtype=torch.float64, device="cuda"))
        u.act_normal(n, x, 0x5EED, counter, 0.25, 0.5, cfg.squashed_gaussian_policy, low, high, **got)
    else:
        got = dict(actions=torch.zeros(n, dtype=torch.int32, device="cuda"), logp=z32(n), logits=z32(n, K), cdf=torch.zeros(n, K, dtype=torch.float64, device="cuda"))
        u.act(n, x, 0x5EED, counter, 0.25, **got)
    torch.cuda.synchronize()
    record(out, case + "/act", **got)


def notsac(out, name):
    """A case of tests/notsac_cases.py: two srlx_notsac_update on a fresh Parameter at the default launch shape and at 16 rows per workgroup, then
    srlx_notsac_forward of the last batch with and without actions."""
    import notsac_cases as C
    from simple_distributed_rl_amd.device.notsac import NotSacUpdate

    B, _, head = C.CASES[name][:3]
    case = "notsac/" + name
    f = lambda x: x.float().cuda()  # noqa: E731
    for rpw in (0, 16):
        p = C.make_parameter(name, "cuda")
        cfg = p.config
        u = NotSacUpdate(p, max_batch=B)
        u.set_rows_per_workgroup(rpw)
        for k, b in enumerate(C.make_batches(name)):
            res = u.update(f(b["state"]), f(b["n_state"]), f(b["action"]) if head else b["action"].argmax(1).int().cuda(), f(b["reward"]), f(b["not_terminated"]),
                           f(b["total_reward"]), b["noise"].cuda(), cfg.lr, cfg.discount, cfg.loss_align_coeff, cfg.max_grad_norm, cfg.squashed_gaussian_policy)
            torch.cuda.synchronize()
            record_update(out, f"{case}/rpw{rpw}/update{k}", res, u)
    actions = f(b["action"])  # the Normal head's stored action, or the stored one-hot
    for tag, a in (("with_actions", actions), ("heads_only", None)):
        heads, q = u.forward(f(b["state"]), a)
        torch.cuda.synchronize()
        record(out, f"{case}/forward/{tag}", head=heads, **({} if q is None else {"q": q}))


def by_case(digests):
    """One SHA-256 per case (the first two parts of a key) over its keys and digests in key order: a whole output in a few dozen lines."""
    cases = {}
    for k in sorted(digests):
        cases.setdefault("/".join(k.split("/")[:2]), hashlib.sha256()).update(f"{k}={digests[k]}\n".encode())
    return {c: h.hexdigest() for c, h in cases.items()}


def compare(a_path, b_path, out_path):
    """Compares two outputs key by key and records both, folded to one digest per case, with the keys that differ; returns how many differ."""
    with open(a_path) as fa, open(b_path) as fb:
        a, b = json.load(fa), json.load(fb)
    differing = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
    result = dict(what="tools/mlp_rows_bits.py on two builds of libsrlx on one box: SHA-256 of every recorded array compared key by key; a_cases / b_cases hold one "
                       "SHA-256 per case over that build's keys and digests",
                  a=os.path.basename(a_path), b=os.path.basename(b_path), digests=len(set(a) | set(b)), differing=differing, a_cases=by_case(a), b_cases=by_case(b))
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(f"{result['digests']} digests, {len(differing)} differ; wrote {out_path}")
    return len(differing)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    args = ap.parse_args()
    if args.compare:
        sys.exit(1 if compare(args.compare[0], args.compare[1], args.out) else 0)
    assert torch.cuda.is_available(), "the tool needs a GPU"
    out = {}
    plain = [dict(obs_dim=1, in_sizes=(), hidden_sizes=(32,), n_actions=2), dict(obs_dim=256, in_sizes=(), hidden_sizes=(512, 32, 512), n_actions=32)]
    for k, (kw, B) in enumerate(zip(plain, (1, 9))):
        case = f"mlpq/plain{k}"
        mlpq_forward(out, case + "/forward", kw, 17, 10 + k)
        mlpq_td(out, case + "/train_step", kw, B, 1, "step", 20 + k)
        mlpq_td(out, case + "/train_nstep1", kw, B, 1, "nstep", 30 + k)
        mlpq_td(out, case + "/train_nstep3", kw, B, 3, "nstep", 40 + k)
    duel = [dict(obs_dim=5, in_sizes=(), hidden_sizes=(), n_actions=3, dueling_units=32), dict(obs_dim=5, in_sizes=(), hidden_sizes=(64, 96), n_actions=3, dueling_units=32)]
    for k, kw in enumerate(duel):
        mlpq_td(out, f"mlpq/dueling{k}/train_nstep3", kw, 5, 3, "nstep", 50 + k, max_nstep=3)
    mlpq_td(out, "mlpq/noisy/train_nstep3", dict(duel[1], noisy=True), 5, 3, "nstep", 60, max_nstep=3, draws=(7, 11))
    mlpq_categorical(out, "mlpq/c51_51", 4, (64,), 2, 51, 9, 70)
    mlpq_categorical(out, "mlpq/c51_256", 4, (64,), 2, 256, 9, 71)
    for i in (0, 3, 4):
        sacd(out, i)
    import notsac_cases
    import vppo_cases

    for name in vppo_cases.NAMES:
        vppo(out, name)
    for name in notsac_cases.NAMES:
        notsac(out, name)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(f"wrote {len(out)} digests to {args.out}")


if __name__ == "__main__":
    main()
