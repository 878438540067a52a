"""The kernels of csrc/srlx_train.hip over the envelope their entry points admit, through the C ABI: the n-step TD / Huber / priority kernel (dense and
packed), the 1-step DQN target, the GAE scan and the multi-tensor Adam step, each against its yardstick of oracle/hot_path_oracle.py (Adam: torch.optim.Adam
on the CPU) on the cases of tests/train_kernels_reference.py -- whose promises about ties, masks, retrace cuts and Huber regions tests/test_train_kernels_cpu.py
asserts without a GPU.  Every buffer a kernel writes has 64 sentinel elements behind it; every refusal is shown to have written nothing.  Each test prints its
worst distance as a fraction of its bar."""
import numpy as np
import pytest

import train_kernels_reference as R
from train_kernels_reference import F32, F64, I64, U8, Buf, D, H, P, refused, same_bits

pytestmark = pytest.mark.gpu


def _env():
    from simple_distributed_rl_amd import _native as N

    return N, N.lib()


def same_bits_where_finite(got, want, what):
    """The same bits wherever the yardstick is finite; elsewhere the same infinity, or NaN on both sides (a NaN's payload is nobody's contract)."""
    fin = np.isfinite(want)
    same_bits(got[fin], want[fin], what)
    np.testing.assert_array_equal(got[~fin], want[~fin], err_msg=what)


# ---- 1. n-step TD, dense and packed ----------------------------------------------------------------------------------------------------------------------------
def _td_inputs(c, d):
    return dict(q_on=D(d["q_on"]), q_tg=D(d["q_tg"]), q0=D(d["q0"]), q_all=D(R.pack_q(d)), act=D(d["act"]), rew=D(d["rew"]), done=D(d["done"]),
                inv=D(None if d["inv"] is None else d["inv"].astype(U8)), w=D(d["w"]))


def _td_call(N, lib, c, t, packed, B=None, n=None, null_output=False):
    B, n, A = c["B"] if B is None else B, c["n"] if n is None else n, c["A"]
    out = dict(target=Buf(max(B, 1)), loss=Buf(1), grad=Buf((max(B, 1), A)), pri=Buf(max(B, 1)))
    discount, h = c["dh"]
    tail = (P(t["act"]), P(t["rew"]), P(t["done"]), P(t["inv"]), P(t["w"]), discount, h, c["dd"], c["rs"], None if null_output else out["target"].ptr(), out["loss"].ptr(),
            out["grad"].ptr(), out["pri"].ptr(), None)
    if packed:
        status = lib.srlx_nstep_td_huber_priority_packed(B, n, A, P(t["q_all"]), P(t["q_tg"]), *tail)
    else:
        status = lib.srlx_nstep_td_huber_priority(B, n, A, P(t["q_on"]), P(t["q_tg"]), P(t["q0"]), *tail)
    return status, out


def _td_run(N, lib, c, t, packed):
    status, out = _td_call(N, lib, c, t, packed)
    N.check(status)
    return {k: b.get() for k, b in out.items()}


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_td_case(c):
    N, lib = _env()
    d = R.nstep_case(c)
    t = _td_inputs(c, d)
    where = R.case_id(c)
    B, A = c["B"], c["A"]
    got = _td_run(N, lib, c, t, packed=False)
    want = R.nstep_oracle(c, d)
    want64 = R.nstep_oracle(c, d, F64)
    assert want.dtype == F32
    with np.errstate(invalid="ignore"):
        if c["rs"]:
            print("ENVELOPE %s target: %.0f %% of the rows bit-equal to the float32 oracle" % (where, 100 * R.bit_equal_share(got["target"], want)))
            R.check("target", got["target"], want, R.RTOL, 1e-6, want64, where)
        else:
            R.check("target", got["target"], want, R.RTOL, 1e-6, want64, where)
            same_bits_where_finite(got["target"], want, where + " target")
        wl, wg, wp = H.huber_loss_grad_priority(d["q0"], d["act"][:, 0], got["target"], d["w"])
        R.check("loss", got["loss"][0], wl, R.RTOL, 0.0, None, where)
        R.check("grad", got["grad"], wg, R.RTOL, 1e-9, None, where)
        same_bits_where_finite(got["pri"], wp.astype(F32), where + " priorities = |target - q0| of the kernel's own target")
    off = np.ones((B, A), bool)
    off[np.arange(B), d["act"][:, 0]] = False
    assert (_u32(got["grad"])[off] == 0).all(), where + ": a gradient entry off the taken action is not +0"
    packed = _td_run(N, lib, c, t, packed=True)
    again = _td_run(N, lib, c, t, packed=False)
    for k in got:
        assert np.array_equal(_u32(packed[k]), _u32(got[k])), f"{where}: packed {k} differs from dense"
        assert np.array_equal(_u32(again[k]), _u32(got[k])), f"{where}: a second call gives another {k}"


@pytest.mark.parametrize("c", R.NSTEP_CASES + R.NSTEP_FINITE_CASES, ids=R.case_id)
def test_nstep_td_envelope(c):
    """Dense and packed entry, thinned cross product of B x n x A x double_dqn x rescale x mask x (discount, retrace_h).  target / loss / gradient seed /
    priorities at the bars of test_nstep_td_random_vs_oracle (rtol 1e-5, atol 1e-6 / 0 / 1e-9, priorities exact); without rescale the target is the float32
    oracle's bits at every n (the discounted sum runs in numpy's pairwise order from 8 terms up); with rescale the bar holds and the bit-equal share is printed
    (the oracle's np.sqrt rounds in float32 arithmetic, the kernel rounds a float64 square root once).  Where a mask is given and double DQN is off, row 0 has
    a step with every action invalid: the reference reads -inf back from the masked target net, so that row's target is -inf or NaN here as there -- and the
    batch's loss with it, on both sides, so in those cases the loss assertion compares nothing; the two cases with "whole0" give that pair (mask given, double DQN
    off) without the all-invalid step, and there the loss is a number."""
    _check_td_case(c)


@pytest.mark.parametrize("c", R.NSTEP_ORDER_CASES, ids=R.case_id)
def test_nstep_target_is_the_oracle_bit_for_bit_at_every_n(c):
    """B = 257, A = 4, no rescale, n in {1, 2, 7, 8, 9, 32}: the target is hot_path_oracle.nstep_target's float32 bits (tests/test_train_kernels_cpu.py shows
    on these inputs that adding the terms one after another is not, from n = 8 up)."""
    _check_td_case(c)


@pytest.mark.parametrize("packed", [False, True], ids=["dense", "packed"])
def test_nstep_td_refusals_write_nothing(packed):
    N, lib = _env()
    c = dict(B=5, n=3, A=4, dd=1, rs=0, mask=1, dh=(0.99, 0.95))
    t = _td_inputs(c, R.nstep_case(c))
    for kw in (dict(n=0), dict(n=33), dict(B=0), dict(null_output=True)):
        status, out = _td_call(N, lib, c, t, packed, **kw)
        refused(N, lib, status, "nstep_td")
        assert all(b.untouched() for b in out.values()), kw


# ---- 2. srlx_dqn_target ----------------------------------------------------------------------------------------------------------------------------------------
def _dqn_call(N, lib, c, d, out, null_online=False):
    inv = None if d["inv"] is None else d["inv"].astype(U8)
    keep = [D(d["q_on"]), D(d["q_tg"]), D(d["rew"]), D(d["undone"]), D(inv), D(d["disc_ps"])]
    return lib.srlx_dqn_target(c["B"], c["A"], None if null_online else P(keep[0]), P(keep[1]), P(keep[2]), P(keep[3]), P(keep[4]), d["discount"], P(keep[5]), c["dd"], c["rs"],
                               c["f64"], out.ptr(), None), keep


def _check_dqn(c, d):
    N, lib = _env()
    where = R.case_id(c)
    out = Buf(c["B"])
    status, keep = _dqn_call(N, lib, c, d, out)
    N.check(status)
    got, want = out.get(), R.dqn_oracle(c, d)
    R.check("target", got, want, R.RTOL, 1e-7, R.dqn_oracle(c, d, f64=True), where)
    if not c["rs"]:
        same_bits(got, want, where)
    else:
        print("ENVELOPE %s target: %.0f %% of the rows bit-equal" % (where, 100 * R.bit_equal_share(got, want)))


@pytest.mark.parametrize("c", R.DQN_CASES, ids=R.case_id)
def test_dqn_target_envelope(c):
    """Thinned cross product of B x A x double_dqn x rescale x f64_accum x per-sample discount x mask; the batch-wide minimum that replaces masked entries sits
    in the last row and decides others.  Without rescale bit-equal to the oracle, with rescale rtol 1e-5 / atol 1e-7."""
    _check_dqn(c, R.dqn_case(c))


@pytest.mark.parametrize("dd", [1, 0])
def test_dqn_target_minimum_inside_a_masked_entry(dd):
    c = dict(B=257, A=18, dd=dd, rs=0, f64=0, ps=0, mask="some")
    _check_dqn(c, R.dqn_case(c, min_masked=True))


def test_dqn_target_refusals_write_nothing():
    N, lib = _env()
    c = dict(B=7, A=3, dd=1, rs=0, f64=1, ps=1, mask="some")
    d = R.dqn_case(c)
    out = Buf(7)
    status, keep = _dqn_call(N, lib, c, d, out)
    refused(N, lib, status, "per-sample discount")
    c = dict(c, f64=0)
    status, keep = _dqn_call(N, lib, c, d, out, null_online=True)
    refused(N, lib, status, "dqn_target")
    status, keep = _dqn_call(N, lib, dict(c, B=0), d, out)
    refused(N, lib, status, "dqn_target")
    assert out.untouched()


# ---- 3. srlx_gae_scan ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.GAE_CASES, ids=R.case_id)
def test_gae_scan_envelope(c):
    """Bit-equal to hot_path_oracle.gae; with done on the last step the bootstrap values (about 10, so that using them would show) must be ignored."""
    N, lib = _env()
    d = R.gae_case(c)
    E, T = c["E"], c["T"]
    keep = [D(d["rew"]), D(d["val"]), D(d["done"]), D(d["last"])]
    out = Buf((T, E))
    N.check(lib.srlx_gae_scan(E, T, P(keep[0]), P(keep[1]), P(keep[2]), P(keep[3]), c["gl"][0], c["gl"][1], out.ptr(), None))
    want = H.gae(d["rew"], d["val"], d["done"], d["last"], *c["gl"])
    same_bits(out.get(), want, R.case_id(c))
    if c["done"] == "last" and c["boot"]:
        same_bits(want, H.gae(d["rew"], d["val"], d["done"], None, *c["gl"]), "the oracle ignores the bootstrap behind a finished episode")
    untouched = Buf((T, E))
    refused(N, lib, lib.srlx_gae_scan(0, T, P(keep[0]), P(keep[1]), P(keep[2]), None, 0.9, 0.9, untouched.ptr(), None), "gae_scan")
    assert untouched.untouched()


# ---- 4. srlx_adam_step -----------------------------------------------------------------------------------------------------------------------------------------
LR, BETAS, EPS = 2.5e-4, (0.9, 0.999), 1e-8
CHUNK_EDGE_SIZES = (1, 1, 3, 4095, 4096, 4097, 8192)  # either side of the 4096-element chunk and of its float4 path; two single-element tensors side by side


def _adam_data(sizes, seed):
    rng = np.random.default_rng([11, seed, len(sizes)])
    p = [(rng.standard_normal(n) * 0.1).astype(F32) for n in sizes]
    g = [(rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-12, 3, n)).astype(F32) for n in sizes]  # 1e-12 .. 1e3
    m = [(rng.standard_normal(n) * 0.01).astype(F32) for n in sizes]
    v = [(rng.random(n) * 1e-4).astype(F32) for n in sizes]
    return p, g, m, v


def _torch_adam(p, g, m, v, steps_taken, dtype):
    import torch

    params = [torch.nn.Parameter(torch.tensor(x, dtype=dtype)) for x in p]
    opt = torch.optim.Adam(params, lr=LR, betas=BETAS, eps=EPS, foreach=False)
    for q, gg, mm, vv in zip(params, g, m, v):
        q.grad = torch.tensor(gg, dtype=dtype)
        opt.state[q] = dict(step=torch.tensor(float(steps_taken)), exp_avg=torch.tensor(mm, dtype=dtype), exp_avg_sq=torch.tensor(vv, dtype=dtype))
    opt.step()
    assert all(float(opt.state[q]["step"]) == steps_taken + 1 for q in params)
    return [q.detach().numpy() for q in params], [opt.state[q]["exp_avg"].numpy() for q in params], [opt.state[q]["exp_avg_sq"].numpy() for q in params]


def _adam_call(N, lib, bufs, g_dev, sizes, step_dev, n_tensors=None, p_offset=0, numels=None):
    k = len(sizes) if n_tensors is None else n_tensors
    arr = lambda ptrs: (N.c_p * len(ptrs))(*[x.value for x in ptrs])  # noqa: E731
    pp = arr([b.ptr(p_offset if i == 0 else 0) for i, b in enumerate(bufs["p"])])
    gg = arr([P(x) for x in g_dev])
    mm, vv = arr([b.ptr() for b in bufs["m"]]), arr([b.ptr() for b in bufs["v"]])
    nn = (N.c_i64 * len(sizes))(*(sizes if numels is None else numels))
    return lib.srlx_adam_step(k, pp, gg, mm, vv, nn, LR, BETAS[0], BETAS[1], EPS, P(step_dev), None)


def _adam_setup(sizes, seed):
    p, g, m, v = _adam_data(sizes, seed)
    bufs = dict(p=[Buf(len(x), F32, x) for x in p], m=[Buf(len(x), F32, x) for x in m], v=[Buf(len(x), F32, x) for x in v])
    return (p, g, m, v), bufs, [D(x) for x in g]


def _adam_check(N, lib, sizes, steps_taken, seed):
    (p, g, m, v), bufs, g_dev = _adam_setup(sizes, seed)
    step_dev = D(np.array([steps_taken], I64))
    N.check(_adam_call(N, lib, bufs, g_dev, sizes, step_dev))
    rp, rm, rv = _torch_adam(p, g, m, v, steps_taken, __import__("torch").float32)
    dp, dm, dv = _torch_adam(p, g, m, v, steps_taken, __import__("torch").float64)
    worst = dict(p=0.0, m=0.0, v=0.0, p64=0.0, ref64=0.0)
    for k in range(len(sizes)):
        gp, gm, gv = bufs["p"][k].get(), bufs["m"][k].get(), bufs["v"][k].get()  # (each checks its sentinels)
        m_atol = 2e-7 * float(np.abs(rm[k]).max())  # m + w (g - m) cancels: compare on the scale of the tensor (test_device_adam_matches_torch_adam)
        worst["m"] = max(worst["m"], R.bar_fraction(gm, rm[k], 2e-6, m_atol))
        worst["v"] = max(worst["v"], R.bar_fraction(gv, rv[k], 2e-6, 1e-20))
        worst["p"] = max(worst["p"], R.bar_fraction(gp, rp[k], 1e-6, 2e-8))
        worst["p64"] = max(worst["p64"], R.bar_fraction(gp, dp[k], 1e-6, 2e-8))
        worst["ref64"] = max(worst["ref64"], R.bar_fraction(rp[k], dp[k], 1e-6, 2e-8))
    print("ENVELOPE adam sizes %s step %d: kernel vs float32 torch, fractions of the bars: p %.3g m %.3g v %.3g; p vs float64 Adam %.3g; float32 torch vs float64 %.3g" % (
        "x".join(map(str, sorted(set(sizes)))), steps_taken, worst["p"], worst["m"], worst["v"], worst["p64"], worst["ref64"]))
    for k in range(len(sizes)):
        gp, gm, gv = bufs["p"][k].get(), bufs["m"][k].get(), bufs["v"][k].get()
        np.testing.assert_allclose(gm, rm[k], rtol=2e-6, atol=2e-7 * float(np.abs(rm[k]).max()), err_msg=f"m {k}")
        np.testing.assert_allclose(gv, rv[k], rtol=2e-6, atol=1e-20, err_msg=f"v {k}")
        np.testing.assert_allclose(gp, rp[k], rtol=1e-6, atol=2e-8, err_msg=f"p {k}")
        assert (gp != p[k]).mean() > 0.5 or len(gp) < 4, k  # the step moved the tensor


@pytest.mark.parametrize("steps_taken", [0, 1, 10 ** 6])
def test_adam_chunk_edges_and_step_counter(steps_taken):
    """One call over tensors of 1, 1, 3, 4095, 4096, 4097 and 8192 elements, gradients from 1e-12 to 1e3, the step count read from the device scalar: 0 and 1
    (bias corrections 0.1 / 0.001 and 0.19 / 0.002) and 10^6 (both 1).  torch.optim.Adam in float32 on the CPU at the bars of
    test_device_adam_matches_torch_adam; a float64 Adam beside it, printed."""
    N, lib = _env()
    _adam_check(N, lib, CHUNK_EDGE_SIZES, steps_taken, 0)


def test_adam_table_edges():
    """24 tensors (the table's size) in one call; 25 are refused and nothing is written."""
    N, lib = _env()
    sizes = tuple(1 + (37 * i) % 300 for i in range(24))
    _adam_check(N, lib, sizes, 3, 1)
    sizes = sizes + (5,)
    (p, g, m, v), bufs, g_dev = _adam_setup(sizes, 2)
    refused(N, lib, _adam_call(N, lib, bufs, g_dev, sizes, D(np.array([0], I64))), "adam_step")
    for name, host in (("p", p), ("m", m), ("v", v)):
        for b, x in zip(bufs[name], host):
            same_bits(b.get(), x, "a refused call wrote")


def test_adam_refusals_write_nothing():
    """A parameter view offset by one float (not 16-byte aligned), an empty tensor, no tensors at all and a NULL step counter."""
    N, lib = _env()
    sizes = (40, 8)
    (p, g, m, v), bufs, g_dev = _adam_setup(sizes, 3)
    step_dev = D(np.array([0], I64))
    refused(N, lib, _adam_call(N, lib, bufs, g_dev, sizes, step_dev, p_offset=1, numels=(39, 8)), "not 16-byte aligned")
    refused(N, lib, _adam_call(N, lib, bufs, g_dev, sizes, step_dev, numels=(40, 0)), "NULL or empty")
    refused(N, lib, _adam_call(N, lib, bufs, g_dev, sizes, step_dev, n_tensors=0), "adam_step")
    refused(N, lib, _adam_call(N, lib, bufs, g_dev, sizes, None), "adam_step")
    for name, host in (("p", p), ("m", m), ("v", v)):
        for b, x in zip(bufs[name], host):
            same_bits(b.get(), x, "a refused call wrote")
