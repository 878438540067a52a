"""The image Q-network envelope tests' own footing, without a GPU (tests/qnet_envelope_reference.py has the tables and the yardstick):
(1) the case tables reach every dispatch class of csrc/srlx_qnet.hip / srlx_qnet_bwd.hip that the GPU file claims to cover, and the check notices a missing row;
(2) the randomised networks have mixed ReLUs at every case; (3) the float64 yardstick is what it says -- the reference-layout network and the float64 copy of the
kernel-layout network agree to float64 round-off, and float32 torch stays within 1e-6 of it, a tenth of the 1e-5 bar the kernels are held to.
The per-case checks use the first rows of the case's own inputs (at most ROWS: the properties are per row, and the whole file has to run in seconds)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qnet_envelope_reference as R  # noqa: E402

ROWS = 4
ALL_CASES = R.FORWARD_CASES + R.BACKWARD_CASES


def missing_classes(cases):
    """Names of the dispatch classes that `cases` do not reach (empty: full coverage)."""
    got = {k: set() for k in ("conv1", "conv_tile", "used", "splits", "head_block", "actions", "head", "fc1_dgrad", "amax")}
    for c in cases:
        d = R.dispatch_classes(c)
        kind = "plain" if c.head == "plain" else "dueling"
        for k, v in d.items():
            got[k] |= {(kind,) + e for e in v} if k == "head_block" else v
        if isinstance(c, R.BackwardCase):
            got["fc1_dgrad"] |= {(p, c.B) for p in d["fc1_dgrad"]}
    want = [("conv1 " + p, p in got["conv1"]) for p in ("fused", "k_conv1_u8/y1", "k_conv1_u8/y2", "AU8", "ANchw")]
    for conv in ("conv2", "conv3"):
        want += [(f"{conv} tile {t}", any(e[0] == conv and e[1] == t for e in got["conv_tile"])) for t in (64, 128)]
    # 84 x 84 with 32 filters: conv2 has 121 rows per sample and one column tile, ceil(121 B / 128) < 200 <=> B <= 210
    want += [("tile boundary B=210 (64 rows)", ("conv2", 64, 210) in got["conv_tile"]), ("tile boundary B=211 (128 rows)", ("conv2", 128, 211) in got["conv_tile"])]
    want += [("used " + r, r in got["used"]) for r in ("<8", "8", "9", "31|32", "33", "64", "34..63/remainder")]
    want += [("used < splits", any(u < s for s, u, _ in got["splits"]))]
    for kind in ("dueling", "plain"):
        want += [(f"{kind} head block 512 at B=256", (kind, 512, 256) in got["head_block"]), (f"{kind} head block 256 at B=257", (kind, 256, 257) in got["head_block"])]
        want += [(f"{kind} A={a}", (a, kind) in got["actions"]) for a in (1, 8, 9, 16, 17, 32)]
    want += [("AMAX %d" % a, a in got["amax"]) for a in (8, 16, 32)]
    want += [("head " + h, h in got["head"]) for h in ("average", "max", "naive", "plain")]
    want += [("fc1 dgrad mfma at B=32", ("mfma", 32) in got["fc1_dgrad"]), ("fc1 dgrad split at B=33", ("split", 33) in got["fc1_dgrad"])]
    return [name for name, ok in want if not ok]


def test_the_case_tables_reach_every_dispatch_class():
    assert missing_classes(ALL_CASES) == []


@pytest.mark.parametrize("row, lost", [
    (R.Case((24, 56), 1, 32, 32, 16, "average", (3,), 3968, ""), ["used 64"]),
    (R.Case((84, 84), 4, 128, 512, 32, "max", (8,), 8, ""), ["dueling A=32"]),
    (R.BackwardCase(44, 8, 64, 17, "naive", 33, 2), ["fc1 dgrad split at B=33"]),
])
def test_the_coverage_check_notices_a_missing_row(row, lost):
    """Rows that are the sole member of a class: without one, the coverage check names exactly what went with it."""
    match = [c for c in ALL_CASES if c[:-1] == row[:-1]] if isinstance(row, R.Case) else [c for c in ALL_CASES if c == row]
    assert len(match) == 1
    assert missing_classes([c for c in ALL_CASES if c is not match[0]]) == lost


def test_the_specified_rows_are_in_the_tables():
    fw = {(c.hw, c.window, c.filters, c.hidden, c.A, c.head) for c in R.FORWARD_CASES}
    for row in [((8, 8), 1, 32, 32, 1, "average"), ((84, 84), 4, 128, 512, 32, "max"), ((84, 84), 4, 64, 256, 17, "naive"), ((84, 84), 4, 32, 512, 6, "average"),
                ((44, 20), 3, 32, 64, 9, "average"), ((21, 37), 2, 64, 96, 16, "plain"), ((96, 88), 4, 32, 64, 8, "max"), ((36, 36), 8, 32, 160, 8, "plain"),
                ((20, 20), 4, 32, 960, 8, "average")]:
        assert row in fw, row
    by_shape = {(c.hw, c.filters): c for c in R.FORWARD_CASES}
    assert set(by_shape[((84, 84), 32)].batches) >= {210, 211, 256, 257}
    assert max(by_shape[((84, 84), 128)].batches) <= 8 and max(by_shape[((84, 84), 64)].batches) <= 37
    assert all(129 <= b <= 257 for b in by_shape[((20, 20), 32)].batches)
    assert any(max(c.batches) == c.max_batch for c in R.FORWARD_CASES) and any(max(c.batches) < c.max_batch for c in R.FORWARD_CASES)
    for row in [(8, 1, 32, 1, "average", 1, 1), (84, 4, 512, 32, "plain", 64, 1), (44, 8, 64, 17, "naive", 33, 2), (12, 3, 96, 9, "average", 31, 3),
                (36, 2, 480, 16, "naive", 32, 1), (20, 4, 32, 8, "plain", 7, 4)]:
        assert R.BackwardCase(*row) in R.BACKWARD_CASES, row


@pytest.mark.parametrize("case", ALL_CASES, ids=R.case_id)
def test_yardstick_and_relu_mix(case):
    net, inp = R.build(case)
    x = inp.x[:ROWS]
    want = R.reference_q(net, x)
    scale = float(want.abs().max())
    # Q-values are O(1): the randomisation's point (the default initialisation gives about 0.07)
    assert 0.3 <= scale <= 30.0, scale
    small = min(R.as_forward(case).batches)  # the smallest batch the GPU test judges against its own max |Q|
    assert small >= ROWS or float(want[:small].abs().max()) >= 0.3
    zeros = R.relu_zero_fractions(net, x)
    assert len(zeros) == (4 if net.plain else 5), zeros
    for name, frac in zeros.items():
        assert 0.2 <= frac <= 0.8, (name, frac)
    # the float64 copy of the kernel-layout network IS the reference-layout network: float64 round-off of at most 30 976 terms in another order (1e-13 leaves 30 x)
    with torch.no_grad():
        engine64 = R.engine_copy64(net)(x.double())
        engine32 = net(x)
    assert float((engine64 - want).abs().max()) <= 1e-13 * scale
    # float32 torch: the yardstick that shows the kernels' 1e-5 bar is about the kernels
    err32 = float((engine32.double() - want).abs().max())
    print(f"QNET-CPU {R.case_id(case)} scale={scale:.3f} f32_err/scale={err32 / scale:.2e} zeros={ {k.split('.')[-2] + '.' + k.split('.')[-1]: round(v, 2) for k, v in zeros.items()} }")
    assert err32 <= 1e-6 * scale


@pytest.mark.parametrize("case", R.BACKWARD_CASES, ids=R.case_id)
def test_no_training_row_unit_sits_on_its_relu_kink(case):
    """The gradient comparison's footing: float32 cannot decide a unit closer to zero than it evaluates pre-activations (qnet_envelope_reference.KINK_MARGIN)."""
    net, inp = R.build(case)
    assert R.kink_margin(net, inp.x[:: case.stride]) >= R.KINK_MARGIN


def test_reference_grads_speak_the_kernels_layouts():
    """Shapes and order of `reference_grads` are those of `kernel_parameters()`; rows outside `rows` contribute nothing; the plain head's unused entries are zero."""
    case = R.BACKWARD_CASES[5]
    net, inp = R.build(case)
    g = torch.Generator().manual_seed(0)
    grad_q = torch.randn((case.B, case.A), generator=g)
    rows = range(0, case.B * case.stride, case.stride)
    a = R.reference_grads(net, inp.x, grad_q, rows)
    assert [tuple(t.shape) for t in a] == [tuple(p.shape) for p in net.kernel_parameters()]
    x2 = inp.x.clone()
    x2[1::case.stride] = 0.5  # rows that are not training rows
    b = R.reference_grads(net, x2, grad_q, rows)
    assert all(torch.equal(s, t) for s, t in zip(a, b))
    assert float(a[8].abs().max()) == 0.0 and float(a[9].abs().max()) == 0.0 and all(float(a[k].abs().max()) > 0 for k in (0, 1, 2, 3, 4, 5, 6, 7, 10, 11))
