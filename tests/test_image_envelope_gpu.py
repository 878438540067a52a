"""srlx_image_preprocess (csrc/srlx_image.hip) over the envelope it admits, bit-equal (uint8 and float32) to oracle/image_oracle.py on random uint8
images.  tests/test_image_processor.py runs the ALE geometries with `normalize = 1`, `max_val = 255`; here every branch and clamp of the kernel's
`axis()` / `tap()` has a geometry of its own -- up-scaling (both border clamps), a 1 x 1 source, a 1 x 1 output, one axis left alone, exact 1/2, 1/3 and
1/4 scales that must take the linear path, the 2 x 2 area path inside a trimming window, windows that end at the last row and column or hold one
pixel -- for one and three images, every normalisation with two divisors over all 256 byte values, and each combination of the two outputs.  Every output
buffer carries a sentinel tail that must survive."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import image_oracle as O  # noqa: E402

from simple_distributed_rl_amd import _native as N  # noqa: E402

pytestmark = pytest.mark.gpu
TAIL, U8_SENTINEL, F32_SENTINEL = 64, 0xA5, -9.25
NORMS = {0: "", 1: "0to1", 2: "-1to1"}

# (id, source shape, to_gray, trimming (top, left, bottom, right) or None, resize (w, h) or None): what the geometry is there for
GEOMETRIES = [
    ("up-5x7-to-16x20", (5, 7), False, None, (20, 16)),  # up-scaling: negative first coordinates clamp to 0, the last ones to src - 1
    ("up-rgb-to-gray", (5, 7, 3), True, None, (20, 16)),
    ("source-1x1", (1, 1, 3), False, None, (4, 4)),  # src - 1 == 0: both clamps on every output pixel
    ("source-1x1-gray", (1, 1), False, None, (4, 4)),
    ("output-1x1", (37, 23, 3), True, None, (1, 1)),  # one tap pair from the middle of the image
    ("output-1x1-rgb", (6, 9, 3), False, None, (1, 1)),
    ("width-only-40x30-to-40x17", (40, 30), False, None, (17, 40)),  # one axis unchanged (weights 2048 / 0), the other resized
    ("height-only-40x30-to-17x30", (40, 30, 3), True, None, (30, 17)),
    ("half-height-only", (40, 30), False, None, (17, 20)),  # one axis exactly x 1/2, the other not: the linear path, not the 2 x 2 area path
    ("half-width-only", (40, 30, 3), False, None, (15, 17)),
    ("third-48-to-16", (48, 48), False, None, (16, 16)),  # exact x 1/3 and x 1/4: linear too (only 2 x 2 has the area special case)
    ("quarter-64-to-16", (64, 64, 3), True, None, (16, 16)),
    ("third-by-quarter", (48, 64), False, None, (16, 16)),
    ("area-2x2-in-a-window", (50, 46, 3), True, (3, 5, 43, 45), (20, 20)),  # the exact 2 x 2 case of the trimming window, not of the source
    ("area-2x2-in-a-window-rgb", (50, 46, 3), False, (3, 5, 43, 45), (20, 20)),
    ("source-2x-but-window-not", (40, 40), False, (0, 0, 39, 40), (20, 20)),  # the source is 2 x the output, the window is not: linear
    ("window-to-the-last-row-and-column", (33, 29), False, (10, 9, 33, 29), None),
    ("window-to-the-last-row-and-column-resized", (33, 29, 3), True, (10, 9, 33, 29), (7, 11)),
    ("window-of-one-pixel", (12, 14, 3), True, (4, 6, 5, 7), None),
    ("window-of-one-pixel-resized", (12, 14, 3), False, (11, 13, 12, 14), (3, 3)),  # the last pixel of the image
    ("rgb-kept-through-window-and-resize", (31, 27, 3), False, (2, 3, 29, 25), (13, 9)),
    ("to-gray-on-one-channel", (20, 24), True, None, (10, 7)),  # to_gray = 1 with nothing to convert
    ("to-gray-on-one-channel-window", (20, 24), True, (1, 2, 19, 20), None),
]


def _call(imgs, to_gray, trim, resize, norm=1, max_val=255.0, want_u8=True, want_f32=True, override=None):
    """One launch; returns (status, uint8 buffer or None, float32 buffer or None, elements per launch), the buffers TAIL elements longer than the output."""
    n, h, w = imgs.shape[0], imgs.shape[1], imgs.shape[2]
    ch = imgs.shape[3] if imgs.ndim == 4 else 1
    top, left, bottom, right = trim if trim else (0, 0, h, w)
    ow, oh = resize if resize else (right - left, bottom - top)
    oc = 1 if (to_gray or ch == 1) else 3
    total = n * oh * ow * oc
    src = torch.from_numpy(imgs).cuda()
    out = torch.full((total + TAIL,), U8_SENTINEL, dtype=torch.uint8, device="cuda") if want_u8 else None
    outf = torch.full((total + TAIL,), F32_SENTINEL, dtype=torch.float32, device="cuda") if want_f32 else None
    args = dict(n=n, h=h, w=w, ch=ch, to_gray=int(to_gray), top=top, left=left, bottom=bottom, right=right, oh=oh, ow=ow, norm=norm)
    args.update(override or {})
    a = args
    status = N.lib().srlx_image_preprocess(a["n"], a["h"], a["w"], a["ch"], N.tptr(src), a["to_gray"], a["top"], a["left"], a["bottom"], a["right"], a["oh"], a["ow"],
                                           N.tptr(out), N.tptr(outf), a["norm"], float(max_val), None)
    torch.cuda.synchronize()
    return status, (None if out is None else out.cpu().numpy()), (None if outf is None else outf.cpu().numpy()), total


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _want(imgs, to_gray, trim, resize, norm="", max_val=255.0):
    return np.stack([O.image_process(im, to_gray, trim, resize, norm, max_val) for im in imgs])


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("name,shape,to_gray,trim,resize", GEOMETRIES, ids=[g[0] for g in GEOMETRIES])
def test_geometry_bit_equal_to_the_oracle(name, shape, to_gray, trim, resize, n):
    rng = np.random.default_rng(len(name) * 1000 + sum(shape) + n)
    imgs = rng.integers(0, 256, (n,) + shape, dtype=np.uint8)
    status, out, outf, total = _call(imgs, to_gray, trim, resize, norm=1)
    N.check(status)
    want = _want(imgs, to_gray, trim, resize)
    assert want.dtype == np.uint8 and want.size == total
    assert np.array_equal(out[:total], want.reshape(-1))
    assert np.array_equal(_bits(outf[:total]), _bits(_want(imgs, to_gray, trim, resize, "0to1").reshape(-1)))
    assert (out[total:] == U8_SENTINEL).all() and (outf[total:] == np.float32(F32_SENTINEL)).all(), "a store past the output"


def test_geometries_reach_their_branches():
    """Conditions on the table itself (no kernel): which geometry is a resize, which the area path, which windows touch the far edge."""
    by = {g[0]: g for g in GEOMETRIES}

    def window(g):
        h, w = g[1][0], g[1][1]
        top, left, bottom, right = g[3] if g[3] else (0, 0, h, w)
        return bottom - top, right - left

    def area(g):
        th, tw = window(g)
        return g[4] is not None and (th, tw) == (2 * g[4][1], 2 * g[4][0])

    assert [g[0] for g in GEOMETRIES if area(g)] == ["area-2x2-in-a-window", "area-2x2-in-a-window-rgb"]
    for name in ("half-height-only", "half-width-only"):
        th, tw = window(by[name])
        assert (th == 2 * by[name][4][1]) != (tw == 2 * by[name][4][0])
    assert window(by["third-48-to-16"]) == (48, 48) and window(by["quarter-64-to-16"]) == (64, 64) and window(by["third-by-quarter"]) == (48, 64)
    th, tw = window(by["width-only-40x30-to-40x17"])
    assert th == by["width-only-40x30-to-40x17"][4][1] and tw != by["width-only-40x30-to-40x17"][4][0]
    th, tw = window(by["height-only-40x30-to-17x30"])
    assert tw == by["height-only-40x30-to-17x30"][4][0] and th != by["height-only-40x30-to-17x30"][4][1]
    for name in ("window-to-the-last-row-and-column", "window-to-the-last-row-and-column-resized", "window-of-one-pixel-resized"):
        g = by[name]
        assert g[3][2] == g[1][0] and g[3][3] == g[1][1] and g[3][0] > 0 and g[3][1] > 0
    assert window(by["window-of-one-pixel"]) == (1, 1) == window(by["window-of-one-pixel-resized"])
    g = by["source-2x-but-window-not"]
    assert (g[1][0], g[1][1]) == (2 * g[4][1], 2 * g[4][0]) and not area(g)
    up = by["up-5x7-to-16x20"]
    assert up[4][0] > up[1][1] and up[4][1] > up[1][0]
    assert not by["rgb-kept-through-window-and-resize"][2] and by["to-gray-on-one-channel"][2] and len(by["to-gray-on-one-channel"][1]) == 2


@pytest.mark.parametrize("outputs", ["u8", "f32", "both"])
@pytest.mark.parametrize("max_val", [255.0, 127.0])
@pytest.mark.parametrize("norm", [0, 1, 2])
def test_normalisation_over_every_byte_value(norm, max_val, outputs):
    img = np.arange(256, dtype=np.uint8).reshape(1, 16, 16)
    status, out, outf, total = _call(img, False, None, None, norm=norm, max_val=max_val, want_u8=outputs != "f32", want_f32=outputs != "u8")
    N.check(status)
    assert total == 256
    if out is not None:
        assert np.array_equal(out[:256], np.arange(256, dtype=np.uint8)) and (out[256:] == U8_SENTINEL).all()
    if outf is not None:
        x, m = np.arange(256, dtype=np.float32), np.float32(max_val)
        want = {0: x, 1: x / m, 2: x / m * np.float32(2) - np.float32(1)}[norm]
        assert want.dtype == np.float32
        oracle = O.image_process(img[0], False, None, None, NORMS[norm], max_val).astype(np.float32).reshape(-1)
        assert np.array_equal(_bits(want), _bits(oracle)), "x / max * 2 - 1 and the oracle's x * 2 / max - 1: the doubling is exact either way"
        assert np.array_equal(_bits(outf[:256]), _bits(want))
        assert (outf[256:] == np.float32(F32_SENTINEL)).all()
        if norm:
            assert want[0] == (0 if norm == 1 else -1) and (want[255] == 1) == (max_val == 255.0)


def test_normalisation_behind_gray_window_and_resize():
    """The float32 output is the normalised uint8 output, on the linear path of an RGB image too, for both divisors."""
    rng = np.random.default_rng(5)
    imgs = rng.integers(0, 256, (3, 31, 27, 3), dtype=np.uint8)
    for norm in (0, 1, 2):
        for max_val in (255.0, 127.0):
            status, out, outf, total = _call(imgs, True, (2, 3, 29, 25), (13, 9), norm=norm, max_val=max_val)
            N.check(status)
            assert np.array_equal(out[:total], _want(imgs, True, (2, 3, 29, 25), (13, 9)).reshape(-1))
            want = _want(imgs, True, (2, 3, 29, 25), (13, 9), NORMS[norm], max_val).astype(np.float32)
            assert np.array_equal(_bits(outf[:total]), _bits(want.reshape(-1)))
            assert (out[total:] == U8_SENTINEL).all() and (outf[total:] == np.float32(F32_SENTINEL)).all()


REFUSALS = [
    ("two-channels", (8, 9, 2), {}),
    ("four-channels", (8, 9, 4), {}),
    ("empty-window-rows", (8, 9, 3), dict(top=4, bottom=4)),
    ("empty-window-columns", (8, 9, 3), dict(left=5, right=5)),
    ("window-past-the-right-edge", (8, 9, 3), dict(right=10)),
    ("window-past-the-bottom-edge", (8, 9, 3), dict(bottom=9)),
    ("negative-top", (8, 9, 3), dict(top=-1)),
    ("negative-left", (8, 9, 3), dict(left=-1)),
    ("out-h-0", (8, 9, 3), dict(oh=0)),
    ("out-w-0", (8, 9, 3), dict(ow=0)),
    ("normalize-3", (8, 9, 3), dict(norm=3)),
    ("normalize-negative", (8, 9, 3), dict(norm=-1)),
    ("no-images", (8, 9, 3), dict(n=0)),
]


@pytest.mark.parametrize("name,shape,override", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_write_nothing(name, shape, override):
    imgs = np.random.default_rng(0).integers(0, 256, (2,) + shape, dtype=np.uint8)
    status, out, outf, _ = _call(imgs, False, None, None, override=override)
    assert status != N.OK
    with pytest.raises(N.SrlxError):
        N.check(status)
    assert (out == U8_SENTINEL).all() and (outf == np.float32(F32_SENTINEL)).all()


def test_both_outputs_null_is_refused():
    imgs = np.zeros((1, 8, 9, 3), np.uint8)
    status, out, outf, _ = _call(imgs, True, None, None, want_u8=False, want_f32=False)
    assert status != N.OK and out is None and outf is None
    src = torch.from_numpy(imgs).cuda()
    out = torch.full((72,), U8_SENTINEL, dtype=torch.uint8, device="cuda")
    assert N.lib().srlx_image_preprocess(1, 8, 9, 3, None, 1, 0, 0, 8, 9, 8, 9, N.tptr(out), None, 0, 255.0, None) != N.OK  # and a NULL source
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == U8_SENTINEL).all()
    N.check(N.lib().srlx_image_preprocess(1, 8, 9, 3, N.tptr(src), 1, 0, 0, 8, 9, 8, 9, N.tptr(out), None, 0, 255.0, None))  # the same call, whole
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0).all()
