"""The cases of tests/test_rank_envelope_gpu.py checked where there is no GPU (tests/rank_cases.py).  Two things: every key population has the
property it is there for, so that the GPU comparison cannot pass on keys that miss their subject; and the cases discriminate -- a numpy emulation of
the sort under the key image of this commit's parent (raw bits: +NaN above +inf, +0.0 above -0.0) leaves numpy's order on exactly the NaN and
signed-zero populations, at every size, while the emulation under the fixed image agrees with the yardstick on every case."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rank_cases as C  # noqa: E402

U32 = np.uint32


@pytest.mark.parametrize("c", C.CASES, ids=C.CASE_IDS)
def test_key_images_against_the_yardstick(c):
    p = C.keys(c)
    want = C.yardstick(p)
    assert np.array_equal(np.sort(want), np.arange(c.n))
    assert np.array_equal(C.order_by(C.fixed_image(p)), want), "the fixed image leaves numpy's stable order"
    parent = C.order_by(C.parent_image(p))
    moves = C.BY_NAME[c.population].moves
    assert (not np.array_equal(parent, want)) == moves, "the parent's image differs from numpy on the NaN and signed-zero populations and nowhere else"
    if moves:
        print(f"RANK-ENV {c.population}-{c.n}: the parent's image misplaces {int((parent != want).sum())} of {c.n} ranks")


def test_the_issue_examples():
    """The two divergences as the issue states them."""
    nan = np.float32(np.nan)
    a = np.array([1, nan, 3, nan, 2, -nan, 0], np.float32)
    assert C.yardstick(a).tolist() == [2, 4, 0, 6, 1, 3, 5] == C.order_by(C.fixed_image(a)).tolist()
    assert C.order_by(C.parent_image(a)).tolist() == [1, 3, 2, 4, 0, 6, 5]
    z = np.array([0.0, -0.0, 1, -0.0, 0.0, -1], np.float32)
    assert C.yardstick(z).tolist() == [2, 0, 1, 3, 4, 5] == C.order_by(C.fixed_image(z)).tolist()
    assert C.order_by(C.parent_image(z)).tolist() == [2, 0, 4, 1, 3, 5]


def test_fixed_image_ends():
    """-inf's image is 0xff800000 and the NaNs' is the one above it; the finite images are untouched by the fix."""
    ninf = np.array([-np.inf], np.float32)
    assert C.fixed_image(ninf)[0] == U32(0xFF800000) == C.parent_image(ninf)[0]
    every_nan = np.array(C.NAN_BITS, np.int64).astype(U32).view(np.float32)
    assert (C.fixed_image(every_nan) == U32(0xFFFFFFFF)).all()
    rng = np.random.default_rng(0)
    finite = rng.integers(0, 1 << 32, 100_000).astype(U32)
    finite = finite[~C.is_nan_bits(finite) & ((finite & U32(0x7FFFFFFF)) != 0)].view(np.float32)
    assert np.array_equal(C.fixed_image(finite), C.parent_image(finite))
    assert (C.fixed_image(finite) < U32(0xFFFFFFFF)).all()


def test_sizes_sit_on_the_kernel_borders():
    s = set(C.SIZES)
    for border in (C.GROUP, C.CHUNK, C.TILE):
        assert {border - 1, border, border + 1} <= s
    blocks = lambda n: -(-n // C.TILE)  # noqa: E731
    assert 256 * blocks(16384) == 1024 and 256 * blocks(16385) == 1280 and blocks(20481) == 6 and 20481 % C.TILE == 1
    assert {1, 2} <= s and max(s) < C.CAPACITY
    assert set(C.BY_NAME["distinct"].sizes) == s, "one population walks every size"
    for pop in C.POPULATIONS:
        assert set(pop.sizes) <= s and len(pop.sizes) >= 4 and pop.why, pop.name
        assert max(pop.sizes) > C.TILE, f"{pop.name}: more than one workgroup"
        assert not pop.moves or min(pop.sizes) >= 2  # one key cannot be misplaced


def _cases(name):
    return [c for c in C.CASES if c.population == name]


def test_populations_have_their_defining_property():
    for c in _cases("distinct"):
        p = C.keys(c)
        assert len(np.unique(p)) == c.n and np.isfinite(p).all() and not (p == 0).any()
        assert c.n == 1 or ((p > 0).any() and (p < 0).any())
    for c in _cases("equal"):
        assert len(np.unique(C.bits(C.keys(c)))) == 1
    for c in _cases("few"):
        values, counts = np.unique(C.keys(c), return_counts=True)
        assert len(values) == 3 and (values < 0).any()
        assert c.n < 16384 or counts.max() > C.TILE, "a tie run longer than a tile"
        assert counts.min() > C.CHUNK
    assert any(c.n >= 16384 for c in _cases("few")) and any(c.n > C.TILE for c in _cases("equal"))
    for c in _cases("ramp"):
        p = C.keys(c)
        assert np.array_equal(p[1:], np.nextafter(p[:-1], np.float32(np.inf)))
        for image in (C.parent_image(p), C.fixed_image(p)):
            first = image[: C.GROUP]
            assert len(np.unique(first & U32(255))) == C.GROUP == 64 and len(np.unique(first >> 8)) == 1, "64 low bytes, one value of the other three"
            assert len(np.unique(image >> 8)) == -(-c.n // 256)
    for c in _cases("top-byte"):
        u = C.bits(C.keys(c))
        assert len(np.unique(u & U32(0x00FFFFFF))) == 1 and len(np.unique(u >> 24)) > min(c.n, 200) // 2
        assert (u >> 31).any() and not (u >> 31).all()
        m, e = np.frexp(C.keys(c).astype(np.float64))
        assert (np.abs(m) == 0.5).all(), "powers of two"
    special = np.array([0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x00800000, 0x80800000, C.TINY, C.TINY | 0x80000000, C.DENORM_MAX,
                        C.DENORM_MAX | 0x80000000], np.int64).astype(U32)
    for c in _cases("extremes"):
        p = C.keys(c)
        assert np.isin(special, C.bits(p)).all() and not np.isnan(p).any() and not (p == 0).any()
        assert np.isfinite(p).sum() > c.n // 2
    for c in _cases("zeros"):
        u = C.bits(C.keys(c))
        pos, neg = np.flatnonzero(u == 0), np.flatnonzero(u == U32(0x80000000))
        assert len(pos) and len(neg) and neg[0] < pos[-1], "a -0.0 in front of a +0.0: index order and the raw bits disagree"
        assert c.n < 64 or (min(len(pos), len(neg)) > c.n // 5 and len(pos) + len(neg) < c.n * 4 // 5)
        assert c.n < 64 or ((C.keys(c) > 0).any() and (C.keys(c) < 0).any())
    for c in _cases("nans"):
        u = C.bits(C.keys(c))
        nan = C.is_nan_bits(u)
        assert np.array_equal(nan, np.isnan(C.keys(c)))
        assert c.n < 63 or 0.1 < nan.mean() < 0.5
        assert c.n < 63 or (set(u[nan].tolist()) == set(C.NAN_BITS) and np.isfinite(C.keys(c)[~nan]).mean() > 0.9)
        if c.n >= 63:
            first_nan, ninf = np.flatnonzero(nan)[0], np.flatnonzero(u == U32(0xFF800000))
            assert len(ninf) and first_nan < ninf[-1] and (u == U32(0x7F800000)).any(), "a NaN in front of a -inf: an image that ties the two is caught"
            tied = np.where(nan, U32(0xFF800000), C.parent_image(C.keys(c)))
            assert not np.array_equal(C.order_by(tied), C.yardstick(C.keys(c)))
        assert (u[nan] >> 31).any() and not (u[nan] >> 31).all(), "NaNs of both signs"
    for c in _cases("all-nan"):
        u = C.bits(C.keys(c))
        assert C.is_nan_bits(u).all() and (c.n < 63 or len(np.unique(u)) == len(C.NAN_BITS))
        assert np.array_equal(C.yardstick(C.keys(c)), np.arange(c.n))


def test_poison_outranks_ordinary_keys():
    """The keys the GPU tests park at and past n_live: +inf and 3e38 would rank ahead of ordinary keys if the sort read them, and a NaN would turn up
    as an index at or past n_live wherever it landed."""
    q = C.poison(8)
    assert np.isnan(q).sum() == 4 and np.isposinf(q).sum() == 2 and (q[np.isfinite(q)] > 2.9e38).all()
    assert (C.bits(q)[[1, 2]] >> 31).tolist() == [0, 1], "NaNs of both signs"


def test_keys_are_reproducible():
    for c in C.CASES[:: 7]:
        assert np.array_equal(C.bits(C.keys(c)), C.bits(C.keys(c)))
