"""The cases of tests/test_rank_envelope_gpu.py: key populations x live sizes for the descending radix sort behind srlx_rank_select
(csrc/srlx_rank.hip), the yardstick, and numpy emulations of the sort's key image -- the one of this commit's parent and the fixed one -- with
which tests/test_rank_envelope_cpu.py proves, without a GPU, that the NaN and signed-zero cases tell the two apart.

The kernel's geometry: a workgroup sorts a tile of 4096 keys as four waves of 1024 contiguous keys, each walked in groups of 64; one workgroup
scans the 256 x workgroups histogram 1024 entries at a time.  SIZES sits on and one either side of every one of those borders."""
from collections import namedtuple

import numpy as np

F32, U32 = np.float32, np.uint32
CAPACITY = 25_000  # the one handle of the GPU tests; every live size is below it
TILE, CHUNK, GROUP = 4096, 1024, 64
SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 16384, 16385, 20481)
# 16384: four workgroups, 1024 histogram entries, exactly one scan round; 16385: five, 1280 entries, the second round runs with its carry;
# 20481: six workgroups, the last tile holds one key

NAN_BITS = (0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF, 0x7FC12345, 0xFFABCDEF)  # both signs, quiet and signalling, payloads
TINY, DENORM_MAX = 0x00000001, 0x007FFFFF  # smallest and largest denormal (bit patterns)
FLT_MAX, FLT_MIN = np.finfo(F32).max, np.finfo(F32).tiny


def _from_bits(bits):
    return np.asarray(bits, np.int64).astype(U32).view(F32)


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


def is_nan_bits(u):
    return (u & U32(0x7FFFFFFF)) > U32(0x7F800000)


# ---- populations: (n, rng) -> float32 [n] ------------------------------------------------------------------------------------------------------------------------
def _distinct(n, rng):
    """Distinct floats of both signs (a shuffled ramp of thirds, no zero among them)."""
    return ((rng.permutation(n).astype(np.float64) - n // 2 + 0.25) / 3).astype(F32)


def _equal(n, rng):
    return np.full(n, 1.5, F32)


def _few(n, rng):
    """Three values: tie runs of about n / 3 keys that cross wave, tile and workgroup borders."""
    return rng.choice(np.array([-2.5, 0.5, 7.0], F32), n)


def _ramp(n, rng):
    """np.nextafter steps up from 1.0 in index order: neighbouring keys differ in the lowest byte only."""
    return _from_bits(0x3F800000 + np.arange(n))


def _top_byte(n, rng):
    """+-2^k with the exponent field odd: mantissa 0 and bit 23 set in every key, so keys differ in bits 24..31 only."""
    e = 2 * rng.integers(0, 127, n) + 1  # exponent fields 1, 3 .. 253
    return _from_bits((rng.integers(0, 2, n) << 31) | (e << 23))


def _extremes(n, rng):
    """+-inf, the largest and smallest normals and denormals of both signs, among ordinary keys of both signs."""
    special = np.concatenate([np.array([np.inf, -np.inf, FLT_MAX, -FLT_MAX, FLT_MIN, -FLT_MIN], F32),
                              _from_bits([TINY, TINY | 0x80000000, DENORM_MAX, DENORM_MAX | 0x80000000, 2, 0x80000002])])
    p = rng.standard_normal(n).astype(F32)
    take = rng.random(n) < 0.4
    p[take] = rng.choice(special, int(take.sum()))
    p[: min(n, len(special))] = special[: min(n, len(special))]  # every one of them at least once
    return rng.permutation(p) if n > len(special) else p


def _zeros(n, rng):
    """Zeros of both signs, a third of the keys each way, among small keys of both signs (denormals included).  Slot 0 is -0.0 and slot 1 is +0.0."""
    other = np.concatenate([rng.standard_normal(n).astype(F32)[: n - n // 2], _from_bits(rng.integers(1, 9, n // 2) | (rng.integers(0, 2, n // 2) << 31))])
    p = rng.permutation(other)
    kind = rng.integers(0, 3, n)
    p[kind == 0] = F32(0.0)
    p[kind == 1] = -F32(0.0)
    p[0] = -F32(0.0)
    if n > 1:
        p[1] = F32(0.0)
    return p


def _nans(n, rng):
    """A quarter NaNs of both signs and several payloads, scattered among finite keys of both signs and a few infinities.  Slot 0 is -NaN, slot 1 is +NaN
    and, where there is room, slot 2 is -inf and slot 3 +inf: a NaN image that only TIES with -inf's would leave slot 0 in front of slot 2."""
    p = (rng.standard_normal(n) * 3).astype(F32)
    u = rng.random(n)
    p[u < 0.25] = _from_bits(rng.choice(np.array(NAN_BITS, np.int64), int((u < 0.25).sum())))
    p[u > 0.98] = rng.choice(np.array([np.inf, -np.inf], F32), int((u > 0.98).sum()))
    head = _from_bits([NAN_BITS[1], NAN_BITS[0], 0xFF800000, 0x7F800000])
    p[: min(n, 4)] = head[: min(n, 4)]
    return p


def _all_nan(n, rng):
    p = _from_bits(rng.choice(np.array(NAN_BITS, np.int64), n))
    head = _from_bits([NAN_BITS[1], NAN_BITS[0]])
    p[: min(n, 2)] = head[: min(n, 2)]
    return p


Population = namedtuple("Population", "name make sizes moves why")
# moves: the parent's key image orders this population differently from numpy (what the fix is for)
POPULATIONS = (
    Population("distinct", _distinct, SIZES, False, "the geometry sweep: every border of group, wave chunk, tile and scan round with nothing else in the way"),
    Population("equal", _equal, (1, 64, 65, 1025, 4096, 4097, 16385, 20481), False,
               "one digit bucket takes every key in all four passes; all 64 lanes of a group are peers; stability alone decides the order"),
    Population("few", _few, (4097, 16384, 16385, 20481), False, "tie runs of thousands of keys across wave, tile and workgroup borders"),
    Population("ramp", _ramp, (64, 65, 1024, 4097, 16385), False, "64 different digits per group in pass 0, one digit in passes 1 to 3 up to 256-key steps"),
    Population("top-byte", _top_byte, (63, 1025, 4096, 20481), False, "passes 0 to 2 must leave the order alone; pass 3 alone sorts, sign byte included"),
    Population("extremes", _extremes, (63, 1023, 4095, 16384), False, "both ends of the image: +-inf, +-FLT_MAX, +-FLT_MIN, denormals next to the zero crossing"),
    Population("zeros", _zeros, (2, 64, 1025, 4097, 16385), True, "-0.0 == +0.0: they tie and keep index order"),
    Population("nans", _nans, (2, 63, 1024, 4097, 16385, 20481), True, "NaN of either sign and any payload ranks behind -inf, in index order"),
    Population("all-nan", _all_nan, (2, 65, 4096, 16385), True, "nothing but NaNs: the identity order"),
)
BY_NAME = {p.name: p for p in POPULATIONS}
Case = namedtuple("Case", "population n")
CASES = tuple(Case(p.name, n) for p in POPULATIONS for n in p.sizes)
CASE_IDS = tuple(f"{c.population}-{c.n}" for c in CASES)


def keys(case):
    """The case's float32 priorities (a fresh array, the same on every call)."""
    pop = BY_NAME[case.population]
    seed = [i for i, p in enumerate(POPULATIONS) if p.name == pop.name][0] * 100_003 + case.n
    p = pop.make(case.n, np.random.default_rng(seed))
    assert p.dtype == F32 and p.shape == (case.n,)
    return p


def poison(n):
    """What the slots at and past n_live hold in the GPU tests: priorities that would rank ahead of ordinary live ones, or show as an index past n_live, if the sort read them (+inf, +NaN, -NaN, 3e38)."""
    return np.resize(_from_bits([0x7F800000, NAN_BITS[0], NAN_BITS[5], 0x7F61B1E6]), n)


# ---- the yardstick and the two key images ------------------------------------------------------------------------------------------------------------------------
def yardstick(p):
    """The whole order: np.argsort(-p, kind="stable") -- numpy's order for distinct keys, NaN last, index order among ties (include/srlx.h)."""
    return np.argsort(-np.asarray(p, F32), kind="stable")


def parent_image(p):
    """desc_image of this commit's parent: the order-preserving integer image of the raw bits, complemented."""
    u = bits(p)
    asc = np.where(u & U32(0x80000000), ~u, u | U32(0x80000000))
    return ~asc


def fixed_image(p):
    """This commit's: -0.0 folded into +0.0 before the image, every NaN on the one image behind -inf's."""
    u = bits(p).copy()
    u[(u & U32(0x7FFFFFFF)) == 0] = 0
    return np.where(is_nan_bits(u), U32(0xFFFFFFFF), parent_image(u.view(F32)))


def order_by(image):
    """What a stable LSD radix sort of (image, index) pairs leaves: ascending image, index order among equal images."""
    return np.argsort(image, kind="stable")
