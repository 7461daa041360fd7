"""The wave and row reductions of the DPP network (csrc/pf_dpp.h), bit for bit.

Every filter kernel's sums and maxima go through one fixed pairing tree:

    quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror   (inside each 16-lane row)
    row_bcast:15 on rows 1 and 3, row_bcast:31 on rows 2 and 3, lane 63    (across the rows)

and the filters' outputs are compared byte for byte between builds, so the tree is part of the
contract: a stage in another order, a stage combining other lanes or a zero of the other sign
changes the last bits of a step's record.  ``pf_test_wave_reduce`` runs ``wave_max_u``,
``wave_sum_u``, ``wave_sum_prod_u3``, ``wave_sum_ud``, ``wave_max_ud`` and, in all 64 lanes,
``row_max_f`` / ``row_sum_f`` / ``row_sum_d`` on given lanes, one 64-lane workgroup per case.  The
expected values come from a NumPy restatement of the tree (below) in float32 / float64 and are
compared as integers, so the sign of a zero counts.  No NaN and no subnormal occurs in a case, so the
denormal mode is not what is tested.
"""

import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from particle_filters_amd import _native as NV

LANES = np.arange(64)
# source lane of every lane, and the lanes written, per stage
STAGES = (
    (LANES ^ 1, np.ones(64, bool)),                                  # quad_perm [1,0,3,2]
    (LANES ^ 2, np.ones(64, bool)),                                  # quad_perm [2,3,0,1]
    ((LANES & ~7) | (7 - (LANES & 7)), np.ones(64, bool)),           # row_half_mirror
    ((LANES & ~15) | (15 - (LANES & 15)), np.ones(64, bool)),        # row_mirror
    ((LANES & ~15) - 1, ((LANES >> 4) & 1) == 1),                    # row_bcast:15, rows 1 and 3
    (np.full(64, 31), (LANES >> 4) >= 2),                            # row_bcast:31, rows 2 and 3
)


def fmax(a, b):
    """The hardware maximum of two non-NaN values: +0 is above -0."""
    return np.where((a > b) | ((a == b) & ~np.signbit(a)), a, b)


def fadd(a, b):
    return a + b  # arrays of one dtype: IEEE round to nearest in that dtype


def tree(v, op, stages=STAGES, n=6):
    """The first n stages on 64 lanes: an enabled lane i gets op(v[src[i]], v[i]), the others keep v[i]."""
    v = np.array(v)
    assert v.shape == (64,) and v.dtype in (np.float32, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        for src, on in stages[:n]:
            v = np.where(on, op(v[np.where(on, src, LANES)], v), v).astype(v.dtype)
    return v


def wave(v, op, stages=STAGES):
    return tree(v, op, stages)[63]


def row(v, op, stages=STAGES):
    return tree(v, op, stages, 4)


def round_f32(q):
    """A rational number rounded once to float32 (nearest, ties to even; normal range)."""
    if q == 0:
        return np.float32(0.0)
    e = abs(q).numerator.bit_length() - abs(q).denominator.bit_length()
    if Fraction(2) ** e > abs(q):
        e -= 1
    assert -126 <= e <= 127 and Fraction(2) ** e <= abs(q) < Fraction(2) ** (e + 1)
    ulp = Fraction(2) ** (e - 23)
    n, r = divmod(abs(q), ulp)
    n = int(n) + (r > ulp / 2 or (r == ulp / 2 and int(n) % 2 == 1))
    return np.float32(float(n * ulp) * (1 if q > 0 else -1))  # n ulp has 25 bits at most: exact as a double


def wave_prod(a, b):
    """wave_sum_prod_u3's tree for a[i] * b: the first stage adds the partner's rounded product to
    the lane's own unrounded one, fma(a, b, p[i ^ 1]) with one rounding; the rest is the plain tree."""
    b = np.float32(b)
    p = (a * b).astype(np.float32)
    first = np.empty(64, np.float32)
    for i in range(64):
        t = p[i ^ 1]
        if np.isfinite(a[i]) and np.isfinite(t):
            q = Fraction(float(a[i])) * Fraction(float(b)) + Fraction(float(t))
            # an exact zero takes the sign of the sum of its zero terms (both round to nearest)
            first[i] = round_f32(q) if q != 0 else np.float32(float(a[i]) * float(b)) + t
        else:
            first[i] = p[i] + t
    return tree(first, fadd, STAGES[1:], 5)[63]


def cases():
    """[ncases][64] float64 values, every one exactly representable in float32."""
    rng = np.random.default_rng(20240607)

    def wide():  # magnitudes from 2^-60 to 2^60, mixed signs
        m = 1.0 + rng.integers(0, 1 << 23, 64) / float(1 << 23)
        return rng.choice([-1.0, 1.0], 64) * np.ldexp(m, rng.integers(-60, 61, 64))

    def close():  # magnitudes within a factor of 16: every add rounds, so every pairing shows
        m = 1.0 + rng.integers(0, 1 << 23, 64) / float(1 << 23)
        return rng.choice([-1.0, 1.0], 64) * np.ldexp(m, rng.integers(-2, 3, 64))

    out = [close(), close(), close(), close(), wide(), wide()]
    one = np.full(64, -np.inf)  # every lane -inf but one
    one[37] = 1.5
    out.append(one)
    r = wide()  # a whole row of -inf
    r[32:48] = -np.inf
    out.append(r)
    out.append(np.where(LANES % 3 == 0, -0.0, 0.0))  # zeros of both signs
    out.append(np.full(64, -0.0))  # only negative zeros: the sum and the maximum stay -0
    z = np.full(64, -0.0)
    z[63] = 0.0
    out.append(z)
    out.append(LANES.astype(np.float64))  # ramps
    out.append((0.1 * (LANES - 20.0)).astype(np.float32).astype(np.float64))
    return np.array(out)


def bits(a):
    a = np.asarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def test_restatement_tells_a_permuted_tree_apart():
    """The restatement against itself: the same stages in another order, and a tree that pairs other
    lanes, give other bits on the case of close magnitudes, so a kernel that did either would fail below."""
    close = cases()[:4]
    v32, v64 = close[0].astype(np.float32), close[0] * (1.0 + 2.0 ** -40)
    swapped = (STAGES[2], STAGES[3], STAGES[0], STAGES[1]) + STAGES[4:]
    shifted = ((LANES ^ 3, STAGES[0][1]),) + STAGES[1:]
    for other in (swapped, shifted):
        # a wave's sum survives a regrouping about every other time (the last rounding absorbs it): some of
        # the four cases must show it, and the rows' 64 results do every time
        for scale, dtype in ((1.0, np.float32), (1.0 + 2.0 ** -40, np.float64)):
            vs = [(c * scale).astype(dtype) for c in close]
            assert sum(bits(wave(v, fadd)) != bits(wave(v, fadd, other)) for v in vs) >= 2
        assert np.any(bits(row(v32, fadd)) != bits(row(v32, fadd, other)))
        assert np.any(bits(row(v64, fadd)) != bits(row(v64, fadd, other)))
    # the maximum does not depend on the order, the sign of its zero does on the operation
    z = np.where(LANES % 3 == 0, -0.0, 0.0).astype(np.float32)
    assert bits(wave(z, fmax)) == bits(np.float32(0.0)) and bits(wave(-np.abs(z), fmax)) == bits(np.float32(-0.0))
    assert bits(wave(z, fadd)) == bits(np.float32(0.0)) and bits(wave(-np.abs(z), fadd)) == bits(np.float32(-0.0))
    # the fused first stage of the product sums is not the sum of the rounded products
    assert bits(wave_prod(v32, 0.7)) != bits(wave((v32 * np.float32(0.7)).astype(np.float32), fadd))
    assert bits(wave_prod(v32, 1.0)) == bits(wave(v32, fadd))
    assert bits(round_f32(Fraction(1) + Fraction(1, 1 << 24))) == bits(np.float32(1.0))  # tie to even
    assert bits(round_f32(Fraction(1) + Fraction(3, 1 << 25))) == bits(np.float32(1.0 + 2.0 ** -23))
    # every lane of a row holds the row's result after the four row stages
    r = row(v32, fadd).reshape(4, 16)
    assert np.all(bits(r) == bits(r[:, :1]))


@pytest.fixture(scope="module")
def device_results():
    cs = cases()
    n = len(cs)
    in_f = np.ascontiguousarray(cs, dtype=np.float32)
    assert np.array_equal(in_f.astype(np.float64), cs, equal_nan=False)
    in_d = np.ascontiguousarray(np.where(np.isfinite(cs), cs * (1.0 + 2.0 ** -40), cs))  # needs the fp64 mantissa
    out_f = np.full((n, 5 + 128), np.nan, dtype=np.float32)
    out_d = np.full((n, 2 + 64), np.nan, dtype=np.float64)
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    NV.check(NV.load().pf_test_wave_reduce(None, n, in_f.ctypes.data_as(fp), in_d.ctypes.data_as(dp),
                                           out_f.ctypes.data_as(fp), out_d.ctypes.data_as(dp)), "pf_test_wave_reduce")
    return in_f, in_d, out_f, out_d


@pytest.mark.gpu
def test_wave_reductions_fp32_match_the_tree_bit_for_bit(device_results):
    in_f, _, out_f, _ = device_results
    for k, v in enumerate(in_f):
        want = [wave(v, fmax), wave(v, fadd), wave_prod(v, 0.7), wave_prod(-v, 1.3), wave_prod(v, 3.0)]
        got = out_f[k, :5]
        assert np.array_equal(bits(got), bits(np.array(want, np.float32))), (k, got, want)


@pytest.mark.gpu
def test_row_reductions_fp32_hold_in_every_lane(device_results):
    in_f, _, out_f, _ = device_results
    for k, v in enumerate(in_f):
        assert np.array_equal(bits(out_f[k, 5:69]), bits(row(v, fmax))), (k, "row_max_f")
        assert np.array_equal(bits(out_f[k, 69:133]), bits(row(v, fadd))), (k, "row_sum_f")


@pytest.mark.gpu
def test_reductions_fp64_match_the_tree_bit_for_bit(device_results):
    _, in_d, _, out_d = device_results
    for k, v in enumerate(in_d):
        want = np.array([wave(v, fadd), wave(v, fmax)])
        assert np.array_equal(bits(out_d[k, :2]), bits(want)), (k, out_d[k, :2], want)
        assert np.array_equal(bits(out_d[k, 2:]), bits(row(v, fadd))), (k, "row_sum_d")
