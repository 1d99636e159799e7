"""tests/ranking_ref.py checked on the host: the restatement the GPU ranking tests compare with has to be right by itself.
fma32 is held to exact rational arithmetic, the chain to the float64 dot product within its forward bound, the ranking
order to a row written out by hand."""
from fractions import Fraction

import numpy as np

from tests import ranking_ref as R


def _exact_fma32(a, b, c):
    """round-to-nearest-even float32 of the rational a * b + c (normal range)."""
    t = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if t == 0:
        return np.float32(0.0)
    sign, mag = (-1 if t < 0 else 1), abs(t)
    e = mag.numerator.bit_length() - mag.denominator.bit_length()
    if Fraction(2) ** e > mag:
        e -= 1                                                     # 2^e <= mag < 2^(e + 1)
    ulp = Fraction(2) ** (e - 23)
    q = mag / ulp
    lo = q.numerator // q.denominator
    rem = q - lo
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and lo % 2 == 1):
        lo += 1
    return np.float32(sign * float(lo * ulp))


def _triples():
    rng = np.random.default_rng(11)
    n = 3000
    a = rng.standard_normal(n).astype(np.float32)
    b = rng.standard_normal(n).astype(np.float32)
    c = (rng.standard_normal(n) * np.float32(2.0) ** rng.integers(-12, 12, n)).astype(np.float32)
    # cancellation: c close to -a * b
    c[:500] = -(a[:500] * b[:500]) * (1 + rng.integers(-3, 4, 500) * np.float32(2.0) ** -23)
    am, bm, cm = _midpoints(rng, 600)
    return np.concatenate([a, am]), np.concatenate([b, bm]), np.concatenate([c, cm])


def _midpoints(rng, n):
    """c in [1, 2) (ulp 2^-23) and a * b = +-(2^-24 - 2^-70): half an ulp of c less a residual far below float64's ulp of
    the sum (2^-52).  fl64(a * b + c) is then EXACTLY the float32 midpoint next to c, the true sum is on c's side of it, and
    the answer is c; rounding the float64 sum to float32 goes to the even neighbour instead, wrong for every odd c."""
    c = (1 + (1 + rng.integers(0, 2 ** 23 - 2, n)) * 2.0 ** -23).astype(np.float32)
    sign = np.where(rng.integers(0, 2, n) == 0, 1.0, -1.0)
    a = (sign * 2.0 ** -24 * (1 + 2.0 ** -23)).astype(np.float32)            # (1 + 2^-23)(1 - 2^-23) = 1 - 2^-46
    b = np.full(n, 1 - 2.0 ** -23, dtype=np.float32)
    return a, b, c


def test_fma32_is_correctly_rounded():
    a, b, c = _triples()
    got = R.fma32(a, b, c)
    assert got.dtype == np.float32
    want = np.array([_exact_fma32(x, y, z) for x, y, z in zip(a, b, c)], dtype=np.float32)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


def test_fma32_midpoint_with_a_residual_is_not_rounded_twice():
    a, b, c = _midpoints(np.random.default_rng(3), 400)
    s64 = a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)
    assert ((s64.view(np.int64) & 0x1FFFFFFF) == 0x10000000).all()             # the float64 sums ARE midpoints
    twice = s64.astype(np.float32)
    assert 100 < (twice != c).sum() < 300                                       # ... and rounding them again is wrong for the odd c
    got = R.fma32(a, b, c)
    assert np.array_equal(got, c)
    assert np.array_equal(R.fma32(-a, b, -c), -c)                               # mirrored about zero
    # no residual: the true sum IS the midpoint, ties go to even
    half = np.full(400, 2.0 ** -24, dtype=np.float32)
    one = np.ones(400, dtype=np.float32)
    tie = R.fma32(half, one, c)
    even = (c.view(np.int32) & 1) == 0
    assert np.array_equal(tie, np.where(even, c, np.nextafter(c, np.float32(4.0))))


def test_chain_scores_against_the_float64_dot_product():
    rng = np.random.default_rng(5)
    for d in (32, 64, 128, 256):
        U = (rng.standard_normal((37, d)) * 0.3).astype(np.float32)
        I = (rng.standard_normal((91, d)) * 0.3).astype(np.float32)
        I[7] *= 40.0
        U[3] = 0.0
        got = R.chain_scores(U, I, block=16)
        assert got.dtype == np.float32 and got.shape == (37, 91)
        want = U.astype(np.float64) @ I.astype(np.float64).T
        bound = d * 2.0 ** -24 * (np.abs(U).astype(np.float64) @ np.abs(I).astype(np.float64).T)
        assert (np.abs(got - want) <= bound).all()
        assert (got[3] == 0).all()
    # the ORDER is the documented one: a row whose halves cancel differently in any other order
    u = np.zeros((1, 4), dtype=np.float32); i = np.ones((1, 4), dtype=np.float32)
    u[0] = [2.0 ** 24, 1.0, -2.0 ** 24, 1.0]                     # dims 0, 2, 1, 3:  2^24 - 2^24 + 1 + 1 = 2
    assert R.chain_scores(u, i)[0, 0] == 2.0                       # (0, 1, 2, 3 would give 2^24 + 1 -> 2^24, - 2^24, + 1 = 1)


def test_rank_orders_by_score_then_id():
    row = np.array([[0.5, 2.0, -1.0, 2.0, 0.5, 0.5, -np.inf, 3.0]], dtype=np.float32)
    ids, sc = R.rank(row, 8)
    assert ids.dtype == np.int32 and sc.dtype == np.float32
    assert ids.tolist() == [[7, 1, 3, 0, 4, 5, 2, 6]]
    assert sc.tolist() == [[3.0, 2.0, 2.0, 0.5, 0.5, 0.5, -1.0, -np.inf]]
    ids3, sc3 = R.rank(np.vstack([row, -row]), 3)
    assert ids3.tolist() == [[7, 1, 3], [6, 2, 0]] and sc3[1].tolist() == [np.inf, 1.0, -0.5]


def test_masked_hit_flags_and_trim_mark():
    scores = np.arange(12, dtype=np.float32).reshape(2, 6)
    indptr = np.array([0, 0, 2, 3]); indices = np.array([1, 5, 9])
    out = R.masked(scores, [2, 1], indptr, indices)                # (user 2's item 9 is beyond a 6-item slice)
    assert out[0].tolist() == scores[0].tolist()
    assert out[1].tolist() == [6.0, -1e9, 8.0, 9.0, 10.0, -1e9] and scores[1, 1] == 7.0
    flags = R.hit_flags(np.array([[1, 5, 2], [9, 0, 1]]), [1, 2], indptr, indices)
    assert flags.tolist() == [[1, 1, 0], [1, 0, 0]]
    assert R.hit_flags(np.array([[1, 5]]), None, indptr, indices).tolist() == [[0, 0]]
    ids, sc = R.trim_mark_ties(np.array([[4, 2, 9], [4, 2, 9], [4, 2, 9]]),
                               np.array([[3.0, 3.0, 1.0], [3.0, 1.0, 1.0], [3.0, 2.0, 1.0]], dtype=np.float32))
    assert ids.tolist() == [[-5, 2], [-5, 2], [4, 2]] and sc.tolist() == [[3.0, 3.0], [3.0, 1.0], [3.0, 2.0]]
