"""The kernel cases of SEPT's tests -- TEST INFRASTRUCTURE ONLY.  tests/test_gpu_sept.py runs the kernels on them;
tests/test_sept_cpu.py measures how many of their top-k cuts are too close for float32 to call.  Every case and its float64
restatement is computed once (lru_cache) and never modified."""
import functools

import numpy as np

from tests import sept_ref

TAU = 0.1                                     # SEPT.py:131-132 hard-codes it
AMBIGUOUS_GAP = 1e-4                          # ~25x the worst-case fp32 dot error d * 2^-24 ~ 4e-6 at d = 64
AMBIGUOUS_SHARE = 0.05
LOSS_BOUND, GRAD_BOUND = 1e-5, 1e-4           # README's standing tolerances: relative; of the matrix's largest magnitude

# (n, d, k, seed, clean): clean = no (pair, row) of the case is ambiguous
TRI_ND_CASES = [
    (10, 64, 10, 0, True),                    # n == k: every j is a positive
    (11, 64, 10, 0, True),
    (11, 64, 10, 1, True),
    (33, 64, 10, 1, True),
    (97, 64, 10, 0, False),                   # two row tiles, a ragged second one
    (131, 128, 10, 0, False),                 # the 128-wide instantiation
    (64, 64, 32, 0, False),                   # the longest list, one exact tile
    (300, 64, 10, 0, False),
    (1030, 64, 10, 0, False),                 # several pass-1 key chunks, the last one ragged
    (40, 48, 1, 0, False),                    # zero-padded by the wrapper, k = 1
]
L2NORM_SHAPES = [(1, 1), (5, 3), (67, 64), (130, 100), (33, 256)]


def case_id(c):
    return "n%d_d%d_k%d_s%d" % c[:4]


def draw(n, d, seed):
    """F, S, R, A in that order from default_rng(seed), each standard_normal((n, d)) cast to float32"""
    rng = np.random.default_rng(seed)
    return tuple(rng.standard_normal((n, d)).astype(np.float32) for _ in range(4))


@functools.lru_cache(maxsize=None)
def tri_nd_case(case):
    n, d, k, seed, _clean = case
    mats = draw(n, d, seed)
    ref = sept_ref.tri_nd(*mats, k, TAU)
    return dict(mats=mats, ref=ref, amb=sept_ref.ambiguous(ref["gap"], AMBIGUOUS_GAP))


@functools.lru_cache(maxsize=None)
def l2norm_case(shape):
    """rows of every kind: ordinary ones, a zero row and a row whose squared norm is below the clamp (the last two share a
    row when n == 1 cannot hold both: then the row is below the clamp and the zero row is checked by the next shape)"""
    n, d = shape
    rng = np.random.default_rng(1000 * n + d)
    y = rng.standard_normal((n, d)).astype(np.float32)
    g = rng.standard_normal((n, d)).astype(np.float32)
    y[n - 1] = (1e-8 * rng.standard_normal(d)).astype(np.float32)      # squared norm ~ d * 1e-16 < 1e-12
    if n > 1:
        y[n // 2 - (1 if n // 2 == n - 1 else 0)] = 0.0
    out, inv, clamped = sept_ref.l2norm(y)
    return dict(y=y, g=g, out=out, inv=inv, clamped=clamped, gy=sept_ref.l2norm_bwd(g, out, inv, clamped))
