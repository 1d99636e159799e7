"""The kernel cases of SEPT's tests -- TEST INFRASTRUCTURE ONLY.  tests/test_gpu_sept.py and tests/test_gpu_sept_edges.py
run the kernels on them; tests/test_sept_cpu.py measures how many of their top-k cuts are too close for float32 to call.
Every case and its float64 restatement is computed once (lru_cache) and never modified."""
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
L2NORM_SHAPES = [(1, 1), (5, 3), (67, 64), (130, 100), (33, 256),
                 # lane c owns columns c, c + 64, c + 128, c + 192: either side of every lane quarter; 4 and 8 rows fill
                 # one and two workgroups exactly
                 (4, 63), (8, 65), (6, 127), (7, 128), (9, 129), (5, 192), (3, 193), (2, 255)]

# ---- the edge cases: input families x the shapes at which sept.hip takes another path ------------------
FAMILIES = ("normal", "scaled", "clamped", "peaked")
# (n, d, k, seed)
EDGE_SHAPES = [
    (33, 64, 10, 0),                          # one ragged tile; the smallest n that holds the planted rows
    (48, 64, 10, 0),                          # three exact 16-key sub-tiles: tn_select's early break taken at the edge
    (49, 64, 10, 0),                          # one key past a 16-key sub-tile: a scan of one key, no break
    (63, 64, 10, 0),                          # the last full tile minus one
    (64, 64, 32, 0),                          # one exact tile, the full LDS list
    (65, 64, 10, 0),                          # one row and one key in the second tile; three mask words (w + 1 == words)
    (65, 64, 32, 0),                          # the same, ragged, with the full LDS list
    (97, 64, 10, 0),                          # a second tile of 33 keys: its second mask word exists and holds one key
    (128, 64, 10, 0),                         # two exact tiles, an even word count
    (129, 128, 10, 0),                        # one key in the third tile, d = 128
    (131, 128, 10, 0),
    (300, 64, 10, 0),
    (833, 128, 10, 0),                        # 14 tiles, 13 chunks of 128 keys: six empty pass-1 chunks; d = 128 chunked
    (1030, 64, 10, 0),                        # 17 tiles, 11 chunks of 128 keys: nine live (the last of 6 keys), two empty
    (40, 48, 1, 0),                           # padded to 64 by the wrapper, k = 1
    (33, 100, 10, 0),                         # padded to 128: a width between 65 and 127
    (33, 8, 10, 0),                           # padded to 64 from 8 columns
]
PLANT_MIN_N = 33


def edge_id(c):
    return "n%d_d%d_k%d_s%d-%s" % (*c[0], c[1])


def edge_cases(families=FAMILIES):
    return [(shape, fam) for shape in EDGE_SHAPES for fam in families]


def case_id(c):
    return "n%d_d%d_k%d_s%d" % c[:4]


def draw(n, d, seed):
    """F, S, R, A in that order from default_rng(seed), each standard_normal((n, d)) cast to float32"""
    rng = np.random.default_rng(seed)
    return tuple(rng.standard_normal((n, d)).astype(np.float32) for _ in range(4))


def row_scales(n, seed):
    """the `scaled` family's factors: (4, n) float64, 10**u with u uniform in [-3, 3] per matrix (F, S, R, A) and row"""
    return 10.0 ** np.random.default_rng(seed + 777).uniform(-3.0, 3.0, (4, n))


def planted_rows(n):
    """the `clamped` family's rows per matrix (F, S, R, A): (the zero row, the row of 1e-8 * standard_normal) -- ten
    distinct indices, so no user is degenerate in two matrices"""
    assert n >= PLANT_MIN_N
    return ((0, n - 1), (n // 2, 5), (6, 7), (8, 9))


def family(name, n, d, seed):
    """(F, S, R, A) float32 of one input family, each starting from draw(n, d, seed):
    normal   draw unchanged (every row norm about sqrt(d))
    scaled   every row of every matrix times its own 10**u (row_scales): the same ids and losses, gradients x 10**-u
    clamped  normal with a zero row and a row of squared norm about d * 1e-16 (far below the 1e-12 clamp) per matrix
    peaked   F, S, R = A + 0.3 * (their own draw): s_ii about 0.96, the softmax at tau = 0.1 peaked on the diagonal"""
    F, S, R, A = draw(n, d, seed)
    if name == "normal":
        return F, S, R, A
    if name == "scaled":
        sc = row_scales(n, seed)
        return tuple((m.astype(np.float64) * sc[i][:, None]).astype(np.float32) for i, m in enumerate((F, S, R, A)))
    if name == "clamped":
        rng = np.random.default_rng(seed + 778)
        out = []
        for m, (zero, tiny) in zip((F, S, R, A), planted_rows(n)):
            m = m.copy()
            m[zero] = 0.0
            m[tiny] = (1e-8 * rng.standard_normal(d)).astype(np.float32)
            out.append(m)
        return tuple(out)
    if name == "peaked":
        return tuple((A + np.float32(0.3) * m).astype(np.float32) for m in (F, S, R)) + (A,)
    raise ValueError(name)


@functools.lru_cache(maxsize=None)
def edge_case(shape, fam):
    """one (shape, family): the inputs, the float64 restatement, its ambiguous (pair, row)s and, per (pair, row), the
    k + 1 best keys in order (what the order check of the ids reads)"""
    n, d, k, seed = shape
    mats = family(fam, n, d, seed)
    ref = sept_ref.tri_nd(*mats, k, TAU)
    top = -np.sort(-ref["key"], axis=2)[:, :, :k + 1]
    return dict(mats=mats, ref=ref, amb=sept_ref.ambiguous(ref["gap"], AMBIGUOUS_GAP), top=top)


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
