"""The kernel cases of MHCN's tests -- TEST INFRASTRUCTURE ONLY.  tests/test_gpu_mhcn.py and tests/test_gpu_mhcn_edges.py
run the kernels on them; tests/test_mhcn_cpu.py measures what plain float32 arithmetic loses on each (the yardstick).
Every case and its float64 restatement is computed once (lru_cache) and never modified.

The shapes sit on either side of every edge of csrc/mhcn.hip as built: 16 rows per wave and 64 per workgroup in the gate
kernels (15 / 16 / 17, 63 / 64 / 65, 129), kRowChunk = 256 rows per weight-gradient partial (256 / 257), kMixChunk = 64 rows
per partial of the mix and MIM reductions, four rows per workgroup of the one-wave-per-row kernels (1, 2, 3, 5), the lane
quarter at column 64 (d = 64 against 128 and the padded 100), and the wrapper's zero padding (48 -> 64, 100 -> 128,
8 -> 64)."""
import functools

import numpy as np

from tests import mhcn_ref

LOSS_BOUND, GRAD_BOUND, FWD_BOUND = 1e-5, 1e-4, 1e-5   # README's standing tolerances; forward: of the largest magnitude

NS = (1, 15, 16, 17, 63, 64, 65, 129)
WIDTHS = (64, 128, 48, 100, 8)

# (n, d, C)
GATE_CASES = [(n, 64, 4) for n in NS] + [(256, 64, 4), (257, 64, 4), (257, 128, 3), (513, 64, 1)] + \
    [(n, d, c) for d in WIDTHS[1:] for n, c in ((17, 1), (65, 3), (129, 4))] + [(64, 64, 1), (65, 64, 3), (16, 128, 1)]

# ((n, d), family, with the addend)
MIX_FAMILIES = ("normal", "equal", "ahead")
MIX_SHAPES = [(n, 64) for n in NS + (2, 3, 5, 128, 257)] + [(n, d) for d in WIDTHS[1:] for n in (17, 65, 129)]
MIX_CASES = [(s, f, x) for s in MIX_SHAPES for f in MIX_FAMILIES for x in (True, False)
             if f == "normal" or (s[0] in (1, 2, 17, 65, 129) and not (f == "ahead" and s[0] == 1))]

# ((n, d), family)
MIM_FAMILIES = ("normal", "identity", "large", "empty")
MIM_SHAPES = [(n, 64) for n in (1, 2, 3, 4, 5, 63, 64, 65, 257, 1030)] + \
    [(65, 128), (257, 128), (3, 48), (65, 100), (63, 8), (257, 48)]
MIM_CASES = [(s, f) for s in MIM_SHAPES for f in MIM_FAMILIES]


def gate_id(c):
    return "n%d_d%d_c%d" % c


def mix_id(c):
    return "n%d_d%d-%s-%s" % (*c[0], c[1], "x" if c[2] else "nox")


def mim_id(c):
    return "n%d_d%d-%s" % (*c[0], c[1])


def seed_of(*key):
    """a seed that is a function of the case alone"""
    return sum((i + 1) * 7919 * int(k) for i, k in enumerate(key))


@functools.lru_cache(maxsize=None)
def gate_case(case):
    n, d, c = case
    rng = np.random.default_rng(seed_of(n, d, c))
    x = (0.5 * rng.standard_normal((n, d))).astype(np.float32)
    w = (rng.standard_normal((c, d, d)) / np.sqrt(d)).astype(np.float32)
    b = (0.1 * rng.standard_normal((c, d))).astype(np.float32)
    gy = rng.standard_normal((c, n, d)).astype(np.float32)
    y, _ = mhcn_ref.gate(x, w, b)
    gx, gw, gb = mhcn_ref.gate_bwd(x, w, b, gy)
    return dict(x=x, w=w, b=b, gy=gy, y=y, gx=gx, gw=gw, gb=gb)


@functools.lru_cache(maxsize=None)
def mix_case(case):
    """normal  three independent channels
    equal   q is zero on the upper half of the columns and the channels differ there alone: the three scores of a row
            are equal in any precision, the softmax exactly 1/3, while the gradients of the three channels differ
    ahead   on every odd row r, channel r % 3 is moved along q until its score leads the other two by 30: a saturated
            softmax (the others are e^-30 ~ 1e-13, below float32's epsilon: that row's gradient through the softmax is
            nothing in either precision).  The even rows stay ordinary, so that dq has a magnitude to be held to."""
    (n, d), fam, with_x = case
    rng = np.random.default_rng(seed_of(n, d, MIX_FAMILIES.index(fam), int(with_x)))
    e = [(0.5 * rng.standard_normal((n, d))).astype(np.float32) for _ in range(3)]
    q = (0.3 * rng.standard_normal(d)).astype(np.float32)
    x = (0.5 * rng.standard_normal((n, d))).astype(np.float32) if with_x else None
    gout = rng.standard_normal((n, d)).astype(np.float32)
    if fam == "equal":
        q[d // 2:] = 0.0
        for t in e[1:]:
            t[:, :d // 2] = e[0][:, :d // 2]
    elif fam == "ahead":
        q64 = q.astype(np.float64)
        w = np.stack([t.astype(np.float64) @ q64 for t in e], axis=1)
        for r in range(1, n, 2):
            c = r % 3
            others = max(w[r][k] for k in range(3) if k != c)
            e[c][r] = (e[c][r].astype(np.float64) + (others + 30.0 - w[r][c]) * q64 / (q64 @ q64)).astype(np.float32)
    elif fam != "normal":
        raise ValueError(fam)
    beta = 0.5 if with_x else 0.0
    out, s = mhcn_ref.chan_mix(e, q, x, beta)
    ge, gx, gq = mhcn_ref.chan_mix_bwd(e, q, s, gout, beta)
    return dict(e=e, q=q, x=x, gout=gout, beta=beta, out=out, s=s, ge=ge, gx=gx, gq=gq)


def mim_inputs(shape, fam):
    """normal    entries of variance 0.7 / sqrt(d): the differences of two inner products are of order 1; random permutations
    identity  normal with every permutation the identity: every local difference is exactly 0, the loss 3 n log 2
    large     rows scaled until the differences are near +-40: float32 sigmoid saturates, -log(sigmoid) would overflow
    empty     normal with every third row of edge zero, as an empty row of H gives"""
    n, d = shape
    rng = np.random.default_rng(seed_of(n, d, MIM_FAMILIES.index(fam)))
    scale = np.sqrt(28.0 / np.sqrt(d)) if fam == "large" else np.sqrt(0.7 / np.sqrt(d))
    em = (scale * rng.standard_normal((n, d))).astype(np.float32)
    edge = (scale * rng.standard_normal((n, d))).astype(np.float32)
    perms = [rng.permutation(n) for _ in range(3)] + [rng.permutation(d) for _ in range(2)]
    if fam == "identity":
        perms = [np.arange(n)] * 3 + [np.arange(d)] * 2
    if fam == "empty":
        edge[::3] = 0.0
    return em, edge, tuple(p.astype(np.int32) for p in perms)


@functools.lru_cache(maxsize=None)
def mim_case(case):
    """-> em, edge, perms, the float64 restatement, and gscale: what an error of a gradient matrix is measured against --
    the matrix's largest magnitude, except in the identity family, whose exact gradients are zero matrices (every term
    k x meets its opposite): there the size of one such term, sigmoid(0) = 1/2 times the largest input magnitude"""
    shape, fam = case
    em, edge, perms = mim_inputs(shape, fam)
    ref = mhcn_ref.mim(em, edge, perms)
    if fam == "identity":
        term = 0.5 * float(max(np.abs(em).max(), np.abs(edge).max()))
        gscale = dict(gem=term, gedge=term)
    else:
        gscale = dict(gem=float(np.abs(ref["gem"]).max()), gedge=float(np.abs(ref["gedge"]).max()))
    return dict(em=em, edge=edge, perms=perms, ref=ref, gscale=gscale)


def mim_grad_error(case, name, got):
    """the largest error of a gradient matrix over its gscale (a zero matrix, as n = 1 of `empty` has, admits no error)"""
    c = mim_case(case)
    err = float(np.abs(np.asarray(got, dtype=np.float64) - c["ref"][name]).max())
    return err / c["gscale"][name] if c["gscale"][name] > 0 else (0.0 if err == 0 else np.inf)


# ---- the model step on the tiny graph ------------------------------------------------------------------------------------
STEP = dict(batch=256, emb=64, n_layer=2, ss_rate=0.01, reg=0.0001)


def step_perms(n, d, seed=17):
    """the injected shuffles of one step: per channel (p1, p2, p3, c2, c3)"""
    rng = np.random.default_rng(seed)
    return [tuple(rng.permutation(m).astype(np.int32) for m in (n, n, n, d, d)) for _ in range(3)]
