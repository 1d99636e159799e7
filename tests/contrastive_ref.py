"""References and seeded cases for the edge tests of the unit-row contrastive kernels and k-means (DESIGN.md 4.15;
csrc/contrastive.hip, csrc/ncl.hip) -- TEST INFRASTRUCTURE ONLY, no GPU needed.

    table_nce / batch_softmax   ncl_ref.table_nce_torch / ssl4rec_ref.batch_softmax as they are, float64 with autograd
                                (dtype=torch.float32 gives the same expressions in plain f32: the floor's yardstick)
    row_errors                  per row: max|got - want| / max(max|want_row|, floor_frac * max|want|)
    kmeans_update_f32           the float32 host restatement of km_sum: ascending rows from 0, then x 1/count
    assign_f64                  float64 distances, the best id (lowest on exact ties), the gap to the runner-up
    chunk_plan                  ct_chunks / ct_chunk_len restated, so the case list can name the layout it reaches

tests/test_contrastive_ref_cpu.py checks the premises of every builder here; tests/test_gpu_contrastive_edges.py runs
the kernels on the cases."""
import numpy as np
import torch

from tests import ncl_ref, ssl4rec_ref

LOSS_TOL = 1e-5      # loss against float64, relative
GRAD_TOL = 1e-4      # gradients against float64, per row through row_errors
# the smallest of FLOORS at which the reference's own expressions, evaluated in plain float32 torch on the CPU, stay
# within GRAD_TOL / 2 per row on every loss case (test_contrastive_ref_cpu.py::test_floor_frac_is_the_smallest_... asserts
# it): rows below floor_frac of the tensor's largest magnitude are measured against that floor
FLOORS = (1e-3, 1e-2, 1e-1, 1.0)
FLOOR_FRAC = 1e-2


# ---- losses ---------------------------------------------------------------------------------------------------------
def _leaf(x, dtype):
    return x.detach().to(dtype).clone().requires_grad_(True)


def table_nce(q, t, idx, tau, scale, dtype=torch.float64):
    """(loss, dL/dq, dL/dt) of scale * ncl_ref.table_nce_torch"""
    q_, t_ = _leaf(q, dtype), _leaf(t, dtype)
    loss = scale * ncl_ref.table_nce_torch(q_, t_, idx.long(), tau)
    loss.backward()
    return float(loss.detach()), q_.grad, t_.grad


def batch_softmax(u, v, tau, dtype=torch.float64):
    """(loss, dL/du, dL/dv) of ssl4rec_ref.batch_softmax"""
    u_, v_ = _leaf(u, dtype), _leaf(v, dtype)
    loss = ssl4rec_ref.batch_softmax(u_, v_, tau)
    loss.backward()
    return float(loss.detach()), u_.grad, v_.grad


def row_errors(got, want, floor_frac):
    """per row: max|got - want| / max(max|want_row|, floor_frac * max|want|), float64 (n,).  A tensor whose exact value
    is all zeros has no scale of its own: its rows come back as 0 where got is 0 too and inf elsewhere."""
    got = torch.as_tensor(got).detach().double().cpu().reshape(len(want), -1)
    want = torch.as_tensor(want).detach().double().cpu().reshape(len(want), -1)
    err = (got - want).abs().amax(dim=1)
    den = torch.clamp(want.abs().amax(dim=1), min=floor_frac * float(want.abs().max()))
    out = err / den
    out[(den == 0) & (err == 0)] = 0.0
    return out


# ---- k-means --------------------------------------------------------------------------------------------------------
def kmeans_update_f32(x, ids, k):
    """(centroids (k, d) float32, counts (k,) int64) as km_sum computes them: per cluster and column, x[row] added in
    float32 in ascending row order from 0, then times float32(1) / float32(count); an empty cluster is zeros; ids outside
    [0, k) are skipped"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    ids = np.asarray(ids, dtype=np.int64)
    sums = np.zeros((k, x.shape[1]), dtype=np.float32)
    counts = np.zeros(k, dtype=np.int64)
    for row in range(len(x)):
        j = int(ids[row])
        if 0 <= j < k:
            sums[j] = sums[j] + x[row]           # one float32 add per column
            counts[j] += 1
    cent = np.zeros_like(sums)
    for j in np.flatnonzero(counts):
        cent[j] = sums[j] * (np.float32(1) / np.float32(counts[j]))
    return cent, counts


def assign_f64(x, c):
    """(dist (n, k) float64 |x_i - c_j|^2, best (n,) the nearest centroid, the lowest id on exact ties, gap (n,) the
    distance of the runner-up minus the best's: 0 on an exact tie, inf when k = 1)"""
    x, c = np.asarray(x, dtype=np.float64), np.asarray(c, dtype=np.float64)
    dist = ((x[:, None, :] - c[None, :, :]) ** 2).sum(-1)
    best = dist.argmin(1)
    rest = dist.copy()
    rest[np.arange(len(x)), best] = np.inf
    return dist, best, rest.min(1) - dist[np.arange(len(x)), best]


def distinct_gap(x, c):
    """(best, gap, scale): as assign_f64, but the runner-up is the nearest centroid that is not a bit-identical copy of
    the best one; scale = |x|^2 + |c_best|^2, what the gap premise and the distance bound are relative to"""
    c = np.asarray(c, dtype=np.float32)
    dist, best, _ = assign_f64(x, c)
    same = (c[best][:, None, :] == c[None, :, :]).all(-1)          # (n, k): c_j equals the row's best centroid
    gap = np.where(same, np.inf, dist).min(1) - dist[np.arange(len(dist)), best]
    x64, c64 = np.asarray(x, dtype=np.float64), c.astype(np.float64)
    return best, gap, (x64 * x64).sum(1) + (c64 * c64).sum(1)[best]


# ---- the pass-1 chunk schedule of csrc/contrastive.hip ----------------------------------------------------------------
CT_ROWS, CT_TILE, CT_TARGET = 64, 64, 512


def chunk_plan(B, N):
    """ct_chunks / ct_chunk_len: chunks, chunk_len, and what they hold -- live (chunks that start below N), empty
    (chunks - live), last_keys (keys of the last live chunk), tiles (key tiles in all)"""
    rtiles, ctiles = -(-B // CT_ROWS), -(-N // CT_TILE)
    chunks = max(1, min(-(-CT_TARGET // rtiles), ctiles))
    chunk_len = -(-(-(-N // chunks)) // CT_TILE) * CT_TILE
    live = -(-N // chunk_len)
    return dict(chunks=chunks, chunk_len=chunk_len, live=live, empty=chunks - live,
                last_keys=N - (live - 1) * chunk_len, tiles=ctiles)


# ---- table InfoNCE cases ----------------------------------------------------------------------------------------------
IDX_FAMILIES = ("one", "ends", "last_tile", "perm")


def make_idx(family, B, N, g):
    if family == "one":                                   # every query names one key
        return torch.full((B,), N // 2, dtype=torch.int64)
    if family == "ends":                                  # only keys 0 and N - 1
        return torch.where(torch.rand(B, generator=g) < 0.5, 0, N - 1).to(torch.int64)
    if family == "last_tile":                             # only keys of the last (partial) tile
        lo = (N - 1) // CT_TILE * CT_TILE
        return torch.randint(lo, N, (B,), generator=g)
    if family == "perm":
        assert B <= N
        return torch.randperm(N, generator=g)[:B]
    raise ValueError(family)


def table_problem(B, N, d, family, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, d, generator=g) * 0.1
    t = torch.randn(N, d, generator=g) * 0.1
    return q, t, make_idx(family, B, N, g)


# (B, N, d, tau): B in {1, 15, 16, 17, 63, 64, 65, 129} crossed sparsely with N in {1, 2, 63, 64, 65, 127, 128, 129, 257};
# every N with N % 64 != 0 and every B with B % 16 != 0 appears at tau = 1.0, where a counted pad would weigh exp(-1)
# The two d = 1 shapes have exact-zero gradients (measured against cancel_scales only), so their (B, N) must come again
# with gradients that row_errors can measure: each is the second problem of the call before it, at that call's d > 1 and
# tau -- (65, 127) at d = 128, tau = 1; (16, 128) at d = 128, tau = 0.2.  test_table_shapes_cover_the_edges asserts this
# pairing, so reordering the list cannot lose it.
TABLE_SHAPES = [
    (1, 257, 64, 1.0), (15, 1, 50, 1.0), (17, 2, 100, 1.0), (63, 63, 128, 1.0), (65, 127, 1, 1.0), (129, 129, 50, 1.0),
    (16, 65, 64, 1.0), (64, 64, 100, 0.03), (129, 2, 128, 0.2), (16, 128, 1, 0.2), (17, 129, 64, 0.03),
    (63, 257, 50, 0.2), (65, 1, 128, 0.03), (1, 64, 100, 0.2), (64, 127, 64, 0.2), (15, 63, 128, 0.03),
]
# the chunk layouts (d = 64), two problems per call: 31 empty trailing chunks + chunks equal to tiles with a 1-key last
# tile; two chunks of which the second holds 2 keys + a single chunk
CHUNK_CALLS = [
    (((512, 4100), (65, 257)), 1.0),
    (((16400, 130), (32769, 130)), 0.2),
]
SCALES = (1.0, 1.5)


def _family(i, B, N):
    f = IDX_FAMILIES[i % 4]
    return "ends" if f == "perm" and B > N else f


def table_calls():
    """[(name, tau, [(q, t, idx, scale), (q, t, idx, scale)])]: every shape of TABLE_SHAPES as the first problem of a call
    with the next shape of the list (at this call's d and tau) as its second, then the chunk-layout calls"""
    out = []
    for i, (B, N, d, tau) in enumerate(TABLE_SHAPES):
        B2, N2 = TABLE_SHAPES[(i + 1) % len(TABLE_SHAPES)][:2]
        probs = [table_problem(B, N, d, _family(i, B, N), 100 + i) + (SCALES[0],),
                 table_problem(B2, N2, d, _family(i + 2, B2, N2), 200 + i) + (SCALES[1],)]
        out.append((f"{B}x{N}+{B2}x{N2}-d{d}-tau{tau}", tau, probs))
    for i, (shapes, tau) in enumerate(CHUNK_CALLS):
        probs = [table_problem(B, N, 64, _family(i + k + 1, B, N), 300 + 2 * i + k) + (SCALES[k],)
                 for k, (B, N) in enumerate(shapes)]
        out.append(("chunks-" + "+".join(f"{B}x{N}" for B, N in shapes), tau, probs))
    return out


def is_zero_gradient(N, d):
    """one key: P = 1 and the positive cancels it; one column: the normalisation backward projects everything out.
    Either way the exact gradients are zero and have no scale of their own."""
    return N == 1 or d == 1


def cancel_scales(q, t, idx, tau, scale):
    """(per query, per key) the size of what cancels in a gradient whose exact value is zero: dL/dq_b is
    (scale / tau) (sum_j P_bj t_j - t_pos) / |q_b|, two unit-sized terms; dL/dt_j is (scale / tau) sum_b (P_bj - [idx_b = j])
    q_b / |t_j|, with sum_b P_bj + #{b: idx_b = j} unit-sized terms.  float32 leaves about 1e-7 of these."""
    nq = torch.nn.functional.normalize(q.double(), dim=1)
    nt = torch.nn.functional.normalize(t.double(), dim=1)
    P = torch.softmax(nq @ nt.T / tau, dim=1)
    hits = torch.bincount(idx.long(), minlength=len(t)).double()
    return (2.0 * scale / tau / q.double().norm(dim=1).clamp_min(1e-12),
            scale / tau * (P.sum(0) + hits) / t.double().norm(dim=1).clamp_min(1e-12))


# ---- degenerate rows ------------------------------------------------------------------------------------------------
DEGENERATE = dict(B=17, N=65, d=64, tau=0.2, zero_q=3, tiny_q=9, near_q=12, zero_t=10, zero_t_pos=64, tiny_t=33, near_t=20)
DEGENERATE["clamped_q"] = tuple(DEGENERATE[k] for k in ("zero_q", "tiny_q", "near_q"))
DEGENERATE["clamped_t"] = tuple(DEGENERATE[k] for k in ("zero_t", "zero_t_pos", "tiny_t", "near_t"))


def degenerate_problem():
    """(q, t, idx): a zero query, a query of 1e-20 entries (below F.normalize's clamp), a zero key nobody names, a zero
    key that is a positive (alone in the last tile), a key of 1e-20 entries that is a positive too -- and a query and a
    key (a positive) of norm 8e-13, just below the clamp: their normalised rows have norm 0.8, so the projection of the
    unclamped backward, wrongly applied, would take 0.64 of the parallel part off (on the rows above it takes off
    nothing that float32 can see)"""
    c = DEGENERATE
    g = torch.Generator().manual_seed(400)
    q = torch.randn(c["B"], c["d"], generator=g) * 0.1
    t = torch.randn(c["N"], c["d"], generator=g) * 0.1
    idx = torch.randint(0, c["N"], (c["B"],), generator=g)
    idx[idx == c["zero_t"]] = 0
    idx[idx == c["near_t"]] = 1
    idx[0], idx[5], idx[c["zero_q"]], idx[7], idx[c["near_q"]] = c["zero_t_pos"], c["tiny_t"], c["zero_t_pos"], c["near_t"], 2
    q[c["zero_q"]] = 0.0
    q[c["tiny_q"]] = 1e-20
    t[c["zero_t"]] = 0.0
    t[c["zero_t_pos"]] = 0.0
    t[c["tiny_t"]] = 1e-20
    q[c["near_q"]] *= 8e-13 / float(q[c["near_q"]].double().norm())
    t[c["near_t"]] *= 8e-13 / float(t[c["near_t"]].double().norm())
    return q, t, idx


# ---- batch softmax cases ----------------------------------------------------------------------------------------------
SOFTMAX_B = (1, 2, 15, 16, 17, 63, 64, 65, 129, 257)
SOFTMAX_D = (50, 64, 128)
SOFTMAX_TAU = (0.07, 1.0)


SOFTMAX_ZERO = dict(B=17, d=64, tau=0.07, seed=401, u_row=4, v_row=7)     # the case with a zero row on either side


def softmax_problem(B, d, seed=None, zero_rows=False):
    """u, v with a third of the rows anti-aligned (p_bb far below 1e-5 there, so the weight w_b matters)"""
    g = torch.Generator().manual_seed(B + d if seed is None else seed)
    u = torch.randn(B, d, generator=g) * 0.1
    v = torch.randn(B, d, generator=g) * 0.1
    v[::3] = -u[::3] + 0.01 * v[::3]
    if zero_rows:
        u[SOFTMAX_ZERO["u_row"]] = 0.0
        v[SOFTMAX_ZERO["v_row"]] = 0.0
    return u, v


# ---- the underflow envelope -------------------------------------------------------------------------------------------
ENVELOPE = {  # kind: (tau, cosines of the keys with query 0)
    "inside": (0.03, (-0.95, -0.96, -0.97, -0.98, -0.99)),
    "outside": (0.01, (-0.95, -0.96, -0.97, -0.98, -0.99)),
    "band": (0.01, (0.05, 0.0, -0.2, -0.5, -0.9)),      # (0.05 - 1) / 0.01 = -95: below exp's normal range (-87.3)
}
F32_MIN_NORMAL = 2.0 ** -126


def envelope_problem(kind, softmax):
    """(q, t, idx, tau): d = 64, N = 5 keys at the listed cosines with query 0, the other queries ordinary; B = 17 and a
    random idx for the table loss, B = 5 (idx = arange) for batch softmax"""
    tau, cosines = ENVELOPE[kind]
    g = torch.Generator().manual_seed(500 + len(kind))
    B, N, d = (5 if softmax else 17), 5, 64
    q = torch.randn(B, d, generator=g, dtype=torch.float64)
    q0 = q[0] / q[0].norm()
    t = torch.empty(N, d, dtype=torch.float64)
    for j, c in enumerate(cosines):
        r = torch.randn(d, generator=g, dtype=torch.float64)
        r = r - (r @ q0) * q0
        t[j] = (c * q0 + (1 - c * c) ** 0.5 * r / r.norm()) * (0.5 + j)
    idx = torch.arange(B) if softmax else torch.randint(0, N, (B,), generator=g)
    return (q * 0.1).float(), (t * 0.1).float(), idx, tau


def shifted_terms_f32(q, t, tau):
    """the kernels' exp((s - 1) / tau) of every (query, key), emulated in float32 torch on the CPU"""
    nq = torch.nn.functional.normalize(q.float(), dim=1)
    nt = torch.nn.functional.normalize(t.float(), dim=1)
    return torch.exp((nq @ nt.T - 1.0) * torch.tensor(1.0 / tau, dtype=torch.float32))


# ---- k-means assign cases ---------------------------------------------------------------------------------------------
ASSIGN_SHAPES = [  # (n, k, d)
    (1, 1, 3), (15, 1, 50), (17, 2, 100), (17, 63, 64), (63, 64, 100), (64, 65, 128), (65, 129, 3), (130, 1025, 64),
    (130, 65, 50), (63, 129, 128),
]
COPY_OFFSETS = (1, 4, 16, 64)
GAP_FRAC = 1e-3       # every row's float64 gap is at least this share of |x|^2 + |c_best|^2 (f32 noise: about 1e-6 of it)


def assign_case(n, k, d, seed, tail_row=False):
    """dict(x, c, copies, kinds): centroids randn + 1.5 (a common offset keeps c_i.c_j > 0) with bit-identical
    copies planted at (j, j + off), one pair ending in the last partial tile; rows [0, n/4) are -3 c_j (every
    |c|^2 - 2 x.c is positive there, so a padded centroid scoring 0 would win), the next n/8 sit exactly on a centroid,
    the next n/8 close to a copied one, the rest are free.  Rows whose gap falls short are redrawn from the seed.
    tail_row (64 does not divide k, k > 64): centroid k - 1, alone in the trailing partial tile, is left out of the copies
    and the last row sits on it (kind "last"), so that tile holds a winner."""
    rs = np.random.RandomState(seed)
    c = (rs.randn(k, d) + 1.5).astype(np.float32)
    copies = []
    for off in COPY_OFFSETS:
        if k > off + 2:
            j = int(rs.randint(0, k - off - (1 if tail_row else 0)))
            if any(j in p or j + off in p for p in copies):
                continue
            c[j + off] = c[j]
            copies.append((j, j + off))
    tail = (k - 1) // 64 * 64                      # first centroid of the last tile
    if not tail_row and k % 64 and k - 1 >= tail >= 64 and not any(k - 1 in p or tail - 1 in p for p in copies):
        c[k - 1] = c[tail - 1]                     # a copy in the last partial tile, its original one tile earlier
        copies.append((tail - 1, k - 1))
    n_neg, n_on, n_tie = n // 4, n // 8, (n // 8 if copies else 0)
    kinds = ["neg"] * n_neg + ["on"] * n_on + ["tie"] * n_tie
    kinds += ["free"] * (n - len(kinds))
    if tail_row:
        assert k % 64 and k > 64
        kinds[-1] = "last"
    x = np.zeros((n, d), dtype=np.float32)
    c64 = c.astype(np.float64)

    def draw(kind, turn):
        if kind == "neg":
            return -3.0 * c[rs.randint(0, k)]
        if kind == "on":
            return c[rs.randint(0, k)].copy()
        if kind == "last":
            return c[k - 1].copy()
        if kind == "tie":
            return c[copies[turn % len(copies)][turn // len(copies) % 2]] + 0.01 * rs.randn(d).astype(np.float32)
        return (rs.randn(d) + 1.5).astype(np.float32)

    for i, kind in enumerate(kinds):
        for turn in range(1000):
            x[i] = draw(kind, i + turn)
            _, gap, scale = distinct_gap(x[i:i + 1], c)
            ok = gap[0] >= 2 * GAP_FRAC * scale[0]
            if kind == "neg":
                xi = x[i].astype(np.float64)
                ok = ok and ((c64 * c64).sum(1) - 2.0 * (c64 @ xi)).min() > 0
            if ok:
                break
        else:
            raise AssertionError(f"assign_case{(n, k, d)}: no admissible row of kind {kind}")
    return dict(x=x, c=c, copies=copies, kinds=kinds)


ASSIGN_TAIL_ROW = (8, 9)      # the second case of k = 65 and of k = 129: a winner in the trailing partial tile


def assign_cases():
    return [assign_case(n, k, d, 600 + i, tail_row=i in ASSIGN_TAIL_ROW) for i, (n, k, d) in enumerate(ASSIGN_SHAPES)]


# ---- k-means update cases ---------------------------------------------------------------------------------------------
UPDATE_SHAPES = [  # (n, k, d)
    (1, 1, 1), (7, 1, 3), (8, 3, 50), (9, 3, 64), (255, 5, 65), (256, 37, 128), (257, 1025, 200), (513, 2049, 64),
    (513, 3, 1), (513, 1, 128),
]
BAD_IDS = (-1, None, 2 ** 31 - 1)       # None: k


def update_case(n, k, d, seed, all_invalid=False):
    """(x, ids int32): k >= 5 and n >= 40 plants clusters 0..4 of exactly 7, 8, 9, 1 and 0 rows (their rows spread over
    the whole range) and draws the rest from [5, k) -- or, at k = 5, leaves them out of the table; smaller shapes draw from
    [0, k).  n >= 7 mixes in ids -1, k and 2^31 - 1 (about one row in nine), except at k = 1 with n = 7 (a cluster of
    exactly 7 = all rows).  k > 1024 plants rows in cluster k - 1 and its neighbours (see below).  x is randn; a single column gets an offset of 2, since the mean of one zero-mean column
    cancels and a bound relative to it would measure the cancellation, not the sum."""
    rs = np.random.RandomState(seed)
    x = (rs.randn(n, d) + (2.0 if d == 1 else 0.0)).astype(np.float32)
    bad = np.array([k if b is None else b for b in BAD_IDS], dtype=np.int64)
    if all_invalid:
        return x, bad[np.arange(n) % 3].astype(np.int32)
    if k >= 5 and n >= 40:
        ids = rs.randint(5, k, n) if k > 5 else bad[np.arange(n) % 3]
        spots = rs.permutation(n)[:25]
        ids[spots] = np.repeat([0, 1, 2, 3], [7, 8, 9, 1])
        free = np.setdiff1d(np.arange(n), spots)
    else:
        ids = rs.randint(0, k, n)
        free = np.arange(n)
    if n >= 7 and not (k == 1 and n == 7):
        hit = free[rs.rand(len(free)) < 1.0 / 9.0]
        if len(hit) == 0:
            hit = free[:1]
        ids[hit] = bad[np.arange(len(hit)) % 3]
    if k > 1024:
        # km_scan gives thread t clusters [t per, (t + 1) per), per = ceil(k / 1024): the last cluster (and, at k = 2049,
        # cluster 1024) exists only through the rounding up.  Rows go into k - 1, into the two clusters below it (at
        # k = 2049 the same thread's) and into 1023 / 1024, so a wrong start[] of any of them moves real rows.
        keep = np.flatnonzero((ids >= 5) & (ids < k))
        plant = [k - 1] * 3 + [k - 2] * 2 + [k - 3] * 2 + ([1024] * 3 + [1023] * 2 if k > 1025 else [])
        ids[keep[np.linspace(0, len(keep) - 1, len(plant)).astype(np.int64)]] = plant
    return x, ids.astype(np.int32)


def update_cases():
    out = [update_case(n, k, d, 700 + i) for i, (n, k, d) in enumerate(UPDATE_SHAPES)]
    out.append(update_case(9, 3, 64, 799, all_invalid=True))
    return out
