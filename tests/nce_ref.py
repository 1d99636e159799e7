"""Restatements and seeded cases for the edge tests of the step's InfoNCE passes (csrc/losses.hip: nce_plan,
nce_tile_f32, nce_tile_lds, the finish kernels) -- TEST INFRASTRUCTURE ONLY, no GPU needed.

    plan                nce_plan line for line in Python integers (max_per=None: the cut as it was before the budget was
                        bounded by kNceMaxPer -- the evidence of the bug and the premise of the cap cases)
    host_most           launch_infonce's upper bound of the task count, from the launch bounds
    split16_ranges      nce_tile_lds's key ranges and LDS stages
    info_nce_rows       loss and both TABLE gradients in closed form, in query chunks (no n x n array held), in the dtype
                        and on the device asked for: float64 is the reference, float32 the yardstick
    row errors          contrastive_ref.row_errors with FLOOR_FRAC below
    problems            the seeded, planted inputs of tests/test_gpu_nce_edges.py and the edges each one is there for

tests/test_nce_ref_cpu.py checks every premise here; tests/test_gpu_nce_edges.py runs the kernels on the cases."""
import numpy as np
import torch

from tests.batch_ref import MARGIN
from tests.contrastive_ref import FLOORS, row_errors  # noqa: F401  (re-exported: the measure of the edge tests)

# ---- geometry of csrc/losses.hip ------------------------------------------------------------------------------------
PAD = 64                 # nce_pad
QUERY_BLOCK = 128        # kNceQueryBlock: 8 waves x 16 queries
WAVE_ROWS = 16
KEY_BLOCK = 32           # kNceKeyBlock
SPLITS = 16              # kNceSplits
MAX_PER = 128            # kNceMaxPer: blocks whose 1 / l values fit the task's LDS array
MAX_PROBLEMS = 4         # kNceMaxProblems
REUSE_MAX = 8192         # kNceReuseMax (decided on the WORKSPACE's padded rows: nce_pad(n_max))
RING_SLOTS = 8           # NceF32::kSlots: a task of more blocks streams through the ring
F32_MAX_N = SPLITS * MAX_PER * KEY_BLOCK          # 65 536: launch_infonce refuses more
SPLIT16_SPLITS = 8       # SRH_NCE_SPLITS as shipped


def pad(n):
    return (n + PAD - 1) // PAD * PAD


def plan(ns, slots, max_per=MAX_PER):
    """nce_plan: dict(n, qb, kb, t, splits, per, first) for 1..4 live row counts on `slots` workgroups.  max_per=None
    restates the search without its bound (the parent of the fix)."""
    assert 1 <= len(ns) <= MAX_PROBLEMS and slots >= 1
    n = [int(x) for x in ns]
    qb, kb = [], []
    t_min, work = 1, 0
    for x in n:
        np_ = pad(x)
        qb.append((np_ + QUERY_BLOCK - 1) // QUERY_BLOCK)
        kb.append(np_ // KEY_BLOCK)
        t_min = max(t_min, (kb[-1] + SPLITS - 1) // SPLITS)
        work += qb[-1] * kb[-1]
    even = (work + slots - 1) // slots
    if max_per is None:
        t = max(t_min, even)
    else:
        t = (even if even < max_per else max_per) if even > t_min else t_min
    best_t, best_cost = t, -1
    it = 0
    while it < 32 and (max_per is None or t <= max_per or it == 0):
        tasks = sum(q * ((k + t - 1) // t) for q, k in zip(qb, kb))
        rounds = (tasks + slots - 1) // slots
        cost = rounds * t
        if best_cost < 0 or cost < best_cost:
            best_cost, best_t = cost, t
        if rounds <= 1:
            break
        it += 1
        t += 1
    splits, per, first = [], [], [0]
    for q, k in zip(qb, kb):
        sp = (k + best_t - 1) // best_t if k > 0 else 0
        splits.append(sp)
        per.append((k + sp - 1) // sp if sp > 0 else 0)
        first.append(first[-1] + q * sp)
    return dict(n=n, qb=qb, kb=kb, t=best_t, splits=splits, per=per, first=first)


def host_most(n_maxes):
    """launch_infonce: the grid is min(slots, this)"""
    return sum((pad(n) + QUERY_BLOCK - 1) // QUERY_BLOCK * SPLITS for n in n_maxes)


def first_over_budget(slots, limit=F32_MAX_N):
    """the smallest padded row count of ONE problem whose unbounded cut gives a task more than MAX_PER blocks"""
    for np_ in range(PAD, limit + 1, PAD):
        if plan((np_,), slots, max_per=None)["per"][0] > MAX_PER:
            return np_
    return None


def nce_chunk(d):
    return 16384 // d


def split16_ranges(np_, d, splits=SPLIT16_SPLITS):
    """nce_tile_lds on a workspace of np_ padded rows: per = roundup32(ceil(np / splits)) keys per range, and for each of
    the `splits` ranges the list of its LDS stages' key counts (empty: the range starts at or past np)"""
    per = ((np_ + splits - 1) // splits + 31) // 32 * 32
    chunk = nce_chunk(d)
    stages = []
    for ks in range(splits):
        kb, ke = ks * per, min(np_, ks * per + per)
        stages.append([min(chunk, ke - c0) for c0 in range(kb, ke, chunk)])
    return per, stages


# ---- the closed form ------------------------------------------------------------------------------------------------
EPS = 1e-12        # F.normalize


def _normalise(x):
    r = x.norm(dim=1, keepdim=True)
    return x / r.clamp_min(EPS), r


def _normalise_bwd(g, xn, r):
    """d/dx of x / max(|x|, eps) applied to g"""
    live = r >= EPS
    return torch.where(live, (g - xn * (xn * g).sum(1, keepdim=True)) / r.clamp_min(EPS), g / EPS)


def info_nce_rows(v1, v2, idx, tau, scale, dtype=torch.float64, device="cpu", chunk=2048):
    """(loss, dL/dv1, dL/dv2) of scale * mean_i(lse_i - s_ii), S = normalize(v1[idx]) normalize(v2[idx])^T / tau: the loss as
    a Python float, the gradients as tables of v1's / v2's shape in `dtype` on `device` (zero on the rows idx does not
    name; idx=None: every row).  P = softmax(S) exists one query chunk at a time:
        dL/dv1n = (P - I) v2n / (n tau),   dL/dv2n = (P - I)^T v1n / (n tau),
    then back through the normalisation and the gather, times scale."""
    t1 = torch.as_tensor(v1).to(device=device, dtype=dtype)
    t2 = torch.as_tensor(v2).to(device=device, dtype=dtype)
    ix = None if idx is None else torch.as_tensor(idx).to(device=device, dtype=torch.int64)
    a, b = (t1, t2) if ix is None else (t1[ix], t2[ix])
    n = a.shape[0]
    an, ra = _normalise(a)
    bn, rb = _normalise(b)
    inv_tau = torch.tensor(1.0 / tau, dtype=dtype, device=device)
    g1n, g2n = torch.empty_like(an), torch.zeros_like(bn)
    loss = torch.zeros((), dtype=dtype, device=device)
    for c0 in range(0, n, chunk):
        c1 = min(n, c0 + chunk)
        s = (an[c0:c1] @ bn.T) * inv_tau
        lse = torch.logsumexp(s, dim=1)
        p = torch.exp(s - lse[:, None])
        # P - I with its diagonal as minus the row's off-diagonal sum (sum_j P_ij = 1): at tau = 0.05 on correlated views
        # 1 - P_ii is 1e-6 .. 1e-8, and P_ii - 1 formed in float32 would lose all of it -- a yardstick of order 1.  The
        # loss likewise: lse_i - s_ii = log1p(sum_{j != i} exp(s_ij - s_ii)), not the difference of two numbers near 20
        own = torch.arange(c0, c1, device=p.device)
        rel = torch.exp(s - s[own - c0, own][:, None])
        rel[own - c0, own] = 0
        loss = loss + torch.log1p(rel.sum(1)).sum()
        p[own - c0, own] = 0
        p[own - c0, own] = -p.sum(1)
        g1n[c0:c1] = p @ bn
        g2n += p.T @ an[c0:c1]
    coef = scale * inv_tau / n
    g1 = _normalise_bwd((g1n * coef), an, ra)
    g2 = _normalise_bwd((g2n * coef), bn, rb)
    if ix is None:
        return float(loss) * scale / n, g1, g2
    G1, G2 = torch.zeros_like(t1), torch.zeros_like(t2)
    G1.index_add_(0, ix, g1)
    G2.index_add_(0, ix, g2)
    return float(loss) * scale / n, G1, G2


# ---- bounds -----------------------------------------------------------------------------------------------------------
LOSS_BOUND = {"f32": 2e-6, "split": 1e-5}      # the bounds of test_f32_infonce_is_the_same_bits... / test_infonce_gathered...
# split-16: the whole-tensor bound of today's tests carried to rows.  What the operand precisions give:
# 2^-18 per P.V product and 2^-22 / tau per logit -- MARGIN x (2^-18 + 2^-22 / 0.05) = 3.4e-5 at the smallest tau here.
ROW_BOUND_SPLIT = 2e-5
# Floor (the rule of DESIGN.md 4.15): the smallest of FLOORS at which float32 torch of info_nce_rows stays, per row,
# within half of the one per-row gradient bound that is fixed beforehand -- ROW_BOUND_SPLIT -- on every f32 case of
# n <= 4160 below.  Measured (tests/test_nce_ref_cpu.py::test_floor_and_yardstick asserts it): 7.1e-5 at 1e-3 and 1e-2,
# 2.2e-5 at 0.1, 6.1e-6 at 1.0.  A row's gradient is sum_j P_ij (v_j - v_i) through the normalisation's projection: unit
# terms that cancel by a factor that grows with sqrt(n), so rows far below the largest carry float32 rounding of the
# LARGE rows' size whatever the order of the sum.  Each row is therefore measured against the tensor's largest row.
GRAD_TOL = ROW_BOUND_SPLIT
FLOOR_FRAC = 1.0
# the worst per-row error of info_nce_rows(dtype=float32) against float64 over those cases at that floor, CPU torch
# (at A's n = 193, d = 128, tau = 0.05; the cases of tau >= 0.2 alone give less)
ROW_YARDSTICK_NCE = 6.2e-6
ROW_BOUND_F32 = MARGIN * ROW_YARDSTICK_NCE


# ---- planted problems -----------------------------------------------------------------------------------------------
def plants(n):
    """(diag, pairs) as positions of the gathered rows.  diag: rows with v2_i = v1_i exactly (s_ii = 1, the largest logit
    on the masked diagonal) in the first 16-row tile, the last full tile and the last partial tile.  pairs: (i, j) made
    identical in BOTH views (s_ij = s_ii) inside one 16-row tile, across two tiles of one 32-key block, and across two
    128-row query blocks.  No position is used twice."""
    diag, pairs = [], []
    if n >= 3:
        diag.append(1)
    if n >= 32:
        diag.append(n // 16 * 16 - 3)               # the last full tile
    if n % 16 and n >= 3:
        diag.append(n - 1)                          # the last partial tile
    if n >= 12:
        pairs.append((4, 9))
    if n >= 24:
        pairs.append((14, 18))
    if n >= 131:
        pairs.append((40, 129))
    used = [p for pr in pairs for p in pr]
    diag = sorted(set(p for p in diag if p not in used))
    assert len(set(diag + used)) == len(diag) + len(used)
    return diag, pairs


def problem(n, d, seed, rows=None, pairs=True):
    """dict(t1, t2, idx, n, diag, pairs): float32 tables of `rows` (default n + 200) rows, correlated views
    (t2 = t1 + 0.2 randn), a sorted random idx of n of them, planted as plants(n) says.  pairs=False leaves the identical
    pairs out: the tau = 0.05 cases.  There P_ii = P_ij = 1/2 to 1e-7 for an identical pair, the pair's two gradient rows
    are the difference of two equal halves -- 1e-7 of either -- and no float32 evaluation in any order holds them to
    more than a digit (float32 torch: 8 % per row), so they would measure float32, not the kernel."""
    rows = n + 200 if rows is None else rows
    rng = np.random.default_rng(seed)
    t1 = (rng.standard_normal((rows, d)) * 0.4).astype(np.float32)
    t2 = (t1 + rng.standard_normal((rows, d)) * 0.2).astype(np.float32)
    idx = np.sort(rng.choice(rows, size=n, replace=False)).astype(np.int32)
    diag, planted_pairs = plants(n)
    pairs = planted_pairs if pairs else []
    for i in diag:
        t2[idx[i]] = t1[idx[i]]
    for i, j in pairs:
        t1[idx[j]] = t1[idx[i]]
        t2[idx[j]] = t2[idx[i]]
    return dict(t1=t1, t2=t2, idx=idx, n=n, d=d, diag=diag, pairs=pairs)


def call(ns, d, seed):
    """the problems of one call: tables of max(ns) + 200 rows each"""
    return [problem(n, d, seed + 17 * k, rows=max(ns) + 200) for k, n in enumerate(ns)]


def edges(n):
    """what a live count of n leaves ragged"""
    return dict(pad_keys=pad(n) - n, wave_tail=n % WAVE_ROWS, block_tail=n % KEY_BLOCK, query_tail=n % QUERY_BLOCK,
                query_blocks=(pad(n) + QUERY_BLOCK - 1) // QUERY_BLOCK)


# A. pad, wave, block: both sides of 16, 32, 64, 128 and 192, and the first count with a third query block
A_NS = (2, 15, 17, 31, 33, 63, 64, 65, 127, 128, 129, 191, 193, 257)
A_TAUS = (1.0, 0.05)
A_LOW_TAU_NS = A_NS[::3]                       # (2, 31, 64, 128, 193): these also at tau = 0.05
A_WIDTHS = {"f32": (64, 128), "split": (64, 128, 256)}
# B. several problems per call
B_CALLS = (((2, 65, 130, 4100), 64), ((257, 63), 128), ((1877, 1640, 300, 129), 128))
B_PLAN_256 = dict(splits=[1, 1, 1, 7], per=[2, 4, 6, 19], first=[0, 1, 2, 4, 235])       # of B_CALLS[0] on 256 workgroups
# C. ring and reuse (f32): (live counts, launch bounds, d).  The reuse form is chosen from the workspace's rows, so the
# largest reuse case has launch bound = live count = 8192; every other bound is n + 100.
C_CALLS = (((4097,), (4197,), 64), ((4160,), (4260,), 64), ((4160,), (4260,), 128), ((8192,), (8192,), 64),
           ((8193,), (8293,), 64), ((8200, 300), (8300, 400), 64))
# D. the cap (f32): (n, launch bound, d); the first two are re-derived from the device's CU count
D_FIXED = ((16384, 16484, 128), (65536, 65536, 64))
# E. split-16 stage edges: (n, launch bound, d).  With a launch bound of n + 100 the LAST key range never holds a live key
# at the small counts (the ranges are cut on the workspace's rows), so one case has 250 of 256 rows live: range 7 of 8.
E_CASES = ((57, 64, 64), (129, 229, 64), (250, 256, 64), (2049, 2149, 64), (1025, 1125, 128), (513, 613, 256))
TAU_LARGE = 0.2          # B-E
TAU_PAIRS = 0.2          # identical pairs are planted from this temperature up (see problem)


def small_f32_cases():
    """[(name, tau, problem)]: every f32 problem of groups A-C with n <= 4160 -- what the floor and the yardstick are
    measured on (each problem once: a call's problems are independent)"""
    out = []
    for d in A_WIDTHS["f32"]:
        for n in A_NS:
            for tau in A_TAUS:
                if tau == 1.0 or n in A_LOW_TAU_NS:
                    out.append((f"A-n{n}-d{d}-tau{tau}", tau, problem(n, d, 1000 + n + d, pairs=tau >= TAU_PAIRS)))
    for ci, (ns, d) in enumerate(B_CALLS):
        for k, p in enumerate(call(ns, d, 2000 + 100 * ci)):
            out.append((f"B{ci}.{k}-n{p['n']}-d{d}", TAU_LARGE, p))
    for ci, (ns, _, d) in enumerate(C_CALLS):
        for k, p in enumerate(call(ns, d, 3000 + 100 * ci)):
            if p["n"] <= 4160:
                out.append((f"C{ci}.{k}-n{p['n']}-d{d}", TAU_LARGE, p))
    return out
