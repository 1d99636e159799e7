"""Float64 restatements, seeded cases and bounds of the rest of util/loss_torch.py on the device: the
pair cross-entropy (csrc/contrastive.hip under PAIR) behind info_nce, InfoNCE(b_cos=False) and InfoNCE below temperature
0.03, and the two row kernels of csrc/rowloss.hip behind triplet_loss and kl_divergence -- TEST INFRASTRUCTURE ONLY, no GPU.

    pair_ce          closed form in the dtype asked for (float64: the reference; float32: the f32-torch-on-the-CPU yardstick)
    info_nce, cosine the two wrappers' closed forms on top of it (cat, labels (m + B) mod 2B, the normalise and its backward)
    triplet, kl      numpy float64
    bounds           pair CE: table_ce_ref's LOSS_TOL / GRAD_TOL / LSE_TOL and contrastive_ref's floor rule, one floor per
                     group of FLOOR_OF; row kernels: batch_ref.MARGIN x the yardsticks recorded below

tests/test_losssurface_ref_cpu.py pins every restatement against float64 torch autograd of the reference's own
expressions, asserts the premises of the cases, and re-measures floors and yardsticks; tests/test_gpu_losssurface.py runs
the kernels.  Every builder is cached and its arrays are never written to."""
import functools

import numpy as np
import torch

from tests.batch_ref import MARGIN, _f64, elem_error, row_error  # noqa: F401  (the measures, re-exported)
from tests.contrastive_ref import CT_TILE, FLOORS, chunk_plan, row_errors  # noqa: F401
from tests.loss_ref import GOUTS, bpr_shapes, loss_error  # noqa: F401
from tests.table_ce_ref import GRAD_TOL, LOSS_TOL, LSE_TOL, ws_carve  # noqa: F401

INF = float("inf")


# ======================================================================================================================
# pair cross-entropy
# ======================================================================================================================
def pair_ce(h, t, labels, inv_temp, loss_scale=1.0, exclude=False, dtype=torch.float64):
    """dict(loss, gh, gt, lse, pos, row_loss) of loss_scale * sum_m (lse_m - s_{m, label_m}), s = inv_temp h t^T, key m left
    out of row m under ``exclude``, every expression in ``dtype``.  A label outside [0, N), or the row's own key under
    exclusion, has no one-hot and makes the loss (and its row term) NaN."""
    H, T = torch.as_tensor(h).to(dtype), torch.as_tensor(t).to(dtype)
    labels = torch.as_tensor(labels).long()
    M, N = len(H), len(T)
    s = (H @ T.T) * inv_temp
    if exclude:
        assert M == N
        s = s.masked_fill(torch.eye(M, dtype=torch.bool), -INF)
    mx = s.max(dim=1, keepdim=True).values
    lse = mx.squeeze(1) + torch.log(torch.exp(s - mx).sum(dim=1))
    ok = (labels >= 0) & (labels < N)
    if exclude:
        ok &= labels != torch.arange(M)
    rows = ok.nonzero().flatten()
    pos = torch.full_like(lse, float("nan"))
    pos[rows] = s[rows, labels[rows]]
    p = torch.exp(s - lse[:, None])
    p[rows, labels[rows]] -= 1.0
    k = loss_scale * inv_temp
    row_loss = lse - pos
    return dict(loss=float(loss_scale * row_loss.sum()), gh=k * (p @ T), gt=k * (p.T @ H), lse=lse, pos=pos, row_loss=row_loss)


ZERO_LOSS = 1e-12          # |loss64| below this: the loss is an exact zero of the mathematics (one key per row)


def loss_den(ref, loss_scale):
    """What an exactly zero loss is measured against (M = N = 2 under exclusion, one key, info_nce at B = 1, InfoNCE at
    n = 1: every row has one key, its positive, so lse_m = s_pos): loss_scale * sum_m max(1, |lse_m|, |s_pos_m|), the sum of
    table_ce_ref's per-row denominators."""
    den = torch.maximum(ref["lse"].abs().clamp_min(1.0), torch.nan_to_num(ref["pos"].abs(), nan=1.0))
    return abs(loss_scale) * float(den.sum())


def loss_figure(got, ref, loss_scale, scale=1.0):
    """table_ce_ref's loss figure, |got - want| / |want| (NaN against NaN is 0), of a loss computed at ``scale`` times the
    reference's; where the reference is an exact zero, |got| over loss_den"""
    want = scale * ref["loss"]
    if want != want:
        return 0.0 if float(got) != float(got) else INF
    if abs(ref["loss"]) < ZERO_LOSS:
        return abs(float(got)) / (abs(scale) * loss_den(ref, loss_scale))
    return abs(float(got) - want) / abs(want)


def grad_figure(got, want, floor_frac):
    """worst row of contrastive_ref.row_errors; NaN anywhere is inf"""
    worst = float(row_errors(got, want, floor_frac).max())
    return worst if worst == worst else INF


def normalize_rows(x, eps, dtype=torch.float64):
    """(y = x / max(|x|, eps), |x|)"""
    X = torch.as_tensor(x).to(dtype)
    nrm = X.norm(dim=1)
    return X / nrm.clamp_min(eps)[:, None], nrm


def normalize_bwd(g, y, nrm, eps):
    """the gradient of x from the gradient g of y = x / max(|x|, eps): (g - y (y.g)) / |x|, g / eps on a clamped row"""
    clamped = (nrm < eps)[:, None]
    den = nrm.clamp_min(eps)[:, None]
    return torch.where(clamped, g / den, (g - y * (y * g).sum(dim=1, keepdim=True)) / den)


def infonce_raw(v1, v2, tau, b_cos, dtype=torch.float64):
    """loss_torch.py:35-50 in closed form: dict(loss, g1, g2) (F.normalize's clamp 1e-12 when b_cos)"""
    n = len(v1)
    labels = torch.arange(n)
    if not b_cos:
        r = pair_ce(v1, v2, labels, 1.0 / tau, 1.0 / n, dtype=dtype)
        return dict(loss=r["loss"], g1=r["gh"], g2=r["gt"], ce=r)
    (y1, n1), (y2, n2) = normalize_rows(v1, 1e-12, dtype), normalize_rows(v2, 1e-12, dtype)
    r = pair_ce(y1, y2, labels, 1.0 / tau, 1.0 / n, dtype=dtype)
    return dict(loss=r["loss"], g1=normalize_bwd(r["gh"], y1, n1, 1e-12), g2=normalize_bwd(r["gt"], y2, n2, 1e-12), ce=r)


def info_nce(z_i, z_j, temp, sim, dtype=torch.float64):
    """loss_torch.py:54-88 in closed form: dict(loss, gi, gj).  'cos': cosine_similarity's clamp 1e-8 on each norm."""
    B = len(z_i)
    z = torch.cat((torch.as_tensor(z_i).to(dtype), torch.as_tensor(z_j).to(dtype)))
    labels = (torch.arange(2 * B) + B) % (2 * B)
    if sim == "cos":
        y, nrm = normalize_rows(z, 1e-8, dtype)
    else:
        y = z
    r = pair_ce(y, y, labels, 1.0 / temp, 1.0 / (2 * B), exclude=True, dtype=dtype)
    gz = r["gh"] + r["gt"]
    if sim == "cos":
        gz = normalize_bwd(gz, y, nrm, 1e-8)
    return dict(loss=r["loss"], gi=gz[:B], gj=gz[B:], ce=r)


# ---- floors ----------------------------------------------------------------------------------------------------------
# contrastive_ref's rule: the smallest of FLOORS at which the same expressions in f32 torch on the CPU stay within
# GRAD_TOL / 2 per row on every case of the group (test_losssurface_ref_cpu.py asserts each is the smallest that does).
#   ordinary  logits of the order of 1..20 (1/tau <= 20 on N(0, 0.3^2) rows)
#   hot       1/tau = 100 on N(0, 0.3^2) rows, rows scaled until s/tau passes 100, unit rows at tau <= 0.02: a logit near
#             100 carries a float32 error of some 1e-5 (its half ulp is 4e-6 and it is a sum of d products), which is the
#             RELATIVE error of every P_mj and so of every small gradient row they make up.
#   extreme   the planted whole-row offsets of +100 .. -130, where EVERY logit of a row carries that error -- the reason
#             table_ce_ref gives its extreme family a floor of its own.  The rule is applied to its two gradients apart:
#             gh meets it at 1e-1 ("extreme_gh"), gt only at 1 ("extreme").  Here every row of h is planted, so there is no
#             split into planted and other rows as table_ce_ref.row_groups makes; splitting the keys into those a label
#             names and the others was measured and leaves gt's floor where it is (8.8e-5 and 9.0e-5 at 1e-1).
FLOOR_OF = {"ordinary": 1e-3, "hot": 1e-1, "extreme_gh": 1e-1, "extreme": 1.0}


def pair_floors(c):
    """(floor of gh, floor of gt) of a direct case"""
    g = pair_group(c)
    return (FLOOR_OF["extreme_gh"], FLOOR_OF["extreme"]) if g == "extreme" else (FLOOR_OF[g], FLOOR_OF[g])


# ---- direct cases of ops.pair_ce_fwd_bwd --------------------------------------------------------------------------------
EXT_OFFSETS = (100.0, -105.0, 0.0, -130.0, 60.0)     # the whole-row logit offsets of the extreme family, row m: m % 5
# (M, N, d, inv_temp, exclude, family).  Exclusion: M = N in {2, 63, 64, 65, 129, 130, 514}; 65 and 129 leave the last row
# alone with its own key in a last tile of one key, 130 has three key chunks.  Without: (1, 1), (65, 65), (100, 300),
# (129, 1030).  d in {64, 128} and 50, 100 through the padding; inv_temp in {1, 5, 100}.  Families: ordinary (N(0, 0.3^2)
# rows), extreme (whole rows offset by EXT_OFFSETS: a naive exp(s) overflows at +100, rows at -105 and -130 lie below every
# float32 exp), alias (H = T, the fused gh + gt, under exclusion).
PAIR_CASES = [
    (2, 2, 64, 1.0, True, "ordinary"), (63, 63, 50, 5.0, True, "ordinary"), (64, 64, 128, 1.0, True, "ordinary"),
    (65, 65, 64, 1.0, True, "ordinary"), (65, 65, 100, 100.0, True, "ordinary"), (129, 129, 64, 5.0, True, "ordinary"),
    (130, 130, 64, 1.0, True, "ordinary"), (130, 130, 128, 100.0, True, "ordinary"), (514, 514, 64, 5.0, True, "ordinary"),
    (65, 65, 64, 5.0, True, "extreme"), (129, 129, 128, 1.0, True, "extreme"), (130, 130, 50, 100.0, True, "extreme"),
    (514, 514, 64, 1.0, True, "extreme"),
    (1, 1, 64, 1.0, False, "ordinary"), (65, 65, 64, 5.0, False, "ordinary"), (100, 300, 50, 1.0, False, "ordinary"),
    (129, 1030, 128, 5.0, False, "ordinary"), (129, 1030, 64, 100.0, False, "ordinary"),
    (65, 65, 128, 100.0, False, "extreme"), (100, 300, 100, 5.0, False, "extreme"), (129, 1030, 64, 1.0, False, "extreme"),
    (2, 2, 64, 5.0, True, "alias"), (65, 65, 64, 1.0, True, "alias"), (129, 129, 50, 5.0, True, "alias"),
    (130, 130, 128, 100.0, True, "alias"), (514, 514, 64, 100.0, True, "alias"),
]
PAIR_SCALES = (1.0, -2.5)                  # loss_scale of the direct calls (and 0.0 on one case: exact zeros)
PAIR_DIRTY = (7, "between", 4)             # PAIR_CASES[7] twice with PAIR_CASES[4] between them on one dirty workspace


def pair_id(c):
    return "M%d_N%d_d%d_it%g_%s_%s" % (c[0], c[1], c[2], c[3], "excl" if c[4] else "full", c[5])


def pair_group(c):
    """the floor group of a direct case"""
    return "extreme" if c[5] == "extreme" else "hot" if c[3] >= 100.0 else "ordinary"


@functools.lru_cache(maxsize=None)
def pair_case(index):
    """(h (M x d), t (N x d), labels (M,) int64) float32 on the host; alias: t is h"""
    M, N, d, inv_temp, exclude, family = PAIR_CASES[index]
    g = torch.Generator().manual_seed(4270 + index)
    h = 0.3 * torch.randn(M, d, generator=g)
    t = h if family == "alias" else 0.3 * torch.randn(N, d, generator=g)
    if family == "extreme":
        # column 0 of every key is 1 and h[m, 0] inv_temp is the row's offset; the rest of the logit is of the order of 1
        h = h / inv_temp ** 0.5
        t = t / inv_temp ** 0.5
        h[:, 1:] *= 3.0
        t[:, 1:] *= 3.0
        t[:, 0] = 1.0
        h[:, 0] = torch.tensor(EXT_OFFSETS)[torch.arange(M) % len(EXT_OFFSETS)] / inv_temp
    if exclude:
        labels = (torch.arange(M) + 1 + torch.randint(0, N - 1, (M,), generator=g)) % N      # never the row itself
        if M >= 6:
            labels[-1] = 0
            labels[0] = N - 1
    else:
        labels = torch.randint(0, N, (M,), generator=g)
        labels[-1] = N - 1
    return h, t, labels


@functools.lru_cache(maxsize=None)
def pair_reference(index, dtype=torch.float64):
    M, N, d, inv_temp, exclude, family = PAIR_CASES[index]
    h, t, labels = pair_case(index)
    return pair_ce(h, t, labels, inv_temp, 1.0, exclude, dtype)


# ---- info_nce cases ---------------------------------------------------------------------------------------------------------
# (B, d, temp, sim): B in {1, 31, 32, 33, 65, 257} (2B = 64 at B = 32: one full tile; 2B = 66 and 130: a last tile of 2 keys),
# d in {64, 50, 128}, temp in {1.0, 0.2, 0.05}, both sims.  'cos' rows keep a norm >= 1e-3 (asserted on the CPU).
INFO_NCE_CASES = [
    (1, 64, 1.0, "dot"), (1, 50, 0.2, "cos"), (31, 64, 0.2, "dot"), (31, 128, 0.05, "cos"), (32, 50, 1.0, "dot"),
    (32, 64, 0.05, "cos"), (33, 128, 0.2, "dot"), (33, 64, 1.0, "cos"), (65, 64, 0.05, "dot"), (65, 50, 0.2, "cos"),
    (257, 64, 1.0, "dot"), (257, 128, 0.05, "dot"), (257, 64, 0.2, "cos"),
]
ZERO_ROW_CASE = (33, 64, 0.2, "cos")       # its row ZERO_ROW of z_i is exactly zero: forward value only
ZERO_ROW = 5


def info_nce_group(c):
    # dot: |s| / temp reaches 0.09 * 64 * 3 / 0.05 ~ 100 only at temp = 0.05 on d = 128 rows; cos: 1 / temp = 20 at most
    return "ordinary"


@functools.lru_cache(maxsize=None)
def info_nce_case(index, zero_row=False):
    B, d, temp, sim = INFO_NCE_CASES[index] if not zero_row else ZERO_ROW_CASE
    g = torch.Generator().manual_seed(5270 + (999 if zero_row else index))
    z_i, z_j = 0.3 * torch.randn(B, d, generator=g), 0.3 * torch.randn(B, d, generator=g)
    if sim == "cos":
        # the positive is nearer than the others (cos ~ 0.45), but not so near that 1 - P_pos, which every gradient row is
        # proportional to, drops to float32's rounding of P_pos (at cos ~ 0.9 and temp 0.05 it is 1e-6: softmax - onehot
        # in float32, torch's or a kernel's, then holds no gradient to better than some 1e-2 of itself)
        z_j = 0.5 * z_i + z_j
        if B >= 31:
            z_i[3] *= 1e-2                      # a short row, norm ~ 0.3 * 8 * 1e-2 = 2.4e-2 >= 1e-3
    if zero_row:
        z_i[ZERO_ROW] = 0.0
    return z_i, z_j


@functools.lru_cache(maxsize=None)
def info_nce_reference(index, dtype=torch.float64):
    B, d, temp, sim = INFO_NCE_CASES[index]
    return info_nce(*info_nce_case(index), temp, sim, dtype)


# ---- InfoNCE(b_cos=False) and InfoNCE(b_cos=True) below temperature 0.03 ----------------------------------------------------
# raw: (n, d, tau, family): n in {1, 63, 64, 65, 129, 1000}, d in {64, 128, 50}, tau in {1.0, 0.2, 0.05}; "normal" N(0, 0.3^2)
# rows, "big" rows scaled so that the largest |s| / tau is RAW_BIG_LOGIT.
RAW_BIG_LOGIT = 150.0
RAW_CASES = [
    (1, 64, 1.0, "normal"), (63, 50, 0.2, "normal"), (64, 128, 0.05, "normal"), (65, 64, 0.2, "normal"),
    (129, 128, 1.0, "normal"), (1000, 64, 0.05, "normal"), (1000, 50, 1.0, "normal"),
    (1, 128, 0.2, "big"), (63, 64, 0.05, "big"), (64, 50, 1.0, "big"), (65, 128, 0.05, "big"), (129, 64, 0.2, "big"),
    (1000, 64, 1.0, "big"),
]
# unit: (n, d, tau): the cosine form at a temperature the unit-row kernels refuse.  Row COLD_ROW of view1 has every entry
# negative and every row of view2 has every entry positive: each of its cosines, the diagonal too, is <= 0, so every
# exp((s - 1) / tau) of the old kernel's row is exp(-1 / tau) <= e^-50 or less -- at tau = 0.01 all underflowed.
UNIT_CASES = [(65, 64, 0.02), (65, 64, 0.01), (512, 64, 0.02), (512, 64, 0.01)]
COLD_ROW = 7
BITS_CASE = (65, 64, 0.2)                  # b_cos=True at a temperature the old path keeps: bit equality with ops.InfoNceFn


def raw_group(c):
    return "hot" if c[3] == "big" or (c[2] <= 0.05 and c[1] >= 128) else "ordinary"


@functools.lru_cache(maxsize=None)
def raw_case(index):
    n, d, tau, family = RAW_CASES[index]
    g = torch.Generator().manual_seed(6270 + index)
    v1, v2 = 0.3 * torch.randn(n, d, generator=g), 0.3 * torch.randn(n, d, generator=g)
    if family == "big":
        top = float((v1.double() @ v2.double().T).abs().max()) / tau
        k = (RAW_BIG_LOGIT / top) ** 0.5
        v1, v2 = v1 * k, v2 * k
    return v1, v2


@functools.lru_cache(maxsize=None)
def raw_reference(index, dtype=torch.float64):
    n, d, tau, family = RAW_CASES[index]
    return infonce_raw(*raw_case(index), tau, False, dtype)


@functools.lru_cache(maxsize=None)
def unit_case(index):
    n, d, tau = UNIT_CASES[index] if index >= 0 else BITS_CASE
    g = torch.Generator().manual_seed(7270 + index)
    v1 = torch.randn(n, d, generator=g)
    v2 = torch.randn(n, d, generator=g).abs() + 0.01
    v1[COLD_ROW] = -(v1[COLD_ROW].abs() + 0.01)
    return v1, v2


@functools.lru_cache(maxsize=None)
def unit_reference(index, dtype=torch.float64):
    n, d, tau = UNIT_CASES[index]
    return infonce_raw(*unit_case(index), tau, True, dtype)


# ======================================================================================================================
# row kernels: bounds
# ======================================================================================================================
# Yardsticks: what the reference's own expressions give in f32 torch autograd on the CPU against this file, the largest
# scaled error over every case, family and upstream gradient below (test_losssurface_ref_cpu.py re-measures them).
#   loss     |loss - loss64| / max(|loss64|, 1)
#   triplet  a gradient row over (2 |gout| / B) max(|u - p|_inf, |u - n|_inf)
#   kl       a gradient element over (|gout| / R) max(1, |lp - lq|_inf of the row)
TRIPLET_LOSS_YARDSTICK = 2.5e-6
TRIPLET_ROW_YARDSTICK = 2.2e-7
KL_LOSS_YARDSTICK = 1.7e-7
KL_ELEM_YARDSTICK = 2.5e-7
TRIPLET_LOSS_BOUND = MARGIN * TRIPLET_LOSS_YARDSTICK
TRIPLET_ROW_BOUND = MARGIN * TRIPLET_ROW_YARDSTICK
KL_LOSS_BOUND = MARGIN * KL_LOSS_YARDSTICK
KL_ELEM_BOUND = MARGIN * KL_ELEM_YARDSTICK

# ---- triplet --------------------------------------------------------------------------------------------------------------
TRIPLET_MARGIN = 0.5
TRIPLET_FAMILIES = ("ordinary", "inactive", "active", "kink")
MIN_ABS_X = 1e-3                # every row of every case keeps |x| >= this: f32 and f64 agree on which rows are active
KINK_AT = 1e-3 + 2e-6           # the kink family's |x|: 1e-3, and 2e-6 so that rounding u to float32 (x moves by some
                                # 1e-7) cannot bring a row under MIN_ABS_X


def triplet(u, p, n, gout, margin=TRIPLET_MARGIN):
    """loss_torch.py:12-16 in float64 from (B, d) operands: the margins x, the loss, the gradients of gout * loss (exact
    zeros on rows with x <= 0) and per row the scale (2 |gout| / B) max(|u - p|_inf, |u - n|_inf)"""
    U, P, N = _f64(u), _f64(p), _f64(n)
    B = U.shape[0]
    x = ((U - P) ** 2).sum(1) - ((U - N) ** 2).sum(1) + margin
    act = (x > 0.0)[:, None]
    k = 2.0 * float(gout) / B
    s = (2.0 * abs(float(gout)) / B) * np.maximum(np.abs(U - P).max(1), np.abs(U - N).max(1))
    return {"x": x, "loss": float(np.maximum(x, 0.0).mean()), "gu": np.where(act, k * (N - P), 0.0),
            "gp": np.where(act, -k * (U - P), 0.0), "gn": np.where(act, k * (U - N), 0.0), "s": s}


@functools.lru_cache(maxsize=None)
def triplet_case(B, d, family, seed=0):
    """Read-only f32 (u, p, n).  Every family starts from N(0, 0.3^2) rows; a row is moved ALONG u by t (n - p), which moves
    x by 2 t |n - p|^2 exactly and nothing else, to its target: inactive uniform in [-3, -0.5], active uniform in [0.5, 3],
    kink +-KINK_AT in turn; ordinary rows stay where they fall unless |x| < 4 MIN_ABS_X (then to 4 MIN_ABS_X, sign kept)."""
    rng = np.random.default_rng([seed, B, d, 40 + TRIPLET_FAMILIES.index(family)])
    u, p, n = ((rng.standard_normal((B, d)) * 0.3).astype(np.float32) for _ in range(3))
    u64, v = _f64(u), _f64(n) - _f64(p)
    x0 = triplet(u, p, n, 1.0)["x"]
    lo = rng.uniform(0.5, 3.0, B)
    target = {"ordinary": np.where(np.abs(x0) < 4 * MIN_ABS_X, np.where(x0 < 0, -4 * MIN_ABS_X, 4 * MIN_ABS_X), x0),
              "inactive": -lo, "active": lo, "kink": np.where(np.arange(B) % 2 == 0, KINK_AT, -KINK_AT)}[family]
    u64 += ((target - x0) / (2.0 * (v * v).sum(1)))[:, None] * v
    out = (u64.astype(np.float32), p, n)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def triplet_reference(B, d, family, gout):
    return triplet(*triplet_case(B, d, family), gout)


def all_triplet_cases():
    for B, d in bpr_shapes():
        for family in TRIPLET_FAMILIES:
            yield B, d, family


# ---- kl ---------------------------------------------------------------------------------------------------------------------
# (R, C): R in {1, 3, 64, 515} (four rows per workgroup: 3 leaves a wave idle, 515 ends on 3), C in {1, 2, 63, 64, 65, 257,
# 1000, 5000} (one wave per row: 63 / 64 / 65 around one column per lane); every R and every C at least twice.
KL_SHAPES = [(1, 1), (3, 1), (1, 2), (64, 2), (3, 63), (515, 63), (1, 64), (64, 64), (3, 65), (515, 65), (64, 257), (1, 257),
             (515, 1000), (3, 1000), (64, 5000), (1, 5000)]
KL_FAMILIES = ("ordinary", "saturated", "underflow")


def kl(a, b, gout):
    """loss_torch.py:91-94 in float64: per row kl_r, the loss, both gradients of gout * loss and per row the scale
    (|gout| / R) max(1, |lp - lq|_inf).  A column with p_c == 0 contributes 0 (lp - lq is finite here)."""
    A, Bq = _f64(a), _f64(b)
    R = A.shape[0]
    lp = A - A.max(1, keepdims=True)
    lp = lp - np.log(np.exp(lp).sum(1, keepdims=True))
    lq = Bq - Bq.max(1, keepdims=True)
    lq = lq - np.log(np.exp(lq).sum(1, keepdims=True))
    p, q = np.exp(lp), np.exp(lq)
    dl = lp - lq
    rows = (p * dl).sum(1)
    k = float(gout) / R
    s = (abs(float(gout)) / R) * np.maximum(1.0, np.abs(dl).max(1))
    return {"rows": rows, "loss": float(rows.mean()), "ga": k * p * (dl - rows[:, None]), "gb": k * (q - p),
            "s": np.broadcast_to(s[:, None], A.shape), "p": p, "dl": dl}


@functools.lru_cache(maxsize=None)
def kl_case(R, C, family, seed=0):
    """Read-only f32 (p_logit, q_logit).  ordinary: N(0, 1) logits (the q side 2 N(0, 1)).  saturated: both sides uniform in
    [-100, 100], so all but a few p_c of a row are exactly 0 in float32 and 1e-40 or less in float64.  underflow: ordinary,
    and q_logit[r, r % C] += 200 (C > 1): log q_c is near -200 on every other column, where p_c is not small."""
    rng = np.random.default_rng([seed, R, C, 80 + KL_FAMILIES.index(family)])
    if family == "saturated":
        a, b = rng.uniform(-100.0, 100.0, (R, C)), rng.uniform(-100.0, 100.0, (R, C))
    else:
        a, b = rng.standard_normal((R, C)), 2.0 * rng.standard_normal((R, C))
        if family == "underflow" and C > 1:
            b[np.arange(R), np.arange(R) % C] += 200.0
    out = (a.astype(np.float32), b.astype(np.float32))
    for x in out:
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def kl_reference(R, C, family, gout):
    return kl(*kl_case(R, C, family), gout)


def all_kl_cases():
    for R, C in KL_SHAPES:
        for family in KL_FAMILIES:
            yield R, C, family
