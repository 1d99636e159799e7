"""References and seeded cases for the edge tests of the table cross-entropy (csrc/contrastive.hip:
ce_pass, ce_finish, ce_loss) -- TEST INFRASTRUCTURE ONLY, no GPU needed.

    reference       bert4rec_ref.table_ce_grads as it is (float64, closed form), plus per row lse_m and lse_m - s_{m, label_m}
    f32_torch       the same expressions in plain float32 torch on the CPU: the yardstick of the floor and of every case
    figures         loss relative, lse / row terms per row against max(1, |lse|), gradients per row through
                    contrastive_ref.row_errors, each group of rows on its own scale
    ws_carve        ce_carve restated: where lse (float32, M) and row_loss (float64, M) lie in the caller's workspace
    cases           the shapes of bert4rec_ref.CE_SHAPES, the chunk layouts of LAYOUTS in three input families, and one call
                    with labels outside the table

tests/test_table_ce_ref_cpu.py checks the premises of every builder here; tests/test_gpu_table_ce_edges.py runs the kernel
on the cases.  Every builder is cached and its tensors are never written to."""
import functools

import torch

from tests import bert4rec_ref
from tests.contrastive_ref import CT_TILE, FLOORS, chunk_plan, row_errors

LOSS_TOL = 1e-5      # the loss against float64, relative
GRAD_TOL = 1e-4      # gradients against float64, per row through row_errors
LSE_TOL = 1e-5       # lse_m against max(1, |lse_m|); the row's loss term lse_m - s_pos against max(1, |lse_m|, |s_pos|)
# the smallest of FLOORS at which f32_torch stays within GRAD_TOL / 2 per row on every case of its group
# (test_table_ce_ref_cpu.py::test_floor_frac_is_the_smallest_that_float32_torch_meets asserts both).  The extreme family
# of bert4rec_ref.ce_case has a floor of its own: its logits of -105 and -130 carry an absolute float32 error of some
# 5e-5 (64 additions at a magnitude whose half ulp is 7.6e-6), which is the RELATIVE error of every P_mj of those rows
# and so of every row of gt they dominate -- float32 cannot hold such a row to 5e-5 of itself.
FLOOR_FRAC = 1e-2
FLOOR_FRAC_EXTREME = 1e-1

# ---- the chunk layouts: (M, N, d) and what chunk_plan must give for them ------------------------------------------------
LAYOUTS = [
    dict(shape=(8193, 300, 64), chunks=4, tiles=2, live=3, empty=1, last_keys=44),
    dict(shape=(4097, 513, 64), chunks=8, tiles=2, live=5, empty=3, last_keys=1),
    dict(shape=(16385, 500, 128), chunks=2, tiles=4, live=2, empty=0, last_keys=244),     # three tiles and 52 keys
    dict(shape=(16321, 200, 64), chunks=2, tiles=2, live=2, empty=0, last_keys=72),       # 16321 = 255 * 64 + 1
    dict(shape=(129, 21958, 64), chunks=171, tiles=3, live=115, empty=56, last_keys=70),
    dict(shape=(100, 16385, 64), chunks=256, tiles=2, live=129, empty=127, last_keys=1),  # M mod 16 = 4
    dict(shape=(1, 32833, 64), chunks=512, tiles=2, live=257, empty=255, last_keys=65),   # one full tile plus 1 key
    dict(shape=(2049, 1030, 100), chunks=16, tiles=2, live=9, empty=7, last_keys=6),      # through the padding to 128
]
FAMILIES = ("ordinary", "staircase", "spike")
STAIR_H = (40.0, -40.0, 100.0, -100.0, 0.0, 8.0, -8.0)      # h[m, 0] of row m is STAIR_H[m % 7]
SPIKE_H = (60.0, 0.0, -60.0)                                # h[m, 0] of row m is SPIKE_H[m % 3]
BAD_LABELS = dict(shape=(17, 130, 64), rows=(5, 11), values=(-1, 130))
DIRTY = (1, "staircase")                                    # the (4097, 513) staircase call
DIRTY_OTHER = ((300, 5000, 64), "extreme")                  # the call of another shape that uses the workspace in between
EXTREME_ROWS, EXTREME_KEYS = (0, 1, 3, 4), (0,)             # the planted rows of bert4rec_ref.ce_case's extreme family


def nz(mask):
    """the indices at which a 1-D tensor is non-zero"""
    return mask.nonzero().flatten()


def spike_keys(N):
    return sorted({0, 63, 64, 127, 128, N // 2, N - 1})


def key_place(j, M, N):
    """(chunk, tile inside the chunk) of key j in pass 1's schedule"""
    p = chunk_plan(M, N)
    return j // p["chunk_len"], j % p["chunk_len"] // CT_TILE


def make_labels(M, N, g):
    """labels drawn from the even keys only, so at least a third of the keys is named by nobody; planted (M >= 6): 0, the
    spike key N / 2, the first key of the last tile, a repeat; the last row always carries N - 1"""
    labels = 2 * torch.randint(0, (N + 1) // 2, (M,), generator=g)
    if M >= 6:
        labels[0], labels[1], labels[2] = 0, N // 2, (N - 1) // CT_TILE * CT_TILE
        labels[4] = labels[3]
    labels[-1] = N - 1
    return labels


def make_inputs(M, N, d, family, seed):
    """ordinary: as bert4rec_ref.ce_case -- rows of norm ~ sqrt(d), table entries ~ 0.05.
    staircase: column 0 of the table is j / N and h[m, 0] = STAIR_H[m % 7]; the other columns of h are scaled by 1 / N,
      which keeps their share of a logit (sigma 0.4 / N to 0.6 / N) below the step 8 / N between two KEYS of a +8 row, so
      that even a last tile of one key raises it: a positive row's maximum rises at every tile and every chunk, a negative
      row's stands in the first tile.
    spike: column 0 of the table is 1 at spike_keys(N) and 0 elsewhere, h[m, 0] = SPIKE_H[m % 3]: a +60 row has its
      largest logits at all the spike keys at once, a -60 row everywhere else."""
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(M, d, generator=g)
    table = 0.05 * torch.randn(N, d, generator=g)
    labels = make_labels(M, N, g)
    if family == "staircase":
        h[:, 1:] *= 1.0 / N
        table[:, 0] = (torch.arange(N, dtype=torch.float64) / N).float()
        h[:, 0] = torch.tensor(STAIR_H)[torch.arange(M) % len(STAIR_H)]
    elif family == "spike":
        table[:, 0] = 0.0
        table[spike_keys(N), 0] = 1.0
        h[:, 0] = torch.tensor(SPIKE_H)[torch.arange(M) % len(SPIKE_H)]
    elif family != "ordinary":
        raise ValueError(family)
    return h, table, labels


# ---- the case list ------------------------------------------------------------------------------------------------------
SHAPE_KEYS = [("shape", s, f) for s in bert4rec_ref.CE_SHAPES for f in bert4rec_ref.CE_FAMILIES]
LAYOUT_KEYS = [("layout", i, f) for i in range(len(LAYOUTS)) for f in FAMILIES]
BAD_KEY = ("bad_labels", 0, "ordinary")
ALL_KEYS = SHAPE_KEYS + LAYOUT_KEYS + [BAD_KEY]


def key_id(key):
    kind, which, family = key
    shape = which if kind == "shape" else (LAYOUTS[which]["shape"] if kind == "layout" else BAD_LABELS["shape"])
    return "%s-M%d_N%d_d%d-%s" % ((kind,) + tuple(shape) + (family,))


@functools.lru_cache(maxsize=None)
def case(key):
    """(h (M x d) float32, table (N x d) float32, labels (M,) int64) on the host"""
    kind, which, family = key
    if kind == "shape":
        return bert4rec_ref.ce_case(which, family)
    if kind == "layout":
        M, N, d = LAYOUTS[which]["shape"]
        return make_inputs(M, N, d, family, 9000 + 10 * which + FAMILIES.index(family))
    M, N, d = BAD_LABELS["shape"]
    h, table, labels = make_inputs(M, N, d, family, 9900)
    for r, v in zip(BAD_LABELS["rows"], BAD_LABELS["values"]):
        labels[r] = v
    return h, table, labels


def floor_of(key):
    return FLOOR_FRAC_EXTREME if key[2] == "extreme" else FLOOR_FRAC


def row_groups(key):
    """(groups of rows of h, groups of keys): each group's gradient rows are measured on their own scale.  The extreme
    family's planted rows (h[0, 0] = 60 ... -130 set the tensor's scale) and key 0 (table[0, 0] = 2) stand apart from the
    rest, as the clamped rows of DESIGN.md 4.15 do."""
    h, table, _ = case(key)
    M, N = len(h), len(table)
    if key[0] != "shape" or key[2] != "extreme":
        return [torch.arange(M)], [torch.arange(N)]

    def split(n, planted):
        m = torch.zeros(n, dtype=torch.bool)
        m[[r for r in planted if r < n]] = True
        return [idx for idx in (nz(m), nz(~m)) if len(idx)]
    return split(M, EXTREME_ROWS), split(N, EXTREME_KEYS)


def _row_terms(h, table, labels):
    """per row in the dtype of h: lse_m (max-subtracted) and lse_m - s_{m, label_m}; NaN where the label is outside"""
    s = h @ table.T
    mx = s.max(dim=1, keepdim=True).values
    lse = mx.squeeze(1) + torch.log(torch.exp(s - mx).sum(dim=1))
    ok = (labels >= 0) & (labels < len(table))
    pos = s[torch.arange(len(h)), labels.clamp(0, len(table) - 1)]
    nan = torch.full_like(lse, float("nan"))
    return lse, torch.where(ok, lse - pos, nan), torch.where(ok, pos, nan)


@functools.lru_cache(maxsize=None)
def reference(key):
    """float64: dict(loss, gh, gt, lse, row_loss) at loss_scale 1.  A label outside the table has no one-hot: its row's
    gradient is sum_j P_mj t_j, it takes nothing off any table row, and the loss is NaN."""
    h, table, labels = case(key)
    ok = (labels >= 0) & (labels < len(table))
    loss, gh, gt = bert4rec_ref.table_ce_grads(h, table, torch.where(ok, labels, torch.zeros_like(labels)))
    if not ok.all():                                   # put back the one-hots that label 0 took off in their place
        gh[~ok] += table[0].double()
        gt[0] += h[~ok].double().sum(dim=0)
        loss = float("nan")
    lse, row_loss, pos = _row_terms(h.double(), table.double(), labels)
    return dict(loss=loss, gh=gh, gt=gt, lse=lse, row_loss=row_loss, pos=pos)


def f32_torch(key):
    """the reference's expressions in plain float32 torch on the CPU, same dict"""
    h, table, labels = case(key)
    ok = (labels >= 0) & (labels < len(table))
    lse, row_loss, _ = _row_terms(h, table, labels)
    p = torch.softmax(h @ table.T, dim=1)
    rows = nz(ok)
    p[rows, labels[rows]] -= 1.0
    return dict(loss=float(row_loss.sum()), gh=p @ table, gt=p.T @ h, lse=lse, row_loss=row_loss)


def figures(got, key, floor_frac=None, scale=1.0):
    """dict(loss, lse, row, gh, gt): the worst figure of ``got`` (a dict as reference()'s, computed at loss_scale
    ``scale``) against float64.  loss: relative (NaN against NaN is 0).  lse: per row, |error| / max(1, |lse_m|).  row: per
    row, |error| / max(1, |lse_m|, |s_pos|); where the label is outside the table both must be NaN, else inf.  gh, gt:
    row_errors per group of row_groups, at the floor of the case's family unless one is given."""
    want = reference(key)
    floor_frac = floor_of(key) if floor_frac is None else floor_frac
    out = {}
    wl, gl = scale * want["loss"], float(got["loss"])
    out["loss"] = (0.0 if gl != gl else float("inf")) if wl != wl else abs(gl - wl) / abs(wl)
    den = want["lse"].abs().clamp_min(1.0)
    if "lse" in got:
        out["lse"] = float(((got["lse"].double().cpu() - want["lse"]).abs() / den).max())
        g, w = got["row_loss"].double().cpu(), want["row_loss"]
        bad = torch.isnan(w)
        den_row = torch.maximum(den, torch.nan_to_num(want["pos"].abs(), nan=1.0))
        err = torch.where(bad, torch.where(torch.isnan(g), 0.0, float("inf")).double(), (g - w).abs() / den_row)
        out["row"] = float(torch.nan_to_num(err, nan=float("inf")).max())
    for name, groups in zip(("gh", "gt"), row_groups(key)):
        g, w = got[name].detach().double().cpu(), scale * want[name]
        assert g.shape == w.shape, (name, g.shape, w.shape)
        worst = max(float(row_errors(g[idx], w[idx], floor_frac).max()) for idx in groups)
        out[name] = worst if worst == worst else float("inf")
    return out


# ---- ce_carve restated ------------------------------------------------------------------------------------------------
def _align256(n):
    return (n + 255) // 256 * 256


def ws_carve(M, N, D):
    """byte offsets of the workspace parts of srh_table_ce_fwd_bwd at the padded width D, and their total"""
    c = chunk_plan(M, N)["chunks"]
    out, cur = {}, 0
    for name, nbytes in (("part_o", 4 * c * M * D), ("part_rs", 8 * c * M), ("part_m", 4 * c * M), ("lse", 4 * M),
                         ("row_loss", 8 * M)):
        out[name] = cur
        cur += _align256(nbytes)
    out["total"] = cur
    return out


__all__ = ["FLOORS", "FLOOR_FRAC", "FLOOR_FRAC_EXTREME", "floor_of", "GRAD_TOL", "LOSS_TOL", "LSE_TOL", "LAYOUTS", "FAMILIES", "ALL_KEYS", "case",
           "reference", "f32_torch", "figures", "ws_carve", "chunk_plan", "key_place", "spike_keys", "row_groups"]
