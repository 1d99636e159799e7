"""Cases and restatements for the edge tests of the SSL4Rec tower kernels and the segment sum (DESIGN.md 4.16;
csrc/ssl4rec.hip) -- TEST INFRASTRUCTURE ONLY, no GPU needed; the product never imports this module.

    weights / case          seeded weight families (init, hot, dead) at Linear(64, 1024) -> Linear(1024, 128), a table of
                            50 rows, ids from 0..39 with one foreign id for n >= 3, an upstream gradient
    routes / route_keep     no mask; an injected and a drawn mask at mask_row0 in {0, n // 3, n - 1}: both carry the mask
                            the counter RNG draws at counters that cross 2^32
    tower_math              y and every gradient (dX, table, W1, b1, W2, b2) written out by hand, float64 by default, under
                            an optional ReLU pattern; dtype=torch.float32 gives the same expressions in plain f32, and
                            ``defect`` plants one of DEFECTS
    relu_band               the width around z = 0 inside which f32 may decide a unit differently from float64
    figures                 the figures the bounds are set on (BOUNDS): whole tensors, and rows through row_errors
    segment_sum_f32         the float32 host restatement of seg_sum: per segment and column, terms in plan order
    segment_problem         the hand-made plans of the stand-alone segment-sum tests

tests/test_tower_ref_cpu.py checks the premises of everything here; tests/test_gpu_tower_edges.py runs the kernels."""
import functools

import numpy as np
import torch

from tests import ssl4rec_ref
from tests.contrastive_ref import FLOOR_FRAC, row_errors

D_IN, D_HID, D_OUT = 64, 1024, 128
ROW_CHUNK = 256                                  # kRowChunk of csrc/ssl4rec.hip
ROWS = [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 513]          # 513: three chunks, the last of one row
FAMILIES = ("init", "hot", "dead")
N_TABLE, ID_HI = 50, 40                          # rows 40..49 are never named
DROP_P = 0.1
DROP_SCALE = np.float32(1.0) / (np.float32(1.0) - np.float32(DROP_P))       # the kernel's 1.f / (1.f - p)
HOT_AMP, HOT_B2 = 0.4, 3.0
DEAD_SHIFT = 0.12                                # b1 -= this: 6.5 .. 8.8 % of the units stay alive
ZERO_BIAS = np.arange(0, D_HID, 32)              # dead: b1 exactly 0 here
ALWAYS_DEAD = np.array([5, 100, 333, 641, 1023])  # dead: b1 = -50 here (|W1 x| <= 64 * 0.08 * max|x| stays below 10)
FOREIGN = {"init": N_TABLE + 3, "hot": -1, "dead": N_TABLE + 3}
NONE_ROWS = (1, 64, 65, 257)                     # the idx=None (full-table) cases

Y_TOL, GRAD_TOL = 1e-5, 1e-4                     # of the tensor's largest magnitude; GRAD_TOL per row too
GRADS = ("gx", "gt", "gw1", "gb1", "gw2", "gb2")
ROW_KEYS = ("gx", "gt", "gw1", "gw2")            # measured per row as well (gw1 / gw2: per weight row)
BOUNDS = dict(y=Y_TOL, **{k: GRAD_TOL for k in GRADS}, **{k + "_row": GRAD_TOL for k in ROW_KEYS})
DEFECTS = ("relu_ge", "tail_chunk", "mask_scale_last", "foreign_row0")


# ---- cases ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def weights(family, seed):
    """(W1, b1, W2, b2) float32.  init: uniform +-0.08 / +-0.05.  hot: uniform +-HOT_AMP (b2 +-HOT_B2), so that a sizeable
    share of the outputs saturates.  dead: init with b1 - DEAD_SHIFT, exact zeros at ZERO_BIAS, -50 at ALWAYS_DEAD."""
    g = torch.Generator().manual_seed(1000 + seed)
    u = lambda shape, a: (torch.rand(shape, generator=g) * 2.0 - 1.0) * a  # noqa: E731
    if family == "hot":
        w1, b1, w2, b2 = u((D_HID, D_IN), HOT_AMP), u((D_HID,), HOT_AMP), u((D_OUT, D_HID), HOT_AMP), u((D_OUT,), HOT_B2)
    else:
        w1, b1, w2, b2 = u((D_HID, D_IN), 0.08), u((D_HID,), 0.05), u((D_OUT, D_HID), 0.08), u((D_OUT,), 0.05)
    if family == "dead":
        b1 = b1 - DEAD_SHIFT
        b1[torch.from_numpy(ZERO_BIAS)] = 0.0
        b1[torch.from_numpy(ALWAYS_DEAD)] = -50.0
    return tuple(t.float().contiguous() for t in (w1, b1, w2, b2))


def foreign_row(n):
    return n // 2 if n >= 3 else None


@functools.lru_cache(maxsize=None)
def case(n, family, gathered=True):
    """dict(n, family, table (N x 64), ids (n,) int64 or None, w, gy (n x 128), foreign: the row with the foreign id or
    None).  gathered=False: the full-table pass, a table of n rows and no ids."""
    g = torch.Generator().manual_seed(7 * n + FAMILIES.index(family) + (0 if gathered else 100000))
    table = torch.randn(N_TABLE if gathered else n, D_IN, generator=g) * 0.2
    ids = None
    if gathered:
        ids = torch.randint(0, ID_HI, (n,), generator=g)
        if foreign_row(n) is not None:
            ids[foreign_row(n)] = FOREIGN[family]
    gy = torch.randn(n, D_OUT, generator=g)
    return dict(n=n, family=family, table=table, ids=ids, w=weights(family, n), gy=gy,
                foreign=foreign_row(n) if gathered else None)


def routes(n):
    """[(kind, mask_row0)]: ("none", None), then ("injected", r) and ("drawn", r) for r in {0, n // 3, n - 1}"""
    out = [("none", None)]
    for r in sorted({0, n // 3, n - 1}):
        out += [("injected", r), ("drawn", r)]
    return out


def rng_args(n, row0):
    """(seed, counter) of the drawn route: the seed's high word is non-zero; the masked rows' counters counter .. counter +
    (n - row0) - 1 end at or past 2^32 - 1, and with two rows or more lie on both sides of 2^32"""
    seed = 0x5EED_0123_4567 + 0x1_0000_0000 * n + row0
    return seed, (1 << 32) - max(1, (n - row0) // 2)


@functools.lru_cache(maxsize=None)
def route_keep(n, row0):
    """(n - row0, 64) bool: the keep mask of both masked routes, the host restatement of what the kernel draws"""
    seed, ctr = rng_args(n, row0)
    return ssl4rec_ref.dropout_keep(seed, ctr, n - row0, DROP_P)


def multiplier(n, row0):
    """(n, 64) float32: 1 on unmasked rows, keep * DROP_SCALE on the others (0 where dropped)"""
    m = np.ones((n, D_IN), dtype=np.float32)
    if row0 is not None and row0 < n:
        m[row0:] = np.where(route_keep(n, row0), DROP_SCALE, np.float32(0))
    return m


def effective_input_f32(c, row0):
    """(n, 64) float32 numpy: f32(table[id]) * m in float32, zero rows for foreign ids: saved[0] bit for bit"""
    x, _ = _gather(c, torch.float32)
    return x.numpy() * multiplier(c["n"], row0)


def _gather(c, dtype, foreign_reads_row0=False):
    table = c["table"].to(dtype)
    if c["ids"] is None:
        return table.clone(), None
    ids = c["ids"]
    valid = (ids >= 0) & (ids < len(table))
    x = torch.where(valid[:, None], table[ids.clamp(0, len(table) - 1)], torch.zeros((), dtype=dtype))     # +0, never -0
    if foreign_reads_row0:
        x = torch.where(valid[:, None], x, table[0][None, :])
    return x, valid


# ---- the restatement ---------------------------------------------------------------------------------------------------
def tower_math(c, row0, pattern=None, dtype=torch.float64, defect=None):
    """dict(x, z, pattern, y, gx, gt, gw1, gb1, gw2, gb2) of y = tanh(W2 h + b2), h = relu(W1 x + b1), x = table[ids] * m,
    against the upstream c["gy"].  pattern (n, 1024) bool: h = z * pattern and the derivative follows it; None: torch's
    relu (alive where z > 0, derivative 0 at z = 0).  gx is the gradient w.r.t. the gathered rows (mask applied, a foreign
    row's included: it is the gradient w.r.t. the zero row read there); gt the table's, which foreign rows do not reach
    (gx itself without ids)."""
    assert defect is None or defect in DEFECTS
    n = c["n"]
    w1, b1, w2, b2 = (t.to(dtype) for t in c["w"])
    gy = c["gy"].to(dtype)
    m = torch.from_numpy(multiplier(n, row0)).to(dtype)
    x0, valid = _gather(c, dtype, foreign_reads_row0=defect == "foreign_row0")
    x = x0 * m
    z = x @ w1.T + b1
    if pattern is None:
        pattern = z > 0
    pattern = torch.as_tensor(pattern)
    h = z * pattern.to(dtype)
    y = torch.tanh(h @ w2.T + b2)
    dz2 = gy * (1.0 - y * y)
    alive = (z >= 0) if defect == "relu_ge" else pattern
    dz1 = (dz2 @ w2) * alive.to(dtype)
    mb = m
    if defect == "mask_scale_last" and row0 is not None and row0 < n:
        mb = m.clone()
        mb[n - 1] = (m[n - 1] != 0).to(dtype)
    gx = (dz1 @ w1) * mb
    top = n
    if defect == "tail_chunk" and n > ROW_CHUNK:
        top = (n - 1) // ROW_CHUNK * ROW_CHUNK
    gw1, gb1 = dz1[:top].T @ x[:top], dz1[:top].sum(0)
    gw2, gb2 = dz2[:top].T @ h[:top], dz2[:top].sum(0)
    if c["ids"] is None:
        gt = gx.clone()
    else:
        gt = torch.zeros_like(c["table"], dtype=dtype).index_add_(0, c["ids"][valid], gx[valid])
    return dict(x=x, z=z, pattern=pattern, y=y, gx=gx, gt=gt, gw1=gw1, gb1=gb1, gw2=gw2, gb2=gb2)


def relu_band(x64, w1, b1):
    """(n, 1024) float64: 2 * 65 * 2^-24 * (|x| |W1|^T + |b1|) -- the classical bound of a dot product of 64 products and
    a bias at unit roundoff 2^-24, doubled for the MFMA's unspecified internal order"""
    x64 = torch.as_tensor(x64).double()
    return 2.0 * 65.0 * 2.0 ** -24 * (x64.abs() @ w1.double().abs().T + b1.double().abs())


def flips(pattern, z64, band):
    """(share of units decided differently from float64, the largest |z64| / band among them (0 without any), units
    alive at z64 == 0)"""
    pattern = torch.as_tensor(pattern).cpu()
    diff = pattern != (z64 > 0)
    worst = float((z64.abs() / band.clamp_min(1e-300))[diff].max()) if bool(diff.any()) else 0.0
    return float(diff.double().mean()), worst, int((pattern & (z64 == 0)).sum())


def rel_max(got, want):
    got, want = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(want).detach().double().cpu()
    return float((got - want).abs().max() / (want.abs().max() + 1e-30))


def figures(got, want):
    """{name: figure} for every key of BOUNDS that ``got`` holds: y and the gradients against the tensor's largest
    magnitude, the _row entries the worst row of row_errors at FLOOR_FRAC"""
    out = {}
    for k in ("y",) + GRADS:
        if k in got:
            out[k] = rel_max(got[k], want[k])
            if k in ROW_KEYS:
                out[k + "_row"] = float(row_errors(got[k], want[k], FLOOR_FRAC).max())
    return out


def worst_ratio(figs):
    """the largest figure / bound"""
    return max(v / BOUNDS[k] for k, v in figs.items())


def show(figs):
    return " ".join(f"{k}={v:.2e}" for k, v in figs.items())


# ---- segment sum -------------------------------------------------------------------------------------------------------
def segment_sum_f32(x, plan, out, store=False):
    """out (n_table, d) float32 after seg_sum: per segment and column acc = f32(0), acc = f32(acc + x[order[p]]) for p
    ascending, out[row] = f32(out[row] + acc).  A seg_row outside the table skips the segment, an order entry outside x
    the term.  store=True plants the defect of a store in place of the add."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    order, seg_start, seg_row = (np.asarray(a, dtype=np.int64) for a in plan)
    out = np.array(out, dtype=np.float32, copy=True)
    for s, row in enumerate(seg_row):
        if not 0 <= row < len(out):
            continue
        acc = np.zeros(x.shape[1], dtype=np.float32)
        for p in range(seg_start[s], seg_start[s + 1]):
            r = order[p]
            if 0 <= r < len(x):
                acc = acc + x[r]                       # one float32 add per column
        out[row] = acc if store else out[row] + acc
    return out


def segment_sum_f64(x, plan, n_table):
    """what the plan adds, float64 (n_table, d), by index_add_"""
    order, seg_start, seg_row = (np.asarray(a, dtype=np.int64) for a in plan)
    rows = np.repeat(seg_row, np.diff(seg_start))
    ok = (rows >= 0) & (rows < n_table) & (order >= 0) & (order < len(x))
    out = torch.zeros(n_table, x.shape[1], dtype=torch.float64)
    return out.index_add_(0, torch.from_numpy(rows[ok]), torch.from_numpy(np.asarray(x, dtype=np.float64))[order[ok]]).numpy()


SEG_WIDTHS = (1, 63, 64, 65, 128, 200)
SEG_LENGTHS = (1, 2, 63, 64, 65, 1000)
SEG_TABLE = 12
SEG_LONG_ROW = 9                                 # the table row of the 1000-row segment


@functools.lru_cache(maxsize=None)
def segment_problem(d):
    """dict(x (n_rows, d) float32, plan (order, seg_start, seg_row) int32, named: the table rows some segment names,
    n_table).  Segments of SEG_LENGTHS rows in a shuffled order of x's rows, their table rows out of sequence; two more
    segments (3 and 2 rows) whose seg_row is -1 and n_table; four order entries of the real segments replaced by -1,
    n_rows, n_rows + 5 and -7.  x is randn (+2 on a single column, whose zero-mean sum would cancel)."""
    rs = np.random.RandomState(900 + d)
    lens = list(SEG_LENGTHS) + [3, 2]
    rows = [7, 0, 3, 11, 4, SEG_LONG_ROW, -1, SEG_TABLE]
    n_rows = sum(lens)
    x = (rs.randn(n_rows, d) + (2.0 if d == 1 else 0.0)).astype(np.float32)
    order = rs.permutation(n_rows).astype(np.int32)
    seg_start = np.r_[0, np.cumsum(lens)].astype(np.int32)
    for p, bad in ((seg_start[2] + 5, -1), (seg_start[3], n_rows), (seg_start[5] + 500, n_rows + 5), (seg_start[5] + 999, -7)):
        order[p] = bad
    plan = (order, seg_start, np.array(rows, dtype=np.int32))
    return dict(x=x, plan=plan, named=np.array(rows[:6]), n_table=SEG_TABLE)
