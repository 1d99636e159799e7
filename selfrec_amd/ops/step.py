"""The training step outside the products (csrc/losses.hip, optim.hip, loader.cpp, exchange.hip): BPR, L2, InfoNCE, Adam,
the batch cursor / fetch / zeroing and the batch-row exchange of column-sharded tables."""
from __future__ import annotations

import ctypes as C

import torch

from ._base import SelfrecHipError, _lib, _p, _stream, check



def bpr_ws(batch: int, device):
    return torch.empty(int(_lib.load().srh_bpr_ws_bytes(batch)), dtype=torch.uint8, device=device)


def _segments(seg, nce_rows):
    """srh_batch_segments_t from a dict of device int32 tensors: n_uniq_u, n_uniq_i, n_uniq_n, seg_rows, seg_end, seg, seg_a, seg_b
    [, batch_no: the arrays are then EPOCH arrays] [, rows_are_zero: bool]."""
    g = _lib.BatchSegments()
    for k in ("n_uniq_u", "n_uniq_i", "n_uniq_n", "seg_rows", "seg_end", "seg", "seg_a", "seg_b"):
        setattr(g, "d_" + k, _p(seg[k], torch.int32))
    g.d_batch_no = _p(seg.get("batch_no"), torch.int32)
    g.nce_rows = int(nce_rows)
    g.rows_are_zero = int(bool(seg.get("rows_are_zero", False)))
    return g


def _bpr_problem(user, item, reg_user, reg_item, u_idx, i_idx, j_idx, batch, n_rows_dev, reg_coef, reg_include_neg, loss_scale,
                 g_user, g_item, greg_user, greg_item, losses, ws, seg, nce_rows):
    b = _lib.BprProblem()
    b.d_user, b.d_item = _p(user, torch.float32), _p(item, torch.float32)
    b.d_reg_user, b.d_reg_item = _p(reg_user, torch.float32), _p(reg_item, torch.float32)
    b.d_u_idx, b.d_i_idx, b.d_j_idx = _p(u_idx, torch.int32), _p(i_idx, torch.int32), _p(j_idx, torch.int32)
    b.B, b.d_n_rows = int(batch), _p(n_rows_dev, torch.int32)
    b.reg_coef, b.reg_include_neg, b.loss_scale = float(reg_coef), int(bool(reg_include_neg)), float(loss_scale)
    b.d_g_user, b.d_g_item = _p(g_user, torch.float32), _p(g_item, torch.float32)
    b.d_greg_user, b.d_greg_item = _p(greg_user, torch.float32), _p(greg_item, torch.float32)
    b.d_losses, b.d_ws = _p(losses, torch.float64), _p(ws)
    if seg is not None:
        b._seg = _segments(seg, nce_rows)          # (kept alive by the struct object)
        b.seg = C.pointer(b._seg)
    return b


def bpr_l2_fwd_bwd(user, item, reg_user, reg_item, u_idx, i_idx, j_idx, *, batch, n_rows_dev=None, reg_coef,
                   reg_include_neg, loss_scale, g_user, g_item, greg_user, greg_item, losses, ws, seg=None):
    """seg: the batch's row -> slot lists (see _segments): the gradients are summed row by row in slot order, no float atomics."""
    d = int(user.shape[1])
    if seg is not None:
        b = _bpr_problem(user, item, reg_user, reg_item, u_idx, i_idx, j_idx, batch, n_rows_dev, reg_coef, reg_include_neg,
                         loss_scale, g_user, g_item, greg_user, greg_item, losses, ws, seg, 0)
        check(_lib.load().srh_bpr_l2_fwd_bwd_p(C.byref(b), d, _stream()), "srh_bpr_l2_fwd_bwd_p")
        return
    check(_lib.load().srh_bpr_l2_fwd_bwd(
        _p(user, torch.float32), _p(item, torch.float32), _p(reg_user, torch.float32), _p(reg_item, torch.float32),
        _p(u_idx, torch.int32), _p(i_idx, torch.int32), _p(j_idx, torch.int32), int(batch),
        _p(n_rows_dev, torch.int32), d, float(reg_coef), int(bool(reg_include_neg)), float(loss_scale),
        _p(g_user, torch.float32), _p(g_item, torch.float32), _p(greg_user, torch.float32),
        _p(greg_item, torch.float32), _p(losses, torch.float64), _p(ws), _stream()), "srh_bpr_l2_fwd_bwd")


_scalar_ws = {}


def scalar_ws(device) -> torch.Tensor:
    """The 64-byte workspace the single-launch loss kernels finish their scalars in (SRH_SCALAR_WS_BYTES): one per device and
    stream, zero before its first use, left zero by every call."""
    # (one per device AND stream: the calls that share a workspace must be ordered, and a stream is what orders them)
    key = (device.index if device.index is not None else torch.cuda.current_device(), _stream())
    ws = _scalar_ws.get(key)
    if ws is None:
        ws = _scalar_ws[key] = torch.zeros(_lib.SCALAR_WS_BYTES // 8, dtype=torch.float64, device=device)
    return ws


def bpr_fwd(u, p, n, loss, coef):
    """loss (0-dim f32) = mean BPR loss of the rows; coef[b] = d loss / d (pos_b - neg_b).  One launch."""
    check(_lib.load().srh_bpr_fwd(_p(u, torch.float32), _p(p, torch.float32), _p(n, torch.float32), u.shape[0],
                                  int(u.shape[1]), scalar_ws(u.device).data_ptr(), _p(loss, torch.float32),
                                  _p(coef, torch.float32), _stream()), "srh_bpr_fwd")


def bpr_bwd(u, p, n, coef, gout, gu, gp, gn):
    """gout: the upstream gradient as a 0-dim f32 DEVICE tensor (read by the kernel: no host synchronisation)."""
    check(_lib.load().srh_bpr_bwd(_p(u, torch.float32), _p(p, torch.float32), _p(n, torch.float32),
                                  _p(coef, torch.float32), u.shape[0], int(u.shape[1]), _p(gout, torch.float32, "gout"),
                                  _p(gu, torch.float32), _p(gp, torch.float32), _p(gn, torch.float32), _stream()),
          "srh_bpr_bwd")


def _l2_blocks(xs, gxs=None):
    arr = (_lib.L2Block * len(xs))()
    for k, x in enumerate(xs):
        arr[k].d_x, arr[k].rows, arr[k].cols = _p(x, torch.float32, "emb"), int(x.shape[0]), int(x.shape[1])
        arr[k].d_gx = _p(gxs[k], torch.float32, "grad") if gxs is not None else None
    return arr


def l2_reg_fwd(xs, reg, norms, loss):
    """loss (0-dim f32) = reg * sum_k ||xs[k]||_F / rows_k; norms[k] = ||xs[k]||_F.  1..4 blocks of rows, one launch."""
    check(_lib.load().srh_l2_reg_fwd(_l2_blocks(xs), len(xs), float(reg), scalar_ws(xs[0].device).data_ptr(),
                                     _p(norms, torch.float32), _p(loss, torch.float32), _stream()), "srh_l2_reg_fwd")


def l2_reg_bwd(xs, reg, norms, gout, gxs):
    check(_lib.load().srh_l2_reg_bwd(_l2_blocks(xs, gxs), len(xs), float(reg), _p(norms, torch.float32),
                                     _p(gout, torch.float32, "gout"), _stream()), "srh_l2_reg_bwd")


# SRH_NCE_SPLIT16, SRH_NCE_F32 (include/selfrec_hip.h); "bf16x3" is the round-1/2 name of the split mode, kept as an alias
NCE_PRECISIONS = {"split": 0, "f32": 1, "bf16x3": 0}
NCE_DEFAULT = -1               # SRH_NCE_DEFAULT: the process default (f32 unless srh_infonce_set_precision / SRH_NCE_SPLIT16 says otherwise)


def _nce_mode(precision):
    """None -> the process default; 'split' | 'f32' -> that arithmetic for this call only."""
    if precision is None:
        return NCE_DEFAULT
    if precision not in NCE_PRECISIONS:
        raise SelfrecHipError(f"InfoNCE precision {precision!r}: one of {sorted(NCE_PRECISIONS)}")
    return NCE_PRECISIONS[precision]


def set_infonce_precision(mode: str):
    """'f32' (the default: every multiply-add of InfoNCE's two n x n x d products on the f32 MFMA, the reference's
    arithmetic) or 'split' (operands as short sums of 16-bit pieces on the 16-bit MFMA pipe -- logits on scaled f16 hi + lo,
    accurate to 2^-22 like an f32 dot product; P.V on bf16 pieces: ~10 us per step faster at the Yelp2018 shape).
    The process DEFAULT: what calls that name no precision run on (the loss mirrors of the op-level tier); a trainer
    carries its own mode and passes it with every call (engine.FusedTrainer.nce_precision)."""
    if mode not in NCE_PRECISIONS:
        raise SelfrecHipError(f"InfoNCE precision {mode!r}: one of {sorted(NCE_PRECISIONS)}")
    check(_lib.load().srh_infonce_set_precision(NCE_PRECISIONS[mode]), "srh_infonce_set_precision")


def get_infonce_precision() -> str:
    return {0: "split", 1: "f32"}[int(_lib.load().srh_infonce_get_precision())]


NCE_F32_MAX_N = 65536          # the all-f32 passes: 16 key ranges of at most 128 blocks of 32 keys


def infonce_plan(ns, slots: int) -> dict:
    """The task cut of the all-f32 passes for problems of ns live rows on `slots` workgroups (srh_infonce_plan: host only,
    nothing is launched): dict(n, per, splits: one entry per problem; first: len(ns) + 1 running task counts; tasks)."""
    ns = [int(n) for n in ns]
    arr = (C.c_int32 * max(len(ns), 1))(*ns)
    out = (C.c_int32 * 17)()
    check(_lib.load().srh_infonce_plan(C.cast(arr, C.c_void_p), len(ns), int(slots), C.cast(out, C.c_void_p)),
          "srh_infonce_plan")
    k = len(ns)
    return dict(n=list(out[0:k]), per=list(out[4:4 + k]), splits=list(out[8:8 + k]), first=list(out[12:13 + k]),
                tasks=int(out[16]))


def infonce_ws(n: int, d: int, device):
    return torch.empty(int(_lib.load().srh_infonce_ws_bytes(n, d)), dtype=torch.uint8, device=device)


def infonce_fwd_bwd(v1, v2, idx, n, *, n_dev=None, tau, loss_scale, loss, g1, g2, ws):
    d = int(v1.shape[1])
    need = int(_lib.load().srh_infonce_ws_bytes(n, d))
    if ws.numel() * ws.element_size() < need:
        raise SelfrecHipError(f"infonce workspace too small: {ws.numel() * ws.element_size()} < {need}")
    check(_lib.load().srh_infonce_fwd_bwd(_p(v1, torch.float32), _p(v2, torch.float32), _p(idx, torch.int32), int(n),
                                          _p(n_dev, torch.int32), d, float(tau), float(loss_scale),
                                          _p(loss, torch.float64), _p(g1, torch.float32), _p(g2, torch.float32),
                                          _p(ws), _stream()), "srh_infonce_fwd_bwd")


def _infonce_problems(problems, d, ws):
    """[(v1, v2, idx, n_max, n_dev, g1, g2[, g2_exclusive]), ...] -> srh_infonce_problem_t[]; ws must hold them all."""
    lib = _lib.load()
    arr = (_lib.InfonceProblem * len(problems))()
    need = 0
    for k, (v1, v2, idx, n, n_dev, g1, g2, *rest) in enumerate(problems):
        arr[k].d_v1, arr[k].d_v2 = _p(v1, torch.float32), _p(v2, torch.float32)
        arr[k].d_idx, arr[k].n, arr[k].d_n = _p(idx, torch.int32), int(n), _p(n_dev, torch.int32)
        arr[k].d_g1, arr[k].d_g2 = _p(g1, torch.float32), _p(g2, torch.float32)
        arr[k].g2_exclusive = int(bool(rest[0])) if rest else 0
        need += int(lib.srh_infonce_ws_bytes(n, d))
    if ws.numel() * ws.element_size() < need:
        raise SelfrecHipError(f"infonce workspace too small: {ws.numel() * ws.element_size()} < {need}")
    return arr


def infonce_multi(problems, *, d, tau, loss_scale, loss, ws, precision=None):
    """problems: [(v1, v2, idx, n_max, n_dev, g1, g2[, g2_exclusive]), ...] evaluated by one set of launches."""
    lib = _lib.load()
    arr = (_lib.InfonceProblem * len(problems))()
    need = 0
    for k, (v1, v2, idx, n, n_dev, g1, g2, *rest) in enumerate(problems):
        arr[k].d_v1, arr[k].d_v2 = _p(v1, torch.float32), _p(v2, torch.float32)
        arr[k].d_idx, arr[k].n, arr[k].d_n = _p(idx, torch.int32), int(n), _p(n_dev, torch.int32)
        arr[k].d_g1, arr[k].d_g2 = _p(g1, torch.float32), _p(g2, torch.float32)
        arr[k].g2_exclusive = int(bool(rest[0])) if rest else 0
        need += int(lib.srh_infonce_ws_bytes(n, d))
    if ws.numel() * ws.element_size() < need:
        raise SelfrecHipError(f"infonce workspace too small: {ws.numel() * ws.element_size()} < {need}")
    check(lib.srh_infonce_fwd_bwd_multi(arr, len(problems), int(d), float(tau), float(loss_scale),
                                        _p(loss, torch.float64), _p(ws), _nce_mode(precision), _stream()),
          "srh_infonce_fwd_bwd_multi")


def bpr_infonce(user, item, reg_user, reg_item, u_idx, i_idx, j_idx, *, batch, n_rows_dev=None, reg_coef,
                reg_include_neg, loss_scale, g_user, g_item, greg_user, greg_item, losses, bpr_ws,
                problems, tau, cl_scale, cl_loss, nce_ws, precision=None, seg=None, nce_rows=0, staged=False):
    """bpr_l2_fwd_bwd + infonce_multi with their O(batch) kernels sharing launches (srh_bpr_infonce_fwd_bwd).
    seg / nce_rows: the batch's row -> slot lists and how the problems name those rows (srh_batch_segments_t): every
    gradient row is then written once, by the row group that owns it, in slot order -- no float atomics.
    staged: an earlier product of the step carried spmm(..., nce_stage=(problems, nce_ws)) -- no prep launch
    (srh_bpr_infonce_fwd_bwd_staged: all-f32 arithmetic, d = 64 / 128)."""
    lib = _lib.load()
    d = int(user.shape[1])
    b = _bpr_problem(user, item, reg_user, reg_item, u_idx, i_idx, j_idx, batch, n_rows_dev, reg_coef, reg_include_neg,
                     loss_scale, g_user, g_item, greg_user, greg_item, losses, bpr_ws, seg, nce_rows)
    arr = (_lib.InfonceProblem * len(problems))()
    need = 0
    for k, (v1, v2, idx, n, n_dev, g1, g2, *rest) in enumerate(problems):
        arr[k].d_v1, arr[k].d_v2 = _p(v1, torch.float32), _p(v2, torch.float32)
        arr[k].d_idx, arr[k].n, arr[k].d_n = _p(idx, torch.int32), int(n), _p(n_dev, torch.int32)
        arr[k].d_g1, arr[k].d_g2 = _p(g1, torch.float32), _p(g2, torch.float32)
        arr[k].g2_exclusive = int(bool(rest[0])) if rest else 0
        need += int(lib.srh_infonce_ws_bytes(n, d))
    if nce_ws.numel() * nce_ws.element_size() < need:
        raise SelfrecHipError(f"infonce workspace too small: {nce_ws.numel() * nce_ws.element_size()} < {need}")
    if staged:
        if precision != "f32":
            raise SelfrecHipError("bpr_infonce(staged=True): the all-f32 passes only (precision='f32')")
        check(lib.srh_bpr_infonce_fwd_bwd_staged(C.byref(b), arr, len(problems), d, float(tau), float(cl_scale),
                                                 _p(cl_loss, torch.float64), _p(nce_ws), _stream()),
              "srh_bpr_infonce_fwd_bwd_staged")
        return
    check(lib.srh_bpr_infonce_fwd_bwd(C.byref(b), arr, len(problems), d, float(tau), float(cl_scale),
                                      _p(cl_loss, torch.float64), _p(nce_ws), _nce_mode(precision), _stream()),
          "srh_bpr_infonce_fwd_bwd")


def adam_step(param, grad, m, v, *, step=0, step_dev=None, lr, beta1=0.9, beta2=0.999, eps=1e-8, clear=None,
              row_mark=None, advance_cursor=None):
    """clear / row_mark / advance_cursor: the fused end-of-step reset (srh_adam_step_reset)."""
    if clear is not None or advance_cursor is not None:
        clear = list(clear or [])
        tables = (C.c_void_p * max(1, len(clear)))(*[_p(t, torch.float32, "clear") for t in clear])
        check(_lib.load().srh_adam_step_reset(_p(param, torch.float32), _p(grad, torch.float32), _p(m, torch.float32),
                                              _p(v, torch.float32), int(param.shape[0]), int(param.shape[1]),
                                              _p(step_dev, torch.int64), float(lr), float(beta1), float(beta2), float(eps),
                                              _p(row_mark, torch.int32), len(clear), tables,
                                              _p(advance_cursor, torch.int64), _stream()), "srh_adam_step_reset")
        return
    check(_lib.load().srh_adam_step(_p(param, torch.float32), _p(grad, torch.float32), _p(m, torch.float32),
                                    _p(v, torch.float32), param.numel(), int(step), _p(step_dev, torch.int64),
                                    float(lr), float(beta1), float(beta2), float(eps), _stream()), "srh_adam_step")


def axpby(a, x, b, y):
    check(_lib.load().srh_axpby(float(a), _p(x, torch.float32), float(b), _p(y, torch.float32), x.numel(), _stream()),
          "srh_axpby")
    return y


def cursor_advance(cursor):
    check(_lib.load().srh_cursor_advance(_p(cursor, torch.int64), _stream()), "srh_cursor_advance")


def zero_rows(lists, d, cursor_advance=None):
    """lists: [(table, idx, count_dev_or_None, n_max, row_offset), ...] (at most 8)."""
    n = len(lists)
    vp = C.c_void_p * n
    tables = vp(*[_p(t, torch.float32, "table") for t, *_ in lists])
    idx = vp(*[_p(i, torch.int32, "idx") for _, i, *_ in lists])
    cnt = vp(*[_p(c, torch.int32, "count") for _, _, c, *_ in lists])
    n_max = (C.c_int32 * n)(*[int(m) for *_, m, _ in lists])
    off = (C.c_int32 * n)(*[int(o) for *_, o in lists])
    check(_lib.load().srh_zero_rows(n, tables, idx, cnt, n_max, off, int(d), _p(cursor_advance, torch.int64),
                                    _stream()), "srh_zero_rows")


def batch_fetch_args(ep, n_edges, batch_size, cursor, stage, meta, row_mark=None, mark_item_offset=0, zero4=None,
                     stage_cat=None, cat_item_offset=0, n_cat=None, now=None, half_batches=0, adam_coef=None, adam_lr=0.0,
                     adam_beta1=0.9, adam_beta2=0.999):
    """srh_batch_fetch_args_t.  ep: dict of device int32 arrays for the epoch (two epochs back to back when half_batches >
    0); stage: dict of staging buffers.  adam_coef: float32[2] that receives this step's Adam constants (SRH_EPI_ADAM)."""
    a = _lib.BatchFetchArgs()
    a.d_epoch_u, a.d_epoch_i, a.d_epoch_j = (_p(ep[k], torch.int32) for k in ("u", "i", "j"))
    a.d_epoch_uniq_u, a.d_epoch_uniq_i = _p(ep.get("uniq_u"), torch.int32), _p(ep.get("uniq_i"), torch.int32)
    a.d_n_uniq_u, a.d_n_uniq_i = _p(ep.get("n_uniq_u"), torch.int32), _p(ep.get("n_uniq_i"), torch.int32)
    a.n_edges, a.batch_size, a.d_cursor = int(n_edges), int(batch_size), _p(cursor, torch.int64)
    a.d_stage_u, a.d_stage_i, a.d_stage_j = (_p(stage[k], torch.int32) for k in ("u", "i", "j"))
    a.d_stage_uniq_u, a.d_stage_uniq_i = _p(stage.get("uniq_u"), torch.int32), _p(stage.get("uniq_i"), torch.int32)
    a.d_meta, a.d_row_mark = _p(meta, torch.int32), _p(row_mark, torch.int32)
    a.mark_item_offset, a.cat_item_offset = int(mark_item_offset), int(cat_item_offset)
    a.d_zero4, a.d_stage_cat, a.d_n_cat = _p(zero4, torch.float64), _p(stage_cat, torch.int32), _p(n_cat, torch.int32)
    a.d_now = _p(now, torch.int64)
    a.half_batches = int(half_batches)
    a.d_adam_coef = _p(adam_coef, torch.float32)
    a.adam_lr, a.adam_beta1, a.adam_beta2 = float(adam_lr), float(adam_beta1), float(adam_beta2)
    a._keepalive = [ep, cursor, stage, meta, row_mark, zero4, stage_cat, n_cat, now, adam_coef]
    return a


def batch_fetch(*args, **kwargs):
    """srh_batch_fetch: same arguments as batch_fetch_args (or one prebuilt BatchFetchArgs)."""
    a = args[0] if len(args) == 1 and isinstance(args[0], _lib.BatchFetchArgs) else batch_fetch_args(*args, **kwargs)
    check(_lib.load().srh_batch_fetch(C.byref(a), _stream()), "srh_batch_fetch")


# ----------------------------------------------------------------------------------------
# (e) column-sharded tables: the batch-row exchange around the loss section (csrc/exchange.hip)
# ----------------------------------------------------------------------------------------
def batch_lists(stage, meta, batch_size):
    """struct srh_batch_lists over the staging buffers of batch_fetch: (u, i, j, uniq_u, uniq_i) with
    their device-side counts (meta[0] for the pair lists, meta[1], meta[2])."""
    bl = _lib.BatchLists()
    keep = []
    for s, (name, cnt) in enumerate((("u", 0), ("i", 0), ("j", 0), ("uniq_u", 1), ("uniq_i", 2))):
        c = meta[cnt:cnt + 1]
        bl.d_idx[s] = _p(stage[name], torch.int32, name)
        bl.d_count[s] = _p(c, torch.int32, "count")
        keep += [stage[name], c]
    bl.B = int(batch_size)
    bl._keepalive = keep
    return bl


def _ptr_array(tensors, name):
    return (C.c_void_p * len(tensors))(*[_p(t, torch.float32, name) for t in tensors])


def batch_pack(lists, tables, send, cat_idx=None, n_cat=None):
    dl = int(tables[0].shape[1])
    rows = 5 * lists.B
    if send.numel() < len(tables) * rows * dl or any(int(t.shape[1]) != dl for t in tables):
        raise SelfrecHipError("batch_pack: send buffer too small / tables of different widths")
    check(_lib.load().srh_batch_pack(C.byref(lists), len(tables), _ptr_array(tables, "table"), dl,
                                     _p(send, torch.float32, "send"), _p(cat_idx, torch.int32, "cat_idx"),
                                     _p(n_cat, torch.int32, "n_cat"), _stream()), "srh_batch_pack")


def batch_unpack(lists, recv, world, dl, compact, compact_grads):
    check(_lib.load().srh_batch_unpack(C.byref(lists), len(compact), int(world), int(dl),
                                       _p(recv, torch.float32, "recv"), _ptr_array(compact, "compact"),
                                       len(compact_grads), _ptr_array(compact_grads, "compact_grad") if compact_grads else None,
                                       _stream()), "srh_batch_unpack")


def batch_scatter(lists, pairs, d_full, col0, dl):
    """pairs: [(compact gradient (5B, d_full), local gradient (N, dl)), ...]"""
    check(_lib.load().srh_batch_scatter(C.byref(lists), len(pairs), _ptr_array([c for c, _ in pairs], "compact_grad"),
                                        _ptr_array([g for _, g in pairs], "local_grad"), int(d_full), int(col0), int(dl),
                                        _stream()), "srh_batch_scatter")
