"""The bootstrap family (csrc/bootstrap.hip): BUIR's and SelfCF's predictor, cosine terms against momentum-mixed targets,
every gradient and the history store in one call; and the momentum update of a table's batch rows."""
import ctypes as C

import torch

from ._base import (TABLE_NCE_WIDTHS, LossGradFn, SelfrecHipError, _lib, _p, _stream, check, cut_cols, kernel_width, to_width,
                    workspace)


def boot_supported(d) -> bool:
    """the row widths srh_boot_fwd_bwd serves once zero-padded: 1 .. 128 columns"""
    return 1 <= int(d) <= TABLE_NCE_WIDTHS[-1]


def _idx(idx, n, name):
    if idx is None:
        return None
    if idx.dim() != 1 or int(idx.shape[0]) != n:
        raise SelfrecHipError(f"boot_fwd_bwd: {name} must hold one id per row ({n})")
    _p(idx, None, name)
    return idx.to(torch.int32).contiguous()


def boot_fwd_bwd(x_u, x_i, W, b, tgt_u, tgt_i, idx_u=None, idx_i=None, store_u=None, store_i=None, alpha=1.0, beta=0.0,
                 eps=1e-12, c0=4.0, c1=2.0, cosine=False, ws=None):
    """The bootstrap loss (BUIR.py:87-95, SelfCF.py:64-91) of the online rows x_u, x_i (B x d), the predictor's W (d x d,
    nn.Linear's out x in) and b (d), with every gradient:
        t_side = alpha * tgt_side[idx_side] + beta * x_side          (tgt_side[r] with idx_side=None; no gradient)
        loss = c0 - c1 * (mean cos(W x_u + b, t_i) + mean cos(W x_i + b, t_u)),  each vector over max(its norm, eps)
    and, LAST, store_side[idx_side] = x_side where a store table is given (it may be tgt_side itself: every target was
    read before).  The defaults are BUIR's; SelfCF is (m, 1 - m, 1e-8, 1, 0.5, cosine=True) with its history tables as tgt
    and store.  cosine says how a prediction shorter than eps differentiates: False as x / max(|x|, eps) (F.normalize), True
    as F.cosine_similarity, which clamps the norm outside the graph (include/selfrec_hip.h (a-23)).
    Returns loss (float64 scalar), parts (2, float64: the two means), gx_u, gx_i (B x d), gw (d x d), gb (d).
    Any d up to 128: narrower rows, W and b are zero-padded, which changes no result (a padded table is a copy, and a
    store into it is copied back).  An id outside its table reads a zero row and stores nothing."""
    if x_u.dim() != 2 or tuple(x_i.shape) != tuple(x_u.shape):
        raise SelfrecHipError("boot_fwd_bwd: x_u and x_i must share one (B x d) shape")
    n, d = int(x_u.shape[0]), int(x_u.shape[1])
    if tuple(W.shape) != (d, d) or tuple(b.shape) != (d,):
        raise SelfrecHipError(f"boot_fwd_bwd: W must be ({d} x {d}) and b ({d},)")
    w = kernel_width(d, TABLE_NCE_WIDTHS, "boot_fwd_bwd", "the kernels serve")
    dev = x_u.device
    lib = _lib.load()
    grads = torch.empty((2, n, w), dtype=torch.float32, device=dev)
    sides, keep, back = [], [], []
    for s, (x, tgt, idx, store, name) in enumerate(((x_u, tgt_u, idx_u, store_u, "user"), (x_i, tgt_i, idx_i, store_i, "item"))):
        _p(x, None, f"x ({name})")
        _p(tgt, None, f"tgt ({name})")
        if tgt.dim() != 2 or int(tgt.shape[1]) != d or (idx is None and int(tgt.shape[0]) != n):
            raise SelfrecHipError(f"boot_fwd_bwd: the {name} target must be (rows x {d}), one row per slot without an index")
        if store is not None and tuple(store.shape) != tuple(tgt.shape):
            raise SelfrecHipError(f"boot_fwd_bwd: the {name} store table must have its target table's shape")
        xs, ix = to_width(x, w), _idx(idx, n, f"idx ({name})")
        same = store is not None and store.data_ptr() == tgt.data_ptr()
        if w == d:
            ts, ss = (store if same else to_width(tgt, w)), store
        else:
            ts = to_width(tgt, w)
            ss = None if store is None else (ts if same else to_width(store, w))
            if store is not None:
                back.append((store, ss))
        keep += [xs, ix, ts, ss]
        sides.append(_lib.BootSide(_p(xs, torch.float32, "x"), _p(ts, torch.float32, "tgt"), _p(ix), int(tgt.shape[0]),
                                   _p(ss, torch.float32, "store"), grads[s].data_ptr()))
    Ws = to_width(W, w) if w == d else to_width(to_width(W, w).t(), w).t().contiguous()
    bs = to_width(b.reshape(1, d), w).reshape(w)
    out = torch.empty(3, dtype=torch.float64, device=dev)               # [loss, mean cu, mean ci]
    gw = torch.empty((w, w), dtype=torch.float32, device=dev)
    gb = torch.empty(w, dtype=torch.float32, device=dev)
    ws = workspace(lib.srh_boot_ws_bytes(n, w), dev, ws)
    check(lib.srh_boot_fwd_bwd(C.byref(sides[0]), C.byref(sides[1]), _p(Ws, torch.float32, "W"), _p(bs, torch.float32, "b"), n,
                               w, float(alpha), float(beta), float(eps), float(c0), float(c1),
                               _lib.SRH_BOOT_CLAMP_COSINE if cosine else _lib.SRH_BOOT_CLAMP_NORMALIZE, out[1:].data_ptr(),
                               out.data_ptr(), gw.data_ptr(), gb.data_ptr(), _p(ws), _stream()), "srh_boot_fwd_bwd")
    for store, ss in back:
        store.copy_(cut_cols(ss, d))
    return out[0], out[1:], cut_cols(grads[0], d), cut_cols(grads[1], d), cut_cols(gw, d)[:d], cut_cols(gb, d)


class BootstrapLossFn(LossGradFn):
    """boot_fwd_bwd as one differentiable op of (x_u, x_i, W, b): the loss as a float32 scalar.  The targets, their index
    lists, the store tables (written in place), the five scalars and the clamp flag take no gradient."""

    @staticmethod
    def forward(ctx, x_u, x_i, W, b, tgt_u, tgt_i, idx_u=None, idx_i=None, store_u=None, store_i=None, alpha=1.0, beta=0.0,
                eps=1e-12, c0=4.0, c1=2.0, cosine=False):
        loss, _parts, gu, gi, gw, gb = boot_fwd_bwd(x_u.detach(), x_i.detach(), W.detach(), b.detach(), tgt_u.detach(),
                                                    tgt_i.detach(), idx_u, idx_i, None if store_u is None else store_u.detach(),
                                                    None if store_i is None else store_i.detach(), alpha, beta, eps, c0, c1,
                                                    cosine)
        return LossGradFn.keep(ctx, loss, gu, gi, gw, gb)


def rows_momentum(tgt, src, idx, m, ws=None):
    """tgt[idx] = tgt[idx] * m + src[idx] * (1 - m) in place on tgt (BUIR.py:69-75), to torch's bits: every slot's row is
    computed from the values tgt held before the call, then stored, so a repeated id is updated once.  tgt and src are
    (rows x d) float32 tables of one shape, any d; an id outside the table is skipped."""
    if tgt.dim() != 2 or tuple(src.shape) != tuple(tgt.shape) or idx.dim() != 1:
        raise SelfrecHipError("rows_momentum: tgt and src must share one (rows x d) shape, idx must be a list of ids")
    n, (rows, d) = int(idx.shape[0]), map(int, tgt.shape)
    _p(idx, None, "idx")
    ix = idx.to(torch.int32).contiguous()
    lib = _lib.load()
    ws = workspace(lib.srh_rows_momentum_ws_bytes(n, d), tgt.device, ws)
    check(lib.srh_rows_momentum_f32(_p(tgt, torch.float32, "tgt"), _p(src, torch.float32, "src"), _p(ix), n, rows, d,
                                    float(m), float(1 - m), _p(ws), _stream()), "srh_rows_momentum_f32")
    return tgt
