"""DirectAU (csrc/au.hip): the alignment and uniformity losses of a batch's rows, forward and backward in one call."""
import torch

from ._base import (TABLE_NCE_WIDTHS, LossGradFn, SelfrecHipError, _lib, _p, _stream, check, cut_cols, kernel_width, to_width,
                    workspace)


def au_supported(d) -> bool:
    """the row widths srh_au_fwd_bwd serves once zero-padded: 1 .. 128 columns"""
    return 1 <= int(d) <= TABLE_NCE_WIDTHS[-1]


def au_fwd_bwd(x, y, t=2.0, w_align=1.0, w_ux=1.0, w_uy=1.0, ws=None):
    """DirectAU's loss (DirectAU.py:37-48) of the un-normalised (n x d) rows x and y, with both gradients:
        loss = w_align * alignment(x, y) + w_ux * uniformity(x, t) + w_uy * uniformity(y, t)
    y=None gives w_ux * uniformity(x, t) alone.  Returns
        loss (float64 scalar), parts (3, float64: alignment, uniformity(x), uniformity(y), unweighted; with y=None only
        parts[1] is written), gx, gy (n x d: dloss/dx and dloss/dy; gy is None with y=None)
    No n x n matrix and no list of pair distances is made.  Any d up to 128 (narrower rows are zero-padded, which changes
    no result), n >= 2; otherwise the library's status as a SelfrecHipError."""
    if x.dim() != 2 or (y is not None and tuple(y.shape) != tuple(x.shape)):
        raise SelfrecHipError("au_fwd_bwd: x and y must share one (n x d) shape")
    n, d = int(x.shape[0]), int(x.shape[1])
    _p(x, None, "x")
    _p(y, None, "y")
    w = kernel_width(d, TABLE_NCE_WIDTHS, "au_fwd_bwd", "the kernels serve")
    dev = x.device
    xs = to_width(x, w)
    ys = None if y is None else to_width(y, w)
    out = torch.empty(4, dtype=torch.float64, device=dev)               # [loss, A, U(x), U(y)]
    grads = torch.empty((1 if y is None else 2, n, w), dtype=torch.float32, device=dev)
    lib = _lib.load()
    ws = workspace(lib.srh_au_ws_bytes(n, w), dev, ws)
    check(lib.srh_au_fwd_bwd(_p(xs, torch.float32, "x"), _p(ys, torch.float32, "y"), n, w, float(t), float(w_align),
                             float(w_ux), float(w_uy), out[1:].data_ptr(), out.data_ptr(), grads[0].data_ptr(),
                             None if y is None else grads[1].data_ptr(), _p(ws), _stream()), "srh_au_fwd_bwd")
    return out[0], out[1:], cut_cols(grads[0], d), None if y is None else cut_cols(grads[1], d)


class AlignUniformFn(LossGradFn):
    """au_fwd_bwd as one differentiable op of (x, y): w_align alignment(x, y) + w_ux uniformity(x, t) + w_uy uniformity(y, t)
    as a float32 scalar; y=None: w_ux uniformity(x, t).  backward() scales the saved gradients by the upstream scalar."""

    @staticmethod
    def forward(ctx, x, y, t=2.0, w_align=1.0, w_ux=1.0, w_uy=1.0):
        loss, _parts, gx, gy = au_fwd_bwd(x.detach(), None if y is None else y.detach(), t, w_align, w_ux, w_uy)
        return LossGradFn.keep(ctx, loss, *((gx,) if y is None else (gx, gy)))
