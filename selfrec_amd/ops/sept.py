"""SEPT (csrc/sept.hip): the row normalise, alone and behind a product, and the tri-training neighbour discrimination."""
import ctypes as C

import torch

from ._base import (TABLE_NCE_WIDTHS, LossGradFn, SelfrecHipError, _lib, _p, _stream, check, cut_cols, kernel_width, to_width,
                    workspace)
from .sparse import spmm_any



L2NORM_MAX_WIDTH = 256                        # srh_rows_l2norm_*_f32
TRI_ND_MAX_K = 32


def rows_l2norm_fwd(y):
    """tf.math.l2_normalize(y, axis=1): (out (n x d), inv (n)) with inv_r = rsqrt(max(sum_c y_rc^2, 1e-12)).  Any
    1 <= d <= 256, any n >= 0."""
    if y.dim() != 2:
        raise SelfrecHipError("rows_l2norm_fwd: an (n x d) matrix expected")
    y = y.contiguous()
    n, d = int(y.shape[0]), int(y.shape[1])
    out = torch.empty_like(y)
    inv = torch.empty(n, dtype=torch.float32, device=y.device)
    check(_lib.load().srh_rows_l2norm_fwd_f32(_p(y, torch.float32, "y"), n, d, _p(out), _p(inv), _stream()),
          "srh_rows_l2norm_fwd_f32")
    return out, inv


def rows_l2norm_bwd(g, out, inv):
    """The gradient of rows_l2norm_fwd's input from the gradient g of its output: (g - out (out . g)) * inv per row,
    g * 1e6 on a clamped row (inv == 1e6)."""
    g, out, inv = g.contiguous(), out.contiguous(), inv.contiguous()
    if g.shape != out.shape or g.dim() != 2 or int(inv.numel()) != int(g.shape[0]):
        raise SelfrecHipError("rows_l2norm_bwd: g and out (n x d) and inv (n) expected")
    n, d = int(g.shape[0]), int(g.shape[1])
    gy = torch.empty_like(g)
    check(_lib.load().srh_rows_l2norm_bwd_f32(_p(g, torch.float32, "g"), _p(out, torch.float32, "out"),
                                              _p(inv, torch.float32, "inv"), n, d, _p(gy), _stream()),
          "srh_rows_l2norm_bwd_f32")
    return gy


class RowsL2NormFn(torch.autograd.Function):
    """tf.math.l2_normalize(y, axis=1) on its own (MHCN keeps the raw propagated rows for the next layer, so the SpMM and
    the normalise are separate ops there): rows_l2norm_fwd / rows_l2norm_bwd."""

    @staticmethod
    def forward(ctx, y):
        out, inv = rows_l2norm_fwd(y)
        ctx.save_for_backward(out, inv)
        return out

    @staticmethod
    def backward(ctx, g):
        out, inv = ctx.saved_tensors
        return rows_l2norm_bwd(g, out, inv)


class NormPropFn(RowsL2NormFn):
    """l2_normalize(A x, axis=1) of one SEPT / MHCN layer (SEPT.py:51-52) as one differentiable op of x: the HIP SpMM and
    the row normalise forward; the normalise backward and the SpMM on the explicit transpose backward (the social views
    are not symmetric)."""

    @staticmethod
    def forward(ctx, handle, x):
        if x.dtype != torch.float32 or not x.is_cuda:
            raise SelfrecHipError("NormPropFn: x must be an fp32 HIP tensor")
        ctx.handle = handle
        return RowsL2NormFn.forward(ctx, spmm_any(handle.csr, x.contiguous()))

    @staticmethod
    def backward(ctx, g):
        return None, spmm_any(ctx.handle.transposed().csr, RowsL2NormFn.backward(ctx, g))


def tri_nd_fwd_bwd(views, aug, k, tau=0.1, loss_scale=1.0, ws=None):
    """SEPT's tri-training step (SEPT.py:98-134) forward and backward in one call.  views = (friend, sharing, rec) and
    aug: the (n x d) gathered rows of the batch's unique users, un-normalised.  Returns
        loss (3, float64)   loss_scale * sum_i [log sum_j e_v[i][j] - log sum_{j in pos_v[i]} e_v[i][j]], e = exp(s / tau)
        grads               (dL/dfriend, dL/dsharing, dL/drec, dL/daug), each (n x d), scaled by loss_scale
        pos (3, n, k int32) the positives of each view and row, best first: the top-k of the OTHER two views' averaged
                            softmax (ties to the lowest index)
    No n x n matrix is made.  Any d up to 128 (narrower rows are zero-padded, which changes no result), 1 <= k <= 32,
    n >= k; otherwise the library's unsupported status as a SelfrecHipError."""
    if len(views) != 3:
        raise SelfrecHipError("tri_nd_fwd_bwd: three views (friend, sharing, rec) expected")
    n, d = int(aug.shape[0]), int(aug.shape[1])
    for t in (*views, aug):
        if t.dim() != 2 or int(t.shape[0]) != n or int(t.shape[1]) != d:
            raise SelfrecHipError("tri_nd_fwd_bwd: the three views and aug must share one (n x d) shape")
        _p(t, None, "view")
    w = kernel_width(d, TABLE_NCE_WIDTHS, "tri_nd_fwd_bwd", "the kernels serve")
    dev = aug.device
    mats = [to_width(t, w) for t in (*views, aug)]
    k = int(k)
    loss = torch.empty(3, dtype=torch.float64, device=dev)
    grads = torch.empty((4, n, w), dtype=torch.float32, device=dev)
    pos = torch.empty((3, n, max(k, 0)), dtype=torch.int32, device=dev)
    a = _lib.TriNdArgs()
    for v in range(3):
        a.d_view[v] = _p(mats[v], torch.float32, "view")
        a.d_gview[v] = grads[v].data_ptr()
    a.d_aug, a.d_gaug = _p(mats[3], torch.float32, "aug"), grads[3].data_ptr()
    a.n, a.d, a.k, a.tau, a.loss_scale = n, w, k, float(tau), float(loss_scale)
    a.d_loss, a.d_pos = _p(loss), pos.data_ptr()
    ws = workspace(_lib.load().srh_tri_nd_ws_bytes(n, w, k), dev, ws)
    check(_lib.load().srh_tri_nd_fwd_bwd(C.byref(a), _p(ws), _stream()), "srh_tri_nd_fwd_bwd")
    return loss, tuple(cut_cols(grads[v], d) for v in range(4)), pos


class TriNdFn(LossGradFn):
    """tri_nd_fwd_bwd as one differentiable op of (friend, sharing, rec, aug): the three losses summed (SEPT.py:149-151);
    backward() scales the saved gradients by the upstream scalar.  ``TriNdFn.last_pos`` keeps the call's positives."""
    last_pos = None

    @staticmethod
    def forward(ctx, friend, sharing, rec, aug, k, tau):
        loss, grads, pos = tri_nd_fwd_bwd((friend, sharing, rec), aug, k, tau)
        TriNdFn.last_pos = pos
        return LossGradFn.keep(ctx, loss.sum(), *grads)
