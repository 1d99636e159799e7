"""DuoRec's contrastive section (csrc/duo.hip): two info_nce terms that share their anchor rows, as one call."""
from __future__ import annotations

import numpy as np
import torch

from ._base import TABLE_NCE_WIDTHS, SelfrecHipError, _lib, _p, _stream, check, cut_cols, kernel_width, to_width, workspace

DUO_WIDTHS = TABLE_NCE_WIDTHS                 # the row-tile kernels' widths; narrower rows are zero-padded


def duo_supported(d: int) -> bool:
    """rows of d columns fit the kernel (as they are, or zero-padded)"""
    return 1 <= int(d) <= DUO_WIDTHS[-1]


def _checked_idx(idx, idx_host, rows, B):
    """the (3, B) int32 index tensor on the device, after the host has seen that its 3B entries lie in [0, rows) and are
    pairwise distinct.  ``idx_host`` is the caller's host copy; without one the device tensor is copied back (a sync)."""
    host = np.asarray(idx_host if idx_host is not None else idx.detach().cpu().numpy()).reshape(-1).astype(np.int64)
    if host.size != 3 * B:
        raise SelfrecHipError(f"duo_nce: three index vectors of {B} entries expected, got {host.size} entries")
    if host.size and (host.min() < 0 or host.max() >= rows):
        raise SelfrecHipError(f"duo_nce: an index lies outside [0, {rows})")
    if np.unique(host).size != host.size:
        raise SelfrecHipError("duo_nce: the 3B indices must be pairwise distinct (a row named twice would be its own key)")
    if not isinstance(idx, torch.Tensor):
        raise SelfrecHipError("duo_nce: idx must be a (3, B) int32 device tensor")
    return idx.to(torch.int32).reshape(3, B).contiguous()


def duo_nce_fwd_bwd(x, idx, B, inv_temp=1.0, scale_u=1.0, scale_s=1.0, idx_host=None, ws=None):
    """Both contrastive terms of a DuoRec step and their whole gradient (srh_duo_nce_fwd_bwd, header (a-25)).

    x (R x d) on the device; idx a (3, B) int32 device tensor [idx_a; idx_p; idx_q] of pairwise distinct rows of x, or None:
    x is then the stacked (3B x d) blocks [a; p; q].  Returns (losses (2,) float64 = [scale_u info_nce(a, p), scale_s
    info_nce(a, q)] at temperature 1 / inv_temp, G (3B x d) = the rows [ga; gp; gq] of d(losses[0] + losses[1]) / dz).
    Rows up to 128 columns (narrower ones zero-padded: no result changes)."""
    if x.dim() != 2:
        raise SelfrecHipError("duo_nce: x must be 2-D")
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise SelfrecHipError("duo_nce: expected a HIP device tensor (the product path has no CPU fallback)")
    R, d, B = int(x.shape[0]), int(x.shape[1]), int(B)
    if B < 1:
        raise SelfrecHipError("duo_nce: B >= 1 expected")
    if not float(inv_temp) > 0.0 or not np.isfinite(float(inv_temp)):
        raise SelfrecHipError("duo_nce: inv_temp must be positive and finite")
    if idx is None:
        if R != 3 * B:
            raise SelfrecHipError(f"duo_nce: without index vectors x holds the 3B = {3 * B} rows, got {R}")
        ptrs = (None, None, None)
    else:
        idx = _checked_idx(idx, idx_host, R, B)
        ptrs = tuple(idx[k].data_ptr() for k in range(3))
    w = kernel_width(d, DUO_WIDTHS)
    xp = to_width(x, w) if w != d or x.dtype != torch.float32 or not x.is_contiguous() else x
    dev = x.device
    lib = _lib.load()
    ws = workspace(lib.srh_duo_nce_ws_bytes(B, w), dev, ws)
    losses = torch.empty(2, dtype=torch.float64, device=dev)
    g = torch.empty((3 * B, w), dtype=torch.float32, device=dev)
    check(lib.srh_duo_nce_fwd_bwd(_p(xp, torch.float32, "x"), R, ptrs[0], ptrs[1], ptrs[2], B, w, float(inv_temp),
                                  float(scale_u), float(scale_s), _p(losses), _p(g), _p(ws), _stream()),
          "srh_duo_nce_fwd_bwd")
    return losses, cut_cols(g, d)


class DuoNceFn(torch.autograd.Function):
    """duo_nce_fwd_bwd as one differentiable op.  ``DuoNceFn.apply(inv_temp, scale_u, scale_s, idx, idx_host, x)`` reads the
    rows of x at idx (3, B) and places G's rows into a zero gradient of x there; ``apply(inv_temp, scale_u, scale_s, None,
    None, a, p, q)`` serves three (B, d) inputs.  Returns the two losses (float32, (2,)), already times their scales."""

    @staticmethod
    def forward(ctx, inv_temp, scale_u, scale_s, idx, idx_host, *xs):
        if idx is None:
            if len(xs) != 3 or not (xs[0].shape == xs[1].shape == xs[2].shape):
                raise SelfrecHipError("DuoNceFn: three (B, d) inputs of one shape expected")
            B = int(xs[0].shape[0])
            losses, g = duo_nce_fwd_bwd(torch.cat([t.float() for t in xs], dim=0), None, B, inv_temp, scale_u, scale_s)
            ctx.rows = None
        else:
            if len(xs) != 1:
                raise SelfrecHipError("DuoNceFn: one input x with the index vectors")
            B = int(idx.numel()) // 3
            losses, g = duo_nce_fwd_bwd(xs[0], idx, B, inv_temp, scale_u, scale_s, idx_host=idx_host)
            ctx.rows = int(xs[0].shape[0])
            ctx.idx = idx.reshape(-1).long()
        ctx.B = B
        ctx.save_for_backward(g)
        return losses.to(torch.float32)

    @staticmethod
    def backward(ctx, gout):
        (g,) = ctx.saved_tensors
        # both losses' gradients come out of the kernel as one sum: the two upstream scalars must agree (a plain sum of the
        # two terms, what the model forms) -- the scales of the call are where a caller weighs them apart
        gg = g * gout[0]
        head = (None, None, None, None, None)
        if ctx.rows is None:
            B = ctx.B
            return head + (gg[:B], gg[B:2 * B], gg[2 * B:])
        gx = torch.zeros((ctx.rows, g.shape[1]), dtype=g.dtype, device=g.device)
        gx.index_copy_(0, ctx.idx, gg)
        return head + (gx,)
