"""What every kernel family's wrappers share: stream and pointer plumbing, the widths the kernels serve, and the four
helpers -- the kernel width with its pad and cut, the workspace, the 64-bit mask, the loss op that saves its gradients."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _lib
from .._lib import SelfrecHipError, SpmmEpilogue, check  # noqa: F401  (the submodules take all their plumbing from here)

require_gpu = _lib.require_gpu


def gpu_available() -> bool:
    return torch.cuda.is_available()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t, dtype=None, name="tensor"):
    """Device address of a contiguous CUDA(HIP) tensor (None -> NULL)."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise SelfrecHipError(f"{name}: expected a HIP device tensor (the product path has no CPU fallback)")
    if dtype is not None and t.dtype != dtype:
        raise SelfrecHipError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise SelfrecHipError(f"{name}: tensor must be contiguous")
    return t.data_ptr()


def _np(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return a, a.ctypes.data_as(C.c_void_p)


def u64(x) -> int:
    """a seed or counter as the unsigned 64-bit value the entry points take"""
    return int(x) & 0xFFFFFFFFFFFFFFFF


# ---- any table width through the boundary (reference base/recommender.py:16: `embedding.size` is any integer) ----
SPMM_WIDTHS = (8, 16, 32, 64, 128, 256)      # row widths srh_spmm_f32 serves (csrc/spmm.hip)
ROW_WIDTHS = (32, 64, 128, 256)              # LPR kernels: BPR / L2 / scoring GEMM (csrc/common.h: dim_supported)
NCE_WIDTHS = (64, 128, 256)                  # srh_infonce_fwd_bwd (256: the split path only)
TABLE_NCE_WIDTHS = (64, 128)                 # the row-tile kernels of contrastive / sept / mhcn.hip and srh_kmeans_assign_f32


def padded_width(d: int, widths) -> int | None:
    """The narrowest width of `widths` that holds d columns (None: wider than the widest)."""
    return next((w for w in widths if w >= int(d)), None)


def pad_cols(t: torch.Tensor, width: int) -> torch.Tensor:
    """(rows, d) -> contiguous (rows, width) with zero columns on the right (a no-op view when d == width).  Zero columns
    change none of the path's results: products, inner products, norms and F.normalize ignore them, their gradients
    are exactly zero."""
    d = int(t.shape[1])
    if d == width:
        return t.contiguous()
    out = torch.zeros((t.shape[0], width), dtype=t.dtype, device=t.device)
    out[:, :d] = t
    return out


def kernel_width(d: int, widths, what=None, serves="the kernel serves") -> int:
    """The width of `widths` that rows of d columns are padded to for a kernel.  A d past the widest raises in the
    caller's name `what`; with what=None it is handed on as it is and the library refuses it with its unsupported status."""
    w = padded_width(d, widths)
    if w is None and what is not None:
        raise SelfrecHipError(f"{what}: rows of {d} columns -- {serves} up to {widths[-1]}")
    return w or int(d)


def to_width(t: torch.Tensor, w: int) -> torch.Tensor:
    """t as contiguous float32 with its last axis zero-padded to w columns (pad_cols; any number of leading axes)"""
    t = t.float()
    if t.dim() == 2:
        return pad_cols(t, w)
    return pad_cols(t.reshape(-1, t.shape[-1]), w).reshape(*t.shape[:-1], w)


def cut_cols(t: torch.Tensor, d: int) -> torch.Tensor:
    """a kernel's output back at the caller's d columns: the tensor itself when nothing was padded, else the view"""
    return t if int(t.shape[-1]) == d else t[..., :d]


def workspace(need, device, ws=None, floor: int = 256):
    """`ws` when it holds at least `need` bytes, else a fresh uint8 buffer of max(need, floor) bytes (never empty, so it
    always has an address to hand over)."""
    if ws is None or ws.numel() * ws.element_size() < int(need):
        ws = torch.empty(max(int(need), floor), dtype=torch.uint8, device=device)
    return ws


class LossGradFn(torch.autograd.Function):
    """Base of the loss ops whose one kernel call returns the loss WITH every gradient.  A subclass's forward() makes the
    call and returns ``LossGradFn.keep(ctx, loss, *grads)``: grads, one per leading input in order, are saved; backward()
    multiplies them by the upstream scalar and gives None to the remaining inputs."""

    @staticmethod
    def keep(ctx, loss, *grads):
        ctx.save_for_backward(*grads)
        return loss.to(torch.float32)

    @staticmethod
    def backward(ctx, gout):
        grads = ctx.saved_tensors
        return tuple(g * gout for g in grads) + (None,) * (len(ctx.needs_input_grad) - len(grads))
