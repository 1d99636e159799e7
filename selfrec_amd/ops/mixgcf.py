"""MixGCF (csrc/mixgcf.hip): the hop mixing -- pick, mix and row gradients."""
from __future__ import annotations

import ctypes as C

import torch

from ._base import SelfrecHipError, _lib, _p, _stream, check, u64, workspace



MIXUP_MAX_HOPS = _lib.SRH_MIXUP_MAX_HOPS


def mixup_supported(d, n_hops, n_negs) -> bool:
    """the shapes srh_mixup_*_f32 serve: d a multiple of 4 in 4..256, 1..8 hop tables, at least one candidate per pair"""
    d, n_hops, n_negs = int(d), int(n_hops), int(n_negs)
    return 4 <= d <= 256 and d % 4 == 0 and 1 <= n_hops <= MIXUP_MAX_HOPS and n_negs >= 1


def _mixup_alpha(alpha, n_hops, shape, device):
    """None, or the H injected (B x C x d) float32 device tensors of a call: a list of H tensors or one (H, B, C, d) array"""
    if alpha is None:
        return None
    if isinstance(alpha, (list, tuple)):
        hops = [torch.as_tensor(a) for a in alpha]
    else:
        alpha = torch.as_tensor(alpha)
        hops = [alpha[k] for k in range(int(alpha.shape[0]))] if alpha.dim() == 4 else None
    if hops is None or len(hops) != n_hops or any(tuple(a.shape) != shape for a in hops):
        raise SelfrecHipError(f"mixup: alpha must be {n_hops} tensors of shape {shape}")
    return [a.to(device=device, dtype=torch.float32).contiguous() for a in hops]


def _mixup_args(dev, n_items, d, n_hops, B, n_negs, pos, neg, alpha, rng_seed, rng_counter, what):
    """the index streams as int32 (converted once) and the args struct without its table pointers; the returned list keeps
    the converted tensors alive until the call is enqueued"""
    if not pos.is_cuda or not neg.is_cuda:
        raise SelfrecHipError(f"{what}: expected HIP device tensors (the product path has no CPU fallback)")
    if pos.dim() != 1 or int(neg.numel()) != B * n_negs:
        raise SelfrecHipError(f"{what}: pos (B) and neg (B * n_negs) expected")
    pos32, neg32 = pos.to(torch.int32).contiguous(), neg.reshape(-1).to(torch.int32).contiguous()
    al = _mixup_alpha(alpha, n_hops, (B, n_negs, d), dev)
    a = _lib.MixupArgs()
    a.d_pos, a.d_neg = pos32.data_ptr(), neg32.data_ptr()
    a.n_items, a.B, a.n_hops, a.n_negs, a.d = n_items, B, n_hops, n_negs, d
    a.rng_seed, a.rng_counter = u64(rng_seed), u64(rng_counter)
    if al is not None:
        for k in range(min(n_hops, MIXUP_MAX_HOPS)):
            a.d_alpha[k] = al[k].data_ptr()
    return a, [pos32, neg32, al]


def _hop_shape(item_hops, what):
    if len(item_hops) < 1 or any(t.dim() != 2 or tuple(t.shape) != tuple(item_hops[0].shape) for t in item_hops):
        raise SelfrecHipError(f"{what}: the hop tables must share one (I x d) shape")
    return int(item_hops[0].shape[0]), int(item_hops[0].shape[1])


def mixup_fwd(u, item_hops, pos, neg, n_negs, *, alpha=None, rng_seed=0, rng_counter=0):
    """MixGCF's hop mixing (MixGCF.py:96-114): per pair and hop the n_negs candidates are mixed with the positive
    (alpha p + (1 - alpha) n, alpha per element), scored against the user row u (B x d), and the hardest one is kept.
    item_hops: H tensors (I x d), handed over as they are (row slices of wider tables included).  alpha: None (drawn in
    the kernel at counters rng_counter + (k B + b) n_negs + c) or H tensors (B x n_negs x d).
    Returns (pos_out, neg_out (B x d): the hop means of the positives and of the kept mixtures, pick (H x B, int32))."""
    n_items, d = _hop_shape(item_hops, "mixup_fwd")
    n_hops, n_negs, B = len(item_hops), int(n_negs), int(pos.numel())
    if u.dim() != 2 or tuple(u.shape) != (B, d):
        raise SelfrecHipError("mixup_fwd: u must be (B x d)")
    dev = u.device
    a, keep = _mixup_args(dev, n_items, d, n_hops, B, n_negs, pos, neg, alpha, rng_seed, rng_counter, "mixup_fwd")
    for k in range(min(n_hops, MIXUP_MAX_HOPS)):
        a.d_table[k] = _p(item_hops[k], torch.float32, f"item_hops[{k}]")
    uc = u.contiguous()
    out = torch.empty((2, B, d), dtype=torch.float32, device=dev)
    pick = torch.empty((n_hops, B), dtype=torch.int32, device=dev)
    check(_lib.load().srh_mixup_fwd_f32(C.byref(a), _p(uc, torch.float32, "u"), out[0].data_ptr(), out[1].data_ptr(),
                                        _p(pick), _stream()), "srh_mixup_fwd_f32")
    return out[0], out[1], pick


def mixup_bwd(item_hops, pos, neg, n_negs, pick, g_pos, g_neg, *, alpha=None, rng_seed=0, rng_counter=0):
    """The gradients of mixup_fwd's two outputs with respect to the hop tables: a list of H dense (I x d) tensors, zero
    outside the touched rows, every row summed in ascending pair order (a pair's positive before its negative).  Only the
    shape of item_hops is read; g_pos / g_neg (B x d) may be None (zero); alpha / rng_* as in the forward call."""
    n_items, d = _hop_shape(item_hops, "mixup_bwd")
    return _mixup_bwd(len(item_hops), n_items, d, pos, neg, n_negs, pick, g_pos, g_neg, alpha, rng_seed, rng_counter)


def _mixup_bwd(n_hops, n_items, d, pos, neg, n_negs, pick, g_pos, g_neg, alpha, rng_seed, rng_counter):
    n_negs, B = int(n_negs), int(pos.numel())
    dev = pos.device
    for g in (g_pos, g_neg):
        if g is not None and tuple(g.shape) != (B, d):
            raise SelfrecHipError("mixup_bwd: g_pos and g_neg must be (B x d)")
    if tuple(pick.shape) != (n_hops, B):
        raise SelfrecHipError("mixup_bwd: pick must be (H x B)")
    a, keep = _mixup_args(dev, n_items, d, n_hops, B, n_negs, pos, neg, alpha, rng_seed, rng_counter, "mixup_bwd")
    grads = torch.empty((n_hops, n_items, d), dtype=torch.float32, device=dev)
    for k in range(min(n_hops, MIXUP_MAX_HOPS)):
        a.d_grad[k] = grads[k].data_ptr()
    gp = None if g_pos is None else g_pos.float().contiguous()
    gn = None if g_neg is None else g_neg.float().contiguous()
    pk = pick.to(torch.int32).contiguous()
    ws = workspace(_lib.load().srh_mixup_bwd_ws_bytes(B, n_hops), dev)
    check(_lib.load().srh_mixup_bwd_f32(C.byref(a), _p(pk, torch.int32, "pick"), _p(gp), _p(gn), _p(ws), _stream()),
          "srh_mixup_bwd_f32")
    return [grads[k] for k in range(n_hops)]


class MixupFn(torch.autograd.Function):
    """mixup_fwd / mixup_bwd as one differentiable op of the H hop tables -> (pos_out, neg_out, pick).  u, the indices,
    alpha and pick carry no gradient (the choice is detached in the reference); the backward pass needs none of the
    tables, only the int32 index streams, pick and the alpha source."""

    @staticmethod
    def forward(ctx, u, pos, neg, n_negs, alpha, rng_seed, rng_counter, *item_hops):
        pos32, neg32 = pos.to(torch.int32), neg.reshape(-1).to(torch.int32)
        al = _mixup_alpha(alpha, len(item_hops), (int(pos.numel()), int(n_negs), int(item_hops[0].shape[1])), u.device)
        pos_out, neg_out, pick = mixup_fwd(u.detach(), [t.detach() for t in item_hops], pos32, neg32, n_negs, alpha=al,
                                           rng_seed=rng_seed, rng_counter=rng_counter)
        ctx.save_for_backward(pos32, neg32, pick, *(al or ()))
        ctx.shape = (len(item_hops), int(item_hops[0].shape[0]), int(item_hops[0].shape[1]))
        ctx.n_negs, ctx.rng = int(n_negs), (rng_seed, rng_counter)
        ctx.mark_non_differentiable(pick)
        return pos_out, neg_out, pick

    @staticmethod
    def backward(ctx, g_pos, g_neg, _g_pick):
        pos32, neg32, pick, *al = ctx.saved_tensors
        grads = _mixup_bwd(*ctx.shape, pos32, neg32, ctx.n_negs, pick, g_pos, g_neg, al or None, *ctx.rng)
        return (None,) * 7 + tuple(grads)
