"""The rest of util/loss_torch.py (csrc/contrastive.hip's pair cross-entropy, csrc/rowloss.hip): pair CE, triplet, KL."""
from __future__ import annotations

import torch

from ._base import (ROW_WIDTHS, TABLE_NCE_WIDTHS, LossGradFn, SelfrecHipError, _lib, _p, _stream, check, cut_cols,
                    kernel_width, to_width, workspace)

TRIPLET_MARGIN = 0.5                          # util/loss_torch.py:15


def _on_device(what, *tensors):
    """(before to_width, which makes strided or expanded operands contiguous: a host tensor must not be moved silently)"""
    for t in tensors:
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise SelfrecHipError(f"{what}: expected HIP device tensors (the product path has no CPU fallback)")


def pair_ce_fwd_bwd(rows, keys, labels, inv_temp=1.0, loss_scale=1.0, exclude_diagonal=False, add_gh_into_gt=False,
                    ws=None):
    """Softmax cross-entropy of the rows (M x d) against the keys (N x d) with logits s_mj = inv_temp * rows_m . keys_j:
    (loss (0-dim float64) = loss_scale * sum_m (lse_m - s_{m, label_m}), dL/drows (M x d), dL/dkeys (N x d)), both
    gradients carrying loss_scale * inv_temp.  labels: int32 device tensor of M entries in [0, N).
    exclude_diagonal (M == N, N > 1): key j = m is left out of row m's softmax; labels[m] == m then makes the loss NaN.
    add_gh_into_gt (M == N): the third result is dL/drows + dL/dkeys -- with rows and keys one tensor z (the two may
    alias), dL/dz.  The M x N logits are never materialised.  Rows up to 128 columns (narrower ones zero-padded: no
    result changes)."""
    if rows.dim() != 2 or keys.dim() != 2 or rows.shape[1] != keys.shape[1]:
        raise SelfrecHipError("pair_ce: rows (M x d) and keys (N x d) expected")
    M, d = int(rows.shape[0]), int(rows.shape[1])
    N = int(keys.shape[0])
    if int(labels.numel()) != M:
        raise SelfrecHipError(f"pair_ce: labels has {int(labels.numel())} entries, expected {M}")
    w = kernel_width(d, TABLE_NCE_WIDTHS, "pair_ce")
    _on_device("pair_ce", rows, keys)
    hp = to_width(rows, w)
    tp = hp if keys is rows else to_width(keys, w)
    dev = rows.device
    lib = _lib.load()
    ws = workspace(lib.srh_pair_ce_ws_bytes(M, N, w), dev, ws)
    loss = torch.empty((), dtype=torch.float64, device=dev)
    gh = torch.empty((M, w), dtype=torch.float32, device=dev)
    gt = torch.empty((N, w), dtype=torch.float32, device=dev)
    check(lib.srh_pair_ce_fwd_bwd(_p(hp, torch.float32, "rows"), M, _p(tp, torch.float32, "keys"), N, w,
                                  _p(labels, torch.int32, "labels"), float(inv_temp), float(loss_scale),
                                  int(bool(exclude_diagonal)), int(bool(add_gh_into_gt)), _p(loss), _p(gh), _p(gt), _p(ws),
                                  _stream()), "srh_pair_ce_fwd_bwd")
    return loss, cut_cols(gh, d), cut_cols(gt, d)


class PairCeFn(LossGradFn):
    """pair_ce_fwd_bwd as one differentiable op of (rows, keys): loss and both gradients come out of the one call;
    backward() scales them by the upstream scalar."""

    @staticmethod
    def forward(ctx, rows, keys, labels, inv_temp, loss_scale, exclude_diagonal=False):
        return LossGradFn.keep(ctx, *pair_ce_fwd_bwd(rows, keys, labels, inv_temp, loss_scale, exclude_diagonal))


class SelfPairCeFn(LossGradFn):
    """The pair cross-entropy of one matrix z against itself without its diagonal (info_nce, util/loss_torch.py:54-88) as
    one differentiable op of z: H = T = z, dL/dz = gh + gt out of pass 2 itself."""

    @staticmethod
    def forward(ctx, z, labels, inv_temp, loss_scale):
        loss, _, gz = pair_ce_fwd_bwd(z, z, labels, inv_temp, loss_scale, exclude_diagonal=True, add_gh_into_gt=True)
        return LossGradFn.keep(ctx, loss, gz)


def triplet_fwd_bwd(u, p, n, margin=TRIPLET_MARGIN, ws=None):
    """triplet_loss (util/loss_torch.py:12-16) and its gradients: (loss (0-dim float64) = mean_b relu(|u-p|^2 - |u-n|^2 +
    margin), dL/du, dL/dp, dL/dn); rows with a margin <= 0 get exact zeros.  Three (B x d) operands of one shape, B >= 1, rows
    up to 256 columns (narrower ones zero-padded: no result changes)."""
    if u.dim() != 2 or u.shape != p.shape or u.shape != n.shape:
        raise SelfrecHipError("triplet: three 2-D operands of one shape expected")
    B, d = int(u.shape[0]), int(u.shape[1])
    w = kernel_width(d, ROW_WIDTHS, "triplet")
    _on_device("triplet", u, p, n)
    up, pp, np_ = to_width(u, w), to_width(p, w), to_width(n, w)
    dev = u.device
    lib = _lib.load()
    ws = workspace(lib.srh_triplet_ws_bytes(B), dev, ws)
    loss = torch.empty((), dtype=torch.float64, device=dev)
    g = torch.empty((3, B, w), dtype=torch.float32, device=dev)
    check(lib.srh_triplet_fwd_bwd(_p(up, torch.float32, "u"), _p(pp, torch.float32, "p"), _p(np_, torch.float32, "n"), B, w,
                                  float(margin), _p(loss), g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(), _p(ws),
                                  _stream()), "srh_triplet_fwd_bwd")
    return loss, cut_cols(g[0], d), cut_cols(g[1], d), cut_cols(g[2], d)


class TripletFn(LossGradFn):
    """triplet_fwd_bwd as one differentiable op of (u, p, n)."""

    @staticmethod
    def forward(ctx, u, p, n):
        return LossGradFn.keep(ctx, *triplet_fwd_bwd(u, p, n))


def kl_div_fwd_bwd(p_logit, q_logit, ws=None):
    """kl_divergence (util/loss_torch.py:91-94) and its gradients: (loss (0-dim float64) = mean_r KL(softmax(p_logit_r) ||
    softmax(q_logit_r)), dL/dp_logit, dL/dq_logit).  Two (R x C) operands, any R >= 1 and C >= 1; the two may be one tensor."""
    if p_logit.dim() != 2 or p_logit.shape != q_logit.shape:
        raise SelfrecHipError("kl_div: two 2-D operands of one shape expected")
    R, C = int(p_logit.shape[0]), int(p_logit.shape[1])
    _on_device("kl_div", p_logit, q_logit)
    a = p_logit.float().contiguous()
    b = a if q_logit is p_logit else q_logit.float().contiguous()
    dev = a.device
    lib = _lib.load()
    ws = workspace(lib.srh_kl_div_ws_bytes(R), dev, ws)
    loss = torch.empty((), dtype=torch.float64, device=dev)
    g = torch.empty((2, R, C), dtype=torch.float32, device=dev)
    check(lib.srh_kl_div_fwd_bwd(_p(a, torch.float32, "p_logit"), _p(b, torch.float32, "q_logit"), R, C, _p(loss),
                                 g[0].data_ptr(), g[1].data_ptr(), _p(ws), _stream()), "srh_kl_div_fwd_bwd")
    return loss, g[0], g[1]


class KlDivFn(LossGradFn):
    """kl_div_fwd_bwd as one differentiable op of (p_logit, q_logit)."""

    @staticmethod
    def forward(ctx, p_logit, q_logit):
        return LossGradFn.keep(ctx, *kl_div_fwd_bwd(p_logit, q_logit))
