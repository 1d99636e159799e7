"""Differentiable losses with the signatures of reference util/loss_torch.py -- all seven of its public functions
(``bpr_loss`` :6-10, ``triplet_loss`` :12-16, ``l2_reg_loss`` :18-22, ``batch_softmax_loss`` :25-32, ``InfoNCE`` :35-50,
``info_nce`` :54-88, ``kl_divergence`` :91-94), computed by fused HIP forward+backward kernels.

What runs where:
  * 2-D fp32 HIP tensors -- what every model file of the reference passes once ``.cuda()`` has run -- ALWAYS take the
    HIP kernels; a missing library or device raises (``ops.SelfrecHipError``), nothing is substituted.  Any
    ``embedding.size`` (base/recommender.py:16): rows are zero-padded to the next width the kernels serve -- zero
    columns change no inner product, norm or F.normalize result and receive exactly zero gradient -- BPR up to
    256 columns, InfoNCE up to 256 (above 128: the split path only), the regulariser any size.  bpr_loss's three operands
    broadcast against each other as the reference's torch.mul does (_bpr_operands); no rows: the torch expression (nan).
    triplet_loss follows bpr_loss in all of this; kl_divergence takes any R x C; info_nce, InfoNCE(b_cos=False) and
    InfoNCE below temperature 0.03 take the pair cross-entropy (ops.pair_ce_fwd_bwd), rows up to 128 columns.
  * CPU tensors, other dtypes, other ranks: the reference's own torch expression (the arithmetic of loss_torch.py:6-50
    restated below), so code that calls these functions off the device -- unit tests of a model file, a CPU dry run --
    behaves as it does with the reference.  This is not a fallback for the HIP path: device fp32 input never reaches it.
  * InfoNCE, BPR or triplet_loss on HIP rows wider than 256 columns, and the pair cross-entropy routes above 128: the
    same torch expression on the device (rocBLAS + ATen), announced once with a RuntimeWarning -- no kernel of this
    package serves those widths yet.
  * The cosine forms that go through the pair cross-entropy (info_nce(sim='cos'), InfoNCE(b_cos=True) below temperature
    0.03) normalise their rows with ops.RowsL2NormFn, x / max(|x|, 1e-6).  F.normalize clamps at 1e-12 and
    cosine_similarity at 1e-8: rows with 0 < |x| < 1e-6 deviate (value and gradient), and an exactly zero row has the
    reference's forward value (all its similarities are 0) but a gradient of g * 1e6 where the reference has g * 1e8
    (cosine_similarity) or g * 1e12 (F.normalize).  No device-to-host check looks for such rows.
"""
import warnings

import torch
import torch.nn.functional as F

from .. import ops


_warned_wide = []


def _on_hip_path(*tensors):
    """True when every tensor is what the kernels take (2-D fp32 HIP); False -> the torch expression."""
    return all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 for t in tensors)


def _padded(width_set, what, *tensors):
    d = int(tensors[0].shape[1])
    w = ops.padded_width(d, width_set)
    if w is None:
        raise ops.SelfrecHipError(f"{what}: rows of {d} columns -- the HIP kernels serve up to {width_set[-1]}")
    return d, w


def _dev_scalar(gout, like):
    """the upstream gradient as the kernels read it: a 0-dim f32 tensor ON THE DEVICE (a float(gout) would be a
    device-to-host sync in the middle of every backward pass -- the host could no longer run ahead of the device)"""
    if gout.device != like.device or gout.dtype != torch.float32:
        gout = gout.to(device=like.device, dtype=torch.float32)
    return gout.contiguous()


class _BprFn(torch.autograd.Function):
    """one launch forward (the mean is finished on the device), one backward"""

    @staticmethod
    def forward(ctx, u, p, n):
        d, w = _padded(ops.ROW_WIDTHS, "bpr_loss", u)
        u, p, n = (ops.pad_cols(t, w) for t in (u, p, n))
        loss = torch.empty((), dtype=torch.float32, device=u.device)
        coef = torch.empty(u.shape[0], dtype=torch.float32, device=u.device)
        ops.bpr_fwd(u, p, n, loss, coef)
        ctx.save_for_backward(u, p, n, coef)
        ctx.d = d
        return loss

    @staticmethod
    def backward(ctx, gout):
        u, p, n, coef = ctx.saved_tensors
        g = torch.empty((3,) + tuple(u.shape), dtype=torch.float32, device=u.device)
        ops.bpr_bwd(u, p, n, coef, _dev_scalar(gout, u), g[0], g[1], g[2])
        d = ctx.d
        return g[0][:, :d], g[1][:, :d], g[2][:, :d]


def _announce_wide(what, d, limit):
    if what not in _warned_wide:
        _warned_wide.append(what)
        warnings.warn(f"{what} on rows of {d} columns: the HIP kernels serve up to {limit}; evaluating the reference's "
                      f"expression (util/loss_torch.py) with ATen on the device", RuntimeWarning, stacklevel=3)


def _bpr_operands(user_emb, pos_item_emb, neg_item_emb):
    """The three operands at one shape, as the reference's torch.mul(user_emb, item_emb) sees them: equal shapes pass
    through, shapes that broadcast are expanded (views, OUTSIDE the autograd Function: autograd sums the gradient back
    over the expanded axis), anything else raises what torch raises.  The kernels take B and the width from one operand
    and cannot know the others' (pad_cols makes the expanded views contiguous)."""
    if user_emb.shape == pos_item_emb.shape == neg_item_emb.shape:
        return user_emb, pos_item_emb, neg_item_emb
    return tuple(torch.broadcast_tensors(user_emb, pos_item_emb, neg_item_emb))


def bpr_loss(user_emb, pos_item_emb, neg_item_emb):
    if _on_hip_path(user_emb, pos_item_emb, neg_item_emb):
        u, p, n = _bpr_operands(user_emb, pos_item_emb, neg_item_emb)
        rows, d = int(u.shape[0]), int(u.shape[1])
        if rows > 0 and d <= ops.ROW_WIDTHS[-1]:
            return _BprFn.apply(u, p, n)
        if d > ops.ROW_WIDTHS[-1]:
            _announce_wide("bpr_loss", d, ops.ROW_WIDTHS[-1])
        # (no rows: the mean of nothing, nan, as the reference returns -- the expression below)
    # loss_torch.py:6-10
    pos_score = torch.mul(user_emb, pos_item_emb).sum(dim=1)
    neg_score = torch.mul(user_emb, neg_item_emb).sum(dim=1)
    loss = -torch.log(10e-6 + torch.sigmoid(pos_score - neg_score))
    return torch.mean(loss)


class _L2RegFn(torch.autograd.Function):
    """reg * sum_k ||emb_k||_F / rows_k over 1..4 blocks of rows: one launch forward, one backward (zero gradient where a
    norm is zero, as torch.norm's)."""
    MAX_BLOCKS = 4

    @staticmethod
    def forward(ctx, reg, *embs):
        xs = [e.contiguous() for e in embs]
        dev = xs[0].device
        norms = torch.empty(len(xs), dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        ops.l2_reg_fwd(xs, reg, norms, loss)
        ctx.save_for_backward(norms, *xs)
        ctx.reg = float(reg)
        return loss

    @staticmethod
    def backward(ctx, gout):
        norms, *xs = ctx.saved_tensors
        gxs = [torch.empty_like(x) for x in xs]
        ops.l2_reg_bwd(xs, ctx.reg, norms, _dev_scalar(gout, norms), gxs)
        return (None, *gxs)


def _triplet_expression(user_emb, pos_item_emb, neg_item_emb):
    """loss_torch.py:12-16"""
    pos_score = ((user_emb - pos_item_emb) ** 2).sum(dim=1)
    neg_score = ((user_emb - neg_item_emb) ** 2).sum(dim=1)
    loss = F.relu(pos_score - neg_score + 0.5)
    return torch.mean(loss)


def triplet_loss(user_emb, pos_item_emb, neg_item_emb):
    """mean_b relu(|u_b - p_b|^2 - |u_b - n_b|^2 + 0.5): one HIP call (ops.TripletFn) produces the loss and the three
    gradients.  The operands broadcast as bpr_loss's; rows up to 256 columns."""
    if _on_hip_path(user_emb, pos_item_emb, neg_item_emb):
        u, p, n = _bpr_operands(user_emb, pos_item_emb, neg_item_emb)
        rows, d = int(u.shape[0]), int(u.shape[1])
        if rows > 0 and 0 < d <= ops.ROW_WIDTHS[-1]:
            return ops.TripletFn.apply(u, p, n)
        if d > ops.ROW_WIDTHS[-1]:
            _announce_wide("triplet_loss", d, ops.ROW_WIDTHS[-1])
        # (no rows: the mean of nothing, nan, as the reference returns -- the expression below)
    return _triplet_expression(user_emb, pos_item_emb, neg_item_emb)


def l2_reg_loss(reg, *args):
    if args and len(args) <= _L2RegFn.MAX_BLOCKS and all(_on_hip_path(e) and e.numel() > 0 for e in args):
        return _L2RegFn.apply(float(reg), *args)
    emb_loss = 0
    for emb in args:
        if _on_hip_path(emb) and emb.numel() > 0:
            emb_loss = emb_loss + _L2RegFn.apply(1.0, emb)                     # = ||emb|| / rows
        else:
            emb_loss = emb_loss + torch.norm(emb, p=2) / emb.shape[0]          # loss_torch.py:18-22
    return emb_loss * reg


def _batch_softmax_expression(user_emb, item_emb, temperature):
    """loss_torch.py:25-32"""
    user_emb, item_emb = F.normalize(user_emb, dim=1), F.normalize(item_emb, dim=1)
    pos_score = (user_emb * item_emb).sum(dim=-1)
    pos_score = torch.exp(pos_score / temperature)
    ttl_score = torch.matmul(user_emb, item_emb.transpose(0, 1))
    ttl_score = torch.exp(ttl_score / temperature).sum(dim=1)
    loss = -torch.log(pos_score / ttl_score + 10e-6)
    return torch.mean(loss)


def batch_softmax_loss(user_emb, item_emb, temperature):
    """mean_b -log(p_bb + 1e-5) of the in-batch softmax (SSL4Rec.py:33): one HIP call (ops.BatchSoftmaxFn) produces the
    loss and both gradients without the B x B logits; rows up to 128 columns."""
    if not _on_hip_path(user_emb, item_emb):
        return _batch_softmax_expression(user_emb, item_emb, temperature)
    if user_emb.shape != item_emb.shape:
        raise ops.SelfrecHipError("batch_softmax_loss: the two sides must have the same shape")
    return ops.BatchSoftmaxFn.apply(user_emb, item_emb, float(temperature))


class _InfoNceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v1, v2, temperature):
        d, w = _padded(ops.NCE_WIDTHS, "InfoNCE", v1)
        v1, v2 = ops.pad_cols(v1, w), ops.pad_cols(v2, w)
        n = v1.shape[0]
        dev = v1.device
        # [dL/dv1 | dL/dv2 | loss (one double)]: the kernels ADD into all three, so all three start at zero -- one fill
        buf = torch.zeros(2 * n * w + 2, dtype=torch.float32, device=dev)
        g = buf[:2 * n * w].view(2, n, w)
        loss = buf[2 * n * w:].view(torch.float64)
        ws = ops.infonce_ws(n, w, dev)
        # forward and backward share every intermediate, so both are produced here with unit
        # upstream gradient and scaled in backward()
        ops.infonce_fwd_bwd(v1, v2, None, n, tau=temperature, loss_scale=1.0, loss=loss, g1=g[0], g2=g[1], ws=ws)
        ctx.save_for_backward(g)
        ctx.d = d
        return loss.to(torch.float32).reshape(())

    @staticmethod
    def backward(ctx, gout):
        (g,) = ctx.saved_tensors
        g = g * gout
        return g[0][:, :ctx.d], g[1][:, :ctx.d], None


def _infonce_expression(view1, view2, temperature, b_cos=True):
    """loss_torch.py:35-50"""
    if b_cos:
        view1, view2 = F.normalize(view1, dim=1), F.normalize(view2, dim=1)
    pos_score = (view1 @ view2.T) / temperature
    score = torch.diag(F.log_softmax(pos_score, dim=1))
    return -score.mean()


INFONCE_UNIT_MIN_TAU = 0.03      # below it the unit-row kernels' exp((s - 1) / tau) underflows (csrc/losses.hip): pair CE


def _arange_labels(n, device, shift=0):
    labels = torch.arange(n, dtype=torch.int32, device=device)
    return labels if not shift else (labels + shift) % n


def InfoNCE(view1, view2, temperature: float, b_cos: bool = True):
    """b_cos=True at temperature >= 0.03: the unit-row InfoNCE kernels (srh_infonce_fwd_bwd), as before.  b_cos=False, and
    b_cos=True below 0.03 (rows normalised by ops.RowsL2NormFn first: F.normalize on every row of norm >= 1e-6, see the
    module docstring): the max-subtracted pair cross-entropy ops.PairCeFn with identity labels, 1 / temperature and
    1 / n, rows up to 128 columns.  ops.set_infonce_precision's process default (the split-16 products) has no meaning on
    that route: its products are f32 MFMA."""
    if not _on_hip_path(view1, view2):
        return _infonce_expression(view1, view2, temperature, b_cos)
    if view1.shape != view2.shape:
        raise ops.SelfrecHipError("InfoNCE: the two views must have the same shape")
    d = int(view1.shape[1])
    if b_cos and float(temperature) >= INFONCE_UNIT_MIN_TAU:
        if d > ops.NCE_WIDTHS[-1]:
            _announce_wide("InfoNCE", d, ops.NCE_WIDTHS[-1])
            return _infonce_expression(view1, view2, temperature, True)
        return _InfoNceFn.apply(view1, view2, float(temperature))
    n = int(view1.shape[0])
    if d > ops.TABLE_NCE_WIDTHS[-1] or n == 0 or d == 0:
        if d > ops.TABLE_NCE_WIDTHS[-1]:
            _announce_wide("InfoNCE (b_cos=False, or temperature < 0.03)", d, ops.TABLE_NCE_WIDTHS[-1])
        return _infonce_expression(view1, view2, temperature, b_cos)
    if b_cos:
        view1, view2 = ops.RowsL2NormFn.apply(view1), ops.RowsL2NormFn.apply(view2)
    return ops.PairCeFn.apply(view1, view2, _arange_labels(n, view1.device), 1.0 / float(temperature), 1.0 / n)


def _info_nce_expression(z_i, z_j, temp, batch_size, sim='dot'):
    """loss_torch.py:54-88"""
    N = 2 * batch_size
    z = torch.cat((z_i, z_j), dim=0)
    if sim == 'cos':
        sim = F.cosine_similarity(z.unsqueeze(1), z.unsqueeze(0), dim=2) / temp
    elif sim == 'dot':
        sim = torch.mm(z, z.T) / temp
    sim_i_j = torch.diag(sim, batch_size)
    sim_j_i = torch.diag(sim, -batch_size)
    positive_samples = torch.cat((sim_i_j, sim_j_i), dim=0).reshape(N, 1)
    mask = torch.ones((N, N), dtype=bool)
    mask = mask.fill_diagonal_(0)
    for i in range(batch_size):
        mask[i, batch_size + i] = 0
        mask[batch_size + i, i] = 0
    negative_samples = sim[mask].reshape(N, -1)
    labels = torch.zeros(N).to(positive_samples.device).long()
    logits = torch.cat((positive_samples, negative_samples), dim=1)
    return F.cross_entropy(logits, labels)


def info_nce(z_i, z_j, temp, batch_size, sim='dot'):
    """RecBole's NT-Xent: z = cat(z_i, z_j) (2B rows), every row against all others, its positive the same item's other
    view.  One pair cross-entropy of z against itself without the diagonal (ops.SelfPairCeFn: labels (m + B) mod 2B,
    1 / temp, 1 / 2B); no (2B)^2 array is made.  sim='cos' normalises the rows first (ops.RowsL2NormFn, clamp 1e-6 where
    cosine_similarity clamps at 1e-8: module docstring).  batch_size != z_i.shape[0], unequal shapes or no rows: the
    reference's expression, which raises what the reference raises.  Rows up to 128 columns."""
    if sim not in ('dot', 'cos'):
        raise ValueError(f"info_nce: sim must be 'dot' or 'cos', got {sim!r}")
    if not _on_hip_path(z_i, z_j) or z_i.shape != z_j.shape or int(z_i.shape[0]) != batch_size or batch_size < 1 \
            or int(z_i.shape[1]) == 0:
        return _info_nce_expression(z_i, z_j, temp, batch_size, sim)
    B, d = int(z_i.shape[0]), int(z_i.shape[1])
    if d > ops.TABLE_NCE_WIDTHS[-1]:
        _announce_wide("info_nce", d, ops.TABLE_NCE_WIDTHS[-1])
        return _info_nce_expression(z_i, z_j, temp, batch_size, sim)
    z = torch.cat((z_i, z_j), dim=0)
    if sim == 'cos':
        z = ops.RowsL2NormFn.apply(z)
    return ops.SelfPairCeFn.apply(z, _arange_labels(2 * B, z.device, B), 1.0 / float(temp), 1.0 / (2 * B))


def _kl_expression(p_logit, q_logit):
    """loss_torch.py:91-94"""
    p = F.softmax(p_logit, dim=-1)
    kl = torch.sum(p * (F.log_softmax(p_logit, dim=-1) - F.log_softmax(q_logit, dim=-1)), 1)
    return torch.mean(kl)


def kl_divergence(p_logit, q_logit):
    """mean_r KL(softmax(p_logit_r) || softmax(q_logit_r)) of (R x C) logits: one HIP call (ops.KlDivFn) produces the loss
    and both gradients, any R >= 1 and C >= 1."""
    if _on_hip_path(p_logit, q_logit) and p_logit.shape == q_logit.shape and p_logit.numel() > 0:
        return ops.KlDivFn.apply(p_logit, q_logit)
    return _kl_expression(p_logit, q_logit)
