"""MHCN (csrc/mhcn.hip): the self-gates, the channel attention and the hierarchical MIM loss.  An unserved width goes to
the library as it is (kernel_width without a name), which refuses it with its unsupported status."""
import ctypes as C

import torch

from ._base import (TABLE_NCE_WIDTHS, LossGradFn, SelfrecHipError, _lib, _p, _stream, check, cut_cols, kernel_width, to_width,
                    workspace)



GATE_MAX = 4                                  # srh_gate_*_f32: gates per call


def _gate_operands(x, w, b, what):
    if x.dim() != 2 or w.dim() != 3 or b.dim() != 2 or w.shape[1] != w.shape[2] or int(w.shape[1]) != int(x.shape[1]) \
            or tuple(b.shape) != (int(w.shape[0]), int(x.shape[1])):
        raise SelfrecHipError(f"{what}: x (n x d), w (C x d x d) and b (C x d) expected")
    n, d, c = int(x.shape[0]), int(x.shape[1]), int(w.shape[0])
    wd = kernel_width(d, TABLE_NCE_WIDTHS)
    wp = w.float().contiguous()
    if wd != d:        # (the one operand padded along two axes: spelled out)
        wp = torch.zeros((c, wd, wd), dtype=torch.float32, device=x.device)
        wp[:, :d, :d] = w
    return to_width(x, wd), wp, to_width(b, wd), n, d, c, wd


def gate_fwd(x, w, b):
    """MHCN's self-gates (MHCN.py:79-83): y[c] = x * sigmoid(x @ w[c] + b[c]) for all C <= 4 gates from one read of x.
    x (n x d), w (C x d x d), b (C x d) -> y (C x n x d).  Any d up to 128 (zero-padded: a padded column gates to 0)."""
    xp, wp, bp, n, d, c, wd = _gate_operands(x, w, b, "gate_fwd")
    y = torch.empty((c, n, wd), dtype=torch.float32, device=x.device)
    check(_lib.load().srh_gate_fwd_f32(_p(xp, torch.float32, "x"), _p(wp, torch.float32, "w"), _p(bp, torch.float32, "b"),
                                       n, wd, c, _p(y), _stream()), "srh_gate_fwd_f32")
    return cut_cols(y, d)


def gate_bwd(x, w, b, gy):
    """The gradients of gate_fwd from gy (C x n x d): (dx (n x d), dw (C x d x d), db (C x d)).  sigmoid(x w + b) is
    recomputed, not saved; the reductions over rows are summed in chunk order."""
    xp, wp, bp, n, d, c, wd = _gate_operands(x, w, b, "gate_bwd")
    if tuple(gy.shape) != (c, n, d):
        raise SelfrecHipError("gate_bwd: gy must be (C x n x d)")
    gp = to_width(gy, wd)
    dev = x.device
    gx = torch.empty((n, wd), dtype=torch.float32, device=dev)
    gw = torch.empty((c, wd, wd), dtype=torch.float32, device=dev)
    gb = torch.empty((c, wd), dtype=torch.float32, device=dev)
    ws = workspace(_lib.load().srh_gate_bwd_ws_bytes(n, wd, c), dev)
    check(_lib.load().srh_gate_bwd_f32(_p(xp, torch.float32, "x"), _p(wp, torch.float32, "w"), _p(bp, torch.float32, "b"),
                                       _p(gp, torch.float32, "gy"), n, wd, c, _p(gx), _p(gw), _p(gb), _p(ws), _stream()),
          "srh_gate_bwd_f32")
    return cut_cols(gx, d), (gw if wd == d else gw[:, :d, :d]), cut_cols(gb, d)


class GateFn(torch.autograd.Function):
    """gate_fwd / gate_bwd as one differentiable op of (x, w, b) -> y (C x n x d)."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w, b)
        return gate_fwd(x, w, b)

    @staticmethod
    def backward(ctx, gy):
        x, w, b = ctx.saved_tensors
        return gate_bwd(x, w, b, gy)


def _mix_operands(e1, e2, e3, q, x, what):
    n, d = int(e1.shape[0]), int(e1.shape[1])
    for t in (e1, e2, e3) + (() if x is None else (x,)):
        if t.dim() != 2 or tuple(t.shape) != (n, d):
            raise SelfrecHipError(f"{what}: the channels (and the addend) must share one (n x d) shape")
    if int(q.numel()) != d:
        raise SelfrecHipError(f"{what}: q must hold d entries")
    wd = kernel_width(d, TABLE_NCE_WIDTHS)
    e1, e2, e3, q = (to_width(t, wd) for t in (e1, e2, e3, q.reshape(-1)))
    return e1, e2, e3, q, (None if x is None else to_width(x, wd)), n, d, wd


def chan_mix_fwd(e1, e2, e3, q, x=None, beta=0.0):
    """MHCN's channel attention (MHCN.py:85-93) with q = attention_mat @ attention^T: w_c = e_c . q per row,
    s = softmax over the three channels, out = sum_c s_c e_c + beta x.  Returns (out (n x d), s (n x 3))."""
    e1, e2, e3, qp, xp, n, d, wd = _mix_operands(e1, e2, e3, q, x, "chan_mix_fwd")
    out = torch.empty((n, wd), dtype=torch.float32, device=e1.device)
    score = torch.empty((n, 3), dtype=torch.float32, device=e1.device)
    check(_lib.load().srh_chan_mix_fwd_f32(_p(e1, torch.float32, "e1"), _p(e2, torch.float32, "e2"),
                                           _p(e3, torch.float32, "e3"), _p(qp, torch.float32, "q"),
                                           _p(xp, torch.float32, "x"), float(beta), n, wd, _p(out), _p(score), _stream()),
          "srh_chan_mix_fwd_f32")
    return cut_cols(out, d), score


def chan_mix_bwd(e1, e2, e3, q, score, gout, beta=0.0, with_x=False):
    """The gradients of chan_mix_fwd's ``out`` from gout (n x d) and the forward's scores:
    (de1, de2, de3, dx or None, dq (d)).  dq is summed over rows in chunk order."""
    e1, e2, e3, qp, gp, n, d, wd = _mix_operands(e1, e2, e3, q, gout, "chan_mix_bwd")
    dev = e1.device
    score = score.float().contiguous()
    if tuple(score.shape) != (n, 3):
        raise SelfrecHipError("chan_mix_bwd: the scores must be (n x 3)")
    g = torch.empty((4 if with_x else 3, n, wd), dtype=torch.float32, device=dev)
    gq = torch.empty(wd, dtype=torch.float32, device=dev)
    ws = workspace(_lib.load().srh_chan_mix_bwd_ws_bytes(n, wd), dev)
    check(_lib.load().srh_chan_mix_bwd_f32(_p(e1, torch.float32, "e1"), _p(e2, torch.float32, "e2"),
                                           _p(e3, torch.float32, "e3"), _p(qp, torch.float32, "q"),
                                           _p(score, torch.float32, "score"), _p(gp, torch.float32, "gout"), float(beta), n,
                                           wd, g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(),
                                           g[3].data_ptr() if with_x else None, _p(gq), _p(ws), _stream()),
          "srh_chan_mix_bwd_f32")
    g = [cut_cols(t, d) for t in g]
    return g[0], g[1], g[2], (g[3] if with_x else None), cut_cols(gq, d)


class ChanMixFn(torch.autograd.Function):
    """chan_mix_fwd / chan_mix_bwd as one differentiable op of (e1, e2, e3, q, x or None) -> (out, scores); the scores
    carry no gradient (MHCN reads them as ``attention_score`` only)."""

    @staticmethod
    def forward(ctx, e1, e2, e3, q, x, beta):
        out, score = chan_mix_fwd(e1, e2, e3, q, x, beta)
        ctx.save_for_backward(e1, e2, e3, q, score)
        ctx.beta, ctx.with_x = float(beta), x is not None
        ctx.mark_non_differentiable(score)
        return out, score

    @staticmethod
    def backward(ctx, gout, _gscore):
        e1, e2, e3, q, score = ctx.saved_tensors
        g1, g2, g3, gx, gq = chan_mix_bwd(e1, e2, e3, q, score, gout, ctx.beta, ctx.with_x)
        return g1, g2, g3, gq.reshape(q.shape), gx, None


def mim_fwd_bwd(em, edge, p1, p2, p3, c2, c3, loss_scale=1.0):
    """MHCN's hierarchical mutual-information loss (MHCN.py:159-181) of one channel, forward and backward in one call, with
    the shuffles given: p1, p2, p3 row permutations of n, c2, c3 column permutations of d.  edge = H @ em is the caller's
    SpMM.  Returns (loss (float64 scalar), dL/dem, dL/dedge), the gradients scaled by loss_scale.  -log(sigmoid(x)) is
    taken as softplus(-x): finite where the reference's form overflows."""
    n, d = int(em.shape[0]), int(em.shape[1])
    if em.dim() != 2 or tuple(edge.shape) != (n, d):
        raise SelfrecHipError("mim_fwd_bwd: em and edge must share one (n x d) shape")
    wd = kernel_width(d, TABLE_NCE_WIDTHS)
    dev = em.device
    rows = [p.to(device=dev, dtype=torch.int32).contiguous() for p in (p1, p2, p3)]
    cols = [c.to(device=dev, dtype=torch.int32).contiguous() for c in (c2, c3)]
    if any(int(p.numel()) != n for p in rows) or any(int(c.numel()) != d for c in cols):
        raise SelfrecHipError("mim_fwd_bwd: three permutations of n rows and two of d columns expected")
    if wd != d:       # the identity over the pad columns
        tail = torch.arange(d, wd, dtype=torch.int32, device=dev)
        cols = [torch.cat([c, tail]) for c in cols]
    emp, edp = to_width(em, wd), to_width(edge, wd)
    loss = torch.empty((), dtype=torch.float64, device=dev)
    g = torch.empty((2, n, wd), dtype=torch.float32, device=dev)
    a = _lib.MimArgs()
    a.d_em, a.d_edge = _p(emp, torch.float32, "em"), _p(edp, torch.float32, "edge")
    for i in range(3):
        a.d_row_perm[i] = rows[i].data_ptr()
    for i in range(2):
        a.d_col_perm[i] = cols[i].data_ptr()
    a.n, a.d, a.loss_scale = n, wd, float(loss_scale)
    a.d_loss, a.d_gem, a.d_gedge = _p(loss), g[0].data_ptr(), g[1].data_ptr()
    ws = workspace(_lib.load().srh_mim_ws_bytes(n, wd), dev)
    check(_lib.load().srh_mim_fwd_bwd(C.byref(a), _p(ws), _stream()), "srh_mim_fwd_bwd")
    return loss, cut_cols(g[0], d), cut_cols(g[1], d)


class MimFn(LossGradFn):
    """mim_fwd_bwd as one differentiable op of (em, edge); backward() scales the saved gradients by the upstream scalar
    (torch chains dL/dedge through the transposed SpMM)."""

    @staticmethod
    def forward(ctx, em, edge, p1, p2, p3, c2, c3):
        return LossGradFn.keep(ctx, *mim_fwd_bwd(em, edge, p1, p2, p3, c2, c3))
