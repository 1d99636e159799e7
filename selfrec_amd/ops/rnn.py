"""Recurrent models (csrc/gru.hip): the GRU recurrence as one launch each way, the layer around it, and the gather whose
table gradient walks the live rows only."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from ._base import SelfrecHipError, _lib, _p, _stream, check, cut_cols, to_width
from .seq import rows_live_sum

GRU_WIDTH = 64                                # srh_gru_*: H == 64 (narrower layers are zero-padded here), 1 <= L <= 512
GRU_MAX_LEN = 512


def gru_supported(L: int, H: int) -> bool:
    """whether a layer of H hidden units over L positions is inside the kernels' envelope (include/selfrec_hip.h (a-26)):
    H == 64, or 32 through the zero pad"""
    return 1 <= int(L) <= GRU_MAX_LEN and int(H) in (32, GRU_WIDTH)


def gru_lengths(lens, B, L, device):
    """the (B,) int32 device tensor of sequence lengths the kernels take.  The kernels never copy the lengths back, so
    0 <= len <= L is the caller's contract (they clamp, so a bad length only gives the wrong rows): a host array is
    checked here before it is uploaded, a device tensor is taken as it is."""
    if isinstance(lens, torch.Tensor) and lens.is_cuda:
        if int(lens.numel()) != int(B):
            raise SelfrecHipError(f"gru: {int(lens.numel())} lengths for {B} sequences")
        return lens.to(torch.int32).contiguous()
    host = np.ascontiguousarray(np.asarray(lens.cpu() if isinstance(lens, torch.Tensor) else lens).reshape(-1), dtype=np.int64)
    if host.size != int(B):
        raise SelfrecHipError(f"gru: {host.size} lengths for {B} sequences")
    if host.size and (host.min() < 0 or host.max() > int(L)):
        raise SelfrecHipError(f"gru: lengths must lie in [0, {int(L)}], got [{int(host.min())}, {int(host.max())}]")
    return torch.from_numpy(host.astype(np.int32)).to(device)


def _shape(t, last, name):
    if t.dim() != 3 or int(t.shape[2]) != last:
        raise SelfrecHipError(f"gru: {name} must be (B, L, {last}), got {tuple(t.shape)}")
    return int(t.shape[0]), int(t.shape[1])


def gru_fwd(gi, w_hh, b_hh, lens, save_gates=True):
    """The recurrence of one GRU layer from its input-side pre-activations gi (B, L, 3H): (out (B, L, H), gates (B, L, 4H)
    = [r, z, n, gh_n], or None without save_gates); rows at t >= len are exact zeros (header (a-26))."""
    H = int(w_hh.shape[1])
    B, L = _shape(gi, 3 * H, "gi")
    if tuple(w_hh.shape) != (3 * H, H) or tuple(b_hh.shape) != (3 * H,):
        raise SelfrecHipError("gru: w_hh must be (3H, H) and b_hh (3H,)")
    lens = gru_lengths(lens, B, L, gi.device)
    out = torch.empty((B, L, H), dtype=torch.float32, device=gi.device)
    gates = torch.empty((B, L, 4 * H), dtype=torch.float32, device=gi.device) if save_gates else None
    check(_lib.load().srh_gru_fwd_f32(_p(gi, torch.float32, "gi"), _p(w_hh, torch.float32, "w_hh"),
                                      _p(b_hh, torch.float32, "b_hh"), _p(lens, torch.int32, "len"), B, L, H, _p(out),
                                      _p(gates), _stream()), "srh_gru_fwd_f32")
    return out, gates


def gru_bwd(go, out, gates, w_hh, lens):
    """(dgi (B, L, 3H), dghn (B, L, H)) of gru_fwd for the upstream gradient go (B, L, H); zeros at t >= len, where go is
    never read."""
    H = int(w_hh.shape[1])
    B, L = _shape(go, H, "go")
    if tuple(out.shape) != (B, L, H) or tuple(gates.shape) != (B, L, 4 * H):
        raise SelfrecHipError("gru: out must be (B, L, H) and gates (B, L, 4H)")
    lens = gru_lengths(lens, B, L, go.device)
    dgi = torch.empty((B, L, 3 * H), dtype=torch.float32, device=go.device)
    dghn = torch.empty((B, L, H), dtype=torch.float32, device=go.device)
    check(_lib.load().srh_gru_bwd_f32(_p(go, torch.float32, "go"), _p(out, torch.float32, "out"),
                                      _p(gates, torch.float32, "gates"), _p(w_hh, torch.float32, "w_hh"),
                                      _p(lens, torch.int32, "len"), B, L, H, _p(dgi), _p(dghn), _stream()),
          "srh_gru_bwd_f32")
    return dgi, dghn


def _pad_gate_rows(w, H, Hp):
    """(3H, ...) -> (3Hp, ...): every gate's block of H rows followed by Hp - H zero rows"""
    if H == Hp:
        return w.contiguous()
    out = torch.zeros((3, Hp) + tuple(w.shape[1:]), dtype=w.dtype, device=w.device)
    out[:, :H] = w.reshape((3, H) + tuple(w.shape[1:]))
    return out.reshape((3 * Hp,) + tuple(w.shape[1:]))


def _cut_gate_rows(w, H, Hp):
    if H == Hp:
        return w
    return w.reshape((3, Hp) + tuple(w.shape[1:]))[:, :H].reshape((3 * H,) + tuple(w.shape[1:]))


def gru_pad_params(w_ih, w_hh, b_ih, b_hh, Hp=GRU_WIDTH):
    """a layer's four parameters at the kernel's width: a padded unit has zero weights and biases both ways, so its
    n = tanh(0) = 0 and h_0 = 0 keep it an exact 0 and every gradient that touches it is a zero"""
    H = int(w_hh.shape[1])
    if H > Hp:
        raise SelfrecHipError(f"gru: {H} hidden units -- the kernels serve up to {Hp}")
    w_hh_p = _pad_gate_rows(w_hh, H, Hp)
    if H != Hp:
        w_hh_p = to_width(w_hh_p, Hp)
    return _pad_gate_rows(w_ih, H, Hp), w_hh_p, _pad_gate_rows(b_ih, H, Hp), _pad_gate_rows(b_hh, H, Hp)


class GruFn(torch.autograd.Function):
    """One torch.nn.GRU layer (batch_first, h_0 = 0) over right-padded sequences, times the live mask, as a
    differentiable op of (x, w_ih, w_hh, b_ih, b_hh): F.linear for the input side, gru_fwd / gru_bwd for the recurrence,
    torch GEMMs on the zero-padded outputs for the parameter gradients.  lens: gru_lengths' argument."""

    @staticmethod
    def forward(ctx, x, w_ih, w_hh, b_ih, b_hh, lens):
        H, Hp = int(w_hh.shape[1]), GRU_WIDTH
        x = x.to(torch.float32).contiguous()
        B, L = int(x.shape[0]), int(x.shape[1])
        w_ih_p, w_hh_p, b_ih_p, b_hh_p = gru_pad_params(w_ih.detach(), w_hh.detach(), b_ih.detach(), b_hh.detach(), Hp)
        lens = gru_lengths(lens, B, L, x.device)
        save = any(ctx.needs_input_grad)
        out, gates = gru_fwd(F.linear(x, w_ih_p, b_ih_p), w_hh_p, b_hh_p, lens, save_gates=save)
        if save:
            ctx.save_for_backward(x, w_ih_p, w_hh_p, out, gates, lens)
        ctx.H = H
        return out if H == Hp else out[..., :H].contiguous()

    @staticmethod
    def backward(ctx, go):
        x, w_ih_p, w_hh_p, out, gates, lens = ctx.saved_tensors
        H, Hp = ctx.H, GRU_WIDTH
        B, L, D = (int(s) for s in x.shape)
        dgi, dghn = gru_bwd(to_width(go, Hp), out, gates, w_hh_p, lens)
        dgi2 = dgi.reshape(B * L, 3 * Hp)
        dgh2 = torch.cat((dgi[..., :2 * Hp], dghn), dim=-1).reshape(B * L, 3 * Hp)
        h_prev = torch.zeros_like(out)
        h_prev[:, 1:] = out[:, :-1]
        dx = (dgi2 @ w_ih_p).reshape(B, L, D)
        dw_ih = _cut_gate_rows(dgi2.t() @ x.reshape(B * L, D), H, Hp)
        db_ih = _cut_gate_rows(dgi2.sum(0), H, Hp)
        dw_hh = cut_cols(_cut_gate_rows(dgh2.t() @ h_prev.reshape(B * L, Hp), H, Hp), H)
        db_hh = _cut_gate_rows(dgh2.sum(0), H, Hp)
        return dx, dw_ih, dw_hh, db_ih, db_hh, None


class GatherLiveRowsFn(torch.autograd.Function):
    """table[idx] whose table gradient is ONE rows_live_sum call over the live rows only (``plan`` = live_plan(idx), live =
    idx != 0): the padding id's rows, the longest segment of a padded batch, are never walked and its gradient row is an
    exact zero."""

    @staticmethod
    def forward(ctx, table, idx, plan):
        ctx.plan, ctx.table_shape = plan, tuple(table.shape)
        return table[idx.long()]

    @staticmethod
    def backward(ctx, g):
        g2 = g.reshape(-1, ctx.table_shape[1]).to(torch.float32).contiguous()
        gt = torch.zeros(ctx.table_shape, dtype=torch.float32, device=g.device)
        return rows_live_sum([dict(x=g2, plan=ctx.plan, out=gt)])[0], None, None
