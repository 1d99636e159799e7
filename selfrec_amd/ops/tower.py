"""SSL4Rec (csrc/ssl4rec.hip): the two MLP towers."""
import ctypes as C

import torch

from ._base import SelfrecHipError, _lib, _p, _stream, check, u64, workspace
from .seq import rows_segment_sum, scatter_plan



TOWER_IN, TOWER_HIDDEN, TOWER_OUT = 64, 1024, 128


def _tower_weights(w1, b1, w2, b2):
    shapes = ((w1, (TOWER_HIDDEN, TOWER_IN)), (b1, (TOWER_HIDDEN,)), (w2, (TOWER_OUT, TOWER_HIDDEN)), (b2, (TOWER_OUT,)))
    for t, shape in shapes:
        if tuple(t.shape) != shape:
            raise SelfrecHipError(f"tower: weight of shape {tuple(t.shape)}, expected {shape} (Linear(64, 1024) -> ReLU -> "
                                  f"Linear(1024, 128) -> Tanh)")
    return _lib.TowerWeights(_p(w1, torch.float32, "w1"), _p(b1, torch.float32, "b1"), _p(w2, torch.float32, "w2"),
                             _p(b2, torch.float32, "b2"))


def tower_fwd(table, idx, w1, b1, w2, b2, *, mask_row0=None, mask=None, drop_p=0.0, rng_seed=0, rng_counter=0,
              save=True):
    """DNN_Encoder's tower (SSL4Rec.py:66-77) over rows table[idx] (table itself when idx is None): (y (n x 128),
    saved) with saved = (x, hidden, keep) for tower_bwd, or None when save is False.

    Rows r >= mask_row0 take nn.Dropout(drop_p): ``mask`` (uint8 (n - mask_row0, 64), 1 = keep) replays given masks;
    without it keep is drawn in-kernel at counter rng_counter + (r - mask_row0) (include/selfrec_hip.h) and returned in
    saved[2].  mask_row0 None: no dropout."""
    if table.dim() != 2 or int(table.shape[1]) != TOWER_IN:
        raise SelfrecHipError(f"tower: rows of {TOWER_IN} columns expected, got {tuple(table.shape)}")
    n = int(table.shape[0]) if idx is None else int(idx.numel())
    if n < 1:
        raise SelfrecHipError("tower: no rows")
    dev = table.device
    row0 = n if mask_row0 is None else int(mask_row0)
    n_mask = n - row0
    if mask is not None and tuple(mask.shape) != (n_mask, TOWER_IN):
        raise SelfrecHipError(f"tower: mask of shape {tuple(mask.shape)}, expected {(n_mask, TOWER_IN)}")
    ip = None if idx is None else idx.to(torch.int32).contiguous()
    w = _tower_weights(w1, b1, w2, b2)
    y = torch.empty((n, TOWER_OUT), dtype=torch.float32, device=dev)
    x = hidden = keep = None
    if save:
        x = torch.empty((n, TOWER_IN), dtype=torch.float32, device=dev)
        hidden = torch.empty((n, TOWER_HIDDEN), dtype=torch.float32, device=dev)
        if n_mask > 0:
            keep = mask.contiguous() if mask is not None else torch.empty((n_mask, TOWER_IN), dtype=torch.uint8, device=dev)
    mask_in = None if (mask is None or n_mask == 0) else mask.contiguous()
    mask_out = keep if (save and n_mask > 0 and mask is None) else None
    check(_lib.load().srh_tower_fwd_f32(_p(table, torch.float32, "table"), _p(ip, torch.int32, "idx"), n,
                                        int(table.shape[0]), C.byref(w), row0, _p(mask_in, torch.uint8, "mask"),
                                        u64(rng_seed), u64(rng_counter), float(drop_p if n_mask > 0 else 0.0),
                                        _p(mask_out), _p(x), _p(hidden), _p(y), _stream()), "srh_tower_fwd_f32")
    return y, ((x, hidden, keep) if save else None)


def tower_bwd(saved, y, gy, w1, b1, w2, b2, *, mask_row0=None, drop_p=0.0, ws=None):
    """Gradients of tower_fwd: (dX (n x 64, w.r.t. the gathered rows), dW1, db1, dW2, db2), every reduction over rows in
    a fixed order."""
    x, hidden, keep = saved
    n = int(x.shape[0])
    row0 = n if mask_row0 is None else int(mask_row0)
    dev = x.device
    w = _tower_weights(w1, b1, w2, b2)
    ws = workspace(_lib.load().srh_tower_bwd_ws_bytes(n), dev, ws)
    gx = torch.empty((n, TOWER_IN), dtype=torch.float32, device=dev)
    gw1, gb1 = torch.empty_like(w1), torch.empty_like(b1)
    gw2, gb2 = torch.empty_like(w2), torch.empty_like(b2)
    gy = gy.to(torch.float32).contiguous()
    check(_lib.load().srh_tower_bwd_f32(_p(x), _p(hidden), _p(y, torch.float32, "y"), _p(gy, torch.float32, "gy"), n,
                                        C.byref(w), row0, _p(keep, torch.uint8, "mask"),
                                        float(drop_p if keep is not None else 0.0), _p(gx), _p(gw1), _p(gb1), _p(gw2),
                                        _p(gb2), _p(ws), _stream()),
          "srh_tower_bwd_f32")
    return gx, gw1, gb1, gw2, gb2


class TowerFn(torch.autograd.Function):
    """y = tower(table[idx]) with the gradient of the WHOLE table (zero outside the rows idx names; repeated ids summed in
    ascending row order by ``plan`` = scatter_plan(idx)) and of the four weight tensors.  ``keep_out`` (optional list)
    receives the dropout keep mask the forward used."""

    @staticmethod
    def forward(ctx, table, w1, b1, w2, b2, idx, plan, mask_row0, mask, drop_p, rng_seed, rng_counter, keep_out):
        y, saved = tower_fwd(table, idx, w1, b1, w2, b2, mask_row0=mask_row0, mask=mask, drop_p=drop_p,
                             rng_seed=rng_seed, rng_counter=rng_counter)
        if keep_out is not None:
            keep_out.append(saved[2])
        ctx.save_for_backward(table, w1, b1, w2, b2, y)
        ctx.x, ctx.hidden, ctx.keep, ctx.idx, ctx.plan, ctx.mask_row0, ctx.drop_p = (*saved, idx, plan, mask_row0, drop_p)
        return y

    @staticmethod
    def backward(ctx, gy):
        table, w1, b1, w2, b2, y = ctx.saved_tensors
        gx, gw1, gb1, gw2, gb2 = tower_bwd((ctx.x, ctx.hidden, ctx.keep), y, gy, w1, b1, w2, b2, mask_row0=ctx.mask_row0,
                                           drop_p=ctx.drop_p)
        if ctx.idx is None:
            gt = gx
        else:
            plan = ctx.plan if ctx.plan is not None else scatter_plan(ctx.idx.cpu().numpy(), table.device)
            gt = rows_segment_sum(gx, plan, torch.zeros_like(table))
        return gt, gw1, gb1, gw2, gb2, None, None, None, None, None, None, None, None
