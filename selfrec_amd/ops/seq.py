"""Sequence models (csrc/seqrec.hip): fused attention, the BCE loss, the embedding front, the segment and live-row sums."""
from __future__ import annotations

import functools

import numpy as np
import torch

from ._base import SelfrecHipError, _lib, _p, _stream, check, u64, workspace



def scatter_plan(ids, device):
    """The segments of srh_rows_segment_sum_f32 for gathered-row ids (host array): a stable sort of the rows by id, so
    each table row sums its rows in ascending row order.  -> (order, seg_start, seg_row) int32 device tensors."""
    return tuple(torch.from_numpy(a).to(device) for a in scatter_plan_host(ids))


def scatter_plan_host(ids):
    """scatter_plan's three int32 arrays on the host, for a caller that uploads them with its batch"""
    ids = np.ascontiguousarray(np.asarray(ids).reshape(-1), dtype=np.int64)
    order = np.argsort(ids, kind="stable")
    s = ids[order]
    first = np.flatnonzero(np.r_[True, s[1:] != s[:-1]]) if s.size else np.zeros(0, dtype=np.int64)
    seg_start = np.r_[first, s.size].astype(np.int32)
    seg_row = s[first].astype(np.int32)
    return tuple(np.ascontiguousarray(a, dtype=np.int32) for a in (order, seg_start, seg_row))


def rows_segment_sum(x, plan, out):
    """out[row] += the rows of x that plan (scatter_plan) names for it, in plan order: a deterministic index_add_."""
    order, seg_start, seg_row = plan
    n_rows, d = int(x.shape[0]), int(x.shape[1])
    if int(order.numel()) != n_rows or int(out.shape[1]) != d:
        raise SelfrecHipError("rows_segment_sum: the plan and the tables do not match")
    if int(seg_row.numel()) == 0:          # no segments: nothing to add (an empty tensor has no address to hand over)
        return out
    check(_lib.load().srh_rows_segment_sum_f32(_p(x.contiguous(), torch.float32, "x"), n_rows, d,
                                               _p(order, torch.int32, "order"), _p(seg_start, torch.int32, "seg_start"),
                                               _p(seg_row, torch.int32, "seg_row"), int(seg_row.numel()),
                                               int(out.shape[0]), _p(out, torch.float32, "out"), _stream()),
          "srh_rows_segment_sum_f32")
    return out


SEQ_ATTN_MAX_LEN = 64                         # srh_seq_attn_*: L <= 64, dh in SEQ_ATTN_HEAD_WIDTHS, H dh <= 128
SEQ_ATTN_HEAD_WIDTHS = (32, 64)
SEQ_ATTN_MAX_WIDTH = 128


def seq_attn_supported(L: int, H: int, dh: int) -> bool:
    """whether (L, H, dh) is inside the fused attention kernel's envelope (include/selfrec_hip.h)"""
    return 1 <= L <= SEQ_ATTN_MAX_LEN and dh in SEQ_ATTN_HEAD_WIDTHS and 1 <= H and H * dh <= SEQ_ATTN_MAX_WIDTH


def _attn_shape(q, k, v, n_heads, keep):
    """B, L, H, dh of the call and its keep mask as contiguous uint8 (None stays None)"""
    if q.dim() != 3 or q.shape != k.shape or q.shape != v.shape:
        raise SelfrecHipError("seq_attn: q, k, v must be (B, L, H * dh) tensors of one shape")
    B, L, E = (int(s) for s in q.shape)
    H = int(n_heads)
    if H < 1 or E % H:
        raise SelfrecHipError(f"seq_attn: width {E} does not split into {H} heads")
    if keep is not None:
        if tuple(keep.shape) != (B, H, L, L):
            raise SelfrecHipError(f"seq_attn: keep mask of shape {tuple(keep.shape)}, expected {(B, H, L, L)}")
        keep = keep.to(torch.uint8).contiguous()
    return B, L, H, E // H, keep


def _seq_attn_fwd(entry, q, k, v, n_heads, keep, drop_p, rng_seed, rng_counter):
    B, L, H, dh, keep = _attn_shape(q, k, v, n_heads, keep)
    out = torch.empty_like(q)
    lse = torch.empty((B, H, L), dtype=torch.float32, device=q.device)
    check(getattr(_lib.load(), entry)(_p(q, torch.float32, "q"), _p(k, torch.float32, "k"), _p(v, torch.float32, "v"),
                                      B, L, H, dh, _p(keep, torch.uint8, "keep"), u64(rng_seed), u64(rng_counter),
                                      float(drop_p), _p(out), _p(lse), _stream()), entry)
    return out, lse


def _seq_attn_bwd(entry, q, k, v, lse, go, n_heads, keep, drop_p, rng_seed, rng_counter):
    B, L, H, dh, keep = _attn_shape(q, k, v, n_heads, keep)
    go = go.to(torch.float32).contiguous()
    gq, gk, gv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    check(getattr(_lib.load(), entry)(_p(q, torch.float32, "q"), _p(k, torch.float32, "k"), _p(v, torch.float32, "v"),
                                      _p(go, torch.float32, "go"), _p(lse, torch.float32, "lse"), B, L, H, dh,
                                      _p(keep, torch.uint8, "keep"), u64(rng_seed), u64(rng_counter), float(drop_p),
                                      _p(gq), _p(gk), _p(gv), _stream()), entry)
    return gq, gk, gv


def seq_attn_fwd(q, k, v, n_heads, *, keep=None, drop_p=0.0, rng_seed=0, rng_counter=0):
    """Causal attention of projected q, k, v (B, L, H * dh): (out (B, L, H * dh), lse (B, H, L)).  Dropout on the
    probabilities: ``keep`` ((B, H, L, L), 1 = keep) replays a given mask; without it and with drop_p > 0 the mask is
    drawn in-kernel at the counters [rng_counter, rng_counter + B * H * L) (include/selfrec_hip.h)."""
    return _seq_attn_fwd("srh_seq_attn_fwd_f32", q, k, v, n_heads, keep, drop_p, rng_seed, rng_counter)


def seq_attn_bwd(q, k, v, lse, go, n_heads, *, keep=None, drop_p=0.0, rng_seed=0, rng_counter=0):
    """(dq, dk, dv) of seq_attn_fwd for the upstream gradient go, with the forward's dropout arguments."""
    return _seq_attn_bwd("srh_seq_attn_bwd_f32", q, k, v, lse, go, n_heads, keep, drop_p, rng_seed, rng_counter)


def seq_attn_full_fwd(q, k, v, n_heads, *, keep=None, drop_p=0.0, rng_seed=0, rng_counter=0):
    """seq_attn_fwd without a mask: every query attends to all L positions (BERT4Rec).  The same arguments, outputs
    and dropout contract."""
    return _seq_attn_fwd("srh_seq_attn_full_fwd_f32", q, k, v, n_heads, keep, drop_p, rng_seed, rng_counter)


def seq_attn_full_bwd(q, k, v, lse, go, n_heads, *, keep=None, drop_p=0.0, rng_seed=0, rng_counter=0):
    """(dq, dk, dv) of seq_attn_full_fwd for the upstream gradient go, with the forward's dropout arguments."""
    return _seq_attn_bwd("srh_seq_attn_full_bwd_f32", q, k, v, lse, go, n_heads, keep, drop_p, rng_seed, rng_counter)


class _SeqAttn(torch.autograd.Function):
    """the fused attention core as one differentiable op of (q, k, v): causal (seq_attn_fwd / seq_attn_bwd) or over all
    positions (seq_attn_full_fwd / seq_attn_full_bwd)"""

    @staticmethod
    def forward(ctx, causal, q, k, v, n_heads, keep, drop_p, rng_seed, rng_counter):
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        ctx.fwd_bwd = (seq_attn_fwd, seq_attn_bwd) if causal else (seq_attn_full_fwd, seq_attn_full_bwd)
        ctx.args = dict(keep=keep, drop_p=drop_p, rng_seed=rng_seed, rng_counter=rng_counter)
        out, lse = ctx.fwd_bwd[0](q, k, v, n_heads, **ctx.args)
        ctx.save_for_backward(q, k, v, lse)
        ctx.n_heads = n_heads
        return out

    @staticmethod
    def backward(ctx, go):
        q, k, v, lse = ctx.saved_tensors
        gq, gk, gv = ctx.fwd_bwd[1](q, k, v, lse, go, ctx.n_heads, **ctx.args)
        return None, gq, gk, gv, None, None, None, None, None


class SeqAttnFn:
    """seq_attn_fwd / seq_attn_bwd as one differentiable op of (q, k, v)."""
    apply = staticmethod(functools.partial(_SeqAttn.apply, True))


class SeqAttnFullFn:
    """seq_attn_full_fwd / seq_attn_full_bwd as one differentiable op of (q, k, v)."""
    apply = staticmethod(functools.partial(_SeqAttn.apply, False))


SEQ_ATTN_TILED_MAX_LEN = 512                  # srh_seq_attn_tiled_*: L <= 512, the widths of srh_seq_attn_*


def seq_attn_tiled_supported(L: int, H: int, dh: int) -> bool:
    """whether (L, H, dh) is inside the tiled attention kernels' envelope (include/selfrec_hip.h (a-25))"""
    return 1 <= L <= SEQ_ATTN_TILED_MAX_LEN and dh in SEQ_ATTN_HEAD_WIDTHS and 1 <= H and H * dh <= SEQ_ATTN_MAX_WIDTH


def seq_attn_tiled_fwd(q, k, v, n_heads, *, causal=True, keep=None, drop_p=0.0, rng_seed=0, rng_counter=0):
    """seq_attn_fwd (causal) or seq_attn_full_fwd (causal=False) for up to SEQ_ATTN_TILED_MAX_LEN positions, walked in
    64-key blocks: (out (B, L, H * dh), lse (B, H, L)), the same dropout contract."""
    B, L, H, dh, keep = _attn_shape(q, k, v, n_heads, keep)
    out = torch.empty_like(q)
    lse = torch.empty((B, H, L), dtype=torch.float32, device=q.device)
    check(_lib.load().srh_seq_attn_tiled_fwd_f32(_p(q, torch.float32, "q"), _p(k, torch.float32, "k"),
                                                 _p(v, torch.float32, "v"), B, L, H, dh, int(bool(causal)),
                                                 _p(keep, torch.uint8, "keep"), u64(rng_seed), u64(rng_counter),
                                                 float(drop_p), _p(out), _p(lse), _stream()), "srh_seq_attn_tiled_fwd_f32")
    return out, lse


def seq_attn_tiled_bwd(q, k, v, out, lse, go, n_heads, *, causal=True, keep=None, drop_p=0.0, rng_seed=0, rng_counter=0):
    """(dq, dk, dv) of seq_attn_tiled_fwd for the upstream gradient go, from the forward's out and lse and its dropout
    arguments."""
    B, L, H, dh, keep = _attn_shape(q, k, v, n_heads, keep)
    if out.shape != q.shape:
        raise SelfrecHipError("seq_attn_tiled_bwd: out must have the shape of q")
    go = go.to(torch.float32).contiguous()
    gq, gk, gv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    check(_lib.load().srh_seq_attn_tiled_bwd_f32(_p(q, torch.float32, "q"), _p(k, torch.float32, "k"),
                                                 _p(v, torch.float32, "v"), _p(out, torch.float32, "out"),
                                                 _p(go, torch.float32, "go"), _p(lse, torch.float32, "lse"), B, L, H, dh,
                                                 int(bool(causal)), _p(keep, torch.uint8, "keep"), u64(rng_seed),
                                                 u64(rng_counter), float(drop_p), _p(gq), _p(gk), _p(gv), _stream()),
          "srh_seq_attn_tiled_bwd_f32")
    return gq, gk, gv


class _SeqAttnTiled(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, n_heads, causal, keep, drop_p, rng_seed, rng_counter):
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        ctx.args = dict(causal=causal, keep=keep, drop_p=drop_p, rng_seed=rng_seed, rng_counter=rng_counter)
        out, lse = seq_attn_tiled_fwd(q, k, v, n_heads, **ctx.args)
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.n_heads = n_heads
        return out

    @staticmethod
    def backward(ctx, go):
        q, k, v, out, lse = ctx.saved_tensors
        gq, gk, gv = seq_attn_tiled_bwd(q, k, v, out, lse, go, ctx.n_heads, **ctx.args)
        return gq, gk, gv, None, None, None, None, None, None


class SeqAttnTiledFn:
    """seq_attn_tiled_fwd / seq_attn_tiled_bwd as one differentiable op of (q, k, v):
    apply(q, k, v, n_heads, causal=True, keep=None, drop_p=0.0, rng_seed=0, rng_counter=0)."""

    @staticmethod
    def apply(q, k, v, n_heads, causal=True, keep=None, drop_p=0.0, rng_seed=0, rng_counter=0):
        return _SeqAttnTiled.apply(q, k, v, n_heads, causal, keep, drop_p, rng_seed, rng_counter)


def seq_bce_fwd_bwd(hidden, table, pos, neg, valid, n_valid=None, ws=None):
    """SASRec.calculate_loss over hidden rows (R x d): (loss2 (2,) float64: the positive and the negative
    BCE-with-logits means over the rows with valid != 0, dL/dhidden (R x d), per-row table gradients (2R x d: rows of
    pos, then of neg)).  pos / neg: int32 item ids, valid: uint8, all of R entries on the device."""
    if hidden.dim() != 2 or table.dim() != 2 or hidden.shape[1] != table.shape[1]:
        raise SelfrecHipError("seq_bce: hidden (R x d) and table (n x d) expected")
    R, d = int(hidden.shape[0]), int(hidden.shape[1])
    for t, name in ((pos, "pos"), (neg, "neg"), (valid, "valid")):
        if int(t.numel()) != R:
            raise SelfrecHipError(f"seq_bce: {name} has {int(t.numel())} entries, expected {R}")
    if n_valid is None:
        n_valid = int(valid.count_nonzero().item())
    dev = hidden.device
    ws = workspace(_lib.load().srh_seq_bce_ws_bytes(R), dev, ws)
    loss2 = torch.empty(2, dtype=torch.float64, device=dev)
    gh = torch.empty((R, d), dtype=torch.float32, device=dev)
    grows = torch.empty((2 * R, d), dtype=torch.float32, device=dev)
    check(_lib.load().srh_seq_bce_fwd_bwd(_p(hidden, torch.float32, "hidden"), R, d, _p(table, torch.float32, "table"),
                                          int(table.shape[0]), _p(pos, torch.int32, "pos"), _p(neg, torch.int32, "neg"),
                                          _p(valid, torch.uint8, "valid"), int(n_valid), _p(loss2), _p(gh), _p(grows),
                                          _p(ws), _stream()), "srh_seq_bce_fwd_bwd")
    return loss2, gh, grows


class SeqBceFn(torch.autograd.Function):
    """The two BCE means of SASRec.calculate_loss as one kernel call; the item table's gradient is the deterministic
    segment sum of the per-row gradients (``plan`` = scatter_plan([pos; neg]))."""

    @staticmethod
    def forward(ctx, hidden, table, pos, neg, valid, n_valid, plan):
        loss2, gh, grows = seq_bce_fwd_bwd(hidden.contiguous(), table, pos, neg, valid, n_valid)
        ctx.save_for_backward(gh, grows)
        ctx.plan, ctx.table_shape = plan, tuple(table.shape)
        return (loss2[0].to(torch.float32) + loss2[1].to(torch.float32))

    table_grad = staticmethod(rows_segment_sum)

    @classmethod
    def backward(cls, ctx, gout):
        gh, grows = ctx.saved_tensors
        gt = cls.table_grad(grows, ctx.plan, torch.zeros(ctx.table_shape, dtype=torch.float32, device=gh.device))
        return gh * gout, gt * gout, None, None, None, None, None


class GatherRowsFn(torch.autograd.Function):
    """table[idx] whose table gradient is the deterministic segment sum (``plan`` = scatter_plan(idx)) instead of an
    atomic index_add."""

    @staticmethod
    def forward(ctx, table, idx, plan):
        ctx.plan, ctx.table_shape = plan, tuple(table.shape)
        return table[idx.long()]

    @staticmethod
    def backward(ctx, g):
        g2 = g.reshape(-1, ctx.table_shape[1]).to(torch.float32).contiguous()
        return rows_segment_sum(g2, ctx.plan, torch.zeros(ctx.table_shape, dtype=torch.float32, device=g.device)), None, None


SEQ_EMBED_WIDTHS = (32, 64, 128)              # srh_seq_embed_fwd_f32 / srh_rows_live_sum_f32
LIVE_SUM_CHUNK = 32                           # SRH_LIVE_SUM_CHUNK
LIVE_SUM_MAX_PROBLEMS = 3                     # SRH_LIVE_SUM_MAX_PROBLEMS


def seq_embed_supported(d: int) -> bool:
    return int(d) in SEQ_EMBED_WIDTHS


def seq_embed_fwd(item, pos_table, seq, posid, *, scale=None, keep=None, drop_p=0.0, rng_seed=0, rng_counter=0):
    """(R x d) rows (item[seq[r]] * scale + pos_table[posid[r]]) * m(r) for the rows with seq[r] != 0, exact zeros for the
    others (include/selfrec_hip.h (a-18)).  seq / posid: int32 device tensors of R entries; scale defaults to sqrt(d);
    ``keep`` ((R, d), 1 = keep) replays a dropout mask, without it and with drop_p > 0 the mask is drawn in-kernel at the
    counters [rng_counter, rng_counter + R)."""
    if item.dim() != 2 or pos_table.dim() != 2 or item.shape[1] != pos_table.shape[1]:
        raise SelfrecHipError("seq_embed: item (n x d) and position (m x d) tables expected")
    R, d = int(seq.numel()), int(item.shape[1])
    if int(posid.numel()) != R or R < 1:
        raise SelfrecHipError(f"seq_embed: {R} item ids and {int(posid.numel())} position ids")
    if keep is not None:
        if int(keep.numel()) != R * d:
            raise SelfrecHipError(f"seq_embed: keep mask of {int(keep.numel())} entries, expected {R} x {d}")
        keep = keep.to(torch.uint8).contiguous()
    out = torch.empty((R, d), dtype=torch.float32, device=item.device)
    check(_lib.load().srh_seq_embed_fwd_f32(_p(item, torch.float32, "item"), int(item.shape[0]),
                                            _p(pos_table, torch.float32, "pos_table"), int(pos_table.shape[0]),
                                            _p(seq, torch.int32, "seq"), _p(posid, torch.int32, "posid"), R, d,
                                            float(d ** 0.5 if scale is None else scale), _p(keep, torch.uint8, "keep"),
                                            u64(rng_seed), u64(rng_counter), float(drop_p), _p(out),
                                            _stream()), "srh_seq_embed_fwd_f32")
    return out


def live_plan_host(ids, live=None, chunk=LIVE_SUM_CHUNK):
    """The plan of srh_rows_live_sum_f32 for gathered-row ids (host array): the rows with ``live`` (default ids != 0)
    sorted stably by id, every id's segment cut into chunks of at most ``chunk`` rows.
    -> (rows, chunk_start, chunk_dst, multi_range, multi_row) int32 host arrays (include/selfrec_hip.h (a-18))."""
    ids = np.ascontiguousarray(np.asarray(ids).reshape(-1), dtype=np.int64)
    live = ids != 0 if live is None else np.asarray(live).reshape(-1).astype(bool)
    rows = np.flatnonzero(live)
    rows = rows[np.argsort(ids[rows], kind="stable")]
    s = ids[rows]
    first = np.flatnonzero(np.r_[True, s[1:] != s[:-1]]) if s.size else np.zeros(0, dtype=np.int64)
    length = np.diff(np.r_[first, s.size])
    n_chunks = (length + chunk - 1) // chunk                                     # chunks per segment
    chunk0 = np.r_[0, np.cumsum(n_chunks)].astype(np.int64)                      # first chunk of each segment
    seg_of_chunk = np.repeat(np.arange(first.size), n_chunks)
    within = np.arange(int(chunk0[-1])) - chunk0[seg_of_chunk]
    chunk_start = np.r_[first[seg_of_chunk] + within * chunk, s.size] if s.size else np.zeros(1, dtype=np.int64)
    chunk_dst = np.where(n_chunks[seg_of_chunk] == 1, s[first][seg_of_chunk], -1)
    multi = np.flatnonzero(n_chunks > 1)
    multi_range = np.stack([chunk0[multi], chunk0[multi + 1]], axis=1).reshape(-1)
    multi_row = s[first][multi]
    return tuple(np.ascontiguousarray(a, dtype=np.int32) for a in (rows, chunk_start, chunk_dst, multi_range, multi_row))


def live_plan(ids, device, live=None, chunk=LIVE_SUM_CHUNK):
    """live_plan_host's five arrays as int32 device tensors"""
    return tuple(torch.from_numpy(a).to(device) for a in live_plan_host(ids, live, chunk))


def rows_live_sum(problems):
    """srh_rows_live_sum_f32 over 1..3 problems, each a dict(x=(n x d), plan=live_plan(...), out=(table x d)[, scale=1.0,
    keep=None, drop_p=0.0, rng_seed=0, rng_counter=0]): out[row] = scale * the sum of the rows of x the plan lists for it,
    each times its dropout multiplier, in plan order.  Rows of out the plan does not name are left as they are."""
    lib = _lib.load()
    if not 1 <= len(problems) <= LIVE_SUM_MAX_PROBLEMS:
        raise SelfrecHipError(f"rows_live_sum: 1..{LIVE_SUM_MAX_PROBLEMS} problems per call")
    arr = (_lib.LiveSumProblem * len(problems))()
    d = int(problems[0]["x"].shape[1])
    hold = []
    for k, pr in enumerate(problems):
        x, out = pr["x"], pr["out"]
        rows, chunk_start, chunk_dst, multi_range, multi_row = pr["plan"]
        if x.dim() != 2 or out.dim() != 2 or int(x.shape[1]) != d or int(out.shape[1]) != d:
            raise SelfrecHipError("rows_live_sum: x (n x d) and out (table x d) of one width expected")
        n_chunk, n_multi = int(chunk_dst.numel()), int(multi_row.numel())
        if int(chunk_start.numel()) != n_chunk + 1 or int(multi_range.numel()) != 2 * n_multi:
            raise SelfrecHipError("rows_live_sum: the plan's arrays do not match")
        keep = pr.get("keep")
        if keep is not None:
            if int(keep.numel()) != int(x.shape[0]) * d:
                raise SelfrecHipError("rows_live_sum: the keep mask does not match x")
            keep = keep.to(torch.uint8).contiguous()
        x = x.contiguous()
        hold += [x, keep]
        a = arr[k]
        a.d_x, a.n_rows = _p(x, torch.float32, "x"), int(x.shape[0])
        a.d_rows, a.d_chunk_start = _p(rows, torch.int32, "rows"), _p(chunk_start, torch.int32, "chunk_start")
        a.d_chunk_dst = _p(chunk_dst, torch.int32, "chunk_dst")
        a.d_multi_range, a.d_multi_row = _p(multi_range, torch.int32, "multi_range"), _p(multi_row, torch.int32, "multi_row")
        a.n_live, a.n_chunk, a.n_multi = int(rows.numel()), n_chunk, n_multi
        a.d_out, a.n_table = _p(out, torch.float32, "out"), int(out.shape[0])
        a.scale, a.drop_p = float(pr.get("scale", 1.0)), float(pr.get("drop_p", 0.0))
        a.d_keep = _p(keep, torch.uint8, "keep")
        a.rng_seed, a.rng_counter = u64(pr.get("rng_seed", 0)), u64(pr.get("rng_counter", 0))
    need = int(lib.srh_rows_live_sum_ws_bytes(arr, len(problems), d))
    ws = workspace(need, problems[0]["x"].device) if need else None        # (no scratch needed: NULL)
    check(lib.srh_rows_live_sum_f32(arr, len(problems), d, _p(ws), _stream()), "srh_rows_live_sum_f32")
    return [pr["out"] for pr in problems]


class SeqEmbedFn(torch.autograd.Function):
    """The embedding front of the sequence encoder as one launch (seq_embed_fwd); both table gradients come from ONE
    rows_live_sum call over the live rows only: the item plan with scale sqrt(d), the position plan with scale 1, the
    dropout multiplier redrawn from the forward's arguments.  item_plan / pos_plan: live_plan of the item / position ids
    with live = (seq != 0)."""

    @staticmethod
    def forward(ctx, item, pos_table, seq, posid, item_plan, pos_plan, keep, drop_p, rng_seed, rng_counter):
        ctx.args = (seq, item_plan, pos_plan, keep, drop_p, rng_seed, rng_counter, tuple(item.shape), tuple(pos_table.shape))
        return seq_embed_fwd(item, pos_table, seq, posid, keep=keep, drop_p=drop_p, rng_seed=rng_seed,
                             rng_counter=rng_counter)

    @staticmethod
    def backward(ctx, g):
        seq, item_plan, pos_plan, keep, drop_p, rng_seed, rng_counter, item_shape, pos_shape = ctx.args
        d = item_shape[1]
        g = g.reshape(-1, d).to(torch.float32).contiguous()
        gi = torch.zeros(item_shape, dtype=torch.float32, device=g.device)
        gp = torch.zeros(pos_shape, dtype=torch.float32, device=g.device)
        drop = dict(keep=keep, drop_p=drop_p, rng_seed=rng_seed, rng_counter=rng_counter)
        rows_live_sum([dict(x=g, plan=item_plan, out=gi, scale=d ** 0.5, **drop), dict(x=g, plan=pos_plan, out=gp, **drop)])
        return gi, gp, None, None, None, None, None, None, None, None


class SeqBceLiveFn(SeqBceFn):
    """SeqBceFn with the item table's gradient summed over the valid rows of [pos; neg] only (``plan`` = live_plan of
    [pos; neg] with live = [valid; valid]): the rows the kernel zeroed are never walked."""

    @staticmethod
    def table_grad(grows, plan, gt):
        return rows_live_sum([dict(x=grows, plan=plan, out=gt)])[0]
