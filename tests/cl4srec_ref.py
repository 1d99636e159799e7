"""float64 restatement of CL4SRec's own parts -- TEST INFRASTRUCTURE ONLY (the product never imports it).

Written from the semantics (include/selfrec_hip.h (a-18)), not from the reference's file: the embedding
front with an injected keep mask, the live-row segment sum, the InfoNCE of the views' last rows, and the step's loss over
tests/sasrec_ref.py's encoder.  tests/test_cl4srec_cpu.py pins it to the reference-run golden."""
import numpy as np
import torch

from tests import counter_rng, sasrec_ref


def embed_front(item, pos_table, seq, posid, keep=None, drop_p=0.0, scale=None):
    """(R, d): (item[seq[r]] * scale + pos_table[posid[r]]) * m(r) for the rows with seq[r] != 0, zeros for the others.
    keep: (R, d) 0 / 1 or None; m = keep / (1 - drop_p)."""
    seq = torch.as_tensor(np.asarray(seq).reshape(-1)).long()
    posid = torch.as_tensor(np.asarray(posid).reshape(-1)).long()
    d = item.shape[1]
    x = item[seq] * (d ** 0.5 if scale is None else scale) + pos_table[posid]
    if keep is not None:
        x = x * torch.as_tensor(np.asarray(keep), dtype=x.dtype).reshape(-1, d) / (1.0 - drop_p)
    return x * (seq != 0).unsqueeze(-1).to(x.dtype)


def embed_keep_drawn(seed, counter, R, d, p):
    """(R, d) bool: the keep mask srh_seq_embed_fwd_f32 draws -- row r at counter + r, column c the word c % 4 of float4
    c / 4, keep = u01(word) >= p"""
    ctr = counter_rng.counters(counter, R)
    w = counter_rng.rng4(ctr[:, None], np.arange(d // 4, dtype=np.uint32)[None, :], seed)          # (R, d / 4, 4)
    return counter_rng.u01(w).reshape(R, d) >= np.float32(p)


def live_sum(x, ids, live, n_table, scale=1.0, mult=None):
    """(n_table, d) float64: row t = scale * the sum of x[r] * mult[r] over the rows r with live[r] and ids[r] == t; the
    rows with live[r] false are not read (they may hold anything)"""
    x = np.asarray(x)
    out = np.zeros((n_table, x.shape[1]), dtype=np.float64)
    ids, live = np.asarray(ids).reshape(-1), np.asarray(live).reshape(-1).astype(bool)
    rows = np.flatnonzero(live)
    v = x[rows].astype(np.float64)
    if mult is not None:
        v = v * np.asarray(mult)[rows].astype(np.float64)
    np.add.at(out, ids[rows], v)
    return out * scale


def brute_force_plan(ids, live, chunk):
    """what ops.live_plan_host must return, by plain loops: the live rows grouped by id in ascending id, each group in
    ascending row order and cut into chunks of at most ``chunk`` rows"""
    ids, live = np.asarray(ids).reshape(-1), np.asarray(live).reshape(-1).astype(bool)
    groups = {}
    for r in range(ids.size):
        if live[r]:
            groups.setdefault(int(ids[r]), []).append(r)
    rows, chunk_start, chunk_dst, multi_range, multi_row = [], [0], [], [], []
    for t in sorted(groups):
        g = groups[t]
        pieces = [g[i:i + chunk] for i in range(0, len(g), chunk)]
        if len(pieces) > 1:
            multi_range += [len(chunk_dst), len(chunk_dst) + len(pieces)]
            multi_row.append(t)
        for piece in pieces:
            rows += piece
            chunk_start.append(len(rows))
            chunk_dst.append(t if len(pieces) == 1 else -1)
    return tuple(np.asarray(a, dtype=np.int32) for a in (rows, chunk_start, chunk_dst, multi_range, multi_row))


def info_nce(v1, v2, tau=1.0):
    """-mean_i log softmax_j(n(v1)_i . n(v2)_j / tau)[i], n = row normalisation (F.normalize: the norm clamped at 1e-12)"""
    n1 = v1 / v1.norm(dim=1, keepdim=True).clamp_min(1e-12)
    n2 = v2 / v2.norm(dim=1, keepdim=True).clamp_min(1e-12)
    s = n1 @ n2.T / tau
    return -(torch.diagonal(s) - torch.logsumexp(s, dim=1)).mean()


def last_rows(hidden, last):
    """row last[i] - 1 of sequence i: hidden (B, L, d), last: B 1-based lengths"""
    idx = torch.as_tensor(np.asarray(last, dtype=np.int64) - 1)
    return hidden[torch.arange(hidden.shape[0]), idx]


def step_losses(params, batch, views, n_blocks, n_heads, reg, cl_rate, stacked=False):
    """(batch loss, rec loss, cl_rate * InfoNCE) of one step.  batch: (seq, pos, y, neg); views: [(seq, pos, last)] * 2.
    stacked: the three encoder passes as one over [batch; view 1; view 2] -- the same function in exact arithmetic."""
    seq, pos, y, neg = (np.asarray(a) for a in batch[:4])
    B = seq.shape[0]
    if stacked:
        all_seq = np.concatenate([seq] + [np.asarray(v[0]) for v in views])
        all_pos = np.concatenate([pos] + [np.asarray(v[1]) for v in views])
        out = sasrec_ref.forward(params, all_seq, all_pos, n_blocks, n_heads)
        hidden, embs = out[:B], [out[B:2 * B], out[2 * B:]]
    else:
        hidden = sasrec_ref.forward(params, seq, pos, n_blocks, n_heads)
        embs = [sasrec_ref.forward(params, v[0], v[1], n_blocks, n_heads) for v in views]
    lp, ln = sasrec_ref.bce_means(hidden, params['item_emb'], y, neg, pos != 0)
    rec = lp + ln
    cl = cl_rate * info_nce(last_rows(embs[0], views[0][2]), last_rows(embs[1], views[1][2]), 1.0)
    l2 = reg * torch.linalg.norm(params['item_emb']) / params['item_emb'].shape[0]
    return rec + l2 + cl, rec, cl
