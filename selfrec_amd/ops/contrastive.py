"""Contrastive losses and NCL's k-means (csrc/contrastive.hip, ncl.hip): table InfoNCE, batch softmax, table CE, InfoNceFn."""
from __future__ import annotations

import numpy as np
import torch

from ._base import (NCE_WIDTHS, TABLE_NCE_WIDTHS, LossGradFn, SelfrecHipError, _lib, _p, _stream, check, cut_cols,
                    kernel_width, pad_cols, to_width, workspace)
from .step import infonce_multi, infonce_ws



def table_nce_ws(problems, d: int, device):
    """Workspace for srh_table_nce_fwd_bwd: problems = [(B, N), ...]."""
    lib = _lib.load()
    need = sum(int(lib.srh_table_nce_ws_bytes(int(b), int(n), int(d))) for b, n in problems)
    return torch.empty(need, dtype=torch.uint8, device=device)


def table_nce_fwd_bwd(problems, *, tau, ws=None):
    """InfoNCE of batch rows against a whole table, forward and backward in one call (NCL.py:57-83 ssl_layer_loss).

    problems: [(q, t, idx, loss_scale), ...] (one or two; NCL passes the user side and the item side): q (B x d) the
    gathered query rows, t (N x d) the whole table, idx (B) the positive row of each query in t.  Per problem
        loss = loss_scale * sum_b [ -q_b.t_idx[b] / tau + log sum_j exp(q_b.t_j / tau) ]   (rows F.normalize'd)
    Returns [(loss (0-dim float64), dL/dq (B x d), dL/dt (N x d)), ...], the gradients scaled by loss_scale.  Any d up
    to 128: narrower rows are zero-padded for the kernels, which changes no result."""
    if not 1 <= len(problems) <= 2:
        raise SelfrecHipError("table_nce_fwd_bwd: one or two problems per call")
    d = int(problems[0][0].shape[1])
    w = kernel_width(d, TABLE_NCE_WIDTHS, "table_nce_fwd_bwd", "the kernels serve")
    dev = problems[0][0].device
    arr = (_lib.TableNceProblem * len(problems))()
    keep, outs, shapes = [], [], []
    for k, (q, t, idx, scale) in enumerate(problems):
        if q.dim() != 2 or t.dim() != 2 or int(q.shape[1]) != d or int(t.shape[1]) != d:
            raise SelfrecHipError("table_nce_fwd_bwd: q and t must be 2-D with the same number of columns")
        if idx.dim() != 1 or int(idx.shape[0]) != int(q.shape[0]):
            raise SelfrecHipError("table_nce_fwd_bwd: idx must hold one entry per query row")
        qp, tp = to_width(q, w), to_width(t, w)
        ip = idx.to(torch.int32).contiguous()
        B, N = int(qp.shape[0]), int(tp.shape[0])
        loss = torch.empty((), dtype=torch.float64, device=dev)
        gq = torch.empty((B, w), dtype=torch.float32, device=dev)
        gt = torch.empty((N, w), dtype=torch.float32, device=dev)
        arr[k].d_q, arr[k].d_t, arr[k].d_idx = _p(qp, torch.float32, "q"), _p(tp, torch.float32, "t"), _p(ip, torch.int32, "idx")
        arr[k].B, arr[k].N, arr[k].loss_scale = B, N, float(scale)
        arr[k].d_loss, arr[k].d_gq, arr[k].d_gt = _p(loss), _p(gq), _p(gt)
        keep += [qp, tp, ip]
        outs.append((loss, gq, gt))
        shapes.append((B, N))
    ws = workspace(sum(int(_lib.load().srh_table_nce_ws_bytes(b, n, w)) for b, n in shapes), dev, ws)
    check(_lib.load().srh_table_nce_fwd_bwd(arr, len(problems), w, float(tau), _p(ws), _stream()), "srh_table_nce_fwd_bwd")
    return [(loss, cut_cols(gq, d), cut_cols(gt, d)) for loss, gq, gt in outs]


def _km_padded(x, what):
    """(pad_cols, not to_width: a table that is not float32 is refused by the call, not converted)"""
    return pad_cols(x, kernel_width(int(x.shape[1]), TABLE_NCE_WIDTHS, what))


def kmeans_assign(x, c):
    """Nearest centroid of every row of x (n x d) among c (k x d) by |c_j|^2 - 2 x.c_j, ties to the lowest j.
    Returns (ids (n,) int32, squared distances (n,) float32)."""
    n, k = int(x.shape[0]), int(c.shape[0])
    if int(c.shape[1]) != int(x.shape[1]):
        raise SelfrecHipError("kmeans_assign: x and c must have the same number of columns")
    xp, cp = _km_padded(x, "kmeans_assign"), _km_padded(c, "kmeans_assign")
    ids = torch.empty(n, dtype=torch.int32, device=x.device)
    dist = torch.empty(n, dtype=torch.float32, device=x.device)
    check(_lib.load().srh_kmeans_assign_f32(_p(xp, torch.float32, "x"), n, _p(cp, torch.float32, "c"), k, int(xp.shape[1]),
                                            _p(ids), _p(dist), _stream()), "srh_kmeans_assign_f32")
    return ids, dist


def kmeans_update(x, ids, k, ws=None):
    """Per-cluster means and counts of the rows of x (n x d) under ids (n,), each cluster summed in ascending row
    order (bit-identical from call to call).  Returns (centroids (k x d) float32, counts (k,) int32); an empty cluster
    has a zero centroid and count 0."""
    n, d = int(x.shape[0]), int(x.shape[1])
    ids = ids.to(torch.int32).contiguous()
    cent = torch.empty((int(k), d), dtype=torch.float32, device=x.device)
    counts = torch.empty(int(k), dtype=torch.int32, device=x.device)
    ws = workspace(_lib.load().srh_kmeans_update_ws_bytes(n, int(k)), x.device, ws)
    check(_lib.load().srh_kmeans_update_f32(_p(x, torch.float32, "x"), n, _p(ids, torch.int32, "ids"), int(k), d, _p(cent),
                                            _p(counts), _p(ws), _stream()), "srh_kmeans_update_f32")
    return cent, counts


KMEANS_MAX_POINTS_PER_CENTROID = 256          # faiss ClusteringParameters.max_points_per_centroid
KMEANS_SPLIT_EPS = 1.0 / 1024.0               # faiss Clustering.cpp split_clusters: EPS


def kmeans_split(centroids, counts):
    """faiss's empty-cluster handling made deterministic (host, in place): every empty cluster, in ascending id, takes
    the largest cluster (lowest id on ties) as its donor, copies its centroid with the +-1/1024 symmetric perturbation
    (even coordinates x(1+eps) on the empty one and x(1-eps) on the donor, odd the other way round) and half its
    count.  centroids: (k, d) float32 numpy, counts: (k,) int64 numpy.  Returns the number of splits."""
    eps = np.float32(KMEANS_SPLIT_EPS)
    up, down = np.float32(1) + eps, np.float32(1) - eps
    nsplit = 0
    for ci in np.flatnonzero(counts == 0):
        if counts[ci] != 0:
            continue
        cj = int(np.argmax(counts))
        centroids[ci] = centroids[cj]
        centroids[ci, 0::2] *= up
        centroids[cj, 0::2] *= down
        centroids[ci, 1::2] *= down
        centroids[cj, 1::2] *= up
        counts[ci] = counts[cj] // 2
        counts[cj] -= counts[ci]
        nsplit += 1
    return nsplit


def kmeans(x, k, niter=25, seed=1234, stats=None):
    """k-means of the rows of x (n x d, on the device) under the defaults of faiss.Kmeans(d, k) as NCL.py:37 uses it,
    with the random choices made deterministic:
      1. perm = np.random.RandomState(seed).permutation(n); n > 256 k: train on rows perm[:256 k]; initial centroids =
         rows perm[:k]
      2. niter times: assign (kmeans_assign), update (kmeans_update), split empty clusters (kmeans_split)
      3. assign all n rows against the final centroids (kmeans.index.search(x, 1))
    Returns (centroids (k, d) float32, assignment (n,) int64), both on the device.  ``stats`` (a dict, optional)
    receives the per-iteration objective (sum of squared distances, before that iteration's update) and the smallest
    count after each update's splits."""
    if x.dim() != 2:
        raise SelfrecHipError("kmeans: x must be 2-D")
    n, k = int(x.shape[0]), int(k)
    if k < 1:
        raise SelfrecHipError("kmeans: k must be >= 1")
    if k > n:
        raise SelfrecHipError(f"kmeans: {n} points are not enough to train {k} centroids (need k <= n)")
    d = int(x.shape[1])
    x = x.detach().float().contiguous()
    xp = _km_padded(x, "kmeans")
    perm = np.random.RandomState(seed).permutation(n)
    if n > KMEANS_MAX_POINTS_PER_CENTROID * k:
        xt = xp.index_select(0, torch.from_numpy(perm[:KMEANS_MAX_POINTS_PER_CENTROID * k]).to(xp.device)).contiguous()
    else:
        xt = xp
    cent = xp.index_select(0, torch.from_numpy(perm[:k]).to(xp.device)).contiguous()
    ws = workspace(_lib.load().srh_kmeans_update_ws_bytes(int(xt.shape[0]), k), x.device)
    if stats is not None:
        stats.setdefault("obj", [])
        stats.setdefault("min_count", [])
    for _ in range(int(niter)):
        ids, dist = kmeans_assign(xt, cent)
        if stats is not None:
            stats["obj"].append(float(dist.double().sum()))
        cent, counts = kmeans_update(xt, ids, k, ws)
        counts_h = counts.cpu().numpy().astype(np.int64)
        if (counts_h == 0).any():
            cent_h = cent.cpu().numpy()
            kmeans_split(cent_h, counts_h)
            cent = torch.from_numpy(cent_h).to(x.device)
        if stats is not None:
            stats["min_count"].append(int(counts_h.min()))
    ids, _ = kmeans_assign(xp, cent)
    return cut_cols(cent, d).contiguous(), ids.long()


def batch_softmax_fwd_bwd(u, v, tau, ws=None):
    """batch_softmax_loss (util/loss_torch.py:25-32) and its gradients: (loss (0-dim float64), dL/du, dL/dv).  Rows up to
    128 columns (narrower ones zero-padded: no result changes)."""
    if u.dim() != 2 or u.shape != v.shape:
        raise SelfrecHipError("batch_softmax: u and v must be 2-D of the same shape")
    B, d = int(u.shape[0]), int(u.shape[1])
    w = kernel_width(d, TABLE_NCE_WIDTHS, "batch_softmax")
    up, vp = to_width(u, w), to_width(v, w)
    dev = u.device
    ws = workspace(_lib.load().srh_batch_softmax_ws_bytes(B, w), dev, ws)
    loss = torch.empty((), dtype=torch.float64, device=dev)
    gu = torch.empty((B, w), dtype=torch.float32, device=dev)
    gv = torch.empty((B, w), dtype=torch.float32, device=dev)
    check(_lib.load().srh_batch_softmax_fwd_bwd(_p(up, torch.float32, "u"), _p(vp, torch.float32, "v"), B, w, float(tau),
                                                _p(loss), _p(gu), _p(gv), _p(ws), _stream()),
          "srh_batch_softmax_fwd_bwd")
    return loss, cut_cols(gu, d), cut_cols(gv, d)


class BatchSoftmaxFn(LossGradFn):
    """batch_softmax_loss as one kernel call: loss and both gradients come out together; backward() scales them."""

    @staticmethod
    def forward(ctx, u, v, tau):
        return LossGradFn.keep(ctx, *batch_softmax_fwd_bwd(u, v, tau))


def table_ce_fwd_bwd(hidden_rows, table, labels, loss_scale=1.0, ws=None):
    """Softmax cross-entropy of the rows (M x d) against the whole table (N x d), logits h_m . t_j:
    (loss (0-dim float64) = loss_scale * sum_m (lse_m - s_{m, label_m}), dL/dhidden_rows (M x d), dL/dtable (N x d, dense)).
    labels: int32 device tensor of M entries in [0, N).  The M x N logits are never materialised.  Rows up to 128 columns
    (narrower ones zero-padded: no result changes)."""
    if hidden_rows.dim() != 2 or table.dim() != 2 or hidden_rows.shape[1] != table.shape[1]:
        raise SelfrecHipError("table_ce: rows (M x d) and table (N x d) expected")
    M, d = int(hidden_rows.shape[0]), int(hidden_rows.shape[1])
    N = int(table.shape[0])
    if int(labels.numel()) != M:
        raise SelfrecHipError(f"table_ce: labels has {int(labels.numel())} entries, expected {M}")
    w = kernel_width(d, TABLE_NCE_WIDTHS, "table_ce")
    _p(hidden_rows, None, "hidden_rows"), _p(table, None, "table")
    hp, tp = to_width(hidden_rows, w), to_width(table, w)
    dev = hidden_rows.device
    ws = workspace(_lib.load().srh_table_ce_ws_bytes(M, N, w), dev, ws)
    loss = torch.empty((), dtype=torch.float64, device=dev)
    gh = torch.empty((M, w), dtype=torch.float32, device=dev)
    gt = torch.empty((N, w), dtype=torch.float32, device=dev)
    check(_lib.load().srh_table_ce_fwd_bwd(_p(hp, torch.float32, "hidden_rows"), M, _p(tp, torch.float32, "table"), N, w,
                                           _p(labels, torch.int32, "labels"), float(loss_scale), _p(loss), _p(gh), _p(gt),
                                           _p(ws), _stream()), "srh_table_ce_fwd_bwd")
    return loss, cut_cols(gh, d), cut_cols(gt, d)


class TableCeFn(LossGradFn):
    """table_ce_fwd_bwd as one differentiable op of (hidden_rows, table): loss and both gradients come out of the one
    call; backward() scales them by the upstream scalar."""

    @staticmethod
    def forward(ctx, hidden_rows, table, labels, loss_scale):
        return LossGradFn.keep(ctx, *table_ce_fwd_bwd(hidden_rows, table, labels, loss_scale))


class InfoNceFn(torch.autograd.Function):
    """util/loss_torch.py InfoNCE(v1, v2, tau, b_cos=True) of two (n x d) row sets as one differentiable op over
    srh_infonce_fwd_bwd_multi (idx = NULL: row i of the gradients belongs to row i).  The gradients start at zero and g2 is
    a table of its own, so it is declared exclusive: plain stores instead of float atomics.  d in NCE_WIDTHS."""

    @staticmethod
    def forward(ctx, v1, v2, tau):
        n, d = int(v1.shape[0]), int(v1.shape[1])
        if v1.shape != v2.shape or d not in NCE_WIDTHS:
            raise SelfrecHipError(f"InfoNceFn: two (n x d) views with d in {NCE_WIDTHS} expected")
        v1, v2 = v1.to(torch.float32).contiguous(), v2.to(torch.float32).contiguous()
        dev = v1.device
        buf = torch.zeros(2 * n * d + 2, dtype=torch.float32, device=dev)       # [g1 | g2 | loss (one double)]
        g = buf[:2 * n * d].view(2, n, d)
        loss = buf[2 * n * d:].view(torch.float64)
        infonce_multi([(v1, v2, None, n, None, g[0], g[1], True)], d=d, tau=float(tau), loss_scale=1.0, loss=loss,
                      ws=infonce_ws(n, d, dev))
        ctx.save_for_backward(g)
        return loss.to(torch.float32).reshape(())

    @staticmethod
    def backward(ctx, gout):
        g = ctx.saved_tensors[0] * gout
        return g[0], g[1], None
