"""Host restatements for the NCL tests (no GPU, no faiss): the k-means of ops.kmeans in numpy float64,
and the structure-contrastive loss of reference model/graph/NCL.py:57-82 in torch float64.

``kmeans_np`` is also the body of the stub ``faiss`` module that tests/golden/make_golden_ncl.py installs when it runs
the reference's NCL.py (faiss is not installed): faiss.Kmeans(d, k)'s defaults -- niter 25, seed 1234, at most 256
points per centroid -- with the random choices made deterministic."""
import numpy as np

MAX_POINTS_PER_CENTROID = 256
SPLIT_EPS = 1.0 / 1024.0


def assign_np(x, c):
    """nearest centroid by |c_j|^2 - 2 x.c_j (lowest j on ties: np.argmin keeps the first); float64 distances"""
    x, c = np.asarray(x, dtype=np.float64), np.asarray(c, dtype=np.float64)
    part = (c * c).sum(1)[None, :] - 2.0 * (x @ c.T)
    ids = part.argmin(1)
    dist = np.maximum((x * x).sum(1) + part[np.arange(len(x)), ids], 0.0)
    return ids.astype(np.int64), dist


def update_np(x, ids, k):
    x = np.asarray(x, dtype=np.float64)
    counts = np.bincount(ids, minlength=k).astype(np.int64)
    sums = np.zeros((k, x.shape[1]), dtype=np.float64)
    np.add.at(sums, ids, x)
    cent = np.where(counts[:, None] > 0, sums / np.maximum(counts, 1)[:, None], 0.0)
    return cent, counts


def split_np(cent, counts):
    """every empty cluster, in ascending id, takes the largest cluster (lowest id on ties) as its donor"""
    for ci in np.flatnonzero(counts == 0):
        cj = int(np.argmax(counts))
        cent[ci] = cent[cj]
        cent[ci, 0::2] *= 1 + SPLIT_EPS
        cent[cj, 0::2] *= 1 - SPLIT_EPS
        cent[ci, 1::2] *= 1 - SPLIT_EPS
        cent[cj, 1::2] *= 1 + SPLIT_EPS
        counts[ci] = counts[cj] // 2
        counts[cj] -= counts[ci]


def kmeans_np(x, k, niter=25, seed=1234):
    """(centroids (k, d) float64, ids (n,) int64, final inertia): the definition ops.kmeans is held to"""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    n = len(x)
    if k > n:
        raise ValueError(f"k-means: {n} points are not enough for {k} centroids")
    perm = np.random.RandomState(seed).permutation(n)
    xt = x[perm[:MAX_POINTS_PER_CENTROID * k]] if n > MAX_POINTS_PER_CENTROID * k else x
    cent = x[perm[:k]].copy()
    for _ in range(niter):
        ids, _ = assign_np(xt, cent)
        cent, counts = update_np(xt, ids, k)
        split_np(cent, counts)
    ids, dist = assign_np(x, cent)
    return cent, ids, float(dist.sum())


def table_nce_torch(q, t, idx, tau):
    """sum_b -log(exp(q_b.t_idx[b]/tau) / sum_j exp(q_b.t_j/tau)) on F.normalize'd rows: NCL.py:59-69 (one side), in
    whatever dtype q and t carry (the tests pass float64)"""
    import torch
    import torch.nn.functional as F
    nq, nt = F.normalize(q), F.normalize(t)
    pos = torch.exp((nq * F.normalize(t[idx])).sum(dim=1) / tau)
    ttl = torch.exp(nq @ nt.T / tau).sum(dim=1)
    return -torch.log(pos / ttl).sum()
