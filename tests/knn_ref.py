"""float64 numpy / scipy restatement of UserKNN / ItemKNN (reference model/graph/UserKNN.py, ItemKNN.py) on id arrays.

Ratings are 1, so the similarity of rows q and v is a function of n = |q & v|, d_q, d_v; numpy's elementwise float64
operations round each step as python's floats do (no fused multiply-add), so these are the reference's bits."""
import heapq

import numpy as np
import scipy.sparse as sp


def binary_csr(rows, cols, n_rows, n_cols):
    """rows x cols 0/1 CSR (int64 values) of the distinct pairs"""
    m = sp.csr_matrix((np.ones(len(rows), dtype=np.int64), (np.asarray(rows), np.asarray(cols))), shape=(n_rows, n_cols))
    m.sum_duplicates()
    m.data[:] = 1
    return m


def name_ranks(names):
    order = sorted(range(len(names)), key=lambda k: names[k])
    rank = np.empty(len(names), dtype=np.int64)
    rank[order] = np.arange(len(names))
    return rank


def neighbours(a, rank, k, shrinkage, rows=None):
    """best k of each query row of the binary CSR a by (sim desc, rank desc): lists of (ids int64, sims float64)"""
    deg = np.diff(a.indptr)
    norm = np.sqrt(deg.astype(np.float64))
    rows = np.arange(a.shape[0]) if rows is None else np.asarray(rows, dtype=np.int64)
    co = (a[rows] @ a.T).tocsr()
    out = []
    for r, q in enumerate(rows.tolist()):
        lo, hi = co.indptr[r], co.indptr[r + 1]
        cand, n = co.indices[lo:hi].astype(np.int64), co.data[lo:hi].astype(np.int64)
        keep = (cand != q) & (n > 0)
        cand, n = cand[keep], n[keep]
        sim = (n / (n + shrinkage)) * (n / (norm[q] * norm[cand] + 1e-8))
        order = np.lexsort((-rank[cand], -sim))[:k]
        out.append((cand[order], sim[order]))
    return out


def score_row(side, u, user_items, lists, n_items):
    """predict() of UserKNN (side "user": lists over users) or ItemKNN (side "item": lists over items) for user id u;
    user_items[u]: u's training items in training-file order"""
    acc = np.zeros(n_items)
    if side == "user":
        for v, s in zip(*lists[u]):
            acc[np.asarray(user_items[v], dtype=np.int64)] += s
    else:
        for i in user_items[u]:
            ids, sims = lists[i]
            acc[ids] += sims
    touched = acc > 0
    acc[touched] = acc[touched] / (acc[touched] + 1e-8)
    return acc


def find_k_largest(k, candidates):
    """util/algorithm.py:144-156 (heapq on (score, position) tuples)"""
    heap = [(float(s), i) for i, s in enumerate(candidates[:k])]
    heapq.heapify(heap)
    for off, s in enumerate(candidates[k:]):
        if s > heap[0][0]:
            heapq.heapreplace(heap, (float(s), off + k))
    heap.sort(key=lambda d: d[0], reverse=True)
    return [p[1] for p in heap], [p[0] for p in heap]


def rank_row(row, train_items, k):
    row = row.copy()
    row[np.asarray(train_items, dtype=np.int64)] = -10e8
    return find_k_largest(k, row)
