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


# ---- how csrc/knn.hip partitions its work (never what it outputs): the tests use these to show that a case reaches the
# path it is named for.  Mirrors of knn.hip's constants; a stale mirror shows as a failed "reaches its path" assertion.
NB_THREADS = 512                              # kNbThreads
NB_CHUNK = 32768                              # kNbChunk
NB_CAP = 1024                                 # kNbCap
SC_THREADS = 256                              # kScThreads
SC_CAP = 2048                                 # kScCap


def _kth_thread_maximum(thread, k):
    """keys sorted best first, thread[j] the owner of the j-th: the place of the k-th best of the owners' maxima, or None
    when fewer than k owners hold a key (the k-th maximum is then a sentinel, which comes after every real key)"""
    _, first = np.unique(thread, return_index=True)
    return int(np.sort(first)[k - 1]) if len(first) >= k else None


def neighbour_pass_counts(a, rank, q, k, shrinkage):
    """[(total, len0, raised), ...] of knn_neighbours_kernel for query row q, one tuple per NB_CHUNK-candidate pass:
    total keys (pass candidates and running-list entries) at or above the bound, the running list's length going in,
    whether the bound came from the list's k-th key.  The bound is the k-th best of the NB_THREADS maxima over the
    candidates i = t (mod NB_THREADS) of the pass; the sentinel maxima of empty threads come after every real key."""
    rank = np.asarray(rank, dtype=np.int64)
    norm = np.sqrt(np.diff(a.indptr).astype(np.float64))
    co = (a[[q]] @ a.T).tocsr()
    cand, n = co.indices.astype(np.int64), co.data.astype(np.int64)
    keep = (cand != q) & (n > 0)
    cand, n = cand[keep], n[keep]
    sim = (n / (n + shrinkage)) * (n / (norm[q] * norm[cand] + 1e-8))
    l_sim, l_rank = np.empty(0), np.empty(0, dtype=np.int64)      # the running list, best first
    out = []
    for c0 in range(0, a.shape[0], NB_CHUNK):
        sel = (cand >= c0) & (cand < c0 + NB_CHUNK)
        c_sim, c_rank, c_thr = sim[sel], rank[cand[sel]], (cand[sel] - c0) % NB_THREADS
        order = np.lexsort((-c_rank, -c_sim))
        c_sim, c_rank, c_thr = c_sim[order], c_rank[order], c_thr[order]
        len0 = len(l_sim)
        at = _kth_thread_maximum(c_thr, k)
        raised = len0 == k and (at is None or (l_sim[-1], l_rank[-1]) > (c_sim[at], c_rank[at]))
        if raised:
            b_sim, b_rank = l_sim[-1], l_rank[-1]
            total = int(((c_sim > b_sim) | ((c_sim == b_sim) & (c_rank >= b_rank))).sum()) + len0
        elif at is None:
            total = len(c_sim) + len0
        else:
            b_sim, b_rank = c_sim[at], c_rank[at]
            total = at + 1 + int(((l_sim > b_sim) | ((l_sim == b_sim) & (l_rank >= b_rank))).sum())
        out.append((total, len0, bool(raised)))
        m_sim, m_rank = np.concatenate([l_sim, c_sim]), np.concatenate([l_rank, c_rank])
        order = np.lexsort((-m_rank, -m_sim))[:k]
        l_sim, l_rank = m_sim[order], m_rank[order]
    return out


def score_pass_count(masked_row, k1):
    """keys of knn_score_topk_kernel's buffer for one finished (and masked) score row: the items at or above the k1-th
    best, by (score desc, id asc), of the SC_THREADS maxima over the items i = t (mod SC_THREADS)"""
    row = np.asarray(masked_row, dtype=np.float64)
    order = np.lexsort((np.arange(len(row)), -row))
    at = _kth_thread_maximum(order % SC_THREADS, k1)
    return len(row) if at is None else at + 1


def rank_top(masked_row, n_top):
    """(ids, scores, tied): the best n_top of the row by (score desc, id asc), and whether two adjacent scores among the
    best n_top + 1 are equal.  knn_score_topk writes this order, with ids[0] replaced by -1 - ids[0] where tied."""
    row = np.asarray(masked_row, dtype=np.float64)
    order = np.lexsort((np.arange(len(row)), -row))[:n_top + 1]
    top = row[order]
    return order[:n_top].astype(np.int64), top[:n_top], bool((top[1:] == top[:-1]).any())
