"""Host restatement of the ranking kernels' contract (csrc/eval.hip, include/selfrec_hip.h: srh_gemm_nt_f32, srh_topk_rows,
srh_score_mask_topk(_filtered), srh_topk_hit_flags, srh_topk_trim_mark_ties) -- TEST INFRASTRUCTURE ONLY: numpy, no GPU,
none of the project's kernels.

The scores are not "a dot product within a tolerance": the header promises one particular float32 fma chain,

    acc = 0;  for s in 0 .. D/2 - 1:  acc = fma(u[s], i[s], acc);  acc = fma(u[D/2 + s], i[D/2 + s], acc)

so the restatement forms exactly that chain with a correctly rounded float32 fma (fma32) and everything downstream --
masking, (score desc, id asc) ranking, hit flags, tie marks -- is integer / comparison work that either matches or does not.
"""
import numpy as np

MASK_VALUE = np.float32(-10e8)          # graph_recommender.py:49-50 of the reference, mask_kernel / bound_rows_kernel


def fma32(a, b, c):
    """round_to_float32(a * b + c) with ONE rounding, elementwise (broadcasting), for float32-valued inputs.

    a * b is exact in float64 (24 + 24 significant bits).  s = fl64(p + c) and its TwoSum residual e give p + c = s + e
    exactly.  Rounding s to float32 is a second rounding, and it can differ from rounding p + c directly only when s sits
    exactly on a float32 midpoint (the 29 low bits of its significand are 1 0...0) while the true sum does not (e != 0):
    then s is moved one float64 ulp towards the true sum, which puts it on the true sum's side of the midpoint.  Valid
    while results stay in float32's normal range or are zero (midpoints of subnormals look different); no inf / nan."""
    p = np.multiply(a, b, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64)
    s = p + c
    bits = s.view(np.int64) if s.ndim else np.asarray(s).reshape(1).view(np.int64)
    mid = (bits & 0x1FFFFFFF) == 0x10000000
    if mid.any():
        p, c = np.broadcast_arrays(p, c)
        s = np.array(s, copy=True)
        sm, pm, cm = s[mid], p[mid], c[mid]
        bb = sm - pm
        e = (pm - (sm - bb)) + (cm - bb)
        s[mid] = np.where(e > 0, np.nextafter(sm, np.inf), np.where(e < 0, np.nextafter(sm, -np.inf), sm))
    return s.astype(np.float32)


def chain_scores(U, I, block=64):
    """(m, n) float32: every score by the documented chain, dimensions s and D/2 + s alternating, acc starting at 0."""
    U = np.ascontiguousarray(U, dtype=np.float32)
    I = np.ascontiguousarray(I, dtype=np.float32)
    m, d = U.shape
    n = I.shape[0]
    assert I.shape[1] == d and d % 2 == 0
    dh = d // 2
    it = np.ascontiguousarray(I.T.astype(np.float64))             # (d, n): one contiguous row per dimension
    out = np.empty((m, n), dtype=np.float32)
    for r0 in range(0, m, block):                                  # (row blocks keep the float64 temporaries small)
        u = U[r0:r0 + block].astype(np.float64)
        acc = np.zeros((u.shape[0], n), dtype=np.float32)
        for s in range(dh):
            acc = fma32(u[:, s, None], it[s][None, :], acc)
            acc = fma32(u[:, dh + s, None], it[dh + s][None, :], acc)
        out[r0:r0 + block] = acc
    return out


def rank(scores, k):
    """ids (rows, k) int32 and scores (rows, k) float32 of each row's k best entries: score descending, then id ascending."""
    scores = np.asarray(scores, dtype=np.float32)
    rows, n = scores.shape
    assert 1 <= k <= n
    ids = np.broadcast_to(np.arange(n, dtype=np.int64), scores.shape)
    order = np.lexsort((ids, -scores.astype(np.float64)), axis=-1)[:, :k]
    return order.astype(np.int32), np.take_along_axis(scores, order, axis=1)


def masked(scores, users, indptr, indices):
    """A copy of `scores` (row q belongs to user users[q]) with -10e8 over every user's training items."""
    out = np.array(scores, dtype=np.float32, copy=True)
    n = out.shape[1]
    for q, u in enumerate(np.asarray(users)):
        items = np.asarray(indices[indptr[u]:indptr[u + 1]])
        out[q, items[items < n]] = MASK_VALUE
    return out


def hit_flags(ids, users, t_indptr, t_indices):
    """uint8 (rows, k): 1 where ids[q][r] is in the (sorted) test row of user users[q] (q itself when users is None)."""
    ids = np.asarray(ids)
    flags = np.zeros(ids.shape, dtype=np.uint8)
    for q in range(ids.shape[0]):
        u = q if users is None else int(users[q])
        truth = set(int(t) for t in t_indices[t_indptr[u]:t_indptr[u + 1]])
        for r in range(ids.shape[1]):
            flags[q, r] = 1 if int(ids[q, r]) in truth else 0
    return flags


def trim_mark_ties(ids_k1, scores_k1):
    """(rows, k + 1) ranked ids / scores -> their first k columns; a row in which two neighbours of the k + 1 scores are
    equal gets ids[row][0] = -1 - id."""
    ids_k1, scores_k1 = np.asarray(ids_k1), np.asarray(scores_k1)
    rows, k1 = ids_k1.shape
    ids = np.array(ids_k1[:, :k1 - 1], dtype=np.int32, copy=True)
    sc = np.array(scores_k1[:, :k1 - 1], dtype=np.float32, copy=True)
    for r in range(rows):
        if any(scores_k1[r, c] == scores_k1[r, c + 1] for c in range(k1 - 1)):
            ids[r, 0] = -1 - ids[r, 0]
    return ids, sc
