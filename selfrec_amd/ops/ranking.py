"""Evaluation (csrc/eval.hip): masked scoring with top-k, the scoring GEMM, hit flags and per-user metrics."""
import ctypes as C

import numpy as np
import torch

from ._base import _lib, _p, _stream, check, workspace



def score_mask_topk(user_emb, user_ids, item_emb, r_indptr, r_indices, k, scores_ws=None):
    """ids, scores (device, (n_query, k)).  scores_ws: (rows, n_items) slab the queries pass through
    `rows` at a time inside the call (default: one slab for all queries)."""
    nq = int(user_ids.numel()) if user_ids is not None else int(user_emb.shape[0])
    n_items, d = int(item_emb.shape[0]), int(item_emb.shape[1])
    dev = item_emb.device
    if scores_ws is None:
        scores_ws = torch.empty((nq, n_items), dtype=torch.float32, device=dev)
    ids = torch.empty((nq, k), dtype=torch.int32, device=dev)
    sc = torch.empty((nq, k), dtype=torch.float32, device=dev)
    check(_lib.load().srh_score_mask_topk(_p(user_emb, torch.float32), _p(user_ids, torch.int32), nq,
                                          _p(item_emb, torch.float32), n_items, d, _p(r_indptr, torch.int32),
                                          _p(r_indices, torch.int32), int(k), _p(scores_ws, torch.float32),
                                          int(scores_ws.shape[0]), _p(ids, torch.int32), _p(sc, torch.float32),
                                          _stream()), "srh_score_mask_topk")
    return ids, sc


def score_mask_topk_filtered(user_emb, user_ids, item_emb, r_indptr, r_indices, k, *, sample_items=3072, cap=1024,
                             chunk_rows=4096, ws=None):
    """ids, scores, counts (device).  Rows with counts > cap are not valid (see include/selfrec_hip.h):
    rank those with score_mask_topk."""
    lib = _lib.load()
    nq = int(user_ids.numel()) if user_ids is not None else int(user_emb.shape[0])
    n_items, d = int(item_emb.shape[0]), int(item_emb.shape[1])
    dev = item_emb.device
    sample_items = max(int(k), min(int(sample_items), n_items))
    chunk_rows = max(1, min(int(chunk_rows), nq))
    need = int(lib.srh_score_mask_topk_filtered_ws_bytes(chunk_rows, sample_items, int(k), int(cap), n_items, d))
    ws = workspace(need, dev, ws)
    ids = torch.empty((nq, k), dtype=torch.int32, device=dev)
    sc = torch.empty((nq, k), dtype=torch.float32, device=dev)
    counts = torch.empty(nq, dtype=torch.int32, device=dev)
    check(lib.srh_score_mask_topk_filtered(_p(user_emb, torch.float32), _p(user_ids, torch.int32), nq,
                                           _p(item_emb, torch.float32), n_items, d, _p(r_indptr, torch.int32),
                                           _p(r_indices, torch.int32), int(k), sample_items, int(cap), chunk_rows,
                                           _p(ws), _p(ids, torch.int32), _p(sc, torch.float32),
                                           _p(counts, torch.int32), _stream()), "srh_score_mask_topk_filtered")
    return ids, sc, counts, ws


def topk_trim_mark_ties(ids_k1, scores_k1):
    """(rows, K + 1) ranked ids / scores -> (rows, K) with rows holding a tie among their K + 1 scores marked ids[:, 0] < 0
    (= -1 - id): one launch (srh_topk_trim_mark_ties)."""
    rows, k1 = int(ids_k1.shape[0]), int(ids_k1.shape[1])
    ids = torch.empty((rows, k1 - 1), dtype=torch.int32, device=ids_k1.device)
    sc = torch.empty((rows, k1 - 1), dtype=torch.float32, device=ids_k1.device)
    check(_lib.load().srh_topk_trim_mark_ties(_p(ids_k1, torch.int32), _p(scores_k1, torch.float32), rows, k1,
                                              _p(ids, torch.int32), _p(sc, torch.float32), _stream()), "srh_topk_trim_mark_ties")
    return ids, sc


def gemm_nt(a, b, out=None):
    m, d = int(a.shape[0]), int(a.shape[1])
    n = int(b.shape[0])
    if out is None:
        out = torch.empty((m, n), dtype=torch.float32, device=a.device)
    check(_lib.load().srh_gemm_nt_f32(_p(a, torch.float32), _p(b, torch.float32), _p(out, torch.float32), m, n, d,
                                      _stream()), "srh_gemm_nt_f32")
    return out


def topk_rows(scores, k):
    rows, n = int(scores.shape[0]), int(scores.shape[1])
    ids = torch.empty((rows, k), dtype=torch.int32, device=scores.device)
    sc = torch.empty((rows, k), dtype=torch.float32, device=scores.device)
    check(_lib.load().srh_topk_rows(_p(scores, torch.float32), rows, n, int(k), _p(ids, torch.int32),
                                    _p(sc, torch.float32), _stream()), "srh_topk_rows")
    return ids, sc


def topk_hit_flags(ids, user_ids, t_indptr, t_indices):
    """uint8 (n_query, k): 1 where the ranked id is one of the user's test items."""
    flags = torch.empty(ids.shape, dtype=torch.uint8, device=ids.device)
    check(_lib.load().srh_topk_hit_flags(_p(ids, torch.int32), int(ids.shape[0]), int(ids.shape[1]),
                                         _p(user_ids, torch.int32), _p(t_indptr, torch.int32),
                                         _p(t_indices, torch.int32), _p(flags, torch.uint8), _stream()),
          "srh_topk_hit_flags")
    return flags


def metric_rows(flags, sizes, cuts):
    """Per-user hits (int32) and DCG / IDCG (float64) at every cut-off of `cuts` (<= 8, each <= K) from the (users, K) hit
    flags and the users' test-set sizes (int32 device tensor): srh_metric_rows.  The gain table and the ideal prefix
    sums are computed HERE with python's math.log exactly as util/evaluation.py:66-78 computes them and handed to the
    kernel, so every quotient is the reference's bit for bit.  Returns (hits, ndcg) of shape (len(cuts), users)."""
    import math
    n, k = int(flags.shape[0]), int(flags.shape[1])
    cuts = [int(c) for c in cuts]
    gains = [1.0 / math.log(pos + 2, 2) for pos in range(k)]
    ideal = np.zeros((len(cuts), k + 1), dtype=np.float64)
    for c, cut in enumerate(cuts):
        acc = 0.0
        for m in range(1, cut + 1):
            acc = acc + 1.0 / math.log(m - 1 + 2, 2)        # sum(... for pos in range(m)): left to right
            ideal[c, m] = acc
    dev = flags.device
    d_gains = torch.tensor(gains, dtype=torch.float64, device=dev)
    d_ideal = torch.from_numpy(ideal).to(dev)
    hits = torch.empty((len(cuts), n), dtype=torch.int32, device=dev)
    ndcg = torch.empty((len(cuts), n), dtype=torch.float64, device=dev)
    arr = (C.c_int32 * len(cuts))(*cuts)
    check(_lib.load().srh_metric_rows(_p(flags, torch.uint8), _p(sizes, torch.int32), n, k, arr, len(cuts),
                                      _p(d_gains, torch.float64), _p(d_ideal, torch.float64), _p(hits, torch.int32),
                                      _p(ndcg, torch.float64), _stream()), "srh_metric_rows")
    return hits, ndcg
