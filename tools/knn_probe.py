"""UserKNN / ItemKNN at the Yelp2018 shape (synthetic, 31,668 users x 38,048 items, topK 50, shrinkage 100, N = 20),
timed between device fences after a warm-up call:
  * the neighbour search of each model (ops.knn_neighbours over every row), with its gather count sum_f deg_f^2 and the
    bound that count sets: 4 B per gathered index at 6.3 TB/s (MI355X_MICROARCH.md, HBM) -- a bound on reading the
    transposed CSR once per increment, though that 6 MB array mostly stays in cache;
  * scoring and ranking every test user (ops.knn_score_topk + the host heap walk over the tied rows), and how many rows
    the host redid;
  * the float64 numpy / scipy restatement (tests/knn_ref.py) on the CPU over 256 rows, scaled to all rows, as the baseline.

    python tools/knn_probe.py [--out profiles/knn_probe.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from selfrec_amd import _lib, ops, synth                                    # noqa: E402
from selfrec_amd.model.graph._knn import _csr                              # noqa: E402
from tests import knn_ref                                                  # noqa: E402

HBM_TBS = 6.3


def timed(fn, warmup=1, iters=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts)), 1e3 * float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/knn_probe.json")
    args = ap.parse_args()
    _lib.require_gpu()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    tu, ti, su, si, U, I = synth.make_dataset("yelp2018")
    K, S, N = 50, 100, 20
    r = knn_ref.binary_csr(tu, ti, U, I)
    rng = np.random.default_rng(0)
    out = {"shape": {"users": U, "items": I, "train": int(r.nnz), "topK": K, "shrinkage": S, "N": N}}
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    up, ui = _csr(tu.astype(np.int64), ti.astype(np.int64), U)               # users -> items, training order
    lists = {}
    for name, a in (("UserKNN", r), ("ItemKNN", r.T.tocsr())):
        tr = a.T.tocsr()
        tr.sort_indices()
        rank = rng.permutation(a.shape[0])
        argv = (t(a.indptr, np.int32), t(a.indices, np.int32), t(tr.indptr, np.int32), t(tr.indices, np.int32),
                t(np.sqrt(np.diff(a.indptr).astype(np.float64)), np.float64), t(rank, np.int32))
        med, mn = timed(lambda: ops.knn_neighbours(*argv, K, S))
        lists[name] = ops.knn_neighbours(*argv, K, S)
        gathers = int((np.diff(tr.indptr).astype(np.int64) ** 2).sum())
        bound_ms = gathers * 4 / (HBM_TBS * 1e12) * 1e3
        rows = rng.choice(a.shape[0], 256, replace=False)
        t0 = time.perf_counter()
        knn_ref.neighbours(a, rank, K, S, rows=rows)
        cpu_s = (time.perf_counter() - t0) * a.shape[0] / len(rows)
        out[name] = {"neighbours_ms": {"median": med, "min": mn}, "gathers": gathers,
                     "gather_bytes_bound_ms": bound_ms, "fraction_of_bound": bound_ms / med,
                     "increments_per_s": gathers / (med * 1e-3),
                     "cpu_restatement_s_scaled": cpu_s, "speedup_vs_cpu_restatement": cpu_s * 1e3 / med}
    test_users = np.unique(su).astype(np.int32)
    uid = t(test_users, np.int32)
    for name, side in (("UserKNN", "user"), ("ItemKNN", "item")):
        ids, sims, lens = lists[name]
        ws = ops.knn_score_ws(1024, I, dev)

        def rank_all():
            i_d, s_d, _ = ops.knn_score_topk(side, uid, t(up, np.int32), t(ui, np.int32), I, ids, sims, lens, N, ws=ws)
            return i_d.cpu().numpy(), s_d.cpu().numpy()

        med, mn = timed(rank_all)
        i_h, _ = rank_all()
        marked = np.flatnonzero(i_h[:, 0] < 0)
        # the host's share: each marked row's score row back from the device and walked (ops.find_k_largest_host_f64)
        redo_s = 0.0
        if marked.size:
            rows_t = t(test_users[marked[:1024]], np.int32)
            _, _, ws2 = ops.knn_score_topk(side, rows_t, t(up, np.int32), t(ui, np.int32), I, ids, sims, lens, N,
                                           ws_rows=1024)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rows_h = ws2[:8 * I * len(marked[:1024])].view(torch.float64).view(-1, I).cpu().numpy()
            for row in rows_h:
                ops.find_k_largest_host_f64(N, row)
            redo_s = (time.perf_counter() - t0) * len(marked) / min(1024, len(marked))
        out[name]["score_rank_test_users"] = {"users": int(len(test_users)), "device_ms": {"median": med, "min": mn},
                                              "rows_redone_on_host": int(len(marked)),
                                              "host_redo_ms_scaled": 1e3 * redo_s}
    out["device"] = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
