"""SEPT at the shape of conf/SEPT.yaml on the douban-book synthetic graph with generated trust pairs (B = 2048, d = 64,
n_layer 2, ins_cnt 10; n = the unique users of the first batch), timed with HIP events around each repeat (warm-up first;
median, min and max).  Every figure has torch's expression on the same GPU as its partner, and the two ALTERNATE inside
one run -- hip, torch, hip, torch ... -- so that a drift of the machine lands on both:
  * the tri-training step forward + backward: ops.TriNdFn (csrc/sept.hip) and the reference's expression on materialised
    n x n matrices (the ``engine.nd: torch`` route), and the peak memory each allocates above its inputs;
  * the NormPropFn chain (n_layer x l2_normalize(A x), forward + backward) over the normalised adjacency and over the
    friend view: ops.NormPropFn and torch's rsqrt / clamp expression around the same HIP SpMM (``engine.norm: torch``);
  * one whole joint step (four encoders, BPR, regulariser, tri-training, backward, torch Adam) by each pair of routes:
    wall time between fences.

    python tools/sept_probe.py [--out profiles/sept_probe.json] [--repeats 20]
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from selfrec_amd import ops, synth                                         # noqa: E402
from sasrec_probe import stats                                             # noqa: E402
from bert4rec_probe import peak_extra_bytes                                # noqa: E402


def alternating(fns, warmup, repeats, wall=False):
    """{name: stats of ms per call}: the partners take turns inside every repeat"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            if wall:
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts[name].append(1e3 * (time.perf_counter() - t0))
            else:
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                fn()
                t1.record()
                t1.synchronize()
                ts[name].append(t0.elapsed_time(t1))
    return {name: stats(v) for name, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/sept_probe.json")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--shape", default="douban-book", choices=sorted(synth.SHAPES))
    args = ap.parse_args()
    assert args.repeats >= 5
    ops.require_gpu()
    torch.cuda.set_device(0)
    from selfrec_amd.model.graph.SEPT import SEPT, TAU, l2_normalize, tri_nd_torch
    from selfrec_amd.util.conf import ModelConf
    from selfrec_amd.util.sampler import next_batch_pairwise
    B, d, k, L = 2048, 64, 10, 2
    tu, ti, su, si, _, _ = synth.make_dataset(args.shape)
    social = synth.make_social(args.shape)

    def make(nd, norm):
        conf = ModelConf({"training.set": "./none", "test.set": "./none", "model": {"name": "SEPT", "type": "graph"},
                          "item.ranking.topN": [10, 20], "embedding.size": d, "max.epoch": 30, "batch.size": B,
                          "learning.rate": 0.001, "reg.lambda": 0.0001, "output": "./results/",
                          "SEPT": {"n_layer": L, "ss_rate": 0.005, "drop_rate": 0.3, "ins_cnt": k},
                          "engine.nd": nd, "engine.norm": norm})
        torch.manual_seed(0)
        random.seed(0)
        m = SEPT(conf, synth.as_triples(tu, ti), synth.as_triples(su, si), **{"social.data": [list(p) for p in social]})
        m.model.cuda()
        m.redraw()
        return m

    models = {"hip": make("hip", "hip"), "torch": make("torch", "torch")}
    base = models["hip"]
    random.seed(1)
    batch = next(iter(next_batch_pairwise(base.data, B, as_arrays=True)))
    idx = [torch.from_numpy(a).cuda() for a in batch]
    uniq = torch.from_numpy(ops.unique_first(batch[0])).cuda()
    n = int(uniq.numel())
    res = {"shape": {"dataset": args.shape, "users": base.data.user_num, "items": base.data.item_num, "B": B, "d": d,
                     "n_layer": L, "ins_cnt": k, "unique_users_n": n, "trust_pairs": base.social_data.size()[1],
                     "friend_nnz": int(base.social_mat.nnz), "sharing_nnz": int(base.sharing_mat.nnz)}}

    # ---- tri_nd on the step's own views ---------------------------------------------------------------------------------
    with torch.no_grad():
        enc = base.model
        rec_u, _ = enc()
        aug_u, _ = enc(base.sub_mat)
        views = [enc.social(enc.friend_adj)[uniq], enc.social(enc.sharing_adj)[uniq], rec_u[uniq], aug_u[uniq]]
        views = [v.contiguous() for v in views]

    def nd(route):
        leaves = [v.detach().requires_grad_(True) for v in views]
        loss = ops.TriNdFn.apply(*leaves, k, TAU) if route == "hip" else tri_nd_torch(*leaves, k, TAU)[0]
        loss.backward()
    res["tri_nd_fwd_bwd_ms"] = alternating({r: (lambda r=r: nd(r)) for r in ("hip", "torch")}, 5, args.repeats)
    res["tri_nd_peak_extra_bytes"] = {r: peak_extra_bytes(lambda r=r: nd(r)) for r in ("hip", "torch")}
    res["tri_nd_one_matrix_bytes"] = 4 * n * n
    res["tri_nd_ws_bytes"] = int(ops._lib.load().srh_tri_nd_ws_bytes(n, d, k))

    # ---- the NormPropFn chain -------------------------------------------------------------------------------------------
    def chain(route, adj, x0, go):
        x = x0.detach().requires_grad_(True)
        y = x
        for _ in range(L):
            y = ops.NormPropFn.apply(adj, y) if route == "hip" else l2_normalize(torch.sparse.mm(adj, y))
        y.backward(go)
    g = torch.Generator().manual_seed(0)
    for name, adj, rows in (("norm_adj", enc.sparse_norm_adj, base.data.user_num + base.data.item_num),
                            ("friend", enc.friend_adj, base.data.user_num)):
        x0, go = (torch.randn(rows, d, generator=g).cuda() for _ in range(2))
        res[f"norm_prop_chain_{name}_ms"] = alternating(
            {r: (lambda r=r: chain(r, adj, x0, go)) for r in ("hip", "torch")}, 5, args.repeats)

    # ---- the whole joint step -------------------------------------------------------------------------------------------
    steps = {}
    for route, m in models.items():
        opt = torch.optim.Adam(m.model.parameters(), lr=1e-3)

        def step(m=m, opt=opt):
            _, _, loss = m.batch_losses(*idx, True, uniq=uniq)
            opt.zero_grad()
            loss.backward()
            opt.step()
        steps[route] = step
    res["joint_step_wall_ms"] = alternating(steps, 5, args.repeats, wall=True)
    res["joint_step_hip_over_torch"] = res["joint_step_wall_ms"]["hip"]["median"] / res["joint_step_wall_ms"]["torch"]["median"]
    res["tri_nd_hip_over_torch"] = res["tri_nd_fwd_bwd_ms"]["hip"]["median"] / res["tri_nd_fwd_bwd_ms"]["torch"]["median"]
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
