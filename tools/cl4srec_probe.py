"""CL4SRec at the shape of conf/CL4SRec.yaml on the beauty-seq synthetic set (B = 256, L = 50, d = 64, 2 blocks, 1 head,
aug_type 0, drop_rate 0.2), timed with HIP events around each repeat (warm-up first; median, min and max over the repeats).
Partners are ALTERNATED inside one loop (a, b, a, b, ...), so a drift of the machine meets both alike:
  * the share of live rows of the batch and of the three stacked views;
  * the embedding front forward + backward: ops.SeqEmbedFn (csrc/seqrec.hip; table gradients over the live rows only) and
    the ``engine.embed: torch`` route (ops.GatherRowsFn twice, mul, add, dropout, mask; srh_rows_segment_sum_f32 over all
    rows), at R = 12,800 (one view) and R = 38,400 (three stacked);
  * the [y; neg] table gradient: srh_rows_live_sum_f32 on the plan of the valid rows and srh_rows_segment_sum_f32 on the
    plan of all 2R rows, over the same per-row gradients;
  * one full training step (staging, forward, losses, backward, torch Adam) for each of the four combinations of
    engine.views x engine.embed: device events and the wall time between fences;
  * the host time of staging (plans + upload) per combination and of the augmentation draws.

    python tools/cl4srec_probe.py [--out profiles/cl4srec_probe.json] [--repeats 20]
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
from sasrec_probe import stats, timed_wall                                 # noqa: E402


def alternated_events(fns, warmup, repeats):
    """{name: stats of ms per call}: every repeat runs each partner once, in turn, one HIP event pair per call"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            ts[name].append(t0.elapsed_time(t1))
    return {name: stats(v) for name, v in ts.items()}


def alternated_wall(fns, warmup, repeats):
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[name].append(1e3 * (time.perf_counter() - t0))
    return {name: stats(v) for name, v in ts.items()}


def verdict(pair, a, b):
    """'a' / 'b' when that partner's median beats the other's by more than either spread (max - min), else 'tie'"""
    sa, sb = pair[a], pair[b]
    spread = max(sa["max"] - sa["min"], sb["max"] - sb["min"])
    if sb["median"] - sa["median"] > spread:
        return a
    if sa["median"] - sb["median"] > spread:
        return b
    return "tie"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/cl4srec_probe.json")
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args()
    assert args.repeats >= 20                      # DESIGN.md 4.10's repeat count is the minimum
    ops.require_gpu()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    from selfrec_amd.model.sequential import CL4SRec as mod
    from selfrec_amd.util.conf import ModelConf
    from selfrec_amd.util.sampler import next_batch_sequence
    B, L, d, p = 256, 50, 64, 0.2
    train, test = synth.make_sequence_dataset("beauty-seq")

    def make(views, embed):
        conf = {"model": {"name": "CL4SRec", "type": "sequential"}, "item.ranking.topN": [10, 20], "embedding.size": d,
                "max.epoch": 1, "batch.size": B, "learning.rate": 0.001, "reg.lambda": 0.0001, "output": "./results/",
                "training.set": "x", "test.set": "y", "max.len": L, "engine.views": views, "engine.embed": embed,
                "CL4SRec": {"n_blocks": 2, "drop_rate": p, "n_heads": 1, "aug_type": 0, "aug_rate": 0.5, "cl_rate": 0.05}}
        torch.manual_seed(0)
        return mod.CL4SRec(ModelConf(conf), train, test)

    base = make("one", "hip")
    data = base.data
    random.seed(0); np.random.seed(0)
    seq, pos, y, neg, seq_len = next(iter(next_batch_sequence(data, B, max_len=L)))
    aug = base.augment(seq, pos, seq_len)
    views3 = [(seq, pos, None)] + list(aug)
    seq3 = np.concatenate([np.asarray(v[0]).reshape(-1) for v in views3])
    pos3 = np.concatenate([np.asarray(v[1]).reshape(-1) for v in views3])
    valid = pos.reshape(-1) != 0
    res = {"shape": {"B": B, "L": L, "d": d, "heads": 1, "blocks": 2, "table_rows": data.item_num + 2, "drop_rate": p,
                     "aug_type": 0, "aug_rate": 0.5, "repeats": args.repeats},
           "live_rows": {"batch": int(np.count_nonzero(seq)), "batch_share": float(np.count_nonzero(seq)) / seq.size,
                         "stacked": int(np.count_nonzero(seq3)), "stacked_share": float(np.count_nonzero(seq3)) / seq3.size,
                         "distinct_items_batch": int(np.unique(seq[seq != 0]).size),
                         "valid_targets": int(valid.sum()), "target_rows": int(2 * valid.size)}}

    g = torch.Generator().manual_seed(0)
    item = (0.1 * torch.randn(data.item_num + 2, d, generator=g)).to(dev)
    pos_table = (0.1 * torch.randn(L + 1, d, generator=g)).to(dev)
    res["embed_fwd_bwd_ms"] = {}
    for label, s_ids, p_ids in (("R12800", seq.reshape(-1), pos.reshape(-1)), ("R38400", seq3, pos3)):
        R = s_ids.size
        ids = torch.from_numpy(np.stack([s_ids, p_ids]).astype(np.int32)).to(dev)
        live = s_ids != 0
        plans_live = [ops.live_plan(s_ids, dev, live), ops.live_plan(p_ids, dev, live)]
        plans_all = [ops.scatter_plan(s_ids, dev), ops.scatter_plan(p_ids, dev)]
        live_t = torch.from_numpy(live).to(dev).unsqueeze(-1)
        go = torch.randn(R, d, generator=g).to(dev)
        drop = torch.nn.Dropout(p)

        def hip():
            a, b = item.detach().requires_grad_(True), pos_table.detach().requires_grad_(True)
            ops.SeqEmbedFn.apply(a, b, ids[0], ids[1], plans_live[0], plans_live[1], None, p, 1234, 0).backward(go)

        def torch_route():
            a, b = item.detach().requires_grad_(True), pos_table.detach().requires_grad_(True)
            x = ops.GatherRowsFn.apply(a, ids[0], plans_all[0]) * d ** 0.5 + ops.GatherRowsFn.apply(b, ids[1], plans_all[1])
            (drop(x) * live_t).backward(go)
        pair = alternated_events({"hip": hip, "torch": torch_route}, 5, args.repeats)
        pair["faster_beyond_spread"] = verdict(pair, "hip", "torch")
        res["embed_fwd_bwd_ms"][label] = pair

    # the [y; neg] table gradient over the BCE kernel's per-row gradients
    R = B * L
    hidden = torch.randn(R, d, generator=g).to(dev)
    yn = np.concatenate([y.reshape(-1), neg.reshape(-1)])
    ids = torch.from_numpy(np.stack([y.reshape(-1), neg.reshape(-1), valid]).astype(np.int32)).to(dev)
    _, _, grows = ops.seq_bce_fwd_bwd(hidden, item, ids[0], ids[1], ids[2].to(torch.uint8), int(valid.sum()))
    plan_live = ops.live_plan(yn, dev, np.concatenate([valid, valid]))
    plan_all = ops.scatter_plan(yn, dev)

    def grad_live():
        ops.rows_live_sum([dict(x=grows, plan=plan_live, out=torch.zeros_like(item))])

    def grad_all():
        ops.rows_segment_sum(grows, plan_all, torch.zeros_like(item))
    pair = alternated_events({"live_sum": grad_live, "segment_sum": grad_all}, 5, args.repeats)
    pair["faster_beyond_spread"] = verdict(pair, "live_sum", "segment_sum")
    res["target_table_grad_ms"] = pair

    # whole steps, the four route combinations in turn
    steps, stagers = {}, {}
    for views in ("one", "three"):
        for embed in ("hip", "torch"):
            model = make(views, embed)
            net = model.model.cuda()
            net.train()
            opt = torch.optim.Adam(net.parameters(), lr=1e-3)

            def step(model=model, opt=opt):
                loss, _, _ = model.step_losses(seq, pos, y, neg, aug)
                opt.zero_grad()
                loss.backward()
                opt.step()
            steps[f"{views}+{embed}"] = step
            stagers[f"{views}+{embed}"] = (lambda v=views, e=embed: mod.StagedViews(views3, y, neg, dev, v, e))
    res["step_events_ms"] = alternated_events(steps, 5, args.repeats)
    res["step_wall_ms"] = alternated_wall(steps, 2, args.repeats)
    for key in ("step_events_ms", "step_wall_ms"):
        t = res[key]
        t["views_faster_beyond_spread"] = {e: verdict(t, f"one+{e}", f"three+{e}") for e in ("hip", "torch")}
        t["embed_faster_beyond_spread"] = {v: verdict(t, f"{v}+hip", f"{v}+torch") for v in ("one", "three")}
    res["stage_host_ms"] = {k: timed_wall(fn, 3, args.repeats) for k, fn in stagers.items()}
    res["augment_host_ms"] = timed_wall(lambda: base.augment(seq, pos, seq_len), 3, args.repeats)
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
