"""SASRec at the shape of conf/SASRec.yaml (B = 256, L = 50, d = 64, 2 blocks, 1 head; 12,101 items), timed with HIP
events around each repeat (warm-up first; median, min and max over the repeats):
  * the attention core forward + backward: ops.SeqAttnFn (csrc/seqrec.hip) and torch's expression on the same projected
    inputs (the ``engine.attention: torch`` route), with dropout 0.2 on the probabilities;
  * the loss with its gradients: ops.SeqBceFn (one kernel + the segment sum) and torch's expression (two gathers, two
    BCEWithLogitsLoss means, autograd);
  * one full training step each way (forward, loss, backward, torch Adam): wall time between fences with the batch's
    staging (scatter plans + upload) included, the same step on a pre-staged batch, and the staging alone;
  * the host sampling of one epoch (util/sampler.next_batch_sequence, plain Python) on the beauty-seq synthetic set.

    python tools/sasrec_probe.py [--out profiles/sasrec_probe.json] [--repeats 20]
"""
import argparse
import json
import os
import random
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, ".")
from selfrec_amd import ops, synth                                         # noqa: E402


def stats(ts):
    return {"median": float(np.median(ts)), "min": float(np.min(ts)), "max": float(np.max(ts)), "repeats": len(ts)}


def timed_events(fn, warmup, repeats):
    """ms per call, one HIP event pair per repeat"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        ts.append(t0.elapsed_time(t1))
    return stats(ts)


def timed_wall(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return stats(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/sasrec_probe.json")
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args()
    assert args.repeats >= 5
    ops.require_gpu()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    from selfrec_amd.model.sequential.SASRec import SASRec_Model, torch_causal_attention
    from selfrec_amd.util.loss_torch import l2_reg_loss
    B, L, d, H, n_items, p = 256, 50, 64, 1, 12101, 0.2
    res = {"shape": {"B": B, "L": L, "d": d, "heads": H, "blocks": 2, "items": n_items, "drop_rate": p}}

    g = torch.Generator().manual_seed(0)
    q, k, v, go = (torch.randn(B, L, d, generator=g).to(dev) for _ in range(4))

    def attn(route):
        qa, ka, va = (t.detach().requires_grad_(True) for t in (q, k, v))
        if route == "hip":
            out = ops.SeqAttnFn.apply(qa, ka, va, H, None, p, 1234, 0)
        else:
            out = torch_causal_attention(qa, ka, va, H, None, p, True)
        out.backward(go)
    res["attention_fwd_bwd_ms"] = {r: timed_events(lambda r=r: attn(r), 5, args.repeats) for r in ("hip", "torch")}

    rs = np.random.RandomState(0)
    seq = rs.randint(1, n_items + 1, size=(B, L))
    seq[:, 40:] = 0                                                      # a fifth of the positions padded
    pos = np.where(seq != 0, np.arange(1, L + 1)[None, :], 0)
    y, neg = rs.randint(1, n_items + 1, size=(B, L)), rs.randint(1, n_items + 1, size=(B, L))
    y[seq == 0] = 0
    neg[seq == 0] = 0
    table = (0.1 * torch.randn(n_items + 1, d, generator=g)).to(dev)
    hidden = torch.randn(B * L, d, generator=g).to(dev)
    valid_np = (pos.reshape(-1) != 0)
    y_t, neg_t = (torch.from_numpy(a.reshape(-1).astype(np.int32)).to(dev) for a in (y, neg))
    valid_t = torch.from_numpy(valid_np.astype(np.uint8)).to(dev)
    plan = ops.scatter_plan(np.concatenate([y.reshape(-1), neg.reshape(-1)]), dev)
    bce = torch.nn.BCEWithLogitsLoss()
    idx = torch.from_numpy(np.flatnonzero(valid_np)).to(dev)

    def loss(route):
        h, t = hidden.detach().requires_grad_(True), table.detach().requires_grad_(True)
        if route == "hip":
            out = ops.SeqBceFn.apply(h, t, y_t, neg_t, valid_t, int(valid_np.sum()), plan)
        else:
            pl, nl = (h * t[y_t.long()]).sum(-1), (h * t[neg_t.long()]).sum(-1)
            out = bce(pl[idx], torch.ones_like(pl[idx])) + bce(nl[idx], torch.zeros_like(nl[idx]))
        out.backward()
    res["bce_fwd_bwd_ms"] = {r: timed_events(lambda r=r: loss(r), 5, args.repeats) for r in ("hip", "torch")}

    from selfrec_amd.model.sequential.SASRec import StagedBatch

    def stage():
        return StagedBatch(seq, pos, y, neg, dev)
    # the step's host share: three stable argsorts (scatter plans) and the batch's one upload
    res["stage_batch_host_ms"] = timed_wall(stage, 5, args.repeats)

    step_ms = {}
    for route in ("hip", "torch"):
        torch.manual_seed(0)
        net = SASRec_Model(types.SimpleNamespace(item_num=n_items), d, L, 2, H, p, attention=route).cuda()
        net.train()
        opt = torch.optim.Adam(net.parameters(), lr=1e-3)
        pre = stage()

        def step(staged=None):
            b = stage() if staged is None else staged
            hid = net(seq, pos, staged=b)
            total = ops.SeqBceFn.apply(hid.reshape(-1, d), net.item_emb, b.y, b.neg, b.valid, b.n_valid,
                                       b.plans[2]) + l2_reg_loss(1e-4, net.item_emb)
            opt.zero_grad()
            total.backward()
            opt.step()
        # wall: as train() runs it, staging included; prestaged: the same step on a batch already on the device
        step_ms[route] = {"wall": timed_wall(step, 5, args.repeats),
                          "prestaged_wall": timed_wall(lambda: step(pre), 5, args.repeats),
                          "prestaged_events": timed_events(lambda: step(pre), 2, args.repeats)}
    res["step_ms"] = step_ms
    res["step_hip_over_torch"] = step_ms["hip"]["wall"]["median"] / step_ms["torch"]["wall"]["median"]
    res["step_host_share_ms"] = {r: step_ms[r]["wall"]["median"] - step_ms[r]["prestaged_wall"]["median"] for r in step_ms}

    from selfrec_amd.data.sequence import Sequence
    from selfrec_amd.util.sampler import next_batch_sequence
    train, test = synth.make_sequence_dataset("beauty-seq")
    data = Sequence({}, train, test)
    ts = []
    for r in range(5):
        random.seed(r)
        t0 = time.perf_counter()
        n_batches = sum(1 for _ in next_batch_sequence(data, B, max_len=L))
        ts.append(1e3 * (time.perf_counter() - t0))
    res["epoch_sampling_ms"] = dict(stats(ts), batches=n_batches, sequences=data.raw_seq_num,
                                    per_batch=float(np.median(ts)) / n_batches)
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
