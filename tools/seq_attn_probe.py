"""The tiled attention kernels (srh_seq_attn_tiled_*) against torch's expression on the same GPU in the same
run, the two routes ALTERNATED repeat by repeat, one HIP event pair per repeat (5 warm-ups, 30 repeats; median, min, max):
  * the attention core forward + backward at B = 256, H = 1, dh = 64, dropout 0.2 on the probabilities, L in {100, 200, 512},
    causal and full: ops.SeqAttnTiledFn and torch_causal_attention on the same projected inputs (the ``engine.attention:
    torch`` route), and the peak memory each allocates above its inputs;
  * one whole SASRec training step (forward, BCE, backward, torch Adam) on a batch of the ml1m-seq synthetic set at
    max.len 200 by ``engine.attention: tiled`` (recorded as "hip": the kernels) and by ``torch``, batch pre-staged.
The partner is torch's expression at the same commit, never the kernel against itself.  ``default_rule`` records the rule of
DESIGN.md 4.28: the tiled route is the default above 64 positions if its median is at or below torch's at L = 100 and at
L = 200 in both flavours.

    python tools/seq_attn_probe.py [--out profiles/seq_attn_tiled_probe.json] [--repeats 30]
"""
import argparse
import json
import os
import random
import sys
import types

import numpy as np
import torch

sys.path.insert(0, ".")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from selfrec_amd import ops, synth                                         # noqa: E402
from bert4rec_probe import peak_extra_bytes                                # noqa: E402
from sasrec_probe import stats                                             # noqa: E402


def timed_alternated(fns, warmup, repeats):
    """{name: ms stats}: every repeat times each fn once, in turn, with a HIP event pair of its own"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/seq_attn_tiled_probe.json")
    ap.add_argument("--repeats", type=int, default=30)
    args = ap.parse_args()
    assert args.repeats >= 5
    ops.require_gpu()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    from selfrec_amd.data.sequence import Sequence
    from selfrec_amd.model.sequential.SASRec import SASRec_Model, StagedBatch, torch_causal_attention
    from selfrec_amd.util.loss_torch import l2_reg_loss
    from selfrec_amd.util.sampler import next_batch_sequence
    B, d, H, p = 256, 64, 1, 0.2
    res = {"shape": {"B": B, "heads": H, "dh": d, "drop_rate": p}, "warmup": 5, "repeats": args.repeats, "core": {}}

    g = torch.Generator().manual_seed(0)
    for L in (100, 200, 512):
        q, k, v, go = (torch.randn(B, L, d, generator=g).to(dev) for _ in range(4))
        for flavour in ("causal", "full"):
            causal = flavour == "causal"

            def attn(route):
                qa, ka, va = (t.detach().requires_grad_(True) for t in (q, k, v))
                if route == "tiled":
                    out = ops.SeqAttnTiledFn.apply(qa, ka, va, H, causal, None, p, 1234, 0)
                else:
                    out = torch_causal_attention(qa, ka, va, H, None, p, True, causal=causal)
                out.backward(go)
            fns = {r: (lambda r=r: attn(r)) for r in ("tiled", "torch")}
            rec = {"fwd_bwd_ms": timed_alternated(fns, 5, args.repeats),
                   "peak_extra_bytes": {r: peak_extra_bytes(fn) for r, fn in fns.items()},
                   "scores_bytes": 4 * B * H * L * L}
            rec["tiled_over_torch"] = rec["fwd_bwd_ms"]["tiled"]["median"] / rec["fwd_bwd_ms"]["torch"]["median"]
            res["core"][f"L{L}_{flavour}"] = rec
            print(f"L{L}_{flavour}", json.dumps(rec), flush=True)
        del q, k, v, go
    res["default_rule"] = {"holds": all(res["core"][f"L{L}_{f}"]["tiled_over_torch"] <= 1.0
                                        for L in (100, 200) for f in ("causal", "full")),
                           "rule": "tiled median <= torch median at L = 100 and L = 200, causal and full"}

    # one SASRec step at max.len 200 on ml1m-seq
    L = 200
    train, test = synth.make_sequence_dataset("ml1m-seq")
    data = Sequence({}, train, test)
    random.seed(0)
    seq, pos, y, neg, _seq_len = next(iter(next_batch_sequence(data, B, max_len=L)))
    steps = {}
    for route in ("hip", "torch"):
        torch.manual_seed(0)
        net = SASRec_Model(types.SimpleNamespace(item_num=data.item_num), d, L, 2, H, p, attention="tiled" if route == "hip" else route).cuda()
        net.train()
        opt = torch.optim.Adam(net.parameters(), lr=1e-3)
        pre = StagedBatch(seq, pos, y, neg, dev)
        assert net.attention_kernel(L) == ("tiled" if route == "hip" else None)

        def step(net=net, opt=opt, pre=pre):
            hid = net(seq, pos, staged=pre)
            total = ops.SeqBceFn.apply(hid.reshape(-1, d), net.item_emb, pre.y, pre.neg, pre.valid, pre.n_valid,
                                       pre.plans[2]) + l2_reg_loss(1e-4, net.item_emb)
            opt.zero_grad()
            total.backward()
            opt.step()
        steps[route] = step
    step_ms = timed_alternated(steps, 5, args.repeats)
    res["sasrec_step_ml1m_seq_L200"] = {"items": int(data.item_num), "sequences": int(data.raw_seq_num),
                                        "live_positions": float(np.mean(np.asarray(seq) != 0)), "prestaged_events_ms": step_ms,
                                        "peak_extra_bytes": {r: peak_extra_bytes(fn) for r, fn in steps.items()},
                                        "hip_over_torch": step_ms["hip"]["median"] / step_ms["torch"]["median"]}
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
