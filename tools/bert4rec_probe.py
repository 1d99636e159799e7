"""BERT4Rec at the shape of conf/BERT4Rec.yaml on the beauty-seq synthetic set (B = 256, L = 50, d = 64, 2 blocks, 1 head,
mask_rate 0.5; the item table has item_num + 2 rows), timed with HIP events around each repeat (warm-up first; median, min
and max over the repeats).  The partner of every figure is torch's expression on the same GPU in the same run:
  * the attention core forward + backward: ops.SeqAttnFullFn (csrc/seqrec.hip, causal flag off) and torch's expression on
    the same projected inputs (the ``engine.attention: torch`` route), with dropout 0.2 on the probabilities;
  * the loss with its gradients: ops.TableCeFn (csrc/contrastive.hip) and F.cross_entropy on materialised logits
    (the ``engine.ce: torch`` route), and the peak memory each allocates above the inputs;
  * one full training step by each pair of routes (forward, loss, backward, torch Adam): wall time between fences with the
    batch's staging (scatter plans + upload) included, the same step on a pre-staged batch, and the staging alone.
M, the number of masked positions, is whatever the mask stream yields for the first batch; it is recorded.

    python tools/bert4rec_probe.py [--out profiles/bert4rec_probe.json] [--repeats 20]
"""
import argparse
import json
import os
import random
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, ".")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from selfrec_amd import ops, synth                                         # noqa: E402
from sasrec_probe import timed_events, timed_wall                          # noqa: E402


def peak_extra_bytes(fn):
    """the most memory fn holds above what is allocated when it starts"""
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/bert4rec_probe.json")
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args()
    assert args.repeats >= 5
    ops.require_gpu()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    from selfrec_amd.data.sequence import Sequence
    from selfrec_amd.model.sequential.BERT4Rec import BERT_Encoder, StagedMaskedBatch, item_mask_for_bert
    from selfrec_amd.model.sequential.SASRec import torch_causal_attention
    from selfrec_amd.util.loss_torch import l2_reg_loss
    from selfrec_amd.util.sampler import next_batch_sequence
    B, L, d, H, p, rate = 256, 50, 64, 1, 0.2, 0.5
    train, test = synth.make_sequence_dataset("beauty-seq")
    data = Sequence({}, train, test)
    random.seed(0)
    seq, pos, _y, _neg, seq_len = next(iter(next_batch_sequence(data, B, max_len=L)))
    aug, masked, labels = item_mask_for_bert(seq, seq_len, rate, data.item_num + 1)
    M, N = int(labels.shape[0]), data.item_num + 2
    res = {"shape": {"B": B, "L": L, "d": d, "heads": H, "blocks": 2, "table_rows": N, "masked_rows_M": M, "drop_rate": p,
                     "mask_rate": rate}}

    g = torch.Generator().manual_seed(0)
    q, k, v, go = (torch.randn(B, L, d, generator=g).to(dev) for _ in range(4))

    def attn(route):
        qa, ka, va = (t.detach().requires_grad_(True) for t in (q, k, v))
        if route == "hip":
            out = ops.SeqAttnFullFn.apply(qa, ka, va, H, None, p, 1234, 0)
        else:
            out = torch_causal_attention(qa, ka, va, H, None, p, True, causal=False)
        out.backward(go)
    res["attention_fwd_bwd_ms"] = {r: timed_events(lambda r=r: attn(r), 5, args.repeats) for r in ("hip", "torch")}

    table = (0.1 * torch.randn(N, d, generator=g)).to(dev)
    rows = torch.randn(M, d, generator=g).to(dev)
    lab32 = torch.from_numpy(np.asarray(labels, dtype=np.int32)).to(dev)
    lab64 = lab32.long()

    def loss(route):
        h, t = rows.detach().requires_grad_(True), table.detach().requires_grad_(True)
        if route == "hip":
            out = ops.TableCeFn.apply(h, t, lab32, 1.0 / (M * M))
        else:
            out = F.cross_entropy(torch.mm(h, t.t()), lab64) / M
        out.backward()
    res["ce_fwd_bwd_ms"] = {r: timed_events(lambda r=r: loss(r), 5, args.repeats) for r in ("hip", "torch")}
    res["ce_peak_extra_bytes"] = {r: peak_extra_bytes(lambda r=r: loss(r)) for r in ("hip", "torch")}
    res["ce_logits_bytes"] = 4 * M * N

    def stage():
        return StagedMaskedBatch(aug, pos, masked, labels, dev)
    res["stage_batch_host_ms"] = timed_wall(stage, 5, args.repeats)

    step_ms = {}
    for route in ("hip", "torch"):
        torch.manual_seed(0)
        net = BERT_Encoder(types.SimpleNamespace(item_num=data.item_num), d, L, 2, H, p, attention=route).cuda()
        net.train()
        opt = torch.optim.Adam(net.parameters(), lr=1e-3)
        pre = stage()

        def step(staged=None):
            b = stage() if staged is None else staged
            hid = net(aug, pos, staged=b).reshape(-1, d)[b.masked_idx.long()]
            if route == "hip":
                ce = ops.TableCeFn.apply(hid, net.item_emb, b.labels, 1.0 / (M * M))
            else:
                ce = F.cross_entropy(torch.mm(hid, net.item_emb.t()), b.labels.long()) / M
            total = ce + l2_reg_loss(1e-4, net.item_emb)
            opt.zero_grad()
            total.backward()
            opt.step()
        step_ms[route] = {"wall": timed_wall(step, 5, args.repeats),
                          "prestaged_wall": timed_wall(lambda: step(pre), 5, args.repeats),
                          "prestaged_events": timed_events(lambda: step(pre), 2, args.repeats)}
    res["step_ms"] = step_ms
    res["step_hip_over_torch"] = step_ms["hip"]["wall"]["median"] / step_ms["torch"]["wall"]["median"]
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
