"""SSL4Rec at the Yelp2018 shape (31,668 users x 38,048 items, d = 64, B = 2048, tau = 0.07), timed between device
fences (median and min over the iterations):
  * tower fwd + bwd: the user tower over B rows and the item tower over 3B rows (plain + two dropout views), forward and
    backward with the table scatter -- 3 x (B + 3B) x 196,608 MACs x 2 FLOP;
  * batch softmax (ops.batch_softmax_fwd_bwd, d = 128): its four B x B x 128 products;
  * one full step (towers, batch softmax, InfoNCE, L2, backward, torch Adam over both tables and the 8 tower tensors);
    the Adam step alone, and srh_adam_step over the same tensors for comparison;
  * the per-epoch evaluation: both full-table tower passes plus test()'s ranking;
  * the same step as the reference's torch expression (SSL4Rec.py:31-37, nn.Sequential towers, autograd) on the same GPU.
The floor is the f32 MFMA rate (155 TFLOP/s, MI355X_MICROARCH.md) over the step's tower and loss FLOP.

    python tools/ssl4rec_probe.py [--out profiles/ssl4rec_probe.json]
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, ".")
from selfrec_amd import ops, synth                                         # noqa: E402
from selfrec_amd.data.loader import FileIO                                 # noqa: E402
from selfrec_amd.util.conf import ModelConf                                # noqa: E402

F32_MFMA_TFLOPS = 155.0
MACS_PER_ROW = 64 * 1024 + 1024 * 128


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return {"median": 1e3 * float(np.median(ts)), "min": 1e3 * float(np.min(ts))}


def bound_ms(flop):
    return flop / (F32_MFMA_TFLOPS * 1e12) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/ssl4rec_probe.json")
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    ops.require_gpu()
    torch.cuda.set_device(0)
    from selfrec_amd.model.graph.SSL4Rec import DNN_Encoder
    from selfrec_amd.util.loss_torch import InfoNCE, batch_softmax_loss, l2_reg_loss
    U, I, d, B, tau, alpha, reg = 31668, 38048, 64, 2048, 0.07, 0.1, 1e-4
    tower_flop = 3 * 4 * B * MACS_PER_ROW * 2
    bs_flop = 4 * 2 * B * B * 128
    nce_flop = 4 * 2 * B * B * 128
    res = {"shape": {"users": U, "items": I, "d": d, "batch": B, "tau": tau},
           "gflop": {"towers": tower_flop / 1e9, "batch_softmax": bs_flop / 1e9, "infonce": nce_flop / 1e9},
           "f32_mfma_bound_ms": {"towers": bound_ms(tower_flop), "batch_softmax": bound_ms(bs_flop),
                                 "step": bound_ms(tower_flop + bs_flop + nce_flop)}}
    torch.manual_seed(0)
    enc = DNN_Encoder(types.SimpleNamespace(user_num=U, item_num=I), d, 0.1, tau).cuda()
    rs = np.random.RandomState(0)
    batches = [(rs.randint(0, U, B), rs.randint(0, I, B)) for _ in range(args.steps + 5)]
    it = {"k": 0}

    def next_batch():
        b = batches[it["k"] % len(batches)]
        it["k"] += 1
        return b

    def towers():
        q, x = next_batch()
        qe, ie, (v1, v2) = enc.encode_batch(q, x)
        torch.autograd.backward([qe, ie, v1, v2], [torch.ones_like(qe), torch.ones_like(ie), torch.ones_like(v1),
                                                   torch.ones_like(v2)])
    r = timed(towers, 3, args.steps)
    r["fraction_of_bound"] = res["f32_mfma_bound_ms"]["towers"] / r["median"]
    res["tower_fwd_bwd_ms"] = r

    g = torch.Generator().manual_seed(1)
    u, v = (torch.randn(B, 128, generator=g) * 0.1).cuda(), (torch.randn(B, 128, generator=g) * 0.1).cuda()
    ws = torch.empty(int(ops._lib.load().srh_batch_softmax_ws_bytes(B, 128)), dtype=torch.uint8, device=u.device)
    r = timed(lambda: ops.batch_softmax_fwd_bwd(u, v, tau, ws=ws), 3, args.steps)
    r["fraction_of_bound"] = res["f32_mfma_bound_ms"]["batch_softmax"] / r["median"]
    res["batch_softmax_ms"] = r

    opt = torch.optim.Adam(enc.parameters(), lr=1e-3)

    def losses(q, x):
        qe, ie, (v1, v2) = enc.encode_batch(q, x)
        return batch_softmax_loss(qe, ie, tau) + l2_reg_loss(reg, qe, ie) + alpha * InfoNCE(v1, v2, tau)

    def step():
        loss = losses(*next_batch())
        opt.zero_grad()
        loss.backward()
        opt.step()
    r = timed(step, 3, args.steps)
    r["fraction_of_bound"] = res["f32_mfma_bound_ms"]["step"] / r["median"]
    r["pairs_per_s"] = B / (r["median"] * 1e-3)
    res["step_ms"] = r
    res["torch_adam_ms"] = timed(opt.step, 3, args.steps)
    params = [p for p in enc.parameters()]
    state = [(p.detach().clone(), torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)) for p in params]

    def hip_adam():
        for p, gr, m, vv in state:
            ops.adam_step(p.view(-1), gr.view(-1), m.view(-1), vv.view(-1), step=1, lr=1e-3)
    try:
        res["srh_adam_step_ms"] = timed(hip_adam, 3, args.steps)
    except Exception as e:  # pragma: no cover
        res["srh_adam_step_ms"] = f"not measured: {e}"

    # the reference's torch expression of the same step (SSL4Rec.py:31-37)
    torch.manual_seed(0)
    ref = DNN_Encoder(types.SimpleNamespace(user_num=U, item_num=I), d, 0.1, tau).cuda()
    ropt = torch.optim.Adam(ref.parameters(), lr=1e-3)

    def ref_step():
        q, x = (torch.from_numpy(a).cuda() for a in next_batch())
        qe, ie = ref.user_tower(ref.initial_user_emb[q]), ref.item_tower(ref.initial_item_emb[x])
        un, vn = F.normalize(qe, dim=1), F.normalize(ie, dim=1)
        pos = torch.exp((un * vn).sum(dim=-1) / tau)
        ttl = torch.exp(torch.matmul(un, vn.transpose(0, 1)) / tau).sum(dim=1)
        rec = torch.mean(-torch.log(pos / ttl + 10e-6))
        e = ref.initial_item_emb[x]
        v1, v2 = ref.item_tower(ref.dropout(e)), ref.item_tower(ref.dropout(e))
        v1, v2 = F.normalize(v1, dim=1), F.normalize(v2, dim=1)
        cl = -torch.diag(F.log_softmax(v1 @ v2.T / tau, dim=1)).mean()
        l2 = reg * (torch.norm(qe, p=2) / B + torch.norm(ie, p=2) / B)
        loss = rec + l2 + alpha * cl
        ropt.zero_grad()
        loss.backward()
        ropt.step()
    ref.train()
    r = timed(ref_step, 3, args.steps)
    res["torch_expression_step_ms"] = r
    res["speedup_vs_torch"] = r["median"] / res["step_ms"]["median"]
    print(json.dumps(res, indent=1), flush=True)

    # the per-epoch evaluation on the model: two full-table tower passes + test()'s ranking
    conf = ModelConf("./conf/SSL4Rec.yaml")
    if not os.path.exists(conf["training.set"]):
        tu, ti, su, si, _, _ = synth.make_dataset("yelp2018")
        os.makedirs(os.path.dirname(conf["training.set"]) or ".", exist_ok=True)
        synth.write_text(conf["training.set"], tu, ti)
        synth.write_text(conf["test.set"], su, si)
    from selfrec_amd.model.graph.SSL4Rec import SSL4Rec
    rec = SSL4Rec(conf, FileIO.load_data_set(conf["training.set"], "graph"), FileIO.load_data_set(conf["test.set"], "graph"))
    rec.model.cuda().eval()

    def full_pass():
        with torch.no_grad():
            rec.query_emb, rec.item_emb = rec.model(None, None)
    r = timed(full_pass, 2, 10)
    eval_flop = (rec.data.user_num + rec.data.item_num) * MACS_PER_ROW * 2
    r["fraction_of_bound"] = bound_ms(eval_flop) / r["median"]
    res["eval_tower_passes_ms"] = r

    def evaluation():
        full_pass()
        rec.test()
    res["eval_epoch_ms"] = timed(evaluation, 1, 3)
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
