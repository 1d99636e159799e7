"""NCL at the Yelp2018 shape (31,668 users x 38,048 items, d = 64, B = 2048, tau = 0.05), timed between device
fences:
  * the table InfoNCE op (ops.table_nce_fwd_bwd: both sides, forward + backward) against the torch expression of
    reference model/graph/NCL.py:59-82 on the same GPU (fp32, autograd), each as a fraction of the f32 MFMA bound of
    its four B x N x d products per side (2 * 4 * B * (N_u + N_i) * d FLOP at 155 TFLOP/s, MI355X_MICROARCH.md);
  * one NCL training step (prototype phase: rec + l2 + ssl + proto, backward, Adam) in ms and pairs/s;
  * one e_step (two k-means runs, k = 2000) in ms.

    python tools/ncl_probe.py [--out profiles/ncl_probe.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from selfrec_amd import ops, synth                                         # noqa: E402
from selfrec_amd.data.loader import FileIO                                 # noqa: E402
from selfrec_amd.util.conf import ModelConf                                # noqa: E402

F32_MFMA_TFLOPS = 155.0          # measured f32 MFMA rate (MI355X_MICROARCH.md, Matrix cores)


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
    return 1e3 * float(np.median(ts)), 1e3 * float(np.min(ts))


def torch_ssl(q_u, t_u, u, q_i, t_i, i, tau, ssl_reg, alpha):
    """NCL.py:59-82 (the reference's expression, the batch rows gathered already)"""
    import torch.nn.functional as F
    out = []
    for q, t, idx in ((q_u, t_u, u), (q_i, t_i, i)):
        n1, n2, na = F.normalize(q), F.normalize(t[idx]), F.normalize(t)
        pos = torch.exp(torch.mul(n1, n2).sum(dim=1) / tau)
        ttl = torch.exp(torch.matmul(n1, na.transpose(0, 1)) / tau).sum(dim=1)
        out.append(-torch.log(pos / ttl).sum())
    return ssl_reg * (out[0] + alpha * out[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/ncl_probe.json")
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    ops.require_gpu()
    torch.cuda.set_device(0)
    U, I, d, B, tau = 31668, 38048, 64, 2048, 0.05
    g = torch.Generator().manual_seed(0)
    t_u, t_i = (torch.randn(U, d, generator=g) * 0.1).cuda(), (torch.randn(I, d, generator=g) * 0.1).cuda()
    u, i = torch.randint(0, U, (B,), generator=g).cuda(), torch.randint(0, I, (B,), generator=g).cuda()
    q_u, q_i = (torch.randn(B, d, generator=g) * 0.1).cuda(), (torch.randn(B, d, generator=g) * 0.1).cuda()
    flop = 2 * 4 * B * (U + I) * d
    bound_ms = flop / (F32_MFMA_TFLOPS * 1e12) * 1e3
    ws = ops.table_nce_ws([(B, U), (B, I)], d, t_u.device)
    res = {"shape": {"users": U, "items": I, "d": d, "batch": B, "tau": tau}, "gflop": flop / 1e9, "f32_mfma_bound_ms": bound_ms}

    def op():
        ops.table_nce_fwd_bwd([(q_u, t_u, u, 1e-6), (q_i, t_i, i, 1.5e-6)], tau=tau, ws=ws)
    med, best = timed(op, 3, 20)
    res["table_op_ms"] = {"median": med, "min": best, "fraction_of_bound": bound_ms / med}

    leaves = [x.clone().requires_grad_(True) for x in (q_u, t_u, q_i, t_i)]

    def ref():
        for x in leaves:
            x.grad = None
        torch_ssl(leaves[0], leaves[1], u, leaves[2], leaves[3], i, tau, 1e-6, 1.5).backward()
    try:
        med, best = timed(ref, 2, 10)
        res["torch_expression_ms"] = {"median": med, "min": best, "fraction_of_bound": bound_ms / med}
        res["speedup"] = res["torch_expression_ms"]["median"] / res["table_op_ms"]["median"]
    except torch.OutOfMemoryError as e:  # pragma: no cover
        res["torch_expression_ms"] = f"out of memory: {e}"
    print(json.dumps(res, indent=1), flush=True)

    # the model at the same shape: one e_step, then steps of the prototype phase
    conf = ModelConf("./conf/NCL.yaml")
    if not os.path.exists(conf["training.set"]):
        tu, ti, su, si, _, _ = synth.make_dataset("yelp2018")
        os.makedirs(os.path.dirname(conf["training.set"]) or ".", exist_ok=True)
        synth.write_text(conf["training.set"], tu, ti)
        synth.write_text(conf["test.set"], su, si)
    from selfrec_amd.model.graph.NCL import NCL
    from selfrec_amd.util.sampler import next_batch_pairwise
    rec = NCL(conf, FileIO.load_data_set(conf["training.set"], "graph"), FileIO.load_data_set(conf["test.set"], "graph"))
    model = rec.model.cuda()
    med, best = timed(rec.e_step, 1, 3)
    res["e_step_ms"] = {"median": med, "min": best, "k": rec.k}
    opt = torch.optim.Adam(model.parameters(), lr=rec.lRate)
    batches = []
    for n, b in enumerate(next_batch_pairwise(rec.data, rec.batch_size, as_arrays=True)):
        if n == args.steps + 3:
            break
        batches.append(tuple(torch.from_numpy(a).cuda() for a in b))
    it = iter(batches)

    def step():
        _, _, _, loss = rec.batch_losses(*next(it), True)
        opt.zero_grad()
        loss.backward()
        opt.step()
    med, best = timed(step, 3, args.steps)
    res["ncl_step_ms"] = {"median": med, "min": best, "pairs_per_s": B / (med * 1e-3)}
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
