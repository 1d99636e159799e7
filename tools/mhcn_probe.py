"""MHCN at the shape of conf/MHCN.yaml on the douban-book synthetic graph with generated trust pairs (B = 2048, d = 64,
n_layer 2; n = the users of the graph), timed with HIP events around each repeat (warm-up first; median, min and max).
Every figure has torch's expression on the same GPU as its partner, and the two ALTERNATE inside one run -- hip, torch,
hip, torch ... -- so that a drift of the machine lands on both:
  * the four gates of the user table forward + backward: ops.GateFn (csrc/mhcn.hip) and x * sigmoid(x @ W + b) four times
    (the ``engine.gate: torch`` route), and the peak memory each allocates above its inputs;
  * the channel attention forward + backward: ops.ChanMixFn and the reference's expression (``engine.mix: torch``);
  * the MIM loss of one channel forward + backward, edge given: ops.MimFn and the reference's gathers and reductions
    (``engine.mim: torch``);
  * one whole step (forward, the three MIM losses, BPR, regulariser, backward, torch Adam) by the defaults and with each
    route, and all three, on torch: wall time between fences.

    python tools/mhcn_probe.py [--out profiles/mhcn_probe.json] [--repeats 20]
"""
import argparse
import json
import os
import random
import sys

import torch

sys.path.insert(0, ".")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from selfrec_amd import ops, synth                                         # noqa: E402
from bert4rec_probe import peak_extra_bytes                                # noqa: E402
from sept_probe import alternating                                         # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/mhcn_probe.json")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--shape", default="douban-book", choices=sorted(synth.SHAPES))
    args = ap.parse_args()
    assert args.repeats >= 5
    ops.require_gpu()
    torch.cuda.set_device(0)
    from selfrec_amd.model.graph import MHCN as M
    from selfrec_amd.util.conf import ModelConf
    from selfrec_amd.util.sampler import next_batch_pairwise
    B, d, L = 2048, 64, 2
    tu, ti, su, si, _, _ = synth.make_dataset(args.shape)
    social = synth.make_social(args.shape)

    def make(gate, mix, mim):
        conf = ModelConf({"training.set": "./none", "test.set": "./none", "model": {"name": "MHCN", "type": "graph"},
                          "item.ranking.topN": [10, 20], "embedding.size": d, "max.epoch": 30, "batch.size": B,
                          "learning.rate": 0.001, "reg.lambda": 0.0001, "output": "./results/",
                          "MHCN": {"n_layer": L, "ss_rate": 0.01},
                          "engine.gate": gate, "engine.mix": mix, "engine.mim": mim})
        torch.manual_seed(0)
        random.seed(0)
        m = M.MHCN(conf, synth.as_triples(tu, ti), synth.as_triples(su, si), **{"social.data": [list(p) for p in social]})
        m.model.cuda()
        return m

    routes = {"hip": ("hip", "hip", "hip"), "gate_torch": ("torch", "hip", "hip"), "mix_torch": ("hip", "torch", "hip"),
              "mim_torch": ("hip", "hip", "torch"), "torch": ("torch", "torch", "torch")}
    models = {name: make(*r) for name, r in routes.items()}
    base = models["hip"]
    enc = base.model
    n = base.data.user_num
    random.seed(1)
    batch = next(iter(next_batch_pairwise(base.data, B, as_arrays=True)))
    idx = [torch.from_numpy(a).cuda() for a in batch]
    res = {"shape": {"dataset": args.shape, "users": n, "items": base.data.item_num, "B": B, "d": d, "n_layer": L,
                     "trust_pairs": base.social_data.size()[1], "H_nnz": [int(h.csr.nnz) for h in enc.H]}}
    g = torch.Generator().manual_seed(0)
    rand = lambda *shape: torch.randn(*shape, generator=g).cuda()  # noqa: E731

    # ---- the four gates of the user table ---------------------------------------------------------------------------------
    x0 = enc.user_embeddings.detach()
    w0 = torch.stack([enc.weights[f"gating{i}"].detach() for i in range(1, 5)])
    b0 = torch.cat([enc.weights[f"gating_bias{i}"].detach() for i in range(1, 5)])
    gy = rand(4, n, d)

    def gates(route):
        x, w, b = (t.clone().requires_grad_(True) for t in (x0, w0, b0))
        y = ops.GateFn.apply(x, w, b) if route == "hip" else torch.stack([M.gate_torch(x, w[c], b[c:c + 1]) for c in range(4)])
        y.backward(gy)
    res["gate4_fwd_bwd_ms"] = alternating({r: (lambda r=r: gates(r)) for r in ("hip", "torch")}, 5, args.repeats)
    res["gate4_peak_extra_bytes"] = {r: peak_extra_bytes(lambda r=r: gates(r)) for r in ("hip", "torch")}

    # ---- channel attention --------------------------------------------------------------------------------------------------
    with torch.no_grad():
        chans = [c.contiguous() for c in enc.gates(x0, 'gating', 4)]
    att, mat, go = enc.weights['attention'].detach(), enc.weights['attention_mat'].detach(), rand(n, d)

    def mix(route):
        e = [c.clone().requires_grad_(True) for c in chans]
        a, m_ = att.clone().requires_grad_(True), mat.clone().requires_grad_(True)
        if route == "hip":
            out, _ = ops.ChanMixFn.apply(e[0], e[1], e[2], (m_ @ a.T).reshape(-1), e[3], 0.5)
        else:
            out = M.chan_mix_torch(e[:3], a, m_)[0] + e[3] / 2
        out.backward(go)
    res["chan_mix_fwd_bwd_ms"] = alternating({r: (lambda r=r: mix(r)) for r in ("hip", "torch")}, 5, args.repeats)
    res["chan_mix_peak_extra_bytes"] = {r: peak_extra_bytes(lambda r=r: mix(r)) for r in ("hip", "torch")}

    # ---- the MIM loss of one channel, edge given ----------------------------------------------------------------------------
    with torch.no_grad():
        em0 = chans[0]
        edge0 = torch.sparse.mm(enc.H[0], em0).contiguous()
    perms = base.perms(0, n, d, em0.device)

    def mim(route):
        em, edge = em0.clone().requires_grad_(True), edge0.clone().requires_grad_(True)
        loss = ops.MimFn.apply(em, edge, *perms) if route == "hip" else M.mim_torch(em, edge, perms)
        loss.backward()
    res["mim_fwd_bwd_ms"] = alternating({r: (lambda r=r: mim(r)) for r in ("hip", "torch")}, 5, args.repeats)
    res["mim_peak_extra_bytes"] = {r: peak_extra_bytes(lambda r=r: mim(r)) for r in ("hip", "torch")}

    # ---- the whole step -----------------------------------------------------------------------------------------------------
    steps = {}
    for name, m in models.items():
        opt = torch.optim.Adam(m.model.parameters(), lr=1e-3)

        def step(m=m, opt=opt):
            loss = m.batch_losses(*idx)[3]
            opt.zero_grad()
            loss.backward()
            opt.step()
        steps[name] = step
    res["step_wall_ms"] = alternating(steps, 5, args.repeats, wall=True)
    res["step_peak_extra_bytes"] = {name: peak_extra_bytes(fn) for name, fn in steps.items()}
    med = lambda key, r: res[key][r]["median"]  # noqa: E731
    res["hip_over_torch"] = {"gate4": med("gate4_fwd_bwd_ms", "hip") / med("gate4_fwd_bwd_ms", "torch"),
                             "chan_mix": med("chan_mix_fwd_bwd_ms", "hip") / med("chan_mix_fwd_bwd_ms", "torch"),
                             "mim": med("mim_fwd_bwd_ms", "hip") / med("mim_fwd_bwd_ms", "torch"),
                             "step": med("step_wall_ms", "hip") / med("step_wall_ms", "torch")}
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
