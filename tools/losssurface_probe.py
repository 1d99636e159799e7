"""The four new entries of util/loss_torch.py by the kernels and by the reference's torch expression on
the same GPU, forward + backward between two HIP events.  The two routes ALTERNATE inside one process -- hip, torch, hip,
torch ... -- so that a drift of the machine lands on both; 5 warm-up rounds, then --repeats (30) timed ones: median [min,
max], and the peak memory each route allocates above its inputs (the leaves exist before the measured call; their .grad,
an output, is inside it).  A route is "faster" only when its whole range lies below its partner's; overlapping ranges are
"NOT faster".  A probe, not a gate: every figure is written as it falls.

    info_nce               B = 256 and 2048, d = 64, temp 0.2, 'dot'
    InfoNCE(b_cos=False)   n = 2048, d = 64, temperature 0.2
    kl_divergence          2048 x 1000
    triplet_loss           B = 2048, d = 64

    python tools/losssurface_probe.py [--out profiles/losssurface_probe.json] [--repeats 30]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, ".")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from selfrec_amd import ops                                                # noqa: E402
from selfrec_amd.util import loss_torch as L                               # noqa: E402
from sept_probe import alternating                                         # noqa: E402
from bert4rec_probe import peak_extra_bytes                                # noqa: E402


def _pair(hip, torch_expr, inputs, repeats):
    """one function on both routes: the same leaves every call (made here, outside every measured span; .grad dropped at
    the end of a call), loss.backward() inside the timed span"""
    leaves = [t.detach().clone().requires_grad_(True) for t in inputs]

    def run(fn):
        loss = fn(*leaves)
        loss.backward()
        loss = loss.detach()
        for t in leaves:          # (dropped before the call returns: the next call's baseline holds the leaves only)
            t.grad = None
        return loss
    routes = {"hip": lambda: run(hip), "torch": lambda: run(torch_expr)}
    values = {r: float(fn()) for r, fn in routes.items()}
    ms = alternating(routes, 5, repeats)
    peak = {r: peak_extra_bytes(fn) for r, fn in routes.items()}
    if ms["hip"]["max"] < ms["torch"]["min"]:
        verdict = "faster"
    elif ms["torch"]["max"] < ms["hip"]["min"]:
        verdict = "NOT faster: slower"
    else:
        verdict = "NOT faster: the ranges overlap"
    return {"loss_value": values, "fwd_bwd_ms": ms, "peak_extra_bytes": peak, "input_bytes": sum(t.numel() * 4 for t in inputs),
            "verdict": verdict}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/losssurface_probe.json")
    ap.add_argument("--repeats", type=int, default=30)
    args = ap.parse_args()
    ops.require_gpu()
    torch.cuda.set_device(0)
    g = torch.Generator().manual_seed(0)

    def rows(n, d, s=0.3):
        return (s * torch.randn(n, d, generator=g)).cuda()
    res = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "warmup": 5}
    for B in (256, 2048):
        res[f"info_nce_B{B}_d64"] = _pair(lambda a, b, B=B: L.info_nce(a, b, 0.2, B), lambda a, b, B=B: L._info_nce_expression(a, b, 0.2, B),
                                          (rows(B, 64), rows(B, 64)), args.repeats)
    res["InfoNCE_raw_n2048_d64"] = _pair(lambda a, b: L.InfoNCE(a, b, 0.2, b_cos=False),
                                         lambda a, b: L._infonce_expression(a, b, 0.2, False), (rows(2048, 64), rows(2048, 64)),
                                         args.repeats)
    res["kl_divergence_2048x1000"] = _pair(L.kl_divergence, L._kl_expression, (rows(2048, 1000, 1.0), rows(2048, 1000, 2.0)),
                                           args.repeats)
    res["triplet_loss_B2048_d64"] = _pair(L.triplet_loss, L._triplet_expression, (rows(2048, 64), rows(2048, 64), rows(2048, 64)),
                                          args.repeats)
    for name, r in res.items():
        if isinstance(r, dict):
            ms, pk = r["fwd_bwd_ms"], r["peak_extra_bytes"]
            print(f"{name}: hip {ms['hip']['median']:.3f} ms [{ms['hip']['min']:.3f}, {ms['hip']['max']:.3f}], torch "
                  f"{ms['torch']['median']:.3f} ms [{ms['torch']['min']:.3f}, {ms['torch']['max']:.3f}] -> {r['verdict']}; peak "
                  f"{pk['hip'] / 1e6:.2f} MB against {pk['torch'] / 1e6:.2f} MB; loss {r['loss_value']}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
