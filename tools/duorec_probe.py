#!/usr/bin/env python3
"""A/B of DuoRec's contrastive section and step (method of 4.27): one MI355X, the routes ``hip`` and ``pair``
alternated in one process, 5 warm-up rounds, 30 repeats, HIP events, median [min, max], peak memory above the inputs.  A
route counts as faster only when its whole range lies below its partner's.

  section   three last-row reads + both info_nce terms, forward + backward, on a (3B L, d) hidden matrix of LayerNormed
            rows (the workload's regime): B = 256 and B = 2048, L = 50, d = 64
  step      one whole training step of the model on beauty-seq at batch.size 256, each route (wall clock, synchronised)
  host      the positive draws and the staging of a step (wall clock)

Writes profiles/duorec_probe.json and prints it.   python tools/duorec_probe.py [--skip-step]"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from selfrec_amd import ops, synth  # noqa: E402
from selfrec_amd.util.loss_torch import info_nce  # noqa: E402

WARMUP, REPEATS = 5, 30
DEV = "cuda:0"


def stats(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs))


def faster(a, b):
    return a["max"] < b["min"]


def section_ab(B, L, d, cl_rate=0.01):
    gen = torch.Generator().manual_seed(B)
    x = torch.nn.functional.layer_norm(torch.randn(3 * B * L, d, generator=gen), (d,)).to(DEV).requires_grad_(True)
    lens = torch.randint(1, L + 1, (3 * B,), generator=gen)
    idx_host = (torch.arange(3 * B) * L + lens - 1).reshape(3, B).numpy()
    idx = torch.from_numpy(idx_host).to(torch.int32).to(DEV)

    def hip():
        loss = ops.DuoNceFn.apply(1.0, cl_rate, cl_rate, idx, idx_host, x).sum()
        loss.backward()

    def pair():
        a, p, q = (x[idx[k].long()] for k in range(3))
        loss = cl_rate * (info_nce(a, p, 1.0, B) + info_nce(a, q, 1.0, B))
        loss.backward()

    routes = dict(hip=hip, pair=pair)
    times = {k: [] for k in routes}
    peak = {}
    for rnd in range(WARMUP + REPEATS):
        for name, fn in routes.items():
            x.grad = None
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            torch.cuda.synchronize()
            if rnd >= WARMUP:
                times[name].append(t0.elapsed_time(t1))
                peak[name] = max(peak.get(name, 0), torch.cuda.max_memory_allocated() - base)
    out = {k: dict(stats(v), peak_bytes=int(peak[k])) for k, v in times.items()}
    out["hip_faster"] = faster(out["hip"], out["pair"])
    return out


def step_ab(tmp):
    from selfrec_amd.data.loader import FileIO
    from selfrec_amd.model.sequential.CL4SRec import StagedViews
    from selfrec_amd.model.sequential.DuoRec import DuoRec
    from selfrec_amd.util.conf import ModelConf
    from selfrec_amd.util.sampler import next_batch_sequence_indexed, same_target_positives
    train, test = synth.make_sequence_dataset("beauty-seq")
    synth.write_sequences(os.path.join(tmp, "train.txt"), train)
    synth.write_sequences(os.path.join(tmp, "test.txt"), test)
    conf = ModelConf(os.path.join(ROOT, "conf", "DuoRec.yaml"))
    conf.config["training.set"], conf.config["test.set"] = os.path.join(tmp, "train.txt"), os.path.join(tmp, "test.txt")
    random.seed(1); torch.manual_seed(1)
    model = DuoRec(conf, FileIO.load_data_set(conf["training.set"], "sequential"),
                   FileIO.load_data_set(conf["test.set"], "sequential"))
    net = model.model.to(DEV)
    net.train()
    adam = torch.optim.Adam(net.parameters(), lr=model.lRate)
    batches = next_batch_sequence_indexed(model.data, model.batch_size, max_len=model.max_len)
    times, host = {"hip": [], "pair": []}, {"draws": [], "staging": []}
    for rnd in range(WARMUP + REPEATS):
        seq, pos, y, neg, seq_len, rows = next(batches)
        t0 = time.perf_counter()
        positives = same_target_positives(model.data, rows, model.max_len)[:3]
        t1 = time.perf_counter()
        StagedViews([(seq, pos, None), (seq, pos, seq_len), positives], y, neg, DEV, "one", "hip", anchor_last=seq_len)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        for duo in ("hip", "pair"):
            model.duo = duo
            torch.cuda.synchronize()
            s0 = time.perf_counter()
            loss, _, _ = model.step_losses(seq, pos, y, neg, seq_len, positives)
            adam.zero_grad()
            loss.backward()
            adam.step()
            torch.cuda.synchronize()
            if rnd >= WARMUP:
                times[duo].append((time.perf_counter() - s0) * 1e3)
        if rnd >= WARMUP:
            host["draws"].append((t1 - t0) * 1e3)
            host["staging"].append((t2 - t1) * 1e3)
    out = {k: stats(v) for k, v in times.items()}
    out["hip_faster"] = faster(out["hip"], out["pair"])
    return out, {k: stats(v) for k, v in host.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "duorec_probe.json"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    result = dict(device=torch.cuda.get_device_name(0), warmup=WARMUP, repeats=REPEATS, unit="ms",
                  section={f"B{B}": section_ab(B, 50, 64) for B in (256, 2048)})
    if not args.skip_step:
        import tempfile
        with tempfile.TemporaryDirectory() as tmp:
            result["step_B256"], result["host_B256"] = step_ab(tmp)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
