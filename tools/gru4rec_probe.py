#!/usr/bin/env python3
"""A/B of GRU4Rec's recurrence, item-table gradient and step (method of 4.27): one MI355X, the two routes
alternated in one process, 5 warm-up rounds, 30 repeats, HIP events, median [min, max], peak memory above the inputs.  A
route counts as faster only when its whole range lies below its partner's.

Measured on a real batch of each data set -- beauty-seq at the conf's shape (B = 256, L = 50, d = 64) and ml1m-seq at
max.len 200 -- with the live fraction of the B L positions and the workgroup count of the kernels noted.  ONE batch is
drawn per set (random.seed(0)) and reused by every round: the sampler's rejection draw of negatives costs minutes of host
time per batch at max.len 200, and the routes are compared on the same batch anyway.  --batches DIR keeps the drawn
batches as .npz files and reads them back on a later run.

  recurrence  one layer forward + backward: ops.GruFn against torch.nn.GRU(...)[0] * live
  gather      the item gather forward + backward: ops.GatherLiveRowsFn against ops.GatherRowsFn
  step        one whole training step of the model, engine.rnn hip against torch (wall clock between synchronised fences)

Writes profiles/gru4rec_probe.json and profiles/NOTES_gru4rec.md and prints the former.
    python tools/gru4rec_probe.py [--out FILE] [--notes FILE] [--batches DIR] [--draw-only]"""
import argparse
import json
import os
import random
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from selfrec_amd import ops, synth  # noqa: E402

WARMUP, REPEATS = 5, 30
DEV = "cuda:0"
SETS = (("beauty-seq", 50), ("ml1m-seq", 200))


def stats(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs))


def faster(a, b):
    return a["max"] < b["min"]


def alternate(routes, reset):
    """every route once per round, HIP events around it -> {route: stats + peak_bytes}"""
    times, peak = {k: [] for k in routes}, {}
    for rnd in range(WARMUP + REPEATS):
        for name, fn in routes.items():
            reset()
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
    return {k: dict(stats(v), peak_bytes=int(peak[k])) for k, v in times.items()}


def recurrence_ab(seq, d):
    B, L = seq.shape
    gen = torch.Generator().manual_seed(B + L)
    gru = torch.nn.GRU(d, d, num_layers=1, batch_first=True).to(DEV)
    params = [gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0]
    live = torch.from_numpy(seq != 0).to(DEV).unsqueeze(-1)
    lens = torch.from_numpy(np.count_nonzero(seq, axis=1).astype(np.int32)).to(DEV)
    x = (torch.randn(B, L, d, generator=gen).to(DEV) * live).requires_grad_(True)
    go = torch.randn(B, L, d, generator=gen).to(DEV)

    def hip():
        ops.GruFn.apply(x, *params, lens).backward(go)

    def torch_route():
        (gru(x)[0] * live).backward(go)

    def reset():
        x.grad = None
        for p in params:
            p.grad = None

    out = alternate(dict(hip=hip, torch=torch_route), reset)
    out["hip_faster"] = faster(out["hip"], out["torch"])
    return out


def gather_ab(seq, n_items, d):
    flat = seq.reshape(-1)
    table = torch.randn(n_items + 1, d, device=DEV, requires_grad=True)
    idx = torch.from_numpy(flat.astype(np.int32)).to(DEV)
    live_plan, scatter_plan = ops.live_plan(flat, DEV), ops.scatter_plan(flat, DEV)
    g = torch.randn(flat.size, d, device=DEV)

    def live():
        ops.GatherLiveRowsFn.apply(table, idx, live_plan).backward(g)

    def segment():
        ops.GatherRowsFn.apply(table, idx, scatter_plan).backward(g)

    def reset():
        table.grad = None

    out = alternate(dict(live=live, segment=segment), reset)
    out["live_faster"] = faster(out["live"], out["segment"])
    return out


def make_model(name, max_len, tmp):
    from selfrec_amd.data.loader import FileIO
    from selfrec_amd.model.sequential.GRU4Rec import GRU4Rec
    from selfrec_amd.util.conf import ModelConf
    train, test = synth.make_sequence_dataset(name)
    paths = [os.path.join(tmp, f"{name}-{k}.txt") for k in ("train", "test")]
    synth.write_sequences(paths[0], train)
    synth.write_sequences(paths[1], test)
    conf = ModelConf(os.path.join(ROOT, "conf", "GRU4Rec.yaml"))
    conf.config["training.set"], conf.config["test.set"], conf.config["max.len"] = paths[0], paths[1], max_len
    random.seed(1); torch.manual_seed(1)
    return GRU4Rec(conf, FileIO.load_data_set(paths[0], "sequential"), FileIO.load_data_set(paths[1], "sequential"))


def draw_batch(model, name, max_len, cache=None):
    """(seq, pos, y, neg) of the first batch of an epoch drawn after random.seed(0), from / into ``cache`` if given"""
    from selfrec_amd.util.sampler import next_batch_sequence
    path = os.path.join(cache, f"{name}-L{max_len}-B{model.batch_size}.npz") if cache else None
    if path and os.path.exists(path):
        with np.load(path) as f:
            return tuple(f[k] for k in ("seq", "pos", "y", "neg"))
    random.seed(0)
    batch = tuple(np.asarray(a) for a in next(iter(next_batch_sequence(model.data, model.batch_size, max_len=max_len)))[:4])
    if path:
        os.makedirs(cache, exist_ok=True)
        np.savez_compressed(path, **dict(zip(("seq", "pos", "y", "neg"), batch)))
    return batch


def step_ab(model, batch):
    from selfrec_amd.model.sequential.GRU4Rec import StagedSeqBatch
    from selfrec_amd.util.loss_torch import l2_reg_loss
    net = model.model.to(DEV)
    net.train()
    adam = torch.optim.Adam(net.parameters(), lr=model.lRate)
    times, staging = {"hip": [], "torch": []}, []
    seq, pos, y, neg = batch
    for rnd in range(WARMUP + REPEATS):
        for rnn in ("hip", "torch"):
            net.rnn = rnn
            torch.cuda.synchronize()
            s0 = time.perf_counter()
            staged = StagedSeqBatch(seq, torch.device(DEV), pos, y, neg)
            s1 = time.perf_counter()
            loss = model.calculate_loss(net.forward(seq, pos, staged=staged), y, neg, pos, staged=staged) \
                + l2_reg_loss(model.reg, net.item_emb)
            adam.zero_grad()
            loss.backward()
            adam.step()
            torch.cuda.synchronize()
            if rnd >= WARMUP:
                times[rnn].append((time.perf_counter() - s0) * 1e3)
                staging.append((s1 - s0) * 1e3)
    out = {k: stats(v) for k, v in times.items()}
    out["hip_faster"] = faster(out["hip"], out["torch"])
    out["staging_host"] = stats(staging)
    return out


def fmt(s):
    return f"{s['median']:.3f} ms [{s['min']:.3f}, {s['max']:.3f}]"


def notes(result):
    lines = ["# GRU4Rec: the recurrence kernels against torch.nn.GRU (tools/gru4rec_probe.py)", "",
             f"Device: {result['device']}.  Routes alternated in one process, {result['warmup']} warm-up rounds, "
             f"{result['repeats']} repeats, HIP events (the step: wall clock between synchronised fences), median [min, max].  "
             "A route counts as faster only when its whole range lies below its partner's.", ""]
    for name, r in result["sets"].items():
        rec, gat, step = r["recurrence"], r["gather"], r["step"]
        lines += [f"## {name}: B = {r['B']}, L = {r['L']}, d = {r['d']}", "",
                  f"- live fraction of the B L positions: {r['live_fraction']:.3f}; the kernels' grid: {r['workgroups']} "
                  "workgroups of 16 sequences on 256 CUs",
                  f"- recurrence forward + backward: `hip` {fmt(rec['hip'])}, peak {rec['hip']['peak_bytes'] / 1e6:.1f} MB; "
                  f"`torch` {fmt(rec['torch'])}, peak {rec['torch']['peak_bytes'] / 1e6:.1f} MB -> "
                  f"{'faster' if rec['hip_faster'] else 'NOT faster'}",
                  f"- item gather forward + backward: live rows {fmt(gat['live'])}; segment sum {fmt(gat['segment'])} -> "
                  f"{'faster' if gat['live_faster'] else 'NOT faster'}",
                  f"- whole step: `engine.rnn: hip` {fmt(step['hip'])}; `torch` {fmt(step['torch'])} -> "
                  f"{'faster' if step['hip_faster'] else 'NOT faster'}; staging on the host {fmt(step['staging_host'])}", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gru4rec_probe.json"))
    ap.add_argument("--notes", default=os.path.join(ROOT, "profiles", "NOTES_gru4rec.md"))
    ap.add_argument("--batches", default=None, help="directory that keeps the drawn batches between runs")
    ap.add_argument("--draw-only", action="store_true", help="draw the batches into --batches and stop (needs no GPU)")
    args = ap.parse_args()
    if not args.draw_only:
        torch.cuda.set_device(0)
        result = dict(device=torch.cuda.get_device_name(0), warmup=WARMUP, repeats=REPEATS, unit="ms", sets={})
    with tempfile.TemporaryDirectory() as tmp:
        for name, max_len in SETS:
            model = make_model(name, max_len, tmp)
            d = model.emb_size
            print(f"{name}: drawing one batch at max.len {max_len}", flush=True)
            batch = draw_batch(model, name, max_len, args.batches)
            seq = batch[0]
            B, L = seq.shape
            print(f"{name}: B = {B}, L = {L}", flush=True)
            if args.draw_only:
                continue
            result["sets"][name] = dict(B=B, L=L, d=d, live_fraction=float(np.count_nonzero(seq)) / seq.size,
                                        workgroups=(B + 15) // 16, recurrence=recurrence_ab(seq, d),
                                        gather=gather_ab(seq, model.data.item_num, d), step=step_ab(model, batch))
            print(f"{name}: " + json.dumps(result["sets"][name]), flush=True)
    if args.draw_only:
        return
    for path, text in ((args.out, json.dumps(result, indent=1)), (args.notes, notes(result))):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(text + "\n")
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
