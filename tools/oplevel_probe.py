"""Where does an op-level model's step go?  Runs N training steps of BUIR / MixGCF / DirectAU / SelfCF on the synthetic
Yelp2018-shaped graph with a device synchronisation after every statement of interest and prints the mean time of each
(GPU box only; tools/gpu_session.sh stage ``oplevel``).

    python tools/oplevel_probe.py BUIR 40

MixGCF's hop mixing has two routes (``engine.mixup``: csrc/mixgcf.hip or the reference's torch expression); ``--ab`` times
them against each other at the conf's shape (Yelp2018-shaped synthetic graph, B = 2048, 64 candidates, 3 layers, d = 64),
ALTERNATED inside one process -- hip, torch, hip, torch ... -- so that a drift of the machine lands on both: the mixing
forward and its backward on fixed hop tables (HIP events), one whole step (wall time between fences), and the peak memory
of each.  Warm-up first; median, min and max of the repeats.

    python tools/oplevel_probe.py MixGCF --ab [--repeats 30] [--out profiles/mixgcf_probe.json]

DirectAU's loss has two routes as well (``engine.au``: csrc/au.hip or the reference's expression over torch.pdist); its
``--ab`` alternates them the same way at the conf's shape (B = 2048, 3 layers, d = 64): the loss forward on the two gathered
blocks, its backward, the peak memory above the inputs, and one whole step.

    python tools/oplevel_probe.py DirectAU --ab [--repeats 30] [--out profiles/directau_probe.json]

BUIR and SelfCF share the bootstrap route (``engine.boot``: csrc/bootstrap.hip or the reference's torch expressions); their
``--ab`` alternates the routes at the conf's shape (B = 2048, 2 layers, d = 64): the model-specific piece -- target gather or
momentum mix, predictor, loss, backward, history store -- forward plus backward on prepared inputs, BUIR's ``update_target``
alone, the peak memory of the piece above its inputs, and one whole step.  Each model writes its own key of the file.

    python tools/oplevel_probe.py BUIR --ab [--repeats 30] [--out profiles/boot_probe.json]
    python tools/oplevel_probe.py SelfCF --ab
"""
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from selfrec_amd import synth                                              # noqa: E402
from selfrec_amd.data.loader import FileIO                                 # noqa: E402,F401
from selfrec_amd.util import torch_rng                                     # noqa: E402
from selfrec_amd.util.conf import ModelConf                                # noqa: E402

ATEN_RAND = bool(int(__import__("os").environ.get("PROBE_ATEN_RAND", "0")))


def build(model_name):
    import importlib
    import os
    conf = ModelConf(f"./conf/{model_name}.yaml")
    if not os.path.exists(conf["training.set"]):
        tu, ti, su, si, _, _ = synth.make_dataset("yelp2018")
        os.makedirs(os.path.dirname(conf["training.set"]) or ".", exist_ok=True)
        synth.write_text(conf["training.set"], tu, ti)
        synth.write_text(conf["test.set"], su, si)
    train = FileIO.load_data_set(conf["training.set"], conf["model"]["type"])
    test = FileIO.load_data_set(conf["test.set"], conf["model"]["type"])
    cls = getattr(importlib.import_module(f"selfrec_amd.model.graph.{model_name}"), model_name)
    return cls(conf, train, test)


class Clock:
    def __init__(self):
        self.t, self.acc, self.n = time.perf_counter(), {}, {}

    def lap(self, name):
        torch.cuda.synchronize()
        now = time.perf_counter()
        self.acc[name] = self.acc.get(name, 0.0) + now - self.t
        self.n[name] = self.n.get(name, 0) + 1
        self.t = time.perf_counter()

    def report(self, steps):
        for k, v in self.acc.items():
            print(f"  {k:34s} {1e3 * v / steps:9.3f} ms/step  ({self.n[k] // steps} per step)")
        print(f"  {'total':34s} {1e3 * sum(self.acc.values()) / steps:9.3f} ms/step")


def probe_buir(rec, steps):
    from selfrec_amd.util.sampler import next_batch_pairwise
    model = rec.model.cuda()
    opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=rec.lRate)
    ck = Clock()

    def enc_forward(enc, inputs):
        rate = np.random.random() * enc.drop_ratio
        if ATEN_RAND:
            keep = torch.floor(1 - rate + torch.rand(enc.sparse_norm_adj._nnz())).type(torch.bool)
        else:
            keep = torch_rng.keep_mask(enc.sparse_norm_adj._nnz(), 1 - rate)
        ck.lap("keep mask (host: %s)" % ("ATen torch.rand" if ATEN_RAND else "util/torch_rng replay"))
        adj = enc.sparse_norm_adj.dropout(keep, 1.0 / (1 - rate))
        ck.lap("SparseAdjHandle.dropout")
        hops = enc.hops(adj)
        ck.lap("hops (SpMM)")
        mean = torch.stack(hops, dim=1).mean(dim=1)
        ck.lap("stack + mean")
        out = mean[:enc.data.user_num][inputs["user"]], mean[enc.data.user_num:][inputs["item"]]
        ck.lap("row gathers")
        return out

    it = next_batch_pairwise(rec.data, rec.batch_size, 1, as_arrays=True)
    for step in range(steps + 3):
        if step == 3:
            ck = Clock()
        u, i, _ = (torch.from_numpy(a).cuda() for a in next(it))
        ck.lap("sampler + H2D")
        inputs = {"user": u, "item": i}
        u_on, i_on = enc_forward(model.online_encoder, inputs)
        u_tg, i_tg = enc_forward(model.target_encoder, inputs)
        loss = model.get_loss((model.predictor(u_on), u_tg, model.predictor(i_on), i_tg))
        ck.lap("predictor + loss")
        opt.zero_grad()
        loss.backward()
        ck.lap("backward")
        opt.step()
        ck.lap("Adam")
        model.update_target(u, i)
        ck.lap("update_target")
    ck.report(steps)


def probe_generic(rec, steps):
    from selfrec_amd.util.sampler import next_batch_pairwise
    model = rec.model.cuda()
    opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=rec.lRate)
    ck = Clock()
    it = next_batch_pairwise(rec.data, rec.batch_size, rec.n_negs, as_arrays=True)
    for step in range(steps + 3):
        if step == 3:
            ck = Clock()
        u, i, j = (torch.from_numpy(a).cuda() for a in next(it))
        ck.lap("sampler + H2D")
        loss = rec.batch_loss(u, i, j)
        ck.lap("batch_loss (forward)")
        opt.zero_grad()
        loss.backward()
        ck.lap("backward")
        opt.step()
        ck.lap("Adam")
        rec.after_step(u, i, j)
        ck.lap("after_step")
    ck.report(steps)


def probe_mixgcf_ab(repeats, out):
    import json
    import os
    import random
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from bert4rec_probe import peak_extra_bytes
    from sept_probe import alternating, stats
    from selfrec_amd import ops
    from selfrec_amd.model.graph.MixGCF import MixGCF, mixup_torch
    from selfrec_amd.util.sampler import next_batch_pairwise
    ops.require_gpu()
    B, C, L, d = 2048, 64, 3, 64
    tu, ti, su, si, _, _ = synth.make_dataset("yelp2018")

    def make(route):
        conf = ModelConf({"training.set": "./none", "test.set": "./none", "model": {"name": "MixGCF", "type": "graph"},
                          "item.ranking.topN": [10, 20], "embedding.size": d, "max.epoch": 1, "batch.size": B,
                          "learning.rate": 0.001, "reg.lambda": 0.0001, "output": "./results/",
                          "MixGCF": {"n_layer": L, "n_negs": C}, "engine.mixup": route})
        torch.manual_seed(0)
        m = MixGCF(conf, synth.as_triples(tu, ti), synth.as_triples(su, si))
        m.model.cuda().train()
        assert m.model.mixup == route
        return m
    models = {r: make(r) for r in ("hip", "torch")}
    base = models["hip"]
    random.seed(1)
    idx = [torch.from_numpy(a).cuda() for a in next(iter(next_batch_pairwise(base.data, B, C, as_arrays=True)))]
    user, pos, neg = idx
    res = {"shape": {"dataset": "yelp2018 (synthetic)", "users": base.data.user_num, "items": base.data.item_num, "B": B,
                     "n_negs": C, "n_layer": L, "d": d}}

    # ---- the mixing alone, on fixed hop tables ----------------------------------------------------------------------------
    with torch.no_grad():
        users, item_hops = base.model.hop_tables()
        u = users[user].contiguous()
        item_hops = [h.contiguous() for h in item_hops]
    g = torch.Generator().manual_seed(0)
    gp, gn = torch.randn(B, d, generator=g).cuda(), torch.randn(B, d, generator=g).cuda()

    def forward(route):
        hops = [h.clone().requires_grad_(True) for h in item_hops]
        if route == "hip":
            return ops.MixupFn.apply(u, pos, neg, C, None, 1234, 0, *hops)[:2]
        return mixup_torch(u, hops, pos, neg, C)
    res["mixup_fwd_ms"] = alternating({r: (lambda r=r: forward(r)) for r in ("hip", "torch")}, 5, repeats)
    ts = {"hip": [], "torch": []}
    for k in range(5 + repeats):
        for r in ts:
            outs = forward(r)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            torch.autograd.backward(list(outs), [gp, gn])
            t1.record()
            t1.synchronize()
            if k >= 5:
                ts[r].append(t0.elapsed_time(t1))
    res["mixup_bwd_ms"] = {r: stats(v) for r, v in ts.items()}

    def fwd_bwd(route):
        torch.autograd.backward(list(forward(route)), [gp, gn])
    res["mixup_peak_extra_bytes"] = {r: peak_extra_bytes(lambda r=r: fwd_bwd(r)) for r in ("hip", "torch")}

    # ---- the whole step -----------------------------------------------------------------------------------------------------
    steps = {}
    for name, m in models.items():
        opt = torch.optim.Adam(m.model.parameters(), lr=1e-3)

        def step(m=m, opt=opt):
            loss = m.batch_loss(*idx)
            opt.zero_grad()
            loss.backward()
            opt.step()
        steps[name] = step
    res["step_wall_ms"] = alternating(steps, 5, repeats, wall=True)
    res["step_peak_extra_bytes"] = {name: peak_extra_bytes(fn) for name, fn in steps.items()}
    peak = {}
    for name, fn in steps.items():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        peak[name] = int(torch.cuda.max_memory_allocated())
    res["step_max_memory_allocated"] = peak
    med = lambda key, r: res[key][r]["median"]  # noqa: E731
    res["hip_over_torch"] = {k: med(k, "hip") / med(k, "torch") for k in ("mixup_fwd_ms", "mixup_bwd_ms", "step_wall_ms")}
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


def probe_directau_ab(repeats, out):
    """DirectAU's loss on its two routes (``engine.au``: csrc/au.hip or the reference's torch expression over torch.pdist)
    at the conf's shape, alternated in one process: the loss forward alone on two fixed gathered B x d blocks, its backward
    alone (HIP events), the peak memory of forward + backward above the inputs, and one whole training step (wall time
    between fences)."""
    import json
    import os
    import random
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from bert4rec_probe import peak_extra_bytes
    from sept_probe import alternating, stats
    from selfrec_amd import ops
    from selfrec_amd.model.graph.DirectAU import DirectAU, alignment, uniformity
    from selfrec_amd.util.sampler import next_batch_pairwise
    ops.require_gpu()
    B, L, d, gamma = 2048, 3, 64, 2.0
    tu, ti, su, si, _, _ = synth.make_dataset("yelp2018")

    def make(route):
        conf = ModelConf({"training.set": "./none", "test.set": "./none", "model": {"name": "DirectAU", "type": "graph"},
                          "item.ranking.topN": [10, 20], "embedding.size": d, "max.epoch": 1, "batch.size": B,
                          "learning.rate": 0.001, "reg.lambda": 0.0001, "output": "./results/",
                          "DirectAU": {"gamma": gamma, "n_layers": L}, "engine.au": route})
        torch.manual_seed(0)
        m = DirectAU(conf, synth.as_triples(tu, ti), synth.as_triples(su, si))
        m.model.cuda().train()
        assert m.au == route
        return m
    os.environ.pop("SRH_DIRECTAU_AU", None)
    models = {r: make(r) for r in ("hip", "torch")}
    base = models["hip"]
    random.seed(1)
    idx = [torch.from_numpy(a).cuda() for a in next(iter(next_batch_pairwise(base.data, B, 1, as_arrays=True)))]
    user, pos, _ = idx
    res = {"shape": {"dataset": "yelp2018 (synthetic)", "users": base.data.user_num, "items": base.data.item_num, "B": B,
                     "n_layers": L, "d": d, "gamma": gamma, "t": 2}}

    # ---- the loss alone, on the two gathered blocks ---------------------------------------------------------------------
    with torch.no_grad():
        users, items = base.model()
        u0, p0 = users[user].contiguous(), items[pos].contiguous()

    def forward(route):
        u, p = u0.clone().requires_grad_(True), p0.clone().requires_grad_(True)
        if route == "hip":
            return ops.AlignUniformFn.apply(u, p, 2.0, 1.0, gamma / 2, gamma / 2)
        return alignment(u, p) + gamma * (uniformity(u) + uniformity(p)) / 2
    with torch.no_grad():
        res["loss_value"] = {r: float(forward(r)) for r in ("hip", "torch")}
    res["loss_fwd_ms"] = alternating({r: (lambda r=r: forward(r)) for r in ("hip", "torch")}, 5, repeats)
    ts = {"hip": [], "torch": []}
    for k in range(5 + repeats):
        for r in ts:
            loss = forward(r)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            loss.backward()
            t1.record()
            t1.synchronize()
            if k >= 5:
                ts[r].append(t0.elapsed_time(t1))
    res["loss_bwd_ms"] = {r: stats(v) for r, v in ts.items()}
    res["loss_peak_extra_bytes"] = {r: peak_extra_bytes(lambda r=r: forward(r).backward()) for r in ("hip", "torch")}

    # ---- the whole step -------------------------------------------------------------------------------------------------
    steps = {}
    for name, m in models.items():
        opt = torch.optim.Adam(m.model.parameters(), lr=1e-3)

        def step(m=m, opt=opt):
            loss = m.batch_loss(*idx)
            opt.zero_grad()
            loss.backward()
            opt.step()
        steps[name] = step
    res["step_wall_ms"] = alternating(steps, 5, repeats, wall=True)
    res["step_peak_extra_bytes"] = {name: peak_extra_bytes(fn) for name, fn in steps.items()}
    med = lambda key, r: res[key][r]["median"]  # noqa: E731
    res["hip_over_torch"] = {k: med(k, "hip") / med(k, "torch") for k in ("loss_fwd_ms", "loss_bwd_ms", "step_wall_ms")}
    res["step_ranges_touch"] = not (res["step_wall_ms"]["hip"]["max"] < res["step_wall_ms"]["torch"]["min"]
                                    or res["step_wall_ms"]["torch"]["max"] < res["step_wall_ms"]["hip"]["min"])
    res["repeats"], res["warmup"] = repeats, 5
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


def probe_boot_ab(name, repeats, out):
    """BUIR's or SelfCF's model-specific piece on its two routes (``engine.boot``), alternated in one process: the piece
    forward + backward on prepared inputs (HIP events), BUIR's update_target alone, the peak memory of the piece above its
    inputs, and one whole training step with its after_step (wall time between fences)."""
    import importlib
    import json
    import os
    import random
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from bert4rec_probe import peak_extra_bytes
    from sept_probe import alternating
    from selfrec_amd import ops
    from selfrec_amd.util.sampler import next_batch_pairwise
    ops.require_gpu()
    B, L, d = 2048, 2, 64
    block = {"BUIR": {"n_layer": L, "tau": 0.995, "drop_rate": 0.2}, "SelfCF": {"n_layer": L, "tau": 0.05}}[name]
    tu, ti, su, si, _, _ = synth.make_dataset("yelp2018")
    cls = getattr(importlib.import_module(f"selfrec_amd.model.graph.{name}"), name)

    def make(route):
        conf = ModelConf({"training.set": "./none", "test.set": "./none", "model": {"name": name, "type": "graph"},
                          "item.ranking.topN": [10, 20], "embedding.size": d, "max.epoch": 1, "batch.size": B,
                          "learning.rate": 0.001, "reg.lambda": 0.0001, "output": "./results/", name: block,
                          "engine.boot": route})
        torch.manual_seed(0)
        m = cls(conf, synth.as_triples(tu, ti), synth.as_triples(su, si))
        m.model.cuda().train()
        assert m.boot == route
        return m
    os.environ.pop("SRH_BOOT", None)
    models = {r: make(r) for r in ("hip", "torch")}
    base = models["hip"].model
    random.seed(1)
    idx = [torch.from_numpy(a).cuda() for a in next(iter(next_batch_pairwise(models["hip"].data, B, 1, as_arrays=True)))]
    user, pos, _ = idx
    u32, p32 = user.to(torch.int32), pos.to(torch.int32)
    res = {"shape": {"dataset": "yelp2018 (synthetic)", "users": models["hip"].data.user_num,
                     "items": models["hip"].data.item_num, "B": B, "n_layer": L, "d": d, **block}}

    # ---- the model-specific piece alone, on prepared inputs ---------------------------------------------------------------
    W, b = base.predictor.weight, base.predictor.bias
    with torch.no_grad():
        on = base.online_encoder
        u_all, i_all = super(type(on), on).forward() if name == "BUIR" else on()        # (BUIR: the tables without dropout)
        u0, i0 = u_all[user].contiguous(), i_all[pos].contiguous()
        if name == "BUIR":
            t_u, t_i = (t.contiguous() for t in super(type(base.target_encoder), base.target_encoder).forward())
        else:
            his = {r: (base.u_target_his.clone(), base.i_target_his.clone()) for r in ("hip", "torch")}
    mom = getattr(base, "momentum", None)

    def piece(route):
        u, i = u0.clone().requires_grad_(True), i0.clone().requires_grad_(True)
        W.grad = b.grad = None
        if name == "BUIR":
            if route == "hip":
                loss = ops.BootstrapLossFn.apply(u, i, W, b, t_u, t_i, u32, p32, None, None, 1.0, 0.0, 1e-12, 4.0, 2.0)
            else:
                loss = base.get_loss((base.predictor(u), t_u[user], base.predictor(i), t_i[pos]))
        else:
            hu, hi = his[route]
            if route == "hip":
                loss = ops.BootstrapLossFn.apply(u, i, W, b, hu, hi, user, pos, hu, hi, mom, 1. - mom, 1e-8, 1.0, 0.5, True)
            else:
                with torch.no_grad():
                    u_target = hu[user] * mom + u.data * (1. - mom)
                    i_target = hi[pos] * mom + i.data * (1. - mom)
                    hu[user, :] = u.data.clone()
                    hi[pos, :] = i.data.clone()
                loss = base.get_loss((base.predictor(u), u_target, base.predictor(i), i_target))
        loss.backward()
        return loss
    res["piece_loss_value"] = {r: float(piece(r)) for r in ("hip", "torch")}
    res["piece_fwd_bwd_ms"] = alternating({r: (lambda r=r: piece(r)) for r in ("hip", "torch")}, 5, repeats)
    res["piece_peak_extra_bytes"] = {r: peak_extra_bytes(lambda r=r: piece(r)) for r in ("hip", "torch")}
    keys = ["piece_fwd_bwd_ms", "step_wall_ms"]
    if name == "BUIR":
        upd = {"hip": lambda: base.update_target_rows(u32, p32), "torch": lambda: base.update_target(user, pos)}
        res["update_target_ms"] = alternating(upd, 5, repeats)
        keys.insert(1, "update_target_ms")

    # ---- the whole step ---------------------------------------------------------------------------------------------------
    steps = {}
    for route, m in models.items():
        opt = torch.optim.Adam([p for p in m.model.parameters() if p.requires_grad], lr=1e-3)

        def step(m=m, opt=opt):
            loss = m.batch_loss(*idx)
            opt.zero_grad()
            loss.backward()
            opt.step()
            m.after_step(*idx)
        steps[route] = step
    res["step_wall_ms"] = alternating(steps, 5, repeats, wall=True)
    res["step_peak_extra_bytes"] = {route: peak_extra_bytes(fn) for route, fn in steps.items()}
    med = lambda key, r: res[key][r]["median"]  # noqa: E731
    res["hip_over_torch"] = {k: med(k, "hip") / med(k, "torch") for k in keys}
    res["step_ranges_touch"] = not (res["step_wall_ms"]["hip"]["max"] < res["step_wall_ms"]["torch"]["min"]
                                    or res["step_wall_ms"]["torch"]["max"] < res["step_wall_ms"]["hip"]["min"])
    res["repeats"], res["warmup"] = repeats, 5
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    whole = {}
    if os.path.exists(out):
        with open(out) as f:
            whole = json.load(f)
    whole[name] = res
    with open(out, "w") as f:
        json.dump(whole, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    if "--ab" in sys.argv:
        import argparse
        ap = argparse.ArgumentParser()
        ap.add_argument("model", choices=["MixGCF", "DirectAU", "BUIR", "SelfCF"])
        ap.add_argument("--ab", action="store_true")
        ap.add_argument("--repeats", type=int, default=30)
        ap.add_argument("--out", default=None)
        args = ap.parse_args()
        assert args.repeats >= 5
        if args.model in ("BUIR", "SelfCF"):
            probe_boot_ab(args.model, args.repeats, args.out or "profiles/boot_probe.json")
        elif args.model == "DirectAU":
            probe_directau_ab(args.repeats, args.out or "profiles/directau_probe.json")
        else:
            probe_mixgcf_ab(args.repeats, args.out or "profiles/mixgcf_probe.json")
        sys.exit(0)
    name = sys.argv[1] if len(sys.argv) > 1 else "BUIR"
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 40
    rec = build(name)
    print(f"{name}: {steps} steps, every statement synchronised")
    (probe_buir if name == "BUIR" else probe_generic)(rec, steps)
