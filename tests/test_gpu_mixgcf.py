"""MixGCF's hop-mixing kernels (csrc/mixgcf.hip through ops.mixup_fwd / mixup_bwd / MixupFn) and the model's kernel route
on the GPU, against the float64 restatement of tests/mixgcf_ref.py on the cases of tests/mixgcf_cases.py.

A pick is judged by the float64 scores: the picked candidate's score is within the float32 margin of the float64 maximum,
and where the float64 top-two gap exceeds that margin the pick IS the float64 argmax.  Outputs and gradient tables are
compared to the restatement evaluated at the kernel's picks, at the project's standing bounds (1e-5 forward, 1e-4
gradients, of the largest magnitude of the compared tensor)."""
import json
import os
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import mixgcf_cases as mc, mixgcf_ref as ref
from tests.test_shapes_cpu import GOLDEN

pytestmark = pytest.mark.gpu


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def on_device(case):
    c = mc.inputs(case)
    return dict(u=dev(c["u"]), hops=[dev(t) for t in c["tables"]], pos=dev(c["pos"]), neg=dev(c["neg"]),
                alpha=dev(c["alpha"]), g_pos=dev(c["g_pos"]), g_neg=dev(c["g_neg"]))


def cpu(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize("case", mc.CASES, ids=mc.case_id)
def test_forward_and_backward(case):
    from selfrec_amd import ops
    fam, B, H, C, d, n_items = case
    c, r, t = mc.inputs(case), mc.reference(case), on_device(case)
    pos_out, neg_out, pick = ops.mixup_fwd(t["u"], t["hops"], t["pos"], t["neg"], C, alpha=t["alpha"])
    assert pick.dtype == torch.int32 and tuple(pick.shape) == (H, B)
    pk = cpu(pick)
    outside, wrong = mc.judge_pick(case, pk)
    want_pos, want_neg = ref.outputs(c["tables"], c["pos"], c["neg"], c["alpha"], pk)
    e_pos, e_neg = mc.rel_err(cpu(pos_out), want_pos), mc.rel_err(cpu(neg_out), want_neg)
    grads = ops.mixup_bwd(t["hops"], t["pos"], t["neg"], C, pick, t["g_pos"], t["g_neg"], alpha=t["alpha"])
    assert len(grads) == H and all(tuple(g.shape) == (n_items, d) for g in grads)
    got = np.stack([cpu(g) for g in grads])
    want = ref.grads(n_items, c["pos"], c["neg"], c["alpha"], pk, c["g_pos"], c["g_neg"])
    e_grad = mc.rel_err(got, want)
    differs = int((pk != r["amax"]).sum())
    print(f"{mc.case_id(case)}: picks outside the margin {outside}, wrong with a clear winner {wrong}, unlike the float64 "
          f"argmax {differs} of {pk.size}; errors pos_out {e_pos:.2e} neg_out {e_neg:.2e} gradients {e_grad:.2e}")
    assert outside == 0 and wrong == 0
    assert e_pos < mc.FWD_BOUND and e_neg < mc.FWD_BOUND
    assert e_grad < mc.GRAD_BOUND
    assert (got[want == 0] == 0).all()                   # written whole: exactly zero outside the touched rows
    # pos_out is the hop-mean table's rows
    mean_rows = torch.stack(t["hops"], 1).mean(1)[t["pos"]]
    assert mc.rel_err(cpu(pos_out), cpu(mean_rows).astype(np.float64)) < mc.FWD_BOUND

    if fam in ("zero_user", "dup"):
        assert (pk == 0).all()
    if fam == "alpha0":
        # the mixture is the candidate's own row, and the positive takes nothing from g_neg
        negs = c["neg"].reshape(B, C)
        raw = np.stack([c["tables"][k][negs[np.arange(B), pk[k]]] for k in range(H)]).astype(np.float64).mean(0)
        assert mc.rel_err(cpu(neg_out), raw) < mc.FWD_BOUND
        only_neg = ops.mixup_bwd(t["hops"], t["pos"], t["neg"], C, pick, None, t["g_neg"], alpha=t["alpha"])
        for k in range(H):
            untouched = np.setdiff1d(c["pos"], negs[np.arange(B), pk[k]])
            assert (cpu(only_neg[k])[untouched] == 0).all()
    if fam == "pos_is_neg":
        # where a pair picked its own positive and no other entry of the hop touches that item, both contributions land in
        # the one row: alpha g + (1 - alpha) g = g_neg, plus g_pos, over H
        negs = c["neg"].reshape(B, C)
        seen = 0
        for k in range(H):
            picked = negs[np.arange(B), pk[k]]
            touched = np.concatenate([c["pos"], picked])
            for b in np.nonzero(picked == c["pos"])[0]:
                if (touched == c["pos"][b]).sum() == 2:
                    w = (c["g_pos"][b].astype(np.float64) + c["g_neg"][b]) / H
                    assert np.abs(got[k, c["pos"][b]] - w).max() < mc.GRAD_BOUND * np.abs(w).max()
                    seen += 1
        assert seen > 0 or C > 1

    if c["drawn"]:
        # the same call with alpha drawn in the kernel: the same bits in every output
        rng = dict(rng_seed=c["rng_seed"], rng_counter=c["rng_counter"])
        pos2, neg2, pick2 = ops.mixup_fwd(t["u"], t["hops"], t["pos"], t["neg"], C, **rng)
        assert torch.equal(pick2, pick) and torch.equal(pos2, pos_out) and torch.equal(neg2, neg_out)
        grads2 = ops.mixup_bwd(t["hops"], t["pos"], t["neg"], C, pick, t["g_pos"], t["g_neg"], **rng)
        assert all(torch.equal(a, b) for a, b in zip(grads, grads2))


def test_mixup_fn_is_the_wrappers_under_autograd():
    from selfrec_amd import ops
    case = ("normal", 65, 4, 64, 64, 300)
    fam, B, H, C, d, n_items = case
    c, t = mc.inputs(case), on_device(case)
    rng = dict(rng_seed=c["rng_seed"], rng_counter=c["rng_counter"])
    # the hop tables as the model hands them over: the item rows of wider (users + items) tables, no copy
    n_u = 7
    wide = [torch.cat([torch.randn(n_u, d, device="cuda"), h], 0).requires_grad_() for h in t["hops"]]
    hops = [w[n_u:] for w in wide]
    u = t["u"].clone().requires_grad_()
    pos_out, neg_out, pick = ops.MixupFn.apply(u, t["pos"], t["neg"], C, None, rng["rng_seed"], rng["rng_counter"], *hops)
    want = ops.mixup_fwd(t["u"], t["hops"], t["pos"], t["neg"], C, **rng)
    assert torch.equal(pos_out, want[0]) and torch.equal(neg_out, want[1]) and torch.equal(pick, want[2])
    assert not pick.requires_grad
    ((pos_out * t["g_pos"]).sum() + (neg_out * t["g_neg"]).sum()).backward()
    grads = ops.mixup_bwd(t["hops"], t["pos"], t["neg"], C, pick, t["g_pos"], t["g_neg"], **rng)
    assert u.grad is None
    for w, g in zip(wide, grads):
        assert torch.equal(w.grad[n_u:], g) and (w.grad[:n_u] == 0).all()
    # injected alpha through the Function: the same results
    u2 = [h.clone().requires_grad_() for h in t["hops"]]
    out = ops.MixupFn.apply(t["u"], t["pos"], t["neg"], C, [a for a in t["alpha"]], 0, 0, *u2)
    assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1]) and torch.equal(out[2], want[2])
    ((out[0] * t["g_pos"]).sum() + (out[1] * t["g_neg"]).sum()).backward()
    assert all(torch.equal(h.grad, g) for h, g in zip(u2, grads))


# ---- the model on the 200 x 300 graph ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def meta():
    with open(os.path.join(GOLDEN, "shapes_meta.json")) as f:
        return json.load(f)["M_MixGCF"]


def build(meta, data, route, epochs=1):
    from selfrec_amd.model.graph.MixGCF import MixGCF
    from selfrec_amd.util.conf import ModelConf
    conf = ModelConf({"model": {"name": "MixGCF", "type": "graph"}, "item.ranking.topN": [10, 20],
                      "embedding.size": meta["emb"], "max.epoch": epochs, "batch.size": meta["batch"],
                      "learning.rate": meta["lr"], "reg.lambda": meta["reg"], "output": "./results/", "training.set": "x",
                      "test.set": "y", "MixGCF": meta["conf"], "engine.mixup": route})
    torch.manual_seed(meta["torch_seed"]); np.random.seed(meta["numpy_seed"]); random.seed(meta["sampler_seed"])
    model = MixGCF(conf, data.training_data, data.test_data)
    model.fast_evaluation = lambda epoch: None
    assert model.model.mixup == route
    return model


def limit_batches(monkeypatch, n_steps, seen):
    from selfrec_amd.util import sampler as sampler_mod
    real = sampler_mod.next_batch_pairwise

    def batches(data, bs, n_negs=1, **kw):
        for k, b in enumerate(real(data, bs, n_negs, **kw)):
            if n_steps is not None and k == n_steps:
                return
            seen.append(b)
            yield b
    monkeypatch.setattr(sampler_mod, "next_batch_pairwise", batches)


def test_model_routes_agree_under_injected_draws(meta, golden_ops, monkeypatch, tmp_path):
    """Two steps by engine.mixup: hip and by torch under the same patched rand_like / F.dropout, both drawing from a seeded
    CPU generator: losses to rtol 2e-5, parameters to 1e-5 (tests/test_gpu_f4.py's bounds for this model)."""
    from tests.conftest import _tiny_interaction
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("SRH_MIXGCF_MIXUP", raising=False)
    real_backward = torch.Tensor.backward
    runs = {}
    for route in ("hip", "torch"):
        gen = torch.Generator().manual_seed(meta["device_rng_seed"])

        def cpu_dropout(x, p=0.5, training=True, inplace=False, gen=gen):
            if not training or p == 0.0:
                return x
            keep = (torch.rand(x.shape, generator=gen) >= p).to(x.dtype).to(x.device)
            return x * keep / (1.0 - p)
        calls, losses = [], []
        with monkeypatch.context() as mp:
            mp.setattr(F, "dropout", cpu_dropout)
            mp.setattr(torch, "rand_like",
                       lambda t, gen=gen, calls=calls, **k: (calls.append(tuple(t.shape)),
                                                             torch.rand(t.shape, generator=gen).to(t.device))[1])
            mp.setattr(torch.Tensor, "backward",
                       lambda t, *a, losses=losses, **k: (losses.append(float(t.detach())), real_backward(t, *a, **k))[1])
            limit_batches(mp, meta["n_steps"], [])
            model = build(meta, _tiny_interaction(golden_ops), route)
            model.train()
        H = meta["conf"]["n_layer"] + 1
        assert len(calls) == H * meta["n_steps"]
        assert all(s == (meta["batch"], meta["conf"]["n_negs"], meta["emb"]) for s in calls)
        runs[route] = (losses, {k: cpu(v) for k, v in model.model.named_parameters()})
    print("losses", runs["hip"][0], runs["torch"][0])
    np.testing.assert_allclose(runs["hip"][0], runs["torch"][0], rtol=2e-5)
    for k, v in runs["hip"][1].items():
        assert np.abs(v - runs["torch"][1][k]).max() < 1e-5, k


def test_model_trains_on_the_kernel_route_and_repeats_bit_for_bit(meta, golden_ops, monkeypatch, tmp_path):
    """Nothing patched: alpha is drawn in the kernel.  Two short epochs; the counter advances by H B C per step; two runs
    from the same torch.manual_seed end with the same bits; test() ranks."""
    from tests.conftest import _tiny_interaction
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("SRH_MIXGCF_MIXUP", raising=False)
    H, C = meta["conf"]["n_layer"] + 1, meta["conf"]["n_negs"]
    ends = []
    for _ in range(2):
        seen = []
        with monkeypatch.context() as mp:
            limit_batches(mp, 3, seen)
            model = build(meta, _tiny_interaction(golden_ops), "hip", epochs=2)
            before = {k: cpu(v).copy() for k, v in model.model.named_parameters()}
            model.train()
        assert len(seen) == 6
        assert model.model.rng_counter == sum(H * len(b[0]) * C for b in seen)
        after = {k: cpu(v) for k, v in model.model.named_parameters()}
        assert all(np.isfinite(v).all() and not np.array_equal(v, before[k]) for k, v in after.items())
        ends.append(after)
    for k, v in ends[0].items():
        assert np.array_equal(v, ends[1][k]), k
    with torch.no_grad():
        model.snapshot()
    rec = model.test()
    assert len(rec) > 0 and all(len(v) == 20 for v in rec.values())
