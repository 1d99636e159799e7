"""MixGCF's hop mixing without a GPU: the float64 restatement the GPU tests compare against (tests/mixgcf_ref.py) is held
to the model's own torch expression under autograd, the inputs of every case are held to what their family promises, the
counter layout of a drawn alpha is spelt out, and plain float32 numpy is measured on every case as the yardstick."""
import numpy as np
import pytest
import torch

from tests import counter_rng, mixgcf_cases as mc, mixgcf_ref as ref


@pytest.fixture(scope="module")
def mixup_torch():
    from selfrec_amd.model.graph.MixGCF import mixup_torch
    return mixup_torch


@pytest.mark.parametrize("case", mc.CASES, ids=mc.case_id)
def test_restatement_is_the_torch_expression_in_float64(case, mixup_torch, monkeypatch):
    """mixup_torch on CPU float64 tensors, its rand_like replaced by the case's alpha hop by hop, against the restatement
    at the restatement's own argmax: outputs and autograd's gradient tables to 1e-12 of their magnitude.  (A wrong pick
    moves a whole row of both, so equal outputs and gradients are equal picks wherever two candidates differ.)"""
    fam, B, H, C, d, n_items = case
    c, r = mc.inputs(case), mc.reference(case)
    hops = iter(c["alpha"])

    def rand_like(t, **kw):
        a = torch.from_numpy(next(hops).astype(np.float64))
        assert tuple(t.shape) == tuple(a.shape)
        return a
    monkeypatch.setattr(torch, "rand_like", rand_like)
    tables = [torch.tensor(t, dtype=torch.float64, requires_grad=True) for t in c["tables"]]
    u = torch.tensor(c["u"], dtype=torch.float64)
    pos_rows, negs = mixup_torch(u, tables, torch.from_numpy(c["pos"]), torch.from_numpy(c["neg"]), C)
    want_pos, want_neg = ref.outputs(c["tables"], c["pos"], c["neg"], c["alpha"], r["amax"])
    assert mc.rel_err(pos_rows.detach().numpy(), want_pos) < 1e-12
    assert mc.rel_err(negs.detach().numpy(), want_neg) < 1e-12
    loss = (pos_rows * torch.from_numpy(c["g_pos"]).double()).sum() + (negs * torch.from_numpy(c["g_neg"]).double()).sum()
    loss.backward()
    got = np.stack([t.grad.numpy() for t in tables])
    want = ref.grads(n_items, c["pos"], c["neg"], c["alpha"], r["amax"], c["g_pos"], c["g_neg"])
    assert mc.rel_err(got, want) < 1e-12
    assert u.grad is None


@pytest.mark.parametrize("case", mc.CASES, ids=mc.case_id)
def test_case_inputs_are_what_their_family_promises(case):
    fam, B, H, C, d, n_items = case
    c, r = mc.inputs(case), mc.reference(case)
    assert c["alpha"].min() >= 0.0 and c["alpha"].max() < 1.0 and c["alpha"].dtype == np.float32
    assert c["pos"].min() >= 0 and c["pos"].max() < n_items and c["neg"].min() >= 0 and c["neg"].max() < n_items
    close = r["gap"] <= r["margin"]
    if fam in ("normal", "pos_is_neg", "all_negative"):   # (collide: I = 3 repeats the positive among its candidates)
        # a condition on the inputs, not a tolerance of the kernel: almost every row has a clear float64 winner
        print(f"{mc.case_id(case)}: {int(close.sum())} of {close.size} rows within the margin")
        assert close.sum() <= mc.NEAR_TIE_CAP * close.size
    if fam == "zero_user":
        assert (r["s"] == 0).all() and not np.signbit(r["s"]).any() and (r["amax"] == 0).all()
    if fam == "all_negative":
        assert (r["s"] < 0).all()
    if fam == "dup":
        assert (r["s"] == r["s"][:, :, :1]).all() and (r["amax"] == 0).all()
    if fam == "pos_is_neg":
        assert (c["neg"].reshape(B, C)[np.arange(B), np.arange(B) % C] == c["pos"]).all()
        assert B > n_items or len(set(c["pos"].tolist())) == B
    if fam == "near_tie":
        order = np.argsort(r["s"], axis=2)
        assert (np.sort(order[:, :, -2:], axis=2) == np.array([0, C - 1])).all()       # the two built candidates lead
        assert close.all() and (r["gap"] < 0.01 * r["margin"]).all()
    if fam == "alpha0":
        assert (c["alpha"] == 0).all()
    if fam == "alpha1m":
        assert (c["alpha"] == np.float32(1.0 - 2.0 ** -24)).all() and (np.float32(1.0) - c["alpha"] == 2.0 ** -24).all()


def test_drawn_alpha_is_one_block_of_consecutive_counters():
    """row (k, b, c) of a drawn alpha is the counter RNG's row at rng_counter + (k B + b) C + c, float4 q at sub = q:
    counter_noise over H B C consecutive counters, reshaped, is the tensor itself"""
    H, B, C, d = 3, 5, 7, 12
    seed, ctr = (0x1234 << 32) | 0x9876, (1 << 32) - 40
    al = ref.drawn_alpha(seed, ctr, H, B, C, d)
    assert al.shape == (H, B, C, d) and al.dtype == np.float32
    assert np.array_equal(al.reshape(-1, d), counter_rng.counter_noise(seed, ctr, H * B * C, d))
    for k, b, c in ((0, 0, 0), (1, 2, 3), (2, 4, 6), (0, 4, 6), (2, 0, 0)):
        row = counter_rng.counter_noise(seed, 0, 1, d, ctrs=np.array([ctr + (k * B + b) * C + c], dtype=np.uint64))[0]
        assert np.array_equal(al[k, b, c], row)
        for q in range(d // 4):
            w = counter_rng.rng4(np.uint64(ctr + (k * B + b) * C + c), np.uint32(q), seed)
            assert np.array_equal(al[k, b, c, 4 * q:4 * q + 4], counter_rng.u01(w).reshape(-1))
    for case in mc.CASES:
        c = mc.inputs(case)
        if c["drawn"]:
            _, B, H, C, d, _ = case
            assert np.array_equal(c["alpha"], ref.drawn_alpha(c["rng_seed"], c["rng_counter"], H, B, C, d))


@pytest.mark.parametrize("case", mc.CASES, ids=mc.case_id)
def test_plain_float32_yardstick(case):
    """What numpy's float32 evaluation of the same expressions loses: its scores stay within the margin the picks are
    judged by, its picks pass the same judgement, and its outputs at its own picks are within the forward bound."""
    fam, B, H, C, d, n_items = case
    c, r = mc.inputs(case), mc.reference(case)
    s32, m32 = ref.f32_scores(c["tables"], c["u"], c["pos"], c["neg"], c["alpha"])
    err = np.abs(s32.astype(np.float64) - r["s"]).max(axis=2)
    worst = float((err / np.maximum(r["margin"], 1e-300)).max()) if fam != "zero_user" else 0.0
    pick = np.argmax(s32, axis=2)
    outside, wrong = mc.judge_pick(case, pick)
    kept = m32[np.arange(H)[:, None], np.arange(B)[None, :], pick]
    neg_out = kept.sum(axis=0, dtype=np.float32) / np.float32(H)
    _, want_neg = ref.outputs(c["tables"], c["pos"], c["neg"], c["alpha"], pick)
    e_out = mc.rel_err(neg_out, want_neg)
    print(f"{mc.case_id(case)}: float32 score error / margin {worst:.3f}, rows outside {outside}, wrong {wrong}, "
          f"neg_out error {e_out:.2e}")
    assert worst <= 1.0 and outside == 0 and wrong == 0
    assert e_out < mc.FWD_BOUND


def test_route_conf_key_and_supported_shapes(monkeypatch):
    import os
    from selfrec_amd import _lib, ops
    from selfrec_amd.model.graph import MixGCF as M
    from selfrec_amd.util.conf import ModelConf
    monkeypatch.delenv("SRH_MIXGCF_MIXUP", raising=False)
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    conf = ModelConf(os.path.join(repo, "conf", "MixGCF.yaml"))
    assert conf.contain("engine.mixup") and M.mixup_route(conf) == "hip" and M.mixup_route(None) == "hip"
    assert M.mixup_route(ModelConf({"engine.mixup": " Torch "})) == "torch"
    monkeypatch.setenv("SRH_MIXGCF_MIXUP", "torch")
    assert M.mixup_route(conf) == "torch"
    monkeypatch.setenv("SRH_MIXGCF_MIXUP", "triton")
    with pytest.raises(ValueError):
        M.mixup_route(conf)
    assert ops.MIXUP_MAX_HOPS == 8
    for d, h, c, ok in ((64, 4, 64, True), (4, 1, 1, True), (256, 8, 1000, True), (60, 3, 5, True), (6, 4, 64, False),
                        (260, 4, 64, False), (0, 4, 64, False), (64, 9, 64, False), (64, 0, 64, False), (64, 4, 0, False)):
        assert ops.mixup_supported(d, h, c) is ok, (d, h, c)
    # the library's view of the same envelope, as far as it answers without a device: the workspace question
    lib = _lib.load()
    assert lib.srh_mixup_bwd_ws_bytes(2048, 4) >= 4 * 2 * 2048 * 4 and lib.srh_mixup_bwd_ws_bytes(2048, 4) % 256 == 0
    assert lib.srh_mixup_bwd_ws_bytes(0, 4) == 0 and lib.srh_mixup_bwd_ws_bytes(5, 9) == 0 and lib.srh_mixup_bwd_ws_bytes(5, 0) == 0
    import ctypes as C
    assert C.sizeof(_lib.MixupArgs) == 3 * 8 * 8 + 2 * 8 + 2 * 8 + 3 * 4 + 4 + 2 * 8
    header = open(os.path.join(repo, "include", "selfrec_hip.h")).read()
    assert "(a-21) MixGCF" in header and "#define SRH_MIXUP_MAX_HOPS 8" in header
