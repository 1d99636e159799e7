"""SSL4Rec without a GPU: the model module keeps the reference's names and is listed, conf/SSL4Rec.yaml carries every key
the model reads, loss_torch has batch_softmax_loss with the reference's signature, the new entry points are declared
and bound, the dropout-mask counter layout, and a float64 restatement of the step (tests/ssl4rec_ref.py) against the
reference-run golden (tests/golden/ssl4rec.npz, make_golden_ssl4rec.py)."""
import inspect
import json
import os
import types

import numpy as np
import torch

from tests import counter_rng, ssl4rec_ref
from tests.test_shapes_cpu import GOLDEN

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("srh_tower_fwd_f32", "srh_tower_bwd_ws_bytes", "srh_tower_bwd_f32", "srh_rows_segment_sum_f32",
           "srh_batch_softmax_ws_bytes", "srh_batch_softmax_fwd_bwd")


def _golden():
    return np.load(os.path.join(GOLDEN, "ssl4rec.npz")), json.load(open(os.path.join(GOLDEN, "ssl4rec_meta.json")))


def test_model_module_keeps_the_reference_names_and_is_listed():
    from selfrec_amd import main
    from selfrec_amd.model.graph import SSL4Rec as mod
    assert "SSL4Rec" in main.MODELS
    for name in ("train", "save", "predict"):
        assert callable(getattr(mod.SSL4Rec, name)), name
    for name in ("forward", "item_encoding", "cal_cl_loss"):
        assert callable(getattr(mod.DNN_Encoder, name)), name
    data = types.SimpleNamespace(user_num=5, item_num=7)
    enc = mod.DNN_Encoder(data, 64, 0.1, 0.07)
    assert list(dict(enc.named_parameters())) == [
        "initial_user_emb", "initial_item_emb", "user_tower.0.weight", "user_tower.0.bias", "user_tower.2.weight",
        "user_tower.2.bias",
        "item_tower.0.weight", "item_tower.0.bias", "item_tower.2.weight", "item_tower.2.bias"]
    assert isinstance(enc.dropout, torch.nn.Dropout) and enc.dropout.p == 0.1


def test_initial_weights_follow_the_reference_rng_order():
    from selfrec_amd.model.graph import SSL4Rec as mod
    gd, meta = _golden()
    torch.manual_seed(meta["torch_seed"])
    data = types.SimpleNamespace(user_num=gd["init_user_emb"].shape[0], item_num=gd["init_item_emb"].shape[0])
    enc = mod.DNN_Encoder(data, 64, 0.1, 0.07)
    assert np.array_equal(enc.initial_user_emb.detach().numpy(), gd["init_user_emb"])
    assert np.array_equal(enc.initial_item_emb.detach().numpy(), gd["init_item_emb"])


def test_conf_has_every_key_the_model_reads():
    from selfrec_amd.util.conf import ModelConf
    conf = ModelConf(os.path.join(REPO, "conf", "SSL4Rec.yaml"))
    for key in ("training.set", "test.set", "model", "item.ranking.topN", "embedding.size", "max.epoch", "batch.size",
                "learning.rate", "reg.lambda", "output"):
        assert key in conf.config, key
    assert conf["model"]["name"] == "SSL4Rec"
    assert {k: float(v) for k, v in conf["SSL4Rec"].items()} == {"tau": 0.07, "alpha": 0.1, "drop": 0.1}


def test_loss_torch_has_batch_softmax_loss():
    from selfrec_amd.util import loss_torch
    assert list(inspect.signature(loss_torch.batch_softmax_loss).parameters) == ["user_emb", "item_emb", "temperature"]
    g = torch.Generator().manual_seed(0)
    u, v = torch.randn(33, 64, generator=g), torch.randn(33, 64, generator=g)
    got = loss_torch.batch_softmax_loss(u.double(), v.double(), 0.07)          # CPU: the reference's expression
    assert abs(float(got) - float(ssl4rec_ref.batch_softmax(u.double(), v.double(), 0.07))) < 1e-12


def test_entry_points_are_declared_and_bound():
    from selfrec_amd import _lib, ops
    header = open(os.path.join(REPO, "include", "selfrec_hip.h")).read()
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert f"{name}(" in header, name
    for name in ("tower_fwd", "tower_bwd", "scatter_plan", "rows_segment_sum", "batch_softmax_fwd_bwd", "TowerFn",
                 "BatchSoftmaxFn"):
        assert getattr(ops, name), name
    assert f"#define SRH_ABI_VERSION {_lib.ABI_VERSION}" in header and _lib.ABI_VERSION == 31


def test_dropout_mask_counter_layout():
    seed, ctr, B, p = 0x1234_5678_9ABC, 1000, 300, 0.1
    k1 = ssl4rec_ref.dropout_keep(seed, ctr, B, p)
    k2 = ssl4rec_ref.dropout_keep(seed, ctr + B, B, p)
    both = ssl4rec_ref.dropout_keep(seed, ctr, 2 * B, p)
    assert np.array_equal(both[:B], k1) and np.array_equal(both[B:], k2)     # one 2B-row draw = the two views
    assert not np.array_equal(k1, k2)
    assert abs(1.0 - k1.mean() - p) < 0.01                                   # ~p of the features dropped
    # column c is word c % 4 of float4 c // 4 at counter ctr + row
    w = counter_rng.rng4(np.uint64(ctr + 7), 5, seed)
    assert np.array_equal(k1[7, 20:24], counter_rng.u01(w) >= np.float32(p))


def test_scatter_plan_is_a_stable_sort():
    from selfrec_amd import ops
    ids = np.array([4, 1, 4, 0, 1, 4])
    order, start, row = (t.numpy() for t in ops.scatter_plan(ids, "cpu"))
    assert order.tolist() == [3, 1, 4, 0, 2, 5] and start.tolist() == [0, 1, 3, 6] and row.tolist() == [0, 1, 4]


def test_batch_softmax_gradient_is_the_weighted_infonce_gradient():
    g = torch.Generator().manual_seed(1)
    u = torch.randn(40, 16, generator=g, dtype=torch.float64)
    v = -u + 0.3 * torch.randn(40, 16, generator=g, dtype=torch.float64)      # p_bb far below 1e-5 on most rows
    u.requires_grad_(True)
    ssl4rec_ref.batch_softmax(u, v, 0.07).backward()
    un, vn = torch.nn.functional.normalize(u.detach(), dim=1), torch.nn.functional.normalize(v, dim=1)
    P = torch.softmax(un @ vn.T / 0.07, dim=1)
    p = P.diagonal()
    assert (p < 1e-7).any()
    w = p / (p + 1e-5)
    ds = w[:, None] * (P - torch.eye(40, dtype=torch.float64)) / (0.07 * 40)
    gn = ds @ vn
    nrm = u.detach().norm(dim=1, keepdim=True)
    want = (gn - un * (un * gn).sum(1, keepdim=True)) / nrm
    assert torch.allclose(u.grad, want, rtol=1e-9, atol=1e-14)


def test_float64_step_matches_the_reference_golden():
    """step 0 of the golden, restated in float64 from the initial weights and the recorded masks: the three losses and
    the sampled pre-Adam gradients"""
    from selfrec_amd.model.graph import SSL4Rec as mod
    gd, meta = _golden()
    torch.manual_seed(meta["torch_seed"])
    data = types.SimpleNamespace(user_num=gd["init_user_emb"].shape[0], item_num=gd["init_item_emb"].shape[0])
    enc = mod.DNN_Encoder(data, 64, meta["conf"]["drop"], meta["conf"]["tau"])
    params = {k: v.detach().double().clone().requires_grad_(True) for k, v in enc.named_parameters()}
    B = gd["batch0_i"].size
    keep = np.unpackbits(gd["step0_mask"], axis=-1)[..., :64].astype(bool)
    assert keep.shape == (2, B, 64) and not np.array_equal(keep[0], keep[1])
    rec, cl, total = ssl4rec_ref.step_losses(params, gd["batch0_q"], gd["batch0_i"], keep, meta["conf"], meta["reg"])
    for got, want in zip((rec, cl, total), gd["step0_loss"]):
        assert abs(float(got.detach()) - want) <= 1e-5 * abs(want), (float(got.detach()), want)
    total.backward()
    for name, p in params.items():
        gr = p.grad.reshape(-1).numpy()
        want = gd[f"grad0_{name}_val"].astype(np.float64)
        assert np.abs(gr[gd[f"sample_{name}"]] - want).max() <= 1e-4 * np.abs(want).max() + 1e-12, name
        assert abs(gr.sum() - gd[f"grad0_{name}_sum"][0]) <= 1e-4 * np.abs(gr).sum(), name
