"""BERT4Rec without a GPU: the float64 restatement (tests/bert4rec_ref.py) against the reference-run golden
(tests/golden/bert4rec.npz, make_golden_bert4rec.py) -- which pins the restatement the GPU tests use to the reference --,
the mirror's item_mask_for_bert stream, the CPU-routed mirror model against the golden's steps, predict() and test(), the
launcher, the conf and the new entry points, and the admissibility of the table-CE inputs of the GPU tests.

Bounds: outputs and losses <= 1e-5, gradients <= 1e-4, each of its tensor's largest magnitude;
parameters after an Adam step within lr / 2."""
import json
import os
import random
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import bert4rec_ref
from tests.test_shapes_cpu import GOLDEN

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("srh_seq_attn_full_fwd_f32", "srh_seq_attn_full_bwd_f32", "srh_table_ce_ws_bytes", "srh_table_ce_fwd_bwd")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "bert4rec.npz")), json.load(open(os.path.join(GOLDEN, "bert4rec_meta.json")))


def make_model(meta, heads, tmp_path, monkeypatch, **engine):
    from selfrec_amd.model.sequential.BERT4Rec import BERT4Rec
    from selfrec_amd.util.conf import ModelConf
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("SRH_SASREC_ATTN", raising=False)
    monkeypatch.delenv("SRH_BERT4REC_CE", raising=False)
    c = meta["conf"]
    conf = {"model": {"name": "BERT4Rec", "type": "sequential"}, "item.ranking.topN": c["topN"], "embedding.size": c["emb"],
            "max.epoch": 1, "batch.size": c["batch"], "learning.rate": c["lr"], "reg.lambda": c["reg"],
            "output": "./results/", "training.set": "x", "test.set": "y", "max.len": c["max_len"],
            "BERT4Rec": {"n_blocks": c["n_blocks"], "drop_rate": c["drop_rate"], "n_heads": heads,
                         "mask_rate": c["mask_rate"]}}
    for key, value in engine.items():
        conf[f"engine.{key}"] = value
    return BERT4Rec(ModelConf(conf), {k: list(v) for k, v in meta["train"].items()},
                    {k: list(v) for k, v in meta["test"].items()})


def check_step0_grads(gd, heads, grads):
    for name, g in grads.items():
        g = np.asarray(g, dtype=np.float64).reshape(-1)
        want_g = gd[f"h{heads}_grad0_{name}_val"].astype(np.float64)
        err = np.abs(g[gd[f"sample_{name}"]] - want_g).max()
        assert err <= 1e-4 * np.abs(want_g).max() + 1e-12, (name, err)
        assert abs(g.sum() - gd[f"h{heads}_grad0_{name}_sum"][0]) <= 1e-4 * np.abs(g).sum() + 1e-12, name


@pytest.mark.parametrize("heads", [1, 2])
def test_float64_restatement_reproduces_the_golden(golden, heads):
    """three Adam steps in float64 from the golden's initial parameters on its batches: the three losses <= 1e-5
    relative, step 0's gradients <= 1e-4 of each tensor's max"""
    gd, meta = golden
    c = meta["conf"]
    params = {n: torch.from_numpy(gd[f"init_{n}"]).double().requires_grad_(True) for n in meta["param_names"]}
    opt = torch.optim.Adam(list(params.values()), lr=c["lr"])
    for s in range(3):
        aug, pos, masked, labels = (gd[f"train{s}_{k}"] for k in ("aug", "pos", "masked", "labels"))
        assert labels.shape[0] == meta["n_masked"][s] == int(masked.sum())
        loss = bert4rec_ref.batch_loss(params, aug, pos, masked, labels, c["n_blocks"], heads, c["reg"])
        want = gd[f"h{heads}_loss"][s]
        assert abs(float(loss.detach()) - want) <= 1e-5 * abs(want), (s, float(loss.detach()), want)
        opt.zero_grad()
        loss.backward()
        if s == 0:
            check_step0_grads(gd, heads, {n: p.grad.numpy() for n, p in params.items()})
        opt.step()


def test_golden_pairs_rows_and_labels_in_different_orders(golden):
    """quirk 3: the labels are in random.sample's order, the rows in ascending position order -- on every recorded batch
    the ids under the mask, read in row order, are NOT the label vector (the same multiset, though)"""
    gd, meta = golden
    for b in range(meta["n_train_batches"]):
        seq, masked, labels, aug = (gd[f"train{b}_{k}"] for k in ("seq", "masked", "labels", "aug"))
        in_row_order = seq[masked > 0]
        assert not np.array_equal(in_row_order, labels)
        assert sorted(in_row_order.tolist()) == sorted(labels.tolist())
        assert (aug[masked > 0] == meta["item_num"] + 1).all() and np.array_equal(aug[masked == 0], seq[masked == 0])


def test_item_mask_stream_equals_the_golden(golden):
    from selfrec_amd.model.sequential.BERT4Rec import item_mask_for_bert
    from selfrec_amd.util.sampler import next_batch_sequence
    from tests.test_sasrec_cpu import make_data
    gd, meta = golden
    data = make_data(meta)
    c = meta["conf"]
    assert data.item_num == meta["item_num"]
    random.seed(meta["sampler_seed"])
    n = 0
    for n, (seq, pos, _y, _neg, ln) in enumerate(next_batch_sequence(data, c["batch"], max_len=c["max_len"])):
        aug, masked, labels = item_mask_for_bert(seq, ln, c["mask_rate"], data.item_num + 1)
        for key, got in zip(("seq", "pos", "len", "aug", "masked", "labels"), (seq, pos, ln, aug, masked, labels)):
            assert np.array_equal(np.asarray(got), gd[f"train{n}_{key}"]), (n, key)
    assert n + 1 == meta["n_train_batches"]
    assert np.array_equal(np.asarray(random.getstate()[1], dtype=np.int64), gd["rng_after_epoch"])


@pytest.mark.parametrize("heads", [1, 2])
def test_cpu_routed_mirror_model_reproduces_the_golden(golden, heads, tmp_path, monkeypatch):
    from selfrec_amd.util.evaluation import ranking_evaluation
    from selfrec_amd.util.loss_torch import l2_reg_loss
    gd, meta = golden
    c = meta["conf"]
    torch.manual_seed(meta["torch_seed"])
    model = make_model(meta, heads, tmp_path, monkeypatch)
    net = model.model
    params = dict(net.named_parameters())
    assert list(params) == meta["param_names"]
    for name, p in params.items():
        assert np.array_equal(p.detach().numpy(), gd[f"init_{name}"]), name
    assert net.item_emb.shape == (meta["item_num"] + 2, c["emb"]) and net.pos_emb.shape == (c["max_len"] + 2, c["emb"])
    assert net.last_layer_norm.eps == 1e-8 and isinstance(net.forward_layers[0].pwff[1], torch.nn.GELU)
    assert not net.uses_kernel(c["max_len"], on_device=False) and not model.uses_ce_kernel(on_device=False)
    optimizer = torch.optim.Adam(net.parameters(), lr=model.lRate)
    lr = model.lRate
    for s in range(3):
        aug, pos, masked, labels = (gd[f"train{s}_{k}"] for k in ("aug", "pos", "masked", "labels"))
        net.train()
        loss = model.calculate_loss(net.forward(aug, pos), masked, labels) + l2_reg_loss(model.reg, net.item_emb)
        want = gd[f"h{heads}_loss"][s]
        assert abs(float(loss.detach()) - want) <= 1e-5 * abs(want), (s, float(loss.detach()), want)
        optimizer.zero_grad()
        loss.backward()
        if s == 0:
            check_step0_grads(gd, heads, {n: p.grad.numpy() for n, p in params.items()})
        optimizer.step()
        for name, p in params.items():
            v = p.detach().reshape(-1).numpy()
            if s < 2:
                assert np.abs(v[gd[f"sample_{name}"]] - gd[f"h{heads}_step{s}_{name}_val"]).max() <= lr / 2, (s, name)
            else:
                assert np.abs(v - gd[f"h{heads}_final_{name}"].reshape(-1)).max() <= lr / 2, (s, name)
    # predict() and test() on the golden's final parameters
    with torch.no_grad():
        for name, p in params.items():
            p.copy_(torch.from_numpy(gd[f"h{heads}_final_{name}"]))
    net.eval()
    full_rows = 0
    for b in range(meta["n_test_batches"]):
        seq, pos, ln = (gd[f"test{b}_{k}"].astype(np.int64) for k in ("seq", "pos", "len"))
        before = seq.copy()
        hidden = model.last_hidden(seq, pos, ln)
        assert np.array_equal(seq, before)                                 # last_hidden edits a copy,
        score = model.predict(seq, pos, ln)                                # predict the arrays themselves
        assert np.array_equal(seq, gd[f"h{heads}_pred{b}_seq"]) and np.array_equal(pos, gd[f"h{heads}_pred{b}_pos"])
        want = gd[f"h{heads}_pred{b}_score"]
        assert score.shape == want.shape == (len(ln), meta["item_num"] + 2)
        assert np.abs(score - want).max() <= 1e-5 * np.abs(want).max()
        assert np.abs(hidden.numpy() @ net.item_emb.detach().numpy().T - want).max() <= 1e-5 * np.abs(want).max()
        full_rows += int((ln == c["max_len"]).sum())
        short = np.flatnonzero(ln < c["max_len"])
        assert (seq[short, ln[short]] == meta["item_num"] + 1).all() and (pos[short, ln[short]] == ln[short] + 1).all()
    assert full_rows == meta["n_full_length_test_rows"] > 0
    rec = model.test()
    d = model.data
    names = [n for n, _ in d.original_seq]
    want_ids, want_sc = gd[f"h{heads}_rec_ids"], gd[f"h{heads}_rec_scores"]
    scale = np.abs(want_sc).max()
    for r, n in enumerate(names):
        keep = want_ids[r] >= 0
        assert [d.item[it] for it, _ in rec[n]] == want_ids[r][keep].tolist(), n
        assert np.abs(np.asarray([sc for _, sc in rec[n]]) - want_sc[r][keep]).max() <= 1e-5 * scale, n
    assert any((want_ids[r] < 0).any() for r in range(len(names)))         # rows 0 / item_num + 1 did leave some list
    ev = meta[f"h{heads}_evaluation"]
    assert ranking_evaluation(d.test_set, rec, model.topN) == ev["topN"]
    assert ranking_evaluation(d.test_set, rec, [model.max_N]) == ev["maxN"]


def test_restatement_attention_sees_every_position_and_replays_masks():
    g = torch.Generator().manual_seed(0)
    q, k, v = (torch.randn(2, 7, 64, generator=g, dtype=torch.float64) for _ in range(3))
    base = bert4rec_ref.attention(q, k, v, 2)
    v2 = v.clone()
    v2[:, 6] += 1.0                                                       # the last position reaches every row
    assert (bert4rec_ref.attention(q, k, v2, 2) - base).abs().min() > 0
    keep = np.ones((2, 2, 7, 7), dtype=bool)
    assert torch.allclose(bert4rec_ref.attention(q, k, v, 2, keep, 0.2), base / 0.8)
    from selfrec_amd.model.sequential.SASRec import torch_causal_attention
    assert torch.allclose(torch_causal_attention(q, k, v, 2, causal=False), base)
    assert not torch.allclose(torch_causal_attention(q, k, v, 2), base)
    drawn = bert4rec_ref.attn_keep_drawn(123, 50, 2, 2, 7, 0.2)
    assert drawn.shape == (2, 2, 7, 7) and drawn[..., np.triu_indices(7, 1)[0], np.triu_indices(7, 1)[1]].any()


def test_routes_launcher_and_conf(monkeypatch):
    from selfrec_amd import main
    from selfrec_amd.model.sequential import BERT4Rec as mod
    from selfrec_amd.util.conf import ModelConf
    assert "BERT4Rec" in main.MODELS
    for name in ("train", "calculate_loss", "predict", "test", "fast_evaluation", "item_mask_for_bert"):
        assert callable(getattr(mod.BERT4Rec, name)), name
    conf = ModelConf(os.path.join(REPO, "conf", "BERT4Rec.yaml"))
    assert set(conf.config) == {"training.set", "test.set", "model", "item.ranking.topN", "embedding.size", "max.epoch",
                                "batch.size", "learning.rate", "reg.lambda", "max.len", "BERT4Rec", "output"}
    assert conf["model"] == {"name": "BERT4Rec", "type": "sequential"}
    assert set(conf["BERT4Rec"]) == {"n_blocks", "drop_rate", "n_heads", "mask_rate"} and int(conf["max.len"]) == 50
    monkeypatch.delenv("SRH_BERT4REC_CE", raising=False)
    assert mod.ce_route(ModelConf({})) == 'hip'
    assert mod.ce_route(ModelConf({"engine.ce": "torch"})) == 'torch'
    monkeypatch.setenv("SRH_BERT4REC_CE", "torch")
    assert mod.ce_route(ModelConf({"engine.ce": "hip"})) == 'torch'
    monkeypatch.setenv("SRH_BERT4REC_CE", "eager")
    with pytest.raises(ValueError):
        mod.ce_route(None)
    net = mod.BERT_Encoder(types.SimpleNamespace(item_num=30), 64, 50, 1, 1, 0.0)
    assert net.uses_kernel(50) and net.uses_kernel(64) and not net.uses_kernel(65)      # max.len > 64: torch's route
    net.attention = 'torch'
    assert not net.uses_kernel(50)


def test_entry_points_are_declared_and_bound():
    from selfrec_amd import _lib, ops
    header = open(os.path.join(REPO, "include", "selfrec_hip.h")).read()
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert f"{name}(" in header, name
    for name in ("seq_attn_full_fwd", "seq_attn_full_bwd", "SeqAttnFullFn", "table_ce_fwd_bwd", "TableCeFn"):
        assert getattr(ops, name) and name in ops.__all__, name
    assert "(a-17)" in header and f"#define SRH_ABI_VERSION {_lib.ABI_VERSION}" in header and _lib.ABI_VERSION == 31
    if os.path.exists(_lib.LIB_PATH):                                    # built: every new symbol is exported
        lib = _lib.load()
        assert all(hasattr(lib, name) for name in SYMBOLS)
    cpu = torch.zeros(4, 8, 64)
    with pytest.raises(ops.SelfrecHipError):                             # device ops refuse CPU tensors
        ops.seq_attn_full_fwd(cpu, cpu, cpu, 1)
    with pytest.raises(ops.SelfrecHipError):
        ops.table_ce_fwd_bwd(cpu[0], cpu[1], torch.zeros(8, dtype=torch.int32))


@pytest.mark.parametrize("family", bert4rec_ref.CE_FAMILIES)
@pytest.mark.parametrize("shape", bert4rec_ref.CE_SHAPES, ids=lambda s: "M%d_N%d_d%d" % s)
def test_table_ce_cases_are_admissible_in_float32(shape, family):
    """float32 torch on the CPU meets the bounds on every table-CE case the GPU tests use: a case that float32 arithmetic
    alone cannot serve would test the number format, not the kernel"""
    M, N, d = shape
    h, table, labels = bert4rec_ref.ce_case(shape, family)
    assert (labels.min() == 0 and labels.max() == N - 1) if M >= 2 else int(labels[0]) in (0, N - 1)   # one row, one label
    if M >= 5:
        assert len(set(labels.tolist())) < M
    want_loss, want_gh, want_gt = bert4rec_ref.table_ce_grads(h, table, labels)
    logits = h.double() @ table.double().T
    if family == "extreme":
        assert logits.max() > 100.0                                       # exp overflows in float32 unshifted
        if M >= 2:
            assert (logits.max(dim=1).values < -100.0).any()              # ... and underflows to a zero row sum
        top = logits.argmax(dim=1)
        assert (top == labels).any() or M == 1
        assert (logits.max(dim=1).values - logits[torch.arange(M), labels]).max() > 50.0
    h32, t32 = h.clone().requires_grad_(True), table.clone().requires_grad_(True)
    loss = F.cross_entropy(h32 @ t32.t(), labels, reduction='sum')
    loss.backward()
    errs = dict(loss=abs(float(loss) - want_loss) / abs(want_loss),
                gh=float((h32.grad.double() - want_gh).abs().max() / want_gh.abs().max()),
                gt=float((t32.grad.double() - want_gt).abs().max() / want_gt.abs().max()))
    print(shape, family, errs)
    assert errs["loss"] <= 1e-5 and errs["gh"] <= 1e-4 and errs["gt"] <= 1e-4, errs
