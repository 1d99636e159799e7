"""SASRec without a GPU: the Sequence mirror and both samplers against the reference-run golden (tests/golden/sasrec.npz,
make_golden_sasrec.py), the float64 restatement (tests/sasrec_ref.py) against the golden's losses and gradients -- which
pins the restatement the GPU tests use to the reference --, the model module's names and initial weights, the conf,
the launcher's list, the synthetic writer and the new entry points."""
import json
import os
import random
import types

import numpy as np
import pytest
import torch

from tests import sasrec_ref
from tests.test_shapes_cpu import GOLDEN

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("srh_seq_attn_fwd_f32", "srh_seq_attn_bwd_f32", "srh_seq_bce_ws_bytes", "srh_seq_bce_fwd_bwd")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "sasrec.npz")), json.load(open(os.path.join(GOLDEN, "sasrec_meta.json")))


def make_data(meta):
    from selfrec_amd.data.sequence import Sequence
    return Sequence({}, {k: list(v) for k, v in meta["train"].items()}, {k: list(v) for k, v in meta["test"].items()})


def test_sequence_mirror_equals_the_golden_maps(golden):
    gd, meta = golden
    data = make_data(meta)
    assert data.raw_seq_num == meta["raw_seq_num"] and data.item_num == meta["item_num"]
    assert [n for n, _ in data.original_seq] == gd["seq_names"].tolist()
    flat, ptr = gd["seq_flat"], gd["seq_ptr"]
    assert [ids for _, ids in data.original_seq] == [flat[ptr[k]:ptr[k + 1]].tolist() for k in range(len(ptr) - 1)]
    assert [data.id2item[i] for i in range(1, data.item_num + 1)] == gd["item_names"].tolist()
    assert 0 not in data.id2item and min(data.item.values()) == 1
    assert data.seq == meta["seq_ids"] and all(data.id2seq[v] == k for k, v in data.seq.items())
    assert {k: dict(v) for k, v in data.test_set.items()} == meta["test_set"]
    assert "s_unseen" not in data.test_set and "s_unseen" in meta["test"]           # absent from training
    dropped = [k for k, v in meta["train"].items() if len(v) < 2]
    assert dropped and all(k not in data.seq and k not in data.test_set for k in dropped)
    assert data.get_item_id(gd["item_names"][0]) == 1 and data.get_seq_id(gd["seq_names"][3]) == 3
    assert data.get_item_id("nope") is None and data.get_seq_id("nope") is None


def test_both_samplers_equal_the_golden_batches_and_leave_the_same_rng_state(golden):
    from selfrec_amd.util.sampler import next_batch_sequence, next_batch_sequence_for_test
    gd, meta = golden
    data = make_data(meta)
    L, bs = meta["conf"]["max_len"], meta["conf"]["batch"]
    assert max(len(ids) for _, ids in data.original_seq) > L                          # the truncation rule is exercised
    random.seed(meta["sampler_seed"])
    batches = list(next_batch_sequence(data, bs, max_len=L))
    state = random.getstate()
    assert len(batches) == meta["n_train_batches"]
    for b, batch in enumerate(batches):
        for key, got in zip(("seq", "pos", "y", "neg", "len"), batch):
            assert np.array_equal(np.asarray(got), gd[f"train{b}_{key}"]), (b, key)
    assert np.array_equal(np.asarray(state[1], dtype=np.int64), gd["rng_after_epoch"])
    tests = list(next_batch_sequence_for_test(data, bs, max_len=L))
    assert len(tests) == meta["n_test_batches"] and random.getstate() == state       # the test sampler draws nothing
    for b, batch in enumerate(tests):
        for key, got in zip(("seq", "pos", "len"), batch):
            assert np.array_equal(np.asarray(got), gd[f"test{b}_{key}"]), (b, key)
    # a longer sequence: training keeps max_len - 1 inputs, testing the last max_len items
    long_rows = [r for r, (_, ids) in enumerate(data.original_seq) if len(ids) > L]
    r = long_rows[0]
    ids = data.original_seq[r][1]
    assert tests[r // bs][0][r % bs].tolist() == ids[-L:] and tests[r // bs][2][r % bs] == L


@pytest.mark.parametrize("heads", [1, 2])
def test_float64_restatement_reproduces_the_golden(golden, heads):
    """three Adam steps in float64 from the golden's initial parameters on its batches: the three losses <= 1e-5
    relative, step 0's gradients <= 1e-4 of each tensor's max"""
    gd, meta = golden
    c = meta["conf"]
    params = {n: torch.from_numpy(gd[f"init_{n}"]).double().requires_grad_(True) for n in meta["param_names"]}
    opt = torch.optim.Adam(list(params.values()), lr=c["lr"])
    for s in range(3):
        seq, pos, y, neg = (gd[f"train{s}_{k}"] for k in ("seq", "pos", "y", "neg"))
        loss = sasrec_ref.batch_loss(params, seq, pos, y, neg, c["n_blocks"], heads, c["reg"])
        want = gd[f"h{heads}_loss"][s]
        assert abs(float(loss.detach()) - want) <= 1e-5 * abs(want), (s, float(loss.detach()), want)
        opt.zero_grad()
        loss.backward()
        if s == 0:
            for name, p in params.items():
                g = p.grad.reshape(-1).numpy()
                want_g = gd[f"h{heads}_grad0_{name}_val"].astype(np.float64)
                err = np.abs(g[gd[f"sample_{name}"]] - want_g).max()
                assert err <= 1e-4 * np.abs(want_g).max() + 1e-12, (name, err)
                assert abs(g.sum() - gd[f"h{heads}_grad0_{name}_sum"][0]) <= 1e-4 * np.abs(g).sum() + 1e-12, name
        opt.step()


def test_restatement_attention_is_causal_and_replays_masks():
    g = torch.Generator().manual_seed(0)
    q, k, v = (torch.randn(2, 7, 64, generator=g, dtype=torch.float64) for _ in range(3))
    base = sasrec_ref.attention(q, k, v, 2)
    k2, v2 = k.clone(), v.clone()
    k2[:, 5:], v2[:, 5:] = 9.0, -9.0                                  # the future of rows < 5
    assert torch.equal(sasrec_ref.attention(q, k2, v2, 2)[:, :5], base[:, :5])
    assert torch.allclose(base[:, 0], v[:, 0])                          # row 0 sees only itself
    keep = np.ones((2, 2, 7, 7), dtype=bool)
    assert torch.allclose(sasrec_ref.attention(q, k, v, 2, keep, 0.2), base / 0.8)
    drawn = sasrec_ref.attn_keep_drawn(123, 50, 2, 2, 7, 0.2)
    again = sasrec_ref.attn_keep_drawn(123, 50 + 2 * 2 * 7, 2, 2, 7, 0.2)
    both = sasrec_ref.attn_keep_drawn(123, 50, 4, 2, 7, 0.2)
    assert np.array_equal(both[:2], drawn) and np.array_equal(both[2:], again) and not np.array_equal(drawn, again)


def test_model_module_keeps_the_reference_names_and_initial_weights(golden):
    from selfrec_amd import main
    from selfrec_amd.model.sequential import SASRec as mod
    gd, meta = golden
    assert "SASRec" in main.MODELS
    for name in ("train", "calculate_loss", "predict", "test", "fast_evaluation"):
        assert callable(getattr(mod.SASRec, name)), name
    c = meta["conf"]
    torch.manual_seed(meta["torch_seed"])
    net = mod.SASRec_Model(types.SimpleNamespace(item_num=meta["item_num"]), c["emb"], c["max_len"], c["n_blocks"], 2,
                           c["drop_rate"])
    assert list(dict(net.named_parameters())) == meta["param_names"]
    for name, p in net.named_parameters():
        assert np.array_equal(p.detach().numpy(), gd[f"init_{name}"]), name
    assert net.item_emb.shape == (meta["item_num"] + 1, c["emb"]) and net.pos_emb.shape == (c["max_len"] + 1, c["emb"])
    assert net.last_layer_norm.eps == 1e-8 and net.attention_layer_norms[0].eps == 1e-8
    assert net.uses_kernel(12) and net.uses_kernel(64) and not net.uses_kernel(65)
    assert not net.uses_kernel(12, on_device=False)                    # a CPU model takes torch's expression
    out = net(gd["train0_seq"], gd["train0_pos"])                        # default route, on the CPU: no kernel call
    assert out.shape == (gd["train0_seq"].shape[0], c["max_len"], c["emb"]) and torch.isfinite(out).all()
    net.attention = 'torch'
    assert not net.uses_kernel(12)


def test_attention_route_switch(monkeypatch):
    from selfrec_amd.model.sequential.SASRec import attention_route
    from selfrec_amd.util.conf import ModelConf
    monkeypatch.delenv("SRH_SASREC_ATTN", raising=False)
    assert attention_route(ModelConf({})) == 'hip'
    assert attention_route(ModelConf({"engine.attention": "torch"})) == 'torch'
    monkeypatch.setenv("SRH_SASREC_ATTN", "torch")
    assert attention_route(ModelConf({"engine.attention": "hip"})) == 'torch'
    monkeypatch.setenv("SRH_SASREC_ATTN", "eager")
    with pytest.raises(ValueError):
        attention_route(None)


def test_conf_has_the_reference_keys():
    from selfrec_amd.util.conf import ModelConf
    conf = ModelConf(os.path.join(REPO, "conf", "SASRec.yaml"))
    assert set(conf.config) == {"training.set", "test.set", "model", "item.ranking.topN", "embedding.size", "max.epoch",
                                "batch.size", "learning.rate", "reg.lambda", "max.len", "SASRec", "output"}
    assert conf["model"] == {"name": "SASRec", "type": "sequential"}
    assert set(conf["SASRec"]) == {"n_blocks", "drop_rate", "n_heads"} and int(conf["max.len"]) == 50


def test_synthetic_writer_round_trips_through_the_loader(tmp_path):
    from selfrec_amd import synth
    from selfrec_amd.data.loader import FileIO
    from selfrec_amd.data.sequence import Sequence
    train, test = synth.make_sequence_dataset("tiny-seq")
    synth.write_sequences(str(tmp_path / "train.txt"), train)
    synth.write_sequences(str(tmp_path / "test.txt"), test)
    assert FileIO.load_data_set(str(tmp_path / "train.txt"), 'sequential') == train
    assert FileIO.load_data_set(str(tmp_path / "test.txt"), 'sequential') == test
    n_seq, n_items, _ = synth.SEQ_SHAPES["tiny-seq"]
    data = Sequence({}, train, test)
    assert data.raw_seq_num == n_seq and len(data.test_set) == n_seq and data.item_num <= n_items
    assert all(len(v) == 1 for v in test.values())
    again, _ = synth.make_sequence_dataset("tiny-seq")
    assert again == train                                                # seeded


def test_main_writes_a_sequence_set_for_a_sequential_conf(tmp_path, monkeypatch):
    from selfrec_amd import main, synth
    conf = tmp_path / "SASRec.yaml"
    text = open(os.path.join(REPO, "conf", "SASRec.yaml")).read()
    conf.write_text(text.replace("./dataset/beauty-seq-synth", str(tmp_path / "data")))
    ran = []
    monkeypatch.setattr(main, "SELFRec", lambda c: types.SimpleNamespace(execute=lambda: ran.append(c)))
    main.main(["SASRec", "--conf", str(conf), "--synthetic", "tiny-seq"])
    assert ran and ran[0]["model"]["type"] == "sequential"
    first = open(tmp_path / "data" / "train.txt").readline()
    assert ":" in first and len(first.split(":")[1].split()) >= 2
    assert synth.SEQ_SHAPES["beauty-seq"][0] > 20000


def test_entry_points_are_declared_and_bound():
    from selfrec_amd import _lib, ops
    header = open(os.path.join(REPO, "include", "selfrec_hip.h")).read()
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert f"{name}(" in header, name
    for name in ("seq_attn_fwd", "seq_attn_bwd", "SeqAttnFn", "seq_bce_fwd_bwd", "SeqBceFn", "GatherRowsFn",
                 "seq_attn_supported"):
        assert getattr(ops, name) and name in ops.__all__, name
    assert "seqrec.hip" in open(os.path.join(REPO, "selfrec_amd", "csrc", "Makefile")).read()
    assert f"#define SRH_ABI_VERSION {_lib.ABI_VERSION}" in header and _lib.ABI_VERSION == 31
    if os.path.exists(_lib.LIB_PATH):                                    # built: every new symbol is exported
        lib = _lib.load()
        assert all(hasattr(lib, name) for name in SYMBOLS)
    assert ops.seq_attn_supported(1, 1, 64) and ops.seq_attn_supported(64, 2, 64) and ops.seq_attn_supported(33, 4, 32)
    assert not ops.seq_attn_supported(65, 1, 64) and not ops.seq_attn_supported(50, 1, 48)
    assert not ops.seq_attn_supported(50, 4, 64)
