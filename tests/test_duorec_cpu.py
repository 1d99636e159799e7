"""DuoRec without a GPU: the registry and the conf, the indexed sampler against next_batch_sequence, the same-target index
and the positive draws against the golden (tests/golden/duorec.npz, make_golden_duorec.py: the reference's own pieces
composed into DESIGN.md 4.29's step), and the CPU model on the golden's three Adam steps and its test() lists."""
import json
import os
import random

import numpy as np
import pytest
import torch

from tests.test_cl4srec_cpu import check_initial_parameters
from tests.test_shapes_cpu import GOLDEN

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTE_ENVS = ("SRH_SASREC_ATTN", "SRH_CL4SREC_VIEWS", "SRH_CL4SREC_EMBED", "SRH_DUOREC_DUO")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "duorec.npz")), json.load(open(os.path.join(GOLDEN, "duorec_meta.json")))


def make_model(meta, heads, tmp_path, monkeypatch, **over):
    from selfrec_amd.model.sequential.DuoRec import DuoRec
    from selfrec_amd.util.conf import ModelConf
    monkeypatch.chdir(tmp_path)
    for env in ROUTE_ENVS:
        monkeypatch.delenv(env, raising=False)
    c = meta["conf"]
    conf = {"model": {"name": "DuoRec", "type": "sequential"}, "item.ranking.topN": c["topN"], "embedding.size": c["emb"],
            "max.epoch": 1, "batch.size": c["batch"], "learning.rate": c["lr"], "reg.lambda": c["reg"], "output": "./results/",
            "training.set": "x", "test.set": "y", "max.len": c["max_len"],
            "DuoRec": {"n_blocks": c["n_blocks"], "drop_rate": over.get("drop_rate", c["drop_rate"]), "n_heads": heads,
                       "cl_rate": c["cl_rate"]}}
    for key in ("views", "embed", "attention", "duo"):
        if key in over:
            conf[f"engine.{key}"] = over[key]
    return DuoRec(ModelConf(conf), {k: list(v) for k, v in meta["train"].items()},
                  {k: list(v) for k, v in meta["test"].items()})


def golden_step(gd, b):
    batch = tuple(gd[f"train{b}_{k}"] for k in ("seq", "pos", "y", "neg", "len", "rows"))
    return batch, tuple(gd[f"pos{b}_{k}"] for k in ("seq", "pos", "len"))


def replay_three_steps(gd, meta, model, heads, device="cpu"):
    """the golden's three Adam steps through model.step_losses: losses <= 1e-5, step 0's gradients <= 1e-4 of each tensor's
    max, parameters within lr / 2"""
    k = f"h{heads}"
    net = model.model
    params = dict(net.named_parameters())
    optimizer = torch.optim.Adam(net.parameters(), lr=model.lRate)
    net.train()
    for s in range(3):
        (seq, pos, y, neg, seq_len, _), positives = golden_step(gd, s)
        loss, rec, cl = model.step_losses(seq, pos, y, neg, seq_len, positives)
        for got, key in ((loss, "loss"), (rec, "rec_loss"), (cl, "cl_loss")):
            want = gd[f"{k}_{key}"][s]
            assert abs(float(got.detach()) - want) <= 1e-5 * abs(want), (s, key, float(got.detach()), want)
        optimizer.zero_grad()
        loss.backward()
        if s == 0:
            for name, p in params.items():
                g = p.grad.detach().cpu().reshape(-1).numpy().astype(np.float64)
                want_g = gd[f"{k}_grad0_{name}_val"].astype(np.float64)
                assert np.abs(g[gd[f"sample_{name}"]] - want_g).max() <= 1e-4 * np.abs(want_g).max() + 1e-12, name
        optimizer.step()
        if s != 1:
            for name, p in params.items():
                v = p.detach().cpu().reshape(-1).numpy()
                assert np.abs(v[gd[f"sample_{name}"]] - gd[f"{k}_step{s}_{name}_val"]).max() <= model.lRate / 2, (s, name)
    return params


def test_registry_and_conf():
    from selfrec_amd import main
    from selfrec_amd.util.conf import ModelConf
    assert "DuoRec" in main.MODELS
    conf = ModelConf(os.path.join(REPO, "conf", "DuoRec.yaml"))
    assert conf["model"] == {"name": "DuoRec", "type": "sequential"}
    assert conf["DuoRec"] == {"n_blocks": 2, "drop_rate": 0.2, "n_heads": 1, "cl_rate": 0.01}      # the reference's values
    assert (conf["embedding.size"], conf["batch.size"], conf["max.len"], conf["max.epoch"]) == (64, 256, 50, 300)
    assert (conf["learning.rate"], conf["reg.lambda"], conf["item.ranking.topN"]) == (0.001, 0.0001, [10, 20])


def test_routes_and_optional_keys(golden, tmp_path, monkeypatch):
    from selfrec_amd.model.sequential.DuoRec import duo_route
    _, meta = golden
    model = make_model(meta, 1, tmp_path, monkeypatch)
    assert (model.duo, model.views, model.embed, model.tau, model.sim) == ("hip", "one", "hip", 1.0, "dot")
    assert model.model.item_emb.shape[0] == meta["item_num"] + 1                                     # no mask token
    assert make_model(meta, 1, tmp_path, monkeypatch, duo="pair").duo == "pair"
    monkeypatch.setenv("SRH_DUOREC_DUO", "pair")
    assert duo_route() == "pair"
    monkeypatch.setenv("SRH_DUOREC_DUO", "triton")
    with pytest.raises(ValueError):
        duo_route()


def test_indexed_sampler_equals_next_batch_sequence_and_leaves_its_state(golden, tmp_path, monkeypatch):
    from selfrec_amd.util.sampler import next_batch_sequence, next_batch_sequence_indexed
    _, meta = golden
    data = make_model(meta, 1, tmp_path, monkeypatch).data
    random.seed(99)
    plain = list(next_batch_sequence(data, 32, max_len=12))
    state = random.getstate()
    random.seed(99)
    indexed = list(next_batch_sequence_indexed(data, 32, max_len=12))
    assert random.getstate() == state and len(plain) == len(indexed)
    for a, b in zip(plain, indexed):
        assert len(b) == 6 and all(np.array_equal(x, y) for x, y in zip(a, b[:5]))
        for n, row in enumerate(b[5]):
            ids = data.original_seq[row][1]
            assert ids[(-12 if len(ids) > 12 else 0):-1] == list(b[0][n, :b[4][n]])


def test_index_and_draws_replay_the_golden(golden, tmp_path, monkeypatch):
    from selfrec_amd.util.sampler import next_batch_sequence_indexed, same_target_positives
    gd, meta = golden
    data = make_model(meta, 1, tmp_path, monkeypatch).data
    index = data.same_target_index()
    assert index is data.same_target_index()                                            # cached
    assert {str(t): v for t, v in index.items()} == meta["same_target"]
    assert meta["targets_shared_by_3"] >= 1 and meta["targets_single"] >= 1 and meta["long_candidates"]
    random.seed(meta["sampler_seed"])
    n = fallbacks = 0
    for b, batch in enumerate(next_batch_sequence_indexed(data, meta["conf"]["batch"], max_len=meta["conf"]["max_len"])):
        want_batch, want_pos = golden_step(gd, b)
        for got, want in zip(batch, want_batch):
            assert np.array_equal(np.asarray(got), want), b
        rows = batch[5]
        alone = [len(index[data.original_seq[r][1][-1]]) == 1 for r in rows]
        before = random.getstate()
        got = same_target_positives(data, rows, meta["conf"]["max_len"])
        if all(alone):
            assert random.getstate() == before
        for g, w in zip(got, want_pos + (gd[f"pos{b}_chosen"],)):
            assert np.array_equal(np.asarray(g), w), b
        assert all(got[3][i] == rows[i] for i in np.flatnonzero(alone))                  # the fallback: the row's own sequence
        fallbacks += int(np.count_nonzero(alone))
        n += 1
    assert n == meta["n_train_batches"] and fallbacks == meta["fallback_rows"] > 0
    # (had a fallback row consumed a draw, the state after the epoch would differ)
    assert np.array_equal(np.asarray(random.getstate()[1], dtype=np.int64), gd["rng_after_epoch"])
    # a single-sequence target on its own: no draw
    lone = next(v[0] for v in index.values() if len(v) == 1)
    before = random.getstate()
    assert same_target_positives(data, [lone], 12)[3].tolist() == [lone] and random.getstate() == before


@pytest.mark.parametrize("heads", [1, 2])
def test_cpu_model_reproduces_the_golden(golden, heads, tmp_path, monkeypatch):
    from selfrec_amd.util.evaluation import ranking_evaluation
    gd, meta = golden
    torch.manual_seed(meta["torch_seed"]); random.seed(meta["sampler_seed"])
    model = make_model(meta, heads, tmp_path, monkeypatch)
    params = dict(model.model.named_parameters())
    assert list(params) == meta["param_names"]
    check_initial_parameters(gd, params)
    replay_three_steps(gd, meta, model, heads)
    if heads != 1:
        return
    with torch.no_grad():
        for name, p in params.items():
            assert np.abs(p.numpy() - gd[f"h1_final_{name}"]).max() <= model.lRate / 2, name
            p.copy_(torch.from_numpy(gd[f"h1_final_{name}"]))
    model.model.eval()
    rec_list = model.test()
    d = model.data
    want_ids, want_sc = gd["h1_rec_ids"], gd["h1_rec_scores"]
    scale = np.abs(want_sc).max()
    for r, (name, _) in enumerate(d.original_seq):
        keep = want_ids[r] >= 0
        assert [d.item[it] for it, _ in rec_list[name]] == want_ids[r][keep].tolist(), name
        assert np.abs(np.asarray([sc for _, sc in rec_list[name]]) - want_sc[r][keep]).max() <= 1e-5 * scale, name
    ev = meta["h1_evaluation"]
    assert ranking_evaluation(d.test_set, rec_list, model.topN) == ev["topN"]
    assert ranking_evaluation(d.test_set, rec_list, [model.max_N]) == ev["maxN"]


def test_header_and_library_carry_the_entry_points():
    from selfrec_amd import _lib
    header = open(os.path.join(REPO, "include", "selfrec_hip.h")).read()
    assert "(a-25)" in header and f"#define SRH_ABI_VERSION {_lib.ABI_VERSION}" in header and _lib.ABI_VERSION == 31
    for name in ("srh_duo_nce_ws_bytes", "srh_duo_nce_fwd_bwd"):
        assert name in header and name in _lib.SIGNATURES
