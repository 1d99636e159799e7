"""CL4SRec without a GPU: the three sequence augmentors against the reference-run golden (tests/golden/cl4srec.npz,
make_golden_cl4srec.py) with both generator states, the live plan against a brute-force grouping, the float64 restatement
(tests/cl4srec_ref.py) and the CPU model against the golden, the conf, the registry and the routes, and the
admissibility of the GPU tests' bounds: float32 torch on the CPU meets them on every case of tests/cl4srec_cases.py."""
import json
import os
import random
import types

import numpy as np
import pytest
import torch

from tests import cl4srec_cases as cases
from tests import cl4srec_ref
from tests.test_shapes_cpu import GOLDEN

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("srh_seq_embed_fwd_f32", "srh_rows_live_sum_ws_bytes", "srh_rows_live_sum_f32")
RUNS = [(0, 1), (0, 2), (1, 1), (2, 1)]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "cl4srec.npz")), json.load(open(os.path.join(GOLDEN, "cl4srec_meta.json")))


def make_model(meta, aug_type, heads, tmp_path, monkeypatch, **over):
    from selfrec_amd.model.sequential.CL4SRec import CL4SRec
    from selfrec_amd.util.conf import ModelConf
    monkeypatch.chdir(tmp_path)
    for env in ("SRH_SASREC_ATTN", "SRH_CL4SREC_VIEWS", "SRH_CL4SREC_EMBED"):
        monkeypatch.delenv(env, raising=False)
    c = meta["conf"]
    conf = {"model": {"name": "CL4SRec", "type": "sequential"}, "item.ranking.topN": c["topN"], "embedding.size": c["emb"],
            "max.epoch": 1, "batch.size": c["batch"], "learning.rate": c["lr"], "reg.lambda": c["reg"], "output": "./results/",
            "training.set": "x", "test.set": "y", "max.len": c["max_len"],
            "CL4SRec": {"n_blocks": c["n_blocks"], "drop_rate": over.get("drop_rate", c["drop_rate"]), "n_heads": heads,
                        "aug_type": aug_type, "aug_rate": c["aug_rate"], "cl_rate": c["cl_rate"]}}
    for key in ("views", "embed", "attention"):
        if key in over:
            conf[f"engine.{key}"] = over[key]
    return CL4SRec(ModelConf(conf), {k: list(v) for k, v in meta["train"].items()},
                   {k: list(v) for k, v in meta["test"].items()})


def golden_step(gd, T, b):
    """(batch, views) of step b of aug_type T as the golden recorded them"""
    batch = tuple(gd[f"t{T}_train{b}_{k}"] for k in ("seq", "pos", "y", "neg", "len"))
    views = [(gd[f"t{T}_aug{b}_seq{v}"], gd[f"t{T}_aug{b}_pos{v}"], gd[f"t{T}_aug{b}_len{v}"]) for v in (1, 2)]
    return batch, views


def seeded(meta):
    torch.manual_seed(meta["torch_seed"]); random.seed(meta["sampler_seed"]); np.random.seed(meta["numpy_seed"])


def check_initial_parameters(gd, params):
    for name, p in params.items():
        v = p.detach().cpu().numpy().reshape(-1)
        assert np.array_equal(v[gd[f"sample_{name}"]], gd[f"init_{name}_val"]), name
        assert abs(v.astype(np.float64).sum() - gd[f"init_{name}_sum"][0]) <= 1e-9 * np.abs(v).sum(), name


@pytest.mark.parametrize("aug_type", [0, 1, 2])
def test_augmentors_equal_the_golden_views_and_leave_both_generator_states(golden, aug_type, tmp_path, monkeypatch):
    """an epoch driven as train() drives it: the sampler's batch n, then the two views of step n, on one random stream"""
    from selfrec_amd.util.sampler import next_batch_sequence
    gd, meta = golden
    seeded(meta)
    model = make_model(meta, aug_type, 1, tmp_path, monkeypatch)
    n = 0
    for b, batch in enumerate(next_batch_sequence(model.data, model.batch_size, max_len=model.max_len)):
        seq, pos, _, _, seq_len = batch
        want_batch, want_views = golden_step(gd, aug_type, b)
        for got, want in zip(batch, want_batch):
            assert np.array_equal(np.asarray(got), want), b
        before = seq.copy()
        for (a_seq, a_pos, a_len), (w_seq, w_pos, w_len) in zip(model.augment(seq, pos, seq_len), want_views):
            assert np.array_equal(a_seq, w_seq) and np.array_equal(a_pos, w_pos), b
            assert np.array_equal(np.asarray(a_len), w_len), b
        assert np.array_equal(seq, before)                            # the batch itself is not edited
        n += 1
    assert n == meta[f"t{aug_type}_n_train_batches"]
    assert np.array_equal(np.asarray(random.getstate()[1], dtype=np.int64), gd[f"t{aug_type}_rng_after_epoch"])
    st = np.random.get_state()
    assert np.array_equal(np.r_[np.asarray(st[1], dtype=np.int64), st[2]], gd[f"t{aug_type}_np_rng_after_epoch"])
    if aug_type == 0:
        lens = np.concatenate([gd[f"t0_train{b}_len"] for b in range(n)])
        assert lens.min() == 1                                        # crop met a sequence of one item


def test_augmentor_semantics_on_a_hand_case():
    from selfrec_amd.data.augmentor import SequenceAugmentor as A
    seq = np.array([[5, 6, 7, 8, 0, 0], [9, 0, 0, 0, 0, 0]])
    random.seed(1); np.random.seed(1)
    a_seq, a_pos, a_len = A.item_crop(seq, [4, 1], 0.5)
    assert a_len == [3, 1] and a_seq[1].tolist() == [9, 0, 0, 0, 0, 0] and a_pos[0].tolist() == [1, 2, 3, 0, 0, 0]
    assert a_seq[0, :3].tolist() in ([5, 6, 7], [6, 7, 8])
    r = A.item_reorder(seq, [4, 1], 0.5)
    assert sorted(r[0].tolist()) == sorted(seq[0].tolist()) and r[1].tolist() == seq[1].tolist() and not r[0, 4:].any()
    m = A.item_mask(seq, [4, 1], 0.5, 99)
    assert (m[0] == 99).sum() == 2 and not (m[0, 4:] != 0).any() and m[1].tolist() == seq[1].tolist()


def test_live_plan_equals_a_brute_force_grouping():
    from selfrec_amd import ops
    assert ops.LIVE_SUM_CHUNK == cases.CHUNK
    header = open(os.path.join(REPO, "include", "selfrec_hip.h")).read()
    assert f"#define SRH_LIVE_SUM_CHUNK {cases.CHUNK}\n" in header
    c = cases.segment_case()
    got = ops.live_plan_host(c["ids"], c["live"])
    want = cl4srec_ref.brute_force_plan(c["ids"], c["live"], cases.CHUNK)
    for a, b in zip(got, want):
        assert a.dtype == np.int32 and np.array_equal(a, b)
    rows, chunk_start, chunk_dst, multi_range, multi_row = got
    assert sorted(np.diff(chunk_start).tolist())[-1] == cases.CHUNK and rows.size == sum(cases.SEGMENT_LENGTHS)
    per_segment = [(n + cases.CHUNK - 1) // cases.CHUNK for n in cases.SEGMENT_LENGTHS]
    assert per_segment == [1, 1, 1, 2, 2, 3, 21] and multi_row.size == 4 and chunk_dst.size == sum(per_segment)
    assert np.diff(multi_range.reshape(-1, 2), axis=1).reshape(-1).tolist() == [2, 2, 3, 21]
    # the default live rule is ids != 0; other chunk lengths; every embed case
    for shape in cases.EMBED_SHAPES:
        e = cases.embed_case(shape)
        for ids in (e["seq"], e["pos"]):
            for a, b in zip(ops.live_plan_host(ids, e["live"]), cl4srec_ref.brute_force_plan(ids, e["live"], cases.CHUNK)):
                assert np.array_equal(a, b), shape
    ids = np.array([0, 4, 4, 0, 2, 4])
    for a, b in zip(ops.live_plan_host(ids, chunk=2), cl4srec_ref.brute_force_plan(ids, ids != 0, 2)):
        assert np.array_equal(a, b)
    # a batch with no live row
    empty = ops.live_plan_host(np.zeros(9, dtype=np.int64))
    assert [a.size for a in empty] == [0, 1, 0, 0, 0] and empty[1][0] == 0


@pytest.mark.parametrize("aug_type,heads", RUNS)
def test_float64_restatement_reproduces_the_golden(golden, aug_type, heads):
    """three Adam steps in float64 on the golden's batches and views: losses <= 1e-5 relative, step 0's gradients <= 1e-4
    of each tensor's max; the stacked pass gives the three passes' losses"""
    from selfrec_amd.model.sequential.CL4SRec import CL4SRec_Model
    gd, meta = golden
    c = meta["conf"]
    k = f"t{aug_type}h{heads}"
    torch.manual_seed(meta["torch_seed"])
    net = CL4SRec_Model(types.SimpleNamespace(item_num=meta["item_num"]), c["emb"], c["max_len"], c["n_blocks"], heads, 0.0)
    check_initial_parameters(gd, dict(net.named_parameters()))
    params = {n: p.detach().double().requires_grad_(True) for n, p in net.named_parameters()}
    opt = torch.optim.Adam(list(params.values()), lr=c["lr"])
    for s in range(3):
        batch, views = golden_step(gd, aug_type, s)
        loss, rec, cl = cl4srec_ref.step_losses(params, batch, views, c["n_blocks"], heads, c["reg"], c["cl_rate"])
        for got, key in ((loss, "loss"), (rec, "rec_loss"), (cl, "cl_loss")):
            want = gd[f"{k}_{key}"][s]
            assert abs(float(got.detach()) - want) <= 1e-5 * abs(want), (s, key, float(got.detach()), want)
        with torch.no_grad():
            stacked = cl4srec_ref.step_losses(params, batch, views, c["n_blocks"], heads, c["reg"], c["cl_rate"], stacked=True)
        assert abs(float(stacked[0]) - float(loss.detach())) <= 1e-12 * abs(float(loss.detach()))
        opt.zero_grad()
        loss.backward()
        if s == 0:
            for name, p in params.items():
                g = p.grad.reshape(-1).numpy()
                want_g = gd[f"{k}_grad0_{name}_val"].astype(np.float64)
                err = np.abs(g[gd[f"sample_{name}"]] - want_g).max()
                assert err <= 1e-4 * np.abs(want_g).max() + 1e-12, (name, err)
                assert abs(g.sum() - gd[f"{k}_grad0_{name}_sum"][0]) <= 1e-4 * np.abs(g).sum() + 1e-12, name
        opt.step()


@pytest.mark.parametrize("aug_type,heads", RUNS)
def test_cpu_model_reproduces_the_golden(golden, aug_type, heads, tmp_path, monkeypatch):
    """the model on the CPU (torch's expressions throughout) on the golden's batches and views: losses <= 1e-5, step 0's
    gradients <= 1e-4 of each tensor's max, parameters within lr / 2; test() on the final parameters"""
    from selfrec_amd.util.evaluation import ranking_evaluation
    gd, meta = golden
    k = f"t{aug_type}h{heads}"
    seeded(meta)
    model = make_model(meta, aug_type, heads, tmp_path, monkeypatch)
    net = model.model
    params = dict(net.named_parameters())
    assert list(params) == meta["param_names"] and net.item_emb.shape[0] == meta["item_num"] + 2
    check_initial_parameters(gd, params)
    optimizer = torch.optim.Adam(net.parameters(), lr=model.lRate)
    lr = model.lRate
    net.train()
    for s in range(3):
        (seq, pos, y, neg, _), views = golden_step(gd, aug_type, s)
        loss, rec, cl = model.step_losses(seq, pos, y, neg, views)
        for got, key in ((loss, "loss"), (rec, "rec_loss"), (cl, "cl_loss")):
            want = gd[f"{k}_{key}"][s]
            assert abs(float(got.detach()) - want) <= 1e-5 * abs(want), (s, key, float(got.detach()), want)
        optimizer.zero_grad()
        loss.backward()
        if s == 0:
            for name, p in params.items():
                g = p.grad.reshape(-1).numpy().astype(np.float64)
                want_g = gd[f"{k}_grad0_{name}_val"].astype(np.float64)
                assert np.abs(g[gd[f"sample_{name}"]] - want_g).max() <= 1e-4 * np.abs(want_g).max() + 1e-12, name
        optimizer.step()
        if s != 1:
            for name, p in params.items():
                v = p.detach().reshape(-1).numpy()
                assert np.abs(v[gd[f"sample_{name}"]] - gd[f"{k}_step{s}_{name}_val"]).max() <= lr / 2, (s, name)
    if f"{k}_final_{meta['param_names'][0]}" not in gd.files:
        return
    with torch.no_grad():
        for name, p in params.items():
            assert np.abs(p.numpy() - gd[f"{k}_final_{name}"]).max() <= lr / 2, name
            p.copy_(torch.from_numpy(gd[f"{k}_final_{name}"]))
    net.eval()
    rec_list = model.test()
    d = model.data
    want_ids, want_sc = gd[f"{k}_rec_ids"], gd[f"{k}_rec_scores"]
    scale = np.abs(want_sc).max()
    for r, (name, _) in enumerate(d.original_seq):
        keep = want_ids[r] >= 0
        assert [d.item[it] for it, _ in rec_list[name]] == want_ids[r][keep].tolist(), name
        assert np.abs(np.asarray([sc for _, sc in rec_list[name]]) - want_sc[r][keep]).max() <= 1e-5 * scale, name
    assert (want_ids < 0).any() and want_ids.max() <= meta["item_num"]          # ids 0 and item_num + 1 left the lists
    ev = meta[f"{k}_evaluation"]
    assert ranking_evaluation(d.test_set, rec_list, model.topN) == ev["topN"]
    assert ranking_evaluation(d.test_set, rec_list, [model.max_N]) == ev["maxN"]


def test_conf_registry_and_routes(monkeypatch):
    from selfrec_amd import main
    from selfrec_amd.model.sequential import CL4SRec as mod
    from selfrec_amd.util.conf import ModelConf
    assert "CL4SRec" in main.MODELS
    conf = ModelConf(os.path.join(REPO, "conf", "CL4SRec.yaml"))
    assert set(conf.config) == {"training.set", "test.set", "model", "item.ranking.topN", "embedding.size", "max.epoch",
                                "batch.size", "learning.rate", "reg.lambda", "max.len", "CL4SRec", "output"}
    assert conf["model"] == {"name": "CL4SRec", "type": "sequential"}
    assert set(conf["CL4SRec"]) == {"n_blocks", "drop_rate", "n_heads", "aug_type", "aug_rate", "cl_rate"}
    for name in ("train", "calculate_loss", "predict", "test", "fast_evaluation", "last_hidden", "item_table"):
        assert callable(getattr(mod.CL4SRec, name)), name
    assert issubclass(mod.CL4SRec_Model, mod.SASRec_Model)
    for fn, env, key, choices in ((mod.views_route, "SRH_CL4SREC_VIEWS", "engine.views", ("one", "three")),
                                  (mod.embed_route, "SRH_CL4SREC_EMBED", "engine.embed", ("hip", "torch"))):
        monkeypatch.delenv(env, raising=False)
        assert fn(ModelConf({})) == choices[0] and fn(None) == choices[0]
        assert fn(ModelConf({key: choices[1]})) == choices[1]
        monkeypatch.setenv(env, choices[1])
        assert fn(ModelConf({key: choices[0]})) == choices[1]
        monkeypatch.setenv(env, "eager")
        with pytest.raises(ValueError):
            fn(None)
        monkeypatch.delenv(env)


def test_entry_points_are_declared_and_bound():
    from selfrec_amd import _lib, ops
    header = open(os.path.join(REPO, "include", "selfrec_hip.h")).read()
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES and f"{name}(" in header, name
    for name in ("seq_embed_fwd", "live_plan_host", "live_plan", "rows_live_sum", "SeqEmbedFn", "SeqBceLiveFn", "InfoNceFn"):
        assert getattr(ops, name) and name in ops.__all__, name
    assert "(a-18)" in header and f"#define SRH_ABI_VERSION {_lib.ABI_VERSION}" in header and _lib.ABI_VERSION == 31
    assert f"#define SRH_LIVE_SUM_MAX_PROBLEMS {ops.LIVE_SUM_MAX_PROBLEMS}\n" in header
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert all(hasattr(lib, name) for name in SYMBOLS)
    assert all(ops.seq_embed_supported(d) for d in (32, 64, 128)) and not ops.seq_embed_supported(48)


def test_restatement_keep_mask_is_one_counter_per_row():
    a = cl4srec_ref.embed_keep_drawn(99, 1000, 6, 64, 0.2)
    b = cl4srec_ref.embed_keep_drawn(99, 1003, 3, 64, 0.2)
    assert a.shape == (6, 64) and np.array_equal(a[3:], b) and not np.array_equal(a[:3], b)
    assert abs(1.0 - cl4srec_ref.embed_keep_drawn(5, 0, 400, 64, 0.2).mean() - 0.2) < 0.02


# ---- admissibility: float32 torch on the CPU meets the GPU tests' bounds on their cases ------------------------------------
@pytest.mark.parametrize("shape", cases.EMBED_SHAPES, ids=cases.shape_id)
def test_float32_torch_meets_the_embed_and_live_sum_bounds(shape):
    c = cases.embed_case(shape)
    B, L, d = shape
    seq, pos, live = c["seq"], c["pos"], torch.from_numpy(c["live"])
    assert not c["out"][~live].any() and c["out"][live].abs().max() > 0
    if B > 1:
        assert (c["pos"].reshape(-1)[~c["live"]] != 0).any()           # seq = 0 with pos != 0
        assert not c["seq"][1].any() and (c["seq"] == cases.N_ITEMS + 1).any()
        assert all(row[0] == cases.REPEATED for row in c["seq"] if row.any())
    for keep, tag in ((None, ""), (c["keep"], "_keep")):
        item, pos_table = c["item"].clone().requires_grad_(True), c["pos_table"].clone().requires_grad_(True)
        out = cases.torch_embed_front(item, pos_table, seq, pos, keep, cases.DROP_P)
        out.backward(c["go"])
        errs = dict(out=cases.rel_err(out.detach(), c["out" + tag]), gi=cases.rel_err(item.grad, c["gi" + tag]),
                    gp=cases.rel_err(pos_table.grad, c["gp" + tag]))
        assert errs["out"] <= cases.OUT_BOUND and max(errs["gi"], errs["gp"]) <= cases.GRAD_BOUND, (tag, errs)


def test_float32_torch_meets_the_segment_and_infonce_bounds():
    c = cases.segment_case()
    got = torch.zeros(c["n_table"], c["x"].shape[1])
    rows = torch.from_numpy(np.flatnonzero(c["live"]))
    got.index_add_(0, torch.from_numpy(c["ids"])[rows].long(), c["x"][rows])
    assert cases.rel_err(got, c["want"]) <= cases.GRAD_BOUND
    for n in cases.NCE_SIZES:
        e = cases.nce_case(n)
        v1, v2 = e["v1"].clone().requires_grad_(True), e["v2"].clone().requires_grad_(True)
        loss = cl4srec_ref.info_nce(v1, v2, 1.0)
        loss.backward()
        if n == 1:
            assert e["loss"] == 0.0 and abs(float(loss)) <= 1e-6 and v1.grad.abs().max() <= 1e-6 and v2.grad.abs().max() <= 1e-6
        else:
            assert abs(float(loss) - e["loss"]) <= cases.OUT_BOUND * abs(e["loss"]), n
            assert max(cases.rel_err(v1.grad, e["g1"]), cases.rel_err(v2.grad, e["g2"])) <= cases.GRAD_BOUND, n
