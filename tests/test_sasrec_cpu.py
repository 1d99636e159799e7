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


# ---- the premises of the sequence-kernel edge tests (tests/seq_attn_ref.py, tests/test_gpu_seq_edges.py) ------------------
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
def test_restatement_lse_reproduces_the_softmax_attention_uses(causal):
    """V = I makes attention() return its own P; exp(s - lse) is that P, and lse is the plain log of the row's sum"""
    from tests import seq_attn_ref
    B, L, H, dh = 2, 17, 2, 32
    g = torch.Generator().manual_seed(11)
    q = 3.0 * torch.randn(B, L, H * dh, generator=g, dtype=torch.float64)
    k = torch.randn(B, L, H * dh, generator=g, dtype=torch.float64)
    v = torch.zeros(B, L, H, dh, dtype=torch.float64)
    v[:, torch.arange(L), :, torch.arange(L)] = 1.0
    p = seq_attn_ref.attention(q, k, v.reshape(B, L, H * dh), H, causal).reshape(B, L, H, dh)[..., :L].permute(0, 2, 1, 3)
    lse = seq_attn_ref.lse(q, k, H, causal)
    assert lse.shape == (B, H, L) and lse.dtype == torch.float64
    s = torch.stack([q[..., h * dh:(h + 1) * dh] @ k[..., h * dh:(h + 1) * dh].transpose(1, 2) for h in range(H)], 1) / dh ** 0.5
    sees = torch.ones(L, L, dtype=torch.bool).tril() if causal else torch.ones(L, L, dtype=torch.bool)
    got = torch.where(sees, torch.exp(s - lse[..., None]), torch.zeros_like(s))
    assert (got - p).abs().max() <= 1e-14
    assert (torch.where(sees, torch.exp(s), torch.zeros_like(s)).sum(-1).log() - lse).abs().max() <= 1e-12
    assert (p.sum(-1) - 1.0).abs().max() <= 1e-14
    if causal:
        assert torch.equal(lse[:, :, 0], s[:, :, 0, 0])                   # row 0 sees one key


def _row_keep(seed, ctr, L, p):
    """one row of the drawn mask at an explicit 64-bit counter, word by word"""
    from tests import counter_rng
    assert 0 <= ctr < 2 ** 64
    out = np.zeros(L, dtype=bool)
    for j in range(L):
        w = counter_rng.rng4(np.uint64(ctr), np.uint32(j // 4), seed).reshape(4)
        out[j] = counter_rng.u01(w[j % 4]) >= np.float32(p)
    return out


@pytest.mark.parametrize("ref_name", ["sasrec_ref", "bert4rec_ref"])
def test_drawn_keep_mask_carries_into_the_high_counter_word(ref_name):
    """counter 2^32 - 5 with B H L = 24 rows: rows 0..4 sit below the carry, rows 5.. at 2^32 + (row - 5); each equals the
    single-row draw at its explicit 64-bit counter, and a counter cut to 32 bits would draw something else"""
    import importlib
    ref = importlib.import_module(f"tests.{ref_name}")
    seed, base, p = 0xA5C319E75DEECE66, 2 ** 32 - 5, 0.2
    B, H, L = 2, 3, 4
    keep = ref.attn_keep_drawn(seed, base, B, H, L, p).reshape(B * H * L, L)
    for r in range(B * H * L):
        ctr = base + r
        assert (ctr >= 2 ** 32) == (r >= 5)
        assert np.array_equal(keep[r], _row_keep(seed, ctr, L, p)), r
    wide = ref.attn_keep_drawn(seed, base, 2, 1, 63, p).reshape(126, 63)
    after = np.stack([_row_keep(seed, base + r, 63, p) for r in (4, 5, 6, 125)])
    assert np.array_equal(wide[[4, 5, 6, 125]], after)
    cut = np.stack([_row_keep(seed, (base + r) & 0xFFFFFFFF, 63, p) for r in (5, 6, 125)])
    assert not np.array_equal(wide[[5, 6, 125]], cut)


@pytest.mark.parametrize("L", [1, 2, 17, 49, 63])
def test_drawn_keep_mask_at_lengths_off_the_float4(L):
    """L not a multiple of 4: the last float4 of a row is drawn whole and cut; column j is still word j % 4 of float4 j / 4,
    and a row's columns do not depend on L"""
    from tests import bert4rec_ref
    seed, base, p = 0x5DEECE66D1234, (1 << 33) + 7, 0.2
    B, H = 2, 2
    for ref in (sasrec_ref, bert4rec_ref):
        keep = ref.attn_keep_drawn(seed, base, B, H, L, p)
        assert keep.shape == (B, H, L, L) and keep.dtype == bool
        flat = keep.reshape(B * H * L, L)
        for r in sorted({0, L // 2, B * H * L - 1}):
            assert np.array_equal(flat[r], _row_keep(seed, base + r, L, p)), r
            assert np.array_equal(flat[r], _row_keep(seed, base + r, 64, p)[:L]), r
    if L >= 17:
        assert abs(1.0 - keep.mean() - p) < 0.05


def test_edge_case_inputs_have_the_properties_their_tests_rely_on():
    from tests import seq_attn_ref, test_gpu_bert4rec, test_gpu_sasrec
    # the shape lists of the two parametrised float64 tests: a near-one-hot row at every L >= 7, the appended shapes included
    for mod in (test_gpu_sasrec, test_gpu_bert4rec):
        assert {(2, 32, 4, 32), (2, 48, 1, 32)} <= set(mod.ATTN_SHAPES)
        for shape in mod.ATTN_SHAPES:
            if shape[0] <= 5 and shape[1] >= 7:
                for masked in (False, True):
                    c = mod.attn_case(shape, masked)
                    assert c["peak"] > 0.99, (mod.__name__, shape, masked)
                    assert c["lse"].shape == (shape[0], shape[2], shape[1])
    # the drawn-route cases: every L once per flavour, every head layout at two or more L, one of them off the tile
    for flavour in seq_attn_ref.FLAVOURS:
        shapes = seq_attn_ref.drawn_shapes(flavour)
        assert sorted(s[1] for s in shapes) == list(seq_attn_ref.EDGE_L) and {s[0] for s in shapes} == {2, 3}
        for heads in seq_attn_ref.EDGE_HEADS:
            at = [s[1] for s in shapes if s[2:] == heads]
            assert len(at) >= 2 and any(L % 16 for L in at), (flavour, heads, at)
            assert heads[0] * heads[1] <= 128
    assert seq_attn_ref.SEED >> 32 and seq_attn_ref.SEED < 2 ** 64
    # the range case: the even rows' logits overflow an unshifted float32 exp, and the ordinary rows alone keep gq and gk
    # of ordinary size, so a relative bound on them means something
    for flavour in seq_attn_ref.FLAVOURS:
        c = seq_attn_ref.range_case(flavour)
        assert 80.0 < c["logit_std_even"] < 125.0 and c["logit_max"] > 200.0
        for name in ("gq", "gk"):
            assert float(c["ordinary"][name].abs().max()) > 1.0, (flavour, name)
            assert float(c["ref"][name].abs().max()) > 1.0, (flavour, name)
        assert all(torch.isfinite(c["ref"][n]).all() for n in c["ref"])
    # the keep-mask edges: the dropped row and column are what the reference says they are
    for flavour in seq_attn_ref.FLAVOURS:
        for shape in seq_attn_ref.KEEP_EDGE_SHAPES:
            c = seq_attn_ref.keep_edge_case(flavour, shape)
            assert not c["keep"][:, :, c["row"]].any() and not c["keep"][:, :, :, c["col"]].any()
            assert c["keep"].mean() > 0.6 and 0 < c["col"] < c["row"] == shape[1] - 1
            assert not c["ref"]["out"][:, c["row"]].any() and not c["ref"]["gq"][:, c["row"]].any()
            assert not c["ref"]["gv"][:, c["col"]].any() and c["ref"]["gv"][:, c["col"] + 1].any()
    # the BCE widths: logits of standard deviation ~24 at every width (3 or 5 rows alone need not reach 30; together they do)
    assert len(seq_attn_ref.BCE_EDGE_CASES) == 21
    small = [seq_attn_ref.bce_edge_case(R, d) for R, d in seq_attn_ref.BCE_EDGE_CASES if R <= 5]
    logits = torch.cat([torch.cat([c["xp"], c["xn"]]) for c in small])
    assert 18.0 < float(logits.std()) < 30.0 and float(logits.max()) > 30.0 and float(logits.min()) < -30.0
    for R, d in seq_attn_ref.BCE_EDGE_CASES:
        c = seq_attn_ref.bce_edge_case(R, d)
        if R >= 255:
            assert c["span"] > 30.0
        assert c["grows"].shape == (2 * R, d) and not c["grows"][:R][~c["valid"]].any()
        # the per-row gradients scatter to the table gradient
        gt = torch.zeros_like(c["gt"]).index_add_(0, torch.cat([c["pos"], c["neg"]]), c["grows"])
        assert (gt - c["gt"]).abs().max() <= 1e-12 * max(1.0, float(c["gt"].abs().max()))
    c = seq_attn_ref.bce_bad_id_case()
    assert int(c["usable"].sum()) == 7 and not c["gh"][~c["usable"]].any() and c["gh"][c["usable"]].any(dim=1).all()
