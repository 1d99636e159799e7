"""The tiled attention kernels (srh_seq_attn_tiled_*, csrc/seqrec.hip) on the device, against float64
(tests/seq_attn_ref.py through tests/seq_attn_tiled_cases.py, whose premises and float32 admissibility
tests/test_seq_attn_tiled_cpu.py checks without a GPU):

* drawn dropout, forward and backward, both flavours, at every L around a 64-row block edge up to 512, two consecutive
  calls whose counters cross the 32-bit carry, and bit for bit against the given-mask route;
* given masks with an empty query row at a block's first row and key columns nobody keeps;
* logits of standard deviation ~100 whose row maximum falls in every key block;
* repeatability, the refusals, and SASRec, BERT4Rec and CL4SRec at max.len 80 against the torch route.

Bounds (tests/test_gpu_seq_edges.py): out and lse <= 1e-5, gradients <= 1e-4, each of its tensor's largest magnitude."""
import random

import numpy as np
import pytest
import torch

from tests import seq_attn_ref as R
from tests import seq_attn_tiled_cases as T

pytestmark = pytest.mark.gpu


def run_pair(flavour, c, H, **kw):
    """one forward / backward pair on the device: {out, lse, gq, gk, gv}"""
    from selfrec_amd import ops
    dev = torch.device("cuda:0")
    q, k, v, go = (c[n].to(dev) for n in ("q", "k", "v", "go"))
    if kw.get("keep") is not None:
        kw["keep"] = torch.as_tensor(kw["keep"]).to(dev)
    kw["causal"] = flavour == "causal"
    out, lse = ops.seq_attn_tiled_fwd(q, k, v, H, **kw)
    return dict(zip(T.NAMES, (out, lse) + tuple(ops.seq_attn_tiled_bwd(q, k, v, out, lse, go, H, **kw))))


@pytest.mark.parametrize("flavour,shape", T.DRAWN_CASES, ids=lambda x: x if isinstance(x, str) else T.shape_id(x))
def test_drawn_dropout_forward_and_backward_match_float64_and_the_given_mask_route(flavour, shape):
    """two consecutive calls at the counters 2^32 - 5 and 2^32 - 5 + B H L: each meets the bounds against float64 under the
    HOST's mask for its counter, and the first equals the given-mask route under that mask bit for bit in all five tensors"""
    B, L, H, dh = shape
    c = T.drawn_case(flavour, shape)
    first, second = c["calls"]
    assert second["counter"] == first["counter"] + B * H * L
    for call in (first, second):
        got = run_pair(flavour, c, H, drop_p=R.DROP_P, rng_seed=R.SEED, rng_counter=call["counter"])
        T.assert_bounds(T.errors(got, call["ref"], L), (flavour, shape, "drawn at", call["counter"]))
        if call is first:
            given = run_pair(flavour, c, H, keep=call["keep"], drop_p=R.DROP_P)
            differ = [n for n in T.NAMES if not torch.equal(got[n], given[n])]
            assert not differ, (flavour, shape, "drawn and given differ in", differ)


@pytest.mark.parametrize("shape", T.KEEP_EDGE_SHAPES, ids=T.shape_id)
@pytest.mark.parametrize("flavour", R.FLAVOURS)
def test_a_dropped_query_row_and_dropped_key_columns_leave_exact_zeros(flavour, shape):
    """the first row of the last 64-row block keeps nothing: out and gq of the row are exact zeros; a key nobody keeps (one in
    the first block, for the full flavour one in the last too) takes no dV; everything else meets the bounds"""
    B, L, H, dh = shape
    c = T.keep_edge_case(flavour, shape)
    got = run_pair(flavour, c, H, keep=c["keep"], drop_p=R.DROP_P)
    assert not got["out"][:, c["row"]].any() and not got["gq"][:, c["row"]].any()
    for col in c["cols"]:
        assert not got["gv"][:, col].any(), col
    T.assert_bounds(T.errors(got, c["ref"], L), (flavour, shape, "row", c["row"], "cols", c["cols"]))


@pytest.mark.parametrize("flavour", R.FLAVOURS)
def test_logits_of_a_hundred_standard_deviations_stay_finite_and_inside_the_bounds(flavour):
    B, L, H, dh = T.RANGE_SHAPE
    c = T.range_case(flavour)
    assert c["logit_max"] > 200.0
    got = run_pair(flavour, c, H)
    for n in T.NAMES:
        assert torch.isfinite(got[n]).all(), n
    T.assert_bounds(T.errors(got, c["ref"], L), (flavour, T.RANGE_SHAPE, "largest |logit|", c["logit_max"]))


@pytest.mark.parametrize("flavour", R.FLAVOURS)
def test_the_same_call_twice_gives_the_same_bits(flavour):
    B, L, H, dh = T.REPEAT_SHAPE
    c = T.drawn_case(flavour, T.REPEAT_SHAPE)
    kw = dict(drop_p=R.DROP_P, rng_seed=R.SEED, rng_counter=R.COUNTER)
    one, two = run_pair(flavour, c, H, **kw), run_pair(flavour, c, H, **kw)
    for n in T.NAMES:
        assert torch.equal(one[n], two[n]), n
    T.assert_bounds(T.errors(one, c["calls"][0]["ref"], L), (flavour, T.REPEAT_SHAPE, "repeat"))


UNSUPPORTED, INVALID = -3, -1                # SRH_ERR_UNSUPPORTED, SRH_ERR_INVALID_ARG
REFUSALS = [("L", (1, 513, 1, 64), 0.0, UNSUPPORTED, "L=513"), ("dh", (1, 100, 1, 16), 0.0, UNSUPPORTED, "head width 16"),
            ("width", (1, 100, 3, 64), 0.0, UNSUPPORTED, "H dh = 192"),
            ("drop_p", (1, 100, 1, 64), 1.0, INVALID, "drop probability")]


@pytest.mark.parametrize("what,shape,drop_p,status,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_come_with_a_message_before_any_launch(what, shape, drop_p, status, message):
    """SRH_ERR_UNSUPPORTED (-3) outside the envelope, SRH_ERR_INVALID_ARG (-1) for drop_p = 1; outputs pre-filled with a
    sentinel are untouched"""
    from selfrec_amd import _lib, ops
    lib = _lib.load()
    B, L, H, dh = shape
    dev = torch.device("cuda:0")
    q, k, v, go, out_in = (torch.randn(B, L, H * dh, device=dev) for _ in range(5))
    lse_in = torch.zeros(B, H, L, device=dev)
    for causal in (1, 0):
        out, gq, gk, gv = (torch.full((B, L, H * dh), 7.0, device=dev) for _ in range(4))
        lse = torch.full((B, H, L), 7.0, device=dev)
        rc = lib.srh_seq_attn_tiled_fwd_f32(q.data_ptr(), k.data_ptr(), v.data_ptr(), B, L, H, dh, causal, None, 1, 2, drop_p,
                                            out.data_ptr(), lse.data_ptr(), None)
        assert rc == status
        with pytest.raises(ops.SelfrecHipError, match=r"\(%d\).*%s" % (status, message)):
            _lib.check(rc, "srh_seq_attn_tiled_fwd_f32")
        rc = lib.srh_seq_attn_tiled_bwd_f32(q.data_ptr(), k.data_ptr(), v.data_ptr(), out_in.data_ptr(), go.data_ptr(),
                                            lse_in.data_ptr(), B, L, H, dh, causal, None, 1, 2, drop_p, gq.data_ptr(),
                                            gk.data_ptr(), gv.data_ptr(), None)
        assert rc == status
        with pytest.raises(ops.SelfrecHipError, match=r"\(%d\).*%s" % (status, message)):
            _lib.check(rc, "srh_seq_attn_tiled_bwd_f32")
        torch.cuda.synchronize()
        for t in (out, lse, gq, gk, gv):
            assert bool((t == 7.0).all())
    if status == UNSUPPORTED:
        assert not ops.seq_attn_tiled_supported(L, H, dh)
    with pytest.raises(ops.SelfrecHipError, match=r"\(%d\)" % status):        # the wrapper passes the refusal on
        ops.seq_attn_tiled_fwd(q, k, v, H, drop_p=drop_p)


# ---- the three models at max.len 80 -----------------------------------------------------------------------------------------
MODEL_LINES = dict(SASRec=[], BERT4Rec=["  mask_rate: 0.5"], CL4SRec=["  aug_type: 0", "  aug_rate: 0.5", "  cl_rate: 0.05"])
MAX_LEN = T.MODEL_MAX_LEN


@pytest.fixture(scope="module")
def long_sequences(tmp_path_factory):
    """the generated set of T.LONG_SEQ on disk: training sequences longer than max.len are among them"""
    from selfrec_amd import synth
    train, test = T.long_sequences()
    assert sum(len(s) > MAX_LEN for s in train.values()) >= 10
    root = tmp_path_factory.mktemp("long_seq")
    synth.write_sequences(str(root / "train.txt"), train)
    synth.write_sequences(str(root / "test.txt"), test)
    return root


def model_conf(root, tmp_path, name, drop, attention):
    lines = [f"training.set: {root / 'train.txt'}", f"test.set: {root / 'test.txt'}", "model:", f"  name: {name}",
             "  type: sequential", "item.ranking.topN: [10,20]", "embedding.size: 64", "max.epoch: 1", "batch.size: 32",
             "learning.rate: 0.001", "reg.lambda: 0.0001", f"max.len: {MAX_LEN}", f"{name}:", "  n_blocks: 2",
             f"  drop_rate: {drop}", "  n_heads: 1"] + MODEL_LINES[name] + ["output: ./results/", f"engine.attention: {attention}"]
    path = tmp_path / f"{name}_{attention}_{drop}.yaml"
    path.write_text("\n".join(lines) + "\n")
    return str(path)


def run_model(name, conf_path, monkeypatch):
    """SELFRec(conf).execute() from fixed seeds, returning the model instance it built"""
    import importlib
    from selfrec_amd.SELFRec import SELFRec
    from selfrec_amd.util.conf import ModelConf
    cls = getattr(importlib.import_module(f"selfrec_amd.model.sequential.{name}"), name)
    made = []
    init = cls.__init__

    def recording_init(self, *a, **k):
        made.append(self)
        init(self, *a, **k)
    monkeypatch.setattr(cls, "__init__", recording_init)
    torch.manual_seed(1); random.seed(1); np.random.seed(1)
    SELFRec(ModelConf(conf_path)).execute()
    monkeypatch.setattr(cls, "__init__", init)
    return made[0]


@pytest.mark.parametrize("name", sorted(MODEL_LINES))
def test_the_three_models_train_on_the_tiled_kernels_at_max_len_80(name, long_sequences, tmp_path, monkeypatch, capsys):
    """one epoch without dropout by engine.attention tiled (the explicit route: the measured default above 64 positions is
    torch) and by torch from the same seeds: per-batch losses agree to 1e-4 of the largest (the convention
    of test_sasrec_end_to_end); one epoch at dropout 0.2: finite losses, counters drawn"""
    torch.cuda.set_device(0)
    monkeypatch.chdir(tmp_path)
    for env in ("SRH_SASREC_ATTN", "SRH_BERT4REC_CE", "SRH_CL4SREC_VIEWS", "SRH_CL4SREC_EMBED"):
        monkeypatch.delenv(env, raising=False)
    runs = {}
    for route in ("tiled", "torch"):
        m = run_model(name, model_conf(long_sequences, tmp_path, name, 0.0, route), monkeypatch)
        assert m.model.attention == route and not m.model.uses_kernel(MAX_LEN)
        assert m.model.attention_kernel(MAX_LEN) == ("tiled" if route == "tiled" else None)
        runs[route] = np.asarray(m.epoch_losses[0])
    assert len(runs["tiled"]) == 3 and np.isfinite(runs["tiled"]).all()
    err = np.abs(runs["tiled"] - runs["torch"]).max()
    print(name, "tiled vs torch losses", err, runs["torch"])
    assert err <= 1e-4 * np.abs(runs["torch"]).max()
    m = run_model(name, model_conf(long_sequences, tmp_path, name, 0.2, "tiled"), monkeypatch)
    capsys.readouterr()
    assert np.isfinite(np.asarray(m.epoch_losses)).all() and m.model.rng_counter > 0
    assert m.model.attention_kernel(MAX_LEN) == "tiled"
