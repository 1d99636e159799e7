"""The tiled attention kernels without a GPU: the bounds tests/test_gpu_seq_attn_tiled.py holds them to are
admissible -- torch's float32 expression on the host meets them on every case --, the range case has the premises it
claims, SeqEncoder.attention_kernel routes by length, and the front end's new names are there."""
import os

import numpy as np
import pytest
import torch

from tests import seq_attn_ref as R
from tests import seq_attn_tiled_cases as T


@pytest.mark.parametrize("flavour,shape", T.DRAWN_CASES, ids=lambda x: x if isinstance(x, str) else T.shape_id(x))
def test_float32_meets_the_bounds_on_every_drawn_case(flavour, shape):
    B, L, H, dh = shape
    c = T.drawn_case(flavour, shape)
    first, second = c["calls"]
    assert first["counter"] == R.COUNTER < 2 ** 32
    assert second["counter"] + B * H * L > 2 ** 32 or L == 1            # rows past the 32-bit carry (L = 1 has 4 rows in all)
    assert second["counter"] == first["counter"] + B * H * L
    assert not np.array_equal(first["keep"], second["keep"])
    for call in c["calls"]:
        got = T.float32_pair(c, H, flavour == "causal", call["keep"], R.DROP_P)
        T.assert_bounds(T.errors(got, call["ref"], L), (flavour, shape, "float32 at", call["counter"]))


def test_the_drawn_shapes_cover_every_block_edge_and_head_layout():
    for flavour in R.FLAVOURS:
        shapes = T.drawn_shapes(flavour)
        assert [s[1] for s in shapes] == list(T.TILED_L)
        assert {s[2:] for s in shapes} == set(R.EDGE_HEADS)
        assert all(s[0] == (2 if s[1] <= 200 else 1) for s in shapes)
    for edge in (64, 128, 192, 256, 512):                             # either side of a block edge; 512 is the envelope's end
        assert edge in T.TILED_L and (edge + 1 in T.TILED_L or edge == 512) and (edge - 1 in T.TILED_L or edge == 64)
    assert {79, 80, 81} <= set(T.TILED_L) and max(T.TILED_L) == 512


@pytest.mark.parametrize("shape", T.KEEP_EDGE_SHAPES, ids=T.shape_id)
@pytest.mark.parametrize("flavour", R.FLAVOURS)
def test_float32_meets_the_bounds_on_the_given_mask_cases_and_their_zeros_are_real(flavour, shape):
    B, L, H, dh = shape
    c = T.keep_edge_case(flavour, shape)
    assert c["row"] == T.BLOCK * ((L - 1) // T.BLOCK) > 0 and c["cols"][0] < T.BLOCK
    assert (flavour == "causal") == (len(c["cols"]) == 1) and c["cols"][-1] // T.BLOCK in (0, (L - 1) // T.BLOCK)
    assert not c["keep"][:, :, c["row"]].any() and not c["keep"][:, :, :, list(c["cols"])].any()
    assert not c["ref"]["out"][:, c["row"]].any() and not c["ref"]["gq"][:, c["row"]].any()
    for col in c["cols"]:
        assert not c["ref"]["gv"][:, col].any()
    got = T.float32_pair(c, H, flavour == "causal", c["keep"], R.DROP_P)
    T.assert_bounds(T.errors(got, c["ref"], L), (flavour, shape, "float32, given mask"))


@pytest.mark.parametrize("flavour", R.FLAVOURS)
def test_the_range_case_has_its_premises_and_float32_meets_the_bounds(flavour):
    B, L, H, dh = T.RANGE_SHAPE
    c = T.range_case(flavour)
    n_blocks = (L + T.BLOCK - 1) // T.BLOCK
    assert n_blocks == 3
    assert c["logit_std_even"] > 80.0 and c["logit_max"] > 200.0        # exp without the maximum taken off overflows at 88.7
    even = list(range(0, L, 2))
    winners = [T.range_winner(i) for i in even]
    assert len(set(winners)) == len(winners) and all(w <= i for w, i in zip(winners, even))   # distinct, seen when causal
    argmax = c["argmax"]
    assert bool((argmax[:, :, even] == torch.tensor(winners)).all())    # every large-logit row's maximum is its winner
    assert c["min_gap"] > 30.0                                          # ... by a margin float32 resolves (row 0 has one key)
    blocks = argmax // T.BLOCK
    assert set(blocks.unique().tolist()) == set(range(n_blocks))       # the row maximum falls in every key block
    # among the rows that walk more than one key block in either flavour: even rows whose maximum is in the FIRST block
    # (the running maximum stays afterwards) and even rows whose maximum is in a LATER one (it rises), the last included
    late = [i for i in even if i >= T.BLOCK]
    assert bool((blocks[:, :, late] == 0).any()) and bool((blocks[:, :, late] == 1).any())
    assert bool((blocks[:, :, late] == n_blocks - 1).any())
    got = T.float32_pair(c, H, flavour == "causal")
    for n in T.NAMES:
        assert torch.isfinite(got[n]).all(), n
    T.assert_bounds(T.errors(got, c["ref"], L), (flavour, T.RANGE_SHAPE, "float32, largest |logit|", c["logit_max"]))


@pytest.mark.parametrize("flavour", R.FLAVOURS)
def test_float32_meets_the_bounds_on_the_repeatability_shape(flavour):
    B, L, H, dh = T.REPEAT_SHAPE
    c = T.drawn_case(flavour, T.REPEAT_SHAPE)
    got = T.float32_pair(c, H, flavour == "causal", c["calls"][0]["keep"], R.DROP_P)
    T.assert_bounds(T.errors(got, c["calls"][0]["ref"], L), (flavour, T.REPEAT_SHAPE, "float32"))


def test_the_three_model_set_has_long_sequences_and_lets_the_sampler_finish():
    """the reference's sampler redraws a row's negatives until they miss all of the row's inputs: the chance of one draw
    must not vanish, or the epoch never starts"""
    import math
    import random
    from selfrec_amd.data.sequence import Sequence
    from selfrec_amd.util.sampler import next_batch_sequence
    train, test = T.long_sequences()
    assert len(train) == T.LONG_SEQ[0] and sum(len(s) > T.MODEL_MAX_LEN for s in train.values()) >= 10
    data = Sequence({}, train, test)
    chance = 1.0
    for _, ids in data.original_seq:
        inputs = ids[-T.MODEL_MAX_LEN:-1]                              # (util/sampler._window: a longer row is cut to max_len - 1)
        free = data.item_num - len(set(inputs))
        chance = min(chance, math.comb(free, len(inputs)) / math.comb(data.item_num, len(inputs)))
    assert chance >= 0.05, chance
    random.seed(1)
    batches = list(next_batch_sequence(data, 32, max_len=T.MODEL_MAX_LEN))
    assert len(batches) == 3 and all(b[0].shape[1] == T.MODEL_MAX_LEN for b in batches)
    assert max(int(b[4].max()) for b in batches) == T.MODEL_MAX_LEN - 1     # rows cut to the window: the kernel sees L = 80


def test_attention_kernel_routes_by_length():
    """the default the measurement chose (profiles/seq_attn_tiled_probe.json: the tiled kernels are not
    faster than torch's expression at L = 200 without a mask): above 64 positions the route 'hip' stays on torch's
    expression and the explicit route 'tiled' takes the tiled kernels"""
    from selfrec_amd.model.sequential.encoder import SeqEncoder
    from selfrec_amd.model.sequential.SASRec import attention_route
    torch.manual_seed(0)
    lengths = (12, 64, 65, 200, 512, 513)
    enc = SeqEncoder(20, 520, 64, 1, 1, 0.2)
    assert [enc.attention_kernel(L) for L in lengths] == ["resident", "resident", None, None, None, None]
    tiled = SeqEncoder(20, 520, 64, 1, 1, 0.2, attention="tiled")
    assert [tiled.attention_kernel(L) for L in lengths] == ["resident", "resident", "tiled", "tiled", "tiled", None]
    assert enc.uses_kernel(64) and not enc.uses_kernel(65)
    for e in (enc, tiled):
        assert all(e.attention_kernel(L, on_device=False) is None for L in lengths)
    torch_route = SeqEncoder(20, 520, 64, 1, 1, 0.2, attention="torch")
    assert all(torch_route.attention_kernel(L) is None for L in lengths)
    assert SeqEncoder(20, 520, 64, 1, 1, 0.2, attention="tiled", causal=False).attention_kernel(200) == "tiled"
    assert SeqEncoder(20, 520, 48, 1, 1, 0.2, attention="tiled").attention_kernel(200) is None    # a head width no kernel serves

    class Conf(dict):
        contain = dict.__contains__
    assert attention_route(Conf({"engine.attention": "tiled"})) == "tiled" and attention_route(Conf()) == "hip"
    with pytest.raises(ValueError):
        attention_route(Conf({"engine.attention": "flash"}))


def test_the_committed_probe_chose_the_default_the_routing_has():
    """the issue's rule: tiled is the default above 64 only if its median is at or below torch's at L = 100 and L = 200 in
    both flavours; the committed measurement says it is not, and the encoder follows it"""
    import json
    from selfrec_amd.model.sequential.encoder import SeqEncoder
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(repo, "profiles", "seq_attn_tiled_probe.json")) as f:
        probe = json.load(f)
    holds = all(probe["core"][f"L{L}_{fl}"]["fwd_bwd_ms"]["tiled"]["median"]
                <= probe["core"][f"L{L}_{fl}"]["fwd_bwd_ms"]["torch"]["median"] for L in (100, 200) for fl in R.FLAVOURS)
    assert holds == probe["default_rule"]["holds"]
    torch.manual_seed(0)
    assert (SeqEncoder(20, 520, 64, 1, 1, 0.2).attention_kernel(200) == "tiled") == holds


def test_the_new_names_are_public_and_the_old_envelope_stands():
    from selfrec_amd import _lib, ops
    for name in ("SEQ_ATTN_TILED_MAX_LEN", "seq_attn_tiled_supported", "seq_attn_tiled_fwd", "seq_attn_tiled_bwd",
                 "SeqAttnTiledFn"):
        assert name in ops.__all__ and hasattr(ops, name), name
    assert ops.SEQ_ATTN_TILED_MAX_LEN == 512 and ops.SEQ_ATTN_MAX_LEN == 64
    assert not ops.seq_attn_supported(65, 1, 64)
    for name in ("srh_seq_attn_tiled_fwd_f32", "srh_seq_attn_tiled_bwd_f32"):
        assert name in _lib.SIGNATURES
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "selfrec_hip.h")) as f:
        header = f.read()
    assert "(a-25)" in header and "srh_seq_attn_tiled_fwd_f32(" in header and "srh_seq_attn_tiled_bwd_f32(" in header


def test_seq_attn_tiled_supported_at_its_corners():
    from selfrec_amd import ops
    ok = ops.seq_attn_tiled_supported
    assert ok(1, 1, 32) and ok(512, 1, 64) and ok(512, 2, 64) and ok(512, 4, 32) and ok(65, 3, 32) and ok(64, 1, 64)
    assert not ok(0, 1, 64) and not ok(513, 1, 64)
    assert not ok(200, 1, 16) and not ok(200, 1, 48) and not ok(200, 1, 128)
    assert not ok(200, 3, 64) and not ok(200, 5, 32) and not ok(200, 0, 64)
