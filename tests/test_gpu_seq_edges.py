"""The sequence kernels of csrc/seqrec.hip at their edges, against float64 (tests/seq_attn_ref.py):

* the DRAWN dropout route of both attention flavours -- the one training takes --, forward and backward, at every L around
  a 16-row tile edge and every head layout of the envelope, with per-row counters that cross the 32-bit carry, against the
  float64 restatement under the host's restatement of the mask, and bit for bit against the injected-mask route;
* injected masks with a whole query row and a whole key column dropped;
* logits far past the point where an exp without the row maximum taken off overflows float32;
* the BCE kernel at widths below, off and above its 64-lane stride and row counts off its 4-row blocks and around the 256
  threads of its reduction, with item ids outside the table, and its refusal of an impossible n_valid.

Bounds: outputs, lse and losses <= 1e-5, gradients <= 1e-4, each of its tensor's largest magnitude."""
import numpy as np
import pytest
import torch

from tests import seq_attn_ref as R

pytestmark = pytest.mark.gpu

NAMES = ("out", "lse", "gq", "gk", "gv")
BOUND = dict(out=1e-5, lse=1e-5, gq=1e-4, gk=1e-4, gv=1e-4)
SHAPE_ID = lambda s: "B%d_L%d_H%d_dh%d" % s  # noqa: E731


def rel_err(got, want):
    """largest error as a fraction of the tensor's largest magnitude"""
    want = want.double().cpu()
    return float((got.double().cpu() - want).abs().max() / want.abs().max().clamp_min(1e-300))


def entry_points(flavour):
    from selfrec_amd import ops
    return (ops.seq_attn_fwd, ops.seq_attn_bwd) if flavour == "causal" else (ops.seq_attn_full_fwd, ops.seq_attn_full_bwd)


def run_pair(flavour, c, H, **kw):
    """one forward / backward pair on the device: {out, lse, gq, gk, gv}"""
    fwd, bwd = entry_points(flavour)
    dev = torch.device("cuda:0")
    q, k, v, go = (c[n].to(dev) for n in ("q", "k", "v", "go"))
    if kw.get("keep") is not None:
        kw["keep"] = torch.as_tensor(kw["keep"]).to(dev)
    out, lse = fwd(q, k, v, H, **kw)
    return dict(zip(NAMES, (out, lse) + tuple(bwd(q, k, v, lse, go, H, **kw))))


def errors(got, ref, L):
    """the five relative errors; at L = 1 the softmax of one key is the constant 1, dQ = dK = 0 in exact arithmetic, and the
    kernel must return exact zeros"""
    errs = {n: rel_err(got[n], ref[n]) for n in NAMES}
    if L == 1:
        assert not ref["gq"].any() and not ref["gk"].any() and not got["gq"].any() and not got["gk"].any()
        errs["gq"] = errs["gk"] = 0.0
    return errs


def assert_bounds(errs, what):
    print(what, errs)
    for n in NAMES:
        assert errs[n] <= BOUND[n], (what, n, errs)


DRAWN_CASES = [(f, s) for f in R.FLAVOURS for s in R.drawn_shapes(f)]


@pytest.mark.parametrize("flavour,shape", DRAWN_CASES, ids=lambda x: x if isinstance(x, str) else SHAPE_ID(x))
def test_drawn_dropout_forward_and_backward_match_float64_and_the_given_mask_route(flavour, shape):
    """two consecutive calls at the counters 2^32 - 5 and 2^32 - 5 + B H L (the rows from the sixth on draw at counters past
    the 32-bit carry -- inside the first call wherever it has six rows, inside the second otherwise): each meets the bounds
    against float64 under the HOST's mask for its counter, and the first equals the injected-mask route under that mask bit
    for bit in all five tensors -- the two routes differ only in where the multiplier comes from, and a column without a
    key (>= L, or above the diagonal) carries P = 0 in both"""
    B, L, H, dh = shape
    c = R.drawn_case(flavour, shape)
    first, second = c["calls"]
    assert first["counter"] < 2 ** 32 < second["counter"] + B * H * L and second["counter"] == first["counter"] + B * H * L
    assert not np.array_equal(first["keep"], second["keep"])              # the second call draws another mask
    for call in (first, second):
        got = run_pair(flavour, c, H, drop_p=R.DROP_P, rng_seed=R.SEED, rng_counter=call["counter"])
        assert_bounds(errors(got, call["ref"], L), (flavour, shape, "drawn at", call["counter"]))
        if call is first:
            given = run_pair(flavour, c, H, keep=call["keep"], drop_p=R.DROP_P)
            differ = [n for n in NAMES if not torch.equal(got[n], given[n])]
            assert not differ, (flavour, shape, "drawn and given differ in", differ)


@pytest.mark.parametrize("shape", R.KEEP_EDGE_SHAPES, ids=SHAPE_ID)
@pytest.mark.parametrize("flavour", R.FLAVOURS)
def test_a_dropped_query_row_and_a_dropped_key_column_leave_exact_zeros(flavour, shape):
    """every dp of a query row that keeps nothing is 0, so delta and dS are: out and gq of the row are exact zeros; a key
    nobody keeps takes no dV; everything else meets the bounds"""
    B, L, H, dh = shape
    c = R.keep_edge_case(flavour, shape)
    got = run_pair(flavour, c, H, keep=c["keep"], drop_p=R.DROP_P)
    assert not c["ref"]["out"][:, c["row"]].any() and not c["ref"]["gq"][:, c["row"]].any()
    assert not c["ref"]["gv"][:, c["col"]].any()
    assert not got["out"][:, c["row"]].any() and not got["gq"][:, c["row"]].any()
    assert not got["gv"][:, c["col"]].any()
    assert_bounds(errors(got, c["ref"], L), (flavour, shape, "row", c["row"], "col", c["col"]))


@pytest.mark.parametrize("flavour", R.FLAVOURS)
def test_logits_of_a_hundred_standard_deviations_stay_finite_and_inside_the_bounds(flavour):
    B, L, H, dh = R.RANGE_SHAPE
    c = R.range_case(flavour)
    assert c["logit_max"] > 200.0
    got = run_pair(flavour, c, H)
    for n in NAMES:
        assert torch.isfinite(got[n]).all(), n
    assert_bounds(errors(got, c["ref"], L), (flavour, R.RANGE_SHAPE, "largest |logit|", c["logit_max"]))


# ---- the BCE kernel ---------------------------------------------------------------------------------------------------------
def bce_errors(c, loss2, gh, grows):
    got = loss2.cpu().numpy()
    return dict(lp=abs(got[0] - c["lp"]) / abs(c["lp"]), ln=abs(got[1] - c["ln"]) / abs(c["ln"]),
                gh=rel_err(gh, c["gh"]), grows=rel_err(grows, c["grows"]))


@pytest.mark.parametrize("R_,d", R.BCE_EDGE_CASES, ids=lambda x: str(x))
def test_bce_kernel_matches_float64_at_every_width_and_row_count(R_, d):
    from selfrec_amd import ops
    c = R.bce_edge_case(R_, d)
    if R_ >= 255:
        assert c["span"] > 30.0                                      # (3 or 5 rows of standard deviation 24 need not get there)
    dev = torch.device("cuda:0")
    hidden, table = c["hidden"].to(dev), c["table"].to(dev)
    pos, neg = c["pos"].to(dev, torch.int32), c["neg"].to(dev, torch.int32)
    loss2, gh, grows = ops.seq_bce_fwd_bwd(hidden, table, pos, neg, c["valid"].to(dev, torch.uint8))
    errs = bce_errors(c, loss2, gh, grows)
    # the table gradient behind it: the segment sum serves every width
    plan = ops.scatter_plan(np.concatenate([c["pos"].numpy(), c["neg"].numpy()]), dev)
    gt = ops.rows_segment_sum(grows, plan, torch.zeros_like(table))
    errs["gt"] = rel_err(gt, c["gt"])
    print((R_, d), "span", c["span"], errs)
    assert errs["lp"] <= 1e-5 and errs["ln"] <= 1e-5, errs
    assert errs["gh"] <= 1e-4 and errs["grows"] <= 1e-4 and errs["gt"] <= 1e-4, errs
    invalid = ~c["valid"].to(dev)
    assert not gh[invalid].any() and not grows[:R_][invalid].any() and not grows[R_:][invalid].any()


def test_bce_rows_with_ids_outside_the_table_take_exact_zeros():
    """a row marked valid whose pos or neg lies outside [0, n_table) is treated as invalid (include/selfrec_hip.h): exact
    zeros in gh and in both of its grows rows, nothing in the loss; n_valid is the caller's count of the usable rows"""
    from selfrec_amd import ops
    c = R.bce_bad_id_case()
    dev = torch.device("cuda:0")
    n_rows = c["hidden"].shape[0]
    n_usable = int(c["usable"].sum())
    assert n_usable == 7 and int(c["valid"].sum()) == n_usable + len(c["bad_rows"])
    loss2, gh, grows = ops.seq_bce_fwd_bwd(c["hidden"].to(dev), c["table"].to(dev), c["pos"].to(dev, torch.int32),
                                           c["neg"].to(dev, torch.int32), c["valid"].to(dev, torch.uint8), n_valid=n_usable)
    for r in c["bad_rows"]:
        assert not gh[r].any() and not grows[r].any() and not grows[n_rows + r].any(), r
    errs = bce_errors(c, loss2, gh, grows)
    print("ids outside the table", errs)
    assert errs["lp"] <= 1e-5 and errs["ln"] <= 1e-5, errs
    assert errs["gh"] <= 1e-4 and errs["grows"] <= 1e-4, errs


def test_bce_refuses_an_impossible_n_valid_before_any_launch():
    """n_valid = 0 and n_valid = R + 1: SRH_ERR_INVALID_ARG (-1) with a message, and none of the outputs is touched"""
    from selfrec_amd import _lib, ops
    lib = _lib.load()
    c = R.bce_edge_case(5, 65)
    dev = torch.device("cuda:0")
    n_rows, d = c["hidden"].shape
    hidden, table = c["hidden"].to(dev), c["table"].to(dev)
    pos, neg = c["pos"].to(dev, torch.int32), c["neg"].to(dev, torch.int32)
    valid = c["valid"].to(dev, torch.uint8)
    ws = torch.zeros(int(lib.srh_seq_bce_ws_bytes(n_rows)), dtype=torch.uint8, device=dev)
    for n_valid in (0, n_rows + 1):
        loss2 = torch.full((2,), 7.0, dtype=torch.float64, device=dev)
        gh = torch.full((n_rows, d), 7.0, device=dev)
        grows = torch.full((2 * n_rows, d), 7.0, device=dev)
        status = lib.srh_seq_bce_fwd_bwd(hidden.data_ptr(), n_rows, d, table.data_ptr(), table.shape[0], pos.data_ptr(),
                                         neg.data_ptr(), valid.data_ptr(), n_valid, loss2.data_ptr(), gh.data_ptr(),
                                         grows.data_ptr(), ws.data_ptr(), None)
        assert status == -1
        with pytest.raises(ops.SelfrecHipError, match=r"\(-1\).*n_valid=%d" % n_valid):
            _lib.check(status, "srh_seq_bce_fwd_bwd")
        torch.cuda.synchronize()
        assert bool((loss2 == 7.0).all()) and bool((gh == 7.0).all()) and bool((grows == 7.0).all())
        assert not ws.any()                                           # nor the workspace
        with pytest.raises(ops.SelfrecHipError, match=r"\(-1\)"):     # the wrapper passes the refusal on
            ops.seq_bce_fwd_bwd(hidden, table, pos, neg, valid, n_valid=n_valid)
