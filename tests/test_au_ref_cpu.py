"""The premises of tests/au_ref.py and tests/au_cases.py and the host side of the DirectAU loss kernels (include/selfrec_hip.h
(a-22), csrc/au.hip): no GPU needed."""
import ctypes as C
import os

import pytest
import torch

from selfrec_amd import _lib
from tests import au_cases as K
from tests import au_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return K.cpu_cases()


@pytest.fixture(scope="module")
def refs(cases):
    """float64 autograd on the reference's expression, once per case"""
    return [R.reference(c["x"], c["y"], c["t"], c["w"]) for c in cases]


def _scales(c):
    if c["cancel_x"] is None and c["cancel_y"] is None:
        return None, None
    return R.cancel_scales(c["x"], c["y"], c["t"], c["w"])


def _worst(c, got, want, floor):
    """the worst row of both gradients of a case under grad_errors"""
    sx, sy = _scales(c)
    ex = R.grad_errors(got[2], want[2], R.clamped_rows(c["x"]), c["cancel_x"], sx, floor)
    ey = R.grad_errors(got[3], want[3], R.clamped_rows(c["y"]), c["cancel_y"], sy, floor)
    return max(float(ex.max()), float(ey.max()))


def test_closed_form_is_the_reference_expression(cases, refs):
    worst = 0.0
    for c, want in zip(cases, refs):
        got = R.closed_form(c["x"], c["y"], c["t"], c["w"])
        assert abs(float(got[0] - want[0])) <= 1e-12 * max(1.0, abs(float(want[0]))), c["name"]
        assert ((got[1] - want[1]).abs() <= 1e-12 * want[1].abs().clamp_min(1.0)).all(), c["name"]
        e = _worst(c, got, want, 1e-3)
        worst = max(worst, e)
        assert e <= 1e-12, (c["name"], e)
    print("closed form against float64 autograd, worst row:", worst)
    # the one-sided form
    c = cases[-1]
    got, want = R.closed_form(c["x"], None, 0.5, (0.0, 1.5, 0.0)), R.reference(c["x"], None, 0.5, (0.0, 1.5, 0.0))
    assert abs(float(got[0] - want[0])) <= 1e-12 and got[3] is None and want[3] is None
    assert float(R.grad_errors(got[2], want[2], R.clamped_rows(c["x"]), floor_frac=1e-3).max()) <= 1e-12


def test_case_premises(cases, refs):
    by_name = {c["name"]: (c, r) for c, r in zip(cases, refs)}
    for n, d in K.DEGENERATE_SHAPES:
        c, (loss, parts, gx, gy) = by_name[f"degenerate-n{n}-d{d}"]
        x, y, g = c["x"], c["y"], K.DEG
        assert torch.isfinite(loss) and torch.isfinite(gx).all() and torch.isfinite(gy).all()
        assert torch.equal(x[g["dup_x"][0]], x[g["dup_x"][1]]) and torch.equal(y[g["dup_y"][0]], y[g["dup_y"][1]])
        assert torch.equal(x[g["equal"]], y[g["equal"]])
        cl_x, cl_y = R.clamped_rows(x), R.clamped_rows(y)
        assert cl_x.nonzero().flatten().tolist() == [g["zero_x"], g["near_x"]]
        assert cl_y.nonzero().flatten().tolist() == [g["tiny_y"], n - 1]
        for m, r in ((x, g["near_x"]), (y, n - 1)):          # just below the clamp, in float32 as in float64
            assert 0.7e-12 < float(m[r].norm()) < 0.9e-12 and 0.7e-12 < float(m[r].double().norm()) < 0.9e-12
        # the clamped rows' gradients are twelve orders above the others; the near-clamp rows tell the two backwards apart
        for grad, cl in ((gx, cl_x), (gy, cl_y)):
            big = grad.abs().amax(1)
            assert (big[cl] > 1e8).all() and (big[~cl] < 1e3).all()
        for grad, m, r in ((gx, x, g["near_x"]), (gy, y, n - 1)):
            h = m[r].double() / 1e-12
            assert float((h * (h @ grad[r])).abs().max()) > 1e-2 * float(grad[r].abs().max())
        # a cancelling row's alignment gradient is zero (the 1e-20 row normalises to 1e-8 entries, which its partner keeps):
        # what is left is far below GRAD_TOL of what cancels
        sx, sy = R.cancel_scales(x, y, c["t"], (1.0, 0.0, 0.0))
        wa = R.reference(x, y, c["t"], (1.0, 0.0, 0.0))
        assert (wa[2][c["cancel_x"]].abs().amax(1) <= 1e-6 * sx[c["cancel_x"]]).all()
        assert (wa[3][c["cancel_y"]].abs().amax(1) <= 1e-12 * sy[c["cancel_y"]]).all()
        c, (loss, parts, gx, gy) = by_name[f"identical-n{n}-d{d}"]
        assert float(parts[1]) == 0.0                          # U(x) = 0 exactly
        ux = R.reference(c["x"], c["y"], c["t"], (0.0, 1.0, 0.0))
        assert float(ux[2].abs().max()) == 0.0
        c, (loss, parts, gx, gy) = by_name[f"antipodal-n{n}-d{d}"]
        assert float(parts[0]) > 3.9 and torch.isfinite(gx).all()
    # duplicates are the normal case of the batch-shaped rows
    c = by_name["n129-d64-t2.0"][0]
    assert len(torch.unique(c["x"], dim=0)) < 129 and len(torch.unique(c["y"], dim=0)) < 129


def test_header_section_and_bindings():
    text = open(os.path.join(REPO, "include", "selfrec_hip.h")).read()
    assert "(a-22) DirectAU" in text and "model/graph/DirectAU.py:37-48" in text
    assert text.index("(a-22) DirectAU") < text.index("(a-20) MHCN")
    for name in ("srh_au_ws_bytes", "srh_au_chunk_plan", "srh_au_fwd_bwd"):
        assert name in _lib.SIGNATURES and name in text[text.index("(a-22) DirectAU"):text.index("(a-20) MHCN")]
    assert _lib.ABI_VERSION == 31 and "#define SRH_ABI_VERSION 31" in text


def test_workspace_size_and_chunk_plan_answer_on_the_host():
    lib = _lib.load()
    assert lib.srh_au_ws_bytes(2048, 96) == 0 and lib.srh_au_ws_bytes(1, 64) == 0 and lib.srh_au_ws_bytes(1 << 24, 64) == 0
    for d in (64, 128):
        for n in (2, 65, 2048, 16384):
            got = lib.srh_au_ws_bytes(n, d)
            assert got > 0 and got % 256 == 0
            # at least the documented arrays: two normalised copies and the per-chunk partials of both sides
            p = R.chunk_plan(n)
            assert got >= 2 * 4 * n * d + 2 * p["chunks"] * (4 * n * d + 8 * n)
    a, b = C.c_int64(), C.c_int64()
    for n in sorted({*K.TILE_N, *(s[0] for s in K.CHUNK_SHAPES), K.LARGE_SHAPE[0], 1088, 1089, 16320, 16321, (1 << 24) - 1}):
        assert lib.srh_au_chunk_plan(n, C.byref(a), C.byref(b)) == 0
        p = R.chunk_plan(n)
        assert (a.value, b.value) == (p["chunks"], p["chunk_len"]), n
        assert p["chunks"] * p["chunk_len"] >= n and p["live"] >= 1
    assert lib.srh_au_chunk_plan(1, C.byref(a), C.byref(b)) == -1 and b"au_chunk_plan" in lib.srh_last_error_string()


def test_refusals_come_before_any_launch():
    """bad arguments are answered on the host: nothing below reaches a kernel (no device is needed)"""
    lib = _lib.load()
    fake = C.c_void_p(4096)
    args = lambda n, d, t=2.0, x=fake: (x, fake, n, d, t, 1.0, 1.0, 1.0, fake, fake, fake, fake, fake, None)  # noqa: E731
    assert lib.srh_au_fwd_bwd(*args(65, 96)) == -3 and b"d=96 unsupported" in lib.srh_last_error_string()
    assert lib.srh_au_fwd_bwd(*args(1, 64)) == -1 and b"no pair" in lib.srh_last_error_string()
    assert lib.srh_au_fwd_bwd(*args(65, 64, t=0.0)) == -1 and b"positive" in lib.srh_last_error_string()
    assert lib.srh_au_fwd_bwd(*args(65, 64, t=float("inf"))) == -1
    assert lib.srh_au_fwd_bwd(*args(65, 64, x=None)) == -1 and b"null" in lib.srh_last_error_string()
    assert lib.srh_au_fwd_bwd(fake, fake, 65, 64, 2.0, 1.0, 1.0, 1.0, fake, fake, fake, None, fake, None) == -1


def test_chunk_layouts_the_cases_reach():
    plan = R.chunk_plan
    assert plan(64)["chunks"] == 1 and plan(2)["chunks"] == 1                       # one chunk
    p = plan(128)
    assert (p["chunks"], p["last_keys"], p["empty"]) == (2, 64, 0)                   # the last chunk holds one tile
    for n in (65, 129, 257):                                                        # ... a single row
        assert plan(n)["last_keys"] == 1 and plan(n)["empty"] == 0
    p = plan(1025)
    assert (p["chunks"], p["chunk_len"], p["empty"], p["last_keys"]) == (16, 128, 7, 1)     # trailing empty chunks
    p = plan(2048)
    assert (p["chunks"], p["chunk_len"], p["empty"], p["last_keys"]) == (8, 256, 0, 256)
    p = plan(2049)
    assert (p["chunks"], p["chunk_len"], p["empty"], p["last_keys"]) == (8, 320, 1, 129)
    p = plan(4100)
    assert (p["chunks"], p["chunk_len"], p["empty"]) == (4, 1088, 0)
    p = plan(K.LARGE_SHAPE[0])
    assert (p["chunks"], p["tiles"]) == (1, 256)                                    # one chunk of many tiles


def test_au_route(monkeypatch):
    from selfrec_amd.model.graph import DirectAU as M
    from selfrec_amd.util.conf import ModelConf
    monkeypatch.delenv("SRH_DIRECTAU_AU", raising=False)
    assert M.au_route(None) == "hip" and M.au_route(ModelConf({})) == "hip"          # the faster route of the A/B
    assert M.au_route(ModelConf({"engine.au": "torch"})) == "torch" and M.au_route(ModelConf({"engine.au": "Hip "})) == "hip"
    monkeypatch.setenv("SRH_DIRECTAU_AU", "hip")
    assert M.au_route(ModelConf({"engine.au": "torch"})) == "hip"
    monkeypatch.setenv("SRH_DIRECTAU_AU", "torch")
    assert M.au_route(ModelConf({"engine.au": "hip"})) == "torch"
    monkeypatch.delenv("SRH_DIRECTAU_AU")
    with pytest.raises(ValueError):
        M.au_route(ModelConf({"engine.au": "triton"}))


def test_au_supported_and_the_model_docstring():
    from selfrec_amd import ops
    from selfrec_amd.model.graph import DirectAU as M
    assert ops.au_supported(64) and ops.au_supported(128) and ops.au_supported(50) and ops.au_supported(2)
    assert not ops.au_supported(129) and not ops.au_supported(256) and not ops.au_supported(0)
    assert "engine.au" in M.__doc__


def test_floor_frac_is_the_smallest_that_float32_torch_meets(cases, refs):
    """DESIGN.md 4.15's rule: the reference's own expression in plain float32 torch on the CPU, every case, clamped and
    ordinary rows each on their own, cancelling rows by cancel_scales"""
    worst = {f: 0.0 for f in R.FLOORS}
    worst_loss = 0.0
    for c, want in zip(cases, refs):
        got = R.reference(c["x"], c["y"], c["t"], c["w"], dtype=torch.float32)
        worst_loss = max(worst_loss, abs(float(got[0]) - float(want[0])) / (R.loss_bound(want[1], c["w"]) / R.LOSS_TOL))
        for f in R.FLOORS:
            worst[f] = max(worst[f], _worst(c, got, want, f))
    print("float32 torch against float64, worst per-row gradient error by floor:", worst, "loss:", worst_loss)
    passing = [f for f in R.FLOORS if worst[f] <= R.GRAD_TOL / 2]
    assert passing and R.FLOOR_FRAC == min(passing), worst
    assert worst_loss <= R.LOSS_TOL / 2
