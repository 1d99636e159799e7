"""The GRU recurrence without a GPU: the float64 restatement (tests/gru_ref.py) against float64 autograd of
torch.nn.GRU(...)[0] * live, the header and the exported symbols, the refusals the library answers on the host, the length
check of ops, and the admissibility of the GPU tests' bounds (float32 arithmetic stays inside half of each)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import gru_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRADS = ("dx", "dw_ih", "dw_hh", "db_ih", "db_hh")


@pytest.mark.parametrize("shape", R.AUTOGRAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_restatement_equals_float64_autograd(shape):
    B, L, H = shape
    g = torch.Generator().manual_seed(B * L + H)
    k = 1.0 / H ** 0.5
    uni = lambda *s: (torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1) * k  # noqa: E731
    x, go = torch.randn(B, L, H, generator=g, dtype=torch.float64), torch.randn(B, L, H, generator=g, dtype=torch.float64)
    params = (uni(3 * H, H), uni(3 * H, H), uni(3 * H), uni(3 * H))
    lens = R.lengths(B, L, "ragged")
    assert lens.min() == 1 and lens.max() == L
    mine, theirs = R.gru_layer(x, *params, lens, go), R.torch_layer(x, *params, lens, go)
    for name in ("out",) + GRADS:
        assert R.rel_err(mine[name], theirs[name]) <= 1e-12, name


def test_restatement_ignores_dead_inputs_and_writes_zeros():
    c = R.case(17, 33, 64, "zero")
    dead = R.dead_mask(c["lens"], 33)
    assert dead.any() and (c["lens"] == 0).any()
    go = c["go"].clone()
    go[dead] = float("nan")
    ref = c["ref"]
    dgi, dghn = R.gru_bwd(go, ref["out"], ref["gates"], c["w_hh"].double(), c["lens"])
    assert torch.equal(dgi, ref["dgi"]) and torch.equal(dghn, ref["dghn"])
    for name in ("out", "gates", "dgi", "dghn"):
        assert float(ref[name][dead].abs().max()) == 0.0, name


def test_header_signatures_and_exports():
    from selfrec_amd import _lib, ops
    header = open(os.path.join(REPO, "include", "selfrec_hip.h")).read()
    assert "(a-26)" in header and f"#define SRH_ABI_VERSION {_lib.ABI_VERSION}" in header and _lib.ABI_VERSION == 31
    section = header[header.index("(a-26)"):]
    lib = _lib.load()
    for name in ("srh_gru_fwd_f32", "srh_gru_bwd_f32"):
        assert name + "(" in section and name in _lib.SIGNATURES and hasattr(lib, name)
    for name in ("GRU_WIDTH", "GRU_MAX_LEN", "gru_supported", "gru_lengths", "gru_fwd", "gru_bwd", "gru_pad_params", "GruFn",
                 "GatherLiveRowsFn"):
        assert name in ops.__all__ and hasattr(ops, name), name
    assert ops.gru_supported(1, 64) and ops.gru_supported(512, 64) and ops.gru_supported(12, 32)
    assert not ops.gru_supported(513, 64) and not ops.gru_supported(0, 64) and not ops.gru_supported(50, 96)
    assert not ops.gru_supported(50, 128)
    makefile = open(os.path.join(REPO, "selfrec_amd", "csrc", "Makefile")).read()
    assert " gru.hip" in makefile


def test_refusals_come_before_any_launch():
    """bad shapes and null pointers are answered on the host: nothing below reaches a kernel (no device is needed)"""
    from selfrec_amd import _lib
    lib = _lib.load()
    fake = C.c_void_p(4096)
    fwd = lambda B=4, L=8, H=64, gi=fake, w=fake, b=fake, ln=fake, out=fake: lib.srh_gru_fwd_f32(  # noqa: E731
        gi, w, b, ln, B, L, H, out, None, None)
    bwd = lambda B=4, L=8, H=64, go=fake, out=fake, gates=fake, w=fake, ln=fake, dgi=fake, dghn=fake: (  # noqa: E731
        lib.srh_gru_bwd_f32(go, out, gates, w, ln, B, L, H, dgi, dghn, None))
    for call in (fwd, bwd):
        assert call(H=96) == -3 and b"H=96 unsupported" in lib.srh_last_error_string()
        assert call(H=128) == -3 and call(H=32) == -3
        assert call(L=513) == -3 and b"L=513 unsupported" in lib.srh_last_error_string()
        assert call(L=0) == -3
        assert call(B=0) == -1 and b"bad B" in lib.srh_last_error_string()
    for arg in ("gi", "w", "b", "ln", "out"):
        assert fwd(**{arg: None}) == -1 and b"null" in lib.srh_last_error_string(), arg
    odd = C.c_void_p(4100)
    assert fwd(w=odd) == -1 and b"aligned" in lib.srh_last_error_string() and fwd(out=odd) == -1
    assert bwd(dgi=odd) == -1 and b"aligned" in lib.srh_last_error_string() and bwd(dghn=odd) == -1
    for arg in ("go", "out", "gates", "w", "ln", "dgi", "dghn"):
        assert bwd(**{arg: None}) == -1 and b"null" in lib.srh_last_error_string(), arg


def test_ops_checks_host_lengths_before_anything_is_uploaded():
    """the library never copies the lengths back, so 0 <= len <= L is the caller's contract there (header (a-26)); ops
    checks a host array"""
    from selfrec_amd import ops
    for bad in ([1, 2, 9], [0, -1, 3], [1, 2]):
        with pytest.raises(ops.SelfrecHipError):
            ops.gru_lengths(np.asarray(bad), 3, 8, "cpu")
    assert ops.gru_lengths(np.asarray([0, 8, 3]), 3, 8, "cpu").tolist() == [0, 8, 3]
    assert ops.gru_lengths([0, 8, 3], 3, 8, "cpu").dtype == torch.int32


def test_padded_parameters_keep_a_padded_unit_at_zero():
    from selfrec_amd import ops
    c = R.case(4, 12, 32, "ragged")
    w_ih, w_hh, b_ih, b_hh = ops.gru_pad_params(c["w_ih"], c["w_hh"], c["b_ih"], c["b_hh"])
    assert w_ih.shape == (192, 32) and w_hh.shape == (192, 64) and b_ih.shape == (192,) and b_hh.shape == (192,)
    out, gates = R.gru_fwd(c["x"].double() @ w_ih.double().T + b_ih.double(), w_hh, b_hh, c["lens"])
    assert float(out[..., 32:].abs().max()) == 0.0
    assert R.rel_err(out[..., :32], c["ref"]["out"]) <= 1e-15
    go = torch.zeros(4, 12, 64, dtype=torch.float64)
    go[..., :32] = c["go"]
    dgi, dghn = R.gru_bwd(go, out, gates, w_hh, c["lens"])
    assert float(dgi.reshape(4, 12, 3, 64)[..., 32:].abs().max()) == 0.0 and float(dghn[..., 32:].abs().max()) == 0.0
    assert R.rel_err(dgi.reshape(4, 12, 3, 64)[..., :32].reshape(4, 12, 96), c["ref"]["dgi"]) <= 1e-15


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_float32_arithmetic_is_inside_half_of_each_bound(shape):
    """admissibility of the GPU tests' bounds on every GPU case: the restatement in float32 (all four kernel outputs and the
    finish) and float32 torch.nn.GRU autograd (out and the five gradients) against the float64 restatement"""
    worst = dict(out=0.0, grad=0.0)
    for (B, L, H, pattern, scale) in [c for c in R.cases() if c[:3] == shape]:
        c = R.case(B, L, H, pattern, scale)
        ref = c["ref"]
        args = (c["x"], c["w_ih"], c["w_hh"], c["b_ih"], c["b_hh"], c["lens"], c["go"])
        f32, tf32 = R.gru_layer(*args, dtype=torch.float32), R.torch_layer(*args, dtype=torch.float32)
        for name in ("out", "gates"):
            worst["out"] = max(worst["out"], R.rel_err(f32[name], ref[name]))
        worst["out"] = max(worst["out"], R.rel_err(tf32["out"], ref["out"]))
        for name in ("dgi", "dghn") + GRADS:
            worst["grad"] = max(worst["grad"], R.rel_err(f32[name], ref[name]))
        for name in GRADS:
            worst["grad"] = max(worst["grad"], R.rel_err(tf32[name], ref[name]))
    print(shape, worst)
    assert worst["out"] <= R.OUT_BOUND / 2 and worst["grad"] <= R.GRAD_BOUND / 2, worst
