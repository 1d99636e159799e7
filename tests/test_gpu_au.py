"""The DirectAU loss kernels (csrc/au.hip; include/selfrec_hip.h (a-22)) against float64 computed on the
device by tests/au_ref.py, on the cases of tests/au_cases.py: tile and chunk edges, degenerate rows, the one-sided form, the
weights, the caller contract, AlignUniformFn through autograd, and the model on both routes.

Every kernel call here goes through `run`, which hands over a workspace and outputs pre-filled with NaN bytes: nothing
relies on the caller zeroing.  Bounds: loss and parts by au_ref.loss_bound / LOSS_TOL, gradients GRAD_TOL per row through
au_ref.grad_errors at FLOOR_FRAC."""
import random

import numpy as np
import pytest
import torch

from selfrec_amd import _lib, ops
from tests import au_cases as K
from tests import au_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN_BYTE = 0xFF      # four (eight) of them are a NaN in float32 (float64)


def _nan(shape, dtype):
    t = torch.empty(shape, dtype=dtype, device=DEV)
    t.view(torch.uint8).fill_(NAN_BYTE)
    return t


def raw(x, y, n, d, t, w, ws=None):
    """srh_au_fwd_bwd as it is: (status, out (4: loss, parts), gx, gy, ws) on NaN-filled outputs and workspace"""
    lib = _lib.load()
    out, gx, gy = _nan(4, torch.float64), _nan((n, d), torch.float32), _nan((n, d), torch.float32)
    if ws is None:
        ws = _nan(max(int(lib.srh_au_ws_bytes(n, d)), 256), torch.uint8)
    st = lib.srh_au_fwd_bwd(x.data_ptr(), None if y is None else y.data_ptr(), n, d, float(t), float(w[0]), float(w[1]),
                            float(w[2]), out[1:].data_ptr(), out.data_ptr(), gx.data_ptr(), gy.data_ptr(), ws.data_ptr(),
                            torch.cuda.current_stream().cuda_stream)
    return st, out, gx, gy, ws


def run(x, y, t, w):
    """the kernels on (x, y) of any d <= 128: rows zero-padded to the kernel width, gradients cut back"""
    n, d = x.shape
    kw = ops.kernel_width(d, ops.TABLE_NCE_WIDTHS)
    xs = ops.to_width(x.to(DEV), kw)
    ys = None if y is None else ops.to_width(y.to(DEV), kw)
    st, out, gx, gy, _ = raw(xs, ys, n, kw, t, w)
    assert st == 0, _lib.load().srh_last_error_string()
    torch.cuda.synchronize()
    if kw > d:                                      # a padded column takes no gradient
        assert float(gx[:, d:].abs().max()) == 0.0 and (y is None or float(gy[:, d:].abs().max()) == 0.0)
    return out[0], out[1:], gx[:, :d], gy[:, :d]


def want_of(c, closed=False):
    f = R.closed_form if closed else R.reference
    return f(c["x"], c["y"], c["t"], c["w"], device=DEV)


def check(c, got, want):
    """a case against its float64 results; returns the figures (loss error over its bound, worst row of gx, of gy)"""
    w, one = c["w"], c["y"] is None
    loss, parts, gx, gy = got
    le = abs(float(loss) - float(want[0])) / R.loss_bound(want[1], w, one)
    for k in ((1,) if one else (0, 1, 2)):
        pe = abs(float(parts[k]) - float(want[1][k])) / (R.LOSS_TOL * max(1.0, abs(float(want[1][k]))))
        assert pe <= 1.0, (c["name"], "part", k, float(parts[k]), float(want[1][k]))
    sx, sy = (None, None) if c["cancel_x"] is None and c["cancel_y"] is None else R.cancel_scales(c["x"], c["y"], c["t"], w)
    ex = float(R.grad_errors(gx, want[2], R.clamped_rows(c["x"]), c["cancel_x"], sx).max())
    ey = 0.0 if one else float(R.grad_errors(gy, want[3], R.clamped_rows(c["y"]), c["cancel_y"], sy).max())
    print(f"{c['name']}: loss {le * R.LOSS_TOL:.2e} of its scale, gx {ex:.2e}, gy {ey:.2e}")
    assert torch.isfinite(gx).all() and (one or torch.isfinite(gy).all()), c["name"]
    assert le <= 1.0 and ex <= R.GRAD_TOL and ey <= R.GRAD_TOL, (c["name"], le * R.LOSS_TOL, ex, ey)
    return le, ex, ey


@pytest.mark.parametrize("n", K.TILE_N)
def test_tile_edges(n):
    for c in K.tile_cases(n):
        check(c, run(c["x"], c["y"], c["t"], c["w"]), want_of(c))


def test_other_temperatures():
    """at t = 0.5 a counted pad row would add exp(-0.5) to r_i"""
    for c in K.t_cases():
        check(c, run(c["x"], c["y"], c["t"], c["w"]), want_of(c))


@pytest.mark.parametrize("shape", K.CHUNK_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_chunk_layouts(shape):
    c = K.plain_case(*shape)
    check(c, run(c["x"], c["y"], c["t"], c["w"]), want_of(c))


def test_one_chunk_of_many_tiles():
    c = K.plain_case(*K.LARGE_SHAPE)
    assert R.chunk_plan(K.LARGE_SHAPE[0])["chunks"] == 1
    check(c, run(c["x"], c["y"], c["t"], c["w"]), want_of(c, closed=True))


@pytest.mark.parametrize("shape", K.DEGENERATE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_degenerate_rows(shape):
    for f in (K.degenerate_case, K.identical_case, K.antipodal_case):
        c = f(*shape)
        got = run(c["x"], c["y"], c["t"], c["w"])
        check(c, got, want_of(c))
        if f is K.identical_case:
            assert abs(float(got[1][1])) <= R.LOSS_TOL                    # U(x) = 0 in the reference


def test_weights():
    for c in K.weight_cases():
        check(c, run(c["x"], c["y"], c["t"], c["w"]), want_of(c))


@pytest.mark.parametrize("shape", [(65, 64), (129, 128), (257, 50)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_uniformity_alone_leaves_the_other_outputs_untouched(shape):
    n, d = shape
    c = dict(K.plain_case(n, d, t=0.5, w=(7.0, 1.5, 9.0)), y=None)
    kw = ops.kernel_width(d, ops.TABLE_NCE_WIDTHS)
    xs = ops.to_width(c["x"].to(DEV), kw)
    st, out, gx, gy, _ = raw(xs, None, n, kw, c["t"], c["w"])
    assert st == 0
    torch.cuda.synchronize()
    # d_gy, d_parts[0] and d_parts[2] still hold the sentinel bytes
    assert bool((gy.view(torch.uint8) == NAN_BYTE).all())
    assert bool((out[1:].view(torch.uint8).reshape(3, 8)[[0, 2]] == NAN_BYTE).all())
    check(c, (out[0], out[1:], gx[:, :d], None), want_of(c))
    # and ops.au_fwd_bwd(x, None) is the same call
    loss, parts, gx2, gy2 = ops.au_fwd_bwd(c["x"].to(DEV), None, c["t"], *c["w"])
    assert gy2 is None and torch.equal(gx2, gx[:, :d]) and float(loss) == float(out[0])


@pytest.mark.parametrize("shape", K.REPEAT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_two_calls_give_the_same_bits_whatever_the_buffers_held(shape):
    n, d = shape
    c = K.plain_case(n, d)
    x, y = c["x"].to(DEV), c["y"].to(DEV)
    a = raw(x, y, n, d, c["t"], c["w"])
    ws = torch.zeros_like(a[4])                       # another fill of the workspace, other output buffers
    b = raw(x, y, n, d, c["t"], c["w"], ws=ws)
    torch.cuda.synchronize()
    assert a[0] == 0 and b[0] == 0
    for p, q in zip(a[1:4], b[1:4]):
        assert torch.equal(p.view(torch.uint8), q.view(torch.uint8))
    # ops.au_fwd_bwd (torch.empty buffers) is the same call
    loss, parts, gx, gy = ops.au_fwd_bwd(x, y, c["t"], *c["w"])
    assert torch.equal(gx, a[2]) and torch.equal(gy, a[3]) and float(loss) == float(a[1][0]) and torch.equal(parts, a[1][1:])


def test_refusals():
    lib = _lib.load()
    x = torch.randn(65, 96, device=DEV)
    st, out, gx, gy, ws = raw(x, x, 65, 96, 2.0, K.W_MODEL)
    assert st == -3 and b"d=96 unsupported" in lib.srh_last_error_string()
    x = torch.randn(1, 64, device=DEV)
    st1, out1, gx1, _, _ = raw(x, x, 1, 64, 2.0, K.W_MODEL)
    assert st1 == -1 and b"no pair" in lib.srh_last_error_string()
    torch.cuda.synchronize()
    for t in (out, gx, gy, out1, gx1):                # refused before any launch: nothing was written
        assert bool((t.view(torch.uint8) == NAN_BYTE).all())
    with pytest.raises(ops.SelfrecHipError):
        ops.au_fwd_bwd(torch.randn(8, 129, device=DEV), torch.randn(8, 129, device=DEV))
    with pytest.raises(ops.SelfrecHipError):
        ops.au_fwd_bwd(torch.randn(8, 64), torch.randn(8, 64))


@pytest.mark.parametrize("shape,one_sided", [((129, 50), False), ((65, 64), False), ((129, 50), True)])
def test_autograd_op(shape, one_sided):
    """AlignUniformFn under a non-unit upstream gradient, against float64 autograd; d = 50: the padding is cut"""
    n, d = shape
    c = K.plain_case(n, d, w=(1.0, 0.7, 1.3), seed=4000 + n)
    up = 0.37
    x = c["x"].to(DEV).requires_grad_(True)
    y = None if one_sided else c["y"].to(DEV).requires_grad_(True)
    loss = ops.AlignUniformFn.apply(x, y, c["t"], *c["w"])
    assert loss.dtype == torch.float32 and loss.dim() == 0
    (up * loss).backward()
    c = dict(c, y=None if one_sided else c["y"])
    want = want_of(c)
    assert x.grad.shape == (n, d) and (one_sided or y.grad.shape == (n, d))
    got = (loss.double(), ops.au_fwd_bwd(x.detach(), None if one_sided else y.detach(), c["t"], *c["w"])[1], x.grad / up,
           None if one_sided else y.grad / up)
    # (the op's loss is float32: one rounding on top of the kernel's double)
    assert abs(float(loss.detach()) - float(want[0])) <= R.loss_bound(want[1], c["w"], one_sided) + 6e-8 * abs(float(want[0]))
    check(c, (want[0], got[1], got[2], got[3]), want)


def _two_steps(route, data, monkeypatch, tmp_path):
    from selfrec_amd.model.graph.DirectAU import DirectAU
    from selfrec_amd.util import sampler as sampler_mod
    from selfrec_amd.util.conf import ModelConf
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("SRH_DIRECTAU_AU", raising=False)
    real_batches = sampler_mod.next_batch_pairwise

    def batches(d, bs, n_negs=1, **kw):
        for k, b in enumerate(real_batches(d, bs, n_negs, **kw)):
            if k == 2:
                return
            yield b
    monkeypatch.setattr(sampler_mod, "next_batch_pairwise", batches)
    losses = []
    real_backward = torch.Tensor.backward
    monkeypatch.setattr(torch.Tensor, "backward",
                        lambda t, *a, **k: (losses.append(float(t.detach())), real_backward(t, *a, **k))[1])
    conf = ModelConf({"model": {"name": "DirectAU", "type": "graph"}, "item.ranking.topN": [10, 20], "embedding.size": 64,
                      "max.epoch": 1, "batch.size": 512, "learning.rate": 0.001, "reg.lambda": 0.0001,
                      "output": "./results/", "training.set": "x", "test.set": "y",
                      "DirectAU": {"gamma": 2.0, "n_layers": 2}, "engine.au": route})
    torch.manual_seed(3); np.random.seed(4); random.seed(5)
    model = DirectAU(conf, data.training_data, data.test_data)
    assert model.au == route
    model.fast_evaluation = lambda epoch: None
    model.train()
    monkeypatch.undo()
    return losses, {k: v.detach().cpu().numpy() for k, v in model.model.named_parameters()}


def test_model_routes_agree(golden_ops, fresh_tiny_data, monkeypatch, tmp_path):
    """two DirectAU steps on the tiny graph from the same seeds, engine.au: hip against engine.au: torch (each on its own
    fresh copy of the data), to the figures test_gpu_f4.py holds the model to against the reference's own run"""
    from tests.conftest import _tiny_interaction
    data = {"hip": fresh_tiny_data, "torch": _tiny_interaction(golden_ops)}
    runs = {r: _two_steps(r, data[r], monkeypatch, tmp_path) for r in ("hip", "torch")}
    (lh, ph), (lt, pt) = runs["hip"], runs["torch"]
    assert len(lh) == 2 and len(lt) == 2
    np.testing.assert_allclose(lh, lt, rtol=2e-5)
    for k in pt:
        assert np.abs(ph[k] - pt[k]).max() < 1e-5, k
