"""The GRU recurrence kernels on the device against float64: srh_gru_fwd_f32 / srh_gru_bwd_f32 through the C
ABI at one step, at tile edges, at every length pattern, through the H = 32 pad and under weights scaled 3x; exact zeros
over NaN-filled outputs at every dead position, NaN upstream gradients there, equal bits twice and without saved gates;
ops.GruFn's parameter gradients, two layers, and its agreement with torch.nn.GRU on the device.  Cases, restatement and
bounds are tests/gru_ref.py's; tests/test_gru_ref_cpu.py checks their premises without a device."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import gru_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
W = 64                                                          # the kernels' width
GRADS = ("dx", "dw_ih", "dw_hh", "db_ih", "db_hh")
CASE_IDS = [f"{B}x{L}x{H}-{p}-s{int(s)}" for (B, L, H, p, s) in R.cases()]
SHAPE_IDS = ["x".join(map(str, s)) for s in R.SHAPES]


def _ops():
    from selfrec_amd import ops
    torch.cuda.set_device(0)
    return ops


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _device_case(c):
    """the case at the kernels' width on the device: gi from F.linear, padded parameters, int32 lengths, padded go"""
    ops = _ops()
    w_ih, w_hh, b_ih, b_hh = (t.to(DEV) for t in ops.gru_pad_params(c["w_ih"], c["w_hh"], c["b_ih"], c["b_hh"]))
    gi = F.linear(c["x"].to(DEV), w_ih, b_ih).contiguous()
    lens = torch.from_numpy(c["lens"].astype(np.int32)).to(DEV)
    return gi, w_hh.contiguous(), b_hh.contiguous(), lens, ops.to_width(c["go"].to(DEV), W)


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _fwd(gi, w_hh, b_hh, lens, save_gates=True):
    """srh_gru_fwd_f32 into NaN-filled outputs"""
    from selfrec_amd import _lib
    B, L = gi.shape[:2]
    out, gates = _nan(B, L, W), (_nan(B, L, 4 * W) if save_gates else None)
    status = _lib.load().srh_gru_fwd_f32(gi.data_ptr(), w_hh.data_ptr(), b_hh.data_ptr(), lens.data_ptr(), B, L, W,
                                         out.data_ptr(), gates.data_ptr() if save_gates else None,
                                         torch.cuda.current_stream().cuda_stream)
    _lib.check(status, "srh_gru_fwd_f32")
    return out, gates


def _bwd(go, out, gates, w_hh, lens):
    """srh_gru_bwd_f32 into NaN-filled outputs"""
    from selfrec_amd import _lib
    B, L = go.shape[:2]
    dgi, dghn = _nan(B, L, 3 * W), _nan(B, L, W)
    status = _lib.load().srh_gru_bwd_f32(go.data_ptr(), out.data_ptr(), gates.data_ptr(), w_hh.data_ptr(), lens.data_ptr(),
                                         B, L, W, dgi.data_ptr(), dghn.data_ptr(), torch.cuda.current_stream().cuda_stream)
    _lib.check(status, "srh_gru_bwd_f32")
    return dgi, dghn


def _cut(t, H, groups):
    """(B, L, groups * W) at the kernels' width -> (B, L, groups * H), and the largest magnitude in the pad columns: a
    padded unit's h, n, gh_n and gradients are exact zeros (of gates only the n and gh_n groups are looked at: its r and z
    are sigmoid(0) = 0.5 at every live step, which no result reads)"""
    B, L = t.shape[:2]
    v = t.reshape(B, L, groups, W)
    held = v[:, :, 2:] if groups == 4 else v
    pad = float(held[..., H:].abs().max()) if H < W else 0.0
    return v[..., :H].reshape(B, L, groups * H), pad


@pytest.mark.parametrize("case", R.cases(), ids=CASE_IDS)
def test_kernels_against_float64(case):
    B, L, H, pattern, scale = case
    c = R.case(*case)
    ref = c["ref"]
    gi, w_hh, b_hh, lens, go = _device_case(c)
    dead = R.dead_mask(c["lens"], L).to(DEV)
    go[dead] = float("nan")                                    # never read there
    out, gates = _fwd(gi, w_hh, b_hh, lens)
    dgi, dghn = _bwd(go, out, gates, w_hh, lens)
    torch.cuda.synchronize()
    figures = {}
    for name, t, groups, bound in (("out", out, 1, R.OUT_BOUND), ("gates", gates, 4, R.OUT_BOUND),
                                   ("dgi", dgi, 3, R.GRAD_BOUND), ("dghn", dghn, 1, R.GRAD_BOUND)):
        assert not bool(torch.isnan(t).any()), name            # every element was written
        if dead.any():
            assert float(t[dead].abs().max()) == 0.0, name     # exact zeros at every dead position
        got, pad = _cut(t, H, groups)
        assert pad == 0.0, name                                # a padded unit stays an exact zero
        figures[name] = (R.rel_err(got, ref[name]), bound)
    print(f"{CASE_IDS[R.cases().index(case)]}: " + ", ".join(f"{k} {v[0]:.3g}" for k, v in figures.items()))
    for name, (err, bound) in figures.items():
        assert err <= bound, (case, name, err)


@pytest.mark.parametrize("shape", R.SHAPES, ids=SHAPE_IDS)
def test_equal_bits_twice_and_without_saved_gates(shape):
    c = R.case(*shape, "ragged")
    gi, w_hh, b_hh, lens, go = _device_case(c)
    out, gates = _fwd(gi, w_hh, b_hh, lens)
    out2, gates2 = _fwd(gi, w_hh, b_hh, lens)
    out_eval, none = _fwd(gi, w_hh, b_hh, lens, save_gates=False)
    assert none is None and _bits(out, out2) and _bits(gates, gates2) and _bits(out, out_eval)
    dgi, dghn = _bwd(go, out, gates, w_hh, lens)
    dgi2, dghn2 = _bwd(go, out, gates, w_hh, lens)
    assert _bits(dgi, dgi2) and _bits(dghn, dghn2)


def _run_grufn(c, layers=1, params=None):
    """ops.GruFn over the case's x (``layers`` times, each layer with ``params[l]``), backward from go with NaN at the
    dead positions -> (out, dx, [the layer's four parameter gradients in GruFn's order w_ih, w_hh, b_ih, b_hh])"""
    ops = _ops()
    params = params or [(c["w_ih"], c["w_hh"], c["b_ih"], c["b_hh"])]
    x = c["x"].to(DEV).requires_grad_(True)
    leaves = [[p.to(DEV).requires_grad_(True) for p in layer] for layer in params]
    h = x
    for layer in leaves:
        h = ops.GruFn.apply(h, *layer, c["lens"])
    go = c["go"].to(DEV).clone()
    go[R.dead_mask(c["lens"], x.shape[1]).to(DEV)] = float("nan")
    h.backward(go)
    return h.detach(), x.grad, [[p.grad for p in layer] for layer in leaves]


@pytest.mark.parametrize("case", R.cases(), ids=CASE_IDS)
def test_grufn_gradients_against_float64(case):
    c = R.case(*case)
    ref = c["ref"]
    out, dx, [(dw_ih, dw_hh, db_ih, db_hh)] = _run_grufn(c)
    got = dict(dx=dx, dw_ih=dw_ih, dw_hh=dw_hh, db_ih=db_ih, db_hh=db_hh)
    figures = {name: R.rel_err(got[name], ref[name]) for name in GRADS}
    print(f"{CASE_IDS[R.cases().index(case)]}: " + ", ".join(f"{k} {v:.3g}" for k, v in figures.items()))
    assert R.rel_err(out, ref["out"]) <= R.OUT_BOUND
    for name in GRADS:
        assert got[name].shape == ref[name].shape and figures[name] <= R.GRAD_BOUND, (case, name, figures[name])


def test_two_layers_through_grufn():
    c = R.case(17, 33, 64, "ragged")
    second = R.case(17, 33, 64, "short")                                          # (its parameters: another draw)
    params = [tuple(c[k] for k in ("w_ih", "w_hh", "b_ih", "b_hh")), tuple(second[k] for k in ("w_ih", "w_hh", "b_ih", "b_hh"))]
    # the restatement, chained: layer 1's out is layer 2's x, layer 2's dx is layer 1's go
    zeros = torch.zeros_like(c["go"])
    mid = R.gru_layer(c["x"], *params[0], c["lens"], zeros)["out"]
    top = R.gru_layer(mid, *params[1], c["lens"], c["go"])
    bottom = R.gru_layer(c["x"], *params[0], c["lens"], top["dx"])
    out, dx, grads = _run_grufn(c, 2, params)
    assert R.rel_err(out, top["out"]) <= R.OUT_BOUND and R.rel_err(dx, bottom["dx"]) <= R.GRAD_BOUND
    for ref, got in ((bottom, grads[0]), (top, grads[1])):
        for name, g in zip(("dw_ih", "dw_hh", "db_ih", "db_hh"), got):
            assert R.rel_err(g, ref[name]) <= R.GRAD_BOUND, name


@pytest.mark.parametrize("shape", [(3, 7, 64), (17, 33, 64), (4, 12, 32)], ids=lambda s: "x".join(map(str, s)))
def test_grufn_agrees_with_the_torch_route_on_the_device(shape):
    """both routes of the model's layer on the device, within twice the bounds (each is inside one of float64)"""
    B, L, H = shape
    c = R.case(B, L, H, "ragged")
    out, dx, [grads] = _run_grufn(c)
    gru = torch.nn.GRU(H, H, num_layers=1, batch_first=True).to(DEV)
    with torch.no_grad():
        for p, k in zip((gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0), ("w_ih", "w_hh", "b_ih", "b_hh")):
            p.copy_(c[k])
    x = c["x"].to(DEV).requires_grad_(True)
    live = (~R.dead_mask(c["lens"], L)).to(DEV).unsqueeze(-1)
    partner = gru(x)[0] * live
    partner.backward(torch.where(live, c["go"].to(DEV), torch.zeros((), device=DEV)))
    assert R.rel_err(out, partner.detach()) <= 2 * R.OUT_BOUND
    assert R.rel_err(dx, x.grad) <= 2 * R.GRAD_BOUND
    for g, p in zip(grads, (gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0)):
        assert R.rel_err(g, p.grad) <= 2 * R.GRAD_BOUND


def test_gather_live_rows_leaves_the_padding_row_an_exact_zero():
    ops = _ops()
    rs = np.random.RandomState(5)
    ids = rs.randint(1, 40, size=(9, 13))
    ids[:, 7:] = 0
    ids[3, 2:] = 0
    table = torch.randn(40, 64, device=DEV, requires_grad=True)
    idx = torch.from_numpy(ids.reshape(-1).astype(np.int32)).to(DEV)
    rows = ops.GatherLiveRowsFn.apply(table, idx, ops.live_plan(ids.reshape(-1), DEV))
    assert torch.equal(rows, table.detach()[idx.long()])
    g = torch.randn(9 * 13, 64, device=DEV)
    rows.backward(g)
    want = torch.zeros(40, 64, dtype=torch.float64).index_add_(0, torch.from_numpy(ids.reshape(-1)), g.double().cpu())
    want[0] = 0.0
    assert float(table.grad[0].abs().max()) == 0.0
    assert R.rel_err(table.grad, want) <= 1e-6
