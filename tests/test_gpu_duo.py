"""DuoRec's fused contrastive section on the device against float64: ops.duo_nce_fwd_bwd / ops.DuoNceFn at
the tile and block edges of both input families, through the pad, through shuffled index vectors, under scales, on a dirty
workspace, twice, at its refusals, and against the ``pair`` route.  Cases, restatement and measures are tests/duo_ref.py's;
tests/test_duo_ref_cpu.py checks their premises without a device."""
import numpy as np
import pytest
import torch

from tests import duo_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _ops():
    from selfrec_amd import ops
    torch.cuda.set_device(0)
    return ops


def _bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _stack(blocks):
    return torch.cat(blocks).to(DEV)


def _contested_figures(losses, g, ref):
    return max(R.rel_loss_figures(losses, ref)), R.grad_figure(g, ref)


@pytest.mark.parametrize("d", R.WIDTHS)
@pytest.mark.parametrize("B", (1,) + R.CONTESTED_B)
def test_contested_against_float64(B, d):
    ops = _ops()
    blocks = R.contested(B, d)
    x = _stack(blocks)
    for temp in R.CONTESTED_TEMPS:
        losses, g = ops.duo_nce_fwd_bwd(x, None, B, 1.0 / temp)
        if B == 1:
            assert float(losses.abs().max()) == 0.0 and float(g.abs().max()) == 0.0 and g.shape == (3, d)
            continue
        ref = R.reference("contested", B, d, temp)
        lf, gf = _contested_figures(losses, g, ref)
        print(f"B={B} d={d} temp={temp}: loss {lf:.3g}, gradient rows {gf:.3g}")
        assert lf <= R.LOSS_TOL and gf <= R.GRAD_TOL, (B, d, temp, lf, gf)


@pytest.mark.parametrize("B", R.PEAKED_B)
def test_peaked_against_float64_with_row_terms(B):
    ops = _ops()
    d = 64
    blocks = R.peaked(B, d)
    x = _stack(blocks)
    carve = R.ws_carve(B)
    assert int(ops._lib.load().srh_duo_nce_ws_bytes(B, d)) == carve["total"]
    ws = torch.empty(carve["total"], dtype=torch.uint8, device=DEV)
    losses, g = ops.duo_nce_fwd_bwd(x, None, B, 1.0, ws=ws)
    ref = R.reference("peaked", B, d, 1.0)
    n = 3 * B
    lse = torch.stack([ws[o:o + 4 * n].view(torch.float32) for o in carve["lse"]])
    terms = torch.stack([ws[o:o + 8 * n].view(torch.float64) for o in carve["term"]])
    has = torch.isfinite(ref["lse"])
    assert torch.equal(torch.isfinite(lse).cpu(), has) and bool((terms.cpu()[~has] == 0).all())
    lse_f, term_f = R.term_figures(torch.where(has, lse.cpu().double(), ref["lse"]), terms, ref)
    loss_f = max(R.peaked_loss_figures(losses, ref, (1.0, 1.0), B))
    grad_f = R.cancel_figure(g, ref, torch.cat(blocks), 1.0, (1.0, 1.0), B)
    print(f"peaked B={B}: lse {lse_f:.3g}, row terms {term_f:.3g}, loss {loss_f:.3g}, gradient {grad_f:.3g}")
    assert lse_f <= R.LOSS_TOL and term_f <= R.LOSS_TOL and loss_f <= R.LOSS_TOL and grad_f <= R.GRAD_TOL


@pytest.mark.parametrize("d", (50, 100))
def test_narrow_rows_through_the_pad(d):
    ops = _ops()
    B, temp = 17, 0.5
    blocks = R.contested(B, d)
    losses, g = ops.duo_nce_fwd_bwd(_stack(blocks), None, B, 1.0 / temp)
    ref = R.duo(*blocks, 1.0 / temp)
    assert float(ref["losses"].min()) > 0.01
    lf, gf = _contested_figures(losses, g, ref)
    assert g.shape == (3 * B, d) and lf <= R.LOSS_TOL and gf <= R.GRAD_TOL, (lf, gf)


@pytest.mark.parametrize("B", (17, 65))
def test_index_vectors_give_the_bits_of_pregathered_blocks(B):
    ops = _ops()
    d, L = 64, 7
    rows = 3 * B * L + 5
    gen = torch.Generator().manual_seed(77 + B)
    x = torch.randn(rows, d, generator=gen) * d ** -0.25
    idx = torch.randperm(rows, generator=gen)[:3 * B].reshape(3, B)
    xd = x.to(DEV).requires_grad_(True)
    idx_d = idx.to(torch.int32).to(DEV)
    want_l, want_g = ops.duo_nce_fwd_bwd(x[idx.reshape(-1)].to(DEV), None, B, 2.0, 0.1, 0.1)
    got_l, got_g = ops.duo_nce_fwd_bwd(xd.detach(), idx_d, B, 2.0, 0.1, 0.1, idx_host=idx.numpy())
    assert _bits(got_l, want_l) and _bits(got_g, want_g)
    out = ops.DuoNceFn.apply(2.0, 0.1, 0.1, idx_d, idx.numpy(), xd)
    assert _bits(out, want_l.to(torch.float32))
    out.sum().backward()
    touched = torch.zeros(rows, dtype=torch.bool)
    touched[idx.reshape(-1)] = True
    assert _bits(xd.grad[idx_d.reshape(-1).long()], want_g)
    assert float(xd.grad[touched.logical_not().to(DEV)].abs().max()) == 0.0
    # the three-input form of the Function: the same losses, each block's rows in its own gradient
    leaves = [x[idx[k]].to(DEV).requires_grad_(True) for k in range(3)]
    out3 = ops.DuoNceFn.apply(2.0, 0.1, 0.1, None, None, *leaves)
    out3.sum().backward()
    assert _bits(out3, out.detach()) and _bits(torch.cat([t.grad for t in leaves]), want_g)


@pytest.mark.parametrize("scales", ((0.1, 0.1), (0.0, 0.3), (-2.5, 1.0)))
def test_scales(scales):
    ops = _ops()
    B, d, temp = 43, 64, 1.0
    blocks = R.contested(B, d)
    losses, g = ops.duo_nce_fwd_bwd(_stack(blocks), None, B, 1.0 / temp, *scales)
    ref = R.duo(*blocks, 1.0 / temp, *scales)
    for t in range(2):
        want = float(ref["losses"][t])
        if scales[t] == 0.0:
            assert float(losses[t]) == 0.0 and want == 0.0
        else:
            assert abs(float(losses[t]) - want) <= R.LOSS_TOL * abs(want)
    assert R.grad_figure(g, ref) <= R.GRAD_TOL
    if scales[0] == 0.0:
        assert float(g[B:2 * B].abs().max()) == 0.0          # P rows belong to the u term alone


def test_dirty_workspace_and_two_calls_give_the_same_bits():
    ops = _ops()
    B, d = 65, 128
    x = _stack(R.contested(B, d))
    first = ops.duo_nce_fwd_bwd(x, None, B, 2.0)
    need = int(ops._lib.load().srh_duo_nce_ws_bytes(B, d))
    ws = torch.full((need // 4,), float("nan"), dtype=torch.float32, device=DEV).view(torch.uint8)
    dirty = ops.duo_nce_fwd_bwd(x, None, B, 2.0, ws=ws)
    again = ops.duo_nce_fwd_bwd(x, None, B, 2.0, ws=ws)
    for a, b in ((first, dirty), (first, again)):
        assert _bits(a[0], b[0]) and _bits(a[1], b[1])
    assert bool(torch.isfinite(first[1]).all())


def test_refusals():
    ops = _ops()
    B = 5
    x = torch.randn(3 * B, 64, device=DEV)
    with pytest.raises(ops.SelfrecHipError):
        ops.duo_nce_fwd_bwd(torch.randn(3 * B, 256, device=DEV), None, B)
    lib = ops._lib.load()
    assert int(lib.srh_duo_nce_ws_bytes(B, 256)) == 0
    losses, g = torch.empty(2, dtype=torch.float64, device=DEV), torch.empty(3 * B, 256, device=DEV)
    ws = torch.empty(4096, dtype=torch.uint8, device=DEV)
    wide = torch.randn(3 * B, 256, device=DEV)
    status = lib.srh_duo_nce_fwd_bwd(wide.data_ptr(), 3 * B, None, None, None, B, 256, 1.0, 1.0, 1.0, losses.data_ptr(),
                                     g.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert status == -3 and "d=256" in lib.srh_last_error_string().decode()     # SRH_ERR_UNSUPPORTED
    for bad in (0.0, -1.0, float("inf")):
        with pytest.raises(ops.SelfrecHipError):
            ops.duo_nce_fwd_bwd(x, None, B, bad)
    status = lib.srh_duo_nce_fwd_bwd(x.data_ptr(), 3 * B, None, None, None, B, 64, 0.0, 1.0, 1.0, losses.data_ptr(),
                                     g.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert status == -1                                                           # SRH_ERR_INVALID_ARG
    idx = np.arange(3 * B).reshape(3, B)
    idx[2, 1] = idx[0, 3]
    with pytest.raises(ops.SelfrecHipError, match="distinct"):
        ops.duo_nce_fwd_bwd(x, torch.from_numpy(idx).to(torch.int32).to(DEV), B)
    idx = np.arange(3 * B).reshape(3, B)
    idx[1, 0] = 3 * B
    with pytest.raises(ops.SelfrecHipError, match="outside"):
        ops.duo_nce_fwd_bwd(x, torch.from_numpy(idx).to(torch.int32).to(DEV), B)
    ops.duo_nce_fwd_bwd(x, None, B)                                                   # (and the next call is served)


@pytest.mark.parametrize("family,B,d", (("contested", 65, 64), ("contested", 129, 128), ("peaked", 64, 64)))
def test_agrees_with_the_pair_route(family, B, d):
    from selfrec_amd.util import loss_torch as L
    ops = _ops()
    blocks = (R.contested if family == "contested" else R.peaked)(B, d)
    losses, g = ops.duo_nce_fwd_bwd(_stack(blocks), None, B, 1.0, 0.1, 0.1)
    leaves = [t.to(DEV).requires_grad_(True) for t in blocks]
    pair = torch.stack((L.info_nce(leaves[0], leaves[1], 1.0, B), L.info_nce(leaves[0], leaves[2], 1.0, B))) * 0.1
    pair.sum().backward()
    pair_g = torch.cat([t.grad for t in leaves])
    ref = R.reference(family, B, d, 1.0, 0.1, 0.1)
    other = dict(ref, losses=pair.detach().double().cpu(), g=pair_g.double().cpu())
    if family == "contested":
        lf, gf = max(R.rel_loss_figures(losses, other)), R.grad_figure(g, other)
    else:
        lf = max(R.peaked_loss_figures(losses, other, (0.1, 0.1), B))
        gf = R.cancel_figure(g, other, torch.cat(blocks), 1.0, (0.1, 0.1), B)
    assert lf <= 2 * R.LOSS_TOL and gf <= 2 * R.GRAD_TOL, (lf, gf)
