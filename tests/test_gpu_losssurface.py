"""The rest of util/loss_torch.py on the device against float64: the pair cross-entropy through
ops.pair_ce_fwd_bwd at its tile, chunk and exclusion edges, info_nce, InfoNCE(b_cos=False) and InfoNCE below temperature
0.03 through the wrappers, and triplet_loss / kl_divergence row by row and element by element.  Cases, restatements and
bounds are tests/losssurface_ref.py's; tests/test_losssurface_ref_cpu.py checks their premises without a device."""
import warnings

import numpy as np
import pytest
import torch

from tests import losssurface_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _mods():
    from selfrec_amd import ops
    from selfrec_amd.util import loss_torch as L
    torch.cuda.set_device(0)
    return ops, L


def _leaf(a, device=DEV):
    a = a.clone() if isinstance(a, torch.Tensor) else torch.tensor(np.array(a))
    return a.to(torch.float32).to(device).requires_grad_(True)


def _gout(value, like):
    return torch.tensor(float(value), dtype=torch.float32, device=like.device)


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.detach().reshape(-1).contiguous().view(torch.uint8), b.detach().reshape(-1).contiguous().view(torch.uint8))


# ---- a. the pair cross-entropy, direct ----------------------------------------------------------------------------------------
def _pair_call(ops, index, scale, ws=None):
    M, N, d, inv_temp, exclude, family = R.PAIR_CASES[index]
    h, t, labels = R.pair_case(index)
    hd = h.to(DEV)
    td = hd if family == "alias" else t.to(DEV)
    return ops.pair_ce_fwd_bwd(hd, td, labels.to(torch.int32).to(DEV), inv_temp, scale, exclude_diagonal=exclude,
                               add_gh_into_gt=family == "alias", ws=ws)


def _pair_figures(index, out, scale):
    c = R.PAIR_CASES[index]
    ref = R.pair_reference(index)
    floor_h, floor_t = R.pair_floors(c)
    loss, gh, gt = out
    want_gt = ref["gh"] + ref["gt"] if c[5] == "alias" else ref["gt"]          # alias: the fused gh + gt
    return {"loss": R.loss_figure(loss.item(), ref, 1.0, scale),
            "gh": R.grad_figure(gh, scale * ref["gh"], floor_h), "gt": R.grad_figure(gt, scale * want_gt, floor_t)}


@pytest.mark.parametrize("index", range(len(R.PAIR_CASES)), ids=lambda i: R.pair_id(R.PAIR_CASES[i]))
def test_pair_ce_row_by_row(index):
    ops, _ = _mods()
    c = R.PAIR_CASES[index]
    M, N, d, inv_temp, exclude, family = c
    w = ops.padded_width(d, ops.TABLE_NCE_WIDTHS)
    carve = R.ws_carve(M, N, w)
    lib = ops._lib.load()
    assert int(lib.srh_pair_ce_ws_bytes(M, N, w)) == carve["total"] == int(lib.srh_table_ce_ws_bytes(M, N, w))
    ref = R.pair_reference(index)
    for scale in R.PAIR_SCALES:
        ws = torch.full((carve["total"],), 0xFF, dtype=torch.uint8, device=DEV)          # NaN wherever it is read unwritten
        out = _pair_call(ops, index, scale, ws)
        assert out[0].dtype == torch.float64 and tuple(out[1].shape) == (M, d) and tuple(out[2].shape) == (N, d)
        figs = _pair_figures(index, out, scale)
        # lse and the row terms, where the finish leaves them
        lse = ws[carve["lse"]:carve["lse"] + 4 * M].view(torch.float32).double().cpu()
        rows = ws[carve["row_loss"]:carve["row_loss"] + 8 * M].view(torch.float64).cpu()
        den = ref["lse"].abs().clamp_min(1.0)
        figs["lse"] = float(((lse - ref["lse"]).abs() / den).max())
        figs["row"] = float(((rows - ref["row_loss"]).abs() / torch.maximum(den, ref["pos"].abs())).max())
        print(f"pair {R.pair_id(c)} scale {scale}: " + ", ".join(f"{k} {v:.2e}" for k, v in figs.items()))
        assert figs["loss"] <= R.LOSS_TOL and figs["lse"] <= R.LSE_TOL and figs["row"] <= R.LSE_TOL, figs
        assert figs["gh"] <= R.GRAD_TOL and figs["gt"] <= R.GRAD_TOL, figs
    again = _pair_call(ops, index, R.PAIR_SCALES[-1])
    assert all(_bits(a, b) for a, b in zip(out, again))                               # the same bits on every call


def test_pair_ce_zero_scale_gives_exact_zeros_and_a_dirty_workspace_changes_nothing():
    ops, _ = _mods()
    i, _, j = R.PAIR_DIRTY
    loss, gh, gt = _pair_call(ops, i, 0.0)
    assert loss.item() == 0.0 and not gh.any().item() and not gt.any().item()
    shapes = [R.PAIR_CASES[k] for k in (i, j)]
    need = max(R.ws_carve(c[0], c[1], ops.padded_width(c[2], ops.TABLE_NCE_WIDTHS))["total"] for c in shapes)
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device=DEV)
    clean = _pair_call(ops, i, 1.0)
    first = _pair_call(ops, i, 1.0, ws)
    _pair_call(ops, j, 1.0, ws)
    second = _pair_call(ops, i, 1.0, ws)
    for a, b, c in zip(clean, first, second):
        assert _bits(a, b) and _bits(a, c)


def test_pair_ce_fused_sum_is_the_sum_of_the_unfused_call():
    """H = T aliased: add_gh_into_gt hands back gh + gt, each as the call without the flag computes it (one float32 add)"""
    ops, _ = _mods()
    for index, c in enumerate(R.PAIR_CASES):
        if c[5] != "alias":
            continue
        h, _, labels = R.pair_case(index)
        hd, lab = h.to(DEV), labels.to(torch.int32).to(DEV)
        loss_f, gh_f, gz = ops.pair_ce_fwd_bwd(hd, hd, lab, c[3], 1.0, exclude_diagonal=True, add_gh_into_gt=True)
        loss_u, gh_u, gt_u = ops.pair_ce_fwd_bwd(hd, hd.clone(), lab, c[3], 1.0, exclude_diagonal=True)
        assert _bits(loss_f, loss_u) and _bits(gh_f, gh_u)
        # gz = gt + gh in one float32 step (the scaling of gt may be contracted into it): within one rounding of each term
        slack = 2.0 ** -23 * (gt_u.abs() + gh_u.abs())
        assert ((gz - (gt_u + gh_u)).abs() <= slack).all().item()


def test_pair_ce_own_key_as_label_under_exclusion_is_nan_and_touches_no_other_row():
    ops, _ = _mods()
    index = next(i for i, c in enumerate(R.PAIR_CASES) if c[:2] == (65, 65) and c[4] and c[5] == "ordinary" and c[3] == 1.0)
    h, t, labels = R.pair_case(index)
    bad = labels.clone()
    bad[64] = 64
    hd, td = h.to(DEV), t.to(DEV)
    loss, gh, gt = ops.pair_ce_fwd_bwd(hd, td, bad.to(torch.int32).to(DEV), 1.0, 1.0, exclude_diagonal=True)
    good = ops.pair_ce_fwd_bwd(hd, td, labels.to(torch.int32).to(DEV), 1.0, 1.0, exclude_diagonal=True)
    assert torch.isnan(loss).item() and torch.isfinite(gh).all().item() and torch.isfinite(gt).all().item()
    assert _bits(gh[:64], good[1][:64])
    # row 64 has no one-hot in either gradient: both against the restatement with the same labels
    M, N, d, inv_temp, exclude, family = R.PAIR_CASES[index]
    ref = R.pair_ce(h, t, bad, inv_temp, 1.0, True)
    assert ref["loss"] != ref["loss"]
    floor = R.FLOOR_OF[R.pair_group(R.PAIR_CASES[index])]
    figs = {"gh": R.grad_figure(gh, ref["gh"], floor), "gt": R.grad_figure(gt, ref["gt"], floor)}
    print(f"own key as label: gh {figs['gh']:.2e}, gt {figs['gt']:.2e}")
    assert figs["gh"] <= R.GRAD_TOL and figs["gt"] <= R.GRAD_TOL, figs
    # (and that is another gt than with the one-hot taken off key 64: the rows differ by h_64)
    with_onehot = ref["gt"].clone()
    with_onehot[64] -= inv_temp * h[64].double()
    assert R.grad_figure(gt, with_onehot, floor) > 100 * R.GRAD_TOL


def test_pair_ce_refuses_what_it_cannot_serve():
    ops, _ = _mods()
    x, y = torch.randn(1, 64, device=DEV), torch.randn(3, 64, device=DEV)
    lab1, lab3 = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(3, dtype=torch.int32, device=DEV)
    with pytest.raises(ops.SelfrecHipError, match="N = 1 leaves no key"):
        ops.pair_ce_fwd_bwd(x, x, lab1, 1.0, 1.0, exclude_diagonal=True)
    with pytest.raises(ops.SelfrecHipError, match="exclude_diagonal needs M == N"):
        ops.pair_ce_fwd_bwd(x, y, lab1, 1.0, 1.0, exclude_diagonal=True)
    with pytest.raises(ops.SelfrecHipError, match="add_gh_into_gt needs M == N"):
        ops.pair_ce_fwd_bwd(y, x, lab3, 1.0, 1.0, add_gh_into_gt=True)
    with pytest.raises(ops.SelfrecHipError, match="inv_temp must be positive"):
        ops.pair_ce_fwd_bwd(y, y, lab3, 0.0, 1.0)
    with pytest.raises(ops.SelfrecHipError, match="up to 128"):
        ops.pair_ce_fwd_bwd(torch.randn(3, 129, device=DEV), torch.randn(3, 129, device=DEV), lab3)
    loss, gh, gt = ops.pair_ce_fwd_bwd(y, y, lab3, 1.0, 1.0)                          # (and the next call is served)
    assert torch.isfinite(loss).item()


# ---- b. info_nce ----------------------------------------------------------------------------------------------------------
def _wrapper_figures(loss, grads, ref, names, loss_scale, floor, gout=1.0):
    figs = {"loss": R.loss_figure(loss.item(), ref["ce"], loss_scale)}
    for g, k in zip(grads, names):
        figs[k] = R.grad_figure(g, gout * ref[k], floor)
    return figs


@pytest.mark.parametrize("index", range(len(R.INFO_NCE_CASES)), ids=lambda i: "B%d_d%d_t%g_%s" % R.INFO_NCE_CASES[i])
def test_info_nce_against_float64(index):
    _, L = _mods()
    c = R.INFO_NCE_CASES[index]
    B, d, temp, sim = c
    z_i, z_j = (_leaf(a) for a in R.info_nce_case(index))
    loss = L.info_nce(z_i, z_j, temp, B, sim)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.is_cuda
    ref = R.info_nce_reference(index)
    floor = R.FLOOR_OF[R.info_nce_group(c)]
    for gout in R.GOUTS:
        gi, gj = torch.autograd.grad(loss, (z_i, z_j), grad_outputs=_gout(gout, loss), retain_graph=True)
        assert tuple(gi.shape) == (B, d) and tuple(gj.shape) == (B, d)
        if B == 1:
            # both rows have one key, their positive: loss 0 (its denominator: max(1, |lse|, |s_pos|) >= 1 per row) and
            # zero gradients, against the size of the two terms that cancel in them: (|gout| / 2B) (1 / temp) max|y|,
            # y the rows as the products see them (unit rows under 'cos')
            y = torch.cat(R.info_nce_case(index)).double()
            top = 1.0 if sim == "cos" else float(y.abs().max())
            scale = abs(gout) / (2 * B) / temp * top / (float(y.norm(dim=1).min()) if sim == "cos" else 1.0)
            worst = max(float(gi.abs().max()), float(gj.abs().max()))
            print(f"info_nce B=1 d={d} {sim} gout {gout}: loss {loss.item():.2e}, largest gradient entry {worst:.2e}")
            assert R.loss_figure(loss.item(), ref["ce"], 1.0 / (2 * B)) <= R.LOSS_TOL and worst <= R.GRAD_TOL * scale
            continue
        figs = _wrapper_figures(loss, (gi, gj), ref, ("gi", "gj"), 1.0 / (2 * B), floor, gout)
        print(f"info_nce {c} gout {gout}: " + ", ".join(f"{k} {v:.2e}" for k, v in figs.items()))
        assert figs["loss"] <= R.LOSS_TOL and figs["gi"] <= R.GRAD_TOL and figs["gj"] <= R.GRAD_TOL, figs
        if gout == 0.0:
            assert not gi.any().item() and not gj.any().item()


def test_info_nce_cos_with_a_zero_row_has_the_reference_forward_value():
    _, L = _mods()
    B, d, temp, sim = R.ZERO_ROW_CASE
    z_i, z_j = R.info_nce_case(0, zero_row=True)
    loss = L.info_nce(z_i.to(DEV), z_j.to(DEV), temp, B, sim)
    ref = R.info_nce(z_i, z_j, temp, sim)
    assert R.loss_figure(loss.item(), ref["ce"], 1.0 / (2 * B)) <= R.LOSS_TOL


def test_info_nce_routes():
    ops, L = _mods()
    z = torch.randn(4, 64, device=DEV)
    with pytest.raises(ValueError, match="sim must be"):
        L.info_nce(z, z, 1.0, 4, sim="l2")
    with pytest.raises((RuntimeError, IndexError)):         # batch_size != rows: the reference's expression, its error
        L.info_nce(z, z, 1.0, 3)
    wide = torch.randn(4, 200, device=DEV, requires_grad=True)
    L._warned_wide[:] = [w for w in L._warned_wide if w != "info_nce"]
    with pytest.warns(RuntimeWarning, match="info_nce on rows of 200 columns"):
        got = L.info_nce(wide, wide.detach(), 0.5, 4)
    want = R.info_nce(wide.detach().cpu(), wide.detach().cpu(), 0.5, "dot")
    assert abs(got.item() - want["loss"]) < 1e-4 * max(1.0, abs(want["loss"]))


# ---- c. InfoNCE(b_cos=False) and InfoNCE(b_cos=True) below 0.03 -------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(R.RAW_CASES)), ids=lambda i: "n%d_d%d_t%g_%s" % R.RAW_CASES[i])
def test_infonce_without_normalisation_against_float64(index):
    _, L = _mods()
    c = R.RAW_CASES[index]
    n, d, tau, family = c
    v1, v2 = (_leaf(a) for a in R.raw_case(index))
    loss = L.InfoNCE(v1, v2, tau, b_cos=False)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    ref = R.raw_reference(index)
    floor = R.FLOOR_OF[R.raw_group(c)]
    for gout in R.GOUTS:
        g1, g2 = torch.autograd.grad(loss, (v1, v2), grad_outputs=_gout(gout, loss), retain_graph=True)
        assert tuple(g1.shape) == (n, d) and tuple(g2.shape) == (n, d)
        if n == 1:
            assert not g1.any().item() and not g2.any().item()                          # P_00 = exp(0) = 1 exactly
        figs = _wrapper_figures(loss, (g1, g2), ref, ("g1", "g2"), 1.0 / n, floor, gout)
        print(f"InfoNCE raw {c} gout {gout}: " + ", ".join(f"{k} {v:.2e}" for k, v in figs.items()))
        assert figs["loss"] <= R.LOSS_TOL and figs["g1"] <= R.GRAD_TOL and figs["g2"] <= R.GRAD_TOL, figs


@pytest.mark.parametrize("index", range(len(R.UNIT_CASES)), ids=lambda i: "n%d_d%d_t%g" % R.UNIT_CASES[i])
def test_infonce_cosine_at_low_temperature_against_float64(index):
    _, L = _mods()
    n, d, tau = R.UNIT_CASES[index]
    v1, v2 = (_leaf(a) for a in R.unit_case(index))
    loss = L.InfoNCE(v1, v2, tau)
    ref = R.unit_reference(index)
    assert np.isfinite(loss.item())
    cold = float(ref["ce"]["row_loss"][R.COLD_ROW])
    for gout in R.GOUTS:
        g1, g2 = torch.autograd.grad(loss, (v1, v2), grad_outputs=_gout(gout, loss), retain_graph=True)
        figs = _wrapper_figures(loss, (g1, g2), ref, ("g1", "g2"), 1.0 / n, R.FLOOR_OF["hot"], gout)
        print(f"InfoNCE cos n={n} tau={tau} gout {gout} (cold row's term {cold:.3f}): "
              + ", ".join(f"{k} {v:.2e}" for k, v in figs.items()))
        assert figs["loss"] <= R.LOSS_TOL and figs["g1"] <= R.GRAD_TOL and figs["g2"] <= R.GRAD_TOL, figs
    # the cold row, whose every term the unit-row kernels' exp((s - 1) / tau) loses: finite, and within the bound above
    g1 = torch.autograd.grad(loss, v1)[0]
    assert np.isfinite(cold) and torch.isfinite(g1[R.COLD_ROW]).all().item() and g1[R.COLD_ROW].any().item()


def test_infonce_at_an_ordinary_temperature_keeps_the_old_path_bit_for_bit():
    ops, L = _mods()
    n, d, tau = R.BITS_CASE
    a1, a2 = R.unit_case(-1)
    v1, v2 = _leaf(a1), _leaf(a2)
    w1, w2 = _leaf(a1), _leaf(a2)
    loss = L.InfoNCE(v1, v2, tau)
    old = ops.InfoNceFn.apply(w1, w2, tau)
    assert _bits(loss, old)
    g = torch.autograd.grad(loss, (v1, v2), grad_outputs=_gout(3.7, loss))
    h = torch.autograd.grad(old, (w1, w2), grad_outputs=_gout(3.7, old))
    assert _bits(g[0], h[0]) and _bits(g[1], h[1])


# ---- d. triplet_loss ---------------------------------------------------------------------------------------------------------
def _triplet_figures(grads, ref):
    return {k: R.row_error(_np(g), ref[k], ref["s"]) for g, k in zip(grads, ("gu", "gp", "gn"))}


@pytest.mark.parametrize("family", R.TRIPLET_FAMILIES)
@pytest.mark.parametrize("shape", R.bpr_shapes(), ids=lambda s: "B%d_d%d" % s)
def test_triplet_loss_row_by_row(shape, family):
    _, L = _mods()
    B, d = shape
    u, p, n = (_leaf(a) for a in R.triplet_case(B, d, family))
    loss = L.triplet_loss(u, p, n)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.is_cuda
    el = R.loss_error(loss.item(), R.triplet_reference(B, d, family, 1.0)["loss"])
    print(f"triplet B={B} d={d} {family}: loss {el:.2e} (bound {R.TRIPLET_LOSS_BOUND:.1e})")
    assert el < R.TRIPLET_LOSS_BOUND
    if family == "inactive":
        assert loss.item() == 0.0
    for gout in R.GOUTS:
        ref = R.triplet_reference(B, d, family, gout)
        grads = torch.autograd.grad(loss, (u, p, n), grad_outputs=_gout(gout, loss), retain_graph=True)
        assert all(tuple(g.shape) == (B, d) for g in grads)
        figs = _triplet_figures(grads, ref)
        print(f"    gout {gout}: " + ", ".join(f"{k} {v:.2e}" for k, v in figs.items()))
        assert max(figs.values()) < R.TRIPLET_ROW_BOUND, (gout, figs)
        inactive = torch.tensor(ref["x"] <= 0.0)
        for g in grads:                                             # exact zeros where the margin is not positive
            assert not g[inactive.to(DEV)].any().item()
        if gout == 0.0:
            assert not any(g.any().item() for g in grads)


@pytest.mark.parametrize("shapes", [((7, 64), (1, 64), (7, 64)), ((7, 50), (7, 50), (1, 50)), ((7, 32), (7, 1), (7, 32)),
                                    ((1, 64), (7, 64), (7, 64))])
def test_triplet_loss_broadcasts_its_operands(shapes):
    _, L = _mods()
    g = torch.Generator().manual_seed(11)
    host = [0.3 * torch.randn(*s, generator=g) for s in shapes]
    leaves = [_leaf(t) for t in host]
    loss = L.triplet_loss(*leaves)
    grads = torch.autograd.grad(loss, leaves, grad_outputs=_gout(3.7, loss))
    full = [t.expand(7, max(s[1] for s in shapes)).numpy() for t in host]
    ref = R.triplet(*full, 3.7)
    assert np.abs(ref["x"]).min() >= R.MIN_ABS_X
    assert R.loss_error(loss.item(), ref["loss"]) < R.TRIPLET_LOSS_BOUND
    for t, got, k in zip(host, grads, ("gu", "gp", "gn")):
        assert got.shape == t.shape
        axes = tuple(a for a in range(2) if t.shape[a] == 1 and ref[k].shape[a] != 1)
        want = ref[k].sum(axis=axes, keepdims=True) if axes else ref[k]
        scale = np.broadcast_to(ref["s"][:, None], ref[k].shape)
        scale = scale.sum(axis=axes, keepdims=True) if axes else scale          # the sum of its terms' scales
        err = float((np.abs(_np(got).astype(np.float64) - want) / scale).max())
        assert err < R.TRIPLET_ROW_BOUND, (k, err)


def test_triplet_loss_wide_rows_take_the_announced_route_and_no_rows_give_nan():
    _, L = _mods()
    u, p, n = (torch.randn(5, 300, device=DEV) for _ in range(3))
    L._warned_wide[:] = [w for w in L._warned_wide if w != "triplet_loss"]
    with pytest.warns(RuntimeWarning, match="triplet_loss on rows of 300 columns"):
        got = L.triplet_loss(u, p, n)
    assert torch.allclose(got, L._triplet_expression(u, p, n))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        L.triplet_loss(u, p, n)                                      # announced once
    e = torch.empty(0, 64, device=DEV)
    assert torch.isnan(L.triplet_loss(e, e, e)).item()


# ---- e. kl_divergence ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", R.KL_FAMILIES)
@pytest.mark.parametrize("shape", R.KL_SHAPES, ids=lambda s: "R%d_C%d" % s)
def test_kl_divergence_element_by_element(shape, family):
    _, L = _mods()
    Rr, C = shape
    a, b = (_leaf(x) for x in R.kl_case(Rr, C, family))
    loss = L.kl_divergence(a, b)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.is_cuda
    el = R.loss_error(loss.item(), R.kl_reference(Rr, C, family, 1.0)["loss"])
    print(f"kl R={Rr} C={C} {family}: loss {el:.2e} (bound {R.KL_LOSS_BOUND:.1e})")
    assert el < R.KL_LOSS_BOUND
    for gout in R.GOUTS:
        ref = R.kl_reference(Rr, C, family, gout)
        ga, gb = torch.autograd.grad(loss, (a, b), grad_outputs=_gout(gout, loss), retain_graph=True)
        assert tuple(ga.shape) == (Rr, C) and tuple(gb.shape) == (Rr, C)
        assert torch.isfinite(ga).all().item() and torch.isfinite(gb).all().item()
        ea, eb = R.elem_error(_np(ga), ref["ga"], ref["s"]), R.elem_error(_np(gb), ref["gb"], ref["s"])
        print(f"    gout {gout}: ga {ea:.2e}, gb {eb:.2e} (bound {R.KL_ELEM_BOUND:.1e})")
        assert max(ea, eb) < R.KL_ELEM_BOUND, (gout, ea, eb)
        if C == 1:
            assert loss.item() == 0.0 and not ga.any().item() and not gb.any().item()


def test_kl_divergence_of_a_tensor_with_itself_is_zero():
    ops, L = _mods()
    for family in R.KL_FAMILIES:
        a = _leaf(R.kl_case(64, 257, family)[0])
        loss = L.kl_divergence(a, a)
        assert loss.item() == 0.0
        direct = ops.kl_div_fwd_bwd(a.detach(), a.detach().clone())
        assert direct[0].item() == 0.0 and not direct[2].any().item()
    e = torch.empty(0, 8, device=DEV)
    assert torch.isnan(L.kl_divergence(e, e)).item()
