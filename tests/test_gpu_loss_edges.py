"""The drop-in loss functions (util/loss_torch.py) on the device against float64, at the single-launch kernels' own edges
(csrc/losses.hip: bpr_plain_fwd / bpr_plain_bwd, l2_reg_fwd_kernel / l2_reg_bwd_kernel): every BPR family, width and row count
of tests/loss_ref.py row by row, every L2 block and call element by element, the wrappers (strides, streams, repeats,
broadcast operands, the wide ATen route) and InfoNCE / batch_softmax_loss through their wrappers at padded widths.  The bounds
are MARGIN x the f32-torch-on-the-CPU yardsticks that tests/test_loss_ref_cpu.py measures."""
import warnings

import numpy as np
import pytest
import torch

from tests import contrastive_ref, loss_ref as R, nce_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _mods():
    from selfrec_amd import ops
    from selfrec_amd.util import loss_torch as L
    torch.cuda.set_device(0)
    return ops, L


def _leaf(a, device=DEV):
    return torch.tensor(np.asarray(a), dtype=torch.float32).to(device).requires_grad_(True)


def _gout(value, like):
    return torch.tensor(float(value), dtype=torch.float32, device=like.device)


def _np(t):
    return t.detach().cpu().numpy()


def _ws_is_zero(ops):
    return not ops.scalar_ws(torch.device(DEV)).any().item()


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32))


def _bpr_row_figures(grads, ref):
    return {g: R.row_error(_np(t), ref[g], ref[s]) for t, (g, s) in zip(grads, (("gu", "s_u"), ("gp", "s_p"), ("gn", "s_n")))}


# ---- a. BPR ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("shape", R.bpr_shapes(), ids=lambda s: "B%d_d%d" % s)
def test_bpr_loss_row_by_row(shape, family):
    ops, L = _mods()
    B, d = shape
    u, p, n = (_leaf(a) for a in R.bpr_case(B, d, family))
    loss = L.bpr_loss(u, p, n)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    assert _ws_is_zero(ops)
    ref = R.bpr_reference(B, d, family, 1.0)
    el = R.loss_error(loss.item(), ref["loss"])
    # coef, as the forward kernel leaves it for the backward one
    w = ops.padded_width(d, ops.ROW_WIDTHS)
    padded = [ops.pad_cols(t.detach(), w) for t in (u, p, n)]
    direct, coef = torch.empty((), device=DEV), torch.full((B,), float("nan"), device=DEV)
    ops.bpr_fwd(*padded, direct, coef)
    assert _ws_is_zero(ops)
    ec = R.elem_error(_np(coef), ref["coef"], ref["s_coef"])
    print(f"bpr B={B} d={d} {family}: loss {el:.2e} (bound {R.LOSS_BOUND:.1e}), coef {ec:.2e} (bound {R.ROW_BOUND:.1e})")
    assert _bits(direct, loss)
    assert el < R.LOSS_BOUND and ec < R.ROW_BOUND
    for gout in R.GOUTS:
        ref = R.bpr_reference(B, d, family, gout)
        grads = torch.autograd.grad(loss, (u, p, n), grad_outputs=_gout(gout, loss), retain_graph=True)
        assert _ws_is_zero(ops)
        assert all(tuple(g.shape) == (B, d) for g in grads)                      # the caller's width, not the kernel's
        figs = _bpr_row_figures(grads, ref)
        print(f"    gout {gout}: " + ", ".join(f"{k} {v:.2e}" for k, v in figs.items()))
        assert max(figs.values()) < R.ROW_BOUND, (gout, figs)
        if gout == 0.0:
            assert not any(g.any().item() for g in grads)


def test_bpr_loss_on_zero_rows_of_device_tensors_is_nan():
    ops, L = _mods()
    for d in (64, 50):
        e = torch.empty(0, d, device=DEV, requires_grad=True)
        out = L.bpr_loss(e, e, e)
        assert out.is_cuda and torch.isnan(out).item()
    assert _ws_is_zero(ops)


# ---- b. L2 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(R.L2_CALLS)),
                         ids=lambda i: R.L2_CALLS[i]["route"] + "_" + "+".join("x".join(map(str, k)) if k != R.ZERO else k
                                                                               for k in R.L2_CALLS[i]["slots"]))
def test_l2_reg_loss_element_by_element(index):
    ops, L = _mods()
    call = R.L2_CALLS[index]
    names = call["slots"]
    on_cpu = {names[j] for j in call["cpu"]}
    leaves = {k: _leaf(R.block(k), "cpu" if k in on_cpu else DEV) for k in dict.fromkeys(names)}
    args = [leaves[k] for k in names]
    loss = L.l2_reg_loss(R.REG, *args)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    assert _ws_is_zero(ops)
    ref = R.l2_reference(index, 1.0)
    el = R.loss_error(loss.item(), ref["loss"])
    # the norms, as the forward kernel leaves them for the backward one: the whole call where it is one launch, else per block
    groups = [list(range(len(names)))] if call["route"] == "launch" else [[j] for j, k in enumerate(names) if k not in on_cpu]
    en = 0.0
    for slots in groups:
        xs = [args[j].detach() for j in slots]
        norms, direct = torch.full((len(xs),), float("nan"), device=DEV), torch.empty((), device=DEV)
        ops.l2_reg_fwd(xs, R.REG, norms, direct)
        assert _ws_is_zero(ops)
        if call["route"] == "launch":
            assert _bits(direct, loss)
        for j, got in zip(slots, _np(norms).astype(np.float64)):
            want = ref["norms"][j]
            if want == 0.0:
                assert got == 0.0
            else:
                en = max(en, abs(got - want) / want)
    print(f"l2 {names} {call['route']}: loss {el:.2e} (bound {R.LOSS_BOUND:.1e}), norms {en:.2e} (bound {R.NORM_BOUND:.1e})")
    assert el < R.LOSS_BOUND and en < R.NORM_BOUND
    for gout in R.GOUTS:
        want = R.l2_by_tensor(R.l2_reference(index, gout), names)
        grads = torch.autograd.grad(loss, list(leaves.values()), grad_outputs=_gout(gout, loss), retain_graph=True)
        assert _ws_is_zero(ops)
        figs = {}
        for k, g in zip(leaves, grads):
            assert g.shape == leaves[k].shape and g.device == leaves[k].device
            figs[k] = R.elem_error(_np(g), want[k][0], np.full(want[k][0].shape, want[k][1]))
        print(f"    gout {gout}: " + ", ".join(f"{k} {v:.2e}" for k, v in figs.items()))
        assert max(figs.values()) < R.ELEM_BOUND, (gout, figs)


# ---- c. the wrappers ------------------------------------------------------------------------------------------------------
def _strided_operands(B, d, seed):
    """(u, p, n) as non-leaf views with gradients: a column slice of a wider tensor, a transposed tensor, an expanded row"""
    g = torch.Generator().manual_seed(seed)
    wide = (torch.randn(B, d + 7, generator=g) * 0.3).to(DEV).requires_grad_(True)
    tall = (torch.randn(d, B, generator=g) * 0.3).to(DEV).requires_grad_(True)
    row = (torch.randn(1, d, generator=g) * 0.3).to(DEV).requires_grad_(True)
    views = wide[:, 3:3 + d], tall.t(), row.expand(B, d)
    assert not any(v.is_contiguous() for v in views)
    return views


def _copies(views):
    return tuple(v.detach().contiguous().requires_grad_(True) for v in views)


@pytest.mark.parametrize("d", [64, 50])
def test_non_contiguous_operands_give_the_bits_of_their_contiguous_copies(d):
    ops, L = _mods()
    B = 37
    views = _strided_operands(B, d, 11)
    copies = _copies(views)
    for fn in (lambda t: L.bpr_loss(*t), lambda t: L.l2_reg_loss(R.REG, *t)):
        a, b = fn(views), fn(copies)
        assert _bits(a, b)
        ga = torch.autograd.grad(a, views, grad_outputs=_gout(3.7, a))
        gb = torch.autograd.grad(b, copies, grad_outputs=_gout(3.7, b))
        assert all(_bits(x, y) for x, y in zip(ga, gb))
        assert _ws_is_zero(ops)
    ref = R.bpr(*(_np(c) for c in copies), 1.0)                    # (and the value is the restatement's, not only repeatable)
    assert R.loss_error(L.bpr_loss(*views).item(), ref["loss"]) < R.LOSS_BOUND


def _both_losses(L, leaves):
    bpr, reg = L.bpr_loss(*leaves), L.l2_reg_loss(R.REG, *leaves)
    grads = torch.autograd.grad(bpr * 3.7 + reg * -2.5, leaves)
    return (bpr, reg) + grads


def test_a_side_stream_gives_the_default_streams_bits_and_leaves_both_workspaces_zero():
    ops, L = _mods()
    leaves = tuple(_leaf(a) for a in R.bpr_case(R.MANY_ROWS, 64, "mixed"))
    here = _both_losses(L, leaves)
    ws_default = ops.scalar_ws(torch.device(DEV))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        there = _both_losses(L, tuple(t.detach().requires_grad_(True) for t in leaves))
        ws_side = ops.scalar_ws(torch.device(DEV))
        side.synchronize()
        assert ws_side.data_ptr() != ws_default.data_ptr()          # one workspace per device AND stream
        assert not ws_side.any().item()
    torch.cuda.synchronize()
    assert not ws_default.any().item()
    assert all(_bits(a, b) for a, b in zip(here, there))


def test_each_function_twice_and_each_backward_twice_give_the_same_bits():
    ops, L = _mods()
    leaves = tuple(_leaf(a) for a in R.bpr_case(R.MANY_ROWS, 128, "mixed"))
    for fn in (lambda: L.bpr_loss(*leaves), lambda: L.l2_reg_loss(R.REG, *leaves, leaves[0])):
        a, b = fn(), fn()
        assert _bits(a, b)
        g1 = torch.autograd.grad(a, leaves, grad_outputs=_gout(-2.5, a), retain_graph=True)
        g2 = torch.autograd.grad(a, leaves, grad_outputs=_gout(-2.5, a), retain_graph=True)
        g3 = torch.autograd.grad(b, leaves, grad_outputs=_gout(-2.5, b))
        assert all(_bits(x, y) and _bits(x, z) for x, y, z in zip(g1, g2, g3))
        assert _ws_is_zero(ops)


# ---- d. broadcast operands (the fixed wrapper only: the kernels take B and the width from one operand) --------------------
@pytest.mark.parametrize("which", ["p_1xd", "n_Bx1", "u_1xd"])
@pytest.mark.parametrize("d", [64, 50])
def test_bpr_loss_broadcasts_like_the_reference(which, d):
    ops, L = _mods()
    B = 33
    u, p, n = (np.array(a) for a in R.bpr_case(B, d, "mixed"))
    if which == "p_1xd":
        p = p[7:8]
    elif which == "n_Bx1":
        n = n[:, 2:3]
    else:
        u = u[5:6] * np.float32(0.25)              # (one user row against every pair: scaled so that the margins stay moderate)
    shapes = [a.shape for a in (u, p, n)]
    full = [np.ascontiguousarray(np.broadcast_to(a, (B, d))) for a in (u, p, n)]
    tu, tp, tn = _leaf(u), _leaf(p), _leaf(n)
    assert tuple(t.shape for t in L._bpr_operands(tu, tp, tn)) == ((B, d),) * 3       # (on the host: before any launch)
    loss = L.bpr_loss(tu, tp, tn)
    assert _ws_is_zero(ops)
    ref = R.bpr(*full, 3.7)
    el = R.loss_error(loss.item(), ref["loss"])
    grads = torch.autograd.grad(loss, (tu, tp, tn), grad_outputs=_gout(3.7, loss))
    figs = {}
    for name, g, shape, key, skey in zip("upn", grads, shapes, ("gu", "gp", "gn"), ("s_u", "s_p", "s_n")):
        assert tuple(g.shape) == shape
        want, scale = ref[key], np.broadcast_to(ref[skey][:, None], (B, d))
        # the gradient of a broadcast operand is the sum over the expanded axis; its scale the sum of the terms' scales
        # (autograd's f32 sum of at most 64 terms adds 6 x 2^-24 of that: far inside the margin)
        for axis in (0, 1):
            if shape[axis] == 1:
                want, scale = want.sum(axis=axis, keepdims=True), scale.sum(axis=axis, keepdims=True)
        figs[name] = R.elem_error(_np(g), want, scale)
    print(f"bpr broadcast {which} d={d}: loss {el:.2e}, gradients {figs}")
    assert el < R.LOSS_BOUND and max(figs.values()) < R.ROW_BOUND, figs


@pytest.mark.parametrize("shapes", [((5, 64), (2, 64), (5, 64)), ((5, 64), (5, 50), (5, 64)), ((5, 50), (5, 50), (5, 40)),
                                    ((5, 64), (5, 64), (4, 1))])
def test_bpr_loss_refuses_operands_that_do_not_broadcast_before_any_launch(shapes):
    ops, L = _mods()
    u, p, n = (torch.zeros(*s, device=DEV) for s in shapes)
    with pytest.raises(RuntimeError, match="must match"):
        L.bpr_loss(u, p, n)
    assert _ws_is_zero(ops)


# ---- e. the wide route: ATen on the device, announced once ------------------------------------------------------------------
def _nce_problem(n, d, seed):
    rng = np.random.default_rng([seed, n, d])
    v1 = (rng.standard_normal((n, d)) * 0.4).astype(np.float32)
    v2 = (v1 + rng.standard_normal((n, d)) * 0.2).astype(np.float32)
    return v1, v2


def _check_nce(loss, g1, g2, v1, v2, tau, scale, precision, tag):
    wl, w1, w2 = nce_ref.info_nce_rows(v1, v2, None, tau, scale)
    el = abs(loss * scale - wl) / abs(wl)
    e1 = float(nce_ref.row_errors(g1, w1, nce_ref.FLOOR_FRAC).max())
    e2 = float(nce_ref.row_errors(g2, w2, nce_ref.FLOOR_FRAC).max())
    bound = nce_ref.ROW_BOUND_F32 if precision == "f32" else nce_ref.ROW_BOUND_SPLIT
    print(f"{tag} {precision}: loss {el:.2e} (bound {nce_ref.LOSS_BOUND[precision]:.0e}), g1 {e1:.2e}, g2 {e2:.2e} "
          f"(bound {bound:.2e})")
    assert el < nce_ref.LOSS_BOUND[precision]
    assert e1 < bound and e2 < bound


def test_wide_rows_take_the_aten_route_and_warn_once_per_function():
    ops, L = _mods()
    B, d, tau = 33, 300, 0.2
    assert d > ops.ROW_WIDTHS[-1] and d > ops.NCE_WIDTHS[-1]
    rng = np.random.default_rng(300)
    u, p, n = ((rng.standard_normal((B, d)) * 0.3).astype(np.float32) for _ in range(3))
    v1, v2 = _nce_problem(17, d, 3)
    saved = list(L._warned_wide)
    L._warned_wide.clear()
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            for _ in range(2):
                tu, tp, tn = _leaf(u), _leaf(p), _leaf(n)
                bpr = L.bpr_loss(tu, tp, tn)
                gb = torch.autograd.grad(bpr, (tu, tp, tn), grad_outputs=_gout(3.7, bpr))
                t1, t2 = _leaf(v1), _leaf(v2)
                nce = L.InfoNCE(t1, t2, tau)
                gn = torch.autograd.grad(nce, (t1, t2), grad_outputs=_gout(3.7, nce))
        ours = [str(w.message) for w in caught if issubclass(w.category, RuntimeWarning)]
        assert sum(m.startswith("bpr_loss") for m in ours) == 1, ours
        assert sum(m.startswith("InfoNCE") for m in ours) == 1, ours
        assert len(ours) == 2 and all("300 columns" in m for m in ours), ours
        assert sorted(L._warned_wide) == ["InfoNCE", "bpr_loss"]
    finally:
        L._warned_wide[:] = saved
    # another f32 evaluation of the same expressions: held to what the kernels are held to
    ref = R.bpr(u, p, n, 3.7)
    el, figs = R.loss_error(bpr.item(), ref["loss"]), _bpr_row_figures(gb, ref)
    print(f"wide bpr d={d}: loss {el:.2e}, rows {figs}")
    assert el < R.LOSS_BOUND and max(figs.values()) < R.ROW_BOUND
    _check_nce(nce.item(), gn[0], gn[1], v1, v2, tau, 3.7, "f32", f"wide InfoNCE d={d}")
    assert _ws_is_zero(ops)


# ---- f. InfoNCE and batch_softmax_loss through their wrappers at padded widths -----------------------------------------------
def _column_slice(a):
    """a device leaf whose columns 2 .. 2 + d are `a`, and that non-contiguous view"""
    wide = np.zeros((a.shape[0], a.shape[1] + 5), dtype=np.float32)
    wide[:, 2:2 + a.shape[1]] = a
    base = _leaf(wide)
    view = base[:, 2:2 + a.shape[1]]
    assert not view.is_contiguous() or a.shape[0] == 1
    return base, view


@pytest.mark.parametrize("d", [50, 96, 200])
@pytest.mark.parametrize("n", [2, 17, 65])
def test_infonce_through_loss_torch_at_padded_widths(n, d):
    ops, L = _mods()
    tau, scale = 0.2, 3.7
    v1, v2 = _nce_problem(n, d, 1)
    base, view = _column_slice(v1)
    t2 = _leaf(v2)
    loss = L.InfoNCE(view, t2, tau)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    (loss * scale).backward()
    g1 = base.grad[:, 2:2 + d]
    assert tuple(t2.grad.shape) == (n, d)
    assert not base.grad[:, :2].any() and not base.grad[:, 2 + d:].any()
    w = ops.padded_width(d, ops.NCE_WIDTHS)
    precision = "split" if w == 256 else ops.get_infonce_precision()          # (256 columns: the split path only)
    _check_nce(loss.item(), g1, t2.grad, v1, v2, tau, scale, precision, f"InfoNCE n={n} d={d} -> {w}")


@pytest.mark.parametrize("d", [50, 96])
@pytest.mark.parametrize("n", [2, 17, 65])
def test_batch_softmax_loss_through_loss_torch_at_padded_widths(n, d):
    ops, L = _mods()
    tau, scale = 0.07, 3.7
    u, v = contrastive_ref.softmax_problem(n, d)
    tu = u.to(DEV).requires_grad_(True)
    base, view = _column_slice(v.numpy())
    loss = L.batch_softmax_loss(tu, view, tau)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    (loss * scale).backward()
    gv = base.grad[:, 2:2 + d]
    assert tuple(tu.grad.shape) == (n, d)
    assert not base.grad[:, :2].any() and not base.grad[:, 2 + d:].any()
    wl, wu, wv = contrastive_ref.batch_softmax(u, v, tau)
    el = abs(loss.item() - wl) / abs(wl)
    eu = float(contrastive_ref.row_errors(tu.grad, scale * wu, contrastive_ref.FLOOR_FRAC).max())
    ev = float(contrastive_ref.row_errors(gv, scale * wv, contrastive_ref.FLOOR_FRAC).max())
    print(f"batch_softmax_loss n={n} d={d}: loss {el:.2e} (bound {contrastive_ref.LOSS_TOL:.0e}), gu {eu:.2e}, gv {ev:.2e} "
          f"(bound {contrastive_ref.GRAD_TOL:.0e})")
    assert el <= contrastive_ref.LOSS_TOL and eu <= contrastive_ref.GRAD_TOL and ev <= contrastive_ref.GRAD_TOL


@pytest.mark.parametrize("shapes", [((17, 50), (16, 50)), ((17, 50), (17, 64)), ((17, 64), (1, 64))])
def test_infonce_and_batch_softmax_refuse_mismatched_shapes_before_any_launch(shapes):
    ops, L = _mods()
    a, b = (torch.ones(*s, device=DEV) for s in shapes)
    with pytest.raises(ops.SelfrecHipError, match="same shape"):
        L.InfoNCE(a, b, 0.2)
    with pytest.raises(ops.SelfrecHipError, match="same shape"):
        L.batch_softmax_loss(a, b, 0.07)
