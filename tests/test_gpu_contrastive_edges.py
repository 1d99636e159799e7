"""The unit-row contrastive kernels (csrc/contrastive.hip: NCL's table InfoNCE, SSL4Rec's batch softmax) and the k-means
kernels (csrc/ncl.hip) against float64 at the edges of their tiles and of the pass-1 chunk schedule, on degenerate rows,
and at the underflow envelope of exp((s - 1) / tau).  DESIGN.md 4.15; the references, the seeded cases and the per-row
error measure are tests/contrastive_ref.py, their premises tests/test_contrastive_ref_cpu.py.

Bounds: loss <= 1e-5 relative, gradients <= 1e-4 per row (row_errors, floor FLOOR_FRAC).  Every
test prints its worst figures."""
import functools

import numpy as np
import pytest
import torch

from tests import contrastive_ref as R
from tests import ncl_ref

pytestmark = pytest.mark.gpu
CALLS = R.table_calls()


def _worst(name, **figs):
    print(f"[{name}] " + "  ".join(f"{k} {v:.2e}" for k, v in figs.items()))


def _rows(got, want, rows=None):
    """the worst per-row error, over all rows or over a subset measured on its own"""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    if rows is not None:
        got, want = got[rows], want[rows]
    return float(R.row_errors(got, want, R.FLOOR_FRAC).max())


def _check_table(q, t, idx, tau, scale, out):
    """one problem of a table call against float64 -> (loss error, gq figure, gt figure)"""
    loss, gq, gt = out
    wl, wq, wt = R.table_nce(q, t, idx, tau, scale)
    N, d = len(t), q.shape[1]
    assert torch.isfinite(loss).item() and torch.isfinite(gq).all() and torch.isfinite(gt).all()
    assert gq.shape == q.shape and gt.shape == t.shape
    if N == 1:                      # the exact loss is 0: the bound is absolute, 1e-5 of the logits' range
        le = abs(float(loss) - wl) * tau
    else:
        le = abs(float(loss) - wl) / abs(wl)
    assert le <= R.LOSS_TOL, (float(loss), wl)
    if R.is_zero_gradient(N, d):    # exact zeros: measured against what cancels in them (cancel_scales)
        sq, st = R.cancel_scales(q, t, idx, tau, scale)
        eq = float(((gq.double().cpu() - wq).abs().amax(1) / sq).max())
        et = float(((gt.double().cpu() - wt).abs().amax(1) / st).max())
    else:
        eq, et = _rows(gq, wq), _rows(gt, wt)
    assert eq <= R.GRAD_TOL and et <= R.GRAD_TOL, (eq, et)
    return le, eq, et


def _run_table(probs, tau):
    from selfrec_amd import ops
    torch.cuda.set_device(0)
    return ops.table_nce_fwd_bwd([(q.cuda(), t.cuda(), idx.cuda(), s) for q, t, idx, s in probs], tau=tau)


# ---- a. table InfoNCE at tile and chunk edges -----------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CALLS)), ids=[c[0] for c in CALLS])
def test_table_nce_tile_and_chunk_edges(i):
    name, tau, probs = CALLS[i]
    got = _run_table(probs, tau)
    figs = [_check_table(q, t, idx, tau, s, out) for (q, t, idx, s), out in zip(probs, got)]
    _worst(name, loss=max(f[0] for f in figs), gq=max(f[1] for f in figs), gt=max(f[2] for f in figs))


# ---- b. degenerate rows ---------------------------------------------------------------------------------------------
def _split(n, rows):
    m = torch.zeros(n, dtype=torch.bool)
    m[list(rows)] = True
    return m


def test_table_nce_zero_and_clamped_rows():
    c = R.DEGENERATE
    q, t, idx = R.degenerate_problem()
    (loss, gq, gt), = _run_table([(q, t, idx, 1.0)], c["tau"])
    wl, wq, wt = R.table_nce(q, t, idx, c["tau"], 1.0)
    assert torch.isfinite(loss).item() and torch.isfinite(gq).all() and torch.isfinite(gt).all()
    le = abs(float(loss) - wl) / abs(wl)
    # the clamped rows' gradients are g / 1e-12 (in float64 too): each group of rows is measured on its own scale
    cq, ck = _split(c["B"], c["clamped_q"]), _split(c["N"], c["clamped_t"])
    figs = dict(loss=le, gq=_rows(gq, wq, ~cq), gq_clamped=_rows(gq, wq, cq), gt=_rows(gt, wt, ~ck), gt_clamped=_rows(gt, wt, ck))
    _worst("degenerate rows", **figs)
    assert le <= R.LOSS_TOL
    assert all(v <= R.GRAD_TOL for k, v in figs.items() if k != "loss"), figs


def test_table_nce_index_outside_the_table():
    c = R.DEGENERATE
    q, t, idx = R.degenerate_problem()
    bad = idx.clone()
    bad[2], bad[11] = -1, c["N"]
    (loss, gq, gt), = _run_table([(q, t, bad, 1.0)], c["tau"])
    assert torch.isnan(loss).item()
    _, wq, _ = R.table_nce(q, t, idx, c["tau"], 1.0)         # dL/dq_b depends on no other query's idx
    rest = ~_split(c["B"], (2, 11) + c["clamped_q"])
    fig = dict(gq=_rows(gq, wq, rest), gq_clamped=_rows(gq, wq, _split(c["B"], c["clamped_q"])))
    _worst("idx outside the table", **fig)
    assert max(fig.values()) <= R.GRAD_TOL, fig


# ---- c. batch softmax -----------------------------------------------------------------------------------------------
def _check_softmax(u, v, tau, out):
    loss, gu, gv = out
    B = len(u)
    wl, wu, wv = R.batch_softmax(u, v, tau)
    assert torch.isfinite(loss).item() and torch.isfinite(gu).all() and torch.isfinite(gv).all()
    assert gu.shape == u.shape and gv.shape == v.shape
    if B == 1:
        # the floors of test_batch_softmax_matches_float64: the loss is -log(1 + 1e-5) with p_bb = 1 to within f32
        # rounding, the exact gradient is zero and the kernel's is f32 rounding, measured against 1e-2
        le = max(abs(float(loss) - wl) - 1e-6, 0.0) / abs(wl)
        eu, ev = (float((g.double().cpu() - w).abs().max()) / max(float(w.abs().max()), 1e-2) for g, w in ((gu, wu), (gv, wv)))
    else:
        le = abs(float(loss) - wl) / abs(wl)
        eu, ev = _rows(gu, wu), _rows(gv, wv)
    assert le <= R.LOSS_TOL, (float(loss), wl)
    assert eu <= R.GRAD_TOL and ev <= R.GRAD_TOL, (eu, ev)
    return le, eu, ev


def _run_softmax(u, v, tau):
    from selfrec_amd import ops
    torch.cuda.set_device(0)
    return ops.batch_softmax_fwd_bwd(u.cuda(), v.cuda(), tau)


@pytest.mark.parametrize("B", R.SOFTMAX_B)
def test_batch_softmax_tile_edges(B):
    figs = []
    for d in R.SOFTMAX_D:
        for tau in R.SOFTMAX_TAU:
            u, v = R.softmax_problem(B, d)
            if B > 3 and tau == 0.07:                      # the anti-aligned third: p_bb far below 1e-5, w_b matters
                un, vn = (torch.nn.functional.normalize(x.double(), dim=1) for x in (u, v))
                assert float(torch.softmax(un @ vn.T / tau, dim=1).diagonal().min()) < 1e-7
            figs.append(_check_softmax(u, v, tau, _run_softmax(u, v, tau)))
    _worst(f"batch softmax B={B}", loss=max(f[0] for f in figs), gu=max(f[1] for f in figs), gv=max(f[2] for f in figs))


def test_batch_softmax_zero_rows():
    z = R.SOFTMAX_ZERO
    u, v = R.softmax_problem(z["B"], z["d"], seed=z["seed"], zero_rows=True)
    assert not u[z["u_row"]].any() and not v[z["v_row"]].any()
    loss, gu, gv = _run_softmax(u, v, z["tau"])
    wl, wu, wv = R.batch_softmax(u, v, z["tau"])
    assert torch.isfinite(loss).item() and torch.isfinite(gu).all() and torch.isfinite(gv).all()
    cu, cv = _split(z["B"], (z["u_row"],)), _split(z["B"], (z["v_row"],))
    figs = dict(loss=abs(float(loss) - wl) / abs(wl), gu=_rows(gu, wu, ~cu), gu_clamped=_rows(gu, wu, cu),
                gv=_rows(gv, wv, ~cv), gv_clamped=_rows(gv, wv, cv))
    _worst("batch softmax, zero rows", **figs)
    assert figs["loss"] <= R.LOSS_TOL
    assert all(x <= R.GRAD_TOL for k, x in figs.items() if k != "loss"), figs


# ---- d. the same bits twice -----------------------------------------------------------------------------------------
def test_same_bits_twice():
    _, tau, probs = CALLS[len(R.TABLE_SHAPES)]                   # (512, 4100) + (65, 257)
    assert [(len(p[0]), len(p[1])) for p in probs] == [(512, 4100), (65, 257)]
    first = [tuple(x.clone() for x in r) for r in _run_table(probs, tau)]
    for a, b in zip(first, _run_table(probs, tau)):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    u, v = R.softmax_problem(129, 64)
    first = tuple(x.clone() for x in _run_softmax(u, v, 0.07))
    for x, y in zip(first, _run_softmax(u, v, 0.07)):
        assert torch.equal(x, y)


# ---- e. the underflow envelope --------------------------------------------------------------------------------------
@pytest.mark.parametrize("softmax", [False, True], ids=["table", "softmax"])
def test_inside_the_underflow_envelope(softmax):
    q, t, idx, tau = R.envelope_problem("inside", softmax)
    if softmax:
        le, eq, et = _check_softmax(q, t, tau, _run_softmax(q, t, tau))
    else:
        le, eq, et = _check_table(q, t, idx, tau, 1.0, _run_table([(q, t, idx, 1.0)], tau)[0])
    _worst(f"envelope inside, tau={tau}", loss=le, gq=eq, gt=et)


@pytest.mark.parametrize("kind", ["outside", "band"])
@pytest.mark.parametrize("softmax", [False, True], ids=["table", "softmax"])
def test_outside_the_underflow_envelope_the_loss_is_nan(kind, softmax):
    """a query whose every exp((s - 1)/tau) underflows (outside: to 0; band: to subnormals) has no usable row sum: the
    float64 loss is finite, the kernel's must be NaN, never a number"""
    q, t, idx, tau = R.envelope_problem(kind, softmax)
    want = R.batch_softmax(q, t, tau)[0] if softmax else R.table_nce(q, t, idx, tau, 1.0)[0]
    assert np.isfinite(want)
    loss = _run_softmax(q, t, tau)[0] if softmax else _run_table([(q, t, idx, 1.0)], tau)[0][0]
    print(f"[envelope {kind}, tau={tau}] float64 loss {want:.6g}, kernel {float(loss)}")
    assert torch.isnan(loss).item(), float(loss)


# ---- f. k-means assign ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _assign_cases():
    return R.assign_cases()


@pytest.mark.parametrize("i", range(len(R.ASSIGN_SHAPES)), ids=[f"{n}x{k}x{d}" for n, k, d in R.ASSIGN_SHAPES])
def test_kmeans_assign_edges(i):
    from selfrec_amd import ops
    torch.cuda.set_device(0)
    cs = _assign_cases()[i]
    x, c = cs["x"], cs["c"]
    ids, dist = ops.kmeans_assign(torch.from_numpy(x).cuda(), torch.from_numpy(c).cuda())
    ids, dist = ids.cpu().numpy().astype(np.int64), dist.cpu().numpy().astype(np.float64)
    full, best, _ = R.assign_f64(x, c)
    _, _, scale = R.distinct_gap(x, c)
    # every row's float64 gap is >= 1e-3 of its scale, the planted copies aside, where the lowest id is best: exact ids
    assert np.array_equal(ids, best), np.flatnonzero(ids != best)
    err = float((np.abs(dist - full[np.arange(len(x)), best]) / scale).max())
    _worst(f"assign {x.shape[0]}x{c.shape[0]}x{x.shape[1]}", dist=err)
    assert (dist >= 0).all() and err <= 1e-5


# ---- g. k-means update ----------------------------------------------------------------------------------------------
UPDATES = list(zip(R.UPDATE_SHAPES, R.update_cases())) + [((9, 3, 64), R.update_cases()[-1])]


@pytest.mark.parametrize("i", range(len(UPDATES)), ids=[f"{n}x{k}x{d}" for (n, k, d), _ in UPDATES[:-1]] + ["all-invalid"])
def test_kmeans_update_edges(i):
    from selfrec_amd import ops
    torch.cuda.set_device(0)
    (n, k, d), (x, ids) = UPDATES[i]
    cent, counts = ops.kmeans_update(torch.from_numpy(x).cuda(), torch.from_numpy(ids).cuda(), k)
    cent, counts = cent.cpu().numpy(), counts.cpu().numpy()
    want_c, want_n = R.kmeans_update_f32(x, ids, k)
    ok = (ids >= 0) & (ids < k)
    c64, n64 = ncl_ref.update_np(x[ok], ids[ok].astype(np.int64), k)
    assert np.array_equal(counts, want_n) and np.array_equal(want_n, n64)
    if i == len(UPDATES) - 1:
        assert not ok.any() and not counts.any() and not cent.any()
    err = float(R.row_errors(cent, c64, R.FLOOR_FRAC).max())
    diff = int((cent.view(np.uint32) != want_c.view(np.uint32)).sum())
    _worst(f"update {n}x{k}x{d}", float64=err, differing_words=float(diff))
    assert diff == 0                       # bit for bit the ascending-row float32 sum times 1 / count
    assert err <= 1e-6
