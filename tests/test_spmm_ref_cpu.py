"""tests/spmm_ref.py -- the float64 restatement the GPU epilogue tests assert against -- held to the project's other CPU
stand-ins, so that it cannot be wrong in the same way as the kernel: the oracle's propagate (XSimGCL_Encoder.forward) for
PERTURB + MEAN, tests/cpu_ops.spmm for marks and AXPY, D^-1/2 A D^-1/2 built explicitly with scipy for the three scaling
masks, torch.optim.Adam in float64 for adam_ref.  Float64 against float64: 1e-12 relative.  No GPU."""
import numpy as np
import scipy.sparse as sp
import torch

from oracle import selfrec_oracle as O

from . import cpu_ops
from . import spmm_ref as R
from .test_gpu_kernels import powerlaw_csr

REL = 1e-12


def rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


def _graph(n=400):
    return powerlaw_csr(n, n, 5000, seed=23, heavy_rows=2, heavy_len=300, empty_rows=10)


def _sparse64(m):
    return O.to_torch_sparse(m).to(torch.float64)          # (float32 values, promoted: exact)


class _CSR64(cpu_ops.DeviceCSR):
    """cpu_ops' matrix with its torch sparse tensor in float64"""
    @property
    def _m(self):
        return super()._m.to(torch.float64)


def _t(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


def test_mean_and_perturb_equal_the_oracle_encoder():
    """Three layers of XSimGCL.py:83-96 (product, perturbation, mean over the layers) = three epilogue_ref launches, the last
    with MEAN over the two earlier outputs."""
    m = _graph()
    s = R.epilogue_inputs(m, 16, seed=1)
    noises = [np.random.default_rng(k).random(s["x"].shape).astype(np.float32) for k in range(3)]
    eps32 = float(np.float32(0.2))                            # (the C struct carries eps as a float)
    final, cl = O.propagate(_sparse64(m), _t(s["x"]), 3, include_ego=False, eps=eps32, noises=[_t(z) for z in noises], layer_cl=2)
    y1, _, _, _ = R.epilogue_ref(m, s["x"], noise=noises[0], eps=0.2)
    y2, _, _, _ = R.epilogue_ref(m, y1, noise=noises[1], eps=0.2)
    y3, mean, by, bm = R.epilogue_ref(m, y2, noise=noises[2], eps=0.2, prev=[y1, y2], mean_div=3.0)
    assert rel(y2, cl.numpy()) < REL and rel(mean, final.numpy()) < REL
    assert by.shape == y3.shape and bm.shape == mean.shape and (by >= 0).all() and (bm > 0).all()
    # LightGCN.py:68-75: the ego table is one of the averaged tensors, no perturbation; n_prev = 0 is the product itself
    final = O.propagate(_sparse64(m), _t(s["x"]), 1, include_ego=True)
    _, mean, _, _ = R.epilogue_ref(m, s["x"], prev=[s["x"]], mean_div=2.0)
    assert rel(mean, final.numpy()) < REL
    y, mean, _, _ = R.epilogue_ref(m, s["x"], prev=[], mean_div=1.0)
    assert np.array_equal(y, mean)


def test_marks_and_axpy_equal_cpu_ops():
    m = _graph()
    n, d = m.shape[0], 16
    s = R.epilogue_inputs(m, d, seed=2)
    csr = _CSR64(m.indptr, m.indices, m.data, m.shape)
    stamp = torch.tensor([17], dtype=torch.int64)
    mark = lambda live: torch.from_numpy(np.where(live, 17, 3).astype(np.int32))        # noqa: E731
    # AXPY with alpha and two addends; addend-only; alpha-only
    for alpha, add, sc in ((0.25, s["add"], [0.5, 2.0]), (1.0, s["add"][:1], [0.3]), (0.25, [], [])):
        out = torch.zeros(n, d, dtype=torch.float64)
        cpu_ops.spmm(csr, _t(s["x"]), out=out, epilogue=dict(add=[_t(a) for a in add], add_scale=[float(np.float32(c)) for c in sc],
                                                             alpha=alpha))
        y, _, _, _ = R.epilogue_ref(m, s["x"], alpha=alpha, add=add, add_scale=sc)
        assert rel(y, out.numpy()) < REL
    # row marks with MEAN: dead rows keep both outputs; column marks with x zero on the dead columns
    out, mean = torch.full((n, d), 7.0, dtype=torch.float64), torch.full((n, d), 7.0, dtype=torch.float64)
    cpu_ops.spmm(csr, _t(s["x_cols"]), out=out,
                 epilogue=dict(row_mark=mark(s["row_live"]), col_mark=mark(s["col_live"]), mark_stamp=stamp,
                               prev=[_t(s["prev"][0])], mean_div=2.0, mean_out=mean))
    sent = np.full((n, d), 7.0)
    y, mn, by, bm = R.epilogue_ref(m, s["x_cols"], row_live=s["row_live"], col_live=s["col_live"], prev=s["prev"][:1], mean_div=2.0,
                                   y_before=sent, mean_before=sent)
    assert rel(y, out.numpy()) < REL and rel(mn, mean.numpy()) < REL
    assert np.all(y[~s["row_live"]] == 7.0) and np.all(mn[~s["row_live"]] == 7.0) and np.all(by[~s["row_live"]] == 0)
    # the column mask matters to the restatement even where x is NOT zero on dead columns (entries count as zero)
    y2, _, _, _ = R.epilogue_ref(m, s["x"], col_live=s["col_live"])
    assert rel(y2, m.astype(np.float64) @ s["x_cols"].astype(np.float64)) < REL
    # a batch-sparse addend is what cpu_ops gets as a table that IS zero off the live rows
    a_zeroed = s["add"][1] * s["add_live"][:, None]
    out = torch.zeros(n, d, dtype=torch.float64)
    cpu_ops.spmm(csr, _t(s["x"]), out=out, epilogue=dict(add=[_t(s["add"][0]), _t(a_zeroed)], add_scale=[1.0, 0.5], alpha=0.5))
    y, _, _, _ = R.epilogue_ref(m, s["x"], alpha=0.5, add=s["add"], add_scale=[1.0, 0.5], add_sparse=[False, True],
                                add_live=s["add_live"])
    assert rel(y, out.numpy()) < REL
    assert rel(R.epilogue_ref(m, s["x"], alpha=0.5, add=s["add"], add_scale=[1.0, 0.5])[0], out.numpy()) > 1e-3


def test_scaling_masks_equal_explicit_normalised_products():
    """A chain of three layers kept in the pre-scaled domain (pattern products, SCALE_IN / SCALE_OUT, prev_unscale) equals
    three true products with D^-1/2 A D^-1/2 built with scipy; an addend with its row-scale bit enters times r."""
    m = _graph()
    n, d = m.shape[0], 16
    s = R.epilogue_inputs(m, d, seed=3)
    r = s["r"].astype(np.float64)
    assert (r == 0).sum() >= 11 and r[int(np.argmax(np.diff(m.indptr)))] == 0
    P = m.astype(np.float64)
    P.data[:] = 1.0
    Ahat = sp.diags(r) @ P @ sp.diags(r)
    E = s["x"].astype(np.float64)
    t1, t2, t3 = Ahat @ E, Ahat @ (Ahat @ E), Ahat @ (Ahat @ (Ahat @ E))
    kw = dict(vals_pattern=True, row_scale=s["r"])
    y1s, _, _, _ = R.epilogue_ref(m, r[:, None] * E, scale_in=True, scale_out=True, **kw)
    y2s, _, _, _ = R.epilogue_ref(m, y1s, scale_in=True, scale_out=True, **kw)
    y3, mean, _, _ = R.epilogue_ref(m, y2s, scale_in=True, prev=[y1s, y2s], prev_unscale=[True, True], mean_div=3.0, **kw)
    assert rel(y1s, r[:, None] * t1) < REL and rel(y2s, r[:, None] * t2) < REL and rel(y3, t3) < REL
    assert rel(mean, (t1 + t2 + t3) / 3.0) < REL                # (rows with r = 0: 1 / r counts as 0, and the true rows are 0)
    # MEAN next to SCALE_OUT: mean_out holds true values, y the scaled ones; a prev table without its bit enters as it is
    y, mean, _, _ = R.epilogue_ref(m, y2s, scale_in=True, scale_out=True, prev=[s["prev"][0], y1s], prev_unscale=[False, True],
                                   mean_div=3.0, **kw)
    assert rel(y, r[:, None] * t3) < REL and rel(mean, (s["prev"][0] + t1 + t3) / 3.0) < REL
    # value product with SCALE_OUT alone; addends with and without the row-scale bit
    A = m.astype(np.float64)
    a0, a1 = (a.astype(np.float64) for a in s["add"])
    y, _, _, _ = R.epilogue_ref(m, s["x"], row_scale=s["r"], scale_out=True)
    assert rel(y, r[:, None] * (A @ E)) < REL
    y, _, _, _ = R.epilogue_ref(m, s["x"], row_scale=s["r"], scale_in=True, scale_out=True, alpha=0.25, add=s["add"],
                                add_scale=[0.5, 2.0], add_rowscale=[True, False])
    assert rel(y, r[:, None] * (0.25 * r[:, None] * (A @ E) + 0.5 * r[:, None] * a0 + 2.0 * a1)) < REL


def test_adam_ref_equals_torch_optim_in_float64():
    rng = np.random.default_rng(4)
    p0 = rng.standard_normal((50, 16)) * 0.1
    ref = torch.nn.Parameter(torch.tensor(p0, dtype=torch.float64))
    opt = torch.optim.Adam([ref], lr=1e-3)
    p, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    for step in range(1, 6):
        g = rng.standard_normal(p0.shape) * 10 ** rng.uniform(-6, 0)
        ref.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        p, m, v = R.adam_ref(p, m, v, g, step, 1e-3, 0.9, 0.999, 1e-8)
        assert rel(p, ref.detach().numpy()) < REL
        state = opt.state[ref]
        assert rel(m, state["exp_avg"].numpy()) < REL and rel(v, state["exp_avg_sq"].numpy()) < REL


def test_bounds_hold_a_float32_restatement_and_are_not_vacuous():
    """The tolerances the GPU tests assert, checked against plain float32 numpy arithmetic on the inputs the GPU tests use:
    a float32 evaluation in ANOTHER order (scipy's) stays inside BOUND_FACTOR * bound; the PERTURB skip count stays under
    its cap; the oracle's float32 Adam lies in the hull, and less than 1 % of the hull is ill-conditioned."""
    m = powerlaw_csr(3000, 3000, 40000, seed=23, heavy_rows=3, heavy_len=1500, empty_rows=40)
    d = 64
    s = R.epilogue_inputs(m, d, seed=d)
    y64, mean64, by, bm = R.epilogue_ref(m, s["x"], row_scale=s["r"], scale_in=True, alpha=0.25, add=s["add"], add_scale=[0.5, 2.0],
                                         add_rowscale=[True, False], prev=s["prev"][:3], prev_unscale=[True, False, True],
                                         mean_div=4.0)
    r32 = s["r"][:, None]
    y32 = np.float32(0.25) * ((m @ s["x"]) * r32) + (np.float32(0.5) * r32) * s["add"][0] + np.float32(2.0) * s["add"][1]
    with np.errstate(divide="ignore"):
        rinv = np.where(r32 > 0, np.float32(1) / r32, np.float32(0)).astype(np.float32)
    mean32 = (s["prev"][0] * rinv + s["prev"][1] + s["prev"][2] * rinv + y32) * np.float32(0.25)
    assert y32.dtype == np.float32 and mean32.dtype == np.float32
    assert R.violations(y32, y64, by)[0] == 0 and R.violations(mean32, mean64, bm)[0] == 0
    short = np.diff(m.indptr) == 3
    heavy = int(np.argmax(np.diff(m.indptr)))
    assert short.any() and by[short].max() * 50 < R.epilogue_ref(m, s["x"])[2][heavy].max()      # short rows are held tighter
    assert R.violations(y32 * np.float32(1.00001), y64, by)[0] > 0                              # and 1e-5 relative is caught
    amb, ok = R.sign_ambiguous(R.epilogue_ref(m, s["x"])[0])
    assert ok, int(amb.sum())
    # ADAM
    a = R.adam_inputs(m, d, seed=d)
    lr, b1, b2, eps = (float(np.float32(c)) for c in (1e-3, 0.9, 0.999, 1e-8))
    g64, _, bg, _ = R.epilogue_ref(m, a["x"], alpha=0.25, add=a["add"], add_scale=[0.25, 1.0], add_sparse=[True, True],
                                   add_live=a["add_live"])
    g32 = (np.float32(0.25) * (m @ a["x"]) + (np.float32(0.25) * a["add"][0] + a["add"][1]) * a["add_live"][:, None]).astype(np.float32)
    assert R.violations(g32, g64, bg)[0] == 0
    for step in (1, 7, 100000):
        want = R.adam_bounds(a["p"], a["m"], a["v"], g64, bg, step, lr, b1, b2, eps)
        assert want["ill"].mean() < 0.01, (step, want["ill"].mean())
        p, mm, vv = a["p"].copy(), a["m"].copy(), a["v"].copy()
        O.adam_step(p, g32, mm, vv, step, lr, b1, b2, eps)
        assert np.all((p >= want["p_lo"]) & (p <= want["p_hi"])), step
        assert R.violations(mm, want["m"], want["bound_m"])[0] == 0 and R.violations(vv, want["v"], want["bound_v"])[0] == 0
        assert np.all(want["update"][a["empty"]] == 0) and np.array_equal(p[a["empty"]], a["p"][a["empty"]])
        assert a["empty"].mean() > 0.01
