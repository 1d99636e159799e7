"""Float64 restatement of srh_spmm_f32's epilogue contract, written from the words of include/selfrec_hip.h
(srh_spmm_epilogue_t), not from csrc/spmm.hip -- TEST INFRASTRUCTURE ONLY, host numpy / scipy.

Every function returns, next to the float64 value of each output element, a PER-ELEMENT error bound: the restatement
knows every term that was added to make an element, so it can state the standard forward bound of a float32 sum taken
in ANY order,

    bound = (n_terms + n_ops) * 2^-24 * S            S = sum of |term| in float64

n_terms: the row's stored entries whose column is live, plus addends, plus `prev` tables; n_ops: one per scaling
multiply, two per reciprocal (the kernel multiplies by a rounded 1 / r, 1 / mean_div where torch divides), one per store.
A row of three entries is thereby held hundreds of times tighter than a 1500-entry row next to it.
"""
import numpy as np
import scipy.sparse as sp

U32 = 2.0 ** -24
# Tests assert |got - want| <= BOUND_FACTOR * bound + ABS_FLOOR per element.  Factor 2: second-order terms and the float32
# rounding of scaled intermediates; it is a constant of the derivation, written once, here.
BOUND_FACTOR = 2.0
ABS_FLOOR = 1e-30
# PERTURB adds eps * 2^-22 (the normalisation: sqrt, reciprocal, two multiplies); elements with 0 < |y64| < SIGN_AMBIGUOUS
# are skipped (sign(y) is not decided in float32), at most 4 + 1e-4 * size of them per output.
PERTURB_EXTRA = 2.0 ** -22
SIGN_AMBIGUOUS = 1e-6


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _bits(flags, n):
    flags = list(flags or [])
    return [bool(flags[t]) if t < len(flags) else False for t in range(n)]


def epilogue_ref(A64, x, *, vals_pattern=False, row_scale=None, scale_in=False, scale_out=False, alpha=None, add=(),
                 add_scale=(), add_rowscale=(), add_sparse=(), add_live=None, prev=(), prev_unscale=(), mean_div=None,
                 row_live=None, col_live=None, y_before=None, mean_before=None, noise=None, eps=0.0):
    """-> y64, mean64 (None without MEAN), bound_y, bound_mean.

    A64: scipy CSR (its pattern alone counts when vals_pattern); x, add[t], prev[t], row_scale, noise: the float32 arrays
    the kernel gets.  alpha None = no AXPY.  mean_div None = no MEAN.  row_live / col_live / add_live: boolean masks
    (None = all live).  noise: injected PERTURB noise, whole rows.  In the header's order:
    product (columns that are not live count as zero) -> SCALE_IN -> alpha, addends (add_rowscale: times r; add_sparse:
    skipped on rows that are not add_live) -> PERTURB -> stored y (times r under SCALE_OUT) -> MEAN over prev (prev_unscale:
    times 1 / r, 0 where r = 0) and the UNSCALED y, divided by mean_div.  Rows that are not row_live keep y_before /
    mean_before."""
    A = sp.csr_matrix(A64, dtype=np.float64, copy=True)
    A.sort_indices()
    n = A.shape[0]
    x = _f64(x)
    data = np.ones_like(A.data) if vals_pattern else A.data
    entry_live = np.ones(A.indices.size) if col_live is None else np.asarray(col_live, dtype=bool)[A.indices].astype(np.float64)
    eff = sp.csr_matrix((data * entry_live, A.indices, A.indptr), shape=A.shape)
    n_terms = np.asarray(sp.csr_matrix((entry_live, A.indices, A.indptr), shape=A.shape).sum(axis=1)).reshape(n, 1)
    y = eff @ x
    S = abs(eff) @ np.abs(x)
    n_ops = 0.0
    r = np.ones((n, 1)) if row_scale is None else _f64(row_scale).reshape(n, 1)
    if scale_in:
        y, S, n_ops = y * r, S * np.abs(r), n_ops + 1
    if alpha is not None:
        a32 = float(np.float32(alpha))
        y, S, n_ops = y * a32, S * abs(a32), n_ops + 1
        rs, spm = _bits(add_rowscale, len(add)), _bits(add_sparse, len(add))
        for t, a in enumerate(add):
            sc = float(np.float32(add_scale[t])) * np.ones((n, 1))
            if rs[t]:
                sc, n_ops = sc * r, n_ops + 1
            if spm[t]:
                sc = sc * np.asarray(add_live, dtype=bool).reshape(n, 1)
            term = sc * _f64(a)
            y, S, n_terms = y + term, S + np.abs(term), n_terms + 1
    extra = 0.0
    if noise is not None:
        u = _f64(noise)
        unit = u / np.maximum(np.linalg.norm(u, axis=1, keepdims=True), 1e-12)
        term = np.sign(y) * float(np.float32(eps)) * unit
        y, S, n_terms = y + term, S + np.abs(term), n_terms + 1
        extra = float(np.float32(eps)) * PERTURB_EXTRA
    y_out, S_y, ops_y, extra_y = y, S, n_ops + 1, extra * np.ones((n, 1))
    if scale_out:
        y_out, S_y, ops_y, extra_y = y * r, S * np.abs(r), ops_y + 1, extra_y * np.abs(r)
    bound_y = (n_terms + ops_y) * U32 * S_y + extra_y
    mean = bound_mean = None
    if mean_div is not None:
        m, Sm, n_m, ops_m = y, S, n_terms, n_ops
        un = _bits(prev_unscale, len(prev))
        with np.errstate(divide="ignore"):
            rinv = np.where(r > 0, 1.0 / np.where(r > 0, r, 1.0), 0.0)
        if any(un):
            ops_m += 2
        for t, p in enumerate(prev):
            term = _f64(p)
            if un[t]:
                term, ops_m = term * rinv, ops_m + 1
            m, Sm, n_m = m + term, Sm + np.abs(term), n_m + 1
        div = float(np.float32(mean_div))
        mean, Sm, ops_m = m / div, Sm / abs(div), ops_m + 2 + 1
        bound_mean = (n_m + ops_m) * U32 * Sm + extra / abs(div)
    if row_live is not None:
        dead = ~np.asarray(row_live, dtype=bool)
        y_out, bound_y = y_out.copy(), bound_y.copy()
        y_out[dead], bound_y[dead] = _f64(y_before)[dead], 0.0
        if mean is not None:
            mean, bound_mean = mean.copy(), bound_mean.copy()
            mean[dead], bound_mean[dead] = _f64(mean_before)[dead], 0.0
    return y_out, mean, bound_y, bound_mean


def violations(got, want, bound, skip=None):
    """Elements that miss |got - want| <= BOUND_FACTOR * bound + ABS_FLOOR -> (count, description of the worst)."""
    got, want = _f64(got), _f64(want)
    err = np.abs(got - want)
    bad = ~(err <= BOUND_FACTOR * bound + ABS_FLOOR)          # (a NaN misses)
    if skip is not None:
        bad &= ~skip
    if not bad.any():
        return 0, ""
    over = np.where(bad, err / (BOUND_FACTOR * bound + ABS_FLOOR), 0.0)
    over = np.where(np.isnan(over), np.inf, over)
    i = np.unravel_index(int(np.argmax(over)), over.shape)
    return int(bad.sum()), f"{int(bad.sum())} elements; worst at {i}: got {got[i]!r} want {want[i]!r} allowed {BOUND_FACTOR * bound[i]:.3e}"


def sign_ambiguous(y64_unperturbed):
    """PERTURB: the elements whose sign float32 may not decide, and whether they stay under the cap."""
    amb = (np.abs(y64_unperturbed) < SIGN_AMBIGUOUS) & (y64_unperturbed != 0)
    return amb, int(amb.sum()) <= 4 + 1e-4 * amb.size


# ------------------------------------------------------------------------------------------------------------------
# ADAM
# ------------------------------------------------------------------------------------------------------------------
def adam_ref(p, m, v, g64, step, lr, b1, b2, eps):
    """torch.optim.Adam's single-tensor formula in float64 (bias corrections in double, as srh_batch_fetch documents):
    -> new p, m, v.  `step` is 1-based."""
    p, m, v, g = _f64(p), _f64(m), _f64(v), _f64(g64)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * (g * g)
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    denom = np.sqrt(v) / np.sqrt(bc2) + eps
    return p - (lr / bc1) * (m / denom), m, v


def adam_bounds(p, m, v, g64, bound_g, step, lr, b1, b2, eps):
    """What an SRH_EPI_ADAM launch may leave, given the float64 gradient and its bound (epilogue_ref's bound_y):
    dict(p, m, v: float64 results; bound_m, bound_v: per-element bounds to assert with BOUND_FACTOR -- two products and one
    add each on top of the gradient's asserted tolerance carried through (1 - b1) g and (1 - b2) g^2; p_lo, p_hi: the hull
    of adam_ref at g64 -/+ bound_g (and at g64), widened by 4 * 2^-24 * |p| + 4 * 2^-24 * |update|; update; ill: the
    elements whose hull, before widening, is wider than 1e-3 |update|)."""
    g, bg = _f64(g64), _f64(bound_g)
    p1, m1, v1 = adam_ref(p, m, v, g, step, lr, b1, b2, eps)
    tol_g = BOUND_FACTOR * bg + ABS_FLOOR
    bound_m = 3 * U32 * (np.abs(b1 * _f64(m)) + np.abs((1 - b1) * g)) + (1 - b1) * tol_g / BOUND_FACTOR
    bound_v = 3 * U32 * (b2 * _f64(v) + (1 - b2) * g * g) + (1 - b2) * (2 * np.abs(g) * tol_g + tol_g ** 2) / BOUND_FACTOR
    ends = [adam_ref(p, m, v, g + s * bg, step, lr, b1, b2, eps)[0] for s in (-1.0, 1.0)] + [p1]
    lo, hi = np.minimum.reduce(ends), np.maximum.reduce(ends)
    update = p1 - _f64(p)
    widen = 4 * U32 * np.abs(p1) + 4 * U32 * np.abs(update)
    return dict(p=p1, m=m1, v=v1, bound_m=bound_m, bound_v=bound_v, p_lo=lo - widen, p_hi=hi + widen, update=update,
                ill=(hi - lo) > 1e-3 * np.abs(update))


# ------------------------------------------------------------------------------------------------------------------
# Seeded inputs shared by the CPU checks of this file and the GPU tests
# ------------------------------------------------------------------------------------------------------------------
def row_scale_with_zeros(m, seed=4):
    """uniform(0.05, 1) with EXACT zeros on ~2 % of the rows, among them one heavy row and every empty row: the r = 0
    branch of 1 / r, and what an isolated node's D^-1/2 is."""
    rng = np.random.default_rng(seed)
    n = m.shape[0]
    lens = np.diff(m.indptr)
    r = rng.uniform(0.05, 1.0, n).astype(np.float32)
    r[lens == 0] = 0.0
    r[int(np.argmax(lens))] = 0.0
    r[rng.choice(n, size=max(1, n // 150), replace=False)] = 0.0
    return r


def epilogue_inputs(m, d, seed):
    """x ~ N(0, 1) (one zero column: exact zeros in y), two addends, SRH_MAX_PREV prev tables, U[0,1) noise, the row scale,
    and three activity masks (rows 40 %, columns 60 %, addend rows 30 % live)."""
    rng = np.random.default_rng(seed)
    n = m.shape[0]
    f = lambda *s: rng.standard_normal(s).astype(np.float32)     # noqa: E731
    x = f(n, d)
    x[:, 1] = 0.0
    col_live = rng.random(n) < 0.6
    return dict(x=x, x_cols=(x * col_live[:, None]).astype(np.float32), add=[f(n, d), f(n, d)],
                prev=[f(n, d) for _ in range(8)], noise=rng.random((n, d)).astype(np.float32),
                r=row_scale_with_zeros(m), row_live=rng.random(n) < 0.4, col_live=col_live, add_live=rng.random(n) < 0.3)


def adam_inputs(m, d, seed):
    """The state of an SRH_EPI_ADAM launch: x ~ 1e-3, addends ~ 1e-2, m0 ~ 1e-3, v0 ~ uniform(0, 1e-5) (sqrt(v_hat) within
    a few orders of eps-sized gradients: the update is ill-conditioned where it should be), and |p0| in [0.05, 0.15] so
    that the parameter's own rounding term of the hull, 4 * 2^-24 * |p|, carries the moments' roundings the hull in g does
    not.  The empty rows (> 1 % of the elements) have addends, m0 and v0 exactly zero: g = 0 exactly, update exactly 0."""
    rng = np.random.default_rng(seed)
    n = m.shape[0]
    f = lambda s: (rng.standard_normal((n, d)) * s).astype(np.float32)     # noqa: E731
    empty = np.diff(m.indptr) == 0
    add_live = rng.random(n) < 0.3
    add_live[empty] = False
    x = (rng.standard_normal((m.shape[1], d)) * 1e-3).astype(np.float32)      # (n_cols rows: the matrix may be rectangular)
    s = dict(x=x, add=[f(1e-2), f(1e-2)], m=f(1e-3), v=(rng.random((n, d)) * 1e-5).astype(np.float32),
             p=(rng.uniform(0.05, 0.15, (n, d)) * rng.choice([-1.0, 1.0], (n, d))).astype(np.float32),
             r=row_scale_with_zeros(m), add_live=add_live, empty=empty)
    for t in s["add"] + [s["m"], s["v"]]:
        t[empty] = 0.0
    return s
