"""Parity of every HIP kernel against the CPU oracle / the reference-generated golden vectors.
All calls go through the C ABI (selfrec_amd.ops -> ctypes -> libselfrec_hip.so).

Tolerances: integer / index outputs bit-exact; fp32 values within 1e-4 relative (the bound
BASELINE.json's north_star states), most checks far tighter.
"""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from oracle import selfrec_oracle as O
from selfrec_amd import ops

from . import spmm_ref as R
from .counter_rng import counter_noise

pytestmark = pytest.mark.gpu
DEV = "cuda"


def rel_err(got, want, floor=1e-7):
    """max |got - want| relative to the largest reference magnitude (floored: an all-zero
    reference, e.g. the InfoNCE gradient at n=1, is compared absolutely)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), floor))


def powerlaw_csr(n_rows, n_cols, nnz, seed, heavy_rows=0, heavy_len=0, empty_rows=0):
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, n_rows + 1) ** 0.8
    rows = rng.choice(n_rows, size=nnz, p=w / w.sum())
    cols = rng.integers(0, n_cols, size=nnz)
    for h in range(heavy_rows):
        extra = rng.choice(n_cols, size=min(heavy_len, n_cols), replace=False)
        rows = np.concatenate([rows, np.full(extra.size, n_rows - 1 - h)])
        cols = np.concatenate([cols, extra])
    vals = rng.standard_normal(rows.size).astype(np.float32)
    m = sp.csr_matrix((vals, (rows, cols)), shape=(n_rows, n_cols), dtype=np.float32)
    if empty_rows:
        lil = m.tolil()
        for r in rng.choice(n_rows, size=empty_rows, replace=False):
            lil.rows[r], lil.data[r] = [], []
        m = lil.tocsr()
    m.sum_duplicates()
    m.sort_indices()
    return m


# ------------------------------------------------------------------------------------------
# (a-3/a-4) SpMM and its epilogues
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [32, 64, 128, 256])
@pytest.mark.parametrize("shape", [(1, 1, 1, 0, 0, 0), (97, 130, 700, 0, 0, 5), (3000, 2500, 40000, 3, 1500, 40)])
def test_spmm_matches_scipy(d, shape):
    n_rows, n_cols, nnz, heavy, heavy_len, empty = shape
    m = powerlaw_csr(n_rows, n_cols, nnz, seed=d + n_rows, heavy_rows=heavy, heavy_len=heavy_len, empty_rows=empty)
    x = np.random.default_rng(1).standard_normal((n_cols, d)).astype(np.float32)
    want = (m.astype(np.float64) @ x.astype(np.float64))
    csr = ops.DeviceCSR.from_scipy(m)
    got = ops.spmm(csr, torch.from_numpy(x).to(DEV)).cpu().numpy()
    assert got.shape == want.shape
    assert rel_err(got, want) < 2e-6
    if heavy:   # split rows: explicit small split length exercises the partial-sum path harder
        csr2 = ops.DeviceCSR.from_scipy(m, split_len=64)
        got2 = ops.spmm(csr2, torch.from_numpy(x).to(DEV)).cpu().numpy()
        assert rel_err(got2, want) < 2e-6
        # fixed reduction order: bitwise reproducible
        assert np.array_equal(got2, ops.spmm(csr2, torch.from_numpy(x).to(DEV)).cpu().numpy())


def test_spmm_epilogues_match_oracle():
    d, n = 64, 1200
    m = powerlaw_csr(n, n, 20000, seed=3, heavy_rows=2, heavy_len=900, empty_rows=10)
    rng = np.random.default_rng(5)
    x = rng.standard_normal((n, d)).astype(np.float32)
    x[:, :3] = 0.0                                        # exact zeros in y -> sign(0) = 0 branch
    noise = rng.random((n, d)).astype(np.float32)
    p0, p1 = rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((n, d)).astype(np.float32)
    csr = ops.DeviceCSR.from_scipy(m)
    tx, tn = torch.from_numpy(x).to(DEV), torch.from_numpy(noise).to(DEV)
    tp0, tp1 = torch.from_numpy(p0).to(DEV), torch.from_numpy(p1).to(DEV)
    # oracle: XSimGCL.py:88-96 on CPU
    y = torch.sparse.mm(O.to_torch_sparse(m), torch.from_numpy(x))
    y = O.perturb_(y, torch.from_numpy(noise), 0.2)
    mean = torch.mean(torch.stack([torch.from_numpy(p0), torch.from_numpy(p1), y], dim=1), dim=1)
    mean_out = torch.empty((n, d), device=DEV)
    ep = ops.make_epilogue(perturb_eps=0.2, noise=tn, prev=[tp0, tp1], mean_div=3.0, mean_out=mean_out)
    got = ops.spmm(csr, tx, epilogue=ep)
    assert rel_err(got.cpu().numpy(), y.numpy()) < 2e-6
    assert rel_err(mean_out.cpu().numpy(), mean.numpy()) < 2e-6
    # backward-style AXPY with alpha, addend aliasing the output
    out = tp0.clone()
    ep = ops.make_epilogue(add=[out, tp1], add_scale=[1.0, 0.25], alpha=0.5)
    ops.spmm(csr, tx, out=out, epilogue=ep)
    want = 0.5 * (m.astype(np.float64) @ x.astype(np.float64)) + p0 + 0.25 * p1
    assert rel_err(out.cpu().numpy(), want) < 2e-6


@pytest.mark.selfcheck
def test_spmm_fanout_equals_separate_launches():
    """One product, three outputs (SimGCL's clean pass + two perturbed views share A.E0 in layer 1): each
    output is bit-identical to a launch of its own, with injected noise and with the counter RNG."""
    d, n = 64, 900
    m = powerlaw_csr(n, n, 15000, seed=21, heavy_rows=2, heavy_len=800, empty_rows=4)
    rng = np.random.default_rng(8)
    x = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)).to(DEV)
    na, nb = (torch.from_numpy(rng.random((n, d)).astype(np.float32)).to(DEV) for _ in range(2))
    csr = ops.DeviceCSR.from_scipy(m)
    clean = ops.spmm(csr, x)
    for injected in (True, False):
        kw = dict(perturb_eps=0.2, rng_seed=77, rng_stride=n * 16)
        if injected:
            sep = [ops.spmm(csr, x, epilogue=ops.make_epilogue(noise=t, **kw)) for t in (na, nb)]
            extra = dict(extra_noise=[na, nb])
        else:
            sep = [ops.spmm(csr, x, epilogue=ops.make_epilogue(rng_offset=off, **kw)) for off in (5 * n, 9 * n)]
            extra = dict(extra_rng_offset=[5 * n, 9 * n])
        ya, yb, y = torch.empty_like(clean), torch.empty_like(clean), torch.empty_like(clean)
        ops.spmm(csr, x, out=y, epilogue=ops.make_epilogue(main_clean=True, extra_out=[ya, yb], **extra, **kw))
        assert torch.equal(y, clean) and torch.equal(ya, sep[0]) and torch.equal(yb, sep[1])
        assert not torch.equal(ya, yb)


@pytest.mark.selfcheck
def test_spmm3_equals_three_launches():
    """Three value arrays over one structure, one traversal (SGL's first layer): bit-identical to three
    launches, split rows and dropped (zero) entries included; other widths are refused."""
    d, n = 64, 1100
    m = powerlaw_csr(n, n, 18000, seed=23, heavy_rows=3, heavy_len=900, empty_rows=6)
    rng = np.random.default_rng(6)
    x = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)).to(DEV)
    base = ops.DeviceCSR.from_scipy(m)
    views = [base]
    for _ in range(2):
        keep = torch.from_numpy((rng.random(m.nnz) > 0.3).astype(np.float32)).to(DEV)
        views.append(base.with_values(base.vals * keep * float(rng.uniform(0.5, 2.0))))
    want = [ops.spmm(v, x) for v in views]
    outs = [torch.full((n, d), 3.0, device=DEV) for _ in range(3)]
    ops.spmm3(views, x, outs)
    for got, ref in zip(outs, want):
        assert torch.equal(got, ref)
    with pytest.raises(ops.SelfrecHipError):
        x128 = torch.zeros((n, 128), device=DEV)
        ops.spmm3(views, x128, [torch.empty((n, 128), device=DEV) for _ in range(3)])


@pytest.mark.parametrize("d", [64, 128])
def test_spmm_xcd_shares_and_probe(d):
    """srh_spmm_plan_set_xcd_shares / srh_spmm_f32_probe: unequal numbers of workgroups per XCD (empty records pad the
    list) change where tasks run, never what they compute -- same product bit for bit, also with split heavy rows, the
    pattern form and row marks -- and the probe launch computes the product too and stamps every task once."""
    n, U = 3000, 1200
    m = powerlaw_csr(n, n, 60000, seed=37, heavy_rows=4, heavy_len=1800, empty_rows=11)
    perm, row_mid = ops.column_class_order(m.indptr, m.indices, 64)
    csr = ops.DeviceCSR(m.indptr, m.indices[perm], m.data[perm], m.shape, xcd_split_row=U, row_mid=row_mid)
    rng = np.random.default_rng(8)
    tx = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)).to(DEV)
    mark = torch.from_numpy(np.where(rng.random(n) < 0.2, 7, 1).astype(np.int32)).to(DEV)
    stamp = torch.tensor([7], dtype=torch.int64, device=DEV)
    ep_rows = lambda: ops.make_epilogue(row_mark=mark, mark_stamp=stamp)          # noqa: E731
    ep_cols = lambda: ops.make_epilogue(col_mark=mark, mark_stamp=stamp)          # noqa: E731
    ref, ref_pat = ops.spmm(csr, tx), ops.spmm(csr, tx, pattern=True)
    ref_cols = ops.spmm(csr, tx, epilogue=ep_cols())
    ref_rows = torch.zeros((n, d), device=DEV); ops.spmm(csr, tx, out=ref_rows, epilogue=ep_rows())
    # the row-masked launch (d = 64: its own instantiation, the next chunk's indices issued AFTER the gathers from inline
    # asm) adds the same entries in the same order as the unmasked kernel: identical bits on the marked rows, with a value
    # stream and as a pattern launch; unmarked rows are not touched
    live = mark == 7
    assert torch.equal(ref_rows[live], ref[live]) and not ref_rows[~live].any()
    pat_rows = torch.zeros((n, d), device=DEV); ops.spmm(csr, tx, out=pat_rows, epilogue=ep_rows(), pattern=True)
    assert torch.equal(pat_rows[live], ref_pat[live]) and not pat_rows[~live].any()
    n_canon = ops.spmm_plan_run_tasks(csr, d)
    nb = (n_canon + 3) // 4
    canon = np.array([len(range(k, nb, 8)) for k in range(8)])
    a, b, few = int(canon.min()) // 2, int(canon.min()) // 3, max(1, int(canon.min()) // 4)
    for shares in (canon, canon + np.array([a, -a, b, -b, 0, 0, 1, -1]), np.array([nb - 7 * few] + [few] * 7)):
        ops.spmm_set_xcd_shares(csr, d, shares)
        assert ops.spmm_plan_run_tasks(csr, d) == int(shares.max()) * 32
        assert torch.equal(ops.spmm(csr, tx), ref) and torch.equal(ops.spmm(csr, tx, pattern=True), ref_pat)
        assert torch.equal(ops.spmm(csr, tx, epilogue=ep_cols()), ref_cols)
        out = torch.zeros((n, d), device=DEV); ops.spmm(csr, tx, out=out, epilogue=ep_rows())
        assert torch.equal(out, ref_rows)
        got = torch.empty((n, d), device=DEV)
        finish, begin, end, xcd = ops.spmm_probe(csr, tx, got)
        assert torch.equal(got, ref)
        assert begin.size == int(shares.max()) * 32 and (end >= begin).all() and set(np.unique(xcd)) <= set(range(8))
        assert finish.shape == (8,) and finish.max() < 1e4                         # us: a sane clock
    with pytest.raises(ops.SelfrecHipError):
        ops.spmm_set_xcd_shares(csr, d, canon + 1)                                 # does not add up
    ops.spmm_set_xcd_shares(csr, d, None)
    assert ops.spmm_plan_run_tasks(csr, d) == n_canon and torch.equal(ops.spmm(csr, tx), ref)
    # srh_spmm_gather_bound: the same schedule and gathers with nothing after them -- runs, touches no operand, and (a strict
    # subset of the product's work) is not slower than the product beyond timer noise on this small graph
    before = tx.clone()
    bound_us = ops.spmm_gather_bound(csr, tx, iters=20)
    assert 0.0 < bound_us < 1e4 and torch.equal(tx, before) and torch.equal(ops.spmm(csr, tx), ref)


@pytest.mark.parametrize("d", [64, 128])
def test_spmm_under_another_plan_of_the_same_arrays(d):
    """DeviceCSR.replanned: the same device arrays under a second schedule (the engine runs the column-masked launch of a
    step on a class-free plan with shorter segments): same product in every flavour -- plain, pattern (no value stream),
    row-masked, column-masked -- split heavy rows included, and the two objects share indices and values."""
    n, U = 2600, 1000
    m = powerlaw_csr(n, n, 52000, seed=31, heavy_rows=4, heavy_len=1700, empty_rows=9)
    perm, row_mid = ops.column_class_order(m.indptr, m.indices, 64)
    base = ops.DeviceCSR(m.indptr, m.indices[perm], m.data[perm], m.shape, xcd_split_row=U, row_mid=row_mid)
    rng = np.random.default_rng(4)
    x = rng.standard_normal((n, d)).astype(np.float32)
    tx = torch.from_numpy(x).to(DEV)
    want = m.astype(np.float64) @ x.astype(np.float64)
    ones = sp.csr_matrix((np.ones_like(m.data), m.indices, m.indptr), shape=m.shape)
    want_pattern = ones.astype(np.float64) @ x.astype(np.float64)
    live = rng.random(n) < 0.25
    mark = torch.from_numpy(np.where(live, 7, 3).astype(np.int32)).to(DEV)
    stamp = torch.tensor([7], dtype=torch.int64, device=DEV)
    xz = x.copy(); xz[~live] = 0.0
    want_cols = m.astype(np.float64) @ xz.astype(np.float64)
    for split, split_row in ((256, 0), (128, 0), (512, U)):
        other = base.replanned(split_len=split, xcd_split_row=split_row)
        assert other.indices.data_ptr() == base.indices.data_ptr() and other.vals.data_ptr() == base.vals.data_ptr()
        assert rel_err(ops.spmm(other, tx).cpu().numpy(), want) < 2e-6
        assert rel_err(ops.spmm(other, tx, pattern=True).cpu().numpy(), want_pattern) < 2e-6
        got = ops.spmm(other, tx, epilogue=ops.make_epilogue(col_mark=mark, mark_stamp=stamp))
        assert rel_err(got.cpu().numpy(), want_cols) < 2e-6
        out = torch.full((n, d), -5.0, device=DEV)
        ops.spmm(other, tx, out=out, epilogue=ops.make_epilogue(row_mark=mark, mark_stamp=stamp))
        out = out.cpu().numpy()
        assert rel_err(out[live], want[live]) < 2e-6 and (out[~live] == -5.0).all()
        assert torch.equal(ops.spmm(other, tx), ops.spmm(other, tx))          # fixed reduction order
    del other
    assert rel_err(ops.spmm(base, tx).cpu().numpy(), want) < 2e-6            # the first plan is untouched


@pytest.mark.parametrize("d,min_len", [(64, 64), (64, 8), (128, 16), (32, 16)])
def test_spmm_with_column_class_schedule_matches_scipy(d, min_len):
    """Rows of >= min_len non-zeros stored [even columns | odd columns] and scheduled as two segments on
    different XCDs (srh_spmm_plan_create h_row_mid): same product, split heavy rows and masks included."""
    n, U = 1300, 500
    m = powerlaw_csr(n, n, 26000, seed=17, heavy_rows=3, heavy_len=1100, empty_rows=7)
    perm, row_mid = ops.column_class_order(m.indptr, m.indices, min_len)
    assert sorted(perm.tolist()) == list(range(m.nnz)) and (row_mid >= 0).sum() == (np.diff(m.indptr) >= min_len).sum()
    csr = ops.DeviceCSR(m.indptr, m.indices[perm], m.data[perm], m.shape, xcd_split_row=U, row_mid=row_mid)
    rng = np.random.default_rng(3)
    x = rng.standard_normal((n, d)).astype(np.float32)
    tx = torch.from_numpy(x).to(DEV)
    want = m.astype(np.float64) @ x.astype(np.float64)
    got = ops.spmm(csr, tx)
    assert rel_err(got.cpu().numpy(), want) < 2e-6
    assert torch.equal(ops.spmm(csr, tx), got)                      # reproducible bit for bit
    # column marks: only the live columns contribute
    live = rng.random(n) < 0.3
    mark = torch.from_numpy(np.where(live, 5, 0).astype(np.int32)).to(DEV)
    stamp = torch.tensor([5], dtype=torch.int64, device=DEV)
    xm = tx * torch.from_numpy(live.astype(np.float32)).to(DEV).unsqueeze(1)
    got_m = ops.spmm(csr, xm, epilogue=ops.make_epilogue(col_mark=mark, mark_stamp=stamp))
    want_m = m.astype(np.float64) @ (x * live[:, None]).astype(np.float64)
    assert rel_err(got_m.cpu().numpy(), want_m) < 2e-6


def test_spmm_rng_perturbation_properties():
    d, n = 64, 500
    m = powerlaw_csr(n, n, 6000, seed=9)
    x = np.random.default_rng(2).standard_normal((n, d)).astype(np.float32)
    csr = ops.DeviceCSR.from_scipy(m)
    tx = torch.from_numpy(x).to(DEV)
    base = ops.spmm(csr, tx)
    a = ops.spmm(csr, tx, epilogue=ops.make_epilogue(perturb_eps=0.2, rng_seed=7, rng_offset=0))
    b = ops.spmm(csr, tx, epilogue=ops.make_epilogue(perturb_eps=0.2, rng_seed=7, rng_offset=0))
    c = ops.spmm(csr, tx, epilogue=ops.make_epilogue(perturb_eps=0.2, rng_seed=7, rng_offset=n))
    assert torch.equal(a, b) and not torch.equal(a, c)          # counter-based: reproducible, offset-dependent
    delta = (a - base).cpu().numpy()
    nz = np.abs(base.cpu().numpy()).sum(1) > 0
    # each perturbed row moved by a vector of norm eps along sign(y) (XSimGCL.py:91)
    assert np.allclose(np.linalg.norm(delta[nz], axis=1), 0.2, rtol=1e-4)
    assert np.all(delta * np.sign(base.cpu().numpy()) >= -1e-7)
    step = torch.tensor([3], dtype=torch.int64, device=DEV)
    e = ops.spmm(csr, tx, epilogue=ops.make_epilogue(perturb_eps=0.2, rng_seed=7, rng_offset=0,
                                                     rng_step=step, rng_stride=n))
    f = ops.spmm(csr, tx, epilogue=ops.make_epilogue(perturb_eps=0.2, rng_seed=7, rng_offset=3 * n))
    assert torch.equal(e, f)


# ---- the in-kernel counter noise, number for number (tests/counter_rng.py restates the mixer on the host)
RNG_SEED = 0xA5C3_0F17_5E1F_0EC9          # a high word that is not zero
RNG_EPS = 0.2


def _counter_modes(n):
    """(name, rng_offset, device step, stride, n_extra, main_clean, row-masked) of the launches every case runs"""
    stride = 16 * n
    near62 = ((1 << 62) - 3 * stride) // stride            # step * stride crosses 2^32 and sits just under 2^62
    return [("plain", 0, None, 0, 0, False, False),
            ("offset_crosses_2^32", (1 << 32) - n // 2, None, 0, 0, False, False),
            ("device_step_near_2^62", 5 * n + 3, near62, stride, 0, False, False),
            ("fanout_main_perturbed", (1 << 32) - 7, 3, stride, 2, False, False),
            ("fanout_main_clean", 11, near62 + 1, stride, 2, True, False),
            ("row_masked", 2 * n, 9, stride, 0, False, True)]


def _check_counter_launch(csr, m64, x, d_full, col0, d_valid, *, pattern=False, row_scale=None, tol=2e-6):
    """Each counter mode: the counter launch == the launch with the restated noise injected (bit for bit on the rows /
    slice kernels, 2e-6 relative on the pair kernel: its injected path sums the norm in another order), both within tol
    of float64 y + sign(y) eps u / ||u|| (u: the restatement, norm over the whole row's valid columns), padding exactly 0,
    unmarked rows untouched."""
    n, d = m64.shape[0], x.shape[1]
    dv = d_full if d_valid is None else d_valid
    tx = torch.from_numpy(x).to(DEV)
    y64 = m64 @ x.astype(np.float64)
    if row_scale is not None:
        y64 = y64 * row_scale.astype(np.float64)[:, None]
    slice_kw = dict(d_full=d_full, col0=col0) if d_full != d else {}
    if d_valid is not None:
        slice_kw["d_valid"] = d_valid
    scale_kw = dict(row_scale=torch.from_numpy(row_scale).to(DEV), scale_in=True) if row_scale is not None else {}
    exact = d != 8
    for name, off, step, stride, n_extra, main_clean, masked in _counter_modes(n):
        extra_off = [off + (k + 1) * n for k in range(n_extra)]
        step_t = torch.tensor([step], dtype=torch.int64, device=DEV) if step is not None else None
        mark_kw, live = {}, np.ones(n, dtype=bool)
        if masked:
            live = np.random.default_rng(n + d).random(n) < 0.4
            mark = torch.from_numpy(np.where(live, 17, 16).astype(np.int32)).to(DEV)
            mark_kw = dict(row_mark=mark, mark_stamp=torch.tensor([17], dtype=torch.int64, device=DEV))

        def restated(o):
            c0 = (o + (step or 0) * stride) & 0xFFFFFFFFFFFFFFFF
            return counter_noise(RNG_SEED, c0, n, d_full, d_valid)

        noises = [restated(o) for o in [off] + extra_off]
        runs = []
        for inject in (False, True):
            outs = [torch.full((n, d), 7.0, device=DEV) for _ in range(1 + n_extra)]
            kw = dict(perturb_eps=RNG_EPS, rng_seed=RNG_SEED, rng_offset=off, rng_step=step_t, rng_stride=stride)
            if inject:
                # (injected noise is whole rows: (n, d_full) under a slice, (n, d) otherwise; the counter fields are ignored)
                kw.update(noise=torch.from_numpy(noises[0]).to(DEV), rng_step=None)
            if n_extra:
                kw.update(extra_out=outs[1:], extra_rng_offset=extra_off, main_clean=main_clean,
                          extra_noise=[torch.from_numpy(z).to(DEV) for z in noises[1:]] if inject else None)
            ops.spmm(csr, tx, out=outs[0], pattern=pattern,
                     epilogue=ops.make_epilogue(**kw, **slice_kw, **scale_kw, **mark_kw))
            runs.append([o.cpu().numpy() for o in outs])
        for k, (got, inj) in enumerate(zip(*runs)):
            what = f"{name} output {k} (d={d} of {d_full}, col0={col0}, d_valid={d_valid})"
            if exact:
                assert np.array_equal(got, inj), what
            else:
                assert rel_err(got, inj) < 2e-6, what
            clean = k == 0 and main_clean
            u = noises[0 if clean else k].astype(np.float64)
            pert = np.sign(y64) * RNG_EPS * (u / np.linalg.norm(u, axis=1, keepdims=True))[:, col0:col0 + d]
            want = y64 if clean else y64 + pert
            assert np.all(got[~live] == 7.0) and np.all(inj[~live] == 7.0), what        # unmarked rows left alone
            ambiguous = (np.abs(y64) < 1e-6) & (y64 != 0)                               # sign(y) not decided in fp32
            assert ambiguous.sum() <= 4 + 1e-4 * ambiguous.size, what
            sel = live[:, None] & ~ambiguous
            for t in (got, inj):
                assert np.abs(t - want)[sel].max() <= tol * np.abs(want).max(), what
                assert np.all(t[live][y64[live] == 0] == 0), what                      # sign(0) = 0: no move
            if d_valid is not None and col0 + d > d_valid:
                assert np.all(got[live][:, max(d_valid - col0, 0):] == 0), what          # padding columns stay exactly 0


def _counter_graph(n_rows=3000, n_cols=2500):
    m = powerlaw_csr(n_rows, n_cols, 40000, seed=23, heavy_rows=3, heavy_len=1500, empty_rows=40)
    # split_len = 64: the heavy rows finish through the coop / partial-sum path
    return m, m.astype(np.float64), ops.DeviceCSR.from_scipy(m, split_len=64)


def _counter_x(n_cols, d, col0, d_valid, seed):
    x = np.random.default_rng(seed).standard_normal((n_cols, d)).astype(np.float32)
    x[:, 1] = 0.0                                            # exact zeros in y: the sign(0) branch
    if d_valid is not None:
        x[:, max(d_valid - col0, 0):] = 0.0                  # the padding columns of the whole row are zero
    return x


def _spmm_path(d):
    return "pair" if d == 8 else "slice" if d <= 32 else "rows"


# (slice width d, whole-row width d_full, d_valid or None): whole rows, column slices, zero-padded rows, padded slices
COUNTER_CASES = [(64, 64, None), (128, 128, None), (256, 256, None), (32, 32, None),
                 (16, 64, None), (32, 64, None), (32, 128, None), (64, 128, None), (64, 256, None), (128, 256, None),
                 (8, 32, None), (8, 64, None),
                 (64, 64, 50), (128, 128, 100), (256, 256, 200),
                 (64, 128, 100), (128, 256, 200)]


@pytest.mark.parametrize("d,d_full,d_valid", COUNTER_CASES,
                         ids=[f"{_spmm_path(c[0])}-{c[0]}of{c[1]}" + (f"-valid{c[2]}" if c[2] else "") for c in COUNTER_CASES])
def test_spmm_counter_noise_equals_host_restatement(d, d_full, d_valid):
    """Which numbers the epilogue's counter RNG draws (spmm_rows_kernel d = 64 / 128 / 256, spmm_slice_kernel d = 16 / 32,
    spmm_pair_kernel d = 8 through thin_perturb), at every col0 of the slice, against tests/counter_rng.py: a seed with a
    high word, a counter offset crossing 2^32 inside the launch, a device step whose step * stride sits near 2^62, FANOUT
    with two extra offsets (main output perturbed and clean), a row-masked launch."""
    m, m64, csr = _counter_graph()
    for col0 in range(0, d_full, d):
        x = _counter_x(m.shape[1], d, col0, d_valid, seed=col0 + d)
        _check_counter_launch(csr, m64, x, d_full, col0, d_valid)


@pytest.mark.parametrize("d,d_full,d_valid", [(64, 64, None), (128, 128, 100), (64, 128, None)])
def test_spmm_counter_noise_value_free_row_scaled(d, d_full, d_valid):
    """The value-free product (pattern=True, row scale applied before the perturbation) draws the same numbers."""
    m, _, csr = _counter_graph()
    pat = m.copy()
    pat.data[:] = 1.0
    scale = np.random.default_rng(4).uniform(0.05, 1.0, m.shape[0]).astype(np.float32)
    for col0 in range(0, d_full, d):
        x = _counter_x(m.shape[1], d, col0, d_valid, seed=col0 + 3)
        _check_counter_launch(csr, pat.astype(np.float64), x, d_full, col0, d_valid, pattern=True, row_scale=scale)


def test_spmm_counter_noise_under_graph_replay_follows_the_device_step():
    """One SpMM launch captured with the rng_step pointer: replays after writing steps 1, 2, 3 draw the restatement's
    numbers of that step (the launch has no parallel branches)."""
    m, m64, csr = _counter_graph()
    n, d = m.shape[0], 64
    x = _counter_x(m.shape[1], d, 0, None, seed=1)
    tx = torch.from_numpy(x).to(DEV)
    out = torch.zeros((n, d), device=DEV)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    off, stride = 3 * n, 16 * n
    ep = ops.make_epilogue(perturb_eps=RNG_EPS, rng_seed=RNG_SEED, rng_offset=off, rng_step=step, rng_stride=stride)
    ops.spmm(csr, tx, out=out, epilogue=ep)                    # warm-up (module load) outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.spmm(csr, tx, out=out, epilogue=ep)
    seen = []
    for s in (1, 2, 3):
        step.fill_(s)
        g.replay()
        torch.cuda.synchronize()
        z = torch.from_numpy(counter_noise(RNG_SEED, off + s * stride, n, d)).to(DEV)
        want = ops.spmm(csr, tx, epilogue=ops.make_epilogue(perturb_eps=RNG_EPS, noise=z))
        got = out.clone()
        assert torch.equal(got, want), s
        seen.append(got)
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


def test_value_free_product_with_row_scaling(tiny_data):
    """srh_spmm_f32 with d_vals == NULL (pattern) + SRH_SCALE_IN / SRH_SCALE_OUT / prev-unscale / addend row scale:
    D^-1/2 A D^-1/2 x without the value stream (graph.py:10-24), as the engine chains it through pre-scaled tables."""
    g = tiny_data.device_graph()
    N, d = g.n_nodes, 64
    rng = np.random.default_rng(5)
    x = rng.standard_normal((N, d)).astype(np.float32)
    a = rng.standard_normal((N, d)).astype(np.float32)
    p0 = rng.standard_normal((N, d)).astype(np.float32)
    A = sp.csr_matrix((g.adj.vals.cpu().numpy(), g.adj.indices.cpu().numpy(), g.adj.indptr.cpu().numpy()), shape=(N, N)).astype(np.float64)
    dinv = g.dinv.cpu().numpy().astype(np.float64)
    want = A @ x.astype(np.float64)                                            # true product
    xs = torch.from_numpy((dinv[:, None] * x).astype(np.float32)).to(DEV)      # the pre-scaled input table
    y = torch.empty((N, d), device=DEV)
    ops.spmm(g.adj, xs, out=y, epilogue=ops.make_epilogue(row_scale=g.dinv, scale_in=True), pattern=True)
    assert rel_err(y.cpu().numpy(), want) < 2e-6
    # stored pre-scaled for the next layer, plus an addend that enters times d_i^-1/2 and one that does not
    ta = torch.from_numpy(a).to(DEV)
    ops.spmm(g.adj, xs, out=y, pattern=True,
             epilogue=ops.make_epilogue(row_scale=g.dinv, scale_in=True, scale_out=True, add=[ta, ta], add_scale=[0.5, 2.0],
                                        alpha=0.25, add_rowscale=[True, False]))
    want2 = dinv[:, None] * (0.25 * want + 0.5 * dinv[:, None] * a + 2.0 * a)
    assert rel_err(y.cpu().numpy(), want2) < 3e-6
    # last layer: mean over a true table, a pre-scaled table and this product
    tp = torch.from_numpy(p0).to(DEV)
    tps = torch.from_numpy((dinv[:, None] * p0).astype(np.float32)).to(DEV)
    mean = torch.empty((N, d), device=DEV)
    ops.spmm(g.adj, xs, out=y, pattern=True,
             epilogue=ops.make_epilogue(row_scale=g.dinv, scale_in=True, prev=[tp, tps], mean_div=3.0, mean_out=mean,
                                        prev_unscale=[False, True]))
    live = dinv > 0
    assert rel_err(mean.cpu().numpy()[live], ((p0 + p0 + want) / 3.0)[live]) < 3e-6
    # the value array path with the same scaling flags (first product of a chain: true input, pre-scaled output)
    tx = torch.from_numpy(x).to(DEV)
    ops.spmm(g.adj, tx, out=y, epilogue=ops.make_epilogue(row_scale=g.dinv, scale_out=True))
    assert rel_err(y.cpu().numpy(), dinv[:, None] * want) < 2e-6


# ---- every epilogue feature, at every width, against the float64 restatement of the header (tests/spmm_ref.py) ----
# Tolerances are the restatement's per-element bounds (derived there, not measured): a three-entry row is held hundreds of
# times tighter than a heavy row.  Every launch runs twice and must repeat bit for bit (fixed reduction order).
EPI_STAMP = 17
EPI_STAMP_BIG = (1 << 33) + 17          # > 2^31: a mark is live iff mark == (int32) stamp
EPI_EPS = 0.2
_U8 = [True] * 8


def _bit(t, n=8):
    return [k == t for k in range(n)]


_AX = dict(alpha=0.25, n_add=2, add_scale=[0.5, 2.0])
# (name, what the launch carries).  pattern: d_vals = NULL; n_prev / mean_div: MEAN; alpha / n_add / add_scale: AXPY; alias0:
# addend 0 is the output; row_mark / col_mark / add_sparse: activity marks (add_sparse needs d_add_mark); stamp: *d_mark_stamp
EPI_CASES = [
    ("mean-prev0", dict(n_prev=0, mean_div=1.0)),
    ("mean-prev1", dict(n_prev=1, mean_div=2.0)),
    ("mean-prev3", dict(n_prev=3, mean_div=4.0)),
    ("mean-prev8", dict(n_prev=8, mean_div=9.0)),
    ("mean-prev3-div2.5", dict(n_prev=3, mean_div=2.5)),
    ("mean-prev0-perturb", dict(n_prev=0, mean_div=1.0, perturb=True)),
    ("mean-prev3-perturb", dict(n_prev=3, mean_div=4.0, perturb=True)),
    ("mean-prev8-perturb-div2.5", dict(n_prev=8, mean_div=2.5, perturb=True)),
    ("axpy-alpha-only", dict(alpha=0.25, n_add=0)),
    ("axpy-add1", dict(alpha=0.5, n_add=1, add_scale=[0.3])),
    ("axpy-add2", dict(alpha=0.5, n_add=2, add_scale=[0.3, -2.0])),
    ("axpy-add0-aliases-out", dict(alpha=0.5, n_add=2, add_scale=[1.0, 0.25], alias0=True)),
    ("axpy-alpha1-addends", dict(alpha=1.0, n_add=2, add_scale=[0.5, 2.0])),
    ("scale-in-pattern", dict(pattern=True, scale_in=True)),
    ("scale-in-values", dict(scale_in=True)),
    ("scale-out", dict(scale_out=True)),
    ("scale-in-out-pattern", dict(pattern=True, scale_in=True, scale_out=True)),
    ("scale-in-out-values", dict(scale_in=True, scale_out=True)),
    ("add-rowscale-01", dict(scale_in=True, add_rowscale=[True, False], **_AX)),
    ("add-rowscale-10", dict(pattern=True, scale_in=True, add_rowscale=[False, True], **_AX)),
    ("add-rowscale-11-scale-out", dict(scale_in=True, scale_out=True, add_rowscale=[True, True], **_AX)),
    ("add-rowscale-01-no-scale-flags", dict(add_rowscale=[True, False], **_AX)),
    ("prev-unscale-bit0", dict(pattern=True, scale_in=True, n_prev=8, mean_div=9.0, prev_unscale=_bit(0))),
    ("prev-unscale-bit1", dict(pattern=True, scale_in=True, n_prev=8, mean_div=9.0, prev_unscale=_bit(1))),
    ("prev-unscale-bit7", dict(scale_in=True, n_prev=8, mean_div=9.0, prev_unscale=_bit(7))),
    ("prev-unscale-all", dict(pattern=True, scale_in=True, n_prev=8, mean_div=9.0, prev_unscale=_U8)),
    ("prev-unscale-101-of-3", dict(pattern=True, scale_in=True, n_prev=3, mean_div=4.0, prev_unscale=[True, False, True])),
    ("mean-scale-out", dict(pattern=True, scale_in=True, scale_out=True, n_prev=3, mean_div=4.0, prev_unscale=[True, False, True])),
    ("mean-scale-out-values-axpy", dict(scale_out=True, n_prev=1, mean_div=2.0, prev_unscale=[True], add_rowscale=[False, True], **_AX)),
    ("rowmark-mean", dict(row_mark=True, n_prev=3, mean_div=4.0)),
    ("rowmark-mean-scaled-perturb", dict(row_mark=True, pattern=True, scale_in=True, scale_out=True, n_prev=3, mean_div=4.0,
                                         prev_unscale=[True, True, False], perturb=True)),
    ("rowmark-stamp>2^31", dict(row_mark=True, n_prev=1, mean_div=2.0, stamp=EPI_STAMP_BIG)),
    ("colmark", dict(col_mark=True)),
    ("colmark-rowmark-mean-scaled", dict(col_mark=True, row_mark=True, scale_in=True, n_prev=3, mean_div=4.0,
                                         prev_unscale=[False, True, False])),
    ("colmark-stamp>2^31", dict(col_mark=True, stamp=EPI_STAMP_BIG, **_AX)),
    ("addmark-sparse-01", dict(add_sparse=[True, False], **_AX)),
    ("addmark-sparse-10", dict(add_sparse=[False, True], **_AX)),
    ("addmark-sparse-11", dict(add_sparse=[True, True], **_AX)),
    ("addmark-sparse-11-rowscale-stamp>2^31", dict(pattern=True, scale_in=True, scale_out=True, add_sparse=[True, True],
                                                  add_rowscale=[False, True], stamp=EPI_STAMP_BIG, **_AX)),
    ("addmark-sparse-10-rowmark", dict(add_sparse=[False, True], row_mark=True, **_AX)),
]
# d = 8 / 16 / 32 (the thin kernels): what the header allows there -- no row scaling, no pattern, no ADAM
THIN_CASES = [c for c in EPI_CASES if c[0] in ("mean-prev0", "mean-prev3", "mean-prev8", "mean-prev3-perturb", "axpy-alpha-only",
                                               "axpy-add1", "axpy-add0-aliases-out", "rowmark-mean", "rowmark-stamp>2^31", "colmark",
                                               "colmark-stamp>2^31", "addmark-sparse-01", "addmark-sparse-10", "addmark-sparse-11",
                                               "addmark-sparse-10-rowmark")]


def _t32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _mark32(live):
    """live rows carry (int32) stamp = 17; the dead ones a mix of other values, 0 and 17 + 2^16 among them"""
    dead = np.array([16, 0, 17 + (1 << 16), -17], dtype=np.int32)[np.arange(live.size) % 4]
    return torch.from_numpy(np.where(live, np.int32(17), dead).astype(np.int32)).to(DEV)


def _epi_env(d, split_len):
    m = powerlaw_csr(3000, 3000, 40000, seed=23, heavy_rows=3, heavy_len=1500, empty_rows=40)
    s = R.epilogue_inputs(m, d, seed=d)
    heavy = np.argsort(np.diff(m.indptr))[-3:]
    assert (s["r"] == 0).sum() >= 60 and (s["r"][heavy] == 0).sum() >= 1 and np.all(s["r"][np.diff(m.indptr) == 0] == 0)
    dev = {k: _t32(s[k]) for k in ("x", "x_cols", "noise", "r")}
    dev.update(add=[_t32(a) for a in s["add"]], prev=[_t32(p) for p in s["prev"]],
               row_mark=_mark32(s["row_live"]), col_mark=_mark32(s["col_live"]), add_mark=_mark32(s["add_live"]))
    return dict(m=m, host=s, dev=dev, csr=ops.DeviceCSR.from_scipy(m, split_len=split_len), n=m.shape[0], d=d)


def _epi_scaled(c):
    return any(c.get(k) for k in ("scale_in", "scale_out", "add_rowscale", "prev_unscale"))


def _epi_kwargs(env, c, y, mean):
    """make_epilogue's arguments of case c on the outputs y / mean"""
    T, kw = env["dev"], {}
    if _epi_scaled(c):
        kw.update(row_scale=T["r"], scale_in=bool(c.get("scale_in")), scale_out=bool(c.get("scale_out")),
                  prev_unscale=c.get("prev_unscale"), add_rowscale=c.get("add_rowscale"))
    if "mean_div" in c:
        kw.update(prev=T["prev"][:c["n_prev"]], mean_div=c["mean_div"], mean_out=mean)
    if "alpha" in c:
        kw.update(add=[y if (t == 0 and c.get("alias0")) else T["add"][t] for t in range(c["n_add"])],
                  add_scale=c.get("add_scale", []), alpha=c["alpha"])
    if c.get("perturb"):
        kw.update(perturb_eps=EPI_EPS, noise=T["noise"])
    if c.get("row_mark") or c.get("col_mark") or c.get("add_sparse"):
        kw.update(mark_stamp=torch.tensor([c.get("stamp", EPI_STAMP)], dtype=torch.int64, device=DEV),
                  row_mark=T["row_mark"] if c.get("row_mark") else None, col_mark=T["col_mark"] if c.get("col_mark") else None,
                  add_mark=T["add_mark"] if c.get("add_sparse") else None, add_sparse=c.get("add_sparse"))
    return kw


def _epi_launch(env, c):
    T, n, d = env["dev"], env["n"], env["d"]
    y = T["add"][0].clone() if c.get("alias0") else torch.full((n, d), 7.0, device=DEV)
    mean = torch.full((n, d), 7.0, device=DEV) if "mean_div" in c else None
    ops.spmm(env["csr"], T["x_cols"] if c.get("col_mark") else T["x"], out=y, pattern=bool(c.get("pattern")),
             epilogue=ops.make_epilogue(**_epi_kwargs(env, c, y, mean)))
    return y, mean


def _epi_ref(env, c, x=None, noise=True):
    s, n, d = env["host"], env["n"], env["d"]
    sent = np.full((n, d), 7.0)
    x = (s["x_cols"] if c.get("col_mark") else s["x"]) if x is None else x
    return R.epilogue_ref(
        env["m"], x, vals_pattern=bool(c.get("pattern")), row_scale=s["r"] if _epi_scaled(c) else None,
        scale_in=bool(c.get("scale_in")), scale_out=bool(c.get("scale_out")),
        alpha=c["alpha"] if ("alpha" in c and (c["n_add"] or c["alpha"] != 1.0)) else None,
        add=s["add"][:c.get("n_add", 0)], add_scale=c.get("add_scale", []), add_rowscale=c.get("add_rowscale"),
        add_sparse=c.get("add_sparse"), add_live=s["add_live"], prev=s["prev"][:c.get("n_prev", 0)],
        prev_unscale=c.get("prev_unscale"), mean_div=c.get("mean_div"), row_live=s["row_live"] if c.get("row_mark") else None,
        col_live=s["col_live"] if c.get("col_mark") else None, y_before=s["add"][0] if c.get("alias0") else sent,
        mean_before=sent, noise=s["noise"] if (c.get("perturb") and noise) else None, eps=EPI_EPS)


def _check_epi_case(env, name, c, report):
    what = f"{name} (d={env['d']})"
    y, mean = _epi_launch(env, c)
    y2, mean2 = _epi_launch(env, c)
    assert torch.equal(y, y2) and (mean is None or torch.equal(mean, mean2)), f"{what}: two launches differ"
    y64, mean64, by, bm = _epi_ref(env, c)
    skip = None
    if c.get("perturb"):
        raw = _epi_ref(env, {**c, "scale_out": False}, noise=False)[0]          # the value whose sign the perturbation takes
        if c.get("row_mark"):
            raw = np.where(env["host"]["row_live"][:, None], raw, 1.0)
        skip, under_cap = R.sign_ambiguous(raw)
        report.append(f"{what}: {int(skip.sum())} sign-ambiguous elements skipped")
        assert under_cap, f"{what}: {int(skip.sum())} sign-ambiguous elements"
        assert np.all(y.cpu().numpy()[raw == 0] == 0), f"{what}: sign(0) = 0"
    for got, want, bound, out in ((y, y64, by, "y"), (mean, mean64, bm, "mean_out")):
        if got is None:
            continue
        bad, worst = R.violations(got.cpu().numpy(), want, bound, skip)
        assert bad == 0, f"{what} {out}: {worst}"
    if c.get("row_mark"):
        dead = ~env["host"]["row_live"]
        assert np.all(y.cpu().numpy()[dead] == 7.0) and (mean is None or np.all(mean.cpu().numpy()[dead] == 7.0)), what


def _print_report(report):
    if report:
        print("\n".join(report))


@pytest.mark.parametrize("split_len", [0, 64], ids=["split-default", "split-64"])
@pytest.mark.parametrize("d", [64, 128, 256])
def test_spmm_epilogue_cases_match_float64_restatement(d, split_len):
    """MEAN, AXPY, the row-scaling masks and the activity marks of srh_spmm_epilogue_t, one launch per EPI_CASES entry, on a
    3000-node power-law graph with three 1500-entry rows (default split: 3 segments each; split 64: 24, the row finished
    by the last segment to arrive), 40 empty rows, and a row scale that is exactly 0 on 2 % of the rows (one heavy row
    and the empty rows among them) -- each output element within the restatement's own bound."""
    env, report = _epi_env(d, split_len), []
    for name, c in EPI_CASES:
        _check_epi_case(env, name, c, report)
    _print_report(report)


@pytest.mark.parametrize("d", [8, 16, 32])
def test_thin_spmm_epilogue_cases_match_float64_restatement(d):
    """The thin kernels (pair: d = 8, slice: d = 16 / 32) on the split-64 graph: MEAN, AXPY, row / column / addend marks
    against the restatement; what the header does not serve there -- row scaling, ADAM, zero-padded rows -- is REFUSED,
    not ignored, before any launch."""
    env, report = _epi_env(d, 64), []
    for name, c in THIN_CASES:
        if c.get("perturb") and d % 32:
            continue        # (PERTURB normalises over whole rows a multiple of 32 wide: narrower tables are slices, COUNTER_CASES)
        _check_epi_case(env, name, c, report)
    _print_report(report)
    T, n = env["dev"], env["n"]
    y, z = torch.full((n, d), 7.0, device=DEV), torch.full((n, d), 7.0, device=DEV)
    coef = torch.tensor([1e-3, 1.0], device=DEV)
    refused = {"scale_in": dict(row_scale=T["r"], scale_in=True), "scale_out": dict(row_scale=T["r"], scale_out=True),
               "add_rowscale": dict(row_scale=T["r"], add=[T["add"][0]], add_scale=[1.0], add_rowscale=[True]),
               "prev_unscale": dict(row_scale=T["r"], prev=[T["prev"][0]], mean_div=2.0, mean_out=z, prev_unscale=[True]),
               "adam": dict(adam=dict(param=z, m=z.clone(), v=z.clone(), coef=coef)),
               "d_valid": dict(perturb_eps=EPI_EPS, noise=T["noise"], d_valid=d - 2)}
    for name, kw in refused.items():
        with pytest.raises(ops.SelfrecHipError):
            ops.spmm(env["csr"], T["x"], out=y, epilogue=ops.make_epilogue(**kw))
        torch.cuda.synchronize()
        assert float((y - 7.0).abs().max()) == 0 and float((z - 7.0).abs().max()) == 0, name


@pytest.mark.parametrize("split_len", [0, 64], ids=["split-default", "split-64"])
@pytest.mark.parametrize("d", [64, 128, 256])
def test_spmm_prescaled_chains_match_true_float64_products(d, split_len):
    """The chains the engine runs in the pre-scaled domain, END TO END against products with diag(r) P diag(r) in float64.
    Forward: (SCALE_IN | SCALE_OUT) twice, then SCALE_IN + MEAN with both earlier layers un-scaled.  Backward: a value
    product stored pre-scaled with two batch-sparse addends (one row-scaled), a pattern product, and the last one
    accumulating into its own output.  The tolerance of a launch is its restatement bound plus the previous launch's
    tolerance carried through |r| P |r| (the operator is non-negative)."""
    env = _epi_env(d, split_len)
    s, T, m, n, csr = env["host"], env["dev"], env["m"], env["n"], env["csr"]
    r = s["r"].astype(np.float64)[:, None]
    with np.errstate(divide="ignore"):
        rinv = np.where(r > 0, 1.0 / np.where(r > 0, r, 1.0), 0.0)
    P = m.astype(np.float64)
    P.data[:] = 1.0
    Ahat = sp.diags(r[:, 0]) @ P @ sp.diags(r[:, 0])

    def held(got, want, tol, what):
        bad, worst = R.violations(got.cpu().numpy(), want, tol / R.BOUND_FACTOR)
        assert bad == 0, f"{what} (d={d}): {worst}"

    # ---- forward ----
    E = s["x"].astype(np.float64)
    xs0 = (r * E).astype(np.float32)
    t1 = Ahat @ E
    t2 = Ahat @ t1
    t3 = Ahat @ t2
    tol0 = R.U32 * np.abs(xs0)
    y1 = torch.full((n, d), 7.0, device=DEV)
    y2, y3, mean = y1.clone(), y1.clone(), y1.clone()
    for out, x_in in ((y1, _t32(xs0)), (y2, y1)):
        ops.spmm(csr, x_in, out=out, pattern=True, epilogue=ops.make_epilogue(row_scale=T["r"], scale_in=True, scale_out=True))
    ops.spmm(csr, y2, out=y3, pattern=True,
             epilogue=ops.make_epilogue(row_scale=T["r"], scale_in=True, prev=[y1, y2], prev_unscale=[True, True], mean_div=3.0,
                                        mean_out=mean))
    c12 = dict(pattern=True, scale_in=True, scale_out=True)
    b1 = _epi_ref(env, c12, x=r * E)[2]
    tol1 = r * r * (P @ tol0) + R.BOUND_FACTOR * b1
    b2 = _epi_ref(env, c12, x=r * t1)[2]
    tol2 = r * r * (P @ tol1) + R.BOUND_FACTOR * b2
    _, _, b3, b3m = R.epilogue_ref(m, r * t2, vals_pattern=True, row_scale=s["r"], scale_in=True, prev=[r * t1, r * t2],
                                   prev_unscale=[True, True], mean_div=3.0)
    tol3 = r * (P @ tol2) + R.BOUND_FACTOR * b3
    tolm = (rinv * tol1 + rinv * tol2 + r * (P @ tol2)) / 3.0 + R.BOUND_FACTOR * b3m
    held(y1, r * t1, tol1, "forward layer 1 (pre-scaled)")
    held(y2, r * t2, tol2, "forward layer 2 (pre-scaled)")
    held(y3, t3, tol3, "forward layer 3 (true)")
    held(mean, (t1 + t2 + t3) / 3.0, tolm, "forward mean")
    assert np.all(mean.cpu().numpy()[r[:, 0] == 0] == 0)               # an isolated node's rows are exactly 0
    # ---- backward ----
    L = s["add_live"][:, None].astype(np.float64)
    a0, a1, G, acc0 = (t.astype(np.float64) for t in (s["add"][0], s["add"][1], s["x"], s["prev"][0]))
    rows = np.repeat(np.arange(n), np.diff(m.indptr))
    vals1 = (s["r"][rows] * s["r"][m.indices]).astype(np.float32)      # D^-1/2 A D^-1/2 as a value array (the chain's first)
    A1 = sp.csr_matrix((vals1.astype(np.float64), m.indices, m.indptr), shape=m.shape)
    csr1 = csr.with_values(_t32(vals1))
    mk = dict(add_mark=T["add_mark"], mark_stamp=torch.tensor([EPI_STAMP], dtype=torch.int64, device=DEV))
    h2, h1, g0 = torch.full((n, d), 7.0, device=DEV), torch.full((n, d), 7.0, device=DEV), T["prev"][0].clone()
    ops.spmm(csr1, T["x"], out=h2, epilogue=ops.make_epilogue(
        row_scale=T["r"], scale_out=True, alpha=0.5, add=T["add"], add_scale=[0.5, 1.0], add_rowscale=[False, True],
        add_sparse=[True, True], **mk))
    ops.spmm(csr, h2, out=h1, pattern=True, epilogue=ops.make_epilogue(
        row_scale=T["r"], scale_in=True, scale_out=True, add=[T["add"][0]], add_scale=[0.5], add_sparse=[True], **mk))
    ops.spmm(csr, h1, out=g0, pattern=True, epilogue=ops.make_epilogue(
        row_scale=T["r"], scale_in=True, add=[g0, T["add"][1]], add_scale=[1.0, 1.0], add_rowscale=[False, True],
        add_sparse=[False, True], **mk))
    H2 = 0.5 * (A1 @ G) + 0.5 * L * a0 + r * L * a1
    H1 = Ahat @ H2 + 0.5 * L * a0
    G0 = Ahat @ H1 + acc0 + r * L * a1
    live = s["add_live"]
    bA = R.epilogue_ref(A1, s["x"], row_scale=s["r"], scale_out=True, alpha=0.5, add=s["add"], add_scale=[0.5, 1.0],
                        add_rowscale=[False, True], add_sparse=[True, True], add_live=live)[2]
    tolA = R.BOUND_FACTOR * bA
    bB = R.epilogue_ref(m, r * H2, vals_pattern=True, row_scale=s["r"], scale_in=True, scale_out=True, alpha=1.0, add=s["add"][:1],
                        add_scale=[0.5], add_sparse=[True], add_live=live)[2]
    tolB = r * r * (P @ tolA) + R.BOUND_FACTOR * bB
    bC = R.epilogue_ref(m, r * H1, vals_pattern=True, row_scale=s["r"], scale_in=True, alpha=1.0, add=[s["prev"][0], s["add"][1]],
                        add_scale=[1.0, 1.0], add_rowscale=[False, True], add_sparse=[False, True], add_live=live)[2]
    tolC = r * (P @ tolB) + R.BOUND_FACTOR * bC
    held(h2, r * H2, tolA, "backward product 1 (pre-scaled)")
    held(h1, r * H1, tolB, "backward product 2 (pre-scaled)")
    held(g0, G0, tolC, "backward product 3 (accumulated, true)")


ADAM_HYPER = tuple(float(np.float32(c)) for c in (1e-3, 0.9, 0.999, 1e-8))       # lr, beta1, beta2, eps as the C ABI carries them
_ADAM_AX = dict(alpha=0.25, n_add=2, add_scale=[0.25, 1.0])
ADAM_CASES = [
    ("adam-step7-sparse11-clear2-cursor", dict(step=7, add_sparse=[True, True], n_clear=2, cursor=True, **_ADAM_AX)),
    ("adam-step1-dense-clear0", dict(step=1, n_clear=0, cursor=False, **_ADAM_AX)),
    ("adam-step100000-scale-in-pattern-clear4-cursor", dict(step=100000, pattern=True, scale_in=True, add_rowscale=[False, True],
                                                            add_sparse=[True, False], n_clear=4, cursor=True, **_ADAM_AX)),
    ("adam-step7-scale-in-values-clear2", dict(step=7, scale_in=True, add_sparse=[True, True], n_clear=2, cursor=False, **_ADAM_AX)),
    ("adam-step1-alpha-only-cursor", dict(step=1, alpha=0.25, n_add=0, n_clear=0, cursor=True)),
    ("adam-step100000-sparse01-clear2-stamp>2^31", dict(step=100000, add_sparse=[False, True], n_clear=2, cursor=False,
                                                       stamp=EPI_STAMP_BIG, **_ADAM_AX)),
]


def _adam_launch(env, c):
    """one SRH_EPI_ADAM launch on fresh state -> dict of the tensors it may touch"""
    a, n, d = env["adam"], env["n"], env["d"]
    lr, b1, b2, eps = ADAM_HYPER
    st = dict(p=_t32(a["p"]), m=_t32(a["m"]), v=_t32(a["v"]), y=torch.full((n, d), 7.0, device=DEV),
              add=[_t32(t) for t in a["add"]], extra=[_t32(t) for t in env["host"]["prev"][:2]],
              cursor=torch.tensor([3, c["step"]], dtype=torch.int64, device=DEV))
    coef = torch.tensor([lr / (1.0 - b1 ** c["step"]), (1.0 - b2 ** c["step"]) ** 0.5], dtype=torch.float32, device=DEV)
    st["clear"] = (st["add"] + st["extra"])[:c["n_clear"]]
    mark = _mark32(a["add_live"])
    adam = dict(param=st["p"], m=st["m"], v=st["v"], coef=coef, beta1=b1, beta2=b2, eps=eps, clear=st["clear"],
                clear_mark=mark if c["n_clear"] else None, cursor=st["cursor"] if c["cursor"] else None)
    kw = dict(add=st["add"][:c["n_add"]], add_scale=c.get("add_scale", []), alpha=c["alpha"], adam=adam)
    if c.get("scale_in"):
        kw.update(row_scale=_t32(a["r"]), scale_in=True, add_rowscale=c.get("add_rowscale"))
    if c.get("add_sparse") or c["n_clear"]:
        kw.update(mark_stamp=torch.tensor([c.get("stamp", EPI_STAMP)], dtype=torch.int64, device=DEV))
    if c.get("add_sparse"):
        kw.update(add_mark=mark, add_sparse=c["add_sparse"])
    ops.spmm(env["csr"], env["adam_x"], out=st["y"], pattern=bool(c.get("pattern")), epilogue=ops.make_epilogue(**kw))
    torch.cuda.synchronize()
    return st


@pytest.mark.parametrize("split_len", [0, 64], ids=["split-default", "split-64"])
@pytest.mark.parametrize("d", [64, 128, 256])
def test_spmm_adam_epilogue_matches_float64_adam(d, split_len):
    """SRH_EPI_ADAM against torch's formula in float64 (spmm_ref.adam_ref) fed the FLOAT64 gradient of the restatement: both
    moments within their bounds; the parameter inside the hull of adam_ref at g -/+ bound_g, widened by 4 * 2^-24 (|p| +
    |update|) -- sqrt(v_hat) is near eps-sized gradients on part of the table, so no blanket number; less than 1 % of the
    hull may be wider than 1e-3 |update| (asserted: the check cannot go vacuous).  d_y keeps its sentinel, the tables to
    clear are zero exactly on the marked rows, the cursor moves by one."""
    env = _epi_env(d, split_len)
    a = env["adam"] = R.adam_inputs(env["m"], d, seed=d)
    env["adam_x"] = _t32(a["x"])
    lr, b1, b2, eps = ADAM_HYPER
    report = []
    for name, c in ADAM_CASES:
        what = f"{name} (d={d})"
        st, st2 = _adam_launch(env, c), _adam_launch(env, c)
        for k in ("p", "m", "v", "cursor"):
            assert torch.equal(st[k], st2[k]), f"{what}: two launches differ in {k}"
        g64, _, bg, _ = R.epilogue_ref(env["m"], a["x"], vals_pattern=bool(c.get("pattern")),
                                       row_scale=a["r"] if c.get("scale_in") else None, scale_in=bool(c.get("scale_in")),
                                       alpha=c["alpha"], add=a["add"][:c["n_add"]], add_scale=c.get("add_scale", []),
                                       add_rowscale=c.get("add_rowscale"), add_sparse=c.get("add_sparse"), add_live=a["add_live"])
        w = R.adam_bounds(a["p"], a["m"], a["v"], g64, bg, c["step"], lr, b1, b2, eps)
        ill = float(w["ill"].mean())
        report.append(f"{what}: ill-conditioned fraction {ill:.5f}")
        assert ill < 0.01, what
        for k in ("m", "v"):
            bad, worst = R.violations(st[k].cpu().numpy(), w[k], w["bound_" + k])
            assert bad == 0, f"{what} {k}: {worst}"
        p = st["p"].cpu().numpy().astype(np.float64)
        out = ~((p >= w["p_lo"]) & (p <= w["p_hi"]))
        i = np.unravel_index(int(np.argmax(np.maximum(w["p_lo"] - p, p - w["p_hi"]))), p.shape)
        assert not out.any(), f"{what} p: {int(out.sum())} outside the hull; at {i}: {p[i]!r} not in [{w['p_lo'][i]!r}, {w['p_hi'][i]!r}]"
        e = a["empty"]                                             # g = 0, m0 = v0 = 0 exactly: 0 / (0 + eps), no move at all
        assert np.all(g64[e] == 0) and np.array_equal(st["p"].cpu().numpy()[e], a["p"][e]), what
        assert np.all(st["m"].cpu().numpy()[e] == 0) and np.all(st["v"].cpu().numpy()[e] == 0), what
        assert float((st["y"] - 7.0).abs().max()) == 0, f"{what}: d_y was written"
        assert st["cursor"].tolist() == ([4, c["step"] + 1] if c["cursor"] else [3, c["step"]]), what
        live = a["add_live"]
        before = a["add"] + env["host"]["prev"][:2]
        for k, t in enumerate(st["add"] + st["extra"]):
            got = t.cpu().numpy()
            if k < c["n_clear"]:
                assert np.all(got[live] == 0) and np.array_equal(got[~live], before[k][~live]), f"{what}: cleared table {k}"
            else:
                assert np.array_equal(got, before[k]), f"{what}: table {k} is not to be cleared"
    _print_report(report)


def test_spmm_epilogue_rejections_happen_before_any_launch():
    """What the header promises to refuse: MEAN with mean_div = 0 or n_prev = 9; n_add = 3; marks without a stamp; an unknown
    scale_flags bit; row scaling without d_row_scale; ADAM next to MEAN / SCALE_OUT / row marks / PERTURB, or with a table
    that is the product's x.  Every output keeps its sentinel."""
    env = _epi_env(64, 0)
    T, n, d, csr = env["dev"], env["n"], 64, env["csr"]
    y, mean = torch.full((n, d), 7.0, device=DEV), torch.full((n, d), 7.0, device=DEV)
    p, mo, v = (torch.full((n, d), 7.0, device=DEV) for _ in range(3))
    coef = torch.tensor([1e-3, 1.0], device=DEV)
    stamp = torch.tensor([EPI_STAMP], dtype=torch.int64, device=DEV)
    adam = dict(param=p, m=mo, v=v, coef=coef)
    x_before = T["x"].clone()

    def changed(ep, **fields):
        for k, val in fields.items():
            setattr(ep, k, val)
        return ep
    L = ops._lib
    cases = {
        "mean_div=0": lambda: ops.make_epilogue(prev=T["prev"][:2], mean_div=0.0, mean_out=mean),
        "n_prev=9": lambda: changed(ops.make_epilogue(prev=T["prev"][:8], mean_div=9.0, mean_out=mean), n_prev=9),
        "n_prev=-1": lambda: changed(ops.make_epilogue(prev=T["prev"][:8], mean_div=9.0, mean_out=mean), n_prev=-1),
        "n_add=3": lambda: changed(ops.make_epilogue(add=T["add"], add_scale=[1.0, 1.0]), n_add=3),
        "row_mark without stamp": lambda: ops.make_epilogue(row_mark=T["row_mark"]),
        "col_mark without stamp": lambda: ops.make_epilogue(col_mark=T["col_mark"]),
        "add_mark without stamp": lambda: ops.make_epilogue(add=T["add"], add_scale=[1.0, 1.0], add_mark=T["add_mark"], add_sparse=[True, True]),
        "unknown scale flag": lambda: changed(ops.make_epilogue(row_scale=T["r"], scale_in=True), scale_flags=L.SRH_SCALE_IN | 4),
        "unknown epilogue flag": lambda: changed(ops.make_epilogue(alpha=0.5), flags=L.SRH_EPI_AXPY | 16),
        "SCALE_IN without d_row_scale": lambda: changed(ops.make_epilogue(alpha=0.5), scale_flags=L.SRH_SCALE_IN),
        "prev_unscale without d_row_scale": lambda: changed(ops.make_epilogue(prev=T["prev"][:1], mean_div=2.0, mean_out=mean), prev_unscale_mask=1),
        "add_rowscale without d_row_scale": lambda: changed(ops.make_epilogue(add=T["add"], add_scale=[1.0, 1.0]), add_rowscale_mask=2),
        "ADAM + MEAN": lambda: ops.make_epilogue(prev=T["prev"][:1], mean_div=2.0, mean_out=mean, adam=adam),
        "ADAM + SCALE_OUT": lambda: ops.make_epilogue(row_scale=T["r"], scale_out=True, adam=adam),
        "ADAM + PERTURB": lambda: ops.make_epilogue(perturb_eps=0.1, noise=T["noise"], adam=adam),
        "ADAM + row marks": lambda: ops.make_epilogue(row_mark=T["row_mark"], mark_stamp=stamp, adam=adam),
        "ADAM + column marks": lambda: ops.make_epilogue(col_mark=T["col_mark"], mark_stamp=stamp, adam=adam),
        "ADAM param is x": lambda: ops.make_epilogue(adam=dict(adam, param=T["x"])),
        "ADAM m is x": lambda: ops.make_epilogue(adam=dict(adam, m=T["x"])),
        "ADAM v is x": lambda: ops.make_epilogue(adam=dict(adam, v=T["x"])),
        "ADAM clears x": lambda: ops.make_epilogue(mark_stamp=stamp, adam=dict(adam, clear=[T["x"]], clear_mark=T["add_mark"])),
        "ADAM clear without marks": lambda: ops.make_epilogue(mark_stamp=stamp, adam=dict(adam, clear=[T["add"][0].clone()])),
        "ADAM without coef": lambda: changed(ops.make_epilogue(adam=adam), d_adam_coef=None),
    }
    for name, make in cases.items():
        with pytest.raises(ops.SelfrecHipError):
            ops.spmm(csr, T["x"], out=y, epilogue=make())
        torch.cuda.synchronize()
        for t in (y, mean, p, mo, v):
            assert float((t - 7.0).abs().max()) == 0, name
        assert torch.equal(T["x"], x_before), name
    with pytest.raises(ops.SelfrecHipError):                      # a pattern product takes no column marks
        ops.spmm(csr, T["x_cols"], out=y, pattern=True, epilogue=ops.make_epilogue(col_mark=T["col_mark"], mark_stamp=stamp))
    torch.cuda.synchronize()
    assert float((y - 7.0).abs().max()) == 0


@pytest.mark.selfcheck
def test_product_with_batch_fetch_rider_equals_the_two_launches(tiny_data):
    """srh_spmm_f32_with_fetch: the product and the staged batch are those of srh_spmm_f32 + srh_batch_fetch."""
    g = tiny_data.device_graph()
    N, d, B, E = g.n_nodes, 64, 32, 100
    rng = np.random.default_rng(11)
    U = g.n_users
    ep = {"u": rng.integers(0, U, E), "i": rng.integers(U, N, E), "j": rng.integers(U, N, E),
          "uniq_u": rng.integers(0, U, E), "uniq_i": rng.integers(U, N, E),
          "n_uniq_u": rng.integers(1, B, (E + B - 1) // B), "n_uniq_i": rng.integers(1, B, (E + B - 1) // B)}
    ep = {k: torch.from_numpy(v.astype(np.int32)).to(DEV) for k, v in ep.items()}
    x = torch.from_numpy(rng.standard_normal((N, d)).astype(np.float32)).to(DEV)
    cursor = torch.tensor([3, 17], dtype=torch.int64, device=DEV)          # the last, short batch: 4 of 32 rows

    def buffers():
        stage = {k: torch.full((B,), -1, dtype=torch.int32, device=DEV) for k in ("u", "i", "j", "uniq_u", "uniq_i")}
        return dict(stage=stage, meta=torch.full((4,), -1, dtype=torch.int32, device=DEV),
                    mark=torch.zeros(N, dtype=torch.int32, device=DEV), zero4=torch.ones(4, dtype=torch.float64, device=DEV),
                    cat=torch.full((2 * B,), -1, dtype=torch.int32, device=DEV), n_cat=torch.zeros(1, dtype=torch.int32, device=DEV),
                    now=torch.zeros(2, dtype=torch.int64, device=DEV))

    def args(b):
        return ops.batch_fetch_args(ep, E, B, cursor, b["stage"], b["meta"], row_mark=b["mark"], zero4=b["zero4"],
                                    stage_cat=b["cat"], cat_item_offset=5, n_cat=b["n_cat"], now=b["now"])
    one, two = buffers(), buffers()
    epi = lambda: ops.make_epilogue(perturb_eps=0.2, rng_seed=3, rng_offset=0)      # noqa: E731
    y1 = ops.spmm(g.adj, x, epilogue=epi(), fetch=args(one))
    ops.batch_fetch(args(two))
    y2 = ops.spmm(g.adj, x, epilogue=epi())
    assert torch.equal(y1, y2)
    assert int(one["meta"][0]) == E - 3 * B and torch.equal(one["now"], cursor) and float(one["zero4"].abs().sum()) == 0.0
    assert int((one["mark"] == 17).sum()) > 0
    for k in ("meta", "mark", "zero4", "cat", "n_cat", "now"):
        assert torch.equal(one[k], two[k]), k
    for k in one["stage"]:
        assert torch.equal(one["stage"][k], two["stage"][k]), k
    # the product may not depend on what the fetch writes
    with pytest.raises(ops.SelfrecHipError):
        ops.spmm(g.adj, x, epilogue=ops.make_epilogue(row_mark=one["mark"], mark_stamp=cursor[1:2]), fetch=args(one))


def test_batch_fetch_over_two_epochs_back_to_back():
    """srh_batch_fetch_args_t::half_batches: the arrays hold two epochs of nb batch slots each; batch no b >= nb is batch
    b - nb of the second epoch -- cut against n_edges with b - nb (the last batch of EITHER epoch is short), read at b.
    Every batch of both halves against the CPU stand-in of the same call (tests/cpu_ops.py)."""
    from tests import cpu_ops
    rng = np.random.default_rng(21)
    B, E, N = 32, 100, 500
    nb = (E + B - 1) // B
    host = {k: rng.integers(0, N, 2 * nb * B).astype(np.int32) for k in ("u", "i", "j", "uniq_u", "uniq_i")}
    host["n_uniq_u"] = rng.integers(1, B, 2 * nb).astype(np.int32)
    host["n_uniq_i"] = rng.integers(1, B, 2 * nb).astype(np.int32)
    dev_ep = {k: torch.from_numpy(v).to(DEV) for k, v in host.items()}
    cpu_ep = {k: torch.from_numpy(v) for k, v in host.items()}

    def buffers(dev):
        return dict(stage={k: torch.full((B,), -1, dtype=torch.int32, device=dev) for k in ("u", "i", "j", "uniq_u", "uniq_i")},
                    meta=torch.full((4,), -1, dtype=torch.int32, device=dev), mark=torch.zeros(N, dtype=torch.int32, device=dev))
    for b in range(2 * nb + 1):                                       # (+ one batch past the end: 0 rows)
        got, want = buffers(DEV), buffers("cpu")
        ops.batch_fetch(dev_ep, E, B, torch.tensor([b, 9], dtype=torch.int64, device=DEV), got["stage"], got["meta"],
                        row_mark=got["mark"], half_batches=nb)
        cpu_ops.batch_fetch(cpu_ep, E, B, torch.tensor([b, 9], dtype=torch.int64), want["stage"], want["meta"],
                            row_mark=want["mark"], half_batches=nb)
        rows = int(want["meta"][0])
        assert rows == (E - (nb - 1) * B if b % nb == nb - 1 and b < 2 * nb else (B if b < 2 * nb else 0)), (b, rows)
        assert torch.equal(got["meta"].cpu(), want["meta"]) and torch.equal(got["mark"].cpu(), want["mark"]), b
        for k in ("u", "i", "j"):
            assert torch.equal(got["stage"][k][:rows].cpu(), want["stage"][k][:rows]), (b, k)
        a, c = int(want["meta"][1]), int(want["meta"][2])
        assert torch.equal(got["stage"]["uniq_u"][:a].cpu(), want["stage"]["uniq_u"][:a])
        assert torch.equal(got["stage"]["uniq_i"][:c].cpu(), want["stage"]["uniq_i"][:c])


# ------------------------------------------------------------------------------------------
# (a-2) normalisation and edge-dropped views
# ------------------------------------------------------------------------------------------
def test_device_normalisation_matches_reference(golden_ops, tiny_data):
    g = tiny_data.device_graph()
    assert np.array_equal(g.adj.indptr.cpu().numpy(), golden_ops["norm_adj_indptr"])
    # (long rows are stored [even columns | odd columns] for the SpMM schedule: compare in sorted order)
    mine = sp.csr_matrix((g.adj.vals.cpu().numpy(), g.adj.indices.cpu().numpy(), g.adj.indptr.cpu().numpy()),
                         shape=(g.n_nodes, g.n_nodes))
    mine.sort_indices()
    assert np.array_equal(mine.indices, golden_ops["norm_adj_indices"])
    assert np.array_equal(mine.data, golden_ops["norm_adj_data"])    # bit-exact (host pow table)
    # edge-dropped, re-normalised view (SGL.py:89-96) from the reference keep-set
    keep = np.zeros(g.n_edges, dtype=np.uint8)
    keep[golden_ops["edge_dropout_keep"]] = 1
    view = g.dropped_view(torch.from_numpy(keep).to(DEV))
    dense = sp.csr_matrix((view.vals.cpu().numpy(), g.adj.indices.cpu().numpy(), g.adj.indptr.cpu().numpy()),
                          shape=(g.n_nodes, g.n_nodes))
    dense.eliminate_zeros()
    dense.sort_indices()
    assert np.array_equal(dense.indptr, golden_ops["edge_dropout_lap_indptr"])
    assert np.array_equal(dense.indices, golden_ops["edge_dropout_lap_indices"])
    assert np.array_equal(dense.data, golden_ops["edge_dropout_lap_data"])


def test_normalisation_isolated_nodes_and_weights():
    # node 2 isolated after dropping its only edge; duplicate interaction -> weight 2 in the full adjacency
    # (scipy sums it, ui_graph.py:47-56) but 1 in a dropped view (augmentor.py:36-39 rebuilds with ones)
    r = sp.csr_matrix((np.array([1, 2, 1, 1], dtype=np.float32), ([0, 0, 1, 2], [0, 1, 1, 2])), shape=(3, 3))
    from selfrec_amd.data.device_graph import DeviceGraph
    g = DeviceGraph(r)
    want = O.laplacian_of(r).tocsr(); want.sort_indices()
    np.testing.assert_allclose(g.adj.vals.cpu().numpy(), want.data, rtol=3e-7)
    keep = torch.tensor([1, 1, 1, 0], dtype=torch.uint8, device=DEV)
    v = g.dropped_view(keep).vals.cpu().numpy()
    r2 = r.copy(); r2.data[:] = 1.0; r2.data[3] = 0; r2.eliminate_zeros()
    with np.errstate(divide="ignore"):
        want2 = O.laplacian_of(r2).toarray()
    got2 = sp.csr_matrix((v, g.adj.indices.cpu().numpy(), g.adj.indptr.cpu().numpy()), shape=(6, 6)).toarray()
    np.testing.assert_allclose(got2, want2, rtol=3e-7)
    assert np.isfinite(v).all()


# ------------------------------------------------------------------------------------------
# (a-5..a-8) losses
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 130, 515])
def test_loss_functions_match_reference_outputs(golden_ops, n):
    from selfrec_amd.util import loss_torch as L
    g = golden_ops
    u, p, q = (torch.tensor(x, device=DEV, requires_grad=True) for x in g[f"ops_{n}_in"])
    bpr, reg, nce = L.bpr_loss(u, p, q), L.l2_reg_loss(1e-4, u, p, q), L.InfoNCE(u, p, 0.2)
    np.testing.assert_allclose([bpr.item(), reg.item()], g[f"ops_{n}_loss"][:2], rtol=2e-6)
    # InfoNCE evaluates its similarity products in split-bf16 (3-term) MFMA: logits carry <= 2e-5 absolute
    # error, which only shows at tiny n where nothing averages out (budget: 1e-4 relative)
    np.testing.assert_allclose(nce.item(), g[f"ops_{n}_loss"][2], rtol=2e-5, atol=5e-6)
    gb = torch.stack(torch.autograd.grad(bpr, (u, p, q))).cpu().numpy()
    gr = torch.stack(torch.autograd.grad(reg, (u, p, q))).cpu().numpy()
    gn = torch.stack(torch.autograd.grad(nce, (u, p))).cpu().numpy()
    assert rel_err(gb, g[f"ops_{n}_g_bpr"]) < 1e-5
    assert rel_err(gr, g[f"ops_{n}_g_reg"]) < 1e-5
    if n == 1:      # a single row: the loss is identically 0 and so is its gradient; ours is rounding noise
        assert np.abs(gn).max() < 1e-5 and not g[f"ops_{n}_g_nce"].any()
    else:
        assert rel_err(gn, g[f"ops_{n}_g_nce"]) < 1e-5


@pytest.mark.parametrize("rows,d", [(1, 64), (2048, 64), (777, 32), (300, 100), (4099, 128)])
def test_single_launch_losses_equal_the_torch_expressions(rows, d):
    """bpr_loss / l2_reg_loss finish their scalars on the device (one launch forward, one backward, a shared 64-byte
    workspace that every call leaves zero): values and gradients against the reference's expressions (loss_torch.py:6-22)
    evaluated by ATen on the same device, with a NON-unit upstream gradient, an all-zero block (zero gradient, as
    torch.norm's), four blocks of different sizes in one call, and the same call repeated."""
    from selfrec_amd import ops
    from selfrec_amd.util import loss_torch as L
    gen = torch.Generator().manual_seed(rows * 31 + d)
    mk = lambda r: (torch.randn(r, d, generator=gen) * 0.3).to(DEV).requires_grad_(True)
    u, p, q = mk(rows), mk(rows), mk(rows)
    z = torch.zeros(5, d, device=DEV, requires_grad=True)
    small = mk(3)

    def expression(u, p, q, z, small):
        pos, neg = torch.mul(u, p).sum(dim=1), torch.mul(u, q).sum(dim=1)
        bpr = torch.mean(-torch.log(10e-6 + torch.sigmoid(pos - neg)))
        emb = 0
        for e in (u, z, p, small):
            emb = emb + torch.norm(e, p=2) / e.shape[0]
        return bpr, emb * 0.37

    for _ in range(3):                                  # (the workspace is shared: repeated calls must not leak into each other)
        bpr, reg = L.bpr_loss(u, p, q), L.l2_reg_loss(0.37, u, z, p, small)
        assert bpr.dtype == torch.float32 and bpr.dim() == 0 and reg.dtype == torch.float32 and reg.dim() == 0
        got = torch.autograd.grad(bpr * 3.7 + reg * -2.5, (u, p, q, z, small))
        wb, wr = expression(u, p, q, z, small)
        want = torch.autograd.grad(wb * 3.7 + wr * -2.5, (u, p, q, z, small))
        np.testing.assert_allclose([bpr.item(), reg.item()], [wb.item(), wr.item()], rtol=2e-6)
        for g, w in zip(got, want):
            assert rel_err(g.cpu().numpy(), w.cpu().numpy()) < 2e-6
        assert not got[3].any()                                         # the zero block
        assert not ops.scalar_ws(u.device).any()
    # five blocks (one more than a launch takes) and a block on the CPU go block by block, same value
    five = L.l2_reg_loss(0.37, u, z, p, small, small)
    assert abs(five.item() - (wr.item() + 0.37 * (torch.norm(small) / 3).item())) < 2e-6 * abs(five.item())
    mixed = L.l2_reg_loss(0.37, u, small.detach().cpu())
    assert abs(mixed.item() - 0.37 * ((torch.norm(u) / rows).item() + (torch.norm(small) / 3).item())) < 2e-6 * abs(mixed.item())
    # the number of launches: what the host pays per call in the op-level tier
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        bpr, reg = L.bpr_loss(u, p, q), L.l2_reg_loss(0.37, u, p)
        (bpr + reg).backward()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    ours = [k for k in names if "bpr_plain" in k or "l2_reg" in k]
    assert len(ours) == 4, names                                        # two forward, two backward


@pytest.fixture(params=["split", "f32"])
def nce_precision(request):
    """Both arithmetic modes of InfoNCE's two n x n x d products (srh_infonce_set_precision): the process default is
    switched for the test and restored."""
    before = ops.get_infonce_precision()
    ops.set_infonce_precision(request.param)
    yield request.param
    ops.set_infonce_precision(before)


@pytest.mark.parametrize("n,d,tau", [(2048, 64, 0.2), (1500, 64, 0.15), (700, 128, 0.2), (17, 64, 0.5), (900, 256, 0.2),
                                     (300, 256, 0.05), (1, 64, 0.2), (64, 64, 0.2), (65, 128, 0.3), (3000, 64, 0.2),
                                     (4096, 64, 0.2), (1100, 128, 0.1), (8300, 64, 0.25)])
def test_infonce_gathered_matches_oracle(n, d, tau, nce_precision):
    if nce_precision == "f32" and d == 256:
        pytest.skip("the all-f32 MFMA passes serve d = 64 / 128")
    if n > 8192 and nce_precision != "f32":
        pytest.skip("n > 8192 is here for the all-f32 passes' second form: pass 2 recomputes the logits (no n x n weight array)")
    rng = np.random.default_rng(n)
    rows = max(5000, n + 200)
    t1 = (rng.standard_normal((rows, d)) * 0.4).astype(np.float32)
    t2 = (t1 + rng.standard_normal((rows, d)) * 0.2).astype(np.float32)
    idx = np.sort(rng.choice(rows, size=n, replace=False)).astype(np.int32)
    # the reference's expression evaluated in float64: at tau = 0.05 on these correlated views the loss is ~3e-6 -- the
    # difference of two numbers near 20 -- and the reference's own f32 arithmetic is off by 1 % there (lse - s_ii with
    # 2e-6 of rounding on each); the kernel forms log1p(l' / e_ii) and is held to the exact value
    a = torch.tensor(t1, dtype=torch.float64, requires_grad=True); b = torch.tensor(t2, dtype=torch.float64, requires_grad=True)
    loss = 0.3 * O.info_nce(a[idx.astype(np.int64)], b[idx.astype(np.int64)], tau)
    loss.backward()
    d1, d2 = torch.from_numpy(t1).to(DEV), torch.from_numpy(t2).to(DEV)
    base = 1e-5                          # g1 is accumulated into, not overwritten
    g1 = torch.full((rows, d), base, device=DEV); g2 = torch.zeros((rows, d), device=DEV)
    out = torch.zeros(1, dtype=torch.float64, device=DEV)
    nmax = n + 100                       # device-side count smaller than the launch bound
    ws = ops.infonce_ws(nmax, d, DEV)
    didx = torch.zeros(nmax, dtype=torch.int32, device=DEV); didx[:n] = torch.from_numpy(idx).to(DEV)
    ops.infonce_fwd_bwd(d1, d2, didx, nmax, n_dev=torch.tensor([n], dtype=torch.int32, device=DEV), tau=tau,
                        loss_scale=0.3, loss=out, g1=g1, g2=g2, ws=ws)
    if n == 1:                           # (one pair: log_softmax of a 1 x 1 matrix -- the loss and its gradients are exactly 0)
        assert out.item() == 0.0 and not (g1 - base).any() and not g2.any()
        return
    assert abs(out.item() - loss.item()) / abs(loss.item()) < 1e-5
    assert rel_err((g1.double() - base).cpu().numpy(), a.grad.numpy()) < (2e-5 if nce_precision == "split" else 3e-6)
    assert rel_err(g2.cpu().numpy(), b.grad.numpy()) < (2e-5 if nce_precision == "split" else 3e-6)


@pytest.mark.parametrize("ns,d", [((1877,), 64), ((2048,), 64), ((4096,), 64), ((1640,), 128), ((1877, 1640), 64),
                                  ((1500, 1999), 128)])
def test_f32_infonce_is_the_same_bits_fifty_times_over(ns, d):
    """The all-f32 passes (persistent workgroups, an LDS ring fed by buffer_load ... lds, hand-placed waits) at the batch
    sizes the benchmark runs -- n ~ 1877 unique users / 1640 unique items of 2048 pairs, d = 64 -- where round 5 found and
    fixed a stale-register bug that showed up as a DIFFERENT loss on every run.  Fifty calls on the same inputs, one and two
    problems per call as the engine issues them: loss and both gradients identical bit for bit across the calls, and within
    2e-6 (loss) / 3e-6 (gradients) of the float64 evaluation of util/loss_torch.py:35-50."""
    tau, scale = 0.2, 0.2
    rng = np.random.default_rng(sum(ns) + d)
    v1 = [(rng.standard_normal((n, d)) * 0.4).astype(np.float32) for n in ns]
    v2 = [(a + rng.standard_normal(a.shape) * 0.2).astype(np.float32) for a in v1]
    want_loss, want_g1, want_g2 = 0.0, [], []
    for a, b in zip(v1, v2):
        ta = torch.tensor(a, dtype=torch.float64, requires_grad=True); tb = torch.tensor(b, dtype=torch.float64, requires_grad=True)
        l = scale * O.info_nce(ta, tb, tau)
        l.backward()
        want_loss += l.item(); want_g1.append(ta.grad.numpy()); want_g2.append(tb.grad.numpy())
    d1 = [torch.from_numpy(a).to(DEV) for a in v1]; d2 = [torch.from_numpy(b).to(DEV) for b in v2]
    g1 = [torch.zeros_like(t) for t in d1]; g2 = [torch.zeros_like(t) for t in d2]
    out = torch.zeros(1, dtype=torch.float64, device=DEV)
    ws = torch.empty(sum(ops.infonce_ws(n, d, DEV).numel() for n in ns), dtype=torch.uint8, device=DEV)
    first = None
    for rep in range(50):
        for t in g1 + g2:
            t.zero_()
        out.zero_()
        ops.infonce_multi([(d1[k], d2[k], None, n, None, g1[k], g2[k]) for k, n in enumerate(ns)], d=d, tau=tau,
                          loss_scale=scale, loss=out, ws=ws, precision="f32")
        got = [out.clone()] + [t.clone() for t in g1 + g2]
        if first is None:
            first = got
            assert abs(out.item() - want_loss) / abs(want_loss) < 2e-6
            for k in range(len(ns)):
                assert rel_err(g1[k].cpu().numpy(), want_g1[k]) < 3e-6
                assert rel_err(g2[k].cpu().numpy(), want_g2[k]) < 3e-6
        else:
            assert all(torch.equal(x, y) for x, y in zip(first, got)), rep


def dev_segments(u, i, j, pad, rows_are_zero=False):
    from .conftest import host_batch_segments
    seg = {k: torch.from_numpy(v).to(DEV) for k, v in host_batch_segments(u, i, j, pad).items()}
    seg["rows_are_zero"] = rows_are_zero
    return seg


@pytest.mark.parametrize("segmented", [False, True, "store"], ids=["atomics", "segments", "segments-store"])
def test_bpr_l2_fused_matches_oracle_with_duplicates(segmented):
    rng = np.random.default_rng(0)
    U, I, d, B = 300, 400, 64, 1000
    ut = (rng.standard_normal((U, d)) * 0.3).astype(np.float32)
    it = (rng.standard_normal((I, d)) * 0.3).astype(np.float32)
    ui, pi, ni = rng.integers(0, U, B), rng.integers(0, I, B), rng.integers(0, I, B)
    for include_neg, ego in ((False, False), (True, False), (True, True)):
        a = torch.tensor(ut, requires_grad=True); b = torch.tensor(it, requires_grad=True)
        ea = torch.tensor(ut * 0.5, requires_grad=True); eb = torch.tensor(it * 0.5, requires_grad=True)
        ra, rb = (ea, eb) if ego else (a, b)
        regs = [ra[ui], rb[pi]] + ([rb[ni]] if include_neg else [])
        bpr = O.bpr_loss(a[ui], b[pi], b[ni]); reg = O.l2_reg_loss(1e-3, *regs)
        (bpr + reg).backward()
        du, di = torch.from_numpy(ut).to(DEV), torch.from_numpy(it).to(DEV)
        dru, dri = (du * 0.5, di * 0.5) if ego else (du, di)
        gu, gi = torch.zeros_like(du), torch.zeros_like(di)
        gru, gri = (torch.zeros_like(du), torch.zeros_like(di)) if ego else (gu, gi)
        losses = torch.zeros(2, dtype=torch.float64, device=DEV)
        cnt = torch.tensor([B], dtype=torch.int32, device=DEV)
        idx = [torch.zeros(B + 24, dtype=torch.int32, device=DEV) for _ in range(3)]
        for t, src in zip(idx, (ui, pi, ni)):
            t[:B] = torch.from_numpy(src.astype(np.int32)).to(DEV)
        # (segmented: every row written once by the row group that owns it, its slots summed in order -- srh_bpr_l2_fwd_bwd_p)
        kw = dict(seg=dev_segments(ui, pi, ni, B + 24, rows_are_zero=segmented == "store")) if segmented else {}
        runs = []
        for rep in range(3 if segmented else 1):
            for t in (gu, gi, gru, gri):
                t.zero_()
            losses.zero_()
            ops.bpr_l2_fwd_bwd(du, di, dru.contiguous(), dri.contiguous(), *idx, batch=B + 24, n_rows_dev=cnt,
                               reg_coef=1e-3, reg_include_neg=include_neg, loss_scale=1.0, g_user=gu, g_item=gi,
                               greg_user=gru, greg_item=gri, losses=losses, ws=ops.bpr_ws(B + 24, DEV), **kw)
            runs.append([t.clone() for t in (gu, gi, gru, gri, losses)])
        np.testing.assert_allclose(losses.cpu().numpy(), [bpr.item(), reg.item()], rtol=2e-6)
        assert rel_err(gu.cpu().numpy(), a.grad.numpy()) < 2e-5
        assert rel_err(gi.cpu().numpy(), b.grad.numpy()) < 2e-5
        if ego:
            assert rel_err(gru.cpu().numpy(), ea.grad.numpy()) < 2e-5
            assert rel_err(gri.cpu().numpy(), eb.grad.numpy()) < 2e-5
        for other in runs[1:]:                      # no float atomics: the same bits every time
            assert all(torch.equal(x, y) for x, y in zip(runs[0], other))


@pytest.mark.parametrize("segmented", [False, True, "store"], ids=["atomics", "segments", "segments-store"])
@pytest.mark.parametrize("d,B", [(64, 2048), (128, 600), (256, 500)])
def test_bpr_infonce_one_call_matches_oracle(d, B, nce_precision, segmented):
    if nce_precision == "f32" and d == 256:
        pytest.skip("the all-f32 MFMA passes serve d = 64 / 128")
    """srh_bpr_infonce_fwd_bwd = XSimGCL.py:30-35: rec + reg + cl_rate * (user InfoNCE + item InfoNCE), with
    the gradients of the final and the contrast-layer tables, against torch autograd on the oracle losses."""
    rng = np.random.default_rng(d + B)
    U, I, tau, cl_rate, reg = 900, 1300, 0.2, 0.2, 1e-4
    F = (rng.standard_normal((U + I, d)) * 0.3).astype(np.float32)
    CL = (F + rng.standard_normal((U + I, d)) * 0.1).astype(np.float32)
    ui, pi, ni = rng.integers(0, U, B), rng.integers(0, I, B), rng.integers(0, I, B)
    uu, up = np.unique(ui), np.unique(pi)
    f = torch.tensor(F, requires_grad=True); c = torch.tensor(CL, requires_grad=True)
    fu, fi, cu, ci = f[:U], f[U:], c[:U], c[U:]
    rec = O.bpr_loss(fu[ui], fi[pi], fi[ni]); l2 = O.l2_reg_loss(reg, fu[ui], fi[pi])
    cl = cl_rate * (O.info_nce(fu[uu], cu[uu], tau) + O.info_nce(fi[up], ci[up], tau))
    (rec + l2 + cl).backward()

    dF, dC = torch.from_numpy(F).to(DEV), torch.from_numpy(CL).to(DEV)
    gF, gC = torch.zeros_like(dF), torch.zeros_like(dC)
    losses = torch.zeros(3, dtype=torch.float64, device=DEV)
    i32 = lambda a, n: torch.cat([torch.from_numpy(a.astype(np.int32)), torch.zeros(n - a.size, dtype=torch.int32)]).to(DEV)
    cnt = lambda n: torch.tensor([n], dtype=torch.int32, device=DEV)
    nce_ws = torch.empty(2 * ops.infonce_ws(B, d, DEV).numel(), dtype=torch.uint8, device=DEV)
    # segmented: the rows' (slot, role) lists come with the call (srh_batch_segments_t, nce_rows = 1: the user-side problem's
    # row i is user group i, the item-side one's positive-item group i) and every gradient row is written exactly once
    kw = dict(seg=dev_segments(ui, pi, ni, B, rows_are_zero=segmented == "store"), nce_rows=1) if segmented else {}
    runs = []
    for rep in range(3):                     # the workspaces re-arm themselves: a second call gives the same
        gF.zero_(); gC.zero_(); losses.zero_()
        ops.bpr_infonce(dF[:U], dF[U:], dF[:U], dF[U:], i32(ui, B), i32(pi, B), i32(ni, B), batch=B, n_rows_dev=cnt(B),
                        reg_coef=reg, reg_include_neg=False, loss_scale=1.0, g_user=gF[:U], g_item=gF[U:],
                        greg_user=gF[:U], greg_item=gF[U:], losses=losses[0:2], bpr_ws=ops.bpr_ws(B, DEV),
                        problems=[(dF[:U], dC[:U], i32(uu, B), B, cnt(uu.size), gF[:U], gC[:U]),
                                  (dF[U:], dC[U:], i32(up, B), B, cnt(up.size), gF[U:], gC[U:])],
                        tau=tau, cl_scale=cl_rate, cl_loss=losses[2:3], nce_ws=nce_ws, **kw)
        np.testing.assert_allclose(losses.cpu().numpy(), [rec.item(), l2.item(), cl.item()], rtol=1e-5)
        assert rel_err(gF.cpu().numpy(), f.grad.numpy()) < 2e-5
        assert rel_err(gC.cpu().numpy(), c.grad.numpy()) < 2e-5
        runs.append((gF.clone(), gC.clone(), losses.clone()))
    if segmented:                            # no float atomics anywhere in the call: the same bits every time
        for other in runs[1:]:
            assert all(torch.equal(x, y) for x, y in zip(runs[0], other))


@pytest.mark.parametrize("d", [64, 128, 256])
def test_filtered_ranking_equals_exact_ranking(d):
    """srh_score_mask_topk_filtered (scores never stored) against srh_score_mask_topk: identical ids and scores
    on every row whose survivor list fits; tie-heavy rows (all-zero user vectors) report an overflow instead."""
    rng = np.random.default_rng(31 + d)
    U, I, K = 1500, 20000, 20
    ue = torch.from_numpy((rng.standard_normal((U, d)) * 0.3).astype(np.float32)).to(DEV)
    ie = torch.from_numpy((rng.standard_normal((I, d)) * 0.3).astype(np.float32)).to(DEV)
    ue[7] = 0.0; ue[900] = 0.0                          # every score equal: thousands of survivors
    ie[100:140] = ie[100]                                # a block of tied items inside the sample slice
    lens = rng.integers(0, 60, U); lens[3] = 5000        # one user with a huge training row
    indptr = np.zeros(U + 1, dtype=np.int32); np.cumsum(lens, out=indptr[1:])
    indices = np.concatenate([np.sort(rng.choice(I, size=n, replace=False)) for n in lens]).astype(np.int32)
    r_indptr, r_indices = torch.from_numpy(indptr).to(DEV), torch.from_numpy(indices).to(DEV)
    users = torch.from_numpy(rng.permutation(U).astype(np.int32)).to(DEV)
    want_ids, want_sc = ops.score_mask_topk(ue, users, ie, r_indptr, r_indices, K)
    for chunk in (4096, 700):                            # one chunk / several chunks with a ragged tail
        ids, sc, counts, _ = ops.score_mask_topk_filtered(ue, users, ie, r_indptr, r_indices, K, sample_items=2048,
                                                          cap=512, chunk_rows=chunk)
        ok = (counts <= 512)
        bad_users = set(users[~ok].tolist())
        assert bad_users == {7, 900}
        assert (counts[ok] >= K).all()
        assert torch.equal(ids[ok], want_ids[ok]) and torch.equal(sc[ok], want_sc[ok])


@pytest.mark.parametrize("d,scale", [(64, 30.0), (64, 1e-3), (128, 5.0)])
def test_split_bf16_filter_never_loses_a_top_k_item(d, scale):
    """At d = 64 / 128 the filter pass of srh_score_mask_topk_filtered decides on bf16 products against per-item error
    bounds (3.94e-3 |u| |i_j|: csrc/eval.hip), and the survivors are re-scored exactly.  Stress for those margins: large and tiny
    magnitudes, a catalogue of near-duplicates (thousands of items within 1e-6 relative of each other, i.e. inside the
    bf16 products' error of the bound), items of very unequal norms -- ids AND scores must still be bit-identical to the
    plain pipeline's on every row that fits."""
    rng = np.random.default_rng(7 + d)
    U, I, K = 700, 12000, 20
    ue = torch.from_numpy((rng.standard_normal((U, d)) * scale).astype(np.float32)).to(DEV)
    base = (rng.standard_normal((40, d)) * scale).astype(np.float32)
    items = base[rng.integers(0, 40, I)] * (1.0 + 1e-6 * rng.standard_normal((I, 1))).astype(np.float32)   # near-duplicates
    items[::7] = (rng.standard_normal((len(items[::7]), d)) * scale * 0.05).astype(np.float32)             # small-norm items
    items[5] *= 20.0                                                                                        # one huge item
    ie = torch.from_numpy(items.astype(np.float32)).to(DEV)
    r_indptr = torch.zeros(U + 1, dtype=torch.int32, device=DEV)
    r_indices = torch.zeros(1, dtype=torch.int32, device=DEV)
    users = torch.arange(U, dtype=torch.int32, device=DEV)
    want_ids, want_sc = ops.score_mask_topk(ue, users, ie, r_indptr, r_indices, K)
    ids, sc, counts, _ = ops.score_mask_topk_filtered(ue, users, ie, r_indptr, r_indices, K, sample_items=2048, cap=1024,
                                                      chunk_rows=512)
    ok = counts <= 1024
    assert ok.float().mean() > 0.5 and (counts[ok] >= K).all()
    assert torch.equal(ids[ok], want_ids[ok]) and torch.equal(sc[ok], want_sc[ok])


# ------------------------------------------------------------------------------------------
# (a-9) Adam
# ------------------------------------------------------------------------------------------
@pytest.mark.selfcheck
@pytest.mark.parametrize("d", [64, 128, 256])
def test_adam_in_the_product_epilogue_equals_product_then_adam(d):
    """SRH_EPI_ADAM: the last backward product with the optimiser step in its row epilogue leaves the bits of
    srh_spmm_f32 (AXPY) followed by srh_adam_step_reset -- parameters, both moments, the cleared batch rows of the sparse
    gradient buffers, the cursor -- with this step's constants written by srh_batch_fetch."""
    rng = np.random.default_rng(90 + d)
    m = powerlaw_csr(3000, 3000, 40000, seed=5, heavy_rows=3, heavy_len=1500, empty_rows=40)
    N, B, E = 3000, 64, 64
    csr = ops.DeviceCSR.from_scipy(m, split_len=64)            # (split rows: the epilogue runs in the last segment to arrive)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)     # noqa: E731
    x = t(rng.standard_normal((N, d)) * 1e-3)
    ids = {k: torch.from_numpy(rng.integers(0, N, E).astype(np.int32)).to(DEV) for k in ("u", "i", "j")}
    step = 7

    def state():
        r = np.random.default_rng(3)
        gF, gCL = np.zeros((N, d), np.float32), np.zeros((N, d), np.float32)
        rows = np.unique(np.concatenate([v.cpu().numpy() for v in ids.values()]))
        gF[rows] = r.standard_normal((rows.size, d)) * 1e-2
        gCL[rows] = r.standard_normal((rows.size, d)) * 1e-2
        return dict(p=t(r.standard_normal((N, d)) * 0.1), m=t(r.standard_normal((N, d)) * 1e-3),
                    v=t(r.random((N, d)) * 1e-5), gF=t(gF), gCL=t(gCL), g=torch.zeros(N, d, device=DEV),
                    cursor=torch.tensor([0, step], dtype=torch.int64, device=DEV), now=torch.zeros(2, dtype=torch.int64, device=DEV),
                    mark=torch.zeros(N, dtype=torch.int32, device=DEV), coef=torch.zeros(2, device=DEV),
                    stage={k: torch.zeros(B, dtype=torch.int32, device=DEV) for k in ("u", "i", "j")},
                    meta=torch.zeros(4, dtype=torch.int32, device=DEV))

    def fetch(s, **kw):
        ops.batch_fetch(ids, E, B, s["cursor"], s["stage"], s["meta"], row_mark=s["mark"], now=s["now"], **kw)
    a, b = state(), state()
    # the separate pass
    fetch(a)
    ops.spmm(csr, x, out=a["g"], epilogue=ops.make_epilogue(add=[a["gF"], a["gCL"]], add_scale=[0.25, 1.0], alpha=0.25,
                                                            add_mark=a["mark"], mark_stamp=a["now"][1:2], add_sparse=[True, True]))
    ops.adam_step(a["p"], a["g"], a["m"], a["v"], step_dev=a["now"][1:2], lr=1e-3, clear=[a["gF"], a["gCL"]],
                  row_mark=a["mark"], advance_cursor=a["cursor"])
    # the fused launch
    fetch(b, adam_coef=b["coef"], adam_lr=1e-3)
    b1, b2, lr = (float(np.float32(c)) for c in (0.9, 0.999, 1e-3))        # (the C ABI takes the betas as float)
    assert np.allclose(b["coef"].cpu().numpy(), (lr / (1 - b1 ** step), (1 - b2 ** step) ** 0.5), rtol=1e-6)
    ops.spmm(csr, x, out=b["g"], epilogue=ops.make_epilogue(
        add=[b["gF"], b["gCL"]], add_scale=[0.25, 1.0], alpha=0.25, add_mark=b["mark"], mark_stamp=b["now"][1:2],
        add_sparse=[True, True],
        adam=dict(param=b["p"], m=b["m"], v=b["v"], coef=b["coef"], clear=[b["gF"], b["gCL"]], clear_mark=b["mark"],
                  cursor=b["cursor"])))
    assert float(a["g"].abs().max()) > 0 and float(b["g"].abs().max()) == 0         # (the gradient is never stored)
    for k in ("p", "m", "v", "gF", "gCL", "cursor"):
        assert torch.equal(a[k], b[k]), k
    assert b["cursor"].tolist() == [1, step + 1] and float(b["gF"].abs().max()) == 0
    assert float((a["p"] - state()["p"]).abs().max()) > 0
    # the stamp may not be the cursor the launch advances; no perturbation / mean next to the optimiser
    with pytest.raises(ops.SelfrecHipError):
        ops.spmm(csr, x, out=b["g"], epilogue=ops.make_epilogue(
            mark_stamp=b["cursor"][1:2], adam=dict(param=b["p"], m=b["m"], v=b["v"], coef=b["coef"], clear=[b["gF"]],
                                                   clear_mark=b["mark"], cursor=b["cursor"][0:2])))
    with pytest.raises(ops.SelfrecHipError):
        ops.spmm(csr, x, out=b["g"], epilogue=ops.make_epilogue(
            perturb_eps=0.1, rng_seed=1, adam=dict(param=b["p"], m=b["m"], v=b["v"], coef=b["coef"])))


def test_adam_matches_torch_optim():
    rng = np.random.default_rng(4)
    p0 = rng.standard_normal((1000, 64)).astype(np.float32) * 0.1
    ref = torch.nn.Parameter(torch.tensor(p0)); opt = torch.optim.Adam([ref], lr=1e-3)
    p, m, v = torch.tensor(p0, device=DEV), torch.zeros(1000, 64, device=DEV), torch.zeros(1000, 64, device=DEV)
    step_dev = torch.zeros(1, dtype=torch.int64, device=DEV)
    for step in range(1, 6):
        g = (rng.standard_normal((1000, 64)) * 10 ** rng.uniform(-6, 0)).astype(np.float32)
        ref.grad = torch.tensor(g); opt.step()
        step_dev += 1
        if step % 2:
            ops.adam_step(p, torch.tensor(g, device=DEV), m, v, step=step, lr=1e-3)
        else:
            ops.adam_step(p, torch.tensor(g, device=DEV), m, v, step_dev=step_dev, lr=1e-3)
        assert rel_err(p.cpu().numpy(), ref.detach().numpy()) < 1e-6
    pn, mn, vn = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)   # numpy oracle agrees too
    O.adam_step(pn, g, mn, vn, 1, 1e-3)
    assert np.isfinite(pn).all()


# ------------------------------------------------------------------------------------------
# (a-10/a-11) scoring GEMM, mask, top-K
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,d", [(1, 33, 64), (70, 1000, 64), (257, 4099, 128), (64, 96, 32), (100, 777, 256)])
def test_gemm_nt_is_exact_f32(m, n, d):
    rng = np.random.default_rng(m + n)
    a = rng.standard_normal((m, d)).astype(np.float32)
    b = rng.standard_normal((n, d)).astype(np.float32)        # asymmetric operands: catches transposes
    got = ops.gemm_nt(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)).cpu().numpy()
    want = a.astype(np.float64) @ b.astype(np.float64).T
    assert got.shape == (m, n) and rel_err(got, want) < 2e-6


def test_topk_rows_order_ties_and_fallback():
    rng = np.random.default_rng(8)
    x = rng.standard_normal((37, 5003)).astype(np.float32)
    x[3, :] = 1.0                                  # all equal: lowest ids win (tie fallback path)
    x[4, ::2] = 7.0                                # 2502 ties for the top: overflows the candidate list
    x[5, 100:130] = -10e8                          # masked block
    ids, sc = ops.topk_rows(torch.from_numpy(x).to(DEV), 20)
    ids, sc = ids.cpu().numpy(), sc.cpu().numpy()
    for r in range(x.shape[0]):
        order = np.lexsort((np.arange(x.shape[1]), -x[r]))[:20]
        assert np.array_equal(ids[r], order), r
        assert np.array_equal(sc[r], x[r][order])


@pytest.mark.parametrize("name", ["MF", "LightGCN", "XSimGCL", "SimGCL", "SGL"])
def test_full_rank_eval_matches_reference(golden_models, tiny_data, name):
    gm, d = golden_models, tiny_data
    ue = torch.from_numpy(gm[f"{name}_final_user"]).to(DEV)
    ie = torch.from_numpy(gm[f"{name}_final_item"]).to(DEV)
    g = d.device_graph()
    users = torch.from_numpy(gm[f"{name}_test_users"]).to(DEV)
    ids, sc = ops.score_mask_topk(ue, users, ie, g.r_indptr, g.r_indices, 20)
    want_ids, want_sc = gm[f"{name}_rec_ids"], gm[f"{name}_rec_scores"]
    ids, sc = ids.cpu().numpy(), sc.cpu().numpy()
    np.testing.assert_allclose(sc, want_sc, rtol=1e-5, atol=1e-7)
    # ids identical except where two neighbouring scores differ by less than fp32 summation noise
    bad = ids != want_ids
    if bad.any():
        gaps = np.abs(np.diff(want_sc, axis=1))
        near = np.zeros_like(bad); near[:, :-1] |= gaps < 1e-6; near[:, 1:] |= gaps < 1e-6
        assert not (bad & ~near).any()


def test_metric_rows_equals_the_host_loops():
    """srh_metric_rows: per-user hits and DCG / IDCG at several cut-offs from the hit flags -- bit-identical to the python
    loops of util/evaluation.py:7-16,66-78 (float64 adds in position order, python's own gain / ideal tables)."""
    import math
    rng = np.random.default_rng(5)
    U, K = 3000, 20
    flags = (rng.random((U, K)) < 0.07).astype(np.uint8)
    flags[3] = 1; flags[4] = 0
    sizes = rng.integers(1, 40, U).astype(np.int32)
    cuts = [5, 10, 20]
    hits, ndcg = ops.metric_rows(torch.from_numpy(flags).to(DEV), torch.from_numpy(sizes).to(DEV), cuts)
    for c, n in enumerate(cuts):
        want_h, want_n = np.zeros(U, dtype=np.int64), np.zeros(U)
        for u in range(U):
            gain = sum(1.0 / math.log(pos + 2, 2) for pos in range(n) if flags[u, pos])
            ideal = sum(1.0 / math.log(pos + 2, 2) for pos in range(min(int(sizes[u]), n)))
            want_h[u], want_n[u] = int(flags[u, :n].sum()), gain / ideal
        assert np.array_equal(hits[c].cpu().numpy(), want_h)
        assert np.array_equal(ndcg[c].cpu().numpy(), want_n)          # bit for bit
