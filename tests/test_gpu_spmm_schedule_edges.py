"""csrc/spmm.hip at every schedule and tail edge, per element against tests/spmm_ref.py.

The structures are tests/spmm_cases.py's (tests/test_spmm_cases_cpu.py shows that they hold the row, piece, tail-round and
live-count edges they are named for).  Every launch writes into outputs pre-filled with the sentinel 7.0, runs twice and
must repeat bit for bit, and every output element is held by spmm_ref.epilogue_ref's own bound through
spmm_ref.violations (BOUND_FACTOR * bound + ABS_FLOOR): no tolerance is set here.  Every test prints its worst
|error| / allowed."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from selfrec_amd import ops

from . import spmm_cases as K
from . import spmm_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = 7.0
STAMP = 17
SPLITS = pytest.mark.parametrize("split_len", [64, 0], ids=["split-64", "split-default"])
ADAM_HYPER = tuple(float(np.float32(c)) for c in (1e-3, 0.9, 0.999, 1e-8))       # lr, beta1, beta2, eps as the C ABI carries them
# The one ADAM launch of this file.  alpha = 1 / 32: one row in eleven of the ladder has 500 and more entries, and the float64
# bound of such a row's gradient is wider than 1e-3 of an update the product dominates (ill-conditioned fraction 2.9 % at
# alpha = 1 / 4, 0.4 - 0.6 % here; tests/test_spmm_cases_cpu.py asserts the cap).  A dropped entry of a short row still moves
# m by about a thousand times bound_m.
ADAM_CASE = dict(step=7, alpha=0.03125, n_add=2, add_scale=[0.25, 1.0], scale_in=True, add_rowscale=[False, True],
                 add_sparse=[True, True], n_clear=2)
AXPY = dict(alpha=0.5, add_scale=[0.3, -2.0])
ROWS_G = {8: 8, 16: 16, 32: 8, 64: 4, 128: 2, 256: 1}                             # short rows per wave at each width


def _t32(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(DEV)


def _mark32(live):
    """live entries carry (int32) stamp; the dead ones a mix of other values, 0 and stamp + 2^16 among them"""
    dead = np.array([16, 0, STAMP + (1 << 16), -STAMP], dtype=np.int32)[np.arange(live.size) % 4]
    return torch.from_numpy(np.where(live, np.int32(STAMP), dead).astype(np.int32)).to(DEV)


def _stamp():
    return torch.tensor([STAMP], dtype=torch.int64, device=DEV)


def _csr(case, split_len=0, **kw):
    """the case's raw arrays (unsorted rows) straight into a DeviceCSR"""
    return ops.DeviceCSR(np.array(case.indptr), np.array(case.indices), np.array(case.vals), case.shape, split_len=split_len, **kw)


class Tally:
    """the worst |error| / allowed of a test, printed at its end"""

    def __init__(self, name):
        self.name, self.worst, self.where, self.launches = name, 0.0, "-", 0

    def held(self, what, launch, want, bound, exact_rows=None):
        """launch() -> tensor: twice, bit-equal, within the bound; exact_rows: rows that must equal `want` exactly"""
        got, again = launch(), launch()
        assert torch.equal(got, again), f"{what}: two launches differ"
        self.check(what, got, want, bound)
        if exact_rows is not None:
            assert np.array_equal(got.cpu().numpy()[exact_rows], np.asarray(want)[exact_rows].astype(np.float32)), what
        return got

    def check(self, what, got, want, bound):
        g = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
        bad, worst = R.violations(g, want, bound)
        assert bad == 0, f"{what}: {worst}"
        frac = float(np.max(np.abs(g.astype(np.float64) - want) / (R.BOUND_FACTOR * bound + R.ABS_FLOOR), initial=0.0))
        self.launches += 1
        if frac > self.worst:
            self.worst, self.where = frac, what

    def report(self):
        print(f"{self.name}: {self.launches} outputs held, worst |err| / allowed = {self.worst:.3f} ({self.where})")


# ---- float64 references, computed once per (structure, width) and never modified ----------------------------------
_REFS = {}


def _env(case, d):
    key = (case.name, d)
    if key not in _REFS:
        n, n_cols = case.shape
        rng = np.random.default_rng([n, n_cols, d])
        m = case.scipy()
        x = rng.standard_normal((n_cols, d)).astype(np.float32)
        add = [rng.standard_normal((n, d)).astype(np.float32) for _ in range(2)]
        r = R.row_scale_with_zeros(m, seed=5)
        col_live = rng.random(n_cols) < 0.5
        e = dict(m=m, x=x, add=add, r=r, col_live=col_live, n=n, d=d)
        e["plain"] = R.epilogue_ref(m, x)
        e["axpy"] = R.epilogue_ref(m, x, alpha=AXPY["alpha"], add=add, add_scale=AXPY["add_scale"])
        e["cols"] = R.epilogue_ref(m, x, col_live=col_live)
        if d >= 64:
            e["pattern"] = R.epilogue_ref(m, x, vals_pattern=True)
            e["forward"] = R.epilogue_ref(m, x, vals_pattern=True, row_scale=r, scale_in=True, scale_out=True)
        for v in e.values():
            if isinstance(v, tuple):
                for a in v:
                    if a is not None:
                        a.setflags(write=False)
        _REFS[key] = e
    return _REFS[key]


def _dev(e):
    return dict(x=_t32(e["x"]), add=[_t32(a) for a in e["add"]], r=_t32(e["r"]), col_mark=_mark32(e["col_live"]))


def _out(e):
    return torch.full((e["n"], e["d"]), SENT, device=DEV)


def _masked_ref(ref, live):
    """a row-masked launch of `ref`'s flavour on sentinel outputs: dead rows keep the sentinel exactly"""
    y, by = ref[0].copy(), ref[2].copy()
    y[~live], by[~live] = SENT, 0.0
    return y, by


def _rows_structs():
    return (K.ladder(), K.mixed_small(), K.short_quads()) + K.tiny_all()


# ---- ADAM ---------------------------------------------------------------------------------------------------------
_ADAM_REFS = {}


def adam_reference(case, d):
    """-> (adam_inputs, adam_bounds, float64 gradient) of ADAM_CASE on the case (computed once)"""
    key = (case.name, d)
    if key not in _ADAM_REFS:
        c, m = ADAM_CASE, case.scipy()
        a = R.adam_inputs(m, d, seed=d + 1)
        g64, _, bg, _ = R.epilogue_ref(m, a["x"], row_scale=a["r"], scale_in=True, alpha=c["alpha"], add=a["add"],
                                       add_scale=c["add_scale"], add_rowscale=c["add_rowscale"], add_sparse=c["add_sparse"],
                                       add_live=a["add_live"])
        lr, b1, b2, eps = ADAM_HYPER
        _ADAM_REFS[key] = (a, R.adam_bounds(a["p"], a["m"], a["v"], g64, bg, c["step"], lr, b1, b2, eps), g64)
    return _ADAM_REFS[key]


def _adam_launch(csr, case, d):
    """one SRH_EPI_ADAM launch of ADAM_CASE on fresh state -> the tensors it may touch"""
    c, (a, _, _) = ADAM_CASE, adam_reference(case, d)
    lr, b1, b2, eps = ADAM_HYPER
    st = dict(p=_t32(a["p"]), m=_t32(a["m"]), v=_t32(a["v"]), y=torch.full((case.shape[0], d), SENT, device=DEV),
              add=[_t32(t) for t in a["add"]], cursor=torch.tensor([3, c["step"]], dtype=torch.int64, device=DEV))
    coef = torch.tensor([lr / (1.0 - b1 ** c["step"]), (1.0 - b2 ** c["step"]) ** 0.5], dtype=torch.float32, device=DEV)
    mark = _mark32(a["add_live"])
    adam = dict(param=st["p"], m=st["m"], v=st["v"], coef=coef, beta1=b1, beta2=b2, eps=eps, clear=st["add"][:c["n_clear"]],
                clear_mark=mark, cursor=st["cursor"])
    ep = ops.make_epilogue(add=st["add"], add_scale=c["add_scale"], alpha=c["alpha"], adam=adam, row_scale=_t32(a["r"]),
                           scale_in=True, add_rowscale=c["add_rowscale"], mark_stamp=_stamp(), add_mark=mark,
                           add_sparse=c["add_sparse"])
    ops.spmm(csr, _t32(a["x"]), out=st["y"], epilogue=ep)
    torch.cuda.synchronize()
    return st


def _check_adam(tally, csr, case, d, what, cap=True):
    """the checks of test_spmm_adam_epilogue_matches_float64_adam on ADAM_CASE -> the first launch's state"""
    a, w, g64 = adam_reference(case, d)
    st, st2 = _adam_launch(csr, case, d), _adam_launch(csr, case, d)
    for k in ("p", "m", "v", "cursor"):
        assert torch.equal(st[k], st2[k]), f"{what}: two launches differ in {k}"
    if cap:
        assert float(w["ill"].mean()) < 0.01, what
    for k in ("m", "v"):
        tally.check(f"{what} {k}", st[k], w[k], w["bound_" + k])
    p = st["p"].cpu().numpy().astype(np.float64)
    out = ~((p >= w["p_lo"]) & (p <= w["p_hi"]))
    i = np.unravel_index(int(np.argmax(np.maximum(w["p_lo"] - p, p - w["p_hi"]))), p.shape)
    assert not out.any(), f"{what} p: {int(out.sum())} outside the hull; at {i}: {p[i]!r} not in [{w['p_lo'][i]!r}, {w['p_hi'][i]!r}]"
    e = a["empty"]
    assert np.all(g64[e] == 0) and np.array_equal(st["p"].cpu().numpy()[e], a["p"][e]), what
    assert np.all(st["m"].cpu().numpy()[e] == 0) and np.all(st["v"].cpu().numpy()[e] == 0), what
    assert float((st["y"] - SENT).abs().max()) == 0, f"{what}: d_y was written"
    assert st["cursor"].tolist() == [4, ADAM_CASE["step"] + 1], f"{what}: the cursor moves once"
    live = a["add_live"]
    for k, t in enumerate(st["add"]):
        got = t.cpu().numpy()
        assert np.all(got[live] == 0) and np.array_equal(got[~live], a["add"][k][~live]), f"{what}: cleared table {k}"
    return st


# ---- the rows kernel ------------------------------------------------------------------------------------------------
@SPLITS
@pytest.mark.parametrize("d", [64, 128, 256])
def test_rows_kernel_flavours_on_every_structure(d, split_len):
    """spmm_rows_kernel's plain, pattern, forward (pattern, SCALE_IN | SCALE_OUT), AXPY, row-masked (late prefetch at
    d = 64) and ADAM flavours on the ladder, mixed_small, short_quads and every tiny structure, the ones without a stored
    entry among them.  Three row masks (spmm_cases.row_masks) make every wave of short rows once all dead, once all live
    and once one live row; split rows are dead under one mask and live under the others.  On the one plan object the order
    is plain -> row-masked -> ... -> plain, and the two plain results are bit-equal: a skipped split row leaves its ticket
    armed."""
    tally = Tally(f"rows d={d} split={split_len}")
    for case in _rows_structs():
        e, what = _env(case, d), f"{case.name} d={d} split={split_len}"
        T, csr = _dev(e), _csr(case, split_len)

        def run(pattern=False, **kw):
            y = _out(e)
            ops.spmm(csr, T["x"], out=y, pattern=pattern, epilogue=ops.make_epilogue(**kw) if kw else None)
            return y
        first = tally.held(f"{what} plain", run, e["plain"][0], e["plain"][2])
        for t, live in enumerate(K.row_masks(case, split_len, ROWS_G[d])):
            y64, by = _masked_ref(e["plain"], live)
            mark = _mark32(live)
            tally.held(f"{what} row-mask {t}", lambda: run(row_mark=mark, mark_stamp=_stamp()), y64, by, exact_rows=~live)
            assert torch.equal(run(), first), f"{what}: plain after row-mask {t} differs from plain before"
        tally.held(f"{what} pattern", lambda: run(pattern=True), e["pattern"][0], e["pattern"][2])
        tally.held(f"{what} forward", lambda: run(pattern=True, row_scale=T["r"], scale_in=True, scale_out=True),
                   e["forward"][0], e["forward"][2])
        tally.held(f"{what} axpy", lambda: run(add=T["add"], **AXPY), e["axpy"][0], e["axpy"][2])
        if case.indices.size == 0:            # no stored entry: zero rows, the addends still added
            assert not first.any()
            s0, s1 = (float(np.float32(sc)) for sc in AXPY["add_scale"])
            assert np.array_equal(e["axpy"][0], s0 * e["add"][0].astype(np.float64) + s1 * e["add"][1].astype(np.float64))
        _check_adam(tally, csr, case, d, f"{what} adam", cap=case.shape[0] > 5)
        assert torch.equal(run(), first), f"{what}: plain after every other flavour differs from plain before"
    tally.report()


@SPLITS
@pytest.mark.parametrize("d", [64, 128, 256])
def test_column_masked_rows_kernel_on_prescribed_live_counts(d, split_len):
    """The column-masked flavour (gather16_compact: 4, 8, 12 or 16 rounds by the fullest block's live count) on
    live_block_case -- every block of 16 stored positions holds a prescribed number of live entries, 13 and 16 among them,
    first, last or interleaved, and x is non-zero on the dead columns, so a dead entry gathered or a live one dropped moves
    its row by one term -- and on the ladder, mixed_small and the tiny structures under a 50 % mask."""
    tally = Tally(f"column-masked d={d} split={split_len}")
    lc = K.live_block_case(d)
    cases = [(lc.case, lc.col_live)] + [(c, None) for c in (K.ladder(), K.mixed_small()) + K.tiny_all()]
    for case, col_live in cases:
        e = _env(case, d)
        ref = e["cols"] if col_live is None else R.epilogue_ref(e["m"], e["x"], col_live=col_live)
        live = e["col_live"] if col_live is None else col_live
        assert np.abs(e["x"][~live]).min() > 0
        x, mark, csr = _t32(e["x"]), _mark32(live), _csr(case, split_len)

        def run():
            y = _out(e)
            ops.spmm(csr, x, out=y, epilogue=ops.make_epilogue(col_mark=mark, mark_stamp=_stamp()))
            return y
        tally.held(f"{case.name} d={d} split={split_len} column-masked", run, ref[0], ref[2])
    tally.report()


# ---- the thin kernels -----------------------------------------------------------------------------------------------
@SPLITS
@pytest.mark.parametrize("d", [8, 16, 32])
def test_thin_kernels_on_every_structure(d, split_len):
    """spmm_pair_kernel (d = 8) and spmm_slice_kernel<4 | 8> (d = 16 / 32): plain, row-masked (the three masks at 8 or 16
    short rows per wave) and column-masked launches on the ladder, mixed_small, short_quads, the tiny structures and
    live_block_case."""
    tally = Tally(f"thin d={d} split={split_len}")
    lc = K.live_block_case(d)
    for case in _rows_structs() + (lc.case,):
        e, what = _env(case, d), f"{case.name} d={d} split={split_len}"
        T, csr = _dev(e), _csr(case, split_len)
        col_live = lc.col_live if case is lc.case else e["col_live"]
        cols = e["cols"] if case is not lc.case else R.epilogue_ref(e["m"], e["x"], col_live=col_live)
        col_mark = _mark32(col_live)

        def run(**kw):
            y = _out(e)
            ops.spmm(csr, T["x"], out=y, epilogue=ops.make_epilogue(**kw) if kw else None)
            return y
        first = tally.held(f"{what} plain", run, e["plain"][0], e["plain"][2])
        for t, live in enumerate(K.row_masks(case, split_len, ROWS_G[d])):
            y64, by = _masked_ref(e["plain"], live)
            mark = _mark32(live)
            tally.held(f"{what} row-mask {t}", lambda: run(row_mark=mark, mark_stamp=_stamp()), y64, by, exact_rows=~live)
        tally.held(f"{what} column-masked", lambda: run(col_mark=col_mark, mark_stamp=_stamp()), cols[0], cols[2])
        assert torch.equal(run(), first), f"{what}: plain after the masked launches differs from plain before"
    tally.report()


# ---- row and column classes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 128])
def test_class_plans_at_the_edges_of_row_mid_and_xcd_split_row(d):
    """Every spmm_cases.class_cases() plan (split_len 64): row_mid with mid = 0, len, 1 and len - 1 and a row whose parts
    are cut into 1 + 3 pieces; every row whole in class 1, so that class 0's workgroups help the other list from the start;
    -1 and -2 mixed; each with xcd_split_row in {0, 1, n / 2, n - 1, n} -- plain and column-masked, by the bound (the parts
    of a row are summed in another order).  Plans that differ ONLY in xcd_split_row hold the same segments in the same
    in-row order: their products are bit-equal."""
    tally = Tally(f"classes d={d}")
    for cc in K.class_cases():
        e, what = _env(cc.case, d), f"{cc.name} d={d}"
        T = _dev(e)
        csr = _csr(cc.case, 64, xcd_split_row=cc.xcd_split_row, row_mid=np.array(cc.row_mid))

        def run(**kw):
            y = _out(e)
            ops.spmm(csr, T["x"], out=y, epilogue=ops.make_epilogue(**kw) if kw else None)
            return y
        tally.held(f"{what} plain", run, e["plain"][0], e["plain"][2])
        tally.held(f"{what} column-masked", lambda: run(col_mark=T["col_mark"], mark_stamp=_stamp()), e["cols"][0], e["cols"][2])
    base = K.ladder()
    e = _env(base, d)
    T, n = _dev(e), base.shape[0]
    for split_len in (64, 0):
        outs = []
        for split_row in (0, 1, n // 2, n - 1, n):
            csr = _csr(base, split_len, xcd_split_row=split_row)
            for kw in ({}, dict(col_mark=T["col_mark"], mark_stamp=_stamp())):
                y = _out(e)
                ops.spmm(csr, T["x"], out=y, epilogue=ops.make_epilogue(**kw) if kw else None)
                outs.append(y)
        for k in range(2, len(outs)):
            assert torch.equal(outs[k], outs[k % 2]), f"d={d} split={split_len}: xcd_split_row changed the bits ({k})"
        tally.check(f"ladder xcd_split_row d={d} split={split_len}", outs[-2], e["plain"][0], e["plain"][2])
    tally.report()


# ---- XCD shares -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 128])
def test_xcd_shares_with_zeros_keep_every_flavours_bits(d):
    """srh_spmm_plan_set_xcd_shares on the ladder's split-64 plan with shares of 0: every workgroup on XCD 3 (seven queues
    of empty records), and XCD 0 given nothing (wave 0 is an empty record).  The plain, pattern, row-masked, column-masked
    and ADAM launches -- whose wave 0 moves the cursor, once -- equal the canonical list's bits; NULL restores the list."""
    case = K.ladder()
    e = _env(case, d)
    T, csr = _dev(e), _csr(case, 64)
    tally = Tally(f"xcd shares d={d}")
    row_mark = _mark32(K.row_masks(case, 64, ROWS_G[d])[1])

    def flavours():
        outs = []
        for pattern, kw in ((False, {}), (True, {}), (False, dict(row_mark=row_mark, mark_stamp=_stamp())),
                            (False, dict(col_mark=T["col_mark"], mark_stamp=_stamp()))):
            y = _out(e)
            ops.spmm(csr, T["x"], out=y, pattern=pattern, epilogue=ops.make_epilogue(**kw) if kw else None)
            outs.append(y)
        st = _adam_launch(csr, case, d)
        assert st["cursor"].tolist() == [4, ADAM_CASE["step"] + 1]
        return outs + [st["p"], st["m"], st["v"]] + st["add"]
    canon = flavours()
    tally.check("canonical plain", canon[0], e["plain"][0], e["plain"][2])
    tally.check("canonical pattern", canon[1], e["pattern"][0], e["pattern"][2])
    tally.check("canonical column-masked", canon[3], e["cols"][0], e["cols"][2])
    _check_adam(tally, csr, case, d, f"canonical adam d={d}")
    n_canon = ops.spmm_plan_run_tasks(csr, d)
    nb = (n_canon + 3) // 4
    rest = [nb // 7 + (1 if k < nb % 7 else 0) for k in range(7)]
    for shares in ([0, 0, 0, nb, 0, 0, 0, 0], [0] + rest, [0, 0, 0, 0, 0, 0, 0, nb]):
        ops.spmm_set_xcd_shares(csr, d, np.array(shares, dtype=np.int32))
        assert ops.spmm_plan_run_tasks(csr, d) == max(shares) * 32
        for k, (got, want) in enumerate(zip(flavours(), canon)):
            assert torch.equal(got, want), f"d={d} shares {shares}: output {k} differs from the canonical list's"
    ops.spmm_set_xcd_shares(csr, d, None)
    assert ops.spmm_plan_run_tasks(csr, d) == n_canon
    for k, (got, want) in enumerate(zip(flavours(), canon)):
        assert torch.equal(got, want), f"d={d} restored list: output {k} differs"
    tally.report()


# ---- three value arrays in one traversal ----------------------------------------------------------------------------
def _spmm3_arrays(case):
    """-> {name: three value arrays}.  (a) the engine's: every value, and two copies with 30 % of the edges dropped;
    (b) zeros in array 0 where arrays 1 and 2 are not zero -- a whole row, a whole block of 16 stored positions, a fifth of
    the rest -- and a few entries zero in all three; (c) array 0 all zero."""
    rng = np.random.default_rng(case.indices.size + 7)
    v, nnz, lens = np.array(case.vals), case.indices.size, case.lens
    keep = lambda p: (rng.random(nnz) < p).astype(np.float32)      # noqa: E731
    a = [v, v * keep(0.7) * np.float32(1.5), v * keep(0.7) * np.float32(0.75)]
    z0 = keep(0.8)
    if nnz:
        r = int(np.argmax(lens >= 100)) if (lens >= 100).any() else int(np.argmax(lens))
        z0[case.indptr[r]:case.indptr[r + 1]] = 0.0                                       # a whole row
        big = int(np.argmax(lens))
        if big != r and lens[big] >= 32:
            z0[case.indptr[big] + 16:case.indptr[big] + 32] = 0.0                         # a whole block of 16
    b1, b2 = v * np.float32(1.5), -v
    none = rng.random(nnz) < 0.03
    b = [np.where(none, 0, v * z0).astype(np.float32), np.where(none, 0, b1).astype(np.float32),
         np.where(none, 0, b2 * keep(0.9)).astype(np.float32)]
    c = [np.zeros_like(v), v, v * keep(0.7)]
    if nnz >= 100:
        assert ((b[0] == 0) & (b[1] != 0) & (b[2] != 0)).sum() >= 16
    return dict(a=a, b=b, c=c)


@SPLITS
def test_spmm3_serves_three_independent_value_arrays(split_len):
    """srh_spmm3_f32 on the ladder, mixed_small, short_quads and the tiny structures: each output bit-equal to ops.spmm of
    its own array and within the float64 bound -- also where array 0 is zero and the others are not (b), and where array 0 is
    zero everywhere (c).  The kernel used to gather an x row only when array 0's value was non-zero: (b) and (c) lost those
    terms of y1 and y2."""
    d = 64
    tally = Tally(f"spmm3 split={split_len}")
    for case in _rows_structs():
        e = _env(case, d)
        x, base = _t32(e["x"]), _csr(case, split_len)
        for name, arrays in _spmm3_arrays(case).items():
            views = [base.with_values(_t32(v)) for v in arrays]

            def run():
                outs = [_out(e) for _ in range(3)]
                ops.spmm3(views, x, outs)
                return torch.stack(outs)
            got, again = run(), run()
            assert torch.equal(got, again), f"{case.name} ({name}): two launches differ"
            for k, v in enumerate(arrays):
                what = f"{case.name} split={split_len} ({name}) y{k}"
                m = sp.csr_matrix((v.astype(np.float64), np.array(case.indices), np.array(case.indptr)), shape=case.shape)
                y64, _, by, _ = R.epilogue_ref(m, e["x"])
                tally.check(what, got[k], y64, by)
                assert torch.equal(got[k], ops.spmm(views[k], x)), f"{what}: not the bits of its own launch"
    tally.report()
