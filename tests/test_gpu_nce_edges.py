"""The step's InfoNCE passes (csrc/losses.hip: nce_prep, nce_tile_f32 on nce_plan's task list, nce_tile_lds, the finish
kernels) against the float64 closed form of tests/nce_ref.py, ROW BY ROW, at the edges of the padding, the 16-row wave
tile, the 32-key block, the 128-row query block, the task list of several problems, the LDS ring, the kept-weights form
and the block budget of a task.

Every call goes through ops.infonce_multi with an explicit precision, on tables of max(n) + 200 rows with a sorted
random idx, a device-side count under a larger launch bound, gradient tables pre-filled with 1e-5 (rows nobody names
must come back bit-identical) and a workspace of 0xFF bytes (nothing promises a clean one: an unwritten slot reads NaN).

Bounds (tests/nce_ref.py): loss 2e-6 (f32) / 1e-5 (split) of float64; gradients per row, measured against the tensor's
largest row: MARGIN x ROW_YARDSTICK_NCE for f32, 2e-5 for split -- plus the rounding of the add into the 1e-5 base, half
an ulp of (base + gradient)."""
import numpy as np
import pytest
import torch

from selfrec_amd import _lib, ops
from selfrec_amd._lib import SelfrecHipError

from . import nce_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BASE = 1e-5
SCALE = 0.3


def slots():
    return torch.cuda.get_device_properties(0).multi_processor_count


def ws_bytes(n_max, d):
    return int(_lib.load().srh_infonce_ws_bytes(n_max, d))


def run(problems, n_maxes, d, tau, precision, reps=1):
    """one call per rep from the same initial state: (loss, [g1 per problem], [g2 per problem]) of the first, and every
    further rep must give the same bits"""
    tabs = [(torch.from_numpy(p["t1"]).to(DEV), torch.from_numpy(p["t2"]).to(DEV)) for p in problems]
    idx, cnt = [], []
    for p, n_max in zip(problems, n_maxes):
        ix = torch.zeros(n_max, dtype=torch.int32, device=DEV)
        ix[:p["n"]] = torch.from_numpy(p["idx"]).to(DEV)
        idx.append(ix)
        cnt.append(torch.tensor([p["n"]], dtype=torch.int32, device=DEV))
    need = sum(ws_bytes(n_max, d) for n_max in n_maxes)
    first = None
    for rep in range(reps):
        ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
        g1 = [torch.full_like(a, BASE) for a, _ in tabs]
        g2 = [torch.full_like(b, BASE) for _, b in tabs]
        loss = torch.zeros(1, dtype=torch.float64, device=DEV)
        ops.infonce_multi([(tabs[k][0], tabs[k][1], idx[k], n_maxes[k], cnt[k], g1[k], g2[k]) for k in range(len(problems))],
                          d=d, tau=tau, loss_scale=SCALE, loss=loss, ws=ws, precision=precision)
        torch.cuda.synchronize()
        if first is None:
            first = (loss, g1, g2)
        else:
            assert torch.equal(loss, first[0]), f"call {rep}: another loss than call 0"
            for k in range(len(problems)):
                assert torch.equal(g1[k], first[1][k]) and torch.equal(g2[k], first[2][k]), f"call {rep}, problem {k}: other bits"
        del ws
    return first


def measure(problems, got, tau, yard=False):
    """(loss error, [per problem: worst row error of g1, of g2, its allowance for the add into the base, the float32
    figure of the closed form when yard]) against info_nce_rows in float64 on the device; asserts the untouched rows"""
    loss, g1s, g2s = got
    want_loss, rows = 0.0, []
    for k, p in enumerate(problems):
        l64, a64, b64 = R.info_nce_rows(p["t1"], p["t2"], p["idx"], tau, SCALE, device=DEV)
        want_loss += l64
        ix = torch.from_numpy(p["idx"].astype(np.int64)).to(DEV)
        other = torch.ones(a64.shape[0], dtype=torch.bool, device=DEV)
        other[ix] = False
        base = torch.full((1,), BASE, dtype=torch.float32, device=DEV)
        errs, allow = [], 0.0
        for g, w in ((g1s[k], a64), (g2s[k], b64)):
            assert torch.isfinite(g).all(), f"problem {k}: a non-finite gradient"
            assert torch.equal(g[other], base.expand_as(g[other])), f"problem {k}: a row that idx does not name was written"
            e = R.row_errors(g[ix].double() - base.double(), w[ix], R.FLOOR_FRAC)
            errs.append((float(e.max()), int(e.argmax())))
            top = float(w.abs().max())
            allow = max(allow, 2.0 ** -24 * (1.0 + BASE / top))
        f32 = None
        if yard:
            _, a32, b32 = R.info_nce_rows(p["t1"], p["t2"], p["idx"], tau, SCALE, dtype=torch.float32, device=DEV)
            f32 = max(float(R.row_errors(a32[ix], a64[ix], R.FLOOR_FRAC).max()),
                      float(R.row_errors(b32[ix], b64[ix], R.FLOOR_FRAC).max()))
        rows.append((errs[0], errs[1], allow, f32))
    return abs(float(loss.item()) - want_loss) / abs(want_loss), rows


def check(tag, problems, got, tau, precision, yard=False):
    """the list of what is out of bounds (empty: all is well); prints every figure"""
    bad = []
    el, rows = measure(problems, got, tau, yard)
    line = f"{tag} {precision}: loss {el:.2e} (bound {R.LOSS_BOUND[precision]:.0e})"
    if not el < R.LOSS_BOUND[precision]:
        bad.append(f"{tag}: loss {el:.2e}")
    for k, ((e1, r1), (e2, r2), allow, f32) in enumerate(rows):
        bound = R.ROW_BOUND_F32 if precision == "f32" else R.ROW_BOUND_SPLIT
        if yard:
            bound = R.MARGIN * max(R.ROW_YARDSTICK_NCE, f32)
        bound += allow
        line += f"; n={problems[k]['n']}: g1 {e1:.2e} at row {r1}, g2 {e2:.2e} at row {r2} (bound {bound:.2e}" + \
                (f", float32 torch {f32:.2e})" if yard else ")")
        if not e1 < bound:
            bad.append(f"{tag} problem {k} (n={problems[k]['n']}): g1 row {r1} {e1:.2e} > {bound:.2e}")
        if not e2 < bound:
            bad.append(f"{tag} problem {k} (n={problems[k]['n']}): g2 row {r2} {e2:.2e} > {bound:.2e}")
    print(line)
    return bad


# ---- A. pad, wave, block ------------------------------------------------------------------------------------------------
A_PARAMS = [(prec, d, tau) for prec in ("f32", "split") for d in R.A_WIDTHS[prec] for tau in R.A_TAUS]


@pytest.mark.parametrize("precision,d,tau", A_PARAMS)
def test_a_pad_wave_and_block_edges(precision, d, tau):
    """n on both sides of 16, 32, 64, 128 and 192 and at 257, every one at tau = 1 -- where a zero-row pad key that was
    counted weighs e^-1, as much as a real key -- and a third of them at tau = 0.05; rows with v2_i = v1_i in the first,
    the last full and the last partial tile, identical pairs inside a tile, across two tiles of a key block and across
    two query blocks (at tau = 0.05 the pairs are left out: nce_ref.problem)."""
    bad = []
    for n in (R.A_NS if tau == 1.0 else R.A_LOW_TAU_NS):
        p = R.problem(n, d, 1000 + n + d, pairs=tau >= R.TAU_PAIRS)
        plan = R.plan((n,), slots())
        if slots() >= 30:          # (3 query blocks x 10 key blocks at n = 257) every key block a task of its own
            assert plan["per"] == [1] and plan["splits"] == plan["kb"], plan
        got = run([p], [n + 100], d, tau, precision)
        bad += check(f"A n={n} d={d} tau={tau}", [p], got, tau, precision)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("precision,d", [("f32", 64), ("f32", 128), ("split", 64), ("split", 256)])
def test_a_one_pair_is_exactly_nothing(precision, d):
    """n = 1: log_softmax of a 1 x 1 matrix -- the loss and both gradients are exactly 0"""
    p = R.problem(1, d, 999)
    loss, g1, g2 = run([p], [101], d, 1.0, precision)
    assert loss.item() == 0.0
    assert torch.equal(g1[0], torch.full_like(g1[0], BASE)) and torch.equal(g2[0], torch.full_like(g2[0], BASE))


# ---- B. several problems per call ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "split"])
@pytest.mark.parametrize("ci", range(len(R.B_CALLS)))
def test_b_several_problems_in_one_call(ci, precision):
    """up to four problems behind one another in the task list, each measured on its own, the call twice bit for bit"""
    ns, d = R.B_CALLS[ci]
    plan = R.plan(ns, slots())
    assert plan["first"][-1] == sum(q * s for q, s in zip(plan["qb"], plan["splits"])) and all(s >= 1 for s in plan["splits"])
    if ci == 0 and slots() == 256:
        assert {k: plan[k] for k in R.B_PLAN_256} == R.B_PLAN_256
    problems = R.call(ns, d, 2000 + 100 * ci)
    got = run(problems, [n + 100 for n in ns], d, R.TAU_LARGE, precision, reps=2)
    bad = check(f"B {ns} d={d}", problems, got, R.TAU_LARGE, precision)
    assert not bad, "\n".join(bad)


# ---- C. ring and reuse --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(len(R.C_CALLS)))
def test_c_streamed_ring_and_kept_weights(ci):
    """tasks of more key blocks than the ring has slots, with pass 1's weights kept (workspace rows <= 8192) and
    recomputed (above; one call mixes 8200 rows with 300, which then take the recompute form too).  Calls with more rows
    than the yardstick's cases (4160) take group D's bound: MARGIN x the larger of the constant and their own float32 figure."""
    ns, n_maxes, d = R.C_CALLS[ci]
    plan = R.plan(ns, slots())
    assert max(plan["per"]) > R.RING_SLOTS, plan
    problems = R.call(ns, d, 3000 + 100 * ci)
    got = run(problems, list(n_maxes), d, R.TAU_LARGE, "f32", reps=2)
    bad = check(f"C {ns} d={d}", problems, got, R.TAU_LARGE, "f32", yard=max(ns) > 4160)
    assert not bad, "\n".join(bad)


# ---- D. the block budget ------------------------------------------------------------------------------------------------
def d_cases():
    """(n, launch bound, d, reps): the first padded count whose unbounded cut gave a task more than kNceMaxPer blocks on
    this device and the one a padding step below it (3 rows short of the padded count each: pad keys too), then the fixed ones"""
    over = R.first_over_budget(slots())
    assert over is not None and R.plan((over,), slots())["per"][0] <= R.MAX_PER < R.plan((over,), slots(), max_per=None)["per"][0]
    assert R.plan((over - R.PAD,), slots(), max_per=None)["per"][0] <= R.MAX_PER
    return [(over - R.PAD - 3, over - R.PAD + 97, 64, 1), (over - 3, over + 97, 64, 2)] + [c + (1,) for c in R.D_FIXED]


@pytest.mark.parametrize("which", range(4))
def test_d_block_budget_of_a_task(which):
    """n above 12 288 (256 workgroups), where nce_plan used to hand out tasks of more than 128 key blocks: 12 285 and
    12 349 (d = 64), 16 384 (d = 128) and the documented limit 65 536 (d = 64; launch bound = live count, there is no
    room above it).  Reference and float32 yardstick: the closed form on the device; bound MARGIN x the larger of
    ROW_YARDSTICK_NCE and the case's own float32 figure (row sums of 1e4 .. 1e5 terms carry more float32 rounding than the
    small cases the constant was measured on)."""
    n, n_max, d, reps = d_cases()[which]
    plan = R.plan((n,), slots())
    assert plan["per"][0] <= R.MAX_PER and plan["splits"][0] <= R.SPLITS
    if which != 0:
        assert R.plan((n,), slots(), max_per=None)["per"][0] > R.MAX_PER
    p = R.problem(n, d, 4000 + which, rows=max(n_max, n + 200))
    got = run([p], [n_max], d, R.TAU_LARGE, "f32", reps=reps)
    bad = check(f"D n={n} d={d}", [p], got, R.TAU_LARGE, "f32", yard=True)
    assert not bad, "\n".join(bad)


def test_d_one_row_past_the_limit_is_refused_before_any_launch():
    n, d = R.F32_MAX_N + 1, 64
    t = torch.zeros(n, d, device=DEV)
    g = torch.full((n, d), BASE, device=DEV)
    loss = torch.zeros(1, dtype=torch.float64, device=DEV)
    ws = torch.empty(ws_bytes(n, d), dtype=torch.uint8, device=DEV)
    with pytest.raises(SelfrecHipError, match=r"\(-3\).*n <= 65536"):          # SRH_ERR_UNSUPPORTED
        ops.infonce_multi([(t, t, None, n, None, g, g)], d=d, tau=0.2, loss_scale=1.0, loss=loss, ws=ws, precision="f32")
    torch.cuda.synchronize()
    assert loss.item() == 0.0 and torch.equal(g, torch.full_like(g, BASE))


# ---- E. split-16 stage edges ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,n_max,d", R.E_CASES)
def test_e_split16_ranges_and_stages(n, n_max, d):
    """a workspace of 64 rows (six of the eight key ranges empty), every range one block (with and without live keys in
    the last one), and the first counts whose ranges need a second LDS stage at d = 64, 128 and 256; per row at 2e-5"""
    per, stages = R.split16_ranges(R.pad(n_max), d)
    assert sum(sum(s) for s in stages) == R.pad(n_max)
    p = R.problem(n, d, 5000 + n)
    got = run([p], [n_max], d, R.TAU_LARGE, "split", reps=2)
    bad = check(f"E n={n} d={d} stages {stages[0]}", [p], got, R.TAU_LARGE, "split")
    assert not bad, "\n".join(bad)


# ---- F. the fused call --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,precision", [(64, "f32"), (64, "split"), (128, "f32"), (128, "split")])
@pytest.mark.parametrize("nce_rows", [1, 2])
@pytest.mark.parametrize("mode", ["atomics", "segments", "segments-store"])
def test_f_fused_call_contrast_gradient_per_row(mode, nce_rows, d, precision):
    """ops.bpr_infonce on the planted batch exactly as test_gpu_batch.test_bpr_infonce_matches_restatement runs it; gC --
    the contrast table's gradient, InfoNCE's alone -- per row at the bound of group A, rows nobody names untouched."""
    from . import batch_ref as B
    from . import test_gpu_batch as T
    U = B.N_USERS
    case, ref = B.planted_batch(d), T.nce_reference(d, nce_rows)
    u, i, j = case["u"], case["i"], case["j"]
    uu, up = ref["uu"], ref["up"]
    batch = u.size + 24
    dF, dC = T.dev(ref["F"]), T.dev(ref["CL"])
    named_F = np.concatenate([np.unique(u), U + np.union1d(i, j)])
    named_C = np.concatenate([uu, U + up])
    init = {"gF": T.initial(mode, ref["gF"], named_F), "gC": T.initial(mode, ref["gC"], named_C)}
    cnt = lambda n: torch.tensor([n], dtype=torch.int32, device=DEV)
    gF, gC = T.dev(init["gF"]), T.dev(init["gC"])
    losses = torch.zeros(3, dtype=torch.float64, device=DEV)
    if nce_rows == 1:
        tabs = (dF[:U], dF[U:]) * 2
        grads = dict(g_user=gF[:U], g_item=gF[U:], greg_user=gF[:U], greg_item=gF[U:])
        problems = [(dF[:U], dC[:U], T.i32(uu, batch), batch, cnt(uu.size), gF[:U], gC[:U]),
                    (dF[U:], dC[U:], T.i32(up, batch), batch, cnt(up.size), gF[U:], gC[U:])]
        io = 0
    else:
        tabs = (dF,) * 4
        grads = dict(g_user=gF, g_item=gF, greg_user=gF, greg_item=gF)
        problems = [(dF, dC, T.i32(np.concatenate([uu, U + up]), 2 * batch), 2 * batch, cnt(uu.size + up.size), gF, gC)]
        io = U
    kw = dict(seg=T.seg_dev(u, i, j, batch, mode, io), nce_rows=nce_rows) if mode != "atomics" else {}
    nce_ws = torch.full((sum(ws_bytes(p[3], d) for p in problems),), 0xFF, dtype=torch.uint8, device=DEV)
    ops.bpr_infonce(*tabs, T.i32(u, batch), T.i32(i + io, batch), T.i32(j + io, batch), batch=batch, n_rows_dev=cnt(u.size),
                    reg_coef=1e-4, reg_include_neg=False, loss_scale=1.0, losses=losses[0:2], bpr_ws=ops.bpr_ws(batch, DEV),
                    problems=problems, tau=ref["tau"], cl_scale=ref["cl_rate"], cl_loss=losses[2:3], nce_ws=nce_ws,
                    precision=precision, **grads, **kw)
    got = T.delta(mode, gC, init["gC"], named_C, "gC")              # (asserts the rows nobody names)
    want = ref["gC"]
    el = abs(losses[2].item() - ref["losses"][2]) / abs(ref["losses"][2])
    bound = R.ROW_BOUND_F32 if precision == "f32" else R.ROW_BOUND_SPLIT
    if mode != "segments-store":      # the add into the base: half an ulp of (base + gradient)
        bound += 2.0 ** -24 * (1.0 + float(np.abs(init["gC"][named_C]).max()) / float(np.abs(want).max()))
    # the two problems of nce_rows = 1 are measured apart: each against its own largest row
    groups = [uu, U + up] if nce_rows == 1 else [named_C]
    errs = [R.row_errors(got[g], want[g], R.FLOOR_FRAC) for g in groups]
    worst = max(float(e.max()) for e in errs)
    print(f"F {mode} nce_rows={nce_rows} d={d} {precision}: cl loss {el:.2e} (bound {R.LOSS_BOUND[precision]:.0e}), "
          f"gC per row {worst:.2e} (bound {bound:.2e})")
    assert el < R.LOSS_BOUND[precision]
    assert worst < bound
