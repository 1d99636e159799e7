"""The kernels every training step of a graph model ends in -- bpr_phase1, bpr_phase2 / rows_finish (csrc/losses.hip), adam_kernel
with and without the fused row clear, zero_rows, axpby, cursor_advance (csrc/optim.hip) -- against the float64 restatement in
tests/batch_ref.py, on its planted cases: slot lists of 1, 7, 8, 9, 16, 17, 40 entries, mixed roles in one list, an i == j
triple, logits at the 10e-6 floor and past both saturation points, batches of 1..5 rows, rows that nobody names.

Bounds (tests/batch_ref.py): whole tensors as the older direct test has them (2e-6 losses, 2e-5 gradients); per row
and per Adam element four times what f32 torch on the CPU gives for the same expressions (tests/test_batch_ref_cpu.py)."""
import functools

import numpy as np
import pytest
import torch

from oracle import selfrec_oracle as O
from selfrec_amd import ops
from selfrec_amd._lib import SelfrecHipError

from . import batch_ref as R
from .conftest import host_batch_segments

pytestmark = pytest.mark.gpu
DEV = "cuda"
U, I = R.N_USERS, R.N_ITEMS
MODES = ["atomics", "segments", "segments-store"]
SENTINEL = np.array([0x7FC0BEEF], dtype=np.uint32).view(np.float32)[0]        # a NaN with a payload: any arithmetic on it shows


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def i32(a, n):
    out = np.zeros(n, dtype=np.int32)
    out[:len(a)] = a
    return dev(out)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def base_of(want):
    """a non-zero starting content for a gradient table that is added into.  Per row 1/64 .. 1/8 of the largest value the call
    is to add there (a power of two times 1..4: the sum's rounding stays that of the terms, yet a store in place of an add
    is thousands of times the per-row bound); 2^-17 .. 2^-15 where nothing is to be added."""
    top = np.abs(want).max(1)
    unit = np.where(top > 0, 2.0 ** (np.floor(np.log2(np.where(top > 0, top, 1.0))) - 5), 2.0 ** -17)
    r, c = np.meshgrid(np.arange(want.shape[0]), np.arange(want.shape[1]), indexing="ij")
    return (unit[:, None] * (1 + (3 * r + c) % 4)).astype(np.float32)


def initial(mode, want, named):
    """add modes: the base everywhere.  Store mode: zero on the rows the batch names (the caller's guarantee), the sentinel on
    every other row."""
    if mode != "segments-store":
        return base_of(want)
    t = np.full(want.shape, SENTINEL, dtype=np.float32)
    t[named] = 0.0
    return t


def delta(mode, got, init, named, what):
    """what the call added, in float64; every row the batch does not name must come back bit-identical"""
    got = got.detach().cpu().numpy()
    other = np.ones(got.shape[0], dtype=bool)
    other[named] = False
    assert np.array_equal(got[other].view(np.int32), init[other].view(np.int32)), f"{what}: a row that no slot names was written"
    out = np.zeros(got.shape, dtype=np.float64)
    out[named] = got[named].astype(np.float64) - (0.0 if mode == "segments-store" else init[named].astype(np.float64))
    return out


def seg_dev(u, i, j, pad, mode, item_row0=0):
    seg = {k: dev(v) for k, v in host_batch_segments(u, i, j, pad, 0, item_row0).items()}
    seg["rows_are_zero"] = mode == "segments-store"
    return seg


@functools.lru_cache(maxsize=None)
def reference(kind, d, family, include_neg, ego, seed=0):
    return R.reference(R.batch_case(kind, d, family, seed), include_neg, ego)


def wanted(ref, ego):
    """the four gradient tables the call is to produce (the regulariser's in the embedding's own where they alias)"""
    if ego:
        return {k: ref[k] for k in ("g_user", "g_item", "greg_user", "greg_item")}
    return {"g_user": ref["g_user"] + ref["greg_user"], "g_item": ref["g_item"] + ref["greg_item"]}


def run_bpr(case, ref, mode, include_neg, ego, batch, *, one_table=False, seg=None, reps=1):
    """One srh_bpr_l2_fwd_bwd[_p] call on the case.  Returns the losses, what was added to each gradient table (float64, user
    and item parts apart) and the raw bits of every output; `reps` calls from the same initial state must give the same bits."""
    u, i, j, d = case["u"], case["i"], case["j"], case["d"]
    B, io = u.size, (U if one_table else 0)
    named_u, named_i = np.unique(u), np.union1d(i, j)
    want = wanted(ref, ego)
    if one_table:
        named = np.concatenate([named_u, U + named_i])
        du = di = dev(np.concatenate([case["user"], case["item"]]))
        dru = dri = dev(np.concatenate([case["ego_user"], case["ego_item"]])) if ego else du
        init = {"g": initial(mode, np.concatenate([want["g_user"], want["g_item"]]), named)}
        if ego:
            init["greg"] = initial(mode, np.concatenate([want["greg_user"], want["greg_item"]]), named)
        names = {"g_user": "g", "g_item": "g", "greg_user": "greg" if ego else "g", "greg_item": "greg" if ego else "g"}
        rows_of = {"g": named, "greg": named}
    else:
        du, di = dev(case["user"]), dev(case["item"])
        dru, dri = (dev(case["ego_user"]), dev(case["ego_item"])) if ego else (du, di)
        init = {k: initial(mode, w, named_u if k.endswith("user") else named_i) for k, w in want.items()}
        names = {k: (k if ego or not k.startswith("greg") else k.replace("greg", "g"))
                 for k in ("g_user", "g_item", "greg_user", "greg_item")}
        rows_of = {"g_user": named_u, "g_item": named_i, "greg_user": named_u, "greg_item": named_i}
    if seg is None and mode != "atomics":
        seg = seg_dev(u, i, j, batch, mode, io)
    kw = dict(seg=seg) if mode != "atomics" else {}
    idx = [i32(u, batch), i32(i + io, batch), i32(j + io, batch)]
    cnt = torch.tensor([B], dtype=torch.int32, device=DEV)
    ws = ops.bpr_ws(batch, DEV)
    first = None
    for rep in range(reps):
        tabs = {k: dev(v) for k, v in init.items()}
        losses = torch.zeros(2, dtype=torch.float64, device=DEV)
        ops.bpr_l2_fwd_bwd(du, di, dru, dri, *idx, batch=batch, n_rows_dev=cnt, reg_coef=R.REG_COEF, reg_include_neg=include_neg,
                           loss_scale=R.LOSS_SCALE, losses=losses, ws=ws, **{k: tabs[t] for k, t in names.items()}, **kw)
        raw = {k: bits(t) for k, t in tabs.items()}
        raw["losses"] = losses.cpu().numpy().view(np.int64)
        if first is None:
            first = raw
            out = {"losses": losses.cpu().numpy(), "raw": raw}
            for k, t in tabs.items():
                out[k] = delta(mode, t, init[k], rows_of[k], k)
        else:
            assert all(np.array_equal(first[k], raw[k]) for k in first), f"call {rep} gave other bits than call 0"
    if one_table:
        halves = {"g_user": out["g"][:U], "g_item": out["g"][U:]}
        if ego:
            halves.update(greg_user=out["greg"][:U], greg_item=out["greg"][U:])
        out.update(halves)
    return out


def check_bpr(out, ref, ego, tag):
    """losses and gradients of one call against the restatement: whole-tensor and per-row bounds; prints what was achieved"""
    el = [abs(out["losses"][0] - ref["bpr"]) / abs(ref["bpr"]), abs(out["losses"][1] - ref["reg"]) / abs(ref["reg"])]
    want = wanted(ref, ego)
    if ego:
        scale = {"g_user": ref["s_user"], "g_item": ref["s_item"], "greg_user": ref["sreg_user"], "greg_item": ref["sreg_item"]}
    else:
        scale = {"g_user": ref["s_user"] + ref["sreg_user"], "g_item": ref["s_item"] + ref["sreg_item"]}
    pairs = [(out[k], want[k], scale[k]) for k in want]
    whole = max(R.rel_err(g, w) for g, w, _ in pairs)
    row = max(R.row_error(g, w, s) for g, w, s in pairs)
    print(f"{tag}: losses {el[0]:.2e} {el[1]:.2e} (bound {R.LOSS_BOUND:.0e}); gradients {whole:.2e} of the tensor "
          f"(bound {R.GRAD_BOUND:.0e}), {row:.2e} of the row (bound {R.ROW_BOUND:.1e})")
    assert max(el) < R.LOSS_BOUND, tag
    assert whole < R.GRAD_BOUND, tag
    assert row < R.ROW_BOUND, tag


# ---------------------------------------------------------------------------------------------------------------------------
# BPR / L2: three finishes x four widths x logit families, planted and tiny batches
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("d", R.WIDTHS)
@pytest.mark.parametrize("mode", MODES)
def test_bpr_l2_matches_restatement(mode, d, family):
    """Every configuration (regulariser on the embedding tables themselves or on separate ego tables with gradient tables of
    their own, negatives in it or not), with the launch bound equal to the device-side count and 24 above it (3 x 203 and
    3 x 227 row groups: a multiple of no workgroup's share, so the last workgroup has dead groups at every width)."""
    for kind in ("planted",) + R.TINY:
        case = R.batch_case(kind, d, family)
        B = case["u"].size
        for include_neg, ego in R.CONFIGS:
            for batch in (B, B + 24):
                ref = reference(kind, d, family, include_neg, ego)
                out = run_bpr(case, ref, mode, include_neg, ego, batch, reps=1 if mode == "atomics" else 3)
                check_bpr(out, ref, ego,
                          f"{mode} d={d} {family} {kind} neg={include_neg} ego={ego} batch={batch}")
                if kind == "planted" and ego and mode != "atomics":
                    # the i == j triple: c (p - n) with p, n the same row -- exactly nothing for its user, who has no other slot
                    lone = case["u"][case["twin_slot"]]
                    assert not out["g_user"][lone].any()


@pytest.mark.parametrize("d", R.WIDTHS)
@pytest.mark.parametrize("mode", MODES[1:])
def test_one_table_form_gives_the_two_table_bits(mode, d):
    """users and items as rows [0, U) and [U, U + I) of ONE table passed for both, item ids and the lists' item rows offset by U
    (user_row0 / item_row0): the same bits as the two-table call, and the restatement's values."""
    for kind, family in (("planted", "mixed"), ("planted", "ordinary"), (3, "floor")):
        case = R.batch_case(kind, d, family)
        batch = case["u"].size + 24
        for include_neg, ego in R.CONFIGS:
            ref = reference(kind, d, family, include_neg, ego)
            two = run_bpr(case, ref, mode, include_neg, ego, batch)
            one = run_bpr(case, ref, mode, include_neg, ego, batch, one_table=True, reps=3)
            check_bpr(one, ref, ego, f"one table {mode} d={d} {family} {kind}")
            assert np.array_equal(one["raw"]["losses"], two["raw"]["losses"])
            for t in ("g", "greg") if ego else ("g",):
                assert np.array_equal(one["raw"][t][:U], two["raw"][t + "_user"])
                assert np.array_equal(one["raw"][t][U:], two["raw"][t + "_item"])


@pytest.mark.parametrize("d", R.WIDTHS)
@pytest.mark.parametrize("mode", MODES[1:])
def test_epoch_arrays_give_the_stand_alone_bits(mode, d):
    """d_batch_no: the segment arrays of three different batches back to back (3 B / B entries per batch, B the launch bound),
    the batch chosen on the device."""
    cases = [R.planted_batch(d, seed, "mixed") for seed in (0, 1, 2)]
    batch = R.PLANTED_B + 24
    segs = [host_batch_segments(c["u"], c["i"], c["j"], batch) for c in cases]
    epoch = {k: dev(np.concatenate([s[k] for s in segs])) for k in ("seg_rows", "seg_end", "seg", "seg_a", "seg_b", "n_uniq_n")}
    for b in (0, 2):
        seg = dict(epoch, n_uniq_u=dev(segs[b]["n_uniq_u"]), n_uniq_i=dev(segs[b]["n_uniq_i"]),
                   batch_no=torch.tensor([b], dtype=torch.int32, device=DEV), rows_are_zero=mode == "segments-store")
        for include_neg, ego in ((True, True), (False, False)):
            ref = reference("planted", d, "mixed", include_neg, ego, seed=b)
            alone = run_bpr(cases[b], ref, mode, include_neg, ego, batch)
            got = run_bpr(cases[b], ref, mode, include_neg, ego, batch, seg=seg, reps=3)
            check_bpr(got, ref, ego, f"epoch arrays {mode} d={d} batch {b}")
            assert all(np.array_equal(alone["raw"][k], got["raw"][k]) for k in alone["raw"])


# ---------------------------------------------------------------------------------------------------------------------------
# with InfoNCE in the call
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def nce_reference(d, nce_rows):
    """batch_ref.bpr_l2 of the planted batch plus cl_rate * InfoNCE (float64 autograd on the oracle's info_nce): nce_rows = 1 two
    problems (unique users; unique positive items), 2 one problem over [users ; positive items]"""
    case = R.planted_batch(d)
    rng = np.random.default_rng(d)
    F = np.concatenate([case["user"], case["item"]])
    CL = (F + rng.standard_normal(F.shape) * 0.1).astype(np.float32)
    uu, up = np.unique(case["u"]), np.unique(case["i"])
    f, c = torch.tensor(F, dtype=torch.float64, requires_grad=True), torch.tensor(CL, dtype=torch.float64, requires_grad=True)
    tau, cl_rate = 0.2, 0.2
    if nce_rows == 1:
        cl = cl_rate * (O.info_nce(f[uu], c[uu], tau) + O.info_nce(f[U + up], c[U + up], tau))
    else:
        cat = np.concatenate([uu, U + up])
        cl = cl_rate * O.info_nce(f[cat], c[cat], tau)
    cl.backward()
    ref = R.bpr_l2(case["user"], case["item"], case["user"], case["item"], case["u"], case["i"], case["j"], 1e-4, False, 1.0)
    gF = f.grad.numpy() + np.concatenate([ref["g_user"] + ref["greg_user"], ref["g_item"] + ref["greg_item"]])
    return dict(F=F, CL=CL, uu=uu, up=up, tau=tau, cl_rate=cl_rate, losses=[ref["bpr"], ref["reg"], cl.item()], gF=gF,
                gC=c.grad.numpy())


@pytest.mark.parametrize("d,precision", [(64, "split"), (64, "f32"), (128, "split"), (128, "f32"), (256, "split")])
@pytest.mark.parametrize("nce_rows", [1, 2])
@pytest.mark.parametrize("mode", MODES)
def test_bpr_infonce_matches_restatement(mode, nce_rows, d, precision):
    """srh_bpr_infonce_fwd_bwd on the planted batch, the rows of both losses finished by one launch; bounds of
    test_bpr_infonce_one_call_matches_oracle.  nce_rows = 2 (the SGL convention) takes the one-table form: the problem's
    row k is row group k, users then positive items."""
    case, ref = R.planted_batch(d), nce_reference(d, nce_rows)
    u, i, j = case["u"], case["i"], case["j"]
    B, uu, up = u.size, ref["uu"], ref["up"]
    batch = B + 24
    dF, dC = dev(ref["F"]), dev(ref["CL"])
    named_F = np.concatenate([np.unique(u), U + np.union1d(i, j)])
    named_C = np.concatenate([uu, U + up])
    init = {"gF": initial(mode, ref["gF"], named_F), "gC": initial(mode, ref["gC"], named_C)}
    cnt = lambda n: torch.tensor([n], dtype=torch.int32, device=DEV)
    first = None
    for rep in range(3):
        gF, gC = dev(init["gF"]), dev(init["gC"])
        losses = torch.zeros(3, dtype=torch.float64, device=DEV)
        if nce_rows == 1:
            tabs = (dF[:U], dF[U:]) * 2
            grads = dict(g_user=gF[:U], g_item=gF[U:], greg_user=gF[:U], greg_item=gF[U:])
            problems = [(dF[:U], dC[:U], i32(uu, batch), batch, cnt(uu.size), gF[:U], gC[:U]),
                        (dF[U:], dC[U:], i32(up, batch), batch, cnt(up.size), gF[U:], gC[U:])]
            io = 0
        else:
            tabs = (dF,) * 4
            grads = dict(g_user=gF, g_item=gF, greg_user=gF, greg_item=gF)
            problems = [(dF, dC, i32(np.concatenate([uu, U + up]), 2 * batch), 2 * batch, cnt(uu.size + up.size), gF, gC)]
            io = U
        kw = dict(seg=seg_dev(u, i, j, batch, mode, io), nce_rows=nce_rows) if mode != "atomics" else {}
        nce_ws = torch.empty(sum(ops.infonce_ws(p[3], d, DEV).numel() for p in problems), dtype=torch.uint8, device=DEV)
        ops.bpr_infonce(*tabs, i32(u, batch), i32(i + io, batch), i32(j + io, batch), batch=batch, n_rows_dev=cnt(B),
                        reg_coef=1e-4, reg_include_neg=False, loss_scale=1.0, losses=losses[0:2], bpr_ws=ops.bpr_ws(batch, DEV),
                        problems=problems, tau=ref["tau"], cl_scale=ref["cl_rate"], cl_loss=losses[2:3], nce_ws=nce_ws,
                        precision=precision, **grads, **kw)
        raw = (bits(gF), bits(gC), losses.cpu().numpy().view(np.int64))
        if first is None:
            first = raw
            got_l = losses.cpu().numpy()
            eF = R.rel_err(delta(mode, gF, init["gF"], named_F, "gF"), ref["gF"])
            eC = R.rel_err(delta(mode, gC, init["gC"], named_C, "gC"), ref["gC"])
            el = np.abs(got_l - ref["losses"]) / np.abs(ref["losses"])
            print(f"{mode} nce_rows={nce_rows} d={d} {precision}: losses {el[0]:.2e} {el[1]:.2e} {el[2]:.2e} (bound 1e-5); "
                  f"gF {eF:.2e}, gC {eC:.2e} (bound 2e-5)")
            assert el.max() < 1e-5 and eF < 2e-5 and eC < 2e-5
        elif mode != "atomics":
            assert all(np.array_equal(a, b) for a, b in zip(first, raw)), rep


# ---------------------------------------------------------------------------------------------------------------------------
# Adam
# ---------------------------------------------------------------------------------------------------------------------------
BIG = (16387, 256)            # 1048768 float4: the grid's 4096 x 256 lanes take a second trip of 192, ending inside a workgroup


def check_adam(got, ref, tag):
    errs = {k: R.elem_error(got[k], ref[k], ref["s_" + k]) for k in "pmv"}
    print(f"{tag}: " + ", ".join(f"{k} {errs[k]:.2e} (bound {R.ADAM_BOUND[k]:.1e})" for k in "pmv"))
    for k in "pmv":
        assert errs[k] < R.ADAM_BOUND[k], (tag, k)


@pytest.mark.parametrize("by_dev", [False, True], ids=["step-host", "step-dev"])
@pytest.mark.parametrize("shape,steps", [((1, 4), R.ADAM_STEPS), ((3, 36), R.ADAM_STEPS), ((1000, 64), R.ADAM_STEPS),
                                         (BIG, (1, 1000))], ids=["1x4", "3x36", "1000x64", "second-trip"])
def test_adam_matches_restatement(shape, steps, by_dev):
    p, g, m, v = R.adam_case(*shape)
    h = R.ADAM_HYPER
    for t in steps:
        dp, dg, dm, dv = (dev(a) for a in (p, g, m, v))
        step = dict(step_dev=torch.tensor([t], dtype=torch.int64, device=DEV)) if by_dev else dict(step=t)
        ops.adam_step(dp, dg, dm, dv, lr=h["lr"], beta1=h["b1"], beta2=h["b2"], eps=h["eps"], **step)
        assert np.array_equal(bits(dg), g.view(np.int32))
        check_adam({"p": dp.cpu().numpy(), "m": dm.cpu().numpy(), "v": dv.cpu().numpy()}, R.adam(p, g, m, v, t, **h),
                   f"adam {shape} t={t}")


@pytest.mark.parametrize("d", [32, 64, 128, 256])
def test_adam_reset_clears_the_stamped_rows_and_nothing_else(d):
    """srh_adam_step_reset: two tables that are non-zero EVERYWHERE; a scattered third of the rows carries this step's stamp, a
    third the previous step's, the rest 0.  The gradient is one of the cleared tables (read before it is cleared)."""
    rows, t = 301, 7
    p, g, m, v = R.adam_case(rows, d, seed=d)
    g = np.where(g == 0, np.float32(1e-3), g)                      # (the cleared tables hold no zero before the call)
    other = (np.random.default_rng(d).standard_normal((rows, d)) + 3.0).astype(np.float32)
    mark = np.zeros(rows, dtype=np.int32)
    perm = np.random.default_rng(d + 1).permutation(rows)
    mark[perm[:100]], mark[perm[100:200]] = t, t - 1
    h = R.ADAM_HYPER
    kw = dict(lr=h["lr"], beta1=h["b1"], beta2=h["b2"], eps=h["eps"])
    plain = [dev(a) for a in (p, g, m, v)]
    ops.adam_step(*plain, step_dev=torch.tensor([t], dtype=torch.int64, device=DEV), **kw)
    dp, dgA, dm, dv, dgB, dmark = (dev(a) for a in (p, g, m, v, other, mark))
    cursor = torch.tensor([5, t], dtype=torch.int64, device=DEV)
    ops.adam_step(dp, dgA, dm, dv, step_dev=torch.tensor([t], dtype=torch.int64, device=DEV), clear=[dgA, dgB], row_mark=dmark,
                  advance_cursor=cursor, **kw)
    for a, b in zip((dp, dm, dv), (plain[0], plain[2], plain[3])):
        assert torch.equal(a, b)                                   # the aliased, clearing call: the plain call's bits
    check_adam({"p": dp.cpu().numpy(), "m": dm.cpu().numpy(), "v": dv.cpu().numpy()}, R.adam(p, g, m, v, t, **h), f"adam reset d={d}")
    assert cursor.tolist() == [6, t + 1]
    for got, was in ((dgA, g), (dgB, other)):
        got = got.cpu().numpy()
        assert not got[mark == t].any()
        assert np.array_equal(got[mark != t].view(np.int32), was[mark != t].view(np.int32))
    assert (mark == t).sum() == 100 and (mark == t - 1).sum() == 100


def test_adam_reset_refuses_a_row_that_is_no_power_of_two_of_float4():
    rows, d, t = 8, 48, 3
    host = [a.copy() for a in R.adam_case(rows, d)] + [np.full((rows, d), 2.0, dtype=np.float32)]
    tens = [dev(a) for a in host]
    mark = torch.full((rows,), t, dtype=torch.int32, device=DEV)
    cursor = torch.tensor([1, t], dtype=torch.int64, device=DEV)
    with pytest.raises(SelfrecHipError, match=r"d = 48 \(rows of a power-of-two number of float4\)"):
        ops.adam_step(*tens[:4], step_dev=torch.tensor([t], dtype=torch.int64, device=DEV), lr=0.01, clear=[tens[4]],
                      row_mark=mark, advance_cursor=cursor)
    torch.cuda.synchronize()
    assert all(np.array_equal(bits(a), b.view(np.int32)) for a, b in zip(tens, host))
    assert cursor.tolist() == [1, t] and mark.tolist() == [t] * rows


# ---------------------------------------------------------------------------------------------------------------------------
# zero_rows, axpby, cursor_advance
# ---------------------------------------------------------------------------------------------------------------------------
def zero_lists(d, n_lists, rng):
    """(host table, idx array, device count or None, n_max, row_offset) per list.  Every idx array is longer than any count
    and holds valid rows to its end: the entries past a list's count name rows that must NOT be cleared."""
    rows, longest = 60, 32
    plans = [(12, None, 0), (10, 6, 7), (10, 10, 0), (9, 25, 7), (1, None, 3), (12, 0, 0), (5, 5, 11), (7, 3, 0)][:n_lists]
    out = []
    for n_max, count, off in plans:
        idx = rng.permutation(40)[:longest].astype(np.int32)
        idx[1] = idx[0]                                            # a duplicate
        live = n_max if count is None else min(count, n_max)
        out.append(dict(table=np.full((rows, d), SENTINEL, dtype=np.float32), idx=idx, count=count, n_max=n_max, off=off,
                        want=np.unique(idx[:live].astype(np.int64) + off)))
    return out


@pytest.mark.parametrize("n_lists", [1, 8])
@pytest.mark.parametrize("d", [4, 36, 64, 256])
def test_zero_rows_clears_the_listed_rows_and_nothing_else(d, n_lists):
    """counts on the device below, equal to and above n_max (clamped) or absent; row offsets; a duplicate index"""
    lists = zero_lists(d, n_lists, np.random.default_rng(d + n_lists))
    tabs = [dev(z["table"]) for z in lists]
    cursor = torch.tensor([3, 9], dtype=torch.int64, device=DEV)
    ops.zero_rows([(t, dev(z["idx"]), None if z["count"] is None else torch.tensor([z["count"]], dtype=torch.int32, device=DEV),
                    z["n_max"], z["off"]) for t, z in zip(tabs, lists)], d, cursor_advance=cursor)
    for k, (t, z) in enumerate(zip(tabs, lists)):
        got = t.cpu().numpy()
        keep = np.ones(got.shape[0], dtype=bool)
        keep[z["want"]] = False
        assert not got[z["want"]].any() and not np.signbit(got[z["want"]]).any(), k
        assert np.array_equal(got[keep].view(np.int32), z["table"][keep].view(np.int32)), k
    assert cursor.tolist() == [4, 10]


def test_zero_rows_with_nothing_to_clear_moves_only_the_cursor_and_refuses_0_and_9_lists():
    d = 8
    tab = torch.full((6, d), 5.0, device=DEV)
    idx = torch.zeros(4, dtype=torch.int32, device=DEV)
    cursor = torch.tensor([0, 1], dtype=torch.int64, device=DEV)
    ops.zero_rows([(tab, idx, None, 0, 0), (tab, idx, torch.tensor([3], dtype=torch.int32, device=DEV), 0, 2)], d, cursor_advance=cursor)
    assert cursor.tolist() == [1, 2] and bool((tab == 5.0).all())
    ops.zero_rows([(tab, idx, None, 0, 0)], d)                      # no cursor either: nothing at all
    assert cursor.tolist() == [1, 2] and bool((tab == 5.0).all())
    for n in (0, 9):
        with pytest.raises(SelfrecHipError, match=r"zero_rows: 1\.\.8 lists"):
            ops.zero_rows([(tab, idx, None, 1, 0)] * n, d, cursor_advance=cursor)
    torch.cuda.synchronize()
    assert cursor.tolist() == [1, 2] and bool((tab == 5.0).all())


AXPBY_SIZES = [4, 1000, 4 * (256 * 16 * 256 + 300)]                # the last: past the grid's one trip, ending inside a workgroup


@pytest.mark.parametrize("n", AXPBY_SIZES)
def test_axpby(n):
    """y = a x + b y.  Bound from the formats: two products and a sum, each rounded once (or one of them fused away):
    2.5 x 2^-24 of |a x| + |b y|.  b == 0 must not read y."""
    rng = np.random.default_rng(n)
    x, y = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    a, b = np.float32(0.37), np.float32(-1.9)
    dx = dev(x)
    dy = torch.full((n,), float("nan"), device=DEV)
    assert ops.axpby(a, dx, 0.0, dy) is dy
    got = dy.cpu().numpy()
    assert np.array_equal(got, a * x) and not np.isnan(got).any()          # (one f32 product: exact agreement)

    def close(got, xs, ys, tag):
        want = float(a) * xs.astype(np.float64) + float(b) * ys.astype(np.float64)
        scale = np.abs(float(a) * xs.astype(np.float64)) + np.abs(float(b) * ys.astype(np.float64))
        err = float((np.abs(got - want) / scale).max())
        print(f"axpby n={n} {tag}: {err:.2e} of |a x| + |b y| (bound {2.5 * 2.0 ** -24:.2e})")
        assert err < 2.5 * 2.0 ** -24
    dy = dev(y)
    ops.axpby(a, dx, b, dy)
    close(dy.cpu().numpy(), x, y, "b != 0")
    assert np.array_equal(bits(dx), x.view(np.int32))
    dz = dev(y)
    ops.axpby(a, dz, b, dz)                                                  # x is y
    close(dz.cpu().numpy(), y, y, "x aliases y")


def test_axpby_refuses_a_size_that_is_no_multiple_of_4():
    x, y = torch.ones(6, device=DEV), torch.full((6,), 2.0, device=DEV)
    with pytest.raises(SelfrecHipError, match="n_elem must be a positive multiple of 4"):
        ops.axpby(1.0, x, 1.0, y)
    torch.cuda.synchronize()
    assert y.tolist() == [2.0] * 6 and x.tolist() == [1.0] * 6


def test_cursor_advance_twice():
    cursor = torch.tensor([41, 2 ** 40], dtype=torch.int64, device=DEV)
    ops.cursor_advance(cursor)
    assert cursor.tolist() == [42, 2 ** 40 + 1]
    ops.cursor_advance(cursor)
    assert cursor.tolist() == [43, 2 ** 40 + 2]
