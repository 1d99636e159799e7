"""The fused step WITHOUT the InfoNCE prep launch: the stage rider on the product that reads the contrast
table (srh_spmm_f32_with_nce_stage: key-side view, counters, plan), pass 1 normalising its own queries and carrying BPR
phase 1 (srh_bpr_infonce_fwd_bwd_staged) -- against the launch sequence with nce_prep_bpr1, which stays in the tree
(SRH_NCE_PREP=1 / FusedTrainer._prep_launch).  The two sequences are the same arithmetic in other launches, so "the same"
means np.array_equal: both normalised views and their norms, the BPR coefficients and partials, the three losses, both
gradient tables -- and every other byte of the two workspaces, which start as 0xFF.  Loss and gradients are also held to
the float64 restatements (tests/nce_ref.py per row, tests/batch_ref.py) at those files' bounds.

Shapes: the unique-user count n on both sides of the 16-row wave tile, the 32-key block, the 128-row query block and at
257; the item-side problem always smaller; the live count at the launch bound and 63 below it (the zero fill up to the
workspace's padded rows); batches of 1, 15, 16, 17 and 37 pairs with repeated users and items (BPR phase 1's tail and the
two 256-thread halves of its 512-thread workgroups); one case at d = 128."""
import numpy as np
import pytest
import torch

from selfrec_amd import _lib, ops

from . import batch_ref as B
from . import nce_ref as R
from . import test_gpu_batch as T
from .conftest import host_batch_segments

pytestmark = pytest.mark.gpu
DEV = "cuda"
NU, NI = 270, 230                # rows of the user / item part of the (NU + NI, d) tables
N = NU + NI
TAU, CL_RATE, REG = 0.2, 0.2, 1e-4


def pad(n):
    return (n + 63) // 64 * 64


def ws_bytes(n_max, d):
    return int(_lib.load().srh_infonce_ws_bytes(n_max, d))


def ws_regions(n_max, d):
    """byte ranges of one problem's workspace that the test names (csrc/losses.hip: carve_nce)"""
    np_ = pad(n_max)
    f = 4
    off = {"v1n": (0, np_ * d * f), "v2n": (np_ * d * f, 2 * np_ * d * f)}
    at = (2 + 2 * 16) * np_ * d * f
    off["norm1"] = (at, at + np_ * f)
    off["norm2"] = (at + np_ * f, at + 2 * np_ * f)
    at += (2 + 16 + 2) * np_ * f
    off["losspart"] = (at, at + 8 * np_)
    at += 8 * np_ + 20 * np_ * d
    off["ticket"] = (at, at + 4 * (np_ // 16 + 1))
    plan = at + (4 * (np_ // 16 + 1) + 127) // 128 * 128
    off["plan"] = (plan, plan + 17 * 4)
    return off


def make_case(b_live, n_u, n_i, bound, d, seed):
    """a batch of b_live pairs naming exactly n_u users and n_i positive items (every one at least once, the rest repeats),
    under a launch bound of `bound` rows; tables of unit-scale rows"""
    assert n_i <= n_u <= b_live <= bound and n_u <= NU and n_i <= NI
    rng = np.random.default_rng(seed)
    users = np.sort(rng.choice(NU, n_u, replace=False))
    items = np.sort(rng.choice(NI, n_i, replace=False))
    u = rng.permutation(np.concatenate([users, rng.choice(users, b_live - n_u)]))
    i = rng.permutation(np.concatenate([items, rng.choice(items, b_live - n_i)]))
    j = rng.integers(0, NI, b_live)
    F = (rng.standard_normal((N, d)) * 0.3).astype(np.float32)
    C = (F + rng.standard_normal((N, d)) * 0.1).astype(np.float32)
    return dict(u=u, i=i, j=j, users=users, items=items, F=F, C=C, bound=bound, d=d)


_GRAPH = {}


def graph():
    """a random sparse (N, N) operator for the product that carries the rider (a few hundred entries a row at most)"""
    if "g" not in _GRAPH:
        import scipy.sparse as sp
        rng = np.random.default_rng(5)
        m = sp.random(N, N, density=0.02, random_state=rng, format="csr", dtype=np.float32)
        _GRAPH["g"] = ops.DeviceCSR.from_scipy(m, torch.device(DEV, torch.cuda.current_device()))
    return _GRAPH["g"]


def run_sequence(c, staged, epilogue=None):
    """one loss section from a 0xFF workspace: the product (with the rider when staged), then the fused loss call.
    -> dict of host arrays"""
    d, bound = c["d"], c["bound"]
    u, i, j = c["u"], c["i"], c["j"]
    dF, dC = T.dev(c["F"]), T.dev(c["C"])
    named_F = np.concatenate([np.unique(u), NU + np.union1d(i, j)])
    named_C = np.concatenate([c["users"], NU + c["items"]])
    zeros = np.zeros((N, d), dtype=np.float32)
    init = {"gF": T.initial("segments-store", zeros, named_F), "gC": T.initial("segments-store", zeros, named_C)}
    gF, gC = T.dev(init["gF"]), T.dev(init["gC"])
    cnt = lambda n: torch.tensor([n], dtype=torch.int32, device=DEV)          # noqa: E731
    problems = [(dF[:NU], dC[:NU], T.i32(c["users"], bound), bound, cnt(c["users"].size), gF[:NU], gC[:NU], True),
                (dF[NU:], dC[NU:], T.i32(c["items"], bound), bound, cnt(c["items"].size), gF[NU:], gC[NU:], True)]
    nce_ws = torch.full((2 * ws_bytes(bound, d),), 0xFF, dtype=torch.uint8, device=DEV)
    bpr_ws = torch.full_like(ops.bpr_ws(bound, DEV), 0xFF)
    losses = torch.zeros(3, dtype=torch.float64, device=DEV)
    seg = {k: T.dev(v) for k, v in host_batch_segments(u, i, j, bound, 0, 0).items()}
    seg["rows_are_zero"] = True
    y = ops.spmm(graph(), dC, epilogue=epilogue() if epilogue else None, **({"nce_stage": (problems, nce_ws)} if staged else {}))
    ops.bpr_infonce(dF[:NU], dF[NU:], dF[:NU], dF[NU:], T.i32(u, bound), T.i32(i, bound), T.i32(j, bound), batch=bound,
                    n_rows_dev=cnt(u.size), reg_coef=REG, reg_include_neg=False, loss_scale=1.0, losses=losses[0:2],
                    bpr_ws=bpr_ws, problems=problems, tau=TAU, cl_scale=CL_RATE, cl_loss=losses[2:3], nce_ws=nce_ws,
                    precision="f32", g_user=gF[:NU], g_item=gF[NU:], greg_user=gF[:NU], greg_item=gF[NU:],
                    seg=seg, nce_rows=1, staged=staged)
    torch.cuda.synchronize()
    return dict(y=y.cpu().numpy(), nce_ws=nce_ws.cpu().numpy(), bpr_ws=bpr_ws.cpu().numpy(), losses=losses.cpu().numpy(),
                gF=gF.cpu().numpy(), gC=gC.cpu().numpy(), init=init, named_F=named_F, named_C=named_C)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def assert_same_run(new, old, c, tag):
    one = ws_bytes(c["bound"], c["d"])
    for k in range(2):
        for name, (lo, hi) in ws_regions(c["bound"], c["d"]).items():
            assert same_bits(new["nce_ws"][k * one + lo:k * one + hi], old["nce_ws"][k * one + lo:k * one + hi]), \
                f"{tag}: problem {k}: {name} differs"
    assert same_bits(new["bpr_ws"], old["bpr_ws"]), f"{tag}: BPR coefficients / partials differ"
    assert same_bits(new["losses"], old["losses"]), f"{tag}: losses {new['losses']} != {old['losses']}"
    assert same_bits(new["gF"], old["gF"]), f"{tag}: gF differs"
    assert same_bits(new["gC"], old["gC"]), f"{tag}: gC differs"
    assert same_bits(new["nce_ws"], old["nce_ws"]), f"{tag}: a workspace byte outside the named arrays differs"
    assert same_bits(new["y"], old["y"]), f"{tag}: the product that carries the rider differs"


def check_against_float64(out, c, tag):
    """cl loss and gC per row against nce_ref.info_nce_rows (that file's bounds: LOSS_BOUND, ROW_BOUND_F32); BPR / reg losses
    and gF against batch_ref.bpr_l2 + the InfoNCE part (the bounds of test_gpu_batch.test_bpr_infonce_matches_restatement)"""
    F, C = c["F"], c["C"]
    parts = [(F[:NU], C[:NU], c["users"], 0), (F[NU:], C[NU:], c["items"], NU)]
    want_cl, gF64 = 0.0, np.zeros((N, c["d"]))
    gC = T.delta("segments-store", torch.from_numpy(out["gC"]), out["init"]["gC"], out["named_C"], "gC")
    worst = 0.0
    for t1, t2, idx, row0 in parts:
        l64, a64, b64 = R.info_nce_rows(t1, t2, idx.astype(np.int32), TAU, CL_RATE, device=DEV)
        want_cl += l64
        gF64[row0:row0 + t1.shape[0]] += a64.cpu().numpy()
        if idx.size > 1:
            e = R.row_errors(gC[row0 + idx], b64[torch.from_numpy(idx.astype(np.int64)).to(DEV)], R.FLOOR_FRAC)
            worst = max(worst, float(e.max()))
        else:
            assert not gC[row0 + idx].any(), f"{tag}: one pair has no gradient"
    ref = B.bpr_l2(F[:NU], F[NU:], F[:NU], F[NU:], c["u"], c["i"], c["j"], REG, False, 1.0)
    gF64[:NU] += ref["g_user"] + ref["greg_user"]
    gF64[NU:] += ref["g_item"] + ref["greg_item"]
    gF = T.delta("segments-store", torch.from_numpy(out["gF"]), out["init"]["gF"], out["named_F"], "gF")
    eF = B.rel_err(gF, gF64)
    got = out["losses"]
    el = [abs(got[0] - ref["bpr"]) / abs(ref["bpr"]), abs(got[1] - ref["reg"]) / abs(ref["reg"]),
          abs(got[2] - want_cl) / abs(want_cl) if want_cl != 0.0 else abs(got[2])]
    print(f"{tag}: bpr {el[0]:.2e} reg {el[1]:.2e} (bound 1e-5), cl {el[2]:.2e} (bound {R.LOSS_BOUND['f32']:.0e}); "
          f"gC per row {worst:.2e} (bound {R.ROW_BOUND_F32:.2e}), gF {eF:.2e} (bound 2e-5)")
    assert el[0] < 1e-5 and el[1] < 1e-5 and el[2] < R.LOSS_BOUND["f32"]
    assert worst < R.ROW_BOUND_F32 and eF < 2e-5


# (pairs, unique users, unique positive items, launch bound, d)
N_EDGES = [(n + 5, n, max(1, min(n - 3, 200)), n + 105, 64) for n in (1, 16, 17, 31, 32, 33, 127, 128, 129, 257)]
BOUND_EDGES = [(128, 128, 100, 128, 64),        # n = n_max
               (150, 129, 90, 192, 64)]         # n = n_max - 63: the plan cuts 192 rows, the live rows end at 129
BATCH_EDGES = [(b, max(1, (2 * b + 2) // 3), max(1, b // 2), b + 24, 64) for b in (1, 15, 16, 17, 37)]
WIDE = [(140, 129, 70, 200, 128)]
CASES = N_EDGES + BOUND_EDGES + BATCH_EDGES + WIDE


@pytest.mark.parametrize("case", CASES, ids=lambda s: "B%d_nu%d_ni%d_max%d_d%d" % s)
def test_staged_sequence_gives_the_prep_launch_bits(case):
    b_live, n_u, n_i, bound, d = case
    c = make_case(b_live, n_u, n_i, bound, d, seed=100 * b_live + n_u)
    tag = "B%d nu=%d ni=%d bound=%d d=%d" % case
    old = run_sequence(c, staged=False)
    new = run_sequence(c, staged=True)
    again = run_sequence(c, staged=True)
    assert_same_run(again, new, c, tag + " (second call)")
    assert_same_run(new, old, c, tag)
    check_against_float64(new, c, tag)


@pytest.mark.parametrize("flavour", ["plain", "perturbed", "row-masked"])
def test_rider_leaves_the_product_alone_and_writes_what_prep_writes(flavour):
    """the product with the rider against the same product without it (y bit-equal, every launch flavour the engine rides
    on), and what the rider alone leaves in a 0xFF workspace: v2n / norm2 / the plan as the prep launch writes them, the
    counters zero, the loss partials unreported, v1n / norm1 zero from the plan's padded rows on and untouched below"""
    b_live, n_u, n_i, bound, d = 150, 129, 90, 260, 64
    c = make_case(b_live, n_u, n_i, bound, d, seed=77)
    dC = T.dev(c["C"])
    mark = torch.zeros(N, dtype=torch.int32, device=DEV)
    mark[torch.from_numpy(np.concatenate([c["users"], NU + c["items"]]))] = 9
    stamp = torch.tensor([9], dtype=torch.int64, device=DEV)
    epi = {"plain": lambda: None, "perturbed": lambda: ops.make_epilogue(perturb_eps=0.2, rng_seed=3, rng_offset=0),
           "row-masked": lambda: ops.make_epilogue(row_mark=mark, mark_stamp=stamp)}[flavour]
    cnt = lambda n: torch.tensor([n], dtype=torch.int32, device=DEV)          # noqa: E731
    g = torch.zeros((N, d), device=DEV)
    problems = [(dC[:NU], dC[:NU], T.i32(c["users"], bound), bound, cnt(n_u), g[:NU], g[:NU], True),
                (dC[NU:], dC[NU:], T.i32(c["items"], bound), bound, cnt(n_i), g[NU:], g[NU:], True)]
    ws = torch.full((2 * ws_bytes(bound, d),), 0xFF, dtype=torch.uint8, device=DEV)
    y0 = torch.full((N, d), 7.0, device=DEV)
    y1 = torch.full((N, d), 7.0, device=DEV)
    ops.spmm(graph(), dC, out=y0, epilogue=epi())
    ops.spmm(graph(), dC, out=y1, epilogue=epi(), nce_stage=(problems, ws))
    torch.cuda.synchronize()
    assert torch.equal(y0, y1)
    old = run_sequence(c, staged=False)                   # (v2n, norm2 and the plan are the prep launch's to the end)
    got, one, reg = ws.cpu().numpy(), ws_bytes(bound, d), ws_regions(bound, d)
    slots = torch.cuda.get_device_properties(0).multi_processor_count
    plan = ops.infonce_plan([n_u, n_i], slots)
    for k, n in enumerate((n_u, n_i)):
        part, was = got[k * one:(k + 1) * one], old["nce_ws"][k * one:(k + 1) * one]
        for name in ("v2n", "norm2"):
            lo, hi = reg[name]
            assert same_bits(part[lo:hi], was[lo:hi]), (k, name)
        assert not part[slice(*reg["ticket"])].any(), (k, "ticket")
        assert (part[slice(*reg["losspart"])] == 0xFF).all(), (k, "losspart")
        v1n = part[slice(*reg["v1n"])].view(np.float32).reshape(pad(bound), d)
        norm1 = part[slice(*reg["norm1"])].view(np.float32)
        assert (part[slice(*reg["v1n"])].reshape(pad(bound), 4 * d)[:pad(n)] == 0xFF).all(), (k, "v1n below the plan's rows")
        assert not v1n[pad(n):].any() and not norm1[pad(n):].any(), (k, "v1n / norm1 past the plan's rows")
    rec = got[slice(*reg["plan"])].view(np.int32)
    assert same_bits(rec, old["nce_ws"][slice(*reg["plan"])])
    assert list(rec[0:2]) == plan["n"] and list(rec[4:6]) == plan["per"] and list(rec[8:10]) == plan["splits"] \
        and int(rec[16]) == plan["tasks"]


def test_rider_refuses_what_it_cannot_serve():
    c = make_case(20, 10, 5, 40, 64, seed=1)
    dC = T.dev(c["C"])
    cnt = lambda n: torch.tensor([n], dtype=torch.int32, device=DEV)          # noqa: E731
    g = torch.zeros((N, 64), device=DEV)
    ws = torch.full((ws_bytes(40, 64),), 0xFF, dtype=torch.uint8, device=DEV)
    y = torch.full((N, 64), 7.0, device=DEV)
    with pytest.raises(ops.SelfrecHipError):                      # the rider would read the table the product writes
        ops.spmm(graph(), dC, out=y, nce_stage=([(dC, y, T.i32(c["users"], 40), 40, cnt(10), g, g, True)], ws))
    torch.cuda.synchronize()
    assert float((y - 7.0).abs().max()) == 0 and (ws == 0xFF).all()


# ---- the engine ---------------------------------------------------------------------------------------------------------
def tiny_trainer(**over):
    from selfrec_amd import synth
    from selfrec_amd.data.ui_graph import Interaction
    from selfrec_amd.engine import FusedTrainer
    tu, ti, su, si, U, I = synth.make_dataset("tiny")
    data = Interaction({}, synth.as_triples(tu, ti), synth.as_triples(su, si))
    torch.manual_seed(0)
    ue = torch.nn.init.xavier_uniform_(torch.empty(U, 64))
    ie = torch.nn.init.xavier_uniform_(torch.empty(I, 64))
    kw = dict(model="XSimGCL", n_layers=3, lr=1e-3, reg=1e-4, cl_rate=0.2, eps=0.2, tau=0.2, layer_cl=1,
              batch_size=(len(tu) + 2) // 3 + 1, user_emb=ue, item_emb=ie, nce_precision="f32")        # three batches an epoch
    kw.update(over)
    return FusedTrainer(data, 64, **kw)


def four_steps(tr, monkeypatch=None):
    """4 steps: the three batches of an epoch and the first of the next -> (tables, Adam moments, losses per step, what
    every loss call was told about `staged`)"""
    from selfrec_amd import engine
    seen = []
    real = engine.ops.bpr_infonce

    def spy(*a, **kw):
        seen.append(bool(kw.get("staged", False)))
        return real(*a, **kw)
    engine.ops.bpr_infonce = spy
    try:
        tr.sampler.seed(5)
        losses, left = [], 4
        while left:
            nb = tr.begin_epoch()
            assert nb == 3
            for _ in range(min(nb, left)):
                tr.step()
                losses.append(tr.read_losses())
                left -= 1
        torch.cuda.synchronize()
    finally:
        engine.ops.bpr_infonce = real
    return dict(E0=tr.E0.cpu().numpy(), m=tr.m.cpu().numpy(), v=tr.v.cpu().numpy(), losses=np.array(losses)), seen


@pytest.mark.parametrize("use_graph", [True, False], ids=["hipgraph", "eager"])
def test_engine_without_the_prep_launch_trains_the_same_bits(use_graph):
    outs = []
    for prep_launch in (False, True):
        tr = tiny_trainer(use_graph=use_graph)
        tr._prep_launch = prep_launch
        assert tr.nce_stage_ok and tr._nce_staged() == (not prep_launch)
        out, seen = four_steps(tr)
        assert seen and all(s == (not prep_launch) for s in seen), seen
        outs.append(out)
    assert np.isfinite(outs[0]["E0"]).all() and np.isfinite(outs[0]["losses"]).all()
    for k in ("E0", "m", "v", "losses"):
        assert np.array_equal(outs[0][k], outs[1][k]), k


@pytest.mark.parametrize("over", [dict(layer_cl=3), dict(nce_precision="split")], ids=["layer_cl=L", "split"])
def test_engine_keeps_the_prep_launch_where_nothing_can_carry_it(over):
    """layer_cl == L (no product after the contrast table) and the split arithmetic: the launch sequence with nce_prep_bpr1,
    the same bits as under the switch"""
    outs = []
    for prep_launch in (False, True):
        tr = tiny_trainer(use_graph=True, **over)
        tr._prep_launch = prep_launch
        assert not tr._nce_staged()
        out, seen = four_steps(tr)
        assert seen and not any(seen), seen
        outs.append(out)
    assert np.isfinite(outs[0]["E0"]).all() and np.isfinite(outs[0]["losses"]).all()
    for k in ("E0", "m", "v", "losses"):
        assert np.array_equal(outs[0][k], outs[1][k]), k


# ---- the built kernel ----------------------------------------------------------------------------------------------------
def test_staged_pass_never_touches_an_unsettled_lds_read():
    """tests/test_isa_async_lds.py's reading of nce_tile_f32, on the kernels of the same body that normalise their own
    queries (d = 64 / 128 x weights kept / recomputed): no instruction touches a register whose opaque LDS read may be in
    flight, the ring is filled by buffer_load ... lds.  The checker's model is one straight line; in these kernels the
    compiler lays the prologue's first S product (eight reads, their wait, MFMAs into a zero accumulator) out BEHIND the key
    loop, after an unconditional s_branch, where a straight-line reading inherits the loop tail's pending reads although
    nothing falls through.  So the stream is read one fall-through region at a time (cut after every s_branch / s_endpgm);
    a region entered only by jumps starts with nothing pending -- weaker than the straight-line reading where that holds,
    which is why nce_tile_f32 keeps the other test."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import device_isa
    ks = device_isa.kernels(name_filter="nce_pass1_raw_f32")
    assert len(ks) == 4, sorted(ks)
    for name, body in ks.items():
        assert sum(i.startswith("ds_read_b128") for i in body) >= 16, name
        assert sum(i.startswith("v_mfma_f32_16x16x4_f32") for i in body) >= 64, name
        regions, cur = [], []
        for ins in body:
            cur.append(ins)
            if ins.split(" ")[0] in ("s_branch", "s_endpgm"):
                regions.append(cur)
                cur = []
        regions.append(cur)
        assert sum(len(r) for r in regions) == len(body)
        for r in regions:
            bad = device_isa.async_lds_violations(r)
            assert not bad, (name, bad[:5])
        assert any("buffer_load_dwordx4" in i and "lds" in i for i in body), name
        assert not any(i.startswith("global_load_lds") for i in body), name
