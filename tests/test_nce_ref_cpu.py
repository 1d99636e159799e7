"""tests/nce_ref.py pinned without a GPU: the plan restatement against the library's own nce_plan (srh_infonce_plan), the
properties the f32 passes rely on for every plan, the closed form against float64 autograd on the oracle's info_nce, the
premises of every case of tests/test_gpu_nce_edges.py, and the floor and float32 yardstick its bounds come from
(DESIGN.md 4.19)."""
import numpy as np
import pytest
import torch

from oracle import selfrec_oracle as O
from selfrec_amd import _lib, ops

from . import nce_ref as R

SLOTS = (1, 64, 104, 128, 228, 256, 304)


def _lib_plan(ns, slots):
    got = ops.infonce_plan(ns, slots)
    return got["n"], got["per"], got["splits"], got["first"]


def _ref_plan(ns, slots):
    p = R.plan(ns, slots)
    return p["n"], p["per"], p["splits"], p["first"]


def _draws(count=3000, seed=11):
    """seeded two- to four-problem calls: counts from one row to the f32 passes' limit, small ones as likely as large"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        k = int(rng.integers(2, R.MAX_PROBLEMS + 1))
        ns = [int(min(R.F32_MAX_N, max(1, round(2.0 ** rng.uniform(0, 16))))) for _ in range(k)]
        out.append((tuple(ns), int(rng.choice(SLOTS))))
    return out


def _all_plans():
    for slots in SLOTS:
        for np_ in range(R.PAD, R.F32_MAX_N + 1, R.PAD):
            yield (np_,), slots
    yield from _draws()


def test_plan_restatement_equals_the_library():
    """nce_ref.plan == srh_infonce_plan: every padded count of one problem at seven workgroup counts, counts just below a
    padding step, and 3000 seeded calls of two to four problems"""
    for slots in SLOTS:
        for np_ in range(R.PAD, R.F32_MAX_N + 1, R.PAD):
            assert _lib_plan((np_,), slots) == _ref_plan((np_,), slots), (np_, slots)
        for n in (1, 2, 63, 65, 4097, 8193, 12289, 65473):
            assert _lib_plan((n,), slots) == _ref_plan((n,), slots), (n, slots)
    for ns, slots in _draws():
        assert _lib_plan(ns, slots) == _ref_plan(ns, slots), (ns, slots)


def test_plan_entry_refuses_what_the_passes_refuse():
    lib = _lib.load()
    import ctypes as C
    out = (C.c_int32 * 17)()
    one = (C.c_int32 * 1)(R.F32_MAX_N + 1)
    assert lib.srh_infonce_plan(C.cast(one, C.c_void_p), 1, 256, C.cast(out, C.c_void_p)) == -3      # SRH_ERR_UNSUPPORTED
    assert b"n <= 65536" in lib.srh_last_error_string()
    assert lib.srh_infonce_plan(None, 1, 256, C.cast(out, C.c_void_p)) == -1
    assert lib.srh_infonce_plan(C.cast(one, C.c_void_p), 5, 256, C.cast(out, C.c_void_p)) == -1
    assert lib.srh_infonce_plan(C.cast(one, C.c_void_p), 1, 0, C.cast(out, C.c_void_p)) == -1
    with pytest.raises(ops.SelfrecHipError):
        ops.infonce_plan((-1,), 256)
    assert ops.infonce_plan((R.F32_MAX_N,), 256)["per"] == [R.MAX_PER]


def test_every_plan_fits_what_the_passes_allocate():
    """For every plan of test_plan_restatement_equals_the_library, as srh_infonce_plan returns it:
        splits <= kNceSplits                    (the split partials' workspace holds 16)
        per <= kNceMaxPer                       (a task's 1 / l values: kNceMaxPer x 32 floats of LDS)
        (splits - 1) per < kb                   (the last key range is not empty: the kernel's "nblk >= 1")
        the ranges of a query block tile [0, kb) exactly once; first[] is the running sum of qb x splits
        launch_infonce's `most` >= min(tasks, slots)   (no workgroup the plan needs is missing from the grid)

    `per <= kNceMaxPer` FAILED before nce_plan bounded its search: on 256 workgroups np = 12 352 gave per 129 (3 splits),
    16 384 gave 256 (2 splits), 65 536 gave 2048 (1 split) -- tasks whose 1 / l array would reach past the workgroup's LDS
    (R.plan(..., max_per=None) restates that search; the assertions at the end hold the figures).  Found by reading and by
    this restatement; the unbounded kernel was never run at those n."""
    for ns, slots in _all_plans():
        p = ops.infonce_plan(ns, slots)                    # the library's own cut
        tag = (ns, slots, p)
        for k in range(len(ns)):
            kb, qb = R.pad(ns[k]) // R.KEY_BLOCK, (R.pad(ns[k]) + R.QUERY_BLOCK - 1) // R.QUERY_BLOCK
            sp, per = p["splits"][k], p["per"][k]
            assert 1 <= sp <= R.SPLITS, tag
            assert 1 <= per <= R.MAX_PER, tag
            assert (sp - 1) * per < kb <= sp * per, tag
            cover = np.zeros(kb, dtype=np.int64)
            for s in range(sp):
                b0 = s * per
                nblk = min(per, kb - b0)
                assert nblk >= 1, tag
                cover[b0:b0 + nblk] += 1
            assert (cover == 1).all(), tag
            assert p["first"][k + 1] - p["first"][k] == qb * sp, tag
        assert p["first"][0] == 0
        assert R.host_most(ns) >= min(p["first"][-1], slots), tag
        assert R.host_most([n + 100 for n in ns]) >= min(p["first"][-1], slots), tag
    # the parent's cut
    for np_, per, splits in ((12288, 128, 3), (12352, 129, 3), (16384, 256, 2), (65536, 2048, 1)):
        old = R.plan((np_,), 256, max_per=None)
        assert (old["per"], old["splits"]) == ([per], [splits]), old
    assert [R.first_over_budget(s) for s in (256, 304, 128, 64)] == [12352, 12352, 8256, 6976]
    assert R.plan((6976,), 64, max_per=None)["per"] == [218]


# nce_plan's cut BEFORE the bound, 256 workgroups (R.plan(ns, 256, max_per=None) at the parent commit)
PARENT_PLANS_256 = {
    (1877, 1640): dict(t=7, splits=[9, 8], per=[7, 7], first=[0, 135, 239]),          # the benchmark's step
    (2048,): dict(t=4, splits=[16], per=[4], first=[0, 256]),
    (4096,): dict(t=16, splits=[8], per=[16], first=[0, 256]),
    (8192,): dict(t=64, splits=[4], per=[64], first=[0, 256]),
}


def test_the_bound_leaves_the_plans_up_to_8192_rows_alone():
    for ns, want in PARENT_PLANS_256.items():
        got = R.plan(ns, 256)
        assert {k: got[k] for k in want} == want, ns
        lib = ops.infonce_plan(ns, 256)
        assert (lib["per"], lib["splits"], lib["first"]) == (want["per"], want["splits"], want["first"]), ns
    for np_ in range(R.PAD, R.REUSE_MAX + 1, R.PAD):
        assert R.plan((np_,), 256) == R.plan((np_,), 256, max_per=None), np_
    for ns, slots in _draws(500, seed=12):
        if max(ns) <= R.REUSE_MAX and slots >= 256:
            assert R.plan(ns, slots) == R.plan(ns, slots, max_per=None), (ns, slots)


@pytest.mark.parametrize("n", [2, 17, 65, 300])
@pytest.mark.parametrize("gather", [False, True])
def test_closed_form_is_autograd_of_the_oracle(n, gather):
    d, tau, scale = 24, 0.3, 0.7
    g = torch.Generator().manual_seed(n)
    rows = n + 9 if gather else n
    t1 = torch.randn(rows, d, generator=g, dtype=torch.float64)
    t2 = t1 + 0.3 * torch.randn(rows, d, generator=g, dtype=torch.float64)
    idx = torch.sort(torch.randperm(rows, generator=g)[:n]).values if gather else None
    a, b = t1.clone().requires_grad_(True), t2.clone().requires_grad_(True)
    loss = scale * (O.info_nce(a[idx], b[idx], tau) if gather else O.info_nce(a, b, tau))
    loss.backward()
    for chunk in (2048, 7):
        got_l, g1, g2 = R.info_nce_rows(t1, t2, idx, tau, scale, chunk=chunk)
        assert abs(got_l - loss.item()) <= 1e-12 * abs(loss.item())
        assert float((g1 - a.grad).abs().max()) <= 1e-12 * float(a.grad.abs().max())
        assert float((g2 - b.grad).abs().max()) <= 1e-12 * float(b.grad.abs().max())


def test_case_premises():
    """which edge each case of tests/test_gpu_nce_edges.py is there for, at 256 workgroups"""
    # A: both sides of every tile size, with and without padded keys
    e = {n: R.edges(n) for n in R.A_NS}
    for m in (16, 32, 64, 128, 192):
        assert m - 1 in e and m + 1 in e, m
    assert {n for n in R.A_NS if e[n]["pad_keys"] == 0} == {64, 128}
    assert max(v["pad_keys"] for v in e.values()) == 63 and e[65]["pad_keys"] == 63 and e[2]["pad_keys"] == 62
    assert {v["query_blocks"] for v in e.values()} == {1, 2, 3}
    assert len(R.A_LOW_TAU_NS) * 3 >= len(R.A_NS) and set(R.A_LOW_TAU_NS) <= set(R.A_NS)
    for n in R.A_NS:
        diag, pairs = R.plants(n)
        p = R.problem(n, 64, 5)
        i = p["idx"].astype(np.int64)
        for r in diag:
            assert np.array_equal(p["t1"][i[r]], p["t2"][i[r]])
        for a, b in pairs:
            assert np.array_equal(p["t1"][i[a]], p["t1"][i[b]]) and np.array_equal(p["t2"][i[a]], p["t2"][i[b]])
            assert not np.array_equal(p["t1"][i[a]], p["t2"][i[a]])
        if n >= 3:
            assert 1 in diag                                               # the first tile
        if n >= 32:
            assert any(r // 16 == n // 16 - 1 for r in diag)               # the last full tile
        if n % 16 and n >= 3:
            assert n - 1 in diag                                           # the last partial tile
        if n >= 24:
            assert any(a // 16 == b // 16 for a, b in pairs)
            assert any(a // 16 != b // 16 and a // 32 == b // 32 for a, b in pairs)
        if n >= 131:
            assert any(a // 128 != b // 128 for a, b in pairs)
    assert R.plants(257)[1] == [(4, 9), (14, 18), (40, 129)]
    # B: four problems, each behind the others' tasks
    p = R.plan(R.B_CALLS[0][0], 256)
    assert {k: p[k] for k in R.B_PLAN_256} == R.B_PLAN_256
    assert all(len(ns) >= 2 for ns, _ in R.B_CALLS) and max(len(ns) for ns, _ in R.B_CALLS) == R.MAX_PROBLEMS
    # C: streamed (more blocks than ring slots) with and without the kept weights
    for ns, n_max, d in R.C_CALLS:
        p = R.plan(ns, 256)
        assert max(p["per"]) > R.RING_SLOTS, ns
    reuse = {ns: all(R.pad(m) <= R.REUSE_MAX for m in n_max) for ns, n_max, _ in R.C_CALLS}
    assert reuse == {(4097,): True, (4160,): True, (8192,): True, (8193,): False, (8200, 300): False}
    assert R.plan((4097,), 256)["per"] == [19] and R.plan((4160,), 256)["per"] == [19]
    mixed = R.plan((8200, 300), 256)                  # the small problem: one task per query block, in the recompute form
    assert mixed["splits"][1] == 1 and mixed["per"][1] == mixed["kb"][1] == 10 and mixed["first"] == [0, 195, 198]
    # D: the budget
    assert R.first_over_budget(256) == 12352
    assert R.plan((12288,), 256, max_per=None)["per"] == [128] and R.plan((12352,), 256)["per"] == [97]
    assert R.plan((16384,), 256)["per"] == [128] and R.plan((65536,), 256)["splits"] == [16]
    for n, n_max, d in R.D_FIXED:
        assert R.pad(n_max) <= R.F32_MAX_N
    assert R.pad(R.F32_MAX_N + 1) > R.F32_MAX_N
    # E: split-16 ranges and stages
    per, st = R.split16_ranges(R.pad(64), 64)
    assert per == 32 and [len(s) for s in st] == [1, 1, 0, 0, 0, 0, 0, 0]
    per, st = R.split16_ranges(R.pad(229), 64)
    assert per == 32 and all(s == [32] for s in st)
    per, st = R.split16_ranges(R.pad(256), 64)
    assert (250, 256, 64) in R.E_CASES and per == 32 and st[7] == [32] and 7 * per < 250          # the last range is live
    want = {(2049, 2149, 64): [256, 32], (1025, 1125, 128): [128, 32], (513, 613, 256): [64, 32]}
    for (n, n_max, d), stages in want.items():
        assert (n, n_max, d) in R.E_CASES
        assert R.split16_ranges(R.pad(n_max), d)[1][0] == stages
        assert R.split16_ranges(R.pad(n - 1), d)[1][0] == [R.nce_chunk(d)]          # one row less: one stage per range
    for n, n_max, d in R.E_CASES:
        assert n <= n_max


def _f32_worst():
    worst = {f: (0.0, None) for f in R.FLOORS}
    worst_loss = 0.0
    for name, tau, p in R.small_f32_cases():
        l64, a64, b64 = R.info_nce_rows(p["t1"], p["t2"], p["idx"], tau, 0.3)
        l32, a32, b32 = R.info_nce_rows(p["t1"], p["t2"], p["idx"], tau, 0.3, dtype=torch.float32)
        i = torch.from_numpy(p["idx"].astype(np.int64))
        worst_loss = max(worst_loss, abs(l32 - l64) / abs(l64))
        for f in R.FLOORS:
            e = max(float(R.row_errors(a32[i], a64[i], f).max()), float(R.row_errors(b32[i], b64[i], f).max()))
            if e > worst[f][0]:
                worst[f] = (e, name)
    return worst, worst_loss


def test_floor_and_yardstick():
    """float32 torch of the closed form against float64, per row, on every f32 case of n <= 4160: the floor is the
    smallest at which it stays within half of GRAD_TOL_F32, and ROW_YARDSTICK_NCE is that measurement rounded up (the
    window allows for another CPU's order of reductions; a constant at its low end only makes the GPU bound stricter)"""
    worst, worst_loss = _f32_worst()
    print("float32 torch against float64, worst per-row gradient error by floor:", worst, "loss:", worst_loss)
    passing = [f for f in R.FLOORS if worst[f][0] <= R.GRAD_TOL / 2]
    assert passing and R.FLOOR_FRAC == min(passing), worst
    got = worst[R.FLOOR_FRAC][0]
    assert R.ROW_YARDSTICK_NCE / 3 <= got <= 1.5 * R.ROW_YARDSTICK_NCE, got
    assert R.ROW_BOUND_F32 == R.MARGIN * R.ROW_YARDSTICK_NCE
