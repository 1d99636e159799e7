"""The premises of tests/contrastive_ref.py, checked without a GPU: the float64 route, the float32
restatement of the k-means update, the chunk layouts the case list claims, the gap condition under which k-means ids
are exact, the choice of the per-row floor, and the underflow envelope of exp((s - 1) / tau)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import contrastive_ref as R
from tests import ncl_ref


# ---- the float64 route ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,d,tau", [(5, 7, 8, 0.2), (17, 3, 50, 1.0), (1, 66, 64, 0.05)])
def test_float64_route_equals_direct_autograd(B, N, d, tau):
    q, t, idx = R.table_problem(B, N, d, "ends", B + N)
    loss, gq, gt = R.table_nce(q, t, idx, tau, 1.5)
    q_, t_ = q.double().requires_grad_(True), t.double().requires_grad_(True)
    ls = F.log_softmax(F.normalize(q_, dim=1) @ F.normalize(t_, dim=1).T / tau, dim=1)
    direct = -1.5 * ls[torch.arange(B), idx].sum()
    direct.backward()
    assert abs(loss - float(direct.detach())) <= 1e-12 * abs(loss)
    assert float((gq - q_.grad).abs().max()) <= 1e-12 * float(gq.abs().max())
    assert float((gt - t_.grad).abs().max()) <= 1e-12 * float(gt.abs().max())

    u, v = R.softmax_problem(max(B, 2), d)
    loss, gu, gv = R.batch_softmax(u, v, tau)
    u_, v_ = u.double().requires_grad_(True), v.double().requires_grad_(True)
    ls = F.log_softmax(F.normalize(u_, dim=1) @ F.normalize(v_, dim=1).T / tau, dim=1)
    direct = -torch.log(torch.exp(ls.diagonal()) + 1e-5).mean()
    direct.backward()
    assert abs(loss - float(direct.detach())) <= 1e-12 * abs(loss)
    assert float((gu - u_.grad).abs().max()) <= 1e-12 * float(gu.abs().max())
    assert float((gv - v_.grad).abs().max()) <= 1e-12 * float(gv.abs().max())


def test_row_errors_sees_a_small_row_under_a_hub():
    want = torch.tensor([[100.0, -50.0], [1.0, 0.5], [1e-6, 0.0]], dtype=torch.float64)
    got = want.clone()
    got[1, 0] += 1e-3                      # 1e-3 of its own row, 1e-5 of the tensor's largest magnitude
    got[2, 1] += 1e-3                      # a row below the floor is measured against the floor
    e = R.row_errors(got, want, 1e-2)
    assert e[0] == 0 and abs(float(e[1]) - 1e-3) < 1e-9 and abs(float(e[2]) - 1e-3) < 1e-9
    z = R.row_errors(torch.zeros(2, 2), torch.zeros(2, 2), 1e-2)
    assert (z == 0).all() and torch.isinf(R.row_errors(torch.ones(2, 2), torch.zeros(2, 2), 1e-2)).all()


# ---- the case lists say what they claim -----------------------------------------------------------------------------
def test_table_shapes_cover_the_edges():
    S = R.TABLE_SHAPES
    assert {b for b, *_ in S} == {1, 15, 16, 17, 63, 64, 65, 129}
    assert {n for _, n, *_ in S} == {1, 2, 63, 64, 65, 127, 128, 129, 257}
    assert {d for *_, d, _ in S} == {1, 50, 64, 100, 128} and {t for *_, t in S} == {0.03, 0.2, 1.0}
    assert any(b > n for b, n, *_ in S)
    at_one = [(b, n) for b, n, _, tau in S if tau == 1.0]
    assert {n for n in (1, 2, 63, 65, 127, 129, 257)} <= {n for _, n in at_one}
    assert {b for b in (1, 15, 17, 63, 65, 129)} <= {b for b, _ in at_one}
    calls = R.table_calls()
    assert len(calls) == len(S) + len(R.CHUNK_CALLS)
    # a d = 1 shape (exact-zero gradients) comes again as the second problem of the call before it, at d > 1 and, where
    # its own tau is 1, at tau = 1: there its gradients go through row_errors
    for i, (b, n, d, tau) in enumerate(S):
        if d == 1:
            _, ptau, pprobs = calls[i - 1]
            assert i > 0 and S[i - 1][2] > 1 and (len(pprobs[1][0]), len(pprobs[1][1])) == (b, n)
            assert pprobs[1][0].shape[1] == S[i - 1][2] and (tau != 1.0 or ptau == 1.0)
    fams = set()
    for i, (b, n, _, _) in enumerate(S):
        fams.add(R._family(i, b, n))
    assert fams == set(R.IDX_FAMILIES)
    for _, _, probs in calls:
        assert len(probs) == 2 and probs[0][3] != probs[1][3]
        for q, t, idx, _ in probs:
            assert 0 <= int(idx.min()) and int(idx.max()) < len(t) and len(idx) == len(q)
    # last_tile: positives only in the last partial tile
    q, t, idx = R.table_problem(63, 257, 50, "last_tile", 1)
    assert (idx == 256).all()
    q, t, idx = R.table_problem(64, 127, 64, "last_tile", 1)
    assert int(idx.min()) >= 64 and len(set(idx.tolist())) > 10


def test_chunk_layouts():
    p = R.chunk_plan(512, 4100)
    assert (p["chunks"], p["chunk_len"], p["live"], p["empty"], p["last_keys"]) == (64, 128, 33, 31, 4)
    p = R.chunk_plan(16400, 130)
    assert (p["chunks"], p["chunk_len"], p["live"], p["empty"], p["last_keys"]) == (2, 128, 2, 0, 2)
    p = R.chunk_plan(32769, 130)
    assert (p["chunks"], p["chunk_len"], p["live"], p["empty"]) == (1, 192, 1, 0)
    p = R.chunk_plan(65, 257)
    assert (p["chunks"], p["chunk_len"], p["tiles"], p["live"], p["last_keys"]) == (5, 64, 5, 5, 1)
    # the shapes of test_gpu_ncl.py: never one chunk, never a last chunk of a few keys, and empty trailing chunks only at
    # (257, 38048), which leaves 3 of 103
    for B, N in ((1, 300), (257, 300), (2048, 300), (1, 31668), (257, 38048), (2048, 31668), (2048, 38048)):
        p = R.chunk_plan(B, N)
        assert p["chunks"] > 1 and p["last_keys"] > 2 and p["empty"] == (3 if (B, N) == (257, 38048) else 0)
    # the schedule covers the table: chunks * chunk_len >= N, whatever is left empty
    for B in (1, 63, 64, 65, 512, 4096, 16400, 32769):
        for N in (1, 2, 64, 65, 130, 257, 4100, 38048):
            p = R.chunk_plan(B, N)
            assert p["chunks"] * p["chunk_len"] >= N and p["chunk_len"] % 64 == 0 and 1 <= p["live"] <= p["chunks"]


# ---- k-means --------------------------------------------------------------------------------------------------------
def test_update_restatement():
    seen = set()
    for (n, k, d), (x, ids) in zip(R.UPDATE_SHAPES, R.update_cases()):
        cent, counts = R.kmeans_update_f32(x, ids, k)
        ok = (ids >= 0) & (ids < k)
        want_c, want_n = ncl_ref.update_np(x[ok], ids[ok].astype(np.int64), k)
        assert np.array_equal(counts, want_n)
        assert float(R.row_errors(cent, want_c, R.FLOOR_FRAC).max()) <= 1e-6, (n, k, d)
        assert (cent[counts == 0] == 0).all()
        seen |= set(counts.tolist())
        if counts.max() == ok.sum() == n:
            seen.add("all")
        if n >= 7 and not (n == 7 and k == 1):
            assert {-1, k, 2 ** 31 - 1} & set(ids.tolist())
    assert {0, 1, 7, 8, 9, "all"} <= seen
    assert {n for n, _, _ in R.UPDATE_SHAPES} == {1, 7, 8, 9, 255, 256, 257, 513}
    assert {k for _, k, _ in R.UPDATE_SHAPES} == {1, 3, 5, 37, 1025, 2049}
    assert {d for _, _, d in R.UPDATE_SHAPES} == {1, 3, 50, 64, 65, 128, 200}
    # the clusters that exist only because km_scan rounds k / 1024 up hold rows, and so do their thread-mates below
    for (n, k, d), (x, ids) in zip(R.UPDATE_SHAPES, R.update_cases()):
        if k > 1024:
            _, counts = R.kmeans_update_f32(x, ids, k)
            per = -(-k // 1024)
            assert k // 1024 < per and counts[k - 1] == 3 and counts[k - 2] > 0 and counts[k - 3] > 0
            assert (k - 1) // per == (k - 3) // per or k == 1025           # k = 2049: one thread owns 2046..2048
            assert k == 1025 or (counts[1024] > 0 and counts[1023] > 0)
            assert counts[:k - 3].sum() > 0                                 # start[k - 1] is not 0
    x, ids = R.update_cases()[-1]
    cent, counts = R.kmeans_update_f32(x, ids, 3)
    assert not counts.any() and not cent.any()


def test_update_order_is_observable():
    """a pairwise float32 sum of the same rows differs from the ascending-row sum in at least one bit: the order the
    header states can be told from another"""
    i = R.UPDATE_SHAPES.index((513, 1, 128))
    x, ids = R.update_cases()[i]
    cent, counts = R.kmeans_update_f32(x, ids, 1)
    rows = np.ascontiguousarray(x[ids == 0].T)                       # (d, count): numpy sums the last axis pairwise
    pairwise = rows.sum(axis=1, dtype=np.float32) * (np.float32(1) / np.float32(counts[0]))
    assert counts[0] > 400 and (pairwise != cent[0]).any()
    assert np.abs(pairwise.astype(np.float64) - cent[0]).max() <= 1e-6 * np.abs(cent[0]).max()


def test_assign_cases_meet_the_gap_condition():
    assert {n for n, _, _ in R.ASSIGN_SHAPES} == {1, 15, 17, 63, 64, 65, 130}
    assert {k for _, k, _ in R.ASSIGN_SHAPES} == {1, 2, 63, 64, 65, 129, 1025}
    assert {d for _, _, d in R.ASSIGN_SHAPES} == {3, 50, 64, 100, 128}
    offsets, neg_k, tail_copy, tail_winner = set(), set(), 0, set()
    for i, ((n, k, d), cs) in enumerate(zip(R.ASSIGN_SHAPES, R.assign_cases())):
        x, c = cs["x"], cs["c"]
        dist, best, gap = R.assign_f64(x, c)
        dbest, dgap, scale = R.distinct_gap(x, c)
        assert np.array_equal(best, dbest)
        assert (dgap >= R.GAP_FRAC * scale).all(), (n, k, d)
        tied = gap < R.GAP_FRAC * scale                               # only the planted copies, and the lowest id wins
        originals = {a for a, _ in cs["copies"]}
        assert all(int(b) in originals for b in best[tied])
        assert (gap[tied] == 0).all()
        for a, b in cs["copies"]:
            assert np.array_equal(c[a], c[b]) and a < b
            offsets.add(b - a)
            tail_copy += b >= (k - 1) // 64 * 64 and k % 64 != 0 and k > 64
        kinds = np.array(cs["kinds"])
        if (kinds == "tie").any():
            assert tied[kinds == "tie"].all()
        neg = kinds == "neg"
        if neg.any():
            neg_k.add(k)
            c64 = c.astype(np.float64)
            part = (c64 * c64).sum(1)[None, :] - 2.0 * x[neg].astype(np.float64) @ c64.T
            assert part.min() > 0                                     # a padded centroid scoring 0 would win here
        on = (kinds == "on") | (kinds == "last")
        if on.any():
            assert (dist[on, best[on]] == 0).all()
        if i in R.ASSIGN_TAIL_ROW:                                     # a winner in the trailing partial tile
            assert k % 64 and k > 64 and kinds[-1] == "last" and best[-1] == k - 1 >= (k - 1) // 64 * 64
            assert not any(k - 1 in p for p in cs["copies"])
            tail_winner.add(k)
    assert offsets >= set(R.COPY_OFFSETS) and tail_copy >= 1 and tail_winner == {65, 129}
    assert neg_k >= {1, 2, 63, 65, 129, 1025}


# ---- the per-row floor ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _f32_torch_worst():
    """{floor: the worst per-row error of the reference's expressions in float32 torch against float64, over every loss
    case with a non-zero gradient}, and the worst loss error"""
    worst, worst_loss = {f: 0.0 for f in R.FLOORS}, 0.0

    def take(l32, g32, l64, g64, groups=(None, None)):
        """groups: per tensor, the clamped rows -- they and the others are measured each on their own, as on the GPU"""
        nonlocal worst_loss
        worst_loss = max(worst_loss, abs(l32 - l64) / abs(l64))
        for f in R.FLOORS:
            for a, b, rows in zip(g32, g64, groups):
                masks = [slice(None)]
                if rows is not None:
                    m = torch.zeros(len(b), dtype=torch.bool)
                    m[list(rows)] = True
                    masks = [m, ~m]
                for m in masks:
                    worst[f] = max(worst[f], float(R.row_errors(a[m], b[m], f).max()))

    for _, tau, probs in R.table_calls():
        for q, t, idx, scale in probs:
            if R.is_zero_gradient(len(t), q.shape[1]):
                continue
            l64, *g64 = R.table_nce(q, t, idx, tau, scale)
            l32, *g32 = R.table_nce(q, t, idx, tau, scale, dtype=torch.float32)
            take(l32, g32, l64, g64)
    for B in R.SOFTMAX_B[1:]:
        for d in R.SOFTMAX_D:
            for tau in R.SOFTMAX_TAU:
                u, v = R.softmax_problem(B, d)
                l64, *g64 = R.batch_softmax(u, v, tau)
                l32, *g32 = R.batch_softmax(u, v, tau, dtype=torch.float32)
                take(l32, g32, l64, g64)
    for softmax in (False, True):
        q, t, idx, tau = R.envelope_problem("inside", softmax)
        fn = (lambda **kw: R.batch_softmax(q, t, tau, **kw)) if softmax else (lambda **kw: R.table_nce(q, t, idx, tau, 1.0, **kw))
        l64, *g64 = fn()
        l32, *g32 = fn(dtype=torch.float32)
        take(l32, g32, l64, g64)
    c = R.DEGENERATE
    q, t, idx = R.degenerate_problem()
    l64, *g64 = R.table_nce(q, t, idx, c["tau"], 1.0)
    l32, *g32 = R.table_nce(q, t, idx, c["tau"], 1.0, dtype=torch.float32)
    take(l32, g32, l64, g64, (c["clamped_q"], c["clamped_t"]))
    z = R.SOFTMAX_ZERO
    u, v = R.softmax_problem(z["B"], z["d"], seed=z["seed"], zero_rows=True)
    l64, *g64 = R.batch_softmax(u, v, z["tau"])
    l32, *g32 = R.batch_softmax(u, v, z["tau"], dtype=torch.float32)
    take(l32, g32, l64, g64, ((z["u_row"],), (z["v_row"],)))
    return worst, worst_loss


def test_floor_frac_is_the_smallest_that_float32_torch_meets():
    worst, worst_loss = _f32_torch_worst()
    print("float32 torch against float64, worst per-row gradient error by floor:", worst, "loss:", worst_loss)
    passing = [f for f in R.FLOORS if worst[f] <= R.GRAD_TOL / 2]
    assert passing and R.FLOOR_FRAC == min(passing), worst
    assert worst_loss <= R.LOSS_TOL / 2


def test_zero_gradient_cases_are_zero():
    for _, tau, probs in R.table_calls():
        for q, t, idx, scale in probs:
            if R.is_zero_gradient(len(t), q.shape[1]):
                _, gq, gt = R.table_nce(q, t, idx, tau, scale)
                sq, st = R.cancel_scales(q, t, idx, tau, scale)
                assert (gq.abs().amax(1) <= 1e-12 * sq).all() and (gt.abs().amax(1) <= 1e-12 * st).all()


def test_degenerate_rows_in_float64():
    c = R.DEGENERATE
    q, t, idx = R.degenerate_problem()
    assert c["zero_t"] not in idx.tolist() and c["zero_t_pos"] in idx.tolist() and c["tiny_t"] in idx.tolist()
    assert float(q[c["tiny_q"]].double().norm()) < 1e-12 and float(t[c["tiny_t"]].double().norm()) < 1e-12
    loss, gq, gt = R.table_nce(q, t, idx, c["tau"], 1.0)
    assert np.isfinite(loss) and torch.isfinite(gq).all() and torch.isfinite(gt).all()
    # the clamped rows' gradients are g / 1e-12: no projection, and twelve orders above the others
    for x, r in ((q, c["near_q"]), (t, c["near_t"])):              # just below the clamp, in float32 as in float64
        assert 0.7e-12 < float(x[r].norm()) < 0.9e-12 and 0.7e-12 < float(x[r].double().norm()) < 0.9e-12
    assert c["near_t"] in idx.tolist()
    for g, rows in ((gq, c["clamped_q"]), (gt, c["clamped_t"])):
        big = g.abs().amax(1)
        mask = torch.zeros(len(g), dtype=torch.bool)
        mask[list(rows)] = True
        assert (big[mask] > 1e9).all() and (big[~mask] < 1e3).all()
    # the near-clamp rows tell the clamped backward from the unclamped one: projecting changes them by far more than 1e-4
    for g, x, r in ((gq, q, c["near_q"]), (gt, t, c["near_t"])):
        y = x[r].double() / 1e-12
        assert float((y * (y @ g[r])).abs().max()) > 1e-2 * float(g[r].abs().max())


# ---- the underflow envelope -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("softmax", [False, True])
def test_underflow_envelope(softmax):
    tiny = R.F32_MIN_NORMAL
    for kind in ("outside", "band"):
        q, t, idx, tau = R.envelope_problem(kind, softmax)
        cos0 = (F.normalize(q.double(), dim=1) @ F.normalize(t.double(), dim=1).T)[0]
        assert float(cos0.max()) < 1 - 87 * tau
        e0 = R.shifted_terms_f32(q, t, tau)[0]
        assert (e0 < tiny).all()                                   # every term of query 0 is zero or subnormal
        assert float(e0.double().sum()) < len(t) * 2.0 ** -130     # below the guard of ct_finish
        if kind == "band":
            assert abs(float(cos0.max()) - 0.05) < 1e-3
        else:
            assert float(cos0.max()) <= -0.95 + 1e-6 and (e0 == 0).all()
        ref = R.batch_softmax(q, t, tau) if softmax else R.table_nce(q, t, idx, tau, 1.0)
        assert np.isfinite(ref[0]) and torch.isfinite(ref[1]).all() and torch.isfinite(ref[2]).all()
    q, t, idx, tau = R.envelope_problem("inside", softmax)
    assert tau >= 0.023
    e = R.shifted_terms_f32(q, t, tau)
    assert (e >= tiny).all() and (e.double().sum(1) >= len(t) * 2.0 ** -130).all()
    # ... and the shifted float32 terms give the float64 softmax of every row to float32 accuracy
    p32 = e.double() / e.double().sum(1, keepdim=True)
    p64 = torch.softmax(F.normalize(q.double(), dim=1) @ F.normalize(t.double(), dim=1).T / tau, dim=1)
    assert float(((p32 - p64).abs() / p64).max()) <= 1e-4
    # for tau >= 0.023 no data reaches either band: the smallest possible term is exp(-2 / tau)
    assert np.exp(np.float32(-2.0 / 0.023)) >= tiny
