"""The premises of tests/test_gpu_knn_edges.py, without a GPU: every case of tests/knn_cases.py reaches the path of
csrc/knn.hip it is named for, by the predictor of tests/knn_ref.py; the predictor agrees with a literal, thread by thread
walk; the restatement agrees with heapq.nlargest in pure Python at heavy ties; rank_top agrees with find_k_largest on untied
rows and flags exactly the tied ones.  The predictor's tuples are printed (pytest -s) and are DESIGN.md 4.17's."""
import heapq
import math

import numpy as np
import pytest

from tests import knn_cases, knn_ref
from tests.test_knn_cpu import golden, golden_problem

NB, SC = sorted(knn_cases.NEIGHBOUR_CASES), sorted(knn_cases.SCORE_CASES)


def python_keys(c, q):
    """[(sim, name rank, row)] of every candidate of query row q, in python floats and sets"""
    a, s = c["a"], c["s"]
    feats = [set(a.indices[a.indptr[r]:a.indptr[r + 1]].tolist()) for r in range(a.shape[0])]
    keys = []
    for v in range(a.shape[0]):
        n = len(feats[q] & feats[v])
        if n > 0 and v != q:
            sim = (n / (n + s)) * (n / (math.sqrt(len(feats[q])) * math.sqrt(len(feats[v])) + 1e-8))
            keys.append((sim, int(c["rank"][v]), v))
    return keys


def walk_neighbour_passes(keys, n_rows, k):
    """knn_neighbours_kernel's partition, literally: thread maxima, their k-th best, the keys at or above the bound"""
    sentinel, out, kept = (-1.0, -1), [], []
    for c0 in range(0, n_rows, knn_ref.NB_CHUNK):
        mine = [(s, r, v) for s, r, v in keys if c0 <= v < c0 + knn_ref.NB_CHUNK]
        best = [sentinel] * knn_ref.NB_THREADS
        for s, r, v in mine:
            t = (v - c0) % knn_ref.NB_THREADS
            best[t] = max(best[t], (s, r))
        bound = sorted(best, reverse=True)[k - 1]
        raised = len(kept) == k and kept[-1][:2] > bound
        if raised:
            bound = kept[-1][:2]
        total = sum(key[:2] >= bound for key in mine) + sum(key[:2] >= bound for key in kept)
        out.append((total, len(kept), raised))
        kept = heapq.nlargest(k, kept + mine)
    return out


@pytest.mark.parametrize("name", NB)
def test_neighbour_case_reaches_its_path(name):
    c = knn_cases.neighbour_case(name)
    print(f"\n{name}: n_rows {c['a'].shape[0]}, K {c['k']}, s {c['s']}, rows {c['rows'].tolist()}: {c['predicted']}")
    assert c["predicted"] == knn_cases.NEIGHBOUR_PASSES[name]
    over = any(total > knn_ref.NB_CAP for passes in c["predicted"] for total, _, _ in passes)
    assert over == ("over" in name)
    assert all(len(p) == -(-c["a"].shape[0] // knn_ref.NB_CHUNK) for p in c["predicted"])


@pytest.mark.parametrize("name", NB)
def test_predictor_and_restatement_against_plain_python(name):
    """the predictor against the literal walk; knn_ref.neighbours against heapq.nlargest(k, [(sim, name rank), ...])"""
    c = knn_cases.neighbour_case(name)
    done = {}
    for q, passes, (ids, sims) in zip(c["rows"].tolist(), c["predicted"], c["want"]):
        if q not in done:
            keys = python_keys(c, q)
            done[q] = walk_neighbour_passes(keys, c["a"].shape[0], c["k"]), heapq.nlargest(c["k"], keys)
        walked, best = done[q]
        assert passes == walked
        assert ids.tolist() == [v for _, _, v in best]
        assert np.array_equal(sims.view(np.uint64), np.asarray([s for s, _, _ in best]).view(np.uint64))
        assert q not in ids.tolist()


def test_named_properties_of_the_neighbour_cases():
    nc, chunk = knn_cases.neighbour_case, knn_ref.NB_CHUNK
    lo, hi = nc("cap_1024"), nc("over_cap_1025")       # one strong row apart, and nothing else
    diff = (lo["a"] != hi["a"])
    assert diff.nnz == 1 and np.array_equal(lo["rank"], hi["rank"]) and (lo["k"], lo["s"]) == (hi["k"], hi["s"])
    assert lo["predicted"][0][0][0] == knn_ref.NB_CAP and hi["predicted"][0][0][0] == knn_ref.NB_CAP + 1
    assert nc("over_one_pass_exact")["a"].shape[0] == chunk and nc("over_one_wide_last_pass")["a"].shape[0] == chunk + 1
    c = nc("over_one_wide_last_pass")                  # for the second query the one candidate of the last pass comes first
    assert c["want"][1][0][0] == chunk and chunk not in c["want"][0][0].tolist()
    c = nc("over_second_pass_full_list")               # the overflowing second pass keeps entries of the list and adds new ones
    for ids, _ in c["want"][:2]:
        assert 0 < (ids < chunk).sum() < c["k"]
    assert int(c["rows"][0]) >= chunk                  # a query in the second pass
    c = nc("over_query_in_strong_set")
    assert all(q in knn_cases._strong(0, c["a"].shape[0], c["k"]) for q in c["rows"].tolist())
    for name in ("over_varied_s0", "over_varied_s10", "over_second_pass_full_list", "lower_bound"):
        assert any(len(set(sims.tolist())) > 1 for _, sims in nc(name)["want"]), name
    for name in ("tied_identity", "tied_reversed", "over_tied_perm"):
        assert all(len(set(sims.tolist())) == 1 for _, sims in nc(name)["want"]), name
    c = nc("lower_bound")
    rows = c["rows"].tolist()
    assert rows != sorted(rows) and len(set(rows)) < len(rows)
    t = c["a"].T.tocsr()
    t.sort_indices()
    below, above, straddle, exact = (t.indices[t.indptr[f]:t.indptr[f + 1]] for f in range(4))
    assert below.max() < chunk and above.min() > chunk and straddle.min() < chunk < straddle.max() and exact.min() == chunk
    held = [set(c["a"].indices[c["a"].indptr[q]:c["a"].indptr[q + 1]].tolist()) for q in rows]
    assert {0, 2} <= held[1] and {1, 2, 3} <= held[0]
    assert nc("over_k128_smax")["s"] == 2 ** 31 - 1 and nc("over_k128")["s"] == 0
    assert np.array_equal(nc("over_k128_smax")["a"].indices, nc("over_k128")["a"].indices)


# ---- scoring ---------------------------------------------------------------------------------------------------------
def walk_score_pass(row, k1):
    best = [(-math.inf, -(2 ** 31 - 1))] * knn_ref.SC_THREADS       # keys as (score, -id): larger is better
    for i, v in enumerate(row.tolist()):
        best[i % knn_ref.SC_THREADS] = max(best[i % knn_ref.SC_THREADS], (v, -i))
    bound = sorted(best, reverse=True)[k1 - 1]
    return sum((v, -i) >= bound for i, v in enumerate(row.tolist()))


@pytest.mark.parametrize("name", SC)
def test_score_case_reaches_its_path(name):
    c = knn_cases.score_case(name)
    got = [(total, top[2]) for total, top in zip(c["predicted"], c["tops"])]
    print(f"\n{name}: {c['mode']}, n_items {c['n_items']}, N {c['n_top']}, users {c['users']}: {got}")
    assert got == knn_cases.SCORE_TOTALS[name]
    assert (c["predicted"][0] > knn_ref.SC_CAP) == ("over" in name)
    assert all(total <= knn_ref.SC_CAP for total in c["predicted"][1:])
    assert c["predicted"] == [walk_score_pass(row, c["n_top"] + 1) for row in c["rows"]]


@pytest.mark.parametrize("name", SC)
def test_rank_top_agrees_with_the_heap_walk_and_flags_the_tied_rows(name):
    c = knn_cases.score_case(name)
    for row, (ids, scores, tied) in zip(c["rows"], c["tops"]):
        top = np.sort(row)[::-1][:c["n_top"] + 1]
        assert tied == bool((top[1:] == top[:-1]).any())
        assert np.array_equal(scores.view(np.uint64), top[:c["n_top"]].view(np.uint64))
        assert np.array_equal(row[ids], scores)
        if not tied:
            wi, ws = knn_ref.find_k_largest(c["n_top"], row)
            assert ids.tolist() == wi and np.array_equal(scores, np.asarray(ws))
        else:                                                       # (score desc, id asc) inside every run of equals
            assert all(a < b for a, b, x, y in zip(ids[:-1], ids[1:], scores[:-1], scores[1:]) if x == y)


def test_named_properties_of_the_score_cases():
    sc = knn_cases.score_case
    lo, hi = sc("cap_2048"), sc("over_cap_2049")
    assert lo["predicted"] == [knn_ref.SC_CAP] and hi["predicted"] == [knn_ref.SC_CAP + 1]
    assert int((lo["rows"][0] != hi["rows"][0]).sum()) == 1            # one item's score apart
    c = sc("items_21")                                                 # N + 1 == n_items: the -10e8 entries are ranked
    assert c["n_items"] == c["n_top"] + 1
    assert all((top[1] == -10e8).any() for top in c["tops"]) and all(len(c["user_items"][u]) >= 2 for u in c["users"])
    assert [sc(f"items_{n}")["n_items"] for n in (255, 256, 257)] == [255, 256, 257]
    assert not sc("items_257_unmasked")["mask_train"] and not (sc("items_257_unmasked")["rows"][0] == -10e8).any()
    for name in ("heavy_empty_heavy_ws1", "heavy_empty_heavy_ws3"):
        c = sc(name)
        ids, scores, tied = c["tops"][1]                               # the empty list: zeros, marked, ids ascending
        free = np.setdiff1d(np.arange(c["n_items"]), c["user_items"][c["users"][1]])
        assert tied and not scores.any() and np.array_equal(ids, free[:c["n_top"]]) and ids[0] == 1
        assert len(c["lists"][c["users"][0]][0]) > 0 and len(c["lists"][c["users"][2]][0]) > 0
    assert sc("heavy_empty_heavy_ws1")["ws_rows"] == 1 and len(sc("heavy_empty_heavy_ws1")["users"]) == 3
    for name, marked in (("tie_at_the_cut", True), ("tie_below_the_cut", False)):
        row = np.sort(sc(name)["rows"][0])[::-1]
        eq = np.flatnonzero(row[1:31] == row[:30])
        assert eq.tolist() == ([19] if marked else [21]) and sc(name)["tops"][0][2] == marked
    c = sc("item_lists_0_1_128")
    assert c["mode"] == "item" and {0, 1, 128} <= {len(c["lists"][i][0]) for u in c["users"] for i in c["user_items"][u]}
    assert all(c["user_items"][u] != sorted(c["user_items"][u]) for u in (0, 1, 3))
    other = knn_ref.score_row("item", 3, [sorted(x) for x in c["user_items"]], c["lists"], c["n_items"])
    other[c["user_items"][3]] = -10e8
    assert not np.array_equal(other, c["rows"][0])                     # the order of the additions shows
    assert {sc(n)["mode"] for n in SC if "over" in n} == {"user", "item"}


def test_which_path_the_golden_graph_reaches():
    """printed, not asserted: the finding is recorded in DESIGN.md 4.17"""
    gd, _ = golden()
    p = golden_problem(gd)
    for side, a, rank in (("user", p["R"], p["user_rank"]), ("item", p["R"].T.tocsr(), p["item_rank"])):
        for k in (50, 128):
            for s in (0, 100):
                totals = [knn_ref.neighbour_pass_counts(a, rank, q, k, s)[0][0] for q in range(a.shape[0])]
                print(f"\ngolden {side} rows, K {k}, s {s}: largest total {max(totals)}, "
                      f"{sum(t > knn_ref.NB_CAP for t in totals)} of {len(totals)} rows overflow")
