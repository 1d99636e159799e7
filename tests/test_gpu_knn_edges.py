"""The KNN kernels (csrc/knn.hip) on every selection path: the cases of tests/knn_cases.py, which
tests/test_knn_edges_cpu.py shows to reach the overflow rounds, the two sides of the buffer's capacity, the running-list
cases of a second pass and the pass boundary, against the restatement of tests/knn_ref.py.  Everything is integers and
separately rounded float64, so every comparison is of bits.  DESIGN.md 4.17."""
import numpy as np
import pytest

from tests import knn_cases
from tests.test_gpu_knn import _t, check_lists, device_side

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    from selfrec_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda", 0)


def run_neighbours(c, dev):
    from selfrec_amd import ops
    return ops.knn_neighbours(*device_side(c["a"], c["rank"], dev), c["k"], c["s"], query_rows=_t(c["rows"], dev, np.int32))


def run_score(c, dev):
    from selfrec_amd import ops
    ui = c["user_items"]
    indptr = np.concatenate([[0], np.cumsum([len(x) for x in ui])])
    items = np.concatenate([np.asarray(x, dtype=np.int64) for x in ui])
    ids, sims, lens = c["nbr"]
    return ops.knn_score_topk(c["mode"], _t(c["users"], dev, np.int32), _t(indptr, dev, np.int32), _t(items, dev, np.int32),
                              c["n_items"], _t(ids, dev, np.int32), _t(sims, dev, np.float64), _t(lens, dev, np.int32),
                              c["n_top"], ws_rows=c["ws_rows"], mask_train=c["mask_train"])


@pytest.mark.parametrize("name", sorted(knn_cases.NEIGHBOUR_CASES))
def test_neighbours_match_the_restatement_on_every_path(dev, name):
    """ids, sim bits, lengths and the -1 / 0 padding.  over_k128_smax fails on a knn_sim that forms n + s in int"""
    c = knn_cases.neighbour_case(name)
    check_lists(*run_neighbours(c, dev), c["want"])


@pytest.mark.parametrize("name", sorted(knn_cases.SCORE_CASES))
def test_score_rows_and_ranking_match_the_restatement(dev, name):
    """the finished workspace rows, the ranked ids and scores of unmarked and marked rows, and where the mark is set"""
    c = knn_cases.score_case(name)
    ids, sc, ws = run_score(c, dev)
    ids, sc = ids.cpu().numpy(), sc.cpu().numpy()
    n_query, n_items = len(c["users"]), c["n_items"]
    ws_rows = min(c["ws_rows"], n_query)
    ws = ws.view(torch.float64)[:ws_rows * n_items].cpu().numpy().reshape(ws_rows, n_items)
    for b in range(ws_rows):                      # workspace row b holds the last user that block b served
        last = b + ((n_query - 1 - b) // ws_rows) * ws_rows
        assert np.array_equal(ws[b].view(np.uint64), c["rows"][last].view(np.uint64)), (b, last)
    for r, (wi, wsc, tied) in enumerate(c["tops"]):
        assert (ids[r, 0] < 0) == tied, r
        got = ids[r].astype(np.int64)
        if tied:
            got[0] = -1 - got[0]
        assert np.array_equal(got, wi), r
        assert np.array_equal(sc[r].view(np.uint64), wsc.view(np.uint64)), r


@pytest.mark.selfcheck
def test_two_calls_of_an_overflow_case_give_the_same_bits(dev):
    c = knn_cases.neighbour_case("over_varied_s10")
    for x, y in zip(run_neighbours(c, dev), run_neighbours(c, dev)):
        assert torch.equal(x, y)
    c = knn_cases.score_case("over_user_26624_n20")
    a, b = run_score(c, dev), run_score(c, dev)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
