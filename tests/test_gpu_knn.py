"""UserKNN / ItemKNN on the device (csrc/knn.hip): bit equality with the reference's own run (tests/golden/knn.npz), the
kernels against the float64 restatement (tests/knn_ref.py) at the Yelp2018 and iFashion shapes, edge cases, tied rankings
against the host heap walk, and repeatability."""
import os

import numpy as np
import pytest

from tests import knn_ref
from tests.test_knn_cpu import golden, golden_lists, golden_problem

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    from selfrec_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda", 0)


def _t(a, dev, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)


def device_side(a, rank, dev):
    """knn_neighbours' inputs for the rows of the binary CSR a (columns ascending in the transpose)"""
    t = a.T.tocsr()
    t.sort_indices()
    norm = np.sqrt(np.diff(a.indptr).astype(np.float64))
    return (_t(a.indptr, dev, np.int32), _t(a.indices, dev, np.int32), _t(t.indptr, dev, np.int32),
            _t(t.indices, dev, np.int32), _t(norm, dev, np.float64), _t(rank, dev, np.int32))


def check_lists(ids, sims, lens, want):
    ids, sims, lens = ids.cpu().numpy(), sims.cpu().numpy(), lens.cpu().numpy()
    for r, (wi, ws) in enumerate(want):
        n = len(wi)
        assert lens[r] == n, r
        assert np.array_equal(ids[r, :n], wi), r
        assert np.array_equal(sims[r, :n].view(np.uint64), ws.view(np.uint64)), r
        assert (ids[r, n:] == -1).all() and (sims[r, n:] == 0).all()


def yelp_like(shape):
    from selfrec_amd import synth
    tu, ti, _, _, U, I = synth.make_dataset(shape)
    r = knn_ref.binary_csr(tu, ti, U, I)
    return r, U, I


# ---- the reference's run ---------------------------------------------------------------------------------------------
def build_model(name, tmp_path, shrinkage=None):
    from selfrec_amd.util.conf import ModelConf
    from selfrec_amd.model.graph import ItemKNN, UserKNN
    gd, meta = golden()
    lines = ["training.set: ./train.txt", "test.set: ./test.txt", "model:", f"  name: {name}", "  type: graph",
             "item.ranking.topN: [10,20]", f"topK: {meta['conf']['topK']}", f"shrinkage: {meta['conf']['shrinkage'] if shrinkage is None else shrinkage}",
             "embedding.size: 64", "max.epoch: 20", "batch.size: 2048", "learning.rate: 0.001", "reg.lambda: 0.0001",
             f"output: {tmp_path}/results/"]
    path = os.path.join(tmp_path, f"{name}.yaml")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    train = [[a, b, 1.0] for a, b in zip(gd["train_user"].tolist(), gd["train_item"].tolist())]
    test = [[a, b, 1.0] for a, b in zip(gd["test_user"].tolist(), gd["test_item"].tolist())]
    cls = UserKNN.UserKNN if name == "UserKNN" else ItemKNN.ItemKNN
    return cls(ModelConf(path), train, test), gd, meta


@pytest.mark.parametrize("name,attr", [("UserKNN", "user_sim"), ("ItemKNN", "item_sim")])
def test_model_matches_the_reference_run_bit_for_bit(dev, tmp_path, name, attr):
    model, gd, meta = build_model(name, tmp_path)
    d = model.data
    assert [d.id2user[k] for k in range(d.user_num)] == gd["user_names"].tolist()
    assert [d.id2item[k] for k in range(d.item_num)] == gd["item_names"].tolist()
    model.execute()                          # build, train, test, evaluate: the reference's strings
    assert model.result == meta[name]["ranking_evaluation"]
    want = golden_lists(gd, name)
    ids, sims, lens = model._nbr
    check_lists(ids, sims, lens, want)
    lists = getattr(model, attr)
    names = gd["user_names"] if name == "UserKNN" else gd["item_names"]
    assert len(lists) == len(want)
    for r in (0, 1, len(want) - 1):
        wi, ws = want[r]
        assert lists[names[r]] == [(float(s), names[v]) for v, s in zip(wi.tolist(), ws.tolist())]
    for r, user in enumerate(meta["predict_users"]):
        row = model.predict(user)
        assert row.dtype == np.float64 and row.shape == (d.item_num,)
        assert np.array_equal(row.view(np.uint64), gd[f"{name}_predict"][r]), user
    rec = model.test()
    for r, user in enumerate(gd["test_users"].tolist()):
        row = rec[user]
        assert [d.item[it] for it, _ in row] == gd[f"{name}_rec_items"][r].tolist(), user
        assert np.array_equal(np.asarray([s for _, s in row]).view(np.uint64), gd[f"{name}_rec_scores"][r]), user
    assert model._last_tie_rows > 0          # the golden has tied rows (the hermit's zeros at least): the host walk ran
    if name != "UserKNN":                    # (the golden keeps the lines evaluate() writes for UserKNN's run)
        return
    for user, line in zip(gd["test_users"].tolist()[:5], meta["rec_lines"]):
        cells = ''.join(f" ({it},{s}){'*' if it in d.test_set[user] else ''}" for it, s in rec[user])
        assert user + ':' + cells + '\n' == line


@pytest.mark.parametrize("name,side", [("UserKNN", "user"), ("ItemKNN", "item")])
def test_predict_adds_the_sources_in_the_reference_order(dev, tmp_path, name, side):
    """S / (S + 1e-8) hides the last bits of S unless S is ~1e-8 or less: a shrinkage of 1e9 brings every sim there, so
    predict() rows show the order of the additions.  Sources in the reference's order (neighbours in list order; the
    user's items in training-file order) give the restatement's bits; another order would not (checked below)."""
    model, gd, meta = build_model(name, tmp_path, shrinkage=10 ** 9)
    p = golden_problem(gd)
    a, rank = (p["R"], p["user_rank"]) if side == "user" else (p["R"].T.tocsr(), p["item_rank"])
    model.train()
    lists = knn_ref.neighbours(a, rank, meta["conf"]["topK"], 10 ** 9)
    check_lists(*model._nbr, lists)
    ui = p["user_items"]
    other = [sorted(x) for x in ui] if side == "item" else ui
    reordered = [(i[::-1], s[::-1]) for i, s in lists] if side == "user" else lists
    sensitive = 0
    for user in gd["test_users"].tolist()[:300]:
        u = p["uid"][user]
        want = knn_ref.score_row(side, u, ui, lists, p["I"])
        assert np.array_equal(model.predict(user).view(np.uint64), want.view(np.uint64)), user
        sensitive += not np.array_equal(knn_ref.score_row(side, u, other, reordered, p["I"]), want)
    assert sensitive > 0


@pytest.mark.parametrize("k,s", [(1, 100), (50, 100), (128, 100), (50, 0), (128, 0)])
def test_neighbours_edge_cases_on_the_golden_graph(dev, k, s):
    """K in {1, 50, 128}, s = 0; the golden graph holds an empty list, short lists, identical rows and hubs"""
    from selfrec_amd import ops
    gd, _ = golden()
    p = golden_problem(gd)
    for a, rank in ((p["R"], p["user_rank"]), (p["R"].T.tocsr(), p["item_rank"])):
        want = knn_ref.neighbours(a, rank, k, s)
        check_lists(*ops.knn_neighbours(*device_side(a, rank, dev), k, s), want)
        lens = [len(w[0]) for w in want]
        assert min(lens) == 0 and (k == 1 or min(x for x in lens if x) < k)
    dups = [p["uid"][f"dup{j}"] for j in range(3)]
    ids, sims, _ = ops.knn_neighbours(*device_side(p["R"], p["user_rank"], dev), 128, s,
                                      query_rows=_t(dups, dev, np.int32))
    sims = sims.cpu().numpy()
    for j, u in enumerate(dups):                 # the two copies come first, tied, the larger name first
        others = [v for v in dups if v != u]
        top = ids[j, :2].cpu().numpy().tolist()
        assert sorted(top) == sorted(others) and sims[j, 0] == sims[j, 1]
        assert p["user_rank"][top[0]] > p["user_rank"][top[1]]


@pytest.mark.parametrize("shape,n_rows", [("yelp2018", 512), ("ifashion", 256)])
def test_neighbours_match_the_restatement_at_scale(dev, shape, n_rows):
    """seeded rows plus the max-degree row; iFashion's 300 k users take ten candidate chunks"""
    from selfrec_amd import ops
    r, U, I = yelp_like(shape)
    rng = np.random.default_rng(17)
    sides = [(r, rng.permutation(U).astype(np.int64))]
    if shape == "yelp2018":
        sides.append((r.T.tocsr(), rng.permutation(I).astype(np.int64)))
    for a, rank in sides:
        deg = np.diff(a.indptr)
        rows = np.unique(np.concatenate([rng.choice(a.shape[0], n_rows - 1, replace=False), [int(np.argmax(deg))]]))
        want = knn_ref.neighbours(a, rank, 50, 100, rows=rows)
        check_lists(*ops.knn_neighbours(*device_side(a, rank, dev), 50, 100, query_rows=_t(rows, dev, np.int32)), want)


@pytest.mark.parametrize("side", ["user", "item"])
def test_ranking_and_tied_rows_match_the_heap_walk(dev, side):
    """knn_score_topk + the host walk over the marked rows == find_k_largest on the restated rows, every golden test
    user; the marked rows really are the tied ones"""
    from selfrec_amd import ops
    gd, meta = golden()
    p = golden_problem(gd)
    a, rank = (p["R"], p["user_rank"]) if side == "user" else (p["R"].T.tocsr(), p["item_rank"])
    nb = ops.knn_neighbours(*device_side(a, rank, dev), 50, 100)
    lists = [(i, s) for i, s in zip(*[x.cpu().numpy() for x in nb[:2]])]
    lists = [(i[:n].astype(np.int64), s[:n]) for (i, s), n in zip(lists, nb[2].cpu().numpy())]
    ui = p["user_items"]
    indptr = np.concatenate([[0], np.cumsum([len(x) for x in ui])])
    items = np.concatenate([np.asarray(x, dtype=np.int64) for x in ui])
    users = np.asarray([p["uid"][u] for u in gd["test_users"].tolist()], dtype=np.int32)
    ids, sc, ws = ops.knn_score_topk(side, _t(users, dev, np.int32), _t(indptr, dev, np.int32), _t(items, dev, np.int32),
                                     p["I"], *nb, 20, ws_rows=64)
    ids, sc = ids.cpu().numpy(), sc.cpu().numpy()
    marked = 0
    for r, u in enumerate(users.tolist()):
        row = knn_ref.score_row(side, u, ui, lists, p["I"])
        wi, wsc = knn_ref.rank_row(row, ui[u], 20)
        masked = row.copy()
        masked[ui[u]] = -10e8
        top = np.sort(masked)[::-1][:21]
        tied = bool((top[1:] == top[:-1]).any())
        assert (ids[r, 0] < 0) == tied, r
        if tied:
            marked += 1
            hi, hs = ops.find_k_largest_host_f64(20, masked)
            assert hi.tolist() == wi and np.array_equal(hs, np.asarray(wsc))
        else:
            assert ids[r].tolist() == wi and np.array_equal(sc[r], np.asarray(wsc))
    assert marked > 0


def test_two_calls_at_the_yelp_shape_give_the_same_bits(dev):
    from selfrec_amd import ops
    r, U, I = yelp_like("yelp2018")
    rank = np.random.default_rng(5).permutation(U)
    args = device_side(r, rank, dev)
    first = ops.knn_neighbours(*args, 50, 100)
    second = ops.knn_neighbours(*args, 50, 100)
    for x, y in zip(first, second):
        assert torch.equal(x, y)
    users = torch.arange(0, U, 7, dtype=torch.int32, device=dev)
    ip, ix = _t(r.indptr, dev, np.int32), _t(r.indices, dev, np.int32)
    a = ops.knn_score_topk("user", users, ip, ix, I, *first, 20, ws_rows=512)
    b = ops.knn_score_topk("user", users, ip, ix, I, *first, 20, ws_rows=512)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
