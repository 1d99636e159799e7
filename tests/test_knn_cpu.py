"""UserKNN / ItemKNN without a GPU: the float64 restatement (tests/knn_ref.py) reproduces the reference's own run bit for
bit (tests/golden/knn.npz), the models keep the reference's names and config keys, every new entry point is bound, and a
topK over the LDS limit is refused before anything runs."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import knn_ref
from tests.test_shapes_cpu import GOLDEN

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def golden():
    gd = np.load(os.path.join(GOLDEN, "knn.npz"))
    meta = json.load(open(os.path.join(GOLDEN, "knn_meta.json")))
    return gd, meta


def golden_problem(gd):
    """reference ids of the golden's training pairs (file order), both CSRs, the users' item lists, the name ranks"""
    uid = {n: k for k, n in enumerate(gd["user_names"].tolist())}
    iid = {n: k for k, n in enumerate(gd["item_names"].tolist())}
    u = np.asarray([uid[n] for n in gd["train_user"].tolist()], dtype=np.int64)
    i = np.asarray([iid[n] for n in gd["train_item"].tolist()], dtype=np.int64)
    U, I = len(uid), len(iid)
    user_items = [[] for _ in range(U)]
    for a, b in zip(u.tolist(), i.tolist()):
        user_items[a].append(b)
    return dict(u=u, i=i, U=U, I=I, R=knn_ref.binary_csr(u, i, U, I), user_items=user_items, uid=uid, iid=iid,
                user_rank=knn_ref.name_ranks(gd["user_names"].tolist()),
                item_rank=knn_ref.name_ranks(gd["item_names"].tolist()))


def golden_lists(gd, name):
    ptr, ids, sims = gd[f"{name}_nbr_ptr"], gd[f"{name}_nbr_ids"], gd[f"{name}_nbr_sims"].view(np.float64)
    return [(ids[ptr[r]:ptr[r + 1]].astype(np.int64), sims[ptr[r]:ptr[r + 1]]) for r in range(len(ptr) - 1)]


@pytest.mark.parametrize("name,side", [("UserKNN", "user"), ("ItemKNN", "item")])
def test_restatement_reproduces_the_reference_run(name, side):
    gd, meta = golden()
    p = golden_problem(gd)
    a = p["R"] if side == "user" else p["R"].T.tocsr()
    rank = p["user_rank"] if side == "user" else p["item_rank"]
    got = knn_ref.neighbours(a, rank, meta["conf"]["topK"], meta["conf"]["shrinkage"])
    want = golden_lists(gd, name)
    assert len(got) == len(want)
    for (gi, gs), (wi, ws) in zip(got, want):
        assert np.array_equal(gi, wi)
        assert np.array_equal(gs.view(np.uint64), ws.view(np.uint64))
    assert meta[name]["empty_lists"] >= 1 and meta[name]["short_lists"] > meta[name]["empty_lists"]
    for r, user in enumerate(meta["predict_users"]):
        row = knn_ref.score_row(side, p["uid"][user], p["user_items"], want, p["I"])
        assert np.array_equal(row.view(np.uint64), gd[f"{name}_predict"][r])
    if side == "user":
        assert not gd[f"{name}_predict"][meta["predict_users"].index("hermit")].any()
    ids, sc = gd[f"{name}_rec_items"], gd[f"{name}_rec_scores"]
    for r, user in enumerate(gd["test_users"].tolist()):
        u = p["uid"][user]
        ri, rs = knn_ref.rank_row(knn_ref.score_row(side, u, p["user_items"], want, p["I"]), p["user_items"][u], ids.shape[1])
        assert ri == ids[r].tolist()
        assert np.array_equal(np.asarray(rs).view(np.uint64), sc[r])


def test_models_configs_and_launcher():
    from selfrec_amd import main
    from selfrec_amd.model.graph import ItemKNN, UserKNN
    from selfrec_amd.util.conf import ModelConf
    assert "UserKNN" in main.MODELS and "ItemKNN" in main.MODELS
    for mod, cls, attr in ((UserKNN, "UserKNN", "user_sim"), (ItemKNN, "ItemKNN", "item_sim")):
        klass = getattr(mod, cls)
        for method in ("train", "predict", "test", "evaluate", "execute"):
            assert callable(getattr(klass, method)), method
        assert isinstance(getattr(klass, attr), property)
        conf = ModelConf(os.path.join(REPO, "conf", f"{cls}.yaml"))
        assert conf["model"]["name"] == cls and conf["model"]["type"] == "graph"
        assert int(conf["topK"]) == 50 and int(conf["shrinkage"]) == 100


def test_entry_points_are_bound_and_abi_unchanged():
    from selfrec_amd import _lib, ops
    for name in ("srh_knn_neighbours", "srh_knn_score_ws_bytes", "srh_knn_score_topk", "srh_find_k_largest_host_f64"):
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.load(), name), name
    for name in ("knn_neighbours", "knn_score_topk", "knn_score_ws", "find_k_largest_host_f64"):
        assert callable(getattr(ops, name)), name
    assert _lib.ABI_VERSION == 31
    assert _lib.load().srh_knn_score_ws_bytes(1024, 38048) == 1024 * 38048 * 8


def test_topk_over_the_lds_limit_is_refused():
    import torch
    from selfrec_amd import _lib, ops
    z = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(ops.SelfrecHipError, match="128"):
        ops.knn_neighbours(z, z, z, z, z.double(), z, 129, 100)
    with pytest.raises(ops.SelfrecHipError, match="128"):
        ops.knn_score_topk("user", z, z, z, 10, torch.zeros((2, 129), dtype=torch.int32), torch.zeros((2, 129)), z, 20)
    lib = _lib.load()
    dummy = C.c_void_p(16)                   # (refused before any pointer is read or any launch)
    rc = lib.srh_knn_neighbours(dummy, dummy, dummy, dummy, dummy, dummy, 10, None, 10, 129, 100, dummy, dummy, dummy, None)
    assert rc == -1 and b"128" in lib.srh_last_error_string()
    rc = lib.srh_knn_score_topk(0, dummy, 1, dummy, dummy, 1000, dummy, dummy, dummy, 129, 20, 1, dummy, 1, dummy, dummy,
                                None)
    assert rc == -1 and b"128" in lib.srh_last_error_string()


def test_shrinkage_outside_32_bits_is_refused():
    """the C entry point takes int32: 2**32 + 5 would arrive as 5"""
    import torch
    from selfrec_amd import ops
    z = torch.zeros(3, dtype=torch.int32)
    for s in (2 ** 31, 2 ** 32 + 5):
        with pytest.raises(ops.SelfrecHipError, match=r"shrinkage.*2\*\*31"):
            ops.knn_neighbours(z, z, z, z, z.double(), z, 50, s)
    with pytest.raises(ops.SelfrecHipError, match="negative shrinkage"):
        ops.knn_neighbours(z, z, z, z, z.double(), z, 50, -1)


def test_host_heap_walk_f64_matches_heapq():
    from selfrec_amd import ops
    rng = np.random.default_rng(3)
    for n, k in ((1000, 20), (50, 21), (10, 20), (4000, 128)):
        cand = rng.choice(np.asarray([0.0, -10e8, 0.5, 0.9999999900000001, 0.99999999, 1.0 - 2 ** -40]), n)
        cand[rng.integers(n, size=n // 10)] = rng.random(n // 10)
        ids, sc = ops.find_k_largest_host_f64(k, cand)
        ri, rs = knn_ref.find_k_largest(k, cand)
        assert ids.tolist() == ri
        assert np.array_equal(sc, np.asarray(rs))
