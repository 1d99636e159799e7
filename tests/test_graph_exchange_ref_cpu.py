"""tests/graph_exchange_ref.py against what already stands, without a GPU: its float64 normalisation against the oracle's scipy
statement (oracle.selfrec_oracle.laplacian_of), its fp32 mirror against the stand-in the CPU distributed tests run
(tests/cpu_ops.adj_sym_normalize) bit for bit, and its pack / unpack / scatter against the stand-ins of tests/cpu_ops.py on the
planted cases of tests/test_gpu_graph_exchange_edges.py -- so the CPU distributed tests and the device kernels answer to one
statement."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from oracle import selfrec_oracle as O

from . import cpu_ops
from . import graph_exchange_ref as R


def _dense(indptr, indices, vals, n):
    return sp.csr_matrix((vals, indices, indptr), shape=(n, n)).toarray()


def _keep_emptying_a_row(r, seed):
    """a keep mask over R's row-major interactions that drops a few and every interaction of user 0"""
    keep = (np.random.default_rng(seed).random(r.nnz) < 0.8).astype(np.uint8)
    keep[r.indptr[0]:r.indptr[1]] = 0
    return keep


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_float64_side_is_scipys_laplacian(seed):
    """Bipartite graphs with duplicate-summed weights and an isolated user and item: the float64 side is within 4.5 * 2^-24 of
    scipy's fp32 D^-1/2 A D^-1/2 (four roundings, as a device value has; numpy's fp32 pow is not correctly rounded in general, but
    at these degrees it stays inside the bound), and the mirror with the host's pow table IS scipy's result, whatever pow's last bit."""
    r = R.interactions(7 + seed, 9, seed)
    assert r.data.max() == 2.0 and np.diff(r.indptr).min() == 0
    n = sum(r.shape)
    indptr, indices, edge_id, weight = R.bipartite_csr(r)
    sentinel = np.full(n, R.SENTINEL, dtype=np.float32)
    (d32, v32), (d64, v64) = R.normalize_ref(indptr, indices, edge_id, weight, None, R.host_table(R.max_degree(r) * 2 + 1), 0, sentinel, 0)
    with np.errstate(divide="ignore"):
        want = O.laplacian_of(r).toarray()
    got64, got32 = _dense(indptr, indices, v64, n), _dense(indptr, indices, v32, n)
    assert np.array_equal((want != 0), (got64 != 0))
    assert (np.abs(got64 - want) <= R.NORM_BOUND * np.abs(got64)).all()
    assert np.array_equal(got32.view(np.int32), want.astype(np.float32).view(np.int32))
    assert d32[r.shape[0] - 1] == 0.0 and d64[r.shape[0] + 9 // 2] == 0.0           # the isolated user and item


@pytest.mark.parametrize("seed", [0, 1])
def test_float64_side_with_a_keep_mask_that_empties_a_row(seed):
    """a dropped view is the Laplacian of the kept interactions with unit weights (DeviceGraph.dropped_view)"""
    r = R.interactions(6, 8, 10 + seed, duplicates=False)
    keep = _keep_emptying_a_row(r, seed)
    n = sum(r.shape)
    indptr, indices, edge_id, _ = R.bipartite_csr(r)
    (d32, v32), (_, v64) = R.normalize_ref(indptr, indices, edge_id, None, keep, None, 0, np.zeros(n, np.float32), 0)
    r2 = r.copy()
    r2.data = keep.astype(np.float32)
    r2.eliminate_zeros()
    with np.errstate(divide="ignore"):
        want = O.laplacian_of(r2).toarray()
    got64 = _dense(indptr, indices, v64, n)
    assert np.array_equal((want != 0), (got64 != 0))
    assert (np.abs(got64 - want) <= R.NORM_BOUND * np.abs(got64)).all()
    assert d32[0] == 0.0 and (v32[indptr[0]:indptr[1]].view(np.int32) == 0).all()    # emptied: dinv 0, entries +0.0


def _cpu_normalize(indptr, indices, edge_id, weight, keep, deg_ws, n_vals, n_rows, row_offset, phase):
    t = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a).astype(dt))    # noqa: E731
    ws = torch.from_numpy(deg_ws.copy())
    out = torch.from_numpy(np.full(n_vals, R.SENTINEL, dtype=np.float32))
    cpu_ops.adj_sym_normalize(t(indptr, np.int32), t(indices, np.int32), t(edge_id, np.int32), t(keep, np.uint8), n_rows,
                              weight=t(weight, np.float32), out=out, deg_ws=ws, row_offset=row_offset, phase=phase)
    return ws.numpy(), out.numpy()


@pytest.mark.parametrize("dropped", [False, True])
@pytest.mark.parametrize("world", [1, 2, 3])
def test_fp32_mirror_is_the_cpu_stand_in_bit_for_bit(world, dropped):
    """phase 0 on the whole graph (world 1), phase 1 of every rank into one vector and phase 2 per rank (worlds 2 and 3: a node
    count the world does not divide, so padding rows and non-zero row offsets), with the table DeviceGraph builds"""
    r = R.interactions(7, 10, 20)
    keep = _keep_emptying_a_row(r, 3) if dropped else None
    indptr, indices, edge_id, weight = R.bipartite_csr(r)
    if dropped:
        weight = None
    n = sum(r.shape)
    table = R.host_table(R.max_degree(r) * 2 + 1)
    if world == 1:
        start = np.full(n, R.SENTINEL, dtype=np.float32)
        (d32, v32), _ = R.normalize_ref(indptr, indices, edge_id, weight, keep, table, 0, start, 0)
        ws, out = _cpu_normalize(indptr, indices, edge_id, weight, keep, start, indices.size, n, 0, 0)
        assert np.array_equal(R.bits(d32), R.bits(ws)) and np.array_equal(R.bits(v32), R.bits(out))
        return
    assert n % world
    shards = [R.shard_rows(indptr, indices, rank, world) for rank in range(world)]
    n_pad = shards[0][3]
    mine = theirs = np.full(world * n_pad, R.SENTINEL, dtype=np.float32)
    for rank, (l_indptr, l_cols, entry, _) in enumerate(shards):
        w = None if weight is None else weight[entry]
        (mine, none), _ = R.normalize_ref(l_indptr, l_cols, edge_id[entry], w, keep, table, rank * n_pad, mine, 1)
        theirs, out = _cpu_normalize(l_indptr, l_cols, edge_id[entry], w, keep, theirs, l_cols.size, n_pad, rank * n_pad, 1)
        assert none is None and (R.bits(out) == R.bits(R.SENTINEL)).all()
        assert np.array_equal(R.bits(mine), R.bits(theirs))
    assert not np.isnan(mine).any()
    whole, _ = R.normalize_ref(indptr, indices, edge_id, weight, keep, table, 0, np.zeros(n, np.float32), 0)
    assert np.array_equal(R.bits(mine[R.gather_order(n, world)]), R.bits(whole[0]))
    for rank, (l_indptr, l_cols, entry, _) in enumerate(shards):
        w = None if weight is None else weight[entry]
        (d32, v32), _ = R.normalize_ref(l_indptr, l_cols, edge_id[entry], w, keep, table, rank * n_pad, mine, 2)
        ws, out = _cpu_normalize(l_indptr, l_cols, edge_id[entry], w, keep, mine, l_cols.size, n_pad, rank * n_pad, 2)
        assert np.array_equal(R.bits(d32), R.bits(mine)) and np.array_equal(R.bits(ws), R.bits(mine))
        assert np.array_equal(R.bits(v32), R.bits(out))
        assert np.array_equal(R.bits(v32), R.bits(whole[1][entry]))       # reassembled: the single-rank values, entry by entry


def test_mirror_paths():
    """the mirror's own branches: a planted table is looked up exactly where the degree is integral and inside it, the formula
    elsewhere, an empty row gives 0, a dropped entry +0.0, and phase 2 follows the planted vector"""
    c = R.stride_case(0, weights="quarters", keep="row", table="planted")
    n = c["n"]
    (d32, v32), (d64, v64) = R.normalize_ref(c["indptr"], c["indices"], c["edge_id"], c["weight"], c["keep"], c["table"], 0,
                                             np.full(n, R.SENTINEL, np.float32), 0)
    looked = R.lookup_rows(c["indptr"], c["edge_id"], c["weight"], c["keep"], c["table"])
    assert looked.any() and not looked.all()
    assert np.isin(d32[looked], c["table"]).all()
    assert (np.abs(d32[~looked] - d64[~looked]) <= R.U24 * d64[~looked]).all()
    empty = int(np.argmax(np.diff(c["indptr"])))
    assert d32[empty] == c["table"][0] == 1.0 and d64[empty] == 0.0        # a planted table[0] is what an empty row looks up
    dropped = c["keep"][c["edge_id"]] == 0
    assert dropped.any() and (R.bits(v32[dropped]) == 0).all() and np.isfinite(v32).all()
    planted = (1.0 + np.arange(n) % 5).astype(np.float32)
    (p32, pv), _ = R.normalize_ref(c["indptr"], c["indices"], c["edge_id"], None, None, None, 0, planted, 2)
    rows = np.repeat(np.arange(n), np.diff(c["indptr"]))
    assert np.array_equal(p32, planted) and np.array_equal(pv, planted[rows] * planted[c["indices"]])


# ---------------------------------------------------------------------------------------------------------------------------
# exchange: the stand-ins of tests/cpu_ops.py on the planted cases they can express (one count for u, i and j)
# ---------------------------------------------------------------------------------------------------------------------------
def _cpu_lists(case):
    n = R.seg_counts(case["counts"], case["B"])
    raw = [case["B"] if c is None else c for c in case["counts"]]
    assert n[0] == n[1] == n[2]
    stage = {k: torch.from_numpy(case["idx"][s].copy()) for s, k in enumerate(("u", "i", "j", "uniq_u", "uniq_i"))}
    return cpu_ops.batch_lists(stage, torch.tensor([raw[0], raw[3], raw[4], 0], dtype=torch.int32), case["B"])


def _expressible(cases, at):
    return [c for c in cases if c[at] in R.CPU_COUNTS]


@pytest.mark.parametrize("shape", _expressible(R.PACK_CASES, 3), ids=str)
def test_pack_stand_in_is_the_restatement(shape):
    case = R.pack_case(*shape)
    B = case["B"]
    want, cat, n_cat = R.pack_ref(case["idx"], case["counts"], B, case["tables"])
    send = torch.full(want.shape, 9.0)
    cat_idx, n_dev = torch.full((2 * B,), -7, dtype=torch.int32), torch.full((1,), -7, dtype=torch.int32)
    cpu_ops.batch_pack(_cpu_lists(case), [torch.from_numpy(t) for t in case["tables"]], send, cat_idx=cat_idx, n_cat=n_dev)
    assert np.array_equal(R.bits(send.numpy()), R.bits(want))
    assert not (R.bits(want) == R.bits(R.POISON)).any()
    assert np.array_equal(cat_idx.numpy()[:n_cat], cat) and (cat_idx.numpy()[n_cat:] == -7).all() and int(n_dev) == n_cat


@pytest.mark.parametrize("shape", _expressible(R.UNPACK_CASES, 5), ids=str)
def test_unpack_stand_in_is_the_restatement(shape):
    case = R.unpack_case(*shape)
    B, d = case["B"], case["world"] * case["dl"]
    start = np.full((R.SEGS * B, d), R.SENTINEL, dtype=np.float32)
    want_c, want_g = R.unpack_ref(case["counts"], B, case["recv"], [start] * case["n_tables"], [start] * case["n_grads"])
    compact = [torch.from_numpy(start.copy()) for _ in range(case["n_tables"])]
    grads = [torch.from_numpy(start.copy()) for _ in range(case["n_grads"])]
    cpu_ops.batch_unpack(_cpu_lists(case), torch.from_numpy(case["recv"]), case["world"], case["dl"], compact, grads)
    for got, want in zip(compact + grads, want_c + want_g):
        assert np.array_equal(R.bits(got.numpy()), R.bits(want))
        assert not (R.bits(want) == R.bits(R.POISON)).any()


@pytest.mark.parametrize("family", ["gauss", "dyadic"])
@pytest.mark.parametrize("shape", _expressible(R.SCATTER_CASES, 5), ids=str)
def test_scatter_stand_in_is_the_restatement(shape, family):
    case = R.scatter_case(*shape, family=family)
    B, col0, dl = case["B"], case["col0"], case["dl"]
    local = [torch.from_numpy(b.copy()) for b in case["bases"]]
    cpu_ops.batch_scatter(_cpu_lists(case), [(torch.from_numpy(g), t) for g, t in zip(case["grads"], local)], case["d_full"], col0, dl)
    for g, base, got in zip(case["grads"], case["bases"], local):
        total, m, S, named = R.scatter_ref(case["idx"], case["counts"], B, g, base, col0, dl)
        got = got.numpy()
        assert np.array_equal(R.bits(got[~named]), R.bits(base[~named])) and not np.isnan(got).any()
        if family == "dyadic":
            assert S.max() * 2.0 ** 17 < 2.0 ** 24          # every partial sum is a multiple of 2^-17 below 2^7: exact
            assert np.array_equal(got.astype(np.float64), total)
        else:
            assert (np.abs(got - total) <= m * R.U24 * S).all()
