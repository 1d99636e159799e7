"""The kernels that move whole graphs and whole batches -- degree_kernel / normalize_kernel (csrc/graph.hip, behind
srh_adj_sym_normalize) and pack_kernel / unpack_kernel / scatter_kernel (csrc/exchange.hip, behind srh_batch_pack / unpack / scatter)
-- each in ONE launch against the restatement in tests/graph_exchange_ref.py, on its planted cases.

Three kinds of bound and no other: bit equality (everything the header states as an order of fp32 operations, and
every pure move), 4.5 * 2^-24 relative to the float64 truth for a normalised value, m * 2^-24 * S for an element that m atomic
fp32 additions built.  Whatever a call may write starts as a NaN with one payload (SENTINEL: what still holds it was not written),
whatever it must not read holds a NaN with another (POISON: it shows wherever it arrives)."""
import numpy as np
import pytest
import torch

from selfrec_amd import _lib, ops
from selfrec_amd.data.device_graph import DeviceGraph, ShardedDeviceGraph

from . import graph_exchange_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT_BITS, POISON_BITS = int(R.bits(R.SENTINEL)[0]), int(R.bits(R.POISON)[0])


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def sentinel(shape):
    return np.full(shape, R.SENTINEL, dtype=np.float32)


# ---------------------------------------------------------------------------------------------------------------------------
# normalisation: one launch against the restatement
# ---------------------------------------------------------------------------------------------------------------------------
def run_norm(c, phase, row_offset, deg_in):
    """one srh_adj_sym_normalize call on the case from a given D^-1/2 vector and sentinel values: (deg_ws, vals) as it leaves them"""
    deg_ws, vals = dev(deg_in), dev(sentinel(c["indices"].size))
    ops.adj_sym_normalize(dev(c["indptr"]), dev(c["indices"]), dev(c["edge_id"]), dev(c["keep"]), c["indptr"].size - 1,
                          weight=dev(c["weight"]), out=vals, deg_ws=deg_ws, inv_sqrt_table=dev(c["table"]), row_offset=row_offset,
                          phase=phase)
    return host(deg_ws), host(vals)


def check_norm(c, got, phase, row_offset, deg_in, truth=True, tag=""):
    got_deg, got_vals = got
    (d32, v32), (_, v64) = R.normalize_ref(c["indptr"], c["indices"], c["edge_id"], c["weight"], c["keep"], c["table"], row_offset,
                                           deg_in, phase)
    # the header's contract on the table path, the correctly rounded float32 of a float64 on the formula path; every slot the
    # call does not own keeps its bits
    assert np.array_equal(R.bits(got_deg), R.bits(d32)), f"{tag}: D^-1/2 differs from the fp32 mirror"
    if phase == 1:
        assert (R.bits(got_vals) == SENT_BITS).all(), f"{tag}: phase 1 wrote values"
        return
    assert np.isfinite(got_vals).all(), tag
    if c["keep"] is not None:
        dropped = c["keep"][c["edge_id"]] == 0
        assert (R.bits(got_vals[dropped]) == 0).all(), f"{tag}: a dropped entry is not +0.0"
    # two fp32 products of the D^-1/2 entries, left to right: with those bit-equal, so are the values
    assert np.array_equal(R.bits(got_vals), R.bits(v32)), f"{tag}: values differ from the fp32 mirror"
    if truth:
        err = np.abs(got_vals.astype(np.float64) - v64)
        worst = float((err / np.where(v64 != 0, np.abs(v64), 1.0)).max(initial=0.0))
        print(f"{tag}: worst value error {worst / R.U24:.2f} * 2^-24 of the float64 truth (bound 4.5)")
        assert (err <= R.NORM_BOUND * np.abs(v64)).all(), tag


AXES = [("none", "none", "none"), ("ints", "some", "cover"), ("quarters", "row", "short"), ("ints", "none", "short"),
        ("quarters", "some", "none"), ("none", "row", "cover"), ("ints", "row", "planted"), ("quarters", "some", "cover")]
SMALL = [(n, AXES[(3 * k + j) % len(AXES)]) for k, n in enumerate((1, 2, 3, 4, 5, 9)) for j in range(3)]


def check_paths(c, got_deg, axes):
    """the case reaches what its axes promise: a looked-up row and a formula row where the table is short or the degrees are not
    integral, and an empty row whose D^-1/2 was written as 0 over the sentinel"""
    looked = R.lookup_rows(c["indptr"], c["edge_id"], c["weight"], c["keep"], c["table"])
    if axes[2] == "none":
        assert not looked.any()
    if axes[2] == "cover" and axes[0] != "quarters":
        assert looked.all()
    w = np.ones(c["indices"].size) if c["weight"] is None else c["weight"]
    kept = np.ones(w.size, dtype=bool) if c["keep"] is None else c["keep"][c["edge_id"]] != 0
    deg = np.bincount(np.repeat(np.arange(c["n"]), np.diff(c["indptr"])), weights=np.where(kept, w, 0.0), minlength=c["n"])
    if axes[2] != "planted":
        assert (R.bits(got_deg[:c["n"]][deg == 0]) == 0).all()
    return looked, deg


@pytest.mark.parametrize("n_rows,axes", SMALL, ids=lambda v: str(v) if isinstance(v, int) else "-".join(v))
def test_normalise_small_row_counts(n_rows, axes):
    """1, 2, 3 rows leave waves of the only block without a row; 4 fills it; 5 and 9 spill into a partial last block"""
    c = R.small_case(n_rows, n_rows, weights=axes[0], keep=axes[1], table=axes[2])
    got = run_norm(c, 0, 0, sentinel(n_rows))
    check_norm(c, got, 0, 0, sentinel(n_rows), truth=axes[2] != "planted", tag=f"n={n_rows} {axes}")
    check_paths(c, got[0], axes)


@pytest.mark.parametrize("axes", AXES, ids="-".join)
def test_normalise_lane_stride_edges(axes):
    """rows of 0, 1, 63, 64, 65, 128, 129 and 200 entries (the `p += 64` loops of both kernels) among 256 rows"""
    c = R.stride_case(7, weights=axes[0], keep=axes[1], table=axes[2])
    assert tuple(np.diff(c["indptr"])[:len(R.STRIDE_LENS)]) == R.STRIDE_LENS
    got = run_norm(c, 0, 0, sentinel(c["n"]))
    check_norm(c, got, 0, 0, sentinel(c["n"]), truth=axes[2] != "planted", tag=f"stride {axes}")
    looked, deg = check_paths(c, got[0], axes)
    if axes[2] in ("short", "planted") or (axes[0] == "quarters" and axes[2] != "none"):
        assert looked.any() and not looked.all()                       # both paths in one launch
    if axes[0] == "quarters":
        assert (np.floor(deg) != deg).any()                            # non-integral degrees
    if axes[1] == "row":
        assert deg[int(np.argmax(np.diff(c["indptr"])))] == 0          # the mask emptied the 200-entry row


@pytest.mark.parametrize("axes", [("none", "none", "cover"), ("quarters", "some", "short")], ids="-".join)
def test_normalise_phase_1_writes_its_slice_only(axes):
    """row_offset 3 into a vector 7 slots longer than the shard: every other slot and all values keep the sentinel bits"""
    c = R.stride_case(8, weights=axes[0], keep=axes[1], table=axes[2])
    start = sentinel(c["n"] + 7)
    got = run_norm(c, 1, 3, start)
    check_norm(c, got, 1, 3, start, tag=f"phase 1 {axes}")
    own = np.zeros(c["n"] + 7, dtype=bool)
    own[3:3 + c["n"]] = True
    assert (R.bits(got[0][~own]) == SENT_BITS).all() and not np.isnan(got[0][own]).any()


@pytest.mark.parametrize("axes", [("none", "none", "cover"), ("ints", "row", "short")], ids="-".join)
def test_normalise_phase_2_follows_the_vector_it_is_given(axes):
    """a planted D^-1/2 vector that is not the graph's (dyadic, so exact products differ visibly): the values follow it, from
    row_offset on for the rows and from 0 on for the columns, and the vector comes back untouched"""
    c = R.stride_case(9, weights=axes[0], keep=axes[1], table=axes[2])
    planted = ((1 + (5 * np.arange(c["n"] + 7)) % 11) * 0.25).astype(np.float32)
    got = run_norm(c, 2, 3, planted)
    check_norm(c, got, 2, 3, planted, tag=f"phase 2 {axes}")
    assert np.array_equal(R.bits(got[0]), R.bits(planted))


def _sharded_inputs(world, dropped, seed):
    r = R.interactions(41, 90, seed, long_row=70)           # 131 nodes: neither 2 nor 3 divides it; one row of 70+ entries
    n = sum(r.shape)
    assert n % world
    indptr, indices, edge_id, weight = R.bipartite_csr(r)
    assert weight is not None
    keep = None
    if dropped:                                              # a dropped view: unit weights, some interactions gone, user 0 emptied
        keep = (np.random.default_rng(seed).random(r.nnz) < 0.8).astype(np.uint8)
        keep[r.indptr[0]:r.indptr[1]] = 0
        weight = None
    # the table as the graph classes build it: entry counts, so a duplicate-summed degree can lie past it (formula path)
    return r, n, indptr, indices, edge_id, weight, keep, R.host_table(R.max_degree(r) + 1)


@pytest.mark.parametrize("dropped", [False, True], ids=["full", "dropped"])
@pytest.mark.parametrize("world", [2, 3])
def test_normalise_virtual_ranks_reassemble_the_single_rank_values(world, dropped):
    """phase 1 of every rank into ONE shared vector (what the all-gather leaves), then phase 2 per rank: each call equals its
    mirror, and the values, put back entry by entry, are those of one phase-0 launch over the whole matrix"""
    r, n, indptr, indices, edge_id, weight, keep, table = _sharded_inputs(world, dropped, 31)
    whole = dict(indptr=indptr.astype(np.int32), indices=indices.astype(np.int32), edge_id=edge_id, weight=weight, keep=keep,
                 table=table, n=n)
    one_deg, one_vals = run_norm(whole, 0, 0, sentinel(n))
    check_norm(whole, (one_deg, one_vals), 0, 0, sentinel(n), truth=False, tag="whole")
    shards = []
    for rank in range(world):
        l_indptr, l_cols, entry, n_pad = R.shard_rows(indptr, indices, rank, world)
        shards.append((dict(indptr=l_indptr, indices=l_cols, edge_id=edge_id[entry], weight=None if weight is None else weight[entry],
                            keep=keep, table=table, n=n_pad), entry))
    n_pad = shards[0][0]["n"]
    assert world * n_pad > n                                                  # padding rows exist
    shared = sentinel(world * n_pad)
    for rank, (c, _) in enumerate(shards):
        got = run_norm(c, 1, rank * n_pad, shared)
        check_norm(c, got, 1, rank * n_pad, shared, tag=f"rank {rank} phase 1")
        shared = got[0]
    assert not np.isnan(shared).any()                                         # every slot written, the padding rows' as 0
    assert np.array_equal(R.bits(shared[R.gather_order(n, world)]), R.bits(one_deg))
    pad = np.ones(world * n_pad, dtype=bool)
    pad[R.gather_order(n, world)] = False
    assert (R.bits(shared[pad]) == 0).all()
    back = sentinel(indices.size)
    for rank, (c, entry) in enumerate(shards):
        got = run_norm(c, 2, rank * n_pad, shared)
        check_norm(c, got, 2, rank * n_pad, shared, truth=False, tag=f"rank {rank} phase 2")
        back[entry] = got[1]
    assert np.array_equal(R.bits(back), R.bits(one_vals))


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_device_graphs_reassemble_the_device_graph(world):
    """the same through the product's own objects: every rank's ShardedDeviceGraph on one device, the all-gather done by the test
    (a first pass with a gather that does nothing collects each rank's slice, a second with one that fills in the assembled
    vector), against DeviceGraph(column_classes=False) -- the full graph and one dropped view"""
    r, n, indptr, indices, edge_id, weight, keep, table = _sharded_inputs(world, True, 32)
    device = torch.device("cuda", torch.cuda.current_device())
    whole = DeviceGraph(r, device=device, column_classes=False)
    assert np.array_equal(host(whole.adj.indices), indices)
    ranks = [ShardedDeviceGraph(r, rank, world, device, lambda t: None) for rank in range(world)]
    entries = []
    for rank, g in enumerate(ranks):
        l_indptr, l_cols, entry, n_pad = R.shard_rows(indptr, indices, rank, world)
        assert g.n_pad == n_pad and g.row_offset == rank * n_pad
        assert np.array_equal(host(g.adj.indptr), l_indptr) and np.array_equal(host(g.adj.indices), l_cols)
        entries.append(entry)
    keep_dev = dev(keep)

    def two_passes(normalise):
        """normalise(g) runs g's two phases into a value array and returns it"""
        for g in ranks:
            g._all_gather = lambda t: None
            normalise(g)
        assembled = torch.cat([g._dinv[g.row_offset:g.row_offset + g.n_pad] for g in ranks])
        back = sentinel(indices.size)
        for g, entry in zip(ranks, entries):
            g._all_gather = lambda t: t.copy_(assembled)
            back[entry] = host(normalise(g))
        return back

    def full(g):
        g._normalize(None, g.adj.vals)
        return g.adj.vals

    assert np.array_equal(R.bits(two_passes(full)), R.bits(host(whole.adj.vals)))
    (_, v32), _ = R.normalize_ref(indptr, indices, edge_id, R.bipartite_csr(r)[3], None, table, 0, np.zeros(n, np.float32), 0)
    assert np.array_equal(R.bits(host(whole.adj.vals)), R.bits(v32))          # and the graph IS the mirror with the host's table
    view = whole.dropped_view(keep_dev)
    got = two_passes(lambda g: g.dropped_view(keep_dev).vals)
    assert np.array_equal(R.bits(got), R.bits(host(view.vals)))
    (_, v32), _ = R.normalize_ref(indptr, indices, edge_id, None, keep, table, 0, np.zeros(n, np.float32), 0)
    assert np.array_equal(R.bits(host(view.vals)), R.bits(v32))
    assert (R.bits(got[keep[edge_id] == 0]) == 0).all() and np.isfinite(got).all()


def test_normalise_rows_past_2_to_the_26():
    """n_rows = 2^26 + 5, every row empty but the last five, one entry each, no table.  The row of a wave must not be computed
    from a 32-bit thread index (blockIdx.x * 256 wraps at block 2^24, the block of row 2^26), and one launch must not be asked
    for 2^32 work-items or more: with one launch of 2^24 + 2 blocks this case left 67,108,861 of its 67,108,869 D^-1/2 slots
    and all five values unwritten, without an error.  Fixed in csrc/graph.hip (at most 2^25 rows per launch, the row formed in
    64 bits from the block index); DESIGN.md 4.23."""
    low, tail = 1 << 26, 5
    n = low + tail
    indptr = torch.zeros(n + 1, dtype=torch.int32, device=DEV)
    indptr[n - tail:] = torch.arange(tail + 1, dtype=torch.int32, device=DEV)
    cols = np.array([3, 0, 4, 1, 2])                                   # among the last five
    w = np.array([4.0, 0.25, 2.25, 9.0, 16.0], dtype=np.float32)      # degrees, so D^-1/2 = 0.5, 2, 2/3, 1/3, 0.25
    deg_ws = torch.full((n,), float("nan"), dtype=torch.float32, device=DEV)
    deg_ws.view(torch.int32).fill_(SENT_BITS)
    vals = dev(sentinel(tail))
    ops.adj_sym_normalize(indptr, dev((low + cols).astype(np.int32)), None, None, n, weight=dev(w), out=vals, deg_ws=deg_ws)
    torch.cuda.synchronize()
    # the mirror on the five rows alone: the same 5 x 5 block with its columns counted from row 2^26
    (d32, v32), _ = R.normalize_ref(np.arange(tail + 1), cols, None, w, None, None, 0, sentinel(tail), 0)
    got_deg, got_vals = host(deg_ws[low:]), host(vals)
    survivors = int((deg_ws.view(torch.int32) == SENT_BITS).sum())
    print(f"rows past 2^26: D^-1/2 {got_deg}, values {got_vals}, {survivors} sentinel slots left in the vector")
    assert np.array_equal(R.bits(got_deg), R.bits(d32))
    assert np.array_equal(R.bits(got_vals), R.bits(v32))
    assert bool((deg_ws[:low].view(torch.int32) == 0).all())          # every empty row written, as +0.0
    assert survivors == 0 and not bool(torch.isnan(deg_ws).any()) and not np.isnan(got_vals).any()


# ---------------------------------------------------------------------------------------------------------------------------
# exchange: pure moves bit for bit, the scatter within m * 2^-24 * S
# ---------------------------------------------------------------------------------------------------------------------------
def raw_lists(case):
    """struct srh_batch_lists with a count of its own per segment, NULL where the case says None"""
    bl, alive = _lib.BatchLists(), []
    for s in range(R.SEGS):
        idx = dev(case["idx"][s])
        bl.d_idx[s] = idx.data_ptr()
        alive.append(idx)
        if case["counts"][s] is None:
            bl.d_count[s] = None
        else:
            cnt = torch.tensor([case["counts"][s]], dtype=torch.int32, device=DEV)
            bl.d_count[s] = cnt.data_ptr()
            alive.append(cnt)
    bl.B = case["B"]
    bl._keepalive = alive
    return bl


@pytest.mark.parametrize("shape", R.PACK_CASES, ids=str)
def test_pack_moves_live_rows_and_nothing_else(shape):
    """send over the sentinel: live slots are the table rows bit for bit (-0.0, a denormal and a NaN payload among them), dead
    slots exactly +0.0 although their index names a row full of poison; the cat list with and without its count"""
    case = R.pack_case(*shape)
    B = case["B"]
    want, cat, n_cat = R.pack_ref(case["idx"], case["counts"], B, case["tables"])
    if len(R.live_slots(case["counts"], B)[0]) >= 60:
        assert all((R.bits(want) == int(R.bits(v)[0])).any() for v in (np.float32(-0.0), np.float32(1e-42), R.PLANTED_NAN))
    lists, tables = raw_lists(case), [dev(t) for t in case["tables"]]
    for with_cat, with_n in ((True, True), (True, False), (False, False)):
        send = dev(sentinel(want.shape))
        cat_idx = torch.full((2 * B,), -7, dtype=torch.int32, device=DEV)
        n_dev = torch.full((1,), -7, dtype=torch.int32, device=DEV)
        ops.batch_pack(lists, tables, send, cat_idx=cat_idx if with_cat else None, n_cat=n_dev if with_n else None)
        got = host(send)
        assert not (R.bits(got) == POISON_BITS).any(), "a dead slot's row was sent"
        assert np.array_equal(R.bits(got), R.bits(want))
        if with_cat:
            assert np.array_equal(host(cat_idx)[:n_cat], cat) and (host(cat_idx)[n_cat:] == -7).all()
        else:
            assert (host(cat_idx) == -7).all()
        assert int(n_dev) == (n_cat if with_n else -7)
    n = R.seg_counts(case["counts"], B)
    if shape[3] == "a0":
        assert n[3] == 0 and n_cat == n[4] > 0 and cat[0] == 4 * B
    if shape[3] == "full":
        assert n_cat == 2 * B


@pytest.mark.parametrize("shape", R.UNPACK_CASES, ids=str)
def test_unpack_writes_live_rows_and_nothing_else(shape):
    """compact and gradient tables over the sentinel, the dead slots of recv full of poison: live rows are the whole rows bit for
    bit (gradient tables: +0.0), dead rows keep the sentinel; without gradient tables the pointer is NULL"""
    case = R.unpack_case(*shape)
    B, d = case["B"], case["world"] * case["dl"]
    start = sentinel((R.SEGS * B, d))
    want_c, want_g = R.unpack_ref(case["counts"], B, case["recv"], [start] * case["n_tables"], [start] * case["n_grads"])
    compact = [dev(start) for _ in range(case["n_tables"])]
    grads = [dev(start) for _ in range(case["n_grads"])]
    recv = dev(case["recv"])
    ops.batch_unpack(raw_lists(case), recv, case["world"], case["dl"], compact, grads)
    dead = np.ones(R.SEGS * B, dtype=bool)
    dead[R.live_slots(case["counts"], B)[0]] = False
    for got, want in zip(compact + grads, want_c + want_g):
        got = host(got)
        assert not (R.bits(got) == POISON_BITS).any(), "a dead slot of recv was read"
        assert (R.bits(got[dead]) == SENT_BITS).all(), "a dead row was written"
        assert np.array_equal(R.bits(got), R.bits(want))
    for g in grads:
        assert (R.bits(host(g)[~dead]) == 0).all()
    assert np.array_equal(R.bits(host(recv)), R.bits(case["recv"]))


def run_scatter(case):
    local = [dev(b) for b in case["bases"]]
    grads = [dev(g) for g in case["grads"]]
    ops.batch_scatter(raw_lists(case), list(zip(grads, local)), case["d_full"], case["col0"], case["dl"])
    for g, g0 in zip(grads, case["grads"]):
        assert np.array_equal(R.bits(host(g)), R.bits(g0))
    return [host(t) for t in local]


@pytest.mark.parametrize("shape", R.SCATTER_CASES, ids=str)
def test_scatter_gaussian_within_the_summation_bound(shape):
    """Heavy duplicates (three nodes), a non-zero base, poison outside [col0, col0 + dl) and on dead rows: each element within
    m * 2^-24 * S of the float64 sum -- m fp32 additions in whatever order the atomics took"""
    case = R.scatter_case(*shape)
    worst = 0.0
    for g, base, got in zip(case["grads"], case["bases"], run_scatter(case)):
        total, m, S, named = R.scatter_ref(case["idx"], case["counts"], case["B"], g, base, case["col0"], case["dl"])
        assert not np.isnan(got).any(), "a column outside the slice or a dead row reached the table"
        assert np.array_equal(R.bits(got[~named]), R.bits(base[~named])), "a row that no live slot names was written"
        err = np.abs(got.astype(np.float64) - total)
        worst = max(worst, float((err / np.where(m > 0, m * R.U24 * S, 1.0)).max()))
        assert (err <= m * R.U24 * S).all()
        assert (R.bits(got[m == 0]) == R.bits(base[m == 0])).all()
    print(f"scatter {shape}: worst error {worst:.3f} of m * 2^-24 * S")


@pytest.mark.parametrize("shape", [(67, 48, 36, 12, 3, "null"), (64, 20, 5, 6, 8, "null"), (5, 8, 0, 4, 1, "null"), (1, 4, 0, 4, 1, "null")],
                         ids=str)
def test_scatter_dyadic_is_the_exact_sum(shape):
    """All 5B slots live over two nodes, addends k * 2^-6 on a dyadic base: every partial sum is a multiple of 2^-17 below 2^7, so
    exact in fp32 in any order -- the table is the float64 sum bit for bit"""
    case = R.scatter_case(*shape, family="dyadic")
    for g, base, got in zip(case["grads"], case["bases"], run_scatter(case)):
        total, m, S, named = R.scatter_ref(case["idx"], case["counts"], case["B"], g, base, case["col0"], case["dl"])
        assert named.sum() <= 2 and S.max() * 2.0 ** 17 < 2.0 ** 24
        assert np.array_equal(total.astype(np.float32).astype(np.float64), total)
        assert np.array_equal(R.bits(got), R.bits(total.astype(np.float32)))
