"""Restatements of the two kernel files that move whole graphs and whole batches -- csrc/graph.hip (degree_kernel, normalize_kernel
behind srh_adj_sym_normalize) and csrc/exchange.hip (pack_kernel, unpack_kernel, scatter_kernel behind srh_batch_pack / unpack /
scatter) -- in plain numpy, with the planted cases that tests/test_graph_exchange_ref_cpu.py (no GPU: scipy and the stand-ins of
tests/cpu_ops.py) and tests/test_gpu_graph_exchange_edges.py (the kernels) both answer to.  TEST INFRASTRUCTURE ONLY.

Normalisation: `normalize_ref` gives the call twice, as the fp32 mirror (the kernel's stated order of operations, every rounding
where the header puts it) and as the float64 truth (the same expression with the true deg^-1/2).  The two bounds a device result
is held to are bit equality with the mirror and NORM_BOUND = 4.5 * 2^-24 relative to the truth.

Exchange: `pack_ref` / `unpack_ref` are pure moves (bit for bit); `scatter_ref` gives per element the float64 sum, base included,
and the two quantities of its bound m * 2^-24 * S (m non-zero addends, S = |base| + sum |addend|)."""
import numpy as np
import scipy.sparse as sp


def _nan(payload):
    return np.array([payload], dtype=np.uint32).view(np.float32)[0]


SENTINEL = _nan(0x7FC0BEEF)          # pre-fill of whatever a call may write: what still holds these bits was not written
POISON = _nan(0x7FC0DEAD)            # content of whatever a call must not read: it shows in any output it reaches
PLANTED_NAN = _nan(0x7FC01234)       # a payload that IS data (a pure move carries it over bit for bit)
U24 = 2.0 ** -24                     # unit roundoff of binary32
# One value = fl(fl(dr * w) * dc), dr = fl(deg_r^-1/2), dc likewise: four roundings, each within 2^-24 relative (the formula path's
# dinv is the correctly rounded float32 of a float64 whose own error is 2^-53).  (1 + u)^4 - 1 = 4u + 6u^2 + ... < 4.5u.
NORM_BOUND = 4.5 * U24
SEGS = 5


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ---------------------------------------------------------------------------------------------------------------------------
# normalisation
# ---------------------------------------------------------------------------------------------------------------------------
def inv_sqrt_table(n):
    """table[k] = k^-1/2 correctly rounded to float32, table[0] = 0 -- what the formula path gives for an integral degree, so a
    kernel-level case can be held to the float64 truth on both paths.  (DeviceGraph builds its table with the host numpy's
    np.power, whose last bit is the host's: `host_table`.)"""
    t = np.zeros(n, dtype=np.float32)
    t[1:] = (1.0 / np.sqrt(np.arange(1, n, dtype=np.float64))).astype(np.float32)
    return t


def host_table(n):
    """as DeviceGraph / ShardedDeviceGraph build it (data/device_graph.py)"""
    with np.errstate(divide="ignore"):
        t = np.power(np.arange(n, dtype=np.float32), -0.5)
    t[0] = 0.0
    return t.astype(np.float32)


def planted_table(n):
    """a table no formula gives (2^-k): equality with the mirror then shows which rows were looked up and which were not"""
    return (2.0 ** -np.arange(n, dtype=np.float64)).astype(np.float32)


def normalize_ref(indptr, indices, edge_id, weight, keep, table, row_offset, deg_ws_in, phase):
    """One srh_adj_sym_normalize call over the CSR rows [row_offset, row_offset + n_rows) of a node table whose D^-1/2 vector is
    deg_ws (columns index the whole of it).  Returns ((deg_ws32, vals32), (deg_ws64, vals64)): the fp32 mirror and the float64
    truth.  vals is None for phase 1 (nothing written); deg_ws is the input for phase 2 (nothing written).  Slots of deg_ws that
    the call does not compute enter the truth as float64(deg_ws_in): they are inputs."""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    n_rows, nnz = indptr.size - 1, indices.size
    rows = np.repeat(np.arange(n_rows), np.diff(indptr))
    w32 = np.ones(nnz, dtype=np.float32) if weight is None else np.asarray(weight, dtype=np.float32)
    kept = np.ones(nnz, dtype=bool) if keep is None else np.asarray(keep)[np.asarray(edge_id, dtype=np.int64)] != 0
    d32 = np.array(deg_ws_in, dtype=np.float32, copy=True)
    d64 = d32.astype(np.float64)
    if phase != 2:
        deg = np.bincount(rows, weights=np.where(kept, w32, 0.0).astype(np.float64), minlength=n_rows)
        deg32 = deg.astype(np.float32)
        assert np.array_equal(deg32.astype(np.float64), deg), "the case's degree sums are not exact in fp32: no lane order is THE sum"
        with np.errstate(divide="ignore"):
            true = np.where(deg > 0, 1.0 / np.sqrt(np.where(deg > 0, deg, 1.0)), 0.0)
        dinv = true.astype(np.float32)                                  # float32(1 / sqrt(float64(deg))); 0 for an empty row
        if table is not None:
            table = np.asarray(table, dtype=np.float32)
            looked_up = (deg32 >= 0) & (deg32 < table.size) & (np.floor(deg32) == deg32)
            dinv[looked_up] = table[deg32[looked_up].astype(np.int64)]
        d32[row_offset:row_offset + n_rows] = dinv
        d64[row_offset:row_offset + n_rows] = true
    if phase == 1:
        return (d32, None), (d64, None)
    v32 = (d32[row_offset + rows] * w32) * d32[indices]                 # two fp32 products, left to right
    v32 = np.where(kept, v32, np.float32(0.0)).astype(np.float32)
    v64 = np.where(kept, (d64[row_offset + rows] * w32.astype(np.float64)) * d64[indices], 0.0)
    return (d32, v32), (d64, v64)


def lookup_rows(indptr, edge_id, weight, keep, table):
    """which rows of a phase 0 / 1 call take the table (integral degree below len(table))"""
    indptr = np.asarray(indptr, dtype=np.int64)
    n_rows = indptr.size - 1
    rows = np.repeat(np.arange(n_rows), np.diff(indptr))
    w = np.ones(rows.size) if weight is None else np.asarray(weight, dtype=np.float64)
    kept = np.ones(rows.size, dtype=bool) if keep is None else np.asarray(keep)[np.asarray(edge_id, dtype=np.int64)] != 0
    deg = np.bincount(rows, weights=np.where(kept, w, 0.0), minlength=n_rows)
    return np.zeros(n_rows, dtype=bool) if table is None else (deg < len(table)) & (np.floor(deg) == deg)


WEIGHTS = ("none", "ints", "quarters")
KEEPS = ("none", "some", "row")
TABLES = ("none", "cover", "short", "planted")


def square_case(lens, seed, weights="none", keep="none", table="none", n_cols=None):
    """A square CSR (not symmetric) whose row r has lens[r] distinct sorted columns; entries share interaction ids in pairs, as
    the two copies of a bipartite edge do.  weights: small integers, or multiples of 0.25 (non-integral degrees such as 2.75) --
    dyadic, so every degree sum is exact in any lane order.  keep: drops about a third of the ids, or ("row") every id of the
    longest row as well, which empties it.  table: absent / covering every degree / 3 entries (degrees 3 and up take the
    formula) / planted values over the first 6 degrees."""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, dtype=np.int64)
    n = lens.size if n_cols is None else n_cols
    assert lens.max(initial=0) <= n
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    indices = np.concatenate([np.sort(rng.choice(n, size=k, replace=False)) for k in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
    nnz = int(indices.size)
    n_ids = nnz // 2 + 1
    edge_id = rng.integers(0, n_ids, nnz).astype(np.int32)
    w = {"none": None, "ints": rng.integers(1, 4, nnz).astype(np.float32),
         "quarters": (rng.integers(1, 9, nnz) * 0.25).astype(np.float32)}[weights]
    k = None
    if keep != "none":
        k = (rng.random(n_ids) < 0.67).astype(np.uint8)
        if keep == "row":
            r = int(np.argmax(lens))
            k[edge_id[indptr[r]:indptr[r + 1]]] = 0
    top = int(np.ceil(float(np.max(np.bincount(np.repeat(np.arange(lens.size), lens), weights=np.ones(nnz) if w is None else w,
                                               minlength=1), initial=0))))
    t = {"none": None, "cover": inv_sqrt_table(top + 2), "short": inv_sqrt_table(3), "planted": planted_table(6)}[table]
    return dict(indptr=indptr, indices=indices, edge_id=edge_id, weight=w, keep=k, table=t, n=int(lens.size))


STRIDE_LENS = (0, 1, 63, 64, 65, 128, 129, 200)     # the edges of the `p += 64` lane loops


def stride_case(seed, **kw):
    """256 rows: the lane-stride lengths first, rows of 0..5 behind them"""
    rng = np.random.default_rng(1000 + seed)
    lens = np.concatenate([STRIDE_LENS, rng.integers(0, 6, 256 - len(STRIDE_LENS))])
    return square_case(lens, seed, **kw)


def small_case(n_rows, seed, **kw):
    """n_rows x n_rows with rows of 0 .. n_rows entries: 1 .. 3 rows leave lanes of the only block without a row, 5 and 9 spill
    into a partial last block of four"""
    rng = np.random.default_rng(2000 + seed)
    lens = rng.integers(0, n_rows + 1, n_rows)
    lens[0] = n_rows                                  # at least one full row
    return square_case(lens, seed, **kw)


def interactions(n_users, n_items, seed, duplicates=True, isolated=True, long_row=0):
    """a small interaction matrix: duplicate-summed weights (an interaction listed twice weighs 2), one user and one item with no
    interaction at all, optionally one user with `long_row` items"""
    rng = np.random.default_rng(seed)
    dense = (rng.random((n_users, n_items)) < 0.3).astype(np.float32)
    if long_row:
        dense[1, :long_row] = 1.0
    if duplicates:
        dense[dense > 0] += (rng.random(int((dense > 0).sum())) < 0.25)
    if isolated:
        dense[n_users - 1, :] = 0.0
        dense[:, n_items // 2] = 0.0
    return sp.csr_matrix(dense)


def bipartite_csr(r):
    """[[0, R], [R^T, 0]] as data/device_graph.py lays it out with column_classes=False: (indptr, indices, edge_id, weight)"""
    r = r.tocsr().astype(np.float32)
    r.sum_duplicates()
    r.sort_indices()
    nu = r.shape[0]
    eid = np.arange(r.nnz, dtype=np.int64)
    rt = sp.csr_matrix((eid + 1, r.indices, r.indptr), shape=r.shape).tocsc()
    rt.sort_indices()
    indptr = np.concatenate([r.indptr, r.indptr[-1] + rt.indptr[1:]]).astype(np.int64)
    indices = np.concatenate([r.indices.astype(np.int64) + nu, rt.indices]).astype(np.int64)
    edge_id = np.concatenate([eid, rt.data - 1]).astype(np.int32)
    weight = None if np.all(r.data == 1.0) else np.concatenate([r.data, r.data[rt.data - 1]]).astype(np.float32)
    return indptr, indices, edge_id, weight


def max_degree(r):
    r = r.tocsr()
    return int(max(np.diff(r.indptr).max(initial=0), np.diff(r.tocsc().indptr).max(initial=0)))


def shard_rows(indptr, indices, rank, world):
    """Rank `rank` of `world`: nodes rank, rank + world, ... as local rows, padded with empty rows to n_pad = ceil(N / world),
    columns rewritten to all-gather order (owner * n_pad + local row).  Returns (l_indptr, l_cols, entry, n_pad): entry[p] is
    the position in the whole matrix of local entry p."""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    n = indptr.size - 1
    n_pad = (n + world - 1) // world
    own = np.arange(rank, n, world)
    lens = np.diff(indptr)[own]
    l_indptr = np.zeros(n_pad + 1, dtype=np.int32)
    l_indptr[1:own.size + 1] = np.cumsum(lens)
    l_indptr[own.size + 1:] = l_indptr[own.size]
    entry = np.concatenate([np.arange(indptr[r], indptr[r + 1]) for r in own] + [np.zeros(0, np.int64)]).astype(np.int64)
    cols = indices[entry]
    l_cols = ((cols % world) * n_pad + cols // world).astype(np.int32)
    return l_indptr, l_cols, entry, n_pad


def gather_order(n, world):
    """node -> slot of the all-gathered D^-1/2 vector"""
    n_pad = (n + world - 1) // world
    nodes = np.arange(n)
    return (nodes % world) * n_pad + nodes // world


# ---------------------------------------------------------------------------------------------------------------------------
# exchange
# ---------------------------------------------------------------------------------------------------------------------------
def seg_counts(counts, B):
    """live slots per segment: None means B, a larger count is clamped to B"""
    return [B if c is None else min(int(c), B) for c in counts]


def live_slots(counts, B):
    """compact slots (segment * B + position) of every live slot, with the segment and position of each"""
    n = seg_counts(counts, B)
    seg = np.concatenate([np.full(n[s], s, dtype=np.int64) for s in range(SEGS)])
    pos = np.concatenate([np.arange(n[s], dtype=np.int64) for s in range(SEGS)])
    return seg * B + pos, seg, pos


def pack_ref(idx, counts, B, tables):
    """send (n_tables, 5B, dl): live slots hold the table row the list names, dead slots +0.0; and the one list of the compact
    slots of [unique users ; unique items] with its length."""
    slots, seg, pos = live_slots(counts, B)
    nodes = np.array([idx[s][p] for s, p in zip(seg, pos)], dtype=np.int64)
    send = np.zeros((len(tables), SEGS * B, tables[0].shape[1]), dtype=np.float32)
    for t, table in enumerate(tables):
        send[t, slots] = table[nodes]
    n = seg_counts(counts, B)
    cat = np.concatenate([3 * B + np.arange(n[3]), 4 * B + np.arange(n[4])]).astype(np.int32)
    return send, cat, int(cat.size)


def unpack_ref(counts, B, recv, compact_in, grads_in):
    """recv (world, n_tables, 5B, dl) -> copies of the compact tables (5B, world * dl) with their live rows replaced by the whole
    rows, and of the gradient tables with their live rows +0.0; dead rows as they came."""
    slots, _, _ = live_slots(counts, B)
    world, n_tables, rows, dl = recv.shape
    compact = [c.copy() for c in compact_in]
    for t in range(n_tables):
        whole = recv[:, t].transpose(1, 0, 2).reshape(rows, world * dl)
        compact[t][slots] = whole[slots]
    grads = [g.copy() for g in grads_in]
    for g in grads:
        g[slots] = np.float32(0.0)
    return compact, grads


def scatter_ref(idx, counts, B, compact_grad, base, col0, dl):
    """local[node, c] = base + sum over live slots naming node of compact_grad[slot, col0 + c].  Returns (sum64, m, S, named):
    the float64 sum, the number of non-zero addends and |base| + sum |addend| per element, and which rows a live slot names."""
    slots, seg, pos = live_slots(counts, B)
    nodes = np.array([idx[s][p] for s, p in zip(seg, pos)], dtype=np.int64)
    add = compact_grad[slots, col0:col0 + dl].astype(np.float64)
    total = base.astype(np.float64)
    m = np.zeros(base.shape, dtype=np.int64)
    S = np.abs(base.astype(np.float64))
    np.add.at(total, nodes, add)
    np.add.at(m, nodes, (add != 0).astype(np.int64))
    np.add.at(S, nodes, np.abs(add))
    named = np.zeros(base.shape[0], dtype=bool)
    named[nodes] = True
    return total, m, S, named


def base_of(want):
    """as tests/test_gpu_batch.py builds it: per row a power of two times 1..4, 1/64 .. 1/8 of the largest value to be added there
    (2^-17 .. 2^-15 where nothing is), so a store in place of an add is far outside any rounding bound"""
    top = np.abs(want).max(1)
    unit = np.where(top > 0, 2.0 ** (np.floor(np.log2(np.where(top > 0, top, 1.0))) - 5), 2.0 ** -17)
    r, c = np.meshgrid(np.arange(want.shape[0]), np.arange(want.shape[1]), indexing="ij")
    return (unit[:, None] * (1 + (3 * r + c) % 4)).astype(np.float32)


# count patterns over [u, i, j, uniq_u, uniq_i] as functions of B: NULL pointers, 0, 1, B, B + 5 (clamped), u / i / j apart
COUNTS = {
    "null": lambda B: [None] * 5,
    "ragged": lambda B: [1, B, B + 5, 0, max(B - 2, 1)],
    "a0": lambda B: [B // 2, 0, 1, 0, B],                       # no unique users: the cat list starts with the items
    "full": lambda B: [B + 5, None, 0, B + 5, None],            # a + c == 2B
    "pairs": lambda B: [max(B - 3, 0)] * 3 + [min(2, B), B + 5],  # one count for u, i, j: what ops.batch_lists can say
    "dead": lambda B: [0] * 5,
}
CPU_COUNTS = ("null", "pairs", "dead")                         # those the stand-ins of tests/cpu_ops.py can express
N_NODES = 13                                                    # rows of a local table; the last one is the poison row

# (B, dl, n_tables, counts)
PACK_CASES = [(1, 4, 1, "null"), (1, 8, 3, "pairs"), (5, 12, 3, "ragged"), (5, 4, 8, "dead"), (64, 8, 8, "full"),
              (67, 64, 1, "a0"), (67, 12, 3, "pairs"), (64, 64, 3, "ragged")]
# (B, dl, world, n_tables, n_grads, counts)
UNPACK_CASES = [(1, 4, 1, 1, 0, "null"), (5, 12, 3, 3, 5, "ragged"), (64, 8, 8, 8, 0, "full"), (67, 64, 2, 1, 7, "a0"),
                (67, 4, 3, 3, 5, "pairs"), (5, 8, 1, 1, 7, "dead"), (64, 12, 2, 8, 0, "pairs")]
# (B, d_full, col0, dl, n_pairs, counts): a slice of any width, the first and the last slice of a 4-way split
SCATTER_CASES = [(5, 20, 5, 6, 3, "ragged"), (64, 32, 0, 8, 1, "null"), (67, 48, 36, 12, 8, "full"), (1, 4, 0, 4, 1, "a0"),
                 (67, 256, 192, 64, 3, "pairs"), (5, 16, 12, 4, 8, "dead"), (64, 20, 5, 6, 3, "pairs")]


def index_lists(B, counts, seed, n_nodes=N_NODES, among=None):
    """five lists of B slots: live slots name nodes 0 .. n_nodes - 2 (or only those of `among`), dead slots the poison row"""
    rng = np.random.default_rng(seed)
    n = seg_counts(counts, B)
    idx = np.full((SEGS, B), n_nodes - 1, dtype=np.int32)
    for s in range(SEGS):
        idx[s, :n[s]] = rng.integers(0, n_nodes - 1, n[s]) if among is None else rng.choice(among, n[s])
    return idx


def plant(a, rng, k=3):
    """-0.0, a denormal and a NaN payload among the values of a (k of each where it has room)"""
    flat = a.reshape(-1)
    for v in (np.float32(-0.0), np.float32(1e-42), PLANTED_NAN):
        flat[rng.integers(0, flat.size, min(k, flat.size))] = v
    return a


def pack_case(B, dl, n_tables, counts, seed=0):
    rng = np.random.default_rng(seed)
    cnt = COUNTS[counts](B)
    tables = [plant(rng.standard_normal((N_NODES, dl)).astype(np.float32), rng, 6) for _ in range(n_tables)]
    for t in tables:
        t[N_NODES - 1] = POISON
    return dict(B=B, dl=dl, counts=cnt, idx=index_lists(B, cnt, seed + 1), tables=tables)


def unpack_case(B, dl, world, n_tables, n_grads, counts, seed=0):
    """recv as an all-gather of packed buffers leaves it, except that its dead slots hold the poison instead of zeros"""
    rng = np.random.default_rng(seed)
    cnt = COUNTS[counts](B)
    recv = plant(rng.standard_normal((world, n_tables, SEGS * B, dl)).astype(np.float32), rng, 6)
    dead = np.ones(SEGS * B, dtype=bool)
    dead[live_slots(cnt, B)[0]] = False
    recv[:, :, dead] = POISON
    return dict(B=B, dl=dl, world=world, counts=cnt, idx=index_lists(B, cnt, seed + 1), recv=recv, n_tables=n_tables, n_grads=n_grads)


def scatter_case(B, d_full, col0, dl, n_pairs, counts, seed=0, family="gauss"):
    """compact gradient tables with the poison outside the slice and on dead rows.  gauss: standard normal addends (with whole
    zero rows, which the kernel skips), live slots over three nodes only -- heavy duplicates.  dyadic: addends k * 2^-6, |k| <= 8,
    live slots over two nodes: every partial sum is exact in fp32, so no order of the atomics can change a bit."""
    rng = np.random.default_rng(seed)
    cnt = COUNTS[counts](B)
    idx = index_lists(B, cnt, seed + 1, among=[2, 7] if family == "dyadic" else [0, 5, 11])
    slots = live_slots(cnt, B)[0]
    grads = []
    for _ in range(n_pairs):
        g = np.full((SEGS * B, d_full), POISON, dtype=np.float32)
        if family == "dyadic":
            live = (rng.integers(-8, 9, (slots.size, dl)) * 2.0 ** -6).astype(np.float32)
        else:
            live = rng.standard_normal((slots.size, dl)).astype(np.float32)
            live[rng.random(slots.size) < 0.2] = 0.0
        g[slots, col0:col0 + dl] = live
        grads.append(g)
    bases = [base_of(scatter_ref(idx, cnt, B, g, np.zeros((N_NODES, dl), np.float32), col0, dl)[0]) for g in grads]
    return dict(B=B, d_full=d_full, col0=col0, dl=dl, counts=cnt, idx=idx, grads=grads, bases=bases)
