"""The ranking kernels of csrc/eval.hip against tests/ranking_ref.py -- a host restatement of the header's contract (the
documented float32 fma chain, the -10e8 mask, (score desc, id asc) order), not against each other: the plain and the filtered
pipeline share gemm_nt_kernel, topk_kernel, the mask value and the clamped tail loads, and a defect they share is invisible
to a comparison between them.  Shapes are ragged on purpose: catalogues that are no whole number of 32-item tiles, a bound
slice that is no multiple of 32, a second 256-row block with 44 rows in it, chunks and slabs that start at lo > 0."""
import functools

import numpy as np
import pytest
import torch

from selfrec_amd import ops
from tests import ranking_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _same_ranking(ids, sc, want_ids, want_sc, rows=None):
    ids, sc = ids.cpu().numpy(), sc.cpu().numpy()
    if rows is not None:
        ids, sc, want_ids, want_sc = ids[rows], sc[rows], want_ids[rows], want_sc[rows]
    bad = np.flatnonzero((ids != want_ids).any(axis=1) | (_bits(sc) != _bits(want_sc)).any(axis=1))
    assert bad.size == 0, f"{bad.size} rows differ, first {bad[:5]}: ids {ids[bad[0]][:8]} want {want_ids[bad[0]][:8]}"


# ------------------------------------------------------------------------------------------
# a. the scoring GEMM: the documented chain, bit for bit
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", [(1, 1), (33, 31), (70, 1031)])
@pytest.mark.parametrize("d", [32, 64, 128, 256])
def test_gemm_nt_is_the_documented_fma_chain(d, m, n):
    """Every output of srh_gemm_nt_f32 equals acc = fma(u[s], i[s], acc); acc = fma(u[D/2 + s], i[D/2 + s], acc) in float32
    -- the statement csrc/eval.hip rests "ids and scores equal bit for bit" on.  (1, 1) and (33, 31): rows and columns past
    the end are clamped loads; (70, 1031): three row blocks, several waves, a tile of 7 columns."""
    rng = np.random.default_rng(1000 * d + n)
    U = (rng.standard_normal((m, d)) * 0.3).astype(np.float32)
    I = (rng.standard_normal((n, d)) * 0.3).astype(np.float32)
    got = ops.gemm_nt(_dev(U), _dev(I)).cpu().numpy()
    want = R.chain_scores(U, I)
    f64 = U.astype(np.float64) @ I.astype(np.float64).T
    bound = d * 2.0 ** -24 * (np.abs(U).astype(np.float64) @ np.abs(I).astype(np.float64).T)
    worst = float((np.abs(got - f64) / np.maximum(bound, 1e-300)).max())
    differ = int((_bits(got) != _bits(want)).sum())
    print(f"gemm_nt d={d} ({m}, {n}): {differ} of {got.size} outputs differ from the chain; |got - f64| / bound <= {worst:.3f}")
    assert worst <= 1.0
    assert differ == 0


# ------------------------------------------------------------------------------------------
# b. srh_topk_rows
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _topk_rows_case(n):
    rng = np.random.default_rng(77 + n)
    x = rng.standard_normal((11, n)).astype(np.float32)
    x[1] = np.float32(0.25)                                        # all scores equal (n > 2048: more than kTopkCap at the bound)
    x[2] = R.MASK_VALUE                                            # -10e8 except 3 entries: fewer than K live ones
    x[2, [0, n // 2, n - 1]] = [0.5, -0.5, 0.5]
    x[3, rng.choice(n, n // 3, replace=False)] = -np.inf           # a row containing -inf
    x[4] = -np.inf                                                 # ... and one that is -inf but for two entries
    x[4, [n - 1, n // 3]] = [1.0, 2.0]
    x[5, rng.choice(n, (3 * n) // 5, replace=False)] = x[5].max() + 1     # 60 % of the row tied at the top (n = 5003: 3001 > 2048)
    x[6, n - 1] = 9.0; x[6, 0] = 9.0                               # the best two at both ends
    x[7] = np.round(x[7] * 2) / 2                                  # a dozen distinct values: ties everywhere
    return x, {k: R.rank(x, k) for k in (1, 20, 128) if k <= n}


@pytest.mark.parametrize("n,k", [(n, k) for n in (20, 255, 257, 1030, 5003) for k in (1, 20, 128) if k <= n])
def test_topk_rows_against_the_host_ranking(n, k):
    """(score desc, id asc) top-K of ragged rows: n % 4 != 0 starts every other row off 16-byte alignment (scalar loads);
    tie-heavy rows rank by id; at n = 5003 two rows put more than 2048 scores at the bound (the K-rounds fallback)."""
    x, want = _topk_rows_case(n)
    ids, sc = ops.topk_rows(_dev(x), k)
    _same_ranking(ids, sc, *want[k])


# ------------------------------------------------------------------------------------------
# c. srh_score_mask_topk
# ------------------------------------------------------------------------------------------
def _csr(rows):
    indptr = np.zeros(len(rows) + 1, dtype=np.int32)
    np.cumsum([len(r) for r in rows], out=indptr[1:])
    flat = np.concatenate([np.sort(np.asarray(r, dtype=np.int32)) for r in rows] + [np.zeros(0, dtype=np.int32)])
    return indptr, np.ascontiguousarray(flat, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def _plain_case(d):
    rng = np.random.default_rng(300 + d)
    m, n, K = 150, 1031, 20
    U = (rng.standard_normal((m, d)) * 0.3).astype(np.float32)
    I = (rng.standard_normal((n, d)) * 0.3).astype(np.float32)
    I[50:60] = I[50]                                               # tied items
    U[9] = 0.0                                                     # a user whose scores are all equal
    scores = R.chain_scores(U, I)
    best = np.argsort(-scores, axis=1)
    rows = []
    for u in range(m):
        own = best[u, rng.choice(10, 2, replace=False)]            # two of the user's ten best items are training items
        rows.append(np.union1d(own, rng.choice(n, rng.integers(5, 60), replace=False)))
    rows[4] = np.zeros(0, dtype=np.int64)                          # an empty training row
    rows[77] = np.setdiff1d(np.arange(n), [3, 500, 501, 1029, 1030])      # all but 5 items: fewer than K left
    rows[149] = np.arange(1000, n)                                 # the last user masks the tail of the catalogue
    indptr, indices = _csr(rows)
    perm = rng.permutation(m).astype(np.int32)
    want = {name: R.rank(R.masked(scores[users], users, indptr, indices), K)
            for name, users in (("none", np.arange(m)), ("shuffled", perm))}
    return U, I, indptr, indices, perm, want, K


@pytest.mark.parametrize("slab_rows", [150, 64], ids=["one-pass", "slab64"])
@pytest.mark.parametrize("ids_kind", ["shuffled", "none"])
@pytest.mark.parametrize("d", [32, 64, 128, 256])
def test_score_mask_topk_against_the_host_ranking(d, ids_kind, slab_rows):
    """scores -> mask -> top-K against rank(masked(chain_scores)): ids and scores equal.  A slab of 64 rows makes three
    passes, two of them with lo > 0 (mask_kernel's user_base + q, d_user_emb + lo * d when there are no user ids)."""
    U, I, indptr, indices, perm, want, K = _plain_case(d)
    users = _dev(perm) if ids_kind == "shuffled" else None
    slab = torch.empty((slab_rows, I.shape[0]), dtype=torch.float32, device=DEV)
    ids, sc = ops.score_mask_topk(_dev(U), users, _dev(I), _dev(indptr), _dev(indices), K, scores_ws=slab)
    _same_ranking(ids, sc, *want[ids_kind])


# ------------------------------------------------------------------------------------------
# d. srh_score_mask_topk_filtered
# ------------------------------------------------------------------------------------------
SAMPLE = 1000                  # bound slice: not a multiple of 32
N_BIG = 1040                   # items of large norm: ids [0, 100) and [140, 1040 + 40) -- see _filtered_case


def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def _build_filtered(d, n_items, m, seed, zero_users, most_user, long_user, dup_user, planted, tail_fans):
    """Tables, masks and expectations of one filtered-ranking scenario.  Everything the test asserts about WHICH rows
    overflow is derived here, on the host, from exact chain scores:

      items of large norm (0.9 .. 1.1): ids [0, 100) + [140, 1040), 1000 of them -- the split path's bound slice (the 1000
      largest norms); the other path's slice is ids [0, 1000).  Everything else has norm 0.3 .. 0.5, so a row's K-th best
      score of either slice is close to its K-th best overall and an ordinary row has about K survivors;
      ids [100, 140): 40 copies of one small item that points at `dup_user` (tied scores inside the leading slice);
      planted[u] items outside both slices point straight at user u (norm 0.78 .. 0.85: above any score of a random
      direction), which gives u that many more survivors -- the rows that overflow a 64-slot list and no larger one;
      zero_users: every score 0, the whole catalogue survives;  most_user: a training row that covers all but 10 items,
      none of them in a slice: the bound is -10e8 and the whole catalogue survives;  long_user: a training row of ~600
      (above rescore_wave_kernel's TRW = 512) that holds five of the user's own best items;  tail_fans: users whose best
      item is one of the last ids of the catalogue (the 5-item tail tile)."""
    rng = np.random.default_rng(seed)
    U = (rng.standard_normal((m, d)) * 0.3).astype(np.float32)
    for u in zero_users:
        U[u] = 0.0
    # the items planted for user u are parallel, so any other user either gets all of them or none: every other user is made
    # orthogonal to the planted directions (their scores on those items are ~0) and the extra survivors stay u's alone
    for t, u in enumerate(planted):
        e = _unit(U[u].astype(np.float64))
        rest = np.array([v for v in range(m) if v != u and v not in list(planted)[:t]])
        U[rest] = (U[rest] - np.outer(U[rest].astype(np.float64) @ e, e)).astype(np.float32)
    big = np.zeros(n_items, dtype=bool)
    big[:100] = True; big[140:N_BIG] = True
    norms = np.where(big, rng.uniform(0.9, 1.1, n_items), rng.uniform(0.3, 0.5, n_items))
    I = (_unit(rng.standard_normal((n_items, d))) * norms[:, None]).astype(np.float32)
    I[100:140] = (0.5 * _unit(0.9 * _unit(U[dup_user].astype(np.float64)) + 0.436 * _unit(rng.standard_normal(d)))).astype(np.float32)
    free = np.arange(N_BIG, n_items - 8)
    taken = rng.choice(free, sum(planted.values()), replace=False)
    at = 0
    for u, cnt in planted.items():
        ids = taken[at:at + cnt]; at += cnt
        I[ids] = (_unit(U[u].astype(np.float64))[None, :] * rng.uniform(0.78, 0.85, cnt)[:, None]).astype(np.float32)
    for t, u in enumerate(tail_fans):
        I[n_items - 1 - 2 * t] = (_unit(U[u].astype(np.float64)) * 0.8).astype(np.float32)
    scores = R.chain_scores(U, I)

    best = np.argsort(-scores, axis=1)[:, :10]
    ordinary = np.setdiff1d(free, taken)
    rows = []
    for u in range(m):
        own = best[u, rng.choice(10, 2, replace=False)]
        n_tr = 0 if u % 9 == 4 else int(rng.integers(30, 50))
        if n_tr == 0:
            rows.append(np.zeros(0, dtype=np.int64))
            continue
        rows.append(np.union1d(own, np.concatenate([rng.choice(N_BIG, n_tr // 2, replace=False),
                                                    rng.choice(n_items, n_tr // 2, replace=False)])))
    rows[long_user] = np.union1d(best[long_user, :5], rng.choice(ordinary, 595, replace=False))     # (none of the slice thinned)
    rows[most_user] = np.setdiff1d(np.arange(n_items), rng.choice(ordinary, 10, replace=False))
    indptr, indices = _csr(rows)
    assert indptr[long_user + 1] - indptr[long_user] > 512 and indices.max() < n_items

    item_norm = np.linalg.norm(I.astype(np.float64), axis=1)
    slices = {True: np.sort(np.argsort(-item_norm, kind="stable")[:SAMPLE]), False: np.arange(SAMPLE)}
    assert set(slices[True]) == set(np.flatnonzero(big))          # a clear gap: float32 norms sort the same way
    case = dict(U=U, I=I, indptr=indptr, indices=indices, m=m, n=n_items, slices=slices, planted=set(planted),
                perm=rng.permutation(m).astype(np.int32), empty=(np.zeros(m + 1, dtype=np.int32), np.zeros(1, dtype=np.int32)))
    all_users = np.arange(m)
    for with_mask in (True, False):
        ms = R.masked(scores, all_users, indptr, indices) if with_mask else scores
        case["ranked", with_mask] = R.rank(ms, 128)
        case["unmasked", with_mask] = (ms != R.MASK_VALUE).sum(axis=1)
        for split in (True, False):
            sl = np.sort(ms[:, slices[split]], axis=1)
            for K in (1, 20, 50, 128):
                # exact survivor count: items (training items included) whose score reaches the K-th best masked score of
                # the bound slice
                case["exact", with_mask, split, K] = (scores >= sl[:, -K][:, None]).sum(axis=1)
    return case


@functools.lru_cache(maxsize=None)
def _filtered_case(d):
    return _build_filtered(d, n_items=4133, m=300, seed=4100 + d, zero_users=(7, 291), most_user=60, long_user=40,
                           dup_user=127, planted={127: 25, 150: 65, 299: 68}, tail_fans=(5, 200))


def _expected_overflow(case, with_mask, split, K, cap, planted_room=False):
    """Rows that must report counts > cap, known BEFORE the call: exact survivor count > cap.  Every other row has to stay
    at or below cap / 2 exactly -- the factor 2 is the room left to the bf16 margins of the split path, which lower the
    bound and widen the filter by amounts nobody has measured at these shapes -- so that no row's fate is left to them."""
    exact = case["exact", with_mask, split, K]
    over = exact > cap
    room = np.full(case["m"], cap // 2)
    if planted_room:
        room[sorted(case["planted"])] = (3 * cap) // 4
    undecided = np.flatnonzero(~over & (exact > room))
    assert undecided.size == 0, f"scenario leaves rows {undecided} with {exact[undecided]} exact survivors for cap {cap}"
    return over, exact


def _run_filtered(case, d, K, cap, chunk_rows, ids_kind, with_mask, planted_room=False, ws=None):
    split = d in (64, 128)
    over_u, exact_u = _expected_overflow(case, with_mask, split, K, cap, planted_room)
    users = case["perm"] if ids_kind == "shuffled" else np.arange(case["m"])
    indptr, indices = (case["indptr"], case["indices"]) if with_mask else (None, None)
    ids, sc, counts, used_ws = ops.score_mask_topk_filtered(
        _dev(case["U"]), _dev(users) if ids_kind == "shuffled" else None, _dev(case["I"]),
        None if indptr is None else _dev(indptr), None if indices is None else _dev(indices), K,
        sample_items=SAMPLE, cap=cap, chunk_rows=chunk_rows, ws=ws)
    assert ws is None or used_ws.data_ptr() == ws.data_ptr()                   # (the caller's workspace was large enough)
    counts = counts.cpu().numpy()
    what = f"d={d} K={K} cap={cap} chunk={chunk_rows} ids={ids_kind} mask={with_mask}"
    got_over = counts > cap
    assert set(users[got_over].tolist()) == set(np.flatnonzero(over_u).tolist()), \
        f"{what}: overflow rows {sorted(users[got_over].tolist())}, counts {counts[got_over]}; exact {exact_u[users][got_over]}"
    ok = ~got_over
    want_ids, want_sc = case["ranked", with_mask]
    _same_ranking(ids, sc, want_ids[users][:, :K], want_sc[users][:, :K], rows=ok)
    assert (counts[ok] >= np.minimum(K, case["unmasked", with_mask][users][ok])).all(), what
    # the header's pass 2: a score is kept iff it reaches the bound -- exactly (f32 filter) or at least (bf16 filter, whose
    # bound is a lower bound of the exact one and whose margins only ever let more through)
    if split:
        assert (counts >= exact_u[users]).all(), what
    else:
        assert np.array_equal(counts, exact_u[users]), what
    return counts


FILTER_KCAP = [(1, 64), (20, 64), (20, 256), (50, 256), (128, 512)]


@pytest.mark.parametrize("K,cap", FILTER_KCAP)
@pytest.mark.parametrize("d", [32, 64, 128, 256])
def test_filtered_ranking_against_the_host_ranking(d, K, cap):
    """srh_score_mask_topk_filtered against rank(masked(chain_scores)) at 4133 items (129 tiles + 5), a bound slice of 1000,
    300 queries (a second 256-row block of 44), chunks of 300 and 128, user ids shuffled and absent, mask CSR present and
    absent.  d = 64 / 128: the split-bf16 filter with both re-score kernels; d = 32 / 256: the f32 filter epilogue and
    cand_topk_kernel.  The rows that overflow are exactly the ones the host predicted; all others equal the expectation
    in ids and score bits.  cap = 64: rows with 64 < counts <= 128 are the ones rescore_wave_kernel has to leave alone."""
    case = _filtered_case(d)
    split = d in (64, 128)
    seen = []
    for chunk_rows in (300, 128):
        for ids_kind in ("shuffled", "none"):
            for with_mask in (True, False):
                seen.append(_run_filtered(case, d, K, cap, chunk_rows, ids_kind, with_mask))
    counts = np.concatenate(seen)
    if K < 128:
        assert (counts <= min(cap, 128)).any()                                 # complete short lists: one wave each
    else:
        assert ((counts > 128) & (counts <= cap)).any()                        # complete long lists: a workgroup each
    if cap == 64:
        assert ((counts > cap) & (counts <= 128)).any()                        # overflowed AND short: nobody ranks them


@pytest.mark.parametrize("d", [32, 64])
def test_filtered_ranking_stays_inside_the_workspace_it_asked_for(d):
    """The entry point carves its workspace by the layout srh_score_mask_topk_filtered_ws_bytes sizes: given exactly that
    many bytes at the head of a larger allocation filled with 0xA5, it leaves the 4096 bytes behind them untouched and
    ranks as ever (K = 20, cap = 64, chunks of 128 -- three of them, the last of 44 rows -- mask present, ids shuffled;
    d = 32: the f32 pipeline, d = 64: the bf16 one).  The guard lies inside the allocation: a layout that disagrees
    with its size fails here and faults nowhere."""
    from selfrec_amd import _lib
    case = _filtered_case(d)
    K, cap, chunk_rows = 20, 64, 128
    need = int(_lib.load().srh_score_mask_topk_filtered_ws_bytes(chunk_rows, SAMPLE, K, cap, case["I"].shape[0], d))
    assert need > 0
    buf = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    _run_filtered(case, d, K, cap, chunk_rows, "shuffled", True, ws=buf[:need])
    torch.cuda.synchronize()
    touched = int((buf[need:] != 0xA5).sum())
    assert touched == 0, f"{touched} of the 4096 bytes behind the workspace's {need} were written"


def test_filtered_ranking_large_catalogue_binary_search():
    """131105 items (above the 131072 an LDS bitmap serves): rescore_topk_kernel looks training items up by binary search.
    Six planted rows carry 120 .. 160 extra survivors so that their lists are long (> 128) and complete (<= cap = 256)."""
    case = _large_case()
    counts = _run_filtered(case, 64, 20, 256, 32, "shuffled", True, planted_room=True)
    long_rows = (counts > 128) & (counts <= 256)
    assert long_rows.sum() >= 5 and (counts <= 128).any()


@functools.lru_cache(maxsize=None)
def _large_case():
    return _build_filtered(64, n_items=131105, m=32, seed=9, zero_users=(3,), most_user=6, long_user=20, dup_user=25,
                           planted={2: 120, 9: 130, 15: 140, 16: 150, 30: 160, 31: 125}, tail_fans=(5, 12))


# ------------------------------------------------------------------------------------------
# e. hit flags and trim / mark
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k1", [2, 21, 129])
def test_hit_flags_and_trim_mark_ties_against_their_restatements(k1):
    rng = np.random.default_rng(500 + k1)
    rows, n_users, n_items = 301, 340, 900                          # (301 rows: a second workgroup of 45 threads)
    ids = np.stack([rng.choice(n_items, k1, replace=False) for _ in range(rows)]).astype(np.int32)
    sc = -np.sort(-rng.standard_normal((rows, k1)).astype(np.float32), axis=1)
    k = k1 - 1
    sc[0, 1 % k1] = sc[0, 0]                                        # a tie at (0, 1)
    sc[1, k] = sc[1, k - 1]                                         # a tie at (k - 1, k): only the dropped column shows it
    if k1 > 3:
        sc[2, k // 2] = sc[2, k // 2 + 1]                           # a tie in the middle
    sc[300, k] = sc[300, k - 1]                                     # ... and in the last row
    users = rng.permutation(n_users)[:rows].astype(np.int32)
    test_rows = []
    for u in range(n_users):
        test_rows.append(np.zeros(0, dtype=np.int64) if u % 5 == 0 else rng.choice(n_items, rng.integers(1, 30), replace=False))
    for q in range(0, rows, 3):                                     # ranked ids at both ends of the user's test row
        row = np.sort(test_rows[users[q]])
        if row.size:
            ids[q, 0] = row[0]; ids[q, k1 - 1] = row[-1]
            ids[q, 1:k1 - 1] = rng.permutation(np.setdiff1d(np.arange(n_items), row[[0, -1]]))[:k1 - 2]
    t_indptr, t_indices = _csr(test_rows)
    assert any(t_indptr[u + 1] == t_indptr[u] for u in users)

    tid, tsc = ops.topk_trim_mark_ties(_dev(ids), _dev(sc))
    want_ids, want_sc = R.trim_mark_ties(ids, sc)
    assert np.array_equal(tid.cpu().numpy(), want_ids) and np.array_equal(_bits(tsc.cpu().numpy()), _bits(want_sc))
    assert want_ids[0, 0] < 0 and want_ids[1, 0] < 0 and want_ids[300, 0] < 0 and (want_ids[3:300, 0] >= 0).all()

    for uids in (users, None):
        flags = ops.topk_hit_flags(_dev(ids), None if uids is None else _dev(uids), _dev(t_indptr), _dev(t_indices))
        want = R.hit_flags(ids, uids, t_indptr, t_indices)
        assert np.array_equal(flags.cpu().numpy(), want)
        assert want.any() and not want.all()
