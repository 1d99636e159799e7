"""The edge cases of the KNN kernels' tests -- TEST INFRASTRUCTURE ONLY.  tests/test_knn_edges_cpu.py shows that every case
reaches the path of csrc/knn.hip it is named for (tests/knn_ref.py's predictor) and keeps the restatement honest;
tests/test_gpu_knn_edges.py runs the kernels on them.  Every case, its restatement and its predictor tuples are computed
once (lru_cache) and never modified.  DESIGN.md 4.17 holds the table.

Neighbour cases.  Feature 0 is held by every row, feature 1 by the queries and the "strong" rows, those in fewer than K
residue classes of the pass (mod 512): every strong key beats every weak one, the K-th best thread maximum is the best
weak key, and the strong keys plus that one go into the buffer.  With s = 0 and no private features all strong sims tie and
the name rank alone orders them."""
import functools

import numpy as np

from tests import knn_ref

S_MAX = 2 ** 31 - 1                           # the largest shrinkage the 32-bit entry point takes


def _matrix(n_rows, feats):
    rows = np.concatenate([np.asarray(f, dtype=np.int64) for f in feats])
    cols = np.concatenate([np.full(len(f), j, dtype=np.int64) for j, f in enumerate(feats)])
    return knn_ref.binary_csr(rows, cols, n_rows, len(feats))


def _strong(lo, hi, k):
    r = np.arange(lo, hi)
    return r[(r % knn_ref.NB_CHUNK) % knn_ref.NB_THREADS < k - 1]


def _with(rows, *extra):
    return np.unique(np.concatenate([rows, np.asarray(extra, dtype=np.int64)]))


def _perm(n, seed):
    return np.random.default_rng(seed).permutation(n).astype(np.int64)


def _two_feature(n_rows, k, queries, strong=None):
    strong = _strong(0, n_rows, k) if strong is None else strong
    return _matrix(n_rows, [np.arange(n_rows), _with(strong, *queries)])


def _nb_over_k128(s=0, rank=None):
    n = 4608                                  # 9 rows per class, 127 strong classes: 1143 strong keys
    return _two_feature(n, 128, [n - 1]), (_perm(n, 1) if rank is None else rank), [n - 1], 128, s


def _nb_query_in_strong_set():
    """the queries are strong rows themselves (a weak-class query would be a 128th strong class for the others): each is
    among the candidates at or above its own bound and has to be left out of the buffer and of every round"""
    n = 4608
    return _two_feature(n, 128, []), _perm(n, 1), [5, 1029, 126], 128, 0


def _nb_over_k50():
    n = 11264                                 # 22 rows per class, 49 strong classes: 1078 strong keys
    return _two_feature(n, 50, [n - 1]), _perm(n, 2), [n - 1], 50, 0


def _nb_one_pass_exact():
    n = knn_ref.NB_CHUNK
    return _two_feature(n, 50, [n - 1]), _perm(n, 3), [n - 1], 50, 0


def _nb_one_wide_last_pass():
    """row 32768 is the only candidate of the second pass, strong and of the highest name rank: for query 515 it is the best
    neighbour; for query 32768 the second pass has no candidate at all.  515 is a strong row (class 3)."""
    n = knn_ref.NB_CHUNK + 1
    rank = _perm(n, 4)
    top = int(np.argmax(rank))
    rank[top], rank[n - 1] = rank[n - 1], rank[top]
    return _two_feature(n, 50, []), rank, [n - 1, 515], 50, 0


def _nb_second_pass_over_full_list():
    """the second pass overflows over a full list and has to keep half of it.  Feature 2 on 64 "super" rows of the first
    pass and on the strong rows of the second, which also hold a private feature 3.  For a strong query of the second pass
    (features 0, 1, 2) the super rows come first, then the strong rows of the second pass, then those of the first: the
    first pass leaves 64 + 64, the second raises the bound to the list's K-th key, finds 1142 candidates above it and
    keeps the 64 super rows.  Query 3, a strong row of the first pass without feature 2, has its list's K-th key above
    every key of the second pass"""
    n, c = 37376, knn_ref.NB_CHUNK
    strong = _strong(0, n, 128)
    late = strong[strong >= c]
    q = [c + 3, c + 1027, 3]
    sup = strong[(strong // knn_ref.NB_THREADS == 7) & (strong % knn_ref.NB_THREADS < 64)]
    a = _matrix(n, [np.arange(n), strong, np.concatenate([sup, late]), np.setdiff1d(late, q)])
    return a, _perm(n, 5), q, 128, 0


def _nb_short_list_carried():
    """only rows >= 32758 share a feature with query 32771: ten neighbours in the first pass, 699 candidates in the second;
    every third of them has a private feature, so two sims occur"""
    n, c = 33468, knn_ref.NB_CHUNK
    near = np.arange(c - 10, n)
    far = np.arange(0, c - 10)
    return _matrix(n, [near, far, near[near % 3 == 0][1:]]), _perm(n, 6), [c + 3], 50, 0


def _nb_cap(n_strong):
    n = 11264
    strong = _strong(0, n, 50)[:n_strong]     # total = the strong keys and the bound key
    return _two_feature(n, 50, [n - 1], strong), _perm(n, 7), [n - 1], 50, 0


def _nb_all_tied(kind):
    """one feature, held by every row: every sim ties.  identity / reversed ranks take the common path; "perm" gives the
    1143 rows of 127 residue classes the highest ranks in a seeded order, and overflows on ties alone"""
    n = 4608
    if kind == "identity":
        rank = np.arange(n, dtype=np.int64)
    elif kind == "reversed":
        rank = np.arange(n, dtype=np.int64)[::-1].copy()
    else:
        strong = _strong(0, n, 128)
        weak = np.setdiff1d(np.arange(n), strong)
        rng = np.random.default_rng(8)
        rank = np.empty(n, dtype=np.int64)
        rank[rng.permutation(weak)] = np.arange(len(weak))
        rank[rng.permutation(strong)] = len(weak) + np.arange(len(strong))
    return _matrix(n, [np.arange(n)]), rank, [n - 1, 0, 2500], 128, 0


def _nb_lower_bound():
    """two passes, four features whose transposed rows lie all below 32768, all at or above it, on both sides of it and from
    exactly 32768 on; a fifth, private one varies the degrees.  Query rows unsorted, one of them twice."""
    n, c = 33000, knn_ref.NB_CHUNK
    q1, q2 = 20000, c + 132
    below = _with(np.arange(100, 400), q1)
    above = _with(np.arange(c + 32, c + 222), q2)
    straddle = _with(np.arange(c - 68, c + 83), q1, q2)
    exact = _with(np.arange(c, c + 33), q2)
    private = np.setdiff1d(np.arange(0, n, 3), [q1, q2])
    return _matrix(n, [below, above, straddle, exact, private]), _perm(n, 9), [q2, q1, q2], 50, 100


def _nb_over_varied(s):
    """the overflow case with two private features (on the rows that are no multiple of 3, of 5): degrees from 2 to 4 among
    the strong rows, so three sims occur inside the buffer, and only every 15th strong row has the best one: the list
    of 128 holds two of them"""
    n = 4608
    q = [5, 2053]                             # strong rows, both of class 5
    strong = _strong(0, n, 128)
    p3 = np.setdiff1d(np.arange(n)[np.arange(n) % 3 != 0], q)
    p5 = np.setdiff1d(np.arange(n)[np.arange(n) % 5 != 0], q)
    return _matrix(n, [np.arange(n), strong, p3, p5]), _perm(n, 10), q, 128, s


# "over" in a name: some pass of some query row has total > NB_CAP; no other case may have one
NEIGHBOUR_CASES = {
    "over_k128": _nb_over_k128,
    "over_query_in_strong_set": _nb_query_in_strong_set,
    "over_k128_smax": lambda: _nb_over_k128(S_MAX),
    "over_k128_identity": lambda: _nb_over_k128(0, np.arange(4608, dtype=np.int64)),
    "over_k50": _nb_over_k50,
    "over_one_pass_exact": _nb_one_pass_exact,
    "over_one_wide_last_pass": _nb_one_wide_last_pass,
    "over_second_pass_full_list": _nb_second_pass_over_full_list,
    "short_list_carried": _nb_short_list_carried,
    "cap_1024": lambda: _nb_cap(1023),
    "over_cap_1025": lambda: _nb_cap(1024),
    "tied_identity": lambda: _nb_all_tied("identity"),
    "tied_reversed": lambda: _nb_all_tied("reversed"),
    "over_tied_perm": lambda: _nb_all_tied("perm"),
    "lower_bound": _nb_lower_bound,
    "over_varied_s0": lambda: _nb_over_varied(0),
    "over_varied_s10": lambda: _nb_over_varied(10),
}

# what the predictor has to give: per query row, one (total, len0, raised) per pass
NEIGHBOUR_PASSES = {
    "over_k128": [[(1144, 0, False)]],
    "over_query_in_strong_set": [[(1143, 0, False)]] * 3,
    "over_k128_smax": [[(1144, 0, False)]],
    "over_k128_identity": [[(1144, 0, False)]],
    "over_k50": [[(1079, 0, False)]],
    "over_one_pass_exact": [[(3137, 0, False)]],
    "over_one_wide_last_pass": [[(3137, 0, False), (50, 50, True)], [(3136, 0, False), (51, 50, True)]],
    "over_second_pass_full_list": [[(8129, 0, False), (1270, 128, True)]] * 2 + [[(8128, 0, False), (128, 128, True)]],
    "short_list_carried": [[(10, 0, False), (52, 10, False)]],
    "cap_1024": [[(1024, 0, False)]],
    "over_cap_1025": [[(1025, 0, False)]],
    "tied_identity": [[(128, 0, False)]] * 3,
    "tied_reversed": [[(128, 0, False)]] * 3,
    "over_tied_perm": [[(1144, 0, False)], [(1143, 0, False)], [(1144, 0, False)]],
    "lower_bound": [[(50, 0, False), (50, 50, False)], [(50, 0, False), (50, 50, True)], [(50, 0, False), (50, 50, False)]],
    "over_varied_s0": [[(1143, 0, False)]] * 2,
    "over_varied_s10": [[(1143, 0, False)]] * 2,
}


@functools.lru_cache(maxsize=None)
def neighbour_case(name):
    a, rank, rows, k, s = NEIGHBOUR_CASES[name]()
    rows = np.asarray(rows, dtype=np.int64)
    return dict(a=a, rank=rank, rows=rows, k=k, s=s, want=knn_ref.neighbours(a, rank, k, s, rows=rows),
                predicted=[knn_ref.neighbour_pass_counts(a, rank, int(q), k, s) for q in rows.tolist()])


# ---- scoring cases: handcrafted neighbour lists (inputs of knn_score_topk; they need not come from knn_neighbours) -----
def _pad_lists(lists, k_nbr):
    ids = np.full((len(lists), k_nbr), -1, dtype=np.int32)
    sims = np.zeros((len(lists), k_nbr))
    lens = np.zeros(len(lists), dtype=np.int32)
    for r, (i, s) in enumerate(lists):
        ids[r, :len(i)], sims[r, :len(i)], lens[r] = i, s, len(i)
    return ids, sims, lens


def _empty():
    return np.empty(0, dtype=np.int64), np.empty(0)


def _positives(n_items, n_top):
    i = np.arange(n_items)
    return i[i % knn_ref.SC_THREADS < n_top]


def _sc_user_overflow(n_items, n_top, seed, n_pos=None, n_random=8, drop_last=False):
    """user 0 is ranked.  Its neighbours 1..4 hold nested prefixes of the positive items (those of n_top residue classes
    mod 256, so that the (n_top + 1)-th thread maximum is a zero), then n_random random thirds: sums differ, and tie where
    two items lie in the same sets (never among 24 sets, here and there among 8).  Its own training items are zeros of high
    id and, outside the cap pair, three positives."""
    rng = np.random.default_rng(seed)
    pos = _positives(n_items, n_top)[:n_pos]
    zeros = np.setdiff1d(np.arange(n_items), pos)
    own = np.concatenate([zeros[-3:], [] if n_pos else rng.choice(pos[40:], 3, replace=False)]).astype(np.int64)
    sets = [pos[:max(1, len(pos) // d)] for d in (1, 2, 5, 17)]
    sets += [rng.choice(pos, len(pos) // 3, replace=False) for _ in range(n_random)]
    if n_pos:                                 # the cap pair: no positive is masked; the last one is there or not
        sets = [np.setdiff1d(x, pos[-1:] if drop_last else []) for x in sets]
    sims = rng.random(len(sets)) + 0.01
    user_items = [rng.permutation(own).tolist()] + [x.tolist() for x in sets]
    lists = [(np.arange(1, len(sets) + 1, dtype=np.int64), sims)] + [_empty()] * len(sets)
    return dict(mode="user", users=[0], user_items=user_items, lists=lists, n_items=n_items, n_top=n_top, k_nbr=32)


def _sc_item_overflow():
    """item mode: the user's 20 training items (zeros, in no sorted order) have lists of 128 over overlapping windows of
    the positives; the overlaps receive two sims"""
    n_items, n_top = 4352, 127
    rng = np.random.default_rng(31)
    pos = _positives(n_items, n_top)
    zeros = np.setdiff1d(np.arange(n_items), pos)
    own = rng.permutation(zeros[100::97][:20]).tolist()
    lists = [_empty()] * n_items
    for j, it in enumerate(own):
        lists[it] = (rng.permutation(pos[j * 107:j * 107 + 128]), rng.random(len(pos[j * 107:j * 107 + 128])) + 0.01)
    return dict(mode="item", users=[0], user_items=[own], lists=lists, n_items=n_items, n_top=n_top, k_nbr=128)


def _sc_small(n_items, mask_train=True):
    """n_top = 20 over a catalogue around the 256 threads; two ranked users with 2 and 5 training items and lists over 40
    neighbours that hold random halves of the catalogue.  At n_items = 21 every item is ranked, the -10e8 ones included,
    and those tie"""
    rng = np.random.default_rng(100 + n_items)
    user_items = [rng.choice(n_items, m, replace=False).tolist() for m in (2, 5)]
    user_items += [rng.choice(n_items, n_items // 2, replace=False).tolist() for _ in range(40)]
    lists = [(rng.permutation(40)[:m].astype(np.int64) + 2, rng.random(m)) for m in (40, 33)] + [_empty()] * 40
    return dict(mode="user", users=[1, 0], user_items=user_items, lists=lists, n_items=n_items, n_top=20, k_nbr=40,
                mask_train=mask_train)


def _sc_heavy_empty_heavy(ws_rows):
    """three ranked users: one with 30 neighbours, one with an empty list (all scores zero: marked, ids ascending over the
    items it has not trained on), one with 12 neighbours.  With one workspace row the empty one follows a heavy one in it"""
    rng = np.random.default_rng(41)
    n_items = 600
    user_items = [rng.choice(n_items, m, replace=False).tolist() for m in (7, 30, 4)]
    user_items[1] = [7, 0, 3] + [i for i in user_items[1] if i > 20]      # the leading ids are not all free
    user_items += [rng.choice(n_items, int(m), replace=False).tolist() for m in rng.integers(100, 400, 30)]
    lists = [(rng.permutation(30).astype(np.int64) + 3, rng.random(30)), _empty(),
             (rng.permutation(30)[:12].astype(np.int64) + 3, rng.random(12))] + [_empty()] * 30
    return dict(mode="user", users=[0, 1, 2], user_items=user_items, lists=lists, n_items=n_items, n_top=20, k_nbr=30,
                ws_rows=ws_rows)


def _sc_tie(at):
    """128 neighbours with one item each: item scores are set one by one.  Thirty items of distinct scores, two of them equal
    at places `at` and `at + 1` (0-based) of the order; the other items are zeros far below.  n_top = 20: a tie at 19 / 20 is
    between the N-th and the (N + 1)-th key and marks the row, a tie at 21 / 22 does not"""
    rng = np.random.default_rng(51)
    n_items = 300
    items = rng.choice(n_items, 30, replace=False)
    sims = np.sort(rng.random(30) + 0.5)[::-1].copy()
    sims[at + 1] = sims[at]
    user_items = [[int(np.setdiff1d(np.arange(n_items), items)[0])]] + [[int(i)] for i in items]
    lists = [(rng.permutation(30).astype(np.int64) + 1, None)] + [_empty()] * 30
    lists[0] = (lists[0][0], sims[lists[0][0] - 1])
    return dict(mode="user", users=[0], user_items=user_items, lists=lists, n_items=n_items, n_top=20, k_nbr=32)


def _sc_item_lists():
    """item mode, lists of length 0, 1 and 128; the users' items in no sorted order (the order of the additions)"""
    rng = np.random.default_rng(61)
    n_items = 300
    lens = rng.integers(2, 40, n_items)
    lens[[3, 77, 150]], lens[[4, 78, 151]], lens[[5, 79, 152]] = 0, 1, 128
    lists = [(rng.choice(n_items, m, replace=False).astype(np.int64), rng.random(m) * 1e-8) for m in lens.tolist()]
    user_items = [[150, 3, 79, 4, 299, 0], [152, 151], [3], [78, 5, 77, 200, 100, 201, 9, 151, 152, 7]]
    return dict(mode="item", users=[3, 0, 1, 2], user_items=user_items, lists=lists, n_items=n_items, n_top=20, k_nbr=128)


# "over" in a name: the row of the first ranked user has total > SC_CAP; no other row of any case may
SCORE_CASES = {
    "over_user_4352_n127": lambda: _sc_user_overflow(4352, 127, 21, n_random=24),
    "over_user_26624_n20": lambda: _sc_user_overflow(26624, 20, 22),
    "over_item_4352_n127": _sc_item_overflow,
    "cap_2048": lambda: _sc_user_overflow(26624, 20, 23, n_pos=2048, drop_last=True),
    "over_cap_2049": lambda: _sc_user_overflow(26624, 20, 23, n_pos=2048),
    "items_21": lambda: _sc_small(21),
    "items_255": lambda: _sc_small(255),
    "items_256": lambda: _sc_small(256),
    "items_257": lambda: _sc_small(257),
    "items_257_unmasked": lambda: _sc_small(257, mask_train=False),
    "heavy_empty_heavy_ws1": lambda: _sc_heavy_empty_heavy(1),
    "heavy_empty_heavy_ws3": lambda: _sc_heavy_empty_heavy(3),
    "tie_at_the_cut": lambda: _sc_tie(19),
    "tie_below_the_cut": lambda: _sc_tie(21),
    "item_lists_0_1_128": _sc_item_lists,
}

# what the predictor and rank_top have to give: per ranked user, the total and whether the row is marked
SCORE_TOTALS = {
    "over_user_4352_n127": [(2157, False)],
    "over_user_26624_n20": [(2078, True)],
    "over_item_4352_n127": [(2160, False)],
    "cap_2048": [(2048, True)],
    "over_cap_2049": [(2049, True)],
    "items_21": [(21, True), (21, True)],
    "items_255": [(21, False), (21, False)],
    "items_256": [(21, False), (21, False)],
    "items_257": [(21, False), (21, False)],
    "items_257_unmasked": [(21, False), (21, False)],
    "heavy_empty_heavy_ws1": [(22, False), (21, True), (22, True)],
    "heavy_empty_heavy_ws3": [(22, False), (21, True), (22, True)],
    "tie_at_the_cut": [(21, True)],
    "tie_below_the_cut": [(21, False)],
    "item_lists_0_1_128": [(21, False), (21, False), (21, False), (21, True)],
}


@functools.lru_cache(maxsize=None)
def score_case(name):
    c = dict(mask_train=True, ws_rows=8)
    c.update(SCORE_CASES[name]())
    side, ui = c["mode"], c["user_items"]
    rows = []
    for u in c["users"]:
        row = knn_ref.score_row(side, u, ui, c["lists"], c["n_items"])
        if c["mask_train"]:
            row[np.asarray(ui[u], dtype=np.int64)] = -10e8
        rows.append(row)
    c.update(rows=rows, tops=[knn_ref.rank_top(r, c["n_top"]) for r in rows],
             predicted=[knn_ref.score_pass_count(r, c["n_top"] + 1) for r in rows], nbr=_pad_lists(c["lists"], c["k_nbr"]))
    return c
