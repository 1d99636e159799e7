"""Seeded synthetic interaction graphs in the shapes BASELINE.json names.

The reference ships no yelp2018 / iFashion files (reference .MISSING_LARGE_BLOBS:1-7), so
every benchmark and parity case runs on a generated bipartite graph with the same
user / item / edge counts and power-law degrees on both sides.  Output formats are the
ones the reference's loader produces (reference data/loader.py:22-33): a list of
``[user_str, item_str, float_weight]`` triples, or the same as ``train.txt`` /
``test.txt`` lines ``"user item weight"``.

Guarantees: no duplicate (user, item) pairs, and every
user and every item owns at least one *training* edge, so ``Interaction`` sees exactly
``n_users`` x ``n_items``.
"""
from __future__ import annotations

import numpy as np

# name -> (n_users, n_items, n_edges_total)   [train+test]
SHAPES = {
    # LightGCN split of Yelp2018: 1,237,259 train + 324,147 test
    "yelp2018": (31668, 38048, 1561406),
    # iFashion (SGL paper): 300,000 x 81,614, 1,607,813 interactions
    "ifashion": (300000, 81614, 1607813),
    # shipped dataset/douban-book/test.txt stands in for the missing train file
    "douban-book": (10882, 19075, 119690),
    # BASELINE.json config 4; E chosen here (avg user degree 50), stated in DESIGN.md
    "1m-500k": (1000000, 500000, 50000000),
    "tiny": (300, 500, 6000),
    "small": (2000, 3000, 60000),
}


def _zipf_weights(n: int, exponent: float, rng: np.random.Generator) -> np.ndarray:
    w = 1.0 / np.power(np.arange(1, n + 1, dtype=np.float64), exponent)
    rng.shuffle(w)  # popularity must not correlate with id
    return w / w.sum()


def generate_edges(n_users: int, n_items: int, n_edges: int, seed: int = 2024,
                   user_exp: float = 0.6, item_exp: float = 0.8):
    """Return (users, items) int64 arrays of unique pairs; each node has >= 2 edges
    where possible so that an 80/20 split can leave one in train."""
    rng = np.random.default_rng(seed)
    if n_edges > n_users * n_items // 2:
        raise ValueError("graph too dense for rejection sampling")
    pu = _zipf_weights(n_users, user_exp, rng)
    pi = _zipf_weights(n_items, item_exp, rng)
    cu, ci = np.cumsum(pu), np.cumsum(pi)
    cu[-1] = ci[-1] = 1.0
    # seed edges: every user and item appears at least once
    base_u = np.concatenate([np.arange(n_users), np.searchsorted(cu, rng.random(n_items), side="right")])
    base_i = np.concatenate([np.searchsorted(ci, rng.random(n_users), side="right"), np.arange(n_items)])
    keys = np.unique(base_u.astype(np.int64) * n_items + base_i.astype(np.int64))
    while keys.size < n_edges:
        need = n_edges - keys.size
        m = int(need * 1.15) + 1024
        u = np.searchsorted(cu, rng.random(m), side="right").astype(np.int64)
        i = np.searchsorted(ci, rng.random(m), side="right").astype(np.int64)
        new = np.setdiff1d(np.unique(u * n_items + i), keys, assume_unique=True)
        if new.size > need:
            new = rng.choice(new, size=need, replace=False)
        keys = np.union1d(keys, new)
    if keys.size > n_edges:
        # only possible when the seed edges alone exceed n_edges
        keys = keys[:n_edges]
    users = keys // n_items
    items = keys % n_items
    order = rng.permutation(keys.size)  # file order is not sorted in real datasets
    return users[order], items[order]


def split_train_test(users: np.ndarray, items: np.ndarray, n_users: int, n_items: int,
                     test_frac: float = 0.2, seed: int = 2024):
    """Random per-edge split, then repair: the first edge of every user and of every
    item (in file order) is forced into train."""
    rng = np.random.default_rng(seed + 1)
    is_test = rng.random(users.size) < test_frac
    first_u = np.full(n_users, -1, dtype=np.int64)
    first_i = np.full(n_items, -1, dtype=np.int64)
    idx = np.arange(users.size - 1, -1, -1)
    first_u[users[idx]] = idx
    first_i[items[idx]] = idx
    is_test[first_u[first_u >= 0]] = False
    is_test[first_i[first_i >= 0]] = False
    tr = ~is_test
    return (users[tr], items[tr]), (users[is_test], items[is_test])


def make_dataset(shape: str = "tiny", seed: int = 2024, test_frac: float = 0.2,
                 n_edges: int | None = None):
    """Return ``(train_u, train_i, test_u, test_i, n_users, n_items)`` int64 id arrays."""
    n_users, n_items, e = SHAPES[shape]
    if n_edges is not None:
        e = n_edges
    u, i = generate_edges(n_users, n_items, e, seed)
    (tu, ti), (su, si) = split_train_test(u, i, n_users, n_items, test_frac, seed)
    return tu, ti, su, si, n_users, n_items


def as_triples(users: np.ndarray, items: np.ndarray, weight: float = 1.0):
    """In-memory format of reference data/loader.py:26-33: [[user_str, item_str, float]]."""
    us = users.astype(str).tolist()
    its = items.astype(str).tolist()
    return [[a, b, weight] for a, b in zip(us, its)]


def write_text(path: str, users: np.ndarray, items: np.ndarray, weight: int = 1) -> None:
    """``"user item weight"`` lines, the on-disk format of reference data/loader.py:26-32."""
    with open(path, "w") as f:
        f.writelines(f"{a} {b} {weight}\n" for a, b in zip(users.tolist(), items.tolist()))


# ---- social relations (conf key social.data: SEPT) ---------------------------------------------------------------------
def make_social(shape: str = "tiny", seed: int = 2024, mean_degree: float = 12.6, reciprocal: float = 0.3,
                closure: float = 0.25):
    """Seeded directed trust pairs over the users of ``shape`` in the loader's in-memory format ``[[u, v, 1], ...]``
    (reference data/loader.py:53-66), user names as make_dataset / as_triples write them.

    Out-degrees are skewed (a capped Pareto tail whose mean is near douban-book's 12.6 trust lines per user), followees
    are drawn from a Zipf popularity, a share ``reciprocal`` of the pairs is followed back, and for a share ``closure`` of
    the pairs u -> v the user u also follows one of v's followees -- triangles, without which SEPT's friend view
    (S.S) (.) S would be empty.  No self-pairs, no duplicates, file order shuffled."""
    n = SHAPES[shape][0]
    rng = np.random.default_rng(seed + 7)
    cap = max(1, min(n - 1, 2000))
    scale = mean_degree / 3.0 / (1.0 + reciprocal + 0.6 * closure)          # E[pareto(1.5) + 1] = 3; the added pairs
    deg = np.minimum(np.floor((rng.pareto(1.5, n) + 1.0) * scale).astype(np.int64), cap)
    cu = np.cumsum(_zipf_weights(n, 0.8, rng))
    cu[-1] = 1.0
    src = np.repeat(np.arange(n, dtype=np.int64), deg)
    dst = np.searchsorted(cu, rng.random(src.size), side="right").astype(np.int64)
    keys = np.unique(src[src != dst] * n + dst[src != dst])
    src, dst = keys // n, keys % n
    back = rng.random(keys.size) < reciprocal
    # u -> v, v -> w  =>  u -> w for a share of the pairs (keys are sorted by source: a CSR without building one)
    indptr = np.searchsorted(src, np.arange(n + 1))
    out_deg = np.diff(indptr)
    close = (rng.random(keys.size) < closure) & (out_deg[dst] > 0)
    w = dst[indptr[dst[close]] + np.floor(rng.random(int(close.sum())) * out_deg[dst[close]]).astype(np.int64)]
    u = src[close]
    keys = np.unique(np.concatenate([keys, dst[back] * n + src[back], u[u != w] * n + w[u != w]]))
    keys = keys[rng.permutation(keys.size)]
    return [[a, b, 1] for a, b in zip((keys // n).astype(str).tolist(), (keys % n).astype(str).tolist())]


def write_social(path: str, lines) -> None:
    """``"user1 user2 weight"`` lines, the format FileIO.load_social_data reads."""
    with open(path, "w") as f:
        f.writelines(f"{a} {b} {w}\n" for a, b, w in lines)


# ---- sequence datasets (model.type: sequential) -----------------------------------------------------------------------
# name -> (n_sequences, n_items, n_interactions_total)   [train + the one held-out item per sequence]
SEQ_SHAPES = {
    # the size of the 5-core Amazon Beauty set conf/SASRec.yaml names (22,363 users, 12,101 items, 198,502 interactions);
    # the counts are this project's choice, stated in DESIGN.md 4.9
    "beauty-seq": (22363, 12101, 198502),
    "tiny-seq": (300, 200, 3600),
    # sized after the MovieLens-1M figures of the SASRec paper (6,040 sequences, 3,416 items, about 1.0 M interactions: a
    # mean length of ~166, the set the paper runs at max.len 200); the counts are this project's choice, stated in
    # DESIGN.md 4.28
    "ml1m-seq": (6040, 3416, 1000000),
}


def generate_sequences(n_seq: int, n_items: int, n_total: int, seed: int = 2024, min_len: int = 3, item_exp: float = 0.8,
                       follow: float = 0.6):
    """List of int64 item-id arrays, one per sequence: lengths min_len + a geometric tail summing to ~n_total, items from
    a Zipf popularity, and with probability ``follow`` the next item is a fixed successor of the current one -- a
    first-order structure a next-item model can learn.  Every item occurs at least once."""
    rng = np.random.default_rng(seed)
    mean_tail = max(n_total / n_seq - min_len, 0.0)
    lens = min_len + (rng.geometric(1.0 / (1.0 + mean_tail), size=n_seq) - 1 if mean_tail > 0 else np.zeros(n_seq, np.int64))
    ci = np.cumsum(_zipf_weights(n_items, item_exp, rng))
    ci[-1] = 1.0
    successor = rng.permutation(n_items)
    seqs = []
    for n in lens.tolist():
        fresh = np.searchsorted(ci, rng.random(n), side="right")
        chain = rng.random(n) < follow
        s = np.empty(n, dtype=np.int64)
        s[0] = fresh[0]
        for t in range(1, n):
            s[t] = successor[s[t - 1]] if chain[t] else fresh[t]
        seqs.append(s)
    # every item at least once: the missing ones replace inner positions of the longest sequences
    missing = np.setdiff1d(np.arange(n_items), np.unique(np.concatenate(seqs)))
    order = np.argsort(-lens, kind="stable")
    for k, it in enumerate(missing.tolist()):
        s = seqs[order[k % n_seq]]
        s[(k // n_seq) % max(len(s) - 1, 1)] = it
    return seqs


def make_sequence_dataset(shape: str = "tiny-seq", seed: int = 2024):
    """(train, test): {seq_name: [item_name, ...]} dicts in the loader's in-memory format; leave-one-out -- the last item
    of every sequence is its test item."""
    n_seq, n_items, n_total = SEQ_SHAPES[shape]
    seqs = generate_sequences(n_seq, n_items, n_total, seed)
    train = {str(k): [str(i) for i in s[:-1].tolist()] for k, s in enumerate(seqs)}
    test = {str(k): [str(int(s[-1]))] for k, s in enumerate(seqs)}
    return train, test


def write_sequences(path: str, sequences) -> None:
    """``"seq_id:item item ..."`` lines, the on-disk format of reference data/loader.py:35-41."""
    with open(path, "w") as f:
        f.writelines(f"{name}:{' '.join(items)}\n" for name, items in sequences.items())
