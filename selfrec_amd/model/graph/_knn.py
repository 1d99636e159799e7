"""UserKNN / ItemKNN on the HIP kernels of csrc/knn.hip: the neighbour lists of train() come from
``ops.knn_neighbours``, predict() and test() from ``ops.knn_score_topk``.  Ratings are all 1, so every figure is the
reference's float64 result bit for bit: similarities, ``user_sim`` / ``item_sim``, predict() rows, ranked lists."""
import time
from collections.abc import Mapping

import numpy as np
import torch

from ... import ops
from ...base.graph_recommender import GraphRecommender, _to_host
from ...util.evaluation import RankedLists


def _csr(rows, cols, n_rows):
    """(indptr, indices) int32 of the pairs, each row's columns in the order the pairs come"""
    order = np.argsort(rows, kind="stable")
    indptr = np.zeros(n_rows + 1, dtype=np.int32)
    np.cumsum(np.bincount(rows, minlength=n_rows), out=indptr[1:])
    return indptr, np.ascontiguousarray(cols[order], dtype=np.int32)


def _name_ranks(id2name, n):
    """rank of each id's name in sorted(names) (python string order: code points)"""
    order = sorted(range(n), key=id2name.__getitem__)
    rank = np.empty(n, dtype=np.int32)
    rank[np.asarray(order, dtype=np.int64)] = np.arange(n, dtype=np.int32)
    return rank


class NeighbourLists(Mapping):
    """{name: [(sim, neighbour name), ...]} of the reference's user_sim / item_sim, read from the neighbour arrays; a row's
    tuples are built when it is looked up."""

    def __init__(self, names, index, ids, sims, lens):
        self._names, self._index = names, index
        self._ids, self._sims, self._lens = ids, sims, lens

    def __getitem__(self, name):
        r = self._index[name]
        n = int(self._lens[r])
        return [(s, self._names[v]) for s, v in zip(self._sims[r, :n].tolist(), self._ids[r, :n].tolist())]

    def __iter__(self):
        return iter(self._names)

    def __len__(self):
        return len(self._names)


class KNNRecommender(GraphRecommender):
    side = None            # 'user' (UserKNN) or 'item' (ItemKNN): whose rows are compared
    SCORE_WS_ROWS = 1024   # float64 score rows in flight: 1024 x 38 k items = 311 MB at the Yelp2018 shape

    def __init__(self, conf, training_set, test_set):
        super().__init__(conf, training_set, test_set)
        self.topk = int(self.config['topK'])
        self.shrinkage = int(self.config['shrinkage'])
        self._nbr = None
        self._dev = None
        self._score_ws = None

    # ---- structure ----------------------------------------------------------------------
    def _structure(self):
        """device CSRs of the training matrix, built once: users -> items in training-file order (predict()'s source
        order and the mask), items -> users and users -> items with ascending columns (the neighbour search)"""
        if self._dev is None:
            d = self.data
            dev = torch.device('cuda', torch.cuda.current_device())
            u, i = np.asarray(d.train_u, dtype=np.int64), np.asarray(d.train_i, dtype=np.int64)
            _, first = np.unique(u * d.item_num + i, return_index=True)      # a repeated pair is one rating of 1
            first.sort()
            u, i = u[first], i[first]
            up, ui = _csr(u, i, d.user_num)
            o = np.lexsort((u, i))
            ip, iu = _csr(i[o], u[o], d.item_num)
            o = np.lexsort((i, u))
            _, ui_sorted = _csr(u[o], i[o], d.user_num)
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            self._dev = dict(device=dev, u_indptr=t(up), u_items=t(ui), u_items_sorted=t(ui_sorted),
                             i_indptr=t(ip), i_users=t(iu),
                             u_norm=t(np.sqrt(np.diff(up).astype(np.float64))),
                             i_norm=t(np.sqrt(np.diff(ip).astype(np.float64))))
        return self._dev

    def _side_arrays(self):
        g = self._structure()
        d = self.data
        if self.side == 'user':
            rank = _name_ranks(d.id2user, d.user_num)
            return (g['u_indptr'], g['u_items'], g['i_indptr'], g['i_users'], g['u_norm'],
                    torch.from_numpy(rank).to(g['device']))
        rank = _name_ranks(d.id2item, d.item_num)
        return (g['i_indptr'], g['i_users'], g['u_indptr'], g['u_items_sorted'], g['i_norm'],
                torch.from_numpy(rank).to(g['device']))

    # ---- train / predict / test ---------------------------------------------------------
    def train(self):
        label = type(self).__name__
        print(f"[{label}] Computing {self.side}-{self.side} similarity with top-{self.topk}...")
        start = time.time()
        ids, sims, lens = ops.knn_neighbours(*self._side_arrays(), self.topk, self.shrinkage)
        torch.cuda.current_stream().synchronize()
        self._nbr = (ids, sims, lens)
        self._nbr_host = None
        print(f"[{label}] Similarity computation done in {time.time() - start:.2f}s.")

    def neighbour_lists(self):
        """the reference's user_sim / item_sim ({name: [(sim, name), ...]}, best first) over the device lists"""
        if self._nbr is None:
            return {}
        if self._nbr_host is None:
            self._nbr_host = _to_host(*self._nbr)
        d = self.data
        if self.side == 'user':
            names = [d.id2user[k] for k in range(d.user_num)]
            index = d.user
        else:
            names = [d.id2item[k] for k in range(d.item_num)]
            index = d.item
        return NeighbourLists(names, index, *self._nbr_host)

    def _score(self, uid, mask_train=True):
        g = self._structure()
        if self._nbr is None:
            raise RuntimeError(f"{type(self).__name__}: train() first")
        ids, sims, lens = self._nbr
        n_top = min(self.max_N, min(ops.KNN_MAX_K, self.data.item_num) - 1)
        out = ops.knn_score_topk(self.side, uid, g['u_indptr'], g['u_items'], self.data.item_num, ids, sims, lens,
                                 max(1, n_top), ws_rows=self.SCORE_WS_ROWS, ws=self._score_ws, mask_train=mask_train)
        self._score_ws = out[2]
        return out

    def predict(self, u):
        """float64 scores of every item for user name u (UserKNN.py:59-81 / ItemKNN.py:58-81); training items unmasked"""
        uid = torch.tensor([self.data.user[u]], dtype=torch.int32, device=self._structure()['device'])
        _, _, ws = self._score(uid, mask_train=False)
        return ws[:8 * self.data.item_num].view(torch.float64).cpu().numpy().copy()

    def _heap_rows(self, uid_host, k):
        """ids / scores of the given users in find_k_largest's heap order (util/algorithm.py:144-156) from their masked rows"""
        n_items = self.data.item_num
        ids = np.empty((len(uid_host), k), dtype=np.int32)
        sc = np.empty((len(uid_host), k), dtype=np.float64)
        step = self.SCORE_WS_ROWS
        for lo in range(0, len(uid_host), step):
            part = uid_host[lo:lo + step]
            _, _, ws = self._score(torch.from_numpy(np.ascontiguousarray(part, dtype=np.int32)).to(self._dev['device']))
            rows, = _to_host(ws[:8 * n_items * len(part)].view(torch.float64).view(len(part), n_items))
            for j in range(len(part)):
                ids[lo + j], sc[lo + j] = ops.find_k_largest_host_f64(k, rows[j])
        return ids, sc

    def rank_users(self, uid_host):
        """(ids int32, scores float64) numpy, (len(uid_host), max_N): test()'s ranking of these user ids, the tied rows
        redone in the reference's heap order"""
        k = self.max_N
        uid = torch.from_numpy(np.ascontiguousarray(uid_host, dtype=np.int32)).to(self._structure()['device'])
        ids_d, sc_d, _ = self._score(uid)
        ids, sc = _to_host(ids_d, sc_d)
        rows = np.flatnonzero(ids[:, 0] < 0)
        self._last_tie_rows = int(rows.size)
        if rows.size:
            ids[rows], sc[rows] = self._heap_rows(np.asarray(uid_host)[rows], k)
        return ids, sc

    def test(self):
        users, uid, names, keys, names_list = self._test_users()
        if not users or self.max_N + 1 > min(ops.KNN_MAX_K, self.data.item_num):
            return super().test()                              # (the reference's per-user loop over predict())
        ids, sc = self.rank_users(uid)
        dev = self._dev['device']
        t_indptr, t_indices, h_indptr = self._test_csr(dev)
        uid_d = torch.from_numpy(np.ascontiguousarray(uid)).to(dev)
        flags = ops.topk_hit_flags(torch.from_numpy(ids).to(dev), uid_d, t_indptr, t_indices)
        cuts = sorted({int(n) for n in self.topN if 1 <= int(n) <= self.max_N})[:8]
        sizes = (t_indptr[1:] - t_indptr[:-1])[uid_d.long()].contiguous()
        hits, ndcg = ops.metric_rows(flags, sizes, cuts)
        got = _to_host(flags, *[t for c in range(len(cuts)) for t in (hits[c], ndcg[c])])
        per_user = {n: (got[1 + 2 * c], got[2 + 2 * c]) for c, n in enumerate(cuts)}
        return RankedLists(users, names, ids, sc, hit_flags=got[0], truth_sizes=np.diff(h_indptr)[uid],
                           origin=self.data.test_set, per_user=per_user, keys=keys, names_list=names_list)
