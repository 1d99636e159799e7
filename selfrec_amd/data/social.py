"""Social relations with the surface of reference data/social.py:7-87 (``Relation``): the trust pairs of a dataset
filtered to the training users, the follower / followee maps, and the scipy matrices SEPT (and MHCN) build their views from.

The reference's quirks are kept because the views depend on them:
  * a pair with either end outside ``user`` is dropped (from the caller's list too, as the reference deletes in place);
  * ``get_social_mat`` lets the csr_matrix constructor SUM duplicate pairs (an entry listed twice is 2.0);
  * ``get_birectional_social_mat`` is ``S.multiply(S)`` -- the element-wise square, not S (.) S^T.
Everything here is host scipy in float32; tests/golden/sept.npz pins it to the reference bit for bit.
"""
from collections import defaultdict

import numpy as np
import scipy.sparse as sp

from .graph import Graph


class Relation(Graph):
    def __init__(self, conf, relation, user):
        super().__init__()
        self.config = conf
        self.social_user = {}
        self.user = user
        relation[:] = [pair for pair in relation if pair[0] in user and pair[1] in user]
        self.relation = relation
        self.followees = defaultdict(dict)
        self.followers = defaultdict(dict)
        for src, dst, weight in relation:
            self.followees[src][dst] = weight
            self.followers[dst][src] = weight

    def get_social_mat(self):
        n = len(self.user)
        rows = np.fromiter((self.user[p[0]] for p in self.relation), dtype=np.int64, count=len(self.relation))
        cols = np.fromiter((self.user[p[1]] for p in self.relation), dtype=np.int64, count=len(self.relation))
        ones = np.ones(rows.size, dtype=np.float32)
        return sp.csr_matrix((ones, (rows, cols)), shape=(n, n), dtype=np.float32)     # duplicates are summed

    def get_birectional_social_mat(self):
        social_mat = self.get_social_mat()
        return social_mat.multiply(social_mat)

    def convert_to_laplacian_mat(self, adj_mat):
        rows, cols = adj_mat.nonzero()
        kept = sp.csr_matrix((adj_mat.data, (rows, cols)), shape=adj_mat.get_shape(), dtype=np.float32)
        return self.normalize_graph_mat(kept)

    def weight(self, u1, u2):
        return self.followees[u1][u2] if self.has_followee(u1, u2) else 0

    def get_followers(self, u):
        return self.followers[u] if u in self.followers else {}

    def get_followees(self, u):
        return self.followees[u] if u in self.followees else {}

    def has_followee(self, u1, u2):
        return u1 in self.followees and u2 in self.followees[u1]

    def has_follower(self, u1, u2):
        return u1 in self.followers and u2 in self.followers[u1]

    def size(self):
        return len(self.followers), len(self.relation)
