"""UserKNN (reference model/graph/UserKNN.py): the top-K most similar users by cosine with shrinkage, and item scores
from their training items.  Config keys ``topK`` and ``shrinkage``.  train() and test() run on csrc/knn.hip."""
from ._knn import KNNRecommender


class UserKNN(KNNRecommender):
    side = 'user'

    @property
    def user_sim(self):
        """{user name: [(sim, neighbour name), ...]} best first (UserKNN.py:12,51), rows built on access"""
        return self.neighbour_lists()
