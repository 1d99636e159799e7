"""ItemKNN (reference model/graph/ItemKNN.py): the top-K most similar items by cosine with shrinkage, and item scores
from the lists of the user's training items.  Config keys ``topK`` and ``shrinkage``.  train() and test() run on
csrc/knn.hip."""
from ._knn import KNNRecommender


class ItemKNN(KNNRecommender):
    side = 'item'

    @property
    def item_sim(self):
        """{item name: [(sim, neighbour name), ...]} best first (ItemKNN.py:12,50), rows built on access"""
        return self.neighbour_lists()
