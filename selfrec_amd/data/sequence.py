"""``Sequence`` with the surface of reference data/sequence.py:6-54: the id maps and the id lists of a sequence dataset
(``{seq_name: [item_name, ...]}``, FileIO.load_data_set(file, 'sequential')).

Item ids start at 1 in first-appearance order of the training file; 0 is the padding id of the batches.  A training
sequence with fewer than two items is dropped (it has no (input, target) pair).  ``test_set[seq][item] = 1`` holds the
FIRST test item of every test sequence that survived in training -- next-item evaluation."""
from collections import defaultdict

from .data import Data


class Sequence(Data):
    def __init__(self, conf, training, test):
        super().__init__(conf, training, test)
        self.item, self.id2item = {}, {}
        self.seq, self.id2seq = {}, {}
        self.test_set = defaultdict(dict)
        self.test_set_item = set()
        self.original_seq = self._index_training()
        self._index_test()
        self.raw_seq_num = len(self.seq)
        self.item_num = len(self.item)

    def _index_training(self):
        """[(seq_name, [item ids])] in file order, filling the maps on the way"""
        kept = []
        for name, items in self.training_data.items():
            if len(items) < 2:
                continue
            if name not in self.seq:
                sid = len(self.seq)
                self.seq[name], self.id2seq[sid] = sid, name
            for it in items:
                if it not in self.item:
                    iid = len(self.item) + 1          # 0 is the padding id
                    self.item[it], self.id2item[iid] = iid, it
            kept.append((name, [self.item[it] for it in items]))
        return kept

    def _index_test(self):
        for name, items in self.test_data.items():
            if name in self.seq:
                self.test_set[name][items[0]] = 1
                self.test_set_item.add(items[0])

    def same_target_index(self):
        """{last training item id: [indices into original_seq]} in file order (cached): the sequences that share a
        target, DuoRec's semantic positives.  The target of a sequence is its last item."""
        if getattr(self, '_same_target', None) is None:
            index = defaultdict(list)
            for n, (_, ids) in enumerate(self.original_seq):
                index[ids[-1]].append(n)
            self._same_target = dict(index)
        return self._same_target

    def get_item_id(self, i):
        return self.item.get(i)

    def get_seq_id(self, i):
        return self.seq.get(i)
