"""``SequentialRecommender`` with the surface of reference base/seq_recommender.py:8-83.

``test()`` ranks ``max_N`` over ALL rows of the item table -- ``item_num + 1`` with the padding row 0 (SASRec),
``item_num + 2`` with BERT4Rec's mask token behind them -- and then drops ids 0 and ``> item_num`` from the list, so a list
can be that many names shorter than ``max_N``.  The reference drops it from the NAMES only and zips
them with the unfiltered scores (seq_recommender.py:49-50): behind row 0's place every name carries its predecessor's
score.  The lists here are the reference's, that pairing included; the ranking metrics read the names only.  A model that exposes
``last_hidden(seq, pos, seq_len)`` and a device ``item_table()`` is scored and ranked on the device: ``ops.gemm_nt`` for
the score rows, the k-largest kernel over ``max_N + 1`` columns, rows holding a tie among those redone in the
reference's heap order on the host (the tie contract of base/graph_recommender.py).  Any other model takes the per-row
loop over ``predict()``."""
import numpy as np
import torch

from .. import ops
from ..data.sequence import Sequence
from ..util.algorithm import find_k_largest
from ..util.evaluation import ranking_evaluation
from ..util.sampler import next_batch_sequence_for_test
from .recommender import Recommender

DEVICE_TOPK_MAX = 128          # srh_topk_rows: k <= 128


class SequentialRecommender(Recommender):
    def __init__(self, conf, training_set, test_set, **kwargs):
        super().__init__(conf, training_set, test_set, **kwargs)
        self.data = Sequence(conf, training_set, test_set)
        self.bestPerformance = []
        self.max_len = int(self.config['max.len'])
        self.topN = [int(num) for num in self.ranking]
        self.max_N = max(self.topN)

    def print_model_info(self):
        super().print_model_info()
        print(f'Training Set Size: (sequence number: {self.data.raw_seq_num}, item number: {self.data.item_num})')
        print('=' * 80)

    def predict(self, seq, pos, seq_len):
        return -1

    # models served on the device override these two
    def last_hidden(self, seq, pos, seq_len):
        """(rows, d) device tensor: the hidden state each sequence is scored with, or None"""
        return None

    def item_table(self):
        return None

    def _rank_on_device(self, hidden, table):
        """ids (int64), scores (float32) numpy (rows, max_N), best first, in find_k_largest's order"""
        k = self.max_N
        w = ops.padded_width(int(table.shape[1]), ops.ROW_WIDTHS)
        scores = ops.gemm_nt(ops.pad_cols(hidden.detach().float(), w), ops.pad_cols(table.detach().float(), w))
        ids_dev, sc_dev = ops.topk_trim_mark_ties(*ops.topk_rows(scores, k + 1))
        ids, sc = ids_dev.cpu().numpy().astype(np.int64), sc_dev.cpu().numpy()
        tied = np.flatnonzero(ids[:, 0] < 0)
        if tied.size:
            rows = scores[torch.from_numpy(tied).to(scores.device)].cpu().numpy()
            for j, r in enumerate(tied.tolist()):
                ids[r], sc[r] = ops.find_k_largest_host(k, rows[j])
        return ids, sc

    def test(self):
        data = self.data
        names = [name for name, _ in data.original_seq]
        table = self.item_table()
        n_rows = data.item_num + 1 if table is None else int(table.shape[0])      # the columns a model scores
        on_device = table is not None and self.max_N + 1 <= min(DEVICE_TOPK_MAX, n_rows)
        rec_list = {}
        for n, (seq, pos, seq_len) in enumerate(next_batch_sequence_for_test(data, self.batch_size, max_len=self.max_len)):
            block = names[n * self.batch_size:(n + 1) * self.batch_size]
            hidden = self.last_hidden(seq, pos, seq_len) if on_device else None
            if hidden is not None:
                ids, scores = self._rank_on_device(hidden, table)
                ranked = zip(ids.tolist(), scores.tolist())
            else:
                ranked = (find_k_largest(self.max_N, row) for row in self.predict(seq, pos, seq_len))
            for name, (row_ids, row_scores) in zip(block, ranked):
                item_names = [data.id2item[i] for i in row_ids if i != 0 and i <= data.item_num]
                rec_list[name] = list(zip(item_names, row_scores))      # (the reference's pairing: see the docstring)
        return rec_list

    def evaluate(self, rec_list):
        return 0

    def fast_evaluation(self, epoch):
        print('Evaluating the model...')
        rec_list = self.test()
        measure = ranking_evaluation(self.data.test_set, rec_list, [self.max_N])
        performance = {}
        for line in measure[1:]:
            key, value = line.strip().split(':')
            performance[key] = float(value)
        improved = not self.bestPerformance
        if self.bestPerformance:
            # majority vote over the metrics, as reference seq_recommender.py:67-71
            votes = sum(1 if self.bestPerformance[1][k] > performance[k] else -1 for k in performance)
            improved = votes < 0
        if improved:
            self.bestPerformance = [epoch + 1, performance]
            self.save()
        print('-' * 80)
        print(f'Real-Time Ranking Performance (Top-{self.max_N} Item Recommendation)')
        print(f'*Current Performance*\nEpoch: {epoch + 1}, ' + ', '.join(f'{k}: {v}' for k, v in performance.items()))
        best = ', '.join(f'{k}: {v}' for k, v in self.bestPerformance[1].items())
        print(f'*Best Performance*\nEpoch: {self.bestPerformance[0]}, {best}')
        print('-' * 80)
        return measure
