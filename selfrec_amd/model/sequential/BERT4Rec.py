"""BERT4Rec (Sun et al., CIKM'19; reference model/sequential/BERT4Rec.py): a bidirectional transformer over each item
sequence, trained to recover randomly masked items with a softmax cross-entropy over the whole item table.  Config block
``BERT4Rec: {n_blocks, drop_rate, n_heads, mask_rate}``, ``max.len``.

What runs where: the attention core of every block -- scores over ALL positions, softmax, dropout on the
probabilities, the product with V -- is one fused launch each way (ops.SeqAttnFullFn, csrc/seqrec.hip with the causal flag
off), and the loss with both its gradients is one call that never materialises the M x N logits (ops.TableCeFn,
csrc/contrastive.hip); the gathers of the two tables scatter their gradients in a fixed order (ops.GatherRowsFn).
LayerNorm, the Linear layers, GELU and Adam are torch's.  ``engine.attention: torch`` (``SRH_SASREC_ATTN=torch``) routes the
attention core, ``engine.ce: torch`` (``SRH_BERT4REC_CE=torch``) the loss through torch's own expressions on the same
inputs: the A/B partners of the kernels, and the routes of shapes outside their envelopes.  A model on the CPU takes
torch's expressions throughout.

The network is encoder.SeqEncoder, shared with SASRec and CL4SRec.  The mirror keeps the reference's semantics, quirks
included:
  * the item table has item_num + 2 rows (0: padding, item_num + 1: the mask token), the position table max_len + 2;
  * no mask of any kind in the attention: padded positions are zero rows, their keys and values the in-projection bias,
    and every query attends to them;
  * item_mask_for_bert appends a sequence's labels in random.sample's order while seq_emb[masked > 0] takes the hidden
    rows in ascending position order, so inside a sequence rows and labels are paired in different orders;
  * the loss is the cross-entropy MEAN over the M masked rows divided by M once more;
  * predict() edits seq and pos in place, puts the mask token BEHIND the last item of a row shorter than max_len and
    still scores the hidden row at seq_len - 1 -- the last real item, not the token;
  * scores run over all item_num + 2 rows; test() drops ids 0 and item_num + 1 from the names.

Host work of a step: ``StagedMaskedBatch`` turns the augmented ids, the positions, the masked positions and the labels
into ONE int32 upload that also carries the two scatter plans."""
import random
from math import floor

import numpy as np
import torch
import torch.nn.functional as F

from ... import ops
from ...base.seq_recommender import SequentialRecommender
from ...util.loss_torch import l2_reg_loss
from ...util.route import route
from ...util.sampler import next_batch_sequence
from .encoder import LastRowScores, SeqEncoder, StagedIds
from .SASRec import attention_route


def ce_route(conf=None):
    """'hip' or 'torch': SRH_BERT4REC_CE, else the conf's engine.ce, else the kernel"""
    return route('SRH_BERT4REC_CE', 'engine.ce', conf)


def item_mask_for_bert(seq, seq_len, mask_ratio, mask_idx):
    """BERT4Rec.py:47-56: per sequence, random.sample(range(len), max(floor(len * ratio), 1)) positions become mask_idx.
    -> (augmented seq, masked (0/1, seq's shape), labels: the replaced ids in the SAMPLE's order, sequence by sequence)"""
    augmented_seq = seq.copy()
    masked = np.zeros_like(augmented_seq)
    labels = []
    for i in range(len(seq)):
        to_be_masked = random.sample(range(seq_len[i]), max(floor(seq_len[i] * mask_ratio), 1))
        masked[i, to_be_masked] = 1
        labels += list(augmented_seq[i, to_be_masked])
        augmented_seq[i, to_be_masked] = mask_idx
    return augmented_seq, masked, np.array(labels)


def place_mask_token(seq, pos, seq_len, max_len, mask_idx):
    """predict()'s in-place edits (BERT4Rec.py:66-74): a full row loses its first item and ends with the token, a shorter
    row gets the token behind its last item"""
    for i, length in enumerate(seq_len):
        if length == max_len:
            seq[i, :length - 1] = seq[i, 1:]
            pos[i, :length - 1] = pos[i, 1:]
            pos[i, length - 1] = length
            seq[i, length - 1] = mask_idx
        else:
            pos[i, length] = length + 1
            seq[i, length] = mask_idx


class StagedMaskedBatch(StagedIds):
    """One batch on the device: ids, positions, the flat indices of the masked positions (ascending), the labels and the
    scatter plans of the two gathers, uploaded together."""

    def __init__(self, seq, pos, masked, labels, device):
        targets = []
        if masked is not None:
            targets = [np.flatnonzero(np.asarray(masked).reshape(-1) > 0), np.asarray(labels).reshape(-1)]
            if targets[0].size != targets[1].size:
                raise ValueError("StagedMaskedBatch: one label per masked position expected")
        super().__init__(seq, pos, device, targets)
        self.masked_idx, self.labels = self.extra
        self.n_masked = int(targets[0].size) if targets else 0


class BERT4Rec(LastRowScores, SequentialRecommender):
    def __init__(self, conf, training_set, test_set):
        super(BERT4Rec, self).__init__(conf, training_set, test_set)
        section = self.config['BERT4Rec']
        self.aug_rate = float(section['mask_rate'])
        self.model = BERT_Encoder(self.data, self.emb_size, self.max_len, int(section['n_blocks']), int(section['n_heads']),
                                  float(section['drop_rate']), attention=attention_route(conf))
        self.ce = ce_route(conf)
        self.epoch_losses = []

    def item_mask_for_bert(self, seq, seq_len, mask_ratio, mask_idx):
        return item_mask_for_bert(seq, seq_len, mask_ratio, mask_idx)

    def train(self):
        net = self.model.cuda()
        adam = torch.optim.Adam(net.parameters(), lr=self.lRate)
        device = net.item_emb.device
        for epoch in range(self.maxEpoch):
            net.train()
            seen = []
            batches = next_batch_sequence(self.data, self.batch_size, max_len=self.max_len)
            for n, (seq, pos, _y, _neg_idx, seq_len) in enumerate(batches):
                aug_seq, masked, labels = self.item_mask_for_bert(seq, seq_len, self.aug_rate, self.data.item_num + 1)
                staged = StagedMaskedBatch(aug_seq, pos, masked, labels, device)
                seq_emb = net.forward(aug_seq, pos, staged=staged)
                rec_loss = self.calculate_loss(seq_emb, masked, labels, staged=staged)
                batch_loss = rec_loss + l2_reg_loss(self.reg, net.item_emb)
                adam.zero_grad()
                batch_loss.backward()
                adam.step()
                seen.append(batch_loss.detach())
                if n % 50 == 0:
                    print('training:', epoch + 1, 'batch', n, 'batch_loss:', batch_loss.item(), 'rec_loss:', rec_loss.item())
            self.epoch_losses.append([float(v) for v in torch.stack(seen).cpu()])
            net.eval()
            self.fast_evaluation(epoch)

    def uses_ce_kernel(self, on_device=True):
        return (self.ce == 'hip' and bool(on_device)
                and ops.padded_width(self.emb_size, ops.TABLE_NCE_WIDTHS) is not None)

    def calculate_loss(self, seq_emb, masked, labels, staged=None):
        """F.cross_entropy(H_masked @ item_emb.T, labels) / M (BERT4Rec.py:58-62): the cross-entropy SUM over the M masked
        rows times 1 / M^2, one kernel call with both gradients"""
        dev = seq_emb.device
        if staged is None or staged.masked_idx is None:
            staged = StagedMaskedBatch(masked, masked, masked, labels, dev)
        M = staged.n_masked
        rows = seq_emb.reshape(-1, seq_emb.shape[-1])[staged.masked_idx.long()]
        table = self.model.item_emb
        if self.uses_ce_kernel(rows.is_cuda):
            return ops.TableCeFn.apply(rows, table, staged.labels, 1.0 / (float(M) * float(M)))
        return F.cross_entropy(torch.mm(rows, table.t()), staged.labels.long()) / M

    def last_hidden(self, seq, pos, seq_len):
        """the rows predict() scores, from copies of seq and pos"""
        return self._scored_rows(np.array(seq, copy=True), np.array(pos, copy=True), seq_len)

    def _scored_rows(self, seq, pos, seq_len):
        """LastRowScores' rows behind the mask token, placed in seq and pos themselves: predict() edits its arguments,
        as the reference does"""
        place_mask_token(seq, pos, seq_len, self.max_len, self.data.item_num + 1)
        return super()._scored_rows(seq, pos, seq_len)


class BERT_Encoder(SeqEncoder):
    """the bidirectional encoder: item_num + 2 item rows (0: padding, item_num + 1: the mask token), max_len + 2
    positions, GELU, no attention mask"""

    def __init__(self, data, emb_size, max_len, n_blocks, n_heads, drop_rate, attention='hip'):
        super(BERT_Encoder, self).__init__(data.item_num + 2, max_len + 2, emb_size, n_blocks, n_heads, drop_rate, attention,
                                           activation='gelu', causal=False)
