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

The mirror keeps the reference's semantics, quirks included:
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
import os
import random
from math import floor

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import ops
from ...base.seq_recommender import SequentialRecommender
from ...util.loss_torch import l2_reg_loss
from ...util.sampler import next_batch_sequence
from ...util.structure import PointWiseFeedForward
from .SASRec import attention_route, torch_causal_attention


def ce_route(conf=None):
    """'hip' or 'torch': SRH_BERT4REC_CE, else the conf's engine.ce, else the kernel"""
    route = os.environ.get('SRH_BERT4REC_CE')
    if route is None and conf is not None and conf.contain('engine.ce'):
        route = conf['engine.ce']
    route = 'hip' if route is None else str(route).strip().lower()
    if route not in ('hip', 'torch'):
        raise ValueError(f"engine.ce / SRH_BERT4REC_CE: {route!r} is neither 'hip' nor 'torch'")
    return route


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


class StagedMaskedBatch:
    """One batch on the device: ids, positions, the flat indices of the masked positions (ascending), the labels and the
    scatter plans of the two gathers, uploaded together."""

    def __init__(self, seq, pos, masked, labels, device):
        seq, pos = np.asarray(seq), np.asarray(pos)
        self.shape = seq.shape
        parts = [seq.reshape(-1), pos.reshape(-1)]
        with_labels = masked is not None
        if with_labels:
            parts += [np.flatnonzero(np.asarray(masked).reshape(-1) > 0), np.asarray(labels).reshape(-1)]
            if parts[2].size != parts[3].size:
                raise ValueError("StagedMaskedBatch: one label per masked position expected")
        plans = [ops.scatter_plan_host(parts[0]), ops.scatter_plan_host(parts[1])]
        parts = [np.ascontiguousarray(a, dtype=np.int32) for a in parts] + [a for plan in plans for a in plan]
        flat = torch.from_numpy(np.concatenate(parts)).to(device)
        views, at = [], 0
        for a in parts:
            views.append(flat[at:at + a.size])
            at += a.size
        n_ids = 4 if with_labels else 2
        self.seq, self.pos = views[0], views[1]
        self.masked_idx, self.labels = (views[2], views[3]) if with_labels else (None, None)
        self.n_masked = int(parts[2].size) if with_labels else 0
        self.plans = [tuple(views[n_ids + 3 * k:n_ids + 3 * k + 3]) for k in range(2)]
        self.live = (self.seq != 0).reshape(*self.shape, 1)


class BERT4Rec(SequentialRecommender):
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
        seq, pos = np.array(seq, copy=True), np.array(pos, copy=True)
        return self._scored_rows(seq, pos, seq_len)

    def _scored_rows(self, seq, pos, seq_len):
        place_mask_token(seq, pos, seq_len, self.max_len, self.data.item_num + 1)
        with torch.no_grad():
            seq_emb = self.model.forward(seq, pos)
            rows = torch.arange(seq_emb.shape[0], device=seq_emb.device)
            last = torch.as_tensor(np.asarray(seq_len, dtype=np.int64) - 1, device=seq_emb.device)
            return seq_emb[rows, last].contiguous()

    def item_table(self):
        table = self.model.item_emb
        return table.detach() if table.is_cuda else None

    def predict(self, seq, pos, seq_len):
        hidden = self._scored_rows(seq, pos, seq_len)          # (edits seq and pos in place, as the reference does)
        with torch.no_grad():
            score = torch.matmul(hidden, self.model.item_emb.transpose(0, 1))
        return score.cpu().numpy()


class BERT_Encoder(nn.Module):
    def __init__(self, data, emb_size, max_len, n_blocks, n_heads, drop_rate, attention='hip'):
        super(BERT_Encoder, self).__init__()
        self.data = data
        self.emb_size, self.max_len = emb_size, max_len
        self.block_num, self.head_num, self.drop_rate = n_blocks, n_heads, drop_rate
        self._init_model()
        self.attention = attention
        # the in-kernel dropout masks of the attention: every call takes the counters [rng_counter, + B H L)
        self.rng_seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        self.rng_counter = 0

    def _init_model(self):
        # creation order = the reference's (state_dict keys and the torch.manual_seed stream depend on it)
        d = self.emb_size
        xavier = nn.init.xavier_uniform_
        self.item_emb = nn.Parameter(xavier(torch.empty(self.data.item_num + 2, d)))   # 0: padding, item_num + 1: mask
        self.pos_emb = nn.Parameter(xavier(torch.empty(self.max_len + 2, d)))
        for name in ('attention_layer_norms', 'attention_layers', 'forward_layer_norms', 'forward_layers'):
            setattr(self, name, nn.ModuleList())
        self.emb_dropout = nn.Dropout(self.drop_rate)
        self.last_layer_norm = nn.LayerNorm(d, eps=1e-8)
        for _ in range(self.block_num):
            self.attention_layer_norms.append(nn.LayerNorm(d, eps=1e-8))
            self.attention_layers.append(nn.MultiheadAttention(d, self.head_num, self.drop_rate))
            self.forward_layer_norms.append(nn.LayerNorm(d, eps=1e-8))
            self.forward_layers.append(PointWiseFeedForward(d, self.drop_rate, 'gelu'))

    def uses_kernel(self, L, on_device=True):
        """whether the attention core of L positions runs on the fused kernel: the route, the envelope, and a model that
        lives on the device (a CPU model takes torch's expression)"""
        return (self.attention == 'hip' and bool(on_device)
                and ops.seq_attn_supported(int(L), self.head_num, self.emb_size // self.head_num))

    def _attention(self, mha, query, memory, keep=None):
        """nn.MultiheadAttention(query, memory, memory, attn_mask=None) on (B, L, d) tensors: the packed in-projection and
        the out-projection are torch's Linear, the core between them the fused kernel or torch's expression"""
        E = self.emb_size
        w, b = mha.in_proj_weight, mha.in_proj_bias
        q = F.linear(query, w[:E], b[:E])
        k = F.linear(memory, w[E:2 * E], b[E:2 * E])
        v = F.linear(memory, w[2 * E:], b[2 * E:])
        p = float(mha.dropout) if self.training else 0.0
        if self.uses_kernel(q.shape[1], q.is_cuda):
            B, L = int(q.shape[0]), int(q.shape[1])
            core = ops.SeqAttnFullFn.apply(q, k, v, self.head_num, keep, p, self.rng_seed, self.rng_counter)
            if keep is None and p > 0.0:
                self.rng_counter += B * self.head_num * L
        else:
            core = torch_causal_attention(q, k, v, self.head_num, keep, p, self.training, causal=False)
        return mha.out_proj(core)

    def forward(self, seq, pos, attn_keep=None, staged=None):
        """(B, L, d) hidden states of the id arrays seq / pos (0 = padding).  attn_keep: optional list, one (B, H, L, L)
        keep mask per block, replayed instead of drawn.  staged: the batch already on the device (StagedMaskedBatch)."""
        dev = self.item_emb.device
        training_on_device = dev.type == 'cuda' and torch.is_grad_enabled()
        if staged is None and training_on_device:
            staged = StagedMaskedBatch(seq, pos, None, None, dev)
        if staged is not None:
            B, L = staged.shape
            items = ops.GatherRowsFn.apply(self.item_emb, staged.seq, staged.plans[0])
            places = ops.GatherRowsFn.apply(self.pos_emb, staged.pos, staged.plans[1])
            live = staged.live
        else:
            seq, pos = np.asarray(seq), np.asarray(pos)
            B, L = seq.shape
            ids = torch.from_numpy(np.stack([seq.reshape(-1), pos.reshape(-1)]).astype(np.int64)).to(dev)
            items, places = self.item_emb[ids[0]], self.pos_emb[ids[1]]
            live = (ids[0] != 0).reshape(B, L, 1)
        seq_emb = (items * self.emb_size ** 0.5 + places).reshape(B, L, self.emb_size)
        seq_emb = self.emb_dropout(seq_emb)
        seq_emb = seq_emb * live
        for i in range(len(self.attention_layers)):
            normalized_emb = self.attention_layer_norms[i](seq_emb)
            keep = None if attn_keep is None else attn_keep[i]
            mha_outputs = self._attention(self.attention_layers[i], normalized_emb, seq_emb, keep)
            seq_emb = normalized_emb + mha_outputs
            seq_emb = self.forward_layer_norms[i](seq_emb)
            seq_emb = self.forward_layers[i](seq_emb)
            seq_emb = seq_emb * live
        return self.last_layer_norm(seq_emb)
