"""SASRec (Kang & McAuley, ICDM'18; reference model/sequential/SASRec.py): a causal transformer over each item sequence,
trained with one sampled negative per position.  Config block ``SASRec: {n_blocks, drop_rate, n_heads}``, ``max.len``.

What runs where: the attention core of every block -- scores, causal mask, softmax, dropout on the
probabilities, the product with V -- is one fused launch each way (ops.SeqAttnFn, csrc/seqrec.hip), and the loss with
its gradients is one kernel (ops.SeqBceFn); the gathers of the item and position tables scatter their gradients in a
fixed order (ops.GatherRowsFn).  LayerNorm, the Linear layers and Adam are torch's.  ``engine.attention: torch`` (or
``SRH_SASREC_ATTN=torch``) routes the attention core through torch's own expression on the same projected inputs: the A/B
partner of the kernel, and the route of shapes outside its envelope (``max.len`` > 64).

The block keeps the reference's semantics, quirks included: the query is the LayerNorm of the input while key and value
are the un-normalised input; the residual adds the normalised query, not the input; the feed-forward block runs on the
output of a second LayerNorm and adds that; only a causal mask (padding sits on the right, so no valid row sees it).
Parameter names and creation order are the reference's, so ``torch.manual_seed`` reproduces its initial weights.

Host work of a step: ``stage_batch`` turns the sampler's four id arrays into ONE int32 upload that also
carries the three scatter plans (items, positions, [targets; negatives]); forward and loss read views of it."""
import math
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import ops
from ...base.seq_recommender import SequentialRecommender
from ...util.loss_torch import l2_reg_loss
from ...util.sampler import next_batch_sequence
from ...util.structure import PointWiseFeedForward


def attention_route(conf=None):
    """'hip' or 'torch': SRH_SASREC_ATTN, else the conf's engine.attention, else the kernel"""
    route = os.environ.get('SRH_SASREC_ATTN')
    if route is None and conf is not None and conf.contain('engine.attention'):
        route = conf['engine.attention']
    route = 'hip' if route is None else str(route).strip().lower()
    if route not in ('hip', 'torch'):
        raise ValueError(f"engine.attention / SRH_SASREC_ATTN: {route!r} is neither 'hip' nor 'torch'")
    return route


def torch_causal_attention(q, k, v, n_heads, keep=None, drop_p=0.0, training=False, causal=True):
    """torch's expression of the attention core on projected (B, L, H dh) tensors: the partner of ops.SeqAttnFn, and
    with causal=False (no mask at all: BERT4Rec) of ops.SeqAttnFullFn"""
    B, L, E = q.shape
    dh = E // n_heads
    qh, kh, vh = (t.reshape(B, L, n_heads, dh).transpose(1, 2) for t in (q, k, v))
    s = torch.matmul(qh * (1.0 / math.sqrt(dh)), kh.transpose(-1, -2))
    if causal:
        s = s.masked_fill(~torch.ones((L, L), dtype=torch.bool, device=q.device).tril(), float('-inf'))
    p = torch.softmax(s, dim=-1)
    if keep is not None:
        p = p * (keep.to(p.dtype) / (1.0 - drop_p))
    elif drop_p > 0.0:
        p = F.dropout(p, drop_p, training)
    return torch.matmul(p, vh).transpose(1, 2).reshape(B, L, E)


class StagedBatch:
    """One training batch on the device: ids, masks and the scatter plans of its three gathers, uploaded together."""

    def __init__(self, seq, pos, y, neg, device):
        seq, pos = np.asarray(seq), np.asarray(pos)
        self.shape = seq.shape
        parts = [seq.reshape(-1), pos.reshape(-1)]
        with_targets = y is not None
        if with_targets:
            y, neg = np.asarray(y).reshape(-1), np.asarray(neg).reshape(-1)
            parts += [y, neg]
        plans = [ops.scatter_plan_host(parts[0]), ops.scatter_plan_host(parts[1])]
        if with_targets:
            plans.append(ops.scatter_plan_host(np.concatenate([y, neg])))
        parts = [np.ascontiguousarray(a, dtype=np.int32) for a in parts] + [a for plan in plans for a in plan]
        flat = torch.from_numpy(np.concatenate(parts)).to(device)
        views, at = [], 0
        for a in parts:
            views.append(flat[at:at + a.size])
            at += a.size
        n_ids = 4 if with_targets else 2
        self.seq, self.pos = views[0], views[1]
        self.y, self.neg = (views[2], views[3]) if with_targets else (None, None)
        self.plans = [tuple(views[n_ids + 3 * k:n_ids + 3 * k + 3]) for k in range(len(plans))]
        self.live = (self.seq != 0).reshape(*self.shape, 1)
        self.valid = (self.pos != 0).to(torch.uint8)
        self.n_valid = int(np.count_nonzero(pos))


class SASRec(SequentialRecommender):
    def __init__(self, conf, training_set, test_set):
        super(SASRec, self).__init__(conf, training_set, test_set)
        section = self.config['SASRec']
        self.model = SASRec_Model(self.data, self.emb_size, self.max_len, int(section['n_blocks']),
                                  int(section['n_heads']), float(section['drop_rate']), attention=attention_route(conf))
        self.rec_loss = torch.nn.BCEWithLogitsLoss()
        self.epoch_losses = []

    def train(self):
        net = self.model.cuda()
        adam = torch.optim.Adam(net.parameters(), lr=self.lRate)
        device = net.item_emb.device
        for epoch in range(self.maxEpoch):
            net.train()
            seen = []
            batches = next_batch_sequence(self.data, self.batch_size, max_len=self.max_len)
            for n, (seq, pos, y, neg_idx, _lens) in enumerate(batches):
                staged = StagedBatch(seq, pos, y, neg_idx, device)
                hidden = net.forward(seq, pos, staged=staged)
                batch_loss = self.calculate_loss(hidden, y, neg_idx, pos, staged=staged) + l2_reg_loss(self.reg, net.item_emb)
                adam.zero_grad()
                batch_loss.backward()
                adam.step()
                seen.append(batch_loss.detach())
                if n % 50 == 0:
                    print('training:', epoch + 1, 'batch', n, 'rec_loss:', batch_loss.item())
            self.epoch_losses.append([float(v) for v in torch.stack(seen).cpu()])
            net.eval()
            self.fast_evaluation(epoch)

    def calculate_loss(self, seq_emb, y, neg, pos, staged=None):
        """both BCE-with-logits means over the positions with pos != 0 (SASRec.py:44-53), one kernel"""
        if staged is None or staged.y is None:
            staged = StagedBatch(pos, pos, y, neg, seq_emb.device)
        hidden = seq_emb.reshape(-1, seq_emb.shape[-1])
        return ops.SeqBceFn.apply(hidden, self.model.item_emb, staged.y, staged.neg, staged.valid, staged.n_valid,
                                  staged.plans[2])

    def last_hidden(self, seq, pos, seq_len):
        with torch.no_grad():
            seq_emb = self.model.forward(seq, pos)
            rows = torch.arange(seq_emb.shape[0], device=seq_emb.device)
            last = torch.as_tensor(np.asarray(seq_len, dtype=np.int64) - 1, device=seq_emb.device)
            return seq_emb[rows, last].contiguous()

    def item_table(self):
        table = self.model.item_emb
        return table.detach() if table.is_cuda else None

    def predict(self, seq, pos, seq_len):
        hidden = self.last_hidden(seq, pos, seq_len)
        with torch.no_grad():
            score = torch.matmul(hidden, self.model.item_emb.transpose(0, 1))
        return score.cpu().numpy()


class SASRec_Model(nn.Module):
    def __init__(self, data, emb_size, max_len, n_blocks, n_heads, drop_rate, attention='hip'):
        super(SASRec_Model, self).__init__()
        self.data = data
        self.emb_size, self.max_len = emb_size, max_len
        self.block_num, self.head_num, self.drop_rate = n_blocks, n_heads, drop_rate
        self._init_model()
        self.attention = attention
        # the in-kernel dropout masks of the attention: every call takes the counters [rng_counter, + B H L)
        self.rng_seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        self.rng_counter = 0

    def _init_model(self):
        # creation order = the reference's (state_dict keys and the torch.manual_seed stream depend on it): both tables,
        # the four empty ModuleLists, the embedding dropout, the last LayerNorm, then block by block
        d = self.emb_size
        xavier = nn.init.xavier_uniform_
        self.item_emb = nn.Parameter(xavier(torch.empty(self.data.item_num + 1, d)))      # row 0: the padding id
        self.pos_emb = nn.Parameter(xavier(torch.empty(self.max_len + 1, d)))
        for name in ('attention_layer_norms', 'attention_layers', 'forward_layer_norms', 'forward_layers'):
            setattr(self, name, nn.ModuleList())
        self.emb_dropout = nn.Dropout(self.drop_rate)
        self.last_layer_norm = nn.LayerNorm(d, eps=1e-8)
        for _ in range(self.block_num):
            self.attention_layer_norms.append(nn.LayerNorm(d, eps=1e-8))
            self.attention_layers.append(nn.MultiheadAttention(d, self.head_num, self.drop_rate))
            self.forward_layer_norms.append(nn.LayerNorm(d, eps=1e-8))
            self.forward_layers.append(PointWiseFeedForward(d, self.drop_rate))

    def uses_kernel(self, L, on_device=True):
        """whether the attention core of L positions runs on the fused kernel: the route, the envelope, and a model that
        lives on the device (a CPU model takes torch's expression)"""
        return (self.attention == 'hip' and bool(on_device)
                and ops.seq_attn_supported(int(L), self.head_num, self.emb_size // self.head_num))

    def _attention(self, mha, query, memory, keep=None):
        """nn.MultiheadAttention(query, memory, memory, attn_mask=causal) on (B, L, d) tensors: the packed in-projection
        and the out-projection are torch's Linear, the core between them the fused kernel or torch's expression"""
        E = self.emb_size
        w, b = mha.in_proj_weight, mha.in_proj_bias
        q = F.linear(query, w[:E], b[:E])
        k = F.linear(memory, w[E:2 * E], b[E:2 * E])
        v = F.linear(memory, w[2 * E:], b[2 * E:])
        p = float(mha.dropout) if self.training else 0.0
        if self.uses_kernel(q.shape[1], q.is_cuda):
            B, L = int(q.shape[0]), int(q.shape[1])
            core = ops.SeqAttnFn.apply(q, k, v, self.head_num, keep, p, self.rng_seed, self.rng_counter)
            if keep is None and p > 0.0:
                self.rng_counter += B * self.head_num * L
        else:
            core = torch_causal_attention(q, k, v, self.head_num, keep, p, self.training)
        return mha.out_proj(core)

    def forward(self, seq, pos, attn_keep=None, staged=None):
        """(B, L, d) hidden states of the id arrays seq / pos (0 = padding).  attn_keep: optional list, one (B, H, L, L)
        keep mask per block, replayed instead of drawn.  staged: the batch already on the device (StagedBatch)."""
        dev = self.item_emb.device
        training_on_device = dev.type == 'cuda' and torch.is_grad_enabled()
        if staged is None and training_on_device:
            staged = StagedBatch(seq, pos, None, None, dev)
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
