"""What SASRec, BERT4Rec and CL4SRec share: the transformer encoder over an item sequence (reference
model/sequential/SASRec.py's SASRec_Model, BERT4Rec.py's BERT_Encoder) and the staging of a batch's int32 host arrays in
one upload.

The block keeps the reference's semantics, quirks included: the query is the LayerNorm of the input while key and value
are the un-normalised input; the residual adds the normalised query, not the input; the feed-forward block runs on the
output of a second LayerNorm and adds that.  Parameter names and creation order are the reference's, so
``torch.manual_seed`` reproduces its initial weights."""
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import ops
from ...util.structure import PointWiseFeedForward


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


def upload(arrays, device):
    """the host arrays as int32 in ONE host-to-device copy -> one flat view of the device tensor per array, in order"""
    arrays = [np.ascontiguousarray(a, dtype=np.int32).reshape(-1) for a in arrays]
    flat = torch.from_numpy(np.concatenate(arrays)).to(device)
    return list(flat.split([a.size for a in arrays]))


def upload_with_plans(ids, plans, device):
    """upload() of id arrays and of the host plans (tuples of arrays: ops.scatter_plan_host, ops.live_plan_host) that
    travel with them -> (the id views, the plans as tuples of views)"""
    views = upload(list(ids) + [a for plan in plans for a in plan], device)
    rest = iter(views[len(ids):])
    return views[:len(ids)], [tuple(next(rest) for _ in plan) for plan in plans]


class Group:
    """one encoder pass on the device: ids, positions, the padding mask and the plans of its two gathers"""
    __slots__ = ('shape', 'seq', 'pos', 'plans', 'live')

    def __init__(self, shape, seq, pos, plans):
        self.shape, self.seq, self.pos, self.plans = tuple(shape), seq, pos, plans
        self.live = (seq != 0).reshape(*self.shape, 1)


class StagedIds:
    """One (B, L) batch on the device as one Group on the torch front: ids, positions, the further id arrays ``extra`` and
    the scatter plans of the two gathers followed by ``extra_plans``, uploaded together."""
    route_embed = 'torch'

    def __init__(self, seq, pos, device, extra=(), extra_plans=()):
        seq, pos = np.asarray(seq), np.asarray(pos)
        ids = [seq.reshape(-1), pos.reshape(-1)]
        plans = [ops.scatter_plan_host(a) for a in ids] + list(extra_plans)
        views, self.plans = upload_with_plans(ids + list(extra), plans, device)
        self.extra = views[2:] or (None, None)
        group = Group(seq.shape, views[0], views[1], self.plans)
        self.groups, self.shape, self.seq, self.pos, self.live = [group], group.shape, group.seq, group.pos, group.live


class SeqEncoder(nn.Module):
    """item and position tables of ``item_rows`` / ``pos_rows`` rows, n_blocks attention + feed-forward blocks with the
    feed-forward ``activation``, a last LayerNorm; ``causal``: every position sees its past only, else all positions."""

    def __init__(self, item_rows, pos_rows, emb_size, n_blocks, n_heads, drop_rate, attention='hip', activation='relu',
                 causal=True):
        super(SeqEncoder, self).__init__()
        self.item_rows, self.pos_rows, self.emb_size = item_rows, pos_rows, emb_size
        self.block_num, self.head_num, self.drop_rate = n_blocks, n_heads, drop_rate
        self.activation, self.causal = activation, causal
        self._init_model()
        self.attention = attention
        # the in-kernel dropout masks: an attention call takes the counters [rng_counter, + B H L), an embedding front
        # [rng_counter, + B L)
        self.rng_seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        self.rng_counter = 0

    def _init_model(self):
        # creation order = the reference's (state_dict keys and the torch.manual_seed stream depend on it): both tables,
        # the four empty ModuleLists, the embedding dropout, the last LayerNorm, then block by block
        d = self.emb_size
        xavier = nn.init.xavier_uniform_
        self.item_emb = nn.Parameter(xavier(torch.empty(self.item_rows, d)))      # row 0: the padding id
        self.pos_emb = nn.Parameter(xavier(torch.empty(self.pos_rows, d)))
        for name in ('attention_layer_norms', 'attention_layers', 'forward_layer_norms', 'forward_layers'):
            setattr(self, name, nn.ModuleList())
        self.emb_dropout = nn.Dropout(self.drop_rate)
        self.last_layer_norm = nn.LayerNorm(d, eps=1e-8)
        for _ in range(self.block_num):
            self.attention_layer_norms.append(nn.LayerNorm(d, eps=1e-8))
            self.attention_layers.append(nn.MultiheadAttention(d, self.head_num, self.drop_rate))
            self.forward_layer_norms.append(nn.LayerNorm(d, eps=1e-8))
            self.forward_layers.append(PointWiseFeedForward(d, self.drop_rate, self.activation))

    def uses_kernel(self, L, on_device=True):
        """whether the attention core of L positions runs on the fused kernel: the route, the envelope, and a model that
        lives on the device (a CPU model takes torch's expression)"""
        return (self.attention == 'hip' and bool(on_device)
                and ops.seq_attn_supported(int(L), self.head_num, self.emb_size // self.head_num))

    def attention_kernel(self, L, on_device=True):
        """which fused kernel the attention core of L positions runs on: 'resident' (one (sequence, head) in LDS, L up to
        ops.SEQ_ATTN_MAX_LEN; the routes 'hip' and 'tiled'), 'tiled' (64-key blocks, L up to ops.SEQ_ATTN_TILED_MAX_LEN; only
        under the explicit route 'tiled': measured against torch's expression it is not faster at every length, DESIGN.md
        4.28), or None for torch's expression (the torch route, a CPU model, a shape outside the route's envelopes)"""
        if self.attention not in ('hip', 'tiled') or not on_device:
            return None
        heads, dh = self.head_num, self.emb_size // self.head_num
        if ops.seq_attn_supported(int(L), heads, dh):
            return 'resident'
        if self.attention == 'tiled' and ops.seq_attn_tiled_supported(int(L), heads, dh):
            return 'tiled'
        return None

    def _attention(self, mha, query, memory, keep=None):
        """nn.MultiheadAttention(query, memory, memory, attn_mask=causal or None) on (B, L, d) tensors: the packed
        in-projection and the out-projection are torch's Linear, the core between them a fused kernel (attention_kernel) or
        torch's expression"""
        E = self.emb_size
        w, b = mha.in_proj_weight, mha.in_proj_bias
        q = F.linear(query, w[:E], b[:E])
        k = F.linear(memory, w[E:2 * E], b[E:2 * E])
        v = F.linear(memory, w[2 * E:], b[2 * E:])
        p = float(mha.dropout) if self.training else 0.0
        kernel = self.attention_kernel(q.shape[1], q.is_cuda)     # ('resident' == uses_kernel under the route 'hip')
        if kernel is not None:
            B, L = int(q.shape[0]), int(q.shape[1])
            if kernel == 'tiled':
                core = ops.SeqAttnTiledFn.apply(q, k, v, self.head_num, self.causal, keep, p, self.rng_seed, self.rng_counter)
            else:
                fn = ops.SeqAttnFn if self.causal else ops.SeqAttnFullFn
                core = fn.apply(q, k, v, self.head_num, keep, p, self.rng_seed, self.rng_counter)
            if keep is None and p > 0.0:
                self.rng_counter += B * self.head_num * L
        else:
            core = torch_causal_attention(q, k, v, self.head_num, keep, p, self.training, causal=self.causal)
        return mha.out_proj(core)

    def front(self, g, route_embed='torch', emb_keep=None):
        """(B, L, d) rows (item_emb[seq] sqrt(d) + pos_emb[pos]) after dropout, zero at the padding, of the Group g:
        one launch (ops.SeqEmbedFn) for route_embed 'hip', else torch's expression over two ops.GatherRowsFn.
        emb_keep: an optional (B, L, d) keep mask of the dropout, replayed instead of drawn."""
        B, L = g.shape
        d = self.emb_size
        if route_embed == 'hip':
            if not ops.seq_embed_supported(d):
                raise ops.SelfrecHipError(f"engine.embed: hip serves widths {ops.SEQ_EMBED_WIDTHS}, not {d}")
            p = float(self.drop_rate) if self.training else 0.0
            seq_emb = ops.SeqEmbedFn.apply(self.item_emb, self.pos_emb, g.seq, g.pos, g.plans[0], g.plans[1], emb_keep, p,
                                           self.rng_seed, self.rng_counter).reshape(B, L, d)
            if emb_keep is None and p > 0.0:
                self.rng_counter += B * L
            return seq_emb
        items = ops.GatherRowsFn.apply(self.item_emb, g.seq, g.plans[0])
        places = ops.GatherRowsFn.apply(self.pos_emb, g.pos, g.plans[1])
        return self._torch_front(items, places, g.live, emb_keep)

    def _torch_front(self, items, places, live, emb_keep=None):
        seq_emb = (items * self.emb_size ** 0.5 + places).reshape(*live.shape[:2], self.emb_size)
        if emb_keep is not None:
            p = float(self.drop_rate) if self.training else 0.0
            seq_emb = seq_emb * (emb_keep.reshape(seq_emb.shape).to(seq_emb.dtype) / (1.0 - p))
        else:
            seq_emb = self.emb_dropout(seq_emb)
        return seq_emb * live

    def blocks(self, seq_emb, live, attn_keep=None):
        """the attention + feed-forward blocks and the last LayerNorm over (B, L, d) rows; live: the (B, L, 1) padding mask"""
        for i in range(len(self.attention_layers)):
            normalized_emb = self.attention_layer_norms[i](seq_emb)
            keep = None if attn_keep is None else attn_keep[i]
            mha_outputs = self._attention(self.attention_layers[i], normalized_emb, seq_emb, keep)
            seq_emb = normalized_emb + mha_outputs
            seq_emb = self.forward_layer_norms[i](seq_emb)
            seq_emb = self.forward_layers[i](seq_emb)
            seq_emb = seq_emb * live
        return self.last_layer_norm(seq_emb)

    def forward(self, seq, pos, attn_keep=None, staged=None, group=0, emb_keep=None):
        """(B, L, d) hidden states of the id arrays seq / pos (0 = padding), or of staged.groups[group] for a batch already
        on the device (StagedIds, CL4SRec's StagedViews).  attn_keep: optional list, one (B, H, L, L) keep mask per block,
        emb_keep: an optional (B, L, d) keep mask of the embedding dropout; both replayed instead of drawn."""
        dev = self.item_emb.device
        if staged is None and dev.type == 'cuda' and torch.is_grad_enabled():
            staged = StagedIds(seq, pos, dev)
        if staged is not None:
            g = staged.groups[group]
            return self.blocks(self.front(g, staged.route_embed, emb_keep), g.live, attn_keep)
        # a CPU model, evaluation: int64 ids and plain indexing
        seq, pos = np.asarray(seq), np.asarray(pos)
        ids = torch.from_numpy(np.stack([seq.reshape(-1), pos.reshape(-1)]).astype(np.int64)).to(dev)
        live = (ids[0] != 0).reshape(*seq.shape, 1)
        return self.blocks(self._torch_front(self.item_emb[ids[0]], self.pos_emb[ids[1]], live, emb_keep), live, attn_keep)


class LastRowScores:
    """last_hidden / item_table / predict of a SequentialRecommender whose ``model`` is a SeqEncoder: every sequence is
    scored with the hidden row of its last item against the whole item table"""

    def _scored_rows(self, seq, pos, seq_len):
        with torch.no_grad():
            seq_emb = self.model.forward(seq, pos)
            rows = torch.arange(seq_emb.shape[0], device=seq_emb.device)
            last = torch.as_tensor(np.asarray(seq_len, dtype=np.int64) - 1, device=seq_emb.device)
            return seq_emb[rows, last].contiguous()

    def last_hidden(self, seq, pos, seq_len):
        return self._scored_rows(seq, pos, seq_len)

    def item_table(self):
        table = self.model.item_emb
        return table.detach() if table.is_cuda else None

    def predict(self, seq, pos, seq_len):
        hidden = self._scored_rows(seq, pos, seq_len)
        with torch.no_grad():
            score = torch.matmul(hidden, self.model.item_emb.transpose(0, 1))
        return score.cpu().numpy()
