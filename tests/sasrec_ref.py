"""float64 torch restatement of SASRec -- TEST INFRASTRUCTURE ONLY (the product never imports it).

Written from the model's semantics, not from the reference's file: ``params`` is a dict of float64
tensors under the reference's state_dict names.  Every dropout takes an INJECTED keep mask (1 = keep), scaled by
1 / (1 - p) as nn.Dropout scales.  tests/test_sasrec_cpu.py pins it to the reference-run golden."""
import math

import numpy as np
import torch

from tests import counter_rng


def layer_norm(x, w, b, eps=1e-8):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def _drop(x, keep, p):
    if keep is None:
        return x
    return x * torch.as_tensor(keep, dtype=x.dtype) / (1.0 - p)


def attention(q, k, v, n_heads, keep=None, drop_p=0.0):
    """causal attention of projected (B, L, H dh) tensors; keep: (B, H, L, L) or None"""
    B, L, E = q.shape
    dh = E // n_heads
    out = torch.zeros_like(q)
    causal = torch.ones(L, L, dtype=torch.bool).tril()
    for h in range(n_heads):
        c = slice(h * dh, (h + 1) * dh)
        s = torch.einsum('bid,bjd->bij', q[..., c], k[..., c]) / math.sqrt(dh)
        p = torch.softmax(s.masked_fill(~causal, float('-inf')), dim=-1)
        p = _drop(p, None if keep is None else torch.as_tensor(keep)[:, h], drop_p)
        out[..., c] = torch.einsum('bij,bjd->bid', p, v[..., c])
    return out


def forward(params, seq, pos, n_blocks, n_heads, drop_p=0.0, emb_keep=None, attn_keep=None, ffn_keep=None):
    """(B, L, d) hidden states.  emb_keep (B, L, d); attn_keep / ffn_keep: one mask per block ((B, H, L, L) / (B, L, d))"""
    seq, pos = np.asarray(seq), np.asarray(pos)
    d = params['item_emb'].shape[1]
    x = params['item_emb'][torch.from_numpy(seq).long()] * d ** 0.5 + params['pos_emb'][torch.from_numpy(pos).long()]
    x = _drop(x, emb_keep, drop_p)
    live = torch.from_numpy(seq != 0).unsqueeze(-1).to(x.dtype)
    x = x * live
    for i in range(n_blocks):
        n = layer_norm(x, params[f'attention_layer_norms.{i}.weight'], params[f'attention_layer_norms.{i}.bias'])
        w, b = params[f'attention_layers.{i}.in_proj_weight'], params[f'attention_layers.{i}.in_proj_bias']
        q = n @ w[:d].T + b[:d]                     # the query is the normalised input,
        k = x @ w[d:2 * d].T + b[d:2 * d]           # key and value the un-normalised one
        v = x @ w[2 * d:].T + b[2 * d:]
        a = attention(q, k, v, n_heads, None if attn_keep is None else attn_keep[i], drop_p)
        a = a @ params[f'attention_layers.{i}.out_proj.weight'].T + params[f'attention_layers.{i}.out_proj.bias']
        x = layer_norm(n + a, params[f'forward_layer_norms.{i}.weight'], params[f'forward_layer_norms.{i}.bias'])
        hdn = torch.relu(x @ params[f'forward_layers.{i}.pwff.0.weight'].T + params[f'forward_layers.{i}.pwff.0.bias'])
        f = hdn @ params[f'forward_layers.{i}.pwff.2.weight'].T + params[f'forward_layers.{i}.pwff.2.bias']
        x = (_drop(f, None if ffn_keep is None else ffn_keep[i], drop_p) + x) * live
    return layer_norm(x, params['last_layer_norm.weight'], params['last_layer_norm.bias'])


def bce_with_logits(x, y):
    """max(x, 0) - x y + log1p(exp(-|x|)), elementwise"""
    return torch.clamp(x, min=0) - x * y + torch.log1p(torch.exp(-x.abs()))


def bce_means(hidden, table, y, neg, valid):
    """(positive mean, negative mean) over the rows with valid: hidden (R, d), ids (R,), valid (R,) bool"""
    idx = torch.from_numpy(np.flatnonzero(np.asarray(valid).reshape(-1)))
    h = hidden.reshape(-1, hidden.shape[-1])[idx]
    yp = torch.from_numpy(np.asarray(y).reshape(-1)).long()[idx]
    yn = torch.from_numpy(np.asarray(neg).reshape(-1)).long()[idx]
    xp, xn = (h * table[yp]).sum(-1), (h * table[yn]).sum(-1)
    return bce_with_logits(xp, torch.ones_like(xp)).mean(), bce_with_logits(xn, torch.zeros_like(xn)).mean()


def batch_loss(params, seq, pos, y, neg, n_blocks, n_heads, reg, **drop):
    """the step's loss: both BCE means over pos != 0 plus reg * ||item_emb||_2 / rows"""
    hidden = forward(params, seq, pos, n_blocks, n_heads, **drop)
    lp, ln = bce_means(hidden, params['item_emb'], y, neg, np.asarray(pos) != 0)
    return lp + ln + reg * torch.linalg.norm(params['item_emb']) / params['item_emb'].shape[0]


def attn_keep_drawn(seed, counter, B, H, L, p):
    """(B, H, L, L) bool: the keep mask srh_seq_attn_fwd_f32 draws -- row (b, h, i) at counter + (b H + h) L + i, column
    j the word j % 4 of float4 j / 4, keep = u01(word) >= p"""
    ctr = counter_rng.counters(counter, B * H * L)
    nq = (L + 3) // 4
    w = counter_rng.rng4(ctr[:, None], np.arange(nq, dtype=np.uint32)[None, :], seed)        # (rows, nq, 4)
    keep = counter_rng.u01(w).reshape(B * H * L, 4 * nq)[:, :L] >= np.float32(p)
    return keep.reshape(B, H, L, L)
