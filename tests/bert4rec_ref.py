"""float64 torch restatement of BERT4Rec -- TEST INFRASTRUCTURE ONLY (the product never imports it).

Written from the model's semantics, not from the reference's file: ``params`` is a dict of float64
tensors under the reference's state_dict names.  Dropout on the attention probabilities takes an INJECTED keep mask
(1 = keep), scaled by 1 / (1 - p).  tests/test_bert4rec_cpu.py pins it to the reference-run golden."""
import math

import numpy as np
import torch

from tests import counter_rng
from tests.sasrec_ref import layer_norm


def attention(q, k, v, n_heads, keep=None, drop_p=0.0):
    """attention of projected (B, L, H dh) tensors with NO mask: every query sees all L keys; keep: (B, H, L, L) or None"""
    B, L, E = q.shape
    dh = E // n_heads
    out = torch.zeros_like(q)
    for h in range(n_heads):
        c = slice(h * dh, (h + 1) * dh)
        p = torch.softmax(torch.einsum('bid,bjd->bij', q[..., c], k[..., c]) / math.sqrt(dh), dim=-1)
        if keep is not None:
            p = p * torch.as_tensor(keep)[:, h].to(p.dtype) / (1.0 - drop_p)
        out[..., c] = torch.einsum('bij,bjd->bid', p, v[..., c])
    return out


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def forward(params, seq, pos, n_blocks, n_heads, drop_p=0.0, attn_keep=None):
    """(B, L, d) hidden states: n = LN_a(x); attention(query n, key = value = x), no mask; x = LN_f(n + attn);
    x = x + W2 gelu(W1 x + b1) + b2; rows with seq == 0 zeroed after the embedding mix and after every block; a last LN"""
    seq, pos = np.asarray(seq), np.asarray(pos)
    d = params['item_emb'].shape[1]
    x = params['item_emb'][torch.from_numpy(seq).long()] * d ** 0.5 + params['pos_emb'][torch.from_numpy(pos).long()]
    live = torch.from_numpy(seq != 0).unsqueeze(-1).to(x.dtype)
    x = x * live
    for i in range(n_blocks):
        n = layer_norm(x, params[f'attention_layer_norms.{i}.weight'], params[f'attention_layer_norms.{i}.bias'])
        w, b = params[f'attention_layers.{i}.in_proj_weight'], params[f'attention_layers.{i}.in_proj_bias']
        q = n @ w[:d].T + b[:d]
        k = x @ w[d:2 * d].T + b[d:2 * d]
        v = x @ w[2 * d:].T + b[2 * d:]
        a = attention(q, k, v, n_heads, None if attn_keep is None else attn_keep[i], drop_p)
        a = a @ params[f'attention_layers.{i}.out_proj.weight'].T + params[f'attention_layers.{i}.out_proj.bias']
        x = layer_norm(n + a, params[f'forward_layer_norms.{i}.weight'], params[f'forward_layer_norms.{i}.bias'])
        hdn = gelu(x @ params[f'forward_layers.{i}.pwff.0.weight'].T + params[f'forward_layers.{i}.pwff.0.bias'])
        x = (hdn @ params[f'forward_layers.{i}.pwff.2.weight'].T + params[f'forward_layers.{i}.pwff.2.bias'] + x) * live
    return layer_norm(x, params['last_layer_norm.weight'], params['last_layer_norm.bias'])


def table_ce(h, table, labels, loss_scale=1.0):
    """loss_scale * sum_m (lse_m - s_{m, label_m}), s = h @ table.T; max-subtracted by hand"""
    s = h @ table.T
    mx = s.max(dim=1, keepdim=True).values
    lse = mx.squeeze(1) + torch.log(torch.exp(s - mx).sum(dim=1))
    lab = torch.as_tensor(np.asarray(labels)).long()
    return loss_scale * (lse - s[torch.arange(s.shape[0]), lab]).sum()


def table_ce_grads(h, table, labels, loss_scale=1.0):
    """(loss, dL/dh, dL/dtable) in float64, the gradients in closed form: P - onehot against the other operand"""
    h, table = h.double(), table.double()
    s = h @ table.T
    p = torch.softmax(s, dim=1)
    lab = torch.as_tensor(np.asarray(labels)).long()
    p[torch.arange(s.shape[0]), lab] -= 1.0
    return float(table_ce(h, table, labels, loss_scale)), loss_scale * (p @ table), loss_scale * (p.T @ h)


def batch_loss(params, aug_seq, pos, masked, labels, n_blocks, n_heads, reg):
    """the step's loss: the cross-entropy mean over the M masked rows (ascending flat position, paired with the labels
    AS GIVEN), divided by M once more, plus reg * ||item_emb||_2 / rows"""
    hidden = forward(params, aug_seq, pos, n_blocks, n_heads)
    idx = torch.from_numpy(np.flatnonzero(np.asarray(masked).reshape(-1) > 0))
    rows = hidden.reshape(-1, hidden.shape[-1])[idx]
    M = rows.shape[0]
    ce = table_ce(rows, params['item_emb'], labels, 1.0 / (M * M))
    return ce + reg * torch.linalg.norm(params['item_emb']) / params['item_emb'].shape[0]


def attn_keep_drawn(seed, counter, B, H, L, p):
    """(B, H, L, L) bool: the keep mask srh_seq_attn_full_fwd_f32 draws over the FULL row -- row (b, h, i) at
    counter + (b H + h) L + i, column j the word j % 4 of float4 j / 4, keep = u01(word) >= p"""
    ctr = counter_rng.counters(counter, B * H * L)
    nq = (L + 3) // 4
    w = counter_rng.rng4(ctr[:, None], np.arange(nq, dtype=np.uint32)[None, :], seed)
    keep = counter_rng.u01(w).reshape(B * H * L, 4 * nq)[:, :L] >= np.float32(p)
    return keep.reshape(B, H, L, L)


# ---- the table-CE cases of the GPU tests (tests/test_bert4rec_cpu.py checks that float32 arithmetic alone meets the
# bounds on every one of them) ----------------------------------------------------------------------------------------
CE_SHAPES = [(1, 2, 64), (5, 83, 64), (93, 82, 64), (70, 1000, 128), (300, 5000, 64)]
CE_FAMILIES = ("ordinary", "extreme")


def ce_case(shape, family):
    """(h (M x d), table (N x d), labels (M,)) float32 / int64 on the host.  Labels repeat and include 0 and N - 1 (a single
    row carries N - 1).
    ordinary: rows of norm ~ sqrt(d), table entries ~ 0.05.
    extreme: column 0 of the table is 1 in every row and 2 in row 0, so a row of h with h[0] = +c has logits ~ c everywhere
      and 2c at key 0, and one with h[0] = -c has ALL its logits near -c.  Row 0 (c = 60: largest logit 120, where an
      unshifted float32 exp overflows) has the arg-max as its label (a single row: the label 60 below it); row 1 (-130) has
      every logit below -100, where an unshifted exp underflows to a zero row sum, and its label 0 at -260 far below its
      arg-max; rows 4 (+110) and 3 (-105) carry random labels."""
    M, N, d = shape
    g = torch.Generator().manual_seed(7000 + 131 * M + N + d + (1 if family == "extreme" else 0))
    h = torch.randn(M, d, generator=g)
    table = 0.05 * torch.randn(N, d, generator=g)
    labels = torch.randint(0, N, (M,), generator=g)
    labels[0] = 0
    labels[-1] = N - 1
    if M >= 5:
        labels[2] = labels[3]                     # a repeated label
        labels[1] = 0
    if family == "extreme":
        table[:, 0] = 1.0
        table[0, 0] = 2.0
        h[0, 0] = 60.0                            # logits ~ 60 everywhere, 120 at column 0: label 0 is the arg-max
        if M >= 2:
            h[1 % M, 0] = -130.0                  # logits ~ -130 everywhere, -260 at column 0: label 0 lies far below
        if M >= 5:
            h[4, 0] = 110.0
            h[3, 0] = -105.0
    return h, table, labels
