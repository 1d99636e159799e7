"""float64 restatement shared by the two flavours of the sequence attention kernels (causal: SASRec, CL4SRec; full:
BERT4Rec) and the edge cases tests/test_gpu_seq_edges.py holds them to -- TEST INFRASTRUCTURE ONLY (the product never
imports it).

``attention`` and ``attn_keep_drawn`` stay where they are (tests/sasrec_ref.py, tests/bert4rec_ref.py); this module adds the
rows' log-sum-exp, one ``reference`` that returns all five tensors a forward / backward pair produces, and the seeded
inputs of the edge cases, so that tests/test_sasrec_cpu.py can check their premises without a GPU."""
import functools
import math

import numpy as np
import torch

from tests import bert4rec_ref, sasrec_ref

DROP_P = 0.2
SEED = 0xA5C3_19E7_5DEE_CE66                  # bits above 32 set: both halves of the seed reach the key
COUNTER = 2 ** 32 - 5                         # rows 5 .. of a call sit past the 32-bit carry of the counter
FLAVOURS = ("causal", "full")

EDGE_L = (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)      # either side of every 16-row tile edge
EDGE_HEADS = ((1, 32), (1, 64), (2, 64), (3, 32), (4, 32))      # (H, dh): the envelope H dh <= 128 from corner to corner


def drawn_shapes(flavour):
    """(B, L, H, dh): every L of EDGE_L once, the head layouts in turn (the full flavour starts two further on, so the two
    flavours pair each L with different heads), B = 3, 2, 3, ...  Each layout meets two or more L, one of them off the tile."""
    shift = 0 if flavour == "causal" else 2
    return [((3, 2)[i % 2], L) + EDGE_HEADS[(i + shift) % len(EDGE_HEADS)] for i, L in enumerate(EDGE_L)]


def scores(q, k, n_heads, causal):
    """(B, H, L, L) float64 logits q_i . k_j / sqrt(dh), -inf where the query does not see the key"""
    B, L, E = q.shape
    dh = E // n_heads
    qh, kh = (t.double().reshape(B, L, n_heads, dh).permute(0, 2, 1, 3) for t in (q, k))
    s = qh @ kh.transpose(2, 3) / math.sqrt(dh)
    if causal:
        s = s.masked_fill(~torch.ones(L, L, dtype=torch.bool).tril(), float('-inf'))
    return s


def lse(q, k, n_heads, causal):
    """(B, H, L) float64: log sum_j exp(s_ij) over the keys row i sees -- the kernels' d_lse"""
    return torch.logsumexp(scores(q, k, n_heads, causal), dim=-1)


def attention(q, k, v, n_heads, causal, keep=None, drop_p=0.0):
    """the restatement of the flavour: tests/sasrec_ref.attention or tests/bert4rec_ref.attention, untouched"""
    return (sasrec_ref if causal else bert4rec_ref).attention(q, k, v, n_heads, keep, drop_p)


def keep_drawn(causal, seed, counter, B, H, L, p):
    return (sasrec_ref if causal else bert4rec_ref).attn_keep_drawn(seed, counter, B, H, L, p)


def reference(q, k, v, go, n_heads, causal, keep=None, drop_p=0.0):
    """float64 out, lse, gq, gk, gv of one forward / backward pair (inputs of any float type, on the host)"""
    q64, k64, v64 = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    out = attention(q64, k64, v64, n_heads, causal, keep, drop_p)
    out.backward(go.double())
    return dict(out=out.detach(), lse=lse(q, k, n_heads, causal), gq=q64.grad, gk=k64.grad, gv=v64.grad)


def general_inputs(shape, salt):
    """q = 8 randn, k = v = go = randn (B, L, H dh) float32: the inputs of the attn_case of the two GPU test files"""
    B, L, H, dh = shape
    g = torch.Generator().manual_seed(salt + 1000 * B + 10 * L + 7 * H + dh)
    q = 8.0 * torch.randn(B, L, H * dh, generator=g)
    k, v, go = (torch.randn(B, L, H * dh, generator=g) for _ in range(3))
    return q, k, v, go


@functools.lru_cache(maxsize=None)
def drawn_case(flavour, shape):
    """general inputs and, for two consecutive calls (counters COUNTER and COUNTER + B H L), the host's drawn keep mask and
    the float64 tensors under it"""
    B, L, H, dh = shape
    causal = flavour == "causal"
    q, k, v, go = general_inputs(shape, 30000 if causal else 40000)
    calls = []
    for n in range(2):
        ctr = COUNTER + n * B * H * L
        keep = keep_drawn(causal, SEED, ctr, B, H, L, DROP_P)
        calls.append(dict(counter=ctr, keep=keep, ref=reference(q, k, v, go, H, causal, keep, DROP_P)))
    return dict(q=q, k=k, v=v, go=go, calls=calls)


KEEP_EDGE_SHAPES = [(2, 17, 2, 32), (2, 49, 3, 32)]


@functools.lru_cache(maxsize=None)
def keep_edge_case(flavour, shape):
    """a random keep mask in which query row ``row`` (the first of the last tile) keeps nothing and key column ``col`` is
    kept by nobody, in every (sequence, head)"""
    B, L, H, dh = shape
    causal = flavour == "causal"
    q, k, v, go = general_inputs(shape, 50000 if causal else 60000)
    g = torch.Generator().manual_seed(L)
    keep = (torch.rand(B, H, L, L, generator=g) >= DROP_P).numpy()
    row, col = 16 * ((L - 1) // 16), 3 if L < 32 else 16
    keep[:, :, row, :] = False
    keep[:, :, :, col] = False
    return dict(q=q, k=k, v=v, go=go, keep=keep, row=row, col=col, ref=reference(q, k, v, go, H, causal, keep, DROP_P))


RANGE_SHAPE = (2, 33, 2, 64)
RANGE_SCALE = 100.0


@functools.lru_cache(maxsize=None)
def range_case(flavour):
    """even query rows 100 randn (logits of standard deviation ~100: an exp without the row maximum taken off overflows
    float32 at 88.7), odd rows 8 randn as everywhere else"""
    B, L, H, dh = RANGE_SHAPE
    causal = flavour == "causal"
    q, k, v, go = general_inputs(RANGE_SHAPE, 70000 if causal else 80000)
    q = q.clone()
    q[:, 0::2] *= RANGE_SCALE / 8.0
    ref = reference(q, k, v, go, H, causal)
    # what the ordinary (odd) rows alone contribute: dS of a row is linear in its row of go, so with the even rows of go
    # zeroed only the odd rows reach gq and gk
    odd_go = go.clone()
    odd_go[:, 0::2] = 0.0
    ordinary = reference(q, k, v, odd_go, H, causal)
    s = scores(q, k, H, causal)
    return dict(q=q, k=k, v=v, go=go, ref=ref, ordinary=ordinary,
                logit_std_even=float(s[:, :, 2::2][torch.isfinite(s[:, :, 2::2])].std()),
                logit_max=float(s[torch.isfinite(s)].abs().max()))


# ---- the BCE kernel's widths and row counts -------------------------------------------------------------------------------
BCE_EDGE_CASES = ([(R, d) for d in (1, 4, 48, 63, 65, 100, 128, 200, 1024) for R in (3, 5)]
                  + [(R, 64) for R in (255, 257, 1023)])
BCE_N_ITEMS = 40


def bce_reference(hidden, table, pos, neg, usable):
    """float64 (lp, ln, gh (R x d), grows (2R x d), gt (n x d)) of the two BCE means over the usable rows"""
    h64, t64 = hidden.double().requires_grad_(True), table.double().requires_grad_(True)
    p = np.where(usable, pos, 0)
    n = np.where(usable, neg, 0)
    # the gathered rows as leaves of their own: their gradients are the kernel's per-row table gradients
    tp, tn = t64[torch.from_numpy(p).long()], t64[torch.from_numpy(n).long()]
    tp.retain_grad()
    tn.retain_grad()
    idx = torch.from_numpy(np.flatnonzero(usable))
    xp, xn = (h64 * tp).sum(-1)[idx], (h64 * tn).sum(-1)[idx]
    lp = sasrec_ref.bce_with_logits(xp, torch.ones_like(xp)).mean()
    ln = sasrec_ref.bce_with_logits(xn, torch.zeros_like(xn)).mean()
    (lp + ln).backward()
    return dict(lp=float(lp.detach()), ln=float(ln.detach()), gh=h64.grad, grows=torch.cat([tp.grad, tn.grad]), gt=t64.grad,
                xp=xp.detach(), xn=xn.detach())


@functools.lru_cache(maxsize=None)
def bce_edge_case(R, d):
    """hidden = (24 / sqrt(d)) randn against a randn table: logits of standard deviation ~24 at every width, both tails of
    the loss; every third row from row 1 invalid where there are rows to spare"""
    g = torch.Generator().manual_seed(9000 + 17 * R + d)
    table = torch.randn(BCE_N_ITEMS, d, generator=g)
    hidden = (24.0 / math.sqrt(d)) * torch.randn(R, d, generator=g)
    pos = torch.randint(0, BCE_N_ITEMS, (R,), generator=g)
    neg = torch.randint(0, BCE_N_ITEMS, (R,), generator=g)
    valid = torch.ones(R, dtype=torch.bool)
    valid[torch.arange(R) % 3 == 1] = False
    ref = bce_reference(hidden, table, pos.numpy(), neg.numpy(), valid.numpy())
    ref_logits = torch.cat([ref["xp"], ref["xn"]])
    return dict(table=table, hidden=hidden, pos=pos, neg=neg, valid=valid, span=float(ref_logits.abs().max()), **ref)


BCE_BAD_IDS = (("pos", -1), ("pos", BCE_N_ITEMS), ("neg", 2 ** 31 - 1), ("neg", -7))


@functools.lru_cache(maxsize=None)
def bce_bad_id_case():
    """13 rows of 65 columns; rows 2, 5, 8 and 11 are marked valid but name an item outside [0, n_table) -- one of BCE_BAD_IDS
    each --, rows 1 and 7 are marked invalid: 7 usable rows"""
    R, d = 13, 65
    g = torch.Generator().manual_seed(4242)
    table = torch.randn(BCE_N_ITEMS, d, generator=g)
    hidden = (24.0 / math.sqrt(d)) * torch.randn(R, d, generator=g)
    pos = torch.randint(0, BCE_N_ITEMS, (R,), generator=g)
    neg = torch.randint(0, BCE_N_ITEMS, (R,), generator=g)
    valid = torch.ones(R, dtype=torch.bool)
    valid[[1, 7]] = False
    bad_rows = [2, 5, 8, 11]
    for r, (which, value) in zip(bad_rows, BCE_BAD_IDS):
        (pos if which == "pos" else neg)[r] = value
    usable = valid.numpy().copy()
    usable[bad_rows] = False
    ref = bce_reference(hidden, table, pos.numpy(), neg.numpy(), usable)
    return dict(table=table, hidden=hidden, pos=pos, neg=neg, valid=valid, usable=torch.from_numpy(usable), bad_rows=bad_rows,
                **ref)
