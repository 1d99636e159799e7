"""float64 numpy restatement of MixGCF's hop mixing -- TEST INFRASTRUCTURE ONLY.

Written from the contract of srh_mixup_fwd_f32 / srh_mixup_bwd_f32 in include/selfrec_hip.h; the product never imports
this module.  tables: (H, I, d); u: (B, d); pos: (B,); neg: (B * C,), pair b owning neg[b C .. b C + C - 1]; alpha:
(H, B, C, d) in [0, 1).  No index outside [0, I) is fed (the header's treatment of such indices is not restated)."""
import numpy as np

from tests import counter_rng


def f64(a):
    return np.asarray(a, dtype=np.float64)


def drawn_alpha(seed, counter, H, B, C, d):
    """the alpha a call draws in the kernel: row (k, b, c) at counter `counter` + (k B + b) C + c, float4 q with sub = q --
    i.e. counter_noise over H B C consecutive counters, reshaped"""
    return counter_rng.counter_noise(seed, counter, H * B * C, d).reshape(H, B, C, d)


def mixed(tables, pos, neg, alpha):
    """(H, B, C, d): m = alpha p + (1 - alpha) n, float64"""
    t, al = f64(tables), f64(alpha)
    H, B, C, d = al.shape
    p = t[:, np.asarray(pos)][:, :, None, :]                              # (H, B, 1, d)
    n = t[:, np.asarray(neg).reshape(B, C)]                               # (H, B, C, d)
    return al * p + (1.0 - al) * n


def scores(tables, u, pos, neg, alpha):
    """(H, B, C) float64 scores s_c = u_b . m_c of every candidate"""
    return np.einsum("bd,hbcd->hbc", f64(u), mixed(tables, pos, neg, alpha))


def argmax(s):
    """(H, B) the first maximum over c (numpy's argmax: the lowest index of an exact tie)"""
    return np.argmax(s, axis=2).astype(np.int32)


def margin(tables, u, pos, neg, alpha):
    """(H, B): what a float32 dot product of d terms (one rounding per mixed element, fma or not, plus the d - 1 additions
    in any order) may differ from the float64 score by: (d + 8) 2^-23 max_c sum_j |u_j| (|alpha p_j| + |(1 - alpha) n_j|)"""
    t, al = f64(tables), f64(alpha)
    H, B, C, d = al.shape
    p = np.abs(t[:, np.asarray(pos)][:, :, None, :])
    n = np.abs(t[:, np.asarray(neg).reshape(B, C)])
    mag = np.einsum("bd,hbcd->hbc", np.abs(f64(u)), al * p + (1.0 - al) * n)
    return (d + 8) * 2.0 ** -23 * mag.max(axis=2)


def outputs(tables, pos, neg, alpha, pick):
    """(pos_out, neg_out) for a GIVEN pick (H, B): the hop means of the positives' rows and of the picked mixtures"""
    t = f64(tables)
    m = mixed(tables, pos, neg, alpha)
    H, B = m.shape[:2]
    pick = np.asarray(pick).astype(np.int64)
    kept = m[np.arange(H)[:, None], np.arange(B)[None, :], pick]          # (H, B, d)
    return t[:, np.asarray(pos)].mean(axis=0), kept.mean(axis=0)


def grads(n_items, pos, neg, alpha, pick, g_pos, g_neg):
    """(H, I, d) float64 gradient tables for a GIVEN pick; g_pos / g_neg (B, d) or None (zero)"""
    al = f64(alpha)
    H, B, C, d = al.shape
    pos, negs, pick = np.asarray(pos), np.asarray(neg).reshape(B, C), np.asarray(pick).astype(np.int64)
    gp = np.zeros((B, d)) if g_pos is None else f64(g_pos)
    gn = np.zeros((B, d)) if g_neg is None else f64(g_neg)
    out = np.zeros((H, n_items, d))
    rows = np.arange(B)
    for k in range(H):
        a_star = al[k, rows, pick[k]]                                      # (B, d)
        np.add.at(out[k], pos, (gp + a_star * gn) / H)
        np.add.at(out[k], negs[rows, pick[k]], ((1.0 - a_star) * gn) / H)
    return out


def f32_scores(tables, u, pos, neg, alpha):
    """the same scores in plain float32 numpy (the yardstick: what float32 arithmetic loses on a case)"""
    t, al, uu = np.asarray(tables, np.float32), np.asarray(alpha, np.float32), np.asarray(u, np.float32)
    H, B, C, d = al.shape
    p = t[:, np.asarray(pos)][:, :, None, :]
    n = t[:, np.asarray(neg).reshape(B, C)]
    m = al * p + (np.float32(1.0) - al) * n
    return (uu[None, :, None, :] * m).sum(axis=3, dtype=np.float32), m
