"""SEPT's step in float64 numpy -- TEST INFRASTRUCTURE ONLY.  A line-by-line restatement of the reference's
model/graph/SEPT.py:48-64 (the encoders), 98-134 (label_prediction, top_k, neighbor_discrimination), 136-154 (the two
losses) and util/loss_tf.py bpr_loss, with the gradients derived by hand (the TF graph itself cannot run here);
tests/test_sept_cpu.py holds them to torch.autograd on the literal expression."""
import numpy as np

from tests import contrastive_ref

EPS = 1e-12                       # tf.nn.l2_normalize's epsilon, on the squared norm
PAIRS = ((1, 2), (0, 2), (0, 1))  # SEPT.py:145-147: friend <- (sharing, rec), sharing <- (friend, rec), rec <- (friend, sharing)


def l2norm(x):
    """tf.math.l2_normalize(x, axis=1): x * rsqrt(max(sum x^2, eps)) -> (out, inv, clamped)"""
    x = np.asarray(x, dtype=np.float64)
    ss = (x * x).sum(1)
    inv = 1.0 / np.sqrt(np.maximum(ss, EPS))
    return x * inv[:, None], inv, ss < EPS


def l2norm_bwd(g, out, inv, clamped):
    """d l2norm / dx applied to g: the maximum passes no gradient to the sum below eps, so a clamped row is g * 1e6"""
    g = np.asarray(g, dtype=np.float64)
    proj = (g - out * (out * g).sum(1, keepdims=True)) * inv[:, None]
    return np.where(clamped[:, None], g * inv[:, None], proj)


def topk_ids(key, k):
    """tf.math.top_k: value descending, ties to the lowest index"""
    return np.argsort(-key, axis=1, kind="stable")[:, :k]


def tri_nd(F, S, R, A, k, tau=0.1, loss_scale=1.0, pos=None):
    """label_prediction x 3 -> generate_pesudo_labels x 3 -> neighbor_discrimination x 3 and their gradients.
    pos (3, n, k), when given, replaces the top-k (the loss and gradients of that index set).
    -> dict: loss (3), grads (dF, dS, dR, dA), pos (3, n, k), key (3, n, n: the averaged softmax each top-k ranks),
             gap (3, n): (t_k - t_{k+1}) / t_k of every (pair, row), inf where n == k"""
    views = [np.asarray(x, dtype=np.float64) for x in (F, S, R)]
    n = views[0].shape[0]
    an, ainv, aclamp = l2norm(A)
    normed = [l2norm(v) for v in views]
    s = [vn @ an.T for vn, _, _ in normed]                             # SEPT.py:103
    prob = []
    for sv in s:
        e = np.exp(sv - sv.max(1, keepdims=True))
        prob.append(e / e.sum(1, keepdims=True))                       # SEPT.py:107
    key = np.stack([(prob[a] + prob[b]) / 2 for a, b in PAIRS])        # SEPT.py:114
    want = np.stack([topk_ids(key[v], k) for v in range(3)])
    srt = -np.sort(-key, axis=2)
    gap = (srt[:, :, k - 1] - srt[:, :, k]) / srt[:, :, k - 1] if n > k else np.full((3, n), np.inf)
    pos = want if pos is None else np.asarray(pos).astype(np.int64)
    loss, grads, gan = np.zeros(3), [], np.zeros_like(an)
    for v in range(3):
        vn, vinv, vclamp = normed[v]
        e = np.exp(s[v] / tau)                                         # SEPT.py:131-132
        member = np.zeros((n, n))
        np.put_along_axis(member, pos[v], 1.0, axis=1)
        ttl, ps = e.sum(1), (e * member).sum(1)
        loss[v] = loss_scale * -np.log(ps / ttl).sum()                 # SEPT.py:133
        ds = loss_scale / tau * (e / ttl[:, None] - member * e / ps[:, None])
        grads.append(l2norm_bwd(ds @ an, vn, vinv, vclamp))
        gan += ds.T @ vn
    grads.append(l2norm_bwd(gan, an, ainv, aclamp))
    return dict(loss=loss, grads=grads, pos=want, key=key, gap=gap)


def ambiguous(gap, bound=1e-4):
    return gap < bound


def row_errors(got, want, floor_frac=0.0):
    """contrastive_ref.row_errors as a float64 numpy (n,): per row max|got - want| / max(max|want_row|, floor_frac *
    max|want|); no floor unless one is asked for"""
    return contrastive_ref.row_errors(np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64),
                                      floor_frac).numpy()


def tri_nd_f32(F, S, R, A, k, tau, pos):
    """tri_nd's own expression at the given ids in plain float32 numpy -- a YARDSTICK, not a second reference: how far
    float32 arithmetic alone moves each loss and each gradient row of an input.  Normalise, exp((s - 1) / tau), the two
    sums, ds, the two products, the normalisation backward; every array float32, numpy's own summation order.
    -> dict: loss (3, float32), grads (dF, dS, dR, dA float32)"""
    f32 = np.float32
    one, eps, inv_tau = f32(1.0), f32(EPS), f32(1.0) / f32(tau)

    def norm(x):
        x = np.asarray(x, dtype=f32)
        ss = (x * x).sum(1, dtype=f32)
        clamped = ss < eps
        inv = np.where(clamped, f32(1e6), one / np.sqrt(np.maximum(ss, eps))).astype(f32)
        return x * inv[:, None], inv, clamped

    def norm_bwd(g, out, inv, clamped):
        proj = (g - out * (out * g).sum(1, keepdims=True, dtype=f32)) * inv[:, None]
        return np.where(clamped[:, None], g * inv[:, None], proj).astype(f32)

    an, ainv, aclamp = norm(A)
    n = an.shape[0]
    pos = np.asarray(pos).astype(np.int64)
    loss, grads, gan = np.zeros(3, dtype=f32), [], np.zeros_like(an)
    for v, V in enumerate((F, S, R)):
        vn, vinv, vclamp = norm(V)
        e = np.exp((vn @ an.T - one) * inv_tau)
        member = np.zeros((n, n), dtype=f32)
        np.put_along_axis(member, pos[v], one, axis=1)
        ttl, ps = e.sum(1, dtype=f32), (e * member).sum(1, dtype=f32)
        loss[v] = -np.log(ps / ttl).sum(dtype=f32)
        ds = inv_tau * (e / ttl[:, None] - member * e / ps[:, None])
        grads.append(norm_bwd(ds @ an, vn, vinv, vclamp))
        gan += ds.T @ vn
    grads.append(norm_bwd(gan, an, ainv, aclamp))
    assert all(g.dtype == f32 for g in grads)
    return dict(loss=loss, grads=grads)


def encoder(emb, adj, n_layers):
    """SEPT.py:48-64: the SUM of the raw table and the normalised layers -> (sum, cache for encoder_bwd)"""
    emb = np.asarray(emb, dtype=np.float64)
    total, cache = emb.copy(), []
    for _ in range(n_layers):
        out, inv, clamped = l2norm(adj @ emb)
        cache.append((out, inv, clamped))
        total = total + out
        emb = out
    return total, cache


def encoder_bwd(g, adj, cache):
    """gradient of the encoder's input table from the gradient g of its sum"""
    g = np.asarray(g, dtype=np.float64)
    acc = g.copy()                       # gradient reaching the deepest layer's output
    for out, inv, clamped in reversed(cache):
        acc = g + adj.T @ l2norm_bwd(acc, out, inv, clamped)
    return acc


def bpr_loss(u, p, q):
    """util/loss_tf.py:4-7 -> (loss, du, dp, dq)"""
    score = (u * p).sum(1) - (u * q).sum(1)
    sig = 1.0 / (1.0 + np.exp(-score))
    loss = -np.log(sig + 10e-8).sum()
    dscore = -(sig * (1.0 - sig)) / (sig + 10e-8)
    return loss, dscore[:, None] * (p - q), dscore[:, None] * u, -dscore[:, None] * u


def unique_first(ids):
    ids = np.asarray(ids).reshape(-1)
    _, first = np.unique(ids, return_index=True)
    return ids[np.sort(first)]


def step(user_emb, item_emb, norm_adj, sub_adj, friend_adj, sharing_adj, u_idx, i_idx, j_idx, *, n_layers, reg, ss_rate, k,
         joint=True, pos=None):
    """One batch of SEPT.train(): rec_loss (SEPT.py:138-139), neighbor_dis_loss (149-151) and the gradients of
    rec_loss + ss_rate * neighbor_dis_loss (joint) or of rec_loss alone with respect to both tables.
    The adjacencies are scipy matrices (any dtype: they are applied in float64)."""
    U = np.asarray(user_emb, dtype=np.float64)
    I = np.asarray(item_emb, dtype=np.float64)
    nu = U.shape[0]
    adj, sub, fr, sh = (m.astype(np.float64).tocsr() for m in (norm_adj, sub_adj, friend_adj, sharing_adj))
    ego = np.concatenate([U, I])
    rec, rec_cache = encoder(ego, adj, n_layers)
    u_idx, i_idx, j_idx = (np.asarray(x).astype(np.int64) for x in (u_idx, i_idx, j_idx))
    bu, bp, bq = rec[u_idx], rec[nu + i_idx], rec[nu + j_idx]
    bpr, du, dp, dq = bpr_loss(bu, bp, bq)
    rec_loss = bpr + reg * ((U * U).sum() / 2 + (I * I).sum() / 2)
    g_rec = np.zeros_like(rec)
    np.add.at(g_rec, u_idx, du)
    np.add.at(g_rec, nu + i_idx, dp)
    np.add.at(g_rec, nu + j_idx, dq)
    g_ego = reg * ego
    out = dict(rec_loss=rec_loss, nd_loss=0.0, pos=None)
    if joint:
        aug, aug_cache = encoder(ego, sub, n_layers)
        fv, f_cache = encoder(U, fr, n_layers)
        sv, s_cache = encoder(U, sh, n_layers)
        uq = unique_first(u_idx)
        nd = tri_nd(fv[uq], sv[uq], rec[uq], aug[uq], k, pos=pos)
        out.update(nd_loss=nd["loss"].sum(), pos=nd["pos"], uniq=uq, nd=nd)
        gf, gs, gr, ga = (ss_rate * g for g in nd["grads"])
        g_rec[uq] += gr
        g_aug = np.zeros_like(aug)
        g_aug[uq] = ga
        g_f, g_s = np.zeros_like(fv), np.zeros_like(sv)
        g_f[uq], g_s[uq] = gf, gs
        g_ego = g_ego + encoder_bwd(g_aug, sub, aug_cache)
        g_ego[:nu] += encoder_bwd(g_f, fr, f_cache) + encoder_bwd(g_s, sh, s_cache)
    g_ego = g_ego + encoder_bwd(g_rec, adj, rec_cache)
    out.update(g_user=g_ego[:nu], g_item=g_ego[nu:], rec_user=rec[:nu], rec_item=rec[nu:])
    return out
