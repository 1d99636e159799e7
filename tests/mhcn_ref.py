"""MHCN's step in float64 numpy -- TEST INFRASTRUCTURE ONLY.  A line-by-line restatement of the reference's
model/graph/MHCN.py:79-83 (the gates), 85-93 (channel_attention), 104-157 (the forward pass), 159-181
(hierarchical_self_supervision) and 184-189 (the loss), with the gradients derived by hand (the TF graph itself cannot run
here); tests/test_mhcn_cpu.py holds them to torch.autograd on the literal expression.  Every function takes ``dt``: float64
is the restatement, float32 the yardstick (the same lines in the precision of the kernels)."""
import numpy as np

from tests import sept_ref

F64 = np.float64


def sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1 / (1 + e), e / (1 + e)).astype(x.dtype)


def softplus(x):
    """log(1 + exp(x)) = -log(sigmoid(-x)), finite for every finite x"""
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))


# ---- the gates ---------------------------------------------------------------------------------------------------------
def gate(x, w, b, dt=F64):
    """y[c] = x * sigmoid(x @ w[c] + b[c])  ->  (y (C, n, d), s (C, n, d))"""
    x, w, b = (np.asarray(t, dtype=dt) for t in (x, w, b))
    s = np.stack([sigmoid(x @ w[c] + b[c][None, :]) for c in range(w.shape[0])]) if x.shape[0] else \
        np.zeros((w.shape[0],) + x.shape, dtype=dt)
    return x[None] * s, s


def gate_bwd(x, w, b, gy, dt=F64):
    """-> (dx, dw, db) with dz[c] = gy[c] * x * s[c] (1 - s[c])"""
    x, w, b, gy = (np.asarray(t, dtype=dt) for t in (x, w, b, gy))
    _, s = gate(x, w, b, dt)
    dz = gy * x[None] * (s * (1 - s))
    dx = (gy * s).sum(0) + sum(dz[c] @ w[c].T for c in range(w.shape[0]))
    dw = np.stack([x.T @ dz[c] for c in range(w.shape[0])])
    return dx, dw, dz.sum(1)


# ---- channel attention ---------------------------------------------------------------------------------------------------
def chan_mix(e, q, x=None, beta=0.0, dt=F64):
    """e: three (n, d) channels; w_c = e_c . q; s = softmax_c; out = sum_c s_c e_c + beta x  ->  (out, s (n, 3))"""
    e = [np.asarray(t, dtype=dt) for t in e]
    q = np.asarray(q, dtype=dt).reshape(-1)
    w = np.stack([t @ q for t in e], axis=1)
    ex = np.exp(w - w.max(1, keepdims=True)) if w.shape[0] else w
    s = ex / ex.sum(1, keepdims=True) if w.shape[0] else w
    out = sum(s[:, c:c + 1] * e[c] for c in range(3))
    if x is not None:
        out = out + dt(beta) * np.asarray(x, dtype=dt)
    return out, s


def chan_mix_bwd(e, q, s, gout, beta=0.0, dt=F64):
    """-> (de (3 x (n, d)), dx = beta gout, dq (d))"""
    e = [np.asarray(t, dtype=dt) for t in e]
    q, s, gout = np.asarray(q, dtype=dt).reshape(-1), np.asarray(s, dtype=dt), np.asarray(gout, dtype=dt)
    a = np.stack([(gout * t).sum(1) for t in e], axis=1)               # dL/ds_c
    dw = s * (a - (s * a).sum(1, keepdims=True))
    de = [s[:, c:c + 1] * gout + dw[:, c:c + 1] * q[None, :] for c in range(3)]
    dq = sum(dw[:, c] @ e[c] for c in range(3))
    return de, dt(beta) * gout, dq


# ---- hierarchical_self_supervision -------------------------------------------------------------------------------------------
def mim_scores(em, edge, perms, dt=F64):
    em, edge = np.asarray(em, dtype=dt), np.asarray(edge, dtype=dt)
    p1, p2, p3, c2, c3 = (np.asarray(p).astype(np.int64) for p in perms)
    n = em.shape[0]
    rcs2, rcs3 = edge[:, c2][p2], edge[:, c3][p3]
    g = edge.sum(0) / dt(n) if n else np.zeros(em.shape[1], dtype=dt)
    pos, n1, n2 = (em * edge).sum(1), (em[p1] * edge).sum(1), (rcs2 * em).sum(1)
    gp, gn = edge @ g, rcs3 @ g
    return dict(em=em, edge=edge, p=(p1, p2, p3), c=(c2, c3), rcs2=rcs2, rcs3=rcs3, g=g,
                x1=n1 - pos, x2=n2 - n1, x3=gn - gp)


def mim(em, edge, perms, loss_scale=1.0, dt=F64):
    """perms = (p1, p2, p3, c2, c3).  loss = scale * sum_r sp(n1 - pos) + sp(n2 - n1) + sp(gn - gp) and its gradients
    -> dict(loss, gem, gedge, x1, x2, x3)"""
    m = mim_scores(em, edge, perms, dt)
    em, edge, g = m["em"], m["edge"], m["g"]
    (p1, p2, p3), (c2, c3) = m["p"], m["c"]
    n = em.shape[0]
    loss = dt(loss_scale) * (softplus(m["x1"]).sum(dtype=F64) + softplus(m["x2"]).sum(dtype=F64) + softplus(m["x3"]).sum(dtype=F64))
    k1, k2, k3 = (dt(loss_scale) * sigmoid(m[k]) for k in ("x1", "x2", "x3"))
    gem = -k1[:, None] * edge + k2[:, None] * m["rcs2"]
    np.add.at(gem, p1, (k1 - k2)[:, None] * edge)
    gedge = -k1[:, None] * em + (k1 - k2)[:, None] * em[p1] - k3[:, None] * g[None, :]
    scat2, scat3 = np.zeros_like(edge), np.zeros_like(edge)
    np.add.at(scat2, p2, k2[:, None] * em)                            # rcs2[r][j] = edge[p2[r]][c2[j]]
    np.add.at(scat3, p3, k3[:, None] * g[None, :])
    gedge[:, c2] += scat2
    gedge[:, c3] += scat3
    if n:
        dg = (k3[:, None] * (m["rcs3"] - edge)).sum(0)
        gedge += dg[None, :] / dt(n)
    return dict(loss=loss, gem=gem, gedge=gedge, x1=m["x1"], x2=m["x2"], x3=m["x3"])


def mim_reference_form(em, edge, perms):
    """the reference's own lines, -log(sigmoid(x)), in float64 (inf where sigmoid underflows)"""
    m = mim_scores(em, edge, perms)
    with np.errstate(divide="ignore", over="ignore"):
        neglogsig = lambda x: -np.log(1.0 / (1.0 + np.exp(-x)))  # noqa: E731
        return neglogsig(-m["x1"]).sum() + neglogsig(-m["x2"]).sum() + neglogsig(-m["x3"]).sum()


# ---- the whole step ------------------------------------------------------------------------------------------------------------
WEIGHT_KEYS = tuple(f"{p}{i}" for i in range(1, 5) for p in ("gating", "gating_bias", "sgating", "sgating_bias")) + \
    ("attention", "attention_mat")


def step(params, H, R, u_idx, i_idx, j_idx, perms, n_layers, reg, ss_rate):
    """One batch of MHCN.train() in float64.  params: the reference's variables by name (user_embeddings, item_embeddings
    and WEIGHT_KEYS; biases and attention (1, d)); H: the three scipy motif matrices; R: the row-normalised interaction
    matrix (users x items); perms: per channel (p1, p2, p3, c2, c3).
    -> dict(rec_loss, reg_loss, ss_loss (ss_rate applied), loss, score (n x 3), user, item, grads {name: array})"""
    P = {k: np.asarray(v, dtype=F64) for k, v in params.items()}
    H = [h.tocsr().astype(F64) for h in H]
    R = R.tocsr().astype(F64)
    U, I0 = P["user_embeddings"], P["item_embeddings"]
    wg = np.stack([P[f"gating{i}"] for i in range(1, 5)])
    bg = np.concatenate([P[f"gating_bias{i}"] for i in range(1, 5)])
    ws = np.stack([P[f"sgating{i}"] for i in range(1, 4)])
    bs = np.concatenate([P[f"sgating_bias{i}"] for i in range(1, 4)])
    att, mat = P["attention"], P["attention_mat"]
    q = (mat @ att.T).reshape(-1)
    norm = sept_ref.l2norm

    y0, _ = gate(U, wg, bg)
    chans, simple, item = [y0[0], y0[1], y0[2]], y0[3], I0
    sums, simple_sum, item_sum = list(chans), simple, I0
    tape = []
    for _ in range(n_layers):
        mixed, score = chan_mix(chans, q, simple, 0.5)
        new_chans = [h @ c for h, c in zip(H, chans)]
        new_item, new_simple = R.T @ mixed, R @ item
        nc, ni, ns = [norm(c) for c in new_chans], norm(new_item), norm(new_simple)
        sums = [s + x[0] for s, x in zip(sums, nc)]
        item_sum, simple_sum = item_sum + ni[0], simple_sum + ns[0]
        tape.append(dict(chans=chans, score=score, nc=nc, ni=ni, ns=ns))
        chans, simple, item = new_chans, new_simple, new_item
    user, score = chan_mix(sums, q, simple_sum, 0.5)
    sg, _ = gate(user, ws, bs)

    grads = {k: reg * P[k] for k in WEIGHT_KEYS}
    g_user, g_item_sum = np.zeros_like(user), np.zeros_like(item_sum)
    # the self-supervised branch
    ss, g_sg = 0.0, []
    for ch in range(3):
        m = mim(sg[ch], H[ch] @ sg[ch], perms[ch], loss_scale=ss_rate)
        ss += m["loss"]
        g_sg.append(m["gem"] + H[ch].T @ m["gedge"])
    gx, gws, gbs = gate_bwd(user, ws, bs, np.stack(g_sg))
    g_user += gx
    for i in range(3):
        grads[f"sgating{i + 1}"] = grads[f"sgating{i + 1}"] + gws[i]
        grads[f"sgating_bias{i + 1}"] = grads[f"sgating_bias{i + 1}"] + gbs[i][None, :]
    # bpr_loss (util/loss_tf.py) and the batch rows' regulariser
    bu, bp, bn = user[u_idx], item_sum[i_idx], item_sum[j_idx]
    x = (bu * bp).sum(1) - (bu * bn).sum(1)
    sig = sigmoid(x)
    rec_loss = -np.log(sig + 10e-8).sum()
    ds = -(sig * (1 - sig)) / (sig + 10e-8)
    np.add.at(g_user, u_idx, ds[:, None] * (bp - bn) + reg * bu)
    np.add.at(g_item_sum, i_idx, ds[:, None] * bu + reg * bp)
    np.add.at(g_item_sum, j_idx, -ds[:, None] * bu + reg * bn)
    reg_loss = reg * (sum((P[k] ** 2).sum() / 2 for k in WEIGHT_KEYS) + ((bu ** 2).sum() + (bp ** 2).sum() + (bn ** 2).sum()) / 2)
    # the final mix, then the layers in reverse
    g_sums, g_simple_sum, gq = chan_mix_bwd(sums, q, score, g_user, 0.5)
    g_chans = [np.zeros_like(user) for _ in range(3)]
    g_simple, g_item = np.zeros_like(user), np.zeros_like(item_sum)
    bwd = lambda g, x: sept_ref.l2norm_bwd(g, *x)  # noqa: E731
    for t in reversed(tape):
        tot_c = [g_chans[i] + bwd(g_sums[i], t["nc"][i]) for i in range(3)]
        tot_i = g_item + bwd(g_item_sum, t["ni"])
        tot_s = g_simple + bwd(g_simple_sum, t["ns"])
        ge, gxs, gq_l = chan_mix_bwd(t["chans"], q, t["score"], R @ tot_i, 0.5)
        gq = gq + gq_l
        g_chans = [H[i].T @ tot_c[i] + ge[i] for i in range(3)]
        g_simple, g_item = gxs, R.T @ tot_s
    g_gates = np.stack([g_chans[i] + g_sums[i] for i in range(3)] + [g_simple + g_simple_sum])
    gU, gwg, gbg = gate_bwd(U, wg, bg, g_gates)
    for i in range(4):
        grads[f"gating{i + 1}"] = grads[f"gating{i + 1}"] + gwg[i]
        grads[f"gating_bias{i + 1}"] = grads[f"gating_bias{i + 1}"] + gbg[i][None, :]
    grads["attention_mat"] = grads["attention_mat"] + gq[:, None] * att
    grads["attention"] = grads["attention"] + (gq @ mat)[None, :]
    grads["user_embeddings"], grads["item_embeddings"] = gU, g_item + g_item_sum
    return dict(rec_loss=rec_loss, reg_loss=reg_loss, ss_loss=ss, loss=rec_loss + reg_loss + ss, score=score, user=user,
                item=item_sum, grads=grads)
