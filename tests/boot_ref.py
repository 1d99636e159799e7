"""References for the bootstrap loss kernels (csrc/bootstrap.hip, include/selfrec_hip.h (a-23)) -- TEST
INFRASTRUCTURE ONLY, written from the header's contract and never imported by the product; no GPU needed.

    reference      the reference's own expressions with autograd, one per model form -- 'buir' (model/graph/BUIR.py:87-95:
                   F.linear, F.normalize, 2 - 2 * sum) and 'selfcf' (model/graph/SelfCF.py:64-91: the momentum mix under
                   no_grad, the history index-assign, F.cosine_similarity with .detach()) -- float64 by default
                   (dtype=torch.float32 gives the same expression in plain f32: the floor's yardstick)
    closed_form    the header's formulas in float64, with dP and the weight-gradient scales S
    grad_errors    per row: the error over the larger of the row's own largest |want| and FLOOR_FRAC times the median
                   row's; the clamped rows are a group of their own, a cancelling row is measured against cancel_scales
    cancel_scales  the size of what cancels in a row whose p is parallel to its t
    momentum_rows  rows_momentum's expression restated in numpy float32

A case (tests/boot_cases.py) is a dict: form, m, x_u, x_i, W, b, T_u, T_i, idx_u, idx_i (None: the targets are one row per
slot), store (bool: the tables also receive x at idx), cancel_u / cancel_i (bool masks or None)."""
import numpy as np
import torch
import torch.nn.functional as F

LOSS_TOL = 1e-5      # |value - ref| <= LOSS_TOL * max(1, |ref|) for the loss and each part
GRAD_TOL = 1e-4      # d_gx against float64 per row through grad_errors; d_gw, d_gb per element against GRAD_TOL * S
# the smallest of FLOORS at which the reference's own expression in plain float32 torch on the CPU stays within
# GRAD_TOL / 2 per row on every case (test_boot_ref_cpu.py::test_floor_frac_is_the_smallest_that_float32_torch_meets)
FLOORS = (1e-3, 1e-2, 1e-1, 1.0)
FLOOR_FRAC = 1e-3
SIDES = ("u", "i")


def cosine(c):
    """the clamp flag of a case's form: SelfCF's loss is F.cosine_similarity"""
    return c["form"] == "selfcf"


def scalars(c):
    """(alpha, beta, eps, c0, c1) of a case's form"""
    if c["form"] == "buir":
        return 1.0, 0.0, 1e-12, 4.0, 2.0
    return c["m"], 1.0 - c["m"], 1e-8, 1.0, 0.5


def gather(T, idx, n):
    """T[idx] with a zero row for an id outside the table; idx None: T itself (one row per slot)"""
    if idx is None:
        return T
    idx = idx.to(T.device).long()
    ok = (idx >= 0) & (idx < len(T))
    return T[idx.clamp(0, len(T) - 1)] * ok[:, None].to(T.dtype)


def scatter(T, idx, x):
    """T[idx] = x on a copy, ids outside the table skipped (duplicates carry equal rows: any order)"""
    T = T.clone()
    idx = idx.to(T.device).long()
    ok = (idx >= 0) & (idx < len(T))
    T[idx[ok]] = x[ok]
    return T


def _cast(c, dtype, device):
    dev = device or c["x_u"].device
    return {k: c[k].detach().to(device=dev, dtype=dtype) for k in ("x_u", "x_i", "W", "b", "T_u", "T_i")}


# ---- the reference's expressions ------------------------------------------------------------------------------------
def reference(c, dtype=torch.float64, device=None):
    """dict(loss, parts (2,), gx_u, gx_i, gw, gb, T_u, T_i (the tables after the call)) by autograd on the model's
    expression.  Every target is gathered from the tables as they were BEFORE the stores of the same call."""
    t = _cast(c, dtype, device)
    x_u, x_i, W, b = (t[k].requires_grad_(True) for k in ("x_u", "x_i", "W", "b"))
    n = len(x_u)
    his = {"u": t["T_u"], "i": t["T_i"]}
    idx = {"u": c["idx_u"], "i": c["idx_i"]}
    now = {"u": x_u, "i": x_i}
    if c["form"] == "buir":
        u_tg, i_tg = gather(his["u"], idx["u"], n), gather(his["i"], idx["i"], n)
        p_u, t_u, p_i, t_i = (F.normalize(v, dim=-1) for v in (F.linear(x_u, W, b), u_tg, F.linear(x_i, W, b), i_tg))
        cu, ci = (p_u * t_i).sum(-1), (p_i * t_u).sum(-1)
        loss = ((2 - 2 * cu) + (2 - 2 * ci)).mean()
    else:
        m = c["m"]
        with torch.no_grad():
            u_target = gather(his["u"], idx["u"], n) * m + x_u.data * (1. - m)
            i_target = gather(his["i"], idx["i"], n) * m + x_i.data * (1. - m)
        p_u, p_i = F.linear(x_u, W, b), F.linear(x_i, W, b)
        cu = F.cosine_similarity(p_u, i_target.detach(), dim=-1)
        ci = F.cosine_similarity(p_i, u_target.detach(), dim=-1)
        loss = (1 - cu.mean()) / 2 + (1 - ci.mean()) / 2
    loss.backward()
    after = {}
    for s in SIDES:
        after[s] = his[s]
        if c["store"]:
            with torch.no_grad():
                after[s] = scatter(his[s], idx[s], now[s].data) if idx[s] is not None else now[s].data.clone()
    return dict(loss=loss.detach(), parts=torch.stack([cu.detach().mean(), ci.detach().mean()]), gx_u=x_u.grad, gx_i=x_i.grad,
                gw=W.grad, gb=b.grad, T_u=after["u"], T_i=after["i"])


# ---- the closed form ------------------------------------------------------------------------------------------------
def closed_form(c, device=None):
    """reference()'s results from the header's formulas in float64, plus per side dP, |p|, |t| and the clamped flags, and
    S_w, S_b: the sums over both sides' rows of |dP_r[j]| |x_r[k]| and of |dP_r[j]|"""
    t = _cast(c, torch.float64, device)
    alpha, beta, eps, c0, c1 = scalars(c)
    x = {"u": t["x_u"], "i": t["x_i"]}
    W, b = t["W"], t["b"]
    n = len(x["u"])
    tgt = {s: alpha * gather(t["T_" + s], c["idx_" + s], n) + beta * x[s] for s in SIDES}
    out = dict(S_w=0.0, S_b=0.0, gw=0.0, gb=0.0)
    parts = []
    for s, o in (("u", "i"), ("i", "u")):
        p = x[s] @ W.T + b
        np_, nt = p.norm(dim=1), tgt[o].norm(dim=1)
        ph, th = p / np_.clamp_min(eps)[:, None], tgt[o] / nt.clamp_min(eps)[:, None]
        cos = (ph * th).sum(1)
        clamped = np_ < eps
        unit = p / np_.clamp_min(1e-300)[:, None]             # p / |p|, 0 at p = 0
        proj = th - cos[:, None] * unit
        # a clamped row: th / eps through F.normalize; F.cosine_similarity clamps outside the graph and keeps the projection
        kept = proj if c["form"] == "selfcf" else torch.where(clamped[:, None], th, proj)
        dp = -(c1 / n) * kept / np_.clamp_min(eps)[:, None]
        parts.append(cos.mean())
        out.update({"dp_" + s: dp, "np_" + s: np_, "nt_" + s: nt, "clamped_" + s: clamped, "th_" + s: th, "gx_" + s: dp @ W})
        out["gw"] = out["gw"] + dp.T @ x[s]
        out["gb"] = out["gb"] + dp.sum(0)
        out["S_w"] = out["S_w"] + dp.abs().T @ x[s].abs()
        out["S_b"] = out["S_b"] + dp.abs().sum(0)
    out["parts"] = torch.stack(parts)
    out["loss"] = c0 - c1 * (parts[0] + parts[1])
    for s in SIDES:
        idx = c["idx_" + s]
        out["T_" + s] = t["T_" + s] if not c["store"] else (scatter(t["T_" + s], idx, x[s]) if idx is not None else x[s].clone())
    return out


def cancel_scales(c, side, cf=None):
    """per row of side's gx: (c1 / B) / max(|p|, eps) * max_k (|th| |W|)[k] -- the size of th and of (ph . th) ph, whose
    difference is (nearly) zero on a row with p parallel or antiparallel to t.  float32 leaves about 1e-7 of it."""
    cf = cf or closed_form(c)
    _, _, eps, _, c1 = scalars(c)
    n = len(c["x_u"])
    w_abs = c["W"].detach().double().abs().to(cf["th_" + side].device)
    return (c1 / n) / cf["np_" + side].clamp_min(eps) * (cf["th_" + side].abs() @ w_abs).amax(1)


# ---- the error measures ---------------------------------------------------------------------------------------------
def grad_errors(got, want, clamped, cancel=None, scales=None, floor_frac=FLOOR_FRAC):
    """per row, float64 (n,): max|got - want| over max(max|want_row|, floor_frac * the MEDIAN row magnitude of the row's
    group) -- the clamped rows (gradients 1 / eps times the others') and the ordinary rows are each a group; a row of
    `cancel` is measured against scales[row] instead"""
    got = torch.as_tensor(got).detach().double().cpu()
    want = torch.as_tensor(want).detach().double().cpu()
    clamped = torch.as_tensor(clamped).cpu()
    err = (got - want).abs().amax(1)
    mag = want.abs().amax(1)
    den = torch.zeros_like(mag)
    for grp in (clamped, ~clamped):
        if grp.any():
            den[grp] = torch.clamp(mag[grp], min=floor_frac * float(mag[grp].median()))
    if cancel is not None and cancel.any():
        cancel = cancel.cpu()
        den[cancel] = torch.as_tensor(scales).double().cpu()[cancel]
    out = err / den
    out[(den == 0) & (err == 0)] = 0.0
    return out


def weight_errors(got_w, got_b, cf):
    """the worst element of d_gw and of d_gb as a fraction of its scale S (0 / 0 counts as 0)"""
    def frac(got, want, s):
        e = (torch.as_tensor(got).detach().double().cpu() - want.cpu()).abs()
        s = s.cpu()
        f = e / s
        f[(s == 0) & (e == 0)] = 0.0
        return float(f.max())
    return frac(got_w, cf["gw"], cf["S_w"]), frac(got_b, cf["gb"], cf["S_b"])


def value_error(got, want):
    """|got - want| over max(1, |want|)"""
    return abs(float(got) - float(want)) / max(1.0, abs(float(want)))


# ---- rows_momentum ----------------------------------------------------------------------------------------------------
def momentum_rows(tgt, src, idx, m):
    """tgt after tgt[idx] = tgt[idx] * m + src[idx] * (1 - m) in numpy float32: two rounded products, one rounded sum, from
    the values tgt held before; ids outside the table skipped"""
    tgt, src, idx = (torch.as_tensor(a).cpu().numpy() for a in (tgt, src, idx))
    tgt, src, idx = tgt.astype(np.float32), src.astype(np.float32), idx.astype(np.int64)      # (astype copies)
    ok = idx[(idx >= 0) & (idx < len(tgt))]
    new = tgt[ok] * np.float32(m) + src[ok] * np.float32(1 - m)
    tgt[ok] = new
    return tgt
