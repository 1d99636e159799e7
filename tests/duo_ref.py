"""Float64 restatement, seeded cases and measures of DuoRec's fused contrastive section (csrc/duo.hip,
ops.duo_nce_fwd_bwd) -- TEST INFRASTRUCTURE ONLY, no GPU needed.

    duo              the header's closed form in the dtype asked for: both losses, the compact G = [ga; gp; gq], both lse
                     vectors, the partner logits and the row terms
    duo_autograd     torch autograd of the reference's info_nce expression (util/loss_torch.py:54-88, as
                     selfrec_amd.util.loss_torch restates it for CPU tensors) called twice on shared anchors
    contested        randn d^(-1/4) rows, partners c a + sqrt(1 - c^2) noise with c = 0.3 (p) and 0.15 (q): every softmax
                     is contested, losses of the order of log 2B, measured relative to themselves
    peaked           the workload's regime: LayerNormed rows of norm sqrt(d), partners the LayerNorm of the row plus
                     noise 0.6 / 1.0; the positive wins by tens of nats and the losses are tiny, so nothing can be held
                     relative to itself (see the measures)

tests/test_duo_ref_cpu.py pins ``duo`` to ``duo_autograd`` in float64 and re-measures the float32 yardsticks;
tests/test_gpu_duo.py runs the kernel on the cases.  Builders are cached; their tensors are never written to."""
import functools

import torch

from tests.contrastive_ref import row_errors  # noqa: F401  (the per-row measure, re-exported)

LOSS_TOL = 1e-5        # losses, lse and row terms
GRAD_TOL = 1e-4        # gradient rows
FLOOR_FRAC = 1e-3      # contested: rows below this share of the largest row are measured against that floor

# 3B rows in tiles of 64: 21 | 22 (one tile, 63 | 66 rows), 43 (129 rows), 63 .. 65 (a block boundary inside, on and past a
# tile edge; at 64 a P row meets a tile of Q keys only), 129, 257 (several row tiles and workgroups)
CONTESTED_B = (2, 15, 16, 17, 21, 22, 43, 63, 64, 65, 129, 257)
PEAKED_B = (17, 64, 257)
WIDTHS = (64, 128)
CONTESTED_TEMPS = (1.0, 0.5)
CONTESTED_C = (0.3, 0.15)
PEAKED_NOISE = (0.6, 1.0)


def duo(za, zp, zq, inv_temp, scale_u=1.0, scale_s=1.0, dtype=torch.float64):
    """dict(losses (2,), g (3B x d), lse (2 x 3B, +inf where the row has no such softmax), pos (2 x 3B, NaN there),
    terms (2 x 3B, 0 there)) of header (a-25), every expression in ``dtype``"""
    A, P, Q = (torch.as_tensor(t).to(dtype) for t in (za, zp, zq))
    B = len(A)
    z = torch.cat((A, P, Q))
    n = 3 * B
    s = (z @ z.T) * inv_temp
    blk = torch.arange(n) // B
    b = torch.arange(n) % B
    g = torch.zeros_like(z)
    losses, lses, poss, terms = [], [], [], []
    for t, scale in enumerate((scale_u, scale_s)):
        other = 2 - t                                            # the block this softmax does not hold
        member = blk != other
        keys = member[:, None] & member[None, :] & ~torch.eye(n, dtype=torch.bool)
        partner = torch.where(blk == 0, (t + 1) * B + b, b)      # a_b <-> p_b (u), a_b <-> q_b (s)
        st = s.masked_fill(~keys, float("-inf"))
        lse = torch.full((n,), float("inf"), dtype=dtype)
        pos = torch.full((n,), float("nan"), dtype=dtype)
        term = torch.zeros(n, dtype=dtype)
        rows = member.nonzero().flatten()
        mx = st[rows].max(dim=1).values                          # (B = 1: one key, the partner; lse = s_pos exactly)
        lse[rows] = mx + torch.log(torch.exp(st[rows] - mx[:, None]).sum(dim=1))
        pos[rows] = s[rows, partner[rows]]
        term[rows] = lse[rows] - pos[rows]
        w = torch.zeros_like(s)
        e = torch.exp(st[rows] - lse[rows][:, None])             # 0 outside the keys
        w[rows] = e
        w = w + w.T                                              # exp(s_rj - lse_r) + exp(s_rj - lse_j): s is symmetric
        w[rows, partner[rows]] -= 2.0
        g = g + (scale * inv_temp / (2 * B)) * (w @ z)
        losses.append(scale / (2 * B) * term.sum())
        lses.append(lse)
        poss.append(pos)
        terms.append(term)
    return dict(losses=torch.stack(losses), g=g, lse=torch.stack(lses), pos=torch.stack(poss), terms=torch.stack(terms))


def duo_autograd(za, zp, zq, temp, scale_u=1.0, scale_s=1.0, dtype=torch.float64):
    """(losses (2,), g (3B x d)) by autograd of the reference's expression called twice"""
    from selfrec_amd.util.loss_torch import _info_nce_expression
    A, P, Q = (torch.as_tensor(t).detach().to(dtype).clone().requires_grad_(True) for t in (za, zp, zq))
    B = len(A)
    lu = scale_u * _info_nce_expression(A, P, temp, B, "dot")
    ls = scale_s * _info_nce_expression(A, Q, temp, B, "dot")
    (lu + ls).backward()
    return torch.stack((lu.detach(), ls.detach())), torch.cat((A.grad, P.grad, Q.grad))


# ---- cases ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def contested(B, d, seed=0):
    """(a, p, q) float32.  The base seed is one at which every loss of every case stays above 0.01 (asserted on the CPU):
    at B = 2 a draw can put one positive 7 nats ahead of its three rivals (d = 128, temp 0.5), the loss drops to 5e-4, and
    float32 torch itself then misses both bounds -- such a softmax is not contested."""
    g = torch.Generator().manual_seed(11290 + 1000 * seed + 7 * B + d)
    k = d ** -0.25
    a = torch.randn(B, d, generator=g) * k
    out = [a]
    for c in CONTESTED_C:
        out.append(c * a + (1.0 - c * c) ** 0.5 * torch.randn(B, d, generator=g) * k)
    return tuple(out)


def _layer_norm(x):
    x = x - x.mean(dim=1, keepdim=True)
    return x / x.pow(2).mean(dim=1, keepdim=True).sqrt()


@functools.lru_cache(maxsize=None)
def peaked(B, d, seed=0):
    """(a, p, q) float32, every row of norm sqrt(d)"""
    g = torch.Generator().manual_seed(9290 + 1000 * seed + 7 * B + d)
    a = _layer_norm(torch.randn(B, d, generator=g))
    return (a,) + tuple(_layer_norm(a + noise * torch.randn(B, d, generator=g)) for noise in PEAKED_NOISE)


@functools.lru_cache(maxsize=None)
def reference(family, B, d, temp, scale_u=1.0, scale_s=1.0):
    a, p, q = (contested if family == "contested" else peaked)(B, d)
    return duo(a, p, q, 1.0 / temp, scale_u, scale_s)


# ---- measures ---------------------------------------------------------------------------------------------------------
def rel_loss_figures(got, ref):
    """contested: |got - want| / |want| of each loss"""
    got = torch.as_tensor(got).detach().double().cpu()
    return [abs(float(got[t]) - float(ref["losses"][t])) / abs(float(ref["losses"][t])) for t in range(2)]


def row_den(ref):
    """per softmax and row max(1, |lse|, |s_pos|) (0 where the row has no such softmax): what lse and the row terms are
    measured against, as table_ce_ref's"""
    has = torch.isfinite(ref["lse"])
    den = torch.maximum(ref["lse"].abs().clamp_min(1.0), torch.nan_to_num(ref["pos"].abs(), nan=1.0))
    return torch.where(has, den, torch.zeros_like(den))


def peaked_loss_figures(got, ref, scales, B):
    """peaked: |got - want| over |scale| / 2B sum_m max(1, |lse_m|, |s_pos_m|), per loss; a zero scale: |got| must be 0"""
    got = torch.as_tensor(got).detach().double().cpu()
    den = row_den(ref).sum(dim=1)
    out = []
    for t in range(2):
        err = abs(float(got[t]) - float(ref["losses"][t]))
        k = abs(scales[t]) / (2 * B) * float(den[t])
        out.append(err / k if k > 0 else (0.0 if err == 0 else float("inf")))
    return out


def term_figures(got_lse, got_terms, ref):
    """(worst lse, worst row term) over both softmaxes, each |got - want| / max(1, |lse|, |s_pos|) on the rows that have one"""
    den = row_den(ref)
    has = den > 0
    el = ((torch.as_tensor(got_lse).double().cpu() - ref["lse"]).abs() / den)[has]
    et = ((torch.as_tensor(got_terms).double().cpu() - ref["terms"]).abs() / den)[has]
    worst = lambda x: float("inf") if bool(torch.isnan(x).any()) else float(x.max())
    return worst(el), worst(et)


def cancel_figure(got, ref, z, inv_temp, scales, B):
    """peaked: the worst gradient entry over what cancels in it, (|scale_u| + |scale_s|) inv_temp / 2B max|z|"""
    got = torch.as_tensor(got).detach().double().cpu()
    den = (abs(scales[0]) + abs(scales[1])) * inv_temp / (2 * B) * float(torch.as_tensor(z).abs().max())
    err = float((got - ref["g"]).abs().max())
    if err != err:
        return float("inf")
    return err / den if den > 0 else (0.0 if err == 0 else float("inf"))


def grad_figure(got, ref, floor_frac=FLOOR_FRAC):
    """contested: the worst row of row_errors; NaN anywhere is inf"""
    worst = float(row_errors(got, ref["g"], floor_frac).max())
    return worst if worst == worst else float("inf")


# ---- the workspace of srh_duo_nce_fwd_bwd, restated ---------------------------------------------------------------------
def ws_carve(B):
    """byte offsets of duo_layout: lse_u, lse_s (3B float32 each), term_u, term_s (3B float64 each), every array on a
    256-byte boundary"""
    al = lambda nbytes: (nbytes + 255) // 256 * 256
    f, dbl = al(4 * 3 * B), al(8 * 3 * B)
    return dict(lse=(0, f), term=(2 * f, 2 * f + dbl), total=2 * f + 2 * dbl)
