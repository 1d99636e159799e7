"""References for the DirectAU loss kernels (csrc/au.hip, include/selfrec_hip.h (a-22)) -- TEST
INFRASTRUCTURE ONLY, written from the header's contract and never imported by the product; no GPU needed.

    reference      the reference's expression (model/graph/DirectAU.py:37-48: F.normalize, torch.pdist) with autograd,
                   float64 by default (dtype=torch.float32 gives the same expression in plain f32: the floor's yardstick)
    closed_form    the header's closed form in float64, in query chunks: nothing n x n is held
    grad_errors    per row, like contrastive_ref.row_errors, with the clamped and the ordinary rows each on their own and
                   the cancelling rows against cancel_scales
    cancel_scales  the size of what cancels in a row whose exact gradient is (nearly) zero
    chunk_plan     srh_au_chunk_plan restated, so the case list can name the layout it reaches
"""
import torch
import torch.nn.functional as F

LOSS_TOL = 1e-5      # |loss - ref| <= LOSS_TOL * sum_k |w_k| max(1, |part_k|); each part to LOSS_TOL * max(1, |part|)
GRAD_TOL = 1e-4      # gradients against float64, per row through grad_errors
# the smallest of FLOORS at which the reference's own expression in plain float32 torch on the CPU stays within
# GRAD_TOL / 2 per row on every case (test_au_ref_cpu.py::test_floor_frac_is_the_smallest_that_float32_torch_meets)
FLOORS = (1e-3, 1e-2, 1e-1, 1.0)
FLOOR_FRAC = 1e-2
NORM_EPS = 1e-12     # F.normalize's eps


# ---- the reference's expression -------------------------------------------------------------------------------------
def alignment(x, y):
    x, y = F.normalize(x, dim=-1), F.normalize(y, dim=-1)
    return (x - y).norm(p=2, dim=1).pow(2).mean()


def uniformity(x, t=2):
    x = F.normalize(x, dim=-1)
    return torch.pdist(x, p=2).pow(2).mul(-t).exp().mean().log()


def _leaf(x, dtype, device):
    return x.detach().to(device=device or x.device, dtype=dtype).clone().requires_grad_(True)


def reference(x, y, t, w, dtype=torch.float64, device=None):
    """(loss, parts (3,), gx, gy) of w[0] alignment(x, y) + w[1] uniformity(x, t) + w[2] uniformity(y, t) by autograd;
    y=None: w[1] uniformity(x, t) alone (parts[0], parts[2] are nan, gy None)"""
    x_ = _leaf(x, dtype, device)
    if y is None:
        ux = uniformity(x_, t)
        (w[1] * ux).backward()
        nan = torch.full((), float("nan"), dtype=dtype, device=x_.device)
        return (w[1] * ux).detach(), torch.stack([nan, ux.detach(), nan]), x_.grad, None
    y_ = _leaf(y, dtype, device)
    parts = [alignment(x_, y_), uniformity(x_, t), uniformity(y_, t)]
    loss = w[0] * parts[0] + w[1] * parts[1] + w[2] * parts[2]
    loss.backward()
    return loss.detach(), torch.stack([p.detach() for p in parts]), x_.grad, y_.grad


# ---- the closed form ------------------------------------------------------------------------------------------------
def _side(x, t, chunk):
    """normalised rows, 1 / max(|x|, eps), the clamped flags, r, Z, U and dU/dxh of one matrix, float64"""
    n = len(x)
    norm = x.norm(dim=1)
    inv = 1.0 / norm.clamp_min(NORM_EPS)
    xh = x * inv[:, None]
    q = (xh * xh).sum(1)
    r = torch.zeros(n, dtype=x.dtype, device=x.device)
    o = torch.zeros_like(xh)
    for i0 in range(0, n, chunk):
        i1 = min(n, i0 + chunk)
        s = xh[i0:i1] @ xh.T
        wgt = torch.exp(-t * (q[i0:i1, None] + q[None, :] - 2.0 * s).clamp_min(0.0))
        wgt[torch.arange(i1 - i0), torch.arange(i0, i1)] = 0.0
        r[i0:i1] = wgt.sum(1)
        o[i0:i1] = wgt @ xh
    z = r.sum()
    return dict(xh=xh, inv=inv, clamped=norm < NORM_EPS, r=r, z=z, u=torch.log(z / (n * (n - 1.0))),
                g=-(4.0 * t / z) * (r[:, None] * xh - o))


def _norm_bwd(g, s):
    proj = g - s["xh"] * (s["xh"] * g).sum(1, keepdim=True)
    return torch.where(s["clamped"][:, None], g, proj) * s["inv"][:, None]


def closed_form(x, y, t, w, chunk=512, device=None):
    """reference()'s results from the header's closed form, float64"""
    n = len(x)
    sx = _side(x.detach().to(device=device or x.device, dtype=torch.float64), t, chunk)
    if y is None:
        nan = torch.full((), float("nan"), dtype=torch.float64, device=sx["u"].device)
        return w[1] * sx["u"], torch.stack([nan, sx["u"], nan]), _norm_bwd(w[1] * sx["g"], sx), None
    sy = _side(y.detach().to(device=device or y.device, dtype=torch.float64), t, chunk)
    dlt = sx["xh"] - sy["xh"]
    a = (dlt * dlt).sum(1).mean()
    ga = 2.0 * w[0] * dlt / n
    loss = w[0] * a + w[1] * sx["u"] + w[2] * sy["u"]
    return (loss, torch.stack([a, sx["u"], sy["u"]]), _norm_bwd(w[1] * sx["g"] + ga, sx),
            _norm_bwd(w[2] * sy["g"] - ga, sy))


def cancel_scales(x, y, t, w, chunk=512):
    """(per row of x, per row of y): (|w_u| 4 t r_i / Z + 2 |w_align| / n) / max(|x_i|, eps), the size of the two radial
    terms r_i xh_i and xh_i that the projection of the normalisation backward (or an equal partner) cancels.  Rows of
    this kind: all rows identical (sum_j w_ij xh_j = r_i xh_i); x_i = y_i; the partner of a clamped (near-zero) row,
    whose alignment gradient is purely radial.  float32 leaves about 1e-7 of these."""
    n = len(x)
    out = []
    for m, wu in ((x, w[1]), (y, w[2])):
        if m is None:
            out.append(None)
            continue
        s = _side(m.detach().double().cpu(), t, chunk)
        out.append((abs(wu) * 4.0 * t * s["r"] / s["z"] + (0.0 if y is None else 2.0 * abs(w[0]) / n)) * s["inv"])
    return tuple(out)


# ---- the error measures ---------------------------------------------------------------------------------------------
def clamped_rows(x):
    """the rows F.normalize clamps, in float64 (the cases keep them clear of the threshold in float32 too)"""
    return x.detach().double().cpu().norm(dim=1) < NORM_EPS


def grad_errors(got, want, clamped, cancel=None, scales=None, floor_frac=FLOOR_FRAC):
    """per row, float64 (n,): max|got - want| over max(max|want_row|, floor_frac * the largest magnitude of the row's
    GROUP) -- the clamped rows (gradients 1e12 times the others') and the ordinary rows are each a group; a row of
    `cancel` is measured against scales[row] instead"""
    got = torch.as_tensor(got).detach().double().cpu()
    want = torch.as_tensor(want).detach().double().cpu()
    err = (got - want).abs().amax(1)
    mag = want.abs().amax(1)
    den = torch.zeros_like(mag)
    for grp in (clamped, ~clamped):
        if grp.any():
            den[grp] = torch.clamp(mag[grp], min=floor_frac * float(mag[grp].max()))
    if cancel is not None and cancel.any():
        den[cancel] = scales[cancel]
    out = err / den
    out[(den == 0) & (err == 0)] = 0.0
    return out


def loss_bound(parts, w, one_sided=False):
    """LOSS_TOL * sum_k |w_k| max(1, |part_k|) over the parts the call computes"""
    ks = (1,) if one_sided else (0, 1, 2)
    return LOSS_TOL * sum(abs(w[k]) * max(1.0, abs(float(parts[k]))) for k in ks)


# ---- the key chunks of csrc/au.hip ----------------------------------------------------------------------------------
AU_ROWS, AU_TARGET = 64, 512


def chunk_plan(n):
    """au_chunks / au_chunk_len (the header's chunk plan): chunks, chunk_len, and what they hold -- live (chunks that
    start below n), empty (chunks - live), last_keys (keys of the last live chunk), tiles (64-row tiles)"""
    tiles = -(-n // AU_ROWS)
    chunks = max(1, min(tiles, -(-AU_TARGET // (2 * tiles))))
    chunk_len = -(-(-(-n // chunks)) // AU_ROWS) * AU_ROWS
    live = -(-n // chunk_len)
    return dict(chunks=chunks, chunk_len=chunk_len, live=live, empty=chunks - live, last_keys=n - (live - 1) * chunk_len,
                tiles=tiles)
