"""Float64 restatement of the GRU recurrence kernels (include/selfrec_hip.h (a-26)) and of ops.GruFn's
finish, literally the header's formulas, with the cases the CPU and GPU tests share.

Bounds (the project's usual two): out and gates <= 1e-5, dgi, dghn and every gradient of GruFn <= 1e-4, each relative to
its tensor's largest magnitude.  tests/test_gru_ref_cpu.py shows float32 arithmetic stays inside half of each on every
case below, so the bounds ask nothing the number format cannot give."""
import functools

import numpy as np
import torch

OUT_BOUND = 1e-5
GRAD_BOUND = 1e-4

# (B, L, H): one sequence of one step; a ragged tile; exactly one tile; one row into a second tile with L off any power of
# two; L at the attention kernels' old edge; three tiles at the conf's length; a long recurrence; H = 32 through the pad
SHAPES = ((1, 1, 64), (3, 7, 64), (16, 16, 64), (17, 33, 64), (5, 64, 64), (33, 50, 64), (2, 200, 64), (4, 12, 32))
PATTERNS = ("full", "ones", "ragged", "short", "zero")
# the closed form against float64 autograd (CPU only; H = 128 is outside the kernels' envelope, not outside the formulas)
AUTOGRAD_SHAPES = ((3, 7, 64), (5, 64, 64), (4, 50, 128), (17, 200, 64))


def lengths(B, L, pattern, seed=0):
    """the int64 (B,) lengths of a pattern: all L; all 1; ragged with a 1 and an L (row 0 is 1 where B >= 2, the last
    row L); the first tile's 16 rows all shorter than L (zeros at L = 1), the rest ragged; ragged with the middle row 0"""
    rs = np.random.RandomState(1000 + 17 * B + L + seed)
    rag = rs.randint(1, L + 1, size=B)
    rag[-1] = L
    if B >= 2:
        rag[0] = 1
    if pattern == "full":
        return np.full(B, L, dtype=np.int64)
    if pattern == "ones":
        return np.ones(B, dtype=np.int64)
    if pattern == "ragged":
        return rag.astype(np.int64)
    if pattern == "short":
        out = rag.copy()
        out[:16] = rs.randint(1, L, size=min(B, 16)) if L > 1 else 0
        return out.astype(np.int64)
    if pattern == "zero":
        out = rag.copy()
        out[B // 2] = 0
        return out.astype(np.int64)
    raise ValueError(pattern)


def gru_fwd(gi, w_hh, b_hh, lens, dtype=torch.float64):
    """(out (B, L, H), gates (B, L, 4H) = [r, z, n, gh_n]) of header (a-26); zeros at t >= len"""
    gi, w_hh, b_hh = (torch.as_tensor(t).to(dtype) for t in (gi, w_hh, b_hh))
    lens = torch.as_tensor(np.asarray(lens)).long()
    B, L, H = gi.shape[0], gi.shape[1], gi.shape[2] // 3
    out, gates = torch.zeros((B, L, H), dtype=dtype), torch.zeros((B, L, 4 * H), dtype=dtype)
    h = torch.zeros((B, H), dtype=dtype)
    for t in range(L):
        a = (t < lens).unsqueeze(1)
        g = torch.where(a, gi[:, t], torch.zeros_like(gi[:, t]))
        gh = h @ w_hh.T + b_hh
        r = torch.sigmoid(g[:, :H] + gh[:, :H])
        z = torch.sigmoid(g[:, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(g[:, 2 * H:] + r * gh[:, 2 * H:])
        hn = (1 - z) * n + z * h
        h = torch.where(a, hn, h)
        out[:, t] = torch.where(a, hn, torch.zeros_like(hn))
        row = torch.cat((r, z, n, gh[:, 2 * H:]), dim=1)
        gates[:, t] = torch.where(a, row, torch.zeros_like(row))
    return out, gates


def gru_bwd(go, out, gates, w_hh, lens, dtype=torch.float64):
    """(dgi (B, L, 3H), dghn (B, L, H)) of header (a-26); zeros at t >= len, where go is not read"""
    go, out, gates, w_hh = (torch.as_tensor(t).to(dtype) for t in (go, out, gates, w_hh))
    lens = torch.as_tensor(np.asarray(lens)).long()
    B, L, H = out.shape
    dgi, dghn = torch.zeros((B, L, 3 * H), dtype=dtype), torch.zeros((B, L, H), dtype=dtype)
    carry = torch.zeros((B, H), dtype=dtype)
    zero = torch.zeros((B, H), dtype=dtype)
    for t in range(L - 1, -1, -1):
        a = (t < lens).unsqueeze(1)
        dh = carry + torch.where(a, go[:, t], zero)
        hp = out[:, t - 1] if t > 0 else zero
        r, z, n, ghn = gates[:, t].split(H, dim=1)
        dn = dh * (1 - z) * (1 - n * n)
        dz = dh * (hp - n) * z * (1 - z)
        dr = dn * ghn * r * (1 - r)
        dnr = dn * r
        row = torch.cat((dr, dz, dn), dim=1)
        dgi[:, t] = torch.where(a, row, torch.zeros_like(row))
        dghn[:, t] = torch.where(a, dnr, zero)
        carry = torch.where(a, dh * z + torch.cat((dr, dz, dnr), dim=1) @ w_hh, zero)
    return dgi, dghn


def gru_finish(x, w_ih, out, dgi, dghn, dtype=torch.float64):
    """ops.GruFn's GEMMs on the zero-padded outputs -> dict(dx, dw_ih, db_ih, dw_hh, db_hh)"""
    x, w_ih, out, dgi, dghn = (torch.as_tensor(t).to(dtype) for t in (x, w_ih, out, dgi, dghn))
    B, L, H = out.shape
    d2 = dgi.reshape(B * L, 3 * H)
    dgh = torch.cat((dgi[..., :2 * H], dghn), dim=-1).reshape(B * L, 3 * H)
    h_prev = torch.zeros_like(out)
    h_prev[:, 1:] = out[:, :-1]
    return dict(dx=(d2 @ w_ih).reshape(x.shape), dw_ih=d2.T @ x.reshape(B * L, -1), db_ih=d2.sum(0),
                dw_hh=dgh.T @ h_prev.reshape(B * L, H), db_hh=dgh.sum(0))


def gru_layer(x, w_ih, w_hh, b_ih, b_hh, lens, go, dtype=torch.float64):
    """one layer forward and backward by the restatement: dict(out, gates, dgi, dghn, dx, dw_ih, dw_hh, db_ih, db_hh)"""
    x, w_ih, w_hh, b_ih, b_hh = (torch.as_tensor(t).to(dtype) for t in (x, w_ih, w_hh, b_ih, b_hh))
    out, gates = gru_fwd(x @ w_ih.T + b_ih, w_hh, b_hh, lens, dtype)
    dgi, dghn = gru_bwd(go, out, gates, w_hh, lens, dtype)
    return dict(out=out, gates=gates, dgi=dgi, dghn=dghn, **gru_finish(x, w_ih, out, dgi, dghn, dtype))


def torch_layer(x, w_ih, w_hh, b_ih, b_hh, lens, go, dtype=torch.float64):
    """the same layer as autograd of torch.nn.GRU(...)[0] * live -> dict(out, dx, dw_ih, dw_hh, db_ih, db_hh)"""
    x = torch.as_tensor(x).to(dtype).clone().requires_grad_(True)
    B, L, D = x.shape
    H = w_hh.shape[1]
    gru = torch.nn.GRU(D, H, num_layers=1, batch_first=True).to(dtype)
    with torch.no_grad():
        for p, v in zip((gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0), (w_ih, w_hh, b_ih, b_hh)):
            p.copy_(torch.as_tensor(v).to(dtype))
    live = (torch.arange(L)[None, :] < torch.as_tensor(np.asarray(lens)).long()[:, None]).unsqueeze(-1)
    out = gru(x)[0] * live
    go = torch.where(live, torch.as_tensor(go).to(dtype), torch.zeros((), dtype=dtype))
    (out * go).sum().backward()
    return dict(out=out.detach(), dx=x.grad, dw_ih=gru.weight_ih_l0.grad, dw_hh=gru.weight_hh_l0.grad,
                db_ih=gru.bias_ih_l0.grad, db_hh=gru.bias_hh_l0.grad)


@functools.lru_cache(maxsize=None)
def case(B, L, H, pattern, scale=1.0):
    """the float32 inputs of a case, made once: x and go ~ N(0, 1), the layer's parameters at torch's default init
    U(-1/sqrt(H), 1/sqrt(H)) times ``scale``, the lengths, and the float64 restatement ``ref`` of the whole layer"""
    g = torch.Generator().manual_seed(7919 * B + 31 * L + H + PATTERNS.index(pattern))
    k = scale / H ** 0.5
    uni = lambda *s: ((torch.rand(*s, generator=g) * 2 - 1) * k).float()  # noqa: E731
    c = dict(x=torch.randn(B, L, H, generator=g), go=torch.randn(B, L, H, generator=g), w_ih=uni(3 * H, H),
             w_hh=uni(3 * H, H), b_ih=uni(3 * H), b_hh=uni(3 * H), lens=lengths(B, L, pattern))
    c["ref"] = gru_layer(c["x"], c["w_ih"], c["w_hh"], c["b_ih"], c["b_hh"], c["lens"], c["go"])
    return c


def cases():
    """every (B, L, H, pattern, scale) the GPU tests run: all patterns at scale 1, the ragged one at 3 too"""
    return [(B, L, H, p, 1.0) for (B, L, H) in SHAPES for p in PATTERNS] + [(B, L, H, "ragged", 3.0) for (B, L, H) in SHAPES]


def rel_err(got, want):
    """max |got - want| over max |want| (over 1 where want is all zeros: the difference itself)"""
    got, want = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double().cpu()
    if got.numel() == 0:
        return 0.0
    top = float(want.abs().max())
    return float((got - want).abs().max()) / (top if top > 0 else 1.0)


def dead_mask(lens, L):
    """(B, L) bool: t >= len"""
    return torch.arange(L)[None, :] >= torch.as_tensor(np.asarray(lens)).long()[:, None]
