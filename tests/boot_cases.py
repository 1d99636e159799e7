"""Seeded cases for the bootstrap loss kernels (csrc/bootstrap.hip) -- TEST INFRASTRUCTURE ONLY.  A case is a dict: name,
form ('buir' | 'selfcf'), m, x_u, x_i (B x d), W (d x d), b (d), T_u, T_i (float32 CPU), idx_u, idx_i (int32, or None with
one target row per slot), store (the tables also receive x), cancel_u / cancel_i (bool masks of the rows measured against
boot_ref.cancel_scales, or None).  tests/test_boot_ref_cpu.py checks their premises; tests/test_gpu_boot.py runs the kernels.

The kernels' edges: 16 rows per wave, 64 rows per workgroup, 256 rows per chunk of the weight-gradient reductions."""
import torch

FORMS = (("buir", None), ("selfcf", 0.05), ("selfcf", 0.995))
ROWS = (1, 15, 16, 17, 63, 64, 65, 129, 255, 256, 257, 513)
LARGE_B = 2049
WIDTHS = (64, 128)
PAD_WIDTHS = (50, 100)
DEGENERATE_SHAPES = ((65, 64), (129, 128))
REPEAT_SHAPES = ((2049, 64), (257, 128))
HISTORY = (2049, 300)        # slots, ids: d_store == d_tgt
DUP = (257, 40)
MOMENTUM_N = (1, 63, 64, 65, 2049)
MOMENTUM_D = (50, 64, 128)


def form_name(form, m):
    return form if m is None else f"{form}-m{m}"


def plain_case(B, d, form="buir", m=None, gathered=False, store=None, ids=None, seed=None):
    """rows as a batch gathers them: x = online table[idx], so slots of one id hold the same bits.  ids = (n_users, n_items)
    (default: about 2 B / 3 and 3 B / 4, so the batch repeats ids); gathered: the targets as one row per slot, no index"""
    g = torch.Generator().manual_seed(1000 + 7 * B + d + (0 if m is None else int(m * 1000)) if seed is None else seed)
    nu, ni = ids or (max(1, (2 * B) // 3), max(1, (3 * B) // 4))
    on_u, on_i = torch.randn(nu, d, generator=g) * 0.1, torch.randn(ni, d, generator=g) * 0.1
    T_u, T_i = torch.randn(nu, d, generator=g) * 0.1, torch.randn(ni, d, generator=g) * 0.1
    W = torch.randn(d, d, generator=g) / d ** 0.5
    b = torch.randn(d, generator=g) * 0.1
    idx_u = torch.randint(0, nu, (B,), generator=g).to(torch.int32)
    idx_i = torch.randint(0, ni, (B,), generator=g).to(torch.int32)
    c = dict(name=f"{form_name(form, m)}-B{B}-d{d}" + ("-gathered" if gathered else ""), form=form, m=m,
             x_u=on_u[idx_u.long()].contiguous(), x_i=on_i[idx_i.long()].contiguous(), W=W, b=b, T_u=T_u, T_i=T_i, idx_u=idx_u,
             idx_i=idx_i, store=(form == "selfcf") if store is None else store, cancel_u=None, cancel_i=None)
    if gathered:
        c.update(T_u=T_u[idx_u.long()].contiguous(), T_i=T_i[idx_i.long()].contiguous(), idx_u=None, idx_i=None, store=False)
    return c


def row_cases(B):
    """every form and width at B rows, the targets as table + idx; and one pre-gathered case per form"""
    out = [plain_case(B, d, f, m) for f, m in FORMS for d in WIDTHS]
    return out + [plain_case(B, 64 if k % 2 else 128, f, m, gathered=True) for k, (f, m) in enumerate(FORMS)]


def pad_cases():
    return [plain_case(B, d, f, m) for B, d in ((65, PAD_WIDTHS[0]), (129, PAD_WIDTHS[1])) for f, m in FORMS]


def large_cases():
    return [plain_case(LARGE_B, 64, "buir"), plain_case(LARGE_B, 128, "selfcf", 0.995)]


DEG = dict(zero_p=5, p_below=6, p_above=7, t_below=8, t_above=9, zero_t=10, parallel=11, antiparallel=12)


def _scale_to(v, norm):
    return (v.double() * (norm / float(v.double().norm()))).float()


def degenerate_case(B, d, form, m):
    """b = 0 and one id per slot (so single rows can be set), user side; the item side mirrors it 13 rows further on.
    zero_p: x = 0, so p = 0; p_below / p_above: |W x| = 0.8 eps / 1.25 eps; t_below / t_above: |t| = 0.8 eps / 1.25 eps;
    zero_t: t = 0; parallel / antiparallel: t = +-0.7 p (the cancelling rows).  Everything is finite."""
    c = plain_case(B, d, form, m, ids=(B, B), seed=5000 + B + d + (0 if m is None else int(m * 1000)))
    g = torch.Generator().manual_seed(77)
    c["idx_u"], c["idx_i"] = torch.randperm(B, generator=g).to(torch.int32), torch.randperm(B, generator=g).to(torch.int32)
    c["b"] = torch.zeros(d)
    c["name"] = "degenerate-" + c["name"]
    alpha, beta, eps = (1.0, 0.0, 1e-12) if form == "buir" else (m, 1.0 - m, 1e-8)
    W64 = c["W"].double()
    x = {"u": c["x_u"], "i": c["x_i"]}
    T = {"u": c["T_u"], "i": c["T_i"]}
    idx = {"u": c["idx_u"].long(), "i": c["idx_i"].long()}
    cancel = {"u": torch.zeros(B, dtype=torch.bool), "i": torch.zeros(B, dtype=torch.bool)}

    def set_target(side, r, t):
        """make t_side[r] = t (to float32 rounding): the table row, given the slot's x row"""
        T[side][idx[side][r]] = ((t.double() - beta * x[side][r].double()) / alpha).float()

    for s, o, off in (("u", "i", 0), ("i", "u", 13)):       # p of side s meets the target of side o
        r = {k: v + off for k, v in DEG.items()}
        x[s][r["zero_p"]] = 0.0
        for key, f in (("p_below", 0.8), ("p_above", 1.25)):
            x[s][r[key]] = _scale_to(x[s][r[key]], f * eps * float(x[s][r[key]].double().norm())
                                     / float((W64 @ x[s][r[key]].double()).norm()))
        v = torch.randn(d, generator=g)
        for key, f in (("t_below", 0.8), ("t_above", 1.25)):
            if beta != 0.0:                                  # the slot's own x row is part of its target: take it out
                x[o][r[key]] = 0.0
            set_target(o, r[key], _scale_to(v, f * eps))
        if beta != 0.0:
            x[o][r["zero_t"]] = 0.0
        set_target(o, r["zero_t"], torch.zeros(d))
        for key, lam in (("parallel", 0.7), ("antiparallel", -0.7)):
            set_target(o, r[key], (lam * (W64 @ x[s][r[key]].double())).float())
            cancel[s][r[key]] = True
    c["cancel_u"], c["cancel_i"] = cancel["u"], cancel["i"]
    return c


def degenerate_cases():
    return [degenerate_case(B, d, f, m) for B, d in DEGENERATE_SHAPES for f, m in FORMS]


def duplicate_cases():
    """257 slots over 40 ids; all slots one id; and slots whose id is -1 or n_tgt (their x rows are the slot's own)"""
    B, ids = DUP
    out = []
    for k, (f, m) in enumerate(FORMS):
        d = WIDTHS[k % 2]
        out.append(dict(plain_case(B, d, f, m, ids=(ids, ids), seed=6000 + k), name=f"dup40-{form_name(f, m)}-d{d}"))
        out.append(dict(plain_case(B, d, f, m, ids=(1, 1), seed=6100 + k), name=f"one-id-{form_name(f, m)}-d{d}"))
        c = dict(plain_case(B, d, f, m, ids=(ids, ids), seed=6200 + k), name=f"outside-{form_name(f, m)}-d{d}")
        g = torch.Generator().manual_seed(6300 + k)
        for side in ("u", "i"):
            idx, x = c["idx_" + side].clone(), c["x_" + side].clone()
            bad = torch.randperm(B, generator=g)[:24]
            idx[bad[:12]], idx[bad[12:]] = -1, ids
            x[bad] = torch.randn(24, d, generator=g) * 0.1
            c["idx_" + side], c["x_" + side], c["bad_" + side] = idx, x, bad
        out.append(c)
    return out


def history_case():
    B, ids = HISTORY
    return dict(plain_case(B, 64, "selfcf", 0.05, ids=(ids, ids), seed=7000), name="history-2049-over-300")


def cpu_cases():
    """every loss case the GPU tests run"""
    out = [c for B in ROWS for c in row_cases(B)]
    return out + pad_cases() + large_cases() + degenerate_cases() + duplicate_cases() + [history_case()]


def momentum_case(n, d, seed=None):
    """tgt, src (rows x d), idx (n slots over about n / 3 ids: heavy duplicates, all inside the table) and m"""
    g = torch.Generator().manual_seed(8000 + 3 * n + d if seed is None else seed)
    rows = max(4, n // 3 + 5)
    tgt, src = torch.randn(rows, d, generator=g), torch.randn(rows, d, generator=g)
    idx = torch.randint(0, max(1, rows - 3), (n,), generator=g).to(torch.int32)      # (the last three rows: never named)
    return dict(tgt=tgt, src=src, idx=idx, m=0.995, rows=rows)
