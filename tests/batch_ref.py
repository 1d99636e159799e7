"""Float64 restatement of the batch-gradient and optimiser kernels (csrc/losses.hip: bpr_phase1, bpr_phase2, rows_finish;
csrc/optim.hip: adam_kernel) in plain numpy, the deterministic cases the GPU tests run them on, and the error bounds those
tests hold the kernels to.  tests/test_batch_ref_cpu.py pins this file against float64 torch autograd / torch.optim.Adam and
measures the yardsticks the bounds below are four times of."""
import functools

import numpy as np

# ---- bounds (one place: tests/test_gpu_batch.py reads them, tests/test_batch_ref_cpu.py re-measures the yardsticks) --------
# Whole-tensor bounds, relative to the tensor's largest magnitude: the ones test_bpr_l2_fused_matches_oracle_with_duplicates has.
LOSS_BOUND = 2e-6
GRAD_BOUND = 2e-5
# Per-row yardsticks: what the SAME expressions give in f32 torch on the CPU (gather, bpr_loss, l2_reg_loss, index_put with
# accumulate; torch.optim.Adam) against this file, as the largest error over every case below divided by the row's / the
# element's scale.  The kernels evaluate the same terms in f32 and differ only in the order of sums of at most 40 terms: 4 x.
ROW_YARDSTICK = 2.3e-6
ADAM_YARDSTICK = {"p": 2.4e-7, "m": 1.1e-7, "v": 1.2e-7}
MARGIN = 4.0
ROW_BOUND = MARGIN * ROW_YARDSTICK
ADAM_BOUND = {k: MARGIN * y for k, y in ADAM_YARDSTICK.items()}

N_USERS, N_ITEMS = 64, 96
WIDTHS = (32, 64, 128, 256)
FAMILIES = ("ordinary", "floor", "saturated", "mixed")
TINY = (1, 2, 3, 5)
# planted list lengths (slots that name one row)
USER_LISTS = (1, 7, 8, 9, 16, 17, 40)
POS_LISTS = (1, 8, 9, 17)
NEG_LISTS = (1, 8, 9, 20)
MIXED_POS, MIXED_NEG = 3, 9
PLANTED_B = 203                 # odd: 3 B and 3 (B + 24) are multiples of no workgroup's row-group count


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def logits(user, item, u, i, j):
    uu = _f64(user)[u]
    return (uu * _f64(item)[i]).sum(1) - (uu * _f64(item)[j]).sum(1)


def bpr_terms(x):
    """sigmoid(x), 1 - sigmoid(x) (its own expression: no cancellation at large x) and the logarithm's argument 10e-6 + sigmoid(x)
    of loss_torch.py:9, float64 (tests/loss_ref.py shares them)"""
    with np.errstate(over="ignore"):
        sig = 1.0 / (1.0 + np.exp(-x))
        one_minus = 1.0 / (1.0 + np.exp(x))
    return sig, one_minus, 10e-6 + sig


def bpr_l2(user, item, reg_user, reg_item, u, i, j, reg_coef, include_neg, loss_scale):
    """loss_torch.py's bpr_loss (-log(10e-6 + sigmoid(x)), mean over rows) and l2_reg_loss (sum of Frobenius norms / rows) of the
    gathered rows with the gradients of loss_scale * (bpr + reg) w.r.t. the four tables, in float64.  A zero norm gives a zero
    gradient.  s_*: per table row, the sum over the slots naming it of the largest magnitude one slot's term can have
    ((loss_scale / rows) max|operand row| as |d loss / d x| < 1; the regulariser's coefficient times max|reg row|) -- what a
    row's error is measured against."""
    u, i, j = (np.asarray(a, dtype=np.int64) for a in (u, i, j))
    U, I, RU, RI = _f64(user), _f64(item), _f64(reg_user), _f64(reg_item)
    rows = u.size
    uu, pp, nn = U[u], I[i], I[j]
    x = (uu * pp).sum(1) - (uu * nn).sum(1)
    sig, one_minus, arg = bpr_terms(x)
    out = {"x": x, "bpr": loss_scale * np.mean(-np.log(arg))}
    c = (-(sig * one_minus) / arg) * (loss_scale / rows)
    g_user, g_item = np.zeros_like(U), np.zeros_like(I)
    np.add.at(g_user, u, c[:, None] * (pp - nn))
    np.add.at(g_item, i, c[:, None] * uu)
    np.add.at(g_item, j, -c[:, None] * uu)
    s_user, s_item = np.zeros(U.shape[0]), np.zeros(I.shape[0])
    np.add.at(s_user, u, (loss_scale / rows) * np.maximum(np.abs(pp).max(1), np.abs(nn).max(1)))
    np.add.at(s_item, i, (loss_scale / rows) * np.abs(uu).max(1))
    np.add.at(s_item, j, (loss_scale / rows) * np.abs(uu).max(1))
    # regulariser: reg_coef * (|Ru| + |Rp| [+ |Rn|]) / rows
    ru, rp, rn = RU[u], RI[i], RI[j]
    nu, npos, nneg = (np.sqrt((r * r).sum()) for r in (ru, rp, rn))
    out["reg"] = loss_scale * reg_coef * (nu + npos + (nneg if include_neg else 0.0)) / rows
    rs = reg_coef * loss_scale / rows
    greg_user, greg_item = np.zeros_like(RU), np.zeros_like(RI)
    sreg_user, sreg_item = np.zeros(RU.shape[0]), np.zeros(RI.shape[0])
    for tab, stab, idx, r, norm, on in ((greg_user, sreg_user, u, ru, nu, True), (greg_item, sreg_item, i, rp, npos, True),
                                        (greg_item, sreg_item, j, rn, nneg, bool(include_neg))):
        if on and norm > 0.0:
            np.add.at(tab, idx, (rs / norm) * r)
            np.add.at(stab, idx, abs(rs / norm) * np.abs(r).max(1))
    out.update(g_user=g_user, g_item=g_item, greg_user=greg_user, greg_item=greg_item, s_user=s_user, s_item=s_item,
               sreg_user=sreg_user, sreg_item=sreg_item)
    return out


def row_error(got, want, scale):
    """Largest |got - want| of a row over the row's scale, over the rows with a scale; rows without one (named by no slot)
    must hold exactly `want` (zero)."""
    got, want, scale = _f64(got), _f64(want), _f64(scale)
    named = scale > 0.0
    assert np.array_equal(got[~named], want[~named]), "a row that no slot names holds something"
    if not named.any():
        return 0.0
    return float((np.abs(got[named] - want[named]).max(1) / scale[named]).max())


def rel_err(got, want, floor=1e-30):
    got, want = _f64(got), _f64(want)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), floor))


def adam(p, g, m, v, t, lr, b1, b2, eps):
    """torch.optim.Adam's single-tensor step (no weight decay, bias-corrected) in float64 from the f32 inputs; lr, betas and eps
    rounded to f32 first, as the C ABI takes them.  Returns p, m, v and, for each, the magnitude of the terms it is made of."""
    lr, b1, b2, eps = (float(np.float32(z)) for z in (lr, b1, b2, eps))
    p, g, m, v = (_f64(a) for a in (p, g, m, v))
    m2 = b1 * m + (1.0 - b1) * g
    v2 = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    step = (lr / bc1) / (np.sqrt(v2) / np.sqrt(bc2) + eps)
    s_m = np.abs(b1 * m) + np.abs((1.0 - b1) * g)           # (not |m2|: the two terms may cancel, and p inherits their error)
    return {"p": p - step * m2, "m": m2, "v": v2, "s_p": np.abs(p) + step * s_m, "s_m": s_m, "s_v": v2}


def elem_error(got, want, scale):
    got, want, scale = _f64(got), _f64(want), _f64(scale)
    on = scale > 0.0
    assert np.array_equal(got[~on], want[~on]), "an element made of zero terms is not exactly its reference"
    return float((np.abs(got[on] - want[on]) / scale[on]).max()) if on.any() else 0.0


# ---- cases --------------------------------------------------------------------------------------------------------------
def _planted_indices(rng):
    """(u, i, j) of PLANTED_B slots over N_USERS x N_ITEMS with the list lengths above; the slot returned fourth is the i == j triple, whose
    user no other slot names.  User 0 and item 0 are named by nobody."""
    users = 1 + rng.permutation(N_USERS - 1)
    items = 1 + rng.permutation(N_ITEMS - 1)
    lone, planted_u, fill_u = users[0], users[:len(USER_LISTS)], users[len(USER_LISTS):len(USER_LISTS) + 21]
    it = iter(items)
    take = lambda n: np.array([next(it) for _ in range(n)])
    twin, mixed, pos, neg, fill_p, fill_n = take(1)[0], take(1)[0], take(len(POS_LISTS)), take(len(NEG_LISTS)), take(25), take(25)
    B = PLANTED_B

    def column(first, planted, counts, extra, fill):
        col = [np.repeat(planted, counts)] + [np.repeat(e, n) for e, n in extra]
        col = np.concatenate(col)
        col = np.concatenate([col, fill[np.arange(B - 1 - col.size) % fill.size]])
        return np.concatenate([[first], rng.permutation(col)])
    u = column(lone, planted_u[1:], USER_LISTS[1:], [], fill_u)          # (USER_LISTS[0] == 1: the lone user)
    i = column(twin, pos, POS_LISTS, [(mixed, MIXED_POS)], fill_p)
    j = column(twin, neg, NEG_LISTS, [(mixed, MIXED_NEG)], fill_n)
    order = rng.permutation(B)
    u, i, j = u[order], i[order], j[order]
    return u, i, j, int(np.flatnonzero(order == 0)[0]), int(mixed)


def _scale_users(user, item, u, i, j, family, rng):
    """The family's logits by scaling user rows: `floor` puts the user's strongest slot at x in [-14, -9], `saturated` at
    |x| = 120 (sign alternating over users), `mixed` deals ordinary / floor / saturated out to the users in turn."""
    if family == "ordinary":
        return user
    user = user.copy()
    x0 = logits(user, item, u, i, j)
    for rank, uid in enumerate(np.unique(u)):
        kind = family if family != "mixed" else ("ordinary", "floor", "saturated")[rank % 3]
        mine = x0[u == uid]
        top = mine[np.argmax(np.abs(mine))]
        if kind == "ordinary" or abs(top) < 0.3:
            continue
        target = rng.uniform(-14.0, -9.0) if kind == "floor" else (120.0 if (rank // 3) % 2 else -120.0)
        user[uid] *= np.float32(target / top)
    return user


@functools.lru_cache(maxsize=None)
def batch_case(kind, d, family, seed=0):
    """kind: 'planted' or a tiny batch size.  Read-only f32 tables (user, item: the family's; ego_user, ego_item: separate
    regulariser tables), int64 u, i, j."""
    rng = np.random.default_rng([seed, d, FAMILIES.index(family), 0 if kind == "planted" else int(kind)])
    case = {"d": d, "family": family, "kind": kind}
    if kind == "planted":
        case["u"], case["i"], case["j"], case["twin_slot"], case["mixed_item"] = _planted_indices(rng)
    else:
        B = int(kind)
        # (i != j: a chance twin's two item terms cancel, and in a batch this small that leaves the row -- at times the whole
        #  table -- made of the cancellation's rounding, which no bound relative to the table's largest value is about;
        #  the planted batch has the one deliberate twin)
        case["u"], case["i"] = rng.integers(0, N_USERS, B), rng.integers(0, N_ITEMS, B)
        case["j"] = (case["i"] + rng.integers(1, N_ITEMS, B)) % N_ITEMS
    tab = lambda n: (rng.standard_normal((n, d)) * 0.3).astype(np.float32)
    user, case["item"], case["ego_user"], case["ego_item"] = tab(N_USERS), tab(N_ITEMS), tab(N_USERS), tab(N_ITEMS)
    case["user"] = _scale_users(user, case["item"], case["u"], case["i"], case["j"], family, rng)
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def planted_batch(d, seed=0, family="ordinary"):
    return batch_case("planted", d, family, seed)


def all_batch_cases():
    for d in WIDTHS:
        for family in FAMILIES:
            for kind in ("planted",) + TINY:
                yield batch_case(kind, d, family)


CONFIGS = ((False, False), (True, False), (True, True), (False, True))          # (include_neg, separate ego tables)
REG_COEF, LOSS_SCALE = 1e-3, 0.75


def reference(case, include_neg, ego):
    ru, ri = (case["ego_user"], case["ego_item"]) if ego else (case["user"], case["item"])
    return bpr_l2(case["user"], case["item"], ru, ri, case["u"], case["i"], case["j"], REG_COEF, include_neg, LOSS_SCALE)


ADAM_STEPS = (1, 2, 10, 1000, 100000)
ADAM_HYPER = dict(lr=0.01, b1=0.9, b2=0.999, eps=1e-8)


def adam_case(rows, d, seed=0):
    """p of the update's order; gradients over ten decades (1e-8 .. 1e2) in one tensor; m, v consistent with such a history;
    every 7th element has g = 0 and v = 0 (half of them m = 0 too)."""
    rng = np.random.default_rng([seed, rows, d])
    n = rows * d
    g = (np.sign(rng.standard_normal(n)) * 10.0 ** rng.uniform(-8.0, 2.0, n)).astype(np.float32)
    m = (g * rng.uniform(-1.0, 1.0, n)).astype(np.float32)
    v = (g.astype(np.float64) ** 2 * rng.uniform(0.5, 1.5, n)).astype(np.float32)
    p = (rng.standard_normal(n) * 0.01).astype(np.float32)
    g[::7] = 0.0
    v[::7] = 0.0
    m[::7] = (rng.standard_normal(m[::7].size) * 1e-9).astype(np.float32)      # (|update| = lr 0.9 m / eps: of p's order)
    m[::14] = 0.0
    return tuple(a.reshape(rows, d) for a in (p, g, m, v))
