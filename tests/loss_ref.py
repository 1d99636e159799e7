"""Float64 restatement of the drop-in loss functions' single-launch kernels (csrc/losses.hip: bpr_plain_fwd, bpr_plain_bwd,
l2_reg_fwd_kernel, l2_reg_bwd_kernel behind util/loss_torch.py's bpr_loss and l2_reg_loss) in plain numpy, the deterministic
cases the GPU tests run them on, and the error bounds those tests hold them to -- TEST INFRASTRUCTURE ONLY, no GPU needed.
tests/test_loss_ref_cpu.py pins this file against float64 torch autograd of the reference's expressions (loss_torch.py:6-22)
and measures the yardsticks the bounds below are four times of; tests/test_gpu_loss_edges.py runs the
kernels."""
import functools

import numpy as np

from tests.batch_ref import FAMILIES, MARGIN, _f64, bpr_terms, elem_error, row_error  # noqa: F401  (the measures, re-exported)

# ---- bounds (one place: tests/test_gpu_loss_edges.py reads them, tests/test_loss_ref_cpu.py re-measures the yardsticks) ----
# Yardsticks: what the reference's own expressions give in f32 torch autograd on the CPU against this file, as the largest
# scaled error over every case, family, shape and upstream gradient below.  The kernels evaluate the same f32 terms and
# differ in the order of sums and in expf / logf: MARGIN x.
#   loss   |loss - loss64| / max(|loss64|, 1), both functions
#   row    BPR: a gradient row over (|gout| / B) max|operand row|, and coef over 1 / B
#   elem   L2: a gradient element over (|gout reg| / rows_k) max|X_k| / ||X_k||
#   norm   L2: ||X_k|| over itself (f32 torch.norm on the CPU)
LOSS_YARDSTICK = 4.0e-7
ROW_YARDSTICK = 8.5e-7
ELEM_YARDSTICK = 1.4e-5
NORM_YARDSTICK = 1.4e-5
LOSS_BOUND = MARGIN * LOSS_YARDSTICK
ROW_BOUND = MARGIN * ROW_YARDSTICK
ELEM_BOUND = MARGIN * ELEM_YARDSTICK
NORM_BOUND = MARGIN * NORM_YARDSTICK

GOUTS = (1.0, 3.7, -2.5, 0.0)          # upstream gradients, both losses


def loss_error(got, want):
    """against max(|want|, 1): a bound relative to the all-saturated-positive loss -log(1 + 1e-5) = -1e-5 would be about
    float32's rounding of 1 + 1e-5, not about the kernel"""
    return abs(float(got) - float(want)) / max(abs(float(want)), 1.0)


# ---- the restatement ----------------------------------------------------------------------------------------------------
def bpr(u, p, n, gout):
    """loss_torch.py:6-10 in float64 from (B, d) operands: the margins x, the rows' losses, their mean, coef = d mean / d x
    (what ops.bpr_fwd leaves), the gradients of gout * mean and, per gradient row, the largest magnitude its terms can
    have: (|gout| / B) max|operand row|, since |d loss / d x| < 1 (batch_ref.bpr_l2 argues it)."""
    U, P, N = _f64(u), _f64(p), _f64(n)
    B = U.shape[0]
    x = (U * P).sum(1) - (U * N).sum(1)
    sig, one_minus, arg = bpr_terms(x)
    rows = -np.log(arg)
    coef = (-(sig * one_minus) / arg) / B
    c = (coef * float(gout))[:, None]
    s = abs(float(gout)) / B
    s_item = s * np.abs(U).max(1)
    return {"x": x, "rows": rows, "loss": float(rows.mean()), "coef": coef, "s_coef": np.full(B, 1.0 / B),
            "gu": c * (P - N), "gp": c * U, "gn": -c * U,
            "s_u": s * np.maximum(np.abs(P).max(1), np.abs(N).max(1)), "s_p": s_item, "s_n": s_item}


def l2(reg, blocks, gout):
    """loss_torch.py:18-22 in float64: reg * sum_k ||X_k||_F / rows_k, the norms, per slot the gradient of gout * loss
    (zero where the norm is zero) and each element's scale (|gout reg| / rows_k) max|X_k| / ||X_k|| (0 for a zero block).
    A tensor given in two slots receives the sum of its slots' gradients, and the sum of their scales: the caller adds."""
    xs = [_f64(b) for b in blocks]
    norms = np.array([np.sqrt((x * x).sum()) for x in xs])
    loss = float(reg) * sum(nk / x.shape[0] for nk, x in zip(norms, xs))
    grads, scales = [], []
    for nk, x in zip(norms, xs):
        if nk > 0.0:
            k = float(gout) * float(reg) / x.shape[0] / nk
            grads.append(k * x)
            scales.append(abs(k) * float(np.abs(x).max()))
        else:
            grads.append(np.zeros_like(x))
            scales.append(0.0)
    return {"loss": float(loss), "norms": norms, "grads": grads, "scales": scales}


def l2_by_tensor(ref, names):
    """the slots of one l2 call folded by the tensor they name: {name: (gradient, scale)}, sums over repeated names"""
    out = {}
    for name, g, s in zip(names, ref["grads"], ref["scales"]):
        out[name] = (out[name][0] + g, out[name][1] + s) if name in out else (g, s)
    return out


# ---- BPR cases ------------------------------------------------------------------------------------------------------------
WIDTHS = (32, 64, 128, 256)
MANY_ROWS = 515          # many workgroups behind the last-arriver ticket (odd: no multiple of any row-group count)
PADDED = ((17, 4), (33, 8), (65, 50), (9, 100), (5, 129), (5, 200))          # (B, d): d pads to 32, 32, 64, 128, 256, 256
FLOOR_RANGE = (-13.0, -10.0)
SATURATED_AT = (40.0, -40.0, -100.0)          # 1 - sigmoid == 0; far below the 10e-6 floor; past expf's overflow


def rows_per_workgroup(d):
    return 1024 // d          # 256 / LPR, LPR = d / 4


def bpr_shapes():
    """(B, d): every served width at the row counts around one and two workgroups of the forward kernel (the backward's
    blocks of 256 threads end at B * d / 4, so r rows fill exactly one), a few hundred rows, and the padded widths"""
    out = []
    for d in WIDTHS:
        r = rows_per_workgroup(d)
        out += [(B, d) for B in (1, r - 1, r, r + 1, 2 * r + 1, MANY_ROWS)]
    return out + list(PADDED)


def _kind(family, b):
    return family if family != "mixed" else ("ordinary", "floor", "saturated")[b % 3]


@functools.lru_cache(maxsize=None)
def bpr_case(B, d, family, seed=0):
    """Read-only f32 (u, p, n), a deterministic function of the key.  Every family starts from N(0, 0.3^2) rows; a row of
    `floor` or `saturated` is moved ALONG u by t (p - n), which moves x by t |p - n|^2 and nothing else, to its target:
    `floor` uniform in FLOOR_RANGE, `saturated` SATURATED_AT in turn; `mixed` deals ordinary / floor / saturated out to
    the rows in turn (its saturated rows take their targets in turn too)."""
    rng = np.random.default_rng([seed, B, d, FAMILIES.index(family)])
    u, p, n = ((rng.standard_normal((B, d)) * 0.3).astype(np.float32) for _ in range(3))
    u64 = _f64(u)
    diff = _f64(p) - _f64(n)
    x0 = (u64 * diff).sum(1)
    targets = rng.uniform(FLOOR_RANGE[0] + 0.25, FLOOR_RANGE[1] - 0.25, B)
    for b in range(B):
        kind = _kind(family, b)
        if kind == "ordinary":
            continue
        turn = b if family == "saturated" else b // 3
        target = targets[b] if kind == "floor" else SATURATED_AT[turn % 3]
        u64[b] += (target - x0[b]) / (diff[b] * diff[b]).sum() * diff[b]
    out = (u64.astype(np.float32), p, n)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def bpr_reference(B, d, family, gout):
    return bpr(*bpr_case(B, d, family), gout)


def all_bpr_cases():
    for B, d in bpr_shapes():
        for family in FAMILIES:
            yield B, d, family


# ---- L2 cases -------------------------------------------------------------------------------------------------------------
# Blocks of rows, (rows, cols).  The forward and backward kernels give a block one workgroup per 1024 elements, at most
# 1024 of them (kL2MaxWg): 8192 x 128 is the last size under the cap, 8193 x 128 the first whose workgroups walk on.
L2_CAP_ELEMS = 1024 * 1024
BLOCKS = ((1, 1), (1, 3), (5, 51), (1, 255), (1, 256), (1, 257), (1023, 1), (1024, 1), (1025, 1), (8192, 128), (8193, 128))
ZERO = "zero"             # an all-zero block of ZERO_SHAPE: zero norm, zero gradient
ZERO_SHAPE = (5, 64)
REG = 0.37


@functools.lru_cache(maxsize=None)
def block(key, seed=0):
    """the read-only f32 block of a key: (rows, cols), (rows, cols, i) for an i-th independent draw of the shape, or ZERO"""
    if key == ZERO:
        x = np.zeros(ZERO_SHAPE, dtype=np.float32)
    else:
        rng = np.random.default_rng([seed, 77] + list(key))
        x = (rng.standard_normal((key[0], key[1])) * 0.3).astype(np.float32)
    x.setflags(write=False)
    return x


# One call: its slots' block keys, in order; a key named twice is ONE tensor in two slots.  `route`: "launch" (1..4 device
# blocks: one launch each way), "five" (more than a launch takes: block by block), "mixed" (the slots listed in `cpu` are
# CPU tensors: block by block, the CPU ones by the torch expression).
L2_CALLS = tuple(dict(slots=(k,), route="launch", cpu=()) for k in BLOCKS + (ZERO,)) + (
    dict(slots=((5, 51), (1, 255)), route="launch", cpu=()),
    dict(slots=((1, 256), ZERO, (1, 257)), route="launch", cpu=()),
    dict(slots=((1023, 1), (1024, 1), (1025, 1), (1, 1)), route="launch", cpu=()),
    dict(slots=((8193, 128), (1, 3), (8192, 128), (5, 51)), route="launch", cpu=()),      # workgroups 1024.. and 2049..
    dict(slots=((5, 51), (1, 257), (5, 51)), route="launch", cpu=()),                     # one tensor, two slots
    dict(slots=((8193, 128), ZERO, (8193, 128), (1, 3)), route="launch", cpu=()),         # and past the cap
    dict(slots=((5, 51), ZERO, (1, 255), (1, 3), (1, 3)), route="five", cpu=()),
    dict(slots=((1025, 1), (5, 51), (1, 257)), route="mixed", cpu=(1,)),
)


@functools.lru_cache(maxsize=None)
def l2_reference(call_index, gout):
    call = L2_CALLS[call_index]
    return l2(REG, [block(k) for k in call["slots"]], gout)
