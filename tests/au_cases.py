"""Seeded cases for the DirectAU loss kernels (csrc/au.hip) -- TEST INFRASTRUCTURE ONLY.  A case is a dict: name, x, y
(float32 CPU, un-normalised), t, w = (w_align, w_ux, w_uy), cancel_x / cancel_y (bool masks of the rows measured against
au_ref.cancel_scales, or None).  tests/test_au_ref_cpu.py checks their premises; tests/test_gpu_au.py runs the kernels."""
import torch

GAMMA = 2.0
W_MODEL = (1.0, GAMMA / 2, GAMMA / 2)
WEIGHTS = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), W_MODEL)

TILE_N = (2, 3, 15, 16, 17, 63, 64, 65, 127, 128, 129, 257)
TILE_D = (2, 50, 64, 100, 128)
T_EDGES = ((65, 64, 0.5), (65, 64, 8.0), (129, 128, 0.5), (129, 128, 8.0))
# the chunk layouts beyond those the tile shapes reach (au_ref.chunk_plan): 16 chunks of 128 keys of which 7 are empty and
# the 9th holds one row; 8 full chunks of 4 tiles; 8 chunks of 320 keys, one empty, the 7th of 129 keys; 4 chunks of 1088
CHUNK_SHAPES = ((1025, 64), (2048, 64), (2049, 64), (4100, 128))
LARGE_SHAPE = (16384, 64)        # one chunk of 256 tiles; on the device only, against the closed form
DEGENERATE_SHAPES = ((65, 64), (129, 128))
REPEAT_SHAPES = ((2049, 64), (129, 128))


def batch_rows(n, d, seed):
    """x, y as a batch gathers them: rows of two small tables drawn with repetition (a batch repeats users, so
    bit-identical rows within x and within y are the normal case)"""
    g = torch.Generator().manual_seed(seed)
    users = torch.randn(max(3, (2 * n) // 3), d, generator=g) * 0.1
    items = torch.randn(max(3, (3 * n) // 4), d, generator=g) * 0.1
    x = users[torch.randint(0, len(users), (n,), generator=g)]
    y = items[torch.randint(0, len(items), (n,), generator=g)]
    if n <= 3:                      # (keep the rows distinct: two equal rows of two have no gradient at all)
        x, y = users[:n].clone(), items[:n].clone()
    return x.contiguous(), y.contiguous()


def plain_case(n, d, t=2.0, w=W_MODEL, seed=None):
    x, y = batch_rows(n, d, 1000 + 7 * n + d if seed is None else seed)
    return dict(name=f"n{n}-d{d}-t{t}", x=x, y=y, t=t, w=w, cancel_x=None, cancel_y=None)


def tile_cases(n):
    return [plain_case(n, d) for d in TILE_D]


def t_cases():
    return [plain_case(n, d, t) for n, d, t in T_EDGES]


def chunk_cases():
    return [plain_case(n, d) for n, d in CHUNK_SHAPES]


DEG = dict(dup_x=(3, 7), dup_y=(4, 9), equal=11, zero_x=5, tiny_y=20, near_x=30)


def degenerate_case(n, d):
    """duplicated rows within x and within y; x_i = y_i; a zero row in x; a row of 1e-20 entries in y; a row of x of norm
    8e-13 and the LAST row of y (alone in its tile) of norm 8e-13, just below the clamp: their normalised rows have norm
    0.8, so the projection of the unclamped backward, wrongly applied, would take 0.64 of the parallel part off.  Cancelling
    rows: `equal` on both sides, and the partners of the zero and the 1e-20 row."""
    c = DEG
    g = torch.Generator().manual_seed(2000 + n + d)
    x = torch.randn(n, d, generator=g) * 0.1
    y = torch.randn(n, d, generator=g) * 0.1 + 0.5 * x
    x[c["dup_x"][1]] = x[c["dup_x"][0]]
    y[c["dup_y"][1]] = y[c["dup_y"][0]]
    y[c["equal"]] = x[c["equal"]]
    x[c["zero_x"]] = 0.0
    y[c["tiny_y"]] = 1e-20
    x[c["near_x"]] *= 8e-13 / float(x[c["near_x"]].double().norm())
    y[n - 1] *= 8e-13 / float(y[n - 1].double().norm())
    cx, cy = torch.zeros(n, dtype=torch.bool), torch.zeros(n, dtype=torch.bool)
    cx[[c["equal"], c["tiny_y"]]] = True
    cy[[c["equal"], c["zero_x"]]] = True
    return dict(name=f"degenerate-n{n}-d{d}", x=x, y=y, t=2.0, w=W_MODEL, cancel_x=cx, cancel_y=cy)


def identical_case(n, d):
    """all rows of x identical: U(x) = 0 exactly in the reference and dU/dx = 0 (every row cancels); y ordinary"""
    g = torch.Generator().manual_seed(2100 + n + d)
    x = (torch.randn(1, d, generator=g) * 0.1).repeat(n, 1)
    y = torch.randn(n, d, generator=g) * 0.1
    return dict(name=f"identical-n{n}-d{d}", x=x, y=y, t=2.0, w=W_MODEL, cancel_x=torch.ones(n, dtype=torch.bool),
                cancel_y=None)


def antipodal_case(n, d):
    """two antipodal clusters: rows +-v with 1 % noise, so w_ij is about 1 inside a cluster and exp(-4 t) across"""
    g = torch.Generator().manual_seed(2200 + n + d)
    v = torch.randn(1, d, generator=g)
    sign = torch.where(torch.arange(n) % 2 == 0, 1.0, -1.0)[:, None]
    x = 0.1 * sign * v + 0.001 * torch.randn(n, d, generator=g)
    y = -0.2 * sign * v + 0.002 * torch.randn(n, d, generator=g)
    return dict(name=f"antipodal-n{n}-d{d}", x=x, y=y, t=2.0, w=W_MODEL, cancel_x=None, cancel_y=None)


def degenerate_cases():
    return [f(n, d) for n, d in DEGENERATE_SHAPES for f in (degenerate_case, identical_case, antipodal_case)]


def weight_cases():
    return [plain_case(65, 64, w=w, seed=3000 + i) for i, w in enumerate(WEIGHTS)]


def cpu_cases():
    """every case the GPU tests run, but LARGE_SHAPE (its pair list is a gigabyte in float64)"""
    out = [c for n in TILE_N for c in tile_cases(n)]
    return out + t_cases() + chunk_cases() + degenerate_cases() + weight_cases()
