"""srh_tower_fwd_f32, srh_tower_bwd_f32 and srh_rows_segment_sum_f32 (csrc/ssl4rec.hip) at their edges, against the float64
restatement of tests/tower_ref.py (premises: tests/test_tower_ref_cpu.py).

The grid: n in ROWS (every 16-row wave, 64-row workgroup and 256-row chunk edge, 513 = two chunks and a 1-row tail) x the
weight families init / hot (saturated tanh) / dead (few units alive, exact-zero biases, units dead on every row) x the
routes no mask / injected / drawn mask at mask_row0 in {0, n // 3, n - 1}, one row of every n >= 3 with an id outside the
table.  The kernel's ReLU pattern (saved hidden > 0) may differ from float64's only inside relu_band and is never alive at an
exact zero; everything else is compared with float64 AT THE KERNEL'S PATTERN: y <= 1e-5 and each gradient <= 1e-4 of the
tensor's largest magnitude, dX, the table gradient and the rows of dW1 / dW2 <= 1e-4 per row (row_errors, FLOOR_FRAC).

A foreign id reads a zero row and reaches no table row.  d_gx there is the gradient w.r.t. that zero row, (dZ1 W1) m, which is
not zero (include/selfrec_hip.h): it is held to float64 like any other row, its effective input must be exact zeros whether or
not the row is masked, and the table gradient must equal, bit for bit, the segment-sum restatement over the kernel's own d_gx
with the foreign segment skipped, with exact zeros in every row no id names.

The bit-for-bit comparisons of the library with itself (drawn against injected, mask_row0 = n, save=False, repeats) are marked
selfcheck."""
import numpy as np
import pytest
import torch

from tests import ssl4rec_ref
from tests import tower_ref as T

pytestmark = pytest.mark.gpu
DEV = "cuda"


def bits(t):
    t = t.detach().cpu().contiguous() if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def dev_weights(c):
    return [t.to(DEV) for t in c["w"]]


def mask_args(c, kind, row0):
    """the keyword arguments of ops.tower_fwd for a route"""
    if kind == "none":
        return dict(mask_row0=None)
    if kind == "injected":
        return dict(mask_row0=row0, mask=torch.from_numpy(T.route_keep(c["n"], row0).astype(np.uint8)).to(DEV), drop_p=T.DROP_P)
    seed, ctr = T.rng_args(c["n"], row0)
    return dict(mask_row0=row0, drop_p=T.DROP_P, rng_seed=seed, rng_counter=ctr)


def run_route(c, kind, row0):
    """the kernels' dict(y, saved, gx, gw1, gb1, gw2, gb2, gt) of a route: ops.tower_fwd / ops.tower_bwd for y, the saved
    tensors, dX and the weight gradients; TowerFn for the table gradient (and y and the weight gradients once more)"""
    from selfrec_amd import ops
    w = dev_weights(c)
    table = c["table"].to(DEV)
    idx = None if c["ids"] is None else c["ids"].to(DEV)
    gy = c["gy"].to(DEV)
    kw = mask_args(c, kind, row0)
    y, saved = ops.tower_fwd(table, idx, *w, **kw)
    gx, gw1, gb1, gw2, gb2 = ops.tower_bwd(saved, y, gy, *w, mask_row0=kw["mask_row0"], drop_p=kw.get("drop_p", 0.0))
    plan = None if idx is None else ops.scatter_plan(c["ids"].numpy(), table.device)
    tab = table.clone().requires_grad_(True)
    ws = [t.clone().requires_grad_(True) for t in w]
    y_fn = ops.TowerFn.apply(tab, *ws, idx, plan, kw["mask_row0"], kw.get("mask"), kw.get("drop_p", 0.0),
                             kw.get("rng_seed", 0), kw.get("rng_counter", 0), None)
    y_fn.backward(gy)
    torch.cuda.synchronize()
    return dict(y=y, saved=saved, gx=gx, gw1=gw1, gb1=gb1, gw2=gw2, gb2=gb2, gt=tab.grad, plan=plan,
                fn=dict(y=y_fn.detach(), gw1=ws[0].grad, gb1=ws[1].grad, gw2=ws[2].grad, gb2=ws[3].grad))


def check_route(c, kind, row0, got, tag):
    """every assertion of section (a) on one route; returns the figures"""
    n, f = c["n"], c["family"]
    x, hidden, keep = got["saved"]
    # the effective input, bit for bit; the drawn mask, bit for bit
    assert same_bits(x, T.effective_input_f32(c, row0)), f"{tag}: effective input"
    if c["foreign"] is not None:
        assert not bool(x[c["foreign"]].any()), f"{tag}: the foreign row read something"
    if kind == "none":
        assert keep is None
    else:
        assert np.array_equal(keep.cpu().numpy().astype(bool), T.route_keep(n, row0)), f"{tag}: keep mask"
    # the pattern
    pattern = (hidden > 0).cpu()
    f64 = T.tower_math(c, row0, pattern=pattern)
    band = T.relu_band(f64["x"], c["w"][0], c["w"][1])
    share, inside, alive_at_zero = T.flips(pattern, f64["z"], band)
    assert inside <= 1.0, f"{tag}: a unit outside the band decided differently from float64 ({inside:.3g} x the band)"
    assert alive_at_zero == 0, f"{tag}: {alive_at_zero} units alive at a pre-activation of exactly 0"
    # against float64 at the kernel's pattern
    figs = T.figures({k: got[k] for k in ("y",) + T.GRADS}, f64)
    fn = {"fn_" + k: T.rel_max(v, f64[k]) for k, v in got["fn"].items()}
    print(f"{tag}: {T.show(figs)} flips={share:.1e} ({inside:.2f} of the band) TowerFn: " +
          " ".join(f"{k[3:]}={v:.1e}" for k, v in fn.items()))
    for k, v in figs.items():
        assert v <= T.BOUNDS[k], f"{tag}: {k} = {v:.3g} > {T.BOUNDS[k]}"
    for k, v in fn.items():
        assert v <= T.BOUNDS[k[3:]], f"{tag}: TowerFn's {k[3:]} = {v:.3g}"
    # exact zeros
    if f == "dead":
        dead = torch.from_numpy(T.ALWAYS_DEAD)
        assert not bool(got["gw1"].cpu()[dead].any()) and not bool(got["gb1"].cpu()[dead].any()), f"{tag}: always-dead units"
    gt = got["gt"].cpu()
    if c["ids"] is not None:
        ids = c["ids"].numpy()
        unnamed = np.setdiff1d(np.arange(T.N_TABLE), ids)
        assert len(unnamed) >= T.N_TABLE - T.ID_HI
        assert not bool(gt[torch.from_numpy(unnamed)].any()), f"{tag}: a table row no id names received something"
        # nothing arrives from the foreign row, and the rest arrives in ascending row order: the restatement over the
        # kernel's own dX (TowerFn's launch repeats the direct call's bits)
        plan = tuple(a.cpu().numpy() for a in got["plan"])
        want = T.segment_sum_f32(got["gx"].cpu().numpy(), plan, np.zeros((T.N_TABLE, T.D_IN), dtype=np.float32))
        assert same_bits(gt, want), f"{tag}: table gradient against the segment-sum restatement"
    return figs


@pytest.mark.parametrize("family", T.FAMILIES)
@pytest.mark.parametrize("n", T.ROWS)
def test_tower_grid_matches_float64(n, family):
    torch.cuda.set_device(0)
    c = T.case(n, family)
    for kind, row0 in T.routes(n):
        tag = f"n={n} {family} {kind}" + ("" if row0 is None else f"@{row0}")
        check_route(c, kind, row0, run_route(c, kind, row0), tag)


@pytest.mark.parametrize("family", T.FAMILIES)
@pytest.mark.parametrize("n", T.NONE_ROWS)
def test_full_table_pass_matches_float64(n, family):
    """idx=None, evaluation's route: the table itself is the batch and gt is gx"""
    torch.cuda.set_device(0)
    c = T.case(n, family, gathered=False)
    for kind, row0 in (("none", None), ("drawn", n // 3)):
        tag = f"full table n={n} {family} {kind}"
        got = run_route(c, kind, row0)
        check_route(c, kind, row0, got, tag)
        assert same_bits(got["gt"], got["gx"]), f"{tag}: without ids the table gradient is dX"


@pytest.mark.parametrize("n", [17, 65, 257])
def test_drawn_mask_at_the_carry_matches_the_host(n):
    """saved[2] against ssl4rec_ref.dropout_keep at counters that cross 2^32, at every mask_row0 of the grid"""
    from selfrec_amd import ops
    torch.cuda.set_device(0)
    c = T.case(n, "init")
    for row0 in sorted({0, n // 3, n - 1}):
        seed, ctr = T.rng_args(n, row0)
        assert ctr < 2 ** 32 <= ctr + (n - row0) and seed >> 32
        _, saved = ops.tower_fwd(c["table"].to(DEV), c["ids"].to(DEV), *dev_weights(c), mask_row0=row0, drop_p=T.DROP_P,
                                 rng_seed=seed, rng_counter=ctr)
        keep = saved[2].cpu().numpy()
        want = ssl4rec_ref.dropout_keep(seed, ctr, n - row0, T.DROP_P)
        assert keep.dtype == np.uint8 and keep.shape == want.shape and set(np.unique(keep).tolist()) <= {0, 1}
        assert np.array_equal(keep.astype(bool), want), (n, row0)
        print(f"n={n} mask_row0={row0}: {keep.size} keep bits equal, kept share {keep.mean():.3f}")


# ---- the segment sum on its own ----------------------------------------------------------------------------------------
def _segment_setup(d):
    from .test_gpu_batch import SENTINEL, base_of
    p = T.segment_problem(d)
    want64 = T.segment_sum_f64(p["x"], p["plan"], p["n_table"])
    init = base_of(want64)
    other = np.setdiff1d(np.arange(p["n_table"]), p["named"])
    init[other] = SENTINEL
    return p, want64, init, other


@pytest.mark.parametrize("d", T.SEG_WIDTHS)
def test_segment_sum_matches_the_restatement(d):
    from selfrec_amd import ops
    torch.cuda.set_device(0)
    p, want64, init, other = _segment_setup(d)
    plan = tuple(torch.from_numpy(a).to(DEV) for a in p["plan"])
    out = torch.from_numpy(init).to(DEV)
    ret = ops.rows_segment_sum(torch.from_numpy(p["x"]).to(DEV), plan, out)
    torch.cuda.synchronize()
    assert ret is out
    got = out.cpu().numpy()
    want = T.segment_sum_f32(p["x"], p["plan"], init)
    assert np.array_equal(got[other].view(np.int32), init[other].view(np.int32)), "a row no segment names was written"
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), "not the float32 restatement's bits"
    # the restatement tied to the truth: what was added, per row, on the named rows (the long segment among them)
    added = np.zeros_like(want64)
    added[p["named"]] = got[p["named"]].astype(np.float64) - init[p["named"]].astype(np.float64)
    err = T.row_errors(added, want64, 0.0)
    print(f"segment sum d={d}: bits equal; against float64 worst row {float(err.max()):.2e}, the 1000-row segment "
          f"{float(err[T.SEG_LONG_ROW]):.2e}")
    assert float(err[T.SEG_LONG_ROW]) <= 1e-5 and float(err.max()) <= 1e-5


def test_segment_sum_without_segments_touches_nothing():
    from selfrec_amd import ops
    torch.cuda.set_device(0)
    p, _, init, _ = _segment_setup(65)
    order = torch.from_numpy(p["plan"][0]).to(DEV)
    empty = (order, torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV))
    out = torch.from_numpy(init).to(DEV)
    ops.rows_segment_sum(torch.from_numpy(p["x"]).to(DEV), empty, out)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.int32), init.view(np.int32))


# ---- the library against itself ----------------------------------------------------------------------------------------
@pytest.mark.selfcheck
@pytest.mark.parametrize("family", T.FAMILIES)
@pytest.mark.parametrize("n", [17, 65, 257, 513])
def test_drawn_route_has_the_bits_of_the_injected_route(n, family):
    torch.cuda.set_device(0)
    c = T.case(n, family)
    for row0 in sorted({0, n // 3, n - 1}):
        a, b = run_route(c, "injected", row0), run_route(c, "drawn", row0)
        for k in ("y",) + T.GRADS:
            assert same_bits(a[k], b[k]), (n, family, row0, k)
        for k in a["fn"]:
            assert same_bits(a["fn"][k], b["fn"][k]) and same_bits(a["fn"][k], a[k]), (n, family, row0, "TowerFn", k)
        assert same_bits(a["saved"][0], b["saved"][0]) and same_bits(a["saved"][1], b["saved"][1])
        assert torch.equal(a["saved"][2], b["saved"][2])


@pytest.mark.selfcheck
@pytest.mark.parametrize("n", [1, 65, 513])
def test_mask_row0_n_and_save_false_change_no_bit(n):
    from selfrec_amd import ops
    torch.cuda.set_device(0)
    c = T.case(n, "hot")
    table, idx, w = c["table"].to(DEV), c["ids"].to(DEV), dev_weights(c)
    y0, s0 = ops.tower_fwd(table, idx, *w)
    # mask_row0 = n with a drop probability: nothing is masked
    y1, s1 = ops.tower_fwd(table, idx, *w, mask_row0=n, drop_p=T.DROP_P, rng_seed=T.rng_args(n, 0)[0], rng_counter=5)
    assert same_bits(y0, y1) and same_bits(s0[0], s1[0]) and same_bits(s0[1], s1[1]) and s1[2] is None
    g0 = ops.tower_bwd(s0, y0, c["gy"].to(DEV), *w)
    g1 = ops.tower_bwd(s1, y1, c["gy"].to(DEV), *w, mask_row0=n, drop_p=T.DROP_P)
    assert all(same_bits(a, b) for a, b in zip(g0, g1))
    # save=False: the same y, nothing saved -- unmasked, injected and drawn
    for kind, row0 in T.routes(n)[:3]:
        kw = mask_args(c, kind, row0)
        ya, sa = ops.tower_fwd(table, idx, *w, **kw)
        yb, sb = ops.tower_fwd(table, idx, *w, save=False, **kw)
        assert sb is None and sa is not None and same_bits(ya, yb), (n, kind, row0)


@pytest.mark.selfcheck
def test_same_bits_twice():
    from selfrec_amd import ops
    torch.cuda.set_device(0)
    c = T.case(513, "hot")
    a, b = run_route(c, "drawn", 171), run_route(c, "drawn", 171)
    for k in ("y",) + T.GRADS:
        assert same_bits(a[k], b[k]), k
    assert all(same_bits(u, v) for u, v in zip(a["saved"][:2], b["saved"][:2])) and torch.equal(a["saved"][2], b["saved"][2])
    p, _, init, _ = _segment_setup(200)
    plan = tuple(torch.from_numpy(t).to(DEV) for t in p["plan"])
    outs = [ops.rows_segment_sum(torch.from_numpy(p["x"]).to(DEV), plan, torch.from_numpy(init).to(DEV)) for _ in range(2)]
    assert same_bits(outs[0], outs[1])
