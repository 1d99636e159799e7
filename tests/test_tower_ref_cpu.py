"""The premises of tests/tower_ref.py, checked without a GPU: plain float32 torch stays within half of every
bound of tests/test_gpu_tower_edges.py on every case, few units sit so close to zero that float32 may decide them
differently, the planted properties of the cases hold, the host's drawn mask crosses the 2^32 carry as the counter RNG says,
each planted defect exceeds the bound it is meant to trip ten times over, and the float32 segment-sum restatement is
index_add_ to rounding."""
import numpy as np
import pytest
import torch

from tests import counter_rng, ssl4rec_ref
from tests import tower_ref as T

GRID = [(n, f) for f in T.FAMILIES for n in T.ROWS]


def _cases():
    """every (case, row0) of the GPU grid once: the two masked routes share their mask, so they are one problem here"""
    for n, f in GRID:
        c = T.case(n, f)
        for kind, row0 in T.routes(n):
            if kind != "drawn":
                yield c, row0
    for n in T.NONE_ROWS:
        for f in T.FAMILIES:
            c = T.case(n, f, gathered=False)
            yield c, None
            yield c, n // 3


def test_f32_torch_stays_within_half_of_every_bound():
    worst = {}
    for c, row0 in _cases():
        f32 = T.tower_math(c, row0, dtype=torch.float32)
        f64 = T.tower_math(c, row0, pattern=f32["pattern"])
        for k, v in T.figures(f32, f64).items():
            key = (c["family"], k)
            if v > worst.get(key, (-1.0,))[0]:
                worst[key] = (v, c["n"], row0, c["ids"] is None)
    for f in T.FAMILIES:
        print(f"f32 torch against float64, {f}: " + " ".join(f"{k}={worst[(f, k)][0]:.2e}(n={worst[(f, k)][1]})"
                                                                 for k in T.BOUNDS))
    for (f, k), (v, n, row0, full) in worst.items():
        assert v <= 0.5 * T.BOUNDS[k], (f, k, v, n, row0, full)


def test_few_units_sit_inside_the_relu_band():
    flipped = 0
    for f in T.FAMILIES:
        worst, total = 0.0, 0
        for c, row0 in _cases():
            if c["family"] != f:
                continue
            f64 = T.tower_math(c, row0)
            band = T.relu_band(f64["x"], c["w"][0], c["w"][1])
            z = f64["z"]
            near = (z.abs() <= band) & (z != 0)            # planted exact zeros are not near misses: they are decided
            worst = max(worst, float(near.double().mean()))
            f32 = T.tower_math(c, row0, dtype=torch.float32)
            share, inside, alive_at_zero = T.flips(f32["pattern"], z, band)
            flipped += int(round(share * z.numel()))
            total += z.numel()
            assert inside <= 1.0, (f, c["n"], row0, inside)      # float32 flips only inside the band
            assert alive_at_zero == 0
        print(f"near-zero share, {f}: worst case {worst:.2e} (bound 1e-3) over {total} units")
        assert worst <= 1e-3
    print(f"float32 torch decides {flipped} units differently from float64, all inside the band")


def test_planted_properties_hold():
    sat, live = [], []
    for n, f in GRID:
        c = T.case(n, f)
        assert int(c["ids"].max()) < T.ID_HI or n >= 3
        if n >= 3:
            bad = c["ids"][c["foreign"]]
            assert bad == T.FOREIGN[f] and not 0 <= int(bad) < T.N_TABLE
            assert int(((c["ids"] < 0) | (c["ids"] >= T.N_TABLE)).sum()) == 1
        for kind, row0 in T.routes(n):
            if kind == "drawn":
                continue
            r = T.tower_math(c, row0)
            if f == "hot":
                share = float((r["y"].abs() > 0.9999).double().mean())
                assert share >= 0.05, (n, row0, share)
                sat.append(share)
            if f == "dead":
                alive = r["pattern"].double().mean()
                assert float(alive) < 0.10, (n, row0, float(alive))
                live.append(float(alive))
                assert not bool(r["pattern"][:, torch.from_numpy(T.ALWAYS_DEAD)].any())
                assert bool((c["w"][1][torch.from_numpy(T.ZERO_BIAS)] == 0).all())
                if n >= 3:
                    zf = r["z"][c["foreign"]]
                    assert bool((zf[torch.from_numpy(T.ZERO_BIAS)] == 0).all()) and bool((r["x"][c["foreign"]] == 0).all())
                    # at the other rows the zero-bias units are ordinary: alive on some, dead on others
                    assert 0 < int(r["pattern"][:, torch.from_numpy(T.ZERO_BIAS)].sum())
            if row0 is not None:
                seed, ctr = T.rng_args(n, row0)
                assert seed >> 32 != 0
                assert ctr < 2 ** 32 <= ctr + (n - row0)
                if n - row0 >= 2:
                    assert ctr + (n - row0) - 1 >= 2 ** 32          # rows on both sides of the carry
                keep = T.route_keep(n, row0)
                assert keep.shape == (n - row0, T.D_IN)
    print(f"hot: |y| > 0.9999 on {min(sat):.3f} .. {max(sat):.3f} of the outputs; dead: {min(live):.3f} .. {max(live):.3f} of the "
          f"units alive")
    # the routes name a single masked row, the two-view call and an ordinary split
    assert T.routes(513) == [("none", None), ("injected", 0), ("drawn", 0), ("injected", 171), ("drawn", 171),
                             ("injected", 512), ("drawn", 512)]
    assert all(T.ROWS[-1] > k * T.ROW_CHUNK for k in (1, 2)) and (T.ROWS[-1] - 1) % T.ROW_CHUNK == 0


def test_host_mask_crosses_the_carry_as_the_counter_rng_says():
    for n in (17, 65, 257, 513):
        for row0 in sorted({0, n // 3, n - 1}):
            seed, ctr = T.rng_args(n, row0)
            got = ssl4rec_ref.dropout_keep(seed, ctr, n - row0, T.DROP_P)
            for r in range(n - row0):
                words = np.stack([counter_rng.rng4(ctr + r, s, seed) for s in range(T.D_IN // 4)]).reshape(-1)
                assert np.array_equal(got[r], counter_rng.u01(words) >= np.float32(T.DROP_P)), (n, row0, r)
    seed, ctr = T.rng_args(257, 0)
    both = ssl4rec_ref.dropout_keep(seed, ctr, 257, T.DROP_P)
    wrapped = ssl4rec_ref.dropout_keep(seed, ctr & 0xFFFFFFFF, 257, T.DROP_P)         # the same: ctr < 2^32
    assert np.array_equal(both, wrapped)
    # a counter truncated to 32 bits draws other rows past the carry
    lo = 2 ** 32 - ctr
    trunc = np.concatenate([both[:lo], ssl4rec_ref.dropout_keep(seed, 0, 257 - lo, T.DROP_P)])
    assert not np.array_equal(both, trunc)
    assert 0.85 < both.mean() < 0.95


def _defect_ratio(defect, keys):
    """the largest figure / bound over the cases, for the float32 restatement with the defect against float64 at the
    defective run's own pattern, on the quantities the defect is meant to trip"""
    best = (0.0, None)
    for c, row0 in _cases():
        if c["ids"] is None:
            continue
        bad = T.tower_math(c, row0, dtype=torch.float32, defect=defect)
        f64 = T.tower_math(c, row0, pattern=bad["pattern"])
        figs = {k: v for k, v in T.figures(bad, f64).items() if k in keys}
        ratio = T.worst_ratio(figs)
        if ratio > best[0]:
            best = (ratio, (c["family"], c["n"], row0))
    return best


@pytest.mark.parametrize("defect,keys", [
    ("relu_ge", ("gx", "gx_row", "gb1")),
    ("tail_chunk", ("gw1", "gw1_row", "gb1", "gw2", "gw2_row", "gb2")),
    ("mask_scale_last", ("gx", "gx_row", "gt", "gt_row")),
    ("foreign_row0", ("y",)),
])
def test_planted_defects_trip_their_bounds(defect, keys):
    ratio, where = _defect_ratio(defect, keys)
    print(f"defect {defect}: {ratio:.3g} x its bound at (family, n, mask_row0) = {where}")
    assert ratio >= 10.0
    if defect == "tail_chunk":
        for k in ("gw1", "gb1", "gw2", "gb2"):                   # each of the four reductions on its own
            r, w = _defect_ratio(defect, (k,))
            print(f"  {k}: {r:.3g} x at {w}")
            assert r >= 10.0


def test_relu_ge_is_alive_at_an_exact_zero():
    """the other check the >= defect trips: a unit alive where float64's pre-activation is exactly 0"""
    c = T.case(17, "dead")
    r = T.tower_math(c, None)
    assert int(((r["z"] >= 0) & (r["z"] == 0)).sum()) == len(T.ZERO_BIAS)


@pytest.mark.parametrize("d", T.SEG_WIDTHS)
def test_segment_sum_restatement(d):
    p = T.segment_problem(d)
    order, seg_start, seg_row = p["plan"]
    assert sorted(np.diff(seg_start)[:6].tolist()) == sorted(T.SEG_LENGTHS) and len(order) == len(p["x"])
    assert int(((order < 0) | (order >= len(p["x"]))).sum()) == 4 and set(seg_row[6:].tolist()) == {-1, p["n_table"]}
    want = T.segment_sum_f64(p["x"], p["plan"], p["n_table"])
    zero = np.zeros((p["n_table"], d), dtype=np.float32)
    got = T.segment_sum_f32(p["x"], p["plan"], zero)
    err = T.row_errors(got, want, 0.0)
    print(f"segment sum d={d}: f32 restatement against float64, worst row {float(err.max()):.2e}")
    assert float(err.max()) <= 1e-5
    other = np.setdiff1d(np.arange(p["n_table"]), p["named"])
    assert not want[other].any() and not got[other].any() and want[p["named"]].any(1).all()
    # an ordinary plan (ops.scatter_plan_host's layout, restated): a stable sort of ids
    ids = np.random.RandomState(d).randint(0, p["n_table"], len(p["x"]))
    o = np.argsort(ids, kind="stable")
    first = np.flatnonzero(np.r_[True, ids[o][1:] != ids[o][:-1]])
    plan = (o, np.r_[first, len(ids)], ids[o][first])
    ref = torch.zeros(p["n_table"], d, dtype=torch.float64).index_add_(0, torch.from_numpy(ids), torch.from_numpy(p["x"]).double())
    assert float(T.row_errors(T.segment_sum_f32(p["x"], plan, zero), ref, 0.0).max()) <= 1e-5
    # the order is observable: summing the long segment backwards changes bits
    rev = order.copy()
    a, b = seg_start[5], seg_start[6]
    rev[a:b] = order[a:b][::-1]
    assert not np.array_equal(T.segment_sum_f32(p["x"], (rev, seg_start, seg_row), zero)[T.SEG_LONG_ROW], got[T.SEG_LONG_ROW])
    # a store in place of the add: ten times the bound and more on a preloaded table
    base = np.full_like(zero, 0.25)
    added = T.segment_sum_f32(p["x"], p["plan"], base).astype(np.float64) - base
    stored = T.segment_sum_f32(p["x"], p["plan"], base, store=True).astype(np.float64) - base
    ok, bad = float(T.row_errors(added, want, 0.0).max()), float(T.row_errors(stored, want, 0.0).max())
    print(f"  store instead of add: {bad / 1e-5:.3g} x the bound (added: {ok:.2e})")
    assert ok <= 1e-5 and bad >= 10 * 1e-5
