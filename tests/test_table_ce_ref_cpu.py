"""The premises of tests/table_ce_ref.py, checked without a GPU: float32 torch meets half of every bound
on every case, the floor is the smallest that it meets, chunk_plan gives each layout case the layout its entry claims, the
staircase rows raise (or fix) the running maximum where the case says, the spike keys and the labels fall where the case
says, and ce_carve's restatement adds up to srh_table_ce_ws_bytes."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import bert4rec_ref
from tests import table_ce_ref as R


# ---- float32 torch on every case, and the floor -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _f32_figures():
    """{key: {floor: figures of float32 torch against float64}}"""
    out = {}
    for key in R.ALL_KEYS:
        got = R.f32_torch(key)
        out[key] = {f: R.figures(got, key, floor_frac=f) for f in R.FLOORS}
    return out


@pytest.mark.parametrize("key", R.ALL_KEYS, ids=R.key_id)
def test_float32_torch_meets_half_of_each_bound(key):
    """a case that float32 arithmetic alone cannot serve would test the number format, not the kernel"""
    fig = _f32_figures()[key][R.floor_of(key)]
    print(R.key_id(key), "  ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    ref = R.reference(key)
    assert torch.isfinite(ref["gh"]).all() and torch.isfinite(ref["gt"]).all() and torch.isfinite(ref["lse"]).all()
    assert fig["loss"] <= R.LOSS_TOL / 2 and fig["lse"] <= R.LSE_TOL / 2 and fig["row"] <= R.LSE_TOL / 2, fig
    assert fig["gh"] <= R.GRAD_TOL / 2 and fig["gt"] <= R.GRAD_TOL / 2, fig
    if key[0] != "shape":                                          # the new families keep |logit| <= about 130
        h, table, _ = R.case(key)
        assert float((h.double() @ table.double().T).abs().max()) <= 135.0


def test_floor_frac_is_the_smallest_that_float32_torch_meets():
    """each of the two floors is the smallest of FLOORS at which float32 torch stays within GRAD_TOL / 2 per row on every
    case of its group: the extreme family of bert4rec_ref.ce_case, and everything else"""
    for name, floor, keys in (("extreme", R.FLOOR_FRAC_EXTREME, [k for k in R.ALL_KEYS if k[2] == "extreme"]),
                              ("others", R.FLOOR_FRAC, [k for k in R.ALL_KEYS if k[2] != "extreme"])):
        assert keys and all(R.floor_of(k) == floor for k in keys)
        worst = {f: {n: max(_f32_figures()[k][f][n] for k in keys) for n in ("loss", "lse", "row", "gh", "gt")}
                 for f in R.FLOORS}
        for f in R.FLOORS:
            print(f"float32 torch against float64, {name}, floor {f:g}: "
                  + "  ".join(f"{k} {v:.2e}" for k, v in worst[f].items()))
        passing = [f for f in R.FLOORS if max(worst[f]["gh"], worst[f]["gt"]) <= R.GRAD_TOL / 2]
        assert passing and floor == min(passing), (name, worst)


def test_the_per_row_measure_sees_what_the_tensor_wide_one_hides():
    """the issue's premise: at (300, 5000) the smallest row of gt is about 1e-3 of the tensor's largest magnitude, so
    1e-4 of the largest allows errors of several percent on such a row"""
    gt = R.reference(("shape", (300, 5000, 64), "ordinary"))["gt"]
    rows = gt.abs().amax(dim=1)
    assert float(rows.min() / rows.max()) < 5e-3
    assert float((rows < 1e-2 * rows.max()).double().mean()) > 0.3


def test_reference_pieces_agree():
    """the per-row terms sum to table_ce_grads' loss; the gradients equal autograd's on the float64 loss; with labels
    outside the table the two one-hots are left out and nothing else changes"""
    for key in (("shape", (93, 82, 64), "extreme"), ("layout", 0, "spike")):
        h, table, labels = R.case(key)
        ref = R.reference(key)
        assert abs(float(ref["row_loss"].sum()) - ref["loss"]) <= 1e-12 * abs(ref["loss"])
        h_, t_ = h.double().requires_grad_(True), table.double().requires_grad_(True)
        torch.nn.functional.cross_entropy(h_ @ t_.T, labels, reduction="sum").backward()
        assert float((ref["gh"] - h_.grad).abs().max()) <= 1e-12 * float(h_.grad.abs().max())
        assert float((ref["gt"] - t_.grad).abs().max()) <= 1e-12 * float(t_.grad.abs().max())
    h, table, labels = R.case(R.BAD_KEY)
    ref = R.reference(R.BAD_KEY)
    s = h.double() @ table.double().T
    p = torch.softmax(s, dim=1)
    ok = (labels >= 0) & (labels < len(table))
    onehot = torch.zeros_like(p)
    onehot[R.nz(ok), labels[ok]] = 1.0
    assert torch.allclose(ref["gh"], (p - onehot) @ table.double(), rtol=0, atol=1e-14)
    assert torch.allclose(ref["gt"], (p - onehot).T @ h.double(), rtol=0, atol=1e-12)
    assert torch.allclose(ref["gh"][~ok], p[~ok] @ table.double(), rtol=0, atol=1e-14)          # sum_j P_mj t_j
    assert ref["loss"] != ref["loss"] and torch.isnan(ref["row_loss"][~ok]).all() and torch.isfinite(ref["row_loss"][ok]).all()


# ---- the layouts ----------------------------------------------------------------------------------------------------------
def test_existing_shapes_have_one_tile_per_chunk():
    """the gap this file closes: no shape of bert4rec_ref.CE_SHAPES has a chunk of two tiles or an empty chunk"""
    for M, N, _ in bert4rec_ref.CE_SHAPES:
        p = R.chunk_plan(M, N)
        assert p["chunk_len"] == 64 and p["empty"] == 0


@pytest.mark.parametrize("i", range(len(R.LAYOUTS)), ids=lambda i: "M%d_N%d_d%d" % R.LAYOUTS[i]["shape"])
def test_chunk_plan_gives_the_layout_the_case_claims(i):
    lay = R.LAYOUTS[i]
    M, N, d = lay["shape"]
    p = R.chunk_plan(M, N)
    got = dict(chunks=p["chunks"], tiles=p["chunk_len"] // 64, live=p["live"], empty=p["empty"], last_keys=p["last_keys"])
    assert got == {k: lay[k] for k in got}, got
    assert lay["tiles"] >= 2                                        # every layout case has the rescale inside a chunk
    assert max(x["shape"][0] * x["shape"][1] for x in R.LAYOUTS) == 16385 * 500


def test_layouts_cover_the_edges():
    L = {x["shape"]: x for x in R.LAYOUTS}
    assert L[(8193, 300, 64)]["empty"] == 1 and L[(4097, 513, 64)]["last_keys"] == 1 and L[(4097, 513, 64)]["empty"] == 3
    assert L[(16385, 500, 128)]["tiles"] == 4 and 500 % 64 != 0
    assert 16321 == 255 * 64 + 1 and 100 % 16 == 4
    assert L[(129, 21958, 64)]["tiles"] == 3 and L[(1, 32833, 64)]["last_keys"] == 64 + 1
    assert {x["shape"][2] for x in R.LAYOUTS} == {64, 100, 128}
    assert {x["tiles"] for x in R.LAYOUTS} == {2, 3, 4}


# ---- the staircase --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.LAYOUTS)), ids=lambda i: "M%d_N%d_d%d" % R.LAYOUTS[i]["shape"])
def test_staircase_rows_raise_or_fix_the_running_maximum(i):
    M, N, d = R.LAYOUTS[i]["shape"]
    h, table, _ = R.case(("layout", i, "staircase"))
    p = R.chunk_plan(M, N)
    T = p["chunk_len"] // 64
    kind = torch.tensor(R.STAIR_H, dtype=torch.float64)[torch.arange(M) % 7]
    assert torch.equal(h[:, 0].double(), kind)
    if M >= 64:                                                      # every 64-row workgroup holds rows of each kind
        for r0 in range(0, M - 6, 64):
            assert set(kind[r0:r0 + 64].tolist()) == set(R.STAIR_H) or M - r0 < 7
    s = h.double() @ table.double().T
    pad = torch.full((M, p["chunks"] * p["chunk_len"] - N), float("-inf"), dtype=torch.float64)
    tile_max = torch.cat([s, pad], dim=1).reshape(M, p["chunks"], T, 64).amax(dim=3)       # -inf: a tile with no key
    flat = tile_max.reshape(M, -1)[:, :-(-N // 64)]                                        # the tiles that hold a key
    run = torch.cummax(flat, dim=1).values
    up = kind > 0
    assert up.any()
    # a rising row: the maximum over tiles 0..i strictly increases with i, through every tile of every chunk
    assert (flat[up][:, 1:] > run[up][:, :-1]).all()
    # ... by a factor that float32 tells from 1 and from 0: alpha = exp(m - m_new) of two neighbouring tiles
    step = (flat[up][:, :-1] - flat[up][:, 1:]).float()
    alpha = torch.exp(step)
    assert (alpha < 1.0).all() and (alpha > 0.0).all()
    gentle = kind == 8.0
    if gentle.any():
        a8 = torch.exp((flat[gentle][:, :-1] - flat[gentle][:, 1:]).float())
        assert float(a8.min()) > 1e-2                               # at +8 the earlier sums survive the rescale
    steep = kind == 100.0
    if steep.any() and p["live"] > 1:
        # at +100 the first chunk's partial weighs exp(-30) or less in the merge: below what float32 keeps of the row sum
        first = tile_max[steep][:, 0].amax(dim=1)
        assert float((first - flat[steep].amax(dim=1)).max()) < -30.0
    down = kind < 0
    if down.any():
        # a falling row: the maximum stands in the first tile; its later tiles weigh less and less
        assert (s[down].argmax(dim=1) < 64).all()
        assert (flat[down][:, 1:] < flat[down][:, :1]).all()
        if (kind == -100.0).any():
            far = kind == -100.0
            assert float((flat[far][:, -1] - flat[far][:, 0]).max()) < -30.0


# ---- the spikes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.LAYOUTS)), ids=lambda i: "M%d_N%d_d%d" % R.LAYOUTS[i]["shape"])
def test_spike_keys_fall_where_the_case_says(i):
    lay = R.LAYOUTS[i]
    M, N, d = lay["shape"]
    h, table, _ = R.case(("layout", i, "spike"))
    keys = R.spike_keys(N)
    assert len(keys) == 7 and torch.equal(R.nz(table[:, 0]), torch.tensor(keys))
    assert torch.equal(h[:, 0], torch.tensor(R.SPIKE_H)[torch.arange(M) % 3])
    place = {j: R.key_place(j, M, N) for j in keys}
    assert place[0] == (0, 0) and place[63] == (0, 0)                      # the first tile
    assert place[64] == (0, 1) and place[127] == (0, 1)                    # the second tile of a chunk
    assert place[128] == ((1, 0) if lay["tiles"] == 2 else (0, 2))         # the next chunk's first tile, or a third tile
    last = place[N - 1]
    assert last[0] == lay["live"] - 1 and last[1] == (lay["last_keys"] - 1) // 64        # the last live chunk's last tile
    if lay["live"] >= 3:
        assert 0 < place[N // 2][0] < lay["live"] - 1                      # a middle chunk
    # a +60 row's largest logits are the spike keys', all of them within the other columns' noise of each other
    s = h.double() @ table.double().T
    hot = R.nz(h[:, 0] == 60.0)
    if len(hot):
        top = s[hot].topk(7, dim=1).indices.sort(dim=1).values
        assert (top == torch.tensor(keys)).all()
    cold = R.nz(h[:, 0] == -60.0)
    if len(cold):
        assert not torch.isin(s[cold].argmax(dim=1), torch.tensor(keys)).any()


def test_hand_checked_spike_places():
    assert {j: R.key_place(j, 4097, 513) for j in R.spike_keys(513)} == {
        0: (0, 0), 63: (0, 0), 64: (0, 1), 127: (0, 1), 128: (1, 0), 256: (2, 0), 512: (4, 0)}
    assert {j: R.key_place(j, 129, 21958) for j in R.spike_keys(21958)} == {
        0: (0, 0), 63: (0, 0), 64: (0, 1), 127: (0, 1), 128: (0, 2), 10979: (57, 0), 21957: (114, 1)}


# ---- the labels -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", R.LAYOUT_KEYS, ids=R.key_id)
def test_labels_are_where_the_case_says(key):
    h, table, labels = R.case(key)
    M, N = len(h), len(table)
    assert labels.dtype == torch.int64 and int(labels.min()) >= 0 and int(labels.max()) == N - 1
    assert int(labels[-1]) == N - 1
    named = set(labels.tolist())
    assert N - len(named) >= N / 3                                          # a third of the keys is named by nobody
    if M >= 6:
        assert 0 in named and N // 2 in named and N // 2 in R.spike_keys(N)
        tail = (N - 1) // 64 * 64
        assert any(tail <= j < N for j in named) and N % 64 != 0            # a key of the last partial tile
        assert len(named) < M                                               # labels repeat
    else:
        assert M == 1 and N - 1 in R.spike_keys(N) and N % 64 == 1          # one row: the key alone in the last tile


def test_labels_outside_the_table_are_where_the_case_says():
    h, table, labels = R.case(R.BAD_KEY)
    M, N, d = R.BAD_LABELS["shape"]
    assert (len(h), len(table), h.shape[1]) == (M, N, d) == (17, 130, 64)
    assert int(labels[5]) == -1 and int(labels[11]) == N
    rest = torch.ones(M, dtype=torch.bool)
    rest[[5, 11]] = False
    assert int(labels[rest].min()) >= 0 and int(labels[rest].max()) == N - 1
    # the untouched cases keep their labels inside
    for key in R.SHAPE_KEYS + R.LAYOUT_KEYS:
        _, t, lab = R.case(key)
        assert 0 <= int(lab.min()) and int(lab.max()) < len(t)


def test_extreme_groups_are_the_planted_rows():
    for shape in bert4rec_ref.CE_SHAPES:
        M, N, _ = shape
        gh, gt = R.row_groups(("shape", shape, "extreme"))
        assert gh[0].tolist() == [r for r in R.EXTREME_ROWS if r < M] and gt[0].tolist() == [0]
        assert sum(len(g) for g in gh) == M and sum(len(g) for g in gt) == N
        h, table, _ = R.case(("shape", shape, "extreme"))
        assert float(h[gh[0], 0].abs().min()) >= 60.0 and float(table[0, 0]) == 2.0
        if M >= 5:
            assert float(h[gh[1], 0].abs().max()) < 6.0
        whole_h, whole_t = R.row_groups(("shape", shape, "ordinary"))
        assert len(whole_h) == 1 and len(whole_h[0]) == M and len(whole_t) == 1 and len(whole_t[0]) == N


# ---- the workspace --------------------------------------------------------------------------------------------------------
def test_carve_restatement_adds_up_to_ws_bytes():
    from selfrec_amd import _lib
    shapes = [x["shape"] for x in R.LAYOUTS] + list(bert4rec_ref.CE_SHAPES) + [R.BAD_LABELS["shape"]]
    for M, N, d in shapes:
        D = 64 if d <= 64 else 128
        c = R.ws_carve(M, N, D)
        offs = [c[k] for k in ("part_o", "part_rs", "part_m", "lse", "row_loss", "total")]
        assert offs[0] == 0 and offs == sorted(offs) and all(o % 256 == 0 for o in offs)
        assert c["total"] - c["row_loss"] >= 8 * M and c["row_loss"] - c["lse"] >= 4 * M
        if os.path.exists(_lib.LIB_PATH):                                   # built: the library's own total
            assert int(_lib.load().srh_table_ce_ws_bytes(M, N, D)) == c["total"], (M, N, D)
    # the dirty-workspace test's other call fits into the workspace of the call it disturbs
    M, N, d = R.LAYOUTS[R.DIRTY[0]]["shape"]
    assert (M, N) == (4097, 513)
    assert R.ws_carve(*R.DIRTY_OTHER[0])["total"] <= R.ws_carve(M, N, d)["total"]
    assert np.prod(R.DIRTY_OTHER[0][:2]) != M * N
