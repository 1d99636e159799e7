"""The table cross-entropy (csrc/contrastive.hip: ce_pass, ce_finish, ce_loss) against float64 per row: at every layout of
the pass-1 chunk schedule (chunks of two to four key tiles, where the running maximum rescales the sums; trailing empty
chunks; last chunks of one key), on inputs that raise the maximum at every tile or fix it in the first, with a dirty
caller-supplied workspace, labels outside the table, and loss scales 0, -1 and 1 / M^2.  DESIGN.md 4.20; the references,
the seeded cases and the measures are tests/table_ce_ref.py, their premises tests/test_table_ce_ref_cpu.py.

Bounds: loss <= 1e-5 relative; lse_m <= 1e-5 max(1, |lse_m|) per row; gradients <= 1e-4 per row
(row_errors, floor FLOOR_FRAC; FLOOR_FRAC_EXTREME for the extreme family).  Every test prints its figures."""
import ctypes as C

import pytest
import torch

from tests import table_ce_ref as R

pytestmark = pytest.mark.gpu


def _padded(d):
    return 64 if d <= 64 else 128


def _run(key, scale=1.0, ws=None):
    """one call on the case with a caller-supplied workspace -> dict(loss, gh, gt, lse, row_loss), the last two read back
    from the workspace (ws_carve: lse float32 (M), row_loss float64 (M)), and the workspace"""
    from selfrec_amd import _lib, ops
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    h, table, labels = R.case(key)
    M, N, D = len(h), len(table), _padded(h.shape[1])
    carve = R.ws_carve(M, N, D)
    assert int(_lib.load().srh_table_ce_ws_bytes(M, N, D)) == carve["total"]
    if ws is None:
        ws = torch.empty(carve["total"], dtype=torch.uint8, device=dev)
    assert ws.numel() >= carve["total"]                       # ... so ops uses this buffer and no other
    loss, gh, gt = ops.table_ce_fwd_bwd(h.to(dev), table.to(dev), labels.to(dev, torch.int32), scale, ws=ws)
    assert gh.shape == h.shape and gt.shape == table.shape and loss.dtype == torch.float64
    lse = ws[carve["lse"]:carve["lse"] + 4 * M].view(torch.float32).clone()
    row_loss = ws[carve["row_loss"]:carve["row_loss"] + 8 * M].view(torch.float64).clone()
    return dict(loss=loss.clone(), gh=gh.clone(), gt=gt.clone(), lse=lse, row_loss=row_loss), ws


def _check(name, got, key, scale=1.0):
    fig = R.figures(got, key, scale=scale)
    print(f"[{name}] " + "  ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    assert fig["loss"] <= R.LOSS_TOL, fig
    assert fig["lse"] <= R.LSE_TOL and fig["row"] <= R.LSE_TOL, fig
    assert fig["gh"] <= R.GRAD_TOL and fig["gt"] <= R.GRAD_TOL, fig
    return fig


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in ("loss", "gh", "gt", "lse", "row_loss"))


# ---- a. the existing shapes, per row ----------------------------------------------------------------------------------
@pytest.mark.parametrize("key", R.SHAPE_KEYS, ids=R.key_id)
def test_existing_shapes_per_row(key):
    M = key[1][0]
    for scale in (1.0, 1.0 / (M * M)):
        got, _ = _run(key, scale)
        assert torch.isfinite(got["gh"]).all() and torch.isfinite(got["gt"]).all()
        _check(f"{R.key_id(key)} scale {scale:.3g}", got, key, scale)


# ---- b. the chunk layouts in every input family -----------------------------------------------------------------------
@pytest.mark.parametrize("key", R.LAYOUT_KEYS, ids=R.key_id)
def test_chunk_layouts(key):
    got, _ = _run(key)
    assert torch.isfinite(got["loss"]).item() and torch.isfinite(got["gh"]).all() and torch.isfinite(got["gt"]).all()
    _check(R.key_id(key), got, key)


# ---- c. a dirty workspace ---------------------------------------------------------------------------------------------
def test_dirty_workspace_changes_nothing():
    """every partial that the finish reads was written by this call, the empty chunks' included: a workspace of NaN
    bytes, and the same one after a call of another shape has used it, give the bits of a fresh one"""
    key = ("layout",) + R.DIRTY
    assert R.LAYOUTS[R.DIRTY[0]]["shape"][:2] == (4097, 513) and R.LAYOUTS[R.DIRTY[0]]["empty"] == 3
    fresh, _ = _run(key)
    _check("dirty workspace, fresh", fresh, key)
    M, N, d = R.LAYOUTS[R.DIRTY[0]]["shape"]
    ws = torch.full((R.ws_carve(M, N, _padded(d))["total"],), 0xFF, dtype=torch.uint8, device="cuda:0")
    assert torch.isnan(ws[:4096].view(torch.float32)).all()
    first, ws = _run(key, ws=ws)
    assert _same(first, fresh)
    other = ("shape",) + R.DIRTY_OTHER
    got, ws2 = _run(other, ws=ws)
    assert ws2 is ws
    _check("dirty workspace, the call in between", got, other)
    second, _ = _run(key, ws=ws)
    assert _same(second, fresh)


def test_same_bits_twice():
    key = ("layout", 4, "staircase")
    assert R.LAYOUTS[4]["shape"] == (129, 21958, 64)
    a, _ = _run(key)
    b, _ = _run(key)
    assert _same(a, b)


# ---- d. labels outside the table --------------------------------------------------------------------------------------
def test_labels_outside_the_table():
    """labels -1 and N: the loss is NaN and so are the two rows' terms; every lse, gh of the other rows and all of gt stay
    inside the bounds against float64 with the two one-hots left out; gh of the two rows is sum_j P_mj t_j"""
    got, _ = _run(R.BAD_KEY)
    assert torch.isnan(got["loss"]).item()
    assert torch.isfinite(got["gh"]).all() and torch.isfinite(got["gt"]).all()
    bad = list(R.BAD_LABELS["rows"])
    assert torch.isnan(got["row_loss"][bad]).all() and int(torch.isnan(got["row_loss"]).sum()) == len(bad)
    fig = _check("labels outside the table", got, R.BAD_KEY)
    want = R.reference(R.BAD_KEY)["gh"][bad]
    two = float(R.row_errors(got["gh"][bad], want, 0.0).max())               # the two rows on their own scale
    print(f"[labels outside the table] gh of the two rows {two:.2e}")
    assert fig["loss"] == 0.0 and two <= R.GRAD_TOL


# ---- e. the loss scale ------------------------------------------------------------------------------------------------
def test_loss_scale():
    """loss_scale is a float32 that multiplies each output once, last: scale -1 negates every bit pattern, 1 / M^2 gives
    float32(1 / M^2) times the outputs of scale 1 to the bit, and 0 gives exact zeros -- no NaN from 0 * inf in the rows
    whose early tiles underflowed"""
    key = ("layout", 1, "staircase")
    M = R.LAYOUTS[1]["shape"][0]
    one, _ = _run(key, 1.0)
    _check("loss scale 1", one, key)
    neg, _ = _run(key, -1.0)
    assert torch.equal(neg["gh"], -one["gh"]) and torch.equal(neg["gt"], -one["gt"]) and torch.equal(neg["loss"], -one["loss"])
    k32 = torch.tensor(1.0 / (M * M), dtype=torch.float32, device="cuda:0")
    small, _ = _run(key, 1.0 / (M * M))
    assert torch.equal(small["gh"], k32 * one["gh"]) and torch.equal(small["gt"], k32 * one["gt"])
    assert torch.equal(small["loss"], k32.double() * one["loss"])
    _check("loss scale 1/M^2", small, key, float(k32))
    zero, _ = _run(key, 0.0)
    assert float(zero["loss"]) == 0.0 and not zero["gh"].any() and not zero["gt"].any()
    # the per-row terms do not depend on the scale
    for other in (neg, small, zero):
        assert torch.equal(other["lse"], one["lse"]) and torch.equal(other["row_loss"], one["row_loss"])


# ---- f. refusals ------------------------------------------------------------------------------------------------------
def test_refusals_touch_nothing():
    """a non-finite scale and M = 0 are refused (SRH_ERR_INVALID_ARG, -1) before any launch: outputs and workspace keep
    their bytes"""
    from selfrec_amd import _lib, ops
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    lib = _lib.load()
    h, t = torch.full((5, 64), 7.0, device=dev), torch.full((83, 64), 7.0, device=dev)
    lab = torch.zeros(5, dtype=torch.int32, device=dev)
    loss = torch.full((), 7.0, dtype=torch.float64, device=dev)
    gh, gt = torch.full_like(h, 7.0), torch.full_like(t, 7.0)
    ws = torch.full((int(lib.srh_table_ce_ws_bytes(5, 83, 64)),), 0x5A, dtype=torch.uint8, device=dev)
    assert lib.srh_table_ce_ws_bytes(0, 83, 64) == 0
    for M, scale, what in ((5, float("inf"), "scale"), (5, float("-inf"), "scale"), (5, float("nan"), "scale"), (0, 1.0, "M")):
        status = lib.srh_table_ce_fwd_bwd(h.data_ptr(), M, t.data_ptr(), 83, 64, lab.data_ptr(), C.c_float(scale),
                                          loss.data_ptr(), gh.data_ptr(), gt.data_ptr(), ws.data_ptr(), None)
        assert status == -1, (M, scale, status)
        with pytest.raises(ops.SelfrecHipError, match=r"\(-1\).*" + what):
            _lib.check(status, "srh_table_ce_fwd_bwd")
    torch.cuda.synchronize()
    assert float(loss) == 7.0 and bool((gh == 7.0).all()) and bool((gt == 7.0).all()) and bool((ws == 0x5A).all())
