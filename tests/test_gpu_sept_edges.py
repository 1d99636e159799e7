"""srh_tri_nd_fwd_bwd and the row normalise (csrc/sept.hip) at their edges, against the float64 restatement of
tests/sept_ref.py (premises: tests/test_sept_cpu.py).

The grid: sept_cases.EDGE_SHAPES (every row-tile, 16-key sub-tile, mask-word and pass-1 chunk edge, both widths, the three
zero-padded widths, k = 1, 10 and 32) x the input families normal / scaled (row norms over six decades) / clamped (a zero
row and a row below the clamp in every matrix) / peaked (views near the aug rows).  One kernel call per (shape, family).

    ids        the restatement's set on every non-ambiguous (pair, row), inside the 1e-4 band elsewhere; best first
               wherever a rank's float64 key stands clear of both neighbours; the planted rows and keys on their own
    loss       each of the three <= LOSS_BOUND against the restatement AT THE KERNEL'S IDS
    gradients  every row of dF, dS, dR and dA <= GRAD_BOUND of that row's own largest entry, no floor; a clamped row
               against its own g * 1e6
    peaked     max(the standing bound, 4 x what sept_ref.tri_nd_f32 -- the same expression in plain float32 -- loses on the
               same case and ids): the loss and the row gradients are small differences of large terms there
    scaled     against normal: the same ids, the same losses, each gradient row times its 10**u the normal row

The comparisons of the library with itself (a poisoned, a zeroed and a reused workspace against a fresh one, bit for bit)
are marked selfcheck."""
import functools

import numpy as np
import pytest
import torch

from selfrec_amd import _lib, ops
from tests import sept_cases, sept_ref
from tests.sept_cases import AMBIGUOUS_GAP, EDGE_SHAPES, FAMILIES, GRAD_BOUND, LOSS_BOUND, TAU

pytestmark = pytest.mark.gpu
MATRICES = ("friend", "sharing", "rec", "aug")
YARD_FACTOR = 4.0         # a different summation order than the yardstick's; a wrong or missing term moves a row by 1e-2


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype)


def run_tri_nd(mats, k, ws=None):
    loss, grads, pos = ops.tri_nd_fwd_bwd([dev(m) for m in mats[:3]], dev(mats[3]), k, TAU, ws=ws)
    torch.cuda.synchronize()
    return loss.cpu().numpy(), [g.cpu().numpy() for g in grads], pos.cpu().numpy()


_RUNS = {}


def kernel_run(case):
    """one kernel call per (shape, family), shared by the tests below"""
    if case not in _RUNS:
        _RUNS[case] = run_tri_nd(sept_cases.edge_case(*case)["mats"], case[0][2])
    return _RUNS[case]


@functools.lru_cache(maxsize=None)
def measure(case):
    """the kernel against the restatement at the kernel's ids: loss_err (3), row_err (4 x (n,)), and the bounds they are
    held to -- the standing ones, or on `peaked` the larger of them and YARD_FACTOR x the float32 yardstick's own error on
    this case and these ids (the loss: the largest of the three views'; a gradient: that matrix's worst row)"""
    (n, d, k, _seed), fam = case
    c = sept_cases.edge_case(*case)
    loss, grads, pos = kernel_run(case)
    ref = sept_ref.tri_nd(*c["mats"], k, TAU, pos=pos)
    out = dict(loss_err=np.abs(loss / ref["loss"] - 1.0), row_err=[sept_ref.row_errors(g, w) for g, w in zip(grads, ref["grads"])],
               loss_bound=LOSS_BOUND, grad_bound=[GRAD_BOUND] * 4, want=ref["grads"], want_loss=ref["loss"])
    if fam == "peaked":
        y = sept_ref.tri_nd_f32(*c["mats"], k, TAU, pos)
        yl = float(np.abs(y["loss"].astype(np.float64) / ref["loss"] - 1.0).max())
        yr = [float(sept_ref.row_errors(g, w).max()) for g, w in zip(y["grads"], ref["grads"])]
        out.update(yard_loss=yl, yard_row=yr, loss_bound=max(LOSS_BOUND, YARD_FACTOR * yl),
                   grad_bound=[max(GRAD_BOUND, YARD_FACTOR * r) for r in yr])
    return out


# ---- ids ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sept_cases.edge_cases(), ids=sept_cases.edge_id)
def test_ids_sets_and_order(case):
    """non-ambiguous (pair, row): the restatement's id set exactly; ambiguous: only indices whose float64 key lies within
    1e-4 relative of the k-th key may differ.  Order: pos[v, i, p] is the restatement's p-th id wherever the float64 key of
    rank p differs from those of ranks p - 1 and p + 1 by more than the same band.  clamped: the planted view rows (as
    row i) and the planted aug rows (as key j) are held on their own, so they cannot hide in the allowance."""
    (n, d, k, _seed), fam = case
    c = sept_cases.edge_case(*case)
    _, _, pos = kernel_run(case)
    assert pos.shape == (3, n, k) and pos.dtype == np.int32 and pos.min() >= 0 and pos.max() < n
    ref, top = c["ref"], c["top"]
    assert (np.sort(pos, axis=2)[:, :, 1:] != np.sort(pos, axis=2)[:, :, :-1]).all()           # k distinct ids per row
    swapped = np.zeros((3, n), dtype=bool)
    for v in range(3):
        for i in range(n):
            got, want = set(pos[v, i].tolist()), set(ref["pos"][v, i].tolist())
            if got == want:
                continue
            assert c["amb"][v, i], f"view {v} row {i}: {sorted(got ^ want)} differ on a clear cut (gap {ref['gap'][v, i]:.3e})"
            key = ref["key"][v, i]
            kth = top[v, i, k - 1]
            assert all(abs(key[j] - kth) <= AMBIGUOUS_GAP * kth for j in got ^ want), (v, i)
            swapped[v, i] = True
    # best first: rank p is clear when its key stands off both neighbours (the (k + 1)-th key is the last one's lower neighbour)
    off = top[:, :, :-1] - top[:, :, 1:] > AMBIGUOUS_GAP * top[:, :, :-1]                       # (3, n, k): rank p against p + 1
    clear = off.copy()
    clear[:, :, 1:] &= off[:, :, :-1]
    assert np.array_equal(pos[clear], ref["pos"][clear])
    print(f"{sept_cases.edge_id(case)}: {int(swapped.sum())} of {3 * n} (pair, row)s chose inside the ambiguous band; "
          f"{float(clear.mean()):.4f} of the ranks held to their order")
    if fam != "clamped":
        return
    planted = sept_cases.planted_rows(n)
    rows = sorted(r for pair in planted[:3] for r in pair)
    for v in range(3):
        for i in rows:
            if not c["amb"][v, i]:
                assert set(pos[v, i].tolist()) == set(ref["pos"][v, i].tolist()), f"planted row {i} of view {v}"
    kth = top[:, :, k - 1]
    for j in planted[3]:
        differ = (pos == j).any(axis=2) != (ref["pos"] == j).any(axis=2)
        near = np.abs(ref["key"][:, :, j] - kth) <= AMBIGUOUS_GAP * kth
        assert not (differ & ~near).any(), f"planted key {j}"
    print(f"{sept_cases.edge_id(case)}: planted rows {rows}: {int(c['amb'][:, rows].sum())} ambiguous, "
          f"{int(swapped[:, rows].sum())} chose inside the band")


# ---- loss and gradients ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sept_cases.edge_cases(), ids=sept_cases.edge_id)
def test_loss_and_gradients_per_row(case):
    """against the restatement evaluated at the kernel's own ids; every gradient row relative to its own largest entry"""
    (n, d, k, _seed), fam = case
    assert n > k
    m = measure(case)
    _, grads, _ = kernel_run(case)
    name = sept_cases.edge_id(case)
    if fam == "peaked":
        print(f"{name} yardstick: loss {m['yard_loss']:.3e} rows {' '.join('%.3e' % r for r in m['yard_row'])} -> bounds "
              f"loss {m['loss_bound']:.3e} rows {' '.join('%.3e' % b for b in m['grad_bound'])}")
    for v in range(3):
        print(f"{name} loss[{v}]: {m['loss_err'][v]:.3e}")
    for mat, g, err in zip(MATRICES, grads, m["row_err"]):
        assert g.shape == (n, d) and err.shape == (n,)
        print(f"{name} d{mat}: worst row {int(err.argmax())} {float(err.max()):.3e}")
    assert np.isfinite(m["loss_err"]).all() and float(m["loss_err"].max()) <= m["loss_bound"]
    for mat, err, bound in zip(MATRICES, m["row_err"], m["grad_bound"]):
        assert np.isfinite(err).all() and float(err.max()) <= bound, (mat, int(err.argmax()))


@pytest.mark.parametrize("fam", FAMILIES)
def test_family_worst_errors(fam):
    """the largest loss and row error of a family over every shape (the figures of DESIGN.md 4.18), held to the family's
    bound once more"""
    worst_loss, worst_row = 0.0, 0.0
    for shape in EDGE_SHAPES:
        m = measure((shape, fam))
        worst_loss = max(worst_loss, float(m["loss_err"].max()))
        worst_row = max(worst_row, max(float(e.max()) for e in m["row_err"]))
        assert float(m["loss_err"].max()) <= m["loss_bound"]
        assert all(float(e.max()) <= b for e, b in zip(m["row_err"], m["grad_bound"]))
    print(f"{fam}: worst loss error {worst_loss:.3e}, worst row error {worst_row:.3e}")


def test_clamped_rows_carry_the_unprojected_gradient():
    """a planted row's gradient is g * 1e6, not the projection: its largest entry is 1e5 times the matrix's largest
    unclamped one or more, and it was measured above like any other row (this names the rows, so that a change of the
    planting cannot quietly leave the clamped branch unrun)"""
    shape = EDGE_SHAPES[0]
    n = shape[0]
    m = measure((shape, "clamped"))
    _, grads, _ = kernel_run((shape, "clamped"))
    for g, want, (zero, tiny), err in zip(grads, m["want"], sept_cases.planted_rows(n), m["row_err"]):
        rest = np.delete(np.abs(want).max(axis=1), (zero, tiny)).max()
        for r in (zero, tiny):
            assert np.abs(want[r]).max() >= 1e5 * rest and np.abs(g[r]).max() >= 1e5 * rest and err[r] <= GRAD_BOUND


# ---- scale invariance -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=lambda s: "n%d_d%d_k%d_s%d" % s)
def test_scaled_agrees_with_normal(shape):
    """rows times 10**u change no normalised row: the id sets agree on every (pair, row) that is clear in both families,
    the losses agree to LOSS_BOUND and every gradient row of `scaled`, times its 10**u, is the `normal` row to 2 GRAD_BOUND
    of that row.  Nothing bit for bit: the scaling itself rounds.  Where an ambiguous row chose differently in the two runs,
    its own view-gradient row is left out, and that view's loss and dA (which see every row's ids) are held to the
    restatement of the normal inputs at the scaled run's ids instead."""
    n, d, k, seed = shape
    cn, cs = sept_cases.edge_case(shape, "normal"), sept_cases.edge_case(shape, "scaled")
    ln, gn, pn = kernel_run((shape, "normal"))
    ls, gs, ps = kernel_run((shape, "scaled"))
    same = (np.sort(pn, axis=2) == np.sort(ps, axis=2)).all(axis=2)
    assert same[~cn["amb"] & ~cs["amb"]].all()
    sc = sept_cases.row_scales(n, seed)
    ref = None if same.all() else sept_ref.tri_nd(*cn["mats"], k, TAU, pos=ps)
    worst = 0.0
    for v in range(3):
        back = gs[v].astype(np.float64) * sc[v][:, None]
        err = sept_ref.row_errors(back[same[v]], gn[v][same[v]])
        worst = max(worst, float(err.max()))
        assert float(err.max()) <= 2 * GRAD_BOUND, (MATRICES[v], int(err.argmax()))
        want_loss = ln[v] if same[v].all() else ref["loss"][v]
        assert abs(ls[v] / want_loss - 1.0) <= LOSS_BOUND, v
    err = sept_ref.row_errors(gs[3].astype(np.float64) * sc[3][:, None], gn[3] if ref is None else ref["grads"][3])
    assert float(err.max()) <= 2 * GRAD_BOUND, ("aug", int(err.argmax()))
    print(f"n{n}_d{d}_k{k}: {int((~same).sum())} (pair, row)s chose differently; worst scaled-back row "
          f"{max(worst, float(err.max())):.3e}")


# ---- rows_l2norm through one layer at a padded width ------------------------------------------------------------------------
def test_norm_prop_fn_against_the_restatement_at_d100():
    """l2_normalize(A x) at a width that is no multiple of 64 (lanes 36 ... 63 of the second quarter masked), forward and
    backward through the explicit transpose; an empty row of A is the clamped zero row"""
    import scipy.sparse as sp
    from selfrec_amd.base.torch_interface import TorchGraphInterface
    rng = np.random.default_rng(5)
    n, d = 70, 100
    dense = ((rng.random((n, n)) < 0.1) * rng.random((n, n))).astype(np.float32)
    dense[5] = 0
    a = sp.csr_matrix(dense)
    x, g = rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((n, d)).astype(np.float32)
    leaf = dev(x).requires_grad_(True)
    y = ops.NormPropFn.apply(TorchGraphInterface.convert_sparse_mat_to_tensor(a), leaf)
    y.backward(dev(g))
    a64 = a.astype(np.float64)
    out, inv, clamped = sept_ref.l2norm(a64 @ x.astype(np.float64))
    want_g = a64.T @ sept_ref.l2norm_bwd(g, out, inv, clamped)
    assert clamped[5] and clamped.sum() == 1
    got = y.detach().cpu().numpy()
    assert np.array_equal(got[5], np.zeros(d, dtype=np.float32))
    assert float(sept_ref.row_errors(got, out).max()) <= 1e-5
    # a row of the input gradient sums the 1e6-scaled clamped row and ordinary ones: relative to the matrix's largest
    assert float(np.abs(leaf.grad.cpu().numpy() - want_g).max()) <= GRAD_BOUND * float(np.abs(want_g).max())


# ---- the workspace: poisoned, zeroed, reused -- comparisons of the library with itself, collected last ------------------------
def same_results(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))


def ws_bytes(shape):
    n, d, k, _seed = shape
    need = int(_lib.load().srh_tri_nd_ws_bytes(n, d, k))
    assert need > 0
    return need


@pytest.mark.selfcheck
@pytest.mark.parametrize("shape", [(97, 64, 10, 0), (833, 128, 10, 0), (65, 64, 32, 0)], ids=lambda s: "n%d_d%d_k%d_s%d" % s)
def test_workspace_contents_do_not_matter(shape):
    """a caller's workspace of exactly the queried size, every byte 0xFF (each float and double a NaN, each mask bit set),
    then every byte zero: loss, gradients and ids equal a fresh workspace's bit for bit -- no cell is read before it is
    written (the mask words are cleared before the OR, the six empty pass-1 chunks of n = 833 publish zeros)"""
    assert shape in EDGE_SHAPES
    mats = sept_cases.edge_case(shape, "normal")["mats"]
    fresh = run_tri_nd(mats, shape[2])
    assert np.isfinite(fresh[0]).all() and all(np.isfinite(g).all() for g in fresh[1])
    need = ws_bytes(shape)
    for fill in (0xFF, 0x00):
        ws = torch.full((need,), fill, dtype=torch.uint8, device="cuda")
        assert same_results(run_tri_nd(mats, shape[2], ws=ws), fresh), hex(fill)


@pytest.mark.selfcheck
def test_workspace_of_a_larger_call_serves_a_smaller_one():
    """one workspace sized for n = 833, used for that call and then for n = 131 (other chunk counts, word counts and
    offsets inside the same bytes), as training reuses it"""
    big, small = (833, 128, 10, 0), (131, 128, 10, 0)
    ws = torch.empty(ws_bytes(big), dtype=torch.uint8, device="cuda")
    assert ws_bytes(small) < ws.numel()
    for shape in (big, small):
        mats = sept_cases.edge_case(shape, "normal")["mats"]
        assert same_results(run_tri_nd(mats, shape[2], ws=ws), run_tri_nd(mats, shape[2])), shape
