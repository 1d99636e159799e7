"""MHCN's kernels at their edges, against the float64 restatement tests/mhcn_ref.py: the channel mix with equal and with
saturated scores, the MIM loss with identity shuffles (every difference exactly 0), with differences near +-40 (where
-log(sigmoid) overflows in float32) and with zero rows of edge; empty inputs, refused shapes, and repeatability."""
import numpy as np
import pytest
import torch

from selfrec_amd import ops
from tests import mhcn_cases
from tests.mhcn_cases import GRAD_BOUND, LOSS_BOUND
from tests.test_gpu_mhcn import check_mim, check_mix, dev, host, run_mim, run_mix

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", [c for c in mhcn_cases.MIX_CASES if c[1] != "normal"], ids=mhcn_cases.mix_id)
def test_chan_mix_families(case):
    c = mhcn_cases.mix_case(case)
    got = run_mix(c)
    check_mix(case, got)
    if case[1] == "equal":          # equal scores in any precision: the same bits in all three, a third each
        assert np.array_equal(got["s"][:, 0], got["s"][:, 1]) and np.array_equal(got["s"][:, 0], got["s"][:, 2])
        assert np.abs(got["s"] - 1.0 / 3.0).max() <= 1e-7
    else:                           # the odd rows are saturated: one score is 1, the others vanish
        sat = np.sort(got["s"][1::2], axis=1)
        assert (sat[:, 2] == 1.0).all() and sat[:, 1].max() < 1e-12


@pytest.mark.parametrize("case", [c for c in mhcn_cases.MIM_CASES if c[1] != "normal"], ids=mhcn_cases.mim_id)
def test_mim_families(case):
    c = mhcn_cases.mim_case(case)
    got = run_mim(c)
    check_mim(case, got)
    (n, d), fam = case
    if fam == "identity":           # every local and global difference is exactly 0: 3 n log 2, and zero gradients
        assert abs(got[0] / (3 * n * np.log(2.0)) - 1) <= LOSS_BOUND
        assert not got[1].any() and not got[2].any()


def test_empty_inputs_return_empty_results():
    z = lambda *shape: torch.empty(shape, device="cuda")  # noqa: E731
    w, b = dev(mhcn_cases.gate_case((17, 64, 1))["w"]), dev(mhcn_cases.gate_case((17, 64, 1))["b"])
    assert ops.gate_fwd(z(0, 64), w, b).shape == (1, 0, 64)
    gx, gw, gb = ops.gate_bwd(z(0, 64), w, b, z(1, 0, 64))
    assert gx.shape == (0, 64) and not host(gw).any() and not host(gb).any()
    q = dev(np.ones(64, dtype=np.float32))
    out, s = ops.chan_mix_fwd(z(0, 64), z(0, 64), z(0, 64), q, None, 0.0)
    assert out.shape == (0, 64) and s.shape == (0, 3)
    g1, g2, g3, gx, gq = ops.chan_mix_bwd(z(0, 64), z(0, 64), z(0, 64), q, s, z(0, 64))
    assert g1.shape == (0, 64) and gx is None and not host(gq).any()
    none, cols = torch.empty(0, dtype=torch.int32, device="cuda"), torch.arange(64, dtype=torch.int32, device="cuda")
    loss, gem, gedge = ops.mim_fwd_bwd(z(0, 64), z(0, 64), none, none, none, cols, cols)
    assert float(loss) == 0.0 and gem.shape == (0, 64) and gedge.shape == (0, 64)


def test_unsupported_shapes_raise_the_library_status():
    x = torch.zeros((4, 130), device="cuda")
    with pytest.raises(ops.SelfrecHipError, match="unsupported"):
        ops.gate_fwd(x, torch.zeros((1, 130, 130), device="cuda"), torch.zeros((1, 130), device="cuda"))
    with pytest.raises(ops.SelfrecHipError, match="unsupported"):
        ops.gate_bwd(x, torch.zeros((1, 130, 130), device="cuda"), torch.zeros((1, 130), device="cuda"),
                     torch.zeros((1, 4, 130), device="cuda"))
    with pytest.raises(ops.SelfrecHipError, match="unsupported"):
        ops.chan_mix_fwd(x, x, x, torch.zeros(130, device="cuda"))
    with pytest.raises(ops.SelfrecHipError, match="unsupported"):
        ops.chan_mix_bwd(x, x, x, torch.zeros(130, device="cuda"), torch.zeros((4, 3), device="cuda"), x)
    rows, cols = torch.arange(4, dtype=torch.int32, device="cuda"), torch.arange(130, dtype=torch.int32, device="cuda")
    with pytest.raises(ops.SelfrecHipError, match="unsupported"):
        ops.mim_fwd_bwd(x, x, rows, rows, rows, cols, cols)
    c = mhcn_cases.gate_case((17, 64, 1))
    with pytest.raises(ops.SelfrecHipError, match="gates unsupported"):      # five gates in one call
        ops.gate_fwd(dev(c["x"]), dev(np.repeat(c["w"], 5, axis=0)), dev(np.repeat(c["b"], 5, axis=0)))


# ---- repeatability: a self-comparison, collected last ------------------------------------------------------------------
@pytest.mark.selfcheck
def test_the_three_ops_return_the_same_bits_twice():
    g = mhcn_cases.gate_case((513, 64, 1))
    args = [dev(g[k]) for k in ("x", "w", "b", "gy")]
    a, b = ops.gate_bwd(*args), ops.gate_bwd(*args)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert torch.equal(ops.gate_fwd(*args[:3]), ops.gate_fwd(*args[:3]))
    m = mhcn_cases.mix_case(((257, 64), "normal", True))
    a, b = run_mix(m), run_mix(m)
    assert np.array_equal(a["out"], b["out"]) and np.array_equal(a["gq"], b["gq"]) and np.array_equal(a["gx"], b["gx"])
    assert all(np.array_equal(x, y) for x, y in zip(a["ge"], b["ge"]))
    for case in (((1030, 64), "normal"), ((257, 128), "large")):
        c = mhcn_cases.mim_case(case)
        a, b = run_mim(c), run_mim(c)
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert GRAD_BOUND > 0
