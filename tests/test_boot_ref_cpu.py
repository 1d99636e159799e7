"""The premises of tests/boot_ref.py and tests/boot_cases.py and the host side of the bootstrap loss kernels
(include/selfrec_hip.h (a-23), csrc/bootstrap.hip): no GPU needed."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from selfrec_amd import _lib
from tests import boot_cases as K
from tests import boot_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return K.cpu_cases()


@pytest.fixture(scope="module")
def refs(cases):
    """float64 autograd on the reference's expression, once per case"""
    return [R.reference(c) for c in cases]


@pytest.fixture(scope="module")
def closed(cases):
    return [R.closed_form(c) for c in cases]


def _worst_row(c, got, want, cf, floor):
    """the worst row of both input gradients of a case under grad_errors"""
    worst = 0.0
    for s in R.SIDES:
        cancel = c["cancel_" + s]
        scales = None if cancel is None else R.cancel_scales(c, s, cf)
        worst = max(worst, float(R.grad_errors(got["gx_" + s], want["gx_" + s], cf["clamped_" + s], cancel, scales, floor).max()))
    return worst


def test_closed_form_is_the_reference_expression(cases, refs, closed):
    worst = 0.0
    for c, want, got in zip(cases, refs, closed):
        assert R.value_error(got["loss"], want["loss"]) <= 1e-12, c["name"]
        assert all(R.value_error(got["parts"][k], want["parts"][k]) <= 1e-12 for k in (0, 1)), c["name"]
        e = _worst_row(c, got, want, got, 1e-3)
        ew, eb = R.weight_errors(want["gw"], want["gb"], got)
        worst = max(worst, e, ew, eb)
        assert e <= 1e-12 and ew <= 1e-12 and eb <= 1e-12, (c["name"], e, ew, eb)
        for s in R.SIDES:
            assert torch.equal(got["T_" + s], want["T_" + s]), c["name"]
    print("closed form against float64 autograd, worst figure:", worst)


def test_case_premises(cases, refs, closed):
    by_name = {c["name"]: (c, r, f) for c, r, f in zip(cases, refs, closed)}
    seen = set()
    for c, want, cf in zip(cases, refs, closed):
        assert all(torch.isfinite(want[k]).all() for k in ("loss", "gx_u", "gx_i", "gw", "gb")), c["name"]
        _, _, eps, _, _ = R.scalars(c)
        for s in R.SIDES:                                  # no norm sits on the threshold: float32 clamps the same rows
            for v in (cf["np_" + s], cf["nt_" + s]):
                assert not ((v > 0.9 * eps) & (v < 1.1 * eps)).any(), c["name"]
        seen.add((c["form"], c["m"], c["idx_u"] is None))
    assert seen == {(f, m, g) for f, m in K.FORMS for g in (False, True)}
    for B, d in K.DEGENERATE_SHAPES:
        for f, m in K.FORMS:
            c, want, cf = by_name[f"degenerate-{K.form_name(f, m)}-B{B}-d{d}"]
            _, _, eps, _, c1 = R.scalars(c)
            assert float(c["b"].abs().max()) == 0.0
            for s, o, off in (("u", "i", 0), ("i", "u", 13)):
                r = {k: v + off for k, v in K.DEG.items()}
                np_, nt = cf["np_" + s], cf["nt_" + s]
                assert float(np_[r["zero_p"]]) == 0.0 and float(nt[r["zero_t"]]) == 0.0
                assert 0.75 * eps < float(np_[r["p_below"]]) < 0.85 * eps and 1.2 * eps < float(np_[r["p_above"]]) < 1.3 * eps
                assert 0.75 * eps < float(nt[r["t_below"]]) < 0.85 * eps and 1.2 * eps < float(nt[r["t_above"]]) < 1.3 * eps
                cl = cf["clamped_" + s]
                assert bool(cl[r["zero_p"]]) and bool(cl[r["p_below"]]) and not bool(cl[r["p_above"]])
                # a clamped row's gradient is th / eps, unprojected: the projection, wrongly applied to the row just
                # below eps, would take 0.64 of its parallel part off
                g = want["gx_" + s]
                assert float(g[r["zero_p"]].abs().max()) > 1e-3 * (c1 / B) / eps
                assert float(want["gx_" + s][r["zero_t"]].abs().max()) == 0.0
                # the cancelling rows: cos = +-1 and the exact gradient is far below GRAD_TOL of what cancels
                cos = ((c["x_" + s].double() @ c["W"].double().T) * cf["th_" + s]).sum(1) / np_.clamp_min(eps)
                assert abs(float(cos[r["parallel"]]) - 1) < 1e-6 and abs(float(cos[r["antiparallel"]]) + 1) < 1e-6
                sc = R.cancel_scales(c, s, cf)
                rows = c["cancel_" + s].nonzero().flatten().tolist()
                assert rows == [r["parallel"], r["antiparallel"]]
                assert (g[rows].abs().amax(1) <= 1e-5 * sc[rows]).all()
    # duplicates are the normal case, and the special lists are what they say
    c = by_name["buir-B129-d64"][0]
    assert len(torch.unique(c["idx_u"])) < 129 and len(torch.unique(c["idx_i"])) < 129
    c = by_name["dup40-buir-d64"][0]
    assert len(c["idx_u"]) == 257 and int(c["idx_u"].max()) < 40 and len(torch.unique(c["idx_u"])) <= 40
    c = by_name["one-id-selfcf-m0.05-d128"][0]
    assert int(c["idx_u"].abs().max()) == 0 and len(torch.unique(c["x_u"], dim=0)) == 1
    c, want, _ = by_name["outside-selfcf-m0.05-d128"]
    for s in R.SIDES:
        bad = c["bad_" + s]
        assert sorted(set(c["idx_" + s][bad].tolist())) == [-1, 40]
        assert float(want["gx_" + s][bad].abs().amin(1).min()) > 0.0      # gradients are per slot
    c, want, _ = by_name["history-2049-over-300"]
    assert c["store"] and len(torch.unique(c["idx_u"])) == 300
    for s in R.SIDES:                                      # the history tables end as the online rows, others untouched
        named = torch.zeros(300, dtype=torch.bool)
        named[c["idx_" + s].long()] = True
        assert torch.equal(want["T_" + s][c["idx_" + s].long()], c["x_" + s].double())
        assert torch.equal(want["T_" + s][~named], c["T_" + s].double()[~named])


def test_floor_frac_is_the_smallest_that_float32_torch_meets(cases, refs, closed):
    """DESIGN.md 4.15's rule: the reference's own expression in plain float32 torch on the CPU, every case, clamped and
    ordinary rows each on their own, cancelling rows by cancel_scales"""
    worst = {f: 0.0 for f in R.FLOORS}
    worst_loss = worst_w = 0.0
    for c, want, cf in zip(cases, refs, closed):
        got = R.reference(c, dtype=torch.float32)
        worst_loss = max(worst_loss, R.value_error(got["loss"], want["loss"]),
                         *(R.value_error(got["parts"][k], want["parts"][k]) for k in (0, 1)))
        worst_w = max(worst_w, *R.weight_errors(got["gw"], got["gb"], cf))
        for f in R.FLOORS:
            worst[f] = max(worst[f], _worst_row(c, got, want, cf, f))
    print("float32 torch against float64, worst per-row gradient error by floor:", worst, "loss:", worst_loss,
          "weights:", worst_w)
    passing = [f for f in R.FLOORS if worst[f] <= R.GRAD_TOL / 2]
    assert passing and R.FLOOR_FRAC == min(passing), worst
    assert worst_loss <= R.LOSS_TOL / 2 and worst_w <= R.GRAD_TOL / 2


def test_momentum_restatement_is_torchs_expression():
    for n in K.MOMENTUM_N:
        for d in K.MOMENTUM_D:
            c = K.momentum_case(n, d)
            tgt, idx = c["tgt"].clone(), c["idx"].long()
            tgt[idx] = tgt[idx] * c["m"] + c["src"][idx] * (1 - c["m"])
            got = R.momentum_rows(c["tgt"], c["src"], c["idx"], c["m"])
            assert np.array_equal(got.view(np.uint32), tgt.numpy().view(np.uint32)), (n, d)
            assert np.array_equal(got[-3:], c["tgt"].numpy()[-3:])
            assert n < 3 or len(torch.unique(idx)) < n
    c = K.momentum_case(65, 50)
    idx = torch.cat([c["idx"], torch.tensor([-1, c["rows"], -7], dtype=torch.int32)])
    assert np.array_equal(R.momentum_rows(c["tgt"], c["src"], idx, c["m"]), R.momentum_rows(c["tgt"], c["src"], c["idx"], c["m"]))


def test_header_section_and_bindings():
    text = open(os.path.join(REPO, "include", "selfrec_hip.h")).read()
    assert "(a-23) Bootstrap losses" in text and "model/graph/BUIR.py:69-95" in text and "model/graph/SelfCF.py:64-91" in text
    a, b = text.index("(a-23) Bootstrap losses"), text.index("(a-20) MHCN")
    assert text.index("(a-22) DirectAU") < a < b
    for name in ("srh_boot_ws_bytes", "srh_boot_fwd_bwd", "srh_rows_momentum_ws_bytes", "srh_rows_momentum_f32"):
        assert name in _lib.SIGNATURES and name in text[a:b]
    assert _lib.ABI_VERSION == 31 and "#define SRH_ABI_VERSION 31" in text
    assert C.sizeof(_lib.BootSide) == 48


def test_workspace_sizes_answer_on_the_host():
    lib = _lib.load()
    for B, d in ((2048, 96), (0, 64), (-1, 64), (1 << 24, 64), (65, 32), (65, 256)):
        assert lib.srh_boot_ws_bytes(B, d) == 0, (B, d)
    for d in (64, 128):
        for B in (1, 65, 2048, (1 << 24) - 1):
            got = lib.srh_boot_ws_bytes(B, d)
            z = -(-B // 256)
            # at least the documented arrays: dP and the row terms of both sides, the chunk partials
            assert got % 256 == 0 and got >= 2 * B * d * 4 + 2 * B * 8 + 2 * z * (d * d + d) * 4
    assert lib.srh_rows_momentum_ws_bytes(0, 64) == 0 and lib.srh_rows_momentum_ws_bytes(5, 0) == 0
    assert lib.srh_rows_momentum_ws_bytes(65, 50) >= 65 * 50 * 4


def _side(fake, **kw):
    f = dict(d_x=fake, d_tgt=fake, d_idx=fake, n_tgt=10, d_store=None, d_gx=fake)
    f.update(kw)
    return _lib.BootSide(**f)


def test_refusals_come_before_any_launch():
    """bad arguments are answered on the host: nothing below reaches a kernel (no device is needed)"""
    lib = _lib.load()
    fake = 4096
    err = lib.srh_last_error_string

    def call(B=65, d=64, alpha=1.0, beta=0.0, eps=1e-12, c0=4.0, c1=2.0, clamp=0, user=None, item=None, w=fake, ws=fake):
        u, i = user or _side(fake), item or _side(fake)
        return lib.srh_boot_fwd_bwd(C.byref(u), C.byref(i), w, fake, B, d, alpha, beta, eps, c0, c1, clamp, fake, fake, fake,
                                    fake, ws, None)
    assert call(d=96) == -3 and b"d=96 unsupported" in err()
    assert call(d=32) == -3 and call(d=256) == -3
    assert call(B=0) == -1 and b"B=0" in err()
    assert call(B=1 << 24) == -1 and b"too large" in err()
    assert call(eps=0.0) == -1 and b"eps" in err()
    assert call(eps=-1e-8) == -1 and call(eps=float("nan")) == -1 and call(eps=float("inf")) == -1
    for k in ("alpha", "beta", "c0", "c1"):
        assert call(**{k: float("inf")}) == -1 and b"finite" in err()
        assert call(**{k: float("nan")}) == -1
    assert call(clamp=2) == -1 and b"clamp=2" in err() and call(clamp=-1) == -1
    assert call(w=None) == -1 and b"null" in err()
    assert call(ws=None) == -1 and b"null" in err()
    assert call(user=_side(fake, d_x=None)) == -1 and b"user side" in err()
    assert call(item=_side(fake, d_gx=None)) == -1 and b"item side" in err()
    assert call(item=_side(fake, d_tgt=None)) == -1
    assert call(user=_side(fake, n_tgt=0)) == -1 and b"n_tgt=0" in err()
    assert lib.srh_boot_fwd_bwd(None, None, fake, fake, 65, 64, 1.0, 0.0, 1e-12, 4.0, 2.0, 1, fake, fake, fake, fake, fake,
                                None) == -1
    mom = lambda n=5, rows=9, d=64, m=0.9, omm=0.1, tgt=fake, idx=fake: lib.srh_rows_momentum_f32(  # noqa: E731
        tgt, fake, idx, n, rows, d, m, omm, fake, None)
    assert mom(d=0) == -1 and b"rows_momentum" in err()
    assert mom(n=-1) == -1 and mom(rows=-1) == -1
    assert mom(m=float("nan")) == -1 and mom(omm=float("inf")) == -1 and b"finite" in err()
    assert mom(tgt=None) == -1 and mom(idx=None) == -1 and b"null" in err()
    assert mom(n=0, tgt=None) == 0                            # nothing to do, nothing launched


def test_routes_and_the_ops_surface(monkeypatch):
    from selfrec_amd import ops
    from selfrec_amd.model.graph import BUIR as M
    from selfrec_amd.model.graph import SelfCF as S
    from selfrec_amd.util.conf import ModelConf
    monkeypatch.delenv("SRH_BOOT", raising=False)
    for model in ("BUIR", "SelfCF"):
        assert M.boot_route(None, model) == M.BOOT_DEFAULT[model] == M.boot_route(ModelConf({}), model)
        assert M.boot_route(ModelConf({"engine.boot": "torch"}), model) == "torch"
        assert M.boot_route(ModelConf({"engine.boot": " HIP"}), model) == "hip"
        with pytest.raises(ValueError):
            M.boot_route(ModelConf({"engine.boot": "triton"}), model)
    monkeypatch.setenv("SRH_BOOT", "torch")
    assert M.boot_route(ModelConf({"engine.boot": "hip"})) == "torch"
    monkeypatch.setenv("SRH_BOOT", "hip")
    assert M.boot_route(ModelConf({"engine.boot": "torch"}), "SelfCF") == "hip"
    assert set(M.BOOT_DEFAULT.values()) <= {"hip", "torch"}
    assert "engine.boot" in M.__doc__ and "engine.boot" in S.__doc__
    assert ops.boot_supported(64) and ops.boot_supported(128) and ops.boot_supported(50) and ops.boot_supported(1)
    assert not ops.boot_supported(129) and not ops.boot_supported(0)
    for name in ("boot_supported", "boot_fwd_bwd", "BootstrapLossFn", "rows_momentum"):
        assert name in ops.__all__ and hasattr(ops, name)
    assert issubclass(ops.BootstrapLossFn, ops.LossGradFn)
