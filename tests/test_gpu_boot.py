"""The bootstrap loss kernels (csrc/bootstrap.hip; include/selfrec_hip.h (a-23)) against float64 computed
on the device by tests/boot_ref.py, on the cases of tests/boot_cases.py: wave, tile and chunk edges (16, 64 and 256 rows),
both model forms, degenerate rows, duplicates and ids outside the table, the history semantics, repeatability,
rows_momentum against torch's own bits, BootstrapLossFn through autograd, and both models on both routes.

Every raw kernel call here goes through `raw`, which hands over a workspace and outputs pre-filled with NaN bytes: nothing
relies on the caller zeroing.  Bounds: LOSS_TOL on the loss and each part, GRAD_TOL per row of d_gx through
boot_ref.grad_errors at FLOOR_FRAC, GRAD_TOL of the element's scale S for d_gw and d_gb."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from selfrec_amd import _lib, ops
from tests import boot_cases as K
from tests import boot_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN_BYTE = 0xFF      # four (eight) of them are a NaN in float32 (float64)


def _fill(shape, dtype, byte=NAN_BYTE):
    t = torch.empty(shape, dtype=dtype, device=DEV)
    t.view(torch.uint8).fill_(byte)
    return t


def _bits(t):
    return t.contiguous().view(torch.int32)


def raw(c, byte=NAN_BYTE, clamp=None, separate_store=False):
    """srh_boot_fwd_bwd as it is, on a case whose d is a kernel width: (status, dict) on byte-filled outputs and workspace.
    A storing case hands its tables over as d_tgt AND d_store (separate_store: a copy of its own as d_store)."""
    lib = _lib.load()
    B, d = c["x_u"].shape
    alpha, beta, eps, c0, c1 = R.scalars(c)
    dev = {k: c[k].to(DEV).contiguous() for k in ("x_u", "x_i", "W", "b", "T_u", "T_i")}
    out = dict(out=_fill(3, torch.float64, byte), gw=_fill((d, d), torch.float32, byte), gb=_fill(d, torch.float32, byte),
               ws=_fill(max(int(lib.srh_boot_ws_bytes(B, d)), 256), torch.uint8, byte))
    sides = []
    for s in R.SIDES:
        idx = None if c["idx_" + s] is None else c["idx_" + s].to(DEV).contiguous()
        out["gx_" + s] = _fill((B, d), torch.float32, byte)
        out["T_" + s] = dev["T_" + s]
        out["S_" + s] = dev["T_" + s].clone() if separate_store else dev["T_" + s]
        out["idx_" + s] = idx
        sides.append(_lib.BootSide(dev["x_" + s].data_ptr(), dev["T_" + s].data_ptr(), None if idx is None else idx.data_ptr(),
                                   len(dev["T_" + s]), out["S_" + s].data_ptr() if c["store"] else None,
                                   out["gx_" + s].data_ptr()))
    out["keep"] = (dev, sides)
    st = lib.srh_boot_fwd_bwd(C.byref(sides[0]), C.byref(sides[1]), dev["W"].data_ptr(), dev["b"].data_ptr(), B, d, alpha, beta,
                              eps, c0, c1, int(R.cosine(c)) if clamp is None else clamp, out["out"][1:].data_ptr(),
                              out["out"].data_ptr(), out["gw"].data_ptr(), out["gb"].data_ptr(), out["ws"].data_ptr(),
                              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out.update(loss=out["out"][0], parts=out["out"][1:])
    return st, out


def run(c):
    st, got = raw(c)
    assert st == 0, _lib.load().srh_last_error_string()
    return got


def check(c, got):
    """a case against float64 autograd on the reference's expression; returns the figures"""
    want, cf = R.reference(c, device=DEV), R.closed_form(c, device=DEV)
    le = max(R.value_error(got["loss"], want["loss"]), *(R.value_error(got["parts"][k], want["parts"][k]) for k in (0, 1)))
    ex = 0.0
    for s in R.SIDES:
        cancel = c["cancel_" + s]
        scales = None if cancel is None else R.cancel_scales(c, s, cf)
        assert torch.isfinite(got["gx_" + s]).all(), c["name"]
        ex = max(ex, float(R.grad_errors(got["gx_" + s], want["gx_" + s], cf["clamped_" + s], cancel, scales).max()))
    ew, eb = R.weight_errors(got["gw"], got["gb"], cf)
    print(f"{c['name']}: loss {le:.2e}, gx rows {ex:.2e}, gw {ew:.2e} and gb {eb:.2e} of their scales")
    assert le <= R.LOSS_TOL and ex <= R.GRAD_TOL and ew <= R.GRAD_TOL and eb <= R.GRAD_TOL, (c["name"], le, ex, ew, eb)
    if "T_u" in got:                    # the tables afterwards: the stored rows bit for bit, every other row untouched
        for s in R.SIDES:
            after = got["S_" + s] if c["store"] else got["T_" + s]
            assert torch.equal(_bits(after), _bits(want["T_" + s].float())), (c["name"], "table", s)
    return le, ex, ew, eb


@pytest.mark.parametrize("B", K.ROWS)
def test_row_edges(B):
    for c in K.row_cases(B):
        check(c, run(c))


def test_large_batch():
    for c in K.large_cases():
        check(c, run(c))


def test_padded_widths_go_through_ops():
    for c in K.pad_cases():
        B, d = c["x_u"].shape
        alpha, beta, eps, c0, c1 = R.scalars(c)
        dev = {k: (None if c[k] is None else c[k].to(DEV)) for k in ("x_u", "x_i", "W", "b", "T_u", "T_i", "idx_u", "idx_i")}
        store = (dev["T_u"], dev["T_i"]) if c["store"] else (None, None)
        loss, parts, gu, gi, gw, gb = ops.boot_fwd_bwd(dev["x_u"], dev["x_i"], dev["W"], dev["b"], dev["T_u"], dev["T_i"],
                                                       dev["idx_u"], dev["idx_i"], *store, alpha, beta, eps, c0, c1, R.cosine(c))
        torch.cuda.synchronize()
        assert gu.shape == (B, d) and gi.shape == (B, d) and gw.shape == (d, d) and gb.shape == (d,)
        kw = ops.kernel_width(d, ops.TABLE_NCE_WIDTHS)
        # the padding is cut, and what was cut is exact zeros: a padded column takes no gradient
        full = gu._base
        assert full.shape == (2, B, kw) and float(full[..., d:].abs().max()) == 0.0
        wfull, bfull = gw._base, gb._base
        assert wfull.shape == (kw, kw) and float(wfull[d:].abs().max()) == 0.0 and float(wfull[:, d:].abs().max()) == 0.0
        assert bfull.shape == (kw,) and float(bfull[d:].abs().max()) == 0.0
        check(c, dict(loss=loss, parts=parts, gx_u=gu, gx_i=gi, gw=gw, gb=gb, T_u=dev["T_u"], T_i=dev["T_i"], S_u=dev["T_u"],
                      S_i=dev["T_i"]))


@pytest.mark.parametrize("shape", K.DEGENERATE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_degenerate_rows(shape):
    for f, m in K.FORMS:
        c = K.degenerate_case(*shape, f, m)
        got = run(c)
        check(c, got)
        for s, off in (("u", 0), ("i", 13)):           # t = 0: no gradient at all
            assert float(got["gx_" + s][K.DEG["zero_t"] + off].abs().max()) == 0.0


def test_the_two_clamp_modes_differ_only_below_eps():
    """SRH_BOOT_CLAMP_COSINE on BUIR's scalars: the rows whose |p| is in (0, eps) change, nothing else does"""
    c = K.degenerate_case(65, 64, "buir", None)
    (sa, a), (sb, b) = raw(c, clamp=0), raw(c, clamp=1)
    assert sa == 0 and sb == 0
    for s, off in (("u", 0), ("i", 13)):
        differ = (_bits(a["gx_" + s]) != _bits(b["gx_" + s])).any(1).nonzero().flatten().tolist()
        assert differ == [K.DEG["p_below"] + off], (s, differ)
    assert float(a["loss"]) == float(b["loss"])


def test_duplicates_and_ids_outside_the_table():
    for c in K.duplicate_cases():
        got = run(c)
        check(c, got)
        if "bad_u" in c:
            # a slot naming no row still takes its own gradient (its p meets the OTHER side's target, which is zero only
            # where that side's id is outside too and nothing of x is mixed in)
            for s, o in (("u", "i"), ("i", "u")):
                ok_o = (c["idx_" + o] >= 0) & (c["idx_" + o] < len(c["T_" + o]))
                bad = c["bad_" + s][ok_o[c["bad_" + s]] | (c["form"] != "buir")]
                assert len(bad) >= 12 and float(got["gx_" + s][bad.to(DEV)].abs().amax(1).min()) > 0.0


def test_history_rows_are_read_before_any_is_stored():
    """d_store == d_tgt at 2049 slots over 300 ids: every slot's target is the table's pre-call row (check() holds the loss
    and d_gx to the reference, which gathers before it scatters), afterwards the named rows are x bit for bit and the
    others untouched; a d_store of its own leaves d_tgt untouched"""
    c = K.history_case()
    got = run(c)
    check(c, got)
    for s in R.SIDES:
        idx = c["idx_" + s].long()
        assert torch.equal(_bits(got["T_" + s][idx.to(DEV)]), _bits(c["x_" + s].to(DEV)))
    st, sep = raw(c, separate_store=True)
    assert st == 0
    for s in R.SIDES:
        assert torch.equal(_bits(sep["T_" + s]), _bits(c["T_" + s].to(DEV)))
        assert torch.equal(_bits(sep["S_" + s]), _bits(got["T_" + s]))
        assert torch.equal(_bits(sep["gx_" + s]), _bits(got["gx_" + s]))


@pytest.mark.parametrize("shape", K.REPEAT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_two_calls_give_the_same_bits_whatever_the_buffers_held(shape):
    B, d = shape
    for f, m in (("buir", None), ("selfcf", 0.05)):
        c = K.plain_case(B, d, f, m)
        (sa, a), (sb, b) = raw(c), raw(c, byte=0x00)
        assert sa == 0 and sb == 0
        for k in ("out", "gx_u", "gx_i", "gw", "gb", "T_u", "T_i"):
            assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), (c["name"], k)
        # ops.boot_fwd_bwd (torch.empty buffers) is the same call
        alpha, beta, eps, c0, c1 = R.scalars(c)
        dev = {k: c[k].to(DEV) for k in ("x_u", "x_i", "W", "b", "T_u", "T_i", "idx_u", "idx_i")}
        store = (dev["T_u"], dev["T_i"]) if c["store"] else (None, None)
        loss, parts, gu, gi, gw, gb = ops.boot_fwd_bwd(dev["x_u"], dev["x_i"], dev["W"], dev["b"], dev["T_u"], dev["T_i"],
                                                       dev["idx_u"], dev["idx_i"], *store, alpha, beta, eps, c0, c1, R.cosine(c))
        assert float(loss) == float(a["loss"]) and torch.equal(parts, a["parts"])
        for x, k in ((gu, "gx_u"), (gi, "gx_i"), (gw, "gw"), (gb, "gb"), (dev["T_u"], "T_u"), (dev["T_i"], "T_i")):
            assert torch.equal(_bits(x), _bits(a[k])), (c["name"], k)


def test_refusals_write_nothing():
    lib = _lib.load()
    c = K.plain_case(65, 64)
    for k, v, status, word in (("x_u", torch.randn(65, 96), -3, b"d=96 unsupported"),):
        bad = dict(c, x_u=v, x_i=v, W=torch.randn(96, 96), b=torch.randn(96), T_u=torch.randn(40, 96), T_i=torch.randn(40, 96))
        st, got = raw(bad)
        assert st == status and word in lib.srh_last_error_string()
        for name in ("out", "gx_u", "gx_i", "gw", "gb"):
            assert bool((got[name].view(torch.uint8) == NAN_BYTE).all())
    st, got = raw(c, clamp=7)
    assert st == -1 and bool((got["gx_u"].view(torch.uint8) == NAN_BYTE).all())
    with pytest.raises(ops.SelfrecHipError):
        x = torch.randn(8, 129, device=DEV)
        ops.boot_fwd_bwd(x, x, torch.randn(129, 129, device=DEV), torch.randn(129, device=DEV), x, x)
    with pytest.raises(ops.SelfrecHipError):
        x = torch.randn(8, 64)
        ops.boot_fwd_bwd(x, x, torch.randn(64, 64), torch.randn(64), x, x)


@pytest.mark.parametrize("n", K.MOMENTUM_N)
def test_rows_momentum_is_torchs_index_assignment(n):
    for d in K.MOMENTUM_D:
        c = K.momentum_case(n, d)
        m = c["m"]
        src, idx = c["src"].to(DEV), c["idx"].to(DEV)
        want = c["tgt"].to(DEV)
        li = idx.long()
        want[li] = want[li] * m + src[li] * (1 - m)
        # the kernel's list also names ids outside the table: skipped
        wide = torch.cat([idx[: n // 2], torch.tensor([-1, c["rows"], -5, 1 << 30], dtype=torch.int32, device=DEV), idx[n // 2:]])
        runs = []
        for k in range(2):
            tgt = c["tgt"].to(DEV)
            need = int(_lib.load().srh_rows_momentum_ws_bytes(len(wide), d))
            ws = _fill(max(need, 256), torch.uint8, NAN_BYTE if k == 0 else 0)
            assert ops.rows_momentum(tgt, src, wide, m, ws=ws) is tgt
            torch.cuda.synchronize()
            runs.append(tgt)
        assert torch.equal(_bits(runs[0]), _bits(want)), (n, d)
        assert torch.equal(_bits(runs[0]), _bits(runs[1]))
        assert torch.equal(_bits(runs[0][-3:]), _bits(c["tgt"][-3:].to(DEV)))            # rows no slot names
        host = R.momentum_rows(c["tgt"], c["src"], c["idx"], m)
        assert np.array_equal(runs[0].cpu().numpy().view(np.uint32), host.view(np.uint32))


@pytest.mark.parametrize("form,m,shape", [("buir", None, (129, 50)), ("selfcf", 0.05, (65, 64)), ("selfcf", 0.995, (257, 100))])
def test_autograd_op(form, m, shape):
    """BootstrapLossFn under a non-unit upstream gradient, against float64 autograd for all four differentiable inputs"""
    B, d = shape
    c = K.plain_case(B, d, form, m, seed=4000 + B)
    alpha, beta, eps, c0, c1 = R.scalars(c)
    up = 0.37
    x_u, x_i, W, b = (c[k].to(DEV).requires_grad_(True) for k in ("x_u", "x_i", "W", "b"))
    T_u, T_i, idx_u, idx_i = (c[k].to(DEV) for k in ("T_u", "T_i", "idx_u", "idx_i"))
    store = (T_u, T_i) if c["store"] else (None, None)
    loss = ops.BootstrapLossFn.apply(x_u, x_i, W, b, T_u, T_i, idx_u, idx_i, *store, alpha, beta, eps, c0, c1, R.cosine(c))
    assert loss.dtype == torch.float32 and loss.dim() == 0
    (up * loss).backward()
    want = R.reference(c, device=DEV)
    assert x_u.grad.shape == (B, d) and W.grad.shape == (d, d) and b.grad.shape == (d,)
    # (the op's loss is float32: one rounding on top of the kernel's double)
    assert R.value_error(loss.detach(), want["loss"]) <= R.LOSS_TOL + 6e-8
    check(c, dict(loss=want["loss"], parts=want["parts"], gx_u=x_u.grad / up, gx_i=x_i.grad / up, gw=W.grad / up, gb=b.grad / up,
                  T_u=T_u, T_i=T_i, S_u=T_u, S_i=T_i))


def _two_steps(name, route, data, monkeypatch, tmp_path):
    import importlib
    from selfrec_amd.util import sampler as sampler_mod
    from selfrec_amd.util.conf import ModelConf
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("SRH_BOOT", raising=False)
    real_batches = sampler_mod.next_batch_pairwise
    seen = []

    def batches(d, bs, n_negs=1, **kw):
        for k, b in enumerate(real_batches(d, bs, n_negs, **kw)):
            if k == 2:
                return
            seen.append(b)
            yield b
    monkeypatch.setattr(sampler_mod, "next_batch_pairwise", batches)
    losses = []
    real_backward = torch.Tensor.backward
    monkeypatch.setattr(torch.Tensor, "backward",
                        lambda t, *a, **k: (losses.append(float(t.detach())), real_backward(t, *a, **k))[1])
    block = {"BUIR": {"n_layer": 2, "tau": 0.995, "drop_rate": 0.2}, "SelfCF": {"n_layer": 2, "tau": 0.05}}[name]
    conf = ModelConf({"model": {"name": name, "type": "graph"}, "item.ranking.topN": [10, 20], "embedding.size": 64,
                      "max.epoch": 1, "batch.size": 1024, "learning.rate": 0.001, "reg.lambda": 0.0001,
                      "output": "./results/", "training.set": "x", "test.set": "y", name: block, "engine.boot": route})
    torch.manual_seed(31); np.random.seed(32); random.seed(2718)
    cls = getattr(importlib.import_module(f"selfrec_amd.model.graph.{name}"), name)
    model = cls(conf, data.training_data, data.test_data)
    assert model.boot == route
    model.fast_evaluation = lambda epoch: None
    snaps = []
    if name == "SelfCF":                 # per step: the online rows as the model gathers them, the history tables afterwards
        real_loss = model.batch_loss

        def batch_loss(u, i, j):
            with torch.no_grad():
                u_all, i_all = model.model.online_encoder()
            out = real_loss(u, i, j)
            enc = model.model
            snaps.append(dict(u=(u, u_all[u], enc.u_target_his.clone()), i=(i, i_all[i], enc.i_target_his.clone())))
            return out
        model.batch_loss = batch_loss
    model.train()
    monkeypatch.undo()
    enc = model.model
    state = {k: v.detach().cpu().numpy() for k, v in enc.named_parameters()}
    if name == "SelfCF":
        state.update(u_target_his=enc.u_target_his.cpu().numpy(), i_target_his=enc.i_target_his.cpu().numpy())
    return losses, state, seen, snaps


@pytest.mark.parametrize("name", ["BUIR", "SelfCF"])
def test_model_routes_agree(name, golden_ops, fresh_tiny_data, monkeypatch, tmp_path):
    """two steps on the tiny graph from the same seeds, engine.boot: hip against engine.boot: torch (each on its own fresh
    copy of the data), to the figures test_gpu_f4.py holds these models to against the reference's own run.  named_parameters
    covers BUIR's target tables; SelfCF's history tables after step 1 are that step's online rows, bit for bit"""
    from tests.conftest import _tiny_interaction
    data = {"hip": fresh_tiny_data, "torch": _tiny_interaction(golden_ops)}
    runs = {r: _two_steps(name, r, data[r], monkeypatch, tmp_path) for r in ("hip", "torch")}
    (lh, ph, bh, snaps), (lt, pt, bt, _) = runs["hip"], runs["torch"]
    assert len(lh) == 2 and len(lt) == 2
    for x, y in zip(bh, bt):
        assert all(np.array_equal(p, q) for p, q in zip(x, y))
    np.testing.assert_allclose(lh, lt, rtol=2e-5)
    if name == "BUIR":
        assert any(k.startswith("target_encoder") for k in pt)
    for k in pt:
        assert np.abs(ph[k] - pt[k]).max() < 1e-5, k
    if name == "SelfCF":
        assert len(snaps) == 2
        for side in ("u", "i"):
            idx, rows, his = snaps[0][side]
            assert torch.equal(his[idx].view(torch.int32), rows.contiguous().view(torch.int32)), side
