"""MHCN on the GPU against the float64 restatement tests/mhcn_ref.py, through the C ABI wrappers of selfrec_amd/ops/mhcn.py: the
gate kernels on every shape, the channel mix and the MIM loss on ordinary inputs (their edge families are in
tests/test_gpu_mhcn_edges.py), the autograd functions, and the model's step, routes and training on the tiny synthetic graph
with generated trust pairs."""
import numpy as np
import pytest
import torch

from selfrec_amd import ops, synth
from tests import mhcn_cases, mhcn_ref
from tests.mhcn_cases import FWD_BOUND, GRAD_BOUND, LOSS_BOUND

pytestmark = pytest.mark.gpu


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype)


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def max_rel(got, want):
    want = np.asarray(want, dtype=np.float64)
    if want.size == 0:
        return 0.0
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / max(np.abs(want).max(), 1e-300))


def check(name, got, want, bound):
    err = max_rel(got, want)
    print(f"{name}: {err:.3e}")
    assert np.isfinite(np.asarray(got)).all(), name
    assert err <= bound, name


# ---- the gates -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", mhcn_cases.GATE_CASES, ids=mhcn_cases.gate_id)
def test_gate_forward_and_backward(case):
    c = mhcn_cases.gate_case(case)
    x, w, b, gy = dev(c["x"]), dev(c["w"]), dev(c["b"]), dev(c["gy"])
    y = ops.gate_fwd(x, w, b)
    gx, gw, gb = ops.gate_bwd(x, w, b, gy)
    assert y.shape == c["y"].shape and gx.shape == c["gx"].shape and gw.shape == c["gw"].shape and gb.shape == c["gb"].shape
    tag = mhcn_cases.gate_id(case)
    check(f"gate {tag} y", host(y), c["y"], FWD_BOUND)
    check(f"gate {tag} gx", host(gx), c["gx"], GRAD_BOUND)
    check(f"gate {tag} gw", host(gw), c["gw"], GRAD_BOUND)
    check(f"gate {tag} gb", host(gb), c["gb"], GRAD_BOUND)


def test_gate_fn_is_the_wrappers_under_autograd():
    c = mhcn_cases.gate_case((65, 64, 3))
    x, w, b = (dev(c[k]).requires_grad_(True) for k in ("x", "w", "b"))
    y = ops.GateFn.apply(x, w, b)
    y.backward(dev(c["gy"]))
    check("GateFn gx", host(x.grad), c["gx"], GRAD_BOUND)
    check("GateFn gw", host(w.grad), c["gw"], GRAD_BOUND)
    check("GateFn gb", host(b.grad), c["gb"], GRAD_BOUND)


# ---- channel mix and MIM on ordinary inputs ---------------------------------------------------------------------------------
def run_mix(c):
    e = [dev(t) for t in c["e"]]
    q, x, gout = dev(c["q"]), (None if c["x"] is None else dev(c["x"])), dev(c["gout"])
    out, s = ops.chan_mix_fwd(*e, q, x, c["beta"])
    g1, g2, g3, gx, gq = ops.chan_mix_bwd(*e, q, s, gout, c["beta"], with_x=x is not None)
    return dict(out=host(out), s=host(s), ge=[host(g1), host(g2), host(g3)], gx=None if gx is None else host(gx), gq=host(gq))


def check_mix(case, got):
    c = mhcn_cases.mix_case(case)
    tag = mhcn_cases.mix_id(case)
    check(f"mix {tag} out", got["out"], c["out"], FWD_BOUND)
    check(f"mix {tag} s", got["s"], c["s"], FWD_BOUND)
    assert np.abs(got["s"].sum(1) - 1).max() <= 1e-6
    for k in range(3):
        check(f"mix {tag} ge{k + 1}", got["ge"][k], c["ge"][k], GRAD_BOUND)
    check(f"mix {tag} gq", got["gq"], c["gq"], GRAD_BOUND)
    if c["x"] is not None:
        check(f"mix {tag} gx", got["gx"], c["gx"], GRAD_BOUND)
    else:
        assert got["gx"] is None


@pytest.mark.parametrize("case", [c for c in mhcn_cases.MIX_CASES if c[1] == "normal"], ids=mhcn_cases.mix_id)
def test_chan_mix_forward_and_backward(case):
    check_mix(case, run_mix(mhcn_cases.mix_case(case)))


def run_mim(c, loss_scale=1.0):
    loss, gem, gedge = ops.mim_fwd_bwd(dev(c["em"]), dev(c["edge"]), *(dev(p, torch.int32) for p in c["perms"]),
                                       loss_scale=loss_scale)
    assert loss.dtype == torch.float64
    return float(loss.cpu()), host(gem), host(gedge)


def check_mim(case, got):
    c = mhcn_cases.mim_case(case)
    tag = mhcn_cases.mim_id(case)
    loss, gem, gedge = got
    err = abs(loss / c["ref"]["loss"] - 1)
    e1, e2 = mhcn_cases.mim_grad_error(case, "gem", gem), mhcn_cases.mim_grad_error(case, "gedge", gedge)
    print(f"mim {tag}: loss {err:.3e} gem {e1:.3e} gedge {e2:.3e}")
    assert np.isfinite(loss) and np.isfinite(gem).all() and np.isfinite(gedge).all()
    assert err <= LOSS_BOUND and e1 <= GRAD_BOUND and e2 <= GRAD_BOUND


@pytest.mark.parametrize("case", [c for c in mhcn_cases.MIM_CASES if c[1] == "normal"], ids=mhcn_cases.mim_id)
def test_mim_loss_and_gradients(case):
    check_mim(case, run_mim(mhcn_cases.mim_case(case)))


def test_mim_loss_scale_scales_everything():
    case = ((65, 64), "normal")
    c = mhcn_cases.mim_case(case)
    loss, gem, gedge = run_mim(c, loss_scale=0.25)
    assert abs(loss / (0.25 * c["ref"]["loss"]) - 1) <= LOSS_BOUND
    assert max_rel(gem, 0.25 * c["ref"]["gem"]) <= GRAD_BOUND and max_rel(gedge, 0.25 * c["ref"]["gedge"]) <= GRAD_BOUND


def test_mix_and_mim_fns_under_autograd():
    case = ((65, 100), "normal", True)
    c = mhcn_cases.mix_case(case)
    e = [dev(t).requires_grad_(True) for t in c["e"]]
    q, x = dev(c["q"]).requires_grad_(True), dev(c["x"]).requires_grad_(True)
    out, s = ops.ChanMixFn.apply(*e, q, x, c["beta"])
    assert not s.requires_grad
    out.backward(dev(c["gout"]))
    check_mix(case, dict(out=host(out), s=host(s), ge=[host(t.grad) for t in e], gx=host(x.grad), gq=host(q.grad)))
    mcase = ((257, 48), "normal")
    m = mhcn_cases.mim_case(mcase)
    em, edge = dev(m["em"]).requires_grad_(True), dev(m["edge"]).requires_grad_(True)
    loss = ops.MimFn.apply(em, edge, *(dev(p, torch.int32) for p in m["perms"]))
    (0.5 * loss).backward()
    assert abs(float(loss.detach()) / m["ref"]["loss"] - 1) <= LOSS_BOUND
    assert max_rel(host(em.grad), 0.5 * m["ref"]["gem"]) <= GRAD_BOUND
    assert max_rel(host(edge.grad), 0.5 * m["ref"]["gedge"]) <= GRAD_BOUND


def test_rows_l2norm_fn_under_autograd():
    from tests import sept_ref
    rng = np.random.default_rng(3)
    y, g = rng.standard_normal((70, 64)).astype(np.float32), rng.standard_normal((70, 64)).astype(np.float32)
    y[5] = 0.0
    leaf = dev(y).requires_grad_(True)
    out = ops.RowsL2NormFn.apply(leaf)
    out.backward(dev(g))
    w_out, inv, clamped = sept_ref.l2norm(y)
    assert max_rel(host(out), w_out) <= 1e-6
    assert max_rel(host(leaf.grad), sept_ref.l2norm_bwd(g, w_out, inv, clamped)) <= 1e-6


# ---- the model ------------------------------------------------------------------------------------------------------------
S = mhcn_cases.STEP


def make_model(gate="hip", mix="hip", mim="hip", max_epoch=2, seed=3):
    import random
    from selfrec_amd.model.graph.MHCN import MHCN
    from selfrec_amd.util.conf import ModelConf
    tu, ti, su, si, _, _ = synth.make_dataset("tiny")
    conf = ModelConf({"training.set": "./none", "test.set": "./none", "model": {"name": "MHCN", "type": "graph"},
                      "item.ranking.topN": [10, 20], "embedding.size": S["emb"], "max.epoch": max_epoch,
                      "batch.size": S["batch"], "learning.rate": 0.001, "reg.lambda": S["reg"], "output": "./results/",
                      "MHCN": {"n_layer": S["n_layer"], "ss_rate": S["ss_rate"]},
                      "engine.gate": gate, "engine.mix": mix, "engine.mim": mim})
    torch.manual_seed(seed)
    random.seed(seed)
    return MHCN(conf, synth.as_triples(tu, ti), synth.as_triples(su, si), **{"social.data": synth.make_social("tiny")})


def first_batch(model):
    import random
    from selfrec_amd.util.sampler import next_batch_pairwise
    random.seed(11)
    return next(iter(next_batch_pairwise(model.data, S["batch"], as_arrays=True)))


def params_of(model):
    enc = model.model
    out = {"user_embeddings": enc.user_embeddings, "item_embeddings": enc.item_embeddings}
    out.update({k: v for k, v in enc.weights.items()})
    return out


def run_step(model, batch, perms):
    model.model.cuda()
    model.draw_perms = lambda ch, n, d, device: perms[ch]
    rec, reg, ss, loss = model.batch_losses(*(torch.from_numpy(a).cuda() for a in batch))
    loss.backward()
    return dict(rec_loss=float(rec.detach()), reg_loss=float(reg.detach()), ss_loss=float(ss.detach()),
                grads={k: host(p.grad) for k, p in params_of(model).items()}, score=host(model.model.attention_score))


@pytest.fixture(scope="module")
def hip_step():
    model = make_model()
    batch = first_batch(model)
    perms = mhcn_cases.step_perms(model.data.user_num, S["emb"])
    params = {k: host(p) for k, p in params_of(model).items()}
    got = run_step(model, batch, perms)
    R = model.data.normalize_graph_mat(model.data.interaction_mat)
    ref = mhcn_ref.step(params, model.build_hyper_adj_mats(), R, *batch, perms, S["n_layer"], S["reg"], S["ss_rate"])
    return model, batch, perms, got, ref


def test_model_has_the_reference_variables():
    model = make_model()
    assert set(params_of(model)) == set(mhcn_ref.WEIGHT_KEYS) | {"user_embeddings", "item_embeddings"}
    assert (model.gate, model.mix, model.mim) == ("hip", "hip", "hip")


def test_model_step_matches_the_restatement(hip_step):
    _, _, _, got, ref = hip_step
    for name in ("rec_loss", "reg_loss", "ss_loss"):
        err = abs(got[name] / ref[name] - 1)
        print(f"model {name}: {got[name]:.6f} vs {ref[name]:.6f} ({err:.3e})")
        assert err <= LOSS_BOUND, name
    assert set(got["grads"]) == set(ref["grads"])
    for name, want in ref["grads"].items():
        check(f"model grad {name}", got["grads"][name].reshape(want.shape), want, GRAD_BOUND)
    check("model attention_score", got["score"], ref["score"], FWD_BOUND)
    assert np.abs(got["score"].sum(1) - 1).max() <= 1e-6


@pytest.mark.parametrize("routes", [("torch", "hip", "hip"), ("hip", "torch", "hip"), ("hip", "hip", "torch"),
                                    ("torch", "torch", "torch")], ids="-".join)
def test_model_routes_agree(hip_step, routes):
    _, batch, perms, got, _ = hip_step
    model = make_model(*routes)
    assert (model.gate, model.mix, model.mim) == routes
    other = run_step(model, batch, perms)
    for name in ("rec_loss", "reg_loss", "ss_loss"):
        assert abs(other[name] / got[name] - 1) <= LOSS_BOUND, name
    for name, want in got["grads"].items():
        check(f"routes {'-'.join(routes)} grad {name}", other["grads"][name], want, GRAD_BOUND)
    check("routes attention_score", other["score"], got["score"], FWD_BOUND)


def test_model_trains_two_epochs_and_ranks():
    """two epochs end to end with fresh shuffles from the seeded device generator, fast_evaluation included: the
    recommendation loss per sample falls, the attention scores are a distribution, test() ranks"""
    model = make_model(max_epoch=2)
    model.train()
    hist = model.rec_loss_history
    print("rec loss per sample by epoch:", hist)
    assert len(hist) == 2 and np.isfinite(hist).all() and hist[1] < hist[0]
    n_batches = -(-len(model.data.training_data) // model.batch_size)
    assert {int(s["step"]) for s in model.optimizer.state.values()} == {2 * n_batches}
    score = host(model.attention_score)
    assert score.shape == (model.data.user_num, 3) and np.abs(score.sum(1) - 1).max() <= 1e-6
    p_a = model.perms(0, 300, 64, "cuda")
    p_b = model.perms(0, 300, 64, "cuda")
    assert not torch.equal(p_a[0], p_b[0])                    # fresh on every call
    assert all(sorted(p.tolist()) == list(range(p.numel())) for p in p_a)
    rec_list = model.test()
    ranked = rec_list[next(iter(model.data.test_set))]
    assert len(ranked) == 20 and all(a[1] >= b[1] for a, b in zip(ranked, ranked[1:]))
    assert hasattr(model, "bestPerformance") and len(model.bestPerformance) == 2
