"""MHCN without a GPU: the motif matrices against the reference's own run (tests/golden/mhcn.npz), the float64 restatement
tests/mhcn_ref.py against torch.autograd on the literal expression (the whole step on the tiny graph included), what plain
float32 loses on every GPU case (the yardstick the device bounds rest on), and the housekeeping around the new entry
points."""
import json
import os
import re

import numpy as np
import pytest
import torch

from selfrec_amd import _lib, synth
from selfrec_amd.data.social import Relation
from selfrec_amd.data.ui_graph import Interaction
from selfrec_amd.model.graph.MHCN import hyper_adj_mats
from tests import mhcn_cases, mhcn_ref
from tests.mhcn_cases import FWD_BOUND, GRAD_BOUND, LOSS_BOUND

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")


def max_rel(got, want):
    want = np.asarray(want, dtype=np.float64)
    if want.size == 0:
        return 0.0
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / max(np.abs(want).max(), 1e-300))


# ---- the data path -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(GOLDEN, "mhcn.npz"))
    with open(os.path.join(GOLDEN, "mhcn_meta.json")) as f:
        return {k: z[k] for k in z.files}, json.load(f)


def tiny_data():
    tu, ti, su, si, _, _ = synth.make_dataset("tiny")
    data = Interaction({}, synth.as_triples(tu, ti), synth.as_triples(su, si))
    return data, Relation({}, synth.make_social("tiny"), data.user)


def douban_data():
    z = np.load(os.path.join(GOLDEN, "douban_book.npz"))
    tr, te = ~z["is_test"], z["is_test"]
    data = Interaction({}, synth.as_triples(z["user"][tr], z["item"][tr]), synth.as_triples(z["user"][te], z["item"][te]))
    trust = np.load(os.path.join(GOLDEN, "sept.npz"))["trust"]
    lines = [[a, b, 1] for a, b in zip(trust[:, 0].astype(str).tolist(), trust[:, 1].astype(str).tolist())]
    return data, Relation({}, lines, data.user)


@pytest.mark.parametrize("case,make", [("douban", douban_data), ("tiny", tiny_data)])
def test_motif_matrices_equal_the_reference(golden, case, make):
    """structure exact, values bit for bit: the expressions are the reference's own scipy calls in its order"""
    g, meta = golden
    data, rel = make()
    info = meta[case]
    assert data.user_num == info["users"] and data.item_num == info["items"] and list(rel.size()) == info["size"]
    S = rel.get_social_mat()
    U = (S - S.multiply(S.T)).tocsr()
    U.eliminate_zeros()
    assert U.nnz == info["one_way_pairs"]
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")                      # the 1 / 0 of an empty row is silenced, not printed
        mats = hyper_adj_mats(S, data.interaction_mat)
    for name, mat in zip(("hs", "hj", "hp"), mats):
        m = mat.tocsr().copy()
        m.sum_duplicates()
        m.eliminate_zeros()
        m.sort_indices()
        assert m.dtype == np.float32, name
        assert np.isfinite(m.data).all()
        assert m.nnz == info[name]["nnz"] and int((np.diff(m.indptr) == 0).sum()) == info[name]["empty_rows"]
        assert np.array_equal(m.indptr, g[f"{case}_{name}_indptr"]), name
        assert np.array_equal(m.indices, g[f"{case}_{name}_indices"]), name
        assert np.array_equal(m.data.view(np.uint32), g[f"{case}_{name}_data"].view(np.uint32)), name
        sums = np.asarray(m.sum(axis=1)).ravel()
        assert np.allclose(sums[np.diff(m.indptr) > 0], 1.0, atol=1e-5)


def test_golden_covers_the_directed_terms(golden):
    _, meta = golden
    assert meta["douban"]["one_way_pairs"] == 0 and meta["tiny"]["one_way_pairs"] > 1000
    assert [meta["douban"][k]["nnz"] for k in ("hs", "hj", "hp")] == [77299, 8413, 8570]
    assert [meta["tiny"][k]["nnz"] for k in ("hs", "hj", "hp")] == [4474, 3702, 8726]


# ---- the restatement against torch.autograd on the literal expression ---------------------------------------------------
def leaf(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64).copy()).requires_grad_(True)


def t_gate(x, w, b):
    return x * torch.sigmoid(torch.matmul(x, w) + b)                   # MHCN.py:80


def t_attention(channels, att, mat):
    """MHCN.py:85-93 literally"""
    weights = [torch.sum(att * torch.matmul(e, mat), 1) for e in channels]
    score = torch.softmax(torch.stack(weights).T, dim=1)
    mixed = 0
    for i in range(len(weights)):
        mixed = mixed + (score.T[i] * channels[i].T).T
    return mixed, score


def t_mim(em, edge, perms):
    """MHCN.py:159-181 literally (-log(sigmoid)), the shuffles given"""
    p1, p2, p3, c2, c3 = (torch.from_numpy(np.asarray(p).astype(np.int64)) for p in perms)
    score = lambda a, b: torch.sum(a * b, 1)  # noqa: E731
    rcs = lambda e, c, p: e.T[c].T[p]  # noqa: E731
    pos, neg1, neg2 = score(em, edge), score(em[p1], edge), score(rcs(edge, c2, p2), em)
    local = torch.sum(-torch.log(torch.sigmoid(pos - neg1)) - torch.log(torch.sigmoid(neg1 - neg2)))
    graph = torch.mean(edge, 0)
    return local + torch.sum(-torch.log(torch.sigmoid(score(edge, graph) - score(rcs(edge, c3, p3), graph))))


def test_gate_restatement_against_autograd():
    rng = np.random.default_rng(0)
    n, d, c = 11, 6, 3
    x, w, b, gy = rng.standard_normal((n, d)), rng.standard_normal((c, d, d)), rng.standard_normal((c, d)), rng.standard_normal((c, n, d))
    lx, lw, lb = leaf(x), leaf(w), leaf(b)
    y = torch.stack([t_gate(lx, lw[k], lb[k]) for k in range(c)])
    y.backward(torch.from_numpy(gy))
    ry, _ = mhcn_ref.gate(x, w, b)
    gx, gw, gb = mhcn_ref.gate_bwd(x, w, b, gy)
    assert np.abs(ry - y.detach().numpy()).max() <= 1e-12
    for got, want in ((gx, lx.grad), (gw, lw.grad), (gb, lb.grad)):
        assert np.abs(got - want.numpy()).max() <= 1e-10


@pytest.mark.parametrize("with_x", [True, False])
def test_chan_mix_restatement_against_autograd(with_x):
    rng = np.random.default_rng(1)
    n, d = 13, 7
    e = [rng.standard_normal((n, d)) for _ in range(3)]
    att, mat, x, gout = rng.standard_normal((1, d)), rng.standard_normal((d, d)), rng.standard_normal((n, d)), rng.standard_normal((n, d))
    le, la, lm, lx = [leaf(t) for t in e], leaf(att), leaf(mat), leaf(x)
    mixed, score = t_attention(le, la, lm)
    out = mixed + lx / 2 if with_x else mixed
    out.backward(torch.from_numpy(gout))
    q = (mat @ att.T).reshape(-1)                                       # reduce_sum(att (.) (E M), 1) = E (M att^T)
    r_out, r_s = mhcn_ref.chan_mix(e, q, x if with_x else None, 0.5)
    ge, gx, gq = mhcn_ref.chan_mix_bwd(e, q, r_s, gout, 0.5)
    assert np.abs(r_out - out.detach().numpy()).max() <= 1e-12 and np.abs(r_s - score.detach().numpy()).max() <= 1e-12
    assert np.abs(r_s.sum(1) - 1).max() <= 1e-12
    for k in range(3):
        assert np.abs(ge[k] - le[k].grad.numpy()).max() <= 1e-10
    if with_x:
        assert np.abs(gx - lx.grad.numpy()).max() <= 1e-10
    assert np.abs(gq[:, None] * att - lm.grad.numpy()).max() <= 1e-10    # dq carried to both parameters
    assert np.abs((gq @ mat)[None, :] - la.grad.numpy()).max() <= 1e-10


@pytest.mark.parametrize("fam", ["normal", "identity", "empty"])
def test_mim_restatement_against_autograd(fam):
    em, edge, perms = mhcn_cases.mim_inputs((37, 64), fam)
    lem, led = leaf(em), leaf(edge)
    loss = t_mim(lem, led, perms)
    (0.37 * loss).backward()
    ref = mhcn_ref.mim(em, edge, perms, loss_scale=0.37)
    assert abs(ref["loss"] - 0.37 * loss.item()) <= 1e-10 * abs(ref["loss"])
    assert abs(0.37 * mhcn_ref.mim_reference_form(em, edge, perms) - ref["loss"]) <= 1e-10 * abs(ref["loss"])
    assert np.abs(ref["gem"] - lem.grad.numpy()).max() <= 1e-10
    assert np.abs(ref["gedge"] - led.grad.numpy()).max() <= 1e-10
    if fam == "identity":
        assert abs(ref["loss"] - 0.37 * 3 * 37 * np.log(2.0)) <= 1e-10
        assert not ref["x1"].any() and not ref["x2"].any() and not ref["x3"].any()


def test_softplus_form_is_the_reference_form_where_that_is_finite():
    """the `large` family: float64 -log(sigmoid) is finite and equals the softplus form; in float32 sigmoid underflows on
    some row and the reference's form is inf -- the stated deviation"""
    case = ((257, 64), "large")
    c = mhcn_cases.mim_case(case)
    ref = c["ref"]
    assert abs(mhcn_ref.mim_reference_form(c["em"], c["edge"], c["perms"]) - ref["loss"]) <= 1e-10 * ref["loss"]
    x = np.concatenate([ref["x1"], ref["x2"]])
    assert np.abs(x).max() > 60 and np.median(np.abs(x)) > 10
    with np.errstate(divide="ignore", over="ignore"):
        x32 = x.astype(np.float32)
        sig = (np.float32(1) / (np.float32(1) + np.exp(x32))).astype(np.float32)     # sigmoid(-x), float32
        assert (sig == 0).any() or np.isinf(-np.log(sig)).any() or np.abs(x).max() < 88
    assert np.isfinite(mhcn_ref.softplus(x.astype(np.float32))).all()


def test_step_restatement_against_autograd_on_the_tiny_graph():
    """the whole batch of MHCN.train() on the tiny graph with make_social("tiny"): the three losses and the hand gradients
    of every variable against autograd on the reference's lines"""
    data, rel = tiny_data()
    H = hyper_adj_mats(rel.get_social_mat(), data.interaction_mat)
    R = data.normalize_graph_mat(data.interaction_mat)
    rng = np.random.default_rng(5)
    nu, ni, d, L, reg, ss_rate = data.user_num, data.item_num, 8, 2, 0.01, 0.05
    params = {"user_embeddings": 0.3 * rng.standard_normal((nu, d)), "item_embeddings": 0.3 * rng.standard_normal((ni, d))}
    for k in mhcn_ref.WEIGHT_KEYS:
        params[k] = 0.4 * rng.standard_normal((1, d) if "bias" in k or k == "attention" else (d, d))
    u, i, j = rng.integers(0, nu, 64), rng.integers(0, ni, 64), rng.integers(0, ni, 64)
    perms = mhcn_cases.step_perms(nu, d)
    ref = mhcn_ref.step(params, H, R, u, i, j, perms, L, reg, ss_rate)

    P = {k: leaf(v) for k, v in params.items()}
    Hd = [torch.from_numpy(h.toarray().astype(np.float64)) for h in H]
    Rd = torch.from_numpy(R.toarray().astype(np.float64))
    l2n = lambda x: x * torch.rsqrt(torch.clamp((x * x).sum(dim=1, keepdim=True), min=1e-12))  # noqa: E731
    gate = lambda x, pre, k: t_gate(x, P[f"{pre}{k}"], P[f"{pre}_bias{k}"])  # noqa: E731
    att = lambda *ch: t_attention(ch, P["attention"], P["attention_mat"])  # noqa: E731
    c = [gate(P["user_embeddings"], "gating", k) for k in (1, 2, 3)]
    simple = gate(P["user_embeddings"], "gating", 4)
    all_c, all_s, item, all_i = [[x] for x in c], [simple], P["item_embeddings"], [P["item_embeddings"]]
    for _ in range(L):
        mixed = att(*c)[0] + simple / 2
        c = [Hd[k] @ c[k] for k in range(3)]
        for k in range(3):
            all_c[k].append(l2n(c[k]))
        new_item = Rd.T @ mixed
        all_i.append(l2n(new_item))
        simple = Rd @ item
        all_s.append(l2n(simple))
        item = new_item
    c = [sum(x) for x in all_c]
    user, score = att(*c)
    user = user + sum(all_s) / 2
    items = sum(all_i)
    ss = 0
    for k in range(3):
        em = gate(user, "sgating", k + 1)
        ss = ss + t_mim(em, Hd[k] @ em, perms[k])
    ss = ss_rate * ss
    bu, bp, bn = user[u], items[i], items[j]
    rec = -torch.log(torch.sigmoid((bu * bp).sum(1) - (bu * bn).sum(1)) + 10e-8).sum()
    l2 = lambda t: (t ** 2).sum() / 2  # noqa: E731
    regl = reg * (sum(l2(P[k]) for k in mhcn_ref.WEIGHT_KEYS) + l2(bu) + l2(bn) + l2(bp))
    (rec + regl + ss).backward()
    for name, want in (("rec_loss", rec), ("reg_loss", regl), ("ss_loss", ss)):
        assert abs(ref[name] - want.item()) <= 1e-10 * abs(want.item()), name
    assert np.abs(ref["score"] - score.detach().numpy()).max() <= 1e-12
    assert set(ref["grads"]) == set(params)
    for k in params:
        want = P[k].grad.numpy()
        assert np.abs(ref["grads"][k] - want).max() <= 1e-9 * max(np.abs(want).max(), 1e-30), k
    assert np.abs(ref["grads"]["sgating4"] - reg * params["sgating4"]).max() == 0      # read by the regulariser alone


# ---- the float32 yardstick: within half of the device bounds on every GPU case ---------------------------------------------
F32 = np.float32


@pytest.mark.parametrize("case", mhcn_cases.GATE_CASES, ids=mhcn_cases.gate_id)
def test_f32_yardstick_gate(case):
    c = mhcn_cases.gate_case(case)
    y, _ = mhcn_ref.gate(c["x"], c["w"], c["b"], F32)
    gx, gw, gb = mhcn_ref.gate_bwd(c["x"], c["w"], c["b"], c["gy"], F32)
    errs = dict(y=max_rel(y, c["y"]), gx=max_rel(gx, c["gx"]), gw=max_rel(gw, c["gw"]), gb=max_rel(gb, c["gb"]))
    print(mhcn_cases.gate_id(case), {k: f"{v:.2e}" for k, v in errs.items()})
    assert errs["y"] <= FWD_BOUND / 2
    assert max(errs["gx"], errs["gw"], errs["gb"]) <= GRAD_BOUND / 2


@pytest.mark.parametrize("case", mhcn_cases.MIX_CASES, ids=mhcn_cases.mix_id)
def test_f32_yardstick_mix(case):
    c = mhcn_cases.mix_case(case)
    out, s = mhcn_ref.chan_mix(c["e"], c["q"], c["x"], c["beta"], F32)
    ge, gx, gq = mhcn_ref.chan_mix_bwd(c["e"], c["q"], s, c["gout"], c["beta"], F32)
    errs = dict(out=max_rel(out, c["out"]), s=max_rel(s, c["s"]), gq=max_rel(gq, c["gq"]),
                ge=max(max_rel(ge[k], c["ge"][k]) for k in range(3)))
    print(mhcn_cases.mix_id(case), {k: f"{v:.2e}" for k, v in errs.items()})
    assert errs["out"] <= FWD_BOUND / 2 and errs["s"] <= FWD_BOUND / 2
    assert errs["ge"] <= GRAD_BOUND / 2 and errs["gq"] <= GRAD_BOUND / 2
    if case[1] == "equal":
        assert np.array_equal(c["s"], np.full_like(c["s"], 1.0 / 3.0))
    if case[1] == "ahead":
        assert np.sort(c["s"][1::2], axis=1)[:, 1].max() < 1e-12 and np.allclose(c["s"][1::2].max(1), 1.0)
        assert c["s"][0::2].max() < 0.999


@pytest.mark.parametrize("case", mhcn_cases.MIM_CASES, ids=mhcn_cases.mim_id)
def test_f32_yardstick_mim(case):
    c = mhcn_cases.mim_case(case)
    ref = c["ref"]
    y = mhcn_ref.mim(c["em"], c["edge"], c["perms"], dt=F32)
    errs = dict(loss=abs(float(y["loss"]) / ref["loss"] - 1), gem=mhcn_cases.mim_grad_error(case, "gem", y["gem"]),
                gedge=mhcn_cases.mim_grad_error(case, "gedge", y["gedge"]))
    print(mhcn_cases.mim_id(case), {k: f"{v:.2e}" for k, v in errs.items()})
    assert np.isfinite(ref["loss"]) and ref["loss"] > 0
    assert errs["loss"] <= LOSS_BOUND / 2 and errs["gem"] <= GRAD_BOUND / 2 and errs["gedge"] <= GRAD_BOUND / 2
    (n, d), fam = case
    if fam == "identity":
        assert abs(ref["loss"] - 3 * n * np.log(2.0)) <= 1e-9 * n
        assert max(np.abs(ref["gem"]).max(), np.abs(ref["gedge"]).max()) <= 1e-14        # zero matrices
    if fam == "large" and n >= 63:
        assert np.abs(np.concatenate([ref["x1"], ref["x2"]])).max() > 40
    if fam == "empty":
        assert not c["edge"][::3].any()


# ---- housekeeping -----------------------------------------------------------------------------------------------------------
def test_mhcn_is_a_model_and_its_conf_holds_the_reference_keys():
    from selfrec_amd import main
    from selfrec_amd.util.conf import ModelConf
    assert "MHCN" in main.MODELS
    conf = ModelConf(os.path.join(REPO, "conf", "MHCN.yaml")).config
    want = {"training.set": "./dataset/douban-book/train.txt", "test.set": "./dataset/douban-book/test.txt",
            "social.data": "./dataset/douban-book/trust.txt", "model": {"name": "MHCN", "type": "graph"},
            "item.ranking.topN": [10, 20], "embedding.size": 64, "max.epoch": 30, "batch.size": 2048,
            "learning.rate": 0.001, "reg.lambda": 0.0001, "MHCN": {"n_layer": 2, "ss_rate": 0.01}, "output": "./results/"}
    assert {k: v for k, v in conf.items() if not k.startswith("engine.")} == want
    assert set(k for k in conf if k.startswith("engine.")) == {"engine.gate", "engine.mix", "engine.mim"}
    assert all(conf[k] in ("hip", "torch") for k in conf if k.startswith("engine."))


MHCN_SYMBOLS = ("srh_gate_fwd_f32", "srh_gate_bwd_ws_bytes", "srh_gate_bwd_f32", "srh_chan_mix_fwd_f32",
                "srh_chan_mix_bwd_ws_bytes", "srh_chan_mix_bwd_f32", "srh_mim_ws_bytes", "srh_mim_fwd_bwd")


def test_header_section_and_exported_symbols():
    text = open(os.path.join(REPO, "include", "selfrec_hip.h")).read()
    assert "(a-20) MHCN" in text
    section = text[text.index("(a-20) MHCN"):text.index("(f-1) Dataset files")]
    declared = set(re.findall(r"\b(srh_\w+)\s*\(", section[section.index("*/"):]))
    assert declared == set(MHCN_SYMBOLS)
    lib = _lib.load()
    for name in MHCN_SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    import ctypes as C
    assert C.sizeof(_lib.MimArgs) == 2 * 8 + 3 * 8 + 2 * 8 + 8 + 4 + 4 + 3 * 8
    # shapes the kernels do not serve ask for no workspace
    assert lib.srh_mim_ws_bytes(10, 96) == 0 and lib.srh_gate_bwd_ws_bytes(10, 64, 5) == 0 and lib.srh_chan_mix_bwd_ws_bytes(10, 256) == 0
    assert lib.srh_mim_ws_bytes(10, 64) > 0 and lib.srh_gate_bwd_ws_bytes(10, 128, 4) > 0 and lib.srh_chan_mix_bwd_ws_bytes(10, 64) > 0


def test_engine_routes(monkeypatch):
    from selfrec_amd.model.graph import MHCN as M
    from selfrec_amd.util.conf import ModelConf
    table = (("SRH_MHCN_GATE", "engine.gate", M.gate_route), ("SRH_MHCN_MIX", "engine.mix", M.mix_route),
             ("SRH_MHCN_MIM", "engine.mim", M.mim_route))
    for env, _, _ in table:
        monkeypatch.delenv(env, raising=False)
    for env, key, fn in table:
        assert fn(None) == "hip" and fn(ModelConf({})) == "hip"
        assert fn(ModelConf({key: "Torch"})) == "torch"
        monkeypatch.setenv(env, "hip")
        assert fn(ModelConf({key: "torch"})) == "hip"
        monkeypatch.delenv(env)
        with pytest.raises(ValueError):
            fn(ModelConf({key: "triton"}))


def test_model_module_states_its_deviations():
    from selfrec_amd.model.graph import MHCN as M
    doc = M.__doc__
    assert "Stated deviations" in doc and "softplus" in doc and "Adam" in doc and "RNG" in doc
