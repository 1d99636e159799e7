"""SEPT without a GPU: the social data path against the reference's own run (tests/golden/sept.npz, sept_mats.npz), the
float64 restatement tests/sept_ref.py against torch.autograd on the literal expression (clamped rows included), how many
top-k cuts of the GPU cases float32 cannot call, what plain float32 loses on the edge cases (the yardstick of
tests/test_gpu_sept_edges.py), and the housekeeping around the new entry points."""
import json
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from selfrec_amd import _lib, synth
from selfrec_amd.data.loader import FileIO
from selfrec_amd.data.social import Relation
from selfrec_amd.data.ui_graph import Interaction
from selfrec_amd.model.graph.SEPT import social_related_views
from tests import sept_cases, sept_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")


# ---- the data path -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    a, b = np.load(os.path.join(GOLDEN, "sept.npz")), np.load(os.path.join(GOLDEN, "sept_mats.npz"))
    out = {k: a[k] for k in a.files}
    out.update({k: b[k] for k in b.files})
    with open(os.path.join(GOLDEN, "sept_meta.json")) as f:
        return out, json.load(f)


@pytest.fixture(scope="module")
def douban_social(golden):
    g, _ = golden
    z = np.load(os.path.join(GOLDEN, "douban_book.npz"))
    tr, te = ~z["is_test"], z["is_test"]
    data = Interaction({}, synth.as_triples(z["user"][tr], z["item"][tr]), synth.as_triples(z["user"][te], z["item"][te]))
    lines = [[a, b, 1] for a, b in zip(g["trust"][:, 0].astype(str).tolist(), g["trust"][:, 1].astype(str).tolist())]
    return data, Relation({}, lines, data.user), lines


def assert_same_csr(mat, g, name):
    m = mat.tocsr().copy()
    m.sum_duplicates()
    m.sort_indices()
    assert m.dtype == np.float32, name
    assert np.array_equal(m.indptr, g[f"{name}_indptr"]), name
    assert np.array_equal(m.indices, g[f"{name}_indices"]), name
    assert np.array_equal(m.data.view(np.uint32), g[f"{name}_data"].view(np.uint32)), name     # bit for bit


def test_relation_equals_the_reference_on_douban_book(golden, douban_social):
    g, meta = golden
    data, rel, lines = douban_social
    assert data.user_num == meta["users"] and data.item_num == meta["items"]
    assert list(rel.size()) == g["size"].tolist() == meta["size"]
    assert len(lines) == rel.size()[1] < meta["trust_lines"]            # the caller's list is filtered in place
    assert_same_csr(rel.get_social_mat(), g, "social")
    assert_same_csr(rel.get_birectional_social_mat(), g, "bi")


def test_social_views_equal_the_reference_on_douban_book(golden, douban_social):
    g, meta = golden
    data, rel, _ = douban_social
    friend, sharing = social_related_views(rel, rel.get_birectional_social_mat(), data.interaction_mat)
    assert_same_csr(friend, g, "friend")
    assert_same_csr(sharing, g, "sharing")
    assert friend.nnz == meta["friend"]["nnz"] and sharing.nnz == meta["sharing"]["nnz"]


def test_relation_quirks_and_accessors():
    user = {"a": 0, "b": 1, "c": 2}
    lines = [["a", "b", 1], ["a", "b", 1], ["b", "a", 0.5], ["a", "z", 1], ["z", "c", 1], ["c", "a", 2.0]]
    rel = Relation({}, lines, user)
    assert [p[:2] for p in lines] == [["a", "b"], ["a", "b"], ["b", "a"], ["c", "a"]]      # outsiders dropped
    s = rel.get_social_mat().toarray()
    assert s.dtype == np.float32 and s[0, 1] == 2.0 and s[1, 0] == 1.0 and s[2, 0] == 1.0    # duplicates are summed
    bi = rel.get_birectional_social_mat().toarray()
    assert np.array_equal(bi, s * s)                                                          # S (.) S, not S (.) S^T
    assert rel.size() == (2, 4)
    assert rel.weight("b", "a") == 0.5 and rel.weight("b", "c") == 0 and rel.weight("q", "a") == 0
    assert rel.get_followees("a") == {"b": 1} and rel.get_followers("a") == {"b": 0.5, "c": 2.0}
    assert rel.get_followees("q") == {} and rel.get_followers("q") == {}
    assert rel.has_followee("a", "b") and not rel.has_followee("b", "c") and rel.has_follower("a", "c")
    lap = rel.convert_to_laplacian_mat(sp.csr_matrix(s)).toarray()
    deg = s.sum(1)
    with np.errstate(divide="ignore"):
        scale = np.where(deg > 0, deg ** -0.5, 0.0).astype(np.float32)
    assert np.allclose(lap, scale[:, None] * s * scale[None, :], rtol=1e-6)


def test_load_social_data_parses_two_and_three_fields(tmp_path):
    p = tmp_path / "trust.txt"
    p.write_text("u1 u2\nu2 u3 0.5\nu3 u1 2\n")
    got = FileIO.load_social_data(str(p))
    assert got == [["u1", "u2", 1], ["u2", "u3", 0.5], ["u3", "u1", 2.0]]
    assert isinstance(got[0][2], int) and isinstance(got[1][2], float)


def test_make_social_is_seed_stable_loads_and_gives_both_views(tmp_path):
    lines = synth.make_social("tiny", seed=5)
    assert lines == synth.make_social("tiny", seed=5) and lines != synth.make_social("tiny", seed=6)
    assert all(w == 1 and a != b for a, b, w in lines) and len({(a, b) for a, b, _ in lines}) == len(lines)
    n_users = synth.SHAPES["tiny"][0]
    assert 6.0 < len(lines) / n_users < 20.0                       # douban-book: 12.6 trust lines per user
    out_deg = np.bincount(np.asarray([int(a) for a, _, _ in lines]), minlength=n_users)
    assert out_deg.max() > 4 * np.median(out_deg)                  # skewed
    pairs = {(a, b) for a, b, _ in lines}
    assert sum((b, a) in pairs for a, b in pairs) > 0.1 * len(pairs)  # some are followed back
    p = str(tmp_path / "trust.txt")
    synth.write_social(p, lines)
    assert FileIO.load_social_data(p) == [[a, b, 1.0] for a, b, _ in lines]
    tu, ti, su, si, _, _ = synth.make_dataset("tiny")
    data = Interaction({}, synth.as_triples(tu, ti), synth.as_triples(su, si))
    rel = Relation({}, lines, data.user)
    bi = rel.get_birectional_social_mat()
    assert bi.dot(bi).multiply(bi).nnz > 0 and data.interaction_mat.dot(data.interaction_mat.T).multiply(bi).nnz > 0
    friend, sharing = social_related_views(rel, bi, data.interaction_mat)
    assert friend.nnz > n_users and sharing.nnz > n_users          # more than the identity each


# ---- the restatement against torch.autograd on the literal expression ---------------------------------------------------
def t_l2n(x):
    return x * torch.rsqrt(torch.clamp((x * x).sum(dim=1, keepdim=True), min=sept_ref.EPS))


def t_tri_nd(F, S, R, A, k, tau):
    """SEPT.py:98-134 literally: softmax, topk, gather, log-ratio -> (three losses, pos)"""
    a = t_l2n(A)
    s = [t_l2n(v) @ a.T for v in (F, S, R)]
    prob = [torch.softmax(x, dim=1) for x in s]
    losses, pos = [], []
    for v, (p, q) in enumerate(sept_ref.PAIRS):
        idx = torch.topk((prob[p] + prob[q]) / 2, k, dim=1)[1]
        pos_score = torch.exp(torch.gather(s[v], 1, idx) / tau).sum(dim=1)
        ttl_score = torch.exp(s[v] / tau).sum(dim=1)
        losses.append(-torch.log(pos_score / ttl_score).sum())
        pos.append(idx)
    return losses, torch.stack(pos)


def test_tri_nd_restatement_against_autograd():
    n, d, k = 33, 8, 10
    mats = sept_cases.draw(n, d, 3)
    leaves = [torch.from_numpy(m).double().requires_grad_(True) for m in mats]
    losses, pos = t_tri_nd(*leaves, k, sept_cases.TAU)
    (0.37 * sum(losses)).backward()
    ref = sept_ref.tri_nd(*mats, k, sept_cases.TAU, loss_scale=0.37)
    assert np.array_equal(np.sort(ref["pos"], axis=2), np.sort(pos.numpy(), axis=2))
    assert np.array_equal(ref["pos"], pos.numpy())                 # best first (no ties in random data)
    for v in range(3):
        assert abs(ref["loss"][v] - 0.37 * losses[v].item()) <= 1e-10
    for g, leaf in zip(ref["grads"], leaves):
        assert np.abs(g - leaf.grad.numpy()).max() <= 1e-10
    # a given index set: the loss and gradients of THAT set
    other = np.stack([np.tile(np.arange(k), (n, 1))] * 3)
    given = sept_ref.tri_nd(*mats, k, sept_cases.TAU, pos=other)
    leaves = [torch.from_numpy(m).double().requires_grad_(True) for m in mats]
    a = t_l2n(leaves[3])
    total = 0
    for v in range(3):
        s = t_l2n(leaves[v]) @ a.T
        total = total - torch.log(torch.exp(s[:, :k] / sept_cases.TAU).sum(1) / torch.exp(s / sept_cases.TAU).sum(1)).sum()
    total.backward()
    assert abs(given["loss"].sum() - total.item()) <= 1e-10
    for g, leaf in zip(given["grads"], leaves):
        assert np.abs(g - leaf.grad.numpy()).max() <= 1e-10
    assert given["gap"].shape == (3, n) and (given["gap"] >= 0).all()


def test_l2norm_restatement_against_autograd():
    rng = np.random.default_rng(0)
    y = rng.standard_normal((9, 5))
    y[2] = 0.0                                    # a zero row
    y[4] = 1e-8 * rng.standard_normal(5)          # squared norm ~ 1e-16: below the clamp
    y[6] *= 1e-5                                  # squared norm ~ 1e-10: small, above the clamp
    g = rng.standard_normal((9, 5))
    out, inv, clamped = sept_ref.l2norm(y)
    assert clamped.tolist() == [False, False, True, False, True, False, False, False, False]
    assert inv[2] == 1e6 and inv[4] == 1e6
    leaf = torch.from_numpy(y).requires_grad_(True)
    t_out = t_l2n(leaf)
    t_out.backward(torch.from_numpy(g))
    assert np.abs(out - t_out.detach().numpy()).max() <= 1e-10
    gy = sept_ref.l2norm_bwd(g, out, inv, clamped)
    assert np.abs(gy - leaf.grad.numpy()).max() <= 1e-10 * np.abs(gy).max()
    assert np.array_equal(gy[2], g[2] * 1e6)


def test_step_restatement_against_autograd():
    """the whole batch of SEPT.train() -- four encoders, BPR, the regulariser, the tri-training loss -- on a small dense
    problem: the hand gradients of both tables against autograd, jointly and for the rec-only optimiser"""
    rng = np.random.default_rng(7)
    nu, ni, d, k, L = 14, 9, 6, 3, 2
    rand_adj = lambda r, c, p: sp.csr_matrix((rng.random((r, c)) < p) * rng.random((r, c)))  # noqa: E731
    adj, sub = rand_adj(nu + ni, nu + ni, 0.3), rand_adj(nu + ni, nu + ni, 0.2)
    fr, sh = rand_adj(nu, nu, 0.4), rand_adj(nu, nu, 0.3)
    U, I = rng.standard_normal((nu, d)) * 0.3, rng.standard_normal((ni, d)) * 0.3
    u_idx = rng.integers(0, nu, 20)
    i_idx, j_idx = rng.integers(0, ni, 20), rng.integers(0, ni, 20)
    kw = dict(n_layers=L, reg=0.01, ss_rate=0.05, k=k)
    for joint in (True, False):
        ref = sept_ref.step(U, I, adj, sub, fr, sh, u_idx, i_idx, j_idx, joint=joint, **kw)
        tu, ti = torch.from_numpy(U).requires_grad_(True), torch.from_numpy(I).requires_grad_(True)
        dense = lambda m: torch.from_numpy(m.toarray())  # noqa: E731

        def enc(emb, a):
            total = emb
            for _ in range(L):
                emb = t_l2n(dense(a) @ emb)
                total = total + emb
            return total

        ego = torch.cat([tu, ti])
        rec = enc(ego, adj)
        ru, rit = rec[:nu], rec[nu:]
        bu, bp, bq = ru[u_idx], rit[i_idx], rit[j_idx]
        score = (bu * bp).sum(1) - (bu * bq).sum(1)
        rec_loss = -torch.log(torch.sigmoid(score) + 10e-8).sum() + 0.01 * ((tu ** 2).sum() / 2 + (ti ** 2).sum() / 2)
        loss = rec_loss
        if joint:
            uq = torch.from_numpy(sept_ref.unique_first(u_idx))
            losses, pos = t_tri_nd(enc(tu, fr)[uq], enc(tu, sh)[uq], ru[uq], enc(ego, sub)[:nu][uq], k, 0.1)
            loss = rec_loss + 0.05 * sum(losses)
            assert abs(ref["nd_loss"] - sum(losses).item()) <= 1e-10 * abs(ref["nd_loss"])
            assert np.array_equal(ref["pos"], pos.numpy())
        loss.backward()
        assert abs(ref["rec_loss"] - rec_loss.item()) <= 1e-10 * abs(ref["rec_loss"])
        assert np.abs(ref["g_user"] - tu.grad.numpy()).max() <= 1e-10 * np.abs(ref["g_user"]).max()
        assert np.abs(ref["g_item"] - ti.grad.numpy()).max() <= 1e-10 * np.abs(ref["g_item"]).max()


def test_unique_first_keeps_first_occurrence_order():
    from selfrec_amd import ops
    ids = np.array([5, 2, 5, 9, 2, 0, 9, 7], dtype=np.int32)
    assert ops.unique_first(ids).tolist() == [5, 2, 9, 0, 7] == sept_ref.unique_first(ids).tolist()
    assert ops.unique_first(np.zeros(0, dtype=np.int64)).size == 0


# ---- how many cuts of the GPU cases float32 cannot call -----------------------------------------------------------------
@pytest.mark.parametrize("case", sept_cases.TRI_ND_CASES, ids=sept_cases.case_id)
def test_gpu_cases_are_mostly_unambiguous(case):
    """A (pair, row) is ambiguous when its float64 gap (t_k - t_{k+1}) / t_k is < 1e-4, ~25x the worst-case fp32 dot error
    d 2^-24 ~ 4e-6 at d = 64: at most 5 % of a case, none of a case marked clean.  Recomputed from the fp32-cast inputs."""
    n, d, k, seed, clean = case
    c = sept_cases.tri_nd_case(case)
    share = float(c["amb"].mean())
    print(f"{sept_cases.case_id(case)}: ambiguous share {share:.4f}, smallest gap {float(c['ref']['gap'].min()):.3e}")
    assert share <= sept_cases.AMBIGUOUS_SHARE
    if clean:
        assert not c["amb"].any()


@pytest.mark.parametrize("case", sept_cases.edge_cases(), ids=sept_cases.edge_id)
def test_edge_cases_are_mostly_unambiguous(case):
    """every (shape, family) of the edge suite keeps the same 5 % cap -- a condition on the cases, measured on the
    restatement alone.  `clamped`: the planted rows, and no others, are below the clamp, far from it on either side, and
    the cap holds without them too (they are checked on their own on the device, not through the allowance)."""
    (n, d, k, seed), fam = case
    c = sept_cases.edge_case(*case)
    share = float(c["amb"].mean())
    print(f"{sept_cases.edge_id(case)}: ambiguous share {share:.4f}, smallest gap {float(c['ref']['gap'].min()):.3e}")
    assert share <= sept_cases.AMBIGUOUS_SHARE
    norms = [np.sqrt((m.astype(np.float64) ** 2).sum(1)) for m in c["mats"]]
    if fam != "clamped":
        assert min(float(x.min()) for x in norms) > 1e-3
        return
    planted = sept_cases.planted_rows(n)
    assert len({r for pair in planted for r in pair}) == 8
    for m, x, (zero, tiny) in zip(c["mats"], norms, planted):
        clamped = sept_ref.l2norm(m)[2]
        assert sorted(np.flatnonzero(clamped).tolist()) == sorted((zero, tiny))
        # 1e-8 * standard_normal(d): a norm of about 1e-8 sqrt(d), at most a quarter of the clamp's 1e-6 at d = 128
        assert x[zero] == 0.0 and 0.0 < x[tiny] < 2.5e-7
        assert float(np.delete(x, (zero, tiny)).min()) > 1e-3
    rest = np.setdiff1d(np.arange(n), [r for pair in planted[:3] for r in pair])
    assert float(c["amb"][:, rest].mean()) <= sept_cases.AMBIGUOUS_SHARE


def test_padded_width_seeds_are_the_smallest_that_meet_the_cap():
    """the two zero-padded shapes carry a literal seed: the smallest of 0 ... 9 at which all four families meet the cap"""
    for shape in sept_cases.EDGE_SHAPES:
        n, d, k, seed = shape
        if d not in (100, 8):
            continue
        ok = [s for s in range(10)
              if all(float(sept_cases.edge_case((n, d, k, s), f)["amb"].mean()) <= sept_cases.AMBIGUOUS_SHARE
                     for f in sept_cases.FAMILIES)]
        assert ok and ok[0] == seed, (shape, ok)
    assert {s[1] for s in sept_cases.EDGE_SHAPES} >= {100, 8}


def test_tri_nd_restatement_against_autograd_with_clamped_rows():
    """the clamped branches of the restatement (a zero row and a row below the clamp in each view and in aug) against
    autograd on x * rsqrt(maximum(sum x^2, 1e-12)): n = 33, d = 8, k = 10, to the same 1e-10 -- absolute on ordinary
    rows, relative to the row's own 1e6-scaled entries on the planted ones"""
    n, d, k = 33, 8, 10
    mats = sept_cases.family("clamped", n, d, 3)
    planted = sept_cases.planted_rows(n)
    leaves = [torch.from_numpy(m).double().requires_grad_(True) for m in mats]
    losses, pos = t_tri_nd(*leaves, k, sept_cases.TAU)
    (0.37 * sum(losses)).backward()
    ref = sept_ref.tri_nd(*mats, k, sept_cases.TAU, loss_scale=0.37)
    assert np.array_equal(ref["pos"], pos.numpy())
    for v in range(3):
        assert abs(ref["loss"][v] - 0.37 * losses[v].item()) <= 1e-10
    for g, leaf, m, rows in zip(ref["grads"], leaves, mats, planted):
        clamped = sept_ref.l2norm(m)[2]
        assert sorted(np.flatnonzero(clamped).tolist()) == sorted(rows)
        want = leaf.grad.numpy()
        assert np.abs(g - want)[~clamped].max() <= 1e-10
        assert sept_ref.row_errors(g, want).max() <= 1e-10
        assert np.abs(want[clamped]).max(1).min() > 1e3          # the planted rows carry g * 1e6, not a projection


# ---- the float32 yardstick of the edge suite ------------------------------------------------------------------------------
YARDSTICK_ROW, YARDSTICK_LOSS = 5e-6, 1e-6


@pytest.mark.parametrize("fam", sept_cases.FAMILIES)
def test_f32_yardstick_against_the_restatement(fam):
    """sept_ref.tri_nd_f32 against sept_ref.tri_nd at the restatement's ids, per row with no floor, on every shape: what
    float32 arithmetic alone does to these inputs, and so what the device bounds rest on.  normal / scaled / clamped
    (the planted rows relative to their own 1e6-scaled entries): <= 5e-6 per row, twice the largest value measured
    (2.4e-6), 20x below GRAD_BOUND; the loss <= 1e-6 (1.5e-7 measured), 10x below LOSS_BOUND.  peaked: the loss and the
    row gradients are small differences of large terms (2.1e-4 and 1.1e-5 at the worst), so the device bound is taken
    per case from this yardstick; here only finite and below 1e-3."""
    worst_row, worst_loss = 0.0, 0.0
    for shape in sept_cases.EDGE_SHAPES:
        c = sept_cases.edge_case(shape, fam)
        y = sept_ref.tri_nd_f32(*c["mats"], shape[2], sept_cases.TAU, c["ref"]["pos"])
        row = max(float(sept_ref.row_errors(g, w).max()) for g, w in zip(y["grads"], c["ref"]["grads"]))
        loss = float(np.abs(y["loss"].astype(np.float64) / c["ref"]["loss"] - 1).max())
        print(f"{sept_cases.edge_id((shape, fam))}: yardstick row {row:.3e} loss {loss:.3e}")
        assert np.isfinite(row) and np.isfinite(loss)
        if fam == "peaked":
            assert row < 1e-3 and loss < 1e-3
        else:
            assert row <= YARDSTICK_ROW and loss <= YARDSTICK_LOSS
        worst_row, worst_loss = max(worst_row, row), max(worst_loss, loss)
    print(f"{fam}: largest yardstick row error {worst_row:.3e}, loss error {worst_loss:.3e}")


# ---- housekeeping -----------------------------------------------------------------------------------------------------------
def test_sept_is_a_model_and_its_conf_holds_the_reference_keys():
    from selfrec_amd import main
    from selfrec_amd.util.conf import ModelConf
    assert "SEPT" in main.MODELS
    conf = ModelConf(os.path.join(REPO, "conf", "SEPT.yaml")).config
    want = {"training.set": "./dataset/douban-book/train.txt", "test.set": "./dataset/douban-book/test.txt",
            "social.data": "./dataset/douban-book/trust.txt", "model": {"name": "SEPT", "type": "graph"},
            "item.ranking.topN": [10, 20], "embedding.size": 64, "max.epoch": 30, "batch.size": 2048,
            "learning.rate": 0.001, "reg.lambda": 0.0001,
            "SEPT": {"n_layer": 2, "ss_rate": 0.005, "drop_rate": 0.3, "ins_cnt": 10}, "output": "./results/"}
    assert {k: v for k, v in conf.items() if not k.startswith("engine.")} == want
    assert {k: conf[k] for k in conf if k.startswith("engine.")} == {"engine.nd": "hip", "engine.norm": "hip"}


def test_header_section_and_abi():
    text = open(os.path.join(REPO, "include", "selfrec_hip.h")).read()
    assert "(a-19) SEPT" in text
    assert re.search(r"#define SRH_ABI_VERSION 31\b", text) and _lib.ABI_VERSION == 31
    for name in ("srh_rows_l2norm_fwd_f32", "srh_rows_l2norm_bwd_f32", "srh_tri_nd_ws_bytes", "srh_tri_nd_fwd_bwd"):
        assert name in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, text)
    import ctypes as C
    assert C.sizeof(_lib.TriNdArgs) == 3 * 8 + 8 + 8 + 4 * 4 + 8 + 3 * 8 + 8 + 8


def test_engine_routes(monkeypatch):
    from selfrec_amd.model.graph import SEPT as M
    from selfrec_amd.util.conf import ModelConf
    monkeypatch.delenv("SRH_SEPT_ND", raising=False)
    monkeypatch.delenv("SRH_SEPT_NORM", raising=False)
    assert M.nd_route(None) == "hip" and M.norm_route(ModelConf({})) == "hip"
    assert M.nd_route(ModelConf({"engine.nd": "torch"})) == "torch" and M.norm_route(ModelConf({"engine.norm": "Torch"})) == "torch"
    monkeypatch.setenv("SRH_SEPT_ND", "hip")
    assert M.nd_route(ModelConf({"engine.nd": "torch"})) == "hip"
    with pytest.raises(ValueError):
        M.norm_route(ModelConf({"engine.norm": "triton"}))


def test_selfrec_passes_the_social_data(tmp_path):
    from selfrec_amd.SELFRec import SELFRec
    from selfrec_amd.util.conf import ModelConf
    for name in ("train.txt", "test.txt"):
        (tmp_path / name).write_text("a x 1\nb y 1\n")
    (tmp_path / "trust.txt").write_text("a b\nb a 1\n")
    base = {"training.set": str(tmp_path / "train.txt"), "test.set": str(tmp_path / "test.txt"),
            "model": {"name": "SEPT", "type": "graph"}}
    assert SELFRec(ModelConf(dict(base))).kwargs == {}
    got = SELFRec(ModelConf(dict(base, **{"social.data": str(tmp_path / "trust.txt")}))).kwargs
    assert got == {"social.data": [["a", "b", 1], ["b", "a", 1.0]]}
