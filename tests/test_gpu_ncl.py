"""NCL (reference model/graph/NCL.py) on the device: the table InfoNCE kernel against a float64 restatement of
NCL.py:59-82, the k-means kernels and ops.kmeans against float64 and the numpy definition (tests/ncl_ref.py), the
model against the reference-run golden (tests/golden/ncl.npz, make_golden_ncl.py), and an end-to-end run."""
import json
import os
import random

import numpy as np
import pytest
import torch

from tests import ncl_ref
from tests.test_shapes_cpu import GOLDEN

pytestmark = pytest.mark.gpu
YELP_U, YELP_I = 31668, 38048


def rel_max(got, want):
    got, want = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double().cpu()
    return float((got - want).abs().max() / (want.abs().max() + 1e-30))


def _problem(B, N, d, seed, n_pos=None):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, d, generator=g) * 0.1
    t = torch.randn(N, d, generator=g) * 0.1
    idx = torch.randint(0, n_pos or max(1, min(N, 40)), (B,), generator=g)   # heavy repeats
    return q, t, idx


def _oracle(q, t, idx, tau, scale):
    q64, t64 = q.double().cuda().requires_grad_(True), t.double().cuda().requires_grad_(True)
    loss = scale * ncl_ref.table_nce_torch(q64, t64, idx.cuda(), tau)
    loss.backward()
    return float(loss), q64.grad, t64.grad


CASES = [  # (B, N, d, tau)
    (1, 300, 64, 0.2), (257, 300, 32, 0.05), (257, 300, 128, 0.2), (2048, 300, 64, 0.05),
    (1, YELP_U, 64, 0.05), (257, YELP_I, 128, 0.2), (2048, YELP_U, 32, 0.2), (2048, YELP_I, 64, 0.05),
    (2048, YELP_I, 128, 0.05), (257, 300, 64, 0.01),
]


@pytest.mark.parametrize("B,N,d,tau", CASES)
def test_table_nce_matches_float64(B, N, d, tau):
    from selfrec_amd import ops
    torch.cuda.set_device(0)
    pu = _problem(B, N, d, 1)
    pi = _problem(max(1, B // 2), 300, d, 2)               # a second problem in the same call, its own scale
    scales = (1.0, 1.5)
    got = ops.table_nce_fwd_bwd([(pu[0].cuda(), pu[1].cuda(), pu[2].cuda(), scales[0]),
                                 (pi[0].cuda(), pi[1].cuda(), pi[2].cuda(), scales[1])], tau=tau)
    for (q, t, idx), scale, (loss, gq, gt) in zip((pu, pi), scales, got):
        wl, wq, wt = _oracle(q, t, idx, tau, scale)
        assert np.isfinite(wl)
        assert torch.isfinite(loss).item() and torch.isfinite(gq).all() and torch.isfinite(gt).all()
        assert abs(float(loss) - wl) <= 1e-5 * abs(wl), (float(loss), wl)
        assert rel_max(gq, wq) <= 1e-4, rel_max(gq, wq)
        assert rel_max(gt, wt) <= 1e-4, rel_max(gt, wt)


def test_table_nce_and_kmeans_repeat_bit_for_bit():
    from selfrec_amd import ops
    torch.cuda.set_device(0)
    pu, pi = _problem(2048, YELP_U, 64, 3), _problem(2048, YELP_I, 64, 4)
    probs = [(pu[0].cuda(), pu[1].cuda(), pu[2].cuda(), 1e-6), (pi[0].cuda(), pi[1].cuda(), pi[2].cuda(), 1.5e-6)]
    first = [tuple(x.clone() for x in r) for r in ops.table_nce_fwd_bwd(probs, tau=0.05)]
    x = (torch.randn(YELP_U, 64, generator=torch.Generator().manual_seed(5)) * 0.1).cuda()
    c0, i0 = ops.kmeans(x, 2000)
    for _ in range(19):
        again = ops.table_nce_fwd_bwd(probs, tau=0.05)
        for a, b in zip(first, again):
            for u, v in zip(a, b):
                assert torch.equal(u, v)
        c, i = ops.kmeans(x, 2000)
        assert torch.equal(c, c0) and torch.equal(i, i0)


def test_kmeans_assign_against_float64():
    from selfrec_amd import ops
    torch.cuda.set_device(0)
    g = torch.Generator().manual_seed(6)
    n, k, d = YELP_U, 2000, 64
    x, c = torch.randn(n, d, generator=g), torch.randn(k, d, generator=g)
    c[10:20] = c[0:10]                                     # exact ties: the lowest id must win
    ids, dist = ops.kmeans_assign(x.cuda(), c.cuda())
    ids, dist = ids.long().cpu().numpy(), dist.cpu().numpy()
    x64, c64 = x.double().numpy(), c.double().numpy()
    full = (x64 * x64).sum(1)[:, None] + (c64 * c64).sum(1)[None, :] - 2 * x64 @ c64.T
    best = full.argmin(1)
    assert not np.isin(ids, np.arange(10, 20)).any()
    diff = np.flatnonzero(ids != best)
    scale = (x64 * x64).sum(1) + (c64 * c64).sum(1)[best]
    gap = full[diff, ids[diff]] - full[diff, best[diff]]
    assert (gap < 1e-5 * scale[diff]).all(), gap.max() if len(gap) else None
    assert len(diff) <= n // 1000, len(diff)
    assert np.abs(dist - full[np.arange(n), ids]).max() <= 1e-5 * scale.max()


def test_kmeans_update_against_float64():
    from selfrec_amd import ops
    torch.cuda.set_device(0)
    g = torch.Generator().manual_seed(7)
    for n, k, d in ((YELP_U, 2000, 64), (1000, 37, 50)):
        x = torch.randn(n, d, generator=g)
        ids = torch.randint(0, k - 1, (n,), generator=g)       # cluster k-1 stays empty
        ids[:300] = 3                                           # one large cluster
        cent, counts = ops.kmeans_update(x.cuda(), ids.cuda(), k)
        want_c, want_n = ncl_ref.update_np(x.numpy(), ids.numpy(), k)
        assert np.array_equal(counts.cpu().numpy(), want_n)
        assert counts[k - 1].item() == 0 and torch.all(cent[k - 1] == 0)
        assert rel_max(cent, want_c) <= 1e-6


def _blobs(n, k, d, seed):
    """k tight, far-apart blobs; the k rows k-means starts from (perm[:k] of seed 1234) lie one in each blob, so no point
    sits near a tie between two centroids"""
    rs = np.random.RandomState(seed)
    centers = rs.randn(k, d).astype(np.float32) * 10
    lab = rs.randint(0, k, n)
    lab[np.random.RandomState(1234).permutation(n)[:k]] = np.arange(k)
    return (centers[lab] + 0.05 * rs.randn(n, d)).astype(np.float32)


def test_kmeans_equals_the_numpy_definition_on_blobs():
    from selfrec_amd import ops
    torch.cuda.set_device(0)
    for n, k, d in ((4000, 8, 32), (6000, 20, 64)):        # (n > 256 k: the first trains on a subsample)
        x = _blobs(n, k, d, n)
        cent, ids = ops.kmeans(torch.from_numpy(x).cuda(), k)
        want_c, want_i, _ = ncl_ref.kmeans_np(x, k)
        assert ids.dtype == torch.int64 and ids.is_cuda and cent.is_cuda and tuple(cent.shape) == (k, d)
        assert np.array_equal(ids.cpu().numpy(), want_i)
        assert rel_max(cent, want_c) <= 1e-6


def test_kmeans_on_the_golden_estep_input():
    from selfrec_amd import ops
    torch.cuda.set_device(0)
    gd = np.load(os.path.join(GOLDEN, "ncl.npz"))
    meta = json.load(open(os.path.join(GOLDEN, "ncl_meta.json")))
    for side in ("user", "item"):
        x = gd[f"warm1_param_{side}_emb"]
        cent, ids = ops.kmeans(torch.from_numpy(x).cuda(), meta["conf"]["num_clusters"])
        c64, i = cent.double().cpu().numpy(), ids.cpu().numpy()
        inertia = float(((x.astype(np.float64) - c64[i]) ** 2).sum())
        want = meta["estep_inertia"][side]
        assert abs(inertia - want) <= 1e-4 * want, (inertia, want)


def test_kmeans_objective_and_counts():
    from selfrec_amd import ops
    torch.cuda.set_device(0)
    rs = np.random.RandomState(8)
    x = rs.randn(3000, 64).astype(np.float32)
    st = {}
    ops.kmeans(torch.from_numpy(x).cuda(), 64, stats=st)
    obj = np.asarray(st["obj"])
    assert len(obj) == 25 and (np.diff(obj) <= 1e-6 * obj[:-1]).all(), obj
    assert min(st["min_count"]) >= 1
    # many duplicate rows: duplicate initial centroids, so clusters go empty and are split
    xd = rs.randn(20, 64).astype(np.float32)[rs.randint(0, 20, 600)]
    st = {}
    cent, ids = ops.kmeans(torch.from_numpy(xd).cuda(), 40, stats=st)
    assert min(st["min_count"]) >= 1
    with pytest.raises(ops.SelfrecHipError):
        ops.kmeans(torch.from_numpy(xd[:10]).cuda(), 40)


def _model(conf_block, tmp_path, monkeypatch, data, **over):
    from selfrec_amd.util.conf import ModelConf
    from selfrec_amd.model.graph.NCL import NCL
    monkeypatch.chdir(tmp_path)
    conf = ModelConf({"model": {"name": "NCL", "type": "graph"}, "item.ranking.topN": [10, 20], "embedding.size": 64,
                      "max.epoch": over.get("max_epoch", 1), "batch.size": 1024, "learning.rate": 0.001,
                      "reg.lambda": 0.0001, "output": "./results/", "training.set": "x", "test.set": "y",
                      "NCL": dict(conf_block)})
    return NCL(conf, data.training_data, data.test_data)


def test_model_matches_the_reference_golden(fresh_tiny_data, tmp_path, monkeypatch):
    gd = np.load(os.path.join(GOLDEN, "ncl.npz"))
    meta = json.load(open(os.path.join(GOLDEN, "ncl_meta.json")))
    torch.manual_seed(meta["torch_seed"]); np.random.seed(meta["numpy_seed"]); random.seed(meta["sampler_seed"])
    model = _model(meta["conf"], tmp_path, monkeypatch, fresh_tiny_data)
    enc = model.model.cuda()
    for k, v in enc.embedding_dict.items():
        assert np.array_equal(v.detach().cpu().numpy(), gd[f"init_{k}"]), k
    opt = torch.optim.Adam(enc.parameters(), lr=model.lRate)
    batch = [tuple(torch.from_numpy(gd[f"batch{b}_{c}"].astype(np.int64)).cuda() for c in "uij") for b in range(3)]

    def step(b, proto):
        rec, ssl, pro, total = model.batch_losses(*batch[b], proto)
        opt.zero_grad()
        total.backward()
        opt.step()
        return [float(t) for t in ((rec, ssl, pro, total) if proto else (rec, ssl, total))]

    for s in range(2):
        got, want = step(s, False), gd[f"warm{s}_loss"]
        for a, w in zip(got, want):
            assert abs(a - w) <= 1e-5 * abs(w), (s, got, want)
        for k, v in enc.embedding_dict.items():
            assert rel_max(v.detach(), gd[f"warm{s}_param_{k}"]) <= 1e-4, (s, k)
    model.user_centroids = torch.from_numpy(gd["estep_user_centroids"]).cuda()
    model.user_2cluster = torch.from_numpy(gd["estep_user_2cluster"]).cuda()
    model.item_centroids = torch.from_numpy(gd["estep_item_centroids"]).cuda()
    model.item_2cluster = torch.from_numpy(gd["estep_item_2cluster"]).cuda()
    got, want = step(2, True), gd["proto_loss"]
    for a, w in zip(got, want):
        assert abs(a - w) <= 1e-5 * abs(w), (got, want)
    for k, v in enc.embedding_dict.items():
        assert rel_max(v.detach(), gd[f"proto_param_{k}"]) <= 1e-4, k
    ctx = torch.from_numpy(gd["sslgrad_context"]).cuda().requires_grad_(True)
    ini = torch.from_numpy(np.concatenate([gd["proto_param_user_emb"], gd["proto_param_item_emb"]])).cuda().requires_grad_(True)
    loss = model.ssl_layer_loss(ctx, ini, batch[0][0], batch[0][1])
    loss.backward()
    assert abs(float(loss) - gd["sslgrad_loss"][0]) <= 1e-5 * abs(gd["sslgrad_loss"][0])
    assert rel_max(ctx.grad, gd["sslgrad_d_context"]) <= 1e-4
    assert rel_max(ini.grad, gd["sslgrad_d_initial"]) <= 1e-4


def test_ncl_end_to_end(tmp_path, monkeypatch, capsys):
    from selfrec_amd import synth
    from selfrec_amd.SELFRec import SELFRec
    from selfrec_amd.util.conf import ModelConf
    from selfrec_amd.model.graph import NCL as ncl_mod
    from selfrec_amd.base import graph_recommender
    torch.cuda.set_device(0)
    monkeypatch.chdir(tmp_path)
    u, i = synth.generate_edges(200, 300, 3600, 11)
    (tu, ti), (su, si) = synth.split_train_test(u, i, 200, 300, 0.2, 11)
    synth.write_text(str(tmp_path / "train.txt"), tu, ti)
    synth.write_text(str(tmp_path / "test.txt"), su, si)
    conf = ModelConf({"model": {"name": "NCL", "type": "graph"}, "item.ranking.topN": [10, 20], "embedding.size": 64,
                      "max.epoch": 3, "batch.size": 1024, "learning.rate": 0.001, "reg.lambda": 0.0001,
                      "output": "./results/", "training.set": str(tmp_path / "train.txt"),
                      "test.set": str(tmp_path / "test.txt"),
                      "NCL": {"n_layer": 3, "ssl_reg": "1e-6", "proto_reg": "1e-7", "tau": 0.05, "hyper_layers": 1,
                              "alpha": 1.5, "num_clusters": 16}})
    monkeypatch.setattr(ncl_mod.NCL, "warm_up_epochs", 1)
    calls, losses, reports = [], [], []
    real_e, real_b = ncl_mod.NCL.e_step, ncl_mod.NCL.batch_losses
    monkeypatch.setattr(ncl_mod.NCL, "e_step", lambda self: (calls.append(1), real_e(self))[1])

    def spy(self, *a):
        out = real_b(self, *a)
        losses.append([float(t) for t in out if t is not None])
        return out
    monkeypatch.setattr(ncl_mod.NCL, "batch_losses", spy)
    real_r = graph_recommender.ranking_evaluation
    monkeypatch.setattr(graph_recommender, "ranking_evaluation", lambda *a: (lambda r: (reports.append(r), r)[1])(real_r(*a)))
    SELFRec(conf).execute()
    assert len(calls) == 2
    assert losses and np.isfinite(np.asarray(losses[-1])).all() and len(losses[-1]) == 4
    final = reports[-1]
    assert [ln.split(':')[0] for ln in final] == ['Top 10\n', 'Hit Ratio', 'Precision', 'Recall', 'NDCG',
                                                 'Top 20\n', 'Hit Ratio', 'Precision', 'Recall', 'NDCG']
    for ln in final:
        if ':' in ln:
            float(ln.split(':')[1])
    assert 'Real-Time Ranking Performance' in capsys.readouterr().out
