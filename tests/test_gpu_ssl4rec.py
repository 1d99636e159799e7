"""SSL4Rec (reference model/graph/SSL4Rec.py) on the device: batch softmax and the tower kernels against float64
restatements (tests/ssl4rec_ref.py), the in-kernel dropout masks bit for bit against the host restatement, the model
against the reference-run golden (tests/golden/ssl4rec.npz, make_golden_ssl4rec.py) under its recorded masks,
repeatability at the Yelp2018 shape, and an end-to-end run."""
import json
import os
import random

import numpy as np
import pytest
import torch

from tests import ssl4rec_ref
from tests.test_shapes_cpu import GOLDEN

pytestmark = pytest.mark.gpu
YELP_U, YELP_I = 31668, 38048


def rel_max(got, want):
    got, want = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double().cpu()
    return float((got - want).abs().max() / (want.abs().max() + 1e-30))


@pytest.mark.parametrize("B", [1, 257, 2048, 4096])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("tau", [0.07, 0.2])
def test_batch_softmax_matches_float64(B, d, tau):
    from selfrec_amd import ops
    torch.cuda.set_device(0)
    g = torch.Generator().manual_seed(B + d)
    u = torch.randn(B, d, generator=g) * 0.1
    v = torch.randn(B, d, generator=g) * 0.1
    v[::3] = -u[::3] + 0.01 * v[::3]            # a third of the rows with p_bb far below 1e-5: the weight w_b matters
    loss, gu, gv = ops.batch_softmax_fwd_bwd(u.cuda(), v.cuda(), tau)
    u64, v64 = u.double().requires_grad_(True), v.double().requires_grad_(True)
    want = ssl4rec_ref.batch_softmax(u64, v64, tau)
    want.backward()
    if B > 1 and tau == 0.07:
        un, vn = torch.nn.functional.normalize(u64.detach(), dim=1), torch.nn.functional.normalize(v64.detach(), dim=1)
        p = torch.softmax(un @ vn.T / tau, dim=1).diagonal()
        assert float(p.min()) < 1e-7
    want = float(want.detach())
    # (+1e-6: at B = 1 the loss is -log(1 + 1e-5) and p_bb = 1 to within the f32 rounding of two dot products)
    assert abs(float(loss) - want) <= 1e-5 * abs(want) + 1e-6, (float(loss), want)
    for got, ref in ((gu, u64.grad), (gv, v64.grad)):
        # (at B = 1 the exact gradient is zero and the kernel's is f32 rounding: measured against a floor of 1e-2)
        err = float((got.double().cpu() - ref).abs().max())
        assert err <= 1e-4 * max(float(ref.abs().max()), 1e-2), err


def _tower_weights(seed):
    lin1, lin2 = torch.nn.Linear(64, 1024), torch.nn.Linear(1024, 128)
    torch.manual_seed(seed)
    for m in (lin1, lin2):
        torch.nn.init.uniform_(m.weight, -0.08, 0.08)
        torch.nn.init.uniform_(m.bias, -0.05, 0.05)
    return [t.detach().cuda() for t in (lin1.weight, lin1.bias, lin2.weight, lin2.bias)]


@pytest.mark.parametrize("n", [1, 255, 2048, 6144])
@pytest.mark.parametrize("masked", [False, True])
def test_tower_fwd_bwd_matches_float64(n, masked):
    from selfrec_amd import ops
    torch.cuda.set_device(0)
    g = torch.Generator().manual_seed(n)
    N = 500
    table = (torch.randn(N, 64, generator=g) * 0.2).cuda()
    ids = torch.randint(0, 40, (n,), generator=g).numpy()            # heavy repeats
    w = _tower_weights(n)
    row0 = n // 3 if masked else None
    keep = (torch.rand(n - n // 3, 64, generator=g) >= 0.1).to(torch.uint8) if masked else None
    idx = torch.from_numpy(ids).cuda()
    plan = ops.scatter_plan(ids, table.device)
    tab = table.clone().requires_grad_(True)
    ws = [t.clone().requires_grad_(True) for t in w]
    y = ops.TowerFn.apply(tab, *ws, idx, plan, row0, None if keep is None else keep.cuda(), 0.1, 0, 0, None)
    gy = torch.randn(n, 128, generator=g)
    y.backward(gy.cuda())
    # float64
    t64 = table.double().cpu().requires_grad_(True)
    w64 = [t.double().cpu().requires_grad_(True) for t in w]
    x = t64[torch.from_numpy(ids)]
    if masked:
        m = torch.ones(n, 64, dtype=torch.float64)
        m[row0:] = keep.double() / (1.0 - 0.1)
        x = x * m
    y64 = ssl4rec_ref.tower(x, *w64)
    y64.backward(gy.double())
    assert rel_max(y, y64) <= 1e-5
    assert rel_max(tab.grad, t64.grad) <= 1e-4
    for a, b in zip(ws, w64):
        assert rel_max(a.grad, b.grad) <= 1e-4


def test_in_kernel_masks_match_the_host_restatement():
    from selfrec_amd import ops
    torch.cuda.set_device(0)
    B, p, seed, ctr = 2048, 0.1, 0x5EED_0123_4567, 3 * 4096
    table = torch.randn(300, 64).cuda()
    w = _tower_weights(1)
    idx = torch.randint(0, 300, (3 * B,)).cuda()
    _, saved = ops.tower_fwd(table, idx, *w, mask_row0=B, drop_p=p, rng_seed=seed, rng_counter=ctr)
    keep = saved[2].cpu().numpy().astype(bool)
    want = ssl4rec_ref.dropout_keep(seed, ctr, 2 * B, p)
    assert np.array_equal(keep, want)
    assert not np.array_equal(keep[:B], keep[B:])
    x = saved[0].cpu()
    ref = table.cpu()[idx.cpu()]
    scale = np.float32(1.0) / np.float32(1.0 - p)
    assert torch.equal(x[:B], ref[:B])
    assert torch.equal(x[B:], ref[B:] * torch.from_numpy(keep.astype(np.float32)) * float(scale))


def _model(meta, tmp_path, monkeypatch, data, **over):
    from selfrec_amd.util.conf import ModelConf
    from selfrec_amd.model.graph.SSL4Rec import SSL4Rec
    monkeypatch.chdir(tmp_path)
    conf = ModelConf({"model": {"name": "SSL4Rec", "type": "graph"}, "item.ranking.topN": [10, 20],
                      "embedding.size": 64, "max.epoch": over.get("max_epoch", 1), "batch.size": meta["batch"],
                      "learning.rate": meta["lr"], "reg.lambda": meta["reg"], "output": "./results/",
                      "training.set": "x", "test.set": "y", "SSL4Rec": dict(meta["conf"])})
    return SSL4Rec(conf, data.training_data, data.test_data)


def test_model_matches_the_reference_golden(fresh_tiny_data, tmp_path, monkeypatch):
    from selfrec_amd.util.evaluation import ranking_evaluation
    gd = np.load(os.path.join(GOLDEN, "ssl4rec.npz"))
    meta = json.load(open(os.path.join(GOLDEN, "ssl4rec_meta.json")))
    torch.cuda.set_device(0)
    torch.manual_seed(meta["torch_seed"]); np.random.seed(meta["numpy_seed"]); random.seed(meta["sampler_seed"])
    model = _model(meta, tmp_path, monkeypatch, fresh_tiny_data)
    enc = model.model.cuda()
    assert np.array_equal(enc.initial_user_emb.detach().cpu().numpy(), gd["init_user_emb"])
    params = dict(enc.named_parameters())
    opt = torch.optim.Adam(enc.parameters(), lr=model.lRate)
    for s in range(3):
        B = gd[f"batch{s}_i"].size
        keep = np.unpackbits(gd[f"step{s}_mask"], axis=-1)[..., :64]
        rec, cl, total = model.batch_losses(gd[f"batch{s}_q"], gd[f"batch{s}_i"], masks=keep.reshape(2 * B, 64))
        opt.zero_grad()
        total.backward()
        if s == 0:
            for name, p in params.items():
                got = p.grad.reshape(-1).cpu().numpy()[gd[f"sample_{name}"]]
                want = gd[f"grad0_{name}_val"]
                assert np.abs(got - want).max() <= 1e-4 * np.abs(want).max() + 1e-12, name
        opt.step()
        for got, want in zip((rec, cl, total), gd[f"step{s}_loss"]):
            assert abs(float(got) - want) <= 1e-5 * abs(want), (s, float(got), want)
        # Adam's first steps move an element by about lr * g / (|g| + eps): where |g| is near eps (1e-8) a gradient
        # that differs in the last bits moves the element by a different fraction of lr, so the parameters are held
        # to half of lr (5e-4), absolute; the losses above pin the trajectory to 1e-5
        tol = 0.5 * model.lRate
        assert float((enc.initial_user_emb.detach().cpu() - torch.from_numpy(gd[f"step{s}_user_emb"])).abs().max()) <= tol, s
        assert float((enc.initial_item_emb.detach().cpu() - torch.from_numpy(gd[f"step{s}_item_emb"])).abs().max()) <= tol, s
        for name in ssl4rec_ref.TOWER_KEYS:
            for side in ("user_tower", "item_tower"):
                key = f"{side}.{name}"
                v = params[key].detach().reshape(-1).cpu()
                want = gd[f"step{s}_{key}_val"]
                assert np.abs(v.numpy()[gd[f"sample_{key}"]] - want).max() <= tol, (s, key)
                assert abs(float(v.double().sum()) - gd[f"step{s}_{key}_sum"][0]) <= 1e-4 * float(v.abs().sum()), (s, key)
    enc.eval()
    with torch.no_grad():
        q, i = enc(None, None)
    assert rel_max(q, gd["eval_query_emb"]) <= 1e-3 and rel_max(i, gd["eval_item_emb"]) <= 1e-3
    # ranking: test() on the golden's own embeddings gives the reference's rec lists and evaluation strings
    model.query_emb = torch.from_numpy(gd["eval_query_emb"]).cuda()
    model.item_emb = torch.from_numpy(gd["eval_item_emb"]).cuda()
    rec = model.test()
    d = model.data
    for r, user in enumerate(gd["test_users"].tolist()):
        assert [d.item[it] for it, _ in rec[user]] == gd["rec_items"][r].tolist(), user
        assert np.allclose([s for _, s in rec[user]], gd["rec_scores"][r], rtol=1e-5, atol=1e-6), user
    assert ranking_evaluation(d.test_set, rec, model.topN) == meta["ranking_evaluation"]


def _yelp_trainer(seed):
    import types
    from selfrec_amd.model.graph.SSL4Rec import DNN_Encoder
    from selfrec_amd.util.loss_torch import InfoNCE, batch_softmax_loss, l2_reg_loss
    torch.manual_seed(seed)
    enc = DNN_Encoder(types.SimpleNamespace(user_num=YELP_U, item_num=YELP_I), 64, 0.1, 0.07).cuda()
    opt = torch.optim.Adam(enc.parameters(), lr=1e-3)
    rs = np.random.RandomState(seed)

    def step():
        q, x = rs.randint(0, YELP_U, 2048), rs.randint(0, YELP_I, 2048)
        qe, ie, (v1, v2) = enc.encode_batch(q, x)
        loss = batch_softmax_loss(qe, ie, 0.07) + l2_reg_loss(1e-4, qe, ie) + 0.1 * InfoNCE(v1, v2, 0.07)
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss.detach()
    return enc, step


def test_training_repeats_bit_for_bit_at_the_yelp_shape():
    torch.cuda.set_device(0)
    runs = []
    for _ in range(2):
        enc, step = _yelp_trainer(7)
        losses = [step() for _ in range(4)]
        runs.append(([l.clone() for l in losses], {k: v.detach().clone() for k, v in enc.state_dict().items()}))
    (l0, s0), (l1, s1) = runs
    assert all(torch.equal(a, b) for a, b in zip(l0, l1))
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k


def test_ssl4rec_end_to_end(tmp_path, monkeypatch, capsys):
    import sys
    from selfrec_amd import main, synth
    torch.cuda.set_device(0)
    monkeypatch.chdir(tmp_path)
    u, i = synth.generate_edges(200, 300, 3600, 11)
    (tu, ti), (su, si) = synth.split_train_test(u, i, 200, 300, 0.2, 11)
    synth.write_text(str(tmp_path / "train.txt"), tu, ti)
    synth.write_text(str(tmp_path / "test.txt"), su, si)
    conf = tmp_path / "SSL4Rec.yaml"
    conf.write_text("\n".join([
        f"training.set: {tmp_path / 'train.txt'}", f"test.set: {tmp_path / 'test.txt'}",
        "model:", "  name: SSL4Rec", "  type: graph", "item.ranking.topN: [10,20]", "embedding.size: 64",
        "max.epoch: 1", "batch.size: 1024", "learning.rate: 0.001", "reg.lambda: 0.0001",
        "SSL4Rec:", "  tau: 0.07", "  alpha: 0.1", "  drop: 0.1", "output: ./results/"]) + "\n")
    monkeypatch.setattr(sys, "argv", ["main"])
    main.main(["SSL4Rec", "--conf", str(conf)])
    out = capsys.readouterr().out
    assert "training: 1 batch 0 rec_loss:" in out and "cl_loss" in out
    assert "Hit Ratio" in out and "NDCG" in out
