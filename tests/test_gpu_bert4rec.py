"""BERT4Rec on the device: the fused full (unmasked) attention and the table cross-entropy kernel against the float64
restatement (tests/bert4rec_ref.py, pinned to the reference by tests/test_bert4rec_cpu.py), the in-kernel dropout mask
over the FULL row against the host restatement of the counter RNG, repeatability, the model against the reference-run
golden by both routes, an end-to-end run, and the envelope.

Bounds: outputs and losses <= 1e-5, gradients <= 1e-4, each of its tensor's largest magnitude;
parameters after an Adam step within lr / 2."""
import ctypes as C
import functools
import json
import os
import random

import numpy as np
import pytest
import torch

from tests import bert4rec_ref, seq_attn_ref
from tests.test_shapes_cpu import GOLDEN

pytestmark = pytest.mark.gpu

ATTN_SHAPES = [(1, 1, 1, 64), (3, 7, 1, 64), (2, 16, 1, 64), (2, 17, 2, 32), (2, 33, 2, 64), (5, 50, 1, 64), (4, 64, 2, 32),
               # the remaining tile edges, and the head layouts where the head offset and the row stride differ
               (2, 31, 3, 32), (2, 32, 4, 32), (2, 48, 1, 32), (2, 49, 2, 64), (2, 63, 1, 64)]
DROP_P = 0.2


def rel_err(got, want):
    """largest error as a fraction of the tensor's largest magnitude"""
    want = want.double().cpu()
    return float((got.double().cpu() - want).abs().max() / want.abs().max().clamp_min(1e-300))


@functools.lru_cache(maxsize=None)
def attn_case(shape, masked):
    """inputs (float32, host), the keep mask and the float64 output and gradients, computed once per case; q scaled as in
    tests/test_gpu_sasrec.attn_case: logits of several units, so near-one-hot rows occur"""
    B, L, H, dh = shape
    g = torch.Generator().manual_seed(2000 * B + 10 * L + H + (5 if masked else 0))
    q = 8.0 * torch.randn(B, L, H * dh, generator=g)
    k, v, go = (torch.randn(B, L, H * dh, generator=g) for _ in range(3))
    keep = (torch.rand(B, H, L, L, generator=g) >= DROP_P) if masked else None
    q64, k64, v64 = (t.double().requires_grad_(True) for t in (q, k, v))
    out = bert4rec_ref.attention(q64, k64, v64, H, None if keep is None else keep.numpy(), DROP_P)
    out.backward(go.double())
    p = torch.softmax(q64.detach()[..., :dh] @ k64.detach()[..., :dh].transpose(1, 2) / dh ** 0.5, -1)
    return dict(q=q, k=k, v=v, go=go, keep=keep, out=out.detach(), gq=q64.grad, gk=k64.grad, gv=v64.grad,
                lse=seq_attn_ref.lse(q, k, H, False), peak=float(p.max()))


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "keep"])
@pytest.mark.parametrize("shape", ATTN_SHAPES, ids=lambda s: "B%d_L%d_H%d_dh%d" % s)
def test_full_attention_forward_and_backward_match_float64(shape, masked):
    from selfrec_amd import ops
    B, L, H, dh = shape
    c = attn_case(shape, masked)
    if L >= 7:
        assert c["peak"] > 0.99                                   # a near-one-hot softmax row is among the inputs
    dev = torch.device("cuda:0")
    q, k, v, go = (c[n].to(dev) for n in ("q", "k", "v", "go"))
    keep = None if c["keep"] is None else c["keep"].to(dev)
    kw = dict(keep=keep, drop_p=DROP_P if masked else 0.0)
    out, lse = ops.seq_attn_full_fwd(q, k, v, H, **kw)
    gq, gk, gv = ops.seq_attn_full_bwd(q, k, v, lse, go, H, **kw)
    if L == 1:
        # the softmax of one key is the constant 1: dQ = dK = 0 in exact arithmetic, and the kernel returns exact zeros
        assert not c["gq"].any() and not c["gk"].any() and not gq.any() and not gk.any()
        errs = dict(out=rel_err(out, c["out"]), gq=0.0, gk=0.0, gv=rel_err(gv, c["gv"]))
    else:
        errs = dict(out=rel_err(out, c["out"]), gq=rel_err(gq, c["gq"]), gk=rel_err(gk, c["gk"]), gv=rel_err(gv, c["gv"]))
    errs["lse"] = rel_err(lse, c["lse"])
    print(shape, masked, errs)
    assert errs["out"] <= 1e-5 and errs["lse"] <= 1e-5, errs
    assert max(errs["gq"], errs["gk"], errs["gv"]) <= 1e-4, errs
    # the autograd wrapper is the same two calls
    qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
    oa = ops.SeqAttnFullFn.apply(qa, ka, va, H, keep, kw["drop_p"], 0, 0)
    oa.backward(go)
    assert torch.equal(oa.detach(), out) and torch.equal(qa.grad, gq) and torch.equal(ka.grad, gk) and torch.equal(va.grad, gv)


def test_in_kernel_dropout_mask_is_the_counter_rng_over_the_full_row():
    """V = I and Q = 0 make row i of the output P~[i, :]: uniform 1 / L over ALL j < L times the dropout multiplier -- the
    keep mask read back equals the host restatement bit for bit, the columns beyond the diagonal included"""
    from selfrec_amd import ops
    B, L, H, dh = 3, 50, 2, 64
    dev = torch.device("cuda:0")
    seed, ctr = 0x5DEECE66D1234, (1 << 33) + 12345
    q = torch.zeros(B, L, H * dh, device=dev)
    v = torch.zeros(B, L, H, dh, device=dev)
    v[:, torch.arange(L), :, torch.arange(L)] = 1.0
    v = v.reshape(B, L, H * dh)
    outs = []
    for call in range(2):
        c0 = ctr + call * B * H * L                                # the advance per call the header states
        out, _ = ops.seq_attn_full_fwd(q, q, v, H, drop_p=DROP_P, rng_seed=seed, rng_counter=c0)
        pt = out.reshape(B, L, H, dh)[..., :L].permute(0, 2, 1, 3).cpu().numpy()       # (B, H, i, j)
        want = bert4rec_ref.attn_keep_drawn(seed, c0, B, H, L, DROP_P)
        assert np.array_equal(pt > 0, want)
        assert np.allclose(pt, want * ((1.0 / (1.0 - DROP_P)) / L), rtol=1e-6)
        assert not out.reshape(B, L, H, dh)[..., L:].any()
        assert abs(1.0 - want.mean() - DROP_P) < 0.03
        outs.append(out)
    q2, v2 = torch.cat([q, q]), torch.cat([v, v])
    both, _ = ops.seq_attn_full_fwd(q2, q2, v2, H, drop_p=DROP_P, rng_seed=seed, rng_counter=ctr)
    assert torch.equal(both, torch.cat(outs))                      # consecutive calls: disjoint, adjacent counters


@functools.lru_cache(maxsize=None)
def ce_reference(shape, family):
    h, table, labels = bert4rec_ref.ce_case(shape, family)
    return (h, table, labels) + bert4rec_ref.table_ce_grads(h, table, labels)


@pytest.mark.parametrize("family", bert4rec_ref.CE_FAMILIES)
@pytest.mark.parametrize("shape", bert4rec_ref.CE_SHAPES, ids=lambda s: "M%d_N%d_d%d" % s)
def test_table_ce_matches_float64(shape, family):
    from selfrec_amd import ops
    M, N, d = shape
    h, table, labels, want_loss, want_gh, want_gt = ce_reference(shape, family)
    dev = torch.device("cuda:0")
    hd, td, ld = h.to(dev), table.to(dev), labels.to(dev, torch.int32)
    for scale in (1.0, 1.0 / (M * M)):
        loss, gh, gt = ops.table_ce_fwd_bwd(hd, td, ld, scale)
        assert gh.shape == (M, d) and gt.shape == (N, d) and loss.dtype == torch.float64
        assert torch.isfinite(gh).all() and torch.isfinite(gt).all()
        errs = dict(loss=abs(float(loss) - scale * want_loss) / abs(scale * want_loss),
                    gh=rel_err(gh, scale * want_gh), gt=rel_err(gt, scale * want_gt))
        print(shape, family, scale, errs)
        assert errs["loss"] <= 1e-5, errs
        assert errs["gh"] <= 1e-4 and errs["gt"] <= 1e-4, errs
    # the autograd wrapper: the same loss and gradients, scaled by the upstream scalar
    ha, ta = hd.clone().requires_grad_(True), td.clone().requires_grad_(True)
    out = ops.TableCeFn.apply(ha, ta, ld, 1.0)
    (2.0 * out).backward()
    loss, gh, gt = ops.table_ce_fwd_bwd(hd, td, ld, 1.0)
    assert abs(float(out) - want_loss) <= 1e-5 * abs(want_loss)
    assert torch.equal(ha.grad, 2.0 * gh) and torch.equal(ta.grad, 2.0 * gt)


def test_table_ce_pads_narrow_rows():
    from selfrec_amd import ops
    dev = torch.device("cuda:0")
    h, table, labels = bert4rec_ref.ce_case((5, 83, 64), "ordinary")
    h, table = h[:, :48].contiguous(), table[:, :48].contiguous()
    want_loss, want_gh, want_gt = bert4rec_ref.table_ce_grads(h, table, labels)
    loss, gh, gt = ops.table_ce_fwd_bwd(h.to(dev), table.to(dev), labels.to(dev, torch.int32), 1.0)
    assert gh.shape == (5, 48) and gt.shape == (83, 48)
    assert abs(float(loss) - want_loss) <= 1e-5 * abs(want_loss)
    assert rel_err(gh, want_gh) <= 1e-4 and rel_err(gt, want_gt) <= 1e-4


def test_new_entry_points_return_the_same_bits_twice():
    from selfrec_amd import ops
    dev = torch.device("cuda:0")
    c = attn_case((5, 50, 1, 64), True)
    q, k, v, go, keep = (c[n].to(dev) for n in ("q", "k", "v", "go", "keep"))
    runs = []
    for _ in range(2):
        out, lse = ops.seq_attn_full_fwd(q, k, v, 1, keep=keep, drop_p=DROP_P)
        runs.append((out, lse) + ops.seq_attn_full_bwd(q, k, v, lse, go, 1, keep=keep, drop_p=DROP_P))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    for family in bert4rec_ref.CE_FAMILIES:
        h, table, labels = bert4rec_ref.ce_case((300, 5000, 64), family)
        args = (h.to(dev), table.to(dev), labels.to(dev, torch.int32), 1.0 / 90000)
        first, second = ops.table_ce_fwd_bwd(*args), ops.table_ce_fwd_bwd(*args)
        assert all(torch.equal(x, y) for x, y in zip(first, second))


def test_envelope_violations_are_refused_before_any_launch():
    """L = 65, dh = 16 and d = 48 unpadded: SRH_ERR_UNSUPPORTED (-3) with a message; the arguments are validated before
    any launch, so the (tiny, valid) buffers are never touched"""
    from selfrec_amd import _lib, ops
    dev = torch.device("cuda:0")
    for B, L, H, dh in ((2, 65, 1, 64), (2, 16, 1, 16), (2, 16, 4, 64)):
        q = torch.zeros(B, L, H * dh, device=dev)
        with pytest.raises(ops.SelfrecHipError, match=r"\(-3\)"):
            ops.seq_attn_full_fwd(q, q, q, H)
        with pytest.raises(ops.SelfrecHipError, match=r"\(-3\)"):
            ops.seq_attn_full_bwd(q, q, q, torch.zeros(B, H, L, device=dev), q, H)
    lib = _lib.load()
    assert lib.srh_table_ce_ws_bytes(5, 83, 48) == 0 and lib.srh_table_ce_ws_bytes(5, 83, 64) > 0
    h, t = torch.full((5, 48), 7.0, device=dev), torch.full((83, 48), 7.0, device=dev)
    lab = torch.zeros(5, dtype=torch.int32, device=dev)
    loss = torch.full((), 7.0, dtype=torch.float64, device=dev)
    gh, gt, ws = torch.full_like(h, 7.0), torch.full_like(t, 7.0), torch.zeros(4096, dtype=torch.uint8, device=dev)
    status = lib.srh_table_ce_fwd_bwd(h.data_ptr(), 5, t.data_ptr(), 83, 48, lab.data_ptr(), C.c_float(1.0), loss.data_ptr(),
                                      gh.data_ptr(), gt.data_ptr(), ws.data_ptr(), None)
    assert status == -3
    with pytest.raises(ops.SelfrecHipError, match=r"\(-3\).*d=48"):
        _lib.check(status, "srh_table_ce_fwd_bwd")
    torch.cuda.synchronize()
    assert float(loss) == 7.0 and bool((gh == 7.0).all()) and bool((gt == 7.0).all())      # nothing was written


# ---- the model ----------------------------------------------------------------------------------------------------------
def golden():
    return np.load(os.path.join(GOLDEN, "bert4rec.npz")), json.load(open(os.path.join(GOLDEN, "bert4rec_meta.json")))


def train_step(model, optimizer, gd, s):
    from selfrec_amd.util.loss_torch import l2_reg_loss
    aug, pos, masked, labels = (gd[f"train{s}_{k}"] for k in ("aug", "pos", "masked", "labels"))
    net = model.model
    net.train()
    seq_emb = net.forward(aug, pos)
    batch_loss = model.calculate_loss(seq_emb, masked, labels) + l2_reg_loss(model.reg, net.item_emb)
    optimizer.zero_grad()
    batch_loss.backward()
    return batch_loss


@pytest.mark.parametrize("heads", [1, 2])
def test_model_matches_the_reference_golden(heads, tmp_path, monkeypatch):
    from selfrec_amd.util.evaluation import ranking_evaluation
    from tests.test_bert4rec_cpu import make_model
    gd, meta = golden()
    torch.cuda.set_device(0)
    torch.manual_seed(meta["torch_seed"])
    model = make_model(meta, heads, tmp_path, monkeypatch)
    net = model.model.cuda()
    params = dict(net.named_parameters())
    assert net.uses_kernel(meta["conf"]["max_len"]) and model.uses_ce_kernel()
    for name, p in params.items():
        assert np.array_equal(p.detach().cpu().numpy(), gd[f"init_{name}"]), name
    optimizer = torch.optim.Adam(net.parameters(), lr=model.lRate)
    lr = model.lRate
    kernel_losses = []
    for s in range(3):
        loss = train_step(model, optimizer, gd, s)
        want = gd[f"h{heads}_loss"][s]
        kernel_losses.append(float(loss.detach()))
        print("step", s, kernel_losses[-1], want)
        assert abs(kernel_losses[-1] - want) <= 1e-5 * abs(want), (s, kernel_losses[-1], want)
        if s == 0:
            for name, p in params.items():
                g = p.grad.reshape(-1).cpu().numpy().astype(np.float64)
                want_g = gd[f"h{heads}_grad0_{name}_val"].astype(np.float64)
                err = np.abs(g[gd[f"sample_{name}"]] - want_g).max()
                assert err <= 1e-4 * np.abs(want_g).max() + 1e-12, (name, err)
        optimizer.step()
        # Adam's first steps move every element by about lr whatever its gradient: within lr / 2
        for name, p in params.items():
            v = p.detach().reshape(-1).cpu().numpy()
            if s < 2:
                assert np.abs(v[gd[f"sample_{name}"]] - gd[f"h{heads}_step{s}_{name}_val"]).max() <= lr / 2, (s, name)
            else:
                assert np.abs(v - gd[f"h{heads}_final_{name}"].reshape(-1)).max() <= lr / 2, (s, name)
    # test() on the golden's final parameters: its lists and its evaluation strings, ranked on the device
    with torch.no_grad():
        for name, p in params.items():
            p.copy_(torch.from_numpy(gd[f"h{heads}_final_{name}"]))
    net.eval()
    assert model.item_table().shape[0] == meta["item_num"] + 2
    rec = model.test()
    d = model.data
    names = [n for n, _ in d.original_seq]
    want_ids, want_sc = gd[f"h{heads}_rec_ids"], gd[f"h{heads}_rec_scores"]
    scale = np.abs(want_sc).max()
    for r, n in enumerate(names):
        keep = want_ids[r] >= 0
        assert [d.item[it] for it, _ in rec[n]] == want_ids[r][keep].tolist(), n
        assert np.abs(np.asarray([sc for _, sc in rec[n]]) - want_sc[r][keep]).max() <= 1e-5 * scale, n
    ev = meta[f"h{heads}_evaluation"]
    assert ranking_evaluation(d.test_set, rec, model.topN) == ev["topN"]
    assert ranking_evaluation(d.test_set, rec, [model.max_N]) == ev["maxN"]
    # both engine routes through torch: the same three losses within the loss bound
    torch.manual_seed(meta["torch_seed"])
    partner = make_model(meta, heads, tmp_path, monkeypatch, attention="torch", ce="torch")
    pnet = partner.model.cuda()
    assert not pnet.uses_kernel(meta["conf"]["max_len"]) and not partner.uses_ce_kernel()
    popt = torch.optim.Adam(pnet.parameters(), lr=partner.lRate)
    for s in range(3):
        loss = float(train_step(partner, popt, gd, s).detach())
        popt.step()
        print("torch routes, step", s, loss, kernel_losses[s])
        assert abs(loss - kernel_losses[s]) <= 1e-5 * abs(kernel_losses[s]), (s, loss, kernel_losses[s])


def test_bert4rec_end_to_end(tmp_path, monkeypatch, capsys):
    from selfrec_amd import synth
    from selfrec_amd.SELFRec import SELFRec
    from selfrec_amd.model.sequential import BERT4Rec as mod
    from selfrec_amd.util.conf import ModelConf
    torch.cuda.set_device(0)
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("SRH_SASREC_ATTN", raising=False)
    monkeypatch.delenv("SRH_BERT4REC_CE", raising=False)
    train, test = synth.make_sequence_dataset("tiny-seq")
    synth.write_sequences(str(tmp_path / "train.txt"), train)
    synth.write_sequences(str(tmp_path / "test.txt"), test)
    path = tmp_path / "BERT4Rec.yaml"
    path.write_text("\n".join([
        f"training.set: {tmp_path / 'train.txt'}", f"test.set: {tmp_path / 'test.txt'}", "model:", "  name: BERT4Rec",
        "  type: sequential", "item.ranking.topN: [10,20]", "embedding.size: 64", "max.epoch: 1", "batch.size: 32",
        "learning.rate: 0.001", "reg.lambda: 0.0001", "max.len: 50", "BERT4Rec:", "  n_blocks: 2", "  drop_rate: 0.2",
        "  n_heads: 1", "  mask_rate: 0.5", "output: ./results/"]) + "\n")
    made = []
    init = mod.BERT4Rec.__init__

    def recording_init(self, *a, **k):
        made.append(self)
        init(self, *a, **k)
    monkeypatch.setattr(mod.BERT4Rec, "__init__", recording_init)
    torch.manual_seed(0); random.seed(0)
    SELFRec(ModelConf(str(path))).execute()
    model = made[0]
    out = capsys.readouterr().out
    assert "training: 1 batch 0 batch_loss:" in out and "Hit Ratio" in out and "NDCG" in out
    losses = model.epoch_losses
    assert len(losses) == 1 and len(losses[0]) == 10 and np.isfinite(np.asarray(losses)).all()
    assert model.bestPerformance and model.bestPerformance[0] == 1 and "NDCG" in model.bestPerformance[1]
    assert model.model.uses_kernel(50) and model.uses_ce_kernel() and model.model.rng_counter > 0
