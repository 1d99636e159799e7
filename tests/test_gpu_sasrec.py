"""SASRec on the device: the fused causal attention and the BCE kernel against the float64 restatement
(tests/sasrec_ref.py, pinned to the reference by tests/test_sasrec_cpu.py), the in-kernel dropout mask against the host
restatement of the counter RNG, repeatability, the model against the reference-run golden, and an end-to-end run.

Bounds: outputs <= 1e-5, gradients <= 1e-4, each of its tensor's largest magnitude."""
import functools
import json
import os
import random

import numpy as np
import pytest
import torch

from tests import sasrec_ref, seq_attn_ref
from tests.test_shapes_cpu import GOLDEN

pytestmark = pytest.mark.gpu

ATTN_SHAPES = [(1, 1, 1, 64), (3, 7, 1, 64), (5, 50, 1, 64), (4, 64, 2, 32), (2, 33, 2, 64), (256, 50, 1, 64),
               # either side of the 16-row tile edges, and the head layouts where the head offset and the row stride differ
               (2, 16, 1, 64), (2, 17, 2, 32), (2, 32, 4, 32), (2, 48, 1, 32), (2, 49, 3, 32)]
DROP_P = 0.2


def rel_err(got, want):
    """largest error as a fraction of the tensor's largest magnitude"""
    want = want.double().cpu()
    return float((got.double().cpu() - want).abs().max() / want.abs().max().clamp_min(1e-300))


@functools.lru_cache(maxsize=None)
def attn_case(shape, masked):
    """inputs (float32, host), the keep mask and the float64 output and gradients, computed once per case"""
    B, L, H, dh = shape
    g = torch.Generator().manual_seed(1000 * B + 10 * L + H + (5 if masked else 0))
    q = 8.0 * torch.randn(B, L, H * dh, generator=g)          # logits of several units: some rows near one-hot
    k, v, go = (torch.randn(B, L, H * dh, generator=g) for _ in range(3))
    keep = (torch.rand(B, H, L, L, generator=g) >= DROP_P) if masked else None
    q64, k64, v64 = (t.double().requires_grad_(True) for t in (q, k, v))
    out = sasrec_ref.attention(q64, k64, v64, H, None if keep is None else keep.numpy(), DROP_P)
    out.backward(go.double())
    p = torch.softmax((q64.detach()[..., :dh] @ k64.detach()[..., :dh].transpose(1, 2) / dh ** 0.5)
                      .masked_fill(~torch.ones(L, L, dtype=torch.bool).tril(), float('-inf')), -1)
    return dict(q=q, k=k, v=v, go=go, keep=keep, out=out.detach(), gq=q64.grad, gk=k64.grad, gv=v64.grad,
                lse=seq_attn_ref.lse(q, k, H, True), peak=float(p[:, L // 2:].max(-1).values.max()))       # (row 0 is one-hot by construction: later rows only)


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "keep"])
@pytest.mark.parametrize("shape", ATTN_SHAPES, ids=lambda s: "B%d_L%d_H%d_dh%d" % s)
def test_attention_forward_and_backward_match_float64(shape, masked):
    from selfrec_amd import ops
    B, L, H, dh = shape
    c = attn_case(shape, masked)
    if L >= 7:
        assert c["peak"] > 0.99                                   # a near-one-hot softmax row is among the inputs
    dev = torch.device("cuda:0")
    q, k, v, go = (c[n].to(dev) for n in ("q", "k", "v", "go"))
    keep = None if c["keep"] is None else c["keep"].to(dev)
    kw = dict(keep=keep, drop_p=DROP_P if masked else 0.0)
    out, lse = ops.seq_attn_fwd(q, k, v, H, **kw)
    gq, gk, gv = ops.seq_attn_bwd(q, k, v, lse, go, H, **kw)
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
    oa = ops.SeqAttnFn.apply(qa, ka, va, H, keep, kw["drop_p"], 0, 0)
    oa.backward(go)
    assert torch.equal(oa.detach(), out) and torch.equal(qa.grad, gq) and torch.equal(ka.grad, gk) and torch.equal(va.grad, gv)


def test_attention_refuses_shapes_outside_the_envelope():
    from selfrec_amd import ops
    dev = torch.device("cuda:0")
    for B, L, H, dh in ((2, 65, 1, 64), (2, 16, 1, 48), (2, 16, 4, 64)):
        q = torch.zeros(B, L, H * dh, device=dev)
        with pytest.raises(ops.SelfrecHipError, match=r"\(-3\)"):     # SRH_ERR_UNSUPPORTED, with its message
            ops.seq_attn_fwd(q, q, q, H)


@pytest.mark.parametrize("shape", [(3, 40, 2, 64), (2, 32, 3, 32)], ids=lambda s: "B%d_L%d_H%d_dh%d" % s)
def test_in_kernel_dropout_mask_is_the_counter_rng(shape):
    """V = I and Q = 0 make row i of the output P~[i, :]: uniform 1 / (i + 1) over j <= i times the dropout multiplier --
    the keep mask read back equals the host restatement bit for bit, and the next call's counters are disjoint"""
    from selfrec_amd import ops
    B, L, H, dh = shape
    dev = torch.device("cuda:0")
    seed, ctr = 0x5DEECE66D1234, (1 << 33) + 12345
    q = torch.zeros(B, L, H * dh, device=dev)
    v = torch.zeros(B, L, H, dh, device=dev)
    v[:, torch.arange(L), :, torch.arange(L)] = 1.0
    v = v.reshape(B, L, H * dh)
    tril = np.tril(np.ones((L, L), dtype=bool))
    masks, outs = [], []
    for call in range(2):
        c0 = ctr + call * B * H * L                                # the advance per call the header states
        out, _ = ops.seq_attn_fwd(q, q, v, H, drop_p=DROP_P, rng_seed=seed, rng_counter=c0)
        pt = out.reshape(B, L, H, dh)[..., :L].permute(0, 2, 1, 3).cpu().numpy()       # (B, H, i, j)
        want = sasrec_ref.attn_keep_drawn(seed, c0, B, H, L, DROP_P)
        assert np.array_equal((pt > 0)[..., tril], want[..., tril])
        scale = (1.0 / (1.0 - DROP_P)) / np.arange(1, L + 1)[:, None]
        assert np.allclose(pt[..., tril], (want * scale)[..., tril], rtol=1e-6)
        assert not pt[..., ~tril].any()
        masks.append(want)
        outs.append(out)
    # the counters of consecutive calls are disjoint and adjacent: ONE call over the 2B sequences draws, bit for bit, what
    # the two calls drew
    q2, v2 = torch.cat([q, q]), torch.cat([v, v])
    both, _ = ops.seq_attn_fwd(q2, q2, v2, H, drop_p=DROP_P, rng_seed=seed, rng_counter=ctr)
    assert torch.equal(both, torch.cat(outs))
    assert abs(1.0 - masks[0][..., tril].mean() - DROP_P) < 0.03


def test_model_advances_the_dropout_counter_per_attention_call():
    from types import SimpleNamespace
    from selfrec_amd.model.sequential.SASRec import SASRec_Model
    torch.manual_seed(3)
    net = SASRec_Model(SimpleNamespace(item_num=30), 64, 10, 2, 2, 0.2).cuda()
    rs = np.random.RandomState(0)
    seq = rs.randint(1, 31, size=(4, 10))
    pos = np.tile(np.arange(1, 11), (4, 1))
    net.train()
    net(seq, pos)
    assert net.rng_counter == 2 * (4 * 2 * 10)                   # two blocks, B H L counters each
    net.eval()
    net(seq, pos)
    assert net.rng_counter == 2 * (4 * 2 * 10)                   # no dropout, no draws


BCE_CASES = [(1, "all"), (50, "third"), (50, "single"), (12800, "third")]


@functools.lru_cache(maxsize=None)
def bce_case(R, which):
    g = torch.Generator().manual_seed(R + len(which))
    n_items, d = 40, 64
    table = torch.randn(n_items, d, generator=g)
    hidden = 3.0 * torch.randn(R, d, generator=g)                  # logits of std 24: both tails of the loss
    pos = torch.randint(0, n_items, (R,), generator=g)
    neg = torch.randint(0, n_items, (R,), generator=g)
    valid = torch.ones(R, dtype=torch.bool)
    if which == "third":
        valid[torch.arange(R) % 3 == 1] = False
    elif which == "single":
        valid[:] = False
        valid[17] = True
    h64, t64 = hidden.double().requires_grad_(True), table.double().requires_grad_(True)
    lp, ln = sasrec_ref.bce_means(h64, t64, pos.numpy(), neg.numpy(), valid.numpy())
    (lp + ln).backward()
    logits = (hidden.double() * table.double()[pos]).sum(-1)[valid]
    return dict(table=table, hidden=hidden, pos=pos, neg=neg, valid=valid, lp=float(lp.detach()), ln=float(ln.detach()), gh=h64.grad,
                gt=t64.grad, span=float(logits.abs().max()))


@pytest.mark.parametrize("R,which", BCE_CASES)
def test_bce_kernel_matches_float64(R, which):
    from selfrec_amd import ops
    c = bce_case(R, which)
    if R > 1:
        assert c["span"] > (30.0 if which != "single" else 0.0)
    dev = torch.device("cuda:0")
    hidden, table = c["hidden"].to(dev), c["table"].to(dev)
    pos, neg = c["pos"].to(dev, torch.int32), c["neg"].to(dev, torch.int32)
    valid = c["valid"].to(dev, torch.uint8)
    loss2, gh, grows = ops.seq_bce_fwd_bwd(hidden, table, pos, neg, valid)
    plan = ops.scatter_plan(np.concatenate([c["pos"].numpy(), c["neg"].numpy()]), dev)
    gt = ops.rows_segment_sum(grows, plan, torch.zeros_like(table))
    got = loss2.cpu().numpy()
    errs = dict(lp=abs(got[0] - c["lp"]) / abs(c["lp"]), ln=abs(got[1] - c["ln"]) / abs(c["ln"]),
                gh=rel_err(gh, c["gh"]), gt=rel_err(gt, c["gt"]))
    print(R, which, errs)
    assert errs["lp"] <= 1e-5 and errs["ln"] <= 1e-5, errs
    assert errs["gh"] <= 1e-4 and errs["gt"] <= 1e-4, errs
    assert not gh[~c["valid"].to(dev)].any()                        # an invalid row takes no gradient
    # the autograd wrapper: the same loss (float32 sum of the two means) and gradients
    ha, ta = hidden.clone().requires_grad_(True), table.clone().requires_grad_(True)
    loss = ops.SeqBceFn.apply(ha, ta, pos, neg, valid, int(c["valid"].sum()), plan)
    loss.backward()
    assert abs(float(loss) - (c["lp"] + c["ln"])) <= 1e-5 * (c["lp"] + c["ln"])
    assert torch.equal(ha.grad, gh) and torch.equal(ta.grad, gt)


def test_kernels_return_the_same_bits_twice():
    from selfrec_amd import ops
    dev = torch.device("cuda:0")
    c = attn_case((5, 50, 1, 64), True)
    q, k, v, go, keep = (c[n].to(dev) for n in ("q", "k", "v", "go", "keep"))
    runs = []
    for _ in range(2):
        out, lse = ops.seq_attn_fwd(q, k, v, 1, keep=keep, drop_p=DROP_P)
        runs.append((out, lse) + ops.seq_attn_bwd(q, k, v, lse, go, 1, keep=keep, drop_p=DROP_P))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    b = bce_case(12800, "third")
    args = (b["hidden"].to(dev), b["table"].to(dev), b["pos"].to(dev, torch.int32), b["neg"].to(dev, torch.int32),
            b["valid"].to(dev, torch.uint8))
    first, second = ops.seq_bce_fwd_bwd(*args), ops.seq_bce_fwd_bwd(*args)
    assert all(torch.equal(x, y) for x, y in zip(first, second))


# ---- the model ----------------------------------------------------------------------------------------------------------
def golden():
    return np.load(os.path.join(GOLDEN, "sasrec.npz")), json.load(open(os.path.join(GOLDEN, "sasrec_meta.json")))


def make_model(meta, heads, tmp_path, monkeypatch, train=None, test=None, **over):
    from selfrec_amd.model.sequential.SASRec import SASRec
    from selfrec_amd.util.conf import ModelConf
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("SRH_SASREC_ATTN", raising=False)
    c = meta["conf"]
    conf = {"model": {"name": "SASRec", "type": "sequential"}, "item.ranking.topN": c["topN"], "embedding.size": c["emb"],
            "max.epoch": over.get("max_epoch", 1), "batch.size": over.get("batch", c["batch"]), "learning.rate": c["lr"],
            "reg.lambda": c["reg"], "output": "./results/", "training.set": "x", "test.set": "y", "max.len": c["max_len"],
            "SASRec": {"n_blocks": c["n_blocks"], "drop_rate": over.get("drop_rate", c["drop_rate"]), "n_heads": heads}}
    if "attention" in over:
        conf["engine.attention"] = over["attention"]
    train = meta["train"] if train is None else train
    test = meta["test"] if test is None else test
    return SASRec(ModelConf(conf), {k: list(v) for k, v in train.items()}, {k: list(v) for k, v in test.items()})


def train_step(model, optimizer, batch):
    from selfrec_amd.util.loss_torch import l2_reg_loss
    seq, pos, y, neg, _ = batch
    net = model.model
    net.train()
    seq_emb = net.forward(seq, pos)
    batch_loss = model.calculate_loss(seq_emb, y, neg, pos) + l2_reg_loss(model.reg, net.item_emb)
    optimizer.zero_grad()
    batch_loss.backward()
    return batch_loss


@pytest.mark.parametrize("heads", [1, 2])
def test_model_matches_the_reference_golden(heads, tmp_path, monkeypatch, capsys):
    from selfrec_amd.util.evaluation import ranking_evaluation
    from selfrec_amd.util.sampler import next_batch_sequence
    gd, meta = golden()
    torch.cuda.set_device(0)
    torch.manual_seed(meta["torch_seed"]); random.seed(meta["sampler_seed"])
    model = make_model(meta, heads, tmp_path, monkeypatch)
    net = model.model.cuda()
    params = dict(net.named_parameters())
    assert net.uses_kernel(meta["conf"]["max_len"])
    for name, p in params.items():
        assert np.array_equal(p.detach().cpu().numpy(), gd[f"init_{name}"]), name
    batches = list(next_batch_sequence(model.data, model.batch_size, max_len=model.max_len))
    for b, batch in enumerate(batches):
        for key, got in zip(("seq", "pos", "y", "neg", "len"), batch):
            assert np.array_equal(np.asarray(got), gd[f"train{b}_{key}"]), (b, key)
    optimizer = torch.optim.Adam(net.parameters(), lr=model.lRate)
    lr = model.lRate
    for s in range(3):
        loss = train_step(model, optimizer, batches[s])
        want = gd[f"h{heads}_loss"][s]
        print("step", s, float(loss), want)
        assert abs(float(loss) - want) <= 1e-5 * abs(want), (s, float(loss), want)
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
    # test() on the golden's final parameters: its lists and its evaluation strings
    with torch.no_grad():
        for name, p in params.items():
            p.copy_(torch.from_numpy(gd[f"h{heads}_final_{name}"]))
    net.eval()
    rec = model.test()
    d = model.data
    names = [n for n, _ in d.original_seq]
    want_ids, want_sc = gd[f"h{heads}_rec_ids"], gd[f"h{heads}_rec_scores"]
    scale = np.abs(want_sc).max()
    for r, n in enumerate(names):
        keep = want_ids[r] >= 0
        assert [d.item[it] for it, _ in rec[n]] == want_ids[r][keep].tolist(), n
        assert np.abs(np.asarray([sc for _, sc in rec[n]]) - want_sc[r][keep]).max() <= 1e-5 * scale, n
    assert any((want_ids[r] < 0).any() for r in range(len(names)))     # row 0 did leave some list
    ev = meta[f"h{heads}_evaluation"]
    assert ranking_evaluation(d.test_set, rec, model.topN) == ev["topN"]
    assert ranking_evaluation(d.test_set, rec, [model.max_N]) == ev["maxN"]
    measure = model.fast_evaluation(0)
    assert measure == ev["maxN"] and model.bestPerformance[0] == 1
    out = capsys.readouterr().out
    assert "*Best Performance*\nEpoch: 1, " + ", ".join(f"{k}: {v}" for k, v in model.bestPerformance[1].items()) in out


def test_two_models_with_the_same_seeds_end_with_the_same_parameters(tmp_path, monkeypatch):
    """4 steps with dropout 0.2, twice, under torch.use_deterministic_algorithms(True) for torch's share (LayerNorm,
    Linear, Adam): identical parameters"""
    from selfrec_amd.util.sampler import next_batch_sequence
    _, meta = golden()
    torch.cuda.set_device(0)
    was = torch.are_deterministic_algorithms_enabled()
    monkeypatch.setenv("CUBLAS_WORKSPACE_CONFIG", ":4096:8")
    torch.use_deterministic_algorithms(True)
    try:
        ends = []
        for _ in range(2):
            torch.manual_seed(7); random.seed(8)
            model = make_model(meta, 2, tmp_path, monkeypatch, drop_rate=0.2)
            net = model.model.cuda()
            optimizer = torch.optim.Adam(net.parameters(), lr=model.lRate)
            losses = []
            for s, batch in enumerate(next_batch_sequence(model.data, model.batch_size, max_len=model.max_len)):
                losses.append(float(train_step(model, optimizer, batch)))
                optimizer.step()
            assert len(losses) == 4
            ends.append((losses, {n: p.detach().clone() for n, p in net.named_parameters()}))
    finally:
        torch.use_deterministic_algorithms(was)
    assert ends[0][0] == ends[1][0]
    for name in ends[0][1]:
        assert torch.equal(ends[0][1][name], ends[1][1][name]), name


def tiny_conf(tmp_path, epochs, drop, attention=None):
    from selfrec_amd import synth
    train, test = synth.make_sequence_dataset("tiny-seq")
    synth.write_sequences(str(tmp_path / "train.txt"), train)
    synth.write_sequences(str(tmp_path / "test.txt"), test)
    lines = [f"training.set: {tmp_path / 'train.txt'}", f"test.set: {tmp_path / 'test.txt'}", "model:", "  name: SASRec",
             "  type: sequential", "item.ranking.topN: [10,20]", "embedding.size: 64", f"max.epoch: {epochs}",
             "batch.size: 32", "learning.rate: 0.001", "reg.lambda: 0.0001", "max.len: 50", "SASRec:", "  n_blocks: 2",
             f"  drop_rate: {drop}", "  n_heads: 1", "output: ./results/"]
    if attention:
        lines.append(f"engine.attention: {attention}")
    path = tmp_path / f"SASRec_{attention or 'hip'}_{epochs}.yaml"
    path.write_text("\n".join(lines) + "\n")
    return str(path)


def run_selfrec(conf_path, monkeypatch):
    """SELFRec(conf).execute(), returning the model instance it built"""
    from selfrec_amd.SELFRec import SELFRec
    from selfrec_amd.model.sequential import SASRec as mod
    from selfrec_amd.util.conf import ModelConf
    made = []
    init = mod.SASRec.__init__

    def recording_init(self, *a, **k):
        made.append(self)
        init(self, *a, **k)
    monkeypatch.setattr(mod.SASRec, "__init__", recording_init)
    SELFRec(ModelConf(conf_path)).execute()
    monkeypatch.setattr(mod.SASRec, "__init__", init)
    return made[0]


def test_sasrec_end_to_end(tmp_path, monkeypatch, capsys):
    torch.cuda.set_device(0)
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("SRH_SASREC_ATTN", raising=False)
    torch.manual_seed(0); random.seed(0)
    model = run_selfrec(tiny_conf(tmp_path, 2, 0.2), monkeypatch)
    out = capsys.readouterr().out
    assert "training: 1 batch 0 rec_loss:" in out and "Training Set Size: (sequence number: 300" in out
    assert "Hit Ratio" in out and "NDCG" in out
    losses = model.epoch_losses
    assert len(losses) == 2 and len(losses[0]) == 10 and np.isfinite(np.asarray(losses)).all()
    print("epoch means", np.mean(losses[0]), np.mean(losses[1]))
    assert np.mean(losses[1]) < np.mean(losses[0])
    assert model.bestPerformance and model.bestPerformance[0] in (1, 2) and "NDCG" in model.bestPerformance[1]
    assert model.model.uses_kernel(50) and model.model.rng_counter > 0
    # the torch route on the same inputs, without dropout: the same losses
    runs = {}
    for route in ("hip", "torch"):
        torch.manual_seed(1); random.seed(1)
        m = run_selfrec(tiny_conf(tmp_path, 1, 0.0, route), monkeypatch)
        assert m.model.attention == route and m.model.uses_kernel(50) == (route == "hip")
        runs[route] = np.asarray(m.epoch_losses[0])
    err = np.abs(runs["hip"] - runs["torch"]).max()
    print("hip vs torch losses", err)
    assert err <= 1e-4 * np.abs(runs["torch"]).max()
