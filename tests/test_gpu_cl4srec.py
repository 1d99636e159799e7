"""CL4SRec on the device: the embedding-front kernel and the live-row segment sum against the float64 restatement
(tests/cl4srec_ref.py, pinned to the reference by tests/test_cl4srec_cpu.py) on the cases of tests/cl4srec_cases.py, the
drawn dropout mask against the host restatement of the counter RNG, repeatability, the autograd functions against their
torch-route partners, InfoNceFn, the model against the reference-run golden on all four routes, and an end-to-end run.

Bounds: outputs <= 1e-5, gradients <= 1e-4, each of its tensor's largest magnitude."""
import json
import os
import random

import numpy as np
import pytest
import torch

from tests import cl4srec_cases as cases
from tests import cl4srec_ref
from tests.test_cl4srec_cpu import check_initial_parameters, golden_step, make_model, seeded
from tests.test_shapes_cpu import GOLDEN

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED, CTR = 0x5DEECE66D1234, (1 << 33) + 777


def dev_ids(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32).reshape(-1)).to(DEV) for a in arrays)


# ---- embed forward ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", cases.EMBED_SHAPES, ids=cases.shape_id)
def test_embed_forward(shape):
    from selfrec_amd import ops
    c = cases.embed_case(shape)
    B, L, d = shape
    item, pos_table = c["item"].to(DEV), c["pos_table"].to(DEV)
    seq, pos = dev_ids(c["seq"], c["pos"])
    dead = torch.from_numpy(~c["live"]).to(DEV)
    # p = 0: the bits of torch's expression on the device (d = 32: a scale that is no power of two catches an fma)
    out = ops.seq_embed_fwd(item, pos_table, seq, pos)
    assert torch.equal(out, cases.torch_embed_front(item, pos_table, c["seq"], c["pos"]))
    assert not out[dead].any() and out.shape == (B * L, d)
    err = cases.rel_err(out, c["out"])
    # an injected keep mask at p = 0.2, against float64
    kept = ops.seq_embed_fwd(item, pos_table, seq, pos, keep=c["keep"].to(DEV), drop_p=cases.DROP_P)
    err_keep = cases.rel_err(kept, c["out_keep"])
    print(shape, err, err_keep)
    assert err <= cases.OUT_BOUND and err_keep <= cases.OUT_BOUND
    assert not kept[dead].any()
    # a drawn mask: the zero pattern is the counter RNG's, bit for bit, and the kept elements are out / (1 - p)
    drawn = ops.seq_embed_fwd(item, pos_table, seq, pos, drop_p=cases.DROP_P, rng_seed=SEED, rng_counter=CTR)
    want_keep = cl4srec_ref.embed_keep_drawn(SEED, CTR, B * L, d, cases.DROP_P)
    live = c["live"]
    assert (c["out"][torch.from_numpy(live)] != 0).all()
    assert np.array_equal((drawn != 0).cpu().numpy()[live], want_keep[live])
    assert not drawn[dead].any()
    want = cl4srec_ref.embed_front(c["item"].double(), c["pos_table"].double(), c["seq"], c["pos"], want_keep, cases.DROP_P)
    assert cases.rel_err(drawn, want) <= cases.OUT_BOUND
    if B * L >= 350:
        assert abs(1.0 - want_keep[live].mean() - cases.DROP_P) < 0.03


def test_embed_forward_refuses_other_widths_and_zeroes_foreign_ids():
    from selfrec_amd import ops
    ids = torch.tensor([1, 2], dtype=torch.int32, device=DEV)
    with pytest.raises(ops.SelfrecHipError, match=r"\(-3\)"):          # SRH_ERR_UNSUPPORTED, with its message
        ops.seq_embed_fwd(torch.zeros(4, 48, device=DEV), torch.zeros(4, 48, device=DEV), ids, ids)
    item, pos_table = torch.ones(4, 64, device=DEV), torch.ones(3, 64, device=DEV)
    seq = torch.tensor([1, 4, -1, 2, 3], dtype=torch.int32, device=DEV)
    pos = torch.tensor([1, 1, 1, 3, 2], dtype=torch.int32, device=DEV)
    out = ops.seq_embed_fwd(item, pos_table, seq, pos)
    assert out[0].eq(9.0).all() and out[4].eq(9.0).all() and not out[1:4].any()      # an id outside its table: a zero row


# ---- live sum -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dropout", ["none", "keep", "drawn"])
@pytest.mark.parametrize("shape", cases.EMBED_SHAPES, ids=cases.shape_id)
def test_live_sum_item_and_position_problems_in_one_call(shape, dropout):
    """the embed backward's call: a scaled (item) and an unscaled (position) problem over an upstream gradient whose dead
    rows are NaN"""
    from selfrec_amd import ops
    c = cases.embed_case(shape)
    B, L, d = shape
    x = c["go_nan"].to(DEV)
    plans = [ops.live_plan(ids, DEV, c["live"]) for ids in (c["seq"], c["pos"])]
    if dropout == "none":
        drop, want = {}, (c["gi"], c["gp"])
    elif dropout == "keep":
        drop, want = dict(keep=c["keep"].to(DEV), drop_p=cases.DROP_P), (c["gi_keep"], c["gp_keep"])
    else:
        drop = dict(drop_p=cases.DROP_P, rng_seed=SEED, rng_counter=CTR)
        mult = cl4srec_ref.embed_keep_drawn(SEED, CTR, B * L, d, cases.DROP_P) / (1.0 - cases.DROP_P)
        want = (cl4srec_ref.live_sum(c["go"].numpy(), c["seq"], c["live"], cases.N_ITEMS + 2, d ** 0.5, mult),
                cl4srec_ref.live_sum(c["go"].numpy(), c["pos"], c["live"], L + 1, 1.0, mult))
    runs = []
    for _ in range(2):
        gi = torch.zeros(cases.N_ITEMS + 2, d, device=DEV)
        gp = torch.zeros(L + 1, d, device=DEV)
        ops.rows_live_sum([dict(x=x, plan=plans[0], out=gi, scale=d ** 0.5, **drop), dict(x=x, plan=plans[1], out=gp, **drop)])
        runs.append((gi, gp))
    gi, gp = runs[0]
    assert torch.isfinite(gi).all() and torch.isfinite(gp).all()
    errs = (cases.rel_err(gi, want[0]), cases.rel_err(gp, want[1]))
    print(shape, dropout, errs)
    assert max(errs) <= cases.GRAD_BOUND
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])       # the same bits twice
    assert not gi[0].any()                                              # the padding id names no live row


@pytest.mark.parametrize("d", [32, 64, 128])
def test_live_sum_segment_lengths_around_the_chunk(d):
    from selfrec_amd import ops
    c = cases.segment_case(d)
    plan = ops.live_plan(c["ids"], DEV, c["live"])
    x = c["x_nan"].to(DEV)
    out = torch.full((c["n_table"], d), 5.0, device=DEV)
    ops.rows_live_sum([dict(x=x, plan=plan, out=out)])
    named = np.unique(c["ids"][c["live"]])
    rest = np.setdiff1d(np.arange(c["n_table"]), named)
    assert torch.isfinite(out).all() and out[torch.from_numpy(rest).to(DEV)].eq(5.0).all()    # unnamed rows left alone
    err = cases.rel_err(out[torch.from_numpy(named).to(DEV)], c["want"][named])
    print(d, err)
    assert err <= cases.GRAD_BOUND
    again = torch.full((c["n_table"], d), 5.0, device=DEV)
    ops.rows_live_sum([dict(x=x, plan=plan, out=again)])
    assert torch.equal(out, again)
    # three problems in one call, the middle one without a live row: it writes nothing
    none = ops.live_plan(np.zeros(7, dtype=np.int64), DEV)
    outs = [torch.full((c["n_table"], d), 5.0, device=DEV) for _ in range(3)]
    ops.rows_live_sum([dict(x=x, plan=plan, out=outs[0]), dict(x=x[:7], plan=none, out=outs[1]),
                       dict(x=x, plan=plan, out=outs[2], scale=2.0)])
    assert torch.equal(outs[0], out) and outs[1].eq(5.0).all()
    assert cases.rel_err(outs[2][torch.from_numpy(named).to(DEV)], 2.0 * c["want"][named]) <= cases.GRAD_BOUND
    # a call whose only problem has no live row returns OK and writes nothing
    lone = torch.full((4, d), 5.0, device=DEV)
    ops.rows_live_sum([dict(x=x[:7], plan=none, out=lone)])
    assert lone.eq(5.0).all()


# ---- the autograd functions against their torch-route partners ---------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 7, 32), (5, 50, 64)], ids=cases.shape_id)
def test_seq_embed_fn_against_the_gather_route(shape):
    from selfrec_amd import ops
    c = cases.embed_case(shape)
    B, L, d = shape
    seq, pos = dev_ids(c["seq"], c["pos"])
    go = c["go"].to(DEV)
    live_t = torch.from_numpy(c["live"]).to(DEV).unsqueeze(-1)
    weight = torch.randn(B * L, d, generator=torch.Generator().manual_seed(1)).to(DEV)
    for keep, tag in ((None, ""), (c["keep"].to(DEV), "_keep")):
        p = 0.0 if keep is None else cases.DROP_P
        ia, pa = c["item"].to(DEV).requires_grad_(True), c["pos_table"].to(DEV).requires_grad_(True)
        out = ops.SeqEmbedFn.apply(ia, pa, seq, pos, ops.live_plan(c["seq"], DEV, c["live"]),
                                   ops.live_plan(c["pos"], DEV, c["live"]), keep, p, 0, 0)
        loss = (out * weight).sum()
        loss.backward()
        ib, pb = c["item"].to(DEV).requires_grad_(True), c["pos_table"].to(DEV).requires_grad_(True)
        x = (ops.GatherRowsFn.apply(ib, seq, ops.scatter_plan(c["seq"], DEV)) * d ** 0.5
             + ops.GatherRowsFn.apply(pb, pos, ops.scatter_plan(c["pos"], DEV)))
        if keep is not None:
            x = x * (keep.to(x.dtype) / (1.0 - p))
        partner = ((x * live_t) * weight).sum()
        partner.backward()
        if keep is None:
            assert torch.equal(loss.detach(), partner.detach())         # the same loss bits at p = 0
        # both against the float64 gradients of sum(out * weight): live_sum of weight's rows
        mult = None if keep is None else c["keep"].numpy() / (1.0 - p)
        want_i = cl4srec_ref.live_sum(weight.cpu().numpy(), c["seq"], c["live"], cases.N_ITEMS + 2, d ** 0.5, mult)
        want_p = cl4srec_ref.live_sum(weight.cpu().numpy(), c["pos"], c["live"], L + 1, 1.0, mult)
        errs = [cases.rel_err(g, w) for g, w in ((ia.grad, want_i), (pa.grad, want_p), (ib.grad, want_i), (pb.grad, want_p))]
        print(shape, tag, errs)
        assert max(errs) <= cases.GRAD_BOUND


@pytest.mark.parametrize("R,which", [(1, "all"), (50, "third"), (50, "single"), (12800, "third")])
def test_seq_bce_live_fn_against_seq_bce_fn(R, which):
    from selfrec_amd import ops
    from tests.test_gpu_sasrec import bce_case
    c = bce_case(R, which)
    hidden, table = c["hidden"].to(DEV), c["table"].to(DEV)
    pos, neg = c["pos"].to(DEV, torch.int32), c["neg"].to(DEV, torch.int32)
    valid = c["valid"].to(DEV, torch.uint8)
    yn = np.concatenate([c["pos"].numpy(), c["neg"].numpy()])
    v2 = np.concatenate([c["valid"].numpy(), c["valid"].numpy()])
    n_valid = int(c["valid"].sum())
    got = {}
    for name, fn, plan in (("live", ops.SeqBceLiveFn, ops.live_plan(yn, DEV, v2)), ("all", ops.SeqBceFn, ops.scatter_plan(yn, DEV))):
        h, t = hidden.clone().requires_grad_(True), table.clone().requires_grad_(True)
        loss = fn.apply(h, t, pos, neg, valid, n_valid, plan)
        (3.0 * loss).backward()
        got[name] = (loss.detach(), h.grad, t.grad)
    assert torch.equal(got["live"][0], got["all"][0]) and torch.equal(got["live"][1], got["all"][1])
    errs = (cases.rel_err(got["live"][2], 3.0 * c["gt"]), cases.rel_err(got["all"][2], 3.0 * c["gt"]))
    print(R, which, errs)
    assert max(errs) <= cases.GRAD_BOUND


@pytest.mark.parametrize("n", cases.NCE_SIZES)
def test_infonce_fn_matches_float64(n):
    from selfrec_amd import ops
    c = cases.nce_case(n)
    v1, v2 = c["v1"].to(DEV).requires_grad_(True), c["v2"].to(DEV).requires_grad_(True)
    loss = ops.InfoNceFn.apply(v1, v2, 1.0)
    loss.backward()
    print(n, float(loss.detach()), c["loss"])
    if n == 1:
        # one row: the softmax of one logit is 1, loss and gradients 0; the absolute size of n = 2's tolerance
        assert abs(float(loss)) <= 1e-6 and v1.grad.abs().max() <= 1e-6 and v2.grad.abs().max() <= 1e-6
    else:
        assert abs(float(loss) - c["loss"]) <= cases.OUT_BOUND * abs(c["loss"])
        assert max(cases.rel_err(v1.grad, c["g1"]), cases.rel_err(v2.grad, c["g2"])) <= cases.GRAD_BOUND
    with pytest.raises(ops.SelfrecHipError):
        ops.InfoNceFn.apply(torch.zeros(4, 48, device=DEV), torch.zeros(4, 48, device=DEV), 1.0)


# ---- the model ----------------------------------------------------------------------------------------------------------
def golden():
    return np.load(os.path.join(GOLDEN, "cl4srec.npz")), json.load(open(os.path.join(GOLDEN, "cl4srec_meta.json")))


@pytest.mark.parametrize("embed", ["hip", "torch"])
@pytest.mark.parametrize("views", ["one", "three"])
@pytest.mark.parametrize("aug_type", [0, 1, 2])
def test_model_matches_the_reference_golden(aug_type, views, embed, tmp_path, monkeypatch, capsys):
    from selfrec_amd.util.evaluation import ranking_evaluation
    gd, meta = golden()
    k = f"t{aug_type}h1"
    torch.cuda.set_device(0)
    seeded(meta)
    model = make_model(meta, aug_type, 1, tmp_path, monkeypatch, views=views, embed=embed)
    assert (model.views, model.embed) == (views, embed)
    net = model.model.cuda()
    params = dict(net.named_parameters())
    assert net.uses_kernel(meta["conf"]["max_len"])
    check_initial_parameters(gd, params)
    optimizer = torch.optim.Adam(net.parameters(), lr=model.lRate)
    lr = model.lRate
    net.train()
    for s in range(3):
        (seq, pos, y, neg, _), aug = golden_step(gd, aug_type, s)
        loss, rec, cl = model.step_losses(seq, pos, y, neg, aug)
        for got, key in ((loss, "loss"), (rec, "rec_loss"), (cl, "cl_loss")):
            want = gd[f"{k}_{key}"][s]
            print("step", s, key, float(got.detach()), want)
            assert abs(float(got.detach()) - want) <= 1e-5 * abs(want), (s, key, float(got.detach()), want)
        optimizer.zero_grad()
        loss.backward()
        if s == 0:
            for name, p in params.items():
                g = p.grad.reshape(-1).cpu().numpy().astype(np.float64)
                want_g = gd[f"{k}_grad0_{name}_val"].astype(np.float64)
                err = np.abs(g[gd[f"sample_{name}"]] - want_g).max()
                assert err <= 1e-4 * np.abs(want_g).max() + 1e-12, (name, err)
        optimizer.step()
        if s != 1:
            # Adam's first steps move every element by about lr whatever its gradient: within lr / 2
            for name, p in params.items():
                v = p.detach().reshape(-1).cpu().numpy()
                assert np.abs(v[gd[f"sample_{name}"]] - gd[f"{k}_step{s}_{name}_val"]).max() <= lr / 2, (s, name)
    if f"{k}_final_{meta['param_names'][0]}" not in gd.files:
        return
    # test() on the golden's final parameters: its lists and its evaluation strings
    with torch.no_grad():
        for name, p in params.items():
            p.copy_(torch.from_numpy(gd[f"{k}_final_{name}"]))
    net.eval()
    rec_list = model.test()
    d = model.data
    want_ids, want_sc = gd[f"{k}_rec_ids"], gd[f"{k}_rec_scores"]
    scale = np.abs(want_sc).max()
    for r, (name, _) in enumerate(d.original_seq):
        keep = want_ids[r] >= 0
        assert [d.item[it] for it, _ in rec_list[name]] == want_ids[r][keep].tolist(), name
        assert np.abs(np.asarray([sc for _, sc in rec_list[name]]) - want_sc[r][keep]).max() <= 1e-5 * scale, name
    ev = meta[f"{k}_evaluation"]
    assert ranking_evaluation(d.test_set, rec_list, model.topN) == ev["topN"]
    assert ranking_evaluation(d.test_set, rec_list, [model.max_N]) == ev["maxN"]
    assert model.fast_evaluation(0) == ev["maxN"] and model.bestPerformance[0] == 1


def test_model_advances_the_dropout_counter_by_rows_and_attention_calls(tmp_path, monkeypatch):
    gd, meta = golden()
    torch.cuda.set_device(0)
    seeded(meta)
    (seq, pos, y, neg, _), aug = golden_step(gd, 0, 0)
    B, L = seq.shape
    for views, passes in (("one", [3 * B]), ("three", [B, B, B])):
        model = make_model(meta, 0, 2, tmp_path, monkeypatch, views=views, drop_rate=0.2)
        net = model.model.cuda()
        net.train()
        loss, _, _ = model.step_losses(seq, pos, y, neg, aug)
        assert torch.isfinite(loss)
        # per encoder pass: rows counters for the embedding dropout, then rows * H * L per block's attention
        assert net.rng_counter == sum(rows * L + 2 * rows * 2 * L for rows in passes)


def tiny_conf(tmp_path, epochs, drop, **engine):
    from selfrec_amd import synth
    train, test = synth.make_sequence_dataset("tiny-seq")
    synth.write_sequences(str(tmp_path / "train.txt"), train)
    synth.write_sequences(str(tmp_path / "test.txt"), test)
    lines = [f"training.set: {tmp_path / 'train.txt'}", f"test.set: {tmp_path / 'test.txt'}", "model:", "  name: CL4SRec",
             "  type: sequential", "item.ranking.topN: [10,20]", "embedding.size: 64", f"max.epoch: {epochs}",
             "batch.size: 32", "learning.rate: 0.001", "reg.lambda: 0.0001", "max.len: 50", "CL4SRec:", "  n_blocks: 2",
             f"  drop_rate: {drop}", "  n_heads: 1", "  aug_type: 0", "  aug_rate: 0.5", "  cl_rate: 0.05",
             "output: ./results/"] + [f"engine.{k}: {v}" for k, v in engine.items()]
    path = tmp_path / ("CL4SRec_" + "_".join(engine.values()) + f"_{epochs}.yaml")
    path.write_text("\n".join(lines) + "\n")
    return str(path)


def test_cl4srec_end_to_end(tmp_path, monkeypatch, capsys):
    from selfrec_amd import main
    from selfrec_amd.model.sequential import CL4SRec as mod
    torch.cuda.set_device(0)
    monkeypatch.chdir(tmp_path)
    for env in ("SRH_SASREC_ATTN", "SRH_CL4SREC_VIEWS", "SRH_CL4SREC_EMBED"):
        monkeypatch.delenv(env, raising=False)
    made = []
    init = mod.CL4SRec.__init__

    def recording_init(self, *a, **kw):
        made.append(self)
        init(self, *a, **kw)
    monkeypatch.setattr(mod.CL4SRec, "__init__", recording_init)
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    main.main(["CL4SRec", "--conf", tiny_conf(tmp_path, 2, 0.2), "--synthetic", "tiny-seq"])
    out = capsys.readouterr().out
    assert "training: 1 batch 0 batch_loss:" in out and "Training Set Size: (sequence number: 300" in out
    assert "Hit Ratio" in out and "NDCG" in out
    model = made[0]
    losses = model.epoch_losses
    assert len(losses) == 2 and len(losses[0]) == 10 and np.isfinite(np.asarray(losses)).all()
    print("epoch means", np.mean(losses[0]), np.mean(losses[1]))
    assert (model.views, model.embed) == ("one", "hip") and model.model.uses_kernel(50) and model.model.rng_counter > 0
    assert model.bestPerformance and model.bestPerformance[0] in (1, 2) and "NDCG" in model.bestPerformance[1]
