"""GRU4Rec without a GPU: the registry, the conf and the route switch, the batch stager's host side, and the CPU model on
the golden (tests/golden/gru4rec.npz, make_golden_gru4rec.py: the reference's own data path, BCE expression and evaluation
around torch.nn.GRU) -- its sampler stream, three Adam steps, predict rows and test() lists, with 1 and 2 layers."""
import json
import os
import random

import numpy as np
import pytest
import torch

from tests.test_shapes_cpu import GOLDEN

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "gru4rec.npz")), json.load(open(os.path.join(GOLDEN, "gru4rec_meta.json")))


def make_model(meta, layers, tmp_path, monkeypatch, **over):
    from selfrec_amd.model.sequential.GRU4Rec import GRU4Rec
    from selfrec_amd.util.conf import ModelConf
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("SRH_GRU4REC_RNN", raising=False)
    c = meta["conf"]
    conf = {"model": {"name": "GRU4Rec", "type": "sequential"}, "item.ranking.topN": c["topN"], "embedding.size": c["emb"],
            "max.epoch": 1, "batch.size": c["batch"], "learning.rate": c["lr"], "reg.lambda": c["reg"], "output": "./results/",
            "training.set": "x", "test.set": "y", "max.len": c["max_len"],
            "GRU4Rec": {"n_layers": layers, "drop_rate": over.get("drop_rate", c["drop_rate"])}}
    if "rnn" in over:
        conf["engine.rnn"] = over["rnn"]
    return GRU4Rec(ModelConf(conf), {k: list(v) for k, v in meta["train"].items()},
                   {k: list(v) for k, v in meta["test"].items()})


def seeded_model(meta, layers, tmp_path, monkeypatch, **over):
    torch.manual_seed(meta["torch_seed"]); random.seed(meta["sampler_seed"])
    return make_model(meta, layers, tmp_path, monkeypatch, **over)


def replay_three_steps(gd, model, layers, device="cpu"):
    """the golden's three Adam steps as GRU4Rec.train() drives them: losses <= 1e-5, step 0's gradients <= 1e-4 of each
    tensor's max, parameters within lr / 2 -> the step-0 gradients by name"""
    from selfrec_amd.model.sequential.GRU4Rec import StagedSeqBatch
    from selfrec_amd.util.loss_torch import l2_reg_loss
    k = f"l{layers}"
    net = model.model
    params = dict(net.named_parameters())
    optimizer = torch.optim.Adam(net.parameters(), lr=model.lRate)
    net.train()
    grads0 = {}
    for s in range(3):
        seq, pos, y, neg = (gd[f"train{s}_{n}"] for n in ("seq", "pos", "y", "neg"))
        staged = StagedSeqBatch(seq, torch.device(device), pos, y, neg) if device != "cpu" else None
        hidden = net.forward(seq, pos, staged=staged)
        loss = model.calculate_loss(hidden, y, neg, pos, staged=staged) + l2_reg_loss(model.reg, net.item_emb)
        want = gd[f"{k}_loss"][s]
        assert abs(float(loss.detach()) - want) <= 1e-5 * abs(want), (s, float(loss.detach()), want)
        optimizer.zero_grad()
        loss.backward()
        if s == 0:
            for name, p in params.items():
                g = p.grad.detach().cpu().reshape(-1).numpy().astype(np.float64)
                want_g = gd[f"{k}_grad0_{name}_val"].astype(np.float64)
                assert np.abs(g[gd[f"sample_{k}_{name}"]] - want_g).max() <= 1e-4 * np.abs(want_g).max() + 1e-12, name
                assert abs(g.sum() - gd[f"{k}_grad0_{name}_sum"][0]) <= 1e-4 * np.abs(g).sum() + 1e-12, name
                grads0[name] = p.grad.detach().clone()
        optimizer.step()
        for name, p in params.items():
            v = p.detach().cpu().numpy()
            if s < 2:
                got, want_v = v.reshape(-1)[gd[f"sample_{k}_{name}"]], gd[f"{k}_step{s}_{name}_val"]
            else:
                got, want_v = v, gd[f"{k}_final_{name}"]
            assert np.abs(got - want_v).max() <= model.lRate / 2, (s, name)
    return grads0


def check_lists(gd, meta, model, layers):
    """predict rows and test() on the golden's final parameters: the lists equal, scores <= 1e-5 of their scale, both
    evaluation strings"""
    from selfrec_amd.util.evaluation import ranking_evaluation
    k = f"l{layers}"
    with torch.no_grad():
        for name, p in model.model.named_parameters():
            p.copy_(torch.from_numpy(gd[f"{k}_final_{name}"]))
    model.model.eval()
    want_rows = gd[f"{k}_predict0"]
    rows = model.predict(*(gd[f"test0_{n}"] for n in ("seq", "pos", "len")))
    assert rows.shape == want_rows.shape and np.abs(rows - want_rows).max() <= 1e-5 * np.abs(want_rows).max()
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


def test_registry_and_conf():
    from selfrec_amd import main
    from selfrec_amd.util.conf import ModelConf
    assert "GRU4Rec" in main.MODELS
    conf = ModelConf(os.path.join(REPO, "conf", "GRU4Rec.yaml"))
    assert conf["model"] == {"name": "GRU4Rec", "type": "sequential"}
    assert conf["GRU4Rec"] == {"n_layers": 1, "drop_rate": 0.2}
    assert (conf["embedding.size"], conf["batch.size"], conf["max.len"]) == (64, 256, 50)
    assert (conf["learning.rate"], conf["reg.lambda"], conf["item.ranking.topN"]) == (0.001, 0.0001, [10, 20])
    assert "beauty-seq" in conf["training.set"]


def test_route_function(golden, tmp_path, monkeypatch):
    from selfrec_amd.model.sequential import GRU4Rec as G
    _, meta = golden
    monkeypatch.delenv("SRH_GRU4REC_RNN", raising=False)
    assert G.rnn_route() == G.RNN_DEFAULT and G.RNN_DEFAULT in ("hip", "torch")
    assert make_model(meta, 1, tmp_path, monkeypatch, rnn="torch").model.rnn == "torch"
    assert make_model(meta, 1, tmp_path, monkeypatch, rnn="hip").model.rnn == "hip"
    monkeypatch.setenv("SRH_GRU4REC_RNN", "hip")
    assert G.rnn_route() == "hip"
    monkeypatch.setenv("SRH_GRU4REC_RNN", "Torch ")
    assert G.rnn_route() == "torch"
    monkeypatch.setenv("SRH_GRU4REC_RNN", "miopen")
    with pytest.raises(ValueError):
        G.rnn_route()


def test_a_cpu_model_and_a_shape_outside_the_envelope_take_torch(golden, tmp_path, monkeypatch):
    _, meta = golden
    net = make_model(meta, 1, tmp_path, monkeypatch, rnn="hip").model
    assert net.uses_kernel(12) and net.uses_kernel(512) and not net.uses_kernel(513) and not net.uses_kernel(12, on_device=False)
    net.rnn = "torch"
    assert not net.uses_kernel(12)
    net.rnn, net.emb_size = "hip", 128
    assert not net.uses_kernel(12)


def test_parameters_are_created_in_the_specified_order(golden, tmp_path, monkeypatch):
    gd, meta = golden
    for layers in meta["layers"]:
        model = seeded_model(meta, layers, tmp_path, monkeypatch)
        params = dict(model.model.named_parameters())
        assert list(params) == meta[f"l{layers}_param_names"]
        assert params["item_emb"].shape == (meta["item_num"] + 1, meta["conf"]["emb"])
        for name, p in params.items():
            assert np.array_equal(p.detach().numpy(), gd[f"l{layers}_init_{name}"]), name
        assert not hasattr(model.model, "pos_emb")


def test_sampler_stream_replays_the_golden(golden, tmp_path, monkeypatch):
    from selfrec_amd.util.sampler import next_batch_sequence, next_batch_sequence_for_test
    gd, meta = golden
    model = seeded_model(meta, 1, tmp_path, monkeypatch)
    c = meta["conf"]
    n = 0
    for b, batch in enumerate(next_batch_sequence(model.data, c["batch"], max_len=c["max_len"])):
        for got, key in zip(batch, ("seq", "pos", "y", "neg", "len")):
            assert np.array_equal(np.asarray(got), gd[f"train{b}_{key}"]), (b, key)
        n += 1
    assert n == meta["n_train_batches"]
    assert np.array_equal(np.asarray(random.getstate()[1], dtype=np.int64), gd["rng_after_epoch"])
    for b, batch in enumerate(next_batch_sequence_for_test(model.data, c["batch"], max_len=c["max_len"])):
        for got, key in zip(batch, ("seq", "pos", "len")):
            assert np.array_equal(np.asarray(got), gd[f"test{b}_{key}"]), (b, key)


def test_staged_batch_host_side(golden):
    """the lengths and both live plans the stager uploads: the padding id is in neither plan's rows"""
    from selfrec_amd import ops
    from selfrec_amd.model.sequential.GRU4Rec import StagedSeqBatch
    gd, _ = golden
    seq, pos, y, neg, ln = (gd[f"train0_{n}"] for n in ("seq", "pos", "y", "neg", "len"))
    st = StagedSeqBatch(seq, torch.device("cpu"), pos, y, neg)
    assert st.lens.tolist() == ln.tolist() and st.lens.dtype == torch.int32 and st.shape == seq.shape
    assert st.n_valid == int(np.count_nonzero(pos)) and st.valid.dtype == torch.uint8
    assert torch.equal(st.live.reshape(-1), torch.from_numpy(seq.reshape(-1) != 0))
    item_plan, bce_plan = st.item_plan, st.bce_plan
    assert [p.tolist() for p in item_plan] == [p.tolist() for p in ops.live_plan_host(seq.reshape(-1))]
    assert int(item_plan[0].numel()) == int(np.count_nonzero(seq)) and int(bce_plan[0].numel()) == 2 * st.n_valid
    assert bool((torch.from_numpy(seq.reshape(-1))[item_plan[0].long()] != 0).all())
    ev = StagedSeqBatch(seq, torch.device("cpu"))
    assert ev.y is None and ev.valid is None and ev.bce_plan is None and len(ev.item_plan) == 5
    bare = StagedSeqBatch(seq, torch.device("cpu"), item_plan=False)                 # evaluation: ids and lengths only
    assert bare.item_plan is None and bare.bce_plan is None and bare.lens.tolist() == ln.tolist()


@pytest.mark.parametrize("layers", [1, 2])
def test_cpu_model_reproduces_the_golden(golden, layers, tmp_path, monkeypatch):
    gd, meta = golden
    model = seeded_model(meta, layers, tmp_path, monkeypatch)
    replay_three_steps(gd, model, layers)
    check_lists(gd, meta, model, layers)


def test_padded_positions_are_exact_zeros_on_the_cpu(golden, tmp_path, monkeypatch):
    gd, meta = golden
    model = seeded_model(meta, 2, tmp_path, monkeypatch)
    model.model.eval()
    seq, pos = gd["train0_seq"], gd["train0_pos"]
    with torch.no_grad():
        hidden = model.model.forward(seq, pos)
    assert hidden.shape == seq.shape + (64,) and float(hidden[torch.from_numpy(seq == 0)].abs().max()) == 0.0
