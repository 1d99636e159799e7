"""DuoRec on the device: the golden's three Adam steps (tests/golden/duorec.npz; the check
tests/test_duorec_cpu.py makes of the CPU model) by ``engine.duo: hip`` and ``pair``, with 1 and 2 heads, on one stacked pass
and on three; the dropout-only view in train mode; and one epoch through the launcher."""
import random

import numpy as np
import pytest
import torch

from tests.test_cl4srec_cpu import check_initial_parameters
from tests.test_duorec_cpu import ROUTE_ENVS, golden, make_model, replay_three_steps  # noqa: F401  (golden: the fixture)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.mark.parametrize("views", ["one", "three"])
@pytest.mark.parametrize("heads", [1, 2])
@pytest.mark.parametrize("duo", ["hip", "pair"])
def test_model_reproduces_the_golden(golden, duo, heads, views, tmp_path, monkeypatch):
    gd, meta = golden
    torch.cuda.set_device(0)
    torch.manual_seed(meta["torch_seed"]); random.seed(meta["sampler_seed"])
    model = make_model(meta, heads, tmp_path, monkeypatch, duo=duo, views=views)
    check_initial_parameters(gd, dict(model.model.named_parameters()))
    model.model.to(DEV)
    assert model.duo_kernel() == (duo == "hip")
    replay_three_steps(gd, meta, model, heads, DEV)


def tiny_conf(tmp_path, duo):
    from selfrec_amd import synth
    train, test = synth.make_sequence_dataset("tiny-seq")
    synth.write_sequences(str(tmp_path / "train.txt"), train)
    synth.write_sequences(str(tmp_path / "test.txt"), test)
    lines = [f"training.set: {tmp_path / 'train.txt'}", f"test.set: {tmp_path / 'test.txt'}", "model:", "  name: DuoRec",
             "  type: sequential", "item.ranking.topN: [10,20]", "embedding.size: 64", "max.epoch: 1", "batch.size: 32",
             "learning.rate: 0.001", "reg.lambda: 0.0001", "max.len: 50", "DuoRec:", "  n_blocks: 2", "  drop_rate: 0.2",
             "  n_heads: 1", "  cl_rate: 0.1", "output: ./results/", f"engine.duo: {duo}"]
    path = tmp_path / f"DuoRec_{duo}.yaml"
    path.write_text("\n".join(lines) + "\n")
    return str(path)


def test_dropout_only_view_differs_in_every_row_and_both_terms_are_finite(tmp_path, monkeypatch):
    from selfrec_amd import ops
    from selfrec_amd.model.sequential.CL4SRec import StagedViews
    from selfrec_amd.model.sequential.DuoRec import DuoRec
    from selfrec_amd.util.conf import ModelConf
    from selfrec_amd.util.sampler import next_batch_sequence_indexed, same_target_positives
    torch.cuda.set_device(0)
    monkeypatch.chdir(tmp_path)
    for env in ROUTE_ENVS:
        monkeypatch.delenv(env, raising=False)
    conf = ModelConf(tiny_conf(tmp_path, "hip"))
    from selfrec_amd.data.loader import FileIO
    random.seed(5); torch.manual_seed(5)
    model = DuoRec(conf, FileIO.load_data_set(conf["training.set"], "sequential"),
                   FileIO.load_data_set(conf["test.set"], "sequential"))
    net = model.model.to(DEV)
    net.train()
    seq, pos, y, neg, seq_len, rows = next(next_batch_sequence_indexed(model.data, model.batch_size, max_len=model.max_len))
    positives = same_target_positives(model.data, rows, model.max_len)[:3]
    staged = StagedViews([(seq, pos, None), (seq, pos, seq_len), positives], y, neg, DEV, "one", "hip", anchor_last=seq_len)
    B = staged.B
    assert staged.idx.shape == (3, B) and np.array_equal(staged.idx.cpu().numpy(), staged.idx_host)
    with torch.no_grad():
        out = net.forward(None, None, staged=staged, group=0).reshape(-1, model.emb_size)
        h_a, h_p = out[staged.idx[0].long()], out[staged.idx[1].long()]
        assert bool((h_a != h_p).any(dim=1).all())                   # the same ids, another dropout draw: every row differs
        losses = ops.DuoNceFn.apply(1.0, 1.0, 1.0, staged.idx, staged.idx_host, out)
    assert losses.shape == (2,) and bool(torch.isfinite(losses).all()) and float(losses.min()) >= 0.0
    total, rec, cl = model.step_losses(seq, pos, y, neg, seq_len, positives)
    assert all(bool(torch.isfinite(t)) for t in (total, rec, cl))
    total.backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())


def test_duorec_end_to_end(tmp_path, monkeypatch, capsys):
    from selfrec_amd import main
    torch.cuda.set_device(0)
    monkeypatch.chdir(tmp_path)
    for env in ROUTE_ENVS:
        monkeypatch.delenv(env, raising=False)
    main.main(["DuoRec", "--conf", tiny_conf(tmp_path, "hip"), "--synthetic", "tiny-seq"])
    out = capsys.readouterr().out
    assert "training: 1 batch 0 batch_loss:" in out and "Hit Ratio" in out and "NDCG" in out
