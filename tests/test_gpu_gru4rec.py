"""GRU4Rec on the device: the golden's three Adam steps, predict rows and test() lists
(tests/golden/gru4rec.npz; the checks tests/test_gru4rec_cpu.py makes of the CPU model) by ``engine.rnn: hip`` and ``torch``,
with 1 and 2 layers; the item gradient's padding row; the evaluation call's bits; and one epoch through the launcher."""
import numpy as np
import pytest
import torch

from tests.test_gru4rec_cpu import check_lists, golden, replay_three_steps, seeded_model  # noqa: F401  (golden: the fixture)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.mark.parametrize("layers", [1, 2])
@pytest.mark.parametrize("rnn", ["hip", "torch"])
def test_model_reproduces_the_golden(golden, rnn, layers, tmp_path, monkeypatch):
    gd, meta = golden
    torch.cuda.set_device(0)
    model = seeded_model(meta, layers, tmp_path, monkeypatch, rnn=rnn)
    for name, p in model.model.named_parameters():
        assert np.array_equal(p.detach().numpy(), gd[f"l{layers}_init_{name}"]), name
    model.model.to(DEV)
    assert model.model.uses_kernel(meta["conf"]["max_len"]) == (rnn == "hip")
    grads0 = replay_three_steps(gd, model, layers, DEV)
    # the padding id's row: l2_reg_loss's share only -- the gather's and the loss's live plans never name it
    table = torch.from_numpy(gd[f"l{layers}_init_item_emb"])
    want = model.reg * table[0] / (table.norm(p=2) * table.shape[0])
    assert np.abs(grads0["item_emb"][0].cpu().numpy() - want.numpy()).max() <= 1e-5 * float(want.abs().max())
    check_lists(gd, meta, model, layers)


def test_item_gradient_padding_row_is_an_exact_zero(golden, tmp_path, monkeypatch):
    from selfrec_amd.model.sequential.GRU4Rec import StagedSeqBatch
    gd, meta = golden
    torch.cuda.set_device(0)
    model = seeded_model(meta, 1, tmp_path, monkeypatch, rnn="hip")
    net = model.model.to(DEV)
    net.train()
    seq, pos, y, neg = (gd[f"train0_{n}"] for n in ("seq", "pos", "y", "neg"))
    assert (seq == 0).any()
    staged = StagedSeqBatch(seq, torch.device(DEV), pos, y, neg)
    hidden = net.forward(seq, pos, staged=staged)
    assert float(hidden.detach()[torch.from_numpy(seq == 0).to(DEV)].abs().max()) == 0.0
    model.calculate_loss(hidden, y, neg, pos, staged=staged).backward()
    grad = net.item_emb.grad
    assert float(grad[0].abs().max()) == 0.0 and float(grad[1:].abs().max()) > 0.0


def test_evaluation_forward_holds_the_training_forward_bits(golden, tmp_path, monkeypatch):
    gd, meta = golden
    torch.cuda.set_device(0)
    model = seeded_model(meta, 2, tmp_path, monkeypatch, rnn="hip")
    net = model.model.to(DEV)
    net.eval()
    seq, pos = gd["test0_seq"], gd["test0_pos"]
    with torch.no_grad():
        plain = net.forward(seq, pos)                       # nothing saved
    saved = net.forward(seq, pos)                           # gates saved for a backward pass
    assert saved.requires_grad and torch.equal(plain, saved.detach())


def tiny_conf(tmp_path, rnn):
    from selfrec_amd import synth
    train, test = synth.make_sequence_dataset("tiny-seq")
    synth.write_sequences(str(tmp_path / "train.txt"), train)
    synth.write_sequences(str(tmp_path / "test.txt"), test)
    lines = [f"training.set: {tmp_path / 'train.txt'}", f"test.set: {tmp_path / 'test.txt'}", "model:", "  name: GRU4Rec",
             "  type: sequential", "item.ranking.topN: [10,20]", "embedding.size: 64", "max.epoch: 1", "batch.size: 32",
             "learning.rate: 0.001", "reg.lambda: 0.0001", "max.len: 50", "GRU4Rec:", "  n_layers: 1", "  drop_rate: 0.2",
             "output: ./results/", f"engine.rnn: {rnn}"]
    path = tmp_path / f"GRU4Rec_{rnn}.yaml"
    path.write_text("\n".join(lines) + "\n")
    return str(path)


def test_gru4rec_end_to_end(tmp_path, monkeypatch, capsys):
    from selfrec_amd import main
    torch.cuda.set_device(0)
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("SRH_GRU4REC_RNN", raising=False)
    from selfrec_amd.model.sequential.GRU4Rec import GRU4Rec
    seen = []
    train = GRU4Rec.train

    def recording_train(self):
        train(self)
        seen.append(self.epoch_losses)
    monkeypatch.setattr(GRU4Rec, "train", recording_train)
    main.main(["GRU4Rec", "--conf", tiny_conf(tmp_path, "hip"), "--synthetic", "tiny-seq"])
    out = capsys.readouterr().out
    assert "training: 1 batch 0 rec_loss:" in out and "Hit Ratio" in out and "NDCG" in out
    [[losses]] = seen                                          # one epoch: every batch's loss
    assert len(losses) > 1 and bool(np.isfinite(losses).all())
