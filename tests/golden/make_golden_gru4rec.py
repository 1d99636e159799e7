#!/usr/bin/env python3
"""Reference-composed golden for GRU4Rec.  The reference ships no GRU4Rec, so this script composes the REFERENCE'S OWN
pieces, imported at generation time on the CPU (make_golden.py's .cuda() shims) -- data/sequence.Sequence,
util/sampler.next_batch_sequence, model/sequential/SASRec.py's BCE expression (calculate_loss), predict and the base
class's test(), util/loss_torch.l2_reg_loss -- around torch's own nn.GRU, into the step DESIGN.md 4.30 specifies:

    x = emb_dropout(item_emb[seq]) * live;  out = gru(x)[0] * live;  loss = BCE(out, y, neg, pos) + l2_reg_loss(reg, item_emb)

on make_golden_sasrec.tiny_sequences(), d = 64, max.len = 12, batch.size = 32, drop_rate = 0, with 1 and 2 layers.  The
network is created after torch.manual_seed(41) in the order item_emb (Xavier-uniform), Dropout, nn.GRU.

Recorded (tests/golden/gru4rec.npz + gru4rec_meta.json), run key k = l{layers}:
  sample_{k}_{param}                             the sampled elements of every parameter (all of tensors up to 512)
  {k}_init_{param}                               initial parameters, whole
  train{b}_{seq,pos,y,neg,len}                   every batch of the first epoch (random.seed(2718));  rng_after_epoch
  test{b}_{seq,pos,len}                          the evaluation batches
  {k}_loss                                       the 3 batch losses (float64 of the float32 values)
  {k}_grad0_{param}_val / _sum                   step 0's gradients, sampled, and their float64 sum
  {k}_step{s}_{param}_val / _sum                 parameters after steps 0 and 1, sampled
  {k}_final_{param}                              parameters after step 2, whole
  {k}_predict0                                   predict() of the first evaluation batch on those (float32 score rows)
  {k}_rec_ids / _rec_scores                      test() on those;  meta {k}_evaluation: both evaluation strings

Run:  python tests/golden/make_golden_gru4rec.py        (writes next to this file)
"""
import contextlib
import io
import json
import os
import random
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402,F401  (numba stub, .cuda() shims, the reference on sys.path)
import make_golden_sasrec as MS  # noqa: E402

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from util.evaluation import ranking_evaluation  # noqa: E402
from util.loss_torch import l2_reg_loss  # noqa: E402
from util import sampler as ref_sampler  # noqa: E402

SEEDS = dict(torch_seed=41, sampler_seed=2718, data_seed=7, sample_seed=43)
CONF = dict(emb=64, max_len=12, batch=32, drop_rate=0.0, lr=0.001, reg=0.0001, topN=[10, 20])
LAYERS = (1, 2)
N_SAMPLE = 512
N_STEPS = 3


class GruNet(nn.Module):
    """DESIGN.md 4.30's network in torch's own words"""

    def __init__(self, item_num, d, n_layers, drop_rate):
        super().__init__()
        self.item_emb = nn.Parameter(nn.init.xavier_uniform_(torch.empty(item_num + 1, d)))
        self.emb_dropout = nn.Dropout(drop_rate)
        self.gru = nn.GRU(d, d, num_layers=n_layers, batch_first=True)

    def forward(self, seq, pos):
        ids = torch.from_numpy(np.asarray(seq).astype(np.int64))
        live = (ids != 0).unsqueeze(-1)
        return self.gru(self.emb_dropout(self.item_emb[ids]) * live)[0] * live


def main():
    import importlib
    mod = importlib.import_module("model.sequential.SASRec")
    train, test = MS.tiny_sequences()
    out, meta = {}, {"conf": CONF, "layers": list(LAYERS), "train": train, "test": test, **SEEDS}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            for n_layers in LAYERS:
                k = f"l{n_layers}"
                first = n_layers == LAYERS[0]
                conf = MS.write_conf(tmp, 1)
                random.seed(SEEDS["sampler_seed"])
                model = mod.SASRec(conf, {n: list(v) for n, v in train.items()}, {n: list(v) for n, v in test.items()})
                d = model.data
                torch.manual_seed(SEEDS["torch_seed"])
                net = model.model = GruNet(d.item_num, model.emb_size, n_layers, CONF["drop_rate"])
                params = dict(net.named_parameters())
                meta[f"{k}_param_names"] = list(params)
                rs = np.random.RandomState(SEEDS["sample_seed"])
                for name, p in params.items():
                    n = p.numel()
                    out[f"sample_{k}_{name}"] = (np.arange(n) if n <= N_SAMPLE else
                                                 np.sort(rs.choice(n, N_SAMPLE, replace=False))).astype(np.int64)
                    out[f"{k}_init_{name}"] = p.detach().numpy().copy()
                batches = list(ref_sampler.next_batch_sequence(d, model.batch_size, max_len=model.max_len))
                state = np.asarray(random.getstate()[1], dtype=np.int64)
                tests = list(ref_sampler.next_batch_sequence_for_test(d, model.batch_size, max_len=model.max_len))
                rec = {"rng_after_epoch": state}
                for b, batch in enumerate(batches):
                    rec.update({f"train{b}_{n}": np.asarray(v, dtype=np.int32)
                                for n, v in zip(("seq", "pos", "y", "neg", "len"), batch)})
                for b, batch in enumerate(tests):
                    rec.update({f"test{b}_{n}": np.asarray(v, dtype=np.int32) for n, v in zip(("seq", "pos", "len"), batch)})
                for key, val in rec.items():
                    if first:
                        out[key] = val
                    else:
                        assert np.array_equal(out[key], val), key
                if first:
                    meta.update(raw_seq_num=d.raw_seq_num, item_num=d.item_num, n_train_batches=len(batches),
                                n_test_batches=len(tests))
                optimizer = torch.optim.Adam(net.parameters(), lr=model.lRate)
                losses = []
                for s in range(N_STEPS):
                    seq, pos, y, neg_idx, _ = batches[s]
                    net.train()
                    seq_emb = net.forward(seq, pos)
                    batch_loss = model.calculate_loss(seq_emb, y, neg_idx, pos) + l2_reg_loss(model.reg, net.item_emb)
                    optimizer.zero_grad()
                    batch_loss.backward()
                    if s == 0:
                        for name, p in params.items():
                            MS.sampled(out, f"{k}_grad0_{name}", p.grad, out[f"sample_{k}_{name}"])
                    optimizer.step()
                    losses.append(float(batch_loss.detach()))
                    for name, p in params.items():
                        if s < N_STEPS - 1:
                            MS.sampled(out, f"{k}_step{s}_{name}", p, out[f"sample_{k}_{name}"])
                        else:
                            out[f"{k}_final_{name}"] = p.detach().numpy().copy()
                out[f"{k}_loss"] = np.asarray(losses, dtype=np.float64)
                meta[f"{k}_losses"] = losses
                net.eval()
                out[f"{k}_predict0"] = np.asarray(model.predict(*tests[0]), dtype=np.float32)
                with contextlib.redirect_stdout(io.StringIO()):
                    rec_list = model.test()
                names = [n for n, _ in d.original_seq]
                ids = np.full((len(names), model.max_N), -1, dtype=np.int32)
                scores = np.zeros((len(names), model.max_N), dtype=np.float64)
                for r, n in enumerate(names):
                    for c, (item, sc) in enumerate(rec_list[n]):
                        ids[r, c], scores[r, c] = d.item[item], float(sc)
                out[f"{k}_rec_ids"], out[f"{k}_rec_scores"] = ids, scores
                meta[f"{k}_evaluation"] = dict(topN=ranking_evaluation(d.test_set, rec_list, model.topN),
                                               maxN=ranking_evaluation(d.test_set, rec_list, [model.max_N]))
        finally:
            os.chdir(cwd)
    meta.update(torch=torch.__version__, numpy=np.__version__)
    np.savez_compressed(os.path.join(HERE, "gru4rec.npz"), **out)
    with open(os.path.join(HERE, "gru4rec_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print(json.dumps({k: v for k, v in meta.items() if k not in ("train", "test")}, indent=1))


if __name__ == "__main__":
    main()
