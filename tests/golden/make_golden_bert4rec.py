#!/usr/bin/env python3
"""Reference-run golden for BERT4Rec: runs the REFERENCE'S OWN model/sequential/BERT4Rec.py on the CPU (make_golden.py's
.cuda() shims) on make_golden_sasrec.tiny_sequences(), d = 64, max.len = 12, 2 blocks, heads 1 and 2, batch.size = 32,
drop_rate = 0, mask_rate = 0.5, lr 1e-3, reg 1e-4.

The steps are driven as BERT4Rec.train() drives them (BERT4Rec.py:31-41: a batch comes off the sampler, item_mask_for_bert
draws its masks from the same ``random`` generator before the sampler goes on; forward, calculate_loss + l2_reg_loss, one
torch.optim.Adam over model.parameters()).

Recorded (tests/golden/bert4rec.npz + bert4rec_meta.json):
  train{b}_{seq,pos,len}               every batch of the first epoch (random.seed(2718)), with its
  train{b}_{aug,masked,labels}         item_mask_for_bert outputs in the reference's order;  rng_after_epoch: the
                                       generator state after the epoch;  test{b}_{seq,pos,len}: the evaluation batches
  init_{param}                         initial parameters (torch.manual_seed(41); the same for both head counts)
  h{H}_loss                            the 3 batch losses (float64 of the float32 values)
  h{H}_grad0_{param}_val / _sum        step 0's gradients: the elements at sample_{param} (every element of tensors up to
                                       512) and the float64 sum
  h{H}_step{s}_{param}_val / _sum      parameters after step s = 0, 1, sampled the same way
  h{H}_final_{param}                   parameters after step 2, whole
  h{H}_pred{b}_{seq,pos,score}         predict() on test batch b with those: the edited seq / pos and the score rows
  h{H}_rec_ids / _rec_scores           test() on those: item ids (-1 padded: rows 0 and item_num + 1 leave the list) and
                                       float64 scores
  meta h{H}_evaluation                 ranking_evaluation(test_set, rec_list, topN) and (.., [max_N])

Run:  python tests/golden/make_golden_bert4rec.py        (writes next to this file)
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
from make_golden_sasrec import N_SAMPLE, SEEDS, sampled, tiny_sequences  # noqa: E402

import torch  # noqa: E402

from util.conf import ModelConf  # noqa: E402
from util.evaluation import ranking_evaluation  # noqa: E402
from util.loss_torch import l2_reg_loss  # noqa: E402
from util import sampler as ref_sampler  # noqa: E402

CONF = dict(emb=64, max_len=12, n_blocks=2, batch=32, drop_rate=0.0, mask_rate=0.5, lr=0.001, reg=0.0001, topN=[10, 20])
HEADS = (1, 2)


def write_conf(tmp, heads):
    path = os.path.join(tmp, "BERT4Rec.yaml")
    with open(path, "w") as f:
        f.write("\n".join([
            "training.set: ./train.txt", "test.set: ./test.txt", "model:", "  name: BERT4Rec", "  type: sequential",
            f"item.ranking.topN: {CONF['topN']}", f"embedding.size: {CONF['emb']}", "max.epoch: 1",
            f"batch.size: {CONF['batch']}", f"learning.rate: {CONF['lr']}", f"reg.lambda: {CONF['reg']}",
            f"max.len: {CONF['max_len']}", "BERT4Rec:", f"  n_blocks: {CONF['n_blocks']}",
            f"  drop_rate: {CONF['drop_rate']}", f"  n_heads: {heads}", f"  mask_rate: {CONF['mask_rate']}",
            "output: ./results/"]) + "\n")
    return ModelConf(path)


def main():
    import importlib
    mod = importlib.import_module("model.sequential.BERT4Rec")
    train, test = tiny_sequences()
    out, meta = {}, {"conf": CONF, "heads": list(HEADS), "train": train, "test": test, **SEEDS}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            for H in HEADS:
                conf = write_conf(tmp, H)
                torch.manual_seed(SEEDS["torch_seed"]); random.seed(SEEDS["sampler_seed"])
                model = mod.BERT4Rec(conf, {k: list(v) for k, v in train.items()}, {k: list(v) for k, v in test.items()})
                d, net = model.data, model.model
                params = dict(net.named_parameters())
                if H == HEADS[0]:
                    meta.update(raw_seq_num=d.raw_seq_num, item_num=d.item_num, param_names=list(params))
                    rs = np.random.RandomState(SEEDS["sample_seed"])
                    for name, p in params.items():
                        n = p.numel()
                        out[f"sample_{name}"] = (np.arange(n) if n <= N_SAMPLE else
                                                 np.sort(rs.choice(n, N_SAMPLE, replace=False))).astype(np.int64)
                        out[f"init_{name}"] = p.detach().numpy().copy()
                else:
                    for name, p in params.items():
                        assert np.array_equal(out[f"init_{name}"], p.detach().numpy()), name
                # the epoch's host stream, as train() interleaves it: sampler batch, then the batch's masks
                batches = []
                for seq, pos, _y, _neg, ln in ref_sampler.next_batch_sequence(d, model.batch_size, max_len=model.max_len):
                    aug, masked, labels = model.item_mask_for_bert(seq, ln, model.aug_rate, d.item_num + 1)
                    batches.append((seq, pos, ln, aug, masked, labels))
                state = random.getstate()
                if H == HEADS[0]:
                    meta["n_train_batches"] = len(batches)
                    meta["n_masked"] = [int(b[5].shape[0]) for b in batches]
                    for b, arrays in enumerate(batches):
                        for k, v in zip(("seq", "pos", "len", "aug", "masked", "labels"), arrays):
                            out[f"train{b}_{k}"] = np.asarray(v, dtype=np.int32)
                    out["rng_after_epoch"] = np.asarray(state[1], dtype=np.int64)
                    tests = [tuple(np.asarray(a).copy() for a in t) for t in
                             ref_sampler.next_batch_sequence_for_test(d, model.batch_size, max_len=model.max_len)]
                    meta["n_test_batches"] = len(tests)
                    meta["n_full_length_test_rows"] = int(sum((t[2] == model.max_len).sum() for t in tests))
                    for b, (seq, pos, ln) in enumerate(tests):
                        for k, v in zip(("seq", "pos", "len"), (seq, pos, ln)):
                            out[f"test{b}_{k}"] = np.asarray(v, dtype=np.int32)
                else:
                    assert np.array_equal(out["rng_after_epoch"], np.asarray(state[1], dtype=np.int64))
                optimizer = torch.optim.Adam(net.parameters(), lr=model.lRate)
                losses = []
                for s in range(3):
                    _seq, pos, _ln, aug, masked, labels = batches[s]
                    net.train()
                    seq_emb = net.forward(aug, pos)
                    rec_loss = model.calculate_loss(seq_emb, masked, labels)
                    batch_loss = rec_loss + l2_reg_loss(model.reg, net.item_emb)
                    optimizer.zero_grad()
                    batch_loss.backward()
                    if s == 0:
                        for name, p in params.items():
                            sampled(out, f"h{H}_grad0_{name}", p.grad, out[f"sample_{name}"])
                    optimizer.step()
                    losses.append(float(batch_loss.detach()))
                    for name, p in params.items():
                        if s < 2:
                            sampled(out, f"h{H}_step{s}_{name}", p, out[f"sample_{name}"])
                        else:
                            out[f"h{H}_final_{name}"] = p.detach().numpy().copy()
                out[f"h{H}_loss"] = np.asarray(losses, dtype=np.float64)
                net.eval()
                for b in range(meta["n_test_batches"]):
                    seq, pos, ln = (out[f"test{b}_{k}"].astype(np.int64) for k in ("seq", "pos", "len"))
                    score = model.predict(seq, pos, ln)                  # (edits seq and pos in place)
                    out[f"h{H}_pred{b}_seq"], out[f"h{H}_pred{b}_pos"] = seq.astype(np.int32), pos.astype(np.int32)
                    out[f"h{H}_pred{b}_score"] = np.asarray(score, dtype=np.float32)
                with contextlib.redirect_stdout(io.StringIO()):
                    rec = model.test()
                names = [n for n, _ in d.original_seq]
                ids = np.full((len(names), model.max_N), -1, dtype=np.int32)
                scores = np.zeros((len(names), model.max_N), dtype=np.float64)
                for r, n in enumerate(names):
                    for c, (item, sc) in enumerate(rec[n]):
                        ids[r, c], scores[r, c] = d.item[item], float(sc)
                out[f"h{H}_rec_ids"], out[f"h{H}_rec_scores"] = ids, scores
                meta[f"h{H}_evaluation"] = dict(topN=ranking_evaluation(d.test_set, rec, model.topN),
                                                maxN=ranking_evaluation(d.test_set, rec, [model.max_N]))
                meta[f"h{H}_losses"] = losses
        finally:
            os.chdir(cwd)
    meta.update(torch=torch.__version__, numpy=np.__version__)
    np.savez_compressed(os.path.join(HERE, "bert4rec.npz"), **out)
    with open(os.path.join(HERE, "bert4rec_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print(json.dumps({k: v for k, v in meta.items() if k not in ("train", "test")}, indent=1))


if __name__ == "__main__":
    main()
