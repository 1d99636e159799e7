#!/usr/bin/env python3
"""Reference-run golden for CL4SRec: runs the REFERENCE'S OWN model/sequential/CL4SRec.py on the CPU (make_golden.py's
.cuda() shims) on make_golden_sasrec.tiny_sequences(), d = 64, max.len = 12, 2 blocks, batch.size = 32, drop_rate = 0,
aug_rate = 0.5, cl_rate = 0.05: aug_type 0 (crop) with 1 and 2 heads, aug_type 1 (reorder) and 2 (mask) with one head.
Sequence lengths run from 1 to 11, so crop meets len = 1.

The steps are driven as CL4SRec.train() drives them (CL4SRec.py:34-64: the same expressions in the same order).  The
sampler is a lazy generator on the same ``random`` stream as the augmentors, so the draws of step n fall between the
sampler's batches n and n + 1: the epoch is recorded in that interleaving.

Recorded (tests/golden/cl4srec.npz + cl4srec_meta.json), with the run key k = t{aug_type}h{heads}:
  sample_{param}                       the sampled element indices of a tensor (every element of tensors up to 512)
  init_{param}_val / _sum              initial parameters (torch.manual_seed(41); the same for every run): the elements
                                       at sample_{param} and the float64 sum
  t{T}_train{b}_{seq,pos,y,neg,len}    every batch of the first epoch (random.seed(2718), np.random.seed(314)) as train()
                                       interleaves it with the augmentation draws
  t{T}_aug{b}_{seq1,pos1,len1,seq2,pos2,len2}   both views of step b (pos / len of types 1 and 2: the batch's own)
  t{T}_rng_after_epoch / t{T}_np_rng_after_epoch   both generator states after the epoch (numpy: the 624 keys, then pos)
  {k}_loss / _rec_loss / _cl_loss      the 3 steps' batch, rec and cl_rate * InfoNCE losses (float64 of the float32 values)
  {k}_grad0_{param}_val / _sum         step 0's gradients, sampled the same way
  {k}_step{s}_{param}_val / _sum       parameters after step s = 0 and after the last step s = 2, sampled the same way
  t0h1_final_{param}                   parameters after step 2, whole: the one copy a file under the size limit for
                                       committed files has room for
  {k}_rec_ids / _rec_scores            test() on the run's final parameters (one-head runs): item ids (-1 padded) and
                                       float64 scores;  meta {k}_evaluation: both evaluation strings.  Only t0h1's can be
                                       replayed from this file (it alone has its parameters whole).

Run:  python tests/golden/make_golden_cl4srec.py        (writes next to this file)
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

from data.augmentor import SequenceAugmentor  # noqa: E402
from util.conf import ModelConf  # noqa: E402
from util.evaluation import ranking_evaluation  # noqa: E402
from util.loss_torch import InfoNCE, l2_reg_loss  # noqa: E402
from util import sampler as ref_sampler  # noqa: E402

SEEDS = dict(torch_seed=41, sampler_seed=2718, numpy_seed=314, data_seed=7, sample_seed=43)
CONF = dict(emb=64, max_len=12, n_blocks=2, batch=32, drop_rate=0.0, lr=0.001, reg=0.0001, topN=[10, 20], aug_rate=0.5,
            cl_rate=0.05)
RUNS = ((0, 1), (0, 2), (1, 1), (2, 1))          # (aug_type, heads)
N_SAMPLE = 512
WHOLE_FINAL = "t0h1"       # a committed file has room for ONE whole copy of the parameters next to the samples


def write_conf(tmp, aug_type, heads):
    path = os.path.join(tmp, "CL4SRec.yaml")
    with open(path, "w") as f:
        f.write("\n".join([
            "training.set: ./train.txt", "test.set: ./test.txt", "model:", "  name: CL4SRec", "  type: sequential",
            f"item.ranking.topN: {CONF['topN']}", f"embedding.size: {CONF['emb']}", "max.epoch: 1",
            f"batch.size: {CONF['batch']}", f"learning.rate: {CONF['lr']}", f"reg.lambda: {CONF['reg']}",
            f"max.len: {CONF['max_len']}", "CL4SRec:", f"  n_blocks: {CONF['n_blocks']}",
            f"  drop_rate: {CONF['drop_rate']}", f"  n_heads: {heads}", f"  aug_type: {aug_type}",
            f"  aug_rate: {CONF['aug_rate']}", f"  cl_rate: {CONF['cl_rate']}", "output: ./results/"]) + "\n")
    return ModelConf(path)


def draw_views(model, seq, pos, seq_len):
    """the two views of CL4SRec.py:37-57, in its order: [(seq, pos, len)] * 2"""
    out = []
    for _ in range(2):
        if model.aug_type == 0:
            out.append(SequenceAugmentor.item_crop(seq, seq_len, model.aug_rate))
        elif model.aug_type == 1:
            out.append((SequenceAugmentor.item_reorder(seq, seq_len, model.aug_rate), pos, seq_len))
        else:
            out.append((SequenceAugmentor.item_mask(seq, seq_len, model.aug_rate, model.data.item_num + 1), pos, seq_len))
    return out


def main():
    import importlib
    mod = importlib.import_module("model.sequential.CL4SRec")
    train, test = MS.tiny_sequences()
    out, meta = {}, {"conf": CONF, "runs": [list(r) for r in RUNS], "train": train, "test": test, **SEEDS}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            for T, H in RUNS:
                k = f"t{T}h{H}"
                conf = write_conf(tmp, T, H)
                torch.manual_seed(SEEDS["torch_seed"]); random.seed(SEEDS["sampler_seed"]); np.random.seed(SEEDS["numpy_seed"])
                model = mod.CL4SRec(conf, {n: list(v) for n, v in train.items()}, {n: list(v) for n, v in test.items()})
                d, net = model.data, model.model
                params = dict(net.named_parameters())
                if "param_names" not in meta:
                    meta.update(raw_seq_num=d.raw_seq_num, item_num=d.item_num, param_names=list(params))
                    rs = np.random.RandomState(SEEDS["sample_seed"])
                    for name, p in params.items():
                        n = p.numel()
                        out[f"sample_{name}"] = (np.arange(n) if n <= N_SAMPLE else
                                                 np.sort(rs.choice(n, N_SAMPLE, replace=False))).astype(np.int64)
                        MS.sampled(out, f"init_{name}", p, out[f"sample_{name}"])
                else:
                    for name, p in params.items():
                        assert np.array_equal(out[f"init_{name}_val"], p.detach().numpy().reshape(-1)[out[f"sample_{name}"]]), name
                optimizer = torch.optim.Adam(net.parameters(), lr=model.lRate)
                losses, rec_losses, cl_losses = [], [], []
                first = f"t{T}_rng_after_epoch" not in out
                n_batches = 0
                net.train()
                for b, batch in enumerate(ref_sampler.next_batch_sequence(d, model.batch_size, max_len=model.max_len)):
                    seq, pos, y, neg_idx, seq_len = batch
                    views = draw_views(model, seq, pos, seq_len)
                    n_batches += 1
                    rec = {f"t{T}_train{b}_{n}": np.asarray(v, dtype=np.int32)
                           for n, v in zip(("seq", "pos", "y", "neg", "len"), batch)}
                    for v, (a_seq, a_pos, a_len) in enumerate(views, 1):
                        rec[f"t{T}_aug{b}_seq{v}"] = np.asarray(a_seq, dtype=np.int32)
                        rec[f"t{T}_aug{b}_pos{v}"] = np.asarray(a_pos, dtype=np.int32)
                        rec[f"t{T}_aug{b}_len{v}"] = np.asarray(a_len, dtype=np.int32)
                    for key, val in rec.items():
                        if first:
                            out[key] = val
                        else:
                            assert np.array_equal(out[key], val), key
                    if b >= 3:
                        continue
                    seq_emb = net.forward(seq, pos)
                    cl_rows = []
                    for a_seq, a_pos, a_len in views:
                        emb = net.forward(a_seq, a_pos)
                        cl_rows.append(torch.cat([emb[i, last - 1, :].view(-1, model.emb_size)
                                                  for i, last in enumerate(a_len)], 0))
                    cl_loss = model.cl_rate * InfoNCE(cl_rows[0], cl_rows[1], 1, True)
                    rec_loss = model.calculate_loss(seq_emb, y, neg_idx, pos)
                    batch_loss = rec_loss + l2_reg_loss(model.reg, net.item_emb) + cl_loss
                    optimizer.zero_grad()
                    batch_loss.backward()
                    if b == 0:
                        for name, p in params.items():
                            MS.sampled(out, f"{k}_grad0_{name}", p.grad, out[f"sample_{name}"])
                    optimizer.step()
                    losses.append(float(batch_loss.detach()))
                    rec_losses.append(float(rec_loss.detach()))
                    cl_losses.append(float(cl_loss.detach()))
                    for name, p in params.items():
                        if b != 1:
                            MS.sampled(out, f"{k}_step{b}_{name}", p, out[f"sample_{name}"])
                        if b == 2 and k == WHOLE_FINAL:
                            out[f"{k}_final_{name}"] = p.detach().numpy().copy()
                state, np_state = random.getstate(), np.random.get_state()
                if first:
                    meta[f"t{T}_n_train_batches"] = n_batches
                    out[f"t{T}_rng_after_epoch"] = np.asarray(state[1], dtype=np.int64)
                    out[f"t{T}_np_rng_after_epoch"] = np.r_[np.asarray(np_state[1], dtype=np.int64), np_state[2]]
                else:
                    assert np.array_equal(out[f"t{T}_rng_after_epoch"], np.asarray(state[1], dtype=np.int64))
                out[f"{k}_loss"] = np.asarray(losses, dtype=np.float64)
                out[f"{k}_rec_loss"] = np.asarray(rec_losses, dtype=np.float64)
                out[f"{k}_cl_loss"] = np.asarray(cl_losses, dtype=np.float64)
                meta[f"{k}_losses"] = losses
                if H != 1:
                    continue
                net.eval()
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
    np.savez_compressed(os.path.join(HERE, "cl4srec.npz"), **out)
    with open(os.path.join(HERE, "cl4srec_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print(json.dumps({k: v for k, v in meta.items() if k not in ("train", "test")}, indent=1))


if __name__ == "__main__":
    main()
