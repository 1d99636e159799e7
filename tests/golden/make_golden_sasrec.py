#!/usr/bin/env python3
"""Reference-run golden for SASRec: runs the REFERENCE'S OWN model/sequential/SASRec.py on the CPU (make_golden.py's
.cuda() shims) on a tiny generated sequence set, d = 64, max.len = 12, 2 blocks, heads 1 and 2, batch.size = 32,
drop_rate = 0 (the masks nn.MultiheadAttention draws cannot be recorded from outside it: the dropout paths are covered
by tests/sasrec_ref.py with injected masks).

The dataset (meta["train"] / meta["test"], the loader's {seq: [items]} dicts): 124 training lines over 80 items -- 6
sequences longer than max.len, 4 of a single item (dropped by Sequence); 125 test lines, one of a sequence that training
does not have and 4 of the dropped ones.

The steps are driven as SASRec.train() drives them (SASRec.py:26-38: the same expressions in the same order, one
torch.optim.Adam over model.parameters()).

Recorded (tests/golden/sasrec.npz + sasrec_meta.json):
  seq_names / seq_flat / seq_ptr       Sequence.original_seq;  item_names: id2item[1..]; meta: test_set, counts
  train{b}_{seq,pos,y,neg,len}         every batch of the first epoch (random.seed(2718));  rng_after_epoch: the
                                       generator state after it;  test{b}_{seq,pos,len}: the evaluation batches
  init_{param}                         initial parameters (torch.manual_seed(41); the same for both head counts)
  h{H}_loss                            the 3 batch losses (float64 of the float32 values)
  h{H}_grad0_{param}_val / _sum        step 0's gradients: the elements at sample_{param} (every element of tensors up to
                                       512) and the float64 sum
  h{H}_step{s}_{param}_val / _sum      parameters after step s = 0, 1, sampled the same way
  h{H}_final_{param}                   parameters after step 2, whole
  h{H}_rec_ids / _rec_scores           test() on those: item ids (-1 padded: row 0 leaves the list) and float64 scores
  meta h{H}_evaluation                 ranking_evaluation(test_set, rec_list, topN) and (.., [max_N])

Run:  python tests/golden/make_golden_sasrec.py        (writes next to this file)
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
import make_golden as MG  # noqa: E402  (numba stub, .cuda() shims, the reference on sys.path)

import torch  # noqa: E402

from util.conf import ModelConf  # noqa: E402
from util.evaluation import ranking_evaluation  # noqa: E402
from util.loss_torch import l2_reg_loss  # noqa: E402
from util import sampler as ref_sampler  # noqa: E402

SEEDS = dict(torch_seed=41, sampler_seed=2718, data_seed=7, sample_seed=43)
CONF = dict(emb=64, max_len=12, n_blocks=2, batch=32, drop_rate=0.0, lr=0.001, reg=0.0001, topN=[10, 20])
HEADS = (1, 2)
N_SAMPLE = 512


def tiny_sequences():
    rs = np.random.RandomState(SEEDS["data_seed"])
    n_items = 80
    succ = rs.permutation(n_items)
    train, test = {}, {}
    for s in range(124):
        if s % 31 == 5:
            n = 1                                           # dropped by Sequence
        elif s % 20 == 3:
            n = int(rs.randint(14, 20))                     # longer than max.len
        else:
            n = int(rs.randint(2, 12))
        items = [int(rs.randint(n_items))]
        while len(items) < n + 1:
            items.append(int(succ[items[-1]]) if rs.rand() < 0.6 else int(rs.randint(n_items)))
        train[f"s{s}"] = [f"i{v}" for v in items[:-1]]
        test[f"s{s}"] = [f"i{items[-1]}"]                   # (ranking_evaluation wants a test line per kept sequence)
    test["s_unseen"] = ["i3", "i4"]                        # a test sequence training does not have
    return train, test


def write_conf(tmp, heads):
    path = os.path.join(tmp, "SASRec.yaml")
    with open(path, "w") as f:
        f.write("\n".join([
            "training.set: ./train.txt", "test.set: ./test.txt", "model:", "  name: SASRec", "  type: sequential",
            f"item.ranking.topN: {CONF['topN']}", f"embedding.size: {CONF['emb']}", "max.epoch: 1",
            f"batch.size: {CONF['batch']}", f"learning.rate: {CONF['lr']}", f"reg.lambda: {CONF['reg']}",
            f"max.len: {CONF['max_len']}", "SASRec:", f"  n_blocks: {CONF['n_blocks']}",
            f"  drop_rate: {CONF['drop_rate']}", f"  n_heads: {heads}", "output: ./results/"]) + "\n")
    return ModelConf(path)


def sampled(out, key, tensor, idx):
    v = tensor.detach().numpy().reshape(-1)
    out[f"{key}_val"] = v[idx].copy()
    out[f"{key}_sum"] = np.asarray([v.astype(np.float64).sum()])


def main():
    import importlib
    mod = importlib.import_module("model.sequential.SASRec")
    train, test = tiny_sequences()
    out, meta = {}, {"conf": CONF, "heads": list(HEADS), "train": train, "test": test, **SEEDS}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            for H in HEADS:
                conf = write_conf(tmp, H)
                torch.manual_seed(SEEDS["torch_seed"]); random.seed(SEEDS["sampler_seed"])
                model = mod.SASRec(conf, {k: list(v) for k, v in train.items()}, {k: list(v) for k, v in test.items()})
                d, net = model.data, model.model
                params = dict(net.named_parameters())
                if H == HEADS[0]:
                    out["seq_names"] = np.asarray([n for n, _ in d.original_seq])
                    out["seq_flat"] = np.asarray([i for _, ids in d.original_seq for i in ids], dtype=np.int32)
                    out["seq_ptr"] = np.cumsum([0] + [len(ids) for _, ids in d.original_seq]).astype(np.int32)
                    out["item_names"] = np.asarray([d.id2item[i] for i in range(1, d.item_num + 1)])
                    meta.update(raw_seq_num=d.raw_seq_num, item_num=d.item_num, seq_ids=d.seq,
                                test_set={k: dict(v) for k, v in d.test_set.items()}, param_names=list(params))
                    rs = np.random.RandomState(SEEDS["sample_seed"])
                    for name, p in params.items():
                        n = p.numel()
                        out[f"sample_{name}"] = (np.arange(n) if n <= N_SAMPLE else
                                                 np.sort(rs.choice(n, N_SAMPLE, replace=False))).astype(np.int64)
                        out[f"init_{name}"] = p.detach().numpy().copy()
                else:
                    for name, p in params.items():
                        assert np.array_equal(out[f"init_{name}"], p.detach().numpy()), name
                batches = list(ref_sampler.next_batch_sequence(d, model.batch_size, max_len=model.max_len))
                state = random.getstate()
                if H == HEADS[0]:
                    meta["n_train_batches"] = len(batches)
                    for b, (seq, pos, y, neg, ln) in enumerate(batches):
                        for k, v in zip(("seq", "pos", "y", "neg", "len"), (seq, pos, y, neg, ln)):
                            out[f"train{b}_{k}"] = np.asarray(v, dtype=np.int32)
                    out["rng_after_epoch"] = np.asarray(state[1], dtype=np.int64)
                    tests = list(ref_sampler.next_batch_sequence_for_test(d, model.batch_size, max_len=model.max_len))
                    meta["n_test_batches"] = len(tests)
                    for b, (seq, pos, ln) in enumerate(tests):
                        for k, v in zip(("seq", "pos", "len"), (seq, pos, ln)):
                            out[f"test{b}_{k}"] = np.asarray(v, dtype=np.int32)
                else:
                    assert np.array_equal(out["rng_after_epoch"], np.asarray(state[1], dtype=np.int64))
                optimizer = torch.optim.Adam(net.parameters(), lr=model.lRate)
                losses = []
                for s in range(3):
                    seq, pos, y, neg_idx, _ = batches[s]
                    net.train()
                    seq_emb = net.forward(seq, pos)
                    rec_loss = model.calculate_loss(seq_emb, y, neg_idx, pos)
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
    np.savez_compressed(os.path.join(HERE, "sasrec.npz"), **out)
    with open(os.path.join(HERE, "sasrec_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print(json.dumps({k: v for k, v in meta.items() if k not in ("train", "test", "test_set", "seq_ids")}, indent=1))


if __name__ == "__main__":
    main()
