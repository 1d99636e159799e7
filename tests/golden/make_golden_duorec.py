#!/usr/bin/env python3
"""Reference-composed golden for DuoRec.  The reference ships conf/DuoRec.yaml and util/loss_torch.info_nce but no model
file, so this script composes the REFERENCE'S OWN pieces, imported at generation time on the CPU (make_golden.py's .cuda()
shims) -- model/sequential/SASRec.py's SASRec_Model and BCE expression (calculate_loss), util/sampler.next_batch_sequence,
util/loss_torch.l2_reg_loss and info_nce -- into the step DESIGN.md 4.29 specifies:

    view 0 the batch, view 1 the same ids again, view 2 a sequence with the same target; h_a, h_p, h_q the hidden rows at
    each view's last live position;  loss = rec + l2_reg_loss(reg, item_emb) + cl_rate (info_nce(h_a, h_p, 1, B, 'dot') +
    info_nce(h_a, h_q, 1, B, 'dot'))

on make_golden_sasrec.tiny_sequences(), d = 64, max.len = 12, 2 blocks, batch.size = 32, drop_rate = 0, cl_rate = 0.1, with
1 and 2 heads.  The positive of a batch row is ``random.choice`` among the OTHER sequences whose last training item is the
row's, in file order; a row whose target no other sequence has keeps its own sequence and draws nothing.  The draws follow
the yield of their batch on the sampler's ``random`` stream, as CL4SRec's augmentor draws do.  The data hold a target shared
by >= 3 sequences, a target with a single sequence and a candidate longer than max.len (asserted, counted in the meta).

Recorded (tests/golden/duorec.npz + duorec_meta.json), run key k = h{heads}:
  sample_{param}, init_{param}_val / _sum        as make_golden_cl4srec.py
  train{b}_{seq,pos,y,neg,len,rows}              every batch of the first epoch (random.seed(2718)); rows: the index into
                                                 original_seq of every batch row
  pos{b}_{seq,pos,len,chosen}                    the positives of batch b and the indices chosen
  rng_after_epoch                                python's generator state after the epoch
  {k}_loss / _rec_loss / _cl_loss                the 3 steps' losses (float64 of the float32 values)
  {k}_grad0_{param}_val / _sum                   step 0's gradients, sampled
  {k}_step{s}_{param}_val / _sum                 parameters after steps 0 and 2, sampled
  h1_final_{param}                               parameters after step 2, whole
  h1_rec_ids / _rec_scores                       test() on h1's final parameters;  meta h1_evaluation: both strings

Run:  python tests/golden/make_golden_duorec.py        (writes next to this file)
"""
import contextlib
import io
import json
import os
import random
import sys
import tempfile
from collections import defaultdict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402,F401  (numba stub, .cuda() shims, the reference on sys.path)
import make_golden_sasrec as MS  # noqa: E402

import torch  # noqa: E402

from util.conf import ModelConf  # noqa: E402
from util.evaluation import ranking_evaluation  # noqa: E402
from util.loss_torch import info_nce, l2_reg_loss  # noqa: E402
from util import sampler as ref_sampler  # noqa: E402

SEEDS = dict(torch_seed=41, sampler_seed=2718, data_seed=7, sample_seed=43)
CONF = dict(emb=64, max_len=12, n_blocks=2, batch=32, drop_rate=0.0, lr=0.001, reg=0.0001, topN=[10, 20], cl_rate=0.1,
            tau=1.0, sim="dot")
HEADS = (1, 2)
N_SAMPLE = 512
N_STEPS = 3


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


def draw_positives(data, index, rows, max_len):
    seq, pos = (np.zeros((len(rows), max_len), dtype=int) for _ in range(2))
    lens, chosen, draws = [], [], 0
    for n, row in enumerate(rows):
        cands = [j for j in index[data.original_seq[row][1][-1]] if j != row]
        pick = row
        if cands:
            pick = random.choice(cands)
            draws += 1
        ids = data.original_seq[pick][1]
        start, end = (-max_len, max_len - 1) if len(ids) > max_len else (0, len(ids) - 1)
        seq[n, :end] = ids[start:-1]
        pos[n, :end] = np.arange(1, end + 1)
        lens.append(end)
        chosen.append(pick)
    return seq, pos, np.asarray(lens), np.asarray(chosen), draws


def last_rows(emb, lens):
    return torch.cat([emb[i, last - 1, :].view(1, -1) for i, last in enumerate(lens)], 0)


def main():
    import importlib
    mod = importlib.import_module("model.sequential.SASRec")
    train, test = MS.tiny_sequences()
    out, meta = {}, {"conf": CONF, "heads": list(HEADS), "train": train, "test": test, **SEEDS}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            for H in HEADS:
                k = f"h{H}"
                conf = write_conf(tmp, H)
                torch.manual_seed(SEEDS["torch_seed"]); random.seed(SEEDS["sampler_seed"])
                model = mod.SASRec(conf, {n: list(v) for n, v in train.items()}, {n: list(v) for n, v in test.items()})
                d, net = model.data, model.model
                L = model.max_len
                params = dict(net.named_parameters())
                index = defaultdict(list)
                for n, (_, ids) in enumerate(d.original_seq):
                    index[ids[-1]].append(n)
                first = H == HEADS[0]
                if first:
                    shared = sorted(t for t, v in index.items() if len(v) >= 3)
                    single = sorted(t for t, v in index.items() if len(v) == 1)
                    long_cands = sorted(j for v in index.values() if len(v) >= 2 for j in v if len(d.original_seq[j][1]) > L)
                    assert shared and single and long_cands
                    meta.update(raw_seq_num=d.raw_seq_num, item_num=d.item_num, param_names=list(params),
                                targets_shared_by_3=len(shared), targets_single=len(single),
                                long_candidates=[int(j) for j in long_cands],
                                same_target={str(t): [int(j) for j in v] for t, v in index.items()})
                    rs = np.random.RandomState(SEEDS["sample_seed"])
                    for name, p in params.items():
                        n = p.numel()
                        out[f"sample_{name}"] = (np.arange(n) if n <= N_SAMPLE else
                                                 np.sort(rs.choice(n, N_SAMPLE, replace=False))).astype(np.int64)
                        MS.sampled(out, f"init_{name}", p, out[f"sample_{name}"])
                optimizer = torch.optim.Adam(net.parameters(), lr=model.lRate)
                losses, rec_losses, cl_losses = [], [], []
                # the reference shuffles the id lists; the same shuffle of an index list names every batch row
                state = random.getstate()
                order = list(range(len(d.original_seq)))
                random.shuffle(order)
                random.setstate(state)
                n_batches = fallbacks = 0
                net.train()
                for b, batch in enumerate(ref_sampler.next_batch_sequence(d, model.batch_size, max_len=L)):
                    seq, pos, y, neg_idx, seq_len = batch
                    rows = order[b * model.batch_size:b * model.batch_size + len(seq)]
                    for n, row in enumerate(rows):
                        ids = d.original_seq[row][1]
                        assert list(seq[n, :seq_len[n]]) == ids[(-L if len(ids) > L else 0):-1]
                    p_seq, p_pos, p_len, chosen, draws = draw_positives(d, index, rows, L)
                    fallbacks += len(rows) - draws
                    n_batches += 1
                    rec = {f"train{b}_{n}": np.asarray(v, dtype=np.int32)
                           for n, v in zip(("seq", "pos", "y", "neg", "len", "rows"), batch + (rows,))}
                    rec.update({f"pos{b}_{n}": np.asarray(v, dtype=np.int32)
                                for n, v in zip(("seq", "pos", "len", "chosen"), (p_seq, p_pos, p_len, chosen))})
                    for key, val in rec.items():
                        if first:
                            out[key] = val
                        else:
                            assert np.array_equal(out[key], val), key
                    if b >= N_STEPS:
                        continue
                    B = len(seq)
                    seq_emb = net.forward(seq, pos)
                    h_a = last_rows(seq_emb, seq_len)
                    h_p = last_rows(net.forward(seq, pos), seq_len)
                    h_q = last_rows(net.forward(p_seq, p_pos), p_len)
                    cl_loss = CONF["cl_rate"] * (info_nce(h_a, h_p, CONF["tau"], B, CONF["sim"])
                                                 + info_nce(h_a, h_q, CONF["tau"], B, CONF["sim"]))
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
                        if b == N_STEPS - 1 and H == 1:
                            out[f"{k}_final_{name}"] = p.detach().numpy().copy()
                state = np.asarray(random.getstate()[1], dtype=np.int64)
                if first:
                    assert fallbacks > 0
                    meta.update(n_train_batches=n_batches, fallback_rows=fallbacks)
                    out["rng_after_epoch"] = state
                else:
                    assert np.array_equal(out["rng_after_epoch"], state)
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
    np.savez_compressed(os.path.join(HERE, "duorec.npz"), **out)
    with open(os.path.join(HERE, "duorec_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print(json.dumps({k: v for k, v in meta.items() if k not in ("train", "test", "same_target")}, indent=1))


if __name__ == "__main__":
    main()
