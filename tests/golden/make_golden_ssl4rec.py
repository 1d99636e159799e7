#!/usr/bin/env python3
"""Reference-run golden for SSL4Rec: runs the REFERENCE'S OWN model/graph/SSL4Rec.py on the CPU, on
make_golden.tiny_graph() (200 x 300), d = 64 and the keys of the reference's conf/SSL4Rec.yaml (tau 0.07, alpha 0.1,
drop 0.1).

The steps are driven as SSL4Rec.train() drives them (SSL4Rec.py:29-40: the same expressions in the same order, one
torch.optim.Adam over model.parameters()).  model.dropout is wrapped so that both masks of every step are recorded.

Recorded (tests/golden/ssl4rec.npz + ssl4rec_meta.json):
  init_user_emb / init_item_emb     the initial tables (torch.manual_seed(41) before the model is built)
  batch{0,1,2}_q / _i               the three batches of the first epoch (random.seed(2718))
  step{s}_mask                      (2, B, 64) packed bits (np.packbits, axis -1): the keep masks of views 1 and 2
  step{s}_loss                      rec_loss, cl_loss, total (float64 of the float32 values)
  step{s}_user_emb / _item_emb      the tables after step s
  step{s}_{tensor}_val / _sum       every tower tensor after step s: the elements at sample_{tensor} (flat indices) and
                                    the float64 sum of the whole tensor
  grad0_{name}_val / _sum           the gradients of step 0 before Adam, sampled the same way (tables included)
  eval_query_emb / eval_item_emb    model(all users, all items) after step 2, no dropout
  test_users, rec_items, rec_scores test() with those embeddings (query_emb / item_emb) and the strings of
                                    ranking_evaluation (meta)

Run:  python tests/golden/make_golden_ssl4rec.py        (writes next to this file)
"""
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

from selfrec_amd import synth  # noqa: E402

CONF = dict(tau=0.07, alpha=0.1, drop=0.1)
SEEDS = dict(torch_seed=41, numpy_seed=42, sampler_seed=2718, sample_seed=43)
N_SAMPLE = 64
TOWER = ("user_tower.0.weight", "user_tower.0.bias", "user_tower.2.weight", "user_tower.2.bias",
         "item_tower.0.weight", "item_tower.0.bias", "item_tower.2.weight", "item_tower.2.bias")

from util.evaluation import ranking_evaluation  # noqa: E402
from util import sampler as ref_sampler  # noqa: E402


class RecordingDropout(torch.nn.Module):
    def __init__(self, inner, log):
        super().__init__()
        self.inner, self.log = inner, log

    def forward(self, x):
        y = self.inner(x)
        self.log.append((y != 0).numpy().copy())     # (no gathered input element is exactly zero: xavier tables)
        return y


def main():
    import importlib
    mod = importlib.import_module("model.graph.SSL4Rec")
    tu, ti, su, si = MG.tiny_graph()
    train, test = synth.as_triples(tu, ti), synth.as_triples(su, si)
    out, meta = {}, {"conf": CONF, "emb": MG.EMB, "batch": MG.BATCH, "lr": 0.001, "reg": 0.0001, **SEEDS}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            conf = MG.make_conf(tmp, "SSL4Rec", dict(CONF))
            torch.manual_seed(SEEDS["torch_seed"]); np.random.seed(SEEDS["numpy_seed"]); random.seed(SEEDS["sampler_seed"])
            model = mod.SSL4Rec(conf, [list(t) for t in train], [list(t) for t in test])
            enc = model.model
            out["init_user_emb"] = enc.initial_user_emb.detach().numpy().copy()
            out["init_item_emb"] = enc.initial_item_emb.detach().numpy().copy()
            batches = list(ref_sampler.next_batch_pairwise(model.data, model.batch_size))[:3]
            for b, (q, i, _j) in enumerate(batches):
                out[f"batch{b}_q"], out[f"batch{b}_i"] = np.asarray(q, dtype=np.int32), np.asarray(i, dtype=np.int32)
            params = dict(enc.named_parameters())
            rs = np.random.RandomState(SEEDS["sample_seed"])
            for name in TOWER:
                out[f"sample_{name}"] = np.sort(rs.choice(params[name].numel(), N_SAMPLE, replace=False)).astype(np.int64)
            for name in ("initial_user_emb", "initial_item_emb"):
                out[f"sample_{name}"] = np.sort(rs.choice(params[name].numel(), N_SAMPLE, replace=False)).astype(np.int64)
            log = []
            enc.dropout = RecordingDropout(enc.dropout, log)
            optimizer = torch.optim.Adam(enc.parameters(), lr=model.lRate)
            for s, (query_idx, item_idx, _neg) in enumerate(batches):
                enc.train()
                query_emb, item_emb = enc(query_idx, item_idx)
                rec_loss = mod.batch_softmax_loss(query_emb, item_emb, model.tau)
                cl_loss = model.cl_rate * enc.cal_cl_loss(item_idx)
                batch_loss = rec_loss + mod.l2_reg_loss(model.reg, query_emb, item_emb) + cl_loss
                optimizer.zero_grad()
                batch_loss.backward()
                if s == 0:
                    for name, p in params.items():
                        g = p.grad.detach().numpy().reshape(-1)
                        out[f"grad0_{name}_val"] = g[out[f"sample_{name}"]].copy()
                        out[f"grad0_{name}_sum"] = np.asarray([g.astype(np.float64).sum()])
                optimizer.step()
                assert len(log) == 2 * (s + 1)
                out[f"step{s}_mask"] = np.packbits(np.stack(log[-2:]).astype(np.uint8), axis=-1)
                out[f"step{s}_loss"] = np.asarray([float(rec_loss), float(cl_loss), float(batch_loss)], dtype=np.float64)
                out[f"step{s}_user_emb"] = enc.initial_user_emb.detach().numpy().copy()
                out[f"step{s}_item_emb"] = enc.initial_item_emb.detach().numpy().copy()
                for name in TOWER:
                    v = params[name].detach().numpy().reshape(-1)
                    out[f"step{s}_{name}_val"] = v[out[f"sample_{name}"]].copy()
                    out[f"step{s}_{name}_sum"] = np.asarray([v.astype(np.float64).sum()])
            enc.eval()
            with torch.no_grad():
                model.query_emb, model.item_emb = enc(list(range(model.data.user_num)), list(range(model.data.item_num)))
            out["eval_query_emb"] = model.query_emb.numpy().copy()
            out["eval_item_emb"] = model.item_emb.numpy().copy()
            rec = model.test()
            d = model.data
            users = list(d.test_set)
            out["test_users"] = np.asarray(users)
            out["rec_items"] = np.asarray([[d.item[it] for it, _ in rec[u]] for u in users], dtype=np.int32)
            out["rec_scores"] = np.asarray([[float(sc) for _, sc in rec[u]] for u in users], dtype=np.float64)
            meta["ranking_evaluation"] = ranking_evaluation(d.test_set, rec, model.topN)
        finally:
            os.chdir(cwd)
    meta.update(torch=torch.__version__, numpy=np.__version__, losses=[out[f"step{s}_loss"].tolist() for s in range(3)])
    np.savez_compressed(os.path.join(HERE, "ssl4rec.npz"), **out)
    with open(os.path.join(HERE, "ssl4rec_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print(json.dumps(meta, indent=1))


if __name__ == "__main__":
    main()
