#!/usr/bin/env python3
"""Reference-run golden for UserKNN and ItemKNN: runs the REFERENCE'S OWN model/graph/UserKNN.py and ItemKNN.py on the CPU
(numba stubbed as in make_golden.py), with the reference's conf keys (topK 50, shrinkage 100, item.ranking.topN [10,20]).

The dataset (written into knn.npz): a zipf graph of 1,200 users x 1,000 items from selfrec_amd.synth, names being the ids
under a seeded permutation written as decimal strings (so "9" > "10": name order is not id order), plus
  dup0..2     three users with the items of one user (their similarities tie with each other)
  loner       a user whose two items nobody else has (ItemKNN: each the other's only neighbour)
  hermit      a user whose single item nobody else has (an empty list on both sides, an all-zero predict() row)
  hub0, hub1  users with 300 items each
Recorded: the reference's id -> name tables; every row's neighbour list (reference ids, sims as raw f64 bits);
predict() rows of a few users; test()'s full rec_list (names as item ids, scores as f64 bits) and the strings of
ranking_evaluation (knn_meta.json).

Run:  python tests/golden/make_golden_knn.py        (writes next to this file; about a minute)
"""
import importlib
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (numba stub, the reference on sys.path)

from util.conf import ModelConf  # noqa: E402
from util.evaluation import ranking_evaluation  # noqa: E402

from selfrec_amd import synth  # noqa: E402

GRAPH = dict(n_users=1200, n_items=1000, n_edges=24000, seed=5)
CONF = dict(topK=50, shrinkage=100)
PREDICT_USERS = ["dup0", "dup1", "loner", "hermit", "hub0"]


def dataset():
    rng = np.random.default_rng(GRAPH["seed"])
    u, i = synth.generate_edges(GRAPH["n_users"], GRAPH["n_items"], GRAPH["n_edges"], GRAPH["seed"])
    (tu, ti), (su, si) = synth.split_train_test(u, i, GRAPH["n_users"], GRAPH["n_items"], 0.2, GRAPH["seed"])
    un = rng.permutation(GRAPH["n_users"]).astype(str)
    inames = rng.permutation(GRAPH["n_items"]).astype(str)
    train = [[un[a], inames[b]] for a, b in zip(tu.tolist(), ti.tolist())]
    test = [[un[a], inames[b]] for a, b in zip(su.tolist(), si.tolist())]
    src = un[int(tu[0])]
    src_items = [it for us, it in train if us == src]
    for k in range(3):
        train += [[f"dup{k}", it] for it in src_items]
        test.append([f"dup{k}", inames[int(rng.integers(GRAPH["n_items"]))]])
    train += [["loner", "x_loner_a"], ["loner", "x_loner_b"], ["hermit", "x_hermit"]]
    test += [["loner", inames[1]], ["hermit", inames[2]]]
    for h in range(2):
        picks = rng.choice(GRAPH["n_items"], 300, replace=False)
        train += [[f"hub{h}", inames[p]] for p in picks.tolist()]
        test.append([f"hub{h}", inames[int(rng.integers(GRAPH["n_items"]))]])
    seen = set()
    train = [p for p in train if not (tuple(p) in seen or seen.add(tuple(p)))]      # one rating per pair
    train_pairs = set(map(tuple, train))
    test = [p for p in test if tuple(p) not in train_pairs]
    return train, test


def conf_file(tmp, model):
    lines = ["training.set: ./train.txt", "test.set: ./test.txt", "model:", f"  name: {model}", "  type: graph",
             "item.ranking.topN: [10,20]", f"topK: {CONF['topK']}", f"shrinkage: {CONF['shrinkage']}",
             "embedding.size: 64", "max.epoch: 20", "batch.size: 2048", "learning.rate: 0.001", "reg.lambda: 0.0001",
             "output: ./results/"]
    path = os.path.join(tmp, f"{model}.yaml")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return ModelConf(path)


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def main():
    train, test = dataset()
    out = {"train_user": np.asarray([p[0] for p in train]), "train_item": np.asarray([p[1] for p in train]),
           "test_user": np.asarray([p[0] for p in test]), "test_item": np.asarray([p[1] for p in test])}
    meta = {"graph": GRAPH, "conf": CONF, "predict_users": PREDICT_USERS}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            for name, attr, side in (("UserKNN", "user_sim", "user"), ("ItemKNN", "item_sim", "item")):
                mod = importlib.import_module(f"model.graph.{name}")
                model = getattr(mod, name)(conf_file(tmp, name), [p + [1.0] for p in train], [p + [1.0] for p in test])
                d = model.data
                ids_of = d.user if side == "user" else d.item
                n = d.user_num if side == "user" else d.item_num
                model.train()
                sims = getattr(model, attr)
                lens = np.asarray([len(sims[(d.id2user if side == "user" else d.id2item)[r]]) for r in range(n)])
                ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
                flat = [e for r in range(n) for e in sims[(d.id2user if side == "user" else d.id2item)[r]]]
                out[f"{name}_nbr_ptr"] = ptr
                out[f"{name}_nbr_ids"] = np.asarray([ids_of[v] for _, v in flat], dtype=np.int32)
                out[f"{name}_nbr_sims"] = bits([s for s, _ in flat])
                out[f"{name}_predict"] = bits(np.stack([model.predict(u) for u in PREDICT_USERS]))
                rec = model.test()
                users = list(d.test_set)
                out[f"{name}_rec_items"] = np.asarray([[d.item[it] for it, _ in rec[u]] for u in users], dtype=np.int32)
                out[f"{name}_rec_scores"] = bits([[float(s) for _, s in rec[u]] for u in users])
                meta[name] = {"ranking_evaluation": ranking_evaluation(d.test_set, rec, model.topN),
                              "n_rows": n, "empty_lists": int((lens == 0).sum()), "short_lists": int((lens < CONF["topK"]).sum())}
                if name == "UserKNN":
                    out["user_names"] = np.asarray([d.id2user[k] for k in range(d.user_num)])
                    out["item_names"] = np.asarray([d.id2item[k] for k in range(d.item_num)])
                    out["test_users"] = np.asarray(users)
                    # the lines evaluate() writes for the first users (graph_recommender.py:63-68)
                    meta["rec_lines"] = [u + ':' + ''.join(f" ({it},{s}){'*' if it in d.test_set[u] else ''}"
                                                           for it, s in rec[u]) + '\n' for u in users[:5]]
        finally:
            os.chdir(cwd)
    meta["numpy"] = np.__version__
    np.savez_compressed(os.path.join(HERE, "knn.npz"), **out)
    with open(os.path.join(HERE, "knn_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print(json.dumps({k: v for k, v in meta.items() if k != "rec_lines"}, indent=1))


if __name__ == "__main__":
    main()
