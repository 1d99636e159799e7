#!/usr/bin/env python3
"""Reference-run golden for SEPT's social data path: runs the REFERENCE'S OWN data/social.py ``Relation`` and
model/graph/SEPT.py ``get_social_related_views`` on the training split of tests/golden/douban_book.npz and the
reference's dataset/douban-book/trust.txt.

TensorFlow is not installed and the TF1 graph of SEPT.py cannot run, so an empty stub ``tensorflow`` module is put in
sys.modules before the import (as make_golden_ncl.py stubs faiss): the constructor and get_social_related_views touch
only numpy / scipy.  The training step itself is pinned by tests/sept_ref.py instead.

Recorded (tests/golden/sept.npz + sept_mats.npz + sept_meta.json; two archives because a committed file stays under 1 MiB:
sept.npz holds trust, size and sharing_*, sept_mats.npz holds social_*, bi_* and friend_*):
  trust             the raw trust pairs (lines x 2, int32, file order): a data fixture, the test's input
  size              Relation.size(): (users with a follower, pairs kept by the user filter)
  social_*, bi_*, friend_*, sharing_*   indptr / indices / data (fp32) of get_social_mat(), get_birectional_social_mat()
                    and the two views of get_social_related_views(), in canonical CSR form (sorted indices)

Run:  python tests/golden/make_golden_sept.py        (writes next to this file)
"""
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402  (numba stub, .cuda() shims, the reference on sys.path)

sys.modules["tensorflow"] = types.ModuleType("tensorflow")

from data.loader import FileIO  # noqa: E402


def canonical(mat):
    m = mat.tocsr().astype(np.float32).copy()
    m.sum_duplicates()
    m.sort_indices()
    return m


def main():
    import importlib
    mod = importlib.import_module("model.graph.SEPT")
    z = np.load(os.path.join(HERE, "douban_book.npz"))
    sel = ~z["is_test"]
    train = [[str(u), str(i), float(r)] for u, i, r in zip(z["user"][sel].tolist(), z["item"][sel].tolist(), z["rating"][sel].tolist())]
    sel = z["is_test"]
    test = [[str(u), str(i), float(r)] for u, i, r in zip(z["user"][sel].tolist(), z["item"][sel].tolist(), z["rating"][sel].tolist())]
    social = FileIO.load_social_data(os.path.join(MG.REF, "dataset", "douban-book", "trust.txt"))
    out = {"trust": np.asarray([[int(a), int(b)] for a, b, _ in social], dtype=np.int32)}
    assert all(w == 1 for _, _, w in social)
    meta = {"trust_lines": len(social)}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            conf = MG.make_conf(tmp, "SEPT", dict(n_layer=2, ss_rate=0.005, drop_rate=0.3, ins_cnt=10))
            model = mod.SEPT(conf, train, test, **{"social.data": social})
            rel = model.social_data
            out["size"] = np.asarray(rel.size(), dtype=np.int64)
            mats = {"social": rel.get_social_mat(), "bi": rel.get_birectional_social_mat()}
            mats["friend"], mats["sharing"] = model.get_social_related_views(mats["bi"], model.data.interaction_mat)
            for name, m in mats.items():
                c = canonical(m)
                out[f"{name}_indptr"], out[f"{name}_indices"] = c.indptr.astype(np.int32), c.indices.astype(np.int32)
                out[f"{name}_data"] = c.data.astype(np.float32)
                meta[name] = {"nnz": int(c.nnz), "longest_row": int(np.diff(c.indptr).max()), "dtype": str(m.dtype)}
            meta.update(users=int(model.data.user_num), items=int(model.data.item_num), size=[int(x) for x in rel.size()])
        finally:
            os.chdir(cwd)
    import scipy
    meta.update(numpy=np.__version__, scipy=scipy.__version__)
    big = {k: out.pop(k) for k in list(out) if k.split("_")[0] in ("social", "bi", "friend")}
    np.savez_compressed(os.path.join(HERE, "sept.npz"), **out)
    np.savez_compressed(os.path.join(HERE, "sept_mats.npz"), **big)
    with open(os.path.join(HERE, "sept_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print(json.dumps(meta, indent=1))


if __name__ == "__main__":
    main()
