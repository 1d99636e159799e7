#!/usr/bin/env python3
"""Reference-run golden for MHCN's motif matrices: runs the REFERENCE'S OWN model/graph/MHCN.py ``build_hyper_adj_mats``
(on its data/social.py ``Relation`` and data/ui_graph.py ``Interaction``) on two datasets.

TensorFlow is not installed and the TF1 graph of MHCN.py cannot run, so an empty stub ``tensorflow`` module is put in
sys.modules before the import (as make_golden_sept.py does): the constructor and build_hyper_adj_mats touch only numpy /
scipy.  The training step itself is pinned by tests/mhcn_ref.py instead.

Cases (tests/golden/mhcn.npz + mhcn_meta.json):
  douban   the training split of tests/golden/douban_book.npz with the trust pairs of tests/golden/sept.npz.  That trust
           list is symmetric: U = S - S (.) S^T is empty and every motif term that holds U vanishes.
  tiny     synth.make_dataset("tiny") with synth.make_social("tiny"), handed to the reference's constructor as lists: U is
           not empty and all ten motif matrices hold entries.
Recorded per case and matrix (hs / hj / hp): indptr / indices (int32) and data (fp32) in canonical CSR form (sorted
indices, duplicates summed, explicit zeros removed).

Run:  python tests/golden/make_golden_mhcn.py        (writes next to this file)
"""
import json
import os
import sys
import tempfile
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402  (numba stub, .cuda() shims, the reference on sys.path)

sys.modules["tensorflow"] = types.ModuleType("tensorflow")

from selfrec_amd import synth  # noqa: E402


def canonical(mat):
    m = mat.tocsr().astype(np.float32).copy()
    m.sum_duplicates()
    m.eliminate_zeros()
    m.sort_indices()
    return m


def douban():
    z = np.load(os.path.join(HERE, "douban_book.npz"))
    tr, te = ~z["is_test"], z["is_test"]
    trust = np.load(os.path.join(HERE, "sept.npz"))["trust"]
    social = [[a, b, 1] for a, b in zip(trust[:, 0].astype(str).tolist(), trust[:, 1].astype(str).tolist())]
    return synth.as_triples(z["user"][tr], z["item"][tr]), synth.as_triples(z["user"][te], z["item"][te]), social


def tiny():
    tu, ti, su, si, _, _ = synth.make_dataset("tiny")
    return synth.as_triples(tu, ti), synth.as_triples(su, si), synth.make_social("tiny")


def main():
    import importlib
    mod = importlib.import_module("model.graph.MHCN")
    out, meta = {}, {}
    cwd = os.getcwd()
    for case, make in (("douban", douban), ("tiny", tiny)):
        train, test, social = make()
        with tempfile.TemporaryDirectory() as tmp:
            os.chdir(tmp)
            try:
                conf = MG.make_conf(tmp, "MHCN", dict(n_layer=2, ss_rate=0.01))
                model = mod.MHCN(conf, train, test, **{"social.data": social})
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")            # the reference's 1 / 0 on empty rows
                    with np.errstate(divide="ignore"):
                        mats = model.build_hyper_adj_mats()
                S = model.social_data.get_social_mat()
                U = S - S.multiply(S.T)
                U.eliminate_zeros()
                info = {"users": int(model.data.user_num), "items": int(model.data.item_num),
                        "size": [int(x) for x in model.social_data.size()], "one_way_pairs": int(U.nnz)}
                for name, m in zip(("hs", "hj", "hp"), mats):
                    c = canonical(m)
                    assert np.isfinite(c.data).all()
                    out[f"{case}_{name}_indptr"] = c.indptr.astype(np.int32)
                    out[f"{case}_{name}_indices"] = c.indices.astype(np.int32)
                    out[f"{case}_{name}_data"] = c.data.astype(np.float32)
                    info[name] = {"nnz": int(c.nnz), "empty_rows": int((np.diff(c.indptr) == 0).sum()), "dtype": str(m.dtype)}
                meta[case] = info
            finally:
                os.chdir(cwd)
    import scipy
    meta.update(numpy=np.__version__, scipy=scipy.__version__)
    np.savez_compressed(os.path.join(HERE, "mhcn.npz"), **out)
    with open(os.path.join(HERE, "mhcn_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print(json.dumps(meta, indent=1))


if __name__ == "__main__":
    main()
