#!/usr/bin/env python3
"""The fused XSimGCL step without the InfoNCE prep launch (the stage rider on the product that reads the contrast table,
pass 1 normalising its own queries and carrying BPR phase 1: 9 launches) against the prep launch (nce_prep_bpr1: 10
launches; what SRH_NCE_PREP=1 selects), A/B in ONE process: alternating fenced regions of the same trainer (the graph is
re-captured at every switch), so that box-to-box drift (+-3 % between bench.py runs) cancels.  Prints ms/step per region
and the paired difference."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from selfrec_amd.engine import FusedTrainer  # noqa: E402

args = bench.parse([])
data, raw = bench.build_data(args.shape, args.seed)
torch.manual_seed(args.seed)
tr = FusedTrainer(data, args.emb, model="XSimGCL", n_layers=3, lr=1e-3, reg=1e-4, cl_rate=0.2, eps=0.2, tau=0.2, layer_cl=1,
                  batch_size=2048, use_graph=True, nce_precision="f32")
assert tr.nce_stage_ok
r = bench.Runner(tr, args.seed)
r.run(50); r.fence()
N = int(os.environ.get("AB_STEPS", 600))
out = {"staged": [], "prep-launch": []}
for rep in range(int(os.environ.get("AB_REPS", 5))):
    for mode in ("staged", "prep-launch"):
        tr._prep_launch = mode == "prep-launch"
        assert tr._nce_staged() == (mode == "staged")
        tr.reset_graph()
        r.run(30); r.fence()
        dt, bounds, _ = r.timed(N, mode)
        out[mode].append(dt / N * 1e3)
        print(f"rep {rep} {mode:11s}: {dt / N * 1e3:.4f} ms/step  ({bounds} epoch boundaries inside)", flush=True)
f, s = np.array(out["staged"]), np.array(out["prep-launch"])
print(f"staged      median {np.median(f):.4f} ms/step = {2048 / np.median(f) / 1e3:.3f} M pairs/s")
print(f"prep-launch median {np.median(s):.4f} ms/step = {2048 / np.median(s) / 1e3:.3f} M pairs/s")
print(f"paired difference staged - prep-launch: mean {np.mean(f - s) * 1e3:.2f}, median {np.median(f - s) * 1e3:.2f} us per step "
      f"(min {np.min(f - s) * 1e3:.2f}, max {np.max(f - s) * 1e3:.2f}); spread of the staged regions {np.ptp(f) * 1e3:.2f} us, "
      f"of the prep-launch regions {np.ptp(s) * 1e3:.2f} us")
