"""The kernel cases of MixGCF's hop-mixing tests -- TEST INFRASTRUCTURE ONLY.  tests/test_gpu_mixgcf.py and
tests/test_gpu_mixgcf_edges.py run the kernels on them; tests/test_mixgcf_ref_cpu.py holds the restatement to torch and
measures what plain float32 arithmetic loses on each (the yardstick).  Every case and its float64 restatement is computed
once (lru_cache) and never modified.  A case is (family, B, H, C, d, I); its seeds are a function of the case alone.

The edges of csrc/mixgcf.hip as built, and the shapes on either side of each:

* lane-group width G = the power of two >= d / 4 (a lane holds one float4): d = 4 -> 1, 8 -> 2, 60 -> 16 with one dead lane,
  64 -> 16, 100 -> 32 with seven dead lanes, 128 -> 32, 256 -> 64 (one row per wave, no group merge).
* candidates per wave iteration 64 / G and kInFlight = 4 iterations loaded before the first use, so a batch of
  256 / G candidates: at d = 64 four per iteration (C = 3 / 4 / 5) and 16 per batch (15 / 16 / 17, 63 / 64 / 65); at d = 256
  one and four (C = 3 / 5); at d = 8 32 and 128 (C = 63 / 64 / 65 / 130); at d = 4 64 and 256 (C = 257); C = 1 and 2 leave
  lane groups without any candidate for the merge.
* one pair per workgroup (every B > 1 is more than one), one wave per hop (H = 1, 2, 4, 8 = SRH_MIXUP_MAX_HOPS).
* backward: four entry waves per workgroup over 2 B H entries (B = 1, 2, 3 with H = 1: a part, one, one and a half
  workgroups); the leader test votes every 256 earlier entries of a hop's 2 B (B = 63 / 64 / 65: around 128; B = 128 / 129:
  256 / 258; B = 257: 514) and the walk over the later ones strides by 64.  There is no sort, hence no sort block."""
import functools

import numpy as np

from tests import mixgcf_ref as ref
from tests.mhcn_cases import FWD_BOUND, GRAD_BOUND, seed_of   # the project's standing bounds: 1e-5 forward, 1e-4 gradients

NEAR_TIE_CAP = 0.01            # share of (pair, hop) rows of a `normal` case whose top-two gap may be within the margin

FAMILIES = ("normal", "zero_user", "all_negative", "alpha0", "alpha1m", "dup", "pos_is_neg", "collide", "near_tie")

S1, S2 = (5, 4, 5, 64, 300), (65, 2, 64, 64, 50)

NORMAL = [(1, 1, 1, 4, 3), (2, 2, 2, 8, 50), (3, 4, 3, 60, 50), (5, 4, 4, 64, 300), (63, 4, 5, 64, 300),
          (64, 4, 63, 64, 300), (65, 4, 64, 64, 300), (257, 4, 65, 64, 300), (5, 8, 130, 64, 300), (65, 2, 5, 128, 50),
          (3, 4, 64, 100, 300), (5, 4, 4, 256, 300), (3, 2, 5, 256, 50), (2, 1, 3, 256, 50), (65, 4, 64, 8, 300),
          (3, 1, 130, 8, 50), (2, 2, 257, 4, 50), (5, 4, 15, 64, 300), (5, 4, 16, 64, 300), (5, 4, 17, 64, 300),
          (128, 1, 2, 64, 300), (129, 2, 3, 64, 50), (3, 1, 1, 64, 50), (63, 8, 65, 128, 300), (67, 4, 64, 256, 300)]

CASES = [("normal",) + s for s in NORMAL] + \
    [("zero_user",) + s for s in (S1, S2)] + \
    [("all_negative",) + s for s in (S1, S2, (3, 1, 130, 8, 50))] + \
    [(f,) + s for f in ("alpha0", "alpha1m") for s in (S1, S2)] + \
    [("dup",) + s for s in (S1, S2, (2, 4, 65, 256, 50))] + \
    [("pos_is_neg",) + s for s in ((5, 4, 1, 64, 300), S1, S2)] + \
    [("collide",) + s for s in ((63, 4, 5, 64, 3), (257, 2, 64, 64, 3), (5, 8, 3, 8, 3))] + \
    [("near_tie",) + s for s in (S1, S2, (3, 2, 2, 256, 50))]


def case_id(c):
    return "%s-B%d_H%d_C%d_d%d_I%d" % c


def seeds(case):
    """(numpy seed, kernel rng seed, kernel rng counter) of a case.  The rng seed has bits in both 32-bit words and the
    counter block of every case crosses 2^32, so both halves of the key take part."""
    fam, *shape = case
    s = seed_of(FAMILIES.index(fam), *shape)
    return s, (s << 33) | (s ^ 0x5DEECE66D), (1 << 32) - 1 - (s % 97)


@functools.lru_cache(maxsize=None)
def inputs(case):
    """normal        tables, user rows at scale 0.1; alpha what the kernel draws at the case's (seed, counter)
    zero_user     u = 0: every score is +0, the pick 0 at every hop
    all_negative  positive tables, negative user rows: every score < 0 (a maximum that starts at 0 picks nothing)
    alpha0        alpha = 0: the mixture is the candidate's own row;  alpha1m: alpha = 1 - 2^-24, the largest float32 < 1
    dup           one item is all C candidates of a pair and alpha is one constant per hop: exact ties, the pick 0
    pos_is_neg    candidate b % C of pair b is its positive (C = 1: the only one); the positives are distinct items
                  where B <= I
    collide       I = 3: every gradient row sums many contributions
    near_tie      candidates 0 and C - 1 of a pair are one large positive row with alpha equal but for one element that
                  differs by 2^-24: they lead all others and their float64 gap is far below the margin"""
    fam, B, H, C, d, n_items = case
    np_seed, rng_seed, rng_ctr = seeds(case)
    rng = np.random.default_rng(np_seed)
    tables = (0.1 * rng.standard_normal((H, n_items, d))).astype(np.float32)
    u = (0.1 * rng.standard_normal((B, d))).astype(np.float32)
    pos = rng.integers(0, n_items, B)
    neg = rng.integers(0, n_items, (B, C))
    alpha = ref.drawn_alpha(rng_seed, rng_ctr, H, B, C, d)
    drawn = True
    if fam == "zero_user":
        u[:] = 0.0
    elif fam == "all_negative":
        tables, u = np.abs(tables) + np.float32(0.01), -np.abs(u) - np.float32(0.01)
    elif fam in ("alpha0", "alpha1m"):
        alpha = np.full((H, B, C, d), 0.0 if fam == "alpha0" else 1.0 - 2.0 ** -24, dtype=np.float32)
        drawn = False
    elif fam == "dup":
        neg = np.repeat(rng.integers(0, n_items, (B, 1)), C, axis=1)
        alpha = np.broadcast_to(rng.random((H, 1, 1, 1)).astype(np.float32), (H, B, C, d)).copy()
        drawn = False
    elif fam == "pos_is_neg":
        pos = rng.permutation(n_items)[:B] if B <= n_items else pos
        neg[np.arange(B), np.arange(B) % C] = pos
    elif fam == "near_tie":
        u = np.abs(u) + np.float32(0.01)
        big = 2 * rng.integers(0, n_items // 2, B)      # even rows are large, every positive is an odd (ordinary) row
        tables[:, big] = (1.0 + np.abs(tables[:, big])).astype(np.float32)
        pos = big + 1
        neg = neg | 1
        neg[:, 0] = big
        neg[:, C - 1] = big
        alpha = alpha.copy()
        alpha[:, :, C - 1] = alpha[:, :, 0]
        a0 = alpha[:, :, 0, d // 2]
        a0 = np.where(a0 < 0.5, a0 + np.float32(0.25), a0)                 # (a spacing of exactly 2^-24 below: [0.5, 1))
        alpha[:, :, 0, d // 2] = a0
        alpha[:, :, C - 1, d // 2] = np.where(a0 >= 0.5, a0 - np.float32(2.0 ** -24), a0)
        drawn = False
    elif fam not in ("normal", "collide"):
        raise ValueError(fam)
    g_pos = rng.standard_normal((B, d)).astype(np.float32)
    g_neg = rng.standard_normal((B, d)).astype(np.float32)
    return dict(tables=tables, u=u, pos=pos.astype(np.int64), neg=neg.reshape(-1).astype(np.int64), alpha=alpha,
                g_pos=g_pos, g_neg=g_neg, drawn=drawn, rng_seed=rng_seed, rng_counter=rng_ctr)


@functools.lru_cache(maxsize=None)
def reference(case):
    """the float64 scores, their argmax, the margin of a float32 dot product and the top-two gap, per (hop, pair)"""
    c = inputs(case)
    s = ref.scores(c["tables"], c["u"], c["pos"], c["neg"], c["alpha"])
    top = np.sort(s, axis=2)
    gap = top[:, :, -1] - top[:, :, -2] if s.shape[2] > 1 else np.full(s.shape[:2], np.inf)
    return dict(s=s, amax=ref.argmax(s), margin=ref.margin(c["tables"], c["u"], c["pos"], c["neg"], c["alpha"]), gap=gap)


def judge_pick(case, pick):
    """-> (rows whose picked candidate scores more than the margin below the float64 maximum, rows with a clear float64
    winner -- top-two gap above the margin -- where the pick is not that winner); both must be 0"""
    r = reference(case)
    pick = np.asarray(pick).astype(np.int64)
    H, B, C = r["s"].shape
    assert pick.shape == (H, B) and pick.min() >= 0 and pick.max() < C
    got = np.take_along_axis(r["s"], pick[:, :, None], axis=2)[:, :, 0]
    outside = int(((r["s"].max(axis=2) - got) > r["margin"]).sum())
    clear = r["gap"] > r["margin"]
    wrong = int((clear & (pick != r["amax"])).sum())
    return outside, wrong


def rel_err(got, want):
    """the largest error over the largest magnitude of the compared tensor (a zero tensor admits no error)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.size == 0:
        return 0.0
    err, scale = float(np.abs(got - want).max()), float(np.abs(want).max())
    return err / scale if scale > 0 else (0.0 if err == 0 else np.inf)
