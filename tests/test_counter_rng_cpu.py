"""The in-kernel perturbation noise as numbers (tests/counter_rng.py restates csrc/spmm.hip's counter RNG; the GPU tests
hold the kernels to that restatement number for number): its moments, its decorrelation along every axis the engine lays
counters out on, what XSimGCL consumes of it (F.normalize of a row), the distinctness of row keys, and the counter map
of every layout.  Fixed seeds and counters: every assertion is deterministic.  No GPU."""
import numpy as np
import pytest
import torch
from scipy import stats

from selfrec_amd import layouts

from .counter_rng import GOLDEN, counter_noise, engine_counter0, lowbias32, rng4, rng_key

SEED = 0x5E1F0EC                  # FusedTrainer's default rng_seed
P_HEADLINE = 69_716               # Yelp2018 shape: 31,668 users + 38,048 items (bench.py's headline run)
P_1M = 1_500_000                  # the 1 M x 500 k shape
RNG_CALLS = 16                    # FusedTrainer._rng_calls at L <= 8
L_HEADLINE = 3


def _stride(P):
    return P * RNG_CALLS


def _draws(P, step, call, d=64, seed=SEED):
    return counter_noise(seed, step * _stride(P) + call * P, P, d)


def _corr_bound(a, b):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    r = np.corrcoef(a, b)[0, 1]
    return abs(r), 5.0 / np.sqrt(a.size)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement itself
# ---------------------------------------------------------------------------------------------------------------------
def test_restatement_matches_the_written_out_mixer():
    """A few words computed step by step from the contract (include/selfrec_hip.h, csrc/spmm.hip), in python ints."""
    def lb(x):
        x ^= x >> 16; x = (x * 0x7FEB352D) & 0xFFFFFFFF; x ^= x >> 15; x = (x * 0x846CA68B) & 0xFFFFFFFF; x ^= x >> 16
        return x
    for seed, ctr, sub in [(SEED, 0, 0), (SEED, 5, 3), (0xDEADBEEF12345678, (1 << 32) + 7, 15), (1, (1 << 62) - 1, 63)]:
        key = (lb((ctr & 0xFFFFFFFF) ^ (seed & 0xFFFFFFFF)) + lb((ctr >> 32) ^ (seed >> 32))) & 0xFFFFFFFF
        base = (key + sub * 0x9E3779B1) & 0xFFFFFFFF
        want = [lb((base + a) & 0xFFFFFFFF) for a in (0, 0x85EBCA6B, 0xC2B2AE35, 0x27D4EB2F)]
        assert rng4(np.array([ctr], dtype=np.uint64), np.array([sub]), seed)[0].tolist() == want
        row = counter_noise(seed, ctr, 1, 4 * (sub + 1))[0]
        assert np.array_equal(row[4 * sub:], np.array([(w >> 8) * 2.0 ** -24 for w in want], dtype=np.float32))
    assert int(lowbias32(np.array([0], dtype=np.uint32))[0]) == 0 and int(GOLDEN) == 0x9E3779B1
    z = counter_noise(SEED, 3, 5, 64, d_valid=50)
    assert not z[:, 50:].any() and np.array_equal(z[:, :50], counter_noise(SEED, 3, 5, 64)[:, :50])


# ---------------------------------------------------------------------------------------------------------------------
# moments
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def headline_draws():
    """2.7e7 draws laid out as the headline step lays them out: P rows x 64 columns, calls 0..2, steps 1 and 2."""
    return np.concatenate([_draws(P_HEADLINE, s, c).ravel() for s in (1, 2) for c in range(L_HEADLINE)])


def test_uniform_moments_range_and_lattice(headline_draws):
    z = headline_draws
    n = z.size
    assert n >= 10_000_000
    assert z.min() >= 0.0 and z.max() <= 1.0 - 2.0 ** -24
    k = z.astype(np.float64) * 2.0 ** 24
    assert np.array_equal(k, np.floor(k))                                   # multiples of 2^-24
    mean, var = z.astype(np.float64).mean(), z.astype(np.float64).var()
    assert abs(mean - 0.5) < 5 * np.sqrt(1 / 12 / n), mean                  # sigma of the mean: sqrt(1/12 / n)
    assert abs(var - 1 / 12) < 5 * np.sqrt(1 / 180 / n), var               # Var[(u - 1/2)^2] = 1/80 - 1/144 = 1/180


def test_chi_square_over_256_bins(headline_draws):
    counts = np.bincount((headline_draws * 256).astype(np.int64), minlength=256)
    assert counts.size == 256
    chi2, p = stats.chisquare(counts)
    assert p > 1e-6, (chi2, p)


def test_the_24_used_bits_are_balanced(headline_draws):
    k = (headline_draws.astype(np.float64) * 2.0 ** 24).astype(np.uint32)
    n = k.size
    for b in range(24):
        ones = np.count_nonzero((k >> np.uint32(b)) & np.uint32(1))
        assert abs(ones / n - 0.5) < 5 * 0.5 / np.sqrt(n), (b, ones / n)


# ---------------------------------------------------------------------------------------------------------------------
# decorrelation: every axis the engine lays counters out on
# ---------------------------------------------------------------------------------------------------------------------
def test_decorrelation_of_rows_columns_steps_and_calls():
    P = P_HEADLINE
    a = _draws(P, 5, 0)
    pairs = {
        "adjacent rows": (a[:-1], a[1:]),
        # columns 4q + j and 4q + j + 1 inside a float4 (one counter_rng4 call), and across its boundary (sub q vs q + 1)
        "inside a float4": (a.reshape(P, 16, 4)[:, :, :3], a.reshape(P, 16, 4)[:, :, 1:]),
        "across a float4": (a.reshape(P, 16, 4)[:, :-1, 3], a.reshape(P, 16, 4)[:, 1:, 0]),
        "consecutive steps (ctr + stride)": (a, _draws(P, 6, 0)),
        "consecutive calls (ctr + P)": (a, _draws(P, 5, 1)),
        # SimGCL: view a perturbs with calls 0..L-1, view b with L..2L-1 (engine._simgcl_forward)
        "SimGCL view a / view b": (a, _draws(P, 5, L_HEADLINE)),
    }
    for what, (x, y) in pairs.items():
        r, bound = _corr_bound(x, y)
        assert r < bound, (what, r, bound)


def test_decorrelation_of_data_parallel_ranks():
    """Every data-parallel rank perturbs with its own seed (layouts.GradientAllReduce.rng_seed) at the same counters."""
    class Comm:
        def __init__(self, rank):
            self.world, self.rank = 4, rank
    seeds = {r: layouts.GradientAllReduce(Comm(r)).rng_seed(SEED) for r in (0, 1, 3)}
    assert seeds[0] == SEED and len(set(seeds.values())) == 3
    z = {r: _draws(P_HEADLINE, 2, 1, seed=s) for r, s in seeds.items()}
    for a, b in ((0, 1), (0, 3), (1, 3)):
        r, bound = _corr_bound(z[a], z[b])
        assert r < bound, (a, b, r, bound)


def test_decorrelation_across_a_2_to_the_32_counter_boundary():
    n = 200_000
    below = counter_noise(SEED, (1 << 32) - n, n, 64)          # high word 0
    above = counter_noise(SEED, 1 << 32, n, 64)                # high word 1
    same_low = counter_noise(SEED, 0, n, 64)                   # the low words of `above` with high word 0
    for what, (x, y) in {"adjacent across 2^32": (below[-1:0:-1][: n - 1], above[: n - 1]),
                         "same low word, high word 0 vs 1": (same_low, above)}.items():
        r, bound = _corr_bound(x, y)
        assert r < bound, (what, r, bound)


# ---------------------------------------------------------------------------------------------------------------------
# what XSimGCL consumes: F.normalize of a row of d uniforms
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [50, 64, 128])
def test_normalised_rows_have_the_moments_of_normalised_uniform_rows(d):
    """XSimGCL adds eps * normalize(noise row) (XSimGCL.py:90-91): per component, the mean and variance of the restated
    rows (d_valid = 50 of 64 for the padded case) match a torch.rand float64 sample of the same size within 5 sigma."""
    n = 150_000
    d_full = 64 if d == 50 else d
    z = counter_noise(SEED, 7 * _stride(P_HEADLINE), n, d_full, d_valid=d)[:, :d].astype(np.float64)
    got = z / np.linalg.norm(z, axis=1, keepdims=True)
    ref = torch.nn.functional.normalize(torch.rand((n, d), generator=torch.Generator().manual_seed(d),
                                                   dtype=torch.float64), dim=1).numpy()
    for what, f in (("mean", lambda t: t), ("variance", lambda t: (t - t.mean(0)) ** 2)):
        a, b = f(got), f(ref)
        se = np.sqrt(a.var(0) / n + b.var(0) / n)
        dev = np.abs(a.mean(0) - b.mean(0)) / se
        assert dev.max() < 5.0, (what, d, float(dev.max()))
    assert np.allclose(np.linalg.norm(got, axis=1), 1.0)


# ---------------------------------------------------------------------------------------------------------------------
# row keys: one launch never repeats a row of noise
# ---------------------------------------------------------------------------------------------------------------------
def _step_keys(P, step, calls=L_HEADLINE):
    ctr = np.uint64(step * _stride(P)) + np.arange(calls * P, dtype=np.uint64)
    return ctr, rng_key(ctr, SEED)


@pytest.mark.parametrize("P,steps", [(P_HEADLINE, (1, 2, 1000, 3849)), (P_1M, (1, 100, 178, 179, 180))])
def test_row_keys_of_one_step_are_distinct(P, steps):
    """While the counter's high word is fixed, the key is lowbias32 (a bijection of 32 bits) of the low word plus a
    constant: the 3 P rows one XSimGCL step perturbs (calls 0..2) get distinct keys, hence distinct noise rows.  At the
    1 M x 500 k shape step * stride crosses 2^32 between steps 178 and 179."""
    for s in steps:
        ctr, key = _step_keys(P, s)
        hi = ctr >> np.uint64(32)
        assert hi[0] == hi[-1], s                                           # (the launch keeps one high word)
        assert np.unique(key).size == key.size, s


@pytest.mark.parametrize("P", [P_HEADLINE, P_1M])
def test_row_keys_across_a_high_word_change_collide_no_more_than_32_bit_birthdays(P):
    """Across a change of the counter's high word the key moves by a constant (lowbias32(hi ^ seed_hi) changes), so the
    two parts of a launch can share keys like two independent sets of 32-bit values: n1 n2 / 2^32 expected.  Measured with
    the default seed: the first launch that straddles 2^32 (step 19252 at the headline P, 3400 at P = 1.5 M) has 2 (2.4
    expected) and 145 (123.7 expected) duplicate keys; two consecutive steps across the change 11 (10.2) and 4,745 (4,715)."""
    stride, n = _stride(P), L_HEADLINE * P
    s = np.arange(1, 1 << 20, dtype=np.int64)
    straddle = int(s[((s * stride) >> 32) != ((s * stride + n - 1) >> 32)][0])
    s1 = (1 << 32) // stride
    for ctr in (np.uint64(straddle * stride) + np.arange(n, dtype=np.uint64),
                np.concatenate([np.uint64(t * stride) + np.arange(n, dtype=np.uint64) for t in (s1, s1 + 1)])):
        hi = ctr >> np.uint64(32)
        n1 = int(np.count_nonzero(hi == hi[0]))
        n2 = ctr.size - n1
        assert n1 and n2
        expect = n1 * n2 / 2.0 ** 32
        dups = ctr.size - np.unique(rng_key(ctr, SEED)).size
        assert dups <= expect + 5 * np.sqrt(expect) + 1, (P, dups, expect)


# ---------------------------------------------------------------------------------------------------------------------
# the counter map of every layout
# ---------------------------------------------------------------------------------------------------------------------
class _Comm:
    """stand-in communicator: the layouts' counter functions read world and rank only"""
    def __init__(self, world, rank):
        self.world, self.rank = world, rank


class _TrainerFields:
    """the fields engine_counter0 reads, as FusedTrainer sets them from its placement (engine.py __init__)"""
    def __init__(self, place, L, seed):
        self.rows, self.P, self.L = place.rows, place.rows.P, L
        self._rng_calls = max(16, 2 * L)
        self.rng_seed = place.sync.rng_seed(seed)


def _placements(layout, world, N, U, d):
    out = []
    for r in range(world):
        if layout == "single":
            p = layouts.make_placement(False, None, d, None, None)
        elif layout.startswith("2d"):
            gc, gr = (int(v) for v in layout.split(":")[1].split("x"))
            comm = (_Comm(gc, r // gr), _Comm(gr, r % gr))
            p = layouts.make_placement(layout, comm, d, None, None)
        else:
            p = layouts.make_placement(layout, _Comm(world, r), d, None, None)
        out.append(p)
    for p in out:
        p.rows.bind(N, U, "cpu")
        p.colx.bind(d, d)
    return out


@pytest.mark.parametrize("model,L", [("XSimGCL", 3), ("SimGCL", 3), ("SimGCL", 9)])
@pytest.mark.parametrize("layout,world", [("single", 1), ("rows", 2), ("rows", 8), ("cols", 4), ("2d:2x2", 4),
                                          ("2d:2x4", 8), ("dp", 4)])
def test_counter_map_of_every_layout(layout, world, model, L):
    """(seed, counter) of every row every rank perturbs in every perturbed call of four consecutive steps: pairwise
    distinct within a rank-row (the ranks that own one set of table rows), across rank-rows and across steps; the column
    blocks of one rank-row regenerate the same whole-row counters, and their slices tile the row."""
    N, U, d = 1003, 401, 64
    calls = L if model == "XSimGCL" else 2 * L
    places = _placements(layout, world, N, U, d)
    groups = {}
    for p in places:
        f = _TrainerFields(p, L, SEED)
        n_rows = p.rows.n_pad                          # the rows this rank's launches cover (rows.own)
        assert p.rows.P >= N and f.P * f._rng_calls == f.P * max(16, 2 * L)
        pairs = []
        for step in range(1, 5):
            for call in range(calls):
                ctr = np.uint64(engine_counter0(f, step, call)) + np.arange(n_rows, dtype=np.uint64)
                pairs.append(np.stack([np.full(n_rows, f.rng_seed, dtype=np.uint64), ctr], 1))
        pairs = np.concatenate(pairs)
        key = (p.rows.part, p.sync.rank)
        groups.setdefault(key, []).append((p, pairs))
    every = []
    for key, members in groups.items():
        p0, pairs0 = members[0]
        assert np.unique(pairs0, axis=0).shape[0] == pairs0.shape[0], key        # no reuse inside a rank-row
        for p, pairs in members[1:]:
            assert np.array_equal(pairs, pairs0), key                          # column blocks: the same whole-row counters
        spans = sorted((m[0].colx.slice_kw().get("col0", 0), m[0].colx.w) for m in members)
        assert all(m[0].colx.slice_kw().get("d_full", d) == d for m in members)
        assert [c0 for c0, _ in spans] == list(range(0, d, spans[0][1])) and sum(w for _, w in spans) == d
        every.append(pairs0)
    every = np.concatenate(every)
    assert np.unique(every, axis=0).shape[0] == every.shape[0]                   # nor across rank-rows, seeds or steps
    if layout in ("rows", "2d:2x2", "2d:2x4"):
        # the row parts together cover the table rows 0..P-1 of every call exactly once
        parts = {m[0].rows.part: m[0] for ms in groups.values() for m in ms}
        assert sorted(parts) == list(range(len(parts)))
        assert sum(pp.rows.n_pad for pp in parts.values()) == next(iter(parts.values())).rows.P
