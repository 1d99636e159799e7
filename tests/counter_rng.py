"""numpy restatement of the in-kernel perturbation noise -- TEST INFRASTRUCTURE ONLY.

The SpMM epilogue's counter RNG (include/selfrec_hip.h, srh_spmm_epilogue::rng_*; csrc/spmm.hip: lowbias32,
counter_rng4, u01) is a pure function of (seed, counter, float4 number of the row), so a host restatement says which
numbers every launch draws.  Written from that contract in numpy uint32 / uint64 arithmetic (wrapping, as on the
device); the product never imports this module.

    key   = lowbias32(lo(ctr) ^ lo(seed)) + lowbias32(hi(ctr) ^ hi(seed))
    base  = key + sub * 0x9E3779B1                                  (sub: float4 number of the row)
    words = lowbias32(base + {0, 0x85EBCA6B, 0xC2B2AE35, 0x27D4EB2F})
    u01   = (w >> 8) * 2^-24

A launch's row r (table row of the rank's slice) uses counter rng_offset + *rng_step * rng_stride + r.  The engine lays
its calls out as step * (P * rng_calls) + call * P + (first table row of the rank) + local row (engine.py, FusedTrainer:
_rng_calls, _rng_offset)."""
import numpy as np
import torch

M32 = np.uint64(0xFFFFFFFF)
MASK62 = (1 << 62) - 1
GOLDEN = np.uint32(0x9E3779B1)
LANE_ADD = np.array([0, 0x85EBCA6B, 0xC2B2AE35, 0x27D4EB2F], dtype=np.uint32)


def lowbias32(x):
    x = np.asarray(x, dtype=np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x


def _u64(v):
    return np.asarray(v, dtype=np.uint64) if not isinstance(v, int) else np.uint64(v & 0xFFFFFFFFFFFFFFFF)


def rng_key(ctr, seed):
    """the per-counter key: lowbias32(lo(ctr) ^ lo(seed)) + lowbias32(hi(ctr) ^ hi(seed)) (uint32, wrapping)"""
    ctr, seed = _u64(ctr), _u64(seed)
    lo = ((ctr & M32) ^ (seed & M32)).astype(np.uint32)
    hi = ((ctr >> np.uint64(32)) ^ (seed >> np.uint64(32))).astype(np.uint32)
    return lowbias32(lo) + lowbias32(hi)


def rng4(ctr, sub, seed):
    """(..., 4) uint32 words of float4 number `sub` at counter `ctr` (broadcast)"""
    base = rng_key(ctr, seed)[..., None] + np.asarray(sub, dtype=np.uint32)[..., None] * GOLDEN
    return lowbias32(base + LANE_ADD)


def u01(w):
    """(w >> 8) * 2^-24 as float32: 24 bits, in [0, 1 - 2^-24]"""
    return ((np.asarray(w, dtype=np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24))


def counters(ctr0, n_rows):
    """uint64 counters ctr0, ctr0 + 1, ... (wrapping at 2^64)"""
    return _u64(ctr0) + np.arange(n_rows, dtype=np.uint64)


def counter_noise(seed, ctr0, n_rows, d_full, d_valid=None, ctrs=None):
    """(n_rows, d_full) float32: row r drawn at counter ctr0 + r (or ctrs[r]), float4 q with sub = q; columns at or past
    d_valid are 0 (zero-padded rows)"""
    assert d_full % 4 == 0
    ctr = counters(ctr0, n_rows) if ctrs is None else _u64(ctrs)
    nq = d_full // 4
    key = rng_key(ctr, seed)[:, None] + np.arange(nq, dtype=np.uint32)[None, :] * GOLDEN      # (rows, nq)
    z = u01(lowbias32(key[..., None] + LANE_ADD)).reshape(ctr.size, d_full)
    if d_valid is not None and d_valid < d_full:
        z[:, d_valid:] = 0.0
    return z


def step_stride(tr):
    """counter distance between two optimiser steps of a trainer (rng_stride of its perturbed launches)"""
    return int(tr.P) * int(tr._rng_calls)


def engine_counter0(tr, step, call):
    """Counter of the first row of the rank's slice for perturbed-layer call `call` of optimiser step `step` (1-based:
    the value of cursor[1] while the step runs): the launch's rng_offset (62 bits) plus step * rng_stride, mod 2^64."""
    off = (int(call) * int(tr.P) + int(tr.rows.rng_row_offset())) & MASK62
    return (off + int(step) * step_stride(tr)) & 0xFFFFFFFFFFFFFFFF


def engine_node_noise(tr, step, call):
    """(N, d) float32: the noise the trainer's call `call` of step `step` draws, one row per NODE (users then items), d_valid
    columns non-zero -- what the oracle's noise_fn is handed.  Node p sits at table row rows.pos[p]; the counter of table row
    t is step * stride + call * P + t (t counts from the first row of the whole table)."""
    base = engine_counter0(tr, step, call) - int(tr.rows.rng_row_offset())
    ctrs = (_u64(base) + np.asarray(tr.rows.pos, dtype=np.uint64))
    return counter_noise(tr.rng_seed, 0, ctrs.size, tr.d, tr.d_valid, ctrs=ctrs)


class EngineNoise:
    """noise_fn for oracle.selfrec_oracle.OracleTrainer that hands out, in the oracle's call order, the noise a trainer
    with noise_fn=None draws in kernel.  Set `step` before each ref.step(...): calls count from 0 there.

    XSimGCL: calls 0..L-1 are layers 1..L.  SimGCL: view a takes calls 0..L-1, view b L..2L-1 (the oracle encodes a
    first).  `lag` (power checks) draws the noise of step - lag; `swap_views` hands view b's noise to view a and back."""

    def __init__(self, tr, lag=0, swap_views=False):
        self.tr, self.lag, self.swap = tr, int(lag), bool(swap_views)
        self.L = int(tr.L)
        self._step, self.call = None, 0

    @property
    def step(self):
        return self._step

    @step.setter
    def step(self, s):
        self._step, self.call = int(s), 0

    def __call__(self, shape):
        n, dv = int(shape[0]), int(shape[1])
        assert self._step is not None, "set .step before the oracle's step"
        assert n == self.tr.N and dv == self.tr.d_valid, (shape, self.tr.N, self.tr.d_valid)
        call = self.call
        if self.swap:
            call = (call + self.L) % (2 * self.L)
        self.call += 1
        z = engine_node_noise(self.tr, self._step - self.lag, call)
        return torch.from_numpy(np.ascontiguousarray(z[:, :dv]))
