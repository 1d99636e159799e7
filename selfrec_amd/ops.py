"""Torch-tensor front end of the C ABI: pointer extraction, shape checks, stream plumbing.

PyTorch is the memory container here and nothing else: every function hands raw device
addresses (``tensor.data_ptr()``) and the current HIP stream to libselfrec_hip.so.
"""
from __future__ import annotations

import ctypes as C
import functools
import random as _pyrandom

import numpy as np
import torch

from . import _lib
from ._lib import SelfrecHipError, SpmmEpilogue, check

require_gpu = _lib.require_gpu


def gpu_available() -> bool:
    return torch.cuda.is_available()

__all__ = ["Sampler", "DeviceCSR", "column_class_order", "spmm", "spmm_any", "pad_cols", "padded_width", "spmm3", "spmm_probe", "spmm_set_xcd_shares", "spmm_plan_run_tasks", "adj_sym_normalize", "bpr_l2_fwd_bwd", "bpr_fwd", "bpr_bwd",
           "sumsq", "set_infonce_precision", "get_infonce_precision", "infonce_fwd_bwd", "infonce_multi", "bpr_infonce", "infonce_ws", "adam_step", "score_mask_topk", "score_mask_topk_filtered", "gemm_nt", "topk_rows", "topk_hit_flags", "metric_rows",
           "axpby", "batch_fetch", "zero_rows", "cursor_advance", "batch_lists", "batch_pack", "batch_unpack", "batch_scatter",
           "table_nce_ws", "table_nce_fwd_bwd", "kmeans_assign", "kmeans_update", "kmeans",
           "find_k_largest_host_f64", "knn_neighbours", "knn_score_ws", "knn_score_topk",
           "tower_fwd", "tower_bwd", "scatter_plan", "scatter_plan_host", "rows_segment_sum", "batch_softmax_fwd_bwd", "TowerFn",
           "BatchSoftmaxFn", "seq_attn_supported", "seq_attn_fwd", "seq_attn_bwd", "SeqAttnFn", "seq_bce_fwd_bwd", "SeqBceFn",
           "GatherRowsFn", "seq_attn_full_fwd", "seq_attn_full_bwd", "SeqAttnFullFn", "table_ce_fwd_bwd", "TableCeFn",
           "seq_embed_fwd", "live_plan_host", "live_plan", "rows_live_sum", "SeqEmbedFn", "SeqBceLiveFn", "InfoNceFn",
           "rows_l2norm_fwd", "rows_l2norm_bwd", "NormPropFn", "tri_nd_fwd_bwd", "TriNdFn", "unique_first",
           "gate_fwd", "gate_bwd", "GateFn", "chan_mix_fwd", "chan_mix_bwd", "ChanMixFn", "mim_fwd_bwd", "MimFn",
           "RowsL2NormFn", "mixup_supported", "mixup_fwd", "mixup_bwd", "MixupFn", "SelfrecHipError"]


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t, dtype=None, name="tensor"):
    """Device address of a contiguous CUDA(HIP) tensor (None -> NULL)."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise SelfrecHipError(f"{name}: expected a HIP device tensor (the product path has no CPU fallback)")
    if dtype is not None and t.dtype != dtype:
        raise SelfrecHipError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise SelfrecHipError(f"{name}: tensor must be contiguous")
    return t.data_ptr()


def _np(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return a, a.ctypes.data_as(C.c_void_p)


def find_k_largest_host(k: int, candidates) -> tuple[np.ndarray, np.ndarray]:
    """ids (int64), scores (float32) of reference util/algorithm.py:144-156 ``find_k_largest`` -- the heap's own order among
    equal scores -- for a float32 vector on the host (srh_find_k_largest_host: python's heapq restated in C++)."""
    cand = np.ascontiguousarray(candidates, dtype=np.float32)
    m = min(int(k), int(cand.size))
    ids, sc = np.empty(m, dtype=np.int64), np.empty(m, dtype=np.float32)
    n_out = C.c_int64()
    check(_lib.load().srh_find_k_largest_host(int(k), cand.ctypes.data_as(C.c_void_p), int(cand.size),
                                              ids.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.c_void_p), C.byref(n_out)),
          "srh_find_k_largest_host")
    assert n_out.value == m
    return ids, sc



def find_k_largest_host_f64(k: int, candidates) -> tuple[np.ndarray, np.ndarray]:
    """find_k_largest_host for a float64 vector (UserKNN / ItemKNN rows): ids (int64), scores (float64) in the reference
    heap walk's order (srh_find_k_largest_host_f64)."""
    cand = np.ascontiguousarray(candidates, dtype=np.float64)
    m = min(int(k), int(cand.size))
    ids, sc = np.empty(m, dtype=np.int64), np.empty(m, dtype=np.float64)
    n_out = C.c_int64()
    check(_lib.load().srh_find_k_largest_host_f64(int(k), cand.ctypes.data_as(C.c_void_p), int(cand.size),
                                                  ids.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.c_void_p),
                                                  C.byref(n_out)), "srh_find_k_largest_host_f64")
    assert n_out.value == m
    return ids, sc

# ----------------------------------------------------------------------------------------
# (a-1) sampler
# ----------------------------------------------------------------------------------------
class Sampler:
    """Host-side bit-exact replay of util/sampler.py:5-28 (see csrc/sampler.cpp)."""

    def __init__(self, edge_user, edge_item, n_users: int, n_items: int):
        self._lib = _lib.load()
        eu, pu = _np(edge_user, np.int32)
        ei, pi = _np(edge_item, np.int32)
        if eu.shape != ei.shape or eu.ndim != 1:
            raise SelfrecHipError("Sampler: edge arrays must be 1-D and of equal length")
        self.n_users, self.n_items, self.n_edges = int(n_users), int(n_items), int(eu.size)
        h = C.c_void_p()
        check(self._lib.srh_sampler_create(C.byref(h), n_users, n_items, eu.size, pu, pi), "srh_sampler_create")
        self._h = h
        self._pushed = None            # the words this object last handed to python's generator (set_state_from_python)
        self._epoch_slots = {}         # epoch(slot=...): arrays the sampler keeps and overwrites

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._lib.srh_sampler_destroy(h)
            self._h = None

    # -- RNG state ------------------------------------------------------------------
    def set_state_from_python(self, state=None):
        """Adopt ``random.getstate()`` (version 3 tuple: 624 words + position).  When python's generator still holds the
        very state this object pushed last (nobody drew from ``random`` in between -- the per-batch case of
        ``next_batch_pairwise``), the C++ generator is already there and nothing is converted: boxing 624 words into
        a numpy array and back cost ~150 us per batch, a tenth of an op-level LightGCN step."""
        state = _pyrandom.getstate() if state is None else state
        if state[0] != 3 or len(state[1]) != 625:
            raise SelfrecHipError("unsupported random.getstate() layout")
        self._gauss = state[2]
        if self._pushed is not None and state[1] == self._pushed:
            return
        words = np.array(state[1][:624], dtype=np.uint32)
        check(self._lib.srh_sampler_set_state(self._h, words.ctypes.data_as(C.c_void_p), int(state[1][624])))
        self._pushed = None

    def python_state(self):
        """The generator state as a tuple ``random.setstate`` accepts."""
        words = np.empty(624, dtype=np.uint32)
        pos = C.c_int32()
        check(self._lib.srh_sampler_get_state(self._h, words.ctypes.data_as(C.c_void_p), C.byref(pos)))
        return (3, tuple(words.tolist()) + (int(pos.value),), getattr(self, "_gauss", None))

    def push_state_to_python(self):
        state = self.python_state()
        _pyrandom.setstate(state)
        self._pushed = state[1]

    def seed(self, seed: int):
        check(self._lib.srh_sampler_seed(self._h, int(seed)), "srh_sampler_seed")
        self._gauss = None
        self._pushed = None

    # -- draws ----------------------------------------------------------------------
    def shuffle(self):
        self._pushed = None                      # (the C++ generator moves on: python's copy is behind until the next push)
        check(self._lib.srh_sampler_shuffle(self._h), "srh_sampler_shuffle")

    def order(self) -> np.ndarray:
        perm = np.empty(self.n_edges, dtype=np.int64)
        check(self._lib.srh_sampler_get_order(self._h, perm.ctypes.data_as(C.c_void_p)))
        return perm

    def next_batch(self, ptr: int, batch_size: int, n_negs: int = 1):
        cnt = min(batch_size, self.n_edges - ptr)
        u = np.empty(cnt, dtype=np.int32)
        i = np.empty(cnt, dtype=np.int32)
        j = np.empty(cnt * n_negs, dtype=np.int32)
        out = C.c_int64()
        self._pushed = None                      # (the C++ generator moves on: python's copy is behind until the next push)
        check(self._lib.srh_sampler_next_batch(self._h, ptr, batch_size, n_negs, u.ctypes.data_as(C.c_void_p),
                                               i.ctypes.data_as(C.c_void_p), j.ctypes.data_as(C.c_void_p),
                                               C.byref(out)), "srh_sampler_next_batch")
        assert out.value == cnt
        return u, i, j

    def epoch(self, batch_size: int, n_negs: int = 1, with_unique: bool = False, slot=None, with_segments: bool = False):
        """shuffle + all batches.  Returns dict of numpy arrays (see srh_sampler_epoch).
        with_segments (True | (user_row0, item_row0)): also the row -> slot lists of every batch (srh_sampler_epoch_segments:
        n_uniq_n, seg_rows, seg_end, seg, seg_a, seg_b -- table rows = ids + the offsets) behind the fixed-order
        batch-gradient reduction.
        slot (None | 0 | 1 | ...): None -- fresh arrays, the caller's to keep.  An integer -- the arrays of that slot, owned
        by the sampler and OVERWRITTEN by the next call with the same slot: a training loop that alternates two slots never
        allocates or frees an epoch's 25 MB (freeing them -- munmap -- beside a thread that is enqueueing GPU work was
        measured to stall it: 0.4 ms per epoch boundary, profiles/r05_o_epoch_boundary_host_cost.txt)."""
        e = self.n_edges
        nb = (e + batch_size - 1) // batch_size
        key = (slot, int(batch_size), int(n_negs), bool(with_unique))
        held = None if slot is None else self._epoch_slots.get(key)
        if held is not None:
            u, i, j = held["u"], held["i"], held["j"]
            res = {"u": u, "i": i, "j": j, "n_batches": nb}
            uu = ui = nuu = nui = None
            if with_unique:
                uu, ui, nuu, nui = held["uniq_u"], held["uniq_i"], held["n_uniq_u"], held["n_uniq_i"]
                for a in (uu, ui, nuu, nui):
                    a.fill(0)
                res.update(uniq_u=uu, uniq_i=ui, n_uniq_u=nuu, n_uniq_i=nui)
        else:
            u = np.empty(e, dtype=np.int32)
            i = np.empty(e, dtype=np.int32)
            j = np.empty(e * n_negs, dtype=np.int32)
            res = {"u": u, "i": i, "j": j, "n_batches": nb}
            uu = ui = nuu = nui = None
            if with_unique:
                uu = np.zeros(nb * batch_size, dtype=np.int32)
                ui = np.zeros(nb * batch_size, dtype=np.int32)
                nuu = np.zeros(nb, dtype=np.int32)
                nui = np.zeros(nb, dtype=np.int32)
                res.update(uniq_u=uu, uniq_i=ui, n_uniq_u=nuu, n_uniq_i=nui)
            if slot is not None:
                self._epoch_slots[key] = {k: v for k, v in res.items() if k != "n_batches"}
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
        self._pushed = None                      # (the C++ generator moves on: python's copy is behind until the next push)
        check(self._lib.srh_sampler_epoch(self._h, batch_size, n_negs, vp(u), vp(i), vp(j), vp(uu), vp(nuu),
                                          vp(ui), vp(nui)), "srh_sampler_epoch")
        if with_segments:
            if not with_unique or n_negs != 1:
                raise SelfrecHipError("Sampler.epoch: with_segments needs with_unique and n_negs = 1")
            user_row0, item_row0 = (0, 0) if with_segments is True else (int(with_segments[0]), int(with_segments[1]))
            seg = None if slot is None else self._epoch_slots.get(key + ("seg",))
            if seg is None:
                seg = {"n_uniq_n": np.zeros(nb, dtype=np.int32), "seg_b": np.zeros(nb * batch_size, dtype=np.int32)}
                seg.update({k: np.zeros(3 * nb * batch_size, dtype=np.int32) for k in ("seg_rows", "seg_end", "seg", "seg_a")})
                if slot is not None:
                    self._epoch_slots[key + ("seg",)] = seg
            check(self._lib.srh_sampler_epoch_segments(self._h, batch_size, vp(u), vp(i), vp(j), vp(uu), vp(nuu), vp(ui), vp(nui),
                                                       user_row0, item_row0, vp(seg["n_uniq_n"]), vp(seg["seg_rows"]),
                                                       vp(seg["seg_end"]), vp(seg["seg"]), vp(seg["seg_a"]), vp(seg["seg_b"])),
                       "srh_sampler_epoch_segments")
            res.update(seg)
        return res

    def sample_range(self, n: int, k: int) -> np.ndarray:
        out = np.empty(k, dtype=np.int64)
        self._pushed = None                      # (the C++ generator moves on: python's copy is behind until the next push)
        check(self._lib.srh_sampler_sample_range(self._h, n, k, out.ctypes.data_as(C.c_void_p)),
              "srh_sampler_sample_range")
        return out

    def next_u32(self) -> int:
        v = C.c_uint32()
        self._pushed = None                      # (the C++ generator moves on: python's copy is behind until the next push)
        check(self._lib.srh_sampler_next_u32(self._h, C.byref(v)))
        return int(v.value)


# ----------------------------------------------------------------------------------------
# (a-2..a-4) device CSR, normalisation, SpMM
# ----------------------------------------------------------------------------------------
class DeviceCSR:
    """CSR matrix resident in HBM (int32 structure, fp32 values) plus its SpMM schedule.

    ``structure_of`` shares indptr/indices/plan with another DeviceCSR (edge-dropped views
    are new value arrays over the same structure).
    """

    def __init__(self, indptr, indices, vals, shape, device=None, split_len: int = 0, structure_of=None,
                 xcd_split_row: int = 0, row_mid=None):
        self._lib = _lib.load()
        _lib.require_gpu()
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
        self.shape = (int(shape[0]), int(shape[1]))
        if structure_of is not None:
            self.indptr, self.indices, self._plan_owner = structure_of.indptr, structure_of.indices, structure_of
            self.h_indptr = structure_of.h_indptr
            self._plan = structure_of._plan
        else:
            h_indptr = np.ascontiguousarray(indptr, dtype=np.int32)
            if h_indptr.size != self.shape[0] + 1:
                raise SelfrecHipError("DeviceCSR: indptr length != n_rows + 1")
            self.h_indptr = h_indptr
            self.indptr = torch.from_numpy(h_indptr).to(device)
            self.indices = torch.as_tensor(np.ascontiguousarray(indices, dtype=np.int32)).to(device)
            h = C.c_void_p()
            h_mid = None if row_mid is None else np.ascontiguousarray(row_mid, dtype=np.int32)
            if h_mid is not None and h_mid.size != self.shape[0]:
                raise SelfrecHipError("DeviceCSR: row_mid needs one entry per row")
            check(self._lib.srh_spmm_plan_create(C.byref(h), self.shape[0], self.shape[1],
                                                 h_indptr.ctypes.data_as(C.c_void_p), split_len, int(xcd_split_row),
                                                 None if h_mid is None else h_mid.ctypes.data_as(C.c_void_p)),
                  "srh_spmm_plan_create")
            self._plan = h
            self._plan_owner = None
        if isinstance(vals, torch.Tensor):
            self.vals = vals.to(device=device, dtype=torch.float32).contiguous()
        else:
            self.vals = torch.as_tensor(np.ascontiguousarray(vals, dtype=np.float32)).to(device)
        self.nnz = int(self.indices.numel())
        if self.vals.numel() != self.nnz:
            raise SelfrecHipError("DeviceCSR: values / indices length mismatch")

    def __del__(self):
        if getattr(self, "_plan_owner", 1) is None and getattr(self, "_plan", None):
            self._lib.srh_spmm_plan_destroy(self._plan)
            self._plan = None

    @classmethod
    def from_scipy(cls, mat, device=None, split_len: int = 0):
        m = mat.tocsr()
        m.sort_indices()
        return cls(m.indptr, m.indices, m.data, m.shape, device=device, split_len=split_len)

    def with_values(self, vals):
        return DeviceCSR(None, None, vals, self.shape, device=self.vals.device, structure_of=self)

    def replanned(self, split_len: int = 0, xcd_split_row: int = 0, row_mid=None):
        """The same matrix (the device arrays are shared) under ANOTHER SpMM schedule: its own segment length and
        task-to-XCD dealing.  The engine runs the column-masked launch of a step on a class-free plan."""
        other = DeviceCSR.__new__(DeviceCSR)
        other._lib = self._lib
        other.shape, other.h_indptr, other.indptr, other.indices = self.shape, self.h_indptr, self.indptr, self.indices
        h = C.c_void_p()
        h_mid = None if row_mid is None else np.ascontiguousarray(row_mid, dtype=np.int32)
        check(self._lib.srh_spmm_plan_create(C.byref(h), self.shape[0], self.shape[1],
                                             self.h_indptr.ctypes.data_as(C.c_void_p), int(split_len), int(xcd_split_row),
                                             None if h_mid is None else h_mid.ctypes.data_as(C.c_void_p)),
              "srh_spmm_plan_create")
        other._plan, other._plan_owner = h, None
        other.vals, other.nnz = self.vals, self.nnz
        other._arrays_of = self                    # (keeps the shared tensors' owner alive)
        return other


def column_class_order(indptr, indices, min_len: int, bit: int = 0):
    """Host helper for DeviceCSR(row_mid=...): reorder the entries of every row with >= min_len non-zeros
    as [class-0 columns | class-1 columns] (stable), leave the others alone; a column's class is bit `bit` of its
    id (0: even / odd).  Returns (perm, row_mid): apply perm to indices / values / anything aligned with them;
    row_mid[r] = number of class-0 entries of a reordered row, or -1 - c for a row left whole whose columns are
    mostly of class c."""
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices)
    n = indptr.size - 1
    lens = np.diff(indptr)
    row_of = np.repeat(np.arange(n, dtype=np.int64), lens)
    odd = ((indices >> int(bit)) & 1).astype(np.int64)
    split = lens >= int(min_len)
    key = row_of * 2 + np.where(split[row_of], odd, 0)
    perm = np.argsort(key, kind="stable")
    n_odd = np.bincount(row_of, weights=odd, minlength=n).astype(np.int64)
    n_even = lens - n_odd
    row_mid = np.where(split, n_even, -1 - (n_odd > n_even).astype(np.int64)).astype(np.int32)
    return perm, row_mid


ADAM_EPILOGUE = True      # make_epilogue(adam=...) / batch_fetch_args(adam_coef=...) exist (engine.py: fuse_adam)


def make_epilogue(*, perturb_eps=None, noise=None, rng_seed=0, rng_offset=0, rng_step=None,
                  rng_stride=0, prev=None, mean_div=None, mean_out=None, add=None, add_scale=None, alpha=1.0,
                  row_mark=None, col_mark=None, mark_stamp=None, add_mark=None, add_sparse=None,
                  extra_out=None, extra_noise=None, extra_rng_offset=None, main_clean=False, d_full=0, col0=0,
                  row_scale=None, scale_in=False, scale_out=False, prev_unscale=None, add_rowscale=None, d_valid=0,
                  adam=None):
    """row_scale / scale_in / scale_out / prev_unscale / add_rowscale: per-row scaling for value-free products
    (include/selfrec_hip.h: SRH_SCALE_*); prev_unscale / add_rowscale are lists of booleans aligned with prev / add.
    adam: dict(param, m, v, coef, beta1, beta2, eps, clear=[tables], clear_mark, cursor) -- SRH_EPI_ADAM: the product (after
    AXPY) is the gradient of `param`, which takes the optimiser's step in the epilogue instead of the gradient being stored;
    mark_stamp must then be batch_fetch's COPY of the step."""
    ep = SpmmEpilogue()
    if row_scale is not None:
        ep.d_row_scale = _p(row_scale, torch.float32, "row_scale")
        ep.scale_flags = (_lib.SRH_SCALE_IN if scale_in else 0) | (_lib.SRH_SCALE_OUT if scale_out else 0)
        ep.prev_unscale_mask = sum(1 << t for t, f in enumerate(prev_unscale or []) if f)
        ep.add_rowscale_mask = sum(1 << t for t, f in enumerate(add_rowscale or []) if f)
    ep.noise_d_full, ep.noise_col0 = int(d_full), int(col0)      # column-sharded tables (0 = whole rows)
    ep.noise_d_valid = int(d_valid)                               # zero-padded rows: PERTURB's noise ends here (0 = all)
    keep = []
    flags = 0
    if perturb_eps is not None:
        flags |= _lib.SRH_EPI_PERTURB
        ep.eps = float(perturb_eps)
        ep.d_noise = _p(noise, torch.float32, "noise")
        ep.rng_seed, ep.rng_offset = int(rng_seed), int(rng_offset)
        ep.d_rng_step = _p(rng_step, torch.int64, "rng_step")
        ep.rng_stride = int(rng_stride)
        keep += [noise, rng_step]
        extra_out = list(extra_out or [])
        if extra_out or main_clean:        # further perturbed copies of the same product (SimGCL layer 1)
            if len(extra_out) > _lib.SRH_MAX_EXTRA:
                raise SelfrecHipError(f"at most {_lib.SRH_MAX_EXTRA} extra perturbed outputs")
            ep.n_extra, ep.main_clean = len(extra_out), int(bool(main_clean))
            for k, t in enumerate(extra_out):
                ep.d_extra_out[k] = _p(t, torch.float32, "extra_out")
                ep.d_extra_noise[k] = _p((extra_noise or [None] * len(extra_out))[k], torch.float32, "extra_noise")
                ep.extra_rng_offset[k] = int((extra_rng_offset or [0] * len(extra_out))[k])
            keep += extra_out + list(extra_noise or [])
    if mean_out is not None:
        flags |= _lib.SRH_EPI_MEAN
        prev = list(prev or [])
        if len(prev) > _lib.SRH_MAX_PREV:
            raise SelfrecHipError(f"at most {_lib.SRH_MAX_PREV} earlier layers can be averaged in the epilogue")
        ep.n_prev = len(prev)
        for t, x in enumerate(prev):
            ep.d_prev[t] = _p(x, torch.float32, "prev")
        ep.mean_div = float(mean_div)
        ep.d_mean_out = _p(mean_out, torch.float32, "mean_out")
        keep += prev + [mean_out]
    if add or alpha != 1.0:
        add = list(add or [])
        flags |= _lib.SRH_EPI_AXPY
        ep.alpha = float(alpha)
        if len(add) > _lib.SRH_MAX_ADD:
            raise SelfrecHipError(f"at most {_lib.SRH_MAX_ADD} addends")
        ep.n_add = len(add)
        for t, x in enumerate(add):
            ep.d_add[t] = _p(x, torch.float32, "add")
            ep.add_scale[t] = float(add_scale[t])
        keep += list(add)
    if row_mark is not None or col_mark is not None or add_mark is not None:
        ep.d_row_mark = _p(row_mark, torch.int32, "row_mark")
        ep.d_col_mark = _p(col_mark, torch.int32, "col_mark")
        ep.d_mark_stamp = _p(mark_stamp, torch.int64, "mark_stamp")
        ep.d_add_mark = _p(add_mark, torch.int32, "add_mark")
        ep.add_sparse_mask = sum(1 << t for t, f in enumerate(add_sparse or []) if f)
        keep += [row_mark, col_mark, mark_stamp, add_mark]
    if adam is not None:
        flags |= _lib.SRH_EPI_ADAM
        ep.d_adam_param, ep.d_adam_m, ep.d_adam_v = (_p(adam[k], torch.float32, k) for k in ("param", "m", "v"))
        ep.d_adam_coef = _p(adam["coef"], torch.float32, "coef")
        ep.adam_beta1, ep.adam_beta2 = float(adam.get("beta1", 0.9)), float(adam.get("beta2", 0.999))
        ep.adam_eps = float(adam.get("eps", 1e-8))
        clear = list(adam.get("clear") or [])
        if len(clear) > _lib.SRH_MAX_ADAM_CLEAR:
            raise SelfrecHipError(f"at most {_lib.SRH_MAX_ADAM_CLEAR} tables to clear")
        ep.adam_n_clear = len(clear)
        for k, t in enumerate(clear):
            ep.d_adam_clear[k] = _p(t, torch.float32, "clear")
        ep.d_adam_clear_mark = _p(adam.get("clear_mark"), torch.int32, "clear_mark")
        ep.d_adam_cursor = _p(adam.get("cursor"), torch.int64, "cursor")
        if mark_stamp is not None and not ep.d_mark_stamp:
            ep.d_mark_stamp = _p(mark_stamp, torch.int64, "mark_stamp")
        keep += [adam, mark_stamp]
    ep.flags = flags
    ep._keepalive = keep + [row_scale]
    return ep


def spmm(csr: DeviceCSR, x: torch.Tensor, out: torch.Tensor | None = None, epilogue: SpmmEpilogue | None = None,
         pattern: bool = False, fetch=None, nce_stage=None):
    """out = csr @ x (+ fused epilogue).  x: (n_cols, d) fp32.  pattern=True: the structure with every stored entry 1
    (no value stream; d >= 64) -- with row scaling in the epilogue this is the value-free form of D^-1/2 A D^-1/2.
    fetch: a BatchFetchArgs (batch_fetch_args) -- the launch also stages the step's batch (srh_spmm_f32_with_fetch).
    nce_stage: (problems, nce_ws) as bpr_infonce(..., staged=True) will get them later in the step -- the launch also
    stages the InfoNCE passes' key-side view, counters and plan (srh_spmm_f32_with_nce_stage)."""
    if x.dim() != 2 or x.shape[0] != csr.shape[1]:
        raise SelfrecHipError(f"spmm: x has shape {tuple(x.shape)}, expected ({csr.shape[1]}, d)")
    d = int(x.shape[1])
    if out is None:
        out = torch.empty((csr.shape[0], d), dtype=torch.float32, device=x.device)
    common = (csr._plan, _p(csr.indptr, torch.int32), _p(csr.indices, torch.int32),
              None if pattern else _p(csr.vals, torch.float32, "vals"), _p(x, torch.float32, "x"),
              _p(out, torch.float32, "out"), d, C.byref(epilogue) if epilogue is not None else None)
    if nce_stage is not None:
        if fetch is not None:
            raise SelfrecHipError("spmm: one rider per launch (fetch or nce_stage)")
        problems, nce_ws = nce_stage
        arr = _infonce_problems(problems, d, nce_ws)
        check(_lib.load().srh_spmm_f32_with_nce_stage(*common, arr, len(problems), _p(nce_ws), _stream()),
              "srh_spmm_f32_with_nce_stage")
    elif fetch is not None:
        check(_lib.load().srh_spmm_f32_with_fetch(*common, C.byref(fetch), _stream()), "srh_spmm_f32_with_fetch")
    else:
        check(_lib.load().srh_spmm_f32(*common, _stream()), "srh_spmm_f32")
    return out


# ---- any table width through the boundary (reference base/recommender.py:16: `embedding.size` is any integer) ----
SPMM_WIDTHS = (8, 16, 32, 64, 128, 256)      # row widths srh_spmm_f32 serves (csrc/spmm.hip)
ROW_WIDTHS = (32, 64, 128, 256)              # LPR kernels: BPR / L2 / scoring GEMM (csrc/common.h: dim_supported)
NCE_WIDTHS = (64, 128, 256)                  # srh_infonce_fwd_bwd (256: the split path only)


def padded_width(d: int, widths) -> int | None:
    """The narrowest width of `widths` that holds d columns (None: wider than the widest)."""
    return next((w for w in widths if w >= int(d)), None)


def pad_cols(t: torch.Tensor, width: int) -> torch.Tensor:
    """(rows, d) -> contiguous (rows, width) with zero columns on the right (a no-op view when d == width).  Zero columns
    change none of the path's results: products, inner products, norms and F.normalize ignore them, their gradients
    are exactly zero."""
    d = int(t.shape[1])
    if d == width:
        return t.contiguous()
    out = torch.zeros((t.shape[0], width), dtype=t.dtype, device=t.device)
    out[:, :d] = t
    return out


def spmm_any(csr: DeviceCSR, x: torch.Tensor) -> torch.Tensor:
    """csr @ x for x of ANY width: 256-column blocks, the last one zero-padded to the next width the kernels serve.
    (Widths the kernels serve directly take the plain call: no copy.)"""
    d = int(x.shape[1])
    if d in SPMM_WIDTHS:
        return spmm(csr, x.contiguous())
    out = torch.empty((csr.shape[0], d), dtype=torch.float32, device=x.device)
    for c0 in range(0, d, SPMM_WIDTHS[-1]):
        wb = min(SPMM_WIDTHS[-1], d - c0)
        y = spmm(csr, pad_cols(x[:, c0:c0 + wb], padded_width(wb, SPMM_WIDTHS)))
        out[:, c0:c0 + wb] = y[:, :wb]
    return out


def spmm_plan_run_tasks(csr: DeviceCSR, d: int) -> int:
    """Records in the task list a launch of `csr` on d-column tables runs now (srh_spmm_plan_run_tasks)."""
    n = int(_lib.load().srh_spmm_plan_run_tasks(csr._plan, int(d)))
    if n < 0:
        raise SelfrecHipError(f"spmm_plan_run_tasks: no task list for d = {d}")
    return n


def spmm_set_xcd_shares(csr: DeviceCSR, d: int, blocks_per_xcd=None):
    """Deal the plan's workgroups of real tasks to the 8 XCDs in these numbers (srh_spmm_plan_set_xcd_shares; None: the
    canonical equal dealing).  Same tasks, same sums; synchronises the device -- never inside a stream capture, and a
    captured launch of this plan must be re-captured afterwards."""
    if blocks_per_xcd is None:
        check(_lib.load().srh_spmm_plan_set_xcd_shares(csr._plan, int(d), None), "srh_spmm_plan_set_xcd_shares")
        return
    h = np.ascontiguousarray(blocks_per_xcd, dtype=np.int32)
    if h.shape != (8,):
        raise SelfrecHipError("spmm_set_xcd_shares: eight shares, one per XCD")
    check(_lib.load().srh_spmm_plan_set_xcd_shares(csr._plan, int(d), h.ctypes.data_as(C.c_void_p)),
          "srh_spmm_plan_set_xcd_shares")


def spmm_probe(csr: DeviceCSR, x: torch.Tensor, out: torch.Tensor, epilogue: SpmmEpilogue | None = None, pattern: bool = False):
    """One srh_spmm_f32_probe launch (no column marks, d = 64 / 128 / 256).  Returns (finish, begin, end, xcd): finish[k]
    = when XCD k's last wave left, in us after the launch's first wave began; begin / end / xcd per stamped wave (us, us,
    0 .. 7) in task order.  A device-to-host sync: calibration and lab work, not the step."""
    d = int(x.shape[1])
    n = spmm_plan_run_tasks(csr, d)
    stamps = torch.zeros(3 * n, dtype=torch.int64, device=x.device)
    check(_lib.load().srh_spmm_f32_probe(csr._plan, _p(csr.indices, torch.int32), None if pattern else _p(csr.vals, torch.float32, "vals"),
                                         _p(x, torch.float32, "x"), _p(out, torch.float32, "out"), d,
                                         C.byref(epilogue) if epilogue is not None else None, stamps.data_ptr(), _stream()),
          "srh_spmm_f32_probe")
    rec = stamps.cpu().numpy().reshape(n, 3)
    rec = rec[rec[:, 1] != 0]
    if rec.shape[0] == 0:
        raise SelfrecHipError("spmm_probe: no wave left a stamp")
    t0 = rec[:, 0].min()
    begin, end, xcd = (rec[:, 0] - t0) / 100.0, (rec[:, 1] - t0) / 100.0, (rec[:, 2] & 0xff).astype(np.int64)
    finish = np.array([end[xcd == k].max() if (xcd == k).any() else 0.0 for k in range(8)])
    return finish, begin, end, xcd


def spmm_gather_bound(csr, x: torch.Tensor, iters: int = 30) -> float:
    """us per launch of srh_spmm_gather_bound on `csr`'s plan: the product's own gathers on the product's own schedule and
    nothing after them -- a measured lower bound of ``spmm(csr, x)`` (HIP events on the launch stream).  Measurement only."""
    d = int(x.shape[1])
    scratch = torch.zeros(d, dtype=torch.float32, device=x.device)
    lib = _lib.load()

    def once():
        check(lib.srh_spmm_gather_bound(csr._plan, _p(csr.indices, torch.int32), _p(x, torch.float32, "x"), scratch.data_ptr(),
                                        d, _stream()), "srh_spmm_gather_bound")
    for _ in range(5):
        once()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        once()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3


def gather_floor_probe(indices: torch.Tensor, x: torch.Tensor, blocks: int = 4096, iters: int = 30) -> float:
    """us per pass of the bare gather stream over `indices` into the (rows, d) table `x` (srh_gather_floor_probe: the row
    fetches of one propagation launch and nothing else), HIP events on the launch stream.  Measurement only."""
    d = int(x.shape[1])
    sink = torch.zeros(4, dtype=torch.float32, device=x.device)
    lib = _lib.load()

    def once():
        check(lib.srh_gather_floor_probe(_p(indices, torch.int32, "indices"), int(indices.numel()), _p(x, torch.float32, "x"),
                                         int(x.shape[0]), d, int(blocks), sink.data_ptr(), _stream()), "srh_gather_floor_probe")
    for _ in range(5):
        once()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        once()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3


def adj_sym_normalize(indptr, indices, edge_id, keep, n_rows: int, weight=None, out=None, deg_ws=None,
                      inv_sqrt_table=None, row_offset: int = 0, phase: int = 0):
    dev = indices.device
    if out is None:
        out = torch.empty(indices.numel(), dtype=torch.float32, device=dev)
    if deg_ws is None:
        deg_ws = torch.empty(n_rows, dtype=torch.float32, device=dev)
    check(_lib.load().srh_adj_sym_normalize(n_rows, _p(indptr, torch.int32), _p(indices, torch.int32),
                                            _p(edge_id, torch.int32), _p(weight, torch.float32),
                                            _p(keep, torch.uint8), _p(inv_sqrt_table, torch.float32),
                                            0 if inv_sqrt_table is None else int(inv_sqrt_table.numel()),
                                            _p(deg_ws, torch.float32),
                                            _p(out, torch.float32), int(row_offset), int(phase), _stream()),
          "srh_adj_sym_normalize")
    return out


def spmm3(csrs, x, outs):
    """outs[v] = csrs[v] @ x for three DeviceCSRs over ONE structure (srh_spmm3_f32: x rows gathered once).
    Raises SelfrecHipError (unsupported) unless d == 64."""
    base = csrs[0]
    if any(c._plan is not base._plan for c in csrs) or len(csrs) != 3 or len(outs) != 3:
        raise SelfrecHipError("spmm3: needs three value arrays over one structure and three outputs")
    check(_lib.load().srh_spmm3_f32(base._plan, _p(base.indices, torch.int32), _p(csrs[0].vals, torch.float32),
                                    _p(csrs[1].vals, torch.float32), _p(csrs[2].vals, torch.float32),
                                    _p(x, torch.float32, "x"), _p(outs[0], torch.float32), _p(outs[1], torch.float32),
                                    _p(outs[2], torch.float32), int(x.shape[1]), _stream()), "srh_spmm3_f32")


# ----------------------------------------------------------------------------------------
# (a-5..a-8) losses
# ----------------------------------------------------------------------------------------
def bpr_ws(batch: int, device):
    return torch.empty(int(_lib.load().srh_bpr_ws_bytes(batch)), dtype=torch.uint8, device=device)


def _segments(seg, nce_rows):
    """srh_batch_segments_t from a dict of device int32 tensors: n_uniq_u, n_uniq_i, n_uniq_n, seg_rows, seg_end, seg, seg_a, seg_b
    [, batch_no: the arrays are then EPOCH arrays] [, rows_are_zero: bool]."""
    g = _lib.BatchSegments()
    for k in ("n_uniq_u", "n_uniq_i", "n_uniq_n", "seg_rows", "seg_end", "seg", "seg_a", "seg_b"):
        setattr(g, "d_" + k, _p(seg[k], torch.int32))
    g.d_batch_no = _p(seg.get("batch_no"), torch.int32)
    g.nce_rows = int(nce_rows)
    g.rows_are_zero = int(bool(seg.get("rows_are_zero", False)))
    return g


def _bpr_problem(user, item, reg_user, reg_item, u_idx, i_idx, j_idx, batch, n_rows_dev, reg_coef, reg_include_neg, loss_scale,
                 g_user, g_item, greg_user, greg_item, losses, ws, seg, nce_rows):
    b = _lib.BprProblem()
    b.d_user, b.d_item = _p(user, torch.float32), _p(item, torch.float32)
    b.d_reg_user, b.d_reg_item = _p(reg_user, torch.float32), _p(reg_item, torch.float32)
    b.d_u_idx, b.d_i_idx, b.d_j_idx = _p(u_idx, torch.int32), _p(i_idx, torch.int32), _p(j_idx, torch.int32)
    b.B, b.d_n_rows = int(batch), _p(n_rows_dev, torch.int32)
    b.reg_coef, b.reg_include_neg, b.loss_scale = float(reg_coef), int(bool(reg_include_neg)), float(loss_scale)
    b.d_g_user, b.d_g_item = _p(g_user, torch.float32), _p(g_item, torch.float32)
    b.d_greg_user, b.d_greg_item = _p(greg_user, torch.float32), _p(greg_item, torch.float32)
    b.d_losses, b.d_ws = _p(losses, torch.float64), _p(ws)
    if seg is not None:
        b._seg = _segments(seg, nce_rows)          # (kept alive by the struct object)
        b.seg = C.pointer(b._seg)
    return b


def bpr_l2_fwd_bwd(user, item, reg_user, reg_item, u_idx, i_idx, j_idx, *, batch, n_rows_dev=None, reg_coef,
                   reg_include_neg, loss_scale, g_user, g_item, greg_user, greg_item, losses, ws, seg=None):
    """seg: the batch's row -> slot lists (see _segments): the gradients are summed row by row in slot order, no float atomics."""
    d = int(user.shape[1])
    if seg is not None:
        b = _bpr_problem(user, item, reg_user, reg_item, u_idx, i_idx, j_idx, batch, n_rows_dev, reg_coef, reg_include_neg,
                         loss_scale, g_user, g_item, greg_user, greg_item, losses, ws, seg, 0)
        check(_lib.load().srh_bpr_l2_fwd_bwd_p(C.byref(b), d, _stream()), "srh_bpr_l2_fwd_bwd_p")
        return
    check(_lib.load().srh_bpr_l2_fwd_bwd(
        _p(user, torch.float32), _p(item, torch.float32), _p(reg_user, torch.float32), _p(reg_item, torch.float32),
        _p(u_idx, torch.int32), _p(i_idx, torch.int32), _p(j_idx, torch.int32), int(batch),
        _p(n_rows_dev, torch.int32), d, float(reg_coef), int(bool(reg_include_neg)), float(loss_scale),
        _p(g_user, torch.float32), _p(g_item, torch.float32), _p(greg_user, torch.float32),
        _p(greg_item, torch.float32), _p(losses, torch.float64), _p(ws), _stream()), "srh_bpr_l2_fwd_bwd")


_scalar_ws = {}


def scalar_ws(device) -> torch.Tensor:
    """The 64-byte workspace the single-launch loss kernels finish their scalars in (SRH_SCALAR_WS_BYTES): one per device and
    stream, zero before its first use, left zero by every call."""
    # (one per device AND stream: the calls that share a workspace must be ordered, and a stream is what orders them)
    key = (device.index if device.index is not None else torch.cuda.current_device(), _stream())
    ws = _scalar_ws.get(key)
    if ws is None:
        ws = _scalar_ws[key] = torch.zeros(_lib.SCALAR_WS_BYTES // 8, dtype=torch.float64, device=device)
    return ws


def bpr_fwd(u, p, n, loss, coef):
    """loss (0-dim f32) = mean BPR loss of the rows; coef[b] = d loss / d (pos_b - neg_b).  One launch."""
    check(_lib.load().srh_bpr_fwd(_p(u, torch.float32), _p(p, torch.float32), _p(n, torch.float32), u.shape[0],
                                  int(u.shape[1]), scalar_ws(u.device).data_ptr(), _p(loss, torch.float32),
                                  _p(coef, torch.float32), _stream()), "srh_bpr_fwd")


def bpr_bwd(u, p, n, coef, gout, gu, gp, gn):
    """gout: the upstream gradient as a 0-dim f32 DEVICE tensor (read by the kernel: no host synchronisation)."""
    check(_lib.load().srh_bpr_bwd(_p(u, torch.float32), _p(p, torch.float32), _p(n, torch.float32),
                                  _p(coef, torch.float32), u.shape[0], int(u.shape[1]), _p(gout, torch.float32, "gout"),
                                  _p(gu, torch.float32), _p(gp, torch.float32), _p(gn, torch.float32), _stream()),
          "srh_bpr_bwd")


def _l2_blocks(xs, gxs=None):
    arr = (_lib.L2Block * len(xs))()
    for k, x in enumerate(xs):
        arr[k].d_x, arr[k].rows, arr[k].cols = _p(x, torch.float32, "emb"), int(x.shape[0]), int(x.shape[1])
        arr[k].d_gx = _p(gxs[k], torch.float32, "grad") if gxs is not None else None
    return arr


def l2_reg_fwd(xs, reg, norms, loss):
    """loss (0-dim f32) = reg * sum_k ||xs[k]||_F / rows_k; norms[k] = ||xs[k]||_F.  1..4 blocks of rows, one launch."""
    check(_lib.load().srh_l2_reg_fwd(_l2_blocks(xs), len(xs), float(reg), scalar_ws(xs[0].device).data_ptr(),
                                     _p(norms, torch.float32), _p(loss, torch.float32), _stream()), "srh_l2_reg_fwd")


def l2_reg_bwd(xs, reg, norms, gout, gxs):
    check(_lib.load().srh_l2_reg_bwd(_l2_blocks(xs, gxs), len(xs), float(reg), _p(norms, torch.float32),
                                     _p(gout, torch.float32, "gout"), _stream()), "srh_l2_reg_bwd")


# SRH_NCE_SPLIT16, SRH_NCE_F32 (include/selfrec_hip.h); "bf16x3" is the round-1/2 name of the split mode, kept as an alias
NCE_PRECISIONS = {"split": 0, "f32": 1, "bf16x3": 0}
NCE_DEFAULT = -1               # SRH_NCE_DEFAULT: the process default (f32 unless srh_infonce_set_precision / SRH_NCE_SPLIT16 says otherwise)


def _nce_mode(precision):
    """None -> the process default; 'split' | 'f32' -> that arithmetic for this call only."""
    if precision is None:
        return NCE_DEFAULT
    if precision not in NCE_PRECISIONS:
        raise SelfrecHipError(f"InfoNCE precision {precision!r}: one of {sorted(NCE_PRECISIONS)}")
    return NCE_PRECISIONS[precision]


def set_infonce_precision(mode: str):
    """'f32' (the default: every multiply-add of InfoNCE's two n x n x d products on the f32 MFMA, the reference's
    arithmetic) or 'split' (operands as short sums of 16-bit pieces on the 16-bit MFMA pipe -- logits on scaled f16 hi + lo,
    accurate to 2^-22 like an f32 dot product; P.V on bf16 pieces: ~10 us per step faster at the Yelp2018 shape).
    The process DEFAULT: what calls that name no precision run on (the loss mirrors of the op-level tier); a trainer
    carries its own mode and passes it with every call (engine.FusedTrainer.nce_precision)."""
    if mode not in NCE_PRECISIONS:
        raise SelfrecHipError(f"InfoNCE precision {mode!r}: one of {sorted(NCE_PRECISIONS)}")
    check(_lib.load().srh_infonce_set_precision(NCE_PRECISIONS[mode]), "srh_infonce_set_precision")


def get_infonce_precision() -> str:
    got = int(_lib.load().srh_infonce_get_precision())
    return {0: "split", 1: "f32"}[got]


NCE_F32_MAX_N = 65536          # the all-f32 passes: 16 key ranges of at most 128 blocks of 32 keys


def infonce_plan(ns, slots: int) -> dict:
    """The task cut of the all-f32 passes for problems of ns live rows on `slots` workgroups (srh_infonce_plan: host only,
    nothing is launched): dict(n, per, splits: one entry per problem; first: len(ns) + 1 running task counts; tasks)."""
    ns = [int(n) for n in ns]
    arr = (C.c_int32 * max(len(ns), 1))(*ns)
    out = (C.c_int32 * 17)()
    check(_lib.load().srh_infonce_plan(C.cast(arr, C.c_void_p), len(ns), int(slots), C.cast(out, C.c_void_p)),
          "srh_infonce_plan")
    k = len(ns)
    return dict(n=list(out[0:k]), per=list(out[4:4 + k]), splits=list(out[8:8 + k]), first=list(out[12:13 + k]),
                tasks=int(out[16]))


def infonce_ws(n: int, d: int, device):
    return torch.empty(int(_lib.load().srh_infonce_ws_bytes(n, d)), dtype=torch.uint8, device=device)


def infonce_fwd_bwd(v1, v2, idx, n, *, n_dev=None, tau, loss_scale, loss, g1, g2, ws):
    d = int(v1.shape[1])
    need = int(_lib.load().srh_infonce_ws_bytes(n, d))
    if ws.numel() * ws.element_size() < need:
        raise SelfrecHipError(f"infonce workspace too small: {ws.numel() * ws.element_size()} < {need}")
    check(_lib.load().srh_infonce_fwd_bwd(_p(v1, torch.float32), _p(v2, torch.float32), _p(idx, torch.int32), int(n),
                                          _p(n_dev, torch.int32), d, float(tau), float(loss_scale),
                                          _p(loss, torch.float64), _p(g1, torch.float32), _p(g2, torch.float32),
                                          _p(ws), _stream()), "srh_infonce_fwd_bwd")


def _infonce_problems(problems, d, ws):
    """[(v1, v2, idx, n_max, n_dev, g1, g2[, g2_exclusive]), ...] -> srh_infonce_problem_t[]; ws must hold them all."""
    lib = _lib.load()
    arr = (_lib.InfonceProblem * len(problems))()
    need = 0
    for k, (v1, v2, idx, n, n_dev, g1, g2, *rest) in enumerate(problems):
        arr[k].d_v1, arr[k].d_v2 = _p(v1, torch.float32), _p(v2, torch.float32)
        arr[k].d_idx, arr[k].n, arr[k].d_n = _p(idx, torch.int32), int(n), _p(n_dev, torch.int32)
        arr[k].d_g1, arr[k].d_g2 = _p(g1, torch.float32), _p(g2, torch.float32)
        arr[k].g2_exclusive = int(bool(rest[0])) if rest else 0
        need += int(lib.srh_infonce_ws_bytes(n, d))
    if ws.numel() * ws.element_size() < need:
        raise SelfrecHipError(f"infonce workspace too small: {ws.numel() * ws.element_size()} < {need}")
    return arr


def infonce_multi(problems, *, d, tau, loss_scale, loss, ws, precision=None):
    """problems: [(v1, v2, idx, n_max, n_dev, g1, g2[, g2_exclusive]), ...] evaluated by one set of launches."""
    lib = _lib.load()
    arr = (_lib.InfonceProblem * len(problems))()
    need = 0
    for k, (v1, v2, idx, n, n_dev, g1, g2, *rest) in enumerate(problems):
        arr[k].d_v1, arr[k].d_v2 = _p(v1, torch.float32), _p(v2, torch.float32)
        arr[k].d_idx, arr[k].n, arr[k].d_n = _p(idx, torch.int32), int(n), _p(n_dev, torch.int32)
        arr[k].d_g1, arr[k].d_g2 = _p(g1, torch.float32), _p(g2, torch.float32)
        arr[k].g2_exclusive = int(bool(rest[0])) if rest else 0
        need += int(lib.srh_infonce_ws_bytes(n, d))
    if ws.numel() * ws.element_size() < need:
        raise SelfrecHipError(f"infonce workspace too small: {ws.numel() * ws.element_size()} < {need}")
    check(lib.srh_infonce_fwd_bwd_multi(arr, len(problems), int(d), float(tau), float(loss_scale),
                                        _p(loss, torch.float64), _p(ws), _nce_mode(precision), _stream()),
          "srh_infonce_fwd_bwd_multi")


def bpr_infonce(user, item, reg_user, reg_item, u_idx, i_idx, j_idx, *, batch, n_rows_dev=None, reg_coef,
                reg_include_neg, loss_scale, g_user, g_item, greg_user, greg_item, losses, bpr_ws,
                problems, tau, cl_scale, cl_loss, nce_ws, precision=None, seg=None, nce_rows=0, staged=False):
    """bpr_l2_fwd_bwd + infonce_multi with their O(batch) kernels sharing launches (srh_bpr_infonce_fwd_bwd).
    seg / nce_rows: the batch's row -> slot lists and how the problems name those rows (srh_batch_segments_t): every
    gradient row is then written once, by the row group that owns it, in slot order -- no float atomics.
    staged: an earlier product of the step carried spmm(..., nce_stage=(problems, nce_ws)) -- no prep launch
    (srh_bpr_infonce_fwd_bwd_staged: all-f32 arithmetic, d = 64 / 128)."""
    lib = _lib.load()
    d = int(user.shape[1])
    b = _bpr_problem(user, item, reg_user, reg_item, u_idx, i_idx, j_idx, batch, n_rows_dev, reg_coef, reg_include_neg,
                     loss_scale, g_user, g_item, greg_user, greg_item, losses, bpr_ws, seg, nce_rows)
    arr = (_lib.InfonceProblem * len(problems))()
    need = 0
    for k, (v1, v2, idx, n, n_dev, g1, g2, *rest) in enumerate(problems):
        arr[k].d_v1, arr[k].d_v2 = _p(v1, torch.float32), _p(v2, torch.float32)
        arr[k].d_idx, arr[k].n, arr[k].d_n = _p(idx, torch.int32), int(n), _p(n_dev, torch.int32)
        arr[k].d_g1, arr[k].d_g2 = _p(g1, torch.float32), _p(g2, torch.float32)
        arr[k].g2_exclusive = int(bool(rest[0])) if rest else 0
        need += int(lib.srh_infonce_ws_bytes(n, d))
    if nce_ws.numel() * nce_ws.element_size() < need:
        raise SelfrecHipError(f"infonce workspace too small: {nce_ws.numel() * nce_ws.element_size()} < {need}")
    if staged:
        if precision != "f32":
            raise SelfrecHipError("bpr_infonce(staged=True): the all-f32 passes only (precision='f32')")
        check(lib.srh_bpr_infonce_fwd_bwd_staged(C.byref(b), arr, len(problems), d, float(tau), float(cl_scale),
                                                 _p(cl_loss, torch.float64), _p(nce_ws), _stream()),
              "srh_bpr_infonce_fwd_bwd_staged")
        return
    check(lib.srh_bpr_infonce_fwd_bwd(C.byref(b), arr, len(problems), d, float(tau), float(cl_scale),
                                      _p(cl_loss, torch.float64), _p(nce_ws), _nce_mode(precision), _stream()),
          "srh_bpr_infonce_fwd_bwd")


# ----------------------------------------------------------------------------------------
# (a-9) optimiser, (a-10/11) evaluation, utilities
# ----------------------------------------------------------------------------------------
def adam_step(param, grad, m, v, *, step=0, step_dev=None, lr, beta1=0.9, beta2=0.999, eps=1e-8, clear=None,
              row_mark=None, advance_cursor=None):
    """clear / row_mark / advance_cursor: the fused end-of-step reset (srh_adam_step_reset)."""
    if clear is not None or advance_cursor is not None:
        clear = list(clear or [])
        tables = (C.c_void_p * max(1, len(clear)))(*[_p(t, torch.float32, "clear") for t in clear])
        check(_lib.load().srh_adam_step_reset(_p(param, torch.float32), _p(grad, torch.float32), _p(m, torch.float32),
                                              _p(v, torch.float32), int(param.shape[0]), int(param.shape[1]),
                                              _p(step_dev, torch.int64), float(lr), float(beta1), float(beta2), float(eps),
                                              _p(row_mark, torch.int32), len(clear), tables,
                                              _p(advance_cursor, torch.int64), _stream()), "srh_adam_step_reset")
        return
    check(_lib.load().srh_adam_step(_p(param, torch.float32), _p(grad, torch.float32), _p(m, torch.float32),
                                    _p(v, torch.float32), param.numel(), int(step), _p(step_dev, torch.int64),
                                    float(lr), float(beta1), float(beta2), float(eps), _stream()), "srh_adam_step")


def score_mask_topk(user_emb, user_ids, item_emb, r_indptr, r_indices, k, scores_ws=None):
    """ids, scores (device, (n_query, k)).  scores_ws: (rows, n_items) slab the queries pass through
    `rows` at a time inside the call (default: one slab for all queries)."""
    nq = int(user_ids.numel()) if user_ids is not None else int(user_emb.shape[0])
    n_items, d = int(item_emb.shape[0]), int(item_emb.shape[1])
    dev = item_emb.device
    if scores_ws is None:
        scores_ws = torch.empty((nq, n_items), dtype=torch.float32, device=dev)
    ids = torch.empty((nq, k), dtype=torch.int32, device=dev)
    sc = torch.empty((nq, k), dtype=torch.float32, device=dev)
    check(_lib.load().srh_score_mask_topk(_p(user_emb, torch.float32), _p(user_ids, torch.int32), nq,
                                          _p(item_emb, torch.float32), n_items, d, _p(r_indptr, torch.int32),
                                          _p(r_indices, torch.int32), int(k), _p(scores_ws, torch.float32),
                                          int(scores_ws.shape[0]), _p(ids, torch.int32), _p(sc, torch.float32),
                                          _stream()), "srh_score_mask_topk")
    return ids, sc


def score_mask_topk_filtered(user_emb, user_ids, item_emb, r_indptr, r_indices, k, *, sample_items=3072, cap=1024,
                             chunk_rows=4096, ws=None):
    """ids, scores, counts (device).  Rows with counts > cap are not valid (see include/selfrec_hip.h):
    rank those with score_mask_topk."""
    lib = _lib.load()
    nq = int(user_ids.numel()) if user_ids is not None else int(user_emb.shape[0])
    n_items, d = int(item_emb.shape[0]), int(item_emb.shape[1])
    dev = item_emb.device
    sample_items = max(int(k), min(int(sample_items), n_items))
    chunk_rows = max(1, min(int(chunk_rows), nq))
    need = int(lib.srh_score_mask_topk_filtered_ws_bytes(chunk_rows, sample_items, int(k), int(cap), n_items, d))
    if ws is None or ws.numel() * ws.element_size() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    ids = torch.empty((nq, k), dtype=torch.int32, device=dev)
    sc = torch.empty((nq, k), dtype=torch.float32, device=dev)
    counts = torch.empty(nq, dtype=torch.int32, device=dev)
    check(lib.srh_score_mask_topk_filtered(_p(user_emb, torch.float32), _p(user_ids, torch.int32), nq,
                                           _p(item_emb, torch.float32), n_items, d, _p(r_indptr, torch.int32),
                                           _p(r_indices, torch.int32), int(k), sample_items, int(cap), chunk_rows,
                                           _p(ws), _p(ids, torch.int32), _p(sc, torch.float32),
                                           _p(counts, torch.int32), _stream()), "srh_score_mask_topk_filtered")
    return ids, sc, counts, ws


def topk_trim_mark_ties(ids_k1, scores_k1):
    """(rows, K + 1) ranked ids / scores -> (rows, K) with rows holding a tie among their K + 1 scores marked ids[:, 0] < 0
    (= -1 - id): one launch (srh_topk_trim_mark_ties)."""
    rows, k1 = int(ids_k1.shape[0]), int(ids_k1.shape[1])
    ids = torch.empty((rows, k1 - 1), dtype=torch.int32, device=ids_k1.device)
    sc = torch.empty((rows, k1 - 1), dtype=torch.float32, device=ids_k1.device)
    check(_lib.load().srh_topk_trim_mark_ties(_p(ids_k1, torch.int32), _p(scores_k1, torch.float32), rows, k1,
                                              _p(ids, torch.int32), _p(sc, torch.float32), _stream()), "srh_topk_trim_mark_ties")
    return ids, sc


def gemm_nt(a, b, out=None):
    m, d = int(a.shape[0]), int(a.shape[1])
    n = int(b.shape[0])
    if out is None:
        out = torch.empty((m, n), dtype=torch.float32, device=a.device)
    check(_lib.load().srh_gemm_nt_f32(_p(a, torch.float32), _p(b, torch.float32), _p(out, torch.float32), m, n, d,
                                      _stream()), "srh_gemm_nt_f32")
    return out


def topk_rows(scores, k):
    rows, n = int(scores.shape[0]), int(scores.shape[1])
    ids = torch.empty((rows, k), dtype=torch.int32, device=scores.device)
    sc = torch.empty((rows, k), dtype=torch.float32, device=scores.device)
    check(_lib.load().srh_topk_rows(_p(scores, torch.float32), rows, n, int(k), _p(ids, torch.int32),
                                    _p(sc, torch.float32), _stream()), "srh_topk_rows")
    return ids, sc


def topk_hit_flags(ids, user_ids, t_indptr, t_indices):
    """uint8 (n_query, k): 1 where the ranked id is one of the user's test items."""
    flags = torch.empty(ids.shape, dtype=torch.uint8, device=ids.device)
    check(_lib.load().srh_topk_hit_flags(_p(ids, torch.int32), int(ids.shape[0]), int(ids.shape[1]),
                                         _p(user_ids, torch.int32), _p(t_indptr, torch.int32),
                                         _p(t_indices, torch.int32), _p(flags, torch.uint8), _stream()),
          "srh_topk_hit_flags")
    return flags


def metric_rows(flags, sizes, cuts):
    """Per-user hits (int32) and DCG / IDCG (float64) at every cut-off of `cuts` (<= 8, each <= K) from the (users, K) hit
    flags and the users' test-set sizes (int32 device tensor): srh_metric_rows.  The gain table and the ideal prefix
    sums are computed HERE with python's math.log exactly as util/evaluation.py:66-78 computes them and handed to the
    kernel, so every quotient is the reference's bit for bit.  Returns (hits, ndcg) of shape (len(cuts), users)."""
    import math
    n, k = int(flags.shape[0]), int(flags.shape[1])
    cuts = [int(c) for c in cuts]
    gains = [1.0 / math.log(pos + 2, 2) for pos in range(k)]
    ideal = np.zeros((len(cuts), k + 1), dtype=np.float64)
    for c, cut in enumerate(cuts):
        acc = 0.0
        for m in range(1, cut + 1):
            acc = acc + 1.0 / math.log(m - 1 + 2, 2)        # sum(... for pos in range(m)): left to right
            ideal[c, m] = acc
    dev = flags.device
    d_gains = torch.tensor(gains, dtype=torch.float64, device=dev)
    d_ideal = torch.from_numpy(ideal).to(dev)
    hits = torch.empty((len(cuts), n), dtype=torch.int32, device=dev)
    ndcg = torch.empty((len(cuts), n), dtype=torch.float64, device=dev)
    arr = (C.c_int32 * len(cuts))(*cuts)
    check(_lib.load().srh_metric_rows(_p(flags, torch.uint8), _p(sizes, torch.int32), n, k, arr, len(cuts),
                                      _p(d_gains, torch.float64), _p(d_ideal, torch.float64), _p(hits, torch.int32),
                                      _p(ndcg, torch.float64), _stream()), "srh_metric_rows")
    return hits, ndcg


def axpby(a, x, b, y):
    check(_lib.load().srh_axpby(float(a), _p(x, torch.float32), float(b), _p(y, torch.float32), x.numel(), _stream()),
          "srh_axpby")
    return y


def cursor_advance(cursor):
    check(_lib.load().srh_cursor_advance(_p(cursor, torch.int64), _stream()), "srh_cursor_advance")


def zero_rows(lists, d, cursor_advance=None):
    """lists: [(table, idx, count_dev_or_None, n_max, row_offset), ...] (at most 8)."""
    n = len(lists)
    vp = C.c_void_p * n
    tables = vp(*[_p(t, torch.float32, "table") for t, *_ in lists])
    idx = vp(*[_p(i, torch.int32, "idx") for _, i, *_ in lists])
    cnt = vp(*[_p(c, torch.int32, "count") for _, _, c, *_ in lists])
    n_max = (C.c_int32 * n)(*[int(m) for *_, m, _ in lists])
    off = (C.c_int32 * n)(*[int(o) for *_, o in lists])
    check(_lib.load().srh_zero_rows(n, tables, idx, cnt, n_max, off, int(d), _p(cursor_advance, torch.int64),
                                    _stream()), "srh_zero_rows")


def batch_fetch_args(ep, n_edges, batch_size, cursor, stage, meta, row_mark=None, mark_item_offset=0, zero4=None,
                     stage_cat=None, cat_item_offset=0, n_cat=None, now=None, half_batches=0, adam_coef=None, adam_lr=0.0,
                     adam_beta1=0.9, adam_beta2=0.999):
    """srh_batch_fetch_args_t.  ep: dict of device int32 arrays for the epoch (two epochs back to back when half_batches >
    0); stage: dict of staging buffers.  adam_coef: float32[2] that receives this step's Adam constants (SRH_EPI_ADAM)."""
    a = _lib.BatchFetchArgs()
    a.d_epoch_u, a.d_epoch_i, a.d_epoch_j = (_p(ep[k], torch.int32) for k in ("u", "i", "j"))
    a.d_epoch_uniq_u, a.d_epoch_uniq_i = _p(ep.get("uniq_u"), torch.int32), _p(ep.get("uniq_i"), torch.int32)
    a.d_n_uniq_u, a.d_n_uniq_i = _p(ep.get("n_uniq_u"), torch.int32), _p(ep.get("n_uniq_i"), torch.int32)
    a.n_edges, a.batch_size, a.d_cursor = int(n_edges), int(batch_size), _p(cursor, torch.int64)
    a.d_stage_u, a.d_stage_i, a.d_stage_j = (_p(stage[k], torch.int32) for k in ("u", "i", "j"))
    a.d_stage_uniq_u, a.d_stage_uniq_i = _p(stage.get("uniq_u"), torch.int32), _p(stage.get("uniq_i"), torch.int32)
    a.d_meta, a.d_row_mark = _p(meta, torch.int32), _p(row_mark, torch.int32)
    a.mark_item_offset, a.cat_item_offset = int(mark_item_offset), int(cat_item_offset)
    a.d_zero4, a.d_stage_cat, a.d_n_cat = _p(zero4, torch.float64), _p(stage_cat, torch.int32), _p(n_cat, torch.int32)
    a.d_now = _p(now, torch.int64)
    a.half_batches = int(half_batches)
    a.d_adam_coef = _p(adam_coef, torch.float32)
    a.adam_lr, a.adam_beta1, a.adam_beta2 = float(adam_lr), float(adam_beta1), float(adam_beta2)
    a._keepalive = [ep, cursor, stage, meta, row_mark, zero4, stage_cat, n_cat, now, adam_coef]
    return a


def batch_fetch(*args, **kwargs):
    """srh_batch_fetch: same arguments as batch_fetch_args (or one prebuilt BatchFetchArgs)."""
    a = args[0] if len(args) == 1 and isinstance(args[0], _lib.BatchFetchArgs) else batch_fetch_args(*args, **kwargs)
    check(_lib.load().srh_batch_fetch(C.byref(a), _stream()), "srh_batch_fetch")


# ----------------------------------------------------------------------------------------
# (e) column-sharded tables: the batch-row exchange around the loss section (csrc/exchange.hip)
# ----------------------------------------------------------------------------------------
def batch_lists(stage, meta, batch_size):
    """struct srh_batch_lists over the staging buffers of batch_fetch: (u, i, j, uniq_u, uniq_i) with
    their device-side counts (meta[0] for the pair lists, meta[1], meta[2])."""
    bl = _lib.BatchLists()
    keep = []
    for s, (name, cnt) in enumerate((("u", 0), ("i", 0), ("j", 0), ("uniq_u", 1), ("uniq_i", 2))):
        c = meta[cnt:cnt + 1]
        bl.d_idx[s] = _p(stage[name], torch.int32, name)
        bl.d_count[s] = _p(c, torch.int32, "count")
        keep += [stage[name], c]
    bl.B = int(batch_size)
    bl._keepalive = keep
    return bl


def _ptr_array(tensors, name):
    return (C.c_void_p * len(tensors))(*[_p(t, torch.float32, name) for t in tensors])


def batch_pack(lists, tables, send, cat_idx=None, n_cat=None):
    dl = int(tables[0].shape[1])
    rows = 5 * lists.B
    if send.numel() < len(tables) * rows * dl or any(int(t.shape[1]) != dl for t in tables):
        raise SelfrecHipError("batch_pack: send buffer too small / tables of different widths")
    check(_lib.load().srh_batch_pack(C.byref(lists), len(tables), _ptr_array(tables, "table"), dl,
                                     _p(send, torch.float32, "send"), _p(cat_idx, torch.int32, "cat_idx"),
                                     _p(n_cat, torch.int32, "n_cat"), _stream()), "srh_batch_pack")


def batch_unpack(lists, recv, world, dl, compact, compact_grads):
    check(_lib.load().srh_batch_unpack(C.byref(lists), len(compact), int(world), int(dl),
                                       _p(recv, torch.float32, "recv"), _ptr_array(compact, "compact"),
                                       len(compact_grads), _ptr_array(compact_grads, "compact_grad") if compact_grads else None,
                                       _stream()), "srh_batch_unpack")


def batch_scatter(lists, pairs, d_full, col0, dl):
    """pairs: [(compact gradient (5B, d_full), local gradient (N, dl)), ...]"""
    check(_lib.load().srh_batch_scatter(C.byref(lists), len(pairs), _ptr_array([c for c, _ in pairs], "compact_grad"),
                                        _ptr_array([g for _, g in pairs], "local_grad"), int(d_full), int(col0), int(dl),
                                        _stream()), "srh_batch_scatter")


# ---- NCL (model/graph/NCL.py): batch rows against a whole table, and the k-means of the E-step ----------------------
TABLE_NCE_WIDTHS = (64, 128)                 # csrc/contrastive.hip / srh_kmeans_assign_f32 (narrower rows: zero-padded)


def table_nce_ws(problems, d: int, device):
    """Workspace for srh_table_nce_fwd_bwd: problems = [(B, N), ...]."""
    lib = _lib.load()
    need = sum(int(lib.srh_table_nce_ws_bytes(int(b), int(n), int(d))) for b, n in problems)
    return torch.empty(need, dtype=torch.uint8, device=device)


def table_nce_fwd_bwd(problems, *, tau, ws=None):
    """InfoNCE of batch rows against a whole table, forward and backward in one call (NCL.py:57-83 ssl_layer_loss).

    problems: [(q, t, idx, loss_scale), ...] (one or two; NCL passes the user side and the item side): q (B x d) the
    gathered query rows, t (N x d) the whole table, idx (B) the positive row of each query in t.  Per problem
        loss = loss_scale * sum_b [ -q_b.t_idx[b] / tau + log sum_j exp(q_b.t_j / tau) ]   (rows F.normalize'd)
    Returns [(loss (0-dim float64), dL/dq (B x d), dL/dt (N x d)), ...], the gradients scaled by loss_scale.  Any d up
    to 128: narrower rows are zero-padded for the kernels, which changes no result."""
    if not 1 <= len(problems) <= 2:
        raise SelfrecHipError("table_nce_fwd_bwd: one or two problems per call")
    d = int(problems[0][0].shape[1])
    w = padded_width(d, TABLE_NCE_WIDTHS)
    if w is None:
        raise SelfrecHipError(f"table_nce_fwd_bwd: rows of {d} columns -- the kernels serve up to {TABLE_NCE_WIDTHS[-1]}")
    dev = problems[0][0].device
    arr = (_lib.TableNceProblem * len(problems))()
    keep, outs, shapes = [], [], []
    for k, (q, t, idx, scale) in enumerate(problems):
        if q.dim() != 2 or t.dim() != 2 or int(q.shape[1]) != d or int(t.shape[1]) != d:
            raise SelfrecHipError("table_nce_fwd_bwd: q and t must be 2-D with the same number of columns")
        if idx.dim() != 1 or int(idx.shape[0]) != int(q.shape[0]):
            raise SelfrecHipError("table_nce_fwd_bwd: idx must hold one entry per query row")
        qp, tp = pad_cols(q.float(), w), pad_cols(t.float(), w)
        ip = idx.to(torch.int32).contiguous()
        B, N = int(qp.shape[0]), int(tp.shape[0])
        loss = torch.empty((), dtype=torch.float64, device=dev)
        gq = torch.empty((B, w), dtype=torch.float32, device=dev)
        gt = torch.empty((N, w), dtype=torch.float32, device=dev)
        arr[k].d_q, arr[k].d_t, arr[k].d_idx = _p(qp, torch.float32, "q"), _p(tp, torch.float32, "t"), _p(ip, torch.int32, "idx")
        arr[k].B, arr[k].N, arr[k].loss_scale = B, N, float(scale)
        arr[k].d_loss, arr[k].d_gq, arr[k].d_gt = _p(loss), _p(gq), _p(gt)
        keep += [qp, tp, ip]
        outs.append((loss, gq, gt))
        shapes.append((B, N))
    need = sum(int(_lib.load().srh_table_nce_ws_bytes(b, n, w)) for b, n in shapes)
    if ws is None or ws.numel() * ws.element_size() < need:
        ws = table_nce_ws(shapes, w, dev)
    check(_lib.load().srh_table_nce_fwd_bwd(arr, len(problems), w, float(tau), _p(ws), _stream()), "srh_table_nce_fwd_bwd")
    return [(loss, gq[:, :d], gt[:, :d]) for loss, gq, gt in outs]


def _km_padded(x, what):
    d = int(x.shape[1])
    w = padded_width(d, TABLE_NCE_WIDTHS)
    if w is None:
        raise SelfrecHipError(f"{what}: rows of {d} columns -- the kernel serves up to {TABLE_NCE_WIDTHS[-1]}")
    return pad_cols(x, w)


def kmeans_assign(x, c):
    """Nearest centroid of every row of x (n x d) among c (k x d) by |c_j|^2 - 2 x.c_j, ties to the lowest j.
    Returns (ids (n,) int32, squared distances (n,) float32)."""
    n, k = int(x.shape[0]), int(c.shape[0])
    if int(c.shape[1]) != int(x.shape[1]):
        raise SelfrecHipError("kmeans_assign: x and c must have the same number of columns")
    xp, cp = _km_padded(x, "kmeans_assign"), _km_padded(c, "kmeans_assign")
    ids = torch.empty(n, dtype=torch.int32, device=x.device)
    dist = torch.empty(n, dtype=torch.float32, device=x.device)
    check(_lib.load().srh_kmeans_assign_f32(_p(xp, torch.float32, "x"), n, _p(cp, torch.float32, "c"), k, int(xp.shape[1]),
                                            _p(ids), _p(dist), _stream()), "srh_kmeans_assign_f32")
    return ids, dist


def kmeans_update(x, ids, k, ws=None):
    """Per-cluster means and counts of the rows of x (n x d) under ids (n,), each cluster summed in ascending row
    order (bit-identical from call to call).  Returns (centroids (k x d) float32, counts (k,) int32); an empty cluster
    has a zero centroid and count 0."""
    n, d = int(x.shape[0]), int(x.shape[1])
    ids = ids.to(torch.int32).contiguous()
    cent = torch.empty((int(k), d), dtype=torch.float32, device=x.device)
    counts = torch.empty(int(k), dtype=torch.int32, device=x.device)
    need = int(_lib.load().srh_kmeans_update_ws_bytes(n, int(k)))
    if ws is None or ws.numel() * ws.element_size() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=x.device)
    check(_lib.load().srh_kmeans_update_f32(_p(x, torch.float32, "x"), n, _p(ids, torch.int32, "ids"), int(k), d, _p(cent),
                                            _p(counts), _p(ws), _stream()), "srh_kmeans_update_f32")
    return cent, counts


KMEANS_MAX_POINTS_PER_CENTROID = 256          # faiss ClusteringParameters.max_points_per_centroid
KMEANS_SPLIT_EPS = 1.0 / 1024.0               # faiss Clustering.cpp split_clusters: EPS


def kmeans_split(centroids, counts):
    """faiss's empty-cluster handling made deterministic (host, in place): every empty cluster, in ascending id, takes
    the largest cluster (lowest id on ties) as its donor, copies its centroid with the +-1/1024 symmetric perturbation
    (even coordinates x(1+eps) on the empty one and x(1-eps) on the donor, odd the other way round) and half its
    count.  centroids: (k, d) float32 numpy, counts: (k,) int64 numpy.  Returns the number of splits."""
    eps = np.float32(KMEANS_SPLIT_EPS)
    up, down = np.float32(1) + eps, np.float32(1) - eps
    nsplit = 0
    for ci in np.flatnonzero(counts == 0):
        if counts[ci] != 0:
            continue
        cj = int(np.argmax(counts))
        centroids[ci] = centroids[cj]
        centroids[ci, 0::2] *= up
        centroids[cj, 0::2] *= down
        centroids[ci, 1::2] *= down
        centroids[cj, 1::2] *= up
        counts[ci] = counts[cj] // 2
        counts[cj] -= counts[ci]
        nsplit += 1
    return nsplit


def kmeans(x, k, niter=25, seed=1234, stats=None):
    """k-means of the rows of x (n x d, on the device) under the defaults of faiss.Kmeans(d, k) as NCL.py:37 uses it,
    with the random choices made deterministic:
      1. perm = np.random.RandomState(seed).permutation(n); n > 256 k: train on rows perm[:256 k]; initial centroids =
         rows perm[:k]
      2. niter times: assign (kmeans_assign), update (kmeans_update), split empty clusters (kmeans_split)
      3. assign all n rows against the final centroids (kmeans.index.search(x, 1))
    Returns (centroids (k, d) float32, assignment (n,) int64), both on the device.  ``stats`` (a dict, optional)
    receives the per-iteration objective (sum of squared distances, before that iteration's update) and the smallest
    count after each update's splits."""
    if x.dim() != 2:
        raise SelfrecHipError("kmeans: x must be 2-D")
    n, k = int(x.shape[0]), int(k)
    if k < 1:
        raise SelfrecHipError("kmeans: k must be >= 1")
    if k > n:
        raise SelfrecHipError(f"kmeans: {n} points are not enough to train {k} centroids (need k <= n)")
    d = int(x.shape[1])
    x = x.detach().float().contiguous()
    xp = _km_padded(x, "kmeans")
    perm = np.random.RandomState(seed).permutation(n)
    if n > KMEANS_MAX_POINTS_PER_CENTROID * k:
        xt = xp.index_select(0, torch.from_numpy(perm[:KMEANS_MAX_POINTS_PER_CENTROID * k]).to(xp.device)).contiguous()
    else:
        xt = xp
    cent = xp.index_select(0, torch.from_numpy(perm[:k]).to(xp.device)).contiguous()
    need = int(_lib.load().srh_kmeans_update_ws_bytes(int(xt.shape[0]), k))
    ws = torch.empty(need, dtype=torch.uint8, device=x.device)
    if stats is not None:
        stats.setdefault("obj", [])
        stats.setdefault("min_count", [])
    for _ in range(int(niter)):
        ids, dist = kmeans_assign(xt, cent)
        if stats is not None:
            stats["obj"].append(float(dist.double().sum()))
        cent, counts = kmeans_update(xt, ids, k, ws)
        counts_h = counts.cpu().numpy().astype(np.int64)
        if (counts_h == 0).any():
            cent_h = cent.cpu().numpy()
            kmeans_split(cent_h, counts_h)
            cent = torch.from_numpy(cent_h).to(x.device)
        if stats is not None:
            stats["min_count"].append(int(counts_h.min()))
    ids, _ = kmeans_assign(xp, cent)
    return cent[:, :d].contiguous(), ids.long()


# ---- UserKNN / ItemKNN (model/graph/UserKNN.py, ItemKNN.py): neighbour lists and their ranking ----------------------
KNN_MAX_K = 128                               # srh_knn_neighbours / srh_knn_score_topk keep their lists in LDS


def knn_neighbours(a_indptr, a_indices, t_indptr, t_indices, norm, name_rank, k, shrinkage, query_rows=None):
    """The best k neighbours of rows of a binary matrix A (UserKNN.py:32-57 / ItemKNN.py:32-56 train()):
    sim = (n / (n + s)) * (n / (norm_q * norm_v + 1e-8)), n the shared features, ordered (sim desc, name_rank desc).
    a_* : A as a CSR (int32 device tensors), t_* : its transpose with ascending rows, norm (float64): sqrt of each row's
    degree, name_rank (int32): each row's place in sorted(names).  query_rows (int32, optional): the rows to serve (all
    when None).  Returns (ids (q, k) int32 -1 padded, sims (q, k) float64 0 padded, lengths (q,) int32)."""
    k, shrinkage = int(k), int(shrinkage)
    if not 1 <= k <= KNN_MAX_K:
        raise SelfrecHipError(f"knn_neighbours: topK = {k} -- the kernels keep at most {KNN_MAX_K} neighbours per row")
    if shrinkage < 0:
        raise SelfrecHipError(f"knn_neighbours: negative shrinkage {shrinkage}")
    if shrinkage >= 2 ** 31:
        raise SelfrecHipError(f"knn_neighbours: shrinkage {shrinkage} -- the entry point takes a 32-bit value, below 2**31")
    n_rows = int(a_indptr.numel()) - 1
    if n_rows < 1 or int(norm.numel()) != n_rows or int(name_rank.numel()) != n_rows:
        raise SelfrecHipError("knn_neighbours: a_indptr, norm and name_rank must describe the same rows")
    ptrs = (_p(a_indptr, torch.int32, "a_indptr"), _p(a_indices, torch.int32, "a_indices"),
            _p(t_indptr, torch.int32, "t_indptr"), _p(t_indices, torch.int32, "t_indices"),
            _p(norm, torch.float64, "norm"), _p(name_rank, torch.int32, "name_rank"))
    if query_rows is not None:
        _p(query_rows, torch.int32, "query_rows")
        n_query = int(query_rows.numel())
        if n_query < 1 or int(query_rows.min()) < 0 or int(query_rows.max()) >= n_rows:
            raise SelfrecHipError(f"knn_neighbours: query rows must lie in [0, {n_rows})")
    else:
        n_query = n_rows
    dev = a_indptr.device
    ids = torch.empty((n_query, k), dtype=torch.int32, device=dev)
    sims = torch.empty((n_query, k), dtype=torch.float64, device=dev)
    lens = torch.empty(n_query, dtype=torch.int32, device=dev)
    check(_lib.load().srh_knn_neighbours(*ptrs, n_rows, _p(query_rows), n_query, k, shrinkage, _p(ids), _p(sims), _p(lens),
                                         _stream()), "srh_knn_neighbours")
    return ids, sims, lens


def knn_score_ws(ws_rows, n_items, device):
    """Workspace of srh_knn_score_topk: ws_rows float64 score rows."""
    return torch.empty(int(_lib.load().srh_knn_score_ws_bytes(int(ws_rows), int(n_items))), dtype=torch.uint8, device=device)


def knn_score_topk(mode, users, r_indptr, r_indices, n_items, nbr_ids, nbr_sims, nbr_len, n_top, ws_rows=1024, ws=None,
                   mask_train=True):
    """Masked float64 score rows of the given users and their best n_top items (UserKNN.py:59-81 with mode "user",
    ItemKNN.py:58-81 with mode "item", ranked as base/graph_recommender.py:44-58 ranks them; mask_train=False leaves
    the training items as predict() returns them).

    r_indptr / r_indices: users x items, each user's items in training-file order.  nbr_*: the neighbour lists of
    knn_neighbours (over users for "user", over items for "item").  Returns (ids (q, n_top) int32, scores (q, n_top)
    float64, ws): ranked (score desc, id asc); a row whose n_top + 1 best hold two equal neighbours is marked
    ids[row, 0] = -1 - id and is to be redone in the reference's heap order (find_k_largest_host_f64).  When the users
    fit in ws_rows, ws.view(float64)[:q * n_items] holds their finished score rows after the call."""
    if mode not in ("user", "item"):
        raise SelfrecHipError(f"knn_score_topk: mode {mode!r} (user or item)")
    k_nbr, n_top, n_items = int(nbr_ids.shape[1]), int(n_top), int(n_items)
    if not 1 <= k_nbr <= KNN_MAX_K:
        raise SelfrecHipError(f"knn_score_topk: topK = {k_nbr} -- the kernels keep at most {KNN_MAX_K} neighbours per row")
    if not (n_top >= 1 and n_top + 1 <= min(KNN_MAX_K, n_items)):
        raise SelfrecHipError(f"knn_score_topk: N = {n_top} needs N + 1 <= min({KNN_MAX_K}, {n_items} items)")
    n_query = int(users.numel())
    n_users = int(r_indptr.numel()) - 1
    n_rows = n_users if mode == "user" else n_items
    if int(nbr_ids.shape[0]) != n_rows or int(nbr_len.numel()) != n_rows or tuple(nbr_sims.shape) != tuple(nbr_ids.shape):
        raise SelfrecHipError(f"knn_score_topk: {mode} mode wants neighbour lists of {n_rows} rows")
    ptrs = (_p(users, torch.int32, "users"), _p(r_indptr, torch.int32, "r_indptr"), _p(r_indices, torch.int32, "r_indices"),
            _p(nbr_ids, torch.int32, "nbr_ids"), _p(nbr_sims, torch.float64, "nbr_sims"), _p(nbr_len, torch.int32, "nbr_len"))
    if n_query < 1 or int(users.min()) < 0 or int(users.max()) >= n_users:
        raise SelfrecHipError(f"knn_score_topk: user ids must lie in [0, {n_users})")
    ws_rows = max(1, min(int(ws_rows), n_query))
    need = int(_lib.load().srh_knn_score_ws_bytes(ws_rows, n_items))
    if ws is None or ws.numel() * ws.element_size() < need:
        ws = knn_score_ws(ws_rows, n_items, users.device)
    ws_rows = (ws.numel() * ws.element_size()) // (8 * n_items)
    dev = users.device
    ids = torch.empty((n_query, n_top), dtype=torch.int32, device=dev)
    sc = torch.empty((n_query, n_top), dtype=torch.float64, device=dev)
    check(_lib.load().srh_knn_score_topk(0 if mode == "user" else 1, ptrs[0], n_query, ptrs[1], ptrs[2], n_items, ptrs[3],
                                         ptrs[4], ptrs[5], k_nbr, n_top, int(bool(mask_train)), _p(ws), int(ws_rows), _p(ids),
                                         _p(sc), _stream()),
          "srh_knn_score_topk")
    return ids, sc, ws


# ---- SSL4Rec: the MLP towers (csrc/ssl4rec.hip) and batch_softmax_loss (csrc/contrastive.hip) --------------------------
TOWER_IN, TOWER_HIDDEN, TOWER_OUT = 64, 1024, 128


def _tower_weights(w1, b1, w2, b2):
    shapes = ((w1, (TOWER_HIDDEN, TOWER_IN)), (b1, (TOWER_HIDDEN,)), (w2, (TOWER_OUT, TOWER_HIDDEN)), (b2, (TOWER_OUT,)))
    for t, shape in shapes:
        if tuple(t.shape) != shape:
            raise SelfrecHipError(f"tower: weight of shape {tuple(t.shape)}, expected {shape} (Linear(64, 1024) -> ReLU -> "
                                  f"Linear(1024, 128) -> Tanh)")
    return _lib.TowerWeights(_p(w1, torch.float32, "w1"), _p(b1, torch.float32, "b1"), _p(w2, torch.float32, "w2"),
                             _p(b2, torch.float32, "b2"))


def tower_fwd(table, idx, w1, b1, w2, b2, *, mask_row0=None, mask=None, drop_p=0.0, rng_seed=0, rng_counter=0,
              save=True):
    """DNN_Encoder's tower (SSL4Rec.py:66-77) over rows table[idx] (table itself when idx is None): (y (n x 128),
    saved) with saved = (x, hidden, keep) for tower_bwd, or None when save is False.

    Rows r >= mask_row0 take nn.Dropout(drop_p): ``mask`` (uint8 (n - mask_row0, 64), 1 = keep) replays given masks;
    without it keep is drawn in-kernel at counter rng_counter + (r - mask_row0) (include/selfrec_hip.h) and returned in
    saved[2].  mask_row0 None: no dropout."""
    if table.dim() != 2 or int(table.shape[1]) != TOWER_IN:
        raise SelfrecHipError(f"tower: rows of {TOWER_IN} columns expected, got {tuple(table.shape)}")
    n = int(table.shape[0]) if idx is None else int(idx.numel())
    if n < 1:
        raise SelfrecHipError("tower: no rows")
    dev = table.device
    row0 = n if mask_row0 is None else int(mask_row0)
    n_mask = n - row0
    if mask is not None and tuple(mask.shape) != (n_mask, TOWER_IN):
        raise SelfrecHipError(f"tower: mask of shape {tuple(mask.shape)}, expected {(n_mask, TOWER_IN)}")
    ip = None if idx is None else idx.to(torch.int32).contiguous()
    w = _tower_weights(w1, b1, w2, b2)
    y = torch.empty((n, TOWER_OUT), dtype=torch.float32, device=dev)
    x = hidden = keep = None
    if save:
        x = torch.empty((n, TOWER_IN), dtype=torch.float32, device=dev)
        hidden = torch.empty((n, TOWER_HIDDEN), dtype=torch.float32, device=dev)
        if n_mask > 0:
            keep = mask.contiguous() if mask is not None else torch.empty((n_mask, TOWER_IN), dtype=torch.uint8, device=dev)
    mask_in = None if (mask is None or n_mask == 0) else mask.contiguous()
    mask_out = keep if (save and n_mask > 0 and mask is None) else None
    check(_lib.load().srh_tower_fwd_f32(_p(table, torch.float32, "table"), _p(ip, torch.int32, "idx"), n,
                                        int(table.shape[0]), C.byref(w), row0, _p(mask_in, torch.uint8, "mask"),
                                        int(rng_seed) & 0xFFFFFFFFFFFFFFFF, int(rng_counter) & 0xFFFFFFFFFFFFFFFF,
                                        float(drop_p if n_mask > 0 else 0.0), _p(mask_out), _p(x), _p(hidden), _p(y),
                                        _stream()),
          "srh_tower_fwd_f32")
    return y, ((x, hidden, keep) if save else None)


def tower_bwd(saved, y, gy, w1, b1, w2, b2, *, mask_row0=None, drop_p=0.0, ws=None):
    """Gradients of tower_fwd: (dX (n x 64, w.r.t. the gathered rows), dW1, db1, dW2, db2), every reduction over rows in
    a fixed order."""
    x, hidden, keep = saved
    n = int(x.shape[0])
    row0 = n if mask_row0 is None else int(mask_row0)
    dev = x.device
    w = _tower_weights(w1, b1, w2, b2)
    need = int(_lib.load().srh_tower_bwd_ws_bytes(n))
    if ws is None or ws.numel() * ws.element_size() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    gx = torch.empty((n, TOWER_IN), dtype=torch.float32, device=dev)
    gw1, gb1 = torch.empty_like(w1), torch.empty_like(b1)
    gw2, gb2 = torch.empty_like(w2), torch.empty_like(b2)
    gy = gy.to(torch.float32).contiguous()
    check(_lib.load().srh_tower_bwd_f32(_p(x), _p(hidden), _p(y, torch.float32, "y"), _p(gy, torch.float32, "gy"), n,
                                        C.byref(w), row0, _p(keep, torch.uint8, "mask"),
                                        float(drop_p if keep is not None else 0.0), _p(gx), _p(gw1), _p(gb1), _p(gw2),
                                        _p(gb2), _p(ws), _stream()),
          "srh_tower_bwd_f32")
    return gx, gw1, gb1, gw2, gb2


def scatter_plan(ids, device):
    """The segments of srh_rows_segment_sum_f32 for gathered-row ids (host array): a stable sort of the rows by id, so
    each table row sums its rows in ascending row order.  -> (order, seg_start, seg_row) int32 device tensors."""
    to = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
    return tuple(to(a) for a in scatter_plan_host(ids))


def scatter_plan_host(ids):
    """scatter_plan's three int32 arrays on the host, for a caller that uploads them with its batch"""
    ids = np.ascontiguousarray(np.asarray(ids).reshape(-1), dtype=np.int64)
    order = np.argsort(ids, kind="stable")
    s = ids[order]
    first = np.flatnonzero(np.r_[True, s[1:] != s[:-1]]) if s.size else np.zeros(0, dtype=np.int64)
    seg_start = np.r_[first, s.size].astype(np.int32)
    seg_row = s[first].astype(np.int32)
    return tuple(np.ascontiguousarray(a, dtype=np.int32) for a in (order, seg_start, seg_row))


def rows_segment_sum(x, plan, out):
    """out[row] += the rows of x that plan (scatter_plan) names for it, in plan order: a deterministic index_add_."""
    order, seg_start, seg_row = plan
    n_rows, d = int(x.shape[0]), int(x.shape[1])
    if int(order.numel()) != n_rows or int(out.shape[1]) != d:
        raise SelfrecHipError("rows_segment_sum: the plan and the tables do not match")
    if int(seg_row.numel()) == 0:          # no segments: nothing to add (an empty tensor has no address to hand over)
        return out
    check(_lib.load().srh_rows_segment_sum_f32(_p(x.contiguous(), torch.float32, "x"), n_rows, d,
                                               _p(order, torch.int32, "order"), _p(seg_start, torch.int32, "seg_start"),
                                               _p(seg_row, torch.int32, "seg_row"), int(seg_row.numel()),
                                               int(out.shape[0]), _p(out, torch.float32, "out"), _stream()),
          "srh_rows_segment_sum_f32")
    return out


def batch_softmax_fwd_bwd(u, v, tau, ws=None):
    """batch_softmax_loss (util/loss_torch.py:25-32) and its gradients: (loss (0-dim float64), dL/du, dL/dv).  Rows up to
    128 columns (narrower ones zero-padded: no result changes)."""
    if u.dim() != 2 or u.shape != v.shape:
        raise SelfrecHipError("batch_softmax: u and v must be 2-D of the same shape")
    B, d = int(u.shape[0]), int(u.shape[1])
    w = padded_width(d, TABLE_NCE_WIDTHS)
    if w is None:
        raise SelfrecHipError(f"batch_softmax: rows of {d} columns -- the kernel serves up to {TABLE_NCE_WIDTHS[-1]}")
    up, vp = pad_cols(u.float(), w), pad_cols(v.float(), w)
    dev = u.device
    need = int(_lib.load().srh_batch_softmax_ws_bytes(B, w))
    if ws is None or ws.numel() * ws.element_size() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    loss = torch.empty((), dtype=torch.float64, device=dev)
    gu = torch.empty((B, w), dtype=torch.float32, device=dev)
    gv = torch.empty((B, w), dtype=torch.float32, device=dev)
    check(_lib.load().srh_batch_softmax_fwd_bwd(_p(up, torch.float32, "u"), _p(vp, torch.float32, "v"), B, w, float(tau),
                                                _p(loss), _p(gu), _p(gv), _p(ws), _stream()),
          "srh_batch_softmax_fwd_bwd")
    return loss, gu[:, :d], gv[:, :d]


class BatchSoftmaxFn(torch.autograd.Function):
    """batch_softmax_loss as one kernel call: loss and both gradients come out together; backward() scales them."""

    @staticmethod
    def forward(ctx, u, v, tau):
        loss, gu, gv = batch_softmax_fwd_bwd(u, v, tau)
        ctx.save_for_backward(gu, gv)
        return loss.to(torch.float32)

    @staticmethod
    def backward(ctx, gout):
        gu, gv = ctx.saved_tensors
        return gu * gout, gv * gout, None


class TowerFn(torch.autograd.Function):
    """y = tower(table[idx]) with the gradient of the WHOLE table (zero outside the rows idx names; repeated ids summed in
    ascending row order by ``plan`` = scatter_plan(idx)) and of the four weight tensors.  ``keep_out`` (optional list)
    receives the dropout keep mask the forward used."""

    @staticmethod
    def forward(ctx, table, w1, b1, w2, b2, idx, plan, mask_row0, mask, drop_p, rng_seed, rng_counter, keep_out):
        y, saved = tower_fwd(table, idx, w1, b1, w2, b2, mask_row0=mask_row0, mask=mask, drop_p=drop_p,
                             rng_seed=rng_seed, rng_counter=rng_counter)
        if keep_out is not None:
            keep_out.append(saved[2])
        ctx.save_for_backward(table, w1, b1, w2, b2, y)
        ctx.x, ctx.hidden, ctx.keep, ctx.idx, ctx.plan, ctx.mask_row0, ctx.drop_p = (*saved, idx, plan, mask_row0, drop_p)
        return y

    @staticmethod
    def backward(ctx, gy):
        table, w1, b1, w2, b2, y = ctx.saved_tensors
        gx, gw1, gb1, gw2, gb2 = tower_bwd((ctx.x, ctx.hidden, ctx.keep), y, gy, w1, b1, w2, b2, mask_row0=ctx.mask_row0,
                                           drop_p=ctx.drop_p)
        if ctx.idx is None:
            gt = gx
        else:
            plan = ctx.plan if ctx.plan is not None else scatter_plan(ctx.idx.cpu().numpy(), table.device)
            gt = rows_segment_sum(gx, plan, torch.zeros_like(table))
        return gt, gw1, gb1, gw2, gb2, None, None, None, None, None, None, None, None


# ---- SASRec (csrc/seqrec.hip) ------------------------------------------------------------------------------------------
SEQ_ATTN_MAX_LEN = 64                         # srh_seq_attn_*: L <= 64, dh in SEQ_ATTN_HEAD_WIDTHS, H dh <= 128
SEQ_ATTN_HEAD_WIDTHS = (32, 64)
SEQ_ATTN_MAX_WIDTH = 128


def seq_attn_supported(L: int, H: int, dh: int) -> bool:
    """whether (L, H, dh) is inside the fused attention kernel's envelope (include/selfrec_hip.h)"""
    return 1 <= L <= SEQ_ATTN_MAX_LEN and dh in SEQ_ATTN_HEAD_WIDTHS and 1 <= H and H * dh <= SEQ_ATTN_MAX_WIDTH


def _attn_shape(q, k, v, n_heads):
    if q.dim() != 3 or q.shape != k.shape or q.shape != v.shape:
        raise SelfrecHipError("seq_attn: q, k, v must be (B, L, H * dh) tensors of one shape")
    B, L, E = (int(s) for s in q.shape)
    H = int(n_heads)
    if H < 1 or E % H:
        raise SelfrecHipError(f"seq_attn: width {E} does not split into {H} heads")
    return B, L, H, E // H


def _attn_keep(keep, B, H, L):
    if keep is None:
        return None
    if tuple(keep.shape) != (B, H, L, L):
        raise SelfrecHipError(f"seq_attn: keep mask of shape {tuple(keep.shape)}, expected {(B, H, L, L)}")
    return keep.to(torch.uint8).contiguous()


def _seq_attn_fwd(entry, q, k, v, n_heads, keep, drop_p, rng_seed, rng_counter):
    B, L, H, dh = _attn_shape(q, k, v, n_heads)
    keep = _attn_keep(keep, B, H, L)
    out = torch.empty_like(q)
    lse = torch.empty((B, H, L), dtype=torch.float32, device=q.device)
    check(getattr(_lib.load(), entry)(_p(q, torch.float32, "q"), _p(k, torch.float32, "k"), _p(v, torch.float32, "v"),
                                      B, L, H, dh, _p(keep, torch.uint8, "keep"),
                                      int(rng_seed) & 0xFFFFFFFFFFFFFFFF, int(rng_counter) & 0xFFFFFFFFFFFFFFFF,
                                      float(drop_p), _p(out), _p(lse), _stream()), entry)
    return out, lse


def _seq_attn_bwd(entry, q, k, v, lse, go, n_heads, keep, drop_p, rng_seed, rng_counter):
    B, L, H, dh = _attn_shape(q, k, v, n_heads)
    keep = _attn_keep(keep, B, H, L)
    go = go.to(torch.float32).contiguous()
    gq, gk, gv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    check(getattr(_lib.load(), entry)(_p(q, torch.float32, "q"), _p(k, torch.float32, "k"), _p(v, torch.float32, "v"),
                                      _p(go, torch.float32, "go"), _p(lse, torch.float32, "lse"), B, L, H, dh,
                                      _p(keep, torch.uint8, "keep"), int(rng_seed) & 0xFFFFFFFFFFFFFFFF,
                                      int(rng_counter) & 0xFFFFFFFFFFFFFFFF, float(drop_p), _p(gq), _p(gk), _p(gv),
                                      _stream()), entry)
    return gq, gk, gv


def seq_attn_fwd(q, k, v, n_heads, *, keep=None, drop_p=0.0, rng_seed=0, rng_counter=0):
    """Causal attention of projected q, k, v (B, L, H * dh): (out (B, L, H * dh), lse (B, H, L)).  Dropout on the
    probabilities: ``keep`` ((B, H, L, L), 1 = keep) replays a given mask; without it and with drop_p > 0 the mask is
    drawn in-kernel at the counters [rng_counter, rng_counter + B * H * L) (include/selfrec_hip.h)."""
    return _seq_attn_fwd("srh_seq_attn_fwd_f32", q, k, v, n_heads, keep, drop_p, rng_seed, rng_counter)


def seq_attn_bwd(q, k, v, lse, go, n_heads, *, keep=None, drop_p=0.0, rng_seed=0, rng_counter=0):
    """(dq, dk, dv) of seq_attn_fwd for the upstream gradient go, with the forward's dropout arguments."""
    return _seq_attn_bwd("srh_seq_attn_bwd_f32", q, k, v, lse, go, n_heads, keep, drop_p, rng_seed, rng_counter)


def seq_attn_full_fwd(q, k, v, n_heads, *, keep=None, drop_p=0.0, rng_seed=0, rng_counter=0):
    """seq_attn_fwd without a mask: every query attends to all L positions (BERT4Rec).  The same arguments, outputs
    and dropout contract."""
    return _seq_attn_fwd("srh_seq_attn_full_fwd_f32", q, k, v, n_heads, keep, drop_p, rng_seed, rng_counter)


def seq_attn_full_bwd(q, k, v, lse, go, n_heads, *, keep=None, drop_p=0.0, rng_seed=0, rng_counter=0):
    """(dq, dk, dv) of seq_attn_full_fwd for the upstream gradient go, with the forward's dropout arguments."""
    return _seq_attn_bwd("srh_seq_attn_full_bwd_f32", q, k, v, lse, go, n_heads, keep, drop_p, rng_seed, rng_counter)


class _SeqAttn(torch.autograd.Function):
    """the fused attention core as one differentiable op of (q, k, v): causal (seq_attn_fwd / seq_attn_bwd) or over all
    positions (seq_attn_full_fwd / seq_attn_full_bwd)"""

    @staticmethod
    def forward(ctx, causal, q, k, v, n_heads, keep, drop_p, rng_seed, rng_counter):
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        ctx.fwd_bwd = (seq_attn_fwd, seq_attn_bwd) if causal else (seq_attn_full_fwd, seq_attn_full_bwd)
        ctx.args = dict(keep=keep, drop_p=drop_p, rng_seed=rng_seed, rng_counter=rng_counter)
        out, lse = ctx.fwd_bwd[0](q, k, v, n_heads, **ctx.args)
        ctx.save_for_backward(q, k, v, lse)
        ctx.n_heads = n_heads
        return out

    @staticmethod
    def backward(ctx, go):
        q, k, v, lse = ctx.saved_tensors
        gq, gk, gv = ctx.fwd_bwd[1](q, k, v, lse, go, ctx.n_heads, **ctx.args)
        return None, gq, gk, gv, None, None, None, None, None


class SeqAttnFn:
    """seq_attn_fwd / seq_attn_bwd as one differentiable op of (q, k, v)."""
    apply = staticmethod(functools.partial(_SeqAttn.apply, True))


class SeqAttnFullFn:
    """seq_attn_full_fwd / seq_attn_full_bwd as one differentiable op of (q, k, v)."""
    apply = staticmethod(functools.partial(_SeqAttn.apply, False))


def seq_bce_fwd_bwd(hidden, table, pos, neg, valid, n_valid=None, ws=None):
    """SASRec.calculate_loss over hidden rows (R x d): (loss2 (2,) float64: the positive and the negative
    BCE-with-logits means over the rows with valid != 0, dL/dhidden (R x d), per-row table gradients (2R x d: rows of
    pos, then of neg)).  pos / neg: int32 item ids, valid: uint8, all of R entries on the device."""
    if hidden.dim() != 2 or table.dim() != 2 or hidden.shape[1] != table.shape[1]:
        raise SelfrecHipError("seq_bce: hidden (R x d) and table (n x d) expected")
    R, d = int(hidden.shape[0]), int(hidden.shape[1])
    for t, name in ((pos, "pos"), (neg, "neg"), (valid, "valid")):
        if int(t.numel()) != R:
            raise SelfrecHipError(f"seq_bce: {name} has {int(t.numel())} entries, expected {R}")
    if n_valid is None:
        n_valid = int(valid.count_nonzero().item())
    dev = hidden.device
    need = int(_lib.load().srh_seq_bce_ws_bytes(R))
    if ws is None or ws.numel() * ws.element_size() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    loss2 = torch.empty(2, dtype=torch.float64, device=dev)
    gh = torch.empty((R, d), dtype=torch.float32, device=dev)
    grows = torch.empty((2 * R, d), dtype=torch.float32, device=dev)
    check(_lib.load().srh_seq_bce_fwd_bwd(_p(hidden, torch.float32, "hidden"), R, d, _p(table, torch.float32, "table"),
                                          int(table.shape[0]), _p(pos, torch.int32, "pos"), _p(neg, torch.int32, "neg"),
                                          _p(valid, torch.uint8, "valid"), int(n_valid), _p(loss2), _p(gh), _p(grows),
                                          _p(ws), _stream()), "srh_seq_bce_fwd_bwd")
    return loss2, gh, grows


class SeqBceFn(torch.autograd.Function):
    """The two BCE means of SASRec.calculate_loss as one kernel call; the item table's gradient is the deterministic
    segment sum of the per-row gradients (``plan`` = scatter_plan([pos; neg]))."""

    @staticmethod
    def forward(ctx, hidden, table, pos, neg, valid, n_valid, plan):
        loss2, gh, grows = seq_bce_fwd_bwd(hidden.contiguous(), table, pos, neg, valid, n_valid)
        ctx.save_for_backward(gh, grows)
        ctx.plan, ctx.table_shape = plan, tuple(table.shape)
        return (loss2[0].to(torch.float32) + loss2[1].to(torch.float32))

    table_grad = staticmethod(rows_segment_sum)

    @classmethod
    def backward(cls, ctx, gout):
        gh, grows = ctx.saved_tensors
        gt = cls.table_grad(grows, ctx.plan, torch.zeros(ctx.table_shape, dtype=torch.float32, device=gh.device))
        return gh * gout, gt * gout, None, None, None, None, None


class GatherRowsFn(torch.autograd.Function):
    """table[idx] whose table gradient is the deterministic segment sum (``plan`` = scatter_plan(idx)) instead of an
    atomic index_add."""

    @staticmethod
    def forward(ctx, table, idx, plan):
        ctx.plan, ctx.table_shape = plan, tuple(table.shape)
        return table[idx.long()]

    @staticmethod
    def backward(ctx, g):
        g2 = g.reshape(-1, ctx.table_shape[1]).to(torch.float32).contiguous()
        return rows_segment_sum(g2, ctx.plan, torch.zeros(ctx.table_shape, dtype=torch.float32, device=g.device)), None, None


# ---- BERT4Rec (csrc/contrastive.hip: the table cross-entropy) -------------------------------------------------------------
def table_ce_fwd_bwd(hidden_rows, table, labels, loss_scale=1.0, ws=None):
    """Softmax cross-entropy of the rows (M x d) against the whole table (N x d), logits h_m . t_j:
    (loss (0-dim float64) = loss_scale * sum_m (lse_m - s_{m, label_m}), dL/dhidden_rows (M x d), dL/dtable (N x d, dense)).
    labels: int32 device tensor of M entries in [0, N).  The M x N logits are never materialised.  Rows up to 128 columns
    (narrower ones zero-padded: no result changes)."""
    if hidden_rows.dim() != 2 or table.dim() != 2 or hidden_rows.shape[1] != table.shape[1]:
        raise SelfrecHipError("table_ce: rows (M x d) and table (N x d) expected")
    M, d = int(hidden_rows.shape[0]), int(hidden_rows.shape[1])
    N = int(table.shape[0])
    if int(labels.numel()) != M:
        raise SelfrecHipError(f"table_ce: labels has {int(labels.numel())} entries, expected {M}")
    w = padded_width(d, TABLE_NCE_WIDTHS)
    if w is None:
        raise SelfrecHipError(f"table_ce: rows of {d} columns -- the kernel serves up to {TABLE_NCE_WIDTHS[-1]}")
    _p(hidden_rows, None, "hidden_rows"), _p(table, None, "table")
    hp, tp = pad_cols(hidden_rows.float(), w).contiguous(), pad_cols(table.float(), w).contiguous()
    dev = hidden_rows.device
    need = int(_lib.load().srh_table_ce_ws_bytes(M, N, w))
    if ws is None or ws.numel() * ws.element_size() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    loss = torch.empty((), dtype=torch.float64, device=dev)
    gh = torch.empty((M, w), dtype=torch.float32, device=dev)
    gt = torch.empty((N, w), dtype=torch.float32, device=dev)
    check(_lib.load().srh_table_ce_fwd_bwd(_p(hp, torch.float32, "hidden_rows"), M, _p(tp, torch.float32, "table"), N, w,
                                           _p(labels, torch.int32, "labels"), float(loss_scale), _p(loss), _p(gh), _p(gt),
                                           _p(ws), _stream()), "srh_table_ce_fwd_bwd")
    return loss, (gh if w == d else gh[:, :d]), (gt if w == d else gt[:, :d])


class TableCeFn(torch.autograd.Function):
    """table_ce_fwd_bwd as one differentiable op of (hidden_rows, table): loss and both gradients come out of the one
    call; backward() scales them by the upstream scalar."""

    @staticmethod
    def forward(ctx, hidden_rows, table, labels, loss_scale):
        loss, gh, gt = table_ce_fwd_bwd(hidden_rows, table, labels, loss_scale)
        ctx.save_for_backward(gh, gt)
        return loss.to(torch.float32)

    @staticmethod
    def backward(ctx, gout):
        gh, gt = ctx.saved_tensors
        return gh * gout, gt * gout, None, None


# ---- CL4SRec (csrc/seqrec.hip: the embedding front and the live-row table gradient) ---------------------------------------
SEQ_EMBED_WIDTHS = (32, 64, 128)              # srh_seq_embed_fwd_f32 / srh_rows_live_sum_f32
LIVE_SUM_CHUNK = 32                           # SRH_LIVE_SUM_CHUNK
LIVE_SUM_MAX_PROBLEMS = 3                     # SRH_LIVE_SUM_MAX_PROBLEMS
_U64 = 0xFFFFFFFFFFFFFFFF


def seq_embed_supported(d: int) -> bool:
    return int(d) in SEQ_EMBED_WIDTHS


def seq_embed_fwd(item, pos_table, seq, posid, *, scale=None, keep=None, drop_p=0.0, rng_seed=0, rng_counter=0):
    """(R x d) rows (item[seq[r]] * scale + pos_table[posid[r]]) * m(r) for the rows with seq[r] != 0, exact zeros for the
    others (include/selfrec_hip.h (a-18)).  seq / posid: int32 device tensors of R entries; scale defaults to sqrt(d);
    ``keep`` ((R, d), 1 = keep) replays a dropout mask, without it and with drop_p > 0 the mask is drawn in-kernel at the
    counters [rng_counter, rng_counter + R)."""
    if item.dim() != 2 or pos_table.dim() != 2 or item.shape[1] != pos_table.shape[1]:
        raise SelfrecHipError("seq_embed: item (n x d) and position (m x d) tables expected")
    R, d = int(seq.numel()), int(item.shape[1])
    if int(posid.numel()) != R or R < 1:
        raise SelfrecHipError(f"seq_embed: {R} item ids and {int(posid.numel())} position ids")
    if keep is not None:
        if int(keep.numel()) != R * d:
            raise SelfrecHipError(f"seq_embed: keep mask of {int(keep.numel())} entries, expected {R} x {d}")
        keep = keep.to(torch.uint8).contiguous()
    out = torch.empty((R, d), dtype=torch.float32, device=item.device)
    check(_lib.load().srh_seq_embed_fwd_f32(_p(item, torch.float32, "item"), int(item.shape[0]),
                                            _p(pos_table, torch.float32, "pos_table"), int(pos_table.shape[0]),
                                            _p(seq, torch.int32, "seq"), _p(posid, torch.int32, "posid"), R, d,
                                            float(d ** 0.5 if scale is None else scale), _p(keep, torch.uint8, "keep"),
                                            int(rng_seed) & _U64, int(rng_counter) & _U64, float(drop_p), _p(out),
                                            _stream()), "srh_seq_embed_fwd_f32")
    return out


def live_plan_host(ids, live=None, chunk=LIVE_SUM_CHUNK):
    """The plan of srh_rows_live_sum_f32 for gathered-row ids (host array): the rows with ``live`` (default ids != 0)
    sorted stably by id, every id's segment cut into chunks of at most ``chunk`` rows.
    -> (rows, chunk_start, chunk_dst, multi_range, multi_row) int32 host arrays (include/selfrec_hip.h (a-18))."""
    ids = np.ascontiguousarray(np.asarray(ids).reshape(-1), dtype=np.int64)
    live = ids != 0 if live is None else np.asarray(live).reshape(-1).astype(bool)
    rows = np.flatnonzero(live)
    rows = rows[np.argsort(ids[rows], kind="stable")]
    s = ids[rows]
    first = np.flatnonzero(np.r_[True, s[1:] != s[:-1]]) if s.size else np.zeros(0, dtype=np.int64)
    length = np.diff(np.r_[first, s.size])
    n_chunks = (length + chunk - 1) // chunk                                     # chunks per segment
    chunk0 = np.r_[0, np.cumsum(n_chunks)].astype(np.int64)                      # first chunk of each segment
    seg_of_chunk = np.repeat(np.arange(first.size), n_chunks)
    within = np.arange(int(chunk0[-1])) - chunk0[seg_of_chunk]
    chunk_start = np.r_[first[seg_of_chunk] + within * chunk, s.size] if s.size else np.zeros(1, dtype=np.int64)
    chunk_dst = np.where(n_chunks[seg_of_chunk] == 1, s[first][seg_of_chunk], -1)
    multi = np.flatnonzero(n_chunks > 1)
    multi_range = np.stack([chunk0[multi], chunk0[multi + 1]], axis=1).reshape(-1)
    multi_row = s[first][multi]
    return tuple(np.ascontiguousarray(a, dtype=np.int32) for a in (rows, chunk_start, chunk_dst, multi_range, multi_row))


def live_plan(ids, device, live=None, chunk=LIVE_SUM_CHUNK):
    """live_plan_host's five arrays as int32 device tensors"""
    return tuple(torch.from_numpy(a).to(device) for a in live_plan_host(ids, live, chunk))


def rows_live_sum(problems):
    """srh_rows_live_sum_f32 over 1..3 problems, each a dict(x=(n x d), plan=live_plan(...), out=(table x d)[, scale=1.0,
    keep=None, drop_p=0.0, rng_seed=0, rng_counter=0]): out[row] = scale * the sum of the rows of x the plan lists for it,
    each times its dropout multiplier, in plan order.  Rows of out the plan does not name are left as they are."""
    lib = _lib.load()
    if not 1 <= len(problems) <= LIVE_SUM_MAX_PROBLEMS:
        raise SelfrecHipError(f"rows_live_sum: 1..{LIVE_SUM_MAX_PROBLEMS} problems per call")
    arr = (_lib.LiveSumProblem * len(problems))()
    d = int(problems[0]["x"].shape[1])
    hold = []
    for k, pr in enumerate(problems):
        x, out = pr["x"], pr["out"]
        rows, chunk_start, chunk_dst, multi_range, multi_row = pr["plan"]
        if x.dim() != 2 or out.dim() != 2 or int(x.shape[1]) != d or int(out.shape[1]) != d:
            raise SelfrecHipError("rows_live_sum: x (n x d) and out (table x d) of one width expected")
        n_chunk, n_multi = int(chunk_dst.numel()), int(multi_row.numel())
        if int(chunk_start.numel()) != n_chunk + 1 or int(multi_range.numel()) != 2 * n_multi:
            raise SelfrecHipError("rows_live_sum: the plan's arrays do not match")
        keep = pr.get("keep")
        if keep is not None:
            if int(keep.numel()) != int(x.shape[0]) * d:
                raise SelfrecHipError("rows_live_sum: the keep mask does not match x")
            keep = keep.to(torch.uint8).contiguous()
        x = x.contiguous()
        hold += [x, keep]
        a = arr[k]
        a.d_x, a.n_rows = _p(x, torch.float32, "x"), int(x.shape[0])
        a.d_rows, a.d_chunk_start = _p(rows, torch.int32, "rows"), _p(chunk_start, torch.int32, "chunk_start")
        a.d_chunk_dst = _p(chunk_dst, torch.int32, "chunk_dst")
        a.d_multi_range, a.d_multi_row = _p(multi_range, torch.int32, "multi_range"), _p(multi_row, torch.int32, "multi_row")
        a.n_live, a.n_chunk, a.n_multi = int(rows.numel()), n_chunk, n_multi
        a.d_out, a.n_table = _p(out, torch.float32, "out"), int(out.shape[0])
        a.scale, a.drop_p = float(pr.get("scale", 1.0)), float(pr.get("drop_p", 0.0))
        a.d_keep = _p(keep, torch.uint8, "keep")
        a.rng_seed, a.rng_counter = int(pr.get("rng_seed", 0)) & _U64, int(pr.get("rng_counter", 0)) & _U64
    need = int(lib.srh_rows_live_sum_ws_bytes(arr, len(problems), d))
    ws = torch.empty(need, dtype=torch.uint8, device=problems[0]["x"].device) if need else None
    check(lib.srh_rows_live_sum_f32(arr, len(problems), d, _p(ws), _stream()), "srh_rows_live_sum_f32")
    return [pr["out"] for pr in problems]


class SeqEmbedFn(torch.autograd.Function):
    """The embedding front of the sequence encoder as one launch (seq_embed_fwd); both table gradients come from ONE
    rows_live_sum call over the live rows only: the item plan with scale sqrt(d), the position plan with scale 1, the
    dropout multiplier redrawn from the forward's arguments.  item_plan / pos_plan: live_plan of the item / position ids
    with live = (seq != 0)."""

    @staticmethod
    def forward(ctx, item, pos_table, seq, posid, item_plan, pos_plan, keep, drop_p, rng_seed, rng_counter):
        ctx.args = (seq, item_plan, pos_plan, keep, drop_p, rng_seed, rng_counter, tuple(item.shape), tuple(pos_table.shape))
        return seq_embed_fwd(item, pos_table, seq, posid, keep=keep, drop_p=drop_p, rng_seed=rng_seed,
                             rng_counter=rng_counter)

    @staticmethod
    def backward(ctx, g):
        seq, item_plan, pos_plan, keep, drop_p, rng_seed, rng_counter, item_shape, pos_shape = ctx.args
        d = item_shape[1]
        g = g.reshape(-1, d).to(torch.float32).contiguous()
        gi = torch.zeros(item_shape, dtype=torch.float32, device=g.device)
        gp = torch.zeros(pos_shape, dtype=torch.float32, device=g.device)
        drop = dict(keep=keep, drop_p=drop_p, rng_seed=rng_seed, rng_counter=rng_counter)
        rows_live_sum([dict(x=g, plan=item_plan, out=gi, scale=d ** 0.5, **drop), dict(x=g, plan=pos_plan, out=gp, **drop)])
        return gi, gp, None, None, None, None, None, None, None, None


class SeqBceLiveFn(SeqBceFn):
    """SeqBceFn with the item table's gradient summed over the valid rows of [pos; neg] only (``plan`` = live_plan of
    [pos; neg] with live = [valid; valid]): the rows the kernel zeroed are never walked."""

    @staticmethod
    def table_grad(grows, plan, gt):
        return rows_live_sum([dict(x=grows, plan=plan, out=gt)])[0]


class InfoNceFn(torch.autograd.Function):
    """util/loss_torch.py InfoNCE(v1, v2, tau, b_cos=True) of two (n x d) row sets as one differentiable op over
    srh_infonce_fwd_bwd_multi (idx = NULL: row i of the gradients belongs to row i).  The gradients start at zero and g2 is
    a table of its own, so it is declared exclusive: plain stores instead of float atomics.  d in NCE_WIDTHS."""

    @staticmethod
    def forward(ctx, v1, v2, tau):
        n, d = int(v1.shape[0]), int(v1.shape[1])
        if v1.shape != v2.shape or d not in NCE_WIDTHS:
            raise SelfrecHipError(f"InfoNceFn: two (n x d) views with d in {NCE_WIDTHS} expected")
        v1, v2 = v1.to(torch.float32).contiguous(), v2.to(torch.float32).contiguous()
        dev = v1.device
        buf = torch.zeros(2 * n * d + 2, dtype=torch.float32, device=dev)       # [g1 | g2 | loss (one double)]
        g = buf[:2 * n * d].view(2, n, d)
        loss = buf[2 * n * d:].view(torch.float64)
        infonce_multi([(v1, v2, None, n, None, g[0], g[1], True)], d=d, tau=float(tau), loss_scale=1.0, loss=loss,
                      ws=infonce_ws(n, d, dev))
        ctx.save_for_backward(g)
        return loss.to(torch.float32).reshape(())

    @staticmethod
    def backward(ctx, gout):
        (g,) = ctx.saved_tensors
        g = g * gout
        return g[0], g[1], None


# ---- SEPT (csrc/sept.hip: the row normalise and the tri-training neighbour discrimination) --------------------------------
L2NORM_MAX_WIDTH = 256                        # srh_rows_l2norm_*_f32
TRI_ND_MAX_K = 32


def rows_l2norm_fwd(y):
    """tf.math.l2_normalize(y, axis=1): (out (n x d), inv (n)) with inv_r = rsqrt(max(sum_c y_rc^2, 1e-12)).  Any
    1 <= d <= 256, any n >= 0."""
    if y.dim() != 2:
        raise SelfrecHipError("rows_l2norm_fwd: an (n x d) matrix expected")
    y = y.contiguous()
    n, d = int(y.shape[0]), int(y.shape[1])
    out = torch.empty_like(y)
    inv = torch.empty(n, dtype=torch.float32, device=y.device)
    check(_lib.load().srh_rows_l2norm_fwd_f32(_p(y, torch.float32, "y"), n, d, _p(out), _p(inv), _stream()),
          "srh_rows_l2norm_fwd_f32")
    return out, inv


def rows_l2norm_bwd(g, out, inv):
    """The gradient of rows_l2norm_fwd's input from the gradient g of its output: (g - out (out . g)) * inv per row,
    g * 1e6 on a clamped row (inv == 1e6)."""
    g, out, inv = g.contiguous(), out.contiguous(), inv.contiguous()
    if g.shape != out.shape or g.dim() != 2 or int(inv.numel()) != int(g.shape[0]):
        raise SelfrecHipError("rows_l2norm_bwd: g and out (n x d) and inv (n) expected")
    n, d = int(g.shape[0]), int(g.shape[1])
    gy = torch.empty_like(g)
    check(_lib.load().srh_rows_l2norm_bwd_f32(_p(g, torch.float32, "g"), _p(out, torch.float32, "out"),
                                              _p(inv, torch.float32, "inv"), n, d, _p(gy), _stream()),
          "srh_rows_l2norm_bwd_f32")
    return gy


class NormPropFn(torch.autograd.Function):
    """l2_normalize(A x, axis=1) of one SEPT / MHCN layer (SEPT.py:51-52) as one differentiable op of x: the HIP SpMM and
    the row normalise forward; the normalise backward and the SpMM on the explicit transpose backward (the social views
    are not symmetric)."""

    @staticmethod
    def forward(ctx, handle, x):
        if x.dtype != torch.float32 or not x.is_cuda:
            raise SelfrecHipError("NormPropFn: x must be an fp32 HIP tensor")
        out, inv = rows_l2norm_fwd(spmm_any(handle.csr, x.contiguous()))
        ctx.handle = handle
        ctx.save_for_backward(out, inv)
        return out

    @staticmethod
    def backward(ctx, g):
        out, inv = ctx.saved_tensors
        return None, spmm_any(ctx.handle.transposed().csr, rows_l2norm_bwd(g, out, inv))


def tri_nd_fwd_bwd(views, aug, k, tau=0.1, loss_scale=1.0, ws=None):
    """SEPT's tri-training step (SEPT.py:98-134) forward and backward in one call.  views = (friend, sharing, rec) and
    aug: the (n x d) gathered rows of the batch's unique users, un-normalised.  Returns
        loss (3, float64)   loss_scale * sum_i [log sum_j e_v[i][j] - log sum_{j in pos_v[i]} e_v[i][j]], e = exp(s / tau)
        grads               (dL/dfriend, dL/dsharing, dL/drec, dL/daug), each (n x d), scaled by loss_scale
        pos (3, n, k int32) the positives of each view and row, best first: the top-k of the OTHER two views' averaged
                            softmax (ties to the lowest index)
    No n x n matrix is made.  Any d up to 128 (narrower rows are zero-padded, which changes no result), 1 <= k <= 32,
    n >= k; otherwise the library's unsupported status as a SelfrecHipError."""
    if len(views) != 3:
        raise SelfrecHipError("tri_nd_fwd_bwd: three views (friend, sharing, rec) expected")
    n, d = int(aug.shape[0]), int(aug.shape[1])
    for t in (*views, aug):
        if t.dim() != 2 or int(t.shape[0]) != n or int(t.shape[1]) != d:
            raise SelfrecHipError("tri_nd_fwd_bwd: the three views and aug must share one (n x d) shape")
        _p(t, None, "view")
    w = padded_width(d, TABLE_NCE_WIDTHS)
    if w is None:
        raise SelfrecHipError(f"tri_nd_fwd_bwd: rows of {d} columns -- the kernels serve up to {TABLE_NCE_WIDTHS[-1]}")
    dev = aug.device
    mats = [pad_cols(t.float(), w) for t in (*views, aug)]
    k = int(k)
    loss = torch.empty(3, dtype=torch.float64, device=dev)
    grads = torch.empty((4, n, w), dtype=torch.float32, device=dev)
    pos = torch.empty((3, n, max(k, 0)), dtype=torch.int32, device=dev)
    a = _lib.TriNdArgs()
    for v in range(3):
        a.d_view[v] = _p(mats[v], torch.float32, "view")
        a.d_gview[v] = grads[v].data_ptr()
    a.d_aug, a.d_gaug = _p(mats[3], torch.float32, "aug"), grads[3].data_ptr()
    a.n, a.d, a.k, a.tau, a.loss_scale = n, w, k, float(tau), float(loss_scale)
    a.d_loss, a.d_pos = _p(loss), pos.data_ptr()
    need = int(_lib.load().srh_tri_nd_ws_bytes(n, w, k))
    if ws is None or ws.numel() * ws.element_size() < need:
        ws = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
    check(_lib.load().srh_tri_nd_fwd_bwd(C.byref(a), _p(ws), _stream()), "srh_tri_nd_fwd_bwd")
    return loss, tuple(grads[v] if w == d else grads[v][:, :d] for v in range(4)), pos


class TriNdFn(torch.autograd.Function):
    """tri_nd_fwd_bwd as one differentiable op of (friend, sharing, rec, aug): the three losses summed (SEPT.py:149-151);
    backward() scales the saved gradients by the upstream scalar.  ``TriNdFn.last_pos`` keeps the call's positives."""
    last_pos = None

    @staticmethod
    def forward(ctx, friend, sharing, rec, aug, k, tau):
        loss, grads, pos = tri_nd_fwd_bwd((friend, sharing, rec), aug, k, tau)
        TriNdFn.last_pos = pos
        ctx.save_for_backward(*grads)
        return loss.sum().to(torch.float32)

    @staticmethod
    def backward(ctx, gout):
        return tuple(g * gout for g in ctx.saved_tensors) + (None, None)


def unique_first(ids_host):
    """The unique ids of a host array in first-occurrence order (tf.unique, SEPT.py:99: not sorted)."""
    ids = np.asarray(ids_host).reshape(-1)
    _, first = np.unique(ids, return_index=True)
    return ids[np.sort(first)]


# ---- MHCN (csrc/mhcn.hip: the self-gates, the channel attention and the hierarchical MIM loss) -----------------------------
GATE_MAX = 4                                  # srh_gate_*_f32: gates per call


def _mhcn_width(d, what=None):
    """the width the rows are padded to; a width the kernels do not serve goes to the library as it is, which refuses it
    with its unsupported status"""
    return padded_width(d, TABLE_NCE_WIDTHS) or int(d)


def _ws(need, device):
    return torch.empty(max(int(need), 256), dtype=torch.uint8, device=device)


def _gate_operands(x, w, b, what):
    if x.dim() != 2 or w.dim() != 3 or b.dim() != 2 or w.shape[1] != w.shape[2] or int(w.shape[1]) != int(x.shape[1]) \
            or tuple(b.shape) != (int(w.shape[0]), int(x.shape[1])):
        raise SelfrecHipError(f"{what}: x (n x d), w (C x d x d) and b (C x d) expected")
    n, d, c = int(x.shape[0]), int(x.shape[1]), int(w.shape[0])
    wd = _mhcn_width(d, what)
    xp = pad_cols(x.float(), wd)
    if wd == d:
        wp, bp = w.float().contiguous(), b.float().contiguous()
    else:
        wp = torch.zeros((c, wd, wd), dtype=torch.float32, device=x.device)
        wp[:, :d, :d] = w
        bp = pad_cols(b.float(), wd)
    return xp, wp, bp, n, d, c, wd


def gate_fwd(x, w, b):
    """MHCN's self-gates (MHCN.py:79-83): y[c] = x * sigmoid(x @ w[c] + b[c]) for all C <= 4 gates from one read of x.
    x (n x d), w (C x d x d), b (C x d) -> y (C x n x d).  Any d up to 128 (zero-padded: a padded column gates to 0)."""
    xp, wp, bp, n, d, c, wd = _gate_operands(x, w, b, "gate_fwd")
    y = torch.empty((c, n, wd), dtype=torch.float32, device=x.device)
    check(_lib.load().srh_gate_fwd_f32(_p(xp, torch.float32, "x"), _p(wp, torch.float32, "w"), _p(bp, torch.float32, "b"),
                                       n, wd, c, _p(y), _stream()), "srh_gate_fwd_f32")
    return y if wd == d else y[:, :, :d]


def gate_bwd(x, w, b, gy):
    """The gradients of gate_fwd from gy (C x n x d): (dx (n x d), dw (C x d x d), db (C x d)).  sigmoid(x w + b) is
    recomputed, not saved; the reductions over rows are summed in chunk order."""
    xp, wp, bp, n, d, c, wd = _gate_operands(x, w, b, "gate_bwd")
    if tuple(gy.shape) != (c, n, d):
        raise SelfrecHipError("gate_bwd: gy must be (C x n x d)")
    if wd == d:
        gp = gy.float().contiguous()
    else:
        gp = torch.zeros((c, n, wd), dtype=torch.float32, device=x.device)
        gp[:, :, :d] = gy
    dev = x.device
    gx = torch.empty((n, wd), dtype=torch.float32, device=dev)
    gw = torch.empty((c, wd, wd), dtype=torch.float32, device=dev)
    gb = torch.empty((c, wd), dtype=torch.float32, device=dev)
    ws = _ws(_lib.load().srh_gate_bwd_ws_bytes(n, wd, c), dev)
    check(_lib.load().srh_gate_bwd_f32(_p(xp, torch.float32, "x"), _p(wp, torch.float32, "w"), _p(bp, torch.float32, "b"),
                                       _p(gp, torch.float32, "gy"), n, wd, c, _p(gx), _p(gw), _p(gb), _p(ws), _stream()),
          "srh_gate_bwd_f32")
    if wd == d:
        return gx, gw, gb
    return gx[:, :d], gw[:, :d, :d], gb[:, :d]


class GateFn(torch.autograd.Function):
    """gate_fwd / gate_bwd as one differentiable op of (x, w, b) -> y (C x n x d)."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w, b)
        return gate_fwd(x, w, b)

    @staticmethod
    def backward(ctx, gy):
        x, w, b = ctx.saved_tensors
        return gate_bwd(x, w, b, gy)


def _mix_operands(e1, e2, e3, q, x, what):
    n, d = int(e1.shape[0]), int(e1.shape[1])
    for t in (e1, e2, e3) + (() if x is None else (x,)):
        if t.dim() != 2 or tuple(t.shape) != (n, d):
            raise SelfrecHipError(f"{what}: the channels (and the addend) must share one (n x d) shape")
    if int(q.numel()) != d:
        raise SelfrecHipError(f"{what}: q must hold d entries")
    wd = _mhcn_width(d, what)
    pad = lambda t: pad_cols(t.float(), wd)  # noqa: E731
    return pad(e1), pad(e2), pad(e3), pad(q.reshape(1, d)).reshape(-1), (None if x is None else pad(x)), n, d, wd


def chan_mix_fwd(e1, e2, e3, q, x=None, beta=0.0):
    """MHCN's channel attention (MHCN.py:85-93) with q = attention_mat @ attention^T: w_c = e_c . q per row,
    s = softmax over the three channels, out = sum_c s_c e_c + beta x.  Returns (out (n x d), s (n x 3))."""
    e1, e2, e3, qp, xp, n, d, wd = _mix_operands(e1, e2, e3, q, x, "chan_mix_fwd")
    out = torch.empty((n, wd), dtype=torch.float32, device=e1.device)
    score = torch.empty((n, 3), dtype=torch.float32, device=e1.device)
    check(_lib.load().srh_chan_mix_fwd_f32(_p(e1, torch.float32, "e1"), _p(e2, torch.float32, "e2"),
                                           _p(e3, torch.float32, "e3"), _p(qp, torch.float32, "q"),
                                           _p(xp, torch.float32, "x"), float(beta), n, wd, _p(out), _p(score), _stream()),
          "srh_chan_mix_fwd_f32")
    return (out if wd == d else out[:, :d]), score


def chan_mix_bwd(e1, e2, e3, q, score, gout, beta=0.0, with_x=False):
    """The gradients of chan_mix_fwd's ``out`` from gout (n x d) and the forward's scores:
    (de1, de2, de3, dx or None, dq (d)).  dq is summed over rows in chunk order."""
    e1, e2, e3, qp, gp, n, d, wd = _mix_operands(e1, e2, e3, q, gout, "chan_mix_bwd")
    dev = e1.device
    score = score.float().contiguous()
    if tuple(score.shape) != (n, 3):
        raise SelfrecHipError("chan_mix_bwd: the scores must be (n x 3)")
    g = torch.empty((4 if with_x else 3, n, wd), dtype=torch.float32, device=dev)
    gq = torch.empty(wd, dtype=torch.float32, device=dev)
    ws = _ws(_lib.load().srh_chan_mix_bwd_ws_bytes(n, wd), dev)
    check(_lib.load().srh_chan_mix_bwd_f32(_p(e1, torch.float32, "e1"), _p(e2, torch.float32, "e2"),
                                           _p(e3, torch.float32, "e3"), _p(qp, torch.float32, "q"),
                                           _p(score, torch.float32, "score"), _p(gp, torch.float32, "gout"), float(beta), n,
                                           wd, g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(),
                                           g[3].data_ptr() if with_x else None, _p(gq), _p(ws), _stream()),
          "srh_chan_mix_bwd_f32")
    cut = (lambda t: t) if wd == d else (lambda t: t[:, :d])
    return cut(g[0]), cut(g[1]), cut(g[2]), (cut(g[3]) if with_x else None), gq[:d]


class ChanMixFn(torch.autograd.Function):
    """chan_mix_fwd / chan_mix_bwd as one differentiable op of (e1, e2, e3, q, x or None) -> (out, scores); the scores
    carry no gradient (MHCN reads them as ``attention_score`` only)."""

    @staticmethod
    def forward(ctx, e1, e2, e3, q, x, beta):
        out, score = chan_mix_fwd(e1, e2, e3, q, x, beta)
        ctx.save_for_backward(e1, e2, e3, q, score)
        ctx.beta, ctx.with_x = float(beta), x is not None
        ctx.mark_non_differentiable(score)
        return out, score

    @staticmethod
    def backward(ctx, gout, _gscore):
        e1, e2, e3, q, score = ctx.saved_tensors
        g1, g2, g3, gx, gq = chan_mix_bwd(e1, e2, e3, q, score, gout, ctx.beta, ctx.with_x)
        return g1, g2, g3, gq.reshape(q.shape), gx, None


def mim_fwd_bwd(em, edge, p1, p2, p3, c2, c3, loss_scale=1.0):
    """MHCN's hierarchical mutual-information loss (MHCN.py:159-181) of one channel, forward and backward in one call, with
    the shuffles given: p1, p2, p3 row permutations of n, c2, c3 column permutations of d.  edge = H @ em is the caller's
    SpMM.  Returns (loss (float64 scalar), dL/dem, dL/dedge), the gradients scaled by loss_scale.  -log(sigmoid(x)) is
    taken as softplus(-x): finite where the reference's form overflows."""
    n, d = int(em.shape[0]), int(em.shape[1])
    if em.dim() != 2 or tuple(edge.shape) != (n, d):
        raise SelfrecHipError("mim_fwd_bwd: em and edge must share one (n x d) shape")
    wd = _mhcn_width(d, "mim_fwd_bwd")
    dev = em.device
    rows = [p.to(device=dev, dtype=torch.int32).contiguous() for p in (p1, p2, p3)]
    cols = [c.to(device=dev, dtype=torch.int32).contiguous() for c in (c2, c3)]
    if any(int(p.numel()) != n for p in rows) or any(int(c.numel()) != d for c in cols):
        raise SelfrecHipError("mim_fwd_bwd: three permutations of n rows and two of d columns expected")
    if wd != d:       # the identity over the pad columns
        tail = torch.arange(d, wd, dtype=torch.int32, device=dev)
        cols = [torch.cat([c, tail]) for c in cols]
    emp, edp = pad_cols(em.float(), wd), pad_cols(edge.float(), wd)
    loss = torch.empty((), dtype=torch.float64, device=dev)
    g = torch.empty((2, n, wd), dtype=torch.float32, device=dev)
    a = _lib.MimArgs()
    a.d_em, a.d_edge = _p(emp, torch.float32, "em"), _p(edp, torch.float32, "edge")
    for i in range(3):
        a.d_row_perm[i] = rows[i].data_ptr()
    for i in range(2):
        a.d_col_perm[i] = cols[i].data_ptr()
    a.n, a.d, a.loss_scale = n, wd, float(loss_scale)
    a.d_loss, a.d_gem, a.d_gedge = _p(loss), g[0].data_ptr(), g[1].data_ptr()
    ws = _ws(_lib.load().srh_mim_ws_bytes(n, wd), dev)
    check(_lib.load().srh_mim_fwd_bwd(C.byref(a), _p(ws), _stream()), "srh_mim_fwd_bwd")
    return loss, (g[0] if wd == d else g[0][:, :d]), (g[1] if wd == d else g[1][:, :d])


class MimFn(torch.autograd.Function):
    """mim_fwd_bwd as one differentiable op of (em, edge); backward() scales the saved gradients by the upstream scalar
    (torch chains dL/dedge through the transposed SpMM)."""

    @staticmethod
    def forward(ctx, em, edge, p1, p2, p3, c2, c3):
        loss, gem, gedge = mim_fwd_bwd(em, edge, p1, p2, p3, c2, c3)
        ctx.save_for_backward(gem, gedge)
        return loss.to(torch.float32)

    @staticmethod
    def backward(ctx, gout):
        gem, gedge = ctx.saved_tensors
        return gem * gout, gedge * gout, None, None, None, None, None


class RowsL2NormFn(torch.autograd.Function):
    """tf.math.l2_normalize(y, axis=1) on its own (MHCN keeps the raw propagated rows for the next layer, so the SpMM and
    the normalise are separate ops there): rows_l2norm_fwd / rows_l2norm_bwd."""

    @staticmethod
    def forward(ctx, y):
        out, inv = rows_l2norm_fwd(y)
        ctx.save_for_backward(out, inv)
        return out

    @staticmethod
    def backward(ctx, g):
        out, inv = ctx.saved_tensors
        return rows_l2norm_bwd(g, out, inv)


# ---- MixGCF (csrc/mixgcf.hip: the hop mixing -- pick, mix and row gradients) -----------------------------------------------
MIXUP_MAX_HOPS = _lib.SRH_MIXUP_MAX_HOPS


def mixup_supported(d, n_hops, n_negs) -> bool:
    """the shapes srh_mixup_*_f32 serve: d a multiple of 4 in 4..256, 1..8 hop tables, at least one candidate per pair"""
    d, n_hops, n_negs = int(d), int(n_hops), int(n_negs)
    return 4 <= d <= 256 and d % 4 == 0 and 1 <= n_hops <= MIXUP_MAX_HOPS and n_negs >= 1


def _mixup_alpha(alpha, n_hops, shape, device):
    """None, or the H injected (B x C x d) float32 device tensors of a call: a list of H tensors or one (H, B, C, d) array"""
    if alpha is None:
        return None
    if isinstance(alpha, (list, tuple)):
        hops = [torch.as_tensor(a) for a in alpha]
    else:
        alpha = torch.as_tensor(alpha)
        hops = [alpha[k] for k in range(int(alpha.shape[0]))] if alpha.dim() == 4 else None
    if hops is None or len(hops) != n_hops or any(tuple(a.shape) != shape for a in hops):
        raise SelfrecHipError(f"mixup: alpha must be {n_hops} tensors of shape {shape}")
    return [a.to(device=device, dtype=torch.float32).contiguous() for a in hops]


def _mixup_args(dev, n_items, d, n_hops, B, n_negs, pos, neg, alpha, rng_seed, rng_counter, what):
    """the index streams as int32 (converted once) and the args struct without its table pointers; the returned list keeps
    the converted tensors alive until the call is enqueued"""
    if not pos.is_cuda or not neg.is_cuda:
        raise SelfrecHipError(f"{what}: expected HIP device tensors (the product path has no CPU fallback)")
    if pos.dim() != 1 or int(neg.numel()) != B * n_negs:
        raise SelfrecHipError(f"{what}: pos (B) and neg (B * n_negs) expected")
    pos32, neg32 = pos.to(torch.int32).contiguous(), neg.reshape(-1).to(torch.int32).contiguous()
    al = _mixup_alpha(alpha, n_hops, (B, n_negs, d), dev)
    a = _lib.MixupArgs()
    a.d_pos, a.d_neg = pos32.data_ptr(), neg32.data_ptr()
    a.n_items, a.B, a.n_hops, a.n_negs, a.d = n_items, B, n_hops, n_negs, d
    a.rng_seed, a.rng_counter = int(rng_seed) & 0xFFFFFFFFFFFFFFFF, int(rng_counter) & 0xFFFFFFFFFFFFFFFF
    if al is not None:
        for k in range(min(n_hops, MIXUP_MAX_HOPS)):
            a.d_alpha[k] = al[k].data_ptr()
    return a, [pos32, neg32, al]


def _hop_shape(item_hops, what):
    if len(item_hops) < 1 or any(t.dim() != 2 or tuple(t.shape) != tuple(item_hops[0].shape) for t in item_hops):
        raise SelfrecHipError(f"{what}: the hop tables must share one (I x d) shape")
    return int(item_hops[0].shape[0]), int(item_hops[0].shape[1])


def mixup_fwd(u, item_hops, pos, neg, n_negs, *, alpha=None, rng_seed=0, rng_counter=0):
    """MixGCF's hop mixing (MixGCF.py:96-114): per pair and hop the n_negs candidates are mixed with the positive
    (alpha p + (1 - alpha) n, alpha per element), scored against the user row u (B x d), and the hardest one is kept.
    item_hops: H tensors (I x d), handed over as they are (row slices of wider tables included).  alpha: None (drawn in
    the kernel at counters rng_counter + (k B + b) n_negs + c) or H tensors (B x n_negs x d).
    Returns (pos_out, neg_out (B x d): the hop means of the positives and of the kept mixtures, pick (H x B, int32))."""
    n_items, d = _hop_shape(item_hops, "mixup_fwd")
    n_hops, n_negs, B = len(item_hops), int(n_negs), int(pos.numel())
    if u.dim() != 2 or tuple(u.shape) != (B, d):
        raise SelfrecHipError("mixup_fwd: u must be (B x d)")
    dev = u.device
    a, keep = _mixup_args(dev, n_items, d, n_hops, B, n_negs, pos, neg, alpha, rng_seed, rng_counter, "mixup_fwd")
    for k in range(min(n_hops, MIXUP_MAX_HOPS)):
        a.d_table[k] = _p(item_hops[k], torch.float32, f"item_hops[{k}]")
    uc = u.contiguous()
    out = torch.empty((2, B, d), dtype=torch.float32, device=dev)
    pick = torch.empty((n_hops, B), dtype=torch.int32, device=dev)
    check(_lib.load().srh_mixup_fwd_f32(C.byref(a), _p(uc, torch.float32, "u"), out[0].data_ptr(), out[1].data_ptr(),
                                        _p(pick), _stream()), "srh_mixup_fwd_f32")
    return out[0], out[1], pick


def mixup_bwd(item_hops, pos, neg, n_negs, pick, g_pos, g_neg, *, alpha=None, rng_seed=0, rng_counter=0):
    """The gradients of mixup_fwd's two outputs with respect to the hop tables: a list of H dense (I x d) tensors, zero
    outside the touched rows, every row summed in ascending pair order (a pair's positive before its negative).  Only the
    shape of item_hops is read; g_pos / g_neg (B x d) may be None (zero); alpha / rng_* as in the forward call."""
    n_items, d = _hop_shape(item_hops, "mixup_bwd")
    return _mixup_bwd(len(item_hops), n_items, d, pos, neg, n_negs, pick, g_pos, g_neg, alpha, rng_seed, rng_counter)


def _mixup_bwd(n_hops, n_items, d, pos, neg, n_negs, pick, g_pos, g_neg, alpha, rng_seed, rng_counter):
    n_negs, B = int(n_negs), int(pos.numel())
    dev = pos.device
    for g in (g_pos, g_neg):
        if g is not None and tuple(g.shape) != (B, d):
            raise SelfrecHipError("mixup_bwd: g_pos and g_neg must be (B x d)")
    if tuple(pick.shape) != (n_hops, B):
        raise SelfrecHipError("mixup_bwd: pick must be (H x B)")
    a, keep = _mixup_args(dev, n_items, d, n_hops, B, n_negs, pos, neg, alpha, rng_seed, rng_counter, "mixup_bwd")
    grads = torch.empty((n_hops, n_items, d), dtype=torch.float32, device=dev)
    for k in range(min(n_hops, MIXUP_MAX_HOPS)):
        a.d_grad[k] = grads[k].data_ptr()
    gp = None if g_pos is None else g_pos.float().contiguous()
    gn = None if g_neg is None else g_neg.float().contiguous()
    pk = pick.to(torch.int32).contiguous()
    ws = _ws(_lib.load().srh_mixup_bwd_ws_bytes(B, n_hops), dev)
    check(_lib.load().srh_mixup_bwd_f32(C.byref(a), _p(pk, torch.int32, "pick"), _p(gp), _p(gn), _p(ws), _stream()),
          "srh_mixup_bwd_f32")
    return [grads[k] for k in range(n_hops)]


class MixupFn(torch.autograd.Function):
    """mixup_fwd / mixup_bwd as one differentiable op of the H hop tables -> (pos_out, neg_out, pick).  u, the indices,
    alpha and pick carry no gradient (the choice is detached in the reference); the backward pass needs none of the
    tables, only the int32 index streams, pick and the alpha source."""

    @staticmethod
    def forward(ctx, u, pos, neg, n_negs, alpha, rng_seed, rng_counter, *item_hops):
        pos32, neg32 = pos.to(torch.int32), neg.reshape(-1).to(torch.int32)
        al = _mixup_alpha(alpha, len(item_hops), (int(pos.numel()), int(n_negs), int(item_hops[0].shape[1])), u.device)
        pos_out, neg_out, pick = mixup_fwd(u.detach(), [t.detach() for t in item_hops], pos32, neg32, n_negs, alpha=al,
                                           rng_seed=rng_seed, rng_counter=rng_counter)
        ctx.save_for_backward(pos32, neg32, pick, *(al or ()))
        ctx.shape = (len(item_hops), int(item_hops[0].shape[0]), int(item_hops[0].shape[1]))
        ctx.n_negs, ctx.rng = int(n_negs), (rng_seed, rng_counter)
        ctx.mark_non_differentiable(pick)
        return pos_out, neg_out, pick

    @staticmethod
    def backward(ctx, g_pos, g_neg, _g_pick):
        pos32, neg32, pick, *al = ctx.saved_tensors
        grads = _mixup_bwd(*ctx.shape, pos32, neg32, ctx.n_negs, pick, g_pos, g_neg, al or None, *ctx.rng)
        return (None,) * 7 + tuple(grads)
