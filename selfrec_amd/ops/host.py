"""Host-only pieces (csrc/sampler.cpp, the host entry points of csrc/eval.hip): sampler replay, heap-order top-k, unique ids."""
from __future__ import annotations

import ctypes as C
import random as _pyrandom

import numpy as np

from ._base import SelfrecHipError, _lib, _np, check


def _find_k_largest(entry, dtype, k, candidates):
    cand, p_cand = _np(candidates, dtype)
    m = min(int(k), int(cand.size))
    (ids, p_ids), (sc, p_sc) = _np(np.empty(m, dtype=np.int64), np.int64), _np(np.empty(m, dtype=dtype), dtype)
    n_out = C.c_int64()
    check(getattr(_lib.load(), entry)(int(k), p_cand, int(cand.size), p_ids, p_sc, C.byref(n_out)), entry)
    assert n_out.value == m
    return ids, sc


def find_k_largest_host(k: int, candidates) -> tuple[np.ndarray, np.ndarray]:
    """ids (int64), scores (float32) of reference util/algorithm.py:144-156 ``find_k_largest`` -- the heap's own order among
    equal scores -- for a float32 vector on the host (srh_find_k_largest_host: python's heapq restated in C++)."""
    return _find_k_largest("srh_find_k_largest_host", np.float32, k, candidates)


def find_k_largest_host_f64(k: int, candidates) -> tuple[np.ndarray, np.ndarray]:
    """find_k_largest_host for a float64 vector (UserKNN / ItemKNN rows): ids (int64), scores (float64) in the reference
    heap walk's order (srh_find_k_largest_host_f64)."""
    return _find_k_largest("srh_find_k_largest_host_f64", np.float64, k, candidates)


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
        uniq = ("uniq_u", "uniq_i", "n_uniq_u", "n_uniq_i") if with_unique else ()
        held = None if slot is None else self._epoch_slots.get(key)
        if held is not None:
            for k in uniq:
                held[k].fill(0)
        else:
            held = {k: np.empty(e * n, dtype=np.int32) for k, n in (("u", 1), ("i", 1), ("j", n_negs))}
            held.update({k: np.zeros(nb if k.startswith("n_") else nb * batch_size, dtype=np.int32) for k in uniq})
            if slot is not None:
                self._epoch_slots[key] = held
        u, i, j = held["u"], held["i"], held["j"]
        uu, ui, nuu, nui = (held.get(k) for k in ("uniq_u", "uniq_i", "n_uniq_u", "n_uniq_i"))
        res = {"u": u, "i": i, "j": j, "n_batches": nb, **{k: held[k] for k in uniq}}
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


def unique_first(ids_host):
    """The unique ids of a host array in first-occurrence order (tf.unique, SEPT.py:99: not sorted)."""
    ids = np.asarray(ids_host).reshape(-1)
    _, first = np.unique(ids, return_index=True)
    return ids[np.sort(first)]
