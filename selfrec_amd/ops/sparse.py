"""Device CSR matrices with their SpMM schedule, the fused epilogue, graph normalisation, the probes (csrc/spmm.hip, graph.hip).
(Not called ``spmm``: ``ops.spmm`` is only ever the function.)"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from ._base import SPMM_WIDTHS, SelfrecHipError, SpmmEpilogue, _lib, _np, _p, _stream, check, pad_cols, padded_width
from .step import _infonce_problems



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
            if row_mid is not None and np.size(row_mid) != self.shape[0]:
                raise SelfrecHipError("DeviceCSR: row_mid needs one entry per row")
            self._plan, self._plan_owner = self._new_plan(split_len, xcd_split_row, row_mid), None
        if isinstance(vals, torch.Tensor):
            self.vals = vals.to(device=device, dtype=torch.float32).contiguous()
        else:
            self.vals = torch.as_tensor(np.ascontiguousarray(vals, dtype=np.float32)).to(device)
        self.nnz = int(self.indices.numel())
        if self.vals.numel() != self.nnz:
            raise SelfrecHipError("DeviceCSR: values / indices length mismatch")

    def _new_plan(self, split_len, xcd_split_row, row_mid):
        """a schedule of this structure (srh_spmm_plan_create); row_mid: None or one int32 per row"""
        h, mid = C.c_void_p(), (None if row_mid is None else _np(row_mid, np.int32))
        check(self._lib.srh_spmm_plan_create(C.byref(h), self.shape[0], self.shape[1], self.h_indptr.ctypes.data_as(C.c_void_p),
                                             int(split_len), int(xcd_split_row), mid and mid[1]), "srh_spmm_plan_create")
        return h

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
        other._plan, other._plan_owner = self._new_plan(split_len, xcd_split_row, row_mid), None
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
    h = p_h = None
    if blocks_per_xcd is not None:
        h, p_h = _np(blocks_per_xcd, np.int32)
        if h.shape != (8,):
            raise SelfrecHipError("spmm_set_xcd_shares: eight shares, one per XCD")
    check(_lib.load().srh_spmm_plan_set_xcd_shares(csr._plan, int(d), p_h), "srh_spmm_plan_set_xcd_shares")


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


def _us_per_launch(once, iters):
    """us per call of once() after 5 warm-up calls: HIP events on the launch stream"""
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


def spmm_gather_bound(csr, x: torch.Tensor, iters: int = 30) -> float:
    """us per launch of srh_spmm_gather_bound on `csr`'s plan: the product's own gathers on the product's own schedule and
    nothing after them -- a measured lower bound of ``spmm(csr, x)`` (HIP events on the launch stream).  Measurement only."""
    d = int(x.shape[1])
    scratch = torch.zeros(d, dtype=torch.float32, device=x.device)
    lib = _lib.load()

    def once():
        check(lib.srh_spmm_gather_bound(csr._plan, _p(csr.indices, torch.int32), _p(x, torch.float32, "x"), scratch.data_ptr(),
                                        d, _stream()), "srh_spmm_gather_bound")
    return _us_per_launch(once, iters)


def gather_floor_probe(indices: torch.Tensor, x: torch.Tensor, blocks: int = 4096, iters: int = 30) -> float:
    """us per pass of the bare gather stream over `indices` into the (rows, d) table `x` (srh_gather_floor_probe: the row
    fetches of one propagation launch and nothing else), HIP events on the launch stream.  Measurement only."""
    d = int(x.shape[1])
    sink = torch.zeros(4, dtype=torch.float32, device=x.device)
    lib = _lib.load()

    def once():
        check(lib.srh_gather_floor_probe(_p(indices, torch.int32, "indices"), int(indices.numel()), _p(x, torch.float32, "x"),
                                         int(x.shape[0]), d, int(blocks), sink.data_ptr(), _stream()), "srh_gather_floor_probe")
    return _us_per_launch(once, iters)


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
