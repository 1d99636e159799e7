"""The host C++ layer under the C ABI -- csrc/common.cpp, sampler.cpp, loader.cpp -- run under ASan + UBSan and under TSan.

`make -C selfrec_amd/csrc host_san` links the three sources with tests/host/host_driver.cpp (a program with its own main)
into build/host_driver_asan and build/host_driver_tsan; the sanitizer runtimes are linked statically, nothing is preloaded.
Every test writes its cases as a driver script, runs BOTH programs on it in fresh processes (exit status 0, nothing on
stderr, leak checking on) and then holds the arrays and statuses they wrote to two yardsticks:
  * bit equality with the production libselfrec_hip.so (-O3), driven through ctypes with the very same script lines -- a
    difference between the two builds would be optimisation-dependent undefined behaviour;
  * an independent restatement: CPython's own `random`, `heapq` on (score, position) tuples, conftest.host_batch_segments,
    np.unique, the python loader path of selfrec_amd/data/loader.py, torch's CPU generator, the golden sampler streams.

CPU only: the module skips itself where a HIP device is visible (sanitizer runs do not belong in a GPU job) and where hipcc
is missing.

Out of scope here:
  * csrc/reclist.c runs inside CPython; it could only be checked with a sanitizer runtime preloaded into python, which this
    project does not do.  It stays unchecked.
  * csrc/collectives.cpp does nothing without RCCL and a device.
  * the host planning code inside the .hip files (srh_spmm_plan_create, srh_infonce_plan, the *_ws_bytes forms) cannot be
    linked without its device side; its CPU tests through ctypes stay as they are.
  * GPU-side sanitizers, XNACK builds, and any sanitizer run of code loaded into python.
"""
import ctypes as C
import heapq
import os
import random
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from selfrec_amd import _lib
from selfrec_amd.data import loader as py_loader

from .conftest import host_batch_segments

if torch.cuda.is_available():
    pytest.skip("sanitizer runs of the host layer belong on the CPU machine, never in a GPU job", allow_module_level=True)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "selfrec_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
    pytest.skip(f"no hipcc ({HIPCC}): the sanitized host drivers cannot be built", allow_module_level=True)

SAMPLER_THREADS = (1, 2, 3, 4, 7, 16, 64)
LOADER_THREADS = (1, 2, 3, 4, 7, 32, 256)
DTYPES = {"i32": np.int32, "u32": np.uint32, "i64": np.int64, "f32": np.float32, "f64": np.float64, "u8": np.uint8}
NAMES = {np.dtype(v): k for k, v in DTYPES.items()}
INVALID, STATE = -1, -5


# ---------------------------------------------------------------------------------------------------------------------------
# scripts, and the two things that run them
# ---------------------------------------------------------------------------------------------------------------------------
def i(v):
    return f"i:{int(v)}"


def fb(v):
    return "fb:%d" % struct.unpack("<I", struct.pack("<f", float(v)))[0]


def s(path):
    return "null" if path is None else f"s:{path}"


class Script:
    """The lines of one driver script (tests/host/host_driver.cpp documents them) and the files its arrays are read from."""

    def __init__(self, root, tag="s"):
        self.root, self.tag, self.lines = str(root), tag, []
        os.makedirs(self.root, exist_ok=True)

    def setenv(self, name, value):
        self.lines.append(f"setenv {name} {value}")

    def buf(self, name, dtype, count):
        self.lines.append(f"buf {name} {dtype} {count}")
        return "@" + name

    def _file(self, how, name, array):
        array = np.ascontiguousarray(array)
        path = os.path.join(self.root, f"{self.tag}.{name}.in")
        array.tofile(path)
        self.lines.append(f"{how} {name} {NAMES[array.dtype]} {path}")
        return "@" + name

    def load(self, name, array):
        return self._file("load", name, array)

    def share(self, name, array):
        return self._file("share", name, array)

    def share_file(self, name, dtype, path):
        """an array another script already wrote: the driver reads a file once, so its threads share the memory"""
        self.lines.append(f"share {name} {dtype} {path}")
        return "@" + name

    def call(self, label, fn, *args):
        self.lines.append(" ".join(["call", label, fn] + [str(a) for a in args]))

    def write(self):
        path = os.path.join(self.root, f"{self.tag}.script")
        with open(path, "w") as f:
            f.write("\n".join(self.lines) + "\n")
        return path


class Result:
    def __init__(self):
        self.a, self.s = {}, {}

    def rc(self, label):
        return self.s[label][0]

    def same_as(self, other, what):
        assert list(self.s) == list(other.s), what
        for k, v in self.s.items():
            assert v == other.s[k], (what, k, v, other.s[k])
        assert list(self.a) == list(other.a), what
        for k, v in self.a.items():
            w = other.a[k]
            assert v.dtype == w.dtype and v.shape == w.shape and v.tobytes() == w.tobytes(), (what, k)


def _read_result(out_dir):
    res = Result()
    with open(os.path.join(out_dir, "index.txt"), "rb") as f:
        for line in f.read().decode().split("\n"):
            if line.startswith("A "):
                _, name, dtype, count = line.split(" ")
                res.a[name] = np.fromfile(os.path.join(out_dir, name + ".bin"), dtype=DTYPES[dtype])
                assert res.a[name].size == int(count)
            elif line.startswith("S "):
                parts = line.split(" ", 3)
                res.s[parts[1]] = (int(parts[2]), parts[3] if len(parts) > 3 else "")
    return res


def run_driver(binary, scripts, out_dir, env=None, limit=120):
    """Fresh process under `timeout`; the sanitizers halt on the first report; exit status 0 and silence are required."""
    paths = [sc.write() for sc in scripts]
    os.makedirs(out_dir)
    if len(scripts) > 1:
        for k in range(len(scripts)):
            os.makedirs(os.path.join(out_dir, f"t{k}"))
    full = {k: v for k, v in os.environ.items() if k not in ("SRH_SAMPLER_THREADS", "SRH_LOADER_THREADS")}
    full.update(ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1",
                TSAN_OPTIONS="halt_on_error=1")
    full.update(env or {})
    done = subprocess.run(["timeout", "-k", "5", str(limit), binary, "run", out_dir] + paths, env=full, capture_output=True,
                          text=True, errors="replace")
    assert done.returncode == 0 and done.stderr == "" and done.stdout == "", \
        f"{os.path.basename(binary)}: exit {done.returncode}\n{done.stdout[-2000:]}\n{done.stderr[-6000:]}"
    if len(scripts) == 1:
        return [_read_result(out_dir)]
    return [_read_result(os.path.join(out_dir, f"t{k}")) for k in range(len(scripts))]


def run_production(script, env=None):
    """The same lines against libselfrec_hip.so through ctypes, argument types from _lib.SIGNATURES."""
    lib = _lib.load()
    res, arrays, handles, returned = Result(), {}, {}, {}
    keep = {k: os.environ.get(k) for k in ("SRH_SAMPLER_THREADS", "SRH_LOADER_THREADS")}

    def count_of(expr):
        total = 0
        for term in expr.split("+"):
            if term.startswith("$"):
                total += returned[term[1:]]
            elif "[" in term:
                name, k = term[:-1].split("[")
                total += int(arrays[name][int(k)])
            else:
                total += int(term)
        return total

    def arg(tok, ctype):
        if tok == "null":
            return None
        if tok.startswith("i:"):
            return int(tok[2:])
        if tok.startswith("fb:"):
            return struct.unpack("<f", struct.pack("<I", int(tok[3:])))[0]
        if tok.startswith("s:"):
            return tok[2:].encode()
        if tok.startswith("@"):
            return C.cast(C.c_void_p(arrays[tok[1:]].ctypes.data), ctype)
        if tok.startswith("&h:"):
            return C.byref(handles.setdefault(tok[3:], C.c_void_p()))
        if tok.startswith("h:"):
            return handles.setdefault(tok[2:], C.c_void_p())
        raise ValueError(tok)

    try:
        for k in keep:
            os.environ.pop(k, None)
        os.environ.update(env or {})
        for line in script.lines:
            t = line.split()
            if t[0] == "setenv":
                os.environ[t[1]] = t[2]
            elif t[0] == "buf":
                arrays[t[1]] = res.a[t[1]] = np.zeros(count_of(t[3]), dtype=DTYPES[t[2]])
            elif t[0] in ("load", "share"):
                arrays[t[1]] = np.fromfile(t[3], dtype=DTYPES[t[2]])
                if t[0] == "load":
                    res.a[t[1]] = arrays[t[1]]
            elif t[0] == "call":
                restype, argtypes = _lib.SIGNATURES[t[2]]
                assert len(argtypes) == len(t) - 3, line
                rc = getattr(lib, t[2])(*[arg(tok, ct) for tok, ct in zip(t[3:], argtypes)])
                if restype is None:
                    rc = 0
                    if t[3] != "null":
                        handles[t[3][2:]] = C.c_void_p()
                returned[t[1]] = int(rc)
                res.s[t[1]] = (int(rc), lib.srh_last_error_string().decode() if rc < 0 else "")
            else:
                raise ValueError(line)
    finally:
        for k, v in keep.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    assert all(not h.value for h in handles.values()), "a handle was not destroyed"
    return res


@pytest.fixture(scope="session")
def drivers():
    done = subprocess.run(["make", "-C", CSRC, "-j4", "host_san"], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout[-3000:] + done.stderr[-6000:]
    asan, tsan = os.path.join(CSRC, "build", "host_driver_asan"), os.path.join(CSRC, "build", "host_driver_tsan")
    about = {b: subprocess.run([b, "--about"], capture_output=True, text=True, check=True).stdout.split() for b in (asan, tsan)}
    assert about[asan][0] == about[tsan][0] == "sanitizers:"
    assert set(about[asan][1:]) == {"address", "undefined"}, f"{asan} is not instrumented: {about[asan]}"
    assert set(about[tsan][1:]) == {"thread"}, f"{tsan} is not instrumented: {about[tsan]}"
    return asan, tsan


def run_everywhere(drivers, tmp_path, scripts, env=None):
    """Both sanitized programs and the production library on the same scripts: one Result per script, equal in all three."""
    scripts = scripts if isinstance(scripts, list) else [scripts]
    want = [run_production(sc, env) for sc in scripts]
    for binary in drivers:
        name = os.path.basename(binary)
        got = run_driver(binary, scripts, str(tmp_path / ("out_" + name)), env)
        for k, (g, w) in enumerate(zip(got, want)):
            g.same_as(w, f"{name} against the production library, script {k}")
    return want


# ---------------------------------------------------------------------------------------------------------------------------
# the sampler, restated with CPython's own generator
# ---------------------------------------------------------------------------------------------------------------------------
def below(rng, n):
    """Lib/random.py _randbelow_with_getrandbits"""
    k = n.bit_length()
    r = rng.getrandbits(k)
    while r >= n:
        r = rng.getrandbits(k)
    return r


class PySampler:
    """util/sampler.py:5-28 of the reference on python lists: shuffle the training list, then one rejection loop per negative."""

    def __init__(self, eu, ei, n_items, rng):
        self.eu, self.ei, self.n_items, self.rng = [int(x) for x in eu], [int(x) for x in ei], n_items, rng
        self.order = list(range(len(self.eu)))
        self.rated = {}
        for u, it in zip(self.eu, self.ei):
            self.rated.setdefault(u, set()).add(it)

    def shuffle(self):
        self.rng.shuffle(self.order)

    def batch(self, ptr, bs, negs):
        es = self.order[ptr:ptr + bs]
        j = []
        for e in es:
            for _ in range(negs):
                c = below(self.rng, self.n_items)
                while c in self.rated[self.eu[e]]:
                    c = below(self.rng, self.n_items)
                j.append(c)
        return [self.eu[e] for e in es], [self.ei[e] for e in es], j

    def epoch(self, negs):
        self.shuffle()
        return self.batch(0, len(self.order), negs)


def add_epoch(sc, p, h, E, bs, negs, uniq, seg_rows0=()):
    """One srh_sampler_epoch into arrays prefixed p (exact sizes: ASan sees a write past any of them), then the segments."""
    nb = (E + bs - 1) // bs
    u, it, j = sc.buf(p + "u", "i32", E), sc.buf(p + "i", "i32", E), sc.buf(p + "j", "i32", E * negs)
    uq = ["null"] * 4
    if uniq:
        uq = [sc.buf(p + "uu", "i32", nb * bs), sc.buf(p + "nuu", "i32", nb), sc.buf(p + "ui", "i32", nb * bs), sc.buf(p + "nui", "i32", nb)]
    sc.call(p + "epoch", "srh_sampler_epoch", h, i(bs), i(negs), u, it, j, *uq)
    for k, (ur0, ir0) in enumerate(seg_rows0):
        q = f"{p}g{k}."
        outs = [sc.buf(q + "nun", "i32", nb)] + [sc.buf(q + n, "i32", 3 * nb * bs) for n in ("rows", "end", "seg", "a")]
        outs.append(sc.buf(q + "b", "i32", nb * bs))
        sc.call(q + "segments", "srh_sampler_epoch_segments", h, i(bs), u, it, j, *uq, i(ur0), i(ir0), *outs)


def check_epoch(res, p, ref, bs, negs, uniq, seg_rows0=()):
    E = len(ref.order)
    u, it, j = ref.epoch(negs)
    assert res.rc(p + "epoch") == 0
    assert res.a[p + "u"].tolist() == u and res.a[p + "i"].tolist() == it and res.a[p + "j"].tolist() == j, p
    nb = (E + bs - 1) // bs
    for b in range(nb if uniq else 0):
        lo, hi = b * bs, min(E, (b + 1) * bs)
        for ids, got, n in ((u, res.a[p + "uu"], res.a[p + "nuu"]), (it, res.a[p + "ui"], res.a[p + "nui"])):
            want = np.unique(ids[lo:hi])
            assert n[b] == want.size and np.array_equal(got[b * bs:b * bs + n[b]], want) and not got[b * bs + n[b]:(b + 1) * bs].any()
    for k, (ur0, ir0) in enumerate(seg_rows0):
        q = f"{p}g{k}."
        assert res.rc(q + "segments") == 0
        for b in range(nb):
            lo, hi = b * bs, min(E, (b + 1) * bs)
            want = host_batch_segments(u[lo:hi], it[lo:hi], j[lo:hi], bs, ur0, ir0)
            assert res.a[q + "nun"][b] == want["n_uniq_n"][0]
            for name, key, width in (("rows", "seg_rows", 3), ("end", "seg_end", 3), ("seg", "seg", 3), ("a", "seg_a", 3), ("b", "seg_b", 1)):
                assert np.array_equal(res.a[q + name][b * width * bs:(b + 1) * width * bs], want[key]), (q, b, name)


def edge_graph(n_users, n_items, rng):
    """A graph on the sampler's bitmap edges: user 0 rates enough items for the exact bitmap (16 deg >= n_items) where the
    catalogue allows a hashed one beside it, user 1 (if any) three items (hashed once n_items > 256), user 2 (if any)
    nothing, the rest a few each; some edges twice; nobody rates every item (the rejection loop would not end)."""
    eu, ei = [], []
    big = min(n_items - 1, max(3, (n_items + 15) // 16 + 1))
    ei += rng.choice(n_items, big, replace=False).tolist()
    eu += [0] * big
    if n_users > 1:
        ei += rng.choice(n_items, 3, replace=False).tolist()
        eu += [1] * 3
    if n_users > 3:
        rest = rng.integers(3, n_users, 240)
        eu += rest.tolist()
        ei += rng.integers(0, n_items, 240).tolist()
        eu += [n_users - 1, n_users - 1]                              # the last user and the last item are in
        ei += [n_items - 1, 0]
    eu, ei = np.asarray(eu, dtype=np.int32), np.asarray(ei, dtype=np.int32)
    dup = rng.integers(0, eu.size, 5)
    eu, ei = np.concatenate([eu, eu[dup]]), np.concatenate([ei, ei[dup]])
    perm = rng.permutation(eu.size)
    return eu[perm], ei[perm]


def test_sampler_with_no_edges(drivers, tmp_path):
    """n_edges == 0 with null edge arrays: create, epoch, next_batch and sample_range(0, 0) all run and write nothing."""
    sc = Script(tmp_path)
    for t in SAMPLER_THREADS:
        p = f"t{t}."
        sc.setenv("SRH_SAMPLER_THREADS", t)
        sc.call(p + "create", "srh_sampler_create", "&h:s", i(3), i(5), i(0), "null", "null")
        sc.call(p + "seed", "srh_sampler_seed", "h:s", i(7))
        add_epoch(sc, p + "e.", "h:s", 0, 4, 2, True, [(0, 0), (0, 3)])
        add_epoch(sc, p + "f.", "h:s", 0, 4, 1, False)
        outs = [sc.buf(p + n, "i32", 0) for n in ("bu", "bi", "bj")] + [sc.buf(p + "bn", "i64", 1)]
        sc.call(p + "batch", "srh_sampler_next_batch", "h:s", i(0), i(4), i(1), *outs)
        sc.call(p + "range", "srh_sampler_sample_range", "h:s", i(0), i(0), sc.buf(p + "r", "i64", 0))
        sc.call(p + "range_null", "srh_sampler_sample_range", "h:s", i(0), i(0), "null")
        sc.call(p + "order", "srh_sampler_get_order", "h:s", sc.buf(p + "o", "i64", 0))
        sc.call(p + "u32", "srh_sampler_next_u32", "h:s", sc.buf(p + "w", "u32", 1))
        sc.call(p + "destroy", "srh_sampler_destroy", "h:s")
    res, = run_everywhere(drivers, tmp_path, sc)
    assert all(rc == 0 for rc, _ in res.s.values())
    for t in SAMPLER_THREADS:
        assert res.a[f"t{t}.bn"][0] == 0
        assert res.a[f"t{t}.w"][0] == random.Random(7).getrandbits(32)          # nothing was drawn before it


@pytest.mark.parametrize("tag", ["a", "b"])
def test_sampler_golden_streams(drivers, tmp_path, golden_ops, tag):
    """The golden 200 x 300 graph: the reference's own ids, next word and final order, with and without the unique lists, at
    every thread count."""
    g = golden_ops
    bs, negs, seed = (int(x) for x in g[f"sampler_{tag}_meta"])
    eu, ei = g["graph_train_u_ids"].astype(np.int32), g["graph_train_i_ids"].astype(np.int32)
    E = eu.size
    sc = Script(tmp_path)
    pu, pi = sc.share("eu", eu), sc.share("ei", ei)
    for t in SAMPLER_THREADS:
        for uniq in (True, False):
            p = f"t{t}.{'q' if uniq else 'n'}."
            sc.setenv("SRH_SAMPLER_THREADS", t)
            sc.call(p + "create", "srh_sampler_create", "&h:s", i(200), i(300), i(E), pu, pi)
            sc.call(p + "seed", "srh_sampler_seed", "h:s", i(seed))
            for e in range(2):
                add_epoch(sc, f"{p}e{e}.", "h:s", E, bs, negs, uniq)
            sc.call(p + "u32", "srh_sampler_next_u32", "h:s", sc.buf(p + "w", "u32", 1))
            sc.call(p + "order", "srh_sampler_get_order", "h:s", sc.buf(p + "o", "i64", E))
            sc.call(p + "destroy", "srh_sampler_destroy", "h:s")
    res, = run_everywhere(drivers, tmp_path, sc)
    assert all(rc == 0 for rc, _ in res.s.values())
    for t in SAMPLER_THREADS:
        for uniq in (True, False):
            p = f"t{t}.{'q' if uniq else 'n'}."
            for n in "uij":
                assert np.array_equal(np.concatenate([res.a[f"{p}e0.{n}"], res.a[f"{p}e1.{n}"]]), g[f"sampler_{tag}_{n}"])
            assert res.a[p + "w"][0] == int(g[f"sampler_{tag}_next_u32"][0])
            assert np.array_equal(eu[res.a[p + "o"]], g[f"sampler_{tag}_final_order_u"])
            for e in range(2 if uniq else 0):
                q = f"{p}e{e}."
                for b in range((E + bs - 1) // bs):
                    lo, hi = b * bs, min(E, (b + 1) * bs)
                    for n in "ui":
                        want = np.unique(res.a[q + n][lo:hi])
                        assert res.a[f"{q}nu{n}"][b] == want.size and np.array_equal(res.a[f"{q}u{n}"][b * bs:b * bs + want.size], want)


BITMAP_SHAPES = [(1, 63), (63, 64), (64, 65), (65, 4095), (4097, 4096), (64, 4097), (4097, 63), (65, 64)]


@pytest.mark.parametrize("n_users,n_items", BITMAP_SHAPES)
def test_sampler_bitmap_edges(drivers, tmp_path, n_users, n_items):
    """n_items and n_users around 64 and 64 x 64, where the two-level seen bitmaps turn over; an exact-bitmap user beside a
    hashed one, a user without edges, duplicate edges; every thread count, more threads than users and than edges among them."""
    eu, ei = edge_graph(n_users, n_items, np.random.default_rng(n_users * 10007 + n_items))
    E, bs, seed = int(eu.size), 7, 2 ** 32 + 17

    def exact(user):                      # srh_sampler_create: the smallest 2^lg >= max(256, 16 deg) bits, exact once >= n_items
        bits = 256
        while bits < 16 * int((eu == user).sum()):
            bits *= 2
        return bits >= n_items
    assert exact(0) and (n_users == 1 or exact(1) == (n_items <= 256)) and (n_users < 3 or not (eu == 2).any())
    sc = Script(tmp_path)
    pu, pi = sc.share("eu", eu), sc.share("ei", ei)
    for t in SAMPLER_THREADS:
        p = f"t{t}."
        sc.setenv("SRH_SAMPLER_THREADS", t)
        sc.call(p + "create", "srh_sampler_create", "&h:s", i(n_users), i(n_items), i(E), pu, pi)
        sc.call(p + "seed", "srh_sampler_seed", "h:s", i(seed))
        add_epoch(sc, p + "e0.", "h:s", E, bs, 1, True, [(0, 0), (0, n_users)])
        add_epoch(sc, p + "e1.", "h:s", E, E, 2, True)
        sc.call(p + "destroy", "srh_sampler_destroy", "h:s")
    res, = run_everywhere(drivers, tmp_path, sc)
    for t in SAMPLER_THREADS:
        ref = PySampler(eu, ei, n_items, random.Random(seed))
        check_epoch(res, f"t{t}.e0.", ref, bs, 1, True, [(0, 0), (0, n_users)])
        check_epoch(res, f"t{t}.e1.", ref, E, 2, True)


def test_sampler_batch_sizes_and_negatives(drivers, tmp_path):
    """Batch sizes 1, 7, E - 1, E, E + 1 with 1, 2 and 4 negatives: the whole epoch, then the same stream batch by batch."""
    n_users, n_items = 65, 4097
    eu, ei = edge_graph(n_users, n_items, np.random.default_rng(99))
    eu, ei = eu[:60], ei[:60]
    E = int(eu.size)
    combos = [(bs, negs) for bs in (1, 7, E - 1, E, E + 1) for negs in (1, 2, 4)]
    sc = Script(tmp_path)
    pu, pi = sc.share("eu", eu), sc.share("ei", ei)
    sc.setenv("SRH_SAMPLER_THREADS", 3)
    sc.call("create", "srh_sampler_create", "&h:s", i(n_users), i(n_items), i(E), pu, pi)
    sc.call("seed", "srh_sampler_seed", "h:s", i(1))
    for c, (bs, negs) in enumerate(combos):
        add_epoch(sc, f"c{c}.e.", "h:s", E, bs, negs, True, [(0, 0), (0, n_users)] if negs == 1 else ())
        sc.call(f"c{c}.shuffle", "srh_sampler_shuffle", "h:s")
        for b, ptr in enumerate(range(0, E, bs)):
            cnt = min(bs, E - ptr)
            outs = [sc.buf(f"c{c}.b{b}.{n}", "i32", cnt * (negs if n == "j" else 1)) for n in "uij"] + [sc.buf(f"c{c}.b{b}.n", "i64", 1)]
            sc.call(f"c{c}.b{b}.batch", "srh_sampler_next_batch", "h:s", i(ptr), i(bs), i(negs), *outs)
        outs = [sc.buf(f"c{c}.end.{n}", "i32", 0) for n in "uij"] + [sc.buf(f"c{c}.end.n", "i64", 1)]
        sc.call(f"c{c}.end.batch", "srh_sampler_next_batch", "h:s", i(E), i(bs), i(negs), *outs)           # ptr == n_edges: empty
    sc.call("destroy", "srh_sampler_destroy", "h:s")
    res, = run_everywhere(drivers, tmp_path, sc)
    assert all(rc == 0 for rc, _ in res.s.values())
    ref = PySampler(eu, ei, n_items, random.Random(1))
    for c, (bs, negs) in enumerate(combos):
        check_epoch(res, f"c{c}.e.", ref, bs, negs, True, [(0, 0), (0, n_users)] if negs == 1 else ())
        ref.shuffle()
        for b, ptr in enumerate(range(0, E, bs)):
            u, it, j = ref.batch(ptr, bs, negs)
            got = [res.a[f"c{c}.b{b}.{n}"].tolist() for n in "uij"]
            assert got == [u, it, j] and res.a[f"c{c}.b{b}.n"][0] == len(u), (bs, negs, b)
        assert res.a[f"c{c}.end.n"][0] == 0


def test_sampler_state_and_seeds(drivers, tmp_path):
    """set_state at positions 0, 623 and 624, get_state back, seeds up to 2^63 - 1; an unseeded handle refuses with
    SRH_ERR_STATE."""
    eu, ei = edge_graph(65, 64, np.random.default_rng(5))
    E = int(eu.size)
    seeds = (0, 1, 2 ** 31, 2 ** 32 + 17, 2 ** 63 - 1)
    sc = Script(tmp_path)
    pu, pi = sc.share("eu", eu), sc.share("ei", ei)
    sc.call("create", "srh_sampler_create", "&h:s", i(65), i(64), i(E), pu, pi)
    sc.call("unseeded.get", "srh_sampler_get_state", "h:s", sc.buf("x.mt", "u32", 624), sc.buf("x.pos", "i32", 1))
    sc.call("unseeded.shuffle", "srh_sampler_shuffle", "h:s")
    for seed in seeds:
        p = f"s{seed}."
        sc.call(p + "seed", "srh_sampler_seed", "h:s", i(seed))
        for k in range(3):
            sc.call(f"{p}u32.{k}", "srh_sampler_next_u32", "h:s", sc.buf(f"{p}w{k}", "u32", 1))
        add_epoch(sc, p + "e.", "h:s", E, 7, 1, False)
        sc.call(p + "get", "srh_sampler_get_state", "h:s", sc.buf(p + "mt", "u32", 624), sc.buf(p + "pos", "i32", 1))
    words = np.asarray(random.Random(12345).getstate()[1][:624], dtype=np.uint32)
    pw = sc.share("words", words)
    for pos in (0, 623, 624):
        p = f"p{pos}."
        sc.call(p + "set", "srh_sampler_set_state", "h:s", pw, i(pos))
        add_epoch(sc, p + "e.", "h:s", E, 7, 2, False)
        sc.call(p + "get", "srh_sampler_get_state", "h:s", sc.buf(p + "mt", "u32", 624), sc.buf(p + "pos", "i32", 1))
    sc.call("destroy", "srh_sampler_destroy", "h:s")
    res, = run_everywhere(drivers, tmp_path, sc)
    assert res.rc("unseeded.get") == STATE and res.rc("unseeded.shuffle") == STATE
    assert "never seeded" in res.s["unseeded.get"][1] and "state not set" in res.s["unseeded.shuffle"][1]
    ref = PySampler(eu, ei, 64, None)                                   # (the order persists across seeds, as in the handle)
    for seed in seeds:
        p = f"s{seed}."
        ref.rng = random.Random(seed)
        assert [int(res.a[f"{p}w{k}"][0]) for k in range(3)] == [ref.rng.getrandbits(32) for _ in range(3)]
        check_epoch(res, p + "e.", ref, 7, 1, False)
        state = ref.rng.getstate()[1]
        assert res.a[p + "mt"].tolist() == list(state[:624]) and res.a[p + "pos"][0] == state[624]
    for pos in (0, 623, 624):
        p = f"p{pos}."
        ref.rng = random.Random()
        ref.rng.setstate((3, tuple(words.tolist()) + (pos,), None))
        check_epoch(res, p + "e.", ref, 7, 2, False)
        state = ref.rng.getstate()[1]
        assert res.a[p + "mt"].tolist() == list(state[:624]) and res.a[p + "pos"][0] == state[624]


def test_sample_range_on_both_paths(drivers, tmp_path):
    """random.sample(range(n), k): the pool path up to n == setsize, the set path from setsize + 1 (setsize = 21, + 4 **
    ceil(log4(3 k)) for k > 5), k = 0, k = n, and the refusal of k > n.  The next word shows how many draws each took."""
    cases = [(21, 5), (22, 5), (85, 6), (86, 6), (85, 21), (86, 21), (277, 22), (278, 22), (10, 0), (0, 0), (7, 7), (30, 30),
             (300, 300), (100000, 50), (2 ** 32 - 1, 9)]
    sc = Script(tmp_path)
    sc.call("create", "srh_sampler_create", "&h:s", i(1), i(2), i(0), "null", "null")
    for c, (n, k) in enumerate(cases):
        sc.call(f"c{c}.seed", "srh_sampler_seed", "h:s", i(100 + c))
        sc.call(f"c{c}.range", "srh_sampler_sample_range", "h:s", i(n), i(k), sc.buf(f"c{c}.out", "i64", k))
        sc.call(f"c{c}.u32", "srh_sampler_next_u32", "h:s", sc.buf(f"c{c}.w", "u32", 1))
    sc.call("refuse.larger", "srh_sampler_sample_range", "h:s", i(5), i(6), sc.buf("r.out", "i64", 6))
    sc.call("destroy", "srh_sampler_destroy", "h:s")
    res, = run_everywhere(drivers, tmp_path, sc)
    for c, (n, k) in enumerate(cases):
        rng = random.Random(100 + c)
        assert res.rc(f"c{c}.range") == 0 and res.a[f"c{c}.out"].tolist() == rng.sample(range(n), k), (n, k)
        assert res.a[f"c{c}.w"][0] == rng.getrandbits(32), (n, k)
    assert res.rc("refuse.larger") == INVALID and "Sample larger than population" in res.s["refuse.larger"][1]
    assert not res.a["r.out"].any()


def refusal_lines(sc, p, eu, ei, pu, pi):
    """Every refusal path of the sampler (prefix p): label -> the status it must return."""
    E, want = int(eu.size), {}

    def refuse(label, fn, *args, status=INVALID):
        want[p + label] = status
        sc.call(p + label, fn, *args)

    refuse("create.null_out", "srh_sampler_create", "null", i(65), i(64), i(E), pu, pi)
    refuse("create.null_u", "srh_sampler_create", "&h:bad", i(65), i(64), i(E), "null", pi)
    refuse("create.null_i", "srh_sampler_create", "&h:bad", i(65), i(64), i(E), pu, "null")
    refuse("create.no_users", "srh_sampler_create", "&h:bad", i(0), i(64), i(E), pu, pi)
    refuse("create.no_items", "srh_sampler_create", "&h:bad", i(65), i(0), i(E), pu, pi)
    refuse("create.neg_edges", "srh_sampler_create", "&h:bad", i(65), i(64), i(-1), pu, pi)
    refuse("create.wide_items", "srh_sampler_create", "&h:bad", i(65), i(2 ** 31), i(E), pu, pi)
    refuse("create.wide_users", "srh_sampler_create", "&h:bad", i(2 ** 31), i(64), i(E), pu, pi)
    refuse("create.wide_edges", "srh_sampler_create", "&h:bad", i(65), i(64), i(2 ** 32), pu, pi)
    for where, at in (("first", 0), ("middle", E // 2), ("last", E - 1)):         # (the half-built handle must be freed)
        for what, (du, di) in (("user", (65, 0)), ("neg_user", (-1, 0)), ("item", (0, 64)), ("neg_item", (0, -1))):
            bu, bi = eu.copy(), ei.copy()
            if du:
                bu[at] = du
            if di:
                bi[at] = di
            refuse(f"create.{where}.{what}", "srh_sampler_create", "&h:bad", i(65), i(64), i(E),
                   sc.share(f"{p}{where}.{what}.u", bu), sc.share(f"{p}{where}.{what}.i", bi))
    sc.call(p + "create", "srh_sampler_create", "&h:s", i(65), i(64), i(E), pu, pi)
    mt, pos = sc.buf(p + "mt", "u32", 624), sc.buf(p + "pos", "i32", 1)
    u, it, j, n = [sc.buf(p + x, "i32", E) for x in "uij"] + [sc.buf(p + "n", "i64", 1)]
    o, w = sc.buf(p + "o", "i64", E), sc.buf(p + "w", "u32", 1)
    uq = [sc.buf(p + x, "i32", E) for x in ("uu", "nuu", "ui", "nui")]
    seg = [sc.buf(p + x, "i32", 3 * E) for x in ("nun", "rows", "end", "seg", "a", "b")]
    refuse("unseeded.batch", "srh_sampler_next_batch", "h:s", i(0), i(E), i(1), u, it, j, n, status=STATE)
    refuse("unseeded.epoch", "srh_sampler_epoch", "h:s", i(E), i(1), u, it, j, "null", "null", "null", "null", status=STATE)
    refuse("unseeded.range", "srh_sampler_sample_range", "h:s", i(5), i(2), o, status=STATE)
    refuse("unseeded.u32", "srh_sampler_next_u32", "h:s", w, status=STATE)
    refuse("seed.null", "srh_sampler_seed", "null", i(1))
    sc.call(p + "seed", "srh_sampler_seed", "h:s", i(3))
    refuse("set.null_handle", "srh_sampler_set_state", "null", mt, i(0))
    refuse("set.null_words", "srh_sampler_set_state", "h:s", "null", i(0))
    refuse("set.neg_pos", "srh_sampler_set_state", "h:s", mt, i(-1))
    refuse("set.far_pos", "srh_sampler_set_state", "h:s", mt, i(625))
    refuse("get.null_handle", "srh_sampler_get_state", "null", mt, pos)
    refuse("get.null_words", "srh_sampler_get_state", "h:s", "null", pos)
    refuse("get.null_pos", "srh_sampler_get_state", "h:s", mt, "null")
    refuse("shuffle.null", "srh_sampler_shuffle", "null")
    refuse("order.null_handle", "srh_sampler_get_order", "null", o)
    refuse("order.null_out", "srh_sampler_get_order", "h:s", "null")
    outs = [u, it, j, n]
    refuse("batch.null_handle", "srh_sampler_next_batch", "null", i(0), i(E), i(1), *outs)
    for k in range(4):
        refuse(f"batch.null_{k}", "srh_sampler_next_batch", "h:s", i(0), i(E), i(1), *[x if m != k else "null" for m, x in enumerate(outs)])
    refuse("batch.neg_ptr", "srh_sampler_next_batch", "h:s", i(-1), i(E), i(1), *outs)
    refuse("batch.far_ptr", "srh_sampler_next_batch", "h:s", i(E + 1), i(E), i(1), *outs)
    refuse("batch.no_size", "srh_sampler_next_batch", "h:s", i(0), i(0), i(1), *outs)
    refuse("batch.no_negs", "srh_sampler_next_batch", "h:s", i(0), i(E), i(0), *outs)
    refuse("epoch.null_handle", "srh_sampler_epoch", "null", i(E), i(1), u, it, j, *uq)
    for k in range(3):
        refuse(f"epoch.null_{k}", "srh_sampler_epoch", "h:s", i(E), i(1), *[x if m != k else "null" for m, x in enumerate((u, it, j))], *uq)
    refuse("epoch.no_size", "srh_sampler_epoch", "h:s", i(0), i(1), u, it, j, *uq)
    refuse("epoch.no_negs", "srh_sampler_epoch", "h:s", i(E), i(0), u, it, j, *uq)
    for k in range(4):
        refuse(f"epoch.part_uniq_{k}", "srh_sampler_epoch", "h:s", i(E), i(1), u, it, j, *[x if m != k else "null" for m, x in enumerate(uq)])
    ins = [u, it, j] + uq
    refuse("seg.null_handle", "srh_sampler_epoch_segments", "null", i(E), *ins, i(0), i(0), *seg)
    for k in range(7):
        refuse(f"seg.null_in_{k}", "srh_sampler_epoch_segments", "h:s", i(E), *[x if m != k else "null" for m, x in enumerate(ins)], i(0), i(0), *seg)
    for k in range(6):
        refuse(f"seg.null_out_{k}", "srh_sampler_epoch_segments", "h:s", i(E), *ins, i(0), i(0), *[x if m != k else "null" for m, x in enumerate(seg)])
    refuse("seg.no_size", "srh_sampler_epoch_segments", "h:s", i(0), *ins, i(0), i(0), *seg)
    refuse("seg.wide_size", "srh_sampler_epoch_segments", "h:s", i(2 ** 28), *ins, i(0), i(0), *seg)
    refuse("range.null_handle", "srh_sampler_sample_range", "null", i(5), i(2), o)
    refuse("range.null_out", "srh_sampler_sample_range", "h:s", i(5), i(2), "null")
    refuse("range.neg_n", "srh_sampler_sample_range", "h:s", i(-1), i(0), o)
    refuse("range.wide_n", "srh_sampler_sample_range", "h:s", i(2 ** 32), i(2), o)
    refuse("range.neg_k", "srh_sampler_sample_range", "h:s", i(5), i(-1), o)
    refuse("range.larger", "srh_sampler_sample_range", "h:s", i(5), i(6), o)
    refuse("u32.null_handle", "srh_sampler_next_u32", "null", w)
    refuse("u32.null_out", "srh_sampler_next_u32", "h:s", "null")
    # the handle still works, and nothing above drew from its generator or wrote into an output
    sc.call(p + "u32", "srh_sampler_next_u32", "h:s", w)
    sc.call(p + "destroy", "srh_sampler_destroy", "h:s")
    sc.call(p + "destroy.null", "srh_sampler_destroy", "null")
    return want


def check_refusals(res, p, want, eu, ei):
    for label, status in want.items():
        assert res.rc(label) == status and res.s[label][1], label
    for where, at in (("first", 0), ("middle", eu.size // 2), ("last", eu.size - 1)):
        assert res.s[f"{p}create.{where}.user"][1] == f"sampler_create: edge {at} (65,{ei[at]}) out of range"
        assert res.s[f"{p}create.{where}.neg_item"][1] == f"sampler_create: edge {at} ({eu[at]},-1) out of range"
    for x in ("u", "i", "j", "n", "o", "uu", "nuu", "ui", "nui", "nun", "rows", "end", "seg", "a", "b", "mt", "pos"):
        assert not res.a[p + x].any(), x
    assert res.a[p + "w"][0] == random.Random(3).getrandbits(32)


def test_sampler_refusals(drivers, tmp_path):
    """Null arguments, bad sizes, an out-of-range edge in the first, a middle and the last position, calls on an unseeded
    handle: each returns its status with a message and writes nothing; with leak checking on, the half-built handle of a
    refused create shows up if it is not freed."""
    eu, ei = edge_graph(65, 64, np.random.default_rng(8))
    sc = Script(tmp_path)
    pu, pi = sc.share("eu", eu), sc.share("ei", ei)
    sc.setenv("SRH_SAMPLER_THREADS", 4)
    want = refusal_lines(sc, "", eu, ei, pu, pi)
    res, = run_everywhere(drivers, tmp_path, sc)
    check_refusals(res, "", want, eu, ei)


def test_sampler_handles_on_concurrent_threads(drivers, tmp_path):
    """Eight driver threads, each with its own handle over the SAME input arrays, run create -> seed -> two epochs ->
    segments -> destroy at the same time (every create and every segments call starting three workers of its own), beside two
    threads that provoke refusals and read the thread-local error string: every thread's arrays and messages are those of the
    script run alone."""
    n_users, n_items = 65, 4097
    eu, ei = edge_graph(n_users, n_items, np.random.default_rng(21))
    E, bs = int(eu.size), 16
    scripts = []
    for k in range(8):
        sc = Script(tmp_path, f"w{k}")
        if k == 0:
            pu, pi = sc.share("eu", eu), sc.share("ei", ei)
            files = [ln.split()[3] for ln in sc.lines]
        else:
            pu, pi = sc.share_file("eu", "i32", files[0]), sc.share_file("ei", "i32", files[1])
        sc.call("create", "srh_sampler_create", "&h:s", i(n_users), i(n_items), i(E), pu, pi)
        sc.call("seed", "srh_sampler_seed", "h:s", i(1000 + k))
        add_epoch(sc, "e0.", "h:s", E, bs, 1, True, [(0, n_users)])
        add_epoch(sc, "e1.", "h:s", E, bs, 1, True, [(0, n_users)])
        sc.call("destroy", "srh_sampler_destroy", "h:s")
        scripts.append(sc)
    small_u, small_i = edge_graph(65, 64, np.random.default_rng(8))
    wants = []
    for k in range(2):
        sc = Script(tmp_path, f"r{k}")
        pu, pi = sc.share("small_u", small_u), sc.share("small_i", small_i)
        want = {}
        for rep in range(3):
            want.update(refusal_lines(sc, f"rep{rep}.", small_u, small_i, pu, pi))
        wants.append(want)
        scripts.append(sc)
    res = run_everywhere(drivers, tmp_path, scripts, env={"SRH_SAMPLER_THREADS": "3"})
    for k in range(8):
        ref = PySampler(eu, ei, n_items, random.Random(1000 + k))
        check_epoch(res[k], "e0.", ref, bs, 1, True, [(0, n_users)])
        check_epoch(res[k], "e1.", ref, bs, 1, True, [(0, n_users)])
    for k in range(2):
        for rep in range(3):
            check_refusals(res[8 + k], f"rep{rep}.", {a: b for a, b in wants[k].items() if a.startswith(f"rep{rep}.")}, small_u, small_i)


# ---------------------------------------------------------------------------------------------------------------------------
# find_k_largest
# ---------------------------------------------------------------------------------------------------------------------------
def heap_walk(k, scores):
    """reference util/algorithm.py:144-156, literally: heapq on (score, position) tuples, heapreplace on a strictly larger
    score, then the stable descending sort by score."""
    heap = [(float(x), p) for p, x in enumerate(scores[:k])]
    heapq.heapify(heap)
    for off, x in enumerate(scores[k:]):
        if x > heap[0][0]:
            heapq.heapreplace(heap, (float(x), off + k))
    heap.sort(key=lambda pair: pair[0], reverse=True)
    return [p for _, p in heap], [x for x, _ in heap]


def heap_inputs(k, n, rng):
    out = {"ties": rng.integers(0, 5, n) * 0.25, "equal": np.full(n, 1.5), "up": np.arange(n) * 0.5 - 3.0,
           "down": 7.0 - np.arange(n) * 0.5}
    inf = rng.standard_normal(n)
    inf[rng.integers(0, max(n, 1), n // 3)] = np.inf
    inf[rng.integers(0, max(n, 1), n // 3)] = -np.inf
    out["inf"] = inf
    zero = np.where(rng.random(n) < 0.5, 0.0, -0.0)
    zero[rng.integers(0, max(n, 1), n // 4)] = -1.0
    out["zeros"] = zero
    planted = rng.standard_normal(n)                      # the k-th best score again on both sides of the heap's first fill
    if n > k:
        kth = np.sort(planted)[::-1][k - 1]
        planted[max(0, k - 3):min(n, k + 3)] = kth
        planted[rng.integers(k, n, 3)] = kth
    out["planted"] = planted
    return out


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_find_k_largest_is_heapq_step_by_step(drivers, tmp_path, dtype):
    """K in {1, 2, 20, 128}, n in {0, 1, K - 1, K, K + 1, 5 K}: all scores equal, ties planted across the heap boundary,
    infinities of both signs, -0.0 against +0.0, ascending and descending inputs -- ids in heapq's own ORDER, scores bit for
    bit.  NaN scores stay out: CPython compares tuples by identity before equality, so a NaN that meets ITSELF in the heap
    counts as equal there, which no restatement over arrays of numbers can reproduce."""
    fn = "srh_find_k_largest_host" if dtype == "f32" else "srh_find_k_largest_host_f64"
    rng = np.random.default_rng(17)
    sc = Script(tmp_path)
    cases = {}
    for k in (1, 2, 20, 128):
        for n in sorted({0, 1, k - 1, k, k + 1, 5 * k}):
            for name, x in heap_inputs(k, n, rng).items():
                p = f"k{k}.n{n}.{name}."
                x = np.asarray(x, dtype=DTYPES[dtype])
                cases[p] = (k, x)
                m = min(k, n)
                sc.call(p + "call", fn, i(k), sc.share(p + "x", x), i(n), sc.buf(p + "ids", "i64", m), sc.buf(p + "sc", dtype, m),
                        sc.buf(p + "m", "i64", 1))
    x = sc.share("x", np.ones(4, dtype=DTYPES[dtype]))
    ids, scs, m = sc.buf("ids", "i64", 4), sc.buf("sc", dtype, 4), sc.buf("m", "i64", 1)
    refused = ["null_x", "null_ids", "null_sc", "null_m", "k0", "neg_n"]
    sc.call("null_x", fn, i(2), "null", i(4), ids, scs, m)
    sc.call("null_ids", fn, i(2), x, i(4), "null", scs, m)
    sc.call("null_sc", fn, i(2), x, i(4), ids, "null", m)
    sc.call("null_m", fn, i(2), x, i(4), ids, scs, "null")
    sc.call("k0", fn, i(0), x, i(4), ids, scs, m)
    sc.call("neg_n", fn, i(2), x, i(-1), ids, scs, m)
    res, = run_everywhere(drivers, tmp_path, sc)
    for p, (k, x) in cases.items():
        want_ids, want_sc = heap_walk(k, x)
        assert res.rc(p + "call") == 0 and res.a[p + "m"][0] == len(want_ids), p
        assert res.a[p + "ids"].tolist() == want_ids, p
        assert res.a[p + "sc"].tobytes() == np.asarray(want_sc, dtype=DTYPES[dtype]).tobytes(), p
    assert all(res.rc(r) == INVALID and res.s[r][1] for r in refused)
    assert not res.a["ids"].any() and not res.a["sc"].any() and not res.a["m"].any()


# ---------------------------------------------------------------------------------------------------------------------------
# srh_mt19937_uniform_f32 against torch's CPU generator
# ---------------------------------------------------------------------------------------------------------------------------
def test_mt19937_uniform_against_torch(drivers, tmp_path):
    """Positions 0, 1, 623, 624 x counts 0, 1, 623, 624, 625, 1500 x keep_addend 0, 0.9, 1, each output null in turn: the
    uniforms, the keep mask and the state left behind are torch.rand's."""
    from selfrec_amd.util import torch_rng
    sc = Script(tmp_path)
    want = {}
    with torch.random.fork_rng():
        torch.manual_seed(2024)
        torch.rand(700)                                            # (a state some blocks into the stream)
        raw0, words0, _ = torch_rng._read_state()
        # torch's generator is never AT position 0 between draws (it regenerates and draws in one step), so position 0 of a
        # block of words is reached from the block before it: words0 at 624 and `words` at 0 give the same numbers
        torch_rng._write_state(raw0, words0, 624)
        torch.rand(1)
        raw, words, one = torch_rng._read_state()
        assert one == 1 and not np.array_equal(words, words0)
        for pos in (0, 1, 623, 624):
            for n in (0, 1, 623, 624, 625, 1500):
                if pos == 0:
                    torch_rng._write_state(raw0, words0, 624)
                else:
                    torch_rng._write_state(raw, words, pos)
                u = torch.rand(n)
                _, end_words, end_pos = torch_rng._read_state()
                if pos == 0 and n == 0:
                    end_words, end_pos = words, 0
                for a, addend in enumerate((0.0, 0.9, 1.0)):
                    keep = torch.floor(addend + u).type(torch.bool).numpy().astype(np.uint8)
                    for outs in ("uk", "u", "k"):
                        p = f"p{pos}.n{n}.a{a}.{outs}."
                        pmt = sc.load(p + "mt", words)
                        ppos = sc.load(p + "pos", np.asarray([pos], dtype=np.int32))
                        pu = sc.buf(p + "u", "f32", n) if "u" in outs else "null"
                        pk = sc.buf(p + "k", "u8", n) if "k" in outs else "null"
                        sc.call(p + "call", "srh_mt19937_uniform_f32", pmt, ppos, i(n), pu, fb(addend), pk)
                        want[p] = (u.numpy(), keep, end_words.copy(), end_pos, outs)
    mt, pos1 = sc.buf("mt", "u32", 624), sc.buf("pos", "i32", 1)
    bad = {"null_state": ("null", pos1, i(1)), "null_pos": (mt, "null", i(1)), "neg_n": (mt, pos1, i(-1)),
           "neg_pos": (mt, sc.load("posm1", np.asarray([-1], dtype=np.int32)), i(1)),
           "far_pos": (mt, sc.load("pos625", np.asarray([625], dtype=np.int32)), i(1))}
    for label, (a, b, c) in bad.items():
        sc.call(label, "srh_mt19937_uniform_f32", a, b, c, sc.buf(label + ".u", "f32", 1), fb(0.0), "null")
    res, = run_everywhere(drivers, tmp_path, sc)
    for p, (u, keep, end_words, end_pos, outs) in want.items():
        assert res.rc(p + "call") == 0
        if "u" in outs:
            assert res.a[p + "u"].tobytes() == u.tobytes(), p
        if "k" in outs:
            assert np.array_equal(res.a[p + "k"], keep), p
        assert np.array_equal(res.a[p + "mt"], end_words) and res.a[p + "pos"][0] == end_pos, p
    for label in bad:
        assert res.rc(label) == INVALID and res.s[label][1] and not res.a[label + ".u"].any()


# ---------------------------------------------------------------------------------------------------------------------------
# the loader
# ---------------------------------------------------------------------------------------------------------------------------
def add_dataset(sc, p, train, test, nulls=False):
    """Load, sizes, ids (every array exactly as long as srh_dataset_sizes says), names in both forms, destroy."""
    sc.call(p + "load", "srh_dataset_load", "&h:d", s(train), s(test))
    sizes = sc.buf(p + "sizes", "i64", 5)
    sc.call(p + "sizes", "srh_dataset_sizes", "h:d", sizes)
    counts = [f"{p}sizes[2]"] * 3 + [f"{p}sizes[3]"] * 2
    kinds = ("tu", "i32"), ("ti", "i32"), ("tw", "f32"), ("su", "i32"), ("si", "i32")
    sc.call(p + "ids", "srh_dataset_copy_ids", "h:d", *[sc.buf(p + n, d, c) for (n, d), c in zip(kinds, counts)])
    for k in range(5 if nulls else 0):                                   # each pointer null in turn
        outs = [sc.buf(f"{p}z{k}.{n}", d, c) if m != k else "null" for m, ((n, d), c) in enumerate(zip(kinds, counts))]
        sc.call(f"{p}z{k}.ids", "srh_dataset_copy_ids", "h:d", *outs)
    for which in (0, 1):
        q = f"{p}w{which}."
        sc.call(q + "bytes", "srh_dataset_names_bytes", "h:d", i(which))
        sc.call(q + "names", "srh_dataset_copy_names", "h:d", i(which), sc.buf(q + "chars", "u8", f"${q}bytes"),
                sc.buf(q + "off", "i64", f"{p}sizes[{which}]+1"))
        sc.call(q + "joined", "srh_dataset_copy_names", "h:d", i(which), sc.buf(q + "lines", "u8", f"${q}bytes+{p}sizes[{which}]"), "null")
    sc.call(p + "destroy", "srh_dataset_destroy", "h:d")


def python_dataset(train, test):
    """selfrec_amd/data/loader.py's line parser, then reference data/ui_graph.py:29-45: ids by first appearance, test pairs
    kept when both ends were seen in training.  Blank test lines are skipped (they are no interactions)."""
    users, items, tu, ti, tw = {}, {}, [], [], []
    for u, it, w in py_loader._read_triples(train):
        tu.append(users.setdefault(u, len(users)))
        ti.append(items.setdefault(it, len(items)))
        tw.append(w)
    su, si, lines = [], [], 0
    if test is not None:
        with open(test) as src:
            for raw in src:
                parts = raw.strip().split(' ')
                if len(parts) < 3:
                    continue
                lines += 1
                if parts[0] in users and parts[1] in items:
                    su.append(users[parts[0]])
                    si.append(items[parts[1]])
    return {"users": list(users), "items": list(items), "tu": tu, "ti": ti, "tw": np.asarray(tw, dtype=np.float32), "su": su,
            "si": si, "test_lines": lines}


def check_dataset(res, p, want, nulls=False):
    for label in ("load", "sizes", "ids", "w0.names", "w0.joined", "w1.names", "w1.joined"):
        assert res.rc(p + label) == 0, (p, label, res.s[p + label])
    assert res.a[p + "sizes"].tolist() == [len(want["users"]), len(want["items"]), len(want["tu"]), len(want["su"]), want["test_lines"]], p
    for n in ("tu", "ti", "su", "si"):
        assert res.a[p + n].tolist() == want[n], (p, n)
    assert res.a[p + "tw"].tobytes() == want["tw"].tobytes(), p
    for k in range(5 if nulls else 0):
        assert res.rc(f"{p}z{k}.ids") == 0
        for m, n in enumerate(("tu", "ti", "tw", "su", "si")):
            assert m == k or res.a[f"{p}z{k}.{n}"].tobytes() == res.a[p + n].tobytes()
    for which, names in ((0, want["users"]), (1, want["items"])):
        q = f"{p}w{which}."
        assert res.rc(q + "bytes") == sum(len(n.encode()) for n in names)
        assert res.a[q + "chars"].tobytes() == "".join(names).encode()
        assert res.a[q + "off"].tolist() == np.concatenate([[0], np.cumsum([len(n.encode()) for n in names])]).tolist()
        assert res.a[q + "lines"].tobytes() == "".join(n + "\n" for n in names).encode()


def loader_files(root):
    """name -> (train text, test text | None | a path that does not exist): the edge files of the loader."""
    rng = np.random.default_rng(31)
    f = {}
    f["empty"] = (b"", None)
    f["empty_with_test"] = (b"", b"a b 1\n")
    f["one_line_no_newline"] = (b"u1 i1 1", b"u1 i1 1")
    f["crlf"] = (b"u1 i1 1\r\nu2 i1 0.5\r\nu1 i2 2.5e0\r\n", b"u2 i2 1\r\n\r\nu3 i1 1\r\n")
    f["blanks_and_fourth_column"] = (b"  u1 i1 1  \n\tu2 i2 0.5 extra column\nu3 i1 1 \t\n u1 i3 2.5e0 9 9\n", b" u3 i3 1 x\n   \nu2 i9 1\n\n")
    long63 = b"0.5" + b"0" * 60
    long64 = b"2.5" + b"0" * 61
    long70 = b"1.25" + b"0" * 66
    assert (len(long63), len(long64), len(long70)) == (63, 64, 70)
    f["weights"] = (b"\n".join(b"u%d i%d %s" % (k, k % 3, w) for k, w in enumerate((b"1", b"0.5", b"2.5e0", long63, long64, long70, b"1"))) + b"\n", None)
    names = [b"x" * n for n in (7, 8, 9, 16, 17)] + [b"y" * n for n in (7, 8, 9, 16, 17)] + [b"x" * 7 + b"z", b"x" * 15 + b"z", b"x" * 16 + b"z"]
    f["name_lengths"] = (b"".join(b"%s %s 1\n" % (a, b) for a in names for b in names[::-1]),
                         b"".join(b"%s %s 1\n" % (a, b) for a, b in zip(names, names[3:] + [b"x" * 18] * 3)))
    # 2 600 users and 2 700 items: the 2^10-slot piece tables grow (at 615 names) at every thread count up to 4, the 2^12-slot
    # partition tables (at 2 458) at one thread; names repeat across pieces and many first appear late
    n = 9000
    us = np.minimum(rng.integers(0, 2600, n), rng.integers(0, 5200, n) % 2600)
    its = rng.integers(0, 2700, n)
    us[:2600] = rng.permutation(2600)
    its[-2700:] = rng.permutation(2700)
    train = b"".join(b"user%d it%d %s\n" % (a, b, (b"1", b"0.25", b"3")[(a + b) % 3]) for a, b in zip(us.tolist(), its.tolist()))
    test = b"".join(b"user%d it%d 1\n" % (a, b) for a, b in zip(rng.integers(0, 2700, 800).tolist(), rng.integers(0, 2800, 800).tolist()))
    f["many_names"] = (train, test + b"\n\nnobody it1 1\nuser1 nothing 1\n")
    fixed = b"".join(b"u%02d %d 1\n" % (k % 50, k % 7) for k in range(64))                 # 64 lines of 8 bytes
    assert len(fixed) == 512 and fixed[255:256] == b"\n" and fixed[127:128] == b"\n"       # halves and quarters start lines
    f["cuts_at_line_starts"] = (fixed, fixed[:80])
    onnl = b"abcdefgh ijklmn 1\n" + fixed                                                      # the half-way cut IS a '\n'
    assert onnl[len(onnl) // 2:len(onnl) // 2 + 1] == b"\n"
    f["cut_on_a_newline"] = (onnl, onnl[:60])
    f["long_last_line"] = (b"a b 1\nc d 1\n" + b"L" * 3000 + b" " + b"M" * 2000 + b" 0.5", b"a d 1\n" + b"L" * 3000 + b" b 1")
    f["test_without_lines"] = (b"a b 1\n", b"")
    f["test_of_blank_lines"] = (b"a b 1\n", b"\n \n\r\n")
    f["no_test_path"] = (b"a b 1\nc b 1\n", None)
    f["missing_test_file"] = (b"a b 1\nc b 1\n", os.path.join(root, "no_such_file.txt"))
    paths = {}
    for name, (train, test) in f.items():
        tr = os.path.join(root, name + ".train.txt")
        with open(tr, "wb") as out:
            out.write(train)
        te = test
        if isinstance(test, bytes):
            te = os.path.join(root, name + ".test.txt")
            with open(te, "wb") as out:
                out.write(test)
        paths[name] = (tr, te)
    return paths


def test_loader_edge_files(drivers, tmp_path):
    """Every edge file at 1, 2, 3, 4, 7, 32 and 256 threads (more threads than lines) against the python path -- which does
    not know about threads, so every thread count gives the 1-thread result: sizes, ids, weights bit for bit, kept test pairs,
    the count of test lines, names in both forms, copy_ids with each pointer null in turn."""
    paths = loader_files(str(tmp_path))
    sc = Script(tmp_path)
    for t in LOADER_THREADS:
        sc.setenv("SRH_LOADER_THREADS", t)
        for name, (tr, te) in paths.items():
            p = f"t{t}.{name}."
            if name == "missing_test_file":
                sc.call(p + "load", "srh_dataset_load", "&h:d", s(tr), s(te))
            else:
                add_dataset(sc, p, tr, te, nulls=name != "many_names" or t == 3)
    res, = run_everywhere(drivers, tmp_path, sc)
    for name, (tr, te) in paths.items():
        if name == "missing_test_file":
            for t in LOADER_THREADS:
                rc, msg = res.s[f"t{t}.{name}.load"]
                assert rc == INVALID and msg == f"dataset_load: cannot read {te}"
            continue
        want = python_dataset(tr, te)
        for t in LOADER_THREADS:
            check_dataset(res, f"t{t}.{name}.", want, nulls=name != "many_names" or t == 3)
    w = res.a["t1.weights.tw"]
    assert w.tolist() == [1.0, 0.5, 2.5, 0.5, 2.5, 1.25, 1.0]
    assert res.a["t4.empty.sizes"].tolist() == [0, 0, 0, 0, 0] and res.a["t4.no_test_path.sizes"].tolist() == [2, 1, 2, 0, 0]
    assert res.a["t7.test_of_blank_lines.sizes"].tolist() == [1, 1, 1, 0, 0]


def test_loader_reports_the_global_line_of_a_malformed_line(drivers, tmp_path):
    """A blank or two-token line in piece 0 and in a later piece: the line number in the message counts from the start of
    the FILE at every thread count; the half-built dataset is freed (leak checking is on).  Missing files and null arguments
    are refused."""
    good = [b"user%d item%d 1" % (k % 37, k % 11) for k in range(400)]
    bad_at = {"blank_first_piece": (3, b""), "two_tokens_first_piece": (10, b"two tokens"), "blank_late": (371, b"   "),
              "two_tokens_late": (399, b"only two"), "one_token_middle": (200, b"lonely")}
    paths = {}
    for name, (at, text) in bad_at.items():
        lines = list(good)
        lines[at] = text
        paths[name] = os.path.join(str(tmp_path), name + ".txt")
        with open(paths[name], "wb") as out:
            out.write(b"\n".join(lines) + b"\n")
    missing = os.path.join(str(tmp_path), "missing.txt")
    sc = Script(tmp_path)
    for t in LOADER_THREADS:
        sc.setenv("SRH_LOADER_THREADS", t)
        for name, path in paths.items():
            sc.call(f"t{t}.{name}", "srh_dataset_load", "&h:d", s(path), "null")
        sc.call(f"t{t}.missing", "srh_dataset_load", "&h:d", s(missing), "null")
    sc.call("null_out", "srh_dataset_load", "null", s(paths["blank_late"]), "null")
    sc.call("null_path", "srh_dataset_load", "&h:d", "null", "null")
    sc.call("sizes.null_handle", "srh_dataset_sizes", "null", sc.buf("sizes", "i64", 5))
    sc.call("ids.null_handle", "srh_dataset_copy_ids", "null", "null", "null", "null", "null", "null")
    sc.call("bytes.null_handle", "srh_dataset_names_bytes", "null", i(0))
    sc.call("names.null_handle", "srh_dataset_copy_names", "null", i(0), sc.buf("chars", "u8", 4), "null")
    good_path = os.path.join(str(tmp_path), "good.txt")
    with open(good_path, "wb") as out:
        out.write(b"a b 1\n")
    sc.call("load", "srh_dataset_load", "&h:d", s(good_path), "null")
    sc.call("sizes.null_out", "srh_dataset_sizes", "h:d", "null")
    sc.call("names.null_buf", "srh_dataset_copy_names", "h:d", i(0), "null", "null")
    sc.call("destroy", "srh_dataset_destroy", "h:d")
    sc.call("destroy.null", "srh_dataset_destroy", "null")
    res, = run_everywhere(drivers, tmp_path, sc)
    for t in LOADER_THREADS:
        for name, (at, _) in bad_at.items():
            rc, msg = res.s[f"t{t}.{name}"]
            assert rc == INVALID and msg == f"dataset_load: {paths[name]} line {at + 1} does not have the form 'user item weight'", (t, name)
            with pytest.raises((IndexError, ValueError)):
                py_loader._read_triples(paths[name])                       # the python path refuses the file too
        assert res.s[f"t{t}.missing"] == (INVALID, f"dataset_load: cannot read {missing}")
    for label in ("null_out", "null_path", "sizes.null_handle", "ids.null_handle", "names.null_handle", "sizes.null_out", "names.null_buf"):
        assert res.rc(label) == INVALID and res.s[label][1], label
    assert res.rc("bytes.null_handle") == 0 and res.rc("load") == 0
