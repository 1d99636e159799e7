"""Deterministic structures that put every schedule and tail edge of csrc/spmm.hip under the per-element bounds of
tests/spmm_ref.py -- TEST INFRASTRUCTURE ONLY, host numpy / scipy, seeded.  tests/test_spmm_cases_cpu.py checks, without a
GPU, that the structures contain what their names say; tests/test_gpu_spmm_schedule_edges.py runs the kernels on them.

Every builder returns a Case: raw indptr / indices / vals, a shape and a name.  Indices are NOT sorted within a row (some
cases fix the stored order), so the arrays go to ops.DeviceCSR(...) directly; Case.scipy() is the float64 matrix for the
restatement, which does not care about the order.

The second half restates the plan's SEGMENTATION and wave packing from the words of include/selfrec_hip.h and of the
comment above spmm_rows_kernel, not from srh_spmm_plan_create:
  * per row, and per part of a row cut at row_mid, pieces of at most split_len entries; a row that stays one piece is a
    plain segment, a row of more than one piece gives each a slot (segmentation);
  * a plain segment of at most SHORT_ROW entries is a short row, G of them per wave, longest first; every other segment
    has a wave to itself and walks chunks of CH = 16 G entries, a chunk of `rem` entries in ceil(rem / G) rounds.
"""
import functools
from collections import namedtuple

import numpy as np
import scipy.sparse as sp

SHORT_ROW = 64                                  # a whole row of at most this many entries shares its wave with G - 1 others
DEFAULT_SPLIT = 512                             # what split_len = 0 means
LADDER_COLS = 1600
LADDER_LONG = (191, 192, 193, 511, 512, 513, 575, 576, 577, 1023, 1024, 1025, 1537)
LIVE_CYCLE = (0, 16, 1, 13, 4, 12, 5, 9, 8)    # live entries per block of 16 stored positions, taken cyclically
LIVE_ROWS = (16, 32, 48, 64, 80, 128, 192, 640)
MIXED_SMALL = (64, 1, 0, 33, 16, 17, 0, 8, 9)


class Case(namedtuple("Case", "name indptr indices vals shape")):
    def scipy(self):
        """float64 CSR of the case (a copy; the order of a row's entries does not matter to it)"""
        return sp.csr_matrix((self.vals.astype(np.float64), self.indices.copy(), self.indptr.copy()), shape=self.shape)

    @property
    def lens(self):
        return np.diff(self.indptr)


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


def _case(name, lens, n_cols, seed, last_col_row=None):
    """rows of the given lengths: distinct random columns in random (unsorted) order, standard normal non-zero values;
    last_col_row: a row whose last stored entry names column n_cols - 1"""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, dtype=np.int64)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    indices = np.zeros(int(lens.sum()), dtype=np.int32)
    for r, n in enumerate(lens):
        cols = rng.choice(n_cols, size=int(n), replace=False)
        if r == last_col_row and n:
            cols = np.concatenate([cols[cols != n_cols - 1][:n - 1], [n_cols - 1]])
        indices[indptr[r]:indptr[r + 1]] = cols
    vals = rng.standard_normal(indices.size).astype(np.float32)
    vals[vals == 0] = 1.0
    _freeze(indptr, indices, vals)
    return Case(name, indptr, indices, vals, (int(lens.size), int(n_cols)))


@functools.lru_cache(maxsize=None)
def ladder(n_cols=LADDER_COLS):
    """One row of every length 0 .. 130 and of LADDER_LONG; a seeded permutation deals the lengths to the row ids, then
    row 0 takes 130 entries, the last row 513 and a middle row none."""
    rng = np.random.default_rng(20)
    lens = rng.permutation(np.array(list(range(131)) + list(LADDER_LONG), dtype=np.int64))
    n = lens.size

    def put(row, length):
        at = int(np.flatnonzero(lens == length)[0])
        lens[at], lens[row] = lens[row], lens[at]
    put(0, 130)
    put(n - 1, 513)
    put(n // 2, 0)
    return _case("ladder", lens, n_cols, seed=21, last_col_row=0)


@functools.lru_cache(maxsize=None)
def mixed_small():
    """nine rows whose neighbours differ widely in length: at every width a wave of unlike rows and a last task of fewer than
    G rows"""
    return _case("mixed-small", MIXED_SMALL, 97, seed=22, last_col_row=3)


@functools.lru_cache(maxsize=None)
def short_quads():
    """Four rows of every length 1 .. 32, row ids shuffled.  Longest first and G to a wave, the ladder's short rows give a
    wave's longest row every length only at G = 1 (multiples of 2 and 4 at G = 2 and 4); here a wave of 4, 2 or 1 rows
    has every longest length 1 .. 32, so an UNMASKED launch runs every tail of 1 .. 16 rounds as a first and as a second
    chunk."""
    rng = np.random.default_rng(23)
    return _case("short-quads", rng.permutation(np.repeat(np.arange(1, 33), 4)), 211, seed=24, last_col_row=5)


TINY_LENS = {1: ((1,), (65,), (0,)),
             2: ((0, 0), (0, 70), (3, 64)),
             3: ((0, 0, 0), (65, 0, 1), (2, 129, 0)),
             4: ((16, 17, 0, 64), (0, 0, 0, 200)),
             5: ((1, 2, 3, 4, 5), (0, 0, 0, 0, 0), (0, 0, 130, 0, 0))}


@functools.lru_cache(maxsize=None)
def tiny(k):
    """The structures of k = 1 .. 5 rows: a single row of 1 and of 65 entries, all rows empty (no stored entry at all), one
    row holding every entry.  Rectangular, and the first row that has an entry names column n_cols - 1."""
    out = []
    for t, lens in enumerate(TINY_LENS[k]):
        full = [r for r, n in enumerate(lens) if n]
        out.append(_case(f"tiny{k}-" + "-".join(map(str, lens)), lens, 211 + k, seed=100 * k + t,
                         last_col_row=full[0] if full else None))
    return tuple(out)


def tiny_all():
    return tuple(c for k in sorted(TINY_LENS) for c in tiny(k))


# ------------------------------------------------------------------------------------------------------------------
# live_block_case: the column-masked flavour's live-entry compaction
# ------------------------------------------------------------------------------------------------------------------
LiveCase = namedtuple("LiveCase", "case col_live block_live")       # block_live[r]: live entries of row r's blocks of 16


def _block_pattern(n_live, kind, size=16):
    """which of `size` consecutive positions are live: first, last, or spread over the block"""
    live = np.zeros(size, dtype=bool)
    n_live = min(n_live, size)
    if kind == 0:
        live[:n_live] = True
    elif kind == 1:
        live[size - n_live:] = True
    else:
        live[(np.arange(n_live) * size) // max(n_live, 1)] = True
    return live


@functools.lru_cache(maxsize=None)
def live_block_case(d):
    """Rows of LIVE_ROWS entries over 1400 columns of which the even ones are live.  Block b (16 consecutive stored
    positions from the row's start -- also from a piece's, every piece starting at a multiple of 64) takes the next
    count of LIVE_CYCLE, the cycle running on from row to row: neighbouring blocks of a row AND the same block of
    neighbouring rows differ, and the four short rows (ten blocks) already hold all nine counts.
    They sit first in the block, last, or interleaved, in turn.  The structure is the same at every width; d seeds the
    columns and values."""
    rng = np.random.default_rng(300 + d)
    n_cols = 1400
    lens = np.array(LIVE_ROWS, dtype=np.int64)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    indices = np.zeros(int(lens.sum()), dtype=np.int32)
    block_live, taken = [], 0
    for k, n in enumerate(lens):
        counts = [LIVE_CYCLE[(taken + b) % len(LIVE_CYCLE)] for b in range(int(n) // 16)]
        taken += len(counts)
        live = np.concatenate([_block_pattern(c, (k + b) % 3) for b, c in enumerate(counts)])
        even = 2 * rng.choice(n_cols // 2, size=int(live.sum()), replace=False)
        odd = 2 * rng.choice(n_cols // 2, size=int((~live).sum()), replace=False) + 1
        cols = np.empty(int(n), dtype=np.int64)
        cols[live], cols[~live] = even, odd
        indices[indptr[k]:indptr[k + 1]] = cols
        block_live.append(tuple(counts))
    vals = rng.standard_normal(indices.size).astype(np.float32)
    vals[vals == 0] = 1.0
    col_live = np.arange(n_cols) % 2 == 0
    _freeze(indptr, indices, vals, col_live)
    return LiveCase(Case(f"live-blocks-d{d}", indptr, indices, vals, (int(lens.size), n_cols)), col_live, tuple(block_live))


# ------------------------------------------------------------------------------------------------------------------
# class_cases: row_mid / xcd_split_row on the ladder's structure
# ------------------------------------------------------------------------------------------------------------------
ClassCase = namedtuple("ClassCase", "name case row_mid xcd_split_row")
ALL_EVEN_LENS, ALL_ODD_LENS = (5, 64, 65, 100), (7, 63, 66, 128)      # rows forced into one column class
ONE_EVEN_LEN, ONE_ODD_LEN = 130, 129                                 # rows with exactly one column of a class


def column_class_order(indptr, indices, min_len):
    """selfrec_amd.ops.column_class_order (pure numpy; imported late: the package is not needed by the other builders)"""
    from selfrec_amd.ops.sparse import column_class_order as order
    return order(indptr, indices, min_len)


@functools.lru_cache(maxsize=None)
def class_cases():
    """-> tuple of ClassCase.  "mid": the ladder with ALL_EVEN_LENS rows all-even (mid = len), ALL_ODD_LENS rows all-odd
    (mid = 0), the 130-entry row with exactly one even column (mid = 1: pieces 1 + 3 under split_len 64) and the 129-entry
    row with exactly one odd one (mid = len - 1), stored [even | odd] by column_class_order(min_len=1).  "whole-1": every
    row whole in class 1 (class 0 has nothing: its workgroups go to the other list at once).  "whole-mix": -1 and -2 in
    turn.  Each under xcd_split_row in {0, 1, n // 2, n - 1, n}."""
    base = ladder()
    rng = np.random.default_rng(40)
    n, n_cols = base.shape
    lens = base.lens
    indices = base.indices.copy()
    even_cols, odd_cols = np.arange(0, n_cols, 2), np.arange(1, n_cols, 2)

    def refill(length, n_even):
        r = int(np.flatnonzero(lens == length)[0])
        cols = np.concatenate([rng.choice(even_cols, n_even, replace=False), rng.choice(odd_cols, length - n_even, replace=False)])
        indices[base.indptr[r]:base.indptr[r + 1]] = rng.permutation(cols)
    for length in ALL_EVEN_LENS:
        refill(length, length)
    for length in ALL_ODD_LENS:
        refill(length, 0)
    refill(ONE_EVEN_LEN, 1)
    refill(ONE_ODD_LEN, ONE_ODD_LEN - 1)
    perm, row_mid = column_class_order(base.indptr, indices, 1)
    mid_indices, mid_vals = indices[perm].astype(np.int32), base.vals[perm]
    _freeze(mid_indices, mid_vals, row_mid)
    mid_case = Case("ladder-classes", base.indptr, mid_indices, mid_vals, base.shape)
    whole1 = np.full(n, -2, dtype=np.int32)
    mix = np.where(np.arange(n) % 2 == 0, -1, -2).astype(np.int32)
    _freeze(whole1, mix)
    out = []
    for split_row in (0, 1, n // 2, n - 1, n):
        out.append(ClassCase(f"mid-xcd{split_row}", mid_case, row_mid, split_row))
        out.append(ClassCase(f"whole-1-xcd{split_row}", base, whole1, split_row))
        out.append(ClassCase(f"whole-mix-xcd{split_row}", base, mix, split_row))
    return tuple(out)


# ------------------------------------------------------------------------------------------------------------------
# The plan's segmentation and wave packing, restated
# ------------------------------------------------------------------------------------------------------------------
Piece = namedtuple("Piece", "row part start end slot")              # slot -1: a plain segment (the whole row)


def segmentation(indptr, split_len=0, row_mid=None):
    """-> list of Piece in row order.  split_len 0 = DEFAULT_SPLIT.  row_mid[r] = m with 0 < m < len: the row has two
    parts, [0, m) and [m, len); m = 0, m = len and negative m leave it one part.  Every part is cut into pieces of at
    most split_len entries; the only piece of a row is plain, several pieces take consecutive slots."""
    split = int(split_len) or DEFAULT_SPLIT
    out, slot = [], 0
    for r in range(len(indptr) - 1):
        s, e = int(indptr[r]), int(indptr[r + 1])
        m = -1 if row_mid is None else int(row_mid[r])
        parts = [(s, s + m), (s + m, e)] if 0 < m < e - s else [(s, e)]
        cut = [(k, a, min(a + split, pe)) for k, (ps, pe) in enumerate(parts) for a in range(ps, max(pe, ps + 1), split)]
        if len(cut) == 1:
            out.append(Piece(r, 0, s, e, -1))
            continue
        for k, a, b in cut:
            out.append(Piece(r, k, a, b, slot))
            slot += 1
    return out


def is_short(p):
    return p.slot < 0 and p.end - p.start <= SHORT_ROW


def short_waves(pieces, G):
    """the short rows, longest first (ties in row order), G to a wave -> list of lists of Piece (no row classes)"""
    shorts = sorted((p for p in pieces if is_short(p)), key=lambda p: -(p.end - p.start))
    return [shorts[k:k + G] for k in range(0, len(shorts), G)]


def coop_pieces(pieces):
    return [p for p in pieces if not is_short(p)]


def coop_tail_rounds(length, G):
    """rounds (1 .. 16) of each chunk of a cooperative segment of `length` entries at G row-groups per wave"""
    ch = 16 * G
    return [min(16, -(-(length - base) // G)) for base in range(0, length, ch)]


def short_tail_rounds(maxlen):
    """rounds (1 .. 16) of each chunk of a wave of short rows whose longest has maxlen entries"""
    return [min(16, maxlen - 16 * q) for q in range(-(-maxlen // 16))]


def row_masks(case, split_len, G):
    """Three row masks for a row-masked launch at G short rows per wave.  Over the three, every wave of short rows is
    once all dead, once all live and once has ONE live row -- row (w // (16 // G)) % G of wave w, so that the live row's
    length, which is then the wave's longest, takes every residue of 16 over the ladder.  Split and long rows are dead in
    one mask and live in the two others, in turn."""
    n = case.shape[0]
    pieces = segmentation(case.indptr, split_len)
    masks = np.zeros((3, n), dtype=bool)
    for w, wave in enumerate(short_waves(pieces, G)):
        one = wave[min((w // max(16 // G, 1)) % G, len(wave) - 1)].row
        for t in range(3):
            kind = (w + t) % 3                                       # 0: all dead, 1: one live, 2: all live
            for p in wave:
                masks[t, p.row] = kind == 2 or (kind == 1 and p.row == one)
    for k, r in enumerate(sorted({p.row for p in coop_pieces(pieces)})):
        for t in range(3):
            masks[t, r] = (k + t) % 3 != 0
    _freeze(masks)
    return masks
