"""The premises of tests/test_gpu_spmm_schedule_edges.py, checked without a GPU: the structures of tests/spmm_cases.py contain
the row lengths, piece lengths, tail rounds, live-entry counts and class layouts they are named for (through the restated
segmentation of that file), and the float64 restatement alone meets the conditions the GPU test carries."""
import numpy as np
import pytest

from . import spmm_cases as K

ROUNDS = set(range(1, 17))


def _piece_lens(pieces, slotted):
    return {p.end - p.start for p in pieces if (p.slot >= 0) == slotted}


def test_ladder_holds_every_length_and_every_piece():
    c = K.ladder()
    lens = c.lens
    assert c.shape == (144, 1600) and sorted(lens.tolist()) == sorted(list(range(131)) + list(K.LADDER_LONG))
    assert lens[0] == 130 and lens[-1] == 513 and lens[c.shape[0] // 2] == 0 and c.indices.size < 20000
    assert c.indices[c.indptr[1] - 1] == c.shape[1] - 1
    for r in range(c.shape[0]):
        cols = c.indices[c.indptr[r]:c.indptr[r + 1]]
        assert np.unique(cols).size == cols.size and (cols >= 0).all() and (cols < c.shape[1]).all()
    assert any(np.any(np.diff(c.indices[c.indptr[r]:c.indptr[r + 1]]) < 0) for r in range(c.shape[0]))       # unsorted rows
    assert np.all(c.vals != 0)
    s64, s512 = K.segmentation(c.indptr, 64), K.segmentation(c.indptr, 0)
    for pieces in (s64, s512):          # the pieces of a row tile it, in order, and slots are consecutive
        at = dict()
        for p in pieces:
            assert p.start == at.get(p.row, c.indptr[p.row]) and p.start <= p.end
            at[p.row] = p.end
        assert all(at[r] == c.indptr[r + 1] for r in range(c.shape[0]))
        slots = [p.slot for p in pieces if p.slot >= 0]
        assert slots == list(range(len(slots)))
    # split 64: every length 65 .. 128 is a full piece plus one of 1 .. 64 entries
    assert _piece_lens(s64, True) == set(range(1, 65)) and _piece_lens(s64, False) == set(range(65))
    two = {r: [p for p in s64 if p.row == r] for r in np.flatnonzero((lens >= 65) & (lens <= 128))}
    assert {(v[0].end - v[0].start, v[1].end - v[1].start) for v in two.values()} == {(64, k) for k in range(1, 65)}
    # default split: plain segments of every length 0 .. 130, last pieces of 1, 65 and 1 entries behind full ones
    assert set(range(131)) <= _piece_lens(s512, False) and {1, 65, 512} <= _piece_lens(s512, True)
    last = {int(lens[p.row]): p.end - p.start for p in s512 if p.slot >= 0}
    assert (last[513], last[577], last[1025], last[1537]) == (1, 65, 1, 1)


@pytest.mark.parametrize("split_len", [64, 0])
@pytest.mark.parametrize("G", [4, 2, 1])
def test_cooperative_chunks_run_every_tail_round(G, split_len):
    c = K.ladder()
    coop = K.coop_pieces(K.segmentation(c.indptr, split_len))
    rounds = {r for p in coop for r in K.coop_tail_rounds(p.end - p.start, G)}
    assert rounds == ROUNDS
    lens = {p.end - p.start for p in coop}
    ch = 16 * G
    # a cooperative segment of one entry, of one chunk and of one chunk plus one (the last: a piece where it fits a piece
    # of 64, else the whole 65-entry row of the default split)
    assert ({1, ch} <= lens and (ch + 1 in lens or ch == 64)) if split_len else ch + 1 in lens or ch < 64
    # the 64 / 65 boundary between a short row and a cooperative one
    whole = {p.end - p.start for p in coop if p.slot < 0}
    assert 64 not in whole and (65 in whole) == (split_len == 0)


@pytest.mark.parametrize("G", [4, 2, 1])
def test_short_row_waves_run_every_tail_round(G):
    """unmasked launches: the ladder alone at one row per wave, with short_quads at two and four; row-masked launches:
    the ladder under row_masks, whose one-live waves make every length the longest of its wave"""
    def tails(case):
        return {r for w in K.short_waves(K.segmentation(case.indptr, 0), G)
                for r in K.short_tail_rounds(max(p.end - p.start for p in w))}
    assert tails(K.short_quads()) == ROUNDS
    if G == 1:
        assert tails(K.ladder()) == ROUNDS
    assert 9 in tails(K.mixed_small())
    c = K.ladder()
    masked = set()
    for mask in K.row_masks(c, 64, G):
        for w in K.short_waves(K.segmentation(c.indptr, 64), G):
            live = [p.end - p.start for p in w if mask[p.row]]
            masked |= set(K.short_tail_rounds(max(live))) if live else set()
    assert masked == ROUNDS


@pytest.mark.parametrize("G", [16, 8, 4, 2, 1])
def test_row_masks_visit_every_wave_dead_single_and_live(G):
    for case in (K.ladder(), K.mixed_small(), K.short_quads()) + K.tiny_all():
        for split_len in (64, 0):
            pieces = K.segmentation(case.indptr, split_len)
            masks = K.row_masks(case, split_len, G)
            for w in K.short_waves(pieces, G):
                counts = sorted(int(sum(m[p.row] for p in w)) for m in masks)
                assert counts == sorted([0, 1, len(w)]), (case.name, G)
            heavy = sorted({p.row for p in K.coop_pieces(pieces)})
            if len(heavy) >= 2:
                assert all((~m[heavy]).any() and m[heavy].any() for m in masks[:min(3, len(heavy))]), case.name
    split = sorted({p.row for p in K.segmentation(K.ladder().indptr, 64) if p.slot >= 0})
    assert all((~m[split]).any() and m[split].any() for m in K.row_masks(K.ladder(), 64, G))


def test_small_structures_are_what_they_are_named():
    assert tuple(K.mixed_small().lens) == K.MIXED_SMALL
    for G in (16, 8, 4, 2):
        assert len(K.short_waves(K.segmentation(K.mixed_small().indptr, 0), G)[-1]) < G       # a last task with count < G
    names = set()
    for k in range(1, 6):
        for c in K.tiny(k):
            assert c.shape[0] == k and c.shape[1] != k
            if c.indices.size:
                assert c.indices.max() == c.shape[1] - 1
            names.add(tuple(c.lens))
    assert {(1,), (65,)} <= names
    assert all(any(len(t) == k and sum(t) == 0 for t in names) for k in (1, 2, 3, 5))          # no stored entry at all
    assert any(len(t) > 1 and sum(t) == max(t) > 0 for t in names)                             # one row holds every entry
    q = K.short_quads()
    assert sorted(q.lens.tolist()) == sorted(list(range(1, 33)) * 4)


@pytest.mark.parametrize("d", [8, 16, 32, 64, 128, 256])
def test_live_block_case_holds_every_live_count(d):
    lc = K.live_block_case(d)
    c = lc.case
    assert tuple(c.lens) == K.LIVE_ROWS and np.all(c.vals != 0)
    for r, counts in enumerate(lc.block_live):
        cols = c.indices[c.indptr[r]:c.indptr[r + 1]]
        assert np.unique(cols).size == cols.size
        got = lc.col_live[cols].reshape(-1, 16).sum(axis=1)
        assert tuple(got) == counts
    short = {n for r, cs in enumerate(lc.block_live) if c.lens[r] <= K.SHORT_ROW for n in cs}
    coop = {n for r, cs in enumerate(lc.block_live) if c.lens[r] > K.SHORT_ROW for n in cs}
    assert short == set(K.LIVE_CYCLE) and coop == set(K.LIVE_CYCLE)
    # first, last and interleaved placements all occur among the blocks that are neither empty nor full
    kinds = set()
    for r in range(c.shape[0]):
        live = lc.col_live[c.indices[c.indptr[r]:c.indptr[r + 1]]].reshape(-1, 16)
        for b in live:
            if 0 < b.sum() < 16:
                kinds.add("first" if b[:b.sum()].all() else "last" if b[16 - b.sum():].all() else "mixed")
    assert kinds == {"first", "last", "mixed"}
    # The rounds a wave issues follow its fullest block of 16 (<= 4, <= 8, <= 12, <= 16: arms 1 .. 4).  At every whole-row
    # width and both split lengths some cooperative chunk's fullest block holds exactly 13 -- the count whose last entry only
    # the fourth arm adds -- and the third and fourth arms run in cooperative chunks and in waves of short rows; the first
    # two need a chunk of few live entries, which four neighbours of LIVE_CYCLE never are: they run at one and two blocks
    # per chunk.
    arms = lambda ns: {(n + 3) // 4 for n in ns if n}      # noqa: E731
    seen = set()
    for G in (4, 2, 1):
        for split_len in (64, 0):
            nmax = set()
            for p in K.coop_pieces(K.segmentation(c.indptr, split_len)):
                blocks = lc.block_live[p.row][(p.start - c.indptr[p.row]) // 16:(p.end - c.indptr[p.row]) // 16]
                nmax |= {max(blocks[k:k + G]) for k in range(0, len(blocks), G)}
            assert 13 in nmax and {3, 4} <= arms(nmax), (G, split_len, nmax)
            seen |= arms(nmax)
        waves = K.short_waves(K.segmentation(c.indptr, 0), G)
        nshort = {max(lc.block_live[p.row][q] for p in w if p.end - p.start > 16 * q)
                  for w in waves for q in range(max(p.end - p.start for p in w) // 16)}
        assert {3, 4} <= arms(nshort), (G, nshort)
        seen |= arms(nshort)
    assert seen == {1, 2, 3, 4}


def test_class_cases_contain_what_their_names_say():
    cases = K.class_cases()
    n = K.ladder().shape[0]
    assert {cc.xcd_split_row for cc in cases} == {0, 1, n // 2, n - 1, n} and len(cases) == 15
    mid = next(cc for cc in cases if cc.name.startswith("mid-"))
    c, lens, rm = mid.case, mid.case.lens, mid.row_mid
    assert np.array_equal(c.indptr, K.ladder().indptr)
    assert sorted(zip(c.indices.tolist(), c.vals.tolist())) != [] and np.all(c.vals != 0)
    for r in range(n):
        cols = c.indices[c.indptr[r]:c.indptr[r + 1]]
        assert np.unique(cols).size == cols.size
        if lens[r]:
            assert 0 <= rm[r] <= lens[r] and np.all(cols[:rm[r]] % 2 == 0) and np.all(cols[rm[r]:] % 2 == 1)
        else:
            assert rm[r] < 0
    assert {int(lens[r]) for r in range(n) if lens[r] and rm[r] == lens[r]} >= set(K.ALL_EVEN_LENS)       # mid = len
    assert {int(lens[r]) for r in range(n) if lens[r] and rm[r] == 0} >= set(K.ALL_ODD_LENS)              # mid = 0
    one_even, one_odd = int(np.flatnonzero(lens == K.ONE_EVEN_LEN)[0]), int(np.flatnonzero(lens == K.ONE_ODD_LEN)[0])
    assert rm[one_even] == 1 and rm[one_odd] == lens[one_odd] - 1
    pieces = K.segmentation(c.indptr, 64, rm)
    per_part = lambda r: [sum(1 for p in pieces if p.row == r and p.part == k) for k in (0, 1)]      # noqa: E731
    assert per_part(one_even) == [1, 3] and per_part(one_odd) == [2, 1]                                 # unlike piece counts
    assert all(p.slot >= 0 for p in pieces if p.row in (one_even, one_odd))
    whole = next(cc for cc in cases if cc.name.startswith("whole-1-"))
    assert np.all(whole.row_mid == -2)
    mix = next(cc for cc in cases if cc.name.startswith("whole-mix-"))
    assert set(mix.row_mid.tolist()) == {-1, -2}


@pytest.mark.parametrize("d", [64, 128, 256])
def test_adam_hull_is_not_vacuous_on_the_cases(d):
    """the cap of test_spmm_adam_epilogue_matches_float64_adam, on the structures the schedule test runs ADAM on"""
    from .test_gpu_spmm_schedule_edges import ADAM_CASE, ADAM_HYPER, adam_reference
    for case in (K.ladder(), K.mixed_small(), K.short_quads()):
        w = adam_reference(case, d)[1]
        assert float(w["ill"].mean()) < 0.01, (case.name, float(w["ill"].mean()))
    assert ADAM_CASE["step"] >= 1 and len(ADAM_HYPER) == 4
