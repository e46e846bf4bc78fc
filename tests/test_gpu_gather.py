"""-m gpu: gather_pairs_kernel (csrc/gather_device.h) -- the kernel that feeds both DP stages and the string builder -- against a plain numpy
model (ngm_host_model.gather_pairs_model), through Mapper.debug_gather_pairs: the launch code of the score and align stages, on a mapper's own
q, corridor, reference and engine, with the read lengths measured as a batch's are.  Words, lens and blk_rows are compared exactly.

The read side is the point: reverse complement through two unaligned dword loads with a byte-wise path wherever the eight characters do not lie
inside the row (a reverse read whose length is no multiple of 8 has a word across its start; lengths from q - 7 on push a word across the row's
end), non-ACGT characters, the table bit of --bs-mapping / --slam-seq runs, lens, blk_rows and the dead lanes of a ragged last block.  The window
side runs along at the places DecodeRefSequence is odd: odd and even offsets, spacers, the genome's end, locations below half a corridor."""
import functools

import numpy as np
import pytest

import ngm_host_model as HM
import simulate as S

pytestmark = pytest.mark.gpu

SHAPES = [(102, 20), (152, 27), (32, 8)]   # q = 102: the last read word lies across the row's end


@functools.lru_cache(maxsize=None)
def _world():
    from nextgenmap_amd.pipeline import Reference
    contigs = S.make_genome([5000, 3001], seed=9, repeat_families=1, copies=1, n_runs=1)
    ref = Reference.from_contigs(contigs)
    g, geom, n_bases = HM.concat_genome(contigs)
    assert n_bases - 1 == ref.concat_len
    return ref, g, n_bases


@functools.lru_cache(maxsize=None)
def _mapper(q, c):
    from nextgenmap_amd.pipeline import Mapper
    return Mapper(_world()[0], q, c)


def _lengths(q):
    return [0, 1, 7, 8, 9, 15, 16, 17, q - 9, q - 8, q - 2, q - 1]


@functools.lru_cache(maxsize=None)
def _rows(q):
    """two reads of every length (an even and an odd read index each), then reads with N, lower case and an IUPAC code"""
    rng = np.random.default_rng(6100 + q)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    lens = [L for L in _lengths(q) for _ in (0, 1)]
    rows = np.zeros((len(lens) + 6, q), np.uint8)
    for i, L in enumerate(lens):
        rows[i, :L] = acgt[rng.integers(0, 4, L)]
    for i in range(len(lens), len(rows)):
        L = [q - 1, q - 3, 13, q - 10, 9, q - 6][i - len(lens)]
        r = acgt[rng.integers(0, 4, L)].copy()
        r[rng.integers(0, L, max(1, L // 6))] = ord("N")
        r[rng.integers(0, L, max(1, L // 6))] |= 0x20
        r[rng.integers(0, L, max(1, L // 8))] = ord("R")
        r[0], r[L - 1] = ord("n"), ord("R")   # (the read's two ends: the first and last character of a reversed word)
        rows[i, :L] = r
    return rows


def _locations(n_bases, c):
    concat = n_bases - 1
    rng = np.random.default_rng(6200 + c)
    inner = [int(x) for x in rng.integers(1000, 6000, 6)]
    return inner + [1001, 1002, 500, 6300, 6301,                                 # odd and even, inside the leading spacer and the one between the contigs
                    concat - 199, concat - 150, concat - 37, concat - 2,        # within 200 bases of the genome's end
                    concat - 1, concat + 7, 0, 1, (c >> 1) - 1, c >> 1]         # ... at and beyond it; below half a corridor (the offset wraps)


def _pairs(q, c, n_bases, n_pairs):
    """every read on both strands first (several pairs share a read), the locations in turn"""
    n_reads = len(_rows(q))
    locs = _locations(n_bases, c)
    p = np.arange(n_pairs)
    pair_read = (p // 2) % n_reads
    pair_sv = (p & 1) | (((p * 7) % 5) << 1)   # bit 0: the strand; the bits above it (votes in the product) are not the kernel's business
    pair_loc = np.array([locs[(k * 5 + k // len(locs)) % len(locs)] for k in p])
    return pair_read.astype(np.uint32), pair_loc.astype(np.uint32), pair_sv.astype(np.uint32)


def _check(q, c, n_pairs, alt_dir, align_stage):
    ref, g, n_bases = _world()
    rows = _rows(q)
    pair_read, pair_loc, pair_sv = _pairs(q, c, n_bases, n_pairs)
    words, lens, blk_rows, rw, fw = _mapper(q, c).debug_gather_pairs(rows, pair_read, pair_loc, pair_sv, alt_dir=alt_dir, align_stage=align_stage)
    m_words, m_lens, m_rows = HM.gather_pairs_model(g, n_bases, rows, pair_read, pair_loc, pair_sv, q, c, rw, fw, alt_dir=alt_dir, align_stage=align_stage)
    assert rw == (q + 7) // 8 and 8 * fw >= q + c
    assert np.array_equal(lens, m_lens), [(int(i), int(lens[i]), int(m_lens[i])) for i in np.nonzero(lens != m_lens)[0][:5]]
    assert np.array_equal(blk_rows, m_rows), (blk_rows, m_rows)
    bad = np.argwhere(words != m_words)
    assert bad.size == 0, "first differences (block, word, slot, have, want, read, loc, sv): %s" % [
        (int(b), int(w), int(s), hex(int(words[b, w, s])), hex(int(m_words[b, w, s])),
         int(pair_read[b * 64 + s]) if b * 64 + s < n_pairs else None, int(pair_loc[b * 64 + s]) if b * 64 + s < n_pairs else None,
         int(pair_sv[b * 64 + s]) if b * 64 + s < n_pairs else None) for b, w, s in bad[:5]]
    return pair_read, pair_loc, pair_sv, m_words, rw


@pytest.mark.parametrize("q,c", SHAPES)
@pytest.mark.parametrize("align_stage", [False, True], ids=["score", "align"])
def test_every_read_on_both_strands(q, c, align_stage):
    """130 pairs: two full blocks and two pairs of a third; every read of _rows on both strands, every location of _locations"""
    n_reads = len(_rows(q))
    assert 2 * n_reads <= 130
    pair_read, pair_loc, pair_sv, m_words, rw = _check(q, c, 130, 0, align_stage)
    # the set is what it claims to be: every read forward and reverse, every location, and windows that fail to decode (all N)
    assert {(int(r), int(s) & 1) for r, s in zip(pair_read, pair_sv)} >= {(r, s) for r in range(n_reads) for s in (0, 1)}
    assert set(int(x) for x in pair_loc) == set(_locations(_world()[2], c))
    all_n = HM.pack8(np.full(8, 5))
    assert np.any(np.all(m_words[:, rw:, :] == all_n, axis=1))


@pytest.mark.parametrize("n_pairs", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("alt_dir", [0, 1, 2])
def test_pair_counts_and_table_bit(n_pairs, alt_dir):
    q, c = 102, 20
    pair_read, pair_loc, pair_sv, m_words, rw = _check(q, c, n_pairs, alt_dir, n_pairs % 2 == 0)
    if alt_dir and n_pairs >= 63:   # the bit is there, and not everywhere; with alt_dir 2 it depends on the read index
        bit = (m_words[:, 0, :].reshape(-1)[:n_pairs] >> 3) & 1
        assert 0 < int(bit.sum()) < n_pairs
        rev, odd = pair_sv & 1, pair_read & 1
        assert np.array_equal(bit, rev if alt_dir == 1 else rev ^ odd)


def test_hook_refuses_bad_arguments():
    from nextgenmap_amd.pipeline import NgmHipError
    q, c = 32, 8
    rows = _rows(q)
    mp = _mapper(q, c)
    one = np.zeros(1, np.uint32)
    with pytest.raises(NgmHipError):
        mp.debug_gather_pairs(rows, np.array([len(rows)], np.uint32), one, one)   # a pair of a read that is not there
    with pytest.raises(NgmHipError):
        mp.debug_gather_pairs(rows, one, one, one, alt_dir=3)
