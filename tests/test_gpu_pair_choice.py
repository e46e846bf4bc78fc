"""-m gpu: pair_simple_kernel (csrc/gather_device.h) and the three instances of pair_choice_kernel (csrc/pair_device.h) against plain
models of ScoreBuffer::top1PE + CheckPairs (src/ScoreBuffer.cpp:368-502), through ngm_debug_pair_select -- the launch sequence map_impl
itself runs.

tests/pair_choice_model.py holds the reference's loop restated literally, the order-free contract the kernels are written to, and the
constructed pairs (each named after the edge it reaches: the list split at 64 candidates, the caps of 2 048 and 8 192 candidates above the
cut-off, 64 listed combinations, 8 listed best ones, strict window bounds, the `int` insert size, negative best scores, persistent
workgroups that take one pair after another); tests/test_pair_choice_model.py checks the contract against the loop and the generator's
coverage without a GPU.  Here every field the mapper downloads is compared: nothing depends on tied_ix values or on the order inside the
lists of best combinations, which come from atomics."""
import ctypes as C

import numpy as np
import pytest

import pair_choice_model as M

pytestmark = pytest.mark.gpu

FOUND, TIED, DUP, HOST = 1, 2, 4, 8
MAPQ_KEPT, NBEST_KEPT = -7, -9   # what the caller puts into mapq / n_best: a pair the kernels do not take leaves them alone


class Run:
    def __init__(self, lib, bt):
        n = bt.n_pairs
        self.bt = bt
        self.cons = [M.contract(bt, p) for p in range(n)]
        self.info = np.zeros(n, np.int32)
        self.mapq = np.full(2 * n, MAPQ_KEPT, np.int32)
        self.n_best = np.full(2 * n, NBEST_KEPT, np.int32)
        self.counts = np.zeros(4, np.uint32)
        self.entries = np.zeros((2 * n + 2, 8), np.int32)   # PairOut: flags, wa, wb, dist, dmin, dmax, tied_ix, pair
        self.tops = np.zeros((n + 1, 3, 8), np.int32)       # PairTop: d[8], a[8], b[8]
        rc = lib.ngm_debug_pair_select(0, n, bt.base.ctypes.data, bt.count.ctypes.data, bt.n_cand, bt.scores.ctypes.data, bt.loc.ctypes.data, bt.read_len.ctypes.data,
                                       bt.min_d, bt.max_insert, bt.cutoff, self.info.ctypes.data, self.mapq.ctypes.data, self.n_best.ctypes.data, self.counts.ctypes.data,
                                       self.entries.ctypes.data, self.tops.ctypes.data)
        assert rc == 0, lib.ngm_pipeline_last_error()

    def entry_row(self, p):
        """the pair's entry, resolved as map_impl resolves it"""
        info = int(self.info[p])
        assert info <= -2
        e = -2 - info
        return self.bt.n_pairs + (e - (1 << 30)) if e >= (1 << 30) else e

    def where(self, p):
        return (self.bt.name, p, self.bt.tags[p])


@pytest.fixture(scope="module")
def runs():
    from nextgenmap_amd.pipeline import _lib
    lib = _lib()
    lib.ngm_debug_pair_select.restype = C.c_int
    lib.ngm_debug_pair_select.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float] + [C.c_void_p] * 6
    return [Run(lib, bt) for bt in M.make_batches()]


def test_one_candidate_pairs_are_settled_as_the_loop_settles_them(runs):
    checked = left = 0
    for r in runs:
        for p, c in enumerate(r.cons):
            if c.cls != "simple":
                continue
            found, wa, wb, equal, dist, mq_a, mq_b = M.literal(r.bt, p)
            assert (found, equal, mq_a, mq_b) == (int(c.found), 0, 60, 60)
            info = int(r.info[p])
            kept = (MAPQ_KEPT, MAPQ_KEPT, NBEST_KEPT, NBEST_KEPT)
            got = (int(r.mapq[2 * p]), int(r.mapq[2 * p + 1]), int(r.n_best[2 * p]), int(r.n_best[2 * p + 1]))
            if info == -1:   # only an insert size that does not fit `info` may be left to the host
                assert found and dist >= 2 ** 30, r.where(p)
                assert got == kept, r.where(p)
                left += 1
                continue
            assert info >= 0 and (info & 1, info >> 1) == (found, dist), r.where(p) + (info, found, dist)
            assert got == ((60, 60, 0, 0) if found else kept), r.where(p)
            checked += 1
    assert checked > 2000 and left <= 8


def test_a_mate_without_candidates_leaves_the_pair_to_the_host(runs):
    seen = set()
    for r in runs:
        for p, c in enumerate(r.cons):
            if c.cls == "empty":
                assert r.info[p] == -1, r.where(p)
                assert (r.mapq[2 * p], r.mapq[2 * p + 1], r.n_best[2 * p], r.n_best[2 * p + 1]) == (MAPQ_KEPT, MAPQ_KEPT, NBEST_KEPT, NBEST_KEPT)
                seen.add((r.bt.mate(p, 0)[1], r.bt.mate(p, 1)[1]))
    assert {(0, 0), (0, 1), (1, 0), (0, 70), (70, 0)} <= seen


def test_lists_counts_and_entries(runs):
    for r in runs:
        n = r.bt.n_pairs
        small = {p for p, c in enumerate(r.cons) if c.cls == "small"}
        large = {p for p, c in enumerate(r.cons) if c.cls == "large"}
        huge = {p for p, c in enumerate(r.cons) if c.huge}
        tied_n, n_small, n_large, n_huge = (int(x) for x in r.counts)
        assert (n_small, n_large, n_huge) == (len(small), len(large), len(huge)), r.bt.name
        # the entries of each list: a permutation of the expected pairs; nothing written beyond them
        assert sorted(r.entries[:n_small, 7].tolist()) == sorted(small)
        assert sorted(r.entries[n:n + n_large, 7].tolist()) == sorted(large)
        assert np.all(r.entries[n_small:n, 7] == -1) and np.all(r.entries[n + n_large:, 7] == -1)
        # info names the pair's own entry: no pair in two lists, none missing
        rows = set()
        for p in small | large:
            row = r.entry_row(p)
            assert (row < n) == (p in small) and r.entries[row, 7] == p, r.where(p)
            rows.add(row)
        assert len(rows) == len(small) + len(large)
        # tied pairs: counted once each, their rows in the list of best combinations distinct
        tied_rows = [row for row in rows if r.entries[row, 0] & TIED]
        assert tied_n == len(tied_rows)
        ix = r.entries[tied_rows, 6]
        assert len(set(ix.tolist())) == len(tied_rows) and (len(ix) == 0 or (ix.min() >= 0 and ix.max() < tied_n))
        assert np.all(r.entries[[row for row in rows if not r.entries[row, 0] & TIED], 6] == -1)
    assert int(runs[0].counts[1]) > 8192 and int(runs[0].counts[2]) > 1024 and int(runs[0].counts[3]) > 256   # each launch's workgroups take several pairs


def test_host_entries_are_exactly_the_models(runs):
    n_host = n_huge_live = 0
    for r in runs:
        for p, c in enumerate(r.cons):
            if c.cls in ("small", "large"):
                flags = int(r.entries[r.entry_row(p), 0])
                assert bool(flags & HOST) == c.host, r.where(p) + (hex(flags), c.n_above)
                if c.host:
                    assert flags & (FOUND | TIED | DUP) == 0
                n_host += c.host
                n_huge_live += c.huge and not c.host   # the third launch's entry has replaced the second launch's placeholder
    assert n_host > 100 and n_huge_live > 150


def test_choice_pairs_match_the_contract_and_the_loop(runs):
    n_settled = n_listed = n_beyond = n_skipped = n_choice = 0
    for r in runs:
        bt = r.bt
        for p, c in enumerate(r.cons):
            if c.cls not in ("small", "large") or c.host:
                continue
            n_choice += 1
            flags, wa, wb, dist, dmin, dmax, tied_ix, pair = (int(x) for x in r.entries[r.entry_row(p)])
            got = (bool(flags & FOUND), bool(flags & TIED), bool(flags & DUP), bool(flags & HOST), (flags >> 8) & 255, (flags >> 16) & 255, (flags >> 24) & 255)
            n_top_field = 0 if c.n_combo > M.COMBOS else min(c.n_top, 15)
            assert got == (c.found, c.tied, c.dup, False, c.mq_a, c.mq_b, n_top_field), r.where(p) + (got, c.n_combo, c.n_top)
            assert pair == p
            if not c.tied:
                assert c.n_combo <= M.LITERAL_LIMIT
                lit = M.literal(bt, p)
                assert (int(c.found), wa, wb, dist) == (lit[0], lit[1], lit[2], lit[4]), r.where(p) + (wa, wb, dist, lit)
                assert lit[3] == 0 and (lit[5], lit[6]) == (c.mq_a, c.mq_b)
                n_settled += 1
            elif c.n_combo > M.COMBOS:
                assert (dmin, dmax) == (bt.min_d, bt.max_d), r.where(p)
                n_beyond += 1
                n_skipped += c.n_combo > M.LITERAL_LIMIT
            elif c.found:
                assert (dmin, dmax) == (c.dmin, c.dmax), r.where(p)
                k = min(c.n_top, 8)
                listed = {(int(r.tops[tied_ix, 0, x]), int(r.tops[tied_ix, 1, x]), int(r.tops[tied_ix, 2, x])) for x in range(k)}
                assert len(listed) == k and listed <= c.tops, r.where(p) + (listed, c.tops)
                if c.n_top <= 8:
                    assert listed == c.tops
                n_listed += 1
    assert n_settled > 3000 and n_listed > 1000 and n_beyond > 1000
    assert n_skipped < 0.05 * n_choice   # the pairs the literal loop is too slow for: tied beyond listing, covered by the contract alone
