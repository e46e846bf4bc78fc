"""-m gpu: `--markdup` -- pipeline.BamSorter(markdup=True) over ngm_bam_sort_set_markdup (csrc/bam_sort.cpp, csrc/markdup_device.h) and
`ngm-hip --bam --sort --markdup` against the plain-Python rules of tests/markdup_model.py.  The check is always the same and leaves no
record out: the inflated members are bam_index_model.sort_records(model(records)), the BAI file is the canonical one of those records,
and markdup_stats() holds the model's six counts."""
import functools
import gzip
import os
import random
import re
import struct
import subprocess

import numpy as np
import pytest

import bam_fixtures as BF
import bam_index_model as M
import markdup_model as MD
import simulate as S
from test_markdup_host import rec

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "nextgenmap_amd", "ngm-hip")
REFS = [(b"chrA", 100000), (b"chrEmpty", 5000), (b"chrB", 40000), (b"chrC", 1000000)]
FIRST = len(BF.bgzf(BF.bam_bytes([], REFS, b"@HD\tVN:1.0\tSO:coordinate\n"), eof=False))
Mop, Iop, Dop, Sop, Hop = 0, 1, 2, 4, 5


def _err():
    from nextgenmap_amd import NgmHipError
    return NgmHipError


def sort_with(runs, order=None, markdup=True, setter=True, n_ref=len(REFS)):
    from nextgenmap_amd import pipeline as P
    s = P.BamSorter(device=0, markdup=markdup) if setter else P.BamSorter(device=0)
    try:
        for seq in (order if order is not None else range(len(runs))):
            s.add(seq, runs[seq])
        s.finish(n_ref)
        members = b"".join(s.members())
        return members, s.index(FIRST), (s.markdup_stats() if markdup else None)
    finally:
        s.close()


def cut(records, n_runs, rnd):
    at = sorted(rnd.randrange(len(records) + 1) for _ in range(n_runs - 1)) if records else []
    return [b"".join(records[a:b]) for a, b in zip([0] + at, at + [len(records)])]


def check(records, runs=None, order=None, n_ref=len(REFS)):
    marked, counts = MD.mark(records)
    want = M.sort_records(marked)
    members, bai, st = sort_with([b"".join(records)] if runs is None else runs, order, n_ref=n_ref)
    got = gzip.decompress(members) if members else b""
    if got != b"".join(want):                              # name the first record that differs before the streams are compared
        recs = [got[o:o + n] for o, n in M.walk(got)]
        for i, (a, b) in enumerate(zip(recs, want)):
            assert a == b, "sorted record %d (%r): flag 0x%x, the model says 0x%x" % (i, MD.parse(b)[3], MD.parse(a)[2], MD.parse(b)[2])
    assert got == b"".join(want)
    sizes, _ = M.member_sizes(members)
    assert bai == M.canonical_bai(want, n_ref, sizes, FIRST)
    assert {k: st[k] for k in MD.COUNT_NAMES} == counts
    assert st["mark_ms"] >= 0 and st["sort_ms"] >= 0
    return marked, counts


def flags(records):
    return [MD.parse(r)[2] & 0x400 for r in records]


Q = lambda v, n=20: bytes([v]) * n


def frag(name, pos, flag=0, cigar=((Mop, 20),), qual=Q(30), ref=0):
    return rec(name, ref, pos, flag, list(cigar), qual)


def pair(name, a, b, qa=Q(30), qb=Q(30)):
    """a, b: (ref, pos, reverse) of the first and the second mate, 20M each"""
    return [rec(name, a[0], a[1], 0x41 | (16 if a[2] else 0) | (0x20 if b[2] else 0), [(Mop, 20)], qa),
            rec(name, b[0], b[1], 0x81 | (16 if b[2] else 0) | (0x20 if a[2] else 0), [(Mop, 20)], qb)]


# ---- the smallest shapes --------------------------------------------------------------------------------------------------------------
def test_empty():
    members, bai, st = sort_with([])
    assert members == b"" and {k: st[k] for k in MD.COUNT_NAMES} == dict.fromkeys(MD.COUNT_NAMES, 0)
    check([], runs=[])


def test_one_record():
    marked, counts = check([frag(b"a", 10)])
    assert flags(marked) == [0] and counts["fragments"] == 1


def test_two_identical_fragments():
    marked, _ = check([frag(b"a", 10), frag(b"b", 10)])
    assert flags(marked) == [0, 0x400]


def test_equal_u5_through_soft_clips():
    marked, _ = check([frag(b"a", 100, cigar=[(Mop, 20)]), frag(b"b", 103, cigar=[(Sop, 3), (Mop, 17)]), frag(b"c", 103, cigar=[(Mop, 17)])])
    assert flags(marked) == [0, 0x400, 0]


def test_forward_and_reverse_at_one_pos_are_no_duplicates():
    marked, _ = check([frag(b"a", 100), frag(b"b", 100, flag=16), frag(b"c", 119, flag=0)])   # (c starts where b's 5' end lies: another strand)
    assert flags(marked) == [0, 0, 0]


def test_reverse_fragments_that_differ_in_trailing_clips():
    recs = [frag(b"a", 100, 16, [(Mop, 20)]), frag(b"b", 100, 16, [(Mop, 17), (Sop, 3)]), frag(b"c", 100, 16, [(Mop, 14), (Sop, 3), (Hop, 3)]), frag(b"d", 100, 16, [(Mop, 17)]),
            frag(b"e", 90, 16, [(Sop, 5), (Mop, 30)])]
    marked, _ = check(recs)
    assert [MD.u5(r) for r in recs] == [119, 119, 119, 116, 119]
    assert flags(marked) == [0, 0x400, 0x400, 0, 0x400]


# ---- group sizes ------------------------------------------------------------------------------------------------------------------------
SIZES = [1, 2, 63, 64, 65, 300]


@pytest.mark.parametrize("scores", ["equal", "best-last"])
def test_group_sizes(scores):
    """in key order the groups lie at places 0, 1, 3, 66, 130 and 195: the group of 300 straddles the boundary of the first block of 256
    threads, and the groups of 64 and 65 the waves at 128 and 192.  In run order the groups are interleaved."""
    rnd = random.Random(11)
    recs, places, at = [], [], 0
    for k, size in enumerate(SIZES):
        places.append(at)
        at += size
        for i in range(size):
            q = Q(30) if scores == "equal" or i < size - 1 else Q(31)
            recs.append((rnd.random() if i < size - 1 else 2.0 + k, k, frag(b"g%d_%d" % (k, i), 1000 * (k + 1), qual=q)))
    assert places[5] < 256 < places[5] + 300
    recs.sort(key=lambda x: x[0])                          # interleaved; with best-last every group's best record comes behind all the others
    records = [r for _, _, r in recs]
    marked, counts = check(records, runs=cut(records, 3, rnd))
    assert counts["duplicate_fragments"] == sum(SIZES) - len(SIZES)
    for k in range(len(SIZES)):
        mine = [f for (_, kk, _), f in zip(recs, flags(marked)) if kk == k]
        assert mine == ([0] + [0x400] * (SIZES[k] - 1) if scores == "equal" else [0x400] * (SIZES[k] - 1) + [0])


def test_pair_group_sizes():
    """the same for pairs: groups of 1, 2, 63, 64, 65 and 300 pairs, the best pair last, an equal-score group among them; every other pair
    has its second mate in front"""
    rnd = random.Random(12)
    items = []
    for k, size in enumerate(SIZES):
        for i in range(size):
            best = i == size - 1 and k != 3                # the group of 64: all scores equal, the first pair survives
            items.append((rnd.random() if i < size - 1 else 2.0 + k, k, pair(b"p%d_%d" % (k, i), (0, 1000 * (k + 1), 0), (0, 1000 * (k + 1) + 200, 1), qb=Q(31 if best else 30))[::1 - 2 * (i % 2)]))
    items.sort(key=lambda x: x[0])
    records = [r for _, _, p in items for r in p]
    marked, counts = check(records, runs=cut(records, 4, rnd))
    assert counts["pairs"] == sum(SIZES) and counts["duplicate_pairs"] == sum(SIZES) - len(SIZES) and counts["fragments"] == 0
    f = flags(marked)
    for k in range(len(SIZES)):
        mine = [f[2 * j] for j, (_, kk, _) in enumerate(items) if kk == k]
        assert mine == ([0] + [0x400] * (SIZES[k] - 1) if k == 3 else [0x400] * (SIZES[k] - 1) + [0])
    assert all(f[2 * j] == f[2 * j + 1] for j in range(len(items)))


# ---- pairs --------------------------------------------------------------------------------------------------------------------------------
def test_fr_pairs_with_swapped_roles_are_duplicates_ff_pairs_are_not():
    fr = pair(b"a", (0, 100, 0), (0, 300, 1)) + pair(b"b", (0, 300, 1), (0, 100, 0), qa=Q(29))
    ff = pair(b"c", (0, 5000, 0), (0, 5300, 0)) + pair(b"d", (0, 5300, 0), (0, 5000, 0))
    ff_dup = pair(b"e", (0, 5000, 0), (0, 5300, 0), qa=Q(40))
    marked, counts = check(fr + ff + ff_dup)
    assert flags(marked) == [0, 0, 0x400, 0x400] + [0x400, 0x400, 0, 0] + [0, 0]
    assert counts["duplicate_pairs"] == 2


def test_pair_on_two_references():
    recs = pair(b"a", (0, 100, 0), (2, 300, 1)) + pair(b"b", (0, 100, 0), (3, 300, 1)) + pair(b"c", (2, 300, 1), (0, 100, 0), qa=Q(35)) + pair(b"d", (0, 100, 0), (0, 300, 1))
    marked, _ = check(recs)
    assert flags(marked) == [0x400, 0x400, 0, 0, 0, 0, 0, 0]


def test_pair_split_across_two_runs():
    recs = pair(b"a", (0, 100, 0), (0, 300, 1)) + pair(b"b", (0, 100, 0), (0, 300, 1), qa=Q(40)) + [frag(b"f", 7000)]
    runs = [b"".join(recs[:1]), b"".join(recs[1:3]), b"".join(recs[3:])]      # both pairs cut between their mates
    marked, counts = check(recs, runs=runs, order=[2, 0, 1])
    assert flags(marked) == [0x400, 0x400, 0, 0, 0] and counts["pairs"] == 2


def test_what_is_no_pair():
    a = lambda name, flag, pos=100, ref=0: rec(name, ref, pos, flag, [(Mop, 20)], Q(30))
    recs = [a(b"x", 0x41), a(b"x", 0x41, 300),                  # 0x40 followed by 0x40
            a(b"y", 0x41), a(b"z", 0x91, 281),                  # equal flags to a pair's, other names
            a(b"m", 0x49), a(b"m", 0x85, 100),                  # the mate is unmapped: the mapped one is a fragment
            a(b"w", 0x91, 881), a(b"w", 0x61, 700),             # a pair with its second mate in front
            a(b"ok", 0x61), a(b"ok", 0x91, 281),                # and one with its first mate in front
            a(b"f", 0, 700)]
    marked, counts = check(recs)
    assert counts["pairs"] == 2 and counts["fragments"] == 6 and counts["examined"] == 10
    # the fragments at pos 100 forward lie on the first end of pair ok, z on its second (reverse, u5 300) and f on the first end of pair w:
    # all marked.  The forward fragment at pos 300 is on no pair end
    assert flags(marked) == [0x400, 0, 0x400, 0x400, 0x400, 0, 0, 0, 0, 0, 0x400]


def test_second_mate_in_front():
    """the order ngm-hip writes.  Both orders give one pair key; three records of one name in a row: the pair with the first mate in front"""
    a, b = pair(b"a", (0, 100, 0), (0, 300, 1)), pair(b"b", (0, 100, 0), (0, 300, 1), qa=Q(40))
    marked, counts = check(a[::-1] + b + pair(b"c", (0, 100, 0), (0, 300, 1))[::-1])
    assert flags(marked) == [0x400, 0x400, 0, 0, 0x400, 0x400] and counts["pairs"] == 3
    x = lambda flag, pos: rec(b"x", 0, pos, flag, [(Mop, 20)], Q(30))
    chain = [x(0x91, 5281), x(0x61, 5100), x(0x91, 5281), x(0x61, 5100)]      # 0x80 0x40 0x80 0x40: the middle two are the pair
    marked, counts = check(chain + pair(b"y", (0, 5100, 0), (0, 5281, 1), qa=Q(20)))
    assert counts["pairs"] == 2 and counts["fragments"] == 2 and flags(marked) == [0x400, 0, 0, 0x400, 0x400, 0x400]


def test_fragments_on_pair_ends():
    recs = pair(b"a", (0, 100, 0), (0, 300, 1), qa=Q(40)) + pair(b"b", (0, 100, 0), (0, 300, 1)) + pair(b"c", (0, 100, 0), (0, 400, 1))
    # a survives, b is its duplicate, c is a pair of its own; the second mates' 5' ends are at 319 (a, b) and 419 (c)
    recs += [frag(b"on-first-end", 100, qual=Q(90)), frag(b"on-reverse-end", 300, 16, qual=Q(90)), frag(b"on-c-end", 403, 16, [(Mop, 17)]), frag(b"near", 101), frag(b"near-r", 299, 16)]
    assert [MD.u5(r) for r in recs[6:]] == [100, 319, 419, 101, 318]
    marked, counts = check(recs)
    assert flags(marked) == [0, 0, 0x400, 0x400, 0, 0] + [0x400, 0x400, 0x400, 0, 0]
    assert counts["duplicate_fragments"] == 3 and counts["duplicate_pairs"] == 1


def test_fragment_on_the_end_of_a_duplicate_pair():
    recs = pair(b"a", (0, 100, 0), (0, 300, 1), qa=Q(40)) + pair(b"b", (0, 100, 0), (0, 300, 1))
    recs += [frag(b"on-both-pairs-end", 300, 16, qual=Q(90)), frag(b"one-base-away", 301, 16, qual=Q(1)), frag(b"other-strand", 319, 0)]
    marked, counts = check(recs)
    assert flags(marked) == [0, 0, 0x400, 0x400, 0x400, 0, 0]
    assert counts["duplicate_fragments"] == 1 and counts["duplicate_pairs"] == 1


# ---- ignored records, flags already set, qualities ----------------------------------------------------------------------------------------
def test_ignored_records_inside_groups():
    recs = [frag(b"a", 100), frag(b"sec", 100, flag=0x100, qual=Q(90)), frag(b"sup", 100, flag=0x800, qual=Q(90)), frag(b"unm", 100, flag=0x4, qual=Q(90)),
            rec(b"noref", -1, 100, 0, [(Mop, 20)], Q(90)), frag(b"b", 100), rec(b"none", -1, -1, 4, [], Q(90))]
    recs += pair(b"p", (0, 100, 0), (0, 300, 1))[:1] + [frag(b"between", 5000, flag=0x100)] + pair(b"p", (0, 100, 0), (0, 300, 1))[1:]   # a record between the mates: no pair
    marked, counts = check(recs)
    assert counts["examined"] == 4 and counts["pairs"] == 0
    assert flags(marked) == [0, 0, 0, 0, 0, 0x400, 0, 0x400, 0, 0]


def test_flag_0x400_on_input():
    recs = [frag(b"a", 100, flag=0x400), frag(b"b", 100), frag(b"c", 100, flag=0x400), frag(b"alone", 900, flag=0x400), frag(b"ign", 100, flag=0x500)]
    marked, counts = check(recs)
    assert flags(marked) == [0x400] * 5                   # a survives and keeps what it came with
    assert counts["duplicate_fragments"] == 2 and counts["newly_marked"] == 1


def test_absent_qualities_and_no_bases_inside_groups():
    recs = [rec(b"absent", 0, 100, 0, [(Mop, 20)], None, l_seq=20), rec(b"empty", 0, 100, 0, [(Mop, 20)], b""), frag(b"low", 100, qual=Q(14)),
            frag(b"one", 100, qual=Q(14, 19) + Q(15, 1)), rec(b"absent2", 0, 100, 0, [(Mop, 20)], None, l_seq=20)]
    marked, _ = check(recs)
    assert flags(marked) == [0x400, 0x400, 0x400, 0, 0x400]
    marked, _ = check(recs[:3] + recs[4:])                 # all scores 0: the first survives
    assert flags(marked) == [0, 0x400, 0x400, 0x400]


def test_odd_lengths_and_alignments_of_the_qualities():
    """names of 1 to 9 bytes and 0 to 3 CIGAR operations move the qualities over every alignment; lengths around the dwords of a wave's round"""
    rnd = random.Random(13)
    recs = []
    for l_seq in (1, 2, 3, 4, 5, 7, 63, 64, 65, 255, 256, 257, 259, 1000):
        for l_name in range(1, 10):
            q = bytes(rnd.choice([14, 15, 40, 93, 0, 255]) for _ in range(l_seq))
            q = bytes([40]) + q[1:]
            recs.append(rec(b"n" * l_name, 0, 100, 0, [(Sop, 1)] * (l_name % 4) + [(Mop, max(l_seq - l_name % 4, 1))], q, tags=b"\xff" * (l_name % 3)))
    rnd.shuffle(recs)
    marked, counts = check(recs)
    assert counts["duplicate_fragments"] + len({MD.end_key(r) for r in recs}) == len(recs)


# ---- the mixed case, its cuts, and marking switched off -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mixed():
    """about 2 500 records: fragments and pairs in duplicate groups, on both strands, with clips, plus records the marker ignores"""
    rnd = random.Random(21)
    recs = []
    sites = [(rnd.choice([0, 2, 3]), rnd.randrange(100, 30000)) for _ in range(150)]
    while len(recs) < 2500:
        x = rnd.random()
        ref, pos = rnd.choice(sites) if x < 0.6 else (rnd.choice([0, 2, 3]), rnd.randrange(100, 30000))
        y = rnd.random()
        l_seq = 40 if y < 0.35 else rnd.randrange(20, 80)  # (mates of one length: pairs on a site share both ends often enough)
        q = rnd.randbytes(l_seq)
        name = b"m%d" % len(recs)
        clip = rnd.choice([0, 0, 3])
        cigar = ([(Sop, clip)] if clip else []) + [(Mop, l_seq - clip)]
        if y < 0.35:
            far = rnd.choice([200, 200, 250])
            s1 = rnd.random() < 0.5
            recs += [rec(name, ref, pos + clip, 0x41 | (16 if s1 else 0), cigar, q), rec(name, ref, pos + far, 0x81 | (0 if s1 and rnd.random() < 0.9 else 16), [(Mop, l_seq)], rnd.randbytes(l_seq))]
        elif y < 0.9:
            recs.append(rec(name, ref, pos + clip, rnd.choice([0, 0, 16, 0x400, 0x49]), cigar, q))
        elif y < 0.95:
            recs.append(rec(name, ref, pos, rnd.choice([0x100, 0x800, 0x4, 0x904]), cigar, q))
        else:
            recs.append(rec(name, -1, -1, rnd.choice([4, 77, 141]), [], q))
    return tuple(recs)


@pytest.mark.parametrize("n_runs", [1, 7, 50])
def test_mixed_does_not_depend_on_the_runs(n_runs):
    recs = list(mixed())
    rnd = random.Random(22 + n_runs)
    order = list(range(n_runs))
    rnd.shuffle(order)
    _, counts = check(recs, runs=cut(recs, n_runs, rnd), order=order)
    assert counts["duplicate_pairs"] > 50 and counts["duplicate_fragments"] > 300 and counts["newly_marked"] < counts["duplicate_fragments"] + 2 * counts["duplicate_pairs"]


def test_off_means_off():
    recs = list(mixed())
    runs = cut(recs, 5, random.Random(23))
    never, bai_never, _ = sort_with(runs, markdup=False, setter=False)
    off, bai_off, _ = sort_with(runs, markdup=False)
    assert off == never and bai_off == bai_never
    assert gzip.decompress(off) == b"".join(M.sort_records(recs))
    on, _, _ = sort_with(runs)
    stream = gzip.decompress(on)
    marked = [stream[o:o + n] for o, n in M.walk(stream)]
    want = M.sort_records(recs)
    came_with = [MD.parse(r)[2] & 0x400 for r in want]
    cleared = [r if c else r[:18] + struct.pack("<H", struct.unpack_from("<H", r, 18)[0] & ~0x400) + r[20:] for r, c in zip(marked, came_with)]
    assert cleared == want and marked != want


def _fast(rnd, name, ref_id, pos, flag, l_seq):
    return rec(name, ref_id, pos, flag, [(Mop, l_seq)], rnd.randbytes(l_seq))


def test_medium():
    """about 50 000 records in 5 runs, a third of them in duplicate groups of fragments and of pairs"""
    rnd = random.Random(31)
    recs = []
    while len(recs) < 50000:
        ref, pos, l_seq = rnd.choice([0, 2, 3]), rnd.randrange(0, 38000), rnd.randrange(100, 151)
        x = rnd.random()
        copies = rnd.randrange(2, 6) if x < 0.1 else 1
        if rnd.random() < 0.4:
            for c in range(copies):
                recs += [_fast(rnd, b"p%d_%d" % (len(recs), c), ref, pos, 0x61, l_seq), _fast(rnd, b"p%d_%d" % (len(recs), c), ref, pos + 300, 0x91, l_seq)]
        else:
            for c in range(copies):
                recs.append(_fast(rnd, b"f%d_%d" % (len(recs), c), ref, pos, rnd.choice([0, 16]), l_seq))
    blocks, at = [], 0                                     # keep mates together, shuffle the rest
    while at < len(recs):
        n = 2 if MD.parse(recs[at])[2] & 0x40 else 1
        blocks.append(recs[at:at + n][::rnd.choice([1, -1])])      # (half of the pairs with the second mate in front)
        at += n
    rnd.shuffle(blocks)
    recs = [r for b in blocks for r in b]
    _, counts = check(recs, runs=cut(recs, 5, rnd))
    in_groups = 2 * counts["duplicate_pairs"] + counts["duplicate_fragments"]
    assert len(recs) // 6 < in_groups < len(recs) // 2 and counts["duplicate_pairs"] > 1000


# ---- errors: each raises with its message, the sorter destroys cleanly, and a new sorter then sorts one record ---------------------------
def _then_single():
    r = frag(b"single", 10)
    members, _, st = sort_with([r])
    assert gzip.decompress(members) == r and st["examined"] == 1


def test_setter_after_an_add():
    from nextgenmap_amd import pipeline as P
    s = P.BamSorter(device=0)
    s.add(0, frag(b"a", 10))
    with pytest.raises(_err(), match=r"ngm_bam_sort_set_markdup: .*before the first ngm_bam_sort_add"):
        s.set_markdup(True)
    s.finish(len(REFS))
    with pytest.raises(_err(), match=r"ngm_bam_sort_set_markdup"):
        s.set_markdup(True)
    assert gzip.decompress(b"".join(s.members())) == frag(b"a", 10)
    s.close()
    _then_single()


def test_stats_with_marking_off_or_before_finish():
    from nextgenmap_amd import pipeline as P
    s = P.BamSorter(device=0)
    s.add(0, frag(b"a", 10))
    s.finish(len(REFS))
    with pytest.raises(_err(), match=r"ngm_bam_sort_markdup_stats: duplicate marking is off"):
        s.markdup_stats()
    s.close()
    s = P.BamSorter(device=0, markdup=True)
    s.add(0, frag(b"a", 10))
    with pytest.raises(_err(), match=r"ngm_bam_sort_markdup_stats: ngm_bam_sort_finish has not succeeded"):
        s.markdup_stats()
    s.close()
    s = P.BamSorter(device=0, markdup=True)
    s.add(3, rec(b"bad", len(REFS), 10, 0, [(Mop, 5)], Q(30, 5)))        # finish refuses it: no statistics of a failed finish
    with pytest.raises(_err(), match=r"ngm_bam_sort_finish: seq 3, record 0"):
        s.finish(len(REFS))
    with pytest.raises(_err(), match=r"ngm_bam_sort_markdup_stats"):
        s.markdup_stats()
    s.close()
    _then_single()


# ---- ngm-hip --bam --sort --markdup -------------------------------------------------------------------------------------------------------
def _cli_case(tmp_path, paired):
    """a small reference; every fifth read (or pair) comes a second and a third time under a new name with other qualities"""
    contigs = S.make_genome([60000, 40001], seed=901, repeat_families=4, repeat_len=300, copies=3)
    fa = str(tmp_path / "ref.fa")
    S.write_fasta(fa, contigs)
    fq = str(tmp_path / "reads.fq")
    rng = np.random.default_rng(9)
    qual = lambda n: bytes(rng.integers(35, 74, n).astype(np.uint8))
    out = []
    if paired:
        r1, r2 = S.make_reads(contigs, 500, 100, seed=902, sub_rate=0.01, indel_rate=0.002, paired=True)
        for k in range(0, 150, 3):                         # mates that do not map: the other mate is a fragment
            r2[k] = (r2[k][0], S.ACGT[rng.integers(0, 4, 100)], r2[k][2])
        units = [[a, b] for a, b in zip(r1, r2)]
    else:
        units = [[r] for r in S.make_reads(contigs, 800, 100, seed=903, sub_rate=0.01, indel_rate=0.002)]
    for k, u in enumerate(units):
        out.append([(n, s, qual(len(s))) for n, s, _ in u])
        if k % 5 == 0:
            for c in range(2):
                out.append([("copy%d_%s" % (c, n), s, qual(len(s))) for n, s, _ in u])
    order = rng.permutation(len(out))
    S.write_fastq(fq, [x for i in order for x in out[i]])
    return fa, (["-p", "-q", fq] if paired else ["-q", fq])


def _run(tmp_path, tag, fa, args, code=0):
    d = tmp_path / tag
    d.mkdir()
    c = subprocess.run([CLI, "-r", fa, "-o", "out.bam", "--affine"] + args, capture_output=True, text=True, cwd=str(d))
    assert c.returncode == code, c.stderr[-2000:]
    return str(d / "out.bam"), c.stderr


@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_cli(tmp_path, paired):
    from test_gpu_bam_sort import split_bam
    fa, inp = _cli_case(tmp_path, paired)
    plain, _ = _run(tmp_path, "plain", fa, inp + ["--bam"])
    unsorted = split_bam(plain)[3]                         # the records in run order
    if paired:                                             # what the pairing rule rests on: the mates next to each other (mate 2 in front), equal names
        assert len(unsorted) % 2 == 0 and all(MD.parse(a)[3] == MD.parse(b)[3] and MD.parse(a)[2] & 0xC1 == 0x81 and MD.parse(b)[2] & 0xC1 == 0x41
                                              for a, b in zip(unsorted[::2], unsorted[1::2]))
    marked, counts = MD.mark(unsorted)
    # (paired: fragments are the mates of the 50 reads that do not map, 10 of them come three times)
    assert (counts["duplicate_fragments"] > 10 and counts["duplicate_pairs"] > 50) if paired else (counts["duplicate_fragments"] > 50 and counts["pairs"] == 0)
    srt, err = _run(tmp_path, "marked", fa, inp + ["--bam", "--sort", "--markdup"])
    first, _, n_ref, recs, members = split_bam(srt)
    assert recs == M.sort_records(marked)
    sizes, _ = M.member_sizes(members)
    assert open(srt + ".bai", "rb").read() == M.canonical_bai(recs, n_ref, sizes, first)
    m = re.search(r"\[SORT\] Duplicates marked on the GPU: (\d+) records examined, (\d+) pairs, (\d+) fragments, (\d+) duplicate pairs, (\d+) duplicate fragments, "
                  r"(\d+) records newly marked; kernels: marking [0-9.]+ ms, sorts [0-9.]+ ms", err)
    assert m, err[-1500:]
    assert dict(zip(MD.COUNT_NAMES, map(int, m.groups()))) == counts
    srt0, err0 = _run(tmp_path, "sorted", fa, inp + ["--bam", "--sort"])
    recs0 = split_bam(srt0)[3]
    assert recs0 == M.sort_records(unsorted) and not any(MD.parse(r)[2] & 0x400 for r in recs0) and "[SORT]" not in err0


def test_cli_markdup_needs_sort(tmp_path):
    _, err = _run(tmp_path, "refused", str(tmp_path / "none.fa"), ["-q", str(tmp_path / "none.fq"), "--bam", "--markdup"], code=1)
    assert "--markdup needs --sort: duplicates are found among the records the sorter holds" in err
    assert "HIP backend (gfx950)" not in err and not os.path.exists(tmp_path / "refused" / "out.bam")
