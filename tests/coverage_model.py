"""The definition of `ngm-hip --coverage`'s file in plain Python / numpy, written from INTEGRATION.md and not from csrc/coverage.h: the
oracle of tests/test_coverage_host.py and tests/test_gpu_coverage.py.

An alignment covers the reference bases under its M, = and X operations; D and N advance without covering; I, S, H and P do neither; what
lies past the contig's last base is clipped.  A line is contig, start (0-based), end (exclusive), depth (> 0), tab-separated: one per maximal
run of equal depth inside one contig, contigs in reference order."""
import re

import numpy as np

_OP = re.compile(r"(\d+)([MIDNSHP=X])")
BAM_OPS = "MIDNSHP=X"


def cigar_ops(cigar):
    if isinstance(cigar, bytes):
        cigar = cigar.decode()
    assert sum(len(m.group(0)) for m in _OP.finditer(cigar)) == len(cigar), cigar
    return [(int(n), op) for n, op in _OP.findall(cigar)]


def covered_blocks(pos0, cigar, contig_len):
    """[(begin, end)] of one alignment, one per covering operation, clipped"""
    out, at = [], pos0
    for n, op in cigar_ops(cigar):
        if op in "M=X":
            b, e = max(at, 0), min(at + n, contig_len)
            if b < e:
                out.append((b, e))
            at += n
        elif op in "DN":
            at += n
    return out


def matched_bases(cigar):
    return sum(n for n, op in cigar_ops(cigar) if op in "M=X")


def depths(contigs, alignments):
    """per contig an int64 array of the depth of every base; contigs: [(name, length)], alignments: [(contig index, pos0, CIGAR)]"""
    diff = [np.zeros(length + 1, dtype=np.int64) for _, length in contigs]
    for c, pos0, cigar in alignments:
        for b, e in covered_blocks(pos0, cigar, contigs[c][1]):
            diff[c][b] += 1
            diff[c][e] -= 1
    return [np.cumsum(d)[:-1] for d in diff]


def bedgraph(contigs, alignments):
    out = []
    for (name, length), d in zip(contigs, depths(contigs, alignments)):
        if length == 0:
            continue
        if isinstance(name, bytes):
            name = name.decode()
        starts = np.concatenate(([0], np.flatnonzero(d[1:] != d[:-1]) + 1))
        ends = np.concatenate((starts[1:], [length]))
        for s, e in zip(starts.tolist(), ends.tolist()):
            if d[s] > 0:
                out.append("%s\t%d\t%d\t%d\n" % (name, s, e, d[s]))
    return "".join(out).encode()


def alignments_of_sam(lines, contigs):
    """the records that count (flag bits 0x4 and 0x100 clear) of the lines of a SAM file"""
    index = {(n.decode() if isinstance(n, bytes) else n): i for i, (n, _) in enumerate(contigs)}
    out = []
    for line in lines:
        if line.startswith("@"):
            continue
        f = line.rstrip("\n").split("\t")
        if int(f[1]) & 0x104:
            continue
        out.append((index[f[2]], int(f[3]) - 1, f[5]))
    return out


def sam_contigs(lines):
    return [(f[1][3:], int(f[2][3:])) for f in (l.rstrip("\n").split("\t") for l in lines if l.startswith("@SQ"))]


def alignments_of_bam(recs):
    """... of the records tests/test_gpu_bam.decode_bam returns"""
    out = []
    for r in recs:
        if r["flag"] & 0x104:
            continue
        words = np.frombuffer(r["cigar"], dtype="<u4")
        out.append((r["ref_id"], r["pos"], "".join("%d%s" % (w >> 4, BAM_OPS[w & 15]) for w in words.tolist())))
    return out


def totals(text):
    """(lines, highest depth, sum of (end - start) * depth) of a bedGraph file's bytes"""
    n, top, total = 0, 0, 0
    for line in text.decode().splitlines():
        _, s, e, d = line.split("\t")
        n += 1
        top = max(top, int(d))
        total += (int(e) - int(s)) * int(d)
    return n, top, total


# ---- the unit cases both test files run: name -> (contigs, alignments) ---------------------------------------------------------------
ONE = [("chr1", 1000)]
TWO = [("chrA", 100), ("chrB", 50)]
UNIT_CASES = {
    "nothing": (TWO, []),
    "one-10M": (ONE, [(0, 5, "10M")]),
    "ends-on-last-base": (ONE, [(0, 990, "10M")]),
    "past-the-end": (ONE, [(0, 995, "10M"), (0, 999, "3S20M"), (0, 1000, "5M"), (0, 2000, "5M")]),
    "same-depth-across-contigs": (TWO, [(0, 90, "10M"), (1, 0, "10M")]),
    "deletion": (ONE, [(0, 100, "5M3D5M")]),
    "skip": (ONE, [(0, 100, "5M100N5M")]),
    "clips-and-insertion": (ONE, [(0, 100, "3S5M2I5M4H")]),
    "eq-and-x": (ONE, [(0, 100, "4=1X4=")]),
    "abutting": (ONE, [(0, 100, "10M"), (0, 110, "10M")]),
    "contention": (ONE, [(0, 300, "20M")] * 5000),
    "length-1": ([("a", 1), ("b", 1), ("c", 7)], [(0, 0, "1M"), (1, 0, "5M"), (1, 0, "1M"), (2, 6, "1M")]),
    "padding-and-empty": (ONE, [(0, 10, "5M2P5M"), (0, 40, ""), (0, 50, "0M"), (0, 60, "10S")]),
    "overlaps": (ONE, [(0, 10, "50M"), (0, 20, "50M"), (0, 30, "10M5D10M"), (0, 59, "1M"), (0, 0, "1M")]),
}
# with scan_chunk = 64 (array offsets = positions on the first contig): a run crossing offset 64, one ending exactly there, one starting
# there, one over three chunks
CHUNK_CASES = {
    "crosses-64": ([("c", 300)], [(0, 60, "10M")]),
    "ends-at-64": ([("c", 300)], [(0, 50, "14M")]),
    "starts-at-64": ([("c", 300)], [(0, 64, "10M")]),
    "three-chunks": ([("c", 300)], [(0, 60, "140M"), (0, 100, "5M")]),
    "contig-boundary-in-a-chunk": ([("c", 63), ("d", 64), ("e", 200)], [(0, 50, "13M"), (1, 0, "64M"), (2, 0, "3M"), (2, 60, "80M")]),
}
