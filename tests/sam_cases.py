"""Constructed mapping results and what the record writers must make of them, shared by the host formatter's tests (tests/test_host_units.py),
the model's (tests/test_sam_model.py) and the GPU writers' (tests/test_gpu_sam_records.py).

Every expected line or field in CASES is typed by hand from the rules the writers cite (SAMWriter.cpp:98-373, BAMWriter.cpp:147-433,
GenericReadWriter.h:190-273, AlignmentBuffer.cpp:165-203); none is taken from any writer's output.  random_batch() makes seeded batches of
consistent records nobody typed, for comparing writers with each other."""
import random
import struct

import numpy as np

CHR1 = "GGACGTNACGTAGG" + "ACGT" * 100   # (the SLAM-seq cases read its first bases)
CHR2 = "ACGTTGCATGCC" + "TGCA" * 100
CONTIGS = [("chr1", len(CHR1), CHR1), ("chr2", len(CHR2), CHR2)]
TAGS = "AS:i:80\tNM:i:0\tNH:i:1\tXI:f:1\tX0:i:1\tXE:i:7\tXR:i:10\tMD:Z:10"   # of hit() as it stands


class Hit:
    def __init__(self, mapped=1, contig=0, pos=100, reverse=0, mapq=60, score=80, identity=1.0, nm=0, qstart=0, qend=0, n_cand=1, n_best=1, votes=7, pair=0, cigar="10M", md="10"):
        self.__dict__.update(locals())
        del self.__dict__["self"]

    def spec(self):
        num = lambda v: "%.9g" % v if isinstance(v, (float, np.floating)) else "%d" % v   # (nine digits: a float32 comes back as it was)
        return "hit %d %d %d %d %d %s %s %d %d %d %d %d %s %d %s %s" % (self.mapped, self.contig, self.pos, self.reverse, self.mapq, num(self.score), num(self.identity), self.nm,
                                                                      self.qstart, self.qend, self.n_cand, self.n_best, num(self.votes), self.pair, self.cigar or "-", self.md or "-")


hit = Hit


class Rec:
    """a read and its topn results.  row: the bases of its row; qual: the characters of its quality row (the first q - 1 of the string at most);
    qual_len: the length of the string as the parser holds it (default: that of qual); empty: the read has no sequence and is discarded"""

    def __init__(self, name, row, qual, *hits, unit=0, polya=0, seq_len=None, qual_len=None):
        self.name, self.row, self.qual, self.hits, self.unit, self.polya = name, row or "", qual or "", list(hits), unit, polya
        self.seq_len = len(self.row) if seq_len is None else seq_len
        self.qual_len = len(self.qual) if qual_len is None else qual_len
        self.empty = self.seq_len == 0
        self.hit = self.hits[0]

    def spec(self):
        return ["rec %s %s %s %d %d %d %d" % (self.name, self.row or "-", self.qual or "*", self.seq_len, self.unit, self.polya, self.qual_len)] + [h.spec() for h in self.hits]


rec = Rec


class Batch:
    """opts: the model's (tests/sam_model.py Model), silent = 1: `clip` stands for --silent-clip, not --hard-clip; those only the host formatter knows (topn, strata, coverage, snp) go through to its driver"""

    def __init__(self, opts, recs, contigs=CONTIGS, q=16):
        self.opts, self.recs, self.contigs, self.q = dict(opts), list(recs), contigs, q

    def spec(self):
        """the text tests/cpp/host_units_driver.cpp's `format` mode reads"""
        lines = ["opt q %d" % self.q] + ["contig %s %s" % (name, bases or "N") for name, length, bases in self.contigs]
        o = dict(self.opts)
        o.pop("silent", 0)   # (--silent-clip and --hard-clip differ in the CIGAR, which is given; the writers clip alike)
        if o.pop("alt_scoring", 0):
            o["slam_seq"] = o.get("slam_seq", 0) | 2   # (the formatter reads the score tables' switch from bit 1)
        for k, v in o.items():
            if not (k == "rg" and not v):
                lines.append("opt %s %s" % (k, "%.9g" % v if isinstance(v, (float, np.floating)) else v))
        for r in self.recs:
            lines += r.spec()
        return "\n".join(lines) + "\n"


def decode_records(data):
    """uncompressed BAM records -> the dicts tests/test_gpu_bam.py's decode_bam makes of a file's"""
    recs, at = [], 0
    while at < len(data):
        block, = struct.unpack_from("<i", data, at)
        ref_id, pos, bin_mq_nl, flag_nc, l_seq, mate_ref, mate_pos, tlen = struct.unpack_from("<iiIIiiii", data, at + 4)
        l_name, n_cig = bin_mq_nl & 0xFF, flag_nc & 0xFFFF
        p = at + 36
        name = data[p:p + l_name - 1]; p += l_name
        cigar = data[p:p + 4 * n_cig]; p += 4 * n_cig
        seq = data[p:p + (l_seq + 1) // 2]; p += (l_seq + 1) // 2
        qual = data[p:p + l_seq]; p += l_seq
        tags = data[p:at + 4 + block]
        recs.append(dict(name=name, ref_id=ref_id, pos=pos, bin=bin_mq_nl >> 16, mapq=(bin_mq_nl >> 8) & 0xFF, flag=flag_nc >> 16, cigar=cigar, l_seq=l_seq,
                         seq=seq, qual=qual, mate_ref=mate_ref, mate_pos=mate_pos, tlen=tlen, tags=tags))
        at += 4 + block
    assert at == len(data)
    return recs


class Run:
    """one batch through one writer: check(out, counts) holds the typed expectations -- out: the SAM lines, or with bam the decoded records;
    counts: reads counted, reads mapped, records written, pairs with both mates mapped, of those broken, insert sizes of the others"""

    def __init__(self, name, opts, recs, check, bam=False):
        self.name, self.batch, self.check, self.bam = name, Batch(opts, recs), check, bam


# ---- the hand-typed cases ---------------------------------------------------------------------------------------------------------------

def _single_end(sam, counts):
    assert sam == [
        "fwd\t0\tchr1\t101\t60\t10M\t*\t0\t0\tACGTACGTAC\tIIIIIHHHHH\t" + TAGS,
        # reverse strand: the reverse complement and the reversed qualities; AS and XE are truncated to integers, XI is printed with %g
        "rev\t16\tchr2\t8\t37\t10M\t*\t0\t0\tGTAACCGGTT\tJIHGFEDCBA\tAS:i:75\tNM:i:1\tNH:i:2\tXI:f:0.9\tX0:i:2\tXE:i:6\tXR:i:10\tMD:Z:4A5",
        "noqual\t0\tchr1\t101\t60\t10M\t*\t0\t0\tACGTACGTAC\t*\t" + TAGS,
        "unmapped\t4\t*\t0\t0\t*\t*\t0\t0\tACGTACGTAC\tIIIIIHHHHH",
        # a quality string shorter than the read: SAM prints what there is
        "shortq\t0\tchr1\t101\t60\t10M\t*\t0\t0\tACGTACGTAC\tABCDEF\t" + TAGS,
        "shortq_rev\t16\tchr1\t101\t60\t10M\t*\t0\t0\tGTACGTACGT\tFEDCBA\t" + TAGS,
    ]
    assert counts == [6, 5, 6, 0, 0, 0]   # the empty read is neither counted nor written


def _bam_short_qualities(recs, counts):
    pad = bytes([ord(":") - 33]) * 4
    assert [(r["name"], r["flag"], r["ref_id"], r["pos"], r["mapq"]) for r in recs] == [(b"shortq", 0, 0, 100, 60), (b"shortq_rev", 16, 0, 100, 60), (b"noqual", 0, 0, 100, 60), (b"unmapped", 4, -1, -1, 0)]
    assert recs[0]["qual"] == bytes(c - 33 for c in b"ABCDEF") + pad
    assert recs[1]["qual"] == bytes(c - 33 for c in b"FEDCBA") + pad
    assert recs[2]["qual"] == bytes([ord(":") - 33]) * 10   # no quality string: ':' for every base (BAMWriter.cpp:223-228)
    assert recs[3]["qual"] == bytes(c - 33 for c in b"ABCDEF") + pad
    nib = {"A": 1, "C": 2, "G": 4, "T": 8}
    pack = lambda s: bytes(nib[s[i]] << 4 | nib[s[i + 1]] for i in range(0, len(s), 2))
    assert recs[0]["seq"] == pack("ACGTACGTAC") and recs[1]["seq"] == pack("GTACGTACGT")
    assert recs[0]["cigar"] == struct.pack("<I", 10 << 4) and recs[3]["cigar"] == b""
    assert recs[0]["tags"] == (b"ASi" + struct.pack("<i", 80) + b"NMi" + struct.pack("<i", 0) + b"NHi" + struct.pack("<i", 1) + b"XIf" + struct.pack("<f", 1.0) +
                               b"X0i" + struct.pack("<i", 1) + b"XEi" + struct.pack("<i", 7) + b"XRi" + struct.pack("<i", 10) + b"MDZ10\0")
    assert recs[3]["tags"] == b""
    assert all((r["mate_ref"], r["mate_pos"], r["tlen"]) == (-1, -1, 0) for r in recs)
    assert counts == [4, 3, 4, 0, 0, 0]


def _filter(sam, counts):
    assert [l.split("\t")[:2] for l in sam] == [["at", "0"], ["below", "4"]]
    assert counts == [2, 1, 2, 0, 0, 0]


def _clip_rg_polya(sam, counts):
    assert sam == [
        # bases 2..6 of the reverse complement GTACGTACGT and of the reversed qualities JIHGFEDCBA; RG in front of the tags, XA:i behind X0:i
        "clip\t16\tchr1\t101\t60\t2H5M3H\t*\t0\t0\tACGTA\tHGFED\tRG:Z:grp\tAS:i:80\tNM:i:0\tNH:i:1\tXI:f:1\tX0:i:1\tXA:i:3\tXE:i:7\tXR:i:5\tMD:Z:5",
        "unmapped\t4\t*\t0\t0\t*\t*\t0\t0\tACGTACGTAC\tABCDEFGHIJ\tXA:i:0\tRG:Z:grp",   # an unmapped record: RG behind everything else
    ]
    assert counts == [2, 1, 2, 0, 0, 0]


def _no_unal(sam, counts):
    assert sam == ["clip\t16\tchr1\t101\t60\t2H5M3H\t*\t0\t0\tGTACGTACGT\tJIHGFEDCBA\tAS:i:80\tNM:i:0\tNH:i:1\tXI:f:1\tX0:i:1\tXE:i:7\tXR:i:5\tMD:Z:5"]   # no clip, no XA:i
    assert counts == [2, 1, 1, 0, 0, 0]


def pair(name, h1, h2, unit=0):
    return [rec(name + "/1", "ACGTACGTAC", "ABCDEFGHIJ", h1, unit=unit), rec(name + "/2", "AACCGGTTAC", "KLMNOPQRST", h2, unit=unit)]


def _pair_branches_sam(sam, counts):
    t1, t2 = TAGS, TAGS.replace("XR:i:10", "XR:i:8")
    assert sam == [
        # the second mate's record comes first; 58 = 150 + 10 - 2 (clipped at the end) - 100
        "fr/2\t147\tchr1\t151\t60\t10M\t=\t101\t-58\tGTAACCGGTT\tTSRQPONMLK\t" + t2,
        "fr/1\t99\tchr1\t101\t60\t10M\t=\t151\t58\tACGTACGTAC\tABCDEFGHIJ\t" + t1,
        "rf/2\t163\tchr1\t101\t60\t10M\t=\t151\t58\tAACCGGTTAC\tKLMNOPQRST\t" + t1,
        "rf/1\t83\tchr1\t151\t60\t10M\t=\t101\t-58\tGTACGTACGT\tJIHGFEDCBA\t" + t2,
        "none/2\t141\t*\t0\t0\t*\t*\t0\t0\tAACCGGTTAC\tKLMNOPQRST",
        "none/1\t77\t*\t0\t0\t*\t*\t0\t0\tACGTACGTAC\tABCDEFGHIJ",
        "m2only/2\t153\tchr1\t151\t60\t10M\t=\t151\t0\tGTAACCGGTT\tTSRQPONMLK\t" + t1,
        "m2only/1\t69\tchr1\t151\t0\t*\t=\t151\t0\tACGTACGTAC\tABCDEFGHIJ",
        "m1only/2\t133\tchr1\t101\t0\t*\t=\t101\t0\tAACCGGTTAC\tKLMNOPQRST",
        "m1only/1\t73\tchr1\t101\t60\t10M\t=\t101\t0\tACGTACGTAC\tABCDEFGHIJ\t" + t1,
        # both mapped, not a proper pair: the mate's contig by name, its strand in 0x20, TLEN 0
        "contigs/2\t145\tchr2\t151\t60\t10M\tchr1\t101\t0\tGTAACCGGTT\tTSRQPONMLK\t" + t1,
        "contigs/1\t97\tchr1\t101\t60\t10M\tchr2\t151\t0\tACGTACGTAC\tABCDEFGHIJ\t" + t1,
    ]   # (the lost pair: no record, not counted)
    # pairs with both mates mapped: fr, rf, contigs; broken: contigs; insert sizes of the others: 60 + 60
    assert counts == [12, 8, 12, 3, 1, 120]


def _pair_branches_bam(recs, counts):
    # BAM: positions 0-based, TLEN over the whole read (60 = 150 + 10 - 100)
    assert [(r["name"], r["flag"], r["ref_id"], r["pos"], r["mate_ref"], r["mate_pos"], r["tlen"]) for r in recs] == [
        (b"fr/2", 147, 0, 150, 0, 100, -60), (b"fr/1", 99, 0, 100, 0, 150, 60),
        (b"rf/2", 163, 0, 100, 0, 150, 60), (b"rf/1", 83, 0, 150, 0, 100, -60),
        (b"none/2", 141, -1, -1, -1, -1, 0), (b"none/1", 77, -1, -1, -1, -1, 0),
        (b"m2only/2", 153, 0, 150, 0, 150, 0), (b"m2only/1", 69, 0, 150, 0, 150, 0),
        (b"m1only/2", 133, 0, 100, 0, 100, 0), (b"m1only/1", 73, 0, 100, 0, 100, 0),
        (b"contigs/2", 145, 1, 150, 0, 100, 0), (b"contigs/1", 97, 0, 100, 1, 150, 0),
    ]
    assert counts == [12, 8, 12, 3, 1, 120]


def _insert_window(sam, counts):
    assert [tuple(l.split("\t")[i] for i in (0, 1, 6, 8)) for l in sam] == [
        ("at_min/2", "147", "=", "-40"), ("at_min/1", "99", "=", "40"), ("at_max/2", "147", "=", "-60"), ("at_max/1", "99", "=", "60"),
        ("below/2", "145", "chr1", "0"), ("below/1", "97", "chr1", "0"), ("above/2", "145", "chr1", "0"), ("above/1", "97", "chr1", "0"),
        ("strand/2", "129", "chr1", "0"), ("strand/1", "65", "chr1", "0"),
        ("failed/2", "145", "chr1", "0"), ("failed/1", "97", "chr1", "0"),   # NGM_PAIR_FAILED: not proper, though its geometry is
    ]
    assert counts == [12, 12, 12, 6, 3, 40 + 60 + 50]   # broken: below, above, strand; the failed pair's 50 counts as an insert size


def _zs_single(sam, counts):
    assert [l.split("\t")[14] for l in sam] == ["ZS:Z:++", "ZS:Z:-+"]


def _zs_pairs(sam, counts):
    assert [(l.split("\t")[0], l.split("\t")[14]) for l in sam] == [("fr/2", "ZS:Z:+-"), ("fr/1", "ZS:Z:++"), ("rf/2", "ZS:Z:--"), ("rf/1", "ZS:Z:-+")]


def _zs_bam(recs, counts):
    assert recs[0]["tags"][21:27] == b"ZSZ-+\0"   # behind AS, NM and NH (7 bytes each)


_RA = ["3,0,0,0,0,0,1,0,0,1,0,0,2,0,0,0,1,0,1,0,1,0,0,0,0", "2,0,0,0,0,0,2,0,0,0,0,0,2,0,0,0,0,0,3,0,0,0,0,0,0", "1,0,1,0,0,0,2,0,0,0,0,0,3,0,0,0,0,0,3,0,0,0,0,0,0"]


def _slam_sam(sam, counts):
    assert [l.split("\t")[19:] for l in sam] == [
        ["TC:i:1", "RA:Z:" + _RA[0], "MP:Z:20:5:5,9:7:7,16:9:9"],   # type = 5 x reference class + read class (A C G T other): N>A, C>N, T>C
        ["TC:i:0", "RA:Z:" + _RA[1]],                                  # no mismatch: no MP
        ["TC:i:1", "RA:Z:" + _RA[2], "MP:Z:2:1:1"],                   # reverse strand: TC counts A>G
    ]
    assert [l.split("\t")[9] for l in sam] == ["ACGTAANGCA", "ACGTTTCATG", "GCGTTGCATG"]


def _slam_bam(recs, counts):
    tail = lambda r: r["tags"][r["tags"].index(b"TCi"):]
    assert tail(recs[0]) == b"TCi" + struct.pack("<i", 1) + b"RAZ" + _RA[0].encode() + b",\0MPZ20:5:5,9:7:7,16:9:9\0"   # BAM: a comma behind every count
    assert tail(recs[1]) == b"TCi" + struct.pack("<i", 0) + b"RAZ" + _RA[1].encode() + b",\0"
    assert tail(recs[2]) == b"TCi" + struct.pack("<i", 1) + b"RAZ" + _RA[2].encode() + b",\0MPZ2:1:1\0"


def _cases():
    c = {}
    c["single_end"] = [Run("single_end", {}, [
        rec("fwd", "ACGTACGTAC", "IIIIIHHHHH", hit()),
        rec("rev", "AACCGGTTAC", "ABCDEFGHIJ", hit(reverse=1, pos=7, contig=1, mapq=37, score=75.7, identity=0.9, nm=1, n_best=2, votes=6.9, md="4A5")),
        rec("noqual", "ACGTACGTAC", "", hit()),
        rec("empty", "", "", hit(mapped=0), seq_len=0),
        rec("unmapped", "ACGTACGTAC", "IIIIIHHHHH", hit(mapped=0)),
        rec("shortq", "ACGTACGTAC", "ABCDEF", hit()),
        rec("shortq_rev", "ACGTACGTAC", "ABCDEF", hit(reverse=1)),
    ], _single_end)]
    c["bam_short_qualities"] = [Run("bam_short_qualities", {}, [
        rec("shortq", "ACGTACGTAC", "ABCDEF", hit()),
        rec("shortq_rev", "ACGTACGTAC", "ABCDEF", hit(reverse=1)),
        rec("noqual", "ACGTACGTAC", "", hit()),
        rec("unmapped", "ACGTACGTAC", "ABCDEF", hit(mapped=0)),
    ], _bam_short_qualities, bam=True)]
    for name, opts, at, below in [
        ("min-mq", {"min_mq": 20}, dict(mapq=20), dict(mapq=19)),
        ("min-identity", {"min_identity": 0.9}, dict(identity=0.9), dict(identity=0.8999)),
        # a fraction of the 10 bases: 5 residues pass, 4 do not
        ("min-residues-fraction", {"min_residues": 0.5}, dict(qstart=3, qend=2, cigar="3S5M2S", md="5"), dict(qstart=3, qend=3, cigar="3S4M3S", md="4")),
        # above 1: a count
        ("min-residues-count", {"min_residues": 8}, dict(qstart=1, qend=1, cigar="1S8M1S", md="8"), dict(qstart=2, qend=1, cigar="2S7M1S", md="7")),
    ]:
        c["filter-" + name] = [Run("filter-" + name, opts, [rec("at", "ACGTACGTAC", "IIIIIIIIII", hit(**at)), rec("below", "ACGTACGTAC", "IIIIIIIIII", hit(**below))], _filter)]
    clip = lambda: [rec("clip", "ACGTACGTAC", "ABCDEFGHIJ", hit(reverse=1, qstart=2, qend=3, cigar="2H5M3H", md="5"), polya=3),
                    rec("unmapped", "ACGTACGTAC", "ABCDEFGHIJ", hit(mapped=0))]
    c["hard_clip"] = [Run("clip_rg_polya", {"clip": 1, "rg": "grp", "xa_tag": 1}, clip(), _clip_rg_polya), Run("no_unal", {"no_unal": 1}, clip(), _no_unal)]
    branches = lambda: (pair("fr", hit(pos=100), hit(pos=150, reverse=1, qend=2)) +      # proper, first mate forward: TLEN from the aligned end of the second mate
                        pair("rf", hit(pos=150, reverse=1, qend=2), hit(pos=100)) +      # proper, first mate reverse
                        pair("none", hit(mapped=0), hit(mapped=0)) +
                        pair("m2only", hit(mapped=0), hit(pos=150, reverse=1)) +
                        pair("m1only", hit(pos=100), hit(mapped=0)) +
                        pair("contigs", hit(pos=100), hit(pos=150, reverse=1, contig=1)) +
                        pair("lost", hit(pos=100, pair=4), hit(pos=150, reverse=1)))
    c["pair_branches"] = [Run("pair_branches_sam", {"paired": 1}, branches(), _pair_branches_sam), Run("pair_branches_bam", {"paired": 1}, branches(), _pair_branches_bam, bam=True)]
    # the distance is the difference of the positions plus the length (10) of the mate on the left
    c["insert_window"] = [Run("insert_window", {"paired": 1, "min_insert": 40, "max_insert": 60},
                              pair("at_min", hit(pos=100), hit(pos=130, reverse=1)) + pair("at_max", hit(pos=100), hit(pos=150, reverse=1)) +
                              pair("below", hit(pos=100), hit(pos=129, reverse=1)) + pair("above", hit(pos=100), hit(pos=151, reverse=1)) +
                              pair("strand", hit(pos=100), hit(pos=140)) + pair("failed", hit(pos=100, pair=2), hit(pos=140, reverse=1)), _insert_window)]
    c["zs_tag"] = [Run("zs_single", {"bs_mapping": 1}, [rec("f", "ACGTACGTAC", "", hit()), rec("r", "ACGTACGTAC", "", hit(reverse=1))], _zs_single),
                   Run("zs_pairs", {"bs_mapping": 1, "paired": 1}, pair("fr", hit(pos=100), hit(pos=150, reverse=1)) + pair("rf", hit(pos=150, reverse=1), hit(pos=100)), _zs_pairs),
                   Run("zs_bam", {"bs_mapping": 1}, [rec("r", "ACGTACGTAC", "", hit(reverse=1))], _zs_bam, bam=True)]
    slam = lambda: [
        # chr1 from base 2: ACGTNACGTA.  Column 5 is N in the reference, column 7 N in the read, column 9 a T>C conversion
        rec("mis", "ACGTAANGCA", "", hit(pos=2, nm=3, md="4N1C1T1")),
        # chr2 from base 0: ACG-TTgCATG: one base inserted behind ACG, the reference's G deleted behind TT, no mismatch
        rec("indel", "ACGTTTCATG", "", hit(pos=0, contig=1, cigar="3M1I2M1D4M", md="5^G4")),
        # reverse strand, chr2 from base 0: ACGTTGCATG against the read's reverse complement GCGTTGCATG: A>G in column 1
        rec("rev", "CATGCAACGC", "", hit(pos=0, contig=1, reverse=1, nm=1, md="0A9")),
    ]
    c["slam_seq"] = [Run("slam_sam", {"slam_seq": 1}, slam(), _slam_sam), Run("slam_bam", {"slam_seq": 1}, slam(), _slam_bam, bam=True)]
    return c


CASES = _cases()
ALL_RUNS = [r for runs in CASES.values() for r in runs]


# ---- random consistent batches -----------------------------------------------------------------------------------------------------------

BIG_CONTIGS = [("chrA", (1 << 31) - 1, None), ("c2", 5000000, None), ("a_contig_with_a_longer_name.3", 1 << 30, None)]
_QUAL_ALPHABET = "".join(chr(c) for c in range(33, 127) if chr(c) != "*")   # ('*' alone is the text formats' "no quality string")
_NAME_ALPHABET = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789/:_.-"
RANDOM_OPTS = dict(min_mq=10, min_identity=0.65, min_insert=50, max_insert=1000)
POS_LIMIT = (1 << 31) - 2000


def _random_cigar(rng, L, qs, qe, clip):
    """a CIGAR whose M and I operations consume the L - qs - qe aligned bases, and an MD string beside it"""
    left = L - qs - qe
    ops = []
    while left > 0:
        n = min(left, rng.randint(1, 40))
        op = "M" if not ops or ops[-1][1] != "M" else rng.choice("ID")
        if op == "D":
            n = rng.randint(1, 6)
        else:
            left -= n
        ops.append((n, op))
    if ops and ops[-1][1] == "D":
        ops.pop()
    mark = {"none": "S", "hard": "H", "silent": ""}[clip]
    text = ("%d%s" % (qs, mark) if qs and mark else "") + "".join("%d%s" % o for o in ops) + ("%d%s" % (qe, mark) if qe and mark else "")
    md = "".join(rng.choice(["%d" % rng.randint(0, 60), rng.choice("ACGTN"), "^" + rng.choice(["A", "CG", "TTT"])]) for _ in range(rng.randint(1, 6)))
    return text, md


def _random_read(rng, q, name, mapped_ok):
    L = 0 if rng.random() < 0.02 and not mapped_ok else rng.randint(1, q - 1)
    row = "".join(rng.choice("ACGT") if rng.random() < 0.95 else rng.choice("NRYKMSW") for _ in range(L))
    kind = rng.random()
    qual_len = 0 if kind < 0.1 else rng.randint(1, max(1, L - 1)) if kind < 0.3 else L if kind < 0.85 else rng.randint(L + 1, L + 30) if kind < 0.95 else rng.randint(q, q + 200)
    qual = "".join(rng.choice(_QUAL_ALPHABET) for _ in range(min(qual_len, q - 1)))
    return name, row, qual, qual_len


def _random_hit(rng, L, clip, fate, contig, pos, reverse, pair):
    """fate: 'pass', 'unmapped', or the filter the hit fails: 'mq', 'identity', 'residues'"""
    if fate == "unmapped":
        return hit(mapped=0, contig=0, pos=0, mapq=0, score=0, identity=0.0, n_cand=0, n_best=0, votes=np.float32(rng.random() * 5), pair=pair, cigar="", md="")
    if fate == "residues":   # fewer than half of the bases aligned
        qs = rng.randint(L // 2 + 1, L)
        qe = rng.randint(0, L - qs)
    else:
        qs = rng.randint(0, L // 4) if rng.random() < 0.5 else 0
        qe = rng.randint(0, L // 2 - qs) if rng.random() < 0.5 else 0
    cigar, md = _random_cigar(rng, L, qs, qe, clip)
    identity = np.float32(rng.uniform(0.3, 0.6499) if fate == "identity" else rng.choice([0.65, 1.0, rng.uniform(0.65, 1.0), rng.randint(6500, 10000) / 10000.0]))
    return hit(mapped=1, contig=contig, pos=pos, reverse=reverse, mapq=rng.randint(0, 9) if fate == "mq" else rng.randint(10, 60), score=np.float32(rng.uniform(-20, 3000)),
               identity=identity, nm=rng.randint(0, 30), qstart=qs, qend=qe, n_cand=rng.randint(1, 50), n_best=rng.randint(1, 9), votes=np.float32(rng.uniform(0, 400)), pair=pair, cigar=cigar, md=md)


def _random_place(rng, span=2000):
    contig = rng.randrange(len(BIG_CONTIGS))
    top = min(BIG_CONTIGS[contig][1], POS_LIMIT) - span
    return contig, rng.choice([rng.randrange(0, 100000), rng.randrange(0, top), top - rng.randrange(0, 1000)])


def random_batch(seed, units, paired, clip="none", no_unal=0, rg="", polya=0, bs_mapping=0, q=80):
    """`units` reads or pairs with consistent results: every writer branch, every filter, both strands, short and absent quality strings"""
    rng = random.Random(seed)
    opts = dict(RANDOM_OPTS, paired=int(paired), clip=int(clip != "none"), silent=int(clip == "silent"), no_unal=no_unal, rg=rg, xa_tag=polya, bs_mapping=bs_mapping, min_residues=0.5)
    if not paired:
        opts.update(min_insert=0, max_insert=0)
    failing = lambda: rng.choice(["unmapped", "unmapped", "unmapped", "mq", "identity", "residues"])
    recs = []
    for u in range(units):
        name = "".join(rng.choice(_NAME_ALPHABET) for _ in range((252 if paired else 254) if rng.random() < 0.01 else rng.randint(1, 40)))   # (with "/1": 254 bytes, the most BAM holds)
        if not paired:
            fate = "pass" if rng.random() < 0.7 else failing()
            nm, row, qual, qual_len = _random_read(rng, q, name, fate != "unmapped")
            contig, pos = _random_place(rng)
            recs.append(rec(nm, row, qual, _random_hit(rng, len(row), clip, fate, contig, pos, rng.randint(0, 1), 0), polya=rng.randint(0, 30) if polya else 0,
                            seq_len=0 if rng.random() < 0.01 else max(len(row), 1), qual_len=qual_len))
            continue
        kind = rng.choice(["none", "only1", "only2", "proper", "proper", "proper", "not_proper", "not_proper", "lost"] if rng.random() < 0.9 else ["lost", "empty", "none"])
        f1 = "pass" if kind in ("only1", "proper", "not_proper", "lost") else failing()
        f2 = "pass" if kind in ("only2", "proper", "not_proper", "lost") else failing()
        r1, r2 = _random_read(rng, q, name + "/1", f1 != "unmapped"), _random_read(rng, q, name + "/2", f2 != "unmapped")
        L1, L2 = len(r1[1]), len(r2[1])
        c1, p1 = _random_place(rng)
        c2, p2, rev1, rev2, flags = c1, p1, rng.randint(0, 1), 0, rng.choice([0, 1])
        if kind == "proper":   # the same contig, opposite strands, the distance inside the window
            rev2 = 1 - rev1
            d = rng.randint(50, 1000)
            p2 = p1 + d - L1 if rng.random() < 0.5 and d - L1 > 0 else max(0, p1 - (d - L2)) if d - L2 >= 0 else p1 + max(d - L1, 1)
        else:
            why = rng.choice(["contig", "strand", "far", "near", "flag"])
            rev2 = rev1 if why == "strand" else 1 - rev1
            c2, p2 = (_random_place(rng) if why == "contig" else (c1, p1 + rng.randint(1500, 1900)) if why == "far" else (c1, p1 + 1) if why == "near" else (c1, p1 + rng.randint(60, 500)))
            flags = 2 if why == "flag" else flags
        if kind == "lost":
            flags |= 4
        h1, h2 = _random_hit(rng, L1, clip, f1, c1, p1, rev1, flags), _random_hit(rng, L2, clip, f2, c2, p2, rev2, flags if rng.random() < 0.5 else flags & 1)
        empty = kind == "empty"
        recs.append(rec(r1[0], r1[1], r1[2], h1, polya=rng.randint(0, 30) if polya else 0, seq_len=0 if empty and rng.random() < 0.5 else max(L1, 1), qual_len=r1[3]))
        recs.append(rec(r2[0], r2[1], r2[2], h2, polya=rng.randint(0, 30) if polya else 0, seq_len=0 if empty and recs[-1].seq_len else max(L2, 1), qual_len=r2[3]))
    return Batch(opts, recs, contigs=BIG_CONTIGS, q=q)


# single-end and paired x the three clip modes, each with a set of the four switches (no_unal, rg, polya, bs_mapping) and with its complement
RANDOM_CONFIGS = []
for _i, (_paired, _clip) in enumerate([(p, c) for p in (0, 1) for c in ("none", "hard", "silent")]):
    _bits = [0b0000, 0b0110, 0b0101, 0b1010, 0b0011, 0b1001][_i]
    for _b in (_bits, _bits ^ 0b1111):
        RANDOM_CONFIGS.append(dict(paired=_paired, clip=_clip, no_unal=_b & 1, rg="grp-%d" % _i if _b & 2 else "", polya=(_b >> 2) & 1, bs_mapping=(_b >> 3) & 1))
RANDOM_UNITS = 2048


def random_config_id(cfg):
    return "%s-%s%s%s%s%s" % ("pe" if cfg["paired"] else "se", cfg["clip"], "-no_unal" if cfg["no_unal"] else "", "-rg" if cfg["rg"] else "", "-polya" if cfg["polya"] else "",
                              "-bs" if cfg["bs_mapping"] else "")


_batches = {}


def random_config_batch(i):
    """batch i of RANDOM_CONFIGS, made once per process"""
    if i not in _batches:
        _batches[i] = random_batch(1000 + i, RANDOM_UNITS, **RANDOM_CONFIGS[i])
    return _batches[i]
