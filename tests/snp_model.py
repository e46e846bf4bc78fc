"""The definition of `ngm-hip --snp`'s file in plain Python / numpy, written from INTEGRATION.md ("--snp") and not from csrc/snp.h: the
oracle of tests/test_snp_host.py and tests/test_gpu_snp.py.

Depth is --coverage's depth (tests/coverage_model.py).  A record walks its CIGAR over its sequence as the SAM record prints it: M, =, X, I
and S consume read bases, H and P nothing.  An M / = / X column at contig position p with read base b and reference base r adds 1 to
alt[p][b] when p is inside the contig, r (case folded) and b are one of ACGT, b != r, and the record has no quality string or the column's
Phred quality is at least Q.  p is a call when depth >= max(1, N) and float(n) >= F * float(depth) for the alternative with the largest
count n > 0, ties to the first of A, C, G, T.

A record is (contig index, 0-based position, CIGAR, sequence, qualities or None); contigs are [(name, sequence)]."""
import numpy as np

import coverage_model as CM

BASES = "ACGT"
BAM_SEQ = "=ACMGRSVTWYHKDBN"


def _s(x):
    return x.decode() if isinstance(x, bytes) else x


def pileup(contigs, records, Q):
    """per contig (depth int64[len], alt int64[len, 4])"""
    depth = CM.depths([(n, len(s)) for n, s in contigs], [(r[0], r[1], r[2]) for r in records])
    alt = [np.zeros((len(s), 4), dtype=np.int64) for _, s in contigs]
    for c, pos0, cigar, seq, qual in records:
        ref, seq = _s(contigs[c][1]).upper(), _s(seq)
        qual = None if qual is None else _s(qual)
        at, ri = pos0, 0
        for n, op in CM.cigar_ops(cigar):
            if op in "M=X":
                for k in range(n):
                    p = at + k
                    if not 0 <= p < len(ref):
                        continue
                    r, b = ref[p], seq[ri + k]
                    if r in BASES and b in BASES and b != r and (qual is None or ord(qual[ri + k]) - 33 >= Q):
                        alt[c][p, BASES.index(b)] += 1
                at += n
                ri += n
            elif op in "DN":
                at += n
            elif op in "IS":
                ri += n
        assert ri == len(seq) and (qual is None or len(qual) == len(seq)), (cigar, seq, qual)
    return depth, alt


def calls(contigs, records, N, F, Q):
    """[(contig index, 0-based position, REF, ALT, depth, n)]"""
    f = float(F)
    out = []
    depth, alt = pileup(contigs, records, Q)
    for c, (_, s) in enumerate(contigs):
        ref = _s(s).upper()
        for p in np.flatnonzero(alt[c].max(axis=1) > 0).tolist() if len(ref) else []:
            a = int(np.argmax(alt[c][p]))   # (the first of the largest)
            n, d = int(alt[c][p, a]), int(depth[c][p])
            if d >= max(1, N) and float(n) >= f * float(d):
                out.append((c, p, ref[p], BASES[a], d, n))
    return out


def header(contigs, N, F, Q):
    h = "##fileformat=VCFv4.2\n##source=ngm-hip --snp (min-cov %d, min-frac %s, min-qual %d)\n" % (N, _s(F) if isinstance(F, (str, bytes)) else repr(F), Q)
    h += "".join("##contig=<ID=%s,length=%d>\n" % (_s(n), len(s)) for n, s in contigs)
    h += '##INFO=<ID=DP,Number=1,Type=Integer,Description="records covering the base">\n'
    h += '##INFO=<ID=AO,Number=1,Type=Integer,Description="records with the ALT base at quality >= %d">\n' % Q
    return h + "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"


def vcf(contigs, records, N=10, F="0.8", Q=15):
    lines = ["%s\t%d\t.\t%s\t%s\t.\tPASS\tDP=%d;AO=%d\n" % (_s(contigs[c][0]), p + 1, r, a, d, n) for c, p, r, a, d, n in calls(contigs, records, N, F, Q)]
    return (header(contigs, N, F, Q) + "".join(lines)).encode()


def totals(contigs, records, N=10, F="0.8", Q=15):
    """what ngm_snp_stats counts after the whole file was handed out"""
    depth, alt = pileup(contigs, records, Q)
    return dict(alignments=len(records), alt_bases=int(sum(a.sum() for a in alt)), calls=len(calls(contigs, records, N, F, Q)),
                text_bytes=len(vcf(contigs, records, N, F, Q)), covered_bases=int(sum(d.sum() for d in depth)))


def parse_vcf(text):
    """[(contig name, 1-based position, REF, ALT, DP, AO)] of a file's bytes"""
    out = []
    for line in text.decode().splitlines():
        if line.startswith("#"):
            continue
        f = line.split("\t")
        info = dict(kv.split("=") for kv in f[7].split(";"))
        out.append((f[0], int(f[1]), f[3], f[4], int(info["DP"]), int(info["AO"])))
    return out


# ---- readers: the records that count (flag bits 0x4 and 0x100 clear) of the file a run wrote ------------------------------------------
def records_of_sam(lines, contigs):
    index = {_s(n): i for i, (n, _) in enumerate(contigs)}
    out = []
    for line in lines:
        if line.startswith("@"):
            continue
        f = line.rstrip("\n").split("\t")
        if int(f[1]) & 0x104:
            continue
        out.append((index[f[2]], int(f[3]) - 1, f[5], f[9], None if f[10] == "*" else f[10]))
    return out


def records_of_bam(recs):
    """... of the records tests/test_gpu_bam.decode_bam returns"""
    out = []
    for r in recs:
        if r["flag"] & 0x104:
            continue
        words = np.frombuffer(r["cigar"], dtype="<u4")
        cigar = "".join("%d%s" % (w >> 4, CM.BAM_OPS[w & 15]) for w in words.tolist())
        seq = "".join(BAM_SEQ[(r["seq"][i >> 1] >> (0 if i & 1 else 4)) & 15] for i in range(r["l_seq"]))
        qual = None if r["l_seq"] and all(q == 0xFF for q in r["qual"]) else "".join(chr(q + 33) for q in r["qual"])
        out.append((r["ref_id"], r["pos"], cigar, seq, qual))
    return out


def read_fasta(path):
    out = []
    for line in open(path):
        if line.startswith(">"):
            out.append([line[1:].split()[0], []])
        else:
            out[-1][1].append(line.strip())
    return [(n, "".join(parts)) for n, parts in out]


# ---- building records ---------------------------------------------------------------------------------------------------------------
def other(base, k=1):
    """the k-th next of ACGT behind the (upper-cased) base; behind a base that is none of them: A, C, G"""
    base = base.upper()
    return BASES[(BASES.index(base) + k) % 4] if base in BASES else BASES[k - 1]


def rec(contigs, c, pos0, cigar, subs=(), qual=None, low=()):
    """a record whose aligned columns repeat the (upper-cased) reference -- 'A' past the contig's end and for inserted and clipped bases --
    except at the read offsets of subs: an offset (-> other(reference base)) or (offset, base).  qual: None, a string, or a Phred value for
    every base, with the offsets of `low` one below it."""
    ref = _s(contigs[c][1])
    seq, at = [], pos0
    for n, op in CM.cigar_ops(cigar):
        if op in "M=X":
            seq += [ref[p].upper() if 0 <= p < len(ref) else "A" for p in range(at, at + n)]
            at += n
        elif op in "DN":
            at += n
        elif op in "IS":
            seq += ["A"] * n
    for s in subs:
        o, b = s if isinstance(s, tuple) else (s, None)
        seq[o] = b if b is not None else other(seq[o])
    if isinstance(qual, int):
        qual = "".join(chr(33 + qual - (1 if i in low else 0)) for i in range(len(seq)))
    return (c, pos0, cigar, "".join(seq), qual)


def _genome(rnd, n):
    return "".join(rnd.choice(BASES) for _ in range(n))


def random_records(rnd, contigs, n, planted=0.05):
    """n random records with random CIGARs (coverage's random shapes), 3 % random substitutions, read Ns, qualities around 15; a share
    `planted` of the positions carries a fixed alternative that 90 % of the reads over it show"""
    plant = [{p: other(_s(s)[p], rnd.randrange(1, 4)) for p in range(len(s)) if rnd.random() < planted} for _, s in contigs]
    out = []
    for _ in range(n):
        c = rnd.randrange(len(contigs))
        ref = _s(contigs[c][1])
        cigar = "".join("%d%s" % (rnd.choice([0, 1, 1, 2, 3, 7, 30, 200]), rnd.choice("MMMM=XIDNSHP")) for _ in range(rnd.randrange(0, 7)))
        pos0 = rnd.randrange(0, len(ref) + 20)
        r = rec(contigs, c, pos0, cigar)
        seq, at, ri = list(r[3]), pos0, 0
        for k, op in CM.cigar_ops(cigar):
            if op in "M=X":
                for j in range(k):
                    p = at + j
                    x = rnd.random()
                    if p in plant[c] and x < 0.9:
                        seq[ri + j] = plant[c][p]
                    elif x > 0.97:
                        seq[ri + j] = rnd.choice("ACGTNa")
                at += k
                ri += k
            elif op in "DN":
                at += k
            elif op in "IS":
                ri += k
        qual = "".join(chr(33 + rnd.choice([2, 14, 15, 15, 16, 30, 40, 40, 40])) for _ in seq)
        out.append((c, pos0, cigar, "".join(seq), None if rnd.random() < 0.125 else qual))   # (one in eight has no quality string)
    return out


# ---- the unit cases both test files run: name -> (contigs, records, N, F, Q) ----------------------------------------------------------
def _cases():
    import random
    rnd = random.Random(4711)
    one = [("chr1", _genome(rnd, 200))]
    two = [("chrA", _genome(rnd, 100)), ("chrB", _genome(rnd, 50))]
    # contigs of 7, 64, 1, 8 and 9 bases: the 64-base one starts at base 7 of the packed reference, the others at 71, 72 and 80
    packed = [("p7", _genome(rnd, 7)), ("p64", _genome(rnd, 64)), ("p1", _genome(rnd, 1)), ("p8", _genome(rnd, 8)), ("p9", _genome(rnd, 9))]
    # reference bases that are excluded or folded: N at 5, IUPAC R at 6, lower case at 8..11
    odd_seq = list(_genome(rnd, 40))
    odd_seq[5], odd_seq[6] = "N", "R"
    odd_seq[8:12] = [x.lower() for x in odd_seq[8:12]]
    odd = [("odd", "".join(odd_seq))]
    U = {}
    U["nothing"] = (two, [], 10, "0.8", 15)
    U["no-call-without-a-mismatch"] = (one, [rec(one, 0, 10, "50M")] * 12, 10, "0.8", 15)
    U["packed-reference"] = (packed, [rec(packed, 0, 0, "7M", [0, 6]), rec(packed, 1, 0, "64M", [0, 1, 7, 8, 9, 63]), rec(packed, 2, 0, "1M", [0]), rec(packed, 3, 0, "8M", [0, 7]),
                                      rec(packed, 4, 0, "9M", [0, 7, 8]), rec(packed, 1, 57, "7M", [0, 6])], 1, "0.5", 15)
    U["first-and-last-column"] = (one, [rec(one, 0, 20, "10M", [0, 9])], 1, "0.8", 15)
    U["contig-last-base"] = (one, [rec(one, 0, 190, "10M", [9])], 1, "0.8", 15)
    U["clipped-at-the-end"] = (one, [rec(one, 0, 195, "10M", [3, 4, 5, 7]), rec(one, 0, 199, "3S20M", [3, 4]), rec(one, 0, 200, "5M", [0]), rec(one, 0, 2000, "5M", [1])], 1, "0.5", 15)
    U["operations-in-front"] = (one, [rec(one, 0, 10, "3M2I5M", [6]), rec(one, 0, 30, "3M2D5M", [4]), rec(one, 0, 50, "3M10N5M", [5]), rec(one, 0, 80, "4S6M", [1, 4]),
                                      rec(one, 0, 100, "4H6M", [0]), rec(one, 0, 120, "4=1X4=", [4]), rec(one, 0, 140, "5M2P5M", [6]), rec(one, 0, 160, "2S3M1I2M1D4M3S", [2, 7, 9, 12])], 1, "0.8", 15)
    U["excluded-bases"] = (odd, [rec(odd, 0, 0, "40M", [(3, "N"), (4, "a"), 5, 6, 8, (9, other(odd_seq[9], 2)), 20]), rec(odd, 0, 2, "20M", [(1, "N"), 6, (7, "N")])], 1, "0.5", 15)
    U["quality-threshold"] = (one, [rec(one, 0, 10, "20M", [5, 6], qual=15), rec(one, 0, 10, "20M", [5, 6], qual=15, low=[5]), rec(one, 0, 10, "20M", [5]), rec(one, 0, 12, "20M", [4], qual=14)], 1, "0.5", 15)
    U["quality-zero-counts-everything"] = (one, [rec(one, 0, 10, "20M", [5], qual=0), rec(one, 0, 10, "20M", [6], qual=93)], 1, "0.5", 0)
    U["depth-n-and-n-minus-1"] = (one, [rec(one, 0, 10, "10M", [2])] * 3 + [rec(one, 0, 40, "10M", [2])] * 2, 3, "0.8", 15)
    U["min-cov-zero-is-one"] = (one, [rec(one, 0, 10, "10M", [2])], 0, "1", 15)
    U["fraction-4-of-5-and-3-of-5"] = (one, [rec(one, 0, 10, "10M", [2])] * 4 + [rec(one, 0, 10, "10M")] + [rec(one, 0, 40, "10M", [2])] * 3 + [rec(one, 0, 40, "10M")] * 2, 1, "0.8", 15)
    U["fraction-8-of-10-and-7-of-10"] = (one, [rec(one, 0, 10, "10M", [2])] * 8 + [rec(one, 0, 10, "10M")] * 2 + [rec(one, 0, 40, "10M", [2])] * 7 + [rec(one, 0, 40, "10M")] * 3, 10, "0.8", 15)
    U["fraction-one"] = (one, [rec(one, 0, 10, "10M", [2])] * 10 + [rec(one, 0, 40, "10M", [2])] * 9 + [rec(one, 0, 40, "10M")], 10, "1.0", 15)
    r10, r40 = one[0][1][10], one[0][1][40]
    U["two-way-tie"] = (one, [rec(one, 0, 10, "5M", [(0, other(r10, 3))])] * 2 + [rec(one, 0, 10, "5M", [(0, other(r10, 1))])] * 2 +
                        [rec(one, 0, 40, "5M", [(0, other(r40, 2))])] * 3 + [rec(one, 0, 40, "5M", [(0, other(r40, 3))])] * 3, 1, "0.5", 15)
    U["three-alternatives"] = (one, [rec(one, 0, 10, "5M", [(0, other(r10, 1))])] + [rec(one, 0, 10, "5M", [(0, other(r10, 2))])] * 3 + [rec(one, 0, 10, "5M", [(0, other(r10, 3))])] * 2, 1, "0.5", 15)
    U["contention"] = (one, [rec(one, 0, 100, "20M", [0, 7, 19])] * 3000 + [rec(one, 0, 100, "20M", [(7, other(one[0][1][107], 2))])] * 500, 10, "0.8", 15)
    U["padding-and-empty"] = (one, [rec(one, 0, 10, "5M2P5M", [9]), rec(one, 0, 40, ""), rec(one, 0, 50, "0M"), rec(one, 0, 60, "10S", [3])], 1, "0.8", 15)
    U["second-contig"] = (two, [rec(two, 0, 95, "10M", [4, 5]), rec(two, 1, 0, "10M", [0]), rec(two, 1, 45, "5M", [4])], 1, "0.8", 15)
    # with scan_chunk = 64 (array offsets = positions on the first contig)
    c300 = [("c", _genome(rnd, 300))]
    mid = [("c", _genome(rnd, 40)), ("d", _genome(rnd, 100)), ("e", _genome(rnd, 23))]   # d begins at slot 41, e at slot 142 (= 2 * 64 + 14)
    K = {}
    K["first-and-last-slot-of-a-chunk"] = (c300, [rec(c300, 0, 0, "5M", [0]), rec(c300, 0, 60, "10M", [3, 4]), rec(c300, 0, 120, "16M", [7, 8]), rec(c300, 0, 250, "50M", [5, 6, 49])], 1, "0.8", 15)
    K["depth-across-three-chunks"] = (c300, [rec(c300, 0, 60, "140M", [3, 4, 70, 90, 132, 139])] * 2 + [rec(c300, 0, 100, "100M", [30])], 2, "0.6", 15)
    K["contig-begins-in-mid-chunk"] = (mid, [rec(mid, 0, 30, "10M", [9]), rec(mid, 1, 0, "100M", [0, 22, 23, 99]), rec(mid, 2, 0, "23M", [0, 22])], 1, "0.8", 15)
    return U, K


UNIT_CASES, CHUNK_CASES = _cases()
RANDOM_CONTIGS_LENGTHS = (1, 64, 1000)


def random_case(seed, n):
    """(contigs, records, N, F, Q) over contigs of 1, 64 and 1 000 bases (some of the reference N, IUPAC and lower case)"""
    import random
    rnd = random.Random(seed)
    contigs = [(name, "".join(rnd.choice("ACGT" * 12 + "NRacgt") for _ in range(length))) for name, length in zip(("one", "sixtyfour", "thousand"), RANDOM_CONTIGS_LENGTHS)]
    return contigs, random_records(rnd, contigs, n), 10, "0.5", 15
