"""The definition of `ngm-hip --count`'s file in plain Python / numpy, written from INTEGRATION.md ("--count") and not from csrc/count.h:
the oracle of tests/test_count_host.py and tests/test_gpu_count.py.  Written for clarity, not for speed: every region looks at every
record.

The records that count are --coverage's and --snp's (flag bits 0x4 and 0x100 clear); a record is forward when bit 0x10 is clear, reverse
when it is set.  A record walks its CIGAR over its sequence as the SAM record prints it.  An M / = / X column at contig position p with read
base b is eligible when p is inside the contig, the case-folded reference base is T (forward record) or A (reverse record), b is one of
ACGT, and the record has no quality string or the column's Phred quality is at least Q.  An eligible column adds 1 to cov[p], and 1 to
conv[p] when b is C (forward) or G (reverse).  A region of strand + takes forward records, - reverse records, . both: reads counts the
records it takes with an M / = / X column inside [start, end), tc_reads those of them with an eligible column inside the region that is a
conversion (the mask is not looked at).  At the finish a region sums cov and conv over its positions whose reference base is T (+), A (-)
or either (.) and that are not in the mask: t_bases counts those positions, masked the ones the mask took away.

A record is (contig index, 0-based position, CIGAR, sequence, qualities or None, reverse); contigs are [(name, sequence)]; a region is
(contig index, start, end, name, strand); the mask is a set of (contig index, position)."""
import re

import numpy as np

import coverage_model as CM

HEADER = "#chrom\tstart\tend\tname\tstrand\tt_bases\tmasked\tcov_on_ts\tconv_on_ts\treads\ttc_reads\n"
DEFAULT_Q = 27
STATS = ("alignments", "met_a_region", "eligible_columns", "conversions", "masked_positions")


def _s(x):
    return x.decode() if isinstance(x, bytes) else x


# ---- the BED file -------------------------------------------------------------------------------------------------------------------
class BedError(ValueError):
    """str(): 'line <n>: <reason>'"""


_NUMBER = re.compile(r"[0-9]{1,10}")


def _number(text):
    return int(text) if _NUMBER.fullmatch(text) and int(text) <= 0xFFFFFFFF else None


def parse_bed(text, contigs):
    """the regions of a BED text, in its order; raises BedError for the first line that is refused"""
    names = [_s(n) for n, _ in contigs]
    out = []
    for no, line in enumerate(_s(text).split("\n"), 1):
        if line.endswith("\r"):
            line = line[:-1]
        if not line or line.startswith(("#", "track", "browser")):
            continue
        f = line.split("\t")
        if len(f) < 3:
            raise BedError("line %d: it has fewer than 3 tab-separated columns" % no)
        if f[0] not in names:
            raise BedError("line %d: contig %s is not in the reference" % (no, f[0]))
        c = names.index(f[0])
        start, end = _number(f[1]), _number(f[2])
        if start is None:
            raise BedError("line %d: its start %s is not a number" % (no, f[1]))
        if end is None:
            raise BedError("line %d: its end %s is not a number" % (no, f[2]))
        if start >= end:
            raise BedError("line %d: its start is not in front of its end" % no)
        if end > len(contigs[c][1]):
            raise BedError("line %d: its end lies behind the contig's last base (%d bases)" % (no, len(contigs[c][1])))
        strand = f[5] if len(f) > 5 else "."
        if strand not in ("+", "-", "."):
            raise BedError("line %d: its strand %s is not +, - or ." % (no, strand))
        out.append((c, start, end, f[3] if len(f) > 3 else ".", strand))
    if not out:
        raise BedError("line 0: the file has no region")
    return out


def bed_text(contigs, regions):
    return "".join("%s\t%d\t%d\t%s\t0\t%s\n" % (_s(contigs[c][0]), s, e, name, strand) for c, s, e, name, strand in regions)


# ---- the count ----------------------------------------------------------------------------------------------------------------------
def columns(refs, record, Q):
    """-> (the aligned segments [(begin, end)] inside the contig, the positions of the eligible columns, those of the conversions)"""
    c, pos0, cigar, seq, qual, reverse = record
    ref = refs[c]
    seq = np.frombuffer(_s(seq).encode(), dtype=np.uint8)
    q = None if qual is None else np.frombuffer(_s(qual).encode(), dtype=np.uint8).astype(np.int64) - 33
    want, to = (ord("A"), ord("G")) if reverse else (ord("T"), ord("C"))
    segments, eligible, conversions = [], [], []
    at, ri = pos0, 0
    for n, op in CM.cigar_ops(cigar):
        if op in "M=X":
            b, e = max(at, 0), min(at + n, len(ref))
            if b < e:
                segments.append((b, e))
                bases = seq[ri + b - at:ri + e - at]
                ok = (ref[b:e] == want) & np.isin(bases, np.frombuffer(b"ACGT", dtype=np.uint8))
                if q is not None:
                    ok &= q[ri + b - at:ri + e - at] >= Q
                eligible.append(b + np.flatnonzero(ok))
                conversions.append(b + np.flatnonzero(ok & (bases == to)))
            at += n
            ri += n
        elif op in "DN":
            at += n
        elif op in "IS":
            ri += n
    assert ri == len(seq) and (q is None or len(q) == len(seq)), (cigar, len(seq))
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
    return segments, cat(eligible), cat(conversions)


def tally(contigs, records, regions, mask=(), Q=DEFAULT_Q):
    """-> ([(t_bases, masked, cov_on_ts, conv_on_ts, reads, tc_reads)] per region, the statistics ngm_count_stats reports)"""
    refs = [np.frombuffer(_s(s).upper().encode(), dtype=np.uint8) for _, s in contigs]
    cov = [np.zeros(len(r), dtype=np.int64) for r in refs]
    conv = [np.zeros(len(r), dtype=np.int64) for r in refs]
    union = [np.zeros(len(r), dtype=bool) for r in refs]
    for c, s, e, _, _ in regions:
        union[c][s:e] = True
    reads, tc_reads = [0] * len(regions), [0] * len(regions)
    met = n_eligible = n_conv = 0
    for record in records:
        c, reverse = record[0], bool(record[5])
        segments, eligible, conversions = columns(refs, record, Q)
        cov[c][eligible] += 1   # (a record has one column per position at most)
        conv[c][conversions] += 1
        n_eligible += int(union[c][eligible].sum())
        n_conv += int(union[c][conversions].sum())
        taken = False
        for R, (rc, s, e, _, strand) in enumerate(regions):
            if rc != c or (strand == "+" and reverse) or (strand == "-" and not reverse):
                continue
            if not any(max(b, s) < min(x, e) for b, x in segments):
                continue
            taken = True
            reads[R] += 1
            if ((conversions >= s) & (conversions < e)).any():
                tc_reads[R] += 1
        met += taken
    mask = set(mask)
    rows = []
    for R, (c, s, e, _, strand) in enumerate(regions):
        letters = {"+": "T", "-": "A", ".": "TA"}[strand]
        t_bases = masked = cov_on_ts = conv_on_ts = 0
        for p in range(s, e):
            if chr(refs[c][p]) not in letters:
                continue
            if (c, p) in mask:
                masked += 1
                continue
            t_bases += 1
            cov_on_ts += int(cov[c][p])
            conv_on_ts += int(conv[c][p])
        rows.append((t_bases, masked, cov_on_ts, conv_on_ts, reads[R], tc_reads[R]))
    hit = sum(1 for c, p in mask if 0 <= c < len(refs) and 0 <= p < len(refs[c]) and union[c][p])
    return rows, dict(zip(STATS, (len(records), met, n_eligible, n_conv, hit)))


def tsv(contigs, regions, rows):
    return (HEADER + "".join("%s\t%d\t%d\t%s\t%s\t%s\n" % (_s(contigs[c][0]), s, e, name, strand, "\t".join(str(x) for x in row))
                             for (c, s, e, name, strand), row in zip(regions, rows))).encode()


def count_file(contigs, records, regions, mask=(), Q=DEFAULT_Q):
    return tsv(contigs, regions, tally(contigs, records, regions, mask, Q)[0])


def parse_tsv(text):
    """[(chrom, start, end, name, strand, t_bases, masked, cov_on_ts, conv_on_ts, reads, tc_reads)]"""
    lines = _s(text).splitlines()
    assert lines[0] + "\n" == HEADER
    return [tuple(f[:1] + [int(f[1]), int(f[2])] + f[3:5] + [int(x) for x in f[5:]]) for f in (l.split("\t") for l in lines[1:])]


# ---- readers: the records that count (flag bits 0x4 and 0x100 clear) of the file a run wrote, and the mask of its VCF -----------------
def records_of_sam(lines, contigs):
    index = {_s(n): i for i, (n, _) in enumerate(contigs)}
    out = []
    for line in lines:
        if line.startswith("@"):
            continue
        f = line.rstrip("\n").split("\t")
        if int(f[1]) & 0x104:
            continue
        out.append((index[f[2]], int(f[3]) - 1, f[5], f[9], None if f[10] == "*" else f[10], bool(int(f[1]) & 0x10)))
    return out


def records_of_bam(recs):
    """... of the records tests/test_gpu_bam.decode_bam returns"""
    import snp_model
    kept = [r for r in recs if not r["flag"] & 0x104]
    return [five + (bool(r["flag"] & 0x10),) for five, r in zip(snp_model.records_of_bam(kept), kept)]


def mask_of_vcf(text, contigs):
    index = {_s(n): i for i, (n, _) in enumerate(contigs)}
    return {(index[f[0]], int(f[1]) - 1) for f in (l.split("\t") for l in _s(text).splitlines() if l and not l.startswith("#"))}


def read_fasta(path):
    import snp_model
    return snp_model.read_fasta(path)


def from_sam(out_path, fasta_path, bed_path, vcf_path=None, Q=DEFAULT_Q):
    """the file the model gives over what a run wrote: its SAM or BAM file, the FASTA, the BED file and (or None) its VCF"""
    contigs = read_fasta(fasta_path)
    if out_path.endswith(".bam"):
        from test_gpu_bam import decode_bam
        records = records_of_bam(decode_bam(out_path)[2])
    else:
        records = records_of_sam(open(out_path).readlines(), contigs)
    regions = parse_bed(open(bed_path).read(), contigs)
    mask = mask_of_vcf(open(vcf_path).read(), contigs) if vcf_path else set()
    return count_file(contigs, records, regions, mask, Q)


# ---- building records ---------------------------------------------------------------------------------------------------------------
def rec(contigs, c, pos0, cigar, reverse=False, conv=(), subs=None, qual=None, low=()):
    """a record whose aligned columns repeat the (upper-cased) reference ('A' past the contig's end and for inserted and clipped bases).
    conv: contig positions read as a conversion where the reference base allows one -- "all": every one; subs: {contig position: base};
    qual: None, or a Phred value for every base, with the columns at the contig positions of `low` one below it."""
    ref = _s(contigs[c][1]).upper()
    want, to = ("A", "G") if reverse else ("T", "C")
    seq, at, where = [], pos0, {}
    for n, op in CM.cigar_ops(cigar):
        if op in "M=X":
            for p in range(at, at + n):
                where[p] = len(seq)
                base = ref[p] if 0 <= p < len(ref) else "A"
                if base == want and (conv == "all" or p in conv):
                    base = to
                seq.append((subs or {}).get(p, base))
            at += n
        elif op in "DN":
            at += n
        elif op in "IS":
            seq += ["A"] * n
    if isinstance(qual, int):
        lows = {where[p] for p in low}
        qual = "".join(chr(33 + qual - (1 if i in lows else 0)) for i in range(len(seq)))
    return (c, pos0, cigar, "".join(seq), qual, bool(reverse))


def positions(contigs, c, letter, s, e):
    """the positions in [s, e) of contig c whose (case-folded) reference base is `letter`"""
    ref = _s(contigs[c][1]).upper()
    return [p for p in range(s, e) if ref[p] == letter]


def _genome(rnd, n):
    """random bases with a lower-case stretch and a stretch of N"""
    g = [rnd.choice("ACGT") for _ in range(n)]
    for p in range(n // 3, min(n, n // 3 + 25)):
        g[p] = g[p].lower()
    for p in range(n // 2, min(n, n // 2 + 6)):
        g[p] = "N"
    return "".join(g)


def _cases():
    import random
    rnd = random.Random(2718)
    # (301, 397 and 211 bases: the second and third contig begin in the middle of a dword of the packed reference)
    W = [("cA", _genome(rnd, 301)), ("cB", _genome(rnd, 397)), ("cC", _genome(rnd, 211))]
    T = lambda c, s, e: positions(W, c, "T", s, e)
    A = lambda c, s, e: positions(W, c, "A", s, e)
    U = {}
    U["crossing-start-and-end"] = (W, [rec(W, 0, 40, "20M", conv="all"), rec(W, 0, 90, "20M", conv="all"), rec(W, 0, 60, "20M", conv="all", qual=40)],
                                   [(0, 50, 100, "utr", "+")], set(), 27)
    U["clipped-at-the-contigs-last-base"] = (W, [rec(W, 0, 291, "20M", conv="all"), rec(W, 0, 300, "3S5M", conv="all"), rec(W, 2, 205, "10M", True, conv="all")],
                                             [(0, 270, 301, "end", "+"), (2, 200, 211, "endC", "-")], set(), 27)
    U["outside-every-region"] = (W, [rec(W, 0, 200, "30M", conv="all"), rec(W, 1, 55, "30M", conv="all"), rec(W, 0, 20, "30M", conv="all"), rec(W, 0, 60, "30M", conv="all")],
                                 [(0, 50, 60, "small", "+")], set(), 27)
    U["spanning-with-a-deletion-only"] = (W, [rec(W, 0, 90, "10M10D10M", conv="all"), rec(W, 0, 85, "15M10N15M", conv="all"), rec(W, 0, 95, "10M5D10M", conv="all")],
                                          [(0, 100, 110, "gap", "+")], set(), 27)
    U["operations-in-front-of-a-conversion"] = (W, [rec(W, 0, 10, "3M2I25M", conv=T(0, 20, 38)), rec(W, 0, 10, "4S26M", conv=T(0, 20, 36)), rec(W, 0, 10, "4H26M", conv=T(0, 20, 36)),
                                                    rec(W, 0, 5, "5M3D22M", conv=T(0, 20, 35)), rec(W, 0, 8, "2S3M1I4M2D10M1I8M3S", conv=T(0, 18, 35), qual=30)],
                                                [(0, 15, 40, "ops", "+")], set(), 27)
    t0 = T(0, 150, 180)
    U["quality-just-below-and-at-q"] = (W, [rec(W, 0, 150, "30M", conv="all", qual=27), rec(W, 0, 150, "30M", conv="all", qual=27, low=t0[:2]), rec(W, 0, 150, "30M", conv="all", qual=26),
                                            rec(W, 0, 150, "30M", conv="all", qual=28, low=t0[1:3])], [(0, 150, 180, "q", "+")], set(), 27)
    U["quality-zero-counts-everything"] = (W, [rec(W, 0, 150, "30M", conv="all", qual=0), rec(W, 0, 150, "30M", conv=t0[:1], qual=93)], [(0, 150, 180, "q0", "+")], set(), 0)
    U["read-n-on-a-t"] = (W, [rec(W, 0, 150, "30M", conv=t0[2:], subs={t0[0]: "N", t0[1]: "a"}), rec(W, 0, 150, "30M", subs={t0[0]: "G"})], [(0, 150, 180, "n", "+")], set(), 27)
    U["no-quality-string"] = (W, [rec(W, 0, 150, "30M", conv="all"), rec(W, 0, 160, "30M", True, conv="all")], [(0, 150, 180, "f", "+"), (0, 150, 180, "r", "-")], set(), 93)
    U["nested-and-repeated-regions"] = (W, [rec(W, 1, 40, "50M", conv="all"), rec(W, 1, 72, "6M", conv="all"), rec(W, 1, 100, "60M", conv="all", qual=35), rec(W, 1, 76, "2M", True, conv="all")],
                                        [(1, 50, 150, "outer", "+"), (1, 70, 90, "inner", "+"), (1, 75, 80, "innermost", "+"), (1, 70, 90, "inner", "+"), (1, 50, 150, "outer-", "-")], set(), 27)
    U["opposite-strands-and-a-dot-region"] = (W, [rec(W, 1, 40, "50M", conv="all"), rec(W, 1, 90, "50M", True, conv="all"), rec(W, 1, 95, "30M", conv="all"), rec(W, 1, 130, "50M", True, conv=A(1, 130, 150)),
                                                  rec(W, 1, 60, "50M", True)],
                                              [(1, 50, 120, "plus", "+"), (1, 100, 170, "minus", "-"), (1, 80, 140, "both", ".")], set(), 27)
    U["region-without-a-record-and-of-one-base"] = (W, [rec(W, 2, 20, "30M", conv="all")] * 3,
                                                    [(2, 100, 140, "empty", "+"), (2, T(2, 20, 50)[1], T(2, 20, 50)[1] + 1, "one-T", "+"), (2, A(2, 20, 50)[0], A(2, 20, 50)[0] + 1, "one-A", "+"),
                                                     (2, 0, 1, "first", "."), (2, 210, 211, "last", ".")], set(), 27)
    U["regions-of-70-and-300-bases"] = (W, [rec(W, 1, p, "40M", p % 3 == 0, conv="all", qual=30 if p % 2 else None) for p in range(0, 360, 7)],
                                        [(1, 13, 83, "seventy", "."), (1, 90, 390, "three-hundred", "+"), (1, 90, 390, "three-hundred-", "-")], set(), 27)
    # (the first region has 13 slots: the second one's first slot is 13, the third one's 13 + 21)
    U["slots-that-are-no-multiple-of-8"] = (W, [rec(W, 0, 0, "60M", conv="all"), rec(W, 0, 30, "60M", conv="all"), rec(W, 1, 0, "30M", True, conv="all"), rec(W, 2, 0, "30M", conv="all")],
                                            [(0, 3, 16, "a", "+"), (0, 41, 62, "b", "+"), (1, 5, 22, "c", "-"), (2, 1, 10, "d", "+")], set(), 27)
    t1 = T(1, 200, 260)
    U["contention"] = (W, [rec(W, 1, t1[0], "1M", conv="all")] * 600 + [rec(W, 1, t1[0], "1M")] * 100, [(1, 200, 260, "hot", "+"), (1, t1[0], t1[0] + 1, "hot-base", ".")], set(), 27)
    U["mask-inside-outside-and-on-the-border"] = (W, [rec(W, 0, 190, "80M", conv="all"), rec(W, 0, 210, "40M", conv="all"), rec(W, 0, 195, "50M", True, conv="all")],
                                                  [(0, 200, 250, "m+", "+"), (0, 200, 250, "m-", "-"), (0, 200, 250, "m.", "."), (0, 230, 270, "next", "+")],
                                                  {(0, 199), (0, 200), (0, 201), (0, 225), (0, 249), (0, 250), (0, 269), (0, 270), (1, 210), (2, 5)} | {(0, p) for p in T(0, 200, 250)[:3]}, 27)
    t2 = T(0, 60, 100)
    U["a-masked-t-leaves-t-bases"] = (W, [rec(W, 0, 60, "40M", conv=t2[:2])] * 5 + [rec(W, 0, 60, "40M")] * 2, [(0, 60, 100, "snp", "+")], {(0, t2[0])}, 27)
    return U


UNIT_CASES = _cases()


def random_case(seed, n):
    """(contigs, records, regions, mask, Q) over contigs of 30, 333 and 1 000 bases: random CIGARs (coverage's random shapes), a quarter of the
    T (forward) or A (reverse) columns converted, 2 % other substitutions and read Ns, qualities around 27, overlapping regions of all strands"""
    import random
    rnd = random.Random(seed)
    contigs = [(name, "".join(rnd.choice("ACGT" * 12 + "NRacgt") for _ in range(length))) for name, length in zip(("thirty", "mid", "thousand"), (30, 333, 1000))]
    regions = []
    for k in range(40):
        c = rnd.randrange(3)
        length = len(contigs[c][1])
        s = rnd.randrange(length)
        e = min(length, s + rnd.choice([1, 2, 9, 40, 64, 65, 200, 500]))
        regions.append((c, s, e, "r%d" % k, rnd.choice("+-.")))
    regions.append(regions[3])
    records = []
    for _ in range(n):
        c = rnd.randrange(3)
        ref = contigs[c][1].upper()
        reverse = rnd.random() < 0.5
        want, to = ("A", "G") if reverse else ("T", "C")
        cigar = "".join("%d%s" % (rnd.choice([0, 1, 1, 2, 3, 7, 30, 200]), rnd.choice("MMMM=XIDNSHP")) for _ in range(rnd.randrange(0, 7)))
        pos0 = rnd.randrange(0, len(ref) + 20)
        seq, at = [], pos0
        for k, op in CM.cigar_ops(cigar):
            if op in "M=X":
                for p in range(at, at + k):
                    base = ref[p] if p < len(ref) else "A"
                    x = rnd.random()
                    if base == want and x < 0.25:
                        base = to
                    elif x > 0.98:
                        base = rnd.choice("ACGTNa")
                    seq.append(base)
                at += k
            elif op in "DN":
                at += k
            elif op in "IS":
                seq += [rnd.choice("ACGT") for _ in range(k)]
        qual = "".join(chr(33 + rnd.choice([2, 26, 27, 27, 28, 30, 40, 40, 40])) for _ in seq)
        records.append((c, pos0, cigar, "".join(seq), None if rnd.random() < 0.125 else qual, reverse))
    mask = {(c, rnd.randrange(len(s))) for c, (_, s) in enumerate(contigs) for _ in range(len(s) // 10)}
    return contigs, records, regions, mask, 27
