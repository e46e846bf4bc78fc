"""The definition of `ngm-hip --bs-mapping --methyl`'s file in plain Python, written from INTEGRATION.md ("--methyl") and not from
csrc/methyl.h: the oracle of tests/test_methyl_host.py and tests/test_gpu_methyl.py.  Written for clarity, not for speed.

The records that count are --coverage's (flag bits 0x4 and 0x100 clear).  A record is top when the first character of its ZS:Z tag is '+'
and bottom when it is '-'.  A record walks its CIGAR over its sequence as the SAM record prints it: S and I consume read bases, H, P, D and
N none.  A column is an M, = or X at contig position p inside the contig with read base b; it counts only if the record has no quality
string or the column's Phred quality is at least Q.  A top record over a reference C (case folded) adds 1 to meth[p] when b is C and 1 to
unmeth[p] when b is T; a bottom record over a reference G adds 1 to meth[p] when b is G and 1 to unmeth[p] when b is A.  Anything else
adds nothing.

A site is a reference C (strand +) or G (strand -).  For a C, n1 = ref[p + 1] and n2 = ref[p + 2]; for a G, n1 = complement(ref[p - 1])
and n2 = complement(ref[p - 2]); a neighbour outside the same contig, or not one of ACGT, is N.  n1 == G: CG; n1 == N: CN; otherwise
n2 == G: CHG, n2 == N: CHN, else CHH.  The file has one line per site with meth + unmeth >= max(1, N) whose context is selected, in
reference order: name, p + 1, strand, meth, unmeth, context, C n1 n2.  The totals: alignments, lines, then meth and unmeth summed over all
sites of context CG, CHG and CHH, whatever is selected.

A record is (contig index, 0-based position, CIGAR, sequence, qualities or None, bottom); contigs are [(name, sequence)]."""
import struct

import coverage_model as CM

DEFAULT_Q = 5
DEFAULT_N = 1
STATS = ("alignments", "lines", "cpg_meth", "cpg_unmeth", "chg_meth", "chg_unmeth", "chh_meth", "chh_unmeth")
SELECTS = {"all": ("CG", "CHG", "CHH", "CN", "CHN"), "CpG": ("CG",), "CHG": ("CHG",), "CHH": ("CHH",)}
COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A"}


def _s(x):
    return x.decode() if isinstance(x, bytes) else x


def tally(contigs, records, Q=DEFAULT_Q):
    """-> (meth, unmeth): one list of counts per contig"""
    refs = [_s(s).upper() for _, s in contigs]
    meth = [[0] * len(r) for r in refs]
    unmeth = [[0] * len(r) for r in refs]
    for c, pos0, cigar, seq, qual, bottom in records:
        ref, seq = refs[c], _s(seq)
        qual = None if qual is None else _s(qual)
        site, kept, converted = ("G", "G", "A") if bottom else ("C", "C", "T")
        at, ri = pos0, 0
        for n, op in CM.cigar_ops(cigar):
            if op in "M=X":
                for k in range(n):
                    p, b = at + k, seq[ri + k]
                    if not 0 <= p < len(ref) or ref[p] != site:
                        continue
                    if qual is not None and ord(qual[ri + k]) - 33 < Q:
                        continue
                    if b == kept:
                        meth[c][p] += 1
                    elif b == converted:
                        unmeth[c][p] += 1
                at += n
                ri += n
            elif op in "DN":
                at += n
            elif op in "IS":
                ri += n
        assert ri == len(seq) and (qual is None or len(qual) == len(seq)), (cigar, len(seq))
    return meth, unmeth


def context_of(ref, p):
    """the site at p of the (upper-case) contig ref: (strand, context, the three letters), or None when ref[p] is neither C nor G"""
    def letter(q, complement):
        if not 0 <= q < len(ref) or ref[q] not in "ACGT":
            return "N"
        return COMPLEMENT[ref[q]] if complement else ref[q]
    if ref[p] == "C":
        strand, n1, n2 = "+", letter(p + 1, False), letter(p + 2, False)
    elif ref[p] == "G":
        strand, n1, n2 = "-", letter(p - 1, True), letter(p - 2, True)
    else:
        return None
    if n1 == "G":
        context = "CG"
    elif n1 == "N":
        context = "CN"
    elif n2 == "G":
        context = "CHG"
    elif n2 == "N":
        context = "CHN"
    else:
        context = "CHH"
    return strand, context, "C" + n1 + n2


def report(contigs, records, Q=DEFAULT_Q, N=DEFAULT_N, context="all"):
    """-> (the file's bytes, the eight totals)"""
    meth, unmeth = tally(contigs, records, Q)
    selected = SELECTS[context]
    lines = []
    sums = {"CG": [0, 0], "CHG": [0, 0], "CHH": [0, 0]}
    for c, (name, s) in enumerate(contigs):
        ref = _s(s).upper()
        for p in range(len(ref)):
            site = context_of(ref, p)
            if site is None:
                continue
            strand, ctx, tri = site
            m, u = meth[c][p], unmeth[c][p]
            if ctx in sums:
                sums[ctx][0] += m
                sums[ctx][1] += u
            if m + u >= max(1, N) and ctx in selected:
                lines.append("%s\t%d\t%s\t%d\t%d\t%s\t%s\n" % (_s(name), p + 1, strand, m, u, ctx, tri))
    totals = [len(records), len(lines)] + sums["CG"] + sums["CHG"] + sums["CHH"]
    return "".join(lines).encode(), dict(zip(STATS, totals))


def parse_report(text):
    """[(name, position (1-based), strand, meth, unmeth, context, three letters)]"""
    return [(f[0], int(f[1]), f[2], int(f[3]), int(f[4]), f[5], f[6]) for f in (l.split("\t") for l in _s(text).splitlines())]


# ---- readers: the records that count (flag bits 0x4 and 0x100 clear) of the file a run wrote, the strand from ZS's first character ------
def records_of_sam(lines, contigs):
    index = {_s(n): i for i, (n, _) in enumerate(contigs)}
    out = []
    for line in lines:
        if line.startswith("@"):
            continue
        f = line.rstrip("\n").split("\t")
        if int(f[1]) & 0x104:
            continue
        zs = [t for t in f[11:] if t.startswith("ZS:Z:")]
        assert len(zs) == 1 and zs[0][5] in "+-", line
        out.append((index[f[2]], int(f[3]) - 1, f[5], f[9], None if f[10] == "*" else f[10], zs[0][5] == "-"))
    return out


def bam_tags(raw):
    """{tag: value} of a BAM record's tag bytes (the types the writer uses: A c C s S i I f Z)"""
    sizes = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
    out, at = {}, 0
    while at < len(raw):
        tag, kind = raw[at:at + 2].decode(), chr(raw[at + 2])
        at += 3
        if kind == "Z":
            end = raw.index(b"\0", at)
            out[tag] = raw[at:end].decode()
            at = end + 1
        else:
            fmt = {"A": "<c", "c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I", "f": "<f"}[kind]
            out[tag] = struct.unpack_from(fmt, raw, at)[0]
            at += sizes[kind]
    return out


def records_of_bam(recs):
    """... of the records tests/test_gpu_bam.decode_bam returns"""
    import snp_model
    kept = [r for r in recs if not r["flag"] & 0x104]
    out = []
    for five, r in zip(snp_model.records_of_bam(kept), kept):
        zs = bam_tags(r["tags"])["ZS"]
        assert zs[0] in "+-"
        out.append(five + (zs[0] == "-",))
    return out


def read_fasta(path):
    import snp_model
    return snp_model.read_fasta(path)


def from_run(out_path, fasta_path, Q=DEFAULT_Q, N=DEFAULT_N, context="all"):
    """(the file, the totals) the model gives over what a run wrote: its SAM or BAM file and the FASTA"""
    contigs = read_fasta(fasta_path)
    if out_path.endswith(".bam"):
        from test_gpu_bam import decode_bam
        records = records_of_bam(decode_bam(out_path)[2])
    else:
        records = records_of_sam(open(out_path).readlines(), contigs)
    return report(contigs, records, Q, N, context)


# ---- building records ---------------------------------------------------------------------------------------------------------------
def rec(contigs, c, pos0, cigar, bottom=False, meth="all", subs=None, qual=None, low=()):
    """a record whose aligned columns repeat the (upper-cased) reference ('A' past the contig's end and for inserted and clipped bases),
    bisulfite-converted on its strand: a top record reads a reference C as T, a bottom record a reference G as A, except at the contig
    positions of meth ("all": everywhere).  subs: {contig position: base}; qual: None, or a Phred value for every base, with the columns
    at the contig positions of `low` one below it."""
    ref = _s(contigs[c][1]).upper()
    site, converted = ("G", "A") if bottom else ("C", "T")
    seq, at, where = [], pos0, {}
    for n, op in CM.cigar_ops(cigar):
        if op in "M=X":
            for p in range(at, at + n):
                where[p] = len(seq)
                base = ref[p] if 0 <= p < len(ref) else "A"
                if base == site and not (meth == "all" or p in meth):
                    base = converted
                seq.append((subs or {}).get(p, base))
            at += n
        elif op in "DN":
            at += n
        elif op in "IS":
            seq += ["A"] * n
    if isinstance(qual, int):
        lows = {where[p] for p in low}
        qual = "".join(chr(33 + qual - (1 if i in lows else 0)) for i in range(len(seq)))
    return (c, pos0, cigar, "".join(seq), qual, bool(bottom))


def _cases():
    """name -> (contigs, records, dict(Q=, N=, context=, scan_chunk=)): the smallest shapes at which the kernels can go wrong"""
    P = lambda **kw: dict(dict(Q=DEFAULT_Q, N=DEFAULT_N, context="all", scan_chunk=0), **kw)
    U = {}
    #             0         1         2         3         4
    #             01234567890123456789012345678901234567890123456789
    G1 = [("g1", "ATCGATTCAGTTACCTGAGGATCCATGCAAGCTTCAGGCTAACGTTAGCA")]
    U["top-and-bottom-over-the-same-c-and-g"] = (G1, [rec(G1, 0, 0, "50M", False, meth={2, 13}), rec(G1, 0, 0, "50M", True, meth={3, 16}),
                                                     rec(G1, 0, 5, "30M", False, meth=()), rec(G1, 0, 5, "30M", True, meth="all")], P())
    # a top record's G>A and a bottom record's C>T, and other letters over a site: nothing
    U["ignored-bases"] = (G1, [rec(G1, 0, 0, "50M", False, subs={3: "A", 9: "A", 2: "G", 7: "N", 13: "c"}), rec(G1, 0, 0, "50M", True, subs={2: "T", 7: "T", 3: "C", 9: "N", 16: "g"})], P())
    # c0 ends in C (and has a C second to last in front of it: its n2 lies outside), c1 begins with G; c2 begins with GG and ends in ...CA, ...C?
    SEAM = [("c0", "ATTAGCATTACC"), ("c1", "GGATTACAGTC"), ("c2", "GATCAGATTTCA"), ("c3", "CG")]
    U["contig-seam"] = (SEAM, [rec(SEAM, c, 0, "%dM" % len(s), b, meth={1, 3, 10, 11}) for c, (_, s) in enumerate(SEAM) for b in (False, True)], P())
    NN = [("low", "acgtnCGncggcNNGcatCRGtgcNcGtcaNatRgaNaG"), ("n-only", "NNNNNNNNNNNN")]
    U["n-neighbour-and-lower-case"] = (NN, [rec(NN, 0, 0, "39M", False, meth={1, 8, 28}), rec(NN, 0, 0, "39M", True), rec(NN, 1, 0, "12M", False), rec(NN, 0, 3, "20M", True, meth=())], P())
    #             0         1         2         3         4         5         6
    #             0123456789012345678901234567890123456789012345678901234567890123456789
    G2 = [("g2", "ACGTCCGGATCGATTACGCGCATGCCGTAGCTAGCCGGATATCGCGATCGGCTAGCTTAGGCTCAGCATG")]
    U["cigar-with-insert-deletion-and-soft-clips"] = (G2, [rec(G2, 0, 7, "5S10M3I10M2D10M4S", False, meth={10, 17, 33}), rec(G2, 0, 7, "5S10M3I10M2D10M4S", True, meth={8, 18, 35}, qual=30),
                                                           rec(G2, 0, 0, "2M1I3M1D4M2N5M1P6M", False, meth=())], P())
    U["hard-clips"] = (G2, [rec(G2, 0, 12, "4H20M6H", False, meth={17, 19}), rec(G2, 0, 12, "4H3S20M2S6H", True, meth={16}, qual=20)], P())
    U["hanging-over-the-contigs-end"] = (G2, [rec(G2, 0, 60, "20M", False), rec(G2, 0, 65, "3S30M", True, qual=40), rec(G2, 0, 69, "1M", True), rec(G2, 0, 70, "5M", False), rec(G2, 0, 90, "5M", True)], P())
    cs = [p for p in range(10, 40) if G2[0][1][p] == "C"]
    U["quality-at-q-and-one-below"] = (G2, [rec(G2, 0, 10, "30M", False, qual=5, low=cs[:2]), rec(G2, 0, 10, "30M", False, meth=(), qual=6, low=cs[1:4]), rec(G2, 0, 10, "30M", False, qual=4),
                                            rec(G2, 0, 10, "30M", True, qual=13, low=[p for p in range(10, 40) if G2[0][1][p] == "G"][:3])], P(Q=5))
    U["quality-threshold-13"] = (G2, U["quality-at-q-and-one-below"][1], P(Q=13))
    U["no-quality-string"] = (G2, [rec(G2, 0, 10, "30M", False), rec(G2, 0, 20, "30M", True, meth=())], P(Q=93))
    U["min-depth-3"] = (G2, [rec(G2, 0, 0, "40M", False), rec(G2, 0, 20, "40M", False, meth=()), rec(G2, 0, 30, "40M", False), rec(G2, 0, 0, "30M", True), rec(G2, 0, 10, "30M", True, meth=()),
                             rec(G2, 0, 25, "30M", True)], P(N=3))
    U["min-depth-0-is-1"] = (G2, U["min-depth-3"][1], P(N=0))
    # all five contexts on both strands: CG, CHG (CAG / CTG), CHH, CN (C in front of N, G behind N) and CHN
    ALL5 = [("five", "TCGATCAGTTCTAACNTTGNATCANGTTNAGCTCC"), ("more", "GGAACTGCGCNG")]
    both = [rec(ALL5, c, 0, "%dM" % len(s), b, meth={1, 5, 7, 9, 14, 18, 22, 25, 30, 33} if k else ()) for c, (_, s) in enumerate(ALL5) for b in (False, True) for k in (0, 1, 1)]
    for name in SELECTS:
        U["context-" + name] = (ALL5, both, P(context=name))
    # 8 bases per dword of the packed reference: sites at p = 7, 8, 15, 16, 23, 24 and their neighbours in the next / previous dword
    #              0       8       16      24      32
    BORDER = [("w", "ATATATACGATATACCGTATATAGCATATATATGCATATA"), ("x", "AAAAAAACGAAAAAA")]
    U["packed-word-border"] = (BORDER, [rec(BORDER, 0, 0, "40M", b, meth={7, 8, 15, 23} if k else ()) for b in (False, True) for k in (0, 1)] +
                               [rec(BORDER, 1, 0, "15M", b, meth=() if b else "all") for b in (False, True)], P())
    import random
    rnd = random.Random(64)
    LONG = [("l", "".join(rnd.choice("ACGT") for _ in range(150))), ("m", "".join(rnd.choice("ACGTN") for _ in range(70)))]
    U["scan-chunk-64"] = (LONG, [rec(LONG, c, p, "35M", (p // 5) % 2 == 1, meth=set(range(0, 150, 3))) for c, n in ((0, 150), (1, 70)) for p in range(0, n - 20, 5)], P(scan_chunk=64))
    return U


UNIT_CASES = _cases()


def random_case(seed, n):
    """(contigs, records, parameters) over contigs of 30, 333 and 1 000 bases: random CIGARs (coverage's random shapes), records of both
    strands, half of the C (top) or G (bottom) columns converted, 2 % other substitutions and read Ns, qualities around Q = 5"""
    import random
    rnd = random.Random(seed)
    contigs = [(name, "".join(rnd.choice("ACGT" * 12 + "NRacgt") for _ in range(length))) for name, length in zip(("thirty", "mid", "thousand"), (30, 333, 1000))]
    records = []
    for _ in range(n):
        c = rnd.randrange(3)
        ref = contigs[c][1].upper()
        bottom = rnd.random() < 0.5
        site, converted = ("G", "A") if bottom else ("C", "T")
        cigar = "".join("%d%s" % (rnd.choice([0, 1, 1, 2, 3, 7, 30, 200]), rnd.choice("MMMM=XIDNSHP")) for _ in range(rnd.randrange(0, 7)))
        pos0 = rnd.randrange(0, len(ref) + 20)
        seq, at = [], pos0
        for k, op in CM.cigar_ops(cigar):
            if op in "M=X":
                for p in range(at, at + k):
                    base = ref[p] if p < len(ref) else "A"
                    x = rnd.random()
                    if base == site and x < 0.5:
                        base = converted
                    elif x > 0.98:
                        base = rnd.choice("ACGTNa")
                    seq.append(base)
                at += k
            elif op in "DN":
                at += k
            elif op in "IS":
                seq += [rnd.choice("ACGT") for _ in range(k)]
        qual = "".join(chr(33 + rnd.choice([0, 4, 5, 5, 6, 20, 40, 40, 40])) for _ in seq)
        records.append((c, pos0, cigar, "".join(seq), None if rnd.random() < 0.125 else qual, bottom))
    return contigs, records, dict(Q=DEFAULT_Q, N=DEFAULT_N, context="all", scan_chunk=0)
