"""Seeded --vcf fixtures (genome + VCF) for tests/test_gpu_vcf.py and tests/make_vcf_goldens.py.

F1: a two-contig repeat-rich genome with ~400 variant sites (SNPs, multi-allelic lines, insertions and deletions up to 10 bp, variants within
    13 bp of a contig end and of the genome end), and every kind of line the reference drops (src/parser/VcfParser.cpp).
F2: a 20 kbp contig with A x 300 at 5000-5299 and five A -> AAAA insertions inside it: the fill pass of the reference stores fewer
    entries than its count pass reserved (PrefixTable.cpp:360-374 against :411-422), so the poly-A list ends in a zero slot.
F3: F1's genome with an indel whose REF does not match the genome in the middle of the file: every later variant is dropped
    (PrefixTable.cpp:553-554)."""
import gzip
import os

import numpy as np

import simulate as S

BASES = np.frombuffer(b"ACGT", np.uint8)


def _write_fa(path, contigs, names):
    S.write_fasta(path, contigs, names=names)


def _f1_genome():
    return S.make_genome([60000, 40001], seed=71, repeat_families=6, repeat_len=300, copies=6, divergence=0.03)


def _f1_lines(contigs, rng, n_snps=400, mismatch_at=None):
    """VCF body lines of F1 (positions ascending per contig, as a VCF would have them)"""
    names = ["chr1", "chr2"]
    recs = []
    for _ in range(n_snps):
        c = int(rng.integers(0, 2))
        p = int(rng.integers(20, len(contigs[c]) - 20))
        recs.append((c, p))
    # near the contig ends (within 13 bp) and at the very end of the genome
    for c in (0, 1):
        for d in (1, 3, 7, 12):
            recs.append((c, d))
            recs.append((c, len(contigs[c]) - d + 1))
    recs.sort()
    lines = []
    for (c, p) in recs:
        g = contigs[c]
        refb = chr(g[p - 1])
        kind = int(rng.integers(0, 10))
        if kind <= 5 or p < 12 or p > len(g) - 12:
            alts = [chr(b) for b in BASES if chr(b) != refb]
            if kind == 0:
                alt = ",".join(rng.choice(alts, size=2, replace=False))   # multi-allelic
            elif kind == 1:
                alt = refb                                                 # ALT equals the genome: ignored
            else:
                alt = str(rng.choice(alts))
            if kind == 2:
                refb = "ACGT"[(("ACGT".index(refb) if refb in "ACGT" else 0) + 1) % 4]   # a SNP's REF is never checked
            lines.append("%s\t%d\t.\t%s\t%s\t50\tPASS\tDP=10" % (names[c], p, refb, alt))
        elif kind <= 7:
            n = int(rng.integers(1, 11))                                   # deletion of up to 10 bases
            ref = bytes(g[p - 1:p + n]).decode()
            lines.append("%s\t%d\trs%d\t%s\t%s\t50\tPASS\tDP=10" % (names[c], p, p, ref, ref[0]))
        else:
            n = int(rng.integers(1, 11))                                   # insertion of up to 10 bases
            ins = bytes(rng.choice(BASES, size=n)).decode()
            ref = chr(g[p - 1])
            alt = ref + ins
            if kind == 9:
                alt += "," + ref + ins[::-1]
            lines.append("%s\t%d\t.\t%s\t%s\t50\tPASS\tDP=10" % (names[c], p, ref, alt))
    if mismatch_at is not None:
        c, p = 0, 30000
        g = contigs[c]
        ref = bytes(g[p - 1:p + 3]).decode()
        bad = ref[0] + "".join("ACGT"[("ACGT".index(x) + 1) % 4] if x in "ACGT" else "A" for x in ref[1:])
        lines.insert(mismatch_at, "chr1\t%d\t.\t%s\t%s\t50\tPASS\tDP=10" % (p, bad, bad[0]))
    # every kind of line the reference drops or reports
    extra = [
        "chr1\t1000\t.\tA\tG\t50\tPASS",                 # fewer than 8 fields
        "chrUn\t1000\t.\tA\tG\t50\tPASS\tDP=1",          # unknown contig
        "chr1\t1001\t.\tA\t.\t50\tPASS\tDP=1",           # missing ALT
        "chr1\t1002\t.\tA\t<DEL>\t50\tPASS\tDP=1",       # symbolic ALT
        "chr1\t1003\t.\ta\tg\t50\tPASS\tDP=1",           # lowercase
        "chr1\t1004\t.\tA\t*\t50\tPASS\tDP=1",           # spanning deletion
        "",
        "  ",
        "chr2\t%d\t.\t%s\t%s\t50\tPASS\t\tDP=1" % (500, chr(contigs[1][499]), "T" if chr(contigs[1][499]) != "T" else "C"),  # double tab
        "\t chr2\t%d\t.\t%s\t%s\t50\tPASS\tDP=1 \t" % (700, chr(contigs[1][699]), "G" if chr(contigs[1][699]) != "G" else "A"),  # padded
    ]
    pos = len(lines) // 3
    for i, e in enumerate(extra):
        lines.insert(pos + 7 * i, e)
    return lines


HEADER = ["##fileformat=VCFv4.2", "##contig=<ID=chr1>", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"]


def _write_vcf(path, lines, crlf_every=5):
    """CRLF on every crlf_every-th line; a .gz path is written with gzip"""
    body = []
    for i, l in enumerate(HEADER + lines):
        body.append(l + ("\r\n" if crlf_every and i % crlf_every == 3 else "\n"))
    data = "".join(body).encode()
    if path.endswith(".gz"):
        with gzip.open(path, "wb") as f:
            f.write(data)
    else:
        with open(path, "wb") as f:
            f.write(data)


def f1(d, gz=False):
    contigs = _f1_genome()
    fa = os.path.join(d, "f1.fa")
    _write_fa(fa, contigs, ["chr1", "chr2"])
    vcf = os.path.join(d, "f1.vcf" + (".gz" if gz else ""))
    _write_vcf(vcf, _f1_lines(contigs, np.random.default_rng(72)))
    return fa, vcf, contigs


def f2(d):
    rng = np.random.default_rng(81)
    g = rng.choice(BASES, size=20000)
    g[5000:5300] = ord("A")
    fa = os.path.join(d, "f2.fa")
    _write_fa(fa, [g], ["chr1"])
    vcf = os.path.join(d, "f2.vcf")
    _write_vcf(vcf, ["chr1\t%d\t.\tA\tAAAA\t50\tPASS\tDP=10" % p for p in (5100, 5115, 5130, 5145, 5160)], crlf_every=0)
    return fa, vcf, [g]


def f3(d):
    contigs = _f1_genome()
    fa = os.path.join(d, "f3.fa")
    _write_fa(fa, contigs, ["chr1", "chr2"])
    vcf = os.path.join(d, "f3.vcf")
    lines = _f1_lines(contigs, np.random.default_rng(72), mismatch_at=200)
    _write_vcf(vcf, lines)
    return fa, vcf, contigs


FIXTURES = {"F1": f1, "F2": f2, "F3": f3}


def alt_contigs(contigs, vcf_path):
    """the contigs with the first ALT allele of every usable VCF line applied (left to right, overlapping ones skipped): reads
    simulated from these carry the variants"""
    op = gzip.open if vcf_path.endswith(".gz") else open
    with op(vcf_path, "rb") as f:
        text = f.read().decode()
    names = {"chr%d" % (i + 1): i for i in range(len(contigs))}
    per = [[] for _ in contigs]
    for line in text.split("\n"):
        parts = [p for p in line.strip("\t\r ").split("\t") if p]
        if not parts or parts[0].startswith("#") or len(parts) < 8 or parts[0] not in names:
            continue
        ref, alt = parts[3], parts[4].split(",")[0]
        if not alt or not set(ref + alt) <= set("ACGTN"):
            continue
        per[names[parts[0]]].append((int(parts[1]), ref, alt))
    out = []
    for g, vs in zip(contigs, per):
        s, at = [], 0
        for p, ref, alt in sorted(vs):
            if p - 1 < at or p - 1 + len(ref) > len(g):
                continue
            s.append(bytes(g[at:p - 1]))
            s.append(alt.encode())
            at = p - 1 + len(ref)
        s.append(bytes(g[at:]))
        out.append(np.frombuffer(b"".join(s), np.uint8).copy())
    return out


def reads_with_alts(contigs, vcf_path, n, seed, paired=False):
    """n reads (pairs), half of them from the contigs with the VCF's ALT alleles applied"""
    alt = alt_contigs(contigs, vcf_path)
    a = S.make_reads(contigs, n // 2, 100, seed=seed, paired=paired)
    b = S.make_reads(alt, n - n // 2, 100, seed=seed + 1, paired=paired)
    ren = lambda rs: [("alt_" + nm, sq, q) for nm, sq, q in rs]
    return (a[0] + ren(b[0]), a[1] + ren(b[1])) if paired else a + ren(b)
