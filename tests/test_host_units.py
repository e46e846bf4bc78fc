"""CPU-only tests of the header-only host pieces of the product (no GPU, no library): the BAM / BGZF writer behind `ngm-hip --bam`
(csrc/bam_writer.h; the GPU tier compares whole files with the reference program's, tests/test_gpu_bam.py) the thread pool
every host stage runs on (csrc/thread_pool.h), and the host formatter of `ngm-hip` (csrc/cli_format.h: records -> SAM lines / BAM records, the
output filter, the pair writer) that the GPU writers are compared against."""
import gzip
import os
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("host_units") / "host_units_driver")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", os.path.join(ROOT, "tests", "cpp", "host_units_driver.cpp"), "-lz", "-o", exe])
    return exe


def reg2bin(beg, end):  # SAM specification, section 5.3
    end -= 1
    for shift, off in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return off + (beg >> shift)
    return 0


def test_bam_writer_produces_a_valid_file(driver, tmp_path):
    out = str(tmp_path / "t.bam")
    r = subprocess.run([driver, "bam", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(out, "rb").read()
    # BGZF: gzip members with the BC extra field and their own size; the last one is the 28-byte end-of-file marker
    assert raw[-28:] == bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
    at, members = 0, 0
    while at < len(raw):
        assert raw[at:at + 4] == b"\x1f\x8b\x08\x04" and raw[at + 12:at + 16] == b"BC\x02\x00"
        bsize, = struct.unpack_from("<H", raw, at + 16)
        isize, = struct.unpack_from("<I", raw, at + bsize + 1 - 4)
        assert isize <= 0xFF00
        at += bsize + 1
        members += 1
    assert at == len(raw) and members >= 5  # header, 3 record chunks (several blocks each), EOF
    data = gzip.decompress(raw)
    assert data[:4] == b"BAM\1"
    l_text, = struct.unpack_from("<i", data, 4)
    assert data[8:8 + l_text].decode().startswith("@HD\tVN:1.0")
    p = 8 + l_text
    n_ref, = struct.unpack_from("<i", data, p)
    p += 4
    refs = []
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", data, p)
        refs.append((data[p + 4:p + 4 + l_name - 1].decode(), struct.unpack_from("<i", data, p + 4 + l_name)[0]))
        p += 8 + l_name
    assert refs == [("chr1", 1000000), ("chrTwo", 54321)]
    n = 0
    while p < len(data):
        block, = struct.unpack_from("<i", data, p)
        ref_id, pos, bin_mq_nl, flag_nc, l_seq, mate_ref, mate_pos, tlen = struct.unpack_from("<iiIIiiii", data, p + 4)
        l_name, n_cig = bin_mq_nl & 0xFF, flag_nc & 0xFFFF
        q = p + 36
        assert data[q:q + l_name] == b"read%05d\0" % n
        q += l_name
        ops = struct.unpack_from("<%dI" % n_cig, data, q)
        q += 4 * n_cig
        unmapped = n % 97 == 0
        want_len = 100 + n % 51
        assert l_seq == want_len
        if unmapped:
            assert (ref_id, pos, n_cig, flag_nc >> 16) == (-1, -1, 0, 4)
            ref_span = 0
        else:
            lead = n % 7 + 1
            assert [(o >> 4, "MIDNSHP=X"[o & 15]) for o in ops] == [(lead, "S"), (20, "M"), (2, "I"), (30, "M"), (1, "D"), (want_len - 53 - lead, "M")]
            assert (ref_id, pos, (bin_mq_nl >> 8) & 0xFF, flag_nc >> 16) == (n % 2, 1000 + 37 * n, 60, 16 if n % 2 else 0)
            ref_span = 20 + 30 + 1 + want_len - 53 - lead
        assert bin_mq_nl >> 16 == reg2bin(pos, pos + ref_span)  # (bamtools' CalculateMinimumBin, also for the unmapped -1 / -1)
        seq = data[q:q + (l_seq + 1) // 2]
        q += (l_seq + 1) // 2
        want = "".join("ACGTN"[(n + 3 * t) % 5] for t in range(l_seq))
        got = "".join("=ACMGRSVTWYHKDBN"[(seq[t // 2] >> (4 if t % 2 == 0 else 0)) & 15] for t in range(l_seq))
        assert got == want
        qual = data[q:q + l_seq]
        q += l_seq
        assert qual == (bytes([ord(":") - 33]) * l_seq if n % 5 == 0 else bytes((n + t) % 40 for t in range(l_seq)))
        tags = data[q:p + 4 + block]
        assert tags == b"ASi" + struct.pack("<i", 1234 - n) + b"NMi" + struct.pack("<i", n % 9) + b"XIf" + struct.pack("<f", 0.9876) + b"MDZ50A49\0"
        assert (mate_ref, mate_pos, tlen) == (-1, -1, 0)
        p += 4 + block
        n += 1
    assert n == 2100
    # CalculateMinimumBin: the smallest bin that holds [begin, end)
    assert r.stdout.split()[1:] == [str(reg2bin(0, 1)), str(reg2bin(16383, 16385)), str(reg2bin(1 << 20, (1 << 20) + 150)), str(reg2bin(-1, -1)), str(reg2bin(100000000, 100000200))]


def test_thread_pool_covers_every_index_once_also_with_concurrent_and_nested_callers(driver):
    r = subprocess.run([driver, "pool"], capture_output=True, text=True, timeout=300, env=dict(os.environ, NGM_HIP_HOST_THREADS="8"))
    assert r.returncode == 0, r.stdout + r.stderr


def test_cli_rejects_what_it_does_not_support_before_touching_a_gpu():
    """`ngm-hip` takes NextGenMap's option names (src/config/Options.h); options of modes that are not built (bisulfite, SLAM-seq,
    fast pairing, argos, vcf) are refused loudly instead of being ignored, and so are unknown ones."""
    from nextgenmap_amd import build
    build.build()
    for bad in (["--bs-mapping"], ["--slam-seq", "2"], ["--frobnicate"]):
        r = subprocess.run([build.CLI, "-r", "x.fa", "-q", "y.fq", "-o", "/dev/null"] + bad, capture_output=True, text=True)
        assert r.returncode != 0, bad
        assert "[ngm-hip] error" in r.stderr, (bad, r.stderr)
    r = subprocess.run([build.CLI, "-r", "/nonexistent/ref.fa", "-q", "y.fq", "-o", "/dev/null"], capture_output=True, text=True)
    assert r.returncode != 0 and "cannot open reference" in (r.stdout + r.stderr)


# ---- the host formatter of `ngm-hip` (csrc/cli_format.h): what the GPU writers are compared against, checked here without a GPU ----------
# Every expected line below is typed by hand from the rules the code cites (SAMWriter.cpp:98-373, BAMWriter.cpp:147-433,
# GenericReadWriter.h:190-273, AlignmentBuffer.cpp:165-203); none is taken from the driver's output.

@pytest.fixture(scope="module")
def format_driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("host_format") / "host_units_driver")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                           os.path.join(ROOT, "tests", "cpp", "host_units_driver.cpp"), "-lz", "-o", exe])
    return exe


CHR1 = "GGACGTNACGTAGG" + "ACGT" * 100   # (the SLAM-seq cases read its first bases)
CHR2 = "ACGTTGCATGCC" + "TGCA" * 100
TAGS = "AS:i:80\tNM:i:0\tNH:i:1\tXI:f:1\tX0:i:1\tXE:i:7\tXR:i:10\tMD:Z:10"   # of hit() as it stands


def hit(mapped=1, contig=0, pos=100, reverse=0, mapq=60, score=80, identity=1.0, nm=0, qstart=0, qend=0, n_cand=1, n_best=1, votes=7, pair=0, cigar="10M", md="10"):
    return "hit %d %d %d %d %d %s %s %d %d %d %d %d %s %d %s %s" % (mapped, contig, pos, reverse, mapq, score, identity, nm, qstart, qend, n_cand, n_best, votes, pair, cigar, md)


def rec(name, row, qual, *hits, unit=0, polya=0, seq_len=None):
    return ["rec %s %s %s %d %d %d" % (name, row or "-", qual or "*", len(row) if seq_len is None else seq_len, unit, polya)] + list(hits)


def run_format(driver, tmp_path, opts, records, bam=False):
    """-> (SAM lines or decoded BAM records, the '#cov' / '#snp' lines, the six counters)"""
    spec = str(tmp_path / "spec.txt")
    with open(spec, "w") as f:
        f.write("contig chr1 %s\ncontig chr2 %s\n" % (CHR1, CHR2))
        for k, v in opts.items():
            f.write("opt %s %s\n" % (k, v))
        for r in records:   # (a record's lines, or one line)
            f.write(r + "\n" if isinstance(r, str) else "\n".join(r) + "\n")
    out = str(tmp_path / "out.bam")
    r = subprocess.run([driver, "format", spec] + ([out] if bam else []), capture_output=True, text=True, timeout=30)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")
    assert lines[-1] == "" and lines[-2].startswith("#counts ")
    body = [l for l in lines[:-2] if not l.startswith("#")]
    side = [l for l in lines[:-2] if l.startswith("#")]
    if bam:
        from test_gpu_bam import decode_bam
        assert body == []
        body = decode_bam(out)[2]
    return body, side, [int(x) for x in lines[-2].split()[1:]]


def test_formatter_single_end_records(format_driver, tmp_path):
    sam, _, counts = run_format(format_driver, tmp_path, {}, [
        rec("fwd", "ACGTACGTAC", "IIIIIHHHHH", hit()),
        rec("rev", "AACCGGTTAC", "ABCDEFGHIJ", hit(reverse=1, pos=7, contig=1, mapq=37, score=75.7, identity=0.9, nm=1, n_best=2, votes=6.9, md="4A5")),
        rec("noqual", "ACGTACGTAC", "", hit()),
        rec("empty", "", "", hit(mapped=0), seq_len=0),
        rec("unmapped", "ACGTACGTAC", "IIIIIHHHHH", hit(mapped=0)),
        rec("shortq", "ACGTACGTAC", "ABCDEF", hit()),
        rec("shortq_rev", "ACGTACGTAC", "ABCDEF", hit(reverse=1)),
    ])
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


def test_formatter_bam_records_pad_short_qualities(format_driver, tmp_path):
    recs, _, counts = run_format(format_driver, tmp_path, {}, [
        rec("shortq", "ACGTACGTAC", "ABCDEF", hit()),
        rec("shortq_rev", "ACGTACGTAC", "ABCDEF", hit(reverse=1)),
        rec("noqual", "ACGTACGTAC", "", hit()),
        rec("unmapped", "ACGTACGTAC", "ABCDEF", hit(mapped=0)),
    ], bam=True)
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


@pytest.mark.parametrize("opts,at,below", [
    ({"min_mq": 20}, dict(mapq=20), dict(mapq=19)),
    ({"min_identity": 0.9}, dict(identity=0.9), dict(identity=0.8999)),
    ({"min_residues": 0.5}, dict(qstart=3, qend=2), dict(qstart=3, qend=3)),     # a fraction of the 10 bases: 5 residues pass, 4 do not
    ({"min_residues": 8}, dict(qstart=1, qend=1), dict(qstart=2, qend=1)),       # above 1: a count
], ids=["min-mq", "min-identity", "min-residues-fraction", "min-residues-count"])
def test_formatter_filters_at_and_below_their_thresholds(format_driver, tmp_path, opts, at, below):
    sam, _, counts = run_format(format_driver, tmp_path, opts, [rec("at", "ACGTACGTAC", "IIIIIIIIII", hit(**at)), rec("below", "ACGTACGTAC", "IIIIIIIIII", hit(**below))])
    assert [l.split("\t")[:2] for l in sam] == [["at", "0"], ["below", "4"]]
    assert counts == [2, 1, 2, 0, 0, 0]


def test_formatter_hard_clip_read_group_polya_tag_and_no_unal(format_driver, tmp_path):
    records = [rec("clip", "ACGTACGTAC", "ABCDEFGHIJ", hit(reverse=1, qstart=2, qend=3, cigar="2H5M3H", md="5"), polya=3),
               rec("unmapped", "ACGTACGTAC", "ABCDEFGHIJ", hit(mapped=0))]
    sam, _, counts = run_format(format_driver, tmp_path, {"clip": 1, "rg": "grp", "xa_tag": 1}, records)
    assert sam == [
        # bases 2..6 of the reverse complement GTACGTACGT and of the reversed qualities JIHGFEDCBA; RG in front of the tags, XA:i behind X0:i
        "clip\t16\tchr1\t101\t60\t2H5M3H\t*\t0\t0\tACGTA\tHGFED\tRG:Z:grp\tAS:i:80\tNM:i:0\tNH:i:1\tXI:f:1\tX0:i:1\tXA:i:3\tXE:i:7\tXR:i:5\tMD:Z:5",
        "unmapped\t4\t*\t0\t0\t*\t*\t0\t0\tACGTACGTAC\tABCDEFGHIJ\tXA:i:0\tRG:Z:grp",   # an unmapped record: RG behind everything else
    ]
    assert counts == [2, 1, 2, 0, 0, 0]
    sam, _, counts = run_format(format_driver, tmp_path, {"no_unal": 1}, records)
    assert sam == ["clip\t16\tchr1\t101\t60\t2H5M3H\t*\t0\t0\tGTACGTACGT\tJIHGFEDCBA\tAS:i:80\tNM:i:0\tNH:i:1\tXI:f:1\tX0:i:1\tXE:i:7\tXR:i:5\tMD:Z:5"]   # no clip, no XA:i
    assert counts == [2, 1, 1, 0, 0, 0]


def test_formatter_topn_writes_distinct_locations_and_keeps_the_reference_quirks(format_driver, tmp_path):
    q = "IIIIIIIIII"
    records = [
        rec("twice", "ACGTACGTAC", q, hit(n_cand=3), hit(n_cand=3), hit(n_cand=3, pos=200)),                 # candidates 0 and 1 at one location: written once
        rec("three", "ACGTACGTAC", q, hit(n_cand=3), hit(pos=300, reverse=1), hit(pos=400, contig=1)),        # 0x100 on all but the first
        rec("sticky", "ACGTACGTAC", q, hit(n_cand=3), hit(pos=300, identity=0.5), hit(pos=400)),              # the second fails the identity filter: the third is not written
        rec("lastbad", "ACGTACGTAC", q, hit(n_cand=3), hit(pos=300), hit(pos=400, mapped=0)),                 # `mapped` is the LAST candidate's
        rec("two", "ACGTACGTAC", q, hit(n_cand=2), hit(pos=300), hit(pos=400)),                               # only n_candidates are looked at
    ]
    sam, _, counts = run_format(format_driver, tmp_path, {"topn": 3}, records)
    assert [tuple(l.split("\t")[:4]) for l in sam] == [
        ("twice", "0", "chr1", "101"), ("twice", "256", "chr1", "201"),
        ("three", "0", "chr1", "101"), ("three", "272", "chr1", "301"), ("three", "256", "chr2", "401"),
        ("sticky", "0", "chr1", "101"),
        ("lastbad", "4", "*", "0"),
        ("two", "0", "chr1", "101"), ("two", "256", "chr1", "301"),
    ]
    assert counts == [5, 4, 9, 0, 0, 0]
    # --strata: more best-scoring candidates than -n asks for -> the read is unmapped
    sam, _, counts = run_format(format_driver, tmp_path, {"topn": 3, "strata": 1}, [rec("many", "ACGTACGTAC", q, hit(n_cand=9, n_best=4), hit(pos=300), hit(pos=400)),
                                                                                   rec("few", "ACGTACGTAC", q, hit(n_cand=9, n_best=2), hit(pos=300), hit(pos=400))])
    assert [tuple(l.split("\t")[:4]) for l in sam] == [("many", "4", "*", "0"), ("few", "0", "chr1", "101"), ("few", "256", "chr1", "301")]
    assert counts == [2, 1, 3, 0, 0, 0]


def _pair(name, h1, h2, unit=0):
    return rec(name + "/1", "ACGTACGTAC", "ABCDEFGHIJ", h1, unit=unit) + rec(name + "/2", "AACCGGTTAC", "KLMNOPQRST", h2, unit=unit)


def test_formatter_pair_writer_branches_and_tlen(format_driver, tmp_path):
    records = (_pair("fr", hit(pos=100), hit(pos=150, reverse=1, qend=2)) +      # proper, first mate forward: TLEN from the aligned end of the second mate
               _pair("rf", hit(pos=150, reverse=1, qend=2), hit(pos=100)) +      # proper, first mate reverse
               _pair("none", hit(mapped=0), hit(mapped=0)) +
               _pair("m2only", hit(mapped=0), hit(pos=150, reverse=1)) +
               _pair("m1only", hit(pos=100), hit(mapped=0)) +
               _pair("contigs", hit(pos=100), hit(pos=150, reverse=1, contig=1)) +
               _pair("lost", hit(pos=100, pair=4), hit(pos=150, reverse=1)))
    t1, t2 = TAGS, TAGS.replace("XR:i:10", "XR:i:8")
    sam, _, counts = run_format(format_driver, tmp_path, {"paired": 1}, records)
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
    # BAM: positions 0-based, TLEN over the whole read (60 = 150 + 10 - 100)
    recs, _, counts_bam = run_format(format_driver, tmp_path, {"paired": 1}, records, bam=True)
    assert [(r["name"], r["flag"], r["ref_id"], r["pos"], r["mate_ref"], r["mate_pos"], r["tlen"]) for r in recs] == [
        (b"fr/2", 147, 0, 150, 0, 100, -60), (b"fr/1", 99, 0, 100, 0, 150, 60),
        (b"rf/2", 163, 0, 100, 0, 150, 60), (b"rf/1", 83, 0, 150, 0, 100, -60),
        (b"none/2", 141, -1, -1, -1, -1, 0), (b"none/1", 77, -1, -1, -1, -1, 0),
        (b"m2only/2", 153, 0, 150, 0, 150, 0), (b"m2only/1", 69, 0, 150, 0, 150, 0),
        (b"m1only/2", 133, 0, 100, 0, 100, 0), (b"m1only/1", 73, 0, 100, 0, 100, 0),
        (b"contigs/2", 145, 1, 150, 0, 100, 0), (b"contigs/1", 97, 0, 100, 1, 150, 0),
    ]
    assert counts_bam == counts


def test_formatter_insert_size_window_strands_and_failed_pairs(format_driver, tmp_path):
    # the distance is the difference of the positions plus the length (10) of the mate on the left
    records = (_pair("at_min", hit(pos=100), hit(pos=130, reverse=1)) + _pair("at_max", hit(pos=100), hit(pos=150, reverse=1)) +
               _pair("below", hit(pos=100), hit(pos=129, reverse=1)) + _pair("above", hit(pos=100), hit(pos=151, reverse=1)) +
               _pair("strand", hit(pos=100), hit(pos=140)) + _pair("failed", hit(pos=100, pair=2), hit(pos=140, reverse=1)))
    sam, _, counts = run_format(format_driver, tmp_path, {"paired": 1, "min_insert": 40, "max_insert": 60}, records)
    assert [tuple(l.split("\t")[i] for i in (0, 1, 6, 8)) for l in sam] == [
        ("at_min/2", "147", "=", "-40"), ("at_min/1", "99", "=", "40"), ("at_max/2", "147", "=", "-60"), ("at_max/1", "99", "=", "60"),
        ("below/2", "145", "chr1", "0"), ("below/1", "97", "chr1", "0"), ("above/2", "145", "chr1", "0"), ("above/1", "97", "chr1", "0"),
        ("strand/2", "129", "chr1", "0"), ("strand/1", "65", "chr1", "0"),
        ("failed/2", "145", "chr1", "0"), ("failed/1", "97", "chr1", "0"),   # NGM_PAIR_FAILED: not proper, though its geometry is
    ]
    assert counts == [12, 12, 12, 6, 3, 40 + 60 + 50]   # broken: below, above, strand; the failed pair's 50 counts as an insert size


def test_formatter_broken_pairs_units(format_driver, tmp_path):
    records = (rec("alone/1", "ACGTACGTAC", "ABCDEFGHIJ", hit(), unit=1) + rec("-", "", "", hit(mapped=0), unit=2, seq_len=0) +
               _pair("swapped", hit(pos=100), hit(pos=150, reverse=1), unit=4))
    sam, _, counts = run_format(format_driver, tmp_path, {"paired": 1}, records)
    assert [tuple(l.split("\t")[:2]) for l in sam] == [("alone/1", "0"), ("swapped/2", "83"), ("swapped/1", "163")]   # 0x40 and 0x80 change places
    assert counts == [3, 3, 3, 1, 0, 60]


def test_formatter_zs_tag_of_bisulfite_runs(format_driver, tmp_path):
    sam, _, _ = run_format(format_driver, tmp_path, {"bs_mapping": 1}, [rec("f", "ACGTACGTAC", "", hit()), rec("r", "ACGTACGTAC", "", hit(reverse=1))])
    assert [l.split("\t")[14] for l in sam] == ["ZS:Z:++", "ZS:Z:-+"]
    sam, _, _ = run_format(format_driver, tmp_path, {"bs_mapping": 1, "paired": 1}, _pair("fr", hit(pos=100), hit(pos=150, reverse=1)) + _pair("rf", hit(pos=150, reverse=1), hit(pos=100)))
    assert [(l.split("\t")[0], l.split("\t")[14]) for l in sam] == [("fr/2", "ZS:Z:+-"), ("fr/1", "ZS:Z:++"), ("rf/2", "ZS:Z:--"), ("rf/1", "ZS:Z:-+")]
    recs, _, _ = run_format(format_driver, tmp_path, {"bs_mapping": 1}, [rec("r", "ACGTACGTAC", "", hit(reverse=1))], bam=True)
    assert recs[0]["tags"][21:27] == b"ZSZ-+\0"   # behind AS, NM and NH (7 bytes each)


def test_formatter_slam_seq_tags_in_sam_and_bam(format_driver, tmp_path):
    records = [
        # chr1 from base 2: ACGTNACGTA.  Column 5 is N in the reference, column 7 N in the read, column 9 a T>C conversion
        rec("mis", "ACGTAANGCA", "", hit(pos=2, nm=3, md="4N1C1T1")),
        # chr2 from base 0: ACG-TTgCATG: one base inserted behind ACG, the reference's G deleted behind TT, no mismatch
        rec("indel", "ACGTTTCATG", "", hit(pos=0, contig=1, cigar="3M1I2M1D4M", md="5^G4")),
        # reverse strand, chr2 from base 0: ACGTTGCATG against the read's reverse complement GCGTTGCATG: A>G in column 1
        rec("rev", "CATGCAACGC", "", hit(pos=0, contig=1, reverse=1, nm=1, md="0A9")),
    ]
    ra = ["3,0,0,0,0,0,1,0,0,1,0,0,2,0,0,0,1,0,1,0,1,0,0,0,0", "2,0,0,0,0,0,2,0,0,0,0,0,2,0,0,0,0,0,3,0,0,0,0,0,0", "1,0,1,0,0,0,2,0,0,0,0,0,3,0,0,0,0,0,3,0,0,0,0,0,0"]
    sam, _, _ = run_format(format_driver, tmp_path, {"slam_seq": 1}, records)
    assert [l.split("\t")[19:] for l in sam] == [
        ["TC:i:1", "RA:Z:" + ra[0], "MP:Z:20:5:5,9:7:7,16:9:9"],   # type = 5 x reference class + read class (A C G T other): N>A, C>N, T>C
        ["TC:i:0", "RA:Z:" + ra[1]],                                  # no mismatch: no MP
        ["TC:i:1", "RA:Z:" + ra[2], "MP:Z:2:1:1"],                   # reverse strand: TC counts A>G
    ]
    assert [l.split("\t")[9] for l in sam] == ["ACGTAANGCA", "ACGTTTCATG", "GCGTTGCATG"]
    recs, _, _ = run_format(format_driver, tmp_path, {"slam_seq": 1}, records, bam=True)
    tail = lambda r: r["tags"][r["tags"].index(b"TCi"):]
    assert tail(recs[0]) == b"TCi" + struct.pack("<i", 1) + b"RAZ" + ra[0].encode() + b",\0MPZ20:5:5,9:7:7,16:9:9\0"   # BAM: a comma behind every count
    assert tail(recs[1]) == b"TCi" + struct.pack("<i", 0) + b"RAZ" + ra[1].encode() + b",\0"
    assert tail(recs[2]) == b"TCi" + struct.pack("<i", 1) + b"RAZ" + ra[2].encode() + b",\0MPZ2:1:1\0"


def test_formatter_hands_primary_records_to_coverage_and_snp(format_driver, tmp_path):
    records = [rec("two", "ACGTACGTAC", "ABCDEF", hit(n_cand=2), hit(pos=300), hit()),                        # its second record carries 0x100
               rec("noqual", "AACCGGTTAC", "", hit(n_cand=1, pos=500, reverse=1, cigar="4M1D6M"), hit(), hit()),
               rec("unmapped", "ACGTACGTAC", "ABCDEFGHIJ", hit(mapped=0, n_cand=0), hit(), hit())]
    for bam in (False, True):
        out, side, counts = run_format(format_driver, tmp_path, {"topn": 3, "coverage": 1, "snp": 1}, records, bam=bam)
        assert len(out) == 4 and counts == [3, 2, 4, 0, 0, 0]
        # one call each per range; the sequence and the qualities as the record prints them, short qualities padded with ':'
        assert side == ["#snp noqual 0:500:4M1D6M:GTAACCGGTT", "#snp qual 0:100:10M:ACGTACGTAC:ABCDEF::::", "#cov 0:100:10M 0:500:4M1D6M"]
    _, side, _ = run_format(format_driver, tmp_path, {"topn": 3}, records)
    assert side == []
