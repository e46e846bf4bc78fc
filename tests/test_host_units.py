"""CPU-only tests of the header-only host pieces of the product (no GPU, no library): the BAM / BGZF writer behind `ngm-hip --bam`
(csrc/bam_writer.h; the GPU tier compares whole files with the reference program's, tests/test_gpu_bam.py) the thread pool
every host stage runs on (csrc/thread_pool.h), and the host formatter of `ngm-hip` (csrc/cli_format.h: records -> SAM lines / BAM records, the
output filter, the pair writer) that the GPU writers are compared against."""
import gzip
import os
import struct
import subprocess

import pytest

from sam_cases import CASES, Batch, hit, pair as _pair, rec   # the formatter's records and their hand-typed expectations, shared with the GPU writers' tests

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


def run_format(driver, tmp_path, opts, records, bam=False):
    """-> (SAM lines or decoded BAM records, the '#cov' / '#snp' lines, the six counters)"""
    return run_batch(driver, tmp_path, Batch(opts, records), bam)


def run_batch(driver, tmp_path, batch, bam=False):
    spec = str(tmp_path / "spec.txt")
    with open(spec, "w") as f:
        f.write(batch.spec())
    out = str(tmp_path / "out.bam")
    r = subprocess.run([driver, "format", spec] + ([out] if bam else []), capture_output=True, text=True, timeout=120)
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


def run_case(driver, tmp_path, name):
    for run in CASES[name]:
        out, _, counts = run_batch(driver, tmp_path, run.batch, run.bam)
        run.check(out, counts)


def test_formatter_single_end_records(format_driver, tmp_path):
    run_case(format_driver, tmp_path, "single_end")


def test_formatter_bam_records_pad_short_qualities(format_driver, tmp_path):
    run_case(format_driver, tmp_path, "bam_short_qualities")


@pytest.mark.parametrize("name", ["min-mq", "min-identity", "min-residues-fraction", "min-residues-count"])
def test_formatter_filters_at_and_below_their_thresholds(format_driver, tmp_path, name):
    run_case(format_driver, tmp_path, "filter-" + name)


def test_formatter_hard_clip_read_group_polya_tag_and_no_unal(format_driver, tmp_path):
    run_case(format_driver, tmp_path, "hard_clip")


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


def test_formatter_pair_writer_branches_and_tlen(format_driver, tmp_path):
    run_case(format_driver, tmp_path, "pair_branches")


def test_formatter_insert_size_window_strands_and_failed_pairs(format_driver, tmp_path):
    run_case(format_driver, tmp_path, "insert_window")


def test_formatter_broken_pairs_units(format_driver, tmp_path):
    records = ([rec("alone/1", "ACGTACGTAC", "ABCDEFGHIJ", hit(), unit=1), rec("-", "", "", hit(mapped=0), unit=2, seq_len=0)] +
               _pair("swapped", hit(pos=100), hit(pos=150, reverse=1), unit=4))
    sam, _, counts = run_format(format_driver, tmp_path, {"paired": 1}, records)
    assert [tuple(l.split("\t")[:2]) for l in sam] == [("alone/1", "0"), ("swapped/2", "83"), ("swapped/1", "163")]   # 0x40 and 0x80 change places
    assert counts == [3, 3, 3, 1, 0, 60]


def test_formatter_zs_tag_of_bisulfite_runs(format_driver, tmp_path):
    run_case(format_driver, tmp_path, "zs_tag")


def test_formatter_slam_seq_tags_in_sam_and_bam(format_driver, tmp_path):
    run_case(format_driver, tmp_path, "slam_seq")


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
