"""No GPU: what `ngm-hip --snp` refuses before any GPU work, the model of tests/snp_model.py pinned on a file written out by hand, the
host-only parts of the SNP caller (nextgenmap_amd/csrc/snp.h: the walk over CIGAR and sequence, the checks, the packed reference, the
counters' layout, the call rule, the serialiser) through tests/cpp/snp_driver.cpp, a stand-alone program built with
g++ -fsanitize=address,undefined, and the host-only VCF reader of --vcf over every file the model writes."""
import os
import subprocess

import pytest

import snp_model as M
from test_vcf_host import _parse as parse_vcf_with_the_reader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "nextgenmap_amd", "ngm-hip")
SRC = os.path.join(ROOT, "tests", "cpp", "snp_driver.cpp")
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")


def _cli(tmp_path, extra, snp=None):
    # (neither input exists: the refusal comes from the option check, before the reference or the reads are opened)
    return subprocess.run([CLI, "-r", str(tmp_path / "none.fa"), "-q", str(tmp_path / "none.fq"), "-o", str(tmp_path / "out.sam"), "--snp", snp or str(tmp_path / "out.vcf")] + extra,
                          capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("extra,message", [
    (["--argos"], "--snp cannot be combined with --argos: "),
    (["--shard", "0/2"], "--snp cannot be combined with --shard: "),
    (["--shard-output"], "--snp cannot be combined with --shard-output: "),
    (["--bs-mapping"], "--snp cannot be combined with --bs-mapping: "),
    (["--vcf", "known.vcf"], "--snp cannot be combined with --vcf: "),
    (["SAME-AS-OUTPUT"], "--snp cannot be combined with -o "),
    (["SAME-AS-COVERAGE"], "--snp cannot be combined with --coverage "),
], ids=["argos", "shard", "shard-output", "bs-mapping", "vcf", "same-as-output", "same-as-coverage"])
def test_snp_refuses_unsupported_combinations(tmp_path, extra, message):
    from nextgenmap_amd import build
    build.build()
    snp = None
    if extra == ["SAME-AS-OUTPUT"]:
        snp, extra = str(tmp_path / "out.sam"), []
    elif extra == ["SAME-AS-COVERAGE"]:
        snp, extra = str(tmp_path / "both.txt"), ["--coverage", str(tmp_path / "both.txt")]
    r = _cli(tmp_path, extra, snp)
    assert r.returncode != 0
    assert message in r.stderr, r.stderr
    assert [m for m in r.stderr.splitlines() if message in m][0].split(message)[1].strip()   # (a reason follows)
    assert not any(os.path.exists(tmp_path / n) for n in ("out.sam", "out.vcf", "both.txt"))
    assert "HIP backend (gfx950)" not in r.stderr + r.stdout and "index entries" not in r.stderr


@pytest.mark.parametrize("extra,message", [
    (["--snp-min-frac", "0"], "--snp-min-frac"), (["--snp-min-frac", "1.01"], "--snp-min-frac"), (["--snp-min-frac", "-0.5"], "--snp-min-frac"),
    (["--snp-min-frac", "half"], "--snp-min-frac"), (["--snp-min-cov", "-1"], "--snp-min-cov"), (["--snp-min-qual", "-1"], "--snp-min-qual"),
    (["--snp-min-qual", "94"], "--snp-min-qual"),
])
def test_snp_refuses_thresholds_out_of_range(tmp_path, extra, message):
    from nextgenmap_amd import build
    build.build()
    r = _cli(tmp_path, extra)
    assert r.returncode != 0 and message + " expects" in r.stderr, r.stderr
    assert not os.path.exists(tmp_path / "out.vcf") and "HIP backend (gfx950)" not in r.stderr + r.stdout


def test_model_equals_a_hand_written_file():
    #                    0123456789012345678901234
    contigs = [("chr1", "ACGTACGTNNacgtACGTACGTACGT"), ("chr2", "TTTTT")]
    records = [(0, 0, "8M", "ACGTACGA", None),              # T>A at 7
               (0, 0, "8M", "AGGTACGA", "IIIIIIII"),        # C>G at 1 and T>A at 7, quality 40
               (0, 2, "2S4M2D4M", "TTGAACNCTG", None),      # G, T>A at 3, A, C | 2D | N over N, C over N, a>T at 10, c>G at 11: no vote over N
               (0, 10, "3M1I2M", "ATGGAA", "I/0III"),       # c>T at 11 at quality 14: no vote; g over g; inserted G; t>A at 13; A over A
               (0, 24, "4M", "GGAA", None),                 # G over G at 24, T>G at 25, the rest is clipped
               (1, 0, "5M", "TTCTN", None), (1, 2, "1M", "C", None), (1, 2, "1M", "G", None)]
    # depths: chr1 0-1: 2, 2: 3, 3-5: 3, 6-7: 2, 8-9: 1, 10-11: 2 (third record's 4M at 8..11, fourth at 10..12), ...
    want_lines = ["chr1\t2\t.\tC\tG\t.\tPASS\tDP=2;AO=1\n",          # 1 of 2
                  "chr1\t4\t.\tT\tA\t.\tPASS\tDP=3;AO=1\n",          # 1 of 3: 1 >= 0.3 * 3
                  "chr1\t8\t.\tT\tA\t.\tPASS\tDP=2;AO=2\n",
                  "chr1\t11\t.\tA\tT\t.\tPASS\tDP=2;AO=1\n",         # lower-case reference, REF upper-case; position 10
                  "chr1\t12\t.\tC\tG\t.\tPASS\tDP=2;AO=1\n",         # position 11: the T at quality 14 does not vote, but counts in the depth
                  "chr1\t14\t.\tT\tA\t.\tPASS\tDP=1;AO=1\n",         # position 13 (behind the insertion)
                  "chr1\t26\t.\tT\tG\t.\tPASS\tDP=1;AO=1\n",         # the contig's last base
                  "chr2\t3\t.\tT\tC\t.\tPASS\tDP=3;AO=2\n"]          # C twice, G once
    head = ("##fileformat=VCFv4.2\n##source=ngm-hip --snp (min-cov 1, min-frac 0.3, min-qual 15)\n##contig=<ID=chr1,length=26>\n##contig=<ID=chr2,length=5>\n"
            '##INFO=<ID=DP,Number=1,Type=Integer,Description="records covering the base">\n'
            '##INFO=<ID=AO,Number=1,Type=Integer,Description="records with the ALT base at quality >= 15">\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n')
    assert M.vcf(contigs, records, 1, "0.3", 15).decode() == head + "".join(want_lines)
    assert M.totals(contigs, records, 1, "0.3", 15) == dict(alignments=8, alt_bases=11, calls=8, text_bytes=len(head + "".join(want_lines)),
                                                            covered_bases=8 + 8 + 8 + 5 + 2 + 5 + 1 + 1)
    assert M.vcf(contigs, records, 2, "0.8", 15).decode() == head.replace("min-cov 1, min-frac 0.3", "min-cov 2, min-frac 0.8") + want_lines[2]
    sam = ["@SQ\tSN:chr1\tLN:26\n", "r\t0\tchr1\t3\t60\t5M\t*\t0\t0\tACGTA\tIIIII\n", "s\t256\tchr1\t3\t60\t5M\t*\t0\t0\tACGTA\t*\n", "u\t4\t*\t0\t0\t*\t*\t0\t0\tA\t*\n",
           "t\t16\tchr1\t9\t60\t2M\t*\t0\t0\tAC\t*\n"]
    assert M.records_of_sam(sam, contigs) == [(0, 2, "5M", "ACGTA", "IIIII"), (0, 8, "2M", "AC", None)]


# ---- the driver ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """the stand-alone program, with AddressSanitizer and UndefinedBehaviorSanitizer in it"""
    d = tmp_path_factory.mktemp("snp_driver")
    out = str(d / "snp_driver_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", out])
    return out, d


def _input(contigs, records, N, F, Q):
    return ("%d\n" % len(contigs) + "".join("%s %s\n" % (n, s or "-") for n, s in contigs) + "%d %s %d\n" % (N, F, Q) +
            "".join("%d %d %s %s %s\n" % (c, p, g or "-", s or "-", "*" if q is None else (q or "-")) for c, p, g, s, q in records))


def _file(exe, case):
    prog, d = exe
    p = str(d / "case.txt")
    with open(p, "w") as f:
        f.write(_input(*case))
    r = subprocess.run([prog, "file", p, p + ".out"], capture_output=True, text=True, env=SAN_ENV)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    return open(p + ".out", "rb").read(), dict(zip(("alignments", "alt_bases", "calls", "covered_bases"), (int(x) for x in r.stdout.split())))


@pytest.mark.parametrize("name", list(M.UNIT_CASES) + list(M.CHUNK_CASES))
def test_driver_equals_the_model_on_the_unit_cases(exe, name):
    case = {**M.UNIT_CASES, **M.CHUNK_CASES}[name]
    text, st = _file(exe, case)
    want = M.vcf(*case)
    assert text == want
    totals = M.totals(*case)
    assert st == {k: totals[k] for k in st}
    if name in ("nothing", "no-call-without-a-mismatch"):
        assert text == M.header(case[0], *case[2:]).encode()
    elif name != "padding-and-empty":
        assert totals["calls"] >= 1


def test_the_unit_cases_decide_what_they_are_named_for():
    """the cases are only worth their names if the model's answers on them are the ones the names promise"""
    pos = lambda name: [(c, p) for c, p, *_ in M.calls(*M.UNIT_CASES[name])]
    assert pos("depth-n-and-n-minus-1") == [(0, 12)] and pos("fraction-4-of-5-and-3-of-5") == [(0, 12)] and pos("fraction-8-of-10-and-7-of-10") == [(0, 12)]
    assert pos("fraction-one") == [(0, 12)] and pos("min-cov-zero-is-one") == [(0, 12)]
    assert pos("clipped-at-the-end") == [(0, 198), (0, 199)]
    # (15: quality 15, quality 14, no quality string; 16: quality 15 twice, quality 14 -- two votes out of a depth of four each time)
    assert [(p, d, n) for _, p, _, _, d, n in M.calls(*M.UNIT_CASES["quality-threshold"])] == [(15, 4, 2), (16, 4, 2)]
    assert [(p, r) for _, p, r, *_ in M.calls(*M.UNIT_CASES["excluded-bases"])] == [(8, M.UNIT_CASES["excluded-bases"][0][0][1][8].upper()), (9, M.UNIT_CASES["excluded-bases"][0][0][1][9].upper()), (20, M.UNIT_CASES["excluded-bases"][0][0][1][20])]
    tie = M.calls(*M.UNIT_CASES["two-way-tie"])
    ref = M.UNIT_CASES["two-way-tie"][0][0][1]
    assert [(p, a, n) for _, p, _, a, _, n in tie] == [(10, min(M.other(ref[10], 3), M.other(ref[10], 1)), 2), (40, min(M.other(ref[40], 2), M.other(ref[40], 3)), 3)]
    assert [(d, n) for *_, d, n in M.calls(*M.UNIT_CASES["three-alternatives"])] == [(6, 3)]
    assert pos("first-and-last-column") == [(0, 20), (0, 29)]
    chunk = lambda name: [(c, p) for c, p, *_ in M.calls(*M.CHUNK_CASES[name])]
    assert chunk("first-and-last-slot-of-a-chunk") == [(0, 0), (0, 63), (0, 64), (0, 127), (0, 128), (0, 255), (0, 256), (0, 299)]
    assert chunk("contig-begins-in-mid-chunk") == [(0, 39), (1, 0), (1, 22), (1, 23), (1, 99), (2, 0), (2, 22)]
    assert len(chunk("depth-across-three-chunks")) == 6


def test_driver_equals_the_model_on_random_records(exe):
    case = M.random_case(77, 4000)
    text, st = _file(exe, case)
    want = M.vcf(*case)
    totals = M.totals(*case)
    assert text == want and totals["calls"] >= 20 and totals["alt_bases"] > 2000
    assert st == {k: totals[k] for k in st}
    # with every threshold at its loosest
    loose = case[:2] + (0, "0.001", 0)
    text, st = _file(exe, loose)
    assert text == M.vcf(*loose) and st["calls"] == M.totals(*loose)["calls"] > 500


# the records ngm_snp_add refuses beyond those ngm_coverage_add refuses (tests/test_coverage_host.BAD), over snp_model's two contigs
BAD = [((0, 0, "5M", "ACGT", None), "its sequence is shorter or longer"), ((0, 0, "5M", "ACGTAC", None), "its sequence is shorter or longer"),
       ((0, 0, "2S3M1I2D1M2H", "ACGTACGT", None), "its sequence is shorter or longer"), ((0, 0, "5M", "", None), "its sequence is shorter or longer"),
       ((0, 0, "4H", "A", None), "its sequence is shorter or longer"), ((0, 0, "5M", "ACGTA", "IIII"), "its quality text has another length"),
       ((2, 0, "5M", "ACGTA", None), "its ref_id is not in [0, n_ref)"), ((0, -1, "5M", "ACGTA", None), "its position is negative"),
       ((0, 0, "5Q", "ACGTA", None), "unknown operation character"), ((0, 0, "268435456M", "A", None), "overflows 2^28"), ((0, 0, "M", "", None), "operation without a number"),
       ((0, 0, "5M3", "ACGTA", None), "number without an operation")]
GOOD = [(0, 0, "2S3M1I2D1M2H", "ACGTACG", None), (1, 49, "1M", "A", "I"), (0, 0, "", "", None), (0, 2147483647, "3S5M", "ACGTACGT", "IIIIIIII"), (0, 5, "4H2P", "", None)]


def test_checks_refuse_every_malformed_record_with_its_message(exe):
    prog, d = exe
    contigs = M.UNIT_CASES["nothing"][0]
    p = str(d / "check.txt")
    with open(p, "w") as f:
        f.write(_input(contigs, [a for a, _ in BAD] + GOOD, 10, "0.8", 15))
    r = subprocess.run([prog, "check", p], capture_output=True, text=True, env=SAN_ENV)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(BAD) + len(GOOD)
    for (a, msg), line in zip(BAD, lines):
        assert not line.startswith("0 ") and msg in line, (a, line)
    for a, line in zip(GOOD, lines[len(BAD):]):
        assert line.startswith("0 "), (a, line)


# ---- --vcf reads what --snp writes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(M.UNIT_CASES) + list(M.CHUNK_CASES))
def test_the_vcf_reader_gives_exactly_the_models_calls(tmp_path, name):
    from nextgenmap_amd import build
    build.build()
    case = {**M.UNIT_CASES, **M.CHUNK_CASES}[name]
    path = tmp_path / "calls.vcf"
    path.write_bytes(M.vcf(*case))
    starts = [(n, 1000000 * i) for i, (n, _) in enumerate(case[0])]
    count, rows = parse_vcf_with_the_reader(str(path), starts)
    want = [(1000000 * c + p + 1, r, a) for c, p, r, a, _, _ in M.calls(*case)]
    assert count == len(want) and rows == want
