"""No GPU: what `ngm-hip --count` refuses before any GPU work -- the combinations, and every error of the BED file, by message -- the model of
tests/count_model.py pinned on a file written out by hand, and the host-only parts of the conversion counter (nextgenmap_amd/csrc/count.h:
the BED reader, the tables, the walk of a record, the sums, the serialiser) through tests/cpp/count_driver.cpp, a stand-alone program
built with g++ -fsanitize=address,undefined and fed through its standard input."""
import os
import subprocess

import pytest

import count_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "nextgenmap_amd", "ngm-hip")
SRC = os.path.join(ROOT, "tests", "cpp", "count_driver.cpp")
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")


def _cli(tmp_path, extra, count_out=None, bed="utrs.bed"):
    # (neither input exists: the refusal comes from the option check, before the reference, the BED file or the reads are opened)
    return subprocess.run([CLI, "-r", str(tmp_path / "none.fa"), "-q", str(tmp_path / "none.fq"), "-o", str(tmp_path / "out.sam"), "--count", str(tmp_path / bed),
                           "--count-out", count_out or str(tmp_path / "out.tsv")] + extra, capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("extra,message", [
    (["--argos"], "--count cannot be combined with --argos: "),
    (["--shard", "0/2"], "--count cannot be combined with --shard: "),
    (["--shard-output"], "--count cannot be combined with --shard-output: "),
    (["--bs-mapping"], "--count cannot be combined with --bs-mapping: "),
    (["SAME-AS-OUTPUT"], "--count cannot be combined with -o "),
    (["SAME-AS-COVERAGE"], "--count cannot be combined with --coverage "),
    (["SAME-AS-SNP"], "--count cannot be combined with --snp "),
], ids=["argos", "shard", "shard-output", "bs-mapping", "same-as-output", "same-as-coverage", "same-as-snp"])
def test_count_refuses_unsupported_combinations(tmp_path, extra, message):
    from nextgenmap_amd import build
    build.build()
    count_out = None
    if extra == ["SAME-AS-OUTPUT"]:
        count_out, extra = str(tmp_path / "out.sam"), []
    elif extra == ["SAME-AS-COVERAGE"]:
        count_out, extra = str(tmp_path / "both.txt"), ["--coverage", str(tmp_path / "both.txt")]
    elif extra == ["SAME-AS-SNP"]:
        count_out, extra = str(tmp_path / "both.txt"), ["--snp", str(tmp_path / "both.txt")]
    r = _cli(tmp_path, extra, count_out)
    assert r.returncode != 0
    assert message in r.stderr, r.stderr
    assert [m for m in r.stderr.splitlines() if message in m][0].split(message)[1].strip()   # (a reason follows)
    assert not any(os.path.exists(tmp_path / n) for n in ("out.sam", "out.tsv", "both.txt"))
    assert "HIP backend (gfx950)" not in r.stderr + r.stdout and "index entries" not in r.stderr


def test_count_and_count_out_need_each_other(tmp_path):
    from nextgenmap_amd import build
    build.build()
    base = [CLI, "-r", str(tmp_path / "none.fa"), "-q", str(tmp_path / "none.fq"), "-o", str(tmp_path / "out.sam")]
    r = subprocess.run(base + ["--count", "utrs.bed"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--count needs --count-out FILE" in r.stderr, r.stderr
    r = subprocess.run(base + ["--count-out", str(tmp_path / "out.tsv")], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--count-out needs --count FILE" in r.stderr, r.stderr
    assert not os.path.exists(tmp_path / "out.tsv") and "HIP backend (gfx950)" not in r.stderr + r.stdout


@pytest.mark.parametrize("q", ["-1", "94", "high", ""])
def test_count_refuses_a_quality_out_of_range(tmp_path, q):
    from nextgenmap_amd import build
    build.build()
    r = _cli(tmp_path, ["--count-min-qual", q])
    assert r.returncode != 0 and "--count-min-qual expects a Phred quality in 0..93" in r.stderr, r.stderr
    assert "HIP backend (gfx950)" not in r.stderr + r.stdout


# ---- the BED file -------------------------------------------------------------------------------------------------------------------
# contigs of 80 and 30 bases (and, for the command line, one of 4 bases, which the reference drops)
BED_CONTIGS = [("c1", "ACGTACGTACGTTTTTACGTACGATCGATCGATCGATTTACGACTAGCATCGACTACGACTAGCACTAGCTAGCATCGAA"), ("c2", "ACGTACGTACGTTTTTACGTACGATCGATC")]
GOOD_LINE = "c1\t5\t20\tu1\t0\t+\n"
BAD_BEDS = {
    "two-columns": (GOOD_LINE + "c1\t5\n", "line 2: it has fewer than 3 tab-separated columns"),
    "spaces-for-tabs": ("c1 5 20\n", "line 1: it has fewer than 3 tab-separated columns"),
    "unknown-contig": (GOOD_LINE + "\n# comment\nchrX\t1\t2\n", "line 4: contig chrX is not in the reference"),
    "start-not-a-number": ("c1\tfive\t20\n", "line 1: its start five is not a number"),
    "start-negative": ("c1\t-1\t20\n", "line 1: its start -1 is not a number"),
    "end-not-a-number": ("c1\t5\t2e1\n", "line 1: its end 2e1 is not a number"),
    "end-empty": ("c1\t5\t\n", "line 1: its end  is not a number"),
    "end-of-eleven-digits": ("c1\t5\t10000000000\n", "line 1: its end 10000000000 is not a number"),
    "end-beyond-32-bits": ("c1\t5\t4294967296\n", "line 1: its end 4294967296 is not a number"),
    "start-equals-end": ("track name=x\nc1\t20\t20\n", "line 2: its start is not in front of its end"),
    "start-behind-end": ("c1\t30\t20\n", "line 1: its start is not in front of its end"),
    "end-behind-the-contig": ("c2\t0\t30\nc2\t5\t31\n", "line 2: its end lies behind the contig's last base (30 bases)"),
    "strand-star": ("c1\t5\t20\tn\t0\t*\n", "line 1: its strand * is not +, - or ."),
    "strand-empty": ("c1\t5\t20\tn\t0\t\n", "line 1: its strand  is not +, - or ."),
    "strand-two-characters": ("c1\t5\t20\tn\t0\t+-\n", "line 1: its strand +- is not +, - or ."),
    "no-region": ("# only\n\ntrack name=x\nbrowser position c1:1-2\n\r\n", "line 0: the file has no region"),
    "empty-file": ("", "line 0: the file has no region"),
}
GOOD_BED = "browser hide all\ntrack name=utrs\n# a comment\n\n" + GOOD_LINE + "c2\t0\t30\r\nc1\t79\t80\tlast\nc1\t5\t20\t\t7\t-\textra\tcolumns\nc2\t3\t4\tno-newline\t0\t."
GOOD_REGIONS = [(0, 5, 20, "u1", "+"), (1, 0, 30, ".", "."), (0, 79, 80, "last", "."), (0, 5, 20, "", "-"), (1, 3, 4, "no-newline", ".")]


def test_the_models_bed_reader():
    assert M.parse_bed(GOOD_BED, BED_CONTIGS) == GOOD_REGIONS
    for name, (text, message) in BAD_BEDS.items():
        with pytest.raises(M.BedError) as e:
            M.parse_bed(text, BED_CONTIGS)
        assert str(e.value) == message, name


@pytest.mark.parametrize("name", list(BAD_BEDS) + ["dropped-contig", "unreadable"])
def test_count_refuses_a_bad_bed_file_by_its_line(tmp_path, name):
    """before any GPU work: the contigs come from the FASTA as the reference will hold them (a contig of 10 bases or fewer is not one)"""
    from nextgenmap_amd import build
    build.build()
    fa, bed = str(tmp_path / "ref.fa"), str(tmp_path / "utrs.bed")
    with open(fa, "w") as f:
        f.write(">c1 the first\n%s\n%s\n>tiny\nACGT\n>c2\tsecond\n%s\n" % (BED_CONTIGS[0][1][:50], BED_CONTIGS[0][1][50:], BED_CONTIGS[1][1]))
    text, message = {"dropped-contig": (GOOD_LINE + "tiny\t0\t2\n", "line 2: contig tiny is not in the reference"), "unreadable": (None, None)}.get(name) or BAD_BEDS[name]
    if text is not None:
        with open(bed, "w", newline="") as f:
            f.write(text)
    r = subprocess.run([CLI, "-r", fa, "-q", str(tmp_path / "none.fq"), "-o", str(tmp_path / "out.sam"), "--count", bed, "--count-out", str(tmp_path / "out.tsv")],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    want = "--count: cannot read " + bed if text is None else "--count: %s %s" % (bed, message)
    assert "[ngm-hip] error: " + want + "\n" in r.stderr, r.stderr
    assert not os.path.exists(tmp_path / "out.tsv") and not os.path.exists(tmp_path / "out.sam")
    assert "HIP backend (gfx950)" not in r.stderr + r.stdout and "index entries" not in r.stderr


# ---- the model, by hand ---------------------------------------------------------------------------------------------------------------
def test_model_equals_a_hand_written_file():
    #                    01234567890123456789
    contigs = [("chr1", "ATTCGTTAACTTGGATTTCA"), ("chr2", "ttaaNTA")]
    regions = [(0, 0, 10, "u1", "+"),     # T at 1 2 5 6
               (0, 5, 20, "u2", "-"),     # A at 7 8 14 19
               (0, 8, 12, "dot", "."),    # A at 8, T at 10 11
               (1, 0, 7, "low", "+")]     # T at 0 1 5 (lower case folded)
    records = [(0, 0, "10M", "ACTCGTCAAC", None, False),          # eligible 1 2 5 6, conversions at 1 and 6
               (0, 4, "2S6M", "GGGCTAAC", "III;<III", False),     # the C over the T at 5 has quality 26: not eligible; the T at 6 has 27: eligible, no conversion
               (0, 7, "3M2D4M", "GACGGGT", None, True),           # reverse: eligible A at 7 8 14, conversions at 7 and 14; 10 and 11 are deleted
               (0, 18, "5M", "CGAAA", None, True),                # G over the A at 19, the contig's last base; the rest is clipped
               (1, 0, "7M", "CCAANNA", None, False)]              # conversions at 0 and 1; N over the T at 5: not eligible
    mask = {(0, 1), (0, 14), (0, 3)}                              # a T of u1, an A of u2, and a C, which no region sums anyway
    want = (M.HEADER +
            "chr1\t0\t10\tu1\t+\t3\t1\t4\t1\t2\t1\n"      # T 2 5 6 (1 is masked): cov 1 + 1 + 2, conv 1 at 6; two forward records, one with a conversion (masked or not)
            "chr1\t5\t20\tu2\t-\t3\t1\t3\t2\t2\t2\n"      # A 7 8 19 (14 is masked): cov 1 + 1 + 1, conv at 7 and 19; two reverse records, both with a conversion
            "chr1\t8\t12\tdot\t.\t3\t0\t1\t0\t3\t0\n"     # A 8, T 10 11: cov 1 at 8; three records have an M column in 8..11 (the third one's deletion does not count)
            "chr2\t0\t7\tlow\t+\t3\t0\t2\t2\t1\t1\n")
    assert M.count_file(contigs, records, regions, mask, 27).decode() == want
    assert M.tally(contigs, records, regions, mask, 27)[1] == dict(alignments=5, met_a_region=5, eligible_columns=11, conversions=7, masked_positions=3)
    # without the mask, and with a quality threshold that lets the second record's C count
    assert M.count_file(contigs, records, regions, set(), 26).decode().splitlines()[1:3] == ["chr1\t0\t10\tu1\t+\t4\t0\t6\t3\t2\t2", "chr1\t5\t20\tu2\t-\t4\t0\t4\t3\t2\t2"]
    sam = ["@SQ\tSN:chr1\tLN:20\n", "r\t0\tchr1\t3\t60\t5M\t*\t0\t0\tACGTA\tIIIII\n", "s\t256\tchr1\t3\t60\t5M\t*\t0\t0\tACGTA\t*\n", "u\t4\t*\t0\t0\t*\t*\t0\t0\tA\t*\n",
           "t\t16\tchr1\t9\t60\t2M\t*\t0\t0\tAC\t*\n", "m\t83\tchr1\t9\t60\t2M\t=\t1\t-10\tAC\t*\n"]
    assert M.records_of_sam(sam, contigs) == [(0, 2, "5M", "ACGTA", "IIIII", False), (0, 8, "2M", "AC", None, True), (0, 8, "2M", "AC", None, True)]
    assert M.mask_of_vcf("##fileformat=VCFv4.2\n#CHROM\tPOS\n\nchr2\t3\t.\tA\tG\nchr1\t20\t.\tA\tC\n", contigs) == {(1, 2), (0, 19)}


def test_the_unit_cases_decide_what_they_are_named_for():
    """the cases are only worth their names if the model's answers on them are the ones the names promise"""
    rows = lambda name: M.tally(*M.UNIT_CASES[name])[0]
    stats = lambda name: M.tally(*M.UNIT_CASES[name])[1]
    t_bases, masked, cov, conv, reads, tc = range(6)
    r = rows("crossing-start-and-end")[0]
    assert r[reads] == r[tc] == 3 and r[conv] == r[cov] == stats("crossing-start-and-end")["eligible_columns"] > 0
    assert stats("outside-every-region") == dict(alignments=4, met_a_region=0, eligible_columns=0, conversions=0, masked_positions=0)
    assert [x[reads] for x in rows("clipped-at-the-contigs-last-base")] == [2, 1]
    assert rows("spanning-with-a-deletion-only")[0][reads] == 1   # (the third record ends inside the region; the first two only span it)
    r = rows("operations-in-front-of-a-conversion")[0]
    assert r[reads] == r[tc] == 5 and r[conv] == r[cov] > 0
    r = rows("quality-just-below-and-at-q")[0]
    assert (r[reads], r[tc]) == (4, 3) and r[cov] == r[conv] == 3 * r[t_bases] - 2
    assert rows("quality-zero-counts-everything")[0][cov] == 2 * rows("quality-zero-counts-everything")[0][t_bases]
    r = rows("read-n-on-a-t")[0]
    assert r[cov] == 2 * r[t_bases] - 2 and r[tc] == 1
    assert rows("no-quality-string")[0][cov] == rows("no-quality-string")[0][t_bases] > 0
    r = rows("nested-and-repeated-regions")
    assert r[1] == r[3] and r[1][reads] == 2 and r[2][reads] == 2 and r[0][reads] == 3 and r[4][reads] == 1
    r = rows("opposite-strands-and-a-dot-region")
    assert r[2][reads] == 5 and r[0][reads] == 2 and r[1][reads] == 3
    r = rows("region-without-a-record-and-of-one-base")
    assert r[0][reads] == 0 and r[0][t_bases] > 0 and r[1][:4] == (1, 0, 3, 3) and r[2][:4] == (0, 0, 0, 0) and r[2][reads] == 3
    r = rows("contention")
    assert r[0][2:] == r[1][2:] == (700, 600, 700, 600)
    r = rows("mask-inside-outside-and-on-the-border")
    assert [x[masked] for x in r] == [3, 2, 5, 0] and stats("mask-inside-outside-and-on-the-border")["masked_positions"] == 9
    r = rows("a-masked-t-leaves-t-bases")[0]
    assert (r[masked], r[conv], r[tc]) == (1, 5, 5)   # (the other converted T counts; tc_reads does not know the mask)
    no_mask = M.tally(*M.UNIT_CASES["a-masked-t-leaves-t-bases"][:3], set(), 27)[0][0]
    assert no_mask[t_bases] == r[t_bases] + 1 and no_mask[conv] == 10


# ---- the driver ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """the stand-alone program, with AddressSanitizer and UndefinedBehaviorSanitizer in it"""
    out = str(tmp_path_factory.mktemp("count_driver") / "count_driver_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", out])
    return out


def _input(contigs, records, regions, mask, Q):
    return ("%d\n" % len(contigs) + "".join("%s %s\n" % (n, s or "-") for n, s in contigs) + "%d\n%d\n" % (Q, len(regions)) + "".join("%d %d %d %s %s\n" % r for r in regions) +
            "%d\n" % len(mask) + "".join("%d %d\n" % m for m in sorted(mask)) +
            "".join("%d %d %s %s %s %d\n" % (c, p, g or "-", s or "-", "*" if q is None else (q or "-"), int(r)) for c, p, g, s, q, r in records))


def _file(exe, case):
    r = subprocess.run([exe, "file"], input=_input(*case).encode(), capture_output=True, env=SAN_ENV)
    assert r.returncode == 0, (r.returncode, r.stderr.decode()[-3000:])
    at = r.stdout.rindex(b"stats ")
    return r.stdout[:at], dict(zip(M.STATS, (int(x) for x in r.stdout[at + 6:].split())))


@pytest.mark.parametrize("name", list(M.UNIT_CASES))
def test_driver_equals_the_model_on_the_unit_cases(exe, name):
    case = M.UNIT_CASES[name]
    rows, stats = M.tally(*case)
    text, st = _file(exe, case)
    assert text == M.tsv(case[0], case[2], rows)
    assert st == stats


@pytest.mark.parametrize("seed", [77, 78])
def test_driver_equals_the_model_on_random_records(exe, seed):
    case = M.random_case(seed, 4000)
    rows, stats = M.tally(*case)
    text, st = _file(exe, case)
    assert text == M.tsv(case[0], case[2], rows) and st == stats
    assert stats["conversions"] > 1000 and stats["masked_positions"] > 10 and sum(1 for r in rows if r[1] > 0) >= 5 and sum(1 for r in rows if r[5] > 0) >= 20
    # without a mask and with every quality counting
    loose = case[:3] + (set(), 0)
    text, st = _file(exe, loose)
    assert text == M.count_file(*loose) and st["eligible_columns"] > stats["eligible_columns"]


def test_the_drivers_bed_reader_equals_the_models(exe):
    head = "%d\n" % len(BED_CONTIGS) + "".join("%s %d\n" % (n, len(s)) for n, s in BED_CONTIGS)
    for name, (text, message) in BAD_BEDS.items():
        r = subprocess.run([exe, "bed"], input=(head + text).encode(), capture_output=True, env=SAN_ENV)
        assert r.returncode == 0 and r.stdout.decode() == "error " + message + "\n", (name, r.stdout, r.stderr[-2000:])
    r = subprocess.run([exe, "bed"], input=(head + GOOD_BED.replace("\t\t7", "\tx\t7")).encode(), capture_output=True, env=SAN_ENV)
    want = [(c, s, e, n or "x", d) for c, s, e, n, d in GOOD_REGIONS]
    assert r.returncode == 0 and r.stdout.decode() == "ok %d\n" % len(want) + "".join("%d %d %d %s %s\n" % x for x in want), (r.stdout, r.stderr[-2000:])
