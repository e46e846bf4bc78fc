"""CPU-only: `-5/--trim5` and `--max-polya` (csrc/read_trim.h, the one place every input route of `ngm-hip` trims a read) against the
records the REAL reference program wrote for the fixtures of tests/make_trim_goldens.py with `-5 12 --max-polya 4`
(tests/golden/trim/*.sam.gz): every read's bases, quality string, poly-A count and whether it is discarded; the same rules with
other settings on the cases whose answer follows from src/parser/IParser.h:70-100 and src/ReadProvider.cpp:428-443; and what the
command line accepts and refuses before any GPU work."""
import gzip
import os
import subprocess

import pytest

import make_trim_goldens as TG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "nextgenmap_amd", "ngm-hip")
COMP = bytes.maketrans(b"ACGTN", b"TGCAN")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("read_trim") / "read_trim_driver")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "read_trim_driver.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def fastq(tmp_path_factory):
    d = tmp_path_factory.mktemp("trim_fq")
    out = {}
    for tag in ("se", "pe"):
        out[tag] = str(d / (tag + ".fq"))
        with open(out[tag], "wb") as f:
            f.write(gzip.open(os.path.join(TG.GOLDEN, tag + ".fq.gz"), "rb").read())
    return out


def run_driver(driver, fq, trim5, max_polya, q):
    r = subprocess.run([driver, fq, str(trim5), str(max_polya), str(q)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rows = [l.split("\t") for l in r.stdout.split("\n")[:-1]]
    return [(n, s, ql, int(a), int(d)) for n, s, ql, a, d in rows]


def qry_max_len(reads, trim5):
    """the estimation pass (src/ReadProvider.cpp:204-304): lengths behind the -5 prefix, BEFORE --max-polya; a read the prefix swallows counts as 1"""
    m = max(min(len(s) - trim5, 9999) if len(s) > trim5 else 1 for _, s, _ in reads if len(s))
    return min(1000, (m | 1) + 1)


def model(seq, qual, trim5, max_polya, q):
    """the two rules restated: -> (bases, quality, polyA, discarded)"""
    if len(seq) <= trim5:
        return "N", "*", 0, 1
    s = "".join(c if c in "ACGT" else "N" for c in seq[trim5:].upper())[:q - 1]
    ql = qual[trim5:] if len(qual) > trim5 else ""
    cut = len(s) - len(s.rstrip("A"))
    if max_polya < 0 or cut <= max_polya:
        cut = 0
    s = s[:len(s) - cut]
    return s, (ql[:len(s)] if ql else "*"), cut, 0


@pytest.mark.parametrize("tag", ["se", "pe"])
def test_trimmed_reads_equal_the_reference_programs_records(driver, fastq, tag):
    reads = TG.read_fastq_gz(os.path.join(TG.GOLDEN, tag + ".fq.gz"))
    q = qry_max_len(reads, 12)
    assert q == (1000 if tag == "se" else 102)   # (se: the read `long` is cut at qry_max_len - 1 = 999 bases)
    got = run_driver(driver, fastq[tag], 12, 4, q)
    assert [g[0] for g in got] == [r[0] for r in reads]
    golden = TG.sam_records(os.path.join(TG.GOLDEN, tag + ".sam.gz"))
    checked = trimmed = discarded = 0
    for i, (name, seq, qual, polya, disc) in enumerate(got):
        if tag == "pe":
            key, mate = (name[:-2], 0x40 if i % 2 == 0 else 0x80), got[i ^ 1]
        else:
            key, mate = (name, 0), None
        gone = bool(disc) or bool(mate and mate[4])   # (a pair goes with either mate: GenericReadWriter.h:250-252)
        assert (key not in golden) == gone, (name, disc)
        discarded += disc
        if gone:
            continue
        f = golden[key].rstrip("\n").split("\t")
        s, ql = f[9], f[10]
        if int(f[1]) & 16:
            s, ql = s.encode().translate(COMP)[::-1].decode(), (ql if ql == "*" else ql[::-1])
        xa = [x for x in f[11:] if x.startswith("XA:i:")]
        assert len(xa) == 1, golden[key]   # on EVERY record once --max-polya is given, 0 included
        assert (seq, qual, polya) == (s, ql, int(xa[0][5:])), (name, golden[key])
        checked += 1
        trimmed += polya > 0
    print(tag, "reads compared:", checked, "with a tail cut:", trimmed, "discarded:", discarded)
    assert checked >= (300 if tag == "se" else 395) and trimmed >= 100 and discarded == (2 if tag == "se" else 1)
    if tag == "se":
        by = {g[0]: g for g in got}
        assert by["all_a"][1:] == ("", "", 100, 0) and by["left5"][1:4:2] == ("CGTAC", 60)
        assert by["tail_n"][1].endswith("AAAAN") and by["tail_n"][3] == 6 and by["tail_lower"][3] == 10
        assert (len(by["left13"][1]), len(by["left14"][1])) == (13, 14) and by["short"][4] == by["exact"][4] == 1
        assert by["long"][1] == "N" * 999 and by["long"][3] == 0
        # tails of 4 bases or fewer stay (XA:i:0), longer ones go whole (an A of the genome in front of a tail belongs to it)
        assert all(g[3] == 0 or g[3] > 4 for g in got) and sum(1 for g in got[:296] if g[3] == 0) >= 100
        assert all(g[3] >= TG.TAILS[i % 6] for i, g in enumerate(got[:296]) if TG.TAILS[i % 6] > 4)


@pytest.mark.parametrize("trim5,max_polya", [(0, 0), (12, -1), (0, -1), (12, 4), (5, 30)])
def test_other_settings_follow_the_rules(driver, fastq, trim5, max_polya):
    reads = TG.read_fastq_gz(os.path.join(TG.GOLDEN, "se.fq.gz"))
    q = qry_max_len(reads, trim5)
    got = run_driver(driver, fastq["se"], trim5, max_polya, q)
    want = [(n,) + model(s.decode(), ql.decode(), trim5, max_polya, q) for n, s, ql in reads]
    assert got == want
    by = {g[0]: g for g in got}
    ad = TG.ADAPTER.decode()
    if (trim5, max_polya) == (0, 0):   # no prefix, every tail goes: `short` (ACGTTGCA) is a read and loses its last base
        assert by["all_a"][1:] == (ad, by["all_a"][2], 100, 0) and len(by["all_a"][2]) == 12
        assert by["short"][1:] == ("ACGTTGC", by["short"][2], 1, 0) and by["exact"][1] == ad and by["left5"][1] == ad + "CGTAC"
    if (trim5, max_polya) == (12, -1):   # the prefix alone: nothing cut, no count, the all-A read keeps its 100 bases
        assert by["all_a"][1:] == ("A" * 100, by["all_a"][2], 0, 0) and len(by["all_a"][2]) == 100
        assert by["short"][4] == by["exact"][4] == 1 and all(g[3] == 0 for g in got)
    if (trim5, max_polya) == (0, -1):
        assert all(g[4] == 0 and g[3] == 0 for g in got) and by["short"][1] == "ACGTTGCA"


def _cli(args):
    from nextgenmap_amd import build
    build.build()
    return subprocess.run([CLI] + args, capture_output=True, text=True)


def test_negative_trim5_is_refused(tmp_path):
    r = _cli(["-r", str(tmp_path / "none.fa"), "-q", str(tmp_path / "none.fq"), "-o", str(tmp_path / "out.sam"), "-5", "-1"])
    assert r.returncode != 0 and "-5/--trim5" in r.stderr, r.stderr
    assert not os.path.exists(tmp_path / "out.sam")


@pytest.mark.parametrize("other", ["--argos", "--vcf"])
def test_max_polya_with_argos_or_vcf_is_refused_before_any_gpu_work(tmp_path, other):
    extra = [other] + ([str(tmp_path / "none.vcf")] if other == "--vcf" else [])
    r = _cli(["-r", str(tmp_path / "none.fa"), "-q", str(tmp_path / "none.fq"), "-o", str(tmp_path / "out.sam"), "--max-polya", "4"] + extra)
    assert r.returncode != 0 and "cannot be combined with --max-polya" in r.stderr and other in r.stderr, r.stderr
    assert "HIP backend (gfx950)" not in r.stderr, "refused while the options are parsed: no reference, no device"
    assert not os.path.exists(tmp_path / "out.sam")


def test_slamdunk_short_options_are_accepted(tmp_path):
    """`-b`, `-d <char>`, `-5`, `--max-polya`: with a reference that does not exist the run fails ON THE REFERENCE, not on an option"""
    r = _cli(["-r", str(tmp_path / "none.fa"), "-q", str(tmp_path / "none.fq"), "-o", str(tmp_path / "out.bam"), "-b", "-d", "_", "-5", "12", "--max-polya", "4",
              "--slam-seq", "2", "-l", "--rg-id", "s", "--rg-sm", "s:pulse:0", "-n", "1", "--strata", "-t", "1", "--no-progress"])
    assert r.returncode != 0
    assert "unknown option" not in r.stderr and "expects" not in r.stderr and "cannot be combined" not in r.stderr, r.stderr
    assert "cannot open reference" in r.stderr and "none.fa" in r.stderr, r.stderr
