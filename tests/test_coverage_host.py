"""No GPU: what `ngm-hip --coverage` refuses before any GPU work, the model of tests/coverage_model.py pinned on a file written out by
hand, and the host-only parts of the coverage (nextgenmap_amd/csrc/coverage.h: the CIGAR walk, the validator, the counter array's layout,
the line serialiser) through tests/cpp/coverage_driver.cpp, a stand-alone program built with g++ -fsanitize=address,undefined."""
import os
import random
import subprocess

import pytest

import coverage_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "nextgenmap_amd", "ngm-hip")
SRC = os.path.join(ROOT, "tests", "cpp", "coverage_driver.cpp")
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")


@pytest.mark.parametrize("extra,message", [
    (["--argos"], "--coverage cannot be combined with --argos"),
    (["--shard", "0/2"], "--coverage cannot be combined with --shard:"),
    (["--shard-output"], "--coverage cannot be combined with --shard-output"),
    (["SAME"], "--coverage cannot write to the -o/--output file"),
], ids=["argos", "shard", "shard-output", "same-file"])
def test_coverage_refuses_unsupported_combinations(tmp_path, extra, message):
    from nextgenmap_amd import build
    build.build()
    cov = str(tmp_path / "out.bedgraph")
    if extra == ["SAME"]:
        cov, extra = str(tmp_path / "out.sam"), []
    # (neither input exists: the refusal comes from the option check, before the reference or the reads are opened)
    r = subprocess.run([CLI, "-r", str(tmp_path / "none.fa"), "-q", str(tmp_path / "none.fq"), "-o", str(tmp_path / "out.sam"), "--coverage", cov] + extra,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert message in r.stderr, r.stderr
    assert not os.path.exists(tmp_path / "out.sam") and not os.path.exists(tmp_path / "out.bedgraph")
    assert "HIP backend (gfx950)" not in r.stderr + r.stdout and "index entries" not in r.stderr


def test_model_equals_a_hand_written_file():
    contigs = [("chr1", 30), ("chr2", 10)]
    alignments = [(0, 2, "5M"),          # [2, 7)
                  (0, 5, "2S3M2D4M1I2M"),  # [5, 8) and [10, 16)
                  (0, 28, "10M"),        # clipped to [28, 30)
                  (1, 0, "4=1X"),        # [0, 5): begins at the same depth the first contig ends with
                  (1, 5, "5M"),          # abuts: one run
                  (1, 3, "2M3N1M")]      # [3, 5) and [8, 9)
    assert M.bedgraph(contigs, alignments) == (b"chr1\t2\t5\t1\nchr1\t5\t7\t2\nchr1\t7\t8\t1\nchr1\t10\t16\t1\nchr1\t28\t30\t1\n"
                                               b"chr2\t0\t3\t1\nchr2\t3\t5\t2\nchr2\t5\t8\t1\nchr2\t8\t9\t2\nchr2\t9\t10\t1\n")
    assert M.totals(M.bedgraph(contigs, alignments)) == (10, 2, 3 + 4 + 1 + 6 + 2 + 3 + 4 + 3 + 2 + 1)
    sam = ["@SQ\tSN:chr1\tLN:30\n", "r\t0\tchr1\t3\t60\t5M\t*\t0\t0\tACGTA\t*\n", "s\t256\tchr1\t3\t60\t5M\t*\t0\t0\tACGTA\t*\n", "u\t4\t*\t0\t0\t*\t*\t0\t0\tA\t*\n",
           "t\t16\tchr1\t9\t60\t2M\t*\t0\t0\tAC\t*\n"]
    assert M.sam_contigs(sam) == [("chr1", 30)]
    assert M.alignments_of_sam(sam, [("chr1", 30)]) == [(0, 2, "5M"), (0, 8, "2M")]


# ---- the driver ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """the stand-alone program, with AddressSanitizer and UndefinedBehaviorSanitizer in it"""
    d = tmp_path_factory.mktemp("coverage_driver")
    out = str(d / "coverage_driver_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", out])
    return out, d


def _input(contigs, alignments):
    return "%d\n" % len(contigs) + "".join("%s %d\n" % c for c in contigs) + "".join("%d %d %s\n" % (c, p, g or "-") for c, p, g in alignments)


def _file(exe, contigs, alignments):
    prog, d = exe
    p = str(d / "case.txt")
    with open(p, "w") as f:
        f.write(_input(contigs, alignments))
    r = subprocess.run([prog, "file", p, p + ".out"], capture_output=True, text=True, env=SAN_ENV)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    covered, runs = (int(x) for x in r.stdout.split())
    return open(p + ".out", "rb").read(), covered, runs


@pytest.mark.parametrize("name", list(M.UNIT_CASES) + list(M.CHUNK_CASES))
def test_driver_equals_the_model_on_the_unit_cases(exe, name):
    contigs, alignments = {**M.UNIT_CASES, **M.CHUNK_CASES}[name]
    text, covered, runs = _file(exe, contigs, alignments)
    want = M.bedgraph(contigs, alignments)
    assert text == want
    assert (runs, covered) == (M.totals(want)[0], M.totals(want)[2])
    if name == "nothing":
        assert text == b""


def random_alignments(rnd, contigs, n):
    out = []
    for _ in range(n):
        c = rnd.randrange(len(contigs))
        ops = "".join("%d%s" % (rnd.choice([0, 1, 1, 2, 3, 7, 30, 200]), rnd.choice("MMMM=XIDNSHP")) for _ in range(rnd.randrange(0, 7)))
        out.append((c, rnd.randrange(0, contigs[c][1] + 20), ops))
    return out


def test_driver_equals_the_model_on_random_alignments(exe):
    contigs = [("one", 1), ("sixtyfour", 64), ("thousand", 1000)]
    alignments = random_alignments(random.Random(77), contigs, 4000)
    text, covered, _ = _file(exe, contigs, alignments)
    want = M.bedgraph(contigs, alignments)
    assert text == want and len(want) > 5000
    assert covered == M.totals(want)[2]


BAD = [((2, 0, "5M"), "its ref_id is not in [0, n_ref)"), ((-1, 0, "5M"), "its ref_id is not in [0, n_ref)"), ((0, -1, "5M"), "its position is negative"),
       ((0, 0, "5M3Q"), "unknown operation character"), ((0, 0, "*"), "unknown operation character"), ((0, 0, "5m"), "unknown operation character"),
       ((0, 0, "268435456M"), "overflows 2^28"), ((0, 0, "99999999999999999999999M"), "overflows 2^28"), ((0, 0, "M"), "operation without a number"),
       ((0, 0, "5MM"), "operation without a number"), ((0, 0, "5M3"), "number without an operation")]


def test_validator_refuses_every_malformed_input_with_its_message(exe):
    prog, d = exe
    good = [(0, 0, "268435455M"), (1, 49, "1M"), (0, 0, ""), (0, 2147483647, "3S5M")]
    p = str(d / "check.txt")
    with open(p, "w") as f:
        f.write(_input(M.TWO, [a for a, _ in BAD] + good))
    r = subprocess.run([prog, "check", p], capture_output=True, text=True, env=SAN_ENV)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(BAD) + len(good)
    for (a, msg), line in zip(BAD, lines):
        assert not line.startswith("0 ") and msg in line, (a, line)
    for a, line in zip(good, lines[len(BAD):]):
        assert line.startswith("0 "), (a, line)
