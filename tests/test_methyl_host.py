"""No GPU: what `ngm-hip --methyl` refuses before any GPU work, by message; the model of tests/methyl_model.py pinned on a report written out
by hand; and the host-only parts of the methylation counter (nextgenmap_amd/csrc/methyl.h: the walk of a record, the context of a site,
the serialiser) through tests/cpp/methyl_driver.cpp, a stand-alone program built with g++ -fsanitize=address,undefined and fed through its
standard input."""
import os
import subprocess

import pytest

import methyl_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "nextgenmap_amd", "ngm-hip")
SRC = os.path.join(ROOT, "tests", "cpp", "methyl_driver.cpp")
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")


def _cli(tmp_path, extra, methyl="out.CX_report.txt", bs=True):
    # (neither input exists: the refusal comes from the option check, before the reference or the reads are opened)
    return subprocess.run([CLI, "-r", str(tmp_path / "none.fa"), "-q", str(tmp_path / "none.fq"), "-o", str(tmp_path / "out.sam")] + (["--bs-mapping"] if bs else []) +
                          (["--methyl", str(tmp_path / methyl)] if methyl else []) + extra, capture_output=True, text=True, timeout=60)


def _refused(tmp_path, r, message):
    assert r.returncode != 0
    assert message in r.stderr, r.stderr
    assert [m for m in r.stderr.splitlines() if message in m][0].split(message)[1].strip()   # (a reason follows)
    assert not any(os.path.exists(tmp_path / n) for n in ("out.sam", "out.CX_report.txt", "both.txt"))
    assert "HIP backend (gfx950)" not in r.stderr + r.stdout and "index entries" not in r.stderr


@pytest.mark.parametrize("extra,message", [
    (["NO-BS-MAPPING"], "--methyl needs --bs-mapping: "),
    (["--argos"], "--methyl cannot be combined with --argos: "),
    (["--shard", "0/2"], "--methyl cannot be combined with --shard: "),
    (["--shard-output"], "--methyl cannot be combined with --shard-output: "),
    (["SAME-AS-OUTPUT"], "--methyl cannot be combined with -o "),
    (["SAME-AS-COVERAGE"], "--methyl cannot be combined with --coverage "),
], ids=["no-bs-mapping", "argos", "shard", "shard-output", "same-as-output", "same-as-coverage"])
def test_methyl_refuses_unsupported_combinations(tmp_path, extra, message):
    from nextgenmap_amd import build
    build.build()
    if extra == ["NO-BS-MAPPING"]:
        r = _cli(tmp_path, [], bs=False)
    elif extra == ["SAME-AS-OUTPUT"]:
        r = _cli(tmp_path, [], methyl="out.sam")
    elif extra == ["SAME-AS-COVERAGE"]:
        r = _cli(tmp_path, ["--coverage", str(tmp_path / "both.txt")], methyl="both.txt")
    else:
        r = _cli(tmp_path, extra)
    _refused(tmp_path, r, message)


@pytest.mark.parametrize("extra,message", [
    (["--methyl-context", "CG"], "--methyl-context expects all, CpG, CHG or CHH"),
    (["--methyl-context", "cpg"], "--methyl-context expects all, CpG, CHG or CHH"),
    (["--methyl-context", ""], "--methyl-context expects all, CpG, CHG or CHH"),
    (["--methyl-min-qual", "-1"], "--methyl-min-qual expects a Phred quality in 0..93"),
    (["--methyl-min-qual", "94"], "--methyl-min-qual expects a Phred quality in 0..93"),
    (["--methyl-min-qual", "high"], "--methyl-min-qual expects a Phred quality in 0..93"),
    (["--methyl-min-qual", ""], "--methyl-min-qual expects a Phred quality in 0..93"),
    (["--methyl-min-depth", "-1"], "--methyl-min-depth expects a count of 0 or more"),
    (["--methyl-min-depth", "3x"], "--methyl-min-depth expects a count of 0 or more"),
])
def test_methyl_refuses_a_bad_value(tmp_path, extra, message):
    from nextgenmap_amd import build
    build.build()
    r = _cli(tmp_path, extra)
    assert r.returncode != 0 and message in r.stderr, r.stderr
    assert not os.path.exists(tmp_path / "out.CX_report.txt") and not os.path.exists(tmp_path / "out.sam")
    assert "HIP backend (gfx950)" not in r.stderr + r.stdout and "index entries" not in r.stderr


@pytest.mark.parametrize("extra", [["--methyl-context", "CpG"], ["--methyl-min-qual", "10"], ["--methyl-min-depth", "2"]])
def test_the_methyl_options_need_methyl(tmp_path, extra):
    from nextgenmap_amd import build
    build.build()
    _refused(tmp_path, _cli(tmp_path, extra, methyl=None), "--methyl-context, --methyl-min-qual and --methyl-min-depth need --methyl FILE: ")


# ---- the model, by hand ---------------------------------------------------------------------------------------------------------------
def test_model_equals_a_hand_written_report():
    #                    0123456789012
    contigs = [("chr1", "ACGTTCAGGCNCC"), ("chr2", "Gtcc")]
    # sites of chr1: C1 (CG: n1 = G), G2 (-: n1 = comp(C) = G: CG), C5 (CAG: CHG), G7 (-: comp(A) = T, comp(C) = G: CHG), G8 (-: comp(G) = C,
    # comp(A) = T: CHH), C9 (n1 = N: CN), C11 (C, then outside: CHN), C12 (outside at once: CN); chr2: G0 (-: outside: CN), C2 (C, outside: CHN), C3 (CN)
    records = [(0, 0, "13M", "ACGTTTAGGCNCC", None, False),            # top: C1 meth, C5 unmeth (T), C9 C11 C12 meth; its Gs say nothing
               (0, 0, "13M", "ATGTTCAAGTNCC", "IIIIIIIIIII&%", False),  # top: C1 unmeth, C5 meth, C9 unmeth, C11 at Phred 5 meth, C12 at Phred 4 nothing
               (0, 1, "2S7M", "TTCATTCAA", None, True),                # bottom over 1..7: its C over C1 and C5 says nothing; G2 and G7 read as A: unmeth; G8 is not reached
               (1, 0, "4M", "GTCC", None, True),                       # bottom: G0 meth; the Cs say nothing
               (1, 0, "1M1D2M", "ACT", None, False)]                   # top: the A over G0 says nothing; 1 is deleted; C2 meth, C3 unmeth
    text, totals = M.report(contigs, records)
    want = ("chr1\t2\t+\t1\t1\tCG\tCGT\n"
            "chr1\t3\t-\t0\t1\tCG\tCGT\n"
            "chr1\t6\t+\t1\t1\tCHG\tCAG\n"
            "chr1\t8\t-\t0\t1\tCHG\tCTG\n"
            "chr1\t10\t+\t1\t1\tCN\tCNC\n"
            "chr1\t12\t+\t2\t0\tCHN\tCCN\n"
            "chr1\t13\t+\t1\t0\tCN\tCNN\n"
            "chr2\t1\t-\t1\t0\tCN\tCNN\n"
            "chr2\t3\t+\t1\t0\tCHN\tCCN\n"
            "chr2\t4\t+\t0\t1\tCN\tCNN\n")
    assert text.decode() == want
    assert totals == dict(alignments=5, lines=10, cpg_meth=1, cpg_unmeth=2, chg_meth=1, chg_unmeth=2, chh_meth=0, chh_unmeth=0)
    assert M.report(contigs, records, context="CpG")[0].decode() == "".join(l for l in want.splitlines(True) if "\tCG\t" in l)
    assert M.report(contigs, records, N=2)[0].decode() == "".join(l for l in want.splitlines(True) if "\t1\t1\t" in l or "\t2\t0\t" in l)
    assert M.report(contigs, records, Q=6)[0].decode() == want.replace("chr1\t12\t+\t2\t0", "chr1\t12\t+\t1\t0")
    sam = ["@SQ\tSN:chr1\tLN:13\n", "r\t0\tchr1\t3\t60\t5M\t*\t0\t0\tACGTA\tIIIII\tAS:i:1\tZS:Z:++\tXI:f:1\n", "s\t256\tchr1\t3\t60\t5M\t*\t0\t0\tACGTA\t*\tZS:Z:++\n",
           "u\t4\t*\t0\t0\t*\t*\t0\t0\tA\t*\n", "t\t16\tchr1\t9\t60\t2M\t*\t0\t0\tAC\t*\tZS:Z:-+\n", "m\t147\tchr1\t9\t60\t2M\t=\t1\t-10\tAC\t*\tZS:Z:+-\n",
           "n\t163\tchr1\t1\t60\t2M\t=\t9\t10\tAC\t*\tZS:Z:--\n"]
    assert M.records_of_sam(sam, contigs) == [(0, 2, "5M", "ACGTA", "IIIII", False), (0, 8, "2M", "AC", None, True), (0, 8, "2M", "AC", None, False), (0, 0, "2M", "AC", None, True)]
    assert M.bam_tags(b"ASi\x05\0\0\0NMC\x01ZSZ-+\0XIf\0\0\x80\x3fMDZ10\0") == dict(AS=5, NM=1, ZS="-+", XI=1.0, MD="10")


def test_the_unit_cases_decide_what_they_are_named_for():
    """the cases are only worth their names if the model's answers on them are the ones the names promise"""
    rows = lambda name, **kw: M.parse_report(M.report(*M.UNIT_CASES[name][:2], **{k: v for k, v in dict(M.UNIT_CASES[name][2], **kw).items() if k != "scan_chunk"})[0])
    r = rows("top-and-bottom-over-the-same-c-and-g")
    assert {x[2] for x in r} == {"+", "-"} and any(x[3] and x[4] for x in r if x[2] == "+") and any(x[3] and x[4] for x in r if x[2] == "-")
    assert rows("ignored-bases") and all(x[3] + x[4] == 1 for x in rows("ignored-bases"))   # (a record's own strand: one call per site it leaves alone)
    by = {(x[0], x[1]): x for x in rows("contig-seam")}
    assert by[("c0", 12)][5:] == ("CN", "CNN") and by[("c0", 11)][5:] == ("CHN", "CCN") and by[("c1", 1)][5:] == ("CN", "CNN") and by[("c1", 2)][5:] == ("CHN", "CCN")
    assert by[("c3", 1)][5:] == ("CG", "CGN") and by[("c3", 2)][5:] == ("CG", "CGN")
    r = rows("n-neighbour-and-lower-case")
    assert {"CN", "CHN", "CG"} <= {x[5] for x in r} and all(x[0] == "low" for x in r) and any(x[1] <= 4 for x in r)
    r = rows("cigar-with-insert-deletion-and-soft-clips")
    assert any(x[3] for x in r) and any(x[4] for x in r) and not any(x[1] - 1 in (27, 28) and x[2] == "+" and x[3] for x in r)
    assert max(x[1] for x in rows("hanging-over-the-contigs-end")) == 70
    a, b = rows("quality-at-q-and-one-below"), rows("quality-threshold-13")
    assert sum(x[3] + x[4] for x in a) > sum(x[3] + x[4] for x in b) > 0 and a != rows("quality-at-q-and-one-below", Q=4) and a != rows("quality-at-q-and-one-below", Q=6)
    assert rows("no-quality-string") and len(rows("no-quality-string")) == len(rows("no-quality-string", Q=0))
    deep = rows("min-depth-3")
    assert deep and all(x[3] + x[4] >= 3 for x in deep) and {2, 3} <= {x[3] + x[4] for x in rows("min-depth-0-is-1")} and rows("min-depth-0-is-1") == rows("min-depth-3", N=1)
    assert {x[5] for x in rows("context-all")} == {"CG", "CHG", "CHH", "CN", "CHN"}
    assert all({x[2] for x in rows("context-all") if x[5] == ctx} == {"+", "-"} for ctx in ("CG", "CHG", "CHH", "CN", "CHN"))
    for name, ctx in (("CpG", "CG"), ("CHG", "CHG"), ("CHH", "CHH")):
        assert rows("context-" + name) == [x for x in rows("context-all") if x[5] == ctx] != []
    totals = [M.report(*M.UNIT_CASES["context-" + n][:2], context=n)[1] for n in M.SELECTS]
    assert all({k: v for k, v in t.items() if k != "lines"} == {k: v for k, v in totals[0].items() if k != "lines"} for t in totals) and all(totals[0][k] > 0 for k in M.STATS)
    assert {7, 0} <= {(x[1] - 1) % 8 for x in rows("packed-word-border")}
    assert sum(1 for x in rows("scan-chunk-64") if x[0] == "l") > 64 and {"l", "m"} == {x[0] for x in rows("scan-chunk-64")}


# ---- the driver ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """the stand-alone program, with AddressSanitizer and UndefinedBehaviorSanitizer in it"""
    out = str(tmp_path_factory.mktemp("methyl_driver") / "methyl_driver_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", out])
    return out


def _input(contigs, records, params):
    return ("%d\n" % len(contigs) + "".join("%s %s\n" % (n, s or "-") for n, s in contigs) + "%d %d %s\n" % (params["Q"], params["N"], params["context"]) +
            "".join("%d %d %s %s %s %d\n" % (c, p, g or "-", s or "-", "*" if q is None else (q or "-"), int(b)) for c, p, g, s, q, b in records))


def _file(exe, case):
    r = subprocess.run([exe, "file"], input=_input(*case).encode(), capture_output=True, env=SAN_ENV)
    assert r.returncode == 0, (r.returncode, r.stderr.decode()[-3000:])
    at = r.stdout.rindex(b"stats ")
    return r.stdout[:at], dict(zip(M.STATS, (int(x) for x in r.stdout[at + 6:].split())))


def _want(case):
    contigs, records, params = case
    return M.report(contigs, records, params["Q"], params["N"], params["context"])


@pytest.mark.parametrize("name", list(M.UNIT_CASES))
def test_driver_equals_the_model_on_the_unit_cases(exe, name):
    case = M.UNIT_CASES[name]
    assert _file(exe, case) == _want(case)


def test_driver_equals_the_model_on_random_records(exe):
    case = M.random_case(78, 3000)
    text, totals = _want(case)
    assert _file(exe, case) == (text, totals)
    rows = M.parse_report(text)
    for strand in "+-":
        assert sum(x[3] for x in rows if x[2] == strand) >= 1000 and sum(x[4] for x in rows if x[2] == strand) >= 1000
    assert all(sum(1 for x in rows if x[5] == ctx) >= 50 for ctx in ("CG", "CHG", "CHH"))
    for params in (dict(case[2], context="CHG", N=3), dict(case[2], Q=0), dict(case[2], Q=41)):
        loose = case[:2] + (params,)
        assert _file(exe, loose) == _want(loose)
