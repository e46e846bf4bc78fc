"""-m gpu: `ngm-hip --bs-mapping --methyl` and the methylation counter behind it (include/ngm_pipeline.h, ngm_methyl_*).  Unit cases through
the ctypes mirror, no genome and no mapper, each compared byte for byte with tests/methyl_model.py; then the command line on a random 60 kb
genome whose cytosines carry a planted methylation state, where the report must equal the model applied to the SAM / BAM file of the same
run and the FASTA, and must show the planted states."""
import os
import random
import re
import subprocess
import threading

import numpy as np
import pytest

import methyl_model as M
import simulate as S
from test_coverage_host import BAD as COVERAGE_BAD
from test_snp_host import BAD as SNP_BAD

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "nextgenmap_amd", "ngm-hip")


def _counter(case):
    from nextgenmap_amd.pipeline import MethylationCounter
    contigs, _, p = case
    return MethylationCounter(contigs, 0, p["Q"], p["N"], p["context"], p["scan_chunk"])


def _add(c, records):
    """(one call takes records that all have a quality string, or none of them)"""
    for part in ([r for r in records if r[4] is None], [r for r in records if r[4] is not None]):
        if part:
            c.add(part)


def _finish(c):
    c.finish()
    text = c.text()
    st = c.stats()
    return text, {k: st[k] for k in M.STATS}


def _want(case):
    contigs, records, p = case
    return M.report(contigs, records, p["Q"], p["N"], p["context"])


# ---- unit cases ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(M.UNIT_CASES))
def test_unit_case_equals_the_model(name):
    case = M.UNIT_CASES[name]
    c = _counter(case)
    try:
        _add(c, case[1])
        assert _finish(c) == _want(case)
    finally:
        c.close()


def test_the_text_comes_in_whole_lines_whatever_the_buffer():
    case = M.UNIT_CASES["scan-chunk-64"]
    c = _counter(case)
    _add(c, case[1])
    c.finish()
    pieces = list(c.pieces(40))   # (smaller than two lines)
    assert b"".join(pieces) == _want(case)[0] and len(pieces) > 20 and all(p.endswith(b"\n") for p in pieces)
    c.close()


@pytest.fixture(scope="module")
def randoms():
    case = M.random_case(78, 3000)
    return case, _want(case)


def test_random_records_equal_the_model(randoms):
    case, want = randoms
    c = _counter(case)
    _add(c, case[1])
    assert _finish(c) == want
    rows = M.parse_report(want[0])
    for strand in "+-":
        assert sum(x[3] for x in rows if x[2] == strand) >= 1000 and sum(x[4] for x in rows if x[2] == strand) >= 1000
    assert all(sum(1 for x in rows if x[5] == ctx) >= 50 for ctx in ("CG", "CHG", "CHH"))
    st = c.stats()
    assert st["add_ms"] > 0 and st["flag_ms"] > 0 and st["text_ms"] > 0
    c.close()


def test_one_call_and_seven_calls_from_three_threads_give_the_same_bytes(randoms):
    case, want = randoms
    order = list(case[1])
    random.Random(5).shuffle(order)
    parts = [order[k::7] for k in range(7)]
    c = _counter(case)
    errors = []

    def work(mine):
        try:
            for p in mine:
                _add(c, p)
        except Exception as e:   # (a failed add must fail the test, not only its thread)
            errors.append(e)

    threads = [threading.Thread(target=work, args=(parts[t::3],)) for t in range(3)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors
    assert _finish(c) == want
    c.close()


# every record ngm_coverage_add refuses (those checks come first, whatever the sequence), then the ones only ngm_snp_add refuses
ALL_BAD = [((c, p, g, "ACGTA", None), msg) for (c, p, g), msg in COVERAGE_BAD] + SNP_BAD


@pytest.mark.parametrize("k", range(len(ALL_BAD)))
def test_add_refuses_a_bad_record_by_its_index_and_adds_nothing(k):
    from nextgenmap_amd.engine import NgmHipError
    from nextgenmap_amd.pipeline import MethylationCounter
    bad, message = ALL_BAD[k]
    contigs = [("chrA", "ACGT" * 25), ("chrB", "TCAGA" * 10)]   # (the two contigs of 100 and 50 bases the bad records are written for)
    good = [M.rec(contigs, 0, 10, "20M", False, meth=set(range(0, 100, 8))), M.rec(contigs, 1, 5, "10M3D10M", True, meth=set(range(0, 50, 10)))]
    c = MethylationCounter(contigs, 0)
    c.add(good)
    batch = [M.rec(contigs, 0, 0, "50M"), M.rec(contigs, 1, 0, "50M", True), M.rec(contigs, 0, 30, "5M", True)]
    batch.insert(2, tuple(bad) + (False,))
    with_q = bad[4] is not None
    if with_q:   # (a call's records all have qualities or none has: the quality text is one string under the sequences' offsets)
        batch = [r[:4] + ("I" * len(r[3]), r[5]) for r in batch[:2]] + [tuple(bad) + (False,)]
    b = lambda x: x.encode()
    off = np.concatenate(([0], np.cumsum([len(r[2]) for r in batch]))).astype(np.uint32)
    soff = np.concatenate(([0], np.cumsum([len(r[3]) for r in batch]))).astype(np.uint32)
    with pytest.raises(NgmHipError) as e:
        c.add_arrays([r[0] for r in batch], [r[1] for r in batch], off, b("".join(r[2] for r in batch)), soff, b("".join(r[3] for r in batch)),
                     b("".join(r[4] for r in batch)) if with_q else None, [int(r[5]) for r in batch])
    assert "ngm_methyl_add: alignment 2:" in str(e.value) and message in str(e.value)
    want = M.report(contigs, good)
    assert _finish(c) == want and want[1]["lines"] > 5   # nothing of the refused call was added
    with pytest.raises(NgmHipError):
        c.add(good)   # after the finish
    c.close()


def test_bad_parameters_are_refused():
    from nextgenmap_amd.engine import NgmHipError
    from nextgenmap_amd.pipeline import MethylationCounter
    contigs = [("chrA", "ACGT" * 25)]
    for kw in (dict(min_qual=94), dict(min_qual=-1), dict(min_depth=-1), dict(context="CG"), dict(context="")):
        with pytest.raises(NgmHipError):
            MethylationCounter(contigs, 0, **kw)


# ---- the command line ---------------------------------------------------------------------------------------------------------------
def _hip(args):
    c = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=120)   # (a run takes 1-2 s)
    assert c.returncode == 0, "returncode=%d\n%s" % (c.returncode, c.stderr[-2500:])
    return c.stderr


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """A seeded random genome of 60 001 bases in three contigs, 300 of them a copy of 300 others.  Every cytosine of either strand (a C, or
    a G of the FASTA) carries a fixed state from a seeded draw, methylated with probability 0.5 whatever its context (the copy has the
    original's states), so that the reads stay half converted and map.  4 000
    single-end reads and 2 000 pairs (fragments of 260..340 bases) of 100 bases, error-free, from both strands: the fragment is cut from
    its strand, its unmethylated Cs become T, the first mate (or the single read) is its first 100 bases as sequenced, the second mate the
    reverse complement of its last 100.  The runs are kept."""
    d = tmp_path_factory.mktemp("methyl")
    rng = np.random.default_rng(4711)
    contigs = [S.ACGT[rng.integers(0, 4, n)] for n in (25000, 20000, 15001)]
    state = [rng.random(len(g)) < 0.5 for g in contigs]   # True: the cytosine at this position (of the strand that has one) is methylated
    contigs[1][1000:1300], state[1][1000:1300] = contigs[0][5000:5300], state[0][5000:5300]   # one exact repeat, states included: reads with two places
    fa = str(d / "ref.fa")
    S.write_fasta(fa, contigs)

    def fragment(length):
        c = int(rng.integers(0, 3))
        p = int(rng.integers(0, len(contigs[c]) - length))
        top = contigs[c][p:p + length].copy()
        meth = state[c][p:p + length]
        if rng.random() < 0.5:   # the top strand: its unmethylated Cs are read as T
            top[(top == ord("C")) & ~meth] = ord("T")
            return top
        top[(top == ord("G")) & ~meth] = ord("A")   # the bottom strand's unmethylated Cs, in the top strand's letters
        return S.revcomp(top)

    qual = lambda i: bytes(33 + 20 + (7 * j + i) % 21 for j in range(100))
    se = [(b"s%d" % i, fragment(100).tobytes(), qual(i)) for i in range(4000)]
    pe = []
    for i in range(2000):
        f = fragment(int(rng.integers(260, 341)))
        pe += [(b"p%d/1" % i, f[:100].tobytes(), qual(i)), (b"p%d/2" % i, S.revcomp(f[-100:]).tobytes(), qual(i + 1))]
    files = {}
    for tag, reads in (("se", se), ("pe", pe)):
        files[tag] = str(d / (tag + ".fq"))
        with open(files[tag], "wb") as f:
            f.write(b"".join(b"@" + n + b"\n" + s + b"\n+\n" + q + b"\n" for n, s, q in reads))
    return d, fa, files, {}, (contigs, state)


def _run(world, reads, opts, methyl_opts=()):
    """-> (output file, report file, log)"""
    d, fa, files, cache, _ = world
    key = (reads, tuple(opts), tuple(methyl_opts))
    if key not in cache:
        out = str(d / ("out%d.%s" % (len(cache), "bam" if "-b" in opts else "sam")))
        rep = str(d / ("out%d.CX_report.txt" % len(cache)))
        log = _hip(["-r", fa, "-o", out, "--bs-mapping"] + (["-p"] if reads == "pe" else []) + ["-q", files[reads]] + list(opts) + ["--methyl", rep] + list(methyl_opts))
        cache[key] = (out, rep, log)
    return cache[key]


CLI_CASES = {
    "se-sam": ("se", []),
    "pe-sorted-bam": ("pe", ["-b", "--sort"]),
    "se-topn-2": ("se", ["-n", "2"]),   # (the host formats the records: the formatter's accumulator)
}
_TOTALS = re.compile(r"\[METHYL\] CpG (\d+) methylated, (\d+) unmethylated \(([0-9.]+)%\); CHG (\d+), (\d+) \(([0-9.]+)%\); CHH (\d+), (\d+) \(([0-9.]+)%\)")


def _log_totals(log):
    m = _TOTALS.search(log)
    assert m, log[-2000:]
    return [int(m.group(k)) for k in (1, 2, 4, 5, 7, 8)], [float(m.group(k)) for k in (3, 6, 9)]


@pytest.mark.parametrize("case", list(CLI_CASES))
def test_report_equals_the_model_over_the_file_the_run_wrote(world, case):
    """and shows the planted states.  Measured on an MI355X, the share of lines that are not pure or do not show the planted state:
    se-sam 0 of 28 507 lines, pe-sorted-bam 0 of 28 596, se-topn-2 0 of 28 507 (the cap of 1 % is for misplaced reads, not a measurement)."""
    reads, opts = CLI_CASES[case]
    out, rep, log = _run(world, reads, opts)
    text = open(rep, "rb").read()
    want, totals = M.from_run(out, world[1])
    assert text == want
    sums, percent = _log_totals(log)
    assert sums == [totals[k] for k in M.STATS[2:]]
    assert all(abs(p - 100.0 * sums[2 * k] / (sums[2 * k] + sums[2 * k + 1])) < 0.006 for k, p in enumerate(percent))
    assert "[MAIN] Methylation on the GPU: %d alignments, %d lines; kernels: add " % (totals["alignments"], totals["lines"]) in log
    print([l for l in log.splitlines() if "Methylation on the GPU" in l][0])
    assert "[MAIN] Methylation counters: " in log and "(8 bytes per base of the reference, held for the whole run)" in log
    # the truth
    contigs, state = world[4]
    rows = M.parse_report(text)
    names = {"chr%d" % (k + 1): k for k in range(3)}
    assert len(rows) >= 20000
    for strand in "+-":
        assert sum(1 for x in rows if x[2] == strand) >= 0.4 * len(rows)
    good = sum(1 for x in rows if (x[3] == 0 or x[4] == 0) and (x[3] > 0) == bool(state[names[x[0]]][x[1] - 1]))
    print("%s: %d lines, %d pure and as planted: %.3f %% are not" % (case, len(rows), good, 100.0 * (len(rows) - good) / len(rows)))
    assert good >= 0.99 * len(rows)
    assert all(chr(contigs[names[x[0]]][x[1] - 1]) == ("C" if x[2] == "+" else "G") for x in rows)
    if case == "se-topn-2":   # the host route: secondary records are written and do not count
        assert any(int(l.split("\t")[1]) & 0x100 for l in open(out) if not l.startswith("@"))
    if case == "pe-sorted-bam":   # second mates of both strands were there
        from test_gpu_bam import decode_bam
        tags = {M.bam_tags(r["tags"])["ZS"] for r in decode_bam(out)[2] if not r["flag"] & 0x104}
        assert tags == {"++", "-+", "+-", "--"}


def test_cpg_at_depth_3_equals_the_model_and_the_totals_are_those_of_all(world):
    out, rep, log = _run(world, "se", [], ["--methyl-context", "CpG", "--methyl-min-depth", "3"])
    want, totals = M.from_run(out, world[1], N=3, context="CpG")
    text = open(rep, "rb").read()
    assert text == want
    rows = M.parse_report(text)
    assert len(rows) > 500 and all(x[5] == "CG" and x[3] + x[4] >= 3 for x in rows)
    assert _log_totals(log) == _log_totals(_run(world, "se", [])[2])
    assert _log_totals(log)[0] == [totals[k] for k in M.STATS[2:]]


def test_report_does_not_depend_on_batches_and_workers(world):
    a = _run(world, "se", [])
    b = _run(world, "se", ["--batch-size", "900", "--workers", "3"])
    assert open(a[1], "rb").read() == open(b[1], "rb").read()


def test_output_is_the_same_with_and_without_the_option(world):
    d, fa, files, _, _ = world
    body = lambda p: [l for l in open(p) if not l.startswith("@PG")]
    with_methyl = _run(world, "se", [])[0]
    without = str(d / "plain.sam")
    log0 = _hip(["-r", fa, "-o", without, "--bs-mapping", "-q", files["se"]])
    assert body(with_methyl) == body(without) and len(body(without)) > 4000
    assert "Methylation" not in log0 and "[METHYL]" not in log0
