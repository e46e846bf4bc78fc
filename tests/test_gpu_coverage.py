"""-m gpu: `ngm-hip --coverage` and the coverage object behind it (include/ngm_pipeline.h, ngm_coverage_*).  Unit cases through the ctypes
mirror, no genome and no mapper, each compared byte for byte with tests/coverage_model.py; then the command line on a 700 kb genome, where
the bedGraph must equal the model applied to the SAM / BAM file the same run wrote."""
import os
import random
import subprocess
import threading

import numpy as np
import pytest

import coverage_model as M
import simulate as S
from test_coverage_host import BAD, random_alignments
from test_gpu_bam import decode_bam

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "nextgenmap_amd", "ngm-hip")


def _coverage(contigs, scan_chunk=0):
    from nextgenmap_amd.pipeline import Coverage
    return Coverage(contigs, 0, scan_chunk)


def _text(contigs, alignments, scan_chunk=0, cap=1 << 20):
    c = _coverage(contigs, scan_chunk)
    try:
        if alignments:
            c.add(alignments)
        c.finish()
        return b"".join(c.pieces(cap)), c.stats()
    finally:
        c.close()


# ---- unit cases ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(M.UNIT_CASES))
def test_unit_case_equals_the_model(name):
    contigs, alignments = M.UNIT_CASES[name]
    text, st = _text(contigs, alignments)
    want = M.bedgraph(contigs, alignments)
    assert text == want
    if name == "nothing":
        assert text == b""
    lines, _, covered = M.totals(want)
    assert (st["alignments"], st["covered_bases"], st["runs"], st["text_bytes"]) == (len(alignments), covered, lines, len(want))


@pytest.mark.parametrize("name", list(M.CHUNK_CASES))
def test_runs_across_the_chunks_of_the_scan(name):
    contigs, alignments = M.CHUNK_CASES[name]
    text, st = _text(contigs, alignments, scan_chunk=64)
    want = M.bedgraph(contigs, alignments)
    assert text == want
    assert st["covered_bases"] == M.totals(want)[2] and st["runs"] == M.totals(want)[0]


@pytest.fixture(scope="module")
def randoms():
    contigs = [("one", 1), ("sixtyfour", 64), ("thousand", 1000)]
    alignments = random_alignments(random.Random(78), contigs, 3000)
    return contigs, alignments, M.bedgraph(contigs, alignments)


@pytest.mark.parametrize("scan_chunk", [0, 64, 100])
def test_random_alignments_equal_the_model(randoms, scan_chunk):
    contigs, alignments, want = randoms
    text, st = _text(contigs, alignments, scan_chunk)
    assert text == want and len(want) > 5000
    assert st["covered_bases"] == M.totals(want)[2]


def test_one_call_and_seven_calls_from_three_threads_give_the_same_bytes(randoms):
    contigs, alignments, want = randoms
    order = list(alignments)
    random.Random(5).shuffle(order)
    parts = [order[k::7] for k in range(7)]
    c = _coverage(contigs, 128)
    errors = []

    def work(mine):
        try:
            for p in mine:
                c.add(p)
        except Exception as e:   # (a failed add must fail the test, not only its thread)
            errors.append(e)

    threads = [threading.Thread(target=work, args=(parts[t::3],)) for t in range(3)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors
    c.finish()
    assert b"".join(c.pieces()) == want
    assert c.stats()["alignments"] == len(alignments)
    c.close()


def test_next_hands_out_whole_lines_only(randoms):
    contigs, alignments, want = randoms
    c = _coverage(contigs, 256)
    c.add(alignments)
    c.finish()
    first = want[:want.index(b"\n") + 1]
    n, data = c.next(len(first) - 1)   # smaller than the first line: its size comes back, nothing is copied
    assert (n, data) == (len(first), b"")
    n, data = c.next(0)
    assert (n, data) == (len(first), b"")
    pieces = []
    while True:
        n, data = c.next(100)
        if n == 0:
            break
        assert 0 < n <= 100 and len(data) == n and data.endswith(b"\n")
        pieces.append(data)
    assert b"".join(pieces) == want and len(pieces) > 50
    assert c.next(100) == (0, b"")
    c.close()


@pytest.mark.parametrize("k", range(len(BAD)))
def test_add_refuses_a_bad_alignment_by_its_index_and_adds_nothing(k):
    from nextgenmap_amd.engine import NgmHipError
    bad, message = BAD[k]
    good = [(0, 10, "20M"), (1, 5, "10M3D10M")]
    c = _coverage(M.TWO)
    c.add(good)
    batch = [(0, 0, "50M"), (1, 0, "50M"), (0, 30, "5M")]
    batch.insert(2, bad)
    with pytest.raises(NgmHipError) as e:
        c.add(batch)
    assert "alignment 2:" in str(e.value) and message in str(e.value)
    c.finish()
    assert b"".join(c.pieces()) == M.bedgraph(M.TWO, good)   # nothing of the refused call was added
    assert c.stats()["alignments"] == len(good)
    with pytest.raises(NgmHipError):
        c.add(good)   # after the finish
    c.close()


def _stats_beside_adds(obj, batch):
    """stats() 200 times on a second thread while this one makes 50 add calls: the last statistics"""
    seen, errors = [], []

    def watch():
        try:
            for _ in range(200):
                seen.append(obj.stats())
        except Exception as e:
            errors.append(e)

    t = threading.Thread(target=watch)
    t.start()
    for _ in range(50):
        obj.add(batch)
    t.join()
    assert not errors and len(seen) == 200
    assert all(0 <= st["alignments"] <= 50 * len(batch) and np.isfinite(st["add_ms"]) and st["add_ms"] >= 0 for st in seen)
    assert [st["alignments"] for st in seen] == sorted(st["alignments"] for st in seen)
    return obj.stats()


def test_stats_from_a_second_thread_while_the_first_adds():
    c = _coverage([("a", 200), ("b", 100)])
    st = _stats_beside_adds(c, [(0, 10, "50M"), (1, 0, "20M5D20M"), (0, 150, "60M"), (1, 90, "10M")])
    assert st["alignments"] == 200 and np.isfinite(st["add_ms"]) and st["add_ms"] >= 0
    c.close()


def test_next_before_the_finish_is_refused_with_its_message():
    from nextgenmap_amd.engine import NgmHipError
    c = _coverage(M.TWO)
    c.add([(0, 10, "20M")])
    with pytest.raises(NgmHipError) as e:
        c.next(100)
    assert str(e.value) == "ngm_coverage_next: ngm_coverage_finish has not been called"
    c.finish()
    with pytest.raises(NgmHipError) as e:
        c.finish()
    assert str(e.value) == "ngm_coverage_finish: called twice"
    assert b"".join(c.pieces()) == M.bedgraph(M.TWO, [(0, 10, "20M")])   # (the refused calls changed nothing)
    c.close()


# ---- the command line ---------------------------------------------------------------------------------------------------------------
def _hip(args, env=None):
    c = subprocess.run([CLI] + args, capture_output=True, text=True, env=dict(os.environ, **(env or {})))
    assert c.returncode == 0, "returncode=%d\n%s" % (c.returncode, c.stderr[-2500:])
    return c.stderr


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """the genome and the reads of tests/test_gpu_bam_input.py's world: two contigs of 400 000 and 300 001 bases, 2 000 single-end reads and
    1 000 pairs of 100 bp; the runs are kept, so that a case several tests look at is mapped once"""
    d = tmp_path_factory.mktemp("coverage")
    contigs = S.make_genome([400000, 300001], seed=801, repeat_families=10, repeat_len=500, copies=6)
    fa = str(d / "ref.fa")
    S.write_fasta(fa, contigs)
    rng = np.random.default_rng(9)
    qual = lambda n, i: bytes(48 + (7 * j + i) % 37 for j in range(n))
    se = [(n.encode(), s.tobytes(), qual(len(s), i)) for i, (n, s, _) in enumerate(S.make_reads(contigs, 2000, 100, seed=811, sub_rate=0.02, indel_rate=0.003))]
    for k in range(0, 40, 2):   # reads that map nowhere
        se[k] = (se[k][0], S.ACGT[rng.integers(0, 4, 100)].tobytes(), se[k][2])
    r1, r2 = S.make_reads(contigs, 1000, 100, seed=812, sub_rate=0.02, indel_rate=0.003, paired=True)
    pe = [(n.encode(), s.tobytes(), qual(len(s), i)) for i, pair in enumerate(zip(r1, r2)) for n, s, _ in pair]
    files = {}
    for tag, reads in (("se", se), ("pe", pe)):
        files[tag] = str(d / (tag + ".fq"))
        with open(files[tag], "wb") as f:
            f.write(b"".join(b"@" + n + b"\n" + s + b"\n+\n" + q + b"\n" for n, s, q in reads))
    return d, fa, files, {}


def _run(world, reads, opts, env=None, coverage=True):
    """-> (output file, bedGraph file or None, log)"""
    d, fa, files, cache = world
    key = (reads, tuple(opts), tuple(sorted((env or {}).items())), coverage)
    if key not in cache:
        out = str(d / ("out%d.%s" % (len(cache), "bam" if "-b" in opts else "sam")))
        bed = str(d / ("out%d.bedgraph" % len(cache))) if coverage else None
        log = _hip(["-r", fa, "-o", out] + (["-p"] if reads == "pe" else []) + ["-q", files[reads]] + list(opts) + (["--coverage", bed] if coverage else []), env)
        cache[key] = (out, bed, log)
    return cache[key]


def _counted(out):
    """(contigs, the alignments that count) of the file a run wrote"""
    if out.endswith(".bam"):
        _, refs, recs = decode_bam(out)
        return refs, M.alignments_of_bam(recs)
    lines = open(out).readlines()
    contigs = M.sam_contigs(lines)
    return contigs, M.alignments_of_sam(lines, contigs)


def _check(out, bed, log):
    contigs, alignments = _counted(out)
    text = open(bed, "rb").read()
    assert text == M.bedgraph(contigs, alignments)
    # no comparison passes on an empty file
    lines, top, total = M.totals(text)
    assert lines >= 1000 and top >= 2
    assert total == sum(M.matched_bases(c) for _, _, c in alignments)
    assert "[MAIN] Coverage on the GPU: %d alignments, %d covered bases, %d runs, %d bytes of bedGraph; kernels: add " % (len(alignments), total, lines, len(text)) in log
    return text


CLI_CASES = {
    "se-affine-sam": ("se", ["--affine"], {}),
    "pe-linear-bam": ("pe", ["-b"], {}),
    "pe-sorted-bam": ("pe", ["-b", "--sort"], {}),
    "se-topn-3": ("se", ["-n", "3"], {}),
    "pe-filters": ("pe", ["--no-unal", "-Q", "10", "-i", "0.9"], {}),
    "se-hard-clip": ("se", ["--hard-clip"], {}),
    "se-slamdunk": ("se", ["--slam-seq", "2", "-5", "12", "--max-polya", "4", "-l"], {}),
    "pe-bam-host-records": ("pe", ["-b"], {"NGM_HIP_BAM_HOST_RECORDS": "1"}),
    "se-small-batches": ("se", ["--affine", "--batch-size", "700", "--workers", "3"], {}),
}


@pytest.mark.parametrize("case", list(CLI_CASES))
def test_bedgraph_equals_the_model_over_the_file_the_run_wrote(world, case):
    reads, opts, env = CLI_CASES[case]
    out, bed, log = _run(world, reads, opts, env)
    text = _check(out, bed, log)
    if case == "se-topn-3":   # the host route: secondary records are written and do not count
        assert any(int(l.split("\t")[1]) & 0x100 for l in open(out) if not l.startswith("@"))
    if case == "pe-filters":   # the filters have removed records
        assert len(_counted(out)[1]) < len(_counted(_run(world, "pe", ["-b"])[0])[1])
    if case == "pe-bam-host-records":
        assert text == open(_run(world, "pe", ["-b"])[1], "rb").read()
    if case == "se-small-batches":
        assert text == open(_run(world, "se", ["--affine"])[1], "rb").read()


def test_output_is_the_same_with_and_without_the_option(world):
    body = lambda p: [l for l in open(p) if not l.startswith("@PG")]
    with_cov, _, log = _run(world, "se", ["--affine"])
    without, _, log0 = _run(world, "se", ["--affine"], coverage=False)
    assert body(with_cov) == body(without) and len(body(without)) > 2000
    assert "Coverage" not in log0 and "Coverage counters: 2.7 MiB on GPU 0" in log
