"""-m gpu: `ngm-hip --count` and the conversion counter behind it (include/ngm_pipeline.h, ngm_count_*).  Unit cases through the ctypes
mirror, no genome and no mapper, each compared byte for byte with tests/count_model.py; then the command line on the 70 kb genome with
planted substitutions of tests/test_gpu_snp.py, its reads carrying T>C conversions, where the TSV must equal the model applied to the
SAM / BAM file, the VCF, the FASTA and the BED file of the same run."""
import os
import random
import subprocess
import threading

import numpy as np
import pytest

import count_model as M
import simulate as S
from snp_model import other
from test_coverage_host import BAD as COVERAGE_BAD
from test_snp_host import BAD as SNP_BAD

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "nextgenmap_amd", "ngm-hip")


def _counter(case):
    from nextgenmap_amd.pipeline import ConversionCounter
    contigs, _, regions, _, Q = case
    return ConversionCounter(contigs, regions, 0, Q)


def _add(c, records):
    """(one call takes records that all have a quality string, or none of them)"""
    for part in ([r for r in records if r[4] is None], [r for r in records if r[4] is not None]):
        if part:
            c.add(part)


def _finish(c, case):
    c.mask(sorted(case[3]))
    c.finish()
    st = c.stats()
    return c.tsv(), {k: st[k] for k in M.STATS}


def _want(case):
    rows, stats = M.tally(*case)
    return M.tsv(case[0], case[2], rows), stats


# ---- unit cases ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(M.UNIT_CASES))
def test_unit_case_equals_the_model(name):
    case = M.UNIT_CASES[name]
    c = _counter(case)
    try:
        _add(c, case[1])
        assert _finish(c, case) == _want(case)
    finally:
        c.close()


@pytest.fixture(scope="module")
def randoms():
    case = M.random_case(78, 3000)
    return case, _want(case)


def test_random_records_equal_the_model(randoms):
    case, want = randoms
    c = _counter(case)
    _add(c, case[1])
    c.mask(sorted(case[3])[:20])   # (the mask may come in several calls, and a position twice)
    c.mask(sorted(case[3])[10:])
    assert _finish(c, case) == want
    rows = M.parse_tsv(want[0])
    assert sum(1 for r in rows if r[8] > 0) >= 20 and sum(1 for r in rows if r[6] > 0) >= 5 and want[1]["conversions"] > 1000
    assert c.stats()["add_ms"] > 0 and c.stats()["reduce_ms"] > 0
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
    assert _finish(c, case) == want
    c.close()


# every record ngm_coverage_add refuses (those checks come first, whatever the sequence), then the ones only ngm_snp_add refuses
ALL_BAD = [((c, p, g, "ACGTA", None), msg) for (c, p, g), msg in COVERAGE_BAD] + SNP_BAD


@pytest.mark.parametrize("k", range(len(ALL_BAD)))
def test_add_refuses_a_bad_record_by_its_index_and_adds_nothing(k):
    from nextgenmap_amd.engine import NgmHipError
    from nextgenmap_amd.pipeline import ConversionCounter
    bad, message = ALL_BAD[k]
    contigs = [("chrA", "ACGT" * 25), ("chrB", "TTAGA" * 10)]   # (the two contigs of 100 and 50 bases the bad records are written for)
    regions = [(0, 0, 100, "a", "."), (1, 0, 50, "b", "+")]
    good = [M.rec(contigs, 0, 10, "20M", conv="all"), M.rec(contigs, 1, 5, "10M3D10M", conv="all")]
    c = ConversionCounter(contigs, regions, 0, 27)
    c.add(good)
    batch = [M.rec(contigs, 0, 0, "50M", conv="all"), M.rec(contigs, 1, 0, "50M", conv="all"), M.rec(contigs, 0, 30, "5M", True, conv="all")]
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
    assert "ngm_count_add: alignment 2:" in str(e.value) and message in str(e.value)
    case = (contigs, good, regions, set(), 27)
    assert _finish(c, case) == _want(case) and _want(case)[1]["conversions"] > 5   # nothing of the refused call was added
    with pytest.raises(NgmHipError):
        c.add(good)   # after the finish
    c.close()


def test_bad_parameters_are_refused():
    from nextgenmap_amd.engine import NgmHipError
    from nextgenmap_amd.pipeline import ConversionCounter
    contigs = [("chrA", "ACGT" * 25)]
    for regions, q in (([], 27), ([(0, 0, 10, "r", "+")], 94), ([(0, 0, 10, "r", "+")], -1), ([(1, 0, 10, "r", "+")], 27), ([(0, 10, 10, "r", "+")], 27), ([(0, 0, 101, "r", "+")], 27),
                       ([(0, 0, 10, "r", "*")], 27)):
        with pytest.raises(NgmHipError):
            ConversionCounter(contigs, regions, 0, q)
    c = ConversionCounter(contigs, [(0, 0, 10, "r", "+")], 0, 27)
    for bad in ([(1, 0)], [(0, 100)], [(0, -1)]):
        with pytest.raises(NgmHipError):
            c.mask(bad)
    c.mask([(0, 50)])   # outside every region: ignored
    c.finish()
    assert c.stats()["masked_positions"] == 0
    c.close()


# ---- the command line ---------------------------------------------------------------------------------------------------------------
def _hip(args, env=None):
    c = subprocess.run([CLI] + args, capture_output=True, text=True, env=dict(os.environ, **(env or {})), timeout=60)   # (a run takes 1-2 s)
    assert c.returncode == 0, "returncode=%d\n%s" % (c.returncode, c.stderr[-2500:])
    return c.stderr


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """the genome of tests/test_gpu_snp.py -- two contigs of 40 000 and 30 001 bases, the FASTA holds the original, the reads are drawn from a
    copy with 150 planted substitutions -- with 6 000 single-end reads and 3 000 pairs of 100 bp; in two reads out of three, one T in twelve is
    read as C (a read that maps to the reverse strand shows them as A>G); Phred qualities 20..40, so that some columns are below Q = 27.
    43 regions on both strands: tiled ones, overlapping ones of opposite strands, a nested and a repeated one.  The runs are kept."""
    d = tmp_path_factory.mktemp("count")
    contigs = S.make_genome([40000, 30001], seed=901, repeat_families=4, repeat_len=300, copies=3)
    fa = str(d / "ref.fa")
    S.write_fasta(fa, contigs)
    rng = np.random.default_rng(19)
    mutated = [g.copy() for g in contigs]
    planted = {}
    while len(planted) < 150:
        c = int(rng.integers(0, 2))
        p = int(rng.integers(200, len(contigs[c]) - 200))
        if (c, p) in planted or chr(contigs[c][p]) not in "ACGT":
            continue
        planted[(c, p)] = other(chr(contigs[c][p]), int(rng.integers(1, 4)))
        mutated[c][p] = ord(planted[(c, p)])
    qual = lambda n, i: bytes(33 + 20 + (7 * j + i) % 21 for j in range(n))

    def labelled(i, s):
        s = s.copy()
        if i % 3:
            ts = np.flatnonzero(s == ord("T"))
            s[ts[rng.random(len(ts)) < 1 / 12]] = ord("C")
        return s.tobytes()

    se = [(n.encode(), labelled(i, s), qual(len(s), i)) for i, (n, s, _) in enumerate(S.make_reads(mutated, 6000, 100, seed=911, sub_rate=0.01, indel_rate=0.002))]
    r1, r2 = S.make_reads(mutated, 3000, 100, seed=912, sub_rate=0.01, indel_rate=0.002, paired=True)
    pe = [(n.encode(), labelled(i, s), qual(len(s), i)) for i, pair in enumerate(zip(r1, r2)) for n, s, _ in pair]
    files = {}
    for tag, reads in (("se", se), ("pe", pe)):
        files[tag] = str(d / (tag + ".fq"))
        with open(files[tag], "wb") as f:
            f.write(b"".join(b"@" + n + b"\n" + s + b"\n+\n" + q + b"\n" for n, s, q in reads))
    regions = [("chr1", 1000 + 1500 * k, 1700 + 1500 * k, "a%d" % k, "+-."[k % 3]) for k in range(24)]
    regions += [("chr2", 800 + 1700 * k, 1700 + 1700 * k, "b%d" % k, "-+"[k % 2]) for k in range(16)]
    regions += [("chr1", 1400, 2900, "over", "-"), ("chr2", 1000, 1100, "nested", "+"), ("chr1", 1000, 1700, "a0", "+")]
    bed = str(d / "utrs.bed")
    with open(bed, "w") as f:
        f.write("track name=utrs\n" + "".join("%s\t%d\t%d\t%s\t0\t%s\n" % r for r in regions))
    return d, fa, files, {}, bed


def _run(world, reads, opts, env=None, snp=True, count=True):
    """-> (output file, VCF file or None, TSV file or None, log)"""
    d, fa, files, cache, bed = world
    key = (reads, tuple(opts), tuple(sorted((env or {}).items())), snp, count)
    if key not in cache:
        out = str(d / ("out%d.%s" % (len(cache), "bam" if "-b" in opts else "sam")))
        vcf = str(d / ("out%d.vcf" % len(cache))) if snp else None
        tsv = str(d / ("out%d.tsv" % len(cache))) if count else None
        log = _hip(["-r", fa, "-o", out] + (["-p"] if reads == "pe" else []) + ["-q", files[reads]] + opts + (["--snp", vcf, "--snp-min-cov", "4"] if snp else []) +
                   (["--count", bed, "--count-out", tsv] if count else []), env)
        cache[key] = (out, vcf, tsv, log)
    return cache[key]


CLI_CASES = {
    "se-slamdunk-sorted-bam-snp": ("se", ["--slam-seq", "2", "-n", "1", "--strata", "-b", "--sort"], {}, True),
    "se-plain-sam-no-snp": ("se", [], {}, False),
    "pe-affine": ("pe", ["--affine"], {}, True),
    "se-topn-2": ("se", ["-n", "2"], {}, True),
}


@pytest.mark.parametrize("case", list(CLI_CASES))
def test_tsv_equals_the_model_over_the_files_the_run_wrote(world, case):
    reads, opts, env, snp = CLI_CASES[case]
    out, vcf, tsv, log = _run(world, reads, opts, env, snp)
    text = open(tsv, "rb").read()
    assert text == M.from_sam(out, world[1], world[4], vcf)
    # no comparison passes on an empty file
    rows = M.parse_tsv(text)
    with_conv = [r for r in rows if r[8] > 0]
    assert len(rows) == 43 and len(with_conv) >= 10 and {"+", "-"} <= {r[4] for r in with_conv}
    assert all(r[8] <= r[7] and r[10] <= r[9] for r in rows) and sum(r[10] for r in rows) >= 100
    if snp:
        masked = [r for r in rows if r[6] > 0]
        assert masked and {"+", "-"} <= {r[4] for r in masked}
        assert text != M.from_sam(out, world[1], world[4], None)   # (the mask decides numbers)
    else:
        assert all(r[6] == 0 for r in rows)
    assert "[MAIN] Conversions on the GPU: " in log and " masked positions in 43 regions; kernels: add " in log
    assert "[MAIN] Conversion counters: 43 regions over " in log
    if case == "se-topn-2":   # the host route: secondary records are written and do not count
        assert any(int(l.split("\t")[1]) & 0x100 for l in open(out) if not l.startswith("@"))


def test_the_log_line_reports_the_models_statistics(world):
    out, vcf, tsv, log = _run(world, "se", [], {}, False)
    contigs = M.read_fasta(world[1])
    stats = M.tally(contigs, M.records_of_sam(open(out).readlines(), contigs), M.parse_bed(open(world[4]).read(), contigs), set())[1]
    assert "[MAIN] Conversions on the GPU: %d alignments, %d of them in a region, %d eligible columns, %d conversions, 0 masked positions in 43 regions; " % (
        stats["alignments"], stats["met_a_region"], stats["eligible_columns"], stats["conversions"]) in log


def test_tsv_does_not_depend_on_batches_and_workers(world):
    a = _run(world, "se", [], {}, False)
    b = _run(world, "se", ["--batch-size", "1100", "--workers", "3"], {}, False)
    assert open(a[2], "rb").read() == open(b[2], "rb").read()


def test_output_is_the_same_with_and_without_the_option(world):
    body = lambda p: [l for l in open(p) if not l.startswith("@PG")]
    with_count, _, _, log = _run(world, "se", [], {}, False)
    without, _, _, log0 = _run(world, "se", [], {}, False, count=False)
    assert body(with_count) == body(without) and len(body(without)) > 6000
    assert "Conversion" not in log0


def test_side_outputs_fed_from_a_second_device_equal_a_one_device_run(tmp_path):
    """the objects live on the first device; with -g 0,1 the second device's mapper hands its records to them through ngm_*_add"""
    import nextgenmap_amd
    if nextgenmap_amd.load_library().ngm_hip_device_count() < 2:
        pytest.skip("one visible GPU: the route from another device needs two")
    contigs = S.make_genome([30000, 20000], seed=77)
    fa, fq, bed = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fq"), str(tmp_path / "r.bed")
    S.write_fasta(fa, contigs)
    with open(fq, "wb") as f:
        f.write(b"".join(b"@" + n.encode() + b"\n" + s.tobytes() + b"\n+\n" + bytes(33 + 20 + (7 * j + i) % 21 for j in range(len(s))) + b"\n"
                         for i, (n, s, _) in enumerate(S.make_reads(contigs, 2000, 100, seed=78, sub_rate=0.02, indel_rate=0.002))))
    with open(bed, "w") as f:
        f.write("".join("chr%d\t%d\t%d\tr%d\t0\t%s\n" % (1 + k % 2, 500 + 900 * k, 1200 + 900 * k, k, "+-"[k % 2]) for k in range(20)))
    files = {}
    for tag, gpus in (("one", "0"), ("two", "0,1")):
        names = [str(tmp_path / (tag + ext)) for ext in (".bedgraph", ".vcf", ".tsv")]
        _hip(["-r", fa, "-q", fq, "-o", str(tmp_path / (tag + ".sam")), "-g", gpus, "--batch-size", "500", "--coverage", names[0], "--snp", names[1], "--snp-min-cov", "2",
              "--count", bed, "--count-out", names[2]])
        files[tag] = [open(n, "rb").read() for n in names]
    assert all(len(t) > 200 for t in files["one"])
    assert files["two"] == files["one"]
