"""-m gpu: `ngm-hip --snp` and the SNP object behind it (include/ngm_pipeline.h, ngm_snp_*).  Unit cases through the ctypes mirror, no
genome and no mapper, each compared byte for byte with tests/snp_model.py; then the command line on a 70 kb genome with planted
substitutions, where the VCF must equal the model applied to the SAM / BAM file the same run wrote and the FASTA."""
import os
import random
import shutil
import subprocess
import threading

import numpy as np
import pytest

import coverage_model as CM
import simulate as S
import snp_model as M
from test_coverage_host import BAD as COVERAGE_BAD
from test_gpu_bam import decode_bam
from test_snp_host import BAD as SNP_BAD

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "nextgenmap_amd", "ngm-hip")
STATS = ("alignments", "alt_bases", "calls", "text_bytes", "covered_bases")


def _caller(case, scan_chunk=0):
    from nextgenmap_amd.pipeline import SnpCaller
    contigs, _, N, F, Q = case
    return SnpCaller(contigs, 0, N, F, Q, scan_chunk)


def _add(c, records):
    """(one call takes records that all have a quality string, or none of them)"""
    for part in ([r for r in records if r[4] is None], [r for r in records if r[4] is not None]):
        if part:
            c.add(part)


def _text(case, scan_chunk=0, cap=1 << 20):
    c = _caller(case, scan_chunk)
    try:
        _add(c, case[1])
        c.finish()
        return b"".join(c.pieces(cap)), c.stats()
    finally:
        c.close()


def _same_totals(st, case):
    want = M.totals(*case)
    assert {k: st[k] for k in STATS} == want


# ---- unit cases ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(M.UNIT_CASES))
def test_unit_case_equals_the_model(name):
    case = M.UNIT_CASES[name]
    text, st = _text(case)
    assert text == M.vcf(*case)
    if name == "nothing":
        assert text == M.header(case[0], *case[2:]).encode()
    _same_totals(st, case)


@pytest.mark.parametrize("name", list(M.CHUNK_CASES))
def test_calls_across_the_chunks_of_the_scan(name):
    case = M.CHUNK_CASES[name]
    text, st = _text(case, scan_chunk=64)
    assert text == M.vcf(*case)
    _same_totals(st, case)


@pytest.fixture(scope="module")
def randoms():
    case = M.random_case(78, 3000)
    return case, M.vcf(*case)


@pytest.mark.parametrize("scan_chunk", [0, 64, 100])
def test_random_records_equal_the_model(randoms, scan_chunk):
    case, want = randoms
    text, st = _text(case, scan_chunk)
    assert text == want and len(M.parse_vcf(want)) >= 20
    _same_totals(st, case)


def test_one_call_and_seven_calls_from_three_threads_give_the_same_bytes(randoms):
    case, want = randoms
    order = list(case[1])
    random.Random(5).shuffle(order)
    parts = [order[k::7] for k in range(7)]
    c = _caller(case, 128)
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
    c.finish()
    assert b"".join(c.pieces()) == want
    _same_totals(c.stats(), case)
    c.close()


def test_next_hands_out_whole_lines_only(randoms):
    case, want = randoms
    c = _caller(case, 256)
    _add(c, case[1])
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
    assert b"".join(pieces) == want and len(pieces) > 20
    assert pieces[0].startswith(b"##fileformat=VCFv4.2\n")   # the header is the first piece
    assert c.next(100) == (0, b"")
    c.close()


# every record ngm_coverage_add refuses (those checks come first, whatever the sequence), then the ones only ngm_snp_add refuses
ALL_BAD = [((c, p, g, "ACGTA", None), msg) for (c, p, g), msg in COVERAGE_BAD] + SNP_BAD


@pytest.mark.parametrize("k", range(len(ALL_BAD)))
def test_add_refuses_a_bad_record_by_its_index_and_adds_nothing(k):
    from nextgenmap_amd.engine import NgmHipError
    from nextgenmap_amd.pipeline import SnpCaller
    bad, message = ALL_BAD[k]
    contigs = M.UNIT_CASES["nothing"][0]
    good = [M.rec(contigs, 0, 10, "20M", [3]), M.rec(contigs, 1, 5, "10M3D10M", [12])]
    c = SnpCaller(contigs, 0, 1, "0.5", 15)
    c.add(good)
    batch = [M.rec(contigs, 0, 0, "50M", [1]), M.rec(contigs, 1, 0, "50M", [2]), M.rec(contigs, 0, 30, "5M", [3])]
    batch.insert(2, bad)
    with_q = bad[4] is not None
    if with_q:   # (a call's records all have qualities or none has: the quality text is one string under the sequences' offsets)
        batch = [r[:4] + ("I" * len(r[3]),) for r in batch[:2]] + [bad]
    b = lambda x: x.encode()
    off = np.concatenate(([0], np.cumsum([len(r[2]) for r in batch]))).astype(np.uint32)
    soff = np.concatenate(([0], np.cumsum([len(r[3]) for r in batch]))).astype(np.uint32)
    with pytest.raises(NgmHipError) as e:
        c.add_arrays([r[0] for r in batch], [r[1] for r in batch], off, b("".join(r[2] for r in batch)), soff, b("".join(r[3] for r in batch)),
                     b("".join(r[4] for r in batch)) if with_q else None)
    assert "ngm_snp_add: alignment 2:" in str(e.value) and message in str(e.value)
    c.finish()
    case = (contigs, good, 1, "0.5", 15)
    assert b"".join(c.pieces()) == M.vcf(*case) and len(M.calls(*case)) == 2   # nothing of the refused call was added
    _same_totals(c.stats(), case)
    with pytest.raises(NgmHipError):
        c.add(good)   # after the finish
    c.close()


def test_a_quality_text_that_goes_on_past_the_last_record_is_refused():
    from nextgenmap_amd.engine import NgmHipError
    from nextgenmap_amd.pipeline import SnpCaller
    contigs = M.UNIT_CASES["nothing"][0]
    c = SnpCaller(contigs, 0, 1, "0.5", 15)
    with pytest.raises(NgmHipError) as e:
        c.add_arrays([0, 0], [0, 5], np.array([0, 2, 4], dtype=np.uint32), b"3M2M", np.array([0, 3, 5], dtype=np.uint32), b"ACGTA", b"IIIIII")
    assert "ngm_snp_add: alignment 1:" in str(e.value) and "its quality text has another length" in str(e.value)
    c.close()


def test_thresholds_out_of_range_are_refused():
    from nextgenmap_amd.engine import NgmHipError
    from nextgenmap_amd.pipeline import SnpCaller
    contigs = M.UNIT_CASES["nothing"][0]
    for kw in (dict(min_frac="0"), dict(min_frac="1.5"), dict(min_qual=94), dict(min_qual=-1)):
        with pytest.raises(NgmHipError):
            SnpCaller(contigs, 0, **kw)


def test_stats_from_a_second_thread_while_the_first_adds():
    from nextgenmap_amd.pipeline import SnpCaller
    from test_gpu_coverage import _stats_beside_adds
    rnd = random.Random(3)
    contigs = [("a", "".join(rnd.choice("ACGT") for _ in range(200))), ("b", "".join(rnd.choice("ACGT") for _ in range(100)))]
    c = SnpCaller(contigs, 0, 1, "0.5", 0)
    st = _stats_beside_adds(c, [(0, 10, "50M", "A" * 50, None), (1, 0, "20M5D20M", "C" * 40, None), (0, 150, "60M", "G" * 60, None), (1, 90, "10M", "T" * 10, None)])
    assert st["alignments"] == 200 and np.isfinite(st["add_ms"]) and st["add_ms"] >= 0
    c.close()


def test_next_before_the_finish_is_refused_with_its_message():
    from nextgenmap_amd.engine import NgmHipError
    case = M.UNIT_CASES[next(iter(M.UNIT_CASES))]
    c = _caller(case)
    with pytest.raises(NgmHipError) as e:
        c.next(100)
    assert str(e.value) == "ngm_snp_next: ngm_snp_finish has not been called"
    _add(c, case[1])
    c.finish()
    with pytest.raises(NgmHipError) as e:
        c.finish()
    assert str(e.value) == "ngm_snp_finish: called twice"
    assert b"".join(c.pieces()) == M.vcf(*case)   # (the refused calls changed nothing)
    c.close()


# ---- the command line ---------------------------------------------------------------------------------------------------------------
def _hip(args, env=None):
    c = subprocess.run([CLI] + args, capture_output=True, text=True, env=dict(os.environ, **(env or {})))
    assert c.returncode == 0, "returncode=%d\n%s" % (c.returncode, c.stderr[-2500:])
    return c.stderr


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """two contigs of 40 000 and 30 001 bases; the FASTA holds the original, the reads -- 10 500 single-end reads and 5 250 pairs of 100 bp,
    a mean depth of 15 -- are drawn from a copy with 150 planted substitutions; Phred qualities 12..40, so that some columns cannot vote.
    The runs are kept, so that a case several tests look at is mapped once."""
    d = tmp_path_factory.mktemp("snp")
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
        planted[(c, p)] = M.other(chr(contigs[c][p]), int(rng.integers(1, 4)))
        mutated[c][p] = ord(planted[(c, p)])
    qual = lambda n, i: bytes(33 + 12 + (7 * j + i) % 29 for j in range(n))
    se = [(n.encode(), s.tobytes(), qual(len(s), i)) for i, (n, s, _) in enumerate(S.make_reads(mutated, 10500, 100, seed=911, sub_rate=0.01, indel_rate=0.002))]
    r1, r2 = S.make_reads(mutated, 5250, 100, seed=912, sub_rate=0.01, indel_rate=0.002, paired=True)
    pe = [(n.encode(), s.tobytes(), qual(len(s), i)) for i, pair in enumerate(zip(r1, r2)) for n, s, _ in pair]
    files = {}
    for tag, reads in (("se", se), ("pe", pe)):
        files[tag] = str(d / (tag + ".fq"))
        with open(files[tag], "wb") as f:
            f.write(b"".join(b"@" + n + b"\n" + s + b"\n+\n" + q + b"\n" for n, s, q in reads))
    return d, fa, files, {}, planted, {}


def _run(world, reads, opts, env=None, snp=True):
    """-> (output file, VCF file or None, log)"""
    d, fa, files, cache = world[:4]
    key = (reads, tuple(opts), tuple(sorted((env or {}).items())), snp)
    if key not in cache:
        out = str(d / ("out%d.%s" % (len(cache), "bam" if "-b" in opts else "sam")))
        vcf = str(d / ("out%d.vcf" % len(cache))) if snp else None
        opts = [o.replace("COVERAGE", out + ".bedgraph") for o in opts]
        log = _hip(["-r", fa, "-o", out] + (["-p"] if reads == "pe" else []) + ["-q", files[reads]] + opts + (["--snp", vcf] if snp else []), env)
        cache[key] = (out, vcf, log)
    return cache[key]


def _counted(world, out):
    """the records that count of the file a run wrote (read once per file)"""
    seen = world[5]
    if out not in seen:
        if out.endswith(".bam"):
            seen[out] = M.records_of_bam(decode_bam(out)[2])
        else:
            seen[out] = M.records_of_sam(open(out).readlines(), M.read_fasta(world[1]))
    return seen[out]


def _check(world, out, vcf, log, N=10, F="0.8", Q=15):
    contigs = M.read_fasta(world[1])
    records = _counted(world, out)
    text = open(vcf, "rb").read()
    case = (contigs, records, N, F, Q)
    assert text == M.vcf(*case)
    t = M.totals(*case)
    assert "[MAIN] SNPs on the GPU: %d alignments, %d mismatching bases counted, %d calls, %d bytes of VCF; kernels: add " % (t["alignments"], t["alt_bases"], t["calls"], t["text_bytes"]) in log
    # no comparison passes on an empty file: at least half of the planted sites are called with the planted base, and every call is deep enough
    calls = M.parse_vcf(text)
    names = [n for n, _ in contigs]
    found = {(names.index(n), p - 1): a for n, p, _, a, _, _ in calls}
    planted = world[4]
    assert sum(1 for site, base in planted.items() if found.get(site) == base) >= len(planted) // 2
    assert all(dp >= max(1, N) and ao <= dp for *_, dp, ao in calls)
    return text


CLI_CASES = {
    "se-affine-sam": ("se", ["--affine"], {}),
    "pe-linear-bam": ("pe", ["-b"], {}),
    "pe-sorted-bam-with-coverage": ("pe", ["-b", "--sort", "--coverage", "COVERAGE"], {}),
    "se-topn-3": ("se", ["-n", "3"], {}),
    "pe-filters": ("pe", ["--no-unal", "-Q", "10", "-i", "0.9"], {}),
    "se-hard-clip": ("se", ["--hard-clip"], {}),
    "se-slamdunk": ("se", ["--slam-seq", "2", "-5", "12", "--max-polya", "4", "-l", "--snp-min-cov", "8", "--snp-min-frac", "0.75", "--snp-min-qual", "13"], {}),
    "pe-bam-host-records": ("pe", ["-b"], {"NGM_HIP_BAM_HOST_RECORDS": "1"}),
    "se-small-batches": ("se", ["--affine", "--batch-size", "700", "--workers", "3"], {}),
}


@pytest.mark.parametrize("case", list(CLI_CASES))
def test_vcf_equals_the_model_over_the_file_the_run_wrote(world, case):
    reads, opts, env = CLI_CASES[case]
    out, vcf, log = _run(world, reads, opts, env)
    text = _check(world, out, vcf, log, *((8, "0.75", 13) if case == "se-slamdunk" else ()))
    if case == "pe-sorted-bam-with-coverage":   # both files of one run, from one pass
        _, refs, recs = decode_bam(out)
        assert open(out + ".bedgraph", "rb").read() == CM.bedgraph(refs, CM.alignments_of_bam(recs))
    if case == "se-topn-3":   # the host route: secondary records are written and do not count
        assert any(int(l.split("\t")[1]) & 0x100 for l in open(out) if not l.startswith("@"))
    if case == "pe-filters":   # the filters have removed records
        assert len(_counted(world, out)) < len(_counted(world, _run(world, "pe", ["-b"])[0]))
    if case == "se-slamdunk":
        assert b"min-cov 8, min-frac 0.75, min-qual 13" in text
    if case == "pe-bam-host-records":
        assert text == open(_run(world, "pe", ["-b"])[1], "rb").read()
    if case == "se-small-batches":
        assert text == open(_run(world, "se", ["--affine"])[1], "rb").read()


def test_output_is_the_same_with_and_without_the_option(world):
    body = lambda p: [l for l in open(p) if not l.startswith("@PG")]
    with_snp, _, log = _run(world, "se", ["--affine"])
    without, _, log0 = _run(world, "se", ["--affine"], snp=False)
    assert body(with_snp) == body(without) and len(body(without)) > 10000
    assert "SNP" not in log0 and "SNP counters: 1.1 MiB on GPU 0 (16 bytes per base" in log


def test_a_second_run_reads_the_written_file_as_its_vcf(world, tmp_path):
    _, vcf, _ = _run(world, "se", ["--affine"])
    calls = len(M.parse_vcf(open(vcf, "rb").read()))
    assert calls >= 75
    fa = str(tmp_path / "ref.fa")   # (a directory without an index cache: an index loaded from a cache is not rebuilt with the VCF)
    shutil.copy(world[1], fa)
    log = _hip(["-r", fa, "-q", world[2]["se"], "-o", str(tmp_path / "again.sam"), "--vcf", vcf, "--skip-save"])
    assert "Loaded VCF (%d variations)" % calls in log
