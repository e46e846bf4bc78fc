"""-m gpu: `ngm-hip -5 N --max-polya M` -- reads trimmed as the reference's parser and ReadProvider trim them, the XA:i tag in all four
writers, and slamdunk's mapping command (`--slam-seq 2 -5 12 --max-polya 4 ... -b`) with BAM records written by the GPU.
 1. the committed fixtures (tests/make_trim_goldens.py) against the records the REAL program wrote for them, SAM and BAM, GPU and host writers;
 2. live against `ngm-core --affine -t 1` on reads with random tails, with --hard-clip, -e and --max-polya 0;
 3. slamdunk's command against the real program with this library behind IAlignment (oracle/_ref/dropin/ngm-core-hip: the linear
    personality SLAM-seq needs; its parser, ReadProvider and writers are the reference's own);
 4. `--slam-seq 1 --bam` without the new options: the GPU's records against the host twin's.
Every comparison is for identical records, every record compared."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import make_trim_goldens as TG
import ref_files as RF
import simulate as S
from test_gpu_bam import decode_bam

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "nextgenmap_amd", "ngm-hip")
DROPIN = os.path.join(ROOT, "oracle", "_ref", "dropin", "ngm-core-hip")
GPU_BAM_LINE = "BAM records and their BGZF blocks written on the GPU"
SLAMDUNK = ["--slam-seq", "2", "-5", "12", "--max-polya", "4", "-l", "--rg-id", "s", "--rg-sm", "s:pulse:0", "-n", "1", "--strata"]


def _hip(args, env=None):
    c = subprocess.run([CLI] + args, capture_output=True, text=True, env=dict(os.environ, **(env or {})))
    assert c.returncode == 0, "returncode=%d\n%s" % (c.returncode, c.stderr[-2500:])
    return c.stderr


def _ref_program(binary, fa, args, out):
    own = os.path.join(os.path.dirname(fa), "refrun")   # (a link of its own: the programs do not share index cache files)
    os.makedirs(own, exist_ok=True)
    if not os.path.exists(os.path.join(own, "ref.fa")):
        os.link(fa, os.path.join(own, "ref.fa"))
    r = subprocess.run([binary, "-r", os.path.join(own, "ref.fa"), "-o", out, "-t", "1", "--no-progress"] + args, capture_output=True, text=True, cwd=own, timeout=600)
    assert "Done" in (r.stdout + r.stderr), (r.stdout + r.stderr)[-2500:]
    return r.stdout + r.stderr


def _same_sam(want, got, n=None):
    a, b = TG.sam_records(want), TG.sam_records(got)
    assert set(a) == set(b) and (n is None or len(a) == n), (len(a), len(b), n)
    diff = [(a[k], b[k]) for k in a if a[k] != b[k]]
    print("SAM records differing:", len(diff), "of", len(a))
    assert not diff, str(diff[:2])[:2000]
    head = lambda p: [l for l in (gzip.open(p, "rt") if p.endswith(".gz") else open(p)) if l.startswith("@") and not l.startswith("@PG")]
    assert head(want) == head(got)
    return a


def _same_bam(want, got, n=None):
    (ta, ra, a), (tb, rb, b) = TG.bam_records(want), TG.bam_records(got)
    strip = lambda t: [l.split("\tCL:")[0] if l.startswith("@PG") else l for l in t.splitlines()]
    assert ra == rb and strip(ta) == strip(tb), (ta, tb)
    assert set(a) == set(b) and (n is None or len(a) == n), (len(a), len(b), n)
    diff = [[(f, a[k][f], b[k][f]) for f in a[k] if a[k][f] != b[k][f]] for k in a if a[k] != b[k]]
    print("BAM records differing:", len(diff), "of", len(a))
    assert not diff, str(diff[:2])[:2000]
    return a


# ---- 1. the committed fixtures ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world(tmp_path_factory):
    d = tmp_path_factory.mktemp("trim_world")
    fa = str(d / "ref.fa")
    TG.write_reference(fa)
    inp = {}
    for tag in ("se", "pe"):
        fq = str(d / (tag + ".fq"))
        with open(fq, "wb") as f:
            f.write(gzip.open(os.path.join(TG.GOLDEN, tag + ".fq.gz"), "rb").read())
        inp[tag] = (["-p"] if tag == "pe" else []) + ["-q", fq]
    return d, fa, inp


@pytest.mark.parametrize("writer", ["sam-gpu", "sam-host", "bam-gpu", "bam-host-records"])
@pytest.mark.parametrize("tag", ["se", "pe"])
def test_fixture_records_equal_the_reference_programs(world, tag, writer):
    d, fa, inp = world
    bam = writer.startswith("bam")
    env = {"sam-host": {"NGM_HIP_HOST_SAM": "1"}, "bam-host-records": {"NGM_HIP_BAM_HOST_RECORDS": "1"}}.get(writer, {})
    out = str(d / ("%s_%s.%s" % (tag, writer, "bam" if bam else "sam")))
    log = _hip(["-r", fa, "-o", out, "--affine"] + TG.TRIM + inp[tag] + (["-b"] if bam else []), env)
    # the estimation pass reads through the parser: lengths behind the -5 prefix, before --max-polya (a read the prefix swallows counts as 1)
    assert ("Average read length: 102 (min: 1, max: 1000)" if tag == "se" else "Average read length: 99 (min: 1, max: 102)") in log, log[:1500]
    assert ("(2 discarded)" in log), log[-2500:]
    if bam:
        assert (GPU_BAM_LINE in log) == (writer == "bam-gpu"), log[-1500:]
        recs = _same_bam(os.path.join(TG.GOLDEN, tag + ".bam"), out, 303 if tag == "se" else 398)
        assert all(b"XAi" in x["tags"] for x in recs.values())
    else:
        assert ("SAM text assembled on the GPU" in log) == (writer == "sam-gpu"), log[-1500:]
        recs = _same_sam(os.path.join(TG.GOLDEN, tag + ".sam.gz"), out, 303 if tag == "se" else 398)
        assert all("\tXA:i:" in l for l in recs.values())
        if tag == "se":
            assert recs[("all_a", 0)] == "all_a\t4\t*\t0\t0\t*\t*\t0\t0\t\t\tXA:i:100\n" and ("short", 0) not in recs and ("exact", 0) not in recs


@pytest.mark.parametrize("fmt", ["sam", "bam"])
@pytest.mark.parametrize("tag", ["se", "pe"])
def test_output_does_not_depend_on_workers(world, tag, fmt):
    d, fa, inp = world
    outs = []
    for w in ("1", "4"):
        out = str(d / ("%s_w%s.%s" % (tag, w, fmt)))
        _hip(["-r", fa, "-o", out, "--affine", "--workers", w, "--batch-size", "1024"] + TG.TRIM + inp[tag] + (["-b"] if fmt == "bam" else []))
        outs.append(decode_bam(out)[1:] if fmt == "bam" else [l for l in open(out) if not l.startswith("@PG")])
    assert outs[0] == outs[1] and len(outs[0]) > 1


@pytest.mark.parametrize("tag", ["se", "pe"])
def test_serial_reader_trims_the_same_way(world, tag):
    """the serial reader (gz, FASTA, multi-line input) writes what the mapped-file route writes"""
    d, fa, inp = world
    out = str(d / (tag + "_serial.sam"))
    _hip(["-r", fa, "-o", out, "--affine", "--serial-reader"] + TG.TRIM + inp[tag])
    _same_sam(os.path.join(TG.GOLDEN, tag + ".sam.gz"), out, 303 if tag == "se" else 398)


# ---- 2. live against the reference program ------------------------------------------------------------------------------
def _tailed(reads, rng, convert=None, all_a=()):
    """reads behind the adapter, every third with a random poly-A tail of 1 .. 40 bases; convert: T>C (second mates: A>G) at 8 %;
    all_a: the reads that are nothing but tail (length 0 after trimming)"""
    out = []
    for i, (name, seq, _) in enumerate(reads):
        s = seq.copy()
        if convert:
            s[(s == ord(convert[0])) & (rng.random(len(s)) < 0.08)] = ord(convert[1])
        if i % 3 == 0:
            s[len(s) - int(rng.integers(1, 41)):] = ord("A")
        if i in all_a:
            s[:] = ord("A")
        s = np.concatenate([np.frombuffer(TG.ADAPTER, np.uint8), s])
        out.append((name, s, bytes(48 + (5 * j + i) % 37 for j in range(len(s)))))
    return out


@pytest.fixture(scope="module")
def live(tmp_path_factory):
    d = tmp_path_factory.mktemp("trim_live")
    contigs = S.make_genome([300000, 200001], seed=931, repeat_families=6, repeat_len=400, copies=4)
    fa = str(d / "ref.fa")
    S.write_fasta(fa, contigs)
    rng = np.random.default_rng(932)
    se, pe = str(d / "se.fq"), str(d / "pe.fq")
    S.write_fastq(se, _tailed(S.make_reads(contigs, 2000, 100, seed=933, sub_rate=0.02, indel_rate=0.003), rng))
    r1, r2 = S.make_reads(contigs, 1000, 100, seed=934, sub_rate=0.02, indel_rate=0.003, paired=True)
    r1, r2 = _tailed(r1, rng), _tailed(r2, rng)
    S.write_fastq(pe, [x for pair in zip(r1, r2) for x in pair])
    S.write_fastq(str(d / "pe_1.fq"), r1)   # (two files: the estimation pass reads the first only)
    S.write_fastq(str(d / "pe_2.fq"), r2)
    return d, fa, {"se": ["-q", se], "pe": ["-p", "-q", pe], "pe2": ["--qry1", str(d / "pe_1.fq"), "--qry2", str(d / "pe_2.fq")]}


@pytest.mark.skipif(not RF.have_reference_binary(), reason="reference binary not built (oracle/ngm_ref.mk)")
@pytest.mark.parametrize("tag,extra", [("se", TG.TRIM), ("pe", TG.TRIM), ("pe2", TG.TRIM), ("pe", TG.TRIM + ["--broken-pairs"]), ("se", TG.TRIM + ["--hard-clip"]),
                                       ("se", TG.TRIM + ["-e"]), ("se", ["-5", "12", "--max-polya", "0"]), ("pe", ["-5", "7", "--max-polya", "0", "-b"])],
                         ids=["se", "pe", "pe-two-files", "pe-broken-pairs", "se-hard-clip", "se-end-to-end", "se-max-polya-0", "pe-max-polya-0-bam"])
def test_live_against_the_reference_program(live, tag, extra):
    d, fa, inp = live
    ident = "_".join(x.strip("-") for x in [tag] + extra)
    ext = "bam" if "-b" in extra else "sam"
    want, got = str(d / ("ref_%s.%s" % (ident, ext))), str(d / ("hip_%s.%s" % (ident, ext)))
    _ref_program(RF.NGM_CORE, fa, ["--affine"] + inp[tag] + extra, want)
    _hip(["-r", fa, "-o", got, "--affine"] + inp[tag] + extra)
    recs = (_same_bam if ext == "bam" else _same_sam)(want, got, 2000 if tag == "se" else None)   # (pairs: the reference loses a few, see ngm_mapper_set_reference_score_buffer)
    assert len(recs) >= 1900
    if tag == "se":
        xa = [int(l.split("\tXA:i:")[1].split()[0]) for l in recs.values()]
        lo = int(extra[extra.index("--max-polya") + 1])
        assert len(xa) == 2000 and sum(1 for x in xa if x > lo) > 300 and all(x == 0 or x > lo for x in xa)


@pytest.mark.parametrize("fmt", ["sam", "bam"])
@pytest.mark.parametrize("tag", ["se", "pe"])
def test_output_does_not_depend_on_workers_over_several_batches(live, tag, fmt):
    """2 000 reads in batches of 1 024: two batches on one worker, on four workers, and the one batch of the default size write the same file"""
    d, fa, inp = live
    outs = []
    for name, extra in (("w1", ["--workers", "1", "--batch-size", "1024"]), ("w4", ["--workers", "4", "--batch-size", "1024"]), ("one", [])):
        out = str(d / ("%s_%s.%s" % (tag, name, fmt)))
        _hip(["-r", fa, "-o", out, "--affine"] + extra + TG.TRIM + inp[tag] + (["-b"] if fmt == "bam" else []))
        outs.append(decode_bam(out)[1:] if fmt == "bam" else [l for l in open(out) if not l.startswith("@PG")])
    assert outs[0] == outs[1] == outs[2]
    n = len(outs[0][1]) if fmt == "bam" else sum(1 for l in outs[0] if not l.startswith("@"))
    assert n >= 1900


@pytest.mark.skipif(not RF.have_reference_binary(), reason="reference binary not built (oracle/ngm_ref.mk)")
def test_trim5_with_argos_equals_the_reference_program(live):
    """`-5` is the parser's and combines with --argos: the prolog and every line (scores of the reads behind the prefix) equal the reference's"""
    d, fa, inp = live
    want, got = str(d / "ref_argos.txt"), str(d / "hip_argos.txt")
    _ref_program(RF.NGM_CORE, fa, ["--affine", "--argos", "-5", "12"] + inp["se"], want)
    _hip(["-r", fa, "-o", got, "--affine", "--argos", "-5", "12"] + inp["se"])
    a, b = open(want, "rb").read(), open(got, "rb").read()
    assert a.split(b"\n")[0] == b"#2000" and a.count(b"\n") > 1900
    diff = [(x, y) for x, y in zip(a.split(b"\n"), b.split(b"\n")) if x != y]
    assert a == b, str(diff[:2])[:1500]


# ---- 3. slamdunk's command against the real program with this library behind IAlignment --------------------------------------
@pytest.fixture(scope="module")
def slam(tmp_path_factory):
    d = tmp_path_factory.mktemp("trim_slam")
    contigs = S.make_genome([300000, 200001], seed=921, repeat_families=6, repeat_len=400, copies=4)
    fa = str(d / "ref.fa")
    S.write_fasta(fa, contigs)
    rng = np.random.default_rng(942)
    se, pe = str(d / "se.fq"), str(d / "pe.fq")
    S.write_fastq(se, _tailed(S.make_reads(contigs, 2500, 100, seed=943, sub_rate=0.01, indel_rate=0.002), rng, "TC", all_a=(7, 1500)))
    r1, r2 = S.make_reads(contigs, 1250, 100, seed=944, sub_rate=0.01, indel_rate=0.002, paired=True)
    S.write_fastq(pe, [x for pair in zip(_tailed(r1, rng, "TC", all_a=(7,)), _tailed(r2, rng, "AG", all_a=(8,))) for x in pair])
    return d, fa, {"se": ["-q", se], "pe": ["-p", "-q", pe]}


needs_dropin = pytest.mark.skipif(not (RF.have_reference_binary() and os.path.exists(DROPIN)), reason="oracle/_ref/dropin/ngm-core-hip not built")


@needs_dropin
@pytest.mark.parametrize("tag", ["se", "pe"])
def test_slamdunk_command_sam_equals_the_real_program(slam, tag):
    d, fa, inp = slam
    want, got = str(d / (tag + "_dropin.sam")), str(d / (tag + "_hip.sam"))
    _ref_program(DROPIN, fa, SLAMDUNK + inp[tag], want)
    log = _hip(["-r", fa, "-o", got, "-t", "4", "--no-progress"] + SLAMDUNK + inp[tag])
    assert "SAM text assembled on the GPU" in log
    recs = _same_sam(want, got, 2500)
    empty = [l for l in recs.values() if l.split("\t")[9] == ""]   # the reads that are all tail: no candidates, written unmapped
    assert len(empty) == 2 and all("\tXA:i:100\tRG:Z:s" in l and int(l.split("\t")[1]) & 4 for l in empty), empty
    mapped = [l for l in recs.values() if not int(l.split("\t")[1]) & 4]
    assert len(mapped) > 0.9 * 2500 and all("\tTC:i:" in l and "\tRA:Z:" in l and "\tXA:i:" in l and "\tRG:Z:s\t" in l for l in mapped)
    assert any("\tMP:Z:" in l for l in mapped) and any("\tMP:Z:" not in l for l in mapped)
    # 8 % of a read's ~25 T (second mates: A) are converted, about two per read; TC counts T>C on forward-strand records and A>G on
    # reverse-strand ones, which is every simulated conversion of a single-end read and those of every other mate of a pair
    tc = sum(int(l.split("\tTC:i:")[1].split("\t")[0]) for l in mapped)
    print("TC summed:", tc)
    assert tc > (2500 if tag == "se" else 1250), "the conversions must be counted"


@needs_dropin
@pytest.mark.parametrize("tag", ["se", "pe"])
def test_slamdunk_command_bam_is_written_by_the_gpu(slam, tag):
    """the command as slamdunk gives it, `-b` included: the records come from the GPU writer (the log says so -- a silent fall-back to the
    host formatter fails here), and decode equal to the real program's and to the host twin's"""
    d, fa, inp = slam
    want, got, twin = str(d / (tag + "_dropin.bam")), str(d / (tag + "_hip.bam")), str(d / (tag + "_hip_host.bam"))
    _ref_program(DROPIN, fa, SLAMDUNK + inp[tag] + ["-b"], want)
    log = _hip(["-r", fa, "-o", got, "-t", "4", "--no-progress"] + SLAMDUNK + inp[tag] + ["-b"])
    assert GPU_BAM_LINE in log and "formatted on the host pool" not in log, log[-2500:]
    log_twin = _hip(["-r", fa, "-o", twin] + SLAMDUNK + inp[tag] + ["-b"], {"NGM_HIP_BAM_HOST_RECORDS": "1"})
    assert GPU_BAM_LINE not in log_twin and "formatted on the host pool" in log_twin
    recs = _same_bam(want, got, 2500)
    assert decode_bam(got)[1:] == decode_bam(twin)[1:]   # (reference dictionary and records, in order; the header text names the output file)
    mapped = [x for x in recs.values() if not x["flag"] & 4]
    assert len(mapped) > 0.9 * 2500 and all(b"TCi" in x["tags"] and b"RAZ" in x["tags"] and b"XAi" in x["tags"] for x in mapped)
    assert any(b"MPZ" in x["tags"] for x in mapped) and any(b"MPZ" not in x["tags"] for x in mapped)
    # the tag block in the reference's order: ... XI XA X0 XE XR MD RG TC RA [MP]
    t = next(x["tags"] for x in mapped if b"MPZ" in x["tags"])
    order = [t.index(k) for k in (b"ASi", b"NMi", b"NHi", b"XIf", b"XAi", b"X0i", b"XEi", b"XRi", b"MDZ", b"RGZs\0", b"TCi", b"RAZ", b"MPZ")]
    assert order == sorted(order) and t.endswith(b"\0")


@needs_dropin
def test_slamdunk_options_with_top3_equal_the_real_program(slam):
    """-n 3 keeps the host formatter; it carries XA:i like every other route"""
    d, fa, inp = slam
    args = [x for x in SLAMDUNK if x not in ("-n", "1", "--strata")] + ["-n", "3"]
    want, got = str(d / "se3_dropin.sam"), str(d / "se3_hip.sam")
    _ref_program(DROPIN, fa, args + inp["se"], want)
    log = _hip(["-r", fa, "-o", got] + args + inp["se"])
    assert "formatted on the host pool" in log
    body = lambda p: sorted(l for l in open(p) if not l.startswith("@"))
    a, b = body(want), body(got)
    assert len(a) >= 2500 and a == b and all("\tXA:i:" in l for l in b)


@needs_dropin
def test_weighted_slam_search_with_trimmed_reads(slam):
    """--slam-seq 6 (the weighted search, csrc/cs_slam_device.h) on trimmed reads, two of them cut to length 0"""
    d, fa, inp = slam
    args = ["--slam-seq", "6"] + SLAMDUNK[2:]
    want, got = str(d / "se6_dropin.sam"), str(d / "se6_hip.sam")
    _ref_program(DROPIN, fa, args + inp["se"], want)
    _hip(["-r", fa, "-o", got] + args + inp["se"])
    recs = _same_sam(want, got, 2500)
    assert sum(1 for l in recs.values() if l.split("\t")[9] == "" and "\tXA:i:100" in l) == 2


# ---- 4. SLAM-seq BAM records without the new options: now the GPU's -------------------------------------------------------------
@pytest.mark.parametrize("tag", ["se", "pe"])
def test_slam_seq_bam_records_on_the_gpu_equal_the_host_twins(slam, tag):
    d, fa, inp = slam
    gpu, host = str(d / (tag + "_slam1_gpu.bam")), str(d / (tag + "_slam1_host.bam"))
    log = _hip(["-r", fa, "-o", gpu, "--slam-seq", "1", "--bam", "--rg-id", "g"] + inp[tag])
    assert GPU_BAM_LINE in log, log[-1500:]
    log = _hip(["-r", fa, "-o", host, "--slam-seq", "1", "--bam", "--rg-id", "g"] + inp[tag], {"NGM_HIP_BAM_HOST_RECORDS": "1"})
    assert GPU_BAM_LINE not in log
    (ta, ra, a), (tb, rb, b) = decode_bam(gpu), decode_bam(host)
    strip = lambda t: [l.split("\tCL:")[0] if l.startswith("@PG") else l for l in t.splitlines()]
    assert strip(ta) == strip(tb) and ra == rb and len(a) == 2500
    bad = [i for i in range(len(a)) if a[i] != b[i]]
    assert not bad, str([(a[i], b[i]) for i in bad[:1]])[:2000]
    assert any(b"MPZ" in x["tags"] for x in a) and all(b"XAi" not in x["tags"] for x in a)


# ---- the C ABI entry through the Python mirror ------------------------------------------------------------------------------------
def test_map_sam_trimmed_entry_point(world):
    """ngm_mapper_map_sam_trimmed through nextgenmap_amd.pipeline: a non-null poly-A array puts XA:i on every record -- an empty read
    (all-NUL row) included, which is written unmapped with empty SEQ and QUAL --, None leaves the records as ngm_mapper_map_sam writes them"""
    from nextgenmap_amd.pipeline import Mapper, Reference
    d, fa, _ = world
    reads = TG.read_fastq_gz(os.path.join(TG.GOLDEN, "se.fq.gz"))[:130]
    seqs = [s[12:] for _, s, _ in reads] + [b"", b"ACGTA"]
    quals = [ql[12:] for _, _, ql in reads] + [b"5" * 100, b"01234"]
    names = [n for n, _, _ in reads] + ["empty", "five"]
    polya = np.arange(len(seqs)) % 7
    ref = Reference.from_fasta(fa)
    m = Mapper(ref, 102, 20, personality=1, gap_read=33, gap_ref=33, gap_extend=3)
    plain, st0 = m.map_sam(seqs, quals, names)
    tagged, st1 = m.map_sam(seqs, quals, names, polya_trimmed=polya)
    m.close()
    ref.close()
    assert st0 == st1 and st0[0] == st0[2] == len(seqs) and st0[1] >= 100
    a, b = plain.decode().splitlines(), tagged.decode().splitlines()
    assert len(a) == len(b) == len(seqs) and not any("XA:i:" in l for l in a)
    for i, (x, y) in enumerate(zip(a, b)):
        f = y.split("\t")
        assert f[0] == names[i] and ("XA:i:%d" % polya[i]) in f
        f.remove("XA:i:%d" % polya[i])
        assert "\t".join(f) == x
        g = y.split("\t")
        at = g.index("XA:i:%d" % polya[i])
        assert at == len(g) - 1 if int(g[1]) & 4 else (g[at - 1].startswith("X0:i:") and g[at + 1].startswith("XE:i:"))
    assert b[-2] == "empty\t4\t*\t0\t0\t*\t*\t0\t0\t\t\tXA:i:%d" % polya[-2]
