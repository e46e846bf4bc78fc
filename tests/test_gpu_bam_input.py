"""-m gpu: `ngm-hip -q reads.bam` / reads.sam / bgzipped FASTQ.  A BAM or SAM of unaligned records (tests/bam_fixtures.py) must map
exactly as the FASTQ file of the same reads does -- every SAM record equal --, on the GPU inflate route (bgzf_inflate_device.h) and on
the host twin (NGM_HIP_BGZF_INFLATE_HOST=1), and as the real program maps it (live where it is built, and against the records
committed under tests/golden/bam_input by tests/make_bam_input_goldens.py)."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import bam_fixtures as BF
import make_bam_input_goldens as BG
import make_trim_goldens as TG
import ref_files as RF
import simulate as S
from test_gpu_bam import decode_bam

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "nextgenmap_amd", "ngm-hip")
DROPIN = os.path.join(ROOT, "oracle", "_ref", "dropin", "ngm-core-hip")
GPU_LINE = "BGZF blocks inflated on the GPU"
HOST = {"NGM_HIP_BGZF_INFLATE_HOST": "1"}
SLAMDUNK = ["--slam-seq", "2", "-5", "12", "--max-polya", "4", "-l", "--rg-id", "s", "--rg-sm", "s:pulse:0", "-n", "1", "--strata"]


def _hip(args, env=None, fails=False):
    c = subprocess.run([CLI] + args, capture_output=True, text=True, env=dict(os.environ, **(env or {})))
    if fails:
        assert c.returncode == 1, "returncode=%d\n%s" % (c.returncode, c.stderr[-2500:])
    else:
        assert c.returncode == 0, "returncode=%d\n%s" % (c.returncode, c.stderr[-2500:])
    return c.stderr


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """the genome of test_gpu_bam.py; 2 000 single-end reads and 1 000 pairs of 100 bp, some with an N or a lower-case stretch"""
    d = tmp_path_factory.mktemp("bam_input")
    contigs = S.make_genome([400000, 300001], seed=801, repeat_families=10, repeat_len=500, copies=6)
    fa = str(d / "ref.fa")
    S.write_fasta(fa, contigs)
    rng = np.random.default_rng(9)
    qual = lambda n, i: bytes(48 + (7 * j + i) % 37 for j in range(n))
    se = [(n.encode(), s.tobytes(), qual(len(s), i)) for i, (n, s, _) in enumerate(S.make_reads(contigs, 2000, 100, seed=811, sub_rate=0.02, indel_rate=0.003))]
    for k in range(0, 40, 2):   # reads that map nowhere
        se[k] = (se[k][0], S.ACGT[rng.integers(0, 4, 100)].tobytes(), se[k][2])
    for k in range(1, 40, 2):   # lower-case bases: the row is upper-cased, the record shows the read as given
        se[k] = (se[k][0], se[k][1][:30] + se[k][1][30:60].lower() + se[k][1][60:], se[k][2])
    r1, r2 = S.make_reads(contigs, 1000, 100, seed=812, sub_rate=0.02, indel_rate=0.003, paired=True)
    pe = [(n.encode(), s.tobytes(), qual(len(s), i)) for i, pair in enumerate(zip(r1, r2)) for n, s, _ in pair]
    files = {}
    for tag, reads in (("se", se), ("pe", pe)):
        fq = b"".join(b"@" + n + b"\n" + s + b"\n+\n" + q + b"\n" for n, s, q in reads)
        sam = BF.sam_text(reads, tag == "pe", 3)
        for name, data in ((".fq", fq), (".bam", BF.unaligned_bam(reads, tag == "pe", member_size=4000 if tag == "se" else 0xFF00)), (".sam", sam), (".sam.gz", gzip.compress(sam)),
                           (".fq.gz", BF.bgzf(fq, 0xFF00)), (".sam.bgz", BF.bgzf(sam, 30011))):
            files[tag + name] = str(d / (tag + name))
            with open(files[tag + name], "wb") as f:
                f.write(data)
    # (BAM with lower-case bases does not exist: the 4-bit codes have no case.  The BAM of the single-end reads holds them upper-cased,
    # and so does the FASTQ it is compared with)
    upper = [(n, s.upper(), q) for n, s, q in se]
    files["se_upper.fq"] = str(d / "se_upper.fq")
    with open(files["se_upper.fq"], "wb") as f:
        f.write(b"".join(b"@" + n + b"\n" + s + b"\n+\n" + q + b"\n" for n, s, q in upper))
    return d, fa, files, {}


def _run(world, name, opts, env=None, ext="sam"):
    """ngm-hip on world file `name` with `opts`; the runs are kept, so that the FASTQ twin of a case is mapped once"""
    d, fa, files, cache = world
    key = (name, tuple(opts), tuple(sorted((env or {}).items())))
    if key not in cache:
        out = str(d / ("out%d.%s" % (len(cache), ext)))
        paired = ["-p"] if name.startswith("pe") else []
        cache[key] = (out, _hip(["-r", fa, "-o", out] + paired + ["-q", files[name]] + list(opts), env))
    return cache[key]


def _body(path):
    return [l for l in open(path) if not l.startswith("@PG")]


def _fq_twin(name):
    return "se_upper.fq" if name == "se.bam" else name.split(".")[0] + ".fq"


CASES = {"se-affine": ("se", ["--affine"]), "se-linear": ("se", []), "pe-affine": ("pe", ["--affine"]), "pe-linear": ("pe", []),
         "se-trim": ("se", ["--affine", "-5", "12", "--max-polya", "4"]), "pe-trim": ("pe", ["-5", "12", "--max-polya", "4"]),
         "se-bam-output": ("se", ["--affine", "--bam"]), "pe-bam-output": ("pe", ["--affine", "--bam"]), "se-argos": ("se", ["--argos"])}


@pytest.mark.parametrize("case", list(CASES))
def test_bam_input_maps_like_the_fastq_of_the_same_reads(world, case):
    tag, opts = CASES[case]
    ext = "bam" if "--bam" in opts else "sam"
    got, log = _run(world, tag + ".bam", opts, ext=ext)
    want, log_fq = _run(world, _fq_twin(tag + ".bam"), opts, ext=ext)
    assert "Input is BAM" in log and GPU_LINE in log and "Input is BAM" not in log_fq and GPU_LINE not in log_fq
    length = lambda l: [x for x in l.splitlines() if "Average read length" in x]
    assert length(log) == length(log_fq) and length(log)
    if ext == "bam":
        assert decode_bam(got)[1:] == decode_bam(want)[1:]
        assert len(decode_bam(got)[2]) == 2000
    else:
        a, b = _body(got), _body(want)
        assert a == b and sum(1 for l in a if not l.startswith("@") and not l.startswith("#")) >= 1900


def test_own_bam_output_fed_back_in(world):
    """`ngm-hip --bam` writes mapped records, half of them on the reverse strand (flag 0x10, sequence reverse-complemented, qualities
    reversed): read back they are the reads again, and map to the same records"""
    first, _ = _run(world, "se_upper.fq", ["--affine", "--bam"], ext="bam")
    recs = decode_bam(first)[2]
    assert sum(1 for x in recs if x["flag"] & 0x10) > 500
    d, fa, files, _ = world
    files["fed_back.bam"] = first
    got, log = _run(world, "fed_back.bam", ["--affine"])
    want, _ = _run(world, "se_upper.fq", ["--affine"])
    assert "Input is BAM" in log and _body(got) == _body(want)


@pytest.mark.parametrize("name", ["se.sam", "se.sam.gz", "se.sam.bgz", "pe.sam", "se.fq.gz", "pe.fq.gz"])
def test_sam_and_bgzipped_inputs_map_like_the_fastq(world, name):
    got, log = _run(world, name, ["--affine"])
    want, _ = _run(world, _fq_twin(name), ["--affine"])
    assert ("Input is SAM" in log) == (".sam" in name)
    assert (GPU_LINE in log) == (name in ("se.sam.bgz", "se.fq.gz", "pe.fq.gz")), log[:3000]
    a = _body(got)
    assert a == _body(want) and len(a) > 1900


@pytest.mark.parametrize("name", ["se.bam", "pe.bam", "se.fq.gz", "se.sam.bgz"])
def test_gpu_inflate_and_host_twin_write_the_same_file(world, name):
    gpu, log_gpu = _run(world, name, ["--affine"])
    host, log_host = _run(world, name, ["--affine"], HOST)
    assert GPU_LINE in log_gpu and GPU_LINE not in log_host
    assert log_gpu.count(GPU_LINE) == 1
    a, b = open(gpu, "rb").read(), open(host, "rb").read()
    assert a.replace(gpu.encode(), b"OUT") == b.replace(host.encode(), b"OUT") and a.count(b"\n") > 1900   # (the @PG line names the output file)


@pytest.mark.parametrize("name", ["se.bam", "pe.bam", "se.sam"])
def test_output_does_not_depend_on_batches_and_workers(world, name):
    one, _ = _run(world, name, ["--affine"])
    many, _ = _run(world, name, ["--affine", "--batch-size", "700", "--workers", "3"])
    assert _body(one) == _body(many)
    par, _ = _run(world, name, ["--affine", "--parse-all"])   # accepted, and the default
    assert _body(one) == _body(par)


def test_a_damaged_member_sends_the_file_to_the_host_reader(world):
    """a member the GPU refuses (a wrong CRC): the whole file goes down the host's path, whose message the user sees"""
    d, fa, files, _ = world
    z = bytearray(open(files["se.bam"], "rb").read())
    first = int.from_bytes(z[16:18], "little") + 1
    z[first - 8] ^= 1   # the CRC-32 of the first member
    files["bad_crc.bam"] = str(d / "bad_crc.bam")
    open(files["bad_crc.bam"], "wb").write(bytes(z))
    log = _hip(["-r", fa, "-o", str(d / "bad.sam"), "-q", files["bad_crc.bam"]], fails=True)
    assert "member 0 refused" in log and GPU_LINE not in log and "[ngm-hip] error:" in log


def test_damaged_records_are_a_clean_error(world):
    d, fa, files, _ = world
    good = [BF.bam_record(b"ok%d" % i, b"ACGTACGTAC" * 5, b"I" * 50, 4) for i in range(30)]
    bad = bytearray(BF.bam_record(b"bad", b"ACGTACGTAC" * 5, b"I" * 50, 4))
    bad[12] = 0   # l_read_name
    for tag, recs, msg in (("name0", good + [bytes(bad)] + good, "l_read_name is 0"), ("truncated", good + [good[0][:-9]], "block_size runs past the end")):
        p = str(d / (tag + ".bam"))
        open(p, "wb").write(BF.bgzf(BF.bam_bytes(recs), 700))
        for env in ({}, HOST):
            log = _hip(["-r", fa, "-o", str(d / "bad.sam"), "-q", p], env, fails=True)
            assert "[ngm-hip] error: BAM input: " + msg in log, log[-1500:]


@pytest.mark.parametrize("opts,msg", [(["--keep-tags"], "option --keep-tags is not supported"), (["--broken-pairs", "-p"], "cannot be combined with --broken-pairs"),
                                      (["--shard", "0/2"], "cannot be combined with --shard"), (["--shard-output"], "cannot be combined with --shard-output")])
@pytest.mark.parametrize("name", ["se.bam", "se.sam"])
def test_refusals(world, name, opts, msg):
    d, fa, files, _ = world
    log = _hip(["-r", fa, "-o", str(d / "refused.sam"), "-q", files[name]] + opts, fails=True)
    assert msg in log and "Input is " + ("BAM" if name == "se.bam" else "SAM") in log and "index entries" not in log   # (before any GPU work)


def test_two_file_input_is_refused_and_bgzipped_fastq_is_not(world):
    d, fa, files, _ = world
    log = _hip(["-r", fa, "-o", str(d / "refused.sam"), "--qry1", files["se.bam"], "--qry2", files["se.bam"]], fails=True)
    assert "cannot be combined with --qry1/--qry2" in log
    out = str(d / "two_bgzipped.sam")
    log = _hip(["-r", fa, "-o", out, "--affine", "--keep-tags", "--qry1", files["se.fq.gz"], "--qry2", files["se.fq.gz"]])
    assert log.count(GPU_LINE) == 1 and sum(1 for l in open(out) if not l.startswith("@")) == 4000


# ---- against the real program -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["se.bam", "se.sam.gz", "pe.bam", "pe.sam.gz"])
def test_committed_inputs_map_as_the_reference_program_mapped_them(tmp_path, name):
    fa = str(tmp_path / "ref.fa")
    TG.write_reference(fa)
    out = str(tmp_path / "out.sam")
    log = _hip(["-r", fa, "-o", out, "--affine"] + (["-p"] if name.startswith("pe") else []) + ["-q", os.path.join(BG.GOLDEN, name)])
    assert ("Input is BAM" if name.endswith(".bam") else "Input is SAM") in log
    a, b = TG.sam_records(os.path.join(BG.GOLDEN, name + ".out.sam.gz")), TG.sam_records(out)
    assert len(a) == 300 and a == b


def _ref_program(binary, fa, args, out):
    own = os.path.join(os.path.dirname(fa), "refrun")   # (a link of its own: the programs do not share index cache files)
    os.makedirs(own, exist_ok=True)
    if not os.path.exists(os.path.join(own, "ref.fa")):
        os.link(fa, os.path.join(own, "ref.fa"))
    r = subprocess.run([binary, "-r", os.path.join(own, "ref.fa"), "-o", out, "-t", "1", "--no-progress"] + args, capture_output=True, text=True, cwd=own, timeout=600)
    assert "Done" in (r.stdout + r.stderr), (r.stdout + r.stderr)[-2500:]


@pytest.mark.skipif(not RF.have_reference_binary(), reason="reference binary not built (oracle/ngm_ref.mk)")
@pytest.mark.parametrize("tag", ["se", "pe"])
def test_live_against_the_reference_program(world, tag):
    d, fa, files, _ = world
    want = str(d / (tag + "_ref.sam"))
    _ref_program(RF.NGM_CORE, fa, ["--affine"] + (["-p"] if tag == "pe" else []) + ["-q", files[tag + ".bam"]], want)
    got, _ = _run(world, tag + ".bam", ["--affine"])
    a, b = TG.sam_records(want), TG.sam_records(got)
    assert set(a) == set(b) and len(a) >= 1900   # (pairs: the reference loses a few, see ngm_mapper_set_reference_score_buffer)
    assert not [(a[k], b[k]) for k in a if a[k] != b[k]][:2]


@pytest.mark.skipif(not (RF.have_reference_binary() and os.path.exists(DROPIN)), reason="oracle/_ref/dropin/ngm-core-hip not built")
def test_slamdunk_command_with_bam_input(world):
    d, fa, files, _ = world
    want = str(d / "slam_ref.bam")
    _ref_program(DROPIN, fa, SLAMDUNK + ["-q", files["se.bam"], "-b"], want)
    got, log = _run(world, "se.bam", ["-t", "4", "--no-progress"] + SLAMDUNK + ["-b"], ext="bam")
    assert GPU_LINE in log and "BAM records and their BGZF blocks written on the GPU" in log
    (ta, ra, a), (tb, rb, b) = TG.bam_records(want), TG.bam_records(got)
    assert ra == rb and len(a) == 2000 and a == b
