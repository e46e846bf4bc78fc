"""-m gpu: `ngm-hip --argos` (ScoreWriter's lines: every scored candidate of a read, ordered on the GPU) against the REAL reference
program -- byte-identical output files and the same `Done` line -- with --affine (ngm-core) and with the linear-gap personality (the real
program with this library behind IAlignment, oracle/_ref/dropin/ngm-core-hip); the order classes and the long-list path through the
library's counters; Mapper.map_argos against the command line."""
import os
import re
import subprocess

import numpy as np
import pytest

import ref_files as RF
import simulate as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "nextgenmap_amd", "ngm-hip")
DROPIN = os.path.join(ROOT, "oracle", "_ref", "dropin", "ngm-core-hip")
needs_ref = pytest.mark.skipif(not RF.have_reference_binary(), reason="reference binary not built (oracle/ngm_ref.mk)")
needs_dropin = pytest.mark.skipif(not (RF.have_reference_binary() and os.path.exists(DROPIN)), reason="oracle/_ref/dropin/ngm-core-hip not built")


def _case(tmp_path, n_reads=3000):
    """a repeat-rich two-contig genome (as test_cli_topn_sam_equals_reference_program) and reads of which some cross the start of chr2"""
    contigs = S.make_genome([200000, 150001], seed=61, repeat_families=12, repeat_len=600, copies=8, divergence=0.03)
    fa = str(tmp_path / "ref.fa")
    with open(fa, "wb") as f:
        for i, g in enumerate(contigs):
            f.write(b">chr%d\n" % (i + 1))
            b = g.tobytes()
            for o in range(0, len(b), 70):
                f.write(b[o:o + 70] + b"\n")
    reads = S.make_reads(contigs, n_reads, 100, seed=62, sub_rate=0.02, indel_rate=0.003)
    rng = np.random.default_rng(63)
    for j in range(60):   # the end of chr1 + the start of chr2, forward and reverse: candidates in the spacer before chr2
        k = int(rng.integers(10, 90))
        seq = np.concatenate([contigs[0][len(contigs[0]) - k:], contigs[1][:100 - k]]).astype(np.uint8)
        if j & 1:
            seq = np.frombuffer(bytes(seq)[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA")), np.uint8).copy()
        reads.append(("junction%d" % j, seq, b"I" * 100))
    fq = str(tmp_path / "reads.fq")
    S.write_fastq(fq, reads)
    return fa, fq, len(reads)


def _done(log):
    m = re.search(r"Done \((.*?lines written)\)", log)
    assert m, log[-2000:]
    return m.group(1)


def _reference(binary, tmp_path, fa, fq, extra, out):
    d1 = tmp_path / ("run_" + os.path.basename(binary))
    d1.mkdir(exist_ok=True)
    fa1 = str(d1 / "ref.fa")
    if not os.path.exists(fa1):
        os.link(fa, fa1)
    r = subprocess.run([binary, "-r", fa1, "-q", fq, "-o", out, "--argos", "-t", "1", "--no-progress"] + extra, capture_output=True, text=True,
                       cwd=str(d1), timeout=1800)
    log = r.stdout + r.stderr
    assert "Done" in log, log[-2500:]
    return log


def _hip(fa, fq, extra, out, env=None):
    e = dict(os.environ)
    e.update(env or {})
    c = subprocess.run([CLI, "-r", fa, "-q", fq, "-o", out, "--argos"] + extra, capture_output=True, text=True, env=e, timeout=1800)
    assert c.returncode == 0, c.stderr[-2500:]
    return c.stderr


def _classes(log):
    m = re.search(r"Argos order classes: U (\d+) .*?, S (\d+) .*?, H (\d+) .*?; (\d+) entries written; long-list path (\d+) reads; order by position \(candidate order unknown\) (\d+) reads", log)
    assert m, log[-2000:]
    return [int(x) for x in m.groups()]


def _same_file(a, b):
    x, y = open(a, "rb").read(), open(b, "rb").read()
    if x != y:
        la, lb = x.split(b"\n"), y.split(b"\n")
        diff = [(p, q) for p, q in zip(la, lb) if p != q]
        print("lines:", len(la), len(lb), "differing:", len(diff))
        for d in diff[:3]:
            print(str(d)[:800])
    return x == y


@needs_ref
@pytest.mark.parametrize("extra", [[], ["--argos-min-score", "0.5"], ["--argos-min-score", "420"], ["-e"]],
                         ids=["no-filter", "min-score-share", "min-score-absolute", "end-to-end"])
def test_argos_affine_equals_reference_program(tmp_path, extra):
    fa, fq, n = _case(tmp_path)
    ref_out, hip_out = str(tmp_path / "ref.txt"), str(tmp_path / "hip.txt")
    log_ref = _reference(RF.NGM_CORE, tmp_path, fa, fq, ["--affine"] + extra, ref_out)
    log_hip = _hip(fa, fq, ["--affine"] + extra, hip_out)
    assert _same_file(ref_out, hip_out)
    assert _done(log_ref) == _done(log_hip)
    u, s, h, entries, _, unknown = _classes(log_hip)
    print("classes U/S/H:", u, s, h, "entries:", entries, "unknown order:", unknown)
    lines = open(hip_out, "rb").read().split(b"\n")
    assert lines[0] == b"#%d" % n and lines[1].startswith(b"#0:chr1\t1:chr2\t")
    assert any(b"\t1:0:" in l for l in lines if l.startswith(b"junction")), "no candidate clamped to the start of chr2"


@needs_dropin
def test_argos_linear_equals_reference_program_with_this_library(tmp_path):
    fa, fq, _ = _case(tmp_path, n_reads=2000)
    ref_out, hip_out = str(tmp_path / "ref.txt"), str(tmp_path / "hip.txt")
    log_ref = _reference(DROPIN, tmp_path, fa, fq, [], ref_out)
    log_hip = _hip(fa, fq, [], hip_out)
    assert _same_file(ref_out, hip_out)
    assert _done(log_ref) == _done(log_hip)


def test_argos_classes_and_the_long_list_path(tmp_path):
    fa, fq, _ = _case(tmp_path)
    a, b = str(tmp_path / "a.txt"), str(tmp_path / "b.txt")
    log_a = _hip(fa, fq, ["--affine"], a)
    u, s, h, entries, long_a, _ = _classes(log_a)
    print("classes U/S/H:", u, s, h, "entries:", entries, "long-list reads:", long_a)
    assert u > 0 and s > 0 and h > 0 and entries > 0
    # an LDS cap of 8 keys: every read with more than 8 candidates is ordered by the long-list path -- the same file
    log_b = _hip(fa, fq, ["--affine", "-g", "0", "--workers", "1"], b, env={"NGM_HIP_TEST_LIMITS": "argos_lds_cap=8"})
    assert _classes(log_b)[:4] == [u, s, h, entries]
    assert _classes(log_b)[4] > 0
    assert open(a, "rb").read() == open(b, "rb").read()
    assert _done(log_a) == _done(log_b)


def test_argos_python_mapper_equals_cli(tmp_path):
    from nextgenmap_amd.pipeline import Mapper, Reference
    fa, fq, n = _case(tmp_path, n_reads=1500)
    out = str(tmp_path / "hip.txt")
    log = _hip(fa, fq, ["--affine", "--argos-min-score", "0.5"], out)
    q = int(re.search(r"Average read length: \d+ \(min: \d+, max: (\d+)\)", log).group(1))
    corridor = int(re.search(r"Corridor width: (\d+)", log).group(1))
    recs = []
    with open(fq, "rb") as f:
        while True:
            h = f.readline()
            if not h:
                break
            seq = f.readline().rstrip(b"\n")
            f.readline(); f.readline()
            recs.append((h[1:].split()[0], seq))
    ref = Reference.from_fasta(fa)
    m = Mapper(ref, q, corridor, sensitivity=0.0, kmer_min=2.0, gap_read=33, gap_ref=33, gap_extend=3, personality=1)   # the --affine personality
    text, stats = m.map_argos([r[1] for r in recs], [r[0] for r in recs], min_score=0.5)
    body = b"".join(l + b"\n" for l in open(out, "rb").read().split(b"\n")[2:] if l)
    assert text == body
    assert stats[0] == n and stats[1] == text.count(b"\n")
    assert ref.argos_prolog(n) == b"".join(l + b"\n" for l in open(out, "rb").read().split(b"\n")[:2])
    m.close()
    ref.close()
