"""-m gpu: `ngm-hip --vcf` builds the index with the k-mers of known variants on the GPU.  The -ht-13-<skip>.3.ngm cache it writes is
byte-identical to the one the reference program writes with --vcf (SHA-256 digests in tests/golden/vcf_index_sha256.json, made by
tests/make_vcf_goldens.py; live against oracle/_ref/ngm/ngm-core where it is built) -- including F2's zero slot, F3's variants cut at a
mismatching indel, --kmer-skip 0, a .vcf.gz and the forced host walk -- and so are the reference's log lines; SAM records against
ngm-core --affine -t 1 --vcf; an existing cache is loaded as it is."""
import hashlib
import json
import os
import subprocess

import pytest

import ref_files as RF
import simulate as S
import vcf_fixtures as V
from make_vcf_goldens import CASES, make, vcf_lines

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "nextgenmap_amd", "ngm-hip")
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "vcf_index_sha256.json")))


def _hip(args, env=None, cwd=None):
    r = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=900, cwd=cwd, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout + r.stderr


def _sha(p):
    return hashlib.sha256(open(p, "rb").read()).hexdigest()


@pytest.mark.parametrize("case,host_walk", [(c, False) for c in CASES] + [("F2", True), ("F1", True)],
                         ids=[c for c in CASES] + ["F2-host-walk", "F1-host-walk"])
def test_vcf_index_cache_is_the_references(tmp_path, case, host_walk):
    fa, vcf, skip = make(case, str(tmp_path))
    env = {"NGM_HIP_TEST_LIMITS": "host_walk=1"} if host_walk else None
    log = _hip(["-r", fa, "--vcf", vcf, "--kmer-skip", str(skip)], env=env)
    ht = fa + "-ht-13-%d.3.ngm" % skip
    assert os.path.exists(ht), (sorted(os.listdir(str(tmp_path))), log[-3000:])
    assert _sha(ht) == GOLD[case]["sha256"], log[-2000:]
    assert vcf_lines(log) == GOLD[case]["lines"], log[-2000:]
    if RF.have_reference_binary() and not host_walk:
        d = tmp_path / "ref"
        d.mkdir()
        fa2, vcf2, _ = make(case, str(d))
        RF.run_ngm(["-r", fa2, "--vcf", vcf2, "--affine", "-t", "1", "--kmer-skip", str(skip)], cwd=str(d))
        assert open(ht, "rb").read() == open(fa2 + "-ht-13-%d.3.ngm" % skip, "rb").read()


def test_vcf_summary_python(tmp_path):
    from nextgenmap_amd import pipeline as N
    fa, vcf, _ = V.f2(str(tmp_path))
    os.environ["NGM_HIP_NO_CACHE"] = "1"
    try:
        ref = N.Reference.from_fasta(fa, vcf=vcf)
        plain = N.Reference.from_fasta(fa)
    finally:
        del os.environ["NGM_HIP_NO_CACHE"]
    s = ref.vcf_summary()
    assert s["variations"] == 5 and s["snps"] == 0 and s["indels"] == 5 and s["ignored"] == 0
    assert s["zero_slots"] == 1 and s["entries"] > 0
    assert plain.vcf_summary() is None
    assert ref.lib.ngm_ref_index_entries(ref.h) == ref.lib.ngm_ref_index_entries(plain.h) + s["entries"] + s["zero_slots"]
    ref.close(); plain.close()


def _records(path):
    return sorted(l for l in open(path) if not l.startswith("@"))


DROPIN = os.path.join(ROOT, "oracle", "_ref", "dropin", "ngm-core-hip")


@pytest.mark.skipif(not RF.have_reference_binary(), reason="reference binary not built (oracle/ngm_ref.mk)")
@pytest.mark.parametrize("personality", ["affine", "linear"])
@pytest.mark.parametrize("paired", [False, True], ids=["SE", "PE"])
@pytest.mark.parametrize("fixture", ["F1", "F2"])
def test_vcf_sam_equals_reference(tmp_path, fixture, paired, personality):
    """half of the reads carry the VCF's ALT alleles; --affine against ngm-core -t 1, the linear personality against the real program
    with this library behind IAlignment (oracle/_ref/dropin/ngm-core-hip); with the variants the SAM differs from the one without"""
    if personality == "linear" and not os.path.exists(DROPIN):
        pytest.skip("oracle/_ref/dropin/ngm-core-hip not built")
    fa, vcf, contigs = V.FIXTURES[fixture](str(tmp_path))
    reads = V.reads_with_alts(contigs, vcf, 1600, seed=91, paired=paired)
    if paired:
        fq = [str(tmp_path / "r1.fq"), str(tmp_path / "r2.fq")]
        S.write_fastq(fq[0], reads[0])
        S.write_fastq(fq[1], reads[1])
        qa = ["-1", fq[0], "-2", fq[1]]
    else:
        fq = str(tmp_path / "r.fq")
        S.write_fastq(fq, reads)
        qa = ["-q", fq]
    pa = ["--affine"] if personality == "affine" else []
    d = tmp_path / "ref"
    d.mkdir()
    fa2, vcf2, _ = V.FIXTURES[fixture](str(d))
    want = str(tmp_path / "want.sam")
    exe = RF.NGM_CORE if personality == "affine" else DROPIN
    r = subprocess.run([exe, "-r", fa2, "--vcf", vcf2, "-o", want, "-t", "1", "--no-progress"] + qa + pa, capture_output=True, text=True,
                       cwd=str(d), timeout=1800)
    assert r.returncode == 0, r.stderr[-2000:]
    got = str(tmp_path / "got.sam")
    _hip(["-r", fa, "--vcf", vcf, "-o", got, "--no-progress"] + qa + pa)
    assert _records(got) == _records(want)
    # the same reads against an index without the variants (a fresh FASTA copy: no cache)
    d3 = tmp_path / "plain"
    d3.mkdir()
    fa3, _, _ = V.FIXTURES[fixture](str(d3))
    nov = str(tmp_path / "nov.sam")
    _hip(["-r", fa3, "-o", nov, "--no-progress"] + qa + pa)
    if fixture == "F1":
        assert _records(nov) != _records(got)
    # loading the cache the reference wrote with --vcf, without --vcf, gives the reference's SAM
    if personality == "affine":
        got2 = str(tmp_path / "got2.sam")
        _hip(["-r", fa2, "-o", got2, "--no-progress"] + qa + pa)
        assert _records(got2) == _records(want)


def test_vcf_with_existing_cache_is_not_applied(tmp_path):
    fa, vcf, _ = V.f2(str(tmp_path))
    _hip(["-r", fa])                                 # a cache without the variants
    before = _sha(fa + "-ht-13-2.3.ngm")
    log = _hip(["-r", fa, "--vcf", vcf])
    assert "not applied" in log and "Loaded VCF" not in log
    assert _sha(fa + "-ht-13-2.3.ngm") == before != GOLD["F2"]["sha256"]
