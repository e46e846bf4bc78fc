"""-m gpu: `ngm-hip` with the candidate-search options off their defaults (-k, --kmer-skip, --bin-size, --max-kfreq, --kmer-min,
--max-cmrs, -s, and an estimated sensitivity with a non-default k) against golden SAM files captured from the REAL reference program
(`ngm --affine -t 1`, oracle/make_search_cli_goldens.py): record by record, every field.  The inputs are those of
tests/test_gpu_cli_golden.py; no reference binary is needed at test time."""
import gzip
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "nextgenmap_amd", "ngm-hip")
INPUTS = os.path.join(ROOT, "tests", "golden", "cli")
GOLD = os.path.join(ROOT, "tests", "golden", "cli_search")

CASES = [
    ("k12_skip1_bin3_s03", ["-q", "se.fq.gz", "-k", "12", "--kmer-skip", "1", "--bin-size", "3", "-s", "0.3"]),
    ("bin1_kmin3", ["-q", "se.fq.gz", "--bin-size", "1", "--kmer-min", "3"]),
    ("cmrs2_kfreq40", ["-q", "se.fq.gz", "--max-cmrs", "2", "--max-kfreq", "40"]),
    ("pe_k11_skip0_bin4", ["-p", "-q", "pe.fq.gz", "-k", "11", "--kmer-skip", "0", "--bin-size", "4"]),
    ("k10_estimated", ["-q", "se.fq.gz", "-k", "10"]),
]


def _records(lines):
    out = {}
    for line in lines:
        if line.startswith("@"):
            continue
        f = line.rstrip("\n").split("\t")
        out.setdefault((f[0], int(f[1]) & 0xC0), []).append(tuple(f[1:]))
    return {k: sorted(v) for k, v in out.items()}


@pytest.mark.parametrize("case,args", CASES, ids=[c for c, _ in CASES])
def test_sam_equals_golden_reference_output(tmp_path, case, args):
    from nextgenmap_amd import build
    build.build()
    argv = [a if not a.endswith(".gz") else os.path.join(INPUTS, a) for a in args]
    out = str(tmp_path / "out.sam")
    c = subprocess.run([CLI, "-r", os.path.join(INPUTS, "ref.fa.gz"), "-o", out, "--affine", "--skip-save"] + argv, capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr[-2000:]
    want_lines = gzip.open(os.path.join(GOLD, case + ".sam.gz"), "rt").read().splitlines(True)
    got_lines = open(out).read().splitlines(True)
    assert [l for l in want_lines if l.startswith("@SQ")] == [l for l in got_lines if l.startswith("@SQ")]
    want, got = _records(want_lines), _records(got_lines)
    assert set(want) == set(got)
    diff = [(k, want[k], got[k]) for k in want if want[k] != got[k]]
    assert not diff, (len(diff), str(diff[:2])[:1500])
