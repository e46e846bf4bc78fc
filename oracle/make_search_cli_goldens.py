#!/usr/bin/env python3
"""Golden SAM files for the candidate-search options on the command line: runs the REAL reference program (oracle/_ref/ngm/ngm-core, built
by oracle/ngm_ref.mk) with -k / --kmer-skip / --bin-size / --max-kfreq / --kmer-min / --max-cmrs / -s off their defaults on the inputs
oracle/make_cli_goldens.py left under tests/golden/cli/ (which this script does not rewrite) and stores the records under
tests/golden/cli_search/.  Runs on the CPU; tests/test_gpu_cli_search_options.py compares `ngm-hip` with these files."""
import gzip
import os
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_files as RF  # noqa: E402

IN = os.path.join(ROOT, "tests", "golden", "cli")
OUT = os.path.join(ROOT, "tests", "golden", "cli_search")
# (the last one has no -s: the estimated sensitivity and its "%f" round trip through a non-default k)
CASES = {
    "k12_skip1_bin3_s03": ["-q", "se.fq.gz", "-k", "12", "--kmer-skip", "1", "--bin-size", "3", "-s", "0.3"],
    "bin1_kmin3": ["-q", "se.fq.gz", "--bin-size", "1", "--kmer-min", "3"],
    "cmrs2_kfreq40": ["-q", "se.fq.gz", "--max-cmrs", "2", "--max-kfreq", "40"],
    "pe_k11_skip0_bin4": ["-p", "-q", "pe.fq.gz", "-k", "11", "--kmer-skip", "0", "--bin-size", "4"],
    "k10_estimated": ["-q", "se.fq.gz", "-k", "10"],
}


def main():
    assert RF.have_reference_binary(), "build the reference first: make -f oracle/ngm_ref.mk"
    os.makedirs(OUT, exist_ok=True)
    with tempfile.TemporaryDirectory() as d:
        for name in ("ref.fa", "se.fq", "pe.fq"):
            with gzip.open(os.path.join(IN, name + ".gz"), "rb") as a, open(os.path.join(d, name), "wb") as b:
                shutil.copyfileobj(a, b)
        for case, args in CASES.items():
            sub = os.path.join(d, case)   # (a directory of its own: the index cache files carry k and skip, not the bin size)
            os.makedirs(sub)
            shutil.copy(os.path.join(d, "ref.fa"), os.path.join(sub, "ref.fa"))
            argv = [a if not a.endswith(".gz") else os.path.join(d, a[:-3]) for a in args]
            out = os.path.join(sub, "out.sam")
            r = RF.run_ngm(["-r", os.path.join(sub, "ref.fa"), "-o", out, "--affine", "-t", "1", "--no-progress"] + argv, cwd=sub)
            assert "Done" in (r.stdout + r.stderr), r.stdout + r.stderr
            n = 0
            with open(out) as f, gzip.GzipFile(os.path.join(OUT, case + ".sam.gz"), "wb", mtime=0) as g:
                for line in f:
                    if not line.startswith("@PG"):
                        g.write(line.encode())
                        n += not line.startswith("@")
            print(case, n, "records")


if __name__ == "__main__":
    main()
