"""Writes tests/golden/vcf_index_sha256.json: SHA-256 of the -ht-<k>-<skip>.3.ngm file and the `Loaded VCF` / `Built SNP region
table` / `SkipBuild` lines the reference program (oracle/_ref/ngm/ngm-core, built by oracle/ngm_ref.mk) writes with --vcf for the
fixtures of tests/vcf_fixtures.py.  Run from the repository root: python tests/make_vcf_goldens.py"""
import hashlib
import json
import os
import re
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_files as RF  # noqa: E402
import vcf_fixtures as V  # noqa: E402

CASES = {"F1": ("F1", 2, False), "F2": ("F2", 2, False), "F3": ("F3", 2, False), "F1_skip0": ("F1", 0, False), "F1_gz": ("F1", 2, True)}
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vcf_index_sha256.json")


def vcf_lines(log):
    return [m.group(0).strip() for m in re.finditer(r"(Loaded VCF \(\d+ variations\)|Built SNP region table \([^)]*\)|SkipBuild \(\d+\) != SkipCount \(\d+\))", log)]


def make(case, d):
    fx, skip, gz = CASES[case]
    fa, vcf, _ = V.f1(d, gz=True) if gz else V.FIXTURES[fx](d)
    return fa, vcf, skip


def main():
    res = {}
    for case in CASES:
        with tempfile.TemporaryDirectory() as d:
            fa, vcf, skip = make(case, d)
            r = RF.run_ngm(["-r", fa, "--vcf", vcf, "--affine", "-t", "1", "--kmer-skip", str(skip)], cwd=d)
            ht = fa + "-ht-13-%d.3.ngm" % skip
            res[case] = dict(sha256=hashlib.sha256(open(ht, "rb").read()).hexdigest(), lines=vcf_lines(r.stdout + r.stderr))
            print(case, res[case])
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
