#!/usr/bin/env python3
"""Golden ABI facts of the drop-in boundary: compiles tests/cpp/abi_probe.cpp against the reference's own
IAlignment.h / IConfig.h / ILog.h (read in place under $NGM_REFERENCE/include, nothing is copied) and stores what it
prints -- vtable slots, struct sizes and offsets, cCookie -- as tests/golden/ialignment_abi.json.  Runs on CPU in the
build container; tests/test_boundary.py then checks include/ngm_ialignment.h against this file even where the
reference tree is absent."""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get("NGM_REFERENCE", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden", "ialignment_abi.json")


def main():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "abi_probe_ref")
        subprocess.check_call(["g++", "-std=gnu++11", "-w", "-DABI_PROBE_REFERENCE", os.path.join(ROOT, "tests", "cpp", "abi_probe.cpp"),
                               "-I", os.path.join(REFERENCE, "include"), "-o", exe])
        facts = json.loads(subprocess.check_output([exe]).decode())
    with open(OUT, "w") as f:
        json.dump(facts, f, indent=1)
        f.write("\n")
    print("%s: %d entries" % (OUT, len(facts)))


if __name__ == "__main__":
    sys.exit(main())
