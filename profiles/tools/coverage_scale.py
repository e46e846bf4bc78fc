"""The coverage object at the size of a human genome, over the ctypes mirror alone (no genome, no mapper): one contig of 3.1 G bases, 2 M random
150 bp alignments added in batches of 2^18, then the finish and the whole bedGraph drained.  Prints the four kernel times (HIP events) and
the bytes per second the scan moved.  python profiles/tools/coverage_scale.py [bases] [alignments]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from nextgenmap_amd import build
from nextgenmap_amd.pipeline import Coverage

HBM = 8.0e12   # the roofline figure of DESIGN.md, bytes per second


def main():
    bases = int(float(sys.argv[1])) if len(sys.argv) > 1 else 3_100_000_000
    n = int(float(sys.argv[2])) if len(sys.argv) > 2 else 2_000_000
    build.build()
    t0 = time.perf_counter()
    cov = Coverage([("chr", bases)])
    t_create = time.perf_counter() - t0
    rng = np.random.default_rng(1)
    pos = rng.integers(0, bases - 150, n).astype(np.int32) if bases < 2**31 else rng.integers(0, 2**31 - 151, n).astype(np.int32)
    step = 1 << 18
    t0 = time.perf_counter()
    for a in range(0, n, step):
        k = min(step, n - a)
        cov.add_arrays(np.zeros(k, dtype=np.int32), pos[a:a + k], np.arange(k + 1, dtype=np.uint32) * 4, b"150M" * k)
    t_add = time.perf_counter() - t0
    t0 = time.perf_counter()
    cov.finish()
    text_bytes = sum(len(p) for p in cov.pieces(64 << 20))
    t_finish = time.perf_counter() - t0
    st = cov.stats()
    cov.close()
    moved = 2 * 4 * (bases + 1)   # the scan reads and writes every counter once
    print("contig of %d bases: %.2f GB of counters, created and zeroed in %.3f s" % (bases, 4 * (bases + 1) / 1e9, t_create))
    print("%d alignments of 150M in batches of %d: %d covered bases, %d runs, %d bytes of bedGraph (%d drained)" %
          (st["alignments"], step, st["covered_bases"], st["runs"], st["text_bytes"], text_bytes))
    print("kernels, ms: add %.3f | scan %.3f | run heads %.3f | text %.3f" % (st["add_ms"], st["scan_ms"], st["runs_ms"], st["text_ms"]))
    print("host wall, s: add calls %.3f (uploads included) | finish + drain %.3f" % (t_add, t_finish))
    rate = moved / (st["scan_ms"] / 1e3)
    print("scan: %.1f GB read + written in %.3f ms = %.2f TB/s, %.0f %% of the %.0f TB/s HBM figure" % (moved / 1e9, st["scan_ms"], rate / 1e12, 100 * rate / HBM, HBM / 1e12))
    gpu = st["scan_ms"] + st["runs_ms"] + st["text_ms"]
    # what the three finish stages move at least: scan 8 B per counter; heads 4 B read + 1 B flag written, select 1 B read; text: per run only
    print("finish kernels together: %.3f ms = %.2f TB/s over the scan's bytes; the largest share is %s" %
          (gpu, moved / (gpu / 1e3) / 1e12, max((st["scan_ms"], "the scan"), (st["runs_ms"], "the run heads (flag kernel + select)"), (st["text_ms"], "the text kernels"))[1]))
    assert st["scan_ms"] > 3.0 or bases < 3_000_000_000, "a scan of 2 x 12.4 GB faster than 3 ms: something was skipped"


if __name__ == "__main__":
    main()
