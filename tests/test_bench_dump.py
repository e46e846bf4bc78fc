"""bench.py --dump-outputs on CPU (--stub-mapper: the mapping call is a deterministic fake): the timed steps' last outputs
land as float32 / float64 .npy files under 64 MB in all, identical between two runs with the same arguments, and --steps is
the number of timed steps that ms_per_step divides by.  A plain run reports the headline figure alone; the other legs wait for --full."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(tmp_path, steps, dump, extra=()):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--stub-mapper",
           "--genome-mbp", "2", "--reads-per-step", "200000", "--dump-outputs", str(dump)] + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_dump_outputs_are_deterministic_and_bounded(tmp_path):
    a, b, c = tmp_path / "a", tmp_path / "b", tmp_path / "c"
    ja = _bench(tmp_path, 3, a)
    jb = _bench(tmp_path, 3, b)
    jc = _bench(tmp_path, 5, c)
    for j, k in ((ja, 3), (jb, 3), (jc, 5)):
        assert j["steps"] == k and j["ms_per_step"] > 0
        assert abs(j["value"] - 200000 * k / (j["ms_per_step"] * k * 1e-3)) < 1e-6 * j["value"]
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b))
    assert {"rows.npy", "hits_mapped.npy", "hits_pos.npy", "cigar.npy", "md.npy"} <= set(names)
    assert sum(os.path.getsize(a / n) for n in names) <= 64 << 20
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype in (np.float32, np.float64), n
        assert x.dtype == y.dtype and np.array_equal(x, y), n
    rows = np.load(a / "rows.npy")
    assert len(rows) == 65536 and np.all(np.diff(rows) > 0) and rows[-1] < 200000
    assert np.all(rows[0::2] % 2 == 0) and np.array_equal(rows[1::2], rows[0::2] + 1)   # whole pairs
    # the stub maps every read where the simulator put it except global reads 999, 1999, ...
    assert np.array_equal(np.load(a / "hits_mapped.npy"), (rows % 1000 != 999).astype(np.float64))


def test_plain_run_is_the_headline_alone_and_full_changes_no_output(tmp_path):
    """Without --full: no leg beyond the timed steps (fields null or absent); with it: the isolated pass runs (the only extra leg the stub
    has), and the result line's headline fields and the dumped arrays are what the plain run gives."""
    a, b = tmp_path / "a", tmp_path / "b"
    ja = _bench(tmp_path, 3, a)
    jb = _bench(tmp_path, 3, b, ["--full"])
    assert ja["full"] is False and jb["full"] is True
    assert ja["end_to_end"] is None and ja["cpu_baseline"] is None and "heavy_tailed_genome" not in ja
    assert ja["roofline"]["candidate_search"]["isolated"] is None
    assert jb["roofline"]["candidate_search"]["isolated"]["reads"] > 0
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup", "n_gpus", "stats_allreduce", "per_read", "accuracy_rank0_shard"):
        assert ja[k] == jb[k], k
    assert ja["value"] > 0 and ja["ms_per_step"] > 0
    for n in sorted(os.listdir(a)):
        assert np.array_equal(np.load(a / n), np.load(b / n)), n


def test_forked_read_sets_are_the_serial_ones():
    """bench.fork_read_sets (one child process per read set) hands back exactly what make_reads gives in this process."""
    sys.path.insert(0, ROOT)
    import bench
    contigs = bench.make_genome(2_000_000, seed=20240601)
    for paired, kw in ((True, {}), (False, {"subs": 0.12, "indel_bases": 0.03})):
        seeds = [20240604, 20240604 + 7919, 5]
        got = bench.fork_read_sets(contigs, 5001 if not paired else 5000, seeds, paired, **kw)()
        for s_, g in zip(seeds, got):
            want = bench.make_reads(contigs, 5001 if not paired else 5000, seed=s_, paired=paired, **kw)
            assert len(g) == 3
            for x, y in zip(g, want):
                assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y)
                assert x.flags.owndata   # a copy in ordinary memory, not the shared mapping
