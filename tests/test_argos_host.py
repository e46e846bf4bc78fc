"""Host logic, no GPU: `ngm-hip --argos` refuses the combinations it does not support before any GPU work, and the ordering of
`--argos` (ScoreBuffer.cpp:150-183: filter, std::sort(sortLocationScore) over the candidates in the reference's candidate order) through
the host-only entry ngm_debug_argos_order against libstdc++'s std::sort restated in tests/test_pair_walk.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_pair_walk import StdSort, UNKNOWN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "nextgenmap_amd", "ngm-hip")


@pytest.mark.parametrize("extra,why", [
    (["-p"], "-p/--paired"),
    (["--qry1", "a.fq", "--qry2", "b.fq"], "--qry1/--qry2"),
    (["--bam"], "--bam"),
    (["--shard", "0/2"], "--shard:"),
    (["--shard-output"], "--shard-output"),
    (["--bs-mapping"], "--bs-mapping"),
    (["--slam-seq", "1"], "--slam-seq"),
], ids=["paired", "qry1-qry2", "bam", "shard", "shard-output", "bs-mapping", "slam-seq"])
def test_argos_refuses_unsupported_combinations(tmp_path, extra, why):
    from nextgenmap_amd import build
    build.build()
    # (neither file exists: the refusal comes from the option check, before the reference or the reads are opened)
    r = subprocess.run([CLI, "-r", str(tmp_path / "none.fa"), "-q", str(tmp_path / "none.fq"), "-o", str(tmp_path / "out.txt"), "--argos"] + extra,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "--argos cannot be combined with " + why in r.stderr, r.stderr
    assert not os.path.exists(tmp_path / "out.txt")


def _lib():
    from nextgenmap_amd.pipeline import _lib as load
    return load()


def _order(lib, score, rank, min_score, read_len=100, match=10):
    n = len(score)
    score = np.ascontiguousarray(score, np.float32)
    rk = None if rank is None else np.ascontiguousarray(rank, np.uint32)
    order = np.zeros(max(1, n), np.uint32)
    out = np.zeros(3, np.uint32)
    rc = lib.ngm_debug_argos_order(n, score.ctypes.data, None if rk is None else rk.ctypes.data, min_score, read_len, match, order.ctypes.data, out.ctypes.data)
    assert rc == 0
    return [int(x) for x in order[:out[0]]], int(out[1]), int(out[2])


def _expected(score, rank, min_score, read_len=100, match=10):
    """the reference: the survivors in its candidate order (the filter keeps it), std::sort by score, the positive prefix printed"""
    n = len(score)
    cs = sorted(range(n), key=lambda x: int(rank[x]))
    if min_score > 0:
        mn = np.float32(min_score) if min_score > 1 else np.float32(np.float32(read_len) * np.float32(match)) * np.float32(min_score)
        cs = [x for x in cs if np.float32(score[x]) >= mn]
    v = StdSort(lambda a, b: score[a] > score[b]).sort(list(cs))
    npos = sum(1 for x in v if score[x] > 0)
    return v, npos


@pytest.mark.parametrize("min_score", [0.0, 0.5, 420.0], ids=["no-filter", "share-of-best", "absolute"])
def test_argos_order_matches_std_sort_on_lists_with_heavy_ties(min_score):
    lib = _lib()
    rng = np.random.default_rng(7)
    seen = {0: 0, 1: 0, 2: 0}
    for it in range(3000):
        n = int(rng.choice([1, 2, 5, 12, 16, 17, 25, 40, 90, 300]))
        levels = rng.integers(1, 8)
        score = rng.choice(np.array([-30, 0, 350, 420, 500, 610, 777, 1000], np.float32)[:max(2, int(levels))], n).astype(np.float32)
        if it % 5 == 0:
            score = rng.permutation(np.arange(n, dtype=np.float32) * 7 + 1)   # distinct scores: class U
        rank = rng.permutation(n).astype(np.uint32) * 2 + rng.integers(0, 2)
        got, npos, cls = _order(lib, score, rank, min_score)
        want, wpos = _expected(score, rank, min_score)
        assert npos == wpos and len(got) == len(want)
        assert got[:npos] == want[:npos], (it, n, cls, score.tolist(), rank.tolist())
        pos = [float(score[x]) for x in want[:npos]]
        tie = len(set(pos)) != len(pos)
        assert cls == (0 if not tie else 1 if len(want) <= 16 else 2)
        seen[cls] += 1
    assert all(seen[c] > 0 for c in (0, 1, 2)), seen


def test_argos_order_without_a_known_candidate_order_falls_back_to_positions():
    lib = _lib()
    score = np.array([500, 500, 700, 500, 0], np.float32)
    rank = np.array([3, UNKNOWN, 1, 0, 2], np.uint32)
    got, npos, cls = _order(lib, score, rank, 0.0)
    assert cls == 1 and npos == 4
    assert got[:npos] == [2, 0, 1, 3]
