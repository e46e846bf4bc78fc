"""No GPU, no library: the host-only pair logic of nextgenmap_amd/csrc/pair_host.h (sort_like_reference, walk_pair, PairSeqKeeper,
eval_pair_seq, select_pair) through tests/cpp/pair_host_driver.cpp, built with plain g++ and once more with -fsanitize=address,undefined,
against the restatements of tests/test_pair_walk.py: libstdc++'s std::sort, the plain double loop over the candidates above the cut-off
and the loop of CheckPairs.  The walk cases go through test_pair_walk.run_case itself -- the driver stands in for the library's
ngm_debug_pair_walk; select_pair is compared with what those restatements give for the whole pair, and its PairTies with their
documented meaning (the comment at the end of select_pair)."""
import ctypes as C
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import test_pair_walk as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "pair_host_driver.cpp")
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
INT_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module", params=["plain", "sanitizers"])
def drive(request, tmp_path_factory):
    """bytes of records in -> bytes of results out, one process per call"""
    d = tmp_path_factory.mktemp("pair_host_" + request.param)
    exe = str(d / "pair_host_driver")
    if request.param == "plain":
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", SRC, "-o", exe])
    else:
        c = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe],
                           capture_output=True, text=True)
        if c.returncode != 0:
            pytest.skip("no sanitizer runtime for g++ here: " + c.stderr[-200:])

    def go(records):
        p = str(d / "in.bin")
        with open(p, "wb") as f:
            f.write(records)
        r = subprocess.run([exe, p, p + ".out"], capture_output=True, env=SAN_ENV if request.param == "sanitizers" else None)
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
        return open(p + ".out", "rb").read()
    return go


def lists_record(kind, cnt_a, len_a, cnt_b, len_b, loc, sv, score, rank, cutoff, min_d, max_d, cap=0, dist_sum=0, dist_count=1):
    head = struct.pack("<IIiIiIfiiQqq", kind, cnt_a, len_a, cnt_b, len_b, 0 if rank is None else 1, cutoff, min_d, max_d, cap, dist_sum, dist_count)
    return head + np.ascontiguousarray(loc, np.uint32).tobytes() + np.ascontiguousarray(sv, np.uint32).tobytes() + \
        np.ascontiguousarray(score, np.float32).tobytes() + (b"" if rank is None else np.ascontiguousarray(rank, np.uint32).tobytes())


def _at(addr, ctype, n):
    return np.ctypeslib.as_array((ctype * max(n, 1)).from_address(addr))[:n]


class DriverAsLibrary:
    """what test_pair_walk.run_case calls on the library, answered by the driver"""

    def __init__(self, drive):
        self.drive = drive

    def ngm_pipeline_last_error(self):
        return "pair_host_driver"

    def ngm_debug_pair_walk(self, cnt_a, len_a, cnt_b, len_b, loc, sv, score, rank, cutoff, min_d, max_d, out_a, out_b, mq_a, mq_b, cap, c_ps, c_d, c_a, c_b, n_combo):
        n = cnt_a + cnt_b
        rec = lists_record(1, cnt_a, len_a, cnt_b, len_b, _at(loc, C.c_uint32, n), _at(sv, C.c_uint32, n), _at(score, C.c_float, n),
                           None if rank is None else _at(rank, C.c_uint32, n), cutoff, min_d, max_d, cap)
        raw = self.drive(rec)
        _at(out_a, C.c_uint32, cnt_a)[:] = np.frombuffer(raw, np.uint32, cnt_a, 0)
        _at(out_b, C.c_uint32, cnt_b)[:] = np.frombuffer(raw, np.uint32, cnt_b, 4 * cnt_a)
        at = 4 * n
        a, b, k = struct.unpack_from("<iiQ", raw, at)
        at += 16
        _at(mq_a, C.c_int, 1)[0] = a; _at(mq_b, C.c_int, 1)[0] = b; _at(n_combo, C.c_uint64, 1)[0] = k
        kept = min(k, cap)
        for addr, ctype, dt in ((c_ps, C.c_float, np.float32), (c_d, C.c_int32, np.int32), (c_a, C.c_int32, np.int32), (c_b, C.c_int32, np.int32)):
            _at(addr, ctype, kept)[:] = np.frombuffer(raw, dt, kept, at)
            at += 4 * kept
        assert at == len(raw)
        return 0


@pytest.mark.parametrize("kind", ["satellite", "families", "edges", "spread"])
@pytest.mark.parametrize("scores", ["ties", "equal", "distinct", "few", "wide"])
def test_walk_matches_the_reference_algorithm(drive, kind, scores):
    """the 20 kind x scores cases of test_pair_walk, list sizes on both sides of every threshold of the two sorts and of the windowed walk"""
    lib = DriverAsLibrary(drive)
    rng = np.random.default_rng(zlib.crc32((kind + "/" + scores).encode()))
    combos = 0
    for cnt_a, cnt_b in ((1, 1), (1, 40), (3, 5), (16, 16), (17, 16), (40, 33), (255, 256), (257, 300), (1200, 900), (2500, 1800)):
        loc, sv, score, rank = W.make_lists(rng, cnt_a, cnt_b, kind, scores)
        _, k = W.run_case(lib, cnt_a, cnt_b, loc, sv, score, rank)
        combos += k
    assert combos > 0 or kind == "spread"


def test_walk_without_ranks_with_repeated_ranks_and_other_windows(drive):
    lib = DriverAsLibrary(drive)
    rng = np.random.default_rng(77)
    loc, sv, score, rank = W.make_lists(rng, 700, 650, "families", "ties")
    W.run_case(lib, 700, 650, loc, sv, score, None)                                # no candidate order at all
    rk = rank.copy(); rk[5] = W.UNKNOWN
    W.run_case(lib, 700, 650, loc, sv, score, rk)                                  # one candidate's order unknown: as without
    rk = rank.copy(); rk[:700] = rk[:700] // 64 * 64                               # repeated ranks: the comparison path
    W.run_case(lib, 700, 650, loc, sv, score, rk)
    for cutoff, lo, hi in ((0.9, 0, 1000), (0.5, 100, 400), (1.0, 0, 0), (0.99, 0, 50_000)):   # (max 0: no upper limit)
        loc, sv, score, rank = W.make_lists(rng, 300, 280, "satellite", "ties")
        W.run_case(lib, 300, 280, loc, sv, score, rank, cutoff=cutoff, min_d=lo, max_d=hi)


def test_evaluation_on_all_and_on_the_kept_combinations(drive):
    """eval_pair_seq against the loop of CheckPairs (test_pair_walk.check_pairs_loop), on every combination and on what PairSeqKeeper keeps"""
    rng = np.random.default_rng(20261001)
    records, wants, sizes = [], [], []
    for case in range(200):
        n = int(rng.choice([0, 1, 2, 7, 64, 500, 3000]))
        ps = [rng.choice([2800.0, 2790.0, 2785.0, 2700.0], n), np.full(n, 2468.0), rng.choice([0.0, -5.0, -20.0], n),
              np.sort(rng.integers(1, 3000, n)).astype(np.float64), rng.integers(-10, 40, n).astype(np.float64)][case % 5]
        d = rng.integers(1, 1000, n) if case % 2 else rng.choice([300, 350, 400], n)
        ps = np.ascontiguousarray(ps, np.float32); d = np.ascontiguousarray(d, np.int32)
        a = np.ascontiguousarray(rng.integers(0, 1 << 20, n), np.int32); b = np.ascontiguousarray(rng.integers(0, 1 << 20, n), np.int32)
        for avg in (int(rng.integers(150, 600)), 0):
            records.append(struct.pack("<IQi", 2, n, avg) + ps.tobytes() + d.tobytes() + a.tobytes() + b.tobytes())
            wants.append(W.check_pairs_loop(ps, d, a, b, avg)); sizes.append(n)
    got = np.frombuffer(drive(b"".join(records)), np.int32).reshape(len(records), 2, 6)
    kept_total = 0
    for x, want in enumerate(wants):
        assert got[x, 0, :5].tolist() == want and got[x, 1, :5].tolist() == want, x
        assert got[x, 0, 5] == sizes[x] and got[x, 1, 5] <= sizes[x]
        kept_total += int(got[x, 1, 5])
    assert 0 < kept_total < sum(sizes)   # (the filter does drop combinations in these cases)


def expected_select(cnt_a, cnt_b, loc, sv, score, rank, cutoff, min_d, max_d, len_a, len_b, dist_sum, dist_count):
    """ScoreBuffer::top1PE + CheckPairs for one pair from the restatements of test_pair_walk, and PairTies as select_pair documents them:
    [found, win_a, win_b, mq_a, mq_b, equal, dist] (None: not written) and [equal_scores, dup, unique_closest, dmin_top, dmax_top, n_top,
    [top_d], [top_a], [top_b]]"""
    n = cnt_a + cnt_b
    avg = dist_sum // max(1, dist_count)
    hi = max_d if max_d > 0 else INT_MAX
    if cnt_a == 1 and cnt_b == 1:
        l1, l2 = int(loc[0]), int(loc[1])
        cur = l2 - l1 + len_b if l2 > l1 else l1 - l2 + len_a
        found = min_d < cur < hi and np.float32(score[0]) + np.float32(score[1]) > 0
        return ([1, 0, 1, 60, 60, 0, cur] if found else [0, None, None, 60, 60, None, None]), [0, 0, 1, 0, 0, 0, [], [], []]
    A, _ = W.reference_order(list(range(cnt_a)), loc, sv, score, rank)
    B, _ = W.reference_order(list(range(cnt_a, n)), loc, sv, score, rank)
    ps, d, a, b = W.expected_walk(A, B, len_a, len_b, loc, score, cutoff, min_d, max_d)
    found, wa, wb, equal, dist = W.check_pairs_loop(ps, d, a, b, avg)
    res = [1, wa, wb, W.mapq(A, score), W.mapq(B, score), equal, dist] if found else [0, None, None, W.mapq(A, score), W.mapq(B, score), None, None]
    k = len(ps)
    if k <= 1:
        return res, [0, 0, 1, 0, 0, 0, [], [], []]
    if k > 64:   # more than select_pair records: everything is left to the exact sequential pass
        return res, [1, 1, 0, min_d, hi, 0, [], [], []]
    top = max(np.float32(0.0), ps.max())
    tops = [x for x in range(k) if ps[x] == top]
    closest = [abs(int(d[x]) - avg) for x in tops]
    equal_scores = len(set(ps.tolist())) < k
    dup = len(set(zip(ps.tolist(), d.tolist()))) < k
    n_top = len(tops) if found else 0
    ties = [int(equal_scores), int(dup or n_top > 8), int(closest.count(min(closest)) <= 1) if tops else 1,
            int(min(d[tops])) if found else 0, int(max(d[tops])) if found else 0, n_top]
    listed = tops[:8] if found else []
    return res, ties + [[int(d[x]) for x in listed], [int(a[x]) for x in listed], [int(b[x]) for x in listed]]


def check_select(drive, cnt_a, cnt_b, loc, sv, score, rank, cutoff=0.9, min_d=0, max_d=1000, len_a=150, len_b=150, dist_sum=0, dist_count=1):
    loc = np.ascontiguousarray(loc, np.uint32); sv = np.ascontiguousarray(sv, np.uint32); score = np.ascontiguousarray(score, np.float32)
    rk = None if rank is None else np.ascontiguousarray(rank, np.uint32)
    raw = drive(lists_record(3, cnt_a, len_a, cnt_b, len_b, loc, sv, score, rk, cutoff, min_d, max_d, 0, dist_sum, dist_count))
    got = np.frombuffer(raw, np.int32)
    assert got.size == 13 + 24
    res, ties = expected_select(cnt_a, cnt_b, loc, sv, score, rk, cutoff, min_d, max_d, len_a, len_b, dist_sum, dist_count)
    assert [g for g, w in zip(got[:7].tolist(), res) if w is not None] == [w for w in res if w is not None], (got[:7], res)
    assert got[7:13].tolist() == ties[:6], (got[7:13], ties)
    for x, want in enumerate(ties[6:]):
        assert got[13 + 8 * x:13 + 8 * x + len(want)].tolist() == want
    return res, ties


def test_select_pair_whole_pairs(drive):
    """select_pair on the cases the issue names: one candidate per mate, more than 64 in-window combinations, more than 8 best-scoring pairs;
    and small tied pairs at several running means"""
    rng = np.random.default_rng(20261020)
    # one candidate per mate: inside the window, outside it, at its bounds, without a positive pair score
    for l1, l2, s1, s2 in ((5000, 5300, 700.0, 650.0), (5300, 5000, 700.0, 650.0), (5000, 9000, 700.0, 650.0), (5000, 5850, 700.0, 650.0), (5000, 5849, 700.0, 650.0),
                           (5000, 5300, -10.0, 5.0), (5000, 5300, 0.0, 0.0)):
        res, _ = check_select(drive, 1, 1, [l1, l2], [0, 1], [s1, s2], [2, 5])
        assert res[0] == (1 if abs(l2 - l1) + 150 < 1000 and s1 + s2 > 0 else 0)
    # more than 64 combinations inside the window
    loc, sv, score, rank = W.make_lists(rng, 40, 33, "satellite", "ties")
    _, ties = check_select(drive, 40, 33, loc, sv, score, rank, max_d=5000, dist_sum=350 * 1000, dist_count=1000)
    assert ties[:3] == [1, 1, 0]
    # more than 8 best-scoring pairs among at most 64 combinations: listed up to 8, left to the sequential pass
    loc, sv, score, rank = W.make_lists(rng, 5, 5, "satellite", "equal")
    _, ties = check_select(drive, 5, 5, loc, sv, score, rank, max_d=5000, dist_sum=400 * 50, dist_count=50)
    assert ties[5] > 8 and ties[1] == 1 and len(ties[6]) == 8
    seen = set()
    for case in range(120):
        cnt_a, cnt_b = int(rng.integers(1, 9)), int(rng.integers(1, 9))
        kind, scores = ("satellite", "families")[case % 2], ("ties", "few", "equal", "wide", "distinct")[case % 5]
        loc, sv, score, rank = W.make_lists(rng, cnt_a, cnt_b, kind, scores)
        mean, count = int(rng.integers(200, 600)), int(rng.integers(1, 5000))
        res, ties = check_select(drive, cnt_a, cnt_b, loc, sv, score, rank if case % 3 else None, max_d=(3500, 1000)[case % 2], dist_sum=mean * count, dist_count=count)
        seen.add((res[0], ties[0], ties[1], ties[2]))
    assert {(1, 0, 0), (1, 1, 0), (1, 1, 1), (0, 0, 0)} <= {s[:3] for s in seen}, seen   # fixed by the scores | tied | equal score and insert size | no pair
