"""No GPU: ngm::Owned (nextgenmap_amd/csrc/buffer.h), the one owner of device and pinned memory, over a counting malloc through
tests/cpp/buffer_driver.cpp, a stand-alone program built with g++ -fsanitize=address,undefined.  The capacities below are worked out by
hand from the three growth rules and typed in:
  reserve(n): n + min(n / 8, 64 MiB / sizeof(T)) elements, exactly n when that request is refused; a no-op when n fits
  alloc(n):   n elements (one is asked for when n is 0)
  grow(n):    n + n / 4 + 64 elements; a no-op when n fits
The sanitizer's leak check at exit is on: the driver ends with nothing live and exit status 0."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "buffer_driver.cpp")

#      n          reserve    grow
CAPS = {
    "u8": [(0, 0, 0), (1, 1, 65), (7, 7, 72), (8, 9, 74), (9, 10, 75), (63, 70, 142), (64, 72, 144), (1000, 1125, 1314),
           (536870920, 603979784, 671088714)],      # n / 8 = 67108865 is past the 67108864 elements of 64 MiB
    "u64": [(0, 0, 0), (1, 1, 65), (7, 7, 72), (8, 9, 74), (9, 10, 75), (63, 70, 142), (64, 72, 144), (1000, 1125, 1314),
            (67108872, 75497480, 83886154)],        # n / 8 = 8388609 is past the 8388608 elements of 64 MiB
}
SIZE = {"u8": 1, "u64": 8}


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("buffer_driver") / "buffer_driver_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", out])
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "LSAN_OPTIONS")}   # (the leak check at exit stays on)
    r = subprocess.run([out], capture_output=True, env=env, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    assert r.stderr == b"", r.stderr[-3000:]
    return [ln.split() for ln in r.stdout.decode().splitlines()]


def _one(lines, key):
    got = [ln[1:] for ln in lines if ln[0] == key]
    assert len(got) == 1, (key, got)
    return [int(x) for x in got[0]]


@pytest.mark.parametrize("t", ["u8", "u64"])
def test_capacities_of_the_three_rules(lines, t):
    got = {(ln[0], int(ln[2])): [int(x) for x in ln[3:]] for ln in lines if ln[0] in ("reserve", "alloc", "grow") and ln[1] == t}
    assert len(got) == 3 * len(CAPS[t])
    for n, reserve, grow in CAPS[t]:
        # return, capacity, bytes of the last request, p set
        assert got[("reserve", n)] == [0, reserve, reserve * SIZE[t], 1 if n else 0], n
        assert got[("alloc", n)] == [0, n, max(n, 1) * SIZE[t], 1], n
        assert got[("grow", n)] == [0, grow, grow * SIZE[t], 1 if n else 0], n
    assert _one(lines, "live") == [0]


def test_what_fits_stays_and_what_does_not_is_freed_first(lines):
    assert _one(lines, "fits") == [112, 1, 0]              # reserve(100) left 112 elements: reserve(112) keeps block and capacity, no request
    assert _one(lines, "regrown") == [127, 1, 1, 127 * 4]  # reserve(113): one free, one request of 113 + 14
    assert _one(lines, "grow_fits") == [127]
    assert _one(lines, "grow_regrown") == [314, 314 * 4]   # grow(200): 200 + 50 + 64
    assert _one(lines, "alloc_shrinks") == [3, 12]


def test_reserve_falls_back_to_exactly_n(lines):
    assert _one(lines, "fallback") == [0, 1000, 2, 4000]   # 1125 refused, then 1000 uint32_t
    assert _one(lines, "both_fail")[0] != 0
    assert _one(lines, "both_fail")[1:] == [0, 0, 0]       # p null, capacity 0, and the 1000 elements held before are gone
    assert _one(lines, "alloc_fail")[0] != 0 and _one(lines, "alloc_fail")[1:] == [0, 0]
    assert _one(lines, "grow_fail")[0] != 0 and _one(lines, "grow_fail")[1:] == [0, 0, 0]


def test_moves_and_swaps_keep_one_owner(lines):
    assert _one(lines, "move_ctor") == [0, 0, 1, 11, 44]          # the source empty, the block and its 11 elements with the target
    assert _one(lines, "move_assign") == [1, 1, 11, 0, 0, 44]     # the target's old block freed exactly once
    assert _one(lines, "swap") == [1, 3, 1, 11, 0, 0]             # no request, no free
    assert _one(lines, "self_move") == [1, 11, 0, 44 + 12]        # harmless: same block, nothing freed
    assert _one(lines, "scope_end") == [0]


def test_an_early_return_leaves_nothing_live(lines):
    assert _one(lines, "early_return") == [-5, 0]
    assert _one(lines, "full_return") == [0, 0]
    live, gets, puts = _one(lines, "end")
    assert live == 0 and gets - 5 == puts                  # (five requests were refused on purpose)
