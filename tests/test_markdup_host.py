"""No GPU: the host-only parts of `ngm-hip --sort --markdup` (nextgenmap_amd/csrc/markdup.h: the unclipped 5' coordinate, the end key and
the pair key, the score, the pair test with its name comparison) through tests/cpp/markdup_driver.cpp, built with g++ and once more with
-fsanitize=address,undefined, against the plain-Python rules of tests/markdup_model.py; and what the option refuses before any GPU work."""
import os
import random
import struct
import subprocess

import pytest

import markdup_model as MD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "nextgenmap_amd", "ngm-hip")
SRC = os.path.join(ROOT, "tests", "cpp", "markdup_driver.cpp")
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
M, I, D, N, S, H = 0, 1, 2, 3, 4, 5


def rec(name, ref_id, pos, flag, cigar=(), qual=b"", l_seq=None, tags=b""):
    """a record without a Python loop per base.  qual: the raw quality bytes, or None for absent ones (0xFF) over l_seq bases"""
    l_seq = len(qual) if l_seq is None else l_seq
    q = b"\xff" * l_seq if qual is None else qual
    assert len(q) == l_seq
    body = struct.pack("<iiIIiiii", ref_id, pos, (4680 << 16) | (len(name) + 1), (flag << 16) | len(cigar), l_seq, -1, -1, 0) + name + b"\0" + \
        b"".join(struct.pack("<I", (n << 4) | op) for op, n in cigar) + bytes((l_seq + 1) // 2) + q + tags
    return struct.pack("<I", len(body)) + body


@pytest.fixture(scope="module", params=["plain", "sanitizers"])
def run(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("markdup_" + request.param)
    out = str(d / "markdup_driver")
    if request.param == "plain":
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", SRC, "-o", out])
    else:
        c = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", out], capture_output=True, text=True)
        if c.returncode != 0:
            pytest.skip("no sanitizer runtime for g++ here: " + c.stderr[-200:])

    def go(chains):
        """[[record]] -> per chain ([(examined, u5, end key, score)], [(pair_order, lo, hi)])"""
        p = str(d / "in.bin")
        with open(p, "wb") as f:
            for recs in chains:
                z = b"".join(recs)
                f.write(struct.pack("<I", len(z)) + z)
        r = subprocess.run([out, p, p + ".out"], capture_output=True, env=SAN_ENV if request.param == "sanitizers" else None)
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
        raw, at, res = open(p + ".out", "rb").read(), 0, []
        for recs in chains:
            n, = struct.unpack_from("<I", raw, at)
            assert n == len(recs)
            at += 4
            per = [struct.unpack_from("<IqQI", raw, at + 24 * i) for i in range(n)]
            at += 24 * n
            nb = [struct.unpack_from("<IQQ", raw, at + 20 * i) for i in range(max(n - 1, 0))]
            at += 20 * max(n - 1, 0)
            res.append((per, nb))
        assert at == len(raw)
        return res
    return go


def _expect(recs):
    per = [(1 if MD.examined(r) else 0, MD.u5(r), MD.end_key(r), MD.score(r)) for r in recs]
    nb = []
    for a, b in zip(recs, recs[1:]):
        lo, hi, role = MD.pair_key(MD.end_key(a), MD.end_key(b))
        nb.append((MD.pair_order(recs, len(nb)), lo, hi | (role << 63)))
    return per, nb


U5_CASES = [
    # (flag, pos, cigar, u5 written out by hand)
    (0, 100, [(S, 5), (M, 50)], 95),
    (0, 100, [(H, 7), (M, 50)], 93),
    (0, 100, [(H, 7), (S, 5), (M, 50)], 88),
    (0, 100, [(M, 50), (S, 9)], 100),                      # trailing clips do not move a forward read
    (0, 100, [(I, 3), (M, 50)], 100),                      # an insertion at the end is no clip
    (0, 100, [(S, 2), (I, 3), (M, 50)], 98),               # ... and ends the run of clips
    (0, 100, [], 100),
    (16, 100, [], 100),
    (16, 100, [(M, 50)], 149),
    (16, 100, [(M, 50), (S, 5)], 154),
    (16, 100, [(M, 50), (H, 7)], 156),
    (16, 100, [(M, 50), (S, 5), (H, 7)], 161),
    (16, 100, [(S, 4), (M, 20), (D, 3), (N, 10), (M, 17), (I, 2)], 149),   # a trailing insertion: neither a clip nor on the reference
    (16, 100, [(M, 50), (I, 3), (S, 5)], 154),
    (16, 100, [(S, 9), (M, 50)], 149),                     # leading clips do not move a reverse read
    (0, 3, [(S, 10), (M, 5)], -7),                         # below zero is kept: it still tells two reads apart
    (0, 100, [(S, 4)], 96),                                # clips only
    (16, 100, [(S, 4)], 104),
]


def test_u5_written_out_by_hand(run):
    recs = [rec(b"r%d" % i, 1, pos, flag, cigar, b"\x1e" * 4) for i, (flag, pos, cigar, _) in enumerate(U5_CASES)]
    assert [MD.u5(r) for r in recs] == [c[3] for c in U5_CASES]
    assert run([recs])[0] == _expect(recs)


def test_u5_is_clamped(run):
    big = (1 << 28) - 1                                    # the longest operation a CIGAR holds
    recs = [rec(b"a", 0, 5, 0, [(S, big)] * 5 + [(M, 10)], b"\x1e"),                  # far below: clamped to -2^30
            rec(b"b", 0, 5, 0, [(S, big)] * 4 + [(M, 10)], b"\x1e"),                  # 5 - (2^30 - 4): not clamped
            rec(b"c", 0, (1 << 29) - 20, 16, [(M, 10)] + [(H, big)] * 3, b"\x1e"),    # far above: clamped to 2^30 - 1
            rec(b"d", 0, (1 << 29) - 20, 16, [(M, 10)] + [(H, big)] * 1, b"\x1e"),
            rec(b"e", 0, 5, 0, [(H, big)] * 60000 + [(M, 10)], b"\x1e")]              # 2^44 of clips: no 32-bit sum
    assert [MD.u5(r) for r in recs] == [MD.U5_MIN, 5 - 4 * big, MD.U5_MAX, (1 << 29) - 20 + 10 - 1 + big, MD.U5_MIN]
    got = run([recs])[0]
    assert got == _expect(recs)
    assert all(k >> 63 == 0 for _, _, k, _ in got[0])


def test_end_keys_do_not_collide_and_order_as_ref_u5_strand(run):
    rnd = random.Random(3)
    coords = set()
    for ref in (0, 1, 7, (1 << 31) - 2):
        for u5 in (MD.U5_MIN, MD.U5_MIN + 1, -1, 0, 1, 12345, MD.U5_MAX - 1, MD.U5_MAX):
            for strand in (0, 1):
                coords.add((ref, u5, strand))
    while len(coords) < 400:
        coords.add((rnd.randrange(0, 1 << 31), rnd.randrange(MD.U5_MIN, MD.U5_MAX + 1), rnd.randrange(2)))
    coords = sorted(coords)
    recs = []
    for i, (ref, u5, strand) in enumerate(coords):         # a forward read starts at u5; a reverse read with 1M ends there
        if strand == 0 and u5 < 0:
            big = (1 << 28) - 1                            # (one operation holds 28 bits)
            recs.append(rec(b"k%d" % i, ref, 0, 0, [(S, big)] * (-u5 // big) + [(S, -u5 % big), (M, 1)], b"\x1e"))
        elif u5 < 0:
            continue                                       # (a reverse read's u5 is at least its pos)
        else:
            recs.append(rec(b"k%d" % i, ref, u5, 16 * strand, [(M, 1)], b"\x1e"))
    want = [(p[0], MD.u5(r), (p[2] >> 4) & 1) for r, p in ((r, MD.parse(r)) for r in recs)]
    assert want == sorted(set(want))
    got = run([recs])[0]
    assert got == _expect(recs)
    keys = [k for _, _, k, _ in got[0]]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)          # the order of (ref, u5, strand), and no two alike


def test_pair_key_is_symmetric_for_fr_and_not_for_ff(run):
    q = b"\x1e" * 10
    f100, f300 = (0, 100, 0, [(M, 10)]), (0, 300, 0, [(M, 10)])
    r300 = (0, 291, 16, [(M, 10)])                                       # reverse, u5 300
    r100 = (0, 91, 16, [(M, 10)])

    def pair(a, b, name=b"p"):
        return [rec(name, a[0], a[1], 0x41 | a[2] | (0x20 if b[2] else 0), a[3], q), rec(name, b[0], b[1], 0x81 | b[2] | (0x20 if a[2] else 0), b[3], q)]
    chains = [pair(f100, r300), pair(r300, f100), pair(f100, f300), pair(f300, f100), pair(r100, r300), pair(r300, r100), pair(f100, f100), pair(f100, (1, 100, 0, [(M, 10)])),
              pair((1, 100, 0, [(M, 10)]), f100)]
    got = run(chains)
    for chain, g in zip(chains, got):
        assert g == _expect(chain) and g[1][0][0] == 1
    key = lambda g: g[1][0][1:]
    fr, rf, ff, ff_swapped, rr, rr_swapped, same, two_refs, two_refs_swapped = map(key, got)
    assert fr == rf                                        # FR and RF: which mate is which does not count
    assert ff != ff_swapped and rr != rr_swapped           # FF and RR: it does
    assert ff[0] == ff_swapped[0] and ff[1] ^ ff_swapped[1] == 1 << 63
    assert same[1] >> 63 == 1                              # equal end keys: the first mate goes first
    assert two_refs != two_refs_swapped and two_refs[0] == two_refs_swapped[0]   # (same strands on two references: FF)
    assert all(lo <= hi & ~(1 << 63) and lo >> 63 == 0 for lo, hi in (fr, rf, ff, ff_swapped, rr, rr_swapped, same, two_refs))


def test_pair_test(run):
    q = b"\x1e" * 4
    a = lambda name, flag, ref=0: rec(name, ref, 10, flag, [(M, 4)], q)
    cases = [([a(b"x", 0x41), a(b"x", 0x81)], 1),
             ([a(b"x", 0x41), a(b"x", 0x41)], 0),          # 0x40 followed by 0x40
             ([a(b"x", 0x81), a(b"x", 0x41)], 2),          # the second mate in front: the order ngm-hip writes
             ([a(b"x", 0x81), a(b"x", 0x41), a(b"x", 0x81)], 0),                  # ... but not beside a pair with the first mate in front
             ([a(b"x", 0x41), a(b"x", 0x81), a(b"x", 0x41)], 1),
             ([a(b"x", 0x81), a(b"x", 0x41), a(b"y", 0x81)], 2),
             ([a(b"x", 0x41), a(b"y", 0x81)], 0),          # names differ
             ([a(b"xa", 0x41), a(b"x", 0x81)], 0),         # one name is the start of the other
             ([a(b"x", 0x41), a(b"xa", 0x81)], 0),
             ([a(b"x", 0x40), a(b"x", 0x81)], 0),          # 0x1 missing
             ([a(b"x", 0xC1), a(b"x", 0x81)], 0),          # both bits
             ([a(b"x", 0x41), a(b"x", 0x81 | 0x4)], 0),    # the mate is unmapped
             ([a(b"x", 0x41 | 0x100), a(b"x", 0x81)], 0),
             ([a(b"x", 0x41), a(b"x", 0x81 | 0x800)], 0),
             ([a(b"x", 0x41, ref=-1), a(b"x", 0x81)], 0),
             ([a(b"x", 0x41 | 0x400), a(b"x", 0x81 | 0x10 | 0x20)], 1),
             ([a(b"n" * 254, 0x41), a(b"n" * 254, 0x81)], 1),
             ([a(b"n" * 253 + b"a", 0x41), a(b"n" * 253 + b"b", 0x81)], 0)]
    got = run([c for c, _ in cases])
    for (chain, want), g in zip(cases, got):
        assert g == _expect(chain) and g[1][0][0] == want, chain


def test_scores(run):
    big = rec(b"big", 0, 10, 0, [(M, 10)], b"\xfe" * 17_000_000)         # 254 * 17 000 000 > 2^32: saturates
    recs = [rec(b"a", 0, 10, 0, [(M, 4)], bytes([14, 15, 14, 15])),      # 14 does not count, 15 does
            rec(b"b", 0, 10, 0, [(M, 4)], bytes([0, 14, 13, 1])),
            rec(b"c", 0, 10, 0, [(M, 4)], None, l_seq=4),                # absent qualities
            rec(b"d", 0, 10, 0, [(M, 4)], bytes([0xFF, 40, 40, 40])),    # the first byte decides
            rec(b"e", 0, 10, 0, [(M, 4)], bytes([40, 0xFF, 40])),
            rec(b"f", 0, 10, 0, [(M, 4)], b""),                          # l_seq 0
            rec(b"g", 0, 10, 0, [], b"", tags=b"XXZ" + b"\x28" * 20 + b"\0"),   # l_seq 0 with tags behind: nothing of them is read as qualities
            rec(b"odd", 0, 10, 0, [(M, 5)], bytes(range(11, 16)) + bytes([93])),
            big]
    assert [MD.score(r) for r in recs[:8]] == [30, 0, 0, 0, 335, 0, 0, 15 + 93]
    assert 254 * 17_000_000 > MD.SCORE_MAX
    got = run([recs])[0]
    assert [s for _, _, _, s in got[0][:8]] == [30, 0, 0, 0, 335, 0, 0, 108]
    assert got[0][8][3] == MD.SCORE_MAX
    assert MD.score(rec(b"s", 0, 10, 0, [(M, 10)], b"\xfe" * 100)) == 25400


def test_random_records_equal_the_model(run):
    rnd = random.Random(44)
    recs = []
    for i in range(600):
        cigar = [(rnd.choice([M, I, D, N, S, H, 7, 8]), rnd.randrange(1, 400)) for _ in range(rnd.randrange(0, 7))]
        flag = rnd.choice([0, 16, 4, 0x41, 0x81, 0x51, 0x91, 0x100, 0x800, 0x400, 0x410])
        name = rnd.choice([b"same", b"r%d" % (i // 2)])
        recs.append(rec(name, rnd.choice([-1, 0, 1, 2]), rnd.randrange(0, 1 << 20), flag, cigar, rnd.randbytes(rnd.randrange(0, 120))))
    assert run([recs, [], recs[:1]]) == [_expect(recs), ([], []), _expect(recs[:1])]


# ---- the model itself, on cases small enough to decide by eye --------------------------------------------------------------------------
def test_model_on_hand_cases():
    q = lambda v, n=10: bytes([v]) * n
    a = rec(b"a", 0, 100, 0, [(M, 10)], q(30))
    b = rec(b"b", 0, 100, 0, [(M, 10)], q(40))                           # the better one, later in run order
    c = rec(b"c", 0, 102, 0, [(S, 2), (M, 8)], q(40))                    # the same u5, equal score: the earlier of b and c survives
    d = rec(b"d", 0, 100, 16, [(M, 10)], q(40))                          # the other strand
    out, counts = MD.mark([a, b, c, d])
    assert [MD.parse(r)[2] & 0x400 for r in out] == [0x400, 0, 0x400, 0]
    assert counts == dict(examined=4, pairs=0, fragments=4, duplicate_pairs=0, duplicate_fragments=2, newly_marked=2)
    p1 = [rec(b"p", 0, 100, 0x61, [(M, 10)], q(30)), rec(b"p", 0, 291, 0x91, [(M, 10)], q(30))]
    p2 = [rec(b"q", 0, 291, 0x51, [(M, 10)], q(30)), rec(b"q", 0, 100, 0xA1, [(M, 10)], q(31))]   # roles swapped, the better pair
    frag_on_end = rec(b"f", 0, 100, 0x400, [(M, 10)], q(60))             # on an end of the pairs: marked whatever its score; it came marked
    frag_near = rec(b"g", 0, 101, 0, [(M, 10)], q(1))
    out, counts = MD.mark(p1 + [frag_on_end] + p2 + [frag_near])
    assert [MD.parse(r)[2] & 0x400 for r in out] == [0x400, 0x400, 0x400, 0, 0, 0]
    assert counts == dict(examined=6, pairs=2, fragments=2, duplicate_pairs=1, duplicate_fragments=1, newly_marked=2)


def test_markdup_needs_sort(tmp_path):
    from nextgenmap_amd import build
    build.build()
    # (neither file exists: the refusal comes from the option check, before the reference or the reads are opened)
    r = subprocess.run([CLI, "-r", str(tmp_path / "none.fa"), "-q", str(tmp_path / "none.fq"), "-o", str(tmp_path / "out.bam"), "--bam", "--markdup"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1
    assert "--markdup needs --sort: duplicates are found among the records the sorter holds" in r.stderr, r.stderr
    assert not os.path.exists(tmp_path / "out.bam") and "HIP backend (gfx950)" not in r.stderr + r.stdout
