"""No GPU: what `ngm-hip --sort` refuses before any GPU work, the model of tests/bam_index_model.py pinned on one BAI file written out by
hand, and the host-only parts of the sorter (nextgenmap_amd/csrc/bam_sort.h: the chain walk with its refusals, the key, the BAI
serialiser fed from arrays) through tests/cpp/bam_sort_driver.cpp, built with g++ and once more with -fsanitize=address,undefined."""
import os
import random
import struct
import subprocess

import pytest

import bam_fixtures as BF
import bam_index_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "nextgenmap_amd", "ngm-hip")
SRC = os.path.join(ROOT, "tests", "cpp", "bam_sort_driver.cpp")
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")


@pytest.mark.parametrize("extra,env,message", [
    ([], {}, "--sort needs -b/--bam"),
    (["--argos"], {}, "--sort cannot be combined with --argos"),
    (["--bam", "--shard", "0/2"], {}, "--sort cannot be combined with --shard:"),
    (["--bam", "--shard-output"], {}, "--sort cannot be combined with --shard-output"),
    (["--bam"], {"NGM_HIP_BAM_ZLIB": "1"}, "--sort cannot be combined with NGM_HIP_BAM_ZLIB=1"),
], ids=["no-bam", "argos", "shard", "shard-output", "zlib"])
def test_sort_refuses_unsupported_combinations(tmp_path, extra, env, message):
    from nextgenmap_amd import build
    build.build()
    # (neither file exists: the refusal comes from the option check, before the reference or the reads are opened)
    r = subprocess.run([CLI, "-r", str(tmp_path / "none.fa"), "-q", str(tmp_path / "none.fq"), "-o", str(tmp_path / "out.bam"), "--sort"] + extra,
                       capture_output=True, text=True, timeout=60, env=dict(os.environ, **env))
    assert r.returncode != 0
    assert message in r.stderr, r.stderr
    assert not os.path.exists(tmp_path / "out.bam") and not os.path.exists(tmp_path / "out.bam.bai")
    assert "HIP backend (gfx950)" not in r.stderr + r.stdout


# ---- the hand-written case: two references, three records, made-up member sizes -----------------------------------------------------
# A: reference 0, pos 16 380, 10M -> [16 380, 16 390): across position 16 384, bin 585, windows 0 and 1; 60 042 bytes
# B: reference 1, pos 100, 50M, reverse strand -> bin 4 681, window 0; 60 042 bytes
# C: refID -1; 53 bytes.  Stream: A [0, 60 042) B [60 042, 120 084) C [120 084, 120 137): two members (65 280 + 54 857 bytes), said to
# compress to 1 000 and 2 000 bytes behind 500 bytes of header members, so member 0 is at file offset 500, member 1 at 1 500
def _hand_case():
    a = BF.bam_record(b"a", b"A" * 40000, None, 0, [(0, 10)], ref_id=0, pos=16380)
    b = BF.bam_record(b"b", b"C" * 40000, None, 16, [(0, 50)], ref_id=1, pos=100)
    c = BF.bam_record(b"c", b"G" * 10, None, 4)
    assert (len(a), len(b), len(c)) == (60042, 60042, 53)
    va0, va1 = (500 << 16) | 0, (500 << 16) | 60042
    vb1 = (1500 << 16) | (120084 - 65280)
    bai = b"".join([
        b"BAI\1", struct.pack("<i", 2),
        # reference 0: bin 585 with one chunk, the pseudo-bin, two windows
        struct.pack("<i", 2),
        struct.pack("<Ii", 585, 1), struct.pack("<QQ", va0, va1),
        struct.pack("<Ii", 37450, 2), struct.pack("<QQ", va0, va1), struct.pack("<QQ", 1, 0),
        struct.pack("<i", 2), struct.pack("<QQ", va0, va0),
        # reference 1: bin 4 681, the pseudo-bin, one window
        struct.pack("<i", 2),
        struct.pack("<Ii", 4681, 1), struct.pack("<QQ", va1, vb1),
        struct.pack("<Ii", 37450, 2), struct.pack("<QQ", va1, vb1), struct.pack("<QQ", 1, 0),
        struct.pack("<i", 1), struct.pack("<Q", va1),
        struct.pack("<Q", 1),
    ])
    return [a, b, c], bai


def test_model_equals_hand_written_bai():
    (a, b, c), bai = _hand_case()
    assert M.sort_records([c, b, a]) == [a, b, c]
    assert M.canonical_bai([a, b, c], 2, [1000, 2000], 500) == bai
    assert M.reg2bin(16380, 16390) == 585 and M.reg2bin(100, 150) == 4681
    # ties keep input order; the reverse strand comes after the forward strand of the same position; refID -1 last
    f = BF.bam_record(b"f", b"AC", None, 0, [(0, 2)], ref_id=0, pos=5)
    r = BF.bam_record(b"r", b"AC", None, 16, [(0, 2)], ref_id=0, pos=5)
    f2 = BF.bam_record(b"f2", b"AC", None, 0, [(0, 2)], ref_id=0, pos=5)
    assert M.sort_records([c, r, f, f2]) == [f, f2, r, c]


# ---- the driver ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("bam_sort")
    out = str(d / "bam_sort_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", SRC, "-o", out])
    return out, d


@pytest.fixture(scope="module")
def exe_san(tmp_path_factory):
    d = tmp_path_factory.mktemp("bam_sort_san")
    out = str(d / "bam_sort_driver_san")
    c = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", out], capture_output=True, text=True)
    if c.returncode != 0:
        pytest.skip("no sanitizer runtime for g++ here: " + c.stderr[-200:])
    return out, d


def _walk(prog, d, chains, env=None):
    """[chain] -> [(accepted, records, message, [(key, end, bin)])] in one process"""
    p = str(d / "chains.bin")
    with open(p, "wb") as f:
        for z in chains:
            f.write(struct.pack("<I", len(z)) + z)
    r = subprocess.run([prog, "walk", p, p + ".out"], capture_output=True, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw, out, at = open(p + ".out", "rb").read(), [], 0
    while at < len(raw):
        ok, n, _, ml = struct.unpack_from("<IIII", raw, at)
        msg = raw[at + 16:at + 16 + ml].decode()
        at += 16 + ml
        recs = [struct.unpack_from("<QqI", raw, at + 20 * i) for i in range(n)] if ok else []
        at += 20 * n if ok else 0
        out.append((ok, n, msg, recs))
    assert len(out) == len(chains)
    return out


def _records(rnd, n):
    out = []
    for i in range(n):
        cigar = [(rnd.choice([0, 1, 2, 3, 4, 7, 8]), rnd.randrange(1, 400)) for _ in range(rnd.randrange(0, 6))]
        out.append(BF.bam_record(b"r%d" % i + b"x" * rnd.randrange(0, 40), bytes(rnd.choice(b"ACGT") for _ in range(rnd.randrange(0, 120))), None, rnd.choice([0, 16, 4, 20]),
                                 cigar, ref_id=rnd.choice([-1, 0, 1, 2]), pos=rnd.randrange(-1, 1 << 20), tags=b"NMi" + struct.pack("<i", i)))
    return out


def _model_record(rec):
    ref_id, pos, end, flag = M.fields(rec)
    k = M.key(rec)
    return (k[0] << 32) | (k[1] << 1) | k[2], end, M.reg2bin(pos, end) if pos >= 0 else 0


def test_walk_key_end_and_bin_equal_the_model(exe):
    prog, d = exe
    rnd = random.Random(41)
    chains = [b"", b"".join(_records(rnd, 1)), b"".join(_records(rnd, 700))]   # (700: more than two ranges of 256 records)
    for chain, (ok, n, msg, recs) in zip(chains, _walk(prog, d, chains)):
        assert ok and not msg
        assert n == len(M.walk(chain))
        assert recs == [_model_record(chain[o:o + s]) for o, s in M.walk(chain)]


def test_walk_refusals_name_the_record(exe):
    prog, d = exe
    recs = _records(random.Random(42), 5)
    good = b"".join(recs)
    at3 = sum(len(r) for r in recs[:3])

    def mod(off, fmt, v):
        b = bytearray(good)
        struct.pack_into(fmt, b, off, v)
        return bytes(b)
    cases = [
        (good[:-1], "record 4", "does not end inside the run"),                      # cut in mid-record
        (good + b"\x28\0\0", "record 5", "does not end inside the run"),             # three stray bytes
        (mod(at3, "<I", 31), "record 3", "block_size 31"),
        (mod(at3, "<I", 0), "record 3", "block_size 0"),
        (mod(at3, "<I", 1 << 31), "record 3", "does not end inside the run"),
        (mod(at3 + 20, "<i", 1 << 20), "record 3", "exceed its block_size"),         # l_seq
        (mod(at3 + 20, "<i", -5), "record 3", "exceed its block_size"),
        (mod(at3 + 16, "<H", 0xFFFF), "record 3", "exceed its block_size"),          # n_cigar_op
    ]
    for (chain, who, why), (ok, _, msg, _) in zip(cases, _walk(prog, d, [c[0] for c in cases])):
        assert not ok and who in msg and why in msg, (who, why, msg)
        with pytest.raises(ValueError):
            M.walk(chain)


def _damaged(rnd, base):
    b = bytearray(base)
    starts = [o for o, _ in M.walk(base)]
    kind = rnd.randrange(5)
    if kind == 0:
        for _ in range(rnd.randrange(1, 8)):
            b[rnd.randrange(len(b))] ^= 1 << rnd.randrange(8)
    elif kind == 1:
        del b[rnd.randrange(len(b)):]
    elif kind == 2:
        struct.pack_into("<I", b, rnd.choice(starts), rnd.choice([0, 31, 1 << 31]))
    elif kind == 3:
        o = rnd.choice(starts)
        for k in range(4, 36):
            b[o + k] = rnd.randrange(256)
    else:
        b += bytes(rnd.randrange(256) for _ in range(rnd.randrange(1, 40)))
    return bytes(b)


def test_damaged_chains_under_sanitizers(exe_san):
    """300 seeded damaged chains: each is refused or walked to exactly its end (the driver checks that, and the keys, ends and bins
    it computes on the way read only what the walk validated); none crashes, none trips a sanitizer; the verdict is the model's"""
    prog, d = exe_san
    rnd = random.Random(43)
    base = b"".join(_records(rnd, 300))
    chains = [_damaged(rnd, base) for _ in range(300)]
    got = _walk(prog, d, chains, env=SAN_ENV)
    refused = 0
    for chain, (ok, n, msg, recs) in zip(chains, got):
        try:
            want = M.walk(chain)
        except ValueError:
            want = None
        assert bool(ok) == (want is not None), msg
        if ok:
            assert n == len(want)
        else:
            refused += 1
            assert "record " in msg
    assert 100 < refused < 300


def _bai_arrays(prog, d, n_ref, chunks, ref_rows, win_base, ioffset, n_no_coor, env=None):
    """chunks: [(key, beg, end)] sorted; ref_rows: [(mapped, unmapped, vbeg, vend)]"""
    a = [c[0] for c in chunks] + [c[1] for c in chunks] + [c[2] for c in chunks]
    for k in range(4):
        a += [r[k] for r in ref_rows]
    a += list(win_base) + list(ioffset)
    p = str(d / "bai.bin")
    open(p, "wb").write(struct.pack("<iQQ", n_ref, len(chunks), n_no_coor) + struct.pack("<%dQ" % len(a), *a))
    r = subprocess.run([prog, "bai", p, p + ".out"], capture_output=True, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw = open(p + ".out", "rb").read()
    return raw[:-8], struct.unpack("<Q", raw[-8:])[0]


@pytest.mark.parametrize("san", [False, True], ids=["plain", "sanitizers"])
def test_serialiser_writes_the_hand_written_bai(request, san):
    prog, d = request.getfixturevalue("exe_san" if san else "exe")
    _, bai = _hand_case()
    va0, va1, vb1 = (500 << 16), (500 << 16) | 60042, (1500 << 16) | 54804
    got, bins = _bai_arrays(prog, d, 2, [((0 << 32) | 585, va0, va1), ((1 << 32) | 4681, va1, vb1)], [(1, 0, va0, va1), (1, 0, va1, vb1)], [0, 2, 3], [va0, va0, va1], 1,
                            env=SAN_ENV if san else None)
    assert got == bai and bins == 2
    # no record at all: empty references, nothing else
    got, bins = _bai_arrays(prog, d, 3, [], [(0, 0, 0, 0)] * 3, [0, 0, 0, 0], [], 0, env=SAN_ENV if san else None)
    assert got == b"BAI\1" + struct.pack("<i", 3) + struct.pack("<ii", 0, 0) * 3 + struct.pack("<Q", 0) and bins == 0
    assert got == M.canonical_bai([], 3, [], 0)
