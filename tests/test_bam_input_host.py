"""No GPU: the inflate core of nextgenmap_amd/csrc/bgzf_inflate_device.h (the __host__ __device__ functions the kernel runs) and
the SAM / BAM record code of nextgenmap_amd/csrc/bam_input.h, through tests/cpp/bam_input_driver.cpp.  The oracle of the inflate is
zlib; of the records a BAM / SAM parser written here after src/parser/BamParser.cpp:57-110 and src/parser/SamParser.cpp:89-161."""
import gzip
import os
import random
import struct
import subprocess
import zlib

import pytest

import bam_fixtures as BF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "bam_input_driver.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("bam_input")
    out = str(d / "bam_input_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", SRC, "-o", out, "-lz"])
    return out, d


@pytest.fixture(scope="module")
def exe_san(tmp_path_factory):
    d = tmp_path_factory.mktemp("bam_input_san")
    out = str(d / "bam_input_driver_san")
    c = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", out, "-lz"], capture_output=True, text=True)
    if c.returncode != 0:
        pytest.skip("no sanitizer runtime for g++ here: " + c.stderr[-200:])
    return out, d


SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")


def _run_cases(prog, d, cases, env=None):
    """[members] -> [(status, text)] in one process"""
    p = str(d / "cases.bin")
    with open(p, "wb") as f:
        for z in cases:
            f.write(struct.pack("<I", len(z)) + z)
    r = subprocess.run([prog, "cases", p, p + ".out"], capture_output=True, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw, out, at = open(p + ".out", "rb").read(), [], 0
    while at < len(raw):
        st, n = struct.unpack_from("<II", raw, at)
        out.append((st, raw[at + 8:at + 8 + n]))
        at += 8 + n
    assert len(out) == len(cases)
    return out


def test_inflate_core_equals_zlib(exe):
    prog, d = exe
    cases = BF.good_cases()
    got = _run_cases(prog, d, [z for z, _ in cases.values()])
    for (name, (z, text)), (st, out) in zip(cases.items(), got):
        assert BF.zlib_text(z) == text, name
        assert st == 0 and out == text, (name, st)


def test_hand_built_members_hold_what_their_names_say():
    """`long_codes`: codes of 13, 14 and 15 bits occur in the literal/length set and in the distance set (the decoder's one-lookup tables
    end at 10 and 8 bits).  `all_distances`: each of the 30 distance codes occurs.  Read off the streams by a DEFLATE reader of the
    test's own; zlib's deflate reaches neither on 65 280 bytes (its longest distance code in this suite has 12 bits)."""
    cases = BF.good_cases()
    lit, dist, _ = BF.deflate_stats(cases["long_codes"][0])
    assert {13, 14, 15} <= lit and {13, 14, 15} <= dist
    _, _, used = BF.deflate_stats(cases["all_distances"][0])
    assert used == set(range(30))
    # (the reader itself, on a member zlib wrote)
    lit, dist, used = BF.deflate_stats(cases["fastq_level6"][0])
    assert max(lit) <= 15 and max(dist) <= 15 and used <= set(range(30))


def test_fixed_damaged_members_are_refused(exe):
    prog, d = exe
    good = BF.member(BF.fastq_text(30, 2))
    for name, z in BF.damaged_cases().items():
        assert BF.zlib_text(z) is None, name
        p = str(d / (name + ".bgzf"))
        open(p, "wb").write(good + z + good)
        r = subprocess.run([prog, "inflate", p, p + ".out"], capture_output=True, text=True)
        assert r.returncode == 3 and r.stdout.startswith("member 1 status"), (name, r.returncode, r.stdout)


def test_chain_walk_refusals(exe):
    """no BC subfield, a BSIZE past the end, an ISIZE above 65536: refused by the host before any launch"""
    prog, d = exe
    good = BF.member(b"hello\n")
    no_bc = bytearray(good); no_bc[12:14] = b"XY"
    past = bytearray(good); struct.pack_into("<H", past, 16, len(good) + 5)
    big = bytearray(good); struct.pack_into("<I", big, len(big) - 4, 65537)
    plain_gzip = gzip.compress(b"hello\n")
    got = _run_cases(prog, d, [bytes(no_bc), bytes(past), bytes(big), plain_gzip, good[:-1], good + b"\0", good])
    assert [st for st, _ in got] == [100, 100, 100, 100, 100, 100, 0]


def test_bc_subfield_behind_another_one(exe):
    """the BC subfield is looked for among all subfields of the extra field, in the first member too (what `ngm-hip` asks before it
    takes the GPU route: inflate::first_member_is_bgzf is the same walk)"""
    prog, d = exe
    text = BF.fastq_text(20, 3)
    good = BF.member(text)
    other = b"XY\x03\0abc"
    size = len(good) + len(other)
    m = good[:10] + struct.pack("<H", 6 + len(other)) + other + b"BC\x02\0" + struct.pack("<H", size - 1) + good[18:]
    assert BF.zlib_text(m + good) == text * 2
    got = _run_cases(prog, d, [m + good, good + m])
    assert got == [(0, text * 2), (0, text * 2)]


def _damaged(rnd, base):
    """one member of `base` with its DEFLATE stream and trailer damaged; the header (BSIZE) fits what is left"""
    body = bytearray(rnd.choice(base)[18:])
    mode = rnd.randrange(4)
    if mode == 0:
        for _ in range(rnd.randrange(1, 4)):
            body[rnd.randrange(len(body))] ^= 1 << rnd.randrange(8)
    elif mode == 1:
        body = body[:rnd.randrange(8, len(body))]
    elif mode == 2:
        a = rnd.randrange(len(body))
        body[a:a + rnd.randrange(1, 50)] = rnd.randbytes(rnd.randrange(1, 50))
    else:
        a = rnd.randrange(len(body))
        del body[a:a + rnd.randrange(1, 30)]
    if len(body) < 8:
        body += bytes(8 - len(body))
    body = body[:65536 - 18]
    crc, isize = struct.unpack_from("<II", body, len(body) - 8)
    return BF.wrap_member(bytes(body[:-8]), crc, isize)


def test_damaged_members_under_sanitizers(exe_san):
    """300 seeded damaged members through the AddressSanitizer + UndefinedBehaviorSanitizer build (text stage and input are heap blocks
    of exactly their sizes): each is refused, or inflated to exactly zlib's bytes; never a crash.  zlib alone refuses more than two
    thirds of this seed's members (asserted), and so must the core."""
    prog, d = exe_san
    rnd = random.Random(20)
    base = [BF.member(BF.fastq_text(200, 1), 1), BF.member(BF.fastq_text(200, 2), 9), BF.member(rnd.randbytes(30000), 6), BF.member(bytes(60000), 6),
            BF.member(BF.bam_like(200, 3), 6), BF.member(BF.fastq_text(100, 4), strategy=zlib.Z_FIXED)]
    cases = [_damaged(rnd, base) for _ in range(300)]
    want = [BF.zlib_text(z) for z in cases]
    assert sum(w is None for w in want) > 200
    got = _run_cases(prog, d, cases, env=SAN_ENV)
    refused = 0
    for i, ((st, out), w) in enumerate(zip(got, want)):
        if st != 0:
            refused += 1
        else:
            assert w is not None and out == w, i
    assert refused > 200
    # the fixed members of the GPU test, and the good ones, through the same build
    fixed = list(BF.damaged_cases().values())
    assert all(st != 0 for st, _ in _run_cases(prog, d, fixed, env=SAN_ENV))
    good = BF.good_cases()
    for (name, (z, text)), (st, out) in zip(good.items(), _run_cases(prog, d, [z for z, _ in good.values()], env=SAN_ENV)):
        assert st == 0 and out == text, name


# ---- records ------------------------------------------------------------------------------------------------------------
def _bam_reads(data):
    """name, sequence, qualities of every record as ngm reads them (BamParser.cpp:57-110; no qualities: '*')"""
    assert data[:4] == b"BAM\1"
    at = 8 + struct.unpack_from("<i", data, 4)[0]
    n_ref, = struct.unpack_from("<i", data, at)
    at += 4
    for _ in range(n_ref):
        at += 8 + struct.unpack_from("<i", data, at)[0]
    out = []
    while at < len(data):
        block, = struct.unpack_from("<i", data, at)
        _, _, bin_mq_nl, flag_nc, l_seq = struct.unpack_from("<iiIIi", data, at + 4)
        l_name, n_cig, flag = bin_mq_nl & 0xFF, flag_nc & 0xFFFF, flag_nc >> 16
        p = at + 36
        name = data[p:p + l_name - 1]; p += l_name + 4 * n_cig
        seq = bytes(BF.CODES[(data[p + (i >> 1)] >> (0 if i & 1 else 4)) & 15] for i in range(l_seq)); p += (l_seq + 1) // 2
        qual = bytes(x + 33 for x in data[p:p + l_seq]) if l_seq and data[p] != 0xFF else b""
        if flag & 0x10:
            seq, qual = BF.revcomp(seq), qual[::-1]
        out.append((name, seq, qual))
        at += 4 + block
    return out


def _lines(reads):
    return b"".join(n + b"\t" + s + b"\t" + (q or b"*") + b"\n" for n, s, q in reads)


def _mixed_records():
    rnd = random.Random(4)
    recs = []
    for i in range(900):
        n = (1, 2, 3, 16, 33, 100, 101, 0)[i % 8]
        seq = bytes(rnd.choice(BF.CODES) for _ in range(n)) if i % 3 else BF.CODES[:n] + bytes(rnd.choice(b"ACGT") for _ in range(max(0, n - 16)))
        qual = None if i % 11 == 0 else bytes(rnd.randrange(33, 74) for _ in range(n))
        flag = (4, 16, 77, 141, 0x110 | 16, 0)[i % 6]
        cigar = [(0, n)] if n and not flag & 4 else []
        recs.append(BF.bam_record(b"rec%d" % i, seq, qual, flag, cigar, ref_id=0 if cigar else -1, pos=i, tags=b"NMi" + struct.pack("<i", i) + b"XSZab c\0"))
    return BF.bam_bytes(recs, refs=[(b"chr1", 1000), (b"chrUn_2", 55)])


def test_bam_records(exe):
    """odd and even l_seq, l_seq 1 and 0, every 4-bit code, flag 0x10, records without qualities, CIGAR and tags present; the BAM cut into
    members of 4 000 bytes, so that records straddle them, inflated by the core and decoded"""
    prog, d = exe
    data = _mixed_records()
    z = BF.bgzf(data, member_size=4000)
    assert len(z) > 10 * 4000 // 3
    p = str(d / "mixed.bam")
    open(p, "wb").write(z)
    assert subprocess.run([prog, "inflate", p, p + ".raw"]).returncode == 0
    assert open(p + ".raw", "rb").read() == data
    assert subprocess.run([prog, "records", p + ".raw", p + ".txt"]).returncode == 0
    want = _bam_reads(data)
    assert len(want) == 900 and any(q == b"" for _, _, q in want)
    assert open(p + ".txt", "rb").read() == _lines(want)
    r = subprocess.run([prog, "index", p + ".raw", "256"], capture_output=True, text=True)
    offs = [int(x) for x in r.stdout.split()]
    assert offs[-1] == 900 and len(offs) == 5
    at, k = data.index(b"rec0\0") - 36, 0
    for i in range(900):
        if i % 256 == 0:
            assert offs[k] == at
            k += 1
        at += 4 + struct.unpack_from("<i", data, at)[0]


def test_sam_lines(exe):
    prog, d = exe
    lines = [b"@HD\tVN:1.0", b"@SQ\tSN:chr1\tLN:1000",   # (an empty line before the first record would make it FASTQ for DetermineParser)
             b"r1\t4\t*\t0\t0\t*\t*\t0\t0\tACGTNacgtn\tIIIIIHHHHH", b"", b"@CO\tlate comment",
             b"r2\t16\tchr1\t5\t60\t10M\t*\t0\t0\tAACCGGTTNRacgt\tABCDEFGHIJKLMN\tNM:i:0\tXS:Z:a b",
             b"r3\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\t*",
             b"r4\t272\tchr1\t5\t0\t4M\t*\t0\t0\tacgT\t*",
             b"", b"r5\t77\t*\t0\t0\t*\t*\t0\t0\tA\t#", b"r6\t141\t*\t0\t0\t*\t*\t0\t0\tC\t$\r"]
    want = [(b"r1", b"ACGTNacgtn", b"IIIIIHHHHH"), (b"r2", b"tgcaRNAACCGGTT", b"NMLKJIHGFEDCBA"), (b"r3", b"ACGT", b""), (b"r4", b"Agca", b""), (b"r5", b"A", b"#"), (b"r6", b"C", b"$")]
    for tail in (b"\n", b""):
        p = str(d / "lines.sam")
        open(p, "wb").write(b"\n".join(lines) + tail)
        assert subprocess.run([prog, "records", p, p + ".txt"]).returncode == 0
        assert open(p + ".txt", "rb").read() == _lines(want)
    open(p, "wb").write(b"r1\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\tIII\n")
    r = subprocess.run([prog, "records", p, p + ".txt"], capture_output=True, text=True)
    assert r.returncode == 3 and "lengths differ (r1)" in r.stderr


def test_format_detection(exe):
    prog, d = exe
    reads = [(b"a%d" % i, b"ACGT" * 10, b"I" * 40) for i in range(50)]
    fq = b"".join(b"@" + n + b"\n" + s + b"\n+\n" + q + b"\n" for n, s, q in reads)
    fa = b"".join(b">" + n + b"\n" + s + b"\n" for n, s, q in reads)
    sam = BF.sam_text(reads)   # (its @CO line has more than 10 tabs: '@' lines do not count)
    long_header = b"".join(b"@SQ\tSN:contig%d\tLN:1000\n" % i for i in range(9000)) + sam
    bam = BF.bam_bytes([BF.bam_record(n, s, q, 4) for n, s, q in reads])
    for name, data, want in (("fq", fq, "fastx"), ("fa", fa, "fastx"), ("sam", sam, "sam"), ("long_header_sam", long_header, "sam"), ("bam", bam, "bam")):
        for tag, blob in (("plain", data), ("gzip", gzip.compress(data)), ("bgzf", BF.bgzf(data, 3000))):
            if name == "bam" and tag == "gzip":
                continue
            p = str(d / ("detect_%s_%s" % (name, tag)))
            open(p, "wb").write(blob)
            assert subprocess.run([prog, "detect", p], capture_output=True, text=True).stdout.strip() == want, (name, tag)


def _damaged_bams():
    good = [BF.bam_record(b"ok%d" % i, b"ACGTACGTAC", b"IIIIIIIIII", 4) for i in range(3)]
    rec = bytearray(BF.bam_record(b"bad", b"ACGTACGTAC", b"IIIIIIIIII", 4))
    def mod(off, fmt, v):
        r = bytearray(rec); struct.pack_into(fmt, r, off, v); return bytes(r)
    return {"block_size_below_32": mod(0, "<I", 31), "block_size_past_the_end": mod(0, "<I", 100000), "l_read_name_0": mod(12, "<B", 0),
            "fields_longer_than_record": mod(20, "<i", 40), "cigar_longer_than_record": mod(16, "<H", 60000), "l_seq_huge": mod(20, "<I", 0xFFFFFFF0),
            "truncated_last_record": bytes(rec[:-7]), "truncated_block_size": bytes(rec[:2])}, good


def test_damaged_records_are_refused(exe, request):
    progs = [exe[0]]
    try:
        progs.append(request.getfixturevalue("exe_san")[0])   # (the sanitizer build too, where there is one: never a crash)
    except pytest.skip.Exception:
        pass
    d = exe[1]
    cases, good = _damaged_bams()
    for prog in progs:
        for name, bad in cases.items():
            p = str(d / (name + ".raw"))
            open(p, "wb").write(BF.bam_bytes(good + [bad]))
            r = subprocess.run([prog, "records", p, p + ".txt"], capture_output=True, text=True, env=SAN_ENV)
            assert r.returncode == 3 and r.stderr.startswith("BAM input: "), (name, r.returncode, r.stderr[-2000:])
        for name, data in (("no_magic", b"BAM\2" + bytes(40)), ("header_past_end", b"BAM\1" + struct.pack("<i", 1000) + bytes(20)),
                           ("dictionary_past_end", b"BAM\1" + struct.pack("<ii", 0, 3) + struct.pack("<i", 500) + bytes(10))):
            p = str(d / (name + ".raw"))
            open(p, "wb").write(data)
            r = subprocess.run([prog, "records", p, p + ".txt"], capture_output=True, text=True, env=SAN_ENV)
            assert r.returncode == 3 and r.stderr.startswith("BAM input: "), (name, r.returncode, r.stderr[-2000:])
