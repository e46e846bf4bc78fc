"""BAM, SAM and BGZF test inputs written in Python (zlib for the DEFLATE streams): the files `ngm-hip -q` is given in
test_gpu_bam_input.py, and the members test_bam_input_host.py / test_gpu_bgzf_inflate.py hand to the inflate core."""
import random
import struct
import zlib

CODES = b"=ACMGRSVTWYHKDBN"
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


# ---- BGZF -------------------------------------------------------------------------------------------------------------
def wrap_member(deflate, crc, isize):
    """a BGZF member around a raw DEFLATE stream: BSIZE from its length, the trailer as given"""
    bsize = 18 + len(deflate) + 8 - 1
    assert bsize < 65536
    return b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", bsize) + deflate + struct.pack("<II", crc & 0xFFFFFFFF, isize & 0xFFFFFFFF)


def member(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=0):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    if flush_every:
        parts = []
        for k, i in enumerate(range(0, len(data), flush_every)):
            parts.append(c.compress(data[i:i + flush_every]))
            parts.append(c.flush(zlib.Z_FULL_FLUSH if k % 2 else zlib.Z_SYNC_FLUSH))
        z = b"".join(parts) + c.flush()
    else:
        z = c.compress(data) + c.flush()
    return wrap_member(z, zlib.crc32(data), len(data))


def bgzf(data, member_size=0xFF00, level=6, eof=True):
    out = [member(data[i:i + member_size], level) for i in range(0, len(data), member_size)]
    return b"".join(out) + (EOF_MEMBER if eof else b"")


# ---- BAM / SAM --------------------------------------------------------------------------------------------------------
def bam_record(name, seq, qual, flag, cigar=(), ref_id=-1, pos=-1, mapq=0, tags=b""):
    """name, seq: bytes; qual: bytes of printable qualities (33 is taken off) or None (0xFF bytes); cigar: [(op, len)]"""
    name = name + b"\0"
    packed = bytearray((len(seq) + 1) // 2)
    for i, b in enumerate(seq):
        packed[i >> 1] |= CODES.index(bytes([b]).upper()) << (0 if i & 1 else 4)
    q = bytes([0xFF]) * len(seq) if qual is None else bytes(x - 33 for x in qual)
    cig = b"".join(struct.pack("<I", (n << 4) | op) for op, n in cigar)
    body = struct.pack("<iiIIiiii", ref_id, pos, (4680 << 16) | (mapq << 8) | len(name), (flag << 16) | len(cigar), len(seq), -1, -1, 0) + name + cig + bytes(packed) + q + tags
    return struct.pack("<I", len(body)) + body


def bam_bytes(records, refs=(), text=b"@HD\tVN:1.0\tSO:unsorted\n"):
    out = [b"BAM\1", struct.pack("<i", len(text)), text, struct.pack("<i", len(refs))]
    for name, length in refs:
        out.append(struct.pack("<i", len(name) + 1) + name + b"\0" + struct.pack("<i", length))
    return b"".join(out) + b"".join(records)


def revcomp(seq):
    return seq.translate(_COMP)[::-1]


def unaligned_bam(reads, paired=False, member_size=0xFF00, level=6):
    """reads: [(name, seq, qual)] as bytes; flags 4, or 77 / 141 for interleaved mates"""
    recs = [bam_record(n, s, q, (77 if i % 2 == 0 else 141) if paired else 4) for i, (n, s, q) in enumerate(reads)]
    return bgzf(bam_bytes(recs), member_size, level)


def sam_text(reads, paired=False, reverse_every=0):
    """an unaligned SAM; every reverse_every-th record is written as a reverse-strand record (flag 0x10: sequence reverse-complemented,
    qualities reversed), which the reader turns back into the read"""
    out = [b"@HD\tVN:1.0\tSO:unsorted\n", b"@CO\ta comment\twith\ttabs\tin\tit\tone\ttwo\tthree\tfour\tfive\tsix\n"]
    for i, (n, s, q) in enumerate(reads):
        flag = (77 if i % 2 == 0 else 141) if paired else 4
        if reverse_every and i % reverse_every == 0:
            flag, s, q = flag | 0x10, revcomp(s), q[::-1]
        out.append(b"\t".join([n, b"%d" % flag, b"*", b"0", b"0", b"*", b"*", b"0", b"0", s, q, b"RG:Z:g1"]) + b"\n")
    return b"".join(out)


# ---- members for the inflate tests ---------------------------------------------------------------------------------------
def fastq_text(n, seed):
    rnd = random.Random(seed)
    return b"".join(b"@read_%09d/1\n%s\n+\n%s\n" % (i, bytes(rnd.choice(b"ACGT") for _ in range(150)), bytes(rnd.choice(b"FFFFFFFFF:,#") for _ in range(150))) for i in range(n))


def bam_like(n, seed):
    rnd = random.Random(seed)
    return b"".join(bam_record(b"read_%09d" % i, bytes(rnd.choice(b"ACGT") for _ in range(150)), bytes(rnd.choice(b"FFFFFFFFF:,#") for _ in range(150)), 4,
                               tags=b"NMi" + struct.pack("<i", rnd.randrange(4)) + b"MDZ150\0") for i in range(n))


def good_cases():
    """name -> (members, text)"""
    rnd = random.Random(17)
    fq, bl = fastq_text(400, 5), bam_like(400, 6)
    c = {}

    def add(name, *parts):   # parts: (data, member bytes)
        c[name] = (b"".join(p[1] for p in parts), b"".join(p[0] for p in parts))

    def m(data, **kw):
        return (data, member(data, **kw))

    eof = (b"", EOF_MEMBER)
    add("eof_alone", eof)
    add("eof_between", m(fq[:3001]), eof, m(fq[3001:7000]), eof)
    add("one_byte", m(b"x"))
    add("stored_65280", m(rnd.randbytes(65280), level=0))
    add("stored_empty", m(b"", level=0))
    add("fixed_distance_one", m(bytes(65280), strategy=zlib.Z_FIXED))
    for lv in (1, 6, 9):
        add("fastq_level%d" % lv, m(fq[:65280], level=lv))
        add("bam_level%d" % lv, m(bl[:65280], level=lv))
    add("huffman_only", m(fq[:65280], strategy=zlib.Z_HUFFMAN_ONLY))
    add("rle", m(fq[:65280], strategy=zlib.Z_RLE))
    # hand-built (zlib's deflate gives neither on 65 280 bytes): codes of 13, 14 and 15 bits in the literal/length AND the distance set, all
    # of them used; and every one of the 30 distance codes, each with its shortest and its longest distance.  What the streams hold is
    # asserted in test_bam_input_host.py with the reader below (deflate_stats)
    add("long_codes", handmade_member(random.Random(31), skewed=True))
    add("all_distances", handmade_member(random.Random(32), skewed=False))
    add("flush_points", m(fq[:60000], flush_every=7001))
    add("isize_65536", m(fq[:65536]))
    add("random_65280", m(rnd.randbytes(65280)))
    add("one_member", m(fq[:12345]))
    add("three_members", m(fq[:1]), m(bl[:30001]), m(fq[1:777]))
    parts, at = [], 0
    for i in range(3000):   # odd sizes: unaligned output offsets, more members than the grid has workgroups
        n = (1, 37, 255, 1021, 4099)[i % 5] if i % 50 else 65280
        src = fq if i % 2 else bl
        at = (at + 977) % (len(src) - 65280)
        parts.append(m(src[at:at + n], level=(1, 6, 9)[i % 3]) if i % 7 else eof)
    add("three_thousand_members", *parts)
    return c


class _Bits:
    def __init__(self):
        self.bits = []

    def put(self, v, n):    # header fields and extra bits: least significant bit first
        self.bits.extend((v >> i) & 1 for i in range(n))

    def code(self, v, n):   # Huffman codes: most significant bit first
        self.bits.extend((v >> (n - 1 - i)) & 1 for i in range(n))

    def bytes(self):
        b = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(sum(x << i for i, x in enumerate(b[k:k + 8])) for k in range(0, len(b), 8))


_LBASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
_LEXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
_DBASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)
_DEXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)


def _complete_lengths(n, skewed):
    """n code lengths of a complete set (Kraft sum 1).  skewed: 1, 2, .. 14, 15, 15 with the shortest code split until there are n --
    the codes of 9 .. 15 bits stay; else as even as n allows"""
    ls = list(range(1, 15)) + [15, 15] if skewed else [1, 1]
    while len(ls) < n:
        ls.sort()
        ls[0:1] = [ls[0] + 1, ls[0] + 1]
    assert sum(2 ** (15 - l) for l in ls) == 2 ** 15 and max(ls) <= 15
    return ls


def _canonical(lens):
    """symbol -> (code, length), RFC 1951 3.2.2"""
    code, out = 0, {}
    for l in range(1, 16):
        for s, sl in enumerate(lens):
            if sl == l:
                out[s] = (code, l)
                code += 1
        code <<= 1
    return out


def handmade_member(rnd, skewed, size=65280):
    """(text, member): one dynamic block written here, token by token: all 286 literal/length codes and all 30 distance codes have a
    length (which symbol gets which is drawn); the tokens go round the 30 distance codes (the shortest and the longest distance of each,
    as soon as the text is long enough for it) and the 29 length codes, with the literals in between going round the 256 bytes"""
    lit_lens, dist_lens = _complete_lengths(286, skewed), _complete_lengths(30, skewed)
    rnd.shuffle(lit_lens)
    rnd.shuffle(dist_lens)
    lit, dist = _canonical(lit_lens), _canonical(dist_lens)
    b = _Bits()
    b.put(1, 1); b.put(2, 2)                       # last block, dynamic codes
    b.put(286 - 257, 5); b.put(30 - 1, 5); b.put(19 - 4, 4)
    for s in (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15):
        b.put(4 if s < 16 else 0, 3)               # the code-length code: 0 .. 15 in four bits each, no repeat codes
    for l in lit_lens + dist_lens:
        b.code(l, 4)
    out, k, nlit = bytearray(), 0, 0
    while len(out) < size:
        for _ in range(rnd.randrange(1, 4)):       # literals
            if len(out) < size:
                b.code(*lit[nlit % 256])
                out.append(nlit % 256)
                nlit += 1
        dc, lc = (k // 2) % 30, k % 29
        extra_d = 0 if k % 2 == 0 else (1 << _DEXTRA[dc]) - 1
        d = _DBASE[dc] + extra_d
        if d > len(out):                           # not that far back yet: a near one in its place
            dc, extra_d = k % 4, 0
            d = _DBASE[dc]
            if d > len(out):
                continue
        extra_l = rnd.randrange(1 << _LEXTRA[lc])
        n = _LBASE[lc] + extra_l
        k += 1
        if n > size - len(out):
            continue
        b.code(*lit[257 + lc]); b.put(extra_l, _LEXTRA[lc])
        b.code(*dist[dc]); b.put(extra_d, _DEXTRA[dc])
        for _ in range(n):
            out.append(out[-d])
    b.code(*lit[256])
    text = bytes(out)
    return text, wrap_member(b.bytes(), zlib.crc32(text), len(text))


def deflate_stats(member_bytes):
    """A reader for the first DEFLATE block of a member, which has to be a dynamic one: (lengths of the literal/length codes that occur
    in the block, lengths of the distance codes that occur, the set of distance codes that occur)"""
    z = member_bytes[18:-8]
    pos = 0

    def bits(n):
        nonlocal pos
        v = 0
        for i in range(n):
            v |= ((z[pos >> 3] >> (pos & 7)) & 1) << i
            pos += 1
        return v

    def reader(lens):
        table = {cl: s for s, cl in _canonical(lens).items()}

        def sym():
            code = 0
            for l in range(1, 16):
                code = (code << 1) | bits(1)
                if (code, l) in table:
                    return table[(code, l)]
            raise ValueError("no such code")
        return sym

    bits(1)
    assert bits(2) == 2
    hlit, hdist, hclen = bits(5) + 257, bits(5) + 1, bits(4) + 4
    pre = [0] * 19
    for s in (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)[:hclen]:
        pre[s] = bits(3)
    psym, lens = reader(pre), []
    while len(lens) < hlit + hdist:
        s = psym()
        if s < 16:
            lens.append(s)
        elif s == 16:
            lens += [lens[-1]] * (3 + bits(2))
        else:
            lens += [0] * (3 + bits(3) if s == 17 else 11 + bits(7))
    lit_lens, dist_lens = lens[:hlit], lens[hlit:]
    lsym, dsym = reader(lit_lens), reader(dist_lens)
    lit_used, dist_used = set(), set()
    while True:
        s = lsym()
        lit_used.add(s)
        if s == 256:
            break
        if s > 256:
            bits(_LEXTRA[s - 257])
            d = dsym()
            dist_used.add(d)
            bits(_DEXTRA[d])
    return {lit_lens[s] for s in lit_used}, {dist_lens[d] for d in dist_used}, dist_used


def damaged_cases():
    """name -> one damaged member (fixed bytes).  zlib refuses every one of them."""
    text = fastq_text(40, 9)
    good = member(text)
    deflate, crc = good[18:-8], zlib.crc32(text)
    d = {"wrong_crc": wrap_member(deflate, crc ^ 0x10, len(text)),
         "isize_too_small": wrap_member(deflate, crc, len(text) - 1),
         "isize_too_large": wrap_member(deflate, crc, len(text) + 1),
         "ends_before_end_of_block": wrap_member(deflate[:-12], crc, len(text))}
    from test_gz_inflate import _incomplete_literal_code_member
    z = _incomplete_literal_code_member()
    d["incomplete_literal_code"] = wrap_member(z[10:-8], zlib.crc32(b"\0\0"), 2)
    b = _Bits()
    b.put(1, 1); b.put(1, 2)           # last block, fixed codes
    b.code(0x30 + ord("a"), 8)         # literal 'a'
    b.code(1, 7)                       # length 3
    b.code(1, 5)                       # distance 2: one byte before the member's first
    b.code(0, 7)                       # end of block
    d["distance_before_first_byte"] = wrap_member(b.bytes(), zlib.crc32(b"aaaa"), 4)
    return d


def zlib_text(members):
    """what zlib makes of a run of members, or None where it refuses one"""
    out, rest = [], members
    try:
        while rest:
            o = zlib.decompressobj(31)
            out.append(o.decompress(rest))
            if not o.eof:
                return None
            rest = o.unused_data
    except zlib.error:
        return None
    return b"".join(out)
