"""A plain-Python restatement of what `ngm-hip --sort` must write (include/ngm_pipeline.h): samtools' coordinate order
with input order as the tie-break, and the canonical BAI file (SAM specification 5.2) of a sorted record stream cut into BGZF members
of 0xFF00 input bytes.  Plus a reader that answers a region query from a BAM file and its BAI the way an index user does: bins of the
region, chunks dropped below the linear offset, a seek by virtual offset, single members inflated with zlib."""
import struct
import zlib

MEMBER = 0xFF00
PSEUDO_BIN = 37450


def walk(data):
    """[(offset, size)] of a run of whole BAM records; ValueError where the sorter's host walk refuses the chain"""
    out, at = [], 0
    while at < len(data):
        if len(data) - at < 4:
            raise ValueError("chain")
        bs, = struct.unpack_from("<I", data, at)
        if bs < 32:
            raise ValueError("block_size")
        if at + 4 + bs > len(data):
            raise ValueError("chain")
        l_name, n_cig, l_seq = data[at + 12], struct.unpack_from("<I", data, at + 16)[0] & 0xFFFF, struct.unpack_from("<i", data, at + 20)[0]
        if l_seq < 0 or l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq > bs - 32:
            raise ValueError("fields")
        out.append((at, bs + 4))
        at += bs + 4
    return out


def fields(rec):
    """(refID, pos, end, flag) of one record: end = pos + the lengths of its M, D, N, = and X operations, pos + 1 without any"""
    ref_id, pos, bmn, fnc = struct.unpack_from("<iiII", rec, 4)
    at, span = 36 + (bmn & 0xFF), 0
    for k in range(fnc & 0xFFFF):
        v, = struct.unpack_from("<I", rec, at + 4 * k)
        if v & 15 in (0, 2, 3, 7, 8):
            span += v >> 4
    return ref_id, pos, pos + (span or 1), fnc >> 16


def key(rec):
    ref_id, pos, _, flag = fields(rec)
    return (ref_id & 0xFFFFFFFF, (pos + 1) & 0x7FFFFFFF, (flag >> 4) & 1)


def sort_records(records):
    """records in input order -> coordinate order (sorted() is stable)"""
    return sorted(records, key=key)


def reg2bin(beg, end):
    end -= 1
    for shift, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return base + (beg >> shift)
    return 0


def reg2bins(beg, end):
    end -= 1
    out = [0]
    for shift, base in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out += range(base + (beg >> shift), base + (end >> shift) + 1)
    return out


def canonical_bai(sorted_records, n_ref, member_sizes, first_member_offset):
    """sorted_records: the records in file order; member_sizes: compressed bytes of every member of their stream"""
    C = [0]
    for z in member_sizes:
        C.append(C[-1] + z)
    V = lambda u: ((first_member_offset + C[u // MEMBER]) << 16) | (u % MEMBER)
    refs = [dict(bins={}, first=None, last=None, mapped=0, unmapped=0, win={}, max_end=0) for _ in range(n_ref)]
    u, no_coor, prev = 0, 0, None
    for rec in sorted_records:
        ref_id, pos, end, flag = fields(rec)
        vbeg, vend = V(u), V(u + len(rec))
        u += len(rec)
        if ref_id < 0:
            no_coor += 1
            continue
        r, b = refs[ref_id], reg2bin(pos, end)
        if prev == (ref_id, b):
            r["bins"][b][-1][1] = vend          # the run of consecutive records of this reference and bin goes on
        else:
            r["bins"].setdefault(b, []).append([vbeg, vend])
        prev = (ref_id, b)
        r["first"] = vbeg if r["first"] is None else r["first"]
        r["last"] = vend
        r["unmapped" if flag & 4 else "mapped"] += 1
        r["max_end"] = max(r["max_end"], end)
        for w in range(pos >> 14, ((end - 1) >> 14) + 1):
            r["win"].setdefault(w, vbeg)          # sorted input: the first record to reach a window has the smallest vbeg
    out = [b"BAI\1", struct.pack("<i", n_ref)]
    for r in refs:
        out.append(struct.pack("<i", len(r["bins"]) + (1 if r["first"] is not None else 0)))
        for b in sorted(r["bins"]):
            out.append(struct.pack("<Ii", b, len(r["bins"][b])) + b"".join(struct.pack("<QQ", *c) for c in r["bins"][b]))
        if r["first"] is not None:
            out.append(struct.pack("<IiQQQQ", PSEUDO_BIN, 2, r["first"], r["last"], r["mapped"], r["unmapped"]))
        n_intv = ((r["max_end"] - 1) >> 14) + 1 if r["max_end"] else 0
        io, nxt = [0] * n_intv, 0
        for w in range(n_intv - 1, -1, -1):       # an empty window takes the value of the next one that has a record
            nxt = r["win"].get(w, nxt)
            io[w] = nxt
        out.append(struct.pack("<i", n_intv) + struct.pack("<%dQ" % n_intv, *io))
    out.append(struct.pack("<Q", no_coor))
    return b"".join(out)


def member_sizes(members):
    """compressed sizes and ISIZEs of a run of whole BGZF members"""
    sizes, isizes, at = [], [], 0
    while at < len(members):
        assert members[at:at + 4] == b"\x1f\x8b\x08\x04" and members[at + 12:at + 16] == b"BC\x02\0", at
        n = struct.unpack_from("<H", members, at + 16)[0] + 1
        sizes.append(n)
        isizes.append(struct.unpack_from("<I", members, at + n - 4)[0])
        at += n
    assert at == len(members)
    return sizes, isizes


def parse_bai(bai):
    assert bai[:4] == b"BAI\1"
    n_ref, = struct.unpack_from("<i", bai, 4)
    at, refs = 8, []
    for _ in range(n_ref):
        n_bin, = struct.unpack_from("<i", bai, at)
        at += 4
        bins = {}
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", bai, at)
            bins[b] = [struct.unpack_from("<QQ", bai, at + 8 + 16 * k) for k in range(n_chunk)]
            at += 8 + 16 * n_chunk
        n_intv, = struct.unpack_from("<i", bai, at)
        refs.append((bins, struct.unpack_from("<%dQ" % n_intv, bai, at + 4)))
        at += 4 + 8 * n_intv
    n_no_coor, = struct.unpack_from("<Q", bai, at)
    assert at + 8 == len(bai)
    return refs, n_no_coor


def query(bam, bai, ref_id, beg, end):
    """the records of file `bam` (bytes) that overlap [beg, end) of reference ref_id, found through the index"""
    refs, _ = parse_bai(bai)
    bins, ioffset = refs[ref_id]
    min_off = ioffset[beg >> 14] if (beg >> 14) < len(ioffset) else (ioffset[-1] if ioffset else 0)
    chunks = sorted(c for b in reg2bins(beg, end) if b in bins and b != PSEUDO_BIN for c in bins[b] if c[1] > min_off)
    found = {}
    for vbeg, vend in chunks:
        coff, at, data, mem = vbeg >> 16, vbeg & 0xFFFF, b"", []   # mem: (file offset of a member, where its text starts and ends in data)

        def more():   # the next member, inflated on its own
            nonlocal coff, data
            assert coff < len(bam), "the chunk runs past the end of the file"
            n = struct.unpack_from("<H", bam, coff + 16)[0] + 1
            text = zlib.decompress(bam[coff + 18:coff + n - 8], -15)
            mem.append((coff, len(data), len(data) + len(text)))
            data += text
            coff += n

        def voff(at):   # (at the end of the inflated text: offset 0 of the next member)
            return next(((fo << 16) | (at - a) for fo, a, e in mem if at < e), coff << 16)
        more()
        while voff(at) < vend:
            while len(data) < at + 4 or len(data) < at + 4 + struct.unpack_from("<I", data, at)[0]:
                more()
            rec = data[at:at + 4 + struct.unpack_from("<I", data, at)[0]]
            r, pos, rend, _ = fields(rec)
            if r != ref_id or pos >= end:
                break
            if rend > beg:
                found[voff(at)] = rec
            at += len(rec)
    return [found[v] for v in sorted(found)]


def scan(records, ref_id, beg, end):
    """the same answer from a scan of all records (file order)"""
    out = []
    for rec in records:
        r, pos, rend, _ = fields(rec)
        if r == ref_id and pos < end and rend > beg:
            out.append(rec)
    return out
