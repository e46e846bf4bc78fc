"""A plain model of the record writers: constructed mapping results -> SAM lines or BAM record bytes, plus the writers' counters.
Written from the reference program's writer code, line by line, with numpy float32 where that code computes in `float`; it is what
tests/test_gpu_sam_records.py holds the GPU writers (csrc/sam_device.h, through ngm_debug_sam_records) against, and what
tests/test_sam_model.py holds against the hand-typed expectations of tests/sam_cases.py and against the host formatter (csrc/cli_format.h).

What it restates:
  src/writer/GenericReadWriter.h:190-304   WriteRead / WritePair: empty reads are discarded, the min_identity / min_residues / min_mq filters
  src/AlignmentBuffer.cpp:175-199          the proper-pair check and its three counters
  src/writer/SAMWriter.cpp:98-372          DoWriteReadGeneric, DoWritePair, DoWriteUnmappedReadGeneric
  src/writer/BAMWriter.cpp:147-433         the same three for BAM (TLEN over the whole read, 0-based mate fields)
  lib/bamtools-2.3.0/src/api/internal/bam/BamWriter_p.cpp:33-41, :180-300   CalculateMinimumBin, WriteAlignment (packed CIGAR, nibbles, phred values)
  src/writer/GenericReadWriter.h:87-186    computeSlaSeqTags

Three things are the project's, not the reference's, and are kept as the project documents them:
  * a quality string shorter than the read: the reference copies `length` bytes from its buffer whatever the string's length; here the string
    is its first min(qual_len, L) characters, SAM prints what there is, BAM pads with ':' (cli_format.h oriented_qual);
  * a base outside "=ACMGRSVTWYHKDBN" makes bamtools throw (BamWriter_p.cpp:125-127); here it is packed as N (15);
  * which columns of an M run the alignment kernel labelled 'X' (the `match` flag of SWOclCigar.cpp:484-540's records) is decided outside the
    writers: `column_is_match` below restates the project's rule for the two kernel variants.
"""
import math
import struct

import numpy as np

F = np.float32
PAIR_FAILED, PAIR_LOST = 2, 4
VARIANT_OCL_CPU = 1
BASES = "=ACMGRSVTWYHKDBN"
BRANCHES = ("none", "only1", "only2", "proper_fwd", "proper_rev", "not_proper")


def complement(ch):
    return {"A": "T", "T": "A", "C": "G", "G": "C"}.get(ch, ch)


def revcomp(s):
    return "".join(complement(c) for c in reversed(s))


def identity_rounded(identity):
    """SAMWriter.cpp:189 / BAMWriter.cpp:256: round(Identity * 10000.0f) / 10000.0f in float, halves away from zero"""
    x = float(F(identity) * F(10000.0))
    if math.isnan(x) or math.isinf(x):
        return F(x)
    r = math.copysign(math.floor(abs(x) + 0.5), x)   # (exact in double: |x| is a float32)
    return F(r) / F(10000.0)


def xi_text(identity):
    return "%g" % float(identity_rounded(identity))   # SAMWriter.cpp:190


def cigar_ops(cigar):
    """BAMWriter.cpp:207-215: (length, operation) of every operation character"""
    ops, num = [], 0
    for ch in cigar:
        if ch.isdigit():
            num = num * 10 + int(ch)
        else:
            ops.append((num, ch))
            num = 0
    return ops


def ref_span(cigar):   # BamAlignment::GetEndPosition: M, D, N, =, X advance the reference
    return sum(n for n, op in cigar_ops(cigar) if op in "MDN=X")


def min_bin(begin, end):   # BamWriter_p.cpp:33-41, signed shifts as there
    end -= 1
    for shift, off in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if begin >> shift == end >> shift:
            return off + (begin >> shift)
    return 0


def ref_class(ch):
    """the packed genome's symbol classes (ngm_ref_create: any case, everything but ACGT is N)"""
    return {"A": 0, "C": 1, "G": 2, "T": 3}.get(ch.upper(), 5)


def column_is_match(variant, alt_scoring, read_ch, ref_cls):
    rc = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 5}.get(read_ch, 4)
    if variant != VARIANT_OCL_CPU:   # the GPU kernels compare the characters
        return read_ch == "ACGTxN"[ref_cls]
    return rc == ref_cls if alt_scoring else (rc <= 3 and rc == ref_cls)


class Model:
    """opts: paired, min_insert, max_insert (<= 0: none), min_mq, min_identity, min_residues, no_unal, rg, bs_mapping, slam_seq, clip (hard or
    silent: both print the aligned part only), variant, alt_scoring, xa_tag.  contigs: (name, length, bases or None)."""

    def __init__(self, opts, contigs, bam):
        o = dict(paired=0, min_insert=0, max_insert=0, min_mq=0, min_identity=0.65, min_residues=0.5, no_unal=0, rg="", bs_mapping=0, slam_seq=0, clip=0,
                 variant=0, alt_scoring=0, xa_tag=0)
        o.update(opts)
        self.o, self.contigs, self.bam = o, contigs, bam
        self.max_insert = o["max_insert"] if o["max_insert"] > 0 else 2147483647
        self.out = []        # one str (SAM line without its newline) or bytes (BAM record) per record written
        self.total = self.mapped = 0
        self.pairs = self.broken = self.insert_sum = 0
        self.tally = dict((b, 0) for b in BRANCHES)
        self.tally.update(fail_mq=0, fail_identity=0, fail_residues=0, short_qual=0, fwd=0, rev=0)

    # ---- GenericReadWriter.h:205-215, :265-283 ----
    def passes(self, r):
        h, L = r.hit, len(r.row)
        if not h.mapped:
            return False
        min_res = F(self.o["min_residues"])
        if min_res <= F(1.0):
            min_res = F(L) * min_res
        ok_mq = h.mapq >= self.o["min_mq"]
        ok_id = F(h.identity) >= F(self.o["min_identity"])
        ok_res = F(L - h.qstart - h.qend) >= min_res
        self.tally["fail_mq"] += not ok_mq
        self.tally["fail_identity"] += not ok_id
        self.tally["fail_residues"] += not ok_res
        return bool(ok_mq and ok_id and ok_res)

    # ---- GenericReadWriter.h:87-186 over the columns of the M runs ----
    def slam_tags(self, r):
        h, L = r.hit, len(r.row)
        name, length, bases = self.contigs[h.contig]
        read = revcomp(r.row) if h.reverse else r.row
        rates, mp = [0] * 25, []
        read_i, ref_i = h.qstart, 0
        for num, op in cigar_ops(h.cigar):
            if op == "M":
                for k in range(num):
                    fc = ref_class(bases[h.pos + ref_i + k])
                    ch = read[read_i + k]
                    rc = {"A": 0, "C": 1, "G": 2, "T": 3}.get(ch, 4)   # trans[]
                    t = 5 * (fc if fc <= 3 else 4) + rc
                    rates[t] += 1
                    if not column_is_match(self.o["variant"], self.o["alt_scoring"], ch, fc):
                        mp.append("%d:%d:%d" % (t, read_i + k + 1, ref_i + k + 1))
                read_i += num
                ref_i += num
            elif op == "I":
                read_i += num
            elif op == "D":
                ref_i += num
        tc = rates[0 * 5 + 2] if h.reverse else rates[3 * 5 + 1]
        return tc, "".join("%d," % v for v in rates), ",".join(mp)   # ra: every count followed by a comma (:172)

    def zs(self, h, flags):   # SAMWriter.cpp:173-187
        second = self.o["paired"] and (flags & 0x80)
        return ("+-" if h.reverse else "--") if second else ("-+" if h.reverse else "++")

    def oriented(self, r):
        """the bases and qualities as a mapped record holds them, and whether there is a quality string"""
        h, L = r.hit, len(r.row)
        qlen = r.qual_len & 0x7FFF
        seq = revcomp(r.row) if h.reverse else r.row
        qual = r.qual[:min(qlen, L)]
        if h.reverse:
            qual = qual[::-1]
        if self.o["clip"]:   # SAMWriter.cpp:143-146, BAMWriter.cpp:189-192
            sl = L - h.qstart - h.qend
            seq, qual = seq[h.qstart:h.qstart + sl], qual[h.qstart:h.qstart + sl]
        if qlen and qlen < L:
            self.tally["short_qual"] += 1
        return seq, qual, qlen == 0

    # ---- SAMWriter.cpp:98-228, BAMWriter.cpp:147-304 ----
    def write_mapped(self, r, flags, rnext, pnext, tlen, bm):
        h, L, o = r.hit, len(r.row), self.o
        if h.reverse:
            flags |= 0x10
        self.tally["rev" if h.reverse else "fwd"] += 1
        seq, qual, noq = self.oriented(r)
        score, votes, xr = int(F(h.score)), int(F(h.votes)), L - h.qstart - h.qend
        if self.bam:
            tags = b"ASi" + struct.pack("<i", score) + b"NMi" + struct.pack("<i", h.nm) + b"NHi" + struct.pack("<i", h.n_best)
            if o["bs_mapping"]:
                tags += b"ZSZ" + self.zs(h, flags).encode() + b"\0"
            tags += b"XIf" + struct.pack("<f", identity_rounded(h.identity))
            if o["xa_tag"]:
                tags += b"XAi" + struct.pack("<i", r.polya)
            tags += b"X0i" + struct.pack("<i", h.n_best) + b"XEi" + struct.pack("<i", votes) + b"XRi" + struct.pack("<i", xr) + b"MDZ" + h.md.encode() + b"\0"
            if o["rg"]:
                tags += b"RGZ" + o["rg"].encode() + b"\0"
            if o["slam_seq"]:
                tc, ra, mp = self.slam_tags(r)
                tags += b"TCi" + struct.pack("<i", tc) + b"RAZ" + ra.encode() + b"\0"
                if mp:
                    tags += b"MPZ" + mp.encode() + b"\0"
            quals = b":" * len(seq) if noq else (qual + ":" * (len(seq) - len(qual))).encode("latin-1")
            self.bam_record(r, flags, h.contig, h.pos, h.mapq, h.cigar, seq, quals, bm[0], bm[1], bm[2], tags)
            return
        f = [r.name, "%d" % flags, self.contigs[h.contig][0], "%d" % (h.pos + 1), "%d" % h.mapq, h.cigar, rnext, "%d" % pnext, "%d" % tlen, seq, "*" if noq else qual]
        if o["rg"]:
            f.append("RG:Z:" + o["rg"])
        f += ["AS:i:%d" % score, "NM:i:%d" % h.nm, "NH:i:%d" % h.n_best]
        if o["bs_mapping"]:
            f.append("ZS:Z:" + self.zs(h, flags))
        f += ["XI:f:" + xi_text(h.identity), "X0:i:%d" % h.n_best]
        if o["xa_tag"]:
            f.append("XA:i:%d" % r.polya)
        f += ["XE:i:%d" % votes, "XR:i:%d" % xr, "MD:Z:" + h.md]
        if o["slam_seq"]:
            tc, ra, mp = self.slam_tags(r)
            f += ["TC:i:%d" % tc, "RA:Z:" + ra[:-1]]   # "%.*s", raIndex - 1 (:213): without the last comma
            if mp:
                f.append("MP:Z:" + mp)
        self.out.append("\t".join(f))

    # ---- SAMWriter.cpp:312-368, BAMWriter.cpp:306-376: contig < 0 prints '*' / -1 ----
    def write_unmapped(self, r, flags, contig, pos1, rnext, pnext1):
        if self.o["no_unal"]:
            return
        o, L = self.o, len(r.row)
        qlen = r.qual_len & 0x7FFF
        qual = r.qual[:min(qlen, L)]
        if qlen and qlen < L:
            self.tally["short_qual"] += 1
        flags |= 0x4
        if self.bam:
            tags = b""
            if o["xa_tag"]:
                tags += b"XAi" + struct.pack("<i", r.polya)
            if o["rg"]:
                tags += b"RGZ" + o["rg"].encode() + b"\0"
            ref, p0 = (contig, pos1 - 1) if contig >= 0 else (-1, -1)
            quals = b":" * L if qlen == 0 else (qual + ":" * (L - len(qual))).encode("latin-1")
            self.bam_record(r, flags, ref, p0, 0, "", r.row, quals, ref, p0, 0, tags)
            return
        line = "\t".join([r.name, "%d" % flags, self.contigs[contig][0] if contig >= 0 else "*", "%d" % pos1, "0", "*", rnext, "%d" % pnext1, "0", r.row, "*" if qlen == 0 else qual])
        if o["xa_tag"]:
            line += "\tXA:i:%d" % r.polya
        if o["rg"]:
            line += "\tRG:Z:" + o["rg"]
        self.out.append(line)

    # ---- BamWriter_p.cpp:208-295 ----
    def bam_record(self, r, flags, ref, pos0, mapq, cigar, seq, quals, mate_ref, mate_pos0, tlen, tags):
        ops = cigar_ops(cigar)
        assert len(seq) <= 1000 and len(ops) <= 512   # (the product's caps: not modelled)
        name = r.name.encode("latin-1") + b"\0"
        packed = b"".join(struct.pack("<I", (n << 4) | "MIDNSHP=X".index(op)) for n, op in ops)
        codes = [BASES.index(c) if c in BASES else 15 for c in seq] + [0]
        nib = bytes((codes[i] << 4) | codes[i + 1] for i in range(0, len(seq), 2))
        phred = bytes((c - 33) & 0xFF for c in quals)
        # (uint32_t arithmetic as in :247: beyond 2^29 the bin no longer fits its 16 bits and its upper bits fall off)
        body = struct.pack("<iiIIiiii", ref, pos0, ((min_bin(pos0, pos0 + ref_span(cigar)) << 16) & 0xFFFFFFFF) | (mapq << 8) | len(name), (flags << 16) | len(ops), len(seq), mate_ref, mate_pos0,
                           tlen) + name + packed + nib + phred + tags
        self.out.append(struct.pack("<I", len(body)) + body)

    # ---- GenericReadWriter.h:190-256 with one alignment per read ----
    def single(self, r):
        if r.empty:
            return
        self.total += 1
        if not self.passes(r):
            self.write_unmapped(r, 0, -1, 0, "*", 0)
            return
        self.mapped += 1
        self.write_mapped(r, 0, "*", 0, 0, (-1, -1, 0))

    # ---- AlignmentBuffer.cpp:175-199, GenericReadWriter.h:258-304, SAMWriter.cpp:230-310, BAMWriter.cpp:404-470 ----
    def pair(self, r1, r2):
        if r1.empty or r2.empty:
            return
        h1, h2 = r1.hit, r2.hit
        if (h1.pair | h2.pair) & PAIR_LOST:   # (the project's: a pair the reference never reaches its writer with)
            return
        self.total += 2
        L1, L2 = len(r1.row), len(r2.row)
        failed = bool((h1.pair | h2.pair) & PAIR_FAILED)
        if h1.mapped and h2.mapped:
            distance = h2.pos - h1.pos + L1 if h2.pos > h1.pos else h1.pos - h2.pos + L2
            self.pairs += 1
            if h1.contig != h2.contig or distance < self.o["min_insert"] or distance > self.max_insert or bool(h1.reverse) == bool(h2.reverse):
                failed = True
                self.broken += 1
            else:
                self.insert_sum += distance
        m1, m2 = self.passes(r1), self.passes(r2)
        self.mapped += m1 + m2
        f1, f2 = 0x1 | 0x40, 0x1 | 0x80
        if not m1 and not m2:
            self.tally["none"] += 1
            self.write_unmapped(r2, f2 | 0x8, -1, 0, "*", 0)
            self.write_unmapped(r1, f1 | 0x8, -1, 0, "*", 0)
        elif not m1:
            self.tally["only2"] += 1
            self.write_mapped(r2, f2 | 0x8, "=", h2.pos + 1, 0, (h2.contig, h2.pos, 0))
            self.write_unmapped(r1, f1, h2.contig, h2.pos + 1, "=", h2.pos + 1)
        elif not m2:
            self.tally["only1"] += 1
            self.write_unmapped(r2, f2, h1.contig, h1.pos + 1, "=", h1.pos + 1)
            self.write_mapped(r1, f1 | 0x8, "=", h1.pos + 1, 0, (h1.contig, h1.pos, 0))
        elif not failed:
            f1 |= 0x2
            f2 |= 0x2
            if not h1.reverse:
                self.tally["proper_fwd"] += 1
                d = (h2.pos + L2 - h2.qstart - h2.qend) - h1.pos
                db = h2.pos + L2 - h1.pos   # BAMWriter.cpp:440
                self.write_mapped(r2, f2, "=", h1.pos + 1, -d, (h2.contig, h1.pos, -db))
                self.write_mapped(r1, f1 | 0x20, "=", h2.pos + 1, d, (h2.contig, h2.pos, db))
            elif not h2.reverse:
                self.tally["proper_rev"] += 1
                d = (h1.pos + L1 - h1.qstart - h1.qend) - h2.pos
                db = h1.pos + L1 - h2.pos
                self.write_mapped(r2, f2 | 0x20, "=", h1.pos + 1, d, (h2.contig, h1.pos, db))
                self.write_mapped(r1, f1, "=", h2.pos + 1, -d, (h2.contig, h2.pos, -db))
        else:
            self.tally["not_proper"] += 1
            self.write_mapped(r2, f2 | (0x20 if h1.reverse else 0), self.contigs[h1.contig][0], h1.pos + 1, 0, (h1.contig, h1.pos, 0))
            self.write_mapped(r1, f1 | (0x20 if h2.reverse else 0), self.contigs[h2.contig][0], h2.pos + 1, 0, (h2.contig, h2.pos, 0))


def format_batch(batch, bam=False):
    """-> (records: SAM lines without their newline, or BAM records as bytes; the seven counters of the GPU writers; the branch tally).
    Per unit the list `units` holds the records it wrote."""
    m = Model(batch.opts, batch.contigs, bam)
    recs = batch.recs
    if m.o["paired"]:
        for i in range(0, len(recs) - 1, 2):
            m.pair(recs[i], recs[i + 1])
    else:
        for r in recs:
            m.single(r)
    nbytes = sum(len(x) for x in m.out) if bam else sum(len(x.encode("latin-1")) + 1 for x in m.out)
    return m.out, [m.total, m.mapped, len(m.out), nbytes, m.pairs, m.broken, m.insert_sum], m.tally


def output_bytes(records, bam):
    return b"".join(records) if bam else "".join(l + "\n" for l in records).encode("latin-1")
