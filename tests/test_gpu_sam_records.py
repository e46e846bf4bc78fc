"""The GPU record writers (sam_lengths_kernel / sam_write_kernel, csrc/sam_device.h) on constructed results, through ngm_debug_sam_records --
the launch sequence ngm_mapper_map_sam runs -- against the hand-typed expectations of tests/sam_cases.py and the plain model of the reference's
writers (tests/sam_model.py; tests/test_sam_model.py pins that model without a GPU).  Every comparison is byte-exact on the text or the
records and exact on the counters."""
import random
import struct

import numpy as np
import pytest

import sam_cases as SC
import sam_model as SM
from nextgenmap_amd import pipeline as P
from test_host_units import reg2bin

pytestmark = pytest.mark.gpu


def marshal(batch, bam):
    """a Batch as the arguments of pipeline.debug_sam_records"""
    o = dict(SM.Model(batch.opts, batch.contigs, bam).o, silent=batch.opts.get("silent", 0))
    n, q = len(batch.recs), batch.q
    reads, quals = np.zeros((n, q), np.uint8), np.zeros((n, q), np.uint8)
    meta, hits = np.zeros(n, P.SAM_READ_DTYPE), np.zeros(n, P.HIT_DTYPE)
    names, cigars, mds = [], [], []
    off = 0
    for i, r in enumerate(batch.recs):
        assert len(r.row) <= q and min(r.qual_len, q - 1) <= len(r.qual) <= q
        reads[i, :len(r.row)] = np.frombuffer(r.row.encode("latin-1"), np.uint8)
        quals[i, :len(r.qual)] = np.frombuffer(r.qual.encode("latin-1"), np.uint8)
        name = r.name.encode("latin-1")
        meta[i] = (off, len(name), (r.qual_len & 0x7FFF) | (0x8000 if r.empty else 0))
        names.append(name)
        off += len(name)
        h = r.hit
        hits[i] = (h.mapped, h.contig, h.pos, h.reverse, h.mapq, h.score, h.identity, h.nm, h.qstart, h.qend, h.n_cand, h.n_best, h.votes, h.pair)
        cigars.append(h.cigar.encode())
        mds.append(h.md.encode())
    so = P.SamOptions(o["paired"], o["min_insert"], o["max_insert"], o["min_mq"], o["min_identity"], o["min_residues"], o["no_unal"], o["rg"].encode() if o["rg"] else None,
                      o["bs_mapping"], o["slam_seq"], int(bam))
    return dict(options=so, reads=reads, quals=quals, names=b"".join(names), meta=meta, hits=hits, cigars=cigars, mds=mds, contig_names=[c[0] for c in batch.contigs],
                contig_lens=[c[1] for c in batch.contigs], polya=np.array([r.polya for r in batch.recs], np.uint16) if o["xa_tag"] else None,
                hard_clip=int(o["clip"] and not o["silent"]), silent_clip=int(o["clip"] and o["silent"]), variant=o["variant"], alt_scoring=o["alt_scoring"])


def gpu_output(batch, bam, reference=None):
    return P.debug_sam_records(reference=reference, **marshal(batch, bam))


def assert_equals_model(batch, bam, reference=None):
    """-> the GPU's output and counters, after comparing both with the model's"""
    out, counters, _ = SM.format_batch(batch, bam)
    want = SM.output_bytes(out, bam)
    got, got_counters = gpu_output(batch, bam, reference)
    if got != want:
        at = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))
        raise AssertionError("%d / %d bytes, first difference at %d: GPU %r, model %r" % (len(got), len(want), at, got[max(0, at - 100):at + 40], want[max(0, at - 100):at + 40]))
    assert got_counters == counters
    return got, got_counters


@pytest.fixture(scope="module")
def typed_reference():
    ref = P.Reference.from_contigs([np.frombuffer(c[2].encode(), np.uint8) for c in SC.CONTIGS], names=[c[0] for c in SC.CONTIGS])
    yield ref
    ref.close()


@pytest.mark.parametrize("run", SC.ALL_RUNS, ids=lambda r: r.name)
def test_hand_typed_cases(run, typed_reference):
    slam = run.batch.opts.get("slam_seq", 0)
    got, counters = gpu_output(run.batch, run.bam, typed_reference if slam else None)
    assert counters[3] == len(got)
    run.check(SC.decode_records(got) if run.bam else got.decode("latin-1").split("\n")[:-1], counters[:3] + counters[4:])
    assert_equals_model(run.batch, run.bam, typed_reference if slam else None)


def test_identity_sweep_text_bits_and_the_filter_boundary():
    """every identity k / 10000 and the float next to every rounding boundary (k + 0.5) / 10000: XI:f as "%g" prints it, the float's bits in
    BAM, and min_identity = 0.9 crossed in float"""
    ids = [x for k in range(10001) for x in (np.float32(k / 10000.0), np.float32((k + 0.5) / 10000.0))]
    assert len(ids) == 20002
    recs = [SC.rec("r%d" % i, "ACGTACGTAC", "IIIIIIIIII", SC.hit(identity=x)) for i, x in enumerate(ids)]
    batch = SC.Batch({"min_identity": 0.9}, recs)
    passing = sum(1 for x in ids if x >= np.float32(0.9))
    assert 0 < passing < len(ids) and np.float32(0.9) in ids
    got, counters = assert_equals_model(batch, False)
    assert counters[:3] == [len(ids), passing, len(ids)]
    lines = got.decode().split("\n")[:-1]
    xi = [l.split("\t")[14] for l in lines if l.split("\t")[1] == "0"]
    assert xi == ["XI:f:" + SM.xi_text(x) for x in ids if x >= np.float32(0.9)]
    got, counters = assert_equals_model(batch, True)
    bits = [r["tags"][21:28] for r in SC.decode_records(got) if r["flag"] == 0]
    assert bits == [b"XIf" + struct.pack("<f", SM.identity_rounded(x)) for x in ids if x >= np.float32(0.9)]


@pytest.mark.parametrize("bam", [False, True], ids=["sam", "bam"])
@pytest.mark.parametrize("paired", [0, 1], ids=["se", "pe"])
@pytest.mark.parametrize("units", [0, 1, 2, 255, 256, 257, 513])
def test_block_tails(units, paired, bam):
    """around the 256-thread blocks, the prefix sums' units + 1 elements, no unit at all"""
    batch = SC.random_batch(7000 + units, units, paired, q=40)
    got, counters = assert_equals_model(batch, bam)
    if units == 0:
        assert got == b"" and counters == [0] * 7


def row_shape_batch(q, clip):
    """reads of every length 0 .. q - 1, through the kinds of quality string (none, shorter than the read, as long, longer, longer than the
    row), discarded reads, names of 1 and 254 bytes, both strands, unmapped"""
    rng = random.Random(q)
    recs = []
    for L in range(q):
        row = "".join(rng.choice("ACGTN") for _ in range(L))
        qual_len = [0, max(L - 1 - L // 3, 0), L, L + 1 + L % 5, q + L % 7][(L // 2) % 5]
        qual = "".join(rng.choice("!#5?IJ~") for _ in range(min(qual_len, q - 1)))
        name = "n" if L % 11 == 0 else "N" * 254 if L % 11 == 1 else "read%d" % L
        if L == 0 or L % 4 == 3:
            h = SC.hit(mapped=0, cigar="", md="")
        else:
            qs, qe = (L // 5, L // 7) if L % 3 == 0 else (0, 0)
            mark = {"none": "S", "hard": "H", "silent": ""}[clip]
            cigar = ("%d%s" % (qs, mark) if qs and mark else "") + "%dM" % (L - qs - qe) + ("%d%s" % (qe, mark) if qe and mark else "")
            h = SC.hit(reverse=L % 2, pos=1000 + L, qstart=qs, qend=qe, cigar=cigar, md="%d" % (L - qs - qe))
        recs.append(SC.rec(name, row, qual, h, qual_len=qual_len, seq_len=0 if L % 13 == 5 else max(L, 1)))
    return SC.Batch(dict(clip=int(clip != "none"), silent=int(clip == "silent"), min_residues=0.0), recs, q=q)


@pytest.mark.parametrize("bam", [False, True], ids=["sam", "bam"])
@pytest.mark.parametrize("clip", ["none", "hard"])
@pytest.mark.parametrize("q", [12, 152, 1001])
def test_row_shapes(q, clip, bam):
    batch = row_shape_batch(q, clip)
    lens = set(r.qual_len for r in batch.recs)
    assert 0 in lens and any(r.qual_len > q - 1 for r in batch.recs) and any(r.empty for r in batch.recs) and any(len(r.row) % 2 for r in batch.recs if r.hit.mapped)
    assert any(0 < r.qual_len < len(r.row) for r in batch.recs) and any(len(r.row) < r.qual_len <= q - 1 for r in batch.recs) and len(batch.recs[0].row) == 0
    assert_equals_model(batch, bam)
    paired = SC.Batch(dict(batch.opts, paired=1), batch.recs[:q - q % 2], q=q)   # (neighbouring lengths as mates)
    assert_equals_model(paired, bam)


def test_bam_bins_around_every_level_boundary():
    """a contig of 2^27 + 2^15 bases, without a sequence: alignments that begin and end one base on either side of multiples of 2^14, 2^17,
    2^20, 2^23 and 2^26, and their unmapped mates placed at the same position.  Expected: reg2bin of the SAM specification (section 5.3) over
    [pos, pos + reference span), and over [pos, pos) for the record without an alignment, as BamWriter_p.cpp:218 calls it"""
    contigs = [("big", (1 << 27) + (1 << 15), None)]
    recs, want = [], []
    for shift in (14, 17, 20, 23, 26):
        for mult in (1, 2, 3, 5, 11, 77, 1023):   # (beyond the first bin of the next level too: there a level's shift decides the bin)
            b = mult << shift
            if b + 200 > contigs[0][1]:
                continue
            for pos, span in ((b - 1, 1), (b - 1, 2), (b, 1), (b + 1, 1), (b - 100, 99), (b - 100, 100), (b - 100, 101), (b - 50, 100), (b, 100)):
                mapped = SC.hit(pos=pos, cigar="%dM" % span, md="%d" % span)
                mates = [SC.rec("p%d/1" % len(recs), "A" * 110, "", mapped), SC.rec("p%d/2" % len(recs), "C" * 20, "", SC.hit(mapped=0, cigar="", md=""))]
                recs += mates if len(want) % 4 else mates[::-1]   # (either mate)
                want += [(pos, reg2bin(pos, pos)), (pos, reg2bin(pos, pos + span))] if len(want) % 4 else [(pos, reg2bin(pos, pos + span)), (pos, reg2bin(pos, pos))]
    batch = SC.Batch({"paired": 1, "min_residues": 0.0}, recs, contigs=contigs, q=128)
    got, _ = assert_equals_model(batch, True)
    assert [(r["pos"], r["bin"]) for r in SC.decode_records(got)] == want
    bins = set(b for _, b in want)
    assert 0 in bins and all(any(lo <= b < hi for b in bins) for lo, hi in ((1, 9), (9, 73), (73, 585), (585, 4681), (4681, 37449)))   # every level


# ---- SLAM-seq tags on a packed genome ------------------------------------------------------------------------------------------------------

def slam_genome():
    rng = random.Random(99)
    contigs = []
    for name, length in (("one", 3002), ("two", 2503), ("three", 4099)):
        s = [rng.choice("ACGT") for _ in range(length)]
        s[500:540] = "N" * 40                                   # an N run
        s[900:1100] = [c.lower() for c in s[900:1100]]           # lower case
        s[1500] = "R"                                            # an IUPAC letter: N in the packed genome
        contigs.append((name, length, "".join(s)))
    return contigs


@pytest.fixture(scope="module")
def slam_reference():
    contigs = slam_genome()
    ref = P.Reference.from_contigs([np.frombuffer(c[2].encode(), np.uint8) for c in contigs], names=[c[0] for c in contigs])
    table = ref.contigs
    assert [(n, l) for n, s, l in table] == [(c[0], c[1]) for c in contigs]
    assert table[1][1] % 8 != 0 and table[2][1] % 8 != 0, table   # the second and third contig start inside a dword of the packed genome
    yield ref, contigs
    ref.close()


def slam_batch(contigs, variant, alt_scoring, seed):
    rng = random.Random(seed)
    recs = []
    for i in range(240):
        c = i % 3
        name, length, bases = contigs[c]
        # the alignment: M runs with a few substitutions, N and lower case in the read, I and D between them
        pos = rng.choice([0, 480, 880, 1480, length - 200, rng.randrange(0, length - 200)])
        at, read, ops = pos, [], []
        for k in range(rng.randint(1, 5)):
            m = rng.randint(1, 30)
            seg = bases[at:at + m].upper()
            read += [ch if rng.random() < 0.85 else rng.choice("ACGTNacgt") for ch in seg]
            ops.append("%dM" % m)
            at += m
            if rng.random() < 0.5:
                ins = rng.randint(1, 3)
                read += [rng.choice("ACGT") for _ in range(ins)]
                ops.append("%dI" % ins)
            elif rng.random() < 0.5:
                d = rng.randint(1, 4)
                ops.append("%dD" % d)
                at += d
        if ops[-1][-1] == "D":
            at -= int(ops.pop()[:-1])
        assert at <= length
        qs, qe = rng.choice([0, 0, 3, 11]), rng.choice([0, 0, 2, 7])
        oriented = "".join([rng.choice("ACGT") for _ in range(qs)] + read + [rng.choice("ACGT") for _ in range(qe)])
        reverse = rng.randint(0, 1)
        row = SM.revcomp(oriented) if reverse else oriented
        cigar = ("%dS" % qs if qs else "") + "".join(ops) + ("%dS" % qe if qe else "")
        recs.append(SC.rec("s%d" % i, row, "", SC.hit(contig=c, pos=pos, reverse=reverse, qstart=qs, qend=qe, cigar=cigar, md="%d" % len(read), nm=i % 7)))
    return SC.Batch(dict(slam_seq=1, variant=variant, alt_scoring=alt_scoring, min_residues=0.0, min_identity=0.0), recs, contigs=contigs, q=200)


@pytest.mark.parametrize("bam", [False, True], ids=["sam", "bam"])
@pytest.mark.parametrize("alt_scoring", [0, 1])
@pytest.mark.parametrize("variant", [0, 1])
def test_slam_seq_tags_on_a_packed_genome(slam_reference, variant, alt_scoring, bam):
    """TC / RA / MP from the packed genome: contigs that start inside a dword, N runs, lower case and IUPAC letters in the reference, both
    strands, insertions, deletions, clipped starts, N and lower case in the reads -- and in BAM the block_size set behind the tags"""
    ref, contigs = slam_reference
    batch = slam_batch(contigs, variant, alt_scoring, 31)
    assert any(r.hit.reverse and r.hit.qstart and "I" in r.hit.cigar and "D" in r.hit.cigar for r in batch.recs)
    got, _ = assert_equals_model(batch, bam, ref)
    if bam:
        recs = SC.decode_records(got)   # (walks the records by their block_size)
        assert len(recs) == len(batch.recs) and sum(1 for r in recs if b"MPZ" in r["tags"]) > 100
    else:
        assert got.count(b"\tMP:Z:") > 100 and got.count(b"\tTC:i:") == len(batch.recs)


@pytest.mark.parametrize("bam", [False, True], ids=["sam", "bam"])
@pytest.mark.parametrize("i", range(len(SC.RANDOM_CONFIGS)), ids=[SC.random_config_id(c) for c in SC.RANDOM_CONFIGS])
def test_random_batches(i, bam):
    """the batches whose coverage of the writers' branches tests/test_sam_model.py asserts"""
    assert_equals_model(SC.random_config_batch(i), bam)


# ---- what the entry refuses ----------------------------------------------------------------------------------------------------------------

def _valid(slam=0):
    return SC.Batch({"slam_seq": slam}, [SC.rec("ok", "ACGTACGTAC", "IIIIIIIIII", SC.hit(pos=2)), SC.rec("other", "ACGTACGTAC", "", SC.hit(pos=5, reverse=1, qstart=2, cigar="2S8M"))])


def _args(batch, reference=None):
    return dict(marshal(batch, False), reference=reference)


def _bad_name_end(a): a["meta"]["name_len"][1] += 1
def _bad_name_long(a): a["names"] = b"x" * 300; a["meta"]["name_off"][0] = 0; a["meta"]["name_len"][0] = 255
def _bad_contig(a): a["hits"]["contig"][1] = 2
def _bad_contig_negative(a): a["hits"]["contig"][0] = -1
def _bad_qstart(a): a["hits"]["qstart"][0] = -1
def _bad_qend(a): a["hits"]["qend"][0] = -1
def _bad_clip_sum(a): a["hits"]["qstart"][0] = 6; a["hits"]["qend"][0] = 5
def _bad_cigar_bases(a): a["cigars"][1] = b"2S9M"
def _bad_cigar_text(a): a["cigars"][0] = b"10Q"
def _slam_no_reference(a): a["reference"] = None
def _slam_other_table(a): a["contig_lens"][1] += 1
def _slam_beyond_contig(a): a["hits"]["pos"][0] = SC.CONTIGS[0][1] - 9


@pytest.mark.parametrize("spoil,slam", [(_bad_name_end, 0), (_bad_name_long, 0), (_bad_contig, 0), (_bad_contig_negative, 0), (_bad_qstart, 0), (_bad_qend, 0), (_bad_clip_sum, 0),
                                        (_bad_cigar_bases, 0), (_bad_cigar_text, 0), (_slam_no_reference, 1), (_slam_other_table, 1), (_slam_beyond_contig, 1)],
                         ids=lambda v: v.__name__.strip("_") if callable(v) else "")
def test_entry_refuses_what_the_kernels_would_index_with(spoil, slam, typed_reference):
    """each validation rule: -22 for one violating input, nothing launched, and the next valid call is correct"""
    batch = _valid(slam)
    args = _args(batch, typed_reference if slam else None)
    spoil(args)
    with pytest.raises(P.NgmHipError) as e:
        P.debug_sam_records(**args)
    assert e.value.code == -22 and "ngm_debug_sam_records" in str(e.value)
    assert_equals_model(batch, False, typed_reference if slam else None)
