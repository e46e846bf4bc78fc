"""-m gpu: `--sort` -- the sorter object (pipeline.BamSorter over ngm_bam_sort_*, csrc/bam_sort.cpp) and `ngm-hip --bam --sort` against the
plain-Python model of tests/bam_index_model.py: the inflated members are the records in samtools' coordinate order with input order as
the tie-break, every member but the last holds 0xFF00 bytes, the members do not depend on chunk_bytes, the BAI file equals the canonical
one byte for byte, and region queries through the index return what a scan returns."""
import functools
import gzip
import os
import random
import re
import struct
import subprocess

import pytest

import bam_fixtures as BF
import bam_index_model as M
from test_gpu_bam import _case, decode_bam

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "nextgenmap_amd", "ngm-hip")
REFS = [(b"chrA", 100000), (b"chrEmpty", 5000), (b"chrB", 40000), (b"chrC", 1000000)]   # (chrEmpty never has a record)
HEADER = BF.bgzf(BF.bam_bytes([], REFS, b"@HD\tVN:1.0\tSO:coordinate\n"), eof=False)
FIRST = len(HEADER)


def _sorter(**kw):
    from nextgenmap_amd import pipeline as P
    return P.BamSorter(**kw)


def sort_with(runs, n_ref, chunk_bytes=0, order=None, max_bytes=0):
    s = _sorter(device=0, chunk_bytes=chunk_bytes, max_bytes=max_bytes)
    try:
        for seq in (order if order is not None else range(len(runs))):
            s.add(seq, runs[seq])
        s.finish(n_ref)
        members = b"".join(s.members())
        return members, s.index(FIRST), s.stats()
    finally:
        s.close()


def cut(records, n_runs, rnd):
    at = sorted(rnd.randrange(len(records) + 1) for _ in range(n_runs - 1)) if records else []
    return [b"".join(records[a:b]) for a, b in zip([0] + at, at + [len(records)])]


def check(records, runs, order=None, queries=(), n_ref=len(REFS)):
    want = M.sort_records(records)
    stream = b"".join(want)
    outs = [sort_with(runs, n_ref, cb, order) for cb in (0xFF00, 3 * 0xFF00, 0)]
    members, bai, st = outs[0]
    assert all(o[0] == members and o[1] == bai for o in outs), "the members or the index depend on chunk_bytes"
    sizes, isizes = M.member_sizes(members)
    assert (gzip.decompress(members) if members else b"") == stream
    assert all(x == 0xFF00 for x in isizes[:-1]) and len(sizes) == (len(stream) + 0xFF00 - 1) // 0xFF00
    assert bai == M.canonical_bai(want, n_ref, sizes, FIRST)
    assert (st["records"], st["record_bytes"], st["members"], st["chunks"]) == (len(records), len(stream), len(sizes), len(sizes))
    assert outs[1][2]["chunks"] == (len(sizes) + 2) // 3
    bam = HEADER + members + BF.EOF_MEMBER
    for q in queries:
        assert M.query(bam, bai, *q) == M.scan(want, *q), q
    return members, bai, want


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def _rec(rnd, ref_id, pos, flag, cigar, l_seq=None, name=None, tags=b""):
    name = name if name is not None else bytes(rnd.choice(b"abcdefghijklmnopqrstuvwxyz0123456789") for _ in range(rnd.randrange(1, 255)))
    l_seq = rnd.randrange(0, 301) if l_seq is None else l_seq
    return BF.bam_record(name, bytes(rnd.choice(b"ACGT") for _ in range(l_seq)), None, flag, cigar, ref_id=ref_id, pos=pos, tags=tags)


def _cigar(rnd, cross=0):
    ops = [(4, rnd.randrange(1, 20))] if rnd.random() < 0.3 else []
    ops += [(0, rnd.randrange(1, 120))]
    for _ in range(rnd.randrange(0, 4)):
        ops += [(rnd.choice([1, 2, 3]), rnd.randrange(1, 30)), (0, rnd.randrange(1, 80))]
    if cross:
        ops += [(3, cross), (0, 10)]
    return ops


@functools.lru_cache(maxsize=None)
def mixed():
    """about 3 000 records over chrA, chrB and chrC (none on chrEmpty), in shuffled input order; also the (reference, position) of a cluster"""
    rnd = random.Random(77)
    recs, cluster_at = [], None
    lens = {0: 100000, 2: 40000, 3: 1000000}
    for _ in range(60):   # clusters of 2 to 40 records on one (reference, position), both strands
        ref = rnd.choice([0, 2, 3])
        pos = rnd.randrange(0, lens[ref] - 2000)
        cluster_at = cluster_at or (ref, pos)
        for _ in range(rnd.randrange(2, 41)):
            recs.append(_rec(rnd, ref, pos, rnd.choice([0, 16]), _cigar(rnd)))
    for k in range(1, 6):   # across multiples of 16 384 and of 131 072
        recs.append(_rec(rnd, 0, 16384 * k - rnd.randrange(1, 50), 0, [(0, 100)]))
        recs.append(_rec(rnd, 3, 131072 * k - 20, 16, _cigar(rnd, cross=rnd.randrange(100, 40000))))
        recs.append(_rec(rnd, 3, 131072 * k - 1, 0, [(0, 1)]))
        recs.append(_rec(rnd, 3, 131072 * k, 0, [(0, 1)]))
    while len(recs) < 3000:
        x = rnd.random()
        if x < 0.05:
            recs.append(_rec(rnd, -1, -1, rnd.choice([4, 77, 141]), []))
        else:
            ref = rnd.choice([0, 2, 3])
            pos = rnd.randrange(0, lens[ref] - 2000)
            if x < 0.10:
                recs.append(_rec(rnd, ref, pos, rnd.choice([4, 20, 73]) | 4, []))      # flag 4 with a reference and a position, no CIGAR
            else:
                recs.append(_rec(rnd, ref, pos, rnd.choice([0, 16, 99, 147]), _cigar(rnd)))
    rnd.shuffle(recs)
    return tuple(recs), cluster_at


def _queries(rnd, cluster_at):
    q = [(r, 0, REFS[r][1]) for r in range(len(REFS))]                   # the whole of each reference, the empty one included
    q += [(cluster_at[0], cluster_at[1], cluster_at[1] + 1), (1, 100, 2000)]
    for _ in range(20):
        r = rnd.choice([0, 2, 3])
        b = rnd.randrange(0, REFS[r][1] - 1)
        q.append((r, b, min(REFS[r][1], b + rnd.choice([1, 100, 5000, 200000]))))
    return q


def test_empty():
    members, bai, _ = check([], [], n_ref=3)
    assert members == b""
    assert bai == b"BAI\1" + struct.pack("<i", 3) + struct.pack("<ii", 0, 0) * 3 + struct.pack("<Q", 0)


def test_single():
    rnd = random.Random(5)
    rec = _rec(rnd, 2, 1234, 16, [(0, 50)], l_seq=50)
    check([rec], [rec], queries=[(2, 0, 40000), (2, 1283, 1284), (2, 1284, 1285), (0, 0, 100000)])


def test_mixed_seven_runs_in_shuffled_seq_order():
    recs, cluster_at = mixed()
    rnd = random.Random(78)
    runs = cut(list(recs), 7, rnd)
    order = list(range(7))
    rnd.shuffle(order)
    check(list(recs), runs, order, _queries(rnd, cluster_at))


@pytest.mark.parametrize("n_runs", [1, 50])
def test_mixed_does_not_depend_on_the_runs(n_runs):
    recs, _ = mixed()
    stream = b"".join(M.sort_records(list(recs)))
    members, _, st = sort_with(cut(list(recs), n_runs, random.Random(79)), len(REFS))
    assert gzip.decompress(members) == stream and st["records"] == len(recs)


def test_long_record_spans_three_members():
    rnd = random.Random(80)
    recs = [_rec(rnd, 0, rnd.randrange(0, 90000), rnd.choice([0, 16]), _cigar(rnd), l_seq=rnd.randrange(30, 120), name=b"s%d" % i) for i in range(300)]
    long_rec = _rec(rnd, 0, 50000, 0, [(0, 90000)], l_seq=90000, name=b"long")
    assert 135000 <= len(long_rec) <= 135100
    recs.insert(150, long_rec)
    _, _, want = check(recs, cut(recs, 3, rnd), queries=[(0, 0, 100000), (0, 50000, 50001), (0, 99999, 100000), (3, 0, 1000)])
    u = sum(len(r) for r in want[:want.index(long_rec)])
    assert (u + len(long_rec) - 1) // 0xFF00 - u // 0xFF00 >= 2     # in three members: with chunk_bytes 0xFF00 a chunk boundary lies inside it


def _fast_rec(rnd, name, ref_id, pos, flag, m_len, l_seq):
    """a record without a Python loop per base (random packed bases and qualities): the large case needs some 10^5 of them"""
    body = struct.pack("<iiIIiiii", ref_id, pos, (4680 << 16) | (len(name) + 1), (flag << 16) | 1, l_seq, -1, -1, 0) + name + b"\0" + struct.pack("<I", m_len << 4) + \
        rnd.randbytes((l_seq + 1) // 2 + l_seq)
    return struct.pack("<I", len(body)) + body


def test_two_default_chunks():
    """about 36 MiB of records with the default chunk_bytes (31.9 MiB): two chunks through the two buffers, and every block of the gather
    goes round its grid-stride loop several times (the grid holds about 8 MiB), the last time with waves that have nothing left"""
    rnd = random.Random(82)
    recs = [_fast_rec(rnd, b"q%06d" % i, rnd.choice([0, 2, 3, 3]), rnd.randrange(0, 38000), rnd.choice([0, 16]), rnd.randrange(1, 200), rnd.randrange(120, 251)) for i in range(120000)]
    want = M.sort_records(recs)
    stream = b"".join(want)
    assert 34 << 20 < len(stream) < 60 << 20
    members, bai, st = sort_with(cut(recs, 5, rnd), len(REFS))
    sizes, isizes = M.member_sizes(members)
    assert gzip.decompress(members) == stream
    assert all(x == 0xFF00 for x in isizes[:-1]) and st["chunks"] == 2 and st["members"] == len(sizes)
    assert bai == M.canonical_bai(want, len(REFS), sizes, FIRST)
    bam = HEADER + members + BF.EOF_MEMBER
    for q in [(3, 20000, 20002), (2, 37999, 40000)]:
        assert M.query(bam, bai, *q) == M.scan(want, *q), q


@pytest.mark.parametrize("whole_stream", [False, True], ids=["mid-stream", "whole-stream"])
def test_record_ends_on_a_member_boundary(whole_stream):
    """tags pad a record so that it ends exactly on a member boundary; with the whole stream a multiple of 0xFF00 the last vend points at
    offset 0 of the end-of-file member"""
    rnd = random.Random(81)
    recs = [_rec(rnd, 0, 100 + 50 * i, 0, [(0, 40)], l_seq=40, name=b"b%04d" % i) for i in range(1500)]   # ascending: input order is file order
    target = 2 * 0xFF00
    if whole_stream:
        k = next(i for i in range(len(recs)) if sum(map(len, recs[:i + 1])) > target - 200)
        recs = recs[:k + 1]
    else:
        k = next(i for i in range(len(recs)) if sum(map(len, recs[:i + 1])) > target - 200)
    need = target - sum(map(len, recs[:k + 1]))
    assert need >= 4
    recs[k] = _rec(rnd, 0, 100 + 50 * k, 0, [(0, 40)], l_seq=40, name=b"b%04d" % k, tags=b"XXZ" + b"p" * (need - 4) + b"\0")
    assert sum(map(len, recs[:k + 1])) == target and (len(recs) == k + 1) == whole_stream
    shuffled = list(recs)
    rnd.shuffle(shuffled)
    members, bai, want = check(shuffled, cut(shuffled, 4, rnd), queries=[(0, 0, 100000), (0, 100 + 50 * k, 101 + 50 * k), (0, 150 + 50 * k, 151 + 50 * k)])
    assert want == recs
    if whole_stream:
        refs, _ = M.parse_bai(bai)
        assert refs[0][0][M.PSEUDO_BIN][0][1] == (FIRST + len(members)) << 16


# ---- errors: each raises with its message, the sorter destroys cleanly, and a new sorter then sorts one record ---------------------------
def _then_single():
    rec = _rec(random.Random(6), 0, 10, 0, [(0, 5)], l_seq=5)
    members, _, _ = sort_with([rec], len(REFS))
    assert gzip.decompress(members) == rec


def _err():
    from nextgenmap_amd import NgmHipError
    return NgmHipError


def _three(rnd, bad=None):
    recs = [_rec(rnd, 0, 10 * i, 0, [(0, 5)], l_seq=5) for i in range(3)]
    if bad:
        recs[1] = _rec(rnd, bad[0], bad[1], 0, [(0, 5)], l_seq=5)
    return b"".join(recs)


@pytest.mark.parametrize("bad,why", [((len(REFS), 10), "refID"), ((0, -1), "negative position")], ids=["refid-is-n_ref", "pos-minus-one"])
def test_finish_names_the_first_bad_record(bad, why):
    rnd = random.Random(90)
    s = _sorter()
    s.add(9, _three(rnd, bad))
    s.add(5, _three(rnd))
    with pytest.raises(_err(), match=r"ngm_bam_sort_finish: seq 9, record 1: .*" + why):
        s.finish(len(REFS))
    with pytest.raises(_err()):
        next(s.members())
    s.close()
    _then_single()


def test_add_refusals():
    rnd = random.Random(91)
    run = _three(rnd)
    s = _sorter()
    with pytest.raises(_err(), match=r"ngm_bam_sort_add: seq 4: record 2 .*does not end inside the run"):
        s.add(4, run[:-7])                                  # cut in mid-record
    s.add(4, run)                                           # (the refused run left nothing behind: its seq is free)
    with pytest.raises(_err(), match=r"ngm_bam_sort_add: seq 4 .*duplicate seq"):
        s.add(4, run)
    s.finish(len(REFS))
    with pytest.raises(_err(), match=r"ngm_bam_sort_add: seq 5: add after ngm_bam_sort_finish"):
        s.add(5, run)
    assert gzip.decompress(b"".join(s.members())) == run
    s.close()
    s = _sorter(max_bytes=2 * len(run) - 1)
    s.add(0, run)
    with pytest.raises(_err(), match=r"ngm_bam_sort_add: seq 1: .*max_bytes"):
        s.add(1, run)
    s.close()
    _then_single()


# ---- ngm-hip --bam --sort ------------------------------------------------------------------------------------------------------------------
def split_bam(path):
    """(file offset of the first record member, header text, dictionary, the records as bytes, the record members)"""
    raw = open(path, "rb").read()
    assert raw[-28:] == BF.EOF_MEMBER, "BGZF end-of-file block missing"
    data = gzip.decompress(raw)
    l_text, = struct.unpack_from("<i", data, 4)
    at = 8 + l_text
    n_ref, = struct.unpack_from("<i", data, at)
    at += 4
    for _ in range(n_ref):
        at += 8 + struct.unpack_from("<i", data, at)[0]
    sizes, isizes = M.member_sizes(raw[:-28])
    first, text = 0, 0
    for z, n in zip(sizes, isizes):   # the header members: whole members that hold exactly the header
        if text >= at:
            break
        first, text = first + z, text + n
    assert text == at, "the header does not end with a member"
    return first, data[8:8 + l_text].decode(), n_ref, [data[at + o:at + o + n] for o, n in M.walk(data[at:])], raw[first:-28]


def rebase(bai, first):
    """the index with the file offset of the first record member taken off every virtual offset (the pseudo-bin's counts stay)"""
    refs, n_no_coor = M.parse_bai(bai)
    off = lambda v: v - (first << 16)
    return [({b: ([(off(ch[0][0]), off(ch[0][1])), ch[1]] if b == M.PSEUDO_BIN else [(off(x), off(y)) for x, y in ch]) for b, ch in bins.items()},
             [off(v) for v in io]) for bins, io in refs], n_no_coor


def run_cli(tmp_path, tag, fa, args, env=None):
    d = tmp_path / tag
    d.mkdir()
    c = subprocess.run([CLI, "-r", fa, "-o", "out.bam", "--affine", "--bam"] + args, capture_output=True, text=True, cwd=str(d), env=dict(os.environ, **(env or {})))
    assert c.returncode == 0, c.stderr[-2000:]
    return str(d / "out.bam"), c.stderr


def check_sorted_file(path, stderr, unsorted_records=None):
    first, text, n_ref, recs, members = split_bam(path)
    assert text.startswith("@HD\tVN:1.0\tSO:coordinate\n")
    if unsorted_records is not None:
        assert recs == M.sort_records(unsorted_records)
    assert recs == M.sort_records(recs)
    sizes, isizes = M.member_sizes(members)
    assert all(x == 0xFF00 for x in isizes[:-1])
    bai = open(path + ".bai", "rb").read()
    assert bai == M.canonical_bai(recs, n_ref, sizes, first)
    m = re.search(r"\[MAIN\] Sorted on the GPU: (\d+) records \(([0-9.]+) MiB held in GPU memory\); kernels: keys [0-9.]+ ms, sort [0-9.]+ ms, gather [0-9.]+ ms, "
                  r"deflate [0-9.]+ ms, index [0-9.]+ ms; (\d+) members in (\d+) chunks, (\d+) bins", stderr)
    assert m, stderr[-1500:]
    assert int(m.group(1)) == len(recs) and int(m.group(3)) == len(sizes)
    return first, recs, members, bai


@pytest.mark.parametrize("layout,extra", [("se", []), ("pe", []), ("se", ["-n", "3"]), ("pe", ["--no-unal", "--rg-id", "x"])],
                         ids=["se", "pe", "se-top3-host-records", "pe-no-unal-rg"])
def test_cli_sorted_file_is_the_sorted_unsorted_file(tmp_path, layout, extra):
    fa, inp = _case(tmp_path, layout == "pe")
    plain, _ = run_cli(tmp_path, "plain", fa, inp + extra)
    srt, err = run_cli(tmp_path, "sorted", fa, inp + extra + ["--sort"])
    _, t0, n0, unsorted, _ = split_bam(plain)
    first, recs, members, bai = check_sorted_file(srt, err, unsorted)
    _, t1, n1, _, _ = split_bam(srt)
    strip = lambda t: [l.split("\tCL:")[0] if l.startswith("@PG") else l for l in t.splitlines()]
    assert strip(t0.replace("SO:unsorted", "SO:coordinate")) == strip(t1) and "SO:unsorted" in t0
    assert decode_bam(plain)[1] == decode_bam(srt)[1] and n0 == n1 == 2
    assert len(recs) > 1000
    bam = open(srt, "rb").read()
    for q in [(0, 0, 400000), (1, 150000, 150500), (0, 399000, 400000)]:
        assert M.query(bam, bai, *q) == M.scan(recs, *q), q


def test_cli_sorted_slam_seq(tmp_path):
    """the SLAM-seq BAM records (TC / RA / MP tags, a kernel of their own) through the sorter; linear-gap scoring, as --slam-seq needs"""
    fa, inp = _case(tmp_path, False)
    outs = []
    for tag, more in (("plain", []), ("sorted", ["--sort"])):
        d = tmp_path / tag
        d.mkdir()
        c = subprocess.run([CLI, "-r", fa, "-o", "out.bam", "--bam", "--slam-seq", "2", "--rg-id", "g", "--rg-sm", "s:t:0"] + inp + more, capture_output=True, text=True, cwd=str(d))
        assert c.returncode == 0, c.stderr[-2000:]
        outs.append((str(d / "out.bam"), c.stderr))
    unsorted = split_bam(outs[0][0])[3]
    _, recs, _, bai = check_sorted_file(outs[1][0], outs[1][1], unsorted)
    bam = open(outs[1][0], "rb").read()
    for q in [(0, 0, 400000), (1, 150000, 150500), (1, 0, 300001)]:
        assert M.query(bam, bai, *q) == M.scan(recs, *q), q


def test_cli_sorted_file_does_not_depend_on_the_route(tmp_path):
    fa, inp = _case(tmp_path, True)
    base, err = run_cli(tmp_path, "base", fa, inp + ["--sort"])
    first, recs, members, bai = check_sorted_file(base, err)
    host, err = run_cli(tmp_path, "host", fa, inp + ["--sort"], env={"NGM_HIP_BAM_HOST_RECORDS": "1"})
    assert "BAM records and their BGZF blocks written on the GPU" not in err
    assert open(host, "rb").read() == open(base, "rb").read() and open(host + ".bai", "rb").read() == bai
    for tag, more in (("w1", ["--workers", "1"]), ("w3", ["--workers", "3"]), ("b1024", ["--batch-size", "1024"])):
        path, err = run_cli(tmp_path, tag, fa, inp + ["--sort"] + more)
        f2, r2, m2, b2 = check_sorted_file(path, err)     # (its index equals the model's for its own header size)
        assert m2 == members and r2 == recs, tag          # from the first record member on: CL: differs in front of it
        assert rebase(b2, f2) == rebase(bai, first), tag  # the same index once the size of the header members is taken off
