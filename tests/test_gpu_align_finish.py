"""-m gpu: the align stage's finishing kernel of the affine personality (affine_finish_kernel, csrc/cigar_device.h: trace matrix ->
CIGAR / NM / identity / clips in one launch, trace words prefetched eight rows at a time) and the thread / wave split of
expand_pairs_kernel (csrc/gather_device.h).

The comparator is the CPU oracle (oracle_lib.oracle_affine, as in tests/test_gpu_affine.py::_check), not the old kernels: CIGAR, position
offset, QStart, QEnd, NM, the identity's bits and MD.  Engine.BatchAlign(finish=True) runs explicit (window, read) pairs through
DP + finishing kernel and reports how many alignments that kernel left to the old traceback and the host (`last_fallback`).
Both alignment modes run: local takes the packed DP's 4-bit trace, end-to-end the 32-bit DP's trace bytes and end-cell flags."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import simulate as S
from pairgen import ACGT, make_pairs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "nextgenmap_amd", "ngm-hip")
MODES = pytest.mark.parametrize("mode", [0, 1], ids=["local", "endfree"])
_engines = {}


def _engine(q, c):
    import nextgenmap_amd as N
    from nextgenmap_amd import engine as E
    if (q, c) not in _engines:
        _engines[(q, c)] = N.Engine(q, c, personality=E.PERSONALITY_AFFINE, gap_read=33, gap_ref=33, gap_extend=3)
    return _engines[(q, c)]


def _compare(al, want, ref, qry, rows=None):
    sc, res, cig = want
    for k, a in enumerate(al):
        i = k if rows is None else rows[k]
        exp = (cig[i], int(res["position_offset"][i]), int(res["qstart"][i]), int(res["qend"][i]), int(res["nm"][i]))
        have = (a["cigar"], a["position_offset"], a["qstart"], a["qend"], a["nm"])
        assert have == exp, (i, have, exp, bytes(ref[k]), bytes(qry[k]))
        wi, hi = np.float32(res["identity"][i]), np.float32(a["identity"])
        assert wi.view(np.uint32) == hi.view(np.uint32) or (np.isnan(wi) and np.isnan(hi)), (i, wi, hi)
        assert a["md"] == b"!!!"  # EndToEndAffine leaves pBuffer2 alone


def _beyond_the_row(cigars):
    """how many of these CIGARs the device must leave to the host: leading clip + runs (everything but a trailing clip) beyond 96 - 16 bytes"""
    return sum(len(re.sub(rb"(?<=[MID])[0-9]+S$", b"", x) if not re.fullmatch(rb"[0-9]+S", x) else b"") > 96 - 16 for x in cigars)


def _check(q, c, mode, ref, qry):
    """-> (oracle cigars, alignments the finishing kernel left to the host); that number is the oracle's, too"""
    eng = _engine(q, c)
    want = O.oracle_affine(mode, ref, qry, c, nthreads=8)
    al = eng.BatchAlign(mode, ref, qry, finish=True)
    _compare(al, want, ref, qry)
    assert eng.last_fallback == _beyond_the_row(want[2])
    return want[2], eng.last_fallback


# ---- pair counts: a wave with and without its second block, a ragged last block; four / two / two trace words per row ----------------
@functools.lru_cache(maxsize=None)
def _count_set(q, c, mode):
    ref, qry = make_pairs(300, q, c, seed=7100 + q + c, read_len=q - 2, indel_rate=0.01)
    return ref, qry, O.oracle_affine(mode, ref, qry, c, nthreads=8)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 128, 129, 300])
@pytest.mark.parametrize("q,c", [(152, 27), (32, 8), (62, 12)])
@MODES
def test_pair_counts(q, c, n, mode):
    ref, qry, want = _count_set(q, c, mode)
    eng = _engine(q, c)
    al = eng.BatchAlign(mode, ref[:n], qry[:n], finish=True)
    assert len(al) == n
    _compare(al, want, ref[:n], qry[:n])
    assert eng.last_fallback == _beyond_the_row(want[2][:n])


# ---- indel-rich pairs (the shape of test_affine_indel_rich_pairs): read lengths 150, 40, and both within one block -------------------
@pytest.mark.parametrize("shape", ["150", "40", "mixed"])
@MODES
def test_indel_rich_pairs(shape, mode):
    q, c = 152, 27
    kw = dict(sub_rate=0.05, indel_rate=0.03, mix=(0.9, 0.05, 0.05))
    if shape == "mixed":
        ra, qa = make_pairs(800, q, c, seed=191, read_len=150, **kw)
        rb, qb = make_pairs(800, q, c, seed=192, read_len=40, **kw)
        pick = np.random.default_rng(193).random(800)[:, None] < 0.5   # rows of both lengths inside every block of 64
        ref, qry = np.where(pick, ra, rb), np.where(pick, qa, qb)
    else:
        ref, qry = make_pairs(800, q, c, seed=190 + int(shape), read_len=int(shape), **kw)
    _check(q, c, mode, ref, qry)


# ---- constructed pairs at (152, 27): the window's main diagonal is band column 13 ----------------------------------------------------
Q, CW = 152, 27


def _pair(rng, build):
    """build(win) -> read bytes; -> (window row, read row)"""
    win = ACGT[rng.integers(0, 4, Q + CW)].copy()
    read = np.asarray(build(win), dtype=np.uint8)[:Q - 1]
    row = np.zeros(Q, np.uint8)
    row[:len(read)] = read
    return win, row


def _constructed():
    rng = np.random.default_rng(4242)
    rnd = lambda k: ACGT[rng.integers(0, 4, k)]
    s = CW // 2   # 13
    cases = [
        # two deletions, 3 and 11 reference bases: the path crosses band columns 15 -> 16 and 23 -> 24 (and ends in the last column, 27)
        ("del3_del11", lambda w: np.concatenate([w[s:s + 50], w[s + 53:s + 103], w[s + 114:s + 164]])),
        # insertion of 6: columns 13 -> 7 (8 -> 7 changes the trace word)
        ("ins6", lambda w: np.concatenate([w[s:s + 70], rnd(6), w[s + 70:s + 144]])),
        # insertion of 13: down to column 0
        ("ins13", lambda w: np.concatenate([w[s:s + 70], rnd(13), w[s + 70:s + 137]])),
        # 6 then 7 inserted bases: 13 -> 7 -> 0
        ("ins6_ins7", lambda w: np.concatenate([w[s:s + 45], rnd(6), w[s + 45:s + 95], rnd(7), w[s + 95:s + 137]])),
        # an indel inside the first 8 and inside the last 8 rows of the read
        ("del_first_rows", lambda w: np.concatenate([w[s:s + 6], w[s + 7:s + 151]])),
        ("ins_first_rows", lambda w: np.concatenate([w[s:s + 6], rnd(1), w[s + 6:s + 149]])),
        ("del_last_rows", lambda w: np.concatenate([w[s:s + 144], w[s + 145:s + 151]])),
        ("ins_last_rows", lambda w: np.concatenate([w[s:s + 144], rnd(1), w[s + 144:s + 149]])),
        # fewer than 8 bases
        ("short5", lambda w: w[s + 20:s + 25]),
        ("short1", lambda w: w[s + 3:s + 4]),
        # soft-clipped at both ends (local mode): unrelated flanks
        ("clipped", lambda w: np.concatenate([np.full(12, ord("N"), np.uint8), w[s + 12:s + 130], np.full(14, ord("N"), np.uint8)])),
        # matches nowhere: score 0, empty alignment
        ("nowhere", lambda w: np.full(150, ord("N"), np.uint8)),
        ("empty", lambda w: np.zeros(0, np.uint8)),
        # a plain full-length read
        ("plain", lambda w: w[s:s + 150]),
    ]
    rows = [_pair(rng, b) for _, b in cases]
    return [n for n, _ in cases], np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


@MODES
def test_constructed_pairs(mode):
    names, ref, qry = _constructed()
    cig, fb = _check(Q, CW, mode, ref, qry)
    assert fb == 0
    if mode == 0:   # the cases are what they claim to be (the oracle's strings)
        by = dict(zip(names, cig))
        assert b"3D" in by["del3_del11"] and b"11D" in by["del3_del11"], by["del3_del11"]
        assert b"6I" in by["ins6"] and b"13I" in by["ins13"], (by["ins6"], by["ins13"])
        assert b"6I" in by["ins6_ins7"] and b"7I" in by["ins6_ins7"], by["ins6_ins7"]
        assert b"1D" in by["del_first_rows"] and b"1D" in by["del_last_rows"], (by["del_first_rows"], by["del_last_rows"])
        assert b"1I" in by["ins_first_rows"] and b"1I" in by["ins_last_rows"], (by["ins_first_rows"], by["ins_last_rows"])
        assert by["clipped"].count(b"S") == 2, by["clipped"]
        assert by["nowhere"] == b"150S", by["nowhere"]
        assert by["short1"] == b"1M" and by["short5"].endswith(b"4M") and by["plain"] == b"150M", (by["short1"], by["short5"], by["plain"])


# ---- a CIGAR beyond the device's row: counted, served by the old traceback + the host, still the oracle's string ----------------------
@MODES
def test_cigar_beyond_the_row_goes_to_the_host(mode):
    q, c = 252, 42
    rng = np.random.default_rng(77)
    s = c // 2
    refs, qrys = [], []
    for k in range(3):
        win = ACGT[rng.integers(0, 4, q + c)].copy()
        parts, at, ins = [], s, True
        while sum(len(p) for p in parts) < 250:
            parts.append(win[at:at + 9]); at += 9
            if ins: parts.append(ACGT[rng.integers(0, 4, 1)])   # one base inserted ...
            else: at += 1                                         # ... the next time one deleted: every 9 bases a 1-base indel
            ins = not ins
        read = np.concatenate(parts)[:250]
        row = np.zeros(q, np.uint8); row[:len(read)] = read
        refs.append(win); qrys.append(row)
    plain = make_pairs(70, q, c, seed=78, read_len=250)   # ... among pairs whose strings the device builds
    ref, qry = np.concatenate([plain[0][:40], np.stack(refs), plain[0][40:]]), np.concatenate([plain[1][:40], np.stack(qrys), plain[1][40:]])
    cig, fb = _check(q, c, mode, ref, qry)
    assert all(len(x) > 96 - 16 for x in cig[40:43]), cig[40:43]
    assert fb >= 3   # non-zero, and (in _check) exactly the oracle's number


# ---- expand_pairs: a thread per read up to 8 candidates, a wave per read above ------------------------------------------------------
def test_expand_pairs_matches_numpy_repeat():
    from nextgenmap_amd import engine as E
    lib = E.load_library()
    lib.ngm_debug_expand_pairs.restype = C.c_int
    lib.ngm_debug_expand_pairs.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    kinds = np.array([0, 1, 8, 9, 64, 65, 5000], np.uint32)
    rng = np.random.default_rng(5)
    count = kinds[rng.integers(0, 6, 700)]          # three workgroups of reads, the last one ragged
    count[:7] = kinds                               # every count, 5 000 included, in the first one
    count[300], count[699] = 5000, 5000
    base = np.concatenate([[0], np.cumsum(count[:-1], dtype=np.uint64)]).astype(np.uint32)
    n_cand = int(count.sum(dtype=np.uint64))
    out = np.zeros(n_cand, np.uint32)
    rc = lib.ngm_debug_expand_pairs(0, len(count), base.ctypes.data, count.ctypes.data, n_cand, out.ctypes.data)
    assert rc == 0
    assert np.array_equal(out, np.repeat(np.arange(len(count), dtype=np.uint32), count))


# ---- pipeline: the one-kernel tail, the three-kernel tail and the host's strings are one result --------------------------------------
def test_align_tail_variants_give_identical_sam(tmp_path):
    """In the pattern of test_kernel_variants_give_identical_sam: a small repeat-rich genome, 2 000 pairs of 150 bp with indels,
    --affine, batches of 1 338 reads (no multiple of 128)."""
    from nextgenmap_amd import build
    build.build()
    contigs = S.make_genome([400_000, 250_001], seed=811, repeat_families=20, repeat_len=600, copies=10, divergence=0.01)
    fa = str(tmp_path / "ref.fa")
    with open(fa, "wb") as f:
        for i, g in enumerate(contigs):
            f.write(b">chr%d\n" % (i + 1))
            b = g.tobytes()
            for o in range(0, len(b), 60):
                f.write(b[o:o + 60] + b"\n")
    r1, r2 = S.make_reads(contigs, 2000, 150, seed=812, sub_rate=0.015, indel_rate=0.01, paired=True)
    f1, f2 = str(tmp_path / "pe_1.fq"), str(tmp_path / "pe_2.fq")
    S.write_fastq(f1, r1)
    S.write_fastq(f2, r2)

    def run(tag, env):
        out = str(tmp_path / (tag + ".sam"))
        e = dict(os.environ)
        e.pop("NGM_HIP_ALIGN_TAIL_SPLIT", None)
        e.pop("NGM_HIP_HOST_CIGAR", None)
        e.update(env)
        c = subprocess.run([CLI, "-r", fa, "-o", out, "-1", f1, "-2", f2, "--affine", "--batch-size", "1338"], capture_output=True, text=True, env=e)
        assert c.returncode == 0, c.stderr[-2000:]
        return [l for l in open(out, "rb") if not l.startswith(b"@PG")]
    base = run("base", {})
    assert len(base) > 4000
    assert sum(1 for l in base if not l.startswith(b"@") and (b"I" in l.split(b"\t")[5] or b"D" in l.split(b"\t")[5])) > 100
    for tag, env in (("split", {"NGM_HIP_ALIGN_TAIL_SPLIT": "1"}), ("hostcigar", {"NGM_HIP_HOST_CIGAR": "1"})):
        other = run(tag, env)
        assert other == base, "%s: %d of %d lines differ" % (tag, sum(a != b for a, b in zip(other, base)), len(base))
