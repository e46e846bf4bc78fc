"""-m gpu: the string builder of a default run's align stage (cigar_strings_kernel<false>, csrc/cigar_device.h: CIGAR / MD / NM / identity /
clips / the conversion rule of --bs-mapping and --slam-seq, built in LDS rows of 96 bytes and packed into one byte stream per workgroup),
through Engine.BatchAlign(device_strings=True): pack, DP + traceback, compact_runs_kernel, the string kernel -- the launch code the align stage
runs -- and the downloads.

The comparator is the CPU oracle (oracle_lib.oracle_align, pinned on the reference's computeCigarMD), never the host builder: every string, every
integer, the identity's float32 bits.  Which of the two built an alignment is compared as well, with a model made from the oracle's strings alone
(_host_built); without it a kernel that gave up on every row would pass on the host builder's work.

Inputs are rows in the pipeline's alphabet (window bytes ACGTNx and NUL, read bytes ACGTN and NUL): the kernel works on symbol classes and is
only ever fed those; lower case and IUPAC codes legitimately differ from the character-comparing host code."""
import functools
import glob
import os
import re

import numpy as np
import pytest

import oracle_lib as O
from pairgen import ACGT, make_alt_pairs, make_pairs
from test_gpu_parity import ALT_CASES

pytestmark = pytest.mark.gpu
MODES = pytest.mark.parametrize("mode", [0, 1], ids=["local", "endfree"])
ROW_LIMIT = 96 - 16   # kCigarRow - 16: bytes of a row a string may fill before its tail (the kernel's `lim`)

_WIN_OK = np.zeros(256, bool); _WIN_OK[list(b"ACGTNx\0")] = True
_READ_OK = np.zeros(256, bool); _READ_OK[list(b"ACGTN\0")] = True
_engines = {}


def _engine(q, c, **kw):
    import nextgenmap_amd as N
    key = (q, c, tuple(sorted(kw.items())))
    if key not in _engines:
        _engines[key] = N.Engine(q, c, **kw)
    return _engines[key]


def _in_alphabet(ref, qry, *more):
    keep = _WIN_OK[ref].all(axis=1) & _READ_OK[qry].all(axis=1)
    return (np.ascontiguousarray(ref[keep]), np.ascontiguousarray(qry[keep])) + tuple(np.ascontiguousarray(m[keep]) for m in more)


def _host_built(cig, md):
    """The kernel tests `co > 80 || mo > 80` at monotone checkpoints, the last one in front of the final MD number, the pending M and the
    trailing clip: an alignment is the host's exactly when the CIGAR without its trailing clip and without a final ...M element, or the MD
    without its trailing digits, is longer than 80 bytes.  (A silent clip's lead is in neither the string nor `co`.)
    Limitation: `md` is the oracle's C string, which ends at the first NUL; the kernel's `mo` goes on counting the NUL bytes of an alignment
    that runs over its window's NUL tail (at most q + c - 1 - the tail's start, a handful).  An MD within that many bytes of the limit over
    such a tail would be the host's while the model says the device's; none of the sets here has one (the comparison would say so)."""
    body = re.sub(rb"(?<=[MID])[0-9]+[SH]$", b"", cig)
    body = re.sub(rb"[0-9]+M$", b"", body)
    return len(body) > ROW_LIMIT or len(re.sub(rb"[0-9]+$", b"", md)) > ROW_LIMIT


def _expected(want, i):
    res, cig, md = want
    return (cig[i], md[i], int(res["position_offset"][i]), int(res["qstart"][i]), int(res["qend"][i]), int(res["nm"][i]),
            np.float32(res["identity"][i]).tobytes(), float(res["score_token"][i]))


def _compare(got, want, ref, qry, rows=None):
    res = want[0]
    for k, g in enumerate(got):
        i = k if rows is None else int(rows[k])
        if not res["ok"][i]:
            assert g["score_token"] == -1.0, "pair %d should be flagged invalid" % i
            continue
        have = (g["cigar"], g["md"], g["position_offset"], g["qstart"], g["qend"], g["nm"], np.float32(g["identity"]).tobytes(), float(g["score_token"]))
        assert have == _expected(want, i), "pair %d: %r != %r\nref=%r\nqry=%r" % (i, have, _expected(want, i), bytes(ref[k]), bytes(qry[k]))


def _model_built_by(want, rows=None):
    """uint8 per alignment: 1 = the device's strings.  (No alignment, score_token -1: nothing to build, the record is the device's.)"""
    res, cig, md = want
    rows = range(len(cig)) if rows is None else rows
    return np.array([0 if res["ok"][i] and _host_built(cig[i], md[i]) else 1 for i in rows], np.uint8)


def _check(eng, mode, ref, qry, want, dirs=None, rows=None, host_rows=None, capacity=0):
    """the hook on (ref, qry) against `want` (rows: their indices in it); -> (built_by, cursor).  host_rows: 0 = no row may be the host's,
    None = at least half of the ok rows are the device's"""
    got = eng.BatchAlign(mode, ref, qry, dirs, device_strings=True, capacity=capacity)
    assert len(got) == len(ref)
    _compare(got, want, ref, qry, rows)
    by = eng.last_built_by.copy()
    if capacity == 0:
        model = _model_built_by(want, rows)
        ok = want[0]["ok"] if rows is None else want[0]["ok"][np.asarray(rows)]
        bad = np.nonzero(by != model)[0]
        assert bad.size == 0, "built-by differs from the model at %s" % [(int(k), int(by[k]), int(model[k])) for k in bad[:5]]
        n_ok, n_host = int(np.count_nonzero(ok)), int(np.count_nonzero(model == 0))
        print("host-built rows: %d of %d" % (n_host, n_ok))
        if host_rows == 0:
            assert n_host == 0
        elif n_ok >= 2:
            assert 2 * (n_ok - n_host) >= n_ok
        # the stream holds exactly the device's strings.  (An alignment that runs over the NUL tail of its window has NUL bytes in its MD, in
        # the reference as here: the C string ends at the first one, the kernel's row -- at most 96 bytes -- goes on.)
        dev = [k for k in range(len(got)) if by[k] and ok[k]]
        lo = sum(len(got[k]["cigar"]) + len(got[k]["md"]) for k in dev)
        hi = lo + sum(96 - len(got[k]["md"]) for k in dev if not ref[k].all())
        assert lo <= eng.last_cursor <= hi, (lo, eng.last_cursor, hi)
    return by, eng.last_cursor


# ---- 1. parity sweep ------------------------------------------------------------------------------------------------------------------
SHAPES = [(32, 8, 28), (62, 12, 60), (152, 27, 150), (252, 42, 250)]


@functools.lru_cache(maxsize=None)
def _sweep_set(q, c, rl, mode, variant):
    ref, qry = _in_alphabet(*make_pairs(600, q, c, seed=5200 + q + c, read_len=rl))
    return ref, qry, O.oracle_align(mode, ref, qry, c, variant=variant, nthreads=8)


@pytest.mark.parametrize("q,c,rl", SHAPES)
@pytest.mark.parametrize("variant", [0, 1], ids=["oclgpu", "oclcpu"])
@MODES
def test_parity_sweep(q, c, rl, mode, variant):
    ref, qry, want = _sweep_set(q, c, rl, mode, variant)
    assert len(ref) >= 570   # the alphabet filter keeps 98-99 % of 600 rows
    _check(_engine(q, c, variant=variant), mode, ref, qry, want, host_rows=0 if mode == 0 else None)


# ---- 2. clip flags, with the custom scoring of test_custom_scoring_and_clipping ---------------------------------------------------------
CLIP_SCORING = dict(match=7, mismatch=-11, gap_read=-13, gap_ref=-17)


@pytest.mark.parametrize("clip", [0, 1, 2], ids=["soft", "hardclip", "silentclip"])
@MODES
def test_clip_flags(clip, mode):
    q, c = 152, 27
    hard, silent = int(clip == 1), int(clip == 2)
    ref, qry = _in_alphabet(*make_pairs(600, q, c, seed=5377, read_len=150))
    want = O.oracle_align(mode, ref, qry, c, CLIP_SCORING, hard_clip=hard, silent_clip=silent, nthreads=8)
    if mode == 0:   # the flags carry weight: clipped alignments, labelled as the flag says
        clipped = [x for i, x in enumerate(want[1]) if want[0]["ok"][i] and (want[0]["qstart"][i] > 0 or want[0]["qend"][i] > 0)]
        assert len(clipped) > 50
        assert all((b"H" in x) == bool(hard) and (b"S" in x) == (not hard and not silent) for x in clipped)
    _check(_engine(q, c, match=7, mismatch=11, gap_read=13, gap_ref=17, hard_clip=hard, silent_clip=silent), mode, ref, qry, want)


# ---- 3. conversion modes: --bs-mapping / --slam-seq with the pairs' direction bytes ----------------------------------------------------
@pytest.mark.parametrize("kind", sorted(ALT_CASES))
@pytest.mark.parametrize("q,c,rl", [(152, 27, 150), (52, 11, 50)])
@pytest.mark.parametrize("variant", [0, 1], ids=["oclgpu", "oclcpu"])
@MODES
def test_conversion_modes(kind, q, c, rl, variant, mode):
    scoring, eng_kw = ALT_CASES[kind]
    ref, qry, dirs = _in_alphabet(*make_alt_pairs(600, q, c, seed=5400 + q + c, read_len=rl, alt=scoring["alt"]))
    want = O.oracle_align(mode, ref, qry, c, scoring, variant=variant, nthreads=8, dirs=dirs)
    # the direction must matter (else the case proves nothing)
    flip = O.oracle_align(mode, ref, qry, c, scoring, variant=variant, nthreads=8, dirs=1 - dirs)
    both = want[0]["ok"] & flip[0]["ok"]
    assert np.any((want[0]["nm"] != flip[0]["nm"])[both] | (want[0]["identity"] != flip[0]["identity"])[both])
    _check(_engine(q, c, variant=variant, **eng_kw), mode, ref, qry, want, dirs=dirs)


# ---- 4. indel-rich pairs: strings at the row limit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("q,c,rl", [(152, 27, 150), (252, 42, 250)])
@MODES
def test_indel_rich_pairs(q, c, rl, mode):
    ref, qry = _in_alphabet(*make_pairs(600, q, c, seed=5500 + q, read_len=rl, sub_rate=0.08, indel_rate=0.03, mix=(0.9, .05, .05)))
    want = O.oracle_align(mode, ref, qry, c, nthreads=8)
    by, _ = _check(_engine(q, c), mode, ref, qry, want)
    if (q, mode) != (152, 0):
        assert np.count_nonzero(by == 0) > 0   # these do reach the limit
    near = [i for i in range(len(ref)) if want[0]["ok"][i] and by[i] and max(len(want[1][i]), len(want[2][i])) > ROW_LIMIT - 12]
    assert near, "no device-built string within 12 bytes of the limit"


# ---- 5. constructed pairs at (152, 27): the window's main diagonal starts at column 13 --------------------------------------------------
Q, CW = 152, 27
GAPPY = dict(match=10, mismatch=30, gap_read=2, gap_ref=2)   # an insertion next to a deletion beats mismatches


def _sub(b):
    return ACGT[(int(np.searchsorted(ACGT, b)) + 1) % 4]


def _every_indel(rng, win, s, step, total):
    """`step` window bases, then in turn one base inserted / one window base skipped, up to `total` read bases"""
    parts, at, ins = [], s, True
    while sum(len(p) for p in parts) < total:
        parts.append(win[at:at + step]); at += step
        if ins: parts.append(ACGT[rng.integers(0, 4, 1)])
        else: at += 1
        ins = not ins
    return np.concatenate(parts)[:total]


def _constructed():
    rng = np.random.default_rng(5600)
    rnd = lambda k: ACGT[rng.integers(0, 4, k)]
    s = CW // 2
    rl = Q + CW

    def plain(w): return w[s:s + 150].copy()

    def nn_run(w):
        w[s + 40:s + 46] = ord("N")
        return w[s:s + 150].copy()

    def all_n_window(w):
        r = w[s:s + 150].copy()
        w[:] = ord("N")
        return r

    def x_tail(w):
        r = w[s:s + 150].copy()
        w[150] = ord("x"); w[151:] = 0
        return r

    def deletion(d):
        def build(w):
            # a run of A is skipped; no A within 16 bases on either side (with per-base gap costs a deleted base that finds a partner splits the gap)
            cgt = ACGT[1:]
            w[s + 54:s + 70] = cgt[rng.integers(0, 3, 16)]
            w[s + 70:s + 70 + d] = ord("A")
            w[s + 70 + d:s + 86 + d] = cgt[rng.integers(0, 3, 16)]
            return np.concatenate([w[s:s + 70], w[s + 70 + d:s + 150 + d]])
        return build

    def ins_del(w): return np.concatenate([w[s:s + 60], rnd(4), w[s + 65:s + 151]])

    def first_last(w):
        r = w[s:s + 150].copy(); r[0] = _sub(r[0]); r[149] = _sub(r[149])
        return r

    def adjacent(w):
        r = w[s:s + 150].copy()
        for k in (50, 51, 52): r[k] = _sub(r[k])
        return r

    def every_2nd(w):
        w[:] = ACGT[:2][rng.integers(0, 2, rl)]   # a window of A and C under a read whose every second base is G: no other diagonal does better
        r = w[s:s + 150].copy()
        r[1::2] = ord("G")
        return r

    cases = [("plain", plain), ("nn_run", nn_run), ("all_n_window", all_n_window), ("x_tail", x_tail), ("del1", deletion(1)), ("del9", deletion(9)),
             ("del10", deletion(10)), ("del13", deletion(13)), ("ins_del", ins_del), ("first_last", first_last), ("adjacent", adjacent),
             ("short1", lambda w: w[s:s + 1].copy()), ("short5", lambda w: w[s:s + 5].copy()), ("empty", lambda w: np.zeros(0, np.uint8)),
             ("every_2nd", every_2nd), ("indel_every_9", lambda w: _every_indel(rng, w, s, 9, 150)), ("indel_every_5", lambda w: _every_indel(rng, w, s, 5, 150))]
    ref, qry = np.zeros((len(cases), rl), np.uint8), np.zeros((len(cases), Q), np.uint8)
    for k, (_, build) in enumerate(cases):
        win = ACGT[rng.integers(0, 4, rl)].copy()
        read = np.asarray(build(win), np.uint8)[:Q - 1]
        ref[k] = win
        qry[k, :len(read)] = read
    return [n for n, _ in cases], ref, qry


@pytest.mark.parametrize("scoring", ["default", "gappy"])
@MODES
def test_constructed_pairs(mode, scoring):
    names, ref, qry = _constructed()
    kw = GAPPY if scoring == "gappy" else {}
    sc = dict(match=kw["match"], mismatch=-kw["mismatch"], gap_read=-kw["gap_read"], gap_ref=-kw["gap_ref"]) if kw else None
    want = O.oracle_align(mode, ref, qry, CW, sc, nthreads=8)
    res, cig, md = want
    by_name = {n: (cig[k], md[k], bool(res["ok"][k])) for k, n in enumerate(names)}
    # the cases are what they claim to be (the oracle's strings)
    if scoring == "gappy":
        # (an insertion and a deletion side by side score the same in either order: which one comes first is the traceback's choice)
        assert re.search(rb"M[0-9]+(I[0-9]+D|D[0-9]+I)", by_name["ins_del"][0]), by_name["ins_del"]
        if mode == 1:
            # with gaps this cheap a mismatch column becomes 1I1D: against the all-N window one pair per base, more runs than window columns.
            # (The run scratch held q + c + 8 runs per pair and the traceback dropped the rest: this row came back valid with NM 217 for 274.)
            c_, m_, ok_ = by_name["all_n_window"]
            assert ok_ and len(re.findall(rb"[0-9]+[MID]", c_)) > Q + CW + 8 and res["nm"][names.index("all_n_window")] == 274, c_
    else:
        assert by_name["plain"][:2] == (b"150M", b"150")
        c_, m_, _ = by_name["nn_run"]
        assert c_ == b"150M" and m_ == b"150", (c_, m_)          # N in the read over N in the window: a match column
        assert not by_name["empty"][2]
        assert not by_name["short1"][2] and by_name["short5"][0] == b"5M", (by_name["short1"], by_name["short5"])   # (one base: the oracle builds no alignment)
        for d in (1, 9, 10, 13):
            c_, m_, _ = by_name["del%d" % d]
            assert c_ == b"70M%dD80M" % d and m_ == b"70^" + b"A" * d + b"80", (d, c_, m_)
        c_, m_, _ = by_name["indel_every_9"]
        assert c_.count(b"I") + c_.count(b"D") >= 12, c_
        c_, m_, _ = by_name["indel_every_5"]
        assert len(c_) > ROW_LIMIT and _host_built(c_, m_), c_    # the CIGAR passes 80 bytes
        c_, m_, _ = by_name["adjacent"]
        assert c_ == b"150M" and re.fullmatch(rb"50[ACGT]{3}97", m_), (c_, m_)   # (computeCigarMD puts no 0 between neighbouring mismatches)
        c_, m_, _ = by_name["ins_del"]
        assert c_ == b"60M1D90M" and m_.startswith(b"60^") and m_.endswith(b"86"), (c_, m_)   # (at 10 / 15 / 20 four mismatches beat the insertion: see "gappy")
        if mode == 1:
            c_, m_, _ = by_name["x_tail"]
            assert c_ == b"150M" and m_.startswith(b"137x"), (c_, m_)   # the read ends over the window's x / NUL tail (the MD's C string ends at the NUL)
            c_, m_, _ = by_name["first_last"]
            assert c_ == b"150M" and re.fullmatch(rb"0[ACGT]148[ACGT]0", m_), (c_, m_)
            c_, m_, _ = by_name["every_2nd"]
            assert c_ == b"150M" and len(m_) > ROW_LIMIT and _host_built(c_, m_), (c_, m_)   # the MD passes 80 bytes under a CIGAR of 4
            c_, m_, ok_ = by_name["all_n_window"]
            assert ok_ and c_ == b"150M" and set(re.sub(rb"[0-9]", b"", m_)) <= set(b"N"), (c_, m_)
        else:   # local alignments end where the score stops growing: the same pairs are clipped, or have no alignment at all
            assert by_name["x_tail"][:2] == (b"137M13S", b"137"), by_name["x_tail"]
            assert by_name["first_last"][:2] == (b"1S148M1S", b"148"), by_name["first_last"]
            assert not by_name["every_2nd"][2] and not by_name["all_n_window"][2], (by_name["every_2nd"], by_name["all_n_window"])
    eng = _engine(Q, CW, **kw)
    _check(eng, mode, ref, qry, want)


# ---- 6. batch sizes: ragged waves and workgroups, a workgroup that asks for no bytes ------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _count_set(mode):
    ref, qry = _in_alphabet(*make_pairs(640, Q, CW, seed=5700, read_len=150))
    ref, qry = ref[:600].copy(), qry[:600].copy()
    qry[256:512] = 0   # empty reads: no alignment, no bytes -- the whole second workgroup
    want = O.oracle_align(mode, ref, qry, CW, nthreads=8)
    assert len(ref) == 600 and not want[0]["ok"][256:512].any()
    return ref, qry, want


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 600])
@MODES
def test_batch_sizes(n, mode):
    ref, qry, want = _count_set(mode)
    _check(_engine(Q, CW), mode, ref[:n], qry[:n], want, rows=np.arange(n), host_rows=0 if mode == 0 else None)


# ---- 8. a full stream: the workgroups that find no room leave their alignments to the host ------------------------------------------------
@MODES
def test_stream_full(mode):
    ref, qry, want = _sweep_set(152, 27, 150, mode, 0)
    eng = _engine(152, 27, variant=0)
    by_full, cursor = _check(eng, mode, ref, qry, want, host_rows=0 if mode == 0 else None)
    capacity = cursor // 3
    assert capacity > 0
    by, cursor_small = _check(eng, mode, ref, qry, want, capacity=capacity)   # (still the oracle's results)
    assert cursor_small == cursor
    ok = want[0]["ok"]
    dev = np.nonzero((by == 1) & ok)[0]
    assert 0 < dev.size < np.count_nonzero((by_full == 1) & ok)
    assert not np.any((by == 1) & (by_full == 0))
    # the device-built rows' cig_len + md_len fit the stream: the C strings' lengths bound that sum from below (an MD over a window's NUL tail
    # ends at the first NUL, the kernel's row goes on -- see _check), and the rows without a NUL in their window give it exactly
    lo = sum(len(want[1][i]) + len(want[2][i]) for i in dev)
    assert lo <= capacity
    if all(ref[i].all() for i in dev):
        print("device-built bytes %d of capacity %d (exact)" % (lo, capacity))


# ---- 9. the reference's own computeCigarMD output -----------------------------------------------------------------------------------------
CIGAR_GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "ngm_ocl_*_cigar.npz")))


@pytest.mark.parametrize("path", CIGAR_GOLDEN, ids=[os.path.basename(p) for p in CIGAR_GOLDEN])
@pytest.mark.parametrize("clip", [0, 1, 2], ids=["soft", "hardclip", "silentclip"])
@MODES
def test_reference_cigar_goldens(path, mode, clip):
    from test_oracle_golden import cigar_golden_rows
    g = np.load(path.replace("_cigar.npz", ".npz"))
    ref, qry, c, variant = g["ref"], g["qry"], int(g["c"]), int(g["variant"])
    rows, want = cigar_golden_rows(path, mode, clip)
    _, dirs, kw = O.golden_case(g)
    keep = np.nonzero(_WIN_OK[ref].all(axis=1) & _READ_OK[qry].all(axis=1))[0]
    at = {int(i): k for k, i in enumerate(keep)}
    eng = _engine(qry.shape[1], c, variant=variant, hard_clip=int(clip == 1), silent_clip=int(clip == 2), **kw)
    got = eng.BatchAlign(mode, np.ascontiguousarray(ref[keep]), np.ascontiguousarray(qry[keep]), None if dirs is None else np.ascontiguousarray(dirs[keep]), device_strings=True)
    n_dev = n_seen = 0
    for j, i in enumerate(rows):
        if int(i) not in at:
            continue
        a = got[at[int(i)]]
        have = (True, a["cigar"], a["md"], a["nm"], np.float32(a["identity"]).tobytes(), a["qstart"], a["qend"], a["position_offset"], float(a["score_token"]))
        assert have == want[j], "row %d: %r != %r" % (i, have, want[j])
        by = int(eng.last_built_by[at[int(i)]])
        assert by == (0 if _host_built(want[j][1], want[j][2]) else 1), (i, by, want[j][1], want[j][2])
        n_seen += 1
        n_dev += by
    assert n_seen >= 0.9 * len(rows) and 2 * n_dev >= n_seen
