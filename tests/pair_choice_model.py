"""Plain models of the paired-end selection, no GPU: what pair_simple_kernel (csrc/gather_device.h) and pair_choice_kernel
(csrc/pair_device.h) have to compute, and the pairs tests/test_pair_choice_model.py and tests/test_gpu_pair_choice.py feed them.

(a) literal_walk / literal: ScoreBuffer::top1PE as written (src/ScoreBuffer.cpp:368-416, :463-502) for one order of the candidates and
    one running mean insert size: a stable sort by descending score, computeMQ, the prefix at or above Scores[0] * cutoff (float32), the
    i / j double loop over CheckPairs.  The loop itself is tests/test_pair_walk.py's (expected_walk, check_pairs_loop, mapq).
(b) contract: the order-free description in the header of pair_device.h, from sets: per mate the best score, how many candidates share
    it, the second best, the candidates at or above best * cutoff; over those the in-window combinations; from them found / tied / dup /
    host, the MAPQs, the best-scoring combinations and the range of their insert sizes.
    `host`: a side with more than 65 535 candidates, or more than 8 192 of them above the cut-off, or a best score that several
    candidates share while !(best * cutoff <= best) -- a negative best score with a cut-off below 1: the reference then pairs only
    Scores[0], "the first" of them.  (With a cut-off of exactly 1 best * cutoff == best, the prefix holds every candidate that shares a
    negative best score, and nothing depends on the order: not `host`.)

All arithmetic on scores is numpy float32, as in the reference and in the kernels."""
import math

import numpy as np

from test_pair_walk import check_pairs_loop, expected_walk, mapq

INT_MAX = 2 ** 31 - 1
COMBOS, TOPS, CAP_LARGE, CAP_HUGE, SPLIT = 64, 8, 2048, 8192, 64   # kPairCombos, PairTop's rows, kPairCap, kPairCapHuge, the list split
LITERAL_LIMIT = 20000   # in-window combinations beyond which the literal loop is not run (Python's speed)


# ---------------------------------------------------------------------------------------------------------------------------------
# a batch of pairs as the score stage holds it
class Batch:
    """reads 2p (mate b) and 2p + 1 (mate a) are pair p; read r owns candidates [base[r], base[r] + count[r]) of scores / loc"""

    def __init__(self, name, min_d, max_insert, cutoff, pairs, rng):
        self.name, self.min_d, self.max_insert, self.cutoff, self.tags = name, int(min_d), int(max_insert), float(cutoff), [p["tag"] for p in pairs]
        self.max_d = self.max_insert if self.max_insert > 0 else INT_MAX
        self.n_pairs = len(pairs)
        n = 2 * self.n_pairs
        self.count = np.zeros(n, np.uint32)
        self.base = np.zeros(n, np.uint32)
        self.read_len = np.zeros(n, np.uint16)
        lists = []
        for p, pr in enumerate(pairs):
            for r, s, l, ln in ((2 * p, pr["sb"], pr["lb"], pr["len_b"]), (2 * p + 1, pr["sa"], pr["la"], pr["len_a"])):
                assert len(s) == len(l)
                self.count[r] = len(s)
                self.read_len[r] = ln
                lists.append((np.asarray(s, np.float32), np.asarray(l, np.int64)))
        # storage order differs from read order (nothing requires monotone bases)
        chunks_s, chunks_l, at = [], [], 0
        for r in rng.permutation(n):
            self.base[r] = at
            chunks_s.append(lists[r][0]); chunks_l.append(lists[r][1])
            at += len(lists[r][0])
        self.scores = np.ascontiguousarray(np.concatenate(chunks_s), np.float32)
        loc = np.concatenate(chunks_l)
        assert loc.min() >= 0 and loc.max() < 2 ** 32
        self.loc = np.ascontiguousarray(loc.astype(np.uint32))
        self.n_cand = at

    def mate(self, p, side):   # side 0: mate a (the odd read), 1: mate b
        r = 2 * p + 1 - side
        return int(self.base[r]), int(self.count[r]), int(self.read_len[r])


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) the literal model
def literal_walk(bt, p, order_a=None, order_b=None):
    """the in-window combinations of pair p in the double loop's order when the candidates arrive in the given orders (permutations of
    range(count); None: as stored): (pair scores, insert sizes, candidates of a, of b -- absolute indices), MAPQ of a, MAPQ of b"""
    lists = []
    for side, order in ((0, order_a), (1, order_b)):
        b, c, _ = bt.mate(p, side)
        v = b + (np.arange(c) if order is None else np.asarray(order, np.int64))
        lists.append(v[np.argsort(-bt.scores[v], kind="stable")])   # std::sort by score; which order equal scores keep is what `order` varies
    A, B = lists
    ps, d, a, b = expected_walk(A, B, bt.mate(p, 0)[2], bt.mate(p, 1)[2], bt.loc, bt.scores, bt.cutoff, bt.min_d, bt.max_insert)
    return (ps, d, a, b), mapq(A, bt.scores), mapq(B, bt.scores)


def literal(bt, p, order_a=None, order_b=None, avg=0):
    """(found, wa, wb, equal, dist, mq_a, mq_b) of top1PE for one candidate order and one running mean"""
    (ps, d, a, b), mq_a, mq_b = literal_walk(bt, p, order_a, order_b)
    return tuple(check_pairs_loop(ps, d, a, b, avg)) + (mq_a, mq_b)


# ---------------------------------------------------------------------------------------------------------------------------------
# (b) the contract model
class Contract:
    __slots__ = ("cls", "host", "huge", "found", "tied", "dup", "mq_a", "mq_b", "n_combo", "n_top", "tops", "dmin", "dmax", "n_above", "edges")
    # cls: "empty" (a mate without candidates), "simple" (1 x 1), "small" / "large" (the two lists)


def _side(bt, p, side):
    b, c, _ = bt.mate(p, side)
    s = bt.scores[b:b + c]
    best = s.max()
    n_best = int(np.count_nonzero(s == best))
    rest = s[s != best]
    second = best if n_best > 1 else (rest.max() if len(rest) else np.float32(0))
    mq = 60
    if c > 1:
        mq = 0
        if best > 0 and second >= 0:
            mq = int(math.ceil(np.float32(np.float32(60.0) * (best - second)) / best))
    mn = np.float32(best) * np.float32(bt.cutoff)
    head_only = not (mn <= best)
    sel = np.nonzero(s == best if head_only else s >= mn)[0]
    return b + sel, mq, c > 65535 or (head_only and n_best > 1)


def contract(bt, p):
    out = Contract()
    ca, cb = bt.mate(p, 0)[1], bt.mate(p, 1)[1]
    out.host = out.huge = out.found = out.tied = out.dup = False
    out.mq_a = out.mq_b = out.n_combo = out.n_top = out.dmin = out.dmax = 0
    out.tops, out.n_above, out.edges = set(), (0, 0), set()
    if ca == 0 or cb == 0:
        out.cls = "empty"
        return out
    out.cls = "simple" if ca == 1 and cb == 1 else ("small" if ca <= SPLIT and cb <= SPLIT else "large")
    ia, out.mq_a, host_a = _side(bt, p, 0)
    ib, out.mq_b, host_b = _side(bt, p, 1)
    out.n_above = (len(ia), len(ib))
    most = max(len(ia), len(ib))
    if out.cls == "simple":
        host_a = host_b = False
    elif host_a or host_b:
        out.host = True
    else:
        out.huge = out.cls == "large" and most > CAP_LARGE
        out.host = most > (CAP_HUGE if out.cls == "large" else SPLIT)   # (a small pair has at most 64 candidates on a side)
    if out.host:
        return out
    la, lb = bt.loc[ia].astype(np.int64)[:, None], bt.loc[ib].astype(np.int64)[None, :]
    cur = np.where(lb > la, lb - la + bt.mate(p, 1)[2], la - lb + bt.mate(p, 0)[2])
    raw = cur
    cur = (cur + 2 ** 31) % 2 ** 32 - 2 ** 31   # the reference's `int`
    # (for the generator's self-check: the edges of the insert size this pair's combinations sit on)
    out.edges = {name for name, v in (("min", bt.min_d), ("min+1", bt.min_d + 1), ("max-1", bt.max_d - 1), ("max", bt.max_d)) if np.any(cur == v)}
    out.edges |= ({"wrap"} if np.any(raw != cur) else set()) | ({"wrap into the window"} if np.any((raw != cur) & (cur > bt.min_d) & (cur < bt.max_d)) else set())
    out.edges |= {"same location"} if np.any(la == lb) else set()
    ii, jj = np.nonzero((cur > bt.min_d) & (cur < bt.max_d))
    ps = (bt.scores[ia][ii] + bt.scores[ib][jj]).astype(np.float32)
    d = cur[ii, jj]
    out.n_combo = len(ps)
    out.found = bool(np.any(ps > 0))
    if out.n_combo > COMBOS:
        out.tied = out.dup = True
        out.dmin, out.dmax = bt.min_d, bt.max_d
        return out
    combos = [(float(ps[x]), int(d[x]), int(ia[ii[x]]), int(ib[jj[x]])) for x in range(out.n_combo)]
    out.tied = len({c[0] for c in combos}) < len(combos)
    out.dup = len({c[:2] for c in combos}) < len(combos)
    if out.found:
        top = max(c[0] for c in combos)
        tops = [c for c in combos if c[0] == top]
        out.n_top = len(tops)
        out.tops = {c[1:] for c in tops}
        out.dmin, out.dmax = min(c[1] for c in tops), max(c[1] for c in tops)
    if out.n_top > TOPS:
        out.dup = True
    if not out.tied:
        out.dup = False
        assert out.n_top <= 1
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the pairs.  Every case names the edge it is there for (tag); the models above decide what each pair is.
LEN_A, LEN_B = 150, 140
FAR_A, FAR_B, STEP = 3_000_000_000, 3_500_000_000, 5000   # candidates nobody pairs with (where an upper window bound exists)


def _pair(sa, la, sb, lb, tag, len_a=LEN_A, len_b=LEN_B):
    return {"sa": list(sa), "la": [int(x) for x in la], "sb": list(sb), "lb": [int(x) for x in lb], "tag": tag, "len_a": len_a, "len_b": len_b}


def _lb_for(l1, d, up, len_a=LEN_A, len_b=LEN_B):
    """the location of a candidate of mate b at insert size d from a candidate of a at l1, after it (l2 > l1) or not"""
    return l1 + d - len_b if up else l1 - (d - len_a)


def insert_size(l1, l2, len_a, len_b):
    """CheckPairs' currentInsertsize (src/ScoreBuffer.cpp:467-473) as the `int` it is stored in"""
    cur = l2 - l1 + len_b if l2 > l1 else l1 - l2 + len_a
    return (cur + 2 ** 31) % 2 ** 32 - 2 ** 31


def _at_size(rng, d, up, len_a, len_b):
    """locations of a candidate of a and one of b at insert size d exactly, b after a (l2 > l1) or not; a size below the read length
    is reached through the 32-bit wrap"""
    assert len_a >= 1 and len_b >= 1
    delta = d - len_b if up else d - len_a
    if delta >= (1 if up else 0):
        l1 = int(rng.integers(10_000_000, 2_000_000_000))
        l2 = l1 + delta if up else l1 - delta
    else:
        assert delta < 0, (d, up, len_a, len_b)   # (b after a by 0 bases does not exist: choose a shorter read)
        lo = int(rng.integers(0, -delta))
        l1, l2 = (lo, lo + 2 ** 32 + delta) if up else (lo + 2 ** 32 + delta, lo)
    assert 0 <= l1 < 2 ** 32 and 0 <= l2 < 2 ** 32 and (l2 > l1) == up and insert_size(l1, l2, len_a, len_b) == d, (d, up, len_a, len_b, l1, l2)
    return l1, l2


def cluster_pair(rng, ca, cb, ka, kb, kind, cfg, tag, above_a=None, above_b=None, origin=None, spread=200, gap=None):
    """ca x cb candidates; the first above_a / above_b of them score at or above the cut-off, the first ka / kb of those lie in one
    cluster -- every combination of them inside the window --, all others far from everything.
    kind: "distinct" (pair scores of the cluster all different while ka * kb <= 140), "ties" (a handful of scores), "equal",
    "nonpos" (nothing positive), "none" (cluster moved out of the window: no combination)"""
    above_a, above_b = ca if above_a is None else above_a, cb if above_b is None else above_b
    assert ka <= above_a <= ca and kb <= above_b <= cb
    origin = int(rng.integers(10_000_000, 2_000_000_000)) if origin is None else origin

    def scores(c, above, k, step):
        if kind == "equal":
            hi = np.full(above, 1350.0)
        elif kind == "ties":
            hi = rng.choice([1400.0, 1390.0, 1385.0], above)
        elif kind == "nonpos":
            hi = np.zeros(above)   # best 0, shared: every candidate at or above 0 * cutoff is kept
        else:
            hi = rng.integers(1300, 1441, above).astype(np.float64)
            hi[:k] = 1300.0 + step * np.arange(k)
        lo = rng.integers(200, 601, c - above).astype(np.float64)   # below 0.5 * 1300
        if kind == "nonpos":
            lo = -rng.integers(1, 50, c - above).astype(np.float64)
        return np.concatenate([hi, lo])

    sa, sb = scores(ca, above_a, ka, max(kb, 1) if ka * kb <= 140 else 1), scores(cb, above_b, kb, 1)
    gap = cfg["min_d"] + 100 if gap is None else gap   # insert sizes of the cluster: min + 40 .. min + 440 (or len_a .. when b comes first)
    shift = gap if kind != "none" else cfg["max_d"] + 5000
    la = np.concatenate([origin + rng.choice(spread, ka, replace=ka > spread), FAR_A + STEP * np.arange(ca - ka) + rng.integers(0, 1000)])
    lb = np.concatenate([origin + shift + rng.choice(spread, kb, replace=kb > spread), FAR_B + STEP * np.arange(cb - kb) + rng.integers(0, 1000)])
    return _pair(sa, la, sb, lb, tag)


def special_pairs(rng, cfg):
    """the hand-made edges, for one window / cut-off"""
    mn, mx, cut = cfg["min_d"], cfg["max_d"], np.float32(cfg["cutoff"])
    L = lambda: int(rng.integers(10_000_000, 2_000_000_000))
    out = []
    add = out.append
    mid = mn + 250
    # ---- window bounds, strictly: d = min, min + 1, max - 1, max; mate b after mate a and not after it; 1 x 1, 2 x 1, 1 x 2.  The lower
    # bound needs reads shorter than min (an insert size is a distance plus a read length); with min = 0 the sizes 0 and 1 come from the
    # 32-bit wrap (and 1 from two mates of length 1 at one location, below)
    bounds = [(mn, "min"), (mn + 1, "min+1")] + ([(mx - 1, "max-1"), (mx, "max")] if mx < INT_MAX else [])   # (no upper bound: unlimited_pairs)
    for d, name in bounds:
        len_a, len_b = (LEN_A, LEN_B) if name.startswith("max") else ((d // 2, d // 3) if mn >= 4 else (40, 50))
        for up in (True, False):
            l1, l2 = _at_size(rng, d, up, len_a, len_b)
            far = l2 ^ 0x80000000   # 2^31 from l2, and so out of every bounded window around l1
            add(_pair([1400], [l1], [1390], [l2], "bound 1x1 d=%s" % name, len_a, len_b))
            add(_pair([1400, 1399], [l1, l1 ^ 0x80000000], [1390], [l2], "bound 2x1 d=%s" % name, len_a, len_b))
            add(_pair([1400], [l1], [1390, 1389], [l2, far], "bound 1x2 d=%s" % name, len_a, len_b))
    l1 = L()
    add(_pair([1400], [l1], [1390], [l1], "same location, length 1: d=1", 1, 1))
    add(_pair([1400, 1399], [l1, l1 ^ 0x80000000], [1390], [l1], "same location 2x1, length 1: d=1", 1, 1))
    l1 = L()
    add(_pair([1400], [l1], [1390], [l1], "same location 1x1"))            # l2 == l1: the `else` branch, d = len_a
    add(_pair([1400, 1399], [l1, l1 + 7], [1390], [l1], "same location 2x1"))
    add(_pair([1400, 1399], [l1, l1 + 7], [1390], [l1 + 3], "len_a != len_b, both branches", len_a=97, len_b=201))
    # ---- both ends of the 32-bit range: the difference wraps in the `int`
    add(_pair([1400], [0xFFFFFF00], [1390], [50], "32-bit ends 1x1, a high"))
    add(_pair([1400], [5], [1390], [0xFFFFFFF0], "32-bit ends 1x1, b high: wraps to a small positive size"))
    add(_pair([1400, 1399], [5, 0xFFFFFF00], [1390, 1388], [0xFFFFFFF0, 50], "32-bit ends 2x2"))
    add(_pair([1400, 1399], [0xFFFFFFFF, 0], [1390], [0xFFFFFFFF - 200], "32-bit ends 2x1"))
    # ---- a mate without candidates, whatever the other has
    for ca, cb in ((0, 0), (0, 1), (1, 0), (0, 70), (70, 0), (0, 3)):
        l1 = L()
        add(_pair(rng.integers(1300, 1400, ca), l1 + np.arange(ca), rng.integers(1300, 1400, cb), l1 + 300 + np.arange(cb), "empty mate %dx%d" % (ca, cb)))
    # ---- 1 x 1: found, out of the window, pair score zero and negative
    for sa, sb, d in ((1400, 1390, mid), (1400, 1390, min(mx, 2 ** 30) + 700), (5, -5, mid), (3, -5, mid), (-3, 5, mid), (0, 0, mid), (0, 1, mid)):
        l1 = L()
        add(_pair([sa], [l1], [sb], [_lb_for(l1, d, True)], "1x1 scores %d %d" % (sa, sb)))
    # ---- numbers of best-scoring combinations: 1, 2, 8, 9 (distinct insert sizes: tied, the mean decides; 9: too many to list)
    for k in (1, 2, 3, 8, 9):
        l1 = L()
        offs = rng.choice(150, k, replace=False)
        add(_pair([1400] * k + [1300], list(l1 + offs) + [l1 + 160], [1390], [l1 + 300], "%d top combinations" % k))
        add(_pair([1390], [l1], [1400] * k + [1300], list(l1 + 300 + offs) + [l1 + 460], "%d top combinations, on b" % k))
    # ---- ties among the non-top combinations only, without and with a shared insert size
    l1 = L()
    add(_pair([1400, 1350, 1350], [l1, l1 + 10, l1 + 20], [1400], [l1 + 300], "tie below the top, sizes differ"))
    add(_pair([1400, 1350, 1350], [l1, l1 + 10, l1 + 10], [1400], [l1 + 300], "tie below the top, size shared"))
    add(_pair([1400, 1350], [l1, l1 + 10], [1400, 1350], [l1 + 300, l1 + 310], "2x2: the middle combinations tie, sizes differ"))
    add(_pair([1400, 1400], [l1, l1 + 10], [1400, 1400], [l1 + 300, l1 + 310], "2x2: all equal, two share the size"))
    add(_pair([1400, 1400], [l1, l1], [1390], [l1 + 300], "top combinations share score and size"))
    # ---- all pair scores equal
    for k in (2, 3):
        l1 = L()
        add(_pair([1350] * k, l1 + rng.choice(100, k, replace=False), [1350] * k, l1 + 300 + 100 * np.arange(k), "all pair scores equal %dx%d" % (k, k)))
    # ---- nothing positive; a zero next to positive ones; zero twice
    l1 = L()
    add(_pair([-5, -6], [l1, l1 + 5], [-7], [l1 + 300], "negative best not shared: pair score negative"))
    add(_pair([-5, -9], [l1, l1 + 5], [100], [l1 + 300], "negative best not shared: pair found"))
    add(_pair([-5, -5], [l1, l1 + 5], [100], [l1 + 300], "negative best shared (host while cutoff < 1)"))
    add(_pair([100], [l1], [-5, -5, -6], [l1 + 300, l1 + 305, l1 + 310], "negative best shared on b (host while cutoff < 1)"))
    add(_pair([0, -3], [l1, l1 + 5], [10], [l1 + 300], "best 0"))
    add(_pair([0, 0], [l1, l1 + 5], [0], [l1 + 300], "best 0 shared: pair scores 0 twice, sizes differ"))
    add(_pair([0, 0], [l1, l1], [0, 0], [l1 + 300, l1 + 300], "pair scores 0 with equal sizes"))
    add(_pair([50, 48, 47], [l1, l1 + 5, l1 + 9], [-48], [l1 + 300], "pair scores 2, 0, -1"))
    add(_pair([50, 50, 48], [l1, l1 + 5, l1 + 9], [-50], [l1 + 300], "pair scores 0, 0, -2: nothing positive, tied"))
    add(_pair([5, 5], [l1, l1 + 5], [-5, -4.75], [l1 + 300, l1 + 301], "pair scores 0 and 0.25"))
    # ---- the positive top inside the window for only one of two otherwise equal combinations
    add(_pair([1400, 1400], [l1, FAR_A], [1400], [l1 + 300], "one of two equal combinations in the window"))
    add(_pair([1400, 1400], [l1, l1 + (min(mx, 2 ** 30) + 300)], [1400], [l1 + 300], "one of two equal combinations in the window (just outside)"))
    # ---- the cut-off, exactly: a candidate at float32(best * float32(cutoff)) and one ulp below it
    for best in (1400.0, 1333.0, 77.0, 3.0):
        at = np.float32(best) * cut
        below = np.nextafter(at, np.float32(-np.inf), dtype=np.float32)
        l1 = L()
        add(_pair([best, at, below], [l1, l1 + 5, l1 + 9], [best], [l1 + 300], "at the cut-off and one ulp below, best %g" % best))
        add(_pair([best], [l1], [below, at, best], [l1 + 300, l1 + 305, l1 + 309], "at the cut-off and one ulp below on b, best %g" % best))
    return out


def count_edge_pairs(rng, cfg):
    """numbers of candidates per mate around the list split (64) and the strides of four waves (256); numbers of in-window combinations
    0, 1, 63, 64, 65"""
    out = []
    for ca, cb in ((1, 2), (2, 1), (2, 2), (63, 1), (64, 1), (65, 1), (1, 63), (1, 64), (1, 65), (63, 63), (64, 64), (65, 65), (64, 65), (65, 64), (63, 65),
                   (256, 1), (257, 2), (300, 3), (1, 256), (2, 257), (3, 300), (256, 257), (300, 300)):
        for kind in ("distinct", "ties", "equal", "none"):
            ka, kb = min(ca, 8), min(cb, 8)
            if kind == "distinct":
                ka, kb = (min(ca, 63), 1) if ca >= cb else (1, min(cb, 63))
            out.append(cluster_pair(rng, ca, cb, ka, kb, kind, cfg, "counts %dx%d %s" % (ca, cb, kind)))
        out.append(cluster_pair(rng, ca, cb, ca if ca <= 70 else 1, cb if cb <= 70 else 1, "distinct", cfg, "counts %dx%d all near" % (ca, cb)))
    for ka, kb in ((0, 1), (1, 1), (63, 1), (9, 7), (64, 1), (8, 8), (65, 1), (13, 5), (1, 63), (1, 64), (1, 65), (5, 13)):
        for kind in ("distinct", "ties", "equal"):
            ca, cb = max(ka, 1) + int(rng.integers(0, 4)), kb + int(rng.integers(0, 4))
            out.append(cluster_pair(rng, ca, cb, ka, kb, kind, cfg, "combinations %dx%d %s" % (ka, kb, kind), above_a=max(ka, 1), above_b=kb))
    return out


def cap_edge_pairs(rng, cfg, with_host=True):
    """numbers of candidates above the cut-off around the caps of the second launch (2 048) and of the third (8 192), and the pairs only
    the host can take"""
    out = []
    for n in (2047, 2048, 2049):
        for kind in ("distinct", "ties", "none"):
            other = 1 + int(rng.integers(0, 3))
            out.append(cluster_pair(rng, n + 5, other, 2, 1, kind, cfg, "cap %d on a, %s" % (n, kind), above_a=n, above_b=other))
            out.append(cluster_pair(rng, other, n + 5, 1, 2, kind, cfg, "cap %d on b, %s" % (n, kind), above_a=other, above_b=n))
        out.append(cluster_pair(rng, n, n, 3, 2, "distinct", cfg, "cap %d on both" % n))
    for n in (8192, 8193):
        out.append(cluster_pair(rng, n + 3, 2, 2, 1, "distinct", cfg, "cap %d on a" % n, above_a=n, above_b=2))
        out.append(cluster_pair(rng, 1, n, 1, 2, "ties", cfg, "cap %d on b" % n))
    # 2 100 x 2 100 in one window: tied beyond listing and found after a few trips of the loop; and with nothing in the window: the full loop
    out.append(cluster_pair(rng, 2100, 2100, 2100, 2100, "ties", cfg, "2100x2100 in one window", spread=100, gap=cfg["min_d"] + 150))
    out.append(cluster_pair(rng, 2100, 2100, 2100, 2100, "ties", cfg, "2100x2100, nothing in the window", spread=100, gap=cfg["max_d"] + 4000))
    out.append(cluster_pair(rng, 2100, 2100, 2100, 2100, "nonpos", cfg, "2100x2100 in one window, nothing positive", spread=100, gap=cfg["min_d"] + 150))
    if with_host:
        out.append(cluster_pair(rng, 65536, 1, 1, 1, "distinct", cfg, "65536 candidates on a", above_a=3, above_b=1))
        out.append(cluster_pair(rng, 2, 65536, 1, 1, "distinct", cfg, "65536 candidates on b", above_a=2, above_b=5))
        out.append(cluster_pair(rng, 65535, 1, 1, 1, "distinct", cfg, "65535 candidates on a", above_a=3, above_b=1))
    return out


def _kinded(rng, cfg, shape, host_kind):
    """one pair of a persistent-loop population: neighbours differ in what they leave in a workgroup's shared state"""
    kind = int(rng.integers(0, 5))
    ca, cb, full = shape(kind)
    if kind == 0:     # found, unique
        return cluster_pair(rng, ca, cb, 1, 1, "distinct", cfg, "loop: found")
    if kind == 1:     # tied with more than 64 combinations (where the shape allows them), found
        ca, cb, ka, kb = full
        return cluster_pair(rng, ca, cb, ka, kb, "ties", cfg, "loop: tied beyond listing")
    if kind == 2:     # no combination
        return cluster_pair(rng, ca, cb, 1, 1, "none", cfg, "loop: no combination")
    if kind == 3:
        return host_kind(ca, cb)
    return cluster_pair(rng, ca, cb, min(ca, 2), 1, "equal", cfg, "loop: tied, listed")


def loop_pairs(rng, cfg, n_small, n_large, n_huge):
    """more pairs per list than its launch has workgroups: each workgroup takes several pairs, one after the other"""
    out = []
    neg_shared = lambda ca, cb: _pair([-5] * max(ca, 2), 10_000_000 + 10 * np.arange(max(ca, 2)), [100] * cb, 10_000_300 + 10 * np.arange(cb), "loop: host (negative best shared)")
    for _ in range(n_small):
        out.append(_kinded(rng, cfg, lambda k: (int(rng.integers(2, 4)), int(rng.integers(1, 4)), (9, 8, 9, 8)), neg_shared))
    for _ in range(n_large):
        out.append(_kinded(rng, cfg, lambda k: (int(rng.integers(65, 71)), int(rng.integers(1, 4)), (int(rng.integers(65, 71)), 3, 65, 1 + int(rng.integers(0, 3)))), neg_shared))
    over = lambda ca, cb: cluster_pair(rng, CAP_HUGE + 1, 1, 1, 1, "distinct", cfg, "loop: host (beyond the third launch)") if rng.random() < 0.3 else \
        cluster_pair(rng, 2100, 1, 1, 1, "none", cfg, "loop: no combination")
    for _ in range(n_huge):
        out.append(_kinded(rng, cfg, lambda k: (2100, 1, (2100, 1, 2100, 1)), over))
    return out


def unlimited_pairs(rng):
    """no upper window bound (max_insert 0): insert sizes around 2^30 -- where pair_simple_kernel's `info` runs out of bits -- and up to
    the largest `int`, on 1 x 1 and 2 x 1 pairs"""
    out = []
    for d in (2 ** 30 - 1, 2 ** 30, 2 ** 30 + 1, 2 ** 31 - 2, 2 ** 31 - 1, 2 ** 31, 2 ** 29, 400):
        for up in (True, False):
            l1 = 1000 + int(rng.integers(0, 1000)) if up else 2 ** 32 - 1 - int(rng.integers(0, 1000))
            l2 = _lb_for(l1, d, up)
            out.append(_pair([1400], [l1], [1390], [l2], "unlimited 1x1 d=%d" % d))
            out.append(_pair([1400], [l1], [-1500], [l2], "unlimited 1x1 d=%d, not positive" % d))
            out.append(_pair([1400, 1000], [l1, l1 + 1], [1390], [l2], "unlimited 2x1 d=%d" % d))
            out.append(_pair([1400, 1400], [l1, l1 + 1], [1390], [l2], "unlimited 2x1 tied d=%d" % d))
    return out


def interleave(rng, groups):
    """all classes mixed, with 1 x 1 and empty pairs between them"""
    pairs = [p for g in groups for p in g]
    n_fill = max(len(pairs) // 3, 600)
    for x in range(n_fill):
        l1 = int(rng.integers(10_000_000, 2_000_000_000))
        if x % 5 == 4:
            pairs.append(_pair([], [], [1400] * (x % 3), l1 + np.arange(x % 3), "filler: empty mate"))
        else:
            pairs.append(_pair([int(rng.integers(-10, 1400))], [l1], [int(rng.integers(1, 1400))], [l1 + int(rng.integers(-1200, 1200))], "filler: 1x1"))
    return [pairs[i] for i in rng.permutation(len(pairs))]


def make_batches(seed=20261019):
    """the batches both test modules use: (window, cut-off) x the edges above"""
    rng = np.random.default_rng(seed)
    out = []
    cfg = {"min_d": 100, "max_d": 1000, "cutoff": 0.9}
    groups = [special_pairs(rng, cfg), count_edge_pairs(rng, cfg), cap_edge_pairs(rng, cfg), loop_pairs(rng, cfg, 9000, 1100, 270)]
    out.append(Batch("window 100..1000, cutoff 0.9", 100, 1000, 0.9, interleave(rng, groups), rng))
    cfg = {"min_d": 0, "max_d": 600, "cutoff": 0.5}
    groups = [special_pairs(rng, cfg), count_edge_pairs(rng, cfg), cap_edge_pairs(rng, cfg, with_host=False)]
    out.append(Batch("window 0..600, cutoff 0.5", 0, 600, 0.5, interleave(rng, groups), rng))
    cfg = {"min_d": 30, "max_d": 2000, "cutoff": 1.0}
    groups = [special_pairs(rng, cfg), count_edge_pairs(rng, cfg)]
    out.append(Batch("window 30..2000, cutoff 1.0", 30, 2000, 1.0, interleave(rng, groups), rng))
    cfg = {"min_d": 0, "max_d": INT_MAX, "cutoff": 0.9}
    groups = [unlimited_pairs(rng), special_pairs(rng, cfg)]
    out.append(Batch("no upper bound, cutoff 0.9", 0, 0, 0.9, interleave(rng, groups), rng))
    return out
