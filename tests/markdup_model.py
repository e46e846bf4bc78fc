"""The rules of `ngm-hip --sort --markdup` (include/ngm_pipeline.h, INTEGRATION.md "Duplicate marking") in plain Python, over a list of BAM
records (bytes) in run order.  This is the specification: nextgenmap_amd/csrc/markdup.h and markdup_device.h must compute exactly this.

  examined   flag 0x4, 0x100 and 0x800 clear and refID >= 0; other records are never marked and never count
  u5         forward strand: pos - leading S/H lengths; reverse strand: end - 1 + trailing S/H lengths (end = pos + M/D/N/=/X lengths,
             pos + 1 without any); clamped to [U5_MIN, U5_MAX]; without CIGAR operations u5 = pos
  end key    (refID, u5, strand), packed as refID << 32 | (u5 - U5_MIN) << 1 | strand
  mates      records g and g + 1, both examined, both 0x1, one has 0x40 and not 0x80, the other 0x80 and not 0x40, equal names
  pair       mates with the first mate (0x40) in front; or mates with the second mate in front (the order ngm-hip writes) of which neither
             is part of a pair of the first kind with its other neighbour -- so pairs never overlap.  Every other examined record is a
             fragment.  A pair's first mate is the record with 0x40, its run-order index that of its record in front
  score      sum of the quality bytes >= 15; 0 with absent qualities (first byte 0xFF) or l_seq 0; pairs: both mates; saturating at 2^32 - 1
  pairs      key = (lower end key, higher end key, "the lower end is the first mate's" when both strands are equal); the highest score
             survives, ties to the lowest g; both mates of the others get 0x400
  fragments  grouped by end key together with both ends of every pair; a group with a pair end marks all its fragments; else the highest
             score survives, ties to the lowest g
  the marker only ORs"""
import struct

U5_MIN, U5_MAX = -(1 << 30), (1 << 30) - 1
MIN_QUAL = 15
SCORE_MAX = (1 << 32) - 1
COUNT_NAMES = ("examined", "pairs", "fragments", "duplicate_pairs", "duplicate_fragments", "newly_marked")


def parse(rec):
    """(refID, pos, flag, name, [(op, len)], qualities)"""
    ref_id, pos, bmn, fnc, l_seq = struct.unpack_from("<iiIIi", rec, 4)
    l_name, n_cigar, flag = bmn & 0xFF, fnc & 0xFFFF, fnc >> 16
    at = 36 + l_name
    cigar = []
    for k in range(n_cigar):
        v, = struct.unpack_from("<I", rec, at + 4 * k)
        cigar.append((v & 15, v >> 4))
    at += 4 * n_cigar + (l_seq + 1) // 2
    return ref_id, pos, flag, rec[36:36 + l_name], cigar, rec[at:at + l_seq]


def examined(rec):
    ref_id, _, flag, _, _, _ = parse(rec)
    return not flag & 0x904 and ref_id >= 0


def u5(rec):
    _, pos, flag, _, cigar, _ = parse(rec)
    if not flag & 0x10:
        v = pos
        for op, n in cigar:
            if op not in (4, 5):
                break
            v -= n
    else:
        span = sum(n for op, n in cigar if op in (0, 2, 3, 7, 8))
        v = pos + (span or 1) - 1
        for op, n in reversed(cigar):
            if op not in (4, 5):
                break
            v += n
    return min(max(v, U5_MIN), U5_MAX)


def end_key(rec):
    ref_id, _, flag, _, _, _ = parse(rec)
    return ((ref_id & 0xFFFFFFFF) << 32) | ((u5(rec) - U5_MIN) << 1) | ((flag >> 4) & 1)   # (examined records have refID >= 0: bit 63 is clear)


def pair_key(e1, e2):
    """e1: the first mate's end key, e2: the second mate's -> (lo, hi, role bit)"""
    first_is_lo = e1 <= e2
    lo, hi = (e1, e2) if first_is_lo else (e2, e1)
    same_strand = (e1 & 1) == (e2 & 1)
    return lo, hi, 1 if same_strand and first_is_lo else 0


def score(rec):
    q = parse(rec)[5]
    if len(q) == 0 or q[0] == 0xFF:
        return 0
    total = 0
    for b in q:
        if b >= MIN_QUAL:
            total += b
    return min(total, SCORE_MAX)


def mates(a, b):
    """a, b: records g and g + 1.  0: no mates, 1: mates with the first mate in front, 2: with the second mate in front"""
    if not (examined(a) and examined(b)) or parse(a)[3] != parse(b)[3]:
        return 0
    roles = (parse(a)[2] & 0xC1, parse(b)[2] & 0xC1)
    return 1 if roles == (0x41, 0x81) else 2 if roles == (0x81, 0x41) else 0


def pair_order(records, g):
    """whether records g and g + 1 form a pair: 0, or which mate is in front"""
    if g < 0 or g + 1 >= len(records):
        return 0
    m = mates(records[g], records[g + 1])
    if m == 2 and ((g > 0 and mates(records[g - 1], records[g]) == 1) or (g + 2 < len(records) and mates(records[g + 1], records[g + 2]) == 1)):
        return 0
    return m


def with_flag(rec, bit):
    flag = struct.unpack_from("<H", rec, 18)[0] | bit
    return rec[:18] + struct.pack("<H", flag) + rec[20:]


def mark(records):
    """records in run order -> (the records with 0x400 applied, the six counts as a dict)"""
    n = len(records)
    kind = [None] * n                      # None: ignored, "f": fragment, 1 / 2: in front / behind in a pair
    first = {}                             # the record in front of a pair -> the pair's first mate (0x40)
    for g in range(n):
        o = pair_order(records, g)
        if o:
            assert kind[g] is None, "pairs overlap"
            kind[g], kind[g + 1] = 1, 2
            first[g] = g if o == 1 else g + 1
        elif kind[g] is None and examined(records[g]):
            kind[g] = "f"
    dup = [False] * n
    pair_groups, end_has_pair, frag_groups = {}, set(), {}
    for g in range(n):
        if kind[g] == 1:
            e1, e2 = end_key(records[first[g]]), end_key(records[2 * g + 1 - first[g]])
            pair_groups.setdefault(pair_key(e1, e2), []).append(g)
            end_has_pair.update((e1, e2))
        elif kind[g] == "f":
            frag_groups.setdefault(end_key(records[g]), []).append(g)
    dup_pairs = dup_frags = 0
    for members in pair_groups.values():
        if len(members) < 2:
            continue
        best = min(members, key=lambda g: (-min(score(records[g]) + score(records[g + 1]), SCORE_MAX), g))
        for g in members:
            if g != best:
                dup[g] = dup[g + 1] = True
                dup_pairs += 1
    for key, members in frag_groups.items():
        if key in end_has_pair:
            losers = members
        elif len(members) < 2:
            continue
        else:
            best = min(members, key=lambda g: (-score(records[g]), g))
            losers = [g for g in members if g != best]
        for g in losers:
            dup[g] = True
            dup_frags += 1
    out, newly = [], 0
    for g, rec in enumerate(records):
        if dup[g]:
            if not parse(rec)[2] & 0x400:
                newly += 1
            rec = with_flag(rec, 0x400)
        out.append(rec)
    counts = dict(examined=sum(k is not None for k in kind), pairs=sum(k == 1 for k in kind), fragments=sum(k == "f" for k in kind),
                  duplicate_pairs=dup_pairs, duplicate_fragments=dup_frags, newly_marked=newly)
    return out, counts
