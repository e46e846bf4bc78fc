"""The candidate search of NextGenMap in plain Python / numpy, restated from the reference's sources and not from csrc/: the oracle of
tests/test_cs_model.py (against results recorded from the reference program, tests/golden/search/) and tests/test_gpu_cs_shapes.py
(the kernels against this model).

The index (PrefixTable.cpp).  The genome is the concatenation of ngm_host_model.concat_genome.  Every contig is walked by PrefixIteration
(CSstatic.cpp:26-76) with the index's kmer_skip: a k-mer of the 2-bit codes A0 C1 T2 G3 is handed on at the first position of a walk and
then at every (skip + 1)-th; an N ends the walk and a new one begins behind it (the skip count starts over); a walk that begins with a run
of n Ns drops everything behind it when n >= remaining length - k; the last two bases of a contig walk as A whatever they are
(PrefixTable.cpp:347-348 with SequenceProvider.cpp:382-441).  CountKmer / BuildPrefixTable (:641-709) leave out a k-mer that equals
the two k-mers handed on before it when it lies in the bin (position >> bin_size) of its predecessor.  The positions of a k-mer are stored
in the order of the walk (ascending).  A k-mer whose count plus the count of its reverse complement is above 9 900 keeps its slots but is
"unused" (createRefTableIndex :432-498: a weight that truncates to 0): a lookup sees it as absent and its slots stay 0.

The search of one read (CS.cpp).  Every k-mer of the read is looked up (the read's walk has skip 0) together with its reverse complement;
both lists are voted when the sum of their lengths is below max_kfreq (:122).  A forward hit at genome position loc of the k-mer at read
position pos votes for bin (loc - pos) >> bin_size, a reverse hit for (loc - (len - (pos + k))) >> bin_size (:140-152).  With the largest
vote count of any (bin, strand) the threshold is max(kmer_min, max * sensitivity) in float32 (:204, :274); every (bin, strand) with at least
that many votes is a candidate at ResolveBin(bin) (CS.h:170-175) -- unless there are max_cmrs of them or more, then the read has none
(:308-310)."""
import hashlib
import math
from collections import namedtuple

import numpy as np

import ngm_host_model as HM

CODE = np.full(256, 4, np.uint8)   # CSstatic.cpp:19-22 ((c >> 1) & 3); 4: N
for _ch, _v in zip(b"ACTG", range(4)):
    CODE[_ch] = _v

UNUSED_ABOVE = 9900       # createRefTableIndex: (10000 - min(total, 10000)) * 100.0f / 10000 stored in a char is 0 from 9 901 on
FIRST_LAST_PREFIX = 111111   # CountKmerFreq / Generate: lastPrefix at the head of a contig

Index = namedtuple("Index", "k skip bin_size kmers raw used starts positions")
Result = namedtuple("Result", "cands max_votes max_combined threshold accepted")


def kmer_starts(codes, k, skip):
    """PrefixIteration: the start positions of the k-mers handed to func, for a sequence of codes (4 = N)"""
    total = len(codes)
    n_at = np.flatnonzero(codes == 4)
    base_at = np.flatnonzero(codes != 4)
    out = []
    s, length = 0, total
    while length >= k:
        if codes[s] == 4:
            i = np.searchsorted(base_at, s)
            n_skip = (int(base_at[i]) if i < len(base_at) else total) - s
            if n_skip >= length - k:
                break
            s += n_skip
            length -= n_skip
        i = np.searchsorted(n_at, s)
        seg = (int(n_at[i]) - s) if i < len(n_at) else length
        if seg >= k:
            out.append(np.arange(s, s + seg - k + 1, skip + 1, dtype=np.int64))
        if seg == length:
            break
        s += seg + 1
        length -= seg + 1
    return np.concatenate(out) if out else np.zeros(0, np.int64)


def kmer_values(codes, k):
    """the k-mer that starts at every position (garbage where it holds an N or runs over the end)"""
    c = np.concatenate([codes.astype(np.uint64) & np.uint64(3), np.zeros(k, np.uint64)])
    v = np.zeros(len(codes), np.uint64)
    for t in range(k):
        v = (v << np.uint64(2)) | c[t:t + len(codes)]
    return v


def revcomp_kmer(v, k):
    v = np.asarray(v, np.uint64).copy()
    out = np.zeros_like(v)
    for _ in range(k):
        out = (out << np.uint64(2)) | ((v & np.uint64(3)) ^ np.uint64(2))
        v >>= np.uint64(2)
    return out


def build_index(contigs, k, skip, bin_size=2):
    g, geom, _ = HM.concat_genome(contigs)
    vals, poss = [], []
    for start, ln in geom:
        codes = CODE[g[start:start + ln]]
        codes[-2:] = 0   # CountKmerFreq / Generate decode a contig with bufferLength = len: DecodeRefSequence writes len - 2 bases, and
        #                  encode() turns its 'x' filler and the zero bytes behind it into code 0: the last two bases walk as A
        st = kmer_starts(codes, k, skip)
        if st.size == 0:
            continue
        v = kmer_values(codes, k)[st]
        pos = st + start
        same = np.empty(len(v), bool)
        same[0] = v[0] == FIRST_LAST_PREFIX
        same[1:] = v[1:] == v[:-1]
        b = pos >> bin_size
        keep = np.ones(len(v), bool)
        keep[1:] = ~(same[1:] & same[:-1] & (b[1:] == b[:-1]))
        vals.append(v[keep])
        poss.append(pos[keep])
    vals = np.concatenate(vals) if vals else np.zeros(0, np.uint64)
    poss = np.concatenate(poss) if poss else np.zeros(0, np.int64)
    order = np.argsort(vals, kind="stable")
    kmers, raw = np.unique(vals, return_counts=True)
    positions = poss[order].astype(np.uint32)
    starts = np.concatenate([[0], np.cumsum(raw)])[:-1].astype(np.int64)
    rc = revcomp_kmer(kmers, k)
    j = np.minimum(np.searchsorted(kmers, rc), max(0, len(kmers) - 1))
    rc_raw = np.where(kmers[j] == rc, raw[j], 0) if len(kmers) else raw
    used = (raw + rc_raw) <= UNUSED_ABOVE
    for s, n in zip(starts[~used], raw[~used]):
        positions[s:s + n] = 0
    return Index(k, skip, bin_size, kmers, raw.astype(np.uint32), used, starts, positions)


def dense_counts(index):
    """(counts as a lookup sees them, raw counts), one entry per k-mer: what ref_files.read_ht_file and Reference.index_copy return"""
    raw = np.zeros(4 ** index.k, np.uint32)
    raw[index.kmers.astype(np.int64)] = index.raw
    counts = raw.copy()
    counts[index.kmers[~index.used].astype(np.int64)] = 0
    return counts, raw


def index_digests(index):
    """SHA-256 of the list lengths -- (k-mer, raw length, used) of every k-mer that occurs -- and of the position table"""
    h = hashlib.sha256()
    for a in (index.kmers.astype("<u8"), index.raw.astype("<u4"), index.used.astype("u1")):
        h.update(a.tobytes())
    return h.hexdigest(), hashlib.sha256(index.positions.astype("<u4").tobytes()).hexdigest()


def auto_max_kfreq(index):
    """CompactPrefixTable::stats (PrefixTable.cpp:150-194), over the raw list lengths"""
    n = float(4 ** index.k)
    r = index.raw.astype(np.float64)
    s, s2 = float(r.sum()), float((r * r).sum())
    avg = s / n
    stdev = math.sqrt(s2 / (n - 1) - 2.0 * avg * (s / (n - 1)) + ((n * avg ** 2) / (n - 1)))
    return int(math.ceil(max(100.0, avg + 5 * stdev)))


def lookup(index, v):
    """GetRefEntry for one strand: (list length, first slot) per k-mer of v"""
    if len(index.kmers) == 0:
        return np.zeros(len(v), np.int64), np.zeros(len(v), np.int64)
    i = np.minimum(np.searchsorted(index.kmers, v), len(index.kmers) - 1)
    hit = (index.kmers[i] == v) & index.used[i]
    return np.where(hit, index.raw[i], 0).astype(np.int64), index.starts[i]


def _gather(index, cnt, start, corr):
    """the genome positions of the lists (cnt, start), each minus its k-mer's correction"""
    tot = int(cnt.sum())
    if tot == 0:
        return np.zeros(0, np.int64)
    first = np.concatenate([[0], np.cumsum(cnt)])[:-1]
    slot = np.repeat(start - first, cnt) + np.arange(tot)
    loc = index.positions[slot].astype(np.int64)
    c = np.repeat(corr, cnt)
    assert np.all(loc >= c), "a hit in front of the genome's first base"
    return loc - c


def read_hits(read, index, max_kfreq):
    """(bins of the forward hits, bins of the reverse hits, k-mer start positions, per k-mer the forward and the reverse list's length)"""
    k = index.k
    codes = CODE[np.frombuffer(bytes(read), np.uint8)]
    st = kmer_starts(codes, k, 0)
    if st.size == 0:
        z = np.zeros(0, np.int64)
        return z, z, st, z, z
    v = kmer_values(codes, k)[st]
    fc, fs = lookup(index, v)
    rc, rs = lookup(index, revcomp_kmer(v, k))
    ok = (fc + rc) < max_kfreq
    fwd = _gather(index, np.where(ok, fc, 0), fs, st) >> index.bin_size
    rev = _gather(index, np.where(ok, rc, 0), rs, len(codes) - (st + k)) >> index.bin_size
    return fwd, rev, st, fc, rc


def resolve_bin(b, bin_size):
    return (b << bin_size) + ((1 << (bin_size - 1)) if bin_size > 0 else 0)


def threshold(max_votes, sensitivity, kmer_min):
    return max(np.float32(kmer_min), np.float32(np.float32(max_votes) * np.float32(sensitivity)))


def search(read, index, k, bin_size, max_kfreq, sensitivity, kmer_min=0.0, max_cmrs=2 ** 31 - 1):
    """-> Result: cands int64[n, 3] of (ResolveBin(bin), strand, votes) sorted, the largest vote count, the largest forward + reverse
    sum of one bin, the float32 threshold, the entries at or above it (before the max_cmrs rule)"""
    assert k == index.k and bin_size == index.bin_size
    fwd, rev, _, _, _ = read_hits(read, index, max_kfreq)
    none = np.zeros((0, 3), np.int64)
    if fwd.size + rev.size == 0:
        return Result(none, 0, 0, threshold(0, sensitivity, kmer_min), 0)
    key, votes = np.unique(np.concatenate([fwd * 2, rev * 2 + 1]), return_counts=True)
    _, inv = np.unique(key >> 1, return_inverse=True)
    max_votes = int(votes.max())
    max_combined = int(np.bincount(inv, weights=votes).max())
    thr = threshold(max_votes, sensitivity, kmer_min)
    acc = votes.astype(np.float32) >= thr
    n_acc = int(acc.sum())
    if n_acc >= max_cmrs:
        return Result(none, max_votes, max_combined, thr, n_acc)
    cands = np.stack([resolve_bin(key[acc] >> 1, bin_size), key[acc] & 1, votes[acc]], axis=1).astype(np.int64)
    return Result(cands, max_votes, max_combined, thr, n_acc)
