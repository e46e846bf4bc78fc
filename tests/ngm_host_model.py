"""Python restatement of the host-side glue of NextGenMap's score/align stages (test infrastructure):
concatenated genome layout, DecodeRefSequence, reverse complement, top1SE / MAPQ, final position.
Used together with the C oracle (oracle/) to predict what the device pipeline must output."""
import math

import numpy as np

COMP = np.arange(256, dtype=np.uint8)
for a, b in zip(b"ACGT", b"TGCA"):
    COMP[a] = b


def concat_genome(contigs):
    """SequenceProvider.cpp:289-326: 1000 N, then per contig: bases (non-ACGT -> N, upper-cased), one N if the
    length is odd, 1000 N.  Contigs of length <= 10 are skipped.  Returns (ascii array, [(start, len)], n_bases)."""
    parts = [np.full(1000, ord("N"), np.uint8)]
    geom = []
    pos = 1000
    lut = np.full(256, ord("N"), np.uint8)
    for a, b in zip(b"ACGTacgt", b"ACGTACGT"):
        lut[a] = b
    for c in contigs:
        c = np.asarray(c, dtype=np.uint8)
        if c.size <= 10:
            continue
        geom.append((pos, int(c.size)))
        parts.append(lut[c])
        pos += c.size
        if c.size & 1:
            parts.append(np.full(1, ord("N"), np.uint8))
            pos += 1
        parts.append(np.full(1000, ord("N"), np.uint8))
        pos += 1000
    g = np.concatenate(parts)
    return g, geom, int(g.size)


def decode_ref(genome, n_bases, offset, buffer_len):
    """_SequenceProvider::DecodeRefSequence (SequenceProvider.cpp:382-441) -> (ok, bytes[buffer_len])."""
    concat_len = n_bases - 1
    out = np.zeros(buffer_len, np.uint8)
    ln = buffer_len - 2
    if offset >= concat_len:
        return False, out
    end = 0
    if offset + ln > concat_len:
        end = offset + ln - concat_len
        ln -= end
    idx = 0
    if offset & 1:
        out[idx] = genome[offset]
        idx += 1
        start = offset + 1
    else:
        start = offset
    k = 2 * ((ln + 1) // 2)
    out[idx:idx + k] = genome[start:start + k]
    idx += k
    if ln & 1:
        out[idx - 1] = ord("x")
    out[idx:idx + end] = ord("x")
    return True, out


def revcomp_row(row, length):
    out = np.zeros_like(row)
    out[:length] = COMP[row[:length][::-1]]
    return out


def compute_mq(best, second):
    if best > 0 and second >= 0:
        return int(math.ceil(np.float32(60.0) * (np.float32(best) - np.float32(second)) / np.float32(best)))
    return 0


def top1(scores, keys):
    """ScoreBuffer::top1SE (ScoreBuffer.cpp:228-277) with the device pipeline's tie rule (smallest key)."""
    best = second = 0.0
    num = 0
    for s in scores:
        if s > second:
            if s > best:
                second, best, num = best, s, 1
            elif s == best:
                num += 1
                second = best
            else:
                second = s
        elif s == best:
            num += 1
    if num > 0:
        cands = [i for i, s in enumerate(scores) if s == best]
    else:
        cands = list(range(len(scores)))
    win = min(cands, key=lambda i: keys[i])
    return win, compute_mq(best, second), num, best


def convert(geom, pos):
    """_SequenceProvider::convert (SequenceProvider.cpp:111-141)."""
    starts = [s for s, _ in geom] + [geom[-1][0] + geom[-1][1] + 1000]
    import bisect
    u = bisect.bisect_right(starts, pos)
    if u == 0 or u >= len(starts):
        return None
    if starts[u] - pos < 1000:
        return None
    return u - 1, pos - starts[u - 1]


# ---- the gather of (read, window) pairs into the DP kernels' packed layout (gather_pairs_kernel, csrc/gather_device.h) ----------------
READ_CLASS = np.full(256, 5, np.uint8)   # reads hold A C G T N (IParser.h:59-121): anything else counts as N
WIN_CLASS = np.full(256, 5, np.uint8)    # what DecodeRefSequence leaves in a window: the genome's A C G T N, 'x', NUL
for _k, _ch in enumerate(b"ACGT"):
    READ_CLASS[_ch] = WIN_CLASS[_ch] = _k
READ_CLASS[0] = WIN_CLASS[0] = 6
WIN_CLASS[ord("x")] = 4


def pack8(k):
    """class codes [..., 8] -> one dword: nibble 2j = base j, nibble 2j + 1 = base j + 4"""
    k = np.asarray(k, np.uint32)
    w = np.zeros(k.shape[:-1], np.uint32)
    for j in range(8):
        w |= k[..., j] << np.uint32(4 * (2 * j if j < 4 else 2 * (j - 4) + 1))
    return w


def gather_pairs_model(genome, n_bases, rows, pair_read, pair_loc, pair_sv, q, c, rw, fw, alt_dir=0, align_stage=False):
    """-> (words uint32 [blocks, rw + fw, 64], lens uint16 [pairs], blk_rows uint16 [blocks]): per pair the read (reverse-complemented for
    a pair on the reverse strand, MappedRead::computeReverseSeq) and its window (DecodeRefSequence at loc - c / 2 with the stage's buffer
    length; all N where that fails -- a loc below c / 2 wraps), as symbol classes, eight per word, rows interleaved over the 64 slots of a
    block.  Bit 3 of the read classes: the pair uses the reverse score table (alt_dir 1: reverse strand; 2: second mates flip).  Lanes
    beyond the last pair hold class 6 everywhere."""
    rows = np.asarray(rows, np.uint8)
    n = len(pair_read)
    nb = (n + 63) // 64
    buffer_len = ((q + c) | 2) if align_stage else (((q + c) | 1) + 1)
    read_len = np.array([int(np.flatnonzero(r == 0)[0]) if (r == 0).any() else q for r in rows])
    cls = np.full((nb * 64, 8 * (rw + fw)), 6, np.uint32)
    lens = np.zeros(n, np.uint16)
    blk_rows = np.zeros(nb, np.uint16)
    for p in range(n):
        ridx, rev = int(pair_read[p]), bool(int(pair_sv[p]) & 1)
        L = int(read_len[ridx])
        read = revcomp_row(rows[ridx], L) if rev else rows[ridx]
        second = alt_dir == 2 and (ridx & 1)
        dbit = 8 if alt_dir and ((not second) if rev else second) else 0
        rc = np.full(8 * rw, 6, np.uint32)
        rc[:L] = READ_CLASS[read[:L]]
        cls[p, :8 * rw] = rc | dbit
        offset = (int(pair_loc[p]) - (c >> 1)) % (1 << 64)
        ok, win = decode_ref(genome, n_bases, offset, buffer_len)
        wc = np.full(8 * fw, 5 if not ok else 6, np.uint32)
        if ok:
            k = min(buffer_len, 8 * fw)
            wc[:k] = WIN_CLASS[win[:k]]
        cls[p, 8 * rw:] = wc
        lens[p] = L
        blk_rows[p // 64] = max(blk_rows[p // 64], L)
    words = pack8(cls.reshape(nb, 64, rw + fw, 8)).transpose(0, 2, 1)
    return np.ascontiguousarray(words), lens, blk_rows
