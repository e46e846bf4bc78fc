"""-m gpu: the BGZF compressor's code-length repair (csrc/bgzf_device.h, build_lengths) on members whose Huffman trees reach three and more
levels below their limit.  The repair makes one move per unit of 2^-max by which the clamped lengths over-subscribe the code; counting
half the clamped leaves instead (as it did before `--sort`) is too few moves for some shapes of such a tree, and the member does not
inflate.  Which shapes depends on the whole histogram: the records case below is one the old count got wrong (its code-length code, limit
7 bits: zlib said "invalid code lengths set"); the Fibonacci cases put literals 16 to 21 levels deep (limit 15 bits) -- on these seeds
both counts agree, the matcher's length symbols decide the parity -- and pin that path with literals where tests/test_gpu_bgzf.py's
"fib" case has runs, which the matcher turns into a handful of matches.  Every member must inflate with zlib to its input."""
import random
import struct
import zlib

import pytest

pytestmark = pytest.mark.gpu
FIB = [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584, 4181, 6765, 10946, 17711]   # sum 46 367: one member


def _members_inflate(data):
    from nextgenmap_amd import pipeline as P
    z = P.Bgzf(0)
    try:
        out = z.compress(data)
    finally:
        z.close()
    at, text = 0, []
    while at < len(out):
        n = struct.unpack_from("<H", out, at + 16)[0] + 1
        text.append(zlib.decompress(out[at + 18:at + n - 8], -15))   # raises on an over-subscribed or incomplete code
        assert struct.unpack_from("<II", out, at + n - 8) == (zlib.crc32(text[-1]), len(text[-1]))
        at += n
    assert b"".join(text) == data


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_literal_tree_far_below_fifteen_bits(seed):
    """22 literals in a chain 21 levels deep before the repair: six leaves at 16 to 21 bits"""
    data = bytearray(b"".join(bytes([65 + i]) * f for i, f in enumerate(FIB)))
    random.Random(seed).shuffle(data)
    _members_inflate(bytes(data))


def test_code_length_code_far_below_seven_bits():
    """BAM records of one shape (the same name pattern, 40 random bases, 40 quality bytes 0xFF, one record padded with a run): few distinct
    literals, so nearly all of the 316 code lengths are 0 and the rest spread thinly -- the code-length code's own tree goes below 7 bits.
    This input did not inflate before the repair counted its moves by the over-subscription."""
    import bam_fixtures as BF
    rnd = random.Random(81)
    recs = [BF.bam_record(b"b%04d" % i, bytes(rnd.choice(b"ACGT") for _ in range(40)), None, 0, [(0, 40)], ref_id=0, pos=100 + 50 * i) for i in range(1500)]
    recs[700] = BF.bam_record(b"b0700", b"ACGT" * 10, None, 0, [(0, 40)], ref_id=0, pos=35100, tags=b"XXZ" + b"p" * 150 + b"\0")
    _members_inflate(b"".join(recs))
