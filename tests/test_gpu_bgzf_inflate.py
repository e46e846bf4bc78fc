"""-m gpu: BGZF members inflated by the GPU (nextgenmap_amd/csrc/bgzf_inflate_device.h) through pipeline.Bgzf.decompress, against
zlib -- the library the reference reads every .gz and BAM input with.  Every comparison is for identical bytes.  The members are
those of tests/bam_fixtures.py; test_bam_input_host.py has run the same ones, good and damaged, through the same decoder functions
on the CPU under sanitizers."""
import pytest

import bam_fixtures as BF

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def z():
    from nextgenmap_amd.pipeline import Bgzf
    z = Bgzf(0)
    yield z
    z.close()


@pytest.fixture(scope="module")
def good():
    return BF.good_cases()


GOOD = ["eof_alone", "eof_between", "one_byte", "stored_65280", "stored_empty", "fixed_distance_one", "fastq_level1", "fastq_level6", "fastq_level9", "bam_level1",
        "bam_level6", "bam_level9", "huffman_only", "rle", "long_codes", "all_distances", "flush_points", "isize_65536", "random_65280", "one_member", "three_members",
        "three_thousand_members"]


@pytest.mark.parametrize("name", GOOD)
def test_good_members(z, good, name):
    assert set(GOOD) == set(good)
    members, text = good[name]
    assert BF.zlib_text(members) == text
    assert z.decompress(members) == text


def test_round_trip_of_the_gpu_compressor(z):
    data = BF.bam_like(900, 8) + BF.fastq_text(700, 9) + bytes(70001)
    assert z.decompress(z.compress(data)) == data


@pytest.mark.parametrize("name", ["wrong_crc", "isize_too_small", "isize_too_large", "incomplete_literal_code", "distance_before_first_byte", "ends_before_end_of_block"])
def test_damaged_member_is_refused_and_the_next_call_works(z, name):
    good = BF.member(BF.fastq_text(30, 2))
    bad = BF.damaged_cases()[name]
    with pytest.raises(RuntimeError, match=r"member 1 refused"):
        z.decompress(good + bad + good)
    assert z.decompress(good + good) == BF.fastq_text(30, 2) * 2


def test_not_bgzf_is_refused_by_the_host(z):
    import gzip
    with pytest.raises(RuntimeError, match="not a run of whole BGZF members"):
        z.decompress(gzip.compress(b"hello"))
    with pytest.raises(RuntimeError, match="not a run of whole BGZF members"):
        z.decompress(BF.member(b"hello")[:-3])
