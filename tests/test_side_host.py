"""No GPU: what the host sides of --coverage, --snp and --count share (nextgenmap_amd/csrc/side_host.h: the checks in front of an add, the
whole-lines rule of a text output's next, the contigs' table) through tests/cpp/side_host_driver.cpp, a stand-alone program built with
g++ -fsanitize=address,undefined.  The expected messages are the ones the three add functions have always set."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "side_host_driver.cpp")
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
N = 10   # alignments of a batch: 5M over five bases each


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("side_host_driver")
    out = str(d / "side_host_driver_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", out])
    return out, d


def _run(exe, args, text=None):
    prog, d = exe
    p = str(d / "case.txt")
    if text is not None:
        with open(p, "wb") as f:
            f.write(text if isinstance(text, bytes) else text.encode())
    r = subprocess.run([prog] + [p if a == "IN" else str(a) for a in args], capture_output=True, env=SAN_ENV, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    return r.stdout


def batch(with_seq=True, qual=None):
    """a batch every check passes: its arrays as lists that a case then damages"""
    return {"n_ref": 2, "ref_id": [i % 2 for i in range(N)], "pos0": [10 * i for i in range(N)], "cigar_off": [2 * i for i in range(N + 1)], "cigar": "5M" * N,
            "seq_off": [5 * i for i in range(N + 1)] if with_seq else None, "seq": "ACGTA" * N if with_seq else None, "qual": qual}


def check(exe, fn, b):
    word = lambda t: "NULL" if t is None else (t or "-")
    nums = lambda v: " ".join(str(x) for x in v)
    text = "%d %d\n%s\n%s\n%s\n%s\n%s\n%s\n%s\n" % (b["n_ref"], N, nums(b["ref_id"]), nums(b["pos0"]), nums(b["cigar_off"]), word(b["cigar"]),
                                                  "NULL" if b["seq_off"] is None else nums(b["seq_off"]), word(b["seq"]), word(b["qual"]))
    out = _run(exe, ["check", fn, "cov" if fn == "ngm_coverage_add" else "snp", "IN"], text).decode().split("\n")
    return int(out[0]), out[1]


FNS = ["ngm_coverage_add", "ngm_snp_add", "ngm_count_add"]


def _batch_for(fn, qual=None):
    return batch(with_seq=fn != "ngm_coverage_add", qual=qual)


@pytest.mark.parametrize("fn", FNS)
def test_check_batch_passes_a_sound_batch(exe, fn):
    assert check(exe, fn, _batch_for(fn)) == (0, "")
    if fn != "ngm_coverage_add":
        assert check(exe, fn, _batch_for(fn, qual="I" * (5 * N))) == (0, "")


@pytest.mark.parametrize("fn", FNS)
@pytest.mark.parametrize("i", [0, 5, N - 1], ids=["first", "middle", "last"])
def test_check_batch_refuses_descending_cigar_offsets_by_index(exe, fn, i):
    b = _batch_for(fn)
    if i == 0:
        b["cigar_off"][0] = b["cigar_off"][1] + 2
    else:
        b["cigar_off"][i + 1] = b["cigar_off"][i] - 1
    assert check(exe, fn, b) == (-22, "%s: alignment %d: its CIGAR offsets do not ascend" % (fn, i))


@pytest.mark.parametrize("fn", FNS[1:])
@pytest.mark.parametrize("i", [0, 5, N - 1], ids=["first", "middle", "last"])
def test_check_batch_refuses_descending_sequence_offsets_by_index(exe, fn, i):
    b = _batch_for(fn)
    if i == 0:
        b["seq_off"][0] = b["seq_off"][1] + 2
    else:
        b["seq_off"][i + 1] = b["seq_off"][i] - 1
    assert check(exe, fn, b) == (-22, "%s: alignment %d: its sequence offsets do not ascend" % (fn, i))


@pytest.mark.parametrize("fn", FNS)
def test_check_batch_refuses_a_missing_text_under_offsets_that_are_not_empty(exe, fn):
    b = _batch_for(fn)
    b["cigar"] = None
    assert check(exe, fn, b) == (-22, "%s: alignment 0: its CIGAR offsets do not ascend" % fn)
    if fn != "ngm_coverage_add":
        b = _batch_for(fn)
        b["seq"] = None
        assert check(exe, fn, b) == (-22, "%s: alignment 0: its sequence offsets do not ascend" % fn)
        # (offsets that are all the same need no text; the validator then refuses the empty sequence under a CIGAR that consumes five bases)
        b["seq_off"] = [7] * (N + 1)
        assert check(exe, fn, b) == (-22, "%s: alignment 0: its sequence is shorter or longer than the read bases its CIGAR consumes" % fn)


@pytest.mark.parametrize("fn", FNS[1:])
def test_check_batch_quality_text_names_the_first_record_it_does_not_reach(exe, fn):
    why = "its quality text has another length than its sequence"
    assert check(exe, fn, _batch_for(fn, qual="I" * (5 * N - 1))) == (-22, "%s: alignment %d: %s" % (fn, N - 1, why))   # one byte short: the last record
    assert check(exe, fn, _batch_for(fn, qual="I" * 22)) == (-22, "%s: alignment 4: %s" % (fn, why))                    # [20, 25) is not reached
    assert check(exe, fn, _batch_for(fn, qual="")) == (-22, "%s: alignment 0: %s" % (fn, why))
    assert check(exe, fn, _batch_for(fn, qual="I" * (5 * N + 1))) == (-22, "%s: alignment %d: %s" % (fn, N - 1, why))   # one byte long


@pytest.mark.parametrize("fn", FNS)
def test_check_batch_hands_on_the_objects_own_verdict_with_its_index(exe, fn):
    b = _batch_for(fn)
    b["ref_id"][3] = 2
    assert check(exe, fn, b) == (-22, "%s: alignment 3: its ref_id is not in [0, n_ref)" % fn)
    b = _batch_for(fn)
    b["pos0"][7] = -1
    assert check(exe, fn, b) == (-22, "%s: alignment 7: its position is negative" % fn)
    # the offsets are looked at first: a record with both faults is refused for its offsets
    b["cigar_off"][8] = b["cigar_off"][7] - 1
    assert check(exe, fn, b) == (-22, "%s: alignment 7: its CIGAR offsets do not ascend" % fn)


# ---- take_whole_lines ---------------------------------------------------------------------------------------------------------------
LINES = b"chr1\t0\t5\t1\n" + b"chr1\t5\t1000\t27\n" + b"chrUn_gl000220\t7\t9\t3\n"   # 11, 15 and 21 bytes


def take(exe, cap, with_out=True, text=LINES):
    out = _run(exe, ["take", "IN", cap, 1 if with_out else 0], text)
    head, _, rest = out.partition(b"\n")
    r, taken = (int(x) for x in head.split())
    assert len(rest) == taken
    return r, rest


def test_take_whole_lines_copies_as_many_whole_lines_as_fit(exe):
    for cap in (0, 1, 10):
        assert take(exe, cap) == (11, b"")               # below the first line: its size, nothing copied
    assert take(exe, 11) == (11, LINES[:11])             # exactly one line
    assert take(exe, 25) == (11, LINES[:11])             # one byte short of two lines
    assert take(exe, 26) == (26, LINES[:26])
    assert take(exe, 46) == (26, LINES[:26])
    assert take(exe, 47) == (47, LINES)
    assert take(exe, 4096) == (47, LINES)
    for cap in (0, 5, 11, 4096):
        assert take(exe, cap, with_out=False) == (11, b"")   # no buffer: the size of the first line


def test_take_whole_lines_drains_three_lines_from_a_buffer_of_one_byte_that_grows(exe):
    out = _run(exe, ["drain", "IN"], LINES)
    head, _, rest = out.partition(b"\n")
    assert [int(x) for x in head.split()] == [11, 15, 21]
    assert rest == LINES


# ---- RefView ------------------------------------------------------------------------------------------------------------------------
def ref(exe, contigs):
    text = "%d\n" % len(contigs) + "".join("%s %d %s\n" % ("NULL" if nm is None else nm, ln, "NULL" if sq is None else (sq or "-")) for nm, ln, sq in contigs)
    return _run(exe, ["ref", "IN"], text).decode().split("\n")


def test_refview_from_the_callers_arrays(exe):
    contigs = [("chr1", 10, "ACGTNacgtn"), ("two", 0, ""), ("chrM", 7, "TTRYGCA")]
    out = ref(exe, contigs)
    assert out[0] == "ok"
    assert [int(x) for x in out[1].split()] == [10, 0, 7]
    assert [int(x) for x in out[2].split()] == [0, 10, 10, 17]
    cls = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 5}
    bases = "".join(sq for _, _, sq in contigs).upper()
    words = [0] * ((len(bases) + 7) // 8 + 1)
    for p, ch in enumerate(bases):
        words[p >> 3] |= cls.get(ch, 4) << (4 * (p & 7))
    assert [int(x, 16) for x in out[3].split()] == words
    assert out[4] == "chr1twochrM" and [int(x) for x in out[5].split()] == [0, 4, 7, 11]


def test_refview_refuses_a_short_sequence_and_a_missing_name_by_the_contigs_index(exe):
    assert ref(exe, [("a", 4, "ACGT"), ("b", 5, "ACGT"), ("c", 9, "AC")])[:2] == ["refused", "ngm_snp_create: the sequence of contig 1 is shorter than its length"]
    assert ref(exe, [("a", 4, "ACGT"), ("b", 4, None)])[:2] == ["refused", "ngm_snp_create: the sequence of contig 1 is shorter than its length"]
    assert ref(exe, [("a", 4, "ACGT"), ("b", 4, "ACGT"), (None, 2, "AC")])[:2] == ["refused", "ngm_snp_create: contig 2 has no name"]
    assert ref(exe, [("a", 3, "ACGT")])[0] == "ok"   # (longer than declared: the declared bases are the contig)
