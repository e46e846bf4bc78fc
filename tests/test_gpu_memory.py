"""-m gpu: every byte of device and pinned host memory the library takes comes back (ngm::Owned, csrc/buffer.h), counted by the two HIP
policies of csrc/device_mem.h and read through ngm_debug_live_memory.  The counters are the library's own, so other processes on the card
do not enter into it, and every test compares against what it read before it created anything.

The world is the smallest genome the pipeline tests build (20 000 random bases, one contig) and one batch of 64 reads of 100 bases, 32
pairs: every stage runs, nothing is sized by the workload."""
import ctypes as C

import numpy as np
import pytest

import sam_cases as SC
from nextgenmap_amd import pipeline as P

pytestmark = pytest.mark.gpu

Q, CORRIDOR, N_READS, READ_LEN = 102, 20, 64, 100


@pytest.fixture(scope="module")
def world():
    rng = np.random.default_rng(20261021)
    genome = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 20000)]
    comp = np.zeros(256, np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    reads = []
    for p in rng.integers(100, 19000, N_READS // 2):
        reads += [genome[p:p + READ_LEN], comp[genome[p + 250:p + 250 + READ_LEN]][::-1]]
    rows = P.Mapper.reads_to_rows(reads, Q)
    return dict(genome=genome, rows=rows, names=["r%d" % i for i in range(N_READS)], quals=[b"I" * READ_LEN] * N_READS)


def _bytes(m):
    return m["device_bytes"], m["pinned_bytes"]


def _calls(m):
    return m["device_allocations"], m["pinned_allocations"]


def _cycle(w):
    """the reference, mappers and every stage and output on device 0, each fed the batch; destroyed again.  Returns live memory behind
    every step (the last sample: while all of them exist)."""
    seen = []
    mark = lambda: seen.append(_bytes(P.live_memory()))
    genome, rows, names, quals = w["genome"], w["rows"], w["names"], w["quals"]
    ref = P.Reference.from_contigs([genome])
    mp = P.Mapper(ref, Q, CORRIDOR)
    hits, _, _ = mp.map_se(rows)
    mark()
    assert int(hits["mapped"].sum()) >= N_READS - 8
    hits, _, _ = mp.map_pe(rows)
    mark()
    assert int((hits["pair_flags"] & 1).sum()) >= N_READS - 16        # (the batch does go through the pair selection)
    sam, stats = mp.map_sam(rows, quals, names, paired=True)
    mark()
    assert stats[0] == N_READS and sam.count(b"\n") == stats[2] > 0
    bam, stats = mp.map_sam(rows, quals, names, paired=True, bam=True)   # through the mapper's BGZF compressor
    mark()
    assert stats[0] == N_READS and bam[:4] == b"\x1f\x8b\x08\x04"
    argos = P.Mapper(ref, Q, CORRIDOR)
    text, stats = argos.map_argos(rows, names)
    mark()
    assert stats[0] == N_READS and text
    # the run-long outputs, fed by one more batch of a mapper they are attached to
    contig = ("chr1", bytes(genome))
    sorter = P.BamSorter(0)
    cov = P.Coverage([("chr1", len(genome))], 0)
    snp = P.SnpCaller(None, 0, reference=ref)
    cnt = P.ConversionCounter([contig], [(0, 0, len(genome), "all", "+")], 0, reference=ref)
    met = P.MethylationCounter(None, 0, reference=ref)
    mp.set_bam_sorter(sorter); mp.set_coverage(cov); mp.set_snp(snp); mp.set_count(cnt); mp.set_methyl(met)
    mark()
    _, stats = mp.map_sam(rows, quals, names, paired=True, bam=True)
    mark()
    assert stats[0] == N_READS
    sorter.finish(1)
    mark()
    assert b"".join(sorter.members())[:4] == b"\x1f\x8b\x08\x04" and sorter.stats()["records"] == stats[2]
    cov.finish(); snp.finish(); cnt.finish(); met.finish()
    mark()
    assert b"".join(cov.pieces()) and b"".join(snp.pieces()) and b"".join(met.pieces()) and cnt.read().shape == (1, 6)
    assert cov.stats()["alignments"] == snp.stats()["alignments"] == cnt.stats()["alignments"] == met.stats()["alignments"] > 0
    mark()
    # ... and a compressor of its own, both ways
    bz = P.Bgzf(0)
    assert bz.decompress(bz.compress(bytes(genome))) == bytes(genome)
    mark()
    for o in (mp, argos, sorter, cov, snp, cnt, met, bz, ref):
        o.close()
    return seen


@pytest.fixture(scope="module")
def first_cycle(world):
    base = P.live_memory()
    held = _cycle(world)
    return base, held, P.live_memory()


def test_everything_comes_back(first_cycle):
    base, seen, after = first_cycle
    assert seen[-1][0] > base["device_bytes"] and seen[-1][1] > base["pinned_bytes"]
    assert _bytes(after) == _bytes(base)


def test_a_second_cycle_holds_the_same(world, first_cycle):
    """live bytes behind every step of the cycle, and so their peak, are those of the first cycle"""
    base, seen, _ = first_cycle
    again = _cycle(world)
    assert again == seen and max(again) == max(seen)
    assert _bytes(P.live_memory()) == _bytes(base)


@pytest.mark.parametrize("call", ["map_se", "map_pe", "map_sam"])
def test_steady_state_allocates_nothing(world, call):
    base = P.live_memory()
    ref = P.Reference.from_contigs([world["genome"]])
    mp = P.Mapper(ref, Q, CORRIDOR)
    run = {"map_se": lambda: mp.map_se(world["rows"]), "map_pe": lambda: mp.map_pe(world["rows"]),
           "map_sam": lambda: mp.map_sam(world["rows"], world["quals"], world["names"], paired=True)}[call]
    run()
    run()
    after_two = P.live_memory()
    run()
    after_three = P.live_memory()
    print(call, "allocations of the third call:", [b - a for a, b in zip(_calls(after_two), _calls(after_three))])
    assert _calls(after_three) == _calls(after_two) and _bytes(after_three) == _bytes(after_two)
    mp.close(); ref.close()
    assert _bytes(P.live_memory()) == _bytes(base)


def test_resident_reads_are_borrowed(world):
    import torch
    base = P.live_memory()
    rows = world["rows"]
    ref = P.Reference.from_contigs([world["genome"]])
    fresh = P.Mapper(ref, Q, CORRIDOR)
    want = fresh.map_pe_raw(rows)
    fresh.close()
    assert int(want[0]["mapped"].sum()) >= N_READS - 8
    d_rows = torch.from_numpy(rows.copy()).to("cuda:0")
    torch.cuda.synchronize()
    mp = P.Mapper(ref, Q, CORRIDOR)
    for d in (d_rows, None, d_rows):   # the caller's device rows, the mapper's own upload, the caller's rows again
        got = mp.map_pe_raw(rows, d)
        for g, x in zip(got, want):
            assert g.tobytes() == x.tobytes()
    mp.close(); ref.close()
    torch.cuda.synchronize()
    assert np.array_equal(d_rows.cpu().numpy(), rows)   # still the caller's, still alive, untouched
    assert _bytes(P.live_memory()) == _bytes(base)


def test_debug_entries_free_what_they_take(world):
    from test_gpu_sam_records import marshal
    lib = P._lib()
    lib.ngm_debug_select_top1.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 2 + [C.c_uint64] + [C.c_void_p] * 7
    lib.ngm_debug_expand_pairs.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    lib.ngm_debug_pair_select.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float] + [C.c_void_p] * 6
    base = P.live_memory()
    # 2 reads (one pair), 3 candidates: read 0 owns two, read 1 one
    b, cnt = np.array([0, 2], np.uint32), np.array([2, 1], np.uint32)
    scores, loc, sv = np.array([50, 90, 70], np.float32), np.array([1000, 3000, 3200], np.uint32), np.array([4, 6, 9], np.uint32)
    win, mq, nb, best = np.zeros(2, np.uint32), np.zeros(2, np.int32), np.zeros(2, np.int32), np.zeros(2, np.float32)
    top1 = lambda n: lib.ngm_debug_select_top1(0, n, b.ctypes.data, cnt.ctypes.data, 3, scores.ctypes.data, loc.ctypes.data, sv.ctypes.data, win.ctypes.data, mq.ctypes.data,
                                               nb.ctypes.data, best.ctypes.data)
    assert top1(2) == 0, lib.ngm_pipeline_last_error()
    assert list(win) == [1, 2] and list(best) == [90, 70]
    assert _bytes(P.live_memory()) == _bytes(base)
    assert top1(0) == -22                      # (no reads: refused before anything is taken)
    assert _bytes(P.live_memory()) == _bytes(base)
    out = np.zeros(3, np.uint32)
    assert lib.ngm_debug_expand_pairs(0, 2, b.ctypes.data, cnt.ctypes.data, 3, out.ctypes.data) == 0, lib.ngm_pipeline_last_error()
    assert list(out) == [0, 0, 1]
    assert _bytes(P.live_memory()) == _bytes(base)
    rl = np.array([100, 100], np.uint16)
    info, counts, entries, tops = np.zeros(1, np.int32), np.zeros(4, np.uint32), np.zeros((4, 8), np.int32), np.zeros((2, 3, 8), np.int32)
    pair = lambda n_cand: lib.ngm_debug_pair_select(0, 1, b.ctypes.data, cnt.ctypes.data, n_cand, scores.ctypes.data, loc.ctypes.data, rl.ctypes.data, 0, 1000, 0.9, info.ctypes.data,
                                                    mq.ctypes.data, nb.ctypes.data, counts.ctypes.data, entries.ctypes.data, tops.ctypes.data)
    assert pair(3) == 0, lib.ngm_pipeline_last_error()
    assert int(counts[1]) + int(counts[2]) == 1   # a pair with choices: listed once, for one of the choice kernels
    assert _bytes(P.live_memory()) == _bytes(base)
    assert pair(2) == -22                      # (read 1 owns a candidate beyond n_cand: refused before anything is taken)
    assert _bytes(P.live_memory()) == _bytes(base)
    batch = SC.Batch({"slam_seq": 0}, [SC.rec("ok", "ACGTACGTAC", "IIIIIIIIII", SC.hit(pos=2)), SC.rec("other", "ACGTACGTAC", "", SC.hit(pos=5, reverse=1, qstart=2, cigar="2S8M"))])
    text, counters = P.debug_sam_records(**marshal(batch, False))
    assert text.count(b"\n") == 2 and counters[0] == 2
    assert _bytes(P.live_memory()) == _bytes(base)
    # the two hooks that work on an engine's / a mapper's own workspace: what they take besides comes back with the call, the rest with the object
    import nextgenmap_amd as N
    from nextgenmap_amd import engine as E
    from pairgen import make_pairs
    pref, pqry = make_pairs(70, Q, CORRIDOR, seed=3, read_len=READ_LEN)
    eng = N.Engine(Q, CORRIDOR)
    assert len(eng.BatchAlign(0, pref, pqry, device_strings=True)) == 70 and int(eng.last_built_by.sum()) > 35
    held = _bytes(P.live_memory())
    eng.BatchAlign(0, pref, pqry, device_strings=True)
    assert _bytes(P.live_memory()) == held
    eng.close()
    assert _bytes(P.live_memory()) == _bytes(base)
    aff = N.Engine(Q, CORRIDOR, personality=E.PERSONALITY_AFFINE, gap_read=33, gap_ref=33, gap_extend=3)
    held = _bytes(P.live_memory())
    with pytest.raises(E.NgmHipError):          # (an affine engine: refused before anything is taken)
        aff.BatchAlign(0, pref, pqry, device_strings=True)
    assert _bytes(P.live_memory()) == held
    aff.close()
    assert _bytes(P.live_memory()) == _bytes(base)
    ref = P.Reference.from_contigs([world["genome"]])
    mp = P.Mapper(ref, Q, CORRIDOR)
    pr, pl, ps = np.arange(70, dtype=np.uint32) % N_READS, np.arange(1000, 1070, dtype=np.uint32), np.arange(70, dtype=np.uint32) & 1
    words, lens, _, rw, fw = mp.debug_gather_pairs(world["rows"], pr, pl, ps)
    assert words.shape == (2, rw + fw, 64) and list(lens) == [READ_LEN] * 70
    mp.debug_gather_pairs(world["rows"], pr, pl, ps)   # (the mapper's own buffers are final from the second batch on, as in test_steady_state_allocates_nothing)
    held = _bytes(P.live_memory())
    mp.debug_gather_pairs(world["rows"], pr, pl, ps, align_stage=True)
    assert _bytes(P.live_memory()) == held
    with pytest.raises(P.NgmHipError):          # (a pair of a read that is not there: refused before anything is taken)
        mp.debug_gather_pairs(world["rows"], pr + N_READS, pl, ps)
    assert _bytes(P.live_memory()) == held
    mp.close(); ref.close()
    assert _bytes(P.live_memory()) == _bytes(base)
