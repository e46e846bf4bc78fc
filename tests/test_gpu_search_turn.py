"""-m gpu: the search + score turn of a mapper (csrc/mapper_search.cpp run_cs, csrc/mapper.cpp begin + search_and_score).

By default the per-read arrays of a search -- candidate offsets, counts, best votes -- travel to the host behind the score stage's last
kernel, outside the turn (cs_enqueue_host_arrays / cs_host_arrays), and the score stage's buffers are reserved in front of the search
for a predicted candidate count.  NGM_HIP_CS_EAGER_ARRAYS=1, read when a mapper is created, keeps the arrays in front of the search's
one synchronisation.  Every case maps the same batches with a mapper of each kind: hits, CIGAR and MD buffers must be byte-equal,
paired-end and single-end.  Mapper.search_turn_counters() (ngm_mapper_search_turn_counters) says what the last call did.

Genome: 300 kbp with one repeat family (600 bp, 24 copies, 1 % divergence): a read from a copy has some 24 candidates, more than the four
slots a read owns, so its candidates go through the shared regions whose overflow NGM_HIP_TEST_LIMITS=cs_cap=N forces."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import simulate as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q, C = 152, 27
KW = dict(sensitivity=0.5, gap_read=33, gap_ref=33, gap_extend=3, personality=1)
FAM_LEN, COPIES, SPACING = 600, 24, 12000


@functools.lru_cache(maxsize=None)
def _genome():
    rng = np.random.default_rng(1101)
    g = S.ACGT[rng.integers(0, 4, 300_000)].copy()
    fam = S.ACGT[rng.integers(0, 4, FAM_LEN)]
    for i in range(COPIES):
        c = fam.copy()
        m = rng.random(FAM_LEN) < 0.01
        c[m] = S.ACGT[rng.integers(0, 4, int(m.sum()))]
        g[1000 + i * SPACING:1000 + i * SPACING + FAM_LEN] = c
    return g


@functools.lru_cache(maxsize=None)
def _reference():
    from nextgenmap_amd.pipeline import Reference
    return Reference.from_contigs([_genome()])


def _rows(seqs):
    from nextgenmap_amd.pipeline import Mapper
    return Mapper.reads_to_rows(seqs, Q)


def unique_rows(n, seed, paired=True):
    """n reads (n / 2 pairs, mates interleaved) drawn uniformly from the genome"""
    if paired:
        r1, r2 = S.make_reads([_genome()], n // 2, 150, seed=seed, paired=True)
        return _rows([s for a, b in zip(r1, r2) for s in (a[1], b[1])])
    return _rows([s for _, s, _ in S.make_reads([_genome()], n, 150, seed=seed)])


def repeat_rows(n, seed):
    """n reads (pairs, interleaved) whose fragments lie inside copies of the repeat family"""
    rng = np.random.default_rng(seed)
    g, out = _genome(), []
    for _ in range(n // 2):
        p = 1000 + int(rng.integers(0, COPIES)) * SPACING + int(rng.integers(0, FAM_LEN - 350))
        frag = g[p:p + 350]
        out += [frag[:150], S.revcomp(frag)[:150]]
    return _rows(out)


def mapper(eager):
    """a mapper of either kind: the switch is read when the mapper is created"""
    from nextgenmap_amd.pipeline import Mapper
    old = os.environ.pop("NGM_HIP_CS_EAGER_ARRAYS", None)
    try:
        if eager:
            os.environ["NGM_HIP_CS_EAGER_ARRAYS"] = "1"
        return Mapper(_reference(), Q, C, **KW)
    finally:
        os.environ.pop("NGM_HIP_CS_EAGER_ARRAYS", None)
        if old is not None:
            os.environ["NGM_HIP_CS_EAGER_ARRAYS"] = old


def run(mp, rows, paired):
    """-> (hits, cigar, md) as bytes, counters of the call"""
    hits, cig, md = mp.map_pe_raw(rows) if paired else mp.map_se_raw(rows)
    return (hits.tobytes(), cig.tobytes(), md.tobytes()), mp.search_turn_counters(), hits


def both(batches, paired):
    """the batches on a default and on an eager mapper: outputs byte-equal; -> per batch (outputs, default counters, hits)"""
    d, e = mapper(False), mapper(True)
    res = []
    try:
        for k, rows in enumerate(batches):
            od, cd, hits = run(d, rows, paired)
            oe, ce, _ = run(e, rows, paired)
            assert cd["arrays_deferred"] == 1 and ce["arrays_deferred"] == 0, (k, cd, ce)
            for name, a, b in zip(("hits", "cigar", "md"), od, oe):
                assert a == b, "batch %d (%d reads, %s): %s differ between the default and the eager mapper" % (k, len(rows), "PE" if paired else "SE", name)
            res.append((od, cd, hits))
    finally:
        d.close(); e.close()
    return res


PAIRED = pytest.mark.parametrize("paired", [True, False], ids=["pe", "se"])


@PAIRED
def test_one_pair(paired):
    (_, ctr, hits), = both([unique_rows(2, 21)], paired)
    assert ctr["search_attempts"] == 1
    assert hits["mapped"].all()


@PAIRED
@pytest.mark.parametrize("n", [63, 64, 65])
def test_block_edges(n, paired):
    if paired:
        n *= 2   # a paired batch holds whole pairs: 63, 64 and 65 pairs (126, 128, 130 reads, around two blocks of 64)
    (_, _, hits), = both([unique_rows(n, 30 + n, paired)], paired)
    assert len(hits) == n and hits["mapped"].mean() > 0.9


@PAIRED
def test_no_candidates(paired):
    """np = 0: the branch that reads the host arrays right after the search"""
    rows = _rows([b"N" * 150] * 66)
    (_, ctr, hits), = both([rows], paired)
    assert not hits["mapped"].any() and (hits["n_candidates"] == 0).all()
    assert ctr["buffers_regrown"] == 0


@PAIRED
def test_prediction_too_small_then_too_large(paired):
    """unique reads, then reads of the repeat family (several times the candidates: the buffers reserved in front of the search for 5/4
    of the first batch's count are too small and grow inside the turn), then unique reads again (the prediction is now far too large:
    nothing grows)"""
    batches = [unique_rows(400, 41, paired), repeat_rows(400, 42), unique_rows(400, 43, paired)]
    res = both(batches, paired)
    cands = [int(h["n_candidates"].sum()) for _, _, h in res]
    assert cands[1] > 3 * cands[0] and cands[1] > 3 * cands[2], cands   # (a twentieth of the uniform reads fall into copies, too)
    assert res[1][1]["buffers_regrown"] >= 1, res[1][1]
    assert res[2][1]["buffers_regrown"] == 0, res[2][1]
    assert all(c["search_attempts"] == 1 for _, c, _ in res)


def test_arrays_outside_the_map_calls():
    """Mapper.candidate_search (ngm_mapper_cs + ngm_mapper_cs_fetch) right after creation: its host arrays are complete on return --
    offsets, best votes and candidates equal the eager mapper's, and the offsets are the counts the map call reports"""
    rows = np.concatenate([unique_rows(130, 51), repeat_rows(20, 52)])
    d, e = mapper(False), mapper(True)
    try:
        got, want = d.candidate_search(rows), e.candidate_search(rows)
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and np.array_equal(a, b)
        offs = got[0]
        assert offs[-1] > len(rows) and len(got[2]) == offs[-1]
        hits, _, _ = d.map_se_raw(rows)
        assert np.array_equal(np.diff(offs.astype(np.int64)), hits["n_candidates"])
        assert np.array_equal(got[1], hits["max_votes"])
        again = d.candidate_search(rows)   # ... and after a map call that deferred them
        for a, b in zip(again, want):
            assert np.array_equal(a, b)
    finally:
        d.close(); e.close()


# ---- forced overflow: NGM_HIP_TEST_LIMITS is read once per process, so the forced run is a child process ---------------------------
def _overflow_run():
    """the overflow batch, paired-end and single-end, on a fresh default mapper each; -> outputs as byte arrays, counters"""
    arrays, counters = {}, {}
    rows = np.concatenate([repeat_rows(200, 61), unique_rows(100, 62)])
    for paired in (True, False):
        mp = mapper(False)
        try:
            (h, c, m), ctr, _ = run(mp, rows, paired)
        finally:
            mp.close()
        tag = "pe" if paired else "se"
        arrays.update({tag + "_hits": np.frombuffer(h, np.uint8), tag + "_cigar": np.frombuffer(c, np.uint8), tag + "_md": np.frombuffer(m, np.uint8)})
        counters[tag] = ctr
    return arrays, counters


def test_forced_overflow(tmp_path):
    """cs_cap=256: one slot per candidate region at first, so the reads of the repeat family (some 24 candidates each, a region of
    their own each) overflow and the batch is searched again with four times the room until it fits; the outputs equal the unforced
    run's (this process: 68 slots per region from the start)"""
    assert "cs_cap" not in os.environ.get("NGM_HIP_TEST_LIMITS", "")
    plain, ctr_plain = _overflow_run()
    out = str(tmp_path / "forced")
    env = dict(os.environ, NGM_HIP_TEST_LIMITS="cs_cap=256")
    env.pop("NGM_HIP_CS_EAGER_ARRAYS", None)
    env["PYTHONPATH"] = os.pathsep.join([ROOT] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    c = subprocess.run([sys.executable, os.path.abspath(__file__), out], capture_output=True, text=True, env=env, timeout=120)
    assert c.returncode == 0, c.stderr[-2000:]
    forced, ctr_forced = np.load(out + ".npz"), json.load(open(out + ".json"))
    for tag in ("pe", "se"):
        assert ctr_plain[tag]["search_attempts"] == 1, ctr_plain
        assert ctr_forced[tag]["search_attempts"] > 1, ctr_forced
        assert ctr_forced[tag]["arrays_deferred"] == 1
    assert sorted(plain) == sorted(forced.files) and len(plain) == 6
    for k in plain:
        assert np.array_equal(plain[k], forced[k]), k


if __name__ == "__main__":   # the child of test_forced_overflow
    _arrays, _counters = _overflow_run()
    np.savez(sys.argv[1] + ".npz", **_arrays)
    with open(sys.argv[1] + ".json", "w") as _f:
        json.dump(_counters, _f)
