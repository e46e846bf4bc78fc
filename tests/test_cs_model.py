"""The plain model of the candidate search (tests/cs_model.py) against the results recorded from the REAL reference program
(tests/golden/search/, written by oracle/make_search_goldens.py): no GPU, no reference binary.  Inputs are regenerated from the seeds and
their digests checked; then every read's candidate set, vote counts, maximum and threshold, the index digests and the automatic max_kfreq
must equal what the reference program logged.  The second half counts, from the model alone, that the read sets reach the edges
tests/test_gpu_cs_shapes.py relies on."""
import json
import os

import numpy as np
import pytest

import cs_model as CM
import cs_worlds as W

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "search")


def _text(a):
    return bytes(a).decode()


@pytest.mark.parametrize("cid", W.GOLDEN_IDS)
def test_model_equals_the_recorded_reference_results(cid):
    cfg = W.BY_ID[cid]
    z = np.load(os.path.join(GOLDEN, cid + ".npz"))
    opts = json.loads(_text(z["options"]))
    assert opts["ngm"] == W.ngm_options(cfg) and int(z["seeds"][0]) == W.GENOME_SEED
    assert W.sha256(W.fasta_bytes(W.genome(cfg.world))) == _text(z["fasta_sha256"])
    assert W.sha256(W.fastq_bytes(W.file_reads_of(cid))) == _text(z["fastq_sha256"])
    idx = W.index_of(cfg.k, cfg.skip, cfg.bins, cfg.world)
    assert CM.index_digests(idx) == (_text(z["counts_sha256"]), _text(z["positions_sha256"]))
    if not cfg.kfreq:
        assert CM.auto_max_kfreq(idx) == int(z["max_kfreq"][0])
    reads, res = W.reads_of(cid), W.results_of(cid)
    offs, cands = z["offsets"], z["cands"]
    assert len(offs) == len(reads) + 1
    bad = []
    for i, r in enumerate(res):
        want = cands[offs[i]:offs[i + 1]]
        if not (np.array_equal(r.cands, want) and r.max_votes == z["max"][i] and float("%f" % r.threshold) == z["theta"][i] and r.accepted == len(want)):
            bad.append((i, reads[i][0]))
    assert not bad, "%d reads differ from the reference program: %s" % (len(bad), bad[:8])


def test_reverse_complement_and_walk_on_small_cases():
    v = np.array([0b000110, 0b111111], np.uint64)            # ACT -> AGT (T2 A0... A0 C1 T2 reversed and complemented), GGG -> CCC
    assert CM.revcomp_kmer(v, 3).tolist() == [0b001110, 0b010101]
    codes = CM.CODE[np.frombuffer(b"NNACGTACGTNACGNNACGTAC", np.uint8)]
    assert CM.kmer_starts(codes, 4, 0).tolist() == [2, 3, 4, 5, 6, 16, 17, 18]      # ACG is too short; NN ACGTAC has 6 > 4 bases left
    assert CM.kmer_starts(codes, 4, 2).tolist() == [2, 5, 16]
    assert CM.kmer_starts(CM.CODE[np.frombuffer(b"NNACGTA", np.uint8)], 4, 0).tolist() == [2, 3]   # 2 < 7 - 4
    assert CM.kmer_starts(CM.CODE[np.frombuffer(b"NNNACGT", np.uint8)], 4, 0).tolist() == []       # 3 >= 7 - 4: the read is dropped
    assert CM.kmer_starts(CM.CODE[np.frombuffer(b"ACGTANNACGT", np.uint8)], 4, 0).tolist() == [0, 1]  # behind NN: 1 >= 5 - 4, dropped
    assert CM.kmer_starts(CM.CODE[np.frombuffer(b"ACGTANACGT", np.uint8)], 4, 0).tolist() == [0, 1, 6]  # behind one N: exactly k bases count


@pytest.mark.parametrize("cid", [c.id for c in W.CONFIGS])
def test_read_sets_reach_the_edges(cid):
    cfg, c = W.BY_ID[cid], W.census(cid)
    print(cid, c)
    names = [n.split("_", 1)[1] for n, _ in W.reads_of(cid) if n.startswith("e")]
    for tag in ("len-%d" % (cfg.k - 1), "len-%d" % cfg.k, "len-%d" % (cfg.k + 1), "all-n", "lead-n-%d" % (cfg.read_len - cfg.k - 1), "lead-n-%d" % (cfg.read_len - cfg.k),
                "lead-n-%d" % (cfg.read_len - cfg.k + 1), "n-every-k", "n-last", "len-q-1", "spacer", "ac", "homopolymer"):
        assert tag in names
    lens = {n.split("_", 1)[1]: len(s) for n, s in W.reads_of(cid) if n.startswith("e")}
    assert lens["len-q-1"] == W.qlen(cfg) - 1 and lens["len-q+5"] == W.qlen(cfg) - 1
    # reads without any k-mer: shorter than k, all N, a leading N run of len - k and of len - k + 1, an N at every k-th base
    assert c["no_kmers"] >= 5
    # The fast path certifies a read only when its threshold exceeds one vote: reads WITH hits and a float32 threshold <= 1 are the ones
    # searched again (reads without a hit have threshold 0 and never leave the fast path, so they do not count here).  kmer_min > 1
    # keeps every threshold above 1: thresholds-s0-kmin2 and thresholds-s09-kmin40 cannot hold such a read.
    if cfg.kmin <= 1.0:
        assert c["hits_thr_le_1"] >= 10
    else:
        assert c["hits_thr_le_1"] == 0 and c["thr_le_1"] == 0
    if cfg.k >= 11:   # (below that, random sequence hits the genome: no read with a maximum of exactly 2 or 3 can be built)
        if cfg.s == 0.5 and cfg.kmin <= 1.0:
            assert c["thr_eq_1"] >= 1 and c["thr_below_1"] >= 1          # maximum 2 and 1
        if cfg.s == 0.34:
            assert c["thr_above_1"] >= 1 and c["thr_below_1"] >= 1       # maximum 3: 1.02, maximum 2: 0.68
    if cfg.kmin < 40:
        assert c["strand_tie"] >= 1      # a read centred on the region that is its own reverse complement
    # a bin that both strands vote for and only one of them reaches the threshold: the read centred on the 20-base self-complementary
    # stretch.  Not with kmer_min above 1: at -s 0 --kmer-min 2 the two or three reverse votes of that stretch reach the threshold of 2
    # as well, and at --kmer-min 40 no 100-base read with k-mers on every third position has a bin with 40 votes but the AC repeat's.
    if cfg.kmin <= 1.0:
        assert c["one_strand"] >= 1
    # an accepted (bin, strand) that only several k-mers of a repeat carry to the threshold (reads from the repeat families)
    assert c["repeat_bin"] >= 1
    if cid == "kfreq-low":
        assert c["kfreq_minus_1"] >= 1 and c["kfreq"] >= 1 and c["kfreq_plus_1"] >= 1
    if cid.startswith("max-cmrs"):
        assert c["cmrs_minus_1"] >= 1 and c["cmrs"] >= 1 and c["cmrs_plus_1"] >= 1
    if cid.startswith("skip-") or cid == "k-9-skip-0":
        assert c["list_w_minus_2"] >= 1 and c["list_w_minus_1"] >= 1 and c["list_w"] >= 1 and c["list_long"] >= 1
    if cid == "k-9-skip-0":
        assert c["bucket_words"] == 16
    if cfg.k % 2 == 0:
        assert c["palindromes"] >= 1
    if cid == "votes-256":
        assert c["votes_gt_255"] >= 1
    if cid == "votes-max":
        # the issue's recipe (300 bases against 700, --kmer-skip 0 --bin-size 8): the reference stores a homopolymer's k-mer once per bin,
        # so an AC repeat is the densest an index gets -- 128 hits per k-mer and 256-base bin, 288 k-mers: 36 864 at the most, which the
        # 16-bit halves of a vote table hold.  More than 65 535 takes longer reads: votes-64k
        assert 30000 < c["max_votes"] <= 36864 and c["votes_gt_65535"] == 0
    if cid == "votes-64k":
        # 600 bases of AC against 1 900: 588 k-mers x 128 = 75 264 votes in one (bin, strand).  The recorded reference result holds that
        # count (test_model_equals_the_recorded_reference_results); the product refuses this combination (W.REFUSED)
        assert c["votes_gt_65535"] >= 1 and c["max_votes"] == 588 * 128
    assert (c["votes_gt_65535"] > 0) == (cid in W.REFUSED)

