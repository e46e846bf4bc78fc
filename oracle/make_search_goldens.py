#!/usr/bin/env python3
"""Recorded candidate-search results of the REAL reference program for the configurations of tests/cs_worlds.py -> tests/golden/search/.

For every configuration: genome and reads from the fixed seeds, one run of oracle/_ref/ngm/ngm-core-debug (built by oracle/ngm_ref.mk)
with the per-read CS log switched on, and -- there and then -- the plain model of tests/cs_model.py held against it: the index against
the reference's own <ref>-ht-<k>-<skip>.3.ngm file, the automatic max_kfreq against the logged one, every read's candidate set, maximum,
threshold and accepted count against the log.  Only when all of that agrees is the configuration's .npz written.  Runs on the CPU;
tests/test_cs_model.py then needs neither the reference binary nor a GPU.  (--max-cmrs is not visible in that log -- it is written
before the rule applies --, so those configurations share the golden of the defaults; oracle/make_search_cli_goldens.py pins the rule.)"""
import io
import json
import os
import re
import sys
import tempfile
import time
import zipfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import cs_model as CM  # noqa: E402
import cs_worlds as W  # noqa: E402
import ref_files as RF  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "search")
RESULT = re.compile(r"8192\tREAD_(\d+)\tCS_RESULTS\tInternal location: (\d+) \(([+-])\).*Score: ([0-9.]+) \(ACCEPT\)")
SUMMARY = re.compile(r"8\tREAD_(\d+)\tCS\tSummary: (\d+) CMRs \((\d+) without filter\), (\d+) accepted, theta: ([0-9.]+), max: ([0-9.]+)")


def save_npz(path, arrays):
    """np.load reads it; the same arrays give the same bytes (no time stamps)"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[name]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


def one(cfg):
    t0 = time.time()
    reads, file_reads = W.reads_of(cfg.id), W.file_reads_of(cfg.id)
    fasta, fastq = W.fasta_bytes(W.genome(cfg.world)), W.fastq_bytes(file_reads)
    idx = W.index_of(cfg.k, cfg.skip, cfg.bins, cfg.world)
    with tempfile.TemporaryDirectory() as d:
        fa, fq = os.path.join(d, "ref.fa"), os.path.join(d, "reads.fq")
        with open(fa, "wb") as f:
            f.write(fasta)
        with open(fq, "wb") as f:
            f.write(fastq)
        r = RF.run_ngm(["-r", fa, "-q", fq, "-o", os.path.join(d, "out.sam"), "--affine", "-t", "1", "--no-progress", "--log", "--log-lvl", "8200"] + W.ngm_options(cfg),
                       debug=True, cwd=d)
        text = r.stdout + r.stderr
        assert "Done" in text, text[-3000:]
        ht = RF.read_ht_file(fa + "-ht-%d-%d.3.ngm" % (cfg.k, cfg.skip))
    # the index
    nz = np.flatnonzero(ht["raw_counts"])
    assert np.array_equal(nz.astype(np.uint64), idx.kmers), "k-mers of the index"
    assert np.array_equal(ht["raw_counts"][nz], idx.raw), "raw_counts"
    assert np.array_equal(ht["counts"][nz] > 0, idx.used) and not np.any(ht["counts"][ht["raw_counts"] == 0]), "counts"
    assert np.array_equal(ht["positions"], idx.positions), "positions"
    logged_kfreq = -1
    if not cfg.kfreq:
        m = re.search(r"Max\. k-mer frequency set so (\d+)", text)
        logged_kfreq = int(m.group(1))
        assert logged_kfreq == CM.auto_max_kfreq(idx), (logged_kfreq, CM.auto_max_kfreq(idx))
    # the search
    want, summ = {}, {}
    for line in r.stdout.splitlines():
        m = RESULT.match(line)
        if m:
            want.setdefault(int(m.group(1)), []).append((int(m.group(2)), 0 if m.group(3) == "+" else 1, int(float(m.group(4)))))
            continue
        m = SUMMARY.match(line)
        if m:
            summ[int(m.group(1))] = (int(m.group(4)), m.group(5), float(m.group(6)))
    assert len(summ) == len(reads), (len(summ), len(reads))
    kw = W.params(cfg, max_cmrs=W.UNLIMITED)
    offs, cands, maxes, thetas = [0], [], [], []
    bad = 0
    for i, (name, seq) in enumerate(reads):
        got = CM.search(seq.tobytes(), **kw)
        exp = sorted((CM.resolve_bin(b, cfg.bins), s, v) for b, s, v in want.get(i, []))
        acc, theta, mx = summ[i]
        if [tuple(x) for x in got.cands.tolist()] != exp or got.max_votes != mx or got.accepted != acc or "%f" % got.threshold != theta:
            bad += 1
            if bad < 6:
                print("  read", i, name, "model", got.cands.tolist()[:5], got.max_votes, "%f" % got.threshold, got.accepted, "reference", exp[:5], mx, theta, acc)
        cands.extend(exp)
        offs.append(len(cands))
        maxes.append(mx)
        thetas.append(float(theta))
    assert bad == 0, "%s: the model differs from the reference on %d of %d reads" % (cfg.id, bad, len(reads))
    counts_sha, positions_sha = CM.index_digests(idx)
    save_npz(os.path.join(OUT, cfg.id + ".npz"), dict(
        options=np.frombuffer(json.dumps(dict(cfg._asdict(), ngm=W.ngm_options(cfg)), sort_keys=True).encode(), np.uint8),
        seeds=np.array([W.GENOME_SEED], np.int64), fasta_sha256=np.frombuffer(W.sha256(fasta).encode(), np.uint8),
        fastq_sha256=np.frombuffer(W.sha256(fastq).encode(), np.uint8), counts_sha256=np.frombuffer(counts_sha.encode(), np.uint8),
        positions_sha256=np.frombuffer(positions_sha.encode(), np.uint8), max_kfreq=np.array([logged_kfreq], np.int64),
        offsets=np.array(offs, np.int32), cands=np.array(cands, np.int64).reshape(-1, 3), max=np.array(maxes, np.float32), theta=np.array(thetas, np.float64)))
    print("%-24s %5d reads, %6d candidates, max_kfreq %5d, %6d bytes, %.1f s" % (cfg.id, len(reads), len(cands), logged_kfreq,
                                                                               os.path.getsize(os.path.join(OUT, cfg.id + ".npz")), time.time() - t0))


def main():
    assert RF.have_reference_binary(), "build the reference first: make -f oracle/ngm_ref.mk"
    os.makedirs(OUT, exist_ok=True)
    only = sys.argv[1:]
    for cid in W.GOLDEN_IDS:
        if not only or cid in only:
            one(W.BY_ID[cid])


if __name__ == "__main__":
    main()
