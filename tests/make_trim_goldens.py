"""Writes tests/golden/trim/: the fixtures of `-5/--trim5` and `--max-polya` and what the reference program (oracle/_ref/ngm/ngm-core,
built by oracle/ngm_ref.mk) writes for them with `--affine -t 1 -5 12 --max-polya 4`, as SAM and as `-b` BAM.
  se.fq.gz                 ~300 single-end reads of 100 bp behind a 12 bp adapter: poly-A tails of 0, 3, 4, 5, 8 and 30 bases, and the
                           edge cases of EDGE_NAMES below
  pe.fq.gz                 ~200 interleaved pairs, both mates behind the adapter: tails on mate 1, one mate 1 that is all A, one mate 2
                           shorter than the adapter
  se.sam.gz / se.bam       the reference's records for se.fq      pe.sam.gz / pe.bam    ... for pe.fq (-p)
The genome is simulate.make_genome(GENOME) -- the tests write the same FASTA, none is committed.  The module is also the tests' helper
(write_reference, record readers).  Run from the repository root: python tests/make_trim_goldens.py"""
import gzip
import os
import shutil
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_files as RF  # noqa: E402
import simulate as S  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trim")
GENOME = [120000, 80001]
ADAPTER = b"ACGTTGCAACGT"
TRIM = ["-5", "12", "--max-polya", "4"]
TAILS = (0, 3, 4, 5, 8, 30)
EDGE_NAMES = ("tail_n", "tail_lower", "all_a", "left5", "left13", "left14", "short", "exact", "long")


def write_reference(path):
    S.write_fasta(path, S.make_genome(GENOME))


def _qual(n, salt):
    # a different character at every position, so that a shifted or mirrored quality string shows ('0' .. 'T': a string that starts with
    # '*' is "no quality" to the reference's writers, SAMWriter.cpp:122)
    return bytes(48 + (7 * i + salt) % 37 for i in range(n))


def _with_tail(seq, t):
    s = seq.copy()
    if t:
        s[len(s) - t:] = ord("A")
    return s


def _prefixed(name, body, salt):
    seq = np.concatenate([np.frombuffer(ADAPTER, np.uint8), np.asarray(body, np.uint8)])
    return name, seq, _qual(len(seq), salt)


def se_reads():
    contigs = S.make_genome(GENOME)
    base = S.make_reads(contigs, 296, 100, seed=4101, sub_rate=0.01, indel_rate=0.002)
    reads = [_prefixed(name, _with_tail(seq, TAILS[i % len(TAILS)]), i) for i, (name, seq, _) in enumerate(base)]
    g = contigs[0]
    arr = lambda b: np.frombuffer(b, np.uint8)
    a = lambda n: np.full(n, ord("A"), np.uint8)

    def not_a(seq):   # the base in front of a tail is not an A, so the count is the tail's
        s = seq.copy()
        if s[-1] == ord("A"):
            s[-1] = ord("C")
        return s
    edge = {
        "tail_n": np.concatenate([not_a(g[5000:5089]), a(4), arr(b"N"), a(6)]),          # the N ends the tail: 6 cut, the read ends in N
        "tail_lower": np.concatenate([not_a(g[7000:7090]), arr(b"a" * 10)]),              # the parser upper-cases first
        "all_a": a(100),                                                                 # length 0 after trimming: written, not discarded
        "left5": np.concatenate([arr(b"CGTAC"), a(60)]),
        "left13": np.concatenate([not_a(g[9000:9013]), a(40)]),                           # exactly one k-mer left
        "left14": np.concatenate([not_a(g[11000:11014]), a(40)]),
        "long": np.concatenate([np.full(1010, ord("N"), np.uint8), a(78)]),               # cut at qry_max_len - 1 = 999: its tail never reaches --max-polya
    }
    for k in ("tail_n", "tail_lower", "all_a", "left5", "left13", "left14"):
        reads.append(_prefixed(k, edge[k], len(reads)))
    reads.append(("short", arr(b"ACGTTGCA"), _qual(8, 3)))                                # shorter than -5: discarded
    reads.append(("exact", arr(ADAPTER), _qual(12, 4)))                                   # exactly -5 bases: discarded
    reads.append(_prefixed("long", edge["long"], 5))
    assert [r[0] for r in reads[-len(EDGE_NAMES):]] == list(EDGE_NAMES)
    return reads


def pe_reads():
    contigs = S.make_genome(GENOME)
    r1, r2 = S.make_reads(contigs, 200, 100, seed=4102, sub_rate=0.01, indel_rate=0.002, paired=True)
    out = []
    for i, ((n1, s1, _), (n2, s2, _)) in enumerate(zip(r1, r2)):
        s1 = _with_tail(s1, TAILS[i % len(TAILS)])
        if i == 5:
            s1 = np.full(100, ord("A"), np.uint8)
        m1, m2 = _prefixed(n1, s1, i), _prefixed(n2, s2, i + 1)
        if i == 9:
            m2 = (n2, np.frombuffer(b"ACGTTGC", np.uint8), _qual(7, 2))
        out += [m1, m2]
    return out


def write_fastq_gz(path, reads):
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        for name, seq, qual in reads:
            f.write(b"@" + name.encode() + b"\n" + bytes(seq) + b"\n+\n" + qual + b"\n")


def read_fastq_gz(path):
    lines = gzip.open(path, "rb").read().split(b"\n")
    return [(lines[i][1:].decode(), lines[i + 1], lines[i + 3]) for i in range(0, len(lines) - 1, 4)]


def sam_records(path):
    """-> {(name, flag & 0xC0): line}: one record per read and mate (the reference writes reads without candidates ahead of the others, its
    record order is not the input order)"""
    op = gzip.open if path.endswith(".gz") else open
    out = {}
    for l in op(path, "rt"):
        if not l.startswith("@"):
            f = l.split("\t", 2)
            assert (f[0], int(f[1]) & 0xC0) not in out
            out[(f[0], int(f[1]) & 0xC0)] = l
    return out


def bam_records(path):
    from test_gpu_bam import decode_bam
    text, refs, recs = decode_bam(path)
    out = {}
    for x in recs:
        assert (x["name"], x["flag"] & 0xC0) not in out
        out[(x["name"], x["flag"] & 0xC0)] = x
    return text, refs, out


def main():
    assert RF.have_reference_binary(), "build the reference program first (make -C oracle)"
    os.makedirs(GOLDEN, exist_ok=True)
    write_fastq_gz(os.path.join(GOLDEN, "se.fq.gz"), se_reads())
    write_fastq_gz(os.path.join(GOLDEN, "pe.fq.gz"), pe_reads())
    for tag, inp in (("se", ["-q"]), ("pe", ["-p", "-q"])):
        with tempfile.TemporaryDirectory() as d:
            fa, fq = os.path.join(d, "ref.fa"), os.path.join(d, tag + ".fq")
            write_reference(fa)
            with open(fq, "wb") as f:
                f.write(gzip.open(os.path.join(GOLDEN, tag + ".fq.gz"), "rb").read())
            for fmt, extra in (("sam", []), ("bam", ["-b"])):
                out = os.path.join(d, "out." + fmt)
                r = RF.run_ngm(["-r", fa, "-o", out, "--affine", "-t", "1", "--no-progress"] + TRIM + inp + [fq] + extra, cwd=d)
                log = r.stdout + r.stderr
                assert "Done" in log, log[-2000:]
                print(tag, fmt, [l.split("] ", 1)[-1] for l in log.splitlines() if "Average read length" in l or "Done" in l])
                if fmt == "sam":
                    with open(out, "rb") as f, gzip.GzipFile(os.path.join(GOLDEN, tag + ".sam.gz"), "wb", mtime=0) as z:
                        z.write(f.read())
                else:
                    shutil.copyfile(out, os.path.join(GOLDEN, tag + ".bam"))   # (BGZF: gzip members already)


if __name__ == "__main__":
    main()
