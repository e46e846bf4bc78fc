"""Writes tests/golden/bam_input/: SAM and BAM INPUT files and what the reference program (oracle/_ref/ngm/ngm-core, built by
oracle/ngm_ref.mk) writes for them with `--affine -t 1`.
  se.bam / se.sam.gz       ~300 single-end reads of 100 bp as unaligned records (flag 4); every fifth is stored as a reverse-strand record
                           (flag 20: sequence reverse-complemented, qualities reversed), which the parsers turn back into the read
  pe.bam / pe.sam.gz       ~150 interleaved pairs (flags 77 / 141), mates named name/1 and name/2
  <input>.out.sam.gz       the reference's records for `-q <input>` (`-p -q` for the pairs)
The BAM files are cut into BGZF members of 4 000 bytes, so that records straddle members.  The genome is that of make_trim_goldens
(simulate.make_genome) -- the tests write the same FASTA, none is committed.  The module is also the tests' helper (reads()).
Run from the repository root: python tests/make_bam_input_goldens.py"""
import gzip
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_fixtures as BF  # noqa: E402
import make_trim_goldens as TG  # noqa: E402
import ref_files as RF  # noqa: E402
import simulate as S  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bam_input")


def _qual(n, salt):
    return bytes(48 + (7 * i + salt) % 37 for i in range(n))   # (a different character at every position: a mirrored string shows)


def reads(paired):
    """[(name, seq, qual)] as bytes; pairs interleaved"""
    g = S.make_genome(TG.GENOME)
    if paired:
        r1, r2 = S.make_reads(g, 150, 100, seed=911, sub_rate=0.02, indel_rate=0.003, paired=True)
        return [(n.encode(), s.tobytes(), _qual(len(s), i)) for i, pair in enumerate(zip(r1, r2)) for n, s, _ in pair]
    return [(n.encode(), s.tobytes(), _qual(len(s), i)) for i, (n, s, _) in enumerate(S.make_reads(g, 300, 100, seed=912, sub_rate=0.02, indel_rate=0.003))]


def input_files(paired):
    """name -> bytes of the committed inputs"""
    rd = reads(paired)
    recs = []
    for i, (n, s, q) in enumerate(rd):
        flag = (77 if i % 2 == 0 else 141) if paired else 4
        if not paired and i % 5 == 0:
            flag, s, q = flag | 0x10, BF.revcomp(s), q[::-1]
        recs.append(BF.bam_record(n, s, q, flag))
    tag = "pe" if paired else "se"
    return {tag + ".bam": BF.bgzf(BF.bam_bytes(recs), 4000), tag + ".sam.gz": gzip.compress(BF.sam_text(rd, paired, 0 if paired else 5), mtime=0)}


def main():
    assert RF.have_reference_binary(), "build the reference program first (make -C oracle)"
    os.makedirs(GOLDEN, exist_ok=True)
    for paired in (False, True):
        for name, data in input_files(paired).items():
            with open(os.path.join(GOLDEN, name), "wb") as f:
                f.write(data)
            with tempfile.TemporaryDirectory() as d:
                fa, inp, out = os.path.join(d, "ref.fa"), os.path.join(d, name), os.path.join(d, "out.sam")
                TG.write_reference(fa)
                with open(inp, "wb") as f:
                    f.write(data)
                r = RF.run_ngm(["-r", fa, "-o", out, "--affine", "-t", "1", "--no-progress"] + (["-p"] if paired else []) + ["-q", inp], cwd=d)
                log = r.stdout + r.stderr
                assert "Done" in log, log[-2000:]
                print(name, [l.split("] ", 1)[-1] for l in log.splitlines() if "Input is" in l or "Average read length" in l or "Done" in l])
                with open(out, "rb") as f, gzip.GzipFile(os.path.join(GOLDEN, name + ".out.sam.gz"), "wb", mtime=0) as z:
                    z.write(f.read())


if __name__ == "__main__":
    main()
