"""Whole-run A/B of `ngm-hip --snp` on one GPU: FASTQ to BAM on simulated 150 bp single-end reads at 1 % divergence (bench.py's genome and
read simulator), the same binary with and without --snp, alternating, after one warm-up run that writes the index cache.  Prints, per run,
the process wall and the program's own log lines; for the --snp runs the add kernel's time per batch next to the SAM stage's kernel time
per batch, the four finish times and the atomics per read the run issued.
python profiles/tools/snp_ab.py [reads] [genome Mbp] [runs each]"""
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
import bench   # noqa: E402  (the simulator only)

CLI = os.path.join(ROOT, "nextgenmap_amd", "ngm-hip")
BATCH = 1 << 18   # ngm-hip's default --batch-size


def grab(pattern, log, cast=float):
    m = re.search(pattern, log)
    return cast(m.group(1)) if m else None


def main():
    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 2_000_000
    mbp = float(sys.argv[2]) if len(sys.argv) > 2 else 30.0
    runs = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    d = tempfile.mkdtemp(prefix="snp_ab_")
    contigs = bench.make_genome(int(mbp * 1e6), 20240601)
    fa, fq = os.path.join(d, "ref.fa"), os.path.join(d, "reads.fq")
    with open(fa, "wb") as f:
        for i, g in enumerate(contigs):
            f.write(b">chr%d\n" % (i + 1))
            b = g.tobytes()
            f.write(b"".join(b[o:o + 70] + b"\n" for o in range(0, len(b), 70)))
    rows, _, _ = bench.make_reads(contigs, n, seed=20240605, subs=0.01)
    bench.write_fastq(rows, [fq])
    bases = sum(len(g) for g in contigs)
    print("ngm-hip --affine -b on %d single-end reads of %d bp, 1 %% substitutions, genome of %d bases in %d contigs (mean depth %.1f); batches of %d reads" %
          (n, bench.READ_LEN, bases, len(contigs), n * bench.READ_LEN / bases, BATCH))

    def run(tag, snp):
        out = os.path.join(d, "out.bam")
        cmd = [CLI, "-r", fa, "-q", fq, "-o", out, "-b", "--affine"] + (["--snp", os.path.join(d, "out.vcf")] if snp else [])
        t0 = time.perf_counter()
        r = subprocess.run(cmd, capture_output=True, text=True)
        wall = time.perf_counter() - t0
        assert r.returncode == 0, r.stderr[-2000:]
        log = r.stderr
        res = dict(wall=wall, mapping=grab(r"Mapping pass: ([0-9.]+) s", log), io=grab(r"Input to output: ([0-9.]+) s", log),
                   sam=grab(r"written on the GPU: ([0-9.]+) s of kernels", log))
        print("%s process wall %.3f s | mapping pass %.3f s | input to output %.3f s | SAM stage kernels (records + BGZF blocks) %.3f s" % (tag, wall, res["mapping"], res["io"], res["sam"]))
        if snp:
            for line in log.splitlines():
                if "SNP" in line:
                    print("    " + line)
            m = re.search(r"SNPs on the GPU: (\d+) alignments, (\d+) mismatching bases counted, (\d+) calls, (\d+) bytes of VCF; kernels: add ([0-9.]+) ms, scan ([0-9.]+) ms, flag ([0-9.]+) ms, text ([0-9.]+) ms", log)
            aln, alt = int(m.group(1)), int(m.group(2))
            batches = (n + BATCH - 1) // BATCH
            res.update(add=float(m.group(5)), finish=[float(m.group(k)) for k in (6, 7, 8)])
            # (an alignment of these reads is one covered block unless it holds a deletion: the +1 / -1 pair is counted once per alignment here, a lower bound)
            print("    per batch (%d batches): add kernel %.3f ms | SAM stage kernels %.3f ms; atomics per read: %.2f mismatching bases + 2 per covered block = at least %.2f" %
                  (batches, res["add"] / batches, 1e3 * res["sam"] / batches, alt / max(1, aln), alt / max(1, aln) + 2.0))
        return res

    run("warm-up (writes the index cache)", False)
    plain, snp = [], []
    for k in range(runs):
        plain.append(run("run %d plain " % (k + 1), False))
        snp.append(run("run %d --snp  " % (k + 1), True))
    mean = lambda rs, key: sum(r[key] for r in rs) / len(rs)
    for tag, rs in (("plain", plain), ("--snp ", snp)):
        print("%s mean: process wall %.3f s | mapping pass %.3f s | input to output %.3f s | SAM stage kernels %.3f s" % (tag, mean(rs, "wall"), mean(rs, "mapping"), mean(rs, "io"), mean(rs, "sam")))
    print("--snp  mean kernels, ms: add %.2f | scan %.2f | flag %.2f | text %.2f" % ((mean(snp, "add"),) + tuple(sum(r["finish"][k] for r in snp) / len(snp) for k in range(3))))
    vcf = open(os.path.join(d, "out.vcf"), "rb").read()
    print("VCF: %d bytes, %d calls" % (len(vcf), sum(1 for l in vcf.splitlines() if not l.startswith(b"#"))))


if __name__ == "__main__":
    main()
