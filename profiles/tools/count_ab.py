"""Whole-run A/B of `ngm-hip --count` on one GPU: FASTQ to BAM on simulated 150 bp single-end reads at 1 % divergence (bench.py's genome and
read simulator), the same binary plain, with --snp, and with --snp --count, alternating, after one warm-up run that writes the index cache.
The BED file tiles a seventh of the genome with regions of 1 500 bases on both strands, every tenth one overlapped by a '.' region.
Prints, per run, the process wall and the program's own log lines; for the --count runs the add kernel's time per batch next to the SAM
stage's kernel time and --snp's add per batch, and the atomics per read the run issued.  No conversion is planted: the second atomic of a
column is rare in real data as well, the first one (every T or A column inside a region) is what the kernel's time is made of.
With a fourth argument, one more --snp --count run is made under `rocprofv3 --kernel-trace --stats -d DIR` and its kernel statistics are printed.
python profiles/tools/count_ab.py [reads] [genome Mbp] [runs each] [trace DIR]"""
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
RUN_LIMIT_S = 120   # a run of the default size takes 1-3 s (10 s under the profiler); a run that hangs ends the script


def grab(pattern, log, cast=float):
    m = re.search(pattern, log)
    return cast(m.group(1)) if m else None


def main():
    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 2_000_000
    mbp = float(sys.argv[2]) if len(sys.argv) > 2 else 30.0
    runs = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    d = tempfile.mkdtemp(prefix="count_ab_")
    contigs = bench.make_genome(int(mbp * 1e6), 20240601)
    fa, fq, bed = os.path.join(d, "ref.fa"), os.path.join(d, "reads.fq"), os.path.join(d, "utrs.bed")
    with open(fa, "wb") as f:
        for i, g in enumerate(contigs):
            f.write(b">chr%d\n" % (i + 1))
            b = g.tobytes()
            f.write(b"".join(b[o:o + 70] + b"\n" for o in range(0, len(b), 70)))
    regions = 0
    with open(bed, "w") as f:
        for i, g in enumerate(contigs):
            for k, s in enumerate(range(2000, len(g) - 2000, 10500)):
                f.write("chr%d\t%d\t%d\tu%d_%d\t0\t%s\n" % (i + 1, s, s + 1500, i + 1, k, "+-"[k % 2]))
                regions += 1
                if k % 10 == 0:
                    f.write("chr%d\t%d\t%d\tv%d_%d\t0\t.\n" % (i + 1, s + 700, s + 2200, i + 1, k))
                    regions += 1
    rows, _, _ = bench.make_reads(contigs, n, seed=20240605, subs=0.01)
    bench.write_fastq(rows, [fq])
    bases = sum(len(g) for g in contigs)
    print("ngm-hip --affine -b on %d single-end reads of %d bp, 1 %% substitutions, genome of %d bases in %d contigs (mean depth %.1f); batches of %d reads; %d regions" %
          (n, bench.READ_LEN, bases, len(contigs), n * bench.READ_LEN / bases, BATCH, regions))

    def run(tag, snp, count, trace=None):
        out = os.path.join(d, "out.bam")
        cmd = [CLI, "-r", fa, "-q", fq, "-o", out, "-b", "--affine"] + (["--snp", os.path.join(d, "out.vcf")] if snp else [])
        cmd += ["--count", bed, "--count-out", os.path.join(d, "out.tsv")] if count else []
        if trace:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", trace, "-o", "count", "--output-format", "csv", "--"] + cmd
        t0 = time.perf_counter()
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=RUN_LIMIT_S)
        wall = time.perf_counter() - t0
        assert r.returncode == 0, r.stderr[-2000:]
        log = r.stderr
        res = dict(wall=wall, mapping=grab(r"Mapping pass: ([0-9.]+) s", log), io=grab(r"Input to output: ([0-9.]+) s", log),
                   sam=grab(r"written on the GPU: ([0-9.]+) s of kernels", log))
        print("%s process wall %.3f s | mapping pass %.3f s | input to output %.3f s | SAM stage kernels (records + BGZF blocks) %.3f s" % (tag, wall, res["mapping"], res["io"], res["sam"]))
        batches = (n + BATCH - 1) // BATCH
        if snp:
            res["snp_add"] = grab(r"SNPs on the GPU: .* kernels: add ([0-9.]+) ms", log)
        if count:
            for line in log.splitlines():
                if "Conversion" in line or "SNPs on the GPU" in line:
                    print("    " + line)
            m = re.search(r"Conversions on the GPU: (\d+) alignments, (\d+) of them in a region, (\d+) eligible columns, (\d+) conversions, (\d+) masked positions in \d+ regions; "
                          r"kernels: add ([0-9.]+) ms, reduce ([0-9.]+) ms", log)
            aln, met, eligible, conv = (int(m.group(k)) for k in (1, 2, 3, 4))
            res.update(add=float(m.group(6)), reduce=float(m.group(7)))
            print("    per batch (%d batches): count add kernel %.3f ms | --snp add kernel %.3f ms | SAM stage kernels %.3f ms; a region took %.1f %% of the alignments; "
                  "32-bit atomics per alignment of the run: %.2f (eligible columns + conversions), 64-bit ones: 1 or 2 per (alignment, region that took it)" %
                  (batches, res["add"] / batches, (res.get("snp_add") or 0.0) / batches, 1e3 * res["sam"] / batches, 100.0 * met / max(1, aln), (eligible + conv) / max(1, aln)))
        return res

    run("warm-up (writes the index cache)", False, False)
    plain, snp, both = [], [], []
    for k in range(runs):
        plain.append(run("run %d plain         " % (k + 1), False, False))
        snp.append(run("run %d --snp          " % (k + 1), True, False))
        both.append(run("run %d --snp --count  " % (k + 1), True, True))
    mean = lambda rs, key: sum(r[key] for r in rs) / len(rs)
    for tag, rs in (("plain        ", plain), ("--snp         ", snp), ("--snp --count ", both)):
        print("%s mean: process wall %.3f s | mapping pass %.3f s | input to output %.3f s | SAM stage kernels %.3f s" % (tag, mean(rs, "wall"), mean(rs, "mapping"), mean(rs, "io"), mean(rs, "sam")))
    print("--count mean kernels, ms: add %.2f | reduce %.2f; --snp add in the same runs %.2f" % (mean(both, "add"), mean(both, "reduce"), mean(both, "snp_add")))
    if len(sys.argv) > 4:
        traced(run, sys.argv[4])
    tsv = open(os.path.join(d, "out.tsv")).read().splitlines()
    print("TSV: %d regions, %d with reads, cov_on_ts summed %d" % (len(tsv) - 1, sum(1 for l in tsv[1:] if int(l.split("\t")[9]) > 0), sum(int(l.split("\t")[7]) for l in tsv[1:])))


def traced(run, trace):
    run("traced --snp --count ", True, True, trace)
    for root, _, files in os.walk(trace):
        for fn in files:
            if fn.endswith("kernel_stats.csv"):
                print("rocprofv3 --kernel-trace --stats, %s:" % fn)
                for line in open(os.path.join(root, fn)).read().splitlines()[:14]:
                    print("    " + line[:200])


if __name__ == "__main__":
    main()
