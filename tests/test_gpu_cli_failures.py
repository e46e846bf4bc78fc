"""-m gpu: the failure paths of the `ngm-hip` pipeline.  A batch that fails in the middle of a paired-end run must end the run -- exit
status 1, the one message, no `Done (` line -- and not leave the other workers waiting for its turn in the pair statistics
(ngm_pair_state: batches take turns, and a failed batch still has to pass its turn on)."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "nextgenmap_amd", "ngm-hip")
N_PAIRS, READ_LEN, BAD_PAIR = 2048, 50, 1100   # 4 096 reads in batches of 1 024: pair 1 100 = records 2 200 / 2 201, in the third batch


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    from nextgenmap_amd import build
    build.build()
    d = tmp_path_factory.mktemp("cli_failures")
    rng = np.random.default_rng(20261019)
    genome = rng.choice(np.frombuffer(b"ACGT", np.uint8), 20000)
    fa = str(d / "ref.fa")
    with open(fa, "wb") as f:
        f.write(b">chr1\n")
        g = genome.tobytes()
        for o in range(0, len(g), 70):
            f.write(g[o:o + 70] + b"\n")
    comp = np.zeros(256, np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    records = []
    for p in range(N_PAIRS):
        at = int(rng.integers(0, len(genome) - 300))
        a = genome[at:at + READ_LEN].tobytes()
        b = comp[genome[at + 200:at + 200 + READ_LEN]][::-1].tobytes()
        records.append((b"p%d/1" % p, a))
        records.append((b"p%d/2" % p, b))

    def write(name, recs):
        path = str(d / name)
        with open(path, "wb") as f:
            for nm, sq in recs:
                f.write(b"@" + nm + b"\n" + sq + b"\n+\n" + b"I" * len(sq) + b"\n")
        return path
    bad = list(records)
    bad[2 * BAD_PAIR + 1] = (b"x%d/2" % BAD_PAIR, bad[2 * BAD_PAIR + 1][1])
    return dict(fa=fa, dir=d, bad_names=write("bad_names.fq", bad), odd=write("odd.fq", records[:-1]))


def _fails_with(case, fq, extra, env, message, out="out.sam"):
    r = subprocess.run([CLI, "-r", case["fa"], "-p", "-q", fq, "-o", str(case["dir"] / out), "--batch-size", "1024", "--workers", "2"] + extra,
                       capture_output=True, text=True, timeout=60, env=dict(os.environ, **env))
    assert r.returncode == 1, (r.returncode, r.stderr[-2000:])
    assert "[ngm-hip] error: " + message in r.stderr.splitlines(), r.stderr[-2000:]
    assert "Done (" not in r.stderr, r.stderr[-2000:]


MATES = "Error while reading paired end reads. Names of mates don't match: p%d and x%d." % (BAD_PAIR, BAD_PAIR)
UNEVEN = "Error in input file. Number of reads in input not even. Please check the input or mapped in single-end mode."


def test_mate_names_that_differ_in_the_third_batch_end_the_run_gpu_text_route(case):
    _fails_with(case, case["bad_names"], [], {}, MATES)


def test_mate_names_that_differ_in_the_third_batch_end_the_run_host_format_route(case):
    _fails_with(case, case["bad_names"], [], {"NGM_HIP_HOST_SAM": "1"}, MATES)


def test_mate_names_that_differ_in_the_third_batch_end_the_run_sorted_bam(case):
    _fails_with(case, case["bad_names"], ["--bam", "--sort"], {}, MATES, out="out.bam")


def test_an_odd_number_of_records_ends_a_serial_reader_run(case):
    _fails_with(case, case["odd"], ["--serial-reader"], {}, UNEVEN)
