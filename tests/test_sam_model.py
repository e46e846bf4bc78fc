"""The plain model of the record writers (tests/sam_model.py) pinned without a GPU: it reproduces every hand-typed expectation of the shared
cases (tests/sam_cases.py), and it equals the host formatter (csrc/cli_format.h, through tests/cpp/host_units_driver.cpp) byte for byte on seeded
random batches -- which is also a differential test of the host formatter on records nobody typed.  The random batches' coverage of the
writers' branches is asserted here, from the model's own tally: tests/test_gpu_sam_records.py runs the same batches through the GPU writers."""
import gzip
import struct
import subprocess

import pytest

import sam_cases as SC
import sam_model as SM
from test_host_units import format_driver  # noqa: F401  (the driver built with the sanitizers)


def counts6(counters):
    return counters[:3] + counters[4:]   # (without the bytes of text)


@pytest.mark.parametrize("run", SC.ALL_RUNS, ids=lambda r: r.name)
def test_model_reproduces_the_hand_typed_expectations(run):
    out, counters, _ = SM.format_batch(run.batch, run.bam)
    run.check(SC.decode_records(b"".join(out)) if run.bam else out, counts6(counters))


@pytest.mark.parametrize("identity,text", [(1.0, "1"), (0.0, "0"), (0.9, "0.9"), (0.98765, "0.9877"), (0.00004, "0"), (0.00005, "0.0001"), (0.5, "0.5"), (0.12, "0.12"),
                                           (0.99995, "1"), (0.30005, "0.3001"), (0.1005, "0.1005")])
def test_model_identity_text(identity, text):
    """XI:f is "%g" of round(identity * 10000.0f) / 10000.0f: at most four decimals, trailing zeros dropped, halves away from zero --
    in float: 0.00005f * 10000.0f is 0.5 exactly, 0.99995f * 10000.0f is 9999.5 exactly, 0.30005f * 10000.0f rounds up to 3000.5"""
    assert SM.xi_text(identity) == text


def host_output(driver, tmp_path, batch, bam):
    """-> the formatter's text, or its records as they stand in the BAM file; its six counters"""
    spec, out = str(tmp_path / "spec.txt"), str(tmp_path / "out.bam")
    with open(spec, "w") as f:
        f.write(batch.spec())
    r = subprocess.run([driver, "format", spec] + ([out] if bam else []), capture_output=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    body, _, last = r.stdout[:-1].rpartition(b"\n")
    assert last.startswith(b"#counts ")
    counts = [int(x) for x in last.split()[1:]]
    if not bam:
        return body + b"\n" if body else b"", counts
    assert body == b""
    data = gzip.decompress(open(out, "rb").read())
    l_text, = struct.unpack_from("<i", data, 4)
    at = 8 + l_text
    n_ref, = struct.unpack_from("<i", data, at)
    at += 4
    for _ in range(n_ref):
        at += 8 + struct.unpack_from("<i", data, at)[0]
    return data[at:], counts


def first_difference(a, b):
    n = next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))
    return "lengths %d / %d, first difference at byte %d: %r / %r" % (len(a), len(b), n, a[max(0, n - 80):n + 40], b[max(0, n - 80):n + 40])


@pytest.mark.parametrize("bam", [False, True], ids=["sam", "bam"])
@pytest.mark.parametrize("i", range(len(SC.RANDOM_CONFIGS)), ids=[SC.random_config_id(c) for c in SC.RANDOM_CONFIGS])
def test_model_equals_the_host_formatter_on_random_batches(format_driver, tmp_path, i, bam):  # noqa: F811
    batch = SC.random_config_batch(i)
    out, counters, _ = SM.format_batch(batch, bam)
    want = SM.output_bytes(out, bam)
    got, counts = host_output(format_driver, tmp_path, batch, bam)
    assert got == want, first_difference(got, want)
    assert counts == counts6(counters) and counters[3] == len(want)


@pytest.mark.parametrize("i", range(len(SC.RANDOM_CONFIGS)), ids=[SC.random_config_id(c) for c in SC.RANDOM_CONFIGS])
def test_random_batches_reach_every_branch(i):
    """the floors the random batches must reach, from the model's tally of the branches it took"""
    cfg, batch = SC.RANDOM_CONFIGS[i], SC.random_config_batch(i)
    _, counters, tally = SM.format_batch(batch, False)
    assert len(batch.recs) == SC.RANDOM_UNITS * (2 if cfg["paired"] else 1)
    if cfg["paired"]:
        for b in SM.BRANCHES:
            assert tally[b] >= 50, (b, tally)
    for f in ("fail_mq", "fail_identity", "fail_residues"):
        assert tally[f] >= 20, (f, tally)
    assert tally["fwd"] >= 50 and tally["rev"] >= 50, tally
    assert tally["short_qual"] >= 100, tally
    assert sum(1 for r in batch.recs if 0 < r.qual_len < len(r.row)) >= 100
    assert all(r.hit.pos < SC.POS_LIMIT for r in batch.recs)   # SAM's and BAM's integer widths agree
    assert any(r.empty for r in batch.recs) and any(len(r.row) == 0 and not r.empty for r in batch.recs) and any(len(r.name) == 254 for r in batch.recs)
    assert any(r.qual_len == 0 for r in batch.recs) and any(r.qual_len > batch.q - 1 for r in batch.recs)
