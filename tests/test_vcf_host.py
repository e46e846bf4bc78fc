"""Host logic of --vcf, no GPU: the VCF reader (src/parser/VcfParser.cpp restated in csrc/vcf.cpp) through the host-only entry
ngm_vcf_parse_text against a Python restatement of VcfParser below, plain and gzip; and the command line's handling of an
unreadable VCF (an error before any GPU work, where the reference logs it and goes on without variants)."""
import ctypes as C
import os
import subprocess

import pytest

import vcf_fixtures as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "nextgenmap_amd", "ngm-hip")


def _lib():
    from nextgenmap_amd.pipeline import _lib as load
    return load()


def _parse(path, contigs):
    """contigs: [(name, start)] -> (count, [(pos, ref, alt)])"""
    lib = _lib()
    n = len(contigs)
    names = (C.c_char_p * n)(*[c[0].encode() for c in contigs])
    starts = (C.c_uint64 * n)(*[c[1] for c in contigs])
    need = C.c_size_t(0)
    cnt = lib.ngm_vcf_parse_text(n, names, starts, path.encode(), None, 0, C.byref(need))
    if cnt < 0:
        return cnt, None
    buf = C.create_string_buffer(max(1, need.value))
    assert lib.ngm_vcf_parse_text(n, names, starts, path.encode(), buf, need.value, C.byref(need)) == cnt
    rows = [l.split("\t") for l in buf.raw[:need.value].decode().splitlines()]
    return cnt, [(int(p), r, a) for p, r, a in rows]


def _c_atoi(s):
    s = s.lstrip(" \t\n\v\f\r")
    sign, i = 1, 0
    if s[:1] in "+-" and s[:1]:
        sign, i = (-1 if s[0] == "-" else 1), 1
    v = 0
    while i < len(s) and s[i].isdigit():
        v = v * 10 + int(s[i])
        i += 1
    return sign * v


def _model(data, contigs):
    """VcfParser::open / parse_line / add_line: lines split on '\\n' only, trimmed of tab/CR/space, split on tabs (empty fields
    dropped), < 8 fields skipped, one variant per ALT allele, unknown contig / '.' / non-ACGTN dropped"""
    starts = {}
    for name, st in contigs:
        starts.setdefault(name, st)
    out = []
    for line in data.split("\n"):
        if not line or line[0] == "#":
            continue
        line = line.strip("\t\r ")
        parts = [p for p in line.split("\t") if p != ""]
        if len(parts) < 8:
            continue
        chrom, pos, ref, alts = parts[0], parts[1], parts[3], parts[4]
        for alt in [a for a in alts.split(",") if a != ""]:
            if chrom not in starts or alt == "." or not set(ref + alt) <= set("ACGTN"):
                continue
            out.append(((starts[chrom] + _c_atoi(pos)) % (1 << 64), ref, alt))
    return out


def _contigs_of(contig_arrays):
    """the concatenated coordinates of the contigs (SequenceProvider.cpp:289-326): 1000 N in front, between and behind, even starts"""
    out, at = [], 1000
    for i, g in enumerate(contig_arrays):
        out.append(("chr%d" % (i + 1), at))
        at += len(g) + (len(g) & 1) + 1000
    return out


@pytest.mark.parametrize("fixture", ["F1", "F2", "F3"])
def test_vcf_reader_matches_vcfparser(tmp_path, fixture):
    from nextgenmap_amd import build
    build.build()
    fa, vcf, contig_arrays = V.FIXTURES[fixture](str(tmp_path))
    contigs = _contigs_of(contig_arrays)
    cnt, got = _parse(vcf, contigs)
    want = _model(open(vcf, "rb").read().decode(), contigs)
    assert cnt == len(want)
    assert got == want


def test_vcf_reader_rules(tmp_path):
    """each rule on its own line: multi-allelic, CRLF, a double tab (columns shift), fewer than 8 fields, unknown contig, '.',
    <DEL>, '*', lowercase, padding, a last line without '\\n'"""
    from nextgenmap_amd import build
    build.build()
    body = ("##x\n#CHROM\n\n"
            "c1\t10\t.\tA\tC,G\t.\t.\t.\r\n"           # 2 variants, CR trimmed
            "c1\t11\t\t.\tA\tT\t.\t.\t.\n"            # double tab: the empty field is dropped, still 8 fields
            "c1\t12\t.\tA\tT\t.\t.\n"                 # 7 fields
            "cX\t13\t.\tA\tT\t.\t.\t.\n"              # unknown contig
            "c1\t14\t.\tA\t.\t.\t.\t.\n"              # missing ALT
            "c1\t15\t.\tA\t<DEL>\t.\t.\t.\n"
            "c1\t16\t.\tA\t*\t.\t.\t.\n"
            "c1\t17\t.\ta\tc\t.\t.\t.\n"
            " \tc2\t18\t.\tAC\tA,,N\t.\t.\t. \t\n"    # padding; an empty allele is skipped
            "c2\t19\t.\tN\tACGTN\t.\t.\t.")          # no final newline
    p = tmp_path / "r.vcf"
    p.write_bytes(body.encode())
    cnt, got = _parse(str(p), [("c1", 1000), ("c2", 5000), ("c1", 9000)])
    assert got == [(1010, "A", "C"), (1010, "A", "G"), (1011, "A", "T"), (5018, "AC", "A"), (5018, "AC", "N"), (5019, "N", "ACGTN")]
    assert got == _model(body, [("c1", 1000), ("c2", 5000), ("c1", 9000)])


def test_vcf_gz_equals_plain(tmp_path):
    from nextgenmap_amd import build
    build.build()
    d1, d2 = tmp_path / "a", tmp_path / "b"
    d1.mkdir(); d2.mkdir()
    fa, vcf, contig_arrays = V.f1(str(d1))
    _, vcf_gz, _ = V.f1(str(d2), gz=True)
    contigs = _contigs_of(contig_arrays)
    a, b = _parse(vcf, contigs), _parse(vcf_gz, contigs)
    assert a[0] > 400 and a == b


def test_vcf_missing_file_is_an_error(tmp_path):
    from nextgenmap_amd import build
    build.build()
    assert _parse(str(tmp_path / "none.vcf"), [("c1", 1000)])[0] < 0
    # the command line: exit 1 with the VCF's error, before the reference is opened and before any GPU work
    r = subprocess.run([CLI, "-r", str(tmp_path / "none.fa"), "-q", str(tmp_path / "none.fq"), "-o", str(tmp_path / "out.sam"),
                        "--vcf", str(tmp_path / "missing.vcf")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1, r.stderr
    assert "Failed to open VCF file" in r.stderr and "missing.vcf" in r.stderr, r.stderr
    assert "not supported" not in r.stderr


def test_vcf_refuses_bs_mapping(tmp_path):
    from nextgenmap_amd import build
    build.build()
    v = tmp_path / "v.vcf"
    v.write_text("#\n")
    r = subprocess.run([CLI, "-r", str(tmp_path / "none.fa"), "-q", str(tmp_path / "none.fq"), "-o", str(tmp_path / "out.sam"),
                        "--vcf", str(v), "--bs-mapping"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1
    assert "--vcf cannot be combined with --bs-mapping" in r.stderr, r.stderr


@pytest.mark.parametrize("extra,why", [
    (["--argos"], "--argos"),
    (["--bam"], "--bam"),
    (["-n", "2"], "-n/--topn above 1"),
    (["-e"], "-e/--end-to-end"),
    (["-g", "0,1"], "several GPUs"),
    (["--shard-output"], "--shard-output"),
    (["--shard", "0/2"], "--shard"),
    (["--bin-size", "1"], "--bin-size below 2"),
], ids=["argos", "bam", "topn", "end-to-end", "gpus", "shard-output", "shard", "bin-size"])
def test_vcf_refuses_untested_modes(tmp_path, extra, why):
    """modes not yet checked against the reference with an index that holds the VCF's k-mers are refused before any GPU work"""
    from nextgenmap_amd import build
    build.build()
    v = tmp_path / "v.vcf"
    v.write_text("#\n")
    r = subprocess.run([CLI, "-r", str(tmp_path / "none.fa"), "-q", str(tmp_path / "none.fq"), "-o", str(tmp_path / "out.sam"),
                        "--vcf", str(v)] + extra, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1
    assert "--vcf cannot be combined with " + why in r.stderr, r.stderr
    assert not os.path.exists(tmp_path / "out.sam")
