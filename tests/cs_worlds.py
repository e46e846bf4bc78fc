"""The configurations, genomes and reads of the candidate-search tests (tests/test_cs_model.py, tests/test_gpu_cs_shapes.py,
oracle/make_search_goldens.py): everything from fixed seeds, so the three see the same bytes.  Test infrastructure.

One genome serves every configuration: three contigs (one of odd length), repeat families of 2, 3, 6, 8 and 24 copies, one N run, a 90-base
run of A, a 700-base AC repeat and a 400-base region that is its own reverse complement.  A configuration's read set is simulated reads
plus the edge reads of edge_reads() plus reads built to reach a vote maximum of exactly 1, 2 and 3 (boundary_reads())."""
import functools
import hashlib
from collections import namedtuple

import numpy as np

import cs_model as CM
import ngm_host_model as HM
import simulate as S

N = ord("N")
GENOME_SEED = 20261
UNLIMITED = 2 ** 31 - 1
SMALL_PAL = 90010                        # the centre of a 20-base stretch of the first contig that is its own reverse complement
ALIGNED, ALIGNED_AT = (7, 8, 9), 60000   # families of exact, phase-aligned copies in the second contig (genome())

Config = namedtuple("Config", "id read_len k skip bins kfreq s kmin cmrs env n_sim golden world")


def _c(id, read_len, k=13, skip=2, bins=2, kfreq=0, s=0.5, kmin=0.0, cmrs=UNLIMITED, env=None, n_sim=400, golden=None, world="main"):
    """kfreq 0: the automatic max_kfreq; golden: the id of the configuration whose recorded reference results these options share ("-": none)"""
    return Config(id, read_len, k, skip, bins, kfreq, s, kmin, cmrs, dict(env or {}), n_sim, golden or id, world)


CONFIGS = [
    _c("defaults-36", 36), _c("defaults-76", 76), _c("defaults-100", 100), _c("defaults-150", 150), _c("defaults-250", 250),
    # (model only: with k = 7 the reference program counts k-mers in memory it has not cleared -- CountKmerFreq's memset clears a quarter
    # of the array, which goes unnoticed only while the array is large enough to come fresh from the system -- and builds no usable index)
    _c("shape2-bin2", 140, k=7, skip=1, golden="-"), _c("shape2-bin3", 140, k=7, skip=1, bins=3, golden="-"),
    _c("bins-3", 150, bins=3), _c("bins-4", 150, bins=4), _c("bins-8", 150, bins=8), _c("bins-1", 100, bins=1), _c("bins-0", 100, bins=0),
    _c("even-k-12", 100, k=12), _c("even-k-10", 150, k=10),
    _c("k-11", 100, k=11), _c("k-14", 100, k=14, n_sim=200), _c("k-9-skip-0", 100, k=9, skip=0),
    _c("skip-0", 100, skip=0), _c("skip-1", 100, skip=1), _c("skip-5", 100, skip=5),
    _c("long-271", 271, n_sim=300), _c("long-300", 300, n_sim=300),
    _c("kfreq-low", 100, kfreq=8), _c("kfreq-high", 150, kfreq=1200),
    _c("waves-1", 100, k=12, env={"NGM_HIP_CS_WAVES": "1"}, golden="even-k-12"),
    _c("waves-1-items-24", 100, k=12, env={"NGM_HIP_CS_WAVES": "1", "NGM_HIP_CS_FAST_ITEMS": "24"}, golden="even-k-12"),
    _c("waves-2", 100, k=12, env={"NGM_HIP_CS_WAVES": "2"}, golden="even-k-12"),
    _c("waves-4", 100, k=12, env={"NGM_HIP_CS_WAVES": "4"}, golden="even-k-12"),
    _c("thresholds-s0-kmin2", 100, s=0.0, kmin=2.0), _c("thresholds-s034", 100, s=0.34), _c("thresholds-s1", 100, s=1.0),
    _c("thresholds-s09-kmin40", 100, s=0.9, kmin=40.0),
    # (model only: the reference's log is written before the max_cmrs rule applies; with reads of their own from the 3-copy family)
    _c("max-cmrs-1", 100, cmrs=1, golden="-"), _c("max-cmrs-2", 100, cmrs=2, golden="-"), _c("max-cmrs-5", 100, cmrs=5, golden="-"),
    _c("votes-256", 100, skip=0, bins=4, kfreq=1000), _c("votes-max", 300, skip=0, bins=8, kfreq=1000, n_sim=200),
    # more votes for one (bin, strand) than a 16-bit half of a vote table holds: 600 bases of AC against 1 900 (world "long-ac") give
    # 588 k-mers x 128 hits per 256-base bin = 75 264.  The reference program counts them; the product refuses the combination (REFUSED)
    _c("votes-64k", 600, skip=0, bins=8, kfreq=1000, n_sim=60, world="long-ac"),
]
# configurations whose mapper the product must refuse to create, with the words of its message (ngm_mapper_create: a read of qry_max_len
# could collect more than 65 535 votes in one bin)
REFUSED = {"votes-64k": "65535 votes"}
# the heavy paths (tests/test_gpu_cs_shapes.py::test_heavy_paths_under_forced_limits): a genome of its own, half of the reads from its families
HEAVY = [_c("heavy-100", 100, n_sim=150, golden="-", world="heavy"), _c("heavy-150", 150, n_sim=150, golden="-", world="heavy")]
BY_ID = {c.id: c for c in CONFIGS + HEAVY}
GOLDEN_IDS = [c.id for c in CONFIGS if c.golden == c.id]


def qlen(cfg):
    return (cfg.read_len | 1) + 1


def ngm_options(cfg):
    """the reference program's (and ngm-hip's) command-line options of a configuration"""
    o = ["-k", str(cfg.k), "--kmer-skip", str(cfg.skip), "--bin-size", str(cfg.bins), "-s", repr(cfg.s), "--kmer-min", str(int(cfg.kmin)),
         "--max-read-length", str(cfg.read_len)]
    if cfg.kfreq:
        o += ["--max-kfreq", str(cfg.kfreq)]
    if cfg.cmrs != UNLIMITED:
        o += ["--max-cmrs", str(cfg.cmrs)]
    return o


def _place(rng, contigs, seq, copies, divergence, where=None):
    for i in range(copies):
        g = contigs[i % len(contigs)] if where is None else contigs[where]
        p = int(rng.integers(2000, len(g) - len(seq) - 2000))
        c = seq.copy()
        m = rng.random(len(seq)) < divergence
        c[m] = S.ACGT[rng.integers(0, 4, int(m.sum()))]
        g[p:p + len(seq)] = c


def _place_family(rng, contigs, length, copies, lo, hi):
    """a family of `copies` copies at lo..hi divergence -> [(contig index, position)]"""
    fam, at = S.ACGT[rng.integers(0, 4, length)], []
    for i in range(copies):
        ci = i % len(contigs)
        while True:
            p = int(rng.integers(2000, len(contigs[ci]) - length - 2000))
            if all(c != ci or abs(p - q) > length for c, q in at):
                break
        c = fam.copy()
        m = rng.random(length) < rng.uniform(lo, hi)
        c[m] = S.ACGT[rng.integers(0, 4, int(m.sum()))]
        contigs[ci][p:p + length] = c
        at.append((ci, p))
    return at


@functools.lru_cache(maxsize=None)
def _heavy_world():
    """one 300 bp family of 60 copies at 1-3 % divergence and one of 24: every k-mer list stays below the automatic max_kfreq"""
    contigs = S.make_genome([150000, 90001, 60000], seed=GENOME_SEED + 10, repeat_families=0, n_runs=0)
    rng = np.random.default_rng(GENOME_SEED + 11)
    at = _place_family(rng, contigs, 300, 60, 0.01, 0.03)
    for ci, p in _place_family(rng, contigs, 300, 24, 0.01, 0.03):
        if all(c != ci or abs(p - q) > 300 for c, q in at):
            at.append((ci, p))
    for g in contigs:
        g.setflags(write=False)
    return tuple(contigs), tuple(at)


def _heavy_reads(cfg):
    contigs, at = _heavy_world()
    rng = np.random.default_rng(GENOME_SEED + 12 + cfg.read_len)
    out = []
    for i in range(cfg.n_sim):
        ci, p = at[int(rng.integers(0, len(at)))]
        r = contigs[ci][p + int(rng.integers(0, 300 - cfg.read_len + 1)):][:cfg.read_len].copy()
        m = rng.random(len(r)) < 0.01
        r[m] = S.ACGT[rng.integers(0, 4, int(m.sum()))]
        out.append(("f%d_%d_%d" % (i, ci, p), S.revcomp(r) if i & 1 else r))
    sim = S.make_reads(list(contigs), cfg.n_sim, cfg.read_len, seed=GENOME_SEED + 13 + cfg.read_len, sub_rate=0.02, indel_rate=0.003)
    return out + [(name, seq) for name, seq, _ in sim]


@functools.lru_cache(maxsize=None)
def genome(world="main"):
    if world == "heavy":
        return _heavy_world()[0]
    if world == "long-ac":   # the main genome with its AC repeat 1 900 bases long
        contigs = [g.copy() for g in genome("main")]
        contigs[1][50000:51900] = np.resize(np.frombuffer(b"AC", np.uint8), 1900)
        half = S.ACGT[np.random.default_rng(GENOME_SEED + 20).integers(0, 4, 600)]
        contigs[2][29600:30800] = np.concatenate([half, S.revcomp(half)])      # (600-base reads: a longer self-complementary region, same centre)
        for g in contigs:
            g.setflags(write=False)
        return tuple(contigs)
    contigs = S.make_genome([170000, 120001, 60000], seed=GENOME_SEED, repeat_families=6, repeat_len=300, copies=2, divergence=0.01, n_runs=0)
    rng = np.random.default_rng(GENOME_SEED + 1)
    for copies in (2, 3, 8, 24):
        _place(rng, contigs, S.ACGT[rng.integers(0, 4, 300)], copies, 0.01)
    half = S.ACGT[rng.integers(0, 4, 200)]
    contigs[2][30000:30400] = np.concatenate([half, S.revcomp(half)])          # its own reverse complement
    ten = S.ACGT[rng.integers(0, 4, 10)]
    contigs[0][SMALL_PAL - 10:SMALL_PAL + 10] = np.concatenate([ten, S.revcomp(ten)])
    contigs[0][40000:40057] = N                                                 # the N run
    # exact copies at positions of one phase of every index step (1, 2, 3, 6): each of their indexed k-mers occurs exactly 7, 8, 9 times
    for j, copies in enumerate(ALIGNED):
        fam = S.ACGT[rng.integers(0, 4, 300)]
        for i in range(copies):
            p = ALIGNED_AT + 6000 * j + 600 * i
            contigs[1][p:p + 300] = fam
    contigs[0][60000:60090] = ord("A")
    contigs[1][50000:50700] = np.resize(np.frombuffer(b"AC", np.uint8), 700)
    for g in contigs:
        g.setflags(write=False)
    return tuple(contigs)


@functools.lru_cache(maxsize=None)
def index_of(k, skip, bins, world="main"):
    return CM.build_index(genome(world), k, skip, bins)


def params(cfg, max_cmrs=None):
    """the keyword arguments of CM.search for a configuration"""
    idx = index_of(cfg.k, cfg.skip, cfg.bins, cfg.world)
    return dict(index=idx, k=cfg.k, bin_size=cfg.bins, max_kfreq=cfg.kfreq or CM.auto_max_kfreq(idx), sensitivity=cfg.s, kmer_min=cfg.kmin,
                max_cmrs=cfg.cmrs if max_cmrs is None else max_cmrs)


@functools.lru_cache(maxsize=None)
def _simulated(read_len, n, world="main"):
    return S.make_reads(list(genome(world)), n, read_len, seed=GENOME_SEED + 2 + read_len, sub_rate=0.02, indel_rate=0.003)


def edge_reads(cfg):
    """[(tag, sequence)]: the read shapes at which a k-mer walk, a bin or a threshold can go wrong"""
    contigs, L, k, q = genome(cfg.world), cfg.read_len, cfg.k, qlen(cfg)
    rng = np.random.default_rng(GENOME_SEED + 3 + L + 1000 * k)
    g0, g1, g2 = contigs
    at = lambda g, p, n=L: g[p:p + n].copy()
    out = []
    for n in (k - 1, k, k + 1):
        out.append(("len-%d" % n, at(g0, 5000, n)))
    out.append(("all-n", np.full(L, N, np.uint8)))
    for lead in (L - k - 1, L - k, L - k + 1):
        r = at(g0, 7000)
        r[:lead] = N
        out.append(("lead-n-%d" % lead, r))
    r = at(g0, 9000)
    r[k - 1::k] = N
    out.append(("n-every-k", r))
    r = at(g0, 11000)
    r[-1] = N
    out.append(("n-last", r))
    r = at(g0, 11500)
    r[L // 2] = N
    out.append(("n-inner", r))
    r = at(g0, 11800)
    r[L // 2:L // 2 + 2] = N      # two Ns: the walk behind them begins with an N
    out.append(("nn-inner", r))
    r = at(g0, 11900)
    r[L - k - 2:L - k] = N        # ... followed by exactly k bases
    out.append(("nn-then-k", r))
    out.append(("len-q-1", at(g0, 13000, q - 1)))
    out.append(("len-q+5", at(g0, 15000, q + 5)))     # the parser keeps q - 1 bases
    out.append(("spacer", np.concatenate([g0[len(g0) - L // 2:], g1[:L - L // 2]])))
    out.append(("spacer-odd", np.concatenate([g1[len(g1) - L // 2:], g2[:L - L // 2]])))
    for p in (0, 1, 3, min(200, len(g0)) - min(L, 200)):
        out.append(("first-%d" % p, at(g0, p)))
        out.append(("first-%d-rc" % p, S.revcomp(at(g0, p))))
    for p in (len(g2) - L, len(g2) - L - 1, len(g2) - L - 3, len(g2) - 200):
        out.append(("last-%d" % p, at(g2, p)))
        out.append(("last-%d-rc" % p, S.revcomp(at(g2, p))))
    for p in (len(g1) - L, len(g1) - L - 2):          # the contig of odd length
        out.append(("odd-last-%d" % p, at(g1, p)))
    for i in range(12):
        out.append(("random-%d" % i, S.ACGT[rng.integers(0, 4, L)]))
    for p in (30000 + 200 - L // 2, 30000 + 201 - L // 2, 30000 + 202 - L // 2, 30000 + 203 - L // 2, 30000 + 150 - L // 2, 30010):
        out.append(("palindrome-%d" % p, at(g2, p)))
    # a read centred on the small self-complementary stretch: the forward strand votes with every k-mer, the reverse strand with the few
    # inside the stretch, for the same bin (one position to either side: an odd length, or a bin border between the two diagonals)
    for d in (-1, 0, 1):
        out.append(("small-pal-%d" % d, at(g0, SMALL_PAL - L // 2 + d)))
    # one k-mer, at an indexed position of a unique stretch: one hit, a maximum of 1, a threshold <= 1 whenever kmer_min allows it
    for i in range(10):
        out.append(("one-kmer-%d" % i, at(g0, 1200 + 420 * i, k)))
    out.append(("ac", np.resize(np.frombuffer(b"AC", np.uint8), L)))
    out.append(("ca", np.resize(np.frombuffer(b"CA", np.uint8), L)))
    out.append(("ac-edge", at(g1, 50000 - L // 2)))
    out.append(("homopolymer", np.full(L, ord("A"), np.uint8)))
    out.append(("homopolymer-t", np.full(L, ord("T"), np.uint8)))
    out.append(("a-run-edge", at(g0, 60000 - L // 3)))
    out.append(("n-run-edge", at(g0, 40000 - L // 2)))
    for j, copies in enumerate(ALIGNED):
        for i in (0, copies - 1):
            out.append(("aligned-%d-%d" % (copies, i), at(g1, ALIGNED_AT + 6000 * j + 600 * i + (300 - min(L, 300)) // 2)))
    # reads around k-mers whose forward + reverse list length is max_kfreq - 1, max_kfreq, max_kfreq + 1: voted, skipped, skipped
    idx = index_of(cfg.k, cfg.skip, cfg.bins, cfg.world)
    mk = cfg.kfreq or CM.auto_max_kfreq(idx)
    rc = CM.revcomp_kmer(idx.kmers, k)
    j = np.minimum(np.searchsorted(idx.kmers, rc), len(idx.kmers) - 1)
    tot = idx.raw.astype(np.int64) + np.where(idx.kmers[j] == rc, idx.raw[j], 0)
    g, geom, _ = HM.concat_genome(contigs)
    for t in (mk - 1, mk, mk + 1):
        at_t = np.flatnonzero(tot == t)
        for n, i in enumerate(at_t[len(at_t) // 6::max(1, len(at_t) // 3)][:3]):
            p = int(idx.positions[idx.starts[i]]) - L // 3
            r = g[p:p + L].copy()
            if len(r) == L:
                out.append(("kfreq-%d-%d" % (t, n), r))
    return out


def boundary_reads(cfg, per=2):
    """[(tag, sequence)]: random reads with a piece of the genome, kept when the model gives them a vote maximum of exactly 1, 2 or 3 --
    at sensitivity 0.5 / 0.34 thresholds of 1.0 (maximum 2), 1.02 (maximum 3) and below 1 (maximum 1)"""
    L, k = cfg.read_len, cfg.k
    rng = np.random.default_rng(GENOME_SEED + 4 + L + 1000 * k + 100000 * cfg.skip)
    g = genome(cfg.world)[0]
    kw = params(cfg, max_cmrs=UNLIMITED)
    got = {1: [], 2: [], 3: []}
    for _ in range(600):
        if all(len(v) >= per for v in got.values()):
            break
        seg = min(L - 1, k + int(rng.integers(0, 4 * (cfg.skip + 1))))
        p, off = int(rng.integers(70000, 160000)), int(rng.integers(0, L - seg))
        r = S.ACGT[rng.integers(0, 4, L)]
        r[off:off + seg] = g[p:p + seg]
        m = CM.search(r.tobytes(), **kw).max_votes
        if m in got and len(got[m]) < per:
            got[m].append(r)
    # (a k so small that random flanks hit the genome leaves some of them out: census() counts what a read set reaches)
    return [("max-%d-%d" % (m, i), r) for m, v in sorted(got.items()) for i, r in enumerate(v)]


@functools.lru_cache(maxsize=None)
def file_reads_of(cfg_id):
    """[(name, sequence)] as the FASTQ file of a configuration holds them (the golden's, where it shares one)"""
    cfg = BY_ID.get(BY_ID[cfg_id].golden, BY_ID[cfg_id])
    if cfg.world == "heavy":
        return [(name, np.ascontiguousarray(seq, dtype=np.uint8)) for name, seq in _heavy_reads(cfg)]
    sim = [(name, seq) for name, seq, _ in _simulated(cfg.read_len, cfg.n_sim, cfg.world)]
    extra = [("e%d_%s" % (i, tag), seq) for i, (tag, seq) in enumerate(edge_reads(cfg) + boundary_reads(cfg))]
    if cfg.cmrs != UNLIMITED:   # reads around k-mers that occur three times: the family of three copies
        idx = index_of(cfg.k, cfg.skip, cfg.bins, cfg.world)
        g = HM.concat_genome(genome(cfg.world))[0]
        at3 = np.flatnonzero(idx.raw == 3)
        for n, i in enumerate(at3[len(at3) // 16::max(1, len(at3) // 8)][:8]):
            p = int(idx.positions[idx.starts[i]]) - cfg.read_len // 3
            extra.append(("c%d_three" % n, g[p:p + cfg.read_len].copy()))
    return [(name, np.ascontiguousarray(seq, dtype=np.uint8)) for name, seq in extra + sim]


def reads_of(cfg_id):
    """... as the parser keeps them: q - 1 bases at the most (IParser.h:59-121)"""
    q = qlen(BY_ID[cfg_id])
    return [(name, seq[:q - 1]) for name, seq in file_reads_of(cfg_id)]


@functools.lru_cache(maxsize=None)
def results_of(cfg_id):
    """the model's Result per read of a configuration, computed once per process"""
    kw = params(BY_ID[cfg_id])
    return [CM.search(seq.tobytes(), **kw) for _, seq in reads_of(cfg_id)]


def bucket_words(index, canonical):
    """W, the dwords of an index bucket (nextgenmap_amd/csrc/refindex.h): the smallest power of two from 4 to 64 (one bucket per k-mer: 32)
    with W - 1 >= mu + 4 sqrt(mu) + 0.5, mu the mean list length per bucket; lists of up to W - 1 entries lie in the bucket, longer ones
    in the position table"""
    n = 4 ** index.k // (2 if canonical else 1)
    mu = float(index.raw.sum()) / n
    lw = 2
    while lw < (6 if canonical else 5) and (1 << lw) - 1 < mu + 4.0 * np.sqrt(mu) + 0.5:
        lw += 1
    return 1 << lw


@functools.lru_cache(maxsize=None)
def census(cfg_id):
    """how often the reads of a configuration reach each edge, counted from the model alone"""
    cfg = BY_ID[cfg_id]
    kw = params(cfg)
    canonical = bool(cfg.k & 1)
    w = bucket_words(kw["index"], canonical)
    c = dict(no_kmers=0, hits=0, thr_le_1=0, hits_thr_le_1=0, votes_gt_65535=0, thr_eq_1=0, thr_above_1=0, thr_below_1=0, strand_tie=0, one_strand=0, repeat_bin=0, max_votes=0, votes_gt_255=0,
             kfreq_minus_1=0, kfreq=0, kfreq_plus_1=0, cmrs_minus_1=0, cmrs=0, cmrs_plus_1=0, list_w_minus_2=0, list_w_minus_1=0, list_w=0, list_long=0, palindromes=0,
             bucket_words=w)
    for (_, seq), res in zip(reads_of(cfg_id), results_of(cfg_id)):
        fwd, rev, st, fc, rc = CM.read_hits(seq.tobytes(), kw["index"], kw["max_kfreq"])
        thr = float(res.threshold)
        c["no_kmers"] += st.size == 0
        c["thr_le_1"] += thr <= 1.0
        c["hits"] += fwd.size + rev.size > 0
        c["hits_thr_le_1"] += fwd.size + rev.size > 0 and thr <= 1.0   # the reads the fast path cannot certify: searched again
        c["votes_gt_65535"] += res.max_votes > 65535
        c["thr_eq_1"] += thr == 1.0
        c["thr_above_1"] += 1.0 < thr < 1.1
        c["thr_below_1"] += 0.0 < thr < 1.0
        c["max_votes"] = max(c["max_votes"], res.max_votes)
        c["votes_gt_255"] += res.max_votes > 255
        tot = fc + rc
        for name, v in (("kfreq_minus_1", kw["max_kfreq"] - 1), ("kfreq", kw["max_kfreq"]), ("kfreq_plus_1", kw["max_kfreq"] + 1)):
            c[name] += int(np.count_nonzero(tot == v))
        for name, v in (("cmrs_minus_1", cfg.cmrs - 1), ("cmrs", cfg.cmrs), ("cmrs_plus_1", cfg.cmrs + 1)):
            c[name] += res.accepted == v
        lists = tot if canonical else np.concatenate([fc, rc])
        for name, v in (("list_w_minus_2", w - 2), ("list_w_minus_1", w - 1), ("list_w", w)):
            c[name] += int(np.count_nonzero(lists == v))
        c["list_long"] += int(np.count_nonzero((lists > w) & (np.concatenate([tot, tot])[:len(lists)] < kw["max_kfreq"])))
        if st.size:
            v = CM.kmer_values(CM.CODE[seq], cfg.k)[st]
            c["palindromes"] += int(np.count_nonzero((v == CM.revcomp_kmer(v, cfg.k)) & (fc > 0)))
        if fwd.size and rev.size:
            fb, fv = np.unique(fwd, return_counts=True)
            rb, rv = np.unique(rev, return_counts=True)
            both, fi, ri = np.intersect1d(fb, rb, return_indices=True)
            f, r = fv[fi].astype(np.float32), rv[ri].astype(np.float32)
            c["strand_tie"] += bool(np.any((f == r) & (f >= res.threshold)))
            c["one_strand"] += bool(np.any((f >= res.threshold) != (r >= res.threshold)))
        if fwd.size + rev.size:
            # an accepted (bin, strand) that no single k-mer's list carries to the threshold: every k-mer voting for it has a list of two
            # or more entries (a repeat), at least two k-mers vote, and each gives fewer votes than the threshold asks for
            ok = tot < kw["max_kfreq"]
            kid = np.arange(len(st))
            key = np.concatenate([fwd * 2, rev * 2 + 1])
            who = np.concatenate([np.repeat(kid, np.where(ok, fc, 0)), np.repeat(kid, np.where(ok, rc, 0))])
            lens = np.concatenate([np.repeat(fc, np.where(ok, fc, 0)), np.repeat(rc, np.where(ok, rc, 0))])
            pair, per = np.unique(np.stack([key, who], axis=1), axis=0, return_counts=True)      # votes of one k-mer for one (bin, strand)
            bins_, first = np.unique(pair[:, 0], return_index=True)
            votes = np.add.reduceat(per, first)
            most = np.maximum.reduceat(per, first)
            n_kmers = np.diff(np.append(first, len(per)))
            shortest = np.full(len(bins_), np.iinfo(np.int64).max)
            np.minimum.at(shortest, np.searchsorted(bins_, key), lens)
            c["repeat_bin"] += bool(np.any((votes.astype(np.float32) >= res.threshold) & (most.astype(np.float32) < res.threshold) & (n_kmers >= 2) & (shortest >= 2)))
    return {k2: int(v) for k2, v in c.items()}


def fasta_bytes(contigs=None):
    out = []
    for i, g in enumerate(genome() if contigs is None else contigs):
        out.append(b">chr%d\n" % (i + 1))
        b = g.tobytes()
        out.extend(b[o:o + 70] + b"\n" for o in range(0, len(b), 70))
    return b"".join(out)


def fastq_bytes(reads):
    return b"".join(b"@" + name.encode() + b"\n" + seq.tobytes() + b"\n+\n" + b"I" * len(seq) + b"\n" for name, seq in reads)


def sha256(b):
    return hashlib.sha256(b).hexdigest()


def concat_len():
    return HM.concat_genome(genome())[2]
