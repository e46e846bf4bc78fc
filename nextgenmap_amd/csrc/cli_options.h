// cli_options.h -- the options of `ngm-hip`: NextGenMap's option names and defaults (src/config/Options.h:13-105,
// src/config/Config.cpp:381-557), what this backend adds, and every refusal that needs no GPU.
#pragma once
#include <getopt.h>
#include <zlib.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ngm_hip.h"
#include "read_trim.h"

namespace ngm::cli {

struct Opts {
	std::string ref, qry, qry1, qry2, out, vcf;
	int paired = 0, min_insert = 0, max_insert = 1000, topn = 1, strata = 0;
	char pe_delimiter = '/';
	int device = 0, kmer = 13, kmer_skip = 2, bin_size = 2, mode = 0, corridor = -1, max_read_length = 0, min_mq = 0, max_kfreq = 0;
	int match = 10, mismatch = 15, gap_read = -1, gap_ref = -1, gap_extend = -1, affine = 0, hard_clip = 0, silent_clip = 0, no_unal = 0, fast_pairing = 0, broken_pairs = 0, max_cmrs = 2147483647;
	int skip_save = 0, bam = 0, workers = 2, serial_reader = 0, keep_tags = 0;
	int argos = 0, kmer_min_set = 0;
	int sort = 0;   // --sort (ours): the BAM coordinate-sorted on the GPU, with its .bai (csrc/bam_sort.cpp)
	int markdup = 0;   // --markdup (ours, with --sort): duplicates get flag 0x400 in the sorter's memory before the sort (csrc/markdup.h)
	std::string coverage;   // --coverage FILE (ours): the depth of the mapped primary records as bedGraph, made on the GPU (csrc/coverage.cpp)
	std::string snp, snp_frac_text = "0.8";   // --snp FILE (ours): SNP calls of the mapped primary records as VCF, made on the GPU (csrc/snp.cpp); --snp-min-frac as given
	long snp_min_cov = 10, snp_min_qual = 15;   // --snp-min-cov, --snp-min-qual
	double snp_min_frac = 0.8;
	std::string count, count_out;   // --count FILE, --count-out FILE (ours): T>C conversion counts per region of the BED file, made on the GPU (csrc/count.cpp)
	long count_min_qual = 27;       // --count-min-qual (slamdunk count's -q)
	std::string methyl, methyl_context = "all";   // --methyl FILE, --methyl-context (ours, with --bs-mapping): per-cytosine methylation calls as Bismark's cytosine report, made on the GPU (csrc/methyl.cpp)
	long methyl_min_qual = 5, methyl_min_depth = 1;   // --methyl-min-qual (MethylDackel's -p), --methyl-min-depth
	bool methyl_opts = false;       // one of the three --methyl-* options was given
	ngm::trim::Options trim;   // -5/--trim5, --max-polya (Options.h:103-104)
	float argos_min = 0.f;   // --argos-min-score (Default(ARGOS_MINSCORE, 0), Config.cpp:505)
	int bs_mapping = 0, bs_cutoff = 6, match_tt = -1, match_tc = -1, match_set = 0, mismatch_set = 0, slam_seq = 0;
	std::vector<int> devices;
	int shard_i = 0, shard_n = 1, shard_output = 0, keep_shards = 0;
	std::string rg[12];  // read group: ID CN DS DT FO KS LB PG PI PL PU SM (SAMWriter.cpp:46-80)
	int very_fast = 0, fast = 0, sensitive = 0, very_sensitive = 0, variant = NGM_VARIANT_OCL_GPU;
	float sensitivity = -1.f, kmer_min = 0.f, min_identity = 0.65f, min_residues = 0.5f;
	int batch = 1 << 18;
	int stats_fd = -1;   // --stats-fd (set by the parent of shard processes): this shard's int64[8] statistics go there
	int ref_score_buffer = -1;   // --reference-score-buffer: entries of NextGenMap's score buffer whose lost pairs are mirrored (-1: 1 024 with --affine, else 0 = none)
	std::string cmdline;
};

[[noreturn]] inline void die(const std::string &msg) { fprintf(stderr, "[ngm-hip] error: %s\n", msg.c_str()); exit(1); }
// (one fprintf per message: stdio locks the stream for the call, so the lines of the reader, the writer and the estimate's thread never interleave)
inline void info(const char *tag, const std::string &msg) { fprintf(stderr, "[%s] %s\n", tag, msg.c_str()); }

inline Opts parse(int argc, char **argv) {
	Opts o;
	for (int i = 1; i < argc; ++i) { if (i > 1) o.cmdline += " "; o.cmdline += argv[i]; }  // Config.cpp:565-574
	enum { KSKIP = 1000, HARD, SILENT, KMIN, MB, MMP, GRP, GFP, MAXCMRS, NOUNAL, NOPROG, MAXRL, BINSZ, MAXKF, VFAST, FAST, SENS, VSENS, DEVICE,
		SKIPSAVE, BATCH, VARIANT, SHARD, SHARDOUT, KEEPSHARDS, BAMOUT, WORKERS, SERIAL, AFFINE, GEP, PEDELIM, STRATA, BSMAP, BSCUT, MBTT, MBTC, SLAM, FASTPAIR, BROKENPAIRS, REFSCOREBUF, STATSFD, MAXPOLYA, RG0, RG_LAST = RG0 + 11, ARGOS, ARGOSMIN, VCF, KEEPTAGS, PARSEALL, SORTOUT, MARKDUP, COVERAGE, SNP, SNPCOV, SNPFRAC, SNPQUAL, COUNT, COUNTOUT, COUNTQUAL, METHYL, METHYLCTX, METHYLQUAL, METHYLDEPTH, UNSUPPORTED };
	static const option lo[] = {
		{"ref", required_argument, 0, 'r'}, {"qry", required_argument, 0, 'q'}, {"output", required_argument, 0, 'o'},
		{"cpu-threads", required_argument, 0, 't'}, {"gpu", no_argument, 0, 'g'}, {"sensitivity", required_argument, 0, 's'},
		{"kmer", required_argument, 0, 'k'}, {"kmer-skip", required_argument, 0, KSKIP}, {"max-consec-indels", required_argument, 0, 'C'},
		{"local", no_argument, 0, 'l'}, {"end-to-end", no_argument, 0, 'e'}, {"min-identity", required_argument, 0, 'i'},
		{"min-residues", required_argument, 0, 'R'}, {"min-mq", required_argument, 0, 'Q'}, {"hard-clip", no_argument, 0, HARD},
		{"silent-clip", no_argument, 0, SILENT}, {"kmer-min", required_argument, 0, KMIN}, {"match-bonus", required_argument, 0, MB},
		{"mismatch-penalty", required_argument, 0, MMP}, {"gap-read-penalty", required_argument, 0, GRP}, {"gap-ref-penalty", required_argument, 0, GFP},
		{"max-cmrs", required_argument, 0, MAXCMRS}, {"no-unal", no_argument, 0, NOUNAL}, {"no-progress", no_argument, 0, NOPROG},
		{"max-read-length", required_argument, 0, MAXRL}, {"bin-size", required_argument, 0, BINSZ}, {"max-kfreq", required_argument, 0, MAXKF},
		{"very-fast", no_argument, 0, VFAST}, {"fast", no_argument, 0, FAST}, {"sensitive", no_argument, 0, SENS}, {"very-sensitive", no_argument, 0, VSENS},
		{"device", required_argument, 0, DEVICE}, {"skip-save", no_argument, 0, SKIPSAVE}, {"batch-size", required_argument, 0, BATCH},
		{"kernel-variant", required_argument, 0, VARIANT}, {"shard", required_argument, 0, SHARD}, {"shard-output", no_argument, 0, SHARDOUT},
		{"keep-shards", no_argument, 0, KEEPSHARDS},
		{"qry1", required_argument, 0, '1'}, {"qry2", required_argument, 0, '2'}, {"paired", no_argument, 0, 'p'},
		{"min-insert-size", required_argument, 0, 'I'}, {"max-insert-size", required_argument, 0, 'X'}, {"pe-delimiter", required_argument, 0, PEDELIM},
		{"rg-id", required_argument, 0, RG0}, {"rg-cn", required_argument, 0, RG0 + 1}, {"rg-ds", required_argument, 0, RG0 + 2},
		{"rg-dt", required_argument, 0, RG0 + 3}, {"rg-fo", required_argument, 0, RG0 + 4}, {"rg-ks", required_argument, 0, RG0 + 5},
		{"rg-lb", required_argument, 0, RG0 + 6}, {"rg-pg", required_argument, 0, RG0 + 7}, {"rg-pi", required_argument, 0, RG0 + 8},
		{"rg-pl", required_argument, 0, RG0 + 9}, {"rg-pu", required_argument, 0, RG0 + 10}, {"rg-sm", required_argument, 0, RG0 + 11},
		{"fast-pairing", no_argument, 0, FASTPAIR}, {"broken-pairs", no_argument, 0, BROKENPAIRS}, {"reference-score-buffer", required_argument, 0, REFSCOREBUF}, {"stats-fd", required_argument, 0, STATSFD},
		{"affine", no_argument, 0, AFFINE}, {"gap-extend-penalty", required_argument, 0, GEP}, {"bam", no_argument, 0, BAMOUT}, {"workers", required_argument, 0, WORKERS}, {"serial-reader", no_argument, 0, SERIAL}, {"bs-mapping", no_argument, 0, BSMAP},
		{"bs-cutoff", required_argument, 0, BSCUT}, {"match-bonus-tt", required_argument, 0, MBTT}, {"match-bonus-tc", required_argument, 0, MBTC},
		{"slam-seq", required_argument, 0, SLAM}, {"topn", required_argument, 0, 'n'}, {"strata", no_argument, 0, STRATA},
		{"argos", no_argument, 0, ARGOS}, {"argos-min-score", required_argument, 0, ARGOSMIN}, {"vcf", required_argument, 0, VCF},
		{"keep-tags", no_argument, 0, KEEPTAGS}, {"parse-all", no_argument, 0, PARSEALL}, {"sort", no_argument, 0, SORTOUT}, {"markdup", no_argument, 0, MARKDUP}, {"coverage", required_argument, 0, COVERAGE},
		{"snp", required_argument, 0, SNP}, {"snp-min-cov", required_argument, 0, SNPCOV}, {"snp-min-frac", required_argument, 0, SNPFRAC}, {"snp-min-qual", required_argument, 0, SNPQUAL},
		{"count", required_argument, 0, COUNT}, {"count-out", required_argument, 0, COUNTOUT}, {"count-min-qual", required_argument, 0, COUNTQUAL},
		{"methyl", required_argument, 0, METHYL}, {"methyl-context", required_argument, 0, METHYLCTX}, {"methyl-min-qual", required_argument, 0, METHYLQUAL}, {"methyl-min-depth", required_argument, 0, METHYLDEPTH},
		{"trim5", required_argument, 0, '5'}, {"max-polya", required_argument, 0, MAXPOLYA}, {"config", required_argument, 0, UNSUPPORTED},
		{0, 0, 0, 0}};
	int c, idx = 0;
	while ((c = getopt_long(argc, argv, "o:q:r:t:gs:k:lei:R:C:Q:p1:2:I:X:n:bd:5:", lo, &idx)) != -1) {
		switch (c) {
		case 'r': o.ref = optarg; break;
		case 'q': o.qry = optarg; break;
		case '1': o.qry1 = optarg; break;
		case '2': o.qry2 = optarg; break;
		case 'p': o.paired = 1; break;
		case 'n': o.topn = std::max(1, atoi(optarg)); break;
		case STRATA: o.strata = 1; break;
		case 'I': o.min_insert = atoi(optarg); break;
		case 'X': o.max_insert = atoi(optarg); break;
		case PEDELIM: case 'd': o.pe_delimiter = optarg[0]; break;
		case '5': o.trim.trim5 = atoi(optarg); if (o.trim.trim5 < 0) die("-5/--trim5 expects a number of bases >= 0"); break;
		case MAXPOLYA: o.trim.max_polya = atoi(optarg); break;
		case 'o': o.out = optarg; break;
		case 't': break;  // host threads follow the machine (NGM_HIP_HOST_THREADS)
		case 'g':  // "-g" or "-g 0,1,..." (optional list without '=', src/config/Config.cpp:624-647); the GPU is not optional here
			if (optind < argc && argv[optind][0] >= '0' && argv[optind][0] <= '9') {
				o.devices.clear();
				for (const char *p = argv[optind]; *p;) { o.devices.push_back(atoi(p)); while (*p && *p != ',') ++p; if (*p == ',') ++p; }
				++optind;
			}
			break;
		case 's': o.sensitivity = (float) atof(optarg); break;
		case 'k': o.kmer = atoi(optarg); break;
		case KSKIP: o.kmer_skip = atoi(optarg); break;
		case 'C': o.corridor = 2 * atoi(optarg); break;  // Config.cpp:540-557
		case 'l': o.mode = 0; break;
		case 'e': o.mode = 1; break;
		case 'i': o.min_identity = (float) atof(optarg); break;
		case 'R': o.min_residues = (float) atof(optarg); break;
		case 'Q': o.min_mq = atoi(optarg); break;
		case HARD: o.hard_clip = 1; break;
		case SILENT: o.silent_clip = 1; break;
		case KMIN: o.kmer_min = (float) atof(optarg); o.kmer_min_set = 1; break;
		case MB: o.match = atoi(optarg); o.match_set = 1; break;
		case MMP: o.mismatch = atoi(optarg); o.mismatch_set = 1; break;
		case BSMAP: o.bs_mapping = 1; break;
		case SLAM: o.slam_seq = atoi(optarg); break;
		case BSCUT: o.bs_cutoff = atoi(optarg); break;
		case MBTT: o.match_tt = atoi(optarg); break;
		case MBTC: o.match_tc = atoi(optarg); break;
		case GRP: o.gap_read = atoi(optarg); break;
		case GFP: o.gap_ref = atoi(optarg); break;
		case AFFINE: o.affine = 1; break;
		case RG0: case RG0 + 1: case RG0 + 2: case RG0 + 3: case RG0 + 4: case RG0 + 5: case RG0 + 6: case RG0 + 7: case RG0 + 8: case RG0 + 9:
		case RG0 + 10: case RG0 + 11: o.rg[c - RG0] = optarg; break;
		case GEP: o.gap_extend = atoi(optarg); break;
		case MAXCMRS: o.max_cmrs = atoi(optarg); break;
		case NOUNAL: o.no_unal = 1; break;
		case NOPROG: break;
		case SKIPSAVE: o.skip_save = 1; break;
		case MAXRL: o.max_read_length = atoi(optarg); break;
		case BINSZ: o.bin_size = atoi(optarg); break;
		case MAXKF: o.max_kfreq = atoi(optarg); break;
		case VFAST: o.very_fast = 1; break;
		case FAST: o.fast = 1; break;
		case SENS: o.sensitive = 1; break;
		case VSENS: o.very_sensitive = 1; break;
		case DEVICE: o.device = atoi(optarg); o.devices.assign(1, o.device); break;
		case BAMOUT: case 'b': o.bam = 1; break;
		case WORKERS: o.workers = std::max(1, atoi(optarg)); break;
		case SERIAL: o.serial_reader = 1; break;
		case BATCH: o.batch = std::max(1024, atoi(optarg)); break;
		case VARIANT: o.variant = atoi(optarg) ? NGM_VARIANT_OCL_CPU : NGM_VARIANT_OCL_GPU; break;
		case SHARD: {  // "i/N": this process maps the i-th of N contiguous ranges of the input and writes their records (the header with shard 0)
			const char *sl = strchr(optarg, '/');
			o.shard_i = atoi(optarg); o.shard_n = sl ? atoi(sl + 1) : 0;
			if (!sl || o.shard_n < 1 || o.shard_i < 0 || o.shard_i >= o.shard_n) die("--shard expects i/N with 0 <= i < N");
			break;
		}
		case SHARDOUT: o.shard_output = 1; break;
		case KEEPSHARDS: o.keep_shards = 1; break;
		case FASTPAIR: o.fast_pairing = 1; break;
		case REFSCOREBUF: o.ref_score_buffer = std::max(0, atoi(optarg)); break;
		case STATSFD: o.stats_fd = atoi(optarg); break;
		case BROKENPAIRS: o.broken_pairs = 1; break;
		case ARGOS: o.argos = 1; break;
		case VCF: o.vcf = optarg; break;
		case KEEPTAGS: o.keep_tags = 1; break;   // (FASTA / FASTQ records have no tags: refused only with SAM / BAM input, in main)
		case PARSEALL: break;                    // every record of a SAM / BAM input is a read: the default (Config.cpp:489)
		case ARGOSMIN: o.argos_min = (float) atof(optarg); break;
		case SORTOUT: o.sort = 1; break;
		case MARKDUP: o.markdup = 1; break;
		case COVERAGE: o.coverage = optarg; if (o.coverage.empty()) die("--coverage expects a file name"); break;
		case SNP: o.snp = optarg; if (o.snp.empty()) die("--snp expects a file name"); break;
		case SNPCOV: { char *e = nullptr; o.snp_min_cov = strtol(optarg, &e, 10); if (e == optarg || *e || o.snp_min_cov < 0 || o.snp_min_cov > 2147483647L) die("--snp-min-cov expects a count of 0 or more"); break; }
		case SNPFRAC: { char *e = nullptr; o.snp_min_frac = strtod(optarg, &e); o.snp_frac_text = optarg; if (e == optarg || *e || !(o.snp_min_frac > 0.0 && o.snp_min_frac <= 1.0)) die("--snp-min-frac expects a fraction in (0, 1]"); break; }
		case SNPQUAL: { char *e = nullptr; o.snp_min_qual = strtol(optarg, &e, 10); if (e == optarg || *e || o.snp_min_qual < 0 || o.snp_min_qual > 93) die("--snp-min-qual expects a Phred quality in 0..93"); break; }
		case COUNT: o.count = optarg; if (o.count.empty()) die("--count expects a BED file name"); break;
		case COUNTOUT: o.count_out = optarg; if (o.count_out.empty()) die("--count-out expects a file name"); break;
		case METHYL: o.methyl = optarg; if (o.methyl.empty()) die("--methyl expects a file name"); break;
		case METHYLCTX:
			o.methyl_context = optarg; o.methyl_opts = true;
			if (o.methyl_context != "all" && o.methyl_context != "CpG" && o.methyl_context != "CHG" && o.methyl_context != "CHH") die("--methyl-context expects all, CpG, CHG or CHH, not " + o.methyl_context);
			break;
		case METHYLQUAL: { char *e = nullptr; o.methyl_opts = true; o.methyl_min_qual = strtol(optarg, &e, 10); if (e == optarg || *e || o.methyl_min_qual < 0 || o.methyl_min_qual > 93) die("--methyl-min-qual expects a Phred quality in 0..93"); break; }
		case METHYLDEPTH: { char *e = nullptr; o.methyl_opts = true; o.methyl_min_depth = strtol(optarg, &e, 10); if (e == optarg || *e || o.methyl_min_depth < 0 || o.methyl_min_depth > 2147483647L) die("--methyl-min-depth expects a count of 0 or more"); break; }
		case COUNTQUAL: { char *e = nullptr; o.count_min_qual = strtol(optarg, &e, 10); if (e == optarg || *e || o.count_min_qual < 0 || o.count_min_qual > 93) die("--count-min-qual expects a Phred quality in 0..93"); break; }
		case UNSUPPORTED: die(std::string("option --") + lo[idx].name + " is not supported by the HIP backend yet");
		default: die("unknown option (see src/config/Options.h of NextGenMap for the option set)");
		}
	}
	if (o.ref.empty()) die("no reference given (-r/--ref)");
	if (o.markdup && !o.sort) die("--markdup needs --sort: duplicates are found among the records the sorter holds");
	if (o.sort) {
		// the sort is over the records of the whole run, kept in the first GPU's memory; refused before any GPU work
		if (o.argos) die("--sort cannot be combined with --argos: argos output is text lines, not BAM records");
		if (!o.bam) die("--sort needs -b/--bam: the sorted output is a BAM file with its .bai index (sorted SAM text is not written)");
		if (o.shard_n > 1) die("--sort cannot be combined with --shard: the sort is over the whole run, not over one shard of it");
		if (o.shard_output) die("--sort cannot be combined with --shard-output: the sort is over the whole run, in one process");
		if (getenv("NGM_HIP_BAM_ZLIB")) die("--sort cannot be combined with NGM_HIP_BAM_ZLIB=1: the blocks of a sorted file only come from the GPU");
	}
	if (!o.coverage.empty()) {
		// the depth is over the records of the whole run, counted in the first GPU's memory; refused before any GPU work
		if (o.argos) die("--coverage cannot be combined with --argos: argos scores candidates, no alignments are made");
		if (o.shard_n > 1) die("--coverage cannot be combined with --shard: the depth is over the whole run, not over one shard of it");
		if (o.shard_output) die("--coverage cannot be combined with --shard-output: the depth is over the whole run, in one process");
		if (o.coverage == o.out) die("--coverage cannot write to the -o/--output file: " + o.out);
	}
	if (!o.snp.empty()) {
		// the pileup is over the records of the whole run, counted in the first GPU's memory; refused before any GPU work
		if (o.argos) die("--snp cannot be combined with --argos: argos scores candidates, no alignments are made");
		if (o.shard_n > 1) die("--snp cannot be combined with --shard: the pileup is over the whole run, not over one shard of it");
		if (o.shard_output) die("--snp cannot be combined with --shard-output: the pileup is over the whole run, in one process");
		if (o.bs_mapping) die("--snp cannot be combined with --bs-mapping: bisulfite conversions are not variants, and a strand-aware pileup is not built");
		if (!o.vcf.empty()) die("--snp cannot be combined with --vcf: calling over an index built with known variants is not checked");
		if (o.snp == o.out) die("--snp cannot be combined with -o " + o.out + ": the calls and the records need a file each");
		if (o.snp == o.coverage) die("--snp cannot be combined with --coverage " + o.coverage + ": the calls and the depth need a file each");
	}
	if (!o.methyl.empty() || o.methyl_opts) {
		// the calls are over the records of the whole run, counted in the first GPU's memory; refused before any GPU work
		if (o.methyl.empty()) die("--methyl-context, --methyl-min-qual and --methyl-min-depth need --methyl FILE: where the report is written");
		if (!o.bs_mapping) die("--methyl needs --bs-mapping: only a bisulfite run's records say which strand a read was converted on");
		if (o.argos) die("--methyl cannot be combined with --argos: argos scores candidates, no alignments are made");
		if (o.shard_n > 1) die("--methyl cannot be combined with --shard: the calls are over the whole run, not over one shard of it");
		if (o.shard_output) die("--methyl cannot be combined with --shard-output: the calls are over the whole run, in one process");
		if (o.methyl == o.out) die("--methyl cannot be combined with -o " + o.out + ": the report and the records need a file each");
		if (o.methyl == o.coverage) die("--methyl cannot be combined with --coverage " + o.coverage + ": the report and the depth need a file each");
	}
	if (!o.count.empty() || !o.count_out.empty()) {
		// the counts are over the records of the whole run, kept in the first GPU's memory; refused before any GPU work
		if (o.count.empty()) die("--count-out needs --count FILE: the BED file of the regions to count in");
		if (o.count_out.empty()) die("--count needs --count-out FILE: where the counts are written");
		if (o.argos) die("--count cannot be combined with --argos: argos scores candidates, no alignments are made");
		if (o.shard_n > 1) die("--count cannot be combined with --shard: the counts are over the whole run, not over one shard of it");
		if (o.shard_output) die("--count cannot be combined with --shard-output: the counts are over the whole run, in one process");
		if (o.bs_mapping) die("--count cannot be combined with --bs-mapping: bisulfite conversions are not SLAM-seq labelling, and they are not told apart");
		if (o.count_out == o.out) die("--count cannot be combined with -o " + o.out + ": the counts and the records need a file each");
		if (o.count_out == o.coverage) die("--count cannot be combined with --coverage " + o.coverage + ": the counts and the depth need a file each");
		if (o.count_out == o.snp) die("--count cannot be combined with --snp " + o.snp + ": the counts and the calls need a file each");
	}
	if (o.argos) {
		// ScoreWriter has no paired or binary form (DoWritePair throws, src/writer/ScoreWriter.cpp:75-77); refused before any GPU work
		if (!o.qry1.empty() || !o.qry2.empty()) die("--argos cannot be combined with --qry1/--qry2: the argos writer is single-end only (ScoreWriter::DoWritePair is not implemented)");
		if (o.paired) die("--argos cannot be combined with -p/--paired: the argos writer is single-end only (ScoreWriter::DoWritePair is not implemented)");
		if (o.bam) die("--argos cannot be combined with --bam: argos output is text lines, not SAM records");
		if (o.shard_n > 1) die("--argos cannot be combined with --shard: the prolog's read count and the single output file belong to the whole input");
		if (o.shard_output) die("--argos cannot be combined with --shard-output: the argos lines are written by one process in input order");
		if (o.bs_mapping) die("--argos cannot be combined with --bs-mapping: that combination is not supported by the HIP backend");
		if (o.slam_seq) die("--argos cannot be combined with --slam-seq: that combination is not supported by the HIP backend");
		if (o.trim.max_polya >= 0) die("--argos cannot be combined with --max-polya: that combination is not checked against the reference and not supported by the HIP backend");
		// Config.cpp:384-388, :517-520: kmer_min 2 and sensitivity 0 unless given; no selection, so -n / --strata / -Q / the identity and
		// residue filters have no effect (ScoreBuffer.cpp:150-183 hands every scored read to the writer)
		if (!o.kmer_min_set) o.kmer_min = 2.f;
		if (o.sensitivity < 0) o.sensitivity = 0.f;
		o.topn = 1; o.strata = 0; o.min_mq = 0;
	}
	if (!o.qry1.empty() && !o.qry2.empty()) o.paired = 1;  // Config.cpp:395-399
	else if (!o.qry1.empty() || !o.qry2.empty()) die("--qry1 and --qry2 must be given together");
	if (o.paired && o.topn > 1) die("Paired end mode with topn > 1 not yet supported.");  // ScoreBuffer::topNPE
	if (o.paired && o.qry.empty() && o.qry1.empty()) die("-p/--paired needs -q (interleaved mates) or --qry1/--qry2");
	if (!o.vcf.empty()) {
		// (the reference builds a bisulfite index with the VCF's k-mers unconverted; that combination is not restated here)
		if (o.bs_mapping) die("--vcf cannot be combined with --bs-mapping: that combination is not supported by the HIP backend");
		// an index built with a VCF holds lists out of genome order, repeated positions and zero slots (refindex.h); the modes below are
		// not yet checked against the reference with such an index and are refused rather than run unchecked.  --argos would print
		// the candidates of the zero slots, where the reference's convert() reads past its contig table (SequenceProvider.cpp:115-119)
		const char *why = o.argos ? "--argos" : o.bam ? "--bam" : o.topn > 1 ? "-n/--topn above 1" : o.mode == 1 ? "-e/--end-to-end" :
				o.devices.size() > 1 ? "several GPUs (-g a,b,..)" : o.shard_output ? "--shard-output" : o.shard_n > 1 ? "--shard" : o.bin_size < 2 ? "--bin-size below 2" :
				o.trim.max_polya >= 0 ? "--max-polya" : nullptr;
		if (why) die(std::string("--vcf cannot be combined with ") + why + ": that combination is not supported by the HIP backend yet");
		gzFile vf = gzopen(o.vcf.c_str(), "rb");  // before any GPU work (the reference logs an unreadable VCF and goes on without it)
		if (!vf) die("Failed to open VCF file " + o.vcf);
		gzclose(vf);
	}
	// scoring defaults depend on the personality (Config.cpp:433-470)
	if (o.bs_mapping) {
		info("MAIN", "Using bs-mapping scoring scheme");
		if (o.affine) die("'--bs-mapping' and '--affine' can't be used at the same time!");
		if (o.mode == 1) die("'--bs-mapping' and '--e/--end-to-end' can't be used at the same time!");
		if (!o.match_set) o.match = 4;
		if (!o.mismatch_set) o.mismatch = 2;
		if (o.gap_read < 0) o.gap_read = 10;
		if (o.gap_ref < 0) o.gap_ref = 10;
		if (o.gap_extend < 0) o.gap_extend = 2;
		if (o.match_tt < 0) o.match_tt = 4;
		if (o.match_tc < 0) o.match_tc = 4;
	}
	if (o.slam_seq) {
		if (o.bs_mapping) die("'--bs-mapping' and '--slam-seq' can't be used at the same time!");   // Config.cpp:454-457
		if (o.affine) die("'--slam-seq' needs the default (linear-gap) scoring: the affine backend produces no per-base records");
	}
	if (o.match_tt < 0) o.match_tt = 10;
	if (o.match_tc < 0) o.match_tc = 2;
	if (o.gap_read < 0) o.gap_read = o.affine ? 33 : 20;
	if (o.gap_ref < 0) o.gap_ref = o.affine ? 33 : 20;
	if (o.gap_extend < 0) o.gap_extend = o.affine ? 3 : 5;
	// the pairs NextGenMap loses (ngm_mapper_set_reference_score_buffer): its SeqAn personality scores in batches of 1 024
	// (src/seqan/EndToEndAffine.h:44-46); the OpenCL personality's batch depends on the device it finds -- nothing to mirror by default
	// The walk that finds those pairs is sequential over the WHOLE input (it follows the reference's CS batches and score-buffer fill from
	// the first read on, as `ngm -t 1` does): a shard that starts in the middle of the input cannot know where the reference's buffer
	// stands at its first read, would lose pairs the reference keeps, and `cat shards` would no longer equal the single run.
	// Sharded runs therefore never mirror them.
	if (o.shard_n > 1) {
		if (o.ref_score_buffer > 0) fprintf(stderr, "[MAIN] --reference-score-buffer is ignored with --shard: the reference's score buffer cannot be followed from the middle of the input\n");
		o.ref_score_buffer = 0;
	}
	if (o.ref_score_buffer < 0) o.ref_score_buffer = o.affine ? 1024 : 0;
	if (o.devices.empty()) o.devices.assign(1, o.device);
	o.device = o.devices[0];
	if (o.broken_pairs) {
		if (!(o.paired && !o.qry.empty())) die("--broken-pairs only works with interleaved paired-end files.");   // ReadProvider.cpp:176-179
		if (o.shard_n > 1 || o.shard_output) die("--broken-pairs cannot be combined with --shard / --shard-output: the pairing of the records is decided while they are read");
		o.serial_reader = 1;   // which records are mates is decided record by record (ReadProvider.cpp:540-575)
	}
	return o;
}
// info() with printf's formatting
__attribute__((format(printf, 2, 3))) inline void infof(const char *tag, const char *fmt, ...) { char m[512]; va_list ap; va_start(ap, fmt); vsnprintf(m, sizeof(m), fmt, ap); va_end(ap); info(tag, m); }

}  // namespace ngm::cli
