/*
 * ngm_pipeline.h -- flat C ABI of the device-resident mapping path that sits ABOVE IAlignment in
 * NextGenMap: encoded reference + k-mer index in HBM, candidate search, window gather, score,
 * candidate selection / MAPQ, alignment.  Rows a1-a5, a7, a8 of SURVEY.md section 8.
 *
 * Reference interfaces replaced (paths relative to the NextGenMap tree):
 *   ngm_ref_*        <- _SequenceProvider (src/SequenceProvider.cpp:228-441: 4-bit concatenated genome with
 *                       1000-N spacers, DecodeRefSequence, convert) and CompactPrefixTable
 *                       (src/PrefixTable.cpp:328-498, :641-817: k-mer index, GetRefEntry, stats/max_kfreq)
 *   ngm_mapper_cs    <- CS::RunBatch / PrefixSearch / AddLocationStd / CollectResultsStd (src/CS.cpp:114-313)
 *   ngm_mapper_map   <- ScoreBuffer::DoRun + top1SE + computeMQ (src/ScoreBuffer.cpp:34-49, :80-277) and
 *                       AlignmentBuffer::DoRun (src/AlignmentBuffer.cpp:64-147) around BatchScore / BatchAlign
 * Plain pointers and sizes only.  All functions return >= 0 on success, a negative errno-style value on
 * failure (ngm_pipeline_last_error() describes it).  No CPU fallback: a HIP device is required.
 */
#ifndef NGM_PIPELINE_H
#define NGM_PIPELINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ngm_ref ngm_ref;
typedef struct ngm_mapper ngm_mapper;

typedef struct ngm_ref_params {
	int kmer;        /* Config "kmer", default 13 (src/config/Config.cpp:383); 4..15 supported here */
	int kmer_skip;   /* Config "kmer_skip", default 2: every (skip+1)-th reference k-mer is indexed */
	int bin_size;    /* Config "bin_size", default 2: candidate bins are 2^bin_size bases wide */
} ngm_ref_params;

const char *ngm_pipeline_last_error(void);

/* Encode a reference (contigs in order; names NUL-terminated; sequences ASCII, any case, non-ACGT -> N;
 * contigs of length <= 10 are skipped like the reference does, SequenceProvider.h:71) and build its
 * k-mer index on `device`. */
ngm_ref *ngm_ref_create(int device, const ngm_ref_params *p, int n_contigs, const char *const *names,
		const uint8_t *const *seqs, const uint64_t *lens);
/* Same, reading a (optionally gzip-compressed) FASTA file. */
ngm_ref *ngm_ref_create_from_fasta(int device, const ngm_ref_params *p, const char *path);
/* Loads NextGenMap's own cache files next to fasta_path -- <fasta>-enc.2.ngm (SequenceProvider.cpp:189-262) and
 * <fasta>-ht-<kmer>-<kmer_skip>.3.ngm (PrefixTable.cpp:819-930) -- written by `ngm` or by ngm_ref_write_ngm_cache, so
 * an existing NextGenMap index drops in.  NULL when absent / built with other parameters / multi-unit.
 * ngm_ref_create_from_fasta tries this first, like the reference (NGM_HIP_NO_CACHE=1 forces a rebuild). */
ngm_ref *ngm_ref_create_from_cache(int device, const ngm_ref_params *params, const char *fasta_path);
/* 1 when the reference came from those cache files (a corrupt / mismatching cache falls back to a build: the caller rewrites it) */
int ngm_ref_loaded_from_cache(const ngm_ref *r);
/* --vcf FILE (PrefixTable.cpp:223-228, :500-574): the index also holds the k-mers of the VCF's variants, built like the reference
 * builds them -- lists in genome order then VCF order, and the zero slots the reference leaves where its fill pass stores less than
 * its count pass reserved.  Plain or gzip VCF.  An existing cache is loaded as it is and the VCF is not read (like the reference);
 * an unreadable VCF, or a variant whose region would start before position 0 or past the end of the genome, is an error (the
 * reference goes on without variants, or reads outside its buffers). */
ngm_ref *ngm_ref_create_from_fasta_vcf(int device, const ngm_ref_params *params, const char *fasta_path, const char *vcf_path);
/* out: variations loaded, SNPs, indels, ignored (the `Loaded VCF` / `Built SNP region table` lines), region entries stored, zero
 * slots.  Returns 1 when the index was built with a VCF, 0 when not (no VCF, or loaded from a cache), < 0 on a bad argument. */
int ngm_ref_vcf_summary(const ngm_ref *r, uint64_t out[6]);
/* the reference's skipCount and skipBuild of a build with a VCF (they differ where the zero slots come from); return as above */
int ngm_ref_vcf_skip_counts(const ngm_ref *r, uint64_t out[2]);
void ngm_ref_destroy(ngm_ref *r);

int ngm_ref_contig_count(const ngm_ref *r);
const char *ngm_ref_contig_name(const ngm_ref *r, int i);
uint64_t ngm_ref_contig_start(const ngm_ref *r, int i); /* position in concatenated coordinates */
uint64_t ngm_ref_contig_len(const ngm_ref *r, int i);
uint64_t ngm_ref_concat_len(const ngm_ref *r);          /* _SequenceProvider::GetConcatRefLen */
int ngm_ref_auto_max_kfreq(const ngm_ref *r);           /* ceil(max(100, avg + 5 sigma)), PrefixTable.cpp:150-194 */
uint64_t ngm_ref_index_entries(const ngm_ref *r);       /* number of stored k-mer positions */
/* copy the index out (tests): counts[4^k] = list length per k-mer as a lookup sees it (0 for k-mers
 * disabled by the 9900-occurrence rule, PrefixTable.cpp:468-478), raw_counts[4^k] = before that rule,
 * positions[index_entries] grouped by k-mer in k-mer order, ascending inside a group. NULL = skip. */
int ngm_ref_index_copy(const ngm_ref *r, uint32_t *counts, uint32_t *raw_counts, uint32_t *positions);
/* _SequenceProvider::DecodeRefSequence(buffer, 0, offset, buffer_len) executed from the HBM copy. */
int ngm_ref_decode(const ngm_ref *r, uint64_t offset, int buffer_len, char *out);
/* _SequenceProvider::convert: concatenated position -> (contig, 0-based position); returns 0 when the
 * position lies in a spacer (reported unmapped), 1 otherwise. */
int ngm_ref_convert(const ngm_ref *r, uint64_t pos, int *contig, uint64_t *contig_pos);

/* n symbol classes (A0 C1 G2 T3 x4 N5) of the encoded genome from concatenated position `pos` on, from the host copy (what a
 * record formatter needs to label the columns of an alignment, e.g. for the SLAM-seq tags); returns the number copied. */
int ngm_ref_host_classes(const ngm_ref *r, uint64_t pos, int n, uint8_t *out);

/* Builds the index layout the candidate search gathers from (one bucket per k-mer pair for odd k) now instead
 * of when the first mapper is created: part of preparing the reference, like loading NextGenMap's cache files
 * (src/PrefixTable.cpp:232-262).  bs_mapping != 0: nothing to build (that mode runs the exact search).  0, or -errno. */
int ngm_ref_prepare_search(ngm_ref *ref, int bs_mapping);

/* Write NextGenMap's own cache files next to `fasta_path` so that the reference program loads this encoded
 * genome and index instead of rebuilding them: <fasta_path>-enc.2.ngm (src/SequenceProvider.cpp:189-208) and
 * <fasta_path>-ht-<k>-<skip>.3.ngm (src/PrefixTable.cpp:819-855).  Content is what NGM itself would write. */
int ngm_ref_write_ngm_cache(const ngm_ref *r, const char *fasta_path);

typedef struct ngm_mapper_params {
	int qry_max_len;       /* bytes per read row */
	int corridor;
	int match_bonus, mismatch_penalty, gap_read_penalty, gap_ref_penalty;
	int mode;              /* 0 local, 1 end-to-end */
	int variant;           /* NGM_VARIANT_* of ngm_hip.h */
	float sensitivity;     /* Config "sensitivity" (-s) */
	float kmer_min;        /* Config "kmer_min" */
	int max_cmrs;          /* Config "max_cmrs" (INT_MAX = unlimited) */
	int max_kfreq;         /* <= 0: use ngm_ref_auto_max_kfreq */
	int hard_clip, silent_clip;
	int personality;       /* NGM_PERSONALITY_* of ngm_hip.h: 1 = `--affine` (EndToEndAffine / SeqAn scoring and CIGARs) */
	int gap_extend_penalty; /* Config "gap_extend_penalty" (affine personality) */
	/* paired-end selection (ScoreBuffer::top1PE / CheckPairs, src/ScoreBuffer.cpp:368-502) */
	int min_insert_size;   /* Config "min_insert_size" (-I), default 0 */
	int max_insert_size;   /* Config "max_insert_size" (-X), default 1000; <= 0: unlimited (src/NGM.cpp:38-41) */
	float pair_score_cutoff; /* Config "pair_score_cutoff"; <= 0: 0.9 */
	/* ScoreBuffer::topNSE (src/ScoreBuffer.cpp:279-327), single-end only as in the reference */
	int topn;              /* Config "topn" (-n): alignments reported per read; <= 1: one */
	int strata;            /* Config "strata": only the equally best ones, none if there are more than topn */
	/* `--bs-mapping` (src/CS.cpp:54-112, :340-376, :553-560; lib/mason/opencl/SWOcl.cpp:225-232): candidate search looks every read
	 * k-mer up in all its T>C (second mates: A>G) conversions, scoring uses the strand-specific tables.  The reference index must
	 * have been built with kmer_skip 0 (src/PrefixTable.cpp:199-207); the run's "kmer_skip" applies to the read instead. */
	int bs_mapping;        /* Config "bs_mapping" */
	int bs_cutoff;         /* Config "bs_cutoff" (6): k-mers with more convertible bases are not looked up */
	int bs_read_skip;      /* Config "kmer_skip" of the run (2) */
	int match_bonus_tt, match_bonus_tc;   /* Config MATCH_BONUS_TT / MATCH_BONUS_TC (4 / 4) */
	/* `--slam-seq <n>` (Config SLAM_SEQ): any value makes computeCigarMD count T>C (reverse strand: A>G) columns as matches and the
	 * writer add TC / RA / MP tags; bit 1 (2) also switches the score tables (scoresSlamSeqFWD / REV, match_bonus_tt / -match_bonus_tc);
	 * bit 2 (4): the weighted k-mer mutation search (src/CS.cpp:57-92, :133-138) -- every read k-mer and its single C > T (second mates
	 * G > A) conversions, float votes of 1 / (convertible bases + 1) summed in the reference's order (csrc/cs_slam_device.h). */
	int slam_seq;
} ngm_mapper_params;

/* Refused (NULL, ngm_pipeline_last_error): a combination in which one (bin, strand) of a read could collect more than 65 535 votes, which
 * the search's vote tables do not hold -- (qry_max_len - kmer) * min(max_kfreq - 1, 2^(bin_size - 1)) > 65535, i.e. bin_size 8 with
 * qry_max_len - kmer of 512 or more (unless max_kfreq is below 129).  The reference program counts such bins; use a smaller bin_size. */
ngm_mapper *ngm_mapper_create(const ngm_ref *ref, const ngm_mapper_params *p);
void ngm_mapper_destroy(ngm_mapper *m);

/* Candidate search for n reads (reads: n rows of qry_max_len bytes, upper-case ACGTN, NUL padded, host
 * memory).  Outputs: cand_offsets[n+1] (prefix sums), max_votes[n] (read->s, SAM XE:i); the candidates
 * themselves are fetched with ngm_mapper_cs_fetch: loc = bin centre in concatenated coordinates
 * (ResolveBin), strand 0/1, votes.  Candidate order inside a read is (loc, strand) ascending -- the
 * reference's order is first-threshold-crossing order, which only matters for exact score ties. */
int ngm_mapper_cs(ngm_mapper *m, int n, const char *reads, uint32_t *cand_offsets, float *max_votes);
int ngm_mapper_cs_fetch(ngm_mapper *m, uint64_t *loc, uint8_t *strand, float *votes);

/* after ngm_mapper_cs: per read, the largest forward + reverse vote sum of any bin -- what the reference's
 * sensitivity estimate is built from (ReadProvider.cpp:57-77, :79-124). out: n floats. */
int ngm_mapper_cs_max_combined(ngm_mapper *m, float *out);

/* Per-read mapping result (single-end, topn = 1). */
typedef struct ngm_hit {
	int mapped;            /* 0: no candidate / no alignment */
	int contig;            /* index into the reference contigs */
	uint64_t pos;          /* 0-based leftmost position on the contig */
	int reverse;           /* 1: read aligned as reverse complement */
	int mapq;
	float score;           /* AS:i (from the score stage, like the reference: SAMWriter.cpp:169) */
	float identity;        /* XI:f */
	int nm;
	int qstart, qend;
	int n_candidates;      /* CMRs scored for this read */
	int n_best;            /* NH:i / X0:i : candidates sharing the best score */
	float max_votes;       /* XE:i */
	int pair_flags;        /* paired-end runs: NGM_PAIR_* */
} ngm_hit;

#define NGM_PAIR_SELECTED 1  /* top1PE found a pair inside the insert-size window; n_best = pairs sharing its score and distance */
#define NGM_PAIR_FAILED 2    /* both mates had candidates but no such pair: NGMNames::PairedFail, mates selected single-end */
#define NGM_PAIR_LOST 4      /* the reference never writes this pair (ngm_mapper_set_reference_score_buffer): no record for either mate */

/* Full single-end path for n reads; cigars/mds: n rows of 4*qry_max_len bytes (NUL-terminated strings).
 * With topn > 1 every read owns topn consecutive entries of hits / rows of cigars and mds (entry k = k-th best
 * candidate, unused entries have mapped = 0 and n_candidates as usual); mapq and n_best are the read's. */
int ngm_mapper_map_se(ngm_mapper *m, int n, const char *reads, ngm_hit *hits, char *cigars, char *mds);
/* Same, with the read batch already resident in HBM (d_reads: n rows of qry_max_len bytes, device memory on
 * the mapper's GPU); `reads` is the host copy the CIGAR/MD pass consults.  What bench.py times. */
int ngm_mapper_map_se_resident(ngm_mapper *m, int n, const char *reads, const void *d_reads, ngm_hit *hits, char *cigars,
		char *mds);

/* Paired-end path: reads 2i and 2i+1 are mates (ReadProvider::GenerateRead, src/ReadProvider.cpp:526-584).
 * Candidate search, scoring and alignment are per read as above; the selection is ScoreBuffer::top1PE: among the
 * candidates within pair_score_cutoff of each mate's best, the best-scoring pair whose insert size lies inside
 * (min_insert_size, max_insert_size), ties by closeness to the running mean insert size (which is carried across
 * calls, like the reference's per-thread state).  MAPQ of a mate = its own best vs second-best candidate.
 * What the writer derives from both mates (proper-pair check, TLEN, flags) is the caller's: ngm-hip does it. */
int ngm_mapper_map_pe(ngm_mapper *m, int n, const char *reads, ngm_hit *hits, char *cigars, char *mds);
int ngm_mapper_map_pe_resident(ngm_mapper *m, int n, const char *reads, const void *d_reads, ngm_hit *hits, char *cigars,
		char *mds);

/* The SAM text of a batch, assembled on the GPU (csrc/sam_device.h): what GenericReadWriter::WriteRead / WritePair
 * (src/writer/GenericReadWriter.h:190-304: min_identity / min_residues / min_mq filters), AlignmentBuffer::WriteRead's
 * proper-pair check (src/AlignmentBuffer.cpp:175-199) and SAMWriter::DoWriteReadGeneric / DoWriteUnmappedReadGeneric /
 * DoWritePair (src/writer/SAMWriter.cpp:98-372) produce for the reads of one ngm_mapper_map_* call, records in input order
 * (the two records of a pair: mate 2 first, as the reference writes them).  Single alignments per read (topn <= 1). */
typedef struct ngm_sam_options {
	int paired;                 /* the calls map pairs (reads 2i, 2i + 1) */
	int min_insert_size, max_insert_size;   /* the writer's proper-pair window (max <= 0: unlimited) */
	int min_mq;                 /* Config "min_mq" */
	float min_identity, min_residues;       /* Config "min_identity" (0.65), "min_residues" (0.5; <= 1: share of the read length) */
	int no_unal;                /* Config "no_unal": unmapped reads are not written */
	const char *rg_id;          /* read group id for the RG:Z tag, or NULL */
	int bs_mapping;             /* Config "bs_mapping": the ZS:Z tag (src/writer/SAMWriter.cpp:173-187) */
	int slam_seq;               /* Config SLAM_SEQ != 0: the TC:i / RA:Z / MP:Z tags (src/writer/SAMWriter.cpp:203-221, GenericReadWriter.h:87-186) */
	int bam;                    /* Config "bam": the records as BAM (src/writer/BAMWriter.cpp:147-375), in BGZF blocks written by the GPU -- what
	                             * ngm_mapper_map_sam returns is then a piece of the BAM file (whole BGZF members); with slam_seq the TC:i / RA:Z /
	                             * MP:Z tags follow RG (src/writer/BAMWriter.cpp:273-292) */
} ngm_sam_options;
int ngm_mapper_set_sam_options(ngm_mapper *m, const ngm_sam_options *o);
typedef struct ngm_sam_read {   /* per read: where its name is, how long its quality string is */
	uint32_t name_off;          /* into `names` */
	uint16_t name_len;
	uint16_t qual_len;          /* bytes of the quality string the parser holds (the row holds the first qry_max_len - 1 of them); 0: none ('*');
	                             * bit 15 set: the read has no sequence and is discarded (NGMNames::Empty, GenericReadWriter.h:245-252) */
} ngm_sam_read;
/* Maps the batch like ngm_mapper_map_se / _pe and formats it.  reads, quals: n rows of qry_max_len bytes (page-locked memory
 * makes the copies asynchronous); names: names_bytes bytes; out: out_cap bytes for the text.  Returns the length of the text
 * (> out_cap: nothing was copied -- call ngm_mapper_sam_fetch with a larger buffer), or < 0.  stats: reads counted, reads
 * mapped, lines written.  kernel_ms (optional): GPU time of the formatting kernels. */
long long ngm_mapper_map_sam(ngm_mapper *m, int n, const char *reads, const char *quals, const char *names, size_t names_bytes,
		const ngm_sam_read *meta, char *out, size_t out_cap, uint64_t stats[3], float *kernel_ms);
/* The same for reads the caller has trimmed (`ngm -5 / --max-polya`: the rows and quality rows hold the trimmed read, as for every
 * entry point).  polya_trimmed: per read, the bases --max-polya cut off (MappedRead::polyATrimmed, src/ReadProvider.cpp:428-443);
 * non-null: every record carries it as XA:i (src/writer/SAMWriter.cpp:192-194, :355-357; BAMWriter.cpp:258-260, :356-358), 0 included.
 * NULL: no XA:i tag -- ngm_mapper_map_sam is this call with NULL.  A read whose row is empty (all NUL) is legal: it has no candidates
 * and is written as an unmapped record with empty SEQ and QUAL. */
long long ngm_mapper_map_sam_trimmed(ngm_mapper *m, int n, const char *reads, const char *quals, const char *names, size_t names_bytes,
		const ngm_sam_read *meta, const uint16_t *polya_trimmed, char *out, size_t out_cap, uint64_t stats[3], float *kernel_ms);
int ngm_mapper_sam_fetch(ngm_mapper *m, char *out, size_t out_cap);

/* Several mappers on ONE input (ngm-hip hands batches to a mapper per worker thread / per GPU, like NextGenMap hands them to
 * its CS threads, src/NGM.cpp:232-279, src/CS.cpp:440-456).  top1PE's tie-break reads the running mean insert size of the
 * pairs selected so far (ScoreBuffer.h:90, ScoreBuffer.cpp:420-422, :487-488) -- sequential state.  Mappers that share an
 * ngm_pair_state take turns for that part of the selection in batch order (ngm_mapper_set_batch_seq before every
 * ngm_mapper_map_pe*, numbers 0, 1, 2 ... without gaps), so the result equals one mapper seeing the batches in order,
 * i.e. `ngm -t 1`.  Everything else of a batch (search, scoring, the order-free part of the selection, alignment)
 * overlaps freely. */
typedef struct ngm_pair_state ngm_pair_state;
ngm_pair_state *ngm_pair_state_create(void);
void ngm_pair_state_destroy(ngm_pair_state *ps);
int ngm_mapper_set_pair_state(ngm_mapper *m, ngm_pair_state *ps);
int ngm_mapper_set_batch_seq(ngm_mapper *m, uint64_t seq);
/* Config "fast_pairing" (--fast-pairing, src/ScoreBuffer.cpp:203-216): paired-end batches select both mates with top1SE instead of
 * top1PE / CheckPairs; whether the two winners form a pair is decided where the records are written (src/AlignmentBuffer.cpp:176-199) */
int ngm_mapper_set_fast_pairing(ngm_mapper *m, int on);

/* BGZF blocks written by the GPU (csrc/bgzf_device.h): what bamtools' BgzfStream does for `ngm --bam`
 * (lib/bamtools-2.3.0/src/api/internal/io/BgzfStream_p.cpp: DeflateBlock per 64 KB, zlib level 6) -- every 0xFF00 input bytes become one
 * BGZF member (its own DEFLATE stream with dynamic Huffman codes, CRC-32, ISIZE), the members one after the other in `out`.
 * raw / out: host memory (page-locked memory of ngm_host_alloc copies at PCIe rate); out_cap >= ngm_bgzf_bound(n).
 * Returns the bytes written, < 0 on error (ngm_pipeline_last_error).  One call at a time per object; objects are independent. */
typedef struct ngm_bgzf ngm_bgzf;
ngm_bgzf *ngm_bgzf_create(int device);
void ngm_bgzf_destroy(ngm_bgzf *z);
size_t ngm_bgzf_bound(size_t n);
long long ngm_bgzf_compress(ngm_bgzf *z, const void *raw, size_t n, void *out, size_t out_cap);
long long ngm_bgzf_compress_device(ngm_bgzf *z, const void *d_raw, size_t n, void *out, size_t out_cap);   /* raw bytes already in the device's memory */
float ngm_bgzf_last_kernel_ms(const ngm_bgzf *z);   /* HIP-event time of the last call's compression kernel (after ngm_bgzf_inflate: the time during which one of its
                                                         inflate kernels ran -- the chunks' kernels may overlap, their intervals are united, not summed) */
/* The other direction (csrc/bgzf_inflate_device.h): a run of whole BGZF members (a BAM, any file written by bgzip) inflated by the
 * GPU, one workgroup per member, length and CRC-32 of every member checked there against its trailer.
 * ngm_bgzf_inflated_size: the host's walk over the chain (BSIZE of the BC subfield, ISIZE of the trailer): the bytes of text, or
 * (size_t)-1 if the data is not made of whole BGZF members (no BC subfield, a BSIZE past the end, an ISIZE above 65536).
 * ngm_bgzf_inflate: the text into out (host memory, out_cap >= the inflated size).  Returns the bytes written; < 0 on error, with the
 * index of the first member the GPU refused in ngm_pipeline_last_error ("... member <i> refused ..."). */
size_t ngm_bgzf_inflated_size(const void *members, size_t n);
long long ngm_bgzf_inflate(ngm_bgzf *z, const void *members, size_t n, void *out, size_t out_cap);

/* ---- `ngm-hip --sort` (csrc/bam_sort.cpp): the BAM records of a whole run kept in the device's memory, sorted there into samtools'
 * coordinate order -- key ((uint32) refID, pos + 1, flag 0x10), ascending, refID -1 last; equal keys keep input order, which is (seq,
 * position in the run): the result depends neither on the order of the add calls nor on how the records were cut into runs -- and handed
 * back as the BGZF members of the sorted file plus its BAI index (SAM specification 5.2).  The sorted records form one byte stream cut into
 * members of exactly 0xFF00 input bytes (only the last one may be shorter; records straddle members), so the members do not depend on
 * chunk_bytes.  Records live in segments, one per add; nothing is spilled: when the device's memory is full, add fails with -12.
 * The index is canonical: per reference its bins ascending, a bin's chunks = the maximal runs of consecutive records of
 * that reference and bin, then pseudo-bin 37450, the linear index from the records' [pos, end), n_no_coor.
 * Errors: < 0 with ngm_pipeline_last_error(); the object stays destroyable after every error. */
typedef struct ngm_bam_sort ngm_bam_sort;
typedef struct ngm_bam_sort_params {
	int device;
	size_t chunk_bytes;  /* uncompressed bytes of sorted records compressed per ngm_bam_sort_next call; 0: 512 members (31.9 MiB);
	                        rounded down to a multiple of 0xFF00, never below 0xFF00 */
	size_t max_bytes;    /* cap on the record bytes held; 0: only the device's memory limits it */
} ngm_bam_sort_params;
ngm_bam_sort *ngm_bam_sort_create(const ngm_bam_sort_params *p);
void ngm_bam_sort_destroy(ngm_bam_sort *s);
/* a run of whole uncompressed BAM records (block_size chain) in host memory; seq orders the runs (any order of calls, every seq once);
 * thread-safe against other add calls.  The chain is walked on the host before a byte reaches the device: -22 with "ngm_bam_sort_add: ...
 * record <i> ..." for a chain that does not end exactly at n_bytes, a block_size below 32, or a record whose name, CIGAR, sequence and
 * qualities exceed its block_size; -22 for a duplicate seq and an add after finish; -12 for a total above max_bytes. */
int ngm_bam_sort_add(ngm_bam_sort *s, uint64_t seq, const void *records, size_t n_bytes);
/* no add after this: validates, sorts; n_ref = entries of the BAM's reference dictionary.  -22 names seq and the index within its run of
 * the first record with a refID at or above n_ref, with a refID >= 0 and pos < 0, or with an end above 2^29. */
int ngm_bam_sort_finish(ngm_bam_sort *s, int n_ref);
/* the next run of whole BGZF members of the sorted record stream; 0: done; > out_cap: nothing copied, call again with that much */
long long ngm_bam_sort_next(ngm_bam_sort *s, void *out, size_t out_cap);
/* after the last next(): the BAI file's bytes; first_member_offset = file offset of the first member next() returned; out NULL: the size */
long long ngm_bam_sort_index(ngm_bam_sort *s, uint64_t first_member_offset, void *out, size_t out_cap);
/* counts: records, record bytes, members written, chunks (ngm_bam_sort_next calls that compressed one), bins of the index (after
 * ngm_bam_sort_index); ms: kernel ms of keys / sort / gather / deflate / index (HIP events) */
int ngm_bam_sort_stats(const ngm_bam_sort *s, uint64_t counts[5], float ms[5]);
/* `ngm-hip --sort --markdup` (csrc/markdup.h, csrc/markdup_device.h): with on != 0, ngm_bam_sort_finish sets flag 0x400 on duplicate
 * records in the device's memory before it sorts them; nothing else about the sorted file changes.  Valid only before the first
 * ngm_bam_sort_add, -22 afterwards.  Off (the default): finish launches no kernel and holds no byte more than before.
 * The rules (INTEGRATION.md "Duplicate marking"; the result depends on the records and their run order -- seq, position in the run -- only):
 *   examined: flag 0x4, 0x100, 0x800 clear and refID >= 0; other records are never marked and never count;
 *   u5: forward strand pos - leading S/H lengths, reverse strand end - 1 + trailing S/H lengths (end as for the sort key: pos + M/D/N/=/X
 *     lengths, pos + 1 without any), clamped to [-2^30, 2^30 - 1]; without CIGAR operations u5 = pos;
 *   end key: ((uint32) refID << 32) | ((u5 + 2^30) << 1) | strand -- (refID, u5, strand) ascending, bit 63 clear;
 *   mates: records g, g + 1 of the run order, both examined, both 0x1, one with 0x40 and not 0x80, the other with 0x80 and not 0x40, equal
 *     names.  Mates with the first mate (0x40) in front are a pair; mates with the second mate in front (the order ngm-hip writes) are a
 *     pair unless one of them is part of a pair of the first kind with its other neighbour, so pairs never overlap.  A pair's first mate
 *     is the record with 0x40, its index g that of its record in front; every other examined record is a fragment;
 *   score: sum of the quality bytes >= 15; 0 with absent qualities (first byte 0xFF) or l_seq 0; a pair: both mates; 32 bits, saturating;
 *   pairs: key = the two end keys ascending (the first mate's first when equal) + one bit "the lower end is the first mate's" that counts
 *     only when both strands are equal; per key the highest score survives, ties to the lowest g; both mates of the others get 0x400;
 *   fragments: grouped by end key with both ends of every pair (survivor or not); a group with a pair end marks all its fragments, else the
 *     highest score survives, ties to the lowest g;
 *   the marker only ORs: a record that arrives with 0x400 keeps it and takes part like any other. */
int ngm_bam_sort_set_markdup(ngm_bam_sort *s, int on);
/* after a successful finish with marking on (-22 before, and when marking is off).  counts: examined records, pairs, fragments, duplicate
 * pairs, duplicate fragments, records newly marked (0x400 was clear); ms: kernel ms of the marking kernels / of its sorts (HIP events) */
int ngm_bam_sort_markdup_stats(const ngm_bam_sort *s, uint64_t counts[6], float ms[2]);
/* with ngm_sam_options::bam set: ngm_mapper_map_sam* hands the batch's records to s under the mapper's batch seq
 * (ngm_mapper_set_batch_seq) and returns 0 bytes instead of BGZF members; NULL detaches.  Same device: a device-to-device copy; another
 * device: the records are downloaded and go through ngm_bam_sort_add.  When the sorter has no device memory left for the batch (its -12),
 * ngm_mapper_map_sam* returns -28, so that the caller can tell it from the mapper's own allocations (-12). */
int ngm_mapper_set_bam_sorter(ngm_mapper *m, ngm_bam_sort *s);

/* ---- `ngm-hip --coverage` (csrc/coverage.cpp): the per-base read depth of a run as bedGraph text.  One int32 counter per base of every
 * contig (plus one slot per contig) lives in the device's memory for the whole run: 4 bytes per base, 12.4 GB for a genome of GRCh38's size.
 * An alignment covers the reference bases under its M, = and X operations; D and N advance without covering; I, S, H and P do neither;
 * what would lie past the contig's last base is clipped.  Lines: contig \t start \t end \t depth \n, start 0-based, end exclusive, depth > 0,
 * one per maximal run of equal depth inside one contig, contigs in the order given, runs ascending, no header.  The sums are integers: the
 * text depends on the set of alignments only, not on how they were cut into calls or which thread made them.  Depth is a 32-bit count.
 * Errors: < 0 with ngm_pipeline_last_error(); the object stays destroyable after every error. */
typedef struct ngm_coverage ngm_coverage;
typedef struct ngm_coverage_params {
	int device;
	int n_ref;
	const uint32_t *ref_len;
	const char *const *ref_name;
	size_t scan_chunk; /* counters scanned at a time by the finish (its temporaries are 5 bytes per counter of a chunk plus the chunk's lines);
	                      0: 2^25; at most 2^30 */
} ngm_coverage_params;
/* allocates and zeroes (bases + n_ref) * 4 bytes on the device; NULL with the error set when that fails */
ngm_coverage *ngm_coverage_create(const ngm_coverage_params *p);
void ngm_coverage_destroy(ngm_coverage *c);
/* n alignments: contig, 0-based position, CIGAR text cigar_text[cigar_off[i] .. cigar_off[i + 1]).  Thread-safe.  Validated on the host
 * first: -22 with "ngm_coverage_add: alignment <i>: ..." names the first one with a ref_id outside [0, n_ref), a negative position, an
 * unknown operation character, a number that overflows 2^28, an operation without a number or a number without an operation -- and adds
 * nothing of the call.  -22 after ngm_coverage_finish. */
int ngm_coverage_add(ngm_coverage *c, const int32_t *ref_id, const int32_t *pos0, const uint32_t *cigar_off /* [n + 1] */, const char *cigar_text, size_t n);
/* no add after this; waits for the adds in flight and sets the scan up */
int ngm_coverage_finish(ngm_coverage *c);
/* the next lines of the file, made chunk by chunk as they are asked for: whole lines only; 0 at the end; > out_cap: nothing copied, call
 * again with that much */
long long ngm_coverage_next(ngm_coverage *c, void *out, size_t out_cap);
/* counts: alignments added, and of the lines handed out so far covered bases (the sum of (end - start) * depth), runs, text bytes;
 * ms: kernel ms of add / scan / run heads / text (HIP events) */
int ngm_coverage_stats(const ngm_coverage *c, uint64_t counts[4], float ms[4]);
/* every batch ngm_mapper_map_sam* finishes adds the records it writes with flag bits 0x4 and 0x100 clear -- after the output filters, the
 * "no sequence" reads and the lost pairs -- to c, in place from the batch's arrays in device memory, on the mapper's stream; NULL detaches.
 * When c lives on another device, the batch's (contig, position, CIGAR) arrays are downloaded and go through ngm_coverage_add. */
int ngm_mapper_set_coverage(ngm_mapper *m, ngm_coverage *c);

/* ---- `ngm-hip --snp` (csrc/snp.cpp): the per-base mismatch pileup of a run and its single-base substitution calls as VCF text
 * ("--snp", holds the definition).  Coverage's difference array (int32) and three uint32 counters per base -- a read base b
 * over a reference base r != b counts in slot (b - r - 1) & 3 -- live in the device's memory for the whole run: 16 bytes per base, about
 * 50 GB for a genome of GRCh38's size.  Depth is ngm_coverage's depth.  An M, = or X column inside the contig votes for its read base when
 * the reference base (case folded) and the read base are one of ACGT and differ, and the record has no quality text or the column's Phred
 * quality is at least min_qual.  A base is a call when depth >= max(1, min_cov) and (double) n >= min_frac * (double) depth for the
 * alternative with the largest count n > 0 (ties: the first of A, C, G, T).  The file: a header (fileformat, source with the three
 * thresholds, one ##contig per contig, the INFO lines of DP and AO, the column line), then one line per call, contigs in the order given,
 * positions ascending: name \t pos (1-based) \t . \t REF \t ALT \t . \t PASS \t DP=depth;AO=n.  The sums are integers: the text depends on
 * the set of alignments and the thresholds only.  Errors: < 0 with ngm_pipeline_last_error(); the object stays destroyable after every error. */
typedef struct ngm_snp ngm_snp;
typedef struct ngm_snp_params {
	int device;
	int n_ref;
	const uint32_t *ref_len;
	const char *const *ref_name;
	const char *const *ref_seq;  /* one ASCII string of ref_len[c] letters per contig (ngm_snp_create only) */
	uint32_t min_cov;            /* N */
	double min_frac;             /* F, in (0, 1] */
	int min_qual;                /* Q, 0..93 */
	const char *min_frac_text;   /* F as the header prints it (the option's text); NULL: printf("%g") of min_frac */
	size_t scan_chunk;           /* slots scanned at a time by the finish (its temporaries are 5 bytes per slot of a chunk plus the chunk's
	                                lines); 0: 2^25; at most 2^30 */
} ngm_snp_params;
/* allocates and zeroes (bases + n_ref) * 16 bytes on the device and uploads the reference packed to 4 bits per base; NULL with the error
 * set when that fails */
ngm_snp *ngm_snp_create(const ngm_snp_params *p);
/* the same over the contigs of r, on r's device, reading r's resident packed genome instead of a copy (n_ref, ref_len, ref_name, ref_seq
 * and device of p are not read); r must outlive the object */
ngm_snp *ngm_snp_create_for_ref(const ngm_ref *r, const ngm_snp_params *p);
void ngm_snp_destroy(ngm_snp *s);
/* n alignments: contig, 0-based position, CIGAR text cigar_text[cigar_off[i] .. cigar_off[i + 1]), the sequence as the SAM record prints it
 * seq_text[seq_off[i] .. seq_off[i + 1]), and qual_text: NULL (no record has qualities), or a C string of Phred+33 characters under the
 * sequence's offsets.  Thread-safe.  Validated on the host first: -22 with "ngm_snp_add: alignment <i>: ..." names the first one that
 * ngm_coverage_add would refuse, whose sequence is shorter or longer than the read bases its CIGAR consumes (M, =, X, I, S), or whose
 * range the quality text does not reach (a quality text that goes on past the last alignment names that one) -- and adds nothing of the
 * call.  -22 after ngm_snp_finish. */
int ngm_snp_add(ngm_snp *s, const int32_t *ref_id, const int32_t *pos0, const uint32_t *cigar_off /* [n + 1] */, const char *cigar_text,
                const uint32_t *seq_off /* [n + 1] */, const char *seq_text, const char *qual_text, size_t n);
/* no add after this; waits for the adds in flight and sets the scan up */
int ngm_snp_finish(ngm_snp *s);
/* the next lines of the file, made chunk by chunk as they are asked for; the header is the first piece: whole lines only; 0 at the end;
 * > out_cap: nothing copied, call again with that much */
long long ngm_snp_next(ngm_snp *s, void *out, size_t out_cap);
/* counts: alignments added, mismatching bases counted, and of the text handed out so far calls, text bytes (header included), covered bases
 * (the sum of the depths); ms: kernel ms of add / scan / call flags / text (HIP events) */
int ngm_snp_stats(const ngm_snp *s, uint64_t counts[5], float ms[4]);
/* every batch ngm_mapper_map_sam* finishes adds the records ngm_mapper_set_coverage would add to s, in place from the batch's arrays in
 * device memory, on the mapper's stream; NULL detaches.  When s lives on another device, the batch's arrays are downloaded and go through
 * ngm_snp_add. */
int ngm_mapper_set_snp(ngm_mapper *m, ngm_snp *s);

/* ---- `ngm-hip --count` (csrc/count.cpp): per-region T>C conversion counts of a run ("--count", holds the definition).
 * Counters exist only for the bases some region covers: the regions of a contig are merged into disjoint intervals, and every base of
 * their union has two uint32 (cov, conv) in the device's memory for the whole run -- 8 bytes per base of the union, about 0.5 GB for all
 * human 3' UTRs -- plus two uint64 (reads, tc_reads) per region.  The records that count are ngm_coverage's.  An M, = or X column inside
 * the contig is eligible when the reference base (case folded) is T under a forward record or A under a reverse one, the read base is one
 * of ACGT, and the record has no quality text or the column's Phred quality is at least min_qual; it adds 1 to cov, and 1 to conv when the
 * read base is C (forward) or G (reverse).  A region of strand '+' takes forward records, '-' reverse ones, '.' both: reads counts the
 * records it takes with an M / = / X column inside it, tc_reads those of them with a conversion inside it.  The finish sums cov and conv
 * over every region's positions whose reference base is T ('+'), A ('-') or either ('.') and that are not in the mask; tc_reads is taken
 * at add time and ignores the mask.  All sums are integers: the result depends on the set of alignments, the regions, the reference and
 * the mask only.  Errors: < 0 with ngm_pipeline_last_error(); the object stays destroyable after every error. */
typedef struct ngm_count ngm_count;
typedef struct ngm_count_params {
	int device;
	int n_ref;
	const uint32_t *ref_len;
	const char *const *ref_name;     /* not read by the object (the caller prints the names) */
	const char *const *ref_seq;      /* one ASCII string of ref_len[c] letters per contig (ngm_count_create only) */
	int min_qual;                    /* Q, 0..93 (slamdunk count's default: 27) */
	size_t n_regions;                /* at least 1; regions may overlap, nest, repeat and come in any order */
	const int32_t *region_ref;       /* [n_regions] contig index */
	const uint32_t *region_start;    /* [n_regions] 0-based */
	const uint32_t *region_end;      /* [n_regions] exclusive, start < end <= ref_len */
	const char *region_strand;       /* [n_regions] '+', '-' or '.' */
} ngm_count_params;
/* allocates and zeroes 8 bytes per base of the regions' union (and one bit per base for the mask) plus 64 bytes per region on the device
 * and uploads the reference packed to 4 bits per base; NULL with the error set ("out of device memory ...") when that fails */
ngm_count *ngm_count_create(const ngm_count_params *p);
/* the same over the contigs of r, on r's device, reading r's resident packed genome instead of a copy (n_ref, ref_len, ref_name, ref_seq
 * and device of p are not read); r must outlive the object */
ngm_count *ngm_count_create_for_ref(const ngm_ref *r, const ngm_count_params *p);
void ngm_count_destroy(ngm_count *c);
/* n alignments as ngm_snp_add takes them, and reverse[i] != 0 for a record with flag bit 0x10.  Thread-safe.  Validated on the host as
 * ngm_snp_add validates: -22 with "ngm_count_add: alignment <i>: ..." names the first one refused, and nothing of the call is added.
 * -22 after ngm_count_finish. */
int ngm_count_add(ngm_count *c, const int32_t *ref_id, const int32_t *pos0, const uint32_t *cigar_off /* [n + 1] */, const char *cigar_text,
                  const uint32_t *seq_off /* [n + 1] */, const char *seq_text, const char *qual_text, const uint8_t *reverse /* [n] */, size_t n);
/* n positions (contig, 0-based) join the mask; any time before ngm_count_finish, thread-safe.  Positions outside every region are
 * ignored; -22 for a ref_id outside [0, n_ref) or a position outside its contig, and then nothing of the call is taken. */
int ngm_count_mask(ngm_count *c, const int32_t *ref_id, const int32_t *pos0, size_t n);
/* no add after this; waits for the adds in flight, uploads the mask and sums every region (one wave per region) */
int ngm_count_finish(ngm_count *c);
/* after the finish: six numbers per region, regions in the order given -- t_bases, masked, cov_on_ts, conv_on_ts, reads, tc_reads.
 * Returns the number of regions (out NULL: only that); -22 when n_regions is another number. */
long long ngm_count_read(ngm_count *c, int64_t *out /* [n_regions][6] */, size_t n_regions);
/* counts: alignments added, alignments that some region took, eligible columns and conversions inside the regions' union, distinct mask
 * positions inside it; ms: kernel ms of add / reduce (HIP events).  Thread-safe beside add and mask; the four device counters are those
 * of the adds that have returned. */
int ngm_count_stats(const ngm_count *c, uint64_t counts[5], float ms[2]);
/* every batch ngm_mapper_map_sam* finishes adds the records ngm_mapper_set_coverage would add to c, in place from the batch's arrays in
 * device memory, on the mapper's stream; NULL detaches.  When c lives on another device, the batch's arrays are downloaded and go through
 * ngm_count_add. */
int ngm_mapper_set_count(ngm_mapper *m, ngm_count *c);

/* ---- `ngm-hip --bs-mapping --methyl` (csrc/methyl.cpp): the per-cytosine methylation calls of a bisulfite run as Bismark's cytosine
 * report ("--methyl", holds the definition).  One pair of uint32 (meth, unmeth) per base of the reference lives in the
 * device's memory for the whole run: 8 bytes per base, about 25 GB for a genome of GRCh38's size.  The records that count are
 * ngm_coverage's.  A record is top or bottom (bottom: the first character of its ZS:Z tag is '-').  An M, = or X column inside the contig
 * counts when the record has no quality text or the column's Phred quality is at least min_qual: over a reference C (case folded) a top
 * record's C adds to meth and its T to unmeth; over a reference G a bottom record's G adds to meth and its A to unmeth.  The file has no
 * header and one line per site (a reference C, strand '+', or G, strand '-') with meth + unmeth >= max(1, min_depth) whose context is
 * selected, contigs in the order given, positions ascending: name \t pos (1-based) \t strand \t meth \t unmeth \t context \t C n1 n2.
 * The sums are integers: the text depends on the set of alignments and the parameters only.  Errors: < 0 with ngm_pipeline_last_error();
 * the object stays destroyable after every error. */
typedef struct ngm_methyl ngm_methyl;
typedef struct ngm_methyl_params {
	int device;
	int n_ref;
	const uint32_t *ref_len;
	const char *const *ref_name;
	const char *const *ref_seq;  /* one ASCII string of ref_len[c] letters per contig (ngm_methyl_create only) */
	int min_qual;                /* Q, 0..93 (MethylDackel's -p: 5) */
	int min_depth;               /* N, 0 or more */
	const char *context;         /* "all", "CpG", "CHG" or "CHH"; NULL: "all" */
	size_t scan_chunk;           /* bases flagged at a time by the finish (its temporaries are 5 bytes per base of a chunk plus the chunk's
	                                lines); 0: 2^25; at most 2^30 */
} ngm_methyl_params;
/* allocates and zeroes 8 bytes per base on the device and uploads the reference packed to 4 bits per base; NULL with the error set when
 * that fails */
ngm_methyl *ngm_methyl_create(const ngm_methyl_params *p);
/* the same over the contigs of r, on r's device, reading r's resident packed genome instead of a copy (n_ref, ref_len, ref_name, ref_seq
 * and device of p are not read); r must outlive the object */
ngm_methyl *ngm_methyl_create_for_ref(const ngm_ref *r, const ngm_methyl_params *p);
void ngm_methyl_destroy(ngm_methyl *c);
/* n alignments as ngm_snp_add takes them, and bottom[i] != 0 for a bottom record.  Thread-safe.  Validated on the host as ngm_snp_add
 * validates: -22 with "ngm_methyl_add: alignment <i>: ..." names the first one refused, and nothing of the call is added.  -22 after
 * ngm_methyl_finish. */
int ngm_methyl_add(ngm_methyl *c, const int32_t *ref_id, const int32_t *pos0, const uint32_t *cigar_off /* [n + 1] */, const char *cigar_text,
                   const uint32_t *seq_off /* [n + 1] */, const char *seq_text, const char *qual_text, const uint8_t *bottom /* [n] */, size_t n);
/* no add after this; waits for the adds in flight and sets the finish up */
int ngm_methyl_finish(ngm_methyl *c);
/* the next lines of the file, made chunk by chunk as they are asked for: whole lines only; 0 at the end; > out_cap: nothing copied, call
 * again with that much */
long long ngm_methyl_next(ngm_methyl *c, void *out, size_t out_cap);
/* counts: alignments added, and of the chunks made so far the lines written and meth, unmeth summed over all sites of context CG, then
 * CHG, then CHH, whatever the selection (complete once ngm_methyl_next has returned 0); ms: kernel ms of add / flags / select / text */
int ngm_methyl_stats(const ngm_methyl *c, uint64_t counts[8], float ms[4]);
/* every batch ngm_mapper_map_sam* finishes adds the records ngm_mapper_set_coverage would add to c, in place from the batch's arrays in
 * device memory, on the mapper's stream -- a record is bottom when its hit is reverse, the other way round for the second mate of a pair;
 * NULL detaches.  When c lives on another device, the batch's arrays are downloaded and go through ngm_methyl_add. */
int ngm_mapper_set_methyl(ngm_mapper *m, ngm_methyl *c);

/* page-locked host memory for read batches (the H2D copy then runs at PCIe rate without a staging copy) */
void *ngm_host_alloc(size_t bytes);
void ngm_host_free(void *p);
/* test hook: what the library itself holds in this process (ngm_host_alloc is the caller's and is not counted) -- out[0] device bytes
 * live, out[1] pinned host bytes live, out[2] device allocations so far, out[3] pinned allocations so far */
int ngm_debug_live_memory(uint64_t out[4]);

/* Host threads next to the GPU.  A two-socket host runs the host stages (read parsing, pair selection, SAM text) at half the
 * rate when their threads and buffers are spread over both sockets (measured with ngm-hip).  This pins the
 * CALLING thread -- and with it every thread it creates afterwards, the library's thread pool included -- to the CPUs of
 * the NUMA node the device hangs on (/sys/bus/pci/devices/<bdf>/numa_node, .../node<N>/cpulist).  Call it first thing, before
 * any other entry point.  Returns the number of CPUs in the set, 0 when nothing was changed (no NUMA information, or
 * NGM_HIP_NO_NUMA_PIN is set), < 0 on error.  (NextGenMap itself leaves placement to the OS; this replaces nothing there.) */
int ngm_host_pin_to_device_node(int device);

/* A reference artefact that IS mirrored on request: NextGenMap hands a read to its ScoreBuffer right after the search
 * (src/CS.cpp:436); when the last score of a pair's first mate fills the score buffer exactly (src/ScoreBuffer.cpp:519-523; the
 * buffer holds IAlignment::GetScoreBatchSize() entries: 1 024 for the SeqAn personality, src/seqan/EndToEndAffine.h:44-46), DoRun
 * sees the mate's Calculated == -1 (src/MappedRead.cpp:14, src/ScoreBuffer.cpp:196) and selects nothing; if the mate then has no
 * candidates it goes to the writer alone (src/CS.cpp:326-329) and the pair is never written -- "(2 discarded)" in the reference's
 * summary.  With entries > 0 the mapper follows the reference's buffer through its batches (sequential state, like the running mean:
 * exact for `ngm -t 1`) and flags such pairs NGM_PAIR_LOST: no alignment, no record.  0 (default): no pair is lost. */
int ngm_mapper_set_reference_score_buffer(ngm_mapper *m, int entries);
/* pairs flagged NGM_PAIR_LOST by this mapper so far */
int ngm_mapper_lost_pairs(ngm_mapper *m, uint64_t *out);
/* ... the reference flushes that buffer at the end of every CS batch of 1 800 000 / qry_avg_len reads (src/CS.cpp:26, :542-543,
 * even for paired input: src/NGM.cpp:238-243); tell the mapper that number (0: never flushed) so that the walk follows it */
int ngm_mapper_set_reference_cs_batch(ngm_mapper *m, int reads);

/* which paths the reads took, summed over all batches of this mapper: [0] reads searched, [1] candidates, [2] reads re-run by the exact
 * search with its table in LDS, [3] ... in global memory, [4] reads whose candidate order (rList, src/CS.cpp:196-211) was replayed because
 * it decides a tie, [5] of those beyond the limits of the LDS replay (replayed exactly through buckets / a table in global memory), [6] reads whose order was
 * left undetermined (ties then resolve by position), [7] reads searched by the heavy-read kernel (more index hits than the fast path takes) */
int ngm_mapper_path_counters(ngm_mapper *m, uint64_t out[8]);

/* of path counter [5] (reads beyond the LDS replay): the reads the bucket replay (csrc/cs_order_bucket_device.h) left to the replay with a
 * table in global memory (cs_order_kernel<true>) -- bisulfite runs, a read with a bucket of more than 256 hits, NGM_HIP_ORDER_NO_BUCKETS */
int ngm_mapper_order_table_reads(ngm_mapper *m, uint64_t *out);

/* Host-only debug / test entry (no GPU needed): what pass 3 of the pair selection does per tied pair -- ScoreBuffer::top1PE's two sorts
 * (src/ScoreBuffer.cpp:373-376: std::sort(sortLocationScore) on the candidate lists in CollectResultsStd's order, here given by `rank`),
 * computeMQ (:34-49), and the CheckPairs double loop (:405-413, :463-502) over the candidates at or above best * cutoff, restricted to
 * the insert-size window.  Candidates of mate a are entries [0, cnt_a) of loc / sv / score / rank, those of mate b [cnt_a, cnt_a + cnt_b).
 * rank may be NULL (no candidate order: any deterministic order).  Returns 0, or a negative error code. */
int ngm_debug_pair_walk(uint32_t cnt_a, int len_a, uint32_t cnt_b, int len_b, const uint32_t *loc, const uint32_t *sv, const float *score, const uint32_t *rank,
		float cutoff, int min_insert, int max_insert, uint32_t *out_a, uint32_t *out_b, int *mq_a, int *mq_b, uint64_t cap, float *combo_score, int *combo_dist, int *combo_a, int *combo_b,
		uint64_t *n_combo);

/* Host-only debug / test entry: the double loop of ScoreBuffer::top1PE over CheckPairs (src/ScoreBuffer.cpp:405-413, :463-502) at the running
 * mean insert size `avg`, on a given sequence of in-window combinations (pair score, insert size, candidate of a, candidate of b) -- on all
 * of them (out_all) and on the ones the product keeps for its sequential pass (out_kept: those that reach the running maximum of the pair
 * score).  out[6] = {found, winner of a, winner of b, equal-score-and-insert-size count, insert size, combinations evaluated}. */
int ngm_debug_pair_eval(uint64_t n, const float *pair_score, const int *dist, const int *ia, const int *ib, int avg, int out_all[6], int out_kept[6]);

/* test hook: ScoreBuffer::top1SE + computeMQ (src/ScoreBuffer.cpp:228-277, :34-49) as the score stage runs it (select_top1_kernel) over
 * host arrays: read i owns candidates [base[i], base[i] + count[i]); out: winner (candidate index, 0xFFFFFFFF: none), MAPQ, number of
 * best-scoring candidates, best score.  tests/test_gpu_select.py compares it with the reference's sequential loop. */
int ngm_debug_select_top1(int device, int n_reads, const uint32_t *base, const uint32_t *count, uint64_t n_cand, const float *scores, const uint32_t *loc,
		const uint32_t *strand_votes, uint32_t *winner, int32_t *mapq, int32_t *n_best, float *best_score);

/* test hook: ngm_hip_batch_align (include/ngm_hip.h) of an AFFINE engine the way the mapper's align stage runs it: the DP, then the one
 * finishing kernel from the trace matrix to CIGAR / NM / identity (affine_finish_kernel, csrc/cigar_device.h).  *n_fallback: the alignments
 * whose CIGAR did not fit the kernel's row -- those are served by the old traceback kernel on the same batch and the host's string builder,
 * like in the mapper.  The engine and the output records are those of include/ngm_hip.h.  Returns n, or a negative error code.  tests/test_gpu_align_finish.py compares it with the CPU oracle. */
int ngm_debug_align_finish(void *engine /* ngm_hip_ctx * */, int mode, int n, const char *const *ref, const char *const *qry, void *out /* ngm_hip_align_out[n] */,
		uint64_t *n_fallback);

/* test hook: ngm_hip_batch_align (include/ngm_hip.h) of a LINEAR engine the way the mapper's align stage of a default run builds its strings: pack,
 * DP + traceback, compact_runs_kernel, cigar_strings_kernel<false> (csrc/cigar_device.h) -- through the launch code the align stage runs -- then
 * the downloads.  dir: the pairs' direction bytes (alt_scoring / alt_cigar engines) or NULL; capacity: bytes of the string stream, 0 = the
 * mapper's n * 96 + 4096.  out[i] is taken from the device's stream where the kernel built the strings (built_by[i] = 1), and made by the
 * host's builder from the compacted runs otherwise (built_by[i] = 0: a string beyond the kernel's row, a read symbol outside ACGTN, a full
 * stream) -- as the mapper does.  *cursor: the stream cursor's final value (all bytes asked for, beyond capacity when the stream was full).
 * Returns n (0 for n <= 0), or a negative error code (ngm_hip_last_error of the engine); -22, before anything is taken, for an engine of the
 * affine personality.  tests/test_gpu_linear_strings.py compares it with the CPU oracle. */
int ngm_debug_linear_strings(void *engine /* ngm_hip_ctx * */, int mode, int n, const char *const *ref, const char *const *qry, const char *dir, uint64_t capacity,
		void *out /* ngm_hip_align_out[n] */, uint8_t *built_by, uint64_t *cursor);

/* test hook: gather_pairs_kernel (csrc/gather_device.h) through the launch code of the score and align stages, for a mapper's q, corridor,
 * reference and engine.  reads: n_reads rows of qry_max_len bytes, uploaded and measured as a batch's are (by the candidate search);
 * pair p = (pair_read[p] < n_reads, pair_loc[p], pair_sv[p]: bit 0 = reverse strand); alt_dir: 0 off, 1 single-end, 2 paired (the table bit
 * of the read classes); align_stage: 0 = the score stage's window geometry, ((q + c) | 1) + 1, 1 = the align stage's, (q + c) | 2.
 * dims = {RW, FW}: read and window words per pair; with words, lens and blk_rows all NULL nothing else is done.  words: the packed
 * workspace as it stands, ceil(n_pairs / 64) * (RW + FW) * 64 dwords (block b, word m, slot s at (b * (RW + FW) + m) * 64 + s; window words
 * from m = RW); lens[n_pairs]; blk_rows[ceil(n_pairs / 64)].  A word the kernel did not write reads as 0xFFFFFFFF.  The call disturbs the
 * mapper's batch state like a map call does: its uploaded reads (batch_reads), the per-read and candidate arrays of the last search (a whole
 * candidate search runs, only to measure the reads) and the search's paired flag (set to single-end).  Returns 0, or a negative error code;
 * -22 before anything is taken for a pair whose read does not exist.  tests/test_gpu_gather.py compares it with tests/ngm_host_model.py. */
int ngm_debug_gather_pairs(ngm_mapper *m, int n_reads, const char *reads, int n_pairs, const uint32_t *pair_read, const uint32_t *pair_loc, const uint32_t *pair_sv,
		int alt_dir, int align_stage, int dims[2], uint32_t *words, uint16_t *lens, uint16_t *blk_rows);

/* test hook: expand_pairs_kernel (csrc/gather_device.h) over host arrays: out[base[i] + k] = i for k < count[i]; out has n_cand entries, the
 * ones no read owns are left as 0xFFFFFFFF. */
int ngm_debug_expand_pairs(int device, int n_reads, const uint32_t *base, const uint32_t *count, uint64_t n_cand, uint32_t *out);

/* test hook: the paired-end selection of the score stage (pair_simple_kernel, csrc/gather_device.h, and the three instances of
 * pair_choice_kernel, csrc/pair_device.h: ScoreBuffer::top1PE + CheckPairs, src/ScoreBuffer.cpp:368-502, as far as the scores alone decide)
 * over host arrays, through the very launch sequence the mapper runs and always with the pairs with choices on the GPU.  Reads 2p and
 * 2p + 1 are pair p (the odd read is mate `a`); read i owns candidates [base[i], base[i] + count[i]); max_insert <= 0: no upper bound.
 * Out, as the mapper downloads them: info[n_pairs] (>= 0: settled, bit 0 = taken, bits 1.. = insert size; -1: the host's; <= -2: entry
 * -2 - info, from 2^30 on in the second half of `entries`), mapq / n_best [2 n_pairs] (in/out: written for taken one-candidate pairs only),
 * counts = {tied, small, large, large beyond 2 048 candidates above the cut-off}, entries (ngm::PairOut[2 n_pairs + 2]: eight int32
 * {flags, wa, wb, dist, dmin, dmax, tied_ix, pair}) and tops (ngm::PairTop[n_pairs + 1]: int32 d[8], a[8], b[8]); what no kernel wrote
 * reads as -1.  tests/test_gpu_pair_choice.py compares it with tests/pair_choice_model.py. */
int ngm_debug_pair_select(int device, int n_pairs, const uint32_t *base, const uint32_t *count, uint64_t n_cand, const float *scores, const uint32_t *loc,
		const uint16_t *read_len, int min_insert, int max_insert, float cutoff, int32_t *info, int32_t *mapq, int32_t *n_best, uint32_t counts[4], void *entries, void *tops);

/* test hook: the record writers of the SAM stage (sam_lengths_kernel / sam_write_kernel, csrc/sam_device.h) over constructed results, through
 * the launch sequence ngm_mapper_map_sam runs (lengths, prefix sums, the 32-bit total checked against the 64-bit one, bytes).  Needs no mapper:
 * opt as for ngm_mapper_set_sam_options; hard_clip / silent_clip / variant as in ngm_mapper_params; alt_scoring: the mapper ran with bs_mapping or
 * slam_seq & 2 (how the SLAM-seq tags label a column '='); reads, quals: n rows of q bytes; names, meta as for ngm_mapper_map_sam; cigars, mds: n
 * NUL-terminated strings (NULL: empty); polya: n values or NULL (no XA:i); the contig table: n_contigs names and lengths; ref: only read with
 * opt->slam_seq (its packed genome; its contigs must be the table's).  out: the SAM text, or with opt->bam the records as they stand in HBM
 * (uncompressed, no BGZF); counters: reads counted, reads mapped, lines written, bytes, pairs with both mates mapped, of those broken, insert
 * sizes of the others.  Returns the length of the text (> out_cap: nothing was copied), or < 0.  -22, before anything is launched, for an
 * input the kernels would index out of bounds with: a name beyond names_bytes or longer than 254 bytes; and for every hit with `mapped`: a
 * contig outside the table, qstart / qend negative or together beyond the read, a CIGAR that is malformed or whose M / I operations consume more
 * bases than follow qstart, with slam_seq an alignment that ends beyond its contig.  tests/test_gpu_sam_records.py compares it with
 * tests/sam_model.py. */
long long ngm_debug_sam_records(int device, const ngm_sam_options *opt, int hard_clip, int silent_clip, int variant, int alt_scoring, int n, int q,
		const char *reads, const char *quals, const char *names, size_t names_bytes, const ngm_sam_read *meta, const ngm_hit *hits, const char *const *cigars,
		const char *const *mds, const uint16_t *polya, int n_contigs, const char *const *contig_names, const uint64_t *contig_lens, const ngm_ref *ref,
		char *out, size_t out_cap, unsigned long long counters[7]);

/* of path counter [7] (reads searched by the heavy-read kernel, csrc/cs_heavy_device.h), summed over all batches: [0] reads given a second
 * pass (T from the first pass's maximum), [1] table passes started over with twice the parts, [2] reads a class could not certify and
 * queued again, [3] times the pool of global-memory vote tables had to grow (one more synchronisation in that batch) */
int ngm_mapper_heavy_counters(ngm_mapper *m, uint64_t out[4]);

/* of the last ngm_mapper_map_* call, how its search + score turn went: [0] 1 when the per-read arrays of the search (candidate offsets,
 * counts, best votes) travelled behind the score stage instead of in front of the search's synchronisation (0 under
 * NGM_HIP_CS_EAGER_ARRAYS=1, read when the mapper is created), [1] search attempts (more than one: the candidate regions overflowed and
 * the batch was searched again with four times the room), [2] score-stage buffers that had to grow behind the synchronisation, inside
 * the turn, because the count predicted in front of the search was too small.  tests/test_gpu_search_turn.py */
int ngm_mapper_search_turn_counters(ngm_mapper *m, uint64_t out[3]);

/* which first-pass kernel the last candidate search launched (read only; tests/test_gpu_cs_shapes.py): [0] 0 = one bucket per k-mer,
 * 1-3 = the shape of cs_canon_kernel over canonical pair buckets, [1] waves per read of cs_fast2_kernel (1: cs_fast_kernel) when [0] is 0,
 * [2] work items per lane (12 / 24), [3] 1 = 16-bit work items, 0 = 32-bit ones */
int ngm_mapper_cs_dispatch(ngm_mapper *m, uint64_t out[4]);

/* work counters of the last candidate search: [0] k-mers looked up, [1] index hits voted, [2] candidates emitted
 * (algorithmic bytes of the search = 20 * kmers + 4 * hits + 16 * candidates) */
int ngm_mapper_cs_counters(ngm_mapper *m, uint64_t out[3]);

/* ---- the one collective of the path: mapping statistics summed over the shard processes --------------------------
 * Reads shard across GPUs with nothing shared on the data path (`ngm-hip -g a,b,... --shard-output`: one process per GPU, the genome and
 * the index replicated); what the reference keeps in process-wide counters that all its CS threads add to (src/NGM.cpp:172-200
 * AddMappedRead / AddUnmappedRead / AddWrittenRead / AddReadRead; the pair counters of src/AlignmentBuffer.cpp:175-199) is, across
 * processes, the vector {reads, mapped, unmapped, written, pairs_total, pairs_broken, insert_sum, insert_cnt} summed with ONE
 * ncclAllReduce (RCCL over xGMI; librccl is loaded at run time).  ngm_stats_unique_id: a new communicator id as 256 hex digits + NUL
 * (the parent makes it and hands it to the shard processes); ngm_stats_comm_create: rank `rank` of `world` on `device` joins (about a
 * second: call it beside the load of the index); ngm_stats_allreduce: v becomes the sum over all ranks.  All return < 0 / NULL with
 * ngm_pipeline_last_error() set when librccl is missing or a call fails -- the parent's sum over the shards' pipes stands then. */
typedef struct ngm_stats_comm ngm_stats_comm;
int ngm_stats_unique_id(char hex[257]);
ngm_stats_comm *ngm_stats_comm_create(int device, int rank, int world, const char *hex);
int ngm_stats_allreduce(ngm_stats_comm *c, int64_t v[8]);
void ngm_stats_comm_destroy(ngm_stats_comm *c);
/* pairs with both mates mapped, those of them the writer flags as broken (other contig / insert size outside the window / same strand),
 * and the sum of the others' insert sizes, of the last ngm_mapper_map_sam call (src/AlignmentBuffer.cpp:175-199 pairInsertCount,
 * brokenPairs, pairInsertSum) */
int ngm_mapper_last_pair_stats(ngm_mapper *m, uint64_t out[3]);

/* kernel wall-clock of the last ngm_mapper_* call, HIP events on the launch stream, ms:
 * [0] candidate search kernels  [1] gather+pack  [2] score  [3] select  [4] gather+pack (align)  [5] align DP
 * [6] traceback  [7] candidate-search stage including host round trips between its passes */
int ngm_mapper_last_kernel_ms(ngm_mapper *m, float ms[8]);
/* ... and of the candidate-order replays of that call (cs_order_kernel: runs on a stream of its own beside the stages above) */
float ngm_mapper_last_order_replay_ms(ngm_mapper *m);

/* ---- `--argos` (src/writer/ScoreWriter.cpp, src/ScoreBuffer.cpp:150-183): every scored candidate of a read, ordered by score --------------
 * ngm_mapper_set_argos: min_score >= 0 turns the mode on for this mapper (Config ARGOS_MINSCORE, `--argos-min-score`: > 0 keeps the
 * candidates with score >= min, min = read length * match_bonus * min_score when min_score <= 1, else min_score itself); < 0 turns it off.
 * Single-end only; not with bs_mapping / slam_seq.  The search parameters the mode implies (sensitivity 0, kmer_min 2 unless given:
 * src/config/Config.cpp:384-388, :517-520) are the caller's, in ngm_mapper_params. */
int ngm_mapper_set_argos(ngm_mapper *m, float min_score);
/* Candidate search and BatchScore of n reads (rows as for ngm_mapper_map_se), then per read ScoreWriter's line
 * "name(\t<contig>:<pos>:<reverse>:<|score difference to the previous entry|>)*\n" over the candidates with a positive score in the order of
 * the reference's std::sort, positions converted with the --argos clamp (src/SequenceProvider.cpp:111-142).  A read without candidates (or
 * without survivors of the filter) writes nothing.  names / meta as for ngm_mapper_map_sam (qual_len is not used).  Returns the length of
 * the text (> out_cap: nothing was copied -- ngm_mapper_sam_fetch with a larger buffer copies it), or < 0.  stats: reads counted, reads
 * with a line (the reference's "mapped"), 0 (ScoreWriter counts no written lines).  kernel_ms (optional): GPU time of the ordering and
 * text kernels. */
long long ngm_mapper_map_argos(ngm_mapper *m, int n, const char *reads, const char *names, size_t names_bytes, const ngm_sam_read *meta,
		char *out, size_t out_cap, uint64_t stats[3], float *kernel_ms);
/* ScoreWriter::DoWriteProlog: "#<total_reads>\n#0:<name>\t1:<name>\t...\n".  Writes it when it fits in cap; returns its length, or < 0. */
int ngm_argos_prolog(const ngm_ref *ref, uint64_t total_reads, char *out, size_t cap);
/* summed over this mapper's ngm_mapper_map_argos calls: [0] reads (with a line) whose positive scores are all distinct (class U: any
 * order prints the same), [1] reads of at most 16 survivors with a tie (class S: ordered on the GPU by score and the reference's candidate
 * order), [2] more than 16 survivors with a tie (class H: libstdc++'s std::sort on the host), [3] entries written */
int ngm_mapper_argos_counters(ngm_mapper *m, uint64_t out[4]);
/* ... [0] reads ordered by the long-list path (more candidates than the LDS holds: a workgroup per read over global memory),
 * [1] reads of class S / H ordered by position because the reference's candidate order could not be determined */
int ngm_mapper_argos_path_counters(ngm_mapper *m, uint64_t out[2]);
/* Host-only test entry: what the --argos ordering does with one read of n candidates (scores, and the reference's candidate order `rank`,
 * may be NULL) under min_score for a read of read_len bases.  order: the survivors (indices into the list) in the order they are printed
 * (the first out[1] of them are); out = {survivors, survivors with a positive score, class 0 U / 1 S / 2 H}. */
int ngm_debug_argos_order(uint32_t n, const float *score, const uint32_t *rank, float min_score, int read_len, int match_bonus, uint32_t *order, uint32_t out[3]);

#ifdef __cplusplus
}
#endif
#endif
