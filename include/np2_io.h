/*
 * np2_io.h — input side of the NextPolish2 hot path.
 *
 * Replaces the reference's rust-htslib / kseq / KmerInfo::new call sites:
 *   FASTA[.gz] records            src/main.rs:1705-1714   (kseq: name = header up to first whitespace)
 *   indexed BAM fetch per contig  src/main.rs:1745-1758   (IndexedReader::from_path + fetch(tid, 0, len))
 *   record admission + packing    src/main.rs:1758-1817   (filters, fill_with_cigar, is_clip, trim(8),
 *                                                          AlignSeq::new, filter_alignseqs_by_clip)
 *   yak v2 dump header + buckets  src/utils/kmer.rs:72-170
 * BGZF inflate and BAM parsing run on the host pool (libdeflate / zlib) or — NP2_INFLATE=gpu, and by default when this
 * rank has fewer than twelve host CPUs to itself, or for a reference with 128 MB of BAM and more — ON THE DEVICE: the contig's BGZF blocks are uploaded as they lie in the
 * file, inflated one wavefront per block (csrc/np2_inflate.hip), the records found by walking the inflated stream along
 * the .bai linear index, and the SEQ bytes read by the columnariser where the inflater left them.  The CIGAR walk /
 * trim(8) / nibble packing is a HIP kernel that writes the packed pileup straight into HBM (np2_contig_t) either way.
 */
#ifndef NP2_IO_H
#define NP2_IO_H
#include "np2.h"
#ifdef __cplusplus
extern "C" {
#endif

/* read-admission options (src/utils/option.rs:267-292) */
typedef struct np2_front_opts {
    uint32_t min_read_len;     /* -l 1000 */
    uint32_t min_map_len;      /* -a integer part, 500 */
    float min_map_fra;         /* -a fractional part, 0.5 */
    int16_t min_map_qual;      /* -q 1 */
    uint32_t max_clip_len;     /* -c 100 */
    uint8_t use_supplementary; /* -s */
    uint8_t use_secondary;     /* -S: np2_contig_from_bam recovers the SEQ of secondary records from the primary record
                                * of the same read (secondary.rs; two passes over the BAM on first use);
                                * np2_contig_from_records expects the caller to pass the recovered SEQ */
} np2_front_opts_t;

/* one alignment record, fields as in the BAM record (what rust-htslib's Record exposes, main.rs:1751-1797) */
typedef struct np2_bamrec {
    int32_t pos;        /* 0-based leftmost position */
    uint16_t flag;
    uint8_t mapq;
    uint8_t pad;
    uint32_t n_cigar;
    uint64_t cigar_off; /* index into cigar[] (u32 each: len << 4 | op, BAM encoding) */
    uint32_t l_seq;
    uint64_t seq_off;   /* byte offset into seq4[] (4-bit packed, BAM encoding, high nibble first) */
} np2_bamrec_t;

/* ---- FASTA[.gz] ---- */
typedef struct np2_fasta np2_fasta_t;
int np2_fasta_open(const char *path, np2_fasta_t **out);
/* returns 1 and borrows name/seq until the next call, 0 at end of file, <0 on error */
int np2_fasta_next(np2_fasta_t *f, const char **name, const uint8_t **seq, uint64_t *len);
void np2_fasta_close(np2_fasta_t *f);

/* ---- yak v2 dump ---- */
/* fills *out with malloc'ed arrays (release with np2_yak_free) */
int np2_yak_load(const char *path, np2_yak_t *out);
void np2_yak_free(np2_yak_t *y);
/* np2_ctx_create for dumps on disk: the files go to the device in pieces as they are read and the HBM tables are built
 * from the file images, without the host arrays of np2_yak_load (KmerInfo::new + the per-phase file reads of
 * kmer.rs:72-170 collapsed into one load).  Tables are ordered by k (option.rs:238).  Errors: np2_io_last_error(). */
int np2_ctx_create_from_files(np2_ctx_t **out, int device, const char *const *paths, int n_paths);

/* ---- indexed BAM ---- */
typedef struct np2_bam np2_bam_t;
/* needs <path>.bai (or <stem>.bai).  A handle keeps device-side staging of the FIRST context it is used with (stream, device):
 * use one handle with contexts of one device only, one thread at a time (nextpolish2_amd.cli: a handle per front-end thread) */
int np2_bam_open(const char *path, np2_bam_t **out);
void np2_bam_close(np2_bam_t *b);
int np2_bam_n_refs(np2_bam_t *b);
const char *np2_bam_ref_name(np2_bam_t *b, int tid, uint32_t *len);
const char *np2_io_last_error(void);

/* Packed pileup of one contig, resident in HBM, built from its alignment records.
 * ref = contig bytes exactly as in the FASTA (case matters for trim, main.rs:447-513). */
int np2_contig_from_records(np2_ctx_t *ctx, const uint8_t *ref, uint32_t L, const np2_bamrec_t *recs,
                            uint32_t n_recs, const uint32_t *cigar, const uint8_t *seq4,
                            const np2_front_opts_t *opts, np2_contig_t **out);
/* same, reading the records of contig `name` from an indexed BAM (must be coordinate sorted) */
int np2_contig_from_bam(np2_ctx_t *ctx, np2_bam_t *bam, const char *name, const uint8_t *ref, uint32_t L,
                        const np2_front_opts_t *opts, np2_contig_t **out);
/* ---- mapping depth of a contig and its stretches of sufficient depth -----------------------------------------------------
 * Depth counts ALIGNMENT RECORDS, not polish-admitted reads: np2_front_opts_t plays no part.  For one record with CIGAR
 * operations (op, len): span = sum of len over M D N = X (a record whose sum is 0 covers 1 position, as htslib's end
 * position does), aligned = sum over M I = X, read_len = sum over M I S H = X.  The record is counted iff
 * (flag & exclude_flags) == 0, mapq >= min_mapq, n_cigar > 0, read_len > 0 and not
 * (double)aligned / (double)read_len < min_aligned_fra (IEEE double).  depth[i], 0 <= i < L, is the number of counted
 * records with pos <= i < min(pos + span, L); records with pos < 0 or pos >= L are ignored.  A run is a maximal [s, e]
 * (0-based, inclusive) with depth >= min_depth throughout; it is kept iff e - s + 1 >= min_len.  min_depth = 0 gives the
 * one run [0, L - 1] even without a record; L = 0 gives nothing.
 * Outputs: starts[i], ends[i] of the *n_runs kept runs in ascending order (release both with np2_free; NULL when there is
 * none), depth (or NULL): the caller's array of L words — the per-base array leaves the device only then.
 * NP2_E_ARG before anything is launched, the context stays usable: min_aligned_fra outside [0, 1] or NaN, a NULL argument,
 * a contig name the BAM header lacks.  L above 4294901760 is NP2_E_UNSUPPORTED. */
typedef struct np2_depth_opts {
    uint32_t min_depth;     /* -d 3 */
    uint32_t min_len;       /* -l 1000 */
    double min_aligned_fra; /* --min_fra 0.8 */
    uint16_t exclude_flags; /* 0x4: unmapped */
    uint8_t min_mapq;       /* 0 */
} np2_depth_opts_t;
typedef struct np2_depth_stats {
    uint64_t records_seen;    /* records handed in or fetched */
    uint64_t records_counted; /* those of them that entered the depth */
    uint64_t sum_depth;  /* over all L positions */
    uint64_t bases_kept; /* positions inside kept runs */
    uint32_t max_depth;
    uint32_t bases_ok;   /* positions with depth >= min_depth */
    uint32_t runs;       /* before the length filter */
    uint32_t runs_kept;  /* = *n_runs */
    float kernel_ms;     /* the depth kernels together (HIP events) */
} np2_depth_stats_t;
/* recs / cigar as np2_contig_from_records takes them (host memory); seq_off and l_seq are not read */
int np2_depth_from_records(np2_ctx_t *ctx, uint32_t L, const np2_bamrec_t *recs, uint32_t n_recs, const uint32_t *cigar,
                           const np2_depth_opts_t *opts, uint32_t **starts, uint32_t **ends, uint32_t *n_runs,
                           uint32_t *depth /* [L] or NULL */, np2_depth_stats_t *stats /* or NULL */);
/* the same over the records of contig `name` of an indexed BAM, fetched the way np2_contig_from_bam fetches them (on the
 * device path the records and CIGAR words are in HBM already; no SEQ byte moves on either path) */
int np2_depth_from_bam(np2_ctx_t *ctx, np2_bam_t *bam, const char *name, uint32_t L, const np2_depth_opts_t *opts,
                       uint32_t **starts, uint32_t **ends, uint32_t *n_runs, uint32_t *depth /* [L] or NULL */,
                       np2_depth_stats_t *stats /* or NULL */);
/* ---- read-supported variants of a contig: pileup counts, left-aligned indel alleles, calls ------------------------------
 * THE RULE IS THIS PROJECT'S OWN: counts and integer thresholds, no quality model.  Equality with DeepVariant, bcftools or any
 * other caller is not claimed.  A site where nearly every read disagrees with the assembly (a homozygous call) is a potential
 * error of the assembly.
 * Inputs: ref[L], case-insensitive, A C G T = codes 0..3, anything else N; records, CIGAR words and 4-bit SEQ as
 * np2_contig_from_records takes them (SEQ nibbles 1 2 4 8 = A C G T, every other nibble N).
 * Admission: a record is counted iff the depth report's rule holds under these options ((flag & exclude_flags) == 0, mapq >=
 *   min_mapq, n_cigar > 0, read_len > 0, not aligned / read_len < min_aligned_fra), 0 <= pos < L, it has no N operation
 *   (else stats.records_skipped) and l_seq equals the sum of its M I S = X lengths (else — SEQ * too — stats.records_no_seq).
 * cov[p]: counted records with pos <= p < min(pos + span, L), span as in the depth report.
 * alt[4 p + b], b = A C G T: counted records with an M/=/X column at p < L whose read base is b, where ref[p] is A C G T and
 *   differs from b.  A read N adds nothing; a reference N has no counts and no SNV.
 * Indel event: an I or D operation of 1 <= n <= max_indel (<= 28) bases whose neighbours in the CIGAR are both M, = or X
 *   (leading and trailing indels, indels next to a clip and adjacent I/D pairs are ignored), with a preceding run — the
 *   consecutive M/=/X operations before it — of m >= 1 columns.  a = the reference position of the column before it, qa = that
 *   column's query index.  D: a + n < L.  I: a + 1 < L and every inserted base is A C G T.
 * Left shift: by the largest t <= m - 1 whose steps j = 0 .. t-1 all satisfy — I: read[qa-j+n] == read[qa-j], both A C G T;
 *   D: ref[a-j] == ref[a-j+n] and read[qa-j] == ref[a-j], all A C G T.  These steps change no column's cov or alt.
 * Allele key: (a' = a - t, kind DEL < INS, n, bases): I: read[qa-t+1 .. qa-t+n], 2 bits a base, the first base highest (numeric
 *   order = lexicographic); D: 0.  An allele's count is the number of its events.
 * Calls, all tests in integers (c * 1000 >= pm * d):
 *   SNV at p: d = cov[p], the alt base of the greatest count (ties A < C < G < T), c its count.
 *   Indel per (a', kind): the allele of the greatest count (ties: the smaller n, then the smaller bases),
 *     d = min(cov[a'], cov[a'+1]).  A deletion and an insertion at one anchor are judged separately; the anchor's base may be N.
 *   Called iff d >= min_depth, c >= min_alt and c * 1000 >= het_pm * d; hom iff c * 1000 >= hom_pm * d, else het.
 *   het_pm = hom_pm: homozygous calls only.  Ascending by pos (the SNV's p, the indel's anchor); at one pos SNV, DEL, INS.
 * Outputs: *calls (release with np2_free; NULL when there is none), *n_calls; cov (or NULL): the caller's L words; alt (or
 *   NULL): the caller's 4 L words.
 * NP2_E_ARG before anything is launched, the context stays usable: hom_pm > 1000, het_pm > hom_pm, max_indel outside 1..28,
 * min_alt 0 (a call needs a read), min_aligned_fra outside [0, 1], a NULL argument, a record whose SEQ or CIGAR lies outside
 * its buffer (np2_varcall_host, which is given the sizes; np2_varcall_from_records takes the buffers to end where the last
 * record's data ends), a contig name the BAM header lacks.  L above 4294901760 is NP2_E_UNSUPPORTED. */
typedef struct np2_varcall_opts {
    double min_aligned_fra; /* --min_fra 0.0 */
    uint32_t min_depth;     /* -d 8 */
    uint32_t min_alt;       /* --min_alt 3 */
    uint32_t hom_pm;        /* --hom 0.8 -> 800 */
    uint32_t het_pm;        /* --het_frac 0.25 -> 250; = hom_pm: homozygous calls only */
    uint32_t max_indel;     /* --max_indel 28 */
    uint16_t exclude_flags; /* 0xF04: unmapped, secondary, QC fail, duplicate, supplementary */
    uint8_t min_mapq;       /* -q 5 */
} np2_varcall_opts_t;
typedef struct np2_varcall {
    uint32_t pos;     /* 0-based: the SNV's position, the indel's anchor (the base before it) */
    uint32_t depth;   /* d */
    uint32_t count;   /* c */
    uint32_t pad0;
    uint64_t bases;   /* INS: the inserted bases, 2 bits each, the first base highest; else 0 */
    uint8_t kind;     /* 0 SNV, 1 DEL, 2 INS */
    uint8_t gt;       /* 1 het, 2 hom */
    uint8_t len;      /* SNV 1; indel: n */
    uint8_t alt_code; /* SNV: the called base, A C G T = 0..3; else 0 */
    uint32_t pad1;
} np2_varcall_t;
typedef struct np2_varcall_stats {
    uint64_t records_seen;    /* handed in or fetched */
    uint64_t records_counted;
    uint64_t records_no_seq;  /* SEQ * or l_seq != the CIGAR's query length */
    uint64_t records_skipped; /* with an N operation */
    uint64_t events;          /* indel events of counted records */
    uint64_t alleles;         /* distinct keys among them */
    uint64_t callable;        /* positions with cov >= min_depth and an A C G T reference base */
    uint64_t calls[6];        /* [kind * 2 + gt - 1]: SNV het, SNV hom, DEL het, DEL hom, INS het, INS hom */
    float kernel_ms;          /* the kernels and sorts together (HIP events): the sum of stage_ms */
    float stage_ms[6];        /* records, coverage scan, key sorts, alleles, calls counted, calls written */
    uint32_t pad;
} np2_varcall_stats_t;
/* ref, recs, cigar, seq4 in host memory */
int np2_varcall_from_records(np2_ctx_t *ctx, const uint8_t *ref, uint32_t L, const np2_bamrec_t *recs, uint32_t n_recs,
                             const uint32_t *cigar, const uint8_t *seq4, const np2_varcall_opts_t *opts, np2_varcall_t **calls,
                             uint32_t *n_calls, uint32_t *cov /* [L] or NULL */, uint32_t *alt /* [4 L] or NULL */,
                             np2_varcall_stats_t *stats /* or NULL */);
/* the same over the records of contig `name` of an indexed BAM, fetched the way np2_contig_from_bam fetches them: records, CIGAR
 * words and SEQ stay where the reader left them (in HBM already on the device path; SEQ streamed there by the host pool) */
int np2_varcall_from_bam(np2_ctx_t *ctx, np2_bam_t *bam, const char *name, const uint8_t *ref, uint32_t L,
                         const np2_varcall_opts_t *opts, np2_varcall_t **calls, uint32_t *n_calls, uint32_t *cov /* [L] or NULL */,
                         uint32_t *alt /* [4 L] or NULL */, np2_varcall_stats_t *stats /* or NULL */);
/* the host twin: the same rule on one CPU thread, no device and no context (kernel_ms stays 0).  n_cigar_words and seq_bytes
 * are the sizes of cigar and seq4: a record that reaches beyond either is NP2_E_ARG */
int np2_varcall_host(const uint8_t *ref, uint32_t L, const np2_bamrec_t *recs, uint32_t n_recs, const uint32_t *cigar,
                     uint64_t n_cigar_words, const uint8_t *seq4, uint64_t seq_bytes, const np2_varcall_opts_t *opts,
                     np2_varcall_t **calls, uint32_t *n_calls, uint32_t *cov /* [L] or NULL */, uint32_t *alt /* [4 L] or NULL */,
                     np2_varcall_stats_t *stats /* or NULL */);
/* ---- an assembly's differences from a reference: alignments of its segments -> runs covered once (R) and calls (V) -------
 * The third over-correction measure of the reference's README (minimap2 -cx asm10 --cs | sort | paftools.js call, then
 * e_use_vcf.py), and the evaluation of a polish against a truth sequence.  THE RULE IS THIS PROJECT'S OWN: equality with
 * minimap2, paftools or any other caller is not claimed (no asm10 scoring, no second affine piece, no shifting of events).
 * Inputs, all in host memory: references T_0 .. T_{n-1} as bytes, case-insensitive, A C G T = codes 0..3, anything else N,
 *   as one concatenation refs with ref_off[n_refs + 1] (ref_off[0] = 0, ascending; reference t is refs[ref_off[t] ..
 *   ref_off[t + 1])); a query stream of bytes in the queries' FORWARD orientation; alignments (np2_asmaln_t) whose CIGAR
 *   (BAM words len << 4 | op) is in SAM orientation: with flag 16 SAM base j is the complement of forward byte q_len - 1 - j
 *   and the owned SAM interval is [q_len - own_hi, q_len - own_lo); otherwise both are the forward ones.
 * Admission: an alignment is admitted iff flag & 4 == 0 and n_cigar > 0 (else stats.alns_unaligned), mapq >= min_mapq (else
 *   stats.alns_low_mapq), every operation is M I D S = or X (an N, H or P operation or an operation code above 8:
 *   stats.alns_skipped) and its reference span, the sum of its M D = X lengths, is at least min_aln (else stats.alns_short);
 *   the first test that fails names the counter.
 * Anchor: an M, = or X column is its own anchor.  An I or D operation's anchor is the last M, = or X column before it in the
 *   CIGAR, however many I or D operations lie between; with no such column the operation is ignored, and so is an operation
 *   of length 0.  A column or operation BELONGS to the alignment iff its anchor's SAM query index lies in the owned SAM
 *   interval.
 * Coverage: every belonging M = X column covers its reference position, every belonging D the n positions it deletes; they
 *   form one interval per alignment, and cov[p] is the number of admitted alignments whose interval holds p.
 * Events of admitted alignments, among belonging columns and operations, where the CIGAR has them (nothing is shifted: the
 *   aligner left-aligns its gaps): SNV at p: an M or X column whose reference and query bases are both A C G T and differ.
 *   DEL (a, n): a D of n bases with anchor position a.  INS (a, n): an I of n bases (any bytes) with anchor position a.
 * Filter: an event is kept iff its whole footprint has cov == 1.  SNV: p.  DEL: a .. a + n.  INS: a, and a + 1 when
 *   a + 1 < |T_tid|.
 * R runs: the maximal runs of cov == 1 inside each reference (a run does not cross from one reference into the next).
 * Order: runs by (tid, start); events by (tid, pos, kind) with SNV < DEL < INS, then alignment index, then CIGAR order.
 * q_pos is a forward index in the alignment's query: SNV that base; INS the lowest forward index of the inserted bases; DEL
 *   the first forward base after the gap, which may be q_len.
 * Tiling (python -m nextpolish2_amd.asmcall, which cuts contigs into the queries): overlap is even, m = overlap / 2, step =
 *   seg - overlap.  A contig of length Lc < seg is one segment; otherwise there are n = max(1, (Lc - overlap) / step) (rounded
 *   down) segments, segment i is [i step, i step + seg) and the last one runs to Lc.  Segment i owns [i step + m, i step + seg
 *   - m) in contig coordinates, the first from 0 and the last to Lc: the owned intervals tile the contig.  q_base is the
 *   segment's start, own_lo / own_hi the owned interval minus q_base.
 * Outputs: *runs and *vars (release with np2_free; NULL when there is none) with their counts; cov (or NULL): the caller's
 *   ref_off[n_refs] words.
 * Checked on the host before anything is launched, the context stays usable.  NP2_E_ARG: a NULL argument, ref_off not
 *   ascending from 0, data outside its buffer (CIGAR words, query bytes), own_lo > own_hi or own_hi > q_len, and for an
 *   alignment with flag & 4 == 0, n_cigar > 0 and no operation but M I D S = X: a tid outside the references, pos + span > |T_tid|, a CIGAR query
 *   length (M I S = X) different from q_len.  NP2_E_UNSUPPORTED: total reference length above 4294901760, or query bytes +
 *   CIGAR words (the bound of the events) above 4294901760.
 * Not here: asm10's scoring and the second affine piece; segments that map across structural rearrangements (they fail
 *   min_aln or mapq and leave coverage 0); VCF output; several ranks; references or assemblies beyond one device's memory. */
typedef struct np2_asmaln {
    int32_t tid;
    uint32_t pos;              /* 0-based reference position of the first M = X column */
    uint32_t flag;             /* bit 16: reverse, bit 4: unaligned */
    uint32_t mapq, n_cigar;
    uint32_t q_len;            /* the query's bytes in the stream */
    uint32_t own_lo, own_hi;   /* the owned forward query interval, 0 <= own_lo <= own_hi <= q_len */
    uint32_t q_id, q_base;     /* reporting only: which contig, and the contig coordinate of query byte 0 */
    uint64_t cigar_off, q_off; /* first CIGAR word, first query byte */
} np2_asmaln_t;
typedef struct np2_asmcall_opts {
    uint32_t min_mapq; /* -q 5 */
    uint32_t min_aln;  /* --min_aln 5000 */
} np2_asmcall_opts_t;
typedef struct np2_asmrun {
    uint32_t tid, start, end; /* [start, end) inside reference tid */
} np2_asmrun_t;
typedef struct np2_asmvar {
    uint32_t tid;
    uint32_t pos;      /* the SNV's position, the indel's anchor */
    uint32_t aln;      /* index of the alignment */
    uint32_t len;      /* SNV 1; indel: n */
    uint32_t q_pos;    /* forward index in the alignment's query (above) */
    uint8_t kind;      /* 0 SNV, 1 DEL, 2 INS */
    uint8_t ref_code;  /* SNV: the reference base, A C G T = 0..3; else 0 */
    uint8_t alt_code;  /* SNV: the query base in the reference's orientation; else 0 */
    uint8_t rev;       /* 1: the alignment has flag 16 */
} np2_asmvar_t;
typedef struct np2_asmcall_stats {
    uint64_t alns_seen, alns_admitted, alns_skipped, alns_low_mapq, alns_short, alns_unaligned;
    uint64_t runs, r_bases;          /* R runs and the bases in them (cov == 1) */
    uint64_t cov0_bases, cov2_bases; /* reference bases at coverage 0 and at coverage >= 2 */
    uint64_t found[3], kept[3];      /* events by kind, before and after the filter */
    uint64_t ins_bases, del_bases;   /* of the kept events */
    float kernel_ms;                 /* the kernels and the sort together (HIP events): the sum of stage_ms */
    float stage_ms[9];               /* walk counted, coverage scan, cov == 1 counts, event offsets, walk written, runs, filter,
                                        sort, gather */
} np2_asmcall_stats_t;
int np2_asmcall(np2_ctx_t *ctx, const uint8_t *refs, const uint64_t *ref_off, uint32_t n_refs, const uint8_t *query,
                uint64_t query_bytes, const np2_asmaln_t *alns, uint32_t n_alns, const uint32_t *cigar, uint64_t n_cigar_words,
                const np2_asmcall_opts_t *opts, np2_asmrun_t **runs, uint32_t *n_runs, np2_asmvar_t **vars, uint32_t *n_vars,
                uint32_t *cov /* [ref_off[n_refs]] or NULL */, np2_asmcall_stats_t *stats /* or NULL */);
/* the host twin: the same rule on one CPU thread, no device and no context (kernel_ms stays 0) */
int np2_asmcall_host(const uint8_t *refs, const uint64_t *ref_off, uint32_t n_refs, const uint8_t *query, uint64_t query_bytes,
                     const np2_asmaln_t *alns, uint32_t n_alns, const uint32_t *cigar, uint64_t n_cigar_words,
                     const np2_asmcall_opts_t *opts, np2_asmrun_t **runs, uint32_t *n_runs, np2_asmvar_t **vars, uint32_t *n_vars,
                     uint32_t *cov /* [ref_off[n_refs]] or NULL */, np2_asmcall_stats_t *stats /* or NULL */);
/* ---- one reference interval of a contig straight from the BAM (multi-GPU: every rank parses only its part) -----------
 * begin: fetch the records overlapping [own_lo - halo, own_hi + halo) through the .bai linear index, admit + columnarise
 *        them; returns the BGZF virtual offsets of the pushed records that START in [own_lo, own_hi) (file order).
 *        The ranks' own intervals must tile the contig (np2_shard_plan's cuts: L * k / n rounded down to 1024).
 * exchange (caller): all-gather those lists in rank order -> the contig's pushed records in file order.
 * finish: numbers the shard's reads contig-wide (1 + place in that list; the reference numbers alignseqs in file order,
 *        main.rs:1813), applies the clip filter in contig coordinates, returns the shard's resident pileup, its plan for
 *        np2_shard_begin and the contig's read count for np2_vote_decide.  Consumes `io` (also on error). */
typedef struct np2_shard_io np2_shard_io_t;
int np2_shard_bam_begin(np2_ctx_t *ctx, np2_bam_t *bam, const char *name, const uint8_t *ref, uint32_t L, uint32_t own_lo,
                        uint32_t own_hi, uint32_t halo, const np2_front_opts_t *opts, np2_shard_io_t **io,
                        const uint64_t **own_voffsets, uint64_t *n_own);
int np2_shard_bam_finish(np2_shard_io_t *io, const uint64_t *all_voffsets, uint64_t n_all, np2_shard_plan_t *plan,
                         np2_contig_t **contig, uint32_t *n_reads_total);
void np2_shard_bam_abort(np2_shard_io_t *io);
/* A run of whole BGZF blocks (`bgzf`, `n` bytes: a BAM file or a piece of one that starts at a block) inflated on ctx's
 * device by the kernel np2_contig_from_bam uses, the bytes copied back to `out` (capacity out_cap; *out_len = what the
 * blocks hold).  kernel_ms (optional): the inflate kernel alone (HIP events).  For parity tests against zlib and for
 * measuring the kernel; the reference's counterpart is rust-htslib's bgzf reader (main.rs:1745-1757). */
int np2_bgzf_inflate_device(np2_ctx_t *ctx, const uint8_t *bgzf, uint64_t n, uint8_t *out, uint64_t out_cap, uint64_t *out_len,
                            float *kernel_ms);
/* CRC-32 (gzip) of n_pieces pieces of `data` — piece i = data[off[i], off[i+1]), each at most 65536 bytes — by the kernel the
 * read paths check every inflated BGZF block with (the block's CRC32 word; a mismatch is NP2_E_ARG "BGZF CRC32 mismatch
 * (block at file offset N)" on every path, host pool and device; NP2_BGZF_CRC=0, read once per process, switches the check
 * off for A/B timing).  kernel_ms (optional): that kernel alone (HIP events).  A piece longer than 65536 bytes, descending
 * offsets or off[n_pieces] > n: NP2_E_ARG.  The reference's counterpart: htslib's bgzf reader checks each block's CRC. */
int np2_crc32_device(np2_ctx_t *ctx, const uint8_t *data, uint64_t n, const uint64_t *off, uint32_t n_pieces,
                     uint32_t *crc_out, float *kernel_ms);
/* ---- BGZF output: DEFLATE on the device, the counterpart of np2_bgzf_inflate_device ----------------------------------------
 * Host bytes become a whole BGZF stream: blocks of block_bytes input bytes (0: 65280, htslib's; else 1 .. 65280; more is
 * NP2_E_ARG), each an 18-byte header with the BC subfield, one raw DEFLATE stream, CRC32 and ISIZE, then the canonical
 * 28-byte EOF block; n = 0 gives the EOF block alone.  A block is tokenised with LZ77 (matches of 8 .. 258 bytes, at most
 * 32768 back, every candidate verified on the input bytes) and coded as one dynamic Huffman block (codes of at most 15 bits,
 * HLIT / HDIST / HCLEN trimmed), or stored when that would be no smaller than its bytes + 5: no block is larger than 65536
 * bytes.  THE BYTES ARE A FUNCTION OF THE INPUT BYTES AND block_bytes ALONE: not of timing, of what the buffers held before,
 * or of where they are computed — np2_bgzf_deflate_host, which uses no device, runs the same code on the CPU (64 lanes in
 * turn) and returns the same bytes; it exists for tests and as the statement of what the kernel must produce.
 * *out_len = the stream's bytes; out_cap too small is NP2_E_ARG, the message says how many are needed (never more than
 * n + 31 per block + 28).  kernel_ms (optional): the deflate kernel alone (HIP events).  Errors: np2_io_last_error().
 * The reference's counterpart: gzip on the host behind its recipe's sr.R1.clean.fastq.gz. */
int np2_bgzf_deflate_device(np2_ctx_t *ctx, const uint8_t *data, uint64_t n, uint32_t block_bytes, uint8_t *out, uint64_t out_cap,
                            uint64_t *out_len, float *kernel_ms);
int np2_bgzf_deflate_host(const uint8_t *data, uint64_t n, uint32_t block_bytes, uint8_t *out, uint64_t out_cap, uint64_t *out_len);
/* A BGZF file written through `device`.  The writer owns a stream and two batches of pinned and device buffers: one batch
 * (256 blocks; NP2_BGZF_TEST_BATCH, in blocks, a test hook read once per writer) is compressed while the caller fills the
 * next.  Blocks are cut every 65280 bytes whatever the sizes of the write calls, so the file is np2_bgzf_deflate_host of
 * the bytes written.  close flushes the partial block, appends the EOF block, reports a write error as NP2_E_ARG "cannot
 * write <path>" and releases the handle whatever it returns; bytes_in / bytes_out / kernel_ms (any may be NULL): what was
 * written to the handle, to the file, and the ms in the deflate kernel.  After a failed write, close adds no EOF block: a
 * writer abandoned on an error leaves a file that readers see as truncated.  Errors: np2_io_last_error(). */
typedef struct np2_bgzf_writer np2_bgzf_writer_t;
int np2_bgzf_writer_open(int device, const char *path, np2_bgzf_writer_t **out);
int np2_bgzf_writer_write(np2_bgzf_writer_t *w, const void *p, uint64_t n);
int np2_bgzf_writer_close(np2_bgzf_writer_t *w, uint64_t *bytes_in, uint64_t *bytes_out, float *kernel_ms);
/* copy a resident packed pileup back to the host (parity tests / debugging); free both with np2_free */
int np2_contig_export(np2_ctx_t *ctx, np2_contig_t *c, np2_read_t **reads, uint32_t *n_reads,
                      uint8_t **nibbles, uint64_t *nib_bytes);

/* ---- k-mer counting: short reads -> yak tables (the `yak count` half of the reference workflow, README steps 2-3) ----
 * Canonical k-mers of FASTA / FASTQ / one-sequence-per-line files (plain or gzip) counted on the device, with the
 * semantics of the reference's lookup side (kmer.rs:255-287 iter2kmer, 102-110 to_hash, 52-58 file word): for every k-mer
 * of the reads, KmerInfo::get on the result returns min(occurrences, 1023).  Words inside a bucket are written in
 * ascending order.  Errors: np2_io_last_error().  Arguments (k, paths, options) are checked before the first device call:
 * k >= 32 or k < 2 is NP2_E_UNSUPPORTED, a file that cannot be opened or a damaged / truncated gzip NP2_E_ARG.
 * Test hooks, read once per call: NP2_KCOUNT_TEST_CAP_LOG2 (initial sub-table capacity), NP2_KCOUNT_TEST_PIECE (piece size
 * in bytes), NP2_KCOUNT_TEST_PASSES (bucket-range passes). */
typedef struct np2_kcount_opts {
    uint16_t min_count; /* words below it are not emitted (an exact threshold); 0 and 1: everything */
    uint64_t mem_bytes; /* device memory for the counting tables of all k together; 0: half of what is free at the call.
                         * A run that would outgrow it counts in several passes over bucket ranges, reading its input again
                         * for each (an input that cannot be read again, a pipe, is NP2_E_ARG in that case only) */
} np2_kcount_opts_t;
/* sequence files -> one table per ks[i]; out[i] released with np2_yak_free */
int np2_kcount_files(int device, const char *const *paths, int n_paths, const uint32_t *ks, int n_k,
                     const np2_kcount_opts_t *opts, np2_yak_t *out /* [n_k] */);
/* the same over a separator stream in host memory: the reads' bytes with one '\n' (any non-base byte) between reads */
int np2_kcount_bytes(int device, const uint8_t *seq, uint64_t n, const uint32_t *ks, int n_k,
                     const np2_kcount_opts_t *opts, np2_yak_t *out);
/* straight to yak v2 dumps on disk, bucket by bucket (no host copy of a whole table) */
int np2_kcount_files_to_dumps(int device, const char *const *paths, int n_paths, const uint32_t *ks, int n_k,
                              const np2_kcount_opts_t *opts, const char *const *out_paths);
/* straight to a polish context: the tables never leave HBM (ordered by k).  Single-pass runs only: a run that would need
 * passes returns NP2_E_NOMEM and says so */
int np2_ctx_create_from_reads(np2_ctx_t **out, int device, const char *const *paths, int n_paths,
                              const uint32_t *ks, int n_k, const np2_kcount_opts_t *opts);
/* statistics of the last successful counting call on this thread (any pointer may be NULL): k-mers hashed and slots
 * claimed (summed over the k values), hashes that went through the spill list, table growths, passes, ms in the count
 * kernel (HIP events), ms the counting thread waited for its reader threads */
int np2_kcount_last_stats(uint64_t *kmers, uint64_t *distinct, uint64_t *spilled, uint32_t *growths, uint32_t *passes,
                          float *kernel_ms, float *read_ms);
/* host only, no device: the separator stream the reader makes of one sequence file (every read followed by one '\n');
 * release with np2_free */
int np2_seqfile_stream(const char *path, uint8_t **out, uint64_t *n);

/* ---- short-read quality trimming and filtering in front of the k-mer counter ---------------------------------------------
 * The preparation step the reference's README calls essential (its recipe: fastp -5 -3 -n 0 -f 5 -F 5 -t 5 -T 5 -q 20),
 * on the device.  THE RULE IS DEFINED HERE, on the options of that recipe; it is not pinned against the fastp binary.
 * One read has n bases s[0..n) and n quality bytes, p[i] = max(0, byte - 33).
 *   1. a = min(trim_front, n), b = max(a, n - trim_tail) (saturating at 0): the kept span is [a, b).
 *   2. cut_front, if on and b > a: the smallest i with a <= i, i + W <= b and p[i] + .. + p[i+W-1] >= M * W.  No such i
 *      (b - a < W included): a = b.  Otherwise a = i, then a += 1 while a < b and s[a] is N or n.
 *   3. cut_tail, if on and b > a: the largest j with j <= b, j - W >= a and p[j-W] + .. + p[j-1] >= M * W.  No such j:
 *      b = a.  Otherwise b = j, then b -= 1 while b > a and s[b-1] is N or n.
 *   4. len = b - a, nN = N / n in [a, b), lowq = positions of [a, b) with p < Q.  Class, in this order: 1 too short
 *      (len < min_len or len == 0), 2 too many N (nN > n_base_limit), 3 low quality (100 * lowq > U * len), else 0 pass.
 *   5. The masked stream: every base of a failed read, and every base of a passing read outside [a, b), becomes 'N';
 *      separators stay.  Counting it gives the tables of the kept substrings counted as reads of their own.
 * Reads are judged one by one (paired files are not kept in step); no adapter, poly-G / poly-X, complexity or
 * average-quality filter.  Options out of range are NP2_E_ARG before the first device call.  Inputs are FASTQ, plain or
 * gzip: FASTA or one sequence per line is NP2_E_ARG naming the file, a record whose quality line is not as long as its
 * sequence NP2_E_ARG naming the file and the 1-based record.  The streams are filtered in pieces that end at a read
 * boundary (8 MiB; NP2_KCOUNT_TEST_PIECE): a read that does not fit an empty piece is NP2_E_UNSUPPORTED. */
#define NP2_SRQC_CUT_FRONT 1u
#define NP2_SRQC_CUT_TAIL 2u
typedef struct np2_srqc_opts {
    uint32_t trim_front;          /* -f / -F 5 */
    uint32_t trim_tail;           /* -t / -T 5 */
    uint32_t cut_window;          /* W: 4, 1 .. 1000 */
    uint32_t cut_mean_q;          /* M: 20, 0 .. 93 */
    uint32_t n_base_limit;        /* -n 0 */
    uint32_t qualified_q;         /* Q: -q 20, 0 .. 93 */
    uint32_t unqualified_percent; /* U: 40, 0 .. 100 */
    uint32_t min_len;             /* 15 */
    uint32_t flags;               /* NP2_SRQC_CUT_FRONT (-5) | NP2_SRQC_CUT_TAIL (-3) */
} np2_srqc_opts_t;
typedef struct np2_srqc_read {
    uint32_t begin, end; /* a and b of the rule as step 4 sees them, from the read's first base */
    uint32_t cls;        /* 0 pass, 1 too short, 2 too many N, 3 low quality */
} np2_srqc_read_t;
typedef struct np2_srqc_stats {
    uint64_t reads, pass, too_short, too_many_n, low_quality, bases_in, bases_out;
} np2_srqc_stats_t;
/* One pair of streams in host memory (the reads' bases / quality bytes, every read followed by one '\n' in both; n bytes
 * each), walked piece by piece.  masked_out (or NULL): n bytes, the masked stream.  reads_out (or NULL): one entry per
 * read.  n_reads must be the number of separators (NP2_E_ARG otherwise); the last byte of a stream that is not empty must
 * be one.  stats may be NULL.  Errors: np2_io_last_error(). */
int np2_srqc_bytes(int device, const uint8_t *seq, const uint8_t *qual, uint64_t n, const np2_srqc_opts_t *opts,
                   uint8_t *masked_out, np2_srqc_read_t *reads_out, uint64_t n_reads, np2_srqc_stats_t *stats);
/* FASTQ files -> totals (stats: [n_paths + 1], per file and then the sum; or NULL) and, with out_paths (or NULL; single
 * entries may be NULL), one cleaned plain-text FASTQ per input: the passing reads in file order, each the header line as
 * read, the kept bases, "+", the kept qualities.  An output path ending in .gz or .bgz is written as BGZF, compressed on
 * `device` (np2_bgzf_writer_* below); every other path is the plain text. */
int np2_srqc_files(int device, const char *const *paths, int n_paths, const np2_srqc_opts_t *opts,
                   const char *const *out_paths, np2_srqc_stats_t *stats);
/* the totals of the last filtering call on this thread (of a multi-pass count: of one pass, not the sum over passes) */
int np2_srqc_last_stats(np2_srqc_stats_t *stats);
/* ms in the filter kernel during that call (HIP events) */
int np2_srqc_last_kernel_ms(float *ms);
/* The three counting entry points with the filter in front of the counter: qc == NULL is exactly the call without it.
 * Every input must then be FASTQ. */
int np2_kcount_files_qc(int device, const char *const *paths, int n_paths, const uint32_t *ks, int n_k,
                        const np2_kcount_opts_t *opts, const np2_srqc_opts_t *qc, np2_yak_t *out /* [n_k] */);
int np2_kcount_files_to_dumps_qc(int device, const char *const *paths, int n_paths, const uint32_t *ks, int n_k,
                                 const np2_kcount_opts_t *opts, const np2_srqc_opts_t *qc, const char *const *out_paths);
int np2_ctx_create_from_reads_qc(np2_ctx_t **out, int device, const char *const *paths, int n_paths, const uint32_t *ks,
                                 int n_k, const np2_kcount_opts_t *opts, const np2_srqc_opts_t *qc);
/* host only, no device: the two streams the reader makes of one FASTQ file (n bytes each; release both with np2_free) */
int np2_seqfile_stream_qual(const char *path, uint8_t **seq, uint8_t **qual, uint64_t *n);

/* ---- short-read adapter trimming in front of the k-mer counter: pair overlap and sequence ------------------------------------
 * What fastp does by default for paired input beside the quality rule above: it finds where the two mates overlap, cuts the
 * read-through adapter off both, and drops a pair as soon as one mate fails.  THE RULE IS DEFINED HERE, on fastp's documented
 * options (overlap_len_require 30, overlap_diff_limit 5, overlap_diff_percent_limit 20, -a / --adapter_sequence,
 * --adapter_sequence_r2); no fastp binary was at hand, and equality with fastp is not claimed.
 * Notation: a base byte is case-folded; A/T and C/G are complements; any other byte is unknown and matches nothing.  Steps
 * 1 - 3 of the quality rule run first, on each read alone, unchanged, and give the kept span [a, b).  With qc == NULL they run
 * with every step off (trims 0, no cuts, n_base_limit 2^32 - 1, Q 0, U 100, min_len 0): the span is the whole read, and step 4
 * below fails only a read that A or B left empty (class 1).
 *   A. Pair overlap (pair mode only).  x = r1[a1, b1), n1 long; y = r2[a2, b2), n2 long; rcy the reverse complement of y.
 *      For a shift s, x[i] faces rcy[i - s].  The overlap is i in [max(0, s), min(n1, n2 + s)), l(s) positions; d(s) is the
 *      number of them where x[i] is unknown, rcy[i - s] is unknown, or the two differ.  s is accepted if l(s) >= O and
 *      d(s) <= min(D, floor(P * l(s) / 100)).  Candidates are tried in the order s = 0, 1, 2, .., then s = -1, -2, ..; the
 *      first accepted one wins (the smallest accepted s >= 0; if there is none, the accepted s < 0 nearest to 0).  On
 *      acceptance T = n2 + s is the insert length as the kept spans see it, b1 = a1 + min(n1, T), b2 = a2 + min(n2, T).  An
 *      accepted s > 0 with n1 <= T trims nothing (an overlap without read-through) and still ends the search.  A pair has no
 *      overlap when either kept span is longer than 1024 bases (the cap bounds the per-wavefront LDS) or shorter than O.
 *   B. Adapter by sequence, for a read step A did not decide: in single mode every read, in pair mode both mates of a pair
 *      with no accepted s.  adapter1 is used for single reads and mate 1, adapter2 for mate 2 (NULL: adapter1); without a
 *      string the step does nothing.  With A the adapter's length and n = b - a (4 <= n <= 1024; other spans are left as
 *      they are): for p = 0 .. n - 4, c = min(n - p, A), m(p) = #{ j < c : fold(read[a + p + j]) != adapter[j] }.  The
 *      smallest p with m(p) <= floor(c / 8) wins, and b = a + p.
 *   C. Step 4 of the quality rule classifies the new [a, b) of every read (classes 0 - 3 unchanged).  In pair mode, if exactly
 *      one mate has a class other than 0, the other mate gets class 4, mate failed.  Masking is step 5 of the quality rule
 *      over the final span and class.
 * Options: O in [1, 1024], D in [0, 1024], P in [0, 100]; an adapter string is 4 - 64 letters of ACGT (upper case); adapter2
 * needs adapter1, and single mode needs adapter1; anything else is NP2_E_ARG before the first device call.
 * Out of scope: interleaved FASTQ, read-name checks (names are not compared), fastp's base correction inside the overlap,
 * merging mates, poly-G / poly-X, adapter auto-detection for single-end input, equality with the fastp binary. */
#define NP2_SRADAPT_PAIRED 1u
typedef struct np2_sradapt_opts {
    uint32_t flags;                /* NP2_SRADAPT_PAIRED: reads 2r and 2r + 1 (files 2i and 2i + 1) are mates */
    uint32_t overlap_min;          /* O: 30 */
    uint32_t overlap_diff;         /* D: 5 */
    uint32_t overlap_diff_percent; /* P: 20 */
    const char *adapter1;          /* or NULL */
    const char *adapter2;          /* or NULL: adapter1 */
} np2_sradapt_opts_t;
typedef struct np2_sradapt_read {
    uint32_t begin, end; /* the final [a, b), from the read's first base */
    uint32_t cls;        /* 0 pass, 1 too short, 2 too many N, 3 low quality, 4 mate failed */
    uint32_t how;        /* 0 untouched by A and B, 1 end moved by A, 2 end moved by B */
    uint32_t insert;     /* T for both mates of a pair with an accepted s, otherwise 0 */
} np2_sradapt_read_t;
typedef struct np2_sradapt_stats {
    uint64_t reads, pass, too_short, too_many_n, low_quality, bases_in, bases_out; /* as np2_srqc_stats_t, of the final classes */
    uint64_t mate_failed;      /* reads of class 4 */
    uint64_t pairs;
    uint64_t pairs_overlap;    /* pairs with an accepted s */
    uint64_t pairs_unsearched; /* pairs past the 1024-base cap */
    uint64_t trimmed_overlap;  /* reads with how 1 */
    uint64_t trimmed_seq;      /* reads with how 2 */
    uint64_t adapter_bases;    /* bases removed by A and B, over all reads */
} np2_sradapt_stats_t;
/* np2_srqc_bytes with the adapter rule.  qc == NULL: see above; ad == NULL: pair mode with the defaults and no sequences.
 * In pair mode the mates are adjacent (read 2r is mate 1, read 2r + 1 mate 2), an odd n_reads is NP2_E_ARG, and a pair
 * that does not fit a piece is NP2_E_UNSUPPORTED. */
int np2_sradapt_bytes(int device, const uint8_t *seq, const uint8_t *qual, uint64_t n, const np2_srqc_opts_t *qc,
                      const np2_sradapt_opts_t *ad, uint8_t *masked_out, np2_sradapt_read_t *reads_out, uint64_t n_reads,
                      np2_sradapt_stats_t *stats);
/* FASTQ files -> totals and, with out_paths (or NULL), one cleaned plain-text FASTQ per input.  In pair mode the paths are
 * R1, R2, R1, R2, .. (an odd n_paths is NP2_E_ARG), the two files of a pair are read in step (files whose record counts
 * differ are NP2_E_ARG; the message names both files and the first record, 1-based, that the shorter one lacks), and a
 * pair is written only when both mates pass, so the outputs stay in step.  stats (or NULL): one entry per unit, a file in
 * single mode and a pair of files in pair mode, then the sum.  An output path ending in .gz or .bgz is written as BGZF,
 * compressed on `device` (np2_bgzf_writer_* below); every other path is the plain text. */
int np2_sradapt_files(int device, const char *const *paths, int n_paths, const np2_srqc_opts_t *qc, const np2_sradapt_opts_t *ad,
                      const char *const *out_paths, np2_sradapt_stats_t *stats);
/* the totals of the last adapter-trimming call on this thread (of a multi-pass count: of one pass) and its kernel's ms */
int np2_sradapt_last_stats(np2_sradapt_stats_t *stats);
int np2_sradapt_last_kernel_ms(float *ms);
/* The three *_qc counting entry points with the adapter rule in front of the counter: ad == NULL is exactly the *_qc call.
 * Every input must be FASTQ; in pair mode the paths are R1, R2, R1, R2, .. */
int np2_kcount_files_ad(int device, const char *const *paths, int n_paths, const uint32_t *ks, int n_k, const np2_kcount_opts_t *opts,
                        const np2_srqc_opts_t *qc, const np2_sradapt_opts_t *ad, np2_yak_t *out /* [n_k] */);
int np2_kcount_files_to_dumps_ad(int device, const char *const *paths, int n_paths, const uint32_t *ks, int n_k,
                                 const np2_kcount_opts_t *opts, const np2_srqc_opts_t *qc, const np2_sradapt_opts_t *ad,
                                 const char *const *out_paths);
int np2_ctx_create_from_reads_ad(np2_ctx_t **out, int device, const char *const *paths, int n_paths, const uint32_t *ks, int n_k,
                                 const np2_kcount_opts_t *opts, const np2_srqc_opts_t *qc, const np2_sradapt_opts_t *ad);

/* Read files -> classes (np2_bin_stream's device path, fed by the counter's reader threads through pinned pieces, in
 * file order; errors: np2_last_error(ctx)).  A read's name is its header up to the first whitespace, without '>' / '@';
 * a record without one (one sequence per line) is named by its 1-based number in its file.  Every path of `out` may be
 * NULL: tsv (a header line, then per read: read class s_pat s_mat n_pat n_mat pm mp kmers len), pat_list / mat_list (the
 * names of the paternal bin p, a, 0 / the maternal bin m, a, 0), pat_fa / mat_fa (the two bins as FASTA, one line per
 * sequence, qualities dropped).  A path of `out` ending in .gz or .bgz is written as BGZF, compressed on ctx's device
 * (np2_bgzf_writer_* below); every other path is a plain file.  counts (or NULL): reads of class p, m, a, 0. */
typedef struct np2_bin_out { const char *tsv, *pat_list, *mat_list, *pat_fa, *mat_fa; } np2_bin_out_t;
int np2_bin_files(np2_ctx_t *ctx, int pat_idx, int mat_idx, const char *const *paths, int n_paths,
                  const np2_bin_opts_t *opts, const np2_bin_out_t *out, uint64_t *counts /* [4] */, float *kernel_ms);
/* host only, no device: what that reader makes of one file.  names: the reads' names, each followed by '\n'
 * (names_bytes bytes); ends: per read the offset of its separator in the file's separator stream; release both with
 * np2_free.  Errors: np2_io_last_error(). */
int np2_seqfile_reads(const char *path, char **names, uint64_t *names_bytes, uint64_t **ends, uint64_t *n_reads);

/* ---- the repetitive k-mers of an assembly (the list winnowmap -W takes; the reference's README, "General usage" step 1:
 * meryl count k=15 output merylDB asm.fa.gz; meryl print greater-than distinct=0.9998 merylDB > repetitive_k15.txt) ----------
 * THE RULE IS DEFINED HERE, on meryl's documented options; it is not pinned against the meryl binary.
 *   Input: FASTA files, plain or gzip, through the counter's reader into a separator stream (np2_seqfile_stream).
 *   Bases: ACGTU in either case are 0..3 (U is counted and printed as T); every other byte (N, separators, bytes >= 0x80)
 *     ends the run of bases.
 *   k: 2 <= k <= 16, 15 by default; anything else is NP2_E_UNSUPPORTED.  A k-mer's index is v = min(fw, rv): its forward and
 *     reverse-complement 2-bit words, first base most significant, A=0 C=1 G=2 T=3: the lexicographically smaller of the two
 *     strings.  A palindrome (even k) is counted once per occurrence.  count[v], a uint32, is the number of stream positions
 *     whose k-mer has index v.  A stream that could hold more than 2^32 - 1 k-mers is NP2_E_UNSUPPORTED (for gzip input this
 *     shows only as the file is read).  A table (4 * 4^k bytes: 4 GiB at k = 15, 16 GiB at k = 16) that does not fit the
 *     device's free memory is NP2_E_NOMEM, and the message says so.
 *   Threshold: D = indices with count > 0, cum(c) = those of them with count <= c.  With distinct = f, 0 <= f <= 1 (NaN or
 *     out of range is NP2_E_ARG): target = (uint64_t)(f * (double)D) in IEEE double, and the threshold is the smallest count
 *     value c that occurs in the table with cum(c) >= target; with f = 0 the smallest occurring count.  With use_min_count
 *     (meryl's greater-than N) the threshold is min_count and distinct is not read.  D = 0: threshold 0, an empty list, NP2_OK.
 *   Listed: every index with count > threshold, in ascending v (ascending ACGT text); in the file one line "KMER\tCOUNT\n"
 *     each, upper-case letters.  both_strands writes a listed k-mer's reverse complement on the line after it with the same
 *     count, unless the k-mer is its own reverse complement (which strand winnowmap's reader expects is not checked here).
 * Every argument is checked before the first device call.  Errors: np2_io_last_error().  Test hook, read once per call:
 * NP2_REP_TEST_PIECE (piece size in bytes; the stream is uploaded in pieces of 8 MiB with a 32-byte halo). */
typedef struct np2_rep_opts {
    uint32_t k;             /* 15 */
    uint32_t use_min_count; /* 0: distinct decides; otherwise min_count does */
    uint32_t min_count;     /* greater-than N */
    double distinct;        /* 0.9998 */
} np2_rep_opts_t;
typedef struct np2_rep_stats {
    uint64_t kmers;              /* k-mers counted: the sum of all counters */
    uint64_t distinct;           /* D */
    uint64_t listed;             /* indices with count > threshold */
    uint64_t listed_occurrences; /* the sum of their counts */
    uint32_t threshold, max_count;
    float count_ms, select_ms, emit_ms; /* the three stages' kernels (HIP events) */
} np2_rep_stats_t;
/* a separator stream in host memory -> the list: index[i] ascending, count[i]; both released with np2_free, both NULL when
 * nothing is listed.  stats may be NULL. */
int np2_rep_bytes(int device, const uint8_t *seq, uint64_t n, const np2_rep_opts_t *opts, uint32_t **index, uint32_t **count,
                  uint64_t *n_listed, np2_rep_stats_t *stats);
/* FASTA files -> the text file out_path */
int np2_rep_files(int device, const char *const *paths, int n_paths, const np2_rep_opts_t *opts, const char *out_path,
                  int both_strands, np2_rep_stats_t *stats);

/* ---- HiFi reads mapped to the assembly: minimizer seeds chained into PAF (the reference's README, "General usage" step 2:
 * winnowmap -W repetitive_k15.txt -ax map-pb asm.fa.gz hifi.fa.gz; here the seed-and-chain half, as `minimap2 -x map-hifi`
 * without -a prints it) ------------------------------------------------------------------------------------------------------
 * THE RULE IS DEFINED HERE, on minimap2's published algorithm (Li 2018, Bioinformatics 34:3094; the integer chaining score of
 * minimap2 <= 2.17).  No minimap2 binary was at hand: equality with its output is not claimed and not tested.
 *   Options (np2_map_opts_t; defaults in brackets): k [19], w [19], max_occ [200], lookback [64], max_gap [10000], bandwidth
 *     [500], min_cnt [3], min_score [40].  11 <= k <= 28, 1 <= w <= 64, 1 <= lookback <= 64, anything else is
 *     NP2_E_UNSUPPORTED; max_occ 1 .. 2^20, max_gap 1 .. 2^30, bandwidth <= 2^20, min_cnt and min_score <= 2^30, anything else
 *     is NP2_E_ARG.  An index is built with k and w; mapping against it with another k or w is NP2_E_ARG.
 *   Sketch (assembly and reads alike).  Bases: ACGT in either case are 0..3; every other byte (N, U, separators, bytes >= 0x80)
 *     ends the run of bases.  The k-mer ending at byte i has the forward word fw and the reverse-complement word rv, first base
 *     most significant; its strand bit is fw > rv and its hash h = yak_hash64(min(fw, rv), 2k-bit mask) (minimap2's hash64).  A
 *     k-mer with fw == rv (even k only) is never chosen, but it does not end the run.  A window is w consecutive k-mer end
 *     positions inside one run of bases.  Position i is a minimizer if and only if some window holds it and (h_i, i) is the
 *     lexicographic minimum of that window over its k-mers with fw != rv: the leftmost of equal hashes wins.  A run with fewer
 *     than w k-mers has no minimizer.
 *   Index.  The assembly's minimizers (h, tid, end position, strand), stably sorted by h from (tid, position) order; occ(h) is
 *     the length of the run of equal h.  It stays in device memory behind the handle.
 *   Seeds.  Every read minimizer with 1 <= occ <= max_occ gives one anchor per index entry: rel = read strand ^ assembly
 *     strand, r = the entry's end position, q = the read k-mer's end position if rel == 0, else qlen - 1 - (end - (k - 1)): its
 *     end on the reverse-complemented read.  A read's anchors are ordered by (rel, tid, r, q).  A minimizer with occ > max_occ
 *     is dropped (and counted), not down-weighted.
 *   Chain.  For anchor i and each j in [max(0, i - lookback), i): j is admissible when it has i's rel and tid, 0 < dr = r_i -
 *     r_j <= max_gap, 0 < dq = q_i - q_j <= max_gap and dd = |dr - dq| <= bandwidth; sc = min(dr, dq, k) - (dd * k / 100 +
 *     (dd > 0 ? ilog2(dd) >> 1 : 0)) in integers with floor division; f[i] = max(k, max_j f[j] + sc); p[i] is the best j, of
 *     equal candidates the largest, and -1 when no candidate exceeds k.  The primary chain ends at the smallest i with the
 *     largest f (s1) and is followed back through p; its anchors are marked.  One forward sweep over the unmarked anchors:
 *     base[i] = 0 if p[i] < 0, f[p[i]] if p[i] is marked, else base[p[i]]; s2 = max(f[i] - base[i]) over them, 0 if there is
 *     none.  With n the chain's anchors, mapq = min(60, (60 * (s1 - s2) / s1) * min(n, 10) / 10), integer divisions in that
 *     order.  A read with n < min_cnt or s1 < min_score is unmapped (tid -1).
 *   Hit.  On the chain's strand the chain covers q' in [q_first - k + 1, q_last + 1) and t in [r_first - k + 1, r_last + 1);
 *     for rel == 1, qs = qlen - q'_end and qe = qlen - q'_start.  matches (PAF column 10) is k for the first anchor plus
 *     min(k, dr, dq) for each later one; block (column 11) is max(qe - qs, te - ts).  A PAF line is
 *     qname qlen qs qe +/- tname tlen ts te matches block mapq tp:A:P cm:i:n s1:i:s1 s2:i:s2, tab-separated, one per mapped
 *     read in read order; a name is the header up to the first whitespace (a record without one: its 1-based number).
 *   Weights (winnowmap -W; the _w entries below).  THE RULE IS DEFINED HERE, on winnowmap's published weighted minimizer
 *     sampling (Jain et al. 2020, Bioinformatics 36:i111); no winnowmap binary was at hand and equality with it is not claimed.
 *     A weight set is (kw, L): L a set of canonical k-mer indices v = min(fw, rv) of length kw, in np2_rep_*'s encoding (A=0
 *     C=1 G=2 T=3, first base most significant), 11 <= kw <= 15; a non-empty set with another kw is NP2_E_UNSUPPORTED (16 <= k
 *     <= 28 would need more than a direct-addressed bitmap).  An index built with weights requires opts.k == kw, otherwise
 *     NP2_E_ARG with both values in the message.  An empty set has kw = 0, fits any k and is the unweighted mapper.
 *     Order.  M = 4^k - 1, h the k-mer's hash as above (k <= 15: h < 2^30).  A k-mer not in L has key = h.  A k-mer in L has
 *     y = M - h, s(y) = (y * y) >> 2k, y8 = s(s(s(y))) and key = M - y8: the fixed-point form of winnowmap's x -> x^8, mirrored
 *     because the smallest hash wins here; the products fit 64 bits and no floating point is used.  Position i is a minimizer
 *     if and only if some window holds it and (key_i, h_i, i) is the lexicographic minimum of that window over its k-mers with
 *     fw != rv: equal keys (y8 collapses) are broken by h, then by leftmost.  A palindrome is never chosen, listed or not.  A
 *     minimizer's identity in the index and in seeding stays h.  max_occ, seeding, chaining, mapq and alignment are untouched.
 *     The assembly and the reads are sketched under the same weights: they belong to the index, which copies what it needs.
 *     List file.  One k-mer a line, KMER or KMER<TAB>anything; ACGT in either case, U read as T; all lines of one length, kw;
 *     \n and \r\n end a line; a k-mer given in either or both orientations sets the one canonical bit; duplicates are
 *     allowed; a bad letter or a line of another length is NP2_E_ARG with the 1-based line number; an empty file is the empty
 *     set; plain text or gzip.  (python -m nextpolish2_amd.repkmers writes such a list.)
 *   Not built: -f occurrence fractions (secondary and supplementary chains: "More chains", below); homopolymer compression; weights for k >= 16 or
 *     per-k-mer weights other than the eighth power;
 *     several devices; an index beyond one device's memory (base-level alignment and SAM: np2_map_align_*, below).
 *     NP2_E_UNSUPPORTED: an assembly of 2^32 bytes or more, a sequence or read longer than 2^31 - 1, a single read with more
 *     anchors than the device budget (2^25).
 * Every argument is checked before the first device call.  Errors: np2_io_last_error().  Test hooks, read once per call:
 * NP2_MAP_TEST_PIECE (bytes; a batch of reads goes up and is sketched in pieces of 8 MiB, eight pieces a batch, wherever the
 * boundary falls in a read), NP2_MAP_TEST_BUDGET (anchors; a batch beyond it is chained in groups of whole reads) and
 * NP2_MAP_TEST_COARSE (0: an index built with weights goes without the coarse level of its bitmap; the results are the same). */
typedef struct np2_map_opts {
    uint32_t k, w, max_occ, lookback, max_gap, bandwidth, min_cnt, min_score;
} np2_map_opts_t;
typedef struct np2_map_hit {
    int32_t tid;                     /* -1: unmapped (only qlen is set then) */
    uint32_t qlen, qs, qe, rev;      /* rev: rel of the chain, 1 = the read's reverse complement matches */
    uint32_t ts, te, matches, block, mapq;
    uint32_t n, s1, s2;              /* cm:i, s1:i, s2:i */
} np2_map_hit_t;
typedef struct np2_map_stats {
    uint64_t reads, mapped, unmapped;
    uint64_t minimizers;             /* of the reads */
    uint64_t anchors, dropped_occ;   /* dropped_occ: read minimizers with occ > max_occ */
    uint64_t index_minimizers;
    uint32_t pieces, groups;
    float sketch_ms, seed_ms, sort_ms, chain_ms; /* the stages' HIP events, summed over batches; 0 from np2_map_host */
    float read_ms, write_ms;         /* np2_map_files: the device thread's wait for its readers, and formatting and writing the PAF */
} np2_map_stats_t;
typedef struct np2_map_index np2_map_index_t;
/* An assembly -> its index on `device`; opts gives k and w (the other options are checked too).  From a separator stream in
 * host memory (every sequence followed by '\n'); names: the sequences' names, each followed by '\n', or NULL (1-based
 * numbers).  From FASTA files, plain or gzip, in the order given. */
int np2_map_index_bytes(int device, const uint8_t *stream, uint64_t n, const char *names, const np2_map_opts_t *opts, np2_map_index_t **out);
int np2_map_index_files(int device, const char *const *paths, int n_paths, const np2_map_opts_t *opts, np2_map_index_t **out);
void np2_map_index_free(np2_map_index_t *ix);
/* any of the outputs may be NULL; build_ms: the build's kernels and sorts (HIP events) */
int np2_map_index_info(const np2_map_index_t *ix, uint32_t *k, uint32_t *w, uint64_t *n_seqs, uint64_t *n_minimizers, float *build_ms);
int np2_map_index_seq(const np2_map_index_t *ix, uint64_t i, const char **name /* the handle's */, uint64_t *len);
/* Reads as a separator stream of n_reads sequences -> hits[n_reads].  With chain and chain_off (both or neither):
 * chain_off[n_reads + 1] (the caller's) and *chain (np2_free), the primary chains' anchors as (r, q) pairs of uint32 on the
 * chain's strand, first to last: read i's are pairs chain_off[i] .. chain_off[i + 1]. */
int np2_map_bytes(const np2_map_index_t *ix, const uint8_t *reads, uint64_t n, uint64_t n_reads, const np2_map_opts_t *opts,
                  np2_map_hit_t *hits, uint32_t **chain, uint64_t *chain_off);
/* read files (FASTA / FASTQ, plain or gzip, through the read binner's reader threads) -> the PAF file out_path; a path ending
 * in .gz or .bgz is written as BGZF, compressed on the index's device.  stats may be NULL. */
int np2_map_files(const np2_map_index_t *ix, const char *const *paths, int n_paths, const np2_map_opts_t *opts, const char *out_path,
                  np2_map_stats_t *stats);
/* host only, no device: the same rule from the same arithmetic (csrc/np2_map_core.hpp), one read at a time */
int np2_map_host(const uint8_t *asm_stream, uint64_t n_asm, const uint8_t *reads, uint64_t n, uint64_t n_reads, const np2_map_opts_t *opts,
                 np2_map_hit_t *hits, uint32_t **chain, uint64_t *chain_off);
/* the counts and stage times of the last np2_map_bytes / np2_map_files / np2_map_host call on this thread */
int np2_map_last_stats(np2_map_stats_t *stats);
/* Weights (the rule: above).  A weight set lives in host memory only.  From canonical indices in any order, duplicates allowed
 * (an index beyond 4^k - 1 or a non-canonical one is NP2_E_ARG; n == 0 is the empty set whatever k says), or from a list file.
 * info: k (0 for the empty set) and the number of distinct listed k-mers; either output may be NULL. */
typedef struct np2_map_weights np2_map_weights_t;
int np2_map_weights_from_indices(uint32_t k, const uint32_t *index, uint64_t n, np2_map_weights_t **out);
int np2_map_weights_from_file(const char *path, np2_map_weights_t **out);
int np2_map_weights_info(const np2_map_weights_t *w, uint32_t *k, uint64_t *n_listed);
void np2_map_weights_free(np2_map_weights_t *w);
/* np2_map_index_bytes / np2_map_index_files under weights: w NULL or empty makes them their plain twins.  The index keeps a
 * bitmap of 4^k bits on the device (128 MiB at k = 15) and every door that takes the index (np2_map_bytes, np2_map_files,
 * np2_map_align_*, np2_sam_from_reads*) sketches the reads under it; w may be freed right after the call. */
int np2_map_index_bytes_w(int device, const uint8_t *stream, uint64_t n, const char *names, const np2_map_opts_t *opts,
                          const np2_map_weights_t *w, np2_map_index_t **out);
int np2_map_index_files_w(int device, const char *const *paths, int n_paths, const np2_map_opts_t *opts, const np2_map_weights_t *w,
                          np2_map_index_t **out);
/* the weights an index was built with: 0, 0 for an unweighted one; either output may be NULL */
int np2_map_index_weights(const np2_map_index_t *ix, uint32_t *k, uint64_t *n_listed);
/* np2_map_host under weights (host only, no device) */
int np2_map_host_w(const uint8_t *asm_stream, uint64_t n_asm, const uint8_t *reads, uint64_t n, uint64_t n_reads, const np2_map_opts_t *opts,
                   const np2_map_weights_t *w, np2_map_hit_t *hits, uint32_t **chain, uint64_t *chain_off);

/* ---- More chains: supplementary and secondary chains of a read, to PAF (what `minimap2 --secondary=yes -N` and its
 * supplementary lines report; the polisher's -s and -S doors read such records) ------------------------------------------------
 * THE RULE IS DEFINED HERE, on minimap2's published chain selection (mm_chain_backtrack, mm_set_parent, mm_select_sub).  No
 * minimap2 binary was at hand: equality with its output is not claimed and not tested.  No floating point is used.
 *   Options (np2_map_multi_opts_t; defaults in brackets): max_chains 1 .. 16 [1] selections per read, the primary among them (1
 *     is the mapper above: no further kernel is launched); supplementary 0 / 1 [0] report supplementary chains; secondary_n
 *     0 .. 15 [0] secondaries kept per parent; mask_pm 1 .. 1000 [500] the overlap threshold and pri_pm 0 .. 1000 [800] the
 *     secondary-to-parent score ratio, both per mille.  Anything else is NP2_E_ARG, before the first device call.
 *   Selection.  f, p, the primary chain, its marks, base[] and the primary's hit are exactly those of the chain rule above.  Then
 *     up to max_chains - 1 further selections.  In each, over the unmarked anchors, score(i) = f[i] - base[i], base as the sweep
 *     above defines it against the current marks; the largest score is taken and, of equal scores, the smallest i; a score
 *     below min_score ends the selections (so does a read with no unmarked anchor, or an unmapped primary).  The chain runs from
 *     i back through p while anchors are unmarked; its anchors are marked and base is swept again.  A chain with fewer than
 *     min_cnt anchors is dropped, but it stays marked and has used up a selection.  f is not monotone along p (f[i] only has to
 *     exceed k), so scores need not fall from one selection to the next: the rule is this procedure.  The first further
 *     selection's score is the primary's s2 whenever s2 >= min_score.
 *   Hit of a further chain.  As the primary's, from the chain's own anchors: interval, rev, tid, matches (k plus min(k, dr, dq)
 *     per later anchor), block and n; s1 is its score.
 *   Classes, in selection order over the chains that were not dropped; the primary is the first parent.  On forward read
 *     coordinates [qs, qe), with ov the overlap of c and P: c is SECONDARY to the first earlier parent P with ov * 1000 >
 *     mask_pm * min(len_c, len_P) (strict); with no such P it is a parent itself and SUPPLEMENTARY.  A secondary is kept when
 *     s1_c * 1000 >= pri_pm * s1_P, P has fewer than secondary_n kept secondaries, and P itself is reported; a supplementary is
 *     kept (reported) only with supplementary = 1, but is a parent either way.  A chain that is classed but not kept still
 *     counts toward its parent's s2.
 *   mapq.  The primary keeps its s2 and mapq in every bit.  A supplementary has s2 = the largest s1 among the chains classed
 *     secondary to it (0 if none) and mapq = the formula above on (s1, s2, n).  A secondary has s2 = 0 and mapq 0.
 *   Units.  A read's units are its primary (mapped or not: unit 0 is the hit of the plain doors) and its kept further chains in
 *     selection order: cls 0 primary, 1 supplementary, 2 secondary; parent is the read-local unit a secondary belongs to, and a
 *     parent's own place otherwise.
 *   PAF.  A read's lines are the primary's first, byte for byte the plain line, then the kept others in selection order, with
 *     tp:A:P for a supplementary and tp:A:S for a secondary.
 *   Alignment (np2_map_align_*_m).  The aligner's rule (below) is unchanged and runs once per unit: a read together with one
 *     kept chain, aligned with that chain's hit and that chain's exported anchors (the job's optional unit_read indirection,
 *     csrc/np2_align.hpp; null is the plain doors' read-indexed job).  Then a read's units are settled: if its primary is
 *     unmapped or overflows max_cells the read is written as the plain doors write it and its other units are dropped; a
 *     further unit that overflows is dropped, and so is a secondary whose parent was dropped; parents are renumbered.  Every
 *     further unit dropped here is counted in overflow_units.
 *   SAM.  A read's records are adjacent: the primary, then the kept others in selection order.  FLAG gets | 2048 for a
 *     supplementary and | 256 for a secondary record.  Clips are always soft and every record carries the full SEQ and, with
 *     NP2_ALN_QUAL, the full QUAL: what `minimap2 -Y --secondary-seq` writes.  NP2_ALN_MD, _CS and _EQX apply to every record
 *     through the one tag walk.  When a read has two or more aligned parent-class records (primary, supplementary), each of
 *     them gets SA:Z: as its last field, after cs:Z:, with rname,pos1,+|-,CIGAR,mapq,NM; for each other parent-class record,
 *     the primary first, then selection order; that CIGAR is in M / I / D / S form even under NP2_ALN_EQX.  With max_chains = 1
 *     the text is np2_map_align_files_x's bytes.
 *   Not built: hard clips and SEQ * for supplementary and secondary records; units through np2_sam_from_reads* / k_alnpack (cli
 *     --from_reads keeps refusing multi-chain mapping) and the polisher's -S through the SAM door (it reads secondaries from a
 *     BAM: samsort --full writes one).  The scratch of a group of reads is (max_chains - 1) slots of 64 bytes a read.
 * Stats: np2_map_last_multi_stats, this thread's last _m call; more_ms is the HIP-event time of the selection kernel, its scan
 * and the units' packing (0 from the host twins and with max_chains = 1). */
typedef struct np2_map_multi_opts {
    uint32_t max_chains, supplementary, secondary_n, mask_pm, pri_pm;
} np2_map_multi_opts_t;
typedef struct np2_map_multi_stats {
    uint64_t units;                  /* all units, the primaries (mapped or not) among them */
    uint64_t selections;             /* further selections that took a chain */
    uint64_t dropped_min_cnt;        /* ... dropped with fewer than min_cnt anchors */
    uint64_t dropped_secondary;      /* ... classed secondary and not kept (pri_pm, secondary_n, or a parent that is not reported) */
    uint64_t kept_supplementary, kept_secondary;
    uint64_t overflow_units;         /* np2_map_align_*_m: further units dropped when the read's units were settled */
    float more_ms;
} np2_map_multi_stats_t;
/* np2_map_bytes per unit.  unit_off[n_reads + 1] is the caller's: read i's units are unit_off[i] .. unit_off[i + 1], one at
 * the least.  *hits, *cls, *parent (np2_free) have unit_off[n_reads] entries.  With chain and chain_off (both or neither):
 * *chain_off (np2_free) has one entry more than there are units, *chain the units' anchors as np2_map_bytes gives the
 * primaries'.  With max_chains = 1 the arrays are np2_map_bytes' and no further kernel is launched. */
int np2_map_bytes_m(const np2_map_index_t *ix, const uint8_t *reads, uint64_t n, uint64_t n_reads, const np2_map_opts_t *opts,
                    const np2_map_multi_opts_t *multi, uint64_t *unit_off, np2_map_hit_t **hits, uint8_t **cls, uint32_t **parent,
                    uint32_t **chain, uint64_t **chain_off);
/* np2_map_files with the further chains' lines */
int np2_map_files_m(const np2_map_index_t *ix, const char *const *paths, int n_paths, const np2_map_opts_t *opts,
                    const np2_map_multi_opts_t *multi, const char *out_path, np2_map_stats_t *stats);
/* host only, no device: np2_map_host_w per unit (w NULL or empty: unweighted) */
int np2_map_host_m(const uint8_t *asm_stream, uint64_t n_asm, const uint8_t *reads, uint64_t n, uint64_t n_reads, const np2_map_opts_t *opts,
                   const np2_map_multi_opts_t *multi, const np2_map_weights_t *w, uint64_t *unit_off, np2_map_hit_t **hits, uint8_t **cls,
                   uint32_t **parent, uint32_t **chain, uint64_t **chain_off);
int np2_map_last_multi_stats(np2_map_multi_stats_t *stats);
/* (the units aligned: np2_map_align_*_m, behind np2_map_align_last_tag_stats below) */

/* ---- the primary chain as a base-level alignment: chains to SAM (the recipe's `winnowmap -ax` / `minimap2 -a`, whose SAM the
 * polisher reads) ----------------------------------------------------------------------------------------------------------------
 * THE RULE IS DEFINED HERE, in the manner of minimap2's alignment between chained anchors with one affine piece (-A1 -B4 -O6
 * -E2).  No minimap2 binary was at hand: equality with its CIGARs is not claimed and not tested.  The fine points (tie orders,
 * the matrix' coordinates, the limits' reasons) stand beside the arithmetic in csrc/np2_align_core.hpp.
 *   Options (np2_align_opts_t; defaults in brackets): match [1], mismatch [4], gap_open [6], gap_ext [2], band [32], end_bonus
 *     [5], ext_max [2048], max_cells [2^23].  A gap of length g costs gap_open + g * gap_ext.  match 1 .. 15, mismatch <= 31,
 *     gap_open <= 255, gap_ext 1 .. 15, band <= 1023, end_bonus <= 2^16, ext_max 1 .. 2^20, max_cells 1 .. 2^24; anything else
 *     is NP2_E_ARG.
 *   Bases.  Two bytes match if and only if both are ACGT in either case and the same base; N matches nothing.  A reverse-strand
 *     read is aligned as its reverse complement; positions are on that strand, as the chain's q are.
 *   Pins.  Walking the primary chain first to last, the first anchor is a pin; a later anchor is a pin if and only if its k-mer
 *     starts at or after the previous pin's end in both r and q (r - k + 1 > r_prev and q - k + 1 > q_prev).  A pin is k match
 *     columns.
 *   Segments.  The bases between two consecutive pins, tl >= 0 of the reference and ql >= 0 of the read.  tl == ql and every
 *     pair matching: all match columns ("equal").  Otherwise the longest matching common prefix, then the longest matching
 *     common suffix of what remains, are match columns and what is left is the core: an empty side is one gap ("pure gap"), 1 x 1
 *     is one mismatch ("snv"), anything else is a global affine alignment (Gotoh's H, E, F) inside the band of diagonals
 *     min(0, d) - band .. max(0, d) + band, d = tl - ql of the core; the optimum inside the band is the answer.  Traceback
 *     prefers the diagonal, then the deletion, then the insertion, and continues an open gap rather than opening another.
 *     A core whose (ql + 1) * band width exceeds max_cells, or whose band is wider than 2048 diagonals, makes the read unaligned:
 *     flag 4, counted in overflow.  (Defaults: max_gap 10000, bandwidth 500, band 32 give at most 10001 * 565 = 5.65 M cells.)
 *   Ends.  The head (the read before the first pin, aligned backwards) and the tail (after the last pin) use the same
 *     recurrence from the pin outwards with the reference end free, in the band -band .. +band.  n = min(remainder, ext_max,
 *     reference left + band) read bases and min(reference left, n + band) reference bases are considered.  The extension ends
 *     at the read-end cell (the best cell of the last row, the smallest column of equal ones; it exists only when n is the
 *     whole remainder) when its score + end_bonus >= the best cell's score, otherwise at the best cell (the largest score; of
 *     equal cells the smallest row, then the smallest column).  Everything beyond the chosen cell is soft-clipped.  An insertion
 *     next to a clip becomes part of it, a deletion next to a clip is dropped.
 *   CIGAR.  Words len << 4 | op with M = 0, I = 1, D = 2, S = 4 only; adjacent equal ops are merged.  Then every gap, left to
 *     right, is left-aligned: it moves one column left while the column before it is a match column whose base equals the
 *     gap's last base; it stops at a mismatch column, at another gap, or when one M column would be left at the start.  Pins do
 *     not stop it.  Gaps of one kind that meet are merged and move on as one.
 *   Record (np2_align_rec_t).  tid and mapq from the hit; pos the first M column's reference position (0-based), end one past
 *     the last; flag 0, 16 or 4; NM = mismatches + gap bases; AS = the final columns' score under the options (pins and trimmed
 *     matches count as matches).  An unmapped or overflowed read has tid -1, flag 4 and no CIGAR.
 *   SAM.  @HD VN:1.6 SO:unsorted, one @SQ SN: LN: per sequence in index order, one @PG; then one line per read in read order:
 *     qname flag rname pos+1 mapq CIGAR * 0 0 SEQ * NM:i: AS:i: cm:i: s1:i: s2:i: (SEQ reverse-complemented with flag 16: ACGT
 *     in their case, any other byte kept), or qname 4 * 0 0 * * 0 0 SEQ * for an unmapped or overflowed read.  QUAL is * unless
 *     NP2_ALN_QUAL asks for it (Tags, below).
 *   Not built: the second affine piece (-O26 -E1); z-drop; direct BAM output (supplementary and secondary records:
 *     np2_map_align_*_m, "More chains" above).  (The records reach the
 *     polisher without SAM text through np2_sam_from_reads, below.)
 * The index keeps the assembly's bytes on the device for this (one byte per assembly base more than the minimizers).  Traceback
 * bits take one byte per matrix cell in a device buffer budgeted per group of whole reads (2^30 bytes; test hook
 * NP2_ALIGN_TEST_BUDGET, bytes); NP2_ALIGN_TEST_CELLS lowers max_cells.  Both are read once per call.  np2_map_stats_t.groups
 * counts these groups when aligning. */
typedef struct np2_align_opts {
    uint32_t match, mismatch, gap_open, gap_ext, band, end_bonus, ext_max, max_cells;
} np2_align_opts_t;
typedef struct np2_align_rec {
    int32_t tid;                     /* -1: unmapped or overflowed (flag 4) */
    uint32_t flag, pos, end, mapq, n_cigar, nm;
    int32_t as;
} np2_align_rec_t;
typedef struct np2_align_stats {
    uint64_t pins, segments, equal, pure_gap, snv, cores;
    uint64_t cells;                  /* matrix cells within the limits, cores and end extensions */
    uint64_t clipped_bases, overflow;
    float pins_ms, classify_ms, dp_ms, assemble_ms; /* HIP events, summed over groups; 0 from np2_map_align_host */
    float write_ms;                  /* np2_map_align_files: formatting and writing the SAM */
} np2_align_stats_t;
/* np2_map_bytes and the alignment: recs[n_reads]; with cigar and cigar_off (both or neither): cigar_off[n_reads + 1] (the
 * caller's) and *cigar (np2_free), read i's words cigar_off[i] .. cigar_off[i + 1].  hits may be NULL. */
int np2_map_align_bytes(const np2_map_index_t *ix, const uint8_t *reads, uint64_t n, uint64_t n_reads, const np2_map_opts_t *map_opts,
                        const np2_align_opts_t *align_opts, np2_map_hit_t *hits, np2_align_rec_t *recs, uint32_t **cigar, uint64_t *cigar_off);
/* read files -> the SAM file out_path (a path ending in .gz or .bgz: BGZF).  stats (the mapper's) may be NULL. */
int np2_map_align_files(const np2_map_index_t *ix, const char *const *paths, int n_paths, const np2_map_opts_t *map_opts,
                        const np2_align_opts_t *align_opts, const char *out_path, np2_map_stats_t *stats);
/* host only, no device: the same rule from the same arithmetic (csrc/np2_align_core.hpp) */
int np2_map_align_host(const uint8_t *asm_stream, uint64_t n_asm, const uint8_t *reads, uint64_t n, uint64_t n_reads,
                       const np2_map_opts_t *map_opts, const np2_align_opts_t *align_opts, np2_map_hit_t *hits, np2_align_rec_t *recs,
                       uint32_t **cigar, uint64_t *cigar_off);
/* np2_map_align_host under weights (np2_map_weights_t, above); w NULL or empty: np2_map_align_host */
int np2_map_align_host_w(const uint8_t *asm_stream, uint64_t n_asm, const uint8_t *reads, uint64_t n, uint64_t n_reads,
                         const np2_map_opts_t *map_opts, const np2_align_opts_t *align_opts, const np2_map_weights_t *w, np2_map_hit_t *hits,
                         np2_align_rec_t *recs, uint32_t **cigar, uint64_t *cigar_off);
/* the alignment counts and stage times of the last np2_map_align_* call on this thread */
int np2_map_align_last_stats(np2_align_stats_t *stats);
/* Caller-built chains: the aligner alone, on the caller's hits and chains (as np2_align_tags_device runs the tag walk on the
 * caller's records).  Nothing is sketched, seeded or chained.  np2_align_chains_device runs the kernels np2_map_align_bytes
 * runs behind its chaining, as one group, against the index's assembly; np2_align_chains_host runs the host aligner against
 * asm_stream.  reads: a separator stream of n_reads reads; hits[n_reads] as the mapping doors return them (of a hit the aligner
 * reads tid, rev, qlen, n and mapq; tid < 0: an unmapped read, flag 4); chain_off[n_reads + 1] and chain: read i's (r, q)
 * pairs are chain_off[i] .. chain_off[i + 1], hits[i].n of them (none for an unmapped read).  recs, cigar and cigar_off as from
 * np2_map_align_bytes; np2_map_align_last_stats has the counts (np2_map_last_stats: reads, mapped, unmapped and, from the
 * device, groups).
 *   Checked on the host before anything is uploaded, a violation being NP2_E_ARG with a message that names the read (and the
 *   anchor): k is the index's (the host door: 11 .. 28); chain_off[0] is 0, chain_off ascends and chain_off[i + 1] -
 *   chain_off[i] is hits[i].n for a mapped read and 0 for an unmapped one; for a mapped read tid names a contig, qlen is the
 *   read's length, rev is 0 or 1 and n >= 1; for every anchor k - 1 <= r < the contig's length and k - 1 <= q < qlen.  Order
 *   among the anchors is not checked: the pin rule ignores an anchor that is not k beyond the last pin on both axes.
 *   probe (NULL: none), for tests: what the matrices held.  want is the caller's: NP2_PROBE_SLOTS asks for slot_off[n_reads +
 *   1], slots and res (read i's slots slot_off[i] .. slot_off[i + 1]: head, segments, tail; none for an unmapped read; res of
 *   a slot without a matrix is all zero); NP2_PROBE_TB for tb_off[n_slots + 1] and tb, one byte of traceback bits per cell of
 *   every matrix, rows of W bytes (bits 0-1: H's source, 0 diagonal, 1 E, 2 F; bit 2: E continues a gap; bit 3: F continues a
 *   gap; a slot outside the matrix: 0).  The arrays are np2_free-owned.  A read over the limits keeps its slots, and those of
 *   its matrices that are within the limits are computed.  On the device the traceback buffer is reused per sub-group
 *   (NP2_ALIGN_TEST_BUDGET), so its bytes are copied out per sub-group and appended. */
typedef struct np2_align_slot {
    uint32_t t0, q0, tl, ql, pre, suf, kind, W; /* kind: 0 equal, 1 pure gap, 2 snv, 3 core, 4 head, 5 tail, 6 nothing */
    int32_t lo;                      /* the band: diagonals lo .. lo + W - 1 */
    uint32_t over;
} np2_align_slot_t;
typedef struct np2_align_res {
    int32_t score;
    uint32_t ei, ej;                 /* the cell the walk starts from */
} np2_align_res_t;
#define NP2_PROBE_SLOTS 1u
#define NP2_PROBE_TB 2u
typedef struct np2_align_probe {
    uint32_t want;                   /* in: a sum of NP2_PROBE_* */
    uint32_t pad;
    uint64_t n_slots;
    uint64_t *slot_off;
    np2_align_slot_t *slots;
    np2_align_res_t *res;
    uint64_t *tb_off;
    uint8_t *tb;
} np2_align_probe_t;
int np2_align_chains_device(const np2_map_index_t *ix, const uint8_t *reads, uint64_t n, uint64_t n_reads, uint32_t k,
                            const np2_map_hit_t *hits, const uint32_t *chain, const uint64_t *chain_off, const np2_align_opts_t *align_opts,
                            np2_align_rec_t *recs, uint32_t **cigar, uint64_t *cigar_off, np2_align_probe_t *probe);
int np2_align_chains_host(const uint8_t *asm_stream, uint64_t n_asm, const uint8_t *reads, uint64_t n, uint64_t n_reads, uint32_t k,
                          const np2_map_hit_t *hits, const uint32_t *chain, const uint64_t *chain_off, const np2_align_opts_t *align_opts,
                          np2_align_rec_t *recs, uint32_t **cigar, uint64_t *cigar_off, np2_align_probe_t *probe);

/* ---- Tags: base qualities, MD, cs and = / X, the aligner's opt-in outputs (what a variant caller or a genome browser reads from
 * the BAM that samsort --full makes of the mapper's SAM) ------------------------------------------------------------------------
 * THE RULE IS DEFINED HERE, on the SAM specification (SAMv1 section 1.4, SAMtags MD) and minimap2's documented short cs form;
 * no minimap2 / samtools binary at hand, equality not claimed.  Its arithmetic: csrc/np2_aligntags_core.hpp, shared by the
 * kernels (csrc/np2_aligntags.hip: k_align_tags_size, scans, k_align_tags_emit, one wavefront per read, launched per sub-group
 * right behind k_align_ops_emit and only when a flag asks), the host twin and a stand-alone program.  Each output is off by
 * default (out_flags, a sum of NP2_ALN_*); with none every entry point launches what it launched before and writes the same
 * bytes.
 *   The walk is over a read's final CIGAR, after left-alignment and clip handling, from rec.pos.  t: the assembly's bytes from
 *     pos on.  q: the read as aligned, its reverse complement for flag 16 (ACGT complemented in their case, any other byte
 *     kept); index 0 is the first CIGAR column, soft clips included.  A column of an M word is a match if and only if both bytes
 *     are ACGT in either case and the same base (N matches nothing): the predicate NM and AS are computed with, so NM = X
 *     columns + I bases + D bases.
 *   NP2_ALN_EQX.  Every M word is replaced, in place and in order, by the maximal runs of match columns (=, op 7) and mismatch
 *     columns (X, op 8) inside it; other words are untouched, lengths are preserved.  n_cigar and cigar_off describe the split
 *     CIGAR; pos, end, nm and as are unchanged.
 *   NP2_ALN_MD.  A counter c = 0.  M columns: a match does ++c; a mismatch emits dec(c), L(t), then c = 0.  A D word: dec(c),
 *     '^', L(t) for each deleted base, then c = 0.  I and S words: nothing (the counter runs on across an insertion).  At the
 *     end: dec(c).  L(t): A-Z kept, a-z upper-cased, any other byte N.  (A mismatch right after a deletion reads ^AC0T.)
 *   NP2_ALN_CS, the short form.  A maximal run of match columns inside one M word: ':' dec(length).  A mismatch: '*' l(t) l(q).
 *     An I word: '+', then l(q) per base.  A D word: '-', then l(t) per base.  S: nothing.  l: letters lower-cased, any other
 *     byte n.
 *   NP2_ALN_QUAL.  A read has qualities when its file is FASTQ, or when the caller's quality stream gives them (quals: the
 *     shape of reads, a newline where reads has one; a read whose first quality byte is 0xFF has none).  SAM QUAL is then the
 *     read's quality bytes, reversed (not complemented) with flag 16; a read without qualities keeps *.  A quality line whose
 *     length differs from its sequence's, or that holds a byte outside '!' .. '~', is NP2_E_ARG naming the file and the 1-based
 *     record; without the flag the quality lines stay unread.  An unmapped or overflowed read (flag 4) has no MD / cs and an
 *     empty CIGAR; its qualities are written forward.  Qualities stay on the host: the text SAM needs them nowhere else.
 *   SAM line.  The fields above in their order; QUAL takes the place of *, the CIGAR may hold = and X; MD:Z: then cs:Z: follow
 *     s2:i:.  A line without flags is the line above byte for byte, and the header is the same.
 *   Doors.  np2_map_align_bytes_x, _files_x, _host_x: the calls above with out_flags; md / md_off and cs / cs_off (each pair
 *     both or neither, required by its flag): *md, *cs (np2_free) and md_off[n_reads + 1], cs_off[n_reads + 1], read i's text
 *     md[md_off[i] .. md_off[i + 1]) (empty for flag 4).  np2_align_tags_device, _host run the walk on the caller's records:
 *     record i's reference columns begin at ref + t_off[i], its read, already oriented, at reads + q_off[i] (first column,
 *     clips included), its words are cigar[cigar_off[i] .. cigar_off[i + 1]) (M, I, D, S only; none: no text at all); outputs
 *     as above plus *eqx (np2_free) and eqx_off[n_recs + 1].  A record whose columns reach beyond either buffer is NP2_E_ARG;
 *     2^30 columns or more in a record, 2^32 in a call: NP2_E_UNSUPPORTED.  Unknown flag bits are NP2_E_ARG (NP2_ALN_QUAL is
 *     unknown to _host_x and the two tag doors); every argument is checked before the first device call.
 *   Stats (np2_map_align_last_tag_stats; this thread's last _x or tag call): bytes and words written, reads that had
 *     qualities, and tags_ms, the HIP-event time of the two kernels, their scans and the copies of their outputs to the host
 *     (0 without a flag and from the host doors).  np2_align_stats_t keeps its layout.
 *   Not built: the long cs form; MD / cs in PAF; qualities or tags through np2_sam_from_reads* (the lean handle has no place for
 *     them; a full BAM from reads goes through the SAM text); the second affine piece, z-drop, secondary or supplementary
 *     records; a CG tag. */
#define NP2_ALN_QUAL 1u
#define NP2_ALN_MD 2u
#define NP2_ALN_CS 4u
#define NP2_ALN_EQX 8u
typedef struct np2_align_tag_stats {
    uint64_t md_bytes, cs_bytes, eqx_words, qual_reads;
    float tags_ms;
} np2_align_tag_stats_t;
int np2_map_align_bytes_x(const np2_map_index_t *ix, const uint8_t *reads, const uint8_t *quals /* NULL: none */, uint64_t n, uint64_t n_reads,
                          const np2_map_opts_t *map_opts, const np2_align_opts_t *align_opts, uint32_t out_flags, np2_map_hit_t *hits,
                          np2_align_rec_t *recs, uint32_t **cigar, uint64_t *cigar_off, char **md, uint64_t *md_off, char **cs, uint64_t *cs_off);
int np2_map_align_files_x(const np2_map_index_t *ix, const char *const *paths, int n_paths, const np2_map_opts_t *map_opts,
                          const np2_align_opts_t *align_opts, uint32_t out_flags, const char *out_path, np2_map_stats_t *stats);
/* host only, no device: the same rule text */
int np2_map_align_host_x(const uint8_t *asm_stream, uint64_t n_asm, const uint8_t *reads, uint64_t n, uint64_t n_reads,
                         const np2_map_opts_t *map_opts, const np2_align_opts_t *align_opts, const np2_map_weights_t *w /* NULL ok */,
                         uint32_t out_flags, np2_map_hit_t *hits, np2_align_rec_t *recs, uint32_t **cigar, uint64_t *cigar_off, char **md,
                         uint64_t *md_off, char **cs, uint64_t *cs_off);
int np2_align_tags_device(int device, const uint8_t *ref, uint64_t n_ref, const uint8_t *reads, uint64_t n_read_bytes, uint64_t n_recs,
                          const uint64_t *t_off, const uint64_t *q_off, const uint32_t *cigar, const uint64_t *cigar_off, uint32_t out_flags, char **md,
                          uint64_t *md_off, char **cs, uint64_t *cs_off, uint32_t **eqx, uint64_t *eqx_off);
int np2_align_tags_host(const uint8_t *ref, uint64_t n_ref, const uint8_t *reads, uint64_t n_read_bytes, uint64_t n_recs, const uint64_t *t_off,
                        const uint64_t *q_off, const uint32_t *cigar, const uint64_t *cigar_off, uint32_t out_flags, char **md, uint64_t *md_off,
                        char **cs, uint64_t *cs_off, uint32_t **eqx, uint64_t *eqx_off);
int np2_map_align_last_tag_stats(np2_align_tag_stats_t *stats);

/* ---- More chains, aligned ---- */
/* The units aligned (the rule: "More chains", Alignment and SAM).  Every pointer is np2_free-owned, one entry per unit unless it
 * says otherwise; md / md_off and cs / cs_off are NULL unless out_flags asks for them (np2_map_align_bytes_x's flags). */
typedef struct np2_map_units {
    uint64_t n_units;
    np2_map_hit_t *hits;
    uint8_t *cls;
    uint32_t *parent;
    np2_align_rec_t *recs;           /* flag holds 16 only: a writer adds 2048 / 256 from cls */
    uint32_t *cigar;
    uint64_t *cigar_off;             /* [n_units + 1] */
    char *md;
    uint64_t *md_off;                /* [n_units + 1] */
    char *cs;
    uint64_t *cs_off;                /* [n_units + 1] */
} np2_map_units_t;
/* np2_map_align_bytes_x per unit; unit_off[n_reads + 1] is the caller's, *out is filled (zeroed first) */
int np2_map_align_bytes_m(const np2_map_index_t *ix, const uint8_t *reads, const uint8_t *quals /* NULL: none */, uint64_t n, uint64_t n_reads,
                          const np2_map_opts_t *map_opts, const np2_map_multi_opts_t *multi, const np2_align_opts_t *align_opts,
                          uint32_t out_flags, uint64_t *unit_off, np2_map_units_t *out);
/* np2_map_align_files_x with the further units' records */
int np2_map_align_files_m(const np2_map_index_t *ix, const char *const *paths, int n_paths, const np2_map_opts_t *map_opts,
                          const np2_map_multi_opts_t *multi, const np2_align_opts_t *align_opts, uint32_t out_flags, const char *out_path,
                          np2_map_stats_t *stats);
/* host only, no device: np2_map_align_host_x per unit (NP2_ALN_QUAL is not taken: there is no text to write) */
int np2_map_align_host_m(const uint8_t *asm_stream, uint64_t n_asm, const uint8_t *reads, uint64_t n, uint64_t n_reads,
                         const np2_map_opts_t *map_opts, const np2_map_multi_opts_t *multi, const np2_align_opts_t *align_opts,
                         const np2_map_weights_t *w /* NULL ok */, uint32_t out_flags, uint64_t *unit_off, np2_map_units_t *out);

/* ---- the mapper's SAM, parsed and coordinate-sorted on the device (the reference's recipe: `| samtools sort -o ... ;
 * samtools index ...`, which exist only so that an indexed reader can fetch one contig's records in coordinate order) -------
 * THE RULE IS DEFINED HERE, on the SAM specification section 1.4 and on what samtools' coordinate comparison is understood to
 * do; it is not pinned against the samtools binary.
 *   Input: one or more files, plain or gzip (or BAM: "BAM input", below), or a stream that cannot be read twice (path "-":
 *     standard input).  The bytes
 *     are taken as they stand, in pieces that end at a line boundary (32 MiB; test hook NP2_SAM_TEST_PIECE, in bytes, read
 *     once per call).  A line that does not fit an empty piece is NP2_E_UNSUPPORTED, naming the 1-based line.  A '\r' directly
 *     before '\n' is dropped, a last line needs no newline, empty lines are skipped.
 *   Header: the lines beginning with '@' before the first alignment line.  @SQ lines give the references in order (SN:, LN:);
 *     other header lines are ignored.  NP2_E_ARG: an '@' line after the first alignment line, an @SQ line without SN or LN, a
 *     duplicate SN, files that do not carry the same @SQ list.  The host reads the header.
 *   Alignment line: at least 11 tab-separated fields (fewer: NP2_E_ARG naming the 1-based line).  Only FLAG, RNAME, POS, MAPQ,
 *     CIGAR and SEQ are read.  FLAG decimal 0..65535; POS decimal 0..2^31-1, pos = POS - 1; MAPQ decimal 0..255; a non-digit
 *     or an overflow in any of them is NP2_E_ARG.  RNAME "*" is tid -1, any other name must be an @SQ name (else NP2_E_ARG).
 *     CIGAR "*" is n_cigar = 0, otherwise one or more of <decimal length below 2^28><one of MIDNSHP=X> (anything else:
 *     NP2_E_ARG), the word len << 4 | op.  SEQ "*" is l_seq = 0, otherwise every byte maps through BAM's "=ACMGRSVTWYHKDBN"
 *     in either case and any other byte to 15; packed 4 bits a base, high nibble first, every record starting at a byte
 *     (np2_bamrec_t.seq_off).  QNAME, RNEXT, PNEXT, TLEN, QUAL and the optional fields are skipped and not validated.
 *   Kept and dropped: a record with tid == -1 or flag & 0x4 is counted in stats.unmapped and not kept.
 *   Order: the kept records ascending by (tid, pos + 1, s), s = (flag >> 4) & 1 with tie_by_strand (the samtools order) and 0
 *     without.  Records equal in that key keep input order: file order, files in argument order.  The reference numbers reads
 *     in file order (main.rs:1813), so this order is part of the result: with tie_by_strand = 0 a BAM whose ties are in input
 *     order gives the same polish through either door.
 *   Errors: the first offending line in input order speaks; the process stays usable.  Device memory that does not suffice
 *     for the packed SEQ, the CIGAR words and the records (about half a byte per base and 40 bytes per record, twice the
 *     records and words while they are sorted) is NP2_E_NOMEM, and the message says how much was needed.
 * Messages: np2_io_last_error() on the calling thread (np2_contig_from_sam: also np2_last_error(ctx)). */
typedef struct np2_sam_opts {
    uint32_t tie_by_strand; /* 1 */
} np2_sam_opts_t;
typedef struct np2_sam_stats {
    uint64_t lines;       /* lines read, header and empty ones included */
    uint64_t records;     /* alignment lines */
    uint64_t unmapped;    /* of them: tid == -1 or flag & 0x4 */
    uint64_t kept;        /* records - unmapped */
    uint64_t cigar_words; /* of the kept records */
    uint64_t seq_bytes;   /* packed SEQ of the kept records */
    float parse_ms;       /* k_sam_lines, k_sam_fields and the scans (HIP events, summed over the pieces) */
    float pack_ms;        /* k_sam_pack */
    float sort_ms;        /* the key sort and k_sam_gather */
    float read_ms;        /* wall time the calling thread waited for its reader thread */
} np2_sam_stats_t;
typedef struct np2_sam np2_sam_t;
/* Reads everything and leaves the sorted records, their CIGAR words and the packed SEQ resident on ctx's device (the work
 * runs on ctx's stream).  opts == NULL: the defaults.  The arguments are checked and every file but "-" is opened once
 * before the first device call: a NULL argument or a file that cannot be opened is NP2_E_ARG.  The handle is read-only
 * afterwards: any number of threads may call np2_contig_from_sam on it, each with a context of its own on that device. */
int np2_sam_open(np2_ctx_t *ctx, const char *const *paths, int n_paths, const np2_sam_opts_t *opts, np2_sam_t **out);
void np2_sam_close(np2_sam_t *s);
int np2_sam_n_refs(np2_sam_t *s);
const char *np2_sam_ref_name(np2_sam_t *s, int tid, uint32_t *len);
int np2_sam_stats(np2_sam_t *s, np2_sam_stats_t *stats);
/* np2_contig_from_bam for a resident SAM: the host copies back the range of records and CIGAR words of reference `name`
 * (binary search on the sorted keys) and the front end reads the SEQ bytes where they are.  use_secondary is
 * NP2_E_UNSUPPORTED (a secondary record needs the SEQ of its read's primary record, found by name: use a BAM, which
 * np2_sam_write_bam below writes from this handle); a name the
 * @SQ lines lack, a NULL argument or a context of another device is NP2_E_ARG.  These are checked before the first device call. */
int np2_contig_from_sam(np2_ctx_t *ctx, np2_sam_t *sam, const char *name, const uint8_t *ref, uint32_t L,
                        const np2_front_opts_t *opts, np2_contig_t **out);
/* SAM text in host memory, header included -> the sorted records on the host, for parity tests and measurements: recs
 * (cigar_off in sorted order, seq_off as the records were met in the text), tids, cigar (n_recs entries / stats.cigar_words
 * words), seq4 (stats.seq_bytes bytes).  Release the four with np2_free; each is NULL when it would be empty.  stats may be
 * NULL. */
int np2_sam_parse_bytes(int device, const uint8_t *text, uint64_t n, const np2_sam_opts_t *opts, np2_bamrec_t **recs, int32_t **tids,
                        uint32_t **cigar, uint8_t **seq4, uint64_t *n_recs, np2_sam_stats_t *stats);
/* the same four arrays of a resident SAM copied back to the host (parity tests of np2_sam_open; np2_sam_stats has the sizes) */
int np2_sam_export(np2_ctx_t *ctx, np2_sam_t *sam, np2_bamrec_t **recs, int32_t **tids, uint32_t **cigar, uint8_t **seq4,
                   uint64_t *n_recs);

/* ---- the resident SAM straight from reads: the aligner's records stay on the device (one process, no SAM text) --------------
 * THE RULE IS ONE SENTENCE: the handle holds exactly what np2_sam_open (np2_sam_open_ex with NP2_SAM_KEEP_NAMES) would hold
 * after reading the SAM that np2_map_align_files writes for the same index, files, mapper options and aligner options: recs
 * (cigar_off in sorted order, seq_off in the order the reads were met), tids, cigar, seq4, with NP2_SAM_KEEP_NAMES names and
 * name_ref, refs and the sorted keys, array for array.  What follows from it, written out (the arithmetic:
 * csrc/np2_alnpack_core.hpp, which the kernels of csrc/np2_alnpack.hip and the host twin below both compile):
 *   Kept reads: a read whose record has tid >= 0 and flag & 4 == 0.  Unmapped and overflowed reads are counted in
 *     stats.unmapped and leave nothing behind.  stats.records is the number of reads, stats.lines that plus the header lines the
 *     text would have (@HD, one @SQ per sequence, @PG).
 *   Record words (np2_bamrec_t): pos, flag | mapq << 16, n_cigar, l_seq = the read's length; seq_off starts every record at a
 *     byte; the pad words are zero.
 *   Key: (tid, pos + 1, s) with s = (flag >> 4) & 1 under tie_by_strand and 0 without, as for the text; equal keys keep read
 *     order, files in argument order.  The sort and the gather are the text door's own.
 *   SEQ: the read's bytes as the SAM line prints them: with flag 16 reversed, ACGT complemented in their case and every other
 *     byte kept as it is.  Each byte maps through BAM's "=ACMGRSVTWYHKDBN" in either case, any other byte to 15; two bases a
 *     byte, high nibble first, the low nibble of an odd read's last byte 0.
 *   Names (NP2_SAM_KEEP_NAMES): the bytes `map -a` prints as QNAME (the header line up to the first white space; np2_sam_from_
 *     read_bytes: names, or the reads' numbers from 1).  A kept read whose name is empty or longer than 254 bytes is NP2_E_ARG,
 *     "QNAME is empty or longer than 254 bytes", naming the read.
 *   NP2_SAM_KEEP_ALL is NP2_E_UNSUPPORTED: the NM, AS, cm, s1 and s2 fields are not kept as binary tails.  The way round: write
 *     the text (`map -a -o map.sam.gz`), then `samsort --full`.  -S, several ranks and inputs beyond one device's memory are out
 *     of scope as for the SAM door.
 *   Errors: option errors are those of np2_map_align_*, checked first; then a NULL argument, unknown flag bits, an index on
 *     another device than the context, a sequence name the index holds twice (as a duplicate @SQ SN is in the text): NP2_E_ARG.
 *     All are checked, and every file is opened once, before the first device call.
 *   Memory: beside the index and the mapper's batch buffers, half a byte a base plus 40 bytes and the CIGAR words a record stay
 *     resident, the records and words twice over while they are sorted; a shortfall is NP2_E_NOMEM and says how much was needed.
 * The mapper works on a stream of its own; the pack kernels and the sort run on that stream too and the call returns once it
 * is drained, so the handle is ready for any context of the device.  Nothing per read comes back to the host beside the
 * mapper's hits: per sub-group of the aligner only the totals that size the arrays.  After a call np2_map_last_stats and
 * np2_map_align_last_stats report it on the calling thread; in np2_sam_stats_t parse_ms is 0, pack_ms the HIP-event time of
 * k_alnpack_sizes, its scans and k_alnpack, read_ms the wait for the read-file readers.  k_alnpack_sizes and its scans run
 * between the events that bracket assemble_ms in np2_align_stats_t; their time is taken out of assemble_ms again, so that for
 * this door assemble_ms is the ops' count, scan and emit as for np2_map_align_* (without their copies to the host) and pack_ms
 * alone carries the pack kernels.
 * Every reader of a handle works on this one unchanged: np2_contig_from_sam, np2_sam_export, np2_sam_stats, and with
 * NP2_SAM_KEEP_NAMES np2_sam_write_bam, np2_sam_bam_stream (lean) and np2_sam_export_names. */
int np2_sam_from_reads(np2_ctx_t *ctx, const np2_map_index_t *ix, const char *const *paths, int n_paths, const np2_map_opts_t *map_opts,
                       const np2_align_opts_t *align_opts, const np2_sam_opts_t *sam_opts, uint32_t flags, np2_sam_t **out);
/* reads in memory: the stream np2_map_align_bytes takes; names NULL (1, 2, ...) or '\n'-terminated */
int np2_sam_from_read_bytes(np2_ctx_t *ctx, const np2_map_index_t *ix, const uint8_t *reads, uint64_t n, uint64_t n_reads,
                            const char *names, const np2_map_opts_t *map_opts, const np2_align_opts_t *align_opts,
                            const np2_sam_opts_t *sam_opts, uint32_t flags, np2_sam_t **out);
/* host only, no device: aligner output (np2_map_align_bytes or np2_map_align_host: recs, cigar, cigar_off[n_reads + 1]) and the
 * read stream -> the four arrays as np2_sam_export returns them, from the same rule text as the kernel.  sam_opts may be NULL.
 * Release the four with np2_free; each is NULL when it would be empty. */
int np2_align_pack_host(const np2_align_rec_t *recs, const uint32_t *cigar, const uint64_t *cigar_off, const uint8_t *reads, uint64_t n,
                        uint64_t n_reads, const np2_sam_opts_t *sam_opts, np2_bamrec_t **out_recs, int32_t **tids, uint32_t **out_cigar,
                        uint8_t **seq4, uint64_t *n_recs);

/* ---- the sorted BAM and its .bai, written from a resident SAM (the reference's recipe: `samtools sort -o hifi.map.sort.bam -`
 * and `samtools index`) ---------------------------------------------------------------------------------------------------
 * THE RULE IS DEFINED HERE, on the SAM specification sections 4.2 (BAM) and 5.2 (BAI).  No samtools binary was at hand:
 * equality with the files of `samtools sort` / `samtools index` is not claimed.
 *   Names: np2_sam_open_ex with NP2_SAM_KEEP_NAMES keeps each kept record's QNAME, the bytes before the first tab as they
 *     stand.  An empty QNAME or one longer than 254 bytes is NP2_E_ARG naming the 1-based line (after every other error of
 *     its piece of text).  np2_bamrec_t stays as it is: per record, beside it and through the sort like the tids, travels
 *     name_ref = offset << 8 | length into the name bytes, which stay where they were met.  Without the flag np2_sam_open_ex
 *     is np2_sam_open and launches what that launches.
 *   Stream S: "BAM\1", l_text, text, n_ref, then per reference l_name, name with NUL, l_ref.  text is
 *     "@HD\tVN:1.6\tSO:coordinate\n" and one "@SQ\tSN:<name>\tLN:<len>\n" per reference in order; other header lines of the
 *     input are not carried.  Then the kept records in the resident order ((tid, pos + 1, strand-or-0), ties in input order),
 *     each: block_size, refID = tid, pos, l_read_name = length + 1, mapq, bin = reg2bin(pos, pos + max(span, 1)) with span the
 *     summed lengths of the M, D, N, = and X operations, n_cigar_op, flag, l_seq, next_refID = -1, next_pos = -1, tlen = 0,
 *     the name with NUL, the CIGAR words, the (l_seq + 1) / 2 packed SEQ bytes as they lie at seq_off with the low nibble of
 *     an odd last byte 0, and l_seq bytes 0xFF.  QUAL, RNEXT, PNEXT, TLEN and the optional fields are not carried (a handle
 *     opened with NP2_SAM_KEEP_ALL carries them: the full stream, below).
 *   Refusals, each naming the record (0-based in the resident order) or the reference, all raised before the output file is
 *     created: a record with pos < 0 (SAM POS 0) is NP2_E_ARG; n_cigar > 65535 is NP2_E_UNSUPPORTED (no CG tag is written);
 *     a reference with LN > 2^29, or a record with pos + max(span, 1) > 2^29, is NP2_E_UNSUPPORTED (BAI's limit; there is no
 *     CSI); a handle opened without NP2_SAM_KEEP_NAMES is NP2_E_ARG.
 *   File: the .bam is np2_bgzf_deflate_host(S, 0) byte for byte: blocks cut every 65280 bytes of S wherever records fall,
 *     and the EOF block.  Records, their length words and their fixed fields straddle blocks.
 *   Index: C[b] is the file offset of BGZF block b (C[n_blk]: the EOF block's), V(u) = C[u / 65280] << 16 | u % 65280.
 *     Record i lies at [off_i, off_i + 4 + block_size_i) of S; beg_i = V(off_i), end_i = V(off_i + 4 + block_size_i).  Per
 *     reference a maximal run of consecutive records of one bin is one chunk [beg of the first, end of the last]; bins
 *     ascending, a bin's chunks in file order.  n_intv = 1 + the largest (pos + max(span, 1) - 1) >> 14 of the reference;
 *     ioffset[w] = beg of the first record in file order that overlaps window w, an empty window takes the previous one's
 *     value, leading empty windows are 0.  A reference without records has n_bin = 0 and n_intv = 0.  No pseudo-bin 37450
 *     and no n_no_coor.
 *   Out of scope: QUAL, RNEXT, PNEXT, TLEN, optional fields and header lines other than @HD and @SQ (all of them carried by
 *     the full stream, NP2_SAM_KEEP_ALL, below); unmapped records; CSI;
 *     the 37450 pseudo-bin; compression levels; several ranks; inputs larger than one device's memory; a BAM on standard
 *     input (BAM files are taken: "BAM input", below).
 * The stream is assembled (k_bam_emit), compressed (k_bgzf_deflate) and indexed on the device; it never passes through host
 * memory.  Test hook, read once per call: NP2_BGZF_TEST_BATCH (blocks per batch). */
#define NP2_SAM_KEEP_NAMES 1u
/* np2_sam_open with a flags word (np2_sam_opts_t keeps its size) */
int np2_sam_open_ex(np2_ctx_t *ctx, const char *const *paths, int n_paths, const np2_sam_opts_t *opts, uint32_t flags,
                    np2_sam_t **out);
typedef struct np2_bamout_stats {
    uint64_t records;      /* written */
    uint64_t stream_bytes; /* of S */
    uint64_t file_bytes;   /* of the .bam */
    uint64_t blocks;       /* BGZF blocks, the EOF block not counted */
    uint64_t bins, chunks; /* of the .bai, all references */
    float sizes_ms;        /* k_bam_sizes and its scan (HIP events; 0 from the host twin, as are the next three) */
    float emit_ms;         /* k_bam_emit, summed over the batches */
    float deflate_ms;      /* k_bgzf_deflate, summed over the batches */
    float index_ms;        /* the index kernels, scans and sort */
} np2_bamout_stats_t;
/* Writes bam_path and bai_path (NULL: bam_path + ".bai").  stats may be NULL.  A refused call leaves no file. */
int np2_sam_write_bam(np2_ctx_t *ctx, np2_sam_t *sam, const char *bam_path, const char *bai_path, np2_bamout_stats_t *stats);
/* the uncompressed stream S on the host, for tests: *S is released with np2_free */
int np2_sam_bam_stream(np2_ctx_t *ctx, np2_sam_t *sam, uint8_t **S, uint64_t *n);
/* The host twin: uses no device.  From the arrays np2_sam_export returns (n_cigar_words and seq_bytes are their sizes), the
 * name bytes and name_ref[i] = offset << 8 | length per record, and the reference list, it writes the same two files by
 * running the kernels' per-record code on the CPU.  bam_path may be NULL (no file is written); S / n_S may be NULL, otherwise
 * *S is the stream, released with np2_free.  Every array is checked against its size first (NP2_E_ARG). */
int np2_bamout_host(const np2_bamrec_t *recs, const int32_t *tids, const uint32_t *cigar, const uint8_t *seq4, uint64_t n_recs,
                    uint64_t n_cigar_words, uint64_t seq_bytes, const uint8_t *names, uint64_t name_bytes, const uint64_t *name_ref,
                    const char *const *ref_names, const uint32_t *ref_lens, int n_refs, const char *bam_path, const char *bai_path,
                    uint8_t **S, uint64_t *n_S, np2_bamout_stats_t *stats);
/* the name bytes and name_ref array of a resident SAM opened with NP2_SAM_KEEP_NAMES, for the host twin and parity tests:
 * both released with np2_free, NULL when empty */
int np2_sam_export_names(np2_ctx_t *ctx, np2_sam_t *sam, uint8_t **names, uint64_t *name_bytes, uint64_t **name_ref, uint64_t *n_recs);

/* ---- the full BAM: QUAL, the mate fields, the optional fields and the header lines carried too ---------------------------------
 * THE RULE IS DEFINED HERE, on the SAM specification sections 1.4, 1.5 and 4.2.4; it is not pinned against samtools.
 * Everything here is opt-in: without NP2_SAM_KEEP_ALL np2_sam_open_ex, np2_sam_write_bam and np2_sam_bam_stream launch what
 * they launch without it and write the same bytes (the lean stream above).
 *   Flag: np2_sam_open_ex with NP2_SAM_KEEP_ALL, which implies NP2_SAM_KEEP_NAMES.
 *   What the handle keeps: per kept record a TAIL in a device buffer of its own, written where the record was met, as the names
 *     are: next_refID i32, next_pos i32, tlen i32, aux_len u32, then l_seq quality bytes if QUAL is present, then aux_len bytes
 *     of binary optional fields, then zero bytes up to a multiple of 4 (every tail begins at a word).  Per record
 *     tail_ref = offset << 1 | has_qual (u64) travels through the sort as name_ref does.  np2_bamrec_t and np2_sam_stats_t keep
 *     their layouts.
 *   RNEXT: "*" is -1, "=" the record's own tid, any other name must be an @SQ name (else NP2_E_ARG).  PNEXT: decimal
 *     0..2^31-1, stored minus 1.  TLEN: an optional sign and a magnitude of at most 2^31-1.  A non-digit or an overflow is
 *     NP2_E_ARG.
 *   QUAL: "*" means no quality bytes; the writer then puts l_seq bytes 0xFF, as the lean stream does.  Otherwise QUAL is exactly
 *     l_seq bytes, each in '!'..'~', stored minus 33.  NP2_E_ARG: a length that differs from SEQ's (an empty QUAL included), a
 *     byte outside that range, QUAL given while SEQ is "*".
 *   Optional fields: every further tab-separated field is TAG:TYPE:VALUE, kept in input order.  TAG is [A-Za-z][A-Za-z0-9].
 *     A: one byte '!'..'~'.
 *     i: an optional sign and decimal digits, value v, stored in the smallest type that holds it: v >= 0: C up to 255, S up to
 *        65535, I up to 2^32-1; v < 0: c down to -128, s down to -32768, i down to -2^31; anything outside is NP2_E_ARG.
 *     f: [-+]?digits[.digits]?([eE][-+]?digits)?.  The value is the double M x 10^e or M / 10^-e from ONE IEEE multiplication
 *        or division, cast to float; M is all the digits read as an integer, e the exponent minus the number of fraction
 *        digits.  Accepted only when M < 2^53 and |e| <= 22: both operands are then exact and the double is correctly rounded,
 *        which is what (float)strtod() gives.  inf, nan and anything outside that window are NP2_E_UNSUPPORTED.  (The library
 *        is built without fast-math; this needs that.)
 *     Z: bytes ' '..'~', possibly none, stored with a NUL.  H: an even number of hex digits, stored as the text with a NUL.
 *     B: [cCsSiIf](,number)*, zero elements allowed, every element range-checked against the subtype (an f element by the f
 *        rule); stored as B, subtype, u32 count, the values.
 *     NP2_E_ARG: a field shorter than 5 bytes, a malformed TAG or colon, an unknown TYPE.  Duplicate tags are not checked, CG
 *     is not special, n_cigar > 65535 stays refused by the writer.
 *   Which line speaks: within one line the first bad field in field order.  Within a piece of text tail errors rank with name
 *     errors: the errors of the lean parse speak first, then the first line in input order with a bad name or tail, giving the
 *     1-based line and the field, or the TAG where there is one.
 *   Header text of the full stream: "@HD\tVN:1.6\tSO:coordinate\n", the @SQ lines as in the lean stream, then every other header
 *     line of the input except @HD, in input order, files in argument order, each without its '\r'; a line byte-identical to an
 *     earlier one is dropped.  The host reads the header.
 *   Stream and index: a record is the lean stream's bytes up to SEQ with next_refID, next_pos and tlen taken from the tail,
 *     then the quality bytes or the run of 0xFF, then the optional fields' bytes; block_size grows by aux_len.  File and index
 *     rules are unchanged: blocks are cut every 65280 bytes, the .bai comes from the records' offsets, the refusals are the same.
 *   Memory: the tails take about 1.5 bytes per base (with the packed SEQ: one for the quality, half for SEQ) plus the optional
 *     fields and 16 bytes a record; device memory that does not suffice is NP2_E_NOMEM, and the message says how much was needed.
 *     The lean handle needs about a third of that.
 *   Out of scope: unmapped records (counted and dropped, as before); a CG tag for long CIGARs, CSI and the 37450 pseudo-bin; a
 *     BAM on standard input; several ranks; inputs larger than one device's memory; validating what a tag means; the sub-fields
 *     of the input's @HD line. */
#define NP2_SAM_KEEP_ALL 2u
/* the tail bytes and the tail_ref array (sorted order) of a resident SAM opened with NP2_SAM_KEEP_ALL: both released with
 * np2_free, NULL when empty */
int np2_sam_export_tails(np2_ctx_t *ctx, np2_sam_t *sam, uint8_t **tails, uint64_t *tail_bytes, uint64_t **tail_ref, uint64_t *n_recs);
/* the header text of the full stream; borrowed until np2_sam_close.  A handle opened without NP2_SAM_KEEP_ALL: NP2_E_ARG */
int np2_sam_header_text(np2_sam_t *sam, const char **text, uint64_t *n);
/* k_sam_tail_len with its scan and k_sam_tail_emit (HIP events, summed over the pieces), and the bytes of all tails; any pointer
 * may be NULL; zeros for a handle opened without NP2_SAM_KEEP_ALL */
int np2_sam_tail_stats(np2_sam_t *sam, float *tail_len_ms, float *tail_emit_ms, uint64_t *tail_bytes);
/* np2_bamout_host with the tails (tail_bytes of them; every offset a multiple of 4), tail_ref[i] per record and the header text
 * as np2_sam_header_text returns it.  tail_ref == NULL: the lean records; header_text == NULL: the lean header.  No device. */
int np2_bamout_host_full(const np2_bamrec_t *recs, const int32_t *tids, const uint32_t *cigar, const uint8_t *seq4, uint64_t n_recs,
                         uint64_t n_cigar_words, uint64_t seq_bytes, const uint8_t *names, uint64_t name_bytes, const uint64_t *name_ref,
                         const uint8_t *tails, uint64_t tail_bytes, const uint64_t *tail_ref, const char *header_text, uint64_t header_bytes,
                         const char *const *ref_names, const uint32_t *ref_lens, int n_refs, const char *bam_path, const char *bai_path,
                         uint8_t **S, uint64_t *n_S, np2_bamout_stats_t *stats);
/* Host only, no device: SAM text in memory, header included, walked as ONE piece by the one-lane text of the rule
 * (csrc/np2_samtail_core.hpp), which is what the kernels' lanes run.  Per alignment line that is not empty, in input order
 * (*n_lines of them): status[i] = 0 for a kept record, whose tail lies at tail_ref[i] >> 1 of *tails (tail_ref[i] & 1:
 * has_qual); 1 for a record that is not kept (unmapped: its tail is not looked at); NP2_E_ARG or NP2_E_UNSUPPORTED for a
 * refused line, where[i] then (field + 1) << 8 | kind for a bad tail (field 0 - 3: RNEXT, PNEXT, TLEN, QUAL; 4 + k: optional
 * field k), a small number for a bad QNAME and 0 for a line the lean parse refuses; tail_ref[i] is all ones unless status[i] is
 * 0.  header_text (or NULL): the full stream's header text.  Release the five with np2_free.  Returns NP2_OK when no line is
 * refused; otherwise the status of the line that speaks, with its message in np2_io_last_error(), the arrays filled all the
 * same.  A bad header line is NP2_E_ARG and returns nothing. */
int np2_sam_tails_host(const uint8_t *text, uint64_t n, uint8_t **tails, uint64_t *tail_bytes, uint64_t **tail_ref, int32_t **status,
                       uint32_t **where, uint64_t *n_lines, char **header_text, uint64_t *header_bytes);

/* ---- BAM input: np2_sam_open / np2_sam_open_ex take BAM files, inflated and unpacked on the device --------------------------
 * THE RULE IS DEFINED HERE, on the SAM specification section 4.2; it is not pinned against samtools.
 *   Inputs: each path is sniffed on its own: a file whose first bytes are a BGZF block that inflates to "BAM\1" is a BAM,
 *     anything else is SAM text, as before.  SAM and BAM inputs may be mixed in one call.  A BAM on standard input is
 *     NP2_E_UNSUPPORTED and the message says so.  No index is read, and the input's own order does not matter.
 *   Header: the binary reference list (n_ref, names, l_ref) is the file's @SQ list, held to the several-files rule: it must
 *     equal the first file's (else NP2_E_ARG with that rule's message).  The lines of the header text other than @HD and @SQ are
 *     carried by a NP2_SAM_KEEP_ALL handle exactly as a SAM file's are.  The host reads the header (zlib on its first blocks).
 *   A record is kept iff refID >= 0 and !(flag & 4); otherwise it counts in stats.unmapped and is looked at no further.  A
 *     refID below -1 or >= n_ref is NP2_E_ARG.
 *   A kept record becomes exactly what its SAM line would: np2_bamrec_t (pos, flag, mapq, n_cigar, l_seq), tid, the sort key of
 *     the SAM path, the CIGAR words as they stand (an operation above 8 is NP2_E_ARG), the (l_seq + 1) / 2 SEQ bytes with the
 *     low nibble of an odd last byte forced to 0; pos below -1 is NP2_E_ARG.  With NP2_SAM_KEEP_NAMES the l_read_name - 1 name
 *     bytes: the name must be 1..254 bytes with a NUL behind them, else NP2_E_ARG.  With NP2_SAM_KEEP_ALL the tail of the full
 *     BAM: next_refID must be -1 or < n_ref, next_pos >= -1 (else NP2_E_ARG), tlen is taken as it stands, aux_len is what
 *     remains of block_size, then the quality bytes, then the optional fields copied verbatim.
 *   Qualities: has_qual = 0 when l_seq == 0 or all l_seq bytes are 0xFF; otherwise every byte must be <= 93 (what the text
 *     rule admits), else NP2_E_ARG.
 *   Optional fields: one lane walks the types: A c C take 1 byte, s S 2, i I f 4, Z H run to a NUL inside the record, B is
 *     subtype, u32 count, values.  The walk must end exactly at the record's end, else NP2_E_ARG.  Values are not re-encoded:
 *     an integer keeps the type the file gave it, a float keeps its bits, inf and nan included.
 *   Refusals: block_size < 32, or fields that overrun the record: NP2_E_ARG.  A last record the stream does not finish:
 *     NP2_E_ARG "truncated BAM".  Fewer than 4 bytes behind the last record (or a block_size below 32 there): NP2_E_ARG.  The
 *     long-CIGAR placeholder (n_cigar == 2, l_seq S, then an N operation): NP2_E_UNSUPPORTED, there is no CG support.  A record
 *     of more than the piece size (4 + block_size bytes; 32 MiB, NP2_SAM_TEST_PIECE): NP2_E_UNSUPPORTED, as for a line.  A
 *     block whose CRC32 fails: the readers' message with the block's file offset.  Every message names the file and the
 *     record's 0-based number in that file; within a record the first check in the order of the W_* list of
 *     csrc/np2_bamin_core.hpp speaks, within a file the first refused record.
 *   Pieces: the reader thread takes the file's bytes into pinned pieces that end at a BGZF block boundary, so that the blocks'
 *     summed ISIZE fits the piece size; a piece always holds at least one whole block.  A record that straddles pieces is
 *     copied, device to device, to the front of the next piece's inflated bytes.  A missing EOF block is accepted, an empty
 *     block anywhere too.
 *   Order of ties is unchanged: input order, files in argument order.  np2_sam_stats_t keeps its layout: `lines` grows by a
 *     BAM file's record count.
 *   Out of scope: BAM on standard input, CG, CSI, unmapped records, several ranks, inputs larger than one device's memory. */
typedef struct np2_bamin_stats {
    uint64_t files;          /* inputs that were BAM */
    uint64_t blocks;         /* their BGZF blocks behind the header, empty ones included */
    uint64_t comp_bytes;     /* file bytes of those blocks */
    uint64_t inflated_bytes; /* what they inflate to */
    uint64_t records;        /* records walked, unmapped ones included */
    float inflate_ms;        /* k_bgzf_inflate (HIP events, summed over the pieces, as the next four) */
    float crc_ms;            /* k_bgzf_crc32 */
    float walk_ms;           /* k_bamin_walk */
    float fields_ms;         /* k_bamin_fields and the scans */
    float pack_ms;           /* k_bamin_pack */
} np2_bamin_stats_t;
/* zeros for a handle none of whose inputs was a BAM */
int np2_sam_bamin_stats(np2_sam_t *sam, np2_bamin_stats_t *stats);
/* The host twin: uses no device.  An inflated BAM stream in host memory, header included, walked by the one-lane text of the
 * rule (csrc/np2_bamin_core.hpp).  flags: 0, NP2_SAM_KEEP_NAMES or NP2_SAM_KEEP_ALL; opts may be NULL.  Per record in input order
 * (*n_records of them): status[i] = 0 for a kept record, 1 for one that is not kept, NP2_E_ARG or NP2_E_UNSUPPORTED for a refused
 * one, where[i] then says which check (np2bamin::W_*; 0 otherwise).  A stream that ends inside a record, or in bytes that are
 * no record, has a last entry for that.  Of the *n_kept kept records, in input order: recs (cigar_off and seq_off index the
 * arrays here), tids, cigar, seq4, names and name_ref (offset << 8 | length; with either flag), tails and tail_ref
 * (offset << 1 | has_qual; with NP2_SAM_KEEP_ALL).  Release the ten with np2_free; each is NULL when empty.  Returns NP2_OK when
 * no record is refused, otherwise the status of the first refused record with its message in np2_io_last_error(), the arrays
 * filled all the same.  A bad header is NP2_E_ARG and returns nothing. */
int np2_bamin_host(const uint8_t *stream, uint64_t n, uint32_t flags, const np2_sam_opts_t *opts, int32_t **status, uint32_t **where,
                   uint64_t *n_records, np2_bamrec_t **recs, int32_t **tids, uint32_t **cigar, uint64_t *n_cigar_words, uint8_t **seq4,
                   uint64_t *seq_bytes, uint8_t **names, uint64_t *name_bytes, uint64_t **name_ref, uint8_t **tails, uint64_t *tail_bytes,
                   uint64_t **tail_ref, uint64_t *n_kept);

#ifdef __cplusplus
}
#endif
#endif
