/*
 * stem_kernel.h -- C ABI of the MI355X stem-kernel Gram engine.
 *
 * Drop-in boundary for the reference's hot path (keio-bioinformatics/stem_kernel
 * rev 296): the per-pair kernel DP evaluated for every (i,j) cell of the Gram
 * matrix by KernelMatrix::calculate (common/kernel_matrix.h:67-105,
 * common/kernel_matrix.cpp:485-575).  Each entry point below names the
 * reference interface it replaces.  Plain pointers and sizes only; every call
 * returns SK_OK (0) or a negative sk_status and never throws.  Host buffers are
 * caller-owned; device buffers (sk_*_device) are addresses in the context's HIP
 * device.
 *
 * Semantics kept from the reference:
 *   - K(x,y) is evaluated with x = row example, y = column example, only for
 *     i <= j, and mirrored (kernel_matrix.cpp:44-55): the DAG kernel is not
 *     symmetric;
 *   - normalisation K_ij / sqrt(K_ii K_jj), diagonal := 1, only when asked
 *     (kernel_matrix.cpp:560-571); NaN from non-positive diagonals propagates;
 *   - libsvm precomputed-kernel text layout (kernel_matrix.cpp:756-770).
 */
#ifndef STEM_KERNEL_H
#define STEM_KERNEL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SK_ABI_VERSION 3

typedef enum {
  SK_OK = 0,
  SK_ERR_INVALID = -1,    /* bad argument (the reference threw const char*) */
  SK_ERR_HIP = -2,        /* HIP runtime error */
  SK_ERR_NO_DEVICE = -3,  /* no gfx950 device / HIP unavailable */
  SK_ERR_ALLOC = -4,      /* host or device allocation failed */
  SK_ERR_RANGE = -5,      /* index out of range */
  SK_ERR_UNSUPPORTED = -6 /* kernel kind / size not supported */
} sk_status;

/* Kernel kinds: the instantiations stem_kernel_lite/main.cpp:180-215 dispatches
 * to, plus their components (stem_kernel_lite/def_kernel.h, ss_kernel.h). */
typedef enum {
  SK_SU_STEM = 0,      /* SuStemKernel(loop_gap, beta, band)        --no-string     */
  SK_SI_STEM = 1,      /* SiStemKernel(loop_gap, stack, covar, band) --no-string --no-ribosum */
  SK_SU_STR = 2,       /* StringKernel(gap, alpha)                                  */
  SK_SI_STR = 3,       /* StringKernel(gap, match, mismatch)                        */
  SK_SU_STEM_STR = 4,  /* SuStemStrKernel == StemStrKernel (ss_kernel.h)  default   */
  SK_SI_STEM_STR = 5,  /* SiStemStrKernel                                --no-ribosum */
  SK_LSU_STEM = 6,     /* LSuStemKernel: beta*log(K_stem)                --log --no-string */
  SK_LSU_STEM_STR = 7, /* LSuStemStrKernel: beta*log K_stem + alpha*log K_str  --log */
  SK_NAIVE_STR = 8,    /* StringKernel<double>(gap) of string_kernel/ (exact character
                          match of row 0, weight gap^2, string_kernel.cpp:11-50) */
  /* BPLAKernel<double,MData> of bpla_kernel/ (bpla_kernel.cpp:159-174) */
  SK_BPLA = 9,         /* local_alignment_exp with BPLAScore            (default)    */
  SK_LA = 10,          /* local_alignment_exp with LAScore               --noBP      */
  SK_BPLA_SW = 11,     /* local_alignment_max with BPLAScore             --SW        */
  SK_LA_SW = 12,       /* local_alignment_max with LAScore               --noBP --SW */
  /* StemKernel<double,BPMat>::full_dp of stem_kernel/ (stem_kernel.cpp:282-351)
   * over single sequences (row 0, lowercased as the loader does) */
  SK_STEM4D = 13,
  /* BPLAKernel<double,AAMData> of bpla_kernel/ (la_kernel: la_main.cpp:131-135,
   * instantiated at bpla_kernel.cpp:406) over protein datasets
   * (sk_dataset_add_protein): LAScore over the 23 amino-acid letters, noBP */
  SK_AA_LA = 14,       /* local_alignment_exp                                        */
  SK_AA_LA_SW = 15,    /* local_alignment_max                            --SW        */
  /* KernelFunc(tolerance) of simpal/ (simpal.cpp:225-280), the "Simple
   * Palindrome Kernel", over palindrome datasets (sk_dataset_add_palindromes).
   * The tolerance (allowable key mismatches, -t, default 1) is read from the
   * mismatch field: it must be integral (else SK_ERR_INVALID), and a negative
   * value is the reference's tolerance_ < 0: every key pair counts. */
  SK_SIMPAL = 16
} sk_kernel_kind;

/* Kernel parameters; defaults are stem_kernel_lite/main.cpp:103-149
 * (sk_kernel_params_default).  BPLA kinds use alpha, beta, gap, ext and
 * score_table with the defaults of bpla_kernel/main.cpp:20-26, 68-76; that
 * CLI parses them as float, so the defaults are float-rounded. */
typedef struct {
  int32_t kind;       /* sk_kernel_kind */
  uint32_t len_band;  /* --length-band (0 = off), default 10 */
  double beta;        /* -b   0.3 */
  double loop_gap;    /* -g   0.2 */
  double stack;       /* -s   1.3 */
  double covar;       /* -v   0.8 */
  double alpha;       /* -a   0.2 */
  double gap;         /* -G   0.8 */
  double match;       /* --match 1.0 */
  double mismatch;    /* --mismatch 0.8; SK_SIMPAL: the tolerance -t (an integer,
                         default 1; negative: every key pair counts) */
  double ext;         /* BPLA -e (gap extension), -0.75 */
  double score_table[16]; /* BPLA --score table, [x residue][y residue] ACGU */
  /* 4-D stem kernel (stem_kernel/main.cpp:40-60; float options): gap -g 0.8,
   * stack -s 1.0 (fields above), and: */
  double subst;       /* -v substitution weight for base pairs, 0.5 */
  double bp_bound;    /* -p pairs count when prob > bp_bound (float compare), 0.0 */
  int32_t bp_model;   /* 0: dataset bpp (BPMatrix/PFWrapper, the -p path),
                         1: NormalBasePair, 2: WobbleBasePair (-w) */
  uint32_t loop;      /* -l minimum loop (Normal/Wobble models), 3 */
  /* -a alignment constraints (stem_kernel.cpp:14-81): when > 0, partial_dp
   * restricted to the PairHMM MAP path's match positions whose posterior is
   * >= ali_bound (PairHMM<Ribosum>, stem_kernel/phmm.cpp), widened by
   * len_band; 0.0 = off.  Sequences must then be ACGU only (the reference
   * asserts in char2rna, phmm.cpp:247-258). */
  double ali_bound;   /* float option, compared as float */
  /* LogValue zerop semantics (log_value.h:374-378).  0: as the reference
   * builds with a C++11 <cmath> (std::isinf returns bool, `<0` is never true,
   * posteriors are NaN and no position is anchored); 1: the intended -inf
   * test (anchored constraints). */
  int32_t ali_zerop_fixed;
  /* SK_AA_LA / SK_AA_LA_SW: the 23x23 amino-acid score table, [x residue][y
   * residue] in char2aa order ARNDCQEGHILKMFPSTWYVBZX (common/aaprofile.cpp:
   * 13-23); default BLOSUM62 (la_main.cpp:21-46).  These kinds use gap, ext
   * and beta (float-rounded defaults -10, -1, 0.11, la_main.cpp:87-90); no
   * other kind reads the field. */
  double aa_score_table[529];
} sk_kernel_params;

void sk_kernel_params_default(sk_kernel_params *p, int32_t kind);

/* ---------------------------------------------------------------- context */
typedef struct sk_context sk_context;

/* One context per GPU (HIP device ordinal).  hip_stream may be NULL (the
 * context creates its own) or a hipStream_t owned by the caller. */
int sk_open(int device, void *hip_stream, sk_context **ctx);
int sk_close(sk_context *ctx);
const char *sk_strerror(int status);
/* Last error message recorded on this context (static storage). */
const char *sk_last_error(const sk_context *ctx);

/* ---------------------------------------------------------------- examples */
/* An example set: the reference's ExampleSet of (label, MData)
 * (common/framework.h:308-353), built host-side and uploaded once. */
typedef struct sk_dataset sk_dataset;

int sk_dataset_create(sk_dataset **ds);
int sk_dataset_free(sk_dataset *ds);

/* Append one example = one alignment of n_rows rows of equal length.
 * bpp_rows[r]: base-pairing probabilities of row r after erase_gap (length
 * n_r = number of non-'-' characters), strict upper triangle packed row-major:
 * p(i,j), 0<=i<j<n_r, at i*n_r - i*(i+1)/2 + (j-i-1).  This is the matrix
 * Vienna pf_fold would give the reference (common/bpmatrix.cpp:151-177).
 * th = --basepair.  use_bp = 0 builds MData(ma) (no DAG; string kernels only).
 * Replaces: new MData(ma, th, pf_scale, opts)  stem_kernel_lite/data.cpp:324-345
 * and DataLoader<MData>::get()  stem_kernel_lite/data.cpp:548-586. */
int sk_dataset_add(sk_dataset *ds, const char *label, int n_rows,
                   const char *const *rows, const double *const *bpp_rows,
                   float th, int use_bp);
/* Append n single-sequence examples, folding each with sk_fold_synthetic and
 * building its DAG on n_threads host threads (0 = hardware concurrency).
 * labels may be NULL ("+1").  Parallel form of the reference's load loop
 * (common/framework.h:308-353 + DataLoader<MData>::get). */
int sk_dataset_add_synthetic(sk_dataset *ds, int32_t n, const char *const *seqs,
                             const char *const *labels, float th, int32_t n_threads);
/* Same for alignments: n examples of n_rows equal-length rows each, rows
 * [i*n_rows + r]; every row is folded gap-erased and lowercased, then the
 * per-row matrices are averaged (common/bpmatrix.cpp:306-342, 399-417). */
int sk_dataset_add_synthetic_rows(sk_dataset *ds, int32_t n, int32_t n_rows,
                                  const char *const *rows, const char *const *labels,
                                  float th, int32_t n_threads);
/* Append one protein example = one alignment of n_rows rows of equal length
 * over the amino-acid alphabet (unequal rows: SK_ERR_INVALID, "wrong
 * alignment", bpla_kernel/data.cpp:284-288; 4,096 rows or more:
 * SK_ERR_UNSUPPORTED).  Each column holds the integer count of every letter
 * of char2aa, any other character ('-', '*', 'U', ...) counted in slot 23
 * (AAProfileSequence::add_sequence, common/aaprofile.cpp:49-60).  A dataset is
 * RNA or protein, decided by its first example: mixing gives SK_ERR_INVALID,
 * and so does an SK_AA_* kind on an RNA dataset or any other kind on a
 * protein dataset.  Replaces: new AAMData(ma)  bpla_kernel/data.cpp:263-293. */
int sk_dataset_add_protein(sk_dataset *ds, const char *label, int n_rows,
                           const char *const *rows);
/* AAProfileSequence of protein example i: prof24 gets len*24 floats (the 23
 * letters of char2aa, then "other"), *n_seqs the row count. */
int sk_dataset_aa_profile(const sk_dataset *ds, int i, float *prof24, float *n_seqs);
/* char2aa (common/aaprofile.cpp:13-23): 0..22 for ARNDCQEGHILKMFPSTWYVBZX in
 * either case, 23 for everything else. */
int sk_char2aa(int c);
/* Append one palindrome example: Pals(seq, seed_length, min_loop, max_dist)
 * of simpal/simpal.cpp:37-218 over the lowercased sequence (load_examples,
 * :298) and its base-pairing probabilities bpp (strict upper triangle packed
 * as in sk_dataset_add, over the n characters of seq; the reference folds with
 * PFWrapper(seq, noGU = true), :128).  An entry per (k-mer, d): forward k-mer
 * at i and an equal k-mer of the reversed complement at r, i and r in
 * [0, n - seed_length) (the last k-mer is skipped, :116), d = n - i - r -
 * 2 seed_length with min_loop <= d <= max_dist; its weight the float product
 * of the seed_length float-rounded p(i+1+t, n-r-t), weights of one (key, d)
 * added in float in the order increasing i, then increasing r (the reference
 * adds them in the iteration order of a hash_multimap).  The "m\tn" lines the
 * reference prints are not reproduced.  n < seed_length: SK_ERR_INVALID (the
 * reference's loop bound wraps); seed_length outside 1..32:
 * SK_ERR_UNSUPPORTED; a seed_length other than the dataset's: SK_ERR_INVALID
 * (the reference asserts equal key lengths, :272).  A dataset is RNA, protein
 * or palindrome, decided by its first example: mixing gives SK_ERR_INVALID,
 * and so does SK_SIMPAL on another dataset or another kind on this one. */
int sk_dataset_add_palindromes(sk_dataset *ds, const char *label, const char *seq,
                               const double *bpp, int32_t seed_length, int32_t min_loop,
                               int32_t max_dist);
/* A palindrome example from explicit entries: keys holds n * seed_length
 * letters of acgu, dist non-negative values, weight finite non-negative
 * floats; anything else, and a duplicate (key, dist), is SK_ERR_INVALID.  The
 * entries are sorted into map order (key, then dist; simpal.cpp:64-67). */
int sk_dataset_add_palindrome_entries(sk_dataset *ds, const char *label, int32_t seed_length,
                                      int32_t n, const char *keys, const int32_t *dist,
                                      const float *weight);
/* The entries of palindrome example i in map order: *n their number, keys
 * n * seed_length letters (no terminator), dist and weight n values each
 * (any pointer may be NULL). */
int sk_dataset_palindromes(const sk_dataset *ds, int i, int32_t *n, char *keys, int32_t *dist,
                           float *weight);
/* The palindrome kernel's compile-time tile sizes (csrc/kernels/simpal.hip):
 * y entries per LDS tile, x entries per lane (a block of x entries is 64 *
 * x_block). */
int sk_simpal_shape(int32_t *y_tile, int32_t *x_block);
/* Append a copy of example i of src (its built DAG, profile and weights: no
 * rebuild) to dst, e.g. to assemble the pair a per-pair Kernel::operator()
 * call evaluates from examples built once.  dst must not be uploaded yet. */
int sk_dataset_add_copy(sk_dataset *dst, const sk_dataset *src, int32_t i);
int sk_dataset_size(const sk_dataset *ds);
/* Examples [first, first + count) as bytes -- their labels, built DAGs,
 * profiles, weights and averaged bp matrices, every field as the dataset
 * holds it -- into buf (cap bytes); *size = the bytes needed (buf NULL: query
 * only; SK_ERR_RANGE when cap is short).  sk_dataset_import appends such a
 * buffer's examples to ds (not uploaded; a malformed buffer appends nothing):
 * ranks that each build a share of the examples and gather the shares in
 * rank order hold a dataset that packs bit for bit as one built whole
 * (stem_kernel_amd/shard.py build_split).  Host-side counterpart of the
 * reference's MPI Gram, where every rank reads and builds every example
 * (common/kernel_matrix.cpp:186-261, common/framework.h:308-353). */
int sk_dataset_export(const sk_dataset *ds, int32_t first, int32_t count, uint8_t *buf,
                      size_t cap, size_t *size);
int sk_dataset_import(sk_dataset *ds, const uint8_t *buf, size_t size);
/* Diagnostic: pack ds on the host (ds not uploaded) and return FNV-1a hashes
 * of every packed array, y-role records and x-role / per-example arrays (the
 * lists of tools/pack_compare.cpp). */
int sk_dataset_pack_digest(sk_dataset *ds, uint64_t *y_hash, uint64_t *x_hash);
/* label of example i (pointer valid while ds lives) */
const char *sk_dataset_label(const sk_dataset *ds, int i);
/* DAG shape of example i: nodes, edges, bp_freq entries, roots, length */
int sk_dataset_shape(const sk_dataset *ds, int i, int32_t *n_nodes,
                     int32_t *n_edges, int32_t *n_bpfreq, int32_t *n_roots,
                     int32_t *seq_len);
/* Row traffic of example i in the x role of the DAG stem kernel's gamma
 * schedule (dag_stem.hip): its rows (the x nodes the schedule
 * computes per pair), the rows it stores in the HBM slab, and the child-row
 * reads of its rows from the slab, the y's Gamma and Phi tables and
 * registers; y_slots = its non-leaf node count, the length of every row a
 * pair (x', example i as y) moves.  Per pair (x, y) the engine moves each of
 * x's row transfers as 8 * y_slots(y) bytes.  Replaces nothing in the
 * reference (its DP keeps K0/G0 tables per pair in host memory,
 * stem_kernel_lite/stem_kernel.cpp:14-95): a roofline input of bench.py.
 * The dataset must be uploaded (packed). */
int sk_dataset_row_traffic(const sk_dataset *ds, int i, int32_t *rows, int32_t *stored,
                           int32_t *slab_reads, int32_t *gamma_reads, int32_t *phi_reads,
                           int32_t *reg_reads, int32_t *y_slots);
/* Shared child sums of example i in the x role: the
 * shared-sum combination rows the factored gamma schedule adds for it and the
 * child records of its rows they replaced; both 0 where the dataset runs the
 * plain gamma schedule.  sk_dataset_row_traffic counts the schedule that
 * runs.  No counterpart in the reference.  The dataset must be uploaded
 * (packed). */
int sk_dataset_shared_sums(const sk_dataset *ds, int i, int32_t *shared_rows,
                           int32_t *member_records);
/* LDS bank model of example i's IY sweep in the y role of the DAG stem kernel
 * (dag_stem.hip), summed over its sweep chunks as packed: read
 * cycles (per 32-lane half of a chunk, the largest number of distinct
 * children on one id mod 32; at least 2 per chunk) and atomic cycles (per
 * 16-lane group, the largest number of records on one parent id mod 16; at
 * least 4 per chunk), and the chunks.  The packer deals each chunk's lanes
 * and numbers equal-length y nodes to lower it.  No counterpart in the
 * reference.  The dataset must be uploaded (packed). */
int sk_dataset_sweep_conflicts(const sk_dataset *ds, int i, int32_t *read_cycles,
                               int32_t *atomic_cycles, int32_t *chunks);
/* Diagnostic, host only: the y role of example i packed alone (uploaded or
 * not), in the packer's numbering or, plain != 0, in the plain stable order
 * by length that the numbering permutes within runs of equal length.  Any
 * pointer may be NULL; call once for the sizes.  node[n_nodes]: the
 * level-order non-leaf node each y id holds; len[n_nodes]: its length;
 * edges[n_edges]: node-major records child:11 | parent:11 | gaps:10;
 * sweep[64 * n_chunks]: the sweep chunks' lane records (dummies: child ==
 * parent); first_chunk[max_len + 2]: the first chunk that reads a child of
 * length >= v; cost[4]: sk_dataset_sweep_conflicts' read and atomic cycles
 * of this pack, then of the plain order.  A y of the big-y kernel has no
 * sweep schedule (n_chunks 0, edge records 0). */
int sk_dataset_y_role(const sk_dataset *ds, int i, int plain, int32_t *n_nodes,
                      int32_t *n_edges, int32_t *n_chunks, int32_t *max_len, uint32_t *node,
                      uint32_t *len, uint32_t *edges, uint32_t *sweep, int32_t *first_chunk,
                      int32_t *cost);
/* DAG arrays of example i (packer-parity introspection; any pointer may be
 * NULL).  Node arrays have n_nodes entries, edge arrays n_edges (node-major,
 * reference list order), bp arrays n_bpfreq. */
int sk_dataset_dag(const sk_dataset *ds, int i, uint32_t *first, uint32_t *last,
                   uint32_t *n_edges, uint32_t *n_bpfreq, float *weight,
                   uint32_t *max_pa, uint32_t *edge_to, uint32_t *edge_gaps,
                   uint32_t *bp_code, float *bp_p, uint32_t *roots,
                   float *pos_weight);

/* ProfileSequence of example i (common/profile.cpp): prof5 gets len*5 floats
 * (A,C,G,U,gap), *n_seqs the row count. */
int sk_dataset_profile(const sk_dataset *ds, int i, float *prof5, float *n_seqs);

/* BPLA position weights of example i (bpla_kernel/data.cpp:19-45: sqrt of
 * the left, right and unpaired probabilities; 0,0,1 without base pairs),
 * len floats each (packer-parity introspection). */
int sk_dataset_bpla_weights(const sk_dataset *ds, int i, float *p_left,
                            float *p_right, float *p_unpair);

/* Upload the packed example set to the context's device (idempotent).
 * Must be called after the last sk_dataset_add and before any compute. */
int sk_dataset_upload(sk_context *ctx, sk_dataset *ds);

/* ---------------------------------------------------------------- compute */
/* Train Gram matrix: K(train[i], train[j]) for i<=j, mirrored, optional
 * normalisation.  out: n*n doubles, row-major, host memory.
 * Replaces: KernelMatrix<double>::calculate(train, kernel, normalize, n_th)
 *           common/kernel_matrix.cpp:485-575. */
int sk_gram(sk_context *ctx, sk_dataset *ds, const sk_kernel_params *kp,
            int normalize, double *out);

/* Arbitrary (x,y) pair list, results to a DEVICE buffer out_dev[k] =
 * K(ds[x[k]], ds[y[k]]).  No normalisation.  Asynchronous on the context's
 * stream; host arrays are read before return.  Used by row-block shards
 * (multi-GPU) and by the benchmark.
 * Replaces: the inner loop CalcTrainMatrix::operator() kernel_matrix.cpp:42-56
 * (and the MPI variant's per-rank share, kernel_matrix.cpp:186-261). */
int sk_pairs_device(sk_context *ctx, sk_dataset *ds, const sk_kernel_params *kp,
                    const int32_t *x, const int32_t *y, int64_t n_pairs,
                    double *out_dev);
/* Same, host output (synchronous). */
int sk_pairs(sk_context *ctx, sk_dataset *ds, const sk_kernel_params *kp,
             const int32_t *x, const int32_t *y, int64_t n_pairs, double *out);

/* Test row: out[i] = K(train[i], test[t]) for i in sv_index[0..n_sv) (all i
 * when sv_index == NULL); out has n_train entries and entries outside
 * sv_index are left untouched (the reference indexes by train position).
 * *self = K(test[t], test[t]) when self != NULL.  test and train may be the
 * same dataset.
 * Replaces: KernelMatrix::calculate(vec, data, train, sv_index, kernel, n_th,
 * data_self)  common/kernel_matrix.cpp:112-182, 635-697. */
int sk_test_row(sk_context *ctx, sk_dataset *test, int t, sk_dataset *train,
                const int32_t *sv_index, int32_t n_sv,
                const sk_kernel_params *kp, double *out, double *self);

/* Diagonal: out[i] = K(train[i], train[i]) for i in sv_index (or all i);
 * out has n_train entries.
 * Replaces: KernelMatrix::diagonal  common/kernel_matrix.cpp:59-110, 577-633. */
int sk_diagonal(sk_context *ctx, sk_dataset *ds, const int32_t *sv_index,
                int32_t n_sv, const sk_kernel_params *kp, double *out);

/* Test x train matrix: out[i*n_train + j] = K(train[j], test[i]).  When
 * norm_test || normalize, self_out[i] = K(test[i], test[i]) (self_out may be
 * NULL otherwise); when normalize, out[i][j] /= sqrt(self[i] * diag[j]).
 * Replaces: KernelMatrix::calculate(test, train, kernel, norm_test,
 * normalize, n_th)  common/kernel_matrix.cpp:699-754. */
int sk_test_matrix(sk_context *ctx, sk_dataset *test, sk_dataset *train,
                   const sk_kernel_params *kp, int norm_test, int normalize,
                   double *out, double *self_out);

/* ---------------------------------------------------------------- multi-GPU
 * One process (or host thread) per GPU, one context each.  The plan is the
 * reference MPI Gram's: upper-triangle cell k (i <= j, row-major) belongs to
 * rank k % world (CalcTrainMatrix::operator(), common/kernel_matrix.cpp:
 * 210-224).  Each rank computes its cells into a device buffer of
 * sk_shard_count(n, 0, world) doubles, one RCCL all-gather over xGMI joins
 * them on every rank, and every rank assembles the mirrored (normalised)
 * matrix -- the reference's Ssend/Recv to rank 0 and its scatter
 * (:225-261, 495-527).  The result is bit-identical to sk_gram. */
/* Cells of `rank` (host only, no GPU): count, and their (x, y) lists. */
int64_t sk_shard_count(int32_t n, int32_t rank, int32_t world);
int sk_shard_cells(int32_t n, int32_t rank, int32_t world, int32_t *x, int32_t *y);
/* Host assembly: gathered = world buffers of per_rank doubles (rank-major,
 * rank r's values in sk_shard_cells order); out = n*n, mirrored, normalised
 * as kernel_matrix.cpp:560-571 when normalize. */
int sk_shard_assemble(int32_t n, int32_t world, const double *gathered, int64_t per_rank,
                      int normalize, double *out);
/* RCCL communicator of the context: rank 0 calls sk_comm_unique_id and
 * hands the 128 bytes to every rank (any channel: MPI_Bcast, a file, a
 * socket); each rank calls sk_comm_init on its own context. */
int sk_comm_unique_id(uint8_t *id, size_t id_bytes);
int sk_comm_init(sk_context *ctx, const uint8_t *id, size_t id_bytes, int32_t rank, int32_t world);
/* ncclAllGather of count doubles per rank on the context's stream
 * (asynchronous; device buffers, recv_dev holds world*count). */
int sk_comm_allgather(sk_context *ctx, const double *send_dev, int64_t count, double *recv_dev);
/* The Gram over the communicator's ranks: every rank passes the same dataset
 * and parameters and receives the whole n*n matrix in out (host).
 * Replaces: KernelMatrix<double>::calculate under HAVE_MPI,
 * common/kernel_matrix.cpp:186-261, 495-527. */
int sk_gram_sharded(sk_context *ctx, sk_dataset *ds, const sk_kernel_params *kp, int normalize,
                    double *out);

/* ---------------------------------------------------------------- output */
/* libsvm precomputed-kernel text: "label 0:(i+1) 1:K_i1 ... n:K_in \n" with
 * ostream default formatting (6 significant digits).  Writes into buf (NUL
 * terminated) if buf_size is large enough; *needed receives the byte count
 * including the NUL.  Replaces: KernelMatrix::print common/kernel_matrix.cpp:756-770. */
int sk_format_libsvm(const double *matrix, int32_t rows, int32_t cols,
                     const char *const *labels, char *buf, size_t buf_size,
                     size_t *needed);

/* ---------------------------------------------------------------- inputs */
/* Synthetic base-pairing probabilities: Boltzmann-weighted Nussinov partition
 * function (GC 1.5, AU 1.0, GU 0.5 in kT units, hairpin >= 3).  Stand-in for
 * Vienna pf_fold; out gets n*(n-1)/2 doubles in the packed layout above. */
int sk_fold_synthetic(const char *seq, int32_t n, int32_t no_gu, double *out);

/* McCaskill base-pairing probabilities on the GPU, one workgroup per
 * sequence (csrc/kernels/fold.hip).  Replaces ViennaRNA pf_fold as the
 * reference calls it: BPMatrix FOLD, common/bpmatrix.cpp:151-177 (per row of
 * an alignment, :404-414), PFWrapper::fold, common/pf_wrapper.cpp:15-36.
 * Loop model: the Turner-1999 core ViennaRNA 1.x compiles in (stacks,
 * hairpin / bulge / interior initiation, Ninio asymmetry, terminal AU/GU,
 * linear multiloop; no mismatch, dangle or special-loop tables: its
 * parameter files are not available, so parity against ViennaRNA is
 * unpinned -- DESIGN.md §9).  seqs[k]: any case, T as U, other characters
 * never pair.  out: for each k in order, n_k(n_k-1)/2 doubles in the packed
 * layout of sk_dataset_add, concatenated.  log_z (optional): ln Z per
 * sequence.  flags: SK_FOLD_NO_GU (--noGU), SK_FOLD_NO_CLOSING_GU
 * (--noClosingGU), SK_FOLD_NO_LONELY_PAIRS (--noLonelyPairs: the legacy
 * ViennaRNA pair-type filter, pairs that can only be isolated removed).  Sequences up to ~1,400 nt (SK_ERR_UNSUPPORTED when Z
 * leaves the double range). */
#define SK_FOLD_NO_GU 1
#define SK_FOLD_NO_CLOSING_GU 2
#define SK_FOLD_NO_LONELY_PAIRS 4
int sk_fold_mccaskill(sk_context *ctx, int32_t n, const char *const *seqs, int32_t flags,
                      double *out, double *log_z);
/* Stochastic structure sampling on the GPU (csrc/kernels/fold_sample.hip):
 * BPMatrix SFOLD, common/bpmatrix.cpp:179-232 (--sampling N: pf_fold, N x
 * pbacktrack, bpp(i,j) = the fraction of samples holding the pair).  After
 * the inside pass of sk_fold_mccaskill's kernel, n_samples structures per
 * sequence are drawn from the Boltzmann ensemble of the same loop model:
 * P(structure) = exp(-E/kT) / Z.  seqs, flags and the length limit are those
 * of sk_fold_mccaskill.  out_bpp (optional): the layout of sk_fold_mccaskill's
 * out, count / n_samples in double.  out_structs (optional): for each k in
 * order, n_samples rows of n_k chars '(' ')' '.', no terminators.  log_z
 * (optional): ln Z per sequence.  At least one of out_bpp and out_structs.
 * Where the reference seeds ViennaRNA's generator from the clock, the result
 * here is a function of the arguments alone: sample s of sequence k is drawn
 * from a counter-based generator keyed by (seed, k, s, decision number), so
 * it does not depend on n_samples or on how the call is batched. */
int sk_fold_sample(sk_context *ctx, int32_t n, const char *const *seqs, int32_t flags,
                   int32_t n_samples, uint64_t seed, double *out_bpp, char *out_structs,
                   double *log_z);
/* The sampler's generator on the host: the uniform double in [0, 1) of draw
 * number draw of sample `sample` of sequence `seq` under seed. */
double sk_fold_sample_uniform(uint64_t seed, int32_t seq, int32_t sample, int32_t draw);
/* Consensus (alifold-style) partition function of alignments on the GPU, one
 * workgroup per alignment (csrc/kernels/fold_ali.hip): base-pairing
 * probabilities of alignment COLUMNS.  Replaces BPMatrix ALIFOLD,
 * common/bpmatrix.cpp:355-397 (ViennaRNA pf_alifold; parity unpinned like
 * sk_fold_mccaskill's, model in DESIGN.md §9).  A consensus structure weighs
 * exp(-(sum over rows of its energy in sk_fold_mccaskill's loop model, loop
 * sizes in columns, - sum over its pairs of the covariance score) / (S kT)),
 * S = rows; a column pair may form when at most half of the rows cannot pair
 * there and its covariance score is at least -200.  rows: alignment after
 * alignment, n_rows[k] rows of equal length each (SK_ERR_INVALID otherwise);
 * A C G U T in any case, every other character a blank.  out: for each
 * alignment in order, n_k(n_k-1)/2 doubles over its n_k columns in the
 * packed layout of sk_dataset_add, concatenated.  log_z (optional): ln Z per
 * alignment.  flags: SK_FOLD_NO_GU, SK_FOLD_NO_LONELY_PAIRS (the filter over
 * the column pairs that may form); SK_FOLD_NO_CLOSING_GU has no per-column
 * meaning when rows differ: SK_ERR_UNSUPPORTED.  S identical gap-free rows
 * give sk_fold_mccaskill of that row. */
int sk_fold_alignment(sk_context *ctx, int32_t n_aln, const int32_t *n_rows,
                      const char *const *rows, int32_t flags, double *out, double *log_z);
/* Append one example whose matrix is the caller's ONE matrix over the
 * alignment's columns (bpp: len(len-1)/2 doubles, len = the rows' length;
 * e.g. sk_fold_alignment's): the example's matrix is bpp itself, no
 * gap-mapped average, and every row's profile reads it in alignment
 * coordinates -- MData(ma, th, ...) when BPMatrix holds one matrix,
 * stem_kernel_lite/data.cpp:332-339, Profiler :109-121. */
int sk_dataset_add_consensus(sk_dataset *ds, const char *label, int n_rows,
                             const char *const *rows, const double *bpp, float th);
/* sk_dataset_add_folded with one sk_fold_alignment matrix per example in
 * place of the averaged per-row folds (BPMatrix ALIFOLD). */
int sk_dataset_add_alifolded(sk_context *ctx, sk_dataset *ds, int32_t n, int32_t n_rows,
                             const char *const *rows, const char *const *labels, float th,
                             int32_t fold_flags, int32_t n_threads);
/* n palindrome examples (sk_dataset_add_palindromes) from sequences folded
 * with sk_fold_mccaskill(fold_flags) as they stand, lowercased; the
 * reference's choice is SK_FOLD_NO_GU (PFWrapper(seq, true),
 * simpal/simpal.cpp:128).  The maps are built on n_threads host threads (0 =
 * hardware concurrency); labels may be NULL ("+1"). */
int sk_dataset_add_palindromes_folded(sk_context *ctx, sk_dataset *ds, int32_t n,
                                      const char *const *seqs, const char *const *labels,
                                      int32_t fold_flags, int32_t seed_length, int32_t min_loop,
                                      int32_t max_dist, int32_t n_threads);
/* n examples of n_rows equal-length rows (rows[i*n_rows + r]), built on
 * n_threads host threads (0 = hardware concurrency) from the caller's
 * per-row bpp (bpp_rows[i*n_rows + r], layout of sk_dataset_add; ignored
 * when use_bp = 0).  Parallel form of the reference's load loop
 * (common/framework.h:308-353 + DataLoader<MData>::get,
 * stem_kernel_lite/data.cpp:548-586). */
int sk_dataset_add_batch(sk_dataset *ds, int32_t n, int32_t n_rows, const char *const *rows,
                         const double *const *bpp_rows, const char *const *labels, float th,
                         int32_t use_bp, int32_t n_threads);
/* Same, folding every gap-erased row with sk_fold_mccaskill on ctx's GPU
 * first: the engine's whole input path (MData(ma, th, pf_scale, opts),
 * data.cpp:324-345, with BPMatrix FOLD) without ViennaRNA. */
int sk_dataset_add_folded(sk_context *ctx, sk_dataset *ds, int32_t n, int32_t n_rows,
                          const char *const *rows, const char *const *labels, float th,
                          int32_t fold_flags, int32_t n_threads);
/* sk_dataset_add_folded with sk_fold_sample's bpp (BPMatrix SFOLD); the
 * generator's sequence index is the row's index i*n_rows + r in the call. */
int sk_dataset_add_sampled(sk_context *ctx, sk_dataset *ds, int32_t n, int32_t n_rows,
                           const char *const *rows, const char *const *labels, float th,
                           int32_t fold_flags, int32_t n_samples, uint64_t seed, int32_t n_threads);

/* BPLA gradients, the bpla_optimizer's per-pair step: for k < n_pairs,
 * value[k] = BPLAKernel::compute_gradients(xs[x[k]], ys[y[k]], score_table,
 * {alpha, beta, gap, ext}, d) and grad[4k..4k+3] = d (d/d alpha, beta, gap,
 * ext).  Replaces bpla_kernel/bpla_kernel.cpp:385-401 (BPLA_Forward :178-243,
 * BPLA_Backward :245-305, BPLA_ForwardBackword :325-383) as called from
 * bpla_kernel/bpla_optimizer.cpp:52-255.  Uses kp->alpha/beta/gap/ext and
 * kp->score_table; examples need base pairs.  Host buffers; synchronous. */
int sk_bpla_gradients(sk_context *ctx, sk_dataset *xs, sk_dataset *ys, const sk_kernel_params *kp,
                      const int32_t *x, const int32_t *y, int64_t n_pairs, double *value,
                      double *grad);

/* Gradients of the protein local-alignment kernel (kind SK_AA_LA), the step
 * an optimizer of beta, gap and ext takes per pair: for k < n_pairs,
 * value[k] = BPLAKernel<double,AAMData>::compute_gradients(xs[x[k]], ys[y[k]],
 * aa_score_table, {1, beta, gap, ext}, d) (bpla_kernel/bpla_kernel.cpp:385-401,
 * instantiated at :406) over examples whose p_left and p_right are 0 and
 * p_unpair 1 -- what the noBP kernel scores; the reference's loader leaves the
 * three vectors empty -- and grad[4k..4k+3] = d = d/d(alpha, beta, gap, ext),
 * sk_bpla_gradients' layout.  The alpha slot is always +0.0.
 *
 * value is NOT sk_pairs' SK_AA_LA value (operator()): compute_gradients'
 * forward model (BPLA_Forward, :178-243) starts alignments through its states
 * F_LX = 1, F_LY = j and so weights alignment starts differently.  It is the
 * model the reference's optimizer differentiates, as sk_bpla_gradients' value
 * is for RNA; it is not symmetric in (x, y), so ordered pairs matter.
 *
 * Uses kp->beta, kp->gap, kp->ext and kp->aa_score_table.  Errors, all before
 * any launch: SK_ERR_INVALID for a dataset that is not protein or a kind other
 * than SK_AA_LA (SK_AA_LA_SW has no gradient), SK_ERR_RANGE for an index
 * outside its dataset, and, on the GPU only, SK_ERR_UNSUPPORTED for a y longer
 * than sk_la_protein_grad_shape reports for its path (the x length is not
 * limited).  Host buffers; synchronous.
 *
 * The GPU call (csrc/kernels/la_protein_grad.hip) runs pairs of examples with
 * one residue kind per column on the code kernel and the rest on the profile
 * kernel; it sums in another order than the reference (about 1e-13 relative)
 * and gives a pair the same bits whatever the batch around it.  The host call
 * restates the reference operation by operation and equals it bit for bit;
 * it needs no upload, and runs pairs on n_threads threads (0: all). */
int sk_la_protein_gradients(sk_context *ctx, sk_dataset *xs, sk_dataset *ys, const sk_kernel_params *kp,
                            const int32_t *x, const int32_t *y, int64_t n_pairs, double *value, double *grad);
int sk_la_protein_gradients_host(sk_dataset *xs, sk_dataset *ys, const sk_kernel_params *kp,
                                 const int32_t *x, const int32_t *y, int64_t n_pairs, int32_t n_threads,
                                 double *value, double *grad);
/* The longest y (columns) of the GPU call's code and profile paths: what a
 * one-wave workgroup's LDS holds. */
int sk_la_protein_grad_shape(int32_t *max_y_code, int32_t *max_y_profile);
/* Kernels the last sk_la_protein_gradients call ran: bit 0 the code kernel,
 * bit 1 the profile kernel (0 after a refused call). */
int sk_last_la_protein_grad(const sk_context *ctx, uint32_t *mask);

/* Gradients of the DAG stem kernels with respect to their own parameters, the
 * step an optimizer of loop_gap, beta, stack and covar takes per pair.  The
 * per-pair function is StemKernel<ST,MData>::operator()
 * (stem_kernel_lite/stem_kernel.cpp:14-95) differentiated in forward mode:
 * every DP quantity (K0, G0, K1, G1, v_s, e_s) carries its value and one
 * tangent per parameter, the product rule applied in the DP's own operation
 * order.  The reference has no such function (stem_kernel/train.cpp calls an
 * inside_outside that was never written), so the derivative is defined as the
 * exact derivative of that DP:
 *   w[k] = w[k-1] * loop_gap        d/dloop_gap = k * w[k-1]  (0 for k = 0)
 *   gap2 = loop_gap * loop_gap      d/dloop_gap = loop_gap + loop_gap
 *   Su:  co_subst[c] = exp(P[c] * beta)       d/dbeta = P[c] * co_subst[c]
 *   Si:  stack where the pair codes are equal, covar otherwise: indicators
 * len_band, the node weights and the bp frequencies are data.
 *
 * For k < n_pairs, value[k] = K(xs[x[k]], ys[y[k]]) and grad[4k..4k+3] =
 * d/d(loop_gap, beta, stack, covar), sk_bpla_gradients' four-slot layout; the
 * slots a kind does not read are +0.0 (stack, covar for the Su kinds, beta for
 * the Si kinds).  Kinds: SK_SU_STEM, SK_SI_STEM; SK_LSU_STEM (V = beta log Ks:
 * d/dloop_gap = beta Ks'/Ks, d/dbeta = log Ks + beta (dKs/dbeta) / Ks);
 * SK_SU_STEM_STR, SK_SI_STEM_STR, SK_LSU_STEM_STR, whose value includes the
 * string term and whose gradient is the stem part's (the string term does not
 * depend on these parameters).  Gradients with respect to the string
 * parameters (gap, alpha, match, mismatch) are not computed.  Under the log
 * kinds a pair with Ks = 0 has the value sk_pairs returns (-inf) and NaN in
 * the loop_gap and beta slots.
 *
 * Errors, all before any launch: SK_ERR_INVALID for any other kind or an
 * example built with use_bp = 0, SK_ERR_RANGE for an index outside its
 * dataset and, on the GPU only, SK_ERR_UNSUPPORTED for a pair whose per-wave
 * scratch does not fit the call's budget (half of the free device memory).
 * Host buffers; synchronous.
 *
 * The GPU call (csrc/kernels/stem_grad.hip) runs one wavefront per pair; it
 * sums in another order than the DP above and gives a pair the same bits
 * whatever the batch around it.  The host call restates the DP operation by
 * operation in double: its value equals the reference's bit for bit; it needs
 * no upload, and runs pairs on n_threads threads (0: all). */
int sk_stem_gradients(sk_context *ctx, sk_dataset *xs, sk_dataset *ys, const sk_kernel_params *kp,
                      const int32_t *x, const int32_t *y, int64_t n_pairs, double *value, double *grad);
int sk_stem_gradients_host(sk_dataset *xs, sk_dataset *ys, const sk_kernel_params *kp,
                           const int32_t *x, const int32_t *y, int64_t n_pairs, int32_t n_threads,
                           double *value, double *grad);
/* Kernels the last sk_stem_gradients call ran: bit 0 the Su instantiation
 * (two tangents), bit 1 the Si instantiation (three) (0 after a refused call). */
int sk_last_stem_grad(const sk_context *ctx, uint32_t *mask);

/* ---------------------------------------------------------------- example files
 * The readers DataLoader<MData>::get (stem_kernel_lite/data.cpp:547-586) pulls
 * examples from, with the reference grammars' exact acceptance (Boost.Spirit
 * classic semantics, csrc/host/readers.cpp):
 *   SK_FMT_FASTA    load_fa   common/fa.cpp:13-55    one sequence per example
 *   SK_FMT_CLUSTAL  load_aln  common/aln.cpp:16-107  one alignment per example
 *   SK_FMT_MAF      load_maf  common/maf.cpp:15-49   one alignment block per example
 * Reading stops at the first example that does not parse.  SK_ERR_INVALID on a
 * missing file, aln's format_error or rows of unequal length ("wrong
 * alignment", data.cpp:574-578); sk_seqfile_last_error() (thread-local) says
 * which.  Rows are returned as written (gaps kept, case kept). */
typedef enum { SK_FMT_FASTA = 0, SK_FMT_CLUSTAL = 1, SK_FMT_MAF = 2 } sk_file_format;
typedef struct sk_seqfile sk_seqfile;
int sk_seqfile_read(const char *path, int32_t format, sk_seqfile **out);
int sk_seqfile_parse(const char *text, size_t len, int32_t format, sk_seqfile **out);
int sk_seqfile_free(sk_seqfile *f);
int64_t sk_seqfile_count(const sk_seqfile *f);                        /* examples */
int32_t sk_seqfile_rows(const sk_seqfile *f, int64_t i);              /* rows of example i */
const char *sk_seqfile_row(const sk_seqfile *f, int64_t i, int32_t r); /* NUL-terminated */
const char *sk_seqfile_last_error(void);
/* splitmix64 sequences over ACGU: n_seqs strings of length len written to
 * out (n_seqs*(len+1) bytes, NUL separated); *state advances. */
int sk_random_sequences(uint64_t *state, int32_t n_seqs, int32_t len, char *out);

/* ---------------------------------------------------------------- SVM prediction
 * Predict mode's Output (f3) feeds every test row through the libsvm models
 * of --model / --predict: SVMPredict (libsvm/svm_util.cpp:11-95) over the
 * reference's vendored libsvm 2.8x, restated in csrc/host/svm_predict.cpp.
 *   sk_svm_model_load   svm_load_model (libsvm/svm.cpp:1288-1475): text
 *                       model, any svm_type / kernel_type (precomputed:
 *                       an SV's value is its 1-based training index);
 *                       SK_ERR_INVALID with sk_svm_last_error() on failure.
 *   sk_svm_model_info   svm_get_svm_type / svm_get_nr_class / svm_get_labels
 *                       (svm.cpp:1024-1039; labels untouched when the model
 *                       has none), and whether probA/probB are present.
 *   sk_svm_predict      SVMPredict::do_svm_predict's arithmetic
 *                       (svm_util.cpp:41-80) on the test vector
 *                       make_svm_node(cnt, row) builds (x[0] = cnt,
 *                       x[i+1] = row[i], row = the test row over the training
 *                       examples): with probability != 0 and a C-SVC / nu-SVC
 *                       model, *label = svm_predict_probability
 *                       (svm.cpp:1152-1189) and values[0..nr_class) = the
 *                       class probabilities (zeros if the model has no
 *                       probA/probB: svm_predict's label); otherwise *label =
 *                       svm_predict (svm.cpp:1108-1150) and
 *                       values[0..max(nr_class(nr_class-1)/2, 1)) = the
 *                       decision values (svm_predict_values, svm.cpp:1053-1106). */
typedef struct sk_svm_model sk_svm_model;
int sk_svm_model_load(const char *path, sk_svm_model **out);
void sk_svm_model_free(sk_svm_model *m);
int sk_svm_model_info(const sk_svm_model *m, int32_t *svm_type, int32_t *nr_class, int32_t *labels,
                      int32_t *has_probability);
int sk_svm_predict(const sk_svm_model *m, int32_t cnt, const double *row, int32_t n, int32_t probability,
                   double *label, double *values);
const char *sk_svm_last_error(void);

/* ---------------------------------------------------------------- SVM training
 * Batched two-class C-SVC training on a precomputed Gram: libsvm's SMO solver,
 * Solver::Solve (libsvm/solver.cpp:81-349) with select_working_set
 * (:352-451) and calculate_rho (:554-592), called as solve_c_svc does
 * (libsvm/svm.cpp:38-71) and as the optimizer's svm_train does
 * (optimizer/gradient.cpp:208-246): p = -1, alpha = 0, G = -1, y = +1 for a
 * label > 0 and -1 otherwise, bounds Cp (y = +1) and Cn.  What replaces
 * `svm-train -t 4` on the printed matrix and the per-fold Solve of
 * GradientComputation::compute (optimizer/gradient.cpp:107-156).  Many
 * (training subset, C) problems over one Gram are solved in one call: on the
 * GPU one workgroup per problem (csrc/kernels/svm_smo.hip), on the host one
 * thread per problem (csrc/host/svm_train.cpp).
 *
 * SHRINKING is a flag of the call (sk_svm_train_batch_ex; the calls without
 * _ex run without it).  Both modes are the reference's own runs bit for bit:
 * alphas, rho, obj and the number of updates of Solve(..., shrinking = 0) and
 * of Solve(..., shrinking = 1), the latter being what `svm-train` runs by
 * default (-h 1) and what gradient.cpp hardcodes (:224).  The two runs end
 * within the same stopping tolerance but not at the same bits (int300 C = 1
 * of tests/golden: 719 updates against 706, rho differs by 4e-4 relative;
 * DESIGN.md).
 *   Without: the active set is always the whole problem and no index is
 *   swapped, so the sequence of working pairs is a function of the inputs.
 *   With: every min(l, 1000) updates do_shrinking (solver.cpp:475-552) moves
 *   the variables at a bound whose gradient rules them out to the tail of a
 *   permuted problem (swap_index, :47-57) and the selection, the G update and
 *   rho run over the active prefix (:368, :393, :272, :561).  G_bar (:279-306)
 *   follows every upper-bound flip over all l positions, i before j;
 *   reconstruct_gradient (:61-79) rebuilds the inactive G[j] from G_bar[j] +
 *   p[j] plus alpha_i Q_i[j] over the free active positions i in ascending
 *   position order, two roundings per term; the unshrink branch runs once,
 *   when Gmax1 + Gmax2 <= 10 eps, on the reconstructed gradient with the Gmax
 *   values from before; an optimal selection on a shrunk set reconstructs,
 *   restores the whole set and selects again (:154-165).  The sums of rho and
 *   obj, and the last-index rule of the selection, follow the permuted
 *   positions (:309-327); the alphas go back through active_set.
 *
 * Arithmetic kept from the reference:
 *   Q_i[k] = (float)(y_i y_k K[t_i][t_k]), QD[k] = (float)K[t_k][t_k]
 *   (SVC_Q, libsvm/qmatrix.cpp:339-362; kernel_precomputed :331-336), t the
 *   problem's training list, K read by row only (row t_i for Q_i);
 *   working-set selection with >= and <=, so of equal candidates the last
 *   index wins (solver.cpp:368-386, :393-443); quad_coef in float arithmetic
 *   (:405, :429, :182, :225), TAU = 1e-12 when it is <= 0; the clipped
 *   two-variable update (:180-265); G[k] += Q_i[k]*da_i + Q_j[k]*da_j with
 *   four roundings and no fused multiply-add (:272-275); stop when
 *   Gmax + Gmax2 < eps (:445); rho and obj as :554-592 and :314-321.
 * One addition: max_iter, a mandatory cap on the iterations (the reference's
 * loop has none).  A problem that needs a further iteration after max_iter
 * returns its state at that point with status SK_SVM_NOT_CONVERGED; that is
 * not an error of the call.
 *
 * Decision values of a problem's test list: sum over a of (alpha_a y_a) *
 * K[s][t_a] - rho (svm_predict, optimizer/gradient.cpp:248-278); the host
 * path sums in training order over alpha_a != 0, the GPU sums in parallel. */
typedef struct {
  const int32_t *train; /* indices into the Gram, in training order */
  int32_t n_train;
  const int32_t *test;  /* examples to evaluate after the solve (may be NULL) */
  int32_t n_test;
  double Cp, Cn, eps;
  int64_t max_iter;
} sk_svm_problem;
typedef enum {
  SK_SVM_CONVERGED = 0,
  SK_SVM_NOT_CONVERGED = 1, /* max_iter reached */
  SK_SVM_NO_PAIR = 2        /* no working pair (a Gram that is not finite) */
} sk_svm_status;
typedef struct {
  double rho, obj;
  int64_t iterations;
  int32_t status;  /* sk_svm_status */
  int32_t n_free;  /* 0 < alpha < C */
  int32_t n_bound; /* alpha at its upper bound */
} sk_svm_solution;
/* gram: n x n row-major host memory as sk_gram writes it, uploaded once per
 * call; labels: n values.  alpha_out (sum of n_train; alpha >= 0, not
 * multiplied by y) and dec_out (sum of n_test; may be NULL when that is 0)
 * are concatenated in problem order; solutions has n_problems entries.
 * SK_ERR_INVALID, with nothing launched, for an index outside [0, n), a
 * training list with one class only (the reference's rho would be infinite),
 * eps <= 0, Cp <= 0 or Cn <= 0, max_iter < 1 or n_train < 2;
 * SK_ERR_UNSUPPORTED, with nothing launched, for a training list longer than
 * sk_svm_train_shape's largest.  The kernel launches are counted by
 * sk_last_launch_ms (one per size class in use). */
int sk_svm_train_batch(sk_context *ctx, const double *gram, int32_t n, const double *labels,
                       const sk_svm_problem *problems, int32_t n_problems, double *alpha_out,
                       double *dec_out, sk_svm_solution *solutions);
/* The same on n_threads host threads (0 = hardware concurrency), any n_train. */
int sk_svm_train_batch_host(const double *gram, int32_t n, const double *labels,
                            const sk_svm_problem *problems, int32_t n_problems, int32_t n_threads,
                            double *alpha_out, double *dec_out, sk_svm_solution *solutions);
/* What a solve with shrinking did, per problem.  A shrink call "shrank" when
 * it left fewer active positions than it found; the call that ran the
 * unshrink branch "regrew" the set when it left more than it found. */
typedef struct {
  int32_t shrink_calls;    /* do_shrinking() calls */
  int32_t shrunk_calls;    /* of those, calls that lowered active_size */
  int32_t min_active;      /* smallest active_size seen (n_train if none) */
  int32_t unshrunk;        /* the one-time unshrink branch ran */
  int32_t regrown;         /* ... and raised active_size */
  int32_t reconstructions; /* selections that reported optimal with active_size < l */
  int32_t resumed;         /* of those, followed by a further iteration */
} sk_svm_shrink_info;
/* sk_svm_train_batch / _host with the shrinking flag (0 or 1) and, when info
 * is not NULL, n_problems records of what the shrinking did.  shrinking = 0
 * is the call without _ex bit for bit, with min_active = n_train and zeros
 * elsewhere in info.  The same checks, errors and launch counts.  With
 * shrinking, solutions[p].iterations still counts updates, and max_iter ends
 * a solve as the reference would end at its optimum: once max_iter updates
 * have run and a further pair was found, the gradient is reconstructed, the
 * active set restored, and rho, obj and the alphas are those of that state
 * (SK_SVM_NOT_CONVERGED). */
int sk_svm_train_batch_ex(sk_context *ctx, const double *gram, int32_t n, const double *labels,
                          const sk_svm_problem *problems, int32_t n_problems, int32_t shrinking,
                          double *alpha_out, double *dec_out, sk_svm_solution *solutions,
                          sk_svm_shrink_info *info);
int sk_svm_train_batch_host_ex(const double *gram, int32_t n, const double *labels,
                               const sk_svm_problem *problems, int32_t n_problems, int32_t n_threads,
                               int32_t shrinking, double *alpha_out, double *dec_out,
                               sk_svm_solution *solutions, sk_svm_shrink_info *info);
/* Size classes of the GPU solver: class c takes n_train <= bounds[c]
 * (ascending; up to 4 written), *n_classes of them, *max_train the last. */
int sk_svm_train_shape(int32_t *bounds, int32_t *n_classes, int32_t *max_train);
/* A two-class C-SVC precomputed-kernel model in svm_save_model's text format
 * (libsvm/svm.cpp:1201-1286: rho %g, coefficients %.16g, support vectors
 * 0:serial with the 1-based serial number train[a] + 1), which
 * sk_svm_model_load reads back.  Classes in svm_group_classes' order
 * (svm.cpp:611-666: by first appearance in the training list, label (int));
 * libsvm's first class is its +1, so when the first training label is not
 * > 0 the coefficients and rho change sign.  Support vectors are the
 * alpha != 0 examples, the first class's before the second's.  SK_ERR_INVALID
 * unless the training labels have exactly two (int) values, one > 0. */
int sk_svm_model_write(const char *path, const double *labels, int32_t n, const int32_t *train,
                       int32_t n_train, const double *alpha, double rho);

/* ------------------------------------------- SVM training: the five formulations
 * svm_train_one (libsvm/svm.cpp:245-300) whole: next to C-SVC the batch
 * solves nu-SVC, one-class, epsilon-SVR and nu-SVR tasks over one Gram, what
 * `svm-train -s 1|2|3|4 -t 4` does on the printed matrix.  WITHOUT SHRINKING:
 * every task is the reference's Solve(..., shrinking = 0) bit for bit;
 * shrinking for the four new types (Solver_NU::do_shrinking included) is not
 * built, and the calls below carry no shrinking flag.
 *
 * Per type, as the reference's solve_* functions set the problem up
 * (svm.cpp:38-234), l = n_train, target_k the target of training example k:
 *   C_SVC        solve_c_svc: sk_svm_train_batch's problem with Cp = Cn = C.
 *   NU_SVC       solve_nu_svc (:73-126): y = sign of the target, p = 0,
 *                bounds 1, the start point alpha_k = min(1, sum) with sum
 *                running down from nu l / 2 per class in list order;
 *                Solver_NU; then alpha_k *= y_k / r, rho /= r, obj /= r r.
 *   ONE_CLASS    solve_one_class (:128-158): y = +1, p = 0, bounds 1, the
 *                first (int)(nu l) alphas 1, the next nu l - (int)(nu l).
 *                Targets are not read.
 *   EPSILON_SVR  solve_epsilon_svr (:160-196): 2 l positions, position k and
 *                k + l both example k with y = +1 and -1 (SVR_Q,
 *                libsvm/qmatrix.cpp:423-475, QD duplicated :438-439), linear
 *                term p - target and p + target, alpha = 0, bounds C.
 *   NU_SVR       solve_nu_svr (:198-234): the same positions, linear term
 *                -target and +target, alpha_k = alpha_{k+l} = min(sum, C) with
 *                sum running down from C nu l / 2 in list order; Solver_NU.
 * Q_i[k] = y_i y_k (float)K[t_i][t_k] over positions (the three Q classes of
 * qmatrix.cpp give this value), K read by row only.  The general Solve
 * (solver.cpp:81-349): G = p, then G[j] += alpha_i Q_i[j] for every i not at
 * its lower bound in ascending order, a multiply and an add (:113-135); obj =
 * sum alpha (G + p) / 2 (:314-321).  Solver_NU: per-class working-set
 * selection (:595-705; >= and <=, the last index wins, quad_coef in float, i
 * from the class of the chosen j, stop on max(Gmaxp + Gmaxp2, Gmaxn + Gmaxn2)
 * < eps; where the reference would index with -1 because no j exists the
 * status is SK_SVM_NO_PAIR) and the two-sided calculate_rho (:799-848), which
 * also gives r.
 *
 * coef_out (n_train per task, concatenated) is what svm_train_one leaves in
 * alpha and what goes into a model's sv_coef: alpha y (C_SVC), alpha (y / r)
 * (NU_SVC), alpha (ONE_CLASS), alpha_k - alpha_{k+l} (both SVR types).  rho
 * and obj are what leaves svm_train_one (NU_SVC: divided by r and r r); r is
 * Solver_NU's si->r as solved, 0 for the plain solver.  n_free and n_bound
 * count the solver's positions (2 l of them for SVR).  Decision values of the
 * test list: sum over coef_a != 0 of coef_a K[s][t_a], minus rho
 * (svm_predict_values, svm.cpp:1053-1070); the host path sums in list order.
 * The GPU path and the host path give the same coef, rho, obj, r, iterations,
 * status and counts, bit for bit. */
typedef enum {
  SK_SVM_C_SVC = 0,
  SK_SVM_NU_SVC = 1,
  SK_SVM_ONE_CLASS = 2,
  SK_SVM_EPSILON_SVR = 3,
  SK_SVM_NU_SVR = 4
} sk_svm_type;
typedef struct {
  const int32_t *train; /* indices into the Gram, in training order */
  int32_t n_train;
  const int32_t *test;  /* examples to evaluate after the solve (may be NULL) */
  int32_t n_test;
  int32_t svm_type;     /* sk_svm_type */
  double C;             /* C_SVC, EPSILON_SVR, NU_SVR */
  double nu;            /* NU_SVC, ONE_CLASS, NU_SVR */
  double p;             /* EPSILON_SVR */
  double eps;
  int64_t max_iter;     /* mandatory, as in sk_svm_problem */
} sk_svm_task;
typedef struct {
  double rho, obj;
  int64_t iterations;
  int32_t status;  /* sk_svm_status */
  int32_t n_free;  /* positions with 0 < alpha < bound */
  int32_t n_bound; /* positions at the upper bound */
  double r;        /* Solver_NU's si->r; 0 for C_SVC, ONE_CLASS, EPSILON_SVR */
} sk_svm_task_solution;
/* targets: n values (class labels for the classifiers, by sign; real values
 * for the SVR types; may be NULL when every task is ONE_CLASS).  Tasks of
 * different types may share a call.  SK_ERR_INVALID, with nothing launched
 * (svm_check_parameter, svm.cpp:1499-1615): an unknown svm_type; nu outside
 * (0, 1] for the three nu types; NU_SVC with nu (n+ + n-) / 2 > min(n+, n-)
 * (:1563-1610) or a classifier with one class only; C <= 0 where C is used;
 * p < 0 for EPSILON_SVR; eps <= 0; max_iter < 1; n_train < 2; an index outside
 * [0, n); an SVR target that is not finite.  SK_ERR_UNSUPPORTED, with nothing
 * launched: a training list longer than sk_svm_solve_shape reports for its
 * type (the GPU call only).  One kernel launch per (solver family, size class)
 * in use, the families being C_SVC, the plain general solver (ONE_CLASS,
 * EPSILON_SVR) and Solver_NU (NU_SVC, NU_SVR). */
int sk_svm_solve_batch(sk_context *ctx, const double *gram, int32_t n, const double *targets,
                       const sk_svm_task *tasks, int32_t n_tasks, double *coef_out, double *dec_out,
                       sk_svm_task_solution *solutions);
int sk_svm_solve_batch_host(const double *gram, int32_t n, const double *targets, const sk_svm_task *tasks,
                            int32_t n_tasks, int32_t n_threads, double *coef_out, double *dec_out,
                            sk_svm_task_solution *solutions);
/* max_train[t], t an sk_svm_type (5 entries): the longest training list the
 * GPU solver takes.  sk_svm_train_shape's max_train for C_SVC, NU_SVC and
 * ONE_CLASS; half of it for the SVR types, whose 2 l positions share the
 * kernel's position capacity (size classes go by positions). */
int sk_svm_solve_shape(int32_t *max_train);
/* svm_save_model's text (svm.cpp:1201-1286) for any svm_type, from coef as
 * sk_svm_solve_batch returns it; sk_svm_model_load reads it back.  C_SVC and
 * NU_SVC: as sk_svm_model_write (classes by first appearance, signs turned
 * when the first training label is not > 0).  ONE_CLASS and the SVR types:
 * nr_class 2, no label and nr_sv lines, the support vectors where
 * fabs(coef) > 0 in list order (svm.cpp:677-717); targets may be NULL. */
int sk_svm_model_write_ex(const char *path, int32_t svm_type, const double *targets, int32_t n,
                          const int32_t *train, int32_t n_train, const double *coef, double rho);

/* ------------------------------------------------- cross-validated AUC gradient
 * Steps 3 to 5 of GradientComputation::compute (optimizer/gradient.cpp:107-156)
 * for many (fold, C) problems over one Gram K and its derivative matrices
 * G[p] = dK/d(parameter p): from a trained fold (alpha, rho: sk_svm_train_batch)
 * and the smoothed AUC's weights delta of its held-out examples, the gradient
 * of that AUC with respect to C (cg) and to every kernel parameter (fg[p]).
 * On the GPU one workgroup per problem (csrc/kernels/auc_grad.hip), on the
 * host one thread per problem (csrc/host/auc_gradient.cpp).
 *
 * Arithmetic kept from the reference (y_k = +1 for a label > 0, else -1; a
 * label 0 is refused; u = the free examples 0 < alpha < C and c = the bound
 * ones alpha >= C, both in training order: find_support_vectors,
 * gradient.cpp:368-403; ts = the test list; every sum starts at 0 and adds
 * its terms in ascending index, as uBLAS's prod and inner_prod do; no fused
 * multiply-add):
 *   solve_d (gradient.cpp:405-456), n_free > 0 only:
 *     P(i,j) = (y_i y_j) K[u_i][u_j], P(i,n_free) = P(n_free,i) = -y_i,
 *     P(n_free,n_free) = 0; r(i) = sum_j (delta_j y_i) K[u_i][ts_j],
 *     r(n_free) = 0 - delta_0 - delta_1 ...; K is read by row only.
 *     d_u = conjugate_gradient(P, r) from 0 (gradient.cpp:622-644): the early
 *     return when r.r < 1e-10, at most n_free + 1 passes, no guard on w.z (a
 *     division by zero propagates inf / NaN to the outputs, as it does there).
 *   calculate_gradient_c (gradient.cpp:511-547):
 *     q(i) = 0 - sum_j (y_i y_j) K[u_i][c_j], q(n_free) = sum_j y_{c_j};
 *     cg = (0 + d_u.q) + sum_i sum_j (delta_i y_{c_j}) K[ts_i][c_j], one chain.
 *   calculate_gradient_p (gradient.cpp:549-620), g = G[p]:
 *     q(i) = 0 - sum_j ((y_i y_j) g[u_i][c_j]) C, q(n_free) = 0;
 *     v = prod(P', beta_u), P'(i,j) = (y_i y_j) g[u_i][u_j] with a zero border,
 *     beta_u = (alpha_u, rho); dpsi(j) = sum_i (delta_i y_j) g[ts_i][t_j];
 *     fg[p] = (0 + d_u.(q - v)) + (dpsi, 0).(alpha, rho).
 * The conjugate gradient on this indefinite system amplifies rounding (a
 * reordered free set moves cg and fg by 1e-5 to 1e-2 relative: DESIGN.md 16),
 * so both paths keep the order above and agree bit for bit.
 *
 * sk_auc_delta is compute_delta (gradient.cpp:159-206): f = the smoothed AUC
 * of dec over the (positive, negative) pairs of the test list, positives
 * outer, negatives inner, and delta = df/d(dec); here a label >= 0 counts as
 * positive, as it does there.  Host only, for both paths: it goes through
 * libm's exp.  A test list with one class only gives f = 0 and delta = 0. */
int sk_auc_delta(const double *dec, const double *labels_of_test, int32_t n_test, double *delta_out,
                 double *f_out);
typedef struct {
  const int32_t *train; /* as sk_svm_problem */
  int32_t n_train;
  const int32_t *test;
  int32_t n_test;
  double C;            /* one C: find_support_vectors has one */
  const double *alpha; /* n_train, in training order, >= 0 */
  double rho;
  const double *delta; /* n_test */
} sk_auc_problem;
typedef struct {
  int32_t n_free, n_bound;
  int32_t cg_iterations; /* products P w the conjugate gradient formed (0: early return or n_free = 0) */
  int32_t finite;        /* 0 when cg, an fg or a d_u entry is inf or NaN */
} sk_auc_info;
/* gram: n x n row-major; grads: n_params matrices of n x n (may be NULL when
 * n_params is 0: then only cg is returned); labels: n values.  cg_out has
 * n_problems entries, fg_out n_problems * n_params (problem-major), info
 * n_problems.  d_u_out may be NULL; otherwise problem p's slot starts at
 * sum over q < p of (n_train_q + 1) and receives its n_free + 1 entries of
 * d_u when n_free > 0 (nothing otherwise; the rest of the slot is not
 * written).  SK_ERR_INVALID, with nothing launched, for an index outside
 * [0, n), a label 0 among a problem's examples, C <= 0, n_test < 1,
 * n_train < 2, an alpha or delta that is not finite (or alpha < 0), or
 * n_params < 0; SK_ERR_UNSUPPORTED, with nothing launched, when a problem
 * has more free examples than sk_auc_gradient_shape's max_free (its P would
 * not fit its share of the scratch).  The kernel launches are counted by
 * sk_last_launch_ms. */
int sk_auc_gradient_batch(sk_context *ctx, const double *gram, const double *grads, int32_t n_params,
                          int32_t n, const double *labels, const sk_auc_problem *problems,
                          int32_t n_problems, double *cg_out, double *fg_out, double *d_u_out,
                          sk_auc_info *info);
/* The same on n_threads host threads (0 = hardware concurrency), any n_free. */
int sk_auc_gradient_batch_host(const double *gram, const double *grads, int32_t n_params, int32_t n,
                               const double *labels, const sk_auc_problem *problems, int32_t n_problems,
                               int32_t n_threads, double *cg_out, double *fg_out, double *d_u_out,
                               sk_auc_info *info);
/* The GPU path's shape: n_free <= *lds_free keeps P in LDS, more keeps it in
 * a device scratch of 8 (n_free + 1)^2 bytes; *max_free is the most one
 * problem may have; the problems of one launch share *scratch_budget bytes. */
int sk_auc_gradient_shape(int32_t *lds_free, int32_t *max_free, int64_t *scratch_budget);

/* ---------------------------------------------------------------- feature-vector Grams */
/* The reference's rbf_optimizer, poly_optimizer and sigmoid_optimizer
 * (Optimizer<RBFKernel|PolyKernel|SigmoidKernel, GradientComputationAUC>) read
 * a libsvm feature file and need a Gram K and its derivative matrices
 * dK/dparam at every step (CM::calculate_matrix, optimizer/rbf_kernel.cpp,
 * poly_kernel.cpp, sigmoid_kernel.cpp).  With d = dot(x, y), libsvm's sparse
 * merge (sum = 0; sum += x.value * y.value over the shared indices in
 * ascending order; multiply and add rounded separately):
 *   SK_FEAT_RBF      params (gamma):        w = dot(x,x) + dot(y,y) - 2 d;
 *                    K = exp(-gamma w); G0 = -w exp(-gamma w)
 *   SK_FEAT_POLY     params (gamma, coef0), integer degree: t = gamma d + coef0;
 *                    K = powi(t, degree); v = powi(t, degree - 1) degree;
 *                    G0 = v d; G1 = v   (powi: libsvm's square-and-multiply)
 *   SK_FEAT_SIGMOID  params (gamma, coef0): t = gamma d + coef0; K = tanh(t);
 *                    w = cosh(t); v = 1 / (w w); G0 = v d; G1 = v
 * The dot matrix is the reference's bit for bit on both paths; so is the whole
 * polynomial kernel; exp / tanh / cosh are libm's on the host path and the
 * device library's on the GPU (within the project's 1e-6 relative bound;
 * DESIGN.md 17 has the measured deviation in ulps). */
typedef struct sk_features sk_features;
typedef enum sk_feature_kernel { SK_FEAT_RBF = 0, SK_FEAT_POLY = 1, SK_FEAT_SIGMOID = 2 } sk_feature_kernel;
/* A feature set from CSR arrays: example i holds index[row_ptr[i] ..
 * row_ptr[i+1]) with their values; row_ptr[0] = 0; labels may be NULL (all
 * 0).  The arrays are copied.  SK_ERR_INVALID for an index < 0, indices not
 * strictly ascending within an example, or a value that is not finite
 * (message: sk_features_last_error). */
int sk_features_create(int32_t n, const int64_t *row_ptr, const int32_t *index, const double *value,
                       const int32_t *labels, sk_features **out);
/* From libsvm text, as the reference's read_data reads it
 * (optimizer/rbf_kernel.cpp:69-104): one example per line, the label atoi of
 * the first token, every further token index:value; a blank line is an example
 * with label 0 and no features.  Stricter than read_data, whose terminator is
 * index -1 and which does not check its sscanf: a token without ':', an index
 * that is not an integer or is < 0, indices not strictly ascending within a
 * line, a value that is not a number or not finite are SK_ERR_INVALID, with a
 * message that begins "line N:". */
int sk_features_parse(const char *text, size_t len, sk_features **out);
int sk_features_read(const char *path, sk_features **out);
/* Also drops the dot matrices any context keeps resident for the set. */
int sk_features_free(sk_features *fs);
/* *n examples, *d used columns (distinct indices), *nnz stored entries. */
int sk_features_shape(const sk_features *fs, int32_t *n, int32_t *d, int64_t *nnz);
int sk_features_labels(const sk_features *fs, int32_t *out);
/* The examples back as CSR: row_ptr n + 1, index and value nnz entries (each
 * may be NULL). */
int sk_features_rows(const sk_features *fs, int64_t *row_ptr, int32_t *index, double *value);
/* The last error of an sk_features_* or sk_feature_*_host call on this thread. */
const char *sk_features_last_error(void);
/* The GPU path's shape and the limits of both paths: the dot kernel computes
 * *tile x *tile outputs per workgroup in k-slices of *k_slice columns.  A set
 * may hold at most *max_n examples (16,384: the resident dot matrix, K and two
 * gradient matrices are 4 n^2 doubles on the device, 8 GiB), and the examples
 * of a call (both sets of a cross call) times the used columns (of their
 * union) at most *max_dense entries (2^28: the examples are stored dense over
 * the compacted columns, 2 GiB).  Over a limit: SK_ERR_UNSUPPORTED before
 * anything is launched, with the limit named in the message. */
int sk_feature_gram_shape(int32_t *tile, int32_t *k_slice, int32_t *max_n, int64_t *max_dense);
/* The dot matrix D[i][j] = dot(xs_i, ys_j) (ys NULL: xs with itself, n x n;
 * otherwise n_xs x n_ys over the union of both sets' columns), downloaded.
 * The context computes D on the first call for the set (or the pair) and
 * keeps it resident on its device until the set is freed or the context is
 * closed (the four most recent per context); the calls below use the same D,
 * so a call with new parameters launches only the epilogue kernel
 * (sk_last_launch_ms counts every kernel launched). */
int sk_feature_dots(sk_context *ctx, const sk_features *xs, const sk_features *ys, double *out);
int sk_feature_dots_host(const sk_features *xs, const sk_features *ys, int32_t n_threads, double *out);
/* K (n x n) and, unless out_g is NULL, the derivative matrices G[P][n][n] (P =
 * 1 for RBF, 2 otherwise: the layout sk_auc_gradient_batch takes), exactly
 * symmetric.  degree is read for SK_FEAT_POLY only (>= 0). */
int sk_feature_gram(sk_context *ctx, const sk_features *xs, int32_t kind, int32_t degree, const double *params,
                    double *out_k, double *out_g);
/* The same on n_threads host threads (0 = hardware concurrency) with libm:
 * what the GPU path is compared with. */
int sk_feature_gram_host(const sk_features *xs, int32_t kind, int32_t degree, const double *params,
                         int32_t n_threads, double *out_k, double *out_g);
/* The rectangular K(test, train), n_test x n_train, for predicting with a
 * model trained at the optimum. */
int sk_feature_gram_cross(sk_context *ctx, const sk_features *test, const sk_features *train, int32_t kind,
                          int32_t degree, const double *params, double *out_k);
int sk_feature_gram_cross_host(const sk_features *test, const sk_features *train, int32_t kind, int32_t degree,
                               const double *params, int32_t n_threads, double *out_k);

/* ---------------------------------------------------------------- diagnostics */
/* Milliseconds spent in the last compute call's dominant kernel (DAG stem
 * DP), measured with HIP events on the context's stream, and its launch
 * count.  Algorithmic work of that launch: *cells = sum |Vx|*|Vy| over the
 * pairs (non-leaf nodes). */
int sk_last_timing(const sk_context *ctx, double *stem_ms, double *string_ms,
                   double *cells, int32_t *launches);
/* Summed durations of the last compute call's dominant-kernel launches (DAG
 * stem, 4-D stem or BPLA), each timed by HIP events around it on its own
 * stream, and their count: *ms_sum / *n_launches is the average launch
 * duration a kernel-trace profiler reports.  Launches on several streams
 * overlap, so the sum can exceed sk_last_timing's span.  The DAG stem
 * launches' shared Gamma tables are built by kernels of their own ahead of
 * all launches (0.5 ms of a 4.7 s step); these are in the span, not here. */
int sk_last_launch_ms(const sk_context *ctx, double *ms_sum, int32_t *n_launches);
/* Asynchronous compute calls (default off).  With on != 0, sk_pairs_device
 * (and every call that returns its results on the device) returns once its
 * work is enqueued on the context's stream, so the host plans call t+1
 * while the GPU runs call t; host inputs are staged through pinned buffers,
 * so they may be freed when the call returns.  Results are ready after a
 * stream synchronisation.  The timing queries above then report totals:
 * sk_sync_timing waits for every call since the previous sk_sync_timing and
 * makes their summed timings (spans, launches, cells) what sk_last_timing and
 * sk_last_launch_ms return.  Turning async off resolves what is pending. */
int sk_set_async(sk_context *ctx, int32_t on);
int sk_sync_timing(sk_context *ctx);
/* Kernel instantiations launched by the last compute call (parity-coverage
 * diagnostic): *stem_maxk_mask has bit MAXK/4 set for every DAG stem register
 * class run (MAXK = 4, 8, ..., 32 64-node slots per lane; bit 17 for the MAXK 17
 * class, y examples of 1,025-1,088 non-leaf nodes) and bit 0 when the
 * big-y kernel ran (y examples of 2,048 non-leaf nodes or more, or with a stem edge
 * gap over 1,023, which the register classes cannot hold); *stem4d_mask has
 * bit log2(CPL) set for every 4-D stem class run (CPL = 1, 2, 4, 8 cells per
 * lane), shifted by 4 for the banded (partial_dp) variant and by 8 for the
 * column-pipelined full_dp kernel. */
int sk_last_classes(const sk_context *ctx, uint32_t *stem_maxk_mask, uint32_t *stem4d_mask);
/* Protein local-alignment kernels the last compute call launched
 * (csrc/kernels/la_protein.hip): bit 0 the code kernel (pairs of examples
 * whose every column holds one residue kind), bit 1 the profile kernel. */
int sk_last_la_protein(const sk_context *ctx, uint32_t *mask);
/* Profile string kernels the last compute call launched
 * (csrc/kernels/profile_string.hip), in the order one-hot fast kernel, dyadic
 * fast kernel, general kernel (the naive mode runs on the general kernel):
 * pairs[k] the number of pairs kernel k took, waves[k] the waves per workgroup
 * of its launch (0: not launched).  All zero after a call without a string
 * part. */
int sk_last_string(const sk_context *ctx, int64_t pairs[3], int32_t waves[3]);
/* The number of DAG stem class launches of the last compute call that read one
 * Gamma table per y example, built by a table kernel ahead of the launch and
 * shared by every workgroup on that y (0 for a null context).  The other
 * launches -- x sets without gamma keys, classes without a gapless y, tables
 * beyond the memory budget -- build a table per workgroup and work item
 * (diagnostic: which path ran). */
int32_t sk_last_gamma_shared(const sk_context *ctx);
/* Shape the column-pipelined 4-D kernel takes for a full_dp Gram batch whose
 * x and y examples have lengths [min_len, max_len]: *nb chained columns per
 * group, *waves waves per pair, *pf rows fetched ahead per wave (diagnostic;
 * bench roofline).  *waves = 0 when that batch does not run on the column
 * kernel: max_len >= 512 (k-tiled span kernel), max_len over the column
 * kernel's x limit (2,048), or min_len too short for the column schedule. */
int sk_stem4d_col_shape(int32_t min_len, int32_t max_len, int32_t *nb, int32_t *waves, int32_t *pf);
/* RIBOSUM85-60 tables as compiled into the library (pinning tests). */
void sk_ribosum_tables(float *s16, float *p256);
int sk_char2rna(int c);
/* 1 in the experiments build (make exp: build/libstem_kernel_amd_exp.so, which
 * reads the A/B switches INTEGRATION.md lists from the environment), 0 in the
 * shipped library (no switches compiled in). */
int sk_experiments(void);

#ifdef __cplusplus
}
#endif
#endif /* STEM_KERNEL_H */
