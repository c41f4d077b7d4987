/*
 * pipelinedp_amd.h — C ABI of the MI355X (gfx950) DPEngine.aggregate hot path.
 *
 * The reference (lagodiuk/PipelineDP 0.2.2rc2) is pure Python and has no C ABI;
 * every entry point below replaces one stage of the reference's LocalBackend
 * execution of DPEngine._aggregate (pipeline_dp/dp_engine.py:109-187).  The
 * citation above each function names the reference code it replaces.
 *
 * Conventions
 *  - Every function returns 0 on success and a negative PDP_E_* code on
 *    failure; pdp_last_error() returns a thread-local message.  No C++
 *    exception crosses this boundary.
 *  - All array arguments are DEVICE pointers owned by the caller (allocated by
 *    hipMalloc or by torch-ROCm).  `stream` is a hipStream_t passed as void*;
 *    NULL means the legacy default stream.  Nothing here synchronises the
 *    stream or allocates memory, so the sequence can be captured in a hipGraph.
 *  - Keys are dense: privacy ids in [0, n_privacy_ids), partition keys in
 *    [0, n_partitions).  The Python host layer dictionary-encodes other keys.
 */
#ifndef PIPELINEDP_AMD_H_
#define PIPELINEDP_AMD_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PDP_ABI_VERSION 21

/* error codes */
#define PDP_OK 0
#define PDP_E_INVALID (-1)   /* bad argument / shape */
#define PDP_E_HIP (-2)       /* a HIP runtime call failed */
#define PDP_E_WORKSPACE (-3) /* workspace too small */
#define PDP_E_UNSUPPORTED (-4)

/* value column kinds */
#define PDP_VALUE_NONE 0
#define PDP_VALUE_F64 1
#define PDP_VALUE_I64 2

/* accumulator flags (pdp_bound_config.flags) */
#define PDP_ACC_SUM 0x1            /* SumCombiner: sum of clipped values */
#define PDP_ACC_NSUM 0x2           /* Mean/Variance: sum of (clip(v) - middle) */
#define PDP_ACC_NSUM2 0x4          /* Variance: sum of (clip(v) - middle)^2 */
#define PDP_SUM_PER_PARTITION 0x8  /* SumCombiner bounds_per_partition: clip(sum_pair) */
#define PDP_SUM_INT 0x10           /* SUM accumulator is int64 (int values, int bounds) */
#define PDP_PROBE_LEVEL1 0x20000000 /* placement probe: pdp_bound_contributions runs the partition pass's
                                      level 1 only (its output is not a bounding result); the API layer
                                      times it on candidate workspaces (executor.py, placement probe) */
#define PDP_DEBUG_CORRUPT_RECORDS 0x40000000 /* tests only: overwrite the level-2 records of buckets 0
                                                and 1 with an out-of-range partition / row before the
                                                bucket kernel, which must flag them in the error word
                                                (pdp_bound_error_flags) instead of reading out of bounds;
                                                rejected (PDP_E_INVALID) unless the environment has
                                                PIPELINEDP_AMD_TEST_HOOKS=1 */

/* One shard's contribution-bounding configuration. */
typedef struct pdp_bound_config {
  int64_t n_rows;        /* rows in this shard (< 2^32) */
  int64_t n_privacy_ids; /* U: privacy ids are dense in [0, U) */
  int64_t n_partitions;  /* P: partition keys are dense in [0, P) (< 2^32) */
  int32_t l0;            /* max_partitions_contributed (1..PDP_MAX_L0); 0 = no
                            cross-partition bounding (LinfSampler / NoOpSampler) */
  int32_t linf;          /* max_contributions_per_partition (1..PDP_MAX_LINF); 0 = keep all rows */
  int32_t value_kind;    /* PDP_VALUE_* */
  int32_t flags;         /* PDP_ACC_* | PDP_SUM_* */
  double min_value;      /* per-value clipping bounds (SUM/MEAN/VARIANCE) */
  double max_value;
  double middle;         /* min_value + (max_value - min_value) / 2 */
  double min_sum;        /* per-partition SUM bounds (PDP_SUM_PER_PARTITION) */
  double max_sum;
  int64_t row_offset;    /* global index of this shard's row 0 (row priorities) */
  uint64_t seed;         /* sampling seed */
  int32_t algorithm;     /* PDP_ALGO_*; every algorithm keeps the same samples */
  int32_t merge;         /* PDP_MERGE_*: how BUCKETED merges kept pairs per partition */
  int32_t max_contributions; /* > 0: SamplingPerPrivacyIdContributionBounder — keep a
                                uniform sample of <= this many rows per privacy id
                                (1..PDP_MAX_CONTRIBUTIONS); needs l0 = linf = 0 */
  int32_t rows_are_units;    /* != 0: contribution_bounds_already_enforced — every row is
                                its own accumulator; privacy_id may be NULL */
  int32_t key_format;        /* PDP_KEYS_*: row record format of the BUCKETED partition passes */
  int32_t sieve;             /* BUCKETED threshold sieve (identical results): 0 = auto, < 0 = off,
                                1..32768 = keep rows whose 32-bit pair hash is below sieve * 2^16
                                (candidate fraction t = sieve / 2^16 <= 1/2) through the partition
                                passes; privacy ids with < l0 candidate pairs are finished from a
                                side band or a re-read of the privacy-id column */
  int32_t sieve_band;        /* with the sieve, the side band: level 1 also lists the rows whose pair
                                hash is in [t, 2t), and the fix-up reads that list; only ids with
                                < l0 pairs below 2t re-read the privacy-id column.  0 = auto (on
                                for t <= 1/4), > 0 = on, < 0 = off (identical results) */
  int32_t sieve_threads;     /* the sieve's level-1 workgroup (identical results): 0 = auto (1024),
                                1024, or 512 (two per CU, when its LDS fits) */
  int32_t bucket_threads;    /* the bucket kernel's workgroup (identical results): 0 = auto (1024),
                                1024, or 512 (buckets of half as many privacy ids, whose LDS lets two
                                workgroups share a CU; needs <= 512 partition ranges) */
} pdp_bound_config;

/* bounds up to int32; above 256 (l0, linf) the pair-table algorithm runs, and
 * a cap above 256 is applied by radix select instead of a sorted sketch */
#define PDP_MAX_L0 2147483647
#define PDP_MAX_LINF 2147483647
#define PDP_MAX_CONTRIBUTIONS 2147483647

/* bounding algorithms (identical results, different data movement) */
#define PDP_ALGO_AUTO 0
#define PDP_ALGO_GLOBAL_SKETCH 1 /* per-pid / per-pair sketches in HBM, device atomics */
#define PDP_ALGO_BUCKETED 2      /* rows partitioned by pid bucket, sketches in LDS */
#define PDP_ALGO_PAIR_TABLE 3    /* device hash table of (pid, pk) pairs: the bounders
                                    without cross-partition sampling (l0 = 0,
                                    max_contributions, rows_are_units), and any bounder
                                    with l0 or linf > 256 (L0 over the table's distinct
                                    pairs, the GLOBAL path's pair keys); chosen by AUTO */

/* row records moved by the BUCKETED partition passes (identical results) */
#define PDP_KEYS_AUTO 0
#define PDP_KEYS_WIDE 1    /* u64 record (bit 63 dead | bucket-within-super and bucket-local
                              pid | partition) + u32 row: 12 B per row and pass; any
                              partition count (pair keys are rebuilt in the bucket kernel) */
#define PDP_KEYS_COMPACT 2 /* u32 (bucket-local pid, partition) + u32 row: 8 B per row and pass;
                              needs super/bucket/partition bits <= 31 (AUTO picks it then) */
#define PDP_KEYS_PACKED 3  /* level 1: one u64 (row within its 65,536-row tile | bucket-local pid |
                              partition), the tile known from the stage block it was read from;
                              level 2 on: the COMPACT pair.  8 B per row and pass: needs bucket +
                              partition bits <= 31 and super + bucket + partition bits <= 47
                              (AUTO's first choice with the tile-local level 1) */
#define PDP_KEYS_PACKED64 5 /* level 1 PACKED (8 B), level 2 on one u64 per record (row << (bucket + partition
                              bits) | bucket-local pid << partition bits | partition; all ones = dead): 8 B
                              per record and pass with no row array, where the bucket + partition bits
                              exceed 31 (C4/C5: P = 1e7) but rows < 2^(64 - bucket - partition bits) - 2 and
                              super + bucket + partition bits <= 47; tile-local level 1 only (AUTO picks it
                              there before PACKED_WIDE) */
#define PDP_KEYS_PACKED_WIDE 4 /* level 1 PACKED (8 B), level 2 on WIDE (u64 key + u32 row):
                              partition counts whose bucket + partition bits exceed 31 (C4/C5:
                              P = 1e7) with super + bucket + partition bits <= 47; tile-local
                              level 1 only (AUTO picks it there before WIDE) */

/* per-partition merge of the kept pairs (BUCKETED; identical sums up to fp
 * summation order) */
#define PDP_MERGE_AUTO 0
#define PDP_MERGE_ATOMIC 1 /* one device atomic per kept pair and field */
#define PDP_MERGE_RANGES 2 /* pair records grouped by partition range, LDS reduction */

typedef struct pdp_bound_plan_info {
  int32_t algorithm;   /* resolved PDP_ALGO_* */
  int32_t bucket_bits; /* privacy ids per bucket = 2^bucket_bits */
  int32_t rand_shift;  /* pair sampling key: random bits [rand_shift, 64) */
  int32_t pk_bits;     /* partition bits [0, pk_bits) */
  int64_t n_buckets;
  int64_t n_tiles;
  int64_t lds_bytes;   /* per bucket workgroup */
  int32_t merge;       /* resolved PDP_MERGE_* (0 for GLOBAL_SKETCH) */
  int32_t n_ranges;    /* PDP_MERGE_RANGES: partition ranges of 2^11 keys */
  int64_t range_group; /* PDP_MERGE_RANGES: records per range-reduce work item */
  int32_t key_format;  /* resolved PDP_KEYS_* (BUCKETED) */
  int32_t sieve;       /* resolved threshold sieve, t = sieve / 2^16 (0 = off) */
  int32_t band;        /* resolved side band, t2 = band / 2^16 (0 = off) */
  int32_t sieve_threads; /* resolved sieve level-1 workgroup size (0 without the sieve) */
  int32_t bucket_threads; /* resolved bucket-kernel workgroup size (BUCKETED) */
  int32_t hist_u16;    /* tile-local level 1 keeps its per-tile bucket counts as u16 halves */
  int32_t fix_ids;     /* sieve fix-up: 1 = one wave per unresolved privacy id (l0 * (1 + linf) <= 32,
                          linf > 0), 0 = fix-up bucket launches */
} pdp_bound_plan_info;

/* Resolves the execution plan for `cfg` (no device work). */
int pdp_bound_plan(const pdp_bound_config* cfg, pdp_bound_plan_info* info);

/* Per-partition accumulators, dense arrays of length n_partitions.  They are
 * the columnar form of CompoundCombiner's accumulator (combiners.py:749-764):
 * row_count, then the children's accumulators. */
typedef struct pdp_partition_accumulators {
  int64_t* privacy_id_count; /* kept (privacy_id, partition) pairs = row_count */
  int64_t* count;            /* CountCombiner / Mean / Variance count */
  void* sum;                 /* SumCombiner: double, or int64 with PDP_SUM_INT */
  double* normalized_sum;    /* Mean/Variance: sum(clip(v) - middle) */
  double* normalized_sum_sq; /* Variance: sum((clip(v) - middle)^2) */
} pdp_partition_accumulators;

int pdp_abi_version(void);
const char* pdp_last_error(void);

/* Bytes of device workspace pdp_bound_contributions needs for `cfg`. */
int pdp_bound_workspace_bytes(const pdp_bound_config* cfg, uint64_t* bytes);

/* Contribution bounding: per privacy id keep at most l0 distinct partitions,
 * per (privacy id, partition) keep at most linf rows, both uniform samples
 * without replacement drawn with counter-based hash priorities.
 * Replaces SamplingCrossAndPerPartitionContributionBounder.bound_contributions
 * (contribution_bounders.py:72-111) and, with linf = 0,
 * SamplingCrossPartitionContributionBounder (contribution_bounders.py:168-201),
 * i.e. LocalBackend.sample_fixed_per_key (pipeline_backend.py:531-547) twice.
 * With l0 = 0: LinfSampler (linf > 0, :204-230) or NoOpSampler (linf = 0,
 * :233-246); with max_contributions: SamplingPerPrivacyIdContributionBounder
 * (:114-156); with rows_are_units: DPEngine's contribution_bounds_already_enforced
 * branch ("Wrap values into accumulators", dp_engine.py:143-150).
 * `pk_allowed` (nullable, u8[n_partitions]) drops rows of non-public
 * partitions first (DPEngine._drop_partitions, dp_engine.py:290-296).
 * The workspace is fully (re)initialised on `stream` by this call.  With
 * PDP_MERGE_RANGES (the default) the whole sampling runs here and leaves
 * per-pair records in the workspace; with PDP_MERGE_ATOMIC the per-bucket
 * sampling runs in pdp_reduce_partitions. */
int pdp_bound_contributions(const pdp_bound_config* cfg, const int64_t* privacy_id,
                            const int64_t* partition_key, const void* value,
                            const uint8_t* pk_allowed, void* workspace,
                            uint64_t workspace_bytes, void* stream);

/* Per-pair accumulators (CompoundCombiner.create_accumulator on the sampled
 * values, combiners.py:749-753) merged per partition key
 * (LocalBackend.combine_accumulators_per_key, pipeline_backend.py:555-565).
 * Must follow pdp_bound_contributions on the same workspace and stream
 * (BUCKETED + PDP_MERGE_ATOMIC: the per-bucket sampling itself runs here).
 * `acc` arrays are ADDED to (zero them first, or chain shards). */
int pdp_reduce_partitions(const pdp_bound_config* cfg, const void* value,
                          void* workspace, uint64_t workspace_bytes,
                          const pdp_partition_accumulators* acc, void* stream);

/* Noise of one additive mechanism, the granularity-snapped secure samplers of
 * Google's differential-privacy library that PyDP wraps (python-dp ~=1.1.5rc4,
 * numerical_mechanisms.LaplaceMechanism / GaussianMechanism, called at
 * dp_computations.py:439-440, 489-491; restated, not vendored):
 *   out = round_to_multiple(x, granularity) + granularity * k,
 * k a two-sided geometric sample P(k) ~ exp(-lambda |k|) (Laplace, found by an
 * integer bisection whose every step is a Bernoulli with the exact conditional
 * mass), or a centred Binomial(n, 1/2) sample drawn by geometric-proposal
 * rejection (Gaussian).  Outputs lie on the power-of-two grid, so their low
 * bits carry no information about x (the floating-point attack of Mironov
 * 2012 on textbook samplers).  The host computes every field
 * (pipelinedp_amd/dp_computations.py: laplace_noise_params /
 * gaussian_noise_params); granularity = 0 means no noise. */
#define PDP_NOISE_LAPLACE 0
#define PDP_NOISE_GAUSSIAN 1

typedef struct pdp_noise_params {
  int32_t kind;        /* PDP_NOISE_* */
  int32_t reserved;
  double scale;        /* Laplace b = sensitivity / eps, Gaussian sigma (reporting) */
  double granularity;  /* output grid, a power of two; 0 = no noise */
  double lambda;       /* Laplace: granularity * eps / (sensitivity + granularity) */
  int64_t step;        /* Gaussian: round(sqrt(2) * sqrt_n + 1), sqrt_n = 2 sigma / granularity */
  double n;            /* Gaussian: sqrt_n^2 (binomial trials) */
  double bound;        /* Gaussian: sqrt_n * sqrt(log(n) / 2), |m| above it has probability 0 */
  double coef;         /* Gaussian: sqrt(2 / pi) / sqrt_n */
  double corr;         /* Gaussian: 1 - 0.4 * (2 log n)^1.5 / sqrt_n */
} pdp_noise_params;

/* partition selection strategies */
#define PDP_SELECT_ALL_NONEMPTY 0 /* keep every partition with row_count > 0 */
#define PDP_SELECT_TRUNCATED_GEOMETRIC 1
#define PDP_SELECT_LAPLACE_THRESHOLDING 2
#define PDP_SELECT_GAUSSIAN_THRESHOLDING 3
#define PDP_SELECT_PUBLIC 4       /* keep partitions with public_mask[p] != 0 */

typedef struct pdp_select_config {
  int64_t n_partitions;          /* length of the slice */
  int64_t partition_offset;      /* global index of slice element 0 (RNG counter) */
  int32_t strategy;              /* PDP_SELECT_* */
  int32_t max_rows_per_privacy_id; /* n = ceil(row_count / this), dp_engine.py:346-353 */
  int32_t pre_threshold;         /* 0 = none */
  int32_t keep_table_len;        /* truncated geometric: keep_prob[0..len-1] */
  const double* keep_prob;       /* device; prob of keep for n; n >= len uses [len-1] */
  pdp_noise_params noise;        /* thresholding strategies: the secure mechanism */
  double threshold;              /* thresholding strategies */
  const uint8_t* public_mask;    /* PDP_SELECT_PUBLIC */
  uint64_t seed;
} pdp_select_config;

/* Private partition selection (dp_engine.py:315-371 → PyDP
 * create_partition_strategy(...).should_keep / noised_value_if_should_keep,
 * partition_selection.py:29-44).  Writes keep[p] in {0,1}; if `noised_count`
 * is non-NULL the thresholding strategies also write the noised
 * privacy-unit count (PostAggregationThresholdingCombiner, combiners.py:353-357). */
int pdp_select_partitions(const pdp_select_config* cfg, const int64_t* row_count,
                          uint8_t* keep, double* noised_count, void* stream);

/* Stream compaction of keep flags into ascending partition indices.
 * `out_count` (device int64[1]) receives the number kept.  Workspace bytes:
 * pdp_compact_workspace_bytes. */
int pdp_compact_workspace_bytes(int64_t n, uint64_t* bytes);
int pdp_compact(const uint8_t* keep, int64_t n, int64_t* out_index, int64_t* out_count,
                void* workspace, uint64_t workspace_bytes, void* stream);

/* metric operations (one per combiner in CompoundCombiner order) */
#define PDP_OP_COUNT 1            /* CountCombiner.compute_metrics, combiners.py:262-263 */
#define PDP_OP_SUM 2              /* SumCombiner, combiners.py:416-417 */
#define PDP_OP_PRIVACY_ID_COUNT 3 /* PrivacyIdCountCombiner, combiners.py:304-305 */
#define PDP_OP_MEAN 4             /* MeanCombiner + MeanMechanism, dp_computations.py:562-568 */
#define PDP_OP_VARIANCE 5         /* VarianceCombiner + compute_dp_var, dp_computations.py:306-365 */
#define PDP_OP_THRESHOLDED_PID 6  /* PostAggregationThresholdingCombiner: copy noised_count */

typedef struct pdp_metric_op {
  int32_t kind;        /* PDP_OP_* */
  int32_t degenerate;  /* VARIANCE: min_value == max_value */
  int32_t out_col[4];  /* output column for each produced metric, -1 = not produced.
                          COUNT/SUM/PID: [0]; MEAN: mean,count,sum;
                          VARIANCE: variance,count,sum,mean */
  pdp_noise_params noise[3]; /* per mechanism: COUNT/SUM/PID: [0]; MEAN: count,nsum;
                                VARIANCE: count,nsum,nsum2 */
  double middle;       /* MEAN/VARIANCE: middle of [min_value, max_value] */
  double min_value;    /* VARIANCE: for min_value == max_value shortcut */
  double sq_min_value; /* VARIANCE: lower end of the squares interval */
} pdp_metric_op;

#define PDP_MAX_OPS 8

/* Noise + compute_metrics for the kept partitions (CompoundCombiner.
 * compute_metrics, combiners.py:766-788).  For each i < n_kept with
 * p = index[i]: out[col * out_stride + i] = metric value (double).
 * `n_kept_dev` (device int64[1], nullable) bounds i on device when n_kept is
 * only known on device; pass n_kept = capacity then. */
int pdp_noise_metrics(const pdp_metric_op* ops, int32_t n_ops, const int64_t* index,
                      int64_t n_kept, const int64_t* n_kept_dev, int64_t partition_offset,
                      const pdp_partition_accumulators* acc, int32_t sum_is_int,
                      const double* noised_count, double* out, int64_t out_stride,
                      uint64_t seed, void* stream);

/* VECTOR_SUM (VectorSumCombiner, combiners.py:800-847): one double[vector_size]
 * per row, summed per partition over the rows the bounder keeps (no per-row
 * clipping); the partition's total is clipped and noised per coordinate by
 * pdp_vector_sum_metrics.  vector_size in [1, PDP_MAX_VECTOR_SIZE]. */
#define PDP_MAX_VECTOR_SIZE 4096

/* NormKind (aggregate_params.py NormKind; dp_computations._clip_vector :197-209) */
#define PDP_NORM_LINF 0 /* clip(v, -max_norm, max_norm) per coordinate */
#define PDP_NORM_L1 1   /* v * min(1, max_norm / sum |v_j|) */
#define PDP_NORM_L2 2   /* v * min(1, max_norm / sqrt(sum v_j^2)) */

/* Philox stream slot of the vector-sum noise.  pdp_noise_metrics uses the slots
 * (op << 4) | mechanism < 0x80 and pdp_add_noise 0x41444E00; this one ("VECS")
 * collides with neither, so a vector sum noised with the seed of the scalar
 * metrics still draws independent noise. */
#define PDP_VECTOR_SUM_SLOT 0x56454353

/* Bytes of device workspace for pdp_bound_contributions followed by
 * pdp_reduce_vector_sum: the pair table's workspace (pdp_bound_workspace_bytes)
 * plus the kept-row list (8 B per row), the per-partition counts and offsets
 * and the partial sums of long partitions. */
int pdp_vector_sum_workspace_bytes(const pdp_bound_config* cfg, int32_t vector_size, uint64_t* bytes);

/* VectorSumCombiner.create_accumulator per kept pair, merged per partition
 * (combiners.py:809-830): vector_acc[p][j] += the sum over the kept rows i of
 * partition p of vectors[i][j].  vectors: row-major double[n_rows][vector_size];
 * vector_acc: row-major double[n_partitions][vector_size], ADDED to.
 * Must follow pdp_bound_contributions on the same workspace (of at least
 * pdp_vector_sum_workspace_bytes) and stream, with the same key columns and
 * pk_allowed, and a cfg that resolves to PDP_ALGO_PAIR_TABLE (any other plan:
 * PDP_E_UNSUPPORTED); cfg->value_kind may be PDP_VALUE_NONE.  A row is kept
 * iff the pair table kept it: keys in range and partition allowed, among its
 * privacy id's max_contributions rows, its pair among the id's l0 pairs, and
 * the row among its pair's linf rows (rows_are_units: every valid allowed
 * row).  Out-of-range keys set bit 0 of the error word and are skipped.  The
 * kept rows are counting-sorted by partition (no value traffic) and summed by
 * waves whose lanes run across coordinates; a partition with many rows is
 * split over waves and its partial sums are combined by a second kernel, so
 * no floating-point atomic is used.  Sums may depend on the floating-point
 * summation order (as with PDP_MERGE_RANGES), on nothing else. */
int pdp_reduce_vector_sum(const pdp_bound_config* cfg, const int64_t* privacy_id, const int64_t* partition_key,
                          const uint8_t* pk_allowed, const double* vectors, int32_t vector_size, void* workspace,
                          uint64_t workspace_bytes, double* vector_acc, void* stream);

/* VectorSumCombiner.compute_metrics (combiners.py:832-838 ->
 * dp_computations.add_noise_vector :212-229) for the kept partitions: for each
 * i < n_kept with p = index[i], vector_acc[p] is clipped by `norm_kind`
 * (PDP_NORM_*; an all-zero vector has coefficient 1, never NaN) and
 *   out[i * vector_size + j] = noise(clipped[j]),
 * the secure mechanism `noise` (host pointer; granularity 0 = clip only) on
 * the Philox streams (seed, (partition_offset + p) * vector_size + j,
 * PDP_VECTOR_SUM_SLOT).  n_kept_dev as in pdp_noise_metrics. */
int pdp_vector_sum_metrics(const double* vector_acc, int32_t vector_size, int32_t norm_kind, double max_norm,
                           const pdp_noise_params* noise, const int64_t* index, int64_t n_kept,
                           const int64_t* n_kept_dev, int64_t partition_offset, double* out, uint64_t seed,
                           void* stream);

/* PERCENTILE (QuantileCombiner, combiners.py:590-669): one quantile tree per
 * partition over [min_value, max_value], height 4, branching factor 16.  The
 * reference delegates the tree to PyDP's QuantileTree; the algorithm these
 * entry points run is restated in DESIGN.md section 3 ("PERCENTILE") and was
 * not compared against PyDP output.  Node 0 is the root (never counted), the
 * children of node i are 16 i + 1 ... 16 i + 16, the 65,536 leaves are the
 * nodes from 4,369 on, and a partition has 69,904 counted nodes.
 *
 * A value's leaf is min(65535, floor((clamp(v) - min_value) / (max_value -
 * min_value) * 65536)) in fp64, clamp(v) to [min_value, max_value]; a NaN
 * value takes no part.  A node's raw count is the number of kept rows whose
 * leaf lies in its leaf range, so the tree of a partition is held as the
 * ascending array of its kept rows' 16-bit leaf codes. */
#define PDP_MAX_QUANTILES 64

/* Philox stream slot of the quantile trees' noise ("QNTL"): none of the slots
 * listed at PDP_VECTOR_SUM_SLOT, nor that one. */
#define PDP_QUANTILE_SLOT 0x514E544C

/* Bytes of device workspace for pdp_bound_contributions followed by
 * pdp_reduce_quantile_leaves: the pair table's workspace, the kept-row marks
 * and per-partition counts, and the leaf sort's key columns (16 B per row). */
int pdp_quantile_workspace_bytes(const pdp_bound_config* cfg, uint64_t* bytes);

/* QuantileCombiner.create_accumulator per kept pair, merged per partition
 * (combiners.py:608-620), in columnar form: leaves[offsets[p] .. offsets[p + 1])
 * = the ascending leaf codes of the rows of partition p the bounder keeps,
 * exactly the rows pdp_reduce_vector_sum would sum, less those whose value is
 * NaN.  value: n_rows doubles (PDP_VALUE_F64) or int64 (PDP_VALUE_I64).
 * leaves: device uint16[n_rows] (only the first offsets[n_partitions] are
 * written); offsets: device uint32[n_partitions + 1].  Both are overwritten.
 * The preconditions are pdp_reduce_vector_sum's: it must follow
 * pdp_bound_contributions on the same workspace (of at least
 * pdp_quantile_workspace_bytes) and stream, with the same cfg, key columns and
 * pk_allowed, and cfg must resolve to PDP_ALGO_PAIR_TABLE (any other plan:
 * PDP_E_UNSUPPORTED); out-of-range keys set bit 0 of the error word and are
 * skipped.  n_rows < 2^31, n_partitions < 2^31 - 1.  The kept rows are marked
 * and counted per partition as for VECTOR_SUM, and the (leaf, partition) keys
 * are ordered by the stable tile sort, 8 bits a pass, leaf digits first: two
 * runs give the same bytes. */
int pdp_reduce_quantile_leaves(const pdp_bound_config* cfg, const int64_t* privacy_id, const int64_t* partition_key,
                               const uint8_t* pk_allowed, const void* value, int32_t value_kind, double min_value,
                               double max_value, void* workspace, uint64_t workspace_bytes, uint16_t* leaves,
                               uint32_t* offsets, void* stream);

/* Most runs pdp_merge_quantile_leaves merges per partition: one per source
 * rank of a process group (the project's multi-GPU scope is 8 ranks). */
#define PDP_MAX_QUANTILE_RUNS 64

/* Bytes of device workspace for pdp_merge_quantile_leaves: the run-major scan
 * of the counts (4 B per run and partition) and a scan's chunk sums.
 * n_runs outside [1, PDP_MAX_QUANTILE_RUNS]: PDP_E_UNSUPPORTED. */
int pdp_quantile_merge_workspace_bytes(int32_t n_runs, int64_t n_partitions, uint64_t* bytes);

/* QuantileCombiner.merge_accumulators (combiners.py:614-620) across the ranks
 * of a process group, in columnar form: the owner of n_partitions partitions
 * holds n_runs leaf arrays of the layout pdp_reduce_quantile_leaves writes,
 * one per source rank, and gets one.  runs: device uint16[n_leaves], the
 * arrays concatenated run-major, then partition-major; run s holds, for each
 * partition p, run_counts[s * n_partitions + p] ascending codes (run_counts:
 * device uint32[n_runs * n_partitions]).  n_leaves (host) is their total,
 * n_leaves < 2^31; n_runs * n_partitions < 2^31.  On return
 *   offsets[p] = the exclusive scan over p of sum_s run_counts[s][p], the
 *     total in offsets[n_partitions] (device uint32[n_partitions + 1]);
 *   leaves[offsets[p] .. offsets[p + 1]) = the ascending merge of the n_runs
 *     runs of p (device uint16[n_leaves]; must not alias runs).
 * Element j of run s of partition p, with code x, goes to offsets[p] + j + the
 * number of codes <= x in the runs before s + the number of codes < x in the
 * runs after s: a permutation, so every slot has one writer, there is no
 * atomic, and two calls give the same bytes.  One thread per element and
 * n_runs - 1 binary searches each.  1 <= n_runs <= PDP_MAX_QUANTILE_RUNS
 * (else PDP_E_UNSUPPORTED); a workspace below
 * pdp_quantile_merge_workspace_bytes returns PDP_E_WORKSPACE; both before
 * any launch.  Nothing synchronises or allocates.  Every read of runs and
 * every store to leaves is bounded by n_leaves on the device: counts whose sum
 * is not n_leaves leave part of leaves unwritten or drop elements, and write
 * nothing out of bounds.  n_leaves == 0 writes offsets only (runs and leaves
 * may be NULL). */
int pdp_merge_quantile_leaves(const uint16_t* runs, int64_t n_leaves, const uint32_t* run_counts, int32_t n_runs,
                              int64_t n_partitions, void* workspace, uint64_t workspace_bytes, uint16_t* leaves,
                              uint32_t* offsets, void* stream);

/* QuantileCombiner.compute_metrics (combiners.py:622-633 ->
 * QuantileTree.compute_quantiles) for the kept partitions: for each i < n_kept
 * with p = index[i] and each j < n_ranks,
 *   out[i * n_ranks + j] = the value at rank ranks[j] of partition p's tree.
 * ranks: HOST array of n_ranks values in [0, 1], 1 <= n_ranks <=
 * PDP_MAX_QUANTILES.  A node's noised count is max(0, noise(raw count)), the
 * secure mechanism `noise` (host pointer; granularity 0 = no noise) on the
 * Philox stream (seed, (partition_offset + p) * 69904 + node - 1,
 * PDP_QUANTILE_SLOT): one value per node, whichever rank asks for it.  The
 * walk from the root takes, four times, the first child whose share of the
 * children's noised total reaches the rank (less 1e-6), rescales the rank into
 * that child and narrows [min_value, max_value] to its sixteenth; it stops
 * early where the children's total is not positive, and returns
 * (1 - rank) * a + rank * b on the range [a, b] it reached.  A partition
 * without rows walks on noise alone (no noise: (1 - rank) * min_value + rank *
 * max_value).  One wave per partition, 16 lanes (children) per rank, four
 * ranks a round; every fp64 operation is rounded on its own (no contraction),
 * in the order DESIGN.md states.  n_kept_dev as in pdp_noise_metrics. */
int pdp_quantile_metrics(const uint16_t* leaves, const uint32_t* offsets, int64_t n_partitions, double min_value,
                         double max_value, const double* ranks, int32_t n_ranks, const pdp_noise_params* noise,
                         const int64_t* index, int64_t n_kept, const int64_t* n_kept_dev, int64_t partition_offset,
                         double* out, uint64_t seed, void* stream);

/* DPEngine.add_dp_noise (dp_engine.py:551-607): out[i] = the secure
 * mechanism `noise` applied to (double)values[i], the `lambda value:
 * create_mechanism().add_noise(float(value))` of its "Add noise" map_values
 * stage (dp_engine.py:595-599) over a column.  values: n int64
 * (PDP_VALUE_I64) or fp64 (PDP_VALUE_F64); `noise` (host pointer): Laplace
 * (l1 = l0*linf, dp_computations.py:430-477) or Gaussian (:480-537).
 * Element i draws from the Philox4x32-10 streams (seed, index_offset + i), so
 * shards of one column noised with their global offsets equal the unsharded
 * result.  values and out: device, 16-byte aligned; out may alias values when
 * both are fp64. */
int pdp_add_noise(const void* values, int32_t value_kind, int64_t n, const pdp_noise_params* noise,
                  uint64_t seed, int64_t index_offset, double* out, void* stream);

/* Device error word: the bounding kernels set bit 0 when a key is outside
 * [0, n_privacy_ids) x [0, n_partitions) (the row is skipped, never read out
 * of bounds), bit 1 if the sieve's fix-up row list would outgrow its
 * workspace region (cannot happen: each list holds distinct rows; checked
 * rather than assumed).  Reads it from the workspace of pdp_bound_contributions
 * (synchronises `stream`). */
int pdp_bound_error_flags(const void* workspace, uint32_t* flags, void* stream);

/* The same error word, copied to `flags` by a copy enqueued on `stream`
 * (nothing synchronises; `flags` should be pinned host memory, valid until the
 * stream has passed the copy).  The library's API layer reads it once the
 * aggregate's result is materialised, so the key check costs no pipeline
 * drain between bounding and the merge. */
int pdp_bound_error_flags_async(const void* workspace, uint32_t* flags, void* stream);

/* What the last pdp_bound_contributions (BUCKETED) moved, read from its
 * workspace (synchronises `stream`): rows that entered the partition passes
 * (every live row, or the sieve's candidates), privacy ids the sieve left
 * unresolved and the rows of those ids its fix-up gathered (from the side
 * band's list and the candidates, or the re-read), the band's rows, the ids
 * the band left unresolved and their re-read rows.  Diagnostics for
 * the measurement (bench.py's algorithmic bytes); zeros for other
 * algorithms. */
typedef struct pdp_bound_stats {
  int64_t rows_partitioned;
  int64_t unresolved_ids;
  int64_t fixup_rows;
  int32_t sieve;        /* resolved sieve (pdp_bound_plan_info.sieve) */
  uint32_t error_flags; /* pdp_bound_error_flags */
  int64_t band_rows;    /* side band: rows level 1 listed (t <= pair hash < t2) */
  int64_t unresolved2_ids; /* side band: ids still unresolved after it (< l0 pairs below t2) */
  int64_t fixup2_rows;  /* their rows, from the re-read of the privacy-id column */
  int32_t band;         /* resolved side band (pdp_bound_plan_info.band) */
  int32_t reserved;
} pdp_bound_stats;

int pdp_bound_stats_read(const pdp_bound_config* cfg, const void* workspace, uint64_t workspace_bytes,
                         pdp_bound_stats* out, void* stream);

/* The sieve's fix-up counters of the last pdp_bound_contributions, copied
 * to out[0..3] = {unresolved ids, fix-up rows, ids the side band left
 * unresolved, their re-read rows} by copies enqueued on `stream` (nothing
 * synchronises; `out` should be pinned host memory, valid until the stream
 * has passed the copies).  Entries a plan has no counter for (no sieve, no
 * band) are set to 0 before returning.  The library's own plan choice uses
 * it: a table whose fix-up needed the whole-column re-read for many ids runs
 * unsieved on the next call (pipelinedp_amd/executor.py, plan feedback). */
int pdp_bound_stats_async(const pdp_bound_config* cfg, const void* workspace, uint64_t workspace_bytes,
                          uint32_t* out, void* stream);

/* Dataset histograms: compute_dataset_histograms
 * (pipeline_dp/dataset_histograms/computing_histograms.py:456-513) over one
 * shard of dense columns privacy_id in [0, n_privacy_ids), partition in
 * [0, n_partitions) and an optional value column (PDP_VALUE_NONE: sums 0).
 * Integer histograms (logarithmic bins, _to_bin_lower_upper_logarithmic
 * :28-47) are indexed densely: index b < 1000 is the bin [b, b + 1); index
 * b >= 1000 is lower = q * 10^e with e = (b - 1000) / 900 + 1,
 * q = (b - 1000) % 900 + 100, upper = lower + 10^e.  Their order in the
 * int_* arrays: L0, L1, LINF, COUNT_PER_PARTITION, PRIVACY_ID_PER_PARTITION
 * (HistogramType, histograms.py:60-76).  Float histograms (LINF_SUM,
 * SUM_PER_PARTITION) have PDP_HIST_SUM_BUCKETS bins over np.linspace(min,
 * max, PDP_HIST_SUM_BUCKETS + 1) (_min_max_lowers :346-370); bin i is
 * [lowers[i], lowers[i + 1]]; float_n_lowers is PDP_HIST_SUM_BUCKETS + 1, 2
 * when min == max (one bin [min, min]), 0 when empty.  A bin with count 0 is
 * absent from the reference's histogram.  All outputs are device arrays the
 * library zeroes and fills on `stream`; out-of-range keys set the error word
 * that pdp_bound_error_flags reads from this workspace.  n_rows < 2^31.
 * Up to ~1e8 rows the (privacy id, partition) pairs are found by hashing rows
 * into buckets, one LDS table per bucket: first by privacy id (every pid's
 * statistics complete in one workgroup), and if a bucket's distinct pairs do
 * not fit (privacy ids with thousands of partitions) by (pid, pk) pair; the
 * call reads one word back after each attempt (it synchronizes `stream`) and
 * redoes the pairs on an HBM pair table if both overflowed (never for hashed
 * real data).  Larger shards use the HBM pair table directly.  value_kind |
 * PDP_HIST_FORCE_PAIR_TABLE (tests) forces the pair table, value_kind |
 * PDP_HIST_FORCE_PAIR_HASH (tests) skips the privacy-id buckets. */
#define PDP_HIST_FORCE_PAIR_TABLE 0x100
#define PDP_HIST_FORCE_PAIR_HASH 0x200
#define PDP_HIST_LOG_BINS 16384
#define PDP_HIST_SUM_BUCKETS 10000
#define PDP_HIST_N_INT 5
#define PDP_HIST_N_FLOAT 2

typedef struct pdp_histogram_bins {
  int64_t* int_count;      /* [PDP_HIST_N_INT][PDP_HIST_LOG_BINS] */
  int64_t* int_sum;        /* [PDP_HIST_N_INT][PDP_HIST_LOG_BINS] */
  int64_t* int_max;        /* [PDP_HIST_N_INT][PDP_HIST_LOG_BINS] */
  int64_t* float_count;    /* [PDP_HIST_N_FLOAT][PDP_HIST_SUM_BUCKETS] */
  double* float_sum;       /* [PDP_HIST_N_FLOAT][PDP_HIST_SUM_BUCKETS] */
  double* float_max;       /* [PDP_HIST_N_FLOAT][PDP_HIST_SUM_BUCKETS] */
  double* float_lowers;    /* [PDP_HIST_N_FLOAT][PDP_HIST_SUM_BUCKETS + 1] */
  int32_t* float_n_lowers; /* [PDP_HIST_N_FLOAT] */
} pdp_histogram_bins;

int pdp_dataset_histograms_workspace_bytes(int64_t n_rows, int64_t n_privacy_ids, int64_t n_partitions,
                                           uint64_t* bytes);
int pdp_dataset_histograms(const int64_t* privacy_id, const int64_t* partition, const void* value,
                           int32_t value_kind, int64_t n_rows, int64_t n_privacy_ids, int64_t n_partitions,
                           const pdp_histogram_bins* out, void* workspace, uint64_t workspace_bytes,
                           void* stream);

/* The same computation in two phases, for rows sharded by privacy id over
 * ranks (pipelinedp_amd.executor.dataset_histograms with torch.distributed).
 * _pairs zeroes `out` and builds the pair table, the per-pid and
 * per-partition statistics and the Linf histogram.  Between the phases the
 * caller reduces across ranks, at the byte offsets that _exchange_offsets
 * gives into the workspace: the per-partition counters (uint64[n_partitions],
 * sum), the per-partition value sums (double[n_partitions], sum), and the
 * pair-sum minimum / maximum (two order-preserving uint64 words at
 * minmax + 0 / + 8: min / max as unsigned integers).  _finish then builds
 * the remaining histograms; partition_histograms = 0 skips the three
 * per-partition histograms (so that one rank owns them).  The bins of all
 * ranks are then merged: counts and sums added, maxima by maximum (only
 * over bins with a count), lowers taken from any rank (pair histogram) or
 * from the rank with partition_histograms = 1. */
int pdp_dataset_histograms_pairs(const int64_t* privacy_id, const int64_t* partition, const void* value,
                                 int32_t value_kind, int64_t n_rows, int64_t n_privacy_ids, int64_t n_partitions,
                                 const pdp_histogram_bins* out, void* workspace, uint64_t workspace_bytes,
                                 void* stream);
int pdp_dataset_histograms_exchange_offsets(int64_t n_rows, int64_t n_privacy_ids, int64_t n_partitions,
                                            uint64_t* pkstat, uint64_t* psum, uint64_t* minmax);
int pdp_dataset_histograms_finish(int32_t value_kind, int64_t n_rows, int64_t n_privacy_ids, int64_t n_partitions,
                                  int32_t partition_histograms, const pdp_histogram_bins* out, void* workspace,
                                  uint64_t workspace_bytes, void* stream);

/* Dataset histograms of pre-aggregated rows:
 * compute_dataset_histograms_on_preaggregated_data
 * (pipeline_dp/dataset_histograms/computing_histograms.py:713-758).  One row
 * per (privacy id, partition) pair, as analysis/pre_aggregation.py:19-58
 * emits them: partition in [0, n_partitions), count (rows of the pair, >= 1),
 * sum (their value sum), n_partitions_of_pid and n_contributions_of_pid (the
 * pair's privacy id's distinct partitions and rows, >= 1); all < 2^62.  The
 * bins are those of pdp_dataset_histograms, except L0 / L1, which weigh every
 * row by 1 / n_partitions_of_pid and count, per distinct value v of
 * n_partitions_of_pid (L0) or n_contributions_of_pid (L1), the weight sum
 * rounded half to even (_compute_weighted_frequency_histogram :81-102): such a
 * bin can hold count 0 with max v, and it is present in the reference's
 * histogram (present bins: count > 0 or max > 0).  Error word bit 0: partition
 * out of range; bit 1: count / n_partitions / n_contributions outside
 * [1, 2^62).  n_rows < 2^31.  The two-phase form mirrors
 * pdp_dataset_histograms_pairs / _finish for rows of one privacy id on one
 * rank: between _rows and _finish the caller sums pk_rows and pk_count
 * (uint64[n_partitions]) and psum (double[n_partitions]) over ranks and takes
 * min / max of the two minmax words, at the offsets _exchange_offsets gives.
 * The L0 / L1 weight sums must be global before they are rounded: between
 * _rows and _finish the caller sums the dense weights (double[2][1000] at
 * _weight_offsets' wsmall: values below 1000) over ranks and keeps them on one
 * rank (zeros elsewhere), takes every live entry of the weight table
 * ({uint64 key, double weight}[wtab_slots] at wtab, key 0 = empty) out of it
 * (zeroing the table), sums the entries per key over ranks, and after _finish
 * adds each key's global sum once with pdp_dataset_histograms_weight_bins. */
int pdp_dataset_histograms_preaggregated_workspace_bytes(int64_t n_rows, int64_t n_partitions, uint64_t* bytes);
int pdp_dataset_histograms_preaggregated(const int64_t* partition, const int64_t* count, const double* sum,
                                         const int64_t* n_partitions_of_pid, const int64_t* n_contributions_of_pid,
                                         int64_t n_rows, int64_t n_partitions, const pdp_histogram_bins* out,
                                         void* workspace, uint64_t workspace_bytes, void* stream);
int pdp_dataset_histograms_preaggregated_rows(const int64_t* partition, const int64_t* count, const double* sum,
                                              const int64_t* n_partitions_of_pid,
                                              const int64_t* n_contributions_of_pid, int64_t n_rows,
                                              int64_t n_partitions, const pdp_histogram_bins* out, void* workspace,
                                              uint64_t workspace_bytes, void* stream);
int pdp_dataset_histograms_preaggregated_exchange_offsets(int64_t n_rows, int64_t n_partitions, uint64_t* pk_rows,
                                                          uint64_t* pk_count, uint64_t* psum, uint64_t* minmax);
int pdp_dataset_histograms_preaggregated_weight_offsets(int64_t n_rows, int64_t n_partitions, uint64_t* wsmall,
                                                        uint64_t* wtab, uint64_t* wtab_slots);
int pdp_dataset_histograms_preaggregated_finish(const double* sum, int64_t n_rows, int64_t n_partitions,
                                                int32_t partition_histograms, const pdp_histogram_bins* out,
                                                void* workspace, uint64_t workspace_bytes, void* stream);
/* Adds n weight-table entries (keys as in the table above: value * 2 +
 * histogram + 1, histogram 0 = L0, 1 = L1; key 0 skipped) to the integer bins:
 * int(round(weight)) elements of the value, half to even; the bin's max is the
 * value even at count 0.  Device arrays; asynchronous on `stream`. */
int pdp_dataset_histograms_weight_bins(const uint64_t* keys, const double* weights, int64_t n,
                                       const pdp_histogram_bins* out, void* stream);

/* Private contribution bounds: the device steps of
 * DPEngine.calculate_private_contribution_bounds (pipeline_dp/dp_engine.py:
 * 450-502), around pdp_dataset_histograms.
 *
 * pdp_filter_rows is DPEngine._drop_partitions (dp_engine.py:417-423) on
 * dense columns: the rows with allowed[partition[i]] != 0 are written to
 * out_privacy_id / out_partition (device int64[n_rows] each, they may not
 * alias the inputs) and their number to *out_count (device int64).  One pass
 * over the 16 B/row; each 2,048-row tile reserves its output range with one
 * integer atomic, so rows keep their order within a tile but the tiles' order
 * in the output is not stable from call to call.  allowed: device
 * uint8[n_partitions].  A partition outside [0, n_partitions) sets bit 0 of
 * the error word at the start of `workspace` (pdp_bound_error_flags); the row
 * is dropped and the mask is not read for it.  Workspace bytes:
 * pdp_filter_rows_workspace_bytes. */
int pdp_filter_rows_workspace_bytes(int64_t n_rows, uint64_t* bytes);
int pdp_filter_rows(const int64_t* privacy_id, const int64_t* partition, const uint8_t* allowed, int64_t n_rows,
                    int64_t n_partitions, int64_t* out_privacy_id, int64_t* out_partition, int64_t* out_count,
                    void* workspace, uint64_t workspace_bytes, void* stream);

/* L0ScoringFunction._l0_impact_dropped (private_contribution_bounds.py:
 * 164-176) for n_candidates bounds at once:
 *   dropped[c] = sum over bins b of max(min(lower(b), upper_bound) - candidates[c], 0) * l0_count[b]
 * l0_count: the L0 row of pdp_histogram_bins.int_count (device
 * int64[PDP_HIST_LOG_BINS], lower(b) as described at pdp_dataset_histograms);
 * candidates (>= 0; a negative one counts as 0) and dropped: device
 * int64[n_candidates].  Integer arithmetic, exact while the sum fits: it is
 * at most (sum of l0_count) * upper_bound, the histogram's counts sum to less
 * than 2^31 (pdp_dataset_histograms: n_rows < 2^31), so upper_bound <= 2^32
 * keeps it below 2^63; a larger upper_bound returns PDP_E_UNSUPPORTED. */
int pdp_l0_impact_dropped(const int64_t* l0_count, int64_t upper_bound, const int64_t* candidates,
                          int64_t n_candidates, int64_t* dropped, void* stream);

/* Utility analysis, the per-partition stage: what the reference's
 * UtilityAnalysisEngine.analyze yields per partition
 * (analysis/per_partition_combiners.py:193-356, CompoundCombiner.compute_metrics)
 * for n_configurations parameter sets in one pass over the data.  Input: one
 * row per (privacy id, partition) pair, as analysis/pre_aggregation.py emits
 * them: partition in [0, n_partitions), count and sum of the pair's rows, and
 * n_partitions_of_pid, the pair's privacy id's distinct partitions (all device
 * arrays; sum may be NULL without PDP_UA_SUM).  With public partitions the
 * reference adds one pair (0, 0, 0) to EVERY public partition
 * (dp_engine.py:298-313 with CompoundCombiner.create_accumulator(()) :383-388):
 * the caller appends those rows, and sets PDP_UA_PUBLIC, which skips the
 * selection probability.
 *
 * Per pair and configuration k, q = min(1, l0_k / n_partitions_of_pid), 0 when
 * that is <= 0; a metric's value x (SUM: sum, bounds [min_sum_k, max_sum_k];
 * COUNT: count, [0, linf_k]; PRIVACY_ID_COUNT: 1[count > 0], [0, 1]) gives
 * c = clip(x), and the partition's sums of x, (c - x)[x < lo], (c - x)[x > hi],
 * -c (1 - q) and c^2 q (1 - q) (SumCombiner.create_accumulator :244-269).
 *
 * Outputs (device, caller-owned, row-major, configuration index fastest so
 * that a wave's 64 lanes = 64 configurations store 512 contiguous bytes):
 *   raw_statistics   int64[n_partitions][2]: pairs of the partition, sum of count
 *   keep_probability double[n_partitions][K] (NULL with PDP_UA_PUBLIC)
 *   metrics          double[M][5][n_partitions][K], M = requested metrics in
 *                    SUM, COUNT, PRIVACY_ID_COUNT order; the 5 fields are
 *                    SumMetrics' sum, clipping_to_min_error,
 *                    clipping_to_max_error, expected_l0_bounding_error,
 *                    std_l0_bounding_error (the square root of the fifth sum).
 * A partition without pairs gets zeros and keep table entry 0.
 *
 * keep_probability: PartitionSelectionCalculator.compute_probability_to_keep
 * (:122-151).  A partition of n <= 100 pairs: the exact Poisson-binomial PMF of
 * its q's (poisson_binomial.compute_pmf); n > 100: the refined normal
 * approximation from sum q, sum q(1-q), sum q(1-q)(1-2q)
 * (compute_pmf_approximation, its sigma == 0 branch and mean +- 8 sigma window
 * included).  Either PMF is dotted with configuration k's keep table,
 * keep_tables[keep_offsets[k] .. keep_offsets[k + 1]) (device doubles;
 * keep_offsets: HOST int64[K + 1], keep_offsets[0] = 0): entry i is the
 * strategy's probability_of_keep(i), tabulated by the host until it is exactly
 * 1.0; entries past the end count as 1.0.  A table of more than
 * PDP_UA_MAX_KEEP_TABLE entries is refused (PDP_E_UNSUPPORTED).
 *
 * params: HOST array of n_configurations entries; it and keep_offsets are
 * copied to the workspace by host-to-device copies enqueued on `stream`.
 * Nothing else synchronises.  No floating-point atomic is used and every
 * summation order is fixed: two calls on the same input give the same bits.
 * A partition code outside [0, n_partitions) sets bit 0 of the error word at
 * the start of the workspace (pdp_bound_error_flags) and the pair is skipped.
 * n_pairs, n_partitions < 2^31.  The workspace (256-byte aligned) holds the
 * sorted pair columns (40 B per pair) and, without PDP_UA_PUBLIC, the three
 * moments (24 B per partition and configuration). */
#define PDP_MAX_CONFIGURATIONS 1024
#define PDP_UA_MAX_KEEP_TABLE 1048576
#define PDP_UA_SUM 0x1
#define PDP_UA_COUNT 0x2
#define PDP_UA_PRIVACY_ID_COUNT 0x4
#define PDP_UA_PUBLIC 0x8 /* public partitions: no selection probability */

typedef struct pdp_ua_config_params {
  int64_t l0;     /* max_partitions_contributed (>= 1) */
  int64_t linf;   /* max_contributions_per_partition (COUNT) */
  double min_sum; /* min_sum_per_partition (SUM) */
  double max_sum; /* max_sum_per_partition (SUM) */
} pdp_ua_config_params;

typedef struct pdp_ua_outputs {
  int64_t* raw_statistics;
  double* keep_probability;
  double* metrics;
} pdp_ua_outputs;

int pdp_utility_analysis_workspace_bytes(int64_t n_pairs, int64_t n_partitions, int32_t n_configurations,
                                         int32_t flags, uint64_t* bytes);
int pdp_utility_analysis(const int64_t* partition, const int64_t* count, const double* sum,
                         const int64_t* n_partitions_of_pid, int64_t n_pairs, int64_t n_partitions,
                         const pdp_ua_config_params* params, int32_t n_configurations, const double* keep_tables,
                         const int64_t* keep_offsets, int32_t flags, const pdp_ua_outputs* out, void* workspace,
                         uint64_t workspace_bytes, void* stream);

/* Utility analysis, the cross-partition stage: what the reference's
 * perform_utility_analysis (analysis/utility_analysis.py, with
 * analysis/cross_partition_combiners.py) folds the per-partition output into:
 * one report per configuration over all partitions, and one per bucket of
 * partition size.  Inputs are the device outputs of pdp_utility_analysis over
 * all n_partitions codes (keep_probability NULL with PDP_UA_PUBLIC, metrics
 * NULL without a metric), the same flags, and std_noise, a HOST array
 * double[M][K] (copied to the workspace on `stream`; NULL without a metric).
 *
 * A partition takes part iff raw_statistics[p][0] > 0.  Its size is
 * configuration 0's sum of the first metric (metrics[0][0][p][0]), or its
 * privacy id count when there is no metric; its bucket is the largest of the
 * PDP_UA_REPORT_BUCKETS lower bounds 0, 1, then 1, 2, 5 times 10^i (i = 1..12)
 * that is <= the size (bucket 0 below 0).
 *
 * Per partition, configuration k and metric m, with s, cmin, cmax, el0, sl0
 * the five metric fields, keep the selection probability (1 when public) and
 * sn = std_noise[m][k], each line rounded operation by operation:
 *   linf_drop = cmin - cmax;  l0_drop = -el0;
 *   after = (s - l0_drop) - linf_drop;  sel_drop = after * (1 - keep);
 *   bias = (el0 + cmin) + cmax;  l0_var = sl0 * sl0;  var = l0_var + sn * sn;
 *   rmse = sqrt(bias * bias + var);
 *   rmse_drop = keep * rmse + (1 - keep) * fabs(s);
 *   abs[8] = {el0, l0_var, cmin, cmax, bias, var, rmse, rmse_drop}, each * keep;
 *   rel[8] = abs / s (abs[1] and abs[5]: / (s * s)), all zero when s == 0.
 *
 * report: device double[PDP_UA_REPORT_BUCKETS + 1][F][K], F = 3 + 20 M, the
 * last entry over all partitions.  Fields: 0 the total weight W = sum keep,
 * 1 sum keep, 2 sum keep (1 - keep) (kept_partitions mean and variance); then
 * per metric, at 3 + 20 m: sum_actual = sum s; the dropped sums l0, linf,
 * partition_selection, each times (sum_actual == 0 ? 1 : 1 / sum_actual); the
 * eight absolute and the eight relative errors (l0 mean, l0 var, linf_min,
 * linf_max, mean, variance, rmse, rmse_with_dropped_partitions), each times
 * (W == 0 ? 0 : 1 / W).  counts: device int64[PDP_UA_REPORT_BUCKETS + 1][2]:
 * partitions taking part; with PDP_UA_PUBLIC those whose raw count
 * (raw_statistics[p][1]) is not 0 in [0] and the empty ones in [1].
 *
 * Partition indices are sorted by bucket (stable), every bucket's run is
 * summed in tiles, tiles in order, and the all-partitions entry adds the
 * buckets' unscaled sums in bucket order: no floating-point atomic, two calls
 * give the same bits.  The workspace (256-byte aligned) holds 5 B per
 * partition and F K doubles per 128 partitions. */
#define PDP_UA_REPORT_BUCKETS 38
int pdp_utility_report_workspace_bytes(int64_t n_partitions, int32_t n_configurations, int32_t flags,
                                       uint64_t* bytes);
int pdp_utility_report(const int64_t* raw_statistics, const double* keep_probability, const double* metrics,
                       int64_t n_partitions, int32_t n_configurations, int32_t flags, const double* std_noise,
                       double* report, int64_t* counts, void* workspace, uint64_t workspace_bytes, void* stream);

/* Multi-GPU sharding check (ColumnarBackend privacy_id_sharding="verify"):
 * counts the ids whose owner rank is not `rank`, where owner(id) =
 * mix(id) mod world with mix(z) = (z ^ (z >> 31)) * 0x9E3779B97F4A7C15, then
 * z ^ (z >> 29) (int64, arithmetic shifts, wrapping multiply; the value
 * taken non-negative mod world) — pipelinedp_amd.parallel.owner_of.  When no
 * rank holds an id it does not own, no id can be on two ranks, so the
 * library skips the exchange of distinct ids (contribution_bounders.py:62-111
 * bounds per privacy id over the whole dataset).  ids: device int64[n];
 * *mismatches: device uint32, overwritten (a saturating count: 2^32 - 1 at most, never wraps to 0). */
int pdp_owner_mismatches(const int64_t* ids, int64_t n, int32_t world, int32_t rank, uint32_t* mismatches,
                         void* stream);

/* Kernel profiler: when enabled, every kernel launch of this library is
 * bracketed by HIP events recorded on its launch stream.  enable(1) clears
 * previous records; report() synchronises on them and returns, per kernel
 * name (first-launch order), the summed milliseconds and the launch count.
 * `names` is max_entries * PDP_PROF_NAME_LEN bytes. */
#define PDP_PROF_NAME_LEN 64
int pdp_profiler_enable(int enable);
int pdp_profiler_report(int32_t max_entries, char* names, double* total_ms, int64_t* calls,
                        int32_t* n_entries);

#ifdef __cplusplus
}
#endif

#endif /* PIPELINEDP_AMD_H_ */
