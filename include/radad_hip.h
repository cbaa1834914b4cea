/*
 * radad_hip.h -- C ABI of libradad_hip.so: the MI355X (gfx950) implementation of RADAD's
 * segment -> embed -> retrieve hot path.
 *
 * Conventions (all entry points):
 *   - plain C types only; no torch / C++ types cross this boundary.
 *   - pointers named *_dev are DEVICE pointers (e.g. torch.Tensor.data_ptr()); *_host are host pointers.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Kernels are enqueued on it
 *     and the call returns without synchronising unless the comment says otherwise.
 *   - every function returns 0 on success and a negative RADAD_E* code on failure; the message for the
 *     calling thread is available from radad_last_error().
 *   - handles are opaque.  A handle may be searched/reconstructed from several threads (host calls are serialised by a
 *     mutex, the device work of consecutive searches by stream order -- a search on ANOTHER stream than the previous one first
 *     records an event behind that stream's work and waits for it: they share one workspace; a stream a handle was last
 *     searched on should therefore outlive the handle's next search, else that search synchronises the device); add/load/destroy
 *     must not race with anything else.
 *   - "without synchronising" has one exception per store: the FIRST large-batch search after the store was created, grown
 *     past its capacity, or re-decided (radad_knn_plane_rebuilds) builds the f16 plane inside the call -- hipDeviceSynchronize,
 *     hipMalloc of 2 bytes per element, one small read-back -- i.e. it stalls every stream of the device once (0.84 ms of
 *     kernel time per million rows of 512).  Build-then-search callers never notice; a caller that interleaves adds and
 *     searches on several streams should radad_knn_reserve up front and run one warm-up search after the last add.
 *   - the maintenance calls synchronise by design: radad_knn_reserve, radad_knn_load / _load_range, radad_knn_save and
 *     radad_knn_remove_ids / _remove_ids_host wait for the whole device before they touch the rows (searches on other streams
 *     may still read them), and the last of these also reads its counts back and returns with its moves complete.
 *
 * Each group cites the reference interface (file:line under the RADAD repository) it replaces.
 */
#ifndef RADAD_HIP_H
#define RADAD_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RADAD_ABI_VERSION 1

/* error codes */
#define RADAD_OK 0
#define RADAD_EINVAL (-1)   /* bad argument (maps to ValueError in the Python mirror)      */
#define RADAD_EHIP (-2)     /* a HIP runtime call failed                                    */
#define RADAD_ENOMEM (-3)   /* device or host allocation failed                             */
#define RADAD_EIO (-4)      /* save/load failed                                             */
#define RADAD_ESTATE (-5)   /* handle in the wrong state (e.g. search on an empty index)   */

/* metric: what faiss.IndexFlatL2 / IndexFlatIP / IndexFlatIP+normalise compute
 * (vector_database.py:61-64, :97, :100-105) */
#define RADAD_METRIC_L2 0      /* squared Euclidean distance, ascending                    */
#define RADAD_METRIC_IP 1      /* inner product, descending                                */
#define RADAD_METRIC_COSINE 2  /* rows and queries L2-normalised (x/(|x|+1e-12)), then IP  */

/* pooling mode (config.tpp_pooling_type, pooling.py:74-80) */
#define RADAD_POOL_MAX 0
#define RADAD_POOL_AVG 1

int radad_abi_version(void);
const char* radad_last_error(void);
/* number of visible HIP devices, or a negative error code */
int radad_device_count(void);

/* ------------------------------------------------------------------------------------------------
 * Vector store + brute-force kNN.
 * Replaces the faiss index object that vector_database.py keeps in `self.index`:
 *   create   -> faiss.IndexFlatL2/IP(dimension)                 vector_database.py:56-97
 *   add      -> index.add(batch) after _maybe_normalize          vector_database.py:100-105,118,138
 *   ntotal   -> index.ntotal                                     vector_database.py:151,169; pipeline.py:465
 *   search   -> index.search(q, k)                               vector_database.py:181
 *   reconstruct -> index.reconstruct(i)                          pipeline.py:503
 *   save/load -> faiss.write_index / read_index                  vector_database.py:203,230
 * ---------------------------------------------------------------------------------------------- */
typedef struct radad_knn_s* radad_knn_t;

/* dim must be a positive multiple of 4.  id_base is added to every returned index (row-shard offset;
 * 0 for an unsharded store).  Rows are stored as fp32 in HBM in insertion order.
 * The width x k limit: a store of any such dim can be created and filled, but a search of it at k needs
 *     dim * 4 + 96 * k + 16 <= 163840
 * (one fp32 query and the eight k-entry lists of the exact float64 kernel in the 160 KB LDS of a compute unit): dim <= 16380 at
 * k = RADAD_KNN_MAX_K = 1024, dim <= 40932 at k = 1.  Every search entry point (radad_knn_search*, _search_begin, _search_excl* -- there
 * with k_fetch for k) returns RADAD_EINVAL beyond it BEFORE anything is enqueued: the output buffers are untouched and the handle
 * stays usable, whether or not the search would have needed the exact kernel. */
int radad_knn_create(int dim, int metric, int device, int64_t id_base, radad_knn_t* out);
/* same with a choice of storage type.  RADAD_STORE_F16 is the reference's `use_float16` knob (faiss
 * GpuIndexFlatConfig.useFloat16, vector_database.py:80): rows are rounded to IEEE fp16 on the way in (after the cosine
 * normalisation), the scan runs on v_mfma_f32_32x32x16_f16 (fp16 operands, fp32 accumulate; dim % 64 == 0 and k <= 26,
 * other shapes decode to fp32 while staging), the float64 re-rank uses the fp32 queries against the decoded rows,
 * reconstruct returns the decoded rows. */
#define RADAD_STORE_F32 0
#define RADAD_STORE_F16 1
int radad_knn_create_ex(int dim, int metric, int store_dtype, int device, int64_t id_base, radad_knn_t* out);
/* Kernel choices of a handle, for experiments and A/B measurements (every value returns the same results; only speed differs).
 * Set them right after creation: HI_PLANE and CENTRE are refused once the f16 plane of the store has been built.
 *   RADAD_KNN_OPT_HI_PLANE   1 (default) / 0: large batches scan the f16 "hi plane" of an fp32 store (certified scan + float64 re-rank)
 *                            / every batch scans on the fp32 kernels (~8x slower 1024-query scans)
 *   RADAD_KNN_OPT_CENTRE     -1 (default: decided per store from |mean|^2 / mean |y|^2) / 0 never / 1 always subtract the rows' column
 *                            mean before rounding the plane
 *   RADAD_KNN_OPT_SMALLQ_HI  1 (default) / 0: batches of <= 16 queries stream the f16 plane / the fp32 rows (twice the bytes)
 *   RADAD_KNN_OPT_WIDE_MIN_Q smallest batch that takes the 256-query tile scan instead of the streaming kernels (default 17)
 *   RADAD_KNN_OPT_DENSE      1 (default) / 0: an fp32 store of <= 6144 rows (<= 16384 for <= 16 queries) is searched by writing out every
 *                            score and selecting on them / by the register-list kernels
 *   RADAD_KNN_OPT_ABANDON    1 (default) / 0: the certified tile scan leaves a 256 x 256 tile after its first K stages when no score
 *                            of it can still reach its query's admission floor (it pays on stores whose k-th neighbour stands clear
 *                            of the bulk of the rows; where it cannot, a scalar gate keeps the test from running) / it never does
 *   RADAD_KNN_OPT_RANGE_SMALLQ  0 (default) / 1: the three range calls answer a batch of <= 16 queries on the float64 exact kernel / by
 *                            streaming the f16 plane once (RADAD_RANGE_STREAM, below); no environment override
 *   RADAD_KNN_OPT_ABANDON_DEAL  0 (default) / 1: every launch of the tile scan walks static chunks / an abandoning launch of <= 8 query
 *                            tiles whose resident workgroups would each draw at least two granules deals its row tiles to the
 *                            workgroups by ticket, so that a skip pattern that is not spread evenly over the store does not leave the
 *                            launch waiting for its slowest chunk.  Off by default: on the benchmark it measured no gain that stands
 *                            clear of the run-to-run spread (profiles/abandon_deal_ab.txt); no environment override
 *   RADAD_KNN_OPT_ABANDON_DEFER  1 (default) / 0: an abandoning launch of <= 8 query tiles that is not dealt and whose rows span less
 *                            than 4 GiB of the plane lists the live rows of a vetoed tile that has at most 16 of them, leaves the tile as
 *                            a skipped one, and scores the listed rows in full against their query tile in a tail behind the scan
 *                            launch (short lists in 16-row groups spread over every CU, long ones in 256-row tiles: each list is
 *                            taken by one of the two) / a vetoed tile is multiplied in full.  Same candidates either way.  Measured:
 *                            profiles/abandon_defer_ab.txt, profiles/row_tail_ab.txt; RADAD_KNN_OPT_ABANDON 0 turns it off too; no
 *                            environment override
 *   RADAD_KNN_OPT_ABANDON_AHEAD  1 (default) / 0: in an abandoning launch that is not dealt, the checkpoint stage of a tile that is
 *                            expected to leave (skipped or deferred: the workgroup's last tested tile left, or it has tested none yet)
 *                            fetches the NEXT tile's first stage instead of its own next one, so that a leaving tile costs one barrier
 *                            and no exposed DMA round trip; a tile that stays after all fetches its own stage then and waits one barrier
 *                            more than before / the checkpoint stage fetches the tile's own next stage, and a leaving tile fetches
 *                            the next tile's head behind its checkpoint.  Same scores, candidates and counts either way.  Measured
 *                            (profiles/abandon_ahead_ab.txt): 1.021-1.025 -> 0.942-0.945 ms per benchmark step, where every tile task
 *                            leaves.  KNOWN LOSS: a store whose tiles strictly alternate between leaving and staying is predicted wrongly
 *                            at every tile and searches 3 % slower with 1 than with 0 (1 M x 512, 1024 queries: 0.975 -> 1.005 ms); the
 *                            predictor has no hysteresis.  A store where every tile stays costs the same either way.
 *                            RADAD_KNN_OPT_ABANDON 0 turns it off too; no environment override
 * The environment variables RADAD_KNN_HI, RADAD_KNN_CENTRE, RADAD_KNN_SMALLQ_HI, RADAD_WIDE_MIN_Q override the DEFAULTS of handles
 * created while they are set (announced once per process on stderr); the product path never needs them. */
#define RADAD_KNN_OPT_HI_PLANE 0
#define RADAD_KNN_OPT_CENTRE 1
#define RADAD_KNN_OPT_SMALLQ_HI 2
#define RADAD_KNN_OPT_WIDE_MIN_Q 3
#define RADAD_KNN_OPT_DENSE 4
#define RADAD_KNN_OPT_ABANDON 5
#define RADAD_KNN_OPT_RANGE_SMALLQ 6
#define RADAD_KNN_OPT_ABANDON_DEAL 7
#define RADAD_KNN_OPT_ABANDON_DEFER 8
#define RADAD_KNN_OPT_ABANDON_AHEAD 9
/*   RADAD_KNN_OPT_REMOVE_STAGE_ROWS  0 (default: as many rows as 64 MiB hold) / n > 0: radad_knn_remove_ids walks the store in slabs of n
 *                            rows and stages a slab in a buffer of n rows; values below 64 are raised to 64.  Same store afterwards
 *                            whatever the value: it exists so that a test store of a few thousand rows spans dozens of slabs. */
#define RADAD_KNN_OPT_REMOVE_STAGE_ROWS 10
int radad_knn_set_option(radad_knn_t h, int option, int value);
int radad_knn_destroy(radad_knn_t h);
int radad_knn_dim(radad_knn_t h, int* dim);
int radad_knn_metric(radad_knn_t h, int* metric);
int radad_knn_ntotal(radad_knn_t h, int64_t* n);
/* reserve HBM for `capacity` rows up front (optional; add grows geometrically otherwise) */
int radad_knn_reserve(radad_knn_t h, int64_t capacity);
/* append n rows [n, dim] fp32 (device pointer).  Cosine: rows are normalised on the way in, so
 * reconstruct returns the normalised row exactly as faiss would return what was added -- in fp32, within a few ulp of
 * x / (|x| + 1e-12f) and bit for bit what radad_rownorm and a cosine search's query preparation give for the same row
 * (tests/test_gpu_store_contents.py: test_ingest_holds_what_the_model_says, test_the_query_a_search_uses). */
int radad_knn_add(radad_knn_t h, const float* rows_dev, int64_t n, void* stream);
/* same, from a host buffer (what index.add(np.ndarray) does); synchronous */
int radad_knn_add_host(radad_knn_t h, const float* rows_host, int64_t n);
/* Remove rows in place, on the device (faiss IndexFlat.remove_ids): the rows named by `ids` go, the others keep their bits and their
 * relative order and hold positions 0 ... ntotal - 1 afterwards, so row i stays aligned with whatever the caller keeps per row.
 *   ids_dev         [n_ids] GLOBAL ids (id_base + position), in any order, repeats allowed.  An id that names no stored row --
 *                   negative, below id_base, at or beyond id_base + ntotal -- is ignored and not counted.  n_ids == 0 removes nothing
 *   old_to_new_dev  NULL, or [ntotal before the call] int64: the new global id of every old position, -1 for a removed one (for the
 *                   caller's own per-row columns, e.g. speaker tags)
 *   n_removed_out   host, may be NULL: the number of DISTINCT rows removed; ntotal falls by it.  capacity is unchanged (no shrink)
 * A synchronising maintenance call like radad_knn_reserve and radad_knn_load: it waits for the device before it touches anything
 * (searches on other streams may still read the rows), reads the removed count back, and returns with the moves complete.  The mark,
 * the prefix sum (integers only: deterministic) and the moves run on `stream`.  Workspace: 5 bytes per stored row plus a staging
 * buffer of RADAD_KNN_OPT_REMOVE_STAGE_ROWS rows (64 MiB by default, never proportional to the store), taken from the handle's search
 * workspace; when it cannot be allocated the call returns RADAD_ENOMEM and the store is exactly as it was.
 * Refused with RADAD_ESTATE while a two-half search is pending (radad_knn_search_begin / _search_excl_begin without its _finish or
 * radad_knn_search_abort), as radad_knn_add is refused; the handle stays usable.  RADAD_EINVAL for NULL ids with n_ids > 0.
 * Afterwards every search path keeps its exactness contract: the f16 plane, its scales and the per-tile terms are kept for the rows
 * in front of the first removed one and brought up to date behind it by the next search that wants them, as after an append -- the
 * plane is not rebuilt.  A store emptied this way behaves like a new one that keeps its capacity.
 * On a row shard (id_base != 0) ids outside the shard's own range are ignored and ids shift inside the shard only: the global id
 * space then has a gap in front of the next shard. */
int radad_knn_remove_ids(radad_knn_t h, const int64_t* ids_dev, int64_t n_ids, int64_t* old_to_new_dev, int64_t* n_removed_out, void* stream);
/* same, with the id list on the host */
int radad_knn_remove_ids_host(radad_knn_t h, const int64_t* ids_host, int64_t n_ids, int64_t* n_removed_out);
/* the last removal's plan (no synchronisation): its move launches and the bytes they read + wrote; 0 / 0 when nothing moved */
int radad_knn_last_remove(radad_knn_t h, int* n_launches, int64_t* bytes_moved);
/* top-k of every query against the whole store.
 *   q_dev        [nq, dim] fp32
 *   out_dist_dev [nq, k] fp32  L2: squared distances ascending; IP/cosine: inner products descending
 *   out_idx_dev  [nq, k] int64 id_base + row; ties are broken towards the LOWER index, always
 *   slots beyond ntotal are filled with index -1 and distance +inf (L2) / -inf (IP), as faiss does.
 * k must be in [1, RADAD_KNN_MAX_K], and dim * 4 + 96 * k + 16 <= 163840 (the width x k limit, radad_knn_create). */
#define RADAD_KNN_MAX_K 1024
int radad_knn_search(radad_knn_t h, const float* q_dev, int64_t nq, int k, float* out_dist_dev,
                     int64_t* out_idx_dev, void* stream);
/* same search, additionally returning the float64 distances the final ranking was made on
 * (out_key_dev [nq, k] double, may be NULL).  The MFMA scan is a filter with a measured error bound eps(q): every listed
 * row whose scan score is within 2 eps of the k-th best is re-scored in float64 from the stored rows (L2 as sum (q-y)^2)
 * and ordered by (float64 distance, id); a per-query certificate checks that no unlisted row can reach that threshold, and
 * the queries it rejects are searched again by an exact float64 kernel (driven from the device, no host round trip).  For
 * every k in [1, RADAD_KNN_MAX_K] within the width x k limit (radad_knn_create: dim * 4 + 96 * k + 16 <= 163840, i.e. dim <= 16380
 * at k = 1024; refused with RADAD_EINVAL before anything is enqueued otherwise) ids and order are therefore those of an exact
 * float64 brute force, ties to the lower id, and
 * out_dist is the correctly rounded distance (k <= 128 takes the f16 MFMA scans where they apply; larger k the fp32 tile
 * kernels, certified the same way).  Sharded
 * searches merge on these keys (radad_topk_merge_f64) so that no cross-shard pair is decided by fp32 rounding.
 * A handle may be searched from several threads and streams: calls are serialised by a mutex and a search enqueued on another
 * stream than the previous one waits (event) for that one's device work, since they share the handle's workspace. */
int radad_knn_search_f64(radad_knn_t h, const float* q_dev, int64_t nq, int k, float* out_dist_dev,
                         int64_t* out_idx_dev, double* out_key_dev, void* stream);
/* same with a choice of query type: RADAD_Q_BF16 = bfloat16 queries [nq, dim] (BASELINE config 5: bf16 embeddings,
 * the reference's autocast knob feature_extractor.py:84,140) -- decoded exactly to fp32 on the device, then the same
 * path (cosine normalisation in fp32, as vector_database.py:166 does on whatever it is handed). */
#define RADAD_Q_F32 0
#define RADAD_Q_BF16 1
int radad_knn_search_ex(radad_knn_t h, const void* q_dev, int q_dtype, int64_t nq, int k, float* out_dist_dev,
                        int64_t* out_idx_dev, double* out_key_dev, void* stream);
/* The same search in two halves, for a store that is ROW-SHARDED over several GPUs (the reference is single-GPU,
 * vector_database.py:23; sharding is this build's, north_star).  _begin prepares the queries and scans this shard; it writes to
 * topk_lower_bounds_dev [nq, k] lower bounds of the exact scores of this shard's k best rows per query, unordered (scores: q.y
 * for inner product / cosine, -|q - y|^2 for L2; -inf where the shard has fewer rows or the scan that ran offers none).  The
 * caller gathers them from all shards (one all-gather of 4 nq k bytes per shard) and takes, per query, the k-th LARGEST of the
 * G k values: a lower bound of the exact k-th best score of the whole store.  _finish, given that [nq] vector, re-ranks in
 * float64 only the candidates that can still be among the GLOBAL k best -- instead of every shard certifying its own top k,
 * G x the work of one GPU on G shards.  With a bound the rows a shard returns are those of its rows that can be in the global
 * top k (fewer than k is normal; the rest is -1 filled); merged over the shards (radad_topk_merge_f64) the result is exactly the
 * unsharded search's.  global_lower_bound_dev == NULL: _finish returns this shard's own top k, i.e. _begin + _finish ==
 * radad_knn_search_ex.  One begun search per handle at a time; other searches on the handle fail until it is finished.  (Each
 * claim above is asserted by tests/test_gpu_sharded_bound.py on the designed stores of tests/sharded_bound_ref.py.) */
int radad_knn_search_begin(radad_knn_t h, const void* q_dev, int q_dtype, int64_t nq, int k, float* topk_lower_bounds_dev, void* stream);
int radad_knn_search_finish(radad_knn_t h, const float* global_lower_bound_dev, float* out_dist_dev, int64_t* out_idx_dev,
                            double* out_key_dev, void* stream);
/* Gives up a begun search (e.g. the exchange of the bounds between the shards failed): the handle accepts searches again.  No-op when
 * nothing was begun.  While a search is begun, add / reserve / load / load_range fail with RADAD_EINVAL (its second half reads the
 * rows live); _finish may run on another stream than _begin (it waits for _begin's device work through an event). */
int radad_knn_search_abort(radad_knn_t h);
/* host-buffer variant (what index.search(np.ndarray, k) does); synchronous */
int radad_knn_search_host(radad_knn_t h, const float* q_host, int64_t nq, int k, float* out_dist_host,
                          int64_t* out_idx_host);
/* batched index.reconstruct: out[i,:] = row (idx[i] - id_base); idx < 0 or out of range -> zeros
 * (the zero padding pipeline.py:511-512 applies) */
int radad_knn_reconstruct(radad_knn_t h, const int64_t* idx_dev, int64_t n, float* out_dev, void* stream);
int radad_knn_reconstruct_host(radad_knn_t h, const int64_t* idx_host, int64_t n, float* out_host);
/* binary snapshot of the store ("RADADKNN" header + rows as stored, fp32 or fp16); load replaces the contents of h
 * (VectorDatabase.save / .load, vector_database.py:190-242).  Both directions stream through two pinned staging
 * buffers on a private stream (file I/O overlaps the DMA); load maps the file read-only, so
 * radad_knn_load_range -- rows [row0, row0 + n_rows) of the snapshot, n_rows < 0 = through the end -- touches only
 * its own byte range: G ranks load one snapshot as G row shards (create each handle with id_base = row0). */
int radad_knn_save(radad_knn_t h, const char* path);
int radad_knn_load(radad_knn_t h, const char* path);
int radad_knn_load_range(radad_knn_t h, const char* path, int64_t row0, int64_t n_rows);
/* header of a snapshot without a handle (any out pointer may be NULL) */
int radad_knn_snapshot_info(const char* path, int* dim_out, int* metric_out, int* store_dtype_out, int64_t* ntotal_out);
/* seconds spent in the most recent search's kernels are NOT measured here; use HIP events on `stream`.
 * Query the launch geometry of the last search (for roofline accounting in bench.py). */
int radad_knn_last_launch(radad_knn_t h, int* n_query_tiles, int* n_db_splits, int* block_threads);
/* which scan kernel the last search ran: what it streams decides the bytes a roofline is quoted on */
#define RADAD_SCAN_F32_TILE 0     /* fp32-MFMA tile kernels (fp32 rows; also the generic kernel) */
#define RADAD_SCAN_HI_TILE 1      /* certified f16-MFMA tile scan over the f16 plane / fp16 store (more than 16 queries) */
#define RADAD_SCAN_F32_SMALLQ 2   /* <= 16 queries, fp32 rows streamed (4 bytes per element) */
#define RADAD_SCAN_HI_SMALLQ 3    /* <= 16 queries, f16 plane / fp16 store streamed (2 bytes per element), certified */
#define RADAD_SCAN_F16_TILE 4     /* fp16 store on the fp16-MFMA tile kernel without the certificate path */
#define RADAD_SCAN_F32_DENSE 5    /* small fp32 store: every (row, query) score written out (fp32 MFMA), selection on the scores */
int radad_knn_last_scan_kind(radad_knn_t h, int* kind);
/* scan-kernel launches of the last search (the certified tile scan covers a large store in two: the first eighth with the
 * sample's admission floor, the rest with the floor the first eighth's candidates give); radad_knn_profile_read has one entry each */
/* How ONE launch of the certified tile scan over n_rows rows and n_queries queries is laid out (pure host arithmetic, no device): 256-query
 * tiles, `chunks` row chunks (a multiple of 8) of rows_per_chunk rows (a multiple of the 256-row tile) -- query_tiles x chunks workgroups.
 * Chosen by what the launch costs: (rounds of 256 workgroups) x (tiles per chunk), both rounded up. */
int radad_knn_scan_geometry(int64_t n_rows, int64_t n_queries, int* query_tiles, int* chunks, int64_t* rows_per_chunk);
int radad_knn_last_scan_launches(radad_knn_t h, int* n_launches);
/* phases of the last tile scan (the most recent search that took the certified tile scan; other scan kinds leave it as it was): 1 + the
 * number of times the admission floors were raised from the candidates emitted so far, one launch per phase with k_kth_floor between them
 * (2 up to ~1.2 M rows, 3 up to ~9.5 M, 4 beyond) -- always equal to that search's radad_knn_last_scan_launches */
int radad_knn_last_scan_phases(radad_knn_t h, int* n_phases);
/* Diagnostics of the last search when it was a certified tile scan of nq queries (synchronises with it): per query the number of
 * candidates the scan emitted (more than the candidate buffer holds -- 1024, 4096 after the handle widened them -- rejects the query)
 * and, optionally, the admission floor the scan ended with.  Host pointers. */
int radad_knn_last_emitted(radad_knn_t h, int* counts_host, float* floors_host, int64_t nq);
/* Early abandon of the last search (synchronises with it): of the `tasks` (query tile, row tile) pairs its abandoning scan launches
 * covered, how many ran the test (`checked`: the gate let them) and how many were left after it (`skipped`).  All three are 0 when
 * no launch of the last search took the abandoning scan. */
int radad_knn_last_abandon(radad_knn_t h, int64_t* checked, int64_t* skipped, int64_t* tasks);
/* ... and how its abandoning launches got their row tiles (no synchronisation: the host's plan): how many of them were dealt by ticket
 * (RADAD_KNN_OPT_ABANDON_DEAL), and of the last dealt one the workgroups launched and the row tiles per granule.  All 0 when none was. */
int radad_knn_last_abandon_deal(radad_knn_t h, int* launches, int* workgroups, int* granule);
/* ... and what its deferring launches (RADAD_KNN_OPT_ABANDON_DEFER) handed to their tails (synchronises with the search): the vetoed tile
 * tasks that listed their live rows and left (`checked` counts them, `skipped` does not), the rows listed over all query tiles, and the
 * tails run (one per deferring launch, whichever kernel took its lists).  All 0 when no launch deferred. */
int radad_knn_last_abandon_defer(radad_knn_t h, int64_t* tile_tasks_deferred, int64_t* rows_listed, int* tail_launches);
/* ... and what became of the heads its launches fetched ahead (RADAD_KNN_OPT_ABANDON_AHEAD; synchronises with the search): the tile tasks
 * that left into a next tile's head already fetched (`heads_used`), and those that stayed and fetched their own stage over one
 * (`heads_wasted`).  Both 0 when no launch of the last search fetched ahead. */
int radad_knn_last_abandon_ahead(radad_knn_t h, int64_t* heads_used, int64_t* heads_wasted);
/* the f16 plane the certified scans read, once a search has built it: built (0/1); centred = the common component (column mean)
 * of the rows is subtracted before rounding (stores of embeddings that share most of their mean); one_scale = one power-of-two
 * scale for all rows (rows of one magnitude: the scan applies no per-score arithmetic) */
int radad_knn_plane_info(radad_knn_t h, int* built, int* centred, int* one_scale);
/* How often the plane of this store was RE-decided (dropped and rebuilt with a new centre and scale): it is decided from the rows the
 * store holds when it is first built; it is decided again -- 0.84 ms per million rows, one synchronisation, inside the first
 * large-batch search that notices -- when the store has doubled since, when appended rows measure 8x beyond what the decision saw
 * (largest element or rounding residual), or when a batch was mostly rejected by the certificate and rows were appended since
 * (vector_database.py:134-138 appends 10 000 rows at a time; a store that drifts keeps the certified scan instead of the 8x slower
 * fp32 fallback).  Results never depend on it. */
int radad_knn_plane_rebuilds(radad_knn_t h, int* n_out);
/* The handle's self-tuning state, read WITHOUT synchronising (advisory; results never depend on it).  Every certified search leaves
 * a report (queries rejected by the certificate, batch size) in pinned host memory when its device work ends; every later search
 * acts on the reports that have arrived since -- however far the host has run ahead.  A batch of >= 64 queries rejected by more
 * than a quarter first re-decides the plane (if rows were appended since), then widens the candidate buffers (cap_boost 1 -> 4),
 * then moves to the fp32 kernels for 8 searches (fp32_searches_left).  reports_consumed counts the reports looked at so far.
 * (The reference has no counterpart: faiss's flat search has one code path, vector_database.py:181.) */
int radad_knn_tuning_info(radad_knn_t h, int* cap_boost, int* fp32_searches_left, int64_t* reports_consumed);
/* Certificate of the most recent search (see radad_knn_search_f64): number of queries the float64 re-rank could NOT certify
 * and that were therefore searched again by the exact float64 kernel (results are exact either way).  Synchronises with
 * that search.  radad_knn_last_certificate additionally returns the batch size and stats6 = {rejected queries, sum over
 * the batch of candidates re-scored in float64, rejections because: more than 512 candidates within the error bound, the scan's
 * candidate buffer (or a chunk's list, on the fp32 kernels) overflowed, the scan's admission floor was above the threshold, the
 * scan dropped a candidate}. */
int radad_knn_last_recheck(radad_knn_t h, int* n_queries);
int radad_knn_last_certificate(radad_knn_t h, int64_t* n_queries, int* stats6);

/* HIP-event timing of the scan kernel alone, on the stream each search is enqueued on:
 * enable = 1 -> every search records an event pair around each scan-kernel launch (ring of 64); enable = n > 1 -> every n-th search
 * does (an event record between dependent kernels delays the next one by ~6 us: four per certified search of a large store);
 * 0 -> off.  read synchronises on the recorded events and returns the kernel durations in ms, oldest first.  For bench.py's
 * roofline line. */
int radad_knn_profile(radad_knn_t h, int enable);
int radad_knn_profile_read(radad_knn_t h, float* ms_out, int cap, int* n_out);

/* merge P partial top-k lists per query into one (used for the multi-GPU all-gather merge and
 * internally by search):  in_dist/in_idx are [P, nq, k]; metric decides the order; (dist, idx)
 * lexicographic, idx -1 entries sort last. */
int radad_topk_merge(int metric, const float* in_dist_dev, const int64_t* in_idx_dev, int n_parts, int64_t nq,
                     int k, float* out_dist_dev, int64_t* out_idx_dev, int device, void* stream);

int radad_topk_merge_f64(int metric, const double* in_key_dev, const int64_t* in_idx_dev, int n_parts, int64_t nq,
                         int k, float* out_dist_dev, int64_t* out_idx_dev, double* out_key_dev, int device,
                         void* stream);

/* Device-side form of the exclusion loop of retrieve_similar_vectors (pipeline.py:491-515): for every query row keep,
 * in order, the first k_keep of its k_in search hits whose row tag is NOT in the exclusion set; pad with id -1 and
 * distance NaN.  row_tags_dev [ntotal] int64 (e.g. a hash of os.path.basename(path), one per stored row, indexed by
 * id - id_base); excl_sorted_dev [n_excl] int64 ascending (may be NULL when n_excl == 0); hits with id < 0 are skipped. */
int radad_filter_topk(const float* in_dist_dev, const int64_t* in_idx_dev, int64_t nq, int k_in, int k_keep,
                      const int64_t* row_tags_dev, int64_t ntotal, int64_t id_base, const int64_t* excl_sorted_dev,
                      int64_t n_excl, float* out_dist_dev, int64_t* out_idx_dev, int device, void* stream);

/* Exclusion-aware search: per query the k nearest rows whose tag is NOT in the exclusion set, however many excluded rows precede
 * them.  The reference searches K + 10 rows (pipeline.py:478), drops the hits with an excluded basename (:491-509) and pads with zero
 * vectors / label 0 / NaN when fewer than K survive (:511-515) -- radad_knn_search_ex + radad_filter_topk reproduce exactly that, and
 * stay the default: a query with more than 10 excluded rows in front of its K-th admissible neighbour (a batch of clips of few
 * speakers excluding each other, :463; the training_file_ids mode, :500-502, where most of the store is excluded) gets padding
 * although admissible neighbours exist.  This call returns them, with the contract of radad_knn_search_f64:
 *   result      the k best admissible rows ordered by (float64 distance, id); out_dist the correctly rounded fp32 distance, out_key
 *               (may be NULL) the float64 key; slots beyond the number of admissible rows hold id -1, distance NaN and key NaN
 *               (radad_filter_topk's padding, not the +-inf of the plain searches)
 *   fast pass   the certified search at k_fetch (clamped to ntotal), every scan path as it is
 *   certificate per query, on the device: the k_fetch hits hold k admissible rows (any admissible row outside the list ranks behind
 *               the whole list), or the list is all the store has
 *   exact pass  float64 brute force over the admissible rows for the queries the certificate cannot prove, driven from the device
 *               (no host round trip; an excluded row costs one bit of a per-call bitmap).  It streams the admissible rows once per
 *               group of <= 8 such queries -- far more work per query than the certified search spends on one (measured where most
 *               of the store is excluded: 0.051 ms per listed query over 100 000 admissible rows x 512, 3.3 ms for 64 listed
 *               queries, profiles/README.md; when most of the store is excluded use radad_knn_search_excl_scan below).
 *               So choose k_fetch for the crowding you expect: k + (the most excluded rows that can precede a query's k-th
 *               admissible neighbour), e.g. k + clips per speaker in a batch; up to 128 the fast pass stays on the f16 scans.
 * row_tags_dev [ntotal] int64 indexed by id - id_base; excl_sorted_dev [n_excl] int64 ASCENDING (the caller's contract, not checked);
 * both may be NULL only when n_excl == 0.  k in [1, RADAD_KNN_MAX_K], k_fetch in [k, RADAD_KNN_MAX_K]; anything else, or a handle
 * with a begun search, is RADAD_EINVAL; an empty store RADAD_ESTATE.  Stream-ordered and serialised like every search;
 * radad_knn_last_launch, _last_certificate, _tuning_info and the like describe the fast pass only. */
int radad_knn_search_excl(radad_knn_t h, const void* q_dev, int q_dtype, int64_t nq, int k, int k_fetch,
                          const int64_t* row_tags_dev /*[ntotal], indexed by id - id_base*/,
                          const int64_t* excl_sorted_dev /*[n_excl] ascending, NULL when n_excl == 0*/, int64_t n_excl,
                          float* out_dist_dev /*[nq,k]*/, int64_t* out_idx_dev /*[nq,k]*/, double* out_key_dev /*[nq,k] or NULL*/,
                          void* stream);
/* batch size of the most recent radad_knn_search_excl on the handle (n_queries may be NULL) and how many of its queries took the
 * exact pass; synchronises with that search.  0 / 0 before the first one. */
int radad_knn_last_excl(radad_knn_t h, int64_t* n_queries, int* n_exact);

/* The exclusion-aware search over a ROW-SHARDED store, in two halves around one certificate across the shards (the reference's
 * over-fetch and exclusion loop: pipeline.py:478,491-515; it is single-GPU, vector_database.py:23 -- the sharding is this build's).
 * A shard cannot prove a query from its own hits, the shards together can (DESIGN, "exclusion over row shards"):
 *   _begin   on every shard: the certified search at k_fetch (clamped to the shard's rows) and the compaction.  Per query it writes
 *            the first <= k admissible hits (float64 key, global id; -1 / NaN padded) and a FRONTIER (key, id): every admissible row
 *            of the shard that is not in the list ranks strictly behind it, in the order (float64 key in the metric's order, lower
 *            id) of radad_knn_search_f64.  The frontier is the k-th survivor when the list holds k; else the last of the k_fetch hits,
 *            admissible or not; else -- the hits are all the shard has -- id -1, key NaN: nothing is unseen.
 *   certify  radad_excl_merge_certify merges the G lists of a query and proves it iff, for every shard whose frontier id is >= 0, the
 *            merged list M holds k entries and M[k-1] is that frontier entry or ranks ahead of it.
 *   _finish  on every shard, given the [nq] flags of the queries NO shard combination proved: the row-filtered float64 exact pass of
 *            radad_knn_search_excl for those of them whose list on this shard is short although rows are unseen (a full list, or one
 *            that is all the shard has, already is the shard's exact admissible top k); every other row comes through as _begin left
 *            it.  After it each shard's rows of the flagged queries are its exact admissible top k: a plain radad_topk_merge_f64 of
 *            the G lists is exact.
 * So the exact pass -- far more work per query than the fast pass -- runs only for queries that nobody can prove: a shard most of
 * whose rows are excluded (the training_file_ids mode, pipeline.py:500-502) does not enter it while another shard holds k admissible
 * rows in front of its frontier.
 * radad_knn_search_excl_begin: arguments, their rules and RADAD_ESTATE on an empty store as radad_knn_search_excl, except nq >= 1;
 * out_key_dev [nq,k] double, out_idx_dev [nq,k], frontier_key_dev [nq] double, frontier_idx_dev [nq] are all required.  The handle
 * then holds a begun search; it holds at most one, of either kind (radad_knn_search_begin or this): every other search, add, reserve
 * or load on it fails with RADAD_EINVAL until the search is finished or given up (radad_knn_search_abort covers both kinds).  The
 * queries, the row tags and the exclusion set must stay alive until _finish.
 * radad_knn_search_excl_finish: unproved_dev [nq] int32, non-zero = flagged (NULL = none flagged).  out_dist is the correctly
 * rounded key, out_key_dev (may be NULL) the key; padding -1 / NaN / NaN.  It may run on another stream than _begin (it waits for
 * _begin's device work through an event); device-driven, no certificate report, the admission bitmap is built only when a query is
 * listed.  RADAD_EINVAL when no exclusion-aware search was begun.  _begin + _finish with the shard's OWN flags (list short and
 * frontier id >= 0) is radad_knn_search_excl, bit for bit.
 * radad_knn_last_excl after _begin reports its batch size and 0; after _finish, the flagged queries this shard answered exactly.
 * The IVF index has a search of its own for this, radad_ivf_search_excl below (exclusion inside the list scans, no over-fetch).
 * Not combined with the cross-shard lower bound of radad_knn_search_begin / _finish: every shard certifies its own k_fetch here,
 * G times the re-rank work of one GPU. */
int radad_knn_search_excl_begin(radad_knn_t h, const void* q_dev, int q_dtype, int64_t nq, int k, int k_fetch,
                                const int64_t* row_tags_dev, const int64_t* excl_sorted_dev, int64_t n_excl,
                                double* out_key_dev /*[nq,k]*/, int64_t* out_idx_dev /*[nq,k]*/, double* frontier_key_dev /*[nq]*/,
                                int64_t* frontier_idx_dev /*[nq]*/, void* stream);
int radad_knn_search_excl_finish(radad_knn_t h, const int* unproved_dev /*[nq] int32, NULL = none*/, float* out_dist_dev /*[nq,k]*/,
                                 int64_t* out_idx_dev /*[nq,k]*/, double* out_key_dev /*[nq,k] or NULL*/, void* stream);
/* Merge + certificate of the sharded exclusion-aware search (pipeline.py:478,491-515 over this build's row shards): in_key_dev /
 * in_idx_dev [n_parts, nq, k] and frontier_key_dev / frontier_idx_dev [n_parts, nq] as the shards' _begin wrote them, in one order of
 * the shards.  One wave per query merges by (key in the metric's order, lower id), id -1 last, as radad_topk_merge_f64 does, and
 * writes out_dist (the rounded key), out_idx, out_key (may be NULL) with padding -1 / NaN / NaN, and unproved_out_dev [nq] int32: 0 =
 * proved by the rule above, 1 = not.  Limits as radad_topk_merge_f64: 1 <= n_parts <= 4096 (4 bytes of LDS per part and wave),
 * 1 <= k <= RADAD_KNN_MAX_K; k merge rounds of ceil(n_parts / 64) reads per lane. */
int radad_excl_merge_certify(int metric, const double* in_key_dev, const int64_t* in_idx_dev, const double* frontier_key_dev,
                             const int64_t* frontier_idx_dev, int n_parts, int64_t nq, int k, float* out_dist_dev,
                             int64_t* out_idx_dev, double* out_key_dev, int* unproved_out_dev, int device, void* stream);

/* The exclusion-aware search with one exclusion set PER QUERY (leave-one-out: a query excludes its own file, or its own speaker's
 * files, and nothing else).  The reference excludes the union of the batch's basenames (pipeline.py:463,498), so what a clip retrieves
 * there depends on which clips share its batch; here the result of a query is a function of the query alone.  Opt-in: the batch-wide
 * calls above stay as they are.
 * Contract: that of radad_knn_search_excl with one change -- row r is admissible for query j iff row_tags[r] is not among the first
 * cnt_j entries of q_tags[j, :], cnt_j = q_tag_counts[j] clamped on the device to [0, m] (NULL = m for every query).  The tags of a
 * query may come in any order and repeat.  Order (float64 key, lower id); out_dist the key rounded once; padding -1 / NaN / NaN;
 * stream-ordered and serialised like every search.  Fast pass, certificate and exact pass as there: the certificate counts the hits
 * the QUERY admits; the exact pass streams the store once per group of <= 8 listed queries, reads one row tag per row and compares it
 * with the tags of the group's queries held in registers, one ballot per query (no bitmap: one per listed query would cost ntotal / 8
 * bytes each); a row none of the group admits is not loaded (its time per listed query has not been measured either,
 * profiles/README.md).  If no tag is carried by more than c rows, k_fetch >= k + m * c proves
 * every query in the fast pass.
 * 0 <= m <= RADAD_EXCL_PQ_MAX_TAGS: one wave compares a row's tag with a query's set in one ballot (and an all-gather carries the sets
 * at that fixed width).  m == 0: nothing is excluded, the result is the certified search at k with this family's padding.  A larger
 * m, or m > 0 with NULL q_tags_dev or row_tags_dev, is RADAD_EINVAL; the other argument rules, RADAD_ESTATE on an empty store and
 * RADAD_EINVAL on a handle with a begun search as radad_knn_search_excl.  radad_knn_last_excl covers it.
 * radad_knn_search_excl_pq_begin is the first half over a ROW SHARD, as radad_knn_search_excl_begin (nq >= 1, all four outputs
 * required).  Its second half is radad_knn_search_excl_finish: the begun search remembers the admission rule it was begun with.
 * radad_excl_merge_certify and radad_knn_search_abort cover it unchanged; the queries, the row tags, the query tags and the counts
 * must stay alive until _finish.  _pq_begin + _finish with the shard's own flags is radad_knn_search_excl_pq, bit for bit.
 * Not offered: a batch-wide set combined with per-query sets in one call; the cross-shard lower bound.  The IVF index has its own
 * call for this, radad_ivf_search_excl_pq below. */
#define RADAD_EXCL_PQ_MAX_TAGS 64
int radad_knn_search_excl_pq(radad_knn_t h, const void* q_dev, int q_dtype, int64_t nq, int k, int k_fetch,
                             const int64_t* row_tags_dev /*[ntotal], by id - id_base*/,
                             const int64_t* q_tags_dev /*[nq, m] row-major; any order, duplicates allowed*/, int m,
                             const int32_t* q_tag_counts_dev /*[nq] or NULL = m for every query*/, float* out_dist_dev /*[nq,k]*/,
                             int64_t* out_idx_dev /*[nq,k]*/, double* out_key_dev /*[nq,k] or NULL*/, void* stream);
int radad_knn_search_excl_pq_begin(radad_knn_t h, const void* q_dev, int q_dtype, int64_t nq, int k, int k_fetch,
                                   const int64_t* row_tags_dev, const int64_t* q_tags_dev, int m, const int32_t* q_tag_counts_dev,
                                   double* out_key_dev /*[nq,k]*/, int64_t* out_idx_dev /*[nq,k]*/, double* frontier_key_dev /*[nq]*/,
                                   int64_t* frontier_idx_dev /*[nq]*/, void* stream);

/* The exclusion-aware search with the admission test INSIDE the certified tile scan: the call for exclusion sets that cover much of the
 * store (the training_file_ids mode, pipeline.py:500-502), where no k_fetch <= 1024 proves a query and radad_knn_search_excl sends
 * the whole batch through its exact pass.  The result contract is radad_knn_search_excl's without k_fetch: the k best admissible rows
 * ordered by (float64 key, lower id), out_dist the key rounded once, id -1 / NaN / NaN where the store has fewer admissible rows.
 * Two routes, chosen on the host (knn_excl_scan_route, knn_plan.h):
 *   RADAD_EXCL_SCAN_TILE   exactly when the plain search of this batch would take RADAD_SCAN_HI_TILE (17 or more queries, dim % 64
 *                 == 0, k <= 128, the plane on, a store large enough for the sample pre-pass -- 16 384 rows at small k --, and the
 *                 handle not on its fp32 fallback).  A pre-pass on `stream` builds the admission bitmap and a per-call bias array
 *                 (the plane's bias, or 0, where a row is admitted; NaN where it is not: 12 bytes read and 4 written per row); the
 *                 scan runs its biased instantiation (RSC 2 / 3; an un-centred IP / cosine store with a zero query constant) with
 *                 that array.  A NaN score passes no compare of the scan (DESIGN, "exclusion inside the tile scan", names each), so
 *                 an excluded row is never emitted and never counts towards a floor: the scan costs what the plain scan costs,
 *                 however much of the store is excluded.  Sample pre-pass, floors, phases, K split and the float64 re-rank are the
 *                 plain search's; the queries its certificate rejects go, driven from the device, to the ROW-FILTERED float64 exact
 *                 kernel with the same bitmap.  The handle's own bias arrays are not written.
 *   RADAD_EXCL_SCAN_EXACT  every other shape (16 or fewer queries, small stores, k > 128, dim % 64 != 0, plane off, fp32 fallback
 *                 active): the row-filtered float64 exact pass for every query.  Correct everywhere; about two fp32 passes over
 *                 the store per group of <= 8 queries, so slow for large batches (k > 128 with hundreds of queries: prefer
 *                 radad_knn_search_excl there when few excluded rows crowd a query).
 * The call posts no certificate report and leaves radad_knn_tuning_info's three values and the plane's re-decision inputs as it
 * found them (a batch with few admissible rows overflows its candidate buffers by design and must not push later plain searches to
 * fp32); it may build the plane, as any first large-batch search does.  radad_knn_last_recheck / _last_certificate keep describing
 * the last plain search.  Arguments and errors as radad_knn_search_excl: row_tags_dev / excl_sorted_dev (ascending) may be NULL only
 * when n_excl == 0; RADAD_ESTATE on an empty store; RADAD_EINVAL on a handle with a begun search or beyond the width x k limit,
 * before anything is enqueued.  Stream-ordered and serialised like every search.
 * Per-query sets: radad_knn_search_excl_scan_pq below (a bias is per row, not per (row, query), so that call filters what the scan
 * emitted instead).  Not offered: a begin / finish pair (a shard's result here IS its exact admissible top k: radad_topk_merge_f64 of
 * the shards' lists is exact).
 * radad_knn_last_excl_scan synchronises with the most recent such call -- this one or radad_knn_search_excl_scan_pq, whichever ran
 * last: its batch size (may be NULL), route and the number of queries the exact kernel answered (all of them on the exact route).
 * 0 / RADAD_EXCL_SCAN_EXACT / 0 before the first one. */
#define RADAD_EXCL_SCAN_TILE 0
#define RADAD_EXCL_SCAN_EXACT 1
int radad_knn_search_excl_scan(radad_knn_t h, const void* q_dev, int q_dtype, int64_t nq, int k,
                               const int64_t* row_tags_dev /*[ntotal], by id - id_base*/,
                               const int64_t* excl_sorted_dev /*[n_excl] ascending, NULL when n_excl == 0*/, int64_t n_excl,
                               float* out_dist_dev /*[nq,k]*/, int64_t* out_idx_dev /*[nq,k]*/, double* out_key_dev /*[nq,k] or NULL*/,
                               void* stream);
int radad_knn_last_excl_scan(radad_knn_t h, int64_t* n_queries, int* route, int* n_exact);

/* One exclusion set PER QUERY on the certified tile scan: leave-one-speaker-out over a flat store, where one tag is carried by
 * hundreds or thousands of rows and no k_fetch <= 1024 lets radad_knn_search_excl_pq prove a query (k_fetch >= k + m * c).
 * Contract: radad_knn_search_excl_pq's without k_fetch -- row r is admissible for query j iff row_tags[r] is not among the first cnt_j
 * entries of q_tags[j, :], cnt_j = q_tag_counts[j] clamped on the device to [0, m] (NULL = m for every query), any order, repeats
 * allowed; per query the k best admissible rows ordered by (float64 key, lower id), out_dist the key rounded once, id -1 / NaN / NaN
 * where the query has fewer admissible rows; the result of a query is a function of that query alone.
 * Routes: knn_excl_scan_route's, as radad_knn_search_excl_scan, reported by radad_knn_last_excl_scan:
 *   RADAD_EXCL_SCAN_TILE   the PLAIN search's plan and launches -- its RSC, no per-call bias, sample pre-pass, phases, K split, early
 *                 abandon -- over candidate buffers of 4096 entries per query (the handle's widened form, whatever its tuning state).
 *                 The scan emits excluded rows like any other; k_excl_pq_scrub (one workgroup per query, the query's tags in LDS)
 *                 clears a query's excluded entries (row -> no entry, score -> -inf) out of the sample's lists before the first
 *                 floor is taken from them, out of the candidate buffers before every floor between two phases, and before the
 *                 float64 re-rank: phases + 1 launches (none when m == 0; a query whose count is 0 leaves at once).  So an excluded
 *                 row never counts towards a floor and never reaches the re-rank; the floors stay lower bounds for admissible rows,
 *                 which is all the abandon needs.  A query whose emitted rows -- excluded ones included -- exceed its buffer is
 *                 rejected by the certificate like any overflow; rejected queries go, driven from the device, to the per-query
 *                 float64 exact kernel (k_exact_scan_any<true, true>) with the query tags (m == 0: the bitmap form, every bit set).
 *   RADAD_EXCL_SCAN_EXACT  every other shape: that exact kernel for every query.  Correct everywhere; it streams the store once per
 *                 group of <= 8 queries, so it is slow for large batches.
 * m == 0, or every count 0: ids and float64 keys of filled slots are those of radad_knn_search_f64 on the same handle, bit for bit;
 * the padding is this family's.
 * Like radad_knn_search_excl_scan the call posts no certificate report, takes no turn off the tuning state and leaves
 * radad_knn_tuning_info as it found it; radad_knn_last_recheck / _last_certificate keep describing the last plain search; it may
 * build the plane.  After it radad_knn_last_emitted counts the rows the scan EMITTED per query, the ones the scrub cleared included.
 * Errors: RADAD_EINVAL before anything is enqueued for m outside [0, RADAD_EXCL_PQ_MAX_TAGS], for m > 0 with NULL q_tags_dev or
 * row_tags_dev, on a handle with a begun search, or beyond the width x k limit; RADAD_ESTATE on an empty store; nq == 0 returns
 * RADAD_OK.  Stream-ordered and serialised like every search.
 * Measured (tools/bench_excl_scan_pq.py, profiles/README.md; 1 M x 512 cosine, 1024 queries, k = 10, every query excluding its own
 * speaker of c rows): 1.19 / 1.26 / 1.58 ms at c = 0 / 200 / 1500 against 0.97 / 1.04 / 1.07 ms for the plain search of the same
 * handle (+22 / +21 / +48 %), all queries certified in the scan; radad_knn_search_excl_pq at k_fetch = min(1024, k + c) takes 469 ms
 * at c = 200 (fp32 tile kernels at k_fetch = 210) and 4.6 s at c = 1500 (every query in the exact pass).  The +22 % at c = 0 is the
 * 4096-entry buffers, not the scrub: they let the 1 M-row store through in ONE scan launch behind the sample's floor (knn_hi_one_go)
 * where the plain search's 1024-entry buffers take two, and that launch emits ~1070 rows per query.
 * Not offered: a begin / finish pair; a batch-wide set combined with per-query sets; a certified route for <= 16 queries. */
int radad_knn_search_excl_scan_pq(radad_knn_t h, const void* q_dev, int q_dtype, int64_t nq, int k,
                                  const int64_t* row_tags_dev /*[ntotal], by id - id_base*/,
                                  const int64_t* q_tags_dev /*[nq, m] row-major; any order, duplicates allowed*/, int m,
                                  const int32_t* q_tag_counts_dev /*[nq] or NULL = m for every query*/, float* out_dist_dev /*[nq,k]*/,
                                  int64_t* out_idx_dev /*[nq,k]*/, double* out_key_dev /*[nq,k] or NULL*/, void* stream);

/* Certified range search: EVERY row within a radius of each query, exactly -- faiss's index.range_search on the flat store.  The
 * reference has only the top-k call (vector_database.py:181) and audits leakage and self-retrieval by file BASENAME
 * (validate_no_leakage, pipeline.py:1105-1110; the exclude_self path of retrieve_similar_vectors, pipeline.py:478-515): a re-encoded
 * or renamed copy of a clip passes both.  "Which stored rows have cosine > 0.98 with this clip" is a range search; over-fetching a
 * guessed k and cutting afterwards is wrong whenever more than k copies exist.
 * Membership: row r is within the radius of query j iff its float64 key passes the threshold STRICTLY, as faiss does --
 *   L2: sum (q - y)^2 < (double)radius;   IP / cosine: q.y > (double)radius
 * -- the key being the value radad_knn_search_f64 reports in out_key, same sign convention; cosine normalises the query in fp32 as
 * every search does; the stored rows are what radad_knn_reconstruct returns.  An infinite radius is legal and means every row (+inf
 * for L2, -inf for IP).
 * Outputs, M = max_per_query: out_count[j] is the EXACT number of rows within the radius, also when it exceeds M; slots
 * 0 .. min(count, M) - 1 hold the best rows ordered by (key, lower id), id = id_base + row, out_dist the key rounded once; the
 * remaining slots hold -1 / NaN / NaN (the padding of the _excl family, not +-inf).
 * Routes, chosen on the host (knn_range_plan, knn_plan.h), reported by radad_knn_last_range:
 *   RADAD_RANGE_TILE   exactly when knn_excl_scan_route says tile at k = 1, whatever M is: 17 or more queries, dim % 64 == 0, the
 *                 plane on, at least 16 384 rows, the handle not on its fp32 fallback.  The plain search's query preparation, RSC
 *                 and bias; k_range_floor writes the admission floor T - eps(q), two ulps lower (T = radius for IP / cosine,
 *                 -radius for L2; eps(q) the scan's measured error bound): exact score >= T implies scan score >= T - eps, so every
 *                 row within the radius is emitted.  No floor is derived from rows: no sample pre-pass, no floor kernels, ONE scan
 *                 launch over 4096-entry candidate buffers, early abandon included (it compares the scan's partial sums with the
 *                 floor the emit uses, whatever the floor came from).  k_range_refine, one workgroup per query, re-scores ALL
 *                 emitted rows in float64 from the stored rows, applies the strict test, counts, sorts the rows that pass by
 *                 (key, id) in LDS (48 KB) and writes the best M.  A query that emitted more than 4096 rows proves nothing: it goes,
 *                 driven from the device, to the exact range kernel.
 *   RADAD_RANGE_STREAM only with RADAD_KNN_OPT_RANGE_SMALLQ set (default 0), and then exactly when the tile route is not taken, the
 *                 handle is not on its fp32 fallback and the plain search of the batch could stream the plane: <= 16 queries,
 *                 dim % 64 == 0, at least 16 384 rows, the plane on, RADAD_KNN_OPT_SMALLQ_HI set, the f16 query block within the LDS
 *                 (16 queries of dim 5376 are not: they take the tile route, as before).  The small-batch search's query
 *                 preparation and eps, the same k_range_floor, then ONE launch of k_range_hi_smallq: the stream body of
 *                 k_knn_hi_smallq (queries in LDS, one wave per row slice, 16 rows per step, two MFMA chains) without lists -- a row
 *                 whose score reaches its query's floor takes a slot of the query's 4096-entry buffer with one returning atomic.
 *                 The same overflow rule and exact pass; the re-rank is k_range_refine's exact-order instantiation, whose float64
 *                 re-score adds a row's products in the exact range kernel's order and with its roundings: counts, ids and the
 *                 float64 keys of such a batch are, bit for bit, what RADAD_RANGE_EXACT returns for it (the plain re-rank's keys
 *                 are 1 - 2 units of the last place off beyond 64 elements).  One wave per slice whatever the store: the
 *                 K-split form of the plain small-batch search (small stores of wide rows) has no range kernel.
 *   RADAD_RANGE_EXACT  every other shape: k_exact_scan_any<false, false, true> for every query -- the float64 key of every row, the
 *                 strict test before the list insertion, one count per wave and slice added to out_count, top-M lists merged as in
 *                 any exact pass.  Correct everywhere; it streams the store once per group of <= 8 queries.
 * The call posts no certificate report, takes no turn off the tuning state and leaves radad_knn_tuning_info, radad_knn_last_recheck
 * and radad_knn_last_certificate as it found them; it may build the plane.  After a tile-route call radad_knn_last_emitted reports
 * the rows emitted per query and the floors T - eps, and radad_knn_last_abandon the one launch's tile tasks; after a stream-route
 * call radad_knn_last_emitted reports the same, radad_knn_last_launch the stream's workgroups, and there are no tile tasks.
 * Errors, before anything is enqueued (outputs untouched, the handle usable): RADAD_EINVAL for M outside [1, RADAD_KNN_MAX_K], beyond
 * the width x k limit with M for k, for a NaN radius, NULL out_count / out_dist / out_idx, or a handle with a begun search;
 * RADAD_ESTATE on an empty store; nq == 0 returns RADAD_OK.  Stream-ordered and serialised like every search.
 * radad_knn_last_range synchronises with the most recent range call: its batch size (may be NULL), route and the number of queries
 * the exact kernel answered (all of them on the exact route); 0 / RADAD_RANGE_EXACT / 0 before the first one.
 * Measured (tools/bench_range.py, profiles/README.md, "Range search"; 1 M x 512 cosine, 1024 queries, threshold 0.9, M = 128, one
 * run on one MI355X): 0.86 / 0.88 / 1.42 ms with 0 / 10 / 1000 rows above the threshold per query against 0.98 / 0.99 / 1.04 ms for
 * the plain k = 10 search of the same handle -- cheaper than the plain search while few rows pass (no sample pre-pass, one launch),
 * +37 % at 1000 hits (the re-score reads ~2 KB of row per emitted row: 0.36 ms; the scan's emits: +0.25 ms).  The scan's eps on that
 * store: 5.5e-4.  Not measured: stores on which the early abandon skips tiles.
 * Measured, <= 16 queries (tools/bench_range_smallq.py, profiles/README.md, "Range search", small batches; the same store shape, 1 / 8 /
 * 16 queries, one run on one MI355X, the three legs alternated on one handle).  RADAD_RANGE_STREAM: 0.18 / 0.18 / 0.18 ms with no row
 * above the threshold, 0.19 / 0.19 / 0.20 ms with 10, 0.38 / 0.37 / 0.42 ms with 1000 per query (the stream launch 0.17 - 0.24 ms, the
 * re-rank of 1000 emitted rows per query 0.18 ms).  RADAD_RANGE_EXACT on the same handle: 3.6 / 10.9 / 10.8 ms whatever passes -- the
 * stream takes 2 - 5 % of it.  The plain k = 10 search of the same handle (k_knn_hi_smallq<16>): 0.23 / 0.28 / 0.33 ms.  The default
 * of RADAD_KNN_OPT_RANGE_SMALLQ is still 0: switching it is a change of its own.
 * Not offered: a begin / finish pair and sharded range search (a shard's answer is exact: concatenating the shards' lists is the
 * merge); results beyond RADAD_KNN_MAX_K per query (the count is exact: the caller can narrow the radius).  The IVF index has its
 * own calls, radad_ivf_range_search and radad_ivf_range_search_excl / _excl_pq below; still not offered on IVF: M > 128.
 * Exclusion sets combined with a radius: the two calls below. */
#define RADAD_RANGE_TILE 0
#define RADAD_RANGE_EXACT 1
#define RADAD_RANGE_STREAM 2
int radad_knn_range_search(radad_knn_t h, const void* q_dev, int q_dtype, int64_t nq, float radius, int max_per_query,
                           int32_t* out_count_dev /*[nq]*/, float* out_dist_dev /*[nq,M]*/, int64_t* out_idx_dev /*[nq,M]*/,
                           double* out_key_dev /*[nq,M] or NULL*/, void* stream);
int radad_knn_last_range(radad_knn_t h, int64_t* n_queries, int* route, int* n_exact);

/* Certified range search among the rows a query does not exclude: every ADMISSIBLE row within the radius, exactly.  The audit of a
 * store by file or by speaker ("which rows of ANOTHER speaker lie within cosine 0.98 of this clip") is this call: filtering the plain
 * range search's lists afterwards leaves the count of the unfiltered set and lets a clip's own copies or a speaker's 1500 rows take
 * every one of the M slots.
 * Outputs: radad_knn_range_search's, word for word, over the admissible rows -- out_count[j] is the EXACT number of admissible rows
 * within the radius (strict float64 membership), also beyond M = max_per_query; slots 0 .. min(count, M) - 1 hold the best admissible
 * rows ordered by (key, lower id); -1 / NaN / NaN behind them.  An excluded row is never counted and never takes a slot.
 *   radad_knn_range_search_excl     ONE set for the batch; arguments and NULL rules of radad_knn_search_excl_scan (row_tags_dev and
 *                 excl_sorted_dev, ascending, may be NULL only when n_excl == 0).
 *   radad_knn_range_search_excl_pq  one set of at most RADAD_EXCL_PQ_MAX_TAGS tags PER QUERY; the admissibility rule of
 *                 radad_knn_search_excl_scan_pq (counts clamped on the device to [0, m], NULL counts = m, any order, repeats allowed).
 * Tags are indexed by id - id_base.  With n_excl == 0, m == 0 or every count 0 the counts, ids and float64 keys are those of
 * radad_knn_range_search on the same handle, bit for bit.
 * Routes: radad_knn_range_search's (knn_range_excl_plan, knn_plan.h: knn_excl_scan_route at k = 1, 4096-entry buffers, one scan
 * launch), reported by radad_knn_last_range, which describes whichever of the three range calls ran last.
 *   RADAD_RANGE_TILE, one set for the batch: the bitmap and per-call bias pre-pass of radad_knn_search_excl_scan (NaN for excluded
 *                 rows; 12 bytes read and 4 written per row), the queries prepared for the biased instantiation (RSC 2 / 3, a zero
 *                 query constant without a centre) so that eps is that instantiation's own, k_range_floor, one scan launch with the
 *                 bias.  A NaN score passes no compare: excluded rows are never emitted, k_range_refine runs unchanged, and the
 *                 buffers hold admissible rows only.  Early abandon: as for any per-call bias (knn_abandon_launch: not taken).  A
 *                 query that still overflows goes, driven from the device, to k_exact_scan_any<true, false, true> with the bitmap.
 *   RADAD_RANGE_TILE, one set per query: the plain range search's launch -- its floors, RSC and early abandon; the scan emits excluded
 *                 rows like any others.  No k_excl_pq_scrub (it serves k_kth_floor, which a range search never runs): the re-rank's
 *                 per-query form stages the query's live tags in LDS and drops an emitted row whose tag is among them while it
 *                 compacts the buffer, so excluded rows are never re-scored, counted or sorted.  Overflow stays "emitted more than
 *                 the buffer holds, excluded rows included": such a query goes to k_exact_scan_any<true, true, true> with the query
 *                 tags.  m == 0 takes the plain range path outright.  radad_knn_last_emitted counts the emitted rows, excluded ones
 *                 included.
 *   RADAD_RANGE_STREAM (RADAD_KNN_OPT_RANGE_SMALLQ, <= 16 queries), one set for the batch: the same bitmap and bias pre-pass, the
 *                 queries prepared for the biased instantiation, and k_range_hi_smallq reads the per-call bias as its row bias: a NaN
 *                 score passes no compare, also against a floor of -inf.  One set per query: the plain stream launch and
 *                 k_range_refine's per-query form, as on the tile route.  Overflow goes to the same exact kernels.
 *   RADAD_RANGE_EXACT: those exact kernels for every query.  With both a radius and a filter the strict test, the count and the list
 *                 insertion happen only for the queries that admit the row; a row nobody admits is not loaded.
 * State: as the sibling calls -- KnnTuning is read (hi_skip), never written; no certificate report, no turn off the tuning state;
 * radad_knn_tuning_info, radad_knn_last_recheck and radad_knn_last_certificate are left as found; the call may build the plane.
 * Errors, before anything is enqueued (outputs untouched, the handle usable): RADAD_EINVAL for everything radad_knn_range_search
 * refuses, for m outside [0, RADAD_EXCL_PQ_MAX_TAGS], for m > 0 or n_excl > 0 with NULL tag arrays (n_excl < 0 too); RADAD_ESTATE on
 * an empty store; nq == 0 returns RADAD_OK.  Stream-ordered and serialised like every search.
 * Measured (tools/bench_range_excl.py, profiles/README.md, "Range search with exclusion"; 1 M x 512 cosine, 1024 queries, threshold
 * 0.9, M = 128, 10 admissible rows above the threshold per query, one run on one MI355X, each call alternated with
 * radad_knn_range_search on the same handle).  Per query, every query excluding its own speaker of c rows above the threshold:
 * 0.87 / 0.93 / 1.22 ms at c = 0 / 200 / 1500 against 0.87 / 0.97 / 1.79 ms for the plain range search (which counts and re-scores
 * the speaker's rows): equal at c = 0, cheaper with a crowd, because the re-rank drops it before the float64 re-score.  One set for
 * the batch with 0 / 50 / 90 % of the rows excluded: 0.90 / 0.88 / 0.85 ms against 0.87: at 0 % the biased instantiation's scan
 * launch is 0.03 ms slower than the plain one (RSC 3 instead of RSC 0 on an un-centred cosine store) and the two pre-pass launches
 * come on top; excluded rows emit nothing, so the cost falls as the set grows.
 * Not offered: a begin / finish pair; a batch-wide set combined with per-query sets; the IVF index. */
int radad_knn_range_search_excl(radad_knn_t h, const void* q_dev, int q_dtype, int64_t nq, float radius, int max_per_query,
                                const int64_t* row_tags_dev /*[ntotal], by id - id_base*/,
                                const int64_t* excl_sorted_dev /*[n_excl] ascending, NULL when n_excl == 0*/, int64_t n_excl,
                                int32_t* out_count_dev /*[nq]*/, float* out_dist_dev /*[nq,M]*/, int64_t* out_idx_dev /*[nq,M]*/,
                                double* out_key_dev /*[nq,M] or NULL*/, void* stream);
int radad_knn_range_search_excl_pq(radad_knn_t h, const void* q_dev, int q_dtype, int64_t nq, float radius, int max_per_query,
                                   const int64_t* row_tags_dev /*[ntotal], by id - id_base*/,
                                   const int64_t* q_tags_dev /*[nq, m] row-major; any order, duplicates allowed*/, int m,
                                   const int32_t* q_tag_counts_dev /*[nq] or NULL = m for every query*/, int32_t* out_count_dev /*[nq]*/,
                                   float* out_dist_dev /*[nq,M]*/, int64_t* out_idx_dev /*[nq,M]*/, double* out_key_dev /*[nq,M] or NULL*/,
                                   void* stream);

/* ------------------------------------------------------------------------------------------------
 * Inverted-file flat index: faiss.IndexIVFFlat(IndexFlatL2 quantiser, d, nlist, METRIC_L2), the reference's optional
 * `vector_db_index_type == "IVF"` (vector_database.py:65-70 create with nlist = max(64, ivf_nlist), :124-128 train on the
 * first <= 50 000 rows, :174-179 nprobe = config.vector_db_nprobe).  dim must be a multiple of 32, k <= 128: up to k = 26 the
 * probed lists are scanned; 27..128 is answered by the exact certified scan of the same rows (recall 1.0).
 * A search returns the exact top-k (squared L2, ties to the lower id) among the rows of the nprobe lists whose
 * centroids are nearest to the query; -1 / +inf where those lists hold fewer than k rows.
 * ---------------------------------------------------------------------------------------------- */
typedef struct radad_ivf_s* radad_ivf_t;
int radad_ivf_create(int dim, int nlist, int device, radad_ivf_t* out);
int radad_ivf_destroy(radad_ivf_t h);
int radad_ivf_is_trained(radad_ivf_t h, int* trained);
int radad_ivf_ntotal(radad_ivf_t h, int64_t* n);
int radad_ivf_nlist(radad_ivf_t h, int* nlist);
/* k-means (Lloyd, `niter` iterations; faiss trains its IVF quantiser with 10) on n training rows; synchronous.
 * Initial centroid c is training row (c * n) / nlist (rows repeat when n < nlist).  Every iteration assigns each row to its nearest
 * centroid -- the float64 argmin, the lower id on a tie: the assignment is a certified flat search -- and replaces every non-empty
 * list's centroid by the fp32 mean of its rows, summed in insertion order and divided once: within gamma_(m-1) sum|x| / m + u |mean|
 * of the exact mean for a list of m rows (u = 2^-24, gamma_k = k u / (1 - k u)); an empty list keeps its centroid.  Deterministic.
 * NON-FINITE ROWS are refused: a training row with a NaN or an infinity has no nearest centroid, and the call returns RADAD_EINVAL
 * naming the first such row.  The index is then exactly as it was: untrained, or with its previous centroids and quantiser.  With
 * niter = 0 only the nlist picked rows are read, so only those are checked.  The same holds for radad_ivf_add: the whole batch is
 * refused (first bad row named), nothing is appended.  faiss differs: it counts such a row in ntotal and puts it in no list. */
int radad_ivf_train(radad_ivf_t h, const float* rows_dev, int64_t n, int niter, void* stream);
/* install centroids computed elsewhere ([nlist, dim] fp32) instead of training; only on an empty index */
int radad_ivf_set_centroids(radad_ivf_t h, const float* centroids_dev, void* stream);
int radad_ivf_centroids(radad_ivf_t h, float* out_dev, void* stream);
/* list of every stored row, in insertion order (host int32 [ntotal]) */
int radad_ivf_assignments_host(radad_ivf_t h, int32_t* out_host, int64_t cap);
/* synchronous.  Every row goes to the list of its nearest centroid (float64 argmin, the lower id on a tie), whatever the batch it
 * arrives in.  A batch with a non-finite row is refused as a whole (RADAD_EINVAL, see radad_ivf_train). */
int radad_ivf_add(radad_ivf_t h, const float* rows_dev, int64_t n, void* stream);
int radad_ivf_search(radad_ivf_t h, const float* q_dev, int64_t nq, int k, int nprobe, float* out_dist_dev,
                     int64_t* out_idx_dev, void* stream);      /* asynchronous on `stream` (the (query, probe) pairs are grouped by list on
                                                                    the device); only the first search after an add rebuilds the list layout
                                                                    synchronously */
/* The exclusion-aware IVF search: for every query the exact top-k by squared L2 among the rows of its nprobe probed lists
 * (vector_database.py:174-179) whose tag is NOT in the exclusion set -- the reference's "search K + 10, drop the excluded basenames,
 * pad" (pipeline.py:478,491-515) without the padding it leaves when more than 10 excluded rows precede a query's K-th admissible
 * neighbour (a batch of clips of few speakers excluding each other; the training_file_ids mode, :500-502, where most of the store is
 * excluded).  The admission test sits INSIDE the list scans: a per-call bitmap by list-major position (one bit per stored row, built
 * on `stream` after the layout is up to date) makes an excluded row no part of the universe -- never emitted, listed or inserted,
 * never counted towards a bound -- so both list scans' certificates and the exact float64 list scan behind them hold as they stand,
 * over fewer rows, and the cost does not depend on how many excluded rows crowd a query.  (The flat recipe, over-fetch + certify + exact
 * pass, does not carry over: the list scans hold k + 6 <= 32 entries per (query, list), so K = 15 could over-fetch 11 rows at most.)
 *   order    (float64 distance, lower id), as radad_ivf_search
 *   padding  slots beyond the admissible rows of the probed lists hold id -1 and distance NaN (radad_filter_topk's and
 *            radad_knn_search_excl's padding, not the +inf of radad_ivf_search)
 *   n_excl == 0: ids and the distances of filled slots are bit-identical to radad_ivf_search
 * k in [1, 26], the range the list scans hold; a larger k is RADAD_EINVAL (it is NOT forwarded to the flat store as radad_ivf_search
 * does: that ignores nprobe and answers another question).  row_tags_dev [ntotal] int64 by insertion id, excl_sorted_dev [n_excl]
 * int64 ASCENDING (the caller's contract, not checked); both may be NULL only when n_excl == 0.  An untrained index is RADAD_EINVAL;
 * a trained index without rows returns all -1 / NaN.  Stream-ordered, serialised by the handle's mutex and ordered against searches
 * on other streams exactly as radad_ivf_search; radad_ivf_last_search_info / _counts describe it when it was the most recent search
 * on the handle, radad_ivf_last_search_exact reports 0. */
int radad_ivf_search_excl(radad_ivf_t h, const float* q_dev, int64_t nq, int k, int nprobe,
                          const int64_t* row_tags_dev /*[ntotal], by insertion id*/,
                          const int64_t* excl_sorted_dev /*[n_excl] ascending*/, int64_t n_excl,
                          float* out_dist_dev, int64_t* out_idx_dev, void* stream);
/* radad_ivf_search_excl with one exclusion set PER QUERY, the rule of radad_knn_search_excl_pq: row r is admissible for query j iff
 * row_tags[r] is not among the first cnt_j entries of q_tags[j, :], cnt_j = q_tag_counts[j] clamped on the device to [0, m] (NULL = m
 * for every query); the tags of a query may come in any order and repeat.  The result of a query is a function of the query alone:
 * the exact top-k by squared L2 among the admissible rows of ITS nprobe probed lists, ordered by (float64 distance, lower id), padding
 * -1 / NaN; k in [1, 26], 0 <= m <= RADAD_EXCL_PQ_MAX_TAGS.
 *   m == 0, or no query excludes a stored row: ids and the distances of filled slots are bit-identical to radad_ivf_search
 *   every query carries the same set S:        bit for bit radad_ivf_search_excl with S sorted
 * How: the list kernels keep ONE bit per list-major position in their inner loops, as radad_ivf_search_excl does, with a weaker
 * meaning -- set = no query of the batch excludes the row.  A pre-pass on `stream` hashes every live tag of the batch into a bitset
 * (two hashes, sized from nq * m so that under 1 % of the rows nobody excludes look suspect) and tests every position's tag against
 * it; a row whose bit is clear is decided exactly per (row, query) in a branch of the kernels, against the query's tags held in LDS
 * (in registers across a wave in the exact float64 list scan).  For every query an excluded row is never emitted, listed or inserted
 * and never counts towards a bound of THAT query, so both certificates hold per query as they stand.  A batch in which no stored row
 * is suspect costs the pre-pass and radad_ivf_search_excl's scan.  The frequent-suspect case -- a tag carried by many rows, e.g. a
 * speaker's, so that most steps take the branch -- costs more; what both cost on an MI355X is measured by tools/bench_ivf.py's
 * excl_pq_ms leg and written down in profiles/README.md.
 * RADAD_EINVAL: m outside its range, k > 26, NULL q_tags_dev or row_tags_dev with m > 0, an untrained index.  A trained index
 * without rows returns all -1 / NaN.  Stream-ordered and serialised like every IVF search; the tag arrays must stay alive until the
 * call's device work ends.  radad_ivf_last_search_info / _counts describe it, radad_ivf_last_search_exact reports 0.
 * Not offered: k > 26, m > 64, a batch-wide set combined with per-query sets in one call, sharded IVF. */
int radad_ivf_search_excl_pq(radad_ivf_t h, const float* q_dev, int64_t nq, int k, int nprobe,
                             const int64_t* row_tags_dev /*[ntotal], by insertion id*/,
                             const int64_t* q_tags_dev /*[nq, m] row-major; any order, duplicates allowed*/, int m,
                             const int32_t* q_tag_counts_dev /*[nq] or NULL = m for every query*/,
                             float* out_dist_dev, int64_t* out_idx_dev, void* stream);
/* 1 if the most recent radad_ivf_search was answered by the exact scan of the index's flat store (26 < k <= 128): every row an IVF
 * search could return AND the ones its probing would have missed -- a superset of faiss.IndexIVFFlat's answer (which holds only rows
 * of the nprobe lists, vector_database.py:174-179), at the flat scan's cost, nprobe ignored.  0: the nprobe lists were scanned. */
int radad_ivf_last_search_exact(radad_ivf_t h, int* exact_out);
/* which list scan answered the most recent radad_ivf_search, and how many of its queries that scan's certificate rejected
 * (synchronises with that search).  Either scan is a FILTER: the float64 re-rank certifies per query that no row of the probed lists
 * it did not see can reach the k-th, and the queries it cannot certify are answered in the same call by the exact float64 scan of
 * their probed lists -- every result is the float64 brute force over the probed lists.
 *   RADAD_IVF_SCAN_F32         fp32 rows, v_mfma_f32_16x16x4_f32, k + 6 candidates per (query, list); float64 re-rank of everything within
 *                              2 eps of the k-th best fp32 score, eps = (dim + 16) 2^-23 (2 |q||y|max + |y|max^2) over the probed lists
 *                              (dim % 64 != 0, no f16 plane, RADAD_IVF_OPT_HI_SCAN 0)
 *   RADAD_IVF_SCAN_HI          the flat store's f16 plane gathered list-major, certified per query as the flat scan is
 *   RADAD_IVF_SCAN_EXACT_FLAT  k > 26: the exact scan of the flat store (radad_ivf_last_search_exact) */
#define RADAD_IVF_SCAN_F32 0
#define RADAD_IVF_SCAN_HI 1
#define RADAD_IVF_SCAN_EXACT_FLAT 2
int radad_ivf_last_search_info(radad_ivf_t h, int* kind_out, int* rejected_out);
/* the same count, and how many queries of the most recent search the exact float64 list scan answered (all the rejected ones) */
int radad_ivf_last_search_counts(radad_ivf_t h, int* rejected_out, int* exact_out);
/* RADAD_IVF_OPT_HI_SCAN 1 (default) / 0: list scans over the f16 plane / over the fp32 rows (A/B measurements; same results);
 * 2 (tests): the f16 scan runs and every query is then treated as rejected by its certificate, i.e. answered by the exact list scan */
#define RADAD_IVF_OPT_HI_SCAN 0
/* RADAD_IVF_OPT_PQ_FILTER 1 (default) / 0 (tests): radad_ivf_search_excl_pq's pre-pass marks the rows some query may exclude / is
 * skipped and every row counts as suspect, so the per-(row, query) test decides every row.  Same results, bit for bit. */
#define RADAD_IVF_OPT_PQ_FILTER 1
int radad_ivf_set_option(radad_ivf_t h, int option, int value);

/* Certified range search over the probed lists: every row of the nprobe lists nearest to each query that lies within a radius,
 * exactly -- faiss's range_search on an IndexIVFFlat (the reference's third index type, vector_database.py:65-70, searched at
 * nprobe, :174-181), which the near-duplicate audit of a store (validate_no_leakage, pipeline.py:1105-1110) needs on the index a
 * user picks because the store is too large to scan whole.  The answer is the exact range search restricted to the union of the
 * probed lists, as radad_ivf_search is the exact top-k restricted to them; with nprobe == nlist it equals radad_knn_range_search on
 * the same rows.  L2 only (an IVF index has no other metric).
 * Every output rule of radad_knn_range_search holds: the key is the float64 sum (q - y)^2 over the stored fp32 values; a row is a
 * member iff key < (double)radius, strictly (a NaN key never passes; radius +inf = every row of the probed lists); out_count[j] is
 * the EXACT number of members, also beyond M = max_per_query; slots 0 .. min(count, M) - 1 hold the best members ordered by (key,
 * lower insertion id) -- insertion ids, not list positions, also in the tie-break --, out_dist the key rounded once to float32; all
 * other slots hold -1 / NaN / NaN.  M lies in [1, 128].
 * Routes, chosen on the host (ivf_plan_range, ivf_plan.h), reported by radad_ivf_last_range:
 *   RADAD_IVF_RANGE_HI     exactly when radad_ivf_search would take the certified f16 list scan (RADAD_IVF_SCAN_HI).  That route's query
 *                 preparation and eps(q); k_range_floor writes thr[q] = -radius - eps(q), two ulps lower; k_ivf_range_hi has the task,
 *                 split and chunk structure of the top-k list scan without its selection, carry and running bound (and so without
 *                 its score tile in LDS): a (row, query) pair whose f16 score reaches thr[q] takes a slot of the query's buffer of
 *                 4096 positions with one returning atomic.  k_ivf_range_refine, one workgroup per query, re-scores every emitted
 *                 position in float64 from the list-major rows (the plain re-score of the flat range search's tile route: its keys
 *                 may differ from the exact route's in the last place or two, never in what the tests can tell), maps positions to
 *                 insertion ids, applies the strict test, counts, sorts the members by (key, id) in LDS and writes the best M.  A
 *                 query that emitted more than 4096 positions goes, driven from the device, to the exact pass.
 *   RADAD_IVF_RANGE_EXACT  every other shape (no plane: dim % 64 != 0, RADAD_IVF_OPT_HI_SCAN 0): k_ivf_range_exact for every query -- the
 *                 float64 key of every row of the probed lists, the strict test before the list insertion, one count per wave and
 *                 (query, list) pair added to out_count, top-M lists per pair merged by the pair that arrives last.
 * RADAD_IVF_OPT_HI_SCAN 2 (tests) sends every query to the exact pass behind the hi route.
 * Errors, before anything is enqueued (outputs untouched, the handle usable): RADAD_EINVAL for M outside [1, 128], a NaN radius,
 * nprobe < 1, NULL out_count / out_dist / out_idx or a plan the index refuses; RADAD_ESTATE for an untrained index.  nq == 0 returns
 * RADAD_OK; a trained index without rows answers count 0 and padding.  Stream-ordered and serialised like every IVF search.
 * radad_ivf_last_range synchronises with the most recent radad_ivf_range_search: its batch size, route, the number of queries the
 * exact pass answered (all of them on the exact route) and the largest number of positions one query emitted (0 on the exact
 * route); any of the four may be NULL.  RADAD_ESTATE when the most recent search of the handle was not a range search; in the
 * opposite case radad_ivf_last_search_info / _counts return RADAD_ESTATE (they describe a top-k search).
 * Measured (tools/bench_ivf_range.py, profiles/ivf_range.md; 1 M x 512 noise rows, nlist 4096, nprobe 32, M = 128, one run on one
 * MI355X, the three legs alternated on one store).  64 groups of near-identical queries: 0.09 / 0.68 / 1.52 ms for 1 / 256 / 1024
 * queries with no member, 0.10 / 0.75 / 1.64 ms with 10 per query, 0.23 / 0.98 / 1.95 ms with 1000 (the re-score of 1000 emitted
 * rows per query: 0.13 / 0.30 / 0.44 ms), against 0.14 / 1.07 / 1.90 ms for radad_ivf_search at k = 10 on the same handle and
 * queries -- 0.64 - 0.89 of it up to 10 members, 1.5 / 0.90 / 1.0 of it at 1000.  Unstructured queries, no member: 0.09 / 0.78 /
 * 1.63 ms against 0.15 / 1.13 / 1.93 ms.  No query left the hi route; max_emitted equalled the members.  The flat store's
 * radad_knn_range_search of the same rows: 3.58 ms for one query (no certified route by default), 0.30 / 0.89 ms for 256 / 1024 --
 * faster than both IVF calls on this store, whose list scans take four times what tools/bench_ivf.py records for its own.
 * Not measured: that tool's store, the exact route at this scale, buffers that overflow.
 * Exclusion sets combined with a radius: radad_ivf_range_search_excl / radad_ivf_range_search_excl_pq below.
 * Not offered: M > 128, sharded IVF. */
#define RADAD_IVF_RANGE_HI 0
#define RADAD_IVF_RANGE_EXACT 1
int radad_ivf_range_search(radad_ivf_t h, const float* q_dev, int64_t nq, int nprobe, float radius, int max_per_query,
                           int32_t* out_count_dev /*[nq]*/, float* out_dist_dev /*[nq,M]*/, int64_t* out_idx_dev /*[nq,M]*/,
                           double* out_key_dev /*[nq,M] or NULL*/, void* stream);
int radad_ivf_last_range(radad_ivf_t h, int64_t* n_queries, int* route, int* n_exact, int* max_emitted);

/* Certified range search among the rows of the probed lists that a query does not exclude: radad_ivf_range_search over the ADMISSIBLE
 * rows.  The near-duplicate audit of an IVF store asks how many OTHER rows lie within the radius; filtering radad_ivf_range_search's
 * lists afterwards leaves the unfiltered count, lets a clip's own segments or a speaker's rows take all M slots, and in the
 * training_file_ids mode (most of the store excluded) lets excluded rows alone push a query past its 4096-position buffer.
 * Outputs: every output rule of radad_ivf_range_search with "row of the probed lists" replaced by "admissible row of the probed lists"
 * -- float64 key over the stored fp32 values, member iff key < (double)radius strictly, out_count[j] the EXACT number of admissible
 * members also beyond M = max_per_query, slots 0 .. min(count, M) - 1 the best admissible members by (key, lower insertion id),
 * -1 / NaN / NaN behind them, M in [1, 128].  An excluded row is never counted, never listed and never takes a slot of a query's
 * candidate buffer, on either route: overflow, and so the cost, depends on the admissible rows near a query alone.
 *   radad_ivf_range_search_excl     ONE set for the batch, the rule of radad_ivf_search_excl: row_tags_dev [ntotal] by insertion id,
 *                 excl_sorted_dev [n_excl] ASCENDING (the caller's contract, not checked); both may be NULL only when n_excl == 0.
 *   radad_ivf_range_search_excl_pq  one set PER QUERY, the rule of radad_ivf_search_excl_pq: row r is admissible for query j iff
 *                 row_tags[r] is not among the first cnt_j entries of q_tags[j, :], cnt_j = q_tag_counts[j] clamped on the device to
 *                 [0, m] (NULL = m for every query); any order, repeats allowed; 0 <= m <= RADAD_EXCL_PQ_MAX_TAGS.
 *   n_excl == 0, m == 0, or no query excludes a stored row: the four outputs equal radad_ivf_range_search's bit for bit (same route)
 *   every query carries the same set S:                      _excl_pq equals _excl with S sorted, bit for bit
 * How: a range scan's floor thr[q] is fixed before the launch and no row sets a bound, so -- unlike the top-k list scans, which must
 * keep excluded rows out of their bounds and therefore fetch admission bits for every step -- admission is decided only for a (row,
 * query) pair that has already passed the score test.
 *   RADAD_IVF_RANGE_HI     k_ivf_range_hi<ADM>: the lane holding a pair at or above the floor asks, before it takes a slot, the pair's bit
 *                 of the admission bitmap (one set for the batch: k_admit_bitmap by list-major position, built on `stream` behind the
 *                 layout as in radad_ivf_search_excl) or compares the row's tag with its query's tags, staged per task in LDS behind
 *                 the f16 queries (one set per query).  The per-query form has NO pre-pass: no suspect bitmap, no hash bitset, and
 *                 RADAD_IVF_OPT_PQ_FILTER has no effect on it.  k_ivf_range_refine runs unchanged: everything emitted is admissible.
 *                 The tag block counts towards the scan's LDS; a shape whose top-k search with the same sets would leave the f16 list
 *                 scan takes the exact route.
 *   RADAD_IVF_RANGE_EXACT, overflow and RADAD_IVF_OPT_HI_SCAN 2: k_ivf_range_exact<ADM>, the admission test behind the strict radius
 *                 test and in front of the count and the list insertion, so only members pay for a tag gather -- the bit, or one
 *                 ballot per member against the query's tags held across a wave's lanes (lane t tag t).
 * Errors, before anything is enqueued (outputs untouched, the handle usable): RADAD_EINVAL for everything radad_ivf_range_search
 * refuses, for n_excl < 0, for m outside [0, RADAD_EXCL_PQ_MAX_TAGS], for NULL row_tags_dev or excl_sorted_dev with n_excl > 0, for NULL
 * row_tags_dev or q_tags_dev with m > 0; RADAD_ESTATE for an untrained index.  nq == 0 returns RADAD_OK; a trained index without rows
 * answers count 0 and padding.  Stream-ordered, serialised by the handle's mutex and ordered against searches on other streams like
 * every IVF search; the tag arrays must stay alive until the call's device work ends.  radad_ivf_last_range describes both calls with
 * the same four fields -- max_emitted counts admissible (row, query) pairs only --, and radad_ivf_last_search_info / _counts return
 * RADAD_ESTATE after either, as after radad_ivf_range_search.
 * Measured (tools/bench_ivf_range_excl.py, profiles/ivf_range_excl.md; 1 M x 512 noise rows, nlist 4096, nprobe 32, M = 128, 10 planted
 * rows of other files per query within the radius, one run on one MI355X, each leg alternated with radad_ivf_range_search on the same
 * handle; 1 / 256 / 1024 queries).  One set per query, every query excluding its own speaker of c rows within the radius: 0.104 /
 * 0.774 / 1.778 ms at c = 0 against 0.102 / 0.772 / 1.738 ms for the plain call (1.02 / 1.00 / 1.02 of it); 0.104 / 0.762 / 1.654 ms
 * at c = 200 (0.83 / 0.96 / 0.98); 0.104 / 0.719 / 1.493 ms at c = 1500 against 0.337 / 1.148 / 2.006 ms (0.31 / 0.63 / 0.74): the crowd
 * takes no slot and is never re-scored, max_emitted 10 instead of 1510.  One set for the batch covering 0 / 50 / 90 % of the rows:
 * 1.01 / 1.17 / 1.08 of the plain call for one query (the bitmap pre-pass over 1 M positions, 0.017 ms), 1.00 / 1.02 / 1.02 for 256,
 * 1.00 / 1.01 / 1.00 for 1024.  Not measured: buffers that overflow at this scale, the exact route at this scale, m = 64.
 * Not offered: M > 128, a batch-wide set combined with per-query sets in one call, sharded IVF, removal from an IVF store. */
int radad_ivf_range_search_excl(radad_ivf_t h, const float* q_dev, int64_t nq, int nprobe, float radius, int max_per_query,
                                const int64_t* row_tags_dev /*[ntotal], by insertion id*/,
                                const int64_t* excl_sorted_dev /*[n_excl] ascending, NULL when n_excl == 0*/, int64_t n_excl,
                                int32_t* out_count_dev /*[nq]*/, float* out_dist_dev /*[nq,M]*/, int64_t* out_idx_dev /*[nq,M]*/,
                                double* out_key_dev /*[nq,M] or NULL*/, void* stream);
int radad_ivf_range_search_excl_pq(radad_ivf_t h, const float* q_dev, int64_t nq, int nprobe, float radius, int max_per_query,
                                   const int64_t* row_tags_dev /*[ntotal], by insertion id*/,
                                   const int64_t* q_tags_dev /*[nq, m] row-major; any order, duplicates allowed*/, int m,
                                   const int32_t* q_tag_counts_dev /*[nq] or NULL = m for every query*/, int32_t* out_count_dev /*[nq]*/,
                                   float* out_dist_dev /*[nq,M]*/, int64_t* out_idx_dev /*[nq,M]*/, double* out_key_dev /*[nq,M] or NULL*/,
                                   void* stream);
int radad_ivf_reconstruct(radad_ivf_t h, const int64_t* idx_dev, int64_t n, float* out_dev, void* stream);

/* out[r] = the k-th largest of the groups x per_group values of row r, value (g, i) at in[(g n + r) per_group + i] -- the layout
 * [groups][n][per_group] an all-gather of the shards' [n][k] bound blocks has (groups = 1: plain [n][m]); groups x per_group <= 1280,
 * 1 <= k <= groups x per_group; NaN ranks lowest.  For the sharded search: the G k lower bounds per query gathered from G
 * shards' radad_knn_search_begin -> the bound radad_knn_search_finish takes. */
int radad_kth_largest(const float* in_dev, int64_t n, int groups, int per_group, int k, float* out_dev, int device, void* stream);
/* row L2 normalisation x / (|x| + 1e-12)  (vector_database.py:100-105); in-place allowed */
int radad_rownorm(const float* in_dev, float* out_dev, int64_t n, int dim, int device, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Embedding: segment -> front-end -> frame projection -> temporal pyramid pooling -> segment mean.
 *   segment plan          segmenter.py:8-39 (n_seg = max(1,(N-L)//hop+1); zero pad only when N < L)
 *   zero-mean/unit-var    feature_extractor.py:25-30 (HF Wav2Vec2FeatureExtractor, eps 1e-7)
 *   log-mel               feature_extractor.py:94-97 (HF WhisperFeatureExtractor: hann 400 / hop 160,
 *                         |X|^2, drop last frame, slaney mel 201->80, log10 clamp 1e-10, max-8, (x+4)/4)
 *   frame projection      stands where the pretrained encoder forward sits (feature_extractor.py:33,110,167)
 *   pooling               pooling.py:66-103 (adaptive max/avg bins, bin-major layout, levels concatenated)
 *   segment mean          pipeline.py:411
 * ---------------------------------------------------------------------------------------------- */
#define RADAD_MAX_LEVELS 8
typedef struct radad_embed_cfg {
    int32_t segment_length;    /* samples per segment (config.segment_length*sample_rate = 32000)   */
    int32_t hop_length;        /* int(segment_length*(1-overlap)) = 16000                            */
    int32_t normalize;         /* 1: per-segment zero-mean/unit-variance before the spectrogram      */
    int32_t n_fft;             /* must be 400                                                        */
    int32_t fft_hop;           /* must be 160                                                        */
    int32_t n_mels;            /* must be 80                                                         */
    int32_t padded_samples;    /* 0: spectrogram of the segment itself (segment_length/160 frames);
                                  otherwise zero-pad to this many samples first (HF pads to 480000)  */
    int32_t feat_dim;          /* F, multiple of 32                                                  */
    int32_t n_levels;          /* pyramid levels (config.tpp_levels)                                 */
    int32_t levels[RADAD_MAX_LEVELS];
    int32_t pool_mode;         /* RADAD_POOL_MAX / RADAD_POOL_AVG                                    */
} radad_embed_cfg;

typedef struct radad_embed_s* radad_embed_t;

/* mel_filters_host [201, 80] fp32 (bins x mels); proj_w_host [80, F] fp32; proj_b_host [F] fp32 */
int radad_embed_create(const radad_embed_cfg* cfg, const float* mel_filters_host, const float* proj_w_host,
                       const float* proj_b_host, int device, radad_embed_t* out);
/* same with a choice of log-mel kernel (for A/B measurements and parity tests): flags = 0 is radad_embed_create.  All give
 * feature_extraction_whisper.py:135-168 per segment; how closely, row by row against the float64 oracle on tones, a chirp, noise
 * floors, a gated clip, level and DC steps (tests/test_gpu_logmel_designed.py, profiles/logmel_designed.md; final (log10 + 4) / 4
 * units): k_logmel_fft_clip and k_logmel within the 1e-4 bar everywhere (worst 8.1e-5 and 4.6e-5).  The two f16-matrix-pipe kernels
 * within it except in cells 7 to 8 decades under the segment maximum of a pure tone over a quiet floor, where the tone's accumulated
 * rounding noise shows: k_logmel_h_clip up to 1.2e-4, k_logmel_h up to 1.6e-4 (numpy's float32 FFT: 2.1e-5).
 *   RADAD_EMBED_NO_SHARED_FRAMES  one transform per (segment, frame) even where overlapping segments share frames (k_logmel_h)
 *   RADAD_EMBED_LOGMEL_F32        the folded DFT on the fp32 matrix pipe, short sums met in float64 (k_logmel, ~3x slower than k_logmel_h)
 *   RADAD_EMBED_LOGMEL_DFT_GEMM   shared frames as a DFT-as-GEMM on the f16 matrix pipe (k_logmel_h_clip) instead of the radix FFT on the
 *                                 vector ALU (k_logmel_fft_clip, the default where the configuration allows sharing)
 * The environment variables RADAD_LOGMEL_SHARED=0, RADAD_LOGMEL_F32=1, RADAD_LOGMEL_FFT=0 set the same bits for extractors created
 * while they are set (announced once per process on stderr). */
#define RADAD_EMBED_NO_SHARED_FRAMES 1
#define RADAD_EMBED_LOGMEL_F32 2
#define RADAD_EMBED_LOGMEL_DFT_GEMM 4
int radad_embed_create_ex(const radad_embed_cfg* cfg, int flags, const float* mel_filters_host, const float* proj_w_host,
                          const float* proj_b_host, int device, radad_embed_t* out);
int radad_embed_destroy(radad_embed_t h);
int radad_embed_output_dim(radad_embed_t h, int* dim);     /* sum(levels)*F  (pooling.py:119-122)    */
int radad_embed_num_frames(radad_embed_t h, int* frames);   /* frames per segment                      */
/* number of segments the plan yields for a clip of n samples (segmenter.py:25) */
int64_t radad_segment_count(int64_t n_samples, int32_t segment_length, int32_t hop_length);
/* clip embeddings for a batch: clip b is wave_dev[clip_offsets_host[b] .. clip_offsets_host[b+1]).
 * out_dev [n_clips, output_dim] fp32.  (process_audio_batch, pipeline.py:392-414, minus file loading) */
int radad_embed_forward(radad_embed_t h, const float* wave_dev, const int64_t* clip_offsets_host, int64_t n_clips,
                        float* out_dev, void* stream);

/* same with a choice of output type: RADAD_OUT_BF16 emits the clip embeddings as bfloat16 (rounded to nearest even in
 * the epilogue of the pooling kernel; BASELINE config 5, the reference's reduced-precision knob feature_extractor.py:84,140) */
#define RADAD_OUT_F32 0
#define RADAD_OUT_BF16 1
int radad_embed_forward_ex(radad_embed_t h, const float* wave_dev, const int64_t* clip_offsets_host, int64_t n_clips,
                           void* out_dev, int out_dtype, void* stream);
/* clip offsets resident on the DEVICE (int64 [n_clips + 1]): the segment plan (segmenter.py:25-39: n_seg per clip,
 * exclusive scan, start / valid samples of every segment) is built by a kernel, nothing synchronises with the host.
 * n_samples_total (= clip_offsets[n_clips], known to the caller from the wave buffer's size) only bounds the number of
 * segments for buffer and grid sizes.
 * Offsets the plan kernel had to repair (radad_embed_plan_flags below): a clip whose own two offsets were valid and whose segments
 * all fit under the cap embeds exactly as in a clean batch (tests/test_gpu_embed_plan.py); the output rows of every other clip of
 * such a batch -- clamped, emptied, cut at the segment cap or behind the cut -- are written from inside the buffers but otherwise
 * UNSPECIFIED (today: the mean over whatever segments the clip kept, not a number for a clip that kept none). */
int radad_embed_forward_dev(radad_embed_t h, const float* wave_dev, const int64_t* clip_offsets_dev, int64_t n_clips,
                            int64_t n_samples_total, void* out_dev, int out_dtype, void* stream);
/* 16-bit PCM (what audio files hold) -> the float32 samples the reference's loader produces (pipeline.py / dataset.py: librosa.load,
 * i.e. sample / 32768, exact in fp32), on the device: upload the PCM, convert here, hand the result to radad_embed_forward* --
 * half the bytes over PCIe.  out_dev may not alias pcm_dev. */
int radad_pcm16_to_f32(const int16_t* pcm_dev, float* out_dev, int64_t n, int device, void* stream);
/* The device-resident offsets cannot be validated by the host without a synchronisation (the host path of
 * radad_embed_forward rejects bad offsets up front, as segmenter.py:18-19 raises on bad input).  The plan kernel therefore
 * REPAIRS them -- every clip is clamped into [0, n_samples_total], a clip that ends before it starts becomes empty, the
 * segment count is capped -- so no kernel reads outside the wave buffer, and records what it repaired.  This call waits for the
 * most recent radad_embed_forward_dev batch and returns (once) those flags: 0 = offsets were fine; bit 0 an offset outside
 * [0, n_samples_total]; bit 1 non-monotone offsets; bit 2 more segments than n_samples_total / hop + n_clips.  A non-zero
 * value means the embeddings of that batch are NOT those of the intended clips. */
int radad_embed_plan_flags(radad_embed_t h, int* flags_out);
/* The same without waiting: the flags of the device-offset batches that have COMPLETED since the last report (OR-ed; each batch is
 * reported once, by whichever of the two calls sees it first), and how many batches are still in flight.  A caller that queues batches
 * back to back polls before each one (it never blocks behind the previous batch) and calls radad_embed_plan_flags once after the
 * last. */
int radad_embed_plan_flags_poll(radad_embed_t h, int* flags_out, int* batches_pending_out);
/* Diagnostic (tests/test_gpu_embed_plan.py compares it with the host model tests/embed_plan_ref.py): the segment and chunk plan that
 * the handle's most recent radad_embed_forward* or stage call (radad_embed_normalize / _logmel / _frame_features) built, copied to the
 * host.  Waits for `stream` (the one that call was enqueued on); launches nothing, changes no plan and leaves the report ring of
 * radad_embed_plan_flags[_poll] alone -- the flags here are read from the plan itself, those calls report exactly as before.
 *   info8 = { n_clips, n_seg, n_chunks (0 when the call took no chunk plan), the repair flags of THIS plan (bits as above),
 *             seg_cap and chunk_cap the plan was built under (host offsets: the exact counts; device offsets: the bounds
 *             n_samples_total / hop + n_clips and the chunk bound derived from it; explicit segments: their number and 0),
 *             RADAD_PLAN_* (which entry built it), RADAD_PLAN_CHUNKS_* (the chunk geometry) }
 *   clip_seg_host  [n_clips + 1] first segment of every clip (explicit segments: one "clip" per segment); clip_capacity entries
 *   seg_start_host, seg_valid_host [n_seg] absolute first sample and real samples of every segment; seg_capacity entries each
 *   chunk_beg_host [n_chunks] int64 and chunk_fields_host [n_chunks][4] int32 = { seg0, n_seg, cidx, avail }: the work list of
 *             k_logmel_h_clip / k_logmel_fft_clip (first sample of the chunk's clip, the clip's first segment and the segments it
 *             kept, the chunk's index inside the clip, samples of the clip those segments cover); chunk_capacity entries
 * NULL array pointers: that array is not wanted (all NULL: info only, e.g. to size the arrays for a second call).  info8 is written
 * before the capacities are checked; an array that is too small is RADAD_EINVAL and nothing is copied.  RADAD_ESTATE before the first
 * plan. */
#define RADAD_PLAN_NONE 0
#define RADAD_PLAN_HOST_OFFSETS 1
#define RADAD_PLAN_DEVICE_OFFSETS 2
#define RADAD_PLAN_SEGMENTS 3
#define RADAD_PLAN_CHUNKS_NONE 0
#define RADAD_PLAN_CHUNKS_GEMM 1   /* k_logmel_h_clip: 104 interior frames per chunk   */
#define RADAD_PLAN_CHUNKS_FFT 2    /* k_logmel_fft_clip: 64 frame slots per chunk      */
int radad_embed_last_plan(radad_embed_t h, int64_t* info8, int64_t* clip_seg_host, int64_t clip_capacity, int64_t* seg_start_host,
                          int32_t* seg_valid_host, int64_t seg_capacity, int64_t* chunk_beg_host, int32_t* chunk_fields_host,
                          int64_t chunk_capacity, void* stream);
/* Which log-mel kernel the most recent embedding call took: 0 = one transform per (segment, frame) (k_logmel_h, or k_logmel under
 * RADAD_LOGMEL_F32); 1, 2 = the frames overlapping segments share were transformed once per CLIP (chosen by the configuration --
 * segment hop a multiple of 160 samples and smaller than the segment, Slaney filter bank -- for calls that hand over clips;
 * RADAD_LOGMEL_SHARED=0 turns it off): 2 = as a radix FFT on the vector ALU (k_logmel_fft_clip, the default), 1 = as a DFT-as-GEMM on
 * the f16 matrix pipe (k_logmel_h_clip: RADAD_LOGMEL_FFT=0, or a filter bank that is not triangular).  All give
 * feature_extraction_whisper.py:135-168 per zero-mean/unit-variance segment. */
int radad_embed_last_logmel_kind(radad_embed_t h, int* kind_out);
/* Diagnostic (tests/test_gpu_logmel_designed.py compares it row by row with the float64 oracle): the log-mel rows the handle's most
 * recent radad_embed_forward* or stage call computed, [S, frames, 80] fp32 with the segments in plan order, clamped with the handle's
 * own segment maxima and scaled (x + 4) / 4 exactly as radad_embed_logmel returns them -- the rows the projection kernel read.
 * Enqueues one small kernel on `stream` (the one that call was enqueued on) and changes nothing in the handle; the hot path does not
 * know about it.  *n_segments_out = S (device-resident offsets: the plan's own count, after waiting for `stream`), written before
 * the capacity is checked; out_dev NULL: the count alone.  RADAD_ESTATE when the handle holds no rows (no forward yet, or its
 * buffers were released), RADAD_EINVAL when segment_capacity < S (nothing is written to out_dev). */
int radad_embed_last_logmel(radad_embed_t h, float* out_dev, int64_t segment_capacity, int64_t* n_segments_out, void* stream);
/* How k_logmel_h_clip cuts a clip of n_segments segments (frames_per_segment frames each, segment hop = hop_frames frames) into
 * workgroup chunks -- host arithmetic only, no device needed (the kernel, the plan kernel and the host share it): out5 = { full
 * chunks of 104 interior frames, interior frames of the tail chunk, edge frames the tail chunk carries, edge-only chunks of <= 32
 * edge frames, total chunks }.  The clip has (n_segments - 1) hop_frames + frames_per_segment - 3 interior frames and
 * 3 n_segments edge frames (a segment's frames 0, 1 and T - 1). */
int radad_embed_clip_chunks(int n_segments, int frames_per_segment, int hop_frames, int32_t* out5);
/* The same for k_logmel_fft_clip (the shared-frame work list as a radix FFT on the vector ALU, csrc/logmel_fft.inc): chunks of 64
 * frame slots; out5 = { full chunks of 64 interior frames, interior frames of the tail chunk, edge frames the tail chunk carries,
 * edge-only chunks of <= 26 edge frames, total chunks }.  Host arithmetic only. */
int radad_embed_fft_clip_chunks(int n_segments, int frames_per_segment, int hop_frames, int32_t* out5);
/* The per-lane constant tables of k_logmel_fft_clip for a mel filter bank [201, 80] (host arithmetic only, no device needed;
 * tests/test_fft_tables.py drives a numpy restatement of the kernel's data flow with them and compares it with numpy.fft.rfft and the
 * oracle's log-mel).  tab_out must hold `cap` >= 2224 floats: 25 groups (index k1, or the sample group m for the window) of
 * [hann(16 m + 2 r), hann(16 m + 2 r + 1)] [cos, sin of W200^(r k1)] [cos, sin of W400^k, k = 25 k2 + k1] [fb[k][b] / 4,
 * fb[k][b + 1] / 4, byte offset of band b's slot in a row of the mel tile (int32 bits), 1 if the next bin starts at band b + 1
 * (int32 bits)], each for the 8 lanes of an octet (lane p holds the residue class r = p < 4 ? p : 11 - p of the packed frame and
 * ends with the bin block k2 = bitrev3(p)); then per lane the constants of the three exchange stages [g1, c1, s1, g2, c2, s2, g3, 0]:
 * own <- (own + g partner)(c + i s); then per band the byte offsets (int32) of the two row slots that add up to it.  info4 =
 * { 1 if the bank has the shape the sparse mel step needs (every bin feeds at most two adjacent bands, the band index never falls and
 * rises by at most one per bin, bin 200 weightless; otherwise the matrix-pipe kernels run), floats written, floats per row of the mel
 * tile, float offset of the band table }. */
int radad_embed_fft_tables(const float* mel_filters_host, float* tab_out, int cap, int32_t* info4);

/* same HIP-event timing for the two embedding kernels (k_logmel, k_proj_pool) of radad_embed_forward */
int radad_embed_profile(radad_embed_t h, int enable);
int radad_embed_profile_read(radad_embed_t h, float* logmel_ms_out, float* projpool_ms_out, int cap, int* n_out);

/* stage entry points, for parity with the reference's per-stage functions ------------------------ */
/* zero-mean/unit-var of S segments: seg s = wave_dev[seg_start_host[s] .. +seg_valid_host[s]) zero
 * padded to segment_length; out_dev [S, segment_length] */
int radad_embed_normalize(radad_embed_t h, const float* wave_dev, const int64_t* seg_start_host,
                          const int32_t* seg_valid_host, int64_t n_seg, float* out_dev, void* stream);
/* log-mel of S segments -> out_dev [S, frames, 80] (frame-major; HF returns [80, frames]) */
int radad_embed_logmel(radad_embed_t h, const float* wave_dev, const int64_t* seg_start_host,
                       const int32_t* seg_valid_host, int64_t n_seg, float* out_dev, void* stream);
/* frame features of S segments -> out_dev [S, frames, F]  (extract_features protocol) */
int radad_embed_frame_features(radad_embed_t h, const float* wave_dev, const int64_t* seg_start_host,
                               const int32_t* seg_valid_host, int64_t n_seg, float* out_dev, void* stream);

/* stand-alone temporal pyramid pooling of one or more [T_i, F] feature blocks stored back to back:
 * item i = feats_dev[row_offsets_host[i]*F .. row_offsets_host[i+1]*F); out_dev [n_items, sum(levels)*F]
 * (TemporalPyramidPooling.pool_features / pool_features_batch, pooling.py:88-117) */
int radad_tpp_forward(const float* feats_dev, const int64_t* row_offsets_host, int64_t n_items, int feat_dim,
                      const int32_t* levels, int n_levels, int pool_mode, float* out_dev, int device,
                      void* stream);
/* mean over groups of rows: out[g,:] = mean(in[group_offsets[g]..group_offsets[g+1], :])  (pipeline.py:411) */
int radad_group_mean(const float* in_dev, const int64_t* group_offsets_host, int64_t n_groups, int dim,
                     float* out_dev, int device, void* stream);

/* ------------------------------------------------------------------------------------------------
 * ProjectionLayer inference forward (projection.py:68-106), fused:
 *   s = W2 tanh(W1 x + b1) + b2; a = softmax_K(s); c = W4 relu(W3 x + b3) + b4; u = sum_K a c;
 *   out = W6 LN(W5 u + b5; eps 1e-6) + b6
 * Weights are given in torch nn.Linear layout ([out, in] row-major), device pointers.
 * One pass over x: a split-K GEMM against [W1;W3], then one block per batch row (csrc/proj.hip).
 * w54t / b54 hold the inference-time fold  W5 (W4 h + b4) + b5 = (W5 W4) h + (W5 b4 + b5): build them once
 * per set of weights with radad_projection_fold and keep them; when NULL the forward re-folds into its
 * workspace on every call (correct, slower).
 * Any dim >= 1 and any alignment of the pointers (4-byte float alignment) are accepted. Limits, each one
 * RADAD_EINVAL: hidden <= 4096; batch * k < 2^31 - 128; the per-row tail keeps
 * 4 * (2*k*hidden + 2*hidden + k + 8) bytes in LDS, at most 160 KB (k = 5: hidden <= 3412; k = 16: hidden <= 1204).
 * ---------------------------------------------------------------------------------------------- */
typedef struct radad_proj_weights {
    const float *w1, *b1;       /* attention_score   [H, D], [H]   */
    const float *w2, *b2;       /* attention_final   [1, H], [1]   */
    const float *w3, *b3;       /* cst_hidden        [H, D], [H]   */
    const float *w4, *b4;       /* cst_output        [D, H], [D]   */
    const float *w5, *b5;       /* weight_sum        [H, D], [H]   */
    const float *ln_g, *ln_b;   /* normalization     [H], [H]      */
    const float *w6, *b6;       /* unified_embedding [O, H], [O]   */
    const float *w54t, *b54;    /* optional fold: (W5 W4)^T [H(in), H(out)], W5 b4 + b5 [H]; NULL = fold per call */
} radad_proj_weights;
int radad_projection_forward(const radad_proj_weights* w, const float* x_dev /*[B,K,D]*/, int64_t batch, int k,
                             int dim, int hidden, int out_dim, float* out_dev /*[B,O]*/, float* workspace_dev,
                             int64_t workspace_bytes, int device, void* stream);
int64_t radad_projection_workspace_bytes(int64_t batch, int k, int dim, int hidden, int out_dim);
/* w54t_out_dev [H,H], b54_out_dev [H] from w->w4,b4,w5,b5 (float64 accumulation, rounded once) */
int radad_projection_fold(const radad_proj_weights* w, int dim, int hidden, float* w54t_out_dev, float* b54_out_dev,
                          int device, void* stream);

/* ------------------------------------------------------------------------------------------------
 * ProjectionLayer training forward and backward (projection.py:68-106 under autograd; csrc/proj_train.inc).
 *   forward:  p = W1 x + b1, t = tanh p, s = W2 t + b2, a = softmax_K s           (:69-71, :87)
 *             q = W3 x + b3, h = relu q, hbar = sum_K a h, u = W4 hbar + b4       (:74-76, :88-89; sum_K taken before W4)
 *             v = W5 u + b5, xh = LN-normalised v, n = xh g + beta                 (:94-99; biased variance, eps 1e-6)
 *             out = W6 (n * mask * inv_keep) + b6                                  (:100-101; dropout by the caller's mask)
 *   backward: the gradient of out with respect to all 14 parameters and, when asked for, x.
 * The fold pointers w54t / b54 of radad_proj_weights are ignored: the weights move every step.
 * mask_dev [B,H] holds 0 / 1 floats drawn by the caller; NULL means no dropout (inv_keep is then ignored).
 * The forward fills the saved-activation buffers, the backward reads them (with the same x, weights, mask and inv_keep).
 * A NULL pointer in radad_proj_grads skips that gradient (dw1 and dw3 come from one product: both or neither); dx_dev NULL
 * skips the input gradient.  No float atomics: every sum has a fixed order, two runs give the same bits.
 * Shapes as the inference forward (any dim, any 4-byte-aligned pointers); limits, each one RADAD_EINVAL: hidden and
 * out_dim <= 4096, dim <= 2^22 - 64, batch * k < 2^31 - 128, and the inference tail's LDS bound on k * hidden.  batch == 0 is
 * RADAD_OK without a launch.  One workspace size serves both calls; -1 for a bad shape.
 * ---------------------------------------------------------------------------------------------- */
typedef struct radad_proj_saved {
    float *t, *h;               /* tanh(p), relu(q)  [B*K, H]      */
    float *a;                   /* softmax weights   [B*K]         */
    float *hbar;                /* sum_K a h         [B, H]        */
    float *u;                   /* W4 hbar + b4      [B, D]        */
    float *xh;                  /* normalised v      [B, H]        */
    float *rstd;                /* 1 / sqrt(var+eps) [B]           */
} radad_proj_saved;
typedef struct radad_proj_grads {   /* shapes of the matching radad_proj_weights members */
    float *dw1, *db1, *dw2, *db2, *dw3, *db3, *dw4, *db4, *dw5, *db5, *dln_g, *dln_b, *dw6, *db6;
} radad_proj_grads;
int64_t radad_projection_train_workspace_bytes(int64_t batch, int k, int dim, int hidden, int out_dim);
int radad_projection_train_forward(const radad_proj_weights* w, const float* x_dev /*[B,K,D]*/, const float* mask_dev /*[B,H] or NULL*/,
                                   float inv_keep /* 1/(1-p) */, int64_t batch, int k, int dim, int hidden, int out_dim,
                                   const radad_proj_saved* saved, float* out_dev /*[B,O]*/, float* workspace_dev,
                                   int64_t workspace_bytes, int device, void* stream);
int radad_projection_backward(const radad_proj_weights* w, const float* x_dev, const float* mask_dev, float inv_keep,
                              const radad_proj_saved* saved, const float* grad_out_dev /*[B,O] contiguous*/, int64_t batch, int k,
                              int dim, int hidden, int out_dim, const radad_proj_grads* grads, float* dx_dev /*[B,K,D] or NULL*/,
                              float* workspace_dev, int64_t workspace_bytes, int device, void* stream);

/* out[r, :] = act(W x[r, :] + bias)   nn.Linear forward, W [out_features, in_features] with row stride ldw;
 * act 0 none / 1 tanh / 2 relu; bias_dev may be NULL.  Split-K MFMA GEMM (few rows x wide in_features still fills
 * the chip).  Any in_features, any strides with ldx, ldw >= in_features and ldo >= out_features, any 4-byte-aligned
 * pointers (16-byte-aligned pointers with in_features, ldx, ldw multiples of 4 take the vector-load path);
 * rows < 2^31 - 128.  Anything else is RADAD_EINVAL. */
int radad_linear_forward(const float* x_dev, int64_t ldx, const float* w_dev, int64_t ldw, const float* bias_dev,
                         int act, int64_t rows, int out_features, int in_features, float* out_dev, int64_t ldo,
                         float* workspace_dev, int64_t workspace_bytes, int device, void* stream);
int64_t radad_linear_workspace_bytes(int64_t rows, int out_features, int in_features);

/* ------------------------------------------------------------------------------------------------
 * RADADModel.forward after the projection (radad_model.py:38-41), inference:
 *   fused  = Wf cat[tpp, proj] + bf                      (:39; the concatenation is never built)
 *   logits = DetectionModel(fused)                       (:40; detection_model.py:41-72 in eval mode:
 *            per hidden layer Linear -> BatchNorm1d (running stats, given as scale/shift) -> ReLU;
 *            dropout = identity; last layer Linear only)
 * n_layers == 0 stops after the fuse Linear.  fused_out_dev may be NULL when n_layers > 0; logits_out_dev is
 * required when n_layers > 0 and unused when n_layers == 0 (then fused_out_dev is the output and required).
 * Any dim and proj_dim >= 1 are accepted. Limits, each one RADAD_EINVAL: 0 <= n_layers <= RADAD_HEAD_MAX_LAYERS
 * (5 hidden layers + the output layer); no width (proj_dim or any dims[i]) above 8192; batch < 2^31 - 128.
 * ---------------------------------------------------------------------------------------------- */
#define RADAD_HEAD_MAX_LAYERS 6
typedef struct radad_head_weights {
    const float *wf, *bf;                           /* fuse [P, D+P], [P]                                  */
    int32_t n_layers;                               /* Linear layers of the detection MLP                  */
    int32_t dims[RADAD_HEAD_MAX_LAYERS + 1];        /* dims[0] = P, dims[i+1] = out width of layer i       */
    const float* lw[RADAD_HEAD_MAX_LAYERS];         /* [dims[i+1], dims[i]]                                */
    const float* lb[RADAD_HEAD_MAX_LAYERS];         /* [dims[i+1]]                                         */
    const float* bn_scale[RADAD_HEAD_MAX_LAYERS];   /* gamma / sqrt(running_var + eps), or NULL            */
    const float* bn_shift[RADAD_HEAD_MAX_LAYERS];   /* beta - running_mean * scale, or NULL                */
} radad_head_weights;
int radad_fuse_head_forward(const radad_head_weights* w, const float* tpp_dev /*[B,D]*/, const float* proj_dev /*[B,P]*/,
                            int64_t batch, int dim, int proj_dim, float* fused_out_dev /*[B,P] or NULL*/,
                            float* logits_out_dev /*[B, dims[n_layers]]*/, float* workspace_dev,
                            int64_t workspace_bytes, int device, void* stream);
int64_t radad_fuse_head_workspace_bytes(int64_t batch, int dim, int proj_dim);

/* ------------------------------------------------------------------------------------------------
 * RADADModel after the projection in training mode, forward and backward (radad_model.py:38-41,
 * detection_model.py:41-72,123-126 under autograd; csrc/head_train.inc).  a_0 = fused; hidden layer i:
 *   fused = Wf[:, :D] tpp + Wf[:, D:] proj + bf                              (the concatenation is never built)
 *   z = W_i a_{i-1} + b_i;  per column over the batch: mean, var = mean_b (z - mean)^2 (biased), rstd = 1 / sqrt(var + eps)
 *   xh = (z - mean) rstd;  y = xh gamma + beta;  a_i = max(y, 0) * mask_i * inv_keep
 *   running_mean <- (1 - f) running_mean + f mean;  running_var <- (1 - f) running_var + f var B / (B - 1)    (in place)
 *   logits = W_L a + b_L                                                      (the last layer: Linear only)
 *   backward, G = d logits:  dW_L = G^T a, db_L = sum_b G, da = G W_L;  per hidden layer from last to first
 *     dy = da * mask * inv_keep [a_i > 0], dgamma = sum_b dy xh, dbeta = sum_b dy, dxh = dy gamma,
 *     dz = rstd (dxh - mean_b dxh - xh mean_b(dxh xh)), dW_i = dz^T a_{i-1}, db_i = sum_b dz, da_{i-1} = dz W_i;
 *     df = da_0, dWf = df^T [tpp | proj], dbf = sum_b df, dproj = df Wf[:, D:], dtpp = df Wf[:, :D].
 * A hidden layer whose bn_gamma / bn_beta are both NULL has no BatchNorm (xh is then z itself, dz = dy, rstd unused); NULL
 * bn_running_mean / bn_running_var leave the running statistics alone.  masks_dev is a host array of n_layers - 1 device
 * pointers, masks_dev[i] a [B, dims[i+1]] array of 0 / 1 floats drawn by the caller (NULL entry, or masks_dev NULL: no dropout
 * there; inv_keep = 1 / (1 - p)).  The forward fills the saved buffers, the backward reads them (same weights, inputs, masks).
 * A NULL member of radad_head_grads skips that gradient; dtpp_dev / dproj_dev NULL skip those products.  No float atomics:
 * every sum has a fixed order, two runs give the same bits.  fp32 throughout.
 * Limits, each one RADAD_EINVAL before any HIP call: 1 <= n_layers <= RADAD_HEAD_MAX_LAYERS; no width (proj_dim, dims[i])
 * above 8192; dims[0] == proj_dim; dim <= 2^22 - 64; batch < 2^31 - 128; batch == 1 with a BatchNorm layer; a NULL required
 * buffer, weight or saved array; a half-NULL gamma / beta or running mean / var pair; a short workspace.  batch == 0 is RADAD_OK
 * without a launch.  One workspace size serves both calls; -1 for a bad shape.
 * ---------------------------------------------------------------------------------------------- */
typedef struct radad_head_train_weights {
    const float *wf, *bf;                                /* fuse [P, D+P], [P]                                  */
    int32_t n_layers;                                    /* Linear layers of the detection MLP                  */
    int32_t dims[RADAD_HEAD_MAX_LAYERS + 1];             /* dims[0] = P, dims[i+1] = out width of layer i       */
    const float* lw[RADAD_HEAD_MAX_LAYERS];              /* [dims[i+1], dims[i]]                                */
    const float* lb[RADAD_HEAD_MAX_LAYERS];              /* [dims[i+1]]                                         */
    const float* bn_gamma[RADAD_HEAD_MAX_LAYERS];        /* hidden layers: [dims[i+1]], or NULL with bn_beta    */
    const float* bn_beta[RADAD_HEAD_MAX_LAYERS];
    float* bn_running_mean[RADAD_HEAD_MAX_LAYERS];       /* updated in place by the forward, or NULL pair       */
    float* bn_running_var[RADAD_HEAD_MAX_LAYERS];
    float bn_eps[RADAD_HEAD_MAX_LAYERS];
    float bn_factor[RADAD_HEAD_MAX_LAYERS];              /* f: momentum, or 1 / num_batches_tracked             */
} radad_head_train_weights;
typedef struct radad_head_saved {
    float* fused;                                        /* [B, P]                                              */
    float* xh[RADAD_HEAD_MAX_LAYERS];                    /* hidden layers: normalised pre-activation [B, d]     */
    float* rstd[RADAD_HEAD_MAX_LAYERS];                  /* [d] (BatchNorm layers only)                         */
    float* act[RADAD_HEAD_MAX_LAYERS];                   /* what the next layer reads [B, d]                    */
} radad_head_saved;
typedef struct radad_head_grads {   /* shapes of the matching radad_head_train_weights members */
    float *dwf, *dbf;
    float* dlw[RADAD_HEAD_MAX_LAYERS];
    float* dlb[RADAD_HEAD_MAX_LAYERS];
    float* dgamma[RADAD_HEAD_MAX_LAYERS];
    float* dbeta[RADAD_HEAD_MAX_LAYERS];
} radad_head_grads;
int64_t radad_fuse_head_train_workspace_bytes(int64_t batch, int dim, int proj_dim, int n_layers, const int32_t* dims);
int radad_fuse_head_train_forward(const radad_head_train_weights* w, const float* tpp_dev /*[B,D]*/, const float* proj_dev /*[B,P]*/,
                                  const float* const* masks_dev, float inv_keep, int64_t batch, int dim, int proj_dim,
                                  const radad_head_saved* saved, float* logits_out_dev /*[B, dims[n_layers]]*/,
                                  float* workspace_dev, int64_t workspace_bytes, int device, void* stream);
int radad_fuse_head_backward(const radad_head_train_weights* w, const float* tpp_dev, const float* proj_dev,
                             const float* const* masks_dev, float inv_keep, const radad_head_saved* saved,
                             const float* grad_logits_dev /*[B, dims[n_layers]] contiguous*/, int64_t batch, int dim, int proj_dim,
                             const radad_head_grads* grads, float* dtpp_dev /*[B,D] or NULL*/, float* dproj_dev /*[B,P] or NULL*/,
                             float* workspace_dev, int64_t workspace_bytes, int device, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The training step behind the backward (pipeline.py:815-836; csrc/optim_step.inc): loss, gradient norms, clipping, Adam and
 * the loss-scale bookkeeping in four launches, without a host round trip.  Everything the loop logs stays on the device.
 * fp32 data; every sum in fp64 in a fixed order, no float atomics: two runs give the same bits.
 *
 * radad_bce_logits -- BCEWithLogitsLoss(pos_weight) (pipeline.py:768-770,815), scaler.scale(loss).backward()'s gradient for
 * the logits (:820) and the accuracy count (:835-836) in one launch.  With w_i = 1 + (pos_weight - 1) y_i:
 *   loss = mean_i (1 - y_i) x_i + w_i (log1p(exp(-|x_i|)) + max(-x_i, 0))           (unscaled, finite at x = +-100)
 *   dlogits_i = (s / n) ((1 - y_i) - w_i sigmoid(-x_i))     s = *scale_dev, or 1 when scale_dev is NULL
 *   correct = #{i : (x_i > 0) == (y_i == 1)}
 * labels are 0 / 1 as float32.  RADAD_EINVAL before any HIP call: n <= 0, pos_weight <= 0 (or NaN), a NULL buffer.
 *
 * radad_optim_step -- scaler.unscale_ x3 (:822-824), clip_grad_norm_ x3 (:825-827), scaler.step x3 over torch.optim.Adam
 * (:829-831, pipeline.py:96-107) and scaler.update (:832), for up to RADAD_OPTIM_MAX_GROUPS optimizers ("groups") at once.
 * Per group g over its tensors that have a gradient, inv = 1 / scale as it stands when the call begins:
 *   grad_norm[g] = sqrt(sum (grad inv)^2)      found_inf[g] = some grad element is inf or NaN
 *   coef = min(1, max_norm / (grad_norm[g] + 1e-6))      (max_norm <= 0: the norm is reported, coef = 1)
 * A group with found_inf set is skipped as a whole when a scale is in use: its param, exp_avg, exp_avg_sq and step count stay
 * as they are, and what its gradients hold afterwards is unspecified.  So is a group none of whose tensors has a gradient
 * (norm 0, step count unchanged).  Every other group steps: t = ++steps[g], and per element
 *   grad <- grad inv coef      (in place: what unscale_ and clip_grad_norm_ leave)
 *   g = grad + weight_decay param     exp_avg <- beta1 exp_avg + (1 - beta1) g     exp_avg_sq <- beta2 exp_avg_sq + (1 - beta2) g^2
 *   param <- param - lr / (1 - beta1^t) * exp_avg / (sqrt(exp_avg_sq) / sqrt(1 - beta2^t) + eps)
 * (torch.optim.Adam's defaults: weight decay added to the gradient, no amsgrad).  The hyperparameters are float32: beta2 =
 * 0.999 is the float nearest to it, and 1 - beta is formed from that float in double.
 * Then GradScaler.update: some group found a non-finite gradient -> scale *= backoff, growth_tracker = 0; else
 * ++growth_tracker, and at growth_interval scale *= growth (if that is finite), growth_tracker = 0.
 * state->scale and state->growth_tracker both NULL: no scaling and no skipping, plain clip + Adam; a non-finite gradient then
 * spreads as it does in torch (found_inf is still reported).
 * A tensor with grad == NULL (a parameter whose .grad is None) or numel == 0 takes no part.  Tensors may be views: an array
 * that does not start on a 16-byte boundary is read and written element by element.  tensors_host and groups_host are host
 * arrays, read during the call; pointers inside them and in state are device pointers.  Stream-ordered, no synchronisation,
 * no allocation, no copy: the tables travel as kernel arguments.
 * RADAD_EINVAL before any HIP call: n_tensors outside 0..RADAD_OPTIM_MAX_TENSORS, n_groups outside 1..RADAD_OPTIM_MAX_GROUPS,
 * a NULL struct, state pointer, workspace or (beside a gradient) param / exp_avg / exp_avg_sq, scale / growth_tracker half
 * NULL, a group index out of range, numel < 0, a beta outside [0, 1), eps <= 0, lr < 0, weight_decay < 0, with a scale growth
 * < 1, backoff outside (0, 1] or growth_interval < 1, a workspace below radad_optim_workspace_bytes (which covers every
 * listed tensor, with or without a gradient; -1 for n_tensors out of range, a NULL list or a negative numel).
 * ---------------------------------------------------------------------------------------------- */
#define RADAD_OPTIM_MAX_TENSORS 64
#define RADAD_OPTIM_MAX_GROUPS 8
typedef struct radad_optim_tensor {
    float* param;
    float* grad;                                         /* NULL: the tensor takes no part in this step         */
    float* exp_avg;
    float* exp_avg_sq;
    int64_t numel;
    int32_t group;
} radad_optim_tensor;
typedef struct radad_optim_group {
    float lr, beta1, beta2, eps, weight_decay, max_norm;
} radad_optim_group;
typedef struct radad_optim_state {   /* device pointers */
    float* scale;                                        /* [1], or NULL with growth_tracker: no loss scale     */
    int32_t* growth_tracker;                             /* [1]                                                 */
    int32_t* steps;                                      /* [n_groups] Adam's t per group                       */
    float* grad_norm;                                    /* [n_groups] out: norm of the unscaled gradients      */
    int32_t* found_inf;                                  /* [n_groups] out: 0 / 1                               */
} radad_optim_state;
int64_t radad_optim_workspace_bytes(const int64_t* numels, int n_tensors);
int radad_optim_step(const radad_optim_tensor* tensors_host, int n_tensors, const radad_optim_group* groups_host, int n_groups,
                     const radad_optim_state* state, float growth, float backoff, int growth_interval, void* ws_dev,
                     int64_t ws_bytes, int device, void* stream);
int radad_bce_logits(const float* logits_dev /*[n]*/, const float* labels_dev /*[n]*/, int64_t n, float pos_weight,
                     const float* scale_dev /*[1] or NULL*/, float* loss_out_dev /*[1]*/, float* dlogits_out_dev /*[n]*/,
                     int32_t* correct_out_dev /*[1]*/, int device, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The validation pass (pipeline.py:691-756, 862-872, 964-987; csrc/eval_metrics.inc, planned by csrc/eval_plan.h): what
 * evaluate_with_scores reads back per batch and what train() / evaluate() then compute in numpy, on the device.
 *
 * radad_eval_append -- per validation batch, replaces loss.item(), (preds == labels).sum().item(), logits.cpu().tolist() and
 * lbls.cpu().tolist() (pipeline.py:727-733).  One launch, stream-ordered, no synchronisation, no allocation.  Writes one
 * 64-bit sort key per sample at keys_dev[offset + i]:
 *   group id (0 .. 2^31 - 1; 0 where group_ids_dev is NULL) << 33 | image(score) << 1 | (label == 1)
 * image() is the order-preserving 32-bit image of the float32 score, with -0.0 mapped to +0.0 (numpy's unique / searchsorted
 * treat them as one threshold).  Adds into acc_dev (RADAD_EVAL_ACC_BYTES: double loss_sum, int64 correct, int64 count, int64
 * nonfinite) the batch's sum of BCEWithLogitsLoss(pos_weight) terms (radad_bce_logits' formula, unscaled, fp64 terms summed in
 * fp64 in one order), #{(x > 0) == (y == 1)}, n and #{x not finite}, by plain read-add-write of one thread: appends that share
 * acc_dev must be ordered on one stream.  val_loss is loss_sum / count (the reference weights batch means by batch size: the
 * same number up to rounding), val_acc is correct / count (:754-755).
 * RADAD_EINVAL before any HIP call: n <= 0, offset < 0, offset + n > RADAD_EVAL_MAX_N, pos_weight <= 0 (or NaN), a NULL
 * logits / labels / keys / acc.
 *
 * radad_eval_metrics -- _compute_eer (:152-175), _compute_macro_eer_by_group (:178-193), _compute_min_tDCF (:277-326),
 * _roc_curve / _auc (:196-234; _roc_curve's three outputs, :196-229, are the columns _plot_and_save_roc_det, :619, writes to
 * its CSV) over keys_dev[0 .. n).  Stream-ordered, no
 * host round trip, bitwise reproducible; keys_dev is not modified (more appends and another call are fine).  Hand-written
 * sort (LDS bitonic tiles + merge-path passes), counts by scan, then per distinct score t of a segment, in ascending order
 * behind -inf and in front of +inf:  fnr = #{positives < t} / P,  fpr = #{negatives >= t} / N  (fp64 divisions of integers).
 *   out[RADAD_EVAL_EER], [_EER_THRESHOLD]   (fnr + fpr) / 2 * 100 at the first candidate with the least |fnr - fpr|, and it
 *   out[RADAD_EVAL_MACRO_EER], [_GROUPS_SCORED]   the fp64 mean of the same EER per group id over the groups that hold both
 *                                classes, added one by one in ascending group id, and how many did; NaN and 0 if none.  has_groups == 0 (every id equal by the
 *                                caller's word) or all ids equal on the device: the pooled EER (1 group, or NaN and 0)
 *   out[RADAD_EVAL_MIN_TDCF], [_MIN_TDCF_THRESHOLD]   the first least ((c0 + (c1 (1 - fnr)) p_fa_spoof_asv) + c2 fnr) / c_def,
 *                                no FMA contraction; NaN, NaN with consts == NULL.  consts is a host struct read during the call:
 *                                c0 = C_miss_asv pi_tar P_miss_asv + C_fa_asv pi_non P_fa_asv, c1 = C_fa_cm pi_spoof,
 *                                c2 = C_miss_cm pi_tar, c_def = min(C_miss_asv pi_tar, C_fa_asv pi_non) (:303-323)
 *   out[RADAD_EVAL_AUC]          sum over distinct scores descending of (fp_i - fp_{i-1}) (tp_i + tp_{i-1}) in int64, exact,
 *                                divided once by 2 P N
 *   out[RADAD_EVAL_NONFINITE], [_POSITIVES], [_NEGATIVES], [_ROC_POINTS], [_DISTINCT]   counts, as doubles
 *   roc_dev (or NULL)            double[3 (n + 2)]: fpr at [0, n + 2), tpr at [n + 2, 2 (n + 2)), threshold behind; the first
 *                                out[RADAD_EVAL_ROC_POINTS] of each are written: (0, 0, max + 1e-6), one point per distinct
 *                                score descending, (1, 1, min - 1e-6)
 *   group_eer_dev (or NULL)      double[n]: the first out[RADAD_EVAL_GROUPS_SCORED] are written: the EER of every group that
 *                                holds both classes, in ascending group id (the terms of the macro-EER)
 * DEVIATION from the reference on tied scores: _roc_curve keeps the first element of each run of equal scores after an unstable
 * argsort, so its ROC points and AUC depend on an unspecified order inside the run.  Here a point carries the counts at the END
 * of its run, which gives the usual AUC = (#{pos > neg} + #{pos == neg} / 2) / (P N).  Without ties the two coincide.
 * P == 0 or N == 0: EER and t-DCF NaN, AUC 0.5, ROC (0, 0, inf), (1, 1, -inf), as the reference.  A non-finite score is outside
 * the contract: every metric is NaN, the count is reported, nothing faults.
 * RADAD_EINVAL before any HIP call: n outside 1..RADAD_EVAL_MAX_N, a NULL keys / out / workspace, a workspace that does not
 * start on a 16-byte boundary or is below radad_eval_metrics_workspace_bytes(n, has_groups) (-1 for n out of range).
 * ---------------------------------------------------------------------------------------------- */
#define RADAD_EVAL_MAX_N (1 << 24)
#define RADAD_EVAL_ACC_BYTES 32
#define RADAD_EVAL_OUT_DOUBLES 16
#define RADAD_EVAL_AUC 0
#define RADAD_EVAL_EER 1
#define RADAD_EVAL_EER_THRESHOLD 2
#define RADAD_EVAL_MACRO_EER 3
#define RADAD_EVAL_GROUPS_SCORED 4
#define RADAD_EVAL_MIN_TDCF 5
#define RADAD_EVAL_MIN_TDCF_THRESHOLD 6
#define RADAD_EVAL_NONFINITE 7
#define RADAD_EVAL_POSITIVES 8
#define RADAD_EVAL_NEGATIVES 9
#define RADAD_EVAL_ROC_POINTS 10
#define RADAD_EVAL_DISTINCT 11
typedef struct radad_tdcf_consts {
    double c0, c1, c2, p_fa_spoof_asv, c_def;
} radad_tdcf_consts;
int64_t radad_eval_metrics_workspace_bytes(int64_t n, int has_groups);
int radad_eval_append(const float* logits_dev /*[n]*/, const float* labels_dev /*[n]*/, const int32_t* group_ids_dev /*[n] or NULL*/,
                      int64_t n, float pos_weight, int64_t offset, uint64_t* keys_dev, void* acc_dev, int device, void* stream);
int radad_eval_metrics(const uint64_t* keys_dev, int64_t n, int has_groups, const radad_tdcf_consts* consts /*host, or NULL*/,
                       double* out_dev /*[RADAD_EVAL_OUT_DOUBLES]*/, double* roc_dev /*[3 (n + 2)] or NULL*/,
                       double* group_eer_dev /*[n] or NULL*/, void* ws_dev,
                       int64_t ws_bytes, int device, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Synthetic inputs (bench / tests only): a stateless integer hash so host and device produce the
 * SAME bits for element (seed, row, col).  See oracle/synth.py for the host twin.
 * ---------------------------------------------------------------------------------------------- */
int radad_synth_rows(float* out_dev, int64_t row0, int64_t n_rows, int dim, uint64_t seed, int device, void* stream);
int radad_synth_audio(float* out_dev, int64_t clip0, int64_t n_clips, int64_t samples_per_clip, uint64_t seed,
                      int device, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RADAD_HIP_H */
