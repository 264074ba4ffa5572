/*
 * p2s_hip.h -- C ABI of the MI355X-native Points2Surf SDF-inference engine (libp2s_hip.so).
 *
 * The reference (ErlerPhilipp/points2surf) is pure Python and has no FFI; its boundary for
 * this path is the Python API
 *     source/points_to_surf_eval.py:297-404   points_to_surf_eval(eval_opt)
 *     source/points_to_surf_model.py:237-352  PointsToSurfModel(**kw).forward(dict) -> [B,2]
 * Each entry point below names the reference call it replaces underneath that API.  The
 * host-side mirror of the Python API (points2surf_amd/dropin/source/...) binds these symbols
 * with ctypes; INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions: plain C types only; every function returns 0 on success or a negative
 * P2S_E* code (message via p2s_last_error(), thread-local).  All "dev" pointers are device
 * (HBM) pointers owned by the caller (e.g. PyTorch-ROCm tensor storage).  `stream` is a
 * hipStream_t passed as void* (NULL = default stream).  Calls are asynchronous on `stream`
 * unless documented otherwise; handles are owned by the library until *_destroy.
 */
#ifndef P2S_HIP_H
#define P2S_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define P2S_ABI_VERSION 5

#define P2S_OK            0
#define P2S_EINVAL       -1   /* bad argument / unsupported configuration */
#define P2S_EHIP         -2   /* HIP runtime error (see p2s_last_error) */
#define P2S_ENOMEM       -3
#define P2S_ECAPACITY    -4   /* caller-provided output buffer too small, or an input beyond a documented size limit */
#define P2S_ENODEVICE    -5   /* no gfx950 device visible */
#define P2S_EIO          -6   /* host file could not be opened / written / closed (the p2s_write_* functions) */

typedef struct p2s_model_s *p2s_model_t;
typedef struct p2s_cloud_s *p2s_cloud_t;
typedef struct p2s_rng_s   *p2s_rng_t;
typedef struct p2s_trimesh_s *p2s_trimesh_t;

int         p2s_abi_version(void);
const char *p2s_last_error(void);
/* number of visible HIP devices (0 if none); never fails */
int         p2s_device_count(void);
/* The library caches device memory per device: the blocks of destroyed cloud handles (so that a handle per shape costs
 * no hipMalloc / hipFree) and the scratch of the volume / iso-surface stages (~2 GB after a 512^3 call).  This gives
 * all of it back to HIP.  Waits for a running p2s_sdf_volume / p2s_marching_cubes on `device`. */
int         p2s_release_scratch(int device);

/* ------------------------------------------------------------------------------------------
 * Model  (replaces make_regressor: PointsToSurfModel(...).cuda(); load_state_dict(); eval(),
 *         reference source/points_to_surf_eval.py:150-171)
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t net_size;            /* 1024 (train --net_size)                                    */
    int32_t points_per_patch;    /* 300  (train --points_per_patch)                            */
    int32_t sub_sample_size;     /* 1000 (train --sub_sample_size)                             */
    int32_t output_dim;          /* 2: [|d| logit, sign logit] (outputs imp_surf_magnitude, imp_surf_sign);
                                    1: the signed-distance logit (output imp_surf, p2s_regression)  */
    int32_t use_point_stn;       /* QSTN present (p2s_vanilla and most ablation models)        */
    int32_t shared_transformer;  /* 1: one QSTN over cat(patch, sub-sample) (p2s_vanilla);
                                    0: the QSTN of feat_global, over the sub-sample only; its
                                       rotation also turns the patch (p2s_uniform, *_kNN ...)  */
    int32_t weighted_subsample;  /* 0: ids = randint (train --uniform_subsample 1, p2s_max);
                                    1: distance-weighted choice without replacement (p2s_vanilla) */
    int32_t encoder_bf16;        /* 0 (default): exact fp32.  1: per-point encoder layers on bf16 MFMA (fp32 accumulate; first
                                    layer, STN/QSTN heads, fold and decoder stay fp32) -- outside the 1e-4 contract.
                                    2 / 3: split precision, every operand as 2 / 3 bf16 pieces (3 / 6 bf16 MFMAs per
                                    product, 16 / 24 mantissa bits).  4: fp16 PAIR per operand, x = h0 + h1 * 2^-11 with
                                    the residual scaled into the normal range and a second accumulator (3 fp16 MFMAs per
                                    product, 22 mantissa bits): as exact as fp32 on the reference's goldens at 2.5x its
                                    throughput.  A query with an activation beyond the half range (6e4) is re-run through
                                    the fp32 kernels inside the same call (p2s_counters.fallback_queries counts them; more
                                    than 16384 per call: P2S_EINVAL) -- safe for an arbitrary checkpoint.  See DESIGN.md  */
    int32_t fixed_subsample;     /* train --fixed_subsample 1 (ablation): the generator is re-seeded with 42 before every
                                    query's draw (reference source/base/utils.py:210-211)                       */
    int32_t single_transformer;  /* train --single_transformer 1 (p2s_shared_encoder): ONE encoder over cat(patch,
                                    sub-sample); enc[0] = enc[1] = feat_local_global.*, the QSTN is its stn1 and sees
                                    all points, d1l / d1g = the two halves of fc1_local_global (1024 -> 1024)  */
    double  patch_radius;        /* train --patch_radius: 0 = the points_per_patch nearest neighbours, radius = their largest
                                    distance; > 0 (p2s_{small,medium,large}_radius: 0.05 / 0.1 / 0.2) = all points within
                                    this distance, a random points_per_patch of them if there are more, padded with the
                                    query point if fewer (reference source/base/point_cloud.py:177-191).  The float64
                                    value of the reference's Python float: the ball test is r * r in float64          */
    int32_t sym_sum;             /* train --sym_op sum (reference source/points_to_surf_model.py:170-175,211-214; set by no
                                    experiment script): the pool of PointNetfeat is a SUM over the points instead of the
                                    max.  The STN / QSTN trunks keep their max-pool in the reference too (:47, :106)  */
    /* stem reuse (fp32 models with a screened conv3 and a max pool): the main encoder pass starts at conv1
       from the conv0b output the STN pass saved in the workspace (16 KB per 64-point tile of a query).  Both took the place of
       reserved slots: the size and the earlier members are unchanged, and zeros are the defaults */
    int32_t stem_recompute;      /* 1: the main pass recomputes the stem, nothing is saved (the A/B switch) */
    int32_t stem_reuse_max_mb;   /* cap of the saved stem in the workspace; 0: 3072 MB, which holds the 2688 MB of an 8192-query
                                    chunk of 300 + 1000 points.  A chunk whose stem would be larger, or does not fit the
                                    device, is reserved without it and recomputes */
    int32_t reserved[1];
} p2s_model_cfg;

/* Offsets (in floats) into the weight blob.  The blob holds BatchNorm-folded fp32 weights,
 * GEMM operands pre-packed in MFMA B-fragment order ([N/32][K/8][64 lanes][4]); it is produced
 * by points2surf_amd/weights.py from a reference state_dict.  enc[0] = feat_local (kNN patch),
 * enc[1] = feat_global (sub-sample).  See DESIGN.md "weight blob". */
typedef struct {
    uint64_t w0a, b0a;           /* conv0a+bn0a: [3][64] plain, [64]                           */
    uint64_t w0b, b0b;           /* conv0b+bn0b: packed K=64 N=64                              */
    uint64_t s1, sb1;            /* stn2.conv1+bn1 packed 64x64                                */
    uint64_t s2, sb2;            /* stn2.conv2+bn2 packed 64x128                               */
    uint64_t s3, sb3;            /* stn2.conv3+bn3 packed 128x1024                             */
    uint64_t sf1, sfb1;          /* stn2.fc1+bn4 packed 1024x512                               */
    uint64_t sf2, sfb2;          /* stn2.fc2+bn5 packed 512x256                                */
    uint64_t sf3, sfb3;          /* stn2.fc3 (+identity in bias) packed 256x4096               */
    uint64_t m1t, mb1;           /* conv1+bn1, transposed & packed as B operand of the fold    */
    uint64_t m2, mb2;            /* conv2+bn2 packed 64x128                                    */
    uint64_t m3, mb3;            /* conv3+bn3 packed 128x1024                                  */
} p2s_encoder_offsets;

typedef struct {
    uint64_t c1, cb1;            /* conv1+bn1: [3][64] plain                                   */
    uint64_t c2, cb2;            /* conv2+bn2 packed 64x128                                    */
    uint64_t c3, cb3;            /* conv3+bn3 packed 128x1024                                  */
    uint64_t f1, fb1;            /* fc1+bn4 packed 1024x512                                    */
    uint64_t f2, fb2;            /* fc2+bn5 packed 512x256                                     */
    uint64_t f3, fb3;            /* fc3 (+[1,0,0,0] in bias): plain [256][4], [4]              */
} p2s_qstn_offsets;

typedef struct {
    p2s_encoder_offsets enc[2];
    p2s_qstn_offsets    qstn;    /* valid iff cfg.use_point_stn: point_stn.* (shared) or
                                    feat_global.stn1.* (not shared)                            */
    uint64_t d1l, db1l;          /* fc1_local+bn1_local   packed 1024x512                      */
    uint64_t d1g, db1g;          /* fc1_global+bn1_global packed 1024x512                      */
    uint64_t d2, db2;            /* fc2+bn2 packed 1024x256                                    */
    uint64_t d3, db3;            /* fc3+bn3 packed 256x128                                     */
    uint64_t d4, db4;            /* fc4: plain [128][2], [2]                                   */
} p2s_weight_offsets;

int p2s_model_create(const p2s_model_cfg *cfg, const float *blob_host, size_t n_floats,
                     const p2s_weight_offsets *offs, int device, p2s_model_t *out);
int p2s_model_destroy(p2s_model_t m);

/* a8 + a9: PointsToSurfModel.forward (reference source/points_to_surf_model.py:296-352) followed
 * by post_process (source/points_to_surf_eval.py:174-196, source/sdf_nn.py:11-21) and the
 * magnitude*sign / NaN->1 of save_evaluation (:263-273, :205-207).
 *   patch_ps_dev [B][points_per_patch][3]   kNN patch in patch space
 *   sub_ms_dev   [B][sub_sample_size][3]    global sub-sample in MODEL space (NOT translated; the
 *                                           kernel subtracts the query point; input is not modified)
 *   query_dev    [B][3], radius_dev [B] (may be NULL iff sdf_out_dev is NULL)
 *   logits_out_dev [B][output_dim] (may be NULL), sdf_out_dev [B] (may be NULL)
 * Work buffers are owned by the model and grown on demand (not thread-safe per model). */
int p2s_encode_decode(p2s_model_t m, const float *patch_ps_dev, const float *sub_ms_dev,
                      const float *query_dev, const float *radius_dev, int B,
                      float *logits_out_dev, float *sdf_out_dev, void *stream);

/* stage-wise access for parity tests: encoder features of both branches
 * (feat_local / feat_global outputs, reference points_to_surf_model.py:333,341), [B][net_size] each */
int p2s_encode_features(p2s_model_t m, const float *patch_ps_dev, const float *sub_ms_dev,
                        const float *query_dev, int B, float *feat_local_dev, float *feat_global_dev,
                        void *stream);

/* ------------------------------------------------------------------------------------------
 * Cloud  (replaces load_shape: cKDTree(pts, leaf_size=1000), reference source/data_loader.py:16-68)
 * ------------------------------------------------------------------------------------------ */
/* The neighbour index -- uniform cell grid G^3 over the bounding box, points counting-sorted by cell (stable: original
 * order inside a cell), 3-D summed-area table of the cell counts -- is built ON THE DEVICE, stream-ordered on `stream`:
 * bounding box + non-finite check, one 32-byte read-back (the call's only blocking operation; non-finite coordinates
 * are rejected with P2S_EINVAL like the reference's kd-tree build would fail), cell histogram, three scan passes,
 * scatter, in-cell ranking.  The handle owns a copy of the points; its memory comes from a per-device block cache
 * (see p2s_release_scratch), so creating a handle per shape allocates nothing once the cache is warm.
 * p2s_cloud_destroy drains the streams the handle was used on before its blocks are recycled. */
int p2s_cloud_create(const float *pts_dev, int n_points, int device, void *stream, p2s_cloud_t *out);
int p2s_cloud_destroy(p2s_cloud_t c);
int p2s_cloud_num_points(p2s_cloud_t c);
/* test / diagnostic read-back of the index (host buffers, any may be NULL): *G_host = cells per axis; geom_host[4] =
 * bounding-box minimum x, y, z and 1 / cell size; cell_start_host [G^3 + 1]; sat_host [(G + 1)^3] (inclusive prefix
 * sums, zero borders); sorted_host [n][4] = x, y, z, original index (int32 bit pattern).  Synchronises `stream`. */
int p2s_cloud_index_export(p2s_cloud_t c, int32_t *G_host, float *geom_host, int32_t *cell_start_host,
                           int32_t *sat_host, float *sorted_host, void *stream);

/* a1: get_voxel_centers_grid_smaller_pc (reference source/sdf.py:46-79).  Writes up to `capacity`
 * query points (C order of the voxel index) to q_out_dev [capacity][3]; *n_queries receives the
 * full count (synchronises `stream`).  Returns P2S_ECAPACITY if capacity is too small (count is
 * still reported) -- call once with capacity 0 to size the buffer. */
int p2s_query_grid(p2s_cloud_t c, int grid_resolution, int epsilon, float *q_out_dev,
                   int64_t capacity, int64_t *n_queries, void *stream);

/* a4 + a5: get_patch_kdtree (kdtree.query(k), fp64 ranking; reference source/base/point_cloud.py:170-175)
 * + get_patch_radii / model_space_to_patch_space (source/base/utils.py:62-69,80-88;
 * source/data_loader.py:341-350).  ids sorted by ascending distance.
 *   ids_out_dev [Q][k] int32 (may be NULL), patch_ps_out_dev [Q][k][3] (may be NULL),
 *   radius_out_dev [Q] (may be NULL) */
int p2s_knn_patch(p2s_cloud_t c, const float *query_dev, int64_t n_queries, int k,
                  int32_t *ids_out_dev, float *patch_ps_out_dev, float *radius_out_dev, void *stream);
/* the same k nearest points as a SET: patch rows in an arbitrary (deterministic) order, no ids -- what the per-shape
 * pipeline uses: the encoders max-pool over the patch, so the order of its points changes no bit of the result, and the
 * k smallest distances are selected by bisection on their bit patterns instead of a sort (~3x faster).  Ties at the
 * k-th distance are broken by id exactly like p2s_knn_patch.  radius_out_dev as above. */
int p2s_knn_patch_set(p2s_cloud_t c, const float *query_dev, int64_t n_queries, int k,
                      float *patch_ps_out_dev, float *radius_out_dev, void *stream);

/* ------------------------------------------------------------------------------------------
 * a6: global sub-sample (reference source/base/utils.py:196-227 with the dataset-wide
 *     np.random.RandomState of source/data_loader.py:274-277)
 * ------------------------------------------------------------------------------------------ */
int p2s_rng_create(uint32_t seed, int device, p2s_rng_t *out);   /* RandomState(seed) */
int p2s_rng_destroy(p2s_rng_t r);
/* copy the 624-word MT19937 state + position out / in (host memory); for sharding + tests */
int p2s_rng_get_state(p2s_rng_t r, uint32_t *mt624_host, int32_t *pos_host, void *stream);
int p2s_rng_set_state(p2s_rng_t r, const uint32_t *mt624_host, int32_t pos, void *stream);

/* Tables for parallel generation of the stream (GF(2) jump-ahead, tools/mt_jump.py ->
 * points2surf_amd/mt_jump_tables.npz): supports of t^(B*2^m*624) mod phi(t), m = 0..levels-1, concatenated
 * (uint16 exponents), counts_host[m] entries each.  Large requests are then served from a *session*: 2^levels
 * streams of B blocks generated at once (1.3 GB for 512 x 1024 blocks), from which consecutive calls take their
 * values; the 624-word state is advanced when the session ends (any call that needs the state, or a request with
 * another modulus).  Results are bit-identical to the serial generator.  Required by p2s_subsample_weighted. */
int p2s_rng_set_jump_tables(p2s_rng_t r, const uint16_t *supports_host, const int32_t *counts_host, int levels,
                            int blocks_per_stream);
/* sticky error of the parallel generator (0 = none); synchronises `stream` */
int p2s_rng_check(p2s_rng_t r, void *stream);

/* uniform mode (p2s_max, uniform_subsample=1): ids = rng.randint(0, N, n) per query, consumed in
 * query order from one continuous stream.  ids_out_dev [Q][n] int32; NULL = only advance the stream past
 * these queries (query-range sharding), pts_out_dev [Q][n][3] gathered points in model space (may be NULL). */
int p2s_subsample_uniform(p2s_rng_t r, p2s_cloud_t c, int64_t n_queries, int n,
                          int32_t *ids_out_dev, float *pts_out_dev, void *stream);
/* distance-weighted mode (p2s_vanilla, uniform_subsample=0; reference source/base/utils.py:200-219):
 * per query p = clip(1 - 1.5 d/max(d), 0.05, 1) / sum (float32, numpy's summation order) and
 * ids = rng.choice(N, n, replace=False, p=p), consumed in query order from the same continuous stream --
 * bit-identical to numpy's legacy RandomState.  Needs the jump tables (p2s_rng_set_jump_tables).
 * q_dev [Q][3] query points (model space), ids_out_dev [Q][n] int32 (NULL = advance only), pts_out_dev as above.
 * Errors found on the device (degenerate distances) are reported by p2s_rng_check.  n <= 1024; clouds of more than
 * 475,040 points are refused with P2S_ECAPACITY before the stream is touched (LDS bitmap of the in-place algorithm). */
int p2s_subsample_weighted(p2s_rng_t r, p2s_cloud_t c, const float *q_dev, int64_t n_queries, int n,
                           int32_t *ids_out_dev, float *pts_out_dev, void *stream);
/* fixed mode (train --fixed_subsample 1; reference source/base/utils.py:210-211): ``rng.seed(seed)`` before EVERY
 * query's draw, seed = 42 in the reference.  q_dev = NULL: uniform draw (every query gets the same ids);
 * q_dev [Q][3]: distance-weighted choice (same random words, per-query probabilities; needs the jump tables).
 * Afterwards the generator is where numpy's is: seeded + the last query's consumption. */
int p2s_subsample_fixed(p2s_rng_t r, p2s_cloud_t c, const float *q_dev, int64_t n_queries, int n, uint32_t seed,
                        int32_t *ids_out_dev, float *pts_out_dev, void *stream);
/* clouds with FEWER points than the sub-sample size (reference source/base/utils.py:221-226): rng.shuffle of the
 * point array (numpy legacy shuffle: rk_interval per row) + zero padding.  The reference shuffles shape.pts IN PLACE
 * under the kd-tree, so every query permutes the array later patches are gathered from; the cloud handle keeps that
 * permutation.  perm_before_dev [Q][N] (may be NULL): row -> original point id BEFORE query i's shuffle (what the
 * patch gather of query i sees); ids_out_dev [Q][n] (may be NULL): the shuffled ids, -1 = zero padding.
 * p2s_subsample_uniform / _weighted / _fixed route here automatically for such clouds. */
int p2s_subsample_shuffle_pad(p2s_rng_t r, p2s_cloud_t c, int64_t n_queries, int n, int32_t *perm_before_dev,
                              int32_t *ids_out_dev, void *stream);
/* a5 from explicit kNN ids (rows looked up through perm_before_dev, NULL = identity): radius + patch space */
int p2s_patch_from_ids(p2s_cloud_t c, const int32_t *ids_dev, const int32_t *perm_before_dev, const float *query_dev,
                       int64_t n_queries, int k, float *patch_ps_out_dev, float *radius_out_dev, void *stream);
/* a4, fixed-radius branch: get_patch_kdtree with patch_radius > 0 (reference source/base/point_cloud.py:177-191,
 * source/data_loader.py:335-350) -- see points2surf_amd/csrc/p2s_ball.hip.
 * p2s_kd_order_host: HOST function (no device needed): the index array of scipy.spatial.cKDTree(pts, leafsize) --
 * query_ball_point returns its hits in this order.  order_out [n]; leaf_start_out [n_leaves + 1] (may be NULL).
 * p2s_ball_count: number of points within `radius` of every query (= len(query_ball_point)).
 * p2s_ball_patch: for queries in order, the patch ids (ids_out_dev [Q][k], may be NULL; padding = 0), the patch in patch
 * space (patch_out_dev [Q][k][3]; NULL = only advance the generator) and radius_out_dev [Q] (may be NULL) = 1: the scale
 * of the distance output, which fixed-radius models do not rescale (source/points_to_surf_eval.py:180,188).  r = the
 * data set's FIRST RandomState (self.rng): a query with more than k points in its ball consumes the words of
 * permutation(count).  with_rotation: every query then also draws the rand(3) of the GT-query pass
 * (data_loader.py:384) and rot_out_dev [Q][9] receives its rotation matrix.  Synchronises `stream` once (hit counts). */
int p2s_kd_order_host(const float *pts_host, int64_t n, int leafsize, int32_t *order_out, int32_t *leaf_start_out,
                      int64_t leaf_cap, int32_t *n_leaves_out);
int p2s_ball_count(p2s_cloud_t c, const float *query_dev, int64_t n_queries, double radius, int32_t *count_out_dev,
                   void *stream);
int p2s_ball_patch(p2s_rng_t r, p2s_cloud_t c, const float *query_dev, int64_t n_queries, double radius,
                   int points_per_patch, int with_rotation, int32_t *ids_out_dev, float *patch_out_dev,
                   float *radius_out_dev, double *rot_out_dev, void *stream);
/* given-ids mode (ids produced elsewhere; id < 0 = zero point) */
int p2s_gather_points(p2s_cloud_t c, const int32_t *ids_dev, int64_t n_ids, float *pts_out_dev,
                      void *stream);

/* ------------------------------------------------------------------------------------------
 * Fused per-shape pipeline: what the batch loop of points_to_surf_eval does for one shape in
 * reconstruction mode (reference source/points_to_surf_eval.py:358-404), queries [q_begin, q_end)
 * of the shape's query list (pass 0, -1 for all).  The RNG stream is consumed for exactly the
 * processed queries.  sdf_out_dev [q_end-q_begin]; q_out_dev [q_end-q_begin][3] (may be NULL).
 * chunk = queries per internal batch (0 = default).
 * ------------------------------------------------------------------------------------------ */
int p2s_infer_shape(p2s_model_t m, p2s_cloud_t c, p2s_rng_t r, int grid_resolution, int epsilon,
                    int64_t q_begin, int64_t q_end, int chunk, float *sdf_out_dev, float *q_out_dev,
                    int64_t *n_done, void *stream);
/* the same for a fixed-radius model (cfg.patch_radius > 0): r_patch = the data set's FIRST RandomState (self.rng), which
 * the patch choice draws from (reference source/data_loader.py:335-338); p2s_infer_shape refuses such a model.  With
 * cfg.patch_radius == 0, r_patch is ignored (may be NULL). */
int p2s_infer_shape_ball(p2s_model_t m, p2s_cloud_t c, p2s_rng_t r, p2s_rng_t r_patch, int grid_resolution, int epsilon,
                         int64_t q_begin, int64_t q_end, int chunk, float *sdf_out_dev, float *q_out_dev,
                         int64_t *n_done, void *stream);

/* ------------------------------------------------------------------------------------------
 * GT-query evaluation pass: the batch loop of points_to_surf_eval with reconstruction=False, the pass
 * full_eval.py:31-33 runs first when <indir>/05_query_dist exists (reference source/data_loader.py:365-393).
 * Query points are given (05_query_pts/<shape>.ply.npy), and every query draws a random rotation
 *     rand_rot = trimesh.transformations.random_rotation_matrix(self.rng.rand(3))     (data_loader.py:384)
 * from the dataset's FIRST RandomState (self.rng, :272; the sub-sample uses the second one, :277), applied in
 * float64 to the sub-sample (model space), the patch (patch space) and the query point, each cast back to float32
 * (:385-393).  r_rot = NULL: no rotation (plain inference at given query points).  sdf_out_dev [n_queries].
 * Fixed-radius models (cfg.patch_radius > 0) need r_rot: the same generator makes every query's patch choice, right
 * before its rotation.  Synchronises `stream`.
 * ------------------------------------------------------------------------------------------ */
int p2s_infer_queries(p2s_model_t m, p2s_cloud_t c, p2s_rng_t r_sub, p2s_rng_t r_rot, const float *q_dev,
                      int64_t n_queries, int chunk, float *sdf_out_dev, void *stream);
/* the two building blocks, for stage-wise parity tests:
 *   n rotations from the stream of r (6 raw words each): rot_out_dev [n][9] float64 row-major upper-left 3x3 of
 *   random_rotation_matrix(r.rand(3)); needs the jump tables */
int p2s_random_rotations(p2s_rng_t r, int64_t n, double *rot_out_dev, void *stream);
/*   trimesh.transformations.transform_points(pts, M).astype(float32) per item: pts_in_dev / pts_out_dev
 *   [n_items][points_per_item][3] (may alias), rot_dev [n_items][9] float64 */
int p2s_rotate_points(const double *rot_dev, const float *pts_in_dev, int points_per_item, int64_t n_items,
                      float *pts_out_dev, void *stream);
/* ------------------------------------------------------------------------------------------
 * Workers mode: the reference's sub-sample streams under ``--workers W --batchSize B`` (W >= 1, B >= 1).
 * torch's DataLoader hands batch b (dataset positions [b B, (b+1) B), across shapes) to worker b mod W, and every
 * worker holds its own copies of both RandomState(seed) generators (reference source/data_loader.py:270-277): the query
 * at dataset position g draws from worker stream (g // B) mod W, and every stream consumes its queries in increasing g.
 *   sub[W]    the workers' twins of the sub-sample generator (rng_global_sample)
 *   first[W]  the workers' twins of the first generator (self.rng): the patch choice of fixed-radius models and the
 *             rotation of the GT-query pass; NULL when the call needs neither
 *   first_position  dataset position of the call's first query (the caller's cursor over the whole sequence)
 * All 2 W handles must be distinct.  A call neither moves nor keeps first_position: the caller advances it.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t n_streams;             /* W */
    int32_t batch;                 /* B */
    int64_t first_position;
    const p2s_rng_t *sub;
    const p2s_rng_t *first;
} p2s_worker_streams;
/* the stream-major permutation of the n queries at positions first_position .. + n - 1: stream 0's queries in increasing
 * position, then stream 1's, ...  q_in_dev / q_out_dev [n][3] (both NULL: no gather; must not alias); src_out_dev [n]
 * int64: the local index each slot came from (may be NULL); counts_host [n_streams] queries per stream (may be NULL). */
int p2s_stream_order(int64_t first_position, int64_t n, int n_streams, int batch, const float *q_in_dev, float *q_out_dev,
                     int64_t *src_out_dev, int64_t *counts_host, void *stream);
/* p2s_infer_shape_ball in workers mode: the whole query grid of the shape (q_begin = 0, q_end = -1 or the grid size; a
 * part of it is refused), positions ws->first_position onwards.  sdf_out_dev and q_out_dev in grid order; the logits
 * capture (p2s_model_capture_logits) applies.  Refused with P2S_EINVAL before any generator moves: W > 1 with a cloud of
 * fewer points than the sub-sample (every worker shuffles its own cached copy of shape.pts), a partial range, bad
 * handles.  Synchronises `stream`. */
int p2s_infer_shape_workers(p2s_model_t m, p2s_cloud_t c, const p2s_worker_streams *ws, int grid_resolution, int epsilon,
                            int64_t q_begin, int64_t q_end, int chunk, float *sdf_out_dev, float *q_out_dev, int64_t *n_done,
                            void *stream);
/* p2s_infer_queries in workers mode: rotate != 0 = the GT-query pass (rotations from ws->first).  sdf_out_dev in query
 * order.  Synchronises `stream`. */
int p2s_infer_queries_workers(p2s_model_t m, p2s_cloud_t c, const p2s_worker_streams *ws, int rotate, const float *q_dev,
                              int64_t n_queries, int chunk, float *sdf_out_dev, void *stream);
/* the global sub-sample of n_queries queries in workers mode, in query order: ids_out_dev [n_queries][n] (NULL: only
 * advance the streams), pts_out_dev [n_queries][n][3] (may be NULL).  weighted = 0: uniform (q_dev may be NULL);
 * 1: the distance-weighted choice at q_dev [n_queries][3].  A cloud with fewer points than n is refused (P2S_EINVAL, no
 * generator moved).  Synchronises `stream`. */
int p2s_subsample_workers(p2s_cloud_t c, const p2s_worker_streams *ws, const float *q_dev, int64_t n_queries, int n, int weighted,
                          int32_t *ids_out_dev, float *pts_out_dev, void *stream);
/* One-shot capture of the decoder's raw logits: the NEXT p2s_infer_shape / p2s_infer_shape_ball / p2s_infer_queries /
 * p2s_infer_shape_workers / p2s_infer_queries_workers call on this model (p2s_encode_* leave the capture in place) also
 * writes logits_out_dev [processed queries][output_dim] (column output_dim - 1 = the sign logit, or the one
 * signed-distance logit of the regression model) -- what post_process (reference source/points_to_surf_eval.py:174-196)
 * starts from.  The drop-in's tie report (P2S_TIE_REPORT) lists the queries whose sign logit lies within fp32 noise of the
 * reference's decision ``logit >= 0`` (source/sdf_nn.py:16-21).  capacity_queries < the queries of that call: the call
 * returns P2S_ECAPACITY.  capacity_queries = 0 cancels. */
int p2s_model_capture_logits(p2s_model_t m, float *logits_out_dev, int64_t capacity_queries);
/* test hook: the next pipeline call on this model fails with P2S_EHIP before chunk `chunk_index` (-1 = off) */
int p2s_debug_fault_chunk(p2s_model_t m, int chunk_index);
/* test hook: the pooled features of the STN pass, [2 encoders: local, global][n_queries][1024], as the last
 * p2s_encode_decode / p2s_encode_features call of n_queries <= 8192 queries (one internal batch) left them in the model's
 * workspace, copied to out_dev on `stream` (the stream of that call) */
int p2s_debug_stn_pool(p2s_model_t m, int n_queries, float *out_dev, void *stream);

/* ------------------------------------------------------------------------------------------
 * "next" row: the consumer of the SDF samples.  add_samples_to_volume + propagate_sign
 * (+ the clamp that follows) of reference source/sdf.py:82-178,199-201: scatter the samples into a dense
 * grid_res^3 volume, set the border faces to -1 (outside), propagate signs into the unknown voxels with a
 * sigma^3 box filter (edge replication) thresholded at certainty_threshold until the number of unknown
 * voxels stops falling.  vol_out_dev: [grid_res]^3 float32 in C order -- every value of the reference's
 * float64 volume (float32 SDF samples, -1, 0, +1) is exactly representable.  One sample per voxel is
 * expected (what the query grid produces).  *iterations (host, may be NULL) = number of sweeps.
 * Synchronises `stream`.
 * ------------------------------------------------------------------------------------------ */
int p2s_sdf_volume(const float *query_dev, const float *sdf_dev, int64_t n, int grid_res, int sigma,
                   float certainty_threshold, int clamp, int device, float *vol_out_dev, int32_t *iterations,
                   void *stream);

/* ------------------------------------------------------------------------------------------
 * "next" row: iso-surface of the clamped volume at level 0 -- the step the reference hands to
 * scikit-image, `measure.marching_cubes_lewiner(volume, 0)` (reference source/sdf.py:211-215) -- followed by the
 * vertex transform ((v + 0.5) / res - 0.5) * 2 (:223, float32 arithmetic like numpy; model_space != 0) and
 * trimesh.repair.fix_inversion (:224-225, fix_inversion != 0: faces are flipped when the signed volume is negative;
 * *inverted reports it).
 * The algorithm is the one scikit-image 0.18.3 runs: Lewiner et al. 2003 -- case / face-test / interior-test look-up
 * tables, tunnel tilings, centre vertex --, "inside" = value > 0, vertices interpolated with the weights
 * 1 / (eps + |value|), every face reversed (gradient_direction='descent').  The mesh equals scikit-image's vertex
 * position for vertex position and triangle for triangle (pinned on the reference's volumes); only the
 * ORDER of vertices and faces is this library's (grid points / cells in C order).
 * vol_dev [res]^3 float32, C order; verts_out_dev [cap_verts][3] float32 (array-index coordinates, or model space),
 * faces_out_dev [cap_faces][3] int32.  *n_verts / *n_faces always receive the full counts; P2S_ECAPACITY if a capacity
 * is too small (call with capacities 0 to size the buffers).  Synchronises `stream`.
 * ------------------------------------------------------------------------------------------ */
int p2s_marching_cubes(const float *vol_dev, int grid_res, float *verts_out_dev, int64_t cap_verts,
                       int32_t *faces_out_dev, int64_t cap_faces, int64_t *n_verts, int64_t *n_faces,
                       int model_space, int fix_inversion, int *inverted, int device, void *stream);
/* single-cube diagnostic, host arithmetic (the decision code the kernels run): values8 = the cube's values minus the
 * level in Lewiner's corner order (0 (0,0,0) 1 (1,0,0) 2 (1,1,0) 3 (0,1,0) 4 (0,0,1) 5 (1,0,1) 6 (1,1,1) 7 (0,1,1) as
 * x, y, z).  *row = the selected row of the tiling table (-1: none), edges36 = its cube edge ids, 3 per triangle,
 * 12 = the centre vertex, -1 padded */
int p2s_mc_cell(const float *values8, int32_t *row, int32_t *n_tri, int32_t *edges36);

/* ------------------------------------------------------------------------------------------
 * "next" row: mesh metrics (reference source/base/evaluation.py:222-305): even surface sampling
 * (trimesh.sample.sample_surface_even), directed Hausdorff and Chamfer distances between the sample sets.
 * ------------------------------------------------------------------------------------------ */
/* RandomState.random_sample(n): n float64 in [0, 1) from the stream of r (2 words each); needs the jump tables */
int p2s_rng_random_sample(p2s_rng_t r, int64_t n, double *out_dev, void *stream);
/* trimesh.sample.sample_surface: u_dev [3 n] float64 uniform deviates laid out as the reference draws them (n face
 * picks, then n x 2 lengths); pts_out_dev [n][3] float32, face_out_dev [n] (may be NULL); *area_host = mesh area */
int p2s_mesh_sample_surface(const float *verts_dev, const int32_t *faces_dev, int64_t n_faces, const double *u_dev,
                            int64_t n_samples, float *pts_out_dev, int32_t *face_out_dev, double *area_host,
                            int device, void *stream);
/* trimesh.points.remove_close + the [:count] cut of sample_surface_even: of every pair of points within `radius` the
 * one with more close neighbours is dropped (ties: the first); the survivors, in order, at most `limit`.  A pair is
 * close when its squared float64 distance is <= radius * radius.  P2S_EINVAL, with nothing written and *n_out left
 * alone: a NULL pointer, m > 2,000,000, limit < 0, or a radius that is negative, infinite or NaN */
int p2s_points_remove_close(const float *pts_dev, int64_t m, double radius, int64_t limit, float *pts_out_dev,
                            int64_t *n_out, int device, void *stream);
/* nearest-neighbour distance (float64, exact) of every query point to the cloud `target`; *max_host = directed
 * Hausdorff distance, *sum_host = the Chamfer term; dist_out_dev [n] float64 may be NULL.  Synchronises. */
int p2s_nn_distance_stats(p2s_cloud_t target, const float *query_dev, int64_t n, double *dist_out_dev, double *max_host,
                          double *sum_host, void *stream);

/* ------------------------------------------------------------------------------------------
 * "next" row: ground-truth signed distance to a triangle mesh -- what the reference obtains from
 * trimesh.proximity.signed_distance in batches of 1000 queries (source/sdf.py:318-348, get_signed_distance) for the
 * GT file 05_query_dist/<shape>.npy of make_dataset.py:447-474.  Exact: nearest triangle in float64 (ties: smallest
 * face id), sign from the pseudonormal of the closest feature (face / edge / vertex), queries whose sign is within
 * rounding of zero re-decided by the generalised winding number.  Positive inside (trimesh), negative outside, a query
 * with d <= 1e-8 (trimesh tol.merge) keeps its unsigned d; a non-finite query, or one so far away that d^2 overflows
 * float64 (coordinates beyond ~1e154), yields NaN and face -1.  A handle serves ONE p2s_mesh_distance call at a time
 * (info[5] is per handle); different handles are independent.
 * ------------------------------------------------------------------------------------------ */
/* replaces trimesh.load / trimesh.Trimesh(vertices, faces) (make_dataset.py:457) + the proximity structures
 * signed_distance builds per call: verts_dev [n_verts][3] float32, faces_dev [n_faces][3] int32 (both read during the
 * call only).  Indices out of range or a non-finite vertex: P2S_EINVAL, before anything dereferences them.  Holds the
 * float64 triangles, face / edge / angle-weighted vertex pseudonormals and the cell + octree index of the triangles' AABBs;
 * an inward-oriented closed mesh is stored flipped (trimesh.repair.fix_inversion).  Build scratch (the edge table, ~150
 * bytes per face) returns to the device's block cache before the call ends.  Synchronises `stream`. */
int p2s_trimesh_create(const float *verts_dev, int64_t n_verts, const int32_t *faces_dev, int64_t n_faces, int device,
                       void *stream, p2s_trimesh_t *out);
int p2s_trimesh_destroy(p2s_trimesh_t m);
/* trimesh's mesh.is_watertight / is_winding_consistent / the sign of mesh.volume.  info_host[8]: [0] n_faces,
 * [1] closed (every undirected edge traversed exactly once in each direction), [2] inverted (closed and signed volume
 * < 0: stored flipped), [3] number of open or non-manifold edges, [4] cells per axis of the index, [5] point-triangle
 * tests of the last indexed p2s_mesh_distance call on this handle, [6] connected components (closed meshes; 0
 * otherwise), [7] faces under the degenerate rule (|ab x ac|^2 <= 2^-90 |ab|^2 |ac|^2; they enter the rounding term of
 * p2s_mesh_winding).  The components of a closed mesh may overlap (a union of solids): with 2..16 components the sign is
 * the sum of the per-component pseudonormal signs (one nearest-triangle pass per component); with more, every signed
 * query is decided by the winding number (O(n_faces) per query). */
int p2s_trimesh_info(p2s_trimesh_t m, int64_t *info_host);
/* trimesh.proximity.signed_distance(mesh, query) (source/sdf.py:329; signed_ = 0: the unsigned closest-point distance of
 * trimesh.proximity.closest_point).  query_dev [n][3] float32 in any order; dist_out_dev [n] float64; face_out_dev [n]
 * (nearest face) and closest_out_dev [n][3] float64 may be NULL.  signed_ != 0 on a mesh that is not closed:
 * P2S_EINVAL, nothing written.  method 0 = index, 1 = exhaustive (every query against every triangle: the yardstick of
 * the index; identical results).  *n_winding_host (may be NULL) = queries decided by the winding number.
 * signed_ = 2: the same distance with EVERY sign from the generalised winding number (p2s_mesh_winding, method 0,
 * tau = 2^-10), inside iff |w| > 0.5: defined on any mesh, closed or not; a query with d <= 1e-8 keeps its unsigned d;
 * *n_winding_host = queries the tree left undecided and the exact sum decided.  Synchronises `stream`. */
int p2s_mesh_distance(p2s_trimesh_t m, const float *query_dev, int64_t n, int signed_, int method, double *dist_out_dev,
                      int32_t *face_out_dev, double *closest_out_dev, int64_t *n_winding_host, void *stream);

/* Generalised winding number (Jacobson et al. 2013) of every query, defined for open meshes too: w_out_dev [n] float64.
 * method 0 = a walk of the handle's octree: a node at distance d from its box centre beyond twice its half-diagonal r is
 * taken as one dipole of its area-weighted normal when its error bound A r / (2 pi (d - r)^3) is at most
 * tau * A / A_root (A the node's area), so the accepted bounds of a query sum to at most tau; other nodes are opened, leaf
 * cells add their triangles exactly.  err_out_dev [n] (may be NULL) = the sum of the accepted bounds plus the rounding term
 *     2^-53 F (K + F / 256 + 32) + D 2^-46 / pi,
 * F = faces, K = terms added for the query (at most F), D = info[7]: |w_out - w_exact| <= err.  A query with
 * | |w| - 0.5 | <= err is re-decided: it gets the exact sum and err 0.  method 1 = the exact sum for every query
 * (O(n_faces) each: the yardstick; err 0).  tau finite in [0, 0.25], else P2S_EINVAL and nothing written; tau = 0 opens
 * every node.  stats_host[4] (may be NULL): nodes accepted, triangles evaluated, queries re-decided exactly, 0.  A
 * non-finite query gives NaN (w and err).  Synchronises `stream`. */
int p2s_mesh_winding(p2s_trimesh_t m, const float *query_dev, int64_t n, int method, double tau, double *w_out_dev,
                     double *err_out_dev, int64_t *stats_host, void *stream);

/* ------------------------------------------------------------------------------------------
 * "next" row: scanning a mesh into a point cloud and drawing the GT query points -- what the reference's
 * make_dataset.py does by starting one BlenSor process per mesh (:242-380: 5..30 time-of-flight scans of 176 x 144 rays)
 * and with trimesh (source/sdf.py:288-315).  First-hit ray casting on the p2s_trimesh_t handle, float64.
 * Rules: the smallest t in (0, t_max] wins, ties go to the smallest face id; both sides of a face are hit; a ray in a
 * face's plane misses it; a degenerate face (|ab x ac|^2 <= 2^-90 |ab|^2 |ac|^2) is never hit; a hit whose computed
 * point lies more than 2^-24 max(|mesh|, |origin|) outside the face's bounding box is discarded (rounding at
 * conditioning beyond 2^-28 only); a direction component below 2^-1022 in magnitude is taken as 0; a ray with a non-finite component (|x| > 1e300) or a zero direction misses.  A miss
 * is face -1, t = +inf; no NaN is ever written.
 * ------------------------------------------------------------------------------------------ */
/* rays_dev [n][6] float64 (origin, direction; the direction need not be normalised: t is in units of it); t_out_dev [n]
 * float64, face_out_dev [n].  method 0 = index (octree descent), 1 = exhaustive (every ray against every triangle: the
 * yardstick; identical results).  *tests_host (may be NULL) = ray-triangle tests performed.  Synchronises `stream`. */
int p2s_mesh_raycast(p2s_trimesh_t m, const double *rays_dev, int64_t n, double t_max, int method, double *t_out_dev,
                     int32_t *face_out_dev, int64_t *tests_host, void *stream);
/* the time-of-flight sensor: width x height pixels, tan(angle / 2) of the horizontal and the vertical opening angle
 * (computed by the caller), the largest distance that returns a hit */
typedef struct {
    int32_t width, height;
    double  tan_half_w, tan_half_h, max_distance;
} p2s_tof_sensor;
/* n_scans scans of the mesh.  Sensor frame: camera at the origin looking along +y, x right, z up; the object is placed
 * at R(q) p + location.  poses_host [n_scans][7]: location[3], UNIT quaternion (w, x, y, z); ||q|^2 - 1| > 2^-49: P2S_EINVAL.  Pixel (i, j) looks along
 * normalise(((i + 1/2 - W/2) 2 tan_half_w / W, 1, (j + 1/2 - H/2) 2 tan_half_h / H)); the ray is cast in model space
 * (origin R^T (-location), direction R^T dir), so t is the sensor distance.  noise_dev [n_scans * H * W] float64
 * standard-normal deviates, one per ray in the order (scan, row j, column i).  The hits are written in that order
 * (stable): noisy_out_dev [hits][3] = o + (t + sigma g) d, clean_out_dev [hits][3] = o + t d, face_out_dev [hits],
 * normal_out_dev [hits][3] = the hit face's stored unit normal; every output holds n_scans * H * W entries.
 * hits_per_scan_host [n_scans], *n_hits_host = their sum, *tests_host (may be NULL) as above.  Synchronises `stream`. */
int p2s_mesh_tof_scan(p2s_trimesh_t m, const double *poses_host, int32_t n_scans, const p2s_tof_sensor *sensor, double sigma,
                      const double *noise_dev, int method, double *noisy_out_dev, double *clean_out_dev, int32_t *face_out_dev,
                      double *normal_out_dev, int32_t *hits_per_scan_host, int64_t *n_hits_host, int64_t *tests_host, void *stream);
/* get_query_pts_for_mesh (source/sdf.py:288-315): out_dev [n_far + n_close][3] float32 = n_far points u - 1/2
 * (u_far_dev [n_far][3] float64 in [0, 1)), then the surface samples samples_dev [n_close][3] float32 of the faces
 * face_dev [n_close] (p2s_mesh_sample_surface) moved along the face's stored unit normal by
 * (u_offset_dev[i] - 1/2) * 2 * patch_radius.  Stream-ordered. */
int p2s_mesh_query_points(p2s_trimesh_t m, const float *samples_dev, const int32_t *face_dev, const double *u_offset_dev,
                          const double *u_far_dev, int64_t n_close, int64_t n_far, double patch_radius, float *out_dev,
                          void *stream);

/* ------------------------------------------------------------------------------------------
 * "next" row: repair of a raw triangle mesh and its normalisation -- the stages 02_meshes_cleaned and
 * 03_meshes of the reference's make_dataset.py (_clean_mesh :383-413: trimesh.process, fill_holes, fix_winding,
 * fix_inversion, is_volume; _normalize_mesh :71-88).  The project's own definition of the stage (unpinned: trimesh
 * absent); every result is a function of the input alone, whatever the order in which threads run.
 * Steps, in this order:
 *  a. indices out of range or a non-finite vertex: P2S_EINVAL, before anything dereferences them;
 *  b. weld: vertices with equal float32 coordinates (-0.0 counts as +0.0; NO rounding to a tolerance) become the one of
 *     the smallest input index;
 *  c. faces with a repeated index after welding are dropped; of faces with the same vertex set (any rotation or winding)
 *     the smallest face id survives; faces under the degenerate rule (|ab x ac|^2 <= 2^-90 |ab|^2 |ac|^2) are counted
 *     and kept (removing them opens T-junctions);
 *  d. orient: faces are neighbours across an undirected edge that exactly two faces use; a component is a connected set
 *     under that relation (edges of more than two faces connect nothing).  Faces are flipped so that neighbours traverse
 *     their shared edge in opposite directions, the face of the smallest id keeping its winding; a component where that
 *     is impossible (a Moebius strip) is left exactly as it came and counted;
 *  e. holes: a boundary edge is used by exactly one face and directed as that face traverses it; a hole is a cycle of
 *     boundary edges whose vertices all have exactly one incoming and one outgoing boundary edge.  Holes of at most
 *     max_hole_edges edges (0..64; 4 = what trimesh.repair.fill_holes fills) get a fan from their smallest vertex index:
 *     with the loop in boundary direction v0, v1, ..., v(n-1), the faces (v0, v(k+1), v(k)), k = 1 .. n-2, appended after
 *     the surviving input faces, holes by ascending v0, k ascending.  Longer holes, holes through a vertex with several
 *     boundary edges and every boundary of an unorientable component are left;
 *  f. components are taken again with the new faces; one without a boundary edge whose six-fold signed volume (float64,
 *     fixed order) is negative is flipped whole; zero volume or an open component: not flipped;
 *  g. unreferenced vertices go, the others keep the order of their representatives; faces keep the order of their input
 *     ids, added faces behind them; a face flipped (in d or f, not both) is written (a, c, b).
 * report_host [16] int64:
 *   [0] n_verts | n_faces << 32 (the input)   [1] vertices out   [2] faces out   [3] vertices welded away
 *   [4] collapsed faces dropped   [5] duplicate faces dropped   [6] degenerate faces kept   [7] faces flipped in d
 *   [8] components (of f)   [9] unorientable components (of d)   [10] components inverted   [11] holes filled
 *   [12] faces added   [13] holes left: connected groups of the boundary edges that remain (two holes through one vertex
 *   are one group)   [14] boundary edges left | edges of more than two faces << 32
 *   [15] verdict bits: 1 watertight (no boundary edge, no edge of more than two faces), 2 winding_consistent (every edge
 *   of exactly two faces is traversed once in each direction), 4 is_volume (both, and the total signed volume > 0).
 * Capacity: every added face closes a hole of n >= 3 boundary edges with n - 2 faces, holes share no boundary edge and a
 * surviving face has 3 edges, so faces added <= 3 faces - 2 holes: cap_faces = 4 * n_faces and cap_verts = n_verts
 * always suffice (n_faces + 3 n_faces (K - 2) / K for max_hole_edges = K >= 3; n_faces below).  Smaller buffers:
 * P2S_EINVAL with the needed counts in report [1], [2], nothing written.  n_faces = 0 is legal (n_verts = 0 too) and so
 * is an empty result.  face_src_out_dev [cap_faces]: the input face id, -1 for an added face.  Build scratch comes from
 * the device's block cache and returns to it before the call ends.  Synchronises `stream`. */
int p2s_mesh_repair(const float *verts_dev, int64_t n_verts, const int32_t *faces_dev, int64_t n_faces, int max_hole_edges,
                    float *verts_out_dev, int64_t cap_verts, int32_t *faces_out_dev, int32_t *face_src_out_dev, int64_t cap_faces,
                    int64_t *report_host, int device, void *stream);
#define P2S_EFLAT        -7   /* p2s_mesh_normalize: the bounding box has a zero extent on an axis (the reference skips the mesh) */
/* _normalize_mesh: in float64 c = (lo + hi) / 2, s = 1 / max extent, v' = (double(v) - c) * s, rounded once to float32
 * (contraction off).  verts_out_dev may be verts_dev.  info_host [4] (may be NULL): c, s.  A non-finite vertex or
 * n_verts < 1: P2S_EINVAL; a zero extent on any axis: P2S_EFLAT; nothing written then.  Synchronises `stream`. */
int p2s_mesh_normalize(const float *verts_dev, int64_t n_verts, float *verts_out_dev, double *info_host, int device, void *stream);

/* ------------------------------------------------------------------------------------------
 * Simplification of a triangle mesh by quadric vertex clustering (Lindstrom 2000, "Out-of-core simplification of large
 * polygonal models"): one grid over the mesh, one vertex per occupied cell, placed by the accumulated plane quadrics of the
 * faces that touch the cell.  The project's own definition -- it does NOT reproduce MeshLab's "Quadric
 * Edge Collapse Decimation", which the reference's tooling uses; every result is a function of the input alone (integer
 * atomics only, float64 sums in a fixed order, contraction off): equal inputs give equal bytes.
 *  a. indices out of range or a non-finite vertex: P2S_EINVAL, before anything dereferences them.  n_faces = 0 (n_verts = 0
 *     too) is legal and gives the empty result: no vertex, no face, vert_map all -1.
 *  b. grid: exactly the grid of p2s_prepare_voxel_thin.  lo = the bounding box minimum of ALL input vertices, ext its largest
 *     extent, cell index per axis i = min(R - 1, floor((p - lo) * (R / ext))) (ext = 0: every vertex in cell 0), cell size
 *     h = ext / R, cell centre g = lo + (i + 1/2) h.  resolution 1..1024 = R.  resolution 0 (needs max_faces >= 0): with
 *     n_faces <= max_faces the input is copied bit for bit (unreferenced vertices too; vert_map and face_src the identity;
 *     report [3] = 0); otherwise lo = 1, hi = 1024; while lo < hi: mid = (lo + hi + 1) / 2; surviving(mid) <= max_faces ?
 *     lo = mid : hi = mid - 1; R = lo.  surviving is the count of c, BEFORE duplicate removal, so the result never has more
 *     than max_faces faces (R = 1 always qualifies).  The count is not monotone over grids that do not nest: the search
 *     is the definition.
 *  c. a face survives iff its three corners lie in three pairwise different cells.
 *  d. one output vertex per cell that holds a corner of at least one surviving face, ordered by the smallest input vertex
 *     id of the cell.  vert_map_out_dev [n_verts] (may be NULL): the output id of the vertex's cell, -1 where the cell has none.
 *  e. placement 0 (mean) or 1 (quadric), in coordinates relative to g.  m = (sum of (p - g) over the cell's input vertices in
 *     ascending vertex id) / count.  placement 0: x = m.  placement 1: every input face with at least one corner in the cell
 *     contributes once, in ASCENDING FACE ID, except faces under the degenerate rule (|ab x ac|^2 <= 2^-90 |ab|^2 |ac|^2 on
 *     the stored coordinates): with its corners a, b, c relative to g, n = (b - a) x (c - a), d = -(n . a), A += n n^T,
 *     r += d n (squared-area weighting).  tr(A) = 0: x = m.  Otherwise x = m - (A + epsilon tr(A) I)^-1 (A m + r) by a
 *     Cholesky factorisation (Tikhonov; no eigenvalue is truncated; condition number <= 1 + 1 / epsilon); epsilon finite in
 *     [1e-6, 1].  Fallback: max |x| > h gives x = m.  The vertex is g + x, rounded once to float32.
 *  f. the surviving faces in input order, mapped to the output ids, winding kept; of faces with the same vertex set (any
 *     rotation or winding) the smallest input face id survives (rule c of p2s_mesh_repair).  face_src_out_dev [cap_faces]
 *     (may be NULL): the input face id.
 *  g. cap_verts >= min(n_verts, occupied cells) and cap_faces >= surviving faces suffice, so do n_verts and n_faces.
 *     Smaller buffers: P2S_EINVAL with the report filled, nothing written.  n_verts, n_faces <= 2^27.  Arguments are checked
 *     before the device is touched; the message names the offending one.
 * report_host [16] int64:
 *   [0] n_verts | n_faces << 32 (the input)   [1] vertices out   [2] faces out   [3] R   [4] occupied cells
 *   [5] faces collapsed   [6] duplicate faces dropped   [7] degenerate input faces (no quadric)   [8] cells placed by the
 *   quadric   [9] cells with tr(A) = 0   [10] cells that fell back to the mean ([8]..[10] are 0 for placement 0)
 *   [11] probes of the search   [12] boundary edges | edges of more than two faces << 32 of the OUTPUT (clustering does not
 *   preserve topology)   [13] the same of the input   [14], [15] 0.
 * Scratch comes from the device's block cache and returns to it before the call ends.  Synchronises `stream`. */
int p2s_mesh_simplify(const float *verts_dev, int64_t n_verts, const int32_t *faces_dev, int64_t n_faces, int resolution,
                      int64_t max_faces, int placement, double epsilon, float *verts_out_dev, int64_t cap_verts,
                      int32_t *faces_out_dev, int32_t *face_src_out_dev, int64_t cap_faces, int32_t *vert_map_out_dev,
                      int64_t *report_host, int device, void *stream);

/* ------------------------------------------------------------------------------------------
 * Connected components of a triangle mesh with their measures, and the sub-mesh of a face mask: what sees
 * and removes the floating blobs and inner cavities of a reconstruction.  The project's own definition -- not trimesh's
 * `split`, not MeshLab's "remove isolated pieces"; every result is a function of the input alone (integer atomics only,
 * float64 sums in an order that the input fixes, contraction off): equal inputs give equal bytes.
 *
 * p2s_mesh_components
 *  a. arguments are checked before the device is touched; the message names the offending one.  An index out of range or a
 *     non-finite vertex: P2S_EINVAL, before anything dereferences it.  n_verts, n_faces <= 2^27.  n_faces = 0 is legal:
 *     0 components, nothing but the report written.
 *  b. two faces are connected iff they share a vertex INDEX; a component is a class of the transitive closure.  Equal
 *     coordinates under different indices do not connect: unwelded input is out of contract (weld with p2s_mesh_repair
 *     first).  Unreferenced vertices belong to no component.  A face with a repeated index is legal: it connects its distinct
 *     indices and has area 0.
 *  c. the components are ordered by their smallest face id; comp_out_dev [n_faces] is the rank 0 .. C - 1 of the face's component.
 *  d. counts_out_dev [cap][5] int64: [0] smallest face id  [1] faces  [2] referenced vertices  [3] boundary edges: undirected
 *     index pairs a != b used by exactly one face  [4] edges used by more than two faces.  (A face uses a pair once, however
 *     often its repeated index makes it traverse the pair.)
 *  e. measures_out_dev [cap][8] float64: [0] area  [1] signed volume  [2..4] minimum and [5..7] maximum of the bounding box of
 *     the referenced vertices (exact).  Per face, from the float64 of the stored corners a, b, c: u = b - a, v = c - a,
 *     n = (u.y v.z - u.z v.y, u.z v.x - u.x v.z, u.x v.y - u.y v.x), area term 0.5 sqrt((n.x n.x + n.y n.y) + n.z n.z),
 *     volume term ((a.x (b.y c.z - b.z c.y) + a.y (b.z c.x - b.x c.z)) + a.z (b.x c.y - b.y c.x)) / 6: a numpy float64
 *     evaluation gives the same bits.  The order of the additions: all faces sorted by (rank, face id) are cut into
 *     blocks of 256 positions; a component's terms are added in ascending face id within each block; of the blocks
 *     that the component touches, counted from its first, sum l of 64 adds the blocks l, l + 64, ... in ascending order; the
 *     64 sums are added in a binary tree (l with l + 32, then with l + 16, ..., l + 1).
 *  f. report_host [8] int64: [0] n_verts | n_faces << 32  [1] C  [2] faces of the largest component by face count  [3] rank of
 *     the component of largest area (of equal ones the smallest rank)  [4] unreferenced vertices  [5] hook rounds (a
 *     diagnostic, not contract)  [6], [7] 0.
 *  g. cap_components < C: P2S_EINVAL with the report filled and nothing else written.  cap_components = n_faces suffices.
 *
 * p2s_mesh_submesh: the faces with keep_dev[f] != 0 in input order, winding kept, and the vertices they reference in input
 * order, copied bit for bit.  vert_map_out_dev [n_verts] (may be NULL): the output id, or -1.  face_src_out_dev [cap_faces]
 * (may be NULL): the input face id.  report_host [3]: [0] n_verts | n_faces << 32  [1] vertices out  [2] faces out.  Smaller
 * buffers than that: P2S_EINVAL with the report filled, nothing written; n_verts and n_faces suffice.  An all-zero mask
 * gives the empty mesh.  The mask is int32 so that p2s_prepare_gather over a [C] keep table, indexed by comp_out_dev,
 * produces it on the device.  Validation and limits as in a.
 *
 * Both: scratch comes from the device's block cache and returns to it before the call ends.  Both synchronise `stream`. */
int p2s_mesh_components(const float *verts_dev, int64_t n_verts, const int32_t *faces_dev, int64_t n_faces, int32_t *comp_out_dev,
                        int64_t cap_components, int64_t *counts_out_dev, double *measures_out_dev, int64_t *report_host, int device,
                        void *stream);
int p2s_mesh_submesh(const float *verts_dev, int64_t n_verts, const int32_t *faces_dev, int64_t n_faces, const int32_t *keep_dev,
                     float *verts_out_dev, int64_t cap_verts, int32_t *faces_out_dev, int32_t *face_src_out_dev, int64_t cap_faces,
                     int32_t *vert_map_out_dev, int64_t *report_host, int device, void *stream);

/* ------------------------------------------------------------------------------------------
 * A triangle mesh made 2-manifold: faces removed at the edges of more than two faces, vertices split where
 * their faces do not form one fan -- the defects that p2s_mesh_repair, p2s_mesh_simplify and p2s_mesh_components count and
 * p2s_mesh_check flags.  The project's own definition -- NOT vcglib's / MeshLab's "Repair non Manifold Edges by removing
 * faces", "... by splitting vertices" or "Repair non Manifold Vertices by splitting", whose place in the reference's
 * hole_filling_mesh_simp.mlx it takes.  Every result is a function of the input alone (integer atomics only): equal inputs
 * give equal bytes.  Vertices are connected by INDEX; coordinates are never compared, and output coordinates are copied bit
 * for bit.
 *  a. arguments are checked before the device is touched; the message names the offending one.  An index out of range, a
 *     non-finite vertex or a face with a repeated index: P2S_EINVAL, before anything dereferences it.  n_verts, n_faces <=
 *     2^27.  mode is 1, 2 or 3.  n_faces = 0 is legal and gives the empty result.  Two faces with the same vertex set are
 *     legal; each counts as a face.
 *  b. mode & 1, remove.  Per face, from the float64 of the stored corners, with u, v, n as in rule e of p2s_mesh_components:
 *     q = (n.x n.x + n.y n.y) + n.z n.z (contraction off).  The faces are ordered by (q descending, face id ascending).  At
 *     every undirected edge used by more than two faces the first two of its faces in that order are the edge's keepers.  A
 *     face is removed iff at least one of its edges has more than two faces and it is not a keeper there.  This is ONE pass,
 *     not a greedy sequence: a face that one edge rejects may have taken a keeper's place at another edge, and that edge may
 *     then end with one face.  Afterwards no edge has more than two faces: every edge retains at most its two keepers.
 *  c. mode & 2, split, on the faces that b left.  The elements are the 3 F face corners (f, i).  For every undirected edge
 *     {a, b} used by exactly two faces f and g the corner of f at a is united with the corner of g at a, and likewise at b;
 *     edges of one face or of more than two faces unite nothing.  Every class of corners becomes one output vertex with the
 *     coordinates of its input vertex.  Without mode & 2 all corners at one input vertex form one class.
 *  d. output vertices are ordered by (input vertex id, smallest face id of the class); input vertices that no surviving face
 *     references are dropped.  vert_src_out_dev [cap_verts] (may be NULL): the input vertex id.  Surviving faces keep their
 *     input order and their winding; face_src_out_dev [cap_faces] (may be NULL): the input face id.  cap_verts = 3 n_faces
 *     and cap_faces = n_faces always suffice.  Smaller buffers than needed: P2S_EINVAL with the report filled and nothing
 *     else written.
 *  e. report_host [16] int64: [0] n_verts | n_faces << 32   [1] vertices out   [2] faces out   [3] edges of more than two
 *     faces in the input   [4] faces removed   [5] input vertices that got more than one class   [6] vertices added: [1]
 *     minus the input vertices that the surviving faces reference   [7] input vertices dropped: n_verts minus those, so
 *     [1] - [6] + [7] = n_verts   [8] boundary edges of the input   [9] boundary edges of the output   [10] output edges of
 *     exactly two faces that lie on an input edge of more than two faces ("rejoined")   [11] hook rounds (a diagnostic, not
 *     contract)   [12..15] 0.
 *  f. after mode & 2 every edge has at most two faces and every vertex's faces form one fan under p2s_mesh_check's definition
 *     (proof: csrc/p2s_meshmanifold.inl); after mode 1 every edge has at most two faces.  The call is idempotent: applied to
 *     its own output it returns the same vertex and face bytes.  Two tetrahedra that share an edge come out of mode 2 as two
 *     separate closed tetrahedra of 8 vertices.  The split leaves vertices of equal coordinates: a later weld
 *     (p2s_mesh_repair) merges them again.
 * Scratch comes from the device's block cache and returns to it before the call ends.  Synchronises `stream`. */
int p2s_mesh_manifold(const float *verts_dev, int64_t n_verts, const int32_t *faces_dev, int64_t n_faces, int mode,
                      float *verts_out_dev, int64_t cap_verts, int32_t *faces_out_dev, int64_t cap_faces,
                      int32_t *vert_src_out_dev, int32_t *face_src_out_dev, int64_t *report_host, int device, void *stream);

/* ------------------------------------------------------------------------------------------
 * The holes of a triangle mesh closed: every simple boundary loop of at most max_hole_edges edges gets the
 * MINIMUM-AREA TRIANGULATION of its vertices (Barequet & Sharir 1995; the first stage of Liepa 2003).  No vertex is added or
 * moved.  The project's own definition -- NOT vcglib's / MeshLab's "Close Holes" (ear cutting with its own weights), whose
 * place in the reference's hole_filling_mesh_simp.mlx it takes, and not the fan of p2s_mesh_repair (rule e there), which
 * stays as it is.  Every result is a function of the input alone (integer atomics only): equal inputs give equal bytes.
 * Vertices are connected by INDEX; the call neither welds nor orients: its contract is oriented, index-connected input
 * (p2s_mesh_repair first; p2s_mesh_manifold mode 2 where boundary vertices are not simple).
 *  a. arguments are checked before the device is touched; the message names the offending one.  An index out of range, a
 *     non-finite vertex or a face with a repeated index: P2S_EINVAL, before anything dereferences it.  n_verts, n_faces <=
 *     2^27.  max_hole_edges in 0 .. 128.  n_faces = 0 is legal: the report is filled and nothing else is written.
 *  b. loops, as in rule e of p2s_mesh_repair.  A boundary edge is an undirected edge of exactly one face, directed a -> b as
 *     that face traverses it.  A vertex is simple if it has exactly one outgoing and one incoming boundary edge.  A loop is
 *     a cycle v0 -> v1 -> ... -> v(n-1) -> v0 of simple vertices along these edges, written from its smallest vertex v0.
 *     Loops of 3 <= n <= max_hole_edges edges are candidates (a loop has at least 3).  Everything else is left and counted:
 *     longer loops, and boundaries through a vertex that is not simple -- two holes that touch, or a neighbour of the
 *     opposite orientation, whose boundary edge runs against the others.
 *  c. weight: float64 from the stored float32 corners p_0 .. p_(n-1) of the loop, contraction off, a correctly rounded square
 *     root.  For positions i < k < j: A(i, k, j) = 0.5 * sqrt((n.x n.x + n.y n.y) + n.z n.z) with n = (p_k - p_i) x (p_j -
 *     p_i), the cross product of the whole unit.  W(i, i + 1) = 0; W(i, j) = min over i < k < j of ((W(i, k) + W(k, j)) +
 *     A(i, k, j)), a tie to the smallest k.  A chord (i, j), j - i >= 2, other than (0, n - 1), whose {v_i, v_j} is ALREADY
 *     AN EDGE of the mesh (of any face count) is forbidden: W(i, j) = +inf -- which is what keeps the fill from making an
 *     edge of more than two faces.  If W(0, n - 1) is infinite the hole is left and counted as blocked.
 *  d. output: the input faces in their order, then the added faces hole by hole in ascending v0; within a hole the pre-order
 *     of the split tree: emit(i, j) writes the face of k = the split of (i, j), then emit(i, k), then emit(k, j).  An added
 *     face is (v_i, v_j, v_k): against the loop, so consistent with its neighbours; for n = 3 the face that the fan of
 *     p2s_mesh_repair writes.  face_src_out_dev [cap_faces] (may be NULL): the input face id, or -1 for an added face.
 *     Per loop in ascending v0, candidates and longer loops alike (both may be NULL): holes_out_dev [cap_holes][4] int32:
 *     v0, n, the id of its first added face or -1, the reason (0 filled, 1 too long, 2 blocked); hole_area_out_dev
 *     [cap_holes] float64: W(0, n - 1), or 0 where the loop is left.  Boundaries through vertices that are not simple are
 *     no loops: they appear in report [9] only.  cap_faces = n_faces + boundary edges - 2 loops always suffices; cap_holes
 *     counts only where one of the two per-loop outputs is given.  Smaller buffers than needed: P2S_EINVAL with the report
 *     filled ([1] faces and [2] loops needed) and nothing else written.
 *  e. report_host [16] int64: [0] n_verts | n_faces << 32   [1] faces out   [2] loops found   [3] holes filled   [4] faces
 *     added   [5] loops too long   [6] loops blocked   [7] boundary edges of the input   [8] boundary edges of the output
 *     [9] connected groups of the boundary edges of the output (edges that share a vertex are connected; "holes left" of
 *     p2s_mesh_repair)   [10] the longest filled loop   [11] edges of more than two faces in the output, which is the
 *     input's count   [12..15] 0.
 *  f. no call adds an edge of more than two faces; a vertex whose faces formed one fan still has one fan; the call is
 *     idempotent for a fixed max_hole_edges: applied to its own output it fills nothing and returns the same face bytes
 *     (proofs: csrc/p2s_meshholes.inl).  Not covered: no vertex is added and large fills are not refined (Liepa's stages 2
 *     and 3); no dihedral-angle weight; the fill is not tested for intersections with the rest of the mesh
 *     (p2s_mesh_check finds such pairs afterwards); the outer boundary of an open sheet is a hole like any other if it
 *     is short enough.
 * Scratch comes from the device's block cache and returns to it before the call ends.  Synchronises `stream`. */
int p2s_mesh_fill_holes(const float *verts_dev, int64_t n_verts, const int32_t *faces_dev, int64_t n_faces, int max_hole_edges,
                        int32_t *faces_out_dev, int64_t cap_faces, int32_t *face_src_out_dev, int32_t *holes_out_dev,
                        double *hole_area_out_dev, int64_t cap_holes, int64_t *report_host, int device, void *stream);

/* ------------------------------------------------------------------------------------------
 * The vertices of a triangle mesh smoothed: `iterations` rounds of the umbrella operator with uniform
 * weights, a half-step with lambda and, if mu != 0, a half-step with mu (Taubin 1995, "lambda | mu"; MeshLab's "Taubin
 * Smooth" has the same defaults 0.5 and -0.53).  mu = 0 is plain Laplacian smoothing.  Faces are not touched; no vertex is
 * added, removed or renumbered.  The project's own definition, not vcglib's.  Every result is a function of the input alone
 * (integer atomics only, float64 sums in one stated order): equal inputs give equal bytes.  Vertices are connected by INDEX:
 * nothing is welded (p2s_mesh_repair first).  Called by nothing else in the library: opt-in.
 *  a. arguments are checked before the device is touched; the message names the offending one.  An index out of range, a
 *     non-finite vertex or a face with a repeated index: P2S_EINVAL, before anything dereferences it, and nothing is written.
 *     n_verts, n_faces <= 2^27.  iterations in 0 .. 10000.  lambda finite, 0 < lambda <= 1.  mu finite, -2 <= mu <= 0.
 *     boundary_mode in 0 .. 2.  verts_out_dev [n_verts][3] is not NULL when n_verts > 0 and must not overlap verts_dev: the
 *     update is simultaneous and does not run in place.  fixed_dev [n_verts] uint8 and class_out_dev [n_verts] uint8 may be
 *     NULL.  n_faces = 0 or iterations = 0 is legal: the output is the input's bytes, the report and the classes are filled.
 *  b. neighbours: N(i) of a vertex i are the other ends of the undirected edges of the face list at i, each once however
 *     many faces have the edge, taken in ASCENDING vertex index.
 *  c. classes, one byte per vertex in class_out_dev; the first that applies:
 *       4 masked: fixed_dev[i] != 0
 *       5 unreferenced: no edge
 *       3 on an edge of more than two faces (modes 0 and 1): fixed
 *       2 boundary, fixed: on an edge of exactly one face, and either mode 0, or mode 1 with a number of such edges at i
 *         other than two
 *       1 boundary, on the curve: mode 1 and exactly two edges of exactly one face at i; its N(i) is the two other ends of
 *         those edges only (ascending), so a boundary curve is smoothed as a curve
 *       0 free: all of N(i)
 *     In mode 2 every referenced, unmasked vertex is class 0.  Classes 2 .. 5 are fixed: the vertex keeps its input bytes,
 *     the sign of a zero included; its neighbours still read it.
 *  d. one half-step with weight w: every vertex of class 0 or 1, with N(i) = j1 < j2 < .. < jd, reads the float32 positions
 *     of the previous half-step and writes, per coordinate, in float64 with contraction off:
 *         s = p_j1 (converted to float64);  s = s + p_jk for k = 2 .. d;  m = s / (double) d;
 *         p' = (float) (p_i + w * (m - p_i)),  the conversion rounded to nearest even, subnormal results kept.
 *     An iteration is a half-step with lambda, then, if mu != 0, one with mu.  Positions are float32 between half-steps.
 *     There is no limit on d.  If an output coordinate is not finite the call fails with P2S_EINVAL ("the result is not
 *     finite"): the report is filled, nothing else is written.
 *  e. report_host [16] int64: [0] n_verts | n_faces << 32   [1] .. [6] the vertices of the classes 0 .. 5   [7] undirected
 *     edges   [8] the largest |N(i)| used (over the classes 0 and 1; 0 if there is none)   [9] half-steps run: iterations,
 *     twice that if mu != 0, and 0 if no vertex is of class 0 or 1   [10] the bits of the float64 maximum over the vertices
 *     of (dx dx + dy dy) + dz dz between input and output, in float64 from the stored float32 values (where [11] > 0: over
 *     the vertices whose output is finite)   [11] non-finite output coordinates   [12..15] 0.
 *  f. the result is a function of the vertex array and of the SET of undirected edges with their face counts: reordering
 *     the faces, rotating or flipping their corners changes no output byte.  Renumbering the vertices may change the last
 *     bit, since the summation follows the index.  Not covered: cotangent or any other weight that depends on the geometry;
 *     a test of the smoothed mesh for self-intersections (p2s_mesh_check finds them afterwards).  This filter rounds every
 *     crease; the feature-preserving one is p2s_mesh_denoise below.
 *     With mu = 0 a closed mesh shrinks; lambda | mu shrinks far less and is no exact volume preservation.
 * Scratch comes from the device's block cache and returns to it before the call ends.  Synchronises `stream`. */
int p2s_mesh_smooth(const float *verts_dev, int64_t n_verts, const int32_t *faces_dev, int64_t n_faces, int iterations, double lambda,
                    double mu, int boundary_mode, const uint8_t *fixed_dev, float *verts_out_dev, uint8_t *class_out_dev,
                    int64_t *report_host, int device, void *stream);

/* ------------------------------------------------------------------------------------------
 * A triangle mesh denoised with its sharp edges kept: the face normals are filtered first, then the
 * vertices are moved toward the filtered normals (Sun, Rosin, Martin and Langbein, "Fast and effective feature-preserving
 * mesh denoising", TVCG 2007; the weight max(0, ni . nj - T)^2 needs +, -, *, / and sqrt only, which are correctly rounded,
 * where a Gaussian bilateral weight needs an exp).  Faces are not touched; no vertex is added, removed or renumbered.  The
 * project's own definition.  Every result is a function of the input alone (integer atomics only, float64 sums in one stated
 * order): equal inputs give equal bytes.  Called by nothing else in the library: opt-in.
 *  a. arguments are checked before the device is touched; the message names the offending one.  An index out of range, a
 *     non-finite vertex or a face with a repeated index: P2S_EINVAL, before anything dereferences it, and nothing is written.
 *     n_verts, n_faces <= 2^27.  threshold (T) finite, 0 <= T < 1.  normal_iterations and vertex_iterations in 0 .. 10000.
 *     boundary_mode 0 (boundary vertices fixed) or 1 (free).  verts_out_dev [n_verts][3] is not NULL when n_verts > 0 and
 *     must not overlap verts_dev: the update is simultaneous and does not run in place.  fixed_dev [n_verts] uint8,
 *     normals_out_dev [n_faces][3] float and class_out_dev [n_verts] uint8 may be NULL.  n_faces = 0 or both counts 0 is
 *     legal: the output is the input's bytes, and the report, the classes and the normals are filled.
 *  b. the geometric normal of a face (a, b, c), in float64 from the float32 positions with contraction off:
 *         e1 = b - a, e2 = c - a per coordinate;  m = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x), every
 *         product rounded, then the difference;  l = sqrt((mx mx + my my) + mz mz);  n = (float) (m / l) per coordinate.
 *     If l is 0 or not finite the normal is (0, 0, 0) and the face is DEAD: it contributes nothing anywhere and keeps its
 *     zero normal.  Every other face is live.
 *  c. neighbours: N(i) of a face i are the faces, dead ones and i itself included, that share at least one vertex INDEX
 *     with i, each once however many vertices it shares, taken in ASCENDING face index.
 *  d. one normal iteration: every live face i reads the float32 normals of the previous iteration (the update is
 *     simultaneous) and computes in float64, s = (0, 0, 0) at first, for j in N(i) in order:
 *         d = (nix njx + niy njy) + niz njz;  if d > T:  w = (d - T) (d - T);  s = s + w nj per coordinate (a rounded
 *         product, then a rounded sum);
 *     then l = sqrt((sx sx + sy sy) + sz sz) and n' = (float) (s / l); if l is 0 or not finite the face keeps its normal.
 *     d = T contributes nothing, and a dead neighbour has d = 0 <= T.  Normals are float32 between iterations.  After
 *     normal_iterations rounds they are the TARGET normals, which normals_out_dev receives (with 0 rounds: the geometric
 *     ones).
 *  e. classes, one byte per vertex in class_out_dev; the first that applies:
 *       2 masked: fixed_dev[i] != 0
 *       3 unreferenced: in no face
 *       4 no live face at the vertex
 *       1 boundary, fixed: mode 0 and the vertex lies on an edge of exactly one face (dead faces count as faces here)
 *       0 free
 *     Classes 1 .. 4 keep their input bytes, the sign of a zero included; the faces around them still read them.
 *  f. one vertex iteration: every vertex p of class 0, with the live faces f1 < f2 < .. < fk that hold it, reads the
 *     float32 positions of the previous iteration (the update is simultaneous) and computes in float64, s = (0, 0, 0) at
 *     first, per face with the corners (a, b, c) as stored and the target normal n:
 *         g = ((a + b) + c) / 3.0 per coordinate;  d = (nx (gx - px) + ny (gy - py)) + nz (gz - pz);  s = s + n d per
 *         coordinate;
 *     then p' = (float) (p + s / (double) k), rounded to nearest even, subnormal results kept.  If an output coordinate is not
 *     finite the call fails with P2S_EINVAL ("the result is not finite"): the report is filled, nothing else is written.
 *  g. report_host [16] int64: [0] n_verts | n_faces << 32   [1] .. [5] the vertices of the classes 0 .. 4   [6] dead faces
 *     [7] the largest |N(i)| over the live faces (0 if there is none)   [8] normal iterations run: normal_iterations, and
 *     0 if no face is live   [9] vertex iterations run: vertex_iterations, and 0 if no vertex is of class 0   [10] the
 *     bits of the float64 maximum over the vertices of (dx dx + dy dy) + dz dz between input and output, as for
 *     p2s_mesh_smooth (0 if [9] is 0)   [11] non-finite output coordinates   [12..15] 0.
 *  h. the result depends on the arrays as given: the sums follow the face index and a centroid the stored corner order, so
 *     renumbering faces or vertices, or rotating a face's corners, may change the last bit.  Flipping a face flips its
 *     normal, and faces of opposite orientation do not see each other (d < 0 <= T): orient the mesh first
 *     (p2s_mesh_repair).  Faces are connected by vertex INDEX: nothing is welded.  Limits: the face weights are uniform (no
 *     area weight); T is the caller's, nothing chooses it; a fan of d faces at one vertex costs O(d^2) per normal
 *     iteration (9 M neighbour visits at d = 3,000); the result is not tested for self-intersections (p2s_mesh_check finds
 *     them afterwards).
 * Scratch comes from the device's block cache and returns to it before the call ends.  Synchronises `stream`. */
int p2s_mesh_denoise(const float *verts_dev, int64_t n_verts, const int32_t *faces_dev, int64_t n_faces, double threshold,
                     int normal_iterations, int vertex_iterations, int boundary_mode, const uint8_t *fixed_dev, float *verts_out_dev,
                     float *normals_out_dev, uint8_t *class_out_dev, int64_t *report_host, int device, void *stream);

/* ------------------------------------------------------------------------------------------
 * A shaded picture of a handle's mesh: what the reference leaves to an external viewer behind
 * source/figure/distance_vis.py.  The project's own definition.  Everything is float64 with contraction off and uses
 * + - * / sqrt min max floor copysign and comparisons only, dot = (x x' + y y') + z z', sums of three terms left to right:
 * equal inputs give equal bytes, and tests/figure_model.py restates it in numpy.  No floating-point atomic.
 *  a. refusals, each P2S_EINVAL with a message and nothing written, in this order: m, prm or rgb_out_dev NULL; width or
 *     height < 1; samples outside 1 .. 4; ao_rays outside 0 .. 64; ao_dirs_dev NULL with ao_rays > 0 (or not NULL with 0);
 *     projection or shading outside 0 .. 1; width * height * samples^2 > 2^28; a camera vector, the extent of the projection
 *     in use (which is also > 0), ao_radius, ao_bias, ambient, diffuse, base_rgb or background_rgb not finite (|x| > 1e300);
 *     right, up, forward not orthonormal (a dot product more than 2^-40 from 1 or 0); ao_radius or ao_bias < 0; then, with
 *     the handle's device current: vertex_rgb_dev, ao_dirs_dev or an output that is not memory of that device.
 *  b. samples.  Pixel (i, j), i from the left and j from the top, has ss x ss samples (a, b), ss = samples:
 *         sx = (2 (i + (a + 0.5) / ss)) / W - 1        sy = 1 - (2 (j + (b + 0.5) / ss)) / H
 *     pinhole (projection 0):       o = eye,  d = (forward + (sx tan_half_w) right) + (sy tan_half_h) up   (not normalised: t
 *                                   is in units of d, as in p2s_mesh_raycast)
 *     orthographic (projection 1):  o = (eye + (sx half_w) right) + (sy half_h) up,  d = forward
 *     The sample image has W ss columns and H ss rows; sample (X, Y) = (i ss + a, j ss + b) is entry Y (W ss) + X.
 *  c. the primary hit is p2s_mesh_raycast's of that ray with t_max = +inf, every rule of that section included:
 *     depth_out_dev and face_out_dev [H ss][W ss] (each may be NULL) equal what it returns, bit for bit; a miss is +inf, -1.
 *  d. shading of a hit on face f with the corners A, B, C in the order the handle stores them (an inward-oriented closed mesh
 *     is stored flipped: B and C swapped): e1 = B - A, e2 = C - A, nf = e1 x e2, s = o - A, q = s x d, dn = d . nf,
 *     u = -(e2 . q) / dn, v = (e1 . q) / dn, w = (1 - u) - v.  Normal: the stored unit normal of f; with shading 1 and no
 *     corner flagged as touching a sliver or zero-area face, m = (w N_A + u N_B) + v N_C per coordinate with N the handle's
 *     angle-weighted vertex normal (fixed point / 2^40, exact), and n = m / sqrt(m . m) unless m . m is 0 or not finite.
 *     dl = d / sqrt(d . d), c = n . dl; if c > 0 both n and c change sign; lambert = -c (a two-sided headlight).
 *     Albedo: base_rgb, or with vertex_rgb_dev [V][3] float (V the handle's vertices; the values are not checked) per
 *     channel (w C_A + u C_B) + v C_C.
 *  e. ambient occlusion, ao_rays = K > 0: sg = copysign(1, nz), a = -1 / (sg + nz), b = (nx ny) a,
 *     t1 = (1 + ((sg nx) nx) a, sg b, -(sg nx)), t2 = (b, sg + (ny ny) a, -ny) (Duff et al., JCGT 2017); for every row h of
 *     ao_dirs_dev [K][3] float64 (unit, z >= 0; not checked: a non-finite row is never occluded)
 *     dir = (hx t1 + hy t2) + hz n per coordinate, from p = (o + t d) + ao_bias n; the ray is occluded iff any face is hit
 *     with t in (0, ao_radius] under the acceptance rules of c (ao_radius 0: none is).  ao = (K - occluded) / K; 1 if K = 0.
 *  f. sample colour per channel = min(max(albedo (ambient ao + diffuse lambert), 0), 1) (a NaN gives 0); a miss gives
 *     background_rgb clamped likewise.  Pixel = (the sum of its samples from 0.0, b outer and a inner) / ss^2;
 *     byte = floor(255 sqrt(x) + 0.5): gamma 2, because sqrt is correctly rounded everywhere.  rgb_out_dev [H][W][3].
 *  g. stats_host [8] (may be NULL): primary rays, primary hits, occlusion rays, occlusion rays occluded, ray-triangle tests
 *     (both walks), 0, 0, 0.  A traversal stack overflow (impossible for an index of at most 7 levels) fails the call with
 *     P2S_EHIP as in p2s_mesh_raycast.
 * Limits: one headlight; no shadow but the occlusion term; no texture; no transparency; the regular sample grid aliases on
 * features thinner than a sample.  Scratch (84 bytes per sample) comes from the device's block cache.  Synchronises `stream`. */
typedef struct {
    int32_t width, height, samples;       /* W, H, ss per axis (1 .. 4) */
    int32_t projection, shading;          /* 0 pinhole, 1 orthographic; 0 flat, 1 smooth */
    int32_t ao_rays;                      /* K, 0 .. 64 */
    double  eye[3], right[3], up[3], forward[3];
    double  tan_half_w, tan_half_h;       /* pinhole */
    double  half_w, half_h;               /* orthographic */
    double  ao_radius, ao_bias, ambient, diffuse;
    double  base_rgb[3], background_rgb[3];
} p2s_render_params;
int p2s_mesh_render(p2s_trimesh_t m, const p2s_render_params *prm, const float *vertex_rgb_dev, const double *ao_dirs_dev,
                    uint8_t *rgb_out_dev, double *depth_out_dev, int32_t *face_out_dev, int64_t *stats_host, void *stream);

/* ------------------------------------------------------------------------------------------
 * "next" row: the pairs of faces of a handle's mesh that intersect, and its non-manifold vertices -- what
 * the verdict "a volume" of p2s_mesh_repair (trimesh's is_volume) does not see, and what the pseudonormal sign of
 * p2s_mesh_distance assumes absent.  The project's own definition (trimesh offers none); every result is a function of
 * the input alone.  Precondition: welded input, as p2s_mesh_repair writes it -- faces share a vertex when they share a
 * vertex INDEX; two vertices with equal coordinates and different indices are different vertices (unwelded input is out of
 * contract: its seams show as touching or coplanar pairs).
 * Arithmetic: float64 on the handle's triangles, contraction off, one operation order:
 *     orient3(a, b, c, d) = ((b - a) x (c - a)) . (d - a)   (the cross product and (x + y) + z dot of the whole unit)
 *     side_T(p) = orient3(a, b, c, p) for T = (a, b, c);  the volume of an edge (p, q) with an edge (x, y) = orient3(p, q, x, y)
 *     orient2 = (bx - ax)(cy - ay) - (by - ay)(cx - ax) on the two axes kept after the axis of the largest |n| is dropped
 *     (n of the pair's smaller face, or of the triangle an edge is tested against; the first axis among equals).
 * A value is a sign only beyond its filter bound, 2^-43 S^3 for orient3 and 2^-47 S^2 for orient2, S the largest
 * |coordinate| of the mesh: beyond it the computed sign IS the exact sign (proof: csrc/p2s_meshcheck.inl); within it the
 * sign is 0.
 * Faces under the degenerate rule (|ab x ac|^2 <= 2^-90 |ab|^2 |ac|^2) are skipped and counted.  A pair (f, g), f < g, of
 * the other faces, with k common indices:
 *  - k = 3: a duplicate, counted, not tested.
 *  - the closed bounding boxes of the two faces do not meet: disjoint.
 *  - the side values of the vertices that are not shared are taken (a shared vertex has the sign 0).  All 0: the pair lies
 *    in one plane.  It is COPLANAR when no edge line of either triangle has all three vertices of the other on its outer
 *    side or on it (orient2 signs, 0 counting as on it): the triangles overlap in an open set; for k = 1 this is "the two
 *    wedges overlap", for k = 2 "the opposite vertices lie strictly on the same side of the shared edge" (a fold).  A pair
 *    in one plane that is not coplanar is disjoint when k > 0 (it meets in its shared vertices) or when some edge line has
 *    the other triangle strictly outside, else TOUCHING (also when a projected triangle has the orientation 0).
 *  - otherwise k = 2 is disjoint, and so is a pair where the unshared vertices of one triangle lie strictly on one side
 *    of the other.  What remains: every edge (p, q) of one triangle whose end points are both unshared (k = 1: the edge
 *    opposite the shared vertex) against the other triangle T.  It PIERCES when side_T(p), side_T(q) are strictly
 *    opposite and its volumes with the three edges of T have one strict sign.  It CANNOT when the sides are strictly
 *    equal, or two volumes are strictly opposite, or -- both sides 0, the edge lies in the plane of T -- in that plane an
 *    edge line of T has p and q strictly outside or the line (p, q) has T strictly on one side.  The pair is INTERSECTING
 *    when an edge pierces, else TOUCHING unless every edge cannot (a vertex on a face, an edge against an edge), else
 *    disjoint.  Touching pairs are counted and stored with their class, never reported as intersecting.
 * A vertex is manifold when its faces form one fan, open or closed: faces are neighbours across an undirected edge that
 * exactly two faces use (edges of more than two faces connect nothing; on a consistently oriented mesh this is the handle's
 * own adjacency), the walk starts at the vertex's smallest face and rotates both ways; the vertex is flagged when it
 * reaches fewer faces than the vertex has.
 * method 0 = a walk of the handle's octree per face with the face's own box (node boxes against it), 1 = every face
 * against every other (the yardstick): identical arrays and reports except report [2].
 * Outputs (device, each may be NULL): pairs_out_dev [cap_pairs][2] int32, (f, g) with f < g ascending by f, then g;
 * class_out_dev [cap_pairs] (1 intersecting, 2 coplanar, 3 touching; needs pairs_out_dev); face_flags_out_dev [n_faces]
 * (bits: 1 / 2 / 4 in an intersecting / coplanar / touching pair, 8 degenerate); vert_flags_out_dev [n_verts] (1: not
 * manifold).  report_host [16] int64:
 *   [0] faces tested   [1] degenerate faces skipped   [2] candidate pairs given to the narrow phase   [3] intersecting pairs
 *   [4] coplanar pairs   [5] touching pairs   [6] duplicate pairs   [7] faces in an intersecting or coplanar pair
 *   [8] intersecting or coplanar pairs inside one component   [9] ... across components (both -1 on a mesh that is not
 *   closed: the handle has no labels)   [10] non-manifold vertices   [11] pairs to store ([3] + [4] + [5])   [12..15] 0.
 * cap_pairs < report [11] with pairs_out_dev: P2S_EINVAL, the report filled, no output written.  Scratch comes from the
 * device's block cache and returns to it before the call ends.  Synchronises `stream`.
 * ------------------------------------------------------------------------------------------ */
int p2s_mesh_check(p2s_trimesh_t m, int method, int64_t cap_pairs, int32_t *pairs_out_dev, uint8_t *class_out_dev,
                   uint8_t *face_flags_out_dev, uint8_t *vert_flags_out_dev, int64_t *report_host, void *stream);

/* ------------------------------------------------------------------------------------------
 * "next" row: inside / outside of a CLOSED mesh on the volume's grid, and the reductions of the
 * reconstruction-quality report (volumetric IoU, F-score, normal consistency: points2surf_amd/metrics.py, mesh_quality).
 * The project's own definition; every result is a function of the input alone.
 * Grid: grid_res = R in 2..1024; voxel (i, j, k) has the centre (c(i), c(j), c(k)), c(i) = the float32 nearest to
 * ((i + 0.5) / R) * 2.0 - 1.0 evaluated in float64 (volume_space_to_model_space of the reference's source/sdf.py:78, rounded as
 * its query grids are): a float32 value held exactly in float64, like every mesh coordinate.  occ_out_dev is [R][R][R]
 * uint8, x-major with z fastest (the layout of p2s_sdf_volume): 1 inside, 0 outside.  The handle must be closed (info[1]),
 * else P2S_EINVAL and nothing written; an inward-oriented closed mesh is stored flipped and voxelised as stored.
 * Arithmetic: float64, contraction off, orient3 and the filter bounds of p2s_mesh_check with S' = max(S, 1) in the place
 * of S (S the mesh's largest |coordinate|; |c| < 1): 2^-47 S'^2 in the plane, 2^-43 S'^3 in space (why the proof carries
 * over: csrc/p2s_meshvoxel.inl).  orient2(a, b, c) = (bx - ax)(cy - ay) - (by - ay)(cx - ax) ALWAYS on x and y, z dropped.
 * A column is the line x = c(i), y = c(j).  For a face T = (a, b, c) of the handle and P = (c(i), c(j)):
 *     sigma = sign orient2(a, b, c);   s0, s1, s2 = sign orient2(b, c, P), orient2(c, a, P), orient2(a, b, P),
 * each a sign only beyond 2^-47 S'^2, else 0.
 *  - The column MISSES T when P lies outside T's closed xy bounding box (exact comparisons), or when some s is > 0 and
 *    another is < 0.
 *  - The column CROSSES T with the direction sigma when sigma != 0 and s0 = s1 = s2 = sigma: all four signs are then
 *    exact and P lies strictly inside the projected triangle.
 *  - Anything else makes the COLUMN UNDECIDED: P within rounding of an edge or a vertex, or the face seen edge-on with P
 *    not strictly clear of it.  Degenerate faces get no rule of their own; they can never be crossed.
 * For a decided column and a crossing (T, sigma), the voxel with the centre p lies below the crossing when
 * sign(orient3(a, b, c, p), beyond 2^-43 S'^3) * sigma < 0 and above it when > 0; the sign 0 makes the VOXEL UNDECIDED.  The
 * winding number of a decided voxel is w = the sum of sigma over the crossings it lies below -- every predicate that
 * decided it is exact, so w is the exact integer winding number -- and occ = (w != 0): a cavity (an inward shell inside an
 * outward one) is empty, the overlap of two solids is inside.
 * The undecided voxels (every voxel of an undecided column and the singly undecided ones, U in all) are decided by the
 * exact winding sum of p2s_mesh_winding, method 1, on their centres: inside iff |w| > 0.5.  flags_out_dev [R][R][R] (may be
 * NULL) is 1 for them, 0 otherwise.  U * n_faces is what they cost: U > max_fallback returns P2S_ECAPACITY with the
 * report filled ([0] then counts the decided voxels only) and NO output written.
 * method 0 = one column per thread walks the handle's octree, a node being opened when its closed xy rectangle contains
 * P (every face sits in exactly one leaf, so none is met twice; a stack overflow fails the call as in the other walks);
 * method 1 = every column against every face (the yardstick): identical arrays and reports except report [4].
 * report_host [8] int64: [0] voxels inside   [1] undecided columns   [2] singly undecided voxels (in decided columns)
 *   [3] U = R * [1] + [2]   [4] (column, face) tests made (method 1: R^2 n_faces)   [5] crossings, over all columns
 *   [6], [7] 0.
 * Scratch comes from the device's block cache and returns to it before the call ends.  Synchronises `stream`.
 * ------------------------------------------------------------------------------------------ */
int p2s_mesh_voxelize(p2s_trimesh_t m, int grid_res, int method, int64_t max_fallback, uint8_t *occ_out_dev,
                      uint8_t *flags_out_dev, int64_t *report_host, void *stream);
/* n surface samples of the mesh `from` measured against the mesh `to`: dist_dev [n] float64 (unsigned, p2s_mesh_distance
 * on `to`), face_from_dev [n] the sample's own face (p2s_mesh_sample_surface), face_to_dev [n] the nearest face on `to`.
 * out_host [4 + n_taus]: sum d, sum d^2, max d, sum |n_from . n_to| (the handles' stored unit normals), then the count of
 * d <= taus_host[t] for each of the n_taus <= 8 thresholds.  *nc_pairs_host = the pairs in the normal sum: a pair with a
 * face under the degenerate rule (its stored normal is 0), or with a face id out of range (-1: a non-finite query), is
 * left out.  float64 sums in an order that depends on n alone (csrc/p2s_meshvoxel.inl): two runs give the same bits.
 * Both handles on one device.  Synchronises `stream`. */
int p2s_surface_stats(p2s_trimesh_t from, p2s_trimesh_t to, const double *dist_dev, const int32_t *face_from_dev,
                      const int32_t *face_to_dev, int64_t n, const double *taus_host, int n_taus, double *out_host,
                      int64_t *nc_pairs_host, void *stream);
/* counts_host [3] = |A|, |B|, |A and B| of two occupancy arrays of n bytes (a byte that is not 0 is occupied).
 * Synchronises `stream`. */
int p2s_occupancy_counts(const uint8_t *occ_a_dev, const uint8_t *occ_b_dev, int64_t n, int64_t *counts_host, int device,
                         void *stream);

/* ------------------------------------------------------------------------------------------
 * Screened Poisson baseline: an oriented cloud -> mesh, without the network.  The reference runs
 * MeshLab's Screened Poisson filter here (eval_dataset.py, poisson.mlx); this is the project's OWN definition of the
 * stage -- regular grids, trilinear elements, a cascade of levels -- and is not pinned against MeshLab.
 *
 * Box: centre = midpoint of the cloud's bounding box, side = scale * its largest extent (float64).  Level d = 3 .. depth
 * has R = 2^d + 1 nodes per axis, h = side / 2^d, node (i, j, k) at lo + h (i, j, k), C order with axis 0 = x.  Per level,
 * with W [n][R^3] the trilinear weights (cell = clamp(floor((p - lo) / h), 0, R - 2) per axis), n_occ the distinct cells
 * that hold a point, a = n_occ h^2 / n and lambda = point_weight a / h:
 *     A = s(x)m(x)m + m(x)s(x)m + m(x)m(x)s + lambda W^T W,    b = (g(x)m(x)m) v_x + (m(x)g(x)m) v_y + (m(x)m(x)g) v_z,
 *     v = (a / h^3) W^T (-N),   m / s / g the 1-D mass / stiffness / derivative matrices with natural ends,
 * solved by CG preconditioned with diag(A) from the trilinear prolongation of the level below (zero at level 3) until
 * |r| <= cg_tol |b| -- tested after every iteration, so a level makes at least one -- or max_iters (reported, no error).
 * iso = the mean of (W chi)_p (float64); volume = chi - iso, float32 [R]^3, every node of the six border faces then set
 * to -|value|; surface = p2s_marching_cubes of it at 0 (inside: value > 0, fix_inversion), vertices mapped to lo + h v.
 * Vectors are float32, every sum over points and every reduction float64, no floating-point atomics: equal inputs give
 * equal bytes.
 *
 * info_host [P2S_POISSON_INFO] (may be NULL): [0..2] lo, [3] h of the finest level made, [4] iso, [5] levels made, then
 * per level d at [8 + 5 (d - 3)]: lambda, n_occ, iterations, final |r| / |b|, milliseconds.
 * P2S_EINVAL before anything is written: n < 1 (or > 2^24), a non-finite point or normal, all normals zero, a cloud of
 * zero extent, point_weight <= 0, scale < 1, cg_tol <= 0, max_iters < 1, depth outside 3..9.
 * ------------------------------------------------------------------------------------------ */
typedef struct p2s_poisson_params_t {
    int32_t depth;            /* 3..9 */
    int32_t max_iters;        /* CG iterations per level, >= 1 */
    double point_weight;      /* alpha > 0 (MeshLab's pointWeight; 4) */
    double scale;             /* >= 1 (1.1) */
    double cg_tol;            /* > 0 (1e-3) */
} p2s_poisson_params_t;
#define P2S_POISSON_INFO 48
/* points_dev / normals_dev [n][3] float32 (normals outward, any length).  vol_out_dev (may be NULL) [R]^3 float32 of the
 * finest level.  verts_out_dev [cap_verts][3], faces_out_dev [cap_faces][3]: *n_verts / *n_faces receive the full counts;
 * too small a capacity is P2S_ECAPACITY as in p2s_marching_cubes (capacities 0 size the buffers; the volume and the info
 * are written either way).  Scratch comes from the device's block cache.  Synchronises `stream`. */
int p2s_poisson_reconstruct(const float *points_dev, const float *normals_dev, int64_t n, const p2s_poisson_params_t *params,
                            float *vol_out_dev, float *verts_out_dev, int64_t cap_verts, int32_t *faces_out_dev,
                            int64_t cap_faces, int64_t *n_verts, int64_t *n_faces, double *info_host, int device, void *stream);
/* The system of ONE level (3 <= level <= params->depth; the box is that of the cloud, whatever the level), the yardstick
 * of the solver: b_out_dev, diag_out_dev [R^3] (each may be NULL) and, when ax_out_dev is given, A . x_in_dev through the
 * kernels the CG runs.  info_host as above with lo, h and the slot of `level` (lambda, n_occ) filled.  Synchronises
 * `stream`. */
int p2s_poisson_system(const float *points_dev, const float *normals_dev, int64_t n, const p2s_poisson_params_t *params,
                       int level, const float *x_in_dev, float *b_out_dev, float *ax_out_dev, float *diag_out_dev,
                       double *info_host, int device, void *stream);

/* ------------------------------------------------------------------------------------------
 * Point normals from the cloud alone: what the Poisson baseline needs where no mesh exists (the
 * reference's 06_poisson_rec / normals_poisson.mlx variant, and real_world).  4 <= k <= 64, k <= n, else P2S_EINVAL; so is
 * a NULL cloud or normal array.  Scratch comes from the device's block cache; no floating-point atomics: equal inputs give
 * equal bytes.  Both synchronise `stream`.
 *
 * p2s_normals_estimate: the neighbourhood of point i is its k nearest points of the cloud as p2s_knn_patch ranks them
 * (float64 distances, ties by id, the point itself and duplicates included).  In float64: centroid c, covariance
 * C = sum (p - c)(p - c)^T, cyclic Jacobi with a fixed number of sweeps, the eigenvector of the smallest eigenvalue
 * (of equal ones the first axis in the order the iteration leaves them), normalised, rounded once to float32 ->
 * normals_out_dev [n][3].  variation_out_dev [n] (may be NULL) = lambda_0 / (lambda_0 + lambda_1 + lambda_2).  C = 0: normal
 * (0, 0, 0), variation 0.  The sign of a normal is unspecified but deterministic.
 *
 * p2s_normals_orient: Hoppe's propagation, made unique.  Graph: the undirected edges {i, j}, i != j, with j among the k
 * nearest of i or the reverse.  d = (a_x b_x + a_y b_y) + a_z b_z in float64 from the float32 normals, w = 1 - |d|.  Tree:
 * the minimum spanning forest under the total order (w, min(i, j), max(i, j)) -- for w >= 0 the order of its bit pattern.
 * Crossing a tree edge flips iff d < 0.  Per component the seed is the point of largest z (of equal ones the smallest id);
 * the component is negated as a whole iff the seed's oriented n_z < 0.  normals_out_dev (may be normals_in_dev) = the input
 * with only sign bits changed (all three of a flipped normal); component_out_dev [n] (may be NULL) = the smallest point id
 * of the point's component; info_host [8] (may be NULL) = components, undirected edges, Boruvka rounds that joined
 * components, normals flipped, 0 ....  A non-finite normal: P2S_EINVAL, nothing written.
 * ------------------------------------------------------------------------------------------ */
int p2s_normals_estimate(p2s_cloud_t c, int k, float *normals_out_dev, float *variation_out_dev, void *stream);
int p2s_normals_orient(p2s_cloud_t c, int k, const float *normals_in_dev, float *normals_out_dev, int32_t *component_out_dev,
                       int64_t *info_host, void *stream);

/* ------------------------------------------------------------------------------------------
 * "next" row: the per-shape text / debug files of save_evaluation and implicit_surface_to_mesh, written
 * by native HOST code (no device is touched; all pointers are host pointers).  Byte-identical to what the reference's
 * numpy / Python calls write.
 * p2s_write_txt_f32:       np.savetxt(path, sdf) (reference source/points_to_surf_eval.py:210): '%.18e' per line.
 * p2s_write_query_vis_ply: sdf.visualize_query_points (source/sdf.py:269-285) in the drop-in's PLY layout
 *                          (points2surf_amd/ply.py): float32 xyz + uchar rgba per query point.
 * p2s_write_coff_samples:  mesh_io.write_off(file, query_pts_ms, [], colors_vertex=...) with the colours of
 *                          source/sdf.py:203-209 (source/base/mesh_io.py:75-140): str() of every number.
 * A file that cannot be opened, written, flushed or closed: P2S_EIO with errno's text (never a silently truncated file).
 * ------------------------------------------------------------------------------------------ */
int p2s_write_txt_f32(const char *path, const float *values_host, int64_t n);
int p2s_write_query_vis_ply(const char *path, const float *query_host, const float *dist_host, int64_t n);
int p2s_write_coff_samples(const char *path, const float *query_host, const float *dist_host, int64_t n);

/* per-stage counters of the last p2s_encode_decode / p2s_infer_shape on this model
 * (HIP-event milliseconds on the launch stream; valid after the stream is synchronised) */
typedef struct {
    double  ms_chain_stn, ms_stn_head, ms_chain_main, ms_decoder, ms_knn, ms_subsample, ms_grid;
    int64_t queries;
    int64_t launches_chain;      /* number of point-chain kernel launches (2 per chunk; 3 with a QSTN) */
    double  ms_chain_qstn;       /* QSTN trunk launch (models with use_point_stn); its head layers count under ms_stn_head */
    int64_t fallback_queries;    /* fp16 pair encoder: queries of the call re-run through the fp32 kernels (activation > 6e4) */
    /* fp32 encoders, screened conv3 (0 with P2S_CONV3_DENSE=1 or where the dense conv3 runs).  The three took
       the place of three reserved slots: the size and the earlier members of the struct are unchanged.  They are counted on
       the device: p2s_get_counters copies them to the host (a blocking copy) and they are those of the last call only once
       the stream that call ran on has been synchronised */
    int64_t conv3_confirmed;     /* fp32 dot products computed for the max-pools of the screened items */
    int64_t conv3_items_dense;   /* items the screen could not decide (activation beyond the half range, ties beyond the
                                    candidate queue): run again through the dense conv3 inside the same kernel */
    int64_t conv3_items;         /* (query, encoder, pass) items that entered the screened kernel */
    /* stem reuse (fp32 models with a screened conv3 and a max pool): (query, encoder) items whose main
       encoder pass started at conv1 from the conv0b output the STN pass had saved; 0 where the stem is recomputed
       (p2s_model_cfg.stem_recompute, a chunk beyond stem_reuse_max_mb, P2S_CONV3_DENSE=1, every other mode).  Counted on the host at launch, in the place of
       a reserved slot: the size and the earlier members are unchanged */
    int64_t stem_items_reused;
    double  reserved[2];
} p2s_counters;
int p2s_set_profiling(p2s_model_t m, int enabled);
int p2s_get_counters(p2s_model_t m, p2s_counters *out);

/* ------------------------------------------------------------------------------------------
 * Training step  (replaces one iteration of the reference's train loop: model.train(); pred = model(batch);
 *                 loss = sum(compute_loss(...)); loss.backward(); optimizer.step() -- reference
 *                 source/points_to_surf_train.py:400-440, :537-563, source/sdf_nn.py:30-40)
 * p2s_max and p2s_max_no_feat_stn only, fp32 throughout; every other configuration is refused at creation with
 * P2S_EINVAL and a message that names the reason (QSTN, shared encoder / transformer, sum pooling, regression, fixed
 * patch radius, a net size other than 1024).  No floating-point atomics: equal inputs and equal state give equal bytes.
 *
 * Parameters (every .weight / .bias), buffers (every .running_mean / .running_var) and gradients are flat float arrays
 * in the order of the reference's state_dict (points2surf_amd/model_spec.py state_shapes); num_batches_tracked is one
 * counter, equal for every batch-norm.
 * ------------------------------------------------------------------------------------------ */
typedef struct p2s_trainer_s *p2s_trainer_t;

/* cfg: points_per_patch / sub_sample_size fix the two point counts; use_feat_stn: 1 = p2s_max, 0 = without the 64 x 64
 * feature transforms.  n_params / n_buffers must match the model (checked). */
int p2s_trainer_create(const p2s_model_cfg *cfg, int use_feat_stn, const float *params_host, int64_t n_params,
                       const float *buffers_host, int64_t n_buffers, int64_t num_batches_tracked, int device,
                       p2s_trainer_t *out);
int p2s_trainer_destroy(p2s_trainer_t t);
/* sizes of the flat arrays, the number of recorded max-pools (4 with feature transforms: feat_local.stn2, feat_local,
 * feat_global.stn2, feat_global; else 2) and the device bytes the trainer holds (any may be NULL) */
int p2s_trainer_sizes(p2s_trainer_t t, int64_t *n_params, int64_t *n_buffers, int64_t *n_pools, int64_t *resident_bytes);
/* Train-mode forward (batch statistics), both losses, backward.  The three network inputs follow p2s_encode_decode
 * (patch in patch space, sub-sample and query in model space; nothing is modified); per item dist_abs_dev [B] = |d|,
 * sign01_dev [B] = the 0 / 1 sign target, radius_dev [B] = the patch radius (the magnitude target is tanh(|d| / r)).
 * losses_host[0] = magnitude loss, [1] = sign loss (both weights 1, the total is their sum).  Blocking: returns after
 * the losses have reached the host.  On success the gradients are ready, the running statistics have been updated
 * (momentum 0.1, unbiased variance) and num_batches_tracked has been incremented.  B < 2: P2S_EINVAL.  A non-finite loss
 * or gradient: P2S_EINVAL, parameters and running statistics unchanged.  All activations stay resident until the next call. */
int p2s_trainer_forward_backward(p2s_trainer_t t, const float *patch_ps_dev, const float *sub_ms_dev, const float *query_dev,
                                 const float *dist_abs_dev, const float *sign01_dev, const float *radius_dev, int B,
                                 double *losses_host, void *stream);
/* torch.optim.SGD(lr, momentum) without dampening, weight decay or Nesterov, one launch over the flat arrays; needs the
 * gradients of a successful p2s_trainer_forward_backward since the last step */
int p2s_trainer_sgd_step(p2s_trainer_t t, double lr, double momentum, void *stream);
/* what: 0 parameters, 1 buffers, 2 gradients of the last step -> host (blocking); num_batches_tracked may be NULL */
int p2s_trainer_copy_out(p2s_trainer_t t, int what, float *host, int64_t n_floats, int64_t *num_batches_tracked);
/* the argmax every max-pool of the last step recorded (lowest index on exact ties): [n_pools][B][1024] int32 */
int p2s_trainer_pool_indices(p2s_trainer_t t, int32_t *host, int64_t n);
/* family_ms (may be NULL) receives the HIP-event milliseconds of the last step per kernel family -- [0] GEMM, [1] column
 * sums, [2] batch-norm apply / backward, [3] max-pool, [4] the small kernels; [5..7] unused -- measured only while
 * profiling is enabled; `enabled` switches it for the following steps */
int p2s_trainer_profile(p2s_trainer_t t, int enabled, double *family_ms);

/* The two losses of given predictions pred_dev [B][2] against the targets of p2s_trainer_forward_backward, without
 * gradients: what a validation pass reports for the logits of the inference path.  The same kernel and the same fixed
 * summation tree as the training step.  B >= 1.  Blocking. */
int p2s_train_losses(const float *pred_dev, const float *dist_abs_dev, const float *sign01_dev, const float *radius_dev,
                     int B, double *losses_host, void *stream);

/* Test hooks: single layers of the training step on caller-supplied shapes, through the host functions and kernels the
 * trainer itself runs (the same slab decisions, the K = 3 path included), with scratch of their own.  All arrays are device
 * memory of one device; blocking (`stream` is synchronised).  Non-positive sizes, arrays that are not device memory and
 * scratch that cannot be allocated are refused with a message.  Training does not call them.
 *
 * One linear layer, M rows: y_dev [M][N] = X W^T + b;  dW = dY^T X, db = column sums of dY, dx_dev [M][K] = dY W, or
 * += dY W with accum = 1.  params_dev and grads_dev share the layout of the trainer's flat arrays: W / dW [N][K] at 0,
 * b / db [N] at b_offset >= N * K (a test may leave a gap between the two). */
int p2s_debug_train_linear(const float *x_dev, const float *params_dev, int64_t b_offset, const float *dy_dev, float *y_dev,
                           float *dx_dev, float *grads_dev, int M, int N, int K, int accum, void *stream);
/* One batch-norm over y_dev [M][C], M >= 2, on batch statistics (eps 1e-5): z_dev [M][C] = gamma xhat + beta, through a
 * ReLU when relu != 0; mean_dev [C], invstd_dev [C]; then its backward: d_dev [M][C] holds dL/dz on entry and dL/dy on
 * return.  params_dev: gamma [C] at 0, beta [C] at second_offset >= C; grads_dev: d gamma and d beta, pending_dev: the batch
 * mean and the unbiased batch variance (what the running statistics are updated with), both laid out like params_dev. */
int p2s_debug_train_bn(const float *y_dev, const float *params_dev, int64_t second_offset, float *z_dev, float *mean_dev,
                       float *invstd_dev, float *pending_dev, float *d_dev, float *grads_dev, int M, int C, int relu, void *stream);
/* Which units the ReLUs of the last p2s_trainer_forward_backward let through (1: output > 0), so that a float64
 * restatement can differentiate the same piece of the piecewise-linear network where a pre-activation lies within fp32
 * rounding of zero -- the counterpart of p2s_trainer_pool_indices.  host [n] bytes: the layers in the order of the
 * reference's forward (feat_global: conv0a, conv0b, with feature transforms stn2.conv1 .. conv3, stn2.fc1, stn2.fc2, then
 * conv1, conv2; fc1_global; the same for feat_local and fc1_local; fc2; fc3), each [rows][channels] as the activations
 * are stored.  n must be the total number of such units (named in the message otherwise).  Blocking. */
int p2s_debug_train_relu_masks(p2s_trainer_t t, uint8_t *host, int64_t n);

/* ------------------------------------------------------------------------------------------
 * A set of clouds behind one handle: batches whose items come from many clouds, one call each
 * (the training loader: a batch of 501 items touches about as many shapes).
 *
 * The set BORROWS its clouds: it copies no points, uploads the table of their descriptors once and keeps their point
 * counts on the host.  The clouds must live on `device` and must outlive the set.  The set notes the streams it is used
 * on and drains them in p2s_cloudset_destroy, as a cloud handle does.
 *
 * cloud_of_host [Q] (HOST memory): item i belongs to clouds[cloud_of_host[i]].  Every call checks it on the host and
 * uploads it into a buffer of the set; P2S_EINVAL with a message that names the item and the cloud for an id outside
 * [0, n_clouds), for k (n) greater than that cloud's point count, and for k beyond the limit of p2s_knn_patch.  The
 * shuffle-and-pad branch of clouds smaller than the sub-sample stays with the per-cloud call.  Q = 0: P2S_OK, no launch.
 * ------------------------------------------------------------------------------------------ */
typedef struct p2s_cloudset_s *p2s_cloudset_t;
int p2s_cloudset_create(const p2s_cloud_t *clouds, int n_clouds, int device, p2s_cloudset_t *out);
int p2s_cloudset_destroy(p2s_cloudset_t s);
int p2s_cloudset_size(p2s_cloudset_t s, int32_t *n_clouds, int32_t *min_points);      /* either may be NULL */
/* item i receives exactly what p2s_knn_patch(clouds[cloud_of_host[i]], query i) writes: ids local to its cloud in
 * ascending distance, the patch in patch space, the radius (any of the three outputs may be NULL) */
int p2s_cloudset_knn_patch(p2s_cloudset_t s, const int32_t *cloud_of_host, const float *query_dev, int64_t n_queries, int k,
                           int32_t *ids_out_dev, float *patch_ps_out_dev, float *radius_out_dev, void *stream);
/* No new random-number definition: the ids are what the ONE stream of `r` gives when item after item, in the order
 * given, draws n ids by numpy's masked rejection for its own cloud -- byte for byte what p2s_subsample_uniform(r,
 * clouds[cloud_of_host[i]], 1, n, ...) for i = 0 .. Q-1 leaves in the outputs and in the generator.  An open session of
 * `r` is closed first.  ids_out_dev [Q][n] (NULL, together with pts_out_dev = NULL: only advance the stream),
 * pts_out_dev [Q][n][3] the points of each item's own cloud (may be NULL). */
int p2s_cloudset_subsample_uniform(p2s_rng_t r, p2s_cloudset_t s, const int32_t *cloud_of_host, int64_t n_queries, int n,
                                   int32_t *ids_out_dev, float *pts_out_dev, void *stream);

/* ------------------------------------------------------------------------------------------
 * Raw scans -> 04_pts (the project's own definitions, stricter than the reference's
 * make_pc_dataset.py): drop non-finite points, crop gross strays, remove statistical outliers, thin to a budget,
 * normalise to the unit cube.  All selection logic is float64 with contraction off; tests/prepare_model.py performs the
 * same operations in numpy.  No floating-point atomics: equal inputs give equal bytes.
 *
 * Common to the five selecting calls: pts_dev [n][3]; pts_out_dev [n][3] and ids_out_dev [n] int32 (neither may be NULL,
 * pts_out_dev must not alias pts_dev) receive the *n_out_host survivors in input order and their ids into the input (one
 * stable compaction: flags, prefix scan, scatter).  0 <= n <= 2^27; n = 0 is legal and gives 0.  Except for
 * p2s_prepare_finite a non-finite coordinate is P2S_EINVAL.  A stage that is switched off copies its input bit for bit.
 * Arguments are checked before the device is touched; the message names the offending argument.  Scratch comes from the
 * device's block cache and returns to it before the call ends.  All synchronise `stream`.
 *
 * p2s_prepare_finite: keeps the points whose three coordinates are finite.
 *
 * p2s_prepare_crop: per axis, on the float32 coordinates (-0 counts as +0), the order statistics of rank
 * floor(q (n - 1)) and ceil((1 - q) (n - 1)) (float64 arithmetic for the ranks), found exactly by bisection on the
 * ordered bit pattern: 32 counting passes.  The box [lo, hi] is widened to [lo - m (hi - lo), hi + m (hi - lo)] in float64;
 * a point is kept iff all three coordinates lie inside (bounds included).  0 <= quantile < 0.5 (0: off), margin >= 0.
 * bounds_host [12] (may be NULL): lo[3], hi[3] (the order statistics), box lo[3], box hi[3].
 *
 * p2s_prepare_outliers: d_i = (sum of the distances from point i to its k + 1 nearest points of the cloud, itself
 * included, in the order of p2s_knn_patch) / k, each distance sqrt((dx dx + dy dy) + dz dz) in float64 from the float32
 * coordinates.  mean and std (population form, two passes) are double sums in a fixed tree.  Point i is kept iff
 * d_i <= mean + std_ratio * std.  1 <= k <= 64, clamped to n - 1; std_ratio >= 0 (0: off); n < 2 keeps everything.
 * d_out_dev [n] float64 (may be NULL) receives d_i (not written when the stage is off or n < 2).  info_host [4] (may be
 * NULL): mean, std, threshold, the k used.
 *
 * p2s_prepare_voxel_thin: at most one point per cell of an R^3 grid over the cube [lo, lo + ext]^3, lo the bounding box's
 * minimum, ext its largest extent.  Cell index per axis min(R - 1, floor((p - lo) (R / ext))) (ext = 0: cell 0); the cell
 * keeps the point of smallest (dx dx + dy dy) + dz dz to its centre lo + (i + 0.5) (ext / R), of equal ones the lowest
 * id (integer atomic minima over the distance's bit pattern, then over the id).  resolution in 1 .. 1024: R given.
 * resolution = 0: n <= max_points copies the input; otherwise R is what this search leaves in lo:
 *   lo = 1, hi = 1024; while lo < hi: mid = (lo + hi + 1) / 2; if occupied(mid) <= max_points: lo = mid; else hi = mid - 1
 * (max_points >= 1).  info_host [2] (may be NULL): R (0 where the input was copied), occupied cells.
 *
 * p2s_prepare_normalize: c = (lo + hi) * 0.5, s = 1 / max extent of the bounding box, p' = (p - c) * s in float64,
 * rounded once to float32.  pts_out_dev may be pts_dev here.  info_host [4] (may be NULL): c, s.  n < 1: P2S_EINVAL; an
 * extent of 0 on every axis: P2S_EFLAT ("extent 0"), nothing written.  A zero extent on one or two axes is legal.
 *
 * p2s_prepare_gather: out row i = src row ids_dev[i], rows of `width` 32-bit words (points: 3, ids: 1); an id outside
 * [0, n_src) is P2S_EINVAL, nothing usable written.  The random thinning gathers a host-drawn permutation with it.
 *
 * p2s_prepare_restore: out [n][3] float64 = double(v) / scale + centre: a reconstruction back in the scan's own frame.
 *
 * p2s_prepare_clusters (a selecting call like the five above): points i != j are linked iff
 * (dx dx + dy dy) + dz dz <= radius * radius, dx, dy, dz the float64 differences of the float32 coordinates (the predicate of
 * p2s_ball_count); a cluster is a class of the transitive closure; label_out_dev [n] (may be NULL) receives the smallest point
 * id of i's cluster.  A cluster is kept iff its size >= min(min_points, size of the largest cluster): the largest always
 * survives, a non-empty cloud never comes back empty.  radius finite and > 0, min_points >= 1.  info_host [4] int64 (may be
 * NULL): clusters, size of the largest, label of the largest (of equal ones the smallest label), clusters removed.  The
 * points are binned into cells of edge radius (1 + 2^-20) over the bounding box and sorted by a 64-bit cell key; every point
 * tests the points of its 27 neighbouring cells and hooks into a union-find (integer atomicMin).  More than 2^20 cells on an
 * axis: P2S_EINVAL, "radius too small for this extent".  Memory is O(n).  A radius comparable to the cloud's extent degrades
 * to O(n^2) pair tests.
 * ------------------------------------------------------------------------------------------ */
int p2s_prepare_finite(const float *pts_dev, int64_t n, float *pts_out_dev, int32_t *ids_out_dev, int64_t *n_out_host, int device,
                       void *stream);
int p2s_prepare_crop(const float *pts_dev, int64_t n, double quantile, double margin, float *pts_out_dev, int32_t *ids_out_dev,
                     int64_t *n_out_host, double *bounds_host, int device, void *stream);
int p2s_prepare_outliers(const float *pts_dev, int64_t n, int k, double std_ratio, double *d_out_dev, float *pts_out_dev,
                         int32_t *ids_out_dev, int64_t *n_out_host, double *info_host, int device, void *stream);
int p2s_prepare_voxel_thin(const float *pts_dev, int64_t n, int64_t max_points, int resolution, float *pts_out_dev,
                           int32_t *ids_out_dev, int64_t *n_out_host, int64_t *info_host, int device, void *stream);
int p2s_prepare_normalize(const float *pts_dev, int64_t n, float *pts_out_dev, double *info_host, int device, void *stream);
int p2s_prepare_gather(const void *src_dev, int64_t n_src, int width, const int32_t *ids_dev, int64_t n_ids, void *out_dev, int device,
                       void *stream);
int p2s_prepare_restore(const float *verts_dev, int64_t n, const double *centre_host, double scale, double *out_dev, int device,
                        void *stream);
int p2s_prepare_clusters(const float *pts_dev, int64_t n, double radius, int64_t min_points, int32_t *label_out_dev, float *pts_out_dev,
                         int32_t *ids_out_dev, int64_t *n_out_host, int64_t *info_host, int device, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* P2S_HIP_H */
