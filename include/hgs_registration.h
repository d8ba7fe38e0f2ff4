/* hgs_registration.h — C-ABI of the MI355X-native scan-matching backend for hdl_graph_slam.
 *
 * This is the drop-in boundary behind
 *     pcl::Registration<PointXYZI,PointXYZI>::Ptr hdl_graph_slam::select_registration_method(ros::NodeHandle&)
 *     (reference: include/hdl_graph_slam/registrations.hpp:17, src/hdl_graph_slam/registrations.cpp:22-124).
 * The pcl::Registration adapter that forwards to these entry points is adapters/registration_hip.hpp; the
 * reference-side patch is shown in INTEGRATION.md.  Every function is extern "C", takes plain pointers and
 * sizes, returns an int status (HGS_OK == 0) and never throws.  There is no global mutable state: each
 * hgs_handle owns one HIP stream and its device buffers, so the two engine instances that live in one
 * nodelet manager (odometry: apps/scan_matching_odometry_nodelet.cpp:106, loop closure:
 * include/hdl_graph_slam/loop_detector.hpp:47) can run concurrently from different threads.
 * Thread safety: calls on ONE engine (and on its clouds) are serialised by a per-engine mutex, different engines are
 * independent.  hgs_destroy is the exception: it must not race with ANY other call on that engine or on one of its clouds
 * (including hgs_cloud_destroy / hgs_cloud_download from a garbage-collector thread) — the mutex it would have to wait on is
 * part of the object it deletes.  Destroy the engine after the threads that use it have finished with it; clouds that outlive
 * it are orphaned safely (hgs_cloud_destroy still frees them).
 *
 * Conventions
 *  - points: array of records with three consecutive floats x,y,z at the start of each record and a byte stride
 *    (32 for pcl::PointXYZI, 16 for float4, 12 for packed xyz).  Non-finite points are ignored.
 *  - 4x4 transforms: float[16], COLUMN-major (Eigen::Matrix4f::data()), mapping source -> target frame.
 *  - indices returned to the caller always refer to the caller's original point order.
 */
#ifndef HGS_REGISTRATION_H
#define HGS_REGISTRATION_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HGS_ABI_VERSION 5

enum hgs_status {
  HGS_OK = 0,
  HGS_ERR_INVALID_ARGUMENT = 1,
  HGS_ERR_NO_TARGET = 2,
  HGS_ERR_NO_SOURCE = 3,
  HGS_ERR_HIP = 4,      /* a HIP runtime call failed; hgs_last_error() has the text */
  HGS_ERR_NO_DEVICE = 5,
  HGS_ERR_UNSUPPORTED = 6,
  HGS_ERR_OUT_OF_MEMORY = 7, /* host allocation failed inside the backend (std::bad_alloc caught at the boundary) */
  HGS_ERR_INTERNAL = 8,      /* any other C++ exception caught at the boundary; hgs_last_error() has the text */
  HGS_ERR_COMM = 9           /* RCCL call failed / hgs_comm_init missing; hgs_last_error() has the text */
};

/* registration_method strings of registrations.cpp:26-121 that this backend implements. */
enum hgs_method {
  HGS_FAST_GICP = 0,  /* fast_gicp::FastGICP      — registrations.cpp:27-36   */
  HGS_FAST_VGICP = 1, /* fast_gicp::FastVGICP     — registrations.cpp:48-56   */
  HGS_NDT_OMP = 2,    /* pclomp::NormalDistributionsTransform — registrations.cpp:101-120 */
  HGS_ICP = 3         /* pcl::IterativeClosestPoint (point-to-point) — registrations.cpp:57-64; name "ICP_HIP" */
};

/* reg_nn_search_method (registrations.cpp:103,112-118) / FastVGICP neighbour search. */
enum hgs_neighbor_search {
  HGS_KDTREE = 0,  /* NDT_OMP only: radius search (resolution) over the centroids of the valid cells */
  HGS_DIRECT1 = 1,
  HGS_DIRECT7 = 2,
  HGS_DIRECT27 = 3
};

/* fast_gicp::RegularizationMethod of the k-NN covariances (FastGICP / FastVGICP::setRegularizationMethod).  hdl_graph_slam
 * never calls the setter, so the constructor default of the fast_gicp checkout applies: FROBENIUS per SURVEY.md A.2; a
 * checkout whose FastGICP constructor selects PLANE is matched by setting HGS_REG_PLANE. */
enum hgs_regularization {
  HGS_REG_FROBENIUS = 0,          /* ((C + 1e-3 I)^-1 / ||.||_F)^-1                         */
  HGS_REG_PLANE = 1,              /* U diag(1, 1, 1e-3) V^T                                 */
  HGS_REG_MIN_EIG = 2,            /* U diag(max(sigma_i, 1e-3)) V^T                         */
  HGS_REG_NORMALIZED_MIN_EIG = 3, /* U diag(max(sigma_i / sigma_max, 1e-3)) V^T             */
  HGS_REG_NONE = 4                /* C itself                                               */
};

typedef struct hgs_params {
  int32_t method;                     /* hgs_method                                                        */
  int32_t max_iterations;             /* reg_maximum_iterations           (64)                             */
  double transformation_epsilon;      /* reg_transformation_epsilon       (0.01)                           */
  double rotation_epsilon;            /* fast_gicp LsqRegistration        (2e-3), not exposed by hdl; ICP (0):
                                         cos(angle) threshold if > 0, else 1 - transformation_epsilon           */
  double max_correspondence_distance; /* reg_max_correspondence_distance  (2.5), FAST_GICP / ICP            */
  int32_t correspondence_randomness;  /* reg_correspondence_randomness    (20) = k of the covariance kNN, 1..64 */
  int32_t neighbor_search;            /* hgs_neighbor_search: NDT (DIRECT7), VGICP (DIRECT1)               */
  double resolution;                  /* reg_resolution                   (NDT 0.5 / VGICP 1.0)            */
  double ndt_step_size;               /* pclomp NDT step_size_            (0.1)                            */
  double ndt_outlier_ratio;           /* pclomp NDT outlier_ratio_        (0.55)                           */
  int32_t ndt_min_points_per_voxel;   /* VoxelGridCovariance              (6)                              */
  int32_t ndt_upstream_hd1_sign;      /* 1: reproduce upstream h_ang_d1 = (.., .., +sy); 0: exact 2nd derivative */
  int32_t lm_max_iterations;          /* fast_gicp LM inner tries         (10)                             */
  double lm_init_lambda_factor;       /* fast_gicp                        (1e-9)                           */
  int32_t device_id;                  /* HIP device ordinal                                                */
  int32_t regularization_method;      /* hgs_regularization               (FROBENIUS), FAST_GICP / FAST_VGICP  */
  int32_t ndt_line_search;            /* 0: ndt_omp as it runs (its More-Thuente loop never executes: every step is the
                                         Newton direction with length clamp(|dp|, eps/2, step_size)); 1: a working
                                         More-Thuente search (<= 10 trials, mu 1e-4, nu 0.9) — NOT the reference's result  */
  int32_t icp_reciprocal;             /* reg_use_reciprocal_correspondences (false), ICP only (was `reserved`, always 0) */
} hgs_params;

typedef struct hgs_result {
  float final_transformation[16]; /* getFinalTransformation(), column-major                                    */
  int32_t converged;              /* hasConverged()                                                            */
  int32_t iterations;             /* outer iterations executed                                                 */
  double error;                   /* GICP/VGICP: last accepted sum e^T M e; NDT: trans_probability (score/N);
                                     ICP: mean d2 of the last iteration's correspondences (DBL_MAX: none)     */
  double fitness_score;           /* getFitnessScore(max_range) — filled by the batch entry point, else NaN    */
  uint32_t num_inliers;           /* #source points with d2 <= max_range in that score                         */
  int32_t candidate_id;           /* index into the caller's candidate list (batch), else 0                    */
  int32_t lm_tries;               /* GICP: total LM tries; NDT: derivative passes; ICP: correspondence passes  */
  int32_t reserved;
} hgs_result;

typedef struct hgs_handle hgs_handle; /* one registration engine instance (one pcl::Registration object)   */
typedef struct hgs_cloud hgs_cloud;   /* a point cloud resident in HBM (a KeyFrame::cloud, keyframe.hpp:42) */

/* ---- engine life cycle -------------------------------------------------------------------------------- */
/* Fill *p with the factory defaults of registrations.cpp for `method`. */
int hgs_params_default(int32_t method, hgs_params* p);
/* Replaces `new fast_gicp::FastGICP / pclomp::NormalDistributionsTransform` + setters, registrations.cpp:27-36,101-120. */
int hgs_create(const hgs_params* p, hgs_handle** out);
/* Destroys the engine.  Clouds created on it that the caller has not destroyed yet are ORPHANED: their device memory is
 * released with the engine, the hgs_cloud objects stay valid for exactly one more call — hgs_cloud_destroy — and every other
 * entry point rejects them with HGS_ERR_INVALID_ARGUMENT (hgs_cloud_size reports 0).  Either order of destruction is safe. */
int hgs_destroy(hgs_handle* h);
const char* hgs_last_error(const hgs_handle* h); /* h may be NULL: error of the last failed hgs_create on this thread */
int hgs_abi_version(void);

/* ---- clouds resident on the device -------------------------------------------------------------------- */
/* Upload a host cloud: records of `stride_bytes` with x, y, z at floats 0..2 and, from 20 bytes on, the intensity at float 4
 * (pcl::PointXYZI: 32).  `pts` may be pageable memory and may be freed or overwritten as soon as the call returns: the host packs the
 * records into pinned chunks while it reads them and the DMA + device-side packing run behind it on the handle's stream (no
 * synchronisation; an error of those shows up at the next call that waits).  The cloud caches its search structure and
 * covariances once an engine has computed them, like fast_gicp keeps them per input pointer.  A cloud belongs to the
 * handle that created it (its memory is recycled in that handle's stream order): using it with another handle is
 * rejected with HGS_ERR_INVALID_ARGUMENT.  The library does not change the process environment; the number of hardware
 * queues the HIP runtime spreads streams over (GPU_MAX_HW_QUEUES, read once at HIP's initialisation) is the launcher's to set:
 * INTEGRATION.md. */
int hgs_cloud_create(hgs_handle* h, const void* pts, size_t n, size_t stride_bytes, hgs_cloud** out);
int hgs_cloud_destroy(hgs_cloud* c);
size_t hgs_cloud_size(const hgs_cloud* c);
/* Device memory the cloud currently holds, in bytes: points, search index, covariances, correspondence seeds and — once it has served as an NDT /
 * VGICP target — its voxel tables.  What a cache of resident keyframes (adapters/loop_match_hip.hpp; the reference keeps every KeyFrame::cloud for the
 * life of the graph, include/hdl_graph_slam/keyframe.hpp:44) budgets against.  0 for NULL or an orphaned cloud. */
size_t hgs_cloud_device_bytes(const hgs_cloud* c);
/* Drop cached search structure / covariances (forces the cold path again; used by benchmarks). */
int hgs_cloud_invalidate(hgs_cloud* c);

/* ---- pcl::Registration surface (methods the callers use: SURVEY §8b) ---------------------------------- */
/* setInputTarget — scan_matching_odometry_nodelet.cpp:172,246 ; loop_detector.hpp:122 */
int hgs_set_target(hgs_handle* h, const void* pts, size_t n, size_t stride_bytes);
int hgs_set_target_cloud(hgs_handle* h, hgs_cloud* c); /* borrowed, must outlive its use */
/* setInputSource — scan_matching_odometry_nodelet.cpp:177 ; loop_detector.hpp:136 */
int hgs_set_source(hgs_handle* h, const void* pts, size_t n, size_t stride_bytes);
int hgs_set_source_cloud(hgs_handle* h, hgs_cloud* c);
/* align(output, guess) + hasConverged() + getFinalTransformation() — odometry_nodelet.cpp:210-220 ; loop_detector.hpp:143-153
 * Deviation from fast_gicp, stated: HGS_FAST_VGICP addresses the target's voxels by a 32-bit linear key over the bounding box of
 * the target's voxel coordinates floor(p / resolution - 0.5) (fast_gicp's GaussianVoxelMap hashes the three coordinates and has no such limit).  A target
 * whose box holds more than INT_MAX = 2147483647 cells (1291 cells per axis; one stray return 1.3 km away at resolution 1.0) has no map: hgs_align,
 * hgs_loop_match_batch[_sharded] and hgs_debug_gicp_linearize / hgs_debug_vgicp_voxels return HGS_ERR_UNSUPPORTED, hgs_last_error() names the grid size,
 * and the engine stays usable (set another target, or remove the stray points: the prefilter's distance filter does). */
int hgs_align(hgs_handle* h, const float guess[16], hgs_result* out);
/* The `output` cloud of align(): out_pts[i].xyz = T * source[i].xyz (records of stride_bytes; other bytes untouched). */
int hgs_transform_source(hgs_handle* h, const float T[16], void* out_pts, size_t stride_bytes);
/* getFitnessScore(max_range) with PCL's semantics (information_matrix_calculator.cpp:49-80): mean of the
 * squared 1-NN distances d2 over source points with d2 <= max_range (sic), DBL_MAX if none. */
int hgs_fitness(hgs_handle* h, const float T[16], double max_range, double* score, uint32_t* num_inliers);
/* getSearchMethodTarget()->nearestKSearch(pt, 1, ...) for a batch of query points (odometry_nodelet.cpp:314-321). */
int hgs_nn_target(hgs_handle* h, const float* q_xyz, size_t nq, size_t stride_bytes, int32_t* idx, float* d2);

/* ---- loop-closure batch: LoopDetector::matching, loop_detector.hpp:117-171 ----------------------------- */
/* Registers every candidate (source) against the handle's current target with its own guess, then evaluates
 * getFitnessScore(max_range) for each.  out[i] is filled for all candidates.  *best receives the index the
 * sequential rule of loop_detector.hpp:147-153 selects (skip non-converged, skip score > best, ties replace ->
 * the LAST minimal candidate wins), or -1 if none. */
int hgs_loop_match_batch(hgs_handle* h, hgs_cloud* const* candidates, size_t n_candidates, const float* guesses /* 16*n */,
                         double max_range, hgs_result* out, int32_t* best);
/* The candidates of SEVERAL new keyframes in one batch: LoopDetector::detect (loop_detector.hpp:57-68) calls matching once per new keyframe of a
 * graph update — up to max_keyframes_per_update of them — and every call is a short launch chain that does not fill the device.  Group g registers
 * candidates[group_offsets[g] .. group_offsets[g + 1]) against targets[g], each followed by getFitnessScore(max_range); out[i].candidate_id is the
 * index inside the group and best[g] what hgs_select_best gives over the group's records (-1: none, also for an empty group).  Every record is
 * bitwise what hgs_set_target_cloud(targets[g]) + hgs_loop_match_batch over that group alone returns.  The handle's own target and source
 * (hgs_set_*) are neither used nor changed.  A group may be empty (its target may then be NULL); n_groups == 0 returns HGS_OK.  Inside one group
 * the candidate clouds must be distinct; across groups a cloud may repeat, and a cloud may be the target of one group and a candidate of another.
 * HGS_FAST_GICP and HGS_ICP; HGS_NDT_OMP and HGS_FAST_VGICP return HGS_ERR_UNSUPPORTED (call hgs_loop_match_batch per target). */
int hgs_loop_match_groups(hgs_handle* h, hgs_cloud* const* targets, size_t n_groups,
                          const size_t* group_offsets /* n_groups + 1, non-decreasing, [0] = 0 */,
                          hgs_cloud* const* candidates /* group_offsets[n_groups] */,
                          const float* guesses /* 16 floats per candidate, column-major */,
                          double max_range, hgs_result* out /* one per candidate */,
                          int32_t* best /* n_groups entries, -1 = none; NULL ok */);
/* n INDEPENDENT registrations in one batch, every registration method: problem i registers sources[i] against targets[i] from the guess at
 * guesses + 16 * i with the handle's method and parameters.  The primitive under the grouped call (repeat a target, hgs_select_best per group —
 * and the way to serve several new keyframes under HGS_NDT_OMP / HGS_FAST_VGICP, which hgs_loop_match_groups refuses) and under several odometry
 * streams in one process (one pair per sensor and sweep, in lock-step).
 * max_range non-NULL: getFitnessScore(*max_range) runs behind every registration, fitness_score and num_inliers are filled as hgs_loop_match_batch
 * fills them; NULL: no fitness pass, fitness_score is NaN and num_inliers 0 as hgs_align returns them.  out[i].candidate_id = i.
 * Every record is bitwise what a fresh engine with the same parameters returns for hgs_set_target_cloud(targets[i]) +
 * hgs_loop_match_batch({sources[i]}, guess i, max_range): a problem's result depends on its own points only.
 * The handle's own target and source (hgs_set_*) are neither read nor written.  A cloud may appear any number of times in either role — the same
 * pair twice, targets[i] == sources[i]: every problem has its own scratch.
 * n == 0 returns HGS_OK.  HGS_ERR_INVALID_ARGUMENT: a NULL array or entry, a cloud of another handle, n > INT_MAX; nothing has been touched.
 * HGS_ERR_UNSUPPORTED: HGS_FAST_VGICP and the voxel grid of one target exceeds INT_MAX cells (see hgs_align) — the whole call, hgs_last_error names the
 * first pair with that target and the grid; the engine stays usable.  An HGS_NDT_OMP target without a valid cell is no error (as hgs_loop_match_batch).
 * An additive symbol: HGS_ABI_VERSION is unchanged. */
int hgs_align_pairs(hgs_handle* h, hgs_cloud* const* targets /* n */, hgs_cloud* const* sources /* n */,
                    const float* guesses /* 16 * n, column-major */, const double* max_range /* NULL: no fitness pass */, size_t n,
                    hgs_result* out /* n */);
/* Pure host helper: the sequential selection rule above applied to an arbitrary record list (used after the
 * multi-GPU all-gather of per-candidate records). */
int hgs_select_best(const hgs_result* records, size_t n, int32_t* best);

/* ---- the same batch sharded over the GPUs of a node, one process (one engine) per GPU — SURVEY §8e --------------------
 * The caller partitions the n_total candidates of a detection over the ranks any way it likes — typically by a stable keyframe
 * identity (keyframe id mod world), so that a keyframe's resident cloud, index and covariances stay on one GPU across
 * detections; a rank may hold none.  Every rank holds the query keyframe as its target
 * (hgs_set_target*: replicated, rebuilding its 1 MB index per rank is cheaper than broadcasting it), registers ITS candidates
 * and contributes their records to ONE all-gather of fixed-size hgs_result records (RCCL ncclAllGather over xGMI, issued on the
 * engine's stream directly behind the kernels that produced the records: no torch, no host staging); afterwards every rank
 * holds all n_total records in candidate order and applies the sequential rule of loop_detector.hpp:146-153 to them.
 * This replaces the loop of loop_detector.hpp:135-154 on a multi-GPU node.
 *
 * hgs_comm_get_unique_id: rank 0 creates the 128-byte RCCL id and hands it to the other ranks out of band (MPI, a file,
 * torch.distributed.broadcast_object_list — whatever launched the processes).  hgs_comm_init is collective over the ranks. */
#define HGS_COMM_UNIQUE_ID_BYTES 128
int hgs_comm_get_unique_id(void* id_out /* HGS_COMM_UNIQUE_ID_BYTES */);
int hgs_comm_init(hgs_handle* h, int32_t rank, int32_t world, const void* unique_id /* HGS_COMM_UNIQUE_ID_BYTES */);
int hgs_comm_finalize(hgs_handle* h); /* also done by hgs_destroy */
/* candidates / candidate_ids / guesses describe THIS rank's n_mine candidates (candidate_ids[i] in [0, n_total) is the position
 * of candidates[i] in the detection's candidate list); all_out receives n_total records, all_out[c].candidate_id == c;
 * *best as hgs_loop_match_batch.  Collective: every rank of the communicator must call it, with the same n_total.
 * Failure behaviour (a collective must not hang the other SLAM processes): only argument errors a correct caller makes on
 * every rank alike (null all_out, n_total == 0, no hgs_comm_init) return before the exchange.  A rank whose OWN share is
 * unusable (no target, a candidate that is not a cloud of this engine, duplicated clouds, a failed launch) still takes part:
 * it contributes no records, the peers see its candidates as "not converged" (fitness DBL_MAX), and it returns its error
 * AFTER the exchange.  A candidate id reported more than once makes every rank return HGS_ERR_INVALID_ARGUMENT (first report
 * kept).  A C++ exception on a rank where its batch runs is treated like any other failure of its share (padding, error
 * after the exchange); a rank that cannot allocate the exchange buffers, whose collective call fails, or that leaves the
 * region between the two collectives any other way aborts ITS communicator (ncclCommAbort).  RCCL does not promise that a
 * peer's abort ends this rank's own all-gather kernel on the intra-node transports, so no rank ever waits behind a
 * collective with a blocking synchronise: it polls the stream, asks ncclCommGetAsyncError, and after a deadline
 * (environment HGS_COMM_TIMEOUT_MS, default 60000, 0 = none; it has to cover the skew with which the processes enter the
 * detection) aborts its own communicator and returns HGS_ERR_COMM; hgs_comm_init creates a new one.  What has run: the
 * two-rank paths on the emulated communicator of tests/emul; on real RCCL only world size 1.
 * Traffic: one 16-byte header per rank (shard size, status) and max(shard size) record slots per rank. */
int hgs_loop_match_batch_sharded(hgs_handle* h, hgs_cloud* const* candidates, size_t n_mine, const int32_t* candidate_ids,
                                 const float* guesses /* 16*n_mine */, size_t n_total, double max_range, hgs_result* all_out,
                                 int32_t* best);

/* ---- "next" row f1: InformationMatrixCalculator::calc_fitness_score (information_matrix_calculator.cpp:49-80) */
int hgs_calc_fitness_score(hgs_handle* h, hgs_cloud* cloud1, hgs_cloud* cloud2, const float relpose[16], double max_range, double* score);
/* All edges of one graph update in one device batch: flush_keyframe_queue adds up to max_keyframes_per_update odometry edges, each with the NEW keyframe
 * as cloud1 (hdl_graph_slam_nodelet.cpp:235), and the loop step one edge per accepted loop (hdl_graph_slam_nodelet.cpp:569); each calls calc_fitness_score
 * (information_matrix_calculator.cpp:49-80) on clouds too small to fill the device.  scores[i] is bit for bit what
 * hgs_calc_fitness_score(h, cloud1[i], cloud2[i], relposes + 16 i, max_range, .) returns on a fresh engine holding the same clouds, num_inliers[i] the
 * number of points behind that mean (0: the score is DBL_MAX).  A cloud may appear in any number of pairs and in either role (keyframe i is the tree of
 * edge i and the query of edge i + 1); cloud1[i] == cloud2[i] is allowed.  Any hgs_method; the handle's target and source are neither read nor changed.
 * The clouds' missing search indices are built in one pass and the missing seed grids of the cloud1s in two launches; more pairs than one launch holds
 * run in chunks.  n_pairs == 0 returns HGS_OK.  HGS_ERR_INVALID_ARGUMENT, before anything is written or launched: a NULL array while n_pairs > 0, a NULL
 * entry, a cloud of another handle, an orphaned cloud.  An additive symbol: HGS_ABI_VERSION is unchanged. */
int hgs_calc_fitness_score_batch(hgs_handle* h, hgs_cloud* const* cloud1 /* n_pairs: the tree side */, hgs_cloud* const* cloud2 /* n_pairs: the query side */,
                                 const float* relposes /* 16 floats per pair, column-major */, size_t n_pairs, double max_range,
                                 double* scores /* n_pairs */, uint32_t* num_inliers /* n_pairs, NULL ok */);

/* ---- "next" row f2: the prefilter in front of the path (apps/prefiltering_nodelet.cpp:131-182) -------------------- */
enum hgs_downsample_method { HGS_DOWNSAMPLE_NONE = 0, HGS_DOWNSAMPLE_VOXELGRID = 1, HGS_DOWNSAMPLE_APPROX_VOXELGRID = 2 }; /* :51-72; pcl::VoxelGrid / pcl::ApproximateVoxelGrid */
/* Deviation from PCL, stated: HGS_DOWNSAMPLE_APPROX_VOXELGRID drops non-finite input points, pcl::ApproximateVoxelGrid has no
 * finiteness check (a NaN point hashes into some bucket and poisons that voxel's centroid).  With use_distance_filter = 1 (the
 * nodelet's default) the distance filter in front has removed them already and the outputs are identical; they differ only for
 * use_distance_filter = 0 on an is_dense = false cloud, where PCL's output contains NaN centroids. */
enum hgs_outlier_removal { HGS_OUTLIER_NONE = 0, HGS_OUTLIER_STATISTICAL = 1, HGS_OUTLIER_RADIUS = 2 }; /* :73-93 */
typedef struct hgs_prefilter_params {
  int32_t use_distance_filter;     /* use_distance_filter   (true)   :94                                  */
  int32_t downsample_method;       /* downsample_method     (VOXELGRID)                                    */
  double distance_near_thresh;     /* distance_near_thresh  (1.0)    :95                                  */
  double distance_far_thresh;      /* distance_far_thresh   (100.0)  :96                                  */
  double downsample_resolution;    /* downsample_resolution (0.1)    :53                                  */
  int32_t outlier_removal_method;  /* outlier_removal_method (STATISTICAL)                                 */
  int32_t statistical_mean_k;      /* statistical_mean_k    (20)                                           */
  double statistical_stddev;       /* statistical_stddev    (1.0)                                          */
  double radius_radius;            /* radius_radius         (0.8)                                          */
  int32_t radius_min_neighbors;    /* radius_min_neighbors  (2)                                            */
  int32_t reserved;
} hgs_prefilter_params;
int hgs_prefilter_params_default(hgs_prefilter_params* p);
/* distance_filter -> downsample -> outlier_removal of PrefilteringNodelet::cloud_callback (:131-133) on the device.
 * Input: pcl::PointXYZI records (intensity = float 4 of each record when stride >= 20).  The result stays resident as
 * an hgs_cloud that can be handed to hgs_set_source_cloud / hgs_set_target_cloud directly (no second upload) and
 * fetched with hgs_cloud_download. */
int hgs_prefilter(hgs_handle* h, const void* pts, size_t n, size_t stride_bytes, const hgs_prefilter_params* p, hgs_cloud** out);
/* The same with the deskewing step of cloud_callback in front (apps/prefiltering_nodelet.cpp:112, :182-243, rosparam
 * "deskewing"): point i of the n input points is rotated back by the first-order rotation the sensor made during
 * scan_period * i / n at the gyro rate of ONE sensor_msgs/Imu sample — imu_angular_velocity[3] = that message's
 * angular_velocity (the nodelet takes the first queued sample stamped after the cloud, else the newest; choosing it stays
 * host logic).  NULL = the nodelet's empty imu_queue: no deskewing.  scan_period: rosparam "scan_period" (0.1). */
int hgs_prefilter_deskewed(hgs_handle* h, const void* pts, size_t n, size_t stride_bytes, const hgs_prefilter_params* p, const double* imu_angular_velocity,
                           double scan_period, hgs_cloud** out);
/* The same with the rigid transform into base_link_frame between the deskewing and the distance filter (apps/prefiltering_nodelet.cpp:114-129; every
 * launch file sets base_link_frame): deskewing -> transform -> distance_filter -> downsample -> outlier_removal, the order of cloud_callback.
 * sensor_to_base: the float 4x4 matrix handed to pcl::transformPointCloud, column-major (Eigen::Matrix4f::data()); NULL = no base_link_frame: no
 * transform, and the call is hgs_prefilter_deskewed.  Turning the tf::StampedTransform of the lookup (:121-127) into that float matrix stays host code of
 * the caller.  Arithmetic: PCL >= 1.10's, per row x*m(r,0) + (y*m(r,1) + (z*m(r,2) + m(r,3))) in unfused floats, applied to the floats the deskewing
 * produced; a point with a non-finite coordinate passes untouched (PCL's non-dense path), the intensity is carried along.  PCL 1.8 sums in another order
 * (DESIGN.md).  HGS_ERR_INVALID_ARGUMENT for a matrix with a non-finite entry or a bottom row other than 0 0 0 1; the rotation block is not checked for
 * orthogonality (PCL does not check it either). */
int hgs_prefilter_framed(hgs_handle* h, const void* pts, size_t n, size_t stride_bytes, const hgs_prefilter_params* p,
                         const double* imu_angular_velocity /* NULL: no deskewing */, double scan_period,
                         const float sensor_to_base[16] /* column-major, NULL: no transform */, hgs_cloud** out);
/* Several sweeps in one device batch: out[i] is, bit for bit, what hgs_prefilter_framed(sweep i, p) returns — the same count, points, order and
 * intensities; a result depends on its own sweep's points only.  One parameter set for all sweeps (one nodelet configuration); the gyro sample, the scan
 * period and the mount matrix are per sweep, each with hgs_prefilter_framed's meaning.  The S LiDARs of one sweep time, or the next sweeps of a recorded run
 * that is replayed into a map, cost one launch sequence and one read-back instead of S: the sweeps lie concatenated on the device, the voxel grids share
 * one sort (sweep ordinal in the key bits above the voxel index) and one scan per compaction.  Batched this way: downsample NONE or VOXELGRID with every
 * outlier removal — none, RADIUS on the voxel grid (radius_radius / downsample_resolution <= 4), and STATISTICAL (the nodelet's default) or RADIUS on a
 * search tree per sweep: those sweeps' trees come from one index build and their flags from one launch, two read-backs per call whatever S is.  Only
 * APPROX_VOXELGRID and a call with one sweep run the single-sweep sequence per sweep inside the call, with the same results.
 * n_sweeps == 0: HGS_OK.  A sweep with n == 0 yields an empty cloud.  HGS_ERR_INVALID_ARGUMENT, with nothing touched, for a NULL array, for a sweep that
 * hgs_prefilter_framed would refuse (stride, n > 2^30, a non-finite scan period next to a gyro sample, a matrix with a non-finite entry or another bottom
 * row than 0 0 0 1), for more than 2^30 points in total and for more than HGS_PREFILTER_BATCH_MAX_SWEEPS sweeps (the ordinal bits of the sort key).  A
 * sweep whose voxel grid overflows ("too fine for this cloud") fails the WHOLE call with HGS_ERR_INVALID_ARGUMENT: hgs_last_error names the sweep, every
 * out[i] is NULL and nothing is left allocated; the engine stays usable.  Touches neither the handle's target nor its source.
 * An additive symbol and struct: HGS_ABI_VERSION is unchanged. */
#define HGS_PREFILTER_BATCH_MAX_SWEEPS 4096
typedef struct hgs_prefilter_sweep {
  const void* pts;                    /* as hgs_prefilter */
  size_t n;
  size_t stride_bytes;
  const double* imu_angular_velocity; /* [3], NULL: no deskewing of this sweep */
  double scan_period;
  const float* sensor_to_base;        /* column-major 4x4, NULL: no transform for this sweep */
} hgs_prefilter_sweep;
int hgs_prefilter_batch(hgs_handle* h, const hgs_prefilter_sweep* sweeps, size_t n_sweeps, const hgs_prefilter_params* p, hgs_cloud** out /* n_sweeps */);
/* Copy a resident cloud back: out_pts[i] = {x, y, z, (1.0), intensity, ...} with the PointXYZI layout for stride >= 20,
 * packed xyz(+w) otherwise.  Needs room for hgs_cloud_size(c) records. */
int hgs_cloud_download(hgs_cloud* c, void* out_pts, size_t stride_bytes);

/* ---- "next" row f3: MapCloudGenerator::generate (src/hdl_graph_slam/map_cloud_generator.cpp:13-51) ------------------ */
/* Every resident keyframe cloud transformed by its pose (float 4x4, column-major, 16 floats each) and concatenated; with
 * resolution > 0 what pcl::octree::OctreePointCloud(resolution).addPointsFromInputCloud() + getOccupiedVoxelCenters() return
 * (:39-44): the octree's bounding box is replayed in input order (the first finite point on the corner of a 2x2x2 root, every
 * point outside doubling the box towards it), the voxel centres (intensity 0) come in the tree's depth-first order; else the
 * transformed points with their intensity.  The map stays resident (*out); fetch it with hgs_cloud_download.  The octree
 * may be up to 21 levels deep (2^21 voxels per axis: 0.01 m over 20 km); HGS_ERR_INVALID_ARGUMENT beyond that. */
int hgs_map_cloud_generate(hgs_handle* h, hgs_cloud* const* keyframes, const float* poses, size_t n_keyframes, double resolution, hgs_cloud** out);

/* ---- row 12: FloorDetectionNodelet::detect (apps/floor_detection_nodelet.cpp:110-238) ------------------------------------ */
/* Height clip -> normal filter -> RANSAC plane -> acceptance tests, on the device, on a resident cloud (what hgs_prefilter returned goes in without a
 * download: the nodelet subscribes to /filtered_points, :44).  Parameters: the nodelet's rosparams (:57-63) and the constants of :140 / :219 and of
 * pcl::RandomSampleConsensus.
 * Deviations from PCL, stated: the hypothesis sequence is a counter-based generator of ours, a pure function of (seed, i, n_filtered)
 * (PCL draws from a boost::mt19937 shuffle); a degenerate triple counts as an iteration (PCL redraws); plane and distance arithmetic is fp64 (PCL: float);
 * the neighbourhood covariance of the normals is centred fp64 (PCL: a float covariance whose form differs between PCL versions); with tilt_deg != 0 the
 * filtered points keep the input's own bits (PCL rotates there and back in float).  With tilt_deg = 0 the clip is bit-exact PCL.  There is no least-squares
 * refinement of the model (the reference never calls one). */
enum hgs_floor_reason {
  HGS_FLOOR_DETECTED = 0,
  HGS_FLOOR_TOO_FEW_POINTS = 1,  /* n_filtered < floor_pts_thresh (:133); also an empty cloud / nothing inside the clip range */
  HGS_FLOOR_TOO_FEW_INLIERS = 2, /* n_inliers < floor_pts_thresh (:147)                                                    */
  HGS_FLOOR_NOT_VERTICAL = 3     /* |n . r| < cos(floor_normal_thresh) (:152-161)                                          */
};
typedef struct hgs_floor_params {
  double tilt_deg;                  /* tilt_deg              (0.0)   :57                                       */
  double sensor_height;             /* sensor_height         (2.0)   :58                                       */
  double height_clip_range;         /* height_clip_range     (1.0)   :59                                       */
  int32_t floor_pts_thresh;         /* floor_pts_thresh      (512)   :60                                       */
  int32_t use_normal_filtering;     /* use_normal_filtering  (true)  :62                                       */
  double floor_normal_thresh;       /* floor_normal_thresh   (10.0)  :61  [deg]                                */
  double normal_filter_thresh;      /* normal_filter_thresh  (20.0)  :63  [deg]                                */
  int32_t normal_k;                 /* ne.setKSearch         (10)    :219, 3..64                               */
  int32_t ransac_max_iterations;    /* pcl::SampleConsensus max_iterations_ (1000)                             */
  double ransac_distance_threshold; /* ransac.setDistanceThreshold (0.1) :140                                  */
  double ransac_probability;        /* pcl::SampleConsensus probability_    (0.99), inside (0, 1)              */
  uint32_t seed;                    /* of the hypothesis generator (0)                                         */
  int32_t reserved;
} hgs_floor_params;
typedef struct hgs_floor_result {
  float coeffs[4];           /* the floor plane a x + b y + c z + d = 0, normal upward (:164-166); zeros without a model   */
  int32_t detected;          /* 1: boost::optional has a value                                                             */
  int32_t reason;            /* hgs_floor_reason                                                                           */
  uint32_t n_clipped;        /* points inside the height clip                                                              */
  uint32_t n_filtered;       /* ... that also pass the normal filter (== n_clipped without it): the RANSAC input           */
  uint32_t n_inliers;        /* filtered points within the threshold of the model                                          */
  int32_t ransac_iterations; /* hypotheses evaluated                                                                       */
} hgs_floor_result;
int hgs_floor_params_default(hgs_floor_params* p);
/* *filtered_out (NULL ok): the RANSAC input as a resident cloud, what floor_filtered_pub publishes (:127-130) — set whenever the call returns HGS_OK;
 * *inliers_out (NULL ok): the model's inliers in order, what floor_points_pub publishes (:168-177) — set when a floor was detected, else NULL.
 * Both belong to `h` and are the caller's to destroy.  HGS_ERR_INVALID_ARGUMENT: negative thresholds, normal_k outside 3..64, ransac_probability outside
 * (0, 1), non-finite parameters, a cloud of another handle.  The work is accounted under HGS_STAGE_PREFILTER.  With use_normal_filtering a clipped cloud of
 * fewer than three points keeps nothing (pcl::NormalEstimation's normal of fewer than three neighbours is NaN): n_filtered 0, TOO_FEW_POINTS. */
int hgs_detect_floor(hgs_handle* h, hgs_cloud* cloud, const hgs_floor_params* p, hgs_floor_result* out, hgs_cloud** filtered_out, hgs_cloud** inliers_out);
/* hgs_detect_floor of several resident clouds in ONE device batch (the sweeps hgs_prefilter_batch returned, already in base_link; one parameter set: one
 * nodelet configuration).  out[i], filtered_out[i] and inliers_out[i] (either array may be NULL) are byte for byte what hgs_detect_floor(clouds[i]) gives on
 * an engine of its own — ransac_iterations included —, and depend on clouds[i]'s points only; inliers_out[i] is NULL where no floor was detected.  A cloud
 * may appear several times; a cloud of 0 points yields TOO_FEW_POINTS and an empty filtered cloud; n_clouds == 0 is HGS_OK.  The number of blocking
 * read-backs does not grow with n_clouds.  The handle's target and source are neither read nor changed; the work is accounted under
 * HGS_STAGE_PREFILTER.  HGS_ERR_INVALID_ARGUMENT, with nothing launched, `out` untouched and every entry of the two cloud arrays NULL: a NULL `clouds`
 * or `out` with n_clouds > 0, a NULL entry, a cloud of another handle or an orphaned one, invalid parameters (as hgs_detect_floor), more than
 * HGS_FLOOR_BATCH_MAX_CLOUDS clouds, more than 2^30 points in total.  A failure behind that (HIP, allocation) frees every cloud the call created, leaves both
 * arrays all NULL and the engine usable.  Additive: HGS_ABI_VERSION is unchanged. */
#define HGS_FLOOR_BATCH_MAX_CLOUDS 4096
int hgs_detect_floor_batch(hgs_handle* h, hgs_cloud* const* clouds, size_t n_clouds, const hgs_floor_params* p, hgs_floor_result* out /* n_clouds */,
                           hgs_cloud** filtered_out /* n_clouds entries, or NULL */, hgs_cloud** inliers_out /* n_clouds entries, or NULL */);

/* ---- measurement ---------------------------------------------------------------------------------------- */
enum hgs_stage {
  HGS_STAGE_UPLOAD = 0,     /* H2D + pack                                            */
  HGS_STAGE_INDEX = 1,      /* spatial sort + bounding-interval tree build           */
  HGS_STAGE_COVARIANCE = 2, /* kNN covariance pre-pass (GICP/VGICP)                  */
  HGS_STAGE_VOXELIZE = 3,   /* Gaussian voxel table build (NDT / VGICP)              */
  HGS_STAGE_LINEARIZE = 4,  /* correspondence search + J^T M J accumulation (GICP) / NDT derivatives / ICP correspondence pass */
  HGS_STAGE_ERROR = 5,      /* LM trial error evaluation                             */
  HGS_STAGE_SOLVE = 6,      /* 6x6 reductions + solve + LM/Newton update (ICP: Umeyama step) */
  HGS_STAGE_FITNESS = 7,    /* fitness score NN pass                                 */
  HGS_STAGE_PREFILTER = 8,  /* distance filter + voxel grid + outlier removal; map cloud; floor detection */
  HGS_STAGE_COUNT = 9
};
/* Enable/disable hipEvent bracketing of every kernel stage on the handle's stream (adds sync cost when read). */
int hgs_profile_enable(hgs_handle* h, int enabled);
/* Accumulated GPU milliseconds and launch counts per stage since the last reset; arrays of HGS_STAGE_COUNT. */
int hgs_profile_read(hgs_handle* h, double* ms, uint64_t* launches, int reset);
/* Block until everything enqueued on the handle's stream has finished. */
int hgs_synchronize(hgs_handle* h);

/* ---- stage-level hooks (parity tests: one kernel stage at a caller-chosen pose; not used by the adapters) ------ */
/* GICP covariances of the current target, original point order: out6[n][6] = xx,xy,xz,yy,yz,zz (float as stored). */
int hgs_debug_target_covariances(hgs_handle* h, float* out6);
/* One fused correspondence + linearisation pass at pose T (double, row-major 3x4): H[36] row-major, b[6], sum of
 * errors, and per source point (original order) the original target index of its correspondence or -1. */
int hgs_debug_gicp_linearize(hgs_handle* h, const double T12[12], double* H36, double* b6, double* err, int32_t* corr);
/* ICP: one correspondence pass at pose T (double, row-major 3x4) with the engine's max_correspondence_distance and
 * icp_reciprocal: sums17 = [pairs, sum p (3), sum q (3), sum q p^T (9, row-major), sum d2] over the kept pairs (p the moved source
 * point as searched, q its target point), and per source point (original order) the original target index of its pair or -1. */
int hgs_debug_icp_correspond(hgs_handle* h, const double T12[12], double* sums17, int32_t* corr);
/* ICP: one control step (the product kernel k_icp_solve: Umeyama step from the sums, final = Delta * final, DefaultConvergenceCriteria)
 * on caller-made sums of one correspondence pass, with the engine's parameters: the state is (T12_in, mse_prev, iterations_in), sums17 as
 * above.  T12_out (double, row-major 3x4 — not the float of hgs_result), flags3 = {converged, done, iterations}, *mse = the state's mse
 * (DBL_MAX when no step was taken).  Needs a source (the kernel takes its tile count from it: HGS_ERR_NO_SOURCE), no target. */
int hgs_debug_icp_step(hgs_handle* h, const double sums17[17], const double T12_in[12], double mse_prev, int32_t iterations_in,
                       double T12_out[12], int32_t flags3[3] /* converged, done, iterations */, double* mse);
/* Floor detection, the two filters: per point of `cloud` (original order) keep_clip[i] / keep_normal[i] = 1 when it passes the height clip / the clip
 * and the normal filter (without use_normal_filtering: equal to keep_clip), and normals3[3 i ..] its fp64 unit normal (NaN for a point outside the clip
 * or without use_normal_filtering).  Any of the three may be NULL. */
int hgs_debug_floor_filter(hgs_handle* h, hgs_cloud* cloud, const hgs_floor_params* p, uint8_t* keep_clip, uint8_t* keep_normal, double* normals3);
/* Floor detection, the RANSAC counting step (k_floor_ransac_planes + k_floor_ransac_count) with `cloud` taken as the filtered set: counts[j] and
 * coeffs4[4 j ..] (fp64 plane, zeros for a degenerate triple) of hypotheses i0 .. i0 + n - 1 under p->seed and p->ransac_distance_threshold. */
int hgs_debug_floor_ransac_counts(hgs_handle* h, hgs_cloud* cloud, const hgs_floor_params* p, uint32_t i0, uint32_t n, int32_t* counts, double* coeffs4);
/* The engine's last hgs_detect_floor_batch: *clouds = the clouds it took, *ransac_clouds = how many of them entered RANSAC (n_filtered > 0 and >=
 * floor_pts_thresh), *ransac_rounds = the rounds (planes + count + decide) it enqueued, *readbacks = the blocking host read-backs it made (stream
 * synchronisations that wait for device results): one per compaction stage in front of RANSAC, one for the final counts and states, one between two
 * launch groups ("floor_batch_group") — never one per cloud.  Any pointer may be NULL.  An additive debug symbol. */
int hgs_debug_floor_batch_stats(hgs_handle* h, int32_t* clouds, int32_t* ransac_clouds, int32_t* ransac_rounds, int32_t* readbacks);
/* The engine's last hgs_prefilter_batch: *sweeps = the sweeps it took, *batched = 1 when the batch sequence ran, 0 when the sweeps ran one after the
 * other (one sweep, APPROX_VOXELGRID, "prefilter_batch_tree" = 0 under a parameter set that needs a search tree), *readbacks = the blocking host
 * read-backs of device results it made, *index_builds = the search-index builds (one per call in the batch sequence, one per sweep otherwise),
 * *tree_launches = the launches of the batch's tree-walk flag kernels (k_pfb_radius_flags / k_pfb_mean_knn_dist: at most 1).  Any pointer may be NULL.
 * An additive debug symbol. */
int hgs_debug_prefilter_batch_stats(hgs_handle* h, int32_t* sweeps, int32_t* batched, int32_t* readbacks, int32_t* index_builds, int32_t* tree_launches);
/* Valid Gaussian cells of the NDT target (any order): linear key, grid coordinates, mean, inverse covariance, count. */
int hgs_debug_ndt_cells(hgs_handle* h, int32_t cap, int32_t* ijk3, double* mean3, float* icov6, int32_t* npts, int32_t* n_cells);
/* Voxels of the FAST_VGICP target's Gaussian voxel map (any order), built for the engine's resolution and correspondence_randomness if needed:
 * the voxel's integer coordinate floor(p / resolution - 0.5) per axis (decoded from its linear key), the mean of its points (double), the mean
 * of their covariances as stored (float: xx,xy,xz,yy,yz,zz) and the number of points.  *n_cells = voxels in the map; the first min(cap, *n_cells)
 * are written; any of the four arrays may be NULL.  An additive debug symbol: HGS_ABI_VERSION is unchanged (no struct or status code changed). */
int hgs_debug_vgicp_voxels(hgs_handle* h, int32_t cap, int32_t* ijk3, double* mean3, float* cov6, int32_t* npts, int32_t* n_cells);
/* The seed grid of a cloud (the three direct-mapped tables the 1-NN searches without correspondences start from, back to back): *entries = the number of
 * 32-bit words of the grid, 0 when the cloud has none (never the tree side of a fitness pass, seed_grid = 0, invalidated); *bits (NULL ok) = log2 of the
 * finest table's size; the first min(cap, *entries) words go to tab (NULL ok with cap 0).  A seed only bounds a search — a wrong table never changes a
 * score — so the tables of hgs_calc_fitness_score_batch's batched build are tested by reading them.  An additive debug symbol. */
int hgs_debug_cloud_seed_grid(hgs_handle* h, hgs_cloud* cloud, uint32_t* tab, size_t cap, int32_t* bits, size_t* entries);
/* One NDT derivative pass at p =(tx,ty,tz,rx,ry,rz): score, gradient[6], Hessian[36]. */
int hgs_debug_ndt_derivatives(hgs_handle* h, const double p6[6], double* score, double* g6, double* H36);
/* the pure-host merge step of hgs_loop_match_batch_sharded: `gathered` = world blocks of `per` slots, of rank r's block the first
 * counts[r] carry records; fills all_out[0 .. n_total) (a candidate nobody reported: not converged, fitness DBL_MAX);
 * *duplicate_id = an id reported more than once (first report kept) or -1.  Needs no device: callable on a CPU-only box. */
int hgs_debug_merge_shard_records(const hgs_result* gathered, const int32_t* counts, int32_t world, size_t per, size_t n_total,
                                  hgs_result* all_out, int32_t* duplicate_id);
/* The lane plan of the engine's last batch of LM / Newton rounds: *lanes = the streams its problems were spread over, *ahead_lanes = how many of them were
 * highest-priority streams running the ahead group ("lane_order"; 0: contiguous lanes of equal priority), *process_streams = the streams all engines of this
 * process hold on the engine's device right now, which is what the hardware-queue budget (GPU_MAX_HW_QUEUES, default 4) is compared with.  Any pointer may
 * be NULL.  An additive debug symbol. */
int hgs_debug_lane_plan(hgs_handle* h, int32_t* lanes, int32_t* ahead_lanes, int32_t* process_streams);
/* The plan a batch of n_problems problems of tiles_per_problem 256-point tiles each WOULD get on this engine as it is now (its options, the streams it
 * already owns), without running anything: ordered != 0 asks for ordered lanes as a FAST_GICP batch does ("lane_order", 8 problems or more).  assume_streams
 * >= 0 plans against that many streams held by the process on the device instead of the counted ones (the budget arithmetic, testable without other
 * engines); < 0: the counted ones.  Pure host code.  An additive debug symbol. */
int hgs_debug_plan_lanes(hgs_handle* h, int32_t n_problems, int32_t tiles_per_problem, int32_t ordered, int32_t assume_streams, int32_t* lanes, int32_t* ahead_lanes);
/* The order the engine's last hgs_loop_match_batch[_sharded] ran in: *n = its length (0: the caller's order, no ordered lanes), order[i] = the caller's
 * position of the problem that ran i-th, the first min(cap, *n) entries.  The first (*n + 1) / 2 are the ahead group.  An additive debug symbol. */
int hgs_debug_batch_order(hgs_handle* h, int32_t* order, int32_t cap, int32_t* n);
/* A measurement / test knob of one engine: "batch_lanes", "lane_start", "lane_order" (1: a FAST_GICP / FAST_VGICP batch of 8 or more problems that opens
 * several lanes runs the half whose guesses lie farthest from the target on highest-priority streams; records are handed back in the caller's order), "ndt_sort", "cov_split", "resident_descs", "knn_qpw_tiny",
 * "seed_grid", "knn_replay", "ndt_resident", "ndt_chunk", "hilbert_levels", "nn_qpw", "nn_qpw16_below", "nn_qpw32_below", "fused_rounds", "fused_rounds_below", "fused_rounds_max_problems", "fused_rounds_max_blocks", "early_result", "early_run_ahead",
 * "knn_tiny_below", "upload_trace", "prefilter_fast", "prefilter_batch_tree" (0: hgs_prefilter_batch runs the outlier removals that need a search tree sweep after sweep), "floor_chunk" (hypotheses per RANSAC round of hgs_detect_floor, 1..4096), "floor_batch_group" (clouds per RANSAC launch group of
 * hgs_detect_floor_batch, 0 = all that its work buffers allow), "pair_chunk" (pairs per launch of hgs_calc_fitness_score_batch, 0 = 65535).  Results never depend on them (the tests
 * that force a code path check exactly that); A/B runs and those tests are the only callers — the library reads no tuning variable from the environment. */
int hgs_debug_set_option(hgs_handle* h, const char* key, int32_t value);

#ifdef __cplusplus
}
#endif
#endif /* HGS_REGISTRATION_H */
