// hgs_engine.hip — host side of the MI355X scan-matching backend: handle/cloud life cycle, batched
// orchestration of the kernels in hgs_kernels.hip, and the extern "C" boundary declared in
// include/hgs_registration.h (the replacement for the engines that
// hdl_graph_slam::select_registration_method constructs, src/hdl_graph_slam/registrations.cpp:22-124).
//
// Control flow: every registration (odometry: ScanMatchingOdometryNodelet::matching,
// apps/scan_matching_odometry_nodelet.cpp:165-262) is a batch of one; LoopDetector::matching
// (include/hdl_graph_slam/loop_detector.hpp:117-171) is a batch of B candidates.  All B optimisers advance in
// lock-step "rounds" of a fixed kernel sequence; each problem carries its own LM / Newton state machine in
// HBM, so there is no per-iteration host decision — the host only polls a done-counter.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <condition_variable>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <limits>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/hgs_registration.h"
#include "hgs_comm.h"
#include "hgs_consts.h"
#include "hgs_device.h"
#include "hgs_resources.h"
#include "hgs_sort.h"

using namespace hgs;

namespace {

thread_local std::string g_create_error;


int next_pow2(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}
size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

}  // namespace

// A voxel hash table of a cloud in the target role: open addressing over cell keys, the cells' records behind it, all in one block.
struct VoxelTable {
  DeviceBuffer block;
  int* hash_keys = nullptr;
  int* hash_vals = nullptr;
  int2* hash_kv = nullptr;  // {key, value} packed per slot (NDT: k_ndt_pack_hash); null where nothing reads it (VGICP)
  NdtCellRec* cells = nullptr;
  int hash_cap = 0;
};

struct hgs_cloud {
  hgs_handle* owner = nullptr;
  size_t n_input = 0;
  int P = 1;
  DeviceBuffer block;
  CloudDesc desc{};
  CloudDesc* dev_desc = nullptr;  // the descriptor inside the cloud's block (pad = 1, sort_off = 0), written by the kernel that fills raw[]: upload_descs of ONE cloud returns it
  float* intensity = nullptr;  // [n_input] PointXYZI intensity (what hgs_cloud_download / the prefilter hand back)
  bool has_index = false;
  bool corr_stale = false;  // hgs_cloud_invalidate: the correspondence seeds are forgotten when the index is rebuilt (k_gather_sorted)
  bool has_cov = false;
  int cov_k = 0;
  // NDT target tables
  bool has_ndt = false;
  double ndt_resolution = 0;
  int ndt_min_points = 0;
  VoxelTable ndt;
  // VGICP Gaussian voxel map (target role)
  bool has_vg = false;
  double vg_resolution = 0;
  int vg_cov_k = 0;
  long long vg_span[3] = {0, 0, 0};  // cells per axis of the map's bounding box; their product above INT_MAX: no map (ensure_vgicp_target)
  bool vg_too_large = false;
  VoxelTable vg;
  // seed grid (target role of the 1-NN kernels: seed_grid_lookup, hgs_kernels.hip)
  bool has_seed = false;
  DeviceBuffer seed_block;
  int seed_bits = 0;
};

struct ProfEvent {
  int stage;
  hipEvent_t a, b;
};

struct hgs_handle {
  hgs_params prm{};
  int device = 0;
  hipStream_t stream = nullptr;
  // extra streams of a batch (run_batch): the problems are split into lanes whose launch chains are independent, so the
  // block-per-problem solve / decide kernels of one lane run under the point kernels of the others
  hipStream_t lane_stream[7] = {};  // kMaxLanes - 1
  hipEvent_t lane_event[8] = {};
  // Ordered lanes (run_batch, FAST_GICP / FAST_VGICP from 8 problems up, DESIGN.md "Ordered lanes"): the half of a batch whose guesses lie farthest from the
  // target (likely the slowest to converge) runs on highest-priority streams, so that its short late rounds are dispatched ahead of the other half's big
  // grids instead of in lock-step with them.  0: contiguous lanes of equal priority.  "lane_order" (hgs_debug_set_option).  64 x 119 k batch, alternating with
  // the parent library, five runs each: 5907.7 - 5979.7 -> 6149.5 - 6209.7 registrations/s (profiles/lane_order_ab_bench.md)
  int lane_order = 1;
  hipStream_t prio_stream[2] = {};  // created on first use (open_lanes), counted against the queue budget like lane_stream, destroyed with them
  std::vector<int> batch_order;     // internal position -> caller's position of the batch whose records sit in `results`; empty: the caller's order
  int last_lanes = 0, last_ahead_lanes = 0;  // the lane plan of the last batch (hgs_debug_lane_plan)
  int lane_start = 1;                // 1: the host synchronises before it releases the lanes of a batch (open_lanes); HGS_LANE_START=0: not (A/B runs)
  int nn_qpw = 0;  // queries per packet of k_gicp_linearize in the two-launch LM rounds: 0 = by launch size (run_batch), 16 / 32 / 64
  int nn_qpw16_below = 96, nn_qpw32_below = 0;  // ... 16 up to this many 256-point tiles in the launch, 32 up to that many
  // levels of the Hilbert curve the index sort compares (HGS_HILBERT_LEVELS, A/B runs; 16 = all 48 bits, rounds 1-3).  64 x 119 k batch, index stage / step:
  // 16 -> 0.915 / 11.99 ms, 13 -> 0.83 / 11.93, 11 -> 0.75 / 11.91, 10 -> 0.75 / 12.1, 9 -> 0.75 / 12.7 (the walks slow down once a cell of the finest compared
  // level holds many points): 13 = 1/8192 of the cloud's extent (2.4 cm on a 200 m scan), one radix pass less for a batch and two for a pair
  int hilbert_levels = 13;
  hipEvent_t comm_event = nullptr;  // hgs_loop_match_batch_sharded: the gathered headers have reached the host
  // measured on the 16 x 120 k-point loop batch: 1 -> 2 -> 4 lanes = 2850 -> 2935 -> 2975 GICP reg/s, 735 -> 772 -> 797 NDT;
  // 8 lanes: 2440 / 665 (the HIP runtime multiplexes streams onto 4 hardware queues by default).  Round 2, 64 x 119 k-point batch:
  // 1 / 2 / 3 / 4 lanes = 3680 / 3999 / 3937 / 3913 GICP reg/s and 1064 / 1403 / 1384 / 1326 NDT — with 32 problems per lane a lane's
  // launches fill the device on their own and two chains are enough to cover each other's solves and tails.
  int prefilter_fast = 1;  // hgs_prefilter: distance filter inside the voxel grid's kernels, RadiusOutlierRemoval on the voxel grid (0: the separate passes + search tree; A/B, tests)
  int upload_trace = 0;
  int floor_chunk = 64;    // hgs_detect_floor: hypotheses per RANSAC round (planes + count + decide); the result does not depend on it (tests)
  int floor_batch_group = 0;  // hgs_detect_floor_batch: clouds per RANSAC launch group (0: what the work buffers allow); the result does not depend on it (tests)
  int fb_clouds = 0, fb_ransac_clouds = 0, fb_rounds = 0, fb_readbacks = 0;  // the last hgs_detect_floor_batch (hgs_debug_floor_batch_stats)
  int prefilter_batch_tree = 1;  // hgs_prefilter_batch: the outlier removals on a search tree run behind the batched front (0: sweep after sweep, prefilter_each; A/B, tests)
  struct PfBatchStats {
    int sweeps = 0, batched = 0, readbacks = 0, index_builds = 0, tree_launches = 0;
  } pb;  // the last hgs_prefilter_batch (hgs_debug_prefilter_batch_stats)
  int early_run_ahead = 2;  // rounds the host keeps queued in front of a single registration that hands its result over early (the surplus drains behind the caller's back; 3 / 4 measured: no gain for the odometry source, config 2 0.837 -> 0.844 / 0.852 ms back to back: profiles/r06_ab16_early_run_ahead.log)
  int early_result = 1;    // a single registration in two-launch rounds hands its result over in host-mapped memory (run_batch; 0: result kernel + copy + synchronisation)
  PinnedBuffer h_early;                // the host-mapped record
  hipEvent_t early_event = nullptr;    // behind the rounds that were still queued when hgs_align returned early
  bool early_pending = false, early_valid = false;
  int fused_rounds = 1;    // launches of a few GICP problems (below) of at most fused_rounds_below points each: the LM round in two launches (control steps replicated per block; 0: four launches per round)
  int fused_rounds_below = 262144;
  // ... or batches of more problems of at most that many 256-point tiles in total: the loop-closure batch of a KITTI run (candidate keyframes are prefiltered
  // sweeps of 11-14 k points).  Under four lanes: 6 / 12 / 24 candidates x 11 k points 0.62 -> 0.57 / 0.73 -> 0.68 / 0.88 -> 0.83 ms per detection, 48
  // candidates (2160 tiles) 1.07 -> 1.12.  Such batches run on ONE lane now (open_lanes), where the two-launch round is worth less: 6 / 12 candidates
  // 0.521 -> 0.514 / 0.633 -> 0.628 ms, 24 candidates (1080 tiles) 0.794 -> 0.819 — hence 640 (scripts/probes/small_batch_probe.py, profiles/r06_small_batch.log)
  int fused_rounds_max_problems = kFusedRoundMaxProblems, fused_rounds_max_blocks = 640;
  int cov_split = 1;       // non-FROBENIUS regularisations: search kernel + k_cov_regularize (0: one kernel with the eigen-decomposition inline; HGS_COV_SPLIT, A/B runs)
  int resident_descs = 1;  // HGS_RESIDENT_DESCS=0: every stage uploads its descriptor array (A/B runs)
  int knn_qpw_tiny = -1;  // queries per packet of small k_knn_cov launches: -1 = by launch size (queries_per_wave), 0 = 32 as before round 6, 8 / 16 / 24 = below knn_tiny_below queries
  int knn_tiny_below = 32768;
  int seed_grid = 1;    // targets of 1-NN searches get a seed grid (ensure_seed_grid); HGS_SEED_GRID=0 (A/B runs)
  int knn_replay = -1;  // k_knn_cov gather: -1 default (2), 0 tree walk, 1 leaf-log replay, 2 per-lane leaf lists; HGS_KNN_REPLAY (A/B runs, tests)
  int batch_lanes = 0;  // 0: open_lanes chooses (4; NDT_OMP above 32 problems 3; never more than the process's hardware-queue budget has room for); HGS_BATCH_LANES fixes it (A/B runs)
  std::string err;
  hgs_cloud* target = nullptr;
  hgs_cloud* source = nullptr;
  bool own_target = false, own_source = false;
  float final_T[16];

  DeviceBuffer staging, sort_keys[2], sort_vals[2], sort_tmp, descs, states, angles, partials, partials_err, results, guesses, done, misc;
  DeviceBuffer lane_partials[7], lane_partials_err[7];
  DeviceBuffer ndt_accum;  // NdtAccum per problem of the running NDT batch
  DeviceBuffer group_tviews, group_corr;  // hgs_loop_match_groups: one TargetView and one correspondence scratch per problem (run_group_batch)
  DeviceBuffer group_vviews;              // hgs_align_pairs, NDT_OMP / FAST_VGICP: one NdtTargetView per problem (run_pair_batch)
  DeviceBuffer seed_jobs;                 // ensure_seed_grids: one SeedGridJob per cloud of the list
  int pair_chunk = 0;                     // hgs_calc_fitness_score_batch: pairs per launch (0: what grid.y holds, 65535); the results do not depend on it (tests)
  hgs::Comm* comm = nullptr;            // hgs_comm_init: the ranks of a sharded loop-closure batch
  DeviceBuffer comm_send, comm_recv, comm_ids;
  DeviceBuffer pf_ukeys;         // prefilter: the voxels' keys in output order (k_pf_grid_radius_flags)
  DeviceBuffer cov_raw;          // staged fp64 neighbourhood covariances between k_knn_cov<.., 2, ..> and k_cov_regularize
  DeviceBuffer ndt_plan;         // per lane: work queue head + tile prefix sums of the running NDT batch
  // blocks per k_ndt_pass launch (0: by the lane count, below); HGS_NDT_RESIDENT (A/B runs).  Two blocks per CU are resident (the round-4 kernel
  // holds 57 KB of LDS per block).  One lane: 768 — the third block per CU fills the tail (512 / 768 / 1024: 497 / 473 / 452 us per whole-device pass
  // but 1024 loses in the batch).  Several concurrent lanes: 512 per launch — the lanes fill each other's tails, and blocks beyond the resident
  // ones only queue in front of the other lanes' (64-candidate batch, 3 lanes, round 4: 384 / 448 / 512 / 576 / 768 = 2272 / 2284 / 2268 / 2213 /
  // 2162 registrations/s; profiles/r04_ndt_knobs.log)
  int ndt_resident_blocks = 0;
  int ndt_chunk = 0;             // largest queue grab in items (0: the default, 8; 1 = one tile per grab); HGS_NDT_CHUNK (A/B runs)
  int ndt_sort = -1;       // NDT source order: -1 Hilbert order if the source has an index, 1 build the index first, 0 input order (HGS_NDT_SORT, A/B runs)
  DeviceBuffer pf_a, pf_b, pf_keep, pf_slot, pf_small, pf_dist;  // prefilter work space
  DeviceBuffer pf_table;         // hgs_prefilter_batch: the sweep table (PfSweep per sweep)
  PinnedBuffer h_pf_table;       // ... and where its counts and overflow flags are read back to
  PinnedBuffer h_results, h_small, h_flags, h_comm;  // h_flags: host-mapped progress mirror (Progress)
  PinnedRing up;                   // small uploads (descriptors, guesses, plans)
  PinnedRing up_points;            // small point uploads: pinned chunks the host packs into (upload_points_packed)
  PinnedBuffer up_big;             // large point uploads: one pinned image of the packed cloud, filled by the pack pool
  hipEvent_t up_big_event = nullptr;  // the last DMA out of up_big
  bool up_big_pending = false;
  PackPool pack_pool;
  PinnedBuffer h_xform;            // hgs_transform_source: the aligned cloud on its way down

  // freed cloud blocks kept for reuse: the odometry path creates and destroys one cloud per sweep, and hipMalloc /
  // hipFree (which synchronises the device) cost more than the upload itself
  std::vector<DeviceBuffer> block_pool;
  // every cloud this engine has created and not yet destroyed: hgs_destroy orphans them (frees their device memory, clears
  // `owner`) so that a later hgs_cloud_destroy / hgs_cloud_download on a cached pointer is safe instead of a use-after-free
  std::vector<hgs_cloud*> live_clouds;
  // One call at a time per engine: a handle is meant to be driven by one thread (like the pcl::Registration object it replaces), but a
  // garbage-collected wrapper may destroy a cloud from another thread while a long call is running on this engine's stream and
  // buffers — entry points that touch the engine take this lock (different engines never contend).
  std::recursive_mutex api_mutex;

  bool profiling = false;
  std::vector<ProfEvent> prof_events;
  std::vector<ProfEvent> prof_free;
  double prof_ms[HGS_STAGE_COUNT];
  uint64_t prof_launches[HGS_STAGE_COUNT];

  hgs_handle() = default;
  hgs_handle(const hgs_handle&) = delete;
  hgs_handle& operator=(const hgs_handle&) = delete;
  void synchronize_streams() {
    if (stream) (void)hipStreamSynchronize(stream);
    for (hipStream_t ls : lane_stream)
      if (ls) (void)hipStreamSynchronize(ls);
    for (hipStream_t ls : prio_stream)
      if (ls) (void)hipStreamSynchronize(ls);
  }
  ~hgs_handle();
};

namespace {

#define HGS_HIP(h, call)                                                                                           \
  do {                                                                                                             \
    hipError_t e__ = (call);                                                                                       \
    if (e__ != hipSuccess) {                                                                                       \
      char buf__[512];                                                                                             \
      snprintf(buf__, sizeof(buf__), "%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__, __LINE__);  \
      (h)->err = buf__;                                                                                            \
      return HGS_ERR_HIP;                                                                                          \
    }                                                                                                              \
  } while (0)

#define HGS_TRY(expr)             \
  do {                            \
    int rc__ = (expr);            \
    if (rc__ != HGS_OK) return rc__; \
  } while (0)

struct StageTimer {
  hgs_handle* h;
  ProfEvent ev{};
  bool active = false;
  StageTimer(hgs_handle* h_, int stage) : h(h_) {
    if (!h->profiling) return;
    if (!h->prof_free.empty()) {
      ev = h->prof_free.back();
      h->prof_free.pop_back();
    } else {
      if (hipEventCreate(&ev.a) != hipSuccess || hipEventCreate(&ev.b) != hipSuccess) return;
    }
    ev.stage = stage;
    active = hipEventRecord(ev.a, h->stream) == hipSuccess;
  }
  ~StageTimer() {
    if (!active) return;
    (void)hipEventRecord(ev.b, h->stream);
    h->prof_events.push_back(ev);
  }
};

// One call at a time per engine (hgs_handle::api_mutex): what every locking entry point opens with.  A null engine, and a cloud that is null or has
// outlived its engine, lock nothing — the entry point rejects them (or frees the orphan) right behind this.
struct ApiLock {
  std::unique_lock<std::recursive_mutex> lk;
  explicit ApiLock(hgs_handle* h) {
    if (h) lk = std::unique_lock<std::recursive_mutex>(h->api_mutex);
  }
  explicit ApiLock(hgs_cloud* c) : ApiLock(c ? c->owner : nullptr) {}
};

int set_device(hgs_handle* h) {
  HGS_HIP(h, hipSetDevice(h->device));
  return HGS_OK;
}

// ---- point upload --------------------------------------------------------------------------------------------
// Host -> device of n strided point records (pcl::PointXYZI: 32 bytes; anything with x, y, z at floats 0..2 and, from 20 bytes on, the intensity
// at float 4) as packed 16-byte records {x, y, z, intensity} in h->staging.  The HOST packs chunk after chunk into pinned buffers (half the bytes
// of a PointXYZI go over PCIe, none of them through the runtime's pageable staging path) and every chunk's DMA runs while the next chunk is packed.
// Round 4 handed the caller's pageable buffer to hipMemcpyAsync and synchronised behind the kernels that followed (profiles/r05_upload.md).
// The caller's buffer has been read completely when this returns; the device side is ordered on h->stream.
constexpr size_t kUploadChunkPoints = 16384;     // 256 KB per pinned chunk
#ifndef HGS_UPLOAD_PARALLEL_POINTS
#define HGS_UPLOAD_PARALLEL_POINTS 49152  // (A/B knob: a huge value keeps every upload on the calling thread)
#endif
constexpr size_t kUploadParallelPoints = HGS_UPLOAD_PARALLEL_POINTS;  // from three chunks on the pack pool helps (below: one thread, the ring of pinned chunks)
// The pinned image of the large uploads: opened (the previous upload's DMA has left it, room for `records`) in front of the packing, closed (event behind
// the last DMA) after it.  A single upload opens and closes it around its own records; hgs_prefilter_batch opens it once for the concatenated image of all
// its sweeps, so that a sweep's packing does not wait for the DMA of the sweep in front.
int upload_image_open(hgs_handle* h, size_t records) {
  if (h->up_big_pending) {
    HGS_HIP(h, hipEventSynchronize(h->up_big_event));  // the previous upload's DMA has left the pinned image (it finished long ago)
    h->up_big_pending = false;
  }
  HGS_HIP(h, h->up_big.reserve(records * sizeof(float4)));
  return HGS_OK;
}
int upload_image_close(hgs_handle* h) {
  if (!h->up_big_event) HGS_HIP(h, hipEventCreateWithFlags(&h->up_big_event, hipEventDisableTiming));
  HGS_HIP(h, hipEventRecord(h->up_big_event, h->stream));
  h->up_big_pending = true;
  return HGS_OK;
}
// n records to h->staging[off ..) (reserved by the caller).  in_image: the caller has opened the pinned image for a concatenated upload that holds these
// records at `off` and closes it behind the last one.
int upload_points_at(hgs_handle* h, const void* pts, size_t n, size_t stride_bytes, size_t off, bool in_image) {
  const bool has_intensity = stride_bytes >= 20;
  const char* src = static_cast<const char*>(pts);
  float4* const dev = h->staging.as<float4>() + off;
  if (n >= kUploadParallelPoints) {
    // large cloud: kWorkers + this thread pack chunks into ONE pinned image; this thread sends chunk c down as soon as it is ready (in order)
    if (!in_image) HGS_TRY(upload_image_open(h, n));
    float4* const image = h->up_big.as<float4>() + (in_image ? off : 0);
    const size_t nchunks = (n + kUploadChunkPoints - 1) / kUploadChunkPoints;
    std::vector<std::atomic<unsigned char>> ready(nchunks);
    for (auto& r : ready) r.store(0, std::memory_order_relaxed);
    PackPool::Job job;
    job.src = src, job.dst = reinterpret_cast<float*>(image), job.n = n, job.stride = stride_bytes, job.chunk = kUploadChunkPoints, job.nchunks = nchunks;
    job.has_intensity = has_intensity, job.ready = ready.data();
    h->pack_pool.post(&job);
    hipError_t err = hipSuccess;
    for (size_t c = 0; c < nchunks; c++) {
      while (!ready[c].load(std::memory_order_acquire))
        if (!PackPool::help(job)) std::this_thread::yield();
      const size_t i0 = c * kUploadChunkPoints, m = std::min(kUploadChunkPoints, n - i0);
      if (err == hipSuccess) err = hipMemcpyAsync(dev + i0, image + i0, m * sizeof(float4), hipMemcpyHostToDevice, h->stream);
    }
    h->pack_pool.retire();  // (`job` and `ready` live on this stack frame)
    HGS_HIP(h, err);
    if (!in_image) HGS_TRY(upload_image_close(h));
    return HGS_OK;
  }
  for (size_t i0 = 0; i0 < n; i0 += kUploadChunkPoints) {
    const size_t m = std::min(kUploadChunkPoints, n - i0);
    void* staged = nullptr;
    int slot = 0;
    HGS_HIP(h, h->up_points.stage(kUploadChunkPoints * sizeof(float4), &staged, &slot));
    float* dst = static_cast<float*>(staged);
    const char* s0 = src + i0 * stride_bytes;
    if (has_intensity) {
      for (size_t i = 0; i < m; i++) {
        const float* f = reinterpret_cast<const float*>(s0 + i * stride_bytes);
        dst[4 * i] = f[0], dst[4 * i + 1] = f[1], dst[4 * i + 2] = f[2], dst[4 * i + 3] = f[4];
      }
    } else {
      for (size_t i = 0; i < m; i++) {
        const float* f = reinterpret_cast<const float*>(s0 + i * stride_bytes);
        dst[4 * i] = f[0], dst[4 * i + 1] = f[1], dst[4 * i + 2] = f[2], dst[4 * i + 3] = 0.f;
      }
    }
    HGS_HIP(h, hipMemcpyAsync(dev + i0, staged, m * sizeof(float4), hipMemcpyHostToDevice, h->stream));
    HGS_HIP(h, h->up_points.commit(slot, h->stream));
  }
  return HGS_OK;
}
int upload_points_packed(hgs_handle* h, const void* pts, size_t n, size_t stride_bytes, const float4** dev) {
  HGS_HIP(h, h->staging.reserve(std::max<size_t>(n, 1) * sizeof(float4)));
  *dev = h->staging.as<float4>();
  return upload_points_at(h, pts, n, stride_bytes, 0, false);
}

// ---- cloud allocation --------------------------------------------------------------------------------------
int cloud_alloc(hgs_handle* h, size_t n, hgs_cloud** out) {
  hgs_cloud* c = new hgs_cloud();
  c->owner = h;
  c->n_input = n;
  c->P = next_pow2((int)((n + kLeaf - 1) / kLeaf));
  if (c->P < 1) c->P = 1;
  const size_t slots = (size_t)c->P * kLeaf;
  // the per-input-point arrays are sized for n rounded up to 8192 points: consecutive sweeps of one sensor differ by a few hundred returns, and a
  // block that is a few bytes too small for the next sweep cannot be reused from the pool — the odometry path then paid a hipMalloc and (pool full)
  // a hipFree, which synchronises the device, on most sweeps: 0.3-0.4 ms of a 0.7 ms raw-sweep step (profiles/r05_upload.md)
  const size_t n_cap = align_up(std::max<size_t>(n, 1), 8192);
  size_t off = 0;
  const size_t o_meta = off;
  off = align_up(off + sizeof(CloudMeta), 256);
  const size_t o_desc = off;
  off = align_up(off + sizeof(CloudDesc), 256);
  const size_t o_raw = off;
  off = align_up(off + n_cap * sizeof(float4), 256);
  const size_t o_pts = off;
  off = align_up(off + slots * sizeof(float4), 256);
  const size_t o_lpts = off;
  off = align_up(off + slots * sizeof(float4), 256);
  const size_t o_nodes = off;
  off = align_up(off + ((size_t)4 * c->P + 32) * sizeof(float4), 256);  // + four 128-byte groups: the 4-ary walks read whole groups, the quad walk four at a time
  const size_t o_cov = off;
  off = align_up(off + 2 * slots * sizeof(float4), 256);
  const size_t o_corr = off;
  off = align_up(off + slots * sizeof(int), 256);
  const size_t o_int = off;
  off = align_up(off + n_cap * sizeof(float), 256);
  hipError_t e = hipSuccess;
  for (size_t k = 0; k < h->block_pool.size(); k++) {
    if (h->block_pool[k].cap >= off && h->block_pool[k].cap <= 2 * off + (1u << 20)) {
      c->block = std::move(h->block_pool[k]);
      h->block_pool.erase(h->block_pool.begin() + k);
      break;
    }
  }
  if (!c->block.p) e = c->block.alloc(off);
  if (e != hipSuccess) {
    h->err = std::string("hipMalloc(cloud) failed: ") + hipGetErrorString(e);
    delete c;
    return HGS_ERR_HIP;
  }
  char* base = c->block.as<char>();
  c->desc.meta = (CloudMeta*)(base + o_meta);
  c->dev_desc = (CloudDesc*)(base + o_desc);
  c->desc.raw = (const float4*)(base + o_raw);
  c->desc.pts = (float4*)(base + o_pts);
  c->desc.lpts = (float4*)(base + o_lpts);
  c->desc.nodes = (float4*)(base + o_nodes);
  c->desc.cov = (float4*)(base + o_cov);
  c->desc.corr = (int*)(base + o_corr);
  c->intensity = (float*)(base + o_int);
  c->desc.n_input = (int)n;
  c->desc.P = c->P;
  c->desc.sort_off = 0;
  c->desc.pad = 0;
  c->corr_stale = true;  // no correspondences yet: k_gather_sorted writes -1 when the index is built (every reader of corr has built it first)
  h->live_clouds.push_back(c);
  *out = c;
  return HGS_OK;
}

// Releases the device memory of a cloud (the struct itself stays): what hgs_destroy does to clouds that outlive their engine.
void cloud_release_device(hgs_cloud* c, bool pool) {
  // stream order makes reuse safe: every kernel that touches the block was enqueued on the owner's stream
  hgs_handle* h = c->owner;
  if (c->block.p && pool && h && h->block_pool.size() < 6) h->block_pool.push_back(std::move(c->block));
  c->block.release(), c->ndt.block.release(), c->vg.block.release(), c->seed_block.release();
  c->has_index = c->has_cov = c->has_ndt = c->has_vg = c->has_seed = false;
}

void cloud_free(hgs_cloud* c) {
  if (!c) return;
  cloud_release_device(c, true);
  if (hgs_handle* h = c->owner) {
    auto it = std::find(h->live_clouds.begin(), h->live_clouds.end(), c);
    if (it != h->live_clouds.end()) h->live_clouds.erase(it);
  }
  delete c;
}

// Upload descriptors of a set of clouds (with their sort offsets) into h->descs; returns device pointer.
// what a cloud's resident descriptor holds: pad = 1 (an index build always follows a creation or an invalidation, both of which ask for corr[] to be
// cleared; nothing else reads pad), sort_off = 0 (a cloud alone in a batch sort)
CloudDesc resident_desc(const hgs_cloud* c) {
  CloudDesc d = c->desc;
  d.sort_off = 0, d.pad = 1;
  return d;
}

// corr_of: a correspondence scratch per entry instead of the clouds' own (run_group_batch: one cloud may be the source of several problems of a batch)
int upload_descs(hgs_handle* h, const std::vector<hgs_cloud*>& clouds, bool with_sort_offsets, const CloudDesc** dev, size_t* total_n, int* const* corr_of = nullptr) {
  const size_t B = clouds.size();
  if (B == 1 && clouds[0]->dev_desc && h->resident_descs && !corr_of) {  // one cloud: its resident descriptor, no copy
    if (total_n) *total_n = clouds[0]->n_input;
    *dev = clouds[0]->dev_desc;
    return HGS_OK;
  }
  HGS_HIP(h, h->descs.reserve(B * sizeof(CloudDesc)));
  void* staged = nullptr;
  int slot = 0;
  HGS_HIP(h, h->up.stage(B * sizeof(CloudDesc), &staged, &slot));
  CloudDesc* hd = static_cast<CloudDesc*>(staged);
  size_t off = 0;
  for (size_t i = 0; i < B; i++) {
    hd[i] = clouds[i]->desc;
    hd[i].sort_off = with_sort_offsets ? (int)off : 0;
    if (corr_of) hd[i].corr = corr_of[i];
    off += clouds[i]->n_input;
  }
  if (total_n) *total_n = off;
  HGS_HIP(h, hipMemcpyAsync(h->descs.p, hd, B * sizeof(CloudDesc), hipMemcpyHostToDevice, h->stream));
  HGS_HIP(h, h->up.commit(slot, h->stream));
  *dev = h->descs.as<CloudDesc>();
  return HGS_OK;
}

// Queries per wave of the kNN covariance kernel.  A launch with few queries cannot fill 1024 SIMDs with 64-query packets
// (one 120 k-point cloud is 1.8 waves per SIMD) and is bound by the dependent-load chain of a single walk; 32-query
// packets walk fewer nodes and put more waves in flight (0.91 -> 0.66 ms for one 120 k-point cloud).  Large batches keep
// 64 (least total work); the 1-NN kernels always do (no measurable gain from shorter packets there).
// Round 6, second visit to the question: a launch of a few packets per SIMD lasts as long as its SLOWEST packet, and those are the packets over sparse far
// returns at ~4x the median's leaves (scripts/probes/knn_probe.py, profiles/r06_knn_probe_before.log).  Shorter packets split them — behind a full pre-fill
// window (k_knn_cov<.., WINDOW>: the first attempt, 16 own points in front of unfilled lists, measured equal).  Same-box (profiles/r06_ab8_knn_short_packets.log):
// the odometry source behind the KITTI prefilter (13.5 k points) hgs_align 0.390 -> 0.355 ms with 8-query packets (16: 0.361); one raw HDL-32E source (65 k)
// 0.843 -> 0.787 ms with 16 (8: 0.808, 24: 0.795); the HDL-32E PAIR in one launch (131 k queries) loses with every short packet (covariance stage 0.234 -> 0.27-0.39 ms).
// `tiny`: -1 = these tiers, 0 = none (32 as before), 8 / 16 / 24 = that packet below `tiny_below` queries (A/B runs, tests).
int queries_per_wave(size_t total_queries, int small, int tiny = 0, size_t tiny_below = 0) {
  if (tiny < 0) {
    if (total_queries < (size_t)32768) return 8;
    if (total_queries < (size_t)100000) return 16;
  } else if (tiny > 0 && total_queries < tiny_below) {
    return tiny;
  }
  return total_queries >= (size_t)600000 ? 64 : small;
}

// ---- rocPRIM on the engine's stream: size query, work space in sort_tmp, the call ----------------------------
int scan_u32(hgs_handle* h, const uint32_t* in, uint32_t* out, size_t n) {
  size_t tmp = 0;
  if (hgs_exclusive_scan_u32(nullptr, &tmp, in, out, n, h->stream) != 0) {
    h->err = "rocprim exclusive_scan (size query) failed";
    return HGS_ERR_HIP;
  }
  HGS_HIP(h, h->sort_tmp.reserve(tmp));
  if (hgs_exclusive_scan_u32(h->sort_tmp.p, &tmp, in, out, n, h->stream) != 0) {
    h->err = "rocprim exclusive_scan failed";
    return HGS_ERR_HIP;
  }
  return HGS_OK;
}

// room for n key / value pairs in both halves of the sort's double buffer
int reserve_sort_pairs(hgs_handle* h, size_t n) {
  for (int i = 0; i < 2; i++) {
    HGS_HIP(h, h->sort_keys[i].reserve(n * sizeof(uint64_t)));
    HGS_HIP(h, h->sort_vals[i].reserve(n * sizeof(uint32_t)));
  }
  return HGS_OK;
}

// stable radix sort of sort_keys[0] / sort_vals[0] into sort_keys[1] / sort_vals[1] by key bits [begin_bit, end_bit)
int sort_pairs(hgs_handle* h, size_t n, int begin_bit, int end_bit) {
  auto sort = [&](void* tmp, size_t* tmp_bytes) {
    return hgs_sort_pairs_u64_u32(tmp, tmp_bytes, h->sort_keys[0].as<uint64_t>(), h->sort_keys[1].as<uint64_t>(), h->sort_vals[0].as<uint32_t>(),
                                  h->sort_vals[1].as<uint32_t>(), n, begin_bit, end_bit, h->stream);
  };
  size_t tmp_bytes = 0;
  if (sort(nullptr, &tmp_bytes) != 0) {
    h->err = "rocprim radix_sort_pairs (size query) failed";
    return HGS_ERR_HIP;
  }
  HGS_HIP(h, h->sort_tmp.reserve(tmp_bytes));
  if (sort(h->sort_tmp.p, &tmp_bytes) != 0) {
    h->err = "rocprim radix_sort_pairs failed";
    return HGS_ERR_HIP;
  }
  return HGS_OK;
}

// Build the search index (Hilbert sort + implicit tree) of every cloud in the list that lacks one — one
// batched kernel sequence and ONE radix sort for the whole list.
int ensure_index(hgs_handle* h, const std::vector<hgs_cloud*>& all) {
  std::vector<hgs_cloud*> todo;
  for (hgs_cloud* c : all)
    if (!c->has_index && std::find(todo.begin(), todo.end(), c) == todo.end()) todo.push_back(c);
  if (todo.empty()) return HGS_OK;
  // the key carries the cloud ordinal in bits 48.. ; process in chunks of at most 65536 clouds
  for (size_t start = 0; start < todo.size(); start += 65536) {
    std::vector<hgs_cloud*> chunk(todo.begin() + start, todo.begin() + std::min(todo.size(), start + 65536));
    StageTimer tm(h, HGS_STAGE_INDEX);
    const CloudDesc* d_descs = nullptr;
    size_t total = 0;
    for (hgs_cloud* c : chunk) c->desc.pad = c->corr_stale ? 1 : 0;  // read by k_gather_sorted
    HGS_TRY(upload_descs(h, chunk, true, &d_descs, &total));
    for (hgs_cloud* c : chunk) c->desc.pad = 0;  // (corr_stale is cleared where has_index is set: a failure below must not lose the invalidate request)
    int max_n = 0, max_P = 1;
    for (hgs_cloud* c : chunk) max_n = std::max(max_n, (int)c->n_input), max_P = std::max(max_P, c->P);
    const int nc = (int)chunk.size();
    // meta (nvalid, bbox) was filled at upload time
    if (total > 0) {
      HGS_TRY(reserve_sort_pairs(h, total));
      // The sort compares the top `hilbert_levels` levels of the curve (3 bits each) + the cloud ordinal: points that share a cell of the finest
      // compared level stay in input order (stable sort), i.e. in firing order — still neighbours.  Fewer compared bits = fewer radix passes.
      const int drop_bits = 3 * (16 - h->hilbert_levels);
      launch_hilbert_keys(h->stream, d_descs, nc, max_n, h->sort_keys[0].as<unsigned long long>(), h->sort_vals[0].as<unsigned>(), drop_bits);
      int bits = 48;
      for (int v = nc - 1; v > 0; v >>= 1) bits++;
      HGS_TRY(sort_pairs(h, total, drop_bits, bits));
    }
    launch_gather_sorted(h->stream, d_descs, nc, max_P * kLeaf, h->sort_vals[1].as<unsigned>());
    launch_build_tree(h->stream, d_descs, nc, max_P);
    HGS_HIP(h, hipGetLastError());
    // (the device-side descs buffer is reused by later stages in stream order; the pinned staging slot is guarded by its event, PinnedRing)
    for (hgs_cloud* c : chunk) c->has_index = true, c->corr_stale = false;
  }
  return HGS_OK;
}

// what a cloud's cached covariances depend on besides its points
int cov_cache_key(const hgs_handle* h, int k) { return k | (h->prm.regularization_method << 16); }

int ensure_cov(hgs_handle* h, const std::vector<hgs_cloud*>& all, int k) {
  HGS_TRY(ensure_index(h, all));
  const int key = cov_cache_key(h, k);
  std::vector<hgs_cloud*> todo;
  for (hgs_cloud* c : all)
    if ((!c->has_cov || c->cov_k != key) && std::find(todo.begin(), todo.end(), c) == todo.end()) todo.push_back(c);
  if (todo.empty()) return HGS_OK;
  StageTimer tm(h, HGS_STAGE_COVARIANCE);
  const CloudDesc* d_descs = nullptr;
  HGS_TRY(upload_descs(h, todo, false, &d_descs, nullptr));
  int max_n = 0;
  for (hgs_cloud* c : todo) max_n = std::max(max_n, (int)c->n_input);
  size_t total_q = 0;
  for (hgs_cloud* c : todo) total_q += c->n_input;
  int qpw = queries_per_wave(total_q, 32, h->knn_qpw_tiny, (size_t)h->knn_tiny_below);  // (32: >= k points in the pre-fill window; shorter packets borrow a window)
  // the leaf-log gather pays for batches of LiDAR keyframes, not for one or two (dense) clouds: see launch_knn_cov
  // pass 2 of k_knn_cov: per-lane leaf lists (mode 2; measured against the leaf-log replay and the second tree walk: 64 LiDAR clouds
  // 4.25 -> 4.0 ms, dense 1 M-point pair 1.46 -> 1.27 ms, one HDL-32E pair unchanged); HGS_KNN_REPLAY=0|1|2 forces a mode (tests, A/B)
  const int gather = h->knn_replay >= 0 ? h->knn_replay : 2;
  if (qpw < 32 && (gather != 2 || k > 20)) qpw = 32;  // (the short-packet instantiation exists for the per-lane lists and k <= 20: launch_knn_cov)
  double* raw_stage = nullptr;
  if (h->prm.regularization_method != 0 && h->cov_split) {  // PLANE / MIN_EIG / ...: the eigen-decompositions in a kernel of their own (k_cov_regularize)
    HGS_HIP(h, h->cov_raw.reserve(todo.size() * (size_t)std::max(max_n, 1) * 6 * sizeof(double)));
    raw_stage = h->cov_raw.as<double>();
  }
  launch_knn_cov(h->stream, d_descs, (int)todo.size(), max_n, k, qpw, h->prm.regularization_method, gather, raw_stage);
  HGS_HIP(h, hipGetLastError());
  for (hgs_cloud* c : todo) c->has_cov = true, c->cov_k = key;
  return HGS_OK;
}

// The voxel table of `c` for `cap` hash slots and up to `max_cells` cells, built from sorted cell keys: (re)allocated when the capacity changed, its keys
// cleared; `grid_params`, `cell_keys(keys, vals)` and `build_cells(sorted keys, sorted vals)` are the method's own launches, in that order around the sort.
template <typename P, typename K, typename C>
int build_voxel_table(hgs_handle* h, const hgs_cloud* c, VoxelTable& t, int cap, int max_cells, bool packed, P&& grid_params, K&& cell_keys, C&& build_cells) {
  const size_t n = c->n_input;
  if (!t.block.p || t.hash_cap != cap) {
    const size_t o_keys = 0, o_vals = align_up((size_t)cap * 4, 256), o_kv = o_vals + align_up((size_t)cap * 4, 256);
    const size_t o_cells = o_kv + (packed ? align_up((size_t)cap * 8, 256) : 0);
    HGS_HIP(h, t.block.alloc(o_cells + (size_t)max_cells * sizeof(NdtCellRec)));
    char* base = t.block.as<char>();
    t.hash_keys = (int*)(base + o_keys);
    t.hash_vals = (int*)(base + o_vals);
    t.hash_kv = packed ? (int2*)(base + o_kv) : nullptr;
    t.cells = (NdtCellRec*)(base + o_cells);
    t.hash_cap = cap;
  }
  HGS_HIP(h, hipMemsetAsync(t.hash_keys, 0xff, (size_t)cap * 4, h->stream));
  grid_params();
  if (n > 0) {
    HGS_TRY(reserve_sort_pairs(h, n));
    cell_keys(h->sort_keys[0].as<unsigned long long>(), h->sort_vals[0].as<unsigned>());
    HGS_TRY(sort_pairs(h, n, 0, 32));
    build_cells(h->sort_keys[1].as<unsigned long long>(), h->sort_vals[1].as<unsigned>());
  }
  return HGS_OK;
}

int ensure_ndt_target(hgs_handle* h, hgs_cloud* c) {
  const double res = h->prm.resolution;
  const int min_pts = h->prm.ndt_min_points_per_voxel;
  if (c->has_ndt && c->ndt_resolution == res && c->ndt_min_points == min_pts) return HGS_OK;
  StageTimer tm(h, HGS_STAGE_VOXELIZE);
  const int max_cells = (int)(c->n_input / (size_t)std::max(1, min_pts)) + 1;
  const int cap = next_pow2(std::max(64, 4 * max_cells));
  const float inv_leaf = 1.0f / (float)res;
  VoxelTable& t = c->ndt;
  HGS_TRY(build_voxel_table(
      h, c, t, cap, max_cells, true, [&] { launch_ndt_grid_params(h->stream, c->desc, inv_leaf); },
      [&](unsigned long long* keys, unsigned* vals) { launch_ndt_cell_keys(h->stream, c->desc, inv_leaf, keys, vals); },
      [&](unsigned long long* keys, unsigned* vals) { launch_ndt_build_cells(h->stream, c->desc, keys, vals, min_pts, t.hash_keys, t.hash_vals, cap - 1, t.cells); }));
  launch_ndt_pack_hash(h->stream, t.hash_keys, t.hash_vals, t.hash_kv, cap);
  HGS_HIP(h, hipGetLastError());
  c->has_ndt = true;
  c->ndt_resolution = res;
  c->ndt_min_points = min_pts;
  return HGS_OK;
}

// A target whose voxel bounding box holds more cells than a 32-bit linear key addresses has no map (k_vgicp_grid_params raised vg_error and every
// key is the sentinel): registering against it would "converge" at the guess without a single correspondence, so the entry points refuse it.
int vgicp_grid_too_large(hgs_handle* h, const hgs_cloud* c) {
  char msg[256];
  snprintf(msg, sizeof(msg),
           "FAST_VGICP: the target's voxel grid spans %lld x %lld x %lld cells at resolution %g, more than the 2147483647 a linear voxel key addresses "
           "(a far stray point in the target?)",
           c->vg_span[0], c->vg_span[1], c->vg_span[2], c->vg_resolution);
  h->err = msg;
  return HGS_ERR_UNSUPPORTED;
}

// FastVGICP's GaussianVoxelMap of the target (needs the target's kNN covariances first).  Upstream rebuilds it at
// the start of every align(); the result only depends on (target, resolution, k), so it is cached on the cloud — and with it whether the grid
// was too large: the flag comes back once per build (one small copy and the wait for it, like the prefilter's), never per align.
int ensure_vgicp_target(hgs_handle* h, hgs_cloud* c) {
  const double res = h->prm.resolution;
  const int k = h->prm.correspondence_randomness;
  if (c->has_vg && c->vg_resolution == res && c->vg_cov_k == cov_cache_key(h, k)) return c->vg_too_large ? vgicp_grid_too_large(h, c) : HGS_OK;
  StageTimer tm(h, HGS_STAGE_VOXELIZE);
  const int max_cells = (int)c->n_input + 1;
  const int cap = next_pow2(std::max<int>(64, 2 * max_cells));
  VoxelTable& t = c->vg;
  HGS_TRY(build_voxel_table(
      h, c, t, cap, max_cells, false, [&] { launch_vgicp_grid_params(h->stream, c->desc, res); },
      [&](unsigned long long* keys, unsigned* vals) { launch_vgicp_cell_keys(h->stream, c->desc, res, keys, vals); },
      [&](unsigned long long* keys, unsigned* vals) { launch_vgicp_build_cells(h->stream, c->desc, keys, vals, t.hash_keys, t.hash_vals, cap - 1, t.cells); }));
  HGS_HIP(h, hipGetLastError());
  HGS_HIP(h, h->h_small.reserve(sizeof(CloudMeta)));
  const CloudMeta* hm = h->h_small.as<CloudMeta>();
  HGS_HIP(h, hipMemcpyAsync(h->h_small.p, c->desc.meta, sizeof(CloudMeta), hipMemcpyDeviceToHost, h->stream));
  HGS_HIP(h, hipStreamSynchronize(h->stream));
  for (int d = 0; d < 3; d++) c->vg_span[d] = (long long)hm->vg_max_b[d] - hm->vg_min_b[d] + 1;
  c->vg_too_large = hm->vg_error != 0;
  c->has_vg = true;
  c->vg_resolution = res;
  c->vg_cov_k = cov_cache_key(h, k);
  return c->vg_too_large ? vgicp_grid_too_large(h, c) : HGS_OK;
}

// inv_leaf: 1 / resolution for NDT's tables, 0 for VGICP's (its kernels take the resolution from VgicpConsts)
NdtTargetView voxel_target_view(const hgs_cloud* c, const VoxelTable& t, float inv_leaf) {
  NdtTargetView tv;
  tv.hash_keys = t.hash_keys, tv.hash_vals = t.hash_vals, tv.cells = t.cells, tv.meta = c->desc.meta, tv.hash_kv = t.hash_kv;
  tv.hash_mask = t.hash_cap - 1, tv.inv_leaf = inv_leaf;
  return tv;
}
NdtTargetView ndt_target_view(const hgs_handle* h, const hgs_cloud* t) { return voxel_target_view(t, t->ndt, 1.0f / (float)h->prm.resolution); }
NdtTargetView vgicp_target_view(const hgs_cloud* t) { return voxel_target_view(t, t->vg, 0.f); }

TargetView target_view(const hgs_cloud* c) {
  TargetView t;
  t.nodes = c->desc.nodes, t.pts = c->desc.pts, t.lpts = c->desc.lpts, t.cov = c->desc.cov, t.meta = c->desc.meta, t.P = c->P;
  t.seed_bits = c->has_seed ? c->seed_bits : 0, t.seed_tab = c->has_seed ? c->seed_block.as<const unsigned>() : nullptr;
  return t;
}

// The seed grid of a cloud that serves as the target of 1-NN searches (hgs_kernels.hip, seed_grid_lookup): built once per index, ~10 us.
int ensure_seed_grid(hgs_handle* h, hgs_cloud* c) {
  if (!h->seed_grid || c->has_seed || !c->has_index || c->n_input == 0) return HGS_OK;
  int bits = 12;
  while (bits < 24 && ((size_t)1 << bits) < 4 * c->n_input) bits++;
  const size_t bytes = seed_grid_entries(bits) * sizeof(unsigned);
  if (!c->seed_block.p || c->seed_bits != bits) {
    HGS_HIP(h, c->seed_block.alloc(bytes));
    c->seed_bits = bits;
  }
  HGS_HIP(h, hipMemsetAsync(c->seed_block.p, 0xff, bytes, h->stream));
  launch_seed_grid_build(h->stream, c->desc.pts, c->desc.meta, (int)c->n_input, c->seed_block.as<unsigned>(), bits);
  HGS_HIP(h, hipGetLastError());
  c->has_seed = true;
  return HGS_OK;
}

// The same for every cloud of a list that lacks one (hgs_calc_fitness_score_batch: the distinct tree sides of a graph update's edges): ONE clearing and
// ONE filling launch over a job list instead of a memset and a launch per cloud; every table is word for word what ensure_seed_grid builds.
int ensure_seed_grids(hgs_handle* h, const std::vector<hgs_cloud*>& all) {
  if (!h->seed_grid) return HGS_OK;
  std::vector<hgs_cloud*> todo;
  for (hgs_cloud* c : all)
    if (!c->has_seed && c->has_index && c->n_input > 0 && std::find(todo.begin(), todo.end(), c) == todo.end()) todo.push_back(c);
  constexpr size_t kMaxJobs = 65535;  // grid.y of one launch
  for (size_t start = 0; start < todo.size(); start += kMaxJobs) {
    const size_t nj = std::min(kMaxJobs, todo.size() - start);
    std::vector<SeedGridJob> jobs(nj);
    size_t max_entries = 0;
    int max_n = 0;
    for (size_t j = 0; j < nj; j++) {
      hgs_cloud* c = todo[start + j];
      int bits = 12;
      while (bits < 24 && ((size_t)1 << bits) < 4 * c->n_input) bits++;
      const size_t entries = seed_grid_entries(bits);
      if (!c->seed_block.p || c->seed_bits != bits) {
        HGS_HIP(h, c->seed_block.alloc(entries * sizeof(unsigned)));
        c->seed_bits = bits;
      }
      jobs[j] = SeedGridJob{c->desc.pts, c->desc.meta, c->seed_block.as<unsigned>(), bits, 0};
      max_entries = std::max(max_entries, entries), max_n = std::max(max_n, (int)c->n_input);
    }
    HGS_HIP(h, h->seed_jobs.reserve(nj * sizeof(SeedGridJob)));
    HGS_HIP(h, h->up.upload(h->seed_jobs.p, jobs.data(), nj * sizeof(SeedGridJob), h->stream));
    launch_seed_grid_build_batch(h->stream, h->seed_jobs.as<SeedGridJob>(), (int)nj, max_entries, max_n);
    HGS_HIP(h, hipGetLastError());
    for (size_t j = 0; j < nj; j++) todo[start + j]->has_seed = true;
  }
  return HGS_OK;
}

// (HGS_TRACE: device-side per-iteration trace, parity debugging; the mapping itself is hgs_consts.h)
NdtConsts engine_ndt_consts(const hgs_params& p) {
  NdtConsts c = ndt_consts(p);
  c.pad = std::getenv("HGS_TRACE") ? 1 : 0;
  return c;
}

// The lanes of a batch are HIP streams, and what makes them concurrent is that the runtime puts them on different hardware queues — of which it uses
// 4 by default (GPU_MAX_HW_QUEUES, read once when the HIP runtime initialises).  One engine's four lanes get one each; in a process that hosts several
// engines (the nodelet manager: the odometry engine AND the loop-closure engine) streams beyond the queue count share a queue and a batch runs 8 % slower
// (measured with three engines on 4 queues, profiles/r04_lanes_queues.log; with 8 queues the effect is gone).  The library does NOT touch the
// environment (rounds 1-4 called setenv from a static initialiser: a plugin must not change its host process).  Instead every stream an engine
// creates is counted against the process's queue budget — GPU_MAX_HW_QUEUES if the launcher set it (INTEGRATION.md recommends 8), HIP's default 4
// otherwise — and a batch opens only as many lanes as the budget still has room for (never fewer than one: the engine's own stream).
// (the budget is per DEVICE: in the one-process-several-GPUs shape — LoopMatcherHIP, bench.py --single-process — every GPU has its own queues)
constexpr int kMaxCountedDevices = 64;
std::atomic<int> g_streams_in_use[kMaxCountedDevices] = {};
std::atomic<int>& streams_in_use(int device) { return g_streams_in_use[(unsigned)device % kMaxCountedDevices]; }
int hw_queue_budget() {
  static const int budget = [] {
    const char* e = std::getenv("GPU_MAX_HW_QUEUES");
    const int v = e ? std::atoi(e) : 0;
    return v > 0 ? v : 4;
  }();
  return budget;
}
constexpr int kFloorMaxChunk = 4096;  // hypotheses per RANSAC round of hgs_detect_floor ("floor_chunk")
constexpr int kMaxLanes = 8;  // HGS_BATCH_LANES up to 8 (A/B runs); the default choice stays at 3-4 and is further bounded by the queue budget above

// Progress mirror of one lane of a batch: device counters + two ints of host-mapped pinned memory the kernels write into.
int make_progress(hgs_handle* h, int lane, int B, Progress* out) {
  if (h->early_pending) {  // the rounds that were queued behind an early result (they tick the mirror) have to be through before the mirror is reset
    HGS_HIP(h, hipEventSynchronize(h->early_event));
    h->early_pending = false;
  }
  HGS_HIP(h, h->done.reserve(64));
  HGS_HIP(h, h->h_flags.reserve(64));
  volatile int* hf = h->h_flags.as<volatile int>() + 2 * lane;
  hf[0] = 0, hf[1] = 0;  // everything enqueued earlier on these streams has completed (results were fetched with a sync)
  out->dev = h->done.as<int>() + 2 * lane;
  out->host_done = hf, out->host_rounds = hf + 1;
  out->B = B, out->pad = 0;
  return HGS_OK;
}

// One lane of a batch: problems [b0, b0 + B) on their own stream with their own progress mirror and partial-sum buffers.
struct BatchLane {
  hipStream_t stream = nullptr;
  int b0 = 0, B = 0;
  Progress prog{};
  double* partials = nullptr;
  double* partials_err = nullptr;
  long round = 0;
  bool finished = false;
};

// How many lanes a batch of B problems opens (`lanes`), and how many of them run the ahead group on priority streams (`ahead`; 0: contiguous lanes of equal
// priority).  ordered: the caller has sorted the problems for ordered lanes (run_batch) — granted only where more than one lane opens anyway.
struct LanePlan {
  int lanes, ahead;
};
// assume_streams >= 0 (hgs_debug_plan_lanes): plan as if the process held that many streams on the device instead of the counted ones.
LanePlan plan_lanes(hgs_handle* h, int B, int tiles_per_problem, bool ordered, int assume_streams = -1) {
  // round 3, 64 x 119 k FAST_GICP batch: 1 / 2 / 3 / 4 lanes = 5615 / 5755 / 5787 / 5811 registrations/s (round 2's kernels preferred 2 above 32 problems)
  // NDT (one launch per iteration, work queue inside): 2 / 3 / 4 lanes = 1679 / 1724 / 1652 on the 64-candidate batch (round 2: 1403 / 1384 / 1326)
  // round 6, batches of SMALL problems (candidate keyframes of a KITTI run: prefiltered sweeps of 11-14 k points; scripts/probes/small_batch_lanes_probe.py,
  // profiles/r06_small_batch_lanes.log): GICP's short kernels gain nothing from concurrent chains and pay for the extra streams — one lane: 6 / 12 / 24 / 48
  // candidates x 11 k points 0.558 -> 0.505 / 0.683 -> 0.624 / 0.810 -> 0.782 / 1.092 -> 1.019 ms per detection (96 candidates: equal; 65 k-point problems:
  // four lanes from 8 candidates on) — while NDT_OMP's passes want all four lanes also above 32 problems (48 x 11 k: 7.9 -> 6.8 ms).
  const bool small_problems = tiles_per_problem > 0 && tiles_per_problem <= 96;
  const int by_size = h->prm.method == HGS_NDT_OMP ? (B > 32 && !small_problems ? 3 : 4) : (small_problems && (long)B * tiles_per_problem <= 3072 ? 1 : 4);
  const int wanted = h->batch_lanes > 0 ? h->batch_lanes : by_size;
  int n = h->profiling ? 1 : std::max(1, std::min(std::min(wanted, kMaxLanes), B));  // (h_flags / done hold 2 ints per lane: 64 bytes = 8 lanes)
  // the process's hardware-queue budget (above): lane streams this engine already owns are free, new ones only while there is room.
  // HGS_BATCH_LANES (A/B runs) overrides the budget.
  int owned = 0, owned_prio = 0;
  while (owned < kMaxLanes - 1 && h->lane_stream[owned]) owned++;
  while (owned_prio < 2 && h->prio_stream[owned_prio]) owned_prio++;
  const int room = std::max(0, hw_queue_budget() - (assume_streams >= 0 ? assume_streams : streams_in_use(h->device).load(std::memory_order_relaxed)));
  const int plain = h->batch_lanes <= 0 ? std::min(n, 1 + owned + room) : n;
  if (!ordered || h->profiling || plain < 2) return LanePlan{plain, 0};
  // ordered lanes: four lanes = two ahead (priority streams) + two crowd (the engine's own stream and one more), three = 1 + 2, two = 1 + 1.  The
  // priority streams are streams like any other to the budget: the largest plan whose NEW streams the budget has room for — and if that is fewer
  // lanes than the plain plan opens (an engine that owns plain lane streams in a process whose budget is spent), the plain plan stands
  n = std::min(n, 4);
  auto ahead_of = [](int lanes) { return lanes >= 4 ? 2 : 1; };
  if (h->batch_lanes <= 0)
    while (n > 1 && std::max(0, ahead_of(n) - owned_prio) + std::max(0, n - ahead_of(n) - 1 - owned) > room) n--;
  if (n < 2 || n < std::min(plain, 4)) return LanePlan{plain, 0};
  return LanePlan{n, ahead_of(n)};
}

// highest-priority, non-blocking; the host emulation of the kernels has no stream priorities: a plain stream there
hipError_t create_priority_stream(hipStream_t* out) {
#ifdef HGS_SIMT_EMULATION
  return hipStreamCreateWithFlags(out, hipStreamNonBlocking);
#else
  int least = 0, greatest = 0;
  const hipError_t e = hipDeviceGetStreamPriorityRange(&least, &greatest);
  if (e != hipSuccess) return e;
  return hipStreamCreateWithPriority(out, hipStreamNonBlocking, greatest);
#endif
}

// Splits B problems into lanes (contiguous ranges) and makes the extra streams wait for what the main stream has enqueued
// so far (indices, covariances, descriptors, guesses).  Profiling keeps one lane: the stage timers bracket launches on the
// main stream and are meant to time kernels that have the device to themselves.
// ahead_problems > 0: the caller has put the batch's ahead group in front (run_batch: problems [0, ahead_problems)); the plan's ahead lanes share it, the
// other lanes the rest.  The lane on the engine's own stream is then not the first of the list — nothing but close_lanes cared.
int open_lanes(hgs_handle* h, int B, size_t partial_bytes_per_problem, size_t partial_err_bytes_per_problem, std::vector<BatchLane>& lanes, int tiles_per_problem,
               int ahead_problems = 0) {
  const LanePlan plan = plan_lanes(h, B, tiles_per_problem, ahead_problems > 0);
  const int n = plan.lanes;
  h->last_lanes = n, h->last_ahead_lanes = plan.ahead;
  lanes.assign(n, BatchLane{});
  for (int i = 0, b0 = 0, extra = 0; i < n; i++) {
    BatchLane& L = lanes[i];
    const bool ahead = i < plan.ahead;
    // (without ahead lanes: one group of all B problems over all n lanes)
    const int group_end = plan.ahead == 0 ? B : (ahead ? ahead_problems : B), group_lanes_left = plan.ahead == 0 ? n - i : (ahead ? plan.ahead - i : n - i);
    L.b0 = b0, L.B = (group_end - b0) / group_lanes_left;
    b0 += L.B;
    HGS_TRY(make_progress(h, i, L.B, &L.prog));
    if (i == plan.ahead) {  // the first lane that is not ahead: the engine's own stream and buffers
      L.stream = h->stream;
      L.partials = h->partials.as<double>(), L.partials_err = h->partials_err.as<double>();
      continue;
    }
    hipStream_t& ls = ahead ? h->prio_stream[i] : h->lane_stream[i - plan.ahead - 1];
    if (!ls) {
      HGS_HIP(h, ahead ? create_priority_stream(&ls) : hipStreamCreateWithFlags(&ls, hipStreamNonBlocking));
      streams_in_use(h->device).fetch_add(1, std::memory_order_relaxed);
    }
    L.stream = ls;
    HGS_HIP(h, h->lane_partials[extra].reserve((size_t)L.B * partial_bytes_per_problem));
    HGS_HIP(h, h->lane_partials_err[extra].reserve((size_t)L.B * partial_err_bytes_per_problem));
    L.partials = h->lane_partials[extra].as<double>(), L.partials_err = h->lane_partials_err[extra].as<double>();
    extra++;
  }
  if (n > 1) {
    // Round 5 removed the host synchronisations behind the index build and the covariance pass (they only protected a pinned staging buffer: PinnedRing).
    // For a batch with several lanes one synchronisation stays HERE, because it measures faster: with it the host enqueues lane after lane onto an idle
    // device; without it every lane's first rounds are already queued behind one event when the covariance pass ends and all lanes are released in the
    // same instant — 5306 instead of 5381 registrations/s FAST_GICP, 7435 / 7574 PLANE, 2307 / 2317 NDT_OMP (same library, HGS_LANE_START=0 / 1,
    // profiles/r05_lane_start.log).  Releasing lane i + 1 behind lane i's first point kernel instead (a deliberate stagger) is worse than both
    // (5250 / 7269): the ramp costs three unseeded linearisations.  A single registration (one lane) never gets here.
    if (h->lane_start != 0) HGS_HIP(h, hipStreamSynchronize(h->stream));
    if (!h->lane_event[0]) HGS_HIP(h, hipEventCreateWithFlags(&h->lane_event[0], hipEventDisableTiming));
    HGS_HIP(h, hipEventRecord(h->lane_event[0], h->stream));
    for (BatchLane& L : lanes)
      if (L.stream != h->stream) HGS_HIP(h, hipStreamWaitEvent(L.stream, h->lane_event[0], 0));
  }
  return HGS_OK;
}

// The main stream continues after every lane has finished.
int close_lanes(hgs_handle* h, std::vector<BatchLane>& lanes) {
  for (size_t i = 0; i < lanes.size(); i++) {
    if (lanes[i].stream == h->stream) continue;
    const size_t ev = i == 0 ? lanes.size() : i;  // (lane_event[0] is open_lanes'; ordered lanes: lane 0 is an ahead lane and at most 4 lanes open)
    if (!h->lane_event[ev]) HGS_HIP(h, hipEventCreateWithFlags(&h->lane_event[ev], hipEventDisableTiming));
    HGS_HIP(h, hipEventRecord(h->lane_event[ev], lanes[i].stream));
    HGS_HIP(h, hipStreamWaitEvent(h->stream, h->lane_event[ev], 0));
  }
  return HGS_OK;
}

// Keeps every lane's queue `kRunAhead` rounds ahead of the device without synchronising: enqueue_round(lane) is called
// whenever a lane that still has unfinished problems has fewer than kRunAhead rounds in flight, on_finished(lane) once
// when the lane's problems have all finished (or max_rounds is exhausted) — what it enqueues runs behind the lane's
// last rounds while the other lanes are still iterating; returns once every lane has finished.  If the mirrors stop advancing although the streams have drained (a launch
// failed) the loop keeps enqueueing up to max_rounds: the caller then sees the error from hipGetLastError.
constexpr long kRunAhead = 2;  // one round executing, one queued behind it (a round is >= 100 us, enqueueing one ~20 us)
template <typename F, typename G>
void drive_lanes(std::vector<BatchLane>& lanes, long max_rounds, F&& enqueue_round, G&& on_finished, long run_ahead = kRunAhead) {
  long spins = 0;
  for (;;) {
    bool all_finished = true, enqueued = false;
    for (BatchLane& L : lanes) {
      if (L.finished) continue;
      if (*L.prog.host_done || L.round >= max_rounds) {
        L.finished = true;
        on_finished(L);
        continue;
      }
      all_finished = false;
      if (L.round - (long)*L.prog.host_rounds < run_ahead) {
        enqueue_round(L);
        L.round++;
        enqueued = true;
      }
    }
    if (all_finished) return;
    if (enqueued) {
      spins = 0;
      continue;
    }
    if ((++spins & 0x3ff) == 0) {
      for (BatchLane& L : lanes)
        if (!L.finished && !*L.prog.host_done && hipStreamQuery(L.stream) == hipSuccess && !*L.prog.host_done &&
            L.round - (long)*L.prog.host_rounds >= run_ahead) {
          enqueue_round(L);  // drained without the mirror advancing: do not spin forever, max_rounds bounds the loop
          L.round++;
        }
    }
#if defined(__x86_64__)
    __builtin_ia32_pause();
#endif
  }
}

// What the launches of a batch are sized by, computed once per batch (batch_shape).
struct BatchShape {
  int B, max_n;
  int qpw, nn_tile;                   // queries per packet and points per block of the 1-NN kernels (k_gicp_linearize / k_fitness)
  bool gicp_round2;                   // the LM round in two launches
  int lin_qpw, lin_tile, lin_blocks;  // ... whose k_gicp_linearize<true> may run shorter packets
  int max_blocks, err_blocks;         // rows of the partial-sum buffers / blocks of the 256-point kernels, per problem
  const CloudDesc* d_descs;           // the sources' descriptors on the device
  const TargetView* d_tviews;         // one target per problem, on the device (run_group_batch); null: every problem against the handle's target
  const NdtTargetView* d_vviews;      // ... and its voxel table (run_pair_batch: NDT_OMP, FAST_VGICP); null: the handle's target's
};

// launch(target): with the lane's slice of the per-problem views, or with the one view `tv` by value — the two families of instantiations of the point kernels
template <typename F>
void with_lane_target(const BatchShape& s, const BatchLane& L, const TargetView& tv, F&& launch) {
  if (s.d_tviews) launch(s.d_tviews + L.b0);
  else launch(tv);
}

// lm_rounds: the batch iterates (run_batch); false: a fitness pass alone (run_fitness), which has no two-launch rounds to size for
int batch_shape(hgs_handle* h, const std::vector<hgs_cloud*>& sources, bool lm_rounds, BatchShape* out, int* const* corr_of = nullptr) {
  BatchShape& s = *out;
  s.d_tviews = nullptr, s.d_vviews = nullptr;
  s.B = (int)sources.size();
  s.max_n = 0;
  for (hgs_cloud* c : sources) s.max_n = std::max(s.max_n, (int)c->n_input);
  const int B = s.B, max_n = s.max_n;
  s.qpw = 64;  // queries per packet of the 1-NN kernels; shorter packets cost a batch ~13 % more work (round 2) ...
  s.nn_tile = (kBlock / 64) * s.qpw * kNW;                 // points per block of k_gicp_linearize / k_fitness (their own tiling formula)
  // ... but a launch of a FEW blocks lasts as long as one packet walk, and a shorter packet walks fewer nodes: the two-launch LM rounds of a small single
  // registration run k_gicp_linearize<true> with 16- / 32-query packets, whose last wave per block redoes the 64-point wave rows so that no bit of the
  // result depends on the packet size (hgs_kernels.hip).  Same-box (profiles/r06_ab12_nn_qpw.log, r06_ab13): the 13.5 k-point odometry source hgs_align
  // 0.344 -> 0.315 ms with 16; by size (profiles/r06_nn_qpw_sizes.log): 7 k points -6 %, 11 k -4 %, 16 k -3 %, 22 k -1 %, 64 k +2 % (32 never wins).
  // nn_qpw (option): 0 = by launch size, 16 / 32 / 64 = that packet.
  // A launch of a few problems (a single registration: the odometry step, config 2) is a chain of ~4 us kernels in which the two per-problem control launches
  // of an LM round cost as much as its two point kernels: such launches run the round in TWO launches, the control steps replicated in every block of
  // k_gicp_linearize<true> / k_gicp_error<true> (hgs_kernels.hip).  The states then alternate between two buffers; a whole round leaves them in the first.
  s.gicp_round2 = lm_rounds && h->prm.method == HGS_FAST_GICP && h->fused_rounds && max_n <= h->fused_rounds_below &&
                  (B <= h->fused_rounds_max_problems || (long)B * ((max_n + kBlock - 1) / kBlock) <= (long)h->fused_rounds_max_blocks);
  const long tiles64 = (long)B * ((max_n + s.nn_tile - 1) / s.nn_tile);
  s.lin_qpw = !s.gicp_round2 ? 64 : h->nn_qpw > 0 ? h->nn_qpw : tiles64 <= (long)h->nn_qpw16_below ? 16 : tiles64 <= (long)h->nn_qpw32_below ? 32 : 64;
  s.lin_tile = (kBlock / 64) * s.lin_qpw * kNW;
  s.lin_blocks = std::max(1, (max_n + s.lin_tile - 1) / s.lin_tile);
  s.max_blocks = std::max(1, s.lin_qpw < 64 ? (max_n + 63) / 64 : (max_n + s.nn_tile - 1) / s.nn_tile);  // >= the tile (row) count of every kernel of the loop
  s.err_blocks = std::max(1, (max_n + kBlock - 1) / kBlock);
  return upload_descs(h, sources, false, &s.d_descs, nullptr, corr_of);
}

// getFitnessScore of one lane's problems at the poses stored in h->results (exact 1-NN of every transformed source point in the target).
// corr_seeds: the sources' corr[] hold their correspondences against THIS target and seed the search; otherwise the target's seed grid does.
bool corr_seeds_fitness(int method) { return method == HGS_FAST_GICP || method == HGS_ICP; }
void lane_fitness(hgs_handle* h, BatchLane& L, const BatchShape& s, double max_range, bool corr_seeds) {
  StageTimer tm(h, HGS_STAGE_FITNESS);
  DevResult* res = h->results.as<DevResult>() + L.b0;
  with_lane_target(s, L, s.d_tviews ? TargetView{} : target_view(h->target),
                   [&](auto tgt) { launch_fitness(L.stream, s.d_descs + L.b0, tgt, res, max_range, L.partials_err, s.max_blocks, L.B, corr_seeds ? 1 : 0, s.qpw); });
  launch_fitness_final(L.stream, s.d_descs + L.b0, L.partials_err, s.max_blocks, res, L.B, s.nn_tile);
}
// behind a lane's result kernel: the fitness pass of a batch that asked for one (FAST_GICP and ICP start it from the final correspondences)
void lane_fitness_tail(hgs_handle* h, BatchLane& L, const BatchShape& s, const double* fit_max_range) {
  if (fit_max_range) lane_fitness(h, L, s, *fit_max_range, corr_seeds_fitness(h->prm.method));
}

// The rounds of a FAST_GICP / FAST_VGICP batch.  guess_in_args: a single GICP registration, whose guess rides in k_gicp_init1's arguments.
// ahead_problems: run_batch has sorted the problems for ordered lanes, the first that many are the ahead group (open_lanes); 0: not.
int run_gicp_rounds(hgs_handle* h, const BatchShape& s, const float* guesses_host, bool guess_in_args, const double* fit_max_range, int ahead_problems = 0) {
  const int B = s.B, max_blocks = s.max_blocks;
  hgs_cloud* tgt = h->target;
  const bool voxel = h->prm.method == HGS_FAST_VGICP;
  const GicpConsts c = gicp_consts(h->prm);
  const VgicpConsts vc = vgicp_consts(h->prm);
  const bool round2 = s.gicp_round2;
  // One registration without a fitness pass behind it (hgs_align: the odometry step): the kernel that finds it finished writes the result record into
  // host-mapped memory in front of the mirror's `done` flag; the poll below returns with it — no result kernel, no copy, no synchronisation.
  const bool early = round2 && B == 1 && !fit_max_range && h->early_result && !h->profiling;
  DevResult* early_out = nullptr;
  if (early) {
    HGS_HIP(h, h->h_early.reserve(sizeof(DevResult)));
    early_out = h->h_early.as<DevResult>();
  }
  HGS_HIP(h, h->states.reserve((size_t)B * sizeof(GicpState) * (round2 ? 2 : 1)));
  GicpState* st = h->states.as<GicpState>();
  GicpState* st_other = st + B;
  const TargetView tv = s.d_tviews || s.d_vviews ? TargetView{} : target_view(tgt);  // (run_group_batch, run_pair_batch: the views are on the device, the handle's target plays no part)
  const NdtTargetView vtv = voxel && !s.d_vviews ? vgicp_target_view(tgt) : NdtTargetView{};  // (run_pair_batch: one voxel map per problem, on the device)
  const long max_rounds = (long)std::max(1, c.max_iterations) * std::max(1, c.lm_max_iterations) + 2 + (round2 ? 1 : 0);  // (round2: a round's accept / reject runs in the next round's first kernel)
  std::vector<BatchLane> lanes;
  HGS_TRY(open_lanes(h, B, (size_t)max_blocks * kAccNdt * sizeof(double), (size_t)max_blocks * 2 * sizeof(double), lanes, s.err_blocks, ahead_problems));
  auto finish_lane = [&](BatchLane& L) {
    if (early && *L.prog.host_done) {  // (not when the lane ran out of rounds: then the result kernel + copy below fetch whatever state it is in)
      h->early_valid = true;
      return;
    }
    launch_gicp_results(L.stream, st + L.b0, h->results.as<DevResult>() + L.b0, L.B);
    lane_fitness_tail(h, L, s, fit_max_range);
  };
  if (guess_in_args) launch_gicp_init1(lanes[0].stream, st, guesses_host, lanes[0].prog);
  else
    for (BatchLane& L : lanes) launch_gicp_init(L.stream, st + L.b0, h->guesses.as<float>() + (size_t)L.b0 * 16, L.B, L.prog);
  drive_lanes(lanes, max_rounds, [&](BatchLane& L) {
    const CloudDesc* dd = s.d_descs + L.b0;
    GicpState* ls = st + L.b0;
    if (round2) {
      {
        StageTimer tm(h, HGS_STAGE_LINEARIZE);
        with_lane_target(s, L, tv, [&](auto t) {
          launch_gicp_linearize_round2(L.stream, dd, t, ls, st_other + L.b0, c, L.partials, L.partials_err, max_blocks, s.lin_blocks, L.B, s.lin_qpw, L.prog,
                                       h->results.as<DevResult>() + L.b0, early_out);
        });
      }
      StageTimer tm(h, HGS_STAGE_ERROR);
      with_lane_target(s, L, tv, [&](auto t) {
        launch_gicp_error_round2(L.stream, dd, t, st_other + L.b0, ls, c, L.partials, L.partials_err, max_blocks, s.err_blocks, L.B, s.lin_tile);
      });
      return;
    }
    {
      StageTimer tm(h, HGS_STAGE_LINEARIZE);
      if (voxel && s.d_vviews) launch_vgicp_linearize(L.stream, dd, s.d_vviews + L.b0, ls, vc, L.partials, max_blocks, L.B);
      else if (voxel) launch_vgicp_linearize(L.stream, dd, vtv, ls, vc, L.partials, max_blocks, L.B);
      else with_lane_target(s, L, tv, [&](auto t) { launch_gicp_linearize(L.stream, dd, t, ls, c, L.partials, max_blocks, L.B, s.qpw); });
    }
    {
      StageTimer tm(h, HGS_STAGE_SOLVE);
      launch_gicp_solve(L.stream, dd, ls, c, L.partials, max_blocks, L.B, voxel ? kBlock : s.nn_tile);
    }
    {
      StageTimer tm(h, HGS_STAGE_ERROR);
      if (voxel && s.d_vviews) launch_vgicp_error(L.stream, dd, s.d_vviews + L.b0, ls, vc, L.partials_err, max_blocks, L.B);
      else if (voxel) launch_vgicp_error(L.stream, dd, vtv, ls, vc, L.partials_err, max_blocks, L.B);
      else with_lane_target(s, L, tv, [&](auto t) { launch_gicp_error(L.stream, dd, t, ls, L.partials_err, max_blocks, L.B); });
    }
    {
      StageTimer tm(h, HGS_STAGE_SOLVE);
      launch_gicp_decide(L.stream, dd, ls, c, L.partials_err, max_blocks, L.B, L.prog);
    }
  }, finish_lane, early ? (long)h->early_run_ahead : kRunAhead);
  HGS_TRY(close_lanes(h, lanes));
  if (h->early_valid) {  // rounds may still be queued (the host runs ahead): the next batch's mirror reset waits for them (make_progress)
    if (!h->early_event) HGS_HIP(h, hipEventCreateWithFlags(&h->early_event, hipEventDisableTiming));
    HGS_HIP(h, hipEventRecord(h->early_event, h->stream));
    h->early_pending = true;
  }
  return HGS_OK;
}

// The rounds of an ICP batch: one correspondence pass + one control step per round; a registration takes at most max(1, max_iterations) rounds
// (+2 as the other methods)
int run_icp_rounds(hgs_handle* h, const BatchShape& s, const double* fit_max_range) {
  const int B = s.B, max_blocks = s.max_blocks;
  const IcpConsts c = icp_consts(h->prm);
  HGS_HIP(h, h->states.reserve((size_t)B * sizeof(IcpState)));
  IcpState* st = h->states.as<IcpState>();
  const TargetView tv = s.d_tviews ? TargetView{} : target_view(h->target);
  const long max_rounds = (long)std::max(0, c.max_iterations) + 2;
  std::vector<BatchLane> lanes;
  HGS_TRY(open_lanes(h, B, (size_t)max_blocks * kAccIcp * sizeof(double), (size_t)max_blocks * 2 * sizeof(double), lanes, s.err_blocks));
  auto finish_lane = [&](BatchLane& L) {
    launch_icp_results(L.stream, st + L.b0, h->results.as<DevResult>() + L.b0, L.B);
    lane_fitness_tail(h, L, s, fit_max_range);
  };
  for (BatchLane& L : lanes) launch_icp_init(L.stream, st + L.b0, h->guesses.as<float>() + (size_t)L.b0 * 16, L.B, L.prog);
  drive_lanes(lanes, max_rounds, [&](BatchLane& L) {
    {
      StageTimer tm(h, HGS_STAGE_LINEARIZE);
      with_lane_target(s, L, tv, [&](auto t) { launch_icp_correspond(L.stream, s.d_descs + L.b0, t, st + L.b0, c, L.partials, max_blocks, L.B); });
    }
    StageTimer tm(h, HGS_STAGE_SOLVE);
    launch_icp_solve(L.stream, s.d_descs + L.b0, st + L.b0, c, L.partials, max_blocks, L.B, L.prog);
  }, finish_lane);
  return close_lanes(h, lanes);
}

// Work plan of every lane of an NDT batch: the (problem, tile) items of a pass are numbered by the prefix sums of the problems' tile counts
// (from n_input: an upper bound of the finite points), and pulled from a queue head in HBM (k_ndt_pass)
struct NdtLanePlan {
  int* tile_base;
  unsigned long long* queues;  // two heads, used alternately (k_ndt_pass)
  int blocks, chunk;
};
int ndt_lane_plans(hgs_handle* h, const std::vector<hgs_cloud*>& sources, const std::vector<BatchLane>& lanes, std::vector<NdtLanePlan>& plans) {
  plans.assign(lanes.size(), NdtLanePlan{});
  const size_t per_lane = align_up(16 + (sources.size() + 1) * sizeof(int), 256);
  bool tile_overflow = false;
  constexpr long long kMaxNdtBlocks = 1 << 16, kMaxNdtChunk = 1 << 10;  // far above anything HGS_NDT_RESIDENT / HGS_NDT_CHUNK are used with
  HGS_HIP(h, h->ndt_plan.reserve(per_lane * lanes.size()));
  void* staged = nullptr;
  int plan_slot = 0;
  HGS_HIP(h, h->up.stage(per_lane * lanes.size(), &staged, &plan_slot));
  std::memset(staged, 0, per_lane * lanes.size());
  char* const host = static_cast<char*>(staged);
  for (size_t li = 0; li < lanes.size(); li++) {
    const BatchLane& L = lanes[li];
    int* tb = reinterpret_cast<int*>(host + li * per_lane + 16);
    tb[0] = 0;
    // k_ndt_pass does its item arithmetic in 32-bit ints (queue head + blocks * chunk must fit): bound the lane's tile count here
    long long tiles64 = 0;
    for (int k = 0; k < L.B; k++) {
      tiles64 += std::max<long long>(1, ((long long)sources[L.b0 + k]->n_input + kBlock - 1) / kBlock);
      tile_overflow = tile_overflow || tiles64 > (long long)INT_MAX - (long long)kMaxNdtBlocks * kMaxNdtChunk;
      tb[k + 1] = tile_overflow ? 0 : (int)tiles64;
    }
    NdtLanePlan& P = plans[li];
    const int total = tb[L.B];
    if (tile_overflow) continue;
    P.blocks = std::max(1, std::min(total, h->ndt_resident_blocks > 0 ? std::min(h->ndt_resident_blocks, (int)kMaxNdtBlocks) : (lanes.size() > 1 ? 512 : 768)));
    // largest queue grab (the kernel sizes each grab by guided self-scheduling, at most this many items).  Fixed grabs
    // measured on the 16 x 119 k batch with 4 lanes: 1 -> 904, 2 -> 1062, 3 -> 980, 4 -> 936, 8 -> 845 registrations/s
    P.chunk = h->ndt_chunk > 0 ? std::min(h->ndt_chunk, (int)kMaxNdtChunk) : 8;
    P.queues = reinterpret_cast<unsigned long long*>((char*)h->ndt_plan.p + li * per_lane);
    P.tile_base = reinterpret_cast<int*>((char*)h->ndt_plan.p + li * per_lane + 16);
  }
  if (tile_overflow) {
    h->err = "NDT batch too large: the tiles of one lane do not fit 32-bit item arithmetic (more than ~5e11 source points in one call)";
    return HGS_ERR_INVALID_ARGUMENT;
  }
  HGS_HIP(h, hipMemcpyAsync(h->ndt_plan.p, host, per_lane * lanes.size(), hipMemcpyHostToDevice, h->stream));  // (round 4: a synchronous hipMemcpy of a pageable vector)
  HGS_HIP(h, h->up.commit(plan_slot, h->stream));
  // open_lanes() released lanes 1.. behind an event recorded BEFORE this copy: order them behind the plan as well, or a lane's first
  // k_ndt_init / k_ndt_pass could read the previous batch's tile_base / queue heads (round-5 advisor finding; tests/test_hip_parity.py
  // ::test_ndt_batches_of_different_shape_back_to_back poisons the plan between batches)
  if (lanes.size() > 1) {
    HGS_HIP(h, hipEventRecord(h->lane_event[0], h->stream));
    for (size_t i = 1; i < lanes.size(); i++) HGS_HIP(h, hipStreamWaitEvent(lanes[i].stream, h->lane_event[0], 0));
  }
  return HGS_OK;
}

// The rounds of an NDT_OMP batch: one kernel per round, the Newton step inside it — nothing to stagger
int run_ndt_rounds(hgs_handle* h, const std::vector<hgs_cloud*>& sources, const BatchShape& s, const double* fit_max_range) {
  const int B = s.B, max_blocks = s.max_blocks;
  const NdtConsts c = engine_ndt_consts(h->prm);
  HGS_HIP(h, h->states.reserve((size_t)B * sizeof(NdtState)));
  HGS_HIP(h, h->angles.reserve((size_t)B * sizeof(NdtAngles)));
  NdtState* st = h->states.as<NdtState>();
  NdtAngles* ang = h->angles.as<NdtAngles>();
  const NdtTargetView tv = s.d_vviews ? NdtTargetView{} : ndt_target_view(h, h->target);  // (run_pair_batch: the views are on the device)
  // the sums are order-independent (hgs_ndt.h): read the sources in Hilbert order whenever they have a search index
  // (neighbouring lanes then share cells), in input order otherwise
  if (h->ndt_sort == 1) HGS_TRY(ensure_index(h, sources));
  bool sorted = h->ndt_sort != 0;
  for (hgs_cloud* sc : sources) sorted = sorted && sc->has_index;
  HGS_HIP(h, h->ndt_accum.reserve((size_t)B * sizeof(NdtAccum)));
  NdtAccum* accum = h->ndt_accum.as<NdtAccum>();  // zeroed by k_ndt_init (one dispatch less than a memset in front of it)
  // one derivative pass per iteration as ndt_omp runs; up to 1 + 10 with the More-Thuente search
  const long max_rounds = ((long)c.max_iterations + 4) * (c.line_search ? 11 : 1);
  std::vector<BatchLane> lanes;
  HGS_TRY(open_lanes(h, B, (size_t)max_blocks * 2 * sizeof(double), (size_t)max_blocks * 2 * sizeof(double), lanes, s.err_blocks));
  auto finish_lane = [&](BatchLane& L) {
    launch_ndt_results(L.stream, s.d_descs + L.b0, st + L.b0, h->results.as<DevResult>() + L.b0, L.B);
    lane_fitness_tail(h, L, s, fit_max_range);
  };
  std::vector<NdtLanePlan> plans;
  HGS_TRY(ndt_lane_plans(h, sources, lanes, plans));
  for (BatchLane& L : lanes) launch_ndt_init(L.stream, st + L.b0, ang + L.b0, h->guesses.as<float>() + (size_t)L.b0 * 16, c, L.B, L.prog, accum + L.b0);
  drive_lanes(lanes, max_rounds, [&](BatchLane& L) {
    StageTimer tm(h, HGS_STAGE_LINEARIZE);
    const NdtLanePlan& P = plans[&L - lanes.data()];
    if (s.d_vviews)  // the lane's slice: a block's items are numbered within the lane, and so are the views it reloads (k_ndt_pass)
      launch_ndt_pass(L.stream, s.d_descs + L.b0, s.d_vviews + L.b0, st + L.b0, ang + L.b0, c, accum + L.b0, P.tile_base, P.queues, L.B, (int)(L.round & 1), P.blocks,
                      P.chunk, sorted ? 1 : 0, 0, L.prog);
    else
      launch_ndt_pass(L.stream, s.d_descs + L.b0, tv, st + L.b0, ang + L.b0, c, accum + L.b0, P.tile_base, P.queues, L.B, (int)(L.round & 1), P.blocks, P.chunk,
                      sorted ? 1 : 0, 0, L.prog);
  }, finish_lane);
  return close_lanes(h, lanes);
}

// Ordered lanes: the order a batch runs in.  The hint of a problem is the squared translation norm of its guess (elements 12, 13, 14 of the column-major
// 4x4; a non-finite one counts as FLT_MAX, so the comparison stays a strict weak order): a candidate far from the query overlaps it less and converges
// slower (DESIGN.md "Ordered lanes").  Stable, descending: order[i] = the caller's position of the problem that runs i-th.
constexpr int kLaneOrderMinProblems = 8;
void lane_order_of(const float* guesses, int B, std::vector<int>& order) {
  std::vector<float> hint(B);
  for (int b = 0; b < B; b++) {
    const float* t = guesses + (size_t)b * 16 + 12;
    const float d2 = t[0] * t[0] + t[1] * t[1] + t[2] * t[2];
    hint[b] = std::isfinite(d2) ? d2 : FLT_MAX;
  }
  order.resize(B);
  for (int b = 0; b < B; b++) order[b] = b;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return hint[a] > hint[b]; });
}

// Run all B registrations (sources vs the handle's target) to completion; results land in h->results (device).
// With fit_max_range the getFitnessScore pass of every problem (fit_sum / fit_count of its result record) is enqueued on
// the problem's lane as soon as the lane has converged, i.e. under the remaining iterations of the other lanes.
int run_batch(hgs_handle* h, const std::vector<hgs_cloud*>& sources, const float* guesses_host, const double* fit_max_range = nullptr) {
  const int B = (int)sources.size();
  h->early_valid = false;
  h->batch_order.clear();
  hgs_cloud* tgt = h->target;
  const int method = h->prm.method;
  const bool gicp = method == HGS_FAST_GICP || method == HGS_FAST_VGICP;
  std::vector<hgs_cloud*> all(sources);
  if (fit_max_range) {
    std::vector<hgs_cloud*> searched(sources);
    searched.push_back(tgt);
    HGS_TRY(ensure_index(h, searched));
  }
  if (gicp) {
    all.push_back(tgt);
    HGS_TRY(ensure_cov(h, all, h->prm.correspondence_randomness));
    if (method == HGS_FAST_VGICP) HGS_TRY(ensure_vgicp_target(h, tgt));
  } else if (method == HGS_ICP) {
    // the target's index always; the sources' too: k_icp_correspond reads them in Hilbert order (a wave's 64 queries are neighbours, and corr[]
    // is indexed like GICP's, so the fitness pass can start from it) and the reciprocal search walks the source's own tree
    all.push_back(tgt);
    HGS_TRY(ensure_index(h, all));
  } else {
    HGS_TRY(ensure_ndt_target(h, tgt));
  }
  if (fit_max_range && method != HGS_FAST_GICP) HGS_TRY(ensure_seed_grid(h, tgt));  // getFitnessScore without correspondences to start from (k_fitness)
  // Ordered lanes (hgs_handle::lane_order): the batch runs in an internal order, farthest guess first, whose first half goes to the ahead lanes.  From here to
  // fetch_results / k_results_to_records everything per problem (descriptors, guesses, states, records, partial sums) is in that order; a record does not
  // depend on where or when its problem runs, so the hint, however wrong, changes no bit of it.
  std::vector<hgs_cloud*> ordered_sources;
  std::vector<float> ordered_guesses;
  int ahead_problems = 0;
  if (gicp && h->lane_order && B >= kLaneOrderMinProblems) {
    int max_n = 0;
    for (hgs_cloud* c : sources) max_n = std::max(max_n, (int)c->n_input);
    if (plan_lanes(h, B, std::max(1, (max_n + kBlock - 1) / kBlock) /* BatchShape::err_blocks */, true).ahead > 0) {
      lane_order_of(guesses_host, B, h->batch_order);
      ordered_sources.resize(B), ordered_guesses.resize((size_t)B * 16);
      for (int i = 0; i < B; i++) {
        ordered_sources[i] = sources[h->batch_order[i]];
        std::memcpy(&ordered_guesses[(size_t)i * 16], guesses_host + (size_t)h->batch_order[i] * 16, 16 * sizeof(float));
      }
      guesses_host = ordered_guesses.data();
      ahead_problems = (B + 1) / 2;
    }
  }
  BatchShape s;
  HGS_TRY(batch_shape(h, ahead_problems ? ordered_sources : sources, true, &s));
  const bool guess_in_args = B == 1 && method == HGS_FAST_GICP;  // (a single GICP registration: the guess rides in k_gicp_init1's arguments)
  HGS_HIP(h, h->guesses.reserve((size_t)B * 16 * sizeof(float)));
  if (!guess_in_args) HGS_HIP(h, h->up.upload(h->guesses.p, guesses_host, (size_t)B * 16 * sizeof(float), h->stream));  // (the caller's array is pageable: through a pinned slot)
  HGS_HIP(h, h->results.reserve((size_t)B * sizeof(DevResult)));
  HGS_HIP(h, h->partials.reserve((size_t)B * s.max_blocks * kAccNdt * sizeof(double)));
  HGS_HIP(h, h->partials_err.reserve((size_t)B * s.max_blocks * 2 * sizeof(double)));
  if (gicp) HGS_TRY(run_gicp_rounds(h, s, guesses_host, guess_in_args, fit_max_range, ahead_problems));
  else if (method == HGS_ICP) HGS_TRY(run_icp_rounds(h, s, fit_max_range));
  else HGS_TRY(run_ndt_rounds(h, sources, s, fit_max_range));
  HGS_HIP(h, hipGetLastError());
  return HGS_OK;
}

// hgs_loop_match_groups: problem b registers sources[b] against targets[b] and runs getFitnessScore(max_range) behind it, all problems in ONE batch — the
// lanes, the two-launch rounds and the packet tiers are chosen by batch_shape / open_lanes on the whole list as for a batch against one target.  What differs:
//   * the target views sit in a device array, one per problem (the point kernels' const TargetView* instantiations read tviews[blockIdx.y]);
//   * every problem has its own correspondence scratch (h->group_corr, through its descriptor) instead of the source cloud's corr[]: one keyframe is a
//     candidate of several new keyframes.  The scratch starts at -1 like a cloud's corr[] behind its index build; the searches are exact and a seed only
//     bounds the walk (k_gicp_linearize), so a record equals the one a batch against that target alone gives, bit for bit;
//   * neither h->target nor h->source is read or written.
// FAST_GICP and ICP only (the caller has checked): their targets are a search index (+ covariances), which every cloud of the union gets in one ensure_* pass.
// fit_max_range null (hgs_align_pairs without a fitness pass): the registrations alone.
int run_group_batch(hgs_handle* h, const std::vector<hgs_cloud*>& targets, const std::vector<hgs_cloud*>& sources, const float* guesses_host, const double* fit_max_range) {
  const int B = (int)sources.size();
  const int method = h->prm.method;
  h->early_valid = false;
  h->batch_order.clear();
  std::vector<hgs_cloud*> all(sources);
  all.insert(all.end(), targets.begin(), targets.end());
  if (method == HGS_FAST_GICP) HGS_TRY(ensure_cov(h, all, h->prm.correspondence_randomness));
  else HGS_TRY(ensure_index(h, all));
  if (fit_max_range && method != HGS_FAST_GICP)  // as run_batch: the fitness pass of a point without a correspondence starts from the target's seed grid
    for (hgs_cloud* t : targets) HGS_TRY(ensure_seed_grid(h, t));
  // the correspondence scratch of problem b: as many entries as the source's own corr[] (its padded point count), 256-byte aligned
  std::vector<size_t> corr_off(B + 1, 0);
  for (int b = 0; b < B; b++) corr_off[b + 1] = corr_off[b] + align_up((size_t)sources[b]->P * kLeaf, 64);
  HGS_HIP(h, h->group_corr.reserve(std::max<size_t>(1, corr_off[B]) * sizeof(int)));
  HGS_HIP(h, hipMemsetAsync(h->group_corr.p, 0xff, corr_off[B] * sizeof(int), h->stream));
  std::vector<int*> corr_of(B);
  for (int b = 0; b < B; b++) corr_of[b] = h->group_corr.as<int>() + corr_off[b];
  std::vector<TargetView> views(B);
  for (int b = 0; b < B; b++) views[b] = target_view(targets[b]);
  HGS_HIP(h, h->group_tviews.reserve((size_t)B * sizeof(TargetView)));
  HGS_HIP(h, h->up.upload(h->group_tviews.p, views.data(), (size_t)B * sizeof(TargetView), h->stream));
  BatchShape s;
  HGS_TRY(batch_shape(h, sources, true, &s, corr_of.data()));
  s.d_tviews = h->group_tviews.as<TargetView>();
  HGS_HIP(h, h->guesses.reserve((size_t)B * 16 * sizeof(float)));
  HGS_HIP(h, h->up.upload(h->guesses.p, guesses_host, (size_t)B * 16 * sizeof(float), h->stream));
  HGS_HIP(h, h->results.reserve((size_t)B * sizeof(DevResult)));
  HGS_HIP(h, h->partials.reserve((size_t)B * s.max_blocks * kAccNdt * sizeof(double)));
  HGS_HIP(h, h->partials_err.reserve((size_t)B * s.max_blocks * 2 * sizeof(double)));
  if (method == HGS_FAST_GICP) HGS_TRY(run_gicp_rounds(h, s, guesses_host, false, fit_max_range));
  else HGS_TRY(run_icp_rounds(h, s, fit_max_range));
  HGS_HIP(h, hipGetLastError());
  return HGS_OK;
}

// hgs_align_pairs: problem b registers sources[b] against targets[b] from its own guess, all problems in ONE batch, with getFitnessScore(*fit_max_range)
// behind each on request.  FAST_GICP and ICP: run_group_batch.  NDT_OMP and FAST_VGICP: their targets are voxel tables, cached on the cloud —
//   * one ensure_* pass over the union of the clouds (FAST_VGICP: covariances; a fitness pass: search indices and the targets' seed grids), one table build
//     per distinct target that lacks one;
//   * one NdtTargetView per problem in a device array (h->group_vviews), read by the const NdtTargetView* instantiations of k_ndt_pass /
//     k_vgicp_linearize / k_vgicp_error; the fitness pass reads h->group_tviews as in run_group_batch;
//   * FAST_VGICP keeps a point's voxel hit count in corr[] between its two kernels, so every problem gets its own scratch as in run_group_batch (a cloud
//     may be the source of several problems); NDT_OMP reads and writes no corr[];
//   * lanes, lane plans and launch shapes are chosen on the whole problem list as for a batch against one target: a lane boundary may fall anywhere;
//   * neither h->target nor h->source is read or written.
int run_pair_batch(hgs_handle* h, const std::vector<hgs_cloud*>& targets, const std::vector<hgs_cloud*>& sources, const float* guesses_host, const double* fit_max_range) {
  const int method = h->prm.method;
  if (method == HGS_FAST_GICP || method == HGS_ICP) return run_group_batch(h, targets, sources, guesses_host, fit_max_range);
  const int B = (int)sources.size();
  const bool voxel = method == HGS_FAST_VGICP;
  h->early_valid = false;
  h->batch_order.clear();
  std::vector<hgs_cloud*> all(sources);
  all.insert(all.end(), targets.begin(), targets.end());
  std::vector<hgs_cloud*> distinct;  // targets, in order of first appearance
  for (hgs_cloud* t : targets)
    if (std::find(distinct.begin(), distinct.end(), t) == distinct.end()) distinct.push_back(t);
  if (fit_max_range) HGS_TRY(ensure_index(h, all));
  if (voxel) {
    HGS_TRY(ensure_cov(h, all, h->prm.correspondence_randomness));
    for (hgs_cloud* t : distinct) {
      const int rc = ensure_vgicp_target(h, t);
      if (rc == HGS_ERR_UNSUPPORTED) {  // (vgicp_grid_too_large has described the grid: say which pair it belongs to)
        const size_t pair = (size_t)(std::find(targets.begin(), targets.end(), t) - targets.begin());
        h->err = "hgs_align_pairs: pair " + std::to_string(pair) + ": " + h->err;
      }
      HGS_TRY(rc);
    }
  } else {
    for (hgs_cloud* t : distinct) HGS_TRY(ensure_ndt_target(h, t));
  }
  if (fit_max_range) HGS_TRY(ensure_seed_grids(h, distinct));
  std::vector<int*> corr_of;
  if (voxel) {
    std::vector<size_t> corr_off(B + 1, 0);
    for (int b = 0; b < B; b++) corr_off[b + 1] = corr_off[b] + align_up((size_t)sources[b]->P * kLeaf, 64);
    HGS_HIP(h, h->group_corr.reserve(std::max<size_t>(1, corr_off[B]) * sizeof(int)));
    HGS_HIP(h, hipMemsetAsync(h->group_corr.p, 0xff, corr_off[B] * sizeof(int), h->stream));
    corr_of.resize(B);
    for (int b = 0; b < B; b++) corr_of[b] = h->group_corr.as<int>() + corr_off[b];
  }
  std::vector<NdtTargetView> vviews(B);
  for (int b = 0; b < B; b++) vviews[b] = voxel ? vgicp_target_view(targets[b]) : ndt_target_view(h, targets[b]);
  HGS_HIP(h, h->group_vviews.reserve((size_t)B * sizeof(NdtTargetView)));
  HGS_HIP(h, h->up.upload(h->group_vviews.p, vviews.data(), (size_t)B * sizeof(NdtTargetView), h->stream));
  if (fit_max_range) {
    std::vector<TargetView> views(B);
    for (int b = 0; b < B; b++) views[b] = target_view(targets[b]);
    HGS_HIP(h, h->group_tviews.reserve((size_t)B * sizeof(TargetView)));
    HGS_HIP(h, h->up.upload(h->group_tviews.p, views.data(), (size_t)B * sizeof(TargetView), h->stream));
  }
  BatchShape s;
  HGS_TRY(batch_shape(h, sources, true, &s, voxel ? corr_of.data() : nullptr));
  s.d_vviews = h->group_vviews.as<NdtTargetView>();
  s.d_tviews = fit_max_range ? h->group_tviews.as<TargetView>() : nullptr;
  HGS_HIP(h, h->guesses.reserve((size_t)B * 16 * sizeof(float)));
  HGS_HIP(h, h->up.upload(h->guesses.p, guesses_host, (size_t)B * 16 * sizeof(float), h->stream));
  HGS_HIP(h, h->results.reserve((size_t)B * sizeof(DevResult)));
  HGS_HIP(h, h->partials.reserve((size_t)B * s.max_blocks * kAccNdt * sizeof(double)));
  HGS_HIP(h, h->partials_err.reserve((size_t)B * s.max_blocks * 2 * sizeof(double)));
  if (voxel) HGS_TRY(run_gicp_rounds(h, s, guesses_host, false, fit_max_range));
  else HGS_TRY(run_ndt_rounds(h, sources, s, fit_max_range));
  HGS_HIP(h, hipGetLastError());
  return HGS_OK;
}

// fitness of B sources against the target with the poses stored in h->results[b].T; fills fit_sum / fit_count
// use_corr_seeds: the sources' corr[] hold their correspondences against THIS target (hgs_fitness right behind a GICP align); otherwise the
// searches start from the target's seed grid
int run_fitness(hgs_handle* h, const std::vector<hgs_cloud*>& sources, double max_range, bool use_corr_seeds) {
  std::vector<hgs_cloud*> all(sources);
  all.push_back(h->target);
  HGS_TRY(ensure_index(h, all));
  if (!use_corr_seeds) HGS_TRY(ensure_seed_grid(h, h->target));
  BatchShape s;
  HGS_TRY(batch_shape(h, sources, false, &s));
  HGS_HIP(h, h->partials_err.reserve((size_t)s.B * s.max_blocks * 2 * sizeof(double)));
  BatchLane whole;  // every problem on the engine's stream
  whole.stream = h->stream, whole.B = s.B, whole.partials_err = h->partials_err.as<double>();
  lane_fitness(h, whole, s, max_range, use_corr_seeds);
  HGS_HIP(h, hipGetLastError());
  return HGS_OK;
}

int fetch_results(hgs_handle* h, int B, std::vector<DevResult>& out) {
  HGS_HIP(h, h->h_results.reserve((size_t)B * sizeof(DevResult)));
  HGS_HIP(h, hipMemcpyAsync(h->h_results.p, h->results.p, (size_t)B * sizeof(DevResult), hipMemcpyDeviceToHost, h->stream));
  HGS_HIP(h, hipStreamSynchronize(h->stream));
  out.assign(h->h_results.as<DevResult>(), h->h_results.as<DevResult>() + B);
  if ((int)h->batch_order.size() == B)  // an ordered batch (run_batch): back to the caller's order
    for (int i = 0; i < B; i++) out[h->batch_order[i]] = h->h_results.as<DevResult>()[i];
  return HGS_OK;
}

// pcl::Registration::getFitnessScore: the mean squared distance of the inliers, DBL_MAX without any
double fitness_score(const DevResult& d) { return d.fit_count > 0 ? d.fit_sum / (double)d.fit_count : std::numeric_limits<double>::max(); }

// hgs_calc_fitness_score_batch: pair i scores cloud2[i], moved by relposes[i], against the tree of cloud1[i] — every edge of a graph update
// (hdl_graph_slam_nodelet.cpp:235,569) in one chain: one index build and one seed-grid build over the clouds that lack them, then per chunk of pairs
// one upload each of the target views, the descriptors and the poses, k_fitness<const TargetView*> + k_fitness_final, one copy back and one
// synchronisation.  No pair reads corr[] (use_seed = 0), so a cloud may repeat in any role; neither h->target nor h->source is read or written.
int run_pair_fitness(hgs_handle* h, hgs_cloud* const* cloud1, hgs_cloud* const* cloud2, const float* relposes, size_t n_pairs, double max_range,
                     std::vector<DevResult>& out) {
  std::vector<hgs_cloud*> all(cloud2, cloud2 + n_pairs);
  all.insert(all.end(), cloud1, cloud1 + n_pairs);
  HGS_TRY(ensure_index(h, all));
  HGS_TRY(ensure_seed_grids(h, std::vector<hgs_cloud*>(cloud1, cloud1 + n_pairs)));
  const size_t chunk = h->pair_chunk > 0 ? (size_t)h->pair_chunk : 65535;  // grid.y of one launch
  out.clear();
  out.reserve(n_pairs);
  for (size_t p0 = 0; p0 < n_pairs; p0 += chunk) {
    const size_t B = std::min(chunk, n_pairs - p0);
    std::vector<TargetView> views(B);
    for (size_t b = 0; b < B; b++) views[b] = target_view(cloud1[p0 + b]);
    HGS_HIP(h, h->group_tviews.reserve(B * sizeof(TargetView)));
    HGS_HIP(h, h->up.upload(h->group_tviews.p, views.data(), B * sizeof(TargetView), h->stream));
    BatchShape s;
    HGS_TRY(batch_shape(h, std::vector<hgs_cloud*>(cloud2 + p0, cloud2 + p0 + B), false, &s));
    s.d_tviews = h->group_tviews.as<TargetView>();
    std::vector<DevResult> poses(B);
    std::memset(poses.data(), 0, B * sizeof(DevResult));
    for (size_t b = 0; b < B; b++) std::memcpy(poses[b].T, relposes + 16 * (p0 + b), sizeof(float) * 16);
    HGS_HIP(h, h->results.reserve(B * sizeof(DevResult)));
    h->batch_order.clear();
    HGS_HIP(h, h->up.upload(h->results.p, poses.data(), B * sizeof(DevResult), h->stream));
    HGS_HIP(h, h->partials_err.reserve(B * s.max_blocks * 2 * sizeof(double)));
    BatchLane whole;  // every pair of the chunk on the engine's stream
    whole.stream = h->stream, whole.B = (int)B, whole.partials_err = h->partials_err.as<double>();
    lane_fitness(h, whole, s, max_range, false);
    HGS_HIP(h, hipGetLastError());
    std::vector<DevResult> r;
    HGS_TRY(fetch_results(h, (int)B, r));
    out.insert(out.end(), r.begin(), r.end());
  }
  return HGS_OK;
}

void to_public(const DevResult& d, int candidate, bool with_fitness, hgs_result* r) {
  std::memcpy(r->final_transformation, d.T, sizeof(float) * 16);
  r->converged = d.converged;
  r->iterations = d.iterations;
  r->error = d.error;
  r->lm_tries = d.lm_tries;
  r->candidate_id = candidate;
  r->reserved = 0;
  if (with_fitness) {
    r->num_inliers = d.fit_count;
    r->fitness_score = fitness_score(d);
  } else {
    r->num_inliers = 0;
    r->fitness_score = std::numeric_limits<double>::quiet_NaN();
  }
}

int upload_pose_as_result(hgs_handle* h, const float T[16]) {
  h->batch_order.clear();
  HGS_HIP(h, h->results.reserve(sizeof(DevResult)));
  HGS_HIP(h, h->h_results.reserve(sizeof(DevResult)));
  DevResult* r = h->h_results.as<DevResult>();
  std::memset(r, 0, sizeof(DevResult));
  std::memcpy(r->T, T, sizeof(float) * 16);
  HGS_HIP(h, hipMemcpyAsync(h->results.p, r, sizeof(DevResult), hipMemcpyHostToDevice, h->stream));
  return HGS_OK;
}

// The C-ABI never lets a C++ exception escape into PCL / ROS frames (include/hgs_registration.h): every entry point is a
// function-try-block whose handler ends here.  Called from inside a catch (...) handler.
int status_of_current_exception(hgs_handle* h) noexcept {
  int rc = HGS_ERR_INTERNAL;
  char what[256] = "unknown C++ exception inside the backend";
  try {
    throw;
  } catch (const std::bad_alloc&) {
    rc = HGS_ERR_OUT_OF_MEMORY;
    snprintf(what, sizeof(what), "out of host memory");
  } catch (const std::exception& e) {
    snprintf(what, sizeof(what), "C++ exception inside the backend: %s", e.what());
  } catch (...) {
  }
  try {
    if (h) h->err = what;
    else g_create_error = what;
  } catch (...) {
  }
  return rc;
}

// hgs_set_target / hgs_set_source and their _cloud forms: `role` is the engine's target or source, `own` whether the engine frees it
int set_role_cloud(hgs_handle* h, hgs_cloud* c, hgs_cloud* hgs_handle::*role, bool hgs_handle::*own) {
  ApiLock lock(h);
  if (!h || !c || c->owner != h) return HGS_ERR_INVALID_ARGUMENT;  // clouds belong to the engine (stream) that created them
  if (h->*own && h->*role != c) cloud_free(h->*role);
  h->*role = c;
  h->*own = false;
  return HGS_OK;
}
int set_role_points(hgs_handle* h, const void* pts, size_t n, size_t stride_bytes, hgs_cloud* hgs_handle::*role, bool hgs_handle::*own) {
  ApiLock lock(h);
  if (!h) return HGS_ERR_INVALID_ARGUMENT;
  hgs_cloud* c = nullptr;
  HGS_TRY(hgs_cloud_create(h, pts, n, stride_bytes, &c));
  if (h->*own) cloud_free(h->*role);  // (its block is reused in stream order, or freed by hipFree, which waits by itself)
  h->*role = c;
  h->*own = true;
  return HGS_OK;
}

}  // namespace

// Everything the engine holds goes here, and only here (hgs_destroy, and hgs_create when it fails half way).  The buffers, rings and pooled blocks free
// themselves once this body is through (hgs_resources.h); what it spells out is the order that matters.
hgs_handle::~hgs_handle() {
  (void)hipSetDevice(device);  // first: one process may hold engines on several GPUs
  synchronize_streams();       // nothing below is still being read by a queued kernel or copy
  pack_pool.shutdown();        // the workers write into pinned memory (up_big, h_xform) that the members' destructors free
  if (comm) hgs::comm_destroy(comm);
  for (hipEvent_t ev : lane_event)
    if (ev) (void)hipEventDestroy(ev);
  for (hipEvent_t ev : {comm_event, early_event, up_big_event})
    if (ev) (void)hipEventDestroy(ev);
  for (const std::vector<ProfEvent>* list : {&prof_events, &prof_free})
    for (const ProfEvent& ev : *list) (void)hipEventDestroy(ev.a), (void)hipEventDestroy(ev.b);
  for (hipStream_t ls : lane_stream)
    if (ls) (void)hipStreamDestroy(ls), streams_in_use(device).fetch_sub(1, std::memory_order_relaxed);  // (counted where each was created: open_lanes,
  for (hipStream_t ls : prio_stream)
    if (ls) (void)hipStreamDestroy(ls), streams_in_use(device).fetch_sub(1, std::memory_order_relaxed);
  if (stream) (void)hipStreamDestroy(stream), streams_in_use(device).fetch_sub(1, std::memory_order_relaxed);  //  hgs_create)
}

// =================================================================================================== C ABI
extern "C" {

int hgs_abi_version(void) { return HGS_ABI_VERSION; }

// Measurement / test knobs of one engine (A/B runs, tests that force a code path).  Rounds 1-5 read them from the environment in hgs_create; a plugin
// should not — the library now reads GPU_MAX_HW_QUEUES (HIP's own variable), HGS_COMM_TIMEOUT_MS and HGS_TRACE only.  The Python harness maps
// HGS_ENGINE_OPTIONS="key=value,..." onto this call (hdl_graph_slam_amd/registration.py); nothing in adapters/ uses it.
int hgs_debug_set_option(hgs_handle* h, const char* key, int value) try {
  ApiLock lock(h);
  if (!h || !key) return HGS_ERR_INVALID_ARGUMENT;
  const std::string k(key);
  if (k == "batch_lanes") h->batch_lanes = value <= 0 ? 0 : std::min(kMaxLanes, value);                  // 0: open_lanes chooses
  else if (k == "lane_start") h->lane_start = value != 0 ? 1 : 0;
  else if (k == "lane_order") h->lane_order = value != 0 ? 1 : 0;
  else if (k == "ndt_sort") h->ndt_sort = std::max(-1, std::min(1, value));
  else if (k == "cov_split") h->cov_split = value != 0 ? 1 : 0;
  else if (k == "fused_rounds") h->fused_rounds = value != 0 ? 1 : 0;
  else if (k == "early_result") h->early_result = value != 0 ? 1 : 0;
  else if (k == "early_run_ahead") h->early_run_ahead = std::max(1, std::min(8, value));
  else if (k == "fused_rounds_max_problems") h->fused_rounds_max_problems = std::max(0, value);
  else if (k == "fused_rounds_max_blocks") h->fused_rounds_max_blocks = std::max(0, value);
  else if (k == "fused_rounds_below") h->fused_rounds_below = std::max(0, value);
  else if (k == "resident_descs") h->resident_descs = value != 0 ? 1 : 0;
  else if (k == "knn_qpw_tiny") h->knn_qpw_tiny = value < 0 ? -1 : std::max(0, std::min(32, value & ~7));
  else if (k == "knn_tiny_below") h->knn_tiny_below = std::max(0, value);
  else if (k == "seed_grid") h->seed_grid = value != 0 ? 1 : 0;
  else if (k == "knn_replay") h->knn_replay = std::max(-1, std::min(2, value));                           // -1: the engine chooses
  else if (k == "ndt_resident") h->ndt_resident_blocks = std::max(0, value);
  else if (k == "ndt_chunk") h->ndt_chunk = std::max(0, value);
  else if (k == "hilbert_levels") h->hilbert_levels = std::max(4, std::min(16, value));
  else if (k == "nn_qpw") h->nn_qpw = value == 16 ? 16 : (value == 32 ? 32 : (value == 64 ? 64 : 0));
  else if (k == "nn_qpw16_below") h->nn_qpw16_below = std::max(0, value);
  else if (k == "nn_qpw32_below") h->nn_qpw32_below = std::max(0, value);
  else if (k == "upload_trace") h->upload_trace = value != 0 ? 1 : 0;
  else if (k == "prefilter_fast") h->prefilter_fast = value != 0 ? 1 : 0;
  else if (k == "prefilter_batch_tree") h->prefilter_batch_tree = value != 0 ? 1 : 0;
  else if (k == "floor_chunk") h->floor_chunk = std::max(1, std::min(kFloorMaxChunk, value));
  else if (k == "floor_batch_group") h->floor_batch_group = std::max(0, value);                            // 0: what the work buffers allow
  else if (k == "pair_chunk") h->pair_chunk = std::max(0, std::min(65535, value));                         // 0: what one launch holds
  else {
    h->err = "hgs_debug_set_option: unknown option '" + k + "'";
    return HGS_ERR_INVALID_ARGUMENT;
  }
  return HGS_OK;
} catch (...) {
  return status_of_current_exception(h);
}

int hgs_debug_lane_plan(hgs_handle* h, int32_t* lanes, int32_t* ahead_lanes, int32_t* process_streams) try {
  ApiLock lock(h);
  if (!h) return HGS_ERR_INVALID_ARGUMENT;
  if (lanes) *lanes = h->last_lanes;
  if (ahead_lanes) *ahead_lanes = h->last_ahead_lanes;
  if (process_streams) *process_streams = streams_in_use(h->device).load(std::memory_order_relaxed);
  return HGS_OK;
} catch (...) {
  return status_of_current_exception(h);
}

int hgs_debug_plan_lanes(hgs_handle* h, int32_t n_problems, int32_t tiles_per_problem, int32_t ordered, int32_t assume_streams, int32_t* lanes, int32_t* ahead_lanes) try {
  ApiLock lock(h);
  if (!h || n_problems < 1) return HGS_ERR_INVALID_ARGUMENT;
  const LanePlan plan = plan_lanes(h, n_problems, tiles_per_problem, ordered != 0 && h->lane_order && n_problems >= kLaneOrderMinProblems, assume_streams);
  if (lanes) *lanes = plan.lanes;
  if (ahead_lanes) *ahead_lanes = plan.ahead;
  return HGS_OK;
} catch (...) {
  return status_of_current_exception(h);
}

int hgs_debug_batch_order(hgs_handle* h, int32_t* order, int32_t cap, int32_t* n) try {
  ApiLock lock(h);
  if (!h || !n || cap < 0 || (cap > 0 && !order)) return HGS_ERR_INVALID_ARGUMENT;
  *n = (int32_t)h->batch_order.size();
  for (int32_t i = 0; i < std::min(cap, *n); i++) order[i] = h->batch_order[i];
  return HGS_OK;
} catch (...) {
  return status_of_current_exception(h);
}

int hgs_params_default(int32_t method, hgs_params* p) try {
  if (!p || method < HGS_FAST_GICP || method > HGS_ICP) return HGS_ERR_INVALID_ARGUMENT;
  std::memset(p, 0, sizeof(*p));
  p->method = method;
  p->max_iterations = 64;                 // reg_maximum_iterations            registrations.cpp:32,54,110
  p->transformation_epsilon = 0.01;       // reg_transformation_epsilon        registrations.cpp:31,53,109
  p->rotation_epsilon = method == HGS_ICP ? 0.0 : 2e-3;  // fast_gicp LsqRegistration default; ICP: hdl never sets it (threshold 1 - transformation_epsilon)
  p->max_correspondence_distance = method == HGS_FAST_GICP || method == HGS_ICP ? 2.5 : (double)FLT_MAX;  // registrations.cpp:33,61 (VGICP: not set)
  p->correspondence_randomness = 20;      // reg_correspondence_randomness     registrations.cpp:34,55
  p->neighbor_search = method == HGS_NDT_OMP ? HGS_DIRECT7 : HGS_DIRECT1;  // registrations.cpp:103
  p->resolution = method == HGS_NDT_OMP ? 0.5 : 1.0;                        // registrations.cpp:93 / :52
  p->ndt_step_size = 0.1;
  p->ndt_outlier_ratio = 0.55;
  p->ndt_min_points_per_voxel = 6;
  p->ndt_upstream_hd1_sign = 1;
  p->lm_max_iterations = 10;
  p->lm_init_lambda_factor = 1e-9;
  p->device_id = 0;
  p->regularization_method = HGS_REG_FROBENIUS;  // fast_gicp constructor default; hdl never calls the setter
  p->ndt_line_search = 0;                        // ndt_omp as it runs
  p->icp_reciprocal = 0;                         // reg_use_reciprocal_correspondences  registrations.cpp:63
  return HGS_OK;
} catch (...) {
  return status_of_current_exception(nullptr);
}

int hgs_create(const hgs_params* p, hgs_handle** out) try {
  if (!p || !out) return HGS_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  if (p->method < HGS_FAST_GICP || p->method > HGS_ICP || p->max_iterations < 0 || p->correspondence_randomness < 1 || p->correspondence_randomness > 64 /* k_knn_cov's largest list */ || !(p->resolution > 0) ||
      p->regularization_method < HGS_REG_FROBENIUS || p->regularization_method > HGS_REG_NONE) {
    g_create_error = "invalid hgs_params";
    return HGS_ERR_INVALID_ARGUMENT;
  }
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0 || p->device_id < 0 || p->device_id >= ndev) {
    g_create_error = std::string("no usable HIP device: ") + (e != hipSuccess ? hipGetErrorString(e) : "device ordinal out of range");
    return HGS_ERR_NO_DEVICE;
  }
  hgs_handle* h = new hgs_handle();
  h->prm = *p;
  h->device = p->device_id;
  for (int i = 0; i < 16; i++) h->final_T[i] = (i % 5 == 0) ? 1.f : 0.f;
  for (int i = 0; i < HGS_STAGE_COUNT; i++) h->prof_ms[i] = 0, h->prof_launches[i] = 0;
  // (measurement / test knobs: hgs_debug_set_option below — the library reads no tuning variable from the environment)
  if (hipSetDevice(h->device) != hipSuccess || hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
    g_create_error = "hipSetDevice / hipStreamCreate failed";
    delete h;
    return HGS_ERR_HIP;
  }
  streams_in_use(h->device).fetch_add(1, std::memory_order_relaxed);
  *out = h;
  return HGS_OK;
} catch (...) {
  return status_of_current_exception(nullptr);
}

int hgs_destroy(hgs_handle* h) try {
  if (!h) return HGS_OK;
  // a call still running on another thread finishes first; a call that STARTS after this line races with the deletion below —
  // hgs_destroy must not be called concurrently with other calls on the engine or its clouds (include/hgs_registration.h)
  { std::lock_guard<std::recursive_mutex> wait_for_running_call(h->api_mutex); }
  (void)hipSetDevice(h->device);
  h->synchronize_streams();
  if (h->own_target) cloud_free(h->target);
  if (h->own_source) cloud_free(h->source);
  // clouds the caller still holds (hgs_cloud_create / hgs_prefilter results, cached keyframes): their device memory goes with
  // the engine, the structs stay valid as orphans — hgs_cloud_destroy frees them, every other call rejects them
  for (hgs_cloud* c : h->live_clouds) {
    cloud_release_device(c, false);
    c->owner = nullptr;
    c->n_input = 0;
  }
  delete h;
  return HGS_OK;
} catch (...) {
  return status_of_current_exception(nullptr);
}

const char* hgs_last_error(const hgs_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int hgs_cloud_create(hgs_handle* h, const void* pts, size_t n, size_t stride_bytes, hgs_cloud** out) try {
  ApiLock lock(h);
  if (!h || !out || (n > 0 && !pts) || stride_bytes < 12 || (stride_bytes % 4) != 0 || n > (size_t)1 << 30) return HGS_ERR_INVALID_ARGUMENT;
  HGS_TRY(set_device(h));
  const bool trace = h->upload_trace != 0;  // host-side phase times of an upload on stderr (diagnostics: hgs_debug_set_option "upload_trace")
  const auto t0 = std::chrono::steady_clock::now();
  hgs_cloud* c = nullptr;
  HGS_TRY(cloud_alloc(h, n, &c));
  const auto t1 = std::chrono::steady_clock::now();
  auto t2 = t1;
  {
    StageTimer tm(h, HGS_STAGE_UPLOAD);
    const float4* staged = nullptr;
    {
      const int rc = upload_points_packed(h, pts, n, stride_bytes, &staged);
      t2 = std::chrono::steady_clock::now();
      if (rc != HGS_OK) {
        cloud_free(c);
        return rc;
      }
    }
    const CloudDesc resident = resident_desc(c);
    launch_pack_aos(h->stream, staged, (int)n, const_cast<float4*>(c->desc.raw), c->intensity, c->desc.meta, &resident, c->dev_desc);  // (n == 0: the meta reset + descriptor alone)
    // nvalid + bounding box of the finite points
    launch_bbox_count(h->stream, c->dev_desc, 1, (int)n);  // (the meta record was reset and the descriptor written by the packing kernel)
    hipError_t e = hipGetLastError();
    // (no synchronisation: the caller's buffer was read by the host while packing; everything else is ordered on the stream)
    if (e != hipSuccess) {
      h->err = std::string("cloud upload failed: ") + hipGetErrorString(e);
      cloud_free(c);
      return HGS_ERR_HIP;
    }
  }
  if (trace) {
    const auto t3 = std::chrono::steady_clock::now();
    auto us = [](auto a, auto b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
    std::fprintf(stderr, "[hgs upload] n %zu: alloc %.1f us, pack + DMA enqueue %.1f us, launches %.1f us\n", n, us(t0, t1), us(t1, t2), us(t2, t3));
  }
  *out = c;
  return HGS_OK;
} catch (...) {
  return status_of_current_exception(h);
}

int hgs_cloud_destroy(hgs_cloud* c) try {
  ApiLock lock(c);
  if (!c) return HGS_OK;
  hgs_handle* h = c->owner;
  if (h) {
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    if (h->target == c) h->target = nullptr, h->own_target = false;
    if (h->source == c) h->source = nullptr, h->own_source = false;
  }
  cloud_free(c);
  c = nullptr;  // gone: the handler below must not look at it
  return HGS_OK;
} catch (...) {
  return status_of_current_exception(nullptr);
}

size_t hgs_cloud_size(const hgs_cloud* c) { return c ? c->n_input : 0; }

size_t hgs_cloud_device_bytes(const hgs_cloud* c) {
  if (!c || !c->owner) return 0;
  return c->block.cap + c->ndt.block.cap + c->vg.block.cap + c->seed_block.cap;
}

int hgs_cloud_invalidate(hgs_cloud* c) try {
  ApiLock lock(c);
  if (!c) return HGS_ERR_INVALID_ARGUMENT;
  c->has_index = false, c->has_cov = false, c->has_ndt = false, c->has_vg = false, c->has_seed = false;
  // also forget the correspondences of earlier registrations (they seed the next search): a truly cold cloud.  No launch here — 65
  // memsets per loop-closure batch were 65 launches of ~3 us —: the kernel that rebuilds the cloud's sorted arrays clears them
  // (a cloud without an index cannot be searched before ensure_index has run).
  c->corr_stale = true;
  return HGS_OK;
} catch (...) {
  return status_of_current_exception((c ? c->owner : nullptr));
}

int hgs_set_target_cloud(hgs_handle* h, hgs_cloud* c) try {
  return set_role_cloud(h, c, &hgs_handle::target, &hgs_handle::own_target);
} catch (...) {
  return status_of_current_exception(h);
}
int hgs_set_source_cloud(hgs_handle* h, hgs_cloud* c) try {
  return set_role_cloud(h, c, &hgs_handle::source, &hgs_handle::own_source);
} catch (...) {
  return status_of_current_exception(h);
}
int hgs_set_target(hgs_handle* h, const void* pts, size_t n, size_t stride_bytes) try {
  return set_role_points(h, pts, n, stride_bytes, &hgs_handle::target, &hgs_handle::own_target);
} catch (...) {
  return status_of_current_exception(h);
}
int hgs_set_source(hgs_handle* h, const void* pts, size_t n, size_t stride_bytes) try {
  return set_role_points(h, pts, n, stride_bytes, &hgs_handle::source, &hgs_handle::own_source);
} catch (...) {
  return status_of_current_exception(h);
}

int hgs_align(hgs_handle* h, const float guess[16], hgs_result* out) try {
  ApiLock lock(h);
  if (!h || !guess || !out) return HGS_ERR_INVALID_ARGUMENT;
  if (!h->target) return HGS_ERR_NO_TARGET;
  if (!h->source) return HGS_ERR_NO_SOURCE;
  HGS_TRY(set_device(h));
  std::vector<hgs_cloud*> src{h->source};
  HGS_TRY(run_batch(h, src, guess));
  std::vector<DevResult> r;
  if (h->early_valid) r.assign(1, *h->h_early.as<DevResult>());  // (written in front of the `done` flag the poll has seen: k_gicp_linearize<true>)
  else HGS_TRY(fetch_results(h, 1, r));
  h->early_valid = false;
  to_public(r[0], 0, false, out);
  std::memcpy(h->final_T, out->final_transformation, sizeof(h->final_T));
  return HGS_OK;
} catch (...) {
  return status_of_current_exception(h);
}

int hgs_transform_source(hgs_handle* h, const float T[16], void* out_pts, size_t stride_bytes) try {
  ApiLock lock(h);
  if (!h || !T || !out_pts || stride_bytes < 12) return HGS_ERR_INVALID_ARGUMENT;
  if (!h->source) return HGS_ERR_NO_SOURCE;
  HGS_TRY(set_device(h));
  const size_t n = h->source->n_input;
  if (n == 0) return HGS_OK;
  HGS_HIP(h, h->misc.reserve(n * sizeof(float4) + 256));
  HGS_HIP(h, h->h_small.reserve(64));
  float* dT = reinterpret_cast<float*>((char*)h->misc.p + n * sizeof(float4));
  std::memcpy(h->h_small.p, T, 64);
  HGS_HIP(h, hipMemcpyAsync(dT, h->h_small.p, 64, hipMemcpyHostToDevice, h->stream));
  launch_transform(h->stream, h->source->desc.raw, (int)n, dT, h->misc.as<float4>());
  // Down through a pinned staging buffer the engine keeps (round 4 copied into a fresh pageable std::vector: 1.9 MB of page faults and a staged
  // pageable D2H per align): one copy, then the scatter into the caller's strided records — for a large cloud a write-allocate pass over 3.8 MB, spread
  // over the pack pool's threads.  (Four overlapped pieces with an event each were tried first: at 13 k points their API calls cost more than they hid.)
  HGS_HIP(h, h->h_xform.reserve(n * sizeof(float4)));
  const float* host = h->h_xform.as<float>();
  char* o = (char*)out_pts;
  HGS_HIP(h, hipMemcpyAsync(h->h_xform.p, h->misc.p, n * sizeof(float4), hipMemcpyDeviceToHost, h->stream));
  HGS_HIP(h, hipStreamSynchronize(h->stream));
  const size_t nchunks = (n + kUploadChunkPoints - 1) / kUploadChunkPoints;
  std::vector<std::atomic<unsigned char>> ready(nchunks);
  for (auto& r : ready) r.store(0, std::memory_order_relaxed);
  PackPool::Job job;
  job.src = reinterpret_cast<const char*>(host), job.dst = reinterpret_cast<float*>(o), job.n = n, job.stride = stride_bytes, job.chunk = kUploadChunkPoints;
  job.nchunks = nchunks, job.scatter = true, job.ready = ready.data();
  if (n >= kUploadParallelPoints) {
    h->pack_pool.post(&job);
    while (PackPool::help(job)) {
    }
    h->pack_pool.retire();  // every chunk has been taken, and nobody is inside the job any more: all of them are done
  } else {
    while (PackPool::help(job)) {  // a small cloud: this thread alone
    }
  }
  return HGS_OK;
} catch (...) {
  return status_of_current_exception(h);
}

int hgs_fitness(hgs_handle* h, const float T[16], double max_range, double* score, uint32_t* num_inliers) try {
  ApiLock lock(h);
  if (!h || !T || !score) return HGS_ERR_INVALID_ARGUMENT;
  if (!h->target) return HGS_ERR_NO_TARGET;
  if (!h->source) return HGS_ERR_NO_SOURCE;
  HGS_TRY(set_device(h));
  HGS_TRY(upload_pose_as_result(h, T));
  std::vector<hgs_cloud*> src{h->source};
  HGS_TRY(run_fitness(h, src, max_range, corr_seeds_fitness(h->prm.method)));
  std::vector<DevResult> r;
  HGS_TRY(fetch_results(h, 1, r));
  *score = fitness_score(r[0]);
  if (num_inliers) *num_inliers = r[0].fit_count;
  return HGS_OK;
} catch (...) {
  return status_of_current_exception(h);
}

int hgs_calc_fitness_score(hgs_handle* h, hgs_cloud* cloud1, hgs_cloud* cloud2, const float relpose[16], double max_range, double* score) try {
  ApiLock lock(h);
  if (!h || !cloud1 || !cloud2 || cloud1->owner != h || cloud2->owner != h || !relpose || !score) return HGS_ERR_INVALID_ARGUMENT;
  HGS_TRY(set_device(h));
  hgs_cloud* saved_t = h->target;
  h->target = cloud1;
  int rc = upload_pose_as_result(h, relpose);
  std::vector<hgs_cloud*> src{cloud2};
  if (rc == HGS_OK) rc = run_fitness(h, src, max_range, false);  // two keyframe clouds: cloud2 holds no correspondences against cloud1
  std::vector<DevResult> r;
  if (rc == HGS_OK) rc = fetch_results(h, 1, r);
  h->target = saved_t;
  if (rc != HGS_OK) return rc;
  *score = fitness_score(r[0]);
  return HGS_OK;
} catch (...) {
  return status_of_current_exception(h);
}

// Every edge of a graph update in one device batch (flush_keyframe_queue's odometry edges, hdl_graph_slam_nodelet.cpp:235, and the loop edges of :569).
int hgs_calc_fitness_score_batch(hgs_handle* h, hgs_cloud* const* cloud1, hgs_cloud* const* cloud2, const float* relposes, size_t n_pairs, double max_range,
                                 double* scores, uint32_t* num_inliers) try {
  ApiLock lock(h);
  if (!h) return HGS_ERR_INVALID_ARGUMENT;
  if (n_pairs == 0) return HGS_OK;
  if (!cloud1 || !cloud2 || !relposes || !scores) return HGS_ERR_INVALID_ARGUMENT;
  for (size_t i = 0; i < n_pairs; i++)  // (an orphaned cloud has no owner)
    if (!cloud1[i] || !cloud2[i] || cloud1[i]->owner != h || cloud2[i]->owner != h) return HGS_ERR_INVALID_ARGUMENT;
  HGS_TRY(set_device(h));
  std::vector<DevResult> r;
  HGS_TRY(run_pair_fitness(h, cloud1, cloud2, relposes, n_pairs, max_range, r));
  for (size_t i = 0; i < n_pairs; i++) {
    scores[i] = fitness_score(r[i]);
    if (num_inliers) num_inliers[i] = r[i].fit_count;
  }
  return HGS_OK;
} catch (...) {
  return status_of_current_exception(h);
}

int hgs_nn_target(hgs_handle* h, const float* q_xyz, size_t nq, size_t stride_bytes, int32_t* idx, float* d2) try {
  ApiLock lock(h);
  if (!h || (nq > 0 && (!q_xyz || !idx || !d2)) || stride_bytes < 12) return HGS_ERR_INVALID_ARGUMENT;
  if (!h->target) return HGS_ERR_NO_TARGET;
  if (nq == 0) return HGS_OK;
  HGS_TRY(set_device(h));
  std::vector<hgs_cloud*> all{h->target};
  HGS_TRY(ensure_index(h, all));
  HGS_HIP(h, h->misc.reserve(nq * (sizeof(float4) + 8) + 512));
  float4* dq = h->misc.as<float4>();
  int* didx = reinterpret_cast<int*>((char*)h->misc.p + align_up(nq * sizeof(float4), 256));
  float* dd2 = reinterpret_cast<float*>(didx + nq);
  const float4* staged = nullptr;
  HGS_TRY(upload_points_packed(h, q_xyz, nq, stride_bytes, &staged));
  launch_pack_aos(h->stream, staged, (int)nq, dq, nullptr, nullptr);
  launch_nn_query(h->stream, target_view(h->target), dq, (int)nq, didx, dd2);
  // the two result arrays come down in ONE copy into pinned memory (they are adjacent on the device: didx[nq] | dd2[nq]) and are handed to the
  // caller's (pageable) arrays from there
  HGS_HIP(h, h->h_xform.reserve(nq * 8));
  HGS_HIP(h, hipMemcpyAsync(h->h_xform.p, didx, nq * 8, hipMemcpyDeviceToHost, h->stream));
  HGS_HIP(h, hipStreamSynchronize(h->stream));
  std::memcpy(idx, h->h_xform.p, nq * sizeof(int));
  std::memcpy(d2, static_cast<const char*>(h->h_xform.p) + nq * sizeof(int), nq * sizeof(float));
  return HGS_OK;
} catch (...) {
  return status_of_current_exception(h);
}

int hgs_select_best(const hgs_result* records, size_t n, int32_t* best) try {
  if (!best || (n > 0 && !records)) return HGS_ERR_INVALID_ARGUMENT;
  // loop_detector.hpp:124,146-153: best_score starts at DBL_MAX; skip if !converged || score > best_score; else replace
  double best_score = std::numeric_limits<double>::max();
  int32_t b = -1;
  for (size_t i = 0; i < n; i++) {
    const double score = records[i].fitness_score;
    if (!records[i].converged || score > best_score || score != score) continue;
    best_score = score;
    b = (int32_t)i;
  }
  *best = b;
  return HGS_OK;
} catch (...) {
  return status_of_current_exception(nullptr);
}

int hgs_loop_match_batch(hgs_handle* h, hgs_cloud* const* candidates, size_t n_candidates, const float* guesses, double max_range, hgs_result* out,
                         int32_t* best) try {
  ApiLock lock(h);
  if (!h || (n_candidates > 0 && (!candidates || !guesses || !out))) return HGS_ERR_INVALID_ARGUMENT;
  if (!h->target) return HGS_ERR_NO_TARGET;
  if (best) *best = -1;
  if (n_candidates == 0) return HGS_OK;
  HGS_TRY(set_device(h));
  std::vector<hgs_cloud*> src(candidates, candidates + n_candidates);
  for (hgs_cloud* c : src)
    if (!c || c->owner != h) return HGS_ERR_INVALID_ARGUMENT;
  {
    // every candidate carries its own correspondence scratch: the same cloud twice in one batch would race on it
    std::vector<hgs_cloud*> sorted(src);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) {
      h->err = "hgs_loop_match_batch: candidate clouds must be distinct";
      return HGS_ERR_INVALID_ARGUMENT;
    }
  }
  HGS_TRY(run_batch(h, src, guesses, &max_range));
  std::vector<DevResult> r;
  HGS_TRY(fetch_results(h, (int)n_candidates, r));
  for (size_t i = 0; i < n_candidates; i++) to_public(r[i], (int)i, true, &out[i]);
  if (best) HGS_TRY(hgs_select_best(out, n_candidates, best));
  return HGS_OK;
} catch (...) {
  return status_of_current_exception(h);
}

// LoopDetector::detect (loop_detector.hpp:57-68) calls matching once per new keyframe of a graph update; this is the candidates of ALL of them in one batch.
int hgs_loop_match_groups(hgs_handle* h, hgs_cloud* const* targets, size_t n_groups, const size_t* group_offsets, hgs_cloud* const* candidates, const float* guesses,
                          double max_range, hgs_result* out, int32_t* best) try {
  ApiLock lock(h);
  if (!h) return HGS_ERR_INVALID_ARGUMENT;
  if (n_groups == 0) return HGS_OK;
  if (!group_offsets || !targets || group_offsets[0] != 0) return HGS_ERR_INVALID_ARGUMENT;
  for (size_t g = 0; g < n_groups; g++)
    if (group_offsets[g + 1] < group_offsets[g]) {
      h->err = "hgs_loop_match_groups: group_offsets must not decrease";
      return HGS_ERR_INVALID_ARGUMENT;
    }
  const size_t n = group_offsets[n_groups];
  if (n > (size_t)INT_MAX || (n > 0 && (!candidates || !guesses || !out))) return HGS_ERR_INVALID_ARGUMENT;
  if (h->prm.method != HGS_FAST_GICP && h->prm.method != HGS_ICP) {
    h->err = "hgs_loop_match_groups: FAST_GICP and ICP only (one hgs_loop_match_batch per target serves the other methods)";
    return HGS_ERR_UNSUPPORTED;
  }
  std::vector<hgs_cloud*> tgt(n), src(candidates, candidates + n);
  for (size_t g = 0; g < n_groups; g++) {
    const size_t g0 = group_offsets[g], g1 = group_offsets[g + 1];
    if (best) best[g] = -1;
    if (g0 == g1) continue;  // (an empty group's target is not looked at)
    if (!targets[g] || targets[g]->owner != h) return HGS_ERR_INVALID_ARGUMENT;
    for (size_t i = g0; i < g1; i++) {
      if (!src[i] || src[i]->owner != h) return HGS_ERR_INVALID_ARGUMENT;
      tgt[i] = targets[g];
    }
    // as hgs_loop_match_batch: the candidates of ONE new keyframe are distinct keyframes (across groups a cloud may repeat)
    std::vector<hgs_cloud*> sorted(src.begin() + g0, src.begin() + g1);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) {
      h->err = "hgs_loop_match_groups: the candidate clouds of one group must be distinct";
      return HGS_ERR_INVALID_ARGUMENT;
    }
  }
  if (n == 0) return HGS_OK;
  HGS_TRY(set_device(h));
  HGS_TRY(run_group_batch(h, tgt, src, guesses, &max_range));
  std::vector<DevResult> r;
  HGS_TRY(fetch_results(h, (int)n, r));
  for (size_t g = 0; g < n_groups; g++) {
    const size_t g0 = group_offsets[g], g1 = group_offsets[g + 1];
    for (size_t i = g0; i < g1; i++) to_public(r[i], (int)(i - g0), true, &out[i]);
    if (best && g1 > g0) HGS_TRY(hgs_select_best(out + g0, g1 - g0, &best[g]));
  }
  return HGS_OK;
} catch (...) {
  return status_of_current_exception(h);
}

// n independent registrations in one batch, every engine: the primitive under the grouped call (repeat the target, select per group) and under several
// odometry streams in lock-step (one pair per sensor).
int hgs_align_pairs(hgs_handle* h, hgs_cloud* const* targets, hgs_cloud* const* sources, const float* guesses, const double* max_range, size_t n,
                    hgs_result* out) try {
  ApiLock lock(h);
  if (!h) return HGS_ERR_INVALID_ARGUMENT;
  if (n == 0) return HGS_OK;
  if (n > (size_t)INT_MAX || !targets || !sources || !guesses || !out) return HGS_ERR_INVALID_ARGUMENT;
  std::vector<hgs_cloud*> tgt(targets, targets + n), src(sources, sources + n);
  for (size_t i = 0; i < n; i++)
    if (!tgt[i] || !src[i] || tgt[i]->owner != h || src[i]->owner != h) return HGS_ERR_INVALID_ARGUMENT;
  HGS_TRY(set_device(h));
  HGS_TRY(run_pair_batch(h, tgt, src, guesses, max_range));
  std::vector<DevResult> r;
  if (h->early_valid) r.assign(1, *h->h_early.as<DevResult>());  // (one FAST_GICP pair without a fitness pass: handed over as hgs_align's result is)
  else HGS_TRY(fetch_results(h, (int)n, r));
  h->early_valid = false;
  for (size_t i = 0; i < n; i++) to_public(r[i], (int)i, max_range != nullptr, &out[i]);
  return HGS_OK;
} catch (...) {
  return status_of_current_exception(h);
}

// ---- multi-GPU: candidate-sharded loop-closure batch, one process per GPU ---------------------------------------
int hgs_comm_get_unique_id(void* id_out) try {
  if (!id_out) return HGS_ERR_INVALID_ARGUMENT;
  char err[256] = "";
  if (hgs::comm_unique_id(id_out, err, sizeof(err)) != 0) {
    g_create_error = err;
    return HGS_ERR_COMM;
  }
  return HGS_OK;
} catch (...) {
  return status_of_current_exception(nullptr);
}

int hgs_comm_init(hgs_handle* h, int32_t rank, int32_t world, const void* unique_id) try {
  ApiLock lock(h);
  if (!h || !unique_id || world < 1 || rank < 0 || rank >= world) return HGS_ERR_INVALID_ARGUMENT;
  HGS_TRY(set_device(h));
  if (h->comm) hgs::comm_destroy(h->comm), h->comm = nullptr;
  char err[256] = "";
  if (hgs::comm_create(&h->comm, rank, world, unique_id, h->device, err, sizeof(err)) != 0) {
    h->err = err;
    return HGS_ERR_COMM;
  }
  return HGS_OK;
} catch (...) {
  return status_of_current_exception(h);
}

int hgs_comm_finalize(hgs_handle* h) try {
  ApiLock lock(h);
  if (!h) return HGS_ERR_INVALID_ARGUMENT;
  if (h->comm) {
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    hgs::comm_destroy(h->comm);
    h->comm = nullptr;
  }
  return HGS_OK;
} catch (...) {
  return status_of_current_exception(h);
}

// Pure host code of the sharded batch: the gathered slots -> the n_total records of the detection.  `gathered` holds `world`
// blocks of `per` slots; of rank r's block the first counts[r] slots carry records, the rest is padding.  A candidate nobody
// reported stays "not converged" (fitness DBL_MAX); a candidate reported twice (two ranks, or twice by one) is an error of the
// caller's partition: *duplicate_id receives the id (else -1) and the first report is kept.
int hgs_debug_merge_shard_records(const hgs_result* gathered, const int32_t* counts, int32_t world, size_t per, size_t n_total, hgs_result* all_out,
                                  int32_t* duplicate_id) try {
  if (!all_out || n_total == 0 || world < 1 || (per > 0 && !gathered) || !counts) return HGS_ERR_INVALID_ARGUMENT;
  for (size_t i = 0; i < n_total; i++) {
    std::memset(&all_out[i], 0, sizeof(hgs_result));
    all_out[i].candidate_id = (int32_t)i;
    all_out[i].fitness_score = std::numeric_limits<double>::max();
  }
  std::vector<char> seen(n_total, 0);
  int32_t dup = -1;
  for (int32_t r = 0; r < world; r++) {
    const size_t n = counts[r] < 0 ? 0 : std::min<size_t>((size_t)counts[r], per);
    for (size_t k = 0; k < n; k++) {
      const hgs_result& rec = gathered[(size_t)r * per + k];
      if (rec.candidate_id < 0 || (size_t)rec.candidate_id >= n_total) continue;  // padding (a rank that failed after announcing its shard)
      if (seen[rec.candidate_id]) {
        if (dup < 0) dup = rec.candidate_id;
        continue;
      }
      seen[rec.candidate_id] = 1;
      all_out[rec.candidate_id] = rec;
    }
  }
  if (duplicate_id) *duplicate_id = dup;
  return HGS_OK;
} catch (...) {
  return status_of_current_exception(nullptr);
}

}  // extern "C"
namespace {
// Waits for something enqueued behind a collective (query = hipEventQuery / hipStreamQuery) WITHOUT an unbounded blocking call.  A rank that aborts
// its communicator only raises its own abort flag: on the intra-node transports (P2P / xGMI / shared memory) RCCL does not promise that the peers'
// all-gather kernel stops spinning, so hipEventSynchronize / hipStreamSynchronize behind it could wait forever.  The wait therefore polls, asks
// the communicator for an asynchronous error (ncclCommGetAsyncError) now and then, and gives up after the deadline (HGS_COMM_TIMEOUT_MS, default
// 60 s, 0 = none; it has to cover the skew with which the SLAM processes enter the detection, not the exchange itself, which is microseconds).
// On error or timeout this rank aborts ITS communicator (which ends its own stuck kernel) and the call returns HGS_ERR_COMM.
long comm_timeout_ms() {
  if (const char* e = std::getenv("HGS_COMM_TIMEOUT_MS")) return std::max(0l, std::atol(e));
  return 60000;
}
template <typename Q>
int comm_wait(hgs_handle* h, Q&& query, const char* what) {
  const long limit_ms = comm_timeout_ms();
  const auto t0 = std::chrono::steady_clock::now();
  auto next_check = t0 + std::chrono::milliseconds(1);
  long sleep_us = 0;  // spin for ~200 us, then sleep with exponential backoff up to 50 us: a rank waiting out peer skew must not burn the core that feeds the
                      // other lanes and engines, but this wait also sits behind the batch of EVERY sharded detection, where it overshoots by half its
                      // last sleep on average — hence 50 us and not the millisecond a pure skew wait could afford
  char err[256] = "";
  for (;;) {
    const hipError_t e = query();
    if (e == hipSuccess) return HGS_OK;
    if (e != hipErrorNotReady) {
      h->err = std::string("hgs_loop_match_batch_sharded: HIP error while waiting for ") + what + ": " + hipGetErrorString(e);
      hgs::comm_abort(h->comm);
      return HGS_ERR_HIP;
    }
    const auto now = std::chrono::steady_clock::now();
    if (now >= next_check) {  // time-based: once a millisecond, whatever the polling rate
      next_check = now + std::chrono::milliseconds(1);
      if (hgs::comm_async_error(h->comm, err, sizeof(err)) != 0) {
        h->err = std::string("hgs_loop_match_batch_sharded: the communicator reported an asynchronous error while waiting for ") + what + ": " + err;
        hgs::comm_abort(h->comm);
        return HGS_ERR_COMM;
      }
      const long waited = (long)std::chrono::duration_cast<std::chrono::milliseconds>(now - t0).count();
      if (limit_ms > 0 && waited > limit_ms) {
        h->err = std::string("hgs_loop_match_batch_sharded: gave up after ") + std::to_string(waited) + " ms waiting for " + what +
                 " (a peer has left the collective or never entered it); the communicator has been aborted";
        hgs::comm_abort(h->comm);
        return HGS_ERR_COMM;
      }
    }
    if (now - t0 > std::chrono::microseconds(200)) {
      sleep_us = sleep_us == 0 ? 5 : std::min(50l, sleep_us * 2);
      std::this_thread::sleep_for(std::chrono::microseconds(sleep_us));
    }
  }
}
// Between the two collectives of a sharded batch the peers already count on this rank: whatever leaves that region without having enqueued the
// record all-gather — an exception nobody expected — must not leave them waiting for it.
struct CommAbortGuard {
  hgs::Comm* comm;
  bool armed = true;
  ~CommAbortGuard() {
    if (armed) hgs::comm_abort(comm);
  }
};
// test hook, compiled ONLY into the host-emulation build (tests/emul/simt.py passes -DHGS_TESTING; the shipped library has neither the code nor
// the string): HGS_FAULT_AFTER_HEADER = "<kind>:<rank>" makes that rank fail between the two collectives — kind "batch": std::bad_alloc where
// run_batch runs (handled: the rank sends padding and reports after the exchange); kind "guard": an exception outside every handler (the guard
// aborts the communicator, the peers get HGS_ERR_COMM)
#ifdef HGS_TESTING
bool fault_after_header(const char* kind, int rank) {
  const char* e = std::getenv("HGS_FAULT_AFTER_HEADER");
  if (!e) return false;
  const size_t n = std::strlen(kind);
  return std::strncmp(e, kind, n) == 0 && e[n] == ':' && std::atoi(e + n + 1) == rank;
}
#else
constexpr bool fault_after_header(const char*, int) { return false; }
#endif
}  // namespace
extern "C" {

// Collective.  Once the arguments that are the same on every rank have been checked, EVERY path of a rank reaches both
// collectives — a rank whose own share is unusable (no target, an invalid or duplicated candidate cloud, a failed launch)
// announces an empty shard / sends padding and reports its error AFTER the exchange, so that a bad keyframe on one rank costs
// that rank's candidates ("not converged" records everywhere) and never blocks the other SLAM processes.  The one thing a rank
// cannot do is take part without device memory for the exchange buffers: it then aborts the communicator (ncclCommAbort), which
// makes the peers' collectives fail with HGS_ERR_COMM instead of hanging.
//   1. all-gather of a 16-byte header per rank {shard size, status}, enqueued in front of the batch's kernels;
//   2. the batch (run_batch), while the headers travel;
//   3. all-gather of max(shard size) record slots per rank — not n_total: an even partition of 512 candidates over 8 ranks moves
//      8 x 64 x 112 B = 57 KB instead of 458 KB — built on the device behind the kernels that produced the results;
//   4. one D2H of world x max(shard) slots, merge (hgs_debug_merge_shard_records), sequential selection rule.
int hgs_loop_match_batch_sharded(hgs_handle* h, hgs_cloud* const* candidates, size_t n_mine, const int32_t* candidate_ids, const float* guesses,
                                 size_t n_total, double max_range, hgs_result* all_out, int32_t* best) try {
  ApiLock lock(h);
  // ---- errors that keep the rank out of the collective: only what a correct caller gets wrong on every rank alike
  if (!h || !all_out || n_total == 0 || n_total > (size_t)1 << 24) return HGS_ERR_INVALID_ARGUMENT;
  if (!h->comm) {
    h->err = "hgs_loop_match_batch_sharded: hgs_comm_init has not been called on this engine";
    return HGS_ERR_COMM;
  }
  if (best) *best = -1;
  const int world = hgs::comm_world(h->comm), rank = hgs::comm_rank(h->comm);
  // ---- this rank's own share: problems found here are reported after the exchange
  int local = HGS_OK;
  std::string local_err;
  auto fail_local = [&](int rc, const std::string& why) {
    if (local == HGS_OK) local = rc, local_err = why;
  };
  if (n_mine > n_total || (n_mine > 0 && (!candidates || !candidate_ids || !guesses))) fail_local(HGS_ERR_INVALID_ARGUMENT, "hgs_loop_match_batch_sharded: bad candidate arrays");
  if (!h->target) fail_local(HGS_ERR_NO_TARGET, "hgs_loop_match_batch_sharded: no target set on this rank");
  std::vector<hgs_cloud*> src;
  if (local == HGS_OK) {
    src.assign(candidates, candidates + n_mine);
    for (size_t i = 0; i < n_mine; i++)
      if (!src[i] || src[i]->owner != h || candidate_ids[i] < 0 || (size_t)candidate_ids[i] >= n_total)
        fail_local(HGS_ERR_INVALID_ARGUMENT, "hgs_loop_match_batch_sharded: candidate " + std::to_string(i) + " is not a cloud of this engine or its id is out of range");
    std::vector<hgs_cloud*> sorted(src);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) fail_local(HGS_ERR_INVALID_ARGUMENT, "hgs_loop_match_batch_sharded: candidate clouds must be distinct");
  }
  const size_t n_send = local == HGS_OK ? n_mine : 0;
  // ---- exchange buffers (persistent, worst case: one rank holds every candidate)
  const size_t hdr_bytes = 16;
  const size_t ids_off = align_up((size_t)world * hdr_bytes + hdr_bytes, 16), rec_off = align_up(ids_off + 2 * n_total * sizeof(int32_t), 16);  // (ids: the candidate ids, and behind them where each slot's record sits in h->results)
  bool mem_ok = set_device(h) == HGS_OK;
  mem_ok = mem_ok && h->results.reserve(std::max<size_t>(n_total, 1) * sizeof(DevResult)) == hipSuccess;
  mem_ok = mem_ok && h->comm_send.reserve(n_total * sizeof(hgs_result) + hdr_bytes) == hipSuccess;
  mem_ok = mem_ok && h->comm_recv.reserve((size_t)world * (n_total * sizeof(hgs_result) + hdr_bytes)) == hipSuccess;
  mem_ok = mem_ok && h->comm_ids.reserve(2 * n_total * sizeof(int32_t)) == hipSuccess;
  mem_ok = mem_ok && h->h_comm.reserve(rec_off + (size_t)world * n_total * sizeof(hgs_result)) == hipSuccess;
  if (!mem_ok) {
    hgs::comm_abort(h->comm);
    h->err = "hgs_loop_match_batch_sharded: no memory for the exchange buffers; the communicator has been aborted (the peers' collective fails instead of waiting)";
    return HGS_ERR_OUT_OF_MEMORY;
  }
  char err[256] = "";
  auto comm_failed = [&](const char* what) {
    h->err = std::string(what) + ": " + err;
    hgs::comm_abort(h->comm);  // whatever state the peers are in, they must not wait for this rank
    return HGS_ERR_COMM;
  };
  // everything the region between the two collectives needs is allocated HERE, in front of the first one: past this point the
  // peers count on this rank, and the only exits are the record all-gather or an abort of the communicator
  std::vector<int32_t> counts(world, 0), statuses(world, 0);
  // ---- 1. headers: device layout comm_send = [header | records], comm_recv = [world headers | world x per records]
  int32_t* h_hdr = static_cast<int32_t*>(h->h_comm.p);  // pinned: [my header][world gathered headers]
  h_hdr[0] = (int32_t)n_send, h_hdr[1] = local, h_hdr[2] = 0, h_hdr[3] = 0;
  char* d_send = static_cast<char*>(h->comm_send.p);
  char* d_recv = static_cast<char*>(h->comm_recv.p);
  bool hip_ok = hipMemcpyAsync(d_send, h_hdr, hdr_bytes, hipMemcpyHostToDevice, h->stream) == hipSuccess;
  if (hgs::comm_all_gather(h->comm, d_send, d_recv, hdr_bytes, h->stream, err, sizeof(err)) != 0) return comm_failed("header all-gather");
  CommAbortGuard guard{h->comm};  // from here to the enqueued record all-gather
  hip_ok = hip_ok && hipMemcpyAsync(h_hdr + 4, d_recv, (size_t)world * hdr_bytes, hipMemcpyDeviceToHost, h->stream) == hipSuccess;
  if (!h->comm_event) hip_ok = hip_ok && hipEventCreateWithFlags(&h->comm_event, hipEventDisableTiming) == hipSuccess;
  hip_ok = hip_ok && hipEventRecord(h->comm_event, h->stream) == hipSuccess;
  if (fault_after_header("guard", rank)) throw std::runtime_error("HGS_FAULT_AFTER_HEADER=guard");
  // ---- 2. the batch.  A C++ exception in here (std::bad_alloc of a host-side vector, ...) is this rank's own problem like any other
  // failure of its share: it sends padding and reports after the exchange
  size_t n_valid = 0;  // records this rank really has
  if (n_send > 0 && hip_ok) {
    int rc;
    try {
      if (fault_after_header("batch", rank)) throw std::bad_alloc();
      rc = run_batch(h, src, guesses, &max_range);
    } catch (...) {
      rc = status_of_current_exception(h);
    }
    if (rc == HGS_OK) {
      n_valid = n_send;
    } else if (local == HGS_OK) {
      local = rc;
      try {
        local_err = h->err;
      } catch (...) {  // no memory for the text: the status code stands
      }
    }
  }
  // ---- 3. records: everybody knows everybody's shard size now
  if (hip_ok) {
    const int rc = comm_wait(h, [&] { return hipEventQuery(h->comm_event); }, "the gathered shard headers");
    if (rc != HGS_OK) {
      guard.armed = false;  // comm_wait has aborted the communicator
      return rc;
    }
  }
  size_t per = 1;
  if (hip_ok)
    for (int r = 0; r < world; r++) {
      counts[r] = std::max(0, std::min<int32_t>(h_hdr[4 + 4 * r], (int32_t)n_total));
      statuses[r] = h_hdr[4 + 4 * r + 1];
      per = std::max(per, (size_t)counts[r]);
    }
  if (!hip_ok) {  // the header never arrived here: this rank cannot know `per`; the guard aborts the communicator
    h->err = std::string("hgs_loop_match_batch_sharded: HIP error around the header exchange: ") + hipGetErrorString(hipGetLastError());
    return HGS_ERR_HIP;
  }
  hgs_result* d_records = reinterpret_cast<hgs_result*>(d_send + hdr_bytes);
  // an ordered batch (run_batch) left its records in its internal order: slot i (the caller's candidate i, with candidate_ids[i]) reads record pos[i]
  const bool ordered = n_valid > 0 && h->batch_order.size() == n_valid;
  if (n_valid > 0) {
    int32_t* h_ids = reinterpret_cast<int32_t*>(static_cast<char*>(h->h_comm.p) + ids_off);
    std::memcpy(h_ids, candidate_ids, n_valid * sizeof(int32_t));
    if (ordered)
      for (size_t i = 0; i < n_valid; i++) h_ids[n_valid + (size_t)h->batch_order[i]] = (int32_t)i;
    if (hipMemcpyAsync(h->comm_ids.p, h_ids, (ordered ? 2 : 1) * n_valid * sizeof(int32_t), hipMemcpyHostToDevice, h->stream) != hipSuccess) n_valid = 0;
  }
  launch_results_to_records(h->stream, h->results.as<DevResult>(), h->comm_ids.as<int>(), ordered && n_valid > 0 ? h->comm_ids.as<int>() + n_valid : nullptr, (int)n_valid,
                            (int)per, d_records);  // padding beyond n_valid
  hgs_result* d_gathered = reinterpret_cast<hgs_result*>(d_recv + (size_t)world * hdr_bytes);
  if (hgs::comm_all_gather(h->comm, d_records, d_gathered, per * sizeof(hgs_result), h->stream, err, sizeof(err)) != 0) {
    guard.armed = false;  // comm_failed aborts
    return comm_failed("record all-gather");
  }
  guard.armed = false;  // both collectives are enqueued: the peers depend on nothing further from this rank
  // ---- 4. merge
  hgs_result* gathered = reinterpret_cast<hgs_result*>(static_cast<char*>(h->h_comm.p) + rec_off);
  HGS_HIP(h, hipMemcpyAsync(gathered, d_gathered, (size_t)world * per * sizeof(hgs_result), hipMemcpyDeviceToHost, h->stream));
  HGS_TRY(comm_wait(h, [&] { return hipStreamQuery(h->stream); }, "the gathered records"));
  int32_t dup = -1;
  HGS_TRY(hgs_debug_merge_shard_records(gathered, counts.data(), world, per, n_total, all_out, &dup));
  if (best) HGS_TRY(hgs_select_best(all_out, n_total, best));
  if (local != HGS_OK) {
    h->err = local_err;
    return local;
  }
  if (dup >= 0) {  // every rank sees the same gathered slots, so every rank returns this
    h->err = "hgs_loop_match_batch_sharded: candidate id " + std::to_string(dup) + " was reported more than once (the first report was kept)";
    return HGS_ERR_INVALID_ARGUMENT;
  }
  h->err.clear();
  for (int r = 0; r < world; r++)
    if (statuses[r] != HGS_OK && r != rank) h->err += "rank " + std::to_string(r) + " reported status " + std::to_string(statuses[r]) + " (its candidates are not converged); ";
  return HGS_OK;
} catch (...) {
  return status_of_current_exception(h);
}

// ---- prefilter (apps/prefiltering_nodelet.cpp:131-182) -------------------------------------------------------
namespace {

// a resident cloud from a device array of {x, y, z, intensity}
int cloud_from_device(hgs_handle* h, const float4* src, size_t m, hgs_cloud** out) {
  hgs_cloud* c = nullptr;
  HGS_TRY(cloud_alloc(h, m, &c));
  const CloudDesc resident = resident_desc(c);
  launch_pf_to_cloud(h->stream, src, (int)m, const_cast<float4*>(c->desc.raw), c->intensity, c->desc.meta, &resident, c->dev_desc);
  launch_bbox_count(h->stream, c->dev_desc, 1, (int)m);  // (the meta record was reset and the descriptor written by k_pf_to_cloud)
  hipError_t e = hipGetLastError();
  // (no synchronisation: `src` is a device array of this engine, read in stream order)
  if (e != hipSuccess) {
    h->err = std::string("prefilter: building the resident cloud failed: ") + hipGetErrorString(e);
    cloud_free(c);
    return HGS_ERR_HIP;
  }
  *out = c;
  return HGS_OK;
}

}  // namespace

extern "C" int hgs_prefilter_params_default(hgs_prefilter_params* p) try {
  if (!p) return HGS_ERR_INVALID_ARGUMENT;
  std::memset(p, 0, sizeof(*p));
  p->use_distance_filter = 1;          // prefiltering_nodelet.cpp:94
  p->distance_near_thresh = 1.0;       // :95
  p->distance_far_thresh = 100.0;      // :96
  p->downsample_method = HGS_DOWNSAMPLE_VOXELGRID;   // :52
  p->downsample_resolution = 0.1;      // :53
  p->outlier_removal_method = HGS_OUTLIER_STATISTICAL;  // :73
  p->statistical_mean_k = 20;          // :75
  p->statistical_stddev = 1.0;         // :76
  p->radius_radius = 0.8;              // :85
  p->radius_min_neighbors = 2;         // :86
  return HGS_OK;
} catch (...) {
  return status_of_current_exception(nullptr);
}

static bool prefilter_params_ok(const hgs_prefilter_params* p) {
  return !(p->downsample_method < HGS_DOWNSAMPLE_NONE || p->downsample_method > HGS_DOWNSAMPLE_APPROX_VOXELGRID || p->outlier_removal_method < HGS_OUTLIER_NONE ||
           p->outlier_removal_method > HGS_OUTLIER_RADIUS || (p->downsample_method != HGS_DOWNSAMPLE_NONE && !(p->downsample_resolution > 0)) ||
           (p->outlier_removal_method == HGS_OUTLIER_STATISTICAL && (p->statistical_mean_k < 1 || p->statistical_mean_k > 62)) ||
           (p->outlier_removal_method == HGS_OUTLIER_RADIUS && (!(p->radius_radius > 0) || p->radius_min_neighbors < 0)));
}
// what one sweep brings besides its points, checked and in the kernels' form: w = -ang_v as floats (null gyro sample: no deskewing, scan period 0),
// the upper three rows of sensor_to_base row-major (null: no transform)
struct PfSweepArgs {
  float w[3] = {0.f, 0.f, 0.f};
  bool deskew = false, framed = false;
  double scan_period = 0.0;
  PfFrame frame{};
};
static int prefilter_sweep_args(hgs_handle* h, const void* pts, size_t n, size_t stride_bytes, const double* imu_angular_velocity, double scan_period,
                                const float* sensor_to_base, PfSweepArgs* a) {
  if ((n > 0 && !pts) || stride_bytes < 12 || (stride_bytes % 4) != 0 || n > (size_t)1 << 30) return HGS_ERR_INVALID_ARGUMENT;
  // ang_v(x, y, z) as floats, times -1 (:219-220); an empty imu_queue passes the cloud as it is (:184-186)
  if (imu_angular_velocity) {
    if (!std::isfinite(scan_period)) return HGS_ERR_INVALID_ARGUMENT;
    for (int k = 0; k < 3; k++) a->w[k] = -(float)imu_angular_velocity[k];
    a->deskew = true, a->scan_period = scan_period;
  }
  if (sensor_to_base) {  // column-major 4x4: a rigid transform's bottom row; the rotation block is not looked at (pcl::transformPointCloud does not either)
    bool finite = true;
    for (int k = 0; k < 16; k++) finite = finite && std::isfinite(sensor_to_base[k]);
    if (!finite || sensor_to_base[3] != 0.f || sensor_to_base[7] != 0.f || sensor_to_base[11] != 0.f || sensor_to_base[15] != 1.f) {
      h->err = finite ? "prefilter: the bottom row of sensor_to_base is not 0 0 0 1" : "prefilter: sensor_to_base has a non-finite entry";
      return HGS_ERR_INVALID_ARGUMENT;
    }
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 4; c++) a->frame.rows[4 * r + c] = sensor_to_base[4 * c + r];
    a->framed = true;
  }
  return HGS_OK;
}

// the one sequence behind hgs_prefilter, hgs_prefilter_deskewed and hgs_prefilter_framed.  imu_angular_velocity null: no deskewing; sensor_to_base null:
// no transform (then the launches and their arguments are those of the two older entry points)
static int prefilter_impl(hgs_handle* h, const void* pts, size_t n, size_t stride_bytes, const hgs_prefilter_params* p, const double* imu_angular_velocity,
                          double scan_period, const float* sensor_to_base, hgs_cloud** out, hgs_handle::PfBatchStats* stats = nullptr) {
  ApiLock lock(h);
  if (!h || !p || !out || !prefilter_params_ok(p)) return HGS_ERR_INVALID_ARGUMENT;
  PfSweepArgs args;
  HGS_TRY(prefilter_sweep_args(h, pts, n, stride_bytes, imu_angular_velocity, scan_period, sensor_to_base, &args));
  const float* deskew_w = args.deskew ? args.w : nullptr;
  scan_period = args.scan_period;
  const PfFrame* frame = args.framed ? &args.frame : nullptr;
  HGS_TRY(set_device(h));
  *out = nullptr;
  StageTimer tm(h, HGS_STAGE_PREFILTER);
  const size_t cap = std::max<size_t>(n, 1);
  HGS_HIP(h, h->pf_a.reserve(cap * sizeof(float4)));
  HGS_HIP(h, h->pf_b.reserve(cap * sizeof(float4)));
  HGS_HIP(h, h->pf_keep.reserve(cap * sizeof(uint32_t)));
  HGS_HIP(h, h->pf_slot.reserve(cap * sizeof(uint32_t)));
  HGS_HIP(h, h->pf_small.reserve(256));
  HGS_HIP(h, h->h_small.reserve(256));
  float4* cur = h->pf_a.as<float4>();
  float4* other = h->pf_b.as<float4>();
  bool grid_radius = false;  // the outlier removal ran on the voxel grid (below): nothing left to do behind the read-back
  int* d_count = h->pf_small.as<int>();                    // [0] current point count
  unsigned* d_meta = h->pf_small.as<unsigned>() + 16;      // voxel-grid bbox / grid parameters
  double* d_stats = reinterpret_cast<double*>(h->pf_small.as<char>() + 192);
  {
    const float4* staged = nullptr;
    if (n > 0) HGS_TRY(upload_points_packed(h, pts, n, stride_bytes, &staged));
    launch_pf_load(h->stream, staged, (int)n, cur, deskew_w, scan_period, frame, d_count, d_meta);  // (also: d_count = n, d_meta = the empty voxel-grid record)
  }
  // VoxelGrid behind the distance filter (every launch file's prefilter): the filter is applied inside the voxel grid's bounding-box and key kernels
  // instead of by flags + scan + compaction in front of them (four launches less; prefilter_fast = 0 keeps the separate pass — A/B, tests)
  const bool voxelgrid = n > 0 && p->downsample_method == HGS_DOWNSAMPLE_VOXELGRID;
  const int inline_dist = (voxelgrid && p->use_distance_filter && h->prefilter_fast) ? 1 : 0;
  if (n > 0 && p->use_distance_filter && !inline_dist) {
    launch_pf_distance_flags(h->stream, cur, (int)n, 1, p->distance_near_thresh, p->distance_far_thresh, h->pf_keep.as<unsigned>());
    HGS_TRY(scan_u32(h, h->pf_keep.as<uint32_t>(), h->pf_slot.as<uint32_t>(), n));
    launch_pf_compact(h->stream, cur, (int)n, h->pf_keep.as<unsigned>(), h->pf_slot.as<unsigned>(), other, d_count);
    std::swap(cur, other);
  }
  if (n > 0 && p->downsample_method == HGS_DOWNSAMPLE_VOXELGRID) {
    const float inv_leaf = 1.0f / (float)p->downsample_resolution;
    launch_pf_bbox(h->stream, cur, d_count, (int)n, d_meta, inline_dist, p->distance_near_thresh, p->distance_far_thresh);
    launch_pf_grid(h->stream, d_meta, inv_leaf);
    HGS_TRY(reserve_sort_pairs(h, n));
    launch_pf_voxel_keys(h->stream, cur, d_count, d_meta, inv_leaf, (int)n, h->sort_keys[0].as<unsigned long long>(), h->sort_vals[0].as<unsigned>(), inline_dist,
                         p->distance_near_thresh, p->distance_far_thresh);
    HGS_TRY(sort_pairs(h, n, 0, 32));
    launch_pf_voxel_heads(h->stream, h->sort_keys[1].as<unsigned long long>(), (int)n, h->pf_keep.as<unsigned>(), kVoxelInvalidKey);
    HGS_TRY(scan_u32(h, h->pf_keep.as<uint32_t>(), h->pf_slot.as<uint32_t>(), n));
    // RadiusOutlierRemoval right behind it (the KITTI launch file's prefilter) needs no search tree: the centroids come out in voxel-key order, a point's
    // neighbours are found by key (k_pf_grid_radius_flags) — no resident cloud + index built only to be thrown away, and no host read-back of the voxel
    // count in the middle of the pipeline to size them (the rows of the r-box: at most (2 ceil(r / leaf) + 2)^2 binary searches per point)
    grid_radius = h->prefilter_fast && p->outlier_removal_method == HGS_OUTLIER_RADIUS && p->radius_radius / p->downsample_resolution <= 4.0;
    unsigned* ukeys = nullptr;
    if (grid_radius) {
      HGS_HIP(h, h->pf_ukeys.reserve(n * sizeof(uint32_t)));
      ukeys = h->pf_ukeys.as<unsigned>();
    }
    launch_pf_voxel_centroids(h->stream, cur, h->sort_keys[1].as<unsigned long long>(), h->sort_vals[1].as<unsigned>(), h->pf_keep.as<unsigned>(),
                              h->pf_slot.as<unsigned>(), (int)n, other, d_count, ukeys);
    std::swap(cur, other);
    if (grid_radius) {
      launch_pf_grid_radius_flags(h->stream, cur, d_count, ukeys, d_meta, inv_leaf, (float)p->radius_radius, (float)(p->radius_radius * p->radius_radius),
                                  p->radius_min_neighbors, (int)n, h->pf_keep.as<unsigned>());
      HGS_TRY(scan_u32(h, h->pf_keep.as<uint32_t>(), h->pf_slot.as<uint32_t>(), n));
      launch_pf_compact(h->stream, cur, (int)n, h->pf_keep.as<unsigned>(), h->pf_slot.as<unsigned>(), other, d_count);
      std::swap(cur, other);
    }
  }
  if (n > 0 && p->downsample_method == HGS_DOWNSAMPLE_APPROX_VOXELGRID) {
    // pcl::ApproximateVoxelGrid: stable sort by history bucket, runs of equal voxel, eviction order (k_pf_approx_*)
    const float inv_leaf = 1.0f / (float)p->downsample_resolution;
    HGS_TRY(reserve_sort_pairs(h, n));
    const size_t o_bucket = align_up(n * sizeof(uint32_t), 256);
    HGS_HIP(h, h->misc.reserve(o_bucket + 2048 * sizeof(uint32_t)));
    unsigned* d_head = h->misc.as<unsigned>();
    unsigned* d_bucket_used = reinterpret_cast<unsigned*>(h->misc.as<char>() + o_bucket);
    unsigned* d_bucket_rank = d_bucket_used + 512;
    launch_pf_approx_keys(h->stream, cur, d_count, inv_leaf, (int)n, h->sort_keys[0].as<unsigned long long>(), h->sort_vals[0].as<unsigned>());
    HGS_TRY(sort_pairs(h, n, 0, 10));
    HGS_HIP(h, hipMemsetAsync(h->pf_keep.p, 0, n * sizeof(uint32_t), h->stream));
    HGS_HIP(h, hipMemsetAsync(d_bucket_used, 0, 1025 * sizeof(uint32_t), h->stream));
    launch_pf_approx_heads(h->stream, cur, h->sort_keys[1].as<unsigned long long>(), h->sort_vals[1].as<unsigned>(), inv_leaf, (int)n, d_head, h->pf_keep.as<unsigned>(),
                           d_bucket_used, d_bucket_rank);
    HGS_TRY(scan_u32(h, h->pf_keep.as<uint32_t>(), h->pf_slot.as<uint32_t>(), n));
    launch_pf_approx_centroids(h->stream, cur, h->sort_keys[1].as<unsigned long long>(), h->sort_vals[1].as<unsigned>(), d_head, h->pf_keep.as<unsigned>(),
                               h->pf_slot.as<unsigned>(), d_bucket_rank, (int)n, other, d_count);
    std::swap(cur, other);
  }
  HGS_HIP(h, hipGetLastError());
  int* hs = h->h_small.as<int>();
  // the point count (pf_small[0]) and the voxel grid's overflow flag (d_meta[12] = pf_small[28]) in ONE copy
  HGS_HIP(h, hipMemcpyAsync(hs, d_count, 32 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HGS_HIP(h, hipStreamSynchronize(h->stream));
  if (stats) stats->readbacks++;
  size_t m = (size_t)std::max(0, hs[0]);
  if (n > 0 && p->downsample_method == HGS_DOWNSAMPLE_VOXELGRID && hs[16 + 12]) {
    h->err = "prefilter: voxel grid too fine for this cloud (index overflow; pcl::VoxelGrid refuses it too)";
    return HGS_ERR_INVALID_ARGUMENT;
  }
  hgs_cloud* c = nullptr;
  HGS_TRY(cloud_from_device(h, cur, m, &c));
  if (m > 0 && p->outlier_removal_method != HGS_OUTLIER_NONE && !grid_radius) {
    std::vector<hgs_cloud*> one{c};
    int rc = ensure_index(h, one);
    if (stats) stats->index_builds++;
    if (rc == HGS_OK) {
      hipError_t e = hipMemsetAsync(h->pf_keep.p, 0, m * sizeof(uint32_t), h->stream);  // non-finite points are dropped: only valid points get a flag
      if (e != hipSuccess) rc = HGS_ERR_HIP;
    }
    if (rc == HGS_OK) {
      if (p->outlier_removal_method == HGS_OUTLIER_RADIUS) {
        launch_pf_radius_flags(h->stream, c->desc, (float)(p->radius_radius * p->radius_radius), p->radius_min_neighbors, h->pf_keep.as<unsigned>());
      } else {
        hipError_t e = h->pf_dist.reserve(m * sizeof(double));
        if (e == hipSuccess) e = hipMemsetAsync(h->pf_dist.p, 0, m * sizeof(double), h->stream);
        if (e != hipSuccess) rc = HGS_ERR_HIP;
        else {
          launch_pf_mean_knn_dist(h->stream, c->desc, p->statistical_mean_k, h->pf_dist.as<double>());
          launch_pf_statistical(h->stream, c->desc, h->pf_dist.as<double>(), d_stats, p->statistical_stddev, h->pf_keep.as<unsigned>());
        }
      }
    }
    if (rc == HGS_OK) rc = scan_u32(h, h->pf_keep.as<uint32_t>(), h->pf_slot.as<uint32_t>(), m);
    if (rc == HGS_OK) {
      launch_pf_compact(h->stream, cur, (int)m, h->pf_keep.as<unsigned>(), h->pf_slot.as<unsigned>(), other, d_count);
      hipError_t e = hipMemcpyAsync(hs, d_count, sizeof(int), hipMemcpyDeviceToHost, h->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
      if (e != hipSuccess) rc = HGS_ERR_HIP;
      if (stats) stats->readbacks++;
    }
    cloud_free(c);
    c = nullptr;
    if (rc != HGS_OK) {
      if (h->err.empty()) h->err = "prefilter: outlier removal failed";
      return rc;
    }
    HGS_TRY(cloud_from_device(h, other, (size_t)std::max(0, hs[0]), &c));
  }
  *out = c;
  return HGS_OK;
}

extern "C" int hgs_prefilter(hgs_handle* h, const void* pts, size_t n, size_t stride_bytes, const hgs_prefilter_params* p, hgs_cloud** out) try {
  return prefilter_impl(h, pts, n, stride_bytes, p, nullptr, 0.0, nullptr, out);
} catch (...) {
  return status_of_current_exception(h);
}

extern "C" int hgs_prefilter_deskewed(hgs_handle* h, const void* pts, size_t n, size_t stride_bytes, const hgs_prefilter_params* p, const double* imu_angular_velocity,
                                      double scan_period, hgs_cloud** out) try {
  return prefilter_impl(h, pts, n, stride_bytes, p, imu_angular_velocity, scan_period, nullptr, out);
} catch (...) {
  return status_of_current_exception(h);
}

extern "C" int hgs_prefilter_framed(hgs_handle* h, const void* pts, size_t n, size_t stride_bytes, const hgs_prefilter_params* p, const double* imu_angular_velocity,
                                    double scan_period, const float* sensor_to_base, hgs_cloud** out) try {
  return prefilter_impl(h, pts, n, stride_bytes, p, imu_angular_velocity, scan_period, sensor_to_base, out);
} catch (...) {
  return status_of_current_exception(h);
}

// ---- several sweeps in one batch (include/hgs_registration.h; the k_pfb_* kernels of hgs_kernels.hip) -------------------------------------------------
namespace {

// RadiusOutlierRemoval on the voxel grid (what prefilter_impl calls grid_radius): no search tree
bool prefilter_grid_radius(const hgs_handle* h, const hgs_prefilter_params* p) {
  return p->downsample_method == HGS_DOWNSAMPLE_VOXELGRID && h->prefilter_fast && p->outlier_removal_method == HGS_OUTLIER_RADIUS &&
         p->radius_radius / p->downsample_resolution <= 4.0;
}

// Which parameter sets the batch runs itself: no downsampling or pcl::VoxelGrid, behind it any outlier removal — none, RadiusOutlierRemoval on the voxel
// grid, or one on a search tree per cloud (STATISTICAL and the other RADIUS shapes: the tail of prefilter_batch_impl; "prefilter_batch_tree" = 0 sends
// those sweep after sweep through prefilter_impl as ApproximateVoxelGrid's sequential history table always goes).
bool prefilter_batched(const hgs_handle* h, const hgs_prefilter_params* p) {
  if (p->downsample_method == HGS_DOWNSAMPLE_APPROX_VOXELGRID) return false;
  return p->outlier_removal_method == HGS_OUTLIER_NONE || prefilter_grid_radius(h, p) || h->prefilter_batch_tree;
}

int floor_batch_clouds(hgs_handle* h, const float4* in, const std::vector<int>& offs, const std::vector<size_t>& counts, hgs_cloud** out);  // (below)

// clouds that live for the length of one call: freed on every way out of it
struct ScratchClouds {
  std::vector<hgs_cloud*> list;
  void release() {
    for (hgs_cloud* c : list) cloud_free(c);
    list.clear();
  }
  ~ScratchClouds() { release(); }
};

void free_clouds(hgs_cloud** out, size_t n) {
  for (size_t i = 0; i < n; i++) {
    if (out[i]) cloud_free(out[i]);
    out[i] = nullptr;
  }
}

// the sweeps one after the other: prefilter_impl's sequence per sweep (S = 1, and the parameter sets the batch does not run)
int prefilter_each(hgs_handle* h, const hgs_prefilter_sweep* sweeps, size_t S, const hgs_prefilter_params* p, hgs_cloud** out) {
  for (size_t i = 0; i < S; i++) {
    const hgs_prefilter_sweep& w = sweeps[i];
    const int rc = prefilter_impl(h, w.pts, w.n, w.stride_bytes, p, w.imu_angular_velocity, w.scan_period, w.sensor_to_base, &out[i], &h->pb);
    if (rc != HGS_OK) {
      h->err = "sweep " + std::to_string(i) + ": " + h->err;
      free_clouds(out, S);
      return rc;
    }
  }
  return HGS_OK;
}

int prefilter_batch_impl(hgs_handle* h, const hgs_prefilter_sweep* sweeps, size_t S, const std::vector<PfSweepArgs>& args, const hgs_prefilter_params* p,
                         hgs_cloud** out) {
  std::vector<size_t> off(S + 1, 0);
  size_t max_n = 0;
  for (size_t i = 0; i < S; i++) off[i + 1] = off[i] + sweeps[i].n, max_n = std::max(max_n, sweeps[i].n);
  const size_t total = off[S], cap = std::max<size_t>(total, 1);
  const size_t table_bytes = S * sizeof(PfSweep);
  HGS_HIP(h, h->pf_a.reserve(cap * sizeof(float4)));
  HGS_HIP(h, h->pf_b.reserve(cap * sizeof(float4)));
  HGS_HIP(h, h->pf_keep.reserve(cap * sizeof(uint32_t)));
  HGS_HIP(h, h->pf_slot.reserve(cap * sizeof(uint32_t)));
  HGS_HIP(h, h->pf_table.reserve(table_bytes));
  HGS_HIP(h, h->h_pf_table.reserve(table_bytes));
  HGS_HIP(h, h->staging.reserve(cap * sizeof(float4)));
  PfSweep* d_sweeps = h->pf_table.as<PfSweep>();
  const int nS = (int)S, mx = (int)max_n;
  {
    StageTimer tm(h, HGS_STAGE_UPLOAD);
    void* staged = nullptr;
    int slot = 0;
    HGS_HIP(h, h->up.stage(table_bytes, &staged, &slot));
    PfSweep* t = static_cast<PfSweep*>(staged);
    bool any_large = false;
    for (size_t i = 0; i < S; i++) {
      t[i] = PfSweep{};
      t[i].off = (int)off[i], t[i].n = (int)sweeps[i].n;
      t[i].deskew = args[i].deskew, t[i].frame = args[i].framed, t[i].scan_period = args[i].scan_period;
      std::memcpy(t[i].w, args[i].w, sizeof(t[i].w));
      std::memcpy(t[i].rows, args[i].frame.rows, sizeof(t[i].rows));
      any_large = any_large || sweeps[i].n >= kUploadParallelPoints;
    }
    HGS_HIP(h, hipMemcpyAsync(d_sweeps, t, table_bytes, hipMemcpyHostToDevice, h->stream));
    HGS_HIP(h, h->up.commit(slot, h->stream));
    // ONE staging image, every sweep at its offset; the large sweeps share one opening of the pinned image (its event logic: upload_image_open / _close)
    if (any_large) HGS_TRY(upload_image_open(h, total));
    for (size_t i = 0; i < S; i++)
      if (sweeps[i].n > 0) HGS_TRY(upload_points_at(h, sweeps[i].pts, sweeps[i].n, sweeps[i].stride_bytes, off[i], any_large));
    if (any_large) HGS_TRY(upload_image_close(h));
  }
  StageTimer tm(h, HGS_STAGE_PREFILTER);
  float4* cur = h->pf_a.as<float4>();
  float4* other = h->pf_b.as<float4>();
  unsigned* keep = h->pf_keep.as<unsigned>();
  unsigned* slot = h->pf_slot.as<unsigned>();
  launch_pfb_load(h->stream, h->staging.as<float4>(), d_sweeps, nS, mx, cur);
  const bool voxelgrid = total > 0 && p->downsample_method == HGS_DOWNSAMPLE_VOXELGRID;
  const int inline_dist = (voxelgrid && p->use_distance_filter && h->prefilter_fast) ? 1 : 0;
  const bool grid_radius = voxelgrid && prefilter_grid_radius(h, p);
  if (total > 0 && p->use_distance_filter && !inline_dist) {
    launch_pfb_distance_flags(h->stream, cur, d_sweeps, nS, mx, p->distance_near_thresh, p->distance_far_thresh, keep);
    HGS_TRY(scan_u32(h, keep, slot, total));
    launch_pfb_compact(h->stream, cur, d_sweeps, nS, mx, keep, slot, other);
    std::swap(cur, other);
  }
  if (voxelgrid) {
    const float inv_leaf = 1.0f / (float)p->downsample_resolution;
    launch_pfb_bbox(h->stream, cur, d_sweeps, nS, mx, inline_dist, p->distance_near_thresh, p->distance_far_thresh);
    launch_pfb_grid(h->stream, d_sweeps, nS, inv_leaf);
    HGS_TRY(reserve_sort_pairs(h, total));
    launch_pfb_voxel_keys(h->stream, cur, d_sweeps, nS, mx, inv_leaf, h->sort_keys[0].as<unsigned long long>(), h->sort_vals[0].as<unsigned>(), inline_dist,
                          p->distance_near_thresh, p->distance_far_thresh);
    int ordinal_bits = 0;
    while (((size_t)1 << ordinal_bits) < S) ordinal_bits++;
    HGS_TRY(sort_pairs(h, total, 0, 32 + ordinal_bits));  // stable: every sweep keeps its slice, in the order its own sort over bits 0..31 gives
    launch_pfb_voxel_heads(h->stream, h->sort_keys[1].as<unsigned long long>(), d_sweeps, nS, mx, keep);
    HGS_TRY(scan_u32(h, keep, slot, total));
    unsigned* ukeys = nullptr;
    if (grid_radius) {
      HGS_HIP(h, h->pf_ukeys.reserve(total * sizeof(uint32_t)));
      ukeys = h->pf_ukeys.as<unsigned>();
    }
    launch_pfb_voxel_centroids(h->stream, cur, h->sort_keys[1].as<unsigned long long>(), h->sort_vals[1].as<unsigned>(), keep, slot, d_sweeps, nS, mx, other, ukeys);
    std::swap(cur, other);
    if (grid_radius) {
      launch_pfb_grid_radius_flags(h->stream, cur, ukeys, d_sweeps, nS, mx, inv_leaf, (float)p->radius_radius, (float)(p->radius_radius * p->radius_radius),
                                   p->radius_min_neighbors, keep);
      HGS_TRY(scan_u32(h, keep, slot, total));
      launch_pfb_compact(h->stream, cur, d_sweeps, nS, mx, keep, slot, other);
      std::swap(cur, other);
    }
  }
  HGS_HIP(h, hipGetLastError());
  // every sweep's count and voxel-grid overflow flag in ONE copy (the table)
  const PfSweep* hs = h->h_pf_table.as<PfSweep>();
  HGS_HIP(h, hipMemcpyAsync(h->h_pf_table.p, d_sweeps, table_bytes, hipMemcpyDeviceToHost, h->stream));
  HGS_HIP(h, hipStreamSynchronize(h->stream));
  h->pb.readbacks++;
  if (voxelgrid)
    for (size_t i = 0; i < S; i++)
      if (sweeps[i].n > 0 && hs[i].meta[12]) {
        h->err = "sweep " + std::to_string(i) + ": prefilter: voxel grid too fine for this cloud (index overflow; pcl::VoxelGrid refuses it too)";
        return HGS_ERR_INVALID_ARGUMENT;
      }
  // The outlier removals on a search tree (prefilter_impl's second half for every sweep at once): the K sweeps that still have points become resident
  // clouds out of their slices in one launch, get their indices in ONE build and their flags in ONE launch over the K descriptors, one grid row per cloud;
  // a flag lands at the point's position in its sweep's slice, so that ONE scan and k_pfb_compact finish every sweep.  Then the table again: the final counts.
  if (p->outlier_removal_method != HGS_OUTLIER_NONE && !grid_radius) {
    std::vector<int> offs;
    std::vector<size_t> counts;
    size_t max_mid = 0;
    for (size_t i = 0; i < S; i++)
      if (hs[i].count > 0) offs.push_back((int)off[i]), counts.push_back((size_t)hs[i].count), max_mid = std::max(max_mid, (size_t)hs[i].count);
    const size_t K = offs.size();
    if (K > 0) {
      ScratchClouds mid;
      mid.list.assign(K, nullptr);
      HGS_TRY(floor_batch_clouds(h, cur, offs, counts, mid.list.data()));
      h->pb.index_builds++;
      HGS_TRY(ensure_index(h, mid.list));
      HGS_HIP(h, hipMemsetAsync(keep, 0, total * sizeof(uint32_t), h->stream));  // non-finite points are dropped: only valid points get a flag
      const size_t o_stats = 256 + align_up(K * sizeof(int), 16);
      HGS_HIP(h, h->pf_small.reserve(o_stats + 2 * K * sizeof(double)));
      int* d_keep_off = reinterpret_cast<int*>(h->pf_small.as<char>() + 256);
      double* d_stats = reinterpret_cast<double*>(h->pf_small.as<char>() + o_stats);
      HGS_HIP(h, h->up.upload(d_keep_off, offs.data(), K * sizeof(int), h->stream));
      const CloudDesc* d_descs = nullptr;
      HGS_TRY(upload_descs(h, mid.list, false, &d_descs, nullptr));
      h->pb.tree_launches++;
      if (p->outlier_removal_method == HGS_OUTLIER_RADIUS) {
        launch_pfb_radius_flags(h->stream, d_descs, (int)K, (int)max_mid, d_keep_off, (float)(p->radius_radius * p->radius_radius), p->radius_min_neighbors, keep);
      } else {
        HGS_HIP(h, h->pf_dist.reserve(total * sizeof(double)));
        HGS_HIP(h, hipMemsetAsync(h->pf_dist.p, 0, total * sizeof(double), h->stream));
        launch_pfb_mean_knn_dist(h->stream, d_descs, (int)K, (int)max_mid, d_keep_off, p->statistical_mean_k, h->pf_dist.as<double>());
        launch_pfb_statistical(h->stream, d_descs, (int)K, (int)max_mid, d_keep_off, h->pf_dist.as<double>(), d_stats, p->statistical_stddev, keep);
      }
      HGS_TRY(scan_u32(h, keep, slot, total));
      launch_pfb_compact(h->stream, cur, d_sweeps, nS, mx, keep, slot, other);
      std::swap(cur, other);
      HGS_HIP(h, hipGetLastError());
      HGS_HIP(h, hipMemcpyAsync(h->h_pf_table.p, d_sweeps, table_bytes, hipMemcpyDeviceToHost, h->stream));
      HGS_HIP(h, hipStreamSynchronize(h->stream));
      h->pb.readbacks++;
      // (nothing queued reads the intermediate clouds any more: their blocks go back to the pool in front of the allocations below)
    }
  }
  size_t max_m = 0;
  for (size_t i = 0; i < S; i++) {
    const size_t m = (size_t)std::max(0, hs[i].count);
    HGS_TRY(cloud_alloc(h, m, &out[i]));
    max_m = std::max(max_m, m);
  }
  // the new clouds' descriptors, where each goes, and the intensity arrays: one staged block
  const size_t o_out = align_up(S * sizeof(CloudDesc), 16), o_int = o_out + S * sizeof(CloudDesc*), tail_bytes = o_int + S * sizeof(float*);
  HGS_HIP(h, h->descs.reserve(tail_bytes));
  void* staged = nullptr;
  int ring_slot = 0;
  HGS_HIP(h, h->up.stage(tail_bytes, &staged, &ring_slot));
  char* hb = static_cast<char*>(staged);
  for (size_t i = 0; i < S; i++) {
    reinterpret_cast<CloudDesc*>(hb)[i] = resident_desc(out[i]);
    reinterpret_cast<CloudDesc**>(hb + o_out)[i] = out[i]->dev_desc;
    reinterpret_cast<float**>(hb + o_int)[i] = out[i]->intensity;
  }
  HGS_HIP(h, hipMemcpyAsync(h->descs.p, hb, tail_bytes, hipMemcpyHostToDevice, h->stream));
  HGS_HIP(h, h->up.commit(ring_slot, h->stream));
  char* db = h->descs.as<char>();
  launch_pfb_to_cloud(h->stream, cur, d_sweeps, reinterpret_cast<const CloudDesc*>(db), reinterpret_cast<CloudDesc* const*>(db + o_out),
                      reinterpret_cast<float* const*>(db + o_int), nS, (int)max_m);
  launch_bbox_count(h->stream, reinterpret_cast<const CloudDesc*>(db), nS, (int)max_m);
  HGS_HIP(h, hipGetLastError());
  return HGS_OK;
}

}  // namespace

extern "C" int hgs_prefilter_batch(hgs_handle* h, const hgs_prefilter_sweep* sweeps, size_t n_sweeps, const hgs_prefilter_params* p, hgs_cloud** out) try {
  ApiLock lock(h);
  if (!h || !p || !prefilter_params_ok(p)) return HGS_ERR_INVALID_ARGUMENT;
  if (n_sweeps == 0) return HGS_OK;
  if (!sweeps || !out) return HGS_ERR_INVALID_ARGUMENT;
  if (n_sweeps > HGS_PREFILTER_BATCH_MAX_SWEEPS) {
    h->err = "hgs_prefilter_batch: more than " + std::to_string(HGS_PREFILTER_BATCH_MAX_SWEEPS) + " sweeps in one call";
    return HGS_ERR_INVALID_ARGUMENT;
  }
  static_assert(HGS_PREFILTER_BATCH_MAX_SWEEPS == 1 << kPfBatchOrdinalBits, "the sort key's ordinal bits");
  std::vector<PfSweepArgs> args(n_sweeps);
  size_t total = 0;
  h->err.clear();
  for (size_t i = 0; i < n_sweeps; i++) {
    const hgs_prefilter_sweep& w = sweeps[i];
    const int rc = prefilter_sweep_args(h, w.pts, w.n, w.stride_bytes, w.imu_angular_velocity, w.scan_period, w.sensor_to_base, &args[i]);
    if (rc != HGS_OK) {
      h->err = "sweep " + std::to_string(i) + ": " + (h->err.empty() ? std::string("invalid points, stride or scan period") : h->err);
      return rc;
    }
    total += w.n;
  }
  if (total > (size_t)1 << 30) {
    h->err = "hgs_prefilter_batch: more than 2^30 points in one call";
    return HGS_ERR_INVALID_ARGUMENT;
  }
  HGS_TRY(set_device(h));
  for (size_t i = 0; i < n_sweeps; i++) out[i] = nullptr;
  h->pb = hgs_handle::PfBatchStats{};
  h->pb.sweeps = (int)n_sweeps;
  if (n_sweeps == 1 || !prefilter_batched(h, p)) return prefilter_each(h, sweeps, n_sweeps, p, out);
  h->pb.batched = 1;
  int rc;
  try {
    rc = prefilter_batch_impl(h, sweeps, n_sweeps, args, p, out);
  } catch (...) {  // (a failed host allocation: the clouds made so far are freed below like after a HIP error)
    rc = status_of_current_exception(h);
  }
  if (rc != HGS_OK) free_clouds(out, n_sweeps);
  return rc;
} catch (...) {
  return status_of_current_exception(h);
}

extern "C" int hgs_debug_prefilter_batch_stats(hgs_handle* h, int32_t* sweeps, int32_t* batched, int32_t* readbacks, int32_t* index_builds, int32_t* tree_launches) try {
  ApiLock lock(h);
  if (!h) return HGS_ERR_INVALID_ARGUMENT;
  if (sweeps) *sweeps = h->pb.sweeps;
  if (batched) *batched = h->pb.batched;
  if (readbacks) *readbacks = h->pb.readbacks;
  if (index_builds) *index_builds = h->pb.index_builds;
  if (tree_launches) *tree_launches = h->pb.tree_launches;
  return HGS_OK;
} catch (...) {
  return status_of_current_exception(h);
}

extern "C" int hgs_cloud_download(hgs_cloud* c, void* out_pts, size_t stride_bytes) try {
  ApiLock lock(c);
  if (!c || !c->owner || stride_bytes < 12 || (stride_bytes % 4) != 0 || (c->n_input > 0 && !out_pts)) return HGS_ERR_INVALID_ARGUMENT;
  hgs_handle* h = c->owner;
  HGS_TRY(set_device(h));
  const size_t n = c->n_input;
  if (n == 0) return HGS_OK;
  HGS_HIP(h, h->h_xform.reserve(n * (sizeof(float4) + sizeof(float))));  // pinned (round 4: two fresh pageable vectors per call)
  const float* xyzw = h->h_xform.as<float>();
  const float* inten = xyzw + 4 * n;
  HGS_HIP(h, hipMemcpyAsync(h->h_xform.p, c->desc.raw, n * sizeof(float4), hipMemcpyDeviceToHost, h->stream));
  HGS_HIP(h, hipMemcpyAsync(h->h_xform.as<float>() + 4 * n, c->intensity, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HGS_HIP(h, hipStreamSynchronize(h->stream));
  char* o = (char*)out_pts;
  for (size_t i = 0; i < n; i++) {
    float* f = reinterpret_cast<float*>(o + i * stride_bytes);
    f[0] = xyzw[4 * i], f[1] = xyzw[4 * i + 1], f[2] = xyzw[4 * i + 2];
    if (stride_bytes >= 16) f[3] = 1.0f;
    if (stride_bytes >= 20) f[4] = inten[i];
  }
  return HGS_OK;
} catch (...) {
  return status_of_current_exception((c ? c->owner : nullptr));
}

// ---- map cloud (src/hdl_graph_slam/map_cloud_generator.cpp:13-51) --------------------------------------------
extern "C" int hgs_map_cloud_generate(hgs_handle* h, hgs_cloud* const* keyframes, const float* poses /* 16 * n, column-major */, size_t n_keyframes,
                                      double resolution, hgs_cloud** out) try {
  ApiLock lock(h);
  if (!h || !out || (n_keyframes > 0 && (!keyframes || !poses))) return HGS_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  size_t total = 0;
  int max_n = 0;
  for (size_t k = 0; k < n_keyframes; k++) {
    if (!keyframes[k] || keyframes[k]->owner != h) return HGS_ERR_INVALID_ARGUMENT;
    total += keyframes[k]->n_input;
    max_n = std::max(max_n, (int)keyframes[k]->n_input);
  }
  if (total > (size_t)1 << 30) return HGS_ERR_INVALID_ARGUMENT;
  HGS_TRY(set_device(h));
  StageTimer tm(h, HGS_STAGE_PREFILTER);
  const size_t cap = std::max<size_t>(total, 1);
  HGS_HIP(h, h->pf_a.reserve(cap * sizeof(float4)));
  HGS_HIP(h, h->pf_b.reserve(cap * sizeof(float4)));
  HGS_HIP(h, h->pf_keep.reserve(cap * sizeof(uint32_t)));
  HGS_HIP(h, h->pf_slot.reserve(cap * sizeof(uint32_t)));
  HGS_HIP(h, h->pf_small.reserve(256 + sizeof(MapOctree)));
  HGS_HIP(h, h->h_small.reserve(std::max<size_t>(64, sizeof(MapOctree))));
  float4* all = h->pf_a.as<float4>();
  if (n_keyframes > 0 && total > 0) {
    std::vector<MapSource> srcs(n_keyframes);
    size_t off = 0;
    for (size_t k = 0; k < n_keyframes; k++) {
      srcs[k].raw = keyframes[k]->desc.raw, srcs[k].intensity = keyframes[k]->intensity;
      srcs[k].n = (int)keyframes[k]->n_input, srcs[k].offset = (int)off;
      std::memcpy(srcs[k].T, poses + 16 * k, sizeof(float) * 16);
      off += keyframes[k]->n_input;
    }
    HGS_HIP(h, h->misc.reserve(n_keyframes * sizeof(MapSource)));
    HGS_HIP(h, hipMemcpyAsync(h->misc.p, srcs.data(), n_keyframes * sizeof(MapSource), hipMemcpyHostToDevice, h->stream));
    launch_map_transform(h->stream, h->misc.as<MapSource>(), (int)n_keyframes, max_n, all);
    HGS_HIP(h, hipStreamSynchronize(h->stream));  // `srcs` is pageable host memory
  }
  size_t m = total;
  float4* result = all;
  if (resolution > 0.0 && total > 0) {
    int* d_count = h->pf_small.as<int>();
    MapOctree* d_oct = reinterpret_cast<MapOctree*>(h->pf_small.as<char>() + 256);
    MapOctree* h_oct = reinterpret_cast<MapOctree*>(h->h_small.p);
    const int n = (int)total;
    // replay the octree's bounding box: one round per point that forced the box to double (at most one per tree level), each a
    // grid-wide "first point outside" search and a one-thread update; the host only watches the done flag (map clouds are
    // generated every few seconds)
    std::memset(h_oct, 0, sizeof(MapOctree));
    h_oct->first = 0x7fffffff;
    HGS_HIP(h, hipMemcpyAsync(d_oct, h_oct, sizeof(MapOctree), hipMemcpyHostToDevice, h->stream));
    launch_map_first_finite(h->stream, all, n, d_oct);
    launch_map_octree_init(h->stream, all, n, resolution, d_oct);
    for (int round = 0; round <= kMapMaxEvents; round++) {
      launch_map_octree_step(h->stream, all, n, resolution, d_oct);
      HGS_HIP(h, hipMemcpyAsync(h_oct, d_oct, sizeof(MapOctree), hipMemcpyDeviceToHost, h->stream));
      HGS_HIP(h, hipStreamSynchronize(h->stream));
      if (h_oct->done) break;
    }
    if (h_oct->overflow || !h_oct->done) {
      h->err = "map cloud: resolution too fine for the extent of the map (the octree would be deeper than 21 levels)";
      return HGS_ERR_INVALID_ARGUMENT;
    }
    HGS_TRY(reserve_sort_pairs(h, total));
    // interleaved keys use 3 * depth bits; one more so that the all-ones key of a non-finite point sorts behind every voxel
    const int key_bits = h_oct->n_events > 0 ? 3 * h_oct->events[h_oct->n_events - 1].depth + 1 : 1;
    launch_map_keys(h->stream, all, n, resolution, d_oct, h->sort_keys[0].as<unsigned long long>(), h->sort_vals[0].as<unsigned>());
    HGS_TRY(sort_pairs(h, total, 0, key_bits));
    launch_pf_voxel_heads(h->stream, h->sort_keys[1].as<unsigned long long>(), n, h->pf_keep.as<unsigned>(), kMapInvalidKey);
    HGS_TRY(scan_u32(h, h->pf_keep.as<uint32_t>(), h->pf_slot.as<uint32_t>(), total));
    launch_map_centers(h->stream, h->sort_keys[1].as<unsigned long long>(), h->pf_keep.as<unsigned>(), h->pf_slot.as<unsigned>(), n, resolution, d_oct,
                       h->pf_b.as<float4>(), d_count);
    HGS_HIP(h, hipGetLastError());
    int* hs = h->h_small.as<int>();
    HGS_HIP(h, hipMemcpyAsync(hs, d_count, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HGS_HIP(h, hipStreamSynchronize(h->stream));
    m = (size_t)std::max(0, hs[0]);
    result = h->pf_b.as<float4>();
  }
  HGS_HIP(h, hipGetLastError());
  return cloud_from_device(h, result, m, out);
} catch (...) {
  return status_of_current_exception(h);
}

// ---- floor detection (apps/floor_detection_nodelet.cpp:110-238) ----------------------------------------------
extern "C" int hgs_floor_params_default(hgs_floor_params* p) try {
  if (!p) return HGS_ERR_INVALID_ARGUMENT;
  std::memset(p, 0, sizeof(*p));
  p->tilt_deg = 0.0;               // floor_detection_nodelet.cpp:57
  p->sensor_height = 2.0;          // :58
  p->height_clip_range = 1.0;      // :59
  p->floor_pts_thresh = 512;       // :60
  p->floor_normal_thresh = 10.0;   // :61
  p->use_normal_filtering = 1;     // :62
  p->normal_filter_thresh = 20.0;  // :63
  p->normal_k = 10;                // :219
  p->ransac_max_iterations = 1000;     // pcl::SampleConsensus
  p->ransac_distance_threshold = 0.1;  // :140
  p->ransac_probability = 0.99;        // pcl::SampleConsensus
  p->seed = 0;
  return HGS_OK;
} catch (...) {
  return status_of_current_exception(nullptr);
}

namespace {

bool floor_params_valid(const hgs_floor_params* p) {
  return std::isfinite(p->tilt_deg) && std::isfinite(p->sensor_height) && std::isfinite(p->height_clip_range) && p->height_clip_range >= 0 && p->floor_pts_thresh >= 0 &&
         std::isfinite(p->floor_normal_thresh) && p->floor_normal_thresh >= 0 && std::isfinite(p->normal_filter_thresh) && p->normal_filter_thresh >= 0 &&
         p->normal_k >= 3 && p->normal_k <= 64 && p->ransac_max_iterations >= 0 && std::isfinite(p->ransac_distance_threshold) && p->ransac_distance_threshold >= 0 &&
         p->ransac_probability > 0 && p->ransac_probability < 1;
}

struct FloorWork {
  float4* filtered = nullptr;  // the RANSAC input {x, y, z, intensity}, input order (pf_a or pf_b)
  float4* spare = nullptr;     // the other of the two
  size_t n_clipped = 0, n_filtered = 0;
  hgs_cloud* clipped = nullptr;  // the clipped cloud with its index (normal filter only); the caller frees it
};

// flags in pf_keep -> stable compaction of `in` into `out`; *m = the number kept (one read-back)
int floor_compact(hgs_handle* h, const float4* in, size_t n, float4* out, size_t* m) {
  int* d_count = h->pf_small.as<int>();
  HGS_TRY(scan_u32(h, h->pf_keep.as<uint32_t>(), h->pf_slot.as<uint32_t>(), n));
  launch_pf_compact(h->stream, in, (int)n, h->pf_keep.as<unsigned>(), h->pf_slot.as<unsigned>(), out, d_count);
  HGS_HIP(h, hipGetLastError());
  int* hs = h->h_small.as<int>();
  HGS_HIP(h, hipMemcpyAsync(hs, d_count, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HGS_HIP(h, hipStreamSynchronize(h->stream));
  *m = (size_t)std::max(0, hs[0]);
  return HGS_OK;
}

// clip + normal filter of steps 1 and 2; keep_clip / keep_normal / normals (host, may be null): the stage hook's outputs
int floor_filter(hgs_handle* h, hgs_cloud* cloud, const hgs_floor_params* p, const FloorConsts& c, FloorWork* w, uint8_t* keep_clip, uint8_t* keep_normal, double* normals3) {
  const size_t n = cloud->n_input;
  const size_t cap = std::max<size_t>(n, 1);
  HGS_HIP(h, h->pf_a.reserve(cap * sizeof(float4)));
  HGS_HIP(h, h->pf_b.reserve(cap * sizeof(float4)));
  HGS_HIP(h, h->pf_keep.reserve(cap * sizeof(uint32_t)));
  HGS_HIP(h, h->pf_slot.reserve(cap * sizeof(uint32_t)));
  HGS_HIP(h, h->pf_small.reserve(256));
  HGS_HIP(h, h->h_small.reserve(256));
  float4* all = h->pf_a.as<float4>();
  float4* clipped = h->pf_b.as<float4>();
  w->filtered = clipped, w->spare = all;
  w->n_clipped = w->n_filtered = 0;
  std::vector<uint32_t> flags;
  if (keep_clip) std::memset(keep_clip, 0, n);
  if (keep_normal) std::memset(keep_normal, 0, n);
  if (normals3)
    for (size_t i = 0; i < 3 * n; i++) normals3[i] = std::numeric_limits<double>::quiet_NaN();
  if (n == 0) return HGS_OK;
  launch_floor_clip_flags(h->stream, cloud->desc.raw, cloud->intensity, (int)n, c, all, h->pf_keep.as<unsigned>());
  if (keep_clip || keep_normal || normals3) {
    flags.resize(n);
    HGS_HIP(h, hipMemcpyAsync(flags.data(), h->pf_keep.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  }
  HGS_TRY(floor_compact(h, all, n, clipped, &w->n_clipped));
  const size_t m = w->n_clipped;
  w->n_filtered = m;
  if (keep_clip)
    for (size_t i = 0; i < n; i++) keep_clip[i] = flags[i] ? 1 : 0;
  if (!p->use_normal_filtering) {
    if (keep_normal)
      for (size_t i = 0; i < n; i++) keep_normal[i] = flags[i] ? 1 : 0;
    return HGS_OK;
  }
  if (!floor_normals_defined(m)) {  // NaN normals: nothing passes (keep_normal and normals3 are already 0 / NaN)
    w->n_filtered = 0;
    return HGS_OK;
  }
  // normal_filtering (:211-238): the clipped cloud gets a search index, k_knn_cov stages every point's fp64 neighbourhood covariance over its exact
  // min(normal_k, n_clipped) nearest neighbours (itself included; a list of k slots never fills in a smaller cloud), k_floor_normal_flags takes the
  // eigenvector of the smallest eigenvalue and tests it.  The viewpoint flip of pcl::NormalEstimation (:220) is irrelevant under |.| and not computed.
  HGS_TRY(cloud_from_device(h, clipped, m, &w->clipped));
  std::vector<hgs_cloud*> one{w->clipped};
  HGS_TRY(ensure_index(h, one));
  const int k = (int)std::min<size_t>((size_t)p->normal_k, m);
  const int gather = h->knn_replay >= 0 ? h->knn_replay : 2;
  int qpw = queries_per_wave(m, 32, h->knn_qpw_tiny, (size_t)h->knn_tiny_below);
  if (qpw < 32 && (gather != 2 || k > 20)) qpw = 32;
  HGS_HIP(h, h->cov_raw.reserve(m * 6 * sizeof(double)));
  double* d_normals = nullptr;
  if (normals3) {
    HGS_HIP(h, h->pf_dist.reserve(m * 3 * sizeof(double)));
    d_normals = h->pf_dist.as<double>();
  }
  const CloudDesc* d_descs = nullptr;
  HGS_TRY(upload_descs(h, one, false, &d_descs, nullptr));
  launch_knn_cov_raw(h->stream, d_descs, (int)m, k, qpw, gather, h->cov_raw.as<double>());
  HGS_HIP(h, hipMemsetAsync(h->pf_keep.p, 0, m * sizeof(uint32_t), h->stream));
  launch_floor_normal_flags(h->stream, w->clipped->desc, h->cov_raw.as<double>(), c, h->pf_keep.as<unsigned>(), d_normals);
  std::vector<uint32_t> nflags;
  std::vector<double> nrm;
  if (keep_normal || normals3) {
    nflags.resize(m);
    HGS_HIP(h, hipMemcpyAsync(nflags.data(), h->pf_keep.p, m * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    if (normals3) {
      nrm.resize(3 * m);
      HGS_HIP(h, hipMemcpyAsync(nrm.data(), d_normals, 3 * m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    }
  }
  HGS_TRY(floor_compact(h, clipped, m, all, &w->n_filtered));
  w->filtered = all, w->spare = clipped;
  if (keep_normal || normals3) {
    size_t j = 0;  // the j-th clipped point is the j-th input point with its clip flag set
    for (size_t i = 0; i < n && j < m; i++) {
      if (!flags[i]) continue;
      if (keep_normal) keep_normal[i] = nflags[j] ? 1 : 0;
      if (normals3) normals3[3 * i] = nrm[3 * j], normals3[3 * i + 1] = nrm[3 * j + 1], normals3[3 * i + 2] = nrm[3 * j + 2];
      j++;
    }
  }
  return HGS_OK;
}

// device work space of the RANSAC rounds inside h->misc: the state, one chunk's counts and planes
struct FloorRansacBufs {
  FloorRansacState* state;
  int* counts;
  double* planes;
};
int floor_ransac_bufs(hgs_handle* h, int chunk, FloorRansacBufs* b) {
  const size_t o_counts = 256, o_planes = o_counts + align_up((size_t)chunk * sizeof(int), 256);
  HGS_HIP(h, h->misc.reserve(o_planes + (size_t)chunk * 4 * sizeof(double)));
  b->state = reinterpret_cast<FloorRansacState*>(h->misc.as<char>());
  b->counts = reinterpret_cast<int*>(h->misc.as<char>() + o_counts);
  b->planes = reinterpret_cast<double*>(h->misc.as<char>() + o_planes);
  return HGS_OK;
}

// the acceptance tests (:147-166) on a finished search and the number of its model's inliers: fills n_inliers, ransac_iterations, reason, detected, coeffs
void floor_accept(const hgs_floor_params* p, const FloorConsts& c, const FloorRansacState& st, size_t n_in, hgs_floor_result* out) {
  out->n_inliers = (uint32_t)n_in;
  out->ransac_iterations = st.iterations;
  float co[4] = {(float)st.plane[0], (float)st.plane[1], (float)st.plane[2], (float)st.plane[3]};
  if (n_in < (size_t)p->floor_pts_thresh || st.best_i < 0) {  // :147
    out->reason = HGS_FLOOR_TOO_FEW_INLIERS;
    return;
  }
  // verticality (:152-161) against r = R^-1 e_z, then the upward flip (:164-166)
  const double dot = (double)co[0] * c.nrx + (double)co[2] * c.nrz;
  if (std::fabs(dot) < std::cos(p->floor_normal_thresh * M_PI / 180.0)) {
    out->reason = HGS_FLOOR_NOT_VERTICAL;
    return;
  }
  if (co[2] < 0.f)
    for (float& v : co) v = -v;
  for (int i = 0; i < 4; i++) out->coeffs[i] = co[i];
  out->detected = 1, out->reason = HGS_FLOOR_DETECTED;
}

int detect_floor_locked(hgs_handle* h, hgs_cloud* cloud, const hgs_floor_params* p, hgs_floor_result* out, hgs_cloud** filtered_out, hgs_cloud** inliers_out, FloorWork& w) {
  StageTimer tm(h, HGS_STAGE_PREFILTER);
  const FloorConsts c = floor_consts(p);
  HGS_TRY(floor_filter(h, cloud, p, c, &w, nullptr, nullptr, nullptr));
  out->n_clipped = (uint32_t)w.n_clipped, out->n_filtered = (uint32_t)w.n_filtered;
  const size_t nf = w.n_filtered;
  if (filtered_out) HGS_TRY(cloud_from_device(h, w.filtered, nf, filtered_out));  // floor_filtered_pub (:127-130): published before the point-count test
  if (nf == 0 || nf < (size_t)p->floor_pts_thresh) {  // :133 (an empty cloud / an empty clip range: not detected)
    out->reason = HGS_FLOOR_TOO_FEW_POINTS;
    return HGS_OK;
  }
  // RANSAC (:138-141) in rounds of `floor_chunk` hypotheses, driven like the engine's optimiser rounds: the decide kernel ticks the host-mapped
  // progress mirror, the host stops enqueueing when it reads `done`, rounds that were queued behind it find the flag and return
  const int chunk = std::max(1, std::min(kFloorMaxChunk, h->floor_chunk));
  FloorRansacBufs b;
  HGS_TRY(floor_ransac_bufs(h, chunk, &b));
  std::vector<BatchLane> lanes(1);
  lanes[0].stream = h->stream, lanes[0].b0 = 0, lanes[0].B = 1;
  HGS_TRY(make_progress(h, 0, 1, &lanes[0].prog));
  launch_floor_ransac_init(h->stream, b.state, c.max_iterations, lanes[0].prog);
  const long max_rounds = ((long)c.max_iterations + chunk - 1) / chunk;
  const float4* pts = w.filtered;
  drive_lanes(
      lanes, max_rounds,
      [&](BatchLane& L) {
        const int i0 = (int)L.round * chunk;
        const int nh = std::min(chunk, c.max_iterations - i0);
        launch_floor_ransac_planes(h->stream, pts, (int)nf, c.seed, i0, nh, b.state, b.planes, b.counts);
        launch_floor_ransac_count(h->stream, pts, (int)nf, c.dist_thresh, b.planes, nh, b.state, b.counts);
        launch_floor_ransac_decide(h->stream, b.counts, b.planes, i0, nh, (int)nf, c.max_iterations, c.log_prob, b.state, L.prog);
      },
      [&](BatchLane&) {});
  // the model = the best plane rounded to float (no refinement: the reference never calls one); its inliers in order (:143-144)
  launch_floor_inlier_flags(h->stream, pts, (int)nf, b.state, c.dist_thresh, h->pf_keep.as<unsigned>());
  size_t n_in = 0;
  HGS_TRY(floor_compact(h, pts, nf, w.spare, &n_in));
  FloorRansacState st;
  HGS_HIP(h, hipMemcpyAsync(&st, b.state, sizeof(st), hipMemcpyDeviceToHost, h->stream));
  HGS_HIP(h, hipStreamSynchronize(h->stream));
  floor_accept(p, c, st, n_in, out);
  if (out->detected && inliers_out) HGS_TRY(cloud_from_device(h, w.spare, n_in, inliers_out));  // floor_points_pub (:168-177)
  return HGS_OK;
}

// ---- several clouds in one batch (include/hgs_registration.h; the k_flb_* kernels of hgs_kernels.hip) ---------------------------------------
// What the RANSAC rounds' counts and planes may take of h->misc (36 bytes per cloud and hypothesis of a chunk): more clouds run in groups, one after
// the other.  The staged covariances of the normal filter (48 bytes per clipped point of the longest cloud of a launch, per cloud) likewise.
constexpr size_t kFloorBatchWorkBytes = (size_t)64 << 20, kFloorBatchCovBytes = (size_t)256 << 20;

// the table's counts (and whatever else the caller has queued for the host) in ONE copy and ONE synchronisation
int floor_batch_readback(hgs_handle* h, size_t table_bytes) {
  HGS_HIP(h, hipGetLastError());
  HGS_HIP(h, hipMemcpyAsync(h->h_pf_table.p, h->pf_table.p, table_bytes, hipMemcpyDeviceToHost, h->stream));
  HGS_HIP(h, hipStreamSynchronize(h->stream));
  h->fb_readbacks++;
  return HGS_OK;
}

// New resident clouds of counts[i] points from in[offs[i] ..): allocated here (out[i]; on a failure the caller frees what is there), made resident by ONE
// k_flb_to_cloud and ONE k_bbox_count.
int floor_batch_clouds(hgs_handle* h, const float4* in, const std::vector<int>& offs, const std::vector<size_t>& counts, hgs_cloud** out) {
  const size_t K = offs.size();
  if (K == 0) return HGS_OK;
  size_t max_m = 0;
  for (size_t i = 0; i < K; i++) {
    HGS_TRY(cloud_alloc(h, counts[i], &out[i]));
    max_m = std::max(max_m, counts[i]);
  }
  const size_t o_out = align_up(K * sizeof(CloudDesc), 16), o_int = o_out + K * sizeof(CloudDesc*), o_off = o_int + K * sizeof(float*), bytes = o_off + K * sizeof(int);
  HGS_HIP(h, h->descs.reserve(bytes));
  void* staged = nullptr;
  int ring_slot = 0;
  HGS_HIP(h, h->up.stage(bytes, &staged, &ring_slot));
  char* hb = static_cast<char*>(staged);
  for (size_t i = 0; i < K; i++) {
    reinterpret_cast<CloudDesc*>(hb)[i] = resident_desc(out[i]);
    reinterpret_cast<CloudDesc**>(hb + o_out)[i] = out[i]->dev_desc;
    reinterpret_cast<float**>(hb + o_int)[i] = out[i]->intensity;
    reinterpret_cast<int*>(hb + o_off)[i] = offs[i];
  }
  HGS_HIP(h, hipMemcpyAsync(h->descs.p, hb, bytes, hipMemcpyHostToDevice, h->stream));
  HGS_HIP(h, h->up.commit(ring_slot, h->stream));
  char* db = h->descs.as<char>();
  launch_flb_to_cloud(h->stream, in, reinterpret_cast<const CloudDesc*>(db), reinterpret_cast<CloudDesc* const*>(db + o_out), reinterpret_cast<float* const*>(db + o_int),
                      reinterpret_cast<const int*>(db + o_off), (int)K, (int)max_m);
  launch_bbox_count(h->stream, reinterpret_cast<const CloudDesc*>(db), (int)K, (int)max_m);
  HGS_HIP(h, hipGetLastError());
  return HGS_OK;
}

// The normal filter of every clipped cloud: one launch of the new clouds, one index build, then k_knn_cov + the normal flags in one launch per set of
// clouds that share k = min(normal_k, n_clipped) and the packet size the single call gives a cloud of that size (queries_per_wave) — the kernel takes one
// of each per launch, and a cloud's sums are those of hgs_detect_floor only under the same two.  Sweeps of one sensor share both.
int floor_batch_normals(hgs_handle* h, const hgs_floor_params* p, const FloorConsts& c, const std::vector<size_t>& off, const std::vector<size_t>& n_clipped,
                        std::vector<hgs_cloud*>& clipped) {
  struct Entry {
    int sweep, k, qpw;
  };
  const int gather = h->knn_replay >= 0 ? h->knn_replay : 2;
  std::vector<Entry> es;
  for (size_t i = 0; i < n_clipped.size(); i++) {
    const size_t m = n_clipped[i];
    if (!floor_normals_defined(m)) continue;  // NaN normals: its flags stay 0 as the caller cleared them
    const int k = (int)std::min<size_t>((size_t)p->normal_k, m);
    int qpw = queries_per_wave(m, 32, h->knn_qpw_tiny, (size_t)h->knn_tiny_below);
    if (qpw < 32 && (gather != 2 || k > 20)) qpw = 32;
    es.push_back(Entry{(int)i, k, qpw});
  }
  const size_t K = es.size();
  if (K == 0) return HGS_OK;
  std::stable_sort(es.begin(), es.end(), [](const Entry& a, const Entry& b) { return a.k != b.k ? a.k > b.k : a.qpw < b.qpw; });
  std::vector<int> offs(K);
  std::vector<size_t> counts(K);
  for (size_t j = 0; j < K; j++) offs[j] = (int)off[es[j].sweep], counts[j] = n_clipped[es[j].sweep];
  clipped.assign(K, nullptr);
  HGS_TRY(floor_batch_clouds(h, h->pf_b.as<float4>(), offs, counts, clipped.data()));
  HGS_TRY(ensure_index(h, clipped));
  // the launches: runs of equal (k, qpw), cut where the staged covariances would pass kFloorBatchCovBytes
  struct Run {
    size_t a, b, max_m;
  };
  std::vector<Run> runs;
  size_t stage_doubles = 0;
  for (size_t a = 0; a < K;) {
    size_t b = a, max_m = 0;
    while (b < K && es[b].k == es[a].k && es[b].qpw == es[a].qpw) {
      const size_t mm = std::max(max_m, counts[b]);
      if (b > a && (b - a + 1) * mm * 6 * sizeof(double) > kFloorBatchCovBytes) break;
      max_m = mm, b++;
    }
    runs.push_back(Run{a, b, max_m});
    stage_doubles = std::max(stage_doubles, (b - a) * max_m * 6);
    a = b;
  }
  HGS_HIP(h, h->cov_raw.reserve(stage_doubles * sizeof(double)));
  HGS_HIP(h, h->pf_small.reserve(256 + K * sizeof(int)));
  int* d_keep_off = reinterpret_cast<int*>(h->pf_small.as<char>() + 256);
  HGS_HIP(h, h->up.upload(d_keep_off, offs.data(), K * sizeof(int), h->stream));
  const CloudDesc* d_descs = nullptr;
  HGS_TRY(upload_descs(h, clipped, false, &d_descs, nullptr));
  for (const Run& r : runs)
    launch_flb_normals(h->stream, d_descs + r.a, (int)(r.b - r.a), (int)r.max_m, es[r.a].k, es[r.a].qpw, gather, h->cov_raw.as<double>(), d_keep_off + r.a, c,
                       h->pf_keep.as<unsigned>());
  HGS_HIP(h, hipGetLastError());
  return HGS_OK;
}

int detect_floor_batch_impl(hgs_handle* h, hgs_cloud* const* clouds, size_t S, const hgs_floor_params* p, hgs_floor_result* out, hgs_cloud** filtered_out,
                            hgs_cloud** inliers_out, std::vector<hgs_cloud*>& clipped) {
  StageTimer tm(h, HGS_STAGE_PREFILTER);
  const FloorConsts c = floor_consts(p);
  std::vector<size_t> off(S + 1, 0);
  size_t max_n = 0;
  for (size_t i = 0; i < S; i++) off[i + 1] = off[i] + clouds[i]->n_input, max_n = std::max(max_n, clouds[i]->n_input);
  const size_t total = off[S], cap = std::max<size_t>(total, 1), table_bytes = S * sizeof(FloorSweep);
  HGS_HIP(h, h->pf_a.reserve(cap * sizeof(float4)));
  HGS_HIP(h, h->pf_b.reserve(cap * sizeof(float4)));
  HGS_HIP(h, h->pf_keep.reserve(cap * sizeof(uint32_t)));
  HGS_HIP(h, h->pf_slot.reserve(cap * sizeof(uint32_t)));
  HGS_HIP(h, h->pf_table.reserve(table_bytes));
  HGS_HIP(h, h->h_pf_table.reserve(table_bytes));
  FloorSweep* d_sweeps = h->pf_table.as<FloorSweep>();
  const FloorSweep* hs = h->h_pf_table.as<FloorSweep>();
  float4* all = h->pf_a.as<float4>();
  float4* clip = h->pf_b.as<float4>();
  unsigned* keep = h->pf_keep.as<unsigned>();
  unsigned* slot = h->pf_slot.as<unsigned>();
  const int nS = (int)S, mx = (int)max_n;
  std::vector<size_t> n_clipped(S, 0), n_filtered(S, 0);
  float4 *filtered = clip, *spare = all;
  if (total > 0) {
    std::vector<FloorSweep> t(S);
    for (size_t i = 0; i < S; i++) t[i] = FloorSweep{clouds[i]->desc.raw, clouds[i]->intensity, (int)off[i], (int)clouds[i]->n_input, 0, 0, 0, 0};
    HGS_HIP(h, h->up.upload(d_sweeps, t.data(), table_bytes, h->stream));
    // steps 1 and 2 of floor_filter, every cloud in its slice: ONE scan per compaction, the counts of all clouds in ONE read-back of the table
    launch_flb_clip_flags(h->stream, d_sweeps, nS, mx, c, all, keep);
    HGS_TRY(scan_u32(h, keep, slot, total));
    launch_flb_compact(h->stream, all, d_sweeps, nS, mx, kFlbClip, keep, slot, clip);
    HGS_TRY(floor_batch_readback(h, table_bytes));
    for (size_t i = 0; i < S; i++) n_clipped[i] = n_filtered[i] = (size_t)std::max(0, hs[i].n_clipped);
    if (p->use_normal_filtering && std::any_of(n_clipped.begin(), n_clipped.end(), [](size_t m) { return m > 0; })) {
      HGS_HIP(h, hipMemsetAsync(keep, 0, total * sizeof(uint32_t), h->stream));
      HGS_TRY(floor_batch_normals(h, p, c, off, n_clipped, clipped));
      HGS_TRY(scan_u32(h, keep, slot, total));
      launch_flb_compact(h->stream, clip, d_sweeps, nS, mx, kFlbNormal, keep, slot, all);
      HGS_TRY(floor_batch_readback(h, table_bytes));
      for (size_t i = 0; i < S; i++) n_filtered[i] = (size_t)std::max(0, hs[i].n_filtered);
      filtered = all, spare = clip;
    }
  }
  std::vector<int> offs(S);
  for (size_t i = 0; i < S; i++) {
    offs[i] = (int)off[i];
    out[i].n_clipped = (uint32_t)n_clipped[i], out[i].n_filtered = (uint32_t)n_filtered[i];
    out[i].reason = HGS_FLOOR_TOO_FEW_POINTS;  // :133 (an empty cloud / an empty clip range: not detected); the clouds that enter RANSAC get theirs below
  }
  if (filtered_out) HGS_TRY(floor_batch_clouds(h, filtered, offs, n_filtered, filtered_out));  // floor_filtered_pub (:127-130)
  // RANSAC (:138-141): job j = the j-th cloud that passes the point-count test (:133).  One BatchLane per group of jobs with Progress::B = the group's
  // jobs: each of them ticks once per round (k_flb_ransac_decide, one wave per job) and `finished` in the round that sets its `done`; the clouds that
  // did not enter have no job, no wave and no tick.
  std::vector<int> job_sweep;
  std::vector<FloorJob> jobs;
  size_t max_nf = 0;
  for (size_t i = 0; i < S; i++)
    if (n_filtered[i] > 0 && n_filtered[i] >= (size_t)p->floor_pts_thresh) {
      job_sweep.push_back((int)i);
      jobs.push_back(FloorJob{(int)off[i], (int)n_filtered[i]});
      max_nf = std::max(max_nf, n_filtered[i]);
    }
  const size_t R = jobs.size();
  h->fb_ransac_clouds = (int)R;
  if (R == 0) return HGS_OK;
  const int chunk = std::max(1, std::min(kFloorMaxChunk, h->floor_chunk));
  const size_t per_job = (size_t)chunk * (sizeof(int) + 4 * sizeof(double));
  size_t G = std::max<size_t>(1, kFloorBatchWorkBytes / per_job);
  if (h->floor_batch_group > 0) G = std::min(G, (size_t)h->floor_batch_group);
  G = std::min(G, R);
  const size_t o_jobs = align_up(R * sizeof(FloorRansacState), 256), o_counts = o_jobs + align_up(R * sizeof(FloorJob), 256),
               o_planes = o_counts + align_up(G * chunk * sizeof(int), 256);
  HGS_HIP(h, h->misc.reserve(o_planes + G * chunk * 4 * sizeof(double)));
  HGS_HIP(h, h->h_small.reserve(std::max<size_t>(256, R * sizeof(FloorRansacState))));
  FloorRansacState* d_states = reinterpret_cast<FloorRansacState*>(h->misc.as<char>());
  FloorJob* d_jobs = reinterpret_cast<FloorJob*>(h->misc.as<char>() + o_jobs);
  int* d_counts = reinterpret_cast<int*>(h->misc.as<char>() + o_counts);
  double* d_planes = reinterpret_cast<double*>(h->misc.as<char>() + o_planes);
  HGS_HIP(h, h->up.upload(d_jobs, jobs.data(), R * sizeof(FloorJob), h->stream));
  const long max_rounds = ((long)c.max_iterations + chunk - 1) / chunk;
  for (size_t g0 = 0; g0 < R; g0 += G) {
    const int ng = (int)std::min(G, R - g0);
    if (g0 > 0) {  // make_progress resets the mirror: the rounds still queued for the group in front (they tick it) have to be through
      HGS_HIP(h, hipStreamSynchronize(h->stream));
      h->fb_readbacks++;
    }
    int group_max = 0;
    for (int j = 0; j < ng; j++) group_max = std::max(group_max, jobs[g0 + j].n);
    std::vector<BatchLane> lanes(1);
    lanes[0].stream = h->stream, lanes[0].b0 = (int)g0, lanes[0].B = ng;
    HGS_TRY(make_progress(h, 0, ng, &lanes[0].prog));
    launch_flb_ransac_init(h->stream, d_states + g0, ng, c.max_iterations, lanes[0].prog);
    drive_lanes(
        lanes, max_rounds,
        [&](BatchLane& L) {
          const int i0 = (int)L.round * chunk;
          const int nh = std::min(chunk, c.max_iterations - i0);
          launch_flb_ransac_planes(h->stream, filtered, d_jobs + g0, ng, c.seed, i0, nh, chunk, d_states + g0, d_planes, d_counts);
          launch_flb_ransac_count(h->stream, filtered, d_jobs + g0, ng, group_max, c.dist_thresh, d_planes, nh, chunk, d_states + g0, d_counts);
          launch_flb_ransac_decide(h->stream, d_counts, d_planes, d_jobs + g0, ng, i0, nh, chunk, c.max_iterations, c.log_prob, d_states + g0, L.prog);
          h->fb_rounds++;
        },
        [&](BatchLane&) {});
  }
  // every job's inliers from its own float-rounded model (:143-144), ONE scan, ONE compaction; counts and states in ONE read-back
  HGS_HIP(h, hipMemsetAsync(keep, 0, total * sizeof(uint32_t), h->stream));
  launch_flb_inlier_flags(h->stream, filtered, d_jobs, (int)R, (int)max_nf, d_states, c.dist_thresh, keep);
  HGS_TRY(scan_u32(h, keep, slot, total));
  launch_flb_compact(h->stream, filtered, d_sweeps, nS, mx, kFlbInliers, keep, slot, spare);
  const FloorRansacState* st = h->h_small.as<FloorRansacState>();
  HGS_HIP(h, hipMemcpyAsync(h->h_small.p, d_states, R * sizeof(FloorRansacState), hipMemcpyDeviceToHost, h->stream));
  HGS_TRY(floor_batch_readback(h, table_bytes));
  std::vector<int> in_offs, in_sweep;
  std::vector<size_t> in_counts;
  for (size_t j = 0; j < R; j++) {
    const int i = job_sweep[j];
    const size_t n_in = (size_t)std::max(0, hs[i].n_inliers);
    floor_accept(p, c, st[j], n_in, &out[i]);
    if (out[i].detected && inliers_out) in_offs.push_back((int)off[i]), in_counts.push_back(n_in), in_sweep.push_back(i);
  }
  std::vector<hgs_cloud*> in_clouds(in_offs.size(), nullptr);
  const int rc = floor_batch_clouds(h, spare, in_offs, in_counts, in_clouds.data());  // floor_points_pub (:168-177)
  for (size_t k = 0; k < in_clouds.size(); k++) inliers_out[in_sweep[k]] = in_clouds[k];  // (a failure: the caller frees them with the array)
  return rc;
}

}  // namespace

extern "C" int hgs_detect_floor(hgs_handle* h, hgs_cloud* cloud, const hgs_floor_params* p, hgs_floor_result* out, hgs_cloud** filtered_out, hgs_cloud** inliers_out) try {
  ApiLock lock(h);
  if (filtered_out) *filtered_out = nullptr;
  if (inliers_out) *inliers_out = nullptr;
  if (!h || !cloud || !p || !out || cloud->owner != h || !floor_params_valid(p)) return HGS_ERR_INVALID_ARGUMENT;
  HGS_TRY(set_device(h));
  std::memset(out, 0, sizeof(*out));
  FloorWork w;
  const int rc = detect_floor_locked(h, cloud, p, out, filtered_out, inliers_out, w);
  cloud_free(w.clipped);
  if (rc != HGS_OK) {
    if (filtered_out && *filtered_out) cloud_free(*filtered_out), *filtered_out = nullptr;
    if (inliers_out && *inliers_out) cloud_free(*inliers_out), *inliers_out = nullptr;
  }
  return rc;
} catch (...) {
  return status_of_current_exception(h);
}

extern "C" int hgs_detect_floor_batch(hgs_handle* h, hgs_cloud* const* clouds, size_t n_clouds, const hgs_floor_params* p, hgs_floor_result* out,
                                      hgs_cloud** filtered_out, hgs_cloud** inliers_out) try {
  ApiLock lock(h);
  for (size_t i = 0; i < n_clouds; i++) {
    if (filtered_out) filtered_out[i] = nullptr;
    if (inliers_out) inliers_out[i] = nullptr;
  }
  if (!h || !p || !floor_params_valid(p)) return HGS_ERR_INVALID_ARGUMENT;
  h->fb_clouds = h->fb_ransac_clouds = h->fb_rounds = h->fb_readbacks = 0;
  if (n_clouds == 0) return HGS_OK;
  if (!clouds || !out) return HGS_ERR_INVALID_ARGUMENT;
  if (n_clouds > HGS_FLOOR_BATCH_MAX_CLOUDS) {
    h->err = "hgs_detect_floor_batch: more than " + std::to_string(HGS_FLOOR_BATCH_MAX_CLOUDS) + " clouds in one call";
    return HGS_ERR_INVALID_ARGUMENT;
  }
  size_t total = 0;
  for (size_t i = 0; i < n_clouds; i++) {
    if (!clouds[i] || clouds[i]->owner != h) {
      h->err = "hgs_detect_floor_batch: cloud " + std::to_string(i) + " is NULL or not a cloud of this engine";
      return HGS_ERR_INVALID_ARGUMENT;
    }
    total += clouds[i]->n_input;
  }
  if (total > (size_t)1 << 30) {
    h->err = "hgs_detect_floor_batch: more than 2^30 points in one call";
    return HGS_ERR_INVALID_ARGUMENT;
  }
  HGS_TRY(set_device(h));
  h->fb_clouds = (int)n_clouds;
  std::memset(out, 0, n_clouds * sizeof(*out));
  std::vector<hgs_cloud*> clipped;  // the clipped clouds with their indices (normal filter only)
  int rc;
  try {
    rc = detect_floor_batch_impl(h, clouds, n_clouds, p, out, filtered_out, inliers_out, clipped);
  } catch (...) {  // (a failed host allocation: the clouds made so far are freed below like after a HIP error)
    rc = status_of_current_exception(h);
  }
  for (hgs_cloud* c : clipped) cloud_free(c);
  if (rc != HGS_OK) {
    if (filtered_out) free_clouds(filtered_out, n_clouds);
    if (inliers_out) free_clouds(inliers_out, n_clouds);
  }
  return rc;
} catch (...) {
  return status_of_current_exception(h);
}

extern "C" int hgs_debug_floor_batch_stats(hgs_handle* h, int32_t* clouds, int32_t* ransac_clouds, int32_t* ransac_rounds, int32_t* readbacks) try {
  ApiLock lock(h);
  if (!h) return HGS_ERR_INVALID_ARGUMENT;
  if (clouds) *clouds = h->fb_clouds;
  if (ransac_clouds) *ransac_clouds = h->fb_ransac_clouds;
  if (ransac_rounds) *ransac_rounds = h->fb_rounds;
  if (readbacks) *readbacks = h->fb_readbacks;
  return HGS_OK;
} catch (...) {
  return status_of_current_exception(h);
}

extern "C" int hgs_debug_floor_filter(hgs_handle* h, hgs_cloud* cloud, const hgs_floor_params* p, uint8_t* keep_clip, uint8_t* keep_normal, double* normals3) try {
  ApiLock lock(h);
  if (!h || !cloud || !p || cloud->owner != h || !floor_params_valid(p)) return HGS_ERR_INVALID_ARGUMENT;
  HGS_TRY(set_device(h));
  FloorWork w;
  const int rc = floor_filter(h, cloud, p, floor_consts(p), &w, keep_clip, keep_normal, normals3);
  cloud_free(w.clipped);
  return rc;
} catch (...) {
  return status_of_current_exception(h);
}

extern "C" int hgs_debug_floor_ransac_counts(hgs_handle* h, hgs_cloud* cloud, const hgs_floor_params* p, uint32_t i0, uint32_t n, int32_t* counts, double* coeffs4) try {
  ApiLock lock(h);
  if (!h || !cloud || !p || cloud->owner != h || !floor_params_valid(p) || (n > 0 && !counts) || (uint64_t)i0 + n > 0x7fffffffull) return HGS_ERR_INVALID_ARGUMENT;
  HGS_TRY(set_device(h));
  const int chunk = std::max(1, std::min(kFloorMaxChunk, h->floor_chunk));
  FloorRansacBufs b;
  HGS_TRY(floor_ransac_bufs(h, chunk, &b));
  const FloorConsts c = floor_consts(p);
  const int np = (int)cloud->n_input;
  for (uint32_t done = 0; done < n; done += (uint32_t)chunk) {
    const int nh = (int)std::min<uint32_t>((uint32_t)chunk, n - done);
    launch_floor_ransac_planes(h->stream, cloud->desc.raw, np, c.seed, (int)(i0 + done), nh, nullptr, b.planes, b.counts);
    launch_floor_ransac_count(h->stream, cloud->desc.raw, np, c.dist_thresh, b.planes, nh, nullptr, b.counts);
    HGS_HIP(h, hipGetLastError());
    HGS_HIP(h, hipMemcpyAsync(counts + done, b.counts, (size_t)nh * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (coeffs4) HGS_HIP(h, hipMemcpyAsync(coeffs4 + 4 * (size_t)done, b.planes, (size_t)nh * 4 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HGS_HIP(h, hipStreamSynchronize(h->stream));
  }
  return HGS_OK;
} catch (...) {
  return status_of_current_exception(h);
}

int hgs_profile_enable(hgs_handle* h, int enabled) try {
  ApiLock lock(h);
  if (!h) return HGS_ERR_INVALID_ARGUMENT;
  h->profiling = enabled != 0;
  return HGS_OK;
} catch (...) {
  return status_of_current_exception(h);
}

int hgs_profile_read(hgs_handle* h, double* ms, uint64_t* launches, int reset) try {
  ApiLock lock(h);
  if (!h) return HGS_ERR_INVALID_ARGUMENT;
  HGS_TRY(set_device(h));
  HGS_HIP(h, hipStreamSynchronize(h->stream));
  for (auto& ev : h->prof_events) {
    float t = 0.f;
    if (hipEventElapsedTime(&t, ev.a, ev.b) == hipSuccess) {
      h->prof_ms[ev.stage] += (double)t;
      h->prof_launches[ev.stage]++;
    }
    h->prof_free.push_back(ev);
  }
  h->prof_events.clear();
  for (int i = 0; i < HGS_STAGE_COUNT; i++) {
    if (ms) ms[i] = h->prof_ms[i];
    if (launches) launches[i] = h->prof_launches[i];
    if (reset) h->prof_ms[i] = 0, h->prof_launches[i] = 0;
  }
  return HGS_OK;
} catch (...) {
  return status_of_current_exception(h);
}

int hgs_synchronize(hgs_handle* h) try {
  ApiLock lock(h);
  if (!h) return HGS_ERR_INVALID_ARGUMENT;
  HGS_TRY(set_device(h));
  HGS_HIP(h, hipStreamSynchronize(h->stream));
  return HGS_OK;
} catch (...) {
  return status_of_current_exception(h);
}

// ---- stage-level hooks for the parity tests ---------------------------------------------------------------
int hgs_debug_target_covariances(hgs_handle* h, float* out6) try {
  ApiLock lock(h);
  if (!h || !out6) return HGS_ERR_INVALID_ARGUMENT;
  if (!h->target) return HGS_ERR_NO_TARGET;
  HGS_TRY(set_device(h));
  hgs_cloud* t = h->target;
  std::vector<hgs_cloud*> all{t};
  HGS_TRY(ensure_cov(h, all, h->prm.correspondence_randomness));
  const size_t slots = (size_t)t->P * kLeaf;
  std::vector<float4> pts(slots), cov(2 * slots);
  int nvalid = 0;
  HGS_HIP(h, hipMemcpyAsync(pts.data(), t->desc.pts, slots * sizeof(float4), hipMemcpyDeviceToHost, h->stream));
  HGS_HIP(h, hipMemcpyAsync(cov.data(), t->desc.cov, 2 * slots * sizeof(float4), hipMemcpyDeviceToHost, h->stream));
  HGS_HIP(h, hipMemcpyAsync(&nvalid, &t->desc.meta->nvalid, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HGS_HIP(h, hipStreamSynchronize(h->stream));
  std::memset(out6, 0, t->n_input * 6 * sizeof(float));
  for (int i = 0; i < nvalid; i++) {
    int o;
    std::memcpy(&o, &pts[i].w, 4);
    if (o < 0 || (size_t)o >= t->n_input) continue;
    float* p = out6 + (size_t)o * 6;
    p[0] = cov[2 * i].x, p[1] = cov[2 * i].y, p[2] = cov[2 * i].z, p[3] = cov[2 * i].w, p[4] = cov[2 * i + 1].x, p[5] = cov[2 * i + 1].y;
  }
  return HGS_OK;
} catch (...) {
  return status_of_current_exception(h);
}

int hgs_debug_gicp_linearize(hgs_handle* h, const double T12[12], double* H36, double* b6, double* err, int32_t* corr) try {
  ApiLock lock(h);
  if (!h || !T12 || !H36 || !b6 || !err) return HGS_ERR_INVALID_ARGUMENT;
  if (h->prm.method != HGS_FAST_GICP && h->prm.method != HGS_FAST_VGICP) return HGS_ERR_UNSUPPORTED;
  if (!h->target) return HGS_ERR_NO_TARGET;
  if (!h->source) return HGS_ERR_NO_SOURCE;
  HGS_TRY(set_device(h));
  hgs_cloud *s = h->source, *t = h->target;
  const bool voxel = h->prm.method == HGS_FAST_VGICP;
  std::vector<hgs_cloud*> all{s, t};
  HGS_TRY(ensure_cov(h, all, h->prm.correspondence_randomness));
  if (voxel) HGS_TRY(ensure_vgicp_target(h, t));
  const int max_blocks = std::max(1, ((int)s->n_input + kBlock - 1) / kBlock);
  std::vector<hgs_cloud*> src{s};
  const CloudDesc* d_descs = nullptr;
  HGS_TRY(upload_descs(h, src, false, &d_descs, nullptr));
  HGS_HIP(h, h->states.reserve(sizeof(GicpState)));
  HGS_HIP(h, h->partials.reserve((size_t)max_blocks * kAcc * sizeof(double)));
  HGS_HIP(h, h->misc.reserve(64 * sizeof(double)));
  HGS_HIP(h, hipMemsetAsync(h->partials.p, 0, (size_t)max_blocks * kAcc * sizeof(double), h->stream));
  HGS_HIP(h, hipMemcpyAsync(h->misc.p, T12, 12 * sizeof(double), hipMemcpyHostToDevice, h->stream));
  launch_gicp_debug_state(h->stream, h->states.as<GicpState>(), h->misc.as<double>());
  if (voxel) launch_vgicp_linearize(h->stream, d_descs, vgicp_target_view(t), h->states.as<GicpState>(), vgicp_consts(h->prm), h->partials.as<double>(), max_blocks, 1);
  else launch_gicp_linearize(h->stream, d_descs, target_view(t), h->states.as<GicpState>(), gicp_consts(h->prm), h->partials.as<double>(), max_blocks, 1, 64);
  double* d_out = h->misc.as<double>() + 16;
  launch_reduce_partials(h->stream, h->partials.as<double>(), max_blocks, kAcc, d_out);
  double acc[kAcc];
  HGS_HIP(h, hipMemcpyAsync(acc, d_out, sizeof(acc), hipMemcpyDeviceToHost, h->stream));
  const size_t s_slots = (size_t)s->P * kLeaf, t_slots = (size_t)t->P * kLeaf;
  std::vector<float4> spts, tpts;
  std::vector<int> dcorr;
  int s_nvalid = 0;
  if (corr) {
    spts.resize(s_slots), tpts.resize(t_slots), dcorr.resize(s_slots);
    HGS_HIP(h, hipMemcpyAsync(spts.data(), s->desc.pts, s_slots * sizeof(float4), hipMemcpyDeviceToHost, h->stream));
    HGS_HIP(h, hipMemcpyAsync(tpts.data(), t->desc.pts, t_slots * sizeof(float4), hipMemcpyDeviceToHost, h->stream));
    HGS_HIP(h, hipMemcpyAsync(dcorr.data(), s->desc.corr, s_slots * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HGS_HIP(h, hipMemcpyAsync(&s_nvalid, &s->desc.meta->nvalid, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  }
  HGS_HIP(h, hipStreamSynchronize(h->stream));
  int k = 0;
  for (int r = 0; r < 6; r++)
    for (int c = r; c < 6; c++) H36[r * 6 + c] = H36[c * 6 + r] = acc[k++];
  for (int i = 0; i < 6; i++) b6[i] = acc[21 + i];
  *err = acc[27];
  if (corr) {
    for (size_t i = 0; i < s->n_input; i++) corr[i] = voxel ? 0 : -1;
    for (int i = 0; i < s_nvalid; i++) {
      int so, to = -1;
      std::memcpy(&so, &spts[i].w, 4);
      const int j = dcorr[i];
      if (voxel) to = j;  // VGICP: number of voxel correspondences of that source point
      else if (j >= 0 && (size_t)j < t_slots) std::memcpy(&to, &tpts[j].w, 4);
      if (so >= 0 && (size_t)so < s->n_input) corr[so] = to;
    }
  }
  return HGS_OK;
} catch (...) {
  return status_of_current_exception(h);
}

int hgs_debug_icp_correspond(hgs_handle* h, const double T12[12], double* sums17, int32_t* corr) try {
  ApiLock lock(h);
  if (!h || !T12 || !sums17) return HGS_ERR_INVALID_ARGUMENT;
  if (h->prm.method != HGS_ICP) return HGS_ERR_UNSUPPORTED;
  if (!h->target) return HGS_ERR_NO_TARGET;
  if (!h->source) return HGS_ERR_NO_SOURCE;
  HGS_TRY(set_device(h));
  hgs_cloud *s = h->source, *t = h->target;
  std::vector<hgs_cloud*> all{s, t};
  HGS_TRY(ensure_index(h, all));
  const int max_blocks = std::max(1, ((int)s->n_input + kTileNN - 1) / kTileNN);
  std::vector<hgs_cloud*> src{s};
  const CloudDesc* d_descs = nullptr;
  HGS_TRY(upload_descs(h, src, false, &d_descs, nullptr));
  IcpState st;
  for (int i = 0; i < 12; i++) st.x.m[i] = T12[i];
  st.mse = st.mse_prev = DBL_MAX, st.phase = ICP_RUN, st.iterations = st.passes = st.converged = 0;
  HGS_HIP(h, h->states.reserve(sizeof(IcpState)));
  HGS_HIP(h, h->partials.reserve((size_t)max_blocks * kAccIcp * sizeof(double)));
  HGS_HIP(h, hipMemcpyAsync(h->states.p, &st, sizeof(st), hipMemcpyHostToDevice, h->stream));
  launch_icp_correspond(h->stream, d_descs, target_view(t), h->states.as<IcpState>(), icp_consts(h->prm), h->partials.as<double>(), max_blocks, 1);
  HGS_HIP(h, hipGetLastError());
  std::vector<double> part((size_t)max_blocks * kAccIcp);
  int s_nvalid = 0;
  HGS_HIP(h, hipMemcpyAsync(&s_nvalid, &s->desc.meta->nvalid, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HGS_HIP(h, hipMemcpyAsync(part.data(), h->partials.p, part.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  const size_t s_slots = (size_t)s->P * kLeaf, t_slots = (size_t)t->P * kLeaf;
  std::vector<float4> spts, tpts;
  std::vector<int> dcorr;
  if (corr) {
    spts.resize(s_slots), tpts.resize(t_slots), dcorr.resize(s_slots);
    HGS_HIP(h, hipMemcpyAsync(spts.data(), s->desc.pts, s_slots * sizeof(float4), hipMemcpyDeviceToHost, h->stream));
    HGS_HIP(h, hipMemcpyAsync(tpts.data(), t->desc.pts, t_slots * sizeof(float4), hipMemcpyDeviceToHost, h->stream));
    HGS_HIP(h, hipMemcpyAsync(dcorr.data(), s->desc.corr, s_slots * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  }
  HGS_HIP(h, hipStreamSynchronize(h->stream));
  const int ntiles = (s_nvalid + kTileNN - 1) / kTileNN;  // (the rows the pass wrote; the sums in tile order)
  for (int k = 0; k < kAccIcp; k++) sums17[k] = 0.0;
  for (int tile = 0; tile < ntiles && tile < max_blocks; tile++)
    for (int k = 0; k < kAccIcp; k++) sums17[k] += part[(size_t)tile * kAccIcp + k];
  if (corr) {
    for (size_t i = 0; i < s->n_input; i++) corr[i] = -1;
    for (int i = 0; i < s_nvalid && (size_t)i < s_slots; i++) {
      int so, to = -1;
      std::memcpy(&so, &spts[i].w, 4);
      const int j = dcorr[i];
      if (j >= 0 && (size_t)j < t_slots) std::memcpy(&to, &tpts[j].w, 4);
      if (so >= 0 && (size_t)so < s->n_input) corr[so] = to;
    }
  }
  return HGS_OK;
} catch (...) {
  return status_of_current_exception(h);
}

int hgs_debug_icp_step(hgs_handle* h, const double sums17[17], const double T12_in[12], double mse_prev, int32_t iterations_in, double T12_out[12],
                       int32_t flags3[3], double* mse) try {
  ApiLock lock(h);
  if (!h || !sums17 || !T12_in || !T12_out || !flags3 || !mse) return HGS_ERR_INVALID_ARGUMENT;
  if (h->prm.method != HGS_ICP) return HGS_ERR_UNSUPPORTED;
  if (!h->source) return HGS_ERR_NO_SOURCE;  // (k_icp_solve takes its tile count from the source's nvalid)
  HGS_TRY(set_device(h));
  hgs_cloud* s = h->source;
  std::vector<hgs_cloud*> src{s};
  HGS_TRY(ensure_index(h, src));
  const int max_blocks = std::max(1, ((int)s->n_input + kTileNN - 1) / kTileNN);
  const CloudDesc* d_descs = nullptr;
  HGS_TRY(upload_descs(h, src, false, &d_descs, nullptr));
  IcpState st;
  for (int i = 0; i < 12; i++) st.x.m[i] = T12_in[i];
  st.mse = DBL_MAX, st.mse_prev = mse_prev, st.phase = ICP_RUN, st.iterations = iterations_in, st.passes = 0, st.converged = 0;
  Progress prog;
  HGS_TRY(make_progress(h, 0, 1, &prog));
  HGS_HIP(h, h->states.reserve(sizeof(IcpState)));
  HGS_HIP(h, h->partials.reserve((size_t)max_blocks * kAccIcp * sizeof(double)));
  HGS_HIP(h, hipMemsetAsync(prog.dev, 0, 2 * sizeof(int), h->stream));
  HGS_HIP(h, hipMemcpyAsync(h->states.p, &st, sizeof(st), hipMemcpyHostToDevice, h->stream));
  HGS_HIP(h, hipMemsetAsync(h->partials.p, 0, (size_t)max_blocks * kAccIcp * sizeof(double), h->stream));  // every tile row but row 0
  HGS_HIP(h, hipMemcpyAsync(h->partials.p, sums17, kAccIcp * sizeof(double), hipMemcpyHostToDevice, h->stream));
  launch_icp_solve(h->stream, d_descs, h->states.as<IcpState>(), icp_consts(h->prm), h->partials.as<double>(), max_blocks, 1, prog);
  HGS_HIP(h, hipGetLastError());
  HGS_HIP(h, hipMemcpyAsync(&st, h->states.p, sizeof(st), hipMemcpyDeviceToHost, h->stream));
  HGS_HIP(h, hipStreamSynchronize(h->stream));
  for (int i = 0; i < 12; i++) T12_out[i] = st.x.m[i];
  flags3[0] = st.converged, flags3[1] = st.phase == ICP_DONE ? 1 : 0, flags3[2] = st.iterations;
  *mse = st.mse;
  return HGS_OK;
} catch (...) {
  return status_of_current_exception(h);
}

int hgs_debug_cloud_seed_grid(hgs_handle* h, hgs_cloud* cloud, uint32_t* tab, size_t cap, int32_t* bits, size_t* entries) try {
  ApiLock lock(h);
  if (!h || !cloud || cloud->owner != h || !entries || (cap > 0 && !tab)) return HGS_ERR_INVALID_ARGUMENT;
  *entries = 0;
  if (bits) *bits = 0;
  if (!cloud->has_seed) return HGS_OK;
  HGS_TRY(set_device(h));
  const size_t n = seed_grid_entries(cloud->seed_bits), m = std::min(cap, n);
  if (m > 0) {
    HGS_HIP(h, h->h_xform.reserve(m * sizeof(uint32_t)));
    HGS_HIP(h, hipMemcpyAsync(h->h_xform.p, cloud->seed_block.p, m * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HGS_HIP(h, hipStreamSynchronize(h->stream));
    std::memcpy(tab, h->h_xform.p, m * sizeof(uint32_t));
  }
  *entries = n;
  if (bits) *bits = cloud->seed_bits;
  return HGS_OK;
} catch (...) {
  return status_of_current_exception(h);
}

int hgs_debug_ndt_cells(hgs_handle* h, int32_t cap, int32_t* ijk3, double* mean3, float* icov6, int32_t* npts, int32_t* n_cells) try {
  ApiLock lock(h);
  if (!h || !n_cells) return HGS_ERR_INVALID_ARGUMENT;
  if (h->prm.method != HGS_NDT_OMP) return HGS_ERR_UNSUPPORTED;
  if (!h->target) return HGS_ERR_NO_TARGET;
  HGS_TRY(set_device(h));
  hgs_cloud* t = h->target;
  HGS_TRY(ensure_ndt_target(h, t));
  CloudMeta meta;
  HGS_HIP(h, hipMemcpyAsync(&meta, t->desc.meta, sizeof(CloudMeta), hipMemcpyDeviceToHost, h->stream));
  HGS_HIP(h, hipStreamSynchronize(h->stream));
  *n_cells = meta.ndt_ncells;
  const int n = std::min<int>(meta.ndt_ncells, cap);
  if (n <= 0) return HGS_OK;
  std::vector<NdtCellRec> cells(n);
  HGS_HIP(h, hipMemcpyAsync(cells.data(), t->ndt.cells, (size_t)n * sizeof(NdtCellRec), hipMemcpyDeviceToHost, h->stream));
  HGS_HIP(h, hipStreamSynchronize(h->stream));
  for (int i = 0; i < n; i++) {
    int key;
    std::memcpy(&key, &cells[i].v1.w, 4);
    if (ijk3) {
      const int m1 = meta.ndt_div_mul[1], m2 = meta.ndt_div_mul[2];
      ijk3[3 * i] = key % m1 + meta.ndt_min_b[0];
      ijk3[3 * i + 1] = (key % m2) / m1 + meta.ndt_min_b[1];
      ijk3[3 * i + 2] = key / m2 + meta.ndt_min_b[2];
    }
    if (mean3) mean3[3 * i] = cells[i].mean[0], mean3[3 * i + 1] = cells[i].mean[1], mean3[3 * i + 2] = cells[i].mean[2];
    if (icov6) {
      float* o = icov6 + 6 * i;
      o[0] = cells[i].v0.x, o[1] = cells[i].v0.y, o[2] = cells[i].v0.z, o[3] = cells[i].v0.w, o[4] = cells[i].v1.x, o[5] = cells[i].v1.y;
    }
    if (npts) npts[i] = (int)cells[i].v1.z;
  }
  return HGS_OK;
} catch (...) {
  return status_of_current_exception(h);
}

int hgs_debug_vgicp_voxels(hgs_handle* h, int32_t cap, int32_t* ijk3, double* mean3, float* cov6, int32_t* npts, int32_t* n_cells) try {
  ApiLock lock(h);
  if (!h || !n_cells) return HGS_ERR_INVALID_ARGUMENT;
  if (h->prm.method != HGS_FAST_VGICP) return HGS_ERR_UNSUPPORTED;
  if (!h->target) return HGS_ERR_NO_TARGET;
  HGS_TRY(set_device(h));
  hgs_cloud* t = h->target;
  std::vector<hgs_cloud*> all{t};
  HGS_TRY(ensure_cov(h, all, h->prm.correspondence_randomness));
  HGS_TRY(ensure_vgicp_target(h, t));
  CloudMeta meta;
  HGS_HIP(h, hipMemcpyAsync(&meta, t->desc.meta, sizeof(CloudMeta), hipMemcpyDeviceToHost, h->stream));
  HGS_HIP(h, hipStreamSynchronize(h->stream));
  *n_cells = meta.vg_ncells;
  const int n = std::min<int>(meta.vg_ncells, cap);
  if (n <= 0) return HGS_OK;
  std::vector<NdtCellRec> cells(n);
  HGS_HIP(h, hipMemcpyAsync(cells.data(), t->vg.cells, (size_t)n * sizeof(NdtCellRec), hipMemcpyDeviceToHost, h->stream));
  HGS_HIP(h, hipStreamSynchronize(h->stream));
  for (int i = 0; i < n; i++) {
    int key;
    std::memcpy(&key, &cells[i].v1.w, 4);
    if (ijk3) {
      const int m1 = meta.vg_div_mul[1], m2 = meta.vg_div_mul[2];
      ijk3[3 * i] = key % m1 + meta.vg_min_b[0];
      ijk3[3 * i + 1] = (key % m2) / m1 + meta.vg_min_b[1];
      ijk3[3 * i + 2] = key / m2 + meta.vg_min_b[2];
    }
    if (mean3) mean3[3 * i] = cells[i].mean[0], mean3[3 * i + 1] = cells[i].mean[1], mean3[3 * i + 2] = cells[i].mean[2];
    if (cov6) {
      float* o = cov6 + 6 * i;
      o[0] = cells[i].v0.x, o[1] = cells[i].v0.y, o[2] = cells[i].v0.z, o[3] = cells[i].v0.w, o[4] = cells[i].v1.x, o[5] = cells[i].v1.y;
    }
    if (npts) npts[i] = (int)cells[i].v1.z;
  }
  return HGS_OK;
} catch (...) {
  return status_of_current_exception(h);
}

int hgs_debug_ndt_derivatives(hgs_handle* h, const double p6[6], double* score, double* g6, double* H36) try {
  ApiLock lock(h);
  if (!h || !p6 || !score || !g6 || !H36) return HGS_ERR_INVALID_ARGUMENT;
  if (h->prm.method != HGS_NDT_OMP) return HGS_ERR_UNSUPPORTED;
  if (!h->target) return HGS_ERR_NO_TARGET;
  if (!h->source) return HGS_ERR_NO_SOURCE;
  HGS_TRY(set_device(h));
  hgs_cloud *s = h->source, *t = h->target;
  HGS_TRY(ensure_ndt_target(h, t));
  const int max_blocks = std::max(1, ((int)s->n_input + kBlock - 1) / kBlock);
  std::vector<hgs_cloud*> src{s};
  const CloudDesc* d_descs = nullptr;
  HGS_TRY(upload_descs(h, src, false, &d_descs, nullptr));
  const NdtConsts c = engine_ndt_consts(h->prm);
  HGS_HIP(h, h->states.reserve(sizeof(NdtState)));
  HGS_HIP(h, h->angles.reserve(sizeof(NdtAngles)));
  HGS_HIP(h, h->ndt_accum.reserve(sizeof(NdtAccum)));
  HGS_HIP(h, h->misc.reserve(128 * sizeof(double)));
  HGS_HIP(h, hipMemsetAsync(h->ndt_accum.p, 0, sizeof(NdtAccum), h->stream));
  HGS_HIP(h, hipMemcpyAsync(h->misc.p, p6, 6 * sizeof(double), hipMemcpyHostToDevice, h->stream));
  launch_ndt_debug_state(h->stream, h->states.as<NdtState>(), h->angles.as<NdtAngles>(), h->misc.as<double>(), c);
  Progress none{};
  HGS_HIP(h, h->ndt_plan.reserve(256));
  struct {
    unsigned long long queue, pad;
    int tile_base[2];
  } plan{0, 0, {0, max_blocks}};
  HGS_HIP(h, hipMemcpy(h->ndt_plan.p, &plan, sizeof(plan), hipMemcpyHostToDevice));
  launch_ndt_pass(h->stream, d_descs, ndt_target_view(h, t), h->states.as<NdtState>(), h->angles.as<NdtAngles>(), c, h->ndt_accum.as<NdtAccum>(),
                  reinterpret_cast<const int*>((char*)h->ndt_plan.p + 16), reinterpret_cast<unsigned long long*>(h->ndt_plan.p), 1, 0, std::min(max_blocks, 96),
                  2 /* several tiles per block, several grabs per block */, (h->ndt_sort != 0 && s->has_index) ? 1 : 0, 1, none);
  double acc[kAccNdt];
  HGS_HIP(h, hipMemcpyAsync(acc, h->ndt_accum.as<NdtAccum>()->out, sizeof(acc), hipMemcpyDeviceToHost, h->stream));
  HGS_HIP(h, hipStreamSynchronize(h->stream));
  for (int i = 0; i < 36; i++) H36[i] = acc[i];
  for (int i = 0; i < 6; i++) g6[i] = acc[36 + i];
  *score = acc[42];
  return HGS_OK;
} catch (...) {
  return status_of_current_exception(h);
}

}  // extern "C"
