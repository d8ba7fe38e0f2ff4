// resident_clouds_hip.hpp — header-only bindings of the three "next" rows of SURVEY §8(f) that sit beside the registration path:
//
//   f1  InformationMatrixCalculator::calc_fitness_score   src/hdl_graph_slam/information_matrix_calculator.cpp:49-80   -> hgs_calc_fitness_score
//   f2  PrefilteringNodelet::cloud_callback :131-133      apps/prefiltering_nodelet.cpp (distance filter, downsample, outlier removal) -> hgs_prefilter
//   f3  MapCloudGenerator::generate                       src/hdl_graph_slam/map_cloud_generator.cpp:13-51              -> hgs_map_cloud_generate
//   12  FloorDetectionNodelet::detect                     apps/floor_detection_nodelet.cpp:110-180 (through adapters/floor_detection_hip.hpp) -> hgs_detect_floor
//
// integration/hdl_graph_slam_hip.patch calls them from the reference's own functions behind #ifdef USE_HGS_HIP; every call returns false when the
// device path could not run (no engine, out of memory, an argument the device refuses) and the reference's CPU code below the hunk runs instead —
// the same "fall through to what was there" rule as LoopDetector::matching's batch hunk.
//
// f1 and f3 work on KEYFRAME clouds: `pcl::PointCloud::ConstPtr`s the pose graph keeps for its whole life (include/hdl_graph_slam/keyframe.hpp:44).
// calc_fitness_score is a static function that sees two cloud pointers and nothing else, so the device copies live in a process-wide cache keyed by
// the cloud OBJECT: the cache holds the shared_ptr (the address cannot be reused for another cloud while its device copy exists), uploads a cloud the
// first time it is seen and releases the least recently used ones beyond a byte budget (setCapacity; default 8 GiB of the 288 GB).  The search index a
// cloud gets as `cloud1` of one edge is reused by every later edge and map update that names it.
//
// Thread safety: one mutex around the engine (hdl_graph_slam_nodelet calls these from its optimisation timer, its map timer and its services).
// Like registration_hip.hpp this header cannot be compiled against the real PCL in this repository's image; tests/cpp/integration_main.cpp compiles
// it against tests/mock_pcl and runs it inside the patched reference functions (host emulation of the kernels on the CPU, libhgs_hip.so with -m gpu).
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include <pcl/point_cloud.h>
#include <pcl/point_types.h>

#include "hgs_registration.h"

namespace hgs_hip {

template <typename PointT>
class ResidentCloudsHIP {
public:
  using Cloud = pcl::PointCloud<PointT>;
  using CloudConstPtr = typename Cloud::ConstPtr;

  // the process-wide instance the static calc_fitness_score reaches
  static ResidentCloudsHIP& instance() {
    static ResidentCloudsHIP* self = new ResidentCloudsHIP();  // never destroyed: at static-destruction time the HIP runtime may be gone already
    return *self;
  }
  ResidentCloudsHIP() = default;
  ~ResidentCloudsHIP() { release(); }
  ResidentCloudsHIP(const ResidentCloudsHIP&) = delete;
  ResidentCloudsHIP& operator=(const ResidentCloudsHIP&) = delete;

  // rosparams `reg_hip_device` (0) and `reg_hip_next_rows` (true) of the nodelet that constructs InformationMatrixCalculator / MapCloudGenerator
  void configure(int device_id, bool enabled) {
    std::lock_guard<std::mutex> lock(mutex_);
    if (device_id != device_id_ && handle_) release_locked();
    device_id_ = device_id, enabled_ = enabled;
  }
  void setCapacity(size_t max_bytes) {
    std::lock_guard<std::mutex> lock(mutex_);
    max_bytes_ = max_bytes;
  }
  bool enabled() const { return enabled_; }
  size_t resident() const { return clouds_.size(); }
  size_t resident_bytes() const { return bytes_; }
  size_t device_calls() const { return device_calls_; }  // successful device-side calls (tests: "the hunk really took the device path")
  const std::string& last_error() const { return last_error_; }

  // f1 — information_matrix_calculator.cpp:49-80.  `relpose_colmajor`: relpose.cast<float>().matrix().data()
  bool fitness_score(const CloudConstPtr& cloud1, const CloudConstPtr& cloud2, const float relpose_colmajor[16], double max_range, double* score) {
    std::lock_guard<std::mutex> lock(mutex_);
    if (!enabled_ || !cloud1 || !cloud2 || cloud1->points.empty()) return false;  // (an empty target: PCL's kd-tree path decides what that means)
    if (cloud2->points.empty()) {  // nr == 0 -> std::numeric_limits<double>::max() (:76-79); nothing to launch
      *score = 1.7976931348623157e308;
      return true;
    }
    if (!engine()) return false;
    const uint64_t tick = ++tick_;
    hgs_cloud* c1 = resident_cloud(cloud1, tick);
    hgs_cloud* c2 = c1 ? resident_cloud(cloud2, tick) : nullptr;
    if (!c1 || !c2) return false;
    const bool ok = check(hgs_calc_fitness_score(handle_, c1, c2, relpose_colmajor, max_range, score), "hgs_calc_fitness_score");
    enforce_capacity(tick);
    device_calls_ += ok ? 1 : 0;
    return ok;
  }

  // f1 for every edge of one graph update — the odometry edges of flush_keyframe_queue (apps/hdl_graph_slam_nodelet.cpp:235) and the loop edges behind them
  // (apps/hdl_graph_slam_nodelet.cpp:569) — in ONE hgs_calc_fitness_score_batch: every cloud of the call is resolved (uploaded when new) first, then one
  // device call.  (*scores)[i] is what fitness_score returns for pairs[i], bit for bit.  false on any failure — and for a pair fitness_score itself would hand
  // back to the CPU (a null cloud, an empty cloud1): the caller then runs its per-edge path.
  struct EdgePair {
    CloudConstPtr cloud1, cloud2;
    float relpose[16];  // relpose.cast<float>().matrix().data()
  };
  bool fitness_scores(const std::vector<EdgePair>& pairs, double max_range, std::vector<double>* scores) {
    std::lock_guard<std::mutex> lock(mutex_);
    if (!enabled_ || !scores) return false;
    for (const EdgePair& p : pairs)
      if (!p.cloud1 || !p.cloud2 || p.cloud1->points.empty()) return false;
    scores->assign(pairs.size(), 1.7976931348623157e308);  // (an empty cloud2: nr == 0 -> DBL_MAX, :76-79; nothing to launch for it)
    std::vector<size_t> which;
    for (size_t i = 0; i < pairs.size(); i++)
      if (!pairs[i].cloud2->points.empty()) which.push_back(i);
    if (which.empty()) return true;
    if (!engine()) return false;
    const uint64_t tick = ++tick_;
    std::vector<hgs_cloud*> c1, c2;
    std::vector<float> poses;
    bool ok = true;
    for (size_t i : which) {
      hgs_cloud* a = resident_cloud(pairs[i].cloud1, tick);
      hgs_cloud* b = a ? resident_cloud(pairs[i].cloud2, tick) : nullptr;
      if (!a || !b) {
        ok = false;
        break;
      }
      c1.push_back(a), c2.push_back(b);
      poses.insert(poses.end(), pairs[i].relpose, pairs[i].relpose + 16);
    }
    std::vector<double> dev(which.size());
    ok = ok && check(hgs_calc_fitness_score_batch(handle_, c1.data(), c2.data(), poses.data(), which.size(), max_range, dev.data(), nullptr), "hgs_calc_fitness_score_batch");
    enforce_capacity(tick);  // (on every exit path behind the first upload)
    if (!ok) return false;
    for (size_t k = 0; k < which.size(); k++) (*scores)[which[k]] = dev[k];
    device_calls_++;
    return true;
  }

  // f3 — map_cloud_generator.cpp:13-51 for resolution > 0: the voxel centres of pcl::octree in the octree's own order, intensity 0.
  // `poses_colmajor`: keyframe->pose.matrix().cast<float>() of every snapshot, 16 floats each.
  bool map_cloud(const std::vector<CloudConstPtr>& keyframe_clouds, const std::vector<float>& poses_colmajor, double resolution, Cloud& out) {
    std::lock_guard<std::mutex> lock(mutex_);
    if (!enabled_ || keyframe_clouds.empty() || poses_colmajor.size() != keyframe_clouds.size() * 16 || !(resolution > 0.0)) return false;
    if (!engine()) return false;
    const uint64_t tick = ++tick_;
    std::vector<hgs_cloud*> dev;
    for (const CloudConstPtr& c : keyframe_clouds) {
      hgs_cloud* d = c ? resident_cloud(c, tick) : nullptr;
      if (!d) return false;
      dev.push_back(d);
    }
    hgs_cloud* map = nullptr;
    bool ok = check(hgs_map_cloud_generate(handle_, dev.data(), poses_colmajor.data(), dev.size(), resolution, &map), "hgs_map_cloud_generate");
    if (ok) {
      out.points.resize(hgs_cloud_size(map));
      ok = out.points.empty() || check(hgs_cloud_download(map, out.points.data(), sizeof(PointT)), "hgs_cloud_download");
    }
    if (map) hgs_cloud_destroy(map);
    enforce_capacity(tick);
    device_calls_ += ok ? 1 : 0;
    return ok;
  }

  // f2 — apps/prefiltering_nodelet.cpp:131-133 (+ the deskewing step of :112,182-243 when `imu_angular_velocity` is given, + the transform into
  // base_link_frame of :114-129 when `sensor_to_base` is given: Eigen::Matrix4f::data() of the matrix pcl_ros::transformPointCloud would apply): the filtered
  // cloud comes back as PointXYZI records (x, y, z, 1, intensity).  The input is a sensor sweep, not a keyframe: it is not cached.
  bool prefilter(const Cloud& src, const hgs_prefilter_params& params, const double* imu_angular_velocity, double scan_period, Cloud& out) {
    return prefilter(src, params, imu_angular_velocity, scan_period, nullptr, out);
  }
  bool prefilter(const Cloud& src, const hgs_prefilter_params& params, const double* imu_angular_velocity, double scan_period, const float* sensor_to_base, Cloud& out) {
    std::lock_guard<std::mutex> lock(mutex_);
    if (!enabled_ || src.points.empty()) return false;
    if (!engine()) return false;
    hgs_cloud* filtered = nullptr;
    bool ok = check(sensor_to_base ? hgs_prefilter_framed(handle_, src.points.data(), src.points.size(), sizeof(PointT), &params, imu_angular_velocity, scan_period, sensor_to_base, &filtered)
                    : imu_angular_velocity ? hgs_prefilter_deskewed(handle_, src.points.data(), src.points.size(), sizeof(PointT), &params, imu_angular_velocity, scan_period, &filtered)
                                           : hgs_prefilter(handle_, src.points.data(), src.points.size(), sizeof(PointT), &params, &filtered),
                    "hgs_prefilter");
    if (ok) {
      out.points.resize(hgs_cloud_size(filtered));
      ok = out.points.empty() || check(hgs_cloud_download(filtered, out.points.data(), sizeof(PointT)), "hgs_cloud_download");
    }
    if (ok && keep_prefiltered_) {  // (floor detection, below: the same sweep comes back as /filtered_points)
      if (prefiltered_) hgs_cloud_destroy(prefiltered_);
      prefiltered_ = filtered, filtered = nullptr;
      if (!out.points.empty()) {
        const PointT &a = out.points.front(), &b = out.points.back();
        const float e[6] = {a.x, a.y, a.z, b.x, b.y, b.z};
        std::memcpy(prefiltered_ends_, e, sizeof(e));
      } else {
        hgs_cloud_destroy(prefiltered_), prefiltered_ = nullptr;
      }
    }
    if (filtered) hgs_cloud_destroy(filtered);
    device_calls_ += ok ? 1 : 0;
    return ok;
  }

  // row 12 — FloorDetectionNodelet::detect (apps/floor_detection_nodelet.cpp:110-180) on the device: adapters/floor_detection_hip.hpp calls this.  The
  // nodelet's input is the prefilter's output (:44): with keepPrefiltered(true) the last prefilter() result stays resident, and a cloud of the same size
  // whose first and last points carry the same bits is taken from the device instead of being uploaded again.  `filtered` / `inliers` (null ok): the clouds
  // of floor_filtered_pub / floor_points_pub (:127-130, :168-177).
  void keepPrefiltered(bool on) {
    std::lock_guard<std::mutex> lock(mutex_);
    keep_prefiltered_ = on;
    if (!on && prefiltered_) hgs_cloud_destroy(prefiltered_), prefiltered_ = nullptr;
  }
  size_t resident_hits() const { return resident_hits_; }  // floor detections that found their input resident
  bool detect_floor(const Cloud& cloud, const hgs_floor_params& params, hgs_floor_result* result, Cloud* filtered, Cloud* inliers) {
    std::lock_guard<std::mutex> lock(mutex_);
    if (!enabled_ || !result || cloud.points.empty()) return false;
    if (!engine()) return false;
    hgs_cloud* in = nullptr;
    bool uploaded = false;
    if (prefiltered_ && hgs_cloud_size(prefiltered_) == cloud.points.size() && same_ends(cloud)) {
      in = prefiltered_;
      resident_hits_++;
    } else {
      if (!check(hgs_cloud_create(handle_, cloud.points.data(), cloud.points.size(), sizeof(PointT), &in), "hgs_cloud_create")) return false;
      uploaded = true;
    }
    hgs_cloud *f = nullptr, *i = nullptr;
    bool ok = check(hgs_detect_floor(handle_, in, &params, result, filtered ? &f : nullptr, inliers ? &i : nullptr), "hgs_detect_floor");
    if (ok && filtered) ok = fetch(f, *filtered);
    if (ok && inliers) ok = fetch(i, *inliers);
    if (f) hgs_cloud_destroy(f);
    if (i) hgs_cloud_destroy(i);
    if (uploaded) hgs_cloud_destroy(in);
    device_calls_ += ok ? 1 : 0;
    return ok;
  }

  // the rosparams of PrefilteringNodelet::initialize_params (apps/prefiltering_nodelet.cpp:50-99) as an hgs_prefilter_params
  static hgs_prefilter_params prefilter_params(const std::string& downsample_method, double downsample_resolution, const std::string& outlier_removal_method, int statistical_mean_k,
                                               double statistical_stddev, double radius_radius, int radius_min_neighbors, bool use_distance_filter, double distance_near_thresh,
                                               double distance_far_thresh) {
    hgs_prefilter_params p;
    hgs_prefilter_params_default(&p);
    p.downsample_method = downsample_method == "VOXELGRID" ? HGS_DOWNSAMPLE_VOXELGRID : (downsample_method == "APPROX_VOXELGRID" ? HGS_DOWNSAMPLE_APPROX_VOXELGRID : HGS_DOWNSAMPLE_NONE);
    p.downsample_resolution = downsample_resolution;
    p.outlier_removal_method = outlier_removal_method == "STATISTICAL" ? HGS_OUTLIER_STATISTICAL : (outlier_removal_method == "RADIUS" ? HGS_OUTLIER_RADIUS : HGS_OUTLIER_NONE);
    p.statistical_mean_k = statistical_mean_k, p.statistical_stddev = statistical_stddev;
    p.radius_radius = radius_radius, p.radius_min_neighbors = radius_min_neighbors;
    p.use_distance_filter = use_distance_filter ? 1 : 0;
    p.distance_near_thresh = distance_near_thresh, p.distance_far_thresh = distance_far_thresh;
    return p;
  }

  void forget_all() {
    std::lock_guard<std::mutex> lock(mutex_);
    while (!clouds_.empty()) drop(clouds_.begin());
  }

private:
  struct Entry {
    CloudConstPtr keep;   // holds the host cloud: its address stays unique while the device copy exists
    hgs_cloud* dev;
    uint64_t last_used;
    size_t bytes;
  };
  std::mutex mutex_;
  hgs_handle* handle_ = nullptr;
  int device_id_ = 0;
  bool enabled_ = true;
  bool create_failed_ = false;
  std::unordered_map<const void*, Entry> clouds_;
  size_t bytes_ = 0, max_bytes_ = (size_t)8 << 30, device_calls_ = 0;
  uint64_t tick_ = 0;
  std::string last_error_;
  bool keep_prefiltered_ = false;
  hgs_cloud* prefiltered_ = nullptr;  // the last prefilter() output (keepPrefiltered)
  size_t resident_hits_ = 0;
  float prefiltered_ends_[6] = {0, 0, 0, 0, 0, 0};

  bool same_ends(const Cloud& c) const {
    const PointT &a = c.points.front(), &b = c.points.back();
    const float e[6] = {a.x, a.y, a.z, b.x, b.y, b.z};
    return std::memcmp(e, prefiltered_ends_, sizeof(e)) == 0;
  }
  bool fetch(hgs_cloud* dev, Cloud& out) {  // a resident cloud (null: none) as PointXYZI records
    out.points.resize(dev ? hgs_cloud_size(dev) : 0);
    out.width = (unsigned)out.points.size(), out.height = 1;
    return out.points.empty() || check(hgs_cloud_download(dev, out.points.data(), sizeof(PointT)), "hgs_cloud_download");
  }

  bool engine() {
    if (handle_) return true;
    if (create_failed_) return false;  // do not retry (and log) on every edge
    hgs_params p;
    hgs_params_default(HGS_FAST_GICP, &p);  // the engine only serves searches and the map cloud: no registration parameter matters
    p.device_id = device_id_;
    if (hgs_create(&p, &handle_) != HGS_OK) {
      last_error_ = std::string("hgs_create: ") + hgs_last_error(nullptr);
      handle_ = nullptr, create_failed_ = true;
      return false;
    }
    return true;
  }
  hgs_cloud* resident_cloud(const CloudConstPtr& c, uint64_t tick) {
    auto it = clouds_.find(c.get());
    if (it == clouds_.end()) {
      hgs_cloud* d = nullptr;
      if (!check(hgs_cloud_create(handle_, c->points.data(), c->points.size(), sizeof(PointT), &d), "hgs_cloud_create")) return nullptr;
      it = clouds_.emplace(c.get(), Entry{c, d, tick, 0}).first;
    }
    it->second.last_used = tick;
    return it->second.dev;
  }
  void drop(typename std::unordered_map<const void*, Entry>::iterator it) {
    bytes_ -= std::min(bytes_, it->second.bytes);
    hgs_cloud_destroy(it->second.dev);
    clouds_.erase(it);
  }
  void enforce_capacity(uint64_t tick) {
    for (auto& kv : clouds_) {
      if (kv.second.last_used != tick) continue;
      const size_t b = hgs_cloud_device_bytes(kv.second.dev);
      bytes_ = bytes_ - std::min(bytes_, kv.second.bytes) + b;
      kv.second.bytes = b;
    }
    if (!max_bytes_ || bytes_ <= max_bytes_) return;
    std::vector<std::pair<uint64_t, const void*>> order;
    for (const auto& kv : clouds_) order.emplace_back(kv.second.last_used, kv.first);
    std::sort(order.begin(), order.end());
    for (const auto& o : order) {
      if (bytes_ <= max_bytes_) break;
      drop(clouds_.find(o.second));
    }
  }
  bool check(int rc, const char* what) {
    if (rc != HGS_OK) last_error_ = std::string(what) + ": " + hgs_last_error(handle_);
    return rc == HGS_OK;
  }
  void release_locked() {
    if (prefiltered_) hgs_cloud_destroy(prefiltered_), prefiltered_ = nullptr;
    while (!clouds_.empty()) drop(clouds_.begin());
    if (handle_) hgs_destroy(handle_);
    handle_ = nullptr, create_failed_ = false;
  }
  void release() {
    std::lock_guard<std::mutex> lock(mutex_);
    release_locked();
  }
};

}  // namespace hgs_hip
