// hgs_resources.h — owners of what the engine allocates through the HIP runtime and of its helper threads (host only): every one of them gives
// back what it holds when it goes out of scope, so hgs_handle and hgs_cloud need no list of things to free (hgs_engine.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

namespace hgs {

struct DeviceAlloc {
  static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static void free(void* p) { (void)hipFree(p); }
};
struct PinnedAlloc {
  static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static void free(void* p) { (void)hipHostFree(p); }
};

// One allocation, owned.  reserve() grows it (contents are lost) with some slack for the next, slightly larger request; alloc() replaces it by exactly
// `bytes` (a cloud's blocks, whose size is reported: hgs_cloud_device_bytes).
template <typename A>
struct Buffer {
  void* p = nullptr;
  size_t cap = 0;
  Buffer() = default;
  Buffer(const Buffer&) = delete;
  Buffer& operator=(const Buffer&) = delete;
  Buffer(Buffer&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
  Buffer& operator=(Buffer&& o) noexcept {
    if (this != &o) release(), p = std::exchange(o.p, nullptr), cap = std::exchange(o.cap, 0);
    return *this;
  }
  ~Buffer() { release(); }
  hipError_t alloc(size_t bytes) {
    release();
    const hipError_t e = A::alloc(&p, bytes);
    if (e == hipSuccess) cap = bytes;
    else p = nullptr;
    return e;
  }
  hipError_t reserve(size_t bytes) { return bytes <= cap ? hipSuccess : alloc(bytes + bytes / 4 + 256); }
  void release() {
    if (p) A::free(p);
    p = nullptr;
    cap = 0;
  }
  template <typename T>
  T* as() const {
    return reinterpret_cast<T*>(p);
  }
};
using DeviceBuffer = Buffer<DeviceAlloc>;
using PinnedBuffer = Buffer<PinnedAlloc>;

// Small host -> device uploads (cloud descriptors, guesses, work plans) go through a ring of pinned slots, each guarded by an event recorded
// behind its copy: a slot is rewritten only after the copy that read it has completed, so no caller has to synchronise the stream just to make a
// staging buffer reusable (rounds 1-4 did, once per index build, once per covariance pass, once per NDT plan: 15-30 us of host latency each on
// the single-registration path).
struct PinnedRing {
  static constexpr int kSlots = 8;
  PinnedBuffer buf[kSlots];
  hipEvent_t ev[kSlots] = {};
  bool pending[kSlots] = {};
  int next = 0;
  // a slot of at least `bytes` whose previous upload has completed; *slot identifies it for commit()
  hipError_t stage(size_t bytes, void** host, int* slot) {
    const int k = next;
    next = (next + 1) % kSlots;
    if (pending[k]) {
      const hipError_t e = hipEventSynchronize(ev[k]);
      if (e != hipSuccess) return e;
      pending[k] = false;
    }
    const hipError_t e = buf[k].reserve(bytes);
    if (e != hipSuccess) return e;
    *host = buf[k].p, *slot = k;
    return hipSuccess;
  }
  // the copy out of the slot has been enqueued on `stream`
  hipError_t commit(int slot, hipStream_t stream) {
    if (!ev[slot]) {
      const hipError_t e = hipEventCreateWithFlags(&ev[slot], hipEventDisableTiming);
      if (e != hipSuccess) return e;
    }
    const hipError_t e = hipEventRecord(ev[slot], stream);
    if (e == hipSuccess) pending[slot] = true;
    return e;
  }
  // H2D of `bytes` from `src` (any host memory) to `dst` through a slot
  hipError_t upload(void* dst, const void* src, size_t bytes, hipStream_t stream) {
    void* host = nullptr;
    int slot = 0;
    hipError_t e = stage(bytes, &host, &slot);
    if (e != hipSuccess) return e;
    std::memcpy(host, src, bytes);
    e = hipMemcpyAsync(dst, host, bytes, hipMemcpyHostToDevice, stream);
    if (e != hipSuccess) return e;
    return commit(slot, stream);
  }
  PinnedRing() = default;
  PinnedRing(const PinnedRing&) = delete;
  PinnedRing& operator=(const PinnedRing&) = delete;
  ~PinnedRing() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

// A few helper threads that pack point records next to the calling thread (upload_points_packed).  One core packs a cold 119 k-point sweep (3.8 MB
// read, 1.9 MB written) in 150 us; kWorkers + 1 threads in 59 us (same box, scripts/probes/upload_probe.py: hgs_set_source 0.164 -> 0.075 ms of a
// 0.39 ms odometry step).  The workers only touch host memory (no HIP call); they sleep on a condition variable between uploads and are joined by
// the destructor (~hgs_handle runs it before the pinned memory the workers write into is freed).
struct PackPool {
  static constexpr int kWorkers = 3;
  struct Job {
    const char* src = nullptr;
    float* dst = nullptr;
    size_t n = 0, stride = 0, chunk = 0, nchunks = 0;
    bool has_intensity = false;
    bool scatter = false;  // false: pack strided records at src into float4 at dst (upload); true: scatter float4 at src into strided records at dst (hgs_transform_source)
    std::atomic<size_t> next{0};
    std::atomic<unsigned char>* ready = nullptr;  // [nchunks]
  };
  std::vector<std::thread> threads;
  std::mutex m;
  std::condition_variable cv;
  Job* job = nullptr;   // guarded by m
  unsigned long generation = 0;
  int active = 0;       // workers inside the current job
  bool stop = false;

  static void pack_chunk(const Job& j, size_t c) {
    const size_t i0 = c * j.chunk, m = std::min(j.chunk, j.n - i0);
    if (j.scatter) {  // x, y, z (and data[3] = 1 when the record has room for it) of the caller's records; everything else in them is left alone
      const float* s4 = reinterpret_cast<const float*>(j.src) + 4 * i0;
      char* o = reinterpret_cast<char*>(j.dst) + i0 * j.stride;
      for (size_t i = 0; i < m; i++) {
        float* f = reinterpret_cast<float*>(o + i * j.stride);
        f[0] = s4[4 * i], f[1] = s4[4 * i + 1], f[2] = s4[4 * i + 2];
        if (j.stride >= 16) f[3] = 1.0f;
      }
      j.ready[c].store(1, std::memory_order_release);
      return;
    }
    const char* s0 = j.src + i0 * j.stride;
    float* dst = j.dst + 4 * i0;
    if (j.has_intensity) {
      for (size_t i = 0; i < m; i++) {
        const float* f = reinterpret_cast<const float*>(s0 + i * j.stride);
        dst[4 * i] = f[0], dst[4 * i + 1] = f[1], dst[4 * i + 2] = f[2], dst[4 * i + 3] = f[4];
      }
    } else {
      for (size_t i = 0; i < m; i++) {
        const float* f = reinterpret_cast<const float*>(s0 + i * j.stride);
        dst[4 * i] = f[0], dst[4 * i + 1] = f[1], dst[4 * i + 2] = f[2], dst[4 * i + 3] = 0.f;
      }
    }
    j.ready[c].store(1, std::memory_order_release);
  }
  // takes chunks until none is left; false if there was none
  static bool help(Job& j) {
    const size_t c = j.next.fetch_add(1, std::memory_order_relaxed);
    if (c >= j.nchunks) return false;
    pack_chunk(j, c);
    return true;
  }
  void worker() {
    unsigned long seen = 0;
    for (;;) {
      Job* j = nullptr;
      {
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [&] { return stop || (job && generation != seen); });
        if (stop) return;
        seen = generation, j = job, active++;
      }
      while (help(*j)) {
      }
      {
        std::lock_guard<std::mutex> lk(m);
        active--;
      }
      cv.notify_all();
    }
  }
  void post(Job* j) {
    {
      std::lock_guard<std::mutex> lk(m);
      if (threads.empty())
        for (int i = 0; i < kWorkers; i++) threads.emplace_back([this] { worker(); });
      job = j, generation++;
    }
    cv.notify_all();
  }
  // the job's memory may go away after this: no worker is inside it, none will enter it
  void retire() {
    std::unique_lock<std::mutex> lk(m);
    job = nullptr;
    cv.wait(lk, [&] { return active == 0; });
  }
  void shutdown() {
    {
      std::lock_guard<std::mutex> lk(m);
      stop = true;
    }
    cv.notify_all();
    for (std::thread& t : threads) t.join();
    threads.clear();
  }
  ~PackPool() { shutdown(); }
};

}  // namespace hgs
