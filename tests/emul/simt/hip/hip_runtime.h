// SIMT emulation shim — TEST INFRASTRUCTURE, never part of the product.
//
// A stand-in for <hip/hip_runtime.h> that lets the product sources (hdl_graph_slam_amd/csrc/*.hip, unchanged) be compiled
// for the host CPU: every GPU thread of a launched block becomes a fiber (cooperative user-level context) inside one OS
// thread, the 64 fibers of a wave meet in the cross-lane operations (__ballot, __shfl_down, readlane, wave barriers) and the
// fibers of a block in __syncthreads, blocks run one after the other, `__shared__` becomes a function-local static.  The
// HIP runtime API is mapped to malloc / memcpy; launches are synchronous.  tests/emul/simt_runtime.cpp holds the scheduler.
// Built by tests/emul/simt.py into tests/emul/libhgs_simt.so, which exports the same C-ABI as libhgs_hip.so and is loaded by
// tests only (tests/test_simt_kernels_host.py): the kernels' and the engine's logic is exercised without a GPU.
#pragma once
#ifndef __HIPCC__
#define __HIPCC__ 1
#endif
#define HGS_SIMT_EMULATION 1
#define HGS_OPAQUE_POINTER(p) asm volatile("" : "+r"(p))
#define HGS_WAIT_VMEM() ((void)0)
#define HGS_OPAQUE_VGPR64(x) ((void)0)
#define HGS_LOAD_GLOBAL_XYZ(p) make_float4((p)->x, (p)->y, (p)->z, 0.f)
#define HGS_OPAQUE_OFFSET(off) asm volatile("" : "+r"(off))
#define HGS_WAIT_VMEM_TRACKED() ((void)0)
#define __builtin_amdgcn_sched_barrier(mask) ((void)0)
#define __builtin_amdgcn_s_setprio(p) ((void)0)
#define HGS_LANE_ID(dst) ((dst) = (int)(threadIdx.x & 63))
#define __HIP_MEMORY_SCOPE_SYSTEM 5
#define __hip_atomic_store(p, v, order, scope) (*(p) = (v))
#define __HIP_MEMORY_SCOPE_WORKGROUP 3
#define __HIP_MEMORY_SCOPE_AGENT 4
#define __hip_atomic_load(p, order, scope) (*(p))
#define HGS_COMPILER_MEMORY_BARRIER() asm volatile("" ::: "memory")
#define __hip_atomic_fetch_add(p, v, order, scope) atomicAdd((p), (v))  /* one OS thread runs every fiber (atomicAdd below) */

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <functional>

// ------------------------------------------------------------------------------------------------ language
#define __host__
#define __device__
#define __global__
#define __forceinline__ inline
#define __noinline__ __attribute__((noinline))
#define __shared__ static thread_local   // one block at a time PER HOST THREAD (engines driven from several threads)
#define __launch_bounds__(...)
#define amdgpu_waves_per_eu(...)  // __attribute__((amdgpu_waves_per_eu(n))) -> __attribute__(())

struct alignas(16) float4 {
  float x, y, z, w;
};
static inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }

struct int2 {
  int x, y;
};
static inline int2 make_int2(int x, int y) { return int2{x, y}; }

struct dim3 {
  unsigned x, y, z;
  dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};

namespace simt {
struct Idx {
  unsigned x, y, z;
};
struct Thread {
  Idx tid;
  int lane, wave;
};
extern thread_local Thread* g_cur;
extern unsigned long long g_record_fetches, g_waves_launched;   // statistics (fetch_record calls of lane 0, waves started)
extern thread_local Idx g_block, g_block_dim, g_grid_dim;
extern std::atomic<long long> g_live_blocks, g_live_streams, g_live_events;  // objects the runtime calls below have handed out and not taken back (simt_read_live_objects)

// all-to-all exchange of one 64-bit value among the live lanes of the calling lane's wave; returns the mask of lanes that took
// part, out[l] = value of lane l.  `kind` must agree among the participants (a mismatch means divergent collectives).
unsigned long long wave_exchange(int kind, unsigned long long mine, unsigned long long out[64]);
void block_barrier();
void launch(dim3 grid, dim3 block, const std::function<void()>& body);

template <typename T>
static inline unsigned long long to_bits(T v) {
  static_assert(sizeof(T) <= 8, "cross-lane operands are at most 64 bits");
  unsigned long long b = 0;
  memcpy(&b, &v, sizeof(T));
  return b;
}
template <typename T>
static inline T from_bits(unsigned long long b) {
  T v;
  memcpy(&v, &b, sizeof(T));
  return v;
}
static inline unsigned long long ballot(bool p, int site = 0) {
  unsigned long long all[64];
  const unsigned long long live = wave_exchange(1 | (site << 4), p ? 1ull : 0ull, all);
  unsigned long long m = 0;
  for (int l = 0; l < 64; l++)
    if (((live >> l) & 1ull) && all[l]) m |= 1ull << l;
  return m;
}
template <typename T>
static inline T shfl_down(T v, unsigned delta, int site = 0) {
  unsigned long long all[64];
  const unsigned long long live = wave_exchange(2 | (site << 4), to_bits(v), all);
  const unsigned src = (unsigned)g_cur->lane + delta;
  return (src < 64u && ((live >> src) & 1ull)) ? from_bits<T>(all[src]) : v;
}
template <typename T>
static inline T readlane(T v, int lane, int site = 0) {
  unsigned long long all[64];
  wave_exchange(3 | (site << 4), to_bits(v), all);
  return from_bits<T>(all[lane & 63]);
}
// v_permlane32_swap / v_permlane16_swap (gfx950): {new first operand, new second operand}
struct Pair32 {
  unsigned v[2];
  unsigned operator[](int i) const { return v[i]; }
};
static inline Pair32 permlane_swap(unsigned a, unsigned b, int width, int site = 0) {
  unsigned long long all[64];
  wave_exchange(5 | (site << 4), ((unsigned long long)b << 32) | a, all);
  const int l = g_cur->lane;
  auto A = [&](int i) { return (unsigned)all[i & 63]; };
  auto B = [&](int i) { return (unsigned)(all[i & 63] >> 32); };
  Pair32 r;
  if (width == 32) {  // upper 32 lanes of the first <-> lower 32 lanes of the second
    r.v[0] = l < 32 ? A(l) : B(l - 32);
    r.v[1] = l < 32 ? A(l + 32) : B(l);
  } else {            // odd 16-lane rows of the first <-> even rows of the second
    const bool odd = (l >> 4) & 1;
    r.v[0] = odd ? B(l - 16) : A(l);
    r.v[1] = odd ? B(l) : A(l + 16);
  }
  return r;
}
// DPP row_shr:n with bound_ctrl (a lane whose source lies outside its 16-lane row reads 0) — the only control used
static inline unsigned update_dpp_row_shr(unsigned src, int ctrl, int site = 0) {
  unsigned long long all[64];
  wave_exchange(6 | (site << 4), src, all);
  const int l = g_cur->lane, n = ctrl & 15;
  if (ctrl < 0x111 || ctrl > 0x11f) abort();
  return (l & 15) >= n ? (unsigned)all[l - n] : 0u;
}
// v_mfma_f64_16x16x4_f64: D = A * B + C with one f64 of A and of B per lane, A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15],
// and four f64 of C / D per lane, register r holding row (lane >> 4) + 4 r of column lane & 15 (MI355X_MICROARCH.md, "f64 MFMA does NOT use
// these maps").  The products are accumulated by fma in k order — the callers feed integer-valued doubles, for which any order is exact.
typedef double f64x4 __attribute__((ext_vector_type(4)));
static inline f64x4 mfma_f64_16x16x4(double a, double b, f64x4 c, int site = 0) {
  unsigned long long A[64], B[64];
  const unsigned long long live_a = wave_exchange(7 | (site << 4), to_bits(a), A);
  wave_exchange(8 | (site << 4), to_bits(b), B);
  if (live_a != ~0ull) abort();  // a matrix instruction of a partial wave: not what the kernels mean
  const int l = g_cur->lane, col = l & 15;
  f64x4 d = c;
  for (int r = 0; r < 4; r++) {
    const int row = (l >> 4) + 4 * r;
    double acc = c[r];
    for (int k = 0; k < 4; k++) acc = fma(from_bits<double>(A[row + 16 * k]), from_bits<double>(B[col + 16 * k]), acc);
    d[r] = acc;
  }
  return d;
}
static inline void wave_barrier(int site = 0) {
  unsigned long long all[64];
  wave_exchange(4 | (site << 4), 0ull, all);
}
}  // namespace simt

#define threadIdx (simt::g_cur->tid)
#define blockIdx simt::g_block
#define blockDim simt::g_block_dim
#define gridDim simt::g_grid_dim

#define __syncthreads() simt::block_barrier()
// the source line identifies the call site: lanes of one wave that meet in the same KIND of operation at different sites (an
// operation inside divergent code) are reported, not silently combined
#define __ballot(p) simt::ballot((p) != 0, __LINE__)
#define __shfl_down(v, d, ...) simt::shfl_down((v), (unsigned)(d), __LINE__)
#define __lane_id() ((unsigned)simt::g_cur->lane)
#define __builtin_amdgcn_readlane(v, l) simt::readlane((v), (l), __LINE__)
#define __builtin_amdgcn_wave_barrier() simt::wave_barrier(__LINE__)
#define __builtin_amdgcn_readfirstlane(v) (v)  /* only used on values that are wave-uniform by construction */
#define __builtin_amdgcn_permlane32_swap(a, b, fi, bc) simt::permlane_swap((a), (b), 32, __LINE__)
#define __builtin_amdgcn_permlane16_swap(a, b, fi, bc) simt::permlane_swap((a), (b), 16, __LINE__)
#define __builtin_amdgcn_update_dpp(old, src, ctrl, rm, bm, bc) simt::update_dpp_row_shr((src), (ctrl), __LINE__)
#define __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, cbsz, abid, blgp) simt::mfma_f64_16x16x4((a), (b), (c), __LINE__)
#define __builtin_amdgcn_fmed3f(a, b, c) fmaxf(fminf((a), (b)), fminf(fmaxf((a), (b)), (c)))
#define __threadfence_system() ((void)0)
#define __threadfence() ((void)0)

template <typename T>
static inline T min(T a, T b) {
  return b < a ? b : a;
}
template <typename T>
static inline T max(T a, T b) {
  return a < b ? b : a;
}
static inline int __float_as_int(float f) { return simt::from_bits<int>(simt::to_bits(f)); }
static inline unsigned __float_as_uint(float f) { return simt::from_bits<unsigned>(simt::to_bits(f)); }
static inline float __int_as_float(int i) { return simt::from_bits<float>(simt::to_bits(i)); }
static inline float __uint_as_float(unsigned u) { return simt::from_bits<float>(simt::to_bits(u)); }
static inline int __clz(int x) { return x ? __builtin_clz((unsigned)x) : 32; }
static inline int __clzll(long long x) { return x ? __builtin_clzll((unsigned long long)x) : 64; }
static inline int __ffsll(long long x) { return __builtin_ffsll(x); }
static inline int __popcll(unsigned long long x) { return __builtin_popcountll(x); }

// one OS thread runs every fiber: plain read-modify-write is atomic
template <typename T>
static inline T atomicAdd(T* p, T v) {
  const T o = *p;
  *p = o + v;
  return o;
}
template <typename T>
static inline T atomicMin(T* p, T v) {
  const T o = *p;
  *p = v < o ? v : o;
  return o;
}
template <typename T>
static inline T atomicMax(T* p, T v) {
  const T o = *p;
  *p = v > o ? v : o;
  return o;
}
template <typename T>
static inline T atomicOr(T* p, T v) {
  const T o = *p;
  *p = o | v;
  return o;
}
template <typename T>
static inline T atomicExch(T* p, T v) {
  const T o = *p;
  *p = v;
  return o;
}
static inline long long __double_as_longlong(double d) { return simt::from_bits<long long>(simt::to_bits(d)); }
static inline double __longlong_as_double(long long i) { return simt::from_bits<double>(simt::to_bits(i)); }
static inline double __hiloint2double(int hi, int lo) { return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo)); }
template <typename T>
static inline T atomicCAS(T* p, T expected, T desired) {
  const T o = *p;
  if (o == expected) *p = desired;
  return o;
}

#define hipLaunchKernelGGL(kernel, grid, block, shmem, stream, ...) simt::launch(dim3(grid), dim3(block), [=]() { kernel(__VA_ARGS__); })

// ------------------------------------------------------------------------------------------------ runtime API
typedef int hipError_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorNotReady = 600 };
typedef void* hipStream_t;
typedef void* hipEvent_t;
enum hipMemcpyKind { hipMemcpyHostToHost = 0, hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2, hipMemcpyDeviceToDevice = 3, hipMemcpyDefault = 4 };
enum { hipStreamNonBlocking = 1, hipEventDisableTiming = 2, hipHostMallocDefault = 0 };

static inline const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "success" : "simt emulation: allocation failed"; }
static inline hipError_t hipGetLastError() { return hipSuccess; }
static inline hipError_t hipSetDevice(int) { return hipSuccess; }
static inline hipError_t hipGetDeviceCount(int* n) {
  *n = 1;
  return hipSuccess;
}
template <typename T>
static inline hipError_t hipMalloc(T** p, size_t bytes) {
  *p = (T*)aligned_alloc(256, (bytes + 255) / 256 * 256 + 256);
  if (*p) simt::g_live_blocks++;
  return *p ? hipSuccess : hipErrorOutOfMemory;
}
static inline hipError_t hipFree(void* p) {
  if (p) simt::g_live_blocks--;
  free(p);
  return hipSuccess;
}
template <typename T>
static inline hipError_t hipHostMalloc(T** p, size_t bytes, unsigned = 0) {
  return hipMalloc(p, bytes);
}
static inline hipError_t hipHostFree(void* p) { return hipFree(p); }
static inline hipError_t hipMemcpyAsync(void* dst, const void* src, size_t n, hipMemcpyKind, hipStream_t = nullptr) {
  memmove(dst, src, n);
  return hipSuccess;
}
static inline hipError_t hipMemcpy(void* dst, const void* src, size_t n, hipMemcpyKind k) { return hipMemcpyAsync(dst, src, n, k); }
static inline hipError_t hipMemsetAsync(void* dst, int v, size_t n, hipStream_t = nullptr) {
  memset(dst, v, n);
  return hipSuccess;
}
static inline hipError_t hipStreamCreate(hipStream_t* s) {
  *s = malloc(1);
  simt::g_live_streams++;
  return hipSuccess;
}
static inline hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { return hipStreamCreate(s); }
static inline hipError_t hipStreamDestroy(hipStream_t s) {
  simt::g_live_streams--;
  free(s);
  return hipSuccess;
}
static inline hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
static inline hipError_t hipStreamQuery(hipStream_t) { return hipSuccess; }
static inline hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned) { return hipSuccess; }
static inline hipError_t hipEventCreate(hipEvent_t* e) {
  *e = malloc(1);
  simt::g_live_events++;
  return hipSuccess;
}
static inline hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return hipEventCreate(e); }
static inline hipError_t hipEventDestroy(hipEvent_t e) {
  simt::g_live_events--;
  free(e);
  return hipSuccess;
}
static inline hipError_t hipEventRecord(hipEvent_t, hipStream_t = nullptr) { return hipSuccess; }
static inline hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
static inline hipError_t hipEventQuery(hipEvent_t) { return hipSuccess; }
static inline hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) {
  *ms = 0.f;
  return hipSuccess;
}
