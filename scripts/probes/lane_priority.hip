// Does the MI355X dispatcher let a highest-priority stream run ahead of a saturating grid on a default-priority stream?  Decides whether a batch's
// likely-long problems can run their LM rounds ahead of the crowd's ("Ordered lanes"): a late LM round is one dependent packet walk of
// 55-90 us in a few hundred blocks, a crowd linearize launch is tens of thousands of 256-thread blocks lasting a few hundred us.
//   load:  back-to-back grids of 30720 blocks x 256 threads, ~300 us each, on a default-priority non-blocking stream;
//   chain: 100 dependent launches of a 512-block kernel whose every thread runs a ~50 us dependent fma chain, on a second stream;
//   cases: the chain alone, under load at equal priority, under load at the highest priority (hipDeviceGetStreamPriorityRange), and, as the
//          engine's lanes would be, TWO loaded default streams against TWO highest-priority chains.
//   hipcc --offload-arch=gfx950 -O2 scripts/probes/lane_priority.hip -o scripts/probes/lane_priority_probe && scripts/probes/lane_priority_probe
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <vector>

#define CHECK(x)                                                                         \
  do {                                                                                   \
    const hipError_t e_ = (x);                                                           \
    if (e_ != hipSuccess) return printf("%s: %s\n", #x, hipGetErrorString(e_)), 1;       \
  } while (0)

// every thread: `iters` dependent fma's; nothing is read from memory, one guarded store keeps the loop alive
__global__ __launch_bounds__(256) void k_spin(int iters, float* sink) {
  float v = (float)threadIdx.x;
  for (int i = 0; i < iters; i++) v = fmaf(v, 1.0000001f, 1e-9f);
  if (v == -1.f) sink[0] = v;
}

static double now_us() {
  return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

constexpr int kLoadBlocks = 30720, kChainBlocks = 512, kChainLaunches = 100;

// time of ONE launch of `blocks` blocks on an idle device, us (events)
static int time_one(hipStream_t s, int blocks, int iters, float* sink, double* us) {
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  float best = 1e30f;
  for (int pass = 0; pass < 4; pass++) {
    CHECK(hipEventRecord(e0, s));
    hipLaunchKernelGGL(k_spin, dim3(blocks), dim3(256), 0, s, iters, sink);
    CHECK(hipEventRecord(e1, s));
    CHECK(hipEventSynchronize(e1));
    float ms = 0;
    CHECK(hipEventElapsedTime(&ms, e0, e1));
    if (pass && ms < best) best = ms;
  }
  *us = 1000.0 * best;
  (void)hipEventDestroy(e0), (void)hipEventDestroy(e1);
  return 0;
}

// Runs `chains.size()` dependent chains while `loads.size()` streams are kept full; returns the slowest chain's us per launch and how many load
// grids completed meanwhile.  The load is enqueued in slices with a host wait per slice, so the queue never runs dry and never grows without bound.
static int run_case(const std::vector<hipStream_t>& loads, const std::vector<hipStream_t>& chains, int load_iters, int chain_iters, float* sink,
                    double* us_per_launch, int* load_grids) {
  const int kLoadAhead = 8;  // grids in flight per load stream
  std::vector<hipEvent_t> c0(chains.size()), c1(chains.size());
  for (size_t i = 0; i < chains.size(); i++) {
    CHECK(hipEventCreate(&c0[i]));
    CHECK(hipEventCreate(&c1[i]));
  }
  std::vector<std::vector<hipEvent_t>> ring(loads.size(), std::vector<hipEvent_t>(kLoadAhead));
  for (auto& r : ring)
    for (auto& e : r) CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  int grids = 0;
  // fill the load streams, and wait until the first grid of each has finished: the device is saturated before the chain starts
  for (size_t l = 0; l < loads.size(); l++)
    for (int k = 0; k < kLoadAhead; k++) {
      hipLaunchKernelGGL(k_spin, dim3(kLoadBlocks), dim3(256), 0, loads[l], load_iters, sink);
      CHECK(hipEventRecord(ring[l][k], loads[l]));
    }
  for (size_t l = 0; l < loads.size(); l++, grids++) CHECK(hipEventSynchronize(ring[l][0]));
  for (size_t i = 0; i < chains.size(); i++) {
    CHECK(hipEventRecord(c0[i], chains[i]));
    for (int k = 0; k < kChainLaunches; k++) hipLaunchKernelGGL(k_spin, dim3(kChainBlocks), dim3(256), 0, chains[i], chain_iters, sink);
    CHECK(hipEventRecord(c1[i], chains[i]));
  }
  // keep the load fed until every chain is through: slot k of a ring is re-armed as soon as its grid has finished
  std::vector<int> head(loads.size(), 1);
  const double t_give_up = now_us() + 20e6;
  for (;;) {
    bool done = true;
    for (size_t i = 0; i < chains.size(); i++) done = done && hipEventQuery(c1[i]) == hipSuccess;
    if (done) break;
    if (now_us() > t_give_up) return puts("chain did not finish within 20 s"), 1;
    for (size_t l = 0; l < loads.size(); l++) {
      const int k = head[l] % kLoadAhead, prev = (head[l] + kLoadAhead - 1) % kLoadAhead;
      if (hipEventQuery(ring[l][k]) != hipSuccess) continue;
      grids++;
      hipLaunchKernelGGL(k_spin, dim3(kLoadBlocks), dim3(256), 0, loads[l], load_iters, sink);
      CHECK(hipEventRecord(ring[l][prev], loads[l]));
      head[l]++;
    }
  }
  double worst = 0;
  for (size_t i = 0; i < chains.size(); i++) {
    float ms = 0;
    CHECK(hipEventSynchronize(c1[i]));
    CHECK(hipEventElapsedTime(&ms, c0[i], c1[i]));
    if (1000.0 * ms / kChainLaunches > worst) worst = 1000.0 * ms / kChainLaunches;
  }
  for (auto s : loads) CHECK(hipStreamSynchronize(s));
  CHECK(hipDeviceSynchronize());
  for (auto& r : ring)
    for (auto& e : r) (void)hipEventDestroy(e);
  for (size_t i = 0; i < chains.size(); i++) (void)hipEventDestroy(c0[i]), (void)hipEventDestroy(c1[i]);
  *us_per_launch = worst;
  *load_grids = grids;
  return 0;
}

int main() {
  float* sink;
  if (hipMalloc(&sink, 64) != hipSuccess) return puts("no device"), 2;
  int least = 0, greatest = 0;
  CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
  printf("stream priority range: least %d, greatest %d%s\n", least, greatest, least == greatest ? "  (degenerate)" : "");
  hipStream_t load[2], equal[2], high[2];
  for (int i = 0; i < 2; i++) {
    CHECK(hipStreamCreateWithFlags(&load[i], hipStreamNonBlocking));
    CHECK(hipStreamCreateWithFlags(&equal[i], hipStreamNonBlocking));
    CHECK(hipStreamCreateWithPriority(&high[i], hipStreamNonBlocking, greatest));
    int p = 0;
    CHECK(hipStreamGetPriority(high[i], &p));
    if (i == 0) printf("highest-priority stream reports priority %d\n", p);
  }
  // calibrate the two kernels' fma counts to ~300 us (load grid) and ~50 us (chain kernel) on the idle device
  int load_iters = 20000, chain_iters = 20000;
  double us = 0;
  if (time_one(load[0], kLoadBlocks, load_iters, sink, &us)) return 1;
  load_iters = (int)(load_iters * 300.0 / us);
  if (time_one(load[0], kLoadBlocks, load_iters, sink, &us)) return 1;
  printf("load grid:    %d blocks x 256, %d fma per thread: %.1f us alone\n", kLoadBlocks, load_iters, us);
  if (time_one(equal[0], kChainBlocks, chain_iters, sink, &us)) return 1;
  chain_iters = (int)(chain_iters * 50.0 / us);
  if (time_one(equal[0], kChainBlocks, chain_iters, sink, &us)) return 1;
  printf("chain kernel: %d blocks x 256, %d fma per thread: %.1f us alone\n", kChainBlocks, chain_iters, us);

  struct Case {
    const char* name;
    int nload;
    hipStream_t* chain;
    int nchain;
  };
  const Case cases[] = {
      {"chain alone, default priority            ", 0, equal, 1},
      {"chain alone, highest priority            ", 0, high, 1},
      {"1 load stream,  1 chain, equal priority  ", 1, equal, 1},
      {"1 load stream,  1 chain, highest priority", 1, high, 1},
      {"2 load streams, 2 chains, equal priority  ", 2, equal, 2},
      {"2 load streams, 2 chains, highest priority", 2, high, 2},
  };
  for (int pass = 0; pass < 2; pass++) {
    printf("pass %d: us per chain launch (%d dependent launches; slowest chain), load grids completed meanwhile\n", pass, kChainLaunches);
    for (const Case& c : cases) {
      std::vector<hipStream_t> loads(load, load + c.nload), chains(c.chain, c.chain + c.nchain);
      int grids = 0;
      if (run_case(loads, chains, load_iters, chain_iters, sink, &us, &grids)) return 1;
      printf("  %s  %8.1f us   %4d grids\n", c.name, us, grids);
    }
  }
  return 0;
}
