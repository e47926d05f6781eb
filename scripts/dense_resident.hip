// dense_resident.hip — standalone harness behind k_icount_dense_resident (the dense count for a plan the Infinity Cache can
// hold).  Not part of the product: it includes the product kernels, checks every variant's counts against a host popcount and
// times them with HIP events over back-to-back launches, on working sets that are re-read by every launch (128 ... 512 MiB)
// and on 4 x 256 MiB cycled (cold).  Variants:
//   (a) k_icount_dense<16>, the `accum` form: what the library launches on cold data
//   (b) k_icount_dense_resident, same direction every launch, grids of 256 / 512 / 768 / 1024 blocks
//   (c) k_icount_dense_resident, direction alternating from launch to launch, same grids
//   (d) (c) with the non-temporal hint on the loads (kStream): does the hint keep the lines out of the L3?
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 scripts/dense_resident.hip -o build_variants/dense_resident
//   build_variants/dense_resident > profiles/dense_resident.txt
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../featurebase_amd/csrc/fbk_kernels.hip.h"

using fbk::u64;

#define CK(x)                                                                   \
  do {                                                                          \
    hipError_t e = (x);                                                         \
    if (e != hipSuccess) {                                                      \
      fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e));                    \
      exit(1);                                                                  \
    }                                                                           \
  } while (0)

__global__ void k_fill(u64* p, size_t n, u64 seed) {
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    u64 z = (i + seed) * 0x9E3779B97F4A7C15ull;  // splitmix64 finaliser
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    p[i] = z ^ (z >> 31);
  }
}

namespace {

constexpr size_t kRowBytes = 16 * 8192;
constexpr uint32_t kMaxPairs = 2048;  // 512 MiB read per launch
constexpr int kSets = 4;              // cold: 4 x 256 MiB
constexpr uint32_t kSetPairs = 1024;
constexpr int kLaunches = 240, kWarm = 24, kRepeats = 3;

enum Variant { kShipped, kSameDir, kAlternating, kAlternatingStream };

struct Operands {
  const uint8_t *a, *b;
};

uint32_t* d_rows;
u64 *d_out, *d_accum;
hipEvent_t e0, e1;

// one launch of variant v; `k` counts the launches on these operands (the alternating variants flip on it)
void launch(Variant v, uint32_t grid, Operands o, uint32_t n, int k) {
  switch (v) {
    case kShipped:
      hipLaunchKernelGGL(fbk::k_icount_dense<16>, dim3(n), dim3(256), 0, 0, o.a, d_rows, o.b, d_rows, d_out, (u64*)nullptr, (uint32_t*)nullptr, n, d_accum);
      break;
    case kSameDir:
      hipLaunchKernelGGL(fbk::k_icount_dense_resident<false>, dim3(std::min(n, grid)), dim3(256), 0, 0, o.a, d_rows, o.b, d_rows, d_out, (u64*)nullptr, (uint32_t*)nullptr, n, d_accum, 0u);
      break;
    case kAlternating:
      hipLaunchKernelGGL(fbk::k_icount_dense_resident<false>, dim3(std::min(n, grid)), dim3(256), 0, 0, o.a, d_rows, o.b, d_rows, d_out, (u64*)nullptr, (uint32_t*)nullptr, n, d_accum, uint32_t(k & 1));
      break;
    case kAlternatingStream:
      hipLaunchKernelGGL(fbk::k_icount_dense_resident<true>, dim3(std::min(n, grid)), dim3(256), 0, 0, o.a, d_rows, o.b, d_rows, d_out, (u64*)nullptr, (uint32_t*)nullptr, n, d_accum, uint32_t(k & 1));
      break;
  }
}

// kRepeats timed regions of kLaunches launches each, cycling over `sets`; microseconds per launch, ascending
void time_variant(const char* name, Variant v, uint32_t grid, const std::vector<Operands>& sets, uint32_t n, const std::vector<u64>& ref) {
  double us[kRepeats];
  for (int r = 0; r < kRepeats; ++r) {
    for (int k = 0; k < kWarm; ++k) launch(v, grid, sets[k % sets.size()], n, int(k / sets.size()));
    CK(hipEventRecord(e0, 0));
    for (int k = 0; k < kLaunches; ++k) launch(v, grid, sets[k % sets.size()], n, int(k / sets.size()));
    CK(hipEventRecord(e1, 0));
    CK(hipEventSynchronize(e1));
    CK(hipGetLastError());
    float ms;
    CK(hipEventElapsedTime(&ms, e0, e1));
    us[r] = ms * 1e3 / kLaunches;
  }
  std::sort(us, us + kRepeats);
  // counts of set 0 against the host popcount, both directions: out[] all written (sentinel), accum = the sum
  bool ok = true;
  for (int k = 0; k < 2; ++k) {
    CK(hipMemset(d_out, 0xEE, kMaxPairs * 8));
    CK(hipMemset(d_accum, 0, 8));
    launch(v, grid, sets[0], n, k);
    std::vector<u64> got(n);
    u64 acc = 0, want = 0;
    CK(hipMemcpy(got.data(), d_out, n * 8, hipMemcpyDeviceToHost));
    CK(hipMemcpy(&acc, d_accum, 8, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; ++i) {
      want += ref[i];
      if (got[i] != ref[i]) ok = false;
    }
    if (acc != want) ok = false;
  }
  const double bytes = 2.0 * n * kRowBytes;
  printf("  %-44s grid %4u  %7.2f %7.2f %7.2f us  (median %6.0f GB/s)  counts %s\n", name, v == kShipped ? n : std::min(n, grid), us[0], us[1], us[2],
         bytes / us[1] / 1e3, ok ? "ok" : "WRONG");
  fflush(stdout);
  if (!ok) exit(2);
}

}  // namespace

int main() {
  // set 0 is the largest (2048 pairs: the re-read working sets are its first n pairs); sets 1..3 hold 1024 pairs each
  std::vector<uint8_t*> A(kSets), B(kSets);
  for (int s = 0; s < kSets; ++s) {
    const size_t bytes = (s == 0 ? kMaxPairs : kSetPairs) * kRowBytes;
    CK(hipMalloc(&A[s], bytes));
    CK(hipMalloc(&B[s], bytes));
    hipLaunchKernelGGL(k_fill, dim3(4096), dim3(256), 0, 0, (u64*)A[s], bytes / 8, (u64)(2 * s + 1) << 40);
    hipLaunchKernelGGL(k_fill, dim3(4096), dim3(256), 0, 0, (u64*)B[s], bytes / 8, (u64)(2 * s + 2) << 40);
  }
  CK(hipMalloc(&d_rows, kMaxPairs * 4));
  CK(hipMalloc(&d_out, kMaxPairs * 8));
  CK(hipMalloc(&d_accum, 8));
  std::vector<uint32_t> hr(kMaxPairs);
  for (uint32_t i = 0; i < kMaxPairs; ++i) hr[i] = i;
  CK(hipMemcpy(d_rows, hr.data(), kMaxPairs * 4, hipMemcpyHostToDevice));
  CK(hipDeviceSynchronize());
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));

  // host popcount of set 0
  std::vector<u64> ref(kMaxPairs);
  {
    std::vector<u64> ha(kMaxPairs * kRowBytes / 8), hb(kMaxPairs * kRowBytes / 8);
    CK(hipMemcpy(ha.data(), A[0], ha.size() * 8, hipMemcpyDeviceToHost));
    CK(hipMemcpy(hb.data(), B[0], hb.size() * 8, hipMemcpyDeviceToHost));
    const size_t wpr = kRowBytes / 8;
    for (uint32_t i = 0; i < kMaxPairs; ++i) {
      u64 c = 0;
      for (size_t w = 0; w < wpr; ++w) c += (u64)__builtin_popcountll(ha[i * wpr + w] & hb[i * wpr + w]);
      ref[i] = c;
    }
  }

  hipDeviceProp_t prop;
  CK(hipGetDeviceProperties(&prop, 0));
  printf("dense_resident: %s, %d CUs; %d launches per timed region after %d warm-up launches, %d regions: min / median / max us per launch\n", prop.gcnArchName,
         prop.multiProcessorCount, kLaunches, kWarm, kRepeats);
  const uint32_t grids[4] = {256, 512, 768, 1024};
  const uint32_t pairs[5] = {512, 768, 1024, 1280, 2048};
  for (uint32_t n : pairs) {
    printf("working set %u MiB (%u row pairs), re-read by every launch\n", unsigned(2 * n * kRowBytes >> 20), n);
    const std::vector<Operands> one = {{A[0], B[0]}};
    time_variant("(a) k_icount_dense<16>, nt loads, accum", kShipped, 0, one, n, ref);
    for (uint32_t g : grids) time_variant("(b) resident, same direction", kSameDir, g, one, n, ref);
    for (uint32_t g : grids) time_variant("(c) resident, alternating direction", kAlternating, g, one, n, ref);
    for (uint32_t g : grids) time_variant("(d) resident, alternating, nt loads", kAlternatingStream, g, one, n, ref);
  }
  printf("working set %d x 256 MiB cycled (cold), %u row pairs per launch\n", kSets, kSetPairs);
  std::vector<Operands> cyc;
  for (int s = 0; s < kSets; ++s) cyc.push_back({A[s], B[s]});
  time_variant("(a) k_icount_dense<16>, nt loads, accum", kShipped, 0, cyc, kSetPairs, ref);
  for (uint32_t g : grids) time_variant("(b) resident, same direction", kSameDir, g, cyc, kSetPairs, ref);
  for (uint32_t g : grids) time_variant("(c) resident, alternating direction", kAlternating, g, cyc, kSetPairs, ref);
  time_variant("(d) resident, alternating, nt loads", kAlternatingStream, 512, cyc, kSetPairs, ref);
  return 0;
}
