// What does ONE dependent scalar read of the kernel arguments cost a block, in front of its first vector load, under
// k_mbatch's launch conditions?  1 264 blocks x 256 threads with 24 KB of LDS each, an 8 KB argument block whose words
// change with every launch (so the first touch of every line misses), launches back to back on one stream.  A block
// walks a chain of D dependent scalar reads through the arguments — D - 1 index words, each on a line of its own, then
// a pointer — and only then can its vector load leave.  The start of the chain depends on the t0 stamp (a term that is
// always zero, which the compiler cannot know), so no read of the chain can be scheduled above the stamp, and the
// stamp itself is taken behind a wait.  t1 is taken when the vector load is back.
//   D = 0: the pointer is a leading argument, not on the chain — one read in a plain build (free to move above t0), none
//          with -mllvm -amdgpu-kernarg-preload-count=2, where it arrives in SGPRs with the wavefront.
// The cost of a dependent trip is the slope of (t1 - t0) over D.
//   hipcc --offload-arch=gfx950 -O3 [-mllvm -amdgpu-kernarg-preload-count=2] kernarg_chain.hip -o kernarg_chain[_pre].bin
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

constexpr unsigned kWords = 512, kMask = kWords - 1u;  // every index is masked: no read leaves the arrays
constexpr unsigned kBlocks = 1264, kLaunches = 300, kWarm = 50, kSlack = 4096;
struct Args {  // 2 KB of index words + 5.9 KB of pointers: 7 952 bytes, 8 KB with the leading arguments
  unsigned w[kWords];
  const float* p[736];
};
static_assert(sizeof(Args) + 32 <= 8192 && sizeof(Args) >= 7900, "an 8 KB argument block");

template <int D>
__global__ __launch_bounds__(256) void k_chain(const float* __restrict__ p0, unsigned start,
                                               unsigned long long* __restrict__ stamp, float* __restrict__ out,
                                               const Args A) {
  __shared__ float lds[6144];  // 24 KB: as many blocks per CU as k_mbatch's
  const unsigned long long t0 = wall_clock64();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  const unsigned zero = unsigned(t0 >> 63);  // (0 for the next 2 900 years)
  const float* p = p0 + zero;
  if (D > 0) {
    unsigned j = (17u + zero) & kMask;  // the chain's head sits at a fixed word: nothing to read before the first trip
#pragma unroll
    for (int h = 1; h < D; ++h) j = A.w[j] & kMask;
    p = A.p[j];
  }
  float v = p[blockIdx.x * 256u + threadIdx.x];
  asm volatile("s_waitcnt vmcnt(0)" : "+v"(v)::"memory");
  const unsigned long long t1 = wall_clock64();
  const unsigned at = (blockIdx.x % 23u) * 256u;
  lds[at + threadIdx.x] = v + float(start);
  __syncthreads();
  out[blockIdx.x * 256u + threadIdx.x] = lds[at + (threadIdx.x ^ 1u)];
  if (threadIdx.x == 0) { stamp[2u * blockIdx.x] = t0; stamp[2u * blockIdx.x + 1u] = t1 - t0; }
}

struct Result { double p10, p50, p90, mean, launch_us; };

template <int D>
int run(const float* in, float* out, unsigned long long* st, std::vector<unsigned long long>& h, Result& r) {
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  Args A;
  for (unsigned l = 0; l < kLaunches; ++l) {
    // fresh values everywhere; the chain of this launch: word 17 -> D - 1 random words 16 apart (a 64-byte line each)
    for (unsigned i = 0; i < kWords; ++i) A.w[i] = unsigned(rand()) & kMask;
    for (auto& q : A.p) q = in + (unsigned(rand()) % kSlack);
    unsigned at = 17u, base = unsigned(rand()) % 32u;
    auto line_of = [&](int hop) { return (5u * unsigned(hop) + base) % 32u; };  // (distinct lines for hop < 32)
    for (bool clash = true; clash;) {  // ... and none of them the head's (line 1)
      clash = false;
      for (int hop = 1; hop < D; ++hop) clash = clash || line_of(hop) == 1u;
      if (clash) base = (base + 1u) % 32u;
    }
    for (int hop = 1; hop < D; ++hop) {
      const unsigned nx = line_of(hop) * 16u + 5u;
      A.w[at] = nx;
      at = nx;
    }
    if (l == kWarm) CK(hipEventRecord(e0, 0));
    hipLaunchKernelGGL(k_chain<D>, dim3(kBlocks), dim3(256), 0, 0, in + (l % kSlack), l, st + size_t(l) * 2u * kBlocks, out, A);
  }
  CK(hipEventRecord(e1, 0));
  CK(hipDeviceSynchronize());
  CK(hipGetLastError());
  float ms = 0.f;
  CK(hipEventElapsedTime(&ms, e0, e1));
  CK(hipMemcpy(h.data(), st, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  std::vector<double> d;
  double sum = 0.0;
  for (unsigned l = kWarm; l < kLaunches; ++l)
    for (unsigned b = 0; b < kBlocks; ++b) { d.push_back(double(h[(size_t(l) * kBlocks + b) * 2u + 1u]) / 100.0); sum += d.back(); }
  std::sort(d.begin(), d.end());
  r = {d[d.size() / 10], d[d.size() / 2], d[d.size() * 9 / 10], sum / double(d.size()), 1000.0 * ms / double(kLaunches - kWarm)};
  CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1));
  return 0;
}

int main() {
  float *in, *out;
  unsigned long long* st;
  const size_t n = size_t(kBlocks) * 256u + 2u * kSlack + 64u;
  CK(hipMalloc(&in, n * sizeof(float)));
  CK(hipMalloc(&out, n * sizeof(float)));
  CK(hipMalloc(&st, size_t(kLaunches) * kBlocks * 16u));
  CK(hipMemset(in, 0, n * sizeof(float)));
  std::vector<unsigned long long> h(size_t(kLaunches) * kBlocks * 2u);
  srand(12345);
  Result r[7];
  const int ds[5] = {0, 1, 2, 4, 6};
  for (int rep = 0; rep < 2; ++rep) {
    if (run<0>(in, out, st, h, r[0]) || run<1>(in, out, st, h, r[1]) || run<2>(in, out, st, h, r[2]) ||
        run<4>(in, out, st, h, r[4]) || run<6>(in, out, st, h, r[6]))
      return 1;
    for (int d : ds)
      printf("{\"rep\": %d, \"dependent_reads\": %d, \"first_load_back_us\": {\"p10\": %.2f, \"p50\": %.2f, \"p90\": %.2f, \"mean\": %.3f}, "
             "\"launch_us\": %.2f}\n", rep, d, r[d].p10, r[d].p50, r[d].p90, r[d].mean, r[d].launch_us);
    printf("{\"rep\": %d, \"us_per_dependent_read\": {\"mean_1_to_6\": %.3f, \"p50_1_to_6\": %.3f, \"mean_1_to_2\": %.3f, \"mean_2_to_4\": %.3f}}\n",
           rep, (r[6].mean - r[1].mean) / 5.0, (r[6].p50 - r[1].p50) / 5.0, r[2].mean - r[1].mean, (r[4].mean - r[2].mean) / 2.0);
  }
  return 0;
}
