// Microbenchmark of gfx950 global atomics on 16-byte RECORDS (device scope, no return) — the premise of k_mbatch's flush:
// what does a record's reduction cost as three instructions from one lane, as one instruction from four adjacent lanes,
// and with neighbouring records sharing a 64-byte line?  The launch's shape: 1 264 blocks x 256 threads, a block flushes
// `rpb` records (the headline's blocks hold ~56; 256 = every thread a record).
// hipcc --offload-arch=gfx950 -O3 atomic_rec.hip -o /tmp/atomic_rec && /tmp/atomic_rec   (one JSON line per shape)
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <algorithm>
#define CK(x) do{hipError_t e=(x); if(e!=hipSuccess){printf("%s: %s\n",#x,hipGetErrorString(e)); exit(1);} }while(0)

constexpr unsigned kBlocks = 1264, kThreads = 256, kMaxRpb = 256;

__device__ __forceinline__ uint32_t mix(uint32_t x) { x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; return x ^ (x >> 16); }

// (a) one lane per record, three instructions (today's merge(): zmx, imx, fst)
__global__ void k_rec3(uint32_t* tab, const uint32_t* idx, unsigned rpb, uint32_t salt) {
  for (unsigned j = threadIdx.x; j < rpb; j += kThreads) {
    const uint32_t r = idx[blockIdx.x * rpb + j], v = mix(r ^ salt);
    uint32_t* a = tab + size_t(r) * 4;
    atomicMax(a + 0, v);
    atomicMax(a + 1, v >> 1);
    atomicMax(a + 2, v >> 2);
  }
}
// (b) four adjacent lanes per record, one instruction; lanes whose word is >= `words` stay inactive
__global__ void k_rec1x4(uint32_t* tab, const uint32_t* idx, unsigned rpb, unsigned words, uint32_t salt) {
  for (unsigned q = threadIdx.x; q < rpb * 4u; q += kThreads) {
    const unsigned j = q >> 2, w = q & 3u;
    const uint32_t r = idx[blockIdx.x * rpb + j], v = mix(r ^ salt);
    if (w < words) atomicMax(tab + size_t(r) * 4 + w, v >> w);
  }
}
// (d) the 64-bit key, one lane per record
__global__ void k_key(unsigned long long* tab, const uint32_t* idx, unsigned rpb, uint32_t salt) {
  for (unsigned j = threadIdx.x; j < rpb; j += kThreads) {
    const uint32_t r = idx[blockIdx.x * rpb + j];
    atomicMin(&tab[r], ((unsigned long long)mix(r ^ salt) << 32) | r);
  }
}

static uint32_t rnd() { return uint32_t(rand()) * 32768u + uint32_t(rand()); }

int main() {
  const unsigned tables[2] = {16u * 22500u, 1440000u};
  const unsigned rpbs[2] = {64u, 256u};
  const unsigned n_idx = kBlocks * kMaxRpb;
  uint32_t *d_aux, *d_idx; unsigned long long* d_key;
  CK(hipMalloc(&d_aux, size_t(tables[1]) * 16)); CK(hipMalloc(&d_key, size_t(tables[1]) * 8)); CK(hipMalloc(&d_idx, size_t(n_idx) * 4));
  std::vector<uint32_t> idx(n_idx);
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  const int kLaunches = 50, kRuns = 7;
  // `per_line` records of a 64-byte line (4 aux records, 8 keys); run: that many neighbouring records in neighbouring lanes
  auto fill = [&](unsigned cells, unsigned per_line, unsigned run) {
    const unsigned lines = cells / per_line;
    for (unsigned i = 0; i < n_idx; i += run) {
      const unsigned line = rnd() % lines, at = run >= per_line ? 0u : (rnd() % (per_line / run)) * run;
      for (unsigned u = 0; u < run && i + u < n_idx; ++u) idx[i + u] = line * per_line + at + u;  // < lines * per_line <= cells
    }
    CK(hipMemcpy(d_idx, idx.data(), size_t(n_idx) * 4, hipMemcpyHostToDevice));
  };
  auto measure = [&](const char* shape, unsigned cells, unsigned rpb, unsigned run, int which, unsigned words) {
    CK(hipMemset(d_aux, 0, size_t(tables[1]) * 16)); CK(hipMemset(d_key, 0xff, size_t(tables[1]) * 8));
    std::vector<float> us;
    uint32_t salt = 1;
    for (int r = 0; r < kRuns + 1; ++r) {  // (the first run warms up and is dropped)
      CK(hipEventRecord(e0));
      for (int l = 0; l < kLaunches; ++l, ++salt) {
        if (which == 0) hipLaunchKernelGGL(k_rec3, dim3(kBlocks), dim3(kThreads), 0, 0, d_aux, d_idx, rpb, salt);
        if (which == 1) hipLaunchKernelGGL(k_rec1x4, dim3(kBlocks), dim3(kThreads), 0, 0, d_aux, d_idx, rpb, words, salt);
        if (which == 2) hipLaunchKernelGGL(k_key, dim3(kBlocks), dim3(kThreads), 0, 0, d_key, d_idx, rpb, salt);
      }
      CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
      float ms; CK(hipEventElapsedTime(&ms, e0, e1));
      if (r) us.push_back(ms * 1e3f / kLaunches);
    }
    std::sort(us.begin(), us.end());
    const double recs = double(kBlocks) * rpb, med = us[us.size() / 2];
    printf("{\"shape\": \"%s\", \"table\": %u, \"rec_per_block\": %u, \"run\": %u, \"us_per_launch\": [%.2f, %.2f, %.2f], "
           "\"Grec_per_s\": [%.2f, %.2f, %.2f], \"spread_pct\": %.1f}\n",
           shape, cells, rpb, run, us.front(), med, us.back(), recs / us.back() * 1e-3, recs / med * 1e-3,
           recs / us.front() * 1e-3, (us.back() - us.front()) / us.front() * 100.0);
    fflush(stdout);
  };
  {  // the launch alone (rpb = 0: no record), to take off the figures above by hand
    fill(tables[0], 4, 1);
    measure("empty_launch", tables[0], 0, 1, 0, 0);
  }
  for (unsigned cells : tables)
    for (unsigned rpb : rpbs) {
      srand(1);
      fill(cells, 4, 1);
      measure("a_3instr_1lane", cells, rpb, 1, 0, 0);
      measure("b_1instr_4lanes_3active", cells, rpb, 1, 1, 3);
      measure("b_1instr_4lanes_4active", cells, rpb, 1, 1, 4);
      for (unsigned run : {2u, 4u}) {
        fill(cells, 4, run);
        measure("c_1instr_4lanes_3active_runs", cells, rpb, run, 1, 3);
        measure("c_1instr_4lanes_4active_runs", cells, rpb, run, 1, 4);
        measure("a_3instr_1lane_runs", cells, rpb, run, 0, 0);
      }
      fill(cells, 8, 1);
      measure("d_key64_1lane", cells, rpb, 1, 2, 0);
      for (unsigned run : {2u, 4u, 8u}) {
        fill(cells, 8, run);
        measure("d_key64_1lane_runs", cells, rpb, run, 2, 0);
      }
    }
  return 0;
}
