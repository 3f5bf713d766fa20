// fdm_register.hpp — the per-iteration hot path of cloud registration (ICP, point-to-plane ICP, GICP), on the device.
// gfx950 only.
//
// Reference being reproduced: nanoPCL registration::alignICP / alignPlaneICP / alignGICP (registration/align.hpp:71-246)
// — per source point p = T * source[i] in double, the nearest target point of p rounded to float within
// max_correspondence_dist (correspondence/kdtree_correspondence.hpp:57-120), one factor in double
// (factors/icp_factor.hpp:35-119, plane_factor.hpp:40-106, gicp_factor.hpp:30-65, 94-204, robust_kernels.hpp:42-74), and
// the sum of the factors' 21 + 6 + 1 numbers and of the inlier count (linearizers/linearizer.hpp:120-146).  The loop
// around it and the 6 x 6 algebra are the host's (fdm_register_host.hpp).
//
//   k_reg_regularize   once per call and cloud (GICP): C_reg = I - (1 - eps) v0 v0T per point, v0 the unit eigenvector
//                      of the covariance's smallest eigenvalue, by cyclic Jacobi sweeps in double over the lower
//                      triangle (what Eigen's SelfAdjointEigenSolver reads); six doubles per point
//   k_reg_linearize    one lane per source point: transform, search, factor; then the block's sum — wavefront shuffles,
//                      LDS across the four wavefronts in wavefront order — one partial of 29 doubles per block
//   k_reg_reduce       the partials in block order: eight contiguous runs of blocks summed side by side, then the eight
//                      in order
// The sums have a fixed shape for a given n: no floating-point atomics, two calls return the same bits.
// The pieces a sibling kernel needs are device functions of their own — reg_regularize_one, reg_transform, the factors,
// reg_block_sum — and voxelized GICP (fdm_vgicp.hpp: k_vg_linearize, the voxel map's C_reg) is built from them.
//
// The search is fdm_knn.hpp's walk over the TARGET's column grid, built once per call (the target does not move), with a
// top-1 that keeps (d2 bits, target input index) as one 64-bit key — the lower index wins among equal distances, this
// project's definition — and the walk's radius exit.  There is no brute-force queue: the host sets the ring limit to the
// rings that cover the radius, capped by the grid, so every lane leaves by the stopping bound, the radius exit or the
// whole-grid exit.  Every loop bound is known on the host before launch.
#pragma once

#include "fdm_normals.hpp"

namespace fdm {

constexpr int kRegThreads = 256;
constexpr int kRegSums = 29;         // 21 H, 6 b, the error, the inlier count (as a double: exact below 2^53)
constexpr int kRegStride = 32;       // doubles per partial
constexpr int kRegSlices = 8;        // k_reg_reduce: runs of blocks summed side by side
enum : int { kRegICP = 0, kRegPlane = 1, kRegGICP = 2, kRegVGICP = 3 };  // (the fourth: fdm_vgicp.hpp, no public number)
enum : int { kRegNone = 0, kRegHuber = 1, kRegTukey = 2, kRegCauchy = 3 };

struct RegTransform {  // rotation row-major, translation
  double r[9], t[3];
};
struct RegTarget {
  const float4* pts;      // the grid's points in column order (w = input index)
  const uint32_t* start;  // column starts
  KnnGrid G;
  int rings;              // ring limit
  float max_d2;           // max_correspondence_dist squared, in float
  unsigned n;
  const float *x, *y, *z;     // the target in input order
  const float *nx, *ny, *nz;  // plane ICP
  const double* creg;         // GICP: six doubles per point (xx, xy, xz, yy, yz, zz)
};

// the top-1 of the walk: NrmTop<1> without the array
struct RegTop {
  unsigned long long best;
  __device__ __forceinline__ void init() { best = kNrmEmpty; }
  __device__ __forceinline__ float kth() const { return __uint_as_float(uint32_t(best >> 32)); }  // NaN while empty
  __device__ __forceinline__ void offer(float d2, float w) {
    const unsigned long long key = nrm_key(d2, w);
    best = key < best ? key : best;
  }
};

// computeRobustWeight (robust_kernels.hpp:42-74)
__device__ __forceinline__ double reg_weight(double residual, int kernel, double k) {
  const double r = fabs(residual);
  if (kernel == kRegHuber) return r <= k ? 1.0 : k / r;
  if (kernel == kRegTukey) {
    if (r > k) return 0.0;
    const double x = r / k, t = 1.0 - x * x;
    return t * t;
  }
  if (kernel == kRegCauchy) {
    const double x = r / k;
    return 1.0 / (1.0 + x * x);
  }
  return 1.0;
}

// ---- the GICP covariances ----
// Cyclic Jacobi on a symmetric 3 x 3 in double: A -> diagonal, V's columns the eigenvectors.  A rotation is skipped
// where the off-diagonal entry is exactly zero, so a diagonal input leaves V = I.  Six sweeps: convergence is quadratic,
// three reach double precision on these inputs.
__device__ __forceinline__ void reg_jacobi3(double A[3][3], double V[3][3]) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) V[r][c] = r == c ? 1.0 : 0.0;
#pragma unroll 1
  for (int sweep = 0; sweep < 6; ++sweep) {
#pragma unroll
    for (int pq = 0; pq < 3; ++pq) {
      const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
      const double apq = A[p][q];
      if (apq != 0.0) {
        const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        A[p][p] -= t * apq;
        A[q][q] += t * apq;
        A[p][q] = A[q][p] = 0.0;
        const int r = 3 - p - q;  // the third index
        const double arp = A[r][p], arq = A[r][q];
        A[r][p] = A[p][r] = c * arp - s * arq;
        A[r][q] = A[q][r] = s * arp + c * arq;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq;
          V[k][q] = s * vkp + c * vkq;
        }
      }
    }
  }
}

// precomputeRegularizedCovariances (gicp_factor.hpp:215-235): cov(0, 0) not finite -> eps I; otherwise
// V diag(eps, 1, 1) VT = I - (1 - eps) v0 v0T.  Among equal smallest eigenvalues the lowest index is taken, which gives
// diag(eps, 1, 1) for the identity (an invalid point of fdm_cloud_estimate_normals); any other coincidence is
// unspecified (the reference's depends on Eigen's iteration).
// (one covariance: c = 9 floats column-major, (r, c) at c * 3 + r, the lower triangle is r >= c; o = six doubles.  Also
// the voxel distribution map's, fdm_vgicp.hpp)
__device__ __forceinline__ void reg_regularize_one(const float* c, double eps, double* o) {
  const float c00 = c[0];
  if (!(fabsf(c00) <= kFltMax)) {
    o[0] = eps; o[1] = 0.0; o[2] = 0.0; o[3] = eps; o[4] = 0.0; o[5] = eps;
    return;
  }
  double A[3][3], V[3][3];
  A[0][0] = double(c00);
  A[1][0] = A[0][1] = double(c[1]);
  A[2][0] = A[0][2] = double(c[2]);
  A[1][1] = double(c[4]);
  A[2][1] = A[1][2] = double(c[5]);
  A[2][2] = double(c[8]);
  reg_jacobi3(A, V);
  int m = 0;
  if (A[1][1] < A[0][0]) m = 1;
  if (A[2][2] < (m == 1 ? A[1][1] : A[0][0])) m = 2;
  double v[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) v[k] = m == 0 ? V[k][0] : (m == 1 ? V[k][1] : V[k][2]);
  const double f = 1.0 - eps;
  o[0] = 1.0 - f * (v[0] * v[0]);
  o[1] = 0.0 - f * (v[0] * v[1]);
  o[2] = 0.0 - f * (v[0] * v[2]);
  o[3] = 1.0 - f * (v[1] * v[1]);
  o[4] = 0.0 - f * (v[1] * v[2]);
  o[5] = 1.0 - f * (v[2] * v[2]);
}
inline __global__ __launch_bounds__(256) void k_reg_regularize(unsigned n, const float* __restrict__ cov9, double eps,
                                                               double* __restrict__ creg) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  reg_regularize_one(cov9 + size_t(i) * 9, eps, creg + size_t(i) * 6);
}

// ---- the factors: each adds one correspondence's 28 numbers to S[0 .. 27] (H row-major upper triangle, b, error) ----
__device__ __forceinline__ void reg_factor_icp(double tx, double ty, double tz, double qx, double qy, double qz,
                                               double* S) {
  const double rx = tx - qx, ry = ty - qy, rz = tz - qz;
  S[0] = 1.0; S[1] = 0.0; S[2] = 0.0; S[3] = -tz; S[4] = ty; S[5] = 0.0;
  S[6] = 1.0; S[7] = 0.0; S[8] = tz; S[9] = 0.0; S[10] = -tx;
  S[11] = 1.0; S[12] = -ty; S[13] = tx; S[14] = 0.0;
  S[15] = ty * ty + tz * tz; S[16] = -tx * ty; S[17] = -tx * tz;
  S[18] = tx * tx + tz * tz; S[19] = -ty * tz;
  S[20] = tx * tx + ty * ty;
  S[21] = rx; S[22] = ry; S[23] = rz;
  S[24] = ty * rz - tz * ry; S[25] = tz * rx - tx * rz; S[26] = tx * ry - ty * rx;
  S[27] = 0.5 * (rx * rx + ry * ry + rz * rz);
}

__device__ __forceinline__ void reg_factor_plane(double tx, double ty, double tz, double qx, double qy, double qz,
                                                 double nx, double ny, double nz, int kernel, double width, double* S) {
  const double r = nx * (tx - qx) + ny * (ty - qy) + nz * (tz - qz);
  const double w = reg_weight(fabs(r), kernel, width);
  const double j3 = ty * nz - tz * ny, j4 = tz * nx - tx * nz, j5 = tx * ny - ty * nx;
  S[0] = w * nx * nx; S[1] = w * nx * ny; S[2] = w * nx * nz; S[3] = w * nx * j3; S[4] = w * nx * j4; S[5] = w * nx * j5;
  S[6] = w * ny * ny; S[7] = w * ny * nz; S[8] = w * ny * j3; S[9] = w * ny * j4; S[10] = w * ny * j5;
  S[11] = w * nz * nz; S[12] = w * nz * j3; S[13] = w * nz * j4; S[14] = w * nz * j5;
  S[15] = w * j3 * j3; S[16] = w * j3 * j4; S[17] = w * j3 * j5;
  S[18] = w * j4 * j4; S[19] = w * j4 * j5;
  S[20] = w * j5 * j5;
  S[21] = w * r * nx; S[22] = w * r * ny; S[23] = w * r * nz;
  S[24] = w * r * j3; S[25] = w * r * j4; S[26] = w * r * j5;
  S[27] = 0.5 * w * r * r;
}

// Cs: the source's regularized covariance (six doubles), rotated here R Cs RT — (R Cs) first, every three-term sum
// (a0 b0 + a1 b1) + a2 b2; Ct: the target's
__device__ __forceinline__ void reg_factor_gicp(double tx, double ty, double tz, double qx, double qy, double qz,
                                                const double* R, const double* Cs, const double* Ct, int kernel,
                                                double width, double* S) {
  const double cs[3][3] = {{Cs[0], Cs[1], Cs[2]}, {Cs[1], Cs[3], Cs[4]}, {Cs[2], Cs[4], Cs[5]}};
  double RC[3][3], M[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) RC[r][c] = (R[r * 3] * cs[0][c] + R[r * 3 + 1] * cs[1][c]) + R[r * 3 + 2] * cs[2][c];
  const double ct[3][3] = {{Ct[0], Ct[1], Ct[2]}, {Ct[1], Ct[3], Ct[4]}, {Ct[2], Ct[4], Ct[5]}};
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      M[r][c] = ((RC[r][0] * R[c * 3] + RC[r][1] * R[c * 3 + 1]) + RC[r][2] * R[c * 3 + 2]) + ct[r][c];
  // inverse3x3 (gicp_factor.hpp:30-49)
  const double det = M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
                     M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
  const double inv_det = 1.0 / det;
  double w00 = (M[1][1] * M[2][2] - M[1][2] * M[2][1]) * inv_det;
  double w01 = (M[0][2] * M[2][1] - M[0][1] * M[2][2]) * inv_det;
  double w02 = (M[0][1] * M[1][2] - M[0][2] * M[1][1]) * inv_det;
  double w11 = (M[0][0] * M[2][2] - M[0][2] * M[2][0]) * inv_det;
  double w12 = (M[0][2] * M[1][0] - M[0][0] * M[1][2]) * inv_det;
  double w22 = (M[0][0] * M[1][1] - M[0][1] * M[1][0]) * inv_det;
  const double rx = tx - qx, ry = ty - qy, rz = tz - qz;
  double wr0 = w00 * rx + w01 * ry + w02 * rz;
  double wr1 = w01 * rx + w11 * ry + w12 * rz;
  double wr2 = w02 * rx + w12 * ry + w22 * rz;
  const double mahal_sq = rx * wr0 + ry * wr1 + rz * wr2;
  const double rw = reg_weight(sqrt(fmax(mahal_sq, 0.0)), kernel, width);
  w00 *= rw; w01 *= rw; w02 *= rw; w11 *= rw; w12 *= rw; w22 *= rw;
  wr0 *= rw; wr1 *= rw; wr2 *= rw;
  const double h03 = -w01 * tz + w02 * ty, h04 = w00 * tz - w02 * tx, h05 = -w00 * ty + w01 * tx;
  const double h13 = -w11 * tz + w12 * ty, h14 = w01 * tz - w12 * tx, h15 = -w01 * ty + w11 * tx;
  const double h23 = -w12 * tz + w22 * ty, h24 = w02 * tz - w22 * tx, h25 = -w02 * ty + w12 * tx;
  S[0] = w00; S[1] = w01; S[2] = w02; S[3] = h03; S[4] = h04; S[5] = h05;
  S[6] = w11; S[7] = w12; S[8] = h13; S[9] = h14; S[10] = h15;
  S[11] = w22; S[12] = h23; S[13] = h24; S[14] = h25;
  S[15] = -(tz * h13 - ty * h23); S[16] = -(tz * h14 - ty * h24); S[17] = -(tz * h15 - ty * h25);
  S[18] = -(-tz * h04 + tx * h24); S[19] = -(-tz * h05 + tx * h25);
  S[20] = -(ty * h05 - tx * h15);
  S[21] = wr0; S[22] = wr1; S[23] = wr2;
  S[24] = ty * wr2 - tz * wr1; S[25] = tz * wr0 - tx * wr2; S[26] = tx * wr1 - ty * wr0;
  S[27] = 0.5 * rw * mahal_sq;
}

// p = T * (x, y, z): ((r0 x + r1 y) + r2 z) + t per row in double, no contraction (ASSUMED order: DESIGN.md §6)
__device__ __forceinline__ void reg_transform(const RegTransform& T, double x, double y, double z, double& px, double& py,
                                              double& pz) {
  px = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(T.r[0], x), __dmul_rn(T.r[1], y)), __dmul_rn(T.r[2], z)), T.t[0]);
  py = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(T.r[3], x), __dmul_rn(T.r[4], y)), __dmul_rn(T.r[5], z)), T.t[1]);
  pz = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(T.r[6], x), __dmul_rn(T.r[7], y)), __dmul_rn(T.r[8], z)), T.t[2]);
}

// The block's sum of every lane's S[0 .. 28] into partial[blockIdx.x]: the wavefront's by a butterfly, the same tree in
// every lane; then LDS across the four wavefronts in wavefront order.  Every thread of the block calls it.
__device__ __forceinline__ void reg_block_sum(double* S, double* __restrict__ partial) {
  __shared__ double s_sum[kRegThreads / 64][kRegStride];
#pragma unroll
  for (int a = 0; a < kRegSums; ++a) {
    double v = S[a];
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
    S[a] = v;
  }
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (lane == 0u) {
#pragma unroll
    for (int a = 0; a < kRegSums; ++a) s_sum[wave][a] = S[a];
  }
  __syncthreads();
  if (threadIdx.x < unsigned(kRegSums)) {
    double v = s_sum[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kRegThreads / 64; ++w) v += s_sum[w][threadIdx.x];
    partial[size_t(blockIdx.x) * kRegStride + threadIdx.x] = v;
  }
}

// corr (nullable): corr[i] = the target index source point i corresponds to, -1 for none
template <int FACTOR>
__global__ __launch_bounds__(kRegThreads) void k_reg_linearize(unsigned n, const float* __restrict__ sx,
                                                               const float* __restrict__ sy,
                                                               const float* __restrict__ sz,
                                                               const double* __restrict__ s_creg, const RegTransform T,
                                                               const RegTarget Q, int kernel, double width,
                                                               double* __restrict__ partial, int32_t* __restrict__ corr) {
  const unsigned i = blockIdx.x * unsigned(kRegThreads) + threadIdx.x;
  double S[kRegSums];
#pragma unroll
  for (int a = 0; a < kRegSums; ++a) S[a] = 0.0;
  if (i < n) {
    // p = T * source[i]: ((r0 x + r1 y) + r2 z) + t per row in double (ASSUMED order: DESIGN.md §6), rounded once to
    // float for the search; the factor takes the double
    double px, py, pz;
    reg_transform(T, double(sx[i]), double(sy[i]), double(sz[i]), px, py, pz);
    const float4 q = make_float4(float(px), float(py), float(pz), 0.0f);
    RegTop top;
    top.init();
    (void)knn_walk<true, RegTop, true>(0u, q, Q.pts, Q.start, Q.G, top, Q.rings, Q.max_d2);
    const bool hit = top.best != kNrmEmpty && top.kth() <= Q.max_d2;
    if (hit) {
      const uint32_t j = min(uint32_t(top.best), Q.n - 1u);  // (an input index of the target: the clamp costs nothing)
      const double qx = double(Q.x[j]), qy = double(Q.y[j]), qz = double(Q.z[j]);
      if (FACTOR == kRegICP) {
        reg_factor_icp(px, py, pz, qx, qy, qz, S);
      } else if (FACTOR == kRegPlane) {
        reg_factor_plane(px, py, pz, qx, qy, qz, double(Q.nx[j]), double(Q.ny[j]), double(Q.nz[j]), kernel, width, S);
      } else {
        double Cs[6], Ct[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) {
          Cs[a] = s_creg[size_t(i) * 6 + size_t(a)];
          Ct[a] = Q.creg[size_t(j) * 6 + size_t(a)];
        }
        reg_factor_gicp(px, py, pz, qx, qy, qz, T.r, Cs, Ct, kernel, width, S);
      }
      S[28] = 1.0;
      if (corr) corr[i] = int32_t(j);
    } else if (corr) {
      corr[i] = -1;
    }
  }
  reg_block_sum(S, partial);
}

// out[0 .. 28] = the nb partials summed: slice s takes blocks [s * per, min(nb, (s + 1) * per)) in order, the slices
// are then added in order
inline __global__ __launch_bounds__(kRegSlices * kRegStride) void k_reg_reduce(unsigned nb,
                                                                              const double* __restrict__ partial,
                                                                              double* __restrict__ out) {
  __shared__ double s_sum[kRegSlices][kRegStride];
  const unsigned v = threadIdx.x & unsigned(kRegStride - 1), slice = threadIdx.x / unsigned(kRegStride);
  const unsigned per = (nb + unsigned(kRegSlices) - 1u) / unsigned(kRegSlices);
  const unsigned b0 = min(nb, slice * per), b1 = min(nb, b0 + per);
  double acc = 0.0;
  if (v < unsigned(kRegSums)) {
#pragma unroll 4
    for (unsigned b = b0; b < b1; ++b) acc += partial[size_t(b) * kRegStride + v];
  }
  s_sum[slice][v] = acc;
  __syncthreads();
  if (threadIdx.x < unsigned(kRegSums)) {
    double t = s_sum[0][threadIdx.x];
#pragma unroll
    for (int s = 1; s < kRegSlices; ++s) t += s_sum[s][threadIdx.x];
    out[threadIdx.x] = t;
  }
}

}  // namespace fdm
