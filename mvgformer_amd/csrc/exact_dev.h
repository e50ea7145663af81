// Device helpers shared by the kernels whose results are compared bit for bit with a host restatement: nms.hip, evalacc.hip,
// track.hip, structural.hip, hungarian.hip (fp64 from fp32 inputs) and criterion.hip, optim.hip, operands.hip (the fixed-order
// workgroup sum, the 16-byte test).
//
// CONTRACTION.  The library is built with -ffp-contract=fast (csrc/Makefile).  Under that flag the back end fuses an fp64
// multiply into the add behind it (v_fma_f64 / v_fmac_f64) wherever it finds one, and a `#pragma clang fp contract(off)` in the
// source does not stop it: the device code of every file listed above is the same with and without that pragma, so none of
// them carries one.  A product is rounded on its own only when it goes through f64_mul / f64_mul_nv below, or does not feed an
// add.  Consequently:
//   * exact, whatever the inputs: dist3_exact (track_eval_kernel), everything in structural.hip, hungarian.hip and the motion
//     model of track.hip (track_predict_kernel, track_correct_kernel), whose products all go through f64_mul / f64_mul_nv;
//   * fused: dist3 and norm3, that is the distances of nms_rank_kernel, nms_close_kernel, eval_match_kernel, eval_pcp_kernel and
//     track_update_kernel.  sqrt((dx*dx + dy*dy) + dz*dz) is computed as sqrt(fma(dz, dz, fma(dy, dy, dx*dx))): dy*dy and dz*dz
//     are not rounded.  That is the documented rounding (every product and sum rounded on its own) whenever those squares are
//     exact in fp64, that is, while a coordinate difference has at most 26 significant bits.  Differences of fp32 values of
//     similar magnitude do (poses in millimetres, the inputs of the tests); not every pair of fp32 values does.
// Which kernel uses which form is part of its results; changing one is a behaviour change.
#pragma once
#include "common.h"

typedef long long i64;
typedef unsigned long long u64;

// a * b rounded on its own: the empty asm statement on the result is a value the compiler cannot fuse across
static __device__ __forceinline__ double f64_mul(double a, double b) {
  double p = a * b;
  asm volatile("" : "+v"(p));
  return p;
}
// The same without `volatile`, for the long product chains of structural.hip: the loads and products of a chain may still be
// scheduled ahead of its adds.  Same values as f64_mul, another instruction order: a kernel keeps the form it was written with.
static __device__ __forceinline__ double f64_mul_nv(double a, double b) {
  double p = a * b;
  asm("" : "+v"(p));
  return p;
}

// the value lane `from` holds; `from` is wave-uniform (v_readlane, a double as two halves)
static __device__ __forceinline__ int lane_of(int v, int from) {
  return __builtin_amdgcn_readlane(v, __builtin_amdgcn_readfirstlane(from));
}
static __device__ __forceinline__ double lane_of(double v, int from) {
  const int l = __builtin_amdgcn_readfirstlane(from);
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

// sqrt((x^2 + y^2) + z^2), correctly rounded sqrt.  norm3 and dist3 are FUSED (see CONTRACTION above): equal to the rounding of
// every operation on its own while y^2 and z^2 are exact in fp64, i.e. while y and z have at most 26 significant bits.
static __device__ __forceinline__ double norm3(double x, double y, double z) { return __builtin_sqrt((x * x + y * y) + z * z); }
static __device__ __forceinline__ double dist3(const float* p, const float* g) {
  return norm3((double)p[0] - (double)g[0], (double)p[1] - (double)g[1], (double)p[2] - (double)g[2]);
}
// every product rounded on its own, for all inputs
static __device__ __forceinline__ double dist3_exact(const float* p, const float* g) {
  const double dx = (double)p[0] - (double)g[0], dy = (double)p[1] - (double)g[1], dz = (double)p[2] - (double)g[2];
  return __builtin_sqrt((f64_mul(dx, dx) + f64_mul(dy, dy)) + f64_mul(dz, dz));
}

// a count read from device memory, brought into [0, hi]
static __device__ __forceinline__ int clamp_count(int v, int hi) { return min(max(v, 0), hi); }
static __device__ __forceinline__ int clamp_count(long v, int hi) { return (int)(v < 0 ? 0 : (v > hi ? hi : v)); }

// The rows of element b of dets (B, R, J, 5) that take part: the first count[2 * b] of them (all R without a count) whose
// flag dets[b, i, 0, 3] is >= 0.
static __device__ __forceinline__ int det_rows(const int* count, int b, int R) {
  return count == nullptr ? R : clamp_count(count[2 * b], R);
}
static __device__ __forceinline__ bool det_flag(const float* dets, int b, int i, int R, int J) {
  return dets[((size_t)b * R + i) * J * 5 + 3] >= 0.f;
}

// Ordered compaction of R rows by a workgroup of SCAN_THREADS threads, for N counts at once (N = 1 or 2).  Thread t owns the
// run [lo, hi) of consecutive rows; tally(i, n) adds row i to the counts n[0 .. N - 1] it belongs to.  The run totals go through
// a ping-pong LDS scan; before(k) is the rows of count k in front of the thread's run, total(k) those of the whole element.  The
// caller walks its run again with the same per-row test to place the rows.  Every thread of the workgroup calls this (it has
// barriers).  before() and total() read s_scan: a caller that reuses the array puts a barrier behind its last call of them.
#define SCAN_THREADS 256                             // of the kernels that call scan_rows; no other kernel depends on it
template <int N>
struct RowScan {
  int lo, hi, mine[N];
  const int (*sums)[SCAN_THREADS];                   // the inclusive scan of the run totals, in LDS
  __device__ __forceinline__ int before(int k) const { return sums[k][threadIdx.x] - mine[k]; }
  __device__ __forceinline__ int total(int k) const { return sums[k][SCAN_THREADS - 1]; }
};
template <int N, class Tally>
static __device__ __forceinline__ RowScan<N> scan_rows(int R, int (*s_scan)[N][SCAN_THREADS], Tally tally) {
  const int t = threadIdx.x;
  RowScan<N> r;
  const int chunk = (R + SCAN_THREADS - 1) / SCAN_THREADS;
  r.lo = min(t * chunk, R);
  r.hi = min(r.lo + chunk, R);
#pragma unroll
  for (int k = 0; k < N; ++k) r.mine[k] = 0;
  for (int i = r.lo; i < r.hi; ++i) tally(i, r.mine);
#pragma unroll
  for (int k = 0; k < N; ++k) s_scan[0][k][t] = r.mine[k];
  __syncthreads();
  int src = 0;
  for (int step = 1; step < SCAN_THREADS; step <<= 1) {
#pragma unroll
    for (int k = 0; k < N; ++k) s_scan[src ^ 1][k][t] = s_scan[src][k][t] + (t >= step ? s_scan[src][k][t - step] : 0);
    src ^= 1;
    __syncthreads();
  }
  r.sums = s_scan[src];
  return r;
}

// fixed-order sum over a workgroup of WAVES wavefronts (lanes: butterfly; wavefronts: in order); valid in thread 0
template <int WAVES>
static __device__ __forceinline__ double block_sum(double v, double* scratch) {
#pragma unroll
  for (int d = 1; d < MVG_WAVE; d <<= 1) v += __shfl_xor(v, d, MVG_WAVE);
  __syncthreads();
  if ((threadIdx.x & (MVG_WAVE - 1)) == 0) scratch[threadIdx.x / MVG_WAVE] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < WAVES; ++w) s += scratch[w];
  return s;
}

static __device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
