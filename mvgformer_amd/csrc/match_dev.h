// Shared by the ground-truth matchers of the training step (criterion.hip: KNN / multiple; hungarian.hip: the one-to-one
// assignment): the launch-argument records, the fp32 norm round trip of the ground truth and the pose cost
// cost[g][q] = 0.01 * sum_{3J} |pose[q] - gt'[g]| (torch.cdist(p=1), matcher.py:165-169).  One device function computes the
// costs for every matcher, so that all of them select on the same fp32 values.
#pragma once
#include <math.h>

#include "common.h"

#define MATCH_THREADS 256

struct SpaceBox {
  float size[3], center[3];
};
struct JointMap {
  uint8_t m[64];               // m[j] = prediction joint of converted joint j, j < Jc
};

// absolute -> norm -> absolute in fp32 in the order of matcher.py:65-78: n = ((x - center) + size / 2) / size, then
// fma(n, size, center) - size / 2.  The product n * size and the addition of center are ONE fused operation: the library is
// built with -ffp-contract=fast, under which the compiler has always fused them in mvg_knn_match (the _rn intrinsics are plain
// operators to it); it is written out here so that every matcher, every build and the tests' restatement state the same value.
// size / 2 is exact, so fusing its two additions changes nothing.  The result differs from the reference's unfused fp32 by at
// most one rounding of n * size.
__device__ __forceinline__ float norm_round_trip_f32(float x, float size, float center) {
  const float half = __fdiv_rn(size, 2.0f);
  const float n = __fdiv_rn(__fadd_rn(__fsub_rn(x, center), half), size);
  return __fsub_rn(fmaf(n, size, center), half);
}

__device__ __forceinline__ long load_count(const void* p, int is64, int i) {
  return is64 ? (long)((const int64_t*)p)[i] : (long)((const int32_t*)p)[i];
}

// cost[g * NQ + q] for g < G, q < NQ, by a workgroup of MATCH_THREADS threads in uniform control flow; query q is computed,
// and its cost written, by thread q % MATCH_THREADS.  pb: the NQ queries of this problem (J joints each, Jp when MAPPED: joint
// j of the ground truth is read at float offset s_map3[j] of the query); gb: the Gmax persons of its batch element, J joints
// each.  gt_lds: 64 * 3 floats of LDS, the round-tripped ground truth of one person at a time (3J <= 192 floats): G * 3J
// round trips, not NQ * G * 3J.  s_map3 must be visible to the workgroup no later than the first barrier in here.  The caller
// puts a barrier between this call and reads of `cost` by other threads.
template <bool MAPPED>
__device__ __forceinline__ void match_pose_costs(const float* __restrict__ pb, const float* __restrict__ gb, const SpaceBox& box,
                                                 int NQ, int G, int J, int Jp, const int* s_map3, float* gt_lds, float* cost) {
  const int tid = threadIdx.x;
  for (int g = 0; g < G; ++g) {
    __syncthreads();
    for (int e = tid; e < J * 3; e += MATCH_THREADS)
      gt_lds[e] = norm_round_trip_f32(gb[(long)g * J * 3 + e], box.size[e % 3], box.center[e % 3]);
    __syncthreads();
    for (int q = tid; q < NQ; q += MATCH_THREADS) {
      const float* x = pb + (long)q * (MAPPED ? Jp : J) * 3;
      float s = 0.f;
      if (MAPPED) {
        for (int j = 0; j < J; ++j) {
          const float* xj = x + s_map3[j];
          for (int c = 0; c < 3; ++c) s += fabsf(xj[c] - gt_lds[j * 3 + c]);
        }
      } else {
        for (int e = 0; e < J * 3; ++e) s += fabsf(x[e] - gt_lds[e]);
      }
      s *= 0.01f;
      cost[(long)g * NQ + q] = (s < INFINITY) ? s : INFINITY;    // NaN / inf poses sort last
    }
  }
}

// joint_map (Jc HOST ints, distinct, inside [0, Jp)) -> the by-value table; NULL = the identity, Jc == Jp.  0 on a bad map.
static inline int pack_joint_map(int Jp, int Jc, const int* joint_map, JointMap* out) {
  if (Jp < 1 || Jp > 64 || Jc < 1 || Jc > 64) return 0;
  for (int j = 0; j < 64; ++j) out->m[j] = 0;
  if (!joint_map) return Jc == Jp;
  bool seen[64] = {};
  for (int j = 0; j < Jc; ++j) {
    const int m = joint_map[j];
    if (m < 0 || m >= Jp || seen[m]) return 0;
    seen[m] = true;
    out->m[j] = (uint8_t)m;
  }
  return 1;
}
