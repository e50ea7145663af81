// One-to-one ground-truth matcher of the training step for gfx950 (lib/models/matcher.py:80-199, methods 'hungarian' and
// 'hungarian-dis'): the reference computes the cost on the device, moves it with .cpu() and runs scipy's linear_sum_assignment per
// batch element; here the P = Lm * B problems of a step are solved in ONE launch, one workgroup per problem, nothing read back.
//
//   mvg_hungarian_match   1 launch, 256 lanes per problem.  Rows are the G <= 64 persons, columns the NQ <= 4096 queries; column q
//                         lives on lane q % 256, slot q / 256: its potential v, its minv and its class term stay in registers
//                         (NS = 4 slots up to 1024 queries, 16 beyond), its used flag is a bit of a per-lane mask.  The fp32 pose
//                         costs of match_dev.h (the values mvg_knn_match selects on) lie in LDS while G x NQ of them fit 40 KB
//                         -- the training shape is 10 x 1024 -- and in the caller's workspace beyond; C[g][q] is recombined from
//                         the pose cost and the column's class term on every read, in fp64, the same operations every time.
//                         Row potentials u, the row of every column and the way[] links live in LDS.
//
// The solver is the algorithm written down for mvg_linear_assignment (include/mvg_decoder.h), stated for the rectangular problem:
// shortest augmenting paths with potentials from 0, rows inserted in order, no padding.  One step of a search: the lanes relax
// their unused columns, take the (value, column) minimum of their slots, the wavefront reduces it with shuffles, the four
// wavefronts meet in LDS (one barrier per step, the exchange buffers alternate), and every lane applies delta to its columns.
// The minimum is taken under a total order (value, NaN as +inf, then column), so the shape of the reduction does not matter.
// u[r] has one writer per step: the lane of the used column whose row is r, thread 0 for the row being inserted.  The path is
// flipped by thread 0 in LDS.  Every loop is counted (a search of row i takes at most i + 1 steps): no input can make it spin.
//
// Arithmetic: fp64, every operation rounded on its own: a product that feeds an add goes through f64_mul (CONTRACTION in
// exact_dev.h).  No floating-point atomics, no atomics at all: two runs give the same bits.
#include <math.h>

#include "exact_dev.h"
#include "match_dev.h"

#define HG_THREADS MATCH_THREADS
#define HG_WAVES (HG_THREADS / MVG_WAVE)
#define HG_LDS_COSTS 10240            // Gmax x NQ fp32 pose costs kept in LDS (40 KB); the caller's workspace beyond
#define HG_NONE 0x7fffffff

static_assert(MVG_HUNGARIAN_MAX_NQ == 16 * HG_THREADS, "16 column slots per lane");
static_assert(MVG_HUNGARIAN_MAX_G == 64, "rows fit a signed byte and one wavefront writes the pairs");

struct HgArgs {
  const float* logits;        // (P, NQ, 2) or null
  const float* poses;         // (P, NQ*Jp, 3)
  const float* gt;            // (B, Gmax, J, 3)
  const void* num_person;     // (B,)
  float* cost_ws;             // (P, Gmax, NQ) when the costs do not fit LDS
  int* pair_query;            // (P, Gmax)
  int* pair_gt;               // (P, Gmax)
  int* pair_count;            // (P,)
  uint8_t* matched;           // (P, NQ)
  double* duals;              // (P, Gmax + NQ) or null
  SpaceBox box;
  int np_is64, dis, B, NQ, Gmax, J, Jp;
  double cost_class, cost_pose;
  JointMap map;
};

// (k, q, d) <- the smaller of (k, q) and (ok, oq) in the order (value, then column), with its raw minv d
static __device__ __forceinline__ void hg_take(double& k, int& q, double& d, double ok, int oq, double od) {
  if (ok < k || (ok == k && oq < q)) {
    k = ok;
    q = oq;
    d = od;
  }
}

template <int NS, bool MAPPED>
__global__ __launch_bounds__(HG_THREADS) void hungarian_match_kernel(HgArgs a) {
  __shared__ float cost_lds[HG_LDS_COSTS];
  __shared__ float gt_lds[64 * 3];
  __shared__ int s_map3[MAPPED ? 64 : 1];
  __shared__ double s_u[MVG_HUNGARIAN_MAX_G];                    // row potentials
  __shared__ short s_way[NS * HG_THREADS];                       // column -> the column its minv came from, -1 = virtual
  __shared__ signed char s_p[NS * HG_THREADS];                   // column -> its row, -1 = free
  __shared__ int s_col[MVG_HUNGARIAN_MAX_G];                     // row -> its column (written at the end)
  __shared__ double s_wk[2][HG_WAVES], s_wd[2][HG_WAVES];        // per-wavefront minimum: key, raw minv
  __shared__ int s_wq[2][HG_WAVES];                              //                        column
  const int p = blockIdx.x, b = p % a.B, tid = threadIdx.x, lane = tid & (MVG_WAVE - 1), wave = tid / MVG_WAVE;
  const int NQ = a.NQ, Gmax = a.Gmax, J = a.J;
  if (MAPPED && tid < J) s_map3[tid] = 3 * (int)a.map.m[tid];    // visible after the first barrier of the cost loop
  const int G = clamp_count(load_count(a.num_person, a.np_is64, b), Gmax);
  float* cost = ((long)NQ * Gmax <= HG_LDS_COSTS) ? cost_lds : a.cost_ws + (long)p * NQ * Gmax;
  const float* pb = a.poses + (long)p * NQ * (MAPPED ? a.Jp : J) * 3;
  const float* gb = a.gt + (long)b * Gmax * J * 3;
  const bool dis = a.dis != 0;
  const double INF = (double)INFINITY;

  double v[NS], minv[NS], cw[NS];                                // per column slot: potential, minv, cost_class * class term
  if (tid < MVG_HUNGARIAN_MAX_G) {
    s_u[tid] = 0.0;
    s_col[tid] = -1;
  }
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const int q = k * HG_THREADS + tid;
    v[k] = 0.0;
    minv[k] = INF;
    cw[k] = 0.0;
    if (q < NQ) {
      s_p[q] = -1;
      if (!dis) {                                                // matcher.py:151-162 with every target in class 1
        const double x = a.logits ? (double)a.logits[((long)p * NQ + q) * 2 + 1] : 1.0;
        const double pr = 1.0 / (1.0 + exp(-x));
        const double om = 1.0 - pr;
        const double pos = f64_mul(f64_mul(0.25, f64_mul(om, om)), -log(pr + 1e-8));
        const double neg = f64_mul(f64_mul(0.75, f64_mul(pr, pr)), -log(om + 1e-8));
        cw[k] = f64_mul(a.cost_class, pos - neg);
      }
    }
  }
  match_pose_costs<MAPPED>(pb, gb, a.box, NQ, G, J, a.Jp, s_map3, gt_lds, cost);     // match_dev.h
  __syncthreads();

  for (int i = 0; i < G; ++i) {                                  // insert row i
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const int q = k * HG_THREADS + tid;
      minv[k] = INF;
      if (q < NQ) s_way[q] = -1;
    }
    unsigned used = 0;                                           // bit k: column slot k of this lane is used
    int j0 = -1, i0 = i;                                         // -1: the virtual column, whose row is i
    bool found = false;
    for (int step = 0; step <= i; ++step) {                      // step k uses a k-th column and at most i columns have a row
      if (j0 >= 0 && (j0 & (HG_THREADS - 1)) == tid) used |= 1u << (j0 / HG_THREADS);
      const double ui0 = s_u[i0];
      double bk = INF, bd = INF;
      int bq = HG_NONE;
#pragma unroll
      for (int k = 0; k < NS; ++k) {
        const int q = k * HG_THREADS + tid;
        if (q < NQ && !((used >> k) & 1u)) {
          const double pc = (double)cost[(long)i0 * NQ + q];
          double c = dis ? pc : f64_mul(a.cost_pose, pc) + cw[k];
          if (!(c <= MVG_LAP_BIG)) c = MVG_LAP_BIG;              // NaN or above
          const double cur = (c - ui0) - v[k];
          if (cur < minv[k]) {
            minv[k] = cur;
            s_way[q] = (short)j0;
          }
          hg_take(bk, bq, bd, minv[k] == minv[k] ? minv[k] : INF, q, minv[k]);
        }
      }
#pragma unroll
      for (int d = 1; d < MVG_WAVE; d <<= 1) {
        const double ok = __shfl_xor(bk, d, MVG_WAVE), od = __shfl_xor(bd, d, MVG_WAVE);
        const int oq = __shfl_xor(bq, d, MVG_WAVE);
        hg_take(bk, bq, bd, ok, oq, od);
      }
      const int buf = step & 1;
      if (lane == 0) {
        s_wk[buf][wave] = bk;
        s_wq[buf][wave] = bq;
        s_wd[buf][wave] = bd;
      }
      __syncthreads();
      bk = s_wk[buf][0];
      bq = s_wq[buf][0];
      bd = s_wd[buf][0];
#pragma unroll
      for (int w = 1; w < HG_WAVES; ++w) hg_take(bk, bq, bd, s_wk[buf][w], s_wq[buf][w], s_wd[buf][w]);
      if (bq == HG_NONE) break;                                  // not reachable: NQ >= Gmax leaves an unused column
      const double delta = bd;
#pragma unroll
      for (int k = 0; k < NS; ++k) {
        const int q = k * HG_THREADS + tid;
        if (q < NQ) {
          if ((used >> k) & 1u) {
            v[k] -= delta;
            s_u[s_p[q]] += delta;                                // a used column has a row, and no other column has it
          } else {
            minv[k] -= delta;
          }
        }
      }
      if (tid == 0) s_u[i] += delta;
      j0 = bq;
      const int pj = s_p[j0];
      if (pj < 0) {
        found = true;
        break;
      }
      i0 = pj;
    }
    __syncthreads();
    if (found && tid == 0) {                                     // flip the path back to the virtual column: <= i + 1 links
      int j = j0;
      for (int k = 0; k <= i; ++k) {
        const int jw = s_way[j];
        s_p[j] = (signed char)(jw < 0 ? i : s_p[jw]);
        j = jw;
        if (j < 0) break;
      }
    }
    __syncthreads();
  }

  uint8_t* mb = a.matched + (long)p * NQ;
  double* du = a.duals ? a.duals + (long)p * (Gmax + NQ) : nullptr;
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const int q = k * HG_THREADS + tid;
    if (q < NQ) {
      const int r = s_p[q];
      mb[q] = r >= 0 ? 1 : 0;
      if (r >= 0) s_col[r] = q;
      if (du) du[Gmax + q] = v[k];
    }
  }
  __syncthreads();
  if (tid < Gmax) {                                              // the pairs in ascending query order, -1 behind them
    int* pq = a.pair_query + (long)p * Gmax;
    int* pg = a.pair_gt + (long)p * Gmax;
    if (du) du[tid] = s_u[tid];
    if (tid < G) {
      const int mine = s_col[tid] < 0 ? HG_NONE : s_col[tid];    // a row without a column (not reachable) goes last
      int rank = 0;
      for (int g = 0; g < G; ++g) {
        const int other = s_col[g] < 0 ? HG_NONE : s_col[g];
        rank += (other < mine || (other == mine && g < tid)) ? 1 : 0;
      }
      pq[rank] = s_col[tid];
      pg[rank] = s_col[tid] < 0 ? -1 : tid;
    } else {
      pq[tid] = -1;
      pg[tid] = -1;
    }
  }
  if (tid == 0) a.pair_count[p] = G;
}

extern "C" {

size_t mvg_hungarian_match_workspace(int P, int NQ, int Gmax) {
  if (P < 1 || NQ < 1 || Gmax < 1) return 0;
  return ((long)NQ * Gmax <= HG_LDS_COSTS) ? 0 : (size_t)P * NQ * Gmax * sizeof(float);
}

int mvg_hungarian_match(const float* logits, const float* poses, const float* joints_3d, const void* num_person,
                        int num_person_is64, const float* space_size, const float* space_center, int method, float cost_class,
                        float cost_pose, int P, int B, int NQ, int Gmax, int Jp, int Jc, const int* joint_map, void* workspace,
                        size_t workspace_bytes, int* pair_query, int* pair_gt, int* pair_count, uint8_t* matched, double* duals,
                        void* stream) {
  if (mvg_any_null({poses, joints_3d, num_person, space_size, space_center, pair_query, pair_gt, pair_count, matched}))
    return MVG_E_BADARG;
  if (method != MVG_MATCH_HUNGARIAN && method != MVG_MATCH_HUNGARIAN_DIS) return MVG_E_BADARG;
  HgArgs a;
  if (B < 1 || P < 1 || P % B != 0 || Gmax < 1 || Gmax > MVG_HUNGARIAN_MAX_G || NQ < Gmax || NQ > MVG_HUNGARIAN_MAX_NQ ||
      !pack_joint_map(Jp, Jc, joint_map, &a.map))
    return MVG_E_BADARG;
  if (mvg_any_misaligned(8, {duals})) return MVG_E_BADARG;       // optional
  const size_t need = mvg_hungarian_match_workspace(P, NQ, Gmax);
  if (need && (!workspace || workspace_bytes < need || mvg_any_misaligned(4, {workspace}))) return MVG_E_BADARG;
  a.logits = logits; a.poses = poses; a.gt = joints_3d; a.num_person = num_person;
  a.cost_ws = (float*)workspace;
  a.pair_query = pair_query; a.pair_gt = pair_gt; a.pair_count = pair_count; a.matched = matched; a.duals = duals;
  for (int i = 0; i < 3; ++i) {
    a.box.size[i] = space_size[i];
    a.box.center[i] = space_center[i];
  }
  a.np_is64 = num_person_is64; a.dis = method == MVG_MATCH_HUNGARIAN_DIS; a.B = B; a.NQ = NQ; a.Gmax = Gmax; a.J = Jc; a.Jp = Jp;
  a.cost_class = (double)cost_class; a.cost_pose = (double)cost_pose;
  const bool small = NQ <= 4 * HG_THREADS;
  if (joint_map) {
    if (small) hipLaunchKernelGGL((hungarian_match_kernel<4, true>), dim3(P), dim3(HG_THREADS), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((hungarian_match_kernel<16, true>), dim3(P), dim3(HG_THREADS), 0, (hipStream_t)stream, a);
  } else {
    if (small) hipLaunchKernelGGL((hungarian_match_kernel<4, false>), dim3(P), dim3(HG_THREADS), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((hungarian_match_kernel<16, false>), dim3(P), dim3(HG_THREADS), 0, (hipStream_t)stream, a);
  }
  MVG_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
