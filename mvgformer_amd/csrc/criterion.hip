// Training criterion of the MVGFormer head for gfx950: the device-side ground-truth matcher (lib/models/matcher.py:80-262,
// methods KNN and multiple) and the per-layer losses of SetCriterion (lib/models/multi_view_pose_transformer.py:491-932) for all
// decoder layers of one step, forward value and gradients in the same pass.  No host round trip, no floating-point atomics:
// every sum is taken in a fixed order, two runs on the same inputs give the same bits.
//
//   mvg_knn_match   1 launch : one workgroup per batch element, one wavefront per ground-truth person for the K arg-min rounds
//   mvg_criterion   3 launches: (A) ground truth -> 2D in all views, (B) one workgroup per (layer, batch element): partial sums,
//                               counts and the dense gradients, (C) one workgroup: the (L, 8) table
//   mvg_knn_match_jm / mvg_criterion_jm: the same launches with a joint map between predictions and ground truth (below)
// The losses are tiny (B x NQ x 2 logits, at most B x G x K pairs), so (A)-(C) evaluate them in fp64 from the fp32 inputs; the
// matcher keeps the reference's fp32 arithmetic (the selection must be the one an fp32 cdist gives).
//
// Joint map (Shelf / Campus joint format, dq_transformer.py:90-104, 582-594): the predictions have Jp joints per query, the ground
// truth Jc, and converted joint j is prediction joint map[j].  The map travels by value in the launch arguments (JointMap); every
// loop and divisor below runs over the Jc converted joints, prediction reads and gradient writes go through the map.  The
// kernels are templates on MAPPED: the instantiation without a map (Jp == Jc, identity) is the code as it was before the map.
#include <math.h>

#include "exact_dev.h"
#include "match_dev.h"

#define CRIT_THREADS MATCH_THREADS
#define CRIT_WAVES (CRIT_THREADS / MVG_WAVE)
#define KNN_LDS_COSTS 10240    // NQ x G fp32 costs kept in LDS up to 1024 x 10 (40 KB); a caller workspace beyond
#define CRIT_MAX_NQ 4096       // int16 chains in LDS
#define CRIT_MAX_PAIRS 4096
#define CRIT_MAX_B 256
#define CRIT_PART 8            // doubles per (layer, batch element) partial record

// the same chain for the criterion's targets, in fp64
__device__ __forceinline__ double norm_round_trip_f64(double x, double size, double center) {
  const double n = (x - center + size / 2.0) / size;
  return n * size + center - size / 2.0;
}

// lexicographic (cost, index) minimum over the 64 lanes of a wavefront; every lane gets the result
__device__ __forceinline__ void wave_argmin(float& c, int& q) {
#pragma unroll
  for (int d = 1; d < MVG_WAVE; d <<= 1) {
    const float oc = __shfl_xor(c, d, MVG_WAVE);
    const int oq = __shfl_xor(q, d, MVG_WAVE);
    if (oc < c || (oc == c && oq < q)) {
      c = oc;
      q = oq;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------------------
// matcher.  cost[g][q] = 0.01 * sum_{3J} |pose[q] - gt'[g]| (torch.cdist(p=1), matcher.py:165-169); J = the Jc joints of the
// ground truth, pose joint map[j] against ground-truth joint j when MAPPED (poses then have Jp joints per query).
//   KNN     : the K smallest-cost queries of every person, pair slot g * K + k (person-major, ascending cost, ties to the lower
//             query index); pair_count = G * K.
//   multiple: every query whose nearest person (ties to the lower person index) is closer than `value`, in ascending query order
//             (matcher.py:201-230: torch.where order); pair_count <= NQ.
template <bool MAPPED>
__global__ __launch_bounds__(CRIT_THREADS) void knn_match_kernel(const float* __restrict__ poses, const float* __restrict__ gt,
                                                                 const void* __restrict__ num_person, int np_is64, SpaceBox box,
                                                                 int method, int K, float value, int NQ, int Gmax, int J, int Pmax,
                                                                 float* __restrict__ cost_ws, int* __restrict__ pair_query,
                                                                 int* __restrict__ pair_gt, int* __restrict__ pair_count,
                                                                 uint8_t* __restrict__ matched, int Jp, JointMap map) {
  __shared__ float cost_lds[KNN_LDS_COSTS];
  __shared__ float gt_lds[64 * 3];
  __shared__ int wave_cnt[CRIT_WAVES];
  __shared__ int base_cnt;
  __shared__ int s_map3[MAPPED ? 64 : 1];                        // 3 * map[j]: the float offset of converted joint j in a query
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (MVG_WAVE - 1), wave = tid / MVG_WAVE;
  if (MAPPED && tid < J) s_map3[tid] = 3 * (int)map.m[tid];      // visible after the first barrier of the person loop
  long Gl = load_count(num_person, np_is64, b);
  const int G = (int)(Gl < 0 ? 0 : (Gl > Gmax ? Gmax : Gl));
  float* cost = ((long)NQ * Gmax <= KNN_LDS_COSTS) ? cost_lds : cost_ws + (long)b * NQ * Gmax;
  const float* pb = poses + (long)b * NQ * (MAPPED ? Jp : J) * 3;
  const float* gb = gt + (long)b * Gmax * J * 3;
  int* pq = pair_query + (long)b * Pmax;
  int* pg = pair_gt + (long)b * Pmax;
  uint8_t* mb = matched + (long)b * NQ;

  for (int q = tid; q < NQ; q += CRIT_THREADS) mb[q] = 0;
  for (int p = tid; p < Pmax; p += CRIT_THREADS) {
    pq[p] = -1;
    pg[p] = -1;
  }
  match_pose_costs<MAPPED>(pb, gb, box, NQ, G, J, Jp, s_map3, gt_lds, cost);     // match_dev.h
  __syncthreads();

  if (method == MVG_MATCH_KNN) {
    for (int g = wave; g < G; g += CRIT_WAVES) {                 // wave-uniform loop: one wavefront owns a person's column
      float* cg = cost + (long)g * NQ;
      for (int k = 0; k < K; ++k) {
        float bc = INFINITY;
        int bq = 0x7fffffff;
        for (int q = lane; q < NQ; q += MVG_WAVE) {
          const float c = cg[q];                                 // taken entries are NaN: never smaller, never equal
          if (c < bc || (c == bc && q < bq)) {
            bc = c;
            bq = q;
          }
        }
        wave_argmin(bc, bq);
        if (bq < NQ) {                                           // always: K <= NQ entries are left
          if (lane == 0) {
            cg[bq] = __builtin_nanf("");
            pq[g * K + k] = bq;
            pg[g * K + k] = g;
            mb[bq] = 1;                                          // several wavefronts may store the same 1
          }
        }
        __builtin_amdgcn_wave_barrier();
        __threadfence_block();
      }
    }
    if (tid == 0) pair_count[b] = G * K;
  } else {                                                       // MVG_MATCH_MULTIPLE
    if (tid == 0) base_cnt = 0;
    __syncthreads();
    for (int q0 = 0; q0 < NQ; q0 += CRIT_THREADS) {
      const int q = q0 + tid;
      int best = -1;
      float bc = INFINITY;
      if (q < NQ)
        for (int g = 0; g < G; ++g) {
          const float c = cost[(long)g * NQ + q];
          if (c < bc) {
            bc = c;
            best = g;
          }
        }
      const bool ok = best >= 0 && bc < value;
      const unsigned long long m = __ballot(ok);
      if (lane == 0) wave_cnt[wave] = __popcll(m);
      __syncthreads();
      int off = base_cnt;
      for (int w = 0; w < wave; ++w) off += wave_cnt[w];
      off += __popcll(m & ((1ull << lane) - 1ull));
      if (ok && off < Pmax) {
        pq[off] = q;
        pg[off] = best;
        mb[q] = 1;
      }
      __syncthreads();
      if (tid == 0) {
        int t = base_cnt;
        for (int w = 0; w < CRIT_WAVES; ++w) t += wave_cnt[w];
        base_cnt = t;
      }
      __syncthreads();
    }
    if (tid == 0) pair_count[b] = base_cnt < Pmax ? base_cnt : Pmax;
  }
}

// ------------------------------------------------------------------------------------------------------------------------------
// (A) ground truth -> 2D: the norm round trip of joints_3d, pinhole + distortion of image n = v * B + b (cameras.py:167-217), then
// the crop affine of view 0 / batch element 0 (meta[0]['center'][0], cameras.py:28-48), NO clamp.  gt2d (B, Gmax, V, J, 2) fp64.
__global__ __launch_bounds__(CRIT_THREADS) void crit_project_gt_kernel(const float* __restrict__ gt, const float* __restrict__ cams,
                                                                       SpaceBox box, double* __restrict__ gt2d, int B, int Gmax, int V,
                                                                       int J, long total) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int j = (int)(idx % J);
  const int v = (int)((idx / J) % V);
  const long bg = idx / ((long)J * V);
  const int b = (int)(bg / Gmax);
  const float* x = gt + (bg * J + j) * 3;
  const float* cam = cams + ((long)v * B + b) * MVG_CAM_STRIDE;
  const double x0 = norm_round_trip_f64(x[0], box.size[0], box.center[0]);
  const double x1 = norm_round_trip_f64(x[1], box.size[1], box.center[1]);
  const double x2 = norm_round_trip_f64(x[2], box.size[2], box.center[2]);
  const double d0 = x0 - cam[9], d1 = x1 - cam[10], d2 = x2 - cam[11];
  const double xc0 = cam[0] * d0 + cam[1] * d1 + cam[2] * d2;
  const double xc1 = cam[3] * d0 + cam[4] * d1 + cam[5] * d2;
  const double xc2 = cam[6] * d0 + cam[7] * d1 + cam[8] * d2;
  const double zz = xc2 + (double)1e-5f;
  double y0 = xc0 / zz, y1 = xc1 / zz;
  const double r2 = y0 * y0 + y1 * y1;
  const double radial = 1.0 + (cam[16] * r2 + cam[17] * (r2 * r2) + cam[18] * (r2 * r2 * r2));
  const double tang = cam[19] * y1 + cam[20] * y0;
  const double corr = radial + 2.0 * tang;
  y0 = y0 * corr + cam[20] * r2;
  y1 = y1 * corr + cam[19] * r2;
  const double u = cam[12] * y0 + cam[14];
  const double w = cam[13] * y1 + cam[15];
  const float* A = cams + 21;                                    // record 0: view 0, batch element 0
  gt2d[idx * 2] = A[0] * u + A[1] * w + A[2];
  gt2d[idx * 2 + 1] = A[3] * u + A[4] * w + A[5];
}

struct CritArgs {
  const float* logits;        // (L, B, NQ, 2)
  const float* poses;         // (L, B, NQ*Jp, 3)
  const float* poses_2d;      // (L, B, V, NQ*Jp, 2)
  const int* pair_query;      // (B, Pmax)
  const int* pair_gt;         // (B, Pmax)
  const int* pair_count;      // (B,)
  const float* gt;            // (B, Gmax, J, 3)
  const float* vis3d;         // (B, Gmax, J, 3)
  const float* vis2d;         // (V, B, Gmax, J, 2)
  const void* num_person;     // (B,)
  const float* num_samples;   // device scalar or null
  const double* gt2d;         // (B, Gmax, V, J, 2)
  double* part;               // (L, B, CRIT_PART)
  float* g_logits;
  float* g_poses;
  float* g_poses_2d;
  SpaceBox box;
  int np_is64, L, B, NQ, J, V, Gmax, Pmax;       // J: joints of the ground truth (Jc)
  float conf_thr, alpha, gamma;
  int Jp;                     // joints per query of the predictions and their gradients; read by the MAPPED kernel only
  JointMap map;
};

// (B) one workgroup per (layer, batch element).  part[l][b] = {sum focal, sum 3D L1, sum 2D L1, pairs classified right, pairs
// recalled, predicted positives, true positives, predictions over the threshold}; the three gradients with their final scale.
// MAPPED: the two pose loops still run over the (query, converted joint, coordinate) elements in the same order and with the same
// thread assignment as a call on gathered predictions would, so the fp64 sums are the same; only the address of the prediction
// read and of the gradient write goes through the map.  Prediction joints that no map entry names are zeroed in a pass of their
// own: every gradient element has exactly one writer.
template <bool MAPPED>
__global__ __launch_bounds__(CRIT_THREADS) void crit_layer_kernel(CritArgs a) {
  __shared__ short s_pq[CRIT_MAX_PAIRS], s_pg[CRIT_MAX_PAIRS], s_next[CRIT_MAX_PAIRS];
  __shared__ short s_first[CRIT_MAX_NQ];
  __shared__ int s_off[CRIT_MAX_B + 1];
  __shared__ double s_red[CRIT_WAVES];
  __shared__ double s_ns;
  __shared__ int s_map[MAPPED ? 64 : 1];         // converted joint -> prediction joint
  __shared__ int s_named[MAPPED ? 64 : 1];       // prediction joint -> 1 if a map entry names it
  const int l = blockIdx.x / a.B, b = blockIdx.x % a.B, tid = threadIdx.x;
  const int NQ = a.NQ, J = a.J, V = a.V, B = a.B;
  const int Jp = MAPPED ? a.Jp : J;
  if (MAPPED) {                                  // visible after the barriers below
    if (tid < 64) s_named[tid] = 0;
    __syncthreads();
    if (tid < J) {
      s_map[tid] = a.map.m[tid];
      s_named[a.map.m[tid]] = 1;                 // entries are distinct: one writer per element
    }
  }

  if (tid == 0) {
    int off = 0;
    long np = 0;
    for (int i = 0; i < B; ++i) {
      s_off[i] = off;
      const int c = a.pair_count[i];
      off += c < 0 ? 0 : (c > a.Pmax ? a.Pmax : c);
      np += load_count(a.num_person, a.np_is64, i);
    }
    s_off[B] = off;
    // multi_view_pose_transformer.py:847-855; under a process group the caller all-reduces and passes the scalar
    s_ns = a.num_samples ? (double)*a.num_samples : fmax((double)(float)np, 1.0);
  }
  __syncthreads();
  const int Pb = s_off[b + 1] - s_off[b], Ptot = s_off[B];
  for (int p = tid; p < Pb; p += CRIT_THREADS) {
    const int q = a.pair_query[(long)b * a.Pmax + p], g = a.pair_gt[(long)b * a.Pmax + p];
    const bool ok = q >= 0 && q < NQ && g >= 0 && g < a.Gmax;
    s_pq[p] = ok ? (short)q : (short)-1;
    s_pg[p] = ok ? (short)g : (short)-1;
  }
  __syncthreads();
  // per-query chains through this batch element's pairs, in pair order (one writer per query)
  for (int q = tid; q < NQ; q += CRIT_THREADS) {
    int first = -1, last = -1;
    for (int p = 0; p < Pb; ++p)
      if (s_pq[p] == q) {
        if (first < 0) first = p; else s_next[last] = (short)p;
        s_next[p] = -1;
        last = p;
      }
    s_first[q] = (short)first;
  }
  __syncthreads();
  const double ns = s_ns;

  // ---- focal class loss (multi_view_pose_transformer.py:49-78, 582-616) + the counts of the logging metrics
  const float* lg = a.logits + ((long)l * B + b) * NQ * 2;
  float* glg = a.g_logits + ((long)l * B + b) * NQ * 2;
  double s_ce = 0.0;
  int n_pos = 0, n_tp = 0, n_card = 0;
  for (int e = tid; e < NQ * 2; e += CRIT_THREADS) {
    const int q = e >> 1, ch = e & 1;
    const bool m = s_first[q] >= 0;
    const double t = (ch == 1 && m) ? 1.0 : 0.0;
    const double x = lg[e];
    const double p = 1.0 / (1.0 + exp(-x));
    const double ce = fmax(x, 0.0) - x * t + log1p(exp(-fabs(x)));
    const double pt = p * t + (1.0 - p) * (1.0 - t);
    const double om = 1.0 - pt;
    const double mod = (a.gamma == 2.f) ? om * om : pow(om, (double)a.gamma);
    const double dmod = (a.gamma == 2.f) ? 2.0 * om : (om > 0.0 ? (double)a.gamma * pow(om, (double)a.gamma - 1.0) : 0.0);
    const double at = a.alpha >= 0.f ? ((double)a.alpha * t + (1.0 - (double)a.alpha) * (1.0 - t)) : 1.0;
    s_ce += at * ce * mod;
    // d ce / dx = p - t;  d (1 - p_t) / dx = -(2 t - 1) p (1 - p);  loss_ce = sum / NQ / ns * NQ
    const double g = at * ((p - t) * mod - ce * dmod * (2.0 * t - 1.0) * p * (1.0 - p));
    glg[e] = (float)(g / (double)NQ / ns * (double)NQ);
    if (ch == 1) {
      const float x1 = lg[e], x0 = lg[e - 1];
      const bool over = 1.f / (1.f + expf(-x1)) > a.conf_thr;     // misc.py:557-558 in fp32
      n_card += over;
      const bool pos = over && x1 > x0;
      n_pos += pos;
      n_tp += pos && m;
    }
  }
  int n_ok = 0, n_rec = 0;
  for (int p = tid; p < Pb; p += CRIT_THREADS) {
    const int q = s_pq[p];
    if (q < 0) continue;
    const float x0 = lg[q * 2], x1 = lg[q * 2 + 1];
    const bool top1 = x1 > x0;
    n_ok += top1 && (1.f / (1.f + expf(-x1)) > 0.f);
    n_rec += top1 && (1.f / (1.f + expf(-x1)) > a.conf_thr);
  }

  // ---- per-joint 3D L1 on the matched pairs (:653-696, loss.py:87-97); prediction as is, target = norm round trip
  const float* ps = a.poses + ((long)l * B + b) * NQ * Jp * 3;
  float* gps = a.g_poses + ((long)l * B + b) * NQ * Jp * 3;
  const double sc3 = 1.0 / ns / (double)(J * 3);
  double s_3d = 0.0;
  for (int e = tid; e < NQ * J * 3; e += CRIT_THREADS) {
    const int c = e % 3, j = (e / 3) % J, q = e / (3 * J);
    const int ep = MAPPED ? (q * Jp + s_map[j]) * 3 + c : e;      // the element of the prediction and of its gradient
    double g = 0.0;
    for (int p = s_first[q]; p >= 0; p = s_next[p]) {
      const long gi = (((long)b * a.Gmax + s_pg[p]) * J + j) * 3;
      const double w = a.vis3d[gi];                                // joints_3d_vis[..., 0:1]
      const double tg = norm_round_trip_f64(a.gt[gi + c], a.box.size[c], a.box.center[c]);
      const double d = (double)ps[ep] * w - tg * w;
      s_3d += fabs(d);
      g += (d > 0.0 ? w : (d < 0.0 ? -w : 0.0));
    }
    gps[ep] = (float)(g * sc3);
  }
  if (MAPPED && J < Jp)
    for (int e = tid; e < NQ * Jp * 3; e += CRIT_THREADS)
      if (!s_named[(e / 3) % Jp]) gps[e] = 0.f;

  // ---- 2D L1 against the projected ground truth (:732-772, loss.py:245-297).  Row r = pair * V + view of the pair-major
  // predictions is weighted by row r of the VIEW-major weights: view r / P, pair r % P over the pairs of the whole batch.
  const float* p2 = a.poses_2d + ((long)l * B + b) * V * NQ * Jp * 2;
  float* gp2 = a.g_poses_2d + ((long)l * B + b) * V * NQ * Jp * 2;
  const double sc2 = 1.0 / (ns * (double)V) / (double)(J * 2);
  double s_2d = 0.0;
  for (long e = tid; e < (long)V * NQ * J * 2; e += CRIT_THREADS) {
    const int c = (int)(e & 1), j = (int)((e >> 1) % J), q = (int)((e >> 1) / J % NQ), v = (int)((e >> 1) / ((long)J * NQ));
    const long ep = MAPPED ? (((long)v * NQ + q) * Jp + s_map[j]) * 2 + c : e;
    double g = 0.0;
    for (int p = s_first[q]; p >= 0; p = s_next[p]) {
      const long r = (long)(s_off[b] + p) * V + v;
      const int vw = (int)(r / Ptot), pw = (int)(r % Ptot);
      int bw = 0;
      while (bw + 1 < B && s_off[bw + 1] <= pw) ++bw;
      int gw = a.pair_gt[(long)bw * a.Pmax + (pw - s_off[bw])];
      double w = 0.0;
      if (gw >= 0 && gw < a.Gmax) w = a.vis2d[((((long)vw * B + bw) * a.Gmax + gw) * J + j) * 2];   // joints_vis[..., 0:1]
      const double tg = a.gt2d[((((long)b * a.Gmax + s_pg[p]) * V + v) * J + j) * 2 + c];
      const double d = (double)p2[ep] * w - tg * w;
      s_2d += fabs(d);
      g += (d > 0.0 ? w : (d < 0.0 ? -w : 0.0));
    }
    gp2[ep] = (float)(g * sc2);
  }
  if (MAPPED && J < Jp)
    for (long e = tid; e < (long)V * NQ * Jp * 2; e += CRIT_THREADS)
      if (!s_named[(int)((e >> 1) % Jp)]) gp2[e] = 0.f;

  double* out = a.part + ((long)l * B + b) * CRIT_PART;
  const auto sum = [&](double v) { return block_sum<CRIT_WAVES>(v, s_red); };      // exact_dev.h; valid in thread 0
  const double r0 = sum(s_ce), r1 = sum(s_3d), r2 = sum(s_2d), r3 = sum((double)n_ok), r4 = sum((double)n_rec);
  const double r5 = sum((double)n_pos), r6 = sum((double)n_tp), r7 = sum((double)n_card);
  if (tid == 0) {
    out[0] = r0; out[1] = r1; out[2] = r2; out[3] = r3; out[4] = r4; out[5] = r5; out[6] = r6; out[7] = r7;
  }
}

// (C) table (L, 8): loss_ce, class_error, class_recall, class_precision, cardinality_error, loss_pose_perjoint,
// loss_pose_perprojection_2d, keep_2d (0 where the 2D loss exceeded 1e5 and was zeroed, :770-771; else 1)
__global__ __launch_bounds__(CRIT_THREADS) void crit_final_kernel(const double* __restrict__ part, const int* __restrict__ pair_count,
                                                                  const void* __restrict__ num_person, int np_is64,
                                                                  const float* __restrict__ num_samples, float* __restrict__ table,
                                                                  int L, int B, int NQ, int J, int V, int Pmax) {
  for (int l = threadIdx.x; l < L; l += CRIT_THREADS) {
    double s[CRIT_PART] = {0, 0, 0, 0, 0, 0, 0, 0};
    double card = 0.0;
    long np = 0, P = 0;
    for (int b = 0; b < B; ++b) {
      const double* p = part + ((long)l * B + b) * CRIT_PART;
      for (int i = 0; i < CRIT_PART; ++i) s[i] += p[i];
      const long n = load_count(num_person, np_is64, b);
      np += n;
      card += fabs(p[7] - (double)n);
      const int c = pair_count[b];
      P += c < 0 ? 0 : (c > Pmax ? Pmax : c);
    }
    const double ns = num_samples ? (double)*num_samples : fmax((double)(float)np, 1.0);
    float* t = table + (long)l * 8;
    t[0] = (float)(s[0] / (double)NQ / ns * (double)NQ);
    t[1] = (float)(100.0 - (P > 0 ? s[3] * (100.0 / (double)P) : 0.0));
    t[2] = (float)(P > 0 ? s[4] * (100.0 / (double)P) : 0.0);
    t[3] = (float)(s[6] * (100.0 / (s[5] + 1e-5)));
    t[4] = (float)(card / (double)B);
    t[5] = (float)(s[1] / ns / (double)(J * 3));
    const float l2d = (float)(s[2] / (ns * (double)V) / (double)(J * 2));
    const bool keep = !(l2d > 1e5f);
    t[6] = keep ? l2d : l2d * 0.0f;
    t[7] = keep ? 1.f : 0.f;
  }
}

extern "C" {

size_t mvg_knn_match_workspace(int B, int NQ, int Gmax) {
  if (B < 1 || NQ < 1 || Gmax < 1) return 0;
  return ((long)NQ * Gmax <= KNN_LDS_COSTS) ? 0 : (size_t)B * NQ * Gmax * sizeof(float);
}

int mvg_knn_match_jm(const float* poses, const float* joints_3d, const void* num_person, int num_person_is64,
                     const float* space_size, const float* space_center, int method, int K, float value, int B, int NQ, int Gmax,
                     int Jp, int Jc, const int* joint_map, int Pmax, void* workspace, size_t workspace_bytes, int* pair_query,
                     int* pair_gt, int* pair_count, uint8_t* matched, void* stream) {
  if (mvg_any_null({poses, joints_3d, num_person, space_size, space_center, pair_query, pair_gt, pair_count, matched}))
    return MVG_E_BADARG;
  JointMap map;
  if (B < 1 || NQ < 1 || Gmax < 1 || Gmax > 64 || !pack_joint_map(Jp, Jc, joint_map, &map)) return MVG_E_BADARG;
  if (method == MVG_MATCH_KNN) {
    if (K < 1 || K > 16 || K > NQ || Pmax < Gmax * K) return MVG_E_BADARG;
  } else if (method == MVG_MATCH_MULTIPLE) {
    if (!(value > 0.f) || Pmax < NQ) return MVG_E_BADARG;
  } else {
    return MVG_E_BADARG;
  }
  const size_t need = mvg_knn_match_workspace(B, NQ, Gmax);
  if (need && (!workspace || workspace_bytes < need)) return MVG_E_BADARG;
  SpaceBox box;
  for (int i = 0; i < 3; ++i) {
    box.size[i] = space_size[i];
    box.center[i] = space_center[i];
  }
  if (joint_map)
    hipLaunchKernelGGL(knn_match_kernel<true>, dim3(B), dim3(CRIT_THREADS), 0, (hipStream_t)stream, poses, joints_3d, num_person,
                       num_person_is64, box, method, K, value, NQ, Gmax, Jc, Pmax, (float*)workspace, pair_query, pair_gt,
                       pair_count, matched, Jp, map);
  else
    hipLaunchKernelGGL(knn_match_kernel<false>, dim3(B), dim3(CRIT_THREADS), 0, (hipStream_t)stream, poses, joints_3d, num_person,
                       num_person_is64, box, method, K, value, NQ, Gmax, Jc, Pmax, (float*)workspace, pair_query, pair_gt,
                       pair_count, matched, Jp, map);
  MVG_LAUNCH_CHECK();
  return 0;
}

int mvg_knn_match(const float* poses, const float* joints_3d, const void* num_person, int num_person_is64, const float* space_size,
                  const float* space_center, int method, int K, float value, int B, int NQ, int Gmax, int J, int Pmax,
                  void* workspace, size_t workspace_bytes, int* pair_query, int* pair_gt, int* pair_count, uint8_t* matched,
                  void* stream) {
  return mvg_knn_match_jm(poses, joints_3d, num_person, num_person_is64, space_size, space_center, method, K, value, B, NQ, Gmax,
                          J, J, nullptr, Pmax, workspace, workspace_bytes, pair_query, pair_gt, pair_count, matched, stream);
}

size_t mvg_criterion_workspace(int L, int B, int Gmax, int V, int J) {
  if (L < 1 || B < 1 || Gmax < 1 || V < 1 || J < 1) return 0;
  return ((size_t)B * Gmax * V * J * 2 + (size_t)L * B * CRIT_PART) * sizeof(double);
}

int mvg_criterion_jm(const float* logits, const float* poses, const float* poses_2d, const int* pair_query, const int* pair_gt,
                     const int* pair_count, const float* joints_3d, const float* joints_3d_vis, const float* joints_vis,
                     const void* num_person, int num_person_is64, const float* num_samples, const float* cams,
                     const float* space_size, const float* space_center, float pred_conf_threshold, float focal_alpha,
                     float focal_gamma, int L, int B, int NQ, int Jp, int Jc, const int* joint_map, int V, int Gmax, int Pmax,
                     void* workspace, size_t workspace_bytes, float* table, float* grad_logits, float* grad_poses,
                     float* grad_poses_2d, void* stream) {
  const int J = Jc;
  if (mvg_any_null({logits, poses, poses_2d, pair_query, pair_gt, pair_count, joints_3d, joints_3d_vis, joints_vis, num_person,
                    cams, space_size, space_center, workspace, table, grad_logits, grad_poses, grad_poses_2d}))
    return MVG_E_BADARG;
  CritArgs a;
  if (L < 1 || B < 1 || B > CRIT_MAX_B || NQ < 1 || NQ > CRIT_MAX_NQ || !pack_joint_map(Jp, Jc, joint_map, &a.map) || V < 1 ||
      Gmax < 1 || Gmax > 64 || Pmax < 1 || Pmax > CRIT_MAX_PAIRS)
    return MVG_E_BADARG;
  if (workspace_bytes < mvg_criterion_workspace(L, B, Gmax, V, J)) return MVG_E_BADARG;
  if (mvg_any_misaligned(8, {workspace})) return MVG_E_BADARG;
  a.logits = logits; a.poses = poses; a.poses_2d = poses_2d;
  a.pair_query = pair_query; a.pair_gt = pair_gt; a.pair_count = pair_count;
  a.gt = joints_3d; a.vis3d = joints_3d_vis; a.vis2d = joints_vis;
  a.num_person = num_person; a.np_is64 = num_person_is64; a.num_samples = num_samples;
  double* gt2d = (double*)workspace;
  a.gt2d = gt2d;
  a.part = gt2d + (size_t)B * Gmax * V * J * 2;
  a.g_logits = grad_logits; a.g_poses = grad_poses; a.g_poses_2d = grad_poses_2d;
  for (int i = 0; i < 3; ++i) {
    a.box.size[i] = space_size[i];
    a.box.center[i] = space_center[i];
  }
  a.L = L; a.B = B; a.NQ = NQ; a.J = J; a.V = V; a.Gmax = Gmax; a.Pmax = Pmax; a.Jp = Jp;
  a.conf_thr = pred_conf_threshold; a.alpha = focal_alpha; a.gamma = focal_gamma;
  const long total = (long)B * Gmax * V * J;
  hipLaunchKernelGGL(crit_project_gt_kernel, dim3(mvg_ceil_div(total, CRIT_THREADS)), dim3(CRIT_THREADS), 0, (hipStream_t)stream,
                     joints_3d, cams, a.box, gt2d, B, Gmax, V, J, total);
  MVG_LAUNCH_CHECK();
  if (joint_map)
    hipLaunchKernelGGL(crit_layer_kernel<true>, dim3(L * B), dim3(CRIT_THREADS), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(crit_layer_kernel<false>, dim3(L * B), dim3(CRIT_THREADS), 0, (hipStream_t)stream, a);
  MVG_LAUNCH_CHECK();
  hipLaunchKernelGGL(crit_final_kernel, dim3(1), dim3(CRIT_THREADS), 0, (hipStream_t)stream, (const double*)a.part, pair_count,
                     num_person, num_person_is64, num_samples, table, L, B, NQ, J, V, Pmax);
  MVG_LAUNCH_CHECK();
  return 0;
}

int mvg_criterion(const float* logits, const float* poses, const float* poses_2d, const int* pair_query, const int* pair_gt,
                  const int* pair_count, const float* joints_3d, const float* joints_3d_vis, const float* joints_vis,
                  const void* num_person, int num_person_is64, const float* num_samples, const float* cams, const float* space_size,
                  const float* space_center, float pred_conf_threshold, float focal_alpha, float focal_gamma, int L, int B, int NQ,
                  int J, int V, int Gmax, int Pmax, void* workspace, size_t workspace_bytes, float* table, float* grad_logits,
                  float* grad_poses, float* grad_poses_2d, void* stream) {
  return mvg_criterion_jm(logits, poses, poses_2d, pair_query, pair_gt, pair_count, joints_3d, joints_3d_vis, joints_vis, num_person,
                          num_person_is64, num_samples, cams, space_size, space_center, pred_conf_threshold, focal_alpha,
                          focal_gamma, L, B, NQ, J, J, nullptr, V, Gmax, Pmax, workspace, workspace_bytes, table, grad_logits,
                          grad_poses, grad_poses_2d, stream);
}

}  // extern "C"
