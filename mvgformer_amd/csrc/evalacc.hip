// Validation scoring for gfx950: the ground-truth matching of Panoptic.evaluate (lib/dataset/panoptic.py:497-556) and the PCP
// counters of Shelf.evaluate / Campus.evaluate (lib/dataset/shelf.py:255-330) on the rows that mvg_pose_nms leaves, accumulated in
// device memory over the frames of a validation run.  Fixed shapes, nothing read back, no host synchronisation: both calls can
// sit behind the NMS in the HIP graph of the decoder forward; the host reads the list / the counters once, at the end of the run.
//
//   mvg_eval_match   2 launches:
//     (A) eval_match_kernel    one workgroup per batch element: participating rows (flag >= 0, row < count), their position in the
//                              element by an LDS scan, the element's offset by counting the rows of the elements in front of it;
//                              one thread per participating row computes the visible-joint mean distance to every person and
//                              appends (mpjpe, score, gt_id) at cursor + offset + position, if that lies below the capacity
//     (B) eval_advance_kernel  one workgroup: counts what (A) appended and moves the cursor, total_gt, frames, kept_rows; sets
//                              `overflow` when the cursor passes the capacity.  (A) only READS the state, so every element of a
//                              call sees the same cursor.
//   mvg_eval_pcp     1 launch, one workgroup: elements and actors in order, threads over the rows; every counter has this one
//                    writer (thread 0).
//
// Arithmetic: fp64 from the fp32 inputs, sqrt((x^2 + y^2) + z^2) with a correctly rounded sqrt, joints summed in joint order.
// The distances are dist3 / norm3 of exact_dev.h, the FUSED form: see CONTRACTION there for when that is the rounding of every
// operation on its own.  The only atomics are integer adds in LDS; no result depends on the order in which workgroups or
// wavefronts run, so two runs give the same bits.
#include <math.h>

#include "exact_dev.h"

#define EVAL_THREADS 256
static_assert(EVAL_THREADS == SCAN_THREADS, "eval_match_kernel calls scan_rows; the other kernels only share the constant");
#define EVAL_MAX_R MVG_EVAL_MAX_R
#define EVAL_MAX_J MVG_EVAL_MAX_J

enum { ST_ENTRIES = 0, ST_TOTAL_GT = 1, ST_FRAMES = 2, ST_OVERFLOW = 3, ST_KEPT_ROWS = 4, ST_MATCH_GT = 5, ST_EMPTY_FRAME = 6 };

// NaN is ordered last in the comparisons (evaluate._nan_last); the stored value stays what it is
static __device__ __forceinline__ double eval_nan_last(double v) { return v != v ? (double)INFINITY : v; }

// participating rows of element b, counted by the whole workgroup into *s_acc (LDS, zeroed by the caller, barrier after)
static __device__ __forceinline__ void eval_count_rows(const float* dets, const int* count, int b, int R, int J, int* s_acc) {
  const int rows = det_rows(count, b, R);
  int mine = 0;
  for (int i = threadIdx.x; i < rows; i += EVAL_THREADS) mine += det_flag(dets, b, i, R, J) ? 1 : 0;
  if (mine) atomicAdd(s_acc, mine);
}

// ------------------------------------------------------------------------------------------------------------------------------
// (A) one workgroup per batch element
__global__ __launch_bounds__(EVAL_THREADS) void eval_match_kernel(const float* __restrict__ dets, const int* __restrict__ count,
                                                                  const float* __restrict__ gt, const float* __restrict__ vis,
                                                                  const int* __restrict__ num_person, int R, int J, int Gmax,
                                                                  double* __restrict__ mpjpe, double* __restrict__ score,
                                                                  i64* __restrict__ gt_id, i64 capacity, const i64* __restrict__ state) {
  __shared__ int s_pos[EVAL_MAX_R];           // position of a participating row inside its element, -1 for the others
  __shared__ int s_scan[2][1][SCAN_THREADS];
  __shared__ int s_before;                    // entries of the elements in front of this one
  const int b = blockIdx.x, t = threadIdx.x;
  const int G = clamp_count(num_person[b], Gmax);
  if (G == 0) return;                          // panoptic.py:508: no entry, nothing added to total_gt (uniform for the workgroup)
  if (t == 0) s_before = 0;
  __syncthreads();
  i64 gt_before = 0;
  for (int e = 0; e < b; ++e) {
    const int Ge = clamp_count(num_person[e], Gmax);
    if (Ge == 0) continue;
    gt_before += Ge;
    eval_count_rows(dets, count, e, R, J, &s_before);
  }
  // the position of every participating row among those of the element
  const int rows = det_rows(count, b, R);
  const auto takes_part = [=](int i) { return i < rows && det_flag(dets, b, i, R, J); };
  const RowScan<1> run = scan_rows<1>(R, s_scan, [=](int i, int* n) { n[0] += takes_part(i) ? 1 : 0; });
  int pos = run.before(0);
  for (int i = run.lo; i < run.hi; ++i) {
    const bool in = takes_part(i);
    s_pos[i] = in ? pos : -1;
    pos += in ? 1 : 0;
  }
  __syncthreads();
  const i64 base = state[ST_ENTRIES] + s_before;
  const i64 first_gt = state[ST_TOTAL_GT] + gt_before;
  const float* g0 = gt + (size_t)b * Gmax * J * 3;
  const float* v0 = vis + (size_t)b * Gmax * J;
  for (int i = t; i < R; i += EVAL_THREADS) {
    if (s_pos[i] < 0) continue;
    const i64 at = base + s_pos[i];
    if (at < 0 || at >= capacity) continue;    // past the capacity: counted by (B), never written
    const float* p = dets + ((size_t)b * R + i) * J * 5;
    int best = 0;
    double best_cmp = 0.0, best_val = 0.0;
    for (int g = 0; g < G; ++g) {
      // (d * w).sum(-1) / w.sum(-1) with w = visible ? 1 : 0: a person without visible joints gives 0 / 0 = NaN, like the host
      double sum = 0.0, w_sum = 0.0;
      for (int j = 0; j < J; ++j) {
        const double w = v0[g * J + j] > 0.f ? 1.0 : 0.0;
        sum += dist3(p + j * 5, g0 + (g * J + j) * 3) * w;
        w_sum += w;
      }
      const double m = sum / w_sum, cmp = eval_nan_last(m);
      if (g == 0 || cmp < best_cmp) {           // first minimum
        best = g;
        best_cmp = cmp;
        best_val = m;
      }
    }
    mpjpe[at] = best_val;
    score[at] = (double)p[4];
    gt_id[at] = first_gt + best;
  }
}

// (B) one workgroup: the cursor moves after every element of the call has read it
__global__ __launch_bounds__(EVAL_THREADS) void eval_advance_kernel(const float* __restrict__ dets, const int* __restrict__ count,
                                                                    const int* __restrict__ num_person, int B, int R, int J, int Gmax,
                                                                    i64 capacity, i64* __restrict__ state) {
  __shared__ int s_acc[2];                    // [0] rows that appended an entry, [1] all participating rows
  if (threadIdx.x < 2) s_acc[threadIdx.x] = 0;
  __syncthreads();
  i64 gts = 0;
  for (int b = 0; b < B; ++b) {
    const int G = clamp_count(num_person[b], Gmax);
    gts += G;
    eval_count_rows(dets, count, b, R, J, &s_acc[1]);
    if (G > 0) eval_count_rows(dets, count, b, R, J, &s_acc[0]);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const i64 n = state[ST_ENTRIES] + s_acc[0];
    state[ST_ENTRIES] = n;
    state[ST_TOTAL_GT] += gts;
    state[ST_FRAMES] += B;
    if (n > capacity) state[ST_OVERFLOW] = 1;
    state[ST_KEPT_ROWS] += s_acc[1];
  }
}

// ------------------------------------------------------------------------------------------------------------------------------
// PCP: the nine limbs of shelf.py:270-271 and the hip-centre / head test of shelf.py:308-315, 14-joint format
__constant__ int c_limb_a[9] = {0, 1, 3, 4, 6, 7, 9, 10, 12};
__constant__ int c_limb_b[9] = {1, 2, 4, 5, 7, 8, 10, 11, 13};

__global__ __launch_bounds__(EVAL_THREADS) void eval_pcp_kernel(const float* __restrict__ dets, const int* __restrict__ count,
                                                                const float* __restrict__ gt, const float* __restrict__ vis,
                                                                const int* __restrict__ num_person, int B, int R, int J, int Gmax, int A,
                                                                double recall_threshold, double alpha, i64* __restrict__ correct,
                                                                i64* __restrict__ total, i64* __restrict__ bone_correct,
                                                                i64* __restrict__ state) {
  __shared__ unsigned char s_part[EVAL_MAX_R];
  __shared__ double s_val[EVAL_THREADS];      // per thread: its smallest mean (NaN ordered last) ...
  __shared__ double s_raw[EVAL_THREADS];      // ... the same mean as computed ...
  __shared__ int s_row[EVAL_THREADS];         // ... and its row, R when the thread saw no participating row
  __shared__ int s_n, s_annotated;
  const int t = threadIdx.x;
  const i64 frame0 = state[ST_FRAMES];
  i64 kept = 0;
  for (int b = 0; b < B; ++b) {
    if (t == 0) s_n = 0;
    __syncthreads();
    const int rows = det_rows(count, b, R);
    int mine = 0;
    for (int i = t; i < R; i += EVAL_THREADS) {
      const bool in = i < rows && det_flag(dets, b, i, R, J);
      s_part[i] = in ? 1 : 0;
      mine += in ? 1 : 0;
    }
    if (mine) atomicAdd(&s_n, mine);
    __syncthreads();
    const int n = s_n;
    kept += n;
    const int actors = min(clamp_count(num_person[b], Gmax), A);
    for (int a = 0; a < actors; ++a) {
      const float* g = gt + ((size_t)b * Gmax + a) * J * 3;
      const float* v = vis + ((size_t)b * Gmax + a) * J;
      if (t == 0) s_annotated = 0;
      __syncthreads();
      if (t < J && v[t] != 0.f) s_annotated = 1;             // validate.actor_ground_truth: some visibility != 0
      __syncthreads();
      const bool annotated = s_annotated != 0;
      __syncthreads();                                         // s_annotated is reset in the next round
      if (!annotated) continue;
      if (n == 0) {                                            // evaluate_pcp raises here; the finaliser does, from this word
        if (t == 0 && state[ST_EMPTY_FRAME] == 0) state[ST_EMPTY_FRAME] = frame0 + b + 1;
        break;
      }
      // the participating row of smallest mean joint distance, first minimum (shelf.py:292-295)
      double my_cmp = (double)INFINITY, my_raw = 0.0;
      int my_row = R;
      for (int i = t; i < R; i += EVAL_THREADS) {
        if (!s_part[i]) continue;
        const float* p = dets + ((size_t)b * R + i) * J * 5;
        double sum = 0.0;
        for (int j = 0; j < J; ++j) sum += dist3(g + j * 3, p + j * 5);
        const double m = sum / (double)J, cmp = eval_nan_last(m);
        if (my_row == R || cmp < my_cmp) {                     // rows of a thread ascend: the first minimum stays
          my_cmp = cmp;
          my_raw = m;
          my_row = i;
        }
      }
      s_val[t] = my_cmp;
      s_raw[t] = my_raw;
      s_row[t] = my_row;
      __syncthreads();
      for (int step = EVAL_THREADS / 2; step > 0; step >>= 1) {
        if (t < step) {
          const double ov = s_val[t + step];
          const int orow = s_row[t + step];
          const bool take = orow < R && (s_row[t] == R || ov < s_val[t] || (ov == s_val[t] && orow < s_row[t]));
          if (take) {
            s_val[t] = ov;
            s_raw[t] = s_raw[t + step];
            s_row[t] = orow;
          }
        }
        __syncthreads();
      }
      if (t == 0) {
        const float* p = dets + ((size_t)b * R + s_row[0]) * J * 5;
        if (s_raw[0] < recall_threshold) state[ST_MATCH_GT] += 1;
        state[ST_TOTAL_GT] += 1;
        int ok_all = 0;
        for (int k = 0; k < 9; ++k) {
          const int ja = c_limb_a[k], jb = c_limb_b[k];
          const double e_s = dist3(p + ja * 5, g + ja * 3), e_e = dist3(p + jb * 5, g + jb * 3);
          const double len = dist3(g + ja * 3, g + jb * 3);
          const int ok = ((e_s + e_e) / 2.0 <= alpha * len) ? 1 : 0;
          bone_correct[a * 10 + k] += ok;
          ok_all += ok;
        }
        double ph[3], gh[3];
        for (int c = 0; c < 3; ++c) {
          ph[c] = ((double)p[2 * 5 + c] + (double)p[3 * 5 + c]) / 2.0;
          gh[c] = ((double)g[2 * 3 + c] + (double)g[3 * 3 + c]) / 2.0;
        }
        const double e_hip = norm3(ph[0] - gh[0], ph[1] - gh[1], ph[2] - gh[2]);
        const double e_head = dist3(p + 12 * 5, g + 12 * 3);
        const double len = norm3(gh[0] - (double)g[12 * 3], gh[1] - (double)g[12 * 3 + 1], gh[2] - (double)g[12 * 3 + 2]);
        const int ok = ((e_hip + e_head) / 2.0 <= alpha * len) ? 1 : 0;
        bone_correct[a * 10 + 9] += ok;
        correct[a] += ok_all + ok;
        total[a] += 10;
      }
      __syncthreads();
    }
    __syncthreads();
  }
  if (t == 0) {
    state[ST_FRAMES] = frame0 + B;
    state[ST_KEPT_ROWS] += kept;
  }
}

static bool eval_bad_shape(int B, int R, int J, int Gmax) {
  return B < 1 || B > MVG_EVAL_MAX_B || R < 1 || R > EVAL_MAX_R || J < 1 || J > EVAL_MAX_J || Gmax < 1 || Gmax > MVG_EVAL_MAX_G;
}

extern "C" {

int mvg_eval_match(const float* dets, const int* count, const float* joints_3d, const float* joints_3d_vis, const int* num_person, int B,
                   int R, int J, int Gmax, double* mpjpe, double* score, int64_t* gt_id, int64_t capacity, int64_t* state,
                   void* stream) {
  if (eval_bad_shape(B, R, J, Gmax) || capacity < 1) return MVG_E_BADARG;
  if (mvg_any_null({dets, joints_3d, joints_3d_vis, num_person, mpjpe, score, gt_id, state})) return MVG_E_BADARG;
  if (mvg_any_misaligned(8, {mpjpe, score, gt_id, state})) return MVG_E_BADARG;
  hipLaunchKernelGGL(eval_match_kernel, dim3(B), dim3(EVAL_THREADS), 0, (hipStream_t)stream, dets, count, joints_3d, joints_3d_vis,
                     num_person, R, J, Gmax, mpjpe, score, (i64*)gt_id, (i64)capacity, (const i64*)state);
  MVG_LAUNCH_CHECK();
  hipLaunchKernelGGL(eval_advance_kernel, dim3(1), dim3(EVAL_THREADS), 0, (hipStream_t)stream, dets, count, num_person, B, R, J, Gmax,
                     (i64)capacity, (i64*)state);
  MVG_LAUNCH_CHECK();
  return 0;
}

int mvg_eval_pcp(const float* dets, const int* count, const float* joints_3d, const float* joints_3d_vis, const int* num_person, int B,
                 int R, int J, int Gmax, int actors, double recall_threshold, double alpha, int64_t* correct, int64_t* total,
                 int64_t* bone_correct, int64_t* state, void* stream) {
  if (eval_bad_shape(B, R, J, Gmax) || J != 14 || actors < 1 || actors > MVG_EVAL_MAX_G) return MVG_E_BADARG;
  if (!(alpha >= 0.0) || recall_threshold != recall_threshold) return MVG_E_BADARG;
  if (mvg_any_null({dets, joints_3d, joints_3d_vis, num_person, correct, total, bone_correct, state})) return MVG_E_BADARG;
  if (mvg_any_misaligned(8, {correct, total, bone_correct, state})) return MVG_E_BADARG;
  hipLaunchKernelGGL(eval_pcp_kernel, dim3(1), dim3(EVAL_THREADS), 0, (hipStream_t)stream, dets, count, joints_3d, joints_3d_vis,
                     num_person, B, R, J, Gmax, actors, recall_threshold, alpha, (i64*)correct, (i64*)total, (i64*)bone_correct,
                     (i64*)state);
  MVG_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
