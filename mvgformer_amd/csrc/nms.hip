// Serving post-processing for gfx950: the classification filter and the nearby-joints NMS of run/validate_3d.py:228-234
// (lib/core/nms.py:210-283) on the packed predictions [x, y, z, flag, score], for a whole batch, without a host round trip and
// with fixed shapes, so that the call can sit in the same HIP graph as the decoder.
//
//   mvg_pose_nms   3 launches:
//     (A) nms_rank_kernel    one workgroup per batch element: candidates (flag >= 0), their visiting rank by counting, the fp64
//                            distance limit of every candidate -> workspace, in RANK space (rank 0 is visited first)
//     (B) nms_close_kernel   grid (column word, row tile, batch element): 64 x 64 pose pairs per workgroup, both tiles staged
//                            in LDS, one 64-bit word of `close` per (row, column word) from a wavefront ballot; workgroups beyond
//                            the candidate count leave at once
//     (C) nms_greedy_kernel  one workgroup per batch element; wavefront 0 runs the greedy pass (lane w owns word w of the ignored
//                            mask and of the current row), then all wavefronts apply max_dets and write keep / count / dets
//
// Arithmetic of the closeness test: fp64 from the fp32 inputs in numpy's order, sqrt((x^2 + y^2) + z^2) with a correctly rounded
// sqrt.  The diagonal and the distances are norm3 of exact_dev.h, the FUSED form: the boolean matrix is the reference's bit for
// bit under the input condition that CONTRACTION there states.  No floating-point atomics, no data-dependent loop bound other
// than the candidate count, which every kernel clamps to N.
#include <math.h>

#include "exact_dev.h"

#define NMS_MAX_N MVG_NMS_MAX_N             // 2048: 32 words of 64 candidates: one lane per word in the greedy pass
#define NMS_MAX_J MVG_NMS_MAX_J
#define NMS_RANK_THREADS 1024
#define NMS_TILE 64                         // rows and columns of `close` per workgroup of (B)
#define NMS_CLOSE_THREADS 256
#define NMS_GREEDY_THREADS 256
#define NMS_PREFETCH 8                      // rows of `close` the greedy pass loads ahead of their use
#define NMS_HEADER 16                       // bytes in front of the per-element arrays: int32 candidate count

// workspace of one batch element (8-byte aligned pieces, doubles and words first)
struct NmsWorkspace {
  int* header;        // [0] = M, the number of candidates
  double* limit;      // (N) distance limit by rank
  u64* close;         // (N, W) bit c of word w of row a: candidate of rank 64 w + c is close to the candidate of rank a
  int* rank2row;      // (N) row index by rank
  int* group_last;    // (N) last rank of the run of equal scores that the rank belongs to
  unsigned* key;      // (N) the score's ordered key by rank
};

static __host__ __device__ inline size_t nms_words(int N) { return (size_t)((N + 63) / 64); }
static __host__ __device__ inline size_t nms_element_bytes(int N) {
  return NMS_HEADER + (size_t)N * sizeof(double) + (size_t)N * nms_words(N) * sizeof(u64) + 3 * (((size_t)N + 1) / 2 * 2) * sizeof(int);
}
static __device__ __forceinline__ NmsWorkspace nms_workspace(void* base, int b, int N) {
  char* p = (char*)base + (size_t)b * nms_element_bytes(N);
  const size_t n_even = ((size_t)N + 1) / 2 * 2;
  NmsWorkspace w;
  w.header = (int*)p;
  p += NMS_HEADER;
  w.limit = (double*)p;
  p += (size_t)N * sizeof(double);
  w.close = (u64*)p;
  p += (size_t)N * nms_words(N) * sizeof(u64);
  w.rank2row = (int*)p;
  w.group_last = w.rank2row + n_even;
  w.key = (unsigned*)(w.group_last + n_even);
  return w;
}
static __device__ __forceinline__ int nms_candidates(const NmsWorkspace& w, int N) { return clamp_count(w.header[0], N); }

// Total order on the scores that agrees with numpy's: -0 == +0, every NaN equal and above +inf (np.argsort puts NaN last, np.argmax
// returns the first NaN).
static __device__ __forceinline__ unsigned score_key(float s) {
  if (s != s) return 0xFFFFFFFFu;
  if (s == 0.f) s = 0.f;
  const unsigned u = __float_as_uint(s);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// ------------------------------------------------------------------------------------------------------------------------------
// (A) candidates, visiting rank, distance limit.  Visiting order: descending score, among equal scores the higher row first
// (np.argsort(scores, kind="stable")[::-1]); rank = number of candidates that are visited earlier.
__global__ __launch_bounds__(NMS_RANK_THREADS) void nms_rank_kernel(const float* __restrict__ pred, void* workspace, int N, int J,
                                                                    double dist_thr) {
  __shared__ unsigned s_key[NMS_MAX_N];
  __shared__ unsigned char s_cand[NMS_MAX_N];
  __shared__ int s_count;
  const int b = blockIdx.x;
  const float* p = pred + (size_t)b * N * J * 5;
  const NmsWorkspace ws = nms_workspace(workspace, b, N);
  if (threadIdx.x == 0) s_count = 0;
  __syncthreads();
  for (int n = threadIdx.x; n < N; n += NMS_RANK_THREADS) {
    const float* row = p + (size_t)n * J * 5;
    const bool cand = row[3] >= 0.f;
    s_cand[n] = cand ? 1 : 0;
    s_key[n] = score_key(row[4]);
    if (cand) atomicAdd(&s_count, 1);
  }
  __syncthreads();
  if (threadIdx.x == 0) ws.header[0] = s_count;
  for (int n = threadIdx.x; n < N; n += NMS_RANK_THREADS) {
    if (!s_cand[n]) continue;
    const unsigned k = s_key[n];
    int before = 0, equal_below = 0;
    for (int m = 0; m < N; ++m) {
      if (!s_cand[m]) continue;
      const unsigned km = s_key[m];
      before += (km > k || (km == k && m > n)) ? 1 : 0;
      equal_below += (km == k && m < n) ? 1 : 0;
    }
    // bounding-box diagonal x dist_thr (nms.py:255-260); a NaN coordinate makes the limit NaN as np.max / np.min do
    const float* row = p + (size_t)n * J * 5;
    float lo[3], hi[3];
    bool nan = false;
    for (int c = 0; c < 3; ++c) lo[c] = hi[c] = row[c];
    for (int j = 0; j < J; ++j)
      for (int c = 0; c < 3; ++c) {
        const float v = row[j * 5 + c];
        nan |= v != v;
        lo[c] = fminf(lo[c], v);
        hi[c] = fmaxf(hi[c], v);
      }
    const double sx = (double)hi[0] - (double)lo[0], sy = (double)hi[1] - (double)lo[1], sz = (double)hi[2] - (double)lo[2];
    const double diag = norm3(sx, sy, sz);
    ws.limit[before] = nan ? (double)NAN : diag * dist_thr;
    ws.rank2row[before] = n;
    ws.group_last[before] = before + equal_below;
    ws.key[before] = k;
  }
}

// ------------------------------------------------------------------------------------------------------------------------------
// (B) close[a][c] = #{ j : |k[a,j] - k[c,j]| < limit_a } > num_nearby_joints_thr, in rank space.  The limit belongs to the row.
__global__ __launch_bounds__(NMS_CLOSE_THREADS) void nms_close_kernel(const float* __restrict__ pred, void* workspace, int N, int J,
                                                                      int num_nearby_joints_thr) {
  extern __shared__ float s_pose[];           // columns [3J][64] (lane-contiguous), then rows [64][3J] (broadcast reads)
  const int b = blockIdx.z;
  const NmsWorkspace ws = nms_workspace(workspace, b, N);
  const int M = nms_candidates(ws, N);
  const int col0 = blockIdx.x * NMS_TILE, row0 = blockIdx.y * NMS_TILE;
  if (col0 >= M || row0 >= M) return;
  const int J3 = 3 * J;
  float* s_col = s_pose;
  float* s_row = s_pose + J3 * NMS_TILE;
  const float* p = pred + (size_t)b * N * J * 5;
  for (int e = threadIdx.x; e < NMS_TILE * J3; e += NMS_CLOSE_THREADS) {
    const int i = e / J3, jc = e - i * J3, j = jc / 3, c = jc - 3 * j;
    // ranks past M: zeros, never read into a result (their bits and rows are masked below)
    s_col[jc * NMS_TILE + i] = (col0 + i < M) ? p[((size_t)ws.rank2row[col0 + i] * J + j) * 5 + c] : 0.f;
    s_row[i * J3 + jc] = (row0 + i < M) ? p[((size_t)ws.rank2row[row0 + i] * J + j) * 5 + c] : 0.f;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool col_ok = col0 + lane < M;
  const size_t W = nms_words(N);
  for (int r = wave; r < NMS_TILE; r += NMS_CLOSE_THREADS / MVG_WAVE) {
    const int a = row0 + r;
    if (a >= M) break;                         // wave-uniform
    const double limit = ws.limit[a];
    const float* ra = s_row + r * J3;
    int near = 0;
    for (int j = 0; j < J; ++j) {
      const double dx = (double)ra[3 * j] - (double)s_col[(3 * j) * NMS_TILE + lane];
      const double dy = (double)ra[3 * j + 1] - (double)s_col[(3 * j + 1) * NMS_TILE + lane];
      const double dz = (double)ra[3 * j + 2] - (double)s_col[(3 * j + 2) * NMS_TILE + lane];
      near += (norm3(dx, dy, dz) < limit) ? 1 : 0;
    }
    const u64 word = __ballot(col_ok && near > num_nearby_joints_thr);
    if (lane == 0) ws.close[(size_t)a * W + blockIdx.x] = word;
  }
}

// ------------------------------------------------------------------------------------------------------------------------------
// (C) greedy pass in rank space, then max_dets and the outputs.
struct GreedyState {
  u64 ignored;        // this lane's word of the ignored mask
  int kept, skipped;  // wave-uniform
};

// one visit (nms.py:270-277); everything except `ignored` and `w` is wave-uniform
static __device__ __forceinline__ void nms_visit(GreedyState& st, int i, u64 w, int lane, const int* s_group_last, int* s_keep) {
  const u64 own = __shfl(st.ignored, i >> 6, MVG_WAVE);
  if ((own >> (i & 63)) & 1ull) return;
  const u64 has = __ballot(w != 0ull);
  if (has == 0ull) {                           // empty neighbourhood: counted, keeps nothing, suppresses nothing
    st.skipped += 1;
    return;
  }
  // best scored member; rank order is descending score with the HIGHER row first among equal scores, np.argmax takes the LOWER
  // row: the last set bit inside the run of equal scores that the first set bit belongs to
  const int l0 = __ffsll((long long)has) - 1;
  const u64 w0 = __shfl(w, l0, MVG_WAVE);
  const int r0 = l0 * 64 + (__ffsll((long long)w0) - 1);
  const int last = s_group_last[r0];
  int best = r0;
  if (last > r0) {
    const int from = max(r0 - lane * 64, 0), to = min(last - lane * 64, 63);
    const u64 in_run = (from > 63 || to < 0 || from > to) ? 0ull : (w & (~0ull << from) & (~0ull >> (63 - to)));
    const u64 has_run = __ballot(in_run != 0ull);
    const int l1 = 63 - __clzll((long long)has_run);
    const u64 w1 = __shfl(in_run, l1, MVG_WAVE);
    best = l1 * 64 + 63 - __clzll((long long)w1);
  }
  const u64 bw = __shfl(st.ignored, best >> 6, MVG_WAVE);
  if ((bw >> (best & 63)) & 1ull) return;
  if (lane == 0) s_keep[st.kept] = best;
  st.kept += 1;
  st.ignored |= w;
}

__global__ __launch_bounds__(NMS_GREEDY_THREADS) void nms_greedy_kernel(const float* __restrict__ pred, void* workspace, int N, int J,
                                                                        int max_dets, int* __restrict__ keep, int* __restrict__ count,
                                                                        float* __restrict__ dets, int dets_rows) {
  __shared__ int s_aux[NMS_MAX_N];            // group_last during the greedy pass, the score keys behind it
  __shared__ int s_keep[NMS_MAX_N];           // kept ranks in keep order
  __shared__ int s_sel[NMS_MAX_N];            // the max_dets selection
  __shared__ int s_cnt[2];
  const int b = blockIdx.x;
  const NmsWorkspace ws = nms_workspace(workspace, b, N);
  const int M = nms_candidates(ws, N);
  const int Wm = (M + 63) >> 6;
  const size_t W = nms_words(N);
  for (int r = threadIdx.x; r < M; r += NMS_GREEDY_THREADS) s_aux[r] = min(max(ws.group_last[r], r), M - 1);
  __syncthreads();
  if (threadIdx.x < MVG_WAVE) {
    const int lane = threadIdx.x;
    GreedyState st = {0ull, 0, 0};
    for (int i0 = 0; i0 < M; i0 += NMS_PREFETCH) {
      u64 w[NMS_PREFETCH];
#pragma unroll
      for (int u = 0; u < NMS_PREFETCH; ++u) w[u] = (i0 + u < M && lane < Wm) ? ws.close[(size_t)(i0 + u) * W + lane] : 0ull;
#pragma unroll
      for (int u = 0; u < NMS_PREFETCH; ++u)
        if (i0 + u < M) nms_visit(st, i0 + u, w[u], lane, s_aux, s_keep);
    }
    if (lane == 0) {
      s_cnt[0] = st.kept;
      s_cnt[1] = st.skipped;
    }
  }
  __syncthreads();
  const int K = min(s_cnt[0], M);
  int Kout = K;
  const int* sel = s_keep;
  if (max_dets > 0 && K > max_dets) {
    // the max_dets best scored kept poses in descending score, among equal scores the later keep position first
    // (np.argsort(scores[keep], kind="stable")[-1:-max_dets-1:-1]): position by counting
    for (int r = threadIdx.x; r < M; r += NMS_GREEDY_THREADS) s_aux[r] = (int)ws.key[r];
    __syncthreads();
    for (int q = threadIdx.x; q < K; q += NMS_GREEDY_THREADS) {
      const unsigned kq = (unsigned)s_aux[s_keep[q]];
      int pos = 0;
      for (int o = 0; o < K; ++o) {
        const unsigned ko = (unsigned)s_aux[s_keep[o]];
        pos += (ko > kq || (ko == kq && o > q)) ? 1 : 0;
      }
      if (pos < max_dets) s_sel[pos] = s_keep[q];
    }
    __syncthreads();
    Kout = max_dets;
    sel = s_sel;
  }
  if (threadIdx.x == 0) {
    count[2 * b] = Kout;
    count[2 * b + 1] = s_cnt[1];
  }
  for (int q = threadIdx.x; q < N; q += NMS_GREEDY_THREADS) keep[(size_t)b * N + q] = (q < Kout) ? ws.rank2row[sel[q]] : -1;
  if (dets != nullptr) {
    const int J5 = J * 5;
    const float* p = pred + (size_t)b * N * J5;
    float* d = dets + (size_t)b * dets_rows * J5;
    for (int e = threadIdx.x; e < dets_rows * J5; e += NMS_GREEDY_THREADS) {
      const int q = e / J5, c = e - q * J5;
      d[e] = (q < Kout) ? p[(size_t)ws.rank2row[sel[q]] * J5 + c] : ((c % 5 == 3) ? -1.f : 0.f);
    }
  }
}

extern "C" {

size_t mvg_pose_nms_workspace(int B, int N, int J) {
  if (B < 1 || N < 1 || N > NMS_MAX_N || J < 1 || J > NMS_MAX_J) return 0;
  return (size_t)B * nms_element_bytes(N);
}

int mvg_pose_nms(const float* pred, int B, int N, int J, double dist_thr, int num_nearby_joints_thr, int max_dets, void* workspace,
                 size_t workspace_bytes, int* keep, int* count, float* dets, int dets_rows, void* stream) {
  if (B < 1 || N < 1 || N > NMS_MAX_N || J < 1 || J > NMS_MAX_J) return MVG_E_BADARG;
  if (!(dist_thr > 0.0) || num_nearby_joints_thr < 0 || num_nearby_joints_thr >= J) return MVG_E_BADARG;
  if (B > 65535 || (dets != nullptr && (dets_rows < 1 || dets_rows > NMS_MAX_N))) return MVG_E_BADARG;
  if (mvg_any_null({pred, keep, count, workspace}) || mvg_any_misaligned(8, {workspace})) return MVG_E_BADARG;
  if (workspace_bytes < mvg_pose_nms_workspace(B, N, J)) return MVG_E_BADARG;
  const int tiles = mvg_ceil_div(N, NMS_TILE);
  const size_t lds = (size_t)2 * NMS_TILE * 3 * J * sizeof(float);
  hipLaunchKernelGGL(nms_rank_kernel, dim3(B), dim3(NMS_RANK_THREADS), 0, (hipStream_t)stream, pred, workspace, N, J, dist_thr);
  MVG_LAUNCH_CHECK();
  hipLaunchKernelGGL(nms_close_kernel, dim3(tiles, tiles, B), dim3(NMS_CLOSE_THREADS), lds, (hipStream_t)stream, pred, workspace, N, J,
                     num_nearby_joints_thr);
  MVG_LAUNCH_CHECK();
  hipLaunchKernelGGL(nms_greedy_kernel, dim3(B), dim3(NMS_GREEDY_THREADS), 0, (hipStream_t)stream, pred, workspace, N, J, max_dets,
                     keep, count, dets, dets_rows);
  MVG_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
