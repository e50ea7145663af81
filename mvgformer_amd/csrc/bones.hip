// Per-track bone lengths for gfx950 (mvg_track_bones): the tracker says which row is which person from frame to frame, a person's
// bones do not change, so every track slot keeps a ring of the bone lengths of its last W detections and their median feeds the
// structural refiner (mvg_structural_triangulate, per-person lengths) instead of one skeleton for everybody.  One launch per
// frame behind mvg_track_update (and mvg_track_correct), one workgroup (256 threads) per stream, fixed shapes, nothing read back,
// NO atomics, every element with one writer, every loop counted: bit-reproducible, capturable in a HIP graph.
//
// The contract -- operation for operation -- is in include/mvg_decoder.h; tests/bones_ref.py restates it in numpy.  In short:
//   1. ownership   a lane per slot: a slot whose id is no longer its owner's forgets its history.
//   2. sample      the lowest detection row of every slot.  Thread t owns a run of consecutive rows (as scan_rows of exact_dev.h
//                  splits them) and forms the 64-bit mask of the slots its run names; an OR scan over the threads (LDS, ping-pong)
//                  gives the slots that lower runs name; the thread walks its run again and takes, in row order, the slots that
//                  are still free.  One writer per slot, no atomics, the lowest row wins.  Then a thread per (slot, bone): the
//                  lengths by dist3_exact from the raw detection, the ring store if all of them are finite.
//   3. estimate    the same thread per (slot, bone): the ring's n <= 32 samples go to registers, the median is selected by rank
//                  counting (n x 32 compares, no sort).  The slots' lengths live in LDS for step 4.
//   4. rows        a thread per row: the slot's length, the fallback or the row's own lengths, and where they came from.
// hist is read from global memory (up to 131 KB per stream): only the rings of the slots that took a sample are touched.
#include <math.h>

#include "exact_dev.h"

#define BONES_THREADS 256
#define BONES_MAXT MVG_TRACK_MAX_T
#define BONES_MAXK (MVG_ST_MAX_J - 1)
#define BONES_SEEN_CAP (1 << 30)

static_assert(BONES_MAXT <= 64, "the slots a run of rows names are a 64-bit mask");
static_assert(BONES_MAXT <= BONES_THREADS, "a thread per slot");

struct BonesTree {
  int parent[MVG_ST_MAX_J];
};

static __device__ __forceinline__ bool bones_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// the length of the bone that ends at joint k of a dets row (J, 5), one rounding to fp32
static __device__ __forceinline__ float bone_of(const float* g, const BonesTree& tree, int k) {
  return (float)dist3_exact(g + k * 5, g + tree.parent[k] * 5);
}

__global__ __launch_bounds__(BONES_THREADS) void track_bones_kernel(const float* __restrict__ dets, const int* __restrict__ count,
                                                                    const int* __restrict__ slots, const int* __restrict__ id,
                                                                    BonesTree tree, int R, int J, int T, int W, int min_frames,
                                                                    const float* __restrict__ fallback, int* __restrict__ owner,
                                                                    int* __restrict__ seen, float* hist, float* __restrict__ length,
                                                                    float* __restrict__ row_length, int* __restrict__ row_source) {
  __shared__ u64 s_or[2][BONES_THREADS];             // the OR scan of the runs' slot masks
  __shared__ float s_len[BONES_MAXT][BONES_MAXK];    // the sample of slot t
  __shared__ float s_length[BONES_MAXT][BONES_MAXK]; // length[b, t, :] as it stands after this call
  __shared__ int s_row[BONES_MAXT];                  // the row slot t samples, or -1
  __shared__ int s_seen[BONES_MAXT];                 // seen[b, t] in front of the sample
  __shared__ int s_now[BONES_MAXT];                  // and behind it
  __shared__ int s_fresh[BONES_MAXT];                // the slot changed hands
  const int b = blockIdx.x, t = threadIdx.x, K = J - 1;

  // 1. ownership
  if (t < BONES_MAXT) {
    s_row[t] = -1;
    int sn = 0, fresh = 0;
    if (t < T) {
      const size_t at = (size_t)b * T + t;
      const int tid = id[at];
      fresh = tid != owner[at];
      if (fresh) owner[at] = tid;
      else sn = seen[at];
    }
    s_seen[t] = sn;
    s_now[t] = sn;
    s_fresh[t] = fresh;
  }
  __syncthreads();
  for (int e = t; e < T * K; e += BONES_THREADS) {
    const int slot = e / K, k = e % K;
    s_length[slot][k] = s_fresh[slot] ? 0.f : length[((size_t)b * T + slot) * K + k];
  }

  // 2. the lowest detection row of every slot
  const int rows = det_rows(count, b, R);
  const auto slot_of = [=](int i) {                  // the slot a detection row names, else -1
    if (i >= rows) return -1;
    const int s = slots[(size_t)b * R + i];
    return (s >= 0 && s < T && det_flag(dets, b, i, R, J)) ? s : -1;
  };
  const int chunk = (R + BONES_THREADS - 1) / BONES_THREADS;
  const int lo = min(t * chunk, R), hi = min(lo + chunk, R);
  u64 named = 0;
  for (int i = lo; i < hi; ++i) {
    const int s = slot_of(i);
    if (s >= 0) named |= 1ull << s;
  }
  s_or[0][t] = named;
  __syncthreads();
  int src = 0;
  for (int step = 1; step < BONES_THREADS; step <<= 1) {
    s_or[src ^ 1][t] = s_or[src][t] | (t >= step ? s_or[src][t - step] : 0ull);
    src ^= 1;
    __syncthreads();
  }
  u64 taken = t > 0 ? s_or[src][t - 1] : 0ull;       // by the runs in front of this one
  if ((named & ~taken) != 0)
    for (int i = lo; i < hi; ++i) {
      const int s = slot_of(i);
      if (s >= 0 && !((taken >> s) & 1ull)) {
        s_row[s] = i;
        taken |= 1ull << s;
      }
    }
  __syncthreads();
  for (int e = t; e < T * K; e += BONES_THREADS) {
    const int slot = e / K, k = e % K;
    const int row = s_row[slot];
    if (row >= 0) s_len[slot][k] = bone_of(dets + ((size_t)b * R + row) * J * 5, tree, k + 1);
  }
  __syncthreads();
  if (t < T) {
    bool take = s_row[t] >= 0;
    if (take)
      for (int k = 0; k < K; ++k) take = take && bones_finite(s_len[t][k]);
    if (take) s_now[t] = min(s_seen[t] + 1, BONES_SEEN_CAP);
    else s_row[t] = -1;
    seen[(size_t)b * T + t] = s_now[t];
  }
  __syncthreads();

  // the ring store, and 3. the median of the ring for the slots that took a sample; every length written
  for (int e = t; e < T * K; e += BONES_THREADS) {
    const int slot = e / K, k = e % K;
    if (s_row[slot] >= 0) {
      const float mine = s_len[slot][k];
      const int pos = s_seen[slot] % W, n = min(s_now[slot], W);
      float* ring = hist + ((size_t)b * T + slot) * W * K + k;      // entry w at ring[w * K]
      ring[(size_t)pos * K] = mine;
      float v[MVG_BONES_MAX_W];
#pragma unroll
      for (int j = 0; j < MVG_BONES_MAX_W; ++j) v[j] = j < n ? (j == pos ? mine : ring[(size_t)j * K]) : 0.f;
      const int r_lo = (n - 1) >> 1, r_hi = n >> 1;
      float m_lo = 0.f, m_hi = 0.f;
      for (int i = 0; i < n; ++i) {
        const float vi = i == pos ? mine : ring[(size_t)i * K];
        int rank = 0;
#pragma unroll
        for (int j = 0; j < MVG_BONES_MAX_W; ++j) rank += (j < n && (v[j] < vi || (v[j] == vi && j < i))) ? 1 : 0;
        if (rank == r_lo) m_lo = vi;
        if (rank == r_hi) m_hi = vi;
      }
      s_length[slot][k] = (n & 1) ? m_lo : (float)(((double)m_lo + (double)m_hi) * 0.5);
    }
    length[((size_t)b * T + slot) * K + k] = s_length[slot][k];
  }
  __syncthreads();

  // 4. the rows
  for (int i = t; i < R; i += BONES_THREADS) {
    float* out = row_length + ((size_t)b * R + i) * K;
    int source = -1;
    if (i < rows && det_flag(dets, b, i, R, J)) {
      const int s = slots[(size_t)b * R + i];
      if (s >= 0 && s < T && s_now[s] >= min_frames) {
        source = 0;
        for (int k = 0; k < K; ++k) out[k] = s_length[s][k];
      } else if (fallback != nullptr) {
        source = 1;
        for (int k = 0; k < K; ++k) out[k] = fallback[k];
      } else {
        source = 2;
        const float* g = dets + ((size_t)b * R + i) * J * 5;
        for (int k = 0; k < K; ++k) out[k] = bone_of(g, tree, k + 1);
      }
    } else {
      for (int k = 0; k < K; ++k) out[k] = 0.f;
    }
    row_source[(size_t)b * R + i] = source;
  }
}

extern "C" {

int mvg_track_bones(const float* dets, const int* count, const int* slots, const int* id, const int* parent_host, int B, int R, int J,
                    int T, int W, int min_frames, const float* fallback, int* owner, int* seen, float* hist, float* length,
                    float* row_length, int* row_source, void* stream) {
  if (B < 1 || B > MVG_TRACK_MAX_B || R < 1 || R > MVG_TRACK_MAX_R || T < 1 || T > MVG_TRACK_MAX_T) return MVG_E_BADARG;
  if (J < 2 || J > MVG_ST_MAX_J || W < 1 || W > MVG_BONES_MAX_W || min_frames < 1) return MVG_E_BADARG;
  if (mvg_any_null({dets, slots, id, parent_host, owner, seen, hist, length, row_length, row_source})) return MVG_E_BADARG;
  // the tree of mvg_structural_triangulate: joint 0 is the root, every other joint reaches it in fewer than J steps
  BonesTree tree;
  if (parent_host[0] != -1) return MVG_E_BADARG;
  for (int i = 0; i < MVG_ST_MAX_J; ++i) tree.parent[i] = 0;
  for (int i = 1; i < J; ++i) {
    if (parent_host[i] < 0 || parent_host[i] >= J || parent_host[i] == i) return MVG_E_BADARG;
    tree.parent[i] = parent_host[i];
  }
  for (int i = 1; i < J; ++i) {
    int j = i;
    for (int step = 0; step < J && j != 0; ++step) j = parent_host[j];
    if (j != 0) return MVG_E_BADARG;
  }
  hipLaunchKernelGGL(track_bones_kernel, dim3((unsigned)B), dim3(BONES_THREADS), 0, (hipStream_t)stream, dets, count, slots, id, tree, R,
                     J, T, W, min_frames, fallback, owner, seen, hist, length, row_length, row_source);
  MVG_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
