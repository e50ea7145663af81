// Person identities across frames for gfx950: a minimum-cost assignment solver on one wavefront (mvg_linear_assignment) and the
// tracker update built on it (mvg_track_update), which associates the poses mvg_pose_nms keeps with the tracks of the frames
// before.  Fixed shapes, nothing read back, no host synchronisation: the update sits behind the NMS in the HIP graph of the
// decoder forward and the host reads the tracks when it wants them.
//
//   mvg_linear_assignment   1 launch, one workgroup of ONE wavefront per batch element: the costs go to LDS, lane j owns column j
//                           (its potential v, minv, way, used flag and assigned row) and row j (its potential u); the only
//                           cross-lane operation of a search step is the minimum of minv with its column (DPP moves inside the
//                           rows of 16 lanes, v_readlane across them, a ballot for the column); wave-uniform lanes are read
//                           with v_readlane.
//   mvg_track_update        1 launch, one workgroup (256 threads) per batch element = stream: ordered compaction of the detection
//                           rows (LDS scan), the active slots (one ballot), the track x detection mean joint distances by all
//                           threads into LDS, the solve on wavefront 0, then matches / misses / deaths (a lane per track),
//                           births (thread 0, in detection order), pose copies and the per-row outputs by all threads.
//   mvg_track_predict,      the optional constant-velocity motion model, 1 launch each around the unchanged update, one workgroup
//   mvg_track_correct       per stream: a Kalman filter per track (position and velocity per joint and axis, one 2 x 2 covariance
//                           per track); the update then associates against predicted poses.  No LDS, no atomics.
//   mvg_track_eval          the scoring of the ids against ground truth, 1 launch behind the tracker, one workgroup per stream: the
//                           same compaction, the person x hypothesis distances into the same LDS tile, the kept correspondences of
//                           CLEAR-MOT (a lane per person), the rest on the same solve, counters and the identity overlap table for
//                           IDF1.  Every element of its state has one writer: no atomics.
//
// The solver is the shortest-augmenting-path Hungarian algorithm with potentials, rows inserted in order, stated so that a host
// restatement gives the same bits (include/mvg_decoder.h): the per-column operations of a step are independent and are executed
// unchanged by the column's lane; the minimum is taken under a total order (value, NaN as +inf, then column), so the shape of
// the reduction does not matter.  Every loop is counted: no input, NaN included, can make a search spin.
//
// Arithmetic: fp64 from the fp32 inputs, sqrt((x^2 + y^2) + z^2) with a correctly rounded sqrt, joints summed in joint order.
// CONTRACTION in exact_dev.h says which products are rounded on their own: the distances of track_update_kernel are dist3, the
// FUSED form; those of track_eval_kernel are dist3_exact and the motion model goes through f64_mul, exact for every input.  The
// only atomics are integer adds on the state block, whose sums do not depend on the order of the workgroups: two runs give
// the same bits.
#include <math.h>

#include "exact_dev.h"

#define LAP_N MVG_LAP_MAX_N
#define LAP_VIRT LAP_N                // the virtual column a row's search starts from
#define TRACK_THREADS 256

static_assert(LAP_N == MVG_WAVE, "a lane per column");
static_assert(TRACK_THREADS == SCAN_THREADS, "track_update_kernel and track_eval_kernel call scan_rows; the others only share it");
static_assert(MVG_TRACK_MAX_D == LAP_N && MVG_TRACK_MAX_T == LAP_N, "tracks and detections are the solver's rows and columns");

enum { TS_FRAMES = 0, TS_MATCHES = 1, TS_BIRTHS = 2, TS_DEATHS = 3, TS_OVERFLOW = 4, TS_DROPPED = 5, TS_ACTIVE = 6, TS_TICKET = 7 };

struct LapPlain {
  __device__ __forceinline__ double operator()(double c) const { return c; }
};
// the tracker's gate: a pair further apart than max_dist, or with a NaN distance, costs what a non-match costs
struct LapGate {
  double max_dist;
  __device__ __forceinline__ double operator()(double c) const { return c <= max_dist ? c : max_dist; }
};

// cross-lane move of a double inside a row of 16 lanes: two 32-bit halves through the DPP network (lane_of of exact_dev.h reads
// from a lane whose index is wave-uniform)
template <int CTRL>
static __device__ __forceinline__ double lap_dpp(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
static __device__ __forceinline__ double lap_min(double a, double b) { return b < a ? b : a; }

// Executed by ONE whole wavefront in uniform control flow.  s_raw: LDS, row stride LAP_N, entries (i < n, j < m) valid; the square
// matrix of the solve is S[i, j] = clamp(f(s_raw[i, j])) there and 0 elsewhere, of size s = max(n, m).  s_col[r] (LDS, LAP_N
// entries) <- the column of row r, -1 for a row that is dead (r >= n) or assigned to a padding column; the caller puts a
// barrier between this call and its reads of s_col.
template <class F>
static __device__ void lap_solve(const double* s_raw, int n, int m, F f, int* s_col, int lane) {
  const int s = max(n, m);
  double u = 0.0, v = 0.0;            // potentials of row `lane` and of column `lane`
  int p = -1;                          // row assigned to column `lane`
  for (int i = 0; i < s; ++i) {
    double minv = (double)INFINITY;
    int way = LAP_VIRT;
    bool used = false, rowused = false;
    int j0 = LAP_VIRT, i0 = i;
    bool found = false;
    for (int step = 0; step < s; ++step) {        // every step uses one more column and at most i are assigned: <= i + 1 steps
      if (lane == j0) used = true;
      if (lane == i0) rowused = true;
      const double ui0 = lane_of(u, i0);
      const bool cand = lane < s && !used;
      if (cand) {
        double sv = 0.0;
        if (i0 < n && lane < m) {
          sv = f(s_raw[i0 * LAP_N + lane]);
          if (sv != sv || sv > MVG_LAP_BIG) sv = MVG_LAP_BIG;
        }
        const double cur = (sv - ui0) - v;
        if (cur < minv) {
          minv = cur;
          way = j0;
        }
      }
      // minimum of minv over the unused columns, lowest column among equals; NaN ordered as +inf, so that without a finite
      // minimum the lowest unused column is taken.  The value first (lane ^ 1, lane ^ 2, the mirrors of 8 and 16 lanes, then
      // the four rows), then the lowest unused lane that holds it.
      const double key = (cand && minv == minv) ? minv : (double)INFINITY;
      double kmin = key;
      kmin = lap_min(kmin, lap_dpp<0xB1>(kmin));
      kmin = lap_min(kmin, lap_dpp<0x4E>(kmin));
      kmin = lap_min(kmin, lap_dpp<0x141>(kmin));
      kmin = lap_min(kmin, lap_dpp<0x140>(kmin));
      kmin = lap_min(lap_min(lane_of(kmin, 0), lane_of(kmin, 16)), lap_min(lane_of(kmin, 32), lane_of(kmin, 48)));
      const u64 holders = __ballot(cand && key == kmin);
      if (holders == 0) break;                     // not reachable: an unused column exists while the search runs
      const int j1 = __builtin_ctzll(holders);
      const double delta = lane_of(minv, j1);
      if (rowused) u += delta;
      if (lane < s) {
        if (used) v -= delta;
        else minv -= delta;
      }
      j0 = j1;
      const int pj0 = lane_of(p, j0);
      if (pj0 < 0) {
        found = true;
        break;
      }
      i0 = pj0;
    }
    if (!found) continue;                          // not reachable: the counted loop above always ends on a free column
    for (int k = 0; k <= s; ++k) {                 // flip the path back to the virtual column: <= i + 1 links
      const int j1 = lane_of(way, j0);
      const int pj1 = j1 == LAP_VIRT ? i : lane_of(p, j1 & (LAP_N - 1));
      if (lane == j0) p = pj1;
      j0 = j1;
      if (j0 == LAP_VIRT) break;
    }
  }
  s_col[lane] = -1;
  if (p >= 0 && p < n && lane < m) s_col[p] = lane;
}

// ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LAP_N) void linear_assignment_kernel(const double* __restrict__ cost, const int* __restrict__ n_live,
                                                                  const int* __restrict__ m_live, int N, int M,
                                                                  int* __restrict__ col_of_row, double* __restrict__ total) {
  __shared__ double s_raw[LAP_N * LAP_N];
  __shared__ int s_col[LAP_N];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int n = n_live == nullptr ? N : clamp_count(n_live[b], N);
  const int m = m_live == nullptr ? M : clamp_count(m_live[b], M);
  const double* c = cost + (size_t)b * N * M;
  for (int e = lane; e < n * m; e += LAP_N) s_raw[(e / m) * LAP_N + (e % m)] = c[(size_t)(e / m) * M + (e % m)];
  __syncthreads();
  lap_solve(s_raw, n, m, LapPlain(), s_col, lane);
  __syncthreads();
  if (lane < N) col_of_row[(size_t)b * N + lane] = s_col[lane];
  if (lane == 0) {
    double sum = 0.0;                              // the entries of the input as given, in row order
    for (int r = 0; r < n; ++r)
      if (s_col[r] >= 0) sum += s_raw[r * LAP_N + s_col[r]];
    total[b] = sum;
  }
}

// ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TRACK_THREADS) void track_update_kernel(const float* __restrict__ dets, const int* __restrict__ count,
                                                                     int B, int R, int J, int T, int* __restrict__ id,
                                                                     int* __restrict__ hits, int* __restrict__ misses,
                                                                     i64* __restrict__ born, float* __restrict__ score,
                                                                     float* pose, int* __restrict__ next_id, i64* state,
                                                                     double max_dist, int max_misses, int min_hits,
                                                                     int* __restrict__ ids, int* __restrict__ slots) {
  __shared__ double s_c[LAP_N * LAP_N];        // ungated mean joint distance of (active track a, detection d)
  __shared__ int s_scan[2][1][SCAN_THREADS];
  __shared__ int s_det[LAP_N];                 // row of detection d
  __shared__ int s_trk[LAP_N];                 // slot of active track a
  __shared__ int s_col[LAP_N];                 // detection assigned to active track a, or -1
  __shared__ int s_det_slot[LAP_N];            // slot of the track detection d belongs to after this frame, or -1
  __shared__ int s_id[LAP_N], s_hits[LAP_N];   // per slot, as they stand after this frame
  __shared__ int s_na, s_matches, s_deaths, s_births, s_overflow;
  __shared__ i64 s_frame;
  const int b = blockIdx.x, t = threadIdx.x;
  if (t == 0) s_frame = __hip_atomic_load(&state[TS_FRAMES], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);

  // detections: the rows in front of count[b, 0] whose flag is >= 0, in row order
  const int rows = det_rows(count, b, R);
  const auto is_det = [=](int i) { return i < rows && det_flag(dets, b, i, R, J); };
  const RowScan<1> run = scan_rows<1>(R, s_scan, [=](int i, int* n) { n[0] += is_det(i) ? 1 : 0; });
  const int lo = run.lo, hi = run.hi;
  const int first = run.before(0);             // detections in front of this thread's run
  const int nd_all = run.total(0);
  const int nd = min(nd_all, MVG_TRACK_MAX_D);
  {
    int pos = first;
    for (int i = lo; i < hi && pos < MVG_TRACK_MAX_D; ++i)
      if (is_det(i)) s_det[pos++] = i;
  }
  // active tracks: the slots with id >= 0, in slot order
  if (t < LAP_N) {
    const int tid = t < T ? id[(size_t)b * T + t] : -1;
    const u64 mask = __ballot(tid >= 0);
    if (tid >= 0) s_trk[__popcll(mask & ((1ull << t) - 1ull))] = t;
    s_id[t] = tid;
    s_hits[t] = t < T ? hits[(size_t)b * T + t] : 0;
    s_det_slot[t] = -1;
    if (t == 0) s_na = __popcll(mask);
  }
  __syncthreads();
  const int na = s_na;

  for (int e = t; e < na * nd; e += TRACK_THREADS) {
    const int a = e / nd, d = e % nd;
    const float* p = pose + ((size_t)b * T + s_trk[a]) * J * 3;
    const float* g = dets + ((size_t)b * R + s_det[d]) * J * 5;
    double sum = 0.0;
    for (int j = 0; j < J; ++j) sum += dist3(p + j * 3, g + j * 5);
    s_c[a * LAP_N + d] = sum / (double)J;
  }
  __syncthreads();
  if (t < LAP_N) lap_solve(s_c, na, nd, LapGate{max_dist}, s_col, t);      // wavefront 0
  __syncthreads();

  // matched tracks take the detection; the others age and die
  if (t < LAP_N) {
    bool matched = false, died = false;
    if (t < na) {
      const int slot = s_trk[t], d = s_col[t];
      const size_t at = (size_t)b * T + slot;
      matched = d >= 0 && s_c[t * LAP_N + d] <= max_dist;               // the ungated cost: NaN is no match
      if (matched) {
        s_det_slot[d] = slot;
        misses[at] = 0;
        hits[at] = s_hits[slot] + 1;
        s_hits[slot] += 1;
      } else {
        const int ms = misses[at] + 1;
        misses[at] = ms;
        died = ms > max_misses;
        if (died) {
          id[at] = -1;
          s_id[slot] = -1;
        }
      }
    }
    const u64 m_mask = __ballot(matched), d_mask = __ballot(died);
    if (t == 0) {
      s_matches = __popcll(m_mask);
      s_deaths = __popcll(d_mask);
    }
  }
  __syncthreads();
  // unmatched detections open tracks in detection order, each in the lowest free slot (those freed above included)
  if (t == 0) {
    u64 free_slots = 0;
    for (int k = 0; k < T; ++k)
      if (s_id[k] < 0) free_slots |= 1ull << k;
    int nid = next_id[b], births = 0, overflow = 0;
    for (int d = 0; d < nd; ++d) {
      if (s_det_slot[d] >= 0) continue;
      if (free_slots == 0) {
        ++overflow;
        continue;
      }
      const int slot = __builtin_ctzll(free_slots);
      free_slots &= free_slots - 1;
      const size_t at = (size_t)b * T + slot;
      s_det_slot[d] = slot;
      s_id[slot] = nid;
      s_hits[slot] = 1;
      id[at] = nid++;
      hits[at] = 1;
      misses[at] = 0;
      born[at] = s_frame;
      ++births;
    }
    next_id[b] = nid;
    s_births = births;
    s_overflow = overflow;
  }
  __syncthreads();
  // the pose (bit for bit) and the score of every detection that has a track now
  for (int e = t; e < nd * J * 3; e += TRACK_THREADS) {
    const int d = e / (J * 3), k = e % (J * 3);
    const int slot = s_det_slot[d];
    if (slot >= 0) pose[((size_t)b * T + slot) * J * 3 + k] = dets[((size_t)b * R + s_det[d]) * J * 5 + (k / 3) * 5 + (k % 3)];
  }
  if (t < nd && s_det_slot[t] >= 0) score[(size_t)b * T + s_det_slot[t]] = dets[((size_t)b * R + s_det[t]) * J * 5 + 4];
  // per row: the slot, and the id once the track has min_hits hits
  {
    int pos = first;
    for (int i = lo; i < hi; ++i) {
      int slot = -1, tid = -1;
      if (is_det(i)) {
        if (pos < MVG_TRACK_MAX_D) {
          slot = s_det_slot[pos];
          if (slot >= 0 && s_hits[slot] >= min_hits) tid = s_id[slot];
        }
        ++pos;
      }
      ids[(size_t)b * R + i] = tid;
      slots[(size_t)b * R + i] = slot;
    }
  }
  // the state block: integer sums over the elements, then the last element of the call to arrive advances the frame counter
  // (every element has read it by then: thread 0 loaded it before anything else and has used it since)
  if (t == 0) {
    u64* st = (u64*)state;
    if (s_matches) atomicAdd(&st[TS_MATCHES], (u64)s_matches);
    if (s_births) atomicAdd(&st[TS_BIRTHS], (u64)s_births);
    if (s_deaths) atomicAdd(&st[TS_DEATHS], (u64)s_deaths);
    if (s_overflow) atomicAdd(&st[TS_OVERFLOW], (u64)s_overflow);
    if (nd_all > nd) atomicAdd(&st[TS_DROPPED], (u64)(nd_all - nd));
    if (s_births != s_deaths) atomicAdd(&st[TS_ACTIVE], (u64)(i64)(s_births - s_deaths));
    __threadfence();
    if (atomicAdd(&st[TS_TICKET], 1ull) == (u64)(B - 1)) {
      atomicExch(&st[TS_TICKET], 0ull);
      atomicAdd(&st[TS_FRAMES], 1ull);
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------------------
// The constant-velocity motion model around the update.  One workgroup per stream, threads striding over the T * J * 3 coordinates
// of its slots; a slot's three covariance entries belong to the thread of its first coordinate.  Each operation below is one
// rounded fp64 operation, in the order of include/mvg_decoder.h: a product that feeds an add goes through f64_mul (exact_dev.h).

__global__ __launch_bounds__(TRACK_THREADS) void track_predict_kernel(int T, int J, const int* __restrict__ id, float* __restrict__ pose,
                                                                      double* __restrict__ mean, double* __restrict__ var, double dt,
                                                                      double q) {
  const int b = blockIdx.x, J3 = J * 3;
  const double dt2 = dt * dt;
  const double dt3 = dt2 * dt, dt4 = dt2 * dt2;
  const double qxx = (q * dt4) / 4.0, qxv = (q * dt3) / 2.0, qvv = q * dt2;
  for (int e = threadIdx.x; e < T * J3; e += TRACK_THREADS) {
    const int t = e / J3, k = e % J3;
    const size_t slot = (size_t)b * T + t;
    if (id[slot] < 0) continue;
    double* m = mean + (slot * J + k / 3) * 6 + k % 3;       // m[0] position, m[3] velocity of this joint and axis
    const double x = m[0] + f64_mul(m[3], dt);
    m[0] = x;
    pose[slot * J3 + k] = (float)x;
    if (k == 0) {
      double* p = var + slot * 3;
      const double pxx = p[0], pxv = p[1], pvv = p[2];
      p[0] = ((pxx + f64_mul(2.0 * dt, pxv)) + f64_mul(dt2, pvv)) + qxx;
      p[1] = (pxv + f64_mul(dt, pvv)) + qxv;
      p[2] = pvv + qvv;
    }
  }
}

// var is read by every thread of a slot and written by one: the writes come behind a barrier, in a second pass.  The rows then
// read the poses the first pass wrote, behind the same barrier (the stream's slots and rows belong to this workgroup alone).
__global__ __launch_bounds__(TRACK_THREADS) void track_correct_kernel(int R, int T, int J, const int* __restrict__ id,
                                                                      const int* __restrict__ hits, const int* __restrict__ misses,
                                                                      const int* __restrict__ slots, float* pose,
                                                                      double* __restrict__ mean, double* var, double r, double v0,
                                                                      float* __restrict__ row_pose) {
  const int b = blockIdx.x, J3 = J * 3;
  for (int e = threadIdx.x; e < T * J3; e += TRACK_THREADS) {
    const int t = e / J3, k = e % J3;
    const size_t slot = (size_t)b * T + t;
    double* m = mean + (slot * J + k / 3) * 6 + k % 3;
    if (id[slot] < 0) {                                        // free
      m[0] = 0.0;
      m[3] = 0.0;
    } else if (misses[slot] > 0) {                             // missed: the prediction stands
    } else if (hits[slot] == 1) {                              // born in this call
      m[0] = (double)pose[slot * J3 + k];
      m[3] = 0.0;
    } else {                                                   // matched: pose holds the detection
      const double pxx = var[slot * 3], pxv = var[slot * 3 + 1];
      const double s = pxx + r;
      const double kx = pxx / s, kv = pxv / s;
      double x = m[0], v = m[3];
      const double d = (double)pose[slot * J3 + k] - x;
      x = x + f64_mul(kx, d);
      v = v + f64_mul(kv, d);
      m[0] = x;
      m[3] = v;
      pose[slot * J3 + k] = (float)x;
    }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < T; t += TRACK_THREADS) {
    const size_t slot = (size_t)b * T + t;
    double* p = var + slot * 3;
    if (id[slot] < 0) {
      p[0] = 0.0;
      p[1] = 0.0;
      p[2] = 0.0;
    } else if (misses[slot] > 0) {
    } else if (hits[slot] == 1) {
      p[0] = r;
      p[1] = 0.0;
      p[2] = v0;
    } else {
      const double pxx = p[0], pxv = p[1], pvv = p[2];
      const double s = pxx + r;
      const double kx = pxx / s, kv = pxv / s;
      p[2] = pvv - f64_mul(kv, pxv);
      p[1] = (1.0 - kx) * pxv;
      p[0] = (1.0 - kx) * pxx;
    }
  }
  for (int e = threadIdx.x; e < R * J3; e += TRACK_THREADS) {
    const int slot = slots[(size_t)b * R + e / J3];
    row_pose[(size_t)b * R * J3 + e] = (slot >= 0 && slot < T) ? pose[((size_t)b * T + slot) * J3 + e % J3] : 0.f;
  }
}

// ------------------------------------------------------------------------------------------------------------------------------
// CLEAR-MOT counts and the identity overlap table of one frame (mvg_track_eval, the rules of include/mvg_decoder.h).  One workgroup
// per stream; every element of the state is written by that workgroup alone, with plain loads and stores: no atomics.
enum { TE_FRAMES = 0, TE_GT, TE_HYP, TE_MATCHES, TE_MISSES, TE_FALSE_POS, TE_SWITCHES, TE_KEPT, TE_DROPPED, TE_UNREPORTED, TE_BAD_ID,
       TE_ID_OVERFLOW, TE_RESERVED };
#define TE_GATHER (LAP_N * LAP_N / TRACK_THREADS)      // entries of the distance tile per thread

static_assert(MVG_TRACK_EVAL_WORDS == TE_RESERVED + 1, "the counters of include/mvg_decoder.h");
static_assert(MVG_TRACK_EVAL_MAX_P == LAP_N, "persons are the solver's rows");
static_assert(TE_GATHER * TRACK_THREADS == LAP_N * LAP_N, "the tile is compacted through TE_GATHER registers per thread");

__global__ __launch_bounds__(TRACK_THREADS) void track_eval_kernel(const float* __restrict__ dets, const int* __restrict__ count,
                                                                   const int* __restrict__ ids, const float* __restrict__ row_pose,
                                                                   const float* __restrict__ joints_3d, const float* __restrict__ vis,
                                                                   const int* __restrict__ num_person,
                                                                   const int* __restrict__ person_id, int R, int J, int G, int P,
                                                                   int K, double thr, int* __restrict__ last_track,
                                                                   i64* __restrict__ counters, double* __restrict__ dist_sum,
                                                                   i64* __restrict__ seen, i64* __restrict__ covered,
                                                                   int* __restrict__ overlap) {
  __shared__ double s_d[LAP_N * LAP_N];        // d[person a, hypothesis h]; from step 6 on: the remaining pairs, compacted
  __shared__ double s_pd[LAP_N];               // distance of person a's match
  __shared__ int s_scan[2][2][SCAN_THREADS];   // [hypotheses, unreported rows]; from step 6 on: the id_overflow counts
  __shared__ int s_row[LAP_N], s_hid[LAP_N];   // row and id of hypothesis h
  __shared__ int s_slot[LAP_N], s_pid[LAP_N];  // slot and identity of person a
  __shared__ int s_ph[LAP_N];                  // hypothesis matched to person a, or -1
  __shared__ int s_taken[LAP_N];               // hypothesis h is matched
  __shared__ int s_rp[LAP_N], s_rh[LAP_N];     // the remaining persons / hypotheses
  __shared__ int s_col[LAP_N];
  __shared__ int s_np, s_bad, s_nrp, s_nrh;
  const int b = blockIdx.x, t = threadIdx.x;
  const int annotated = num_person[b];
  if (annotated < 0) return;                   // the whole workgroup: a frame without annotation

  // hypotheses: the detection rows that carry an id, in row order; the detection rows without one are only counted
  const int rows = det_rows(count, b, R);
  const auto is_det = [=](int i) { return i < rows && det_flag(dets, b, i, R, J); };
  const RowScan<2> run = scan_rows<2>(R, s_scan, [=](int i, int* n) {
    if (is_det(i)) {
      if (ids[(size_t)b * R + i] >= 0) ++n[0];
      else ++n[1];
    }
  });
  const int nh_all = run.total(0), unreported = run.total(1);
  const int nh = min(nh_all, MVG_TRACK_MAX_D);
  {
    int pos = run.before(0);
    for (int i = run.lo; i < run.hi && pos < MVG_TRACK_MAX_D; ++i)
      if (is_det(i) && ids[(size_t)b * R + i] >= 0) {
        s_row[pos] = i;
        s_hid[pos++] = ids[(size_t)b * R + i];
      }
  }
  // persons: a lane per slot; an identity out of range or already taken by a lower slot is a bad id
  if (t < LAP_N) {
    bool live = false;
    int p = -1;
    if (t < min(annotated, G)) {
      const float* w = vis + ((size_t)b * G + t) * J;
      for (int j = 0; j < J; ++j) live = live || w[j] > 0.f;
      p = person_id == nullptr ? t : person_id[(size_t)b * G + t];
    }
    const int pin = (live && p >= 0 && p < P) ? p : -1;
    bool twice = false;
    for (int k = 0; k < LAP_N; ++k) {
      const int pk = lane_of(pin, k);
      twice = twice || (k < t && pk >= 0 && pk == pin);
    }
    const bool ok = pin >= 0 && !twice;
    const u64 ok_mask = __ballot(ok), bad_mask = __ballot(live && !ok);
    if (ok) {
      const int a = __popcll(ok_mask & ((1ull << t) - 1ull));
      s_slot[a] = t;
      s_pid[a] = pin;
    }
    s_ph[t] = -1;
    s_taken[t] = 0;
    if (t == 0) {
      s_np = __popcll(ok_mask);
      s_bad = __popcll(bad_mask);
    }
  }
  __syncthreads();
  const int np = s_np;

  const int hs = row_pose == nullptr ? 5 : 3;                                   // floats per joint of a hypothesis' pose
  const float* hyp = row_pose == nullptr ? dets + (size_t)b * R * J * 5 : row_pose + (size_t)b * R * J * 3;
  for (int e = t; e < np * nh; e += TRACK_THREADS) {
    const int a = e / nh, h = e % nh;
    const float* x = hyp + (size_t)s_row[h] * J * hs;
    const float* g = joints_3d + ((size_t)b * G + s_slot[a]) * J * 3;
    const float* w = vis + ((size_t)b * G + s_slot[a]) * J;
    double sum = 0.0;
    int n = 0;
    for (int j = 0; j < J; ++j)
      if (w[j] > 0.f) {
        sum += dist3_exact(x + j * hs, g + j * 3);       // summed into dist_sum, compared bit for bit
        ++n;
      }
    s_d[a * LAP_N + h] = sum / (double)n;                                       // n >= 1: a person has a visible joint
  }
  __syncthreads();

  // step 5 on wavefront 0, a lane per person: the hypothesis that carries the person's last id; among the persons that could keep
  // the same hypothesis the lowest slot does
  int kept = 0;
  if (t < LAP_N) {
    int cand = -1;
    double d = 0.0;
    if (t < np) {
      const int last = last_track[(size_t)b * P + s_pid[t]];
      if (last >= 0)
        for (int h = 0; h < nh; ++h)
          if (cand < 0 && s_hid[h] == last) cand = h;
      if (cand >= 0) {
        d = s_d[t * LAP_N + cand];
        if (!(d <= thr)) cand = -1;
      }
    }
    bool keep = cand >= 0;
    for (int k = 0; k < LAP_N; ++k) {
      const int ck = lane_of(cand, k);
      if (k < t && ck >= 0 && ck == cand) keep = false;
    }
    if (keep) {
      s_ph[t] = cand;
      s_taken[cand] = 1;
      s_pd[t] = d;
    }
    kept = __popcll(__ballot(keep));
  }
  // step 9 by all threads, from the full tile
  int over = 0;
  for (int e = t; e < np * nh; e += TRACK_THREADS) {
    const int a = e / nh, h = e % nh;
    if (s_d[a * LAP_N + h] <= thr) {
      const int tid = s_hid[h];
      if (tid < K) overlap[((size_t)b * P + s_pid[a]) * K + tid] += 1;
      else ++over;
    }
  }
  __syncthreads();

  // step 6: the remaining persons x hypotheses, compacted in place through registers, then the solve on wavefront 0
  if (t < LAP_N) {
    const bool rp = t < np && s_ph[t] < 0, rh = t < nh && s_taken[t] == 0;
    const u64 rp_mask = __ballot(rp), rh_mask = __ballot(rh);
    if (rp) s_rp[__popcll(rp_mask & ((1ull << t) - 1ull))] = t;
    if (rh) s_rh[__popcll(rh_mask & ((1ull << t) - 1ull))] = t;
    if (t == 0) {
      s_nrp = __popcll(rp_mask);
      s_nrh = __popcll(rh_mask);
    }
  }
  s_scan[0][0][t] = over;                        // `run` was last read barriers ago: the per-thread id_overflow counts
  __syncthreads();
  const int nrp = s_nrp, nrh = s_nrh;
  double moved[TE_GATHER];
#pragma unroll
  for (int k = 0; k < TE_GATHER; ++k) {
    const int e = t + k * TRACK_THREADS;
    moved[k] = e < nrp * nrh ? s_d[s_rp[e / nrh] * LAP_N + s_rh[e % nrh]] : 0.0;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < TE_GATHER; ++k) {
    const int e = t + k * TRACK_THREADS;
    if (e < nrp * nrh) s_d[(e / nrh) * LAP_N + e % nrh] = moved[k];
  }
  __syncthreads();
  if (t < LAP_N) lap_solve(s_d, nrp, nrh, LapGate{thr}, s_col, t);
  __syncthreads();
  if (t < nrp) {
    const int j = s_col[t];
    if (j >= 0 && s_d[t * LAP_N + j] <= thr) {                                  // the ungated distance: NaN is no match
      s_ph[s_rp[t]] = s_rh[j];
      s_pd[s_rp[t]] = s_d[t * LAP_N + j];
    }
  }
  __syncthreads();

  // steps 7 and 8 on wavefront 0: a lane per person (the identities are distinct), the distance sum and the counters by lane 0
  if (t < LAP_N) {
    bool matched = false, switched = false;
    if (t < np) {
      const size_t at = (size_t)b * P + s_pid[t];
      seen[at] += 1;
      matched = s_ph[t] >= 0;
      if (matched) {
        const int tid = s_hid[s_ph[t]], last = last_track[at];
        covered[at] += 1;
        switched = last >= 0 && last != tid;
        last_track[at] = tid;
      }
    }
    const int matches = __popcll(__ballot(matched)), switches = __popcll(__ballot(switched));
    int overflow = (s_scan[0][0][t] + s_scan[0][0][t + LAP_N]) + (s_scan[0][0][t + 2 * LAP_N] + s_scan[0][0][t + 3 * LAP_N]);
    for (int off = LAP_N / 2; off > 0; off >>= 1) overflow += __shfl_xor(overflow, off);
    if (t == 0) {
      double sum = dist_sum[b];
      for (int a = 0; a < np; ++a)
        if (s_ph[a] >= 0) sum = sum + s_pd[a];
      dist_sum[b] = sum;
      i64* c = counters + (size_t)b * MVG_TRACK_EVAL_WORDS;
      c[TE_FRAMES] += 1;
      c[TE_GT] += np;
      c[TE_HYP] += nh;
      c[TE_MATCHES] += matches;
      c[TE_MISSES] += np - matches;
      c[TE_FALSE_POS] += nh - matches;
      c[TE_SWITCHES] += switches;
      c[TE_KEPT] += kept;
      c[TE_DROPPED] += nh_all - nh;
      c[TE_UNREPORTED] += unreported;
      c[TE_BAD_ID] += s_bad;
      c[TE_ID_OVERFLOW] += overflow;
    }
  }
}

static bool track_noise_ok(double v, bool zero_ok) { return (zero_ok ? v >= 0.0 : v > 0.0) && v <= MVG_LAP_BIG; }   // false for NaN

extern "C" {

int mvg_track_predict(int B, int T, int J, const int* id, float* pose, double* mean, double* var, double dt, double q, void* stream) {
  if (B < 1 || B > MVG_TRACK_MAX_B || T < 1 || T > MVG_TRACK_MAX_T || J < 1 || J > MVG_TRACK_MAX_J) return MVG_E_BADARG;
  if (mvg_any_null({id, pose, mean, var}) || mvg_any_misaligned(8, {mean, var})) return MVG_E_BADARG;
  if (!(dt > 0.0) || !(dt <= 1.79769313486231570815e+308) || !track_noise_ok(q, true)) return MVG_E_BADARG;
  hipLaunchKernelGGL(track_predict_kernel, dim3(B), dim3(TRACK_THREADS), 0, (hipStream_t)stream, T, J, id, pose, mean, var, dt, q);
  MVG_LAUNCH_CHECK();
  return 0;
}

int mvg_track_correct(int B, int R, int T, int J, const int* id, const int* hits, const int* misses, const int* slots, float* pose,
                      double* mean, double* var, double r, double v0, float* row_pose, void* stream) {
  if (B < 1 || B > MVG_TRACK_MAX_B || R < 1 || R > MVG_TRACK_MAX_R || J < 1 || J > MVG_TRACK_MAX_J || T < 1 || T > MVG_TRACK_MAX_T)
    return MVG_E_BADARG;
  if (mvg_any_null({id, hits, misses, slots, pose, mean, var, row_pose}) || mvg_any_misaligned(8, {mean, var})) return MVG_E_BADARG;
  if (!track_noise_ok(r, false) || !track_noise_ok(v0, true)) return MVG_E_BADARG;
  hipLaunchKernelGGL(track_correct_kernel, dim3(B), dim3(TRACK_THREADS), 0, (hipStream_t)stream, R, T, J, id, hits, misses, slots, pose,
                     mean, var, r, v0, row_pose);
  MVG_LAUNCH_CHECK();
  return 0;
}

int mvg_linear_assignment(const double* cost, const int* n, const int* m, int B, int N, int M, int* col_of_row, double* total,
                          void* stream) {
  if (B < 1 || B > MVG_TRACK_MAX_B || N < 1 || N > MVG_LAP_MAX_N || M < 1 || M > MVG_LAP_MAX_N) return MVG_E_BADARG;
  if (mvg_any_null({cost, col_of_row, total}) || mvg_any_misaligned(8, {cost, total})) return MVG_E_BADARG;
  hipLaunchKernelGGL(linear_assignment_kernel, dim3(B), dim3(LAP_N), 0, (hipStream_t)stream, cost, n, m, N, M, col_of_row, total);
  MVG_LAUNCH_CHECK();
  return 0;
}

int mvg_track_update(const float* dets, const int* count, int B, int R, int J, int T, int* id, int* hits, int* misses, int64_t* born,
                     float* score, float* pose, int* next_id, int64_t* state, double max_dist, int max_misses, int min_hits,
                     int* ids, int* slots, void* stream) {
  if (B < 1 || B > MVG_TRACK_MAX_B || R < 1 || R > MVG_TRACK_MAX_R || J < 1 || J > MVG_TRACK_MAX_J || T < 1 || T > MVG_TRACK_MAX_T)
    return MVG_E_BADARG;
  if (!(max_dist >= 0.0) || max_dist > MVG_LAP_BIG || max_misses < 0 || min_hits < 0) return MVG_E_BADARG;
  if (mvg_any_null({dets, id, hits, misses, born, score, pose, next_id, state, ids, slots})) return MVG_E_BADARG;
  if (mvg_any_misaligned(8, {born, state})) return MVG_E_BADARG;
  hipLaunchKernelGGL(track_update_kernel, dim3(B), dim3(TRACK_THREADS), 0, (hipStream_t)stream, dets, count, B, R, J, T, id, hits,
                     misses, (i64*)born, score, pose, next_id, (i64*)state, max_dist, max_misses, min_hits, ids, slots);
  MVG_LAUNCH_CHECK();
  return 0;
}

int mvg_track_eval(const float* dets, const int* count, const int* ids, const float* row_pose, const float* joints_3d,
                   const float* joints_3d_vis, const int* num_person, const int* person_id, int B, int R, int J, int G, int P, int K,
                   double dist_thr, int* last_track, int64_t* counters, double* dist_sum, int64_t* seen, int64_t* covered,
                   int* overlap, void* stream) {
  if (B < 1 || B > MVG_TRACK_MAX_B || R < 1 || R > MVG_TRACK_MAX_R || J < 1 || J > MVG_TRACK_MAX_J) return MVG_E_BADARG;
  if (G < 1 || P < G || P > MVG_TRACK_EVAL_MAX_P || K < 1 || K > MVG_TRACK_EVAL_MAX_K) return MVG_E_BADARG;
  if (!(dist_thr >= 0.0) || dist_thr > MVG_LAP_BIG) return MVG_E_BADARG;
  if (mvg_any_null({dets, ids, joints_3d, joints_3d_vis, num_person, last_track, counters, dist_sum, seen, covered, overlap}))
    return MVG_E_BADARG;
  if (mvg_any_misaligned(8, {counters, dist_sum, seen, covered})) return MVG_E_BADARG;
  hipLaunchKernelGGL(track_eval_kernel, dim3(B), dim3(TRACK_THREADS), 0, (hipStream_t)stream, dets, count, ids, row_pose, joints_3d,
                     joints_3d_vis, num_person, person_id, R, J, G, P, K, dist_thr, last_track, (i64*)counters, dist_sum, (i64*)seen,
                     (i64*)covered, overlap);
  MVG_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
