// Structural triangulation for gfx950 (mvg_structural_triangulate): a person's J joints re-solved from their 2D observations in V
// views under fixed bone lengths (the reference's lib/structural/), one launch, ONE wavefront (= one workgroup of 64 threads) per
// person, fp64.  Fixed shapes, nothing read back, no atomics, every element with one writer: bit-reproducible, independent of
// the other persons of the launch, capturable in a HIP graph behind mvg_pose_nms.
//
// The contract -- operation for operation -- is in include/mvg_decoder.h; tests/st_ref.py restates it in numpy.  In short, with
// n = 3 (J - 1) and K = J - 1:
//   1. lane i < J:   D_i (3 x 3, symmetric) and m_i of joint i, views in ascending order.
//   2. tree sums T, mu, C_k, cm_k (a lane per entry, joints ascending); T^-1; W_k = T^-1 C_k, tm = T^-1 mu; the lower triangle of
//      A (n x n) and beta, an entry per lane and pass.
//   3. Inv = A^-1 through the Cholesky factor; b = Inv beta (lane r: row r).
//   4. ST: n_steps times  S (K x K, lower), its Cholesky factor, lambda by two substitutions, the lower triangle of
//      Inv - Inv diag(2 lambda) Inv mirrored into the other LDS matrix (the two swap roles), b = Inv beta.
//   5. the root from T^-1, the joints by the tree sums (lane i < J), one rounding to fp32.
//
// Factorisations: Cholesky, column by column (j ascending): lane i >= j forms s_i = M[i][j] - sum_{k<j ascending} L[i][k] L[j][k];
// the pivot s_j must be > 0 (a NaN is not), d = sqrt(s_j), L[j][j] = d, L[i][j] = s_i / d.  The inverse: lane c solves
// L y = e_c downwards from row c (Y = L^-1, lower), then Inv[r][c] = sum_{k = r ascending}^{n-1} Y[k][r] Y[k][c] for c <= r, written
// to both triangles.  Every sum is formed by one lane in ascending index order from +0.0, every product is rounded on its own
// (through f64_mul_nv: see CONTRACTION in exact_dev.h; this file has no product outside it that feeds an add), sqrt
// and division are correctly rounded.  Every loop is counted; a failed pivot ends the person (status 1 or 2), wave-uniformly.
//
// LDS: two n x n fp64 matrices with a row stride of 49 (odd: a column walk touches all banks) = 2 x 18.4 KB, plus ~7 KB of small
// tables (45.3 KB in all): three persons a CU by LDS.
#include <math.h>

#include "exact_dev.h"

#define ST_THREADS MVG_WAVE
#define ST_MAXJ MVG_ST_MAX_J
#define ST_MAXK (ST_MAXJ - 1)
#define ST_MAXN (3 * ST_MAXK)
#define ST_LD (ST_MAXN + 1)
#define ST_SLD (ST_MAXK + 1)

static_assert(ST_MAXN <= ST_THREADS, "a lane per row of the reduced system");
static_assert(ST_MAXJ <= 32, "ancestor sets are 32-bit masks");

struct StTree {
  unsigned anc[ST_MAXJ];      // bit k of anc[i]: bone k (the one that ends at joint k >= 1) lies on the path root -> i
};

// entry e of a lower triangle stored row by row: e = r (r + 1) / 2 + c, c <= r
static __device__ __forceinline__ void st_tri(int e, int& r, int& c) {
  int g = (int)((sqrtf(8.f * (float)e + 1.f) - 1.f) * 0.5f);
  if (g * (g + 1) / 2 > e) --g;
  if ((g + 1) * (g + 2) / 2 <= e) ++g;
  r = g;
  c = e - g * (g + 1) / 2;
}

// In place on the lower triangle of M (n x n, row stride ld); uniform result, false at the first pivot that is not > 0.  The
// caller has a barrier in front; a barrier follows every column.
static __device__ bool st_chol(double* M, int n, int ld, int lane) {
  for (int j = 0; j < n; ++j) {
    double s = 0.0;
    if (lane >= j && lane < n) {
      s = M[lane * ld + j];
      for (int k = 0; k < j; ++k) s = s - f64_mul_nv(M[lane * ld + k], M[j * ld + k]);
    }
    const double piv = lane_of(s, j);
    if (!(piv > 0.0)) return false;
    const double d = __builtin_sqrt(piv);
    if (lane == j) M[j * ld + j] = d;
    else if (lane > j && lane < n) M[lane * ld + j] = s / d;
    __syncthreads();
  }
  return true;
}

// Lm: a Cholesky factor (lower); Y <- Lm^-1 (lower triangle only); Inv <- Y^T Y, both triangles.  Inv may be Lm.
static __device__ void st_inverse(const double* Lm, double* Y, double* Inv, int n, int lane) {
  if (lane < n) {
    const int c = lane;
    for (int i = c; i < n; ++i) {
      double s = i == c ? 1.0 : 0.0;
      for (int k = c; k < i; ++k) s = s - f64_mul_nv(Lm[i * ST_LD + k], Y[k * ST_LD + c]);
      Y[i * ST_LD + c] = s / Lm[i * ST_LD + i];
    }
  }
  __syncthreads();
  for (int e = lane; e < n * (n + 1) / 2; e += ST_THREADS) {
    int r, c;
    st_tri(e, r, c);
    double acc = 0.0;
    for (int k = r; k < n; ++k) acc = acc + f64_mul_nv(Y[k * ST_LD + r], Y[k * ST_LD + c]);
    Inv[r * ST_LD + c] = acc;
    Inv[c * ST_LD + r] = acc;
  }
  __syncthreads();
}

__global__ __launch_bounds__(ST_THREADS) void structural_kernel(const float* __restrict__ ud, const float* __restrict__ conf,
                                                                const float* __restrict__ Pm, const uint8_t* __restrict__ valid,
                                                                const int* __restrict__ rows, int rows_ld,
                                                                const int* __restrict__ count, StTree tree,
                                                                const float* __restrict__ bone_len, int per_person, int method,
                                                                int n_steps, float* __restrict__ X, int* __restrict__ status, int V,
                                                                int NQ, int P, int J) {
  __shared__ double s_m0[ST_MAXN * ST_LD];
  __shared__ double s_m1[ST_MAXN * ST_LD];
  __shared__ double s_D[ST_MAXJ][12];          // D_i row-major in 0..8, m_i in 9..11
  __shared__ double s_C[ST_MAXK][12];          // C_k, cm_k of bone k + 1
  __shared__ double s_W[ST_MAXK][9];           // T^-1 C_k
  __shared__ double s_T[12];                   // T, mu
  __shared__ double s_Tinv[9];
  __shared__ double s_tm[3];
  __shared__ double s_beta[ST_MAXN];
  __shared__ double s_b[ST_MAXN];
  __shared__ double s_S[ST_MAXK * ST_SLD];
  __shared__ double s_lam[ST_MAXK];
  __shared__ double s_x0[3];

  const int lane = threadIdx.x;
  const int b = blockIdx.x / P, p = blockIdx.x % P;
  const int K = J - 1, n = 3 * K;
  float* Xo = X + (size_t)blockIdx.x * J * 3;

  // which query, if any (wave-uniform)
  int q = -1;
  if (rows != nullptr) {
    const int live = det_rows(count, b, P);
    if (p < live) q = rows[(size_t)b * rows_ld + p];
  } else if (valid == nullptr || valid[(size_t)b * NQ + p] != 0) {
    q = p;
  }
  if (q < 0 || q >= NQ) {
    if (lane < J * 3) Xo[lane] = 0.f;
    if (lane == 0) status[blockIdx.x] = -1;
    return;
  }

  // 1. the quadratic of joint `lane`
  if (lane < J) {
    double D00 = 0.0, D01 = 0.0, D02 = 0.0, D11 = 0.0, D12 = 0.0, D22 = 0.0, m0 = 0.0, m1 = 0.0, m2 = 0.0;
    const double cdef = 1.0 / (double)V;
    for (int v = 0; v < V; ++v) {
      const size_t tok = ((size_t)b * V + v) * ((size_t)NQ * J) + (size_t)q * J + lane;
      const float* Pv = Pm + ((size_t)b * V + v) * 12;
      const double u = (double)ud[tok * 2], w = (double)ud[tok * 2 + 1];
      const double c2 = 2.0 * (conf == nullptr ? cdef : (double)conf[tok]);
      const double r20 = (double)Pv[8], r21 = (double)Pv[9], r22 = (double)Pv[10], t2 = (double)Pv[11];
      const double g00 = (double)Pv[0] - f64_mul_nv(u, r20), g01 = (double)Pv[1] - f64_mul_nv(u, r21);
      const double g02 = (double)Pv[2] - f64_mul_nv(u, r22);
      const double g10 = (double)Pv[4] - f64_mul_nv(w, r20), g11 = (double)Pv[5] - f64_mul_nv(w, r21);
      const double g12 = (double)Pv[6] - f64_mul_nv(w, r22);
      const double h0 = (double)Pv[3] - f64_mul_nv(u, t2), h1 = (double)Pv[7] - f64_mul_nv(w, t2);
      D00 = D00 + f64_mul_nv(c2, f64_mul_nv(g00, g00) + f64_mul_nv(g10, g10));
      D01 = D01 + f64_mul_nv(c2, f64_mul_nv(g00, g01) + f64_mul_nv(g10, g11));
      D02 = D02 + f64_mul_nv(c2, f64_mul_nv(g00, g02) + f64_mul_nv(g10, g12));
      D11 = D11 + f64_mul_nv(c2, f64_mul_nv(g01, g01) + f64_mul_nv(g11, g11));
      D12 = D12 + f64_mul_nv(c2, f64_mul_nv(g01, g02) + f64_mul_nv(g11, g12));
      D22 = D22 + f64_mul_nv(c2, f64_mul_nv(g02, g02) + f64_mul_nv(g12, g12));
      m0 = m0 - f64_mul_nv(c2, f64_mul_nv(g00, h0) + f64_mul_nv(g10, h1));
      m1 = m1 - f64_mul_nv(c2, f64_mul_nv(g01, h0) + f64_mul_nv(g11, h1));
      m2 = m2 - f64_mul_nv(c2, f64_mul_nv(g02, h0) + f64_mul_nv(g12, h1));
    }
    double* d = s_D[lane];
    d[0] = D00; d[1] = D01; d[2] = D02;
    d[3] = D01; d[4] = D11; d[5] = D12;
    d[6] = D02; d[7] = D12; d[8] = D22;
    d[9] = m0; d[10] = m1; d[11] = m2;
  }
  __syncthreads();

  // 2. tree sums: entry e of T | mu and of every C_k | cm_k, joints in ascending order
  if (lane < 12) {
    double acc = 0.0;
    for (int i = 0; i < J; ++i) acc = acc + s_D[i][lane];
    s_T[lane] = acc;
  }
  for (int w = lane; w < K * 12; w += ST_THREADS) {
    const int k = w / 12 + 1, e = w % 12;
    double acc = 0.0;
    for (int i = 0; i < J; ++i)
      if ((tree.anc[i] >> k) & 1u) acc = acc + s_D[i][e];
    s_C[k - 1][e] = acc;
  }
  __syncthreads();
  if (lane < 9) s_m0[(lane / 3) * ST_LD + lane % 3] = s_T[lane];      // T goes through the same factorisation as A, at n = 3
  __syncthreads();
  bool ok = st_chol(s_m0, 3, ST_LD, lane);
  if (ok) {
    st_inverse(s_m0, s_m1, s_m0, 3, lane);
    if (lane < 9) s_Tinv[lane] = s_m0[(lane / 3) * ST_LD + lane % 3];
    __syncthreads();
    for (int w = lane; w < K * 9; w += ST_THREADS) {
      const int k = w / 9, a = (w % 9) / 3, c = w % 3;
      double acc = 0.0;
      for (int t = 0; t < 3; ++t) acc = acc + f64_mul_nv(s_Tinv[a * 3 + t], s_C[k][t * 3 + c]);
      s_W[k][a * 3 + c] = acc;
    }
    if (lane < 3) {
      double acc = 0.0;
      for (int t = 0; t < 3; ++t) acc = acc + f64_mul_nv(s_Tinv[lane * 3 + t], s_T[9 + t]);
      s_tm[lane] = acc;
    }
    __syncthreads();
    for (int e = lane; e < n * (n + 1) / 2; e += ST_THREADS) {
      int r, c;
      st_tri(e, r, c);
      const int k = r / 3 + 1, a = r % 3, l = c / 3 + 1, bb = c % 3;
      double base = 0.0;
      if ((tree.anc[l] >> k) & 1u) base = s_C[l - 1][a * 3 + bb];
      else if ((tree.anc[k] >> l) & 1u) base = s_C[k - 1][a * 3 + bb];
      double acc = 0.0;
      for (int t = 0; t < 3; ++t) acc = acc + f64_mul_nv(s_C[k - 1][a * 3 + t], s_W[l - 1][t * 3 + bb]);
      s_m0[r * ST_LD + c] = base - acc;
    }
    if (lane < n) {
      const int k = lane / 3, a = lane % 3;
      double acc = 0.0;
      for (int t = 0; t < 3; ++t) acc = acc + f64_mul_nv(s_C[k][a * 3 + t], s_tm[t]);
      s_beta[lane] = s_C[k][9 + a] - acc;
    }
    __syncthreads();
    ok = st_chol(s_m0, n, ST_LD, lane);
  }
  if (!ok) {
    if (lane < J * 3) Xo[lane] = 0.f;
    if (lane == 0) status[blockIdx.x] = 1;
    return;
  }

  // 3. Inv = A^-1 (in s_m0), b = Inv beta
  st_inverse(s_m0, s_m1, s_m0, n, lane);
  double* Inv = s_m0;
  double* Alt = s_m1;
  if (lane < n) {
    double acc = 0.0;
    for (int c = 0; c < n; ++c) acc = acc + f64_mul_nv(Inv[lane * ST_LD + c], s_beta[c]);
    s_b[lane] = acc;
  }
  __syncthreads();

  // 4. the constrained steps
  int stat = 0;
  if (method == MVG_ST_ST) {
    for (int s = 0; s < n_steps; ++s) {
      double rhs = 0.0;
      if (lane < K) {
        const double b0 = s_b[3 * lane], b1 = s_b[3 * lane + 1], b2 = s_b[3 * lane + 2];
        const double start = __builtin_sqrt((f64_mul_nv(b0, b0) + f64_mul_nv(b1, b1)) + f64_mul_nv(b2, b2));
        const double len = (double)bone_len[per_person ? (size_t)blockIdx.x * K + lane : (size_t)lane];
        const double target = (f64_mul_nv(start, (double)(n_steps - s - 1)) + len) / (double)(n_steps - s);
        rhs = (f64_mul_nv(start, start) - f64_mul_nv(target, target)) / 4.0;
      }
      for (int e = lane; e < K * (K + 1) / 2; e += ST_THREADS) {
        int k, l;
        st_tri(e, k, l);
        double acc = 0.0;
        for (int a = 0; a < 3; ++a) {
          double t = 0.0;
          for (int c = 0; c < 3; ++c) t = t + f64_mul_nv(Inv[(3 * k + a) * ST_LD + 3 * l + c], s_b[3 * l + c]);
          acc = acc + f64_mul_nv(s_b[3 * k + a], t);
        }
        s_S[k * ST_SLD + l] = acc;
      }
      __syncthreads();
      if (!st_chol(s_S, K, ST_SLD, lane)) {
        stat = 2;
        break;
      }
      // lambda = S^-1 rhs: lane i holds rhs_i; y downwards, lambda upwards, one lane at a time
      for (int i = 0; i < K; ++i) {
        if (lane == i) {
          double acc = rhs;
          for (int k = 0; k < i; ++k) acc = acc - f64_mul_nv(s_S[i * ST_SLD + k], s_lam[k]);
          s_lam[i] = acc / s_S[i * ST_SLD + i];
        }
        __syncthreads();
      }
      const double y = lane < K ? s_lam[lane] : 0.0;
      __syncthreads();
      for (int i = K - 1; i >= 0; --i) {
        if (lane == i) {
          double acc = y;
          for (int k = i + 1; k < K; ++k) acc = acc - f64_mul_nv(s_S[k * ST_SLD + i], s_lam[k]);
          s_lam[i] = acc / s_S[i * ST_SLD + i];
        }
        __syncthreads();
      }
      for (int e = lane; e < n * (n + 1) / 2; e += ST_THREADS) {
        int r, c;
        st_tri(e, r, c);
        double acc = 0.0;
        for (int j = 0; j < n; ++j)
          acc = acc + f64_mul_nv(f64_mul_nv(Inv[r * ST_LD + j], 2.0 * s_lam[j / 3]), Inv[j * ST_LD + c]);
        const double val = Inv[r * ST_LD + c] - acc;
        Alt[r * ST_LD + c] = val;
        Alt[c * ST_LD + r] = val;
      }
      __syncthreads();
      double* swap = Inv;
      Inv = Alt;
      Alt = swap;
      if (lane < n) {
        double acc = 0.0;
        for (int c = 0; c < n; ++c) acc = acc + f64_mul_nv(Inv[lane * ST_LD + c], s_beta[c]);
        s_b[lane] = acc;
      }
      __syncthreads();
    }
  }

  // 5. the root, then the joints along the tree
  if (lane < 3) {
    double qa = 0.0;
    for (int j = 0; j < n; ++j) qa = qa + f64_mul_nv(s_C[j / 3][lane * 3 + j % 3], s_b[j]);
    s_x0[lane] = s_T[9 + lane] - qa;          // mu - q, T^-1 applied below
  }
  __syncthreads();
  if (lane < J) {
    for (int a = 0; a < 3; ++a) {
      double x = 0.0;
      for (int t = 0; t < 3; ++t) x = x + f64_mul_nv(s_Tinv[a * 3 + t], s_x0[t]);
      for (int k = 1; k < J; ++k)
        if ((tree.anc[lane] >> k) & 1u) x = x + s_b[3 * (k - 1) + a];
      Xo[lane * 3 + a] = (float)x;
    }
  }
  if (lane == 0) status[blockIdx.x] = stat;
}

extern "C" {

int mvg_structural_triangulate(const float* ud, const float* conf, const float* Pm, const uint8_t* valid, const int* rows, int rows_ld,
                               const int* count, const int* parent_host, const float* bone_len, int bone_len_per_person, int method,
                               int n_steps, float* X, int* status, int V, int B, int NQ, int P, int J, void* stream) {
  if (J < 2 || J > MVG_ST_MAX_J || V < 1 || V > MVG_ST_MAX_V || B < 1 || NQ < 1 || P < 1) return MVG_E_BADARG;
  if ((long long)B * P > 0x7fffffffLL || (long long)NQ * J > 0x7fffffffLL) return MVG_E_BADARG;
  if (method != MVG_ST_LS && method != MVG_ST_ST) return MVG_E_BADARG;
  if (n_steps < 1 || n_steps > MVG_ST_MAX_STEPS) return MVG_E_BADARG;
  if (mvg_any_null({ud, Pm, X, status, parent_host})) return MVG_E_BADARG;
  if (method == MVG_ST_ST && bone_len == nullptr) return MVG_E_BADARG;
  if (rows != nullptr && (valid != nullptr || rows_ld < P)) return MVG_E_BADARG;
  if (rows == nullptr && (count != nullptr || P != NQ)) return MVG_E_BADARG;
  // the tree: joint 0 is the root, every other joint reaches it in fewer than J steps
  StTree tree;
  if (parent_host[0] != -1) return MVG_E_BADARG;
  for (int i = 0; i < ST_MAXJ; ++i) tree.anc[i] = 0u;
  for (int i = 1; i < J; ++i)
    if (parent_host[i] < 0 || parent_host[i] >= J || parent_host[i] == i) return MVG_E_BADARG;
  for (int i = 1; i < J; ++i) {
    int j = i;
    for (int step = 0; step < J && j != 0; ++step) {
      tree.anc[i] |= 1u << j;
      j = parent_host[j];
    }
    if (j != 0) return MVG_E_BADARG;
  }
  hipLaunchKernelGGL(structural_kernel, dim3((unsigned)(B * P)), dim3(ST_THREADS), 0, (hipStream_t)stream, ud, conf, Pm, valid, rows,
                     rows_ld, count, tree, bone_len, bone_len_per_person, method, n_steps, X, status, V, NQ, P, J);
  MVG_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
