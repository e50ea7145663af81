// Query self-attention of the decoder layer (init_self_attention, dq_decoder.py:281-283,532-539): softmax attention of the Lq
// tokens of one batch element against each other, 8 heads of width 32, flash-style -- no Lq x Lq matrix in memory, an online
// softmax with a running maximum and sum per query row.
//
// One workgroup = 4 wavefronts = 128 query rows of one (head, batch element); a wavefront owns 32 rows.  Keys / values arrive in
// tiles of 64 rows, staged once per workgroup through LDS (two buffers, one barrier per tile; the next tile's global loads are in
// flight under the current tile's products).  Both products keep the QUERY on the lane:
//   S^T (key, query) = K Q^T     A = K tile (from LDS), B = Q (registers, loaded once)
//   O^T (d,   query) = V^T P^T   A = V^T (from LDS),    B = the S^T accumulator itself (an accumulator tile is the next
//                                                          product's B operand with no lane movement)
// so a lane holds 16 of the 32 scores of ITS query per 32-key block, the row maximum is 31 max + one exchange with lane ^ 32, the
// rescale factor and the row sum are lane-local, and nothing but K and V ever touches LDS.
//
// Arithmetic.  c = log2(e) / sqrt(32).  Scores, maximum, sum and rescale are fp32; p = exp2((s - m) c) with m the running
// maximum of the RAW scores (c > 0).  c is applied to the fp32 score (one fma per score in the bf16 variant, exactly the cost of
// the subtraction it replaces) instead of being folded into an operand: a rescaled bf16 Q would be rounded a second time, which
// at |score| = 80 moves a probability by 17 %.
//   bf16: Q, K, V bf16, products on v_mfma_f32_32x32x16_bf16 with fp32 accumulation; P is rounded to bf16 only as the operand of
//         P V (the row sum adds the unrounded fp32 p); O is rounded to bf16 once, after the division by the row sum.
//   fp32: Q, K, V fp32, products on v_mfma_f32_32x32x2_f32: a k-ordered fp32 fma chain, one rounding per product -- the
//         reference's arithmetic class at every input range (no split operands, hence no validity range to state); P stays fp32.
// Fixed reduction order (tiles ascending, one writer per output element, no atomics): results are bit-identical from run to run
// and do not depend on the other batch elements.  Finite inputs only: a NaN / Inf in Q, K or V spreads over the rows that read it.
// Rows whose scores are all equal, and score magnitudes far beyond +-80, stay finite: every exponent is <= 0 (bf16: up to the
// rounding of m c, 2^-24 |m c|) and the maximum's own term is 1 (to that rounding), so the row sum lies in [1, Lq].
#include "common.h"

namespace mha {

constexpr int ROWS = 128;       // query rows per workgroup (4 wavefronts x 32)
constexpr int KT = 64;          // keys per tile
constexpr int THREADS = 256;
constexpr int D = 32, C = 256, M = 8;

// LDS images of one tile.  bf16: K row-major (pitch 80 B: conflict-free 16-B reads), V transposed [d][key] (pitch 136 B).
// fp32: K and V row-major (pitch 144 B).
constexpr int KP16 = 40, VP16 = 68;                       // pitches in bf16 elements
constexpr int KP32 = 36;                                  // pitch in floats
constexpr int BUF16 = KT * KP16 * 2 + D * VP16 * 2;       // 9472 B
constexpr int BUF32 = 2 * KT * KP32 * 4;                  // 18432 B

template <bool BF> struct Stage;

template <> struct Stage<true> {
  uint4 k, v;
  __device__ __forceinline__ void load(const void* K, const void* V, long ldk, long ldv, int key0, int Lq, int t) {
    const int key = t >> 2, ch = t & 3, g = key0 + key;
    k = v = uint4{0u, 0u, 0u, 0u};
    if (g < Lq) {
      k = *reinterpret_cast<const uint4*>(reinterpret_cast<const bf16_t*>(K) + g * ldk + 8 * ch);
      v = *reinterpret_cast<const uint4*>(reinterpret_cast<const bf16_t*>(V) + g * ldv + 8 * ch);
    }
  }
  __device__ __forceinline__ void store(char* buf, int t) const {
    const int key = t >> 2, ch = t & 3;
    bf16_t* ks = reinterpret_cast<bf16_t*>(buf);
    bf16_t* vt = ks + KT * KP16;
    *reinterpret_cast<uint4*>(ks + key * KP16 + 8 * ch) = k;
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      vt[(8 * ch + 2 * i) * VP16 + key] = (bf16_t)(w[i] & 0xffffu);
      vt[(8 * ch + 2 * i + 1) * VP16 + key] = (bf16_t)(w[i] >> 16);
    }
  }
};

template <> struct Stage<false> {
  f32x4 k[2], v[2];
  __device__ __forceinline__ void load(const void* K, const void* V, long ldk, long ldv, int key0, int Lq, int t) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int idx = t + THREADS * i, key = idx >> 3, ch = idx & 7, g = key0 + key;
      k[i] = v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (g < Lq) {
        k[i] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(K) + g * ldk + 4 * ch);
        v[i] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(V) + g * ldv + 4 * ch);
      }
    }
  }
  __device__ __forceinline__ void store(char* buf, int t) const {
    float* ks = reinterpret_cast<float*>(buf);
    float* vs = ks + KT * KP32;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int idx = t + THREADS * i, key = idx >> 3, ch = idx & 7;
      *reinterpret_cast<f32x4*>(ks + key * KP32 + 4 * ch) = k[i];
      *reinterpret_cast<f32x4*>(vs + key * KP32 + 4 * ch) = v[i];
    }
  }
};

// row of a 32x32 accumulator tile held in register e of lane half h
__device__ __forceinline__ int acc_row(int e, int h) { return (e & 3) + 8 * (e >> 2) + 4 * h; }

template <bool BF>
__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(BF ? 4 : 3, BF ? 4 : 3))) void self_attention_kernel(const void* __restrict__ Qv, const void* __restrict__ Kv,
                                                                  const void* __restrict__ Vv, void* __restrict__ Ov, int Lq,
                                                                  long ldq, long ldk, long ldv, float c) {
  __shared__ __attribute__((aligned(16))) char lds[2 * (BF ? BUF16 : BUF32)];
  constexpr int BUF = BF ? BUF16 : BUF32;
  constexpr int ES = BF ? 2 : 4;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
  const int head = blockIdx.y, b = blockIdx.z;
  const int q = blockIdx.x * ROWS + wave * 32 + r;
  const bool q_ok = q < Lq;
  const char* Qb = reinterpret_cast<const char*>(Qv) + ((long)b * Lq * ldq + D * head) * ES;
  const char* Kb = reinterpret_cast<const char*>(Kv) + ((long)b * Lq * ldk + D * head) * ES;
  const char* Vb = reinterpret_cast<const char*>(Vv) + ((long)b * Lq * ldv + D * head) * ES;

  // the wavefront's Q operand: bf16 k-step s, element j <-> d = 16 s + 8 h + j; fp32 k-step s <-> d = 16 h + s
  bf16x8 q16[2];
  float q32[16];
  if constexpr (BF) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      uint4 w = uint4{0u, 0u, 0u, 0u};
      if (q_ok) w = *reinterpret_cast<const uint4*>(reinterpret_cast<const bf16_t*>(Qb) + q * ldq + 16 * s + 8 * h);
      q16[s] = __builtin_bit_cast(bf16x8, w);
    }
  } else {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      f32x4 w = f32x4{0.f, 0.f, 0.f, 0.f};
      if (q_ok) w = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(Qb) + q * ldq + 16 * h + 4 * g);
#pragma unroll
      for (int i = 0; i < 4; ++i) q32[4 * g + i] = w[i];
    }
  }

  f32x16 oacc;
#pragma unroll
  for (int e = 0; e < 16; ++e) oacc[e] = 0.f;
  float m = -INFINITY, l = 0.f;       // running maximum of the raw scores; this lane's share of the row sum

  const int tiles = (Lq + KT - 1) / KT;
  Stage<BF> st;
  st.load(Kb, Vb, ldk, ldv, 0, Lq, t);
  st.store(lds, t);
  __syncthreads();

  for (int tile = 0; tile < tiles; ++tile) {
    const char* buf = lds + (tile & 1) * BUF;
    if (tile + 1 < tiles) st.load(Kb, Vb, ldk, ldv, (tile + 1) * KT, Lq, t);

    // ---- S^T = K Q^T: sacc[kb][e] = score of key 64 tile + 32 kb + acc_row(e, h) with query q
    f32x16 sacc[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
      for (int e = 0; e < 16; ++e) sacc[kb][e] = 0.f;
      if constexpr (BF) {
        const bf16_t* ks = reinterpret_cast<const bf16_t*>(buf) + (32 * kb + r) * KP16 + 8 * h;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const bf16x8 a = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(ks + 16 * s));
          sacc[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, q16[s], sacc[kb], 0, 0, 0);
        }
      } else {
        const float* ks = reinterpret_cast<const float*>(buf) + (32 * kb + r) * KP32 + 16 * h;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x4 a = *reinterpret_cast<const f32x4*>(ks + 4 * g);
#pragma unroll
          for (int i = 0; i < 4; ++i) sacc[kb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], q32[4 * g + i], sacc[kb], 0, 0, 0);
        }
      }
    }
    if ((tile + 1) * KT > Lq) {         // the last tile's keys behind the sequence (wave-uniform)
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int e = 0; e < 16; ++e)
          if (tile * KT + 32 * kb + acc_row(e, h) >= Lq) sacc[kb][e] = -INFINITY;
    }

    // ---- online softmax: every tile holds at least one key of the sequence, so m is finite from the first tile on
    float mx = sacc[0][0];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int e = 0; e < 16; ++e) mx = fmaxf(mx, sacc[kb][e]);
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float m_new = fmaxf(m, mx);
    const float alpha = __builtin_amdgcn_exp2f((m - m_new) * c);     // first tile: exp2(-inf) = 0 on l = 0, O = 0
    m = m_new;
    float psum = 0.f;
    if constexpr (BF) {
      const float mc = -m_new * c;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          sacc[kb][e] = __builtin_amdgcn_exp2f(__builtin_fmaf(sacc[kb][e], c, mc));
          psum += sacc[kb][e];
        }
    } else {
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          sacc[kb][e] = __builtin_amdgcn_exp2f((sacc[kb][e] - m_new) * c);
          psum += sacc[kb][e];
        }
    }
    l = l * alpha + psum;
#pragma unroll
    for (int e = 0; e < 16; ++e) oacc[e] *= alpha;

    // ---- O^T += V^T P^T: the score tile is the B operand as it stands
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      if constexpr (BF) {
        // k-step s, element j of lane half h <-> key 32 kb + 16 s + 8 (j >> 2) + 4 h + (j & 3) (registers 8 s + j of the tile)
        const bf16_t* vt = reinterpret_cast<const bf16_t*>(buf) + KT * KP16 + r * VP16 + 32 * kb + 4 * h;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const uint2 v0 = *reinterpret_cast<const uint2*>(vt + 16 * s), v1 = *reinterpret_cast<const uint2*>(vt + 16 * s + 8);
          const bf16x8 a = __builtin_bit_cast(bf16x8, uint4{v0.x, v0.y, v1.x, v1.y});
          const uint4 pw = uint4{pack_bf16(sacc[kb][8 * s], sacc[kb][8 * s + 1]), pack_bf16(sacc[kb][8 * s + 2], sacc[kb][8 * s + 3]),
                                 pack_bf16(sacc[kb][8 * s + 4], sacc[kb][8 * s + 5]), pack_bf16(sacc[kb][8 * s + 6], sacc[kb][8 * s + 7])};
          oacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, __builtin_bit_cast(bf16x8, pw), oacc, 0, 0, 0);
        }
      } else {
        // k-step e: lane half h <-> key 32 kb + acc_row(e, h); A = V[that key][d = r]
        const float* vs = reinterpret_cast<const float*>(buf) + KT * KP32 + (32 * kb + 4 * h) * KP32 + r;
#pragma unroll
        for (int e = 0; e < 16; ++e)
          oacc = __builtin_amdgcn_mfma_f32_32x32x2f32(vs[((e & 3) + 8 * (e >> 2)) * KP32], sacc[kb][e], oacc, 0, 0, 0);
      }
    }

    // the other buffer was last read in tile - 1, which every wavefront left through the barrier below
    if (tile + 1 < tiles) st.store(lds + ((tile + 1) & 1) * BUF, t);
    __syncthreads();
  }

  // ---- O[q][32 head + d], d = acc_row(e, h): registers 4 g .. 4 g + 3 are d = 8 g + 4 h .. + 3
  const float inv = 1.f / (l + __shfl_xor(l, 32));
  if (q_ok) {
    if constexpr (BF) {
      bf16_t* o = reinterpret_cast<bf16_t*>(Ov) + ((long)b * Lq + q) * C + D * head + 4 * h;
#pragma unroll
      for (int g = 0; g < 4; ++g)
        store_vec4<bf16_t>(o + 8 * g, oacc[4 * g] * inv, oacc[4 * g + 1] * inv, oacc[4 * g + 2] * inv, oacc[4 * g + 3] * inv);
    } else {
      float* o = reinterpret_cast<float*>(Ov) + ((long)b * Lq + q) * C + D * head + 4 * h;
#pragma unroll
      for (int g = 0; g < 4; ++g)
        store_vec4<float>(o + 8 * g, oacc[4 * g] * inv, oacc[4 * g + 1] * inv, oacc[4 * g + 2] * inv, oacc[4 * g + 3] * inv);
    }
  }
}

}  // namespace mha

extern "C" {

int mvg_self_attention(const void* q, const void* k, const void* v, void* out, int ldq, int ldk, int ldv, int B, int Lq, int C, int M,
                       int dtype, void* stream) {
  if (C != mha::C || M != mha::M || B < 1 || B > 65535 || Lq < 1 || Lq > (1 << 24)) return MVG_E_BADARG;
  if (dtype != MVG_F32 && dtype != MVG_BF16) return MVG_E_BADARG;
  if (q == nullptr || k == nullptr || v == nullptr || out == nullptr) return MVG_E_BADARG;
  const int vec = dtype == MVG_BF16 ? 8 : 4;          // elements per 16-byte access
  if (ldq < C || ldk < C || ldv < C || ldq % vec || ldk % vec || ldv % vec) return MVG_E_BADARG;
  if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) & 15) return MVG_E_BADARG;
  const float c = 1.4426950408889634f / sqrtf((float)mha::D);
  const dim3 grid(mvg_ceil_div(Lq, mha::ROWS), M, B);
  if (dtype == MVG_BF16)
    hipLaunchKernelGGL(mha::self_attention_kernel<true>, grid, dim3(mha::THREADS), 0, (hipStream_t)stream, q, k, v, out, Lq, (long)ldq,
                       (long)ldk, (long)ldv, c);
  else
    hipLaunchKernelGGL(mha::self_attention_kernel<false>, grid, dim3(mha::THREADS), 0, (hipStream_t)stream, q, k, v, out, Lq, (long)ldq,
                       (long)ldk, (long)ldv, c);
  MVG_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
