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
#include "mha_dropout.h"

namespace mha {

constexpr int ROWS = 128;       // query rows per workgroup (4 wavefronts x 32)
constexpr int KT = 64;          // keys per tile
constexpr int THREADS = 256;
constexpr int D = 32, C = 256, M = 8;
constexpr float RS = 0.17677669529663687f;     // 1 / sqrt(D)
constexpr float LOG2E = 1.4426950408889634f;

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

// TRAIN: the forward of the training path (section "Training" below): the same kernel, plus the row statistic lse and attention
// dropout.  The inference instantiation (TRAIN = false) reads none of the four extra arguments.
template <bool BF, bool TRAIN>
__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(BF && !TRAIN ? 4 : 3, BF && !TRAIN ? 4 : 3))) void self_attention_kernel(const void* __restrict__ Qv, const void* __restrict__ Kv,
                                                                  const void* __restrict__ Vv, void* __restrict__ Ov, int Lq,
                                                                  long ldq, long ldk, long ldv, float c, float* __restrict__ lse,
                                                                  int thresh, float zscale, const uint64_t* __restrict__ seed) {
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
  uint32_t row_key = 0u;
  if constexpr (TRAIN)
    if (thresh > 0) row_key = drop_row_key(drop_head_key(*seed, b, head), q);

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
    if constexpr (TRAIN) {
      // dropout after the row sum (which adds the undropped p): registers 4 g .. 4 g + 3 are four consecutive keys, one word
      if (thresh > 0) {
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const uint32_t w = drop_word(row_key, (uint32_t)((tile * KT + 32 * kb) >> 2) + 2 * g + h);
#pragma unroll
            for (int i = 0; i < 4; ++i)
              if ((int)((w >> (8 * i)) & 255u) < thresh) sacc[kb][4 * g + i] = 0.f;
          }
      }
    }

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
  const float lsum = l + __shfl_xor(l, 32);
  float inv = 1.f / lsum;
  if constexpr (TRAIN) {
    inv *= zscale;                    // 1 / (1 - p_q) once per row instead of once per kept element; 1.0f without dropout
    if (q_ok && h == 0) lse[((long)b * M + head) * Lq + q] = __builtin_fmaf(m, RS, logf(lsum));
  }
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

// ================================================================ Training: backward =========================================
// P is recomputed from Q, K and the forward's lse: p = exp(s / sqrt(32) - lse) -- no maximum, no row sum.  With
// delta_i = sum_d dO_id O_id (attn_delta_kernel) and Z = keep / (1 - p_q):
//   dV = (Z o P)^T dO     dP = dO V^T     dS = P o (Z o dP - delta) / sqrt(32)     dQ = dS K     dK = dS^T Q
// Two kernels, each the forward's structure (one operand set in registers, 64-row tiles of the other through two LDS buffers,
// one barrier per tile), each recomputing S and dP: seven products per tile pair instead of five, and in exchange every output
// element has one writer, no sum crosses a workgroup, there is no atomic and no hand-off between workgroups, and every loop is
// bounded by Lq.  1 / sqrt(32) enters dS once, in fp32 (the forward's double-rounding argument).
//   attn_dq_kernel    query on the lane, as in the forward: S^T = K Q^T, dP^T = V dO^T (Q, dO in registers), dS^T lane-local with
//                     lse and delta as lane constants, dQ^T += K^T dS^T with the dS^T accumulator as the B operand.
//   attn_dkdv_kernel  key on the lane: a workgroup owns 128 keys, a wavefront 32 (K, V in registers) and sweeps 64-row tiles of Q
//                     and dO with the rows' lse and delta alongside; S = Q K^T, dP = dO V^T; their accumulators are the B operands
//                     of dV^T += dO^T (Z o P) and dK^T += Q^T dS.
// Rows behind the sequence are zero-filled with lse = delta = 0: p = 1, dP = 0, dS = 0 and every product with them adds an exact
// 0.  Keys behind the sequence get p = 0 (so no exp of a missing key's score can overflow into a stored value).
// bf16: Q, K, V, dO, O bf16; Z o P and dS rounded to bf16 only as MFMA operands; lse, delta, P, dP, dS fp32; dQ, dK, dV rounded
// once on store.  fp32: v_mfma_f32_32x32x2_f32 chains as in the forward.
//
// Dropout mask (mha_dropout.h): one 32-bit word = drop_mix(row key + chunk * const) decides the four keys 4 c .. 4 c + 3 of a
// query, 8 bits each.  drop_mix is 8 VALU instructions, two of them 32-bit multiplies (quarter rate): ~14 issue slots.
//   query on the lane (forward, dQ): registers 4 g .. 4 g + 3 are four consecutive keys -> one word per four scores, plus
//     shift / and / compare / select per score: ~7 slots per score with dropout on, against ~5 of the bf16 forward without.
//   key on the lane (dK/dV): registers 4 g .. 4 g + 3 are four consecutive queries of ONE key, four words.  The four lanes of a
//     quad hold the four keys of one chunk, so lane (key & 3) = i computes the word of query 4 g + i and the quad exchanges the
//     four words with DPP quad broadcasts (full rate, no LDS): again one word per four scores, plus one move per score.  The
//     row keys of a tile's 64 queries are computed once per tile by 64 threads and staged in LDS next to lse and delta.
// With dropout off (threshold 0) none of it runs: the branches are wave-uniform.  The forward applies 1 / (1 - p_q) once per
// row (to the final 1 / row sum), the backward per kept element.

// p = exp(s / sqrt(32) - lse).  The product is rounded on its own, NOT fused into the subtraction: the forward's lse is
// round(m / sqrt(32) + ln(row sum)), so on a row one key dominates (row sum 1) the rounded product of that key IS lse and p is
// exactly 1; an fma would keep the product's rounding residue, 4e-6 at |score| 80, as an error of p.
__device__ __forceinline__ float recompute_p(float s, float lse) {
  float x = s * RS;
  asm("" : "+v"(x));                // -ffp-contract=fast would fuse the product into the subtraction (it does so through __fmul_rn too)
  return __builtin_amdgcn_exp2f((x - lse) * LOG2E);
}

template <bool BF> struct Img {     // LDS images of one backward tile: two 64 x 32 operands X, Y by rows; bf16: also transposed
  static constexpr int ROWB = BF ? KP16 * 2 : KP32 * 4;                // bytes per row
  static constexpr int XR = 0, YR = KT * ROWB;
  static constexpr int XT = BF ? 2 * KT * ROWB : XR, YT = BF ? XT + D * VP16 * 2 : YR;   // fp32 reads the row image by columns
  static constexpr int STAT = BF ? YT + D * VP16 * 2 : 2 * KT * ROWB;  // lse[64], delta[64], row keys[64] of the tile's rows
  static constexpr int BYTES = STAT + 3 * KT * 4;
};

template <bool BF, bool XT_, bool YT_> __device__ __forceinline__ void stage_store(const Stage<BF>& st, char* buf, int t) {
  if constexpr (BF) {
    const int key = t >> 2, ch = t & 3;
    *reinterpret_cast<uint4*>(buf + Img<true>::XR + key * Img<true>::ROWB + 16 * ch) = st.k;
    *reinterpret_cast<uint4*>(buf + Img<true>::YR + key * Img<true>::ROWB + 16 * ch) = st.v;
    const unsigned wk[4] = {st.k.x, st.k.y, st.k.z, st.k.w}, wv[4] = {st.v.x, st.v.y, st.v.z, st.v.w};
    bf16_t* xt = reinterpret_cast<bf16_t*>(buf + Img<true>::XT);
    bf16_t* yt = reinterpret_cast<bf16_t*>(buf + Img<true>::YT);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if constexpr (XT_) {
        xt[(8 * ch + 2 * i) * VP16 + key] = (bf16_t)(wk[i] & 0xffffu);
        xt[(8 * ch + 2 * i + 1) * VP16 + key] = (bf16_t)(wk[i] >> 16);
      }
      if constexpr (YT_) {
        yt[(8 * ch + 2 * i) * VP16 + key] = (bf16_t)(wv[i] & 0xffffu);
        yt[(8 * ch + 2 * i + 1) * VP16 + key] = (bf16_t)(wv[i] >> 16);
      }
    }
  } else {
    st.store(buf, t);               // X rows, Y rows: the forward's fp32 image
  }
}

// one row of 32 elements per lane (lane's row `row` of a (.., ld) matrix, zero when !ok) as the B operand of a product that sums
// over d: bf16 k-step s, element j <-> d = 16 s + 8 h + j; fp32 k-step s <-> d = 16 h + s
template <bool BF> struct RowOp {
  bf16x8 v16[2];
  float v32[16];
  __device__ __forceinline__ void load(const char* base, long row, long ld, bool ok, int h) {
    if constexpr (BF) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        uint4 w = uint4{0u, 0u, 0u, 0u};
        if (ok) w = *reinterpret_cast<const uint4*>(reinterpret_cast<const bf16_t*>(base) + row * ld + 16 * s + 8 * h);
        v16[s] = __builtin_bit_cast(bf16x8, w);
      }
    } else {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f32x4 w = f32x4{0.f, 0.f, 0.f, 0.f};
        if (ok) w = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(base) + row * ld + 16 * h + 4 * g);
#pragma unroll
        for (int i = 0; i < 4; ++i) v32[4 * g + i] = w[i];
      }
    }
  }
};

// acc (tile row, lane row) += sum_d IMG[32 blk + tile row][d] * b[d]: the row image `img` (X or Y) as the A operand
template <bool BF> __device__ __forceinline__ void mma_rows(f32x16& acc, const char* img, int blk, int r, int h, const RowOp<BF>& b) {
  if constexpr (BF) {
    const bf16_t* a0 = reinterpret_cast<const bf16_t*>(img) + (32 * blk + r) * KP16 + 8 * h;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const bf16x8 a = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(a0 + 16 * s));
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b.v16[s], acc, 0, 0, 0);
    }
  } else {
    const float* a0 = reinterpret_cast<const float*>(img) + (32 * blk + r) * KP32 + 16 * h;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(a0 + 4 * g);
#pragma unroll
      for (int i = 0; i < 4; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b.v32[4 * g + i], acc, 0, 0, 0);
    }
  }
}

// acc (d, lane row) += sum_rows IMG[32 blk + row][d] * x[row][lane row]: the accumulator tile x is the B operand as it stands;
// `imgt` is the transposed image (bf16: XT / YT, read in the accumulator's permuted k order) or the row image itself (fp32)
template <bool BF> __device__ __forceinline__ void mma_cols(f32x16& acc, const char* imgt, int blk, int r, int h, const f32x16& x) {
  if constexpr (BF) {
    const bf16_t* at = reinterpret_cast<const bf16_t*>(imgt) + r * VP16 + 32 * blk + 4 * h;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const uint2 a0 = *reinterpret_cast<const uint2*>(at + 16 * s), a1 = *reinterpret_cast<const uint2*>(at + 16 * s + 8);
      const bf16x8 a = __builtin_bit_cast(bf16x8, uint4{a0.x, a0.y, a1.x, a1.y});
      const uint4 xw = uint4{pack_bf16(x[8 * s], x[8 * s + 1]), pack_bf16(x[8 * s + 2], x[8 * s + 3]),
                             pack_bf16(x[8 * s + 4], x[8 * s + 5]), pack_bf16(x[8 * s + 6], x[8 * s + 7])};
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, __builtin_bit_cast(bf16x8, xw), acc, 0, 0, 0);
    }
  } else {
    const float* a0 = reinterpret_cast<const float*>(imgt) + (32 * blk + 4 * h) * KP32 + r;
#pragma unroll
    for (int e = 0; e < 16; ++e)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[((e & 3) + 8 * (e >> 2)) * KP32], x[e], acc, 0, 0, 0);
  }
}

// an accumulator tile (d = acc_row(e, h), lane's row) to row `row` of a (.., ld) matrix at column `col0`, rounded once
template <bool BF> __device__ __forceinline__ void store_rows(void* base, long row, long ld, int col0, int h, const f32x16& acc) {
  if constexpr (BF) {
    bf16_t* o = reinterpret_cast<bf16_t*>(base) + row * ld + col0 + 4 * h;
#pragma unroll
    for (int g = 0; g < 4; ++g) store_vec4<bf16_t>(o + 8 * g, acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]);
  } else {
    float* o = reinterpret_cast<float*>(base) + row * ld + col0 + 4 * h;
#pragma unroll
    for (int g = 0; g < 4; ++g) store_vec4<float>(o + 8 * g, acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]);
  }
}

// delta[b, h, i] = sum_d O[b, i, 32 h + d] * dO[b, i, 32 h + d] as the diagonal of the 32 x 32 product O dO^T of a wavefront's 32
// rows, on the MFMA chain of dP (O in V's place, dO where dO is): 31 of 32 results are thrown away -- the launch is 4.6 / Lq of the
// backward's multiply-adds -- and in exchange delta has dP's summation order.  On a row one key dominates (P = 1, O = that key's V bit
// for bit; every row at Lq = 1) dP - delta is then exactly 0, as the true dS is, instead of the rounding noise of two orders.
// One workgroup = 128 rows of one (head, batch element), as in the other kernels.
template <bool BF>
__global__ __launch_bounds__(THREADS) void attn_delta_kernel(const void* __restrict__ Ov, const void* __restrict__ dOv,
                                                             float* __restrict__ delta, int Lq) {
  constexpr int ES = BF ? 2 : 4;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
  const int head = blockIdx.y, b = blockIdx.z;
  const int q = blockIdx.x * ROWS + wave * 32 + r;
  const bool q_ok = q < Lq;
  const long base = ((long)b * Lq * C + D * head) * ES;
  RowOp<BF> oop, gop;
  oop.load(reinterpret_cast<const char*>(Ov) + base, q, C, q_ok, h);
  gop.load(reinterpret_cast<const char*>(dOv) + base, q, C, q_ok, h);
  f32x16 acc;                                   // (row acc_row(e, h) of O, row r of dO)
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  if constexpr (BF) {
#pragma unroll
    for (int s = 0; s < 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(oop.v16[s], gop.v16[s], acc, 0, 0, 0);
  } else {
#pragma unroll
    for (int s = 0; s < 16; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(oop.v32[s], gop.v32[s], acc, 0, 0, 0);
  }
  // the diagonal element of row r lies in lane half (r >> 2) & 1, register (r & 3) + 4 (r >> 3)
  float d = 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e)
    if (e == (r & 3) + 4 * (r >> 3)) d = acc[e];
  if (q_ok && h == ((r >> 2) & 1)) delta[((long)b * M + head) * Lq + q] = d;
}

template <bool BF>
__global__ __launch_bounds__(THREADS) void attn_dq_kernel(const void* __restrict__ Qv, const void* __restrict__ Kv,
                                                          const void* __restrict__ Vv, const void* __restrict__ dOv,
                                                          const float* __restrict__ lse, const float* __restrict__ delta,
                                                          void* __restrict__ dQv, int Lq, long ldq, long ldk, long ldv, long lddq,
                                                          int thresh, float zscale, const uint64_t* __restrict__ seed) {
  using I = Img<BF>;
  __shared__ __attribute__((aligned(16))) char lds[2 * I::BYTES];
  constexpr int ES = BF ? 2 : 4;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
  const int head = blockIdx.y, b = blockIdx.z;
  const int q = blockIdx.x * ROWS + wave * 32 + r;
  const bool q_ok = q < Lq;
  const char* Qb = reinterpret_cast<const char*>(Qv) + ((long)b * Lq * ldq + D * head) * ES;
  const char* Kb = reinterpret_cast<const char*>(Kv) + ((long)b * Lq * ldk + D * head) * ES;
  const char* Vb = reinterpret_cast<const char*>(Vv) + ((long)b * Lq * ldv + D * head) * ES;
  const char* Gb = reinterpret_cast<const char*>(dOv) + ((long)b * Lq * C + D * head) * ES;

  RowOp<BF> qop, gop;
  qop.load(Qb, q, ldq, q_ok, h);
  gop.load(Gb, q, C, q_ok, h);
  const long stat = ((long)b * M + head) * Lq + q;
  const float lse_q = q_ok ? lse[stat] : 0.f, delta_q = q_ok ? delta[stat] : 0.f;
  uint32_t row_key = 0u;
  if (thresh > 0) row_key = drop_row_key(drop_head_key(*seed, b, head), q);

  f32x16 dq;
#pragma unroll
  for (int e = 0; e < 16; ++e) dq[e] = 0.f;

  const int tiles = (Lq + KT - 1) / KT;
  Stage<BF> st;
  st.load(Kb, Vb, ldk, ldv, 0, Lq, t);
  stage_store<BF, true, false>(st, lds, t);
  __syncthreads();

  for (int tile = 0; tile < tiles; ++tile) {
    const char* buf = lds + (tile & 1) * I::BYTES;
    if (tile + 1 < tiles) st.load(Kb, Vb, ldk, ldv, (tile + 1) * KT, Lq, t);
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      const int key0 = tile * KT + 32 * kb;
      if (key0 >= Lq) break;                      // a block of keys wholly behind the sequence (uniform)
      f32x16 s, dp;                               // (key 32 kb + acc_row(e, h), query q)
#pragma unroll
      for (int e = 0; e < 16; ++e) s[e] = dp[e] = 0.f;
      mma_rows<BF>(s, buf + I::XR, kb, r, h, qop);        // S^T  = K Q^T
      mma_rows<BF>(dp, buf + I::YR, kb, r, h, gop);       // dP^T = V dO^T
#pragma unroll
      for (int e = 0; e < 16; ++e) s[e] = recompute_p(s[e], lse_q);
      if (key0 + 32 > Lq) {
#pragma unroll
        for (int e = 0; e < 16; ++e)
          if (key0 + acc_row(e, h) >= Lq) s[e] = 0.f;
      }
      if (thresh > 0) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const uint32_t w = drop_word(row_key, (uint32_t)(key0 >> 2) + 2 * g + h);
#pragma unroll
          for (int i = 0; i < 4; ++i) dp[4 * g + i] = (int)((w >> (8 * i)) & 255u) < thresh ? 0.f : dp[4 * g + i] * zscale;
        }
      }
#pragma unroll
      for (int e = 0; e < 16; ++e) s[e] = s[e] * (dp[e] - delta_q) * RS;       // dS^T
      mma_cols<BF>(dq, buf + I::XT, kb, r, h, s);         // dQ^T += K^T dS^T
    }
    if (tile + 1 < tiles) stage_store<BF, true, false>(st, lds + ((tile + 1) & 1) * I::BYTES, t);
    __syncthreads();
  }
  if (q_ok) store_rows<BF>(dQv, (long)b * Lq + q, lddq, D * head, h, dq);
}

template <bool BF>
__global__ __launch_bounds__(THREADS) void attn_dkdv_kernel(const void* __restrict__ Qv, const void* __restrict__ Kv,
                                                            const void* __restrict__ Vv, const void* __restrict__ dOv,
                                                            const float* __restrict__ lse, const float* __restrict__ delta,
                                                            void* __restrict__ dKv, void* __restrict__ dVv, int Lq, long ldq,
                                                            long ldk, long ldv, long lddk, long lddv, int thresh, float zscale,
                                                            const uint64_t* __restrict__ seed) {
  using I = Img<BF>;
  __shared__ __attribute__((aligned(16))) char lds[2 * I::BYTES];
  constexpr int ES = BF ? 2 : 4;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
  const int head = blockIdx.y, b = blockIdx.z;
  const int key = blockIdx.x * ROWS + wave * 32 + r;
  const bool key_ok = key < Lq;
  const bool ragged = blockIdx.x * ROWS + wave * 32 + 32 > Lq;      // some lane of this wavefront has no key (uniform)
  const char* Qb = reinterpret_cast<const char*>(Qv) + ((long)b * Lq * ldq + D * head) * ES;
  const char* Kb = reinterpret_cast<const char*>(Kv) + ((long)b * Lq * ldk + D * head) * ES;
  const char* Vb = reinterpret_cast<const char*>(Vv) + ((long)b * Lq * ldv + D * head) * ES;
  const char* Gb = reinterpret_cast<const char*>(dOv) + ((long)b * Lq * C + D * head) * ES;
  const float* lse_b = lse + ((long)b * M + head) * Lq;
  const float* delta_b = delta + ((long)b * M + head) * Lq;

  RowOp<BF> kop, vop;
  kop.load(Kb, key, ldk, key_ok, h);
  vop.load(Vb, key, ldv, key_ok, h);
  const uint32_t head_key = thresh > 0 ? drop_head_key(*seed, b, head) : 0u;
  const uint32_t chunk_g = ((uint32_t)key >> 2) * DROP_GOLD;       // drop_word's second term: this lane's key chunk
  const int byte_sh = 8 * (key & 3);

  f32x16 dk, dv;
#pragma unroll
  for (int e = 0; e < 16; ++e) dk[e] = dv[e] = 0.f;

  // the tile's row statistics: wavefront 0 lse, 1 delta, 2 the dropout row keys
  float stat = 0.f;
  auto load_stat = [&](int row0) {
    const int row = row0 + lane;
    stat = 0.f;
    if (wave == 0) { if (row < Lq) stat = lse_b[row]; }
    else if (wave == 1) { if (row < Lq) stat = delta_b[row]; }
    else if (wave == 2) { if (thresh > 0) stat = __uint_as_float(drop_row_key(head_key, row)); }
  };
  auto store_stat = [&](char* buf) {
    if (wave < 3) reinterpret_cast<float*>(buf + I::STAT)[t] = stat;
  };

  const int tiles = (Lq + KT - 1) / KT;
  Stage<BF> st;
  st.load(Qb, Gb, ldq, C, 0, Lq, t);
  load_stat(0);
  stage_store<BF, true, true>(st, lds, t);
  store_stat(lds);
  __syncthreads();

  for (int tile = 0; tile < tiles; ++tile) {
    const char* buf = lds + (tile & 1) * I::BYTES;
    if (tile + 1 < tiles) {
      st.load(Qb, Gb, ldq, C, (tile + 1) * KT, Lq, t);
      load_stat((tile + 1) * KT);
    }
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
      if (tile * KT + 32 * qb >= Lq) break;       // a block of rows wholly behind the sequence (uniform)
      f32x16 s, dp;                               // (query 32 qb + acc_row(e, h), key)
#pragma unroll
      for (int e = 0; e < 16; ++e) s[e] = dp[e] = 0.f;
      mma_rows<BF>(s, buf + I::XR, qb, r, h, kop);        // S  = Q K^T
      mma_rows<BF>(dp, buf + I::YR, qb, r, h, vop);       // dP = dO V^T
      const float* ls = reinterpret_cast<const float*>(buf + I::STAT) + 32 * qb + 4 * h;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 l4 = *reinterpret_cast<const f32x4*>(ls + 8 * g);
#pragma unroll
        for (int i = 0; i < 4; ++i) s[4 * g + i] = recompute_p(s[4 * g + i], l4[i]);
      }
      if (ragged) {
#pragma unroll
        for (int e = 0; e < 16; ++e) s[e] = key_ok ? s[e] : 0.f;
      }
      f32x16 zp = s;                              // Z o P
      if (thresh > 0) {
        const unsigned* rk = reinterpret_cast<const unsigned*>(buf + I::STAT) + 2 * KT + 32 * qb + 4 * h + (r & 3);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          // this lane's word: query 8 g + 4 h + (key & 3) with the quad's key chunk; word i of the quad is query 8 g + 4 h + i
          const int mine = (int)drop_mix(rk[8 * g] + chunk_g);
          const int w[4] = {__builtin_amdgcn_update_dpp(0, mine, 0x00, 0xf, 0xf, false), __builtin_amdgcn_update_dpp(0, mine, 0x55, 0xf, 0xf, false),
                            __builtin_amdgcn_update_dpp(0, mine, 0xaa, 0xf, 0xf, false), __builtin_amdgcn_update_dpp(0, mine, 0xff, 0xf, 0xf, false)};
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const bool drop = (int)(((unsigned)w[i] >> byte_sh) & 255u) < thresh;
            zp[4 * g + i] = drop ? 0.f : zp[4 * g + i] * zscale;
            dp[4 * g + i] = drop ? 0.f : dp[4 * g + i] * zscale;
          }
        }
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 d4 = *reinterpret_cast<const f32x4*>(ls + KT + 8 * g);
#pragma unroll
        for (int i = 0; i < 4; ++i) s[4 * g + i] = s[4 * g + i] * (dp[4 * g + i] - d4[i]) * RS;     // dS
      }
      mma_cols<BF>(dv, buf + I::YT, qb, r, h, zp);        // dV^T += dO^T (Z o P)
      mma_cols<BF>(dk, buf + I::XT, qb, r, h, s);         // dK^T += Q^T dS
    }
    if (tile + 1 < tiles) {
      char* nxt = lds + ((tile + 1) & 1) * I::BYTES;
      stage_store<BF, true, true>(st, nxt, t);
      store_stat(nxt);
    }
    __syncthreads();
  }
  if (key_ok) {
    store_rows<BF>(dKv, (long)b * Lq + key, lddk, D * head, h, dk);
    store_rows<BF>(dVv, (long)b * Lq + key, lddv, D * head, h, dv);
  }
}

// the keep mask as bytes, (B, 8, Lq, Lq): the decision every kernel above takes for (b, head, query, key)
__global__ __launch_bounds__(THREADS) void dropout_mask_kernel(unsigned char* __restrict__ mask, int Lq, int thresh,
                                                               const uint64_t* __restrict__ seed) {
  const int idx = blockIdx.x * THREADS + threadIdx.x, head = blockIdx.y, b = blockIdx.z;
  if (idx >= Lq * Lq) return;
  const int query = idx / Lq, key = idx - query * Lq;
  mask[((long)b * M + head) * Lq * Lq + idx] = thresh == 0 || drop_keep(*seed, b, head, query, key, thresh) ? 1 : 0;
}

static int check_qkv(const void* q, const void* k, const void* v, int ldq, int ldk, int ldv, int B, int Lq, int C_, int M_, int dtype) {
  if (C_ != C || M_ != M || B < 1 || B > 65535 || Lq < 1 || Lq > (1 << 24)) return MVG_E_BADARG;
  if (dtype != MVG_F32 && dtype != MVG_BF16) return MVG_E_BADARG;
  if (q == nullptr || k == nullptr || v == nullptr) return MVG_E_BADARG;
  const int vec = dtype == MVG_BF16 ? 8 : 4;          // elements per 16-byte access
  if (ldq < C || ldk < C || ldv < C || ldq % vec || ldk % vec || ldv % vec) return MVG_E_BADARG;
  if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) & 15) return MVG_E_BADARG;
  return 0;
}

static int check_dropout(float p_drop, const uint64_t* seed) {
  if (!(p_drop >= 0.f && p_drop < 1.f)) return MVG_E_BADARG;
  if (p_drop > 0.f && (seed == nullptr || ((uintptr_t)seed & 7))) return MVG_E_BADARG;
  return 0;
}

}  // namespace mha

extern "C" {

int mvg_self_attention(const void* q, const void* k, const void* v, void* out, int ldq, int ldk, int ldv, int B, int Lq, int C, int M,
                       int dtype, void* stream) {
  if (mha::check_qkv(q, k, v, ldq, ldk, ldv, B, Lq, C, M, dtype) || out == nullptr || ((uintptr_t)out & 15)) return MVG_E_BADARG;
  const float c = 1.4426950408889634f / sqrtf((float)mha::D);
  const dim3 grid(mvg_ceil_div(Lq, mha::ROWS), M, B);
  if (dtype == MVG_BF16)
    hipLaunchKernelGGL((mha::self_attention_kernel<true, false>), grid, dim3(mha::THREADS), 0, (hipStream_t)stream, q, k, v, out, Lq,
                       (long)ldq, (long)ldk, (long)ldv, c, (float*)nullptr, 0, 1.f, (const uint64_t*)nullptr);
  else
    hipLaunchKernelGGL((mha::self_attention_kernel<false, false>), grid, dim3(mha::THREADS), 0, (hipStream_t)stream, q, k, v, out, Lq,
                       (long)ldq, (long)ldk, (long)ldv, c, (float*)nullptr, 0, 1.f, (const uint64_t*)nullptr);
  MVG_LAUNCH_CHECK();
  return 0;
}

int mvg_self_attention_train(const void* q, const void* k, const void* v, void* out, float* lse, int ldq, int ldk, int ldv, int B, int Lq,
                             int C, int M, int dtype, float p_drop, const uint64_t* seed, void* stream) {
  if (mha::check_qkv(q, k, v, ldq, ldk, ldv, B, Lq, C, M, dtype) || out == nullptr || ((uintptr_t)out & 15)) return MVG_E_BADARG;
  if (lse == nullptr || ((uintptr_t)lse & 3) || mha::check_dropout(p_drop, seed)) return MVG_E_BADARG;
  const float c = 1.4426950408889634f / sqrtf((float)mha::D);
  const int thresh = mha::drop_threshold(p_drop);
  const float zscale = 256.f / (float)(256 - thresh);
  const dim3 grid(mvg_ceil_div(Lq, mha::ROWS), M, B);
  if (dtype == MVG_BF16)
    hipLaunchKernelGGL((mha::self_attention_kernel<true, true>), grid, dim3(mha::THREADS), 0, (hipStream_t)stream, q, k, v, out, Lq,
                       (long)ldq, (long)ldk, (long)ldv, c, lse, thresh, zscale, seed);
  else
    hipLaunchKernelGGL((mha::self_attention_kernel<false, true>), grid, dim3(mha::THREADS), 0, (hipStream_t)stream, q, k, v, out, Lq,
                       (long)ldq, (long)ldk, (long)ldv, c, lse, thresh, zscale, seed);
  MVG_LAUNCH_CHECK();
  return 0;
}

size_t mvg_self_attention_backward_workspace(int B, int Lq) {
  if (B < 1 || B > 65535 || Lq < 1 || Lq > (1 << 24)) return 0;
  return (size_t)B * mha::M * Lq * sizeof(float);
}

int mvg_self_attention_backward(const void* q, const void* k, const void* v, const void* out, const void* dout, const float* lse, void* dq,
                                void* dk, void* dv, int ldq, int ldk, int ldv, int lddq, int lddk, int lddv, int B, int Lq, int C, int M,
                                int dtype, float p_drop, const uint64_t* seed, void* workspace, size_t workspace_bytes, void* stream) {
  if (mha::check_qkv(q, k, v, ldq, ldk, ldv, B, Lq, C, M, dtype) || mha::check_qkv(dq, dk, dv, lddq, lddk, lddv, B, Lq, C, M, dtype))
    return MVG_E_BADARG;
  if (out == nullptr || dout == nullptr || (((uintptr_t)out | (uintptr_t)dout) & 15)) return MVG_E_BADARG;
  if (lse == nullptr || ((uintptr_t)lse & 3) || mha::check_dropout(p_drop, seed)) return MVG_E_BADARG;
  if (workspace == nullptr || ((uintptr_t)workspace & 3) || workspace_bytes < mvg_self_attention_backward_workspace(B, Lq))
    return MVG_E_BADARG;
  float* delta = reinterpret_cast<float*>(workspace);
  const int thresh = mha::drop_threshold(p_drop);
  const float zscale = 256.f / (float)(256 - thresh);
  const hipStream_t s = (hipStream_t)stream;
  const dim3 grid(mvg_ceil_div(Lq, mha::ROWS), M, B), block(mha::THREADS);
  if (dtype == MVG_BF16) {
    hipLaunchKernelGGL(mha::attn_delta_kernel<true>, grid, block, 0, s, out, dout, delta, Lq);
    hipLaunchKernelGGL(mha::attn_dq_kernel<true>, grid, block, 0, s, q, k, v, dout, lse, (const float*)delta, dq, Lq, (long)ldq, (long)ldk,
                       (long)ldv, (long)lddq, thresh, zscale, seed);
    hipLaunchKernelGGL(mha::attn_dkdv_kernel<true>, grid, block, 0, s, q, k, v, dout, lse, (const float*)delta, dk, dv, Lq, (long)ldq,
                       (long)ldk, (long)ldv, (long)lddk, (long)lddv, thresh, zscale, seed);
  } else {
    hipLaunchKernelGGL(mha::attn_delta_kernel<false>, grid, block, 0, s, out, dout, delta, Lq);
    hipLaunchKernelGGL(mha::attn_dq_kernel<false>, grid, block, 0, s, q, k, v, dout, lse, (const float*)delta, dq, Lq, (long)ldq, (long)ldk,
                       (long)ldv, (long)lddq, thresh, zscale, seed);
    hipLaunchKernelGGL(mha::attn_dkdv_kernel<false>, grid, block, 0, s, q, k, v, dout, lse, (const float*)delta, dk, dv, Lq, (long)ldq,
                       (long)ldk, (long)ldv, (long)lddk, (long)lddv, thresh, zscale, seed);
  }
  MVG_LAUNCH_CHECK();
  return 0;
}

int mvg_self_attention_dropout_mask(unsigned char* mask, int B, int Lq, float p_drop, const uint64_t* seed, void* stream) {
  if (mask == nullptr || B < 1 || B > 65535 || Lq < 1 || Lq > MVG_MHA_MASK_MAX_LQ || mha::check_dropout(p_drop, seed)) return MVG_E_BADARG;
  const dim3 grid(mvg_ceil_div((long)Lq * Lq, mha::THREADS), mha::M, B);
  hipLaunchKernelGGL(mha::dropout_mask_kernel, grid, dim3(mha::THREADS), 0, (hipStream_t)stream, mask, Lq, mha::drop_threshold(p_drop), seed);
  MVG_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"

