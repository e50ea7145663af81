// Derived bf16 operands of the bf16 training path for gfx950: for every fp32 master weight W (N x K, row-major) the row-major
// bf16 copy W16 and the transposed bf16 copy W16^T (K x N) that LinearBF16 multiplies by, rewritten in ONE launch driven by
// tables in device memory (mvg_decoder.h), so that the launch can sit in a HIP graph right behind the optimizer's update kernel
// and no kernel argument depends on the parameter set.  Ordinary vector stores only: no atomics, no memset, nothing read back.
//
// One workgroup of 256 threads converts one 64 x 64 tile:
//   load     thread (g = t & 7, r = t >> 3) holds columns 8g .. 8g+7 of rows r and r + 32: two 16-byte loads per row
//   convert  round to nearest even, the bits of tensor.to(torch.bfloat16) (a NaN becomes the quiet NaN 0x7FC0, as there)
//   dst      straight from the registers: 8 bf16 = one 16-byte store per row
//   dstT     through an LDS tile of 64 x 64 dwords (the bf16 bits, one per dword), then thread (ng = t & 7, k = t >> 3 and k + 32)
//            gathers rows 8ng .. 8ng+7 of column k: 8 bf16 = one 16-byte store, eight neighbouring lanes fill one 128-byte line
// Edge tiles, leading dimensions or pointers that do not allow 16-byte accesses take the element path of the same thread
// mapping; the value stored is the same function of the source element on every path.
//
// The LDS tile: pitch 64 dwords, NO padding, columns XOR-ed with 4 * ((row >> 3) & 7).  Why not a padded pitch: the rows are
// written with 16-byte ds_write_b128, so a pitch must be a multiple of 4 dwords; the column gather reads, in one 32-lane half of a
// ds_read_b32, rows 8ng + j (ng = 0 .. 7) of four neighbouring columns, and 8 * ng * pitch is then a multiple of 32 dwords for EVERY
// such pitch: the eight row groups would sit on the same four banks (8-way) whatever the padding.  The XOR moves row group ng by
// 4 * ng columns instead: bank = ((k0 ^ 4ng) + kk) mod 32 with k0 a multiple of 4 and kk = 0 .. 3 -- 32 lanes, 32 banks.  It keeps
// every aligned group of 4 columns together, so the row writes stay 16-byte writes; ds_write_b128 is serviced in groups of 8
// contiguous lanes (one row, g = 0 .. 7), whose 16-byte pieces at columns 8g + {0, 4} would meet pairwise (g and g + 4 are 32
// dwords apart): lanes g >= 4 write their second piece first, the eight pieces of one pass are then at columns
// {0, 8, 16, 24, 36, 44, 52, 60} ^ s = banks {0, 8, 16, 24, 4, 12, 20, 28} ^ s, four dwords each: 32 banks.
#include "exact_dev.h"

#define OPD_THREADS 256
#define OPD_TILE MVG_OPERANDS_TILE
static_assert(OPD_TILE == 64 && OPD_THREADS == 256, "the thread mapping below is written for 64 x 64 tiles and 256 threads");

struct OpdRecord {          // MVG_OPERANDS_RECORD_WORDS x 8 bytes
  const float* src;         // fp32, row-major N x K
  long N, K, src_ld;
  bf16_t* dst;              // bf16 N x K, or NULL
  long dst_ld;
  bf16_t* dstT;             // bf16 K x N, or NULL
  long dstT_ld;
};
struct OpdTile {            // 8 bytes
  int record;
  int tile;                 // row-major over ceil(N / 64) x ceil(K / 64)
};
static_assert(sizeof(OpdRecord) == MVG_OPERANDS_RECORD_WORDS * 8 && sizeof(OpdTile) == 8, "table layout of mvg_decoder.h");

// The pointers come out of a table, so the compiler takes them for generic (flat) addresses; they are global memory.
typedef __attribute__((address_space(1))) const float opd_gfloat;
typedef __attribute__((address_space(1))) const f32x4 opd_gf32x4;
typedef __attribute__((address_space(1))) bf16_t opd_gbf16;
typedef unsigned opd_u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) opd_u32x4 opd_guint4;

// fp32 -> bf16 bits exactly as c10::BFloat16(float) rounds: nearest, ties to even; +-Inf and +-0 keep their bits, a finite value
// at or above the midpoint beyond the largest bf16 becomes Inf, a NaN becomes 0x7FC0
__device__ __forceinline__ unsigned opd_bf16_bits(float f) {
  const unsigned u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

__global__ __launch_bounds__(OPD_THREADS) void refresh_operands_kernel(const OpdRecord* __restrict__ records, int n_records,
                                                                       const OpdTile* __restrict__ tiles) {
  __shared__ __attribute__((aligned(16))) unsigned s_tile[OPD_TILE * OPD_TILE];
  const OpdTile job = tiles[blockIdx.x];
  if (job.record < 0 || job.record >= n_records || job.tile < 0) return;
  const OpdRecord rec = records[job.record];
  if (!rec.src || rec.N < 1 || rec.K < 1) return;
  const long tiles_k = (rec.K + OPD_TILE - 1) / OPD_TILE, tiles_n = (rec.N + OPD_TILE - 1) / OPD_TILE;
  if (job.tile >= tiles_n * tiles_k) return;
  const long n0 = (job.tile / tiles_k) * OPD_TILE, k0 = (job.tile % tiles_k) * OPD_TILE;
  const bool full = n0 + OPD_TILE <= rec.N && k0 + OPD_TILE <= rec.K;
  const int t = threadIdx.x, g = t & 7, r = t >> 3;

  // ---- load + convert: bits[i][e] = element (n0 + r + 32 i, k0 + 8 g + e); zero outside the matrix (never stored)
  const bool src_vec = full && aligned16(rec.src) && (rec.src_ld & 3) == 0;
  const bool dst_vec = rec.dst && full && aligned16(rec.dst) && (rec.dst_ld & 7) == 0;
  opd_gfloat* src = (opd_gfloat*)rec.src;
  opd_gbf16* dst = (opd_gbf16*)rec.dst;
  unsigned bits[2][8];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const long n = n0 + r + 32 * i, k = k0 + 8 * g;
    if (src_vec) {
      const f32x4 a = *(opd_gf32x4*)(src + n * rec.src_ld + k), b = *(opd_gf32x4*)(src + n * rec.src_ld + k + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        bits[i][e] = opd_bf16_bits(a[e]);
        bits[i][4 + e] = opd_bf16_bits(b[e]);
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) bits[i][e] = (n < rec.N && k + e < rec.K) ? opd_bf16_bits(src[n * rec.src_ld + k + e]) : 0u;
    }
    if (dst_vec) {
      *(opd_guint4*)(dst + n * rec.dst_ld + k) = opd_u32x4{bits[i][0] | (bits[i][1] << 16), bits[i][2] | (bits[i][3] << 16),
                                                       bits[i][4] | (bits[i][5] << 16), bits[i][6] | (bits[i][7] << 16)};
    } else if (rec.dst && n < rec.N) {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (k + e < rec.K) dst[n * rec.dst_ld + k + e] = (bf16_t)bits[i][e];
    }
  }
  if (!rec.dstT) return;                                          // workgroup-uniform: nobody waits at the barrier below

  // ---- rows into the LDS tile (layout: header comment)
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = r + 32 * i, swz = ((row >> 3) & 7) << 2;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
      const bool hi = (pass ^ (g >> 2)) & 1;                      // lanes g >= 4 write their second piece first
      const opd_u32x4 piece = hi ? opd_u32x4{bits[i][4], bits[i][5], bits[i][6], bits[i][7]}
                             : opd_u32x4{bits[i][0], bits[i][1], bits[i][2], bits[i][3]};
      *reinterpret_cast<opd_u32x4*>(&s_tile[row * OPD_TILE + ((8 * g + (hi ? 4 : 0)) ^ swz)]) = piece;
    }
  }
  __syncthreads();

  // ---- column gather: thread (ng, kk) stores dstT[k0 + kk][n0 + 8 ng .. + 7]
  const bool dstT_vec = full && aligned16(rec.dstT) && (rec.dstT_ld & 7) == 0;
  opd_gbf16* dstT = (opd_gbf16*)rec.dstT;
  const int ng = g;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int kk = r + 32 * i;
    unsigned v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = s_tile[(8 * ng + j) * OPD_TILE + (kk ^ (ng << 2))];     // rows 8ng + j: swizzle 4 * ng
    const long k = k0 + kk, n = n0 + 8 * ng;
    if (dstT_vec) {
      *(opd_guint4*)(dstT + k * rec.dstT_ld + n) = opd_u32x4{v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16),
                                                         v[6] | (v[7] << 16)};
    } else if (k < rec.K) {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (n + j < rec.N) dstT[k * rec.dstT_ld + n + j] = (bf16_t)v[j];
    }
  }
}

extern "C" {

int mvg_refresh_operands(const void* record_table, int n_records, const void* tile_table, int n_tiles, void* stream) {
  if (n_records < 0 || n_tiles < 0) return MVG_E_BADARG;
  if (n_tiles > 0 && (mvg_any_null({record_table, tile_table}) || n_records < 1)) return MVG_E_BADARG;
  if (mvg_any_misaligned(8, {record_table, tile_table})) return MVG_E_BADARG;
  if (n_tiles == 0) return 0;
  hipLaunchKernelGGL(refresh_operands_kernel, dim3(n_tiles), dim3(OPD_THREADS), 0, (hipStream_t)stream,
                     (const OpdRecord*)record_table, n_records, (const OpdTile*)tile_table);
  MVG_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
