// In-kernel stamp recorder of the probe builds (-DCHAIN_STAMPS, -DGSAMP_STAMPS, -DTRI_STAMPS, -DWREG_STAMPS=n, -DPYRWS_STAMPS=n;
// tools/probes/stamps_*.py build, bind and parse them).  The product is built with none of these macros and gets nothing from
// this header.  A kernel's own macros (CSTAMP, TSTAMP, W2STAMP, PWSTAMP) decide what is stamped and which thread flushes;
// storage, hardware id, append and the host readers are here.
#pragma once
#if defined(CHAIN_STAMPS) || defined(GSAMP_STAMPS) || defined(TRI_STAMPS) || defined(WREG_STAMPS) || defined(PYRWS_STAMPS)
#include <hip/hip_runtime.h>

typedef unsigned long long stamp_t;

// where the calling wavefront runs: XCC_ID << 32 | HW_ID
__device__ __forceinline__ stamp_t stamp_hw_id() {
  unsigned hw, xcc;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  return ((stamp_t)xcc << 32) | hw;
}

// claims the next record of an append log and writes it; records past the capacity are counted and dropped
template <int CAP, int WORDS>
__device__ __forceinline__ void stamp_append(stamp_t* log, unsigned* count, const stamp_t* record) {
  const unsigned slot = atomicAdd(count, 1u);
  if (slot < CAP)
    for (int i = 0; i < WORDS; ++i) log[slot * WORDS + i] = record[i];
}

// -> records copied to host (at most max_records; host may be null to only count or reset), or the negated HIP error
static int stamp_read(const void* log_symbol, const void* count_symbol, unsigned cap, int words, stamp_t* host, int max_records,
                      int reset) {
  unsigned n = 0;
  hipError_t e = hipMemcpyFromSymbol(&n, count_symbol, sizeof(n));
  if (e != hipSuccess) return -(int)e;
  if (n > cap) n = cap;
  if ((int)n > max_records) n = max_records;
  if (host && n) e = hipMemcpyFromSymbol(host, log_symbol, sizeof(stamp_t) * words * n);
  if (e != hipSuccess) return -(int)e;
  if (reset) {
    const unsigned z = 0;
    e = hipMemcpyToSymbol(count_symbol, &z, sizeof(z));
    if (e != hipSuccess) return -(int)e;
  }
  return (int)n;
}

// Append log NAME: CAP records of WORDS 64-bit words and a counter, NAME_append(record) on the device, READER on the host.
#define MVG_STAMP_LOG(NAME, CAP, WORDS, READER)                                                                           \
  __device__ stamp_t NAME[(CAP) * (WORDS)];                                                                               \
  __device__ unsigned int NAME##_count;                                                                                   \
  __device__ __forceinline__ void NAME##_append(const stamp_t* record) {                                                  \
    stamp_append<CAP, WORDS>(NAME, &NAME##_count, record);                                                                \
  }                                                                                                                       \
  extern "C" int READER(stamp_t* host, int max_records, int reset) {                                                      \
    return stamp_read(&NAME, &NAME##_count, CAP, WORDS, host, max_records, reset);                                        \
  }

// Indexed log NAME: 16 words for every wavefront (WAVES per workgroup) of the first BLOCKS workgroups, NAME_at(wave, i) = word i
// of the calling workgroup's wavefront; READER copies the first n_blocks workgroups and returns the HIP error.
#define MVG_STAMP_GRID(NAME, BLOCKS, WAVES, READER)                                                                       \
  __device__ stamp_t NAME[(BLOCKS) * (WAVES) * 16];                                                                       \
  __device__ __forceinline__ stamp_t& NAME##_at(int wave, int i) { return NAME[(blockIdx.x * (WAVES) + wave) * 16 + i]; } \
  extern "C" int READER(stamp_t* host, int n_blocks) {                                                                    \
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(NAME), sizeof(stamp_t) * (WAVES) * 16 * n_blocks);                   \
  }
#endif
