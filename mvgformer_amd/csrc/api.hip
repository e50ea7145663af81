// Library identification, device probe and tuning knobs for libmvgformer_hip (host only).
#include <string.h>

#include "common.h"
#include "tuning.h"

extern "C" {

const char* mvg_version(void) { return "mvgformer_amd 0.1 (gfx950)"; }

int mvg_device_info(char* arch_out, int arch_len, int* cu_count) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return MVG_E_NOGPU;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return MVG_E_NOGPU;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return MVG_E_NOGPU;
  if (arch_out && arch_len > 0) {
    strncpy(arch_out, prop.gcnArchName, arch_len - 1);
    arch_out[arch_len - 1] = 0;
  }
  if (cu_count) *cu_count = prop.multiProcessorCount;
  return 0;
}

}  // extern "C"

// ---- tuning knobs: the instance and one row per knob.  A knob's default is its in-class initialiser (tuning.h).
MvgTuning g_tune;

namespace {
struct Knob {
  const char* key;
  int MvgTuning::*member;
  bool (*accepts)(int);
};
const Knob KNOBS[] = {
    {"linear_tiles", &MvgTuning::linear_tiles, [](int v) { return v >= 0 && v <= 2; }},
    {"f32_split", &MvgTuning::f32_split, [](int v) { return v == 0 || v == 1; }},
    {"f32h_rows", &MvgTuning::f32h_rows, [](int v) { return v == 0 || v == 32 || v == 64; }},
    {"chain_rm", &MvgTuning::chain_rm, [](int v) { return v == 64 || v == 128 || v == 256; }},
    {"wreg_grid", &MvgTuning::wreg_grid, [](int v) { return v > 0; }},
    {"bin_multi", &MvgTuning::bin_multi, [](int v) { return v == 0 || v == 1; }},
    {"auto_small", &MvgTuning::auto_small, [](int v) { return v == 0 || v == 1; }},
    {"gsamp_map", &MvgTuning::gsamp_map, [](int v) { return v >= 0 && v <= 4096; }},
    {"fwd_map", &MvgTuning::fwd_map, [](int v) { return v >= 0 && v <= 2; }},
    {"gfused_chunk", &MvgTuning::gfused_chunk, [](int v) { return v >= 0 && v <= 4096; }},
    {"gsamp_pipe", &MvgTuning::gsamp_pipe, [](int v) { return v >= 0 && v <= 2; }},
    {"chain_a_lds_pad", &MvgTuning::chain_a_lds_pad, [](int v) { return v >= 0 && v <= 120 * 1024; }},
    {"gsamp_lds_pad", &MvgTuning::gsamp_lds_pad, [](int v) { return v >= 0 && v <= 120 * 1024; }},
    {"gsamp_threads", &MvgTuning::gsamp_threads, [](int v) { return v == 128 || v == 256 || v == 512 || v == 1024; }},
};
constexpr int N_KNOBS = sizeof(KNOBS) / sizeof(KNOBS[0]);
static_assert(N_KNOBS * sizeof(int) == sizeof(MvgTuning), "one row per knob");
}  // namespace

extern "C" int mvg_set_tuning(const char* key, int value) {
  if (!key) return MVG_E_BADARG;
  for (const Knob& k : KNOBS)
    if (!strcmp(key, k.key)) {
      if (!k.accepts(value)) return MVG_E_BADARG;
      g_tune.*k.member = value;
      return 0;
    }
  return MVG_E_BADARG;
}

extern "C" int mvg_tuning_knob(int index, const char** key, int* value) {
  if (index < 0 || index >= N_KNOBS || !key || !value) return MVG_E_BADARG;
  *key = KNOBS[index].key;
  *value = g_tune.*KNOBS[index].member;
  return 0;
}
