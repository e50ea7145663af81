// Kernel-variant knobs of libmvgformer_hip (mvg_set_tuning / mvg_tuning_knob, include/mvg_decoder.h): one process-global
// instance, read by the host launch code only.  Keys and accepted values: the table in api.hip.
#pragma once

struct MvgTuning {
  int linear_tiles = 1;     // tuning knob "linear_tiles": 0 = always 128 x 128 tiles (rounds 1-2)
  int f32_split = 1;        // tuning knob "f32_split": 1 = fp32 GEMMs as six bf16 MFMAs on 3-way split operands (see gemm.hip)
  int f32h_rows = 0;        // tuning knob "f32h_rows": rows per tile of the two fp32 chains (0 = by the row count | 32 | 64); both sizes sum a row identically
  int chain_rm = 128;       // tuning knob "chain_rm": rows per workgroup of chain A (64 | 128 | 256); 128: 65 -> 55 us (half the weight
                            // bytes per row).  Geometries measured and deleted (rounds 1-4, Appendix A of DESIGN.md): 8 wavefronts for
                            // chain A (93 vs 79 us), 4 wavefronts / row-block split / fragment rings of 8 and 16 for chain B.
  int wreg_grid = 512;      // tuning knob (mvg_set_tuning "wreg_grid"): persistent workgroups
  int bin_multi = 1;        // tuning knob "bin_multi": 0 = always the single-workgroup binning kernel
  int auto_small = 1;       // tuning knob "auto_small": small launches pick their own workgroup / tile sizes (see mvg_msda_gsamp);
                            // chain A and chain B: launches with few rows pick smaller tiles (bit-identical rows)
  int gsamp_map = 4;        // tuning knob "gsamp_map": 0 = head per XCD (159 us), n > 0 = chunks of n slot blocks per
                            // XCD with their 8 heads back to back (1..4: 155 us, 8: 159, 16: 168, 64: 243)
  int fwd_map = 1;          // tuning knob "fwd_map": mvg_msda_forward, 0 = a wavefront takes the M heads of a query, 1 = one head per workgroup (D = 32: per-sample arithmetic shared out over the unit's 8 lanes), 2 = one head per workgroup, every lane computes every sample
  int gfused_chunk = 4;     // tuning knob "gfused_chunk": hp kernel, 0 = one head per XCD (270 us at cfg-2), n > 0 = chunks of n pair blocks per XCD with their 8 heads back to back (1..4: 252 us, 16: 263)
  int gsamp_pipe = 0;       // tuning knob "gsamp_pipe": gathers double-buffered in half batches (93 VGPRs) -- 0 = from 32 768 pairs per launch on, 1 = always, 2 = never
  int chain_a_lds_pad = 0;  // probe knob "chain_a_lds_pad": unused dynamic LDS per chain-A workgroup (caps the workgroups per CU)
  int gsamp_lds_pad = 0;    // probe knob "gsamp_lds_pad": bytes of unused dynamic LDS per workgroup (caps the workgroups per CU)
  int gsamp_threads = 256;  // tuning knob "gsamp_threads": workgroup size of msda_gsamp_kernel (256 | 512 | 1024)
};

extern MvgTuning g_tune;
