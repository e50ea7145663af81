// Optimizer step of the training loop for gfx950: torch.nn.utils.clip_grad_norm_ followed by torch.optim.Adam / AdamW
// (lib/core/function.py:167-178, run/train_3d.py:116-146) over ALL parameter tensors of a model in three launches, with the
// reference's `if losses > 0` guard decided on the device.  No memset, no copy, no atomics, nothing read back: the step can sit
// in a HIP graph.  Every sum is taken in a fixed order in fp64, two runs on the same inputs give the same bits.
//
//   (A) optim_sumsq_kernel   one workgroup per chunk: sum of grad^2 in fp64 -> one partial per chunk
//   (B) optim_state_kernel   one workgroup: total norm, clip coefficient, loss guard, step count, per-group bias corrections
//   (C) optim_update_kernel  one workgroup per chunk: the fp32 update of p, exp_avg, exp_avg_sq and the gradient left behind
//
// The launches are driven by tables in device memory (mvg_decoder.h), so no kernel argument depends on the parameter set: one
// grid covers every tensor with MVG_OPTIM_CHUNK elements per workgroup, whatever the tensors' sizes are.
#include <math.h>

#include "exact_dev.h"

#define OPT_THREADS 256
#define OPT_WAVES (OPT_THREADS / MVG_WAVE)
#define OPT_VEC 4                                                 // elements per 16-byte access
#define OPT_ITERS (MVG_OPTIM_CHUNK / (OPT_THREADS * OPT_VEC))     // 16-byte groups per thread and chunk
static_assert(MVG_OPTIM_CHUNK % (OPT_THREADS * OPT_VEC) == 0, "a chunk is a whole number of workgroup-wide 16-byte rows");

struct OptTensor {          // MVG_OPTIM_TENSOR_WORDS x 8 bytes
  float* p;
  float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  long n;
  long group;
};
struct OptChunk {           // 8 bytes
  int tensor;
  int index;                // chunk number inside the tensor: elements [index * CHUNK, min(n, (index + 1) * CHUNK))
};
struct OptGroup {           // MVG_OPTIM_GROUP_WORDS doubles
  double lr, beta1, beta2, eps, weight_decay, decoupled;
};
struct OptGroupState {      // what (B) leaves for (C), 16 bytes per group behind the state header
  float step_size;          // lr / (1 - beta1^t)
  float bc2_sqrt;           // sqrt(1 - beta2^t)
  float decay;              // 1 - lr * weight_decay (AdamW)
  float pad;
};
struct OptState {           // MVG_OPTIM_STATE_HEADER bytes
  long step;                // optimizer steps taken; the only field that lives from call to call
  double total_norm;        // of this call: sqrt(sum grad^2), before clipping
  float clip_coef;
  int skip;
  float loss_seen;          // the loss scalar (B) tested, 0 without one
  int pad[9];
};
static_assert(sizeof(OptTensor) == MVG_OPTIM_TENSOR_WORDS * 8 && sizeof(OptChunk) == 8, "table layout of mvg_decoder.h");
static_assert(sizeof(OptGroup) == MVG_OPTIM_GROUP_WORDS * 8 && sizeof(OptGroupState) == MVG_OPTIM_STATE_PER_GROUP, "table layout");
static_assert(sizeof(OptState) == MVG_OPTIM_STATE_HEADER, "state header of mvg_decoder.h");

// The tensors' pointers come out of a table, so the compiler takes them for generic (flat) addresses; they are global memory.
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) f32x4 gf32x4;
__device__ __forceinline__ gfloat* opt_global(float* p) { return (gfloat*)p; }
__device__ __forceinline__ f32x4 opt_load4(gfloat* p) { return *(gf32x4*)p; }
__device__ __forceinline__ void opt_store4(gfloat* p, f32x4 v) { *(gf32x4*)p = v; }

// Thread t of a chunk owns the 16-byte groups t, t + 256, ... of it, on the vector path and on the scalar path alike, so the
// order of every sum is a function of the element index alone.
__global__ __launch_bounds__(OPT_THREADS) void optim_sumsq_kernel(const OptTensor* __restrict__ tensors,
                                                                  const OptChunk* __restrict__ chunks, int n_tensors,
                                                                  double* __restrict__ partial) {
  __shared__ double s_red[OPT_WAVES];
  const OptChunk c = chunks[blockIdx.x];
  double acc = 0.0;
  if (c.tensor >= 0 && c.tensor < n_tensors && c.index >= 0) {
    const OptTensor t = tensors[c.tensor];
    const long base = (long)c.index * MVG_OPTIM_CHUNK;
    const bool vec = aligned16(t.grad);
    gfloat* grad = opt_global(t.grad);
#pragma unroll
    for (int k = 0; k < OPT_ITERS; ++k) {
      const long i = base + (long)(threadIdx.x + k * OPT_THREADS) * OPT_VEC;
      if (vec && i + OPT_VEC <= t.n) {
        const f32x4 g = opt_load4(grad + i);
#pragma unroll
        for (int e = 0; e < OPT_VEC; ++e) acc += (double)g[e] * (double)g[e];
      } else {
        for (int e = 0; e < OPT_VEC; ++e)
          if (i + e < t.n) {
            const double g = grad[i + e];
            acc += g * g;
          }
      }
    }
  }
  const double s = block_sum<OPT_WAVES>(acc, s_red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// One workgroup.  Thread t adds the partials t, t + 256, ... in ascending chunk order, then the fixed-order workgroup sum.
__global__ __launch_bounds__(OPT_THREADS) void optim_state_kernel(const double* __restrict__ partial, int n_chunks,
                                                                  const OptGroup* __restrict__ groups, int n_groups,
                                                                  const float* __restrict__ loss, float max_norm,
                                                                  OptState* __restrict__ state, float* __restrict__ norm_out) {
  __shared__ double s_red[OPT_WAVES];
  __shared__ long s_step;
  double acc = 0.0;
  for (int i = threadIdx.x; i < n_chunks; i += OPT_THREADS) acc += partial[i];
  const double sum = block_sum<OPT_WAVES>(acc, s_red);
  if (threadIdx.x == 0) {
    const double norm = sqrt(sum);
    double coef = 1.0;
    if (max_norm > 0.f) {                                         // clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max = 1)
      coef = (double)max_norm / (norm + 1e-6);
      coef = coef > 1.0 ? 1.0 : coef;                             // a NaN norm stays a NaN coefficient, as in torch
    }
    const float lv = loss ? *loss : 0.f;
    const int skip = loss ? !(lv > 0.f) : 0;                      // function.py:167 `if losses > 0`: 0, negative and NaN skip
    const long step = state->step + (skip ? 0 : 1);
    state->step = step;
    state->total_norm = norm;
    state->clip_coef = (float)coef;
    state->skip = skip;
    state->loss_seen = lv;
    if (norm_out) *norm_out = (float)norm;
    s_step = step;
  }
  __syncthreads();
  const double t = (double)s_step;
  OptGroupState* gs = reinterpret_cast<OptGroupState*>(state + 1);
  for (int g = threadIdx.x; g < n_groups; g += OPT_THREADS) {
    const OptGroup h = groups[g];
    const double bc1 = 1.0 - pow(h.beta1, t), bc2 = 1.0 - pow(h.beta2, t);
    OptGroupState o;
    o.step_size = (float)(h.lr / bc1);
    o.bc2_sqrt = (float)sqrt(bc2);
    o.decay = (float)(1.0 - h.lr * h.weight_decay);
    o.pad = 0.f;
    gs[g] = o;
  }
}

struct OptHyper {
  float b1, omb1, b2, omb2, eps, wd, step_size, bc2_sqrt, decay, clip;
  bool decoupled, store_grad, zero_grad;
};

// torch.optim.Adam's single-tensor order of operations in fp32
__device__ __forceinline__ void opt_update1(const OptHyper& h, float& p, float& g, float& m, float& v) {
  g *= h.clip;
  float ge = g;
  if (h.wd != 0.f) {
    if (h.decoupled) p *= h.decay; else ge += h.wd * p;
  }
  m = h.b1 * m + h.omb1 * ge;
  v = h.b2 * v + h.omb2 * ge * ge;
  const float denom = sqrtf(v) / h.bc2_sqrt + h.eps;
  p -= h.step_size * (m / denom);
}

__global__ __launch_bounds__(OPT_THREADS) void optim_update_kernel(const OptTensor* __restrict__ tensors,
                                                                   const OptChunk* __restrict__ chunks, int n_tensors,
                                                                   const OptGroup* __restrict__ groups, int n_groups,
                                                                   const OptState* __restrict__ state, int zero_grad) {
  const OptChunk c = chunks[blockIdx.x];
  if (c.tensor < 0 || c.tensor >= n_tensors || c.index < 0) return;
  const OptTensor t = tensors[c.tensor];
  if (t.group < 0 || t.group >= n_groups) return;
  const long base = (long)c.index * MVG_OPTIM_CHUNK;
  const bool skip = state->skip != 0;
  if (skip && !zero_grad) return;
  const bool vec = aligned16(t.p) && aligned16(t.grad) && aligned16(t.exp_avg) && aligned16(t.exp_avg_sq);
  gfloat* tp = opt_global(t.p);
  gfloat* tg = opt_global(t.grad);
  gfloat* tm = opt_global(t.exp_avg);
  gfloat* tv = opt_global(t.exp_avg_sq);

  if (skip) {                                                     // a skipped step still leaves the gradients zeroed
#pragma unroll
    for (int k = 0; k < OPT_ITERS; ++k) {
      const long i = base + (long)(threadIdx.x + k * OPT_THREADS) * OPT_VEC;
      if (vec && i + OPT_VEC <= t.n) {
        opt_store4(tg + i, f32x4{0.f, 0.f, 0.f, 0.f});
      } else {
        for (int e = 0; e < OPT_VEC; ++e)
          if (i + e < t.n) tg[i + e] = 0.f;
      }
    }
    return;
  }

  const OptGroup hg = groups[t.group];
  const OptGroupState gs = reinterpret_cast<const OptGroupState*>(state + 1)[t.group];
  OptHyper h;
  h.b1 = (float)hg.beta1; h.omb1 = (float)(1.0 - hg.beta1);
  h.b2 = (float)hg.beta2; h.omb2 = (float)(1.0 - hg.beta2);
  h.eps = (float)hg.eps; h.wd = (float)hg.weight_decay;
  h.step_size = gs.step_size; h.bc2_sqrt = gs.bc2_sqrt; h.decay = gs.decay;
  h.clip = state->clip_coef;
  h.decoupled = hg.decoupled != 0.0;
  h.zero_grad = zero_grad != 0;
  h.store_grad = h.zero_grad || h.clip != 1.0f;                   // grad * 1.0f is the stored value: no write needed

#pragma unroll
  for (int k = 0; k < OPT_ITERS; ++k) {
    const long i = base + (long)(threadIdx.x + k * OPT_THREADS) * OPT_VEC;
    if (vec && i + OPT_VEC <= t.n) {
      f32x4 p = opt_load4(tp + i), g = opt_load4(tg + i), m = opt_load4(tm + i), v = opt_load4(tv + i);
#pragma unroll
      for (int e = 0; e < OPT_VEC; ++e) {
        float pe = p[e], ge = g[e], me = m[e], ve = v[e];
        opt_update1(h, pe, ge, me, ve);
        p[e] = pe; g[e] = h.zero_grad ? 0.f : ge; m[e] = me; v[e] = ve;
      }
      opt_store4(tp + i, p);
      opt_store4(tm + i, m);
      opt_store4(tv + i, v);
      if (h.store_grad) opt_store4(tg + i, g);
    } else {
      for (int e = 0; e < OPT_VEC; ++e)
        if (i + e < t.n) {
          float pe = tp[i + e], ge = tg[i + e], me = tm[i + e], ve = tv[i + e];
          opt_update1(h, pe, ge, me, ve);
          tp[i + e] = pe;
          tm[i + e] = me;
          tv[i + e] = ve;
          if (h.store_grad) tg[i + e] = h.zero_grad ? 0.f : ge;
        }
    }
  }
}

extern "C" {

size_t mvg_optim_workspace(int n_chunks) {
  if (n_chunks < 0) return 0;
  return (size_t)(n_chunks > 0 ? n_chunks : 1) * sizeof(double);
}

int mvg_optim_step(const void* tensor_table, int n_tensors, const void* chunk_table, int n_chunks, const void* group_table,
                   int n_groups, void* state, size_t state_bytes, void* workspace, size_t workspace_bytes, const float* loss,
                   float max_norm, int zero_grad, float* norm_out, void* stream) {
  if (mvg_any_null({group_table, state, workspace})) return MVG_E_BADARG;
  if (n_tensors < 0 || n_chunks < 0 || n_groups < 1 || n_groups > MVG_OPTIM_MAX_GROUPS) return MVG_E_BADARG;
  if (n_chunks > 0 && (mvg_any_null({tensor_table, chunk_table}) || n_tensors < 1)) return MVG_E_BADARG;
  if (mvg_any_misaligned(8, {tensor_table, chunk_table, group_table, state, workspace})) return MVG_E_BADARG;
  if (mvg_any_misaligned(4, {loss, norm_out})) return MVG_E_BADARG;      // both optional
  if (state_bytes < (size_t)MVG_OPTIM_STATE_HEADER + (size_t)n_groups * MVG_OPTIM_STATE_PER_GROUP) return MVG_E_BADARG;
  if (workspace_bytes < mvg_optim_workspace(n_chunks)) return MVG_E_BADARG;
  if (!(max_norm == max_norm)) return MVG_E_BADARG;
  const OptTensor* tensors = (const OptTensor*)tensor_table;
  const OptChunk* chunks = (const OptChunk*)chunk_table;
  const OptGroup* groups = (const OptGroup*)group_table;
  if (n_chunks > 0) {
    hipLaunchKernelGGL(optim_sumsq_kernel, dim3(n_chunks), dim3(OPT_THREADS), 0, (hipStream_t)stream, tensors, chunks, n_tensors,
                       (double*)workspace);
    MVG_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(optim_state_kernel, dim3(1), dim3(OPT_THREADS), 0, (hipStream_t)stream, (const double*)workspace, n_chunks,
                     groups, n_groups, loss, max_norm, (OptState*)state, norm_out);
  MVG_LAUNCH_CHECK();
  if (n_chunks > 0) {
    hipLaunchKernelGGL(optim_update_kernel, dim3(n_chunks), dim3(OPT_THREADS), 0, (hipStream_t)stream, tensors, chunks, n_tensors,
                       groups, n_groups, (const OptState*)state, zero_grad);
    MVG_LAUNCH_CHECK();
  }
  return 0;
}

}  // extern "C"
