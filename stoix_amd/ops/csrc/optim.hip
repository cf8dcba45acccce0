// Fused optimiser kernels (K8/K9 of SURVEY.md §2.9).
//
// The reference's optax chain(clip_by_global_norm, adam) + apply_updates +
// incremental_update (ff_ppo.py:456-463, ff_dqn.py:207-209) become three
// kernels over ONE flat parameter buffer: a grid-stride squared-norm
// reduction (one atomicAdd per block), a fused clip+Adam update reading the
// norm from device memory (no host sync inside the graph), and a polyak
// target update. All are memory-bound: loads are float4-vectorised.
#include "common.h"
#include "launchers.h"

// partial squared-norm: block-level shuffle reduction + one atomic per block
extern "C" __global__ void grad_sqnorm_kernel(
    const float* __restrict__ grad, float* __restrict__ out, long n) {
  long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  float acc = 0.0f;
  long nvec = n / 4;  // flat buffers are 16B-aligned (torch allocator)
  const float4* g4 = reinterpret_cast<const float4*>(grad);
  for (long v = tid; v < nvec; v += stride) {
    float4 g = g4[v];
    acc += g.x * g.x + g.y * g.y + g.z * g.z + g.w * g.w;
  }
  for (long j = nvec * 4 + tid; j < n; j += stride) acc += grad[j] * grad[j];
  // wave reduce (wave64): wave_sum_down() spelled out, see
  // grad_sqnorm_bf16_kernel
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
  __shared__ float warp_sums[16];
  int lane = threadIdx.x & 63;
  int wid = threadIdx.x >> 6;
  if (lane == 0) warp_sums[wid] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.0f;
    int nw = (blockDim.x + 63) / 64;
    for (int w = 0; w < nw; ++w) s += warp_sums[w];
    atomicAdd(out, s);
  }
}

// fused global-norm clip + Adam. sqnorm is a 1-element device buffer written
// by grad_sqnorm_kernel; step_t a device int64 incremented by the caller
// kernel-side (adam_inc) so the whole sequence is graph-replayable.
extern "C" __global__ void adam_update_kernel(
    float* __restrict__ param,
    const float* __restrict__ grad,
    float* __restrict__ exp_avg,
    float* __restrict__ exp_avg_sq,
    const float* __restrict__ sqnorm,   // [1]
    const long* __restrict__ step_t,    // [1] (already incremented)
    long n, float lr, float beta1, float beta2, float eps, float max_norm) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  float clip = 1.0f;
  if (max_norm > 0.0f) {
    float norm = sqrtf(*sqnorm);
    clip = (norm > max_norm) ? (max_norm / (norm + 1e-6f)) : 1.0f;
  }
  long t = *step_t;
  float bc1 = 1.0f - powf(beta1, (float)t);
  float bc2 = 1.0f - powf(beta2, (float)t);
  for (; i < n; i += stride) {
    float g = grad[i] * clip;
    float m = exp_avg[i] = beta1 * exp_avg[i] + (1.0f - beta1) * g;
    float v = exp_avg_sq[i] = beta2 * exp_avg_sq[i] + (1.0f - beta2) * g * g;
    float mhat = m / bc1;
    float vhat = v / bc2;
    param[i] -= lr * mhat / (sqrtf(vhat) + eps);
  }
}

extern "C" __global__ void adam_prologue_kernel(float* __restrict__ sqnorm,
                                                long* __restrict__ step_t) {
  adam_prologue(sqnorm, step_t);
}

// bf16-gradient variants for the fused update path (stoix_amd/ops/csrc/
// mlp.hip): the minibatch backward produces bf16 grads written straight
// into one flat buffer by the wgrad GEMMs; the RCCL all-reduce runs on the
// bf16 buffer; Adam reads bf16 grads, keeps the fp32 master param, and
// mirrors the updated param to bf16 (the GEMM/rollout-kernel weights) in
// the same pass — no separate cast kernels anywhere in the loop.
#include <hip/hip_bf16.h>
typedef __bf16 opt_bf16;
typedef __bf16 opt_bf16x8 __attribute__((ext_vector_type(8)));

// The two pieces adam_update_bf16_kernel and adam_pair_kernel share, which
// is what keeps the paired tail bit-equal to the single-chain launches.

// Factor on every gradient element, max_norm > 0: grad_scale, times the
// global-norm clip where the scaled norm sqrt(sq) * grad_scale exceeds it.
DEV_INLINE float adam_clip_factor(float sq, float max_norm, float grad_scale) {
  float norm = sqrtf(sq) * grad_scale;
  return norm > max_norm ? grad_scale * max_norm / (norm + 1e-6f) : grad_scale;
}

// Element i: moments, fp32 master param, bf16 mirror (if any).
DEV_INLINE void adam_step_bf16(float* param, const opt_bf16* grad,
                               float* exp_avg, float* exp_avg_sq,
                               opt_bf16* param_bf16, long i, float clip,
                               float lr, float beta1, float beta2, float eps,
                               float bc1, float bc2) {
  float g = (float)grad[i] * clip;
  float m = exp_avg[i] = beta1 * exp_avg[i] + (1.0f - beta1) * g;
  float v = exp_avg_sq[i] = beta2 * exp_avg_sq[i] + (1.0f - beta2) * g * g;
  float p = param[i] - lr * (m / bc1) / (sqrtf(v / bc2) + eps);
  param[i] = p;
  if (param_bf16) {
    opt_bf16* mirror = param_bf16 + i;
    *mirror = (opt_bf16)p;
  }
}

// `partials` non-null: block b stores its sum in partials[b] and
// adam_update_bf16_kernel adds them up in index order, so the norm (hence
// the clip factor and every clipped update) is bit-reproducible run to run.
// Null: one float atomicAdd per block into *out (order varies in the last
// bits).
extern "C" __global__ void grad_sqnorm_bf16_kernel(
    const opt_bf16* __restrict__ grad, float* __restrict__ out,
    float* __restrict__ partials, long n) {
  long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  float acc = 0.0f;
  long nvec = n / 8;
  const opt_bf16x8* g8 = reinterpret_cast<const opt_bf16x8*>(grad);
  for (long v = tid; v < nvec; v += stride) {
    opt_bf16x8 g = g8[v];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float x = (float)g[j];
      acc += x * x;
    }
  }
  for (long j = nvec * 8 + tid; j < n; j += stride) {
    float x = (float)grad[j];
    acc += x * x;
  }
  // wave_sum_down() (common.h) spelled out: through the helper the compiler
  // orders two instructions of the lane-0 store differently, and this
  // kernel's code is kept as it was. The adds are the helper's.
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
  __shared__ float warp_sums[16];
  int lane = threadIdx.x & 63;
  int wid = threadIdx.x >> 6;
  if (lane == 0) warp_sums[wid] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.0f;
    int nw = (blockDim.x + 63) / 64;
    for (int w = 0; w < nw; ++w) s += warp_sums[w];
    if (partials)
      partials[blockIdx.x] = s;
    else
      atomicAdd(out, s);
  }
}

// n_partials > 0: sqnorm[1 .. n_partials] hold grad_sqnorm_bf16_kernel's
// per-block sums; every block adds them in the same fixed order (wave 0:
// lane-strided, then the shuffle tree) and block 0 stores the total in
// sqnorm[0]. n_partials == 0: sqnorm[0] already holds the atomic total.
extern "C" __global__ void adam_update_bf16_kernel(
    float* __restrict__ param, const opt_bf16* __restrict__ grad,
    float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq,
    float* __restrict__ sqnorm, const long* __restrict__ step_t,
    opt_bf16* __restrict__ param_bf16, long n, float lr, float beta1,
    float beta2, float eps, float max_norm, float grad_scale,
    int n_partials) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  float clip = grad_scale;
  if (max_norm > 0.0f) {
    float sq;
    if (n_partials > 0) {
      __shared__ float total;
      if (threadIdx.x < 64) {
        float acc = 0.0f;
        for (int p = threadIdx.x; p < n_partials; p += 64)
          acc += sqnorm[1 + p];
        acc = wave_sum_down(acc);
        if (threadIdx.x == 0) {
          total = acc;
          if (blockIdx.x == 0) sqnorm[0] = acc;
        }
      }
      __syncthreads();
      sq = total;
    } else {
      sq = *sqnorm;
    }
    clip = adam_clip_factor(sq, max_norm, grad_scale);
  }
  long t = *step_t;
  float bc1 = 1.0f - powf(beta1, (float)t);
  float bc2 = 1.0f - powf(beta2, (float)t);
  for (; i < n; i += stride)
    adam_step_bf16(param, grad, exp_avg, exp_avg_sq, param_bf16, i, clip, lr,
                   beta1, beta2, eps, bc1, bc2);
}

extern "C" void launch_fused_adam_bf16(float* param, const void* grad,
                                       float* exp_avg, float* exp_avg_sq,
                                       float* sqnorm, long* step_t,
                                       void* param_bf16, long n, float lr,
                                       float beta1, float beta2, float eps,
                                       float max_norm, float grad_scale,
                                       int do_prologue, long sqnorm_len,
                                       void* stream) {
  // sqnorm_len: floats in the sqnorm buffer. With room for one partial per
  // block behind sqnorm[0] the norm is summed in a fixed order
  // (reproducible); a 1-element buffer keeps the atomic form.
  hipStream_t s = (hipStream_t)stream;
  // the prologue (zero sqnorm, step+1) can ride along in slab_reduce
  // (wgrad.hip) when that kernel precedes this one in the same stream
  if (do_prologue)
    hipLaunchKernelGGL(adam_prologue_kernel, dim3(1), dim3(1), 0, s, sqnorm,
                       step_t);
  int threads = 256;
  int blocks = flat_blocks(n / 8, threads);
  int n_partials = 0;
  if (max_norm > 0.0f) {
    bool ordered = sqnorm_len >= 1 + (long)blocks;
    if (ordered) n_partials = blocks;
    hipLaunchKernelGGL(grad_sqnorm_bf16_kernel, dim3(blocks), dim3(threads),
                       0, s, (const opt_bf16*)grad, sqnorm,
                       ordered ? sqnorm + 1 : (float*)nullptr, n);
  }
  hipLaunchKernelGGL(adam_update_bf16_kernel, dim3(flat_blocks(n, threads)),
                     dim3(threads), 0, s, param, (const opt_bf16*)grad,
                     exp_avg, exp_avg_sq, sqnorm, step_t,
                     (opt_bf16*)param_bf16, n, lr, beta1, beta2, eps, max_norm,
                     grad_scale, n_partials);
}

// Both chains' clip + Adam in one launch (blockIdx.y picks the chain, an
// AdamChain of launchers.h), for the two-launch optimiser tail:
// slab_reduce_norm_pair (wgrad.hip) has left the finished squared norm in
// sqnorm[0], so this is adam_update_bf16_kernel's n_partials == 0 form, by
// the same adam_clip_factor() and adam_step_bf16().
extern "C" __global__ void adam_pair_kernel(AdamChain c0, AdamChain c1,
                                            float beta1, float beta2,
                                            float eps, float max_norm,
                                            float grad_scale) {
  const AdamChain c = blockIdx.y ? c1 : c0;
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  float clip = grad_scale;
  if (max_norm > 0.0f)
    clip = adam_clip_factor(*c.sqnorm, max_norm, grad_scale);
  long t = *c.step_t;
  float bc1 = 1.0f - powf(beta1, (float)t);
  float bc2 = 1.0f - powf(beta2, (float)t);
  for (; i < c.n; i += stride)
    adam_step_bf16(c.param, (const opt_bf16*)c.grad, c.exp_avg, c.exp_avg_sq,
                   (opt_bf16*)c.param_bf16, i, clip, c.lr, beta1, beta2, eps,
                   bc1, bc2);
}

extern "C" void launch_adam_pair(const AdamChain& c0, const AdamChain& c1,
                                 float beta1, float beta2, float eps,
                                 float max_norm, float grad_scale,
                                 void* stream) {
  int threads = 256;
  int blocks = flat_blocks(c0.n > c1.n ? c0.n : c1.n, threads);
  hipLaunchKernelGGL(adam_pair_kernel, dim3(blocks, 2), dim3(threads), 0,
                     (hipStream_t)stream, c0, c1, beta1, beta2, eps, max_norm,
                     grad_scale);
}

// polyak: target <- tau * online + (1 - tau) * target (ff_dqn.py:207-209)
extern "C" __global__ void polyak_kernel(const float* __restrict__ online,
                                         float* __restrict__ target,
                                         long n, float tau) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < n; i += stride)
    target[i] = tau * online[i] + (1.0f - tau) * target[i];
}

// ----------------------------------------------------------- host launchers
extern "C" void launch_fused_adam(float* param, const float* grad,
                                  float* exp_avg, float* exp_avg_sq,
                                  float* sqnorm, long* step_t, long n,
                                  float lr, float beta1, float beta2,
                                  float eps, float max_norm, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(adam_prologue_kernel, dim3(1), dim3(1), 0, s, sqnorm, step_t);
  int threads = 256;
  if (max_norm > 0.0f) {
    hipLaunchKernelGGL(grad_sqnorm_kernel, dim3(flat_blocks(n / 4, threads)),
                       dim3(threads), 0, s, grad, sqnorm, n);
  }
  hipLaunchKernelGGL(adam_update_kernel, dim3(flat_blocks(n, threads)),
                     dim3(threads), 0, s, param, grad, exp_avg, exp_avg_sq,
                     sqnorm, step_t, n, lr, beta1, beta2, eps, max_norm);
}

extern "C" void launch_polyak(const float* online, float* target, long n,
                              float tau, void* stream) {
  int threads = 256;
  hipLaunchKernelGGL(polyak_kernel, dim3(flat_blocks(n, threads)),
                     dim3(threads), 0,
                     (hipStream_t)stream, online, target, n, tau);
}
