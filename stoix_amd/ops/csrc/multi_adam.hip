// Multi-tensor optimiser tail: global-norm clip + Adam + polyak for up to
// MADAM_MAX_CHAINS chains of separately allocated fp32 tensors, in two
// launches (K8/K9 of SURVEY.md for the learners whose state is torch's own:
// p, p.grad and the exp_avg / exp_avg_sq / step of torch.optim.Adam).
//
// Per chain, in torch's formulation (clip_grad_norm_, capturable Adam,
// _foreach polyak), fp32:
//   norm = sqrt(sum over the chain's grads of g^2)
//   coef = max_norm / (norm + 1e-6);  coef = coef > 1 ? 1 : coef   (NaN stays)
//   g    = grad * coef                          (grad itself is not rewritten)
//   t    = step + 1                             (per parameter, as torch keeps it)
//   m    = m + (1 - b1) (g - m)        v = b2 v + ((1 - b2) g) g
//   p    = p - ((lr / (1 - b1^t)) m) / (sqrt(v) / sqrt(1 - b2^t) + eps)
//   tgt  = tgt (1 - tau) + tau p                (chains with a target)
//
// A parameter without a gradient is skipped as torch's Adam skips it; where
// it has a target, its entry stays in the table with a null g and only the
// polyak line runs.
//
// Work split. The host passes one table by value (launchers.h): per tensor
// the six pointers, numel, its chain and its first block; per chain the
// hyper-parameters and its block range. A 256-thread block owns one chunk of
// MADAM_CHUNK elements of one tensor and finds the tensor by a binary search
// of the first-block prefix: the table is a kernel argument and the block
// index is uniform, so the search is scalar loads with no divergence. The
// table carries addresses only, so a host that rebuilds it per call (the
// gradients of zero_grad(set_to_none=True) move every step) reads pointers
// and copies nothing to the device.
//
// Launch A (multi_adam_norm_kernel): a block of a clipped chain sums the
// squares of its chunk (16-byte loads when the gradient is 16-byte aligned,
// by element otherwise: a parameter may be a view at any 4-byte offset),
// reduces over the wave with the __shfl_down tree, over the 4 waves through
// LDS in wave order, and stores ONE partial into partials[block]. No float
// atomics, no ticket. Thread 0 of a tensor's first block stores step + 1;
// nothing else in launch A touches step. Blocks of an unclipped chain do only
// that.
//
// Launch B (multi_adam_update_kernel): wave 0 of EVERY block adds its chain's
// partials (lane l takes l, l + 64, ... ascending, then the same tree), so
// every block of a chain holds the same bits of the norm; lane 0 forms coef,
// the step size and sqrt(1 - b2^t) once and broadcasts them through LDS. The
// element loop then reads p, g, m, v, tgt once and writes p, m, v, tgt once,
// with the same vector / by-element split. Every order is fixed: two runs on
// the same inputs give the same bits.
//
// b^t: t is torch's fp32 step, an integer. 1 - b^t cancels (b2 = 0.999,
// t = 1: three digits lost), so an fp32 powf within 1 ulp would leave
// 1 - b2^t off by 1000 ulp where torch's pow(b, 1) is exact. The two powers
// are taken in fp64 by the one lane that needs them and 1 - b^t is rounded to
// fp32 once: never further from the exact value than torch's own fp32 result.
//
// FMA contraction is off for the file, so every product and sum above rounds
// as the separate torch kernels round it. Built as its own object with packed
// fp32 operations off (ops/build.py).
//
// Resources (-Rpass-analysis=kernel-resource-usage, gfx950): the norm kernel
// 10 VGPRs, 16 B LDS; the update kernel 48 VGPRs, 12 B LDS; both no AGPRs, no
// scratch, 8 waves/SIMD, no packed fp32 instruction. The table is 3816 bytes
// of the 3824-byte kernel-argument segment.
#include "common.h"
#include "launchers.h"

#pragma clang fp contract(off)

#define MADAM_THREADS 256
#define MADAM_WAVES (MADAM_THREADS / 64)

// The tensor that owns block blk: the last i with first_block[i] <= blk.
// Uniform over the block.
DEV_INLINE int madam_find_tensor(const MultiAdamTable& T, unsigned int blk) {
  int lo = 0, hi = T.n_tensors - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((unsigned int)T.t[mid].first_block <= blk)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

DEV_INLINE bool madam_aligned16(const void* a) {
  return ((uintptr_t)a & 15) == 0;
}

__global__ __launch_bounds__(MADAM_THREADS)
void multi_adam_norm_kernel(const MultiAdamTable T, float* __restrict__ partials) {
  __shared__ float wave_part[MADAM_WAVES];
  const unsigned int blk = blockIdx.x;
  const MultiAdamTensor& t = T.t[madam_find_tensor(T, blk)];
  const unsigned int chunk = blk - t.first_block;
  const int tid = threadIdx.x;
  if (chunk == 0 && tid == 0 && t.g) *t.step = *t.step + 1.0f;
  if (!T.c[t.chain].clip) return;  // uniform: the whole block leaves

  // a tensor without a gradient (polyak only) adds 0 to its chain's norm
  const unsigned int base = chunk * MADAM_CHUNK;
  const unsigned int len =
      t.g ? min((unsigned int)MADAM_CHUNK, t.numel - base) : 0u;
  const float* __restrict__ g = t.g + base;
  float acc = 0.0f;
  const unsigned int nvec = madam_aligned16(g) ? len / 4 : 0;
  for (unsigned int i = tid; i < nvec; i += MADAM_THREADS) {
    const float4 x = ((const float4*)g)[i];
    acc += x.x * x.x;
    acc += x.y * x.y;
    acc += x.z * x.z;
    acc += x.w * x.w;
  }
  for (unsigned int i = nvec * 4 + tid; i < len; i += MADAM_THREADS) {
    const float x = g[i];
    acc += x * x;
  }
  acc = wave_sum_down(acc);
  if ((tid & 63) == 0) wave_part[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    float s = wave_part[0];
#pragma unroll
    for (int w = 1; w < MADAM_WAVES; ++w) s += wave_part[w];
    partials[blk] = s;
  }
}

// One element of the chain. The scalars are the block's; tgt may be null.
struct MadamScalars {
  float coef, step_size, bc2_sqrt;
};

DEV_INLINE void madam_element(float gr, float& p, float& m, float& v,
                              const MadamScalars& s, const MultiAdamChain& c) {
  const float g = gr * s.coef;
  m = m + c.omb1 * (g - m);
  v = c.b2 * v + (c.omb2 * g) * g;
  const float denom = sqrtf(v) / s.bc2_sqrt + c.eps;
  p = p - (s.step_size * m) / denom;
}

DEV_INLINE float madam_polyak(float tgt, float p, const MultiAdamChain& c) {
  return tgt * c.omt + c.tau * p;
}

__global__ __launch_bounds__(MADAM_THREADS)
void multi_adam_update_kernel(const MultiAdamTable T,
                              const float* __restrict__ partials) {
  __shared__ MadamScalars bcast;
  const unsigned int blk = blockIdx.x;
  const MultiAdamTensor& t = T.t[madam_find_tensor(T, blk)];
  const MultiAdamChain& c = T.c[t.chain];
  const int tid = threadIdx.x;
  const unsigned int base = (blk - t.first_block) * MADAM_CHUNK;
  const unsigned int len = min((unsigned int)MADAM_CHUNK, t.numel - base);

  if (!t.g) {
    // No gradient this step: torch's Adam skips the parameter, the polyak of
    // its target still runs. Uniform: the whole block takes this path.
    for (unsigned int i = tid; i < len; i += MADAM_THREADS)
      t.tgt[base + i] = madam_polyak(t.tgt[base + i], t.p[base + i], c);
    return;
  }

  if (tid < 64) {
    float sq = 0.0f;
    if (c.clip) {
      for (unsigned int k = tid; k < c.part_count; k += 64)
        sq += partials[c.part_begin + k];
      sq = wave_sum_down(sq);
    }
    if (tid == 0) {
      float coef = 1.0f;
      if (c.clip) {
        coef = c.max_norm / (sqrtf(sq) + 1e-6f);
        coef = coef > 1.0f ? 1.0f : coef;
      }
      const double step = (double)*t.step;  // launch A left step + 1 here
      const float bc1 = (float)(1.0 - pow((double)c.b1, step));
      const float bc2 = (float)(1.0 - pow((double)c.b2, step));
      const float lr = c.lr_ptr ? *c.lr_ptr : c.lr;
      bcast.coef = coef;
      bcast.step_size = lr / bc1;
      bcast.bc2_sqrt = sqrtf(bc2);
    }
  }
  __syncthreads();
  const MadamScalars s = bcast;

  const float* __restrict__ g = t.g + base;
  float* __restrict__ p = t.p + base;
  float* __restrict__ m = t.m + base;
  float* __restrict__ v = t.v + base;
  float* __restrict__ tgt = t.tgt ? t.tgt + base : nullptr;
  const bool vec = madam_aligned16(g) && madam_aligned16(p) &&
                   madam_aligned16(m) && madam_aligned16(v) &&
                   madam_aligned16(tgt);
  const unsigned int nvec = vec ? len / 4 : 0;
  for (unsigned int i = tid; i < nvec; i += MADAM_THREADS) {
    const float4 g4 = ((const float4*)g)[i];
    float4 p4 = ((float4*)p)[i], m4 = ((float4*)m)[i], v4 = ((float4*)v)[i];
    madam_element(g4.x, p4.x, m4.x, v4.x, s, c);
    madam_element(g4.y, p4.y, m4.y, v4.y, s, c);
    madam_element(g4.z, p4.z, m4.z, v4.z, s, c);
    madam_element(g4.w, p4.w, m4.w, v4.w, s, c);
    ((float4*)p)[i] = p4;
    ((float4*)m)[i] = m4;
    ((float4*)v)[i] = v4;
    if (tgt) {
      float4 t4 = ((float4*)tgt)[i];
      t4.x = madam_polyak(t4.x, p4.x, c);
      t4.y = madam_polyak(t4.y, p4.y, c);
      t4.z = madam_polyak(t4.z, p4.z, c);
      t4.w = madam_polyak(t4.w, p4.w, c);
      ((float4*)tgt)[i] = t4;
    }
  }
  for (unsigned int i = nvec * 4 + tid; i < len; i += MADAM_THREADS) {
    float pi = p[i], mi = m[i], vi = v[i];
    madam_element(g[i], pi, mi, vi, s, c);
    p[i] = pi;
    m[i] = mi;
    v[i] = vi;
    if (tgt) tgt[i] = madam_polyak(tgt[i], pi, c);
  }
}

extern "C" void launch_multi_adam_norm(const MultiAdamTable& T, float* partials,
                                       void* stream) {
  if (T.n_blocks <= 0) return;
  hipLaunchKernelGGL(multi_adam_norm_kernel, dim3(T.n_blocks),
                     dim3(MADAM_THREADS), 0, (hipStream_t)stream, T, partials);
}

extern "C" void launch_multi_adam_update(const MultiAdamTable& T,
                                         const float* partials, void* stream) {
  if (T.n_blocks <= 0) return;
  hipLaunchKernelGGL(multi_adam_update_kernel, dim3(T.n_blocks),
                     dim3(MADAM_THREADS), 0, (hipStream_t)stream, T, partials);
}
