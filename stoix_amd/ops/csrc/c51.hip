// Categorical (C51) distributional TD loss, forward and analytic backward
// (K11 of SURVEY.md: Rainbow, C51 and the D4PG critic).
//
// Forward, per batch row b:
//   best   = argmax_a selector[b, a]                 (ties -> lowest index)
//   p      = softmax(logits_t[b, best, :])           [N]
//   z_i    = clamp(r + d * atoms_t[i], vmin, vmax)
//   bpos_i = (z_i - vmin) / dz,  lo_i = floor(bpos_i),  hi_i = min(lo_i+1, M-1)
//   target[j] = sum_i p_i*(1-frac_i)*[lo_i == j] + p_i*frac_i*[hi_i == j]
//   lse    = logsumexp(logits_tm1[b, a_tm1[b], :])
//   ce     = -sum_j target[j] * (logit_j - lse)
// Backward: dlogits[b, a, j] = g_b * (exp(logit_j - lse_b) * sum_k target[b,k]
//                                     - target[b, j])   for a == a_tm1[b],
//           0 for every other action; every element is written.
//
// Geometry: one WAVE owns one row, 4 rows per 256-thread workgroup, lanes
// stride over atoms. The projection is a GATHER, not a scatter: each source
// atom leaves (lo, p*w_lo, p*w_hi) in a wave-private LDS slice, and the lane
// that owns destination j walks the sources in ascending i, reading every
// triple at the same address in all lanes (an LDS broadcast, no bank
// conflict) and adding the lo term before the hi term. No atomics anywhere,
// so the summation order, and with it target, ce and the priorities written
// back from ce, is the same on every run. hi = min(lo+1, M-1) with
// w_hi = bpos - lo keeps the mass in the corner cases: an integral bpos
// gives w_hi = 0, and a z clamped to vmax sends both terms to atom M-1.
//
// The per-row vectors a_tm1, r_t, d_t and grad_ce come with an element
// stride: a column of a replay batch or the expanded gradient of a mean is
// read in place, with no copy kernel in front.
//
// There is NO workgroup barrier in this file: the LDS slices are private to
// a wave, so a wave without a row (B % 4 != 0) simply returns. Reductions
// are __shfl_xor butterflies over all 64 lanes; a lane without an atom
// contributes the identity (-inf to max, 0 to sums).
//
// exp/log are the hardware __expf/__logf (design rule 6 of docs/KERNELS.md):
// every exp argument is x - max <= 0 or logit - lse <= ~0, where
// exp2(x*log2e) is off by about |x| * 6e-8 relative, on terms that are
// themselves e^x small; the softmax normalisation divides the same rounded
// terms by their own sum, so the mass is unaffected.
#include "common.h"
#include "launchers.h"
#include <hip/hip_bf16.h>

typedef __bf16 bf16_t;

#define C51_WAVES 4
#define C51_THREADS (C51_WAVES * 64)

// fp32 or bf16 element, upcast in registers
DEV_INLINE float c51_ld(const void* __restrict__ p, long i, int is_bf16) {
  return is_bf16 ? (float)((const bf16_t*)p)[i] : ((const float*)p)[i];
}

DEV_INLINE float c51_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

DEV_INLINE float c51_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// Orders a wave's LDS stores before its later LDS loads (other lanes' data)
// for the compiler; the hardware runs one wave's LDS operations in order.
DEV_INLINE void c51_wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

extern "C" __global__ void __launch_bounds__(C51_THREADS) c51_loss_fwd_kernel(
    const void* __restrict__ logits_tm1, const float* __restrict__ atoms_tm1,
    const long* __restrict__ a_tm1, const float* __restrict__ r_t,
    const float* __restrict__ d_t, const void* __restrict__ logits_t,
    const float* __restrict__ atoms_t, const float* __restrict__ selector,
    float* __restrict__ ce, float* __restrict__ lse_out,
    float* __restrict__ target, int B, int A, int N, int M, int tm1_bf16,
    int t_bf16, long a_stride, long r_stride, long d_stride) {
  extern __shared__ float c51_lds[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * C51_WAVES + wave;
  if (b >= B) return;  // no workgroup barrier below
  float* __restrict__ w_lo_s = c51_lds + (size_t)wave * 3 * N;
  float* __restrict__ w_hi_s = w_lo_s + N;
  int* __restrict__ lo_s = (int*)(w_hi_s + N);

  // 1. greedy action of the selector; an empty selector means A == 1
  int best = 0;
  if (selector != nullptr) {
    float v = -INFINITY;
    int idx = lane;
    if (lane < A) {
      v = selector[(long)b * A + lane];
      if (v != v) v = INFINITY;  // NaN counts as the maximum, as in argmax
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      float ov = __shfl_xor(v, o);
      int oi = __shfl_xor(idx, o);
      if (ov > v || (ov == v && oi < idx)) {
        v = ov;
        idx = oi;
      }
    }
    best = min(__builtin_amdgcn_readfirstlane(idx), A - 1);
  }

  // 2. softmax of the target logits at that action (unnormalised terms
  // parked in the w_lo slots; the same lane reads them back)
  const long t_off = ((long)b * A + best) * N;
  float mx = -INFINITY;
  for (int i = lane; i < N; i += 64)
    mx = fmaxf(mx, c51_ld(logits_t, t_off + i, t_bf16));
  mx = c51_wave_max(mx);
  float s = 0.f;
  for (int i = lane; i < N; i += 64) {
    float e = __expf(c51_ld(logits_t, t_off + i, t_bf16) - mx);
    w_lo_s[i] = e;
    s += e;
  }
  s = c51_wave_sum(s);

  // 3. shift/scale the source atoms and split each onto its two neighbours
  const float vmin = atoms_tm1[0], vmax = atoms_tm1[M - 1];
  const float dz = __fdiv_rn(vmax - vmin, (float)(M - 1));
  const float r = r_t[b * r_stride], d = d_t[b * d_stride];
  for (int i = lane; i < N; i += 64) {
    float p = __fdiv_rn(w_lo_s[i], s);
    float z = __fadd_rn(r, __fmul_rn(d, atoms_t[i]));
    z = z < vmin ? vmin : (z > vmax ? vmax : z);  // keeps a NaN a NaN
    float bpos = M > 1 ? __fdiv_rn(z - vmin, dz) : 0.f;
    float fl = floorf(bpos);
    float w_hi = bpos - fl;
    float w_lo = 1.f - w_hi;
    lo_s[i] = max(0, min((int)fl, M - 1));
    w_lo_s[i] = p * w_lo;
    w_hi_s[i] = p * w_hi;
  }
  c51_wave_lds_sync();

  // 5a. log-sum-exp of the taken action's logits; an action outside [0, A)
  // reads action 0 and poisons ce below
  const long a = a_tm1 != nullptr ? a_tm1[b * a_stride] : 0;
  const bool a_ok = a >= 0 && a < (long)A;
  const long l_off = ((long)b * A + (a_ok ? a : 0)) * M;
  float mx1 = -INFINITY;
  for (int j = lane; j < M; j += 64)
    mx1 = fmaxf(mx1, c51_ld(logits_tm1, l_off + j, tm1_bf16));
  mx1 = c51_wave_max(mx1);
  float s1 = 0.f;
  for (int j = lane; j < M; j += 64)
    s1 += __expf(c51_ld(logits_tm1, l_off + j, tm1_bf16) - mx1);
  s1 = c51_wave_sum(s1);
  const float lse = mx1 + __logf(s1);

  // 4 + 5b. fixed-order gather of the projection, and the cross-entropy
  const int top = M - 1;
  float dot = 0.f;
  for (int j = lane; j < M; j += 64) {
    float acc = 0.f;
    for (int i = 0; i < N; ++i) {
      int lo = lo_s[i];
      int hi = min(lo + 1, top);
      acc += lo == j ? w_lo_s[i] : 0.f;
      acc += hi == j ? w_hi_s[i] : 0.f;
    }
    target[(long)b * M + j] = acc;
    dot += acc * (c51_ld(logits_tm1, l_off + j, tm1_bf16) - lse);
  }
  dot = c51_wave_sum(dot);
  if (lane == 0) {
    ce[b] = a_ok ? -dot : NAN;
    lse_out[b] = lse;
  }
}

extern "C" __global__ void __launch_bounds__(C51_THREADS) c51_loss_bwd_kernel(
    const float* __restrict__ grad_ce, long grad_stride,
    const void* __restrict__ logits_tm1, const long* __restrict__ a_tm1,
    const float* __restrict__ lse, const float* __restrict__ target,
    void* __restrict__ dlogits, int B, int A, int M, int is_bf16,
    long a_stride) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * C51_WAVES + wave;
  if (b >= B) return;
  const float* __restrict__ trow = target + (long)b * M;
  float tsum = 0.f;
  for (int j = lane; j < M; j += 64) tsum += trow[j];
  tsum = c51_wave_sum(tsum);
  const long a = a_tm1 != nullptr ? a_tm1[b * a_stride] : 0;
  const int AM = A * M;
  // first flat index of the taken action's atoms; none for a bad action
  const int first = (a >= 0 && a < (long)A) ? (int)a * M : AM;
  const float g = grad_ce[(long)b * grad_stride], l = lse[b];
  const long row = (long)b * AM;
  for (int k = lane; k < AM; k += 64) {
    const int j = k - first;
    float v = 0.f;
    if (j >= 0 && j < M)
      v = g * (__expf(c51_ld(logits_tm1, row + k, is_bf16) - l) * tsum -
               trow[j]);
    if (is_bf16)
      ((bf16_t*)dlogits)[row + k] = (bf16_t)v;  // one round-to-nearest-even
    else
      ((float*)dlogits)[row + k] = v;
  }
}

// ----------------------------------------------------------- host launchers

extern "C" void launch_c51_loss_fwd(
    const void* logits_tm1, const float* atoms_tm1, const long* a_tm1,
    const float* r_t, const float* d_t, const void* logits_t,
    const float* atoms_t, const float* selector, float* ce, float* lse,
    float* target, int B, int A, int N, int M, int tm1_bf16, int t_bf16,
    long a_stride, long r_stride, long d_stride, void* stream) {
  if (B <= 0) return;
  const int blocks = (B + C51_WAVES - 1) / C51_WAVES;
  // per wave: N x (lo, p*w_lo, p*w_hi); at most 4 * 3 * 1024 * 4 B = 48 KB
  const size_t lds = (size_t)C51_WAVES * 3 * N * sizeof(float);
  hipLaunchKernelGGL(c51_loss_fwd_kernel, dim3(blocks), dim3(C51_THREADS), lds,
                     (hipStream_t)stream, logits_tm1, atoms_tm1, a_tm1, r_t,
                     d_t, logits_t, atoms_t, selector, ce, lse, target, B, A,
                     N, M, tm1_bf16, t_bf16, a_stride, r_stride, d_stride);
}

extern "C" void launch_c51_loss_bwd(const float* grad_ce, long grad_stride,
                                    const void* logits_tm1, const long* a_tm1,
                                    const float* lse, const float* target,
                                    void* dlogits, int B, int A, int M,
                                    int is_bf16, long a_stride,
                                    void* stream) {
  if (B <= 0) return;
  const int blocks = (B + C51_WAVES - 1) / C51_WAVES;
  hipLaunchKernelGGL(c51_loss_bwd_kernel, dim3(blocks), dim3(C51_THREADS), 0,
                     (hipStream_t)stream, grad_ce, grad_stride, logits_tm1,
                     a_tm1, lse, target, dlogits, B, A, M, is_bf16, a_stride);
}
