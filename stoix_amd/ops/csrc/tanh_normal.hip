// The sampling and loss chain of the SAC update (the continuous counterpart
// of c51.hip / qr.hip): a reparameterised sample of the tanh-squashed,
// affinely mapped Gaussian with its log-probability, forward and analytic
// backward, and the per-row SAC critic / actor / temperature terms.
//
// tanh_normal_rsample_fwd_kernel, per element of loc, scale, eps [B, A]:
//   u     = loc + scale * eps                  (fp32, multiply THEN add)
//   t     = tanh(u)
//   a     = t * scale_affine + shift_affine    (fp32, then loc's dtype)
//   lp_i  = -0.5 eps^2 - log(scale) - 0.5 log(2 pi)
//           - (2 (log 2 - u - softplus(-2u)) + log(scale_affine))
//   logp  = sum_i lp_i
// The base density is written in eps, not in (u - loc) / scale: the two are
// the same number and eps is the one without a cancellation.
// One exponential serves tanh and softplus: with m = expm1(-2|u|),
//   tanh|u| = -m / (2 + m),   log 2 - u - softplus(-2u) = log 2 - |u| - log1p(1 + m)
// (the log-det is even in u). These, log(scale) and the sum of lp_i's terms
// are evaluated in fp64 and rounded to fp32 ONCE per element: the chain is a
// few thousand elements, so t, a and lp_i are the correctly rounded
// functions of the fp32 u at the price of fp64 transcendentals on each. What
// that price is has NOT been measured: there is no fp32 variant of the kernel
// to time it against; the kernel as it is runs 3.9 us at B = 2048, A = 17.
//
// tanh_normal_rsample_bwd_kernel, with g = da * scale_affine * (1 - t^2)
// + dlogp * 2 t (d a / d u and d logp / d u; d(-logdet)/du = 2 tanh u):
//   dloc   = g
//   dscale = eps * g - dlogp / scale
// The base density -0.5 eps^2 does not depend on loc or scale once
// u = loc + scale * eps is substituted, and -log(scale) gives -1 / scale.
// The two sums are formed in fp64 from the fp32 operands and rounded once to
// the parameter's dtype. Every element is written.
//
// Geometry of both (as mcts.hip): a group of G = min(64, next_pow2(A)) lanes
// owns a row and lane i owns dimension i, so a group's loads and stores are
// one contiguous run of A elements (for A == G, G <= 8 included, a wave's are
// one run of 64); 256 / G rows per 256-thread workgroup. logp is a width-G
// __shfl_xor butterfly over the fp32 lp_i (lanes past A hold 0), the same
// order on every run. A group past B returns before it touches memory, lanes
// past A touch none. No LDS, no barrier, no atomics, no scratch.
//
// sac_critic_rows_kernel / sac_actor_rows_kernel / sac_rows_bwd_kernel: flat,
// one batch row per thread, Q <= 4 critics held in registers, fp32 in the
// order of the torch expressions they replace (FMA contraction is off for the
// file). log_alpha is read from device memory, so nothing here needs the host
// to know it: the kernels can be captured. alpha = exp(log_alpha) is the
// fp64 exponential rounded to fp32. The per-row vectors come with an element
// stride (a column of a replay batch, the expanded gradient of a mean).
//
// Built as its own object with packed fp32 operations off (ops/build.py).
//
// Resources (-Rpass-analysis=kernel-resource-usage, gfx950) are listed in
// docs/KERNELS.md; no kernel here uses LDS, AGPRs or scratch.
#include "common.h"
#include "launchers.h"
#include <hip/hip_bf16.h>

#pragma clang fp contract(off)

typedef __bf16 bf16_t;

#define TN_THREADS 256
#define SAC_THREADS 256
#define SAC_MAX_Q 4

// fp32 or bf16 element, upcast in registers
DEV_INLINE float tn_ld(const void* __restrict__ p, long i, int is_bf16) {
  return is_bf16 ? (float)((const bf16_t*)p)[i] : ((const float*)p)[i];
}

// one round-to-nearest-even for bf16
DEV_INLINE void tn_st(void* __restrict__ p, long i, int is_bf16, float v) {
  if (is_bf16)
    ((bf16_t*)p)[i] = (bf16_t)v;
  else
    ((float*)p)[i] = v;
}

extern "C" __global__ void __launch_bounds__(TN_THREADS)
    tanh_normal_rsample_fwd_kernel(
        const void* __restrict__ loc, const void* __restrict__ scale,
        const float* __restrict__ eps, void* __restrict__ a_out,
        float* __restrict__ logp, float* __restrict__ t_out, int B, int A,
        int log2_g, int loc_bf16, int scale_bf16, float scale_affine,
        float shift_affine, double log_scale_affine) {
  const int G = 1 << log2_g;
  const int i = threadIdx.x & (G - 1);
  const long b = (long)blockIdx.x * (TN_THREADS >> log2_g) +
                 (threadIdx.x >> log2_g);
  if (b >= B) return;  // whole groups leave: the shuffles below stay in-group
  float lp = 0.f;
  if (i < A) {
    const long e = b * A + i;
    const float s = tn_ld(scale, e, scale_bf16);
    const float n = eps[e];
    const float u = tn_ld(loc, e, loc_bf16) + s * n;  // two roundings
    const double au = fabs((double)u);
    const double m = expm1(-2.0 * au);  // in [-1, 0]
    const float t = copysignf((float)(-m / (2.0 + m)), u);  // NaN stays NaN
    tn_st(a_out, e, loc_bf16, t * scale_affine + shift_affine);
    if (t_out != nullptr) t_out[e] = t;
    const double log_det =
        2.0 * (0.6931471805599453 - au - log1p(1.0 + m)) + log_scale_affine;
    lp = (float)(-0.5 * ((double)n * (double)n) - log((double)s) -
                 0.9189385332046727 - log_det);
  }
  for (int o = G >> 1; o > 0; o >>= 1) lp += __shfl_xor(lp, o);
  if (i == 0) logp[b] = lp;
}

extern "C" __global__ void __launch_bounds__(TN_THREADS)
    tanh_normal_rsample_bwd_kernel(
        const void* __restrict__ da, const float* __restrict__ dlogp,
        long dlogp_stride, const float* __restrict__ t_in,
        const float* __restrict__ eps, const void* __restrict__ scale,
        void* __restrict__ dloc, void* __restrict__ dscale, int B, int A,
        int log2_g, int loc_bf16, int scale_bf16, float scale_affine) {
  const int G = 1 << log2_g;
  const int i = threadIdx.x & (G - 1);
  const long b = (long)blockIdx.x * (TN_THREADS >> log2_g) +
                 (threadIdx.x >> log2_g);
  if (b >= B || i >= A) return;  // no shuffle below
  const long e = b * A + i;
  const double gl = (double)dlogp[b * dlogp_stride];
  const double t = (double)t_in[e];
  const double g = (double)tn_ld(da, e, loc_bf16) * (double)scale_affine *
                       ((1.0 - t) * (1.0 + t)) +
                   gl * (2.0 * t);
  tn_st(dloc, e, loc_bf16, (float)g);
  const double s = (double)tn_ld(scale, e, scale_bf16);
  tn_st(dscale, e, scale_bf16, (float)((double)eps[e] * g - gl / s));
}

// torch.min over the critics: the lowest index among equals, a NaN wins and
// the first NaN stays.
DEV_INLINE float sac_min(const float* q, int Q, int* idx) {
  float m = q[0];
  int at = 0;
#pragma unroll
  for (int k = 1; k < SAC_MAX_Q; ++k)
    if (k < Q && !(m != m) && (q[k] < m || q[k] != q[k])) {
      m = q[k];
      at = k;
    }
  *idx = at;
  return m;
}

DEV_INLINE float sac_alpha(const float* __restrict__ log_alpha) {
  return (float)exp((double)log_alpha[0]);
}

extern "C" __global__ void __launch_bounds__(SAC_THREADS)
    sac_critic_rows_kernel(
        const float* __restrict__ q_pred, const float* __restrict__ q_next,
        const float* __restrict__ logp_next, long lp_stride,
        const float* __restrict__ r_t, long r_stride,
        const float* __restrict__ d_t, long d_stride,
        const float* __restrict__ log_alpha, float gamma,
        float* __restrict__ target, float* __restrict__ rows,
        float* __restrict__ dq, int Q, int B) {
  const long b = (long)blockIdx.x * SAC_THREADS + threadIdx.x;
  if (b >= B) return;
  float qn[SAC_MAX_Q];
#pragma unroll
  for (int k = 0; k < SAC_MAX_Q; ++k) qn[k] = k < Q ? q_next[(long)k * B + b] : 0.f;
  int unused;
  const float mn = sac_min(qn, Q, &unused);
  const float alpha = sac_alpha(log_alpha);
  // r + (gamma * d) * (min - alpha * logp), each step one fp32 rounding
  const float y = r_t[b * r_stride] +
                  (gamma * d_t[b * d_stride]) * (mn - alpha * logp_next[b * lp_stride]);
  target[b] = y;
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < SAC_MAX_Q; ++k)
    if (k < Q) {
      const float dl = q_pred[(long)k * B + b] - y;
      dq[(long)k * B + b] = dl;
      acc += dl * dl;
    }
  rows[b] = 0.5f * acc;
}

extern "C" __global__ void __launch_bounds__(SAC_THREADS)
    sac_actor_rows_kernel(
        const float* __restrict__ q_new, const float* __restrict__ logp_new,
        long lp_stride, const float* __restrict__ log_alpha,
        float target_entropy, float* __restrict__ actor_rows,
        float* __restrict__ alpha_rows, int* __restrict__ argmin,
        float* __restrict__ entropy_rows, int Q, int B) {
  const long b = (long)blockIdx.x * SAC_THREADS + threadIdx.x;
  if (b >= B) return;
  float q[SAC_MAX_Q];
#pragma unroll
  for (int k = 0; k < SAC_MAX_Q; ++k) q[k] = k < Q ? q_new[(long)k * B + b] : 0.f;
  int at;
  const float mn = sac_min(q, Q, &at);
  const float la = log_alpha[0];
  const float lp = logp_new[b * lp_stride];
  actor_rows[b] = sac_alpha(log_alpha) * lp - mn;
  alpha_rows[b] = -(la * (lp + target_entropy));
  argmin[b] = at;
  entropy_rows[b] = -lp;
}

// Backward of both row kernels. Critic half (g_rows != null):
//   dq_pred[q, b] = g_rows[b] * dq[q, b].
// Actor half (g_actor != null):
//   dq_new[q, b] = q == argmin[b] ? -g_actor[b] : 0   (every element written)
//   dlogp_new[b] = g_actor[b] * alpha                 (alpha is a constant)
//   dla_rows[b]  = -g_alpha[b] * (logp_new[b] + target_entropy)
// (logp_new is a constant of the dual).
extern "C" __global__ void __launch_bounds__(SAC_THREADS) sac_rows_bwd_kernel(
    const float* __restrict__ g_rows, long g_rows_stride,
    const float* __restrict__ dq, float* __restrict__ dq_pred,
    const float* __restrict__ g_actor, long g_actor_stride,
    const float* __restrict__ g_alpha, long g_alpha_stride,
    const int* __restrict__ argmin, const float* __restrict__ logp_new,
    long lp_stride, const float* __restrict__ log_alpha, float target_entropy,
    float* __restrict__ dq_new, float* __restrict__ dlogp_new,
    float* __restrict__ dla_rows, int Q, int B) {
  const long b = (long)blockIdx.x * SAC_THREADS + threadIdx.x;
  if (b >= B) return;
  if (g_rows != nullptr) {
    const float g = g_rows[b * g_rows_stride];
#pragma unroll
    for (int k = 0; k < SAC_MAX_Q; ++k)
      if (k < Q) dq_pred[(long)k * B + b] = g * dq[(long)k * B + b];
  }
  if (g_actor != nullptr) {
    const float g = g_actor[b * g_actor_stride];
    const int at = argmin[b];
#pragma unroll
    for (int k = 0; k < SAC_MAX_Q; ++k)
      if (k < Q) dq_new[(long)k * B + b] = k == at ? -g : 0.f;
    dlogp_new[b] = g * sac_alpha(log_alpha);
    dla_rows[b] =
        -(g_alpha[b * g_alpha_stride] * (logp_new[b * lp_stride] + target_entropy));
  }
}

// ----------------------------------------------------------- host launchers

static int tn_log2_group(int A) {
  int l = 0;
  while ((1 << l) < A) ++l;
  return l;  // A <= 64: at most 6
}

#define TN_SIZES_OK(B, A) ((A) >= 1 && (A) <= 64 && (B) >= 0)

extern "C" int launch_tanh_normal_rsample_fwd(
    const void* loc, const void* scale, const float* eps, void* a, float* logp,
    float* t, int B, int A, int loc_bf16, int scale_bf16, float scale_affine,
    float shift_affine, void* stream) {
  if (!TN_SIZES_OK(B, A) || !(scale_affine > 0.f)) return 1;
  if (B == 0) return 0;
  const int l2 = tn_log2_group(A);
  const int rows = TN_THREADS >> l2;
  hipLaunchKernelGGL(tanh_normal_rsample_fwd_kernel, dim3((B + rows - 1) / rows),
                     dim3(TN_THREADS), 0, (hipStream_t)stream, loc, scale, eps,
                     a, logp, t, B, A, l2, loc_bf16, scale_bf16, scale_affine,
                     shift_affine, log((double)scale_affine));
  return 0;
}

extern "C" int launch_tanh_normal_rsample_bwd(
    const void* da, const float* dlogp, long dlogp_stride, const float* t,
    const float* eps, const void* scale, void* dloc, void* dscale, int B,
    int A, int loc_bf16, int scale_bf16, float scale_affine, void* stream) {
  if (!TN_SIZES_OK(B, A) || dlogp_stride < 0) return 1;
  if (B == 0) return 0;
  const int l2 = tn_log2_group(A);
  const int rows = TN_THREADS >> l2;
  hipLaunchKernelGGL(tanh_normal_rsample_bwd_kernel, dim3((B + rows - 1) / rows),
                     dim3(TN_THREADS), 0, (hipStream_t)stream, da, dlogp,
                     dlogp_stride, t, eps, scale, dloc, dscale, B, A, l2,
                     loc_bf16, scale_bf16, scale_affine);
  return 0;
}

#define SAC_SIZES_OK(Q, B) ((Q) >= 1 && (Q) <= SAC_MAX_Q && (B) >= 0)
#define SAC_GRID(B) dim3(((B) + SAC_THREADS - 1) / SAC_THREADS)

extern "C" int launch_sac_critic_rows(
    const float* q_pred, const float* q_next, const float* logp_next,
    long lp_stride, const float* r_t, long r_stride, const float* d_t,
    long d_stride, const float* log_alpha, float gamma, float* target,
    float* rows, float* dq, int Q, int B, void* stream) {
  if (!SAC_SIZES_OK(Q, B) || lp_stride < 0 || r_stride < 0 || d_stride < 0)
    return 1;
  if (B == 0) return 0;
  hipLaunchKernelGGL(sac_critic_rows_kernel, SAC_GRID(B), dim3(SAC_THREADS), 0,
                     (hipStream_t)stream, q_pred, q_next, logp_next, lp_stride,
                     r_t, r_stride, d_t, d_stride, log_alpha, gamma, target,
                     rows, dq, Q, B);
  return 0;
}

extern "C" int launch_sac_actor_rows(
    const float* q_new, const float* logp_new, long lp_stride,
    const float* log_alpha, float target_entropy, float* actor_rows,
    float* alpha_rows, int* argmin, float* entropy_rows, int Q, int B,
    void* stream) {
  if (!SAC_SIZES_OK(Q, B) || lp_stride < 0) return 1;
  if (B == 0) return 0;
  hipLaunchKernelGGL(sac_actor_rows_kernel, SAC_GRID(B), dim3(SAC_THREADS), 0,
                     (hipStream_t)stream, q_new, logp_new, lp_stride, log_alpha,
                     target_entropy, actor_rows, alpha_rows, argmin,
                     entropy_rows, Q, B);
  return 0;
}

extern "C" int launch_sac_rows_bwd(
    const float* g_rows, long g_rows_stride, const float* dq, float* dq_pred,
    const float* g_actor, long g_actor_stride, const float* g_alpha,
    long g_alpha_stride, const int* argmin, const float* logp_new,
    long lp_stride, const float* log_alpha, float target_entropy,
    float* dq_new, float* dlogp_new, float* dla_rows, int Q, int B,
    void* stream) {
  if (!SAC_SIZES_OK(Q, B)) return 1;
  if (g_rows_stride < 0 || g_actor_stride < 0 || g_alpha_stride < 0 ||
      lp_stride < 0)
    return 1;
  if ((g_rows == nullptr) == (g_actor == nullptr)) return 1;  // one half
  if (B == 0) return 0;
  hipLaunchKernelGGL(sac_rows_bwd_kernel, SAC_GRID(B), dim3(SAC_THREADS), 0,
                     (hipStream_t)stream, g_rows, g_rows_stride, dq, dq_pred,
                     g_actor, g_actor_stride, g_alpha, g_alpha_stride, argmin,
                     logp_new, lp_stride, log_alpha, target_entropy, dq_new,
                     dlogp_new, dla_rows, Q, B);
  return 0;
}
