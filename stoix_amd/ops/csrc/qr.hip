// Quantile-regression (QR-DQN) pinball / quantile-Huber loss, forward and
// analytic backward (K11 of SURVEY.md: the QR half of the distributional
// losses; c51.hip is the categorical half).
//
// Per batch row b, with src [B, N, A], tgt [B, M, A], sel [B, Ns, A] (the
// quantile head's layouts, action innermost), tau [N] or [B, N]:
//   best   = argmax_a mean_j sel[b, j, a]    (ties -> lowest a, NaN = max;
//                                             no selector: best = 0)
//   t_j    = r_b + d_b * tgt[b, j, best]     (fp32, multiply THEN add; no r/d:
//                                             t_j = tgt[b, j, best])
//   th_i   = src[b, i, a_b]                  (no action vector: A == 1)
//   dl_ij  = t_j - th_i,  w_ij = |tau_i - [dl_ij < 0]|
//   rho    = k > 0 ? (|dl| <= k ? 0.5 dl^2 : k (|dl| - 0.5 k)) / k : |dl|
//   rho'   = k > 0 ? clamp(dl, -k, k) / k : sign(dl)
//   loss_b = sum_i (1/M) sum_j w_ij rho(dl_ij)
//   gth_bi = -(1/M) sum_j w_ij rho'(dl_ij)          = d loss_b / d th_i
// Backward: dsrc[b, i, a] = g_b * gth_bi for a == a_b, 0 for every other
// action; every element is written.
//
// Forward geometry: one WAVE owns one row, 4 rows per 256-thread workgroup.
//  1. Selector means. The [Ns, A] row is contiguous; lanes 0..S-1 read it
//     with lane stride S = (64 / A) * A, the largest multiple of A that fits
//     a wave, so consecutive lanes read consecutive addresses and a lane only
//     ever meets action lane % A. The 64 partials go to LDS and lane a < A
//     adds its 64 / A of them in ascending lane order; the arg-max is the
//     (value, index) butterfly of c51.hip.
//  2. The target samples t_j are formed while the stride-A column of tgt is
//     gathered, and parked in a wave-private LDS slice (M floats, <= 4 KB).
//  3. Pairs. A lane owns source quantile i = lane + 64 p and holds th_i, the
//     two weights |tau_i - 1| and |tau_i| and two accumulators (loss,
//     gradient) in registers, P = min(4, ceil(N / 64)) quantiles at a time
//     (a template parameter, so the arrays never leave registers). It sweeps
//     j ascending over 16-byte LDS reads that every lane issues at the same
//     address (a broadcast, no bank conflict); each t_j serves P pairs, and
//     one pass over the N x M pairs yields loss AND gth, so the backward
//     never revisits them. N > 256 repeats the sweep per block of 256
//     quantiles (passes past N in the last block idle).
//     The 1 / k and 1 / M factors are applied once per (b, i), after the sum.
//  4. loss_b is a __shfl_xor butterfly over the 64 lane sums.
// No atomics anywhere and every order is fixed: two runs give the same bits.
//
// There is NO workgroup barrier in this file: the LDS slices are private to
// a wave, so a wave without a row (B % 4 != 0) simply returns.
//
// The per-row vectors a, r, d and grad come with an element stride, tau with
// a row stride (0 for a shared or expanded [N]): a column of a replay batch
// or the expanded gradient of a mean is read in place.
//
// FMA contraction is off for the file: t_j is fl(r + fl(d * x)) as the two
// torch ops give it, and dl = fl(t - th) then has the sign of the exact
// difference of those two floats, so the indicator [dl < 0] is the one an
// fp64 evaluation of the same t and th takes. The accumulations are explicit
// fmaf calls (one rounding per pair), which no flag changes.
// Built as its own object with packed fp32 operations off (ops/build.py).
//
// Resources (-Rpass-analysis=kernel-resource-usage, gfx950): the forward's
// eight instantiations 34-62 VGPRs, no AGPRs, no scratch, 8 waves/SIMD,
// dynamic LDS 4 * (64 + M) floats (at most 17 KB); the backward 9 VGPRs, no
// LDS, no scratch.
#include "common.h"
#include "launchers.h"
#include <hip/hip_bf16.h>

#pragma clang fp contract(off)

typedef __bf16 bf16_t;

#define QR_WAVES 4
#define QR_THREADS (QR_WAVES * 64)
#define QR_PART 64  // selector partials per wave, in front of its t slice

// fp32 or bf16 element, upcast in registers
DEV_INLINE float qr_ld(const void* __restrict__ p, long i, int is_bf16) {
  return is_bf16 ? (float)((const bf16_t*)p)[i] : ((const float*)p)[i];
}

// floats of one wave's LDS slice: partials + M samples, 16-byte granular
#define QR_SLICE(M) (QR_PART + (((M) + 3) & ~3))

// Orders a wave's LDS stores before its later LDS loads (other lanes' data)
// for the compiler; the hardware runs one wave's LDS operations in order.
DEV_INLINE void qr_wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// One (i, j) pair into the two accumulators of quantile i. The 1 / k of the
// Huber form is left to the caller. A NaN dl stays a NaN in both.
template <bool HUBER>
DEV_INLINE void qr_pair(float t, float th, float w_neg, float w_pos, float k,
                        float& acc_loss, float& acc_grad) {
  const float dl = t - th;
  const float w = dl < 0.f ? w_neg : w_pos;
  const float ad = fabsf(dl);
  float rho, drho;
  if (HUBER) {
    rho = ad <= k ? 0.5f * (dl * dl) : k * (ad - 0.5f * k);
    drho = dl < -k ? -k : (dl > k ? k : dl);
  } else {
    rho = ad;
    drho = dl > 0.f ? 1.f : (dl < 0.f ? -1.f : dl);  // sign(0) = 0
  }
  acc_loss = fmaf(w, rho, acc_loss);
  acc_grad = fmaf(w, drho, acc_grad);
}

template <int P, bool HUBER>
__global__ void __launch_bounds__(QR_THREADS) qr_loss_fwd_kernel(
    const void* __restrict__ src, const float* __restrict__ tau,
    const long* __restrict__ a_tm1, const float* __restrict__ r_t,
    const float* __restrict__ d_t, const void* __restrict__ sel,
    const void* __restrict__ tgt, float* __restrict__ loss,
    float* __restrict__ gth, int B, int A, int N, int M, int Ns, int src_bf16,
    int tgt_bf16, int sel_bf16, float k, long tau_stride, long a_stride,
    long r_stride, long d_stride) {
  extern __shared__ __attribute__((aligned(16))) float qr_lds[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * QR_WAVES + wave;
  if (b >= B) return;  // no workgroup barrier below
  float* __restrict__ part_s = qr_lds + (size_t)wave * QR_SLICE(M);
  float* __restrict__ t_s = part_s + QR_PART;

  // 1. greedy action of the selector's mean over its quantiles
  int best = 0;
  if (sel != nullptr) {
    const int S = (64 / A) * A;
    const int row = Ns * A;  // <= 1024 * 64
    const long s_off = (long)b * row;
    float part = 0.f;
    if (lane < S)
      for (int e = lane; e < row; e += S) part += qr_ld(sel, s_off + e, sel_bf16);
    part_s[lane] = part;
    qr_wave_lds_sync();
    float v = -INFINITY;
    int idx = lane;
    if (lane < A) {
      float s = 0.f;
      for (int g = lane; g < S; g += A) s += part_s[g];
      v = __fdiv_rn(s, (float)Ns);
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

  // 2. target samples of that action, shifted and scaled on the way to LDS
  {
    const bool shift = r_t != nullptr;
    const float r = shift ? r_t[b * r_stride] : 0.f;
    const float d = shift ? d_t[b * d_stride] : 1.f;
    const long t_off = (long)b * M * A + best;
    for (int j = lane; j < M; j += 64) {
      const float x = qr_ld(tgt, t_off + (long)j * A, tgt_bf16);
      t_s[j] = shift ? r + d * x : x;  // two roundings: contraction is off
    }
  }
  qr_wave_lds_sync();

  // 3. all pairs; an action outside [0, A) reads action 0 and poisons loss
  const long a = a_tm1 != nullptr ? a_tm1[b * a_stride] : 0;
  const bool a_ok = a >= 0 && a < (long)A;
  const long th_off = (long)b * N * A + (a_ok ? a : 0);
  const float* __restrict__ tau_row = tau + (long)b * tau_stride;
  const int M4 = M & ~3;
  const float fM = (float)M;
  float row_loss = 0.f;
  for (int i0 = 0; i0 < N; i0 += 64 * P) {
    float th[P], w_neg[P], w_pos[P], acc_l[P], acc_g[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const int i = i0 + p * 64 + lane;
      const bool ok = i < N;
      th[p] = ok ? qr_ld(src, th_off + (long)i * A, src_bf16) : 0.f;
      const float tq = ok ? tau_row[i] : 0.f;
      w_neg[p] = fabsf(tq - 1.f);  // |tau - [dl < 0]| for either indicator
      w_pos[p] = fabsf(tq);
      acc_l[p] = 0.f;
      acc_g[p] = 0.f;
    }
    for (int j = 0; j < M4; j += 4) {
      const float4 t = *(const float4*)(t_s + j);
#pragma unroll
      for (int p = 0; p < P; ++p) {
        qr_pair<HUBER>(t.x, th[p], w_neg[p], w_pos[p], k, acc_l[p], acc_g[p]);
        qr_pair<HUBER>(t.y, th[p], w_neg[p], w_pos[p], k, acc_l[p], acc_g[p]);
        qr_pair<HUBER>(t.z, th[p], w_neg[p], w_pos[p], k, acc_l[p], acc_g[p]);
        qr_pair<HUBER>(t.w, th[p], w_neg[p], w_pos[p], k, acc_l[p], acc_g[p]);
      }
    }
    for (int j = M4; j < M; ++j) {
      const float t = t_s[j];
#pragma unroll
      for (int p = 0; p < P; ++p)
        qr_pair<HUBER>(t, th[p], w_neg[p], w_pos[p], k, acc_l[p], acc_g[p]);
    }
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const int i = i0 + p * 64 + lane;
      if (i < N) {
        float l = acc_l[p], g = acc_g[p];
        if (HUBER) {
          l = __fdiv_rn(l, k);
          g = __fdiv_rn(g, k);
        }
        row_loss += __fdiv_rn(l, fM);
        gth[(long)b * N + i] = -__fdiv_rn(g, fM);
      }
    }
  }

  // 4. fixed-order row sum
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) row_loss += __shfl_xor(row_loss, o);
  if (lane == 0) loss[b] = a_ok ? row_loss : NAN;
}

// One wave per row, lanes stride the flattened [N, A] row: consecutive
// lanes store consecutive elements. No LDS.
extern "C" __global__ void __launch_bounds__(QR_THREADS)
    qr_loss_bwd_kernel(const float* __restrict__ grad, long grad_stride,
                       const float* __restrict__ gth,
                       const long* __restrict__ a_tm1, long a_stride,
                       void* __restrict__ dsrc, int B, int N, int A,
                       int is_bf16) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * QR_WAVES + wave;
  if (b >= B) return;
  const long a = a_tm1 != nullptr ? a_tm1[b * a_stride] : 0;
  // no element matches a bad action: the whole row is zero
  const int taken = (a >= 0 && a < (long)A) ? (int)a : -1;
  const float g = grad[(long)b * grad_stride];
  const float* __restrict__ grow = gth + (long)b * N;
  const int NA = N * A;  // <= 1024 * 64
  const long row = (long)b * NA;
  for (int e = lane; e < NA; e += 64) {
    const int i = e / A;
    const float v = (e - i * A) == taken ? g * grow[i] : 0.f;
    if (is_bf16)
      ((bf16_t*)dsrc)[row + e] = (bf16_t)v;  // one round-to-nearest-even
    else
      ((float*)dsrc)[row + e] = v;
  }
}

// ----------------------------------------------------------- host launchers

#define QR_SIZES_OK(B, A, N, M, Ns)                                          \
  ((A) >= 1 && (A) <= 64 && (N) >= 1 && (N) <= 1024 && (M) >= 1 &&           \
   (M) <= 1024 && (Ns) >= 1 && (Ns) <= 1024 && (B) >= 0)

template <int P>
static void qr_launch_fwd(bool huber, dim3 grid, size_t lds, hipStream_t st,
                          const void* src, const float* tau, const long* a_tm1,
                          const float* r_t, const float* d_t, const void* sel,
                          const void* tgt, float* loss, float* gth, int B,
                          int A, int N, int M, int Ns, int src_bf16,
                          int tgt_bf16, int sel_bf16, float k, long tau_stride,
                          long a_stride, long r_stride, long d_stride) {
  if (huber)
    hipLaunchKernelGGL((qr_loss_fwd_kernel<P, true>), grid, dim3(QR_THREADS),
                       lds, st, src, tau, a_tm1, r_t, d_t, sel, tgt, loss, gth,
                       B, A, N, M, Ns, src_bf16, tgt_bf16, sel_bf16, k,
                       tau_stride, a_stride, r_stride, d_stride);
  else
    hipLaunchKernelGGL((qr_loss_fwd_kernel<P, false>), grid, dim3(QR_THREADS),
                       lds, st, src, tau, a_tm1, r_t, d_t, sel, tgt, loss, gth,
                       B, A, N, M, Ns, src_bf16, tgt_bf16, sel_bf16, k,
                       tau_stride, a_stride, r_stride, d_stride);
}

extern "C" int launch_qr_loss_fwd(
    const void* src, const float* tau, const long* a_tm1, const float* r_t,
    const float* d_t, const void* sel, const void* tgt, float* loss,
    float* gth, int B, int A, int N, int M, int Ns, int src_bf16,
    int tgt_bf16, int sel_bf16, float huber_param, long tau_stride,
    long a_stride, long r_stride, long d_stride, void* stream) {
  if (!QR_SIZES_OK(B, A, N, M, sel != nullptr ? Ns : 1)) return 1;
  if ((a_tm1 == nullptr || sel == nullptr) && A != 1) return 1;
  if ((r_t == nullptr) != (d_t == nullptr)) return 1;
  if (tau_stride < 0 || a_stride < 0 || r_stride < 0 || d_stride < 0) return 1;
  if (B == 0) return 0;
  const dim3 grid((B + QR_WAVES - 1) / QR_WAVES);
  // per wave 64 partials + M samples: at most 4 * (64 + 1024) * 4 B = 17 KB
  const size_t lds = (size_t)QR_WAVES * QR_SLICE(M) * sizeof(float);
  const bool huber = huber_param > 0.f;
  const int passes = (N + 63) / 64;
#define QR_FWD(P)                                                            \
  qr_launch_fwd<P>(huber, grid, lds, (hipStream_t)stream, src, tau, a_tm1,   \
                   r_t, d_t, sel, tgt, loss, gth, B, A, N, M, Ns, src_bf16,  \
                   tgt_bf16, sel_bf16, huber_param, tau_stride, a_stride,    \
                   r_stride, d_stride)
  switch (passes < 4 ? passes : 4) {
    case 1: QR_FWD(1); break;
    case 2: QR_FWD(2); break;
    case 3: QR_FWD(3); break;
    default: QR_FWD(4); break;
  }
#undef QR_FWD
  return 0;
}

extern "C" int launch_qr_loss_bwd(const float* grad, long grad_stride,
                                  const float* gth, const long* a_tm1,
                                  long a_stride, void* dsrc, int B, int N,
                                  int A, int is_bf16, void* stream) {
  if (!QR_SIZES_OK(B, A, N, 1, 1)) return 1;
  if (a_tm1 == nullptr && A != 1) return 1;
  if (grad_stride < 0 || a_stride < 0) return 1;
  if (B == 0) return 0;
  const int blocks = (B + QR_WAVES - 1) / QR_WAVES;
  hipLaunchKernelGGL(qr_loss_bwd_kernel, dim3(blocks), dim3(QR_THREADS), 0,
                     (hipStream_t)stream, grad, grad_stride, gth, a_tm1,
                     a_stride, dsrc, B, N, A, is_bf16);
  return 0;
}
