// Factorised-Gaussian NoisyLinear (K17 of SURVEY.md: every Rainbow forward
// and backward), with the noisy weight formed inside the GEMM kernels:
//
//   W[n,k] = bf16(mu_w[n,k] + sigma_w[n,k] * (eps_out[n] * eps_in[k]))
//   b[n]   = mu_b[n] + sigma_b[n] * eps_out[n]                    (fp32)
//   forward  Z = X @ W^T + b, H = act(Z)            noisy_linear_fwd_kernel
//   dgrad    dX = dZ @ W (* act'(Z_prev))           noisy_linear_dgrad_kernel
//   wgrad    dW = dZ^T @ X, db = colsum(dZ)         noisy_linear_wgrad_kernel
//            dmu_w = dW, dsigma_w = dW * (eps_out x eps_in),
//            dmu_b = db, dsigma_b = db * eps_out    noisy_wgrad_reduce_kernel
//   noise    x <- sign(x) * sqrt(|x|) in place      noise_transform_kernel
//
// W never exists in memory. A thread that stages a piece of the B tile loads
// 8 consecutive k of mu and sigma (fp32, 2 x 16 B each), forms the bf16
// weight in registers and writes it to LDS, so the MFMA sees the very bf16
// weight that materialize() followed by the autocast cast produces: the
// expression is evaluated in that order in fp32, and the whole file is
// compiled with contraction off so that no product is fused into the add.
// noisy == 0 (eval) reads mu only.
//
// All three GEMMs share one scheme: 256 threads = 4 waves as 2 x 2 over the
// workgroup tile, 32-deep reduction steps, operands of step i+1 loaded into
// registers before the MFMAs of step i and written to the other LDS buffer
// after them (one barrier per step), +8-column padded LDS rows, and
// v_mfma_f32_16x16x32_bf16 with the operand layout mfma_probe_kernel
// validates (lane l: A[m = l&15][k = (l>>4)*8 + j], B[k][n = l&15],
// D[row = (l>>4)*4 + r][col = l&15]). Each kernel puts the operand whose
// index is contiguous in the output on the A side, so a lane ends up with 4
// consecutive output elements of one row and stores them as one 8- or
// 16-byte piece. The last reduction step is peeled: the MFMA chain and the
// first read of its accumulator stay in straight-line code (docs/KERNELS.md),
// with bias and eps fetched before the loop.
//
// Tails: rows past S and columns past N are never read or written; a
// reduction tail (K % 32 in the forward, N % 32 in the dgrad, S % 32 in the
// wgrad) is zero-filled in LDS. K % 8 == 0 is required (16-byte pieces of
// the fp32 parameters and of X); the launchers report anything else as
// ineligible and launch nothing. eps_in / eps_out are views at arbitrary
// offsets of the NoiseBank buffer and are read element by element.
//
// The wgrad splits S over up to 16 workgroups per tile. Each writes its
// partial dW | db into its own fp32 slab; the reduce kernel adds the slabs in
// ascending order and applies the noise epilogue. No atomics: two runs give
// the same bits.
#include "common.h"
#include "launchers.h"
#include <hip/hip_bf16.h>

#pragma clang fp contract(off)

typedef __bf16 bf16_t;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define MFMA_BF16_16x16x32 __builtin_amdgcn_mfma_f32_16x16x32_bf16

#define NZ_THREADS 256
#define NZ_BK 32
#define NZ_LD (NZ_BK + 8)  // padded LDS row, in elements
#define NZ_ACT_NONE 0
#define NZ_ACT_SILU 1
#define NZ_ACT_RELU 2
#define NZ_MAX_SPLIT 16

// fp32 or bf16 element, upcast in registers
DEV_INLINE float nz_ld(const void* __restrict__ p, long i, int is_bf16) {
  return is_bf16 ? (float)((const bf16_t*)p)[i] : ((const float*)p)[i];
}

DEV_INLINE float nz_act(float z, int act) {
  if (act == NZ_ACT_SILU) return z / (1.0f + __expf(-z));
  if (act == NZ_ACT_RELU) return z > 0.f ? z : 0.f;
  return z;
}

DEV_INLINE float nz_act_grad(float z, int act) {
  if (act == NZ_ACT_SILU) {
    float s = 1.0f / (1.0f + __expf(-z));
    return s * (1.0f + z * (1.0f - s));
  }
  if (act == NZ_ACT_RELU) return z > 0.f ? 1.f : 0.f;
  return 1.f;
}

// Elements [col, col + 8) of a row of `ncols` that starts at element `row`
// of p, rounded to bf16; zero where the row or the column is out of range.
// `vec`: the rows are 16-byte aligned and ncols % 8 == 0.
DEV_INLINE bf16x8 nz_ld8(const void* __restrict__ p, long row, int col,
                         int ncols, bool row_ok, int is_bf16, bool vec) {
  bf16x8 v;
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = (bf16_t)0.f;
  if (!row_ok || col >= ncols) return v;
  if (vec) {
    if (is_bf16) {
      v = *reinterpret_cast<const bf16x8*>((const bf16_t*)p + row + col);
    } else {
      const float4 a =
          *reinterpret_cast<const float4*>((const float*)p + row + col);
      const float4 b =
          *reinterpret_cast<const float4*>((const float*)p + row + col + 4);
      v[0] = (bf16_t)a.x; v[1] = (bf16_t)a.y; v[2] = (bf16_t)a.z;
      v[3] = (bf16_t)a.w; v[4] = (bf16_t)b.x; v[5] = (bf16_t)b.y;
      v[6] = (bf16_t)b.z; v[7] = (bf16_t)b.w;
    }
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (col + i < ncols) v[i] = (bf16_t)nz_ld(p, row + col + i, is_bf16);
  }
  return v;
}

// 8 consecutive k of mu and sigma, as loaded; zeros out of range
struct NzW8 {
  float4 m0, m1, s0, s1;
};

DEV_INLINE NzW8 nz_ldw(const float* __restrict__ mu,
                       const float* __restrict__ sigma, long off, bool ok,
                       int noisy) {
  const float4 z = {0.f, 0.f, 0.f, 0.f};
  NzW8 w = {z, z, z, z};
  if (ok) {
    w.m0 = *reinterpret_cast<const float4*>(mu + off);
    w.m1 = *reinterpret_cast<const float4*>(mu + off + 4);
    if (noisy) {
      w.s0 = *reinterpret_cast<const float4*>(sigma + off);
      w.s1 = *reinterpret_cast<const float4*>(sigma + off + 4);
    }
  }
  return w;
}

// bf16(mu + sigma * (eps_out * eps_in)): the product of the two noise
// factors first, then the sigma product, then the add, each rounded to fp32
DEV_INLINE bf16x8 nz_form(const NzW8& w, float eo, const float (&ein)[8],
                          int noisy) {
  const float m[8] = {w.m0.x, w.m0.y, w.m0.z, w.m0.w,
                      w.m1.x, w.m1.y, w.m1.z, w.m1.w};
  const float s[8] = {w.s0.x, w.s0.y, w.s0.z, w.s0.w,
                      w.s1.x, w.s1.y, w.s1.z, w.s1.w};
  bf16x8 v;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float e = eo * ein[i];
    const float se = s[i] * e;
    v[i] = (bf16_t)(noisy ? m[i] + se : m[i]);
  }
  return v;
}

// ------------------------------------------------------------------ forward
// Workgroup tile 128 rows x BN columns. BN = 128: waves 2 x 2, 64 x 64 each;
// BN = 64 (N <= 64, the value head): waves 4 x 1, 32 x 64 each, so the head
// does not run MFMAs on three quarters of a 128-wide tile that is not there.
// A operand = W fragment, B operand = X fragment: acc[mi][nj][r] is row
// mi*16 + (lane&15), column nj*16 + (lane>>4)*4 + r of the wave's tile.
template <int BN>
struct alignas(16) NzFwdLds {
  bf16_t X[2][128][NZ_LD];
  bf16_t W[2][BN][NZ_LD];
};

template <int BN, int ACT>
__launch_bounds__(NZ_THREADS) __global__ void noisy_linear_fwd_kernel(
    const void* __restrict__ X,         // [S, K] fp32 or bf16
    const float* __restrict__ mu_w,     // [N, K]
    const float* __restrict__ sigma_w,  // [N, K]
    const float* __restrict__ mu_b,     // [N]
    const float* __restrict__ sigma_b,  // [N]
    const float* __restrict__ eps_in,   // [K]
    const float* __restrict__ eps_out,  // [N]
    bf16_t* __restrict__ Z,             // [S, N] or null
    bf16_t* __restrict__ H,             // [S, N] or null (ACT != none)
    int S, int K, int N, int x_bf16, int noisy) {
  constexpr int MI = BN == 128 ? 4 : 2;  // 16-row tiles per wave
  constexpr int WQ = BN / 64;            // W pieces per thread and step
  __shared__ NzFwdLds<BN> lds;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int m0 = blockIdx.x * 128;
  const int n_blk = blockIdx.y * BN;
  const int wm = BN == 128 ? (wid >> 1) * 64 : wid * 32;
  const int wn = BN == 128 ? (wid & 1) * 64 : 0;
  const int l15 = lane & 15;
  const int g = lane >> 4;
  // staging: this thread's piece is row srow (+64 per q), columns kh..kh+7
  const int srow = tid >> 2;
  const int kh = (tid & 3) * 8;

  float eo[WQ];
  bool n_ok[WQ];
#pragma unroll
  for (int q = 0; q < WQ; ++q) {
    const int n = n_blk + srow + q * 64;
    n_ok[q] = n < N;
    eo[q] = (noisy && n_ok[q]) ? eps_out[n] : 0.f;
  }
  float bv[4][4];
#pragma unroll
  for (int nj = 0; nj < 4; ++nj)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = n_blk + wn + nj * 16 + g * 4 + r;
      float b = 0.f;
      if (n < N) {
        b = mu_b[n];
        if (noisy) {
          const float sb = sigma_b[n] * eps_out[n];
          b = b + sb;
        }
      }
      bv[nj][r] = b;
    }

  f32x4 acc[MI][4];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  bf16x8 xr[2];
  NzW8 wr[WQ];
  float ein[8];
  auto load = [&](int ks) {
    const int k = ks * NZ_BK + kh;
    const bool k_ok = k < K;  // K % 8 == 0: a piece is all in or all out
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int m = m0 + srow + q * 64;
      xr[q] = nz_ld8(X, (long)m * K, k, K, m < S, x_bf16, true);
    }
#pragma unroll
    for (int q = 0; q < WQ; ++q)
      wr[q] = nz_ldw(mu_w, sigma_w, (long)(n_blk + srow + q * 64) * K + k,
                     n_ok[q] && k_ok, noisy);
#pragma unroll
    for (int i = 0; i < 8; ++i)
      ein[i] = (noisy && k_ok) ? eps_in[k + i] : 0.f;
  };
  auto store = [&](int pp) {
#pragma unroll
    for (int q = 0; q < 2; ++q)
      *reinterpret_cast<bf16x8*>(&lds.X[pp][srow + q * 64][kh]) = xr[q];
#pragma unroll
    for (int q = 0; q < WQ; ++q)
      *reinterpret_cast<bf16x8*>(&lds.W[pp][srow + q * 64][kh]) =
          nz_form(wr[q], eo[q], ein, noisy);
  };
  auto mma = [&](int pp) {
    bf16x8 xf[MI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
      xf[mi] = *reinterpret_cast<const bf16x8*>(
          &lds.X[pp][wm + mi * 16 + l15][g * 8]);
#pragma unroll
    for (int nj = 0; nj < 4; ++nj) {
      const bf16x8 wf = *reinterpret_cast<const bf16x8*>(
          &lds.W[pp][wn + nj * 16 + l15][g * 8]);
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
        acc[mi][nj] = MFMA_BF16_16x16x32(wf, xf[mi], acc[mi][nj], 0, 0, 0);
    }
  };

  const int KS = (K + NZ_BK - 1) / NZ_BK;
  load(0);
  store(0);
  for (int ks = 0; ks + 1 < KS; ++ks) {
    __syncthreads();
    load(ks + 1);
    mma(ks & 1);
    store((ks + 1) & 1);
  }
  __syncthreads();
  mma((KS - 1) & 1);
  // z = acc + b in fp32, straight after the chain
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int nj = 0; nj < 4; ++nj)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[mi][nj][r] = acc[mi][nj][r] + bv[nj][r];

  const bool vec = (N & 3) == 0;  // 8-byte aligned groups of 4 columns
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    const int m = m0 + wm + mi * 16 + l15;
    if (m >= S) continue;
#pragma unroll
    for (int nj = 0; nj < 4; ++nj) {
      const int n = n_blk + wn + nj * 16 + g * 4;
      if (n >= N) continue;
      bf16x4 z4, h4;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        z4[r] = (bf16_t)acc[mi][nj][r];  // the single rounding of Z
        // H from the stored Z, as the backward will see it
        h4[r] = (bf16_t)nz_act((float)z4[r], ACT);
      }
      const long o = (long)m * N + n;
      if (vec) {  // N % 4 == 0 and n % 4 == 0: n + 3 < N
        if (Z) *reinterpret_cast<bf16x4*>(Z + o) = z4;
        if (ACT != NZ_ACT_NONE && H) *reinterpret_cast<bf16x4*>(H + o) = h4;
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (n + r >= N) break;
          if (Z) Z[o + r] = z4[r];
          if (ACT != NZ_ACT_NONE && H) H[o + r] = h4[r];
        }
      }
    }
  }
}

// -------------------------------------------------------------------- dgrad
// dX[S, K] = dZ[S, N] @ W[N, K], reduction over n. Workgroup tile 128 rows x
// 128 k-columns, waves 2 x 2. The W tile goes to LDS transposed ([k][n], the
// 8 weights a thread formed scattered as 2-byte writes; consecutive lanes
// hold consecutive n of one k-piece, so the writes of an instruction fall on
// consecutive banks). A operand = W^T fragment, B operand = dZ fragment:
// acc[mi][kj][r] is row mi*16 + (lane&15), k-column kj*16 + (lane>>4)*4 + r.
// With ACT != none the epilogue multiplies dX by act'(Z_prev) and the result
// is the previous layer's dZ; dX itself is never stored. The product is
// taken on the fp32 accumulator and rounded to bf16 once: rounding dX first
// (as heads_bwd_silu_kernel does) makes two roundings, up to 2**-7 relative,
// and the layer's gradient test allows one.
struct alignas(16) NzDgradLds {
  bf16_t dZ[2][128][NZ_LD];
  bf16_t Wt[2][128][NZ_LD];
};

template <int ACT>
__launch_bounds__(NZ_THREADS) __global__ void noisy_linear_dgrad_kernel(
    const void* __restrict__ dZ,        // [S, N] fp32 or bf16
    const float* __restrict__ mu_w,     // [N, K]
    const float* __restrict__ sigma_w,  // [N, K]
    const float* __restrict__ eps_in,   // [K]
    const float* __restrict__ eps_out,  // [N]
    const bf16_t* __restrict__ Z_prev,  // [S, K] (ACT != none)
    bf16_t* __restrict__ out,           // [S, K]
    int S, int K, int N, int dz_bf16, int noisy) {
  __shared__ NzDgradLds lds;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int m0 = blockIdx.x * 128;
  const int k_blk = blockIdx.y * 128;
  const int wm = (wid >> 1) * 64;
  const int wk = (wid & 1) * 64;
  const int l15 = lane & 15;
  const int g = lane >> 4;
  // dZ staging: row srow (+64 per q), reduction columns nh..nh+7
  const int srow = tid >> 2;
  const int nh = (tid & 3) * 8;
  // W staging: reduction row wn_, k-piece wkc (+64 columns per q)
  const int wn_ = tid & 31;
  const int wkc = (tid >> 5) * 8;
  const bool vec_n = (N & 7) == 0;

  float ein[2][8];
  bool kc_ok[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int k = k_blk + wkc + q * 64;
    kc_ok[q] = k < K;
#pragma unroll
    for (int i = 0; i < 8; ++i)
      ein[q][i] = (noisy && kc_ok[q]) ? eps_in[k + i] : 0.f;
  }

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  bf16x8 zr[2];
  NzW8 wr[2];
  float eo;
  auto load = [&](int ns) {
    const int n0 = ns * NZ_BK;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int m = m0 + srow + q * 64;
      zr[q] = nz_ld8(dZ, (long)m * N, n0 + nh, N, m < S, dz_bf16, vec_n);
    }
    const int n = n0 + wn_;
    const bool n_ok = n < N;
    eo = (noisy && n_ok) ? eps_out[n] : 0.f;
#pragma unroll
    for (int q = 0; q < 2; ++q)
      wr[q] = nz_ldw(mu_w, sigma_w, (long)n * K + k_blk + wkc + q * 64,
                     n_ok && kc_ok[q], noisy);
  };
  auto store = [&](int pp) {
#pragma unroll
    for (int q = 0; q < 2; ++q)
      *reinterpret_cast<bf16x8*>(&lds.dZ[pp][srow + q * 64][nh]) = zr[q];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const bf16x8 w = nz_form(wr[q], eo, ein[q], noisy);
#pragma unroll
      for (int i = 0; i < 8; ++i) lds.Wt[pp][wkc + q * 64 + i][wn_] = w[i];
    }
  };
  auto mma = [&](int pp) {
    bf16x8 zf[4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
      zf[mi] = *reinterpret_cast<const bf16x8*>(
          &lds.dZ[pp][wm + mi * 16 + l15][g * 8]);
#pragma unroll
    for (int kj = 0; kj < 4; ++kj) {
      const bf16x8 wf = *reinterpret_cast<const bf16x8*>(
          &lds.Wt[pp][wk + kj * 16 + l15][g * 8]);
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
        acc[mi][kj] = MFMA_BF16_16x16x32(wf, zf[mi], acc[mi][kj], 0, 0, 0);
    }
  };

  const int NS = (N + NZ_BK - 1) / NZ_BK;
  load(0);
  store(0);
  for (int ns = 0; ns + 1 < NS; ++ns) {
    __syncthreads();
    load(ns + 1);
    mma(ns & 1);
    store((ns + 1) & 1);
  }
  __syncthreads();
  mma((NS - 1) & 1);
  // The first read of the accumulator, in straight-line code after the
  // chain and ahead of the guarded stores (x + 0.0f is a real add).
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int kj = 0; kj < 4; ++kj)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[mi][kj][r] = acc[mi][kj][r] + 0.0f;

#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    const int m = m0 + wm + mi * 16 + l15;
    if (m >= S) continue;
#pragma unroll
    for (int kj = 0; kj < 4; ++kj) {
      const int k = k_blk + wk + kj * 16 + g * 4;
      if (k >= K) continue;  // K % 8 == 0 and k % 4 == 0: k + 3 < K
      const long o = (long)m * K + k;
      bf16x4 d4;
      if (ACT != NZ_ACT_NONE) {
        const bf16x4 zp = *reinterpret_cast<const bf16x4*>(Z_prev + o);
#pragma unroll
        for (int r = 0; r < 4; ++r)
          d4[r] = (bf16_t)(acc[mi][kj][r] * nz_act_grad((float)zp[r], ACT));
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) d4[r] = (bf16_t)acc[mi][kj][r];
      }
      *reinterpret_cast<bf16x4*>(out + o) = d4;
    }
  }
}

// -------------------------------------------------------------------- wgrad
// Partial dW[N, K] = dZ^T @ X over one slice of S, and the partial column
// sums of dZ. Grid (ceil(N/64), ceil(K/128), slices); workgroup tile 64 n x
// 128 k, waves 2 x 2 (32 n x 64 k each). Both tiles go to LDS transposed
// ([n][s] and [k][s]), consecutive lanes holding consecutive s of one piece.
// A operand = X^T fragment, B operand = dZ^T fragment: acc[ki][ni][r] is
// dW[n = ni*16 + (lane&15)][k = ki*16 + (lane>>4)*4 + r], one 16-byte store.
// The column sums come from the dZ^T fragments of the workgroups with
// blockIdx.y == 0. Slab image of a slice: dW [N*K] then db [N].
struct alignas(16) NzWgradLds {
  bf16_t dZt[2][64][NZ_LD];
  bf16_t Xt[2][128][NZ_LD];
};

__launch_bounds__(NZ_THREADS) __global__ void noisy_linear_wgrad_kernel(
    const void* __restrict__ dZ,  // [S, N] fp32 or bf16
    const void* __restrict__ X,   // [S, K] fp32 or bf16
    float* __restrict__ slab,     // [slices, slab_stride]
    long slab_stride, int S, int K, int N, int s_per, int dz_bf16,
    int x_bf16) {
  __shared__ NzWgradLds lds;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int n_blk = blockIdx.x * 64;
  const int k_blk = blockIdx.y * 128;
  const int s_begin = blockIdx.z * s_per;
  const int s_end = min(S, s_begin + s_per);
  const int wn = (wid >> 1) * 32;
  const int wk = (wid & 1) * 64;
  const int l15 = lane & 15;
  const int g = lane >> 4;
  // staging: row ss of the 32-row step, piece pc (dZ: 8 pieces of n; X: 16
  // pieces of k, two per thread)
  const int ss = tid & 31;
  const int pc = (tid >> 5) * 8;
  const bool vec_n = (N & 7) == 0;
  const bool do_db = blockIdx.y == 0 && wk == 0;

  f32x4 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};
  float db_acc[2] = {0.f, 0.f};

  bf16x8 zr, xr[2];
  auto load = [&](int st) {
    const int s = s_begin + st * NZ_BK + ss;
    const bool s_ok = s < s_end;
    zr = nz_ld8(dZ, (long)s * N, n_blk + pc, N, s_ok, dz_bf16, vec_n);
#pragma unroll
    for (int q = 0; q < 2; ++q)
      xr[q] = nz_ld8(X, (long)s * K, k_blk + pc + q * 64, K, s_ok, x_bf16,
                     true);
  };
  auto store = [&](int pp) {
#pragma unroll
    for (int i = 0; i < 8; ++i) lds.dZt[pp][pc + i][ss] = zr[i];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int i = 0; i < 8; ++i) lds.Xt[pp][pc + q * 64 + i][ss] = xr[q][i];
  };
  auto mma = [&](int pp) {
    bf16x8 zf[2];
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      zf[ni] = *reinterpret_cast<const bf16x8*>(
          &lds.dZt[pp][wn + ni * 16 + l15][g * 8]);
      if (do_db) {
#pragma unroll
        for (int j = 0; j < 8; ++j) db_acc[ni] += (float)zf[ni][j];
      }
    }
#pragma unroll
    for (int ki = 0; ki < 4; ++ki) {
      const bf16x8 xf = *reinterpret_cast<const bf16x8*>(
          &lds.Xt[pp][wk + ki * 16 + l15][g * 8]);
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
        acc[ki][ni] = MFMA_BF16_16x16x32(xf, zf[ni], acc[ki][ni], 0, 0, 0);
    }
  };

  const int NST = (s_end - s_begin + NZ_BK - 1) / NZ_BK;  // >= 1
  load(0);
  store(0);
  for (int st = 0; st + 1 < NST; ++st) {
    __syncthreads();
    load(st + 1);
    mma(st & 1);
    store((st + 1) & 1);
  }
  __syncthreads();
  mma((NST - 1) & 1);

  float* __restrict__ o = slab + (long)blockIdx.z * slab_stride;
  // The first read of the accumulator, in straight-line code after the
  // chain and ahead of the guarded stores: x + 0.0f is a real add (it turns
  // -0 into +0, so it cannot be folded away).
#pragma unroll
  for (int ki = 0; ki < 4; ++ki)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[ki][ni][r] = acc[ki][ni][r] + 0.0f;
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const int n = n_blk + wn + ni * 16 + l15;
    if (do_db) {
      float d = db_acc[ni];
      d += __shfl_xor(d, 16);
      d += __shfl_xor(d, 32);
      if (g == 0 && n < N) o[(long)N * K + n] = d;
    }
    if (n >= N) continue;
#pragma unroll
    for (int ki = 0; ki < 4; ++ki) {
      const int k = k_blk + wk + ki * 16 + g * 4;
      if (k < K)  // K % 8 == 0 and k % 4 == 0: k + 3 < K
        *reinterpret_cast<f32x4*>(o + (long)n * K + k) = acc[ki][ni];
    }
  }
}

// Sum the slices' slabs in ascending order and write the five gradients,
// each element once. dsigma_w / dsigma_b may be null (noise off).
extern "C" __global__ void __launch_bounds__(NZ_THREADS)
    noisy_wgrad_reduce_kernel(const float* __restrict__ slab,
                              long slab_stride, int slices,
                              const float* __restrict__ eps_in,
                              const float* __restrict__ eps_out,
                              float* __restrict__ dmu_w,
                              float* __restrict__ dsigma_w,
                              float* __restrict__ dmu_b,
                              float* __restrict__ dsigma_b, int K, int N) {
  const long nk = (long)N * K;
  const long total = nk + N;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += stride) {
    float s = 0.f;
    for (int z = 0; z < slices; ++z) s += slab[(long)z * slab_stride + i];
    if (i < nk) {
      const int n = (int)(i / K), k = (int)(i - (long)n * K);
      dmu_w[i] = s;
      if (dsigma_w) {
        const float e = eps_out[n] * eps_in[k];
        dsigma_w[i] = s * e;
      }
    } else {
      const int n = (int)(i - nk);
      dmu_b[n] = s;
      if (dsigma_b) dsigma_b[n] = s * eps_out[n];
    }
  }
}

// f(x) = sign(x) * sqrt(|x|) in place, bit for bit what the torch sequence
// sign / abs_ / sqrt_ / mul_ leaves: sign(+-0) = 0 (so f(+-0) = +0), the
// correctly rounded square root, one fp32 product.
extern "C" __global__ void __launch_bounds__(NZ_THREADS)
    noise_transform_kernel(float* __restrict__ x, long n) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    const float v = x[i];
    const float sg = (float)((0.f < v) - (v < 0.f));
    x[i] = sqrtf(fabsf(v)) * sg;  // IEEE sqrt; __fsqrt_rn is the native one
  }
}

// ----------------------------------------------------------- host launchers

static bool nz_shape_ok(int S, int K, int N) {
  return S >= 1 && N >= 1 && K >= 8 && (K & 7) == 0;
}

template <int BN>
static void nz_launch_fwd(const void* X, const float* mu_w,
                          const float* sigma_w, const float* mu_b,
                          const float* sigma_b, const float* eps_in,
                          const float* eps_out, void* Z, void* H, int S, int K,
                          int N, int x_bf16, int act, int noisy,
                          hipStream_t st) {
  dim3 grid((S + 127) / 128, (N + BN - 1) / BN), block(NZ_THREADS);
  auto kernel = act == NZ_ACT_SILU
                    ? noisy_linear_fwd_kernel<BN, NZ_ACT_SILU>
                    : act == NZ_ACT_RELU
                          ? noisy_linear_fwd_kernel<BN, NZ_ACT_RELU>
                          : noisy_linear_fwd_kernel<BN, NZ_ACT_NONE>;
  hipLaunchKernelGGL(kernel, grid, block, 0, st, X, mu_w, sigma_w, mu_b,
                     sigma_b, eps_in, eps_out, (bf16_t*)Z, (bf16_t*)H, S, K, N,
                     x_bf16, noisy);
}

extern "C" int launch_noisy_linear_fwd(
    const void* X, const float* mu_w, const float* sigma_w, const float* mu_b,
    const float* sigma_b, const float* eps_in, const float* eps_out, void* Z,
    void* H, int S, int K, int N, int x_bf16, int act, int noisy,
    void* stream) {
  if (!nz_shape_ok(S, K, N) || act < NZ_ACT_NONE || act > NZ_ACT_RELU)
    return 1;
  if (N <= 64)
    nz_launch_fwd<64>(X, mu_w, sigma_w, mu_b, sigma_b, eps_in, eps_out, Z, H,
                      S, K, N, x_bf16, act, noisy, (hipStream_t)stream);
  else
    nz_launch_fwd<128>(X, mu_w, sigma_w, mu_b, sigma_b, eps_in, eps_out, Z, H,
                       S, K, N, x_bf16, act, noisy, (hipStream_t)stream);
  return 0;
}

extern "C" int launch_noisy_linear_dgrad(
    const void* dZ, const float* mu_w, const float* sigma_w,
    const float* eps_in, const float* eps_out, const void* Z_prev, void* out,
    int S, int K, int N, int dz_bf16, int act_prev, int noisy, void* stream) {
  if (!nz_shape_ok(S, K, N) || act_prev < NZ_ACT_NONE ||
      act_prev > NZ_ACT_RELU || (act_prev != NZ_ACT_NONE && !Z_prev))
    return 1;
  dim3 grid((S + 127) / 128, (K + 127) / 128), block(NZ_THREADS);
  auto kernel = act_prev == NZ_ACT_SILU
                    ? noisy_linear_dgrad_kernel<NZ_ACT_SILU>
                    : act_prev == NZ_ACT_RELU
                          ? noisy_linear_dgrad_kernel<NZ_ACT_RELU>
                          : noisy_linear_dgrad_kernel<NZ_ACT_NONE>;
  hipLaunchKernelGGL(kernel, grid, block, 0, (hipStream_t)stream, dZ, mu_w,
                     sigma_w, eps_in, eps_out, (const bf16_t*)Z_prev,
                     (bf16_t*)out, S, K, N, dz_bf16, noisy);
  return 0;
}

// Slices of S: about 256 rows each, at most NZ_MAX_SPLIT, whole 32-row
// steps. A function of S alone, so the sum order is too.
extern "C" void noisy_wgrad_geometry(int S, int K, int N, int* slices,
                                     int* s_per, long* slab_stride) {
  int want = (S + 255) / 256;
  want = want < 1 ? 1 : (want > NZ_MAX_SPLIT ? NZ_MAX_SPLIT : want);
  int per = (S + want - 1) / want;
  per = (per + NZ_BK - 1) / NZ_BK * NZ_BK;
  *s_per = per;
  *slices = (S + per - 1) / per;
  // 16-byte aligned slab images for the 4-float stores
  *slab_stride = ((long)N * K + N + 3) / 4 * 4;
}

extern "C" int launch_noisy_linear_wgrad(
    const void* dZ, const void* X, float* slab, const float* eps_in,
    const float* eps_out, float* dmu_w, float* dsigma_w, float* dmu_b,
    float* dsigma_b, int S, int K, int N, int dz_bf16, int x_bf16,
    void* stream) {
  if (!nz_shape_ok(S, K, N)) return 1;
  int slices, s_per;
  long slab_stride;
  noisy_wgrad_geometry(S, K, N, &slices, &s_per, &slab_stride);
  dim3 grid((N + 63) / 64, (K + 127) / 128, slices), block(NZ_THREADS);
  hipLaunchKernelGGL(noisy_linear_wgrad_kernel, grid, block, 0,
                     (hipStream_t)stream, dZ, X, slab, slab_stride, S, K, N,
                     s_per, dz_bf16, x_bf16);
  const long total = (long)N * K + N;
  hipLaunchKernelGGL(noisy_wgrad_reduce_kernel,
                     dim3(flat_blocks(total, NZ_THREADS)), dim3(NZ_THREADS), 0,
                     (hipStream_t)stream, slab, slab_stride, slices, eps_in,
                     eps_out, dmu_w, dsigma_w, dmu_b, dsigma_b, K, N);
  return 0;
}

extern "C" void launch_noise_transform(float* x, long n, void* stream) {
  if (n <= 0) return;
  hipLaunchKernelGGL(noise_transform_kernel,
                     dim3(flat_blocks(n, NZ_THREADS)), dim3(NZ_THREADS), 0,
                     (hipStream_t)stream, x, n);
}
