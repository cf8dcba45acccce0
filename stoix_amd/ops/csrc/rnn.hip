// K13: fused done-masked RNN sequence scan.
//
// The reference's ScannedRNN (stoix/networks/base.py:124-159) is an
// nn.scan of a GRU/LSTM cell with per-step hidden reset on done. The
// recurrence is sequential in T but per-ROW independent, so the MI355X
// mapping is: one 16-row tile per workgroup that owns its rows for the
// WHOLE T loop — hidden state lives in LDS (fp32 master + bf16 mirror for
// MFMA) and never leaves the CU between steps; the input-side projection
// Xp = x @ W_ih^T + b_ih for ALL T is hoisted into one big hipBLASLt GEMM
// by the caller (the classic cuDNN trick), so the kernel does only the
// recurrent half: per step one [16,H]x[H,G*H] MFMA GEMM + gate math.
//
// Gate math matches nn.GRUCell / nn.LSTMCell exactly:
//   GRU  (gates r|z|n):  r = s(xr+hr)  z = s(xz+hz)
//                        n = tanh(xn + r*(h Whn + bhn));  h' = (1-z)n + z h
//   LSTM (gates i|f|g|o): c' = s(f)*c + s(i)*tanh(g);  h' = s(o)*tanh(c')
// The keep-mask (reset-before-consume) is applied to the fp32 master and
// the bf16 mirror at the top of each step.
//
// rnn_scan_kernel<H, LSTM, false> is the no-grad path (rollout acting,
// evaluation, R2D2 burn-in — which the reference runs under stop_gradient,
// rec_r2d2.py:300-317). The training scan is the same kernel with SAVE=true,
// which also stores the activated gates and one auxiliary value per element
// (GRU: hn = h Whn + bhn, LSTM: the new cell state), and rnn_scan_bwd_kernel
// below, the reverse scan that turns dHout into dXp, dHg and dh0/dc0
// (ops/rnn.py _RnnScan; weight and bias gradients are GEMMs in the caller).
#include "common.h"
#include "launchers.h"
#include <hip/hip_bf16.h>

typedef __bf16 bf16_t;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define MFMA_BF16_16x16x32 __builtin_amdgcn_mfma_f32_16x16x32_bf16

DEV_INLINE float bf2fr(bf16_t x) { return (float)x; }
DEV_INLINE bf16_t f2bfr(float x) { return (bf16_t)x; }
DEV_INLINE float sigm(float x) { return 1.0f / (1.0f + __expf(-x)); }
DEV_INLINE float tanh_r(float x) {
  return 1.0f - 2.0f / (__expf(2.0f * x) + 1.0f);
}

// B fragment loader: W row-major [G*H, H] bf16; tile row base `nrow`.
DEV_INLINE bf16x8 rnn_w_frag(const bf16_t* __restrict__ W, int K, int nrow,
                             int ks, int lane) {
  int n = nrow + (lane & 15);
  int k0 = ks * 32 + (lane >> 4) * 8;
  return *reinterpret_cast<const bf16x8*>(W + (long)n * K + k0);
}

constexpr int RPAD = 8;  // bf16 mirror column pad (conflict-free b128 reads)

template <int H, int GATES>
struct RnnLds {
  float hf[16][H];
  bf16_t hb[16][H + RPAD];
  float cf[16][GATES == 4 ? H : 1];  // LSTM cell state
};

template <int H, bool LSTM, bool SAVE>
__launch_bounds__(256, 2) __global__ void rnn_scan_kernel(
    const float* __restrict__ Xp,      // [T, B, G*H] input projections
    const bf16_t* __restrict__ Whh,    // [G*H, H] bf16
    const float* __restrict__ bhh,     // [G*H]
    const unsigned char* __restrict__ resets,  // [T, B]
    const float* __restrict__ h0,      // [B, H]
    const float* __restrict__ c0,      // [B, H] (LSTM) or null
    float* __restrict__ Hout,          // [T, B, H]
    float* __restrict__ hT,            // [B, H]
    float* __restrict__ cT,            // [B, H] (LSTM) or null
    float* __restrict__ gates,         // SAVE: [T, B, G*H] activated gates
    float* __restrict__ aux,           // SAVE: [T, B, H] hn (GRU) / c_t (LSTM)
    int T, int B) {
  constexpr int G = LSTM ? 4 : 3;
  __shared__ RnnLds<H, G> lds;
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int rbase = blockIdx.x * 16;
  if (rbase >= B) return;
  constexpr int STRIP = H / 4;       // columns per wave
  constexpr int NTW = STRIP / 16;    // 16-col tiles per gate per wave
  const int strip0 = wid * STRIP;

  // stage h0 (and c0)
  for (int i = threadIdx.x; i < 16 * H; i += 256) {
    int r = i / H, k = i - r * H;
    float v = (rbase + r < B) ? h0[(long)(rbase + r) * H + k] : 0.0f;
    lds.hf[r][k] = v;
    lds.hb[r][k] = f2bfr(v);
    if (LSTM) {
      float cv = (rbase + r < B && c0) ? c0[(long)(rbase + r) * H + k] : 0.0f;
      lds.cf[r][k] = cv;
    }
  }
  __syncthreads();

  const int arow = lane & 15;
  const int ak0 = (lane >> 4) * 8;
  const int col = lane & 15;
  const int grp = lane >> 4;

  for (int t = 0; t < T; ++t) {
    // ---- reset-before-consume mask
    for (int i = threadIdx.x; i < 16 * H; i += 256) {
      int r = i / H, k = i - r * H;
      unsigned char rs =
          (rbase + r < B) ? resets[(long)t * B + rbase + r] : 0;
      if (rs) {
        lds.hf[r][k] = 0.0f;
        lds.hb[r][k] = f2bfr(0.0f);
        if (LSTM) lds.cf[r][k] = 0.0f;
      }
    }
    __syncthreads();

    // ---- recurrent GEMM: gates for this wave's column strip
    f32x4 acc[4][NTW];  // [gate][tile]
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int n = 0; n < NTW; ++n) acc[g][n] = {0.f, 0.f, 0.f, 0.f};
    for (int ks = 0; ks < H / 32; ++ks) {
      const bf16x8 a = *reinterpret_cast<const bf16x8*>(
          &lds.hb[arow][0] + ks * 32 + ak0);
#pragma unroll
      for (int g = 0; g < G; ++g) {
#pragma unroll
        for (int n = 0; n < NTW; ++n) {
          bf16x8 b = rnn_w_frag(Whh, H, g * H + strip0 + n * 16, ks, lane);
          acc[g][n] = MFMA_BF16_16x16x32(a, b, acc[g][n], 0, 0, 0);
        }
      }
    }
    // ---- read own h_old (and c_old) BEFORE the write barrier
    float hold[4][NTW], cold[4][NTW];
#pragma unroll
    for (int n = 0; n < NTW; ++n) {
      int cg = strip0 + n * 16 + col;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        hold[r][n] = lds.hf[grp * 4 + r][cg];
        if (LSTM) cold[r][n] = lds.cf[grp * 4 + r][cg];
      }
    }
    __syncthreads();

    // ---- gate math + state update + output write
#pragma unroll
    for (int n = 0; n < NTW; ++n) {
      int cg = strip0 + n * 16 + col;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = grp * 4 + r;
        int grow = rbase + row;
        if (grow >= B) continue;
        const long xbase = ((long)t * B + grow) * (G * H);
        float hnew;
        if (!LSTM) {
          float xr = Xp[xbase + cg];
          float xz = Xp[xbase + H + cg];
          float xn = Xp[xbase + 2 * H + cg];
          float hr = acc[0][n][r] + bhh[cg];
          float hz = acc[1][n][r] + bhh[H + cg];
          float hn = acc[2][n][r] + bhh[2 * H + cg];
          float rg = sigm(xr + hr);
          float zg = sigm(xz + hz);
          float ng = tanh_r(xn + rg * hn);
          hnew = (1.0f - zg) * ng + zg * hold[r][n];
          if (SAVE) {
            gates[xbase + cg] = rg;
            gates[xbase + H + cg] = zg;
            gates[xbase + 2 * H + cg] = ng;
            aux[((long)t * B + grow) * H + cg] = hn;
          }
        } else {
          float xi = Xp[xbase + cg];
          float xf = Xp[xbase + H + cg];
          float xg = Xp[xbase + 2 * H + cg];
          float xo = Xp[xbase + 3 * H + cg];
          float ig = sigm(xi + acc[0][n][r] + bhh[cg]);
          float fg = sigm(xf + acc[1][n][r] + bhh[H + cg]);
          float gg = tanh_r(xg + acc[2][n][r] + bhh[2 * H + cg]);
          float og = sigm(xo + acc[3][n][r] + bhh[3 * H + cg]);
          float cnew = fg * cold[r][n] + ig * gg;
          lds.cf[row][cg] = cnew;
          hnew = og * tanh_r(cnew);
          if (SAVE) {
            gates[xbase + cg] = ig;
            gates[xbase + H + cg] = fg;
            gates[xbase + 2 * H + cg] = gg;
            gates[xbase + 3 * H + cg] = og;
            aux[((long)t * B + grow) * H + cg] = cnew;
          }
        }
        lds.hf[row][cg] = hnew;
        lds.hb[row][cg] = f2bfr(hnew);
        Hout[((long)t * B + grow) * H + cg] = hnew;
      }
    }
    __syncthreads();
  }

  // ---- final state
  for (int i = threadIdx.x; i < 16 * H; i += 256) {
    int r = i / H, k = i - r * H;
    if (rbase + r < B) {
      hT[(long)(rbase + r) * H + k] = lds.hf[r][k];
      if (LSTM && cT) cT[(long)(rbase + r) * H + k] = lds.cf[r][k];
    }
  }
}

// ------------------------------------------------ backward through time
//
// Reverse scan t = T-1 .. 0 over what the SAVE forward stored. Same tiling
// as the forward: one 16-row tile per workgroup, wave w owns hidden columns
// [w*H/4, (w+1)*H/4), and a thread owns the (row, col) elements of the MFMA
// accumulator layout (rows 4*grp+r, column col of each 16-column tile). The
// recurrent product dh_prev = dHg[16, G*H] @ Whh[G*H, H] has H output
// columns, so its accumulator lands on exactly the elements whose gate math
// the thread does: the dh/dc carries never change owner and stay in
// registers for the whole T loop. LDS holds only the bf16 A tile of dHg.
//
//   GRU :  dn = dh(1-z)(1-n^2)  dz = dh(h_prev-n)z(1-z)  dr = dn*hn*r(1-r)
//          dXp = (dr,dz,dn)   dHg = (dr,dz,dn*r)   direct = dh*z
//   LSTM:  dc += dh*o(1-tanh(c)^2)
//          dXp = dHg = (dc*g*i(1-i), dc*c_prev*f(1-f), dc*i(1-g^2),
//                       dh*tanh(c)*o(1-o))          dc_prev = dc*f
//   carry: dh = keep_t*(direct + dh_prev), dc = keep_t*dc_prev
//
// h_prev / c_prev are rebuilt as keep_t * (t == 0 ? h0 : Hout[t-1]) (and
// c0 / aux). Every element of dXp, dHg, dh0, dc0 in rows < B is written
// once; rows >= B of the last tile are neither read nor written (their A
// tile rows are zero). No atomics.

template <int H, int GATES>
struct RnnBwdLds {
  bf16_t a[16][GATES * H + RPAD];  // same 16-byte row skew as RnnLds::hb
};

template <int H, bool LSTM>
__launch_bounds__(256, 2) __global__ void rnn_scan_bwd_kernel(
    const float* __restrict__ dHout,   // [T, B, H]
    const float* __restrict__ dhT,     // [B, H] or null (zeros)
    const float* __restrict__ dcT,     // [B, H] or null (zeros)
    const float* __restrict__ gates,   // [T, B, G*H] activated gates
    const float* __restrict__ aux,     // [T, B, H] hn (GRU) / c_t (LSTM)
    const float* __restrict__ Hout,    // [T, B, H]
    const float* __restrict__ h0,      // [B, H]
    const float* __restrict__ c0,      // [B, H] (LSTM) or null
    const unsigned char* __restrict__ resets,  // [T, B]
    const bf16_t* __restrict__ WhhT,   // [H, G*H] bf16 = Whh^T
    float* __restrict__ dXp,           // [T, B, G*H]
    float* __restrict__ dHg,           // [T, B, G*H] (GRU; LSTM: dXp is dHg)
    float* __restrict__ dh0,           // [B, H]
    float* __restrict__ dc0,           // [B, H] (LSTM) or null
    int T, int B) {
  constexpr int G = LSTM ? 4 : 3;
  constexpr int GH = G * H;
  __shared__ RnnBwdLds<H, G> lds;
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int rbase = blockIdx.x * 16;
  if (rbase >= B) return;
  constexpr int STRIP = H / 4;
  constexpr int NTW = STRIP / 16;
  const int strip0 = wid * STRIP;
  const int arow = lane & 15;
  const int ak0 = (lane >> 4) * 8;
  const int col = lane & 15;
  const int grp = lane >> 4;

  float dh[4][NTW], dc[4][NTW];
#pragma unroll
  for (int n = 0; n < NTW; ++n) {
    int cg = strip0 + n * 16 + col;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int grow = rbase + grp * 4 + r;
      bool ok = grow < B;
      dh[r][n] = (ok && dhT) ? dhT[(long)grow * H + cg] : 0.0f;
      dc[r][n] = (LSTM && ok && dcT) ? dcT[(long)grow * H + cg] : 0.0f;
    }
  }

  for (int t = T - 1; t >= 0; --t) {
    float keep[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int grow = rbase + grp * 4 + r;
      keep[r] = (grow < B && resets[(long)t * B + grow]) ? 0.0f : 1.0f;
    }

    // ---- gate math on the thread's own elements; bf16(dHg) -> A tile
    float direct[4][NTW];
#pragma unroll
    for (int n = 0; n < NTW; ++n) {
      int cg = strip0 + n * 16 + col;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = grp * 4 + r;
        int grow = rbase + row;
        float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f, dir = 0.f;
        if (grow < B) {
          const long hb = ((long)t * B + grow) * H + cg;
          const long gb = ((long)t * B + grow) * GH + cg;
          const long sb = (long)grow * H + cg;
          const float dhv = dh[r][n] + dHout[hb];
          if (!LSTM) {
            float rg = gates[gb];
            float zg = gates[gb + H];
            float ng = gates[gb + 2 * H];
            float hn = aux[hb];
            float hp = keep[r] * (t == 0 ? h0[sb] : Hout[hb - (long)B * H]);
            float dn_pre = dhv * (1.0f - zg) * (1.0f - ng * ng);
            float dz_pre = dhv * (hp - ng) * zg * (1.0f - zg);
            float dr_pre = dn_pre * hn * rg * (1.0f - rg);
            float dhn = dn_pre * rg;
            dir = dhv * zg;
            dXp[gb] = dr_pre;
            dXp[gb + H] = dz_pre;
            dXp[gb + 2 * H] = dn_pre;
            dHg[gb] = dr_pre;
            dHg[gb + H] = dz_pre;
            dHg[gb + 2 * H] = dhn;
            v0 = dr_pre;
            v1 = dz_pre;
            v2 = dhn;
          } else {
            float ig = gates[gb];
            float fg = gates[gb + H];
            float gg = gates[gb + 2 * H];
            float og = gates[gb + 3 * H];
            float ct = aux[hb];
            float c_in = t == 0 ? (c0 ? c0[sb] : 0.0f) : aux[hb - (long)B * H];
            float cp = keep[r] * c_in;
            float tc = tanh_r(ct);
            float dcv = dc[r][n] + dhv * og * (1.0f - tc * tc);
            v0 = dcv * gg * ig * (1.0f - ig);
            v1 = dcv * cp * fg * (1.0f - fg);
            v2 = dcv * ig * (1.0f - gg * gg);
            v3 = dhv * tc * og * (1.0f - og);
            dc[r][n] = dcv * fg;  // dc_prev; keep_t applied with the carry
            dXp[gb] = v0;
            dXp[gb + H] = v1;
            dXp[gb + 2 * H] = v2;
            dXp[gb + 3 * H] = v3;
          }
        }
        direct[r][n] = dir;
        lds.a[row][cg] = f2bfr(v0);
        lds.a[row][H + cg] = f2bfr(v1);
        lds.a[row][2 * H + cg] = f2bfr(v2);
        if (LSTM) lds.a[row][3 * H + cg] = f2bfr(v3);
      }
    }
    __syncthreads();

    // ---- dh_prev = dHg @ Whh for this wave's column strip; even and odd
    // k-steps go to two accumulators so each tile has two MFMA chains
    f32x4 acc[2][NTW];
#pragma unroll
    for (int n = 0; n < NTW; ++n) {
      acc[0][n] = {0.f, 0.f, 0.f, 0.f};
      acc[1][n] = {0.f, 0.f, 0.f, 0.f};
    }
    // A full unroll lets the compiler hoist the t-invariant Whh fragments
    // out of the T loop: at H=128 they fit in registers (no spill) and the
    // weights are then read once; at H=256 they spill ~1 KB/lane, so there
    // only two iterations are kept in flight.
    constexpr int KUNROLL = H == 128 ? GH / 64 : 2;
#pragma unroll KUNROLL
    for (int ks = 0; ks < GH / 32; ks += 2) {
      const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(
          &lds.a[arow][0] + ks * 32 + ak0);
      const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(
          &lds.a[arow][0] + (ks + 1) * 32 + ak0);
#pragma unroll
      for (int n = 0; n < NTW; ++n) {
        bf16x8 b0 = rnn_w_frag(WhhT, GH, strip0 + n * 16, ks, lane);
        bf16x8 b1 = rnn_w_frag(WhhT, GH, strip0 + n * 16, ks + 1, lane);
        acc[0][n] = MFMA_BF16_16x16x32(a0, b0, acc[0][n], 0, 0, 0);
        acc[1][n] = MFMA_BF16_16x16x32(a1, b1, acc[1][n], 0, 0, 0);
      }
    }
    // ---- new carry: straight-line after the MFMA chain, no branch before
    // the first accumulator read (docs/KERNELS.md)
#pragma unroll
    for (int n = 0; n < NTW; ++n) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        dh[r][n] = keep[r] * (direct[r][n] + (acc[0][n][r] + acc[1][n][r]));
        if (LSTM) dc[r][n] = keep[r] * dc[r][n];
      }
    }
    __syncthreads();  // A tile is rewritten by the next step
  }

  // ---- carries after t = 0 are dh0 / dc0
#pragma unroll
  for (int n = 0; n < NTW; ++n) {
    int cg = strip0 + n * 16 + col;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int grow = rbase + grp * 4 + r;
      if (grow < B) {
        dh0[(long)grow * H + cg] = dh[r][n];
        if (LSTM && dc0) dc0[(long)grow * H + cg] = dc[r][n];
      }
    }
  }
}

// --------------------------------------------------------- host launchers

template <bool SAVE>
static void rnn_scan_dispatch(const float* Xp, const void* Whh,
                              const float* bhh, const unsigned char* resets,
                              const float* h0, const float* c0, float* Hout,
                              float* hT, float* cT, float* gates, float* aux,
                              int T, int B, int H, int lstm, hipStream_t s) {
  dim3 grid((B + 15) / 16), block(256);
  const bf16_t* W = (const bf16_t*)Whh;
  if (H == 256) {
    if (lstm)
      hipLaunchKernelGGL((rnn_scan_kernel<256, true, SAVE>), grid, block, 0,
                         s, Xp, W, bhh, resets, h0, c0, Hout, hT, cT, gates,
                         aux, T, B);
    else
      hipLaunchKernelGGL((rnn_scan_kernel<256, false, SAVE>), grid, block, 0,
                         s, Xp, W, bhh, resets, h0, c0, Hout, hT, cT, gates,
                         aux, T, B);
  } else {
    if (lstm)
      hipLaunchKernelGGL((rnn_scan_kernel<128, true, SAVE>), grid, block, 0,
                         s, Xp, W, bhh, resets, h0, c0, Hout, hT, cT, gates,
                         aux, T, B);
    else
      hipLaunchKernelGGL((rnn_scan_kernel<128, false, SAVE>), grid, block, 0,
                         s, Xp, W, bhh, resets, h0, c0, Hout, hT, cT, gates,
                         aux, T, B);
  }
}

extern "C" void launch_rnn_scan(const float* Xp, const void* Whh,
                                const float* bhh,
                                const unsigned char* resets, const float* h0,
                                const float* c0, float* Hout, float* hT,
                                float* cT, int T, int B, int H, int lstm,
                                void* stream) {
  rnn_scan_dispatch<false>(Xp, Whh, bhh, resets, h0, c0, Hout, hT, cT,
                           nullptr, nullptr, T, B, H, lstm,
                           (hipStream_t)stream);
}

extern "C" void launch_rnn_scan_train_fwd(
    const float* Xp, const void* Whh, const float* bhh,
    const unsigned char* resets, const float* h0, const float* c0,
    float* Hout, float* hT, float* cT, float* gates, float* aux, int T, int B,
    int H, int lstm, void* stream) {
  rnn_scan_dispatch<true>(Xp, Whh, bhh, resets, h0, c0, Hout, hT, cT, gates,
                          aux, T, B, H, lstm, (hipStream_t)stream);
}

extern "C" void launch_rnn_scan_bwd(
    const float* dHout, const float* dhT, const float* dcT,
    const float* gates, const float* aux, const float* Hout, const float* h0,
    const float* c0, const unsigned char* resets, const void* WhhT,
    float* dXp, float* dHg, float* dh0, float* dc0, int T, int B, int H,
    int lstm, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  dim3 grid((B + 15) / 16), block(256);
  const bf16_t* W = (const bf16_t*)WhhT;
  if (H == 256) {
    if (lstm)
      hipLaunchKernelGGL((rnn_scan_bwd_kernel<256, true>), grid, block, 0, s,
                         dHout, dhT, dcT, gates, aux, Hout, h0, c0, resets, W,
                         dXp, dHg, dh0, dc0, T, B);
    else
      hipLaunchKernelGGL((rnn_scan_bwd_kernel<256, false>), grid, block, 0, s,
                         dHout, dhT, dcT, gates, aux, Hout, h0, c0, resets, W,
                         dXp, dHg, dh0, dc0, T, B);
  } else {
    if (lstm)
      hipLaunchKernelGGL((rnn_scan_bwd_kernel<128, true>), grid, block, 0, s,
                         dHout, dhT, dcT, gates, aux, Hout, h0, c0, resets, W,
                         dXp, dHg, dh0, dc0, T, B);
    else
      hipLaunchKernelGGL((rnn_scan_bwd_kernel<128, false>), grid, block, 0, s,
                         dHout, dhT, dcT, gates, aux, Hout, h0, c0, resets, W,
                         dXp, dHg, dh0, dc0, T, B);
  }
}

