// The fp32 Gaussian actor (FeedForwardActor: MLPTorso + NormalAffineTanh head,
// the actor of SAC, MPO, AWR and the other fp32 continuous systems) as two
// kernels on v_mfma_f32_16x16x4_f32:
//
//   forward  H_l = act(H_{l-1} W_l^T + b_l), l = 1..L, then
//            loc = H_L Wloc^T + bloc,
//            scale = softplus(H_L Wscale^T + bscale) + min_scale
//                                                        actor_mlp_fwd_kernel
//   dgrad    dspre = dscale * softplus'(spre),
//            dH_L = dloc Wloc + dspre Wscale, dZ_l = dH_l * act'(.),
//            dH_{l-1} = dZ_l W_l, l = L..2               actor_mlp_dgrad_kernel
//
// each the whole chain in ONE launch. The weight gradients are the Q-ensemble
// wgrad kernel's (qens.hip) on the dZ_l this file stores.
//
// Split of the work: a workgroup of 256 threads = 4 waves owns one 16-row
// tile of the batch through every layer (128 workgroups at S = 2048). The
// tile's activations stay in LDS, two buffers [16][256 + 4] that swap roles
// from layer to layer; a layer's 16-column output tiles are dealt to the four
// waves round-robin (tile t to wave t % 4), one accumulator each.
//
// With one row tile per workgroup a weight element meets exactly one MFMA of
// that workgroup, so W is not staged in LDS: a lane loads its fragment from
// global / L2 straight into registers, one batch of four 16-deep reduction
// groups (64 k) ahead of the MFMAs that use it. In the forward lane (i, kq)
// needs W[n0 + i][k + 4 kq .. + 3]: one 16-byte load (by element where the row
// length or the pointer forbid it, K0 = 27). In the dgrad the reduction runs
// down a column of W: four 4-byte loads, the 16 lanes of an i-group reading
// one 64-byte run of a row.
//
// Operand mapping as in qens.hip: lane (i, kq) takes k = 4 kq + s at MFMA step
// s on both operands, so the activation fragment of a group is ONE
// ds_read_b128 at [i][16 group + 4 kq]. LDS rows are 260 floats: the 16 rows of
// a b128 phase start at 260 i mod 64 = 4 i, 16 distinct multiples of 4, so
// 16 x 4 dwords cover the 64 banks once (the bank rule of docs/KERNELS.md).
// A operand = W fragment, B operand = activation fragment: a lane ends with
// row i, columns n0 + 4 kq .. + 3, i.e. 16-byte LDS and global stores.
//
// A batch always runs its four groups: the buffer columns between a layer's
// width and the next multiple of 64 are zero-filled (and the W fragments of a
// group past the end are zeros), so the last batch of a chain and the first
// read of its accumulator are straight-line code with no branch in between
// (docs/KERNELS.md, "Who wins which GEMM"); biases and the saved H / Z of the
// epilogue are fetched ahead of the chain.
//
// The layer-1 input is staged through LDS in chunks of 256 columns (register
// prefetch of the next chunk behind the MFMAs of this one), the K tail and the
// rows past S zero-filled; every later input is already there. Rows past S are
// never read from or written to memory. No atomics, every sum in a fixed
// order: two runs give the same bits.
#include "common.h"
#include "launchers.h"

// No product is fused into an add: softplus, its derivative and act' round as
// the expressions are written.
#pragma clang fp contract(off)

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define MFMA_F32_16x16x4 __builtin_amdgcn_mfma_f32_16x16x4f32

#define AM_THREADS 256
#define AM_ROWS 16
#define AM_KC 256            // widest layer, and the layer-1 chunk
#define AM_LD (AM_KC + 4)    // padded LDS row, in floats
#define AM_ACT_SILU 1        // the codes of ops/noisy.py ACT_CODES
#define AM_ACT_RELU 2
#define AM_SOFTPLUS_THRESHOLD 20.f
// 16-byte access flags: bit l = W of hidden layer l, then the head, then X
#define AM_VEC_HEAD (1 << ACTOR_MAX_L)
#define AM_VEC_X (2 << ACTOR_MAX_L)

typedef float (*AmTile)[AM_LD];

// Entry l of a by-value table, without indexing the kernel argument by a
// register (which would move the table to scratch).
template <typename T>
DEV_INLINE T am_pick(const T (&p)[ACTOR_MAX_L], int l) {
  return l == 0 ? p[0] : l == 1 ? p[1] : l == 2 ? p[2] : p[3];
}

// Where this lane sits: wave, row i of a fragment, k-quarter kq.
struct AmLane {
  int tid, wid, i, kq;
};

// Elements [col, col + 4) of the row at p[row]; zero where !ok or past ncols.
DEV_INLINE f32x4 am_ld4(const float* __restrict__ p, long row, int col,
                        int ncols, bool ok, bool vec) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (!ok || col >= ncols) return v;
  if (vec && col + 3 < ncols)
    return *reinterpret_cast<const f32x4*>(p + row + col);
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (col + j < ncols) v[j] = p[row + col + j];
  return v;
}

// ------------------------------------------------- weight fragment loaders
// ld(n0, k): the lane's four A-operand values of the 16-deep reduction group
// that starts at k, for the output tile that starts at column n0.

// Forward, hidden layer: W [N, K], output column = row of W.
struct AmWRow {
  const float* __restrict__ W;
  int K, N;
  bool vec;
  DEV_INLINE f32x4 ld(const AmLane& ln, int n0, int k) const {
    const int n = n0 + ln.i;
    return am_ld4(W, (long)n * K, k + 4 * ln.kq, K, n < N, vec);
  }
};

// Forward, head: [Wloc | Wscale] as one layer of 2A columns, each [A, K].
struct AmWHeadRow {
  const float* __restrict__ Wl;
  const float* __restrict__ Ws;
  int K, A;
  bool vec;
  DEV_INLINE f32x4 ld(const AmLane& ln, int n0, int k) const {
    const int n = n0 + ln.i;
    const float* __restrict__ p = n < A ? Wl + (long)n * K : Ws + (long)(n - A) * K;
    return am_ld4(p, 0, k + 4 * ln.kq, K, n < 2 * A, vec);
  }
};

// Dgrad, hidden layer: dX = dZ W with W [N, K], reduction over the rows of W,
// output column n0 + i < K (K is a multiple of 16).
struct AmWCol {
  const float* __restrict__ W;
  int K, N;
  DEV_INLINE f32x4 ld(const AmLane& ln, int n0, int k) const {
    f32x4 v;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int n = k + 4 * ln.kq + s;
      v[s] = n < N ? W[(long)n * K + n0 + ln.i] : 0.f;
    }
    return v;
  }
};

// Dgrad, head: dH_L = [dloc | dspre] [Wloc ; Wscale], one reduction over 2A.
struct AmWHeadCol {
  const float* __restrict__ Wl;
  const float* __restrict__ Ws;
  int K, A;
  DEV_INLINE f32x4 ld(const AmLane& ln, int n0, int k) const {
    f32x4 v;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int n = k + 4 * ln.kq + s;
      const long c = n0 + ln.i;
      v[s] = n < A ? Wl[(long)n * K + c]
                   : n < 2 * A ? Ws[(long)(n - A) * K + c] : 0.f;
    }
    return v;
  }
};

// ---------------------------------------------------------- the MFMA chain
// Batch b of a chunk: the W fragments of groups 4b .. 4b + 3, zeros past G.
template <class WL>
DEV_INLINE void am_ldbatch(const WL& wl, const AmLane& ln, int n0, int k0,
                           int b, int G, f32x4 (&w)[4]) {
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int gi = 4 * b + p;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    w[p] = gi < G ? wl.ld(ln, n0, k0 + 16 * gi) : zero;
  }
}

// 16 MFMAs on one batch; x points at the lane's [i][4 kq] of the batch.
DEV_INLINE void am_mma_batch(f32x4& acc, const f32x4 (&w)[4],
                             const float* x) {
  f32x4 xf[4];
#pragma unroll
  for (int p = 0; p < 4; ++p)
    xf[p] = *reinterpret_cast<const f32x4*>(x + 16 * p);
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int s = 0; s < 4; ++s)
      acc = MFMA_F32_16x16x4(w[p][s], xf[p][s], acc, 0, 0, 0);
}

// acc += the G reduction groups of one chunk (G >= 1, at most 16): W batch
// b + 1 is in flight behind the MFMAs of batch b; the last batch is peeled.
template <class WL>
DEV_INLINE void am_chunk(f32x4& acc, const WL& wl, const AmLane& ln, int n0,
                         int k0, int G, const float* xrow) {
  const int NB = (G + 3) >> 2;
  f32x4 w[4], wn[4];
  am_ldbatch(wl, ln, n0, k0, 0, G, w);
  for (int b = 0; b + 1 < NB; ++b) {
    am_ldbatch(wl, ln, n0, k0, b + 1, G, wn);
    am_mma_batch(acc, w, xrow + 64 * b);
#pragma unroll
    for (int p = 0; p < 4; ++p) w[p] = wn[p];
  }
  am_mma_batch(acc, w, xrow + 64 * (NB - 1));
}

// The layer-1 input: X [S, K0] staged chunk by chunk, 4 x 16 bytes a thread.
struct AmStage {
  const float* __restrict__ X;
  int S, K0, m0;
  bool vec;
  DEV_INLINE void load(const AmLane& ln, int c, f32x4 (&xr)[4]) const {
    const int r = ln.tid >> 4;
    const long m = m0 + r;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      xr[q] = am_ld4(X, m * K0, c * AM_KC + (ln.tid & 15) * 4 + q * 64, K0,
                     m < S, vec);
  }
  DEV_INLINE void store(const AmLane& ln, AmTile in, const f32x4 (&xr)[4]) const {
#pragma unroll
    for (int q = 0; q < 4; ++q)
      *reinterpret_cast<f32x4*>(&in[ln.tid >> 4][(ln.tid & 15) * 4 + q * 64]) =
          xr[q];
  }
};

// One layer for the workgroup's row tile: out tile t (columns 16 t ..) =
// epi(in[16][K] x the loader's W), the tiles t = wave, wave + 4, .. of each
// wave one after the other. `in` holds the input (K <= 256), complete and
// fenced by the caller's barrier, with zeros up to the next multiple of 64
// columns.
template <class WL, class EPI>
DEV_INLINE void am_layer(AmTile in, const WL& wl, int ntiles, int K,
                         const EPI& epi, const AmLane& ln) {
  const float* xrow = &in[ln.i][4 * ln.kq];
  const int G = (K + 15) >> 4;
  for (int t = ln.wid; t < ntiles; t += 4) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const f32x4 pre = epi.fetch(ln, t * 16);
    am_chunk(acc, wl, ln, t * 16, 0, G, xrow);
    epi.finish(ln, t * 16, acc, pre);
  }
}

// The first layer: the input comes from memory in chunks of 256 columns, so
// a wave keeps the accumulators of its (at most four) tiles across the
// chunks. Every thread of the workgroup must call this (barriers inside).
template <class WL, class EPI>
DEV_INLINE void am_layer_staged(AmTile in, const WL& wl, int ntiles, int K,
                                const AmStage& stage, const EPI& epi,
                                const AmLane& ln) {
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc[4] = {zero, zero, zero, zero};
  const float* xrow = &in[ln.i][4 * ln.kq];
  const int NC = (K + AM_KC - 1) / AM_KC;
  f32x4 xr[4];
  stage.load(ln, 0, xr);
  for (int c = 0; c + 1 < NC; ++c) {
    __syncthreads();  // the previous chunk has been read
    stage.store(ln, in, xr);
    __syncthreads();
    stage.load(ln, c + 1, xr);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int t = ln.wid + 4 * j;
      if (t < ntiles)
        am_chunk(acc[j], wl, ln, t * 16, c * AM_KC, AM_KC / 16, xrow);
    }
  }
  __syncthreads();
  stage.store(ln, in, xr);
  __syncthreads();
  const int k0 = (NC - 1) * AM_KC;
  const int G = (K - k0 + 15) >> 4;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int t = ln.wid + 4 * j;
    if (t < ntiles) {
      const f32x4 pre = epi.fetch(ln, t * 16);
      am_chunk(acc[j], wl, ln, t * 16, k0, G, xrow);
      epi.finish(ln, t * 16, acc[j], pre);
    }
  }
}

// Zeros in columns [N, next multiple of 64) of a buffer whose first N columns
// (N a multiple of 16) the layer's epilogues write.
DEV_INLINE void am_zero_pad(AmTile out, int N, const AmLane& ln) {
  const int n4 = (((N + 63) & ~63) - N) >> 2;  // 16-byte pieces per row, <= 12
  if (ln.tid < AM_ROWS * n4) {
    const int r = ln.tid / n4;
    const int c = N + (ln.tid - r * n4) * 4;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    *reinterpret_cast<f32x4*>(&out[r][c]) = zero;
  }
}

// ---------------------------------------------------------------- epilogues
// fetch() runs ahead of the chain, finish() straight after it; the lane holds
// row i, columns n0 + 4 kq .. + 3 of the tile.

// Forward hidden layer: h = act(acc + b) to LDS, H (and Z for SiLU) to memory
// when a backward follows.
template <int ACT>
struct AmEpiHidden {
  const float* __restrict__ b;
  float* __restrict__ H;  // [S, N] or null
  float* __restrict__ Z;  // [S, N] or null
  AmTile out;
  int N;
  long m;  // this lane's row of the batch
  bool row_ok;
  DEV_INLINE f32x4 fetch(const AmLane& ln, int n0) const {
    const int n = n0 + 4 * ln.kq;
    const f32x4 v = {b[n], b[n + 1], b[n + 2], b[n + 3]};
    return v;
  }
  DEV_INLINE void finish(const AmLane& ln, int n0, f32x4 acc, f32x4 bv) const {
    f32x4 z, h;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      z[r] = acc[r] + bv[r];
      h[r] = ACT == AM_ACT_SILU ? silu_f(z[r]) : (z[r] > 0.f ? z[r] : 0.f);
    }
    const int n = n0 + 4 * ln.kq;
    *reinterpret_cast<f32x4*>(&out[ln.i][n]) = h;
    if (row_ok && H) {
      *reinterpret_cast<f32x4*>(H + m * N + n) = h;
      if (ACT == AM_ACT_SILU && Z) *reinterpret_cast<f32x4*>(Z + m * N + n) = z;
    }
  }
};

// torch's softplus (beta 1, threshold 20) and its derivative.
DEV_INLINE float am_softplus(float x) {
  return x > AM_SOFTPLUS_THRESHOLD ? x : log1pf(expf(x));
}
DEV_INLINE float am_softplus_grad(float x) {
  const float z = expf(x);
  return x > AM_SOFTPLUS_THRESHOLD ? 1.f : z / (z + 1.f);
}

// Forward head: columns [0, A) are loc, [A, 2A) the scale's pre-activation.
struct AmEpiHead {
  const float* __restrict__ bl;
  const float* __restrict__ bs;
  float* __restrict__ loc;
  float* __restrict__ scale;
  float* __restrict__ spre;  // or null
  int A;
  float min_scale;
  long m;
  bool row_ok;
  DEV_INLINE f32x4 fetch(const AmLane& ln, int n0) const {
    f32x4 v;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = n0 + 4 * ln.kq + r;
      v[r] = n < A ? bl[n] : n < 2 * A ? bs[n - A] : 0.f;
    }
    return v;
  }
  DEV_INLINE void finish(const AmLane& ln, int n0, f32x4 acc, f32x4 bv) const {
    f32x4 z;
#pragma unroll
    for (int r = 0; r < 4; ++r) z[r] = acc[r] + bv[r];
    if (!row_ok) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = n0 + 4 * ln.kq + r;
      if (n < A) {
        loc[m * A + n] = z[r];
      } else if (n < 2 * A) {
        if (spre) spre[m * A + (n - A)] = z[r];
        scale[m * A + (n - A)] = am_softplus(z[r]) + min_scale;
      }
    }
  }
};

// Dgrad: dZ = acc * act'(aux) to LDS and to memory; aux is the layer's saved
// H (ReLU, H > 0 as torch's threshold_backward) or Z (SiLU).
template <int ACT>
struct AmEpiDz {
  const float* __restrict__ aux;  // [S, N]
  float* __restrict__ dZ;         // [S, N]
  AmTile out;
  int N;
  long m;
  bool row_ok;
  DEV_INLINE f32x4 fetch(const AmLane& ln, int n0) const {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (row_ok)
      v = *reinterpret_cast<const f32x4*>(aux + m * N + n0 + 4 * ln.kq);
    return v;
  }
  DEV_INLINE void finish(const AmLane& ln, int n0, f32x4 acc, f32x4 ax) const {
    f32x4 dz;
#pragma unroll
    for (int r = 0; r < 4; ++r)
      dz[r] = ACT == AM_ACT_SILU ? acc[r] * silu_grad_f(ax[r])
                                 : (ax[r] > 0.f ? acc[r] : 0.f);
    const int n = n0 + 4 * ln.kq;
    *reinterpret_cast<f32x4*>(&out[ln.i][n]) = dz;
    if (row_ok) *reinterpret_cast<f32x4*>(dZ + m * N + n) = dz;
  }
};

DEV_INLINE AmLane am_lane() {
  const int tid = threadIdx.x;
  const AmLane ln = {tid, tid >> 6, tid & 15, (tid & 63) >> 4};
  return ln;
}

// ------------------------------------------------------------------ forward
// Grid ceil(S / 16). H.p[l] / Z.p[l] null: not stored.
template <int ACT>
__launch_bounds__(AM_THREADS) __global__ void actor_mlp_fwd_kernel(
    const float* __restrict__ X, ActorNet net, float min_scale,
    float* __restrict__ loc, float* __restrict__ scale,
    float* __restrict__ spre, ActorBufs Hs, ActorBufs Zs, int vflags) {
  __shared__ alignas(16) float lds[2][AM_ROWS][AM_LD];
  const AmLane ln = am_lane();
  const int m0 = blockIdx.x * AM_ROWS;
  const long m = m0 + ln.i;
  const bool row_ok = m < net.S;
  const AmStage stage = {X, net.S, net.K0, m0, (vflags & AM_VEC_X) != 0};

  int p = 0;  // the buffer that holds the layer's input
  int K = net.K0;
  for (int l = 0; l < net.L; ++l) {
    const int N = am_pick(net.N, l);
    const AmWRow wl = {am_pick(net.W, l), K, N, ((vflags >> l) & 1) != 0};
    const AmEpiHidden<ACT> epi = {am_pick(net.b, l), am_pick(Hs.p, l),
                                  am_pick(Zs.p, l),  lds[p ^ 1],
                                  N,                 m,
                                  row_ok};
    am_zero_pad(lds[p ^ 1], N, ln);
    if (l == 0)
      am_layer_staged(lds[0], wl, N >> 4, K, stage, epi, ln);
    else
      am_layer(lds[p], wl, N >> 4, K, epi, ln);
    __syncthreads();
    p ^= 1;
    K = N;
  }
  const AmWHeadRow wl = {net.Wloc, net.Wscale, K, net.A,
                         (vflags & AM_VEC_HEAD) != 0};
  const AmEpiHead epi = {net.bloc, net.bscale, loc, scale, spre,
                         net.A,    min_scale,  m,   row_ok};
  am_layer(lds[p], wl, (2 * net.A + 15) >> 4, K, epi, ln);
}

// -------------------------------------------------------------------- dgrad
// Grid ceil(S / 16). Stores dZ.p[l] [S, N_l] for every hidden layer and the
// head's dZh [2, S, A] = (dloc, dspre).
template <int ACT>
__launch_bounds__(AM_THREADS) __global__ void actor_mlp_dgrad_kernel(
    const float* __restrict__ dloc, const float* __restrict__ dscale,
    const float* __restrict__ spre, ActorNet net, ActorBufs aux, ActorBufs dZ,
    float* __restrict__ dZh) {
  __shared__ alignas(16) float lds[2][AM_ROWS][AM_LD];
  const AmLane ln = am_lane();
  const int m0 = blockIdx.x * AM_ROWS;
  const long m = m0 + ln.i;
  const int S = net.S, A = net.A, L = net.L;
  const bool row_ok = m < S;

  // [dloc | dspre] of the tile, zeros up to the next multiple of 64 columns
  const int W64 = (2 * A + 63) & ~63;  // at most 128
  for (int idx = ln.tid; idx < AM_ROWS * W64; idx += AM_THREADS) {
    const int r = idx / W64;
    const int c = idx - r * W64;
    const long mm = m0 + r;
    float v = 0.f;
    if (mm < S && c < 2 * A) {
      if (c < A) {
        v = dloc[mm * A + c];
        dZh[mm * A + c] = v;
      } else {
        const long at = mm * A + (c - A);
        v = dscale[at] * am_softplus_grad(spre[at]);
        dZh[(long)S * A + at] = v;
      }
    }
    lds[0][r][c] = v;
  }
  __syncthreads();

  int p = 0;
  {
    const int N = am_pick(net.N, L - 1);
    const AmWHeadCol wl = {net.Wloc, net.Wscale, N, A};
    const AmEpiDz<ACT> epi = {am_pick(aux.p, L - 1), am_pick(dZ.p, L - 1),
                              lds[1], N, m, row_ok};
    am_zero_pad(lds[1], N, ln);
    am_layer(lds[0], wl, N >> 4, 2 * A, epi, ln);
    __syncthreads();
    p = 1;
  }
  for (int l = L - 1; l >= 1; --l) {  // dZ_l -> dZ_{l-1} through W_l
    const int Nin = am_pick(net.N, l), N = am_pick(net.N, l - 1);
    const AmWCol wl = {am_pick(net.W, l), N, Nin};
    const AmEpiDz<ACT> epi = {am_pick(aux.p, l - 1), am_pick(dZ.p, l - 1),
                              lds[p ^ 1], N, m, row_ok};
    am_zero_pad(lds[p ^ 1], N, ln);
    am_layer(lds[p], wl, N >> 4, Nin, epi, ln);
    __syncthreads();
    p ^= 1;
  }
}

// ----------------------------------------------------------- host launchers

static bool am_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static bool am_net_ok(const ActorNet& net, int act) {
  if (net.L < 1 || net.L > ACTOR_MAX_L || net.K0 < 1 || net.A < 1 ||
      net.A > 64 || net.S < 1 || net.S > (1 << 30) ||
      (act != AM_ACT_SILU && act != AM_ACT_RELU))
    return false;
  for (int l = 0; l < net.L; ++l)
    if (net.N[l] < 16 || net.N[l] > AM_KC || (net.N[l] & 15) != 0 ||
        !net.W[l] || !net.b[l])
      return false;
  return net.Wloc && net.bloc && net.Wscale && net.bscale;
}

extern "C" int launch_actor_mlp_fwd(const float* X, const ActorNet& net,
                                    float min_scale, int act, float* loc,
                                    float* scale, float* spre,
                                    const ActorBufs& H, const ActorBufs& Z,
                                    void* stream) {
  if (!am_net_ok(net, act) || !X || !loc || !scale) return 1;
  int vflags = 0;
  for (int l = 0; l < net.L; ++l) {
    const int K = l == 0 ? net.K0 : net.N[l - 1];
    if ((K & 3) == 0 && am_al16(net.W[l])) vflags |= 1 << l;
    // the 16-byte stores of the saved activations
    if (!am_al16(H.p[l]) || !am_al16(Z.p[l])) return 1;
  }
  if (am_al16(net.Wloc) && am_al16(net.Wscale)) vflags |= AM_VEC_HEAD;
  if ((net.K0 & 3) == 0 && am_al16(X)) vflags |= AM_VEC_X;
  dim3 grid((net.S + AM_ROWS - 1) / AM_ROWS), block(AM_THREADS);
  auto kernel = act == AM_ACT_SILU ? actor_mlp_fwd_kernel<AM_ACT_SILU>
                                   : actor_mlp_fwd_kernel<AM_ACT_RELU>;
  hipLaunchKernelGGL(kernel, grid, block, 0, (hipStream_t)stream, X, net,
                     min_scale, loc, scale, spre, H, Z, vflags);
  return 0;
}

extern "C" int launch_actor_mlp_dgrad(const float* dloc, const float* dscale,
                                      const float* spre, const ActorNet& net,
                                      int act, const ActorBufs& aux,
                                      const ActorBufs& dZ, float* dZh,
                                      void* stream) {
  if (!am_net_ok(net, act) || !dloc || !dscale || !spre || !dZh) return 1;
  for (int l = 0; l < net.L; ++l)
    if (!aux.p[l] || !dZ.p[l] || !am_al16(aux.p[l]) || !am_al16(dZ.p[l]))
      return 1;
  dim3 grid((net.S + AM_ROWS - 1) / AM_ROWS), block(AM_THREADS);
  auto kernel = act == AM_ACT_SILU ? actor_mlp_dgrad_kernel<AM_ACT_SILU>
                                   : actor_mlp_dgrad_kernel<AM_ACT_RELU>;
  hipLaunchKernelGGL(kernel, grid, block, 0, (hipStream_t)stream, dloc, dscale,
                     spre, net, aux, dZ, dZh);
  return 0;
}
