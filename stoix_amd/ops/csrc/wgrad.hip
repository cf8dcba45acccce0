// Split-K weight-gradient kernels (the K6/K7 backward of SURVEY.md §2.9).
//
// dW[N,K] = dZ^T[N,S] @ X[S,K]  and  db[N] = colsum(dZ),  S = minibatch
// (32768 for the flagship config). hipBLASLt's best NT kernel for this
// K-huge/MN-tiny shape runs at ~56 TFLOP/s (tunableop_gfx950.csv:
// nt_256_256_32768 = 77 us); these kernels split S over 16 wave-slices,
// each wave MFMA-accumulating its slice into a private fp32 slab, and one
// slab_reduce kernel sums the 16 slabs straight into the flat bf16 grad
// buffer (zeroing the slab for the next minibatch in the same pass). The
// bias column-sum rides along for free from the A-operand fragments.
//
// Geometry per wgrad launch: grid (N/16) x (K/(16*KPG)) x 4, block 256
// (4 waves). wave-slice = blockIdx.z*4 + wid in [0,16); each wave stages
// 32-deep s-tiles of dZ and X into LDS *transposed* (scatter b16 writes,
// contiguous ds_read_b128 fragment reads) and issues KPG
// mfma_f32_16x16x32_bf16 per s-step.
//
// wgrad_pair_kernel / slab_reduce_pair_kernel (further down) are what the
// PPO engine runs by default: the same sums, both nets per launch, tiles
// staged row-major and read transposed, loads pipelined behind the MFMAs.
#include "common.h"
#include "launchers.h"
#include <cstdlib>
#include <hip/hip_bf16.h>

typedef __bf16 bf16_t;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define MFMA_BF16_16x16x32 __builtin_amdgcn_mfma_f32_16x16x32_bf16

#define WG_SLICES 64  // max wave-slices; the launcher picks the
// largest power of two <= 64 that divides S/32 (small minibatches use fewer)
#define SPAD 8        // +8 cols on the 32-wide transposed tiles

// One wave's private staging: dZt [NTB*16 n][32+8 s], Xt [KPG*16 k][32+8 s].
// NTB n-tiles per workgroup cut the X read-amplification (every n-tile
// group re-reads the whole X k-slice; at NTB=1 a 256x256 wgrad re-reads
// the 16 MB X sixteen times = 256 MB -> the kernel is HBM/L2-traffic
// bound). NTB=4, KPG=8: per-wave 4*16*40*2 + 8*16*40*2 = 15.3 KB; x4
// waves = 61 KB.
struct WgradLds {
  bf16_t dZt[4][4 * 16][32 + SPAD];
  bf16_t Xt[4][8 * 16][32 + SPAD];
};

template <int KPG, int NTB>
__launch_bounds__(256, 2) __global__ void wgrad_kernel(
    const bf16_t* __restrict__ dZ,  // [S, N_STRIDE]
    const bf16_t* __restrict__ X,   // [S, K]
    float* __restrict__ slab,       // [WG_SLICES, slab_stride] fp32
    long dW_off,                    // element offset of dW[N,K] in a slab
    long db_off,                    // element offset of db[N] (or -1)
    long slab_stride, int S, int N_STRIDE, int K, int N_VALID,
    int n_slices) {
  __shared__ WgradLds lds;
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int nt = blockIdx.x * NTB;   // NTB 16-row n-tiles per workgroup
  const int k0 = blockIdx.y * KPG * 16;
  const int slice = blockIdx.z * 4 + wid;  // [0, n_slices)
  const int s_per = S / n_slices;
  const int s_begin = slice * s_per;
  const int s_end = s_begin + s_per;
  const int n0 = nt * 16;

  bf16_t(*dZt)[32 + SPAD] = lds.dZt[wid];
  bf16_t(*Xt)[32 + SPAD] = lds.Xt[wid];

  f32x4 acc[NTB][KPG];
#pragma unroll
  for (int u = 0; u < NTB; ++u)
#pragma unroll
    for (int t = 0; t < KPG; ++t) acc[u][t] = {0.f, 0.f, 0.f, 0.f};
  float db_acc[NTB];
#pragma unroll
  for (int u = 0; u < NTB; ++u) db_acc[u] = 0.0f;

  const int arow = lane & 15;
  const int ak0 = (lane >> 4) * 8;

  for (int s0 = s_begin; s0 < s_end; s0 += 32) {
    // ---- stage dZ tiles [32 s][NTB*16 n] -> dZt [NTB*16 n][32 s]
#pragma unroll
    for (int u = 0; u < NTB; ++u) {
      int srow = lane >> 1, nh = (lane & 1) * 8;
      bf16x8 v = *reinterpret_cast<const bf16x8*>(
          dZ + (long)(s0 + srow) * N_STRIDE + n0 + u * 16 + nh);
#pragma unroll
      for (int i = 0; i < 8; ++i) dZt[u * 16 + nh + i][srow] = v[i];
    }
    // ---- stage X tiles [32 s][KPG*16 k] -> Xt [KPG*16 k][32 s].
    // Lane mapping: consecutive lanes take consecutive s-rows of ONE
    // k-chunk, so the 8 transposed b16 scatter-writes per lane hit
    // consecutive banks (srow-consecutive) instead of a 16-way conflict
    // (kh-strided, 160 dwords = bank 0 for every lane). The global loads
    // become 16B row-strided, but successive q iterations re-touch the
    // same 32 rows' cache lines, so L1 serves 7/8 of them.
#pragma unroll
    for (int q = 0; q < KPG; ++q) {
      int flat = q * 64 + lane;
      int srow = flat & 31;
      int kh = (flat >> 5) * 8;
      bf16x8 v = *reinterpret_cast<const bf16x8*>(
          X + (long)(s0 + srow) * K + k0 + kh);
#pragma unroll
      for (int i = 0; i < 8; ++i) Xt[kh + i][srow] = v[i];
    }
    // within-wave LDS write->read ordering is compiler-tracked (lgkmcnt);
    // no cross-wave sharing, so no barrier.
    // ---- fragments + MFMA (B fragments shared by the NTB A tiles)
#pragma unroll
    for (int t = 0; t < KPG; ++t) {
      const bf16x8 b =
          *reinterpret_cast<const bf16x8*>(&Xt[t * 16 + arow][ak0]);
#pragma unroll
      for (int u = 0; u < NTB; ++u) {
        const bf16x8 a =
            *reinterpret_cast<const bf16x8*>(&dZt[u * 16 + arow][ak0]);
        acc[u][t] = MFMA_BF16_16x16x32(a, b, acc[u][t], 0, 0, 0);
      }
    }
    // ---- bias partials from the A fragments (kt-group-0 blocks only)
    if (db_off >= 0 && blockIdx.y == 0) {
#pragma unroll
      for (int u = 0; u < NTB; ++u) {
        const bf16x8 a =
            *reinterpret_cast<const bf16x8*>(&dZt[u * 16 + arow][ak0]);
#pragma unroll
        for (int j = 0; j < 8; ++j) db_acc[u] += (float)a[j];
      }
    }
  }

  // ---- write this wave's slab slice
  float* out = slab + (long)slice * slab_stride;
  const int col = lane & 15;  // k within tile
  const int g = lane >> 4;
#pragma unroll
  for (int u = 0; u < NTB; ++u) {
#pragma unroll
    for (int t = 0; t < KPG; ++t) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int n = u * 16 + g * 4 + r;  // D row = n (A is dZ^T)
        if (n0 + n < N_VALID)
          out[dW_off + (long)(n0 + n) * K + k0 + t * 16 + col] = acc[u][t][r];
      }
    }
    if (db_off >= 0 && blockIdx.y == 0) {
      float d = db_acc[u];
      d += __shfl_xor(d, 16);
      d += __shfl_xor(d, 32);
      if ((lane >> 4) == 0 && n0 + u * 16 + arow < N_VALID)
        out[db_off + n0 + u * 16 + arow] = d;
    }
  }
}

// Sum the WG_SLICES slabs into the flat bf16 grad buffer and zero them for
// the next minibatch. One launch covers a whole chain's gradient.
extern "C" __global__ void slab_reduce_kernel(float* __restrict__ slab,
                                              __bf16* __restrict__ grad16,
                                              long slab_stride, long n,
                                              float* __restrict__ sqnorm,
                                              long* __restrict__ step_t) {
  // fused Adam prologue rides along: this kernel always runs right before
  // the chain's Adam
  if (sqnorm) adam_prologue(sqnorm, step_t);
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  // The same ascending sum as slab_sum() below, kept as its own interleaved
  // load/add/zero loop on purpose: this is the knob-off reference, and its
  // memory pattern is part of what the A/B against the paired kernels
  // compares.
  for (; i < n; i += stride) {
    float s = 0.0f;
#pragma unroll
    for (int z = 0; z < WG_SLICES; ++z) {
      s += slab[(long)z * slab_stride + i];
      slab[(long)z * slab_stride + i] = 0.0f;
    }
    grad16[i] = (__bf16)s;
  }
}

// ------------------------------------------------- pipelined, paired wgrad
// Same result as wgrad_kernel, bit for bit (same slices, one accumulator
// chain per 16x16 tile, one MFMA per 32-row step in ascending row order,
// row s0+8g+j in k-slot (g, j); same db sum), but:
//  * both nets in one launch (blockIdx.z picks the net),
//  * one workgroup = one slice x (WN*NTW*16) n x (WK*KTW*16) k, the four
//    waves laid out WN x WK over the tile, all staging cooperative,
//  * s-tiles are stored ROW-major in LDS with 16-byte writes and the MFMA
//    operands come out of ds_read_b64_tr_b16 already transposed (two reads
//    per fragment: block rows 8g..8g+3 and 8g+4..8g+7),
//  * register prefetch + LDS double buffer: the global loads of stage i+1
//    (SB 32-row steps) are in flight while stage i's MFMAs run; one barrier
//    per stage.
//
// LDS image of a [R rows][C cols] tile: byte offset of (row, col) =
// row*P + (row>>3)*128 + col*2 with P = the row bytes padded up to
// 32 (mod 64). A 32-lane half of a transposed read takes rows r..r+3 and
// r+8..r+11 of one 32-byte column group: with P = 32*odd the first four
// rows land on four distinct 8-bank groups whose indices differ by
// o, 2o, 3o (mod 8, o odd), never by 4, and the 128-byte step per 8 rows
// moves the other four by 32 banks = 4 groups, so the eight 32-byte
// segments tile the 64 banks: conflict-free by the (a/4)%64 bank rule.
//
// A net's operands arrive as a WgradNet (launchers.h).

typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;

__host__ __device__ constexpr int wp_pitch(int row_bytes) {
  return ((row_bytes + 31) / 64) * 64 + 32;
}

__device__ __forceinline__ bf16x8 wp_tr_frag(const unsigned char* p,
                                             int pitch) {
  bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)p);
  bf16x4 hi =
      __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(p + 4 * pitch));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

template <int NTW, int KTW, int WN, int WK, int SB>
__launch_bounds__(256) __global__ void wgrad_pair_kernel(
    WgradNet net0, WgradNet net1, int S, int N_STRIDE, int K, int n_slices,
    int kblocks, int slice_major) {
  static_assert(WN * WK == 4, "four waves");
  constexpr int TN = WN * NTW * 16, TK = WK * KTW * 16;
  constexpr int CZ = TN / 8, CX = TK / 8;  // 16-byte chunks per tile row
  constexpr int PZ = wp_pitch(TN * 2), PX = wp_pitch(TK * 2);
  constexpr int ROWS = 32 * SB;
  constexpr int ZSTEP = 32 * PZ + 4 * 128, XSTEP = 32 * PX + 4 * 128;
  constexpr int ZB = SB * ZSTEP, XB = SB * XSTEP;
  constexpr int NZ = ROWS * CZ, NX = ROWS * CX;
  constexpr int LZ = (NZ + 255) / 256, LX = (NX + 255) / 256;
  static_assert(2 * (ZB + XB) <= 160 * 1024, "gfx950 LDS");
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * (ZB + XB)];

  const bool second = blockIdx.z != 0;
  const bf16_t* __restrict__ dZ = (const bf16_t*)(second ? net1.dZ : net0.dZ);
  const bf16_t* __restrict__ X = (const bf16_t*)(second ? net1.X : net0.X);
  float* __restrict__ slab = second ? net1.slab : net0.slab;
  const long dW_off = second ? net1.dW_off : net0.dW_off;
  const long db_off = second ? net1.db_off : net0.db_off;
  const long slab_stride = second ? net1.slab_stride : net0.slab_stride;
  const int N_VALID = second ? net1.N_VALID : net0.N_VALID;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  // wave id as a scalar, so the per-wave branches are scalar branches
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wn = wid / WK, wk = wid % WK;
  // slice_major: the slice runs along blockIdx.x, so the workgroups that
  // share one slice's dZ / X rows have linear ids a multiple of 8 apart and
  // land on the same XCD (one L2)
  const int tile = slice_major ? blockIdx.y : blockIdx.x;
  const int n0 = (tile / kblocks) * TN;
  const int kblk = tile % kblocks;
  const int k0 = kblk * TK;
  const int slice = slice_major ? blockIdx.x : blockIdx.y;  // [0, n_slices)
  const int s_per = S / n_slices;
  const int s_begin = slice * s_per;
  const int s_end = s_begin + s_per;
  const int steps = s_per / 32;
  const int nstages = (steps + SB - 1) / SB;
  const bool do_db = db_off >= 0 && kblk == 0;  // workgroup-uniform

  f32x4 acc[NTW][KTW];
#pragma unroll
  for (int u = 0; u < NTW; ++u)
#pragma unroll
    for (int t = 0; t < KTW; ++t) acc[u][t] = {0.f, 0.f, 0.f, 0.f};
  float db_acc[NTW];
#pragma unroll
  for (int u = 0; u < NTW; ++u) db_acc[u] = 0.0f;

  // transposed-read lane address: lane 4q+p of 16-lane group g supplies
  // row 8g+q, columns 4p..4p+3 of the block; it receives column (lane&15)
  const int g = lane >> 4;
  const int q = (lane >> 2) & 3, p = lane & 3;
  const int zl = (8 * g + q) * PZ + g * 128 + (wn * NTW * 16 + 4 * p) * 2;
  const int xl = (8 * g + q) * PX + g * 128 + (wk * KTW * 16 + 4 * p) * 2;

  bf16x8 rz[LZ], rx[LX];  // register prefetch of one stage

  auto gload = [&](int st) {
    const int r0 = s_begin + st * ROWS;
#pragma unroll
    for (int i = 0; i < LZ; ++i) {
      const int c = tid + i * 256;
      if (NZ % 256 == 0 || c < NZ) {
        // rows past the slice end (a partial last stage) are clamped to
        // its last row: in bounds, staged, never consumed
        int gr = r0 + c / CZ;
        gr = gr < s_end ? gr : s_end - 1;
        rz[i] = *reinterpret_cast<const bf16x8*>(
            dZ + (long)gr * N_STRIDE + n0 + (c % CZ) * 8);
      }
    }
#pragma unroll
    for (int i = 0; i < LX; ++i) {
      const int c = tid + i * 256;
      if (NX % 256 == 0 || c < NX) {
        int gr = r0 + c / CX;
        gr = gr < s_end ? gr : s_end - 1;
        rx[i] = *reinterpret_cast<const bf16x8*>(
            X + (long)gr * K + k0 + (c % CX) * 8);
      }
    }
  };
  auto lwrite = [&](int buf) {
    unsigned char* zb = lds + buf * (ZB + XB);
    unsigned char* xb = zb + ZB;
#pragma unroll
    for (int i = 0; i < LZ; ++i) {
      const int c = tid + i * 256;
      if (NZ % 256 == 0 || c < NZ) {
        const int row = c / CZ;
        *reinterpret_cast<bf16x8*>(zb + row * PZ + (row >> 3) * 128 +
                                   (c % CZ) * 16) = rz[i];
      }
    }
#pragma unroll
    for (int i = 0; i < LX; ++i) {
      const int c = tid + i * 256;
      if (NX % 256 == 0 || c < NX) {
        const int row = c / CX;
        *reinterpret_cast<bf16x8*>(xb + row * PX + (row >> 3) * 128 +
                                   (c % CX) * 16) = rx[i];
      }
    }
  };

  gload(0);
  lwrite(0);
  __syncthreads();
  for (int st = 0; st < nstages; ++st) {
    const bool more = st + 1 < nstages;
    if (more) gload(st + 1);
    const unsigned char* zb = lds + (st & 1) * (ZB + XB);
    const unsigned char* xb = zb + ZB;
    const int nst = steps - st * SB;  // valid steps in this stage (>= 1)
    // every branch below is workgroup- or wave-uniform: the transposed
    // reads always run with EXEC all ones
#pragma unroll
    for (int sb = 0; sb < SB; ++sb) {
      if (sb < nst) {
        bf16x8 a[NTW];
#pragma unroll
        for (int u = 0; u < NTW; ++u)
          a[u] = wp_tr_frag(zb + zl + sb * ZSTEP + u * 32, PZ);
#pragma unroll
        for (int t = 0; t < KTW; ++t) {
          const bf16x8 b = wp_tr_frag(xb + xl + sb * XSTEP + t * 32, PX);
#pragma unroll
          for (int u = 0; u < NTW; ++u)
            acc[u][t] = MFMA_BF16_16x16x32(a[u], b, acc[u][t], 0, 0, 0);
        }
        // bias partials; the WK waves that share an n-range split its tiles
        if (do_db) {
#pragma unroll
          for (int u = 0; u < NTW; ++u) {
            if (u % WK == wk) {
#pragma unroll
              for (int j = 0; j < 8; ++j) db_acc[u] += (float)a[u][j];
            }
          }
        }
      }
    }
    if (more) lwrite((st + 1) & 1);
    __syncthreads();
  }

  // ---- write this workgroup's part of slab image `slice`
  float* out = slab + (long)slice * slab_stride;
  const int col = lane & 15;
#pragma unroll
  for (int u = 0; u < NTW; ++u) {
    const int nb = n0 + (wn * NTW + u) * 16;
#pragma unroll
    for (int t = 0; t < KTW; ++t) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = nb + g * 4 + r;  // D row = n (A is dZ^T)
        if (n < N_VALID)
          out[dW_off + (long)n * K + k0 + (wk * KTW + t) * 16 + col] =
              acc[u][t][r];
      }
    }
    if (do_db && u % WK == wk) {
      float d = db_acc[u];
      d += __shfl_xor(d, 16);
      d += __shfl_xor(d, 32);
      if (g == 0 && nb + col < N_VALID) out[db_off + nb + col] = d;
    }
  }
}

// Element i of a chain's gradient: the ascending sum over the WG_SLICES
// slab images, in slab_reduce_kernel's order. Every paired reduce takes its
// sums from here.
DEV_INLINE float slab_sum(const float* __restrict__ slab, long slab_stride,
                          long i) {
  // all 64 loads go out before the first add (the compiler left two in
  // flight when load and add shared one loop); the adds keep their order
  float v[WG_SLICES];
#pragma unroll
  for (int z = 0; z < WG_SLICES; ++z) v[z] = slab[(long)z * slab_stride + i];
  float s = 0.0f;
#pragma unroll
  for (int z = 0; z < WG_SLICES; ++z) s += v[z];
  return s;
}

// Both chains' slabs -> their flat bf16 grads in one launch (blockIdx.y
// picks the chain), slab_sum() and the fused Adam prologue of
// slab_reduce_kernel (adam_prologue(), common.h), but NO stores to the slab.
// That is safe wherever the slab is only ever filled by the wgrad kernels
// with a fixed set of (offset, shape) calls, as in the PPO engine: they
// store (never accumulate), so every valid element of the used images is
// overwritten by the next minibatch's wgrads before it is read again, and
// unused images and padding rows are never written, so they keep the zeros
// the slab was allocated with.
extern "C" __launch_bounds__(256) __global__ void slab_reduce_pair_kernel(
    const float* __restrict__ slab0, __bf16* __restrict__ grad0, long stride0,
    long n0, float* __restrict__ sqnorm0, long* __restrict__ step0,
    const float* __restrict__ slab1, __bf16* __restrict__ grad1, long stride1,
    long n1, float* __restrict__ sqnorm1, long* __restrict__ step1) {
  const bool second = blockIdx.y != 0;
  const float* __restrict__ slab = second ? slab1 : slab0;
  __bf16* __restrict__ grad16 = second ? grad1 : grad0;
  const long slab_stride = second ? stride1 : stride0;
  const long n = second ? n1 : n0;
  float* sqnorm = second ? sqnorm1 : sqnorm0;
  long* step_t = second ? step1 : step0;
  if (sqnorm) adam_prologue(sqnorm, step_t);
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < n; i += stride)
    grad16[i] = (__bf16)slab_sum(slab, slab_stride, i);
}

// slab_reduce_pair_kernel plus the squared gradient norm of each chain, so
// that the optimiser tail is this launch and adam_pair (optim.hip). It
// leaves in sqnorm[0] the very float that grad_sqnorm_bf16_kernel (ordered
// partials) and adam_update_bf16_kernel's sum of them produce, which fixes
// the order of the float adds:
//   * per group of 8 consecutive elements, acc = 0; acc += x_j * x_j in
//     ascending j (x = the bf16 gradient as float);
//   * the n % 8 tail elements go to the accumulators of groups 0..n%8-1,
//     after the group's own sum;
//   * 64 consecutive groups through the __shfl_down tree (one wave of the
//     norm kernel = one 512-element block here);
//   * four consecutive tree sums added in order from 0 (one 2048-element
//     block of the norm kernel);
//   * those sums lane-strided by 64 from 0, then the same tree.
// One element per thread as in slab_reduce_pair_kernel (the 64-image sum is
// where the traffic is), 512 threads so that a block holds one whole tree:
// wave 0 forms the 64 group sums from the block's bf16 results (LDS) and
// stores the tree sum at sqnorm[1 + block], write-through. Thread 0 then
// bumps the chain's integer counter; the block that draws the last ticket adds
// the tree sums up in the fixed order, stores sqnorm[0] and resets the
// counter for the next launch. No block waits for another, and no float
// atomic enters the sum. Block 0 recomputes the (at most 7) tail elements
// from the slab, the same ascending sum, so it needs nothing from the
// block that owns them. The trees are wave_sum_down() (common.h), the one
// adam_update_bf16_kernel sums the norm kernel's partials with. A chain's
// operands arrive as a TailChain (launchers.h).
extern "C" __launch_bounds__(512) __global__
    void slab_reduce_norm_pair_kernel(TailChain c0, TailChain c1) {
  const TailChain c = blockIdx.y ? c1 : c0;
  const long n = c.n;
  const int nblk = (int)((n + 511) / 512);
  if ((int)blockIdx.x >= nblk) return;  // the shorter chain's spare blocks
  if (blockIdx.x == 0 && threadIdx.x == 0) *c.step_t += 1;
  __shared__ float x[512];
  __shared__ int is_last;
  const long i = (long)blockIdx.x * 512 + threadIdx.x;
  float xv = 0.0f;
  if (i < n) {
    const __bf16 q = (__bf16)slab_sum(c.slab, c.slab_stride, i);
    ((__bf16*)c.grad16)[i] = q;
    xv = (float)q;
  }
  x[threadIdx.x] = xv;
  __syncthreads();
  const long nvec = n / 8;
  if (threadIdx.x < 64) {
    float acc = 0.0f;
    if ((long)blockIdx.x * 64 + threadIdx.x < nvec) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float v = x[threadIdx.x * 8 + j];
        acc += v * v;
      }
    }
    if (blockIdx.x == 0 && (long)threadIdx.x < n - nvec * 8) {
      float v = (float)(__bf16)slab_sum(c.slab, c.slab_stride,
                                        nvec * 8 + threadIdx.x);
      acc += v * v;
    }
    acc = wave_sum_down(acc);
    if (threadIdx.x == 0) {
      // publish the one float write-through and wait for it, then take a
      // ticket. A release fence here would write the whole L2 back, the
      // block's share of grad16 included, once per block (measured: 22 us
      // for the launch against 9 us for the plain reduce).
      __hip_atomic_store(c.sqnorm + 1 + blockIdx.x, acc, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      is_last = __hip_atomic_fetch_add(c.counter, 1u, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT) ==
                (unsigned int)(nblk - 1);
    }
  }
  __syncthreads();
  if (!is_last || threadIdx.x >= 64) return;
  // every block sum was acknowledged before its ticket; read them past
  // this CU's cache (agent-scope loads)
  // the norm kernel's blocks: 256 groups each, at least one
  const long nb = nvec > 256 ? (nvec + 255) / 256 : 1;
  float acc = 0.0f;
  for (long p = threadIdx.x; p < nb; p += 64) {
    float s = 0.0f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const long b = 4 * p + w;
      // a tree the norm kernel would run over no data is a zero
      s += b < nblk ? __hip_atomic_load(c.sqnorm + 1 + b, __ATOMIC_RELAXED,
                                        __HIP_MEMORY_SCOPE_AGENT)
                    : 0.0f;
    }
    acc += s;
  }
  // wave_sum_down() spelled out: through the helper the compiler schedules
  // this kernel differently, and its code is kept as it was
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
  if (threadIdx.x == 0) {
    c.sqnorm[0] = acc;
    __hip_atomic_store(c.counter, 0u, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  }
}

// n0, n1 >= 1; each sqnorm holds 1 + ceil(n / 512) floats (bind.cpp checks)
extern "C" void launch_slab_reduce_norm_pair(const TailChain& c0,
                                             const TailChain& c1,
                                             void* stream) {
  long nmax = c0.n > c1.n ? c0.n : c1.n;
  int blocks = (int)((nmax + 511) / 512);
  hipLaunchKernelGGL(slab_reduce_norm_pair_kernel, dim3(blocks, 2), dim3(512),
                     0, (hipStream_t)stream, c0, c1);
}

// ------------------------------------------------------------- tr probe
// Empirically maps __builtin_amdgcn_ds_read_tr16_b64_v4bf16: stages 1024
// known bf16 values linearly in LDS, issues the tr read with per-lane base
// = base_mode ? lane-pattern : uniform, dumps each lane's 4 elements.
extern "C" __global__ void tr16_probe_kernel(const bf16_t* __restrict__ in,
                                             float* __restrict__ out,
                                             int base_mode) {
  __shared__ bf16_t l[1024];
  int t = threadIdx.x;
  for (int i = t; i < 1024; i += 64) l[i] = in[i];
  __syncthreads();
  if (t >= 64) return;
  int off = 0;
  if (base_mode == 1) off = (t >> 4) * 64;       // group-strided base
  else if (base_mode == 2) off = (t >> 4) * 128; // doubled group stride
  bf16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
      (__attribute__((address_space(3))) bf16x4*)&l[off]);
#pragma unroll
  for (int j = 0; j < 4; ++j) out[t * 4 + j] = (float)v[j];
}

// --------------------------------------------------------- host launchers

// Wave-slices S is split over: WG_SLICES, or STOIX_WGRAD_SLICES in
// [4, WG_SLICES], halved until the slices divide S into whole 32-row steps
// (down to 4).
static int pick_slices(int S) {
  int n_slices = WG_SLICES;
  if (const char* e = getenv("STOIX_WGRAD_SLICES")) {
    int v = atoi(e);
    if (v >= 4 && v <= WG_SLICES) n_slices = v;
  }
  while (n_slices > 4 && (S % (n_slices * 32)) != 0) n_slices >>= 1;
  return n_slices;
}

extern "C" void launch_wgrad(const void* dZ, const void* X, float* slab,
                             long dW_off, long db_off, long slab_stride,
                             int S, int N_STRIDE, int K, int N_VALID,
                             int kpg_override, int ntb_override,
                             void* stream) {
  hipStream_t s = (hipStream_t)stream;
  int NT = (N_VALID + 15) / 16;
  // NTB n-tiles per workgroup (X-amplification = NT/NTB); KPG picked per
  // shape so the grid spans the whole 256-CU chip (swept on MI355X,
  // tools/wgrad_sweep.py): fill beats per-WG tile depth at these shapes.
  int NTB = (NT % 4 == 0) ? 4 : 1;
  int KPG = 1;
  if (ntb_override > 0) NTB = ntb_override;
  if (kpg_override > 0) {
    KPG = kpg_override;
  } else if (NT <= 1) {
    // head grads (N<=16): swept best is KPG=4 x 16 slices = 64 WGs
    // (per-WG k-depth beats chip fill at this tiny N)
    KPG = (K % 64 == 0) ? 4 : ((K % 32 == 0) ? 2 : 1);
  } else if (K % 64 == 0 && (NT / NTB) * (K / 64) >= 16) {
    // big-K layer grads: KPG=4 puts exactly 256 WGs on the 256 CUs
    // (KPG=8 halves the grid; KPG<=2 doubles it past the fill point) --
    // 27.4 -> 20.6 us for the 256x256/S=32768 shape (tools/wgrad_sweep.py)
    KPG = 4;
  } else if (K % 32 == 0) {
    KPG = 2;
  }
  int KTG = K / (16 * KPG);
  int n_slices = pick_slices(S);
  dim3 grid(NT / NTB, KTG, n_slices / 4), block(256);
#define WGRAD_LAUNCH(KPGV, NTBV)                                            \
  hipLaunchKernelGGL((wgrad_kernel<KPGV, NTBV>), grid, block, 0, s,         \
                     (const bf16_t*)dZ, (const bf16_t*)X, slab, dW_off,     \
                     db_off, slab_stride, S, N_STRIDE, K, N_VALID, n_slices)
  if (NTB == 4) {
    if (KPG == 8) WGRAD_LAUNCH(8, 4);
    else if (KPG == 4) WGRAD_LAUNCH(4, 4);
    else if (KPG == 2) WGRAD_LAUNCH(2, 4);
    else WGRAD_LAUNCH(1, 4);
  } else {
    if (KPG == 8) WGRAD_LAUNCH(8, 1);
    else if (KPG == 4) WGRAD_LAUNCH(4, 1);
    else if (KPG == 2) WGRAD_LAUNCH(2, 1);
    else WGRAD_LAUNCH(1, 1);
  }
#undef WGRAD_LAUNCH
}

extern "C" void launch_slab_reduce(float* slab, void* grad16,
                                   long slab_stride, long n, float* sqnorm,
                                   long* step_t, void* stream) {
  int threads = 256;
  hipLaunchKernelGGL(slab_reduce_kernel, dim3(flat_blocks(n, threads)),
                     dim3(threads), 0,
                     (hipStream_t)stream, slab, (__bf16*)grad16, slab_stride,
                     n, sqnorm, step_t);
}

// Paired launch. Tiles per shape (tools/wgrad_sweep.py --pair):
//   heads  N_STRIDE=16, K in {128,256,512}: 16n x 128k, 2 steps a stage
//   K in {32,64,96}  (layer 1):             128n x K, waves split n
//   K = 128:                                128n x 128k, waves split k
//   K in {256,512}   (layer 2):             128n x 128k, waves split k,
//                                           slice-major grid
// variant >= 0 picks one of the alternatives the sweep compares. A shape
// outside this table goes to the old kernels, one launch per net, never to
// a neighbouring instantiation. Returns 1 if the paired kernel ran.
extern "C" int launch_wgrad_pair(const WgradNet& a, const WgradNet& b, int S,
                                 int N_STRIDE, int K, int variant,
                                 void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const int nv0 = a.N_VALID, nv1 = b.N_VALID;
  int n_slices = pick_slices(S);
  // variant < 0: the baked winners = variant 0, except layer 2 (K 256/512)
  // = variant 6. variants >= 4: the tiles of variant - 4 with the slice
  // along blockIdx.x (needs n_slices % 8 == 0 to line up with the 8 XCDs)
  if (variant < 0) variant = (K == 256 || K == 512) && N_STRIDE != 16 ? 6 : 0;
  const int slice_major = variant >= 4 && n_slices % 8 == 0;
  if (variant >= 4) variant -= 4;
#define WPAIR_LAUNCH(NTW, KTW, WN, WK, SB)                                   \
  do {                                                                       \
    constexpr int TN = WN * NTW * 16, TK = WK * KTW * 16;                    \
    int kblocks = K / TK;                                                    \
    int tiles = (N_STRIDE / TN) * kblocks;                                   \
    dim3 grid(slice_major ? n_slices : tiles, slice_major ? tiles : n_slices, \
              2), block(256);                                                \
    hipLaunchKernelGGL((wgrad_pair_kernel<NTW, KTW, WN, WK, SB>), grid,      \
                       block, 0, s, a, b, S, N_STRIDE, K, n_slices,          \
                       kblocks, slice_major);                                \
    return 1;                                                                \
  } while (0)
  const bool ok = (S % (n_slices * 32)) == 0 && n_slices % 4 == 0;
  const bool hid = N_STRIDE == 128 || N_STRIDE == 256 || N_STRIDE == 512;
  if (ok && N_STRIDE == 16 && nv0 >= 1 && nv0 <= 16 && nv1 >= 1 &&
      nv1 <= 16 && (K == 128 || K == 256 || K == 512)) {
    if (variant == 1) WPAIR_LAUNCH(1, 2, 1, 4, 1);
    if (variant == 2) WPAIR_LAUNCH(1, 1, 1, 4, 2);  // 16n x 64k
    if (variant == 3) WPAIR_LAUNCH(1, 2, 1, 4, 4);
    WPAIR_LAUNCH(1, 2, 1, 4, 2);
  }
  if (ok && hid && nv0 == N_STRIDE && nv1 == N_STRIDE) {
    if (K == 32) {
      if (variant == 1) WPAIR_LAUNCH(2, 2, 4, 1, 1);
      if (variant == 2) WPAIR_LAUNCH(1, 2, 4, 1, 2);  // 64n x 32k
      if (variant == 3) WPAIR_LAUNCH(2, 2, 4, 1, 4);
      WPAIR_LAUNCH(2, 2, 4, 1, 2);
    }
    if (K == 64) WPAIR_LAUNCH(2, 4, 4, 1, 2);
    if (K == 96) WPAIR_LAUNCH(2, 6, 4, 1, 1);
    if (K == 128) WPAIR_LAUNCH(8, 2, 1, 4, 1);
    if (K == 256 || K == 512) {
      if (variant == 1) WPAIR_LAUNCH(4, 4, 1, 4, 1);  // 64n x 256k
      if (variant == 2) WPAIR_LAUNCH(8, 2, 1, 4, 1);  // 128n x 128k
      if (variant == 3) WPAIR_LAUNCH(8, 4, 1, 4, 2);
      WPAIR_LAUNCH(8, 4, 1, 4, 1);
    }
  }
#undef WPAIR_LAUNCH
  for (const WgradNet* n : {&a, &b})
    launch_wgrad(n->dZ, n->X, n->slab, n->dW_off, n->db_off, n->slab_stride, S,
                 N_STRIDE, K, n->N_VALID, 0, 0, stream);
  return 0;
}

// c.counter is not used here
extern "C" void launch_slab_reduce_pair(const TailChain& c0,
                                        const TailChain& c1, void* stream) {
  int threads = 256;
  int blocks = flat_blocks(c0.n > c1.n ? c0.n : c1.n, threads);
  hipLaunchKernelGGL(slab_reduce_pair_kernel, dim3(blocks, 2), dim3(threads),
                     0, (hipStream_t)stream, c0.slab, (__bf16*)c0.grad16,
                     c0.slab_stride, c0.n, c0.sqnorm, c0.step_t, c1.slab,
                     (__bf16*)c1.grad16, c1.slab_stride, c1.n, c1.sqnorm,
                     c1.step_t);
}

extern "C" void launch_tr16_probe(const void* in, float* out, int base_mode,
                                  void* stream) {
  hipLaunchKernelGGL(tr16_probe_kernel, dim3(1), dim3(64), 0,
                     (hipStream_t)stream, (const bf16_t*)in, out, base_mode);
}
