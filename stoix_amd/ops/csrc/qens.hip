// Dense layers of a Q-ensemble (the twin critics of SAC / TD3 / DDPG, up to
// four members) in fp32 on v_mfma_f32_16x16x4_f32, every member in one launch:
//
//   forward  Z_e = [X0 | X1] W_e^T + b_e, H_e = act(Z_e)   qens_linear_fwd_kernel
//   dgrad    dX = dZ @ W[:, c0:c1), per member or summed    qens_linear_dgrad_kernel
//   wgrad    dW_e = dZ_e^T [X0 | X1], db_e = colsum(dZ_e)   qens_linear_wgrad_kernel
//            slabs -> the members' gradient tensors         qens_wgrad_reduce_kernel
//
// with dZ = dH * act'(.) formed in registers while the dH tile is staged (ReLU
// from the saved H, SiLU from the saved Z), so dZ never reaches memory, and
// the input [obs | action] concatenated while the X tile is staged, so no
// concatenated tensor exists either. W_e and b_e are the members' own
// nn.Linear parameters, read in place through a by-value struct of pointers.
//
// One scheme for the three GEMMs: 256 threads = 4 waves, 32-deep reduction
// steps, the operands of step i+1 loaded into registers before the MFMAs of
// step i and written to the other LDS buffer after them (one barrier per
// step), last step peeled so that the MFMA chain and the first read of its
// accumulator stay in straight-line code (docs/KERNELS.md).
//
// Operand layout of v_mfma_f32_16x16x4_f32: lane l gives A[i = l&15][k = l>>4]
// and B[k = l>>4][j = l&15], one float each, and gets D[(l>>4)*4 + r][l&15].
// A dot product may take its k in any order as long as both operands take
// the same one, so within a group of 16 reduction indices lane (i, kq) takes
// k = 4*kq + s at MFMA step s: its four values of the group are adjacent in
// an LDS row and come as ONE ds_read_b128 per operand, not four ds_read_b32.
// LDS rows are 36 floats (32 + 4): the 16 lanes of a b128 phase read rows
// i..i+15 at the same column, 36*i mod 64 = {0, 36, 8, 44, ...} are 16
// distinct multiples of 4, so the 16 x 4 dwords cover the 64 banks once.
//
// Each kernel puts the operand whose index is contiguous in the output on
// the A side, so a lane ends with 4 consecutive output elements of one row:
// one 16-byte store where the row length and the pointer allow, 4-byte
// stores otherwise. The same holds for loads: rows are only 4-byte aligned in
// general (K = 376 + 17), and a 16-byte load is used where the row length is
// a multiple of 4 and the base is aligned. Rows past S and columns past N / K
// are never read or written; reduction tails are zero-filled in LDS.
//
// No atomics, every sum in a fixed order, every output element written once.
#include "common.h"
#include "launchers.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define MFMA_F32_16x16x4 __builtin_amdgcn_mfma_f32_16x16x4f32

#define QE_THREADS 256
#define QE_BK 32
#define QE_LD (QE_BK + 4)  // padded LDS row, in floats
#define QE_ACT_NONE 0
#define QE_ACT_SILU 1
#define QE_ACT_RELU 2
#define QE_MAX_SPLIT 16
// which accesses may be 16 bytes wide
#define QE_VEC_X0 1
#define QE_VEC_X1 2
#define QE_VEC_W 4
#define QE_VEC_OUT 8
#define QE_VEC_DH 16

DEV_INLINE const float* qe_pick(const QensIn& s, int e) {
  return e == 0 ? s.p[0] : e == 1 ? s.p[1] : e == 2 ? s.p[2] : s.p[3];
}
DEV_INLINE float* qe_pick(const QensOut& s, int e) {
  return e == 0 ? s.p[0] : e == 1 ? s.p[1] : e == 2 ? s.p[2] : s.p[3];
}

DEV_INLINE float qe_act(float z, int act) {
  if (act == QE_ACT_SILU) return silu_f(z);
  if (act == QE_ACT_RELU) return z > 0.f ? z : 0.f;
  return z;
}

// Elements [col, col + 4) of the row that starts at p[row] and ends before
// column `ncols`; zero where the row or a column is out of range. `vec`: the
// row start and col are multiples of 4 floats from a 16-byte aligned base.
DEV_INLINE f32x4 qe_ld4(const float* __restrict__ p, long row, int col,
                        int ncols, bool ok, bool vec) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (!ok || col >= ncols) return v;
  if (vec && col + 3 < ncols)
    return *reinterpret_cast<const f32x4*>(p + row + col);
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (col + i < ncols) v[i] = p[row + col + i];
  return v;
}

// The input of a layer as two pieces: columns [0, K0) from x0 (one member's
// [S, K0]), columns [K0, K0 + K1) from x1 ([S, K1], may be absent).
struct QeCat {
  const float* x0;
  const float* x1;
  int K0, K1;
  bool vec0, vec1;
};

// Columns [k, k + 4) of row m of [x0 | x1], k a multiple of 4. A group that
// lies in one piece is one 16-byte load where that piece allows it; the
// group that holds the join, and everything in a piece with 4-byte aligned
// rows, is read by element.
DEV_INLINE f32x4 qe_ldcat(const QeCat& c, long m, int k, bool ok) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (!ok) return v;
  if (k + 3 < c.K0) {
    if (c.vec0) return *reinterpret_cast<const f32x4*>(c.x0 + m * c.K0 + k);
  } else if (k >= c.K0 && c.vec1 && k - c.K0 + 3 < c.K1) {
    return *reinterpret_cast<const f32x4*>(c.x1 + m * c.K1 + (k - c.K0));
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int kk = k + i;
    if (kk < c.K0)
      v[i] = c.x0[m * c.K0 + kk];
    else if (kk < c.K0 + c.K1)
      v[i] = c.x1[m * c.K1 + (kk - c.K0)];
  }
  return v;
}

// dZ = dH * act'(.): ReLU from the layer's output (H > 0, as torch's
// threshold_backward), SiLU from its pre-activation. Zero-filled tails stay 0.
template <int ACT>
DEV_INLINE f32x4 qe_dz(f32x4 dh, f32x4 aux) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (ACT == QE_ACT_RELU) dh[i] = aux[i] > 0.f ? dh[i] : 0.f;
    if (ACT == QE_ACT_SILU) dh[i] = dh[i] * silu_grad_f(aux[i]);
  }
  return dh;
}

// s += x with the rounding error of the add collected in c (Knuth's TwoSum,
// fp32 adds only). The bias gradient is a plain column sum of S values that
// largely cancel, one output element per column; carried this way its error
// is about one rounding of the result whatever the order of the rows.
DEV_INLINE void qe_two_sum(float& s, float& c, float x) {
  const float t = s + x;
  const float bp = t - s;
  c += (s - (t - bp)) + (x - bp);
  s = t;
}

// 4 consecutive elements of an output row of `ncols`, starting at column col
// (a multiple of 4); elements past ncols are dropped.
DEV_INLINE void qe_st4(float* __restrict__ p, long off, int col, int ncols,
                       f32x4 v, bool vec) {
  if (vec && col + 3 < ncols) {
    *reinterpret_cast<f32x4*>(p + off) = v;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (col + i < ncols) p[off + i] = v[i];
  }
}

// ------------------------------------------------------------------ forward
// Grid (ceil(S/64), ceil(N/BN), E). Workgroup tile 64 rows x BN columns.
// BN = 64: waves 2 x 2, 32 x 32 each as four 16 x 16 accumulators. BN = 16
// (N <= 16, the scalar head): waves 4 x 1, 16 x 16 each, so the head does not
// run MFMAs on 48 columns that are not there. A operand = W fragment, B
// operand = X fragment: acc[nj][mi][r] is row mi*16 + (lane&15), column
// nj*16 + (lane>>4)*4 + r of the wave's tile.
template <int BN>
struct alignas(16) QeFwdLds {
  float X[2][64][QE_LD];
  float W[2][BN][QE_LD];
};

template <int BN, int ACT>
__launch_bounds__(QE_THREADS) __global__ void qens_linear_fwd_kernel(
    const float* __restrict__ X0,  // [S, K0], member stride x0_es (0: shared)
    long x0_es,
    const float* __restrict__ X1,  // [S, K1] or null
    QensIn W,                      // E x [N, K0 + K1]
    QensIn B,                      // E x [N]
    float* __restrict__ Z,         // null, or as H
    float* __restrict__ H,         // rows of N, row stride out_ld, member out_es
    long out_ld, long out_es, int S, int K0, int K1, int N, int vflags) {
  constexpr int MI = BN == 64 ? 2 : 1;  // 16-row fragments per wave
  constexpr int NJ = BN == 64 ? 2 : 1;  // 16-column fragments per wave
  constexpr int WQ = BN == 64 ? 2 : 1;  // W pieces per thread and step
  __shared__ QeFwdLds<BN> lds;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int e = blockIdx.z;
  const int m0 = blockIdx.x * 64;
  const int n_blk = blockIdx.y * BN;
  const int wm = BN == 64 ? (wid >> 1) * 32 : wid * 16;
  const int wn = BN == 64 ? (wid & 1) * 32 : 0;
  const int l15 = lane & 15;
  const int g = lane >> 4;
  // staging: this thread's piece is row srow (+32 per q), columns k4..k4+3
  const int srow = tid >> 3;
  const int k4 = (tid & 7) * 4;
  const int K = K0 + K1;
  const float* __restrict__ Wp = qe_pick(W, e);
  const float* __restrict__ Bp = qe_pick(B, e);
  const QeCat cat = {X0 + (long)e * x0_es, X1, K0, K1,
                     (vflags & QE_VEC_X0) != 0, (vflags & QE_VEC_X1) != 0};
  const bool vec_w = (vflags & QE_VEC_W) != 0;
  const bool w_mine = BN == 64 || srow < BN;

  float bv[NJ][4];
#pragma unroll
  for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = n_blk + wn + nj * 16 + g * 4 + r;
      bv[nj][r] = n < N ? Bp[n] : 0.f;
    }

  f32x4 acc[NJ][MI];
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int i = 0; i < MI; ++i) acc[j][i] = {0.f, 0.f, 0.f, 0.f};

  f32x4 xr[2], wr[WQ];
  auto load = [&](int ks) {
    const int k = ks * QE_BK + k4;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int m = m0 + srow + q * 32;
      xr[q] = qe_ldcat(cat, m, k, m < S);
    }
#pragma unroll
    for (int q = 0; q < WQ; ++q) {
      const int n = n_blk + srow + q * 32;
      wr[q] = qe_ld4(Wp, (long)n * K, k, K, w_mine && n < N, vec_w);
    }
  };
  auto store = [&](int pp) {
#pragma unroll
    for (int q = 0; q < 2; ++q)
      *reinterpret_cast<f32x4*>(&lds.X[pp][srow + q * 32][k4]) = xr[q];
    if (w_mine) {
#pragma unroll
      for (int q = 0; q < WQ; ++q)
        *reinterpret_cast<f32x4*>(&lds.W[pp][srow + q * 32][k4]) = wr[q];
    }
  };
  auto mma = [&](int pp) {
#pragma unroll
    for (int g2 = 0; g2 < QE_BK / 16; ++g2) {
      f32x4 xf[MI], wf[NJ];
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
        xf[mi] = *reinterpret_cast<const f32x4*>(
            &lds.X[pp][wm + mi * 16 + l15][g2 * 16 + g * 4]);
#pragma unroll
      for (int nj = 0; nj < NJ; ++nj)
        wf[nj] = *reinterpret_cast<const f32x4*>(
            &lds.W[pp][wn + nj * 16 + l15][g2 * 16 + g * 4]);
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
          for (int mi = 0; mi < MI; ++mi)
            acc[nj][mi] =
                MFMA_F32_16x16x4(wf[nj][s], xf[mi][s], acc[nj][mi], 0, 0, 0);
    }
  };

  const int KS = (K + QE_BK - 1) / QE_BK;
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
  // z = acc + b, straight after the chain
#pragma unroll
  for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[nj][mi][r] = acc[nj][mi][r] + bv[nj][r];

  const bool vec_out = (vflags & QE_VEC_OUT) != 0;
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    const int m = m0 + wm + mi * 16 + l15;
    if (m >= S) continue;
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj) {
      const int n = n_blk + wn + nj * 16 + g * 4;
      if (n >= N) continue;
      const long o = (long)e * out_es + (long)m * out_ld + n;
      const f32x4 z4 = acc[nj][mi];
      if (ACT == QE_ACT_NONE) {
        qe_st4(H, o, n, N, z4, vec_out);
      } else {
        f32x4 h4;
#pragma unroll
        for (int r = 0; r < 4; ++r) h4[r] = qe_act(z4[r], ACT);
        if (ACT == QE_ACT_SILU && Z) qe_st4(Z, o, n, N, z4, vec_out);
        qe_st4(H, o, n, N, h4, vec_out);
      }
    }
  }
}

// -------------------------------------------------------------------- dgrad
// dX[S, c0:c1) = dZ[S, N] @ W[N, c0:c1), reduction over n. Grid (ceil(S/64),
// ceil((c1-c0)/64), E or 1); workgroup tile 64 rows x 64 input columns, waves
// 2 x 2. The W tile goes to LDS transposed ([k][n]). A operand = W^T
// fragment, B operand = dZ fragment: acc[kj][mi][r] is row mi*16 + (lane&15),
// input column kj*16 + (lane>>4)*4 + r.
// members == 1: one member per blockIdx.z, dX [E, S, c1-c0]. members == E
// (grid z = 1): the reduction loop runs over n of member 0, then member 1,
// ... into the same accumulator, and dX [S, c1-c0] is the sum over members
// (the gradient of the shared action); no per-member intermediate exists.
struct alignas(16) QeDgradLds {
  float dZ[2][64][QE_LD];
  float Wt[2][64][QE_LD];
};

template <int ACT>
__launch_bounds__(QE_THREADS) __global__ void qens_linear_dgrad_kernel(
    const float* __restrict__ dH,   // [E, S, N]
    const float* __restrict__ AUX,  // [E, S, N]: H (ReLU) or Z (SiLU)
    QensIn W,                       // E x [N, K]
    float* __restrict__ dX,  // rows of c1-c0, row stride dx_ld, member dx_es
    long dx_ld, long dx_es, int S, int K, int N, int c0, int c1, int members,
    int vflags) {
  __shared__ QeDgradLds lds;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int e0 = blockIdx.z;  // 0 in the summed mode
  const int m0 = blockIdx.x * 64;
  const int k_blk = blockIdx.y * 64;
  const int wm = (wid >> 1) * 32;
  const int wk = (wid & 1) * 32;
  const int l15 = lane & 15;
  const int g = lane >> 4;
  // dZ staging: row srow (+32 per q), reduction columns n4..n4+3.
  // W staging: reduction row srow, input columns k4 (+32 per q) .. +3.
  const int srow = tid >> 3;
  const int n4 = (tid & 7) * 4;
  const int k4 = (tid & 7) * 4;
  const bool vec_dh = (vflags & QE_VEC_DH) != 0;
  const bool vec_w = (vflags & QE_VEC_W) != 0;
  const int KW = c1 - c0;

  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  const int NS = (N + QE_BK - 1) / QE_BK;
  f32x4 zr[2], wr[2];
  auto load = [&](int t) {
    const int em = members == 1 ? e0 : t / NS;
    const int n0 = (members == 1 ? t : t - em * NS) * QE_BK;
    const long ebase = (long)em * S * N;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int m = m0 + srow + q * 32;
      const f32x4 dh = qe_ld4(dH + ebase, (long)m * N, n0 + n4, N, m < S, vec_dh);
      f32x4 ax = {0.f, 0.f, 0.f, 0.f};
      if (ACT != QE_ACT_NONE)
        ax = qe_ld4(AUX + ebase, (long)m * N, n0 + n4, N, m < S, vec_dh);
      zr[q] = qe_dz<ACT>(dh, ax);
    }
    const float* __restrict__ Wp = qe_pick(W, em);
    const int n = n0 + srow;
#pragma unroll
    for (int q = 0; q < 2; ++q)
      wr[q] = qe_ld4(Wp, (long)n * K, c0 + k_blk + k4 + q * 32, c1, n < N, vec_w);
  };
  auto store = [&](int pp) {
#pragma unroll
    for (int q = 0; q < 2; ++q)
      *reinterpret_cast<f32x4*>(&lds.dZ[pp][srow + q * 32][n4]) = zr[q];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int i = 0; i < 4; ++i) lds.Wt[pp][k4 + q * 32 + i][srow] = wr[q][i];
  };
  auto mma = [&](int pp) {
#pragma unroll
    for (int g2 = 0; g2 < QE_BK / 16; ++g2) {
      f32x4 zf[2], wf[2];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
        zf[mi] = *reinterpret_cast<const f32x4*>(
            &lds.dZ[pp][wm + mi * 16 + l15][g2 * 16 + g * 4]);
#pragma unroll
      for (int kj = 0; kj < 2; ++kj)
        wf[kj] = *reinterpret_cast<const f32x4*>(
            &lds.Wt[pp][wk + kj * 16 + l15][g2 * 16 + g * 4]);
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int kj = 0; kj < 2; ++kj)
#pragma unroll
          for (int mi = 0; mi < 2; ++mi)
            acc[kj][mi] =
                MFMA_F32_16x16x4(wf[kj][s], zf[mi][s], acc[kj][mi], 0, 0, 0);
    }
  };

  const int T = NS * members;  // >= 1
  load(0);
  store(0);
  for (int t = 0; t + 1 < T; ++t) {
    __syncthreads();
    load(t + 1);
    mma(t & 1);
    store((t + 1) & 1);
  }
  __syncthreads();
  mma((T - 1) & 1);
  // The first read of the accumulator, in straight-line code after the
  // chain and ahead of the guarded stores (x + 0.0f is a real add).
#pragma unroll
  for (int kj = 0; kj < 2; ++kj)
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[kj][mi][r] = acc[kj][mi][r] + 0.0f;

  const bool vec_out = (vflags & QE_VEC_OUT) != 0;
#pragma unroll
  for (int mi = 0; mi < 2; ++mi) {
    const int m = m0 + wm + mi * 16 + l15;
    if (m >= S) continue;
#pragma unroll
    for (int kj = 0; kj < 2; ++kj) {
      const int k = k_blk + wk + kj * 16 + g * 4;
      if (k >= KW) continue;
      qe_st4(dX, (long)e0 * dx_es + (long)m * dx_ld + k, k, KW, acc[kj][mi],
             vec_out);
    }
  }
}

// -------------------------------------------------------------------- wgrad
// Partial dW_e[N, K] = dZ_e^T @ [X0 | X1] over one slice of S, and the
// partial column sums of dZ_e. Grid (ceil(N/64), ceil(K/64), E * slices);
// workgroup tile 64 n x 64 k, waves 2 x 2 (32 n x 32 k each): at the bench
// point (N 256, K 393, E 2, 8 slices) 448 workgroups, a 64 x 128 tile would
// leave 256 with twice the work each and a 7th k-tile that is 9 columns
// wide. Both tiles go to LDS transposed ([n][s] and [k][s]), consecutive
// lanes holding consecutive s of one piece. A operand = X^T fragment, B
// operand = dZ^T fragment: acc[ki][ni][r] is dW[n = ni*16 + (lane&15)]
// [k = ki*16 + (lane>>4)*4 + r]. The column sums come from the dZ^T
// fragments of the workgroups with blockIdx.y == 0. Slab image of a (member,
// slice): dW [N][KP], KP = K rounded up to 4 so that every store is 16 bytes
// (the pad columns hold the zeros of the k tail), then db [N].
struct alignas(16) QeWgradLds {
  float dZt[2][64][QE_LD];
  float Xt[2][64][QE_LD];
};

template <int ACT>
__launch_bounds__(QE_THREADS) __global__ void qens_linear_wgrad_kernel(
    const float* __restrict__ dH,   // [E, S, N]
    const float* __restrict__ AUX,  // [E, S, N]: H (ReLU) or Z (SiLU)
    const float* __restrict__ X0, long x0_es, const float* __restrict__ X1,
    float* __restrict__ slab,  // [E, slices, slab_stride]
    long slab_stride, int slices, int S, int K0, int K1, int N, int s_per,
    int vflags) {
  __shared__ QeWgradLds lds;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int e = blockIdx.z / slices;
  const int sl = blockIdx.z - e * slices;
  const int n_blk = blockIdx.x * 64;
  const int k_blk = blockIdx.y * 64;
  const int s_begin = sl * s_per;
  const int s_end = min(S, s_begin + s_per);
  const int wn = (wid >> 1) * 32;
  const int wk = (wid & 1) * 32;
  const int l15 = lane & 15;
  const int g = lane >> 4;
  // staging: row ss of the 32-row step, pieces pc and pc + 32 of n and of k
  const int ss = tid & 31;
  const int pc = (tid >> 5) * 4;
  const int K = K0 + K1;
  const int KP = (K + 3) & ~3;
  const bool vec_dh = (vflags & QE_VEC_DH) != 0;
  const bool do_db = blockIdx.y == 0 && wk == 0;
  const long ebase = (long)e * S * N;
  const QeCat cat = {X0 + (long)e * x0_es, X1, K0, K1,
                     (vflags & QE_VEC_X0) != 0, (vflags & QE_VEC_X1) != 0};

  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};
  float db_acc[2] = {0.f, 0.f}, db_c[2] = {0.f, 0.f};

  f32x4 zr[2], xr[2];
  auto load = [&](int st) {
    const int s = s_begin + st * QE_BK + ss;
    const bool s_ok = s < s_end;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int n = n_blk + pc + q * 32;
      const f32x4 dh = qe_ld4(dH + ebase, (long)s * N, n, N, s_ok, vec_dh);
      f32x4 ax = {0.f, 0.f, 0.f, 0.f};
      if (ACT != QE_ACT_NONE)
        ax = qe_ld4(AUX + ebase, (long)s * N, n, N, s_ok, vec_dh);
      zr[q] = qe_dz<ACT>(dh, ax);
      xr[q] = qe_ldcat(cat, s, k_blk + pc + q * 32, s_ok);
    }
  };
  auto store = [&](int pp) {
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        lds.dZt[pp][pc + q * 32 + i][ss] = zr[q][i];
        lds.Xt[pp][pc + q * 32 + i][ss] = xr[q][i];
      }
  };
  auto mma = [&](int pp) {
#pragma unroll
    for (int g2 = 0; g2 < QE_BK / 16; ++g2) {
      f32x4 zf[2], xf[2];
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        zf[ni] = *reinterpret_cast<const f32x4*>(
            &lds.dZt[pp][wn + ni * 16 + l15][g2 * 16 + g * 4]);
        if (do_db) {
#pragma unroll
          for (int j = 0; j < 4; ++j) qe_two_sum(db_acc[ni], db_c[ni], zf[ni][j]);
        }
      }
#pragma unroll
      for (int ki = 0; ki < 2; ++ki)
        xf[ki] = *reinterpret_cast<const f32x4*>(
            &lds.Xt[pp][wk + ki * 16 + l15][g2 * 16 + g * 4]);
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int ki = 0; ki < 2; ++ki)
#pragma unroll
          for (int ni = 0; ni < 2; ++ni)
            acc[ki][ni] =
                MFMA_F32_16x16x4(xf[ki][s], zf[ni][s], acc[ki][ni], 0, 0, 0);
    }
  };

  const int NST = (s_end - s_begin + QE_BK - 1) / QE_BK;  // >= 1
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

  float* __restrict__ o = slab + ((long)e * slices + sl) * slab_stride;
  // The first read of the accumulator, in straight-line code after the
  // chain and ahead of the guarded stores (x + 0.0f is a real add).
#pragma unroll
  for (int ki = 0; ki < 2; ++ki)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[ki][ni][r] = acc[ki][ni][r] + 0.0f;
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const int n = n_blk + wn + ni * 16 + l15;
    if (do_db) {
      float d = db_acc[ni], c = db_c[ni];
#pragma unroll
      for (int off = 16; off <= 32; off <<= 1) {
        const float od = __shfl_xor(d, off), oc = __shfl_xor(c, off);
        qe_two_sum(d, c, od);
        c += oc;
      }
      if (g == 0 && n < N) o[(long)N * KP + n] = d + c;
    }
    if (n >= N) continue;
#pragma unroll
    for (int ki = 0; ki < 2; ++ki) {
      const int k = k_blk + wk + ki * 16 + g * 4;
      if (k < KP)  // k % 4 == 0 and KP % 4 == 0: k + 3 < KP
        *reinterpret_cast<f32x4*>(o + (long)n * KP + k) = acc[ki][ni];
    }
  }
}

// Sum the slices' slabs in ascending order into the members' dW and db, each
// element once. Grid (blocks, E).
__launch_bounds__(QE_THREADS) __global__ void qens_wgrad_reduce_kernel(
    const float* __restrict__ slab, long slab_stride, int slices, QensOut dW,
    QensOut dB, int K, int N) {
  const int e = blockIdx.y;
  const int KP = (K + 3) & ~3;
  const long nk = (long)N * K;
  const long total = nk + N;
  const long stride = (long)gridDim.x * blockDim.x;
  const float* __restrict__ src = slab + (long)e * slices * slab_stride;
  float* __restrict__ dw = qe_pick(dW, e);
  float* __restrict__ db = qe_pick(dB, e);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += stride) {
    long at;
    if (i < nk) {
      const long n = i / K;
      at = n * KP + (i - n * K);
    } else {
      at = (long)N * KP + (i - nk);
    }
    float s = 0.f;
    for (int z = 0; z < slices; ++z) s += src[(long)z * slab_stride + at];
    if (i < nk)
      dw[i] = s;
    else
      db[i - nk] = s;
  }
}

// ----------------------------------------------------------- host launchers

static bool qe_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static bool qe_shape_ok(int S, int K0, int K1, int N, int E, int act) {
  return S >= 1 && K0 >= 1 && K1 >= 0 && N >= 1 && E >= 1 && E <= QENS_MAX_E &&
         act >= QE_ACT_NONE && act <= QE_ACT_RELU;
}

static bool qe_members_al16(const QensIn& s, int E) {
  for (int e = 0; e < E; ++e)
    if (!qe_al16(s.p[e])) return false;
  return true;
}

// 16-byte access flags of the two input pieces
static int qe_cat_flags(const float* X0, long x0_es, const float* X1, int K0,
                        int K1) {
  int f = 0;
  if ((K0 & 3) == 0 && qe_al16(X0) && (x0_es & 3) == 0) f |= QE_VEC_X0;
  if ((K0 & 3) == 0 && K1 > 0 && (K1 & 3) == 0 && qe_al16(X1)) f |= QE_VEC_X1;
  return f;
}

template <int BN>
static void qe_launch_fwd(const float* X0, long x0_es, const float* X1,
                          const QensIn& W, const QensIn& B, float* Z, float* H,
                          long out_ld, long out_es, int S, int K0, int K1,
                          int N, int E, int act, int vflags, hipStream_t st) {
  dim3 grid((S + 63) / 64, (N + BN - 1) / BN, E), block(QE_THREADS);
  auto kernel = act == QE_ACT_SILU
                    ? qens_linear_fwd_kernel<BN, QE_ACT_SILU>
                    : act == QE_ACT_RELU
                          ? qens_linear_fwd_kernel<BN, QE_ACT_RELU>
                          : qens_linear_fwd_kernel<BN, QE_ACT_NONE>;
  hipLaunchKernelGGL(kernel, grid, block, 0, st, X0, x0_es, X1, W, B, Z, H,
                     out_ld, out_es, S, K0, K1, N, vflags);
}

extern "C" int launch_qens_linear_fwd(
    const float* X0, long x0_es, const float* X1, const QensIn& W,
    const QensIn& B, float* Z, float* H, long out_ld, long out_es, int S,
    int K0, int K1, int N, int E, int act, void* stream) {
  if (!qe_shape_ok(S, K0, K1, N, E, act) || (N + 63) / 64 > 65535) return 1;
  const int K = K0 + K1;
  int vflags = qe_cat_flags(X0, x0_es, X1, K0, K1);
  if ((K & 3) == 0 && qe_members_al16(W, E)) vflags |= QE_VEC_W;
  if ((out_ld & 3) == 0 && (out_es & 3) == 0 && qe_al16(H) && qe_al16(Z))
    vflags |= QE_VEC_OUT;
  if (N <= 16)
    qe_launch_fwd<16>(X0, x0_es, X1, W, B, Z, H, out_ld, out_es, S, K0, K1, N,
                      E, act, vflags, (hipStream_t)stream);
  else
    qe_launch_fwd<64>(X0, x0_es, X1, W, B, Z, H, out_ld, out_es, S, K0, K1, N,
                      E, act, vflags, (hipStream_t)stream);
  return 0;
}

extern "C" int launch_qens_linear_dgrad(
    const float* dH, const float* AUX, const QensIn& W, float* dX, long dx_ld,
    long dx_es, int S, int K, int N, int c0, int c1, int E, int summed,
    int act, void* stream) {
  if (!qe_shape_ok(S, K, 0, N, E, act) || c0 < 0 || c1 <= c0 || c1 > K ||
      (act != QE_ACT_NONE && !AUX) || (c1 - c0 + 63) / 64 > 65535)
    return 1;
  int vflags = 0;
  if ((K & 3) == 0 && (c0 & 3) == 0 && qe_members_al16(W, E))
    vflags |= QE_VEC_W;
  if ((N & 3) == 0 && qe_al16(dH) && qe_al16(AUX)) vflags |= QE_VEC_DH;
  if ((dx_ld & 3) == 0 && (dx_es & 3) == 0 && qe_al16(dX))
    vflags |= QE_VEC_OUT;
  dim3 grid((S + 63) / 64, (c1 - c0 + 63) / 64, summed ? 1 : E),
      block(QE_THREADS);
  auto kernel = act == QE_ACT_SILU
                    ? qens_linear_dgrad_kernel<QE_ACT_SILU>
                    : act == QE_ACT_RELU ? qens_linear_dgrad_kernel<QE_ACT_RELU>
                                         : qens_linear_dgrad_kernel<QE_ACT_NONE>;
  hipLaunchKernelGGL(kernel, grid, block, 0, (hipStream_t)stream, dH, AUX, W,
                     dX, dx_ld, dx_es, S, K, N, c0, c1, summed ? E : 1, vflags);
  return 0;
}

// Slices of S: about 256 rows each, at most QE_MAX_SPLIT, whole 32-row
// steps. A function of S alone, so the sum order is too.
extern "C" void qens_wgrad_geometry(int S, int K, int N, int* slices,
                                    int* s_per, long* slab_stride) {
  int want = (S + 255) / 256;
  want = want < 1 ? 1 : (want > QE_MAX_SPLIT ? QE_MAX_SPLIT : want);
  int per = (S + want - 1) / want;
  per = (per + QE_BK - 1) / QE_BK * QE_BK;
  *s_per = per;
  *slices = (S + per - 1) / per;
  const long KP = (K + 3) & ~3;
  *slab_stride = ((long)N * KP + N + 3) / 4 * 4;
}

extern "C" int launch_qens_linear_wgrad(
    const float* dH, const float* AUX, const float* X0, long x0_es,
    const float* X1, float* slab, const QensOut& dW, const QensOut& dB, int S,
    int K0, int K1, int N, int E, int act, void* stream) {
  if (!qe_shape_ok(S, K0, K1, N, E, act) || (act != QE_ACT_NONE && !AUX))
    return 1;
  const int K = K0 + K1;
  int slices, s_per;
  long slab_stride;
  qens_wgrad_geometry(S, K, N, &slices, &s_per, &slab_stride);
  if ((K + 63) / 64 > 65535 || (long)E * slices > 65535 || !qe_al16(slab))
    return 1;
  int vflags = qe_cat_flags(X0, x0_es, X1, K0, K1);
  if ((N & 3) == 0 && qe_al16(dH) && qe_al16(AUX)) vflags |= QE_VEC_DH;
  dim3 grid((N + 63) / 64, (K + 63) / 64, E * slices), block(QE_THREADS);
  auto kernel = act == QE_ACT_SILU
                    ? qens_linear_wgrad_kernel<QE_ACT_SILU>
                    : act == QE_ACT_RELU ? qens_linear_wgrad_kernel<QE_ACT_RELU>
                                         : qens_linear_wgrad_kernel<QE_ACT_NONE>;
  hipLaunchKernelGGL(kernel, grid, block, 0, (hipStream_t)stream, dH, AUX, X0,
                     x0_es, X1, slab, slab_stride, slices, S, K0, K1, N, s_per,
                     vflags);
  const long total = (long)N * K + N;
  hipLaunchKernelGGL(qens_wgrad_reduce_kernel,
                     dim3(flat_blocks(total, QE_THREADS), E), dim3(QE_THREADS),
                     0, (hipStream_t)stream, slab, slab_stride, slices, dW, dB,
                     K, N);
  return 0;
}
