// Batched MCTS over the search arena (K16 of SURVEY.md): PUCT selection and
// expansion + value backup, one launch each per simulation.
//
// The arena is the struct-of-arrays of search/mcts.py::_Arena, B independent
// trees of N = num_simulations + 1 node slots and A actions:
//   visit, value_sum, reward, discount  [B, N]     f32
//   prior                               [B, N, A]  f32
//   children                            [B, N, A]  i64 (-1: no child)
//   parent, act_from_parent             [B, N]     i64 (-1: the root)
//   min_q, max_q                        [B]        f32 (value normalisation)
//
// mcts_select_kernel, per tree: start at node 0; score every action
//   cv, cs, r, g = visit, value_sum, reward, discount of the child (0 if none)
//   q_edge = r + g * (cs / max(cv, 1))
//   span   = max(max_q - min_q, 1e-3)
//   q_norm = cv > 0 ? (q_edge - min_q) / span
//                   : (q(node) - min_q) / span          (the parent's value)
//   score  = q_norm + ((c_puct * prior) * sqrt(max(visit[node], 1))) / (1 + cv)
// take the arg-max (ties -> lowest action); an edge without a child ends the
// descent with (node, action), otherwise step to the child. A path in a tree
// of N slots has fewer than N edges, so the loop over N levels ends by itself.
//
// mcts_expand_backup_kernel, per tree: fill slot new_node (reward, discount,
// prior row, parent, act_from_parent), link it under (sel_parent, sel_action)
// and walk new_node -> root: visit += 1, value_sum += g,
// q = value_sum / max(visit, 1) into min_q / max_q, g = reward + discount * g.
//
// Both kernels reproduce the torch composition in search/mcts.py bit for bit:
// a search is a chain of arg-maxes, and one differing last bit picks another
// action and grows another tree. So every operation is the single correctly
// rounded f32 operation torch runs, in torch's order, and FMA contraction is
// off for the whole file (hipcc contracts a * b + c by default, and
// __fmul_rn / __fadd_rn are plain operators that contract as well). Division
// and sqrtf are hipcc's correctly rounded defaults. Inputs are assumed
// finite: a NaN score is never the arg-max here, as it is in torch.argmax.
//
// Geometry: a group of G = min(64, next_pow2(A)) lanes owns one tree, lane l
// scoring actions l, l + G, ...; 256 / G trees per 256-thread workgroup. The
// work is a pointer chase over a few hundred bytes per tree, so what counts is
// the chain of dependent loads: per level children[node, a] and then the four
// child statistics together (the node's own visit / value_sum go out with the
// first). The arg-max is a width-G __shfl_xor butterfly on (score, action).
// No LDS, no workgroup barrier, no atomics: a tree belongs to one group, and a
// group without a tree returns before it touches memory. The backup walk runs
// in lane 0 of the group; the other lanes copy the prior row.
//
// Indices read from the arena are used only inside [0, N) x [0, A): a child
// or parent outside the range counts as none, and a tree whose selection is
// outside it is left as it was.
#include "common.h"
#include "launchers.h"

#pragma clang fp contract(off)

#define MCTS_THREADS 256

extern "C" __global__ void __launch_bounds__(MCTS_THREADS) mcts_select_kernel(
    const float* __restrict__ visit, const float* __restrict__ value_sum,
    const float* __restrict__ reward, const float* __restrict__ discount,
    const float* __restrict__ prior, const long* __restrict__ children,
    const float* __restrict__ min_q, const float* __restrict__ max_q,
    long* __restrict__ sel_parent, long* __restrict__ sel_action, int B, int N,
    int A, int log2_g, float c_puct) {
  const int G = 1 << log2_g;
  const int lane = threadIdx.x & (G - 1);
  const long b = (long)blockIdx.x * (MCTS_THREADS >> log2_g) +
                 (threadIdx.x >> log2_g);
  if (b >= B) return;  // whole groups leave: the shuffles below stay in-group
  const float* __restrict__ v_b = visit + b * N;
  const float* __restrict__ s_b = value_sum + b * N;
  const float* __restrict__ r_b = reward + b * N;
  const float* __restrict__ g_b = discount + b * N;
  const float* __restrict__ p_b = prior + b * N * A;
  const long* __restrict__ c_b = children + b * N * A;
  const float lo = min_q[b];
  const float span = fmaxf(max_q[b] - lo, 1e-3f);

  int node = 0;
  for (int level = 0; level < N; ++level) {
    const float pv = v_b[node];
    const float pq = pv > 0.f ? s_b[node] / fmaxf(pv, 1.f) : 0.f;
    const float parent_qn = (pq - lo) / span;
    const float root_n = sqrtf(fmaxf(pv, 1.f));
    float best = -INFINITY;
    int best_a = A;
    int best_c = -1;
    for (int a = lane; a < A; a += G) {
      const long e = (long)node * A + a;
      const long c = c_b[e];
      const float p = p_b[e];
      const bool has = c >= 0 && c < N;
      const long ci = has ? c : 0;
      const float cv = has ? v_b[ci] : 0.f;
      const float cs = has ? s_b[ci] : 0.f;
      const float r = has ? r_b[ci] : 0.f;
      const float g = has ? g_b[ci] : 0.f;
      const float q_edge = r + g * (cs / fmaxf(cv, 1.f));
      const float q_norm = cv > 0.f ? (q_edge - lo) / span : parent_qn;
      const float score = q_norm + ((c_puct * p) * root_n) / (1.f + cv);
      if (score > best) {  // ascending a: a tie keeps the lower action
        best = score;
        best_a = a;
        best_c = has ? (int)c : -1;
      }
    }
    for (int o = G >> 1; o > 0; o >>= 1) {
      const float ov = __shfl_xor(best, o, G);
      const int oa = __shfl_xor(best_a, o, G);
      if (ov > best || (ov == best && oa < best_a)) {
        best = ov;
        best_a = oa;
      }
    }
    best_a = min(best_a, A - 1);
    // the lane that owns best_a holds it as its own best, with the child
    const int child = __shfl(best_c, best_a & (G - 1), G);
    if (child < 0 || level == N - 1) {
      if (lane == 0) {
        sel_parent[b] = node;
        sel_action[b] = best_a;
      }
      break;
    }
    node = child;
  }
}

extern "C" __global__ void __launch_bounds__(MCTS_THREADS)
    mcts_expand_backup_kernel(
        float* visit, float* value_sum, float* reward, float* discount,
        float* prior, long* children, long* parent, long* act_from_parent,
        float* min_q, float* max_q, const long* __restrict__ sel_parent,
        const long* __restrict__ sel_action,
        const float* __restrict__ reward_new,
        const float* __restrict__ discount_new,
        const float* __restrict__ prior_new,
        const float* __restrict__ value_new, int B, int N, int A, int log2_g,
        int new_node) {
  const int G = 1 << log2_g;
  const int lane = threadIdx.x & (G - 1);
  const long b = (long)blockIdx.x * (MCTS_THREADS >> log2_g) +
                 (threadIdx.x >> log2_g);
  if (b >= B) return;
  const long sp = sel_parent[b], sa = sel_action[b];
  if (sp < 0 || sp >= N || sa < 0 || sa >= A) return;
  const long row = b * N;

  for (int a = lane; a < A; a += G)
    prior[(row + new_node) * A + a] = prior_new[b * A + a];
  if (lane != 0) return;

  float r = reward_new[b], d = discount_new[b];
  reward[row + new_node] = r;
  discount[row + new_node] = d;
  parent[row + new_node] = sp;
  act_from_parent[row + new_node] = sa;
  children[(row + sp) * A + sa] = new_node;

  // the new node's reward, discount and parent stay in registers; every
  // later node costs one round of loads, all indexed by cur
  float g = value_new[b];
  float lo = min_q[b], hi = max_q[b];
  long cur = new_node, nxt = sp;
  for (int step = 0; step < N; ++step) {
    const float v = visit[row + cur] + 1.f;
    const float s = value_sum[row + cur] + g;
    visit[row + cur] = v;
    value_sum[row + cur] = s;
    const float q = s / fmaxf(v, 1.f);
    lo = fminf(lo, q);
    hi = fmaxf(hi, q);
    g = r + d * g;
    if (nxt < 0 || nxt >= N) break;  // cur was the root
    cur = nxt;
    r = reward[row + cur];
    d = discount[row + cur];
    nxt = parent[row + cur];
  }
  min_q[b] = lo;
  max_q[b] = hi;
}

// ----------------------------------------------------------- host launchers

// log2 of the group width min(64, next_pow2(A))
static int mcts_log2_group(int A) {
  int l = 0;
  while ((1 << l) < A && l < 6) ++l;
  return l;
}

extern "C" void launch_mcts_select(
    const float* visit, const float* value_sum, const float* reward,
    const float* discount, const float* prior, const long* children,
    const float* min_q, const float* max_q, long* sel_parent, long* sel_action,
    int B, int N, int A, float c_puct, void* stream) {
  if (B <= 0) return;
  const int log2_g = mcts_log2_group(A);
  const int trees = MCTS_THREADS >> log2_g;
  hipLaunchKernelGGL(mcts_select_kernel, dim3((B + trees - 1) / trees),
                     dim3(MCTS_THREADS), 0, (hipStream_t)stream, visit,
                     value_sum, reward, discount, prior, children, min_q,
                     max_q, sel_parent, sel_action, B, N, A, log2_g, c_puct);
}

extern "C" void launch_mcts_expand_backup(
    float* visit, float* value_sum, float* reward, float* discount,
    float* prior, long* children, long* parent, long* act_from_parent,
    float* min_q, float* max_q, const long* sel_parent, const long* sel_action,
    const float* reward_new, const float* discount_new, const float* prior_new,
    const float* value_new, int B, int N, int A, int new_node, void* stream) {
  if (B <= 0) return;
  const int log2_g = mcts_log2_group(A);
  const int trees = MCTS_THREADS >> log2_g;
  hipLaunchKernelGGL(mcts_expand_backup_kernel, dim3((B + trees - 1) / trees),
                     dim3(MCTS_THREADS), 0, (hipStream_t)stream, visit,
                     value_sum, reward, discount, prior, children, parent,
                     act_from_parent, min_q, max_q, sel_parent, sel_action,
                     reward_new, discount_new, prior_new, value_new, B, N, A,
                     log2_g, new_node);
}
