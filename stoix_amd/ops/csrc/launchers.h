// The host launcher of every kernel: the one declaration that bind.cpp calls
// and that the .hip file defining the launcher is compiled against. The
// launchers have C linkage, so the linker sees no types; a definition that
// disagrees with its line here is a compile error (conflicting declaration)
// in the .hip file that holds it.
//
// Plain C++, no HIP headers: the host compiler that builds bind.cpp reads
// this file. Streams are hipStream_t passed as void*, bf16 buffers are void*.
#pragma once
#include <cstdint>

// ---- operands of the paired launchers, one struct per net or chain. The
// kernels take these structs by value (wgrad.hip, optim.hip, mlp.hip).

// One net's split-K weight gradient: dW = dZ^T @ X, db = colsum(dZ).
struct WgradNet {
  const void* dZ;  // bf16 [S, N_STRIDE]
  const void* X;   // bf16 [S, K]
  float* slab;     // [WG_SLICES, slab_stride]
  long dW_off, db_off, slab_stride;  // db_off < 0: no bias sum
  int N_VALID;
  // null: dZ is the operand. Else bf16 [S, N_STRIDE], the pre-activation of
  // the layer, and the operand is dZ * silu'(Zact), formed while staging.
  const void* Zact;
};

// One chain's slab reduce into its flat bf16 grad.
struct TailChain {
  const float* slab;  // [WG_SLICES, slab_stride]
  void* grad16;       // bf16 [n]
  long slab_stride, n;
  float* sqnorm;  // [0] = total, [1 + b] = tree sum of block b; or null
  long* step_t;   // null with sqnorm
  unsigned int* counter;  // slab_reduce_norm_pair only: zero between launches
};

// One chain's clip + Adam + bf16 mirror.
struct AdamChain {
  float* param;
  const void* grad;  // bf16 [n]
  float* exp_avg;
  float* exp_avg_sq;
  const float* sqnorm;
  const long* step_t;
  void* param_bf16;  // bf16 [n] or null
  long n;
  float lr;
};

// One net's Linear(+bias)+SiLU forward.
struct LinSiluNet {
  const void* W;      // bf16 [N, K] row-major
  const float* bias;  // [N]
  void* Z;            // bf16 [S, N]
  void* H;            // bf16 [S, N]
};

// The members of a Q-ensemble layer (qens.hip): one pointer per member for an
// operand that stays in the members' own tensors (weights, biases, their
// gradients). Entries past the member count are not read.
#define QENS_MAX_E 4
struct QensIn {
  const float* p[QENS_MAX_E];
};
struct QensOut {
  float* p[QENS_MAX_E];
};

// The Gaussian actor MLP (actor_mlp.hip): 1..ACTOR_MAX_L hidden nn.Linear
// layers and the two head linears, all read in place, passed by value.
// Entries past L are not read.
#define ACTOR_MAX_L 4
struct ActorNet {
  const float* W[ACTOR_MAX_L];  // [N[l], N[l-1]] (layer 0: [N[0], K0])
  const float* b[ACTOR_MAX_L];  // [N[l]]
  int N[ACTOR_MAX_L];
  const float *Wloc, *bloc, *Wscale, *bscale;  // [A, N[L-1]], [A]
  int L, K0, A, S;
};
// One [S, N[l]] fp32 buffer per hidden layer (saved H / Z, dZ); null: absent.
struct ActorBufs {
  float* p[ACTOR_MAX_L];
};

// The multi-tensor optimiser tail (multi_adam.hip): every tensor of up to
// MADAM_MAX_CHAINS clip + Adam (+ polyak) chains, passed to both kernels by
// value. A chain's tensors are adjacent, in chain order; tensor i owns the
// blocks [first_block, first_block of i + 1), one per MADAM_CHUNK elements,
// and block b of the grid keeps its sum of squares in partials[b].
#define MADAM_MAX_TENSORS 64
#define MADAM_MAX_CHAINS 4
#define MADAM_CHUNK 2048       // elements per 256-thread block
#define MADAM_MAX_CHUNKS 4096  // blocks of one chain
struct MultiAdamTensor {
  float* p;
  const float* g;  // null: no gradient this step, only tgt is updated
  float* m;
  float* v;
  float* tgt;   // polyak target or null
  float* step;  // torch's 0-dim fp32 step of this parameter
  unsigned int numel;
  unsigned short first_block, chain;
};
struct MultiAdamChain {
  float b1, b2, omb1, omb2, eps, max_norm, tau, omt;  // omX = fl(1 - X)
  float lr;             // used when lr_ptr is null
  int clip;             // 0: no norm, coef = 1
  const float* lr_ptr;  // a tensor lr, read on the device
  unsigned int part_begin, part_count;  // the chain's blocks
};
struct MultiAdamTable {
  MultiAdamTensor t[MADAM_MAX_TENSORS];
  MultiAdamChain c[MADAM_MAX_CHAINS];
  int n_tensors, n_blocks;
};
static_assert(sizeof(MultiAdamTable) <= 3968,
              "the table is a kernel argument: 4 KB with room for the rest");

extern "C" {

// ---- multi_adam.hip. partials holds n_blocks floats. Launch A writes the
// per-block sums of squares of the clipped chains and every tensor's
// step + 1; launch B reads both.
void launch_multi_adam_norm(const MultiAdamTable& T, float* partials,
                            void* stream);
void launch_multi_adam_update(const MultiAdamTable& T, const float* partials,
                              void* stream);

// ---- envs.hip. The three step launchers take one parameter list, written
// once; only the action type differs.
#define ENV_STEP_PARAMS(Action)                                               \
  float *state, const Action *action, int *step_count, float *ep_return,      \
      int *ep_length, float *last_ep_return, int *last_ep_length,             \
      float *obs_out, float *next_obs_out, float *reward_out,                 \
      float *discount_out, unsigned char *steptype_out,                       \
      unsigned char *done_out, int B, int max_episode_steps, uint64_t seed,   \
      unsigned int *draw_buf, unsigned int draw_offset, int do_bump,          \
      void *stream
void launch_cartpole_step(ENV_STEP_PARAMS(long));
void launch_ant_step(ENV_STEP_PARAMS(float));
void launch_humanoid_step(ENV_STEP_PARAMS(float));
void launch_ant_reset(float* state, int B, uint64_t seed, uint32_t draw,
                      void* stream);

// ---- snake.hip
void launch_snake_step(
    int* grid, long* head_r, long* head_c, long* fruit_r, long* fruit_c,
    int* length, const long* action, int* step_count, float* ep_return,
    int* ep_length, float* last_ep_return, int* last_ep_length,
    float* obs_out, float* next_obs_out, float* reward_out,
    float* discount_out, unsigned char* steptype_out,
    unsigned char* done_out, int B, int max_episode_steps, uint64_t seed,
    unsigned int* draw_buf, unsigned int draw_offset, int do_bump,
    void* stream);

// ---- scan.hip
void launch_gae(const float* r_t, const float* discount_t, const float* v_tm1,
                const float* v_t, const unsigned char* trunc_t, float* adv_out,
                float* target_out, int T, int B, float lambda_, void* stream);
void launch_lambda_returns(const float* r_t, const float* discount_t,
                           const float* v_t, float* out, int T, int B,
                           float lambda_, void* stream);
void launch_vtrace(const float* v_tm1, const float* v_t, const float* r_t,
                   const float* discount_t, const float* rho_tm1,
                   float* errors_out, float* pg_adv_out, int T, int B,
                   float lambda_, float clip_rho, float clip_pg_rho,
                   void* stream);
void launch_offpolicy_returns(const float* q_t, const float* v_t,
                              const float* r_t, const float* discount_t,
                              const float* c_t, float* out, int T, int B,
                              void* stream);

// ---- optim.hip
void launch_fused_adam(float* param, const float* grad, float* exp_avg,
                       float* exp_avg_sq, float* sqnorm, long* step_t, long n,
                       float lr, float beta1, float beta2, float eps,
                       float max_norm, void* stream);
void launch_fused_adam_bf16(float* param, const void* grad, float* exp_avg,
                            float* exp_avg_sq, float* sqnorm, long* step_t,
                            void* param_bf16, long n, float lr, float beta1,
                            float beta2, float eps, float max_norm,
                            float grad_scale, int do_prologue, long sqnorm_len,
                            void* stream);
void launch_adam_pair(const AdamChain& c0, const AdamChain& c1, float beta1,
                      float beta2, float eps, float max_norm, float grad_scale,
                      void* stream);
void launch_polyak(const float* online, float* target, long n, float tau,
                   void* stream);

// ---- wgrad.hip
void launch_wgrad(const void* dZ, const void* X, float* slab, long dW_off,
                  long db_off, long slab_stride, int S, int N_STRIDE, int K,
                  int N_VALID, int kpg_override, int ntb_override,
                  void* stream);
void launch_slab_reduce(float* slab, void* grad16, long slab_stride, long n,
                        float* sqnorm, long* step_t, void* stream);
// Returns 1 if the paired kernel ran, 0 after the per-net fallback. With a
// Zact on either net there is no fallback: the fused kernel runs (1) when
// both nets carry one and the shape is a layer-1 shape, else nothing is
// launched and the call returns WGRAD_PAIR_NOT_TAKEN.
#define WGRAD_PAIR_NOT_TAKEN (-1)
int launch_wgrad_pair(const WgradNet& net0, const WgradNet& net1, int S,
                      int N_STRIDE, int K, int variant, void* stream);
void launch_slab_reduce_pair(const TailChain& c0, const TailChain& c1,
                             void* stream);
void launch_slab_reduce_norm_pair(const TailChain& c0, const TailChain& c1,
                                  void* stream);
void launch_tr16_probe(const void* in, float* out, int base_mode,
                       void* stream);

// ---- mlp.hip
void launch_mfma_probe(const void* A, const void* B, float* D0, float* D1,
                       void* stream);
void launch_bump_add(unsigned int* p, unsigned int n, void* stream);
void launch_policy_value_step(
    const float* obs, const void* W1a, const float* b1a, const void* W2a,
    const float* b2a, const void* Wha, const float* bha, const void* W1c,
    const float* b1c, const void* W2c, const float* b2c, const void* Wvc,
    const float* bvc, float* obs_mirror, float* action_out, float* logp_out,
    float* value_out, const float* nmean, const float* nvar, int B, int OBS,
    int ACT, int HID, float min_scale, float aff_scale, float aff_shift,
    float log_aff_scale, int greedy, uint64_t seed, unsigned int* draw_buf,
    unsigned int draw_offset, int do_bump, void* stream);
void launch_policy_value_step_disc(
    const float* obs, const void* W1a, const float* b1a, const void* W2a,
    const float* b2a, const void* Wha, const float* bha, const void* W1c,
    const float* b1c, const void* W2c, const float* b2c, const void* Wvc,
    const float* bvc, float* obs_mirror, long* action_out, float* logp_out,
    float* value_out, const float* nmean, const float* nvar, int B, int OBS,
    int ACT, int HID, int greedy, uint64_t seed, unsigned int* draw_buf,
    unsigned int draw_offset, int do_bump, void* stream);
void launch_value_forward(const float* obs, const void* W1c, const float* b1c,
                          const void* W2c, const float* b2c, const void* Wvc,
                          const float* bvc, float* value_out,
                          const float* nmean, const float* nvar, int B,
                          int OBS, int HID, void* stream);
void launch_rollout_step_ant(
    float* obs_io, float* env_state, int* step_count, float* ep_return,
    int* ep_length, float* last_ep_return, int* last_ep_length,
    const void* W1a, const float* b1a, const void* W2a, const float* b2a,
    const void* Wha, const float* bha, const void* W1c, const float* b1c,
    const void* W2c, const float* b2c, const void* Wvc, const float* bvc,
    float* buf_obs, float* buf_action, float* buf_logp, float* buf_value,
    float* buf_bootstrap, float* buf_reward, float* buf_discount,
    unsigned char* buf_steptype, int B, int OBS, int ACT, int HID,
    int max_episode_steps, float min_scale, float aff_scale, float aff_shift,
    float log_aff_scale, uint64_t policy_seed, uint64_t env_seed,
    unsigned int* policy_draw, unsigned int* env_draw,
    unsigned int draw_offset, void* stream);
void launch_linear_silu(const void* X, const void* W, const float* bias,
                        void* Z, void* H, int S, int K, int N, int do_silu,
                        void* stream);
// Returns 0 after the launch, 1 for a shape the kernel does not take.
int launch_linear_silu_pair(const void* X, const LinSiluNet& net0,
                            const LinSiluNet& net1, int S, int K, int N,
                            void* stream);
void launch_silu_fwd(const void* z, void* h, long n, void* stream);
void launch_silu_bwd(const void* dh, const void* z, void* dz, long n,
                     void* stream);
void launch_silu_heads_fwd(const void* Z2, const void* Wh, const void* bh,
                           const void* Wv, const void* bv, void* H2,
                           void* heads, void* vpred, int S, int HID,
                           void* stream);
void launch_heads_bwd_silu(const void* dhead, const void* dv, const void* Wh,
                           const void* Wv, const void* Z2, void* dZ2, int S,
                           int HID, void* stream);
// Layer-2 Linear + SiLU + heads over the stacked [2, S, HID] buffers, W2 held
// in LDS. Returns 0 after the launch, 1 for a shape the kernel does not take
// (S % 128 != 0, or a HID other than 128/256: W2 at 512 does not fit in LDS).
int launch_l2_fwd_heads(const void* H1, const void* W2a, const void* b2a,
                        const void* W2c, const void* b2c, const void* Wh,
                        const void* bh, const void* Wv, const void* bv,
                        void* Z2, void* H2, void* heads, void* vpred, int S,
                        int HID, void* stream);
void launch_ppo_gather(const long* idx, int mb_size, const float* obs, int OBS,
                       int OBS_PAD, const float* action, int ACT,
                       const float* logp, const float* value, const float* adv,
                       const float* targets, void* obs_out, float* action_out,
                       float* logp_out, float* value_out, float* adv_out,
                       float* targets_out, const float* nmean,
                       const float* nvar, void* stream);
void launch_ppo_gather_disc(
    const long* idx, int mb_size, const float* obs, int OBS, int OBS_PAD,
    const long* action, const float* logp, const float* value,
    const float* adv, const float* targets, void* obs_out, long* action_out,
    float* logp_out, float* value_out, float* adv_out, float* targets_out,
    const float* nmean, const float* nvar, void* stream);
// The two gathers above for n rows at once, built for bandwidth (8 lanes per
// row, 32 rows per wave): same outputs bit for bit. OBS_PAD in {32, 64, 96,
// 128}. action / action_out are float [., ACT] (ACT 1..8), or with disc != 0
// one int64 per row. Returns 0 after the launch, 1 for a shape it does not
// take, launching nothing.
int launch_ppo_gather_rows(
    const long* idx, long n, const float* obs, int OBS, int OBS_PAD,
    const void* action, int ACT, int disc, const float* logp,
    const float* value, const float* adv, const float* targets, void* obs_out,
    void* action_out, float* logp_out, float* value_out, float* adv_out,
    float* targets_out, const float* nmean, const float* nvar, void* stream);
void launch_ppo_head_loss(
    const void* heads, const void* v_in, const float* action,
    const float* old_logp, const float* old_value, const float* adv,
    const float* targets, void* dhead, void* dv_out, void* dv16_out,
    float* metrics, int B, int ACT, float clip_eps, float ent_coef,
    float vf_coef, float min_scale, float aff_scale, float aff_shift,
    float log_aff_scale, uint64_t seed, unsigned int* draw_buf,
    unsigned int draw_offset, int do_bump, void* stream);
void launch_ppo_head_loss_disc(
    const void* heads, const void* v_in, const long* action,
    const float* old_logp, const float* old_value, const float* adv,
    const float* targets, void* dhead, void* dv_out, void* dv16_out,
    float* metrics, int B, int ACT, float clip_eps, float ent_coef,
    float vf_coef, void* stream);

// ---- per.hip
void launch_sumtree_update(float* tree, const long* idx, const float* prio,
                           long n, int cap, int depth, void* stream);
void launch_sumtree_sample(const float* tree, const float* u, long* out,
                           long n, int cap, int depth, int n_items,
                           void* stream);

// ---- rnn.hip
void launch_rnn_scan(const float* Xp, const void* Whh, const float* bhh,
                     const unsigned char* resets, const float* h0,
                     const float* c0, float* Hout, float* hT, float* cT, int T,
                     int B, int H, int lstm, void* stream);
void launch_rnn_scan_train_fwd(
    const float* Xp, const void* Whh, const float* bhh,
    const unsigned char* resets, const float* h0, const float* c0,
    float* Hout, float* hT, float* cT, float* gates, float* aux, int T, int B,
    int H, int lstm, void* stream);
void launch_rnn_scan_bwd(
    const float* dHout, const float* dhT, const float* dcT,
    const float* gates, const float* aux, const float* Hout, const float* h0,
    const float* c0, const unsigned char* resets, const void* WhhT,
    float* dXp, float* dHg, float* dh0, float* dc0, int T, int B, int H,
    int lstm, void* stream);

// ---- c51.hip
void launch_c51_loss_fwd(
    const void* logits_tm1, const float* atoms_tm1, const long* a_tm1,
    const float* r_t, const float* d_t, const void* logits_t,
    const float* atoms_t, const float* selector, float* ce, float* lse,
    float* target, int B, int A, int N, int M, int tm1_bf16, int t_bf16,
    long a_stride, long r_stride, long d_stride, void* stream);
void launch_c51_loss_bwd(const float* grad_ce, long grad_stride,
                         const void* logits_tm1, const long* a_tm1,
                         const float* lse, const float* target, void* dlogits,
                         int B, int A, int M, int is_bf16, long a_stride,
                         void* stream);

// ---- qr.hip. Null a_tm1 / sel: A == 1; null r_t and d_t together: the
// target samples are read as they are. tau_stride is the row stride of tau
// (0: one [N] for every row). Both return 0 after the launch, 1 for sizes
// the kernels do not take (1 <= N, M, Ns <= 1024, 1 <= A <= 64), launching
// nothing.
int launch_qr_loss_fwd(
    const void* src, const float* tau, const long* a_tm1, const float* r_t,
    const float* d_t, const void* sel, const void* tgt, float* loss,
    float* gth, int B, int A, int N, int M, int Ns, int src_bf16,
    int tgt_bf16, int sel_bf16, float huber_param, long tau_stride,
    long a_stride, long r_stride, long d_stride, void* stream);
int launch_qr_loss_bwd(const float* grad, long grad_stride, const float* gth,
                       const long* a_tm1, long a_stride, void* dsrc, int B,
                       int N, int A, int is_bf16, void* stream);

// ---- tanh_normal.hip. loc / scale / a / da / dloc / dscale are fp32 or bf16
// [B, A] with contiguous rows (a, da, dloc in loc's dtype, dscale in
// scale's); t may be null in the forward (not saved). The SAC row kernels
// take fp32 [Q, B] critic values, 1 <= Q <= 4; per-row vectors come with an
// element stride; log_alpha is one fp32 value in device memory. All return 0
// after the launch, 1 for sizes the kernels do not take (1 <= A <= 64),
// launching nothing. launch_sac_rows_bwd runs the critic half (g_rows set,
// g_actor null) or the actor half (the reverse).
int launch_tanh_normal_rsample_fwd(
    const void* loc, const void* scale, const float* eps, void* a, float* logp,
    float* t, int B, int A, int loc_bf16, int scale_bf16, float scale_affine,
    float shift_affine, void* stream);
int launch_tanh_normal_rsample_bwd(
    const void* da, const float* dlogp, long dlogp_stride, const float* t,
    const float* eps, const void* scale, void* dloc, void* dscale, int B,
    int A, int loc_bf16, int scale_bf16, float scale_affine, void* stream);
int launch_sac_critic_rows(
    const float* q_pred, const float* q_next, const float* logp_next,
    long lp_stride, const float* r_t, long r_stride, const float* d_t,
    long d_stride, const float* log_alpha, float gamma, float* target,
    float* rows, float* dq, int Q, int B, void* stream);
int launch_sac_actor_rows(
    const float* q_new, const float* logp_new, long lp_stride,
    const float* log_alpha, float target_entropy, float* actor_rows,
    float* alpha_rows, int* argmin, float* entropy_rows, int Q, int B,
    void* stream);
int launch_sac_rows_bwd(
    const float* g_rows, long g_rows_stride, const float* dq, float* dq_pred,
    const float* g_actor, long g_actor_stride, const float* g_alpha,
    long g_alpha_stride, const int* argmin, const float* logp_new,
    long lp_stride, const float* log_alpha, float target_entropy,
    float* dq_new, float* dlogp_new, float* dla_rows, int Q, int B,
    void* stream);

// ---- mcts.hip
void launch_mcts_select(
    const float* visit, const float* value_sum, const float* reward,
    const float* discount, const float* prior, const long* children,
    const float* min_q, const float* max_q, long* sel_parent, long* sel_action,
    int B, int N, int A, float c_puct, void* stream);
void launch_mcts_expand_backup(
    float* visit, float* value_sum, float* reward, float* discount,
    float* prior, long* children, long* parent, long* act_from_parent,
    float* min_q, float* max_q, const long* sel_parent, const long* sel_action,
    const float* reward_new, const float* discount_new, const float* prior_new,
    const float* value_new, int B, int N, int A, int new_node, void* stream);

// ---- noisy.hip. act: 0 none, 1 SiLU, 2 ReLU. noisy = 0 reads mu only. The
// three GEMM launchers return 0 after the launch, 1 for a shape the kernels
// do not take (K % 8 != 0, an empty dimension), launching nothing.
int launch_noisy_linear_fwd(
    const void* X, const float* mu_w, const float* sigma_w, const float* mu_b,
    const float* sigma_b, const float* eps_in, const float* eps_out, void* Z,
    void* H, int S, int K, int N, int x_bf16, int act, int noisy,
    void* stream);
int launch_noisy_linear_dgrad(
    const void* dZ, const float* mu_w, const float* sigma_w,
    const float* eps_in, const float* eps_out, const void* Z_prev, void* out,
    int S, int K, int N, int dz_bf16, int act_prev, int noisy, void* stream);
// Slices of S the wgrad runs with and the fp32 elements of one slab image.
void noisy_wgrad_geometry(int S, int K, int N, int* slices, int* s_per,
                          long* slab_stride);
// slab holds slices * slab_stride floats; dsigma_w / dsigma_b may be null.
int launch_noisy_linear_wgrad(
    const void* dZ, const void* X, float* slab, const float* eps_in,
    const float* eps_out, float* dmu_w, float* dsigma_w, float* dmu_b,
    float* dsigma_b, int S, int K, int N, int dz_bf16, int x_bf16,
    void* stream);
void launch_noise_transform(float* x, long n, void* stream);

// ---- qens.hip. fp32 throughout, E members (1..QENS_MAX_E). act: 0 none, 1
// SiLU, 2 ReLU. The layer input is [X0 | X1]: X0 [S, K0] with member stride
// x0_es in floats (0: one X0 for all members), X1 [S, K1] shared or null with
// K1 == 0. Outputs are rows with unit element stride, a row stride and a
// member stride in floats. All return 0 after the launch, 1 for sizes the
// kernels do not take (an empty dimension, E outside 1..4), launching nothing.
// Z: null, or written next to H (SiLU only).
int launch_qens_linear_fwd(const float* X0, long x0_es, const float* X1,
                           const QensIn& W, const QensIn& B, float* Z,
                           float* H, long out_ld, long out_es, int S, int K0,
                           int K1, int N, int E, int act, void* stream);
// dX = (dH * act'(AUX)) @ W[:, c0:c1): per member into [E, S, c1-c0], or with
// summed != 0 added over the members in ascending order into [S, c1-c0].
// AUX is the layer's H (ReLU) or Z (SiLU), [E, S, N] as dH; null for act 0.
int launch_qens_linear_dgrad(const float* dH, const float* AUX,
                             const QensIn& W, float* dX, long dx_ld,
                             long dx_es, int S, int K, int N, int c0, int c1,
                             int E, int summed, int act, void* stream);
// Slices of S the wgrad runs with and the fp32 elements of one slab image.
void qens_wgrad_geometry(int S, int K, int N, int* slices, int* s_per,
                         long* slab_stride);
// slab holds E * slices * slab_stride floats, 16-byte aligned.
int launch_qens_linear_wgrad(const float* dH, const float* AUX,
                             const float* X0, long x0_es, const float* X1,
                             float* slab, const QensOut& dW, const QensOut& dB,
                             int S, int K0, int K1, int N, int E, int act,
                             void* stream);

// ---- actor_mlp.hip. fp32 throughout. act: 1 SiLU, 2 ReLU. Eligible: 1..4
// hidden layers, each width a multiple of 16 and at most 256, K0 >= 1,
// 1 <= A <= 64, S >= 1, 16-byte aligned H / Z / dZ buffers. Both return 0
// after the launch, 1 for anything else, launching nothing.
// loc / scale [S, A]; spre [S, A] (the scale's pre-softplus value) and
// H.p[l] / Z.p[l] [S, N[l]] may be null: not stored (Z is stored for SiLU
// only).
int launch_actor_mlp_fwd(const float* X, const ActorNet& net, float min_scale,
                         int act, float* loc, float* scale, float* spre,
                         const ActorBufs& H, const ActorBufs& Z, void* stream);
// aux.p[l]: the saved H (ReLU) or Z (SiLU) of layer l. Writes dZ.p[l]
// [S, N[l]] for every hidden layer and dZh [2, S, A] = (dloc, dscale *
// softplus'(spre)).
int launch_actor_mlp_dgrad(const float* dloc, const float* dscale,
                           const float* spre, const ActorNet& net, int act,
                           const ActorBufs& aux, const ActorBufs& dZ,
                           float* dZh, void* stream);

}  // extern "C"
