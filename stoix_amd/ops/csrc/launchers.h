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

extern "C" {

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
// Returns 1 if the paired kernel ran, 0 after the per-net fallback.
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

}  // extern "C"
