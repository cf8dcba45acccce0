// Python bindings for the stoix_amd gfx950 kernels.
//
// Pure-C++ translation layer: validates torch tensors, extracts raw
// pointers + the current HIP stream, and calls the extern "C" launchers
// that launchers.h declares and the .hip files define. Every entry point
// takes the stream from PyTorch's current stream so the kernels compose with
// torch ops and with hip graph capture.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "launchers.h"

namespace {

void* cur_stream() {
  return (void*)at::hip::getCurrentHIPStream().stream();
}

#define CHK(t, ty)                                                     \
  TORCH_CHECK((t).is_cuda(), #t " must be on GPU");                    \
  TORCH_CHECK((t).is_contiguous(), #t " must be contiguous");          \
  TORCH_CHECK((t).scalar_type() == ty, #t " has wrong dtype");

// Optional operands: a tensor with no elements stands for a null pointer.
template <typename T>
T* ptr_or_null(const torch::Tensor& t) {
  return t.numel() > 0 ? t.data_ptr<T>() : nullptr;
}

float* fptr_or_null(const torch::Tensor& t) { return ptr_or_null<float>(t); }

void* vptr_or_null(const torch::Tensor& t) {
  return t.numel() > 0 ? t.data_ptr() : nullptr;
}

unsigned int* draw_or_null(const torch::Tensor& draw_buf) {
  return (unsigned int*)ptr_or_null<int>(draw_buf);
}

// cartpole_step, ant_step and humanoid_step: one wrapper, the action type
// and the launcher differ.
template <typename Action, auto Launch>
void env_step(torch::Tensor state, torch::Tensor action,
              torch::Tensor step_count, torch::Tensor ep_return,
              torch::Tensor ep_length, torch::Tensor last_ep_return,
              torch::Tensor last_ep_length, torch::Tensor obs_out,
              torch::Tensor next_obs_out, torch::Tensor reward_out,
              torch::Tensor discount_out, torch::Tensor steptype_out,
              torch::Tensor done_out, int64_t max_episode_steps, int64_t seed,
              torch::Tensor draw_buf, int64_t draw_offset, int64_t do_bump) {
  CHK(state, torch::kFloat32);
  CHK(action, c10::CppTypeToScalarType<Action>::value);
  int B = state.size(0);
  Launch(
      state.data_ptr<float>(), action.data_ptr<Action>(),
      step_count.data_ptr<int>(), ep_return.data_ptr<float>(),
      ep_length.data_ptr<int>(), last_ep_return.data_ptr<float>(),
      last_ep_length.data_ptr<int>(), obs_out.data_ptr<float>(),
      next_obs_out.data_ptr<float>(), reward_out.data_ptr<float>(),
      discount_out.data_ptr<float>(), steptype_out.data_ptr<unsigned char>(),
      done_out.data_ptr<unsigned char>(), B, (int)max_episode_steps,
      (uint64_t)seed, (unsigned int*)draw_buf.data_ptr<int>(),
      (unsigned int)draw_offset, (int)do_bump, cur_stream());
}

void ant_reset(torch::Tensor state, int64_t seed, int64_t draw) {
  CHK(state, torch::kFloat32);
  launch_ant_reset(state.data_ptr<float>(), state.size(0), (uint64_t)seed,
                   (uint32_t)draw, cur_stream());
}

// The scan kernels index every operand as r_t's contiguous [T, B] matrix, so
// each one has to be exactly that: on r_t's device, contiguous, of the
// kernel's dtype and of r_t's shape. T * B is an int in the kernels.
void scan_shape_check(const torch::Tensor& r_t) {
  CHK(r_t, torch::kFloat32);
  TORCH_CHECK(r_t.dim() == 2 && r_t.size(0) >= 1 && r_t.size(1) >= 1,
              "scan: r_t must be a non-empty [T, B] matrix, got ", r_t.sizes());
  TORCH_CHECK(r_t.numel() < (int64_t(1) << 31), "scan: T * B must fit an int");
}

void scan_operand_check(const torch::Tensor& t, const torch::Tensor& r_t,
                        const char* name,
                        torch::ScalarType ty = torch::kFloat32) {
  TORCH_CHECK(t.is_cuda() && t.device() == r_t.device(), "scan: ", name,
              " must be on r_t's GPU");
  TORCH_CHECK(t.is_contiguous(), "scan: ", name, " must be contiguous");
  TORCH_CHECK(t.scalar_type() == ty, "scan: ", name, " must be ", ty);
  TORCH_CHECK(t.sizes() == r_t.sizes(), "scan: ", name, " has shape ",
              t.sizes(), ", r_t has ", r_t.sizes());
}

void gae(torch::Tensor r_t, torch::Tensor discount_t, torch::Tensor v_tm1,
         torch::Tensor v_t, torch::Tensor trunc_t, torch::Tensor adv_out,
         torch::Tensor target_out, double lambda_) {
  scan_shape_check(r_t);
  scan_operand_check(discount_t, r_t, "discount_t");
  scan_operand_check(v_tm1, r_t, "v_tm1");
  scan_operand_check(v_t, r_t, "v_t");
  scan_operand_check(adv_out, r_t, "adv_out");
  scan_operand_check(target_out, r_t, "target_out");
  if (trunc_t.numel() > 0)
    scan_operand_check(trunc_t, r_t, "trunc_t", torch::kUInt8);
  int T = r_t.size(0), B = r_t.size(1);
  launch_gae(r_t.data_ptr<float>(), discount_t.data_ptr<float>(),
             v_tm1.data_ptr<float>(), v_t.data_ptr<float>(),
             ptr_or_null<unsigned char>(trunc_t),
             adv_out.data_ptr<float>(), target_out.data_ptr<float>(), T, B,
             (float)lambda_, cur_stream());
}

void lambda_returns(torch::Tensor r_t, torch::Tensor discount_t,
                    torch::Tensor v_t, torch::Tensor out, double lambda_) {
  scan_shape_check(r_t);
  scan_operand_check(discount_t, r_t, "discount_t");
  scan_operand_check(v_t, r_t, "v_t");
  scan_operand_check(out, r_t, "out");
  launch_lambda_returns(r_t.data_ptr<float>(), discount_t.data_ptr<float>(),
                        v_t.data_ptr<float>(), out.data_ptr<float>(),
                        r_t.size(0), r_t.size(1), (float)lambda_,
                        cur_stream());
}

void vtrace(torch::Tensor v_tm1, torch::Tensor v_t, torch::Tensor r_t,
            torch::Tensor discount_t, torch::Tensor rho_tm1,
            torch::Tensor errors_out, torch::Tensor pg_adv_out, double lambda_,
            double clip_rho, double clip_pg_rho) {
  scan_shape_check(r_t);
  scan_operand_check(v_tm1, r_t, "v_tm1");
  scan_operand_check(v_t, r_t, "v_t");
  scan_operand_check(discount_t, r_t, "discount_t");
  scan_operand_check(rho_tm1, r_t, "rho_tm1");
  scan_operand_check(errors_out, r_t, "errors_out");
  scan_operand_check(pg_adv_out, r_t, "pg_adv_out");
  launch_vtrace(v_tm1.data_ptr<float>(), v_t.data_ptr<float>(),
                r_t.data_ptr<float>(), discount_t.data_ptr<float>(),
                rho_tm1.data_ptr<float>(), errors_out.data_ptr<float>(),
                pg_adv_out.data_ptr<float>(), r_t.size(0), r_t.size(1),
                (float)lambda_, (float)clip_rho, (float)clip_pg_rho,
                cur_stream());
}

void offpolicy_returns(torch::Tensor q_t, torch::Tensor v_t, torch::Tensor r_t,
                       torch::Tensor discount_t, torch::Tensor c_t,
                       torch::Tensor out) {
  scan_shape_check(r_t);
  scan_operand_check(q_t, r_t, "q_t");
  scan_operand_check(v_t, r_t, "v_t");
  scan_operand_check(discount_t, r_t, "discount_t");
  scan_operand_check(c_t, r_t, "c_t");
  scan_operand_check(out, r_t, "out");
  launch_offpolicy_returns(q_t.data_ptr<float>(), v_t.data_ptr<float>(),
                           r_t.data_ptr<float>(), discount_t.data_ptr<float>(),
                           c_t.data_ptr<float>(), out.data_ptr<float>(),
                           r_t.size(0), r_t.size(1), cur_stream());
}

void fused_adam(torch::Tensor param, torch::Tensor grad, torch::Tensor exp_avg,
                torch::Tensor exp_avg_sq, torch::Tensor sqnorm,
                torch::Tensor step_t, double lr, double beta1, double beta2,
                double eps, double max_norm) {
  CHK(param, torch::kFloat32);
  CHK(grad, torch::kFloat32);
  launch_fused_adam(param.data_ptr<float>(), grad.data_ptr<float>(),
                    exp_avg.data_ptr<float>(), exp_avg_sq.data_ptr<float>(),
                    sqnorm.data_ptr<float>(), step_t.data_ptr<long>(),
                    param.numel(), (float)lr, (float)beta1, (float)beta2,
                    (float)eps, (float)max_norm, cur_stream());
}

void polyak(torch::Tensor online, torch::Tensor target, double tau) {
  CHK(online, torch::kFloat32);
  launch_polyak(online.data_ptr<float>(), target.data_ptr<float>(),
                online.numel(), (float)tau, cur_stream());
}

void fused_adam_bf16(torch::Tensor param, torch::Tensor grad,
                     torch::Tensor exp_avg, torch::Tensor exp_avg_sq,
                     torch::Tensor sqnorm, torch::Tensor step_t,
                     torch::Tensor param_bf16, double lr, double beta1,
                     double beta2, double eps, double max_norm,
                     double grad_scale, int64_t do_prologue) {
  CHK(param, torch::kFloat32);
  CHK(grad, torch::kBFloat16);
  launch_fused_adam_bf16(param.data_ptr<float>(), grad.data_ptr(),
                         exp_avg.data_ptr<float>(),
                         exp_avg_sq.data_ptr<float>(),
                         sqnorm.data_ptr<float>(), step_t.data_ptr<long>(),
                         vptr_or_null(param_bf16), param.numel(), (float)lr,
                         (float)beta1,
                         (float)beta2, (float)eps, (float)max_norm,
                         (float)grad_scale, (int)do_prologue,
                         (long)sqnorm.numel(), cur_stream());
}

void mfma_probe(torch::Tensor A, torch::Tensor B, torch::Tensor D0,
                torch::Tensor D1) {
  CHK(A, torch::kBFloat16);
  launch_mfma_probe(A.data_ptr(), B.data_ptr(), D0.data_ptr<float>(),
                    D1.data_ptr<float>(), cur_stream());
}

// A fused-MLP weight (mlp.hip): contiguous bf16 on the GPU, `rows` x `cols`.
void check_fused_weight(const torch::Tensor& w, const char* name,
                        int64_t rows, int64_t cols) {
  TORCH_CHECK(w.is_cuda() && w.is_contiguous() &&
                  w.scalar_type() == torch::kBFloat16,
              name, " must be a contiguous bf16 GPU tensor");
  TORCH_CHECK(w.numel() == rows * cols && w.size(0) == rows, name,
              " must be [", rows, ", ", cols, "]");
}

// Argument checks shared by the fused-MLP wrappers (mlp.hip). The kernels
// exist for HID 128/256/512 only (HID = rows of the critic's W2), stage at
// most 128 obs columns and read W1 with the obs width padded to the MFMA
// K-step. Returns HID.
int check_fused_mlp(const torch::Tensor& obs, const torch::Tensor& W1c,
                    const torch::Tensor& W2c, const torch::Tensor& Wvc) {
  CHK(obs, torch::kFloat32);
  const int64_t HID = W2c.size(0), OBS = obs.size(1);
  TORCH_CHECK(HID == 512 || HID == 256 || HID == 128,
              "fused MLP supports HID 128/256/512, got ", HID);
  TORCH_CHECK(OBS <= 128, "fused MLP supports OBS <= 128, got ", OBS);
  check_fused_weight(W1c, "W1c", HID, (OBS + 31) & ~31);
  check_fused_weight(W2c, "W2c", HID, HID);
  check_fused_weight(Wvc.view({-1, 1}), "Wvc", HID, 1);
  return (int)HID;
}

// The same with an actor of the same width, whose head is one 16-column
// tile holding at most `act_max` actions (8 tanh-normal dims or 16 logits).
int check_fused_mlp(const torch::Tensor& obs, const torch::Tensor& W1a,
                    const torch::Tensor& W2a, const torch::Tensor& Wha,
                    const torch::Tensor& W1c, const torch::Tensor& W2c,
                    const torch::Tensor& Wvc, int64_t ACT, int64_t act_max) {
  const int HID = check_fused_mlp(obs, W1c, W2c, Wvc);
  check_fused_weight(W1a, "W1a", HID, W1c.size(1));
  check_fused_weight(W2a, "W2a", HID, HID);
  check_fused_weight(Wha, "Wha", 16, HID);
  TORCH_CHECK(ACT <= act_max, "fused policy head supports ACT <= ", act_max,
              ", got ", ACT);
  return HID;
}

void policy_value_step(torch::Tensor obs, torch::Tensor W1a, torch::Tensor b1a,
                       torch::Tensor W2a, torch::Tensor b2a, torch::Tensor Wha,
                       torch::Tensor bha, torch::Tensor W1c, torch::Tensor b1c,
                       torch::Tensor W2c, torch::Tensor b2c, torch::Tensor Wvc,
                       torch::Tensor bvc, torch::Tensor obs_mirror,
                       torch::Tensor action_out, torch::Tensor logp_out,
                       torch::Tensor value_out, torch::Tensor nmean,
                       torch::Tensor nvar, double min_scale, double aff_scale,
                       double aff_shift, double log_aff_scale, int64_t greedy,
                       int64_t seed, torch::Tensor draw_buf,
                       int64_t draw_offset, int64_t do_bump) {
  int B = obs.size(0), OBS = obs.size(1);
  int ACT = action_out.size(1);
  int HID = check_fused_mlp(obs, W1a, W2a, Wha, W1c, W2c, Wvc, ACT, 8);
  launch_policy_value_step(
      obs.data_ptr<float>(), W1a.data_ptr(), b1a.data_ptr<float>(),
      W2a.data_ptr(), b2a.data_ptr<float>(), Wha.data_ptr(),
      bha.data_ptr<float>(), W1c.data_ptr(), b1c.data_ptr<float>(),
      W2c.data_ptr(), b2c.data_ptr<float>(), Wvc.data_ptr(),
      bvc.data_ptr<float>(), fptr_or_null(obs_mirror),
      action_out.data_ptr<float>(), logp_out.data_ptr<float>(),
      value_out.data_ptr<float>(), fptr_or_null(nmean), fptr_or_null(nvar), B,
      OBS, ACT, HID, (float)min_scale, (float)aff_scale, (float)aff_shift,
      (float)log_aff_scale, (int)greedy, (uint64_t)seed,
      draw_or_null(draw_buf), (unsigned int)draw_offset, (int)do_bump,
      cur_stream());
}

void policy_value_step_disc(
    torch::Tensor obs, torch::Tensor W1a, torch::Tensor b1a,
    torch::Tensor W2a, torch::Tensor b2a, torch::Tensor Wha,
    torch::Tensor bha, torch::Tensor W1c, torch::Tensor b1c,
    torch::Tensor W2c, torch::Tensor b2c, torch::Tensor Wvc,
    torch::Tensor bvc, torch::Tensor obs_mirror, torch::Tensor action_out,
    torch::Tensor logp_out, torch::Tensor value_out, torch::Tensor nmean,
    torch::Tensor nvar, int64_t num_actions, int64_t greedy, int64_t seed,
    torch::Tensor draw_buf, int64_t draw_offset, int64_t do_bump) {
  CHK(action_out, torch::kInt64);
  int B = obs.size(0), OBS = obs.size(1);
  int ACT = (int)num_actions;
  int HID = check_fused_mlp(obs, W1a, W2a, Wha, W1c, W2c, Wvc, ACT, 16);
  launch_policy_value_step_disc(
      obs.data_ptr<float>(), W1a.data_ptr(), b1a.data_ptr<float>(),
      W2a.data_ptr(), b2a.data_ptr<float>(), Wha.data_ptr(),
      bha.data_ptr<float>(), W1c.data_ptr(), b1c.data_ptr<float>(),
      W2c.data_ptr(), b2c.data_ptr<float>(), Wvc.data_ptr(),
      bvc.data_ptr<float>(), fptr_or_null(obs_mirror),
      action_out.data_ptr<long>(), logp_out.data_ptr<float>(),
      value_out.data_ptr<float>(), fptr_or_null(nmean), fptr_or_null(nvar), B,
      OBS, ACT, HID, (int)greedy,
      (uint64_t)seed, draw_or_null(draw_buf), (unsigned int)draw_offset,
      (int)do_bump, cur_stream());
}

void ppo_head_loss_disc(torch::Tensor heads, torch::Tensor v_in,
                        torch::Tensor action, torch::Tensor old_logp,
                        torch::Tensor old_value, torch::Tensor adv,
                        torch::Tensor targets, torch::Tensor dhead,
                        torch::Tensor dv, torch::Tensor dv16,
                        torch::Tensor metrics, int64_t num_actions,
                        double clip_eps, double ent_coef, double vf_coef) {
  CHK(heads, torch::kBFloat16);
  CHK(action, torch::kInt64);
  int B = heads.size(0);
  launch_ppo_head_loss_disc(
      heads.data_ptr(), v_in.data_ptr(), action.data_ptr<long>(),
      old_logp.data_ptr<float>(), old_value.data_ptr<float>(),
      adv.data_ptr<float>(), targets.data_ptr<float>(), dhead.data_ptr(),
      dv.data_ptr(), vptr_or_null(dv16), fptr_or_null(metrics), B,
      (int)num_actions, (float)clip_eps, (float)ent_coef, (float)vf_coef,
      cur_stream());
}

void ppo_gather_disc(torch::Tensor idx, torch::Tensor obs,
                     torch::Tensor action, torch::Tensor logp,
                     torch::Tensor value, torch::Tensor adv,
                     torch::Tensor targets, torch::Tensor obs_out,
                     torch::Tensor action_out, torch::Tensor logp_out,
                     torch::Tensor value_out, torch::Tensor adv_out,
                     torch::Tensor targets_out, torch::Tensor nmean,
                     torch::Tensor nvar) {
  CHK(idx, torch::kInt64);
  CHK(obs, torch::kFloat32);
  CHK(obs_out, torch::kBFloat16);
  CHK(action, torch::kInt64);
  int mb = idx.numel();
  launch_ppo_gather_disc(
      idx.data_ptr<long>(), mb, obs.data_ptr<float>(), obs.size(1),
      obs_out.size(1), action.data_ptr<long>(), logp.data_ptr<float>(),
      value.data_ptr<float>(), adv.data_ptr<float>(),
      targets.data_ptr<float>(), obs_out.data_ptr(),
      action_out.data_ptr<long>(), logp_out.data_ptr<float>(),
      value_out.data_ptr<float>(), adv_out.data_ptr<float>(),
      targets_out.data_ptr<float>(), fptr_or_null(nmean), fptr_or_null(nvar),
      cur_stream());
}

void value_forward(torch::Tensor obs, torch::Tensor W1c, torch::Tensor b1c,
                   torch::Tensor W2c, torch::Tensor b2c, torch::Tensor Wvc,
                   torch::Tensor bvc, torch::Tensor value_out,
                   torch::Tensor nmean, torch::Tensor nvar) {
  int B = obs.size(0), OBS = obs.size(1);
  int HID = check_fused_mlp(obs, W1c, W2c, Wvc);
  launch_value_forward(obs.data_ptr<float>(), W1c.data_ptr(),
                       b1c.data_ptr<float>(), W2c.data_ptr(),
                       b2c.data_ptr<float>(), Wvc.data_ptr(),
                       bvc.data_ptr<float>(), value_out.data_ptr<float>(),
                       fptr_or_null(nmean), fptr_or_null(nvar), B, OBS, HID,
                       cur_stream());
}

void rollout_step_ant(torch::Tensor obs_io, torch::Tensor env_state,
                      torch::Tensor step_count, torch::Tensor ep_return,
                      torch::Tensor ep_length, torch::Tensor last_ep_return,
                      torch::Tensor last_ep_length, torch::Tensor W1a,
                      torch::Tensor b1a, torch::Tensor W2a, torch::Tensor b2a,
                      torch::Tensor Wha, torch::Tensor bha, torch::Tensor W1c,
                      torch::Tensor b1c, torch::Tensor W2c, torch::Tensor b2c,
                      torch::Tensor Wvc, torch::Tensor bvc,
                      torch::Tensor buf_obs, torch::Tensor buf_action,
                      torch::Tensor buf_logp, torch::Tensor buf_value,
                      torch::Tensor buf_bootstrap, torch::Tensor buf_reward,
                      torch::Tensor buf_discount, torch::Tensor buf_steptype,
                      int64_t max_episode_steps, double min_scale,
                      double aff_scale, double aff_shift,
                      double log_aff_scale, int64_t policy_seed,
                      int64_t env_seed, torch::Tensor policy_draw,
                      torch::Tensor env_draw, int64_t draw_offset) {
  CHK(env_state, torch::kFloat32);
  int B = obs_io.size(0), OBS = obs_io.size(1), ACT = buf_action.size(1);
  int HID =
      check_fused_mlp(obs_io, W1a, W2a, Wha, W1c, W2c, Wvc, ACT, 8);
  // the megakernel hard-codes the Ant's shapes (ant_core.h)
  TORCH_CHECK(OBS == 27 && ACT == 8,
              "rollout_step_ant needs OBS == 27 and ACT == 8, got ", OBS,
              " and ", ACT);
  launch_rollout_step_ant(
      obs_io.data_ptr<float>(), env_state.data_ptr<float>(),
      step_count.data_ptr<int>(), ep_return.data_ptr<float>(),
      ep_length.data_ptr<int>(), last_ep_return.data_ptr<float>(),
      last_ep_length.data_ptr<int>(), W1a.data_ptr(), b1a.data_ptr<float>(),
      W2a.data_ptr(), b2a.data_ptr<float>(), Wha.data_ptr(),
      bha.data_ptr<float>(), W1c.data_ptr(), b1c.data_ptr<float>(),
      W2c.data_ptr(), b2c.data_ptr<float>(), Wvc.data_ptr(),
      bvc.data_ptr<float>(), buf_obs.data_ptr<float>(),
      buf_action.data_ptr<float>(), buf_logp.data_ptr<float>(),
      buf_value.data_ptr<float>(), buf_bootstrap.data_ptr<float>(),
      buf_reward.data_ptr<float>(), buf_discount.data_ptr<float>(),
      buf_steptype.data_ptr<unsigned char>(), B, OBS, ACT, HID,
      (int)max_episode_steps, (float)min_scale, (float)aff_scale,
      (float)aff_shift, (float)log_aff_scale, (uint64_t)policy_seed,
      (uint64_t)env_seed, (unsigned int*)policy_draw.data_ptr<int>(),
      (unsigned int*)env_draw.data_ptr<int>(), (unsigned int)draw_offset,
      cur_stream());
}

void linear_silu(torch::Tensor X, torch::Tensor W, torch::Tensor bias,
                 torch::Tensor Z, torch::Tensor H, int64_t do_silu) {
  CHK(X, torch::kBFloat16);
  CHK(W, torch::kBFloat16);
  CHK(bias, torch::kFloat32);
  int S = X.size(0), K = X.size(1), N = W.size(0);
  TORCH_CHECK(S % 128 == 0 && N % 128 == 0 && K % 32 == 0,
              "linear_silu tile constraints");
  launch_linear_silu(X.data_ptr(), W.data_ptr(), bias.data_ptr<float>(),
                     Z.data_ptr(), vptr_or_null(H), S, K, N, (int)do_silu,
                     cur_stream());
}

// Both nets' layer-1 Linear+SiLU in one launch over a shared X. Returns
// false, with nothing launched, for a shape the paired kernel does not take
// (S or N not a multiple of 128): the caller then runs linear_silu per net.
bool linear_silu_pair(torch::Tensor X, torch::Tensor W_a, torch::Tensor b_a,
                      torch::Tensor Z_a, torch::Tensor H_a, torch::Tensor W_c,
                      torch::Tensor b_c, torch::Tensor Z_c,
                      torch::Tensor H_c) {
  CHK(X, torch::kBFloat16);
  CHK(W_a, torch::kBFloat16);
  CHK(W_c, torch::kBFloat16);
  CHK(b_a, torch::kFloat32);
  CHK(b_c, torch::kFloat32);
  CHK(Z_a, torch::kBFloat16);
  CHK(H_a, torch::kBFloat16);
  CHK(Z_c, torch::kBFloat16);
  CHK(H_c, torch::kBFloat16);
  TORCH_CHECK(X.dim() == 2 && W_a.dim() == 2 && W_c.dim() == 2,
              "linear_silu_pair: X and W must be 2-D");
  const int64_t S = X.size(0), K = X.size(1), N = W_a.size(0);
  TORCH_CHECK(W_a.size(1) == K && W_c.size(0) == N && W_c.size(1) == K,
              "linear_silu_pair: the two nets' weight shapes differ");
  TORCH_CHECK(b_a.numel() == N && b_c.numel() == N,
              "linear_silu_pair: bias length");
  TORCH_CHECK(Z_a.numel() == S * N && H_a.numel() == S * N &&
                  Z_c.numel() == S * N && H_c.numel() == S * N,
              "linear_silu_pair: outputs must hold S * N elements");
  TORCH_CHECK(K > 0 && K % 32 == 0,
              "linear_silu_pair: K must be a multiple of 32");
  for (const torch::Tensor* t : {&X, &W_a, &W_c, &Z_a, &H_a, &Z_c, &H_c})
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0,
                "linear_silu_pair: operands must be 16-byte aligned");
  const LinSiluNet na{W_a.data_ptr(), b_a.data_ptr<float>(), Z_a.data_ptr(),
                      H_a.data_ptr()};
  const LinSiluNet nc{W_c.data_ptr(), b_c.data_ptr<float>(), Z_c.data_ptr(),
                      H_c.data_ptr()};
  return launch_linear_silu_pair(X.data_ptr(), na, nc, (int)S, (int)K, (int)N,
                                 cur_stream()) == 0;
}

void silu_fwd(torch::Tensor z, torch::Tensor h) {
  CHK(z, torch::kBFloat16);
  TORCH_CHECK(z.numel() % 8 == 0, "silu_fwd needs numel % 8 == 0");
  launch_silu_fwd(z.data_ptr(), h.data_ptr(), z.numel(), cur_stream());
}

void silu_bwd(torch::Tensor dh, torch::Tensor z, torch::Tensor dz) {
  CHK(z, torch::kBFloat16);
  TORCH_CHECK(z.numel() % 8 == 0, "silu_bwd needs numel % 8 == 0");
  launch_silu_bwd(dh.data_ptr(), z.data_ptr(), dz.data_ptr(), z.numel(),
                  cur_stream());
}

// Shape checks shared by the two fused head kernels over the stacked
// [2, S, HID] buffers. `rows1` may be empty where it is optional. Returns
// S; HID comes back through `hid`.
int check_stacked_heads(const torch::Tensor& Z2, const torch::Tensor& other,
                        const torch::Tensor& Wh, const torch::Tensor& Wv,
                        const torch::Tensor& rows16, const torch::Tensor& rows1,
                        bool rows1_optional, int* hid) {
  CHK(Z2, torch::kBFloat16);
  CHK(other, torch::kBFloat16);
  CHK(rows16, torch::kBFloat16);
  CHK(rows1, torch::kBFloat16);
  TORCH_CHECK(Z2.dim() == 3 && Z2.size(0) == 2,
              "fused heads need stacked [2, S, HID] buffers");
  const int64_t S = Z2.size(1), HID = Z2.size(2);
  TORCH_CHECK(HID == 512 || HID == 256 || HID == 128,
              "fused heads support HID 128/256/512, got ", HID);
  TORCH_CHECK(S % 16 == 0, "fused heads need S % 16 == 0, got ", S);
  TORCH_CHECK(other.sizes() == Z2.sizes(),
              "fused heads: [2, S, HID] buffers differ in shape");
  check_fused_weight(Wh, "Wh", 16, HID);
  check_fused_weight(Wv.view({-1, 1}), "Wv", HID, 1);
  TORCH_CHECK(rows16.numel() == S * 16, "fused heads: expected [S, 16]");
  TORCH_CHECK(rows1.numel() == S || (rows1_optional && rows1.numel() == 0),
              "fused heads: expected [S]");
  *hid = (int)HID;
  return (int)S;
}

void silu_heads_fwd(torch::Tensor Z2, torch::Tensor Wh, torch::Tensor bh,
                    torch::Tensor Wv, torch::Tensor bv, torch::Tensor H2,
                    torch::Tensor heads, torch::Tensor vpred) {
  int HID;
  // an empty vpred leaves the value head to the caller (critic: silu only)
  int S = check_stacked_heads(Z2, H2, Wh, Wv, heads, vpred, true, &HID);
  CHK(bh, torch::kBFloat16);
  CHK(bv, torch::kBFloat16);
  TORCH_CHECK(bh.numel() == 16 && bv.numel() == 1,
              "silu_heads_fwd: bh must be [16] and bv [1]");
  launch_silu_heads_fwd(Z2.data_ptr(), Wh.data_ptr(), bh.data_ptr(),
                        Wv.data_ptr(), bv.data_ptr(), H2.data_ptr(),
                        heads.data_ptr(),
                        vptr_or_null(vpred), S,
                        HID, cur_stream());
}

// Layer-2 Linear + SiLU + heads of both nets in one launch, over the stacked
// [2, S, HID] buffers: Z2 = H1 @ W2^T + b2 (bf16 mirror biases), H2 =
// silu(Z2), heads and, with a non-empty vpred, the value head, as
// silu_heads_fwd forms them. Returns false, with nothing launched, for a
// shape the kernel does not take (S % 128 != 0, HID not 128/256): the caller
// then runs the GEMMs and silu_heads_fwd.
bool linear_silu_heads_pair(torch::Tensor H1, torch::Tensor W2a,
                            torch::Tensor b2a, torch::Tensor W2c,
                            torch::Tensor b2c, torch::Tensor Wh,
                            torch::Tensor bh, torch::Tensor Wv,
                            torch::Tensor bv, torch::Tensor Z2,
                            torch::Tensor H2, torch::Tensor heads,
                            torch::Tensor vpred) {
  for (const torch::Tensor* t : {&H1, &b2a, &b2c, &bh, &bv, &Z2, &H2, &heads})
    TORCH_CHECK(t->is_cuda() && t->is_contiguous() &&
                    t->scalar_type() == torch::kBFloat16,
                "linear_silu_heads_pair: contiguous bf16 GPU tensors expected");
  TORCH_CHECK(H1.dim() == 3 && H1.size(0) == 2,
              "linear_silu_heads_pair needs stacked [2, S, HID] buffers");
  const int64_t S = H1.size(1), HID = H1.size(2);
  TORCH_CHECK(Z2.sizes() == H1.sizes() && H2.sizes() == H1.sizes(),
              "linear_silu_heads_pair: [2, S, HID] buffers differ in shape");
  check_fused_weight(W2a, "W2a", HID, HID);
  check_fused_weight(W2c, "W2c", HID, HID);
  check_fused_weight(Wh, "Wh", 16, HID);
  check_fused_weight(Wv.view({-1, 1}), "Wv", HID, 1);
  TORCH_CHECK(b2a.numel() == HID && b2c.numel() == HID && bh.numel() == 16 &&
                  bv.numel() == 1,
              "linear_silu_heads_pair: b2 must be [HID], bh [16] and bv [1]");
  TORCH_CHECK(heads.numel() == S * 16, "linear_silu_heads_pair: heads [S, 16]");
  if (vpred.numel() > 0) {
    CHK(vpred, torch::kBFloat16);
    TORCH_CHECK(vpred.numel() == S, "linear_silu_heads_pair: vpred [S]");
  }
  for (const torch::Tensor* t : {&H1, &W2a, &b2a, &W2c, &b2c, &Wh, &Wv, &Z2,
                                 &H2, &heads})
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0,
                "linear_silu_heads_pair: operands must be 16-byte aligned");
  return launch_l2_fwd_heads(H1.data_ptr(), W2a.data_ptr(), b2a.data_ptr(),
                             W2c.data_ptr(), b2c.data_ptr(), Wh.data_ptr(),
                             bh.data_ptr(), Wv.data_ptr(), bv.data_ptr(),
                             Z2.data_ptr(), H2.data_ptr(), heads.data_ptr(),
                             vptr_or_null(vpred), (int)S, (int)HID,
                             cur_stream()) == 0;
}

void heads_bwd_silu(torch::Tensor dhead, torch::Tensor dv, torch::Tensor Wh,
                    torch::Tensor Wv, torch::Tensor Z2, torch::Tensor dZ2) {
  int HID;
  int S = check_stacked_heads(Z2, dZ2, Wh, Wv, dhead, dv, false, &HID);
  launch_heads_bwd_silu(dhead.data_ptr(), dv.data_ptr(), Wh.data_ptr(),
                        Wv.data_ptr(), Z2.data_ptr(), dZ2.data_ptr(), S, HID,
                        cur_stream());
}

void ppo_gather(torch::Tensor idx, torch::Tensor obs, torch::Tensor action,
                torch::Tensor logp, torch::Tensor value, torch::Tensor adv,
                torch::Tensor targets, torch::Tensor obs_out,
                torch::Tensor action_out, torch::Tensor logp_out,
                torch::Tensor value_out, torch::Tensor adv_out,
                torch::Tensor targets_out, torch::Tensor nmean,
                torch::Tensor nvar) {
  CHK(idx, torch::kInt64);
  CHK(obs, torch::kFloat32);
  CHK(obs_out, torch::kBFloat16);
  int mb = idx.numel();
  launch_ppo_gather(idx.data_ptr<long>(), mb, obs.data_ptr<float>(),
                    obs.size(1), obs_out.size(1), action.data_ptr<float>(),
                    action.size(1),
                    logp.data_ptr<float>(), value.data_ptr<float>(),
                    adv.data_ptr<float>(), targets.data_ptr<float>(),
                    obs_out.data_ptr(), action_out.data_ptr<float>(),
                    logp_out.data_ptr<float>(), value_out.data_ptr<float>(),
                    adv_out.data_ptr<float>(), targets_out.data_ptr<float>(),
                    fptr_or_null(nmean), fptr_or_null(nvar), cur_stream());
}

void ppo_head_loss(torch::Tensor heads, torch::Tensor v_in,
                   torch::Tensor action, torch::Tensor old_logp,
                   torch::Tensor old_value, torch::Tensor adv,
                   torch::Tensor targets, torch::Tensor dhead,
                   torch::Tensor dv, torch::Tensor dv16,
                   torch::Tensor metrics, double clip_eps,
                   double ent_coef, double vf_coef, double min_scale,
                   double aff_scale, double aff_shift, double log_aff_scale,
                   int64_t seed, torch::Tensor draw_buf, int64_t draw_offset,
                   int64_t do_bump) {
  CHK(heads, torch::kBFloat16);
  CHK(v_in, torch::kBFloat16);
  CHK(action, torch::kFloat32);
  int B = heads.size(0), ACT = action.size(1);
  TORCH_CHECK(heads.size(1) == 16, "heads must be [B,16] (loc|scale packed)");
  launch_ppo_head_loss(
      heads.data_ptr(), v_in.data_ptr(), action.data_ptr<float>(),
      old_logp.data_ptr<float>(), old_value.data_ptr<float>(),
      adv.data_ptr<float>(), targets.data_ptr<float>(), dhead.data_ptr(),
      dv.data_ptr(), vptr_or_null(dv16), fptr_or_null(metrics), B, ACT,
      (float)clip_eps, (float)ent_coef, (float)vf_coef, (float)min_scale,
      (float)aff_scale, (float)aff_shift, (float)log_aff_scale, (uint64_t)seed,
      draw_or_null(draw_buf), (unsigned int)draw_offset, (int)do_bump,
      cur_stream());
}

// One net's operands for wgrad() / wgrad_pair() (wgrad.hip): dZ [S, N_STRIDE]
// and X [S, K] in bf16, and the dW [n_valid, K] and db [n_valid] ranges
// inside one image of the [>= 64, stride] fp32 slab. S is dZ's row count for
// wgrad(), net 0's for wgrad_pair().
WgradNet check_wgrad_net(const char* op, const torch::Tensor& dZ,
                         const torch::Tensor& X, const torch::Tensor& slab,
                         int64_t dW_off, int64_t db_off, int64_t n_valid,
                         int64_t S) {
  CHK(dZ, torch::kBFloat16);
  CHK(X, torch::kBFloat16);
  CHK(slab, torch::kFloat32);
  TORCH_CHECK(dZ.dim() == 2 && X.dim() == 2, op, ": operands must be 2-D");
  TORCH_CHECK(dZ.size(0) == S && X.size(0) == S, op, ": dZ/X row mismatch");
  TORCH_CHECK(S % (4 * 32) == 0, op, ": S must be a multiple of 128");
  const int64_t K = X.size(1);
  TORCH_CHECK(n_valid >= 1 && n_valid <= dZ.size(1), op,
              ": n_valid must be in [1, dZ width]");
  TORCH_CHECK(slab.dim() == 2 && slab.size(0) >= 64, op,
              ": slab must be [>=64, stride]");
  TORCH_CHECK(dW_off >= 0 && dW_off + n_valid * K <= slab.size(1), op,
              ": dW range outside the slab");
  TORCH_CHECK(db_off < 0 || db_off + n_valid <= slab.size(1), op,
              ": db range outside the slab");
  return {dZ.data_ptr(), X.data_ptr(), slab.data_ptr<float>(), (long)dW_off,
          (long)db_off, (long)slab.size(1), (int)n_valid};
}

void wgrad(torch::Tensor dZ, torch::Tensor X, torch::Tensor slab,
           int64_t dW_off, int64_t db_off, int64_t n_valid,
           int64_t kpg = 0, int64_t ntb = 0) {
  const int64_t S = dZ.dim() == 2 ? dZ.size(0) : -1;
  const WgradNet n =
      check_wgrad_net("wgrad", dZ, X, slab, dW_off, db_off, n_valid, S);
  launch_wgrad(n.dZ, n.X, n.slab, n.dW_off, n.db_off, n.slab_stride, (int)S,
               (int)dZ.size(1), (int)X.size(1), n.N_VALID, (int)kpg, (int)ntb,
               cur_stream());
}

// Both nets' dW = dZ^T @ X and db = colsum(dZ) in one launch of the
// pipelined kernel (wgrad.hip); bit-equal to two wgrad() calls. Returns true
// if the paired kernel covered the shape, false if the launcher fell back to
// the old kernels.
bool wgrad_pair(torch::Tensor dZ0, torch::Tensor X0, torch::Tensor slab0,
                int64_t dW_off0, int64_t db_off0, int64_t n_valid0,
                torch::Tensor dZ1, torch::Tensor X1, torch::Tensor slab1,
                int64_t dW_off1, int64_t db_off1, int64_t n_valid1,
                int64_t variant = -1) {
  const char* op = "wgrad_pair";
  const int64_t S = dZ0.dim() == 2 ? dZ0.size(0) : -1;
  const WgradNet n0 =
      check_wgrad_net(op, dZ0, X0, slab0, dW_off0, db_off0, n_valid0, S);
  const WgradNet n1 =
      check_wgrad_net(op, dZ1, X1, slab1, dW_off1, db_off1, n_valid1, S);
  const int64_t N_STRIDE = dZ0.size(1), K = X0.size(1);
  TORCH_CHECK(dZ1.size(1) == N_STRIDE && X1.size(1) == K,
              "wgrad_pair: the two nets' operand widths differ");
  TORCH_CHECK(K % 32 == 0, "wgrad_pair: K must be a multiple of 32");
  TORCH_CHECK(N_STRIDE % 16 == 0,
              "wgrad_pair: dZ width must be a multiple of 16");
  return launch_wgrad_pair(n0, n1, (int)S, (int)N_STRIDE, (int)K, (int)variant,
                           cur_stream()) != 0;
}

// Layer-1 wgrad_pair with the SiLU backward inside: a net's operand is
// dH * silu'(Z), formed while the kernel stages the tile, so neither the
// silu_bwd launch nor the dZ buffer is needed. Bit-equal to silu_bwd +
// wgrad_pair. Returns true after the launch; false = not taken (a Z on one
// net only, where an empty tensor stands for none, or a shape outside the
// layer-1 table), nothing launched, the slab untouched: the caller runs
// silu_bwd + wgrad_pair. Z gets the checks dH gets.
bool wgrad_pair_act(torch::Tensor dH0, torch::Tensor Z0, torch::Tensor X0,
                    torch::Tensor slab0, int64_t dW_off0, int64_t db_off0,
                    int64_t n_valid0, torch::Tensor dH1, torch::Tensor Z1,
                    torch::Tensor X1, torch::Tensor slab1, int64_t dW_off1,
                    int64_t db_off1, int64_t n_valid1, int64_t variant = -1) {
  const char* op = "wgrad_pair_act";
  const int64_t S = dH0.dim() == 2 ? dH0.size(0) : -1;
  WgradNet n0 =
      check_wgrad_net(op, dH0, X0, slab0, dW_off0, db_off0, n_valid0, S);
  WgradNet n1 =
      check_wgrad_net(op, dH1, X1, slab1, dW_off1, db_off1, n_valid1, S);
  const int64_t N_STRIDE = dH0.size(1), K = X0.size(1);
  TORCH_CHECK(dH1.size(1) == N_STRIDE && X1.size(1) == K,
              "wgrad_pair_act: the two nets' operand widths differ");
  TORCH_CHECK(K % 32 == 0, "wgrad_pair_act: K must be a multiple of 32");
  TORCH_CHECK(N_STRIDE % 16 == 0,
              "wgrad_pair_act: dH width must be a multiple of 16");
  auto zact = [&](const torch::Tensor& Z, const torch::Tensor& dH) {
    if (Z.numel() == 0) return (const void*)nullptr;
    CHK(Z, torch::kBFloat16);
    TORCH_CHECK(Z.dim() == 2 && Z.size(0) == S && Z.size(1) == N_STRIDE, op,
                ": Z must have dH's shape");
    TORCH_CHECK(Z.device() == dH.device(), op, ": Z on another device");
    TORCH_CHECK((uintptr_t)Z.data_ptr() % 16 == 0 &&
                    (uintptr_t)dH.data_ptr() % 16 == 0,
                op, ": dH and Z must be 16-byte aligned");
    return (const void*)Z.data_ptr();
  };
  n0.Zact = zact(Z0, dH0);
  n1.Zact = zact(Z1, dH1);
  if (!n0.Zact && !n1.Zact) return false;
  return launch_wgrad_pair(n0, n1, (int)S, (int)N_STRIDE, (int)K, (int)variant,
                           cur_stream()) == 1;
}

// ppo_gather / ppo_gather_disc for all rows of idx in one bandwidth-built
// launch (mlp.hip ppo_gather_rows_kernel), outputs bit-equal. action int64
// [rows] = the discrete form, float [rows, ACT <= 8] the continuous one.
// Returns false, launching nothing, for a shape the kernel does not take.
bool ppo_gather_rows(torch::Tensor idx, torch::Tensor obs,
                     torch::Tensor action, torch::Tensor logp,
                     torch::Tensor value, torch::Tensor adv,
                     torch::Tensor targets, torch::Tensor obs_out,
                     torch::Tensor action_out, torch::Tensor logp_out,
                     torch::Tensor value_out, torch::Tensor adv_out,
                     torch::Tensor targets_out, torch::Tensor nmean,
                     torch::Tensor nvar) {
  const char* op = "ppo_gather_rows";
  CHK(idx, torch::kInt64);
  CHK(obs, torch::kFloat32);
  CHK(obs_out, torch::kBFloat16);
  const bool disc = action.scalar_type() == torch::kInt64;
  const auto act_ty = disc ? torch::kInt64 : torch::kFloat32;
  CHK(action, act_ty);
  CHK(action_out, act_ty);
  const int64_t n = idx.numel();
  TORCH_CHECK(obs.dim() == 2 && obs_out.dim() == 2 && obs_out.size(0) >= n, op,
              ": obs [rows, OBS], obs_out [>= n, OBS_PAD]");
  const int64_t rows = obs.size(0), OBS = obs.size(1), PAD = obs_out.size(1);
  TORCH_CHECK((uintptr_t)obs_out.data_ptr() % 8 == 0, op,
              ": obs_out must be 8-byte aligned");
  int64_t ACT = 1;
  if (disc) {
    TORCH_CHECK(action.numel() == rows && action_out.numel() >= n, op,
                ": discrete action is one int64 per row");
  } else {
    TORCH_CHECK(action.dim() == 2 && action.size(0) == rows &&
                    action_out.dim() == 2 && action_out.size(0) >= n &&
                    action_out.size(1) == action.size(1),
                op, ": action [rows, ACT], action_out [>= n, ACT]");
    ACT = action.size(1);
  }
  for (const torch::Tensor* t : {&logp, &value, &adv, &targets}) {
    CHK(*t, torch::kFloat32);
    TORCH_CHECK(t->numel() == rows, op, ": a source field per obs row");
  }
  for (const torch::Tensor* t :
       {&logp_out, &value_out, &adv_out, &targets_out}) {
    CHK(*t, torch::kFloat32);
    TORCH_CHECK(t->numel() >= n, op, ": an output field shorter than idx");
  }
  if (nmean.numel() > 0 || nvar.numel() > 0) {
    CHK(nmean, torch::kFloat32);
    CHK(nvar, torch::kFloat32);
    TORCH_CHECK(nmean.numel() == OBS && nvar.numel() == OBS, op,
                ": nmean / nvar must hold OBS floats");
  }
  if (n == 0) return false;
  return launch_ppo_gather_rows(
             idx.data_ptr<long>(), (long)n, obs.data_ptr<float>(), (int)OBS,
             (int)PAD, action.data_ptr(), (int)ACT, disc ? 1 : 0,
             logp.data_ptr<float>(), value.data_ptr<float>(),
             adv.data_ptr<float>(), targets.data_ptr<float>(),
             obs_out.data_ptr(), action_out.data_ptr(),
             logp_out.data_ptr<float>(), value_out.data_ptr<float>(),
             adv_out.data_ptr<float>(), targets_out.data_ptr<float>(),
             fptr_or_null(nmean), fptr_or_null(nvar), cur_stream()) == 0;
}

// The largest chain the two-launch tail takes: beyond it the norm kernel of
// fused_adam_bf16 (2048 blocks of 256 threads, one 8-vector per thread)
// goes grid-stride and the order of its adds is another one.
constexpr int64_t kTailMaxN = 2048LL * 256 * 8;

// One chain of a slab reduce: the [64, stride] slab, its flat bf16 grad and
// the Adam prologue's sqnorm / step_t (both empty: no prologue). With a
// `counter` the chain is slab_reduce_norm_pair's, whose ordered norm needs
// 1 + ceil(n / 512) floats of sqnorm and one int32 that is zero between
// calls.
TailChain check_reduce_chain(const char* op, const torch::Tensor& slab,
                             const torch::Tensor& grad,
                             const torch::Tensor& sqnorm,
                             const torch::Tensor& step,
                             const torch::Tensor* counter = nullptr) {
  CHK(slab, torch::kFloat32);
  CHK(grad, torch::kBFloat16);
  TORCH_CHECK(slab.dim() == 2 && slab.size(0) == 64, op,
              ": slabs must be [64, n]");
  const int64_t n = grad.numel();
  TORCH_CHECK(n <= slab.size(1), op, ": grad longer than a slab image");
  TORCH_CHECK((sqnorm.numel() > 0) == (step.numel() > 0), op,
              ": sqnorm and step_t go together");
  if (counter) {
    CHK(sqnorm, torch::kFloat32);
    CHK(step, torch::kInt64);
    CHK(*counter, torch::kInt32);
    TORCH_CHECK(n >= 1 && n <= kTailMaxN, op,
                ": grad empty or too long for the ordered norm");
    TORCH_CHECK(sqnorm.numel() >= 1 + (n + 511) / 512, op,
                ": sqnorm needs 1 + ceil(n / 512) floats");
    TORCH_CHECK(step.numel() == 1 && counter->numel() == 1, op,
                ": step_t and counter hold one element");
  }
  return {slab.data_ptr<float>(), grad.data_ptr(), (long)slab.size(1), (long)n,
          fptr_or_null(sqnorm), ptr_or_null<long>(step),
          counter ? (unsigned int*)counter->data_ptr<int>() : nullptr};
}

void slab_reduce(torch::Tensor slab, torch::Tensor grad16,
                 torch::Tensor sqnorm, torch::Tensor step_t) {
  const TailChain c =
      check_reduce_chain("slab_reduce", slab, grad16, sqnorm, step_t);
  // this kernel zeroes the slab behind its sums
  launch_slab_reduce(slab.data_ptr<float>(), c.grad16, c.slab_stride, c.n,
                     c.sqnorm, c.step_t, cur_stream());
}

// One launch over both chains' slabs; same sums and Adam prologue as
// slab_reduce(), but the slabs are left as they are (not zeroed).
void slab_reduce_pair(torch::Tensor slab0, torch::Tensor grad0,
                      torch::Tensor sqnorm0, torch::Tensor step0,
                      torch::Tensor slab1, torch::Tensor grad1,
                      torch::Tensor sqnorm1, torch::Tensor step1) {
  const char* op = "slab_reduce_pair";
  launch_slab_reduce_pair(
      check_reduce_chain(op, slab0, grad0, sqnorm0, step0),
      check_reduce_chain(op, slab1, grad1, sqnorm1, step1), cur_stream());
}

// slab_reduce_pair plus each chain's squared gradient norm, left in
// sqnorm[0] with the bit pattern fused_adam_bf16's ordered norm gives.
void slab_reduce_norm_pair(torch::Tensor slab0, torch::Tensor grad0,
                           torch::Tensor sqnorm0, torch::Tensor step0,
                           torch::Tensor counter0, torch::Tensor slab1,
                           torch::Tensor grad1, torch::Tensor sqnorm1,
                           torch::Tensor step1, torch::Tensor counter1) {
  const char* op = "slab_reduce_norm_pair";
  launch_slab_reduce_norm_pair(
      check_reduce_chain(op, slab0, grad0, sqnorm0, step0, &counter0),
      check_reduce_chain(op, slab1, grad1, sqnorm1, step1, &counter1),
      cur_stream());
}

// One chain of adam_pair: fp32 master param and moments, bf16 grad and
// (optional) bf16 mirror of one length, the finished norm in sqnorm[0].
AdamChain check_adam_chain(const torch::Tensor& param,
                           const torch::Tensor& grad, const torch::Tensor& m,
                           const torch::Tensor& v, const torch::Tensor& sqnorm,
                           const torch::Tensor& step,
                           const torch::Tensor& param_bf16, double lr) {
  CHK(param, torch::kFloat32);
  CHK(grad, torch::kBFloat16);
  CHK(m, torch::kFloat32);
  CHK(v, torch::kFloat32);
  CHK(sqnorm, torch::kFloat32);
  CHK(step, torch::kInt64);
  const int64_t n = param.numel();
  TORCH_CHECK(grad.numel() == n && m.numel() == n && v.numel() == n,
              "adam_pair: param, grad and moments must have one length");
  TORCH_CHECK(sqnorm.numel() >= 1 && step.numel() == 1,
              "adam_pair: sqnorm and step_t must not be empty");
  if (param_bf16.numel() > 0) {
    CHK(param_bf16, torch::kBFloat16);
    TORCH_CHECK(param_bf16.numel() == n, "adam_pair: bf16 mirror length");
  }
  return {param.data_ptr<float>(), grad.data_ptr(), m.data_ptr<float>(),
          v.data_ptr<float>(), sqnorm.data_ptr<float>(), step.data_ptr<long>(),
          vptr_or_null(param_bf16), (long)n, (float)lr};
}

// Both chains' clip + Adam + bf16 mirror in one launch, reading the
// finished norm from sqnorm[0] (slab_reduce_norm_pair).
void adam_pair(torch::Tensor param0, torch::Tensor grad0, torch::Tensor m0,
               torch::Tensor v0, torch::Tensor sqnorm0, torch::Tensor step0,
               torch::Tensor param_bf16_0, double lr0, torch::Tensor param1,
               torch::Tensor grad1, torch::Tensor m1, torch::Tensor v1,
               torch::Tensor sqnorm1, torch::Tensor step1,
               torch::Tensor param_bf16_1, double lr1, double beta1,
               double beta2, double eps, double max_norm, double grad_scale) {
  launch_adam_pair(
      check_adam_chain(param0, grad0, m0, v0, sqnorm0, step0, param_bf16_0,
                       lr0),
      check_adam_chain(param1, grad1, m1, v1, sqnorm1, step1, param_bf16_1,
                       lr1),
      (float)beta1, (float)beta2, (float)eps, (float)max_norm,
      (float)grad_scale, cur_stream());
}

void bump_add(torch::Tensor draw_buf, int64_t n) {
  launch_bump_add((unsigned int*)draw_buf.data_ptr<int>(), (unsigned int)n,
                  cur_stream());
}

void tr16_probe(torch::Tensor in, torch::Tensor out, int64_t base_mode) {
  CHK(in, torch::kBFloat16);
  launch_tr16_probe(in.data_ptr(), out.data_ptr<float>(), (int)base_mode,
                    cur_stream());
}

// Argument checks shared by the two C51 loss launchers (c51.hip): logits are
// contiguous fp32 or bf16 [B, A, atoms] with 1 <= A <= 64 and
// 1 <= atoms <= 1024; the action vector is int64 [B], or empty for A == 1.
// Per-row vectors (a_tm1, r_t, d_t, grad_ce) may be strided views, e.g. a
// column of a batch or an expanded scalar. Returns 1 for bf16 logits.
int check_c51_logits(const torch::Tensor& logits, const char* name,
                     int64_t B, int64_t A) {
  TORCH_CHECK(logits.is_cuda() && logits.is_contiguous(), name,
              " must be a contiguous GPU tensor");
  TORCH_CHECK(logits.scalar_type() == torch::kFloat32 ||
                  logits.scalar_type() == torch::kBFloat16,
              name, " must be fp32 or bf16");
  TORCH_CHECK(logits.dim() == 3 && logits.size(0) == B && logits.size(1) == A,
              name, " must be [", B, ", ", A, ", atoms]");
  TORCH_CHECK(A >= 1 && A <= 64, "c51 loss supports 1 <= A <= 64, got ", A);
  TORCH_CHECK(logits.size(2) >= 1 && logits.size(2) <= 1024,
              "c51 loss supports 1 <= atoms <= 1024, got ", logits.size(2));
  return logits.scalar_type() == torch::kBFloat16 ? 1 : 0;
}

// A vector of B values on the GPU with a non-negative element stride.
void check_c51_vector(const torch::Tensor& t, const char* name,
                      torch::ScalarType ty, int64_t B) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == ty && t.dim() == 1 &&
                  t.size(0) == B && t.stride(0) >= 0,
              name, " must be a GPU vector of ", B, " ", ty, " values");
}

const long* check_c51_actions(const torch::Tensor& a_tm1, int64_t B,
                              int64_t A) {
  if (a_tm1.numel() == 0) {
    TORCH_CHECK(A == 1, "c51 loss: an empty a_tm1 needs A == 1, got ", A);
    return nullptr;
  }
  check_c51_vector(a_tm1, "a_tm1", torch::kInt64, B);
  return a_tm1.data_ptr<long>();
}

void check_c51_rows(const torch::Tensor& t, const char* name, int64_t rows,
                    int64_t cols) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() &&
                  t.scalar_type() == torch::kFloat32,
              name, " must be a contiguous fp32 GPU tensor");
  TORCH_CHECK(t.numel() == rows * cols && t.size(0) == rows, name,
              " must hold ", rows, " x ", cols, " values");
}

void c51_loss_fwd(torch::Tensor logits_tm1, torch::Tensor atoms_tm1,
                  torch::Tensor a_tm1, torch::Tensor r_t, torch::Tensor d_t,
                  torch::Tensor logits_t, torch::Tensor atoms_t,
                  torch::Tensor selector, torch::Tensor ce, torch::Tensor lse,
                  torch::Tensor target) {
  TORCH_CHECK(logits_tm1.dim() == 3, "logits_tm1 must be [B, A, M]");
  const int64_t B = logits_tm1.size(0), A = logits_tm1.size(1);
  const int tm1_bf16 = check_c51_logits(logits_tm1, "logits_tm1", B, A);
  const int t_bf16 = check_c51_logits(logits_t, "logits_t", B, A);
  const int64_t M = logits_tm1.size(2), N = logits_t.size(2);
  const long* ap = check_c51_actions(a_tm1, B, A);
  check_c51_rows(atoms_tm1, "atoms_tm1", M, 1);
  check_c51_rows(atoms_t, "atoms_t", N, 1);
  check_c51_vector(r_t, "r_t", torch::kFloat32, B);
  check_c51_vector(d_t, "d_t", torch::kFloat32, B);
  check_c51_rows(ce, "ce", B, 1);
  check_c51_rows(lse, "lse", B, 1);
  check_c51_rows(target, "target", B, M);
  const float* sel = nullptr;
  if (selector.numel() > 0) {
    check_c51_rows(selector, "selector", B, A);
    sel = selector.data_ptr<float>();
  } else {
    TORCH_CHECK(A == 1, "c51 loss: an empty selector needs A == 1, got ", A);
  }
  launch_c51_loss_fwd(logits_tm1.data_ptr(), atoms_tm1.data_ptr<float>(), ap,
                      r_t.data_ptr<float>(), d_t.data_ptr<float>(),
                      logits_t.data_ptr(), atoms_t.data_ptr<float>(), sel,
                      ce.data_ptr<float>(), lse.data_ptr<float>(),
                      target.data_ptr<float>(), (int)B, (int)A, (int)N,
                      (int)M, tm1_bf16, t_bf16, ap ? (long)a_tm1.stride(0) : 0,
                      (long)r_t.stride(0), (long)d_t.stride(0), cur_stream());
}

void c51_loss_bwd(torch::Tensor grad_ce, torch::Tensor logits_tm1,
                  torch::Tensor a_tm1, torch::Tensor lse, torch::Tensor target,
                  torch::Tensor dlogits) {
  TORCH_CHECK(logits_tm1.dim() == 3, "logits_tm1 must be [B, A, M]");
  const int64_t B = logits_tm1.size(0), A = logits_tm1.size(1);
  const int is_bf16 = check_c51_logits(logits_tm1, "logits_tm1", B, A);
  const int64_t M = logits_tm1.size(2);
  check_c51_logits(dlogits, "dlogits", B, A);
  TORCH_CHECK(dlogits.scalar_type() == logits_tm1.scalar_type() &&
                  dlogits.size(2) == M,
              "dlogits must match logits_tm1 in dtype and shape");
  const long* ap = check_c51_actions(a_tm1, B, A);
  check_c51_rows(lse, "lse", B, 1);
  check_c51_rows(target, "target", B, M);
  check_c51_vector(grad_ce, "grad_ce", torch::kFloat32, B);
  launch_c51_loss_bwd(grad_ce.data_ptr<float>(), (long)grad_ce.stride(0),
                      logits_tm1.data_ptr(), ap, lse.data_ptr<float>(),
                      target.data_ptr<float>(), dlogits.data_ptr(), (int)B,
                      (int)A, (int)M, is_bf16, ap ? (long)a_tm1.stride(0) : 0,
                      cur_stream());
}

// Argument checks shared by the two QR loss launchers (qr.hip): quantile
// tensors are contiguous fp32 or bf16 [B, quantiles, A], action innermost,
// with 1 <= A <= 64 and 1 <= quantiles <= 1024; the per-row vectors follow
// check_c51_vector. Returns 1 for bf16.
int check_qr_dist(const torch::Tensor& t, const char* name, int64_t B,
                  int64_t A) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous(), name,
              " must be a contiguous GPU tensor");
  TORCH_CHECK(t.scalar_type() == torch::kFloat32 ||
                  t.scalar_type() == torch::kBFloat16,
              name, " must be fp32 or bf16");
  TORCH_CHECK(t.dim() == 3 && t.size(0) == B && t.size(2) == A, name,
              " must be [", B, ", quantiles, ", A, "]");
  TORCH_CHECK(A >= 1 && A <= 64, "qr loss supports 1 <= A <= 64, got ", A);
  TORCH_CHECK(t.size(1) >= 1 && t.size(1) <= 1024,
              "qr loss supports 1 <= quantiles <= 1024, got ", t.size(1));
  return t.scalar_type() == torch::kBFloat16 ? 1 : 0;
}

const long* check_qr_actions(const torch::Tensor& a_tm1, int64_t B,
                             int64_t A) {
  if (a_tm1.numel() == 0) {
    TORCH_CHECK(A == 1, "qr loss: an empty a_tm1 needs A == 1, got ", A);
    return nullptr;
  }
  check_c51_vector(a_tm1, "a_tm1", torch::kInt64, B);
  return a_tm1.data_ptr<long>();
}

void qr_loss_fwd(torch::Tensor src, torch::Tensor tau, torch::Tensor a_tm1,
                 torch::Tensor r_t, torch::Tensor d_t, torch::Tensor sel,
                 torch::Tensor tgt, torch::Tensor loss, torch::Tensor gth,
                 double huber_param) {
  TORCH_CHECK(src.dim() == 3, "src must be [B, N, A]");
  const int64_t B = src.size(0), N = src.size(1), A = src.size(2);
  const int src_bf16 = check_qr_dist(src, "src", B, A);
  const int tgt_bf16 = check_qr_dist(tgt, "tgt", B, A);
  const int64_t M = tgt.size(1);
  // tau: [N], or [B, N] rows of unit element stride (row stride 0 for an
  // expanded view)
  TORCH_CHECK(tau.is_cuda() && tau.scalar_type() == torch::kFloat32 &&
                  (tau.dim() == 1 || tau.dim() == 2) && tau.size(-1) == N &&
                  (N == 1 || tau.stride(-1) == 1),
              "tau must be fp32 [N] or [B, N] with contiguous rows");
  int64_t tau_stride = 0;
  if (tau.dim() == 2) {
    TORCH_CHECK(tau.size(0) == B && tau.stride(0) >= 0,
                "tau must be [", B, ", ", N, "] with a non-negative row stride");
    tau_stride = tau.stride(0);
  }
  const long* ap = check_qr_actions(a_tm1, B, A);
  const float *rp = nullptr, *dp = nullptr;
  TORCH_CHECK((r_t.numel() == 0) == (d_t.numel() == 0) || B == 0,
              "qr loss: r_t and d_t come together");
  if (r_t.numel() > 0) {
    check_c51_vector(r_t, "r_t", torch::kFloat32, B);
    check_c51_vector(d_t, "d_t", torch::kFloat32, B);
    rp = r_t.data_ptr<float>();
    dp = d_t.data_ptr<float>();
  }
  const void* sp = nullptr;
  int sel_bf16 = 0;
  int64_t Ns = 1;
  if (sel.numel() > 0) {
    sel_bf16 = check_qr_dist(sel, "sel", B, A);
    Ns = sel.size(1);
    sp = sel.data_ptr();
  } else {
    TORCH_CHECK(A == 1, "qr loss: an empty selector needs A == 1, got ", A);
  }
  check_c51_rows(loss, "loss", B, 1);
  check_c51_rows(gth, "gth", B, N);
  const int rc = launch_qr_loss_fwd(
      src.data_ptr(), tau.data_ptr<float>(), ap, rp, dp, sp, tgt.data_ptr(),
      loss.data_ptr<float>(), gth.data_ptr<float>(), (int)B, (int)A, (int)N,
      (int)M, (int)Ns, src_bf16, tgt_bf16, sel_bf16, (float)huber_param,
      (long)tau_stride, ap ? (long)a_tm1.stride(0) : 0,
      rp ? (long)r_t.stride(0) : 0, dp ? (long)d_t.stride(0) : 0,
      cur_stream());
  TORCH_CHECK(rc == 0, "qr_loss_fwd: sizes outside the kernel's range");
}

void qr_loss_bwd(torch::Tensor grad, torch::Tensor gth, torch::Tensor a_tm1,
                 torch::Tensor dsrc) {
  TORCH_CHECK(dsrc.dim() == 3, "dsrc must be [B, N, A]");
  const int64_t B = dsrc.size(0), N = dsrc.size(1), A = dsrc.size(2);
  const int is_bf16 = check_qr_dist(dsrc, "dsrc", B, A);
  const long* ap = check_qr_actions(a_tm1, B, A);
  check_c51_rows(gth, "gth", B, N);
  check_c51_vector(grad, "grad", torch::kFloat32, B);
  const int rc = launch_qr_loss_bwd(
      grad.data_ptr<float>(), (long)grad.stride(0), gth.data_ptr<float>(), ap,
      ap ? (long)a_tm1.stride(0) : 0, dsrc.data_ptr(), (int)B, (int)N, (int)A,
      is_bf16, cur_stream());
  TORCH_CHECK(rc == 0, "qr_loss_bwd: sizes outside the kernel's range");
}

// Argument checks of the tanh-Normal launchers (tanh_normal.hip): [B, A]
// contiguous fp32 or bf16 (or exactly `ty` when given). Returns 1 for bf16.
int check_tn_rows(const torch::Tensor& t, const char* name, int64_t B,
                  int64_t A, c10::optional<torch::ScalarType> ty = c10::nullopt) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.dim() == 2 &&
                  t.size(0) == B && t.size(1) == A,
              name, " must be a contiguous GPU tensor [", B, ", ", A, "]");
  TORCH_CHECK(ty ? t.scalar_type() == *ty
                 : (t.scalar_type() == torch::kFloat32 ||
                    t.scalar_type() == torch::kBFloat16),
              name, " has the wrong dtype");
  return t.scalar_type() == torch::kBFloat16 ? 1 : 0;
}

void tanh_normal_rsample_fwd(torch::Tensor loc, torch::Tensor scale,
                             torch::Tensor eps, torch::Tensor a,
                             torch::Tensor logp, torch::Tensor t,
                             double scale_affine, double shift_affine) {
  TORCH_CHECK(loc.dim() == 2, "loc must be [B, A]");
  const int64_t B = loc.size(0), A = loc.size(1);
  TORCH_CHECK(B < (int64_t(1) << 31) - 256, "tanh_normal: too many rows");
  const int loc_bf16 = check_tn_rows(loc, "loc", B, A);
  const int scale_bf16 = check_tn_rows(scale, "scale", B, A);
  check_tn_rows(eps, "eps", B, A, torch::kFloat32);
  check_tn_rows(a, "a", B, A, loc.scalar_type());
  check_c51_rows(logp, "logp", B, 1);
  if (t.numel() > 0) check_tn_rows(t, "t", B, A, torch::kFloat32);  // else unsaved
  const int rc = launch_tanh_normal_rsample_fwd(
      loc.data_ptr(), scale.data_ptr(), eps.data_ptr<float>(), a.data_ptr(),
      logp.data_ptr<float>(), fptr_or_null(t), (int)B, (int)A, loc_bf16,
      scale_bf16, (float)scale_affine, (float)shift_affine, cur_stream());
  TORCH_CHECK(rc == 0, "tanh_normal_rsample_fwd: needs 1 <= A <= 64 and a "
                       "positive scale_affine");
}

void tanh_normal_rsample_bwd(torch::Tensor da, torch::Tensor dlogp,
                             torch::Tensor t, torch::Tensor eps,
                             torch::Tensor scale, torch::Tensor dloc,
                             torch::Tensor dscale, double scale_affine) {
  TORCH_CHECK(dloc.dim() == 2, "dloc must be [B, A]");
  const int64_t B = dloc.size(0), A = dloc.size(1);
  TORCH_CHECK(B < (int64_t(1) << 31) - 256, "tanh_normal: too many rows");
  const int loc_bf16 = check_tn_rows(dloc, "dloc", B, A);
  const int scale_bf16 = check_tn_rows(scale, "scale", B, A);
  check_tn_rows(da, "da", B, A, dloc.scalar_type());
  check_tn_rows(dscale, "dscale", B, A, scale.scalar_type());
  check_tn_rows(t, "t", B, A, torch::kFloat32);
  check_tn_rows(eps, "eps", B, A, torch::kFloat32);
  check_c51_vector(dlogp, "dlogp", torch::kFloat32, B);
  const int rc = launch_tanh_normal_rsample_bwd(
      da.data_ptr(), dlogp.data_ptr<float>(), (long)dlogp.stride(0),
      t.data_ptr<float>(), eps.data_ptr<float>(), scale.data_ptr(),
      dloc.data_ptr(), dscale.data_ptr(), (int)B, (int)A, loc_bf16, scale_bf16,
      (float)scale_affine, cur_stream());
  TORCH_CHECK(rc == 0, "tanh_normal_rsample_bwd: needs 1 <= A <= 64");
}

// SAC row kernels (tanh_normal.hip): critic values are contiguous fp32
// [Q, B] with 1 <= Q <= 4, log_alpha one fp32 value on the GPU.
void check_sac_q(const torch::Tensor& t, const char* name, int64_t Q,
                 int64_t B) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() &&
                  t.scalar_type() == torch::kFloat32 && t.dim() == 2 &&
                  t.size(0) == Q && t.size(1) == B,
              name, " must be a contiguous fp32 GPU tensor [", Q, ", ", B, "]");
  TORCH_CHECK(Q >= 1 && Q <= 4, "sac rows support 1 <= Q <= 4, got ", Q);
  TORCH_CHECK(B < (int64_t(1) << 31) - 256, "sac rows: too many rows");
}

const float* check_sac_log_alpha(const torch::Tensor& t) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kFloat32 &&
                  t.numel() == 1,
              "log_alpha must be one fp32 value on the GPU");
  return t.data_ptr<float>();
}

void sac_critic_rows(torch::Tensor q_pred, torch::Tensor q_next,
                     torch::Tensor logp_next, torch::Tensor r_t,
                     torch::Tensor d_t, torch::Tensor log_alpha, double gamma,
                     torch::Tensor target, torch::Tensor rows,
                     torch::Tensor dq) {
  TORCH_CHECK(q_pred.dim() == 2, "q_pred must be [Q, B]");
  const int64_t Q = q_pred.size(0), B = q_pred.size(1);
  check_sac_q(q_pred, "q_pred", Q, B);
  check_sac_q(q_next, "q_next", Q, B);
  check_sac_q(dq, "dq", Q, B);
  check_c51_vector(logp_next, "logp_next", torch::kFloat32, B);
  check_c51_vector(r_t, "r_t", torch::kFloat32, B);
  check_c51_vector(d_t, "d_t", torch::kFloat32, B);
  check_c51_rows(target, "target", B, 1);
  check_c51_rows(rows, "rows", B, 1);
  const int rc = launch_sac_critic_rows(
      q_pred.data_ptr<float>(), q_next.data_ptr<float>(),
      logp_next.data_ptr<float>(), (long)logp_next.stride(0),
      r_t.data_ptr<float>(), (long)r_t.stride(0), d_t.data_ptr<float>(),
      (long)d_t.stride(0), check_sac_log_alpha(log_alpha), (float)gamma,
      target.data_ptr<float>(), rows.data_ptr<float>(), dq.data_ptr<float>(),
      (int)Q, (int)B, cur_stream());
  TORCH_CHECK(rc == 0, "sac_critic_rows: sizes outside the kernel's range");
}

void sac_actor_rows(torch::Tensor q_new, torch::Tensor logp_new,
                    torch::Tensor log_alpha, double target_entropy,
                    torch::Tensor actor_rows, torch::Tensor alpha_rows,
                    torch::Tensor argmin, torch::Tensor entropy_rows) {
  TORCH_CHECK(q_new.dim() == 2, "q_new must be [Q, B]");
  const int64_t Q = q_new.size(0), B = q_new.size(1);
  check_sac_q(q_new, "q_new", Q, B);
  check_c51_vector(logp_new, "logp_new", torch::kFloat32, B);
  check_c51_rows(actor_rows, "actor_rows", B, 1);
  check_c51_rows(alpha_rows, "alpha_rows", B, 1);
  check_c51_rows(entropy_rows, "entropy_rows", B, 1);
  TORCH_CHECK(argmin.is_cuda() && argmin.is_contiguous() &&
                  argmin.scalar_type() == torch::kInt32 && argmin.numel() == B,
              "argmin must be a contiguous int32 GPU vector of ", B);
  const int rc = launch_sac_actor_rows(
      q_new.data_ptr<float>(), logp_new.data_ptr<float>(),
      (long)logp_new.stride(0), check_sac_log_alpha(log_alpha),
      (float)target_entropy, actor_rows.data_ptr<float>(),
      alpha_rows.data_ptr<float>(), argmin.data_ptr<int>(),
      entropy_rows.data_ptr<float>(), (int)Q, (int)B, cur_stream());
  TORCH_CHECK(rc == 0, "sac_actor_rows: sizes outside the kernel's range");
}

// Critic half: g_rows, dq -> dq_pred. The actor half's tensors are unused.
void sac_critic_rows_bwd(torch::Tensor g_rows, torch::Tensor dq,
                         torch::Tensor dq_pred) {
  TORCH_CHECK(dq.dim() == 2, "dq must be [Q, B]");
  const int64_t Q = dq.size(0), B = dq.size(1);
  check_sac_q(dq, "dq", Q, B);
  check_sac_q(dq_pred, "dq_pred", Q, B);
  check_c51_vector(g_rows, "g_rows", torch::kFloat32, B);
  const int rc = launch_sac_rows_bwd(
      g_rows.data_ptr<float>(), (long)g_rows.stride(0), dq.data_ptr<float>(),
      dq_pred.data_ptr<float>(), nullptr, 0, nullptr, 0, nullptr, nullptr, 0,
      nullptr, 0.f, nullptr, nullptr, nullptr, (int)Q, (int)B, cur_stream());
  TORCH_CHECK(rc == 0, "sac_critic_rows_bwd: sizes outside the kernel's range");
}

// Actor half: g_actor, g_alpha -> dq_new, dlogp_new, dla_rows.
void sac_actor_rows_bwd(torch::Tensor g_actor, torch::Tensor g_alpha,
                        torch::Tensor argmin, torch::Tensor logp_new,
                        torch::Tensor log_alpha, double target_entropy,
                        torch::Tensor dq_new, torch::Tensor dlogp_new,
                        torch::Tensor dla_rows) {
  TORCH_CHECK(dq_new.dim() == 2, "dq_new must be [Q, B]");
  const int64_t Q = dq_new.size(0), B = dq_new.size(1);
  check_sac_q(dq_new, "dq_new", Q, B);
  check_c51_vector(g_actor, "g_actor", torch::kFloat32, B);
  check_c51_vector(g_alpha, "g_alpha", torch::kFloat32, B);
  check_c51_vector(logp_new, "logp_new", torch::kFloat32, B);
  check_c51_rows(dlogp_new, "dlogp_new", B, 1);
  check_c51_rows(dla_rows, "dla_rows", B, 1);
  TORCH_CHECK(argmin.is_cuda() && argmin.is_contiguous() &&
                  argmin.scalar_type() == torch::kInt32 && argmin.numel() == B,
              "argmin must be a contiguous int32 GPU vector of ", B);
  const int rc = launch_sac_rows_bwd(
      nullptr, 0, nullptr, nullptr, g_actor.data_ptr<float>(),
      (long)g_actor.stride(0), g_alpha.data_ptr<float>(),
      (long)g_alpha.stride(0), argmin.data_ptr<int>(),
      logp_new.data_ptr<float>(), (long)logp_new.stride(0),
      check_sac_log_alpha(log_alpha), (float)target_entropy,
      dq_new.data_ptr<float>(), dlogp_new.data_ptr<float>(),
      dla_rows.data_ptr<float>(), (int)Q, (int)B, cur_stream());
  TORCH_CHECK(rc == 0, "sac_actor_rows_bwd: sizes outside the kernel's range");
}

// Argument checks shared by the NoisyLinear launchers (noisy.hip): the fp32
// parameters mu_w / sigma_w [N, K] contiguous and 16-byte aligned, the noise
// vectors fp32 views of the NoiseBank buffer (any offset, unit stride), and
// activations / gradients as contiguous, 16-byte aligned fp32 or bf16
// [rows, cols]. check_noisy_act returns 1 for bf16.
struct NoisyShape {
  int64_t N, K;
};

void check_noisy_f32(const torch::Tensor& t, const char* name, int64_t n) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kFloat32 &&
                  t.numel() == n && t.is_contiguous(),
              name, " must be a contiguous fp32 GPU tensor of ", n, " values");
}

NoisyShape check_noisy_params(const torch::Tensor& mu_w,
                              const torch::Tensor& sigma_w,
                              const torch::Tensor& eps_in,
                              const torch::Tensor& eps_out) {
  TORCH_CHECK(mu_w.dim() == 2, "mu_w must be [N, K]");
  const NoisyShape s{mu_w.size(0), mu_w.size(1)};
  check_noisy_f32(mu_w, "mu_w", s.N * s.K);
  check_noisy_f32(sigma_w, "sigma_w", s.N * s.K);
  check_noisy_f32(eps_in, "eps_in", s.K);
  check_noisy_f32(eps_out, "eps_out", s.N);
  TORCH_CHECK((uintptr_t)mu_w.data_ptr() % 16 == 0 &&
                  (uintptr_t)sigma_w.data_ptr() % 16 == 0,
              "mu_w and sigma_w must be 16-byte aligned");
  return s;
}

int check_noisy_act(const torch::Tensor& t, const char* name, int64_t rows,
                    int64_t cols) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() &&
                  (uintptr_t)t.data_ptr() % 16 == 0,
              name, " must be a contiguous, 16-byte aligned GPU tensor");
  TORCH_CHECK(t.scalar_type() == torch::kFloat32 ||
                  t.scalar_type() == torch::kBFloat16,
              name, " must be fp32 or bf16");
  TORCH_CHECK(t.dim() == 2 && t.size(0) == rows && t.size(1) == cols, name,
              " must be [", rows, ", ", cols, "]");
  return t.scalar_type() == torch::kBFloat16 ? 1 : 0;
}

// An optional bf16 [rows, cols] tensor (empty = absent) -> pointer or null.
void* noisy_opt_bf16(const torch::Tensor& t, const char* name, int64_t rows,
                     int64_t cols) {
  if (t.numel() == 0) return nullptr;
  TORCH_CHECK(check_noisy_act(t, name, rows, cols) == 1, name,
              " must be bf16");
  return t.data_ptr();
}

// Z / H: empty tensors are not written. False for an ineligible shape.
bool noisy_linear_fwd(torch::Tensor X, torch::Tensor mu_w,
                      torch::Tensor sigma_w, torch::Tensor mu_b,
                      torch::Tensor sigma_b, torch::Tensor eps_in,
                      torch::Tensor eps_out, torch::Tensor Z, torch::Tensor H,
                      int64_t act, bool noisy) {
  const NoisyShape s = check_noisy_params(mu_w, sigma_w, eps_in, eps_out);
  TORCH_CHECK(X.dim() == 2, "X must be [S, K]");
  const int64_t S = X.size(0);
  const int x_bf16 = check_noisy_act(X, "X", S, s.K);
  check_noisy_f32(mu_b, "mu_b", s.N);
  check_noisy_f32(sigma_b, "sigma_b", s.N);
  void* zp = noisy_opt_bf16(Z, "Z", S, s.N);
  void* hp = noisy_opt_bf16(H, "H", S, s.N);
  TORCH_CHECK(zp || hp, "noisy_linear_fwd needs Z or H");
  TORCH_CHECK(act != 0 || zp, "noisy_linear_fwd without activation writes Z");
  return launch_noisy_linear_fwd(
             X.data_ptr(), mu_w.data_ptr<float>(), sigma_w.data_ptr<float>(),
             mu_b.data_ptr<float>(), sigma_b.data_ptr<float>(),
             eps_in.data_ptr<float>(), eps_out.data_ptr<float>(), zp, hp,
             (int)S, (int)s.K, (int)s.N, x_bf16, (int)act, noisy ? 1 : 0,
             cur_stream()) == 0;
}

// out = dZ @ W, times act_prev'(Z_prev) when act_prev != 0.
bool noisy_linear_dgrad(torch::Tensor dZ, torch::Tensor mu_w,
                        torch::Tensor sigma_w, torch::Tensor eps_in,
                        torch::Tensor eps_out, torch::Tensor Z_prev,
                        torch::Tensor out, int64_t act_prev, bool noisy) {
  const NoisyShape s = check_noisy_params(mu_w, sigma_w, eps_in, eps_out);
  TORCH_CHECK(dZ.dim() == 2, "dZ must be [S, N]");
  const int64_t S = dZ.size(0);
  const int dz_bf16 = check_noisy_act(dZ, "dZ", S, s.N);
  void* zp = noisy_opt_bf16(Z_prev, "Z_prev", S, s.K);
  TORCH_CHECK(act_prev == 0 || zp, "act_prev needs Z_prev");
  TORCH_CHECK(noisy_opt_bf16(out, "out", S, s.K), "out must be bf16 [S, K]");
  return launch_noisy_linear_dgrad(
             dZ.data_ptr(), mu_w.data_ptr<float>(), sigma_w.data_ptr<float>(),
             eps_in.data_ptr<float>(), eps_out.data_ptr<float>(), zp,
             out.data_ptr(), (int)S, (int)s.K, (int)s.N, dz_bf16,
             (int)act_prev, noisy ? 1 : 0, cur_stream()) == 0;
}

// dsigma_w / dsigma_b: empty tensors are not written (noise off).
bool noisy_linear_wgrad(torch::Tensor dZ, torch::Tensor X,
                        torch::Tensor eps_in, torch::Tensor eps_out,
                        torch::Tensor dmu_w, torch::Tensor dsigma_w,
                        torch::Tensor dmu_b, torch::Tensor dsigma_b) {
  TORCH_CHECK(dZ.dim() == 2 && X.dim() == 2, "dZ [S, N] and X [S, K]");
  const int64_t S = dZ.size(0), N = dZ.size(1), K = X.size(1);
  const int dz_bf16 = check_noisy_act(dZ, "dZ", S, N);
  const int x_bf16 = check_noisy_act(X, "X", S, K);
  check_noisy_f32(eps_in, "eps_in", K);
  check_noisy_f32(eps_out, "eps_out", N);
  check_noisy_f32(dmu_w, "dmu_w", N * K);
  check_noisy_f32(dmu_b, "dmu_b", N);
  float *sw = nullptr, *sb = nullptr;
  if (dsigma_w.numel() > 0) {
    check_noisy_f32(dsigma_w, "dsigma_w", N * K);
    check_noisy_f32(dsigma_b, "dsigma_b", N);
    sw = dsigma_w.data_ptr<float>();
    sb = dsigma_b.data_ptr<float>();
  }
  if (S < 1 || N < 1 || K < 8 || K % 8 != 0) return false;
  int slices, s_per;
  long slab_stride;
  noisy_wgrad_geometry((int)S, (int)K, (int)N, &slices, &s_per, &slab_stride);
  torch::Tensor slab = torch::empty(
      {(int64_t)slices * slab_stride}, dmu_w.options());
  return launch_noisy_linear_wgrad(
             dZ.data_ptr(), X.data_ptr(), slab.data_ptr<float>(),
             eps_in.data_ptr<float>(), eps_out.data_ptr<float>(),
             dmu_w.data_ptr<float>(), sw, dmu_b.data_ptr<float>(), sb, (int)S,
             (int)K, (int)N, dz_bf16, x_bf16, cur_stream()) == 0;
}

void noise_transform(torch::Tensor x) {
  check_noisy_f32(x, "x", x.numel());
  launch_noise_transform(x.data_ptr<float>(), (long)x.numel(), cur_stream());
}

// Argument checks shared by the Q-ensemble launchers (qens.hip). A dtype or a
// member count the kernels do not take makes the call ineligible (false,
// nothing launched); tensors on the wrong device, of the wrong shape or not
// contiguous are errors.
bool qens_f32(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous(), name,
              " must be a contiguous GPU tensor");
  return t.scalar_type() == torch::kFloat32;
}

// E same-shaped fp32 tensors -> one pointer per member. False: ineligible.
template <typename Members>
bool qens_members(const std::vector<torch::Tensor>& ts, const char* name,
                  c10::IntArrayRef shape, Members* out) {
  const size_t E = ts.size();
  if (E < 1 || E > QENS_MAX_E) return false;
  for (size_t e = 0; e < QENS_MAX_E; ++e) out->p[e] = nullptr;
  for (size_t e = 0; e < E; ++e) {
    if (!qens_f32(ts[e], name)) return false;
    TORCH_CHECK(ts[e].sizes() == shape, name, ": member ", e, " has shape ",
                ts[e].sizes(), ", expected ", shape);
    out->p[e] = ts[e].data_ptr<float>();
  }
  return true;
}

// The two input pieces: X0 [S, K0] (shared) or [E, S, K0], X1 [S, K1] or empty.
struct QensInput {
  const float *x0, *x1;
  int64_t x0_es, S, K0, K1;
};

bool qens_input(const torch::Tensor& X0, const torch::Tensor& X1, int64_t E,
                QensInput* in) {
  if (!qens_f32(X0, "X0")) return false;
  TORCH_CHECK(X0.dim() == 2 || (X0.dim() == 3 && X0.size(0) == E),
              "X0 must be [S, K0] or [E, S, K0]");
  in->S = X0.size(-2);
  in->K0 = X0.size(-1);
  in->x0_es = X0.dim() == 3 ? in->S * in->K0 : 0;
  in->x0 = X0.data_ptr<float>();
  in->x1 = nullptr;
  in->K1 = 0;
  if (X1.numel() > 0) {
    if (!qens_f32(X1, "X1")) return false;
    TORCH_CHECK(X1.dim() == 2 && X1.size(0) == in->S, "X1 must be [S, K1]");
    in->K1 = X1.size(1);
    in->x1 = X1.data_ptr<float>();
  }
  return in->S >= 1 && in->K0 >= 1 && in->S < (1LL << 31) - 64;
}

// dH and the saved H / Z: contiguous fp32 [E, S, N]; aux empty for act 0.
bool qens_dh(const torch::Tensor& dH, const torch::Tensor& aux, int64_t act,
             const float** ax) {
  TORCH_CHECK(dH.dim() == 3, "dH must be [E, S, N]");
  if (!qens_f32(dH, "dH")) return false;
  *ax = nullptr;
  if (act != 0) {
    if (!qens_f32(aux, "aux")) return false;
    TORCH_CHECK(aux.sizes() == dH.sizes(), "aux must have dH's shape");
    *ax = aux.data_ptr<float>();
  }
  return dH.numel() > 0;
}

// An output of rows [.., S, cols] that may be a view with margins: unit
// element stride, any row and member stride.
void check_qens_out(const torch::Tensor& t, const char* name, int64_t E,
                    int64_t S, int64_t cols) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kFloat32, name,
              " must be an fp32 GPU tensor");
  const bool ok3 = t.dim() == 3 && t.size(0) == E;
  TORCH_CHECK((ok3 || (E == 1 && t.dim() == 2)) && t.size(-2) == S &&
                  t.size(-1) == cols && (t.stride(-1) == 1 || cols == 1),
              name, " must be [", E, ", ", S, ", ", cols,
              "] with unit element stride");
}

// H [E, S, N] = act([X0 | X1] W_e^T + b_e) for every member in one launch; Z
// (empty: not written) takes the pre-activation. False: ineligible.
bool qens_linear_fwd(torch::Tensor X0, torch::Tensor X1,
                     std::vector<torch::Tensor> W, std::vector<torch::Tensor> b,
                     torch::Tensor Z, torch::Tensor H, int64_t act) {
  const int64_t E = (int64_t)W.size();
  QensInput in;
  if (E < 1 || E > QENS_MAX_E || b.size() != W.size() ||
      !qens_input(X0, X1, E, &in))
    return false;
  TORCH_CHECK(W[0].dim() == 2 && W[0].size(1) == in.K0 + in.K1,
              "W must be [N, K0 + K1]");
  const int64_t N = W[0].size(0);
  QensIn Wp, Bp;
  if (!qens_members(W, "W", {N, in.K0 + in.K1}, &Wp) ||
      !qens_members(b, "b", {N}, &Bp))
    return false;
  check_qens_out(H, "H", E, in.S, N);
  float* zp = nullptr;
  if (Z.numel() > 0) {
    check_qens_out(Z, "Z", E, in.S, N);
    TORCH_CHECK(Z.strides() == H.strides(), "Z must have H's strides");
    zp = Z.data_ptr<float>();
  }
  return launch_qens_linear_fwd(
             in.x0, (long)in.x0_es, in.x1, Wp, Bp, zp, H.data_ptr<float>(),
             (long)H.stride(-2), H.dim() == 3 ? (long)H.stride(0) : 0L,
             (int)in.S, (int)in.K0, (int)in.K1, (int)N, (int)E, (int)act,
             cur_stream()) == 0;
}

// dX = (dH * act'(aux)) @ W_e[:, c0 : c0 + dX.size(-1)]: per member into dX
// [E, S, .], or with summed over the members into dX [S, .].
bool qens_linear_dgrad(torch::Tensor dH, torch::Tensor aux,
                       std::vector<torch::Tensor> W, torch::Tensor dX,
                       int64_t c0, int64_t act, bool summed) {
  const float* ax;
  if (!qens_dh(dH, aux, act, &ax)) return false;
  const int64_t E = dH.size(0), S = dH.size(1), N = dH.size(2);
  if (W.empty() || (int64_t)W.size() != E) return false;
  TORCH_CHECK(W[0].dim() == 2 && W[0].size(0) == N, "W must be [N, K]");
  const int64_t K = W[0].size(1), KW = dX.size(-1);
  QensIn Wp;
  if (!qens_members(W, "W", {N, K}, &Wp)) return false;
  check_qens_out(dX, "dX", summed ? 1 : E, S, KW);
  TORCH_CHECK(c0 >= 0 && KW >= 1 && c0 + KW <= K, "column range outside W");
  return launch_qens_linear_dgrad(
             dH.data_ptr<float>(), ax, Wp, dX.data_ptr<float>(),
             (long)dX.stride(-2), dX.dim() == 3 ? (long)dX.stride(0) : 0L,
             (int)S, (int)K, (int)N, (int)c0, (int)(c0 + KW), (int)E,
             summed ? 1 : 0, (int)act, cur_stream()) == 0;
}

// dW_e = (dH_e * act'(aux_e))^T [X0 | X1] and db_e = its column sums, written
// into the members' gradient tensors.
bool qens_linear_wgrad(torch::Tensor dH, torch::Tensor aux, torch::Tensor X0,
                       torch::Tensor X1, std::vector<torch::Tensor> dW,
                       std::vector<torch::Tensor> db, int64_t act) {
  const float* ax;
  if (!qens_dh(dH, aux, act, &ax)) return false;
  const int64_t E = dH.size(0), S = dH.size(1), N = dH.size(2);
  QensInput in;
  if ((int64_t)dW.size() != E || db.size() != dW.size() ||
      !qens_input(X0, X1, E, &in))
    return false;
  TORCH_CHECK(in.S == S, "X0 and dH disagree on S");
  const int64_t K = in.K0 + in.K1;
  QensOut Wg, Bg;
  if (!qens_members(dW, "dW", {N, K}, &Wg) ||
      !qens_members(db, "db", {N}, &Bg))
    return false;
  int slices, s_per;
  long slab_stride;
  qens_wgrad_geometry((int)S, (int)K, (int)N, &slices, &s_per, &slab_stride);
  torch::Tensor slab =
      torch::empty({E * (int64_t)slices * slab_stride}, dH.options());
  return launch_qens_linear_wgrad(
             dH.data_ptr<float>(), ax, in.x0, (long)in.x0_es, in.x1,
             slab.data_ptr<float>(), Wg, Bg, (int)S, (int)in.K0, (int)in.K1,
             (int)N, (int)E, (int)act, cur_stream()) == 0;
}

// The Gaussian actor MLP (actor_mlp.hip). The net's tensors as a by-value
// ActorNet; false: ineligible (a dtype, a layer count or a width the kernels
// do not take). Wrong devices, shapes that disagree with each other and
// non-contiguous tensors are errors.
bool actor_net(const torch::Tensor& X_like, int64_t K0,
               const std::vector<torch::Tensor>& W,
               const std::vector<torch::Tensor>& b, const torch::Tensor& Wloc,
               const torch::Tensor& bloc, const torch::Tensor& Wscale,
               const torch::Tensor& bscale, ActorNet* net) {
  const size_t L = W.size();
  if (L < 1 || L > ACTOR_MAX_L || b.size() != L) return false;
  const int64_t S = X_like.size(0);
  if (S < 1 || S > (1LL << 30) || K0 < 1) return false;
  int64_t K = K0;
  for (size_t l = 0; l < ACTOR_MAX_L; ++l) {
    net->W[l] = net->b[l] = nullptr;
    net->N[l] = 0;
  }
  for (size_t l = 0; l < L; ++l) {
    if (!qens_f32(W[l], "W") || !qens_f32(b[l], "b")) return false;
    TORCH_CHECK(W[l].dim() == 2 && W[l].size(1) == K && b[l].dim() == 1 &&
                    b[l].size(0) == W[l].size(0),
                "layer ", l, ": W must be [N, ", K, "] and b [N]");
    const int64_t N = W[l].size(0);
    if (N < 16 || N > 256 || N % 16 != 0) return false;
    net->W[l] = W[l].data_ptr<float>();
    net->b[l] = b[l].data_ptr<float>();
    net->N[l] = (int)N;
    K = N;
  }
  if (!qens_f32(Wloc, "Wloc") || !qens_f32(bloc, "bloc") ||
      !qens_f32(Wscale, "Wscale") || !qens_f32(bscale, "bscale"))
    return false;
  TORCH_CHECK(Wloc.dim() == 2 && Wloc.size(1) == K &&
                  Wscale.sizes() == Wloc.sizes() && bloc.dim() == 1 &&
                  bloc.size(0) == Wloc.size(0) &&
                  bscale.sizes() == bloc.sizes(),
              "the head must be two [A, ", K, "] linears with [A] biases");
  const int64_t A = Wloc.size(0);
  if (A < 1 || A > 64) return false;
  net->Wloc = Wloc.data_ptr<float>();
  net->bloc = bloc.data_ptr<float>();
  net->Wscale = Wscale.data_ptr<float>();
  net->bscale = bscale.data_ptr<float>();
  net->L = (int)L;
  net->K0 = (int)K0;
  net->A = (int)A;
  net->S = (int)S;
  return true;
}

// One [S, N[l]] buffer per hidden layer, or an empty list (all absent).
void actor_bufs(const std::vector<torch::Tensor>& ts, const char* name,
                const ActorNet& net, ActorBufs* out) {
  for (int l = 0; l < ACTOR_MAX_L; ++l) out->p[l] = nullptr;
  if (ts.empty()) return;
  TORCH_CHECK((int)ts.size() == net.L, name, ": one tensor per hidden layer");
  for (int l = 0; l < net.L; ++l) {
    TORCH_CHECK(ts[l].is_cuda() && ts[l].is_contiguous() &&
                    ts[l].scalar_type() == torch::kFloat32 &&
                    ts[l].dim() == 2 && ts[l].size(0) == net.S &&
                    ts[l].size(1) == net.N[l],
                name, "[", l, "] must be contiguous fp32 [", net.S, ", ",
                net.N[l], "]");
    out->p[l] = ts[l].data_ptr<float>();
  }
}

void check_actor_rows(const torch::Tensor& t, const char* name,
                      const ActorNet& net) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() &&
                  t.scalar_type() == torch::kFloat32 && t.dim() == 2 &&
                  t.size(0) == net.S && t.size(1) == net.A,
              name, " must be contiguous fp32 [", net.S, ", ", net.A, "]");
}

// The whole actor in one launch: loc and scale [S, A]; with a backward to
// follow also spre [S, A], H[l] and (SiLU) Z[l] [S, N_l], else empty / empty
// lists. False: ineligible, nothing launched.
bool actor_mlp_fwd(torch::Tensor X, std::vector<torch::Tensor> W,
                   std::vector<torch::Tensor> b, torch::Tensor Wloc,
                   torch::Tensor bloc, torch::Tensor Wscale,
                   torch::Tensor bscale, double min_scale, int64_t act,
                   torch::Tensor loc, torch::Tensor scale, torch::Tensor spre,
                   std::vector<torch::Tensor> H, std::vector<torch::Tensor> Z) {
  TORCH_CHECK(X.dim() == 2, "X must be [S, K0]");
  ActorNet net;
  if (!qens_f32(X, "X") ||
      !actor_net(X, X.size(1), W, b, Wloc, bloc, Wscale, bscale, &net))
    return false;
  check_actor_rows(loc, "loc", net);
  check_actor_rows(scale, "scale", net);
  float* sp = nullptr;
  if (spre.numel() > 0) {
    check_actor_rows(spre, "spre", net);
    sp = spre.data_ptr<float>();
  }
  ActorBufs Hp, Zp;
  actor_bufs(H, "H", net, &Hp);
  actor_bufs(Z, "Z", net, &Zp);
  return launch_actor_mlp_fwd(X.data_ptr<float>(), net, (float)min_scale,
                              (int)act, loc.data_ptr<float>(),
                              scale.data_ptr<float>(), sp, Hp, Zp,
                              cur_stream()) == 0;
}

// The whole input-gradient chain in one launch: dZ[l] [S, N_l] of every hidden
// layer and dZh [2, S, A] = (dloc, dscale * softplus'(spre)). aux[l] is the
// saved H (ReLU) or Z (SiLU). W[0] is not read (there is no dX).
bool actor_mlp_dgrad(torch::Tensor dloc, torch::Tensor dscale,
                     torch::Tensor spre, int64_t K0,
                     std::vector<torch::Tensor> W, std::vector<torch::Tensor> b,
                     torch::Tensor Wloc, torch::Tensor bloc,
                     torch::Tensor Wscale, torch::Tensor bscale, int64_t act,
                     std::vector<torch::Tensor> aux,
                     std::vector<torch::Tensor> dZ, torch::Tensor dZh) {
  TORCH_CHECK(dloc.dim() == 2, "dloc must be [S, A]");
  ActorNet net;
  if (!qens_f32(dloc, "dloc") ||
      !actor_net(dloc, K0, W, b, Wloc, bloc, Wscale, bscale, &net))
    return false;
  check_actor_rows(dloc, "dloc", net);
  check_actor_rows(dscale, "dscale", net);
  check_actor_rows(spre, "spre", net);
  TORCH_CHECK(dZh.is_cuda() && dZh.is_contiguous() &&
                  dZh.scalar_type() == torch::kFloat32 && dZh.dim() == 3 &&
                  dZh.size(0) == 2 && dZh.size(1) == net.S &&
                  dZh.size(2) == net.A,
              "dZh must be contiguous fp32 [2, S, A]");
  TORCH_CHECK(!aux.empty() && !dZ.empty(), "aux and dZ: one per hidden layer");
  ActorBufs ax, dz;
  actor_bufs(aux, "aux", net, &ax);
  actor_bufs(dZ, "dZ", net, &dz);
  return launch_actor_mlp_dgrad(dloc.data_ptr<float>(),
                                dscale.data_ptr<float>(),
                                spre.data_ptr<float>(), net, (int)act, ax, dz,
                                dZh.data_ptr<float>(), cur_stream()) == 0;
}

// The by-value table of the multi-tensor optimiser tail (multi_adam.hip),
// built from the tensors torch's Adam owns: pointer reads only, no device
// sync and nothing copied to the device. Tensor i belongs to chain
// chain_of[i] (non-decreasing); hyper[c] = {beta1, beta2, eps, lr, max_norm,
// clip, tau}; lr_tensors[c] replaces hyper[c][3] when the param group holds a
// tensor. False: the call is ineligible (more tensors, chains or chunks than
// the table takes, a tensor that is not contiguous fp32 on partials' device)
// and nothing may be launched. Mismatched list lengths are errors.
using OptTensors = std::vector<c10::optional<torch::Tensor>>;

bool madam_f32(const torch::Tensor& t, const torch::Device& dev) {
  return t.is_cuda() && t.device() == dev &&
         t.scalar_type() == torch::kFloat32 && t.is_contiguous();
}

bool madam_table(const std::vector<torch::Tensor>& params,
                 const OptTensors& grads,
                 const OptTensors& exp_avgs,
                 const OptTensors& exp_avg_sqs,
                 const OptTensors& steps,
                 const OptTensors& targets,
                 const std::vector<int64_t>& chain_of,
                 const std::vector<std::vector<double>>& hyper,
                 const OptTensors& lr_tensors, const torch::Tensor& partials,
                 MultiAdamTable* T) {
  const size_t n = params.size(), nc = hyper.size();
  TORCH_CHECK(grads.size() == n && exp_avgs.size() == n &&
                  exp_avg_sqs.size() == n && steps.size() == n &&
                  targets.size() == n && chain_of.size() == n,
              "multi_adam: one entry per tensor in every list");
  TORCH_CHECK(lr_tensors.size() == nc, "multi_adam: one lr entry per chain");
  TORCH_CHECK(partials.is_cuda() && partials.is_contiguous() &&
                  partials.scalar_type() == torch::kFloat32,
              "multi_adam: partials must be a contiguous fp32 GPU tensor");
  if (n > MADAM_MAX_TENSORS || nc > MADAM_MAX_CHAINS) return false;
  const torch::Device dev = partials.device();
  std::memset(T, 0, sizeof(*T));

  for (size_t c = 0; c < nc; ++c) {
    TORCH_CHECK(hyper[c].size() == 7, "multi_adam: 7 values per chain");
    MultiAdamChain& ch = T->c[c];
    const double b1 = hyper[c][0], b2 = hyper[c][1], tau = hyper[c][6];
    ch.b1 = (float)b1;
    ch.b2 = (float)b2;
    ch.omb1 = (float)(1.0 - b1);
    ch.omb2 = (float)(1.0 - b2);
    ch.eps = (float)hyper[c][2];
    ch.lr = (float)hyper[c][3];
    ch.max_norm = (float)hyper[c][4];
    ch.clip = hyper[c][5] != 0.0;
    ch.tau = (float)tau;
    ch.omt = (float)(1.0 - tau);
    if (lr_tensors[c].has_value()) {
      const torch::Tensor& lr = *lr_tensors[c];
      if (!madam_f32(lr, dev) || lr.numel() != 1) return false;
      ch.lr_ptr = lr.data_ptr<float>();
    }
  }

  int64_t block = 0, prev_chain = -1;
  for (size_t i = 0; i < n; ++i) {
    const int64_t c = chain_of[i];
    TORCH_CHECK(c >= 0 && c < (int64_t)nc && c >= prev_chain,
                "multi_adam: chain ids must ascend within [0, chains)");
    const torch::Tensor& p = params[i];
    const int64_t numel = p.numel();
    if (!madam_f32(p, dev) || numel < 1) return false;
    MultiAdamTensor& t = T->t[i];
    t.p = p.data_ptr<float>();
    if (grads[i].has_value()) {
      TORCH_CHECK(exp_avgs[i].has_value() && exp_avg_sqs[i].has_value() &&
                      steps[i].has_value(),
                  "multi_adam: a tensor with a gradient needs its Adam state");
      const torch::Tensor &g = *grads[i], &m = *exp_avgs[i],
                          &v = *exp_avg_sqs[i], &st = *steps[i];
      if (!madam_f32(g, dev) || !madam_f32(m, dev) || !madam_f32(v, dev) ||
          !madam_f32(st, dev) || st.numel() != 1 || g.numel() != numel ||
          m.numel() != numel || v.numel() != numel)
        return false;
      t.g = g.data_ptr<float>();
      t.m = m.data_ptr<float>();
      t.v = v.data_ptr<float>();
      t.step = st.data_ptr<float>();
    } else {
      // no gradient this step: the entry is there for its polyak only
      TORCH_CHECK(targets[i].has_value(),
                  "multi_adam: a tensor with neither gradient nor target");
    }
    if (targets[i].has_value()) {
      const torch::Tensor& tg = *targets[i];
      if (!madam_f32(tg, dev) || tg.numel() != numel) return false;
      t.tgt = tg.data_ptr<float>();
    }
    MultiAdamChain& ch = T->c[c];
    if (c != prev_chain) ch.part_begin = (unsigned int)block;
    const int64_t chunks = (numel + MADAM_CHUNK - 1) / MADAM_CHUNK;
    if ((int64_t)ch.part_count + chunks > MADAM_MAX_CHUNKS) return false;
    ch.part_count += (unsigned int)chunks;
    t.numel = (unsigned int)numel;
    t.first_block = (unsigned short)block;
    t.chain = (unsigned short)c;
    block += chunks;
    prev_chain = c;
  }
  T->n_tensors = (int)n;
  T->n_blocks = (int)block;
  TORCH_CHECK(partials.numel() >= block, "multi_adam: partials holds ",
              partials.numel(), " floats, the call has ", block, " blocks");
  return true;
}

// Launch A of the tail: the per-block sums of squares of the clipped chains
// into partials, and step + 1 into every tensor's step. False: ineligible.
bool multi_adam_norm(std::vector<torch::Tensor> params,
                     OptTensors grads,
                     OptTensors exp_avgs,
                     OptTensors exp_avg_sqs,
                     OptTensors steps, OptTensors targets,
                     std::vector<int64_t> chain_of,
                     std::vector<std::vector<double>> hyper,
                     OptTensors lr_tensors, torch::Tensor partials) {
  MultiAdamTable T;
  if (!madam_table(params, grads, exp_avgs, exp_avg_sqs, steps, targets,
                   chain_of, hyper, lr_tensors, partials, &T))
    return false;
  launch_multi_adam_norm(T, partials.data_ptr<float>(), cur_stream());
  return true;
}

// Launch B: clip coefficient from the partials, Adam and polyak, every tensor
// read and written once. Takes what multi_adam_norm took.
bool multi_adam_update(std::vector<torch::Tensor> params,
                       OptTensors grads,
                       OptTensors exp_avgs,
                       OptTensors exp_avg_sqs,
                       OptTensors steps, OptTensors targets,
                       std::vector<int64_t> chain_of,
                       std::vector<std::vector<double>> hyper,
                       OptTensors lr_tensors, torch::Tensor partials) {
  MultiAdamTable T;
  if (!madam_table(params, grads, exp_avgs, exp_avg_sqs, steps, targets,
                   chain_of, hyper, lr_tensors, partials, &T))
    return false;
  launch_multi_adam_update(T, partials.data_ptr<float>(), cur_stream());
  return true;
}

// Argument checks shared by the two MCTS launchers (mcts.hip): the arena of
// search/mcts.py, contiguous on one GPU, B trees x N node slots x A actions.
struct MctsShape {
  int64_t B, N, A;
};

void check_mcts_tensor(const torch::Tensor& t, const char* name,
                       torch::ScalarType ty, const torch::Device& dev,
                       std::initializer_list<int64_t> shape) {
  TORCH_CHECK(t.is_cuda() && t.device() == dev && t.is_contiguous(), "mcts: ",
              name, " must be a contiguous tensor on ", dev);
  TORCH_CHECK(t.scalar_type() == ty, "mcts: ", name, " must be ", ty);
  TORCH_CHECK(t.sizes() == torch::IntArrayRef(shape), "mcts: ", name,
              " must have shape ", torch::IntArrayRef(shape), ", got ",
              t.sizes());
}

MctsShape check_mcts_arena(const torch::Tensor& visit,
                           const torch::Tensor& value_sum,
                           const torch::Tensor& reward,
                           const torch::Tensor& discount,
                           const torch::Tensor& prior,
                           const torch::Tensor& children,
                           const torch::Tensor& min_q,
                           const torch::Tensor& max_q) {
  TORCH_CHECK(prior.dim() == 3, "mcts: prior must be [B, N, A]");
  const int64_t B = prior.size(0), N = prior.size(1), A = prior.size(2);
  TORCH_CHECK(N >= 1 && A >= 1, "mcts: the arena needs N >= 1 and A >= 1");
  TORCH_CHECK(B * N * A < (int64_t(1) << 31) && B < (int64_t(1) << 31) - 256,
              "mcts: arena too large for the kernels' int sizes");
  const torch::Device dev = prior.device();
  check_mcts_tensor(visit, "visit", torch::kFloat32, dev, {B, N});
  check_mcts_tensor(value_sum, "value_sum", torch::kFloat32, dev, {B, N});
  check_mcts_tensor(reward, "reward", torch::kFloat32, dev, {B, N});
  check_mcts_tensor(discount, "discount", torch::kFloat32, dev, {B, N});
  check_mcts_tensor(prior, "prior", torch::kFloat32, dev, {B, N, A});
  check_mcts_tensor(children, "children", torch::kInt64, dev, {B, N, A});
  check_mcts_tensor(min_q, "min_q", torch::kFloat32, dev, {B});
  check_mcts_tensor(max_q, "max_q", torch::kFloat32, dev, {B});
  return {B, N, A};
}

void mcts_select(torch::Tensor visit, torch::Tensor value_sum,
                 torch::Tensor reward, torch::Tensor discount,
                 torch::Tensor prior, torch::Tensor children,
                 torch::Tensor min_q, torch::Tensor max_q, double c_puct,
                 torch::Tensor sel_parent, torch::Tensor sel_action) {
  const MctsShape s = check_mcts_arena(visit, value_sum, reward, discount,
                                       prior, children, min_q, max_q);
  const torch::Device dev = prior.device();
  check_mcts_tensor(sel_parent, "sel_parent", torch::kInt64, dev, {s.B});
  check_mcts_tensor(sel_action, "sel_action", torch::kInt64, dev, {s.B});
  launch_mcts_select(visit.data_ptr<float>(), value_sum.data_ptr<float>(),
                     reward.data_ptr<float>(), discount.data_ptr<float>(),
                     prior.data_ptr<float>(), children.data_ptr<long>(),
                     min_q.data_ptr<float>(), max_q.data_ptr<float>(),
                     sel_parent.data_ptr<long>(), sel_action.data_ptr<long>(),
                     (int)s.B, (int)s.N, (int)s.A, (float)c_puct,
                     cur_stream());
}

void mcts_expand_backup(torch::Tensor visit, torch::Tensor value_sum,
                        torch::Tensor reward, torch::Tensor discount,
                        torch::Tensor prior, torch::Tensor children,
                        torch::Tensor parent, torch::Tensor act_from_parent,
                        torch::Tensor min_q, torch::Tensor max_q,
                        torch::Tensor sel_parent, torch::Tensor sel_action,
                        int64_t new_node, torch::Tensor reward_new,
                        torch::Tensor discount_new, torch::Tensor prior_new,
                        torch::Tensor value_new) {
  const MctsShape s = check_mcts_arena(visit, value_sum, reward, discount,
                                       prior, children, min_q, max_q);
  const torch::Device dev = prior.device();
  check_mcts_tensor(parent, "parent", torch::kInt64, dev, {s.B, s.N});
  check_mcts_tensor(act_from_parent, "act_from_parent", torch::kInt64, dev,
                    {s.B, s.N});
  check_mcts_tensor(sel_parent, "sel_parent", torch::kInt64, dev, {s.B});
  check_mcts_tensor(sel_action, "sel_action", torch::kInt64, dev, {s.B});
  check_mcts_tensor(reward_new, "reward", torch::kFloat32, dev, {s.B});
  check_mcts_tensor(discount_new, "discount", torch::kFloat32, dev, {s.B});
  check_mcts_tensor(prior_new, "prior_new", torch::kFloat32, dev, {s.B, s.A});
  check_mcts_tensor(value_new, "value", torch::kFloat32, dev, {s.B});
  TORCH_CHECK(new_node >= 1 && new_node < s.N, "mcts: new_node ", new_node,
              " is outside [1, ", s.N, ")");
  launch_mcts_expand_backup(
      visit.data_ptr<float>(), value_sum.data_ptr<float>(),
      reward.data_ptr<float>(), discount.data_ptr<float>(),
      prior.data_ptr<float>(), children.data_ptr<long>(),
      parent.data_ptr<long>(), act_from_parent.data_ptr<long>(),
      min_q.data_ptr<float>(), max_q.data_ptr<float>(),
      sel_parent.data_ptr<long>(), sel_action.data_ptr<long>(),
      reward_new.data_ptr<float>(), discount_new.data_ptr<float>(),
      prior_new.data_ptr<float>(), value_new.data_ptr<float>(), (int)s.B,
      (int)s.N, (int)s.A, (int)new_node, cur_stream());
}

}  // namespace

void sumtree_tree_check(const torch::Tensor& tree, int64_t cap,
                        int64_t depth) {
  TORCH_CHECK(depth >= 0 && depth < 31 && cap == (int64_t(1) << depth),
              "sumtree: cap ", cap, " is not 1 << depth (depth ", depth, ")");
  TORCH_CHECK(tree.numel() == 2 * cap, "sumtree: tree holds ", tree.numel(),
              " floats, expected 2 * cap = ", 2 * cap);
}

void sumtree_update(torch::Tensor tree, torch::Tensor idx,
                    torch::Tensor prio, int64_t cap, int64_t depth) {
  CHK(tree, torch::kFloat32);
  CHK(idx, torch::kInt64);
  CHK(prio, torch::kFloat32);
  sumtree_tree_check(tree, cap, depth);
  TORCH_CHECK(prio.numel() == idx.numel(), "sumtree_update: ", prio.numel(),
              " priorities for ", idx.numel(), " indices");
  launch_sumtree_update(tree.data_ptr<float>(), idx.data_ptr<long>(),
                        prio.data_ptr<float>(), idx.numel(), (int)cap,
                        (int)depth, cur_stream());
}

void sumtree_sample(torch::Tensor tree, torch::Tensor u, torch::Tensor out,
                    int64_t cap, int64_t depth, int64_t n_items) {
  CHK(tree, torch::kFloat32);
  CHK(u, torch::kFloat32);
  CHK(out, torch::kInt64);
  sumtree_tree_check(tree, cap, depth);
  TORCH_CHECK(n_items >= 1 && n_items <= cap, "sumtree_sample: n_items ",
              n_items, " outside [1, cap = ", cap, "]");
  TORCH_CHECK(out.numel() == u.numel(), "sumtree_sample: out holds ",
              out.numel(), " slots for ", u.numel(), " draws");
  // the kernel reads both children of a node as one 8-byte load
  TORCH_CHECK(reinterpret_cast<uintptr_t>(tree.data_ptr<float>()) % 8 == 0,
              "sumtree_sample: tree must be 8-byte aligned");
  launch_sumtree_sample(tree.data_ptr<float>(), u.data_ptr<float>(),
                        out.data_ptr<long>(), u.numel(), (int)cap, (int)depth,
                        (int)n_items, cur_stream());
}

void rnn_scan(torch::Tensor Xp, torch::Tensor Whh, torch::Tensor bhh,
              torch::Tensor resets, torch::Tensor h0, torch::Tensor c0,
              torch::Tensor Hout, torch::Tensor hT, torch::Tensor cT,
              int64_t lstm) {
  CHK(Xp, torch::kFloat32);
  CHK(Whh, torch::kBFloat16);
  CHK(resets, torch::kUInt8);
  CHK(h0, torch::kFloat32);
  int T = Xp.size(0), B = Xp.size(1);
  int H = h0.size(1);
  TORCH_CHECK(H == 128 || H == 256, "rnn_scan supports H 128/256");
  TORCH_CHECK(Xp.size(2) == (lstm ? 4 : 3) * H, "Xp gate dim mismatch");
  launch_rnn_scan(
      Xp.data_ptr<float>(), Whh.data_ptr(), bhh.data_ptr<float>(),
      resets.data_ptr<unsigned char>(), h0.data_ptr<float>(),
      fptr_or_null(c0),
      Hout.data_ptr<float>(), hT.data_ptr<float>(),
      fptr_or_null(cT), T, B, H, (int)lstm,
      cur_stream());
}

// Shape/dtype/contiguity check for the training scan's tensors (rnn.hip).
void check_rnn_tensor(const torch::Tensor& t, const char* name,
                      c10::ScalarType ty, at::IntArrayRef shape) {
  TORCH_CHECK(t.is_cuda(), "rnn scan: ", name, " must be on GPU");
  TORCH_CHECK(t.scalar_type() == ty, "rnn scan: ", name, " has wrong dtype");
  TORCH_CHECK(t.is_contiguous(), "rnn scan: ", name, " must be contiguous");
  TORCH_CHECK(t.sizes() == shape, "rnn scan: ", name, " has shape ",
              t.sizes(), ", expected ", shape);
}

// An optional [B, H] tensor: numel 0 stands for "absent" (null pointer).
float* rnn_opt_state(const torch::Tensor& t, const char* name, int64_t B,
                     int64_t H) {
  if (t.numel() == 0) return nullptr;
  check_rnn_tensor(t, name, torch::kFloat32, {B, H});
  return t.data_ptr<float>();
}

void rnn_scan_train_fwd(torch::Tensor Xp, torch::Tensor Whh,
                        torch::Tensor bhh, torch::Tensor resets,
                        torch::Tensor h0, torch::Tensor c0,
                        torch::Tensor Hout, torch::Tensor hT,
                        torch::Tensor cT, torch::Tensor gates,
                        torch::Tensor aux, int64_t lstm) {
  TORCH_CHECK(Xp.dim() == 3 && h0.dim() == 2,
              "rnn_scan_train_fwd: Xp is [T, B, G*H], h0 is [B, H]");
  const int64_t T = Xp.size(0), B = Xp.size(1), H = h0.size(1);
  const int64_t G = lstm ? 4 : 3;
  TORCH_CHECK(H == 128 || H == 256, "rnn_scan_train_fwd supports H 128/256");
  TORCH_CHECK(Xp.size(2) == G * H, "Xp gate dim mismatch");
  TORCH_CHECK(T >= 1 && B >= 1, "rnn_scan_train_fwd needs T >= 1, B >= 1");
  check_rnn_tensor(Xp, "Xp", torch::kFloat32, {T, B, G * H});
  check_rnn_tensor(Whh, "Whh", torch::kBFloat16, {G * H, H});
  check_rnn_tensor(bhh, "bhh", torch::kFloat32, {G * H});
  check_rnn_tensor(resets, "resets", torch::kUInt8, {T, B});
  check_rnn_tensor(h0, "h0", torch::kFloat32, {B, H});
  check_rnn_tensor(Hout, "Hout", torch::kFloat32, {T, B, H});
  check_rnn_tensor(hT, "hT", torch::kFloat32, {B, H});
  check_rnn_tensor(gates, "gates", torch::kFloat32, {T, B, G * H});
  check_rnn_tensor(aux, "aux", torch::kFloat32, {T, B, H});
  const float* c0p = lstm ? rnn_opt_state(c0, "c0", B, H) : nullptr;
  float* cTp = lstm ? rnn_opt_state(cT, "cT", B, H) : nullptr;
  launch_rnn_scan_train_fwd(
      Xp.data_ptr<float>(), Whh.data_ptr(), bhh.data_ptr<float>(),
      resets.data_ptr<unsigned char>(), h0.data_ptr<float>(), c0p,
      Hout.data_ptr<float>(), hT.data_ptr<float>(), cTp,
      gates.data_ptr<float>(), aux.data_ptr<float>(), (int)T, (int)B, (int)H,
      (int)lstm, cur_stream());
}

void rnn_scan_bwd(torch::Tensor dHout, torch::Tensor dhT, torch::Tensor dcT,
                  torch::Tensor gates, torch::Tensor aux, torch::Tensor Hout,
                  torch::Tensor h0, torch::Tensor c0, torch::Tensor resets,
                  torch::Tensor WhhT, torch::Tensor dXp, torch::Tensor dHg,
                  torch::Tensor dh0, torch::Tensor dc0, int64_t lstm) {
  TORCH_CHECK(gates.dim() == 3 && h0.dim() == 2,
              "rnn_scan_bwd: gates is [T, B, G*H], h0 is [B, H]");
  const int64_t T = gates.size(0), B = gates.size(1), H = h0.size(1);
  const int64_t G = lstm ? 4 : 3;
  TORCH_CHECK(H == 128 || H == 256, "rnn_scan_bwd supports H 128/256");
  TORCH_CHECK(gates.size(2) == G * H, "gates gate dim mismatch");
  TORCH_CHECK(T >= 1 && B >= 1, "rnn_scan_bwd needs T >= 1, B >= 1");
  check_rnn_tensor(dHout, "dHout", torch::kFloat32, {T, B, H});
  check_rnn_tensor(gates, "gates", torch::kFloat32, {T, B, G * H});
  check_rnn_tensor(aux, "aux", torch::kFloat32, {T, B, H});
  check_rnn_tensor(Hout, "Hout", torch::kFloat32, {T, B, H});
  check_rnn_tensor(h0, "h0", torch::kFloat32, {B, H});
  check_rnn_tensor(resets, "resets", torch::kUInt8, {T, B});
  check_rnn_tensor(WhhT, "WhhT", torch::kBFloat16, {H, G * H});
  check_rnn_tensor(dXp, "dXp", torch::kFloat32, {T, B, G * H});
  check_rnn_tensor(dh0, "dh0", torch::kFloat32, {B, H});
  // GRU: dHg differs from dXp in the n block; LSTM: dXp is dHg.
  float* dHgp = nullptr;
  if (!lstm) {
    check_rnn_tensor(dHg, "dHg", torch::kFloat32, {T, B, G * H});
    dHgp = dHg.data_ptr<float>();
  }
  launch_rnn_scan_bwd(
      dHout.data_ptr<float>(), rnn_opt_state(dhT, "dhT", B, H),
      lstm ? rnn_opt_state(dcT, "dcT", B, H) : nullptr,
      gates.data_ptr<float>(), aux.data_ptr<float>(), Hout.data_ptr<float>(),
      h0.data_ptr<float>(), lstm ? rnn_opt_state(c0, "c0", B, H) : nullptr,
      resets.data_ptr<unsigned char>(), WhhT.data_ptr(),
      dXp.data_ptr<float>(), dHgp, dh0.data_ptr<float>(),
      lstm ? rnn_opt_state(dc0, "dc0", B, H) : nullptr, (int)T, (int)B,
      (int)H, (int)lstm, cur_stream());
}

void snake_step(torch::Tensor grid, torch::Tensor head_r,
                torch::Tensor head_c, torch::Tensor fruit_r,
                torch::Tensor fruit_c, torch::Tensor length,
                torch::Tensor action, torch::Tensor step_count,
                torch::Tensor ep_return, torch::Tensor ep_length,
                torch::Tensor last_ep_return, torch::Tensor last_ep_length,
                torch::Tensor obs_out, torch::Tensor next_obs_out,
                torch::Tensor reward_out, torch::Tensor discount_out,
                torch::Tensor steptype_out, torch::Tensor done_out,
                int64_t max_episode_steps, int64_t seed,
                torch::Tensor draw_buf, int64_t draw_offset,
                int64_t do_bump) {
  CHK(grid, torch::kInt32);
  CHK(head_r, torch::kInt64);
  CHK(action, torch::kInt64);
  CHK(length, torch::kInt32);
  int B = grid.size(0);
  launch_snake_step(
      grid.data_ptr<int>(), head_r.data_ptr<long>(), head_c.data_ptr<long>(),
      fruit_r.data_ptr<long>(), fruit_c.data_ptr<long>(),
      length.data_ptr<int>(), action.data_ptr<long>(),
      step_count.data_ptr<int>(), ep_return.data_ptr<float>(),
      ep_length.data_ptr<int>(), last_ep_return.data_ptr<float>(),
      last_ep_length.data_ptr<int>(), obs_out.data_ptr<float>(),
      next_obs_out.data_ptr<float>(), reward_out.data_ptr<float>(),
      discount_out.data_ptr<float>(),
      steptype_out.data_ptr<unsigned char>(),
      done_out.data_ptr<unsigned char>(), B, (int)max_episode_steps,
      (uint64_t)seed, draw_or_null(draw_buf), (unsigned int)draw_offset,
      (int)do_bump, cur_stream());
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("mcts_select", &mcts_select,
        "MCTS: PUCT descent of every tree to its expansion edge");
  m.def("mcts_expand_backup", &mcts_expand_backup,
        "MCTS: write the new node, link it and back its value up to the root");
  m.def("c51_loss_fwd", &c51_loss_fwd,
        "C51 categorical TD loss: softmax + fixed-order projection + CE");
  m.def("c51_loss_bwd", &c51_loss_bwd,
        "C51 categorical TD loss: analytic logits backward");
  m.def("qr_loss_fwd", &qr_loss_fwd,
        "QR-DQN quantile loss: selector argmax + target + all pairs, one "
        "pass giving the per-row loss and d loss / d source quantile");
  m.def("qr_loss_bwd", &qr_loss_bwd,
        "QR-DQN quantile loss: scatter of the saved gradient to [B, N, A]");
  m.def("tanh_normal_rsample_fwd", &tanh_normal_rsample_fwd,
        "tanh-squashed affine Gaussian: sample a, logp and the saved tanh(u)");
  m.def("tanh_normal_rsample_bwd", &tanh_normal_rsample_bwd,
        "tanh-squashed affine Gaussian: closed-form dloc and dscale");
  m.def("sac_critic_rows", &sac_critic_rows,
        "SAC: soft TD target, per-row twin-Q squared error and q_pred - target");
  m.def("sac_actor_rows", &sac_actor_rows,
        "SAC: per-row actor term, temperature dual term, argmin and entropy");
  m.def("sac_critic_rows_bwd", &sac_critic_rows_bwd,
        "SAC: dq_pred from the per-row gradient (sac_rows_bwd_kernel)");
  m.def("sac_actor_rows_bwd", &sac_actor_rows_bwd,
        "SAC: dq_new, dlogp_new and the rows of dlog_alpha (sac_rows_bwd_kernel)");
  m.def("noisy_linear_fwd", &noisy_linear_fwd,
        "NoisyLinear forward, the noisy weight formed while staging");
  m.def("noisy_linear_dgrad", &noisy_linear_dgrad,
        "NoisyLinear input gradient, optionally times act'(Z_prev)");
  m.def("noisy_linear_wgrad", &noisy_linear_wgrad,
        "NoisyLinear mu/sigma weight and bias gradients (split-S + reduce)");
  m.def("noise_transform", &noise_transform,
        "in-place f(x) = sign(x) sqrt(|x|) over the NoiseBank buffer");
  m.def("qens_linear_fwd", &qens_linear_fwd,
        "Q-ensemble dense layer forward, all members in one launch (fp32)");
  m.def("qens_linear_dgrad", &qens_linear_dgrad,
        "Q-ensemble input gradient, per member or summed over members");
  m.def("qens_linear_wgrad", &qens_linear_wgrad,
        "Q-ensemble weight and bias gradients (split-S + reduce)");
  m.def("actor_mlp_fwd", &actor_mlp_fwd,
        "Gaussian actor MLP forward, every layer and the head in one launch "
        "(fp32)");
  m.def("actor_mlp_dgrad", &actor_mlp_dgrad,
        "Gaussian actor MLP input-gradient chain in one launch: dZ of every "
        "layer and of the head");
  m.def("multi_adam_norm", &multi_adam_norm,
        "optimiser tail, launch A: ordered grad-norm partials and step + 1 "
        "for up to 4 chains of torch-owned tensors");
  m.def("multi_adam_update", &multi_adam_update,
        "optimiser tail, launch B: clip + Adam + polyak on the same table");
  m.def("snake_step", &snake_step,
        "fused Snake env step (dynamics + metrics + autoreset + render)");
  m.def("rnn_scan", &rnn_scan,
        "fused done-masked GRU/LSTM sequence scan (K13)");
  m.def("rnn_scan_train_fwd", &rnn_scan_train_fwd,
        "K13 training forward: rnn_scan + saved gates/aux for the backward");
  m.def("rnn_scan_bwd", &rnn_scan_bwd,
        "K13 backward through time: dXp, dHg, dh0/dc0 from dHout");
  m.def("policy_value_step_disc", &policy_value_step_disc,
        "fused actor+critic fwd, categorical Gumbel-max sample (MFMA)");
  m.def("ppo_head_loss_disc", &ppo_head_loss_disc,
        "categorical PPO losses + analytic logits backward");
  m.def("ppo_gather_disc", &ppo_gather_disc,
        "fused minibatch gather (int64 actions)");
  m.def("sumtree_update", &sumtree_update,
        "scatter leaf priorities + repair ancestors (device sum-tree)");
  m.def("sumtree_sample", &sumtree_sample,
        "stratified proportional sum-tree descent");
  m.def("cartpole_step", &env_step<long, launch_cartpole_step>,
        "fused CartPole env step");
  m.def("ant_step", &env_step<float, launch_ant_step>, "fused Ant env step");
  m.def("ant_reset", &ant_reset, "Ant reset");
  m.def("humanoid_step", &env_step<float, launch_humanoid_step>,
        "fused Humanoid env step");
  m.def("gae", &gae, "truncation-aware GAE reverse scan");
  m.def("lambda_returns", &lambda_returns, "lambda returns reverse scan");
  m.def("vtrace", &vtrace, "vtrace errors + pg advantage");
  m.def("offpolicy_returns", &offpolicy_returns, "retrace-style returns");
  m.def("fused_adam", &fused_adam, "fused global-norm-clip + Adam");
  m.def("fused_adam_bf16", &fused_adam_bf16,
        "fused clip + Adam, bf16 grads + bf16 param mirror");
  m.def("polyak", &polyak, "polyak target update");
  m.def("mfma_probe", &mfma_probe, "MFMA 16x16x32 bf16 layout probe");
  m.def("policy_value_step", &policy_value_step,
        "fused actor+critic fwd + tanh-normal sample (MFMA)");
  m.def("value_forward", &value_forward, "fused critic fwd (MFMA)");
  m.def("rollout_step_ant", &rollout_step_ant,
        "fused rollout step: policy + Ant physics + bootstrap, one launch");
  m.def("linear_silu", &linear_silu,
        "fused Linear(+bias)+SiLU forward, MFMA tiled");
  m.def("silu_fwd", &silu_fwd, "bf16 silu forward");
  m.def("silu_bwd", &silu_bwd, "bf16 silu backward");
  m.def("silu_heads_fwd", &silu_heads_fwd,
        "stacked silu forward fused with the actor/critic head GEMMs");
  m.def("heads_bwd_silu", &heads_bwd_silu,
        "head dgrads (K=16 / K=1) fused with the stacked silu backward");
  m.def("ppo_gather", &ppo_gather, "fused minibatch gather");
  m.def("ppo_head_loss", &ppo_head_loss,
        "fused PPO head fwd + losses + analytic head bwd");
  m.def("wgrad", &wgrad, "split-K MFMA weight grad + bias colsum -> slab",
        py::arg("dZ"), py::arg("X"), py::arg("slab"), py::arg("dW_off"),
        py::arg("db_off"), py::arg("n_valid"), py::arg("kpg") = 0,
        py::arg("ntb") = 0);
  m.def("slab_reduce", &slab_reduce,
        "sum wgrad slabs into flat bf16 grads (+ fused Adam prologue)");
  m.def("wgrad_pair", &wgrad_pair,
        "both nets' split-K wgrads in one pipelined launch -> slabs",
        py::arg("dZ0"), py::arg("X0"), py::arg("slab0"), py::arg("dW_off0"),
        py::arg("db_off0"), py::arg("n_valid0"), py::arg("dZ1"),
        py::arg("X1"), py::arg("slab1"), py::arg("dW_off1"),
        py::arg("db_off1"), py::arg("n_valid1"), py::arg("variant") = -1);
  m.def("wgrad_pair_act", &wgrad_pair_act,
        "layer-1 wgrad_pair with dZ = dH * silu'(Z) formed in the staging; "
        "false = not taken, nothing launched",
        py::arg("dH0"), py::arg("Z0"), py::arg("X0"), py::arg("slab0"),
        py::arg("dW_off0"), py::arg("db_off0"), py::arg("n_valid0"),
        py::arg("dH1"), py::arg("Z1"), py::arg("X1"), py::arg("slab1"),
        py::arg("dW_off1"), py::arg("db_off1"), py::arg("n_valid1"),
        py::arg("variant") = -1);
  m.def("ppo_gather_rows", &ppo_gather_rows,
        "ppo_gather / ppo_gather_disc for a whole epoch's rows in one "
        "launch; false = shape not taken, nothing launched");
  m.def("slab_reduce_pair", &slab_reduce_pair,
        "both chains' slabs -> flat bf16 grads, slabs left un-zeroed");
  m.def("linear_silu_pair", &linear_silu_pair,
        "both nets' Linear(+bias)+SiLU forward over one X, row-contiguous "
        "stores; false = shape not taken, nothing launched");
  m.def("linear_silu_heads_pair", &linear_silu_heads_pair,
        "both nets' layer-2 Linear(+bias)+SiLU and the heads in one launch, "
        "W2 held in LDS; false = shape not taken, nothing launched");
  m.def("slab_reduce_norm_pair", &slab_reduce_norm_pair,
        "slab_reduce_pair + each chain's ordered squared grad norm");
  m.def("adam_pair", &adam_pair,
        "both chains' clip + Adam + bf16 mirror in one launch");
  m.attr("TAIL_MAX_N") = kTailMaxN;
  m.def("bump_add", &bump_add, "add N to a device RNG draw counter");
  m.def("tr16_probe", &tr16_probe, "ds_read_tr16_b64 semantics probe");
}
