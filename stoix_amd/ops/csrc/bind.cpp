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
  m.def("slab_reduce_pair", &slab_reduce_pair,
        "both chains' slabs -> flat bf16 grads, slabs left un-zeroed");
  m.def("linear_silu_pair", &linear_silu_pair,
        "both nets' Linear(+bias)+SiLU forward over one X, row-contiguous "
        "stores; false = shape not taken, nothing launched");
  m.def("slab_reduce_norm_pair", &slab_reduce_norm_pair,
        "slab_reduce_pair + each chain's ordered squared grad norm");
  m.def("adam_pair", &adam_pair,
        "both chains' clip + Adam + bf16 mirror in one launch");
  m.attr("TAIL_MAX_N") = kTailMaxN;
  m.def("bump_add", &bump_add, "add N to a device RNG draw counter");
  m.def("tr16_probe", &tr16_probe, "ds_read_tr16_b64 semantics probe");
}
