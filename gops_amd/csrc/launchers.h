// Host entry points of every kernel source but the rollout kernels' as api.hip calls them: included by both sides, so that a
// signature is written once.  (The rollout kernels' launchers: rollout_choice.h.)
#pragma once
#include "common.h"
#include "dw_plan.h"

// ---- prologue.hip: parameter upload, weight packing, reference tables ----
hipError_t launch_upload_params(const RolloutParams& p, RolloutParams* dst, hipStream_t s);
hipError_t launch_prologue(const RolloutParams& p, RolloutParams* dst, int P, float pdt, hipStream_t s);

// ---- dw_gemm.hip: the weight-gradient stage (its record and launch_dw: dw_plan.h) ----
hipError_t launch_reduce(const ReduceJobs& jobs, hipStream_t s);

// ---- optim.hip: Adam, Polyak averaging, loss scalars ----
hipError_t launch_polyak(const GopsAdamTensors& T, float omt, float tau, hipStream_t s);
hipError_t launch_batch_loss(const float* a, const float* b, int n, float gsc, float sc0, float* grad, float* stats, hipStream_t s);
hipError_t launch_adam(const GopsAdamTensors& T, GopsAdamState* st, double beta1, double beta2, float eps, hipStream_t s);

// ---- aux_kernels.hip: any-width output layer, zero fill, single env step / constraint ----
hipError_t launch_linear_out_fwd(const float* h, int K, const float* Wo, const float* bo, int W, int B, float* y, hipStream_t s);
hipError_t launch_linear_out_bwd(const float* gy, int W, int Wp, const float* Wo, int K, int B, long long S, float* gh,
                                 float* gyp, hipStream_t s);
hipError_t launch_fill_zero(float* p, size_t n, hipStream_t s);
hipError_t launch_env_step(const GopsEnv& env, int B, const GopsStepIO& io, float pdt, hipStream_t s);
hipError_t launch_env_constraint(const GopsEnv& env, int B, const GopsStepIO& io, hipStream_t s);

// ---- rollout_poly.hip: POLY approximators, one lane per trajectory ----
size_t poly_rollout_workspace_bytes(const GopsRolloutDesc& d);
int poly_rollout_forward(const GopsRolloutDesc& d, const GopsRolloutIn& in, const GopsRolloutOut& out, void* ws, size_t bytes, hipStream_t s);
int poly_rollout_backward(const GopsRolloutDesc& d, const float* grad_v, const GopsMlpGrad& g, void* ws, size_t bytes, hipStream_t s);
size_t poly_value_workspace_bytes(const GopsMlp& v, int B);
int poly_value_forward(const GopsMlp& v, int B, const float* obs, float* out, hipStream_t s);
int poly_value_backward(const GopsMlp& v, int B, const float* obs, const float* grad_v, const GopsMlpGrad& g, void* ws, size_t bytes,
                        hipStream_t s);

// ---- rollout_rpi.hip: RPI's policy evaluation, one workgroup, one lane per batch row ----
size_t rpi_state_bytes(int kind, int B);
int rpi_evaluate(int kind, int B, int max_steps, const float* consts, float* w, const float* wt, const float* max_step,
                 const float* pool, void* state, size_t state_bytes, double lr, double beta1, double beta2, double eps, float* result,
                 float* trace, hipStream_t s);

// ---- rollout_rpi_mlp.hip: the same with an MLP value net, one workgroup, batch rows in tiles of 64 ----
size_t rpi_mlp_state_bytes(int kind, int B, const GopsMlp* v);
int rpi_mlp_evaluate(int kind, int B, int max_steps, const float* consts, const GopsMlp* v, const GopsMlp* t, const float* max_step,
                     const float* pool, void* state, size_t state_bytes, double lr, double beta1, double beta2, double eps,
                     float* result, float* trace, hipStream_t s);

// ---- rollout_episode.hip: closed-loop evaluation episodes, 16 per workgroup, every step in one launch ----
size_t episode_workspace_bytes(const GopsEnv* env, const GopsMlp* policy, int E, int T);
int episode_rollout(const GopsEnv* env, const GopsMlp* policy, int E, int T, const GopsStepIO* init, const GopsEpisodeOut* out, void* ws,
                    size_t ws_bytes, float pdt, hipStream_t s);

// ---- rollout_lips.hip: LipsNet policies - an MLP with its input Jacobian, forward and reverse, a tile of samples per workgroup ----
size_t lips_workspace_bytes(const GopsLipsNet& d, int B);
int lips_forward(const GopsLipsNet& d, int B, const float* obs, float* action, float* K, float* N, void* ws, size_t bytes, hipStream_t s);
int lips_backward(const GopsLipsNet& d, int B, const float* obs, const float* grad_action, const GopsLipsGrad& g, void* ws, size_t bytes,
                  hipStream_t s);

// ---- actor_critic.hip: the no-grad half of a DDPG / TD3 update - Bellman backup in one launch, critic losses in one launch ----
size_t ac_backup_workspace_bytes(const GopsAcBackup* d, int B);
int ac_backup(const GopsAcBackup* d, int B, const float* obs2, const float* rew, const float* done, const float* xi, float* backup,
              float* a2, float* q_targ, void* ws, size_t ws_bytes, hipStream_t s);
int ac_critic_loss(const float* q, const float* backup, const float* weight, int nq, int B, float* seed, float* abs_err, float* stats,
                   hipStream_t s);
size_t soft_backup_workspace_bytes(const GopsSoftBackup* d, int B);
int soft_backup(const GopsSoftBackup* d, int B, const float* obs2, const float* rew, const float* done, const float* eps, const float* z,
                float* tq, float* tqs, float* a2, float* logp, float* q_targ, void* ws, size_t ws_bytes, hipStream_t s);
size_t soft_q_backup_workspace_bytes(const GopsSoftQBackup* d, int B);
int soft_q_backup(const GopsSoftQBackup* d, int B, const float* obs2, const float* rew, const float* done, const float* eps, const float* z,
                  float* backup, float* a2, float* logp, float* q_targ, void* ws, size_t ws_bytes, hipStream_t s);
size_t dqn_backup_workspace_bytes(const GopsDqnBackup* d, int B);
int dqn_backup(const GopsDqnBackup* d, int B, const float* obs2, const float* rew, const float* done, float* backup, float* q_targ,
               int* a_star, void* ws, size_t ws_bytes, hipStream_t s);
int dqn_loss(const float* q_all, const float* act, const float* backup, const float* weight, int N, int B, float* seed, float* abs_err,
             float* stats, hipStream_t s);

// (the nets the tile kernels take: fp32, 1 .. 3 hidden layers of widths that are multiples of 16 up to 256; also trpo.hip's)
int ac_check_net(const GopsMlp& m, int in, int out);

// ---- trpo.hip: the Fisher-vector product's tangent forward, TRPO's surrogate with the line search's verdict, conjugate gradients ----
int gauss_fisher_seed(const GopsMlp& m, const GopsMlpGrad& tangent, int B, const float* x, double min_ls, double max_ls, float* seed,
                      hipStream_t s);
int trpo_surrogate(int M, int A, double min_ls, double max_ls, const float* head_new, const float* head_old, const float* act,
                   const float* adv, const float* hyper, float* seed, float* stats, hipStream_t s);
int cg_init(const float* g, float* x, float* r, float* p, int n, double atol, GopsCgState* st, hipStream_t s);
int cg_step(float* p, float* Ap, float* x, float* r, int n, double damping, double atol, GopsCgState* st, hipStream_t s);
int cg_finish(const float* g, const float* x, float* step, int n, const float* hyper, GopsCgState* st, hipStream_t s);

// ---- dsact.hip: DSAC-T's and DSAC's critic losses with their seeds, and the tanh-Gaussian sampling head forward and reverse ----
int dsact_critic_loss(const float* qraw, const float* tq, const float* tqs, int B, double tau_b, GopsDsactState* st, float* seed,
                      float* stats, hipStream_t s);
int dsac_critic_loss(const float* qraw, const float* tq, int B, int bound, float* seed, float* stats, hipStream_t s);
int tanh_gauss_forward(const GopsTanhGauss& d, int B, const float* head, const float* eps, double target_entropy, float* act, float* logp,
                       float* stats, hipStream_t s);
int tanh_gauss_backward(const GopsTanhGauss& d, int B, const float* head, const float* eps, const float* g_act, const float* g_logp,
                        float* g_head, hipStream_t s);

// ---- ppo.hip: PPO's losses with their seeds, the advantage normalisation, GAE over all environments ----
int ppo_loss(const GopsPpoLoss& d, int M, const float* head_new, const float* v_new, const float* act, const float* logp_old, const float* adv,
             const float* ret, const float* val_old, const float* logits_old, const float* hyper, float* seed_head, float* seed_v, float* stats,
             hipStream_t s);
int adv_normalize(const float* adv, int n, double eps, float* out, float* stats, hipStream_t s);
int gae(const float* rew, const float* val, const float* val_next, const float* done, const float* end, int T, int N, double gamma,
        double lambda, float* ret, float* adv, hipStream_t s);
