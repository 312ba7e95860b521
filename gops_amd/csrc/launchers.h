// What one kernel source calls in another: included by both sides, so that a signature is written once.  (The rollout kernels'
// launchers: rollout_choice.h; the weight-gradient stage's launch_dw: dw_plan.h.)  The C entry points of include/gops_hip.h are not
// here: each is defined once, with all of its argument checks, in the source that holds its kernels - gops_rollout_* / gops_value_* /
// gops_mlp_* / gops_dw_plan_query / gops_hip_version / gops_profile_* in api.hip, every other family beside its kernels.
#pragma once
#include "common.h"
#include "dw_plan.h"

// ---- prologue.hip: parameter upload, weight packing, reference tables ----
hipError_t launch_upload_params(const RolloutParams& p, RolloutParams* dst, hipStream_t s);
hipError_t launch_prologue(const RolloutParams& p, RolloutParams* dst, int P, float pdt, hipStream_t s);

// ---- dw_gemm.hip: the fixed-order reduce of split-K slabs (also the partials of rollout_poly.hip, rollout_rbf.hip, rollout_lips.hip) ----
hipError_t launch_reduce(const ReduceJobs& jobs, hipStream_t s);

// ---- optim.hip: the loss scalars of a batch (dw_gemm.hip: the loss mean that rides on a reduce) ----
hipError_t launch_batch_loss(const float* a, const float* b, int n, float gsc, float sc0, float* grad, float* stats, hipStream_t s);

// ---- aux_kernels.hip: any-width output layer, zero fill ----
hipError_t launch_linear_out_fwd(const float* h, int K, const float* Wo, const float* bo, int W, int B, float* y, hipStream_t s);
hipError_t launch_linear_out_bwd(const float* gy, int W, int Wp, const float* Wo, int K, int B, long long S, float* gh,
                                 float* gyp, hipStream_t s);
hipError_t launch_fill_zero(float* p, size_t n, hipStream_t s);

// ---- actor_critic.hip: the nets the tile kernels take - fp32, 1 .. 3 hidden layers of widths that are multiples of 16 up to 256
// (trpo.hip's fisher_seed_kernel accepts the same) ----
int ac_check_net(const GopsMlp& m, int in, int out);
