// The per-element double arithmetic of the soft actor-critic kernels (actor_critic.hip: soft_backup_kernel, soft_q_backup_kernel;
// dsact.hip: the critic losses and the sampling head), stated once.  The kernels differ in where the operands come from and where
// the results go; every value below is formed by the same expression in all of them, so they return the same bits.
// (dsact.hip's tanh_gauss_fwd_kernel writes tanh_gauss_dim's expressions out in place - see there - and must follow any change here.)
#pragma once
#include "gauss_math.h"   // HALF_LOG_2PI

__device__ __forceinline__ double softplus_d(double x) { return x > 20.0 ? x : log1p(exp(x)); }   // (torch's threshold)
__device__ __forceinline__ double softplus_grad_d(double x) { return x > 20.0 ? 1.0 : 1.0 / (1.0 + exp(-x)); }

// One action dimension of StochaPolicy's tanh-Gaussian head: std = exp(clamp(log std)), u = mean + std eps, the action
// half * tanh(u) + mid on [lo, hi] (unrounded) and the dimension's share of log pi(action):
//   Normal(mean, std).log_prob(u) - log(1 + 1e-6 - tanh(u)^2) - log(half)      (act_distribution_type.py:41-51)
struct TanhGaussDim {
    double act, logp;
};

__device__ __forceinline__ TanhGaussDim tanh_gauss_dim(double mean, double ls, double e, double lo, double hi, double min_ls,
                                                       double max_ls) {
    TanhGaussDim d;
    const double sd = exp(fmin(fmax(ls, min_ls), max_ls));
    const double u = mean + sd * e, th = tanh(u), du = u - mean;
    const double half = (hi - lo) / 2;
    d.act = half * th + (hi + lo) / 2;
    d.logp = (-(du * du) / (2 * sd * sd) - log(sd) - HALF_LOG_2PI) - log(1.0 + 1e-6 - th * th) - log(half);
    return d;
}
