// The per-dimension double arithmetic of a diagonal Gaussian on a policy's RAW head (mean, raw log std), stated once for the
// on-policy kernels (ppo.hip: ppo_loss_kernel; trpo.hip: trpo_surrogate_kernel and the head of fisher_seed_kernel).  The kernels
// differ in where the operands come from and where the results go; every value below is formed by the same expression in all of
// them, so they return the same bits.  A header of its own, under soft_math.h: the tanh-Gaussian head there builds on a Gaussian,
// not the other way round, and the on-policy kernels need nothing else of the soft actor-critic family's.
// (soft_math.h's tanh_gauss_dim subtracts log(sd), not the clamped log std: a different expression, not formed from these.)
#pragma once

constexpr double HALF_LOG_2PI = 0.91893853320467274178;   // log(sqrt(2 pi)): the constant of a normal density's logarithm

// One dimension of the clamped head: ls = clamp(raw), sd = exp(ls); `inside`: the clamp passes its gradient (on the closed
// interval, as torch's).
struct GaussDim {
    double ls, sd;
    bool inside;
};

__device__ __forceinline__ GaussDim gauss_dim(double raw, double min_ls, double max_ls) {
    GaussDim g;
    g.ls = fmin(fmax(raw, min_ls), max_ls);
    g.sd = exp(g.ls);
    g.inside = raw >= min_ls && raw <= max_ls;
    return g;
}

// The dimension's share of log N(x; mean, sd), d = x - mean.
__device__ __forceinline__ double gauss_logp_term(double d, double ls, double sd) { return -(d * d) / (2 * sd * sd) - ls - HALF_LOG_2PI; }

// The dimension's share of KL(p || q).
__device__ __forceinline__ double gauss_kl_term(double ls_p, double sd_p, double m_p, double ls_q, double sd_q, double m_q) {
    return ls_q - ls_p + (sd_p * sd_p + (m_p - m_q) * (m_p - m_q)) / (2 * sd_q * sd_q) - 0.5;
}

// g d logp / d (mean, raw log std) of the dimension: d = x - mean, iv = 1 / sd^2.
struct GaussSeed {
    double mean, ls;
};

__device__ __forceinline__ GaussSeed gauss_logp_seed(double g, double d, double iv, bool inside) {
    GaussSeed s;
    s.mean = g * d * iv;
    s.ls = inside ? g * (d * d * iv - 1.0) : 0.0;
    return s;
}
