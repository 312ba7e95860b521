// The elementwise stages of a DSAC-T update (gops/algorithm/dsact.py), and of a DSAC update, that sit between the MLP launches.
//
// dsact_loss_kernel: the variance-weighted critic losses and their gradient seeds with respect to the critics' RAW head outputs
//   (dsact.py:243-251, 284-313).  The seeds depend on the batch mean of std through the running mean_std (the 3 mean_std clamp and
//   the factor mean_std^2 + 0.1), so the kernel has two phases: (1) the batch moments - mean q_i, mean / min std_i - and the update
//   of mean_std in the device state; (2) seeds and losses.  Up to 8192 rows ONE block runs both in one launch; beyond that the
//   entry point issues TWO launches of 64 blocks (phase 1, then phase 2), each folding its blocks' partial sums in the block that
//   draws the last ticket.  Nothing waits on another workgroup.
// dsac_loss_kernel: DSAC's one-critic loss (gops/algorithm/dsac.py:235-252) and its seeds on the same two-phase scheme; the batch
//   mean of std enters through td_bound = 3 mean(std).
// tanh_gauss_fwd_kernel / tanh_gauss_bwd_kernel: StochaPolicy's sampling head - clamp, exp, u = mean + std eps, tanh squash,
//   log-probability - and its reverse, one thread per row; the forward reduces mean(logp), mean(tanh(mean)) and mean(std).  The
//   forward spells out soft_math.h's tanh_gauss_dim in place: through the helper it took four more registers.
// Every value is formed in double from the fp32 inputs and rounded once where it is stored; sums are doubles in the fixed order of
// block_reduce.h, which depends on B only.
#include <stdint.h>

#include "block_reduce.h"
#include "common.h"
#include "soft_math.h"

namespace {

constexpr int DS_BLOCKS = 64;
constexpr int DS_ONE_BLOCK_MAX = 8192;
constexpr int DS_RESULTS = 16;   // floats in front of the partial sums
constexpr int DS_PART = 6;       // doubles per block

__global__ __launch_bounds__(256) void dsact_loss_kernel(const float* __restrict__ qraw, const float* __restrict__ tq,
                                                         const float* __restrict__ tqs, int B, double tau_b, int phases,
                                                         GopsDsactState* __restrict__ st, float* __restrict__ seed,
                                                         float* __restrict__ stats) {
    __shared__ double red[DS_PART][4];
    __shared__ bool last;
    __shared__ float ms_sh[2];
    double* part = reinterpret_cast<double*>(stats + DS_RESULTS);   // [DS_BLOCKS][DS_PART]
    unsigned* ticket = reinterpret_cast<unsigned*>(stats + DS_RESULTS + 2 * DS_PART * DS_BLOCKS);
    const float* q2raw = qraw + (size_t)2 * B;
    if (phases & 1) {   // ---- batch moments, running mean_std (dsact.py:243-251) ----
        double s[4] = {0.0, 0.0, 0.0, 0.0};          // sum q1, sum q2, sum std1, sum std2
        double mn[2] = {INFINITY, INFINITY};          // min std1, min std2
        for (int i = blockIdx.x * 256 + threadIdx.x; i < B; i += gridDim.x * 256) {
            const double sd1 = softplus_d((double)qraw[2 * (size_t)i + 1]), sd2 = softplus_d((double)q2raw[2 * (size_t)i + 1]);
            s[0] += (double)qraw[2 * (size_t)i], s[1] += (double)q2raw[2 * (size_t)i], s[2] += sd1, s[3] += sd2;
            mn[0] = fmin(mn[0], sd1), mn[1] = fmin(mn[1], sd2);
        }
        block_fold<4, false>(s, red);
        block_fold<2, true>(mn, red);
        bool fin = gridDim.x == 1;
        if (!fin) {
            double v[6] = {s[0], s[1], s[2], s[3], mn[0], mn[1]};
            fin = last_block<6>(v, part, DS_PART, ticket, &last);
            if (fin) {
                double vs[4] = {v[0], v[1], v[2], v[3]};
                double vm[2] = {threadIdx.x < gridDim.x ? v[4] : INFINITY, threadIdx.x < gridDim.x ? v[5] : INFINITY};
                block_fold<4, false>(vs, red);
                block_fold<2, true>(vm, red);
                for (int i = 0; i < 4; ++i) s[i] = vs[i];
                mn[0] = vm[0], mn[1] = vm[1];
            }
        }
        if (fin && threadIdx.x == 0) {
            const double b1 = s[2] / (double)B, b2 = s[3] / (double)B;
            const bool init = st->initialised != 0u;
            const float ms1 = (float)(init ? (1.0 - tau_b) * (double)st->mean_std[0] + tau_b * b1 : b1);
            const float ms2 = (float)(init ? (1.0 - tau_b) * (double)st->mean_std[1] + tau_b * b2 : b2);
            st->mean_std[0] = ms1, st->mean_std[1] = ms2, st->initialised = 1u;
            ms_sh[0] = ms1, ms_sh[1] = ms2;
            stats[1] = (float)(s[0] / (double)B), stats[2] = (float)(s[1] / (double)B);
            stats[3] = (float)b1, stats[4] = (float)b2, stats[5] = (float)mn[0], stats[6] = (float)mn[1];
            stats[7] = ms1, stats[8] = ms2;
        }
        if (phases == 1) return;
        __syncthreads();   // one block ran phase 1: ms_sh is visible
    } else if (threadIdx.x == 0) {
        ms_sh[0] = st->mean_std[0], ms_sh[1] = st->mean_std[1];
    }
    if (!(phases & 1)) __syncthreads();
    // ---- seeds and losses (dsact.py:284-313): q and std stand for themselves in the loss, everything else is detached ----
    const double ms[2] = {(double)ms_sh[0], (double)ms_sh[1]};
    double l[2] = {0.0, 0.0};
    for (int i = blockIdx.x * 256 + threadIdx.x; i < B; i += gridDim.x * 256) {
        const double t = (double)tq[i], ts = (double)tqs[i];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const size_t at = 2 * ((size_t)c * B + i);
            const double q = (double)qraw[at], raw = (double)qraw[at + 1], sd = softplus_d(raw);
            const double bound = q + fmin(fmax(ts - q, -3.0 * ms[c]), 3.0 * ms[c]);      // target_q_bound
            const double wq = -(t - q) / (sd * sd + 0.1);
            const double ws = -((q - bound) * (q - bound) - sd * sd) / (sd * sd * sd + 0.1);
            const double fac = (ms[c] * ms[c] + 0.1) / (double)B;
            seed[at] = (float)(fac * wq);
            seed[at + 1] = (float)(fac * ws * softplus_grad_d(raw));
            l[c] += wq * q + ws * sd;
        }
    }
    if (grid_fold<2>(l, red, part, DS_PART, ticket, &last) && threadIdx.x == 0) {
        const float l1 = (float)((ms[0] * ms[0] + 0.1) * l[0] / (double)B), l2 = (float)((ms[1] * ms[1] + 0.1) * l[1] / (double)B);
        stats[0] = l1 + l2, stats[9] = l1, stats[10] = l2;
    }
}
static_assert(DS_RESULTS + 2 * DS_PART * DS_BLOCKS + 1 <= GOPS_DSACT_STATS_FLOATS, "stats: results, the blocks' partial sums, the ticket");

// ---- DSAC: the one-critic loss (gops/algorithm/dsac.py:235-252) ----------------------------------------------------------------------
// dsact_loss_kernel's scheme: phase 1 - mean q, mean std and td_bound = 3 mean(std), left in stats[1 .. 3] as fp32; phase 2 - seeds
// and the loss with td_bound read back from stats[3] (the same fp32 value in the one-launch and in the two-launch path).
constexpr int DC_RESULTS = 4;   // floats in front of the partial sums
constexpr int DC_PART = 2;      // doubles per block

__global__ __launch_bounds__(256) void dsac_loss_kernel(const float* __restrict__ qraw, const float* __restrict__ tq, int B, int bound,
                                                        int phases, float* __restrict__ seed, float* __restrict__ stats) {
    __shared__ double red[DC_PART][4];
    __shared__ bool last;
    __shared__ float td_sh;
    double* part = reinterpret_cast<double*>(stats + DC_RESULTS);   // [DS_BLOCKS][DC_PART]
    unsigned* ticket = reinterpret_cast<unsigned*>(stats + DC_RESULTS + 2 * DC_PART * DS_BLOCKS);
    if (phases & 1) {   // ---- batch moments, td_bound (dsac.py:243, 249) ----
        double s[2] = {0.0, 0.0};   // sum q, sum std
        for (int i = blockIdx.x * 256 + threadIdx.x; i < B; i += gridDim.x * 256)
            s[0] += (double)qraw[2 * (size_t)i], s[1] += softplus_d((double)qraw[2 * (size_t)i + 1]);
        if (grid_fold<2>(s, red, part, DC_PART, ticket, &last) && threadIdx.x == 0) {
            const float td = (float)(3.0 * (s[1] / (double)B));
            stats[1] = (float)(s[0] / (double)B), stats[2] = (float)(s[1] / (double)B), stats[3] = td;
            td_sh = td;
        }
        if (phases == 1) return;
        __syncthreads();   // one block ran phase 1: td_sh is visible
    } else {
        if (threadIdx.x == 0) td_sh = stats[3];
        __syncthreads();
    }
    // ---- seeds and loss (dsac.py:235-242): with `bound`, the first term is live in q, the second and third in std ----
    const double td = (double)td_sh;
    double l[1] = {0.0};
    for (int i = blockIdx.x * 256 + threadIdx.x; i < B; i += gridDim.x * 256) {
        const double q = (double)qraw[2 * (size_t)i], raw = (double)qraw[2 * (size_t)i + 1], sd = softplus_d(raw);
        const double e = (double)tq[i] - q;                            // target_q - q
        const double eb = bound ? fmin(fmax(e, -td), td) : e;          // target_q_bound - q
        const double v = sd * sd;
        seed[2 * (size_t)i] = (float)(-e / v / (double)B);
        seed[2 * (size_t)i + 1] = (float)((1.0 / sd - eb * eb / (v * sd)) * softplus_grad_d(raw) / (double)B);
        l[0] += bound ? e * e / (2 * v) + eb * eb / (2 * v) + log(sd) : e * e / (2 * v) + log(sd) + HALF_LOG_2PI;
    }
    if (grid_fold<1>(l, red, part, DC_PART, ticket, &last) && threadIdx.x == 0) stats[0] = (float)(l[0] / (double)B);
}
static_assert(DC_RESULTS + 2 * DC_PART * DS_BLOCKS + 1 <= GOPS_DSAC_STATS_FLOATS, "stats: results, the blocks' partial sums, the ticket");

// ---- the sampling head ----------------------------------------------------------------------------------------------------------
struct TgParams {
    int B, A;
    float low[GOPS_MAX_ACT], high[GOPS_MAX_ACT];
    double min_ls, max_ls;
};

__global__ __launch_bounds__(256) void tanh_gauss_fwd_kernel(const TgParams p, const float* __restrict__ head, const float* __restrict__ eps,
                                                             double target_entropy, float* __restrict__ act, float* __restrict__ logp,
                                                             float* __restrict__ stats) {
    __shared__ double red[3][4];
    __shared__ bool last;
    const int A = p.A;
    double s[3] = {0.0, 0.0, 0.0};   // sum logp, sum tanh(mean), sum std
    for (int i = blockIdx.x * 256 + threadIdx.x; i < p.B; i += gridDim.x * 256) {
        const float* h = head + (size_t)i * 2 * A;
        double lp = 0.0;
        for (int a = 0; a < A; ++a) {
            const double mean = (double)h[a], sd = exp(fmin(fmax((double)h[A + a], p.min_ls), p.max_ls));
            const double u = mean + sd * (double)eps[(size_t)i * A + a], th = tanh(u), du = u - mean;
            const double half = ((double)p.high[a] - (double)p.low[a]) / 2;
            act[(size_t)i * A + a] = (float)(half * th + ((double)p.high[a] + (double)p.low[a]) / 2);
            lp += (-(du * du) / (2 * sd * sd) - log(sd) - HALF_LOG_2PI) - log(1.0 + 1e-6 - th * th) - log(half);   // soft_math.h: tanh_gauss_dim
            s[1] += tanh(mean), s[2] += sd;
        }
        logp[i] = (float)lp;
        s[0] += lp;
    }
    double* part = reinterpret_cast<double*>(stats + 4);   // [DS_BLOCKS][DS_PART]
    if (grid_fold<3>(s, red, part, DS_PART, reinterpret_cast<unsigned*>(stats + 4 + 2 * DS_PART * DS_BLOCKS), &last) && threadIdx.x == 0) {
        const double mlp = s[0] / (double)p.B, n = (double)p.B * (double)A;
        stats[0] = (float)mlp, stats[1] = (float)(s[1] / n), stats[2] = (float)(s[2] / n);
        stats[3] = (float)(-(mlp + target_entropy));   // d loss_alpha / d log_alpha (dsact.py:323-329)
    }
}
static_assert(4 + 2 * DS_PART * DS_BLOCKS + 1 <= GOPS_TANH_GAUSS_STATS_FLOATS, "stats: four results, the blocks' partial sums, the ticket");

__global__ __launch_bounds__(256) void tanh_gauss_bwd_kernel(const TgParams p, const float* __restrict__ head, const float* __restrict__ eps,
                                                             const float* __restrict__ g_act, const float* __restrict__ g_logp,
                                                             float* __restrict__ g_head) {
    const int A = p.A;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < p.B; i += gridDim.x * 256) {
        const float* h = head + (size_t)i * 2 * A;
        const double gl = (double)g_logp[i];
        for (int a = 0; a < A; ++a) {
            const double ls = (double)h[A + a];
            const bool inside = ls >= p.min_ls && ls <= p.max_ls;   // (the clamp passes its gradient on the closed interval, as torch's)
            const double sd = exp(fmin(fmax(ls, p.min_ls), p.max_ls)), e = (double)eps[(size_t)i * A + a];
            const double th = tanh((double)h[a] + sd * e), sech2 = 1.0 - th * th;
            const double half = ((double)p.high[a] - (double)p.low[a]) / 2;
            // d act / d u = half (1 - th^2);  d logp / d u = 2 th (1 - th^2) / (1 + 1e-6 - th^2);  the Gaussian term is -eps^2 / 2 - log std
            const double gu = (double)g_act[(size_t)i * A + a] * half * sech2 + gl * 2.0 * th * sech2 / (1.0 + 1e-6 - th * th);
            g_head[(size_t)i * 2 * A + a] = (float)gu;
            g_head[(size_t)i * 2 * A + A + a] = inside ? (float)(gu * e * sd - gl) : 0.f;
        }
    }
}

inline unsigned ds_grid(int B) { return B <= DS_ONE_BLOCK_MAX ? 1u : (unsigned)DS_BLOCKS; }

TgParams tg_params(const GopsTanhGauss& d, int B) {
    TgParams p;
    p.B = B, p.A = d.act_dim;
    for (int a = 0; a < GOPS_MAX_ACT; ++a) p.low[a] = d.act_low[a], p.high[a] = d.act_high[a];
    p.min_ls = d.min_log_std, p.max_ls = d.max_log_std;
    return p;
}

bool tanh_gauss_ok(const GopsTanhGauss* d, int B) { return d && B >= 1 && d->act_dim >= 1 && d->act_dim <= GOPS_MAX_ACT; }

}  // namespace

extern "C" {

int gops_dsact_critic_loss(const float* qraw, const float* tq, const float* tqs, int32_t B, double tau_b, GopsDsactState* st, float* seed,
                           float* stats, void* stream) {
    if (!qraw || !tq || !tqs || !st || !seed || !stats || B < 1) return GOPS_ERR_BAD_ARG;
    if (!stats_aligned(stats)) return GOPS_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (B <= DS_ONE_BLOCK_MAX) {
        hipLaunchKernelGGL(dsact_loss_kernel, dim3(1), dim3(256), 0, s, qraw, tq, tqs, B, tau_b, 3, st, seed, stats);
    } else {
        hipLaunchKernelGGL(dsact_loss_kernel, dim3(DS_BLOCKS), dim3(256), 0, s, qraw, tq, tqs, B, tau_b, 1, st, seed, stats);
        hipLaunchKernelGGL(dsact_loss_kernel, dim3(DS_BLOCKS), dim3(256), 0, s, qraw, tq, tqs, B, tau_b, 2, st, seed, stats);
    }
    return (int)hipGetLastError();
}

int gops_dsac_critic_loss(const float* qraw, const float* tq, int32_t B, int32_t bound, float* seed, float* stats, void* stream) {
    if (!qraw || !tq || !seed || !stats || B < 1) return GOPS_ERR_BAD_ARG;
    if (!stats_aligned(stats)) return GOPS_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (B <= DS_ONE_BLOCK_MAX) {
        hipLaunchKernelGGL(dsac_loss_kernel, dim3(1), dim3(256), 0, s, qraw, tq, B, bound != 0, 3, seed, stats);
    } else {
        hipLaunchKernelGGL(dsac_loss_kernel, dim3(DS_BLOCKS), dim3(256), 0, s, qraw, tq, B, bound != 0, 1, seed, stats);
        hipLaunchKernelGGL(dsac_loss_kernel, dim3(DS_BLOCKS), dim3(256), 0, s, qraw, tq, B, bound != 0, 2, seed, stats);
    }
    return (int)hipGetLastError();
}

int gops_tanh_gauss_forward(const GopsTanhGauss* d, int32_t B, const float* head, const float* eps, double target_entropy, float* act,
                            float* logp, float* stats, void* stream) {
    if (!tanh_gauss_ok(d, B) || !head || !eps || !act || !logp || !stats) return GOPS_ERR_BAD_ARG;
    if (!stats_aligned(stats)) return GOPS_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(tanh_gauss_fwd_kernel, dim3(ds_grid(B)), dim3(256), 0, s, tg_params(*d, B), head, eps, target_entropy, act, logp, stats);
    return (int)hipGetLastError();
}

int gops_tanh_gauss_backward(const GopsTanhGauss* d, int32_t B, const float* head, const float* eps, const float* g_act,
                             const float* g_logp, float* g_head, void* stream) {
    if (!tanh_gauss_ok(d, B) || !head || !eps || !g_act || !g_logp || !g_head) return GOPS_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(tanh_gauss_bwd_kernel, dim3(ds_grid(B)), dim3(256), 0, s, tg_params(*d, B), head, eps, g_act, g_logp, g_head);
    return (int)hipGetLastError();
}

}  // extern "C"
