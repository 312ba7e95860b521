// The elementwise stages of a PPO update (gops/algorithm/ppo.py) and of the on-policy sampler (gops/trainer/sampler/on_sampler.py)
// that sit between the MLP launches.
//
// ppo_loss_kernel: the clipped-surrogate, value, entropy and KL terms of ppo.py:167-240 and the gradient seeds of loss_total with
//   respect to the policy's RAW head (mean, log_std) and the value output.  loss_value_norm divides by 6 std(ret) of the minibatch,
//   which the seeds need: dsac_loss_kernel's two-phase scheme - phase 1 the moments of ret, phase 2 seeds and sums.  Up to
//   LOSS_ONE_BLOCK_MAX rows ONE block runs both in one launch; beyond that the entry point issues TWO launches of 64 blocks, each
//   folding its blocks' partial sums in the block that draws the last ticket.  Without loss_value_norm: phase 2 alone, one launch.
// adv_normalize_kernel: (adv - mean) / (std + eps) with the unbiased std (ppo.py:123-125) on the same scheme.
// gae_kernel: on_sampler.py:168-187 for every environment at once, one lane per environment walking T steps backwards.
// Every value is formed in double from the fp32 inputs and rounded once where it is stored - the Gaussian head's terms by
// gauss_math.h's expressions, which trpo.hip shares; sums are doubles in the fixed order of block_reduce.h's grid_fold, which
// depends on the row count only.  Nothing waits on another workgroup.
//
// Ties (torch's rules, see include/gops_hip.h): min(sur1, sur2) passes the surrogate's gradient where sur1 <= sur2 - inside the clip
// the two are the same number and clamp passes its gradient on the closed interval; max(l1, l2) passes the value's gradient where
// l1 >= l2 or the value clamp is idle.
#include <stdint.h>

#include "block_reduce.h"
#include "common.h"
#include "gauss_math.h"

namespace {

constexpr int PPO_BLOCKS = 64;
constexpr int PPO_RESULTS = 8;    // floats in front: the six results, two spare
constexpr int PPO_NORM_AT = 8;    // one double behind them: 6 std(ret)
constexpr int PPO_PART_AT = 10;   // the blocks' partial sums
constexpr int PPO_PART = 5;       // doubles per block

struct PpoParams {
    int M, A, value_clip, value_norm;
    double min_ls, max_ls;
};

// Shifted moments of x[0 .. n): s[0] = sum (x - x[0]), s[1] = sum (x - x[0])^2 - the pivot keeps the variance's subtraction benign.
__device__ __forceinline__ void shifted_moments(const float* x, int n, double (&s)[2]) {
    const double x0 = (double)x[0];
    s[0] = 0.0, s[1] = 0.0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const double d = (double)x[i] - x0;
        s[0] += d, s[1] += d * d;
    }
}

__device__ __forceinline__ double unbiased_std(const double (&s)[2], int n) {
    return sqrt(fmax(s[1] - s[0] * s[0] / (double)n, 0.0) / (double)(n - 1));
}

// Phase 1 of both two-phase normalisers: the grid's shifted moments of x[0 .. n); true where they are final (block_reduce.h: grid_fold).
__device__ __forceinline__ bool grid_moments(const float* x, int n, double (&s)[2], double (*red)[4], double* part, int stride,
                                             unsigned* ticket, bool* last) {
    shifted_moments(x, n, s);
    return grid_fold<2>(s, red, part, stride, ticket, last);
}

__global__ __launch_bounds__(256) void ppo_loss_kernel(const PpoParams p, int phases, const float* __restrict__ head, const float* __restrict__ v_new,
                                                       const float* __restrict__ act, const float* __restrict__ logp_old,
                                                       const float* __restrict__ adv, const float* __restrict__ ret,
                                                       const float* __restrict__ val_old, const float* __restrict__ logits_old,
                                                       const float* __restrict__ hyper, float* __restrict__ seed_head,
                                                       float* __restrict__ seed_v, float* __restrict__ stats) {
    __shared__ double red[PPO_PART][4];
    __shared__ bool last;
    __shared__ double norm_sh;
    double* norm_at = reinterpret_cast<double*>(stats + PPO_NORM_AT);
    double* part = reinterpret_cast<double*>(stats + PPO_PART_AT);   // [PPO_BLOCKS][PPO_PART]
    unsigned* ticket = reinterpret_cast<unsigned*>(stats + PPO_PART_AT + 2 * PPO_PART * PPO_BLOCKS);
    const int M = p.M, A = p.A;
    if (phases & 1) {   // ---- 6 std(ret) over the minibatch (ppo.py:207-209) ----
        double s[2];
        if (grid_moments(ret, M, s, red, part, PPO_PART, ticket, &last) && threadIdx.x == 0) {
            const double n6 = 6.0 * unbiased_std(s, M);
            *norm_at = n6, norm_sh = n6;
        }
        if (phases == 1) return;
        __syncthreads();   // one block ran phase 1: norm_sh is visible
    } else {
        if (threadIdx.x == 0) norm_sh = p.value_norm ? *norm_at : 1.0;
        __syncthreads();
    }
    // ---- seeds and sums (ppo.py:178-226) ----
    const double norm = norm_sh;
    const double clip = (double)hyper[0], vclip = (double)hyper[1], c_kl = (double)hyper[2], c_v = (double)hyper[3], c_ent = (double)hyper[4];
    const double inv_m = 1.0 / (double)M;
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};   // sum sur, value_loss, entropy, kl, clipped
    for (int i = blockIdx.x * 256 + threadIdx.x; i < M; i += gridDim.x * 256) {
        const float* h = head + (size_t)i * 2 * A;
        const float* lo = logits_old + (size_t)i * 2 * A;
        double lp = 0.0, ent = 0.0, kl = 0.0;
        for (int a = 0; a < A; ++a) {
            const double mean = (double)h[a];
            const GaussDim n = gauss_dim((double)h[A + a], p.min_ls, p.max_ls);
            const double d = (double)act[(size_t)i * A + a] - mean, mo = (double)lo[a], so = (double)lo[A + a];
            lp += gauss_logp_term(d, n.ls, n.sd);
            ent += 0.5 + HALF_LOG_2PI + n.ls;
            kl += gauss_kl_term(log(so), so, mo, n.ls, n.sd, mean);   // KL(N(old) || N(new))
        }
        const double ratio = exp(lp - (double)logp_old[i]), ad = (double)adv[i];
        const double sur1 = ratio * ad, sur2 = fmin(fmax(ratio, 1.0 - clip), 1.0 + clip) * ad;
        const double g_lp = sur1 <= sur2 ? -inv_m * ad * ratio : 0.0;   // d loss_total / d logp_new of the row
        for (int a = 0; a < A; ++a) {
            const GaussDim n = gauss_dim((double)h[A + a], p.min_ls, p.max_ls);
            const double mean = (double)h[a], iv = 1.0 / (n.sd * n.sd);
            const double d = (double)act[(size_t)i * A + a] - mean, mo = (double)lo[a], so = (double)lo[A + a];
            const double q = (so * so + (mo - mean) * (mo - mean)) * iv;
            const GaussSeed g = gauss_logp_seed(g_lp, d, iv, n.inside);
            seed_head[(size_t)i * 2 * A + a] = (float)(g.mean + c_kl * inv_m * (mean - mo) * iv);
            seed_head[(size_t)i * 2 * A + A + a] = n.inside ? (float)(g.ls + c_kl * inv_m * (1.0 - q) - c_ent * inv_m) : 0.f;
        }
        const double v = (double)v_new[i], r = (double)ret[i], vo = (double)val_old[i];
        const double l1 = (v - r) * (v - r);
        double vl = l1;
        bool live = true;
        if (p.value_clip) {
            const double vc = vo + fmin(fmax(v - vo, -vclip), vclip), l2 = (vc - r) * (vc - r);
            vl = fmax(l1, l2);
            live = l1 >= l2 || fabs(v - vo) <= vclip;
        }
        seed_v[i] = live ? (float)(2.0 * c_v * inv_m * (v - r) / norm) : 0.f;
        s[0] += fmin(sur1, sur2), s[1] += vl, s[2] += ent, s[3] += kl, s[4] += fabs(ratio - 1.0) > clip ? 1.0 : 0.0;
    }
    if (grid_fold<5>(s, red, part, PPO_PART, ticket, &last) && threadIdx.x == 0) {
        const double l_sur = -s[0] * inv_m, l_v = s[1] * inv_m / norm, ent = s[2] * inv_m, kl = s[3] * inv_m;
        stats[0] = (float)(l_sur + c_kl * kl + c_v * l_v - c_ent * ent);
        stats[1] = (float)l_sur, stats[2] = (float)l_v, stats[3] = (float)ent, stats[4] = (float)kl, stats[5] = (float)(s[4] * inv_m);
    }
}
static_assert(PPO_PART_AT + 2 * PPO_PART * PPO_BLOCKS + 1 <= GOPS_PPO_STATS_FLOATS, "stats: results, the norm, the blocks' partial sums, the ticket");
static_assert(PPO_RESULTS == PPO_NORM_AT && PPO_NORM_AT % 2 == 0 && PPO_PART_AT % 2 == 0, "the doubles behind the results are 8-byte aligned");

// ---- advantage normalisation (ppo.py:123-125) ----------------------------------------------------------------------------------
constexpr int AN_MOMENTS_AT = 2;   // two doubles behind the two results: mean, std
constexpr int AN_PART_AT = 6;
constexpr int AN_PART = 2;

// (x and out may be the same array: every read of phase 1 precedes a barrier, phase 2 reads an element only to write it)
__global__ __launch_bounds__(256) void adv_normalize_kernel(const float* x, int n, double eps, int phases, float* out, float* __restrict__ stats) {
    __shared__ double red[AN_PART][4];
    __shared__ bool last;
    __shared__ double mom_sh[2];
    double* mom_at = reinterpret_cast<double*>(stats + AN_MOMENTS_AT);
    double* part = reinterpret_cast<double*>(stats + AN_PART_AT);   // [PPO_BLOCKS][AN_PART]
    unsigned* ticket = reinterpret_cast<unsigned*>(stats + AN_PART_AT + 2 * AN_PART * PPO_BLOCKS);
    if (phases & 1) {
        double s[2];
        const double x0 = (double)x[0];
        if (grid_moments(x, n, s, red, part, AN_PART, ticket, &last) && threadIdx.x == 0) {
            const double mean = x0 + s[0] / (double)n, sd = unbiased_std(s, n);
            mom_at[0] = mean, mom_at[1] = sd, mom_sh[0] = mean, mom_sh[1] = sd;
            stats[0] = (float)mean, stats[1] = (float)sd;
        }
        if (phases == 1) return;
        __syncthreads();
    } else {
        if (threadIdx.x == 0) mom_sh[0] = mom_at[0], mom_sh[1] = mom_at[1];
        __syncthreads();
    }
    const double mean = mom_sh[0], den = mom_sh[1] + eps;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) out[i] = (float)(((double)x[i] - mean) / den);
}
static_assert(AN_PART_AT + 2 * AN_PART * PPO_BLOCKS + 1 <= GOPS_ADV_STATS_FLOATS, "stats: results, the moments, the blocks' partial sums, the ticket");

// ---- generalised advantage estimation (on_sampler.py:168-187) --------------------------------------------------------------------
__global__ __launch_bounds__(256) void gae_kernel(const float* __restrict__ rew, const float* __restrict__ val, const float* __restrict__ val_next,
                                                  const float* __restrict__ done, const float* __restrict__ end, int T, int N, double gamma,
                                                  double lambda, float* __restrict__ ret, float* __restrict__ adv) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    double gae = 0.0, next_v = 0.0;
    for (int t = T - 1; t >= 0; --t) {
        const size_t at = (size_t)t * N + n;
        const double v = (double)val[at];
        if (t == T - 1 || end[at] != 0.f) {   // the last step of a segment: bootstrap from the value after it, nothing carried
            next_v = (double)val_next[at] * (1.0 - (double)done[at]);
            gae = 0.0;
        }
        const double delta = (double)rew[at] + gamma * next_v - v;
        gae = delta + gamma * lambda * gae;
        ret[at] = (float)(gae + v), adv[at] = (float)gae;
        next_v = v;
    }
}

}  // namespace

extern "C" {

int gops_ppo_loss(const GopsPpoLoss* d, int32_t M, const float* head_new, const float* v_new, const float* act, const float* logp_old,
                  const float* adv, const float* ret, const float* val_old, const float* logits_old, const float* hyper, float* seed_head,
                  float* seed_v, float* stats, void* stream) {
    if (!d || M < 1 || d->act_dim < 1 || d->act_dim > GOPS_MAX_ACT) return GOPS_ERR_BAD_ARG;
    if (!head_new || !v_new || !act || !logp_old || !adv || !ret || !val_old || !logits_old || !hyper || !seed_head || !seed_v || !stats)
        return GOPS_ERR_BAD_ARG;
    if (d->loss_value_norm && M < 2) return GOPS_ERR_BAD_ARG;   // the unbiased std of one return does not exist
    if (!stats_aligned(stats)) return GOPS_ERR_BAD_ARG;         // (the norm behind the results is a double too)
    hipStream_t s = static_cast<hipStream_t>(stream);
    PpoParams p;
    p.M = M, p.A = d->act_dim, p.value_clip = d->loss_value_clip != 0, p.value_norm = d->loss_value_norm != 0;
    p.min_ls = d->min_log_std, p.max_ls = d->max_log_std;
    const dim3 one(1), many(PPO_BLOCKS), threads(256);
#define PPO_LAUNCH(grid, phases) \
    hipLaunchKernelGGL(ppo_loss_kernel, grid, threads, 0, s, p, phases, head_new, v_new, act, logp_old, adv, ret, val_old, logits_old, hyper, seed_head, seed_v, stats)
    if (!p.value_norm) {
        PPO_LAUNCH(M <= LOSS_ONE_BLOCK_MAX ? one : many, 2);
    } else if (M <= LOSS_ONE_BLOCK_MAX) {
        PPO_LAUNCH(one, 3);
    } else {
        PPO_LAUNCH(many, 1);
        PPO_LAUNCH(many, 2);
    }
#undef PPO_LAUNCH
    return (int)hipGetLastError();
}

int gops_adv_normalize(const float* adv, int32_t n, double eps, float* out, float* stats, void* stream) {
    if (!adv || !out || !stats || n < 2) return GOPS_ERR_BAD_ARG;
    if (!stats_aligned(stats)) return GOPS_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n <= LOSS_ONE_BLOCK_MAX) {
        hipLaunchKernelGGL(adv_normalize_kernel, dim3(1), dim3(256), 0, s, adv, n, eps, 3, out, stats);
    } else {
        hipLaunchKernelGGL(adv_normalize_kernel, dim3(PPO_BLOCKS), dim3(256), 0, s, adv, n, eps, 1, out, stats);
        hipLaunchKernelGGL(adv_normalize_kernel, dim3(PPO_BLOCKS), dim3(256), 0, s, adv, n, eps, 2, out, stats);
    }
    return (int)hipGetLastError();
}

int gops_gae(const float* rew, const float* val, const float* val_next, const float* done, const float* end, int32_t T, int32_t N,
             double gamma, double lambda, float* ret, float* adv, void* stream) {
    if (!rew || !val || !val_next || !done || !end || !ret || !adv || T < 1 || N < 1) return GOPS_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(gae_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, rew, val, val_next, done, end, T, N, gamma, lambda, ret, adv);
    return (int)hipGetLastError();
}

}  // extern "C"
