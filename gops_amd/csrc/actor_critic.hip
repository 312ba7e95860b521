// The no-grad half of a DDPG / TD3 / DSAC-T / SAC / DSAC update (gops/algorithm/ddpg.py:149-151, td3.py:166-183, dsact.py:237-313,
// sac.py:214-223, dsac.py:199-252).
//
// ac_backup_kernel: the Bellman backup in ONE launch, forward only, nothing stashed.  A workgroup of 256 threads owns a tile of R
// batch rows (R = 16, 32 or 64) and evaluates the target policy and the one or two target critics on it, one net after the other:
//   LDS:  in0 [R][O + A]   the tile's obs2 and, behind it, the smoothed target action (the critics' concatenated input lives here only);
//         xa, xb [R][ldx]  hidden activations, ping-pong;
//         wb               one chunk of a layer's weights, TRANSPOSED ([K][NC], so that the four features a thread owns are one
//                          16-byte read, the same address for all lanes of a row group: a broadcast), its biases behind it.
//   thread (r = tid % R, g = tid / R): row r, feature quads g, g + 256 / R, ..; every output is eight fp32 fmaf chains (input k
//   goes to chain k mod 8, k ascending) added pairwise, bias last - the same bits whatever R and the chunk size are.  (One
//   chain over 256 inputs measured 2.6x the rounding error of the MFMA path's blocked accumulation; eight independent chains
//   also hide the fmaf latency.)  The output layers (act_dim and one output), the squash, the noise clamps, the minimum and the
//   backup are the same chains in DOUBLE, rounded once where a value is stored.
//   Row strides of in0 / xa / xb are odd: the R rows a wave reads at one k sit in different banks.
// soft_backup_kernel: DSAC-T's distributional soft backup (dsact.py:237-313) on the same tile scheme - a tanh-Gaussian target policy
// (one thread per (row, action dimension) forms that dimension's mean and log std), two critics with (mean, softplus std) heads.
// soft_q_backup_kernel: SAC's and DSAC's soft Q backup on the same tile and policy head - one or two scalar critics with their minimum,
// or one critic with a (mean, softplus std) head and a clipped return sample.
// dqn_backup_kernel: DQN's max-Q backup on the same tile - one network on obs2 alone, its act_num head outputs in double, their maximum
// and arg-max per row; dqn_loss_kernel: the dense output-layer seed of the taken action's regression, with ac_critic_loss_kernel's sums.
// What the three kernels share is stated once and inlined into each: the tile prologue (ac_tile), the hidden layers and the head
// staging (ac_hidden, ac_stage_head; ac_tile.h: ac_head_dot, chain_sum8), and for the two soft kernels the policy head (soft_policy_head, its scalar
// arithmetic in soft_math.h), the distributional critic head (distri_head) and the row's entropy terms (soft_entropy_terms).  The
// host side likewise: one description of the nets (AcShape), one plan, one fill of AcParams' nets, one row-count dispatch.
// ac_tile.h holds what trpo.hip's fisher_seed_kernel takes from this scheme as well: the AC_* tile constants, ac_up4, the row-count
// ladder (ac_choose_rows), rows_dispatch, chain_sum8 and ac_head_dot.
// ac_critic_loss_kernel: gradient seeds, losses, mean(q) and |q - backup| of the critic regression in one launch; sums in double
// in the fixed order of block_reduce.h's grid_fold (gops_value_loss's scheme: one block up to 8192 rows, else 64 blocks' partials folded by the last one).
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "ac_tile.h"
#include "block_reduce.h"
#include "launchers.h"
#include "soft_math.h"

namespace {

constexpr int AC_MAX_WIDTH = 256;    // hidden width (multiples of 16)
constexpr int AC_MAX_HIDDEN = 3;     // hidden layers per net
constexpr int AC_MAX_IN = 64;        // obs_dim + act_dim
constexpr size_t AC_WORKSPACE = 256;

struct AcNet {
    int nl, act;
    int dims[GOPS_MAX_LAYERS + 1];
    int nc[GOPS_MAX_LAYERS];   // output features per staged chunk of layer j (hidden layers)
    const float* W[GOPS_MAX_LAYERS];
    const float* Bv[GOPS_MAX_LAYERS];
};

struct AcParams {
    AcNet net[3];   // 0: policy, 1 .. n_q: critics
    int n_q, smooth, B, O, A;
    int ld0, ldx, xa_off, xb_off, e_off, w_off;   // floats
    float sq_low[GOPS_MAX_ACT], sq_high[GOPS_MAX_ACT], act_low[GOPS_MAX_ACT], act_high[GOPS_MAX_ACT];
    double sigma, clip, rscale, gamma;
    const float *obs2, *rew, *done, *xi;
    float *backup, *a2, *q_targ;
};

}  // namespace

int ac_check_net(const GopsMlp& m, int in, int out) {   // (launchers.h: trpo.hip accepts the same nets)
    if (m.n_layers < 2 || m.n_layers > AC_MAX_HIDDEN + 1) return GOPS_ERR_UNSUPPORTED;   // (n_layers = 1: a POLY net)
    if (m.dtype != GOPS_DTYPE_F32 || m.variant_flags != 0) return GOPS_ERR_UNSUPPORTED;
    if (m.sizes[0] != in || m.sizes[m.n_layers] != out) return GOPS_ERR_BAD_ARG;
    for (int j = 1; j < m.n_layers; ++j)
        if (m.sizes[j] < 16 || (m.sizes[j] & 15) || m.sizes[j] > AC_MAX_WIDTH) return GOPS_ERR_UNSUPPORTED;
    if (m.hidden_act < GOPS_ACT_LINEAR || m.hidden_act > GOPS_ACT_TANH) return GOPS_ERR_BAD_ARG;
    for (int j = 0; j < m.n_layers; ++j)
        if (m.weight[j] == nullptr || m.bias[j] == nullptr) return GOPS_ERR_BAD_ARG;
    return GOPS_OK;
}

namespace {

int ac_check(const GopsAcBackup* d, int B) {
    if (!d || B < 1) return GOPS_ERR_BAD_ARG;
    if (d->n_q < 1 || d->n_q > 2) return GOPS_ERR_BAD_ARG;
    if (d->policy.n_layers < 1 || d->policy.n_layers > GOPS_MAX_LAYERS) return GOPS_ERR_BAD_ARG;
    const int O = d->policy.sizes[0], A = d->policy.sizes[d->policy.n_layers];
    if (O < 1 || A < 1 || A > GOPS_MAX_ACT) return GOPS_ERR_BAD_ARG;
    if (O + A > AC_MAX_IN) return GOPS_ERR_UNSUPPORTED;
    int rc = ac_check_net(d->policy, O, A);
    for (int i = 0; i < d->n_q && rc == GOPS_OK; ++i) rc = ac_check_net(d->q[i], O + A, 1);
    return rc;
}

// The stochastic-policy descriptions (gops_soft_backup, gops_soft_q_backup): a policy with 2 A outputs (means, then log stds) and
// n_q critics of `out` outputs on (obs, action).
int soft_check_nets(const GopsMlp& policy, const GopsMlp* q, int n_q, int out) {
    if (policy.n_layers < 1 || policy.n_layers > GOPS_MAX_LAYERS) return GOPS_ERR_BAD_ARG;
    const int O = policy.sizes[0], A2 = policy.sizes[policy.n_layers], A = A2 / 2;
    if (O < 1 || A < 1 || (A2 & 1) || A > GOPS_MAX_ACT) return GOPS_ERR_BAD_ARG;
    if (O + A > AC_MAX_IN) return GOPS_ERR_UNSUPPORTED;
    int rc = ac_check_net(policy, O, 2 * A);
    for (int i = 0; i < n_q && rc == GOPS_OK; ++i) rc = ac_check_net(q[i], O + A, out);
    return rc;
}

int soft_check(const GopsSoftBackup* d, int B) {
    if (!d || B < 1) return GOPS_ERR_BAD_ARG;
    return soft_check_nets(d->policy, d->q, 2, 2);
}

int soft_q_check(const GopsSoftQBackup* d, int B) {
    if (!d || B < 1) return GOPS_ERR_BAD_ARG;
    if (d->n_q < 1 || d->n_q > 2 || d->distri < 0 || d->distri > 1) return GOPS_ERR_BAD_ARG;
    if (d->distri && d->n_q == 2) return GOPS_ERR_UNSUPPORTED;   // gops_soft_backup's case
    return soft_check_nets(d->policy, d->q, d->n_q, d->distri ? 2 : 1);
}

int dqn_check(const GopsDqnBackup* d, int B) {
    if (!d || B < 1) return GOPS_ERR_BAD_ARG;
    if (d->q.n_layers < 1 || d->q.n_layers > GOPS_MAX_LAYERS || d->q.sizes[0] < 1 || d->act_num < 1) return GOPS_ERR_BAD_ARG;
    if (d->act_num < 2 || d->act_num > GOPS_DQN_MAX_ACTIONS || d->q.sizes[0] > AC_MAX_IN) return GOPS_ERR_UNSUPPORTED;
    return ac_check_net(d->q, d->q.sizes[0], d->act_num);
}

// What the LDS plan and the kernels' nets are made from - `nets`: the policy and the n_q critics; O / A: observation and action
// width; `extra`: floats per tile row kept between the networks besides in0, in front of the weight chunk.
struct AcShape {
    const GopsMlp* nets[3];
    int n_q, O, A, extra;
};
AcShape ac_shape(const GopsAcBackup& d) {
    return {{&d.policy, &d.q[0], &d.q[1]}, d.n_q, d.policy.sizes[0], d.policy.sizes[d.policy.n_layers], 0};
}
AcShape dqn_shape(const GopsDqnBackup& d) {   // one net, no action input; extra: the head's outputs, act_num doubles per row
    return {{&d.q, nullptr, nullptr}, 0, d.q.sizes[0], 0, 2 * d.act_num};
}
AcShape soft_shape(const GopsMlp& policy, const GopsMlp* q, int n_q) {
    const int A = policy.sizes[policy.n_layers] / 2;
    return {{&policy, &q[0], &q[1]}, n_q, policy.sizes[0], A, 2 * A};   // extra: the log-probability terms, A doubles per row
}

// LDS plan for tiles of R rows within `limit` bytes; every hidden layer must get chunks of at least `min_nc` features (or the
// whole layer).  Fills the offsets and the chunk sizes; returns the dynamic LDS bytes, 0 when it does not fit.
size_t ac_plan(const AcShape& sh, int R, size_t limit, int min_nc, AcParams& p) {
    int maxh = 0;
    for (int n = 0; n <= sh.n_q; ++n)
        for (int j = 1; j < sh.nets[n]->n_layers; ++j) maxh = std::max(maxh, (int)sh.nets[n]->sizes[j]);
    p.ld0 = (sh.O + sh.A) | 1;
    p.ldx = maxh | 1;
    p.xa_off = ac_up4(R * p.ld0);
    p.xb_off = p.xa_off + ac_up4(R * p.ldx);
    p.e_off = p.xb_off + ac_up4(R * p.ldx);
    p.w_off = p.e_off + ac_up4(R * sh.extra);   // 16-byte aligned: the weight quads are read as one f32x4
    const long long wfloats = (long long)(limit / sizeof(float)) - p.w_off;
    if (wfloats <= 0) return 0;
    long long used = 0;
    for (int n = 0; n <= sh.n_q; ++n) {
        const GopsMlp& m = *sh.nets[n];
        for (int j = 0; j < m.n_layers - 1; ++j) {
            const int K = m.sizes[j], N = m.sizes[j + 1];
            int nc = (int)std::min<long long>(N, (wfloats / (K + 1)) & ~15LL);
            if (nc < std::min(N, min_nc)) return 0;
            p.net[n].nc[j] = nc;
            used = std::max(used, (long long)(K + 1) * nc);
        }
        const long long head = (long long)(m.sizes[m.n_layers - 1] + 1) * m.sizes[m.n_layers];
        if (head > wfloats) return 0;
        used = std::max(used, head);
    }
    return ((size_t)p.w_off + (size_t)used) * sizeof(float);
}

// Tile rows and LDS bytes for a description (ac_tile.h: the row-count ladder).
size_t ac_choose(const AcShape& sh, int B, AcParams& p, int& R) {
    return ac_choose_rows(B, R, [&](int rows, size_t limit, int min_nc) { return ac_plan(sh, rows, limit, min_nc, p); });
}

// The workspace a checked description needs at batch B: 0 when no plan fits.
size_t ac_workspace_bytes(const AcShape& sh, int B) {
    AcParams p;
    int R;
    return ac_choose(sh, B, p, R) == 0 ? 0 : AC_WORKSPACE;
}

// The nets of a plan as the kernels read them, and what every description carries: batch, widths, action limits.
void ac_fill(const AcShape& sh, int B, const float* act_low, const float* act_high, AcParams& p) {
    for (int n = 0; n <= sh.n_q; ++n) {
        const GopsMlp& m = *sh.nets[n];
        AcNet& a = p.net[n];
        a.nl = m.n_layers, a.act = m.hidden_act;
        for (int j = 0; j <= a.nl; ++j) a.dims[j] = m.sizes[j];
        for (int j = 0; j < a.nl; ++j) { a.W[j] = m.weight[j]; a.Bv[j] = m.bias[j]; }
    }
    p.n_q = sh.n_q, p.B = B, p.O = sh.O, p.A = sh.A;
    for (int a = 0; a < p.A; ++a) p.act_low[a] = act_low[a], p.act_high[a] = act_high[a];
}

// The hidden layers of `net` on the tile's rows: input `in0` (row stride ld0), activations ping-pong between xa and xb (row stride
// ldx), one weight chunk at a time through wb.  Returns where the last hidden activations are (row stride ldx).  Begins with a
// barrier: what the caller wrote into in0 before the call is visible to every thread of the workgroup.
template <int R>
__device__ __forceinline__ const float* ac_hidden(const AcNet& net, const float* in0, int ld0, float* xa, float* xb, int ldx, float* wb) {
    constexpr int G = AC_THREADS / R;   // feature quads in flight per row
    const int tid = threadIdx.x, r = tid % R, g = tid / R;
    const float* cur = in0;
    int ldc = ld0;
    float* nxt = xa;
#pragma unroll 1
    for (int j = 0; j < net.nl - 1; ++j) {
        const int K = net.dims[j], N = net.dims[j + 1], NC = net.nc[j];
        const float* __restrict__ Wg = net.W[j];
#pragma unroll 1
        for (int n0 = 0; n0 < N; n0 += NC) {
            const int nc = min(NC, N - n0);
            __syncthreads();   // the previous readers of wb are done; what the previous layer (or the staging above) wrote is visible
            for (int idx = tid; idx < nc * K; idx += AC_THREADS) {
                const int k = idx / nc, nn = idx - k * nc;
                wb[k * NC + nn] = Wg[(size_t)(n0 + nn) * K + k];
            }
            for (int idx = tid; idx < nc; idx += AC_THREADS) wb[K * NC + idx] = net.Bv[j][n0 + idx];
            __syncthreads();
            const float* xr = cur + r * ldc;
            act_dispatch(net.act, [&]<int ACT>() {
                for (int fg = g; fg < (nc >> 2); fg += G) {
                    const float* wq = wb + 4 * fg;
                    f32x4 c[AC_CHAINS];
#pragma unroll
                    for (int i = 0; i < AC_CHAINS; ++i) c[i] = f32x4{0.f, 0.f, 0.f, 0.f};
                    const int K8 = K & ~(AC_CHAINS - 1);
                    for (int k = 0; k < K8; k += AC_CHAINS) {
#pragma unroll
                        for (int i = 0; i < AC_CHAINS; ++i) {
                            const float x = xr[k + i];
                            const f32x4 w = *reinterpret_cast<const f32x4*>(wq + (k + i) * NC);
#pragma unroll
                            for (int e = 0; e < 4; ++e) c[i][e] = fmaf(x, w[e], c[i][e]);
                        }
                    }
#pragma unroll
                    for (int i = 0; i < AC_CHAINS - 1; ++i) {
                        if (K8 + i < K) {
                            const float x = xr[K8 + i];
                            const f32x4 w = *reinterpret_cast<const f32x4*>(wq + (K8 + i) * NC);
#pragma unroll
                            for (int e = 0; e < 4; ++e) c[i][e] = fmaf(x, w[e], c[i][e]);
                        }
                    }
                    const float* bq = wb + K * NC + 4 * fg;
                    float* yr = nxt + r * ldx + n0 + 4 * fg;
                    const f32x4 sum = chain_sum8(c);
#pragma unroll
                    for (int e = 0; e < 4; ++e) yr[e] = act_fwd_t<ACT>(sum[e] + bq[e]);
                }
            });
        }
        cur = nxt;
        ldc = ldx;
        nxt = nxt == xa ? xb : xa;
    }
    return cur;
}

// The output layer's weights, row-major [N][K], and its biases behind them into wb (barriers on both sides).
__device__ __forceinline__ void ac_stage_head(const AcNet& net, float* wb) {
    const int K = net.dims[net.nl - 1], N = net.dims[net.nl];
    __syncthreads();
    for (int idx = threadIdx.x; idx < N * K; idx += AC_THREADS) wb[idx] = net.W[net.nl - 1][idx];
    for (int idx = threadIdx.x; idx < N; idx += AC_THREADS) wb[N * K + idx] = net.Bv[net.nl - 1][idx];
    __syncthreads();
}

// A workgroup's tile: the first batch row and how many of the R rows are inside the batch, the widths and row strides, the
// sections of the LDS plan.
struct AcTile {
    int b0, nvalid, O, A, ld0, ldx;
    float *in0, *xa, *xb, *extra, *wb;
};

// The tile prologue of every kernel here: carves the plan's sections out of `lds` and stages the tile's obs2 into in0.
template <int R>
__device__ __forceinline__ AcTile ac_tile(const AcParams& p, float* lds) {
    AcTile t;
    t.b0 = blockIdx.x * R;
    t.nvalid = min(R, p.B - t.b0);
    t.O = p.O, t.A = p.A, t.ld0 = p.ld0, t.ldx = p.ldx;
    t.in0 = lds, t.xa = lds + p.xa_off, t.xb = lds + p.xb_off, t.extra = lds + p.e_off, t.wb = lds + p.w_off;
    for (int idx = threadIdx.x; idx < R * t.O; idx += AC_THREADS) {   // rows beyond the batch: zeros (evaluated, never stored)
        const int m = idx / t.O, k = idx - m * t.O;
        t.in0[m * t.ld0 + k] = m < t.nvalid ? p.obs2[(size_t)(t.b0 + m) * t.O + k] : 0.f;
    }
    return t;
}

template <int R>
__global__ __launch_bounds__(AC_THREADS) void ac_backup_kernel(const AcParams p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, r = tid % R, g = tid / R;
    const AcTile t = ac_tile<R>(p, lds);
    const int b0 = t.b0, nvalid = t.nvalid, O = t.O, A = t.A, ld0 = t.ld0, ldx = t.ldx;
    float *in0 = t.in0, *xa = t.xa, *xb = t.xb, *wb = t.wb;

    double q_min = 0.0;   // of row r, in the threads with g == 0
#pragma unroll 1
    for (int n = 0; n <= p.n_q; ++n) {
        const AcNet& net = p.net[n];
        const float* cur = ac_hidden<R>(net, in0, ld0, xa, xb, ldx, wb);
        // ---- output layer: row-major [N][K] in wb, one thread per (row, output) ----
        const int K = net.dims[net.nl - 1], N = net.dims[net.nl];
        ac_stage_head(net, wb);
        if (g < N) {
            // The output layer, the squash and the backup are formed in double and rounded once where they are stored: one thread
            // per (row, output), K <= 256 products - a negligible share of the work, and what is left of the kernel's error is the
            // fp32 rounding of the hidden layers alone.
            const double y = ac_head_dot(cur + r * ldx, wb + g * K, K) + (double)wb[N * K + g];
            if (n == 0) {   // the policy's own squash, then TD3's smoothing (td3.py:168-177)
                const double lo_s = g == 0 ? p.sq_low[0] : g == 1 ? p.sq_low[1] : g == 2 ? p.sq_low[2] : p.sq_low[3];
                const double hi_s = g == 0 ? p.sq_high[0] : g == 1 ? p.sq_high[1] : g == 2 ? p.sq_high[2] : p.sq_high[3];
                double a = (hi_s - lo_s) / 2 * tanh(y) + (hi_s + lo_s) / 2;
                if (p.smooth) {
                    const double lo = g == 0 ? p.act_low[0] : g == 1 ? p.act_low[1] : g == 2 ? p.act_low[2] : p.act_low[3];
                    const double hi = g == 0 ? p.act_high[0] : g == 1 ? p.act_high[1] : g == 2 ? p.act_high[2] : p.act_high[3];
                    const double xi = r < nvalid ? (double)p.xi[(size_t)(b0 + r) * A + g] : 0.0;
                    const double eps = fmin(fmax(xi * p.sigma, -p.clip), p.clip);
                    a = fmin(fmax(a + eps, lo), hi);
                }
                const float af = (float)a;
                in0[r * ld0 + O + g] = af;   // (published by the barrier at the top of the critic's first chunk)
                if (p.a2 != nullptr && r < nvalid) p.a2[(size_t)(b0 + r) * A + g] = af;
            } else {        // g == 0
                if (p.q_targ != nullptr && r < nvalid) p.q_targ[(size_t)(n - 1) * p.B + b0 + r] = (float)y;
                q_min = n == 1 ? y : fmin(q_min, y);
            }
        }
    }
    if (g == 0 && r < nvalid)   // backup = r * reward_scale + gamma * (1 - d) * q   (ddpg.py:151, td3.py:183)
        p.backup[b0 + r] = (float)((double)p.rew[b0 + r] * p.rscale + p.gamma * (1.0 - (double)p.done[b0 + r]) * q_min);
}

// ---- DSAC-T: the distributional soft backup (gops/algorithm/dsact.py:237-313, the no-grad part) -----------------------------------
// Same tile, staging and chains as ac_backup_kernel.  The policy head has 2 A outputs (means, then log stds) but a 64-row tile has only
// four feature groups per row: thread (r, g < A) forms BOTH outputs of action dimension g, samples, squashes, and leaves that
// dimension's log-probability term in LDS (lp [A][R], doubles, in the plan's extra section); thread (r, 0) forms both outputs of each
// critic and, at the end, the row's two targets.
struct SoftParams {
    AcParams ac;   // net, B, O, A, the LDS plan, act_low / act_high, gamma, obs2 / rew / done, a2, q_targ ([2, B, 2] here)
    double min_ls, max_ls, alpha;
    const float *log_alpha, *eps, *z;
    float *tq, *tqs, *logp;
};

// The tanh-Gaussian policy at the tile's obs2, of both soft kernels: u = mean + std * eps, a2 = half * tanh(u) + mid into in0 behind
// obs2 (and into p.a2), the dimension's share of log pi(a2 | obs2) into lp[g * R + r] (soft_math.h: tanh_gauss_dim).  Both are
// published by the barrier at the top of the first critic's first chunk.
template <int R>
__device__ __forceinline__ void soft_policy_head(const SoftParams& sp, const AcTile& t, double* lp) {
    const AcParams& p = sp.ac;
    const int tid = threadIdx.x, r = tid % R, g = tid / R;
    const int O = t.O, A = t.A, ld0 = t.ld0, ldx = t.ldx;
    const AcNet& net = p.net[0];
    const float* cur = ac_hidden<R>(net, t.in0, ld0, t.xa, t.xb, ldx, t.wb);
    const int K = net.dims[net.nl - 1];
    const float* wb = t.wb;
    ac_stage_head(net, t.wb);
    if (g < A) {
        const float* xr = cur + r * ldx;
        const double mean = ac_head_dot(xr, wb + g * K, K) + (double)wb[2 * A * K + g];
        const double ls = ac_head_dot(xr, wb + (A + g) * K, K) + (double)wb[2 * A * K + A + g];
        const double e = r < t.nvalid ? (double)sp.eps[(size_t)(t.b0 + r) * A + g] : 0.0;
        const double lo = g == 0 ? p.act_low[0] : g == 1 ? p.act_low[1] : g == 2 ? p.act_low[2] : p.act_low[3];
        const double hi = g == 0 ? p.act_high[0] : g == 1 ? p.act_high[1] : g == 2 ? p.act_high[2] : p.act_high[3];
        const TanhGaussDim d = tanh_gauss_dim(mean, ls, e, lo, hi, sp.min_ls, sp.max_ls);
        const float af = (float)d.act;
        t.in0[r * ld0 + O + g] = af;
        if (p.a2 != nullptr && r < t.nvalid) p.a2[(size_t)(t.b0 + r) * A + g] = af;
        lp[g * R + r] = d.logp;
    }
}

// (m, softplus s) of a distributional critic's row from its staged head (row-major [2][K], the two biases behind), stored to qt
// unless that is null.
__device__ __forceinline__ void distri_head(const float* xr, const float* wb, int K, float* qt, double& m, double& sd) {
    m = ac_head_dot(xr, wb, K) + (double)wb[2 * K];
    sd = softplus_d(ac_head_dot(xr, wb + K, K) + (double)wb[2 * K + 1]);
    if (qt != nullptr) qt[0] = (float)m, qt[1] = (float)sd;
}

// log pi(a2 | obs2) of row r - its dimensions' terms in ascending order - and the temperature.
template <int R>
__device__ __forceinline__ void soft_entropy_terms(const SoftParams& sp, const double* lp, int A, int r, double& logp, double& alpha) {
    logp = 0.0;
    for (int a = 0; a < A; ++a) logp += lp[a * R + r];
    alpha = sp.log_alpha != nullptr ? exp((double)*sp.log_alpha) : sp.alpha;
}

template <int R>
__global__ __launch_bounds__(AC_THREADS) void soft_backup_kernel(const SoftParams sp) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const AcParams& p = sp.ac;
    const int tid = threadIdx.x, r = tid % R, g = tid / R;
    const AcTile t = ac_tile<R>(p, lds);
    const int b0 = t.b0, nvalid = t.nvalid;
    double* lp = reinterpret_cast<double*>(t.extra);
    soft_policy_head<R>(sp, t, lp);   // the target policy
    double m1 = 0.0, s1 = 0.0, m2 = 0.0, s2 = 0.0;   // of row r, in the threads with g == 0
#pragma unroll 1
    for (int n = 1; n <= 2; ++n) {
        const AcNet& net = p.net[n];
        const float* cur = ac_hidden<R>(net, t.in0, t.ld0, t.xa, t.xb, t.ldx, t.wb);
        const int K = net.dims[net.nl - 1];
        ac_stage_head(net, t.wb);
        if (g == 0) {
            float* qt = p.q_targ != nullptr && r < nvalid ? p.q_targ + ((size_t)(n - 1) * p.B + b0 + r) * 2 : nullptr;
            double m, sd;
            distri_head(cur + r * t.ldx, t.wb, K, qt, m, sd);
            if (n == 1) m1 = m, s1 = sd;
            else m2 = m, s2 = sd;
        }
    }
    if (g == 0 && r < nvalid) {
        const int b = b0 + r;
        double logp, alpha;
        soft_entropy_terms<R>(sp, lp, t.A, r, logp, alpha);
        const double z1 = fmin(fmax((double)sp.z[b], -3.0), 3.0), z2 = fmin(fmax((double)sp.z[(size_t)p.B + b], -3.0), 3.0);
        const double q_next = fmin(m1, m2), q_sample = m1 < m2 ? m1 + z1 * s1 : m2 + z2 * s2;
        const double rew = (double)p.rew[b], live = (1.0 - (double)p.done[b]) * p.gamma;
        sp.tq[b] = (float)(rew + live * (q_next - alpha * logp));    // dsact.py:304-309
        sp.tqs[b] = (float)(rew + live * (q_sample - alpha * logp));
        if (sp.logp != nullptr) sp.logp[b] = (float)logp;
    }
}

// ---- SAC / DSAC: the soft Q backup (gops/algorithm/sac.py:214-223, dsac.py:199-252, the no-grad part) ------------------------------
// soft_backup_kernel's tile, policy head and log-probability (the same helpers), then one or two scalar critics with their minimum
// (distri = 0), or one critic with a (mean, softplus std) head and a clipped return sample (distri = 1).
struct SoftQParams {
    SoftParams s;   // ac.n_q: the critics; tq: the backup; z: [B] (distri); ac.q_targ: [n_q, B], or [B, 2] = (m, s) with distri
    int distri;
};

template <int R>
__global__ __launch_bounds__(AC_THREADS) void soft_q_backup_kernel(const SoftQParams qp) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const SoftParams& sp = qp.s;
    const AcParams& p = sp.ac;
    const int tid = threadIdx.x, r = tid % R, g = tid / R;
    const AcTile t = ac_tile<R>(p, lds);
    const int b0 = t.b0, nvalid = t.nvalid;
    double* lp = reinterpret_cast<double*>(t.extra);
    soft_policy_head<R>(sp, t, lp);   // the policy at obs2
    double q_next = 0.0, s_next = 0.0;   // of row r, in the threads with g == 0: min_i q_i, or (m, s) of the one distributional critic
#pragma unroll 1
    for (int n = 1; n <= p.n_q; ++n) {
        const AcNet& net = p.net[n];
        const float* cur = ac_hidden<R>(net, t.in0, t.ld0, t.xa, t.xb, t.ldx, t.wb);
        const int K = net.dims[net.nl - 1];
        ac_stage_head(net, t.wb);
        if (g == 0) {
            const float* xr = cur + r * t.ldx;
            if (qp.distri) {
                distri_head(xr, t.wb, K, p.q_targ != nullptr && r < nvalid ? p.q_targ + (size_t)(b0 + r) * 2 : nullptr, q_next, s_next);
            } else {
                const double y = ac_head_dot(xr, t.wb, K) + (double)t.wb[K];
                if (p.q_targ != nullptr && r < nvalid) p.q_targ[(size_t)(n - 1) * p.B + b0 + r] = (float)y;
                q_next = n == 1 ? y : fmin(q_next, y);
            }
        }
    }
    if (g == 0 && r < nvalid) {
        const int b = b0 + r;
        double logp, alpha;
        soft_entropy_terms<R>(sp, lp, t.A, r, logp, alpha);
        if (qp.distri) q_next += fmin(fmax((double)sp.z[b], -3.0), 3.0) * s_next;   // dsac.py:206-208
        sp.tq[b] = (float)((double)p.rew[b] + (1.0 - (double)p.done[b]) * p.gamma * (q_next - alpha * logp));   // sac.py:221, dsac.py:246
        if (sp.logp != nullptr) sp.logp[b] = (float)logp;
    }
}

// ---- DQN: the max-Q backup (gops/algorithm/dqn.py:138-140) -------------------------------------------------------------------------
// Same tile, staging and chains as ac_backup_kernel, one network (obs2 alone is its input).  The head has act_num <= 16 outputs but a
// 64-row tile has only four feature groups per row: thread (r, g) forms outputs g, g + 256 / R, .. in double and parks them in LDS
// (qv [act_num][R], doubles, in the plan's extra section); thread (r, 0) then takes the row's maximum over the doubles in index
// order - the lowest index among bit-equal maxima - and forms the backup.
struct DqnParams {
    AcParams ac;   // net[0], B, O (A = 0), the LDS plan, rscale, gamma, obs2 / rew / done, backup, q_targ ([B, act_num] here)
    int* a_star;
};

template <int R>
__global__ __launch_bounds__(AC_THREADS) void dqn_backup_kernel(const DqnParams dp) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int G = AC_THREADS / R;
    const AcParams& p = dp.ac;
    const int tid = threadIdx.x, r = tid % R, g = tid / R;
    const AcTile t = ac_tile<R>(p, lds);
    const int b0 = t.b0, nvalid = t.nvalid;
    const AcNet& net = p.net[0];
    const float* cur = ac_hidden<R>(net, t.in0, t.ld0, t.xa, t.xb, t.ldx, t.wb);
    const int K = net.dims[net.nl - 1], N = net.dims[net.nl];
    ac_stage_head(net, t.wb);
    double* qv = reinterpret_cast<double*>(t.extra);
    for (int a = g; a < N; a += G) {
        const double y = ac_head_dot(cur + r * t.ldx, t.wb + a * K, K) + (double)t.wb[N * K + a];
        qv[a * R + r] = y;
        if (p.q_targ != nullptr && r < nvalid) p.q_targ[(size_t)(b0 + r) * N + a] = (float)y;
    }
    __syncthreads();
    if (g == 0 && r < nvalid) {
        double q_max = qv[r];
        int best = 0;
        for (int a = 1; a < N; ++a) {
            const double v = qv[a * R + r];
            if (v > q_max || (v != v && q_max == q_max)) q_max = v, best = a;   // (a NaN is the maximum, as for torch.max)
        }
        const int b = b0 + r;   // backup = r * reward_scale + gamma * (1 - d) * max_a q_target(o2)[a]   (dqn.py:104,140)
        p.backup[b] = (float)((double)p.rew[b] * p.rscale + p.gamma * (1.0 - (double)p.done[b]) * q_max);
        if (dp.a_star != nullptr) dp.a_star[b] = best;
    }
}

// ---- critic regression: seeds, losses, mean(q), |q - backup| -------------------------------------------------------------------
constexpr int ACL_BLOCKS = 64;
constexpr int ACL_ONE_BLOCK_MAX = 8192;

__global__ __launch_bounds__(256) void ac_critic_loss_kernel(const float* __restrict__ q, const float* __restrict__ backup,
                                                             const float* __restrict__ weight, int nq, int B, float gsc,
                                                             float* __restrict__ seed, float* __restrict__ abs_err,
                                                             float* __restrict__ stats) {
    __shared__ double red[3][4];
    __shared__ bool last;
    double s[3] = {0.0, 0.0, 0.0};   // sum w d0^2, sum w d1^2, sum q0
    for (int i = blockIdx.x * 256 + threadIdx.x; i < B; i += gridDim.x * 256) {
        const float bk = backup[i], q0 = q[i];
        const float d0 = q0 - bk;
        const float w = weight != nullptr ? weight[i] : 1.f;
        seed[i] = weight != nullptr ? gsc * (w * d0) : gsc * d0;
        s[0] += (double)(weight != nullptr ? w * (d0 * d0) : d0 * d0);
        s[2] += (double)q0;
        if (abs_err != nullptr) abs_err[i] = fabsf(d0);
        if (nq == 2) {
            const float d1 = q[(size_t)B + i] - bk;
            seed[(size_t)B + i] = weight != nullptr ? gsc * (w * d1) : gsc * d1;
            s[1] += (double)(weight != nullptr ? w * (d1 * d1) : d1 * d1);
        }
    }
    // the blocks' partial sums [ACL_BLOCKS][3] behind the four results, then the ticket
    if (grid_fold<3>(s, red, reinterpret_cast<double*>(stats + 4), 3, reinterpret_cast<unsigned*>(stats + 4 + 6 * ACL_BLOCKS), &last) &&
        threadIdx.x == 0) {
        const float l0 = (float)(s[0] / (double)B), l1 = (float)(s[1] / (double)B);
        stats[0] = l0;
        stats[1] = l1;
        stats[2] = (float)(s[2] / (double)B);
        stats[3] = l0 + l1;
    }
}
static_assert(4 + 6 * ACL_BLOCKS + 1 <= GOPS_AC_LOSS_STATS_FLOATS, "stats: four results, the blocks' partial sums, the ticket");

// DQN's regression on the taken action's value (dqn.py:136-141, 146-153): the dense output-layer seed [B, N], |q_sel - backup|, the
// loss, mean(q_sel) and the count of rows whose index is outside [0, N).  One thread per row; the same fold and `stats` layout as
// ac_critic_loss_kernel.
__global__ __launch_bounds__(256) void dqn_loss_kernel(const float* __restrict__ q_all, const float* __restrict__ act,
                                                       const float* __restrict__ backup, const float* __restrict__ weight, int N, int B,
                                                       float gsc, float* __restrict__ seed, float* __restrict__ abs_err,
                                                       float* __restrict__ stats) {
    __shared__ double red[3][4];
    __shared__ bool last;
    double s[3] = {0.0, 0.0, 0.0};   // sum w d^2, sum q_sel, rows with an index outside [0, N)
    for (int i = blockIdx.x * 256 + threadIdx.x; i < B; i += gridDim.x * 256) {
        const float af = act[i];
        const bool ok = af > -1.f && af < (float)N;   // truncation towards zero lands in [0, N); false for a NaN
        const int a = ok ? (int)af : -1;
        float g = 0.f, e = 0.f;
        if (ok) {
            const float q = q_all[(size_t)i * N + a];
            const float d = q - backup[i];
            const float w = weight != nullptr ? weight[i] : 1.f;
            g = weight != nullptr ? gsc * (w * d) : gsc * d;
            e = fabsf(d);
            s[0] += (double)(weight != nullptr ? w * (d * d) : d * d);
            s[1] += (double)q;
        } else {
            s[2] += 1.0;
        }
        float* srow = seed + (size_t)i * N;
        for (int c = 0; c < N; ++c) srow[c] = c == a ? g : 0.f;
        if (abs_err != nullptr) abs_err[i] = e;
    }
    if (grid_fold<3>(s, red, reinterpret_cast<double*>(stats + 4), 3, reinterpret_cast<unsigned*>(stats + 4 + 6 * ACL_BLOCKS), &last) &&
        threadIdx.x == 0) {
        stats[0] = (float)(s[0] / (double)B);
        stats[1] = (float)(s[1] / (double)B);
        stats[2] = (float)s[2];
        stats[3] = 0.f;
    }
}
static_assert(4 + 6 * ACL_BLOCKS + 1 <= GOPS_DQN_LOSS_STATS_FLOATS, "stats: the results, the blocks' partial sums, the ticket");

}  // namespace

namespace {

// What every backup entry point does between its argument checks and its launch: the plan (GOPS_ERR_UNSUPPORTED when none fits),
// the workspace check, the fill of the plan's nets and widths.
int ac_prepare(const AcShape& sh, int B, const float* act_low, const float* act_high, const void* ws, size_t ws_bytes, AcParams& p,
               int& R, size_t& lds) {
    lds = ac_choose(sh, B, p, R);
    if (lds == 0) return GOPS_ERR_UNSUPPORTED;
    if (!ws || ws_bytes < AC_WORKSPACE) return GOPS_ERR_WORKSPACE;
    ac_fill(sh, B, act_low, act_high, p);
    return GOPS_OK;
}

// The fields GopsSoftBackup and GopsSoftQBackup share, and the tensors both kernels take.
template <typename Desc>
void soft_fill(const Desc& d, const float* obs2, const float* rew, const float* done, const float* eps, const float* z, float* a2,
               float* logp, float* q_targ, SoftParams& sp) {
    AcParams& p = sp.ac;
    p.gamma = d.gamma;
    p.obs2 = obs2, p.rew = rew, p.done = done, p.a2 = a2, p.q_targ = q_targ;
    sp.min_ls = d.min_log_std, sp.max_ls = d.max_log_std, sp.alpha = d.alpha, sp.log_alpha = d.log_alpha;
    sp.eps = eps, sp.z = z, sp.logp = logp;
}

inline dim3 ac_grid(int B, int R) { return dim3((unsigned)((B + R - 1) / R)); }

}  // namespace

extern "C" {

size_t gops_ac_backup_workspace_bytes(const GopsAcBackup* d, int32_t B) {
    return ac_check(d, B) != GOPS_OK ? 0 : ac_workspace_bytes(ac_shape(*d), B);
}

int gops_ac_backup(const GopsAcBackup* d, int32_t B, const float* obs2, const float* rew, const float* done, const float* xi, float* backup,
                   float* a2, float* q_targ, void* ws, size_t ws_bytes, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = ac_check(d, B);
    if (rc != GOPS_OK) return rc;
    if (!obs2 || !rew || !done || !backup || (d->smooth && !xi)) return GOPS_ERR_BAD_ARG;
    AcParams p;
    memset(&p, 0, sizeof(p));
    int R;
    size_t lds;
    rc = ac_prepare(ac_shape(*d), B, d->act_low, d->act_high, ws, ws_bytes, p, R, lds);
    if (rc != GOPS_OK) return rc;
    p.smooth = d->smooth != 0;
    for (int a = 0; a < p.A; ++a) p.sq_low[a] = d->squash_low[a], p.sq_high[a] = d->squash_high[a];
    p.sigma = d->target_noise, p.clip = d->noise_clip, p.rscale = d->reward_scale, p.gamma = d->gamma;
    p.obs2 = obs2, p.rew = rew, p.done = done, p.xi = xi;
    p.backup = backup, p.a2 = a2, p.q_targ = q_targ;
    rows_dispatch(R, [&]<int RR>() { launch_with_lds(ac_backup_kernel<RR>, ac_grid(B, RR), dim3(AC_THREADS), lds, s, p); });
    return (int)hipGetLastError();
}

int gops_ac_critic_loss(const float* q, const float* backup, const float* weight, int32_t nq, int32_t B, float* seed, float* abs_err,
                        float* stats, void* stream) {
    if (!q || !backup || !seed || !stats || B < 1 || nq < 1 || nq > 2) return GOPS_ERR_BAD_ARG;
    if (!stats_aligned(stats)) return GOPS_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(ac_critic_loss_kernel, dim3(B <= ACL_ONE_BLOCK_MAX ? 1 : ACL_BLOCKS), dim3(256), 0, s, q, backup, weight, nq, B,
                       (float)(2.0 / B), seed, abs_err, stats);
    return (int)hipGetLastError();
}

size_t gops_dqn_backup_workspace_bytes(const GopsDqnBackup* d, int32_t B) {
    return dqn_check(d, B) != GOPS_OK ? 0 : ac_workspace_bytes(dqn_shape(*d), B);
}

int gops_dqn_backup(const GopsDqnBackup* d, int32_t B, const float* obs2, const float* rew, const float* done, float* backup,
                    float* q_targ, int32_t* a_star, void* ws, size_t ws_bytes, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = dqn_check(d, B);
    if (rc != GOPS_OK) return rc;
    if (!obs2 || !rew || !done || !backup) return GOPS_ERR_BAD_ARG;
    DqnParams dp;
    memset(&dp, 0, sizeof(dp));
    AcParams& p = dp.ac;
    int R;
    size_t lds;
    rc = ac_prepare(dqn_shape(*d), B, nullptr, nullptr, ws, ws_bytes, p, R, lds);
    if (rc != GOPS_OK) return rc;
    p.rscale = d->reward_scale, p.gamma = d->gamma;
    p.obs2 = obs2, p.rew = rew, p.done = done;
    p.backup = backup, p.q_targ = q_targ;
    dp.a_star = a_star;
    rows_dispatch(R, [&]<int RR>() { launch_with_lds(dqn_backup_kernel<RR>, ac_grid(B, RR), dim3(AC_THREADS), lds, s, dp); });
    return (int)hipGetLastError();
}

int gops_dqn_loss(const float* q_all, const float* act, const float* backup, const float* weight, int32_t N, int32_t B, float* seed,
                  float* abs_err, float* stats, void* stream) {
    if (!q_all || !act || !backup || !seed || !stats || B < 1 || N < 1) return GOPS_ERR_BAD_ARG;
    if (!stats_aligned(stats)) return GOPS_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(dqn_loss_kernel, dim3(B <= ACL_ONE_BLOCK_MAX ? 1 : ACL_BLOCKS), dim3(256), 0, s, q_all, act, backup, weight, N, B,
                       (float)(2.0 / B), seed, abs_err, stats);
    return (int)hipGetLastError();
}

size_t gops_soft_backup_workspace_bytes(const GopsSoftBackup* d, int32_t B) {
    return soft_check(d, B) != GOPS_OK ? 0 : ac_workspace_bytes(soft_shape(d->policy, d->q, 2), B);
}

int gops_soft_backup(const GopsSoftBackup* d, int32_t B, const float* obs2, const float* rew, const float* done, const float* eps,
                     const float* z, float* tq, float* tqs, float* a2, float* logp, float* q_targ, void* ws, size_t ws_bytes, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = soft_check(d, B);
    if (rc != GOPS_OK) return rc;
    if (!obs2 || !rew || !done || !eps || !z || !tq || !tqs) return GOPS_ERR_BAD_ARG;
    SoftParams sp;
    memset(&sp, 0, sizeof(sp));
    int R;
    size_t lds;
    rc = ac_prepare(soft_shape(d->policy, d->q, 2), B, d->act_low, d->act_high, ws, ws_bytes, sp.ac, R, lds);
    if (rc != GOPS_OK) return rc;
    soft_fill(*d, obs2, rew, done, eps, z, a2, logp, q_targ, sp);
    sp.tq = tq, sp.tqs = tqs;
    rows_dispatch(R, [&]<int RR>() { launch_with_lds(soft_backup_kernel<RR>, ac_grid(B, RR), dim3(AC_THREADS), lds, s, sp); });
    return (int)hipGetLastError();
}

size_t gops_soft_q_backup_workspace_bytes(const GopsSoftQBackup* d, int32_t B) {
    return soft_q_check(d, B) != GOPS_OK ? 0 : ac_workspace_bytes(soft_shape(d->policy, d->q, d->n_q), B);
}

int gops_soft_q_backup(const GopsSoftQBackup* d, int32_t B, const float* obs2, const float* rew, const float* done, const float* eps,
                       const float* z, float* backup, float* a2, float* logp, float* q_targ, void* ws, size_t ws_bytes, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = soft_q_check(d, B);
    if (rc != GOPS_OK) return rc;
    if (!obs2 || !rew || !done || !eps || (d->distri && !z) || !backup) return GOPS_ERR_BAD_ARG;
    SoftQParams qp;
    memset(&qp, 0, sizeof(qp));
    int R;
    size_t lds;
    rc = ac_prepare(soft_shape(d->policy, d->q, d->n_q), B, d->act_low, d->act_high, ws, ws_bytes, qp.s.ac, R, lds);
    if (rc != GOPS_OK) return rc;
    soft_fill(*d, obs2, rew, done, eps, z, a2, logp, q_targ, qp.s);
    qp.s.tq = backup;
    qp.distri = d->distri;
    rows_dispatch(R, [&]<int RR>() { launch_with_lds(soft_q_backup_kernel<RR>, ac_grid(B, RR), dim3(AC_THREADS), lds, s, qp); });
    return (int)hipGetLastError();
}

}  // extern "C"
