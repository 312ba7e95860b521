// The stages of a TRPO update (gops/algorithm/trpo.py) that the MLP launches do not cover.
//
// What this file shares with others is stated there: the Gaussian head's double arithmetic in gauss_math.h (with ppo.hip), the tile
// constants, row-count ladder, rows_dispatch, chain_sum8 and ac_head_dot in ac_tile.h (with actor_critic.hip), the sums in
// block_reduce.h's grid_fold.
// fisher_seed_kernel: the Gauss-Newton form of the KL Hessian-vector product needs J v, the directional derivative of the policy's
//   RAW head (mean, raw log std) along a parameter tangent v = (V_j, c_j).  A workgroup of 256 threads owns a tile of R batch rows
//   (actor_critic.hip's scheme) and carries, per layer, the primal row h and ONE tangent row t:
//       z = W h + b,   u = W t + V h + c,   h' = act(z),   t' = act'(z) u,      t_0 = 0
//   LDS:  in0 [R][O]; xa, xb [R][ldx] primal activations, ping-pong; ta, tb [R][ldx] tangents, ping-pong; wb: one chunk of W,
//         TRANSPOSED ([K][NC]) with its biases behind it, and the same chunk of V with c behind that.
//   thread (r = tid % R, g = tid / R): row r, feature quads g, g + 256 / R, ..; z is eight fp32 fmaf chains (input k in chain k mod 8,
//   k ascending) added pairwise, bias last; u is two such sets of chains, one for W t and one for V h, added, then c -
//   the same bits whatever R and the chunk size are.  The head (its outputs and their tangents) is the same chains in DOUBLE; the
//   kernel takes it as a template parameter: GaussHead (2A outputs, one thread per (row, action dimension), the metric of the
//   Gaussian's KL) or CatHead (N logits, the softmax Fisher metric diag(p) - p p^T) - each scales by 1 / B as well.  No atomics, no
//   workgroup waits.
// trpo_surrogate_kernel: mean(exp(logp_new - logp_old) adv), mean KL(new || old), the seed d surrogate / d head_new and the line
//   search's verdict, ppo_loss_kernel's style: values in double, rounded once where stored, sums in the fixed order of block_reduce.h.
// cat_surrogate_kernel: the same for a categorical policy over N <= 16 action indices, from the logits; rows whose index is outside
//   [0, N) are counted and left out, as in actor_critic.hip's dqn_loss_kernel.
// cg_*_kernel: trpo.py:226-267 on flat fp32 vectors with every scalar in a device state block (GopsCgState of gops_hip.h).
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "ac_tile.h"
#include "block_reduce.h"
#include "gauss_math.h"
#include "launchers.h"

namespace {

struct FsParams {
    int nl, act, B, O, A;
    int dims[GOPS_MAX_LAYERS + 1];
    int nc[GOPS_MAX_LAYERS];   // output features per staged chunk of hidden layer j
    const float* W[GOPS_MAX_LAYERS];
    const float* Bv[GOPS_MAX_LAYERS];
    const float* V[GOPS_MAX_LAYERS];    // the tangent's weight slices
    const float* Cv[GOPS_MAX_LAYERS];   // and its bias slices
    int ld0, ldx, xa_off, xb_off, ta_off, tb_off, w_off;   // floats
    int park_off;              // floats: the head's parked doubles, behind the staged output layer (CatHead)
    double min_ls, max_ls;     // (GaussHead)
    const float* x;
    float* seed;
};

// LDS plan for tiles of R rows within `limit` bytes (actor_critic.hip's ac_plan with four activation planes and two weight chunks).
// `park`: doubles per tile row the head parks behind the staged output layer (0: the Gaussian head parks none).
size_t fs_plan(const GopsMlp& m, int R, size_t limit, int min_nc, int park, FsParams& p) {
    int maxh = 0;
    for (int j = 1; j < m.n_layers; ++j) maxh = std::max(maxh, (int)m.sizes[j]);
    p.ld0 = m.sizes[0] | 1;
    p.ldx = maxh | 1;
    const int plane = ac_up4(R * p.ldx);
    p.xa_off = ac_up4(R * p.ld0);
    p.xb_off = p.xa_off + plane;
    p.ta_off = p.xb_off + plane;
    p.tb_off = p.ta_off + plane;
    p.w_off = p.tb_off + plane;   // 16-byte aligned: the weight quads are read as one f32x4
    const long long wfloats = (long long)(limit / sizeof(float)) - p.w_off;
    if (wfloats <= 0) return 0;
    long long used = 0;
    for (int j = 0; j < m.n_layers - 1; ++j) {
        const int K = m.sizes[j], N = m.sizes[j + 1];
        int nc = (int)std::min<long long>(N, (wfloats / (2 * (K + 1))) & ~15LL);
        if (nc < std::min(N, min_nc)) return 0;
        p.nc[j] = nc;
        used = std::max(used, 2LL * (K + 1) * nc);
    }
    const long long staged = 2LL * (m.sizes[m.n_layers - 1] + 1) * m.sizes[m.n_layers];   // (even: doubles behind it are 8-byte aligned)
    const long long head = staged + 2LL * park * R;
    if (head > wfloats) return 0;
    p.park_off = p.w_off + (int)staged;
    used = std::max(used, head);
    return ((size_t)p.w_off + (size_t)used) * sizeof(float);
}

size_t fs_choose(const GopsMlp& m, int B, int park, FsParams& p, int& R) {
    return ac_choose_rows(B, R, [&](int rows, size_t limit, int min_nc) { return fs_plan(m, rows, limit, min_nc, park, p); });
}

// h = act(z), d = act'(z) as torch evaluates them (common.h: act3_t, fp32 libm - erf-form GELU, expm1f for ELU / SELU).  The fast
// forms of the rollout kernels' forward (polynomial Phi, hardware exp: absolute error ~1e-7) would be the largest term of a seed's
// error; here the product feeds ten conjugate-gradient iterations.
template <int ACT>
__device__ __forceinline__ void fs_act(float z, float& h, float& d) {
    float d2;
    act3_t<ACT>(z, h, d, d2);
}

// ---- the heads of fisher_seed_kernel: run<R>(p, lds, xr, tr, wb, K, N, r, g, nvalid, out) - thread (r, g) of a tile of R rows; xr, tr: the
// row's last hidden activations and their tangents; wb: the staged output layer (W_L [N][K], b_L [N], then V_L, c_L likewise); out: the
// row's N seed values (rows r >= nvalid are evaluated on zeros and never stored).  Every thread of the workgroup calls run.
// Gaussian (N = 2A: means, then raw log stds): one thread per (row, action dimension); the tangent scaled by the metric of the Gaussian's
// KL, M = diag(1 / sigma^2, 2 inside the clamp | 0 outside), sigma = exp(clamp(raw)) of the primal it has just formed, and by 1 / B.
struct GaussHead {
    static int park(int) { return 0; }   // doubles per tile row behind the staged output layer
    template <int R>
    static __device__ __forceinline__ void run(const FsParams& p, float*, const float* xr, const float* tr, const float* wb, int K, int N,
                                               int r, int g, int nvalid, float* out) {
        const int A = p.A;
        if (g < A && r < nvalid) {
            const float* vb = wb + N * K + N;
            const double raw = ac_head_dot(xr, wb + (A + g) * K, K) + (double)wb[N * K + A + g];
            const double t_mean = (ac_head_dot(tr, wb + g * K, K) + ac_head_dot(xr, vb + g * K, K)) + (double)vb[N * K + g];
            const double t_raw = (ac_head_dot(tr, wb + (A + g) * K, K) + ac_head_dot(xr, vb + (A + g) * K, K)) + (double)vb[N * K + A + g];
            const GaussDim n = gauss_dim(raw, p.min_ls, p.max_ls);
            const double inv_b = 1.0 / (double)p.B;
            out[g] = (float)(t_mean / (n.sd * n.sd) * inv_b);
            out[A + g] = n.inside ? (float)(2.0 * t_raw * inv_b) : 0.f;
        }
    }
};

// Categorical (N logits): thread (r, g) forms the logits z_k and their tangents u_k of k = g, g + 256 / R, .. in double and parks them in
// LDS ([N][R] each, dqn_backup_kernel's scheme); behind the barrier every thread with an output walks its row in index order -
// m = max z, S = sum exp(z - m), pu = sum (exp(z - m) / S) u - and stores p_k (u_k - pu) / B: the softmax Fisher metric
// diag(p) - p p^T applied to u.  The order depends on N alone: the same bits whatever R is.
struct CatHead {
    static int park(int N) { return 2 * N; }   // z and u of every logit
    template <int R>
    static __device__ __forceinline__ void run(const FsParams& p, float* lds, const float* xr, const float* tr, const float* wb, int K, int N,
                                               int r, int g, int nvalid, float* out) {
        constexpr int G = AC_THREADS / R;
        double* zq = reinterpret_cast<double*>(lds + p.park_off);
        double* uq = zq + N * R;
        const float* vb = wb + N * K + N;
        for (int k = g; k < N; k += G) {
            zq[k * R + r] = ac_head_dot(xr, wb + k * K, K) + (double)wb[N * K + k];
            uq[k * R + r] = (ac_head_dot(tr, wb + k * K, K) + ac_head_dot(xr, vb + k * K, K)) + (double)vb[N * K + k];
        }
        __syncthreads();
        if (g < N && r < nvalid) {
            double m = zq[r];
            for (int k = 1; k < N; ++k) m = fmax(m, zq[k * R + r]);
            double S = 0.0, pu = 0.0;
            for (int k = 0; k < N; ++k) S += exp(zq[k * R + r] - m);
            for (int k = 0; k < N; ++k) pu += exp(zq[k * R + r] - m) / S * uq[k * R + r];
            for (int k = g; k < N; k += G) out[k] = (float)(exp(zq[k * R + r] - m) / S * (uq[k * R + r] - pu) / (double)p.B);
        }
    }
};

template <int R, typename Head>
__global__ __launch_bounds__(AC_THREADS) void fisher_seed_kernel(const FsParams p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int G = AC_THREADS / R;
    const int tid = threadIdx.x, r = tid % R, g = tid / R;
    const int b0 = blockIdx.x * R, nvalid = min(R, p.B - b0), O = p.O, ldx = p.ldx;
    float *in0 = lds, *xa = lds + p.xa_off, *xb = lds + p.xb_off, *ta = lds + p.ta_off, *tb = lds + p.tb_off, *wb = lds + p.w_off;
    for (int idx = tid; idx < R * O; idx += AC_THREADS) {   // rows beyond the batch: zeros (evaluated, never stored)
        const int m = idx / O, k = idx - m * O;
        in0[m * p.ld0 + k] = m < nvalid ? p.x[(size_t)(b0 + m) * O + k] : 0.f;
    }
    const float *cur = in0, *curt = ta;   // (curt is not read in layer 0: t_0 = 0)
    int ldc = p.ld0;
    float *nxt = xa, *nxtt = ta;
#pragma unroll 1
    for (int j = 0; j < p.nl - 1; ++j) {
        const int K = p.dims[j], N = p.dims[j + 1], NC = p.nc[j];
        const float* __restrict__ Wg = p.W[j];
        const float* __restrict__ Vg = p.V[j];
        float* vb = wb + (K + 1) * NC;   // the tangent's chunk, behind W's chunk and biases
        const bool first = j == 0;
#pragma unroll 1
        for (int n0 = 0; n0 < N; n0 += NC) {
            const int nc = min(NC, N - n0);
            __syncthreads();   // the previous readers of wb are done; what the previous layer (or the staging above) wrote is visible
            for (int idx = tid; idx < nc * K; idx += AC_THREADS) {
                const int k = idx / nc, nn = idx - k * nc;
                wb[k * NC + nn] = Wg[(size_t)(n0 + nn) * K + k];
                vb[k * NC + nn] = Vg[(size_t)(n0 + nn) * K + k];
            }
            for (int idx = tid; idx < nc; idx += AC_THREADS) {
                wb[K * NC + idx] = p.Bv[j][n0 + idx];
                vb[K * NC + idx] = p.Cv[j][n0 + idx];
            }
            __syncthreads();
            const float* xr = cur + r * ldc;
            const float* tr = curt + r * ldx;
            act_dispatch(p.act, [&]<int ACT>() {
                for (int fg = g; fg < (nc >> 2); fg += G) {
                    const float* wq = wb + 4 * fg;
                    const float* vq = vb + 4 * fg;
                    f32x4 c[AC_CHAINS], cu[AC_CHAINS], cv[AC_CHAINS];
#pragma unroll
                    for (int i = 0; i < AC_CHAINS; ++i) c[i] = cu[i] = cv[i] = f32x4{0.f, 0.f, 0.f, 0.f};
                    const int K8 = K & ~(AC_CHAINS - 1);
                    auto term = [&](int k, int i) {
                        const float x = xr[k];
                        const f32x4 w = *reinterpret_cast<const f32x4*>(wq + k * NC);
                        const f32x4 v = *reinterpret_cast<const f32x4*>(vq + k * NC);
                        if (!first) {
                            const float t = tr[k];
#pragma unroll
                            for (int e = 0; e < 4; ++e) cu[i][e] = fmaf(t, w[e], cu[i][e]);
                        }
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            c[i][e] = fmaf(x, w[e], c[i][e]);
                            cv[i][e] = fmaf(x, v[e], cv[i][e]);
                        }
                    };
                    for (int k = 0; k < K8; k += AC_CHAINS) {
#pragma unroll
                        for (int i = 0; i < AC_CHAINS; ++i) term(k + i, i);
                    }
#pragma unroll
                    for (int i = 0; i < AC_CHAINS - 1; ++i)
                        if (K8 + i < K) term(K8 + i, i);
                    const float* bq = wb + K * NC + 4 * fg;
                    const float* cq = vb + K * NC + 4 * fg;
                    float* yr = nxt + r * ldx + n0 + 4 * fg;
                    float* ur = nxtt + r * ldx + n0 + 4 * fg;
                    const f32x4 wh = chain_sum8(c), wt = chain_sum8(cu), vh = chain_sum8(cv);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float z = wh[e] + bq[e];
                        const float u = (wt[e] + vh[e]) + cq[e];
                        float h, d;
                        fs_act<ACT>(z, h, d);
                        yr[e] = h;
                        ur[e] = d * u;
                    }
                }
            });
        }
        cur = nxt, curt = nxtt, ldc = ldx;
        nxt = nxt == xa ? xb : xa;
        nxtt = nxtt == ta ? tb : ta;
    }
    // ---- head: W_L [N][K] with b_L behind it, V_L and c_L behind those ----
    const int L = p.nl - 1, K = p.dims[L], N = p.dims[L + 1];
    __syncthreads();
    for (int idx = tid; idx < N * K; idx += AC_THREADS) wb[idx] = p.W[L][idx], wb[N * K + N + idx] = p.V[L][idx];
    for (int idx = tid; idx < N; idx += AC_THREADS) wb[N * K + idx] = p.Bv[L][idx], wb[2 * N * K + N + idx] = p.Cv[L][idx];
    __syncthreads();
    Head::template run<R>(p, lds, cur + r * ldx, curt + r * ldx, wb, K, N, r, g, nvalid, p.seed + (size_t)(b0 + r) * N);
}

// ---- surrogate advantage, KL and the line search's verdict (trpo.py:133-138, 148, 185-196) ---------------------------------------
constexpr int TS_BLOCKS = 64;
constexpr int TS_VERDICT_AT = 2;   // int32 behind the two results, one spare float behind it
constexpr int TS_PART_AT = 4;      // the blocks' partial sums
constexpr int TS_PART = 2;

__global__ __launch_bounds__(256) void trpo_surrogate_kernel(int M, int A, double min_ls, double max_ls, const float* head_new,
                                                             const float* head_old, const float* __restrict__ act,
                                                             const float* __restrict__ adv, const float* __restrict__ hyper,
                                                             float* __restrict__ seed, float* __restrict__ stats) {
    __shared__ double red[TS_PART][4];
    __shared__ bool last;
    double* part = reinterpret_cast<double*>(stats + TS_PART_AT);   // [TS_BLOCKS][TS_PART]
    unsigned* ticket = reinterpret_cast<unsigned*>(stats + TS_PART_AT + 2 * TS_PART * TS_BLOCKS);
    const double inv_m = 1.0 / (double)M;
    double s[2] = {0.0, 0.0};   // sum ratio adv, sum kl
    for (int i = blockIdx.x * 256 + threadIdx.x; i < M; i += gridDim.x * 256) {
        const float* hn = head_new + (size_t)i * 2 * A;
        const float* ho = head_old + (size_t)i * 2 * A;
        double lpn = 0.0, lpo = 0.0, kl = 0.0;
        for (int a = 0; a < A; ++a) {
            const double x = (double)act[(size_t)i * A + a];
            const double mn = (double)hn[a], mo = (double)ho[a];
            const GaussDim n = gauss_dim((double)hn[A + a], min_ls, max_ls), o = gauss_dim((double)ho[A + a], min_ls, max_ls);
            lpn += gauss_logp_term(x - mn, n.ls, n.sd);
            lpo += gauss_logp_term(x - mo, o.ls, o.sd);
            kl += gauss_kl_term(n.ls, n.sd, mn, o.ls, o.sd, mo);   // KL(N(new) || N(old))
        }
        const double ratio = exp(lpn - lpo), ad = (double)adv[i];
        if (seed != nullptr) {
            const double g_lp = inv_m * ad * ratio;   // d surrogate / d logp_new of the row
            for (int a = 0; a < A; ++a) {
                const GaussDim n = gauss_dim((double)hn[A + a], min_ls, max_ls);
                const GaussSeed g = gauss_logp_seed(g_lp, (double)act[(size_t)i * A + a] - (double)hn[a], 1.0 / (n.sd * n.sd), n.inside);
                seed[(size_t)i * 2 * A + a] = (float)g.mean;
                seed[(size_t)i * 2 * A + A + a] = (float)g.ls;
            }
        }
        s[0] += ratio * ad, s[1] += kl;
    }
    if (grid_fold<2>(s, red, part, TS_PART, ticket, &last) && threadIdx.x == 0) {
        const float sur = (float)(s[0] * inv_m), kl = (float)(s[1] * inv_m);   // (the reference compares its fp32 values)
        stats[0] = sur, stats[1] = kl;
        reinterpret_cast<int*>(stats)[TS_VERDICT_AT] = sur > 0.f && kl < hyper[0] ? 1 : 0;
    }
}
static_assert(TS_PART_AT + 2 * TS_PART * TS_BLOCKS + 1 <= GOPS_TRPO_STATS_FLOATS, "stats: results, the verdict, the blocks' partial sums, the ticket");

// ---- the same for a categorical policy (CategoricalDistribution's log_prob and kl_divergence on the logits) ------------------------
constexpr int TS_BAD_AT = 3;                                        // int32: rows whose index is outside [0, N)
constexpr int TS_BAD_ACC_AT = TS_PART_AT + 2 * TS_PART * TS_BLOCKS + 1;   // int32 behind the ticket: the running count, zero between launches
static_assert(TS_BAD_ACC_AT < GOPS_TRPO_STATS_FLOATS, "stats: the running count of bad rows behind the ticket");

// max_k z_k and sum_k exp(z_k - max) in index order
__device__ __forceinline__ void cat_max_sum(const float* z, int N, double& m, double& S) {
    m = (double)z[0];
    for (int k = 1; k < N; ++k) m = fmax(m, (double)z[k]);
    S = 0.0;
    for (int k = 0; k < N; ++k) S += exp((double)z[k] - m);
}

// One thread per row.  The two sums go through grid_fold as trpo_surrogate_kernel's do; the count of bad rows is an integer: thread 0 of
// a block adds the block's count to the running count (exact in any order) before it parks the block's sums and draws its ticket, and
// the thread that stores the results takes the total and leaves zero.
__global__ __launch_bounds__(256) void cat_surrogate_kernel(int M, int N, const float* logits_new, const float* logits_old,
                                                            const float* __restrict__ act, const float* __restrict__ adv,
                                                            const float* __restrict__ hyper, float* __restrict__ seed,
                                                            float* __restrict__ stats) {
    __shared__ double red[TS_PART][4];
    __shared__ bool last;
    double* part = reinterpret_cast<double*>(stats + TS_PART_AT);   // [TS_BLOCKS][TS_PART]
    unsigned* ticket = reinterpret_cast<unsigned*>(stats + TS_PART_AT + 2 * TS_PART * TS_BLOCKS);
    int* bad_acc = reinterpret_cast<int*>(stats) + TS_BAD_ACC_AT;
    const double inv_m = 1.0 / (double)M;
    double s[2] = {0.0, 0.0};   // sum ratio adv, sum kl
    double bad[1] = {0.0};
    for (int i = blockIdx.x * 256 + threadIdx.x; i < M; i += gridDim.x * 256) {
        const float af = act[i];
        const bool ok = af > -1.f && af < (float)N;   // truncation towards zero lands in [0, N); false for a NaN
        float* srow = seed != nullptr ? seed + (size_t)i * N : nullptr;
        if (!ok) {
            bad[0] += 1.0;
            if (srow != nullptr)
                for (int k = 0; k < N; ++k) srow[k] = 0.f;
            continue;
        }
        const int a = (int)af;
        const float* zn = logits_new + (size_t)i * N;
        const float* zo = logits_old + (size_t)i * N;
        double mn, Sn, mo, So;
        cat_max_sum(zn, N, mn, Sn);
        cat_max_sum(zo, N, mo, So);
        const double lse_n = mn + log(Sn), lse_o = mo + log(So);
        double kl = 0.0;
        for (int k = 0; k < N; ++k) {   // KL(new || old); a p_new that underflows to 0 contributes 0
            const double zk = (double)zn[k];
            kl += exp(zk - mn) / Sn * ((zk - lse_n) - ((double)zo[k] - lse_o));
        }
        const double ratio = exp(((double)zn[a] - lse_n) - ((double)zo[a] - lse_o)), ad = (double)adv[i];
        if (srow != nullptr) {
            const double g_lp = inv_m * ad * ratio;   // d surrogate / d logp_new[a] of the row; d logp_new[a] / d z_k = (k == a) - p_new,k
            for (int k = 0; k < N; ++k) srow[k] = (float)(g_lp * ((k == a ? 1.0 : 0.0) - exp((double)zn[k] - mn) / Sn));
        }
        s[0] += ratio * ad, s[1] += kl;
    }
    block_fold<1, false>(bad, red);
    if (threadIdx.x == 0 && bad[0] != 0.0) atomicAdd(bad_acc, (int)bad[0]);   // (ordered before this block's ticket by last_block's fence)
    if (grid_fold<2>(s, red, part, TS_PART, ticket, &last) && threadIdx.x == 0) {
        const float sur = (float)(s[0] * inv_m), kl = (float)(s[1] * inv_m);
        stats[0] = sur, stats[1] = kl;
        reinterpret_cast<int*>(stats)[TS_VERDICT_AT] = sur > 0.f && kl < hyper[0] ? 1 : 0;
        reinterpret_cast<int*>(stats)[TS_BAD_AT] = atomicExch(bad_acc, 0);
    }
}

// ---- conjugate gradients (trpo.py:226-267) ---------------------------------------------------------------------------------------
constexpr int CG_BLOCKS = 64;
constexpr double CG_EPS = 1e-8;   // trpo.py:35
static_assert(sizeof(GopsCgState) == GOPS_CG_STATE_FLOATS * sizeof(float) && sizeof(GopsCgState::part) == 2 * CG_BLOCKS * sizeof(double),
              "GopsCgState: the scalars, the counters, 64 blocks' two partial sums");

// The sums of the block's (or, in the block that draws the last ticket, the grid's) `s`; true where they are final.
__device__ __forceinline__ bool cg_fold(double (&s)[2], GopsCgState* st, double (*red)[4], bool* last) {
    return grid_fold<2>(s, red, st->part, 2, reinterpret_cast<unsigned*>(&st->ticket), last);
}

// x = 0, r = p = g, r_dot = r.r, done = all(|r| <= atol)   (the reference's first Ax(x0) is a product with zero: not formed)
__global__ __launch_bounds__(256) void cg_init_kernel(const float* __restrict__ gvec, float* __restrict__ x, float* __restrict__ r,
                                                      float* __restrict__ p, int n, double atol, GopsCgState* st) {
    __shared__ double red[2][4];
    __shared__ bool last;
    double s[2] = {0.0, 0.0};   // r.r, elements with not |r| <= atol
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const float v = gvec[i];
        x[i] = 0.f, r[i] = v, p[i] = v;
        s[0] += (double)v * (double)v, s[1] += fabs((double)v) <= atol ? 0.0 : 1.0;
    }
    if (cg_fold(s, st, red, &last) && threadIdx.x == 0) {
        st->r_dot = s[0], st->p_ap = 0.0, st->alpha = 0.0, st->beta = 0.0, st->g_x = 0.0, st->scale = 0.0;
        st->done = s[1] == 0.0 ? 1 : 0, st->calls = 0, st->iterations = 0;
    }
}

// One iteration in three phases (bits 1, 2, 4): one workgroup runs all three in one launch; 64 workgroups one phase per launch.
// Every thread owns the same elements in every phase, so inside one workgroup only the scalars cross threads (through cg_fold).
__global__ __launch_bounds__(256) void cg_step_kernel(int phases, float* __restrict__ p, float* __restrict__ Ap, float* __restrict__ x,
                                                      float* __restrict__ r, int n, double damping, double atol, GopsCgState* st) {
    __shared__ double red[2][4];
    __shared__ bool last;
    const int first = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
    const bool done_in = st->done != 0;   // (phases 1 and 2: as the call found it; phase 4: as phase 2 left it)
    if (phases & 1) {
        if (blockIdx.x == 0 && threadIdx.x == 0) st->calls = st->calls + 1;
    }
    if (done_in) return;   // nothing changes once the residual is within atol
    double alpha = 0.0, beta = 0.0;
    bool done = false;
    if (phases & 1) {   // Ap += damping p;  alpha = r_dot / (p.Ap + 1e-8)
        double s[2] = {0.0, 0.0};
        for (int i = first; i < n; i += stride) {
            const float pi = p[i], ap = (float)((double)Ap[i] + damping * (double)pi);
            Ap[i] = ap;
            s[0] += (double)pi * (double)ap;
        }
        const bool fin = cg_fold(s, st, red, &last);
        alpha = st->r_dot / (s[0] + CG_EPS);   // (final where fin; one workgroup: in every thread)
        if (fin && threadIdx.x == 0) st->p_ap = s[0], st->alpha = alpha;
        if (phases == 1) return;
    } else {
        alpha = st->alpha;
    }
    if (phases & 2) {   // x += alpha p;  r -= alpha Ap;  done = all(|r| <= atol);  beta = r_dot' / (r_dot + 1e-8)
        double s[2] = {0.0, 0.0};
        const double r_dot = st->r_dot;
        for (int i = first; i < n; i += stride) {
            x[i] = (float)((double)x[i] + alpha * (double)p[i]);
            const float rn = (float)((double)r[i] - alpha * (double)Ap[i]);
            r[i] = rn;
            s[0] += (double)rn * (double)rn, s[1] += fabs((double)rn) <= atol ? 0.0 : 1.0;
        }
        __syncthreads();   // (one workgroup: every thread has read st->r_dot before thread 0 replaces it)
        const bool fin = cg_fold(s, st, red, &last);
        beta = s[0] / (r_dot + CG_EPS), done = s[1] == 0.0;
        if (fin && threadIdx.x == 0) {
            st->r_dot = s[0], st->beta = beta, st->iterations = st->iterations + 1;
            st->done = done ? 1 : 0;
        }
        if (phases == 2) return;
    } else {
        beta = st->beta;
    }
    if (done) return;
    for (int i = first; i < n; i += stride) p[i] = (float)((double)r[i] + beta * (double)p[i]);   // p = r + beta p
}

// step = sqrt(2 delta / (g.x + 1e-8)) x   (trpo.py:175-177); phases 1 (the dot), 2 (the scaling)
__global__ __launch_bounds__(256) void cg_finish_kernel(int phases, const float* __restrict__ gvec, const float* __restrict__ x,
                                                        float* __restrict__ step, int n, const float* __restrict__ hyper, GopsCgState* st) {
    __shared__ double red[2][4];
    __shared__ bool last;
    double scale;
    if (phases & 1) {
        double s[2] = {0.0, 0.0};
        for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) s[0] += (double)gvec[i] * (double)x[i];
        const bool fin = cg_fold(s, st, red, &last);
        scale = sqrt(2.0 * (double)hyper[0] / (s[0] + CG_EPS));
        if (fin && threadIdx.x == 0) st->g_x = s[0], st->scale = scale;
        if (phases == 1) return;
    } else {
        scale = st->scale;
    }
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) step[i] = (float)(scale * (double)x[i]);
}

// What both fisher-seed entry points do behind their checks: the plan (GOPS_ERR_UNSUPPORTED when none fits), the fill, the launch.
template <typename Head>
int fs_launch(const GopsMlp& m, const GopsMlpGrad& tangent, int B, int A, const float* x, double min_ls, double max_ls, float* seed,
              hipStream_t s) {
    FsParams p;
    memset(&p, 0, sizeof(p));
    int R;
    const size_t lds = fs_choose(m, B, Head::park(m.sizes[m.n_layers]), p, R);
    if (lds == 0) return GOPS_ERR_UNSUPPORTED;
    p.nl = m.n_layers, p.act = m.hidden_act, p.B = B, p.O = m.sizes[0], p.A = A;
    for (int j = 0; j <= p.nl; ++j) p.dims[j] = m.sizes[j];
    for (int j = 0; j < p.nl; ++j) p.W[j] = m.weight[j], p.Bv[j] = m.bias[j], p.V[j] = tangent.weight[j], p.Cv[j] = tangent.bias[j];
    p.min_ls = min_ls, p.max_ls = max_ls, p.x = x, p.seed = seed;
    const dim3 grid((unsigned)((B + R - 1) / R)), threads(AC_THREADS);
    rows_dispatch(R, [&]<int RR>() { launch_with_lds(fisher_seed_kernel<RR, Head>, grid, threads, lds, s, p); });
    return (int)hipGetLastError();
}

bool cg_state_ok(const GopsCgState* st, int n) { return st && n >= 1 && stats_aligned(st); }

}  // namespace

extern "C" {

int gops_gauss_fisher_seed(const GopsMlp* policy, const GopsMlpGrad* tangent_in, int32_t B, const float* x, double min_ls, double max_ls,
                           float* seed, void* stream) {
    if (!policy || !tangent_in || !x || !seed || B < 1) return GOPS_ERR_BAD_ARG;
    if (policy->n_layers < 1 || policy->n_layers > GOPS_MAX_LAYERS) return GOPS_ERR_BAD_ARG;
    const GopsMlp& m = *policy;
    const GopsMlpGrad& tangent = *tangent_in;
    const int O = m.sizes[0], A2 = m.sizes[m.n_layers], A = A2 / 2;
    if (O < 1 || A < 1 || (A2 & 1) || A > GOPS_MAX_ACT) return GOPS_ERR_BAD_ARG;
    if (O > 64) return GOPS_ERR_UNSUPPORTED;
    const int rc = ac_check_net(m, O, A2);
    if (rc != GOPS_OK) return rc;
    for (int j = 0; j < m.n_layers; ++j)
        if (tangent.weight[j] == nullptr || tangent.bias[j] == nullptr) return GOPS_ERR_BAD_ARG;
    return fs_launch<GaussHead>(m, tangent, B, A, x, min_ls, max_ls, seed, static_cast<hipStream_t>(stream));
}

int gops_cat_fisher_seed(const GopsMlp* policy, const GopsMlpGrad* tangent_in, int32_t B, const float* x, float* seed, void* stream) {
    if (!policy || !tangent_in || !x || !seed || B < 1) return GOPS_ERR_BAD_ARG;
    if (policy->n_layers < 1 || policy->n_layers > GOPS_MAX_LAYERS) return GOPS_ERR_BAD_ARG;
    const GopsMlp& m = *policy;
    const GopsMlpGrad& tangent = *tangent_in;
    const int O = m.sizes[0], N = m.sizes[m.n_layers];
    if (O < 1 || N < 1) return GOPS_ERR_BAD_ARG;
    if (N < 2 || N > GOPS_DQN_MAX_ACTIONS || O > 64) return GOPS_ERR_UNSUPPORTED;
    const int rc = ac_check_net(m, O, N);
    if (rc != GOPS_OK) return rc;
    for (int j = 0; j < m.n_layers; ++j)
        if (tangent.weight[j] == nullptr || tangent.bias[j] == nullptr) return GOPS_ERR_BAD_ARG;
    return fs_launch<CatHead>(m, tangent, B, 0, x, 0.0, 0.0, seed, static_cast<hipStream_t>(stream));
}

int gops_trpo_surrogate(int32_t A, int32_t M, double min_ls, double max_ls, const float* head_new, const float* head_old, const float* act,
                        const float* adv, const float* hyper, float* seed, float* stats, void* stream) {
    if (M < 1 || A < 1 || A > GOPS_MAX_ACT) return GOPS_ERR_BAD_ARG;
    if (!head_new || !head_old || !act || !adv || !hyper || !stats) return GOPS_ERR_BAD_ARG;
    if (!stats_aligned(stats)) return GOPS_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(trpo_surrogate_kernel, dim3(M <= LOSS_ONE_BLOCK_MAX ? 1 : TS_BLOCKS), dim3(256), 0, s, M, A, min_ls, max_ls, head_new,
                       head_old, act, adv, hyper, seed, stats);
    return (int)hipGetLastError();
}

int gops_cat_trpo_surrogate(int32_t N, int32_t M, const float* logits_new, const float* logits_old, const float* act, const float* adv,
                            const float* hyper, float* seed, float* stats, void* stream) {
    if (M < 1 || N < 1) return GOPS_ERR_BAD_ARG;
    if (!logits_new || !logits_old || !act || !adv || !hyper || !stats) return GOPS_ERR_BAD_ARG;
    if (!stats_aligned(stats)) return GOPS_ERR_BAD_ARG;
    if (N < 2 || N > GOPS_DQN_MAX_ACTIONS) return GOPS_ERR_UNSUPPORTED;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(cat_surrogate_kernel, dim3(M <= LOSS_ONE_BLOCK_MAX ? 1 : TS_BLOCKS), dim3(256), 0, s, M, N, logits_new, logits_old, act,
                       adv, hyper, seed, stats);
    return (int)hipGetLastError();
}

int gops_cg_init(const float* g, float* x, float* r, float* p, int32_t n, double atol, GopsCgState* st, void* stream) {
    if (!g || !x || !r || !p || !cg_state_ok(st, n)) return GOPS_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(cg_init_kernel, dim3(n <= GOPS_CG_ONE_BLOCK_MAX ? 1 : CG_BLOCKS), dim3(256), 0, s, g, x, r, p, n, atol, st);
    return (int)hipGetLastError();
}

int gops_cg_step(float* p, float* Ap, float* x, float* r, int32_t n, double damping, double atol, GopsCgState* st, void* stream) {
    if (!p || !Ap || !x || !r || !cg_state_ok(st, n)) return GOPS_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n <= GOPS_CG_ONE_BLOCK_MAX) {
        hipLaunchKernelGGL(cg_step_kernel, dim3(1), dim3(256), 0, s, 7, p, Ap, x, r, n, damping, atol, st);
    } else {
        for (int phase = 1; phase <= 4; phase <<= 1)
            hipLaunchKernelGGL(cg_step_kernel, dim3(CG_BLOCKS), dim3(256), 0, s, phase, p, Ap, x, r, n, damping, atol, st);
    }
    return (int)hipGetLastError();
}

int gops_cg_finish(const float* g, const float* x, float* step, int32_t n, const float* hyper, GopsCgState* st, void* stream) {
    if (!g || !x || !step || !hyper || !cg_state_ok(st, n)) return GOPS_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n <= GOPS_CG_ONE_BLOCK_MAX) {
        hipLaunchKernelGGL(cg_finish_kernel, dim3(1), dim3(256), 0, s, 3, g, x, step, n, hyper, st);
    } else {
        hipLaunchKernelGGL(cg_finish_kernel, dim3(CG_BLOCKS), dim3(256), 0, s, 1, g, x, step, n, hyper, st);
        hipLaunchKernelGGL(cg_finish_kernel, dim3(CG_BLOCKS), dim3(256), 0, s, 2, g, x, step, n, hyper, st);
    }
    return (int)hipGetLastError();
}

}  // extern "C"
