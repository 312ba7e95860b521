// Batched box-constrained L-BFGS for shooting MPC (gops_mpc_state_bytes / _init / _step / _finish / _advance and the block-writing halves of the
// augmented Lagrangian, gops_mpc_al_update / _al_advance, of include/gops_hip.h): B independent
// problems of n variables, each moved by one call of gops_mpc_step per cost-and-gradient evaluation, with no value read on the host.
//
// Work assignment: a sub-group of W lanes owns one problem - W = 64 (one wave per problem) for n > 64, else the smallest of
// 4, 8, 16, 32 with 2 W >= n, so that several problems share a wave.  Lane l owns the elements l, l + W, .. of EVERY vector of
// its problem, so nothing but the scalars crosses lanes, and those cross through sub_sum / sub_max: each lane adds its own elements
// in index order in double, then the xor butterfly (W / 2, .., 1) of block_reduce.h's block_fold, which leaves the same bits in
// every lane.  No atomics, no LDS; every stored float is formed in double and rounded once.  A problem's arithmetic sees neither B
// nor its row index, so its bits depend on neither.
//
// State block (gops_hip.h has the same table): [B][GOPS_MPC_SCALARS + m] doubles, [B][GOPS_MPC_COUNTERS] int32, lo [n], hi [n],
// [B][GOPS_MPC_VECTORS + 2 m][n] floats - a problem's vectors are contiguous rows of n floats, so the lanes of a sub-group read
// consecutive addresses.  The ring of (s, y) pairs stays in global memory (L2-resident at these sizes); the recursion keeps only
// q (E doubles) and the m coefficients in registers.
#include "common.h"

// No fused multiply-adds in this file: x + alpha d and the like are a rounded product and a rounded sum in double, as the rule in
// gops_hip.h states them, so that a restatement in plain IEEE double arithmetic reproduces every stored float.
#pragma clang fp contract(off)

namespace {

constexpr int MPC_THREADS = 256;
enum { SC_F, SC_F_PREV, SC_ALPHA, SC_DPHI, SC_GAMMA, SC_RHO };                                     // doubles of one problem
enum { CT_STATUS, CT_ITER, CT_EVAL, CT_LS, CT_HEAD, CT_COUNT };                                     // int32 of one problem
enum { VE_X, VE_G, VE_X_PREV, VE_G_PREV, VE_D, VE_X_TRIAL, VE_RING };                               // rows of n floats
enum { HY_C1, HY_SHRINK, HY_MAX_LS, HY_PGTOL, HY_FTOL, HY_CURV_EPS };
static_assert(SC_RHO == GOPS_MPC_SCALARS && VE_RING == GOPS_MPC_VECTORS && CT_COUNT < GOPS_MPC_COUNTERS && HY_CURV_EPS < GOPS_MPC_HYPER_FLOATS,
              "the state block's table in gops_hip.h");

struct MpcBlock {   // the sections of one state block
    double* scalars;
    int32_t* counters;
    float *lo, *hi, *vectors;
};

__host__ __device__ inline size_t mpc_bounds_floats(int n) { return 2 * (size_t)((n + 1) & ~1); }   // (keeps the vectors 8-byte aligned)
__host__ __device__ inline MpcBlock mpc_sections(void* state, int B, int n, int m) {
    MpcBlock b;
    b.scalars = static_cast<double*>(state);
    b.counters = reinterpret_cast<int32_t*>(b.scalars + (size_t)B * (GOPS_MPC_SCALARS + m));
    b.lo = reinterpret_cast<float*>(b.counters + (size_t)B * GOPS_MPC_COUNTERS);
    b.hi = b.lo + mpc_bounds_floats(n) / 2;
    b.vectors = b.lo + mpc_bounds_floats(n);
    return b;
}
inline size_t mpc_bytes(int B, int n, int m) {
    return (size_t)B * (GOPS_MPC_SCALARS + m) * sizeof(double) + (size_t)B * GOPS_MPC_COUNTERS * sizeof(int32_t) +
           mpc_bounds_floats(n) * sizeof(float) + (size_t)B * (GOPS_MPC_VECTORS + 2 * m) * n * sizeof(float);
}

template <int W>
__device__ __forceinline__ double sub_sum(double v) {
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
template <int W>
__device__ __forceinline__ double sub_max(double v) {
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double clampd(double v, double lo, double hi) { return fmin(fmax(v, lo), hi); }

// One problem as its sub-group sees it: E elements per lane, element e of lane l is l + e W.
template <int W>
struct Problem {
    static constexpr int E = W == 64 ? GOPS_MPC_MAX_DIM / 64 : 2;
    int n, m, lane;
    double* sc;
    int32_t* ct;
    const float *lo, *hi;
    float* vec;

    __device__ __forceinline__ float* row(int r) const { return vec + (size_t)r * n; }
    __device__ __forceinline__ float* ring_s(int k) const { return row(VE_RING + k); }
    __device__ __forceinline__ float* ring_y(int k) const { return row(VE_RING + m + k); }
    // free: not on a bound with the gradient pointing outward
    __device__ __forceinline__ bool is_free(int i, float x, float g) const { return !((x <= lo[i] && g > 0.f) || (x >= hi[i] && g < 0.f)); }

    __device__ __forceinline__ void copy_out(int r, float* dst) const {
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int i = lane + e * W;
            if (i < n) dst[i] = row(r)[i];
        }
    }

    // d <- -g on the free variables, 0 on the fixed ones; returns |d|
    __device__ __forceinline__ double steepest() const {
        double dd = 0.0;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int i = lane + e * W;
            if (i < n) {
                const float g = row(VE_G)[i], d = is_free(i, row(VE_X)[i], g) ? -g : 0.f;
                row(VE_D)[i] = d;
                dd += (double)d * (double)d;
            }
        }
        return sqrt(sub_sum<W>(dd));
    }

    // d <- -H g restricted to the free variables: the two-loop recursion over the `count` newest pairs, newest at head - 1.
    // Every sub-group walks all m slots (a slot that holds no pair contributes a zero coefficient), so the walk is uniform.
    // (slot `fresh` was pushed by this very call: its rho and gamma come in registers, the other slots' from the block)
    __device__ __forceinline__ void two_loop(int head, int count, int fresh, double rho_fresh, double gamma_fresh) const {
        double q[E], a[GOPS_MPC_MAX_HISTORY];
        bool fr[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int i = lane + e * W;
            fr[e] = false, q[e] = 0.0;
            if (i < n) {
                const float g = row(VE_G)[i];
                fr[e] = is_free(i, row(VE_X)[i], g);
                q[e] = fr[e] ? (double)g : 0.0;
            }
        }
#pragma unroll
        for (int j = 0; j < GOPS_MPC_MAX_HISTORY; ++j) {
            a[j] = 0.0;
            if (j < m) {
                const int k = (head + 2 * m - 1 - j) % m;
                double t = 0.0;
#pragma unroll
                for (int e = 0; e < E; ++e)
                    if (fr[e]) t += (double)ring_s(k)[lane + e * W] * q[e];
                t = sub_sum<W>(t);
                a[j] = j < count ? (k == fresh ? rho_fresh : sc[SC_RHO + k]) * t : 0.0;
#pragma unroll
                for (int e = 0; e < E; ++e)
                    if (fr[e]) q[e] -= a[j] * (double)ring_y(k)[lane + e * W];
            }
        }
        const double gamma = fresh >= 0 ? gamma_fresh : sc[SC_GAMMA];
#pragma unroll
        for (int e = 0; e < E; ++e) q[e] *= gamma;
#pragma unroll
        for (int j = GOPS_MPC_MAX_HISTORY - 1; j >= 0; --j) {
            if (j < m) {
                const int k = (head + 2 * m - 1 - j) % m;
                double t = 0.0;
#pragma unroll
                for (int e = 0; e < E; ++e)
                    if (fr[e]) t += (double)ring_y(k)[lane + e * W] * q[e];
                t = sub_sum<W>(t);
                const double c = j < count ? a[j] - (k == fresh ? rho_fresh : sc[SC_RHO + k]) * t : 0.0;
#pragma unroll
                for (int e = 0; e < E; ++e)
                    if (fr[e]) q[e] += c * (double)ring_s(k)[lane + e * W];
            }
        }
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int i = lane + e * W;
            if (i < n) row(VE_D)[i] = (float)-q[e];
        }
    }

    // x_trial <- clamp(x + alpha d); returns dphi = g . (x_trial - x), the directional derivative along the projected step
    __device__ __forceinline__ double project(double alpha, float* out) const {
        double dphi = 0.0;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int i = lane + e * W;
            if (i < n) {
                const double x = (double)row(VE_X)[i];
                const float xt = (float)clampd(x + alpha * (double)row(VE_D)[i], (double)lo[i], (double)hi[i]);
                row(VE_X_TRIAL)[i] = xt, out[i] = xt;
                dphi += (double)row(VE_G)[i] * ((double)xt - x);
            }
        }
        return sub_sum<W>(dphi);
    }

    // The trial point of step length alpha along d.  A projected step that is no descent step (dphi >= 0) drops the ring and falls
    // back on the projected steepest descent, whose every term g_i (x_trial_i - x_i) is <= 0.
    __device__ __forceinline__ void trial(double alpha, int count, float* out) const {
        double dphi = project(alpha, out);
        if (dphi >= 0.0 && count > 0) {
            const double dn = steepest();
            alpha = dn > 1.0 ? 1.0 / dn : 1.0;
            dphi = project(alpha, out);
            if (lane == 0) ct[CT_COUNT] = 0;
        }
        if (lane == 0) sc[SC_ALPHA] = alpha, sc[SC_DPHI] = dphi;
    }
};

template <int W>
__device__ __forceinline__ bool mpc_problem(Problem<W>& p, void* state, int B, int n, int m, size_t& r) {
    r = (size_t)blockIdx.x * (MPC_THREADS / W) + threadIdx.x / W;
    if (r >= (size_t)B) return false;
    const MpcBlock b = mpc_sections(state, B, n, m);
    p.n = n, p.m = m, p.lane = threadIdx.x % W;
    p.sc = b.scalars + r * (GOPS_MPC_SCALARS + m), p.ct = b.counters + r * GOPS_MPC_COUNTERS;
    p.lo = b.lo, p.hi = b.hi, p.vec = b.vectors + r * (GOPS_MPC_VECTORS + 2 * m) * n;
    return true;
}

template <int W>
__global__ __launch_bounds__(MPC_THREADS) void mpc_init_kernel(void* state, int B, int n, int m, const float* __restrict__ x0,
                                                               const float* __restrict__ lo, const float* __restrict__ hi,
                                                               float* __restrict__ x_trial) {
    Problem<W> p;
    size_t r;
    if (!mpc_problem(p, state, B, n, m, r)) return;
    const MpcBlock b = mpc_sections(state, B, n, m);
#pragma unroll
    for (int e = 0; e < Problem<W>::E; ++e) {
        const int i = p.lane + e * W;
        if (i < n) {
            if (r == 0) b.lo[i] = lo[i], b.hi[i] = hi[i];
            const float x = (float)clampd((double)x0[r * n + i], (double)lo[i], (double)hi[i]);
            for (int v = 0; v < GOPS_MPC_VECTORS + 2 * m; ++v) p.row(v)[i] = 0.f;
            p.row(VE_X)[i] = x, p.row(VE_X_TRIAL)[i] = x, x_trial[r * n + i] = x;
        }
    }
    if (p.lane == 0) {
        for (int k = 0; k < GOPS_MPC_SCALARS + m; ++k) p.sc[k] = 0.0;
        p.sc[SC_GAMMA] = 1.0;
        for (int k = 0; k < GOPS_MPC_COUNTERS; ++k) p.ct[k] = 0;
    }
}

template <int W>
__global__ __launch_bounds__(MPC_THREADS) void mpc_step_kernel(void* state, int B, int n, int m, const float* __restrict__ f_in,
                                                               const float* __restrict__ g_in, float* __restrict__ x_trial,
                                                               const float* __restrict__ hyper) {
    constexpr int E = Problem<W>::E;
    Problem<W> p;
    size_t r;
    if (!mpc_problem(p, state, B, n, m, r)) return;
    float* out = x_trial + r * n;
    const float* gin = g_in + r * n;
    if (p.ct[CT_STATUS] != GOPS_MPC_RUNNING) {   // left untouched; its row of the shared rollout stays its accepted point
        p.copy_out(VE_X, out);
        return;
    }
    const int evals = p.ct[CT_EVAL];
    const bool first = evals == 0;   // f, g belong to the clamped x0: accepted without a test
    const float fin = f_in[r];
    double bad = isfinite(fin) ? 0.0 : 1.0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = p.lane + e * W;
        if (i < n && !isfinite(gin[i])) bad = 1.0;
    }
    if (sub_max<W>(bad) != 0.0) {
        if (p.lane == 0) p.ct[CT_STATUS] = GOPS_MPC_NONFINITE, p.ct[CT_EVAL] = evals + 1;
        p.copy_out(VE_X, out);
        return;
    }
    int count = p.ct[CT_COUNT], head = p.ct[CT_HEAD];
    const double f_acc = p.sc[SC_F];
    if (!first && !((double)fin <= f_acc + (double)hyper[HY_C1] * p.sc[SC_DPHI])) {   // Armijo fails: backtrack
        const int ls = p.ct[CT_LS] + 1;
        const bool spent = ls >= (int)hyper[HY_MAX_LS];
        const double alpha = p.sc[SC_ALPHA] * (double)hyper[HY_SHRINK];
        if (p.lane == 0) {
            p.ct[CT_EVAL] = evals + 1, p.ct[CT_LS] = ls;
            if (spent) p.ct[CT_STATUS] = GOPS_MPC_LINE_SEARCH;
        }
        if (spent)
            p.copy_out(VE_X, out);
        else
            p.trial(alpha, count, out);
        return;
    }
    // accepted: the pair, the move, the tests, the next direction
    int fresh = -1;
    double rho_fresh = 0.0, gamma_fresh = 1.0;
    if (!first) {
        float s[E], y[E];
        double sy = 0.0, yy = 0.0;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int i = p.lane + e * W;
            s[e] = y[e] = 0.f;
            if (i < n) {
                s[e] = (float)((double)p.row(VE_X_TRIAL)[i] - (double)p.row(VE_X)[i]);
                y[e] = (float)((double)gin[i] - (double)p.row(VE_G)[i]);
                sy += (double)s[e] * (double)y[e], yy += (double)y[e] * (double)y[e];
            }
        }
        sy = sub_sum<W>(sy), yy = sub_sum<W>(yy);
        if (sy > (double)hyper[HY_CURV_EPS] * yy) {   // scipy's L-BFGS-B skips the pair otherwise
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int i = p.lane + e * W;
                if (i < n) p.ring_s(head)[i] = s[e], p.ring_y(head)[i] = y[e];
            }
            fresh = head, rho_fresh = 1.0 / sy, gamma_fresh = sy / yy;
            if (p.lane == 0) p.sc[SC_RHO + head] = rho_fresh, p.sc[SC_GAMMA] = gamma_fresh;
            head = (head + 1) % m, count = count < m ? count + 1 : m;
        }
    }
    double pg = 0.0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = p.lane + e * W;
        if (i < n) {
            const float x = first ? p.row(VE_X)[i] : p.row(VE_X_TRIAL)[i], g = gin[i];
            p.row(VE_X_PREV)[i] = p.row(VE_X)[i], p.row(VE_G_PREV)[i] = p.row(VE_G)[i];
            p.row(VE_X)[i] = x, p.row(VE_G)[i] = g;
            pg = fmax(pg, fabs((double)x - clampd((double)x - (double)g, (double)p.lo[i], (double)p.hi[i])));
        }
    }
    pg = sub_max<W>(pg);
    int status = GOPS_MPC_RUNNING;
    if (pg <= (double)hyper[HY_PGTOL])
        status = GOPS_MPC_CONVERGED_PG;
    else if (!first && f_acc - (double)fin <= (double)hyper[HY_FTOL] * fmax(fmax(fabs(f_acc), fabs((double)fin)), 1.0))
        status = GOPS_MPC_CONVERGED_F;
    if (p.lane == 0) {
        p.sc[SC_F_PREV] = f_acc, p.sc[SC_F] = (double)fin;
        p.ct[CT_STATUS] = status, p.ct[CT_ITER] = p.ct[CT_ITER] + (first ? 0 : 1), p.ct[CT_EVAL] = evals + 1, p.ct[CT_LS] = 0;
        p.ct[CT_HEAD] = head, p.ct[CT_COUNT] = count;
    }
    if (status != GOPS_MPC_RUNNING) {
        p.copy_out(VE_X, out);
        return;
    }
    double alpha = 1.0;
    if (count > 0) {
        p.two_loop(head, count, fresh, rho_fresh, gamma_fresh);
    } else {
        const double dn = p.steepest();
        alpha = dn > 1.0 ? 1.0 / dn : 1.0;   // scipy's first step: min(1, 1 / |d|)
    }
    p.trial(alpha, count, out);
}

template <int W>
__global__ __launch_bounds__(MPC_THREADS) void mpc_finish_kernel(void* state, int B, int n, int m, float* __restrict__ x, float* __restrict__ f,
                                                                 int32_t* __restrict__ status, int32_t* __restrict__ iterations) {
    Problem<W> p;
    size_t r;
    if (!mpc_problem(p, state, B, n, m, r)) return;
    p.copy_out(VE_X, x + r * n);
    if (p.lane == 0) f[r] = (float)p.sc[SC_F], status[r] = p.ct[CT_STATUS], iterations[r] = p.ct[CT_ITER];
}

// The receding-horizon hand-over between two solves of a closed loop (gops_mpc_advance): per row what gops_mpc_finish, the shift of
// the plan by one control point and gops_mpc_init do one after the other.  x0[i] = x[i + A] below n - A and x[i] from there on (drop
// the first control point, repeat the last); every lane reads the elements it needs - its own and the ones A further, which other
// lanes of its wave own - and the row's scalars before any lane writes, so the result does not depend on the order of the lanes.
template <int W>
__global__ __launch_bounds__(MPC_THREADS) void mpc_advance_kernel(void* state, int B, int n, int m, int A, const float* __restrict__ frozen,
                                                                  float* __restrict__ action, int32_t* __restrict__ record,
                                                                  float* __restrict__ x_trial) {
    constexpr int E = Problem<W>::E;
    Problem<W> p;
    size_t r;
    if (!mpc_problem(p, state, B, n, m, r)) return;
    const bool fz = frozen[r] != 0.f;
    float own[E], next[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = p.lane + e * W;
        own[e] = next[e] = 0.f;
        if (i < n) {
            own[e] = p.row(VE_X)[i];
            next[e] = i + A < n ? p.row(VE_X)[i + A] : own[e];
        }
    }
    const int status = p.ct[CT_STATUS], iterations = p.ct[CT_ITER], evals = p.ct[CT_EVAL];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = p.lane + e * W;
        if (i < n) {
            if (i < A) action[r * A + i] = fz ? 0.f : own[e];
            const float x = (float)clampd((double)next[e], (double)p.lo[i], (double)p.hi[i]);
            for (int v = 0; v < GOPS_MPC_VECTORS + 2 * m; ++v) p.row(v)[i] = 0.f;
            p.row(VE_X)[i] = x, p.row(VE_X_TRIAL)[i] = x, x_trial[r * n + i] = x;
        }
    }
    if (p.lane == 0) {
        int32_t* rec = record + r * 4;
        rec[0] = fz ? GOPS_MPC_FROZEN : status;
        if (!fz) rec[1] += iterations, rec[2] += evals, rec[3] += 1;
        for (int k = 0; k < GOPS_MPC_SCALARS + m; ++k) p.sc[k] = 0.0;
        p.sc[SC_GAMMA] = 1.0;
        for (int k = 0; k < GOPS_MPC_COUNTERS; ++k) p.ct[k] = 0;
        if (fz) p.ct[CT_STATUS] = GOPS_MPC_FROZEN;
    }
}

// The outer step of the augmented Lagrangian (gops_mpc_al_update): it writes the solver block (the re-arm), so it sits here with the
// block's layout.  Term j = t n_c + k of row r: c[(t B + r) n_c + k], lambda[r J + j], J = H n_c; lane l of the row's sub-group
// owns the terms l, l + W, ..  Every lane reads the row's scalars before lane 0 writes them (one wave, program order).
enum { AH_RHO0, AH_GROWTH, AH_RHO_MAX, AH_SHRINK_TARGET, AH_CSTR_TOL, AH_MAX_OUTER, AH_LAMBDA_TOL };
enum { AO_STATUS, AO_ITER, AO_EVAL };
static_assert(AH_LAMBDA_TOL < GOPS_MPC_AL_HYPER_FLOATS && AO_EVAL < GOPS_MPC_AL_COUNTERS, "the tables of gops_mpc_al_update in gops_hip.h");

template <int W>
__global__ __launch_bounds__(MPC_THREADS) void mpc_al_update_kernel(void* state, int B, int n, int m, int H, int nc, const float* __restrict__ c,
                                                                    float* __restrict__ lambda, float* __restrict__ rho,
                                                                    const float* __restrict__ viol, float* __restrict__ viol_prev,
                                                                    int32_t* __restrict__ outer, const float* __restrict__ hyper) {
    Problem<W> p;
    size_t r;
    if (!mpc_problem(p, state, B, n, m, r)) return;
    const int inner = p.ct[CT_STATUS];
    int32_t* ao = outer + r * GOPS_MPC_AL_COUNTERS;
    if ((inner != GOPS_MPC_CONVERGED_PG && inner != GOPS_MPC_CONVERGED_F && inner != GOPS_MPC_LINE_SEARCH) || ao[AO_STATUS] != GOPS_MPC_AL_RUNNING)
        return;
    const int J = H * nc;
    const double rh = (double)rho[r], vio = (double)viol[r], vprev = (double)viol_prev[r];
    const int iters = ao[AO_ITER] + 1, evals = p.ct[CT_EVAL];
    double change = 0.0;
    for (int j = p.lane; j < J; j += W) {
        const int t = j / nc, k = j - t * nc;
        const float lam = lambda[r * J + j];
        const float ln = (float)fmax(0.0, (double)lam + rh * (double)c[((size_t)t * B + r) * nc + k]);
        change = fmax(change, fabs((double)ln - (double)lam));
        lambda[r * J + j] = ln;
    }
    change = sub_max<W>(change);
    if (p.lane != 0) return;
    if (!(vio <= (double)hyper[AH_SHRINK_TARGET] * vprev)) rho[r] = (float)fmin(rh * (double)hyper[AH_GROWTH], (double)hyper[AH_RHO_MAX]);
    viol_prev[r] = (float)vio;
    ao[AO_ITER] = iters;
    if (vio <= (double)hyper[AH_CSTR_TOL] && change <= (double)hyper[AH_LAMBDA_TOL] * rh) {
        ao[AO_STATUS] = GOPS_MPC_AL_CONVERGED;
    } else if (iters >= (int)hyper[AH_MAX_OUTER]) {
        ao[AO_STATUS] = GOPS_MPC_AL_MAX_OUTER;
    } else {   // re-arm: x stays; the pairs and f_prev belong to the old objective; evaluations = 0 makes the next step accept x untested
        ao[AO_EVAL] += evals;
        p.sc[SC_F_PREV] = 0.0;
        p.ct[CT_STATUS] = GOPS_MPC_RUNNING, p.ct[CT_EVAL] = 0, p.ct[CT_LS] = 0, p.ct[CT_HEAD] = 0, p.ct[CT_COUNT] = 0;
    }
}

// The multiplier side of the hand-over (gops_mpc_al_advance), launched behind mpc_advance_kernel: out of place, so no lane reads what
// another has written.  Frozen rows are copied.
template <int W>
__global__ __launch_bounds__(MPC_THREADS) void mpc_al_shift_kernel(int B, int n, int J, int S, const float* __restrict__ frozen,
                                                                   int32_t* __restrict__ record, const float* __restrict__ lambda_in,
                                                                   float* __restrict__ lambda_out, float* __restrict__ rho,
                                                                   float* __restrict__ viol_prev, int32_t* __restrict__ outer,
                                                                   const float* __restrict__ hyper) {
    const size_t r = (size_t)blockIdx.x * (MPC_THREADS / W) + threadIdx.x / W;
    if (r >= (size_t)B) return;
    const int lane = threadIdx.x % W;
    const bool fz = frozen[r] != 0.f;
    for (int j = lane; j < J; j += W) lambda_out[r * J + j] = fz ? lambda_in[r * J + j] : (j + S < J ? lambda_in[r * J + j + S] : 0.f);
    if (lane != 0 || fz) return;
    int32_t* ao = outer + r * GOPS_MPC_AL_COUNTERS;
    record[r * 4 + 2] += ao[AO_EVAL];   // the evaluations the re-arms took out of the block's counter
    for (int k = 0; k < GOPS_MPC_AL_COUNTERS; ++k) ao[k] = 0;
    rho[r] = hyper[AH_RHO0], viol_prev[r] = INFINITY;
}

int mpc_width(int n) { return n > 64 ? 64 : n > 32 ? 32 : n > 16 ? 16 : n > 8 ? 8 : 4; }

// calls f.template operator()<W>() for the sub-group width of n
template <typename F>
void mpc_dispatch(int n, F&& f) {
    switch (mpc_width(n)) {
        case 64: f.template operator()<64>(); break;
        case 32: f.template operator()<32>(); break;
        case 16: f.template operator()<16>(); break;
        case 8: f.template operator()<8>(); break;
        default: f.template operator()<4>(); break;
    }
}

dim3 mpc_grid(int B, int n) {
    const int per = MPC_THREADS / mpc_width(n);
    return dim3((unsigned)(((size_t)B + per - 1) / per));
}

// The checks every entry point makes on the block and the sizes, in this order; GOPS_OK when the call may launch.
int mpc_check(const void* state, size_t state_bytes, int B, int n, int m, bool ptrs) {
    if (!state || !ptrs || B < 1 || n < 1 || m < 1 || m > GOPS_MPC_MAX_HISTORY) return GOPS_ERR_BAD_ARG;
    if (reinterpret_cast<uintptr_t>(state) & 7) return GOPS_ERR_BAD_ARG;
    if (n > GOPS_MPC_MAX_DIM) return GOPS_ERR_UNSUPPORTED;
    if (state_bytes < mpc_bytes(B, n, m)) return GOPS_ERR_WORKSPACE;
    return GOPS_OK;
}

}  // namespace

extern "C" {

size_t gops_mpc_state_bytes(int32_t B, int32_t n, int32_t m) {
    if (B < 1 || n < 1 || n > GOPS_MPC_MAX_DIM || m < 1 || m > GOPS_MPC_MAX_HISTORY) return 0;
    return mpc_bytes(B, n, m);
}

int gops_mpc_init(void* state, size_t state_bytes, int32_t B, int32_t n, int32_t m, const float* x0, const float* lo, const float* hi,
                  float* x_trial, void* stream) {
    const int rc = mpc_check(state, state_bytes, B, n, m, x0 && lo && hi && x_trial);
    if (rc != GOPS_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    mpc_dispatch(n, [&]<int W>() { hipLaunchKernelGGL(mpc_init_kernel<W>, mpc_grid(B, n), dim3(MPC_THREADS), 0, s, state, B, n, m, x0, lo, hi, x_trial); });
    return (int)hipGetLastError();
}

int gops_mpc_step(void* state, size_t state_bytes, int32_t B, int32_t n, int32_t m, const float* f, const float* g, float* x_trial,
                  const float* hyper, void* stream) {
    const int rc = mpc_check(state, state_bytes, B, n, m, f && g && x_trial && hyper);
    if (rc != GOPS_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    mpc_dispatch(n, [&]<int W>() { hipLaunchKernelGGL(mpc_step_kernel<W>, mpc_grid(B, n), dim3(MPC_THREADS), 0, s, state, B, n, m, f, g, x_trial, hyper); });
    return (int)hipGetLastError();
}

int gops_mpc_finish(void* state, size_t state_bytes, int32_t B, int32_t n, int32_t m, float* x, float* f, int32_t* status,
                    int32_t* iterations, void* stream) {
    const int rc = mpc_check(state, state_bytes, B, n, m, x && f && status && iterations);
    if (rc != GOPS_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    mpc_dispatch(n, [&]<int W>() { hipLaunchKernelGGL(mpc_finish_kernel<W>, mpc_grid(B, n), dim3(MPC_THREADS), 0, s, state, B, n, m, x, f, status, iterations); });
    return (int)hipGetLastError();
}

int gops_mpc_advance(void* state, size_t state_bytes, int32_t B, int32_t n, int32_t m, int32_t act_dim, const float* frozen, float* action,
                     int32_t* record, float* x_trial, void* stream) {
    if (!state || !frozen || !action || !record || !x_trial || B < 1 || n < 1 || n > GOPS_MPC_MAX_DIM || m < 1 || m > GOPS_MPC_MAX_HISTORY ||
        act_dim < 1 || n % act_dim != 0 || (reinterpret_cast<uintptr_t>(state) & 7) || state_bytes != mpc_bytes(B, n, m))
        return GOPS_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    mpc_dispatch(n, [&]<int W>() {
        hipLaunchKernelGGL(mpc_advance_kernel<W>, mpc_grid(B, n), dim3(MPC_THREADS), 0, s, state, B, n, m, act_dim, frozen, action, record, x_trial);
    });
    return (int)hipGetLastError();
}

int gops_mpc_al_update(void* state, size_t state_bytes, int32_t B, int32_t n, int32_t m, int32_t H, int32_t n_c, const float* c, float* lambda,
                       float* rho, const float* viol, float* viol_prev, int32_t* outer, const float* al_hyper, void* stream) {
    if (!state || !c || !lambda || !rho || !viol || !viol_prev || !outer || !al_hyper || B < 1 || n < 1 || n > GOPS_MPC_MAX_DIM || m < 1 ||
        m > GOPS_MPC_MAX_HISTORY || H < 1 || H > GOPS_MPC_AL_MAX_H || n_c < 1 || n_c > GOPS_MAX_CONSTRAINT || (reinterpret_cast<uintptr_t>(state) & 7) ||
        state_bytes != mpc_bytes(B, n, m))
        return GOPS_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    mpc_dispatch(n, [&]<int W>() {
        hipLaunchKernelGGL(mpc_al_update_kernel<W>, mpc_grid(B, n), dim3(MPC_THREADS), 0, s, state, B, n, m, H, n_c, c, lambda, rho, viol, viol_prev,
                           outer, al_hyper);
    });
    return (int)hipGetLastError();
}

int gops_mpc_al_advance(void* state, size_t state_bytes, int32_t B, int32_t n, int32_t m, int32_t act_dim, const float* frozen, float* action,
                        int32_t* record, float* x_trial, int32_t H, int32_t n_c, int32_t shift, const float* lambda_in, float* lambda_out,
                        float* rho, float* viol_prev, int32_t* outer, const float* al_hyper, void* stream) {
    if (!lambda_in || !lambda_out || lambda_in == lambda_out || !rho || !viol_prev || !outer || !al_hyper || H < 1 || H > GOPS_MPC_AL_MAX_H || n_c < 1 ||
        n_c > GOPS_MAX_CONSTRAINT || shift < 1)
        return GOPS_ERR_BAD_ARG;
    const int rc = gops_mpc_advance(state, state_bytes, B, n, m, act_dim, frozen, action, record, x_trial, stream);
    if (rc != GOPS_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int J = H * n_c, S = shift < H ? shift * n_c : J;
    mpc_dispatch(n, [&]<int W>() {
        hipLaunchKernelGGL(mpc_al_shift_kernel<W>, mpc_grid(B, n), dim3(MPC_THREADS), 0, s, B, n, J, S, frozen, record, lambda_in, lambda_out, rho,
                           viol_prev, outer, al_hyper);
    });
    return (int)hipGetLastError();
}

}  // extern "C"
