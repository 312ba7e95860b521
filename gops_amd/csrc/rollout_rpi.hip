// RPI (relaxed policy iteration, gops/algorithm/rpi.py): the whole policy evaluation of one local_update in ONE launch.
//
// The reference performs up to max_step_update_value gradient steps per Newton iteration, each on a batch of B states with 3 .. 10
// weights: an env step, two autograd passes, an Adam step, a second Hamiltonian on a held-out set and a host-side test.  Here one
// workgroup runs that chain: one lane per batch row (B <= 1024), the weights, Adam moments and the lane's state in registers, two
// batch-wide reductions per step.  More workgroups would only add grid syncs to a chain this short.
//
// Reductions have a fixed order - butterfly inside each wave, then the waves in index order through LDS, summed by EVERY thread
// (wave_sum of common.h, as rollout_poly.hip) - so every thread holds the same sums bit for bit, takes the same Adam step in its own
// registers and reaches the same continue/stop decision: no barrier sits under divergent control flow, no float atomics, results
// are reproducible run to run.  The trip count is bounded by max_steps, never by convergence alone.
//
// Per step (rpi.py:183-197, sample() :289-327): action and adversary from the TARGET weights at the lane's state, the bare Euler
// step with the raw values, done / time-limit flags, the Hamiltonian h = U(x, u', w') + dV/dx . f(x, u', w') at the PRE-step state
// with the wrapped values (ScaleAction / ClipAction, create_env_model's chain) and the CURRENT weights, loss mean|h|, gradient
// mean sign(h) d(dV/dx . f)/dw (sign(0) = 0; the bias has none), Adam, the held-out mean|h| with the new weights, the reset select.
#include "common.h"
#include "rpi_env.h"

namespace {

constexpr int RPI_MAX_F = 10;
constexpr int RPI_MAX_WAVES = GOPS_RPI_MAX_BATCH / 64;

struct RpiParams {
    float c[GOPS_RPI_CONST_COUNT];
    int B, max_steps;
    float* w;                // [F] value weights, stepped in place
    const float* wt;         // [F] target weights
    const float* max_step;   // [B] time limit of each lane
    const float* pool;       // [max_steps + 1][S][B]: held-out set, then one reset draw per step
    float* state;            // the state block (gops_hip.h)
    float* result;           // [4]
    float* trace;            // [max_steps][2] or nullptr
    double lr, beta1, beta2, eps;
};

// dV/dx of V = sum_{i<=j} w_ij y_i y_j, y = x * norm (apprfunc/poly.py StateValue, degree 2)
template <int S>
__device__ __forceinline__ void rpi_grad_v(const float* w, const float* norm, const float* x, float* dv) {
    float y[S];
#pragma unroll
    for (int m = 0; m < S; ++m) { y[m] = x[m] * norm[m]; dv[m] = 0.f; }
    int k = 0;
#pragma unroll
    for (int i = 0; i < S; ++i)
#pragma unroll
        for (int j = i; j < S; ++j, ++k) { dv[i] += w[k] * y[j]; dv[j] += w[k] * y[i]; }
#pragma unroll
    for (int m = 0; m < S; ++m) dv[m] *= norm[m];
}

// raw action / adversary from the weights `w` at x, and their wrapped values
template <int KIND, int S>
__device__ __forceinline__ void rpi_policy(const float* c, const float* w, const float* x, float& u, float& a, float& uw, float& aw) {
    float dv[S];
    rpi_grad_v<S>(w, c + GOPS_RPI_C_NORM, x, dv);
    rpi_pair<KIND>(c, x, dv, u, a, uw, aw);
}

template <int KIND>
__global__ __launch_bounds__(GOPS_RPI_MAX_BATCH) void rpi_evaluate_kernel(const RpiParams p) {
    constexpr int S = rpi_state_dim(KIND);
    constexpr int F = S * (S + 1) / 2;
    static_assert(F <= RPI_MAX_F, "feature count");
    __shared__ float red1[RPI_MAX_WAVES * (F + 1)];
    __shared__ float red2[RPI_MAX_WAVES];
    const float* c = p.c;
    const float* norm = c + GOPS_RPI_C_NORM;
    const int b = threadIdx.x, B = p.B;
    const bool valid = b < B;
    const int nwaves = (int)(blockDim.x >> 6);
    const float invB_den = (float)B;
    float* hdr = p.state;
    float* st_x = p.state + GOPS_RPI_STATE_HEADER;
    float* st_cnt = st_x + (size_t)S * B;
    float* st_shown = st_cnt + B;

    float w[F], wt[F], am[F], av[F];
#pragma unroll
    for (int k = 0; k < F; ++k) { w[k] = p.w[k]; wt[k] = p.wt[k]; am[k] = hdr[k]; av[k] = hdr[RPI_MAX_F + k]; }
    // The Adam step count and the lanes' counters are floats in the state block: exact up to 2^24, where they stop advancing.  By
    // then beta1^t and beta2^t are 0 in double (0.99^t < 1e-300 from t = 68 732), so the bias corrections are exactly 1 either way,
    // and a lane's counter has long passed any time limit (max_step < 2^24), so its test stays true.
    float tcount = hdr[2 * RPI_MAX_F];
    RpiAdam adam(p.lr, p.beta1, p.beta2, p.eps, tcount);

    float x[S], xs[S], ds[S], Us = 0.f, cnt = 0.f, shown = -1.f, maxs = 0.f;
#pragma unroll
    for (int m = 0; m < S; ++m) { x[m] = 0.f; xs[m] = 0.f; ds[m] = 0.f; }
    if (valid) {
#pragma unroll
        for (int m = 0; m < S; ++m) { x[m] = st_x[(size_t)m * B + b]; xs[m] = p.pool[(size_t)m * B + b]; }
        cnt = st_cnt[b], shown = st_shown[b], maxs = p.max_step[b];
        // held-out set: the target's wrapped action pair is the same at every step, and with it U and f
        float u, a, uw, aw;
        rpi_policy<KIND, S>(c, wt, xs, u, a, uw, aw);
        rpi_derivative<KIND>(c, xs, uw, aw, ds);
        Us = rpi_cost<S>(c, xs, uw, aw);
    }
    auto heldout = [&]() {
        float dv[S], h = Us;
        rpi_grad_v<S>(w, norm, xs, dv);
#pragma unroll
        for (int m = 0; m < S; ++m) h += dv[m] * ds[m];
        return valid ? fabsf(h) : 0.f;
    };
    wave_sum(heldout(), red2, 0, 1);
    __syncthreads();
    const float before = rpi_block_sum(red2, 0, 1, nwaves) / invB_den;
    float after = before, loss = 0.f;
    int steps = 0;

#pragma unroll 1
    for (int i = 0; i < p.max_steps; ++i) {
        // sample(): target policy, bare step with the raw pair, flags
        float u, a, uw, aw, d[S], xn[S];
        rpi_policy<KIND, S>(c, wt, x, u, a, uw, aw);
        rpi_derivative<KIND>(c, x, u, a, d);
        bool reset = false;
#pragma unroll
        for (int m = 0; m < S; ++m) {
            xn[m] = x[m] + d[m] * c[GOPS_RPI_C_DT];
            reset = reset || fabsf(xn[m]) > c[GOPS_RPI_C_THRESHOLD + m];
        }
        cnt += 1.f;
        reset = reset || cnt > maxs;
        // Hamiltonian at the pre-step state: wrapped pair, current weights
        float dv[S], y[S];
        rpi_derivative<KIND>(c, x, uw, aw, d);
        rpi_grad_v<S>(w, norm, x, dv);
        float h = rpi_cost<S>(c, x, uw, aw);
#pragma unroll
        for (int m = 0; m < S; ++m) { h += dv[m] * d[m]; y[m] = x[m] * norm[m]; }
        const float sg = !valid ? 0.f : h > 0.f ? 1.f : h < 0.f ? -1.f : 0.f;
        wave_sum(valid ? fabsf(h) : 0.f, red1, F, F + 1);
        {
            int k = 0;
#pragma unroll
            for (int ii = 0; ii < S; ++ii)
#pragma unroll
                for (int jj = ii; jj < S; ++jj, ++k)
                    wave_sum(sg * ((norm[ii] * d[ii]) * y[jj] + (norm[jj] * d[jj]) * y[ii]), red1, k, F + 1);
        }
        __syncthreads();
        loss = rpi_block_sum(red1, F, F + 1, nwaves) / invB_den;
        tcount += 1.f;
        adam.advance();
#pragma unroll
        for (int k = 0; k < F; ++k) adam.update(w[k], am[k], av[k], rpi_block_sum(red1, k, F + 1, nwaves) / invB_den);
        // held-out norm with the new weights
        wave_sum(heldout(), red2, 0, 1);
        __syncthreads();
        after = rpi_block_sum(red2, 0, 1, nwaves) / invB_den;
        // reset select (rpi.py:315-325): this step's draw for lanes that ended
        if (valid) {
            const float prev = shown < 0.f ? cnt : shown;   // the first assignment reads the counter the step has just advanced
            shown = reset ? 0.f : prev;
#pragma unroll
            for (int m = 0; m < S; ++m) x[m] = reset ? p.pool[((size_t)(i + 1) * S + m) * B + b] : xn[m];
        }
        steps = i + 1;
        if (p.trace != nullptr && b == 0) { p.trace[2 * (size_t)i] = loss; p.trace[2 * (size_t)i + 1] = after; }
        // continue_evaluation (rpi.py:164-168): the same sums in every thread, so the branch is uniform
        if (!(fabs((double)after) > 0.88 * fabs((double)before))) break;
    }

    if (valid) {
#pragma unroll
        for (int m = 0; m < S; ++m) st_x[(size_t)m * B + b] = x[m];
        st_cnt[b] = cnt, st_shown[b] = shown;
    }
    if (b == 0) {
#pragma unroll
        for (int k = 0; k < F; ++k) { p.w[k] = w[k]; hdr[k] = am[k]; hdr[RPI_MAX_F + k] = av[k]; }
        hdr[2 * RPI_MAX_F] = tcount;
        p.result[0] = (float)steps, p.result[1] = loss, p.result[2] = before, p.result[3] = after;
    }
}

}  // namespace

extern "C" {

size_t gops_rpi_state_bytes(int32_t kind, int32_t B) {
    const int S = rpi_state_dim(kind);
    if (S == 0 || B < 1 || B > GOPS_RPI_MAX_BATCH) return 0;
    return sizeof(float) * ((size_t)GOPS_RPI_STATE_HEADER + (size_t)(S + 2) * B);
}

int gops_rpi_evaluate(int32_t kind, int32_t B, int32_t max_steps, const float* consts, float* w, const float* wt, const float* max_step,
                      const float* pool, void* state, size_t state_bytes, double lr, double beta1, double beta2, double eps, float* result,
                      float* trace, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (rpi_state_dim(kind) == 0 || B > GOPS_RPI_MAX_BATCH) return GOPS_ERR_UNSUPPORTED;
    if (B < 1 || max_steps < 1 || max_steps > GOPS_RPI_MAX_STEPS) return GOPS_ERR_BAD_ARG;
    if (!consts || !w || !wt || !max_step || !pool || !state || !result) return GOPS_ERR_BAD_ARG;
    if (state_bytes < gops_rpi_state_bytes(kind, B)) return GOPS_ERR_WORKSPACE;
    RpiParams p;
    for (int i = 0; i < GOPS_RPI_CONST_COUNT; ++i) p.c[i] = consts[i];
    p.B = B, p.max_steps = max_steps, p.w = w, p.wt = wt, p.max_step = max_step, p.pool = pool;
    p.state = static_cast<float*>(state), p.result = result, p.trace = trace;
    p.lr = lr, p.beta1 = beta1, p.beta2 = beta2, p.eps = eps;
    const dim3 block((unsigned)((B + 63) / 64 * 64));
    if (kind == GOPS_RPI_ENV_OSCILLATOR) rpi_evaluate_kernel<GOPS_RPI_ENV_OSCILLATOR><<<1, block, 0, s>>>(p);
    else if (kind == GOPS_RPI_ENV_AIRCRAFT) rpi_evaluate_kernel<GOPS_RPI_ENV_AIRCRAFT><<<1, block, 0, s>>>(p);
    else rpi_evaluate_kernel<GOPS_RPI_ENV_SUSPENSION><<<1, block, 0, s>>>(p);
    return (int)hipGetLastError();
}

}  // extern "C"
