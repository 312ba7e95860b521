// Small kernels beside the rollout: the any-width output layer of gops_mlp_*, the zero fill, and the single-step env-model and
// constraint entry points.
#include <algorithm>
#include "common.h"
#include "env_models.h"
#include "env_step.h"
#include "launchers.h"

// ---------------------------------------------------------------------------------------------
// Output layer of ANY width W (gops_mlp_forward / _backward: FiniteHorizonFullPolicy emits act_dim * pre_horizon
// values): y = h Wo^T + b over the stashed last hidden activation h [S][K] (tile-major rows == batch rows for H = 1),
// and its input adjoint g_h = g_y Wo together with a zero-padded copy g_yp [S][Wp] of g_y that the regular dW GEMM
// takes as its delta operand.  63 MFLOP at B = 4096, W = 60: plain VALU, 16 rows per block staged in LDS.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void linear_out_fwd_kernel(const float* __restrict__ h, int K, const float* __restrict__ Wo,
                                                             const float* __restrict__ bo, int W, int B, float* __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) float hs[];   // [16][K + 4] row-major copy of the FM tile
    const int b0 = blockIdx.x * 16, rows = min(16, B - b0), ld = K + 4;
    for (int i = threadIdx.x; i < 4 * K; i += 256) {   // 16-byte unit i of the tile: feature i >> 2, rows 4 (i & 3) .. +3
        const f32x4 v = reinterpret_cast<const f32x4*>(h + (size_t)blockIdx.x * 16 * K)[i];
        const int k = i >> 2, m0 = (i & 3) << 2;
#pragma unroll
        for (int r = 0; r < 4; ++r) hs[(m0 + r) * ld + k] = v[r];
    }
    __syncthreads();
    for (int o = threadIdx.x; o < 16 * W; o += 256) {   // o = m * W + w: consecutive threads -> consecutive y elements
        const int m = o / W, w = o - m * W;
        if (m >= rows) continue;
        const f32x4* wr = reinterpret_cast<const f32x4*>(Wo + (size_t)w * K);
        const f32x4* hr = reinterpret_cast<const f32x4*>(hs + m * ld);
        float acc = 0.f;
        for (int c = 0; c < (K >> 2); ++c) {
            const f32x4 a = hr[c], bq = wr[c];
            acc += a[0] * bq[0] + a[1] * bq[1] + a[2] * bq[2] + a[3] * bq[3];
        }
        y[(size_t)(b0 + m) * W + w] = acc + bo[w];
    }
}

// g_h stays row-major [S][K] (rollout_bwd reads it as `ext_delta`); g_yp is the FM delta operand [S/16][Wp][16]
// The 16 rows of g_y are staged LOB_WC columns at a time (64 KiB, the dynamic LDS a launch gets without asking): an output layer
// of up to LOB_WC padded columns takes one pass - [16][Wp], as before - and a wider one (plan_mlp admits W <= 4096) continues
// each g_h sum from the value the pass before stored, i.e. in the same order as one long loop (one more read and write of g_h per
// pass, which has not been timed).
constexpr int LOB_WC = 1024;
__global__ __launch_bounds__(256) void linear_out_bwd_kernel(const float* __restrict__ gy, int W, int Wp, const float* __restrict__ Wo,
                                                             int K, int B, long long S, float* __restrict__ gh, float* __restrict__ gyp) {
    extern __shared__ __attribute__((aligned(16))) float gs[];   // [16][min(Wp, LOB_WC)]
    const long long s0 = (long long)blockIdx.x * 16;
    for (int w0 = 0; w0 < Wp; w0 += LOB_WC) {
        const int wc = min(LOB_WC, Wp - w0), wlive = min(wc, W - w0);   // staged columns (a multiple of 16) / those that exist
        if (w0 > 0) __syncthreads();
        for (int i = threadIdx.x; i < 16 * wc; i += 256) {
            const int m = i / wc, w = i - m * wc;
            gs[i] = (s0 + m < B && w0 + w < W) ? gy[(size_t)(s0 + m) * W + w0 + w] : 0.f;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < 16 * wc; i += 256) {   // i = w * 16 + m: the FM tile in memory order
            const int w = i >> 4, m = i & 15;
            gyp[(size_t)blockIdx.x * 16 * Wp + (size_t)w0 * 16 + i] = gs[m * wc + w];
        }
        for (int o = threadIdx.x; o < 16 * K; o += 256) {   // o = m * K + k: coalesced reads of Wo rows and writes of g_h
            const int m = o / K, k = o - m * K;
            if (s0 + m >= S) continue;
            float acc = w0 > 0 ? gh[(size_t)(s0 + m) * K + k] : 0.f;
            for (int w = 0; w < wlive; ++w) acc += gs[m * wc + w] * Wo[(size_t)(w0 + w) * K + k];
            gh[(size_t)(s0 + m) * K + k] = acc;
        }
    }
}

hipError_t launch_linear_out_fwd(const float* h, int K, const float* Wo, const float* bo, int W, int B, float* y, hipStream_t s) {
    hipLaunchKernelGGL(linear_out_fwd_kernel, dim3((B + 15) / 16), dim3(256), 16 * (K + 4) * sizeof(float), s, h, K, Wo, bo, W, B, y);
    return hipGetLastError();
}

hipError_t launch_linear_out_bwd(const float* gy, int W, int Wp, const float* Wo, int K, int B, long long S, float* gh,
                                 float* gyp, hipStream_t s) {
    hipLaunchKernelGGL(linear_out_bwd_kernel, dim3((unsigned)((S + 15) / 16)), dim3(256), 16 * (size_t)std::min(Wp, LOB_WC) * sizeof(float), s, gy, W, Wp, Wo,
                       K, B, S, gh, gyp);
    return hipGetLastError();
}

// Zero fill as a KERNEL on the caller's stream: inside a captured HIP graph a hipMemsetAsync becomes a memset node,
// which was measured to race with the neighbouring kernel nodes on replay (non-reproducible gradients); a kernel node
// is ordered like every other launch.
__global__ __launch_bounds__(256) void fill_zero_kernel(f32x4* __restrict__ p4, size_t n4, float* __restrict__ tail, int ntail) {
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) p4[i] = z;
    if (blockIdx.x == 0 && (int)threadIdx.x < ntail) tail[threadIdx.x] = 0.f;
}

hipError_t launch_fill_zero(float* p, size_t n, hipStream_t s) {   // p is 16-byte aligned (workspace carving)
    if (n == 0) return hipSuccess;
    const size_t n4 = n >> 2;
    const unsigned blocks = (unsigned)std::min<size_t>(2048, std::max<size_t>(1, (n4 + 255) / 256));
    hipLaunchKernelGGL(fill_zero_kernel, dim3(blocks), dim3(256), 0, s, reinterpret_cast<f32x4*>(p), n4, p + (n4 << 2), (int)(n & 3));
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Single wrapped env-model step (pyth_base_model.py:59-67 contract), one thread per trajectory: env_step.h
// ---------------------------------------------------------------------------------------------
__global__ void env_step_kernel(const GopsEnv env, int B, const GopsStepIO io, float pdt) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    env_step_one(env, b, io, pdt);
}

// model.get_constraint(obs, info), one thread per row (gops_env_constraint)
__global__ void env_constraint_kernel(const GopsEnv env, int B, const GopsStepIO io) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int nc = env.n_constraint;
    if (env.cstr_err) {
        const float* ob = io.obs + (size_t)b * env.obs_dim;
        if (env.kind == GOPS_ENV_VEH2DOF) {
            io.constraint[b] = fabsf(ob[0]) - env.err_tol[0];
        } else {
            io.constraint[(size_t)b * 2 + 0] = fabsf(ob[1]) - env.err_tol[0];
            io.constraint[(size_t)b * 2 + 1] = fabsf(ob[3]) - env.err_tol[1];
        }
        return;
    }
    const float* st = io.state + (size_t)b * 6;
    f32x4 pts[GOPS_MAX_SURR];
    for (int i = 0; i < GOPS_MAX_SURR; ++i) {
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        pts[i] = z;
        if (i < env.n_surr) {
            const float* sv = io.surr_state + ((size_t)b * env.n_surr + i) * 5;
            pts[i][0] = sv[0]; pts[i][1] = sv[1]; pts[i][2] = sv[2]; pts[i][3] = sv[3];
        }
    }
    float sp, cp;
    sincosf(st[2], &sp, &cp);
    SurrCstr sc;
    surr_constraint<false>(env, st[0], st[1], sp, cp, pts, sc);
    for (int k = 0; k < nc; ++k) io.constraint[(size_t)b * nc + k] = sc.c[k];
}

extern "C" {

int gops_env_constraint(const GopsEnv* env, int32_t B, const GopsStepIO* io, void* stream) {
    if (!env || !io || B < 1 || !io->constraint) return GOPS_ERR_BAD_ARG;
    const bool err = env->cstr_err != 0 && (env->kind == GOPS_ENV_VEH3DOF_SURR || env->kind == GOPS_ENV_VEH2DOF);
    const bool surr = env->kind == GOPS_ENV_VEH3DOF_SURR && !env->cstr_err;
    if (!err && !surr) return GOPS_ERR_UNSUPPORTED;   // the model defines no get_constraint
    if (err && (!io->obs || env->n_constraint != (env->kind == GOPS_ENV_VEH2DOF ? 1 : 2))) return GOPS_ERR_BAD_ARG;
    if (surr && (!io->state || !io->surr_state || env->n_surr < 1 || env->n_surr > GOPS_MAX_SURR ||
                 (env->n_constraint != 1 && env->n_constraint != 3))) return GOPS_ERR_BAD_ARG;
    hipLaunchKernelGGL(env_constraint_kernel, dim3((B + 127) / 128), dim3(128), 0, static_cast<hipStream_t>(stream), *env, B, *io);
    return (int)hipGetLastError();
}

int gops_env_step(const GopsEnv* env, int32_t B, const GopsStepIO* io, void* stream) {
    if (!env || !io || B < 1) return GOPS_ERR_BAD_ARG;
    if (env->kind < GOPS_ENV_LQ || env->kind > GOPS_ENV_MOUNTAINCAR) return GOPS_ERR_BAD_ARG;
    if (env->kind == GOPS_ENV_MOBILEROBOT &&
        (env->obs_dim != MOB_OBS || env->act_dim != 2 || env->n_constraint != 1 || env->scale_obs || !io->constraint)) return GOPS_ERR_BAD_ARG;
    if (env->kind == GOPS_ENV_MOUNTAINCAR && mcar_check_env(*env) != GOPS_OK) return GOPS_ERR_BAD_ARG;
    if (env->data_env && (env->kind == GOPS_ENV_PENDULUM || env->kind == GOPS_ENV_MOUNTAINCAR || (env->kind == GOPS_ENV_VEH2DOF && env->cstr_err)))
        return GOPS_ERR_UNSUPPORTED;   // these data envs are not restated
    if (!io->obs || !io->action || !io->next_obs || !io->reward || !io->next_done) return GOPS_ERR_BAD_ARG;
    if (env->kind == GOPS_ENV_VEH3DOF_SURR &&
        (env->data_env || env->n_surr < (env->cstr_err ? 0 : 1) || env->n_surr > (env->cstr_err ? 0 : GOPS_MAX_SURR) ||
         (env->cstr_err ? env->n_constraint != 2 : (env->n_constraint != 1 && env->n_constraint != 3)) ||
         (env->n_surr > 0 && (!io->surr_state || !io->next_surr_state)) || !io->constraint)) return GOPS_ERR_BAD_ARG;
    if (env_has_ref_table(env->kind) &&
        (!io->state || !io->ref_points || !io->path_num || !io->u_num || !io->ref_time ||
         !io->next_state || !io->next_ref_points || !io->next_ref_time)) return GOPS_ERR_BAD_ARG;
    if (env->kind == GOPS_ENV_LQ && env->obs_dim > GOPS_MAX_LQ_STATE) return GOPS_ERR_UNSUPPORTED;
    if (env->scale_obs && env->kind != GOPS_ENV_LQ && env->kind != GOPS_ENV_IDPENDULUM && env->kind < GOPS_ENV_CARTPOLE) return GOPS_ERR_UNSUPPORTED;
    if (env->repeat_num < 0 || env->repeat_num > GOPS_MAX_REPEAT) return GOPS_ERR_BAD_ARG;
    if (env->repeat_num > 1 && (env->data_env || (env->kind != GOPS_ENV_LQ && env->kind != GOPS_ENV_IDPENDULUM &&
                                                  env->kind != GOPS_ENV_CARTPOLE && env->kind != GOPS_ENV_PENDULUM &&
                                                  env->kind != GOPS_ENV_MOUNTAINCAR)))
        return GOPS_ERR_UNSUPPORTED;
    GopsEnv e = *env;   // the library's own copy: reference constants filled, LQ matrices padded
    fill_ref_defaults(e);
    lq_pad_env(e);
    hipLaunchKernelGGL(env_step_kernel, dim3((B + 127) / 128), dim3(128), 0, static_cast<hipStream_t>(stream), e, B, *io, pdt_of(e));
    return (int)hipGetLastError();
}

}  // extern "C"
