// Env arithmetic and block sums shared by RPI's two single-launch policy-evaluation kernels (rollout_rpi.hip: POLY value,
// rollout_rpi_mlp.hip: MLP value): the three zero-sum game models in the host models' order of operations, the wrapper chain, the
// utility, the Adam step, and the fixed-order block sum.
#pragma once
#include "common.h"

constexpr int rpi_state_dim(int kind) {
    return kind == GOPS_RPI_ENV_OSCILLATOR ? 2 : kind == GOPS_RPI_ENV_AIRCRAFT ? 3 : kind == GOPS_RPI_ENV_SUSPENSION ? 4 : 0;
}

// dx/dt at x under action u and adversary w, in the order of operations of the host models (env/env_ocp/env_model/pyth_*conti_model.py)
template <int KIND>
__device__ __forceinline__ void rpi_derivative(const float* c, const float* x, float u, float w, float* d) {
    if constexpr (KIND == GOPS_RPI_ENV_OSCILLATOR) {
        const float ga = c[GOPS_RPI_C_GAMMA_ATTE];
        const float a = x[0], b = x[1];
        d[0] = -0.25f * a;
        d[1] = 0.5f * ((a * a) * b) - (1.f / (2.f * (ga * ga))) * (b * b * b) - 0.5f * b + a * u + b * w;
    } else if constexpr (KIND == GOPS_RPI_ENV_AIRCRAFT) {
        d[0] = (-1.01887f * x[0] + 0.90506f * x[1] + -0.00215f * x[2]) + w;
        d[1] = 0.82225f * x[0] + -1.07741f * x[1] + -0.17555f * x[2];
        d[2] = -x[2] + u;
    } else {
        constexpr float M_b = 300.f, M_us = 60.f, K_t = 190000.f, K_a = 16000.f, K_n = 1600.f, C_a = 1000.f, gain = 1000.f;
        const float dp = x[0] - x[2], dvel = x[1] - x[3];
        const float spring = K_a * dp + K_n * (dp * dp * dp) + C_a * dvel;
        d[0] = x[1];
        d[1] = -(spring - gain * u) / M_b;
        d[2] = x[3];
        d[3] = (spring - K_t * (x[2] - w) - gain * u) / M_us;
    }
}

// g(x)' dv and k(x)' dv (one action column, one adversary column)
template <int KIND>
__device__ __forceinline__ void rpi_gk_dot(const float* x, const float* dv, float& gdv, float& kdv) {
    if constexpr (KIND == GOPS_RPI_ENV_OSCILLATOR) {
        gdv = x[0] * dv[1];
        kdv = x[1] * dv[1];
    } else if constexpr (KIND == GOPS_RPI_ENV_AIRCRAFT) {
        gdv = dv[2];
        kdv = dv[0];
    } else {
        gdv = (1000.f / 300.f) * dv[1] + (-1000.f / 60.f) * dv[3];
        kdv = (190000.f / 60.f) * dv[3];
    }
}

// ScaleAction from [lo_s, hi_s] onto [lo, hi], then ClipAction (wrapper/scale_action.py:75-83, clip_action.py:34-36)
__device__ __forceinline__ float rpi_wrap(const float* c, float a, float lo_s, float hi_s, float lo, float hi) {
    if (c[GOPS_RPI_C_ACTION_SCALE] != 0.f) {
        a = fminf(fmaxf(a, lo_s), hi_s);
        a = lo + (hi - lo) * ((a - lo_s) / (hi_s - lo_s));
        a = fminf(fmaxf(a, lo), hi);
    }
    if (c[GOPS_RPI_C_CLIP_ACTION] != 0.f) a = fminf(fmaxf(a, lo), hi);
    return a;
}

// raw action / adversary from dV/dx = `dv` at x, and their wrapped values
template <int KIND>
__device__ __forceinline__ void rpi_pair(const float* c, const float* x, const float* dv, float& u, float& a, float& uw, float& aw) {
    float gdv, kdv;
    rpi_gk_dot<KIND>(x, dv, gdv, kdv);
    const float ga = c[GOPS_RPI_C_GAMMA_ATTE];
    u = -0.5f * (1.f / c[GOPS_RPI_C_R]) * gdv;
    a = 0.5f / (ga * ga) * kdv;
    uw = rpi_wrap(c, u, c[GOPS_RPI_C_SCALE_ACT_LOW], c[GOPS_RPI_C_SCALE_ACT_HIGH], c[GOPS_RPI_C_ACT_LOW], c[GOPS_RPI_C_ACT_HIGH]);
    aw = rpi_wrap(c, a, c[GOPS_RPI_C_SCALE_ADV_LOW], c[GOPS_RPI_C_SCALE_ADV_HIGH], c[GOPS_RPI_C_ADV_LOW], c[GOPS_RPI_C_ADV_HIGH]);
}

template <int S>
__device__ __forceinline__ float rpi_cost(const float* c, const float* x, float u, float a) {
    float cost = c[GOPS_RPI_C_Q] * (x[0] * x[0]);
#pragma unroll
    for (int m = 1; m < S; ++m) cost += c[GOPS_RPI_C_Q + m] * (x[m] * x[m]);
    const float ga = c[GOPS_RPI_C_GAMMA_ATTE];
    return cost + c[GOPS_RPI_C_R] * (u * u) - (ga * ga) * (a * a);
}

// torch.optim.Adam, single-tensor form, as both evaluation kernels step it: the bias corrections in double as the host computes
// them, the element update in fp32.  `tcount`: the steps taken so far.
struct RpiAdam {
    float lerp_w, beta2f, omb2, epsf, step_size, bc2s;
    double lr, beta1, beta2, b1p, b2p;
    __device__ __forceinline__ RpiAdam(double lr_, double beta1_, double beta2_, double eps, float tcount)
        : lerp_w((float)(1.0 - beta1_)), beta2f((float)beta2_), omb2((float)(1.0 - beta2_)), epsf((float)eps), step_size(0.f), bc2s(0.f),
          lr(lr_), beta1(beta1_), beta2(beta2_), b1p(pow(beta1_, (double)tcount)), b2p(pow(beta2_, (double)tcount)) {}
    // the next step's size and second-moment correction
    __device__ __forceinline__ void advance() {
        b1p *= beta1;
        b2p *= beta2;
        step_size = (float)(lr / (1.0 - b1p));
        bc2s = (float)sqrt(1.0 - b2p);
    }
    __device__ __forceinline__ void update(float& w, float& m, float& v, float g) const {
        m = m + lerp_w * (g - m);
        v = v * beta2f + omb2 * (g * g);
        const float denom = sqrtf(v) / bc2s + epsf;
        w = w - step_size * (m / denom);
    }
};

// after the barrier that follows wave_sum (common.h): the waves' sums in index order, the same value in every thread
__device__ __forceinline__ float rpi_block_sum(const float* red, int slot, int nslots, int nwaves) {
    float s = red[slot];
    for (int wv = 1; wv < nwaves; ++wv) s += red[wv * nslots + slot];
    return s;
}

