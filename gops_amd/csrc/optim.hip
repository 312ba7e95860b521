// The stand-alone optimizer and loss launches: Adam over a table of tensors, Polyak averaging of a target network, and the
// loss scalars of a batch.
#include <algorithm>
#include "common.h"
#include "block_reduce.h"
#include "launchers.h"

// ---------------------------------------------------------------------------------------------
// Adam over a table of tensors, one launch.  Same update as torch.optim.Adam (foreach path):
//   m = lerp(m, g, 1-b1); v = b2 v + (1-b2) g^2; p -= (lr / (1-b1^t)) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
// lr and the step count are read from device memory (graph-replayable); the scalar factors are
// formed in double like torch's host code, then rounded to fp32.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void adam_kernel(const GopsAdamTensors T, GopsAdamState* st, double beta1,
                                                   double beta2, float eps) {
    const double b1p = st->beta1_pow * beta1, b2p = st->beta2_pow * beta2;   // beta^t, t = step + 1
    const float step_size = (float)(st->lr / (1.0 - b1p)), bc2_sqrt = (float)sqrt(1.0 - b2p);
    const float omb1 = (float)(1.0 - beta1), omb2 = (float)(1.0 - beta2), b2 = (float)beta2;
    const float gsc = (float)st->grad_scale;   // 1/N of the data-parallel mean (1 otherwise)
    const int ti = blockIdx.y;
    const long long n = T.numel[ti];
    float* __restrict__ p = T.param[ti];
    const float* __restrict__ g = T.grad[ti];
    float* __restrict__ m = T.exp_avg[ti];
    float* __restrict__ v = T.exp_avg_sq[ti];
    // 4 elements per thread with all 16 loads in flight together: the kernel is a chain of memory round trips (load g, m, v, p - store),
    // and a load - store loop pays one per element (65536-element layers, 64 blocks: 9.2 us; one element per thread on 256 blocks costs
    // more than it saves - every block takes the ticket below)
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x; i0 < n; i0 += 4 * stride) {
        float gq[4], mq[4], vq[4], pq[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const long long i = i0 + q * stride;
            const bool ok = i < n;
            gq[q] = ok ? g[i] : 0.f; mq[q] = ok ? m[i] : 0.f; vq[q] = ok ? v[i] : 0.f; pq[q] = ok ? p[i] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const long long i = i0 + q * stride;
            if (i < n && !grad_is_finite(gq[q] * gsc)) {
                atomicAdd(&st->skipped_nonfinite, 1u);   // no step for this element (common.h grad_is_finite)
            } else if (i < n) {
                // restates common.h adam_element, operation for operation: with the call in its place hipcc schedules this loop
                // on 74 instead of 72 VGPRs (7 -> 6 waves per SIMD)
                const float gi = gq[q] * gsc;
                const float mi = mq[q] + (gi - mq[q]) * omb1;
                const float vi = vq[q] * b2 + omb2 * gi * gi;
                m[i] = mi;
                v[i] = vi;
                p[i] = pq[q] - step_size * (mi / (sqrtf(vi) / bc2_sqrt + eps));
            }
        }
    }
    // Every block has read the state (its values feed the arithmetic above) before it takes a ticket;
    // the last one publishes the advanced state.  No fence: the next reader is a later kernel.
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned total = gridDim.x * gridDim.y;
        if (atomicAdd(&st->ticket, 1u) == total - 1) {
            st->ticket = 0;
            st->step += 1;
            st->beta1_pow = b1p;
            st->beta2_pow = b2p;
        }
    }
}

// Polyak averaging of target networks (gops/algorithm/infadp.py:124-133: p_targ.mul_(1 - tau); p_targ.add_(tau * p)), all
// tensors of a network in ONE launch; the same two roundings per element as the two torch passes it replaces.
// Table: param[] = target tensors, grad[] = online tensors (GopsAdamTensors reused; the moment slots are ignored).
__global__ __launch_bounds__(256) void polyak_kernel(const GopsAdamTensors T, float omt, float tau) {
    const int ti = blockIdx.y;
    const long long n = T.numel[ti];
    float* __restrict__ t = T.param[ti];
    const float* __restrict__ o = T.grad[ti];
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        t[i] = polyak_element(t[i], o[i], omt, tau);
}

// Loss scalars of a batch in ONE launch (they were three torch reductions + three elementwise passes per INFADP update pair:
// ~10 % of a cfg5 fp16 update).  a, b: [n]; grad (nullable) <- gsc * (a - b);  stats[0] <- sum((a - b)^2) / n (b null: sc0 * sum(a) / n),
// stats[1] <- sum(a) / n.  Blocks add up their elements in double in a fixed order and park the partial sums behind the two results
// (stats[2 ..]: GOPS_LOSS_STATS_FLOATS floats in all, the last one a ticket that must be zero on entry and is left zero); the last block to
// finish adds the partials in block order - deterministic (block_reduce.h).
#define LOSS_BLOCKS 64
__global__ __launch_bounds__(256) void batch_loss_kernel(const float* __restrict__ a, const float* __restrict__ b, int n, float gsc, float sc0,
                                                         float* __restrict__ grad, float* __restrict__ stats) {
    __shared__ double red[2][4];
    __shared__ bool last;
    double s[2] = {0.0, 0.0};
    // 8 elements per thread in flight (a load - add loop pays one memory round trip per element); added in index order
    const int stride = gridDim.x * 256;
    for (int i0 = blockIdx.x * 256 + threadIdx.x; i0 < n; i0 += 8 * stride) {
        float av[8], bv[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int i = i0 + q * stride;
            av[q] = i < n ? a[i] : 0.f;
            bv[q] = (b != nullptr && i < n) ? b[i] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int i = i0 + q * stride;
            if (i < n) {
                if (b != nullptr) {
                    const float d = av[q] - bv[q];
                    if (grad != nullptr) grad[i] = gsc * d;
                    s[0] += (double)(d * d);
                } else {
                    s[0] += (double)av[q];
                }
                s[1] += (double)av[q];
            }
        }
    }
    // the blocks' partial sums [LOSS_BLOCKS][2] behind the two results, then the ticket
    if (grid_fold<2>(s, red, reinterpret_cast<double*>(stats + 2), 2, reinterpret_cast<unsigned*>(stats + 2 + 4 * LOSS_BLOCKS), &last) &&
        threadIdx.x == 0) {
        stats[0] = (float)((b != nullptr ? 1.0 : (double)sc0) * s[0] / (double)n);
        stats[1] = (float)(s[1] / (double)n);
    }
}
hipError_t launch_batch_loss(const float* a, const float* b, int n, float gsc, float sc0, float* grad, float* stats, hipStream_t s) {
    hipLaunchKernelGGL(batch_loss_kernel, dim3(n <= LOSS_ONE_BLOCK_MAX ? 1 : LOSS_BLOCKS), dim3(256), 0, s, a, b, n, gsc, sc0, grad, stats);
    return hipGetLastError();
}

extern "C" {

int gops_adam_step(const GopsAdamTensors* tensors, GopsAdamState* st, double beta1, double beta2, double eps, void* stream) {
    if (!tensors || !st || tensors->n < 1 || tensors->n > GOPS_ADAM_MAX_TENSORS) return GOPS_ERR_BAD_ARG;
    const GopsAdamTensors& T = *tensors;
    for (int i = 0; i < T.n; ++i)
        if (!T.param[i] || !T.grad[i] || !T.exp_avg[i] || !T.exp_avg_sq[i] || T.numel[i] < 1) return GOPS_ERR_BAD_ARG;
    long long nmax = 1;
    for (int i = 0; i < T.n; ++i) nmax = T.numel[i] > nmax ? T.numel[i] : nmax;
    int bx = (int)((nmax + 1023) / 1024);   // >= 4 elements per thread of the largest tensor
    if (bx > 64) bx = 64;
    hipLaunchKernelGGL(adam_kernel, dim3(bx, T.n), dim3(256), 0, static_cast<hipStream_t>(stream), T, st, beta1, beta2, (float)eps);
    return (int)hipGetLastError();
}

int gops_polyak_update(const GopsAdamTensors* tensors, double tau, void* stream) {
    if (!tensors || tensors->n < 1 || tensors->n > GOPS_ADAM_MAX_TENSORS) return GOPS_ERR_BAD_ARG;
    const GopsAdamTensors& T = *tensors;
    for (int i = 0; i < T.n; ++i)
        if (!T.param[i] || !T.grad[i] || T.numel[i] < 1) return GOPS_ERR_BAD_ARG;
    long long nmax = 1;
    for (int i = 0; i < T.n; ++i) nmax = std::max<long long>(nmax, T.numel[i]);
    const int bx = (int)std::min<long long>((nmax + 255) / 256, 64);
    hipLaunchKernelGGL(polyak_kernel, dim3(bx, T.n), dim3(256), 0, static_cast<hipStream_t>(stream), T, (float)(1.0 - tau), (float)tau);
    return (int)hipGetLastError();
}

int gops_value_loss(const float* v, const float* target, int32_t n, float* grad, float* stats, void* stream) {
    if (!v || !target || !stats || n < 1) return GOPS_ERR_BAD_ARG;
    return (int)launch_batch_loss(v, target, n, (float)(2.0 / n), 1.f, grad, stats, static_cast<hipStream_t>(stream));
}

int gops_mean_loss(const float* x, int32_t n, double scale, float* stats, void* stream) {
    if (!x || !stats || n < 1) return GOPS_ERR_BAD_ARG;
    return (int)launch_batch_loss(x, nullptr, n, 0.f, (float)scale, nullptr, stats, static_cast<hipStream_t>(stream));
}

}  // extern "C"
