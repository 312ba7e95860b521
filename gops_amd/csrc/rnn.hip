// Recurrent networks (gops/apprfunc/rnn.py): an Elman recurrence over a stack of L observations, h_t = tanh(W_ih x_t + b_ih +
// W_hh h_{t-1} + b_hh) with h_0 = 0, whose last hidden state feeds one or two MLP heads - include/gops_hip.h:
// gops_rnn_workspace_bytes / _forward / _backward.
//
// Mapping.  A workgroup of 256 threads owns a tile of TB = 16 samples, the M of v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32
// accumulation).  The H hidden columns are cut into 16-wide blocks dealt round-robin to the four waves (block nt -> wave nt & 3), so
// a wave owns at most NB = 2 blocks at H = 128.
//   forward (one launch):  a wave loads the B-operand fragments of ITS blocks of W_hh ([16 c + 4 g + i][n], c < H / 16: 4 NB f32x4
//     per block) and of W_ih once and keeps them in registers for all L steps.  The tile's h lives in LDS in two buffers (read
//     t - 1, write t); x_{t+1} is staged into the other of two x buffers while step t computes.  Per step: one MFMA chain over
//     k = O, then k = H, into the same accumulators; bias, tanh, the store to the other h buffer and to the stash [L][Bpad][H]; one
//     barrier.  The heads then run on the same tile: activations in LDS, weights streamed from L2 in torch layout, each hidden
//     layer's activation AND its derivative to the stash (the sweep evaluates no transcendental), the output layer as one masked
//     16-column block.
//   backward (sweep + reduce):  a workgroup walks its tiles (tile = block, block + grid, ...; the grid is capped at RNN_GRID_MAX).
//     Heads in reverse give dh_L (two heads: summed); their weight gradients are MFMAs whose K is the 16 samples, added into the
//     workgroup's slot of the workspace.  Then t = L .. 1: dz_t = dh_t (1 - h_t^2) and h_{t-1}, x_t go to LDS; the wave's rows of
//     dW_hh += dz_t^T h_{t-1} and dW_ih += dz_t^T x_t are accumulated IN REGISTERS over all t and all tiles; dh_{t-1} = dz_t W_hh
//     with W_hh register-stationary in the transposed orientation; db is summed per element by the thread that formed dz.  At the
//     end every workgroup writes [dW_ih | dW_hh | db | heads] to its slot, and rnn_reduce_kernel sums the slots in workgroup order.
// No float atomics anywhere: results are bitwise reproducible.  Rows beyond B are computed on zeros (the forward) or carry zero
// deltas (the sweep); nothing is stored to y for them and grad_y is not read there.
#include <hip/hip_runtime.h>
#include <math.h>

#include "common.h"
#include "rnn_tile.h"

#define RNN_MAX_SEGS (3 + 2 * GOPS_MAX_LAYERS * GOPS_RNN_MAX_HEADS)
#define RNN_MAX_XB (GOPS_RNN_MAX_OBS / 16)                    // 16-column blocks of the padded x tile

// (RnnHeadDev, RnnDev, rnn_stage_x: rnn_tile.h)
struct RnnSegs {   // the slot layout as (start, destination) pairs for the reduce
    int n, G, P, pad_;
    int start[RNN_MAX_SEGS + 1];
    float* dst[RNN_MAX_SEGS];
    float* dst2[RNN_MAX_SEGS];         // db goes to bias_ih and bias_hh
};

// (rnn_dense, the forward orientation of a head's layer: rnn_tile.h)
// [TB][K] = D [TB][N] (LDS, columns up to the next multiple of 16 zero) W, W [N][K]; blocks of 16 columns k dealt to the waves.
// epi(acc, k): acc[r] = element (row 4 g + r, column k).  K is a multiple of 16.
template <class Epi>
__device__ __forceinline__ void rnn_dense_t(const float* D, int ldd, int N, const float* W, int K, int lane, int wave, Epi&& epi) {
    const int l15 = lane & 15, g = lane >> 4;
    for (int kt = wave; 16 * kt < K; kt += 4) {
        const int k = 16 * kt + l15;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int c = 0; 16 * c < N; ++c) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(D + l15 * ldd + 16 * c + 4 * g);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int n = 16 * c + 4 * g + i;
                const float b = n < N ? gptr(W)[(size_t)n * K + k] : 0.f;
                acc = mfma4(a[i], b, acc);
            }
        }
        epi(acc, k);
    }
}

// slot [N][K] (+)= D^T A over the 16 samples of the tile: D [TB][N], A [TB][K] in LDS, both zero up to the next multiple of 16
// columns; the (N / 16) x (K / 16) blocks are dealt to the waves - the same (wave, lane) owns an element for every tile.
__device__ __forceinline__ void rnn_dw(const float* D, int ldd, int N, const float* A, int lda, int K, float* slot, bool first, int lane,
                                       int wave) {
    const int l15 = lane & 15, g = lane >> 4;
    const int nbj = (K + 15) >> 4, nblk = ((N + 15) >> 4) * nbj;
    for (int blk = wave; blk < nblk; blk += 4) {
        const int it = blk / nbj, jt = blk - it * nbj;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < 4; ++q) acc = mfma4(D[(4 * q + g) * ldd + 16 * it + l15], A[(4 * q + g) * lda + 16 * jt + l15], acc);
        const int j = 16 * jt + l15;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = 16 * it + 4 * g + r;
            if (i < N && j < K) {
                GLOBAL_AS float* dst = gptr(slot) + (size_t)i * K + j;
                *dst = first ? acc[r] : *dst + acc[r];
            }
        }
    }
}

// ---- forward ------------------------------------------------------------------------------------------------------------------------
// LDS: three hidden tiles [TB][ldw] (two of the recurrence, a third so that h_L survives the first head), two x tiles [TB][ldx].
template <int NB>
__global__ __launch_bounds__(NTHREADS) void rnn_fwd_kernel(const RnnDev p, const float* __restrict__ x, float* __restrict__ y) {
    extern __shared__ float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4;
    const int ldw = p.ldw, ldx = p.ldx, L = p.L;
    const int row0 = blockIdx.x * TB;
    float* const hb = lds;
    float* const xb = lds + 3 * TB * ldw;

    RnnRegs<NB> w;
    rnn_load_regs<NB>(p, wave, lane, w);
    rnn_stage_x(p, x, row0, 0, xb, tid);
    __syncthreads();

    for (int t = 0; t < L; ++t) {
        const int cur = t & 1;   // h_t in hidden tile cur, h_{t+1} into the other
        rnn_step<NB>(p, w, t, row0, hb + cur * TB * ldw, hb + (cur ^ 1) * TB * ldw, xb + cur * TB * ldx, true, wave, lane);
        if (t + 1 < L) rnn_stage_x(p, x, row0, t + 1, xb + (cur ^ 1) * TB * ldx, tid);
        __syncthreads();
    }

    rnn_heads(p, hb, row0, true, lane, wave, [&](const RnnHeadDev& hp, const f32x4& acc, float bn, int n) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row0 + 4 * g + r;
            if (row < p.B) gptr(y)[(size_t)row * p.ny + hp.yoff + n] = acc[r] + bn;
        }
    });
}

// ---- backward sweep -------------------------------------------------------------------------------------------------------------------
// LDS: four hidden-width tiles [TB][ldw] - dh (the adjoint of h_t), dz, the layer input / h_{t-1}, a second delta tile for the heads -
// and one x tile [TB][ldx].
template <int NB>
__global__ __launch_bounds__(NTHREADS) void rnn_bwd_kernel(const RnnDev p, const float* __restrict__ x, const float* __restrict__ gy) {
    extern __shared__ float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4;
    const int H = p.H, nhb = H >> 4, ldw = p.ldw, ldx = p.ldx, L = p.L, nxb = p.O16 >> 4;
    float* const dh = lds;
    float* const dz = lds + TB * ldw;
    float* const hin = lds + 2 * TB * ldw;
    float* const d2 = lds + 3 * TB * ldw;
    float* const xs = lds + 4 * TB * ldw;
    float* const slot = p.slots + (size_t)blockIdx.x * p.P;
    const int ntiles = p.Bpad / TB;

    // W_hh in the transposed orientation (the B operand of dh_{t-1} = dz_t W_hh) for the wave's column blocks: resident
    f32x4 wt[4 * NB][NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const int kt = wave + 4 * j, k = 16 * kt + l15;
#pragma unroll
        for (int c = 0; c < 4 * NB; ++c)
#pragma unroll
            for (int i = 0; i < 4; ++i)
                wt[c][j][i] = (kt < nhb && c < nhb) ? gptr(p.whh)[(size_t)(16 * c + 4 * g + i) * H + k] : 0.f;
    }
    // the wave's rows of dW_hh and dW_ih, and this thread's elements of sum_t dz_t: accumulated over all steps and tiles
    f32x4 ahh[NB][4 * NB] = {}, aih[NB][RNN_MAX_XB] = {};
    float dzs[4 * NB] = {};

    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int row0 = tile * TB;
        const bool first = tile == (int)blockIdx.x;
        // ---- heads, output layer first: dh <- sum over heads of the adjoint of h_L
        for (int hd = 0; hd < p.nheads; ++hd) {
            const RnnHeadDev& hp = p.head[hd];
            float *dc = dz, *dn = d2;
            const int out = hp.dims[hp.nl];
            for (int idx = tid; idx < TB * 16; idx += NTHREADS) {
                const int m = idx >> 4, n = idx & 15;
                dc[m * ldw + n] = (row0 + m < p.B && n < out) ? gptr(gy)[(size_t)(row0 + m) * p.ny + hp.yoff + n] : 0.f;
            }
            for (int l = hp.nl - 1; l >= 0; --l) {
                const int K = hp.dims[l], N = hp.dims[l + 1], k4 = K >> 2;
                const float* src = l == 0 ? p.hst + ((size_t)(L - 1) * p.Bpad + row0) * H : hp.sh[l - 1] + (size_t)row0 * K;
                for (int idx = tid; idx < TB * k4; idx += NTHREADS) {
                    const int m = idx / k4, c4 = idx - m * k4;
                    *reinterpret_cast<f32x4*>(hin + m * ldw + 4 * c4) = ld4(gptr(src) + (size_t)m * K + 4 * c4);
                }
                __syncthreads();
                rnn_dw(dc, ldw, N, hin, ldw, K, slot + hp.off_w[l], first, lane, wave);
                if (tid < N) {
                    float s = 0.f;
                    for (int m = 0; m < TB; ++m) s += dc[m * ldw + tid];
                    GLOBAL_AS float* dst = gptr(slot) + hp.off_b[l] + tid;
                    *dst = first ? s : *dst + s;
                }
                if (l > 0) {
                    const float* sd = hp.sd[l - 1];
                    rnn_dense_t(dc, ldw, N, hp.w[l], K, lane, wave, [&](const f32x4& acc, int k) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int row = 4 * g + r;
                            dn[row * ldw + k] = acc[r] * gptr(sd)[(size_t)(row0 + row) * K + k];
                        }
                    });
                } else {
                    rnn_dense_t(dc, ldw, N, hp.w[l], K, lane, wave, [&](const f32x4& acc, int k) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            float* d = dh + (4 * g + r) * ldw + k;
                            *d = hd == 0 ? acc[r] : *d + acc[r];
                        }
                    });
                }
                __syncthreads();
                float* sw = dc; dc = dn; dn = sw;
            }
        }
        // ---- the recurrence in reverse: step t (0-based) has h_{t+1} at stash row t
        for (int t = L - 1; t >= 0; --t) {
#pragma unroll
            for (int e = 0; e < 4 * NB; ++e)
                if (e < nhb) {
                    const int idx = tid + NTHREADS * e, m = idx / H, n = idx - m * H;
                    const size_t at = ((size_t)t * p.Bpad + row0 + m) * H + n;
                    const float hv = gptr(p.hst)[at];
                    const float d = dh[m * ldw + n] * (1.f - hv * hv);
                    dz[m * ldw + n] = d;
                    dzs[e] += d;
                    hin[m * ldw + n] = t > 0 ? gptr(p.hst)[at - (size_t)p.Bpad * H] : 0.f;
                }
            rnn_stage_x(p, x, row0, t, xs, tid);
            __syncthreads();
            if (wave < nhb) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int m = 4 * q + g;
                    float a[NB];
#pragma unroll
                    for (int j = 0; j < NB; ++j) a[j] = (wave + 4 * j < nhb) ? dz[m * ldw + 16 * (wave + 4 * j) + l15] : 0.f;
                    if (t > 0) {   // h_0 = 0: dW_hh takes nothing from the first step (exactly zero for L = 1)
#pragma unroll
                        for (int jt = 0; jt < 4 * NB; ++jt)
                            if (jt < nhb) {
                                const float b = hin[m * ldw + 16 * jt + l15];
#pragma unroll
                                for (int j = 0; j < NB; ++j) ahh[j][jt] = mfma4(a[j], b, ahh[j][jt]);
                            }
                    }
#pragma unroll
                    for (int jt = 0; jt < RNN_MAX_XB; ++jt)
                        if (jt < nxb) {
                            const float b = xs[m * ldx + 16 * jt + l15];
#pragma unroll
                            for (int j = 0; j < NB; ++j) aih[j][jt] = mfma4(a[j], b, aih[j][jt]);
                        }
                }
                if (t > 0) {
                    f32x4 acc[NB] = {};
#pragma unroll
                    for (int c = 0; c < 4 * NB; ++c)
                        if (c < nhb) {
                            const f32x4 a = *reinterpret_cast<const f32x4*>(dz + l15 * ldw + 16 * c + 4 * g);
#pragma unroll
                            for (int i = 0; i < 4; ++i)
#pragma unroll
                                for (int j = 0; j < NB; ++j) acc[j] = mfma4(a[i], wt[c][j][i], acc[j]);
                        }
#pragma unroll
                    for (int j = 0; j < NB; ++j)
                        if (wave + 4 * j < nhb) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) dh[(4 * g + r) * ldw + 16 * (wave + 4 * j) + l15] = acc[j][r];
                        }
                }
            }
            __syncthreads();
        }
    }

    // ---- this workgroup's partial of the recurrent gradients -> its slot
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const int it = wave + 4 * j;
        if (it < nhb) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = 16 * it + 4 * g + r;
#pragma unroll
                for (int jt = 0; jt < 4 * NB; ++jt)
                    if (jt < nhb) gptr(slot)[p.off_whh + (size_t)i * H + 16 * jt + l15] = ahh[j][jt][r];
#pragma unroll
                for (int jt = 0; jt < RNN_MAX_XB; ++jt)
                    if (jt < nxb && 16 * jt + l15 < p.O) gptr(slot)[p.off_wih + (size_t)i * p.O + 16 * jt + l15] = aih[j][jt][r];
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 4 * NB; ++e)
        if (e < nhb) {
            const int idx = tid + NTHREADS * e, m = idx / H, n = idx - m * H;
            dz[m * ldw + n] = dzs[e];
        }
    __syncthreads();
    if (tid < H) {
        float s = 0.f;
        for (int m = 0; m < TB; ++m) s += dz[m * ldw + tid];
        gptr(slot)[p.off_b + tid] = s;
    }
}

// element e of the gradient set = the sum of element e of every slot, in slot order
__global__ __launch_bounds__(NTHREADS) void rnn_reduce_kernel(const float* __restrict__ slots, const RnnSegs s) {
    const int e = blockIdx.x * NTHREADS + threadIdx.x;
    if (e >= s.P) return;
    float sum = gptr(slots)[e];
    for (int gi = 1; gi < s.G; ++gi) sum += gptr(slots)[(size_t)gi * s.P + e];
#pragma unroll
    for (int i = 0; i < RNN_MAX_SEGS; ++i)
        if (i < s.n && e >= s.start[i] && e < s.start[i + 1]) {
            gptr(s.dst[i])[e - s.start[i]] = sum;
            if (s.dst2[i] != nullptr) gptr(s.dst2[i])[e - s.start[i]] = sum;
        }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
// (the checks of the description - rnn_check - and its plan - rnn_plan -: rnn_tile.h)

extern "C" {

size_t gops_rnn_workspace_bytes(const GopsRnn* net, int32_t B) {
    if (!net || rnn_check(*net, B) != GOPS_OK) return 0;
    return rnn_plan(*net, B, nullptr).bytes;
}

int gops_rnn_forward(const GopsRnn* net, int32_t B, const float* x, float* y, void* ws, size_t bytes, void* stream) {
    if (net == nullptr) return GOPS_ERR_BAD_ARG;
    const int rc = rnn_check(*net, B);
    if (rc != GOPS_OK) return rc;
    if (x == nullptr || y == nullptr) return GOPS_ERR_BAD_ARG;
    if (ws == nullptr || bytes < rnn_plan(*net, B, nullptr).bytes) return GOPS_ERR_WORKSPACE;
    const RnnPlan pl = rnn_plan(*net, B, ws);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (net->hidden <= 64)
        hipLaunchKernelGGL(rnn_fwd_kernel<1>, dim3(pl.ntiles), dim3(NTHREADS), pl.lds_fwd, s, pl.dev, x, y);
    else
        hipLaunchKernelGGL(rnn_fwd_kernel<2>, dim3(pl.ntiles), dim3(NTHREADS), pl.lds_fwd, s, pl.dev, x, y);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? GOPS_OK : (int)e;
}

int gops_rnn_backward(const GopsRnn* net, int32_t B, const float* x, const float* grad_y, const GopsRnnGrad* grad, void* ws, size_t bytes,
                      void* stream) {
    if (net == nullptr || grad == nullptr) return GOPS_ERR_BAD_ARG;
    const int rc = rnn_check(*net, B);
    if (rc != GOPS_OK) return rc;
    if (x == nullptr || grad_y == nullptr) return GOPS_ERR_BAD_ARG;
    if (!grad->weight_ih || !grad->weight_hh || !grad->bias_ih || !grad->bias_hh) return GOPS_ERR_BAD_ARG;
    for (int h = 0; h < net->n_heads; ++h)
        for (int l = 0; l < net->head[h].n_layers; ++l)
            if (!grad->head[h].weight[l] || !grad->head[h].bias[l]) return GOPS_ERR_BAD_ARG;
    if (ws == nullptr || bytes < rnn_plan(*net, B, nullptr).bytes) return GOPS_ERR_WORKSPACE;
    const RnnPlan pl = rnn_plan(*net, B, ws);
    const RnnDev& p = pl.dev;
    RnnSegs sg = {};
    sg.G = p.G; sg.P = p.P;
    auto seg = [&](int start, float* dst, float* dst2) { sg.start[sg.n] = start; sg.dst[sg.n] = dst; sg.dst2[sg.n] = dst2; ++sg.n; };
    seg(p.off_wih, grad->weight_ih, nullptr);
    seg(p.off_whh, grad->weight_hh, nullptr);
    seg(p.off_b, grad->bias_ih, grad->bias_hh);
    for (int h = 0; h < net->n_heads; ++h)
        for (int l = 0; l < net->head[h].n_layers; ++l) {
            seg(p.head[h].off_w[l], grad->head[h].weight[l], nullptr);
            seg(p.head[h].off_b[l], grad->head[h].bias[l], nullptr);
        }
    sg.start[sg.n] = p.P;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (net->hidden <= 64)
        hipLaunchKernelGGL(rnn_bwd_kernel<1>, dim3(p.G), dim3(NTHREADS), pl.lds_bwd, s, p, x, grad_y);
    else
        hipLaunchKernelGGL(rnn_bwd_kernel<2>, dim3(p.G), dim3(NTHREADS), pl.lds_bwd, s, p, x, grad_y);
    hipLaunchKernelGGL(rnn_reduce_kernel, dim3((p.P + NTHREADS - 1) / NTHREADS), dim3(NTHREADS), 0, s, p.slots, sg);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? GOPS_OK : (int)e;
}

}  // extern "C"
