// Convolution stacks (gops/apprfunc/cnn.py): n_conv layers Conv2d(C_in, C_out, k, stride) + ReLU, no padding, no dilation, on
// x [B, C, H, W]; the last layer's output in (C, H, W) order is the feature row the MLP heads read - include/gops_hip.h:
// gops_conv_workspace_bytes / _forward / _backward.
//
// Every kernel is an implicit GEMM on v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation) whose A operand is GATHERED
// from an activation tensor into an LDS tile; the weights are read in torch layout [C_out][C_in][k][k] and re-ordered on their way
// into LDS (no pack launch).  Inner activations and every dZ are channels-last [B][Ho][Wo][C]: four consecutive k of one tap are one
// 16-byte load (the VEC instantiations, C a multiple of 4).  The first layer gathers from the caller's NCHW tensor (k = (c, kh, kw):
// torch's own weight order); the last layer stores NCHW, which IS the feature tensor.
//   forward, one launch per layer (conv_fwd_kernel):  M = output pixels (b, oh, ow) of the whole batch, N = C_out, K = C_in k k.  A
//     workgroup of 256 threads owns a 64 x 64 tile (grid: M tiles x N tiles); wave w has rows 16 w .. 16 w + 15 and up to four
//     16-column accumulator blocks.  K is walked in chunks of CV_KC = 32: A [64][32] and W [64][32] go to LDS in the same K order
//     (rows beyond C_out and columns beyond K zero), the next chunk's global loads are in flight during the MFMAs.  Epilogue: bias,
//     ReLU, one store - the next layer's input and the backward's stash.
//   data gradient, one launch for each of layers 2 .. n (conv_dgrad_kernel):  gather form, no atomics.  M = input pixels, N = C_in,
//     K = (kh, kw, c_out).  blockIdx.z is the stride phase (ih mod s, iw mod s): the rows of a tile share the taps kh = ph (mod s),
//     kw = pw (mod s), so K holds valid taps only; a tap outside the output extent is masked per row (the border, and the rows /
//     columns the floor in (H - k) / s + 1 never reads: exactly zero).  Epilogue: times relu' of the stashed activation -> dZ of
//     the previous layer.
//   weight gradient, one launch per layer (conv_wgrad_kernel) + one reduce:  dW[n][k] = sum_m dZ[m][n] A[m][k], the MFMA's K is 16
//     pixels.  A workgroup owns a 64 (n) x 64 (k) tile of dW and one of S slices of M, accumulates in registers over its slice (32
//     pixels per LDS chunk) and leaves ONE partial in its slot, in torch's weight order; db = the column sums of the same dZ tiles
//     (the k-tile-0 workgroups).  conv_reduce_kernel sums the slots in slice order: bitwise reproducible.
//   conv_seed_kernel forms the last layer's dZ = (grad_a + grad_b) relu'(features), channels-last.
#include <hip/hip_runtime.h>

#include "common.h"

#define CV_TM 64                        // pixels (GEMM rows) of a forward / data-gradient tile
#define CV_TN 64                        // columns of it
#define CV_KC 32                        // K chunk
#define CV_LD (CV_KC + 4)               // LDS leading dim of both tiles (floats): 16-byte aligned rows, f32x4 reads spread over the banks
#define CV_WM 32                        // pixels per LDS chunk of the weight gradient
#define CV_WT 64                        // its tile of dW: CV_WT (n) x CV_WT (k)
#define CV_WLD (CV_WT + 16)             // rows 4 q + g of a scalar fragment read fall on distinct banks
#define CV_SLICE_ROWS 512               // a slice of M is at least this many pixels ...
#define CV_MAX_SLICES 256               // ... there are at most this many ...
#define CV_SLOT_BUDGET ((size_t)4 << 20)   // ... and a layer's slots take at most 4 MiB of the workspace (one slot always fits)
#define CV_MAX_ELEMS (1 << 30)          // batch x the largest per-sample tensor: offsets are ints

enum { CV_NCHW = 0, CV_NHWC = 1, CV_DGRAD = 2 };   // what the A operand is gathered from

struct ConvDev {   // one layer of one launch
    int B, C, H, W;            // the layer's input: channels and extent
    int N, ks, st, Ho, Wo;     // output channels, kernel, stride, output extent
    int K, M;                  // C ks ks and B Ho Wo
    int out_nchw;              // forward: the last layer stores (C, H, W) order, to dst and dst2
    int S, rows, P;            // weight gradient: slices, pixels per slice (a multiple of CV_WM), floats per slot = N K + N
    const float *src, *w, *bias;   // forward / weight gradient: the layer's input; weights [N][C][ks][ks]
    float *dst, *dst2;
    const float *dz, *act;     // dZ of this layer [M][N]; data gradient: the stashed input activation [B][H][W][C]
    float* dzo;                // data gradient: dZ of the previous layer [B][H][W][C]
    float* slots;              // [S][P]
};
struct ConvReduce {
    int n, pad_;
    int S[GOPS_CONV_MAX_LAYERS], P[GOPS_CONV_MAX_LAYERS], NK[GOPS_CONV_MAX_LAYERS];
    const float* slots[GOPS_CONV_MAX_LAYERS];
    float* dw[GOPS_CONV_MAX_LAYERS];
    float* db[GOPS_CONV_MAX_LAYERS];
};

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 acc) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0); }

// the GEMM a launch sees: K, M, and for the data gradient its stride phase, taps per row of taps and phase extent
struct ConvView { int K, M, ph, pw, Tkw, Hp, Wp; };
template <int MODE>
__device__ __forceinline__ ConvView conv_view(const ConvDev& p, int phase) {
    ConvView v = {p.K, p.M, 0, 0, 1, 1, 1};
    if constexpr (MODE == CV_DGRAD) {
        v.ph = phase / p.st; v.pw = phase - v.ph * p.st;
        v.Tkw = (p.ks - v.pw + p.st - 1) / p.st;
        v.Hp = (p.H - v.ph + p.st - 1) / p.st; v.Wp = (p.W - v.pw + p.st - 1) / p.st;   // (>= 1: ph < s <= k <= H)
        v.K = ((p.ks - v.ph + p.st - 1) / p.st) * v.Tkw * p.N; v.M = p.B * v.Hp * v.Wp;
    }
    return v;
}

// GEMM row m -> the offset of its origin in the gathered tensor (data gradient: of output pixel (a, b), which may lie beyond the
// output extent - its taps are then masked - with the phase coordinates kept for that mask)
struct ConvRow { int base, a, b; bool ok; };
template <int MODE>
__device__ __forceinline__ ConvRow conv_row(const ConvDev& p, const ConvView& v, int m, bool ok) {
    ConvRow r = {0, 0, 0, ok};
    if (!ok) return r;
    if constexpr (MODE == CV_DGRAD) {
        const int hw = v.Hp * v.Wp, b = m / hw, q = m - b * hw;
        r.a = q / v.Wp; r.b = q - r.a * v.Wp;
        r.base = ((b * p.Ho + r.a) * p.Wo + r.b) * p.N;
    } else {
        const int hw = p.Ho * p.Wo, b = m / hw, q = m - b * hw, oh = q / p.Wo, ow = q - oh * p.Wo;
        r.base = MODE == CV_NCHW ? (b * p.C * p.H + oh * p.st) * p.W + ow * p.st : ((b * p.H + oh * p.st) * p.W + ow * p.st) * p.C;
    }
    return r;
}

// GEMM column k -> its offset from a row's origin, its offset in a row of the weights (row stride: K forward, ks ks data gradient),
// and for the data gradient the tap's distance (th, tw) in output pixels
struct ConvK { int aoff, woff, th, tw; };
template <int MODE>
__device__ __forceinline__ ConvK conv_k(const ConvDev& p, const ConvView& v, int k) {
    ConvK d = {0, 0, 0, 0};
    if constexpr (MODE == CV_NCHW) {         // k = (c, kh, kw)
        const int kk = p.ks * p.ks, c = k / kk, q = k - c * kk, kh = q / p.ks, kw = q - kh * p.ks;
        d.aoff = (c * p.H + kh) * p.W + kw; d.woff = k;
    } else if constexpr (MODE == CV_NHWC) {  // k = (kh, kw, c)
        const int tap = k / p.C, c = k - tap * p.C, kh = tap / p.ks, kw = tap - kh * p.ks;
        d.aoff = (kh * p.W + kw) * p.C + c; d.woff = (c * p.ks + kh) * p.ks + kw;
    } else {                                 // k = (th, tw, c_out), kh = ph + s th, kw = pw + s tw
        const int tap = k / p.N, co = k - tap * p.N;
        d.th = tap / v.Tkw; d.tw = tap - d.th * v.Tkw;
        d.aoff = co - (d.th * p.Wo + d.tw) * p.N;
        d.woff = (co * p.C * p.ks + v.ph + p.st * d.th) * p.ks + v.pw + p.st * d.tw;
    }
    return d;
}

// ---- forward and data gradient: one main loop -------------------------------------------------------------------------------------
// acc[j] += A [64 rows from m0][K] W^T for the column blocks j < nblk of the tile at n0.  A thread's share of the A tile: scalar - 8 rows
// (tid >> 5) + 8 e at column tid & 31; VEC - 2 rows (tid >> 3) + 32 e at the four columns from 4 (tid & 7).  The weight tile is
// always the scalar share.  `wrow`: the weights' row stride; `ncols`: the GEMM's N.
template <int MODE, bool VEC>
__device__ __forceinline__ void conv_mainloop(const ConvDev& p, const ConvView& v, const float* __restrict__ src, int m0, int n0, int ncols,
                                              int wrow, int nblk, f32x4 (&acc)[4], float* As, float* Bs) {
    constexpr int NR = VEC ? 2 : 8, STEP = VEC ? 32 : 8;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4;
    const int arow = VEC ? tid >> 3 : tid >> 5, akk = VEC ? 4 * (tid & 7) : tid & 31, brow = tid >> 5, bkk = tid & 31;
    ConvRow rows[NR];
#pragma unroll
    for (int e = 0; e < NR; ++e) {
        const int m = m0 + arow + STEP * e;
        rows[e] = conv_row<MODE>(p, v, m, m < v.M);
    }
    float ra[8], rb[8];
    auto load = [&](int k0) {
        const int k = k0 + akk;
        const ConvK d = conv_k<MODE>(p, v, k);
#pragma unroll
        for (int e = 0; e < NR; ++e) {
            bool ok = rows[e].ok && k < v.K;
            if constexpr (MODE == CV_DGRAD) ok = ok && (unsigned)(rows[e].a - d.th) < (unsigned)p.Ho && (unsigned)(rows[e].b - d.tw) < (unsigned)p.Wo;
            if constexpr (VEC) {
                const f32x4 z = {0.f, 0.f, 0.f, 0.f};
                const f32x4 t = ok ? ld4(gptr(src) + rows[e].base + d.aoff) : z;
#pragma unroll
                for (int i = 0; i < 4; ++i) ra[4 * e + i] = t[i];
            } else {
                ra[e] = ok ? gptr(src)[rows[e].base + d.aoff] : 0.f;
            }
        }
        const int kb = k0 + bkk;
        const ConvK db = conv_k<MODE>(p, v, kb);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int n = n0 + brow + 8 * e;
            rb[e] = (n < ncols && kb < v.K) ? gptr(p.w)[(size_t)n * wrow + db.woff] : 0.f;
        }
    };
    load(0);
    for (int k0 = 0; k0 < v.K; k0 += CV_KC) {
#pragma unroll
        for (int e = 0; e < NR; ++e) {
            float* at = As + (arow + STEP * e) * CV_LD + akk;
            if constexpr (VEC) {
                const f32x4 t = {ra[4 * e], ra[4 * e + 1], ra[4 * e + 2], ra[4 * e + 3]};
                *reinterpret_cast<f32x4*>(at) = t;
            } else {
                *at = ra[e];
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) Bs[(brow + 8 * e) * CV_LD + bkk] = rb[e];
        __syncthreads();
        if (k0 + CV_KC < v.K) load(k0 + CV_KC);   // in flight during the MFMAs
#pragma unroll
        for (int c = 0; c < CV_KC / 16; ++c) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(As + (16 * wave + l15) * CV_LD + 16 * c + 4 * g);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < nblk) {
                    const f32x4 b = *reinterpret_cast<const f32x4*>(Bs + (16 * j + l15) * CV_LD + 16 * c + 4 * g);
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[j] = mfma4(a[i], b[i], acc[j]);
                }
        }
        __syncthreads();
    }
}

template <int MODE, bool VEC>
__global__ __launch_bounds__(NTHREADS) void conv_fwd_kernel(const ConvDev p) {
    __shared__ __attribute__((aligned(16))) float As[CV_TM * CV_LD];
    __shared__ __attribute__((aligned(16))) float Bs[CV_TN * CV_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4;
    const ConvView v = conv_view<MODE>(p, 0);
    const int m0 = blockIdx.x * CV_TM, n0 = blockIdx.y * CV_TN;
    const int left = (p.N - n0 + 15) >> 4, nblk = left < 4 ? left : 4;
    f32x4 acc[4] = {};
    conv_mainloop<MODE, VEC>(p, v, p.src, m0, n0, p.N, p.K, nblk, acc, As, Bs);
    const int hw = p.Ho * p.Wo;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = n0 + 16 * j + l15;
        if (j < nblk && n < p.N) {
            const float bn = gptr(p.bias)[n];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + 16 * wave + 4 * g + r;
                if (m < p.M) {
                    const float h = fmaxf(acc[j][r] + bn, 0.f);
                    if (p.out_nchw) {
                        const int b = m / hw, q = m - b * hw;
                        const size_t at = ((size_t)b * p.N + n) * hw + q;
                        gptr(p.dst)[at] = h;
                        gptr(p.dst2)[at] = h;
                    } else {
                        gptr(p.dst)[(size_t)m * p.N + n] = h;
                    }
                }
            }
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(NTHREADS) void conv_dgrad_kernel(const ConvDev p) {
    __shared__ __attribute__((aligned(16))) float As[CV_TM * CV_LD];
    __shared__ __attribute__((aligned(16))) float Bs[CV_TN * CV_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4;
    const ConvView v = conv_view<CV_DGRAD>(p, blockIdx.z);
    const int m0 = blockIdx.x * CV_TM, n0 = blockIdx.y * CV_TN;
    if (m0 >= v.M) return;   // (the grid is sized for phase 0, the largest: uniform, before any barrier)
    const int left = (p.C - n0 + 15) >> 4, nblk = left < 4 ? left : 4;
    f32x4 acc[4] = {};
    conv_mainloop<CV_DGRAD, VEC>(p, v, p.dz, m0, n0, p.C, p.ks * p.ks, nblk, acc, As, Bs);
    const int hw = v.Hp * v.Wp;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int m = m0 + 16 * wave + 4 * g + r;
        if (m < v.M) {
            const int b = m / hw, q = m - b * hw, a = q / v.Wp, bq = q - a * v.Wp;
            const size_t pix = ((size_t)b * p.H + v.ph + p.st * a) * p.W + v.pw + p.st * bq;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int ci = n0 + 16 * j + l15;
                if (j < nblk && ci < p.C) gptr(p.dzo)[pix * p.C + ci] = gptr(p.act)[pix * p.C + ci] > 0.f ? acc[j][r] : 0.f;   // relu'(0) = 0
            }
        }
    }
}

// ---- weight gradient ----------------------------------------------------------------------------------------------------------------
// A thread's share of the A chunk [32][64]: row tid >> 3 at columns (tid & 7) + 8 e (VEC: the four from 4 ((tid & 7) + 8 e)) - the
// columns are the same for every chunk, so k is decoded once; of the dZ chunk [32][64]: element tid + 256 e.
template <int MODE, bool VEC>
__global__ __launch_bounds__(NTHREADS) void conv_wgrad_kernel(const ConvDev p) {
    __shared__ __attribute__((aligned(16))) float Ds[CV_WM * CV_WLD];
    __shared__ __attribute__((aligned(16))) float As[CV_WM * CV_WLD];
    constexpr int NKK = VEC ? 2 : 8;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4;
    const ConvView v = conv_view<MODE>(p, 0);
    const int n0 = blockIdx.x * CV_WT, k0 = blockIdx.y * CV_WT;
    const int mbeg = blockIdx.z * p.rows, mend = mbeg + p.rows < p.M ? mbeg + p.rows : p.M;
    const int arow = tid >> 3;
    int aoff[NKK];
    bool kok[NKK];
#pragma unroll
    for (int e = 0; e < NKK; ++e) {
        const int k = k0 + (VEC ? 4 : 1) * ((tid & 7) + 8 * e);
        kok[e] = k < p.K;
        aoff[e] = conv_k<MODE>(p, v, k).aoff;
    }
    const bool wave_on = n0 + 16 * wave < p.N, with_db = blockIdx.y == 0 && tid < CV_WT;
    f32x4 acc[4] = {};
    float dbs = 0.f, ra[8], rd[8];
    auto load = [&](int mc) {
        const int m = mc + arow;
        const ConvRow r = conv_row<MODE>(p, v, m, m < mend);
#pragma unroll
        for (int e = 0; e < NKK; ++e) {
            const bool ok = r.ok && kok[e];
            if constexpr (VEC) {
                const f32x4 z = {0.f, 0.f, 0.f, 0.f};
                const f32x4 t = ok ? ld4(gptr(p.src) + r.base + aoff[e]) : z;
#pragma unroll
                for (int i = 0; i < 4; ++i) ra[4 * e + i] = t[i];
            } else {
                ra[e] = ok ? gptr(p.src)[r.base + aoff[e]] : 0.f;
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int idx = tid + NTHREADS * e, md = mc + (idx >> 6), n = n0 + (idx & 63);
            rd[e] = (md < mend && n < p.N) ? gptr(p.dz)[(size_t)md * p.N + n] : 0.f;
        }
    };
    load(mbeg);
    for (int mc = mbeg; mc < mend; mc += CV_WM) {
#pragma unroll
        for (int e = 0; e < NKK; ++e) {
            float* at = As + arow * CV_WLD + (VEC ? 4 : 1) * ((tid & 7) + 8 * e);
            if constexpr (VEC) {
                const f32x4 t = {ra[4 * e], ra[4 * e + 1], ra[4 * e + 2], ra[4 * e + 3]};
                *reinterpret_cast<f32x4*>(at) = t;
            } else {
                *at = ra[e];
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int idx = tid + NTHREADS * e;
            Ds[(idx >> 6) * CV_WLD + (idx & 63)] = rd[e];
        }
        __syncthreads();
        if (mc + CV_WM < mend) load(mc + CV_WM);
        if (wave_on) {
#pragma unroll
            for (int q = 0; q < CV_WM / 4; ++q) {
                const int m = 4 * q + g;
                const float a = Ds[m * CV_WLD + 16 * wave + l15];
#pragma unroll
                for (int jt = 0; jt < 4; ++jt)
                    if (k0 + 16 * jt < p.K) acc[jt] = mfma4(a, As[m * CV_WLD + 16 * jt + l15], acc[jt]);
            }
        }
        if (with_db)
            for (int m = 0; m < CV_WM; ++m) dbs += Ds[m * CV_WLD + tid];
        __syncthreads();
    }
    // the partial -> this slice's slot, in torch's weight order
    GLOBAL_AS float* slot = gptr(p.slots) + (size_t)blockIdx.z * p.P;
    if (wave_on) {
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) {
            const int k = k0 + 16 * jt + l15;
            if (k < p.K) {
                const int woff = conv_k<MODE>(p, v, k).woff;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int n = n0 + 16 * wave + 4 * g + r;
                    if (n < p.N) slot[(size_t)n * p.K + woff] = acc[jt][r];
                }
            }
        }
    }
    if (with_db && n0 + tid < p.N) slot[(size_t)p.N * p.K + n0 + tid] = dbs;
}

// element e of layer blockIdx.y's (dW | db) = the sum of element e of its slots, in slice order
__global__ __launch_bounds__(NTHREADS) void conv_reduce_kernel(const ConvReduce r) {
    const int l = blockIdx.y, e = blockIdx.x * NTHREADS + threadIdx.x, P = r.P[l];
    if (e >= P) return;
    const GLOBAL_AS float* slots = gptr(r.slots[l]);
    float sum = slots[e];
    for (int s = 1; s < r.S[l]; ++s) sum += slots[(size_t)s * P + e];
    if (e < r.NK[l]) gptr(r.dw[l])[e] = sum;
    else gptr(r.db[l])[e - r.NK[l]] = sum;
}

// dZ of the last layer, channels-last [B][hw][N], from the feature gradients in (C, H, W) order: (ga + gb) relu'(feature)
__global__ __launch_bounds__(NTHREADS) void conv_seed_kernel(const float* __restrict__ feat, const float* __restrict__ ga,
                                                             const float* __restrict__ gb, float* __restrict__ dz, int N, int hw, int total) {
    const int e = blockIdx.x * NTHREADS + threadIdx.x;
    if (e >= total) return;
    const int m = e / N, n = e - m * N, b = m / hw, q = m - b * hw;
    const size_t f = ((size_t)b * N + n) * hw + q;
    float gsum = gptr(ga)[f];
    if (gb != nullptr) gsum += gptr(gb)[f];
    gptr(dz)[e] = gptr(feat)[f] > 0.f ? gsum : 0.f;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
// every check of the description: GOPS_OK, or the code the three entry points refuse it with
static int conv_check(const GopsConv& d, int B) {
    if (B < 1 || d.n_conv < 1) return GOPS_ERR_BAD_ARG;
    if (d.n_conv > GOPS_CONV_MAX_LAYERS) return GOPS_ERR_UNSUPPORTED;
    for (int l = 0; l < d.n_conv; ++l)
        if (!d.weight[l] || !d.bias[l]) return GOPS_ERR_BAD_ARG;
    if (d.in_channels < 1 || d.in_channels > GOPS_CONV_MAX_CHANNELS) return GOPS_ERR_UNSUPPORTED;
    if (d.in_h < 1 || d.in_h > GOPS_CONV_MAX_EXTENT || d.in_w < 1 || d.in_w > GOPS_CONV_MAX_EXTENT) return GOPS_ERR_UNSUPPORTED;
    int H = d.in_h, W = d.in_w;
    long long most = (long long)d.in_channels * H * W;
    for (int l = 0; l < d.n_conv; ++l) {
        const int k = d.kernel[l], s = d.stride[l], N = d.channels[l];
        if (N < 1 || N > GOPS_CONV_MAX_CHANNELS || k < 1 || k > GOPS_CONV_MAX_KERNEL || s < 1 || s > GOPS_CONV_MAX_STRIDE || s > k) return GOPS_ERR_UNSUPPORTED;
        if (H < k || W < k) return GOPS_ERR_UNSUPPORTED;   // an output extent of 0
        const int Hin = H, Win = W;
        H = (H - k) / s + 1; W = (W - k) / s + 1;
        // (the data gradient forms offsets of output pixels up to the phase extent, ceil(Hin / s) x ceil(Win / s))
        const long long reach = (long long)N * ((Hin + s - 1) / s) * ((Win + s - 1) / s);
        most = reach > most ? reach : most;
    }
    if ((long long)B * most >= CV_MAX_ELEMS) return GOPS_ERR_UNSUPPORTED;
    return GOPS_OK;
}

struct ConvPlan {
    int n;
    ConvDev layer[GOPS_CONV_MAX_LAYERS];
    float* dzbuf[GOPS_CONV_MAX_LAYERS];   // dZ of layer l, channels-last
    float* feat;                          // the workspace's copy of the features: relu' of the last layer
    int F;
    size_t bytes;
};

// the device description of a checked stack: geometry, slices and - with a workspace - the stash, dZ and slot sections
static ConvPlan conv_plan(const GopsConv& d, int B, void* ws) {
    ConvPlan pl = {};
    pl.n = d.n_conv;
    char* base = static_cast<char*>(ws);
    size_t off = 0;
    auto section = [&](size_t floats) {
        float* at = base ? reinterpret_cast<float*>(base + off) : nullptr;
        off += align256(floats * sizeof(float));
        return at;
    };
    int C = d.in_channels, H = d.in_h, W = d.in_w;
    for (int l = 0; l < d.n_conv; ++l) {
        ConvDev& p = pl.layer[l];
        p.B = B; p.C = C; p.H = H; p.W = W;
        p.N = d.channels[l]; p.ks = d.kernel[l]; p.st = d.stride[l];
        p.Ho = (H - p.ks) / p.st + 1; p.Wo = (W - p.ks) / p.st + 1;
        p.K = C * p.ks * p.ks; p.M = B * p.Ho * p.Wo;
        p.out_nchw = l == d.n_conv - 1;
        p.w = d.weight[l]; p.bias = d.bias[l];
        // slices of M: at least CV_SLICE_ROWS pixels each, at most CV_MAX_SLICES, their slots within CV_SLOT_BUDGET
        p.P = p.N * p.K + p.N;
        int S = (p.M + CV_SLICE_ROWS - 1) / CV_SLICE_ROWS;
        const int fit = (int)(CV_SLOT_BUDGET / ((size_t)p.P * sizeof(float)));
        S = S > CV_MAX_SLICES ? CV_MAX_SLICES : S;
        S = S > fit ? fit : S;
        S = S < 1 ? 1 : S;
        p.rows = ((p.M + S - 1) / S + CV_WM - 1) / CV_WM * CV_WM;
        p.S = (p.M + p.rows - 1) / p.rows;   // (no empty slice)
        const size_t out = (size_t)p.M * p.N;
        p.dst = section(out);                // inner layers: the channels-last stash; the last: the copy of the features
        pl.dzbuf[l] = section(out);
        p.slots = section((size_t)p.S * p.P);
        C = p.N; H = p.Ho; W = p.Wo;
    }
    pl.F = C * H * W;
    pl.feat = pl.layer[d.n_conv - 1].dst;
    pl.bytes = off;
    return pl;
}

template <int MODE>
static void conv_launch_fwd(const ConvDev& p, hipStream_t s) {
    const dim3 grid((p.M + CV_TM - 1) / CV_TM, (p.N + CV_TN - 1) / CV_TN);
    if constexpr (MODE == CV_NHWC) {
        if (p.C % 4 == 0) {   // four consecutive k of a tap: one 16-byte load
            hipLaunchKernelGGL((conv_fwd_kernel<MODE, true>), grid, dim3(NTHREADS), 0, s, p);
            return;
        }
    }
    hipLaunchKernelGGL((conv_fwd_kernel<MODE, false>), grid, dim3(NTHREADS), 0, s, p);
}
template <int MODE>
static void conv_launch_wgrad(const ConvDev& p, hipStream_t s) {
    const dim3 grid((p.N + CV_WT - 1) / CV_WT, (p.K + CV_WT - 1) / CV_WT, p.S);
    if constexpr (MODE == CV_NHWC) {
        if (p.C % 4 == 0) {   // four consecutive k of a tap: one 16-byte load
            hipLaunchKernelGGL((conv_wgrad_kernel<MODE, true>), grid, dim3(NTHREADS), 0, s, p);
            return;
        }
    }
    hipLaunchKernelGGL((conv_wgrad_kernel<MODE, false>), grid, dim3(NTHREADS), 0, s, p);
}

extern "C" {

size_t gops_conv_workspace_bytes(const GopsConv* net, int32_t B) {
    if (!net || conv_check(*net, B) != GOPS_OK) return 0;
    return conv_plan(*net, B, nullptr).bytes;
}

int gops_conv_forward(const GopsConv* net, int32_t B, const float* x, float* features, void* ws, size_t bytes, void* stream) {
    if (net == nullptr) return GOPS_ERR_BAD_ARG;
    const int rc = conv_check(*net, B);
    if (rc != GOPS_OK) return rc;
    if (x == nullptr || features == nullptr) return GOPS_ERR_BAD_ARG;
    if (ws == nullptr || bytes < conv_plan(*net, B, nullptr).bytes) return GOPS_ERR_WORKSPACE;
    ConvPlan pl = conv_plan(*net, B, ws);
    hipStream_t s = static_cast<hipStream_t>(stream);
    for (int l = 0; l < pl.n; ++l) {
        ConvDev& p = pl.layer[l];
        p.src = l == 0 ? x : pl.layer[l - 1].dst;
        if (p.out_nchw) { p.dst2 = p.dst; p.dst = features; }
        if (l == 0) conv_launch_fwd<CV_NCHW>(p, s);
        else conv_launch_fwd<CV_NHWC>(p, s);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? GOPS_OK : (int)e;
}

int gops_conv_backward(const GopsConv* net, int32_t B, const float* x, const float* grad_a, const float* grad_b, const GopsConvGrad* grad,
                       void* ws, size_t bytes, void* stream) {
    if (net == nullptr || grad == nullptr) return GOPS_ERR_BAD_ARG;
    const int rc = conv_check(*net, B);
    if (rc != GOPS_OK) return rc;
    if (x == nullptr || grad_a == nullptr) return GOPS_ERR_BAD_ARG;
    for (int l = 0; l < net->n_conv; ++l)
        if (!grad->weight[l] || !grad->bias[l]) return GOPS_ERR_BAD_ARG;
    if (ws == nullptr || bytes < conv_plan(*net, B, nullptr).bytes) return GOPS_ERR_WORKSPACE;
    ConvPlan pl = conv_plan(*net, B, ws);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int n = pl.n;
    {
        const ConvDev& p = pl.layer[n - 1];
        const int total = p.M * p.N;
        hipLaunchKernelGGL(conv_seed_kernel, dim3((total + NTHREADS - 1) / NTHREADS), dim3(NTHREADS), 0, s, pl.feat, grad_a, grad_b,
                           pl.dzbuf[n - 1], p.N, p.Ho * p.Wo, total);
    }
    ConvReduce red = {};
    red.n = n;
    int maxP = 0;
    for (int l = n - 1; l >= 0; --l) {
        ConvDev& p = pl.layer[l];
        p.src = l == 0 ? x : pl.layer[l - 1].dst;
        p.dz = pl.dzbuf[l];
        if (l == 0) conv_launch_wgrad<CV_NCHW>(p, s);
        else conv_launch_wgrad<CV_NHWC>(p, s);
        red.S[l] = p.S; red.P[l] = p.P; red.NK[l] = p.N * p.K;
        red.slots[l] = p.slots; red.dw[l] = grad->weight[l]; red.db[l] = grad->bias[l];
        maxP = p.P > maxP ? p.P : maxP;
        if (l > 0) {   // dZ of layer l - 1 from dZ of layer l (layer 0's input is the observation: no gradient)
            p.act = pl.layer[l - 1].dst; p.dzo = pl.dzbuf[l - 1];
            const int mp = B * ((p.H + p.st - 1) / p.st) * ((p.W + p.st - 1) / p.st);   // phase (0, 0), the largest
            const dim3 grid((mp + CV_TM - 1) / CV_TM, (p.C + CV_TN - 1) / CV_TN, p.st * p.st);
            if (p.N % 4 == 0)
                hipLaunchKernelGGL(conv_dgrad_kernel<true>, grid, dim3(NTHREADS), 0, s, p);
            else
                hipLaunchKernelGGL(conv_dgrad_kernel<false>, grid, dim3(NTHREADS), 0, s, p);
        }
    }
    hipLaunchKernelGGL(conv_reduce_kernel, dim3((maxP + NTHREADS - 1) / NTHREADS, n), dim3(NTHREADS), 0, s, red);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? GOPS_OK : (int)e;
}

}  // extern "C"
