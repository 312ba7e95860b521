// RPI with an MLP value function (gops/algorithm/rpi.py:174-197, sample() :289-327): the whole policy evaluation of one
// local_update in ONE launch of ONE workgroup, the contract of rpi_evaluate_kernel (rollout_rpi.hip) with the value net
// S -> H1 [-> H2] -> 1 (linear output) in place of the degree-2 polynomial.
//
// 256 threads walk the batch in tiles of 64 rows.  In the row stages thread (r, g) = (tid & 63, tid >> 6) owns row r of the tile
// and the 16 units 16 g .. 16 g + 15 of a layer; in the weight-gradient stages thread (k, g) owns the 16 elements
// W2[16 g .. 16 g + 15][k].  All products are fp32 fmaf chains over LDS operands, every sum has a fixed order (k ascending, rows
// ascending, tiles ascending; the wave butterfly for row sums), there are no float atomics: results are bitwise reproducible.
//
// Per gradient step and tile:
//   target net:  plain forward and reverse at the lanes' states x -> dV/dx -> raw and wrapped action / adversary pair, the bare
//                Euler step, the flags, f(x, u', w') and U(x, u', w') (wave 0, one lane per row), the reset select;
//   value net:   forward with the tangent along f (a'_l = act'(z_l) z'_l), h = U + W_L a'_{L-1}; reverse over that pass with the
//                seed sign(h) / B: adj z'_l = p_l act'(z_l), adj z_l = p_l act''(z_l) z'_l + q_l act'(z_l),
//                dW_l += adj z_l a_{l-1}' + adj z'_l a'_{l-1}', db_l += adj z_l (the output bias has no gradient);
// then Adam on every weight and hidden bias (RpiAdam of rpi_env.h, as rpi_evaluate_kernel; each parameter has ONE owning thread that keeps
// its moments in registers and its value in LDS), the held-out mean|h| with the new weights (forward-tangent pass only; the
// held-out f and U under the target's pair are evaluated once before the loop), and the 0.88 test.  The loss and the norm are
// summed by thread 0 in tile order and read back by every thread from LDS after a barrier, so all threads take the same decision
// from the same bits: no barrier sits under divergent control flow.  The trip count is bounded by max_steps.
//
// Per-row state in global memory (lane states, counters, the held-out f and U) is only ever touched by lane r of wave 0, so
// program order keeps it coherent.
//
// LDS (one dynamic array, RPI_MLP_LDS_BYTES = 143 488 bytes of the 160 KiB = 163 840 a workgroup may declare):
//   value and target net, zero-padded to 64 x 64 (W1 [64][4], b1, W2 [64][64], b2, W_L)   2 x 4 544 floats   36 352 B
//   layer 1 of the tile: a_1, a'_1, act'(z_1), act''(z_1) z'_1, [unit][row] at stride 65   4 x 4 160 floats   66 560 B
//   layer 2 adjoints adj z_2, adj z'_2, [unit][row] at stride 64                           2 x 4 096 floats   32 768 B
//   x, f [4][64], U, seed [64], partial sums [4][4][64], db_2, dW_L [64], 4 scalars                 2 052 floats    8 208 B
#include "common.h"
#include "rpi_env.h"

namespace {

constexpr int RM_NT = 256, RM_LDA = 65;
constexpr int N_W1 = 0, N_B1 = 256, N_W2 = 320, N_B2 = N_W2 + 4096, N_WL = N_B2 + 64, N_FLOATS = N_WL + 64;   // one net in LDS
constexpr int L_V = 0, L_T = N_FLOATS, L_A1 = 2 * N_FLOATS, L_AP1 = L_A1 + 64 * RM_LDA, L_D1 = L_AP1 + 64 * RM_LDA,
              L_E1 = L_D1 + 64 * RM_LDA, L_G2 = L_E1 + 64 * RM_LDA, L_GP2 = L_G2 + 4096, L_X = L_GP2 + 4096, L_F = L_X + 256,
              L_U = L_F + 256, L_SEED = L_U + 64, L_PART = L_SEED + 64, L_GB2 = L_PART + 1024, L_GWL = L_GB2 + 64, L_RED = L_GWL + 64,
              L_TOTAL = L_RED + 4;
constexpr size_t RPI_MLP_LDS_BYTES = sizeof(float) * L_TOTAL;
static_assert(RPI_MLP_LDS_BYTES <= 160 * 1024, "LDS budget of one workgroup");
static_assert(L_T % 4 == 0 && N_W2 % 4 == 0 && L_G2 % 4 == 0 && L_GP2 % 4 == 0, "16-byte LDS reads");

struct RpiMlpParams {
    float c[GOPS_RPI_CONST_COUNT];
    int B, max_steps, H1, H2;
    float* vw[3];            // value net, stepped in place: weights of the Linear layers ...
    float* vb[3];            // ... and their biases
    const float* tw[3];      // target net
    const float* tb[3];
    const float* max_step;   // [B] time limit of each lane
    const float* pool;       // [max_steps + 1][S][B]: held-out set, then one reset draw per step
    float* state;            // the state block (gops_hip.h)
    float* result;           // [4]
    float* trace;            // [max_steps][2] or nullptr
    double lr, beta1, beta2, eps;
};

__device__ __forceinline__ float4 lds4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// one net from global memory into its zero-padded LDS image (the caller has zeroed it)
template <int S, int NH>
__device__ __forceinline__ void rpi_mlp_stage_net(float* N, const float* const* w, const float* const* b, int H1, int H2, int tid) {
    for (int i = tid; i < H1 * S; i += RM_NT) N[N_W1 + (i / S) * 4 + i % S] = w[0][i];
    for (int i = tid; i < H1; i += RM_NT) N[N_B1 + i] = b[0][i];
    if constexpr (NH == 2) {
        for (int i = tid; i < H2 * H1; i += RM_NT) N[N_W2 + (i / H1) * 64 + i % H1] = w[1][i];
        for (int i = tid; i < H2; i += RM_NT) { N[N_B2 + i] = b[1][i]; N[N_WL + i] = w[2][i]; }
    } else {
        for (int i = tid; i < H1; i += RM_NT) N[N_WL + i] = w[1][i];
    }
}

template <int KIND, int NH, int ACT>
__global__ __launch_bounds__(RM_NT) void rpi_mlp_evaluate_kernel(const RpiMlpParams p) {
    constexpr int S = rpi_state_dim(KIND);
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* const NV = lds + L_V;
    float* const NT = lds + L_T;
    float* const A1 = lds + L_A1;
    float* const AP1 = lds + L_AP1;
    float* const D1 = lds + L_D1;
    float* const E1 = lds + L_E1;
    float* const G2 = lds + L_G2;
    float* const GP2 = lds + L_GP2;
    float* const X = lds + L_X;
    float* const F = lds + L_F;
    float* const U = lds + L_U;
    float* const SEED = lds + L_SEED;
    float* const PART = lds + L_PART;
    float* const GB2 = lds + L_GB2;
    float* const GWL = lds + L_GWL;
    float* const RED = lds + L_RED;

    const float* c = p.c;
    const int tid = threadIdx.x, r = tid & 63, g = tid >> 6;
    const int B = p.B, H1 = p.H1, H2 = NH == 2 ? p.H2 : 0;
    const int ng1 = H1 >> 4, ng2 = H2 >> 4, ngl = NH == 2 ? ng2 : ng1;   // 16-unit groups of layer 1, layer 2, the last hidden layer
    const int ntiles = (B + 63) >> 6;
    const float Bf = (float)B;
    // parameters() order of the moments in the state block: W1, b1, [W2, b2,] W_L, b_L
    const int oW1 = 0, ob1 = H1 * S, oW2 = ob1 + H1, ob2 = oW2 + H2 * H1, oWL = NH == 2 ? ob2 + H2 : oW2;
    const int P = oWL + (NH == 2 ? H2 : H1) + 1;
    float* hdr = p.state;
    float* st_x = p.state + GOPS_RPI_STATE_HEADER;
    float* st_cnt = st_x + (size_t)S * B;
    float* st_shown = st_cnt + B;
    float* st_m = st_shown + B;
    float* st_v = st_m + P;
    float* st_fs = st_v + P;                 // [S][B] held-out f under the target's pair
    float* st_us = st_fs + (size_t)S * B;    // [B] held-out U

    for (int i = tid; i < L_TOTAL; i += RM_NT) lds[i] = 0.f;
    __syncthreads();
    rpi_mlp_stage_net<S, NH>(NV, p.vw, p.vb, H1, H2, tid);
    rpi_mlp_stage_net<S, NH>(NT, p.tw, p.tb, H1, H2, tid);

    // ---- the parameters this thread owns, their moments and gradient sums ----
    const bool own2 = NH == 2 && g < ng2 && r < H1;   // W2[16 g + i][r], i < 16
    const bool own1 = g < S && r < H1;                // W1[r][g]
    const bool ownb1 = g == 0 && r < H1;              // b1[r]
    const bool ownb2 = NH == 2 && g == 0 && r < H2;   // b2[r]
    const bool ownl = g == 0 && r < (NH == 2 ? H2 : H1);   // W_L[r]
    float m2[16], v2[16], acc2[16];
    float m1 = 0.f, v1 = 0.f, acc1 = 0.f, mb1 = 0.f, vb1 = 0.f, accb1 = 0.f, mb2 = 0.f, vb2 = 0.f, ml = 0.f, vl = 0.f, accl = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int o = oW2 + (16 * g + i) * H1 + r;
        m2[i] = own2 ? st_m[o] : 0.f;
        v2[i] = own2 ? st_v[o] : 0.f;
        acc2[i] = 0.f;
    }
    if (own1) { m1 = st_m[oW1 + r * S + g]; v1 = st_v[oW1 + r * S + g]; }
    if (ownb1) { mb1 = st_m[ob1 + r]; vb1 = st_v[ob1 + r]; }
    if (ownb2) { mb2 = st_m[ob2 + r]; vb2 = st_v[ob2 + r]; }
    if (ownl) { ml = st_m[oWL + r]; vl = st_v[oWL + r]; }
    // The Adam step count and the lanes' counters are floats in the state block, as in rpi_evaluate_kernel (exact up to 2^24).
    float tcount = hdr[0];
    RpiAdam adam(p.lr, p.beta1, p.beta2, p.eps, tcount);
    __syncthreads();

    // ---- stages of one tile ----
    float d1r[16], er[16], apr[16];   // the last hidden layer's act', act'' z' and a' of this thread's row and units

    // layer 1 of net N at (X, F): a_1, act' into the tile arrays, with TAN also a'_1 and act'' z'_1
    auto layer1 = [&](const float* N, auto tan) {
        constexpr bool TAN = decltype(tan)::value;
        if (g < ng1) {
            float x[S], f[S];
#pragma unroll
            for (int m = 0; m < S; ++m) { x[m] = X[m * 64 + r]; f[m] = F[m * 64 + r]; }
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int j = 16 * g + i;
                float z = N[N_B1 + j], zp = 0.f;
#pragma unroll
                for (int m = 0; m < S; ++m) {
                    const float w = N[N_W1 + j * 4 + m];
                    z = fmaf(w, x[m], z);
                    if (TAN) zp = fmaf(w, f[m], zp);
                }
                float a, d1, d2;
                act3_t<ACT>(z, a, d1, d2);
                A1[j * RM_LDA + r] = a;
                D1[j * RM_LDA + r] = d1;
                if (TAN) { AP1[j * RM_LDA + r] = d1 * zp; E1[j * RM_LDA + r] = d2 * zp; }
                if (NH == 1) { d1r[i] = d1; er[i] = d2 * zp; apr[i] = d1 * zp; }
            }
        }
    };
    // layer 2 of net N from the tile arrays into d1r (and, with TAN, er and apr)
    auto layer2 = [&](const float* N, auto tan) {
        constexpr bool TAN = decltype(tan)::value;
        if (g < ng2) {
            float z[16], zp[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) { z[i] = N[N_B2 + 16 * g + i]; zp[i] = 0.f; }
            for (int k = 0; k < H1; k += 4) {
                float a[4], ap[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) { a[q] = A1[(k + q) * RM_LDA + r]; ap[q] = TAN ? AP1[(k + q) * RM_LDA + r] : 0.f; }
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float4 w = lds4(N + N_W2 + (16 * g + i) * 64 + k);
                    z[i] = fmaf(w.w, a[3], fmaf(w.z, a[2], fmaf(w.y, a[1], fmaf(w.x, a[0], z[i]))));
                    if (TAN) zp[i] = fmaf(w.w, ap[3], fmaf(w.z, ap[2], fmaf(w.y, ap[1], fmaf(w.x, ap[0], zp[i]))));
                }
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                float a, d1, d2;
                act3_t<ACT>(z[i], a, d1, d2);
                d1r[i] = d1; er[i] = d2 * zp[i]; apr[i] = d1 * zp[i];
            }
        }
    };
    // dV/dx of the TARGET net at X: ends with the per-group partial sums in PART [g][m][row] (read them after a barrier)
    auto target_gradient = [&]() {
        layer1(NT, std::false_type{});
        if constexpr (NH == 2) {
            __syncthreads();
            layer2(NT, std::false_type{});
            if (g < ng2) {
#pragma unroll
                for (int i = 0; i < 16; ++i) G2[(16 * g + i) * 64 + r] = NT[N_WL + 16 * g + i] * d1r[i];
            }
            __syncthreads();
        }
        if (g < ng1) {
            float az[16];
            if constexpr (NH == 2) {
#pragma unroll
                for (int i = 0; i < 16; ++i) az[i] = 0.f;
                for (int j = 0; j < H2; ++j) {
                    const float gj = G2[j * 64 + r];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float4 w = lds4(NT + N_W2 + j * 64 + 16 * g + 4 * q);
                        az[4 * q] = fmaf(w.x, gj, az[4 * q]); az[4 * q + 1] = fmaf(w.y, gj, az[4 * q + 1]);
                        az[4 * q + 2] = fmaf(w.z, gj, az[4 * q + 2]); az[4 * q + 3] = fmaf(w.w, gj, az[4 * q + 3]);
                    }
                }
#pragma unroll
                for (int i = 0; i < 16; ++i) az[i] *= D1[(16 * g + i) * RM_LDA + r];
            } else {
#pragma unroll
                for (int i = 0; i < 16; ++i) az[i] = NT[N_WL + 16 * g + i] * d1r[i];
            }
#pragma unroll
            for (int m = 0; m < S; ++m) {
                float s = 0.f;
#pragma unroll
                for (int i = 0; i < 16; ++i) s = fmaf(NT[N_W1 + (16 * g + i) * 4 + m], az[i], s);
                PART[(g * 4 + m) * 64 + r] = s;
            }
        }
    };
    auto read_gradient = [&](float* dv) {   // wave 0, after the barrier that follows target_gradient
#pragma unroll
        for (int m = 0; m < S; ++m) {
            float s = PART[m * 64 + r];
            for (int q = 1; q < ng1; ++q) s += PART[(q * 4 + m) * 64 + r];
            dv[m] = s;
        }
    };
    // h of the VALUE net at (X, F, U): the same value in the four threads of a row.  Leaves d1r / er / apr for the reverse pass.
    auto hamiltonian = [&]() -> float {
        layer1(NV, std::true_type{});
        if constexpr (NH == 2) {
            __syncthreads();
            layer2(NV, std::true_type{});
        }
        if (g < ngl) {
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) s = fmaf(NV[N_WL + 16 * g + i], apr[i], s);
            PART[g * 64 + r] = s;
        }
        __syncthreads();
        float s = PART[r];
        for (int q = 1; q < ngl; ++q) s += PART[q * 64 + r];
        return U[r] + s;
    };
    // wave 0: the sum over the tile's rows, added to thread 0's running sum
    auto add_rows = [&](float v, float& sum) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        sum += v;
    };

    // ---- held-out set: f and U under the target's wrapped pair once, and the norm before the first step ----
    float sum = 0.f;
    for (int t = 0; t < ntiles; ++t) {
        const int row = t * 64 + r;
        const bool valid = row < B;
        if (g == 0) {
#pragma unroll
            for (int m = 0; m < S; ++m) X[m * 64 + r] = valid ? p.pool[(size_t)m * B + row] : 0.f;
        }
        __syncthreads();
        target_gradient();
        __syncthreads();
        if (g == 0) {
            float x[S], dv[S], d[S], u, a, uw, aw;
#pragma unroll
            for (int m = 0; m < S; ++m) x[m] = X[m * 64 + r];
            read_gradient(dv);
            rpi_pair<KIND>(c, x, dv, u, a, uw, aw);
            rpi_derivative<KIND>(c, x, uw, aw, d);
            const float us = rpi_cost<S>(c, x, uw, aw);
#pragma unroll
            for (int m = 0; m < S; ++m) {
                F[m * 64 + r] = valid ? d[m] : 0.f;
                if (valid) st_fs[(size_t)m * B + row] = d[m];
            }
            U[r] = valid ? us : 0.f;
            if (valid) st_us[row] = us;
        }
        __syncthreads();
        const float h = hamiltonian();
        if (g == 0) add_rows(valid ? fabsf(h) : 0.f, sum);
        __syncthreads();
    }
    if (tid == 0) RED[0] = sum / Bf;
    __syncthreads();
    const float before = RED[0];
    float after = before, loss = 0.f;
    int steps = 0;

#pragma unroll 1
    for (int it = 0; it < p.max_steps; ++it) {
        sum = 0.f;
#pragma unroll 1
        for (int t = 0; t < ntiles; ++t) {
            const int row = t * 64 + r;
            const bool valid = row < B;
            if (g == 0) {
#pragma unroll
                for (int m = 0; m < S; ++m) X[m * 64 + r] = valid ? st_x[(size_t)m * B + row] : 0.f;
            }
            __syncthreads();
            target_gradient();
            __syncthreads();
            if (g == 0) {
                // sample(): the target's pair, the bare step with the raw values, the flags, the reset select (rpi.py:315-325)
                float x[S], dv[S], d[S], xn[S], u, a, uw, aw;
#pragma unroll
                for (int m = 0; m < S; ++m) x[m] = X[m * 64 + r];
                read_gradient(dv);
                rpi_pair<KIND>(c, x, dv, u, a, uw, aw);
                rpi_derivative<KIND>(c, x, u, a, d);
                bool reset = false;
#pragma unroll
                for (int m = 0; m < S; ++m) {
                    xn[m] = x[m] + d[m] * c[GOPS_RPI_C_DT];
                    reset = reset || fabsf(xn[m]) > c[GOPS_RPI_C_THRESHOLD + m];
                }
                // the Hamiltonian's f and U at the pre-step state under the wrapped pair
                rpi_derivative<KIND>(c, x, uw, aw, d);
                const float us = rpi_cost<S>(c, x, uw, aw);
#pragma unroll
                for (int m = 0; m < S; ++m) F[m * 64 + r] = valid ? d[m] : 0.f;
                U[r] = valid ? us : 0.f;
                if (valid) {
                    const float cnt = st_cnt[row] + 1.f, shown = st_shown[row];
                    reset = reset || cnt > p.max_step[row];
                    const float prev = shown < 0.f ? cnt : shown;   // the first assignment reads the counter the step has just advanced
                    st_cnt[row] = cnt;
                    st_shown[row] = reset ? 0.f : prev;
#pragma unroll
                    for (int m = 0; m < S; ++m) st_x[(size_t)m * B + row] = reset ? p.pool[((size_t)(it + 1) * S + m) * B + row] : xn[m];
                }
            }
            __syncthreads();
            const float h = hamiltonian();
            const float seed = !valid ? 0.f : h > 0.f ? 1.f / Bf : h < 0.f ? -1.f / Bf : 0.f;
            if (g == 0) {
                add_rows(valid ? fabsf(h) : 0.f, sum);
                SEED[r] = seed;
            }
            // reverse: the last hidden layer's adjoints from the seed
            if constexpr (NH == 2) {
                if (g < ng2) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int j = 16 * g + i;
                        const float pj = seed * NV[N_WL + j];
                        GP2[j * 64 + r] = pj * d1r[i];
                        G2[j * 64 + r] = pj * er[i];
                        float s = seed * apr[i];
#pragma unroll
                        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
                        if (r == 0) GWL[j] += s;
                    }
                }
                __syncthreads();
                // dW2 and db2 of this tile (thread (k, g)), then the adjoints of layer 1 (thread (row, g))
                if (g < ng2) {
                    float bs[16];
#pragma unroll
                    for (int i = 0; i < 16; ++i) bs[i] = 0.f;
                    for (int r4 = 0; r4 < 64; r4 += 4) {
                        float a[4], ap[4];
#pragma unroll
                        for (int q = 0; q < 4; ++q) { a[q] = A1[r * RM_LDA + r4 + q]; ap[q] = AP1[r * RM_LDA + r4 + q]; }
#pragma unroll
                        for (int i = 0; i < 16; ++i) {
                            const float4 gz = lds4(G2 + (16 * g + i) * 64 + r4), gp = lds4(GP2 + (16 * g + i) * 64 + r4);
                            float s = acc2[i];
                            s = fmaf(gp.x, ap[0], fmaf(gz.x, a[0], s));
                            s = fmaf(gp.y, ap[1], fmaf(gz.y, a[1], s));
                            s = fmaf(gp.z, ap[2], fmaf(gz.z, a[2], s));
                            s = fmaf(gp.w, ap[3], fmaf(gz.w, a[3], s));
                            acc2[i] = s;
                            bs[i] = (((bs[i] + gz.x) + gz.y) + gz.z) + gz.w;
                        }
                    }
                    if (r == 0) {
#pragma unroll
                        for (int i = 0; i < 16; ++i) GB2[16 * g + i] += bs[i];
                    }
                }
                if (g < ng1) {
                    float q1[16], p1[16];
#pragma unroll
                    for (int i = 0; i < 16; ++i) { q1[i] = 0.f; p1[i] = 0.f; }
                    for (int j = 0; j < H2; ++j) {
                        const float gj = G2[j * 64 + r], gpj = GP2[j * 64 + r];
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const float4 w = lds4(NV + N_W2 + j * 64 + 16 * g + 4 * q);
                            q1[4 * q] = fmaf(w.x, gj, q1[4 * q]); q1[4 * q + 1] = fmaf(w.y, gj, q1[4 * q + 1]);
                            q1[4 * q + 2] = fmaf(w.z, gj, q1[4 * q + 2]); q1[4 * q + 3] = fmaf(w.w, gj, q1[4 * q + 3]);
                            p1[4 * q] = fmaf(w.x, gpj, p1[4 * q]); p1[4 * q + 1] = fmaf(w.y, gpj, p1[4 * q + 1]);
                            p1[4 * q + 2] = fmaf(w.z, gpj, p1[4 * q + 2]); p1[4 * q + 3] = fmaf(w.w, gpj, p1[4 * q + 3]);
                        }
                    }
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int o = (16 * g + i) * RM_LDA + r;
                        const float d1 = D1[o], e = E1[o];
                        D1[o] = fmaf(p1[i], e, q1[i] * d1);   // adj z_1
                        E1[o] = p1[i] * d1;                   // adj z'_1
                    }
                }
            } else {
                if (g < ng1) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int o = (16 * g + i) * RM_LDA + r;
                        const float pk = seed * NV[N_WL + 16 * g + i];
                        D1[o] = pk * er[i];
                        E1[o] = pk * d1r[i];
                    }
                }
            }
            __syncthreads();
            // dW1[k][m] (thread (k, m)), db1[k] and, with one hidden layer, dW_L[k] (thread (k, 0))
            if (g < S) {
                float s = acc1, sb = accb1, sl = accl;
                for (int rr = 0; rr < 64; ++rr) {
                    const float gz = D1[r * RM_LDA + rr], gp = E1[r * RM_LDA + rr];
                    s = fmaf(gp, F[g * 64 + rr], fmaf(gz, X[g * 64 + rr], s));
                    if (g == 0) {
                        sb += gz;
                        if (NH == 1) sl = fmaf(SEED[rr], AP1[r * RM_LDA + rr], sl);
                    }
                }
                acc1 = s, accb1 = sb, accl = sl;
            }
            __syncthreads();
        }
        if (tid == 0) RED[1] = sum / Bf;

        // Adam, by the owners
        tcount += 1.f;
        adam.advance();
        if (own2) {
#pragma unroll
            for (int i = 0; i < 16; ++i) { adam.update(NV[N_W2 + (16 * g + i) * 64 + r], m2[i], v2[i], acc2[i]); acc2[i] = 0.f; }
        }
        if (own1) adam.update(NV[N_W1 + r * 4 + g], m1, v1, acc1);
        if (ownb1) adam.update(NV[N_B1 + r], mb1, vb1, accb1);
        if (ownb2) adam.update(NV[N_B2 + r], mb2, vb2, GB2[r]);
        if (ownl) adam.update(NV[N_WL + r], ml, vl, NH == 2 ? GWL[r] : accl);
        acc1 = 0.f, accb1 = 0.f, accl = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc2[i] = 0.f;
        if (g == 0) { GB2[r] = 0.f; GWL[r] = 0.f; }
        __syncthreads();
        loss = RED[1];

        // held-out norm with the new weights
        sum = 0.f;
#pragma unroll 1
        for (int t = 0; t < ntiles; ++t) {
            const int row = t * 64 + r;
            const bool valid = row < B;
            if (g == 0) {
#pragma unroll
                for (int m = 0; m < S; ++m) {
                    X[m * 64 + r] = valid ? p.pool[(size_t)m * B + row] : 0.f;
                    F[m * 64 + r] = valid ? st_fs[(size_t)m * B + row] : 0.f;
                }
                U[r] = valid ? st_us[row] : 0.f;
            }
            __syncthreads();
            const float h = hamiltonian();
            if (g == 0) add_rows(valid ? fabsf(h) : 0.f, sum);
            __syncthreads();
        }
        if (tid == 0) RED[2] = sum / Bf;
        __syncthreads();
        after = RED[2];
        steps = it + 1;
        if (p.trace != nullptr && tid == 0) { p.trace[2 * (size_t)it] = loss; p.trace[2 * (size_t)it + 1] = after; }
        // continue_evaluation (rpi.py:164-168): every thread has read the same two floats, so the branch is uniform
        if (!(fabs((double)after) > 0.88 * fabs((double)before))) break;
    }

    // ---- the stepped parameters and their moments, each by its owner ----
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        if (own2) {
            const int o = (16 * g + i) * H1 + r;
            p.vw[1][o] = NV[N_W2 + (16 * g + i) * 64 + r];
            st_m[oW2 + o] = m2[i];
            st_v[oW2 + o] = v2[i];
        }
    }
    if (own1) { p.vw[0][r * S + g] = NV[N_W1 + r * 4 + g]; st_m[oW1 + r * S + g] = m1; st_v[oW1 + r * S + g] = v1; }
    if (ownb1) { p.vb[0][r] = NV[N_B1 + r]; st_m[ob1 + r] = mb1; st_v[ob1 + r] = vb1; }
    if (ownb2) { p.vb[1][r] = NV[N_B2 + r]; st_m[ob2 + r] = mb2; st_v[ob2 + r] = vb2; }
    if (ownl) { p.vw[NH][r] = NV[N_WL + r]; st_m[oWL + r] = ml; st_v[oWL + r] = vl; }
    if (tid == 0) {
        hdr[0] = tcount;
        p.result[0] = (float)steps, p.result[1] = loss, p.result[2] = before, p.result[3] = after;
    }
}

// 0 = unsupported; otherwise the number of hidden layers
int rpi_mlp_hidden_layers(int kind, int B, const GopsMlp* v) {
    const int S = rpi_state_dim(kind);
    if (S == 0 || !v || B > GOPS_RPI_MAX_BATCH) return 0;
    const int nh = v->n_layers - 1;
    if (nh < 1 || nh > 2 || v->sizes[0] != S || v->sizes[nh + 1] != 1 || v->dtype != GOPS_DTYPE_F32) return 0;
    for (int l = 1; l <= nh; ++l)
        if (v->sizes[l] < 16 || v->sizes[l] > 64 || v->sizes[l] % 16) return 0;
    const int a = v->hidden_act;
    if (a != GOPS_ACT_ELU && a != GOPS_ACT_GELU && a != GOPS_ACT_TANH && a != GOPS_ACT_SIGMOID) return 0;
    return nh;
}

size_t rpi_mlp_param_count(const GopsMlp& v) {
    size_t n = 0;
    for (int l = 0; l < v.n_layers; ++l) n += (size_t)v.sizes[l + 1] * (v.sizes[l] + 1);
    return n;
}

template <int KIND, int NH>
void rpi_mlp_launch_act(int act, const RpiMlpParams& p, hipStream_t s) {
    const dim3 grid(1), block(RM_NT);
    switch (act) {
        case GOPS_ACT_ELU: launch_with_lds(rpi_mlp_evaluate_kernel<KIND, NH, GOPS_ACT_ELU>, grid, block, RPI_MLP_LDS_BYTES, s, p); break;
        case GOPS_ACT_GELU: launch_with_lds(rpi_mlp_evaluate_kernel<KIND, NH, GOPS_ACT_GELU>, grid, block, RPI_MLP_LDS_BYTES, s, p); break;
        case GOPS_ACT_TANH: launch_with_lds(rpi_mlp_evaluate_kernel<KIND, NH, GOPS_ACT_TANH>, grid, block, RPI_MLP_LDS_BYTES, s, p); break;
        default: launch_with_lds(rpi_mlp_evaluate_kernel<KIND, NH, GOPS_ACT_SIGMOID>, grid, block, RPI_MLP_LDS_BYTES, s, p); break;
    }
}

template <int KIND>
void rpi_mlp_launch(int nh, int act, const RpiMlpParams& p, hipStream_t s) {
    if (nh == 1) rpi_mlp_launch_act<KIND, 1>(act, p, s);
    else rpi_mlp_launch_act<KIND, 2>(act, p, s);
}

}  // namespace

extern "C" {

size_t gops_rpi_mlp_state_bytes(int32_t kind, int32_t B, const GopsMlp* v) {
    if (B < 1 || rpi_mlp_hidden_layers(kind, B, v) == 0) return 0;
    const int S = rpi_state_dim(kind);
    return sizeof(float) * ((size_t)GOPS_RPI_STATE_HEADER + (size_t)(S + 2) * B + 2 * rpi_mlp_param_count(*v) + (size_t)(S + 1) * B);
}

int gops_rpi_mlp_evaluate(int32_t kind, int32_t B, int32_t max_steps, const float* consts, const GopsMlp* v, const GopsMlp* t,
                          const float* max_step, const float* pool, void* state, size_t state_bytes, double lr, double beta1, double beta2,
                          double eps, float* result, float* trace, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!v || !t) return GOPS_ERR_BAD_ARG;
    const int nh = rpi_mlp_hidden_layers(kind, B, v);
    if (nh == 0 || rpi_mlp_hidden_layers(kind, B, t) != nh || v->hidden_act != t->hidden_act) return GOPS_ERR_UNSUPPORTED;
    for (int l = 1; l <= nh; ++l)
        if (v->sizes[l] != t->sizes[l]) return GOPS_ERR_UNSUPPORTED;
    if (B < 1 || max_steps < 1 || max_steps > GOPS_RPI_MAX_STEPS) return GOPS_ERR_BAD_ARG;
    if (!consts || !max_step || !pool || !state || !result) return GOPS_ERR_BAD_ARG;
    for (int l = 0; l <= nh; ++l)
        if (!v->weight[l] || !v->bias[l] || !t->weight[l] || !t->bias[l]) return GOPS_ERR_BAD_ARG;
    if (state_bytes < gops_rpi_mlp_state_bytes(kind, B, v)) return GOPS_ERR_WORKSPACE;
    RpiMlpParams p;
    for (int i = 0; i < GOPS_RPI_CONST_COUNT; ++i) p.c[i] = consts[i];
    p.B = B, p.max_steps = max_steps, p.H1 = v->sizes[1], p.H2 = nh == 2 ? v->sizes[2] : 0;
    for (int l = 0; l < 3; ++l) {
        const bool on = l <= nh;
        p.vw[l] = on ? const_cast<float*>(v->weight[l]) : nullptr;
        p.vb[l] = on ? const_cast<float*>(v->bias[l]) : nullptr;
        p.tw[l] = on ? t->weight[l] : nullptr;
        p.tb[l] = on ? t->bias[l] : nullptr;
    }
    p.max_step = max_step, p.pool = pool, p.state = static_cast<float*>(state), p.result = result, p.trace = trace;
    p.lr = lr, p.beta1 = beta1, p.beta2 = beta2, p.eps = eps;
    if (kind == GOPS_RPI_ENV_OSCILLATOR) rpi_mlp_launch<GOPS_RPI_ENV_OSCILLATOR>(nh, v->hidden_act, p, s);
    else if (kind == GOPS_RPI_ENV_AIRCRAFT) rpi_mlp_launch<GOPS_RPI_ENV_AIRCRAFT>(nh, v->hidden_act, p, s);
    else rpi_mlp_launch<GOPS_RPI_ENV_SUSPENSION>(nh, v->hidden_act, p, s);
    return (int)hipGetLastError();
}

}  // extern "C"
