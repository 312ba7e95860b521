// Closed loops on gym_cartpolecontiwithstack under a recurrent StochaPolicy (gops/apprfunc/rnn.py), each in ONE launch -
// include/gops_hip.h: gops_stack_sample_rollout (a whole sample() of T steps, as rollout_sample.hip is for an MLP) and
// gops_stack_episode_rollout (all episodes of an evaluation, as rollout_episode.hip).  The observation is the window of the last L
// states; the policy restarts its recurrence from h_0 = 0 on every env step, so an env step costs L recurrent steps.
//
// Mapping.  A workgroup of 256 threads owns 16 instances (the M of v_mfma_f32_16x16x4_f32) for all T steps.  The H hidden columns are
// cut into 16-wide blocks dealt round-robin to the four waves as in rnn.hip (NB = 1 up to H = 64, NB = 2 up to 128); a wave loads the
// B-operand fragments of its blocks of W_hh and W_ih and its summed bias ONCE per launch and keeps them in registers.
//   ring [L][16][H + 4] (LDS): the bare x chain W_ih x - no bias - of every row of the window.  A state enters the window once and
//     stays for L env steps, and W_ih x does not depend on its position, so an env step projects ONE row (one MFMA per block) into
//     the slot of the row that leaves.  Logical row j (0 = oldest) lives in slot (base + j) % L; `base` is uniform over the tile,
//     because every instance advances by one row per step and a reset writes the same projected row into all L slots.
//   win [L][16][4] (LDS): the states themselves, in the same slots - the source of the stored obs / next_obs rows.
//   Per env step:  L times "accumulators = ring row, MFMA chain over k = H against the register-resident W_hh (not at the first
//     row: h_0 = 0), bias, tanh, store to the other of two hidden tiles, barrier" - the floating-point order of gops_rnn_forward (x
//     chain from zero, h chain, bias), so the outputs are RnnNet's on the same stack, bit for bit; the heads on the same tile as in
//     rnn_fwd_kernel (weights streamed from L2 in torch layout), their outputs to LDS; one lane per instance forms the action (the
//     sampler: mean + exp(clamp(log std)) noise and its log-probability, in double, gauss_math.h; the evaluator: the mean clamped
//     to the policy's limits), steps the env on the newest row (env_models.h: cart_forward with cart_stack_const), keeps the books
//     and overwrites the oldest row of win; barrier; all threads store next_obs, the next step's obs (or the persistent state) and
//     apply the reset - one pass in which every element of win is read and written by one thread only - while the waves project the
//     new row into the ring; barrier.
// Instances beyond n_envs compute on zeros and store nothing.  A row depends on its own instance only; no atomics; every loop is
// bounded by `steps` and L <= GOPS_STACK_MAX_LEN.
// LDS bytes = 4 (L 16 (H + 4) + 3 16 (W + 4) + L 16 4 + 16 4 + 16 2 + 16), W = the largest of H and the heads' hidden widths:
// 95 424 at L = 8, H = W = 128 (above the 64-KiB default: launch_with_lds).
#include <stdint.h>
#include <string.h>

#include "env_models.h"
#include "common.h"
#include "rnn_tile.h"
#include "gauss_math.h"

namespace {

constexpr int STACK_OBS = 4;   // the cart-pole's state: the k of ONE v_mfma_f32_16x16x4_f32

struct StackHead {
    int nl, act;
    int dims[GOPS_MAX_LAYERS + 1];
    const float* w[GOPS_MAX_LAYERS];   // torch layout [dims[l + 1]][dims[l]]
    const float* b[GOPS_MAX_LAYERS];
};
struct StackNet {
    int L, H, ldw, ldr;                              // LDS leading dims of the hidden tiles / the ring (floats)
    int off_hb, off_win, off_xs, off_y, off_flags;   // float offsets into LDS (the ring is at 0)
    const float *wih, *whh, *bih, *bhh;
    StackHead head[2];                               // mean, raw log std
};
struct StackSampleParams {
    GopsEnv env;
    StackNet net;
    int N, T, R, max_steps;
    double min_ls, max_ls;
    GopsSampleState st;
    GopsSamplePool pool;
    const float* noise;
    GopsSampleOut out;
    float* books[4];   // out.rew, .done, .time_limited, .end
};
struct StackEpisodeParams {
    GopsEnv env;
    StackNet net;
    int E, T;
    const float* init;   // [E][STACK_OBS]
    GopsEpisodeOut out;
};
static_assert(sizeof(StackSampleParams) <= 4096 && sizeof(StackEpisodeParams) <= 4096, "kernel arguments are passed by value");

template <int NB>
struct StackRegs {   // the wave's blocks of W_hh and W_ih and the summed bias of its columns: resident for the whole launch
    f32x4 whh[4 * NB][NB];
    float wih[NB], bias[NB];
};

template <int NB>
__device__ __forceinline__ void stack_load_weights(const StackNet& p, StackRegs<NB>& w, int wave, int l15, int g) {
    const int H = p.H, nhb = H >> 4;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const int nt = wave + 4 * j, n = 16 * nt + l15;
        const bool ok = nt < nhb;
        w.bias[j] = ok ? gptr(p.bih)[n] + gptr(p.bhh)[n] : 0.f;
#pragma unroll
        for (int c = 0; c < 4 * NB; ++c) {
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            w.whh[c][j] = (ok && c < nhb) ? ld4(gptr(p.whh) + (size_t)n * H + 16 * c + 4 * g) : z;
        }
        w.wih[j] = ok ? gptr(p.wih)[(size_t)n * STACK_OBS + g] : 0.f;
    }
}

// ring <- the bare x chain of the tile's rows xs [16][4]: into `slot`, or - rows with all_slots[row] != 0: a reset - into all L slots
template <int NB>
__device__ __forceinline__ void stack_project(const StackNet& p, const StackRegs<NB>& w, const float* xs, float* ring, int slot,
                                              const int* all_slots, int wave, int l15, int g) {
    const int nhb = p.H >> 4, ldr = p.ldr;
    if (wave >= nhb) return;
    const float a = xs[l15 * STACK_OBS + g];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const int nt = wave + 4 * j, n = 16 * nt + l15;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        acc = mfma4(a, w.wih[j], acc);
        if (nt < nhb) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 4 * g + r;
                if (all_slots != nullptr && all_slots[row] != 0) {
                    for (int s = 0; s < p.L; ++s) ring[(s * TB + row) * ldr + n] = acc[r];
                } else {
                    ring[(slot * TB + row) * ldr + n] = acc[r];
                }
            }
        }
    }
}

// The recurrence over the window from h_0 = 0 -> h_L, in hidden tile (L & 1).  Ends with a barrier.
template <int NB>
__device__ __forceinline__ const float* stack_recur(const StackNet& p, const StackRegs<NB>& w, const float* ring, float* hb, int base,
                                                    int wave, int l15, int g) {
    const int L = p.L, nhb = p.H >> 4, ldw = p.ldw, ldr = p.ldr;
    for (int t = 0; t < L; ++t) {
        const int cur = t & 1;
        const float* hr = hb + cur * TB * ldw;   // h_t (t = 0: h_0 = 0, not read)
        float* hw = hb + (cur ^ 1) * TB * ldw;
        int slot = base + t;
        if (slot >= L) slot -= L;
        if (wave < nhb) {
            f32x4 acc[NB];
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                const int nt = wave + 4 * j, n = 16 * nt + l15;
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[j][r] = nt < nhb ? ring[(slot * TB + 4 * g + r) * ldr + n] : 0.f;
            }
            if (t > 0) {
#pragma unroll
                for (int c = 0; c < 4 * NB; ++c)
                    if (c < nhb) {
                        const f32x4 a = *reinterpret_cast<const f32x4*>(hr + l15 * ldw + 16 * c + 4 * g);
#pragma unroll
                        for (int i = 0; i < 4; ++i)
#pragma unroll
                            for (int j = 0; j < NB; ++j) acc[j] = mfma4(a[i], w.whh[c][j][i], acc[j]);
                    }
            }
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                const int nt = wave + 4 * j, n = 16 * nt + l15;
                if (nt < nhb) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) hw[(4 * g + r) * ldw + n] = tanhf(acc[j][r] + w.bias[j]);
                }
            }
        }
        __syncthreads();
    }
    return hb + (L & 1) * TB * ldw;
}

// The first `nheads` heads on h_L (rnn_fwd_kernel's layers without the stash): column 0 of head hd -> yout[row][hd].  Ends with a barrier.
__device__ __forceinline__ void stack_heads(const StackNet& p, float* hb, const float* hL, float* yout, int nheads, int lane, int wave) {
    const int g = lane >> 4, ldw = p.ldw, L = p.L;
    float* const pp[2] = {hb + ((L & 1) ^ 1) * TB * ldw, hb + 2 * TB * ldw};
    for (int hd = 0; hd < nheads; ++hd) {
        const StackHead& hp = p.head[hd];
        const float* in = hL;
        for (int l = 0; l < hp.nl; ++l) {
            const int K = hp.dims[l], N = hp.dims[l + 1];
            const float* bl = hp.b[l];
            if (l + 1 < hp.nl) {
                float* out = (l & 1) ? pp[1] : pp[0];
                act_dispatch(hp.act, [&]<int ACT>() {
                    rnn_dense(in, ldw, K, hp.w[l], N, lane, wave, [&](const f32x4& acc, int n, bool) {
                        const float bn = gptr(bl)[n];
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            float h, dh;
                            rnn_act_pair<ACT>(acc[r] + bn, h, dh);
                            out[(4 * g + r) * ldw + n] = h;
                        }
                    });
                });
                in = out;
            } else {
                rnn_dense(in, ldw, K, hp.w[l], N, lane, wave, [&](const f32x4& acc, int n, bool) {
                    if (n != 0) return;   // one action dimension
                    const float bn = gptr(bl)[0];
#pragma unroll
                    for (int r = 0; r < 4; ++r) yout[(4 * g + r) * 2 + hd] = acc[r] + bn;
                });
            }
            __syncthreads();
        }
    }
}

// One step of gym_cartpolecontiwithstack's data env on the newest state: the action through the description's ScaleAction / ClipAction
// range as gops_env_step takes it, cart_forward with the stacked env's force, reward 1 also for the step that ends the episode.
__device__ __forceinline__ bool stack_env_step(const GopsEnv& env, const float* x, float act, float* xn) {
    float r;
    bool done;
    cart_forward(cart_stack_const(), x, wrap_action(env, 0, act), xn, r, done);
    return done;
}

// The launch's start: zeroed tiles, the window (row j of instance m from src(m, j, k); zeros beyond nvalid) and its L projections.
template <int NB, class Src>
__device__ __forceinline__ void stack_prologue(const StackNet& p, const StackRegs<NB>& w, float* lds, int nvalid, Src&& src, int tid, int wave,
                                               int l15, int g) {
    const int L = p.L;
    float* win = lds + p.off_win;
    float* xs = lds + p.off_xs;
    for (int idx = tid; idx < L * TB * STACK_OBS; idx += NTHREADS) {
        const int j = idx / (TB * STACK_OBS), m = (idx >> 2) & (TB - 1), k = idx & 3;
        win[idx] = m < nvalid ? src(m, j, k) : 0.f;
    }
    if (tid < TB * STACK_OBS) xs[tid] = 0.f;
    __syncthreads();
    for (int j = 0; j < L; ++j) stack_project<NB>(p, w, win + j * TB * STACK_OBS, lds, j, nullptr, wave, l15, g);
    __syncthreads();
}

template <int NB>
__global__ __launch_bounds__(NTHREADS) void stack_sample_kernel(const StackSampleParams p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4;
    const int e0 = blockIdx.x * TB, nvalid = min(TB, p.N - e0);
    const int N = p.N, T = p.T, L = p.net.L, W = L * STACK_OBS;   // W: floats of one stored window
    float* const ring = lds;
    float* const hb = lds + p.net.off_hb;
    float* const win = lds + p.net.off_win;
    float* const xs = lds + p.net.off_xs;
    float* const yout = lds + p.net.off_y;
    int* const s_reset = reinterpret_cast<int*>(lds + p.net.off_flags);

    StackRegs<NB> w;
    stack_load_weights<NB>(p.net, w, wave, l15, g);
    if (tid < TB) s_reset[tid] = 0;
    stack_prologue<NB>(p.net, w, lds, nvalid, [&](int m, int j, int k) { return p.st.obs[(size_t)(e0 + m) * W + j * STACK_OBS + k]; }, tid,
                       wave, l15, g);
    for (int idx = tid; idx < nvalid * W; idx += NTHREADS) {   // the stored window of step 0: the persistent state
        const int m = idx / W, q = idx - m * W;
        p.out.obs[(size_t)(e0 + m) * W + q] = win[((q >> 2) * TB + m) * STACK_OBS + (q & 3)];
    }
    // the instance's books, in the registers of its lane (tid < nvalid)
    int ti = 0, rc = 0;
    if (tid < nvalid) { ti = p.st.t[e0 + tid]; rc = p.st.reset_count[e0 + tid]; }
    int base = 0;

#pragma unroll 1
    for (int t = 0; t < T; ++t) {
        const size_t row0 = (size_t)t * N + e0;   // the tile's first row of step t in a [T, N] column
        const float* hL = stack_recur<NB>(p.net, w, ring, hb, base, wave, l15, g);
        stack_heads(p.net, hb, hL, yout, 2, lane, wave);
        // one lane per instance: the exploration head in double, the env step on the newest row, the books
        if (tid < nvalid) {
            const int e = e0 + tid;
            const size_t row = row0 + tid;
            const double mean = (double)yout[2 * tid], eps = (double)p.noise[row];
            const GaussDim gd = gauss_dim((double)yout[2 * tid + 1], p.min_ls, p.max_ls);
            const float act = (float)(mean + gd.sd * eps);
            p.out.act[row] = act;
            p.out.logp[row] = (float)(-(eps * eps) / 2 - gd.ls - HALF_LOG_2PI);
            const int newest = base == 0 ? L - 1 : base - 1;
            float x[STACK_OBS], xn[STACK_OBS];
#pragma unroll
            for (int k = 0; k < STACK_OBS; ++k) x[k] = win[(newest * TB + tid) * STACK_OBS + k];
            const bool dn = stack_env_step(p.env, x, act, xn);
            ti += 1;
            const bool over = dn || ti >= p.max_steps;
            // rew, done, time_limited, end: one store in a rolled loop over the column table - four more base pointers held across
            // the step loop cost the kernel its scratch-free register allocation
#pragma unroll 1
            for (int c = 0; c < 4; ++c)
                p.books[c][row] = c == 0 ? 1.f : c == 1 ? (dn ? 1.f : 0.f) : c == 2 ? ((over && !dn) ? 1.f : 0.f) : ((over || t == T - 1) ? 1.f : 0.f);
            const float* fresh = p.pool.obs + ((size_t)(rc % p.R) * N + e) * STACK_OBS;   // (read only where `over`)
#pragma unroll
            for (int k = 0; k < STACK_OBS; ++k) {
                win[(base * TB + tid) * STACK_OBS + k] = xn[k];   // the oldest row leaves
                xs[tid * STACK_OBS + k] = over ? fresh[k] : xn[k];   // the row the ring takes
            }
            s_reset[tid] = over ? 1 : 0;
            if (over) { rc += 1; ti = 0; }
        }
        __syncthreads();
        // next_obs of step t, the window step t + 1 starts from (its obs row, or the persistent state) and the reset: element
        // (slot, m, k) of win is read and written by this thread alone; meanwhile the waves project the new row
        const int nbase = base + 1 == L ? 0 : base + 1;
        float* const next = t + 1 < T ? p.out.obs + (row0 + N) * W : p.st.obs + (size_t)e0 * W;
        for (int idx = tid; idx < nvalid * W; idx += NTHREADS) {
            const int m = idx / W, q = idx - m * W, k = q & 3;
            int slot = nbase + (q >> 2);
            if (slot >= L) slot -= L;
            float* at = win + (slot * TB + m) * STACK_OBS + k;
            const float v = *at;
            p.out.obs2[(row0 + m) * W + q] = v;
            const float vn = s_reset[m] ? xs[m * STACK_OBS + k] : v;
            next[(size_t)m * W + q] = vn;
            *at = vn;
        }
        stack_project<NB>(p.net, w, xs, ring, base, s_reset, wave, l15, g);
        base = nbase;
        __syncthreads();
    }
    if (tid < nvalid) { p.st.t[e0 + tid] = ti; p.st.reset_count[e0 + tid] = rc; }
}

template <int NB>
__global__ __launch_bounds__(NTHREADS) void stack_episode_kernel(const StackEpisodeParams p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4;
    const int e0 = blockIdx.x * TB, nvalid = min(TB, p.E - e0);
    const int T = p.T, L = p.net.L, W = L * STACK_OBS;
    float* const ring = lds;
    float* const hb = lds + p.net.off_hb;
    float* const win = lds + p.net.off_win;
    float* const xs = lds + p.net.off_xs;
    float* const yout = lds + p.net.off_y;
    int* const s_alive = reinterpret_cast<int*>(lds + p.net.off_flags);

    StackRegs<NB> w;
    stack_load_weights<NB>(p.net, w, wave, l15, g);
    if (tid < TB) s_alive[tid] = tid < nvalid ? 1 : 0;
    // a reset fills every row of the window with the initial state
    stack_prologue<NB>(p.net, w, lds, nvalid, [&](int m, int, int k) { return p.init[(size_t)(e0 + m) * STACK_OBS + k]; }, tid, wave, l15, g);
    // the episode's books, in the registers of its lane
    bool alive = tid < nvalid;
    double ret = 0.0;
    int length = 0, base = 0;

#pragma unroll 1
    for (int t = 0; t < T; ++t) {
        const float* hL = stack_recur<NB>(p.net, w, ring, hb, base, wave, l15, g);
        stack_heads(p.net, hb, hL, yout, 1, lane, wave);
        if (alive) {   // GaussDistribution.mode: clamp(mean, low, high); a NaN stays one
            const int e = e0 + tid;
            const float lo = p.env.policy_low[0], hi = p.env.policy_high[0], ya = yout[2 * tid];
            float act = ya < lo ? lo : ya;
            act = act > hi ? hi : act;
            if (p.out.trace_obs != nullptr)
                for (int q = 0; q < W; ++q) {
                    int slot = base + (q >> 2);
                    if (slot >= L) slot -= L;
                    p.out.trace_obs[((size_t)e * T + t) * W + q] = win[(slot * TB + tid) * STACK_OBS + (q & 3)];
                }
            const int newest = base == 0 ? L - 1 : base - 1;
            float x[STACK_OBS], xn[STACK_OBS];
#pragma unroll
            for (int k = 0; k < STACK_OBS; ++k) x[k] = win[(newest * TB + tid) * STACK_OBS + k];
            const bool dn = stack_env_step(p.env, x, act, xn);
#pragma unroll
            for (int k = 0; k < STACK_OBS; ++k) win[(base * TB + tid) * STACK_OBS + k] = xs[tid * STACK_OBS + k] = xn[k];
            ret += 1.0;
            length = t + 1;
            if (p.out.trace_act != nullptr) p.out.trace_act[(size_t)e * T + t] = act;
            if (p.out.trace_rew != nullptr) p.out.trace_rew[(size_t)e * T + t] = 1.f;
            if (dn || length == T) {
                alive = false;
                s_alive[tid] = 0;
                p.out.ret[e] = (float)ret;
                p.out.length[e] = length;
                p.out.terminated[e] = dn ? 1.f : 0.f;
            }
        }
        __syncthreads();   // publishes xs and s_alive; then the same 16 flags read by every thread: a uniform decision
        int any = 0;
#pragma unroll
        for (int m = 0; m < TB; ++m) any |= s_alive[m];
        if (!any) break;
        stack_project<NB>(p.net, w, xs, ring, base, nullptr, wave, l15, g);   // (an episode that ended keeps its last row: never read again)
        base = base + 1 == L ? 0 : base + 1;
        __syncthreads();
    }
}

// The description alone: GOPS_OK, or the code both families refuse it with.  The ORDER of the tests is part of the ABI.
int stack_check(const GopsEnv* env, const GopsRnn* pol, int n, int T) {
    if (!env || !pol || n < 1 || T < 1) return GOPS_ERR_BAD_ARG;
    if (!env->data_env) return GOPS_ERR_BAD_ARG;
    if (env->kind != GOPS_ENV_CARTPOLE) return GOPS_ERR_UNSUPPORTED;
    if (env->repeat_num > 1 || env->scale_obs || env->shaping) return GOPS_ERR_UNSUPPORTED;
    if (env->obs_dim != STACK_OBS || env->act_dim != 1) return GOPS_ERR_BAD_ARG;
    if (pol->n_heads != 2) return GOPS_ERR_BAD_ARG;
    const int rc = rnn_check(*pol, n);
    if (rc != GOPS_OK) return rc;
    if (pol->seq_len > GOPS_STACK_MAX_LEN) return GOPS_ERR_UNSUPPORTED;
    if (pol->obs_dim != STACK_OBS) return GOPS_ERR_BAD_ARG;
    for (int h = 0; h < 2; ++h)
        if (pol->head[h].sizes[pol->head[h].n_layers] != 1) return GOPS_ERR_BAD_ARG;
    return GOPS_OK;
}

// The device description of a checked net and its LDS bytes.
size_t stack_plan(const GopsRnn& d, StackNet& p) {
    p.L = d.seq_len; p.H = d.hidden;
    p.wih = d.weight_ih; p.whh = d.weight_hh; p.bih = d.bias_ih; p.bhh = d.bias_hh;
    int maxw = d.hidden;
    for (int h = 0; h < 2; ++h) {
        const GopsMlp& m = d.head[h];
        StackHead& hd = p.head[h];
        hd.nl = m.n_layers; hd.act = m.hidden_act;
        for (int l = 0; l <= m.n_layers; ++l) hd.dims[l] = m.sizes[l];
        for (int l = 0; l < m.n_layers; ++l) {
            hd.w[l] = m.weight[l]; hd.b[l] = m.bias[l];
            if (l + 1 < m.n_layers && m.sizes[l + 1] > maxw) maxw = m.sizes[l + 1];
        }
    }
    p.ldw = maxw + 4; p.ldr = p.H + 4;
    int off = p.L * TB * p.ldr;
    p.off_hb = off; off += 3 * TB * p.ldw;
    p.off_win = off; off += p.L * TB * STACK_OBS;
    p.off_xs = off; off += TB * STACK_OBS;
    p.off_y = off; off += TB * 2;
    p.off_flags = off; off += TB;
    return (size_t)off * sizeof(float);
}

template <class Params, class K1, class K2>
int stack_launch(K1 k1, K2 k2, const Params& p, size_t lds, int n, void* stream) {
    const dim3 grid((unsigned)((n + TB - 1) / TB)), block(NTHREADS);
    if (p.net.H <= 64) launch_with_lds(k1, grid, block, lds, static_cast<hipStream_t>(stream), p);
    else launch_with_lds(k2, grid, block, lds, static_cast<hipStream_t>(stream), p);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

size_t gops_stack_sample_workspace_bytes(const GopsEnv* env, const GopsRnn* policy, int32_t n_envs, int32_t steps) {
    return stack_check(env, policy, n_envs, steps) == GOPS_OK ? GOPS_SAMPLE_WORKSPACE_BYTES : 0;
}

int gops_stack_sample_rollout(const GopsEnv* env, const GopsRnn* policy, const GopsSampleDesc* desc, int32_t n_envs, int32_t steps,
                              const GopsSampleState* state, const GopsSamplePool* pool, const float* noise, const GopsSampleOut* out,
                              void* ws, size_t ws_bytes, void* stream) {
    if (!env || !policy || !desc || !state || !pool || !noise || !out || steps < 1 || n_envs < 1) return GOPS_ERR_BAD_ARG;
    if (desc->pool_rows < 1 || desc->max_episode_steps < 1) return GOPS_ERR_BAD_ARG;
    if (desc->head < GOPS_SAMPLE_DETERM || desc->head > GOPS_SAMPLE_TANH_GAUSS) return GOPS_ERR_BAD_ARG;
    if (desc->head != GOPS_SAMPLE_GAUSS) return GOPS_ERR_UNSUPPORTED;
    const int rc = stack_check(env, policy, n_envs, steps);
    if (rc != GOPS_OK) return rc;
    if (!state->obs || !state->t || !state->reset_count || !pool->obs) return GOPS_ERR_BAD_ARG;
    if (!out->obs || !out->act || !out->rew || !out->done || !out->obs2 || !out->logp || !out->time_limited || !out->end) return GOPS_ERR_BAD_ARG;
    if (!ws || ws_bytes < GOPS_SAMPLE_WORKSPACE_BYTES) return GOPS_ERR_WORKSPACE;
    StackSampleParams p;
    memset(&p, 0, sizeof(p));
    const size_t lds = stack_plan(*policy, p.net);
    p.env = *env;
    p.N = n_envs, p.T = steps, p.R = desc->pool_rows, p.max_steps = desc->max_episode_steps;
    p.min_ls = desc->min_log_std, p.max_ls = desc->max_log_std;
    p.st = *state, p.pool = *pool, p.noise = noise, p.out = *out;
    p.books[0] = out->rew, p.books[1] = out->done, p.books[2] = out->time_limited, p.books[3] = out->end;
    return stack_launch(stack_sample_kernel<1>, stack_sample_kernel<2>, p, lds, n_envs, stream);
}

size_t gops_stack_episode_workspace_bytes(const GopsEnv* env, const GopsRnn* policy, int32_t episodes, int32_t max_steps) {
    return stack_check(env, policy, episodes, max_steps) == GOPS_OK ? GOPS_SAMPLE_WORKSPACE_BYTES : 0;
}

int gops_stack_episode_rollout(const GopsEnv* env, const GopsRnn* policy, int32_t episodes, int32_t max_steps, const float* init_state,
                               const GopsEpisodeOut* out, void* ws, size_t ws_bytes, void* stream) {
    const int rc = stack_check(env, policy, episodes, max_steps);
    if (rc != GOPS_OK) return rc;
    if (!init_state || !out || !out->ret || !out->length || !out->terminated) return GOPS_ERR_BAD_ARG;
    if (!ws || ws_bytes < GOPS_SAMPLE_WORKSPACE_BYTES) return GOPS_ERR_WORKSPACE;
    StackEpisodeParams p;
    memset(&p, 0, sizeof(p));
    const size_t lds = stack_plan(*policy, p.net);
    p.env = *env;
    p.E = episodes, p.T = max_steps, p.init = init_state, p.out = *out;
    return stack_launch(stack_episode_kernel<1>, stack_episode_kernel<2>, p, lds, episodes, stream);
}

}  // extern "C"
