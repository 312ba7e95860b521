// A whole sample() of the device samplers (gops_amd/trainer/sampler/device_env_sampler.py: _step_once, T times) in ONE launch:
// policy, exploration head, env step, the stored transition row, episode bookkeeping and the re-seeding of finished instances.
//
// A workgroup of 256 threads owns a tile of 16 environment instances (GOPS_TILE = MFMA M) for all T steps.  Per step t:
//   1. carry: all threads write the tile's rows of step t - observation and, for the vehicle families, the info tensors - from where
//      each row continues (the persistent state at t = 0; the previous step's next_* row; or, after a reset, the instance's own
//      column of the reset pool) into the time-major outputs, contiguous per tile, and the observations into LDS;
//   2. the hidden layers on v_mfma_f32_16x16x4_f32 and the head's dot products (policy_tile.h, shared with the episode kernel);
//   3. one lane per instance forms the head in double - DETERM / GAUSS / TANH_GAUSS, gauss_math.h / soft_math.h - from this
//      step's noise row and stores act and logp, each rounded once; with an action table (gops_sample_rollout_dis) the outputs are
//      action values / logits instead: EPS_GREEDY / CATEGORICAL pick an index from two uniforms, `act` is the index and the env
//      steps with the table's row (env_act);
//   4. one lane per instance takes the env step through env_step_one (env_step.h: the function gops_env_step calls) with the
//      step's output rows as its operands - obs2, rew, done and the next_* info ARE the stored row -, then keeps the books:
//      t += 1, over = done or t >= max_episode_steps, time_limited, end, and where the row continues from (an LDS flag per row).
// After the last step the same carry writes the persistent state.  A row depends on its own instance only: the pool row is
// reset_count[i] % R of column i.  No workgroup reads what another wrote; no atomics; every loop is bounded by `steps`.
// Which descriptions the kernel admits, the widths of the info tensors and the workspace queries' rule: closed_loop.h, shared with
// the episode kernel (the rules that differ are SAMPLE_RULES below).
#include <stdint.h>
#include <string.h>

#include "env_step.h"
#include "common.h"
#include "closed_loop.h"
#include "policy_tile.h"
#include "soft_math.h"

namespace {

struct SampleParams {
    GopsEnv env;   // padded (lq_pad_env), reference constants filled
    PolicyTile net;
    int N, T, O, A, head, R, max_steps;
    InfoWidths info;
    float pdt;
    double noise_std, min_ls, max_ls;
    GopsSampleState st;
    GopsSamplePool pool;
    const float* noise;
    GopsSampleOut out;
    // the discrete heads (act_num = 0: none): the table [act_num, A] in device memory, the applied rows [T, N, A]
    int act_num;
    double epsilon;
    const float* table;
    float* env_act;
};
static_assert(sizeof(SampleParams) <= 4096, "kernel arguments are passed by value");

// Data envs and - pendulum, mountaincar: no data-env restatement - env models; no time-augmented policies (FiniteHorizonPolicy);
// output width A or 2A (the entry point then holds the width against the head).
constexpr ClosedLoopRules SAMPLE_RULES = {CLOSED_LOOP_DATA_KINDS, 1u << GOPS_ENV_PENDULUM | 1u << GOPS_ENV_MOUNTAINCAR, false, true};

// Where row m continues from: src < 0 the persistent state, 0 the previous step's next_* row, k + 1 pool row k of its column.
__device__ __forceinline__ float carried(int src, const float* st, const float* prev, const float* pool, size_t N, size_t i, int w, int k) {
    return src < 0 ? st[i * w + k] : src == 0 ? prev[i * w + k] : pool[((size_t)(src - 1) * N + i) * w + k];
}

// One field of the tile's rows, all threads: dst[e0 .. e0 + nvalid) (contiguous) from where each row continues.
__device__ __forceinline__ void carry_field(float* dst, const float* st, const float* prev, const float* pool, const int* s_src, int N,
                                            int e0, int nvalid, int w, int tid) {
    for (int idx = tid; idx < nvalid * w; idx += PT_THREADS) {
        const int m = idx / w, k = idx - m * w;
        dst[(size_t)e0 * w + idx] = carried(s_src[m], st, prev, pool, (size_t)N, (size_t)(e0 + m), w, k);
    }
}

// The five info tensors of the tile's rows (the vehicle families) into the destinations given: the step's rows of the outputs, or the
// persistent state itself.  `prow0`: the first row of the previous step - a continuing episode carries its next_* rows (the ids: its own).
__device__ __forceinline__ void carry_info(const SampleParams& p, float* state, float* ref_points, float* path_num, float* u_num,
                                           float* ref_time, size_t prow0, const int* s_src, int N, int sd, int rf, int e0, int nvalid, int tid) {
    carry_field(state, p.st.state, p.out.next_state + prow0 * sd, p.pool.state, s_src, N, e0, nvalid, sd, tid);
    carry_field(ref_points, p.st.ref_points, p.out.next_ref_points + prow0 * rf, p.pool.ref_points, s_src, N, e0, nvalid, rf, tid);
    carry_field(path_num, p.st.path_num, p.out.path_num + prow0, p.pool.path_num, s_src, N, e0, nvalid, 1, tid);
    carry_field(u_num, p.st.u_num, p.out.u_num + prow0, p.pool.u_num, s_src, N, e0, nvalid, 1, tid);
    carry_field(ref_time, p.st.ref_time, p.out.next_ref_time + prow0, p.pool.ref_time, s_src, N, e0, nvalid, 1, tid);
}

__global__ __launch_bounds__(PT_THREADS) void sample_kernel(const SampleParams p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int e0 = blockIdx.x * GOPS_TILE;
    const int nvalid = min(GOPS_TILE, p.N - e0);
    const int N = p.N, T = p.T, O = p.O, A = p.A, nl = p.net.nl, ldx = p.net.ldx;
    const int sd = p.info.state_dim, rf = p.info.ref_floats;
    float* xa = lds;
    float* xb = lds + GOPS_TILE * ldx;
    int* s_src = reinterpret_cast<int*>(lds + p.net.flags_off);

    policy_tile_load(p.net, lds, tid);
    if (tid < GOPS_TILE) s_src[tid] = -1;   // the first step continues from the persistent state
    // the instance's books, in the registers of its lane (tid < nvalid)
    int ti = 0, rc = 0;
    if (tid < nvalid) { ti = p.st.t[e0 + tid]; rc = p.st.reset_count[e0 + tid]; }
    __syncthreads();

    const int K0p = (O + 15) & ~15;
#pragma unroll 1
    for (int t = 0; t < T; ++t) {
        const size_t row0 = (size_t)t * N;                    // first row of step t in a [T, N] column
        const size_t prow0 = t > 0 ? row0 - (size_t)N : 0;    // of step t - 1 (not read at t = 0: every src is < 0)
        // 1. carry the tile's rows of step t; observations also -> xa (zero padded)
        for (int idx = tid; idx < GOPS_TILE * K0p; idx += PT_THREADS) {
            const int m = idx / K0p, k = idx - m * K0p;
            float v = 0.f;
            if (m < nvalid && k < O) {
                v = carried(s_src[m], p.st.obs, p.out.obs2 + prow0 * O, p.pool.obs, (size_t)N, (size_t)(e0 + m), O, k);
                p.out.obs[(row0 + e0 + m) * O + k] = v;
            }
            xa[m * ldx + k] = v;
        }
        if (sd > 0)
            carry_info(p, p.out.state + row0 * sd, p.out.ref_points + row0 * rf, p.out.path_num + row0, p.out.u_num + row0,
                       p.out.ref_time + row0, prow0, s_src, N, sd, rf, e0, nvalid, tid);
        __syncthreads();
        // 2. hidden layers
        const float* cur_x = policy_tile_hidden(p.net, lds, xa, xb, lane, wave);
        // 3. head: 16 lanes per instance form the dot products, the group's first lane the action and its log-probability
        if (p.act_num > 0) {   // an action table: y = action values (EPS_GREEDY) or logits (CATEGORICAL), two uniforms per row
            const int m = tid >> 4, part = tid & 15, n = p.act_num;
            float y[GOPS_DQN_MAX_ACTIONS];
            policy_tile_values(p.net, lds, cur_x, m, part, n, y);
            if (part == 0 && m < nvalid) {
                const size_t row = row0 + e0 + m;
                const double u0 = (double)p.noise[row * 2], u1 = (double)p.noise[row * 2 + 1];
                const int greedy = policy_tile_greedy(y, n);
                int index;
                double lp = 0.0;
                if (p.head == GOPS_SAMPLE_EPS_GREEDY) {
                    const int uniform = max(min((int)(u1 * n), n - 1), 0);
                    index = u0 < p.epsilon ? uniform : greedy;
                } else {
                    index = policy_tile_categorical(y, n, greedy, u0, lp);
                }
                p.out.act[row] = (float)index;
                p.out.logp[row] = (float)lp;
                for (int a = 0; a < A; ++a) p.env_act[row * A + a] = p.table[index * A + a];   // 0 <= index < act_num on every path
            }
        } else {
            const int m = tid >> 4, part = tid & 15;
            float ym[GOPS_MAX_ACT], yl[GOPS_MAX_ACT];
            policy_tile_head(p.net, lds, cur_x, m, part, 0, A, ym);
            if (p.head != GOPS_SAMPLE_DETERM) policy_tile_head(p.net, lds, cur_x, m, part, A, A, yl);
            if (part == 0 && m < nvalid) {
                const size_t row = row0 + e0 + m;
                const float* bo = lds + p.net.b_off[nl - 1];
                double lp = 0.0;
#pragma unroll
                for (int a = 0; a < GOPS_MAX_ACT; ++a) {
                    if (a < A) {
                        const double mean = (double)(ym[a] + bo[a]), e = (double)p.noise[row * A + a];
                        const double lo = (double)p.env.policy_low[a], hi = (double)p.env.policy_high[a];
                        double act;
                        if (p.head == GOPS_SAMPLE_DETERM) {
                            act = (hi - lo) / 2 * tanh(mean) + (hi + lo) / 2 + p.noise_std * e;
                        } else if (p.head == GOPS_SAMPLE_GAUSS) {
                            const GaussDim g = gauss_dim((double)(yl[a] + bo[A + a]), p.min_ls, p.max_ls);
                            act = mean + g.sd * e;
                            lp += -(e * e) / 2 - g.ls - HALF_LOG_2PI;
                        } else {
                            const TanhGaussDim d = tanh_gauss_dim(mean, (double)(yl[a] + bo[A + a]), e, lo, hi, p.min_ls, p.max_ls);
                            act = d.act;
                            lp += d.logp;
                        }
                        p.out.act[row * A + a] = (float)act;
                    }
                }
                p.out.logp[row] = (float)lp;
            }
        }
        __syncthreads();   // (also orders the action stores before the env lane's loads: one workgroup, global memory)
        // 4. one lane per instance: the env step on the stored row, the instance's books
        if (tid < nvalid) {
            const int e = e0 + tid;
            const size_t row = row0 + e;
            GopsStepIO io = {};
            io.obs = p.out.obs + row0 * O; io.action = (p.act_num > 0 ? p.env_act : p.out.act) + row0 * A; io.done = nullptr;
            io.next_obs = p.out.obs2 + row0 * O; io.reward = p.out.rew + row0; io.next_done = p.out.done + row0;
            if (sd > 0) {
                io.state = p.out.state + row0 * sd; io.ref_points = p.out.ref_points + row0 * rf;
                io.path_num = p.out.path_num + row0; io.u_num = p.out.u_num + row0; io.ref_time = p.out.ref_time + row0;
                io.next_state = p.out.next_state + row0 * sd; io.next_ref_points = p.out.next_ref_points + row0 * rf;
                io.next_ref_time = p.out.next_ref_time + row0;
            }
            env_step_one(p.env, e, io, p.pdt);
            if (sd > 0) {   // the ids do not change within an episode
                p.out.next_path_num[row] = p.out.path_num[row];
                p.out.next_u_num[row] = p.out.u_num[row];
            }
            const bool dn = p.out.done[row] != 0.f;
            ti += 1;
            const bool over = dn || ti >= p.max_steps;
            p.out.time_limited[row] = (over && !dn) ? 1.f : 0.f;
            p.out.end[row] = (over || t == T - 1) ? 1.f : 0.f;
            if (over) {
                s_src[tid] = rc % p.R + 1;
                rc += 1;
                ti = 0;
            } else {
                s_src[tid] = 0;
            }
        }
        __syncthreads();   // publishes the step's next_* rows and s_src to the tile
    }
    // the persistent state: where step T would have continued from
    {
        const size_t prow0 = (size_t)(T - 1) * N;
        carry_field(p.st.obs, p.st.obs, p.out.obs2 + prow0 * O, p.pool.obs, s_src, N, e0, nvalid, O, tid);
        if (sd > 0) carry_info(p, p.st.state, p.st.ref_points, p.st.path_num, p.st.u_num, p.st.ref_time, prow0, s_src, N, sd, rf, e0, nvalid, tid);
        if (tid < nvalid) { p.st.t[e0 + tid] = ti; p.st.reset_count[e0 + tid] = rc; }
    }
}

// What both entry points do once their own head checks passed: the pointer checks, the parameters, the launch.
int sample_launch(const GopsEnv* env, const GopsMlp* policy, const GopsSampleDesc* desc, int head, const GopsSampleDis* dis, int n_envs,
                  int steps, const GopsSampleState* state, const GopsSamplePool* pool, const float* noise, const GopsSampleOut* out,
                  void* ws, size_t ws_bytes, void* stream) {
    const int A = env->act_dim;
    if (!state->obs || !state->t || !state->reset_count || !pool->obs) return GOPS_ERR_BAD_ARG;
    if (!out->obs || !out->act || !out->rew || !out->done || !out->obs2 || !out->logp || !out->time_limited || !out->end) return GOPS_ERR_BAD_ARG;
    if (env_has_ref_table(env->kind)) {
        if (!state->state || !state->ref_points || !state->path_num || !state->u_num || !state->ref_time) return GOPS_ERR_BAD_ARG;
        if (!pool->state || !pool->ref_points || !pool->path_num || !pool->u_num || !pool->ref_time) return GOPS_ERR_BAD_ARG;
        if (!out->state || !out->next_state || !out->ref_points || !out->next_ref_points || !out->path_num || !out->next_path_num ||
            !out->u_num || !out->next_u_num || !out->ref_time || !out->next_ref_time)
            return GOPS_ERR_BAD_ARG;
    }
    SampleParams p;
    memset(&p, 0, sizeof(p));
    const size_t lds = policy_tile_plan(*policy, p.net);
    if (lds == 0) return GOPS_ERR_UNSUPPORTED;
    if (!ws || ws_bytes < GOPS_SAMPLE_WORKSPACE_BYTES) return GOPS_ERR_WORKSPACE;
    p.env = *env;
    fill_ref_defaults(p.env);
    lq_pad_env(p.env);
    policy_tile_bind(*policy, p.net);
    p.N = n_envs, p.T = steps, p.O = env->obs_dim, p.A = A;
    p.head = head, p.R = desc->pool_rows, p.max_steps = desc->max_episode_steps;
    p.noise_std = desc->noise_std, p.min_ls = desc->min_log_std, p.max_ls = desc->max_log_std;
    p.info = info_widths(*env);
    p.pdt = pdt_of(*env);
    p.st = *state, p.pool = *pool, p.noise = noise, p.out = *out;
    if (dis) p.act_num = dis->act_num, p.epsilon = dis->epsilon, p.table = dis->action_table, p.env_act = dis->env_act;
    launch_with_lds(sample_kernel, dim3((unsigned)((n_envs + GOPS_TILE - 1) / GOPS_TILE)), dim3(PT_THREADS), lds, static_cast<hipStream_t>(stream), p);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

size_t gops_sample_workspace_bytes(const GopsEnv* env, const GopsMlp* policy, int32_t n_envs, int32_t steps) {
    return closed_loop_takes(SAMPLE_RULES, env, policy, n_envs, steps, 0) ? GOPS_SAMPLE_WORKSPACE_BYTES : 0;
}

size_t gops_sample_dis_workspace_bytes(const GopsEnv* env, const GopsMlp* policy, int32_t act_num, int32_t n_envs, int32_t steps) {
    if (act_num < 2 || act_num > GOPS_DQN_MAX_ACTIONS) return 0;
    return closed_loop_takes(SAMPLE_RULES, env, policy, n_envs, steps, act_num) ? GOPS_SAMPLE_WORKSPACE_BYTES : 0;
}

int gops_sample_rollout(const GopsEnv* env, const GopsMlp* policy, const GopsSampleDesc* desc, int32_t n_envs, int32_t steps,
                        const GopsSampleState* state, const GopsSamplePool* pool, const float* noise, const GopsSampleOut* out,
                        void* ws, size_t ws_bytes, void* stream) {
    if (!env || !policy || !desc || !state || !pool || !noise || !out || steps < 1 || n_envs < 1) return GOPS_ERR_BAD_ARG;
    if (desc->pool_rows < 1 || desc->max_episode_steps < 1) return GOPS_ERR_BAD_ARG;
    if (desc->head < GOPS_SAMPLE_DETERM || desc->head > GOPS_SAMPLE_TANH_GAUSS) return GOPS_ERR_BAD_ARG;
    const int rc = closed_loop_check(SAMPLE_RULES, env, policy, n_envs, steps, 0);
    if (rc != GOPS_OK) return rc;
    const int A = env->act_dim, n_out = policy->sizes[policy->n_layers];
    if (n_out != (desc->head == GOPS_SAMPLE_DETERM ? A : 2 * A)) return GOPS_ERR_BAD_ARG;   // (an odd width for the Gaussian heads included)
    return sample_launch(env, policy, desc, desc->head, nullptr, n_envs, steps, state, pool, noise, out, ws, ws_bytes, stream);
}

int gops_sample_rollout_dis(const GopsEnv* env, const GopsMlp* policy, const GopsSampleDesc* desc, const GopsSampleDis* dis,
                            int32_t n_envs, int32_t steps, const GopsSampleState* state, const GopsSamplePool* pool, const float* noise,
                            const GopsSampleOut* out, void* ws, size_t ws_bytes, void* stream) {
    if (!env || !policy || !desc || !dis || !state || !pool || !noise || !out || steps < 1 || n_envs < 1) return GOPS_ERR_BAD_ARG;
    if (desc->pool_rows < 1 || desc->max_episode_steps < 1) return GOPS_ERR_BAD_ARG;
    if (!dis->action_table || !dis->env_act) return GOPS_ERR_BAD_ARG;
    if (dis->head != GOPS_SAMPLE_EPS_GREEDY && dis->head != GOPS_SAMPLE_CATEGORICAL) return GOPS_ERR_BAD_ARG;
    if (!(dis->epsilon >= 0.0 && dis->epsilon <= 1.0)) return GOPS_ERR_BAD_ARG;   // (a NaN included)
    if (dis->head == GOPS_SAMPLE_CATEGORICAL && dis->epsilon != 0.0) return GOPS_ERR_BAD_ARG;
    if (dis->act_num < 2 || dis->act_num > GOPS_DQN_MAX_ACTIONS) return GOPS_ERR_UNSUPPORTED;
    const int rc = closed_loop_check(SAMPLE_RULES, env, policy, n_envs, steps, dis->act_num);   // (BAD_ARG for an output width other than act_num)
    if (rc != GOPS_OK) return rc;
    return sample_launch(env, policy, desc, dis->head, dis, n_envs, steps, state, pool, noise, out, ws, ws_bytes, stream);
}

}  // extern "C"
