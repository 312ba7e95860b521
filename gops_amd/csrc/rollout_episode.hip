// Closed-loop evaluation episodes (gops/trainer/evaluator.py:45-86 run_an_episode): policy, DATA-env step, termination, time limit
// and return of E episodes over up to T steps in ONE launch, no host sync inside.
//
// A workgroup of 256 threads owns a tile of 16 episodes (GOPS_TILE = MFMA M) from the first step to the last:
//   1. all threads stage the tile's observations [16][K0] in LDS (a FiniteHorizonPolicy gets virtual_t = 1 behind them: the
//      reference evaluator calls policy(obs) with the default) and record them in trace_obs;
//   2. all four waves evaluate the hidden layers on v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation: evaluation
//      does not depend on the plane-split precision guard), wave w the 16-feature tiles w, w + 4, ..; activations ping-pong
//      between two LDS tiles; weights are read in place from the live parameter tensors - staged in LDS once per launch when the
//      whole network fits next to the tiles, else streamed from L2 every step;
//   3. 16 lanes per episode form the head's dot products (DPP sum), lane a squashes action a (tanh, act limits) and stores it;
//      with a mode head (gops_episode_rollout_mode) the stack is 2A wide - A means, then A log stds - and lane a stores the mode
//      of the action distribution, formed from mean a alone (the log-std rows take part in no dot product);
//      with an action table (gops_episode_rollout_dis) the outputs are action values / logits: lane a stores component a of the
//      table's row at their arg-max, and the trace keeps the index;
//   4. one lane per episode takes the data env's step through env_step_one (env_step.h) - the function env_step_kernel calls, so
//      the trace of an episode is reproduced by gops_env_step step by step - and keeps the episode's books in registers.
// The per-episode step buffers (obs, state, ref_points ring, ref_time) ping-pong between two sets in the workspace; each
// workgroup touches its own 16 rows only, which stay in L2.  Episodes that ended take no further step and write no further
// trace row; the workgroup leaves the loop once all of its episodes have ended (the alive flags in LDS, read by every thread: a uniform decision).
// Which descriptions the kernel admits, the widths of the info tensors and the workspace queries' rule: closed_loop.h, shared with
// the sampler kernel (the rules that differ are EPISODE_RULES below).
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "env_step.h"
#include "common.h"
#include "closed_loop.h"
#include "policy_tile.h"

namespace {

constexpr int EP_THREADS = PT_THREADS;

struct EpisodeParams {
    GopsEnv env;   // padded (lq_pad_env), reference constants filled
    PolicyTile net;
    int E, T, O, A, fh;
    InfoWidths info;
    float pdt;
    GopsStepIO init;
    float* obs[2];
    float* state[2];
    float* refp[2];
    float* reft[2];
    float *action, *reward, *done;
    GopsEpisodeOut out;
    int head;             // GOPS_SAMPLE_DETERM, or a mode head over a 2A-wide stack: GOPS_SAMPLE_GAUSS / _TANH_GAUSS
    int act_num;          // the greedy head over an action table (0: none)
    const float* table;   // [act_num, A], device memory
};

struct EpisodeLayout {
    size_t obs, state, refp, reft, action, reward, done, bytes;   // float offsets of the first buffer of each pair
    size_t obs_n, state_n, refp_n, reft_n;
};

EpisodeLayout episode_layout(const GopsEnv& e, int E) {
    EpisodeLayout l{};
    const bool ref = env_has_ref_table(e.kind);
    auto ep_align = [](size_t nfloats) { return align256(nfloats * sizeof(float)) / sizeof(float); };   // the layout counts floats
    const InfoWidths w = info_widths(e);
    l.obs_n = ep_align((size_t)E * e.obs_dim);
    l.state_n = ref ? ep_align((size_t)E * w.state_dim) : 0;
    l.refp_n = ref ? ep_align((size_t)E * w.ref_floats) : 0;
    l.reft_n = ref ? ep_align((size_t)E) : 0;
    size_t off = 0;
    l.obs = off; off += 2 * l.obs_n;
    l.state = off; off += 2 * l.state_n;
    l.refp = off; off += 2 * l.refp_n;
    l.reft = off; off += 2 * l.reft_n;
    l.action = off; off += ep_align((size_t)E * e.act_dim);
    l.reward = off; off += ep_align((size_t)E);
    l.done = off; off += ep_align((size_t)E);
    l.bytes = off * sizeof(float);
    return l;
}

// Evaluation steps the DATA environment (pendulum, mountaincar: no data-env restatement); a FiniteHorizonPolicy's time input is
// taken (virtual_t = 1); output width A, the deterministic head's.
constexpr ClosedLoopRules EPISODE_RULES = {CLOSED_LOOP_DATA_KINDS, 0, true, false};
// The mode heads: the same, with the sampler's width rule (the entry point then holds the width against 2A).
constexpr ClosedLoopRules EPISODE_MODE_RULES = {CLOSED_LOOP_DATA_KINDS, 0, true, true};

__global__ __launch_bounds__(EP_THREADS) void episode_kernel(const EpisodeParams p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int e0 = blockIdx.x * GOPS_TILE;
    const int nvalid = min(GOPS_TILE, p.E - e0);
    const int O = p.O, A = p.A, nl = p.net.nl, ldx = p.net.ldx;
    float* xa = lds;
    float* xb = lds + GOPS_TILE * ldx;
    int* s_alive = reinterpret_cast<int*>(lds + p.net.flags_off);

    // ---- once per launch: biases (and weights) into LDS, the tile's initial condition into step buffer 0 ----
    policy_tile_load(p.net, lds, tid);
    if (tid < GOPS_TILE) s_alive[tid] = tid < nvalid ? 1 : 0;
    for (int idx = tid; idx < nvalid * O; idx += EP_THREADS) p.obs[0][(size_t)e0 * O + idx] = p.init.obs[(size_t)e0 * O + idx];
    if (p.info.state_dim > 0) {
        for (int idx = tid; idx < nvalid * p.info.state_dim; idx += EP_THREADS)
            p.state[0][(size_t)e0 * p.info.state_dim + idx] = p.init.state[(size_t)e0 * p.info.state_dim + idx];
        for (int idx = tid; idx < nvalid * p.info.ref_floats; idx += EP_THREADS)
            p.refp[0][(size_t)e0 * p.info.ref_floats + idx] = p.init.ref_points[(size_t)e0 * p.info.ref_floats + idx];
        if (tid < nvalid) p.reft[0][e0 + tid] = p.init.ref_time[e0 + tid];
    }
    // the episode's books, in the registers of its lane (tid < nvalid)
    bool alive = tid < nvalid;
    double ret = 0.0;   // (one add per step in one lane: the return carries no summation error of its own)
    int length = 0;
    __syncthreads();

    const int K0 = p.net.dims[0], K0p = (K0 + 15) & ~15;
#pragma unroll 1
    for (int t = 0; t < p.T; ++t) {
        const int cur = t & 1;
        // 1. observations of the tile -> xa (zero padded; virtual_t = 1 for a FiniteHorizonPolicy), trace_obs
        {
            const float* ob = p.obs[cur];
            for (int idx = tid; idx < GOPS_TILE * K0p; idx += EP_THREADS) {
                const int m = idx / K0p, k = idx - m * K0p;
                float v = 0.f;
                if (m < nvalid) {
                    if (k < O) {
                        v = ob[(size_t)(e0 + m) * O + k];
                        if (p.out.trace_obs != nullptr && s_alive[m]) p.out.trace_obs[((size_t)(e0 + m) * p.T + t) * O + k] = v;
                    } else if (k == O && p.fh) {
                        v = 1.f;
                    }
                }
                xa[m * ldx + k] = v;
            }
        }
        __syncthreads();
        // 2. hidden layers
        const float* cur_x = policy_tile_hidden(p.net, lds, xa, xb, lane, wave);
        // 3. head: 16 lanes per episode, lane a squashes and stores action a
        if (p.act_num > 0) {   // the greedy head: every lane of the group holds all values, lane a stores the table row's component a
            const int m = tid >> 4, part = tid & 15;
            float y[GOPS_DQN_MAX_ACTIONS];
            policy_tile_values(p.net, lds, cur_x, m, part, p.act_num, y);
            const int index = policy_tile_greedy(y, p.act_num);   // 0 <= index < act_num
            if (part < A && m < nvalid) {
                p.action[(size_t)(e0 + m) * A + part] = p.table[index * A + part];
                if (part == 0 && p.out.trace_act != nullptr && s_alive[m]) p.out.trace_act[(size_t)(e0 + m) * p.T + t] = (float)index;
            }
        } else {
            const int m = tid >> 4, part = tid & 15;
            float y[GOPS_MAX_ACT];
            policy_tile_head(p.net, lds, cur_x, m, part, 0, A, y);
            if (part < A && m < nvalid) {
                const float ya = (part == 0 ? y[0] : part == 1 ? y[1] : part == 2 ? y[2] : y[3]) + lds[p.net.b_off[nl - 1] + part];
                const float lo = p.env.policy_low[part], hi = p.env.policy_high[part];
                float act;
                if (p.head == GOPS_SAMPLE_GAUSS) {   // GaussDistribution.mode: clamp(mean, low, high); a NaN stays one
                    act = ya < lo ? lo : ya;
                    act = act > hi ? hi : act;
                } else {   // the deterministic head, and TanhGaussDistribution.mode: the same squash of the mean
                    const float sc = (hi - lo) / 2.f;
                    const float of = (hi + lo) / 2.f;
                    act = sc * tanhf(ya) + of;
                }
                p.action[(size_t)(e0 + m) * A + part] = act;
                if (p.out.trace_act != nullptr && s_alive[m]) p.out.trace_act[((size_t)(e0 + m) * p.T + t) * A + part] = act;
            }
        }
        __syncthreads();   // (also orders the action stores before the env lane's loads: one workgroup, global memory)
        // 4. one lane per episode: the data env's step, the episode's books
        if (alive) {
            const int e = e0 + tid;
            GopsStepIO io = {};
            io.obs = p.obs[cur]; io.action = p.action; io.done = nullptr;
            io.state = p.state[cur]; io.ref_points = p.refp[cur]; io.path_num = p.init.path_num; io.u_num = p.init.u_num;
            io.ref_time = p.reft[cur];
            io.next_obs = p.obs[cur ^ 1]; io.reward = p.reward; io.next_done = p.done;
            io.next_state = p.state[cur ^ 1]; io.next_ref_points = p.refp[cur ^ 1]; io.next_ref_time = p.reft[cur ^ 1];
            env_step_one(p.env, e, io, p.pdt);
            const float r = p.reward[e];
            const bool dn = p.done[e] != 0.f;
            ret += (double)r;
            length = t + 1;
            if (p.out.trace_rew != nullptr) p.out.trace_rew[(size_t)e * p.T + t] = r;
            if (dn || length == p.T) {
                alive = false;
                s_alive[tid] = 0;
                p.out.ret[e] = (float)ret;
                p.out.length[e] = length;
                p.out.terminated[e] = dn ? 1.f : 0.f;
            }
        }
        // The barrier that publishes next_obs / s_alive to the tile, then the same 16 flags read by every thread: a uniform
        // decision.  (Not __syncthreads_or: it adds static LDS, and hipFuncSetAttribute then refuses the 160-KiB dynamic limit.)
        __syncthreads();
        int any = 0;
#pragma unroll
        for (int m = 0; m < GOPS_TILE; ++m) any |= s_alive[m];
        if (!any) break;
    }
}

// What the entry points do once the description passed: the pointer checks, the workspace, the launch.
int episode_launch(const GopsEnv* env, const GopsMlp* policy, int head, const float* table, int act_num, int E, int T,
                   const GopsStepIO* init, const GopsEpisodeOut* out, void* ws, size_t ws_bytes, void* stream) {
    if (!init || !out || !init->obs || !out->ret || !out->length || !out->terminated) return GOPS_ERR_BAD_ARG;
    const bool ref = env_has_ref_table(env->kind);
    if (ref && (!init->state || !init->ref_points || !init->path_num || !init->u_num || !init->ref_time)) return GOPS_ERR_BAD_ARG;
    EpisodeParams p;
    memset(&p, 0, sizeof(p));
    const size_t lds = policy_tile_plan(*policy, p.net);
    if (lds == 0) return GOPS_ERR_UNSUPPORTED;
    const EpisodeLayout l = episode_layout(*env, E);
    if (!ws || ws_bytes < l.bytes) return GOPS_ERR_WORKSPACE;
    p.env = *env;
    fill_ref_defaults(p.env);
    lq_pad_env(p.env);
    p.E = E, p.T = T, p.O = env->obs_dim, p.A = env->act_dim;
    p.fh = policy->sizes[0] == env->obs_dim + 1;
    policy_tile_bind(*policy, p.net);
    p.info = info_widths(*env);
    p.pdt = pdt_of(*env);
    p.init = *init;
    float* f = static_cast<float*>(ws);
    for (int i = 0; i < 2; ++i) {
        p.obs[i] = f + l.obs + i * l.obs_n;
        p.state[i] = ref ? f + l.state + i * l.state_n : nullptr;
        p.refp[i] = ref ? f + l.refp + i * l.refp_n : nullptr;
        p.reft[i] = ref ? f + l.reft + i * l.reft_n : nullptr;
    }
    p.action = f + l.action, p.reward = f + l.reward, p.done = f + l.done;
    p.out = *out;
    p.head = head, p.act_num = act_num, p.table = table;
    launch_with_lds(episode_kernel, dim3((unsigned)((E + GOPS_TILE - 1) / GOPS_TILE)), dim3(EP_THREADS), lds, static_cast<hipStream_t>(stream), p);
    return (int)hipGetLastError();
}

// gops_episode_rollout_mode's description: a Gaussian head code, the shared check, output width 2A (an odd one is refused here).
int episode_mode_check(const GopsEnv* env, const GopsMlp* policy, int head, int E, int T) {
    if (head != GOPS_SAMPLE_GAUSS && head != GOPS_SAMPLE_TANH_GAUSS) return GOPS_ERR_BAD_ARG;
    const int rc = closed_loop_check(EPISODE_MODE_RULES, env, policy, E, T, 0);
    if (rc != GOPS_OK) return rc;
    return policy->sizes[policy->n_layers] == 2 * env->act_dim ? GOPS_OK : GOPS_ERR_BAD_ARG;
}

}  // namespace

extern "C" {

size_t gops_episode_workspace_bytes(const GopsEnv* env, const GopsMlp* policy, int32_t E, int32_t T) {
    return closed_loop_takes(EPISODE_RULES, env, policy, E, T, 0) ? episode_layout(*env, E).bytes : 0;
}

size_t gops_episode_dis_workspace_bytes(const GopsEnv* env, const GopsMlp* policy, int32_t act_num, int32_t E, int32_t T) {
    if (act_num < 2 || act_num > GOPS_DQN_MAX_ACTIONS) return 0;
    return closed_loop_takes(EPISODE_RULES, env, policy, E, T, act_num) ? episode_layout(*env, E).bytes : 0;
}

int gops_episode_rollout(const GopsEnv* env, const GopsMlp* policy, int32_t E, int32_t T, const GopsStepIO* init, const GopsEpisodeOut* out,
                         void* ws, size_t ws_bytes, void* stream) {
    const int rc = closed_loop_check(EPISODE_RULES, env, policy, E, T, 0);
    if (rc != GOPS_OK) return rc;
    return episode_launch(env, policy, GOPS_SAMPLE_DETERM, nullptr, 0, E, T, init, out, ws, ws_bytes, stream);
}

int gops_episode_rollout_dis(const GopsEnv* env, const GopsMlp* policy, const float* action_table, int32_t act_num, int32_t E, int32_t T,
                             const GopsStepIO* init, const GopsEpisodeOut* out, void* ws, size_t ws_bytes, void* stream) {
    if (!action_table) return GOPS_ERR_BAD_ARG;
    if (act_num < 2 || act_num > GOPS_DQN_MAX_ACTIONS) return GOPS_ERR_UNSUPPORTED;
    const int rc = closed_loop_check(EPISODE_RULES, env, policy, E, T, act_num);   // (BAD_ARG for an output width other than act_num)
    if (rc != GOPS_OK) return rc;
    return episode_launch(env, policy, GOPS_SAMPLE_DETERM, action_table, act_num, E, T, init, out, ws, ws_bytes, stream);
}

size_t gops_episode_mode_workspace_bytes(const GopsEnv* env, const GopsMlp* policy, int32_t head, int32_t E, int32_t T) {
    PolicyTile net;
    return episode_mode_check(env, policy, head, E, T) == GOPS_OK && policy_tile_plan(*policy, net) != 0 ? episode_layout(*env, E).bytes : 0;
}

int gops_episode_rollout_mode(const GopsEnv* env, const GopsMlp* policy, int32_t head, int32_t E, int32_t T, const GopsStepIO* init,
                              const GopsEpisodeOut* out, void* ws, size_t ws_bytes, void* stream) {
    const int rc = episode_mode_check(env, policy, head, E, T);
    if (rc != GOPS_OK) return rc;
    return episode_launch(env, policy, head, nullptr, 0, E, T, init, out, ws, ws_bytes, stream);
}

}  // extern "C"
