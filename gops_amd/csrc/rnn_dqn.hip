// DQN on recurrent ActionValueDis networks (gops_amd/algorithm/dqn.py with value_func_type "RNN"): the target recurrence on obs2, the
// online recurrence on obs and the TD seam between them in ONE launch - include/gops_hip.h: gops_rnn_dqn_step.
//
// Mapping.  A workgroup of 512 threads (8 waves) owns a tile of TB = 16 transitions: row i of obs and row i of obs2 belong to the same
// transition, so everything between the two forwards and the backward - maximum, arg-max, backup, selected value, seed, |TD error| -
// is local to the tile.  Waves 0 - 3 carry the ONLINE net and waves 4 - 7 the TARGET net, each set with rnn_fwd_kernel's mapping
// (rnn_tile.h: 16-column blocks of H dealt round-robin to the set's four waves, NB = 1 up to H = 64 and 2 up to 128; the wave's
// W_hh / W_ih fragments and summed bias resident in registers for all L steps; exact fp32 v_mfma_f32_16x16x4_f32).  The hardware
// deals the waves of a workgroup round-robin to the four SIMDs, so every SIMD holds one wave of each chain: the two recurrences are
// independent, latency-bound serial chains (MFMA chain, tanhf, LDS store, barrier), and one chain's MFMAs fill the other's tanhf /
// LDS / barrier latency.  Both chains have the same L: the one barrier per step serves both.
//   LDS: per net the forward's three hidden tiles and two x tiles (x_{t+1} staged while step t computes), then two [16][17] tiles
//   that take the heads' outputs, behind 256 bytes of the fold's scratch - 256 + 2 x 34 048 + 2 176 bytes at the largest shape
//   (above the 64-KiB default: launch_with_lds; all of it dynamic).
//   The online set stashes exactly what gops_rnn_forward stashes, into the online net's gops_rnn workspace, and writes q_all; the
//   target set skips every stash store (its description carries no stash pointers at all) and writes only its LDS tile.
//   Seam (after the heads' last barrier): thread r < 16 owns row r - a_star = the lowest index attaining the maximum of the target
//   row (a NaN counts as the maximum), backup in double rounded once, the action index by truncation, the dense seed row, |q_sel -
//   backup| - and the three sums (w d^2, q_sel, rows with an index out of range) as doubles.  Every workgroup folds its sums
//   (block_reduce.h: grid_fold on eight waves), parks them in the call's scratch and draws a ticket; the workgroup that draws the
//   last one adds the tiles' partials in tile order (thread b: tiles b, b + 512, ..) and folds again.  No float atomics: two calls
//   give the same bits.  Rows beyond B are computed on zeros, never stored, and add nothing to the sums.
// The k-order and block order of every MFMA chain are rnn_fwd_kernel's (the same functions of rnn_tile.h), so the online q_all and
// the stash are bit-equal to what gops_rnn_forward leaves, and gops_rnn_backward follows unchanged.
#include <hip/hip_runtime.h>
#include <math.h>

#include "common.h"
#include "block_reduce.h"
#include "rnn_tile.h"

#define RD_THREADS (2 * NTHREADS)   // waves 0 - 3: the online net, 4 - 7: the target net
#define RD_LDQ 17                   // leading dim of the heads' output tiles [TB][RD_LDQ]
#define RD_FOLD_FLOATS 64           // head of the dynamic LDS: the fold's [3][8] doubles and its flag

struct RnnDqnParams {
    RnnDev net[2];                  // online (with its stash sections), target (without)
    const float *x[2];              // obs, obs2 [B, L, O]
    const float *act, *rew, *done, *weight;
    float *q_all, *backup, *seed, *abs_err, *stats;
    int* a_star;
    double* part;                   // [tiles][3]
    unsigned* ticket;
    double rscale, gamma;
    float gsc;                      // 2 / B
    int N;
};
static_assert(sizeof(RnnDqnParams) <= 4000, "RnnDqnParams is a kernel argument");

template <int NB>
__global__ __launch_bounds__(RD_THREADS) void rnn_dqn_kernel(const RnnDqnParams q) {
    extern __shared__ __attribute__((aligned(16))) float lds_all[];
    // (no static LDS: launch_with_lds raises the kernel's dynamic limit to the whole 160 KiB, which leaves no room beside it)
    double (*red)[8] = reinterpret_cast<double (*)[8]>(lds_all);        // [3][8]: the fold's scratch
    bool* const last = reinterpret_cast<bool*>(lds_all + RD_FOLD_FLOATS - 4);
    float* const lds = lds_all + RD_FOLD_FLOATS;
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4;
    const int set = __builtin_amdgcn_readfirstlane(tid >> 8), wave = __builtin_amdgcn_readfirstlane((tid >> 6) & 3), stid = tid & (NTHREADS - 1);
    const RnnDev& p = q.net[set];
    const float* x = q.x[set];
    const bool online = set == 0;
    const int ldw = p.ldw, ldx = p.ldx, L = p.L, N = q.N;
    const int row0 = blockIdx.x * TB;
    const int per_net = 3 * TB * ldw + 2 * TB * ldx;   // (both nets have the same widths: rnn_dqn_check)
    float* const hb = lds + set * per_net;
    float* const xb = hb + 3 * TB * ldw;
    float* const qt = lds + 2 * per_net;               // [2][TB][RD_LDQ]: online, target

    RnnRegs<NB> w;
    rnn_load_regs<NB>(p, wave, lane, w);
    rnn_stage_x(p, x, row0, 0, xb, stid);
    __syncthreads();

    for (int t = 0; t < L; ++t) {
        const int cur = t & 1;
        rnn_step<NB>(p, w, t, row0, hb + cur * TB * ldw, hb + (cur ^ 1) * TB * ldw, xb + cur * TB * ldx, online, wave, lane);
        if (t + 1 < L) rnn_stage_x(p, x, row0, t + 1, xb + (cur ^ 1) * TB * ldx, stid);
        __syncthreads();
    }

    float* const qs = qt + set * TB * RD_LDQ;
    rnn_heads(p, hb, row0, online, lane, wave, [&](const RnnHeadDev&, const f32x4& acc, float bn, int n) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = 4 * g + r;
            const float v = acc[r] + bn;
            qs[m * RD_LDQ + n] = v;
            if (online && row0 + m < p.B) gptr(q.q_all)[(size_t)(row0 + m) * N + n] = v;
        }
    });   // (ends in a barrier: both tiles are complete)

    // ---- the seam: gops_dqn_backup's and gops_dqn_loss's definitions, one thread per row
    double s[3] = {0.0, 0.0, 0.0};   // sum w d^2, sum q_sel, rows with an index outside [0, N)
    const int b = row0 + tid;
    if (tid < TB && b < p.B) {
        const float* tr = qt + TB * RD_LDQ + tid * RD_LDQ;
        float q_max = tr[0];
        int best = 0;
        for (int a = 1; a < N; ++a) {
            const float v = tr[a];
            if (v > q_max || (v != v && q_max == q_max)) q_max = v, best = a;   // (a NaN is the maximum, as for torch.max)
        }
        const float bk = (float)((double)gptr(q.rew)[b] * q.rscale + q.gamma * (1.0 - (double)gptr(q.done)[b]) * (double)q_max);
        gptr(q.backup)[b] = bk;
        gptr(q.a_star)[b] = best;
        const float af = gptr(q.act)[b];
        const bool ok = af > -1.f && af < (float)N;   // truncation towards zero lands in [0, N); false for a NaN
        const int a = ok ? (int)af : -1;
        float gs = 0.f, e = 0.f;
        if (ok) {
            const float qv = qt[tid * RD_LDQ + a];
            const float d = qv - bk;
            const float wt = q.weight != nullptr ? gptr(q.weight)[b] : 1.f;
            gs = q.weight != nullptr ? q.gsc * (wt * d) : q.gsc * d;
            e = fabsf(d);
            s[0] = (double)(q.weight != nullptr ? wt * (d * d) : d * d);
            s[1] = (double)qv;
        } else {
            s[2] = 1.0;
        }
        for (int c = 0; c < N; ++c) gptr(q.seed)[(size_t)b * N + c] = c == a ? gs : 0.f;
        gptr(q.abs_err)[b] = e;
    }
    if (grid_fold<3>(s, red, q.part, 3, q.ticket, last) && tid == 0) {
        q.stats[0] = (float)(s[0] / (double)p.B);
        q.stats[1] = (float)(s[1] / (double)p.B);
        q.stats[2] = (float)s[2];
        q.stats[3] = 0.f;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
namespace {

// every check of the pair of descriptions: GOPS_OK, or the code the entry points refuse it with
int rnn_dqn_check(const GopsRnn* on, const GopsRnn* tg, const GopsRnnDqn* d, int B) {
    if (!on || !tg || !d || B < 1 || on->n_heads != 1 || tg->n_heads != 1) return GOPS_ERR_BAD_ARG;
    for (const GopsRnn* n : {on, tg}) {
        const int rc = rnn_check(*n, B);
        if (rc != GOPS_OK) return rc;
    }
    const GopsMlp &a = on->head[0], &b = tg->head[0];
    if (on->seq_len != tg->seq_len || on->obs_dim != tg->obs_dim || on->hidden != tg->hidden || a.n_layers != b.n_layers) return GOPS_ERR_UNSUPPORTED;
    for (int l = 0; l <= a.n_layers; ++l)
        if (a.sizes[l] != b.sizes[l]) return GOPS_ERR_UNSUPPORTED;
    if (d->act_num < 2 || d->act_num > GOPS_DQN_MAX_ACTIONS || a.sizes[a.n_layers] != d->act_num) return GOPS_ERR_UNSUPPORTED;
    return GOPS_OK;
}

// the call's scratch: the tiles' partial sums [tiles][3] doubles, then the ticket
size_t rnn_dqn_part_bytes(int B) { return align256((size_t)((B + TB - 1) / TB) * 3 * sizeof(double)); }

}  // namespace

extern "C" {

size_t gops_rnn_dqn_step_workspace_bytes(const GopsRnn* online, const GopsRnn* target, const GopsRnnDqn* desc, int32_t B) {
    if (rnn_dqn_check(online, target, desc, B) != GOPS_OK) return 0;
    return rnn_dqn_part_bytes(B) + 256;
}

int gops_rnn_dqn_step(const GopsRnn* online, const GopsRnn* target, const GopsRnnDqn* desc, int32_t B, const float* obs, const float* obs2,
                      const float* act, const float* rew, const float* done, const float* weight, float* q_all, float* backup,
                      int32_t* a_star, float* seed, float* abs_err, float* stats, void* rnn_ws, size_t rnn_ws_bytes, void* ws,
                      size_t ws_bytes, void* stream) {
    const int rc = rnn_dqn_check(online, target, desc, B);
    if (rc != GOPS_OK) return rc;
    if (!obs || !obs2 || !act || !rew || !done || !q_all || !backup || !a_star || !seed || !abs_err || !stats) return GOPS_ERR_BAD_ARG;
    if (rnn_ws == nullptr || rnn_ws_bytes < rnn_plan(*online, B, nullptr).bytes) return GOPS_ERR_WORKSPACE;
    if (ws == nullptr || ws_bytes < rnn_dqn_part_bytes(B) + 256 || !stats_aligned(ws)) return GOPS_ERR_WORKSPACE;
    const RnnPlan pl = rnn_plan(*online, B, rnn_ws);
    RnnDqnParams q = {};
    q.net[0] = pl.dev;
    q.net[1] = rnn_plan(*target, B, nullptr).dev;   // (no workspace: no stash pointers)
    q.x[0] = obs; q.x[1] = obs2;
    q.act = act; q.rew = rew; q.done = done; q.weight = weight;
    q.q_all = q_all; q.backup = backup; q.a_star = a_star; q.seed = seed; q.abs_err = abs_err; q.stats = stats;
    q.part = static_cast<double*>(ws);
    q.ticket = reinterpret_cast<unsigned*>(static_cast<char*>(ws) + rnn_dqn_part_bytes(B));
    q.rscale = desc->reward_scale; q.gamma = desc->gamma;
    q.gsc = (float)(2.0 / B);
    q.N = desc->act_num;
    const size_t lds = 2 * pl.lds_fwd + (2 * TB * RD_LDQ + RD_FOLD_FLOATS) * sizeof(float);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (online->hidden <= 64) launch_with_lds(rnn_dqn_kernel<1>, dim3(pl.ntiles), dim3(RD_THREADS), lds, s, q);
    else launch_with_lds(rnn_dqn_kernel<2>, dim3(pl.ntiles), dim3(RD_THREADS), lds, s, q);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? GOPS_OK : (int)e;
}

}  // extern "C"
