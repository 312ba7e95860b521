// Host side of the rollout / value / MLP family of the C ABI (include/gops_hip.h) - gops_rollout_*, gops_value_*, gops_mlp_*,
// gops_dw_plan_query - with gops_hip_version and gops_profile_*: argument checking, workspace carving, launch sequencing.  Every
// other entry point is defined, with all of its checks, in the source that holds its kernels (launchers.h names what the sources
// call in one another).  Nothing here allocates device memory or synchronises the stream.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "common.h"
#include "launchers.h"
#include "rollout_choice.h"

// One hipFuncSetAttribute per kernel (common.h: launch_with_lds).
bool lds_attr_needed(const void* kernel) {
    static std::mutex mu;
    static std::vector<const void*> seen;
    std::lock_guard<std::mutex> lk(mu);
    for (const void* k : seen)
        if (k == kernel) return false;
    seen.push_back(kernel);
    return true;
}

namespace {

inline int pad16(int x) { return (x + 15) & ~15; }
inline int pad32(int x) { return (x + 31) & ~31; }
constexpr size_t kAlign = 256;   // bytes

// ---- opt-in kernel timing (bench.py) ---------------------------------------------------------
struct ProfState {
    std::mutex mu;
    bool on = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[6];   // 0-2: rollout fwd / bwd / dW; 3-5: the same for plain MLP batches (value net)
} g_prof;

struct ProfScope {
    int id;
    hipStream_t s;
    hipEvent_t a = nullptr, b = nullptr;
    ProfScope(int id_, hipStream_t s_) : id(id_), s(s_) {
        if (g_prof.on) {
            (void)hipEventCreate(&a);
            (void)hipEventCreate(&b);
            (void)hipEventRecord(a, s);
        }
    }
    ~ProfScope() {
        if (a != nullptr) {
            (void)hipEventRecord(b, s);
            std::lock_guard<std::mutex> lk(g_prof.mu);
            g_prof.ev[id].emplace_back(a, b);
        }
    }
};

// ---- workspace plan ----------------------------------------------------------------------------
struct Carver {
    char* base;
    size_t off = 0;
    explicit Carver(void* b) : base(static_cast<char*>(b)) {}
    float* take(size_t nfloats) {
        off = (off + kAlign - 1) / kAlign * kAlign;
        float* p = base ? reinterpret_cast<float*>(base + off) : nullptr;
        off += nfloats * sizeof(float);
        return p;
    }
};

// Phase counters of block 0 (make dbg: GOPS_DBG_BUILD; tools/dbg_run.py with GOPS_DBG_TIMING=1): 16 counters per direction
// (`slot` 0: forward, 1: backward), or null.  The product library reads no environment and allocates nothing here.
unsigned long long* dbg_timing_buffer(int slot) {
#ifdef GOPS_DBG_BUILD
    static unsigned long long* const buf = [] {
        unsigned long long* b = nullptr;
        if (getenv("GOPS_DBG_TIMING") != nullptr) (void)hipMalloc(&b, 32 * sizeof(unsigned long long));
        return b;
    }();
    return buf != nullptr ? buf + 16 * slot : nullptr;
#else
    (void)slot;
    return nullptr;
#endif
}

int check_mlp(const GopsMlp& m, int in_dim, int out_dim, bool f16) {
    if (m.n_layers < 2 || m.n_layers > GOPS_MAX_LAYERS) return GOPS_ERR_UNSUPPORTED;
    if (m.sizes[0] != in_dim || m.sizes[m.n_layers] != out_dim) return GOPS_ERR_BAD_ARG;
    if (out_dim < 1 || out_dim > GOPS_MAX_ACT) return GOPS_ERR_UNSUPPORTED;
    for (int j = 1; j < m.n_layers; ++j)
        if (m.sizes[j] < 16 || (m.sizes[j] & (f16 ? 63 : 15))) return GOPS_ERR_UNSUPPORTED;
    if (m.hidden_act < GOPS_ACT_LINEAR || m.hidden_act > GOPS_ACT_TANH) return GOPS_ERR_BAD_ARG;
    for (int j = 0; j < m.n_layers; ++j)
        if (m.weight[j] == nullptr || m.bias[j] == nullptr) return GOPS_ERR_BAD_ARG;
    return GOPS_OK;
}

void fill_mlp(MlpDev& d, const GopsMlp& m) {
    memset(&d, 0, sizeof(d));
    d.nl = m.n_layers;
    d.act = m.hidden_act;
    for (int j = 0; j <= m.n_layers; ++j) d.dims[j] = m.sizes[j];
    for (int j = 0; j < m.n_layers; ++j) {
        d.kp[j] = pad16(m.sizes[j]);
        d.kp32[j] = pad32(m.sizes[j]);
        d.w[j] = m.weight[j];
        d.b[j] = m.bias[j];
    }
}

void carve_packs(Carver& c, MlpDev& d, bool f16) {
    for (int j = 0; j < d.nl - 1; ++j) {
        if (f16) {   // half fragments: N x kp32 elements each (2 per float)
            const size_t n = ((size_t)d.dims[j + 1] * d.kp32[j] + 1) / 2;
            d.wph[j] = reinterpret_cast<const f16x8*>(c.take(n));
            d.wpth[j] = reinterpret_cast<const f16x8*>(c.take(n));
            continue;
        }
        const size_t n = (size_t)d.dims[j + 1] * d.kp[j];
        d.wp[j] = reinterpret_cast<const f32x4*>(c.take(n));
        d.wpt[j] = reinterpret_cast<const f32x4*>(c.take(n));
    }
}

struct Plan {
    RolloutParams p;
    RolloutChoice choice;                  // which kernels run (rollout_choice.h); p's variant fields are copies of it
    RolloutParams* dev_params = nullptr;   // device copy read by the rollout kernels
    DwLayer dw[GOPS_MAX_LAYERS];              // the weight-gradient stage, one record per Linear layer (dw_plan.h)
    float* dw_part[GOPS_MAX_LAYERS] = {};     // split-K partial slabs, one region per Linear layer
    float* dw_part_b[GOPS_MAX_LAYERS] = {};
    float* dummy = nullptr;                   // open loop: stand-in policy weights
    size_t dummy_floats = 0;
    size_t bytes = 0;
};

// Builds kernel parameters and carves the workspace.  ws == nullptr: size query only.
int build_plan(const GopsRolloutDesc& desc, void* ws, Plan& plan) {
    RolloutParams& p = plan.p;
    memset(&p, 0, sizeof(p));
    const GopsEnv& e = desc.env;
    if (desc.batch < 1 || desc.horizon < 1 || desc.horizon > GOPS_MAX_HORIZON) return GOPS_ERR_BAD_ARG;
    if (desc.variant_flags & ~GOPS_VF_ALL) return GOPS_ERR_BAD_ARG;   // a retired or unknown bit is refused, not ignored (ABI v14)
    if (e.kind < GOPS_ENV_NONE || e.kind > GOPS_ENV_MOUNTAINCAR) return GOPS_ERR_BAD_ARG;
    if (e.obs_dim < 1 || e.data_env) return GOPS_ERR_BAD_ARG;   // data-env semantics exist for gops_env_step only
    const int pol_out = (e.kind == GOPS_ENV_NONE) ? 1 : e.act_dim;
    if (desc.dtype != GOPS_DTYPE_F32 && desc.dtype != GOPS_DTYPE_F16) return GOPS_ERR_BAD_ARG;
    const bool f16 = desc.dtype == GOPS_DTYPE_F16;
    int rc = GOPS_OK;
    if (desc.open_loop) {   // no policy inside the rollout (FHADP2)
        if (e.kind == GOPS_ENV_NONE || desc.tail_value || desc.finite_horizon || f16) return GOPS_ERR_BAD_ARG;
    } else if ((rc = check_mlp(desc.policy, e.obs_dim + (desc.finite_horizon ? 1 : 0), pol_out, f16)) != GOPS_OK) {
        return rc;
    }
    if (desc.tail_value && (rc = check_mlp(desc.value, e.obs_dim, 1, f16)) != GOPS_OK) return rc;
    if (e.kind == GOPS_ENV_NONE && (desc.horizon != 1 || desc.tail_value || desc.finite_horizon)) return GOPS_ERR_BAD_ARG;
    if (e.scale_obs && e.kind != GOPS_ENV_LQ && e.kind != GOPS_ENV_IDPENDULUM && e.kind < GOPS_ENV_CARTPOLE) return GOPS_ERR_UNSUPPORTED;   // obs_dim <= 8 only
    if (e.kind == GOPS_ENV_CARTPOLE && (e.obs_dim != 4 || e.act_dim != 1)) return GOPS_ERR_BAD_ARG;
    if (e.kind == GOPS_ENV_PENDULUM && (e.obs_dim != 3 || e.act_dim != 1)) return GOPS_ERR_BAD_ARG;
    if (e.kind == GOPS_ENV_MOUNTAINCAR && mcar_check_env(e) != GOPS_OK) return GOPS_ERR_BAD_ARG;
    if (e.kind == GOPS_ENV_VEH2DOF && (e.act_dim != 1 || e.pre_horizon < 1 || e.obs_dim != 4 + e.pre_horizon || e.clip_obs ||
                                        (e.cstr_err && e.n_constraint != 1))) return GOPS_ERR_BAD_ARG;
    if (e.kind == GOPS_ENV_MOBILEROBOT && (e.obs_dim != MOB_OBS || e.act_dim != 2 || e.n_constraint != 1 || e.scale_obs)) return GOPS_ERR_BAD_ARG;
    if (e.kind >= GOPS_ENV_CARTPOLE && f16) return GOPS_ERR_UNSUPPORTED;   // the half-precision kernels are built for the BASELINE envs
    if (e.kind == GOPS_ENV_LQ && (e.obs_dim > GOPS_MAX_LQ_STATE || e.act_dim > GOPS_MAX_ACT)) return GOPS_ERR_UNSUPPORTED;
    if (e.kind == GOPS_ENV_IDPENDULUM && (e.obs_dim != 6 || e.act_dim != 1 || e.clip_obs)) return GOPS_ERR_BAD_ARG;
    if (e.kind == GOPS_ENV_VEH3DOFCONTI &&
        (e.act_dim != 2 || e.pre_horizon < 1 || e.obs_dim != 6 + 4 * e.pre_horizon || e.clip_obs))
        return GOPS_ERR_BAD_ARG;
    if (e.kind == GOPS_ENV_VEH3DOF_SURR &&
        (e.act_dim != 2 || e.pre_horizon < 1 || e.n_surr < (e.cstr_err ? 0 : 1) || e.n_surr > (e.cstr_err ? 0 : GOPS_MAX_SURR) ||
         (e.cstr_err ? e.n_constraint != 2 : (e.n_constraint != 1 && e.n_constraint != 3)) ||
         e.obs_dim != 6 + 4 * e.pre_horizon + 4 * e.n_surr || e.clip_obs ||
         (e.surr_penalty && (e.n_surr != 1 || e.n_constraint != 1)) ||
         desc.open_loop == 1 || desc.dtype != GOPS_DTYPE_F32))   // (open_loop 2: OptController's raw-action rollouts)
        return GOPS_ERR_BAD_ARG;
    if (e.clip_obs && e.obs_dim > (e.kind == GOPS_ENV_MOBILEROBOT ? GOPS_MAX_CLIP_OBS : 8)) return GOPS_ERR_UNSUPPORTED;
    if (e.repeat_num < 0 || e.repeat_num > GOPS_MAX_REPEAT) return GOPS_ERR_BAD_ARG;
    if (e.repeat_num > 1 && (f16 || (e.kind != GOPS_ENV_LQ && e.kind != GOPS_ENV_IDPENDULUM && e.kind != GOPS_ENV_CARTPOLE &&
                                     e.kind != GOPS_ENV_PENDULUM && e.kind != GOPS_ENV_MOUNTAINCAR)))
        return GOPS_ERR_UNSUPPORTED;   // ActionRepeatModel: obs == state models, fp32

    p.B = desc.batch;
    p.H = desc.horizon;
    p.fh = desc.finite_horizon ? 1 : 0;
    p.need_grad = desc.need_grad ? 1 : 0;
    p.tail = desc.tail_value ? 1 : 0;
    p.tail_unmasked = (desc.tail_value && desc.tail_unmasked) ? 1 : 0;
    p.env = e;
    lq_pad_env(p.env);   // (env_models.h: the LQ matrices with compile-time strides)
    fill_ref_defaults(p.env);   // (common.h, like lq_pad_env)
    p.open_loop = desc.open_loop == 2 ? 2 : (desc.open_loop ? 1 : 0);
    p.f16 = f16 ? 1 : 0;
    p.vflags = desc.variant_flags;
    p.dw_wgs = desc.dw_workgroups > 0 ? desc.dw_workgroups : 512;
    if (p.open_loop) {
        // The kernels keep their tile / stash bookkeeping in terms of a policy: give them the
        // smallest one (obs -> 16 -> act, weights zeroed in the workspace); its layers are never
        // evaluated, only the observation stash (env adjoints read it) is live.
        GopsMlp dummy;
        memset(&dummy, 0, sizeof(dummy));
        dummy.n_layers = 2;
        dummy.sizes[0] = e.obs_dim; dummy.sizes[1] = 16; dummy.sizes[2] = e.act_dim;
        dummy.hidden_act = GOPS_ACT_RELU;
        fill_mlp(p.pol, dummy);
    } else {
        fill_mlp(p.pol, desc.policy);
    }
    if (p.tail) fill_mlp(p.val, desc.value);
    int kp0 = p.pol.kp[0], hmax = 16;
    if (p.tail && p.val.kp[0] > kp0) kp0 = p.val.kp[0];
    for (int j = 1; j < p.pol.nl; ++j) hmax = p.pol.dims[j] > hmax ? p.pol.dims[j] : hmax;
    if (p.tail)
        for (int j = 1; j < p.val.nl; ++j) hmax = p.val.dims[j] > hmax ? p.val.dims[j] : hmax;
    p.ldx = kp0 + 4;
    p.ldh = hmax + 4;
    const bool veh = env_has_ref_table(e.kind);
    const int ref_pts = ref_points_in_lds(p, false);
    if (rollout_fwd_lds_bytes(p.ldx, p.ldh, ref_pts, f16, 0) > 160 * 1024 || rollout_bwd_lds_bytes(p.ldx, p.ldh, ref_pts, f16, false) > 160 * 1024)
        return GOPS_ERR_UNSUPPORTED;
    RolloutChoice& ch = plan.choice;
    if (!choose_forward(p, ch)) return GOPS_ERR_UNSUPPORTED;
    p.touch_mode = desc.l2_warmup > 0 ? desc.l2_warmup - 1 : ch.touch_mode;   // (tuning knob)
    p.sp.on = ch.split, p.h64 = ch.h64, p.ss = ch.ss, p.ssb = ch.ssb, p.tail_fp32 = ch.tail_fp32;
    p.narrow = ch.narrow, p.narrow_floats = ch.narrow_floats, p.narrow_off_fwd = ch.narrow_off_fwd, p.narrow_off_bwd = ch.narrow_off_bwd;
    const int tile_rows = p.h64 ? 64 : TB;
    for (int t = 0; t <= p.H; ++t) p.gpow[t] = (float)pow(desc.gamma, (double)t);

    Carver c(ws);
    plan.dev_params = reinterpret_cast<RolloutParams*>(c.take((sizeof(RolloutParams) + 3) / 4));
    if (p.open_loop) {   // zeroed stand-in weights (run_forward clears them)
        plan.dummy_floats = (size_t)16 * p.pol.dims[0] + 16 + (size_t)p.pol.dims[2] * 16 + p.pol.dims[2];
        float* z = c.take(plan.dummy_floats);
        plan.dummy = z;
        p.pol.w[0] = z; p.pol.b[0] = z + (size_t)16 * p.pol.dims[0];
        p.pol.w[1] = p.pol.b[0] + 16; p.pol.b[1] = p.pol.w[1] + (size_t)p.pol.dims[2] * 16;
    }
    carve_packs(c, p.pol, f16);
    if (p.tail) carve_packs(c, p.val, f16);
    if (p.sp.on) {   // plane-split operands (2 bytes per element and plane) + one scale per n-tile
        SplitDev& sp = p.sp;
        const int n1 = p.pol.dims[1], n2 = p.pol.dims[2];
        sp.kc[0] = p.pol.kp32[0] >> 5;
        sp.kc[1] = n1 >> 5;
        auto take_pair = [&](size_t elems, const bf16x8*& w1, const f16x8*& r) {
            w1 = reinterpret_cast<const bf16x8*>(c.take((elems + 1) / 2));
            r = reinterpret_cast<const f16x8*>(c.take((elems + 1) / 2));
        };
        take_pair((size_t)n1 * 32 * sp.kc[0], sp.w1[0], sp.r[0]);
        take_pair((size_t)n2 * 32 * sp.kc[1], sp.w1[1], sp.r[1]);
        take_pair((size_t)n1 * n2, sp.w1t[1], sp.rt[1]);                 // tiles over the n1 inputs of layer 1, slots over its n2 outputs
        take_pair((size_t)p.pol.kp[0] * n1, sp.w1t[0], sp.rt[0]);        // tiles over the (16-padded) inputs of layer 0, slots over its n1 outputs
        sp.inv[0] = c.take(n1 >> 4);
        sp.inv[1] = c.take(n2 >> 4);
        sp.invt[1] = c.take(n1 >> 4);
        sp.invt[0] = c.take(p.pol.kp[0] >> 4);
    }
    if (p.ss) {   // streamed-split forward: planes of every hidden layer of the policy (and of the tail value net)
        for (int m = 0; m < (p.tail ? 2 : 1); ++m) {
            const MlpDev& d = m ? p.val : p.pol;
            SplitNetDev& sn = m ? p.ssv : p.ssp;
            for (int j = 0; j < d.nl - 1; ++j) {
                sn.kc[j] = (j == 0) ? ss_kc0(d.kp32[0]) : d.dims[j] >> 5;
                const size_t elems = (size_t)d.dims[j + 1] * 32 * sn.kc[j];
                sn.w1[j] = reinterpret_cast<const bf16x8*>(c.take((elems + 1) / 2));
                sn.r[j] = reinterpret_cast<const f16x8*>(c.take((elems + 1) / 2));
                sn.inv[j] = c.take(d.dims[j + 1] >> 4);
            }
        }
    }
    // the sweep of the same launch on the streamed-split kernel too: transposed planes (n-tiles over a layer's inputs)
    if (p.ssb) {
        for (int m = 0; m < (p.tail ? 2 : 1); ++m) {
            const MlpDev& d = m ? p.val : p.pol;
            SplitNetDev& sn = m ? p.ssvt : p.sspt;
            for (int j = 0; j < d.nl - 1; ++j) {
                const int nin = (j == 0) ? d.kp[0] : d.dims[j];   // (16-padded) inputs of the layer = columns of the transposed operand
                sn.kc[j] = d.dims[j + 1] >> 5;
                const size_t elems = (size_t)nin * d.dims[j + 1];
                sn.w1[j] = reinterpret_cast<const bf16x8*>(c.take((elems + 1) / 2));
                sn.r[j] = reinterpret_cast<const f16x8*>(c.take((elems + 1) / 2));
                sn.inv[j] = c.take(nin >> 4);
            }
        }
    }
    p.gscale = c.take(8);   // [4 ..]: the fused Adam step's scalar factors (adam_snapshot); [0 .. 1]: max|grad_v| / max|delta_y| of a backward launch (f16 sweep scale; delta scale of the weight-gradient GEMM)
    // stash rows: every tile stores all 16 rows of every step (tile-major order)
    const long long S = (long long)((p.B + tile_rows - 1) / tile_rows) * tile_rows * p.H;
    if (veh) p.ref_table = c.take((size_t)p.B * (e.pre_horizon + 1 + p.H) * 4);
    if (e.kind == GOPS_ENV_VEH3DOF_SURR)
        p.surr_table = reinterpret_cast<const f32x4*>(c.take((size_t)p.B * (p.H + 1) * e.n_surr * 4));
    if (p.need_grad) {
        const bool gelu = p.pol.act == GOPS_ACT_GELU;
        const size_t el = f16 ? 2 : 1;   // stash elements per float of workspace (half: 2)
        p.st.x = c.take(((size_t)S * (f16 ? p.pol.kp32[0] : p.pol.kp[0]) + el - 1) / el);
        if (f16) p.st.xf = c.take((size_t)S * 8);
        for (int j = 1; j < p.pol.nl; ++j) {
            p.st.h[j] = c.take(((size_t)S * p.pol.dims[j] + el - 1) / el);
            p.st.d[j] = c.take(((size_t)S * p.pol.dims[j] + el - 1) / el);
            if (gelu) p.st.z[j] = c.take(((size_t)S * p.pol.dims[j] + el - 1) / el);
        }
        p.st.dy = c.take((size_t)S * 4);
        p.st.env = c.take((size_t)S * ENV_STASH);
        if (ch.idp_parking) p.st.idp = c.take((size_t)S * IDP_PARK);
        if (p.tail) {
            for (int j = 1; j < p.val.nl; ++j) {
                const size_t rows = (size_t)((p.B + tile_rows - 1) / tile_rows) * tile_rows;   // whole tiles (FM stash tiles are written whole)
                p.st.tail_h[j] = c.take((rows * p.val.dims[j] + el - 1) / el);
                if (p.val.act == GOPS_ACT_GELU) p.st.tail_z[j] = c.take((rows * p.val.dims[j] + el - 1) / el);
            }
        }
        p.st.tail_done = c.take((size_t)p.B);
        // split-K partial slabs of the weight-gradient GEMMs: one region per layer so that all
        // partial sums can be reduced by a single launch at the end
        const int Lh = p.pol.nl - 1;
        for (int j = 0; j < Lh; ++j) plan.dw[j] = plan_dw(p.pol.dims[j + 1], p.pol.dims[j], f16 ? p.pol.kp32[j] : p.pol.kp[j], S, f16, p.dw_wgs);
        plan.dw[Lh] = plan_dw_out(p.pol.dims[Lh], p.pol.dims[Lh + 1], S);
        if (ch.fuse_dw0) {   // ... or one slab [N][H64_W0_COLS] / [N] per workgroup of the 64-row sweep (rollout_h64.hip)
            DwLayer& d = plan.dw[0];
            d.slab_w = std::max(d.slab_w, (size_t)h64_sweep_grid(p) * d.N * H64_W0_COLS);
            d.slab_b = std::max(d.slab_b, (size_t)h64_sweep_grid(p) * d.N);
        }
        for (int j = 0; j <= Lh; ++j) {
            plan.dw_part[j] = c.take(plan.dw[j].slab_w);
            plan.dw_part_b[j] = c.take(plan.dw[j].slab_b);
        }
    }
    plan.bytes = c.off + kAlign;
    return GOPS_OK;
}

// The phase-counter tables of `make dbg` (tools/dbg_run.py), one per direction; nothing in the product library.
#ifdef GOPS_DBG_BUILD
void dbg_print_forward(const RolloutParams& p) {
    if (p.dbg == nullptr) return;
    unsigned long long h[16];
    (void)hipMemcpy(h, p.dbg, sizeof(h), hipMemcpyDeviceToHost);
    if (p.h64)
        fprintf(stderr, "[gops dbg] fwd 64-row half cycles/step: top+sync %llu | convert+xstash+sync %llu | L0 gemm %llu epi %llu sync %llu | "
                "L1 gemm %llu epi %llu sync %llu | head %llu sync %llu | env %llu\n",
                h[0] / p.H, h[1] / p.H, h[2] / p.H, h[3] / p.H, h[4] / p.H, h[5] / p.H, h[6] / p.H, h[7] / p.H, h[8] / p.H, h[9] / p.H, h[10] / p.H);
    else if (p.ss)   // (grid-stride launches: the counters add up over the tiles block 0 walked)
        fprintf(stderr, "[gops dbg] fwd streamed-split cycles/step (x tiles of block 0): top+sync %llu | planes of X+sync %llu | L0 gemm %llu | "
                "epilogues %llu | plane store+sync %llu | L1.. gemm %llu sync %llu | head partials+combine %llu | tanh+wrap %llu sync %llu | "
                "envstash %llu | env %llu\n", h[0] / p.H, h[1] / p.H, h[14] / p.H, h[8] / p.H, h[12] / p.H, h[11] / p.H, h[9] / p.H, h[2] / p.H,
                h[7] / p.H, h[3] / p.H, h[4] / p.H, h[5] / p.H);
    else if (p.sp.on)
        fprintf(stderr, "[gops dbg] fwd SPLIT cycles/step: top+sync %llu | xstash+convert+sync %llu | gemm0 %llu | epi0+planes %llu | sync %llu | "
                "gemm1 %llu | epi1+head fma %llu | head reduce %llu | sync+combine %llu | tanh+wrap %llu | sync %llu | envstash %llu | env %llu || sum %llu\n",
                h[0] / p.H, h[1] / p.H, h[14] / p.H, h[8] / p.H, h[9] / p.H, h[11] / p.H, h[12] / p.H, h[2] / p.H, h[6] / p.H, h[7] / p.H,
                h[3] / p.H, h[4] / p.H, h[5] / p.H,
                (h[0] + h[1] + h[14] + h[8] + h[9] + h[11] + h[12] + h[2] + h[6] + h[7] + h[3] + h[4] + h[5]) / p.H);
    if (p.sp.on) fprintf(stderr, "[gops dbg] fwd SPLIT per launch (cycles of block 0): kernel entry -> first step %llu | behind the last step %llu\n", h[13], h[15]);
    else
    fprintf(stderr, "[gops dbg] fwd cycles/step: top+sync %llu | xstash %llu | hidden-rest %llu | head %llu | envstash %llu | env %llu"
            " || L0 epi %llu sync %llu stash %llu | L1 epi %llu sync %llu stash %llu | gemm(L0+L1) %llu || head: dot %llu tanh+wrap %llu barrier %llu\n",
            h[0] / p.H, h[1] / p.H, h[2] / p.H, h[3] / p.H, h[4] / p.H, h[5] / p.H, h[8] / p.H, h[9] / p.H,
            h[10] / p.H, h[11] / p.H, h[12] / p.H, h[13] / p.H, h[14] / p.H, h[6] / p.H, h[7] / p.H, h[3] / p.H);
}
void dbg_print_backward(const RolloutParams& p) {
    if (p.dbg == nullptr) return;
    unsigned long long h[16];
    (void)hipMemcpy(h, p.dbg, sizeof(h), hipMemcpyDeviceToHost);
    if (p.h64)
        fprintf(stderr, "[gops dbg] bwd 64-row half cycles/step: env adjoint %llu sync %llu | head %llu sync %llu | gemm %llu sync %llu epi %llu sync %llu | "
                "g_x %llu | end sync %llu\n", h[0] / p.H, h[1] / p.H, h[2] / p.H, h[3] / p.H, h[4] / p.H, h[5] / p.H, h[6] / p.H, h[7] / p.H, h[8] / p.H,
                h[9] / p.H);
    else if (p.sp.on)
        fprintf(stderr, "[gops dbg] bwd SPLIT cycles/step: top %llu | env points %llu | reduce+sync %llu | env finish+sync %llu | head delta+planes %llu | "
                "sync %llu | hook %llu | gemm1+epi+planes %llu | sync %llu | gemm0+G %llu | end sync %llu || sum %llu\n",
                h[0] / p.H, h[10] / p.H, h[11] / p.H, h[1] / p.H, h[3] / p.H, h[4] / p.H, h[5] / p.H, h[6] / p.H, (h[7] + h[8]) / p.H, h[9] / p.H,
                h[2] / p.H, (h[0] + h[10] + h[11] + h[1] + h[3] + h[4] + h[5] + h[6] + h[7] + h[8] + h[9] + h[2]) / p.H);
    else
    fprintf(stderr, "[gops dbg] bwd cycles/step: touch %llu | env(points %llu, reduce+sync %llu, finish %llu) | head-bwd %llu sync %llu stash %llu | "
            "gemm1+epi %llu sync %llu stash %llu | gemm0+epi %llu | end sync %llu\n",
            h[0] / p.H, h[10] / p.H, h[11] / p.H, h[1] / p.H, h[3] / p.H, h[4] / p.H, h[5] / p.H, h[6] / p.H, h[7] / p.H,
            h[8] / p.H, h[9] / p.H, h[2] / p.H);
}
#else
inline void dbg_print_forward(const RolloutParams&) {}
inline void dbg_print_backward(const RolloutParams&) {}
#endif

int run_forward(const GopsRolloutDesc& desc, const GopsRolloutIn& in, const GopsRolloutOut& out,
                void* ws, size_t ws_bytes, hipStream_t s) {
    Plan plan;
    int rc = build_plan(desc, ws, plan);
    if (rc != GOPS_OK) return rc;
    if (ws == nullptr || ws_bytes < plan.bytes) return GOPS_ERR_WORKSPACE;
    if (in.obs == nullptr || out.v_pi == nullptr) return GOPS_ERR_BAD_ARG;
    if (env_has_ref_table(desc.env.kind) &&
        (!in.state || !in.ref_points || !in.path_num || !in.u_num || !in.ref_time)) return GOPS_ERR_BAD_ARG;
    if (desc.env.kind == GOPS_ENV_VEH3DOF_SURR && desc.env.n_surr > 0 && !in.surr_state) return GOPS_ERR_BAD_ARG;
    RolloutParams& p = plan.p;
    p.in = in;
    p.out = out;
    if (p.open_loop) {
        if (in.head_pre == nullptr) return GOPS_ERR_BAD_ARG;
        hipError_t me = launch_fill_zero(plan.dummy, plan.dummy_floats, s);
        if (me != hipSuccess) return (int)me;
    }
    p.dbg = dbg_timing_buffer(0);
    // parameter block upload + weight packing + reference table: one launch
    hipError_t ue = launch_prologue(p, plan.dev_params, desc.env.pre_horizon, pdt_of(desc.env), s);
    if (ue != hipSuccess) return (int)ue;
    int ret;
    {
        ProfScope scope(desc.env.kind == GOPS_ENV_NONE ? 3 : 0, s);
        ret = (int)launch_rollout_fwd(p, plan.choice.fwd, plan.dev_params, s);
    }
    dbg_print_forward(p);
    return ret;
}

// What an extern "C" entry point hands to run_backward beyond the description and the workspace.
struct BackwardCall {
    const GopsRolloutIn* in = nullptr;
    const float* grad_v = nullptr;
    const GopsMlpGrad* grad = nullptr;         // parameter gradients (read when want_params)
    bool want_params = true;
    float* g_head_pre = nullptr;               // open loop: gradient of the raw actions
    const float* ext_delta = nullptr;          // gops_mlp_backward: the head is a stand-in, its gradient is not formed
    const GopsRolloutAdjoint* adj = nullptr;   // gops_rollout_backward_adj / gops_mlp_backward_x
    const GopsUpdateTail* tail = nullptr;      // gops_rollout_backward_update
};

// GOPS_VF_BWD_PHASE_A / _B: the call is one half of a backward (see gops_hip.h) - phase A: sweep and every layer but 0,
// phase B: no sweep, layer 0 (both bits: a whole backward)
struct Phase {
    bool only_a, only_b;
    explicit Phase(unsigned vflags)
        : only_a((vflags & (GOPS_VF_BWD_PHASE_A | GOPS_VF_BWD_PHASE_B)) == GOPS_VF_BWD_PHASE_A),
          only_b((vflags & (GOPS_VF_BWD_PHASE_A | GOPS_VF_BWD_PHASE_B)) == GOPS_VF_BWD_PHASE_B) {}
};

// gops_rollout_backward_update's tail
int check_update_tail(const GopsRolloutDesc& desc, const RolloutParams& p, const BackwardCall& c) {
    const GopsUpdateTail* tail = c.tail;
    if (p.open_loop || !c.want_params || c.ext_delta != nullptr || c.adj != nullptr) return GOPS_ERR_BAD_ARG;
    // half a backward (GOPS_VF_BWD_PHASE_A / _B: a data-parallel update all-reduces between gradient and optimizer step) can carry
    // the LOSS MEAN on phase A's reduce launch - it needs no gradient - but never an optimizer / Polyak step
    const unsigned ph = desc.variant_flags & (GOPS_VF_BWD_PHASE_A | GOPS_VF_BWD_PHASE_B);
    if (ph != 0 && (ph != GOPS_VF_BWD_PHASE_A || tail->adam != nullptr || tail->polyak != nullptr)) return GOPS_ERR_BAD_ARG;
    if (tail->mean_x != nullptr && (tail->mean_stats == nullptr || tail->mean_n < 1)) return GOPS_ERR_BAD_ARG;
    if (tail->adam != nullptr) {
        const GopsAdamTensors& T = *tail->adam;
        if (tail->adam_state == nullptr || T.n != 2 * p.pol.nl) return GOPS_ERR_BAD_ARG;
        for (int j = 0; j < p.pol.nl; ++j) {   // every gradient tensor of the policy has its parameter / moments in the table
            const long long nw = (long long)p.pol.dims[j + 1] * p.pol.dims[j], nb = p.pol.dims[j + 1];
            int fw = -1, fb = -1;
            for (int k = 0; k < T.n; ++k) {
                if (T.grad[k] == c.grad->weight[j] && T.numel[k] == nw) fw = k;
                if (T.grad[k] == c.grad->bias[j] && T.numel[k] == nb) fb = k;
            }
            if (fw < 0 || fb < 0 || !T.param[fw] || !T.exp_avg[fw] || !T.exp_avg_sq[fw] || !T.param[fb] || !T.exp_avg[fb] || !T.exp_avg_sq[fb])
                return GOPS_ERR_BAD_ARG;
        }
    }
    if (tail->polyak != nullptr) {   // every online tensor of the averaging table is a parameter this call steps
        if (tail->adam == nullptr || tail->polyak->n != tail->adam->n) return GOPS_ERR_BAD_ARG;
        for (int k = 0; k < tail->polyak->n; ++k) {
            bool found = false;
            for (int i = 0; i < tail->adam->n; ++i)
                found = found || (tail->polyak->grad[k] == tail->adam->param[i] && tail->polyak->numel[k] == tail->adam->numel[i]);
            if (!found || tail->polyak->param[k] == nullptr) return GOPS_ERR_BAD_ARG;
        }
    }
    return GOPS_OK;
}

// Everything about a call that can be refused without knowing its kernels: checked before anything is launched
int check_backward_call(const GopsRolloutDesc& desc, const RolloutParams& p, const BackwardCall& c) {
    if ((p.open_loop != 0) != (c.g_head_pre != nullptr)) return GOPS_ERR_BAD_ARG;
    if (p.open_loop && c.in->head_pre == nullptr) return GOPS_ERR_BAD_ARG;
    if (c.ext_delta != nullptr && desc.env.kind != GOPS_ENV_NONE) return GOPS_ERR_BAD_ARG;
    if (!p.open_loop && c.want_params)
        for (int j = 0; j < p.pol.nl - (c.ext_delta != nullptr ? 1 : 0); ++j)
            if (c.grad->weight[j] == nullptr || c.grad->bias[j] == nullptr) return GOPS_ERR_BAD_ARG;
    int rc = GOPS_OK;
    if (c.tail != nullptr && (rc = check_update_tail(desc, p, c)) != GOPS_OK) return rc;
    if (c.adj != nullptr && (p.tail || p.f16)) return GOPS_ERR_UNSUPPORTED;   // (open loop: gops_rollout_backward_open_loop_adj)
    const Phase ph(p.vflags);
    if ((ph.only_a || ph.only_b) && (p.open_loop || !c.want_params || c.ext_delta != nullptr || c.adj != nullptr)) return GOPS_ERR_UNSUPPORTED;
    return GOPS_OK;
}

// Which kernel forms each layer's weight gradient in this call (plan.dw: dw_plan.h).  false: a sweep would write more slabs
// than the carve holds.
bool choose_dw_stage(Plan& plan, const BackwardCall& c, const SweepCall& call) {
    const RolloutParams& p = plan.p;
    const KernelChoice& sweep = plan.choice.bwd;
    if (p.open_loop || !c.want_params) return true;   // no parameters behind the rollout / none wanted: no layer takes part
    const Phase ph(p.vflags);
    const int L = p.pol.nl - 1;
    const bool own_sweep = c.adj == nullptr && c.ext_delta == nullptr;
    // Two-half-plane weight-gradient GEMM: its delta scale is derived from max|grad_v|, which bounds the deltas only when
    // grad_v is the sweep's one gradient source - a terminal observation adjoint or constraint-sum gradients can be orders of
    // magnitude larger, so those launches keep the exact three-plane product.  The penalty model's constraint outputs carry
    // no gradient (gops_hip.h): its seeds are not a gradient source, and must not change the result.
    const bool cstr_seeds = !(p.env.kind == GOPS_ENV_VEH3DOF_SURR && p.env.surr_penalty) &&
                            (c.in->grad_constraint != nullptr || c.in->grad_constraint_prod != nullptr || c.in->grad_constraint_step != nullptr);
    const bool scaled = own_sweep && !cstr_seeds;
    for (int j = 0; j < L; ++j) {   // dW_j = D_{j+1}^T * (j == 0 ? X : H_j)
        if ((ph.only_a && j == 0) || (ph.only_b && j != 0)) continue;   // (two-phase backward: layer 0 is phase B)
        if (j == 0 && plan.choice.fuse_dw0 && own_sweep && !(p.vflags & (GOPS_VF_BWD_PHASE_A | GOPS_VF_BWD_PHASE_B))) {
            // formed inside the 64-row sweep, one slab [N][H64_W0_COLS] per workgroup (h64_can_fuse_dw0: K <= H64_W0_COLS)
            if (!choose_dw_in_sweep(plan.dw[0], sweep.grid, H64_W0_COLS)) return false;
        } else {
            choose_dw_gemm(plan.dw[j], p.f16 != 0, scaled, p.vflags);
        }
    }
    if (c.ext_delta == nullptr && !ph.only_b) {
        // Split sweep: the output layer's weight gradient is accumulated inside the sweep (one partial [A][K] per workgroup) - no
        // dw_out pass.  (GELU: the sweep's act' operand is gelu'(z), so it fetches H_2 next to it.)  The streamed-split sweep does
        // the same for the env kinds whose instantiation has the registers (ssb_fuse_kind).
        if (!sweep_fuses_out(sweep, call)) choose_dw_out(plan.dw[L], p.f16 != 0);
        else if (!choose_dw_in_sweep(plan.dw[L], sweep.grid, plan.dw[L].K)) return false;
    }
    return true;
}

// What this call adds to the forward's device copy of the parameter block travels as a kernel argument (BwdPatch); only the
// half sweep, which needs max|grad_v| before it starts, still takes the upload launch - so the host copy `p` gets the same.
void fill_patch(Plan& plan, const BackwardCall& c, const SweepCall& call, BwdPatch& q) {
    RolloutParams& p = plan.p;
    const int L = p.pol.nl - 1;
    p.in = *c.in;
    p.grad_v = c.grad_v;
    p.g_head_pre = c.g_head_pre;
    p.ext_delta = c.ext_delta;
    p.ext = call.ext;
    if (c.adj != nullptr) {
        p.adj_gfo = c.adj->grad_final_obs;
        p.adj_gobs = c.adj->grad_obs;
        p.adj_first_only = (c.adj->first_step_only != 0 && p.H > 1) ? 1 : 0;
    }
    p.dbg = dbg_timing_buffer(1);
    if (sweep_fuses_out(plan.choice.bwd, call)) {
        p.sp.out_part = plan.dw_part[L];
        p.sp.out_part_b = plan.dw_part_b[L];
    }
    memset(&q, 0, sizeof(q));
    q.in = *c.in;
    q.grad_v = c.grad_v;
    q.g_head_pre = c.g_head_pre;
    q.ext_delta = c.ext_delta;
    q.adj_gfo = p.adj_gfo;
    q.adj_gobs = p.adj_gobs;
    q.adj_first_only = p.adj_first_only;
    q.out_part = p.sp.out_part;
    q.out_part_b = p.sp.out_part_b;
    q.dbg = p.dbg;
    if (plan.dw[0].kernel == DwKernel::InSweep) {
        q.w0_part = plan.dw_part[0];
        q.w0_part_b = plan.dw_part_b[0];
    }
    if (c.tail != nullptr && c.tail->adam != nullptr) {   // the sweep's thread 0 advances the optimizer state and leaves this step's factors
        q.ad_st = c.tail->adam_state;
        q.ad_snap = p.gscale + 4;
        q.ad_b1 = c.tail->beta1; q.ad_b2 = c.tail->beta2;
    }
}

hipError_t launch_sweep(const GopsRolloutDesc& desc, const Plan& plan, const BackwardCall& c, const BwdPatch& q, hipStream_t s) {
    const RolloutParams& p = plan.p;
    hipError_t e;
    if (p.adj_first_only && c.want_params) {   // the sweep writes the step-0 deltas only: the rest of the stash is zero
        const size_t S0 = (size_t)tiles(p) * TB * p.H;
        for (int j = 1; j < p.pol.nl; ++j)
            if ((e = launch_fill_zero(p.st.d[j], S0 * p.pol.dims[j], s)) != hipSuccess) return e;
        if ((e = launch_fill_zero(p.st.dy, S0 * 4, s)) != hipSuccess) return e;
    }
    if (Phase(p.vflags).only_b) return hipSuccess;   // the sweep ran in phase A
    if (p.f16 && (e = launch_upload_params(p, plan.dev_params, s)) != hipSuccess) return e;
    ProfScope scope(desc.env.kind == GOPS_ENV_NONE ? 4 : 1, s);
    return launch_rollout_bwd(p, plan.choice.bwd, plan.dev_params, q, s);
}

// One layer of the weight-gradient stage: its GEMM (none when the sweep formed the slabs) and its two reduce jobs
hipError_t launch_dw_layer(const DwLayer& d, const void* D, const void* X, float* part, float* part_b, const float* dscale, int rows,
                           float* gw, float* gb, ReduceJobs& jobs, hipStream_t s) {
    const hipError_t e = launch_dw(d, D, X, part, part_b, dscale, s);
    if (e == hipSuccess) add_reduce_jobs(jobs, d, part, part_b, rows, gw, gb);
    return e;
}

// The update's tail rides on the reduce: Adam per gradient element, the loss mean in one more block
void attach_update_tail(ReduceJobs& jobs, const GopsUpdateTail& tail, const RolloutParams& p) {
    if (tail.adam != nullptr) {
        const GopsAdamTensors& T = *tail.adam;
        for (int i = 0; i < jobs.n; ++i)
            for (int k = 0; k < T.n; ++k)
                if (T.grad[k] == jobs.out[i]) { jobs.ad_p[i] = T.param[k]; jobs.ad_m[i] = T.exp_avg[k]; jobs.ad_v[i] = T.exp_avg_sq[k]; }
        jobs.ad_snap = p.gscale + 4;
        jobs.ad_skipped = &tail.adam_state->skipped_nonfinite;
        jobs.ad_b1 = tail.beta1; jobs.ad_b2 = tail.beta2; jobs.ad_eps = (float)tail.eps;
        if (tail.polyak != nullptr) {
            for (int i = 0; i < jobs.n; ++i)
                for (int k = 0; k < tail.polyak->n; ++k)
                    if (jobs.ad_p[i] != nullptr && tail.polyak->grad[k] == jobs.ad_p[i]) jobs.pk_t[i] = tail.polyak->param[k];
            jobs.pk_omt = (float)(1.0 - tail.polyak_tau);
            jobs.pk_tau = (float)tail.polyak_tau;
        }
    }
    if (tail.mean_x != nullptr) {
        jobs.mean_x = tail.mean_x; jobs.mean_n = tail.mean_n; jobs.mean_sc = (float)tail.mean_scale; jobs.mean_stats = tail.mean_stats;
    }
}

int run_backward(const GopsRolloutDesc& desc, const BackwardCall& c, void* ws, size_t ws_bytes, hipStream_t s) {
    if (!desc.need_grad || c.grad_v == nullptr) return GOPS_ERR_BAD_ARG;
    Plan plan;
    int rc = build_plan(desc, ws, plan);
    if (rc != GOPS_OK) return rc;
    if (ws == nullptr || ws_bytes < plan.bytes) return GOPS_ERR_WORKSPACE;
    const RolloutParams& p = plan.p;
    if ((rc = check_backward_call(desc, p, c)) != GOPS_OK) return rc;
    // ActionRepeatModel, gops_rollout_backward_adj / gops_mlp_backward_x: the general (EXT) instantiations of the sweep
    const SweepCall call{desc.env.repeat_num > 1 || c.adj != nullptr, c.ext_delta != nullptr, c.want_params};
    if (!choose_sweep(p, plan.choice, call, plan.choice.bwd) || !choose_dw_stage(plan, c, call)) return GOPS_ERR_UNSUPPORTED;
    BwdPatch q;
    fill_patch(plan, c, call, q);
    hipError_t e;
    if ((e = launch_sweep(desc, plan, c, q, s)) != hipSuccess) return (int)e;
    dbg_print_backward(p);
    // max|grad_v| belongs to THIS backward call: the sweep (fp32) / the upload kernel (half) only ever raise gscale[0], so a
    // second backward after the same forward with a much smaller grad_v would inherit the larger scale and push its scaled
    // deltas into half subnormals (advisor finding, round 3).  Invariant: gscale[0] is ZERO when a backward call starts - the
    // forward's prologue zeroes it, and every backward call leaves it zero behind its last reader: fp32 calls that end with the
    // split-K reduce reset it there (ReduceJobs.reset: no extra launch - round 5; it was a 1-block fill in front of every sweep),
    // the others (half precision: the reduce itself reads it; open loop / no parameter gradients: no reduce) with a fill at their end.
    if (p.open_loop || !c.want_params) return (int)launch_fill_zero(p.gscale, 4, s);
    ProfScope scope(desc.env.kind == GOPS_ENV_NONE ? 5 : 2, s);
    ReduceJobs jobs;
    memset(&jobs, 0, sizeof(jobs));
    if (p.f16) jobs.unscale = p.gscale;   // the sweep ran on gradients scaled by f16_grad_scale(max|grad_v|)
    else jobs.poison = reinterpret_cast<const unsigned*>(p.gscale) + 3;   // (set by a plane-split forward / sweep whose conversions overflowed)
    const int L = p.pol.nl - 1;
    for (int j = 0; j <= L; ++j) {
        const DwLayer& d = plan.dw[j];
        if (d.kernel == DwKernel::None) continue;
        if ((e = launch_dw_layer(d, j < L ? p.st.d[j + 1] : p.st.dy, j == 0 ? p.st.x : p.st.h[j], plan.dw_part[j], plan.dw_part_b[j], p.gscale,
                                 d.N, c.grad->weight[j], c.grad->bias[j], jobs, s)) != hipSuccess) return (int)e;
    }
    // (two-phase backward: phase B's GEMM still reads the scale phase A's sweep left - the reset belongs to the LAST reduce of the call pair)
    const bool only_a = Phase(p.vflags).only_a;
    if (!p.f16 && !only_a && jobs.n > 0) jobs.reset = p.gscale;
    if (c.tail != nullptr) attach_update_tail(jobs, *c.tail, p);
    if ((e = launch_reduce(jobs, s)) != hipSuccess) return (int)e;
    if ((p.f16 || jobs.n == 0) && !only_a && (e = launch_fill_zero(p.gscale, 4, s)) != hipSuccess) return (int)e;
    return GOPS_OK;
}

GopsRolloutDesc value_desc(const GopsMlp& value, int batch) {
    GopsRolloutDesc d;
    memset(&d, 0, sizeof(d));
    d.batch = batch;
    d.horizon = 1;
    d.need_grad = 1;
    d.gamma = 1.0;
    d.env.kind = GOPS_ENV_NONE;
    d.env.obs_dim = value.sizes[0];
    d.env.act_dim = 1;
    d.policy = value;
    d.dtype = value.dtype;
    d.variant_flags = value.variant_flags;   // (ABI v10: plain MLP batches carry their variant flags in GopsMlp)
    return d;
}

// ---- gops_mlp_*: hidden stack on the GOPS_ENV_NONE tiles + an output layer of any width ------------------------
struct MlpPlan {
    GopsRolloutDesc d;        // hidden stack with a 1-wide stand-in head (zero weights in the workspace)
    size_t inner = 0;         // bytes of the rollout workspace at the front
    float* zeros = nullptr;   // [K + 1] stand-in head weight + bias
    float* v = nullptr;       // [B] stand-in output
    float* gv = nullptr;      // [B] zeros: grad of the stand-in output
    float* gh = nullptr;      // [S][K] adjoint of the last hidden activation
    float* gyp = nullptr;     // [S][Wp] zero-padded copy of grad_y (delta operand of the output layer's dW GEMM)
    float* part = nullptr;    // split-K slabs of the output layer [splits][Wp][K]
    float* part_b = nullptr;  // [splits][Wp]
    DwLayer out;              // the output layer's weight-gradient GEMM (dw_plan.h)
    int K = 0, W = 0, Wp = 0;
    long long S = 0;
    size_t bytes = 0;
};

int plan_mlp(const GopsMlp& mlp, int batch, void* ws, MlpPlan& m) {
    if (mlp.n_layers < 2 || mlp.n_layers > GOPS_MAX_LAYERS || batch < 1) return GOPS_ERR_BAD_ARG;
    if (mlp.dtype != GOPS_DTYPE_F32) return GOPS_ERR_UNSUPPORTED;
    m.W = mlp.sizes[mlp.n_layers];
    m.K = mlp.sizes[mlp.n_layers - 1];
    if (m.W < 1 || m.W > 4096 || (m.K & 15)) return GOPS_ERR_UNSUPPORTED;
    m.Wp = pad16(m.W);
    m.S = (long long)((batch + TB - 1) / TB) * TB;
    GopsMlp hidden = mlp;
    hidden.sizes[mlp.n_layers] = 1;
    m.d = value_desc(hidden, batch);
    Plan inner;
    // the stand-in head pointers only have to be non-null for the size query
    m.d.policy.weight[mlp.n_layers - 1] = reinterpret_cast<const float*>(&m);
    m.d.policy.bias[mlp.n_layers - 1] = reinterpret_cast<const float*>(&m);
    int rc = build_plan(m.d, nullptr, inner);
    if (rc != GOPS_OK) return rc;
    m.inner = (inner.bytes + kAlign - 1) / kAlign * kAlign;
    Carver c(ws ? static_cast<char*>(ws) + m.inner : nullptr);
    m.zeros = c.take((size_t)m.K + 16);
    m.v = c.take((size_t)batch);
    m.gv = c.take((size_t)batch);
    m.gh = c.take((size_t)m.S * m.K);
    m.gyp = c.take((size_t)m.S * m.Wp);
    m.out = plan_dw(m.Wp, m.K, m.K, m.S, false, 0);   // (dw_workgroups: the default)
    m.part = c.take(m.out.slab_w);
    m.part_b = c.take(m.out.slab_b);
    m.bytes = m.inner + c.off + kAlign;
    m.d.policy.weight[mlp.n_layers - 1] = m.zeros;
    m.d.policy.bias[mlp.n_layers - 1] = m.zeros ? m.zeros + m.K : nullptr;
    return GOPS_OK;
}

}  // namespace

extern "C" {

size_t gops_mlp_workspace_bytes(const GopsMlp* mlp, int32_t batch) {
    if (!mlp) return 0;
    MlpPlan m;
    return plan_mlp(*mlp, batch, nullptr, m) == GOPS_OK ? m.bytes : 0;
}

int gops_mlp_forward(const GopsMlp* mlp, int32_t batch, const float* x, float* y, void* workspace, size_t workspace_bytes,
                     void* stream) {
    if (!mlp || !x || !y) return GOPS_ERR_BAD_ARG;
    MlpPlan m;
    int rc = plan_mlp(*mlp, batch, workspace, m);
    if (rc != GOPS_OK) return rc;
    if (workspace == nullptr || workspace_bytes < m.bytes) return GOPS_ERR_WORKSPACE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = launch_fill_zero(m.zeros, (size_t)m.K + 16, s);
    if (e != hipSuccess) return (int)e;
    GopsRolloutIn in;
    memset(&in, 0, sizeof(in));
    in.obs = x;
    GopsRolloutOut out;
    memset(&out, 0, sizeof(out));
    out.v_pi = m.v;
    if ((rc = run_forward(m.d, in, out, workspace, m.inner, s)) != GOPS_OK) return rc;   // stashes the hidden activations
    Plan inner;
    build_plan(m.d, workspace, inner);
    const int L = mlp->n_layers - 1;
    return (int)launch_linear_out_fwd(inner.p.st.h[L], m.K, mlp->weight[L], mlp->bias[L], m.W, batch, y, s);
}

static int mlp_backward_impl(const GopsMlp* mlp, int32_t batch, const float* x, const float* grad_y, const GopsMlpGrad* grad,
                             float* grad_x, void* workspace, size_t workspace_bytes, void* stream) {
    if (!mlp || !x || !grad_y || (!grad && !grad_x)) return GOPS_ERR_BAD_ARG;
    MlpPlan m;
    int rc = plan_mlp(*mlp, batch, workspace, m);
    if (rc != GOPS_OK) return rc;
    if (workspace == nullptr || workspace_bytes < m.bytes) return GOPS_ERR_WORKSPACE;
    const int L = mlp->n_layers - 1;
    if (grad && (!grad->weight[L] || !grad->bias[L])) return GOPS_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e;
    if ((e = launch_fill_zero(m.gv, (size_t)batch, s)) != hipSuccess) return (int)e;
    // output layer: g_h = g_y Wo (+ padded copy of g_y), dWo = g_y^T h and db = column sums through the regular dW GEMM
    if ((e = launch_linear_out_bwd(grad_y, m.W, m.Wp, mlp->weight[L], m.K, batch, m.S, m.gh, m.gyp, s)) != hipSuccess) return (int)e;
    Plan inner;
    build_plan(m.d, workspace, inner);
    if (grad) {
        choose_dw_gemm(m.out, false, false, mlp->variant_flags);   // (no delta scale: g_y is the caller's)
        ReduceJobs jobs;
        memset(&jobs, 0, sizeof(jobs));
        if ((e = launch_dw_layer(m.out, m.gyp, inner.p.st.h[L], m.part, m.part_b, nullptr, m.W, grad->weight[L], grad->bias[L], jobs, s)) != hipSuccess)
            return (int)e;
        if ((e = launch_reduce(jobs, s)) != hipSuccess) return (int)e;
    }
    // hidden stack: the sweep starts from g_h instead of a head
    GopsRolloutIn in;
    memset(&in, 0, sizeof(in));
    in.obs = x;
    GopsRolloutAdjoint adj;
    memset(&adj, 0, sizeof(adj));
    adj.grad_obs = grad_x;
    BackwardCall call;
    call.in = &in, call.grad_v = m.gv, call.grad = grad, call.want_params = grad != nullptr;
    call.ext_delta = m.gh, call.adj = grad_x ? &adj : nullptr;
    return run_backward(m.d, call, workspace, m.inner, s);
}

int gops_mlp_backward(const GopsMlp* mlp, int32_t batch, const float* x, const float* grad_y, const GopsMlpGrad* grad,
                      void* workspace, size_t workspace_bytes, void* stream) {
    if (!grad) return GOPS_ERR_BAD_ARG;
    return mlp_backward_impl(mlp, batch, x, grad_y, grad, nullptr, workspace, workspace_bytes, stream);
}

int gops_mlp_backward_x(const GopsMlp* mlp, int32_t batch, const float* x, const float* grad_y, const GopsMlpGrad* grad,
                        float* grad_x, void* workspace, size_t workspace_bytes, void* stream) {
    if (!grad_x) return GOPS_ERR_BAD_ARG;
    return mlp_backward_impl(mlp, batch, x, grad_y, grad, grad_x, workspace, workspace_bytes, stream);
}

int gops_hip_version(void) { return GOPS_HIP_ABI_VERSION; }

size_t gops_rollout_workspace_bytes(const GopsRolloutDesc* desc) {
    if (desc == nullptr) return 0;
    Plan plan;
    if (build_plan(*desc, nullptr, plan) != GOPS_OK) return 0;
    return plan.bytes;
}

int gops_rollout_variant(const GopsRolloutDesc* desc) {
    if (desc == nullptr) return GOPS_ERR_BAD_ARG;
    Plan plan;
    const int rc = build_plan(*desc, nullptr, plan);
    if (rc != GOPS_OK) return rc;
    switch (plan.choice.fwd.family) {
        case Family::Split: return GOPS_VARIANT_SPLIT;
        case Family::StreamedSplit: return GOPS_VARIANT_STREAMED_SPLIT_FWD;
        case Family::Half64: return GOPS_VARIANT_HALF_TILE64;
        case Family::Stationary: return GOPS_VARIANT_STATIONARY_F32;
        default: return 0;
    }
}

int gops_dw_plan_query(int32_t N, int32_t K, int32_t Kp, int64_t S, int32_t f16, int32_t scaled, uint32_t vflags,
                       int32_t dw_workgroups, int32_t out[4]) {
    static_assert((int)DwKernel::None == GOPS_DW_NONE && (int)DwKernel::Spec == GOPS_DW_SPEC && (int)DwKernel::RingH2 == GOPS_DW_RING_H2 &&
                  (int)DwKernel::RingExact == GOPS_DW_RING_EXACT && (int)DwKernel::Skinny == GOPS_DW_SKINNY &&
                  (int)DwKernel::Fm4Bf3 == GOPS_DW_FM4_BF3 && (int)DwKernel::Fm4F32 == GOPS_DW_FM4_F32 &&
                  (int)DwKernel::Fm2Bf3 == GOPS_DW_FM2_BF3 && (int)DwKernel::Fm2F32 == GOPS_DW_FM2_F32 && (int)DwKernel::F16 == GOPS_DW_F16,
                  "gops_hip.h GOPS_DW_* are DwKernel's values");
    if (out == nullptr || N < 1 || K < 1 || Kp < K || (Kp & 15) || S < 1 || (vflags & ~GOPS_VF_ALL)) return GOPS_ERR_BAD_ARG;
    DwLayer L = plan_dw(N, K, Kp, S, f16 != 0, dw_workgroups);
    choose_dw_gemm(L, f16 != 0, scaled != 0, vflags);
    out[0] = (int)L.kernel, out[1] = L.splits, out[2] = L.chunks_per_split, out[3] = L.grid;
    return GOPS_OK;
}

int gops_rollout_forward(const GopsRolloutDesc* desc, const GopsRolloutIn* in, const GopsRolloutOut* out,
                         void* workspace, size_t workspace_bytes, void* stream) {
    if (!desc || !in || !out) return GOPS_ERR_BAD_ARG;
    return run_forward(*desc, *in, *out, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

int gops_rollout_backward(const GopsRolloutDesc* desc, const GopsRolloutIn* in, const float* grad_v,
                          const GopsMlpGrad* policy_grad, void* workspace, size_t workspace_bytes,
                          void* stream) {
    if (!desc || !in || !policy_grad) return GOPS_ERR_BAD_ARG;
    BackwardCall call;
    call.in = in, call.grad_v = grad_v, call.grad = policy_grad;
    return run_backward(*desc, call, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

int gops_rollout_backward_update(const GopsRolloutDesc* desc, const GopsRolloutIn* in, const float* grad_v,
                                 const GopsMlpGrad* policy_grad, const GopsUpdateTail* tail, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    if (!desc || !in || !policy_grad || !tail) return GOPS_ERR_BAD_ARG;
    BackwardCall call;
    call.in = in, call.grad_v = grad_v, call.grad = policy_grad, call.tail = tail;
    return run_backward(*desc, call, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

int gops_rollout_backward_adj(const GopsRolloutDesc* desc, const GopsRolloutIn* in, const float* grad_v,
                              const GopsMlpGrad* policy_grad, const GopsRolloutAdjoint* adj, void* workspace,
                              size_t workspace_bytes, void* stream) {
    if (!desc || !in || !adj) return GOPS_ERR_BAD_ARG;
    BackwardCall call;
    call.in = in, call.grad_v = grad_v, call.grad = policy_grad, call.want_params = policy_grad != nullptr, call.adj = adj;
    return run_backward(*desc, call, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

int gops_rollout_backward_open_loop(const GopsRolloutDesc* desc, const GopsRolloutIn* in, const float* grad_v,
                                    float* grad_head_pre, void* workspace, size_t workspace_bytes, void* stream) {
    if (!desc || !in || !grad_head_pre || !desc->open_loop) return GOPS_ERR_BAD_ARG;
    BackwardCall call;   // (want_params stays set: run_backward knows that an open loop has no parameters behind it)
    call.in = in, call.grad_v = grad_v, call.g_head_pre = grad_head_pre;
    return run_backward(*desc, call, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

int gops_rollout_backward_open_loop_adj(const GopsRolloutDesc* desc, const GopsRolloutIn* in, const float* grad_v,
                                        float* grad_head_pre, const GopsRolloutAdjoint* adj, void* workspace,
                                        size_t workspace_bytes, void* stream) {
    if (!desc || !in || !grad_head_pre || !adj || !desc->open_loop) return GOPS_ERR_BAD_ARG;
    GopsRolloutAdjoint a = *adj;
    a.first_step_only = 0;
    BackwardCall call;
    call.in = in, call.grad_v = grad_v, call.want_params = false, call.g_head_pre = grad_head_pre, call.adj = &a;
    return run_backward(*desc, call, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

size_t gops_value_workspace_bytes(const GopsMlp* value, int32_t batch) {
    if (!value) return 0;
    const GopsRolloutDesc d = value_desc(*value, batch);
    return gops_rollout_workspace_bytes(&d);
}

int gops_value_forward(const GopsMlp* value, int32_t batch, const float* obs, float* v, void* workspace,
                       size_t workspace_bytes, void* stream) {
    if (!value || !obs || !v) return GOPS_ERR_BAD_ARG;
    const GopsRolloutDesc d = value_desc(*value, batch);
    GopsRolloutIn in;
    memset(&in, 0, sizeof(in));
    in.obs = obs;
    GopsRolloutOut out;
    memset(&out, 0, sizeof(out));
    out.v_pi = v;
    return run_forward(d, in, out, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

int gops_value_backward(const GopsMlp* value, int32_t batch, const float* obs, const float* grad_v,
                        const GopsMlpGrad* grad, void* workspace, size_t workspace_bytes, void* stream) {
    if (!value || !obs || !grad_v || !grad) return GOPS_ERR_BAD_ARG;
    const GopsRolloutDesc d = value_desc(*value, batch);
    GopsRolloutIn in;
    memset(&in, 0, sizeof(in));
    in.obs = obs;
    BackwardCall call;
    call.in = &in, call.grad_v = grad_v, call.grad = grad;
    return run_backward(d, call, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

int gops_value_backward_update(const GopsMlp* value, int32_t batch, const float* obs, const float* grad_v,
                               const GopsMlpGrad* grad, const GopsUpdateTail* tail, void* workspace, size_t workspace_bytes, void* stream) {
    if (!value || !obs || !grad_v || !grad || !tail) return GOPS_ERR_BAD_ARG;
    const GopsRolloutDesc d = value_desc(*value, batch);
    GopsRolloutIn in;
    memset(&in, 0, sizeof(in));
    in.obs = obs;
    BackwardCall call;
    call.in = &in, call.grad_v = grad_v, call.grad = grad, call.tail = tail;
    return run_backward(d, call, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

void gops_profile_enable(int32_t on) {
    std::lock_guard<std::mutex> lk(g_prof.mu);
    g_prof.on = on != 0;
}

void gops_profile_reset(void) {
    std::lock_guard<std::mutex> lk(g_prof.mu);
    for (auto& v : g_prof.ev) {
        for (auto& pr : v) {
            (void)hipEventDestroy(pr.first);
            (void)hipEventDestroy(pr.second);
        }
        v.clear();
    }
}

int gops_profile_read(int32_t kernel_id, double* avg_ms, int64_t* launches) {
    if (kernel_id < 0 || kernel_id > 5 || !avg_ms || !launches) return GOPS_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(g_prof.mu);
    double tot = 0.0;
    int64_t n = 0;
    for (auto& pr : g_prof.ev[kernel_id]) {
        if (hipEventSynchronize(pr.second) != hipSuccess) continue;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) {
            tot += ms;
            ++n;
        }
    }
    *avg_ms = n ? tot / n : 0.0;
    *launches = n;
    return GOPS_OK;
}

}  // extern "C"
