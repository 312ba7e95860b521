// Which kernels a planned rollout runs (host only).  One record - RolloutChoice - is filled from the description by
// choose_forward (rollout_fwd.hip) and, per backward call, by choose_sweep (rollout_bwd.hip); the workspace carve
// (api.hip build_plan), the launchers and gops_rollout_variant all read it.  The instantiated kernels of every family are
// listed ONCE, as data: a family is eligible when the table holds the launch's (env kind, shape, tail) and the launcher
// dispatches over the same table, so a launch cannot be eligible and have no kernel.
#pragma once
#include <algorithm>
#include <type_traits>
#include <utility>

#include "common.h"

enum class Family {
    None,
    Half64,         // GOPS_DTYPE_F16 on 64-trajectory tiles (rollout_h64.hip)
    Split,          // register-stationary plane-split (s0 = KC0 chunks of 32 inputs; sweep: PT0 = (KC0 + 1) / 2)
    StreamedSplit,  // plane-split, planes streamed from L2 (forward: SS, sweep: SSB)
    Half16,         // GOPS_DTYPE_F16 on 16-row tiles
    General,        // forward: ActionRepeat (GEN); sweep: adjoint I/O / ActionRepeat (EXT)
    Stationary,     // register-stationary fp32 MFMA (s0 / s1 = SK0 / SK1)
    Plain,          // streamed fp32
    PlainN64,       // ... obs -> 64 -> 64 -> act written out
};

// One instantiated (env kind, shape): both TAIL values exist unless tail_ok is false.
struct Inst {
    int env;
    int s0 = 0, s1 = 0;
    bool tail_ok = true;
    int pt0 = 1;   // stationary fp32 sweep only
};

inline constexpr Inst kEveryEnv[] = {{GOPS_ENV_NONE}, {GOPS_ENV_LQ}, {GOPS_ENV_IDPENDULUM}, {GOPS_ENV_VEH3DOFCONTI}, {GOPS_ENV_VEH3DOF_SURR},
                                     {GOPS_ENV_CARTPOLE}, {GOPS_ENV_PENDULUM}, {GOPS_ENV_VEH2DOF}, {GOPS_ENV_MOBILEROBOT}, {GOPS_ENV_MOUNTAINCAR}};
inline constexpr auto& kPlain = kEveryEnv;           // forward and sweep, Plain and PlainN64
inline constexpr auto& kStreamedSplit = kEveryEnv;   // forward and sweep
inline constexpr Inst kHalf64[] = {{GOPS_ENV_NONE, 0, 0, false}, {GOPS_ENV_LQ}};
inline constexpr Inst kHalf16[] = {{GOPS_ENV_NONE}, {GOPS_ENV_LQ}, {GOPS_ENV_IDPENDULUM}, {GOPS_ENV_VEH3DOFCONTI}};
// forward <ENV, KC0, 8> and sweep <ENV, 8, 8, PT0>; more than 128 inputs (veh3dofconti with P > 30): layer 0's planes stream
// from L2 - instantiated without the tail value net
inline constexpr Inst kSplit[] = {{GOPS_ENV_LQ, 1},           {GOPS_ENV_IDPENDULUM, 1},      {GOPS_ENV_VEH3DOFCONTI, 2},
                                  {GOPS_ENV_VEH3DOFCONTI, 3}, {GOPS_ENV_VEH3DOFCONTI, 4},    {GOPS_ENV_VEH3DOFCONTI, 5, 0, false},
                                  {GOPS_ENV_VEH3DOFCONTI, 6, 0, false}, {GOPS_ENV_VEH3DOFCONTI, 7, 0, false}, {GOPS_ENV_VEH3DOFCONTI, 8, 0, false}};
inline constexpr Inst kGenFwd[] = {{GOPS_ENV_LQ}, {GOPS_ENV_IDPENDULUM}, {GOPS_ENV_CARTPOLE}, {GOPS_ENV_PENDULUM},
                                   {GOPS_ENV_MOUNTAINCAR}};   // obs == state models
inline constexpr Inst kExtBwd[] = {{GOPS_ENV_NONE, 0, 0, false}, {GOPS_ENV_LQ}, {GOPS_ENV_IDPENDULUM}, {GOPS_ENV_CARTPOLE}, {GOPS_ENV_PENDULUM},
                                   {GOPS_ENV_MOBILEROBOT}, {GOPS_ENV_MOUNTAINCAR}};
// veh3dofconti forward: 3 chunks of 16 inputs (P = 10) fully stationary; from 6 chunks up the first 6 stay in registers and
// the rest streams (P = 30: 6 + 2, P = 50: 6 + 7); else layer 0 streams
inline constexpr Inst kStationaryFwd[] = {{GOPS_ENV_LQ, 1, 16}, {GOPS_ENV_IDPENDULUM, 1, 16}, {GOPS_ENV_VEH3DOFCONTI, 6, 16},
                                          {GOPS_ENV_VEH3DOFCONTI, 3, 16}, {GOPS_ENV_VEH3DOFCONTI, 0, 16}};
// sweep: s0 counts stationary K-chunks (of 16) of the delta_1 -> g_x GEMM.  kp0 = 128: 12 of them (2 n-tiles per wave);
// kp0 = 16: all 16 (1 tile, wave 0); anything else streams
inline constexpr Inst kStationaryBwd[] = {{GOPS_ENV_LQ, 16, 16}, {GOPS_ENV_IDPENDULUM, 16, 16}, {GOPS_ENV_VEH3DOFCONTI, 12, 16, true, 2},
                                          {GOPS_ENV_VEH3DOFCONTI, 0, 16}};

template <size_t N>
constexpr bool has_inst(const Inst (&table)[N], int env, int s0, int s1, bool tail) {
    for (const Inst& e : table)
        if (e.env == env && e.s0 == s0 && e.s1 == s1 && (e.tail_ok || !tail)) return true;
    return false;
}

struct KernelChoice {
    Family family = Family::None;
    int env = 0, s0 = 0, s1 = 0;
    bool tail = false;
    bool multi = false;   // grid-stride walk over the tiles (Split: more tiles than CUs; StreamedSplit sweep: ssb_fuse_kind)
    int grid = 0;
    size_t lds = 0;
};

// Calls f.template operator()<E, TAIL>() for the entry E of `Table` the choice names; false: no such instantiation.
template <const auto& Table, class F, size_t... I>
bool dispatch_impl(const KernelChoice& k, F&& f, std::index_sequence<I...>) {
    auto one = [&]<size_t J>() {
        constexpr Inst e = Table[J];
        if (e.env != k.env || e.s0 != k.s0 || e.s1 != k.s1 || (k.tail && !e.tail_ok)) return false;
        if (!k.tail) f.template operator()<e, false>();
        else if constexpr (e.tail_ok) f.template operator()<e, true>();
        return true;
    };
    return (one.template operator()<I>() || ...);
}
template <const auto& Table, class F>
bool dispatch(const KernelChoice& k, F&& f) {
    return dispatch_impl<Table>(k, f, std::make_index_sequence<std::extent_v<std::remove_reference_t<decltype(Table)>>>{});
}
template <class F>
void dispatch_bool(bool b, F&& f) { b ? f(std::true_type{}) : f(std::false_type{}); }

// What a planned rollout runs.  `fwd` and everything below it follow from the description alone (choose_forward); `bwd`
// is filled per backward call (choose_sweep).
struct RolloutChoice {
    KernelChoice fwd, bwd;
    // ---- what the workspace carve depends on ----
    // These hold for EVERY sweep that can follow the forward - the family's own sweep, the General (EXT) sweep of an adjoint
    // call, the Plain sweep of gops_mlp_backward's hidden stack, either phase of a two-phase backward - because they are
    // derived with the per-call facts (adjoint I/O, ext_delta) absent, and those only ever move a call to the Plain / General
    // sweeps: both read the narrow LDS image and the idpendulum parking when the plan has them, and neither reads plane operands.
    bool split = false, ss = false, ssb = false, h64 = false;   // -> RolloutParams sp.on / ss / ssb / h64
    bool tail_fp32 = false;
    bool stationary_bwd = false;   // the default sweep is Family::Stationary
    int narrow = 0, narrow_floats = 0, narrow_off_fwd = 0, narrow_off_bwd = 0;
    bool idp_parking = false;      // StashDev.idp: written by the forward, read by the sweeps that stage nothing else
    bool fuse_dw0 = false;         // the Half64 sweep can form layer 0's weight gradient (slabs per workgroup in dw_part[0])
    int touch_mode = 0;
};

// What run_backward knows about one call beyond the plan.
struct SweepCall {
    bool ext, ext_delta, want_params;   // adjoint I/O or ActionRepeat; gops_mlp_backward's hidden-stack deltas; parameter gradients wanted
};

inline int tiles(const RolloutParams& p) { return (p.B + TB - 1) / TB; }
// reference-table points per trajectory the kernels keep in LDS
inline int ref_table_points(const RolloutParams& p) { return env_has_ref_table(p.env.kind) ? p.env.pre_horizon + 1 + p.H : 0; }
// ... of a sweep: the table, or the idpendulum sub-step parking (common.h IDP_POINTS)
inline int ref_points_in_lds(const RolloutParams& p, bool split) {
    return env_has_ref_table(p.env.kind) ? ref_table_points(p) : (p.env.kind == GOPS_ENV_IDPENDULUM ? IDP_POINTS(split) : 0);
}

int device_cus();   // rollout_fwd.hip
size_t rollout_fwd_lds_bytes(int ldx, int ldh, int ref_points, bool f16, int split_k0, bool ss = false);
size_t rollout_bwd_lds_bytes(int ldx, int ldh, int ref_points, bool f16, bool split, bool ssb = false);
size_t rollout_fwd_h64_lds_bytes(int ldx, int ldh);   // rollout_h64.hip
size_t rollout_bwd_h64_lds_bytes(int ldx, int ldh);
bool h64_shape_ok(const RolloutParams& p);
int h64_fwd_grid(const RolloutParams& p);
bool h64_can_fuse_dw0(const RolloutParams& p);
int h64_sweep_grid(const RolloutParams& p);
size_t split_bwd_lds_bytes(const RolloutParams& p);   // rollout_bwd.hip
size_t ssb_lds_bytes(const RolloutParams& p);
int ssb_grid_limit();
bool stationary_shape(const RolloutParams& p);                  // rollout_fwd.hip
bool stationary_bwd_shape(const RolloutParams& p, int& s0);

// false: the description has no kernel (GOPS_ERR_UNSUPPORTED)
bool choose_forward(const RolloutParams& p, RolloutChoice& c);
bool choose_sweep(const RolloutParams& p, const RolloutChoice& c, const SweepCall& call, KernelChoice& k);
inline bool sweep_fuses_out(const KernelChoice& k, const SweepCall& call) {   // output-layer weight gradient inside the sweep
    return call.want_params && (k.family == Family::Split || (k.family == Family::StreamedSplit && k.multi));
}
hipError_t launch_rollout_fwd(const RolloutParams& p, const KernelChoice& k, const RolloutParams* dp, hipStream_t stream);
hipError_t launch_rollout_bwd(const RolloutParams& p, const KernelChoice& k, const RolloutParams* dp, const BwdPatch& q, hipStream_t stream);
hipError_t launch_rollout_fwd_h64(const RolloutParams& p, const KernelChoice& k, const RolloutParams* dp, hipStream_t stream);
hipError_t launch_rollout_bwd_h64(const RolloutParams& p, const KernelChoice& k, const RolloutParams* dp, const BwdPatch& q, hipStream_t stream);
