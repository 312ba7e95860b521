// The weight-gradient stage of a backward call (host only): per Linear layer ONE record - DwLayer - that says which kernel
// forms the layer's split-K partial slabs, on which grid, and how the reduce launch reads them.  plan_dw fills what the
// workspace carve needs (api.hip build_plan / plan_mlp keep the record in their plan), choose_dw_* add what a call decides;
// launch_dw and add_reduce_jobs read the record and nothing else.  The functions live next to the kernels (dw_gemm.hip).
#pragma once
#include "common.h"

enum class DwKernel {
    None,        // the layer is not part of this call (other phase of a two-phase backward; gops_mlp_backward's stand-in head)
    Spec,        // dw_gemm_spec_kernel: wave-specialised two-half-plane GEMM, 256 x 128 tiles, 512 threads
    RingH2,      // dw_gemm_ring_kernel<true>: two-half-plane GEMM, 128 x 128 tiles
    RingExact,   // dw_gemm_ring_kernel<false>: exact three-plane bf16 split on the same ring
    Skinny,      // dw_skinny_kernel: 16 (padded) inputs, one workgroup per 256 features and split
    Fm4Bf3,      // dw_gemm_fm_kernel<4, true>: 128 x 128 tiles, three-plane bf16 split
    Fm4F32,      // dw_gemm_fm_kernel<4, false>: ... fp32 MFMA (GOPS_VF_DW_F32)
    Fm2Bf3,      // dw_gemm_fm_kernel<2, true>: 64 x 64 tiles
    Fm2F32,      // dw_gemm_fm_kernel<2, false>
    F16,         // dw_gemm_f16_kernel (GOPS_DTYPE_F16): 128 x 128 tiles, 64-sample chunks
    InSweep,     // no launch: the sweep wrote one slab per workgroup (layer 0 of the 64-row half sweep; the output layer of the
                 // Split / StreamedSplit-multi sweeps)
    OutFm,       // dw_out_fm_kernel: output layer (<= GOPS_MAX_ACT wide) over the feature-major fp32 stash
    OutH,        // dw_out_h_kernel: ... over the row-major half stash
};

struct DwLayer {
    // ---- what the workspace carve depends on (plan_dw / plan_dw_out) ----
    // These follow from the layer's shape, the stash rows S, the dtype and dw_workgroups alone - no per-call fact (delta scale
    // present, GOPS_VF_DW_*, phase, adjoint I/O, ext_delta) enters - and every GEMM kernel a call can choose writes exactly
    // `splits` slabs [N][Kp] / [N], so slab_w / slab_b cover every call that can follow the forward.  The slabs a sweep writes
    // itself are counted in its workgroups: layer 0 of the 64-row sweep is carved for h64_sweep_grid (a function of the batch),
    // and choose_dw_in_sweep refuses a call whose sweep has more workgroups than the region has slabs.
    int N = 0, K = 0, Kp = 0;   // outputs (rows of a slab), inputs, padded inputs
    long long S = 0;            // stash rows (samples of the contraction)
    int tile = 0;               // edge of the GEMM's square output tile (128 / 64)
    int splits = 0, chunks_per_split = 0;
    size_t slab_w = 0, slab_b = 0;   // floats carved for the weight / bias partial slabs
    // ---- per call (choose_dw_gemm / choose_dw_out / choose_dw_in_sweep) ----
    DwKernel kernel = DwKernel::None;
    int grid = 0, block = 0;
    size_t lds = 0;
    int guard = 1;              // two-half-plane kernels: re-run saturated tiles exactly (0: GOPS_VF_DW_NO_GUARD)
    int ld = 0;                 // row stride of a slab as the reduce job reads it
};

bool dw_skinny_ok(int N, int Kp);
DwLayer plan_dw(int N, int K, int Kp, long long S, bool f16, int wg_target);
DwLayer plan_dw_out(int K, int A, long long S);   // output layer of a rollout policy: carved for DW_OUT_SPLITS slabs [GOPS_MAX_ACT][K]
// scaled: the launch has max|grad_v| as the deltas' magnitude reference (two-half-plane products); else the exact kernels
void choose_dw_gemm(DwLayer& L, bool f16, bool scaled, unsigned vflags);
void choose_dw_out(DwLayer& L, bool f16);
// the sweep leaves `slabs` slabs [N][ld] / [N]; false: they do not fit the carved region
bool choose_dw_in_sweep(DwLayer& L, int slabs, int ld);
// D / X: delta and activation stash (dy / h of the output layer); dscale: device pointer to max|grad_v| or null
hipError_t launch_dw(const DwLayer& L, const void* D, const void* X, float* part, float* part_b, const float* dscale, hipStream_t s);
// job: `splits` slabs [slab_rows (0: rows)][ld] summed into out[rows][cols]
void reduce_jobs_add(ReduceJobs& jobs, const float* part, int splits, int rows, int cols, int ld, float* out, int slab_rows = 0);
// the layer's weight and bias job; rows < L.N: gops_mlp_backward's padded output layer
void add_reduce_jobs(ReduceJobs& jobs, const DwLayer& L, const float* part, const float* part_b, int rows, float* gw, float* gb);
