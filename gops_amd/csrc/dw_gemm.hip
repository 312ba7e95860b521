// The weight-gradient stage of a backward call: the GEMMs dW = delta^T * input over all B*H samples that write split-K partial
// slabs, the stage's record (dw_plan.h), and the reduce launch that sums the slabs - with the fused Adam / Polyak step and loss mean.
#include <algorithm>
#include "common.h"
#include "block_reduce.h"
#include "launchers.h"

// Streams that are read ONCE (stash operands of the weight-gradient GEMMs, split-K partials) are loaded with the non-temporal
// policy: MI355X_MICROARCH.md measures LDS-DMA fills 18 % earlier with `nt` and 6.5 - 6.8 instead of 6.4 TB/s chip-wide; here the
// wave-specialised GEMM went from 4.2 to 4.9 TB/s (target: weight-gradient group 140 -> 126 us) - the data does not displace
// the other kernels' working set in L2 / MALL either.
#define DW_STREAM_LOAD(ptr) __builtin_nontemporal_load(ptr)   // (LDS-DMA fills of these streams: async_copy16_to_lds<true>)

// ---------------------------------------------------------------------------------------------
// dW GEMM:  part[split][n][k] = sum_{s in split} D[s][n] * X[s][k]      (n < N, k < Kp)
//
// Both operands are feature-major stash tensors (common.h StashDev: element (tile q, feature f, row m) at
// (q * F + f) * 16 + m), and the contraction index IS the sample: an MFMA operand fragment - consecutive
// samples of one feature - is therefore contiguous in memory and is loaded straight from global into the
// registers of the lane that feeds it to the matrix core.  No LDS, no transposes, no barriers.
//
// Workgroup tile 32R x 32R outputs, 2 x 2 waves of 16R x 16R (R x R MFMA tiles).  A K-block is 32 samples = two
// sample tiles q0, q0 + 1; lane (f = lane & 15, g = lane >> 4) of a fragment holds samples 4g .. 4g+3 of both
// tiles: two dwordx4 loads, each of which covers a fully contiguous KiB per wave (16 features x 64 B).  (The order
// of the 32 samples inside the contraction is free as long as both operands use the same one.)  The next
// block's fragments are in flight while the current ones are multiplied.
//
// BF3: "bf16x3" products on v_mfma_f32_16x16x32_bf16 with fp32 results - every fp32 operand a is split EXACTLY
// into three bf16 planes a = a1 + a2 + a3 (a1 = bf16(a), a2 = bf16(a - a1), a3 = bf16(a - a1 - a2): 3 x 8
// significant bits cover the 24 of fp32) and a*b is accumulated in fp32 from the six plane products a1b1, a1b2,
// a2b1, a1b3, a2b2, a3b1; the three dropped ones are below 2^-25 |ab|, i.e. under fp32 rounding.  Six of these
// MFMAs cost 96 cycles against 256 for the eight v_mfma_f32_16x16x4_f32 of the same 32-deep block.
// !BF3: the fp32 matrix-core instruction itself (A/B knob GOPS_DW_F32, and the reference for the split).
//
// Workgroups whose k-tile is 0 also accumulate the bias gradient (column sums of D).
// ---------------------------------------------------------------------------------------------
// (split3: common.h)

// 8 fp32 samples of one feature -> the three bf16x8 plane fragments
__device__ __forceinline__ void split_frag(const f32x4& lo, const f32x4& hi, bf16x8 (&pl)[3]) {
    unsigned p0[3], p1[3], p2[3], p3[3];
    split3(lo[0], lo[1], p0);
    split3(lo[2], lo[3], p1);
    split3(hi[0], hi[1], p2);
    split3(hi[2], hi[3], p3);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const u32x4 v = {p0[q], p1[q], p2[q], p3[q]};
        pl[q] = __builtin_bit_cast(bf16x8, v);
    }
}

template <int R, bool BF3>
__global__ __launch_bounds__(NTHREADS, 2) void dw_gemm_fm_kernel(const float* __restrict__ D, int N,
                                                                  const float* __restrict__ X, int Kp,
                                                                  long long Q, int splits, int chunks_per_split,
                                                                  float* __restrict__ part,
                                                                  float* __restrict__ part_b) {
    constexpr int T = 32 * R;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tiles_k = (Kp + T - 1) / T, tiles = tiles_k * ((N + T - 1) / T);
    // XCD-aware order: workgroup b runs on XCD b % 8.  All output tiles of one sample split read the
    // same D / X blocks, so they get the same XCD and adjacent slots: the second reader of a block
    // hits that XCD's L2 instead of HBM.
    const int xcd = blockIdx.x & 7, local = blockIdx.x >> 3;
    const int tile = local % tiles, split = (local / tiles) * 8 + xcd;
    if (split >= splits) return;
    const int tile_n = tile / tiles_k, tile_k = tile - tile_n * tiles_k;
    const int wn = wave >> 1, wk = wave & 1;
    const int nb = tile_n * T + wn * 16 * R, kb = tile_k * T + wk * 16 * R;   // first feature of this wave's rows / columns
    const int f = lane & 15, g = lane >> 4;
    const bool want_bias = part_b != nullptr && tile_k == 0 && wk == 0;

    // Per-fragment element offsets inside a sample tile.  Features past the matrix edge are CLAMPED to the last one
    // (their products land in accumulator rows / columns that are never stored) and the block index of a prefetch is
    // clamped to the split's last block, so that every load is unconditional: the loop body is one basic block that
    // the scheduler can interleave freely (loads, bf16 splits and MFMAs of different fragments).
    int doff[R], xoff[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
        doff[i] = min(nb + 16 * i + f, N - 1) * 16 + 4 * g;
        xoff[i] = min(kb + 16 * i + f, Kp - 1) * 16 + 4 * g;
    }
    const GLOBAL_AS float* Dg = gptr(D);
    const GLOBAL_AS float* Xg = gptr(X);
    const size_t dtile = (size_t)N * 16, xtile = (size_t)Kp * 16;
    // Split s owns the 32-sample blocks s, s + splits, s + 2 splits, ...: at any moment the resident workgroups read
    // one contiguous window of the stash (like a streaming kernel).  Contiguous per-split ranges would walk `splits`
    // streams in lockstep at a fixed large stride, which lands them on the same few HBM channels.
    const long long nblk_all = (Q + 1) >> 1;
    const int nblk = (int)((nblk_all - split + splits - 1) / splits);         // >= 1: splits <= nblk_all
    const bool odd_tail = (Q & 1) && ((nblk_all - 1) % splits == split);      // the very last block has one sample tile only
    auto blk_of = [&](int c) { return (long long)split + (long long)min(c, nblk - 1) * splits; };

    f32x4 acc[R][R] = {};
    float bsum[R];
#pragma unroll
    for (int i = 0; i < R; ++i) bsum[i] = 0.f;
    // Raw fragments: ONE register set.  A fragment's registers are refilled with the same fragment of the NEXT block
    // right after this block's copy has been split / consumed, so every load has a whole block of work to land
    // and no second buffer adds to the register pressure (spilling here would put scratch traffic - and its
    // in-order vmcnt waits - in front of the prefetches).
    f32x4 dra[R][2], xra[R][2];
    auto load_d = [&](long long blk, int i) {
#pragma unroll
        for (int h = 0; h < 2; ++h) dra[i][h] = ld4(Dg + (size_t)min(2 * blk + h, Q - 1) * dtile + doff[i]);
    };
    auto load_x = [&](long long blk, int j) {
#pragma unroll
        for (int h = 0; h < 2; ++h) xra[j][h] = ld4(Xg + (size_t)min(2 * blk + h, Q - 1) * xtile + xoff[j]);
    };
    // one 32-sample block; LAST_HALF_EMPTY: the second sample tile does not exist (odd tile count): its (clamped,
    // i.e. duplicate) fragments are replaced by zeros
    auto block = [&]<bool LAST_HALF_EMPTY>(long long next_blk) {
        const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
        if constexpr (BF3) {
            bf16x8 b[R][3];
#pragma unroll
            for (int j = 0; j < R; ++j) {
                split_frag(xra[j][0], LAST_HALF_EMPTY ? zero4 : xra[j][1], b[j]);
                load_x(next_blk, j);
            }
#pragma unroll
            for (int i = 0; i < R; ++i) {
                const f32x4 d0 = dra[i][0], d1 = LAST_HALF_EMPTY ? zero4 : dra[i][1];
                bf16x8 a[3];
                split_frag(d0, d1, a);
                bsum[i] += ((d0[0] + d0[1]) + (d0[2] + d0[3])) + ((d1[0] + d1[1]) + (d1[2] + d1[3]));   // (every wave: no branch in the block)
                load_d(next_blk, i);
                // six plane products, smallest terms first; consecutive MFMAs go to different accumulators
                constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
                for (int q = 0; q < 6; ++q)
#pragma unroll
                    for (int j = 0; j < R; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[PA[q]], b[j][PB[q]], acc[i][j], 0, 0, 0);
            }
        } else {
            f32x4 xc[R][2];
#pragma unroll
            for (int j = 0; j < R; ++j) {
                xc[j][0] = xra[j][0]; xc[j][1] = LAST_HALF_EMPTY ? zero4 : xra[j][1];
                load_x(next_blk, j);
            }
#pragma unroll
            for (int i = 0; i < R; ++i) {
                const f32x4 d0 = dra[i][0], d1 = LAST_HALF_EMPTY ? zero4 : dra[i][1];
                bsum[i] += ((d0[0] + d0[1]) + (d0[2] + d0[3])) + ((d1[0] + d1[1]) + (d1[2] + d1[3]));   // (every wave: no branch in the block)
                load_d(next_blk, i);
#pragma unroll
                for (int u = 0; u < 8; ++u)
#pragma unroll
                    for (int j = 0; j < R; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(u < 4 ? d0[u & 3] : d1[u & 3], xc[j][u >> 2][u & 3], acc[i][j], 0, 0, 0);
            }
        }
    };

#pragma unroll
    for (int j = 0; j < R; ++j) load_x(blk_of(0), j);
#pragma unroll
    for (int i = 0; i < R; ++i) load_d(blk_of(0), i);
    const int nfull = odd_tail ? nblk - 1 : nblk;
    for (int c = 0; c < nfull; ++c) block.template operator()<false>(blk_of(c + 1));
    if (odd_tail) block.template operator()<true>(blk_of(nblk));
    float* pbase = part + (size_t)split * N * Kp;
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const int k = kb + 16 * j + f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = nb + 16 * i + 4 * g + r;
                if (n < N && k < Kp) pbase[(size_t)n * Kp + k] = acc[i][j][r];
            }
        }
    if (want_bias) {   // column sums of D: the four sample groups of a feature sit in lanes f, f+16, f+32, f+48
#pragma unroll
        for (int i = 0; i < R; ++i) {
            float t = bsum[i];
            t += __shfl_xor(t, 16);
            t += __shfl_xor(t, 32);
            if (g == 0 && nb + 16 * i + f < N) part_b[(size_t)split * N + nb + 16 * i + f] = t;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// The same GEMM for the large layers (N % 128 == 0, Kp % 128 == 0): the operand tiles of a
// 32-sample block (128 features x 2 sample tiles of each operand = 4 x 8 KiB of CONTIGUOUS stash memory) travel
// HBM -> LDS with global_load_lds_dwordx4 - no register holds them - into a ring of DWR_STAGES stages, DWR_STAGES - 1
// blocks ahead of the block being multiplied; wave w copies region w of a stage (eight 1-KiB copies).  Two stages and
// two workgroups per CU measured best (layer-2 GEMM of the target: 103 us; four stages with one workgroup per CU 141 us:
// with a single wave per SIMD nothing overlaps the bf16 split on the VALU with the MFMAs).
// Every element is fetched from L2 / HBM ONCE per workgroup (the register-direct kernel above fetches it once per
// wave that needs it).  A lane's fragment (feature f = lane & 15, samples 4 g .. 4 g + 3 of both sample tiles) is two
// conflict-free ds_read_b128 of the LDS image; it is split into the three bf16 planes in registers and multiplied.
// One barrier per block: it publishes block c (each wave first waits for its own copies of that block) and frees the
// stage that block c - 1 was read from for the copies of block c + DWR_STAGES - 1.
// ---------------------------------------------------------------------------------------------
// Two-half-plane form of an fp32 operand fragment for the H2 variant of the ring GEMM: with v = x * s,
//     hi = f16(v)  (round toward zero: a finite v never becomes inf),   lo = f16((v - hi) * 2^11)  (likewise),
// so v = hi + lo * 2^-11 to 2^-21 |v| (22 significant bits), and the product of two such operands is
//     d * a = dh * ah + (dh * al + dl * ah) * 2^-11 + O(2^-21 |d a|)
// - three v_mfma_f32_16x16x32_f16 per 32-sample block instead of the six bf16 MFMAs of the exact three-plane split, and 3-4
// VALU instructions per element instead of 5.5.  Mode 2 (adopted) keeps lo UNSCALED (lo = f16(v - hi), one accumulator):
// lo is a normal half for |v| >= 0.06 and a subnormal one below (absolute error <= 6e-8 in scaled units), so the scales
// put typical magnitudes near 1..30: activations as they are, deltas times the power of two that brings max|grad_v| into
// [16, 32).  Range: |x * s| >= 65504 saturates (round toward zero never produces inf); the converting threads watch for it
// and a workgroup whose operands saturated repeats ITS blocks with the exact three-plane split before it stores anything -
// a diverged rollout costs time, never a wrong gradient.
#define DW_H2_SA 1.0f      // (unscaled lo planes: keep typical magnitudes near 1 so that lo stays a normal half)
#define DW_H2_LO 1.0f
__device__ __forceinline__ void split2h(const f32x4& lo4, const f32x4& hi4, float s, f16x8& ph, f16x8& pl) {
    const float s2 = s * DW_H2_LO;
    u32x4 uh, ul;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float x0 = e < 2 ? lo4[2 * e] : hi4[2 * e - 4], x1 = e < 2 ? lo4[2 * e + 1] : hi4[2 * e - 3];
        const f16x2 h = __builtin_bit_cast(f16x2, __builtin_amdgcn_cvt_pkrtz(x0 * s, x1 * s));
        const float r0 = fmaf((float)h[0], -DW_H2_LO, x0 * s2), r1 = fmaf((float)h[1], -DW_H2_LO, x1 * s2);   // (v - hi) * 2^11, exact
        uh[e] = __builtin_bit_cast(unsigned, h);
        ul[e] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(r0, r1));
    }
    ph = __builtin_bit_cast(f16x8, uh);
    pl = __builtin_bit_cast(f16x8, ul);
}

// The same split for the wave-specialised kernel's converting waves, spelled in the instructions it should cost: v_fma_mixlo / mixhi_f16
// form f16(s x) and f16(s x - hi) in ONE instruction each (fp32 product-sum, one rounding to half, written to one half of the
// destination) - 4 VALU per element pair instead of the 6 hipcc emits for the expression above (v_mul x 2, v_cvt_pkrtz, v_fma_mix x 2,
// v_cvt_pkrtz).  Rounding is to nearest here (toward zero there): lo then needs one bit less, the pair carries the same 22 bits;
// |s x| >= 65520 becomes inf instead of saturating - the callers' range watch (vmax < 65504) is on the fp32 values and unchanged.
__device__ __forceinline__ void split2h_mix(const f32x4& lo4, const f32x4& hi4, float s, f16x8& ph, f16x8& pl) {
    u32x4 uh, ul;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float x0 = e < 2 ? lo4[2 * e] : hi4[2 * e - 4], x1 = e < 2 ? lo4[2 * e + 1] : hi4[2 * e - 3];
        unsigned h, l;
        asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(h) : "v"(s), "v"(x0));
        asm("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(h) : "v"(s), "v"(x1));
        asm("v_fma_mixlo_f16 %0, %1, %2, -%3 op_sel_hi:[0,0,1]" : "=v"(l) : "v"(s), "v"(x0), "v"(h));
        asm("v_fma_mixhi_f16 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(l) : "v"(s), "v"(x1), "v"(h));
        uh[e] = h;
        ul[e] = l;
    }
    ph = __builtin_bit_cast(f16x8, uh);
    pl = __builtin_bit_cast(f16x8, ul);
}
// running maximum of |a|, |b| in one instruction (hipcc spells fmaxf(m, fmaxf(fabsf(a), fabsf(b))) as two canonicalising v_max + v_max3)
__device__ __forceinline__ void absmax2(float& m, float a, float b) { asm("v_max3_f32 %0, |%1|, |%2|, %0" : "+v"(m) : "v"(a), "v"(b)); }

// What the hidden deltas of a backward call are measured against when they are scaled for the half planes (dscale =
// RolloutParams::gscale): the largest |delta_y| of the sweep (slot 1: the plane-split sweeps track it, rollout_bwd.hip) where there
// is one, else max|grad_v| (slot 0).  Whatever the choice, a block that still saturates is redone exactly.
__device__ __forceinline__ float dw_delta_yardstick(const float* dscale) {
    const float dy = gptr(dscale)[1], gv = gptr(dscale)[0];
    return dy > 0.f ? dy : gv;
}

#define DWR_STAGES 2
#define DWR_STAGE_FLOATS (4 * 2048)   // [D tile q0][D tile q0+1][X tile q0][X tile q0+1], each [128 features][16 rows]

// H2: the two-half-plane products (split2h) instead of the exact three-plane bf16 split; dscale -> max|grad_v| of the launch
// (RolloutParams::gscale): the deltas are multiplied by f16_grad_scale(max|grad_v|) / 64 before they are halved.  The
// staged fp32 tiles of a block are converted IN PLACE, once per workgroup: work item (operand, feature f, sample group g)
// reads the two 16-byte vectors that are lane (f, g)'s fragment (rows 4g..4g+3 of both sample tiles), forms the hi / lo
// half planes of those 8 samples and writes hi where the first tile's vector was, lo where the second's was - 1024 items
// per block, 4 per thread, the same items every block (so the bias column sums accumulate in the converting thread).  The
// MFMA phase then reads ready-made operands (two ds_read_b128 per fragment) and issues no VALU work at all.
template <bool H2>
__global__ __launch_bounds__(NTHREADS, 2) void dw_gemm_ring_kernel(const float* __restrict__ D, int N,
                                                                    const float* __restrict__ X, int Kp,
                                                                    long long Q, int splits, int chunks_per_split,
                                                                    float* __restrict__ part,
                                                                    float* __restrict__ part_b, const float* __restrict__ dscale, int redo_guard) {
    extern __shared__ __attribute__((aligned(16))) float ring[];   // [DWR_STAGES][DWR_STAGE_FLOATS]
    constexpr int T = 128, R = 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tiles_k = (Kp + T - 1) / T, tiles = tiles_k * (N / T);   // (the last K-tile may be partial: Kp is a multiple of 16)
    const int xcd = blockIdx.x & 7, local = blockIdx.x >> 3;   // XCD-aware order, as above
    const int tile = local % tiles, split = (local / tiles) * 8 + xcd;
    if (split >= splits) return;
    const int tile_n = tile / tiles_k, tile_k = tile - tile_n * tiles_k;
    const int wn = wave >> 1, wk = wave & 1;
    const int f = lane & 15, g = lane >> 4;
    const bool want_bias = part_b != nullptr && tile_k == 0 && wk == 0;
    const long long nblk_all = (Q + 1) >> 1;                                  // block c of this split is block split + c * splits
    const int nblk = (int)((nblk_all - split + splits - 1) / splits);
    const bool odd_tail = (Q & 1) && ((nblk_all - 1) % splits == split);

    // this wave's copy job: region `wave` of a stage = sample tile (wave & 1) of operand (wave >> 1)
    const float* csrc = (wave < 2) ? D + (size_t)tile_n * T * 16 : X + (size_t)tile_k * T * 16;
    const size_t ctile = (size_t)((wave < 2) ? N : Kp) * 16;
    // features of a partial last K-tile that do not exist (>= Kp) are fetched from the tile's first features instead: finite
    // values whose products land in columns that are never stored
    const int kvalid = (wave < 2) ? T : min(T, Kp - tile_k * T);   // valid features of this wave's operand tile
    auto copy_block = [&](int c, int stage) {   // block index clamped: the copy count per block is constant
        const long long bq = min(((long long)split + (long long)min(c, nblk - 1) * splits) * 2 + (wave & 1), Q - 1);
        const float* src = csrc + (size_t)bq * ctile + 4 * lane;
        const float* dst = ring + stage * DWR_STAGE_FLOATS + wave * 2048;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int feat = u * 16 + (lane >> 2);
            async_copy16_to_lds<true>(feat < kvalid ? src + u * 256 : src + u * 256 - (size_t)(feat - (feat % kvalid)) * 16, dst + u * 256);
        }
    };

    f32x4 acc[R][R] = {};
    float bsum[R] = {0.f, 0.f, 0.f, 0.f};
    float sd = 1.f;
    if constexpr (H2) sd = f16_grad_scale(dw_delta_yardstick(dscale)) * 16.f;
    auto block = [&]<bool LAST_HALF_EMPTY, bool M2>(int stage) {
        const float* st = ring + stage * DWR_STAGE_FLOATS;
        const float* da = st + (wn * 64 + f) * 16 + 4 * g;          // D fragments of row-tile i: + 256 i  (+ 2048: second tile)
        const float* xa = st + 4096 + (wk * 64 + f) * 16 + 4 * g;   // X fragments of column-tile j
        const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
        if constexpr (M2) {   // operands were converted in place by convert_stage(): hi plane in the first tile's slot, lo in the second's
            f16x8 bh[R], bl[R];
#pragma unroll
            for (int j = 0; j < R; ++j) {
                bh[j] = *reinterpret_cast<const f16x8*>(xa + 256 * j);
                bl[j] = *reinterpret_cast<const f16x8*>(xa + 256 * j + 2048);
            }
#pragma unroll
            for (int i = 0; i < R; ++i) {
                const f16x8 ah = *reinterpret_cast<const f16x8*>(da + 256 * i), al = *reinterpret_cast<const f16x8*>(da + 256 * i + 2048);
#pragma unroll
                for (int j = 0; j < R; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh[j], acc[i][j], 0, 0, 0);
#pragma unroll
                for (int j = 0; j < R; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl[j], acc[i][j], 0, 0, 0);
#pragma unroll
                for (int j = 0; j < R; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh[j], acc[i][j], 0, 0, 0);
            }
            return;
        }
        bf16x8 b[R][3];
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const f32x4 x0 = *reinterpret_cast<const f32x4*>(xa + 256 * j);
            const f32x4 x1 = LAST_HALF_EMPTY ? zero4 : *reinterpret_cast<const f32x4*>(xa + 256 * j + 2048);
            split_frag(x0, x1, b[j]);
        }
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const f32x4 d0 = *reinterpret_cast<const f32x4*>(da + 256 * i);
            const f32x4 d1 = LAST_HALF_EMPTY ? zero4 : *reinterpret_cast<const f32x4*>(da + 256 * i + 2048);
            bf16x8 a[3];
            split_frag(d0, d1, a);
            bsum[i] += ((d0[0] + d0[1]) + (d0[2] + d0[3])) + ((d1[0] + d1[1]) + (d1[2] + d1[3]));
            constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};   // smallest terms first
#pragma unroll
            for (int q = 0; q < 6; ++q)
#pragma unroll
                for (int j = 0; j < R; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[PA[q]], b[j][PB[q]], acc[i][j], 0, 0, 0);
        }
    };

    // H2: in-place conversion of a landed stage; item id = tid + 256 k: operand id >> 9, feature (id >> 2) & 127, group id & 3
    float vmax = 0.f;             // largest scaled magnitude this thread converted (saturation watch)
    float csum[2] = {0.f, 0.f};   // column sums of D over the two D items of this thread (features tid >> 2 and 64 + (tid >> 2), group tid & 3)
    auto convert_stage = [&]<bool LAST_HALF_EMPTY>(int stage) {
        float* st = ring + stage * DWR_STAGE_FLOATS;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int id = tid + NTHREADS * k, op = id >> 9, fe = (id >> 2) & 127, gg = id & 3;
            float* at = st + op * 4096 + fe * 16 + 4 * gg;
            const f32x4 v0 = *reinterpret_cast<const f32x4*>(at);
            const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
            const f32x4 v1 = LAST_HALF_EMPTY ? zero4 : *reinterpret_cast<const f32x4*>(at + 2048);
            if (k < 2) csum[k] += ((v0[0] + v0[1]) + (v0[2] + v0[3])) + ((v1[0] + v1[1]) + (v1[2] + v1[3]));
            const float sc = k < 2 ? sd : DW_H2_SA;
            const float m0 = fmaxf(fmaxf(fabsf(v0[0]), fabsf(v0[1])), fmaxf(fabsf(v0[2]), fabsf(v0[3])));
            const float m1 = fmaxf(fmaxf(fabsf(v1[0]), fabsf(v1[1])), fmaxf(fabsf(v1[2]), fabsf(v1[3])));
            vmax = fmaxf(vmax, fmaxf(m0, m1) * sc);   // (NaN-free inputs: a NaN in the stash is NaN in the result either way)
            f16x8 ph, pl;
            split2h(v0, v1, sc, ph, pl);
            *reinterpret_cast<f16x8*>(at) = ph;
            *reinterpret_cast<f16x8*>(at + 2048) = pl;
        }
    };
    const int nfull = odd_tail ? nblk - 1 : nblk;
    // one pass over this workgroup's blocks: M2 = two-half-plane products (with the in-place conversion), else the exact split
    auto run = [&]<bool M2>() {
#pragma unroll
        for (int d = 0; d < DWR_STAGES - 1; ++d) copy_block(d, d);
        for (int c = 0; c < nblk; ++c) {
            // this wave's copies of block c have landed once at most the 8 x (DWR_STAGES - 2) younger ones are outstanding
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(8 * (DWR_STAGES - 2)) : "memory");
            __syncthreads();
            copy_block(c + DWR_STAGES - 1, (c + DWR_STAGES - 1) % DWR_STAGES);
            if constexpr (M2) {
                if (c < nfull) convert_stage.template operator()<false>(c % DWR_STAGES);
                else convert_stage.template operator()<true>(c % DWR_STAGES);
                __syncthreads();
            }
            if (c < nfull) block.template operator()<false, M2>(c % DWR_STAGES);
            else block.template operator()<true, M2>(c % DWR_STAGES);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the clamped tail copies must not outlive the workgroup's LDS / the pass
    };
    bool redone = false;
    if constexpr (H2) {
        if (tid == 0) ring[DWR_STAGES * DWR_STAGE_FLOATS] = 0.f;
        run.template operator()<true>();
        // A half plane of THIS workgroup's operands saturated (|x * s| >= 65504: a diverged rollout): its products are wrong,
        // so the workgroup repeats its blocks with the exact three-plane split - time, never a wrong gradient.  (The
        // column sums were formed from the fp32 values and stand.)
        // (the flag word sits behind the ring in DYNAMIC LDS: __syncthreads_or would add static LDS to a 64-KiB dynamic
        // allocation, and hipFuncSetAttribute then refuses the 160-KiB dynamic limit the launch needs)
        unsigned* sat = reinterpret_cast<unsigned*>(ring + DWR_STAGES * DWR_STAGE_FLOATS);
        if (!(vmax < 65504.f)) *sat = 1u;   // (zeroed by thread 0 before the first barrier of the pass above)
        __syncthreads();
        if (*sat != 0u && redo_guard) {
            redone = true;
#pragma unroll
            for (int i = 0; i < R; ++i)
#pragma unroll
                for (int j = 0; j < R; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
            run.template operator()<false>();
        }
    } else {
        run.template operator()<false>();
    }

    const int nb = tile_n * T + wn * 64, kb = tile_k * T + wk * 64;
    float* pbase = part + (size_t)split * N * Kp;
    const float unscale = (H2 && !redone) ? 1.f / (sd * DW_H2_SA) : 1.f;   // (powers of two: exact)
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const int k = kb + 16 * j + f;
            if (k >= Kp) continue;   // (partial last K-tile)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = acc[i][j][r];
                if constexpr (H2) v *= unscale;
                pbase[(size_t)(nb + 16 * i + 4 * g + r) * Kp + k] = v;
            }
        }
    if constexpr (H2) {   // the converting threads hold the column sums: groups gg = tid & 3 of a feature sit in 4 adjacent lanes
        if (part_b != nullptr && tile_k == 0) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                float t = csum[k];
                t += __shfl_xor(t, 1);
                t += __shfl_xor(t, 2);
                if ((tid & 3) == 0) part_b[(size_t)split * N + tile_n * T + 64 * k + (tid >> 2)] = t;
            }
        }
    } else
    if (want_bias) {
#pragma unroll
        for (int i = 0; i < R; ++i) {
            float t = bsum[i];
            t += __shfl_xor(t, 16);
            t += __shfl_xor(t, 32);
            if (g == 0) part_b[(size_t)split * N + nb + 16 * i + f] = t;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Wave-specialised ring GEMM (two-half-plane products) for the layers with N % 256 == 0.  Measured on the 4-wave ring
// kernel at the target (two GEMMs per update, 165 us): without the conversion 128 us, without the MFMAs 123 us - stash
// stream (~85 us at 6 TB/s), conversion VALU and MFMAs ADD, because all waves of a workgroup convert, then all multiply, and
// the co-resident workgroup falls into the same rhythm.  Here the two kinds of work run side by side on every SIMD:
//   * 512 threads, one workgroup per CU, 256 x 128 outputs (every delta element is fetched and converted by ONE workgroup
//     per K-tile), three 48-KiB stages [D q0][D q0+1][X q0][X q0+1] of 32 samples;
//   * waves 0-3 load the fp32 fragments of later blocks into their registers and CONVERT block c + 2 into a stage (fp32 ->
//     hi / lo half planes, 6 items per thread) while waves 4-7 MULTIPLY block c (128 x 64 outputs per wave, 96 MFMAs) - the
//     register-direct feed in the kernel below;
//   * ONE barrier per block: converted block c + 2 is published, block c's stage is free for the conversion of block c + 3.
// Saturated half planes (a diverged rollout): the workgroup repeats its blocks with the exact three-plane split on the same
// four multiplying waves, from fp32 stages copied again (dw_spec_exact_pass).
// ---------------------------------------------------------------------------------------------
struct DwSpec {
    static constexpr int NW = 8, NT = 512, TN = 256, T = 128;
    static constexpr int DT = TN * 16;                       // floats of one D sample tile
    static constexpr int STAGES = 3;
    static constexpr int STAGE_FLOATS = 2 * DT + 4096;       // 48 KiB
    static constexpr int PIECES = STAGE_FLOATS / 256 / NW;   // 1-KiB copies per wave and block
    static constexpr size_t lds_bytes() { return (size_t)STAGES * STAGE_FLOATS * sizeof(float) + 16; }
};

struct DwSpecGeo {
    const float* dbase;   // D + tile_n * 256 * 16
    const float* xbase;   // X + tile_k * 128 * 16
    float* pbase;         // part + split * N * Kp
    long long Q;
    int N, Kp, split, splits, nblk, nfull, xgroups, tile_n, tile_k;
};
// copy job of a wave: pieces wave * PIECES .. + PIECES - 1 of a stage; a piece = 16 features x 16 rows (1 KiB, contiguous in the
// stash) of one sample tile of one operand, in the stage's order.  Feature groups of a partial last K-tile that do not exist
// (>= Kp) are fetched from the tile's first groups instead: finite values whose columns are never stored.
__device__ __forceinline__ void dw_spec_copy(const DwSpecGeo& G, float* ring, int c, int stage, int wave, int lane) {
    constexpr int T = DwSpec::T, TN = DwSpec::TN, PC = DwSpec::PIECES;
    const long long b0 = ((long long)G.split + (long long)c * G.splits) * 2;
    float* dst = ring + stage * DwSpec::STAGE_FLOATS + wave * PC * 256;
#pragma unroll
    for (int u = 0; u < PC; ++u) {
        const int pc = wave * PC + u;   // (wave-uniform)
        const bool isx = pc >= 2 * (TN / 16);
        const int q = isx ? pc - 2 * (TN / 16) : pc, per = isx ? T / 16 : TN / 16;
        const int st_tile = q / per;
        int grp = q - st_tile * per;
        if (isx && grp >= G.xgroups) grp %= G.xgroups;
        const size_t bq = (size_t)min(b0 + st_tile, G.Q - 1);
        const float* src = (isx ? G.xbase + bq * ((size_t)G.Kp * 16) : G.dbase + bq * ((size_t)G.N * 16)) + grp * 256 + 4 * lane;
        async_copy16_to_lds<true>(src, dst + u * 256);
    }
}
__device__ __forceinline__ void dw_spec_store(const DwSpecGeo& G, const f32x4 (&acc)[8][4], int wn, int wk, int f, int g, float unscale) {
    const int nb = G.tile_n * DwSpec::TN + wn * 128, kb = G.tile_k * DwSpec::T + wk * 64;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = kb + 16 * j + f;
            if (k >= G.Kp) continue;   // (partial last K-tile)
#pragma unroll
            for (int r = 0; r < 4; ++r) G.pbase[(size_t)(nb + 16 * i + 4 * g + r) * G.Kp + k] = acc[i][j][r] * unscale;
        }
}
// Exact pass of a workgroup whose half planes saturated: the same blocks from unconverted stages, three-plane bf16 split on
// the four multiplying waves, results stored here.  A separate (non-inlined) function: its 128 accumulator + 60 operand
// registers would otherwise shape the register allocation of the kernel's main loop.
__device__ __attribute__((noinline)) void dw_spec_exact_pass(const DwSpecGeo G, float* ring) {
    constexpr int DT = DwSpec::DT, SF = DwSpec::STAGE_FLOATS, NST = DwSpec::STAGES;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool mul_wave = wave >= 4;
    const int mw = wave & 3, wn = mw >> 1, wk = mw & 1, f = lane & 15, g = lane >> 4;
    f32x4 acc[8][4] = {};
    dw_spec_copy(G, ring, 0, 0, wave, lane);
    if (G.nblk > 1) dw_spec_copy(G, ring, 1, 1, wave, lane);
    for (int c = 0; c < G.nblk; ++c) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();   // block c (and c + 1) landed; every wave is past block c - 1
        if (c + 2 < G.nblk) dw_spec_copy(G, ring, c + 2, (c + 2) % NST, wave, lane);
        if (mul_wave) {
            const bool half_empty = c >= G.nfull;
            const float* st = ring + (c % NST) * SF;
            const float* da = st + (wn * 128 + f) * 16 + 4 * g;
            const float* xa = st + 2 * DT + (wk * 64 + f) * 16 + 4 * g;
            const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
            bf16x8 b[4][3];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x4 x0 = *reinterpret_cast<const f32x4*>(xa + 256 * j);
                const f32x4 x1 = half_empty ? zero4 : *reinterpret_cast<const f32x4*>(xa + 256 * j + 2048);
                split_frag(x0, x1, b[j]);
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const f32x4 d0 = *reinterpret_cast<const f32x4*>(da + 256 * i);
                const f32x4 d1 = half_empty ? zero4 : *reinterpret_cast<const f32x4*>(da + 256 * i + DT);
                bf16x8 a[3];
                split_frag(d0, d1, a);
                constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};   // smallest terms first
#pragma unroll
                for (int q = 0; q < 6; ++q)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[PA[q]], b[j][PB[q]], acc[i][j], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    if (mul_wave) dw_spec_store(G, acc, wn, wk, f, g, 1.f);
}

__global__ __launch_bounds__(512, 1) void dw_gemm_spec_kernel(const float* __restrict__ D, int N, const float* __restrict__ X, int Kp, long long Q,
                                                              int splits, float* __restrict__ part, float* __restrict__ part_b,
                                                              const float* __restrict__ dscale, int guard) {
    extern __shared__ __attribute__((aligned(16))) float ring[];   // [STAGES][STAGE_FLOATS] + flag word
    constexpr int T = DwSpec::T, TN = DwSpec::TN, DT = DwSpec::DT, SF = DwSpec::STAGE_FLOATS, NST = DwSpec::STAGES;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool mul_wave = wave >= 4;   // (waves w and w + 4 share a SIMD: one converting, one multiplying)
    const int tiles_k = (Kp + T - 1) / T, tiles = tiles_k * (N / TN);
    const int xcd = blockIdx.x & 7, local = blockIdx.x >> 3;   // XCD-aware order, as above
    const int tile = local % tiles, split = (local / tiles) * 8 + xcd;
    if (split >= splits) return;
    const int f = lane & 15, g = lane >> 4;
    DwSpecGeo G;
    G.tile_n = tile / tiles_k;
    G.tile_k = tile - G.tile_n * tiles_k;
    G.N = N; G.Kp = Kp; G.Q = Q; G.split = split; G.splits = splits;
    const long long nblk_all = (Q + 1) >> 1;                                  // block c of this split is block split + c * splits
    G.nblk = (int)((nblk_all - split + splits - 1) / splits);
    const bool odd_tail = (Q & 1) && ((nblk_all - 1) % splits == split);
    G.nfull = odd_tail ? G.nblk - 1 : G.nblk;
    G.xgroups = min(T, Kp - G.tile_k * T) >> 4;
    G.dbase = D + (size_t)G.tile_n * TN * 16;
    G.xbase = X + (size_t)G.tile_k * T * 16;
    G.pbase = part + (size_t)split * N * Kp;
    const int nblk = G.nblk, nfull = G.nfull;

    const int mw = wave & 3, wn = mw >> 1, wk = mw & 1;
    const float sd = f16_grad_scale(dw_delta_yardstick(dscale)) * 16.f;
    // converting waves (threads 0 .. 255): items k < 4: D feature (tid >> 2) + 64 k, k = 4, 5: X feature (tid >> 2) + 64 (k - 4);
    // sample group tid & 3.  The same items every block: the bias column sums accumulate in the converting thread.
    float vmax = 0.f, vmax_d = 0.f, vmax_x = 0.f;   // largest |delta| / |activation| this thread converted (unscaled; folded into vmax at the end)
    float csum[4] = {0.f, 0.f, 0.f, 0.f};
    const bool want_csum = part_b != nullptr && G.tile_k == 0;   // (the bias gradient = column sums of D: once per row of output tiles)

    unsigned* sat = reinterpret_cast<unsigned*>(ring + NST * SF);
    if (tid == 0) *sat = 0u;
    // Register-direct feed (round 6).  The LDS-DMA ring gave a block's copies ONE iteration to land and kept <= 48 KiB per CU in
    // flight - knock-out builds: without the MFMAs -10 us, without the conversion -1 us, i.e. the copy path set the pace (4.2 TB/s).
    // Here the four converting waves LOAD the fp32 fragments themselves (non-temporal 16-byte loads: a wave's instruction covers
    // 1 KiB of contiguous stash), hold two blocks in registers (2 x 48 of their 256), convert from registers and store only the
    // half planes: block c + 2 is converted while block c is multiplied, blocks c + 3 and c + 4 are in flight - two full
    // iterations of latency cover, ~96 KiB per CU in flight, and 144 instead of 240 KiB of LDS traffic per block.
    struct Raw { f32x4 v[6][2]; };
    Raw r0, r1;
    const int gg = tid & 3;
    long long lofs[6];   // float offset of item k inside a sample tile of its operand (+ operand / tile_k base)
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const bool isd = k < 4;
        int fe = (tid >> 2) + 64 * (isd ? k : k - 4);
        if (!isd) { int grp = fe >> 4; if (grp >= G.xgroups) grp %= G.xgroups; fe = (grp << 4) | (fe & 15); }   // partial last K-tile: finite stand-ins
        lofs[k] = (long long)fe * 16 + 4 * gg;
    }
    const size_t dtile = (size_t)N * 16, xtile = (size_t)Kp * 16;
    auto load_block = [&](int c, Raw& r) {
        const size_t q0 = (size_t)(((long long)split + (long long)c * splits) * 2);
        const bool second = c < nfull;
        const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const float* base = (k < 4 ? G.dbase + q0 * dtile : G.xbase + q0 * xtile) + lofs[k];
            r.v[k][0] = DW_STREAM_LOAD(reinterpret_cast<const f32x4*>(base));
            r.v[k][1] = second ? DW_STREAM_LOAD(reinterpret_cast<const f32x4*>(base + (k < 4 ? dtile : xtile))) : zero4;
        }
    };
    auto convert_block = [&](const Raw& r, int stage) {
        float* st = ring + stage * SF;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const bool isd = k < 4;
            const int fe = (tid >> 2) + 64 * (isd ? k : k - 4), second = isd ? DT : 2048;
            float* at = st + (isd ? 0 : 2 * DT) + fe * 16 + 4 * gg;
            const f32x4 v0 = r.v[k][0], v1 = r.v[k][1];
            if (isd && want_csum) csum[k & 3] += ((v0[0] + v0[1]) + (v0[2] + v0[3])) + ((v1[0] + v1[1]) + (v1[2] + v1[3]));
            float& vm = isd ? vmax_d : vmax_x;
            absmax2(vm, v0[0], v0[1]); absmax2(vm, v0[2], v0[3]);
            absmax2(vm, v1[0], v1[1]); absmax2(vm, v1[2], v1[3]);
            f16x8 ph, pl;
            split2h_mix(v0, v1, isd ? sd : DW_H2_SA, ph, pl);
            *reinterpret_cast<f16x8*>(at) = ph;
            *reinterpret_cast<f16x8*>(at + second) = pl;
        }
    };
    // The two kinds of waves run SEPARATE loops with the same number of barriers: the multiplying waves' 128 accumulator
    // registers and the converting waves' 96 raw-fragment registers are then live in different regions of the control-flow graph
    // and share the 256-register budget (one loop with a role branch inside keeps both live across it: spills).
    if (mul_wave) {
        f32x4 acc[8][4] = {};
        auto block_h2 = [&](int stage) {
            const float* st = ring + stage * SF;
            const float* da = st + (wn * 128 + f) * 16 + 4 * g;            // D fragments of row-tile i: + 256 i  (lo plane: + DT)
            const float* xa = st + 2 * DT + (wk * 64 + f) * 16 + 4 * g;    // X fragments of column-tile j: + 256 j  (lo plane: + 2048)
            f16x8 bh[4], bl[4];
    #pragma unroll
            for (int j = 0; j < 4; ++j) {
                bh[j] = *reinterpret_cast<const f16x8*>(xa + 256 * j);
                bl[j] = *reinterpret_cast<const f16x8*>(xa + 256 * j + 2048);
            }
            // D fragments double-buffered behind scheduling barriers (left alone, hipcc hoists all sixteen reads: 64 registers, spills)
            f16x8 ah = *reinterpret_cast<const f16x8*>(da), al = *reinterpret_cast<const f16x8*>(da + DT);
    #pragma unroll
            for (int i = 0; i < 8; ++i) {
                f16x8 nh = ah, nl = al;
                if (i + 1 < 8) {
                    nh = *reinterpret_cast<const f16x8*>(da + 256 * (i + 1));
                    nl = *reinterpret_cast<const f16x8*>(da + 256 * (i + 1) + DT);
                }
                __builtin_amdgcn_sched_barrier(0);
    #pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh[j], acc[i][j], 0, 0, 0);
    #pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl[j], acc[i][j], 0, 0, 0);
    #pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh[j], acc[i][j], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                ah = nh; al = nl;
            }
        };

        __syncthreads();                                  // blocks 0, 1 converted
        for (int c = 0; c < nblk; ++c) {
            block_h2(c % NST);
            __syncthreads();
        }
        __syncthreads();                                  // the converting waves' verdict on the half range
        if (*sat != 0u && guard) {   // a diverged rollout: time, never a wrong gradient
            dw_spec_exact_pass(G, ring);
            return;
        }
        dw_spec_store(G, acc, wn, wk, f, g, 1.f / (sd * DW_H2_SA));   // (powers of two: exact)
        return;
    }
    load_block(0, r0);   // blocks 0, 1 converted, blocks 2, 3 in flight
    if (nblk > 1) load_block(1, r1);
    convert_block(r0, 0);
    if (nblk > 2) load_block(2, r0);
    if (nblk > 1) convert_block(r1, 1);
    if (nblk > 3) load_block(3, r1);
    __syncthreads();
    auto iteration = [&](int c, Raw& r) {   // r holds block c + 2
        if (c + 2 < nblk) {
            convert_block(r, (c + 2) % NST);   // (stage of block c - 1: its multiplication ended before the last barrier)
            if (c + 4 < nblk) load_block(c + 4, r);
        }
        __syncthreads();
    };
    for (int c = 0; c < nblk; c += 2) {
        iteration(c, r0);
        if (c + 1 < nblk) iteration(c + 1, r1);
    }
    if (!mul_wave) {
        vmax = fmaxf(vmax_d * sd, vmax_x * DW_H2_SA);
        if (!(vmax < 65504.f)) *sat = 1u;
        if (want_csum) {   // groups gg = tid & 3 of a feature sit in 4 adjacent lanes (formed from the fp32 values)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float t = csum[k];
                t += __shfl_xor(t, 1);
                t += __shfl_xor(t, 2);
                if ((tid & 3) == 0) part_b[(size_t)split * N + G.tile_n * TN + 64 * k + (tid >> 2)] = t;
            }
        }
    }
    __syncthreads();
    if (*sat != 0u && guard) {   // a diverged rollout: time, never a wrong gradient
        dw_spec_exact_pass(G, ring);
        return;
    }
}

// ---------------------------------------------------------------------------------------------
// Weight gradient of a layer with 16 (padded) inputs - layer 0 of the pyth_lq / pyth_idpendulum / gym / mobilerobot nets:
// dW[n][k] = sum_s D[s][n] X[s][k], k < 16.  Bound by the D stream (4 N bytes per sample; X adds 64): with 16 output columns
// the matrix core has next to nothing to do (4 MFMAs per 16 features and sample tile), so the products are EXACT fp32
// (`v_mfma_f32_16x16x4_f32`) - no operand split, no scale, no fallback; the 64 x 64-tile kernel above spends three quarters
// of its splits and MFMAs on padding columns here (cfg5: 138 us for 335 MB).  Lane (f, g) of a fragment holds samples
// 4g .. 4g+3 of feature f - ONE 16-byte load per 16 features x 16 samples, a contiguous KiB per wave; MFMA e of a tile
// contracts samples {e, 4 + e, 8 + e, 12 + e} (element e of every lane's vector, the same order for both operands).
// Workgroup = 4 waves x up to 4 blocks of 16 features (256 features); split s takes the sample tiles s, s + splits, ...;
// two batches of DWK_U tiles alternate in registers (one in flight while the other is multiplied).
// ---------------------------------------------------------------------------------------------
#define DWK_U 2
__global__ __launch_bounds__(NTHREADS, 3) void dw_skinny_kernel(const float* __restrict__ D, int N, const float* __restrict__ X, long long Q,
                                                                 int splits, float* __restrict__ part, float* __restrict__ part_b) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f = lane & 15, g = lane >> 4;
    const int ngroups = (N + 255) / 256;
    const int xcd = blockIdx.x & 7, local = blockIdx.x >> 3;   // XCD-aware order, as above
    const int grp = local % ngroups, split = (local / ngroups) * 8 + xcd;
    if (split >= splits) return;
    int doff[4], nfeat[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        nfeat[i] = 256 * grp + 16 * (wave + 4 * i);                       // first feature of this wave's block i
        doff[i] = min(nfeat[i] + f, N - 1) * 16 + 4 * g;                  // (blocks past N: clamped, never stored)
    }
    const int xoff = f * 16 + 4 * g;
    const GLOBAL_AS float* Dg = gptr(D);
    const GLOBAL_AS float* Xg = gptr(X);
    const size_t dtile = (size_t)N * 16;
    struct Batch { f32x4 d[DWK_U][4]; f32x4 x[DWK_U]; };
    auto load = [&](long long q0, Batch& b) {   // tiles q0, q0 + splits, ...: past the end -> the last tile with X = 0
#pragma unroll
        for (int u = 0; u < DWK_U; ++u) {
            const long long q = q0 + (long long)u * splits;
            const size_t qq = (size_t)min(q, Q - 1);
#pragma unroll
            for (int i = 0; i < 4; ++i) b.d[u][i] = DW_STREAM_LOAD(reinterpret_cast<const GLOBAL_AS f32x4*>(Dg + qq * dtile + doff[i]));
            b.x[u] = DW_STREAM_LOAD(reinterpret_cast<const GLOBAL_AS f32x4*>(Xg + qq * 256 + xoff));
        }
    };
    f32x4 acc[4] = {};
    float bsum[4] = {0.f, 0.f, 0.f, 0.f};
    auto mul = [&](long long q0, const Batch& b) {
#pragma unroll
        for (int u = 0; u < DWK_U; ++u) {
            const bool live = q0 + (long long)u * splits < Q;
            f32x4 x = b.x[u];
#pragma unroll
            for (int e = 0; e < 4; ++e) x[e] = live ? x[e] : 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const f32x4 d = b.d[u][i];
                bsum[i] += live ? (d[0] + d[1]) + (d[2] + d[3]) : 0.f;
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(d[e], x[e], acc[i], 0, 0, 0);
            }
        }
    };
    const long long stride = (long long)DWK_U * splits;
    Batch b0, b1;
    load(split, b0);
    for (long long q = split; q < Q; q += 2 * stride) {
        load(q + stride, b1);
        mul(q, b0);
        load(q + 2 * stride, b0);
        mul(q + stride, b1);
    }
    float* pbase = part + (size_t)split * N * 16;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (nfeat[i] >= N) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) pbase[(size_t)(nfeat[i] + 4 * g + r) * 16 + f] = acc[i][r];
        if (part_b != nullptr) {
            float t = bsum[i];
            t += __shfl_xor(t, 16);
            t += __shfl_xor(t, 32);
            if (g == 0) part_b[(size_t)split * N + nfeat[i] + f] = t;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// dW GEMM, half-precision operands (GOPS_DTYPE_F16):  part[split][n][k] = sum_s D[s][n] * X[s][k] with D, X
// row-major _Float16 stash tiles, fp32 accumulation on v_mfma_f32_16x16x32_f16.  Same decomposition as the
// bf16x3 kernel (128 x 128 outputs per workgroup, 2 x 2 waves of 64 x 64, split-K over samples, XCD-aware
// block order); a chunk is 64 samples = two MFMA K-steps.  The contraction index (samples) is the ROW
// index of both operands in memory, so the staging transposes: a thread loads 4 rows x 8 columns (one
// dwordx4 per row, 256-byte coalesced rows), regroups them with v_perm_b32 into 8 columns x 4 samples and
// writes [g = s/8][column][8 samples] fragments (ds_write_b64); a lane's MFMA fragment is one ds_read_b128.
// 16-byte units are XOR-swizzled (column ^ (column >> 3 & 7)) so that both directions are conflict-free.
// ---------------------------------------------------------------------------------------------
#define DWH_T 128                       // tile edge
#define DWH_PLANE (8 * DWH_T * 8)       // halfs per operand: [8 g][128 cols][8 samples]

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(NTHREADS, 2) void dw_gemm_f16_kernel(const _Float16* __restrict__ D, int N,
                                                                   const _Float16* __restrict__ X, int Kp,
                                                                   long long S, int splits, int chunks_per_split,
                                                                   float* __restrict__ part,
                                                                   float* __restrict__ part_b) {
    __shared__ __attribute__((aligned(16))) _Float16 As[DWH_PLANE];   // D^T
    __shared__ __attribute__((aligned(16))) _Float16 Bs[DWH_PLANE];   // X
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tiles_k = (Kp + DWH_T - 1) / DWH_T, tiles = tiles_k * ((N + DWH_T - 1) / DWH_T);
    const int xcd = blockIdx.x & 7, local = blockIdx.x >> 3;   // same XCD-aware order as dw_gemm_kernel
    const int tile = local % tiles, split = (local / tiles) * 8 + xcd;
    if (split >= splits) return;
    const int tile_n = tile / tiles_k, tile_k = tile - tile_n * tiles_k;
    const int n0 = tile_n * DWH_T, k0 = tile_k * DWH_T;
    const long long s_begin = (long long)split * chunks_per_split * DWH_SC;
    const int wn = wave >> 1, wk = wave & 1;

    // Staging item of this thread: columns 8*c8 .. +7, samples 4*s4 .. +3 of the chunk.  Lane bits ->
    // (s4 bit 0, c8 bits 0..2, c8 bit 3, s4 bit 1), wave -> s4 bits 2..3: one load instruction covers four
    // full 256-byte rows, and the 16 lanes of a ds_write_b64 group hit 16 distinct 8-byte slots.
    const int c8 = ((lane >> 1) & 7) | (((lane >> 4) & 1) << 3);
    const int s4 = (lane & 1) | (((lane >> 5) & 1) << 1) | (wave << 2);
    int wofs[8];   // LDS half-offset of column 8*c8 + i
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int n = 8 * c8 + i, nsw = n ^ ((n >> 3) & 7);
        wofs[i] = (((s4 >> 1) * DWH_T + nsw) << 3) + ((s4 & 1) << 2);
    }
    const bool want_bias = part_b != nullptr && tile_k == 0;

    f32x4 acc[4][4] = {};
    u32x4 dreg[4], xreg[4];
    float bsum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

    auto gload = [&](long long s0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long srow = s0 + 4 * s4 + r;
            const int n = n0 + 8 * c8, k = k0 + 8 * c8;
            const u32x4 z = {0u, 0u, 0u, 0u};
            // (default cache policy: with 128 x 128 output tiles every operand slice is read by two workgroups, the second time from
            // L2 - the non-temporal policy measured 2 % slower here, cfg5 fp16)
            dreg[r] = (srow < S && n < N) ? *reinterpret_cast<const u32x4*>(D + srow * N + n) : z;
            xreg[r] = (srow < S && k < Kp) ? *reinterpret_cast<const u32x4*>(X + srow * Kp + k) : z;
        }
    };
    // 4 rows x 8 halfs -> for each column pair (2w, 2w+1): samples 0..3 as two dwords each
    auto lstore = [&]<bool SUM>(const u32x4& q0, const u32x4& q1, const u32x4& q2, const u32x4& q3, _Float16* base) {
        #pragma unroll
        for (int w = 0; w < 4; ++w) {
            const unsigned r0w = q0[w], r1w = q1[w], r2w = q2[w], r3w = q3[w];
            // (low halfs of rows 0,1), (rows 2,3) = column 2w; (high halfs) = column 2w+1  (hipcc folds these to v_perm_b32)
            const unsigned lo01 = (r0w & 0xffffu) | (r1w << 16), lo23 = (r2w & 0xffffu) | (r3w << 16);
            const unsigned hi01 = (r0w >> 16) | (r1w & 0xffff0000u), hi23 = (r2w >> 16) | (r3w & 0xffff0000u);
            { const u32x2 v = {lo01, lo23}; *reinterpret_cast<u32x2*>(base + wofs[2 * w]) = v; }
            { const u32x2 v = {hi01, hi23}; *reinterpret_cast<u32x2*>(base + wofs[2 * w + 1]) = v; }
            if (SUM && want_bias) {
                const f16x2 a0 = __builtin_bit_cast(f16x2, lo01), a1 = __builtin_bit_cast(f16x2, lo23);
                const f16x2 b0 = __builtin_bit_cast(f16x2, hi01), b1 = __builtin_bit_cast(f16x2, hi23);
                bsum[2 * w] += ((float)a0[0] + (float)a0[1]) + ((float)a1[0] + (float)a1[1]);
                bsum[2 * w + 1] += ((float)b0[0] + (float)b0[1]) + ((float)b1[0] + (float)b1[1]);
            }
        }
    };
    // fragment (8 consecutive samples of tile-local column `col`) of this lane in K-step ks
    auto frag = [&](const _Float16* base, int ks, int col) {
        const int nsw = col ^ ((col >> 3) & 7);
        return *reinterpret_cast<const f16x8*>(base + (((4 * ks + (lane >> 4)) * DWH_T + nsw) << 3));
    };

    gload(s_begin);
    for (int c = 0; c < chunks_per_split; ++c) {
        __syncthreads();
        lstore.template operator()<true>(dreg[0], dreg[1], dreg[2], dreg[3], As);
        lstore.template operator()<false>(xreg[0], xreg[1], xreg[2], xreg[3], Bs);
        __syncthreads();
        if (c + 1 < chunks_per_split) gload(s_begin + (long long)(c + 1) * DWH_SC);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            f16x8 b[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = frag(Bs, ks, wk * 64 + 16 * j + (lane & 15));
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const f16x8 a = frag(As, ks, wn * 64 + 16 * i + (lane & 15));
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b[j], acc[i][j], 0, 0, 0);
            }
        }
    }
    float* pbase = part + (size_t)split * N * Kp;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = k0 + wk * 64 + 16 * j + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = n0 + wn * 64 + 16 * i + 4 * (lane >> 4) + r;
                if (n < N && k < Kp) pbase[(size_t)n * Kp + k] = acc[i][j][r];
            }
        }
    if (want_bias) {   // column sums of D: 16 sample groups per column, combined in a fixed order
        __syncthreads();
        float* red = reinterpret_cast<float*>(As);   // [16][128] floats = 8 KiB of the 16 KiB plane
#pragma unroll
        for (int i = 0; i < 8; ++i) red[s4 * DWH_T + 8 * c8 + i] = bsum[i];
        __syncthreads();
        if (tid < DWH_T && n0 + tid < N) {
            float t = 0.f;
#pragma unroll
            for (int q = 0; q < 16; ++q) t += red[q * DWH_T + tid];
            part_b[(size_t)split * N + n0 + tid] = t;
        }
    }
}

// Output layer (width A <= 4) on the VALU: part[split][a][k] = sum_s dy[s][a] * h[s][k].
// Row-major half h (GOPS_DTYPE_F16 stash): thread = (8 columns, sample lane): one 16-byte read of h per sample, four samples
// in flight per thread (a workgroup keeps 16 KiB of the stream in flight; the round-3 form - 8-byte reads, 8 KiB - ran at
// 2.6 TB/s); the two sample lanes of a wave are combined by a lane exchange, the four waves through LDS, in a fixed order.
__global__ __launch_bounds__(NTHREADS) void dw_out_h_kernel(const float* __restrict__ dy, const _Float16* __restrict__ h, int K, int A,
                                                            long long S, long long per_split, float* __restrict__ part,
                                                            float* __restrict__ part_b) {
    __shared__ __attribute__((aligned(16))) float red[4][GOPS_MAX_ACT][256];
    __shared__ float redb[4][GOPS_MAX_ACT];
    const int split = blockIdx.x, tid = threadIdx.x, c8 = tid & 31, sl = tid >> 5, wave = tid >> 6;
    const long long s0 = split * per_split, s1 = min(S, s0 + per_split);
    const int nblk = K >> 3;   // (half nets: K is a multiple of 64)
    for (int cb0 = 0; cb0 < nblk; cb0 += 32) {   // uniform trip count: every lane reaches the barriers
        const int cb = cb0 + c8;
        const bool col_ok = cb < nblk;
        float acc[GOPS_MAX_ACT][8] = {};
        float accb[GOPS_MAX_ACT] = {0.f, 0.f, 0.f, 0.f};
        if (col_ok) {
            const GLOBAL_AS _Float16* hp = gptr(h) + 8 * cb;
#pragma unroll 4
            for (long long sidx = s0 + sl; sidx < s1; sidx += 8) {
                const f32x4 g = *gptr(reinterpret_cast<const f32x4*>(dy) + sidx);
                const f16x8 hv = *reinterpret_cast<const GLOBAL_AS f16x8*>(hp + sidx * K);
#pragma unroll
                for (int a = 0; a < GOPS_MAX_ACT; ++a) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[a][e] = fmaf(g[a], (float)hv[e], acc[a][e]);
                    accb[a] += g[a];
                }
            }
        }
#pragma unroll
        for (int a = 0; a < GOPS_MAX_ACT; ++a) {
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[a][e] += __shfl_xor(acc[a][e], 32);
            accb[a] += __shfl_xor(accb[a], 32);
        }
        if ((tid & 32) == 0) {
#pragma unroll
            for (int a = 0; a < GOPS_MAX_ACT; ++a) {
                *reinterpret_cast<f32x4*>(&red[wave][a][8 * c8]) = f32x4{acc[a][0], acc[a][1], acc[a][2], acc[a][3]};
                *reinterpret_cast<f32x4*>(&red[wave][a][8 * c8 + 4]) = f32x4{acc[a][4], acc[a][5], acc[a][6], acc[a][7]};
            }
            if (c8 == 0 && cb0 == 0)
                for (int a = 0; a < GOPS_MAX_ACT; ++a) redb[wave][a] = accb[a];
        }
        __syncthreads();
        const int k = 8 * cb0 + tid;
        if (k < K)
            for (int a = 0; a < A; ++a)
                part[((size_t)split * A + a) * K + k] = (red[0][a][tid] + red[1][a][tid]) + (red[2][a][tid] + red[3][a][tid]);
        if (tid == 0 && cb0 == 0)
            for (int a = 0; a < A; ++a) part_b[(size_t)split * A + a] = (redb[0][a] + redb[1][a]) + (redb[2][a] + redb[3][a]);
        __syncthreads();
    }
}

// Feature-major fp32 h (common.h StashDev): a split is a run of whole sample tiles; thread k owns feature k - its 16
// rows of a tile are 64 contiguous bytes, a wave reads 4 contiguous KiB per tile - and needs no cross-thread reduction;
// the tile's 16 x 4 block of dy is the same for every thread (uniform loads through the scalar cache).
__global__ __launch_bounds__(NTHREADS) void dw_out_fm_kernel(const float* __restrict__ dy, const float* __restrict__ h, int K, int A,
                                                             long long Q, long long tiles_per_split,
                                                             float* __restrict__ part, float* __restrict__ part_b) {
    const int split = blockIdx.x;
    const long long q0 = split * tiles_per_split, q1 = min(Q, q0 + tiles_per_split);
    for (int k = threadIdx.x; k < ((K + NTHREADS - 1) / NTHREADS) * NTHREADS; k += NTHREADS) {
        const bool col_ok = k < K;
        const int kc = col_ok ? k : K - 1;
        float acc[GOPS_MAX_ACT] = {0.f, 0.f, 0.f, 0.f}, accb[GOPS_MAX_ACT] = {0.f, 0.f, 0.f, 0.f};
        for (long long qb = q0; qb < q1; qb += 2) {   // two tiles (8 vectors) in flight per thread
            f32x4 hv[2][4];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const long long q = min(qb + u, q1 - 1);
#pragma unroll
                for (int rg = 0; rg < 4; ++rg) hv[u][rg] = ld4(gptr(h) + ((size_t)q * K + kc) * 16 + 4 * rg);
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                if (qb + u < q1) {
                    const f32x4* gp = reinterpret_cast<const f32x4*>(dy) + (size_t)(qb + u) * 16;   // uniform: [16 rows][4]
#pragma unroll
                    for (int m = 0; m < 16; ++m) {
                        const f32x4 g = gp[m];
#pragma unroll
                        for (int a = 0; a < GOPS_MAX_ACT; ++a) { acc[a] += g[a] * hv[u][m >> 2][m & 3]; accb[a] += g[a]; }
                    }
                }
            }
        }
        if (col_ok) {
            for (int a = 0; a < A; ++a) part[((size_t)split * A + a) * K + k] = acc[a];
            if (k == 0)
                for (int a = 0; a < A; ++a) part_b[(size_t)split * A + a] = accb[a];
        }
    }
}

// ---------------------------------------------------------------------------------------------
// The weight-gradient stage's record (dw_plan.h): which of the kernels above forms a layer's partial slabs, on which grid.
// ---------------------------------------------------------------------------------------------
static_assert(DW_SC == 2 * TB, "a K-block of the fp32 dW GEMMs is two sample tiles (nblk_all = (Q + 1) >> 1)");
static inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// The layers the 16-input kernel takes
bool dw_skinny_ok(int N, int Kp) { return Kp == 16 && (N % 16) == 0; }

DwLayer plan_dw(int N, int K, int Kp, long long S, bool f16, int wg_target) {
    DwLayer L;
    L.N = N, L.K = K, L.Kp = Kp, L.S = S, L.ld = Kp;
    L.tile = (f16 || (N >= 128 && Kp >= 128)) ? 128 : 64;   // (the half-precision GEMM has one tile size, DWH_T)
    // Workgroups per split that the split count is derived from.  This is the launched grid's number but for two cases, kept as
    // they are because another count would move the split-K summation order (and the benchmark): a layer that choose_dw_gemm
    // gives to dw_gemm_spec_kernel is counted in 128 x 128 tiles although that kernel's are 256 x 128 (half as many workgroups
    // as counted), and a 16-input layer is counted as the skinny kernel's even where GOPS_VF_DW_F32 moves it to 64 x 64 tiles.
    const int counted = (!f16 && dw_skinny_ok(N, Kp)) ? cdiv(N, 256) : cdiv(N, L.tile) * cdiv(Kp, L.tile);
    const int sc = f16 ? DWH_SC : DW_SC;
    const long long chunks = (S + sc - 1) / sc;
    if (wg_target < 1) wg_target = 512;
    long long splits = (wg_target + counted - 1) / counted;
    if (splits > chunks) splits = chunks;
    if (splits < 1) splits = 1;
    L.chunks_per_split = (int)((chunks + splits - 1) / splits);
    L.splits = (int)((chunks + L.chunks_per_split - 1) / L.chunks_per_split);
    L.slab_w = (size_t)L.splits * N * Kp;
    L.slab_b = (size_t)L.splits * N;
    return L;
}

DwLayer plan_dw_out(int K, int A, long long S) {
    DwLayer L;
    L.N = A, L.K = L.Kp = L.ld = K, L.S = S;
    L.splits = (int)std::min<long long>(DW_OUT_SPLITS, S);
    L.slab_w = (size_t)DW_OUT_SPLITS * GOPS_MAX_ACT * K;
    L.slab_b = (size_t)DW_OUT_SPLITS * GOPS_MAX_ACT;
    return L;
}

// With the delta scale the large layers run the two-half-plane products (22 significant bits per operand); without it - or
// with GOPS_VF_DW_EXACT in the description's variant flags - the exact three-plane bf16 split.
void choose_dw_gemm(DwLayer& L, bool f16, bool scaled, unsigned vflags) {
    const int N = L.N, Kp = L.Kp;
    const bool f32 = (vflags & GOPS_VF_DW_F32) != 0, big = L.tile == 128;   // (A/B knob: fp32 MFMA GEMM)
    int tiles = cdiv(N, L.tile) * cdiv(Kp, L.tile);
    L.block = NTHREADS, L.lds = 0;
    L.guard = (vflags & GOPS_VF_DW_NO_GUARD) ? 0 : 1;   // (test knob: skip the exact re-run behind a saturated launch)
    if (f16) {
        L.kernel = DwKernel::F16;
    } else if (!f32 && big && (N % 128) == 0 && ((Kp % 128) == 0 || (Kp > 128 && (Kp % 16) == 0))) {   // the ring kernels' shapes
        const bool h2 = scaled && !(vflags & GOPS_VF_DW_EXACT);
        L.kernel = !h2 ? DwKernel::RingExact : ((N % 256) == 0 ? DwKernel::Spec : DwKernel::RingH2);   // (DwSpec::TN = 256 features)
        L.lds = (size_t)DWR_STAGES * DWR_STAGE_FLOATS * sizeof(float) + (h2 ? 16 : 0);
        if (L.kernel == DwKernel::Spec) tiles = (N / DwSpec::TN) * cdiv(Kp, DwSpec::T), L.block = DwSpec::NT, L.lds = DwSpec::lds_bytes();
    } else if (!f32 && dw_skinny_ok(N, Kp)) {
        L.kernel = DwKernel::Skinny;
        tiles = cdiv(N, 256);
    } else {
        L.kernel = big ? (f32 ? DwKernel::Fm4F32 : DwKernel::Fm4Bf3) : (f32 ? DwKernel::Fm2F32 : DwKernel::Fm2Bf3);
    }
    L.grid = tiles * cdiv(L.splits, 8) * 8;   // (XCD-aware block order: splits in groups of 8)
}

void choose_dw_out(DwLayer& L, bool f16) {
    L.kernel = f16 ? DwKernel::OutH : DwKernel::OutFm;
    L.grid = L.splits, L.block = NTHREADS, L.lds = 0;
}

bool choose_dw_in_sweep(DwLayer& L, int slabs, int ld) {
    if ((size_t)slabs * L.N * ld > L.slab_w || (size_t)slabs * L.N > L.slab_b) return false;
    L.kernel = DwKernel::InSweep;
    L.splits = slabs, L.ld = ld;
    L.grid = L.block = 0, L.lds = 0;
    return true;
}

hipError_t launch_dw(const DwLayer& L, const void* Dv, const void* Xv, float* part, float* part_b, const float* dscale, hipStream_t s) {
    const float* D = static_cast<const float*>(Dv);
    const float* X = static_cast<const float*>(Xv);
    const _Float16* Xh = static_cast<const _Float16*>(Xv);
    const float* none = nullptr;
    const dim3 grid(L.grid), block(L.block);
    const long long Q = (L.S + TB - 1) / TB;
    auto fm = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, block, 0, s, D, L.N, X, L.Kp, Q, L.splits, L.chunks_per_split, part, part_b); };
    auto ring = [&](auto kernel, const float* scale, int guard) {
        launch_with_lds(kernel, grid, block, L.lds, s, D, L.N, X, L.Kp, Q, L.splits, L.chunks_per_split, part, part_b, scale, guard);
    };
    switch (L.kernel) {
        case DwKernel::None:
        case DwKernel::InSweep: return hipSuccess;
        case DwKernel::Spec: launch_with_lds(dw_gemm_spec_kernel, grid, block, L.lds, s, D, L.N, X, L.Kp, Q, L.splits, part, part_b, dscale, L.guard); break;
        case DwKernel::RingH2: ring(dw_gemm_ring_kernel<true>, dscale, L.guard); break;
        case DwKernel::RingExact: ring(dw_gemm_ring_kernel<false>, none, 1); break;
        case DwKernel::Skinny: hipLaunchKernelGGL(dw_skinny_kernel, grid, block, 0, s, D, L.N, X, Q, L.splits, part, part_b); break;
        case DwKernel::Fm4Bf3: fm(dw_gemm_fm_kernel<4, true>); break;
        case DwKernel::Fm4F32: fm(dw_gemm_fm_kernel<4, false>); break;
        case DwKernel::Fm2Bf3: fm(dw_gemm_fm_kernel<2, true>); break;
        case DwKernel::Fm2F32: fm(dw_gemm_fm_kernel<2, false>); break;
        case DwKernel::F16:
            hipLaunchKernelGGL(dw_gemm_f16_kernel, grid, block, 0, s, static_cast<const _Float16*>(Dv), L.N, Xh, L.Kp, L.S, L.splits,
                               L.chunks_per_split, part, part_b);
            break;
        case DwKernel::OutH:
            hipLaunchKernelGGL(dw_out_h_kernel, grid, block, 0, s, D, Xh, L.K, L.N, L.S, (L.S + L.splits - 1) / L.splits, part, part_b);
            break;
        case DwKernel::OutFm:   // splits beyond the tile count produce zero slabs (their loops are empty)
            hipLaunchKernelGGL(dw_out_fm_kernel, grid, block, 0, s, D, X, L.K, L.N, Q, (Q + L.splits - 1) / L.splits, part, part_b);
            break;
    }
    return hipGetLastError();
}

// Sum of n values in double, one block, in batch_loss_kernel's single-block order (optim.hip; the two produce the same bits):
// mean_stats[0] = sc * mean(x), mean_stats[1] = mean(x).
__device__ __forceinline__ void mean_block(const float* __restrict__ a, int n, float sc, float* __restrict__ stats, double (*red2)[4]) {
    double s[2] = {0.0, 0.0};
    for (int i0 = threadIdx.x; i0 < n; i0 += 8 * 256) {
        float av[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int i = i0 + q * 256;
            av[q] = i < n ? a[i] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (i0 + q * 256 < n) { s[0] += (double)av[q]; s[1] += (double)av[q]; }
    }
    block_fold<2, false>(s, red2);
    if (threadIdx.x == 0) {
        stats[0] = (float)((double)sc * s[0] / (double)n);
        stats[1] = (float)(s[1] / (double)n);
    }
}

// out[r][c] = sum_split part[split][r][c]   for c < cols (row stride `ld` inside a split), for every
// job of the table in ONE launch.  Block = 64 outputs x 4 split lanes; each lane sums every 4th split
// with independent loads in flight, then the 4 lanes are combined through LDS (fixed order ->
// deterministic).
__global__ __launch_bounds__(256) void reduce_partials_kernel(const ReduceJobs jobs) {
    __shared__ float red[4][64];
    __shared__ double red2[2][4];
    if (jobs.reset != nullptr && blockIdx.x == 0 && threadIdx.x == 0) jobs.reset[0] = jobs.reset[1] = 0.f;
    // fused Adam step (gops_rollout_backward_update): this step's scalar factors, left by the sweep kernel of the same call
    // (common.h adam_snapshot: adam_kernel's, formed once instead of per block)
    const bool adam = jobs.ad_snap != nullptr;
    float step_size = 0.f, bc2_sqrt = 1.f, omb1 = 0.f, omb2 = 0.f, b2 = 0.f, gsc = 1.f;
    if (adam) {
        step_size = jobs.ad_snap[0]; bc2_sqrt = jobs.ad_snap[1]; gsc = jobs.ad_snap[2];
        omb1 = (float)(1.0 - jobs.ad_b1); omb2 = (float)(1.0 - jobs.ad_b2); b2 = (float)jobs.ad_b2;
    }
    if ((int)blockIdx.x >= jobs.block0[jobs.n]) {   // the extra block: the loss mean
        mean_block(jobs.mean_x, jobs.mean_n, jobs.mean_sc, jobs.mean_stats, red2);
    } else {
    int j = 0;
    while (j + 1 < jobs.n && (int)blockIdx.x >= jobs.block0[j + 1]) ++j;
    const float* __restrict__ part = jobs.part[j];
    const int splits = jobs.splits[j], rows = jobs.rows[j], cols = jobs.cols[j], ld = jobs.ld[j];
    const int o = threadIdx.x & 63, sl = threadIdx.x >> 6;
    const int idx = (blockIdx.x - jobs.block0[j]) * 64 + o;
    const bool valid = idx < rows * cols;
    // the element's Adam operands travel with the partial sums (they are needed when the sums are)
    float pm = 0.f, pv = 0.f, pp = 0.f;
    const bool step_here = adam && jobs.ad_p[j] != nullptr && sl == 0 && valid;
    float pt = 0.f;
    const bool avg_here = step_here && jobs.pk_t[j] != nullptr;
    if (step_here) { pm = jobs.ad_m[j][idx]; pv = jobs.ad_v[j][idx]; pp = jobs.ad_p[j][idx]; }
    if (avg_here) pt = jobs.pk_t[j][idx];
    float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, acc3 = 0.f;
    if (valid) {
        const int r = idx / cols, c = idx - r * cols;
        const size_t stride = (size_t)jobs.slab_rows[j] * ld;
        const float* p = part + (size_t)r * ld + c;
        int s = sl;
        // 8 independent loads in flight per thread (the kernel is latency-bound: one 256-byte row segment per wave and
        // split); the pairs are added in a fixed order, so the result does not depend on the unrolling
        // (jobs with hundreds of splits - one slab per sweep workgroup, rollout_h64.hip's fused first-layer gradient: 1024 at cfg5 -
        // take 16 at a time; element i of a thread's sequence goes to accumulator i % 4 in every form of the loop, so the sums
        // do not depend on which form ran)
        for (; s + 60 < splits; s += 64) {
            float v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = DW_STREAM_LOAD(p + (size_t)(s + 4 * u) * stride);
#pragma unroll
            for (int u = 0; u < 16; u += 4) { acc0 += v[u]; acc1 += v[u + 1]; acc2 += v[u + 2]; acc3 += v[u + 3]; }
        }
        for (; s + 28 < splits; s += 32) {
            const float v0 = DW_STREAM_LOAD(p + (size_t)s * stride), v1 = DW_STREAM_LOAD(p + (size_t)(s + 4) * stride),
                        v2 = DW_STREAM_LOAD(p + (size_t)(s + 8) * stride), v3 = DW_STREAM_LOAD(p + (size_t)(s + 12) * stride),
                        v4 = DW_STREAM_LOAD(p + (size_t)(s + 16) * stride), v5 = DW_STREAM_LOAD(p + (size_t)(s + 20) * stride),
                        v6 = DW_STREAM_LOAD(p + (size_t)(s + 24) * stride), v7 = DW_STREAM_LOAD(p + (size_t)(s + 28) * stride);
            acc0 += v0; acc1 += v1; acc2 += v2; acc3 += v3;
            acc0 += v4; acc1 += v5; acc2 += v6; acc3 += v7;
        }
        for (; s + 12 < splits; s += 16) {
            acc0 += p[(size_t)s * stride];
            acc1 += p[(size_t)(s + 4) * stride];
            acc2 += p[(size_t)(s + 8) * stride];
            acc3 += p[(size_t)(s + 12) * stride];
        }
        for (; s < splits; s += 4) acc0 += p[(size_t)s * stride];
    }
    red[sl][o] = (acc0 + acc1) + (acc2 + acc3);
    __syncthreads();
    if (sl == 0 && valid) {
        float t = (red[0][o] + red[1][o]) + (red[2][o] + red[3][o]);
        if (jobs.unscale != nullptr) t *= 1.f / f16_grad_scale(*jobs.unscale);   // power of two: exact
        // a plane conversion of the forward or of the sweep left the half range (their tiles' returns / one delta are NaN already):
        // no element of this call's gradient is to be trusted - all of them leave as NaN, and none takes an optimizer step
        if (jobs.poison != nullptr && *jobs.poison != 0u) t = __builtin_nanf("");
        jobs.out[j][idx] = t;
        if (step_here && !grad_is_finite(t * gsc)) {
            atomicAdd(jobs.ad_skipped, 1u);   // (only on the failure path: no contention in a healthy update)
        } else if (step_here) {   // adam_kernel's element, then polyak_kernel's
            adam_element(t * gsc, pm, pv, pp, step_size, bc2_sqrt, omb1, omb2, b2, jobs.ad_eps);
            jobs.ad_m[j][idx] = pm;
            jobs.ad_v[j][idx] = pv;
            jobs.ad_p[j][idx] = pp;
            if (avg_here) jobs.pk_t[j][idx] = polyak_element(pt, pp, jobs.pk_omt, jobs.pk_tau);
        }
    }
    }
}

void reduce_jobs_add(ReduceJobs& jobs, const float* part, int splits, int rows, int cols, int ld, float* out, int slab_rows) {
    const int i = jobs.n++;
    jobs.part[i] = part; jobs.out[i] = out;
    jobs.splits[i] = splits; jobs.rows[i] = rows; jobs.cols[i] = cols; jobs.ld[i] = ld;
    jobs.slab_rows[i] = slab_rows > 0 ? slab_rows : rows;
    if (i == 0) jobs.block0[0] = 0;
    jobs.block0[i + 1] = jobs.block0[i] + (rows * cols + 63) / 64;
}
void add_reduce_jobs(ReduceJobs& jobs, const DwLayer& L, const float* part, const float* part_b, int rows, float* gw, float* gb) {
    reduce_jobs_add(jobs, part, L.splits, rows, L.K, L.ld, gw, L.N);
    reduce_jobs_add(jobs, part_b, L.splits, 1, rows, L.N, gb);
}

hipError_t launch_reduce(const ReduceJobs& jobs_in, hipStream_t s) {
    if (jobs_in.n == 0) return hipSuccess;
    ReduceJobs jobs = jobs_in;
    const bool own_mean = jobs.mean_x != nullptr && jobs.mean_n > LOSS_ONE_BLOCK_MAX;   // too long for one block: its own launch
    if (own_mean) jobs.mean_x = nullptr;
    hipLaunchKernelGGL(reduce_partials_kernel, dim3(jobs.block0[jobs.n] + (jobs.mean_x != nullptr ? 1 : 0)), dim3(256), 0, s, jobs);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && own_mean) e = launch_batch_loss(jobs_in.mean_x, nullptr, jobs_in.mean_n, 0.f, jobs_in.mean_sc, nullptr, jobs_in.mean_stats, s);
    return e;
}
