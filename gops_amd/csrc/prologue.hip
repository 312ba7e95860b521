// What a rollout forward prepares before its kernels run: the parameter block's upload, the MFMA-fragment and plane-split
// weight packings, and the reference / surrounding-vehicle tables - all of it in the one launch of prologue_kernel.
#include "common.h"
#include "env_models.h"
#include "env_step.h"
#include "launchers.h"

// ---------------------------------------------------------------------------------------------
// Weight packing.  For Linear layer W [N][K] (torch layout):
//   fwd:  element ((nt*kch + c)*64 + lane)*4 + i  =  W[16nt + (lane&15)][16c + 4(lane>>4) + i]
//   bwd:  element ((nt*kch + c)*64 + lane)*4 + i  =  W[16c + 4(lane>>4) + i][16nt + (lane&15)]
// (zero where the input index is in the padding), so that lane `lane` fetches with one dwordx4 the
// B operands of four consecutive v_mfma_f32_16x16x4_f32.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void pack_element(const float* __restrict__ W, int N, int K, int Kp,
                                             float* __restrict__ wp, float* __restrict__ wpt, int e) {
    if (e >= N * Kp) return;
    const int i = e & 3, lane = (e >> 2) & 63, blk = e >> 8;
    {   // forward: n tiles over N, chunks over Kp
        const int kch = Kp >> 4, nt = blk / kch, c = blk - nt * kch;
        const int n = 16 * nt + (lane & 15), k = 16 * c + 4 * (lane >> 4) + i;
        wp[e] = (k < K) ? W[(size_t)n * K + k] : 0.f;
    }
    {   // backward: n tiles over Kp (input index), chunks over N (output index)
        const int kch = N >> 4, nt = blk / kch, c = blk - nt * kch;
        const int kin = 16 * nt + (lane & 15), nout = 16 * c + 4 * (lane >> 4) + i;
        wpt[e] = (kin < K) ? W[(size_t)nout * K + kin] : 0.f;
    }
}

// Half-precision packings (rollout_f16.h: the weights are the A operand of v_mfma_f32_16x16x32_f16, 8 halfs
// per lane).  Element e = ((blk * 64 + lane) * 8 + i8):
//   wph[j]  (forward)   blk = (4q + jt) * kch + c, kch = kp32 / 32:  W[64q + 16(r>>2) + 4jt + (r&3)][32c + 8(lane>>4) + i8], r = lane & 15
//   wpth[j] (backward, j >= 1) same with roles swapped: rows = inputs of the layer (quads over dims[j]),
//           chunks over its outputs:  W[32c + 8(lane>>4) + i8][64q + 16(r>>2) + 4jt + (r&3)]
//   wpth[0] (backward, input adjoint) plain 16-row tiles over the 16-padded inputs:  W[32c + 8(lane>>4) + i8][16nt + r]
__device__ __forceinline__ void pack_element_h(const float* __restrict__ W, int N, int K, int Kp16, int Kp32, int layer,
                                               _Float16* __restrict__ wph, _Float16* __restrict__ wpth, int e) {
    const int i8 = e & 7, lane = (e >> 3) & 63, blk = e >> 9, r = lane & 15, kg = lane >> 4;
    if (e < N * Kp32) {   // forward
        const int kch = Kp32 >> 5, c = blk % kch, t = blk / kch, jt = t & 3, q = t >> 2;
        const int n = 64 * q + 16 * (r >> 2) + 4 * jt + (r & 3), k = 32 * c + 8 * kg + i8;
        wph[e] = (_Float16)((k < K) ? W[(size_t)n * K + k] : 0.f);
    }
    const int kchN = N >> 5;   // outputs are a multiple of 64
    if (layer >= 1) {
        if (e < N * K) {      // K = width of the previous hidden layer, a multiple of 64
            const int c = blk % kchN, t = blk / kchN, jt = t & 3, q = t >> 2;
            const int kin = 64 * q + 16 * (r >> 2) + 4 * jt + (r & 3), nout = 32 * c + 8 * kg + i8;
            wpth[e] = (_Float16)W[(size_t)nout * K + kin];
        }
    } else if (e < N * Kp16) {
        const int c = blk % kchN, nt = blk / kchN;
        const int kin = 16 * nt + r, nout = 32 * c + 8 * kg + i8;
        wpth[e] = (_Float16)((kin < K) ? W[(size_t)nout * K + kin] : 0.f);
    }
}

// Plane-split operands (common.h SplitDev).  One block packs one n-tile: 16 columns x 32 kc contraction slots.
//   forward,  layer j: column = OUTPUT feature 16 nt + col, slot s <-> input feature (j == 0 ? s : split_perm(s))
//   backward, layer j: column = INPUT feature 16 nt + col,  slot s <-> output feature split_perm(s)
// element ((c * 64 + lane) * 8 + i) of the tile = (column lane & 15, slot 32 c + 8 (lane >> 4) + i): the B operand of
// v_mfma_f32_16x16x32_f16 for chunk c.  w1 / rf: the hi / lo half planes of w s_w (below); inv[nt] = 1 / s_w.
__device__ __forceinline__ void pack_split_tile(const float* __restrict__ W, int N, int K, bool transposed, bool perm_slots,
                                                int kc, int nt, unsigned short* __restrict__ w1, _Float16* __restrict__ rf,
                                                float* __restrict__ inv) {
    __shared__ float red[256];
    const int tid = threadIdx.x, total = 16 * 32 * kc;
    auto wval = [&](int e) -> float {
        const int i = e & 7, lane = (e >> 3) & 63, c = e >> 9;
        const int col = 16 * nt + (lane & 15), slot = 32 * c + 8 * (lane >> 4) + i;
        const int f = perm_slots ? split_perm(slot) : slot;
        if (!transposed) return (col < N && f < K) ? W[(size_t)col * K + f] : 0.f;   // W[out = col][in = f]
        return (f < N && col < K) ? W[(size_t)f * K + col] : 0.f;                     // W[out = f][in = col]
    };
    // two half planes of w s_w: wh = f16(w s_w) (round to nearest), wl = f16((w s_w - wh) 2^11); s_w = the power of two that brings the
    // tile's largest |w| into [2^13, 2^14) - fp32's exponent range for the weights, and small-weight tiles use the half's normal range.
    // The tile's <= 16 elements per thread are loaded ONCE, all loads in flight together (a load - use - load loop costs one L2 round
    // trip per element: this kernel sits on the critical path of every update, round 5: 11 -> 5 us).
    constexpr int PER = 16;   // kc <= 8: 16 * 32 * 8 / 256
    float v[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int e = tid + 256 * q;
        v[q] = e < total ? wval(e) : 0.f;
    }
    float mx = 0.f;
#pragma unroll
    for (int q = 0; q < PER; ++q) mx = fmaxf(mx, fabsf(v[q]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float s_w = 1.f;
    if (mx > 0.f && mx < 3.0e38f) {
        int ex;
        (void)frexpf(mx, &ex);   // mx = f * 2^ex, f in [0.5, 1)
        s_w = ldexpf(1.f, 14 - ex);
    }
    const size_t off = (size_t)nt * total;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int e = tid + 256 * q;
        if (e < total) {
            const float w = v[q] * s_w;   // (exact: a power of two)
            const _Float16 h = (_Float16)w;
            w1[off + e] = __builtin_bit_cast(unsigned short, h);
            rf[off + e] = (_Float16)((w - (float)h) * SPLIT_LO_SCALE);
        }
    }
    if (tid == 0) inv[nt] = 1.f / s_w;
}
// The fp32 MFMA-fragment packings (wp / wpt) of the POLICY are read by the exact-fp32 kernels only.  A veh3dofconti launch on the
// register-stationary plane-split kernels never reaches one - its sweep is the stationary plane-split sweep, and the calls that
// would divert a backward to the fp32 kernels after the forward has planned (terminal adjoints / gops_rollout_backward_adj,
// ActionRepeat, open loop: the EXT / GEN instantiations) do not exist for the vehicle models - so the 384 blocks of that packing
// (obs -> 256 -> 256) would be written for nobody.  Every other launch keeps it (an lq / idpendulum rollout may get an `_adj`
// backward, a value / MLP batch an `ext_delta` one, decided only at backward time).  The tail value net always keeps its packing
// (exact-fp32 tail evaluation).  Returns the first net to pack.
__host__ __device__ inline int fp32_pack_first_net(const RolloutParams& p) {
    return (!p.f16 && p.sp.on && p.env.kind == GOPS_ENV_VEH3DOFCONTI) ? 1 : 0;
}

__host__ __device__ inline int split_pack_blocks(const RolloutParams& p) {
    if (p.ss || p.ssb) {   // streamed-split forward: one block per n-tile of every hidden layer of the policy (and the tail value net)
        int nb = 0;
        for (int m = 0; m < (p.tail ? 2 : 1); ++m) {
            const MlpDev& d = m ? p.val : p.pol;
            for (int j = 0; j < d.nl - 1; ++j) {
                if (p.ss) nb += d.dims[j + 1] >> 4;
                if (p.ssb) nb += ((j == 0) ? d.kp[0] : d.dims[j]) >> 4;   // transposed planes of the sweep
            }
        }
        return nb;
    }
    if (!p.sp.on) return 0;
    return (p.pol.dims[1] >> 4) + (p.pol.dims[2] >> 4) + (p.pol.dims[1] >> 4) + (p.pol.kp[0] >> 4);
}

// Copies the by-value parameter block into device memory (stream ordered, no host staging): the
// rollout kernels then read it with uniform scalar loads instead of a per-lane scratch copy.
// F16 launches: every block also folds its slice of grad_v into max|g| (atomicMax on the bit pattern - for
// non-negative floats the unsigned order is the numeric order) in p.gscale[0], which the forward prologue
// zeroed.  The sweep and the reduce kernel derive the power-of-two scale from it (f16_grad_scale, common.h).
__global__ __launch_bounds__(256) void upload_params_kernel(const RolloutParams p, RolloutParams* dst) {
    if (blockIdx.x == 0) {
        const unsigned* src = reinterpret_cast<const unsigned*>(&p);
        unsigned* d = reinterpret_cast<unsigned*>(dst);
        for (unsigned i = threadIdx.x; i < sizeof(RolloutParams) / 4; i += blockDim.x) d[i] = src[i];
    }
    if (p.gscale != nullptr && p.grad_v != nullptr) {
        __shared__ float red[256];
        float mx = 0.f;
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < p.B; i += gridDim.x * blockDim.x) mx = fmaxf(mx, fabsf(p.grad_v[i]));
        red[threadIdx.x] = mx;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + w]);
            __syncthreads();
        }
        if (threadIdx.x == 0 && red[0] < 3.0e38f) atomicMax(reinterpret_cast<unsigned*>(p.gscale), __float_as_uint(red[0]));
    }
}

hipError_t launch_upload_params(const RolloutParams& p, RolloutParams* dst, hipStream_t s) {
    static_assert(sizeof(RolloutParams) % 4 == 0, "parameter block must be dword sized");
    int nb = (p.B + 4095) / 4096;
    nb = nb < 1 ? 1 : (nb > 128 ? 128 : nb);   // >= 16 elements per thread
    hipLaunchKernelGGL(upload_params_kernel, dim3(nb), dim3(256), 0, s, p, dst);
    return hipGetLastError();
}

// (reference trajectories of pyth_veh3dofconti, ref_point_ids: env_step.h)

// table[b][i] : i <= P copies info["ref_points"][b][i]; i = P + s (s >= 1) is the point the model
// appends at rollout step s-1: evaluated at (t0 + s*dt accumulated in fp32) + P*dt.
__device__ __forceinline__ void ref_table_element(int B, int P, int H, const float* __restrict__ ref_points,
                                                  const float* __restrict__ path_num,
                                                  const float* __restrict__ u_num,
                                                  const float* __restrict__ ref_time, float pdt,
                                                  float* __restrict__ table, int idx, bool yphi_only,
                                                  const float* __restrict__ refc, const float* __restrict__ appended) {
    const int TL = P + 1 + H;
    if (idx >= B * TL) return;
    const int b = idx / TL, i = idx - b * TL;
    f32x4 v;
    if (i <= P) {
        if (yphi_only) {   // pyth_veh2dofconti: info["ref_points"] [B, P+1, 2] = (y, phi)
            const float* rp = ref_points + ((size_t)b * (P + 1) + i) * 2;
            v = f32x4{0.f, rp[0], rp[1], 0.f};
        } else {
            v = reinterpret_cast<const f32x4*>(ref_points)[(size_t)b * (P + 1) + i];
        }
    } else if (appended != nullptr) {   // bit-parity mode: the caller's points [B][H][4]
        v = reinterpret_cast<const f32x4*>(appended)[(size_t)b * H + (i - P - 1)];
    } else {
        // the 24 path constants, the three per-trajectory scalars: loaded together up front (read where they are used, inside the
        // branches of ref_xy, each costs a memory round trip of its own)
        float c[24];
#pragma unroll
        for (int q = 0; q < 24; ++q) c[q] = refc[q];
        const float pn = path_num[b], un = u_num[b];
        float t = ref_time[b];
        for (int s = 0; s < i - P; ++s) t = RADD(t, 0.1f);
        v = ref_point_ids(c, RADD(t, pdt), pn, un);
    }
    reinterpret_cast<f32x4*>(table)[idx] = v;
}

// ---------------------------------------------------------------------------------------------
// Forward prologue, ONE launch: block 0 uploads the parameter block, the next blocks pack the
// hidden-layer weights of the policy (and of the tail value net), the rest fill the reference table.
// ---------------------------------------------------------------------------------------------
__host__ __device__ inline int pack_blocks(const MlpDev& d) {
    int nb = 0;
    for (int j = 0; j < d.nl - 1; ++j) nb += (d.dims[j + 1] * d.kp[j] + 255) / 256;
    return nb;
}
__host__ __device__ inline int pack_blocks_h(const MlpDev& d, int j) {   // covers wph[j] (N x kp32) and wpth[j]
    return (d.dims[j + 1] * d.kp32[j] + 255) / 256;
}

__global__ __launch_bounds__(256) void prologue_kernel(const RolloutParams p, RolloutParams* dst, int P, float pdt) {
    int b = blockIdx.x;
    if (b == 0) {
        const unsigned* src = reinterpret_cast<const unsigned*>(&p);
        unsigned* d = reinterpret_cast<unsigned*>(dst);
        constexpr unsigned NW = sizeof(RolloutParams) / 4, PER = (NW + 255) / 256;
        unsigned w[PER];   // all loads first, then the stores (a load - store loop: one round trip per 1 KB)
#pragma unroll
        for (unsigned q = 0; q < PER; ++q) {
            const unsigned i = threadIdx.x + 256 * q;
            w[q] = i < NW ? src[i] : 0u;
        }
#pragma unroll
        for (unsigned q = 0; q < PER; ++q) {
            const unsigned i = threadIdx.x + 256 * q;
            if (i < NW) d[i] = w[q];
        }
        if (p.gscale != nullptr && threadIdx.x == 0) p.gscale[0] = p.gscale[1] = p.gscale[3] = 0.f;   // max|grad_v| / max|delta_y| of the coming backward; [3]: the overflow mark of forward + sweep
        return;
    }
    b -= 1;
    for (int m = fp32_pack_first_net(p); m < (p.tail ? 2 : 1); ++m) {
        const MlpDev& d = m ? p.val : p.pol;
        for (int j = 0; j < d.nl - 1; ++j) {
            if (p.f16) {
                const int nb = pack_blocks_h(d, j);
                if (b < nb) {
                    pack_element_h(d.w[j], d.dims[j + 1], d.dims[j], d.kp[j], d.kp32[j], j,
                                   const_cast<_Float16*>(reinterpret_cast<const _Float16*>(d.wph[j])),
                                   const_cast<_Float16*>(reinterpret_cast<const _Float16*>(d.wpth[j])), b * 256 + threadIdx.x);
                    return;
                }
                b -= nb;
                continue;
            }
            const int nb = (d.dims[j + 1] * d.kp[j] + 255) / 256;
            if (b < nb) {
                pack_element(d.w[j], d.dims[j + 1], d.dims[j], d.kp[j],
                             const_cast<float*>(reinterpret_cast<const float*>(d.wp[j])),
                             const_cast<float*>(reinterpret_cast<const float*>(d.wpt[j])), b * 256 + threadIdx.x);
                return;
            }
            b -= nb;
        }
    }
    if (p.ss || p.ssb) {   // plane-split operands of the streamed-split forward kernels (p.ss) and of the streamed-split sweep (p.ssb)
        auto us = [](const bf16x8* q) { return const_cast<unsigned short*>(reinterpret_cast<const unsigned short*>(q)); };
        auto hf = [](const f16x8* q) { return const_cast<_Float16*>(reinterpret_cast<const _Float16*>(q)); };
        for (int m = 0; m < (p.tail ? 2 : 1); ++m) {
            const MlpDev& d = m ? p.val : p.pol;
            const SplitNetDev& sn = m ? p.ssv : p.ssp;
            for (int j = 0; j < d.nl - 1; ++j) {
                const int nt = p.ss ? d.dims[j + 1] >> 4 : 0;
                if (b < nt) {   // layer 0: natural input order; deeper layers read the plane image of the previous activation
                    pack_split_tile(d.w[j], d.dims[j + 1], d.dims[j], false, j > 0, sn.kc[j], b, us(sn.w1[j]), hf(sn.r[j]), const_cast<float*>(sn.inv[j]));
                    return;
                }
                b -= nt;
                if (p.ssb) {   // sweep: delta_{j+1} -> delta_j (j = 0: g_x) through W_j, tiles over its inputs, slots over its outputs
                    const SplitNetDev& st = m ? p.ssvt : p.sspt;
                    const int ntt = ((j == 0) ? d.kp[0] : d.dims[j]) >> 4;
                    if (b < ntt) {
                        pack_split_tile(d.w[j], d.dims[j + 1], d.dims[j], true, true, st.kc[j], b, us(st.w1[j]), hf(st.r[j]), const_cast<float*>(st.inv[j]));
                        return;
                    }
                    b -= ntt;
                }
            }
        }
    }
    if (p.sp.on) {   // plane-split operands of the stationary kernels: one block per n-tile
        const MlpDev& d = p.pol;
        const int n1 = d.dims[1] >> 4, n2 = d.dims[2] >> 4, k0 = d.kp[0] >> 4;
        auto us = [](const bf16x8* q) { return const_cast<unsigned short*>(reinterpret_cast<const unsigned short*>(q)); };
        auto hf = [](const f16x8* q) { return const_cast<_Float16*>(reinterpret_cast<const _Float16*>(q)); };
        if (b < n1) {            // forward layer 0: natural input order
            pack_split_tile(d.w[0], d.dims[1], d.dims[0], false, false, p.sp.kc[0], b, us(p.sp.w1[0]), hf(p.sp.r[0]), const_cast<float*>(p.sp.inv[0]));
            return;
        }
        b -= n1;
        if (b < n2) {            // forward layer 1: its input is the plane image of H_1
            pack_split_tile(d.w[1], d.dims[2], d.dims[1], false, true, p.sp.kc[1], b, us(p.sp.w1[1]), hf(p.sp.r[1]), const_cast<float*>(p.sp.inv[1]));
            return;
        }
        b -= n2;
        if (b < n1) {            // backward delta_2 -> delta_1 through W_1: tiles over its inputs, slots over its outputs
            pack_split_tile(d.w[1], d.dims[2], d.dims[1], true, true, d.dims[2] >> 5, b, us(p.sp.w1t[1]), hf(p.sp.rt[1]), const_cast<float*>(p.sp.invt[1]));
            return;
        }
        b -= n1;
        if (b < k0) {            // backward delta_1 -> g_x through W_0
            pack_split_tile(d.w[0], d.dims[1], d.dims[0], true, true, d.dims[1] >> 5, b, us(p.sp.w1t[0]), hf(p.sp.rt[0]), const_cast<float*>(p.sp.invt[0]));
            return;
        }
        b -= k0;
    }
    if (env_has_ref_table(p.env.kind)) {
        const int nrt = (p.B * (P + 1 + p.H) + 255) / 256;
        if (b < nrt) {
            ref_table_element(p.B, P, p.H, p.in.ref_points, p.in.path_num, p.in.u_num, p.in.ref_time, pdt,
                              const_cast<float*>(p.ref_table), b * 256 + threadIdx.x, p.env.kind == GOPS_ENV_VEH2DOF, p.env.ref_c,
                              p.in.ref_appended);
            return;
        }
        b -= nrt;
    }
    if (p.env.kind == GOPS_ENV_VEH3DOF_SURR) {
        // surrounding vehicles move independently of the policy: their (x, y, phi, u) after t = 0 .. H steps, one
        // thread per (trajectory, vehicle)
        const int ns = p.env.n_surr, idx = b * 256 + threadIdx.x;
        if (idx < p.B * ns) {
            const int bb = idx / ns, i = idx - bb * ns;
            const float* s5 = p.in.surr_state + ((size_t)bb * ns + i) * 5;
            f32x4 cur = {s5[0], s5[1], s5[2], s5[3]};
            const float delta = s5[4];
            f32x4* tab = const_cast<f32x4*>(p.surr_table) + (size_t)bb * (p.H + 1) * ns + i;
            for (int t = 0; t <= p.H; ++t) {
                tab[(size_t)t * ns] = cur;
                cur = surr_next(cur, delta);
            }
        }
    }
}

hipError_t launch_prologue(const RolloutParams& p, RolloutParams* dst, int P, float pdt, hipStream_t s) {
    int nb = 1;
    for (int m = fp32_pack_first_net(p); m < (p.tail ? 2 : 1); ++m) {
        const MlpDev& d = m ? p.val : p.pol;
        if (!p.f16) { nb += pack_blocks(d); continue; }
        for (int j = 0; j < d.nl - 1; ++j) nb += pack_blocks_h(d, j);
    }
    nb += split_pack_blocks(p);
    if (env_has_ref_table(p.env.kind)) nb += (p.B * (P + 1 + p.H) + 255) / 256;
    if (p.env.kind == GOPS_ENV_VEH3DOF_SURR) nb += (p.B * p.env.n_surr + 255) / 256;
    hipLaunchKernelGGL(prologue_kernel, dim3(nb), dim3(256), 0, s, p, dst, P, pdt);
    return hipGetLastError();
}
