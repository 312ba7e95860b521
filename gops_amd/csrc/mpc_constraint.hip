// Path constraints of the batched shooting MPC by an augmented Lagrangian (gops_mpc_al_eval of include/gops_hip.h): per row the
// objective the device L-BFGS of mpc_lbfgs.hip minimises between two multiplier updates,
//
//     f_al = f + (1 / (2 rho)) sum_{t,k} (max(0, lambda_tk + rho c_tk)^2 - lambda_tk^2),
//
// its seed d f_al / d c_tk = max(0, lambda_tk + rho c_tk) in the layout GopsRolloutIn.grad_constraint_step takes, and the row's
// largest violation.  The outer step (gops_mpc_al_update) and the hand-over (gops_mpc_al_advance) write the solver block and sit in
// mpc_lbfgs.hip.
//
// Work assignment: ONE wave per row whatever H, n_c and batch are, four rows per workgroup.  Term j = t n_c + k of row r reads
// c[(t B + r) n_c + k] and lambda[r J + j], J = H n_c; lane l adds the terms l, l + 64, .. in index order in double, then the xor
// butterfly (32, .., 1) of block_reduce.h's block_fold combines the 64 lanes - a fixed order that sees neither the batch nor the row
// index, so a row's bits depend on neither.  No LDS, no atomics; every stored float is formed in double and rounded once.
#include "common.h"

// No fused multiply-adds: lambda + rho c is a rounded product and a rounded sum in double, so that a restatement in plain IEEE
// double arithmetic reproduces every stored float.
#pragma clang fp contract(off)

namespace {

constexpr int AL_THREADS = 256;

__global__ __launch_bounds__(AL_THREADS) void mpc_al_eval_kernel(int B, int H, int nc, const float* __restrict__ c, const float* __restrict__ lambda,
                                                                 const float* __restrict__ rho, const float* __restrict__ f,
                                                                 float* __restrict__ f_al, float* __restrict__ seed, float* __restrict__ viol) {
    const size_t r = (size_t)blockIdx.x * (AL_THREADS / 64) + threadIdx.x / 64;
    if (r >= (size_t)B) return;
    const int lane = threadIdx.x & 63, J = H * nc;
    const double rh = (double)rho[r];
    double sum = 0.0, worst = 0.0, bad = 0.0;
    for (int j = lane; j < J; j += 64) {
        const int t = j / nc, k = j - t * nc;
        const size_t at = ((size_t)t * B + r) * nc + k;
        const double cv = (double)c[at], lam = (double)lambda[r * J + j];
        const double u = lam + rh * cv;
        const double p = u != u ? u : fmax(0.0, u);   // (fmax drops a NaN; the seed of a NaN constraint is NaN)
        sum += p * p - lam * lam;
        seed[at] = (float)p;
        worst = fmax(worst, fmax(0.0, cv));
        if (!isfinite(cv)) bad = 1.0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sum += __shfl_xor(sum, o);
        worst = fmax(worst, __shfl_xor(worst, o));
        bad = fmax(bad, __shfl_xor(bad, o));
    }
    if (lane == 0) {
        f_al[r] = bad != 0.0 ? NAN : (float)((double)f[r] + sum / (2.0 * rh));
        viol[r] = (float)worst;
    }
}

}  // namespace

extern "C" {

int gops_mpc_al_eval(int32_t B, int32_t H, int32_t n_c, const float* c, const float* lambda, const float* rho, const float* f, float* f_al,
                     float* seed, float* viol, void* stream) {
    if (!c || !lambda || !rho || !f || !f_al || !seed || !viol || B < 1 || H < 1 || H > GOPS_MPC_AL_MAX_H || n_c < 1 || n_c > GOPS_MAX_CONSTRAINT)
        return GOPS_ERR_BAD_ARG;
    const unsigned blocks = (unsigned)(((size_t)B + AL_THREADS / 64 - 1) / (AL_THREADS / 64));
    hipLaunchKernelGGL(mpc_al_eval_kernel, dim3(blocks), dim3(AL_THREADS), 0, static_cast<hipStream_t>(stream), (int)B, (int)H, (int)n_c, c, lambda,
                       rho, f, f_al, seed, viol);
    return (int)hipGetLastError();
}

}  // extern "C"
