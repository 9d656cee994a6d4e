// phgpu.hip -- MI355X (gfx950) kernels + C-ABI for the batched PH hot path.
//
// Design: every local scenario is one LP/QP that shares the CSR
// pattern of the rank; per-scenario arrays are stored scenario-fastest ([k][S]) so
// that the 64 lanes of a wavefront process 64 scenarios and every load/store of a
// pattern position is one coalesced 512-byte access, while the pattern itself
// (row_ptr, col_idx, col_ptr, row_idx, perm) is wave-uniform and goes through the
// scalar cache.  One lane runs its scenario's whole restarted-Halpern PDHG solve in a
// single launch (no grid-wide synchronisation: scenarios are independent), with its
// own primal weight, restart state and KKT termination test.
//
// Reference behaviour replaced (mpi-sppy, /root/reference):
//   SPOpt.solve_loop / solve_one        spopt.py:226-307 / 85-223
//   PH objective terms                  phbase.py:617-699
//   _Compute_Xbar / Update_W / conv     phbase.py:27-107, 293-343
//   Ebound / Eobjective / E1 / feas     spopt.py:310-439
//   NormRhoUpdater residuals and rule   extensions/norm_rho_updater.py:55-143
//   converger sums                      convergers/primal_dual_converger.py:58-110,
//                                       convergers/norm_rho_converger.py:23-29
//   gradient cost, W_diff, cost-proportional rho
//                                       utils/gradient.py:65-81, utils/wtracker.py:134-157,
//                                       utils/find_rho.py:78-203,
//                                       extensions/gradient_extension.py:65-95
//   APH's projective step, dispatch and partial solve loop
//                                       opt/aph.py:151-195, 254-310, 394-408, 453-496, 602-668
//   the L-shaped method's cuts and master LP
//                                       opt/lshaped.py:477-560, 600-666
//   the extensive form's interior point  opt/ef.py:60-140, opt/sc.py:60-105 (ph_ef.inc)
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdarg.h>
#include <string.h>
#include <new>
#include <stdlib.h>
#include <algorithm>
#include <chrono>
#include <vector>
#include <mutex>
#include <map>
#include <string>
#include <cctype>

#include "phgpu.h"

#define WAVE 64
#define BLOCK 64
#define ORDER_BINS 256  // counting-sort bins of the longest-first work queue (solve_reg.inc)
#define XL_T 1024        // threads per block of k_ph_update_local at most
#define XL_NN_MAX 16     // nonants per scenario at most for the folded x̄ paths (k_ph_update_local, IPM epilogues)
#define XL_PF 4          // k_ph_update_local: nonants whose operands are loaded ahead of the x̄ sums
#define XP_CHUNK_MIN 16  // smallest x̄-partial chunk of the IPM epilogues (256 / 16 lanes)

// ------------------------------------------------------------------ errors
static thread_local char g_err[512] = {0};

static int set_err(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIPCHK(call)                                                                 \
    do {                                                                             \
        hipError_t e_ = (call);                                                      \
        if (e_ != hipSuccess)                                                        \
            return set_err(-2, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                           __FILE__, __LINE__);                                      \
    } while (0)

#include "ph_state.h"

#define IX(k) ((size_t)(k) * (size_t)S + (size_t)s)

// ------------------------------------------------------------------ device helpers
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, WAVE);
    return v;
}

__device__ __forceinline__ double clampd(double v, double lo, double hi) {
    return fmin(fmax(v, lo), hi);
}

// y-part of the PDHG dual step for a ranged row rl <= a'x <= ru:
// maximise -y*ax + (rl y+ - ru y-) - (y - yk)^2/(2 sig)
__device__ __forceinline__ double dual_prox(double v, double sig, double rlh, double ruh) {
    double a = v + sig * rlh;
    double b = v + sig * ruh;
    return a > 0.0 ? a : (b < 0.0 ? b : 0.0);
}

// contribution of row i to the Lagrangian dual objective: min_{s in [rl,ru]} y s,
// projected (an infinite side with the wrong-sign multiplier contributes 0)
__device__ __forceinline__ double row_dual_term(double y, double rl, double ru) {
    if (y > 0.0) return isfinite(rl) ? rl * y : 0.0;
    if (y < 0.0) return isfinite(ru) ? ru * y : 0.0;
    return 0.0;
}

// min over x in [lb,ub] of r x + q/2 x^2 (projected for infinite sides when q == 0)
__device__ __forceinline__ double col_dual_term(double r, double qq, double lb, double ub) {
    if (qq > 0.0) {
        double xm = clampd(-r / qq, lb, ub);
        return r * xm + 0.5 * qq * xm * xm;
    }
    if (r > 0.0) return isfinite(lb) ? r * lb : 0.0;
    if (r < 0.0) return isfinite(ub) ? r * ub : 0.0;
    return 0.0;
}

// ---------------------------------------------------------- infeasibility certificates
// PDLP-style tests on the fixed-point residual d = T(z) - z, which for an infeasible or
// unbounded problem converges to the minimal displacement of the PDHG operator (its dual
// part is a Farkas ray, its primal part a ray of descent).  All quantities are in the
// original space.  The reference marks such a scenario infeasible (spopt.py:175-194) and
// Iter0 stops on it (phbase.py:818-823).
//
// Primal infeasibility: dual ray d (rows), ray reduced cost r = -(A^T d) (columns).  The
// ray objective sum_i min_{s in [rl,ru]} s d_i + sum_j min_{x in [lb,ub]} r_j x_j must be
// > 0 while every component that points at an infinite side (where the min is -inf) is
// ~0: certificate if sqrt(viol2) <= eps * obj.
__device__ __forceinline__ void ray_row_terms(double d, double rl, double ru, double& obj, double& viol2) {
    if (d > 0.0) {
        if (isfinite(rl)) obj += rl * d;
        else viol2 += d * d;
    } else if (d < 0.0) {
        if (isfinite(ru)) obj += ru * d;
        else viol2 += d * d;
    }
}
__device__ __forceinline__ void ray_col_terms(double r, double lb, double ub, double& obj, double& viol2) {
    if (r > 0.0) {
        if (isfinite(lb)) obj += lb * r;
        else viol2 += r * r;
    } else if (r < 0.0) {
        if (isfinite(ub)) obj += ub * r;
        else viol2 += r * r;
    }
}
// Dual infeasibility (unbounded primal): primal ray dx with c'dx < 0, Q dx = 0, A dx in
// the recession cone of [rl, ru] and dx in that of [lb, ub]; squared distance to the cone.
__device__ __forceinline__ double recession_viol2(double a, double lo, double hi) {
    double v = 0.0;
    if (isfinite(lo) && a < 0.0) v += a * a;
    if (isfinite(hi) && a > 0.0) v += a * a;
    return v;
}
__device__ __forceinline__ bool is_certificate(double obj, double viol2, double eps) {
    return obj > 0.0 && viol2 <= (eps * obj) * (eps * obj);
}

// ------------------------------------------------------------------ setup kernel
// Per scenario: copy A, Ruiz (iters) + Pock-Chambolle(alpha=1) scaling, scaled
// bounds, CSC copy of the scaled values and ||A_scaled||_2 by power iteration.
__global__ void __launch_bounds__(BLOCK) k_setup(pdhg_view st, int ruiz_iters, int power_iters) {
    const int64_t S = st.S;
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const int n = st.n, m = st.m, nnz = st.nnz;
    double* Ah = st.Ah_csr;
    for (int k = 0; k < nnz; ++k) Ah[IX(k)] = st.A[IX(k)];
    for (int i = 0; i < m; ++i) st.Dr[IX(i)] = 1.0;
    for (int j = 0; j < n; ++j) st.Dc[IX(j)] = 1.0;
    // temporaries: row factors in yt, column factors in xt
    for (int pass = 0; pass <= ruiz_iters; ++pass) {
        const bool pc = (pass == ruiz_iters);  // last pass: Pock-Chambolle alpha = 1
        for (int i = 0; i < m; ++i) {
            double a = 0.0;
            for (int k = st.row_ptr[i]; k < st.row_ptr[i + 1]; ++k) {
                double v = fabs(Ah[IX(k)]);
                a = pc ? a + v : fmax(a, v);
            }
            st.yt[IX(i)] = a > 0.0 ? 1.0 / sqrt(a) : 1.0;
        }
        for (int j = 0; j < n; ++j) {
            double a = 0.0;
            for (int kc = st.col_ptr[j]; kc < st.col_ptr[j + 1]; ++kc) {
                double v = fabs(Ah[IX(st.perm[kc])]);
                a = pc ? a + v : fmax(a, v);
            }
            st.xt[IX(j)] = a > 0.0 ? 1.0 / sqrt(a) : 1.0;
        }
        for (int i = 0; i < m; ++i) {
            const double ri = st.yt[IX(i)];
            st.Dr[IX(i)] *= ri;
            for (int k = st.row_ptr[i]; k < st.row_ptr[i + 1]; ++k)
                Ah[IX(k)] *= ri * st.xt[IX(st.col_idx[k])];
        }
        for (int j = 0; j < n; ++j) st.Dc[IX(j)] *= st.xt[IX(j)];
    }
    for (int kc = 0; kc < nnz; ++kc) st.Ah_csc[IX(kc)] = Ah[IX(st.perm[kc])];
    for (int j = 0; j < n; ++j) {
        const double d = st.Dc[IX(j)];
        st.lbh[IX(j)] = st.lb[IX(j)] / d;
        st.ubh[IX(j)] = st.ub[IX(j)] / d;
        st.x[IX(j)] = 0.0;
    }
    for (int i = 0; i < m; ++i) {
        const double d = st.Dr[IX(i)];
        st.rlh[IX(i)] = st.rl[IX(i)] * d;
        st.ruh[IX(i)] = st.ru[IX(i)] * d;
        st.y[IX(i)] = 0.0;
    }
    // power iteration on A^T A (v in xe, A v in yt, A^T A v in xt)
    for (int j = 0; j < n; ++j) st.xe[IX(j)] = 1.0 + 0.5 * sin(1.7 * j);
    double lam = 0.0;
    for (int it = 0; it < power_iters; ++it) {
        for (int i = 0; i < m; ++i) {
            double a = 0.0;
            for (int k = st.row_ptr[i]; k < st.row_ptr[i + 1]; ++k)
                a += Ah[IX(k)] * st.xe[IX(st.col_idx[k])];
            st.yt[IX(i)] = a;
        }
        double nv = 0.0;
        for (int j = 0; j < n; ++j) {
            double a = 0.0;
            for (int kc = st.col_ptr[j]; kc < st.col_ptr[j + 1]; ++kc)
                a += st.Ah_csc[IX(kc)] * st.yt[IX(st.row_idx[kc])];
            st.xt[IX(j)] = a;
            nv += a * a;
        }
        nv = sqrt(nv);
        lam = nv;  // ||A^T A v|| with ||v|| = 1 (after the first pass)
        const double inv = nv > 0.0 ? 1.0 / nv : 0.0;
        for (int j = 0; j < n; ++j) st.xe[IX(j)] = st.xt[IX(j)] * inv;
    }
    // power iteration under-estimates ||A||_2 (slowly when the top singular values are
    // close); 1% margin keeps tau * sigma * ||A||^2 < 1 (a violated step condition makes
    // the reflected Halpern iteration diverge)
    st.normA[s] = lam > 0.0 ? 1.01 * sqrt(lam) : 1.0;
    st.omega[s] = 1.0;
}

// ------------------------------------------------------------------ parallel setup
// k_setup's algorithm with (row | column | nonzero, scenario) pairs over threads, the
// scenario fastest (coalesced [k][S] accesses): for patterns with many nonzeros, where
// one lane per scenario walking 2 nnz x 200 power steps serially is the bottleneck
// (farmer cm=64: 439 ms).  Same operations in the same order per scenario, so the
// scaled problem and ||A|| are bit-identical to k_setup's.
#define SU_T 256
__global__ void __launch_bounds__(SU_T) k_su_init(ph_data st) {
    const int64_t S = st.S;
    const int64_t t = (int64_t)blockIdx.x * SU_T + threadIdx.x;
    const int64_t K = (int64_t)(st.nnz > st.n ? (st.nnz > st.m ? st.nnz : st.m) : (st.n > st.m ? st.n : st.m));
    if (t >= K * S) return;
    const int64_t k = t / S, s = t - k * S;
    if (k < st.nnz) st.Ah_csr[IX(k)] = st.A[IX(k)];
    if (k < st.m) st.Dr[IX(k)] = 1.0;
    if (k < st.n) st.Dc[IX(k)] = 1.0;
}

// row factors into yt (pc: Pock-Chambolle sum, else Ruiz max)
__global__ void __launch_bounds__(SU_T) k_su_rowfac(pdhg_view st, int pc) {
    const int64_t S = st.S;
    const int64_t t = (int64_t)blockIdx.x * SU_T + threadIdx.x;
    if (t >= (int64_t)st.m * S) return;
    const int i = (int)(t / S);
    const int64_t s = t - (int64_t)i * S;
    double a = 0.0;
    for (int k = st.row_ptr[i]; k < st.row_ptr[i + 1]; ++k) {
        const double v = fabs(st.Ah_csr[IX(k)]);
        a = pc ? a + v : fmax(a, v);
    }
    st.yt[IX(i)] = a > 0.0 ? 1.0 / sqrt(a) : 1.0;
}

__global__ void __launch_bounds__(SU_T) k_su_colfac(pdhg_view st, int pc) {
    const int64_t S = st.S;
    const int64_t t = (int64_t)blockIdx.x * SU_T + threadIdx.x;
    if (t >= (int64_t)st.n * S) return;
    const int j = (int)(t / S);
    const int64_t s = t - (int64_t)j * S;
    double a = 0.0;
    for (int kc = st.col_ptr[j]; kc < st.col_ptr[j + 1]; ++kc) {
        const double v = fabs(st.Ah_csr[IX(st.perm[kc])]);
        a = pc ? a + v : fmax(a, v);
    }
    st.xt[IX(j)] = a > 0.0 ? 1.0 / sqrt(a) : 1.0;
}

__global__ void __launch_bounds__(SU_T) k_su_apply(pdhg_view st) {
    const int64_t S = st.S;
    const int64_t t = (int64_t)blockIdx.x * SU_T + threadIdx.x;
    const int64_t K = (int64_t)(st.nnz > st.n ? (st.nnz > st.m ? st.nnz : st.m) : (st.n > st.m ? st.n : st.m));
    if (t >= K * S) return;
    const int64_t k = t / S, s = t - k * S;
    if (k < st.nnz) st.Ah_csr[IX(k)] *= st.yt[IX(st.row_of[k])] * st.xt[IX(st.col_idx[k])];
    if (k < st.m) st.Dr[IX(k)] *= st.yt[IX(k)];
    if (k < st.n) st.Dc[IX(k)] *= st.xt[IX(k)];
}

// CSC copy, scaled bounds, zero iterates, power-iteration start vector
__global__ void __launch_bounds__(SU_T) k_su_finish(pdhg_view st) {
    const int64_t S = st.S;
    const int64_t t = (int64_t)blockIdx.x * SU_T + threadIdx.x;
    const int64_t K = (int64_t)(st.nnz > st.n ? (st.nnz > st.m ? st.nnz : st.m) : (st.n > st.m ? st.n : st.m));
    if (t >= K * S) return;
    const int64_t k = t / S, s = t - k * S;
    if (k < st.nnz) st.Ah_csc[IX(k)] = st.Ah_csr[IX(st.perm[k])];
    if (k < st.n) {
        const double d = st.Dc[IX(k)];
        st.lbh[IX(k)] = st.lb[IX(k)] / d;
        st.ubh[IX(k)] = st.ub[IX(k)] / d;
        st.x[IX(k)] = 0.0;
        st.xe[IX(k)] = 1.0 + 0.5 * sin(1.7 * (int)k);
    }
    if (k < st.m) {
        const double d = st.Dr[IX(k)];
        st.rlh[IX(k)] = st.rl[IX(k)] * d;
        st.ruh[IX(k)] = st.ru[IX(k)] * d;
        st.y[IX(k)] = 0.0;
    }
}

__global__ void __launch_bounds__(SU_T) k_su_rowmv(pdhg_view st) {
    const int64_t S = st.S;
    const int64_t t = (int64_t)blockIdx.x * SU_T + threadIdx.x;
    if (t >= (int64_t)st.m * S) return;
    const int i = (int)(t / S);
    const int64_t s = t - (int64_t)i * S;
    double a = 0.0;
    for (int k = st.row_ptr[i]; k < st.row_ptr[i + 1]; ++k) a += st.Ah_csr[IX(k)] * st.xe[IX(st.col_idx[k])];
    st.yt[IX(i)] = a;
}

__global__ void __launch_bounds__(SU_T) k_su_colmv(pdhg_view st) {
    const int64_t S = st.S;
    const int64_t t = (int64_t)blockIdx.x * SU_T + threadIdx.x;
    if (t >= (int64_t)st.n * S) return;
    const int j = (int)(t / S);
    const int64_t s = t - (int64_t)j * S;
    double a = 0.0;
    for (int kc = st.col_ptr[j]; kc < st.col_ptr[j + 1]; ++kc) a += st.Ah_csc[IX(kc)] * st.yt[IX(st.row_idx[kc])];
    st.xt[IX(j)] = a;
}

// per scenario: lam = ||A^T A v||, v = A^T A v / lam (normA holds lam until the end);
// a block holds 32 scenarios x 8 column chunks (chunk c: columns c, c+8, ...), partial
// sums of squares added in chunk order
#define SU_CH 8
__global__ void __launch_bounds__(SU_T) k_su_norm(pdhg_view st) {
    __shared__ double part[SU_CH][SU_T / SU_CH];
    const int64_t S = st.S;
    const int c = threadIdx.x / (SU_T / SU_CH), l = threadIdx.x % (SU_T / SU_CH);
    const int64_t s = (int64_t)blockIdx.x * (SU_T / SU_CH) + l;
    double a2 = 0.0;
    if (s < S)
        for (int j = c; j < st.n; j += SU_CH) {
            const double a = st.xt[IX(j)];
            a2 += a * a;
        }
    part[c][l] = a2;
    __syncthreads();
    double nv = 0.0;
    for (int k = 0; k < SU_CH; ++k) nv += part[k][l];
    nv = sqrt(nv);
    if (s >= S) return;
    if (c == 0) st.normA[s] = nv;
    const double inv = nv > 0.0 ? 1.0 / nv : 0.0;
    for (int j = c; j < st.n; j += SU_CH) st.xe[IX(j)] = st.xt[IX(j)] * inv;
}

__global__ void __launch_bounds__(SU_T) k_su_done(pdhg_view st) {
    const int64_t s = (int64_t)blockIdx.x * SU_T + threadIdx.x;
    if (s >= st.S) return;
    const double lam = st.normA[s];
    st.normA[s] = lam > 0.0 ? 1.01 * sqrt(lam) : 1.0;
    st.omega[s] = 1.0;
}

// setup of a non-shared handle: k_setup (lane per scenario) for small patterns, the
// parallel kernels above for patterns with more than SETUP_PAR_NNZ nonzeros
#define SETUP_PAR_NNZ 128
static hipError_t run_setup(phgpu_state* h, hipStream_t st) {
    if (h->nnz <= SETUP_PAR_NNZ) {
        hipLaunchKernelGGL(k_setup, dim3((unsigned)((h->S + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, *h, 10, 200);
        return hipGetLastError();
    }
    const int64_t S = h->S;
    const int64_t K = std::max<int64_t>(h->nnz, std::max(h->n, h->m));
    auto g = [&](int64_t cnt) { return dim3((unsigned)((cnt + SU_T - 1) / SU_T)); };
    hipLaunchKernelGGL(k_su_init, g(K * S), dim3(SU_T), 0, st, *h);
    for (int pass = 0; pass <= 10; ++pass) {
        const int pc = pass == 10;
        if (h->m) hipLaunchKernelGGL(k_su_rowfac, g((int64_t)h->m * S), dim3(SU_T), 0, st, *h, pc);
        hipLaunchKernelGGL(k_su_colfac, g((int64_t)h->n * S), dim3(SU_T), 0, st, *h, pc);
        hipLaunchKernelGGL(k_su_apply, g(K * S), dim3(SU_T), 0, st, *h);
    }
    hipLaunchKernelGGL(k_su_finish, g(K * S), dim3(SU_T), 0, st, *h);
    for (int it = 0; it < 200; ++it) {
        if (h->m) hipLaunchKernelGGL(k_su_rowmv, g((int64_t)h->m * S), dim3(SU_T), 0, st, *h);
        hipLaunchKernelGGL(k_su_colmv, g((int64_t)h->n * S), dim3(SU_T), 0, st, *h);
        hipLaunchKernelGGL(k_su_norm, dim3((unsigned)((S + SU_T / SU_CH - 1) / (SU_T / SU_CH))), dim3(SU_T), 0, st,
                           *h);
    }
    hipLaunchKernelGGL(k_su_done, g(S), dim3(SU_T), 0, st, *h);
    return hipGetLastError();
}

// ------------------------------------------------------------------ record transposes
// [K][S] (scenario-fastest, the C-ABI layout) <-> scenario-major records pk[s * stride +
// off + k], through a 32 x 33 LDS tile so both sides are full-line accesses.
#define TT 32
__global__ void __launch_bounds__(256) k_to_records(const double* __restrict__ in, int K, int64_t S,
                                                    double* __restrict__ pk, int64_t stride, int off) {
    __shared__ double tile[TT][TT + 1];
    const int64_t s0 = (int64_t)blockIdx.x * TT;
    const int k0 = blockIdx.y * TT;
    const int tx = threadIdx.x % TT, ty = threadIdx.x / TT;
    for (int r = ty; r < TT; r += 256 / TT) {
        const int k = k0 + r;
        const int64_t s = s0 + tx;
        tile[r][tx] = (k < K && s < S) ? in[(size_t)k * (size_t)S + (size_t)s] : 0.0;
    }
    __syncthreads();
    for (int r = ty; r < TT; r += 256 / TT) {
        const int64_t s = s0 + r;
        const int k = k0 + tx;
        if (s < S && k < K) pk[(size_t)s * (size_t)stride + off + k] = tile[tx][r];
    }
}

// the PH state of a solve into the records in one launch: W | rho | xbar are consecutive
// record fields of nn entries each (pk_W, pk_RHO, pk_XB); a null source is skipped
__device__ __forceinline__ void to_records_ph_tile(double (*tile)[TT + 1], int bx, int by, const double* __restrict__ W,
                                                   const double* __restrict__ rho, const double* __restrict__ xbar,
                                                   int nn, int64_t S, double* __restrict__ pk, int64_t stride,
                                                   int off) {
    const int64_t s0 = (int64_t)bx * TT;
    const int k0 = by * TT;
    const int K = 3 * nn;
    const int tx = threadIdx.x % TT, ty = threadIdx.x / TT;
    for (int r = ty; r < TT; r += 256 / TT) {
        const int k = k0 + r;
        const int64_t s = s0 + tx;
        const int part = k < nn ? 0 : (k < 2 * nn ? 1 : 2);
        const double* a = part == 0 ? W : (part == 1 ? rho : xbar);
        double v = 0.0;
        if (k < K && a && s < S) v = a[(size_t)(k - part * nn) * (size_t)S + (size_t)s];
        tile[r][tx] = v;
    }
    __syncthreads();
    for (int r = ty; r < TT; r += 256 / TT) {
        const int64_t s = s0 + r;
        const int k = k0 + tx;
        const int part = k < nn ? 0 : (k < 2 * nn ? 1 : 2);
        const bool have = part == 0 ? W != nullptr : (part == 1 ? rho != nullptr : xbar != nullptr);
        if (s < S && k < K && have) pk[(size_t)s * (size_t)stride + off + k] = tile[tx][r];
    }
}

__global__ void __launch_bounds__(256) k_to_records_ph(const double* __restrict__ W, const double* __restrict__ rho,
                                                       const double* __restrict__ xbar, int nn, int64_t S,
                                                       double* __restrict__ pk, int64_t stride, int off) {
    __shared__ double tile[TT][TT + 1];
    to_records_ph_tile(tile, blockIdx.x, blockIdx.y, W, rho, xbar, nn, S, pk, stride, off);
}

// out[k][s] = pk[s][off + k] * (moff >= 0 ? pk[s][moff + k] : 1)
__global__ void __launch_bounds__(256) k_from_records(const double* __restrict__ pk, int64_t stride, int off,
                                                      int moff, int K, int64_t S, double* __restrict__ out) {
    __shared__ double tile[TT][TT + 1];
    const int64_t s0 = (int64_t)blockIdx.x * TT;
    const int k0 = blockIdx.y * TT;
    const int tx = threadIdx.x % TT, ty = threadIdx.x / TT;
    for (int r = ty; r < TT; r += 256 / TT) {
        const int64_t s = s0 + r;
        const int k = k0 + tx;
        double v = 0.0;
        if (s < S && k < K) {
            const size_t b = (size_t)s * (size_t)stride;
            v = pk[b + off + k];
            if (moff >= 0) v *= pk[b + moff + k];
        }
        tile[tx][r] = v;
    }
    __syncthreads();
    for (int r = ty; r < TT; r += 256 / TT) {
        const int k = k0 + r;
        const int64_t s = s0 + tx;
        if (k < K && s < S) out[(size_t)k * (size_t)S + (size_t)s] = tile[r][tx];
    }
}

// ------------------------------------------------------------------ solve kernel
struct solve_params {
    double eps_rel, eps_abs, gamma, bsuff, bnec, bart, eta_frac, omega0, wmin, wmax, eps_inf;
    int max_iter, check_every, restart_every, warm, keep_omega, infeas_start;
};

__global__ void __launch_bounds__(BLOCK)
k_solve(pdhg_view st, solve_params P, double* __restrict__ xout, double* __restrict__ yout,
        double* __restrict__ obj, double* __restrict__ bound, int32_t* __restrict__ status,
        int32_t* __restrict__ iters, const int32_t* __restrict__ list = nullptr,
        const int32_t* __restrict__ list_n = nullptr, unsigned long long* __restrict__ stats = nullptr) {
    const int64_t S = st.S;
    int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    // list mode (the fallback of path 6's workgroup IPM): lane q solves list[q]
    if (list) {
        if (s >= *list_n) return;
        s = list[s];
    } else if (s >= S) {
        return;
    }
    const int n = st.n, m = st.m;
    const int32_t* __restrict__ row_ptr = st.row_ptr;
    const int32_t* __restrict__ col_idx = st.col_idx;
    const int32_t* __restrict__ col_ptr = st.col_ptr;
    const int32_t* __restrict__ row_idx = st.row_idx;
    const double* __restrict__ Ahr = st.Ah_csr;
    const double* __restrict__ Ahc = st.Ah_csc;
    // the iterate lives in the write slot (the read slot for an ordinary solve); the
    // warm start is read from st.x / st.y
    double* __restrict__ x = st.xw;
    double* __restrict__ x0 = st.x0;
    double* __restrict__ xe = st.xe;
    double* __restrict__ xt = st.xt;
    double* __restrict__ aty = st.aty;
    double* __restrict__ aty0 = st.aty0;
    double* __restrict__ y = st.yw;
    double* __restrict__ y0 = st.y0;
    double* __restrict__ yt = st.yt;
    const double* __restrict__ ch = st.ch;
    const double* __restrict__ qh = st.qh;

    // ---- effective objective of this solve (phbase.py:617-699), scaled
    double cnorm2 = 0.0, const_term = st.objc ? st.objc[s] : 0.0;
    for (int j = 0; j < n; ++j) {
        double cj = st.c[IX(j)];
        double qj = st.q ? st.q[IX(j)] : 0.0;
        const int k = st.nonant_slot[j];
        if (k >= 0) {
            if (st.W_on) cj += st.W[IX(k)];
            if (st.prox_on) {
                const double r = st.rho[IX(k)], xb = st.xbar[IX(k)];
                cj -= r * xb;
                qj += r;
                const_term += 0.5 * r * xb * xb;
            }
        }
        const double d = st.Dc[IX(j)];
        st.ch[IX(j)] = d * cj;
        st.qh[IX(j)] = d * d * qj;
        cnorm2 += cj * cj;
    }
    double bnorm2 = 0.0;
    for (int i = 0; i < m; ++i) {
        const double a = st.rl[IX(i)], b = st.ru[IX(i)];
        if (isfinite(a)) bnorm2 += a * a;
        if (isfinite(b) && b != a) bnorm2 += b * b;
    }
    const double cnorm = sqrt(cnorm2), bnorm = sqrt(bnorm2);

    // ---- start point
    for (int j = 0; j < n; ++j) {
        double v = P.warm ? st.x[IX(j)] : 0.0;
        v = clampd(v, st.lbh[IX(j)], st.ubh[IX(j)]);
        x[IX(j)] = v;
        x0[IX(j)] = v;
    }
    for (int i = 0; i < m; ++i) {
        const double v = P.warm ? st.y[IX(i)] : 0.0;
        y[IX(i)] = v;
        y0[IX(i)] = v;
    }
    for (int j = 0; j < n; ++j) {
        double a = 0.0;
        for (int kc = col_ptr[j]; kc < col_ptr[j + 1]; ++kc) a += Ahc[IX(kc)] * y[IX(row_idx[kc])];
        aty[IX(j)] = a;
        aty0[IX(j)] = a;
    }
    double omega = st.omega[s];
    if (!(P.keep_omega && P.warm) && P.omega0 > 0.0) omega = P.omega0;
    const double eta = P.eta_frac / st.normA[s];
    const double g = P.gamma;

    double r0 = -1.0, rlast = INFINITY;
    double pobj = 0.0, dobj = 0.0;
    int hk = 0;  // Halpern counter since the last restart
    int it = 0;
    int stat = PHGPU_ITER_LIMIT;
    bool final_is_t = false;  // true: solution is T(z) (in xt/yt/xe)
    for (; it < P.max_iter; ++it) {
        const double tau = eta / omega, sig = eta * omega;
        const bool kkt = (it % P.check_every) == 0;
        // non-fused iteration (T(z) kept in xt / yt / xe) at restart-test points and on
        // the last iteration (the iteration-limit answer is T(z), which is box-feasible)
        const bool check = kkt || (it % P.restart_every) == 0 || it == P.max_iter - 1;
        const double a1 = (hk + 1.0) / (hk + 2.0), a0 = 1.0 / (hk + 2.0);
        double dx2 = 0.0, dy2 = 0.0;
        // --- primal step: xt = prox(x - tau (c - A^T y)); xe = 2 xt - x
        for (int j = 0; j < n; ++j) {
            const double xj = x[IX(j)];
            const double qj = qh[IX(j)];
            const double num = xj - tau * (ch[IX(j)] - aty[IX(j)]);
            const double xtj = clampd(qj != 0.0 ? num / (1.0 + tau * qj) : num, st.lbh[IX(j)], st.ubh[IX(j)]);
            xe[IX(j)] = 2.0 * xtj - xj;
            const double d = xj - xtj;
            dx2 += d * d;
            if (check) xt[IX(j)] = xtj;
            else x[IX(j)] = a1 * ((1.0 + g) * xtj - g * xj) + a0 * x0[IX(j)];
        }
        // --- dual step: yt = prox(y - sig A xe)
        for (int i = 0; i < m; ++i) {
            double ax = 0.0;
            for (int k = row_ptr[i]; k < row_ptr[i + 1]; ++k) ax += Ahr[IX(k)] * xe[IX(col_idx[k])];
            const double yi = y[IX(i)];
            const double yti = dual_prox(yi - sig * ax, sig, st.rlh[IX(i)], st.ruh[IX(i)]);
            yt[IX(i)] = yti;
            const double d = yi - yti;
            dy2 += d * d;
            if (!check) y[IX(i)] = a1 * ((1.0 + g) * yti - g * yi) + a0 * y0[IX(i)];
        }
        // --- A^T yt (Halpern-combined in place, or kept in xe at checks)
        for (int j = 0; j < n; ++j) {
            double a = 0.0;
            for (int kc = col_ptr[j]; kc < col_ptr[j + 1]; ++kc) a += Ahc[IX(kc)] * yt[IX(row_idx[kc])];
            if (check) xe[IX(j)] = a;
            else aty[IX(j)] = a1 * ((1.0 + g) * a - g * aty[IX(j)]) + a0 * aty0[IX(j)];
        }
        const double r = sqrt(omega * dx2 + dy2 / omega);
        if (r0 < 0.0) r0 = r;
        if (!check) {
            ++hk;
            continue;
        }
        // ---- KKT test on T(z) = (xt, yt), original space
        if (kkt) {
        double pres2 = 0.0, dres2 = 0.0;
        pobj = const_term;
        dobj = const_term;
        for (int i = 0; i < m; ++i) {
            double ax = 0.0;
            for (int k = row_ptr[i]; k < row_ptr[i + 1]; ++k) ax += Ahr[IX(k)] * xt[IX(col_idx[k])];
            const double dr = st.Dr[IX(i)];
            ax /= dr;
            const double rl = st.rl[IX(i)], ru = st.ru[IX(i)];
            const double v = ax - clampd(ax, rl, ru);
            pres2 += v * v;
            dobj += row_dual_term(yt[IX(i)] * dr, rl, ru);
        }
        for (int j = 0; j < n; ++j) {
            const double d = st.Dc[IX(j)];
            const double xo = d * xt[IX(j)];
            const double ce = ch[IX(j)] / d, qe = qh[IX(j)] / (d * d);
            const double at = xe[IX(j)] / d;
            // working bounds (phgpu_fix_nonants may have fixed this column)
            const double lbj = st.lbh[IX(j)] * d, ubj = st.ubh[IX(j)] * d;
            const double rc = ce + qe * xo - at;
            double lam;
            if (isfinite(lbj) && isfinite(ubj)) lam = rc;
            else if (isfinite(lbj)) lam = fmax(rc, 0.0);
            else if (isfinite(ubj)) lam = fmin(rc, 0.0);
            else lam = 0.0;
            const double dr = rc - lam;
            dres2 += dr * dr;
            pobj += ce * xo + 0.5 * qe * xo * xo;
            dobj += col_dual_term(ce - at, qe, lbj, ubj);
        }
        const bool conv = sqrt(pres2) <= P.eps_abs + P.eps_rel * (1.0 + bnorm) &&
                          sqrt(dres2) <= P.eps_abs + P.eps_rel * (1.0 + cnorm) &&
                          fabs(pobj - dobj) <= P.eps_abs + P.eps_rel * (1.0 + fabs(pobj) + fabs(dobj));
        if (conv) {
            stat = PHGPU_OPTIMAL;
            final_is_t = true;
            break;
        }
        if (P.infeas_start >= 0 && it >= P.infeas_start) {
            // certificates from d = T(z) - z (x, y: the iterate; xt, yt: T(z); aty = A^T y,
            // xe = A^T yt)
            double pobj_r = 0.0, pviol = 0.0, cdx = 0.0, dviol = 0.0;
            for (int i = 0; i < m; ++i) {
                const double dr = st.Dr[IX(i)];
                const double rl = st.rl[IX(i)], ru = st.ru[IX(i)];
                ray_row_terms(dr * (yt[IX(i)] - y[IX(i)]), rl, ru, pobj_r, pviol);
                double adx = 0.0;
                for (int k = row_ptr[i]; k < row_ptr[i + 1]; ++k)
                    adx += Ahr[IX(k)] * (xt[IX(col_idx[k])] - x[IX(col_idx[k])]);
                dviol += recession_viol2(adx / dr, rl, ru);
            }
            for (int j = 0; j < n; ++j) {
                const double d = st.Dc[IX(j)];
                const double lbj = st.lbh[IX(j)] * d, ubj = st.ubh[IX(j)] * d;
                ray_col_terms(-(xe[IX(j)] - aty[IX(j)]) / d, lbj, ubj, pobj_r, pviol);
                const double dxo = d * (xt[IX(j)] - x[IX(j)]);
                const double qe = qh[IX(j)] / (d * d);
                cdx += (ch[IX(j)] / d) * dxo;
                dviol += recession_viol2(dxo, lbj, ubj) + (qe * dxo) * (qe * dxo);
            }
            if (is_certificate(pobj_r, pviol, P.eps_inf)) {
                stat = PHGPU_PRIMAL_INFEASIBLE;
                break;
            }
            if (is_certificate(-cdx, dviol, P.eps_inf)) {
                stat = PHGPU_DUAL_INFEASIBLE;
                break;
            }
        }
        }
        // ---- restart test (cuPDLP+-style: sufficient decay / necessary decay without
        // progress / artificial: the Halpern run is a fixed fraction of the solve)
        const bool restart = (r <= P.bsuff * r0) || (r <= P.bnec * r0 && r > rlast) ||
                             (it > 0 && hk >= P.bart * it);
        rlast = r;
        if (restart) {
            double ddx = 0.0, ddy = 0.0;
            for (int j = 0; j < n; ++j) {
                const double v = xt[IX(j)];
                const double d = v - x0[IX(j)];
                ddx += d * d;
                x[IX(j)] = v;
                x0[IX(j)] = v;
                aty[IX(j)] = xe[IX(j)];
                aty0[IX(j)] = xe[IX(j)];
            }
            for (int i = 0; i < m; ++i) {
                const double v = yt[IX(i)];
                const double d = v - y0[IX(i)];
                ddy += d * d;
                y[IX(i)] = v;
                y0[IX(i)] = v;
            }
            ddx = sqrt(ddx);
            ddy = sqrt(ddy);
            if (ddx > 1e-10 && ddy > 1e-10)
                // geometric mean of omega and ||dy|| / ||dx||: exp(0.5 log(ddy/ddx) + 0.5 log(omega))
                // as one sqrt (fp64 exp / log are long software sequences)
                omega = clampd(sqrt(omega * (ddy / ddx)), P.wmin, P.wmax);
            hk = 0;
            r0 = -1.0;
            rlast = INFINITY;
        } else {
            for (int j = 0; j < n; ++j) {
                x[IX(j)] = a1 * ((1.0 + g) * xt[IX(j)] - g * x[IX(j)]) + a0 * x0[IX(j)];
                aty[IX(j)] = a1 * ((1.0 + g) * xe[IX(j)] - g * aty[IX(j)]) + a0 * aty0[IX(j)];
            }
            for (int i = 0; i < m; ++i)
                y[IX(i)] = a1 * ((1.0 + g) * yt[IX(i)] - g * y[IX(i)]) + a0 * y0[IX(i)];
            ++hk;
        }
    }
    // ---- write back: converged -> T(z); iteration limit -> current z
    if (final_is_t) {
        for (int j = 0; j < n; ++j) x[IX(j)] = xt[IX(j)];
        for (int i = 0; i < m; ++i) y[IX(i)] = yt[IX(i)];
    } else {
        // iteration limit: answer T(z) of the last iteration (xt, yt, A^T yt in xe)
        for (int j = 0; j < n; ++j) {
            x[IX(j)] = xt[IX(j)];
            aty[IX(j)] = xe[IX(j)];
        }
        for (int i = 0; i < m; ++i) y[IX(i)] = yt[IX(i)];
        pobj = const_term;
        dobj = const_term;
        for (int i = 0; i < m; ++i) dobj += row_dual_term(y[IX(i)] * st.Dr[IX(i)], st.rl[IX(i)], st.ru[IX(i)]);
        for (int j = 0; j < n; ++j) {
            const double d = st.Dc[IX(j)];
            const double xo = d * x[IX(j)];
            const double ce = ch[IX(j)] / d, qe = qh[IX(j)] / (d * d);
            pobj += ce * xo + 0.5 * qe * xo * xo;
            dobj += col_dual_term(ce - aty[IX(j)] / d, qe, st.lbh[IX(j)] * d, st.ubh[IX(j)] * d);
        }
    }
    if (stat == PHGPU_PRIMAL_INFEASIBLE) pobj = dobj = INFINITY;
    if (stat == PHGPU_DUAL_INFEASIBLE) pobj = dobj = -INFINITY;
    for (int j = 0; j < n; ++j) xout[IX(j)] = st.Dc[IX(j)] * x[IX(j)];
    if (yout)
        for (int i = 0; i < m; ++i) yout[IX(i)] = st.Dr[IX(i)] * y[IX(i)];
    st.omega_w[s] = omega;
    obj[s] = pobj;
    bound[s] = dobj;
    status[s] = stat;
    if (iters) iters[s] = (stat == PHGPU_ITER_LIMIT) ? P.max_iter : it;
    if (stats) {  // list mode: this solve's statistics (the IPM counted the others)
        const unsigned long long its = (unsigned long long)((stat == PHGPU_ITER_LIMIT) ? P.max_iter : it);
        atomicAdd(&stats[stat], 1ull);
        atomicAdd(&stats[4], its);
        atomicMax(&stats[5], its);
    }
}

// The path-6 statistics {OPTIMAL, ITER_LIMIT, PRIMAL_INF, DUAL_INF, iteration sum, iteration
// maximum, jam hand-overs, re-centrings} are PHGPU_STATS_COPIES copies, one 128-B line each:
// wave w of a path-6 kernel adds to copy w % copies.  One copy took every wave's atomics,
// thousands on one L2 line, serialised there for ~20 us at the end of the 8,192-share launch
// (the stores and epilogue queued behind them; tools/ipm_prof.py).  Readers sum
// the copies (the maximum for word 5); stats_gen (paths without in-kernel statistics) is one
// copy.
#define PHGPU_STATS_COPIES 32
#define PHGPU_STATS_STRIDE 16
#define PHGPU_STATS_WORDS (PHGPU_STATS_COPIES * PHGPU_STATS_STRIDE)
inline unsigned long long stats_word(const unsigned long long* s, int copies, int k) {
    unsigned long long a = 0;
    for (int c = 0; c < copies; ++c) {
        const unsigned long long v = s[c * PHGPU_STATS_STRIDE + k];
        a = (k == 5) ? (v > a ? v : a) : a + v;
    }
    return a;
}

// the six statistics summed over the copies by a whole wave: lane t < copies reads copy t (one
// load latency; a thread reading the 32 copies in turn took 8 us), the wave reduces, every
// lane returns them
__device__ __forceinline__ void stats_wave(const unsigned long long* __restrict__ s, int copies,
                                           unsigned long long v[6]) {
    const int t = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] = t < copies ? s[t * PHGPU_STATS_STRIDE + k] : 0ull;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const unsigned long long u = __shfl_xor(v[k], o, 64);
            v[k] = k == 5 ? (u > v[k] ? u : v[k]) : v[k] + u;
        }
}

// the six statistics of a solve into out (int64): one wave
__global__ void k_stats_copy(const unsigned long long* __restrict__ src, int copies, int64_t* __restrict__ out) {
    unsigned long long v[6];
    stats_wave(src, copies, v);
    if (threadIdx.x < 6) {
        unsigned long long w = v[0];
#pragma unroll
        for (int k = 1; k < 6; ++k) w = (int)threadIdx.x == k ? v[k] : w;
        out[threadIdx.x] = (int64_t)w;
    }
}

#include "solve_reg.inc"
#include "solve_wg.inc"
#include "solve_stream.inc"
#include "solve_jit.inc"
#include "solve_ipm.inc"

// ------------------------------------------------------------------ PH reductions
// (kernels and device helpers; their entry points are under "C-ABI" below)
#include "ph_reduce.inc"
#include "ph_fixer.inc"
#include "ph_fwph.inc"
#include "ph_aph.inc"
#include "ph_lshaped.inc"
#include "ph_ef.inc"
#include "ph_ef_tree.inc"
#include "ph_gap.inc"

// Xhat_Eval._fix_nonants (utils/xhat_eval.py; spopt.py _fix_nonants): nonant columns of
// every scenario get lb = ub = xfix[k, s] (scaled); xfix == NULL restores the model bounds.
__global__ void __launch_bounds__(BLOCK)
k_fix_nonants(ph_data st, const double* __restrict__ xfix) {
    const int64_t S = st.S;
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    for (int k = 0; k < st.nn; ++k) {
        const int j = st.nonant_col[k];
        const double d = st.Dc[IX(j)];
        const double xv = xfix ? xfix[IX(k)] : NAN;
        if (!isnan(xv)) {
            const double v = fmin(fmax(xv, st.lb[IX(j)]), st.ub[IX(j)]);
            st.lbh[IX(j)] = v / d;
            st.ubh[IX(j)] = v / d;
        } else {
            st.lbh[IX(j)] = st.lb[IX(j)] / d;
            st.ubh[IX(j)] = st.ub[IX(j)] / d;
        }
    }
}

// ------------------------------------------------------------------ lane plan (host)
#include <vector>
#include <algorithm>

// Build the per-lane plan of solve_reg.inc for L lanes per scenario: lane l owns
// columns j = l + q L and rows i = l + r L; each column's CSC entries and each row's
// CSR entries are padded to the instance's ZC / ZR slots.  Returns false if no
// compiled instance fits (then the global-memory kernel is used).
// register-cost estimate of an instance, in doubles per lane
static inline long reg_cost(const reg_instance& r) {
    return (long)r.KC * (13 + r.ZC) + (long)r.KR * (7 + r.ZR);
}

// an instance that spills more than REG_SPILL_MAX bytes of scratch per lane at 2 waves /
// SIMD is skipped by the lane search (L doubles past it).  Both variants are checked --
// scenario order (fn) and record mode (fn_rec), whichever phgpu_solve will launch.
// Measured on farmer 65,536 cm=1 (profiles/r01): <8,4,4,4> at L=2 spills 1.5 KB -> 14.4 ms
// per solve; <2,3,1,4> at L=8, no spill -> 0.77 ms.  <3,3,2,4> (the headline instance)
// spills 28 B (fn) / 268 B (fn_rec), all of it outside the PDHG step loop: the scratch
// operations of its code object sit in the prologue, the scenario load / refill, the check
// iteration and the write-back, none in the R-1 plain steps (tools/scratch_regions.py,
// profiles/r03/scratch_regions.txt) -- so the cap sits above 268 B.  The first instance
// whose step loop spills is <6,4,2,4> (568 / 940 B, 43 / 37 scratch ops in the loop);
// <4,4,2,4> (216 / 508 B) keeps its loop clean but spills 98 / 174 times in the check and
// refill paths, and stays excluded as before.
#ifndef REG_SPILL_MAX
#define REG_SPILL_MAX 320
#endif
static bool reg_spills(const reg_instance& r) {
    for (reg_kernel_t f : {r.fn, r.fn_rec}) {
        hipFuncAttributes a;
        if (hipFuncGetAttributes(&a, (const void*)f) != hipSuccess) continue;
        if (a.localSizeBytes > REG_SPILL_MAX) return true;
    }
    return false;
}

static bool build_plan(int L, int n, int m, const int32_t* row_ptr, const int32_t* col_idx,
                       int* inst_out, int* kc_out, int* zc_out, int* kr_out, int* zr_out,
                       std::vector<int32_t>& col_k, std::vector<int32_t>& col_r,
                       std::vector<int32_t>& row_k, std::vector<int32_t>& row_c) {
    if (m < 1 || n < 1) return false;
    const int kc = (n + L - 1) / L;
    const int kr = (m + L - 1) / L;
    std::vector<std::vector<std::pair<int, int>>> cols(n);  // (csr k, row)
    for (int i = 0; i < m; ++i)
        for (int k = row_ptr[i]; k < row_ptr[i + 1]; ++k) cols[col_idx[k]].push_back({k, i});
    int zc = 1, zr = 1;
    for (int j = 0; j < n; ++j) zc = std::max(zc, (int)cols[j].size());
    for (int i = 0; i < m; ++i) zr = std::max(zr, (int)(row_ptr[i + 1] - row_ptr[i]));
    int inst = -1;
    long best = 0;
    const int ninst = (int)(sizeof(g_reg_instances) / sizeof(g_reg_instances[0]));
    for (int a = 0; a < ninst; ++a) {
        const reg_instance& r = g_reg_instances[a];
        if (r.KC >= kc && r.ZC >= zc && r.KR >= kr && r.ZR >= zr) {
            const long cost = reg_cost(r);
            if (inst < 0 || cost < best) {
                inst = a;
                best = cost;
            }
        }
    }
    if (inst < 0) return false;
    col_k.assign((size_t)L * kc * zc, -1);
    col_r.assign((size_t)L * kc * zc, 0);
    for (int u = 0; u < L; ++u)
        for (int q = 0; q < kc; ++q) {
            const int j = u + q * L;
            if (j >= n) continue;
            for (int z = 0; z < (int)cols[j].size(); ++z) {
                col_k[((size_t)u * kc + q) * zc + z] = cols[j][z].first;
                col_r[((size_t)u * kc + q) * zc + z] = cols[j][z].second;
            }
        }
    row_k.assign((size_t)L * kr * zr, -1);
    row_c.assign((size_t)L * kr * zr, 0);
    for (int u = 0; u < L; ++u)
        for (int r = 0; r < kr; ++r) {
            const int i = u + r * L;
            if (i >= m) continue;
            for (int k = row_ptr[i], z = 0; k < row_ptr[i + 1]; ++k, ++z) {
                row_k[((size_t)u * kr + r) * zr + z] = k;
                row_c[((size_t)u * kr + r) * zr + z] = col_idx[k];
            }
        }
    *inst_out = inst;
    *kc_out = kc;
    *zc_out = zc;
    *kr_out = kr;
    *zr_out = zr;
    return true;
}

// per-lane VALU estimate of one PDHG iteration of a slot layout, shared by the path
// choice: a column slot ~ 10 + 2 ZC instructions, a row slot ~ 8 + 2 ZR, each long slot's
// wave reduction ~ 20.  A scenario costs (lanes / 64) times that.
static inline long slot_cost(int KC, int ZC, int KR, int ZR, int nlong) {
    return (long)KC * (10 + 2 * ZC) + (long)KR * (8 + 2 * ZR) + 20L * nlong;
}

// The workgroup kernels spill only around a scenario's load and write-back (the solve
// loops of every instance are scratch-free: objdump of the code object), once per
// several hundred PDHG iterations, so their cap is looser than the register path's.
#define WG_SPILL_MAX 512
static bool wg_spills(const wg_instance& g) {
    hipFuncAttributes a;
    if (hipFuncGetAttributes(&a, (const void*)g.fn) != hipSuccess) return false;
    return a.localSizeBytes > WG_SPILL_MAX;
}

struct wg_plan_host {
    int nlong = 0, long_per_wave = 0;
    std::vector<int32_t> col_id, row_id, col_long, row_long, col_k, col_r, row_k, row_c;
};

// Assign K slots x L lanes to N items (rows or columns) with entry lists ``items``
// (pairs CSR position, partner index), padded to Z entries per slot.  An item with more
// than Z entries is long: it takes a whole wave slot (from the last slot / wave
// backwards), its entries split evenly over the wave's 64 lanes; the short items fill the
// remaining (slot, lane) positions in order.  False if they do not fit.
static bool wg_assign(int K, int Z, int W, const std::vector<std::vector<std::pair<int, int>>>& items,
                      std::vector<int32_t>& id, std::vector<int32_t>& lng, std::vector<int32_t>& ek,
                      std::vector<int32_t>& eo, int& nlong, std::vector<int>& per_wave) {
    const int L = WAVE * W;
    const int N = (int)items.size();
    id.assign((size_t)K * L, -1);
    lng.assign((size_t)K * W, 0);
    ek.assign((size_t)K * L * Z, -1);
    eo.assign((size_t)K * L * Z, 0);
    std::vector<char> taken((size_t)K * W, 0);
    int ws = K * W - 1;
    for (int a = 0; a < N; ++a) {
        const int d = (int)items[a].size();
        if (d <= Z) continue;
        if (d > WAVE * Z || ws < 0) return false;
        const int q = ws / W, w = ws % W;
        --ws;
        taken[(size_t)q * W + w] = 1;
        lng[(size_t)q * W + w] = 1;
        ++nlong;
        ++per_wave[w];
        const int per = (d + WAVE - 1) / WAVE;
        for (int l = 0; l < WAVE; ++l) {
            const size_t slot = (size_t)q * L + w * WAVE + l;
            id[slot] = a;
            for (int z = 0; z < per; ++z) {
                const int e = l * per + z;
                if (e >= d) break;
                ek[slot * Z + z] = items[a][e].first;
                eo[slot * Z + z] = items[a][e].second;
            }
        }
    }
    long pos = 0;  // q-major over (slot, lane)
    for (int a = 0; a < N; ++a) {
        const int d = (int)items[a].size();
        if (d > Z) continue;
        while (pos < (long)K * L && taken[(size_t)(pos / L) * W + (pos % L) / WAVE])
            pos = (pos / WAVE + 1) * WAVE;     // skip the rest of a long-item wave slot
        if (pos >= (long)K * L) return false;
        const size_t slot = (size_t)pos;
        id[slot] = a;
        for (int z = 0; z < d; ++z) {
            ek[slot * Z + z] = items[a][z].first;
            eo[slot * Z + z] = items[a][z].second;
        }
        ++pos;
    }
    return true;
}

// Plan of solve_wg.inc for one instance.
static bool build_wg_plan(const wg_instance& g, int n, int m, const int32_t* row_ptr, const int32_t* col_idx,
                          wg_plan_host& out) {
    if (m < 1 || n < 1) return false;
    std::vector<std::vector<std::pair<int, int>>> cols(n), rows(m);
    for (int i = 0; i < m; ++i)
        for (int k = row_ptr[i]; k < row_ptr[i + 1]; ++k) {
            cols[col_idx[k]].push_back({k, i});
            rows[i].push_back({k, col_idx[k]});
        }
    std::vector<int> pwc(g.WPS, 0), pwr(g.WPS, 0);
    int nl = 0;
    if (!wg_assign(g.KC, g.ZC, g.WPS, cols, out.col_id, out.col_long, out.col_k, out.col_r, nl, pwc)) return false;
    if (!wg_assign(g.KR, g.ZR, g.WPS, rows, out.row_id, out.row_long, out.row_k, out.row_c, nl, pwr)) return false;
    out.nlong = nl;
    out.long_per_wave = 0;
    for (int w = 0; w < g.WPS; ++w) out.long_per_wave = std::max(out.long_per_wave, pwc[w] + pwr[w]);
    return true;
}

// ------------------------------------------------------------------ C-ABI
// ---------------------------------------------------------- scenario-major records
static hipError_t to_records(phgpu_state* h, const double* in, int K, int off, hipStream_t st) {
    if (K <= 0) return hipSuccess;
    const dim3 g((unsigned)((h->S + TT - 1) / TT), (unsigned)((K + TT - 1) / TT));
    hipLaunchKernelGGL(k_to_records, g, dim3(256), 0, st, in, K, h->S, h->pk, h->pk_stride, off);
    return hipGetLastError();
}

// this solve's PH state (W if on, rho and xbar if the prox term is on) into the records
static hipError_t ph_to_records(phgpu_state* h, hipStream_t st) {
    if (h->nn <= 0 || (!h->W_on && !h->prox_on)) return hipSuccess;
    const dim3 g((unsigned)((h->S + TT - 1) / TT), (unsigned)((3 * h->nn + TT - 1) / TT));
    hipLaunchKernelGGL(k_to_records_ph, g, dim3(256), 0, st, h->W_on ? h->W : nullptr,
                       h->prox_on ? h->rho : nullptr, h->prox_on ? h->xbar : nullptr, h->nn, h->S, h->pk,
                       h->pk_stride, h->pk_W);
    return hipGetLastError();
}

static hipError_t from_records(phgpu_state* h, int off, int moff, int K, double* out, hipStream_t st) {
    if (K <= 0 || !out) return hipSuccess;
    const dim3 g((unsigned)((h->S + TT - 1) / TT), (unsigned)((K + TT - 1) / TT));
    hipLaunchKernelGGL(k_from_records, g, dim3(256), 0, st, (const double*)h->pk, h->pk_stride, off, moff, K,
                       h->S, out);
    return hipGetLastError();
}

// Point the warm-state fields at slot wslot (read) and slot ``wq`` (write; == wslot except
// during a deferred solve) -- see the slot fields of phgpu_state.
static void bind_slots(phgpu_state* h) {
    const int p = h->wslot, wq = h->wq;
    h->x = h->xs[p];
    h->y = h->ys[p];
    h->omega = h->oms[p];
    h->sk_iters = h->its_s[p];
    h->pk_X = h->pkXs[p];
    h->pk_Y = h->pkYs[p];
    h->have_solution = h->have_s[p];
    h->warm_rec = h->warm_rec_s[p];
    h->xw = h->xs[wq];
    h->yw = h->ys[wq];
    h->omega_w = h->oms[wq];
    h->its_w = h->its_s[wq];
    h->pk_XW = h->pkXs[wq];
    h->pk_YW = h->pkYs[wq];
}

// record layout: A (CSR order) | c q Dc lb^ ub^ (n) | rl ru Dr rl^ ru^ (m) | x^ (n) y^ (m)
// warm start of slot 0 | W rho xbar (nn) PH state of the current solve | x^ (n) y^ (m) warm
// start of slot 1; stride rounded to 16 doubles
static int pack_alloc(phgpu_state* h) {
    if (h->pk) return 0;
    const int n = h->n, m = h->m, nnz = h->nnz, nn = h->nn;
    int o = 0;
    h->pk_A = o; o += nnz;
    h->pk_C = o; o += n;
    h->pk_Q = o; o += n;
    h->pk_DC = o; o += n;
    h->pk_LB = o; o += n;
    h->pk_UB = o; o += n;
    h->pk_RL = o; o += m;
    h->pk_RU = o; o += m;
    h->pk_DR = o; o += m;
    h->pk_RLH = o; o += m;
    h->pk_RUH = o; o += m;
    h->pk_X = o; o += n;
    h->pk_Y = o; o += m;
    h->pk_W = o; o += nn;
    h->pk_RHO = o; o += nn;
    h->pk_XB = o; o += nn;
    h->pkXs[0] = h->pk_X;
    h->pkYs[0] = h->pk_Y;
    h->pkXs[1] = o; o += n;
    h->pkYs[1] = o; o += m;
    h->pk_stride = (o + 15) / 16 * 16;
    bind_slots(h);
    return dalloc(h, &h->pk, (size_t)h->pk_stride * (size_t)h->S);
}

// copy the scaled problem (k_setup's output) into the records
static hipError_t pack_fill(phgpu_state* h, hipStream_t st) {
    struct { const double* a; int K, off; } f[] = {
        {h->Ah_csr, h->nnz, h->pk_A}, {h->c, h->n, h->pk_C}, {h->q, h->n, h->pk_Q}, {h->Dc, h->n, h->pk_DC},
        {h->lbh, h->n, h->pk_LB}, {h->ubh, h->n, h->pk_UB}, {h->rl, h->m, h->pk_RL}, {h->ru, h->m, h->pk_RU},
        {h->Dr, h->m, h->pk_DR}, {h->rlh, h->m, h->pk_RLH}, {h->ruh, h->m, h->pk_RUH}, {h->x, h->n, h->pk_X},
        {h->y, h->m, h->pk_Y}};
    for (auto& e : f) {
        const hipError_t r = to_records(h, e.a, e.K, e.off, st);
        if (r != hipSuccess) return r;
    }
    return hipSuccess;
}

// sliced-ELL layout of the shared pattern (rows and columns in slices of 64); values are
// filled from the scaled CSR / CSC copies by k_sh_sell_vals
static int sell_one(phgpu_state* h, int K, const std::vector<int32_t>& ptr, const std::vector<int32_t>& idx,
                    const std::vector<int32_t>& src, int& nsl, int& nent, int32_t** d_off, int32_t** d_len, int32_t** d_idx,
                    int32_t** d_src, double** d_val, int32_t** d_wptr, int32_t** d_wslc) {
    nsl = (K + WAVE - 1) / WAVE;
    std::vector<int32_t> off((size_t)nsl + 1), len((size_t)nsl);
    int64_t tot = 0;
    for (int sl = 0; sl < nsl; ++sl) {
        int L = 0;
        for (int l = 0; l < WAVE; ++l) {
            const int r = sl * WAVE + l;
            if (r < K) L = std::max(L, ptr[r + 1] - ptr[r]);
        }
        off[sl] = (int32_t)tot;
        len[sl] = L;
        tot += (int64_t)L * WAVE;
        if (tot >= (1LL << 31)) return set_err(-1, "sliced-ELL copy too large");
    }
    off[nsl] = (int32_t)tot;
    nent = (int)tot;
    std::vector<int32_t> e_idx((size_t)std::max<int64_t>(tot, 1), 0), e_src((size_t)std::max<int64_t>(tot, 1), -1);
    for (int sl = 0; sl < nsl; ++sl)
        for (int l = 0; l < WAVE; ++l) {
            const int r = sl * WAVE + l;
            if (r >= K) continue;
            for (int k = 0; k < ptr[r + 1] - ptr[r]; ++k) {
                const size_t e = (size_t)off[sl] + (size_t)k * WAVE + l;
                e_idx[e] = idx[ptr[r] + k];
                e_src[e] = src[ptr[r] + k];
            }
        }
    // slices -> waves of the streaming workgroup: longest first onto the least loaded wave
    // (cost = entries per lane + a fixed per-slice overhead), each wave's list in slice order
    std::vector<int32_t> bysz((size_t)nsl);
    for (int sl = 0; sl < nsl; ++sl) bysz[sl] = sl;
    std::stable_sort(bysz.begin(), bysz.end(), [&](int a, int b) { return len[a] > len[b]; });
    std::vector<int64_t> load(SWAVES, 0);
    std::vector<std::vector<int32_t>> lists(SWAVES);
    for (int sl : bysz) {
        int w = 0;
        for (int v = 1; v < SWAVES; ++v)
            if (load[v] < load[w]) w = v;
        load[w] += len[sl] + 4;
        lists[w].push_back(sl);
    }
    std::vector<int32_t> wptr(SWAVES + 1, 0), wslc;
    for (int w = 0; w < SWAVES; ++w) {
        std::sort(lists[w].begin(), lists[w].end());
        wslc.insert(wslc.end(), lists[w].begin(), lists[w].end());
        wptr[w + 1] = (int32_t)wslc.size();
    }
    struct { int32_t** d; const std::vector<int32_t>* v; } up[] = {
        {d_off, &off}, {d_len, &len}, {d_idx, &e_idx}, {d_src, &e_src}, {d_wptr, &wptr}, {d_wslc, &wslc}};
    int rc = dalloc(h, d_val, e_idx.size());
    for (auto& u : up)
        if (!rc) rc = dupload(h, u.d, *u.v, "sliced-ELL");
    return rc;
}

static int build_sell(phgpu_state* h, const int32_t* row_ptr, const int32_t* col_idx) {
    const int n = h->n, m = h->m, nnz = h->nnz;
    // rows: CSR as given, source = CSR position
    std::vector<int32_t> rp(row_ptr, row_ptr + m + 1), ci(col_idx, col_idx + nnz), rsrc((size_t)nnz);
    for (int k = 0; k < nnz; ++k) rsrc[k] = k;
    int rc = sell_one(h, m, rp, ci, rsrc, h->nsl_r, h->nent_r, &h->rs_off, &h->rs_len, &h->rs_idx, &h->rs_src, &h->rs_val,
                      &h->rw_ptr, &h->rw_slc);
    if (rc) return rc;
    // columns: the CSC order of phgpu_create (rows ascending within a column), source =
    // CSC position
    std::vector<int32_t> cp((size_t)n + 1, 0), ri((size_t)nnz), csrc((size_t)nnz);
    for (int k = 0; k < nnz; ++k) cp[col_idx[k] + 1]++;
    for (int j = 0; j < n; ++j) cp[j + 1] += cp[j];
    std::vector<int32_t> fill(cp.begin(), cp.end() - 1);
    for (int i = 0; i < m; ++i)
        for (int k = row_ptr[i]; k < row_ptr[i + 1]; ++k) {
            const int p = fill[col_idx[k]]++;
            ri[p] = i;
            csrc[p] = p;
        }
    return sell_one(h, n, cp, ri, csrc, h->nsl_c, h->nent_c, &h->cs_off, &h->cs_len, &h->cs_idx, &h->cs_src, &h->cs_val,
                    &h->cw_ptr, &h->cw_slc);
}

// several plan vectors onto the device; an allocation failure as "<what> allocation failed"
struct plan_upload {
    int32_t** d;
    const std::vector<int32_t>* v;
};
static int plan_uploads(phgpu_state* h, const plan_upload* up, int cnt, const char* what) {
    int rc = 0;
    for (int k = 0; k < cnt && !rc; ++k) rc = dupload(h, up[k].d, *up[k].v, what);
    if (rc == -3) return set_err(-3, "%s allocation failed", what);
    return rc;
}

// register-resident path: lanes per scenario L (power of two <= 64): the smallest L
// with a fitting instance, doubled while S * L lanes would not fill REG_WAVES_PER_EU
// waves on every SIMD of the chip and a scenario still has columns to spread
// (measured on farmer cm=1: L=4 at S >= 32768, 8 at 16384, 16 at 8192 -- profiles/r01),
// and past any L whose instance spills (reg_spills);
// PHGPU_LANES=<L> pins it (tuning / tests)
static int reg_plan_select(phgpu_state* h, const int32_t* row_ptr, const int32_t* col_idx) {
    const int n = h->n, m = h->m;
    const int64_t target = (int64_t)h->num_cus * 4 * WAVE * REG_WAVES_PER_EU;
    const char* env = getenv("PHGPU_LANES");
    const int pinned = env ? atoi(env) : 0;
    int chosen = -1;
    bool chosen_spills = false;
    std::vector<int32_t> ck, cr, rk, rc;
    int inst = -1, kc = 0, zc = 0, kr = 0, zr = 0;
    for (int L = 1; L <= WAVE; L *= 2) {
        if (pinned > 0 && L != pinned) continue;
        std::vector<int32_t> a1, a2, a3, a4;
        int i1, i2, i3, i4, i5;
        if (!build_plan(L, n, m, row_ptr, col_idx, &i1, &i2, &i3, &i4, &i5, a1, a2, a3, a4)) continue;
        if (pinned <= 0 && chosen >= 0 && (h->S * (int64_t)chosen >= target || chosen >= n) &&
            !chosen_spills)
            break;
        chosen = L;
        chosen_spills = reg_spills(g_reg_instances[i1]);
        inst = i1; kc = i2; zc = i3; kr = i4; zr = i5;
        ck.swap(a1); cr.swap(a2); rk.swap(a3); rc.swap(a4);
    }
    if (chosen <= 0) return 0;
    const plan_upload up[] = {{&h->pl_col_k, &ck}, {&h->pl_col_r, &cr}, {&h->pl_row_k, &rk}, {&h->pl_row_c, &rc}};
    const int rcu = plan_uploads(h, up, 4, "plan");
    if (rcu) return rcu;
    h->reg_inst = inst;
    h->reg_L = chosen;
    h->reg_kc = kc;
    h->reg_zc = zc;
    h->reg_kr = kr;
    h->reg_zr = zr;
    return 0;
}

// workgroup-per-scenario path: the cheapest non-spilling instance by slot_cost x waves
// per scenario (PHGPU_WPS=<waves> pins the waves per scenario); *best = its cost
static int wg_plan_select(phgpu_state* h, const int32_t* row_ptr, const int32_t* col_idx, long* best) {
    const char* env = getenv("PHGPU_WPS");
    const int pinned = env ? atoi(env) : 0;
    const int ninst = (int)(sizeof(g_wg_instances) / sizeof(g_wg_instances[0]));
    wg_plan_host bp;
    *best = 0;
    for (int a = 0; a < ninst; ++a) {
        const wg_instance& g = g_wg_instances[a];
        if (pinned > 0 && g.WPS != pinned) continue;
        wg_plan_host p;
        if (!build_wg_plan(g, h->n, h->m, row_ptr, col_idx, p)) continue;
        if (wg_spills(g)) continue;
        const long cost = (long)g.WPS * slot_cost(g.KC, g.ZC, g.KR, g.ZR, p.long_per_wave);
        if (h->wg_inst < 0 || cost < *best) {
            h->wg_inst = a;
            *best = cost;
            bp = std::move(p);
        }
    }
    if (h->wg_inst < 0) return 0;
    const plan_upload up[] = {{&h->wg_col_id, &bp.col_id},     {&h->wg_row_id, &bp.row_id},
                              {&h->wg_col_long, &bp.col_long}, {&h->wg_row_long, &bp.row_long},
                              {&h->wg_col_k, &bp.col_k},       {&h->wg_col_r, &bp.col_r},
                              {&h->wg_row_k, &bp.row_k},       {&h->wg_row_c, &bp.row_c}};
    const int rc = plan_uploads(h, up, 8, "workgroup plan");
    if (rc) return rc;
    h->wg_long = bp.nlong;
    return 0;
}

static int step_local_impl(phgpu_state* h, const double* x, double* node_buf, double* xbar, double* W,
                           const double* rho, int update_W, double* conv_local, int64_t* stats_out, hipStream_t st);

static bool xp_valid(const phgpu_state* h, const double* x);

// run a deferred PH step now (its recorded stream), if one is pending
static int flush_step(phgpu_state* h) {
    if (!h || !h->pend.active) return 0;
    phgpu_state::ph_pending q = h->pend;
    h->pend.active = 0;
    return step_local_impl(h, q.x, q.node_buf, q.xbar, q.W, q.rho, q.update_W, q.conv, q.stats, q.stream);
}
#define FLUSH_STEP(h)                      \
    do {                                   \
        const int frc_ = flush_step(h);    \
        if (frc_) return frc_;             \
    } while (0)

extern "C" int phgpu_default_options(phgpu_options* o) {
    if (!o) return set_err(-1, "null options");
    o->eps_rel = 1e-9;
    o->eps_abs = 1e-12;
    o->max_iter = 100000;
    o->check_every = 64;
    o->gamma = 1.0;
    o->beta_sufficient = 0.2;
    o->beta_necessary = 0.8;
    o->eta_frac = 0.998;
    o->omega0 = 1.0;
    o->keep_omega = 1;
    o->restart_every = 16;
    o->beta_artificial = 0.36;
    o->omega_clamp = 1e4;
    o->kernel = 0;
    o->infeas_start = 512;
    o->eps_infeas = 1e-8;
    o->split_longest = 0;
    return 0;
}

extern "C" int phgpu_create(phgpu_handle* out, int device, int64_t S, int32_t n, int32_t m,
                            int32_t nnz, const int32_t* row_ptr, const int32_t* col_idx,
                            int32_t nn, const int32_t* nonant_col, const int32_t* nonant_depth,
                            const int32_t* nonant_off, int32_t depth, int32_t num_nodes,
                            int32_t nlen_max) {
    return phgpu_create2(out, device, S, n, m, nnz, row_ptr, col_idx, nn, nonant_col, nonant_depth, nonant_off,
                         depth, num_nodes, nlen_max, 0u);
}

extern "C" int phgpu_create2(phgpu_handle* out, int device, int64_t S, int32_t n, int32_t m,
                             int32_t nnz, const int32_t* row_ptr, const int32_t* col_idx,
                             int32_t nn, const int32_t* nonant_col, const int32_t* nonant_depth,
                             const int32_t* nonant_off, int32_t depth, int32_t num_nodes,
                             int32_t nlen_max, uint32_t flags) {
    if (flags & ~(uint32_t)PHGPU_SHARED_MATRIX) return set_err(-1, "unknown flags 0x%x", flags);
    if (!out) return set_err(-1, "null handle pointer");
    *out = nullptr;
    if (S <= 0 || S >= (1LL << 31) || n <= 0 || m < 0 || nnz < 0 || nn < 0 || depth < 1 || num_nodes < 1 ||
        nlen_max < 0)
        return set_err(-1, "bad sizes S=%lld n=%d m=%d nnz=%d nn=%d depth=%d nodes=%d",
                       (long long)S, n, m, nnz, nn, depth, num_nodes);
    if (!row_ptr || (nnz > 0 && !col_idx) || (nn > 0 && (!nonant_col || !nonant_depth || !nonant_off)))
        return set_err(-1, "null pattern pointer");
    // host-side validation of the shared pattern
    if (row_ptr[0] != 0 || row_ptr[m] != nnz) return set_err(-1, "row_ptr must start at 0 and end at nnz");
    for (int i = 0; i < m; ++i)
        if (row_ptr[i + 1] < row_ptr[i]) return set_err(-1, "row_ptr not monotone at row %d", i);
    for (int k = 0; k < nnz; ++k)
        if (col_idx[k] < 0 || col_idx[k] >= n) return set_err(-1, "col_idx[%d]=%d out of range", k, col_idx[k]);
    std::vector<int32_t> slot((size_t)n, -1);
    for (int k = 0; k < nn; ++k) {
        if (nonant_col[k] < 0 || nonant_col[k] >= n || slot[nonant_col[k]] >= 0 ||
            nonant_depth[k] < 0 || nonant_depth[k] >= depth || nonant_off[k] < 0 ||
            nonant_off[k] >= nlen_max)
            return set_err(-1, "bad nonant map at %d", k);
        slot[nonant_col[k]] = k;
    }
    HIPCHK(hipSetDevice(device));
    phgpu_state* h = new (std::nothrow) phgpu_owner();  // value-initialised: every layer's fields start at zero
    if (!h) return set_err(-3, "out of host memory");
    h->last_rec = -1;
    h->device = device;
    h->S = S;
    h->n = n;
    h->m = m;
    h->nnz = nnz;
    h->nn = nn;
    h->depth = depth;
    h->num_nodes = num_nodes;
    h->nlen_max = nlen_max;
    h->nwaves = (S + WAVE - 1) / WAVE;
    h->xbar_mixed = -1;
    // transposed pattern (host)
    std::vector<int32_t> cptr((size_t)n + 1, 0), ridx((size_t)nnz), perm((size_t)nnz), rowof((size_t)nnz);
    for (int k = 0; k < nnz; ++k) cptr[col_idx[k] + 1]++;
    for (int j = 0; j < n; ++j) cptr[j + 1] += cptr[j];
    {
        std::vector<int32_t> fill(cptr.begin(), cptr.end() - 1);
        for (int i = 0; i < m; ++i)
            for (int k = row_ptr[i]; k < row_ptr[i + 1]; ++k) {
                const int p = fill[col_idx[k]]++;
                ridx[p] = i;
                perm[p] = k;
                rowof[k] = i;
            }
    }
    const size_t Sz = (size_t)S;
    ALLOC(h->row_ptr, m + 1);
    ALLOC(h->col_idx, nnz);
    ALLOC(h->col_ptr, n + 1);
    ALLOC(h->row_idx, nnz);
    ALLOC(h->perm, nnz);
    ALLOC(h->row_of, nnz);
    ALLOC(h->nonant_col, nn);
    ALLOC(h->nonant_depth, nn);
    ALLOC(h->nonant_off, nn);
    ALLOC(h->nonant_slot, n);
    ALLOC(h->objc, Sz);
    ALLOC(h->prob, Sz);
    ALLOC(h->pcoef, (size_t)depth * Sz);
    ALLOC(h->node_of, (size_t)depth * Sz);
    ALLOC(h->omega, Sz);
    h->shared = (flags & PHGPU_SHARED_MATRIX) ? 1 : 0;
    // longest-first work queue (paths 2 and 4): iteration counts of the last solve, the
    // queue order and the counting-sort bins
    ALLOC(h->sk_iters, Sz);
    ALLOC(h->sk_order, Sz);
    ALLOC(h->sk_bins, 4 * ORDER_BINS);
    if (hipMemset(h->sk_bins, 0, 4 * ORDER_BINS * sizeof(int32_t)) != hipSuccess) {
        phgpu_destroy(h);
        return set_err(-2, "hipMemset failed");
    }
    if (h->shared) {
        // one scaled matrix; iterates and per-scenario data live in the stream records
        // (allocated by phgpu_set_scenarios once the per-scenario column set is known)
        ALLOC(h->A, nnz);
        ALLOC(h->Ah_csr, nnz);
        ALLOC(h->Ah_csc, nnz);
        ALLOC(h->Dr, m);
        ALLOC(h->Dc, n);
        ALLOC(h->cmap, n);
        ALLOC(h->rmap, m);
        ALLOC(h->sh_col, 4 * (size_t)n);
        ALLOC(h->sh_row, 4 * (size_t)m);
        ALLOC(h->sh_norm, 4);
        ALLOC(h->sh_v, n);
        ALLOC(h->sh_u, n);
        ALLOC(h->sh_w, m);
        ALLOC(h->sh_part, (size_t)(n + 255) / 256 + 1);
    } else {
        ALLOC(h->A, (size_t)nnz * Sz);
        ALLOC(h->c, (size_t)n * Sz);
        ALLOC(h->lb, (size_t)n * Sz);
        ALLOC(h->ub, (size_t)n * Sz);
        ALLOC(h->q, (size_t)n * Sz);
        ALLOC(h->rl, (size_t)m * Sz);
        ALLOC(h->ru, (size_t)m * Sz);
        ALLOC(h->Ah_csr, (size_t)nnz * Sz);
        ALLOC(h->Ah_csc, (size_t)nnz * Sz);
        ALLOC(h->Dr, (size_t)m * Sz);
        ALLOC(h->Dc, (size_t)n * Sz);
        ALLOC(h->normA, Sz);
        ALLOC(h->lbh, (size_t)n * Sz);
        ALLOC(h->ubh, (size_t)n * Sz);
        ALLOC(h->rlh, (size_t)m * Sz);
        ALLOC(h->ruh, (size_t)m * Sz);
        ALLOC(h->ch, (size_t)n * Sz);
        ALLOC(h->qh, (size_t)n * Sz);
        ALLOC(h->x, (size_t)n * Sz);
        ALLOC(h->x0, (size_t)n * Sz);
        ALLOC(h->xe, (size_t)n * Sz);
        ALLOC(h->xt, (size_t)n * Sz);
        ALLOC(h->aty, (size_t)n * Sz);
        ALLOC(h->aty0, (size_t)n * Sz);
        ALLOC(h->y, (size_t)m * Sz);
        ALLOC(h->y0, (size_t)m * Sz);
        ALLOC(h->yt, (size_t)m * Sz);
    }
    ALLOC(h->qhead, 1);
    ALLOC(h->stats_gen, 8);
    if (!h->shared) {  // path 6: the pattern's factor size, the fallback list and its counters
        h->ipm_nf = ipm_nf_bound(n, m, row_ptr, col_idx);
        if (!(h->ipm_nf > 0 && h->ipm_nf <= IPM_MAX_NF && n <= JIT_MAX_N && m <= JIT_MAX_M && nnz <= JIT_MAX_NNZ))
            h->ipm_wave = ipm_wg_bound(n, m, nnz, row_ptr, col_idx);
        if (h->ipm_nf > 0 || h->ipm_wave > 0) {
            ALLOC(h->ipm_list, Sz);
            ALLOC(h->ipm_cnt, 6);
            ALLOC(h->ipm_stats, 2 * PHGPU_STATS_WORDS);
            if (getenv("PHGPU_IPM_PROF")) {  // diagnostics: 16 words per wave of the widest plan
                h->ipm_prof_n = 16 * ((Sz * 64 + 63) / 64 + 64);
                ALLOC(h->ipm_prof, h->ipm_prof_n);
            }
            if (hipMemset(h->ipm_cnt, 0, 6 * sizeof(int32_t)) != hipSuccess ||
                hipMemset(h->ipm_stats, 0, 2 * PHGPU_STATS_WORDS * sizeof(unsigned long long)) != hipSuccess) {
                phgpu_destroy(h);
                return set_err(-2, "hipMemset failed");
            }
        }
    }
    // warm-start slots: slot 0 is the arrays above; slot 1 (deferred solves, paths 1-3)
    h->xs[0] = h->x;
    h->ys[0] = h->y;
    h->oms[0] = h->omega;
    h->its_s[0] = h->sk_iters;
    if (h->shared) {  // path 4 solves are never deferred: both slots are slot 0
        h->xs[1] = h->x;
        h->ys[1] = h->y;
        h->oms[1] = h->omega;
        h->its_s[1] = h->sk_iters;
    } else {
        ALLOC(h->xs[1], (size_t)n * Sz);
        ALLOC(h->ys[1], (size_t)m * Sz);
        ALLOC(h->oms[1], Sz);
        ALLOC(h->its_s[1], Sz);
    }
    h->pending = -1;
    bind_slots(h);
    {
        int ncu = 0;
        if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || ncu < 1)
            ncu = 256;
        h->num_cus = ncu;
    }
    {
        // per-wave partials [nwaves * K] + the conv partials of phgpu_ph_step_local [nwaves]
        size_t K = (size_t)(2 * nn > 5 ? 2 * nn : 5);
        ALLOC(h->part, (size_t)h->nwaves * (K + 1));
        ALLOC(h->part_node, (size_t)h->nwaves * (nn > 0 ? nn : 1));
        // path-6 epilogue partials (two slots) and the update kernels' conv partials (one
        // per block of the widest update grid: 64 lanes per block at least)
        if (!h->shared && h->ipm_nf > 0 && nn > 0 && nn <= XL_NN_MAX) {
            const size_t nch = (Sz + XP_CHUNK_MIN - 1) / XP_CHUNK_MIN;
            for (int k = 0; k < 2; ++k) {
                ALLOC(h->xp[k], nch * 2 * (size_t)nn);
                ALLOC(h->xp_node[k], nch * (size_t)nn);
                ALLOC(h->xp_dirty[k], nch);
            }
        }
        // one per block of the widest grid (path-6 lane groups of 16; k_ph_update's nonant x
        // scenario-block grid)
        ALLOC(h->cpart_blk, std::max<size_t>((Sz + 15) / 16 + 1, (size_t)std::max(nn, 1) * ((Sz + UPD_T - 1) / UPD_T) + 1));
        ALLOC(h->blk_cnt, 4);
        if (hipMemset(h->blk_cnt, 0, 4 * sizeof(int32_t)) != hipSuccess) {
            phgpu_destroy(h);
            return set_err(-2, "hipMemset failed");
        }
    }
    hipError_t e = hipSuccess;
    e = hipMemcpy(h->row_ptr, row_ptr, (m + 1) * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess && nnz) e = hipMemcpy(h->col_idx, col_idx, nnz * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(h->col_ptr, cptr.data(), (n + 1) * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess && nnz) e = hipMemcpy(h->row_idx, ridx.data(), nnz * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess && nnz) e = hipMemcpy(h->perm, perm.data(), nnz * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess && nnz) e = hipMemcpy(h->row_of, rowof.data(), nnz * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess && nn) e = hipMemcpy(h->nonant_col, nonant_col, nn * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess && nn) e = hipMemcpy(h->nonant_depth, nonant_depth, nn * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess && nn) e = hipMemcpy(h->nonant_off, nonant_off, nn * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(h->nonant_slot, slot.data(), n * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        phgpu_destroy(h);
        return set_err(-2, "pattern upload failed: %s", hipGetErrorString(e));
    }
    h->reg_inst = -1;
    h->wg_inst = -1;
    long best = 0;
    int rcp = 0;
    if (h->shared) {
        rcp = build_sell(h, row_ptr, col_idx);
        h->default_kernel = 4;
    } else {
        rcp = reg_plan_select(h, row_ptr, col_idx);
        if (!rcp) rcp = wg_plan_select(h, row_ptr, col_idx, &best);
    }
    if (!rcp && !h->shared) {
        // default path: the cheaper per scenario (register path at its chosen L)
        long reg_cost_s = -1;
        if (h->reg_inst >= 0) {
            const reg_instance& r = g_reg_instances[h->reg_inst];
            reg_cost_s = (long)h->reg_L * slot_cost(r.KC, r.ZC, r.KR, r.ZR, 0) / WAVE;
        }
        if (h->reg_inst >= 0 && (h->wg_inst < 0 || reg_cost_s <= best)) h->default_kernel = 2;
        else if (h->wg_inst >= 0) h->default_kernel = 3;
        else h->default_kernel = 1;
        if (h->default_kernel == 3) rcp = pack_alloc(h);
    }
    if (rcp) {
        phgpu_destroy(h);
        return rcp;
    }
    *out = h;
    return 0;
}

static inline dim3 grid_for(int64_t S) { return dim3((unsigned)((S + BLOCK - 1) / BLOCK)); }

// phgpu_set_scenarios on a shared-matrix handle: A_val holds nnz values (one copy for
// all scenarios).  Scales A once, finds the columns / rows whose data differ between
// scenarios (plus every nonant column), sizes the stream records and fills them.  Sizing
// the records needs those counts on the host: this call synchronises the stream once.
static int set_scenarios_shared(phgpu_state* h, const double* A_val, const double* c, const double* lb,
                                const double* ub, const double* rl, const double* ru, const double* q,
                                const double* obj_const, const double* prob, const int32_t* node_of,
                                const double* prob_coeff, hipStream_t st) {
    const size_t Sz = (size_t)h->S;
    const int n = h->n, m = h->m, nnz = h->nnz;
    auto cp = [&](double* dst, const double* src, size_t cnt) -> hipError_t {
        if (cnt == 0) return hipSuccess;
        return hipMemcpyAsync(dst, src, cnt * sizeof(double), hipMemcpyDeviceToDevice, st);
    };
    HIPCHK(cp(h->A, A_val, (size_t)nnz));
    if (obj_const) HIPCHK(cp(h->objc, obj_const, Sz));
    else HIPCHK(hipMemsetAsync(h->objc, 0, Sz * sizeof(double), st));
    HIPCHK(cp(h->prob, prob, Sz));
    HIPCHK(cp(h->pcoef, prob_coeff, (size_t)h->depth * Sz));
    HIPCHK(hipMemcpyAsync(h->node_of, node_of, (size_t)h->depth * Sz * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    h->xbar_mixed = -1;
    h->fx_valid = 0;
    dfree(h, &h->nb_idx);
    const int big = std::max(nnz, std::max(n, m));
    const dim3 gb((unsigned)((big + 255) / 256)), gn((unsigned)((n + 255) / 256)), gm((unsigned)((m + 255) / 256));
    const dim3 gz((unsigned)((nnz + 255) / 256 > 0 ? (nnz + 255) / 256 : 1));
    // Ruiz (10 max passes) + Pock-Chambolle (sum) pass, as k_setup
    hipLaunchKernelGGL(k_sh_init, gb, dim3(256), 0, st, *h);
    for (int pass = 0; pass <= 10; ++pass) {
        const int pc = pass == 10;
        if (m) hipLaunchKernelGGL(k_sh_rowfac, gm, dim3(256), 0, st, *h, pc, h->sh_w);
        hipLaunchKernelGGL(k_sh_colfac, gn, dim3(256), 0, st, *h, pc, h->sh_u);
        hipLaunchKernelGGL(k_sh_apply, gb, dim3(256), 0, st, *h, (const double*)h->sh_w, (const double*)h->sh_u);
    }
    hipLaunchKernelGGL(k_sh_csc, gz, dim3(256), 0, st, *h);
    {
        const int tot_c = h->nent_c, tot_r = h->nent_r;
        if (tot_c) hipLaunchKernelGGL(k_sh_sell_vals, dim3((unsigned)((tot_c + 255) / 256)), dim3(256), 0, st,
                                      (const int32_t*)h->cs_src, (const double*)h->Ah_csc, tot_c, h->cs_val);
        if (tot_r) hipLaunchKernelGGL(k_sh_sell_vals, dim3((unsigned)((tot_r + 255) / 256)), dim3(256), 0, st,
                                      (const int32_t*)h->rs_src, (const double*)h->Ah_csr, tot_r, h->rs_val);
    }
    // ||A_scaled||_2: 200 power iterations on A^T A
    hipLaunchKernelGGL(k_sh_vinit, gn, dim3(256), 0, st, *h, h->sh_v);
    for (int it = 0; it < 200; ++it) {
        if (m) hipLaunchKernelGGL(k_sh_rowmv, gm, dim3(256), 0, st, *h, (const double*)h->sh_v, h->sh_w);
        hipLaunchKernelGGL(k_sh_colmv, gn, dim3(256), 0, st, *h, (const double*)h->sh_w, h->sh_u, h->sh_part);
        hipLaunchKernelGGL(k_sh_norm, dim3(1), dim3(256), 0, st, (const double*)h->sh_part, (int)gn.x, h->sh_norm + 3);
        hipLaunchKernelGGL(k_sh_normalize, gn, dim3(256), 0, st, *h, (const double*)h->sh_u,
                           (const double*)(h->sh_norm + 3), h->sh_v);
    }
    hipLaunchKernelGGL(k_sh_finish_norm, dim3(1), dim3(1), 0, st, *h);
    hipLaunchKernelGGL(k_sh_base, gb, dim3(256), 0, st, *h, c, q, lb, ub, rl, ru);
    HIPCHK(hipGetLastError());
    // which columns / rows differ between scenarios (one wave per entry)
    dev_tmp<int32_t> flags;
    HIPCHK(flags.alloc((size_t)(n + m + 1)));
    hipLaunchKernelGGL(k_sh_vary, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, c, q, lb, ub, n, h->S, flags.p);
    if (m) hipLaunchKernelGGL(k_sh_vary, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, st, rl, ru, (const double*)nullptr,
                              (const double*)nullptr, m, h->S, flags.p + n);
    HIPCHK(hipGetLastError());
    std::vector<int32_t> fl((size_t)n + m + 1, 0), slot((size_t)n, -1);
    HIPCHK(hipMemcpyAsync(fl.data(), flags.p, (size_t)(n + m) * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(slot.data(), h->nonant_slot, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    flags.release();
    std::vector<int32_t> cmap((size_t)n, -1), rmap((size_t)m + 1, -1), pcol, prow;
    for (int j = 0; j < n; ++j)
        if (fl[j] || slot[j] >= 0) {
            cmap[j] = (int32_t)pcol.size();
            pcol.push_back(j);
        }
    for (int i = 0; i < m; ++i)
        if (fl[(size_t)n + i]) {
            rmap[i] = (int32_t)prow.size();
            prow.push_back(i);
        }
    h->np = (int)pcol.size();
    h->nr = (int)prow.size();
    dfree(h, &h->pcol);
    dfree(h, &h->prow);
    if (dalloc(h, &h->pcol, pcol.size()) || dalloc(h, &h->prow, prow.size())) return -3;
    HIPCHK(hipMemcpy(h->cmap, cmap.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
    if (m) HIPCHK(hipMemcpy(h->rmap, rmap.data(), (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice));
    if (!pcol.empty()) HIPCHK(hipMemcpy(h->pcol, pcol.data(), pcol.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    if (!prow.empty()) HIPCHK(hipMemcpy(h->prow, prow.data(), prow.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    // record layout, every part aligned to 16 doubles (128 B)
    auto al = [](int64_t v) { return (v + 15) / 16 * 16; };
    int64_t o = 0;
    h->sk_X = o; o += al(n);
    h->sk_X0 = o; o += al(n);
    h->sk_U = o; o += al(n);
    h->sk_XT = o; o += al(n);
    h->sk_Y = o; o += al(m);
    h->sk_Y0 = o; o += al(m);
    h->sk_YT = o; o += al(m);
    h->sk_PC = o; o += al(8 * (int64_t)h->np);
    h->sk_PR = o; o += al(4 * (int64_t)h->nr);
    h->sk_stride = o;
    const int64_t need = o * h->S;
    if (need > h->sk_cap) {
        dfree(h, &h->sk);
        h->sk_cap = 0;
        const int rc = dalloc(h, &h->sk, (size_t)need);
        if (rc) return rc;
        h->sk_cap = need;
    }
    const int64_t per = (int64_t)h->np + h->nr;
    if (per > 0) {
        const int64_t tot = per * h->S;
        hipLaunchKernelGGL(k_sh_fill, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, *h, c, q, lb, ub, rl, ru);
    }
    hipLaunchKernelGGL(k_sh_normbase, dim3(1), dim3(256), 0, st, *h, c, rl, ru);
    hipLaunchKernelGGL(k_sh_fill_omega, dim3((unsigned)((h->S + 255) / 256)), dim3(256), 0, st, *h);
    HIPCHK(hipGetLastError());
    h->wslot = h->wq = 0;
    h->pending = -1;
    h->have_s[0] = h->have_s[1] = 0;
    h->warm_rec_s[0] = h->warm_rec_s[1] = 0;
    bind_slots(h);
    h->scen_set = 1;
    h->last_path = 0;
    return 0;
}

extern "C" int phgpu_set_scenarios(phgpu_handle h, const double* A_val, const double* c,
                                   const double* lb, const double* ub, const double* rl,
                                   const double* ru, const double* q, const double* obj_const,
                                   const double* prob, const int32_t* node_of,
                                   const double* prob_coeff, void* stream) {
    FLUSH_STEP(h);
    if (!h) return set_err(-1, "null handle");
    if ((h->nnz && !A_val) || !c || !lb || !ub || (h->m && (!rl || !ru)) || !prob || !node_of || !prob_coeff)
        return set_err(-1, "null scenario array");
    hipStream_t st = (hipStream_t)stream;
    if (h->shared) return set_scenarios_shared(h, A_val, c, lb, ub, rl, ru, q, obj_const, prob, node_of, prob_coeff, st);
    const size_t Sz = (size_t)h->S;
    auto cp = [&](double* dst, const double* src, size_t cnt) -> hipError_t {
        if (cnt == 0) return hipSuccess;
        return hipMemcpyAsync(dst, src, cnt * sizeof(double), hipMemcpyDeviceToDevice, st);
    };
    HIPCHK(cp(h->A, A_val, (size_t)h->nnz * Sz));
    HIPCHK(cp(h->c, c, (size_t)h->n * Sz));
    HIPCHK(cp(h->lb, lb, (size_t)h->n * Sz));
    HIPCHK(cp(h->ub, ub, (size_t)h->n * Sz));
    HIPCHK(cp(h->rl, rl, (size_t)h->m * Sz));
    HIPCHK(cp(h->ru, ru, (size_t)h->m * Sz));
    if (q) HIPCHK(cp(h->q, q, (size_t)h->n * Sz));
    else HIPCHK(hipMemsetAsync(h->q, 0, (size_t)h->n * Sz * sizeof(double), st));
    if (obj_const) HIPCHK(cp(h->objc, obj_const, Sz));
    else HIPCHK(hipMemsetAsync(h->objc, 0, Sz * sizeof(double), st));
    HIPCHK(cp(h->prob, prob, Sz));
    HIPCHK(cp(h->pcoef, prob_coeff, (size_t)h->depth * Sz));
    HIPCHK(hipMemcpyAsync(h->node_of, node_of, (size_t)h->depth * Sz * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    h->xbar_mixed = -1;
    h->fx_valid = 0;
    dfree(h, &h->nb_idx);
    h->wslot = h->wq = 0;
    h->pending = -1;
    h->have_s[0] = h->have_s[1] = 0;
    h->warm_rec_s[0] = h->warm_rec_s[1] = 0;
    h->jit_kinds_valid = 0;
    // new data: the path-6 module is specialised again at the next solve (and a spill or a
    // failed compile of the previous data no longer decides the path)
    h->ipm_flags_valid = 0;
    h->ipm_off = 0;
    h->ipm_spill1 = 0;
    h->ipm_lds = 0;
    bind_slots(h);
    HIPCHK(run_setup(h, st));
    // the setup's start omega (slot 0) for slot 1 too
    HIPCHK(hipMemcpyAsync(h->oms[1], h->oms[0], (size_t)h->S * sizeof(double), hipMemcpyDeviceToDevice, st));
    if (h->pk) HIPCHK(pack_fill(h, st));
    h->scen_set = 1;
    h->last_path = 0;
    return 0;
}

extern "C" int phgpu_set_nonant_probs(phgpu_handle h, const double* pvar) {
    FLUSH_STEP(h);
    if (!h) return set_err(-1, "null handle");
    const double* nv = h->nn > 0 ? pvar : nullptr;
    // the path-6 epilogue partials of both slots were weighted with the per-node prob_coeff
    // (or the previous pvar, whose values the caller may have rewritten in place): a later
    // phgpu_ph_reduce must not take them for this x
    h->xp_C[0] = h->xp_C[1] = 0;
    h->pvar = nv;
    return 0;
}

extern "C" int phgpu_set_ph_state(phgpu_handle h, const double* W, const double* rho,
                                  const double* xbar, int W_on, int prox_on) {
    FLUSH_STEP(h);
    if (!h) return set_err(-1, "null handle");
    if (h->nn > 0 && ((W_on && !W) || (prox_on && (!rho || !xbar))))
        return set_err(-1, "W / rho / xbar pointer missing for the requested terms");
    h->W = W;
    h->rho = rho;
    h->xbar = xbar;
    h->W_on = W_on ? 1 : 0;
    h->prox_on = prox_on ? 1 : 0;
    return 0;
}

static int solve_impl(phgpu_handle h, const phgpu_options* opt, int warm_start, int defer, double* x, double* y,
                      double* obj, double* bound, int32_t* status, int32_t* iters, void* stream);

extern "C" int phgpu_solve(phgpu_handle h, const phgpu_options* opt, int warm_start, double* x,
                           double* y, double* obj, double* bound, int32_t* status,
                           int32_t* iters, void* stream) {
    return solve_impl(h, opt, warm_start, 0, x, y, obj, bound, status, iters, stream);
}

extern "C" int phgpu_solve_deferred(phgpu_handle h, const phgpu_options* opt, int warm_start, double* x,
                                    double* y, double* obj, double* bound, int32_t* status,
                                    int32_t* iters, void* stream) {
    return solve_impl(h, opt, warm_start, 1, x, y, obj, bound, status, iters, stream);
}

extern "C" int phgpu_commit(phgpu_handle h) {
    if (!h) return set_err(-1, "null handle");
    if (h->pending >= 0) {
        h->wslot = h->wq = h->pending;
        h->pending = -1;
        bind_slots(h);
    }
    return 0;
}

// the path phgpu_solve takes for kernel 0 (gamma = 1): the interior-point kernel (path 6)
// where it applies (PHGPU_IPM=0 turns it off, a module that spills takes it out), then
// the pattern-specialised PDHG kernel (path 5) when PHGPU_JIT asks for it, else the path
// chosen at phgpu_create
static int default_path(const phgpu_state* h) {
    const char* ie = getenv("PHGPU_IPM");
    if (ipm_eligible(h) && !h->ipm_off && !(ie && atoi(ie) == 0)) return 6;
    const char* env = getenv("PHGPU_JIT");
    if (env && atoi(env) == 0) return h->default_kernel;
    if (jit_eligible(h) && (env || h->S >= JIT_MIN_S)) return 5;
    return h->default_kernel;
}

#include "solve_launch.inc"

// the options of a solve (null: the defaults), checked
static int solve_options(const phgpu_options* opt, phgpu_options& o) {
    if (opt) o = *opt;
    else phgpu_default_options(&o);
    if (o.check_every < 1 || o.max_iter < 1 || !(o.eta_frac > 0.0 && o.eta_frac < 1.0) ||
        o.gamma < 0.0 || o.gamma > 1.0 || o.restart_every < 1 || o.check_every % o.restart_every != 0 ||
        o.max_iter % o.restart_every != 0 || !(o.eps_infeas > 0.0))
        return set_err(-1, "bad options (check_every=%d restart_every=%d max_iter=%d eta_frac=%g gamma=%g "
                       "eps_infeas=%g; check_every and max_iter must be multiples of restart_every)",
                       o.check_every, o.restart_every, o.max_iter, o.eta_frac, o.gamma, o.eps_infeas);
    return 0;
}

static int solve_impl(phgpu_handle h, const phgpu_options* opt, int warm_start, int defer, double* x, double* y,
                      double* obj, double* bound, int32_t* status, int32_t* iters, void* stream) {
    if (!h) return set_err(-1, "null handle");
    if (!x || !obj || !bound || !status) return set_err(-1, "null output pointer");
    if (defer && h->shared)
        return set_err(-1, "phgpu_solve_deferred: a shared-matrix handle (path 4) keeps one warm-start slot");
    // read the committed slot; write it in place, or the other slot for a deferred solve
    // (an uncommitted deferred solve is dropped by this one)
    h->pending = -1;
    h->wq = defer ? 1 - h->wslot : h->wslot;
    bind_slots(h);
    phgpu_options o;
    {
        const int orc = solve_options(opt, o);
        if (orc) return orc;
    }
    const solve_params P = make_solve_params(o, (warm_start && h->have_solution) ? 1 : 0);
    hipStream_t st = (hipStream_t)stream;
    // the register-resident kernels are specialised for the reflected step (gamma = 1, the
    // default); another gamma runs on the global-memory kernel
    if (o.kernel < 0 || o.kernel > 6) return set_err(-1, "bad kernel option %d", o.kernel);
    if (h->shared != (o.kernel == 4 || (o.kernel == 0 && h->shared)))
        return set_err(-1, "kernel option %d: a shared-matrix handle solves with path 4 only (kernel 0 or 4), "
                       "other handles with paths 1-3, 5 and 6", o.kernel);
    if (h->shared) {
        if (!h->scen_set) return set_err(-1, "phgpu_set_scenarios has not been called");
        const int rc4 = launch_stream(h, P, x, y, obj, bound, status, iters, st, o.split_longest);
        if (rc4) return rc4;
        h->last_stats = nullptr;
        solve_done(h, 4, 0, 0, status, iters);
        return 0;
    }
    if (o.kernel == 2 && h->reg_inst < 0)
        return set_err(-1, "register-resident kernel requested but no compiled instance fits this pattern");
    if (o.kernel == 3 && h->wg_inst < 0)
        return set_err(-1, "workgroup-per-scenario kernel requested but no compiled instance fits this pattern");
    if ((o.kernel == 2 || o.kernel == 3 || o.kernel == 5) && o.gamma != 1.0)
        return set_err(-1, "register-resident kernels require gamma = 1 (got %g)", o.gamma);
    if (o.kernel == 5 && !jit_eligible(h))
        return set_err(-1, "kernel 5 (pattern-specialised) needs n <= %d, m <= %d, nnz <= %d (got %d, %d, %d)",
                       JIT_MAX_N, JIT_MAX_M, JIT_MAX_NNZ, h->n, h->m, h->nnz);
    if (o.kernel == 6 && !ipm_eligible(h))
        return set_err(-1, "kernel 6 (interior point) needs n <= %d, m <= %d, nnz <= %d and <= %d factor entries "
                       "(got %d, %d, %d, %d)", IPM_MAX_N, IPM_MAX_M, IPM_MAX_NNZ, IPM_MAX_NF, h->n, h->m, h->nnz,
                       h->ipm_nf);
    int path = o.kernel != 0 ? o.kernel : (o.gamma == 1.0 ? default_path(h) : 1);
    // the statistics / status buffers phgpu_solve_stats and phgpu_ph_update_ex read: this
    // solve's, once it is launched (a rejected solve leaves the previous ones)
    unsigned long long* stats_keep = h->last_stats;
    h->last_stats = nullptr;  // path 6 sets it when its kernels produce the statistics
    if (path == 6) {
        const int rc6 = ipm_prepare(h, st);
        if (rc6) {
            h->last_stats = stats_keep;
            if (o.kernel != 0) return rc6;
            // the automatic choice: a module that does not compile or load (a hipRTC runtime
            // problem, an unusual pattern) turns path 6 off for this handle's data and the
            // solve runs on the handle's PDHG path; phgpu_last_error keeps the reason and
            // phgpu_ipm_info reports it (off = 2)
            h->ipm_off = 2;
            fprintf(stderr, "phgpu: path 6 unavailable (%s); solving on the PDHG path\n", g_err);
            path = default_path(h);
        } else if (o.kernel == 0 && h->ipm->private_bytes > ipm_spill_max()) {
            h->ipm_off = 1;  // the automatic choice falls back to the handle's PDHG path
            path = default_path(h);
        }
    }
    // a deferred one-rank PH step (phgpu_ph_step_defer): folded into this launch's prologue
    // when it is a path-6 deferred solve that writes other buffers than the step reads and
    // the previous solve's partials / statistics are path 6's; else run now
    h->fuse_now = 0;
    if (h->pend.active) {
        const phgpu_state::ph_pending& q = h->pend;
        const char* fe = getenv("PHGPU_FUSE_STEP");
        // (the one-lane kernel only: folded into the lane-group kernel the step measured
        // slower, 8,192 scenarios 0.095 ms per PH iteration against 0.079 as its own launch,
        // profiles/r04/o/; PHGPU_FUSE_STEP=1 folds there too)
        const bool fuse = path == 6 && defer && !(fe && atoi(fe) == 0) && q.stream == st && q.x != x &&
                          // (the workgroup kernels, L >= 64, carry no folded step at all)
                          (h->ipm && (h->ipm->L == 1 || (fe && atoi(fe) == 1 && h->ipm->L < 64))) &&
                          h->nb_idx && h->xbar_single && h->xbar_mixed == 0 && h->nn > 0 && h->nn <= XL_NN_MAX &&
                          xp_valid(h, q.x) && q.W == h->W && q.xbar == h->xbar && q.rho == h->rho &&
                          (!q.stats || (stats_keep && stats_keep == h->ipm_stats + PHGPU_STATS_WORDS * (1 - h->ipm_parity)));
        if (fuse) {
            h->fuse_now = 1;
            ++h->folded;
        }
        else {
            // (the step's statistics are the previous solve's: its in-kernel ones if any)
            h->last_stats = stats_keep;
            const int frc = flush_step(h);
            h->last_stats = nullptr;
            if (frc) return frc;
        }
    }
    int rc = 0;
    if (path == 3) rc = launch_wg(h, P, x, y, obj, bound, status, iters, st);
    else if (path == 2) rc = launch_reg(h, P, x, y, obj, bound, status, iters, st);
    else {
        rc = warm_from_records(h, P, st);
        if (!rc && path == 5) rc = jit_prepare(h, st);
        if (rc) return rc;
        if (path == 5) rc = jit_launch(h, P, x, y, obj, bound, status, iters, st);
        else if (path == 6) rc = ipm_launch(h, P, x, y, obj, bound, status, iters, st);
        else rc = launch_global(h, P, x, y, obj, bound, status, iters, st);
    }
    if (rc) return rc;
    HIPCHK(hipGetLastError());
    // the warm state this solve wrote lives in the records on path 3 and in path 2's record mode
    solve_done(h, path, path == 3 || (path == 2 && h->last_rec == 1), defer, status, iters);
    return 0;
}

// Once per scenario data: does any wave span two nodes (xbar_mixed), is every nonant on one
// node (xbar_single), and the node_buf index of each nonant for the folded PH step (nb_idx)
static int xbar_layout(phgpu_state* h, hipStream_t st) {
    if (h->xbar_mixed >= 0) return 0;
    dev_tmp<int32_t> d;
    int32_t v[2] = {0, 0};
    HIPCHK(d.alloc(2));
    HIPCHK(hipMemsetAsync(d.p, 0, 2 * sizeof(int32_t), st));
    hipLaunchKernelGGL(k_xbar_mixed, grid_for(h->S), dim3(BLOCK), 0, st, *h, d.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(v, d.p, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    d.release();
    h->xbar_mixed = v[0] ? 1 : 0;
    h->xbar_single = v[1] ? 0 : 1;
    if (h->xbar_single && h->nn > 0 && h->nn <= XL_NN_MAX && !h->nb_idx) {
        // node_buf index of each nonant (its one node, offset) for the folded PH step
        std::vector<int32_t> dep(h->nn), off(h->nn), idx(h->nn);
        HIPCHK(hipMemcpy(dep.data(), h->nonant_depth, h->nn * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(off.data(), h->nonant_off, h->nn * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (int k = 0; k < h->nn; ++k) {
            int32_t g = 0;
            HIPCHK(hipMemcpy(&g, h->node_of + (size_t)dep[k] * h->S, sizeof(int32_t), hipMemcpyDeviceToHost));
            idx[k] = g * h->nlen_max + off[k];
        }
        // (uncounted, as split_part, loop_dbl and loop_cnt: not part of phgpu_workspace_bytes)
        const int rc = dalloc(h, &h->nb_idx, (size_t)h->nn, false);
        if (rc) return rc;
        HIPCHK(hipMemcpy(h->nb_idx, idx.data(), h->nn * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    return 0;
}

// The PH loop of one rank in one cooperative launch (include/phgpu.h, solve_ipm.inc's
// IPM_LOOP module)
extern "C" int phgpu_ph_loop(phgpu_handle h, const phgpu_options* opt, int max_iters, double convthresh,
                             double* x, double* y, double* obj, double* bound, int32_t* status, int32_t* iters,
                             double* node_buf, double* conv_hist, int64_t* out, void* stream) {
    if (!h || !x || !obj || !bound || !status || !node_buf || !conv_hist || !out) return set_err(-1, "null argument");
    if (max_iters < 1) return set_err(-1, "phgpu_ph_loop: max_iters must be >= 1");
    FLUSH_STEP(h);
    hipStream_t st = (hipStream_t)stream;
    {
        const int rc = xbar_layout(h, st);  // (known after the first phgpu_ph_reduce otherwise)
        if (rc) return rc;
    }
    const int why = ph_loop_eligible(h);
    if (why) return set_err(-3, "phgpu_ph_loop: not eligible (reason %d); run the PH steps one by one", why);
    phgpu_options o;
    if (opt) o = *opt;
    else phgpu_default_options(&o);
    if (o.kernel != 0 && o.kernel != 6) return set_err(-3, "phgpu_ph_loop: path 6 only");
    {
        const int rc = ipm_prepare(h, st);
        if (rc) return rc;
    }
    if (h->ipm->L != 1 || h->ipm->private_bytes > ipm_spill_max()) return set_err(-3, "phgpu_ph_loop: no one-lane module");
    {
        const int rc = ipm_loop_prepare(h);
        if (rc) return rc;
    }
    ipm_module* im = h->ipm_loop;
    const int64_t nblk = (h->S + 255) / 256;
    if ((int64_t)std::max(im->per_cu_ipm, 0) * h->num_cus < nblk)
        return set_err(-3, "phgpu_ph_loop: %lld workgroups do not fit the GPU at once", (long long)nblk);
    // buffers
    const int64_t nd = nblk * 16 + 16 + max_iters;
    if (h->loop_dbl_n < nd) {
        dfree(h, &h->loop_dbl);
        h->loop_dbl_n = 0;
        const int rc = dalloc(h, &h->loop_dbl, (size_t)nd, false);
        if (rc) return rc;
        h->loop_dbl_n = nd;
    }
    if (!h->loop_cnt) {
        const int rc = dalloc(h, &h->loop_cnt, (size_t)(2 + PHGPU_STATS_WORDS), false);
        if (rc) return rc;
    }
    HIPCHK(hipMemsetAsync(h->loop_cnt, 0, (size_t)(2 + PHGPU_STATS_WORDS) * sizeof(unsigned long long), st));
    // a plain (non-deferred) solve's slot bookkeeping (solve_impl)
    h->pending = -1;
    h->wq = h->wslot;
    bind_slots(h);
    const int wq = h->wq;
    const solve_params P = make_solve_params(o, h->have_solution ? 1 : 0);  // (options not validated here)
    const int par = h->ipm_parity;
    h->ipm_parity ^= 1;
    ipm_params a{};
    ipm_fill_args(h, P, par, x, y, obj, bound, status, iters, a);
    a.prof = nullptr;
    a.xp = nullptr;  // (no epilogue partials: the loop ends on its own PH state)
    a.xp_node = h->xp_node[wq];
    a.xp_dirty = h->xp_dirty[wq];
    a.pcoef = h->pcoef;
    a.node_of = h->node_of;
    a.xprev = x;
    a.W_w = const_cast<double*>(h->W);
    a.xbar_w = const_cast<double*>(h->xbar);
    a.node_buf = node_buf;
    a.nb_idx = h->nb_idx;
    a.nb_half = (long long)h->num_nodes * h->nlen_max;
    a.gpart = h->loop_dbl;
    a.gpub = h->loop_dbl + nblk * 16;
    a.conv_hist = h->loop_dbl + nblk * 16 + 16;
    a.gsync = (unsigned*)h->loop_cnt;
    a.loop_out = (int*)(h->loop_cnt + 1);
    a.loop_its = h->loop_cnt + 2;
    a.conv_scale = 1.0 / ((double)h->S * (double)h->nn);
    a.convthresh = convthresh;
    a.loop_K = max_iters;
    h->xp_C[wq] = 0;
    void* args[] = {&a};
    HIPCHK(hipModuleLaunchCooperativeKernel(im->fn_ipm, (unsigned)nblk, 1, 1, 256, 1, 1, 0, st, args));
    {
        const int rc = ipm_fallback_launch(h, im, P, x, y, obj, bound, status, iters, a.fail_n + 1, a.fail_n, a.stats, st);
        if (rc) return rc;
    }
    HIPCHK(hipGetLastError());
    solve_done(h, 6, 0, 0, status, iters);
    // the loop's record (one synchronisation: the loop is one call of the host's PH loop)
    std::vector<unsigned long long> cnt((size_t)(2 + PHGPU_STATS_WORDS));
    HIPCHK(hipMemcpyAsync(cnt.data(), h->loop_cnt, cnt.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(conv_hist, a.conv_hist, (size_t)max_iters * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const int* lo = (const int*)(cnt.data() + 1);
    out[0] = lo[0];
    out[1] = lo[1];
    out[2] = (int64_t)stats_word(cnt.data() + 2, PHGPU_STATS_COPIES, 0);
    out[3] = 0;
    if (lo[1] == 3) return set_err(-2, "phgpu_ph_loop: a grid step timed out (the launch was not co-resident)");
    return 0;
}

// counts[c] = number of local scenarios with status c (c = 0..3), one block
// counts[k] = #{s : status[s] == k}: one block, four statuses per load, several loads in
// flight per thread (a device-wide "last block" reduction needs a release fence, i.e. an
// L2 writeback of every XCD, which costs more than the whole count)
#define SC_T 1024
__global__ void __launch_bounds__(SC_T) k_status_counts(const int32_t* __restrict__ status, int64_t S,
                                                        int32_t* __restrict__ counts) {
    __shared__ int32_t c[4];
    if (threadIdx.x < 4) c[threadIdx.x] = 0;
    __syncthreads();
    int32_t loc[4] = {0, 0, 0, 0};
    // (a macro, not a lambda: a by-reference capture of loc[] would put it in scratch)
#define SC_ADD(v) loc[0] += (v) == 0, loc[1] += (v) == 1, loc[2] += (v) == 2, loc[3] += (v) == 3
    const int64_t S4 = ((uintptr_t)status % 16 == 0) ? S / 4 : 0;  // int4 part
    const int4* s4 = (const int4*)status;
    int64_t i = threadIdx.x;
    for (; i + 3 * SC_T < S4; i += 4 * SC_T) {
        const int4 a = s4[i], b = s4[i + SC_T], d = s4[i + 2 * SC_T], e = s4[i + 3 * SC_T];
        SC_ADD(a.x); SC_ADD(a.y); SC_ADD(a.z); SC_ADD(a.w);
        SC_ADD(b.x); SC_ADD(b.y); SC_ADD(b.z); SC_ADD(b.w);
        SC_ADD(d.x); SC_ADD(d.y); SC_ADD(d.z); SC_ADD(d.w);
        SC_ADD(e.x); SC_ADD(e.y); SC_ADD(e.z); SC_ADD(e.w);
    }
    for (; i < S4; i += SC_T) {
        const int4 a = s4[i];
        SC_ADD(a.x); SC_ADD(a.y); SC_ADD(a.z); SC_ADD(a.w);
    }
    for (int64_t t = 4 * S4 + threadIdx.x; t < S; t += SC_T) SC_ADD(status[t]);
#undef SC_ADD
    for (int k = 0; k < 4; ++k)
        if (loc[k]) atomicAdd(&c[k], loc[k]);
    __syncthreads();
    if (threadIdx.x < 4) counts[threadIdx.x] = c[threadIdx.x];
}

extern "C" int phgpu_status_counts(phgpu_handle h, const int32_t* status, int32_t* counts, void* stream) {
    if (!h || !status || !counts) return set_err(-1, "null argument");
    FLUSH_STEP(h);
    hipLaunchKernelGGL(k_status_counts, dim3(1), dim3(SC_T), 0, (hipStream_t)stream, status, h->S, counts);
    HIPCHK(hipGetLastError());
    return 0;
}

// statistics of a solve from its outputs: counts by status, iteration sum and maximum
__global__ void __launch_bounds__(SC_T) k_solve_stats(const int32_t* __restrict__ status,
                                                     const int32_t* __restrict__ iters, int64_t S,
                                                     unsigned long long* __restrict__ out) {
    __shared__ unsigned long long c[6];
    if (threadIdx.x < 6) c[threadIdx.x] = 0;
    __syncthreads();
    unsigned long long loc[4] = {0, 0, 0, 0}, isum = 0, imax = 0;
    for (int64_t t = threadIdx.x; t < S; t += SC_T) {
        const int v = status[t];
        loc[0] += v == 0, loc[1] += v == 1, loc[2] += v == 2, loc[3] += v == 3;
        if (iters) {
            const unsigned long long i = (unsigned long long)iters[t];
            isum += i;
            imax = i > imax ? i : imax;
        }
    }
    for (int k = 0; k < 4; ++k)
        if (loc[k]) atomicAdd(&c[k], loc[k]);
    if (isum) atomicAdd(&c[4], isum);
    if (imax) atomicMax(&c[5], imax);
    __syncthreads();
    if (threadIdx.x < 6) out[threadIdx.x] = c[threadIdx.x];
}

extern "C" int phgpu_solve_stats(phgpu_handle h, int64_t* out, void* stream) {
    if (!h || !out) return set_err(-1, "null argument");
    FLUSH_STEP(h);
    if (!h->last_status) return set_err(-1, "phgpu_solve_stats: no solve yet");
    hipStream_t st = (hipStream_t)stream;
    const unsigned long long* src = h->last_stats;
    if (!src) {
        hipLaunchKernelGGL(k_solve_stats, dim3(1), dim3(SC_T), 0, st, h->last_status, h->last_iters, h->S,
                           h->stats_gen);
        HIPCHK(hipGetLastError());
        src = h->stats_gen;
    } else {  // the path-6 copies, summed into stats_gen (out may be pageable host memory)
        hipLaunchKernelGGL(k_stats_copy, dim3(1), dim3(64), 0, st, src, PHGPU_STATS_COPIES, (int64_t*)h->stats_gen);
        HIPCHK(hipGetLastError());
        src = h->stats_gen;
    }
    HIPCHK(hipMemcpyAsync(out, src, 6 * sizeof(int64_t), hipMemcpyDefault, st));
    return 0;
}

// the x̄ partial sums of phgpu_ph_reduce (node_buf cleared, per-wave partials in part)
static int xbar_partials(phgpu_state* h, const double* x, double* node_buf, hipStream_t st) {
    const size_t nb = (size_t)2 * h->num_nodes * h->nlen_max;
    {
        const int rc = xbar_layout(h, st);
        if (rc) return rc;
    }
    if (h->xbar_mixed) HIPCHK(hipMemsetAsync(node_buf, 0, nb * sizeof(double), st));
    {
        dim3 g = grid_for(h->S);
        g.y = (unsigned)std::max(h->nn, 1);
        hipLaunchKernelGGL(k_xbar_partial, g, dim3(BLOCK), 0, st, *h, x, node_buf, h->xbar_mixed ? 0 : 1);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// the path-6 epilogue partials of x when the last solve writing the current slot produced
// them for this x buffer, else null
static bool xp_valid(const phgpu_state* h, const double* x, int k) {
    return k >= 0 && h->xp[k] && h->xp_C[k] > 0 && h->xp_x[k] == x && h->xbar_mixed == 0;
}
static bool xp_valid(const phgpu_state* h, const double* x) { return xp_valid(h, x, h->wslot); }
static ph_tree xp_view(const phgpu_state* h, int k) {  // the tree with part = the epilogue partials
    ph_tree v = *h;
    v.part = h->xp[k];
    v.part_node = h->xp_node[k];
    v.nwaves = h->xp_n[k];
    return v;
}
static ph_tree xp_view(const phgpu_state* h) { return xp_view(h, h->wslot); }

// one tree node whose every plane entry is a nonant's (two-stage problems): every wave is
// uniform and k_node_final's fast path stores each entry, so the planes need no clearing
static int assign_ok(const phgpu_state* h) { return (h->num_nodes == 1 && h->nlen_max == h->nn) ? 1 : 0; }

static int two_stage_only(phgpu_state* h, const char* who) {
    if (h->depth != 1 || h->num_nodes != 1)
        return set_err(-3, "%s: two-stage handles only (depth %d, %d nodes)", who, h->depth, h->num_nodes);
    return 0;
}

// A reduction's workspace at its first use: both buffers or neither.  wave_ws: per-wave
// partials of nv planes and node tags; ticket_ws: npart per-block partials and the (zeroed)
// last-block counter.
static int ws_alloc(phgpu_state* h, ph_ws& w, size_t npart, size_t ntag) {
    int rc = dalloc(h, &w.part, npart);
    if (!rc) rc = dalloc(h, &w.tag, ntag);
    if (rc) dfree(h, &w.part);
    return rc;
}
static int wave_ws(phgpu_state* h, ph_ws& w, int nv) {
    const size_t cnt = (size_t)h->nwaves * (size_t)h->nn;
    return w.part ? 0 : ws_alloc(h, w, cnt * nv, cnt);
}
static int ticket_ws(phgpu_state* h, ph_ws& w, size_t npart, hipStream_t st) {
    if (w.part) return 0;
    const int rc = ws_alloc(h, w, npart, 1);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(w.tag, 0, sizeof(int32_t), st));
    return 0;
}

// The planes of a node-segmented reduction from its per-wave partials in w: cleared to their
// identities (and extra, one more plane if given, to 0) unless every entry is stored, then
// partial (the caller's launch of its partial kernel) and k_node_final
template <int MAXMASK, int NV, typename Partial>
static int node_reduce(phgpu_state* h, ph_ws& w, double* planes, double* extra, hipStream_t st, Partial partial) {
    const int64_t half = (int64_t)h->num_nodes * h->nlen_max;
    const int assign = assign_ok(h);
    if (!assign) {
        const int64_t nex = extra ? half : 0;
        const int64_t nblk = std::max<int64_t>(1, std::min<int64_t>((NV * half + nex + 255) / 256, 256));
        hipLaunchKernelGGL((k_planes_clear<MAXMASK, NV>), dim3((unsigned)nblk), dim3(256), 0, st, planes, half, extra,
                           nex);
        HIPCHK(hipGetLastError());
    }
    if (h->nn == 0) return 0;
    const int rc = wave_ws(h, w, NV);
    if (rc) return rc;
    partial();
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL((k_node_final<MAXMASK, NV>), dim3(h->nn), dim3(XF_THREADS), 0, st, *h, (const double*)w.part,
                       (const int32_t*)w.tag, planes, assign);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int phgpu_ph_reduce(phgpu_handle h, const double* x, double* node_buf, void* stream) {
    if (!h || !x || !node_buf) return set_err(-1, "null argument");
    FLUSH_STEP(h);
    hipStream_t st = (hipStream_t)stream;
    const size_t nb = (size_t)2 * h->num_nodes * h->nlen_max;
    if (h->nn == 0) return hipMemsetAsync(node_buf, 0, nb * sizeof(double), st) == hipSuccess
                               ? 0 : set_err(-2, "hipMemsetAsync failed");
    // the current slot's solve, or a deferred solve not yet committed (x its output: the PH
    // loop reduces a speculative solve's x ahead of its convergence test, engine.xbar_ahead)
    const int k = xp_valid(h, x) ? h->wslot : (xp_valid(h, x, h->pending) ? h->pending : -1);
    if (k >= 0) {
        // the solve's epilogue wrote the per-chunk partials: final sums.  With one tree node
        // every node_buf entry is a nonant's (its block stores it); else clear it first
        const int assign = assign_ok(h);
        if (!assign) HIPCHK(hipMemsetAsync(node_buf, 0, nb * sizeof(double), st));
        hipLaunchKernelGGL(k_xbar_final, dim3(h->nn), dim3(XF_THREADS), 0, st, xp_view(h, k), node_buf,
                           (const int32_t*)h->xp_dirty[k], h->xp_C[k], x, assign);
        HIPCHK(hipGetLastError());
        return 0;
    }
    const int rc = xbar_partials(h, x, node_buf, st);
    if (rc) return rc;
    hipLaunchKernelGGL(k_xbar_final, dim3(h->nn), dim3(XF_THREADS), 0, st, *h, node_buf, nullptr, 0, nullptr);
    HIPCHK(hipGetLastError());
    return 0;
}

// the conv / statistics sink of the update kernels; launches k_solve_stats first when the
// last solve's path has no in-kernel statistics
static int make_sink(phgpu_state* h, double* conv_local, int64_t* stats_out, hipStream_t st, conv_sink& o) {
    o.conv = conv_local;
    o.stats_dst = stats_out;
    o.stats_src = stats_out ? h->last_stats : nullptr;
    o.stats_copies = PHGPU_STATS_COPIES;  // last_stats: the path-6 statistics
    if (stats_out && !o.stats_src) {  // a path without in-kernel statistics
        hipLaunchKernelGGL(k_solve_stats, dim3(1), dim3(SC_T), 0, st, h->last_status, h->last_iters, h->S,
                           h->stats_gen);
        HIPCHK(hipGetLastError());
        o.stats_src = h->stats_gen;
        o.stats_copies = 1;
    }
    o.scale = (h->nn > 0) ? 1.0 / ((double)h->S * (double)h->nn) : 0.0;
    o.cpart = h->cpart_blk;
    o.cnt = h->blk_cnt;
    return 0;
}

extern "C" int phgpu_ph_update_ex(phgpu_handle h, const double* x, const double* node_buf,
                                  double* xbar, double* W, const double* rho, int update_W,
                                  double* conv_local, int64_t* stats_out, void* stream) {
    if (!h || !x || !node_buf || !xbar || !conv_local || (update_W && (!W || !rho)))
        return set_err(-1, "null argument");
    if (stats_out && !h->last_status) return set_err(-1, "phgpu_ph_update_ex: stats_out before any solve");
    FLUSH_STEP(h);
    hipStream_t st = (hipStream_t)stream;
    conv_sink o;
    const int rc = make_sink(h, conv_local, stats_out, st, o);
    if (rc) return rc;
    // one launch: x̄ scatter, W update, conv (last-block reduction) and the statistics
    // (grid bound measured on config 4, k_ph_update us by kernel trace: 64 blocks 21.1, 128
    // 14.6, 256 12.9, 512 14.8, unbounded (1,536) 28.2; profiles/r06/ll/)
    const int64_t bx = std::min<int64_t>((h->S + UPD_T - 1) / UPD_T, std::max<int64_t>(1, UPD_BLOCKS / std::max(h->nn, 1)));
    hipLaunchKernelGGL(k_ph_update, dim3((unsigned)bx, (unsigned)std::max(h->nn, 1)), dim3(UPD_T), 0, st, *h, x,
                       node_buf, xbar, W, rho, update_W ? 1 : 0, o);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int phgpu_ph_update(phgpu_handle h, const double* x, const double* node_buf,
                               double* xbar, double* W, const double* rho, int update_W,
                               double* conv_local, void* stream) {
    return phgpu_ph_update_ex(h, x, node_buf, xbar, W, rho, update_W, conv_local, nullptr, stream);
}

extern "C" int phgpu_ph_step_local(phgpu_handle h, const double* x, double* node_buf, double* xbar, double* W,
                                   const double* rho, int update_W, double* conv_local, int64_t* stats_out,
                                   void* stream) {
    if (!h || !x || !node_buf || !xbar || !conv_local || (update_W && (!W || !rho)))
        return set_err(-1, "null argument");
    if (stats_out && !h->last_status) return set_err(-1, "phgpu_ph_step_local: stats_out before any solve");
    FLUSH_STEP(h);
    if (h->pvar) {
        // variable probabilities: the generic reduce + update (per-nonant weights, W mask)
        const int rc = phgpu_ph_reduce(h, x, node_buf, stream);
        if (rc) return rc;
        return phgpu_ph_update_ex(h, x, node_buf, xbar, W, rho, update_W, conv_local, stats_out, stream);
    }
    return step_local_impl(h, x, node_buf, xbar, W, rho, update_W, conv_local, stats_out, (hipStream_t)stream);
}

extern "C" int phgpu_ph_step_defer(phgpu_handle h, const double* x, double* node_buf, double* xbar, double* W,
                                   const double* rho, int update_W, double* conv_local, int64_t* stats_out,
                                   void* stream) {
    if (!h || !x || !node_buf || !xbar || !conv_local || (update_W && (!W || !rho)))
        return set_err(-1, "null argument");
    if (stats_out && !h->last_status) return set_err(-1, "phgpu_ph_step_defer: stats_out before any solve");
    FLUSH_STEP(h);
    // (variable probabilities: no folded step, the step runs now)
    if (h->pvar) return phgpu_ph_step_local(h, x, node_buf, xbar, W, rho, update_W, conv_local, stats_out, stream);
    phgpu_state::ph_pending& q = h->pend;
    q.active = 1;
    q.x = x;
    q.node_buf = node_buf;
    q.xbar = xbar;
    q.W = W;
    q.rho = rho;
    q.update_W = update_W ? 1 : 0;
    q.conv = conv_local;
    q.stats = stats_out;
    q.stream = (hipStream_t)stream;
    return 0;
}

extern "C" int phgpu_ph_step_flush(phgpu_handle h) {
    if (!h) return set_err(-1, "null handle");
    return flush_step(h);
}

static int step_local_impl(phgpu_state* h, const double* x, double* node_buf, double* xbar, double* W,
                           const double* rho, int update_W, double* conv_local, int64_t* stats_out, hipStream_t st) {
    void* stream = (void*)st;
    if (h->nn == 0 || h->nn > XL_NN_MAX || h->xbar_mixed != 0 || !h->xbar_single) {
        // the general route (also the first call, which finds out xbar_mixed / _single)
        const int rc = phgpu_ph_reduce(h, x, node_buf, stream);
        if (rc) return rc;
        return phgpu_ph_update_ex(h, x, node_buf, xbar, W, rho, update_W, conv_local, stats_out, stream);
    }
    // the per-chunk x̄ partials: from the path-6 epilogue when it wrote them for this x,
    // else from k_xbar_partial
    const bool xp = xp_valid(h, x);
    if (!xp) {
        const int rc = xbar_partials(h, x, node_buf, st);
        if (rc) return rc;
    }
    conv_sink o;
    const int rc = make_sink(h, conv_local, stats_out, st, o);
    if (rc) return rc;
    // 1,024-thread blocks for a large batch (fewer re-sums of the partials: 10.5 us at
    // 65,536 scenarios vs 14 us with 64-thread blocks), 256 for a small one (8,192: the update
    // part spread over 32 blocks; profiles/r03/x/)
    const unsigned T = h->S > 16384 ? XL_T : 256;
    hipLaunchKernelGGL(k_ph_update_local, dim3((unsigned)((h->S + T - 1) / T)), dim3(T), 0, st,
                       xp ? xp_view(h) : ph_tree(*h), x, node_buf, xbar, W, rho, update_W ? 1 : 0, o,
                       xp ? (const int32_t*)h->xp_dirty[h->wslot] : nullptr, xp ? h->xp_C[h->wslot] : 0);
    HIPCHK(hipGetLastError());
    return 0;
}

// norm_rho_updater.py:55-104 and the convergers' sums (include/phgpu.h)
extern "C" int phgpu_ph_residuals(phgpu_handle h, const double* x, const double* xbar, const double* rho,
                                  double* planes, double* rho_last, void* stream) {
    if (!h || !x || !xbar || !rho || !planes || !rho_last) return set_err(-1, "null argument");
    FLUSH_STEP(h);
    hipStream_t st = (hipStream_t)stream;
    // (when nothing is cleared, assign_ok, the last scenario's lane stores rho_last: both
    // outputs are overwritten in full)
    return node_reduce<0, RS_NV>(h, h->rs, planes, rho_last, st, [&] {
        dim3 g = grid_for(h->S);
        g.y = (unsigned)h->nn;
        hipLaunchKernelGGL(k_resid_partial, g, dim3(BLOCK), 0, st, *h, h->rs, x, xbar, rho, planes, rho_last);
    });
}

// norm_rho_updater.py:128-143
extern "C" int phgpu_norm_rho_update(phgpu_handle h, const phgpu_norm_rho_params* prm, const double* planes,
                                     const double* rho_last, const double* xbar_node, const double* xbar_prev,
                                     double* rho, int64_t* counts, void* stream) {
    if (!h || !prm || !planes || !rho_last || !xbar_node || !xbar_prev || !rho) return set_err(-1, "null argument");
    FLUSH_STEP(h);
    hipStream_t st = (hipStream_t)stream;
    if (counts) HIPCHK(hipMemsetAsync(counts, 0, 4 * sizeof(int64_t), st));
    if (h->nn == 0) return 0;
    const int64_t bx = std::min<int64_t>((h->S + NR_T - 1) / NR_T, std::max<int64_t>(1, UPD_BLOCKS / h->nn));
    hipLaunchKernelGGL(k_norm_rho_update, dim3((unsigned)bx, (unsigned)h->nn), dim3(NR_T), 0, st, *h, *prm, planes,
                       rho_last, xbar_node, xbar_prev, rho, (unsigned long long*)counts);
    HIPCHK(hipGetLastError());
    return 0;
}

// extensions/xhatxbar.py:38-55, cylinders/slam_heuristic.py:57-84 (include/phgpu.h)
extern "C" int phgpu_nonant_stats(phgpu_handle h, const double* v, double* planes, void* stream) {
    if (!h || !v || !planes) return set_err(-1, "null argument");
    FLUSH_STEP(h);
    hipStream_t st = (hipStream_t)stream;
    return node_reduce<0xC, RS_NV>(h, h->ns, planes, nullptr, st, [&] {
        dim3 g = grid_for(h->S);
        g.y = (unsigned)((h->nn + NS_KU - 1) / NS_KU);
        hipLaunchKernelGGL(k_nstats_partial, g, dim3(BLOCK), 0, st, *h, h->ns, v, planes);
    });
}

// extensions/xhatclosest.py:37-51
extern "C" int phgpu_nonant_closest(phgpu_handle h, const double* v, const double* xbar_node,
                                    const double* xsqbar_node, double* dist, double* best, void* stream) {
    if (!h || !v || !xbar_node || !xsqbar_node || !best) return set_err(-1, "null argument");
    if (two_stage_only(h, "phgpu_nonant_closest")) return -3;
    FLUSH_STEP(h);
    hipStream_t st = (hipStream_t)stream;
    const int64_t nblk = (h->S + NC_T - 1) / NC_T;
    const int rc = ticket_ws(h, h->nc, (size_t)(2 * nblk), st);
    if (rc) return rc;
    hipLaunchKernelGGL(k_nonant_closest, dim3((unsigned)nblk), dim3(NC_T), 0, st, *h, v, xbar_node, xsqbar_node, dist,
                       h->nc.part, h->nc.tag, best);
    HIPCHK(hipGetLastError());
    return 0;
}

// utils/gradient.py:65-81
extern "C" int phgpu_grad_cost(phgpu_handle h, const double* xn, double* cost, void* stream) {
    if (!h || !xn || !cost) return set_err(-1, "null argument");
    if (!h->scen_set) return set_err(-1, "phgpu_grad_cost: no scenario data yet");
    FLUSH_STEP(h);
    if (h->nn == 0) return 0;
    const int64_t bx = std::min<int64_t>((h->S + GR_T - 1) / GR_T, 65535);
    hipLaunchKernelGGL(k_grad_cost, dim3((unsigned)bx, (unsigned)std::min(h->nn, GR_ROWS)), dim3(GR_T), 0,
                       (hipStream_t)stream, *h, xn, cost);
    HIPCHK(hipGetLastError());
    return 0;
}

// utils/wtracker.py:141-154
extern "C" int phgpu_w_diff(phgpu_handle h, const double* W, double* W_prev, double* out, void* stream) {
    if (!h || !W || !W_prev || !out) return set_err(-1, "null argument");
    FLUSH_STEP(h);
    hipStream_t st = (hipStream_t)stream;
    if (h->nn == 0) {
        HIPCHK(hipMemsetAsync(out, 0, sizeof(double), st));
        return 0;
    }
    const int rc = ticket_ws(h, h->wd, (size_t)WD_BLOCKS, st);
    if (rc) return rc;
    const int64_t tot = (int64_t)h->nn * h->S;
    // four elements per thread before the grid is capped
    const int64_t nblk = std::max<int64_t>(1, std::min<int64_t>((tot + 4 * GR_T - 1) / (4 * GR_T), WD_BLOCKS));
    hipLaunchKernelGGL(k_w_diff, dim3((unsigned)nblk), dim3(GR_T), 0, st, W, W_prev, tot, 1.0 / (double)tot,
                       h->wd.part, h->wd.tag, out);
    HIPCHK(hipGetLastError());
    return 0;
}

// utils/find_rho.py:78-147 and 170-203
extern "C" int phgpu_rho_ratio_stats(phgpu_handle h, const double* cost, const double* x, const double* xbar,
                                     const double* gden, double* planes, void* stream) {
    if (!h || !cost || !planes || (!gden && (!x || !xbar))) return set_err(-1, "null argument");
    if (two_stage_only(h, "phgpu_rho_ratio_stats")) return -3;
    FLUSH_STEP(h);
    hipStream_t st = (hipStream_t)stream;
    return node_reduce<0x6, RR_NV>(h, h->rr, planes, nullptr, st, [&] {
        hipLaunchKernelGGL(k_rho_ratio_partial, grid_for(h->S), dim3(BLOCK), 0, st, *h, h->rr, cost, x, xbar, gden);
    });
}

// utils/find_rho.py:150-168, extensions/gradient_extension.py:65-68 and 85-94
extern "C" int phgpu_rho_from_stats(phgpu_handle h, const double* planes, int64_t S_total, double order_stat,
                                    const double* gate, double thr, double* rho, int32_t* applied, void* stream) {
    if (!h || !planes || !rho) return set_err(-1, "null argument");
    if (!(order_stat >= 0.0 && order_stat <= 1.0))
        return set_err(-1, "phgpu_rho_from_stats: order_stat %g is not in [0, 1] (0 the min, 0.5 the mean, 1 the max)",
                       order_stat);
    if (S_total <= 0) return set_err(-1, "phgpu_rho_from_stats: S_total %lld", (long long)S_total);
    if (two_stage_only(h, "phgpu_rho_from_stats")) return -3;
    FLUSH_STEP(h);
    const int64_t bx = std::min<int64_t>((h->S + GR_T - 1) / GR_T, std::max<int64_t>(1, UPD_BLOCKS / std::max(1, h->nn)));
    const unsigned rows = (unsigned)std::min(std::max(1, h->nn), GR_ROWS);
    hipLaunchKernelGGL(k_rho_from_stats, dim3((unsigned)bx, rows), dim3(GR_T), 0,
                       (hipStream_t)stream, *h, planes, (double)S_total, order_stat, gate, thr, rho, applied);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int phgpu_expectations(phgpu_handle h, const double* obj, const double* bound,
                                  const int32_t* status, double* out, void* stream) {
    if (!h || !obj || !bound || !status || !out) return set_err(-1, "null argument");
    FLUSH_STEP(h);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_expect_partial, grid_for(h->S), dim3(BLOCK), 0, st, *h, obj, bound, status);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_sum_partials, dim3(5), dim3(256), 0, st, (const double*)h->part, h->nwaves, 5, 1.0,
                       out);
    HIPCHK(hipGetLastError());
    return 0;
}

// confidence_intervals/ciutils.py:400-415 (and zhat4xhat.py:94 with the x* side NULL)
extern "C" int phgpu_gap_moments(phgpu_handle h, const double* f_hat, const int32_t* st_hat, const double* f_star,
                                 const int32_t* st_star, const int64_t* seg_ptr, int32_t nseg, int64_t s_off,
                                 double* out, void* stream) {
    if (!h || !f_hat || !st_hat || !seg_ptr || !out) return set_err(-1, "null argument");
    if (nseg < 1) return set_err(-1, "phgpu_gap_moments: nseg %d", (int)nseg);
    if ((f_star == nullptr) != (st_star == nullptr))
        return set_err(-1, "phgpu_gap_moments: f_star and st_star go together (both or neither)");
    if (!h->scen_set) return set_err(-1, "phgpu_gap_moments: no scenario data yet");
    FLUSH_STEP(h);
    hipStream_t st = (hipStream_t)stream;
    if (!h->gm.part) {
        const int rc = ws_alloc(h, h->gm, (size_t)h->nwaves * 2 * GM_NV, (size_t)h->nwaves * 2);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(k_gap_partial, grid_for(h->S), dim3(BLOCK), 0, st, *h, f_hat, st_hat, f_star, st_star, seg_ptr,
                       (int)nseg, s_off, h->gm.part, h->gm.tag, out);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_gap_final, dim3((unsigned)nseg), dim3(WAVE), 0, st, h->S, seg_ptr, s_off,
                       (const double*)h->gm.part, (const int32_t*)h->gm.tag, out);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int phgpu_fix_nonants(phgpu_handle h, const double* xfix, void* stream) {
    if (!h) return set_err(-1, "null handle");
    FLUSH_STEP(h);
    if (h->nn == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (h->shared) {
        const int64_t tot = (int64_t)h->nn * h->S;
        hipLaunchKernelGGL(k_fix_nonants_sh, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, *h, xfix);
        HIPCHK(hipGetLastError());
        return 0;
    }
    hipLaunchKernelGGL(k_fix_nonants, grid_for(h->S), dim3(BLOCK), 0, st, *h, xfix);
    HIPCHK(hipGetLastError());
    if (h->pk) {
        HIPCHK(to_records(h, h->lbh, h->n, h->pk_LB, st));
        HIPCHK(to_records(h, h->ubh, h->n, h->pk_UB, st));
    }
    return 0;
}

// extensions/fixer.py:114-128 (_update_fix_counts), 131-223 (iter0), 226-304 (iterk)
extern "C" int phgpu_fixer_step(phgpu_handle h, const phgpu_fixer_params* prm, const double* node_buf,
                                const double* th, const int32_t* nb, const int32_t* lb, const int32_t* ub,
                                int32_t* count, double* fixval, int32_t* nfix, int64_t* totals, void* stream) {
    if (!h || !prm || !node_buf || !th || !nb || !lb || !ub || !count || !fixval || !nfix || !totals)
        return set_err(-1, "null argument");
    if (!h->scen_set) return set_err(-1, "phgpu_fixer_step: no scenario data yet");
    FLUSH_STEP(h);
    hipStream_t st = (hipStream_t)stream;
    const int64_t half = (int64_t)h->num_nodes * h->nlen_max;
    if (h->nn == 0) {
        HIPCHK(hipMemsetAsync(nfix, 0, (size_t)half * sizeof(int32_t), st));
        return 0;
    }
    const dim3 g((unsigned)std::min<int64_t>((h->S + FX_T - 1) / FX_T, FX_BLOCKS), (unsigned)std::min(h->nn, GR_ROWS));
    if (!h->fx_nloc) {  // {nloc | acc}, acc zero between calls (k_fixer_totals clears what it read)
        const int rc = dalloc(h, &h->fx_nloc, (size_t)(2 * half));
        if (rc) return rc;
        HIPCHK(hipMemsetAsync(h->fx_nloc, 0, (size_t)(2 * half) * sizeof(int32_t), st));
        h->fx_valid = 0;
    } else if (!h->fx_valid) {
        HIPCHK(hipMemsetAsync(h->fx_nloc, 0, (size_t)half * sizeof(int32_t), st));
    }
    if (!h->fx_valid) {
        hipLaunchKernelGGL(k_fixer_nloc, g, dim3(FX_T), 0, st, *h, h->fx_nloc);
        HIPCHK(hipGetLastError());
        h->fx_valid = 1;
    }
    int32_t* acc = h->fx_nloc + half;
    if (h->shared)
        hipLaunchKernelGGL(k_fixer_step<true>, g, dim3(FX_T), 0, st, *h, *prm, node_buf, th, nb, lb, ub, count, fixval,
                           acc, (unsigned long long*)totals);
    else
        hipLaunchKernelGGL(k_fixer_step<false>, g, dim3(FX_T), 0, st, *h, *prm, node_buf, th, nb, lb, ub, count,
                           fixval, acc, (unsigned long long*)totals);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_fixer_totals, dim3(1), dim3(FX_T), 0, st, acc, (const int32_t*)h->fx_nloc, half, nfix,
                       (long long*)totals);
    HIPCHK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ FWPH (ph_fwph.inc)
static void fwph_release(phgpu_state* h) {
    fwph_store* fw = h->fw;
    if (!fw) return;
    dfree(h, &fw->X);
    dfree(h, &fw->f);
    dfree(h, &fw->a);
    dfree(h, &fw->G);
    dfree(h, &fw->L);
    dfree(h, &fw->lin);
    dfree(h, &fw->u);
    dfree(h, &fw->v);
    dfree(h, &fw->xq);
    dfree(h, &fw->phi);
    dfree(h, &fw->ncols);
    dfree(h, &fw->active);
    dfree(h, &fw->last);
    dfree(h, &fw->nit);
    dfree(h, &fw->acc);
    delete fw;
    h->fw = nullptr;
}

// fwph.py:685-771 (_initialize_QP_subproblems): one store for all local scenarios
extern "C" int phgpu_fwph_init(phgpu_handle h, int32_t max_cols, void* stream) {
    if (!h) return set_err(-1, "null handle");
    if (max_cols < 2 || max_cols > 64) return set_err(-1, "phgpu_fwph_init: max_cols %d is not in [2, 64]", max_cols);
    if (!h->scen_set) return set_err(-1, "phgpu_fwph_init: no scenario data yet");
    FLUSH_STEP(h);
    hipStream_t st = (hipStream_t)stream;
    if (h->fw && h->fw->max_cols != max_cols) {
        HIPCHK(hipStreamSynchronize(st));  // (a resize: nothing of the old store may be in flight)
        fwph_release(h);
    }
    const size_t S = (size_t)h->S, nn = (size_t)std::max(1, h->nn), K = (size_t)max_cols, T = K * (K + 1) / 2;
    if (!h->fw) {
        fwph_store* fw = new (std::nothrow) fwph_store();
        if (!fw) return set_err(-3, "out of host memory");
        memset(fw, 0, sizeof(*fw));
        fw->max_cols = max_cols;
        h->fw = fw;
        int rc = dalloc(h, &fw->X, K * nn * S);
        if (!rc) rc = dalloc(h, &fw->f, K * S);
        if (!rc) rc = dalloc(h, &fw->a, K * S);
        if (!rc) rc = dalloc(h, &fw->G, T * S);
        if (!rc) rc = dalloc(h, &fw->L, T * S);
        if (!rc) rc = dalloc(h, &fw->lin, K * S);
        if (!rc) rc = dalloc(h, &fw->u, K * S);
        if (!rc) rc = dalloc(h, &fw->v, K * S);
        if (!rc) rc = dalloc(h, &fw->xq, nn * S);
        if (!rc) rc = dalloc(h, &fw->phi, S);
        if (!rc) rc = dalloc(h, &fw->ncols, S);
        if (!rc) rc = dalloc(h, &fw->active, S);
        if (!rc) rc = dalloc(h, &fw->last, S);
        if (!rc) rc = dalloc(h, &fw->nit, S);
        if (!rc) rc = dalloc(h, &fw->acc, (size_t)4);
        if (rc) {
            fwph_release(h);
            return rc;
        }
    }
    fwph_store* fw = h->fw;
    HIPCHK(hipMemsetAsync(fw->xq, 0, nn * S * sizeof(double), st));
    HIPCHK(hipMemsetAsync(fw->phi, 0, S * sizeof(double), st));
    HIPCHK(hipMemsetAsync(fw->ncols, 0, S * sizeof(int32_t), st));
    HIPCHK(hipMemsetAsync(fw->active, 0, S * sizeof(int32_t), st));
    HIPCHK(hipMemsetAsync(fw->last, 0, S * sizeof(int32_t), st));
    HIPCHK(hipMemsetAsync(fw->nit, 0, S * sizeof(int32_t), st));
    HIPCHK(hipMemsetAsync(fw->acc, 0, 4 * sizeof(int32_t), st));
    return 0;
}

#define FWPH_READY(h, who)                                                        \
    do {                                                                          \
        if (!(h)) return set_err(-1, "null handle");                              \
        if (!(h)->fw) return set_err(-1, who ": phgpu_fwph_init has not run");   \
        FLUSH_STEP(h);                                                            \
    } while (0)

// fwph.py:773-791 (_initialize_QP_var_values) and the initial points of :744-755
extern "C" int phgpu_fwph_load(phgpu_handle h, int32_t K, const double* X, const double* f, const double* a,
                               const double* rho, double* xq, double* xqx, void* stream) {
    FWPH_READY(h, "phgpu_fwph_load");
    if (!X || !f || !rho) return set_err(-1, "null argument");
    if (K < 1 || K > h->fw->max_cols) return set_err(-1, "phgpu_fwph_load: %d columns, the store holds 1..%d", K, h->fw->max_cols);
    hipLaunchKernelGGL(k_fw_load, dim3((unsigned)((h->S + FW_T - 1) / FW_T)), dim3(FW_T), 0, (hipStream_t)stream, *h,
                       *h->fw, (int)K, X, f, a, rho, xq, xqx);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int phgpu_fwph_export(phgpu_handle h, double* X, double* f, double* a, int32_t* ncols, double* xq,
                                 double* phi, int32_t* active, int32_t* nit, void* stream) {
    FWPH_READY(h, "phgpu_fwph_export");
    hipLaunchKernelGGL(k_fw_export, dim3((unsigned)((h->S + FW_T - 1) / FW_T)), dim3(FW_T), 0, (hipStream_t)stream,
                       *h, *h->fw, X, f, a, ncols, xq, phi, active, nit);
    HIPCHK(hipGetLastError());
    return 0;
}

// fwph.py:227-247
extern "C" int phgpu_fwph_direction(phgpu_handle h, int t0, double alpha, const double* W, const double* rho,
                                    const double* xbar, double* What, void* stream) {
    FWPH_READY(h, "phgpu_fwph_direction");
    if (!W || !rho || !xbar || !What) return set_err(-1, "null argument");
    if (h->nn == 0) return 0;
    const int64_t bx = std::min<int64_t>((h->S + GR_T - 1) / GR_T, std::max<int64_t>(1, UPD_BLOCKS / std::max(1, h->nn)));
    hipLaunchKernelGGL(k_fw_direction, dim3((unsigned)bx, (unsigned)std::min(h->nn, GR_ROWS)), dim3(GR_T), 0,
                       (hipStream_t)stream, *h, *h->fw, t0 ? 1 : 0, alpha, W, rho, xbar, What);
    HIPCHK(hipGetLastError());
    return 0;
}

// fwph.py:256-292 and 305-370 (_add_QP_column)
extern "C" int phgpu_fwph_column(phgpu_handle h, const phgpu_fwph_params* prm, int t0, const double* x,
                                 const double* obj, const double* bound, const int32_t* status, const double* W,
                                 const double* What, const double* rho, const double* xbar, double* gamma,
                                 double* dual_bound, int32_t* ncols, double* xq, double* xqx, int32_t* counts,
                                 void* stream) {
    FWPH_READY(h, "phgpu_fwph_column");
    if (!prm || !x || !obj || !bound || !status || !W || !What || !rho || !xbar || !gamma || !dual_bound || !ncols ||
        !xq || !xqx || !counts)
        return set_err(-1, "null argument");
    hipLaunchKernelGGL(k_fw_column, dim3((unsigned)((h->S + FW_T - 1) / FW_T)), dim3(FW_T), 0, (hipStream_t)stream, *h,
                       *h->fw, *prm, t0 ? 1 : 0, x, obj, bound, status, W, What, rho, xbar, gamma, dual_bound, ncols, xq,
                       xqx, counts);
    HIPCHK(hipGetLastError());
    return 0;
}

// fwph.py:528-547 (_conv_diff)
extern "C" int phgpu_fwph_diff(phgpu_handle h, const double* xbar, double* out, void* stream) {
    FWPH_READY(h, "phgpu_fwph_diff");
    if (!xbar || !out) return set_err(-1, "null argument");
    hipStream_t st = (hipStream_t)stream;
    const int rc = ticket_ws(h, h->fwd, WD_BLOCKS, st);
    if (rc) return rc;
    const int64_t nblk = std::max<int64_t>(1, std::min<int64_t>((h->S + GR_T - 1) / GR_T, WD_BLOCKS));
    hipLaunchKernelGGL(k_fw_diff, dim3((unsigned)nblk), dim3(GR_T), 0, st, *h, *h->fw, xbar, h->fwd.part, h->fwd.tag,
                       out);
    HIPCHK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ APH (ph_aph.inc)
// aph.py:151-181 and 394-408
extern "C" int phgpu_aph_reduce(phgpu_handle h, int first, const int32_t* mask, const double* x, const double* W_use,
                                const double* z_use, const double* rho, double* y, double* planes, void* stream) {
    if (!h || !x || !y || !planes || (!first && (!W_use || !z_use || !rho))) return set_err(-1, "null argument");
    FLUSH_STEP(h);
    hipStream_t st = (hipStream_t)stream;
    return node_reduce<0, AP_NV>(h, h->apr, planes, nullptr, st, [&] {
        dim3 g = grid_for(h->S);
        g.y = (unsigned)h->nn;
        hipLaunchKernelGGL(k_aph_reduce_partial, g, dim3(BLOCK), 0, st, *h, h->apr, first ? 1 : 0, mask, x, W_use,
                           z_use, rho, y, planes);
    });
}

static inline unsigned aph_blocks(const phgpu_state* h) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((h->S + GR_T - 1) / GR_T, WD_BLOCKS));
}

// aph.py:254-310 and 185-195
extern "C" int phgpu_aph_norms(phgpu_handle h, double gamma, const double* planes, const double* x, const double* y,
                               const double* W, const double* z, double* xbar, double* u, double* phi, double* out,
                               void* stream) {
    if (!h || !planes || !x || !y || !W || !z || !xbar || !u || !phi || !out) return set_err(-1, "null argument");
    if (!(gamma > 0.0)) return set_err(-1, "phgpu_aph_norms: gamma %g is not positive", gamma);
    FLUSH_STEP(h);
    hipStream_t st = (hipStream_t)stream;
    const int rc = ticket_ws(h, h->apn, (size_t)4 * WD_BLOCKS, st);
    if (rc) return rc;
    hipLaunchKernelGGL(k_aph_norms, dim3(aph_blocks(h)), dim3(GR_T), 0, st, *h, gamma, planes, x, y, W, z, xbar, u, phi,
                       h->apn.part, h->apn.tag, out);
    HIPCHK(hipGetLastError());
    return 0;
}

// aph.py:453-496 and 756
extern "C" int phgpu_aph_update(phgpu_handle h, int first, double nu, double gamma, const double* red,
                                const double* planes, const double* x, const double* y, const double* u, double* W,
                                double* z, double* phi, double* out, void* stream) {
    if (!h || !red || !planes || !x || !y || !u || !W || !z || !phi || !out) return set_err(-1, "null argument");
    if (!(gamma > 0.0)) return set_err(-1, "phgpu_aph_update: gamma %g is not positive", gamma);
    FLUSH_STEP(h);
    hipStream_t st = (hipStream_t)stream;
    const int rc = ticket_ws(h, h->apu, (size_t)3 * WD_BLOCKS, st);
    if (rc) return rc;
    hipLaunchKernelGGL(k_aph_update, dim3(aph_blocks(h)), dim3(GR_T), 0, st, *h, first ? 1 : 0, nu, gamma, red, planes,
                       x, y, u, W, z, phi, h->apu.part, h->apu.tag, out);
    HIPCHK(hipGetLastError());
    return 0;
}

// aph.py:646, 529-550 and the sort keys of :610-611 and :626-629
extern "C" int phgpu_aph_mark(phgpu_handle h, const int32_t* mask, int32_t iter, int32_t shelf_life, int round_robin,
                              const double* phi, int32_t* last_iter, double* last_phi, double* k1, const double* W,
                              const double* z, double* W_lag, double* z_lag, void* stream) {
    if (!h || !mask || !phi || !last_iter || !last_phi || !k1) return set_err(-1, "null argument");
    if ((W_lag != nullptr) != (z_lag != nullptr) || (W_lag && (!W || !z)))
        return set_err(-1, "phgpu_aph_mark: the lagged copies need W, z, W_lag and z_lag");
    FLUSH_STEP(h);
    hipLaunchKernelGGL(k_aph_mark, dim3(aph_blocks(h)), dim3(GR_T), 0, (hipStream_t)stream, *h, mask, (int)iter,
                       (int)shelf_life, round_robin ? 1 : 0, phi, last_iter, last_phi, k1, W, z, W_lag, z_lag);
    HIPCHK(hipGetLastError());
    return 0;
}

// the dispatch list of aph.py:602-632
extern "C" int phgpu_select_smallest(phgpu_handle h, const double* k1, const double* k2, int32_t count, int32_t* mask,
                                     int32_t* list, void* stream) {
    if (!h || !k2 || !mask || !list) return set_err(-1, "null argument");
    if (h->S >= (1LL << 31) || count < 1 || (int64_t)count > h->S)
        return set_err(-1, "phgpu_select_smallest: count %d of %lld scenarios", (int)count, (long long)h->S);
    FLUSH_STEP(h);
    hipStream_t st = (hipStream_t)stream;
    if (!h->sel) {
        const int rc = dalloc(h, &h->sel, 1);
        if (rc) return rc;
        HIPCHK(hipMemsetAsync(h->sel, 0, sizeof(sel_state), st));
    }
    const int64_t S = h->S;
    // four scenarios per thread before the grid is capped
    const unsigned nb = (unsigned)std::max<int64_t>(1, std::min<int64_t>((S + 4 * SEL_T - 1) / (4 * SEL_T), SEL_BLOCKS));
    int cnt0 = count;  // (the first launch starts the state)
    for (int which = k1 ? 0 : 1; which < 2; ++which)
        for (int pass = 0; pass < SEL_PASSES; ++pass) {
            hipLaunchKernelGGL(k_sel_pass, dim3(nb), dim3(SEL_T), 0, st, S, k1, k2, which, pass, cnt0, h->sel);
            cnt0 = 0;
        }
    const int64_t ne = std::max<int64_t>(1, std::min<int64_t>((S + SEL_T - 1) / SEL_T, SEL_EMIT_BLOCKS));
    const int64_t chunk = (((S + ne - 1) / ne + SEL_T - 1) / SEL_T) * SEL_T;
    hipLaunchKernelGGL(k_sel_count, dim3((unsigned)ne), dim3(SEL_T), 0, st, S, chunk, k1, k2, h->sel);
    hipLaunchKernelGGL(k_sel_emit, dim3((unsigned)ne), dim3(SEL_T), 0, st, S, chunk, (int)count, k1, k2,
                       (const sel_state*)h->sel, mask, list);
    HIPCHK(hipGetLastError());
    return 0;
}

// A warm solve of the listed scenarios only, in place, on a kernel with a list mode: path 5 of
// the handle's path-6 module where path 6 is the default (as ipm_fallback_launch binds it), the
// handle's own path-5 module where that is the default, else k_solve
extern "C" int phgpu_solve_list(phgpu_handle h, const phgpu_options* opt, const int32_t* list, int32_t count,
                                double* x, double* y, double* obj, double* bound, int32_t* status, int32_t* iters,
                                void* stream) {
    if (!h) return set_err(-1, "null handle");
    if (count < 0 || (int64_t)count > h->S)
        return set_err(-1, "phgpu_solve_list: %d entries for %lld scenarios", (int)count, (long long)h->S);
    if (count == 0) return 0;
    if (h->shared)
        return set_err(-3, "phgpu_solve_list: a shared-matrix handle (path 4) has no list mode");
    if (!list || !x || !obj || !bound || !status) return set_err(-1, "null argument");
    FLUSH_STEP(h);
    // in place in the committed slot; an uncommitted deferred solve is dropped
    h->pending = -1;
    h->wq = h->wslot;
    bind_slots(h);
    if (!h->have_solution) return set_err(-1, "phgpu_solve_list: a warm solve, and no solve has run yet");
    phgpu_options o;
    {
        const int orc = solve_options(opt, o);
        if (orc) return orc;
    }
    const solve_params P = make_solve_params(o, 1);
    hipStream_t st = (hipStream_t)stream;
    if (!h->list_n) {
        const int rc = dalloc(h, &h->list_n, 1);
        if (rc) return rc;
    }
    int rc = warm_from_records(h, P, st);
    if (rc) return rc;
    hipFunction_t fn = nullptr;
    int per_cu = 0;
    if (o.gamma == 1.0) {
        const int path = default_path(h);
        if (path == 6 && ipm_prepare(h, st) == 0 && h->ipm->fn_pdhg) {
            fn = h->ipm->fn_pdhg;
            per_cu = h->ipm->per_cu_pdhg;
        } else if (path == 5) {
            rc = jit_prepare(h, st);
            if (rc) return rc;
            fn = h->jit->fn;
            per_cu = h->jit->per_cu;
        }
    }
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)h->list_n, (int)count, 1, st));
    if (fn) {
        jit_params a{};
        a.A = h->Ah_csr; a.c = h->c; a.q = h->q; a.Dc = h->Dc; a.lbh = h->lbh; a.ubh = h->ubh; a.Dr = h->Dr;
        a.rlh = h->rlh; a.ruh = h->ruh; a.rl = h->rl; a.ru = h->ru; a.objc = h->objc; a.normA = h->normA;
        a.W = h->W; a.rho = h->rho; a.xbar = h->xbar;
        a.omega_in = h->omega; a.x_in = h->x; a.y_in = h->y;
        a.omega_out = h->omega_w; a.x_w = h->xw; a.y_w = h->yw;
        a.xout = x; a.yout = y; a.obj = obj; a.bound = bound;
        a.status = status; a.iters = iters; a.qhead = h->qhead;
        a.list = list; a.list_n = h->list_n; a.stats = nullptr;
        a.S = h->S;
        a.W_on = h->W_on; a.prox_on = h->prox_on;
        a.eps_rel = P.eps_rel; a.eps_abs = P.eps_abs; a.bsuff = P.bsuff; a.bnec = P.bnec; a.bart = P.bart;
        a.eta_frac = P.eta_frac; a.omega0 = P.omega0; a.wmin = P.wmin; a.wmax = P.wmax; a.eps_inf = P.eps_inf;
        a.max_iter = P.max_iter; a.check_every = P.check_every; a.restart_every = P.restart_every; a.warm = 1;
        a.keep_omega = P.keep_omega; a.infeas_start = P.infeas_start;
        // a persistent grid that drains the list through the queue (first_dyn 0: the kernel's
        // static first assignment is by scenario index, not by list entry)
        const int64_t per = (int64_t)(per_cu < 1 ? 1 : per_cu) * h->num_cus * 256;
        const int64_t nblk = (std::min<int64_t>(per, count) + 255) / 256;
        a.first_dyn = 0;
        HIPCHK(hipMemsetAsync(h->qhead, 0, sizeof(int), st));
        void* args[] = {&a};
        HIPCHK(hipModuleLaunchKernel(fn, (unsigned)nblk, 1, 1, 256, 1, 1, 0, st, args, nullptr));
    } else {
        hipLaunchKernelGGL(k_solve, dim3((unsigned)((count + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, *h, P, x, y, obj,
                           bound, status, iters, list, (const int32_t*)h->list_n);
        HIPCHK(hipGetLastError());
    }
    h->last_stats = nullptr;
    solve_done(h, fn ? 5 : 1, 0, 0, status, iters);
    return 0;
}

// ------------------------------------------------------------------ the L-shaped method (ph_lshaped.inc)
static void lshaped_release(phgpu_state* h) {
    ls_store* L = h->ls;
    if (!L) return;
    dfree(h, &L->cut_a); dfree(h, &L->cut_b); dfree(h, &L->cut_g); dfree(h, &L->ncuts);
    dfree(h, &L->R); dfree(h, &L->rl); dfree(h, &L->ru); dfree(h, &L->eq);
    dfree(h, &L->xlb); dfree(h, &L->xub); dfree(h, &L->etalb);
    dfree(h, &L->zw); dfree(h, &L->has_w);
    dfree(h, &L->s); dfree(h, &L->lam); dfree(h, &L->rp); dfree(h, &L->ds); dfree(h, &L->dl);
    dfree(h, &L->t); dfree(h, &L->w); dfree(h, &L->V); dfree(h, &L->terms);
    delete L;
    h->ls = nullptr;
}

template <typename T>
static int ls_upload(phgpu_state* h, T** d, const T* src, size_t count) {
    const int rc = dalloc(h, d, count);
    if (rc) return rc;
    if (count && src) HIPCHK(hipMemcpy(*d, src, count * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}

// lshaped.py:84-160 (the root problem without its cuts) and the cut store
extern "C" int phgpu_lshaped_init(phgpu_handle h, int32_t G, int32_t max_cuts, int64_t s_off, int64_t S_total,
                                  int32_t n_rows, const double* R, const double* rl, const double* ru,
                                  const double* xlb, const double* xub, const double* etalb, void* stream) {
    if (!h) return set_err(-1, "null handle");
    if (!h->scen_set) return set_err(-1, "phgpu_lshaped_init: no scenario data yet");
    if (h->shared) return set_err(-3, "phgpu_lshaped_init: a shared-matrix handle is not served");
    if (h->depth != 1 || h->num_nodes != 1)
        return set_err(-3, "phgpu_lshaped_init: two-stage handles only (depth %d, %d nodes)", h->depth, h->num_nodes);
    if (h->nn < 1 || h->nn > LS_NN_MAX || G < 1 || G > LS_G_MAX || n_rows < 0 || n_rows > LS_ROWS_MAX)
        return set_err(-1, "phgpu_lshaped_init: nn %d (1..%d), G %d (1..%d), n_rows %d (0..%d)", h->nn, LS_NN_MAX, (int)G,
                       LS_G_MAX, (int)n_rows, LS_ROWS_MAX);
    if (max_cuts < 1 || max_cuts > (1 << 20)) return set_err(-1, "phgpu_lshaped_init: max_cuts %d", (int)max_cuts);
    if (S_total < 1 || s_off < 0 || s_off + h->S > S_total)
        return set_err(-1, "phgpu_lshaped_init: scenarios [%lld, %lld) of %lld", (long long)s_off,
                       (long long)(s_off + h->S), (long long)S_total);
    if (!xlb || !xub || !etalb || (n_rows && (!R || !rl || !ru))) return set_err(-1, "null argument");
    const int nn = h->nn;
    std::vector<int32_t> eq;
    for (int k = 0; k < nn; ++k)
        if (!(xlb[k] < xub[k]) || xlb[k] == INFINITY || xub[k] == -INFINITY)
            return set_err(-1, "phgpu_lshaped_init: nonant %d has bounds [%g, %g] (no interior)", k, xlb[k], xub[k]);
    for (int g = 0; g < G; ++g)
        if (!isfinite(etalb[g])) return set_err(-1, "phgpu_lshaped_init: etalb[%d] = %g is not finite", g, etalb[g]);
    for (int r = 0; r < n_rows; ++r) {
        if (rl[r] > ru[r] || rl[r] == INFINITY || ru[r] == -INFINITY || rl[r] != rl[r] || ru[r] != ru[r])
            return set_err(-1, "phgpu_lshaped_init: row %d has sides [%g, %g]", r, rl[r], ru[r]);
        if (rl[r] == ru[r]) eq.push_back(r);
    }
    FLUSH_STEP(h);
    hipStream_t st = (hipStream_t)stream;
    if (h->ls) {
        HIPCHK(hipStreamSynchronize(st));  // (nothing of the old store may be in flight)
        lshaped_release(h);
    }
    ls_store* L = new (std::nothrow) ls_store();
    if (!L) return set_err(-3, "out of host memory");
    memset(L, 0, sizeof(*L));
    h->ls = L;
    L->G = G; L->nn = nn; L->N = nn + G; L->ld = (nn + G) | 1; L->max_cuts = max_cuts; L->n_rows = n_rows;
    L->ne = (int)eq.size();
    L->NI = 2 * nn + G + 2 * n_rows + max_cuts;
    L->s_off = s_off; L->S_total = S_total;
    const size_t NI = (size_t)L->NI, S = (size_t)h->S;
    int rc = dalloc(h, &L->cut_a, (size_t)nn * max_cuts);
    if (!rc) rc = dalloc(h, &L->cut_b, (size_t)max_cuts);
    if (!rc) rc = dalloc(h, &L->cut_g, (size_t)max_cuts);
    if (!rc) rc = dalloc(h, &L->ncuts, 1);
    if (!rc) rc = ls_upload(h, &L->R, R, (size_t)n_rows * nn);
    if (!rc) rc = ls_upload(h, &L->rl, rl, (size_t)n_rows);
    if (!rc) rc = ls_upload(h, &L->ru, ru, (size_t)n_rows);
    if (!rc) rc = ls_upload(h, &L->eq, eq.data(), eq.size());
    if (!rc) rc = ls_upload(h, &L->xlb, xlb, (size_t)nn);
    if (!rc) rc = ls_upload(h, &L->xub, xub, (size_t)nn);
    if (!rc) rc = ls_upload(h, &L->etalb, etalb, (size_t)G);
    if (!rc) rc = dalloc(h, &L->zw, (size_t)L->N);
    if (!rc) rc = dalloc(h, &L->has_w, 1);
    if (!rc) rc = dalloc(h, &L->s, NI);
    if (!rc) rc = dalloc(h, &L->lam, NI);
    if (!rc) rc = dalloc(h, &L->rp, NI);
    if (!rc) rc = dalloc(h, &L->ds, NI);
    if (!rc) rc = dalloc(h, &L->dl, NI);
    if (!rc) rc = dalloc(h, &L->t, NI);
    if (!rc) rc = dalloc(h, &L->w, NI);
    if (!rc) rc = dalloc(h, &L->V, (size_t)L->N * std::max(1, L->ne));
    if (!rc) rc = dalloc(h, &L->terms, (size_t)(nn + 3) * S);
    if (rc) {
        lshaped_release(h);
        return rc;
    }
    HIPCHK(hipMemsetAsync(L->cut_a, 0, (size_t)nn * max_cuts * sizeof(double), st));
    HIPCHK(hipMemsetAsync(L->cut_b, 0, (size_t)max_cuts * sizeof(double), st));
    HIPCHK(hipMemsetAsync(L->cut_g, 0, (size_t)max_cuts * sizeof(int32_t), st));
    HIPCHK(hipMemsetAsync(L->ncuts, 0, sizeof(int32_t), st));
    HIPCHK(hipMemsetAsync(L->has_w, 0, sizeof(int32_t), st));
    HIPCHK(hipMemsetAsync(L->zw, 0, (size_t)L->N * sizeof(double), st));
    return 0;
}

#define LSHAPED_READY(h, who)                                                       \
    do {                                                                            \
        if (!(h)) return set_err(-1, "null handle");                                \
        if (!(h)->ls) return set_err(-1, who ": phgpu_lshaped_init has not run");  \
        FLUSH_STEP(h);                                                              \
    } while (0)

// lshaped.py:477-520, all local scenarios and their group sums
extern "C" int phgpu_lshaped_cuts(phgpu_handle h, const double* x, const double* y, const double* obj,
                                  const int32_t* status, double* cutbuf, void* stream) {
    LSHAPED_READY(h, "phgpu_lshaped_cuts");
    if (!x || !y || !obj || !status || !cutbuf) return set_err(-1, "null argument");
    hipStream_t st = (hipStream_t)stream;
    const ls_store& L = *h->ls;
    hipLaunchKernelGGL(k_ls_terms, dim3((unsigned)((h->S + GR_T - 1) / GR_T)), dim3(GR_T), 0, st, *h, L, x, y, obj,
                       status);
    hipLaunchKernelGGL(k_ls_gsum, dim3((unsigned)(L.G * (L.nn + 2) + 1)), dim3(GR_T), 0, st, L, h->S, cutbuf);
    HIPCHK(hipGetLastError());
    return 0;
}

// lshaped.py:540-560
extern "C" int phgpu_lshaped_append(phgpu_handle h, const double* cutbuf, const double* eta, double tol, double* info,
                                    void* stream) {
    LSHAPED_READY(h, "phgpu_lshaped_append");
    if (!cutbuf || !eta || !info) return set_err(-1, "null argument");
    if (!(tol >= 0.0)) return set_err(-1, "phgpu_lshaped_append: tol %g", tol);
    hipLaunchKernelGGL(k_ls_append, dim3(1), dim3(WAVE), 0, (hipStream_t)stream, *h->ls, cutbuf, eta, tol, info);
    HIPCHK(hipGetLastError());
    return 0;
}

// lshaped.py:600-630 (the root solve)
extern "C" int phgpu_lshaped_master(phgpu_handle h, const phgpu_options* opt, double* xhat, double* eta, double* info,
                                    void* stream) {
    LSHAPED_READY(h, "phgpu_lshaped_master");
    if (!xhat || !eta || !info) return set_err(-1, "null argument");
    phgpu_options o;
    if (opt) o = *opt;
    else phgpu_default_options(&o);
    if (!(o.eps_rel > 0.0) || !(o.eps_infeas > 0.0))
        return set_err(-1, "phgpu_lshaped_master: eps_rel %g, eps_infeas %g", o.eps_rel, o.eps_infeas);
    const ls_store& L = *h->ls;
    const size_t lds = ls_shared_doubles(L.N, L.ld, L.ne) * sizeof(double);
    if (lds > (size_t)160 * 1024) return set_err(-3, "phgpu_lshaped_master: %zu bytes of LDS", lds);
    HIPCHK(hipFuncSetAttribute((const void*)k_ls_master, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_ls_master, dim3(1), dim3(LS_T), lds, (hipStream_t)stream, L, h->S, o.eps_rel, o.eps_infeas,
                       LS_ITER_CAP, xhat, eta, info);
    HIPCHK(hipGetLastError());
    return 0;
}

// the store from / to the host (tests, checkpoints): K cuts as group [K], a [K][nn], b [K]
extern "C" int phgpu_lshaped_load(phgpu_handle h, int32_t K, const int32_t* group, const double* a, const double* b,
                                  void* stream) {
    LSHAPED_READY(h, "phgpu_lshaped_load");
    ls_store& L = *h->ls;
    if (K < 0 || K > L.max_cuts) return set_err(-1, "phgpu_lshaped_load: %d cuts, the store holds %d", (int)K, L.max_cuts);
    if (K && (!group || !a || !b)) return set_err(-1, "null argument");
    for (int c = 0; c < K; ++c)
        if (group[c] < 0 || group[c] >= L.G) return set_err(-1, "phgpu_lshaped_load: cut %d in group %d", c, (int)group[c]);
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipStreamSynchronize(st));
    std::vector<double> at((size_t)L.nn * L.max_cuts, 0.0);
    for (int c = 0; c < K; ++c)
        for (int k = 0; k < L.nn; ++k) at[(size_t)k * L.max_cuts + c] = a[(size_t)c * L.nn + k];
    HIPCHK(hipMemcpy(L.cut_a, at.data(), at.size() * sizeof(double), hipMemcpyHostToDevice));
    if (K) HIPCHK(hipMemcpy(L.cut_b, b, (size_t)K * sizeof(double), hipMemcpyHostToDevice));
    if (K) HIPCHK(hipMemcpy(L.cut_g, group, (size_t)K * sizeof(int32_t), hipMemcpyHostToDevice));
    const int32_t k32 = K, zero = 0;
    HIPCHK(hipMemcpy(L.ncuts, &k32, sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(L.has_w, &zero, sizeof(int32_t), hipMemcpyHostToDevice));
    return 0;
}

extern "C" int phgpu_lshaped_export(phgpu_handle h, int32_t* ncuts, int32_t* group, double* a, double* b, void* stream) {
    LSHAPED_READY(h, "phgpu_lshaped_export");
    if (!ncuts) return set_err(-1, "null argument");
    ls_store& L = *h->ls;
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    int32_t K = 0;
    HIPCHK(hipMemcpy(&K, L.ncuts, sizeof(int32_t), hipMemcpyDeviceToHost));
    K = std::min(K, (int32_t)L.max_cuts);
    *ncuts = K;
    if (K && group) HIPCHK(hipMemcpy(group, L.cut_g, (size_t)K * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (K && b) HIPCHK(hipMemcpy(b, L.cut_b, (size_t)K * sizeof(double), hipMemcpyDeviceToHost));
    if (K && a) {
        std::vector<double> at((size_t)L.nn * L.max_cuts);
        HIPCHK(hipMemcpy(at.data(), L.cut_a, at.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (int c = 0; c < K; ++c)
            for (int k = 0; k < L.nn; ++k) a[(size_t)c * L.nn + k] = at[(size_t)k * L.max_cuts + c];
    }
    return 0;
}

// ------------------------------------------------------------------ the extensive form (ph_ef.inc)
static void ef_release(phgpu_state* h) {
    ef_store* E = h->ef;
    if (!E) return;
    dfree(h, &E->x); dfree(h, &E->zl); dfree(h, &E->zu); dfree(h, &E->dx); dfree(h, &E->dxa); dfree(h, &E->D);
    dfree(h, &E->w); dfree(h, &E->vl); dfree(h, &E->vu); dfree(h, &E->y); dfree(h, &E->dw); dfree(h, &E->dwa);
    dfree(h, &E->dy); dfree(h, &E->dya); dfree(h, &E->g); dfree(h, &E->wk); dfree(h, &E->rp); dfree(h, &E->E);
    dfree(h, &E->fac); dfree(h, &E->terms); dfree(h, &E->zd); dfree(h, &E->C); dfree(h, &E->ctl);
    delete E;
    h->ef = nullptr;
}

static inline int ef_nsum0(const ef_store& E) { return E.ntri + 2 * E.nn + 2; }

// ef.py:60-100 / sc.py:60-100 (build the problem): the iterate's start
extern "C" int phgpu_ef_init(phgpu_handle h, const double* zlb, const double* zub, const double* cz, const double* qz,
                             double ncomp, double cmax, double tol, int32_t qp, void* stream) {
    if (!h) return set_err(-1, "null handle");
    if (!h->scen_set) return set_err(-1, "phgpu_ef_init: no scenario data yet");
    if (h->shared) return set_err(-3, "phgpu_ef_init: a shared-matrix handle is not served");
    if (h->depth != 1 || h->num_nodes != 1)
        return set_err(-3, "phgpu_ef_init: two-stage handles only (depth %d, %d nodes)", h->depth, h->num_nodes);
    if (h->nn < 1 || h->nn > EF_NN_MAX || h->m < 1 || h->m > EF_M_MAX)
        return set_err(-1, "phgpu_ef_init: nn %d (1..%d), m %d (1..%d)", h->nn, EF_NN_MAX, h->m, EF_M_MAX);
    if (!zlb || !zub || !cz || !qz) return set_err(-1, "null argument");
    if (!(ncomp >= 1.0) || !(cmax >= 0.0) || !(tol > 0.0))
        return set_err(-1, "phgpu_ef_init: ncomp %g, cmax %g, tol %g", ncomp, cmax, tol);
    const int nn = h->nn, m = h->m, n = h->n;
    for (int k = 0; k < nn; ++k)
        if (!(zlb[k] < zub[k]) || zlb[k] == INFINITY || zub[k] == -INFINITY || !(qz[k] >= 0.0))
            return set_err(-1, "phgpu_ef_init: nonant %d has bounds [%g, %g] (no interior) or q %g", k, zlb[k], zub[k],
                           qz[k]);
    FLUSH_STEP(h);
    hipStream_t st = (hipStream_t)stream;
    if (h->ef) {
        HIPCHK(hipStreamSynchronize(st));  // (nothing of the old store may be in flight)
        ef_release(h);
    }
    ef_store* E = new (std::nothrow) ef_store();
    if (!E) return set_err(-3, "out of host memory");
    memset(E, 0, sizeof(*E));
    h->ef = E;
    E->nn = nn; E->m = m; E->n = n; E->ntri = nn * (nn + 1) / 2; E->ld = nn | 1;
    E->nplanes = ef_nsum0(*E) + 2;
    const size_t S = (size_t)h->S;
    int rc = 0;
    for (double** p : {&E->x, &E->zl, &E->zu, &E->dx, &E->dxa, &E->D})
        if (!rc) rc = dalloc(h, p, (size_t)n * S);
    for (double** p : {&E->w, &E->vl, &E->vu, &E->y, &E->dw, &E->dwa, &E->dy, &E->dya, &E->g, &E->wk, &E->rp, &E->E})
        if (!rc) rc = dalloc(h, p, (size_t)m * S);
    if (!rc) rc = dalloc(h, &E->fac, (size_t)(m * (m + 1) / 2) * S);
    if (!rc) rc = dalloc(h, &E->terms, (size_t)E->nplanes * S);
    if (!rc) rc = dalloc(h, &E->C, (size_t)nn * E->ld);
    if (!rc) rc = dalloc(h, &E->ctl, (size_t)EF_CTL);
    std::vector<double> zd((size_t)(EZ_N + 1) * nn, 0.0), ctl(EF_CTL, 0.0);
    for (int k = 0; k < nn; ++k) {
        zd[(size_t)EZ_LB * nn + k] = zlb[k];
        zd[(size_t)EZ_UB * nn + k] = zub[k];
        zd[(size_t)EZ_C * nn + k] = cz[k];
        zd[(size_t)EZ_Q * nn + k] = qz[k];
        zd[(size_t)EZ_Z * nn + k] = ef_inside(zlb[k], zub[k]);
        zd[(size_t)EZ_ZL * nn + k] = isfinite(zlb[k]) ? 1.0 + fabs(cz[k]) : 0.0;
        zd[(size_t)EZ_ZU * nn + k] = isfinite(zub[k]) ? 1.0 + fabs(cz[k]) : 0.0;
    }
    ctl[EC_NCOMP] = ncomp; ctl[EC_CMAX] = cmax; ctl[EC_TOL] = tol; ctl[EC_QP] = qp ? 1.0 : 0.0;
    if (!rc) rc = ls_upload(h, &E->zd, zd.data(), zd.size());
    if (rc) {
        ef_release(h);
        return rc;
    }
    HIPCHK(hipMemcpy(E->ctl, ctl.data(), ctl.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemsetAsync(E->terms, 0, (size_t)E->nplanes * S * sizeof(double), st));
    hipLaunchKernelGGL(k_ef_start, dim3((unsigned)((h->S + EF_T - 1) / EF_T)), dim3(EF_T), 0, st, *h, *E);
    HIPCHK(hipGetLastError());
    return 0;
}

#define EF_READY(h, who, stage)                                                              \
    do {                                                                                     \
        if (!(h)) return set_err(-1, "null handle");                                         \
        if (!(h)->ef) return set_err(-1, who ": phgpu_ef_init has not run");                 \
        if ((stage) != 0 && (stage) != 1) return set_err(-1, who ": stage %d", (int)(stage)); \
        FLUSH_STEP(h);                                                                       \
    } while (0)

// the scenario pass and its sums over the local scenarios
extern "C" int phgpu_ef_schur(phgpu_handle h, int32_t stage, double* rsum, double* rmax, void* stream) {
    EF_READY(h, "phgpu_ef_schur", stage);
    if (!rsum || !rmax) return set_err(-1, "null argument");
    hipStream_t st = (hipStream_t)stream;
    const ef_store& E = *h->ef;
    const dim3 grid((unsigned)((h->S + EF_T - 1) / EF_T));
    hipLaunchKernelGGL(k_ef_schur, grid, dim3(EF_T), 0, st, *h, E, (int)stage);
    const int nsum = stage == 0 ? ef_nsum0(E) : E.nn, nmax = stage == 0 ? 2 : 0;
    hipLaunchKernelGGL(k_ef_reduce, dim3((unsigned)(nsum + nmax)), dim3(GR_T), 0, st, E, h->S, nsum, rsum, rmax);
    HIPCHK(hipGetLastError());
    return 0;
}

// the Schur complement's solve, the direction pass and its sums and maxima
extern "C" int phgpu_ef_direction(phgpu_handle h, int32_t stage, double* rsum, double* rmax, double* info, void* stream) {
    EF_READY(h, "phgpu_ef_direction", stage);
    if (!rsum || !rmax || !info) return set_err(-1, "null argument");
    hipStream_t st = (hipStream_t)stream;
    const ef_store& E = *h->ef;
    const size_t lds = ((size_t)E.nn * E.ld + E.nn) * sizeof(double);
    hipLaunchKernelGGL(k_ef_solve, dim3(1), dim3(LS_T), lds, st, E, (int)stage, (const double*)rsum, (const double*)rmax,
                       info);
    const dim3 grid((unsigned)((h->S + EF_T - 1) / EF_T));
    hipLaunchKernelGGL(k_ef_direction, grid, dim3(EF_T), 0, st, *h, E, (int)stage);
    hipLaunchKernelGGL(k_ef_reduce, dim3(5), dim3(GR_T), 0, st, E, h->S, 3, rsum, rmax);
    HIPCHK(hipGetLastError());
    return 0;
}

// the step lengths and sigma (stage 0), the step (stage 1)
extern "C" int phgpu_ef_step(phgpu_handle h, int32_t stage, const double* rsum, const double* rmax, void* stream) {
    EF_READY(h, "phgpu_ef_step", stage);
    if (!rsum || !rmax) return set_err(-1, "null argument");
    hipStream_t st = (hipStream_t)stream;
    const ef_store& E = *h->ef;
    const dim3 grid((unsigned)((h->S + EF_T - 1) / EF_T));
    hipLaunchKernelGGL(k_ef_ctrl, dim3(1), dim3(WAVE), 0, st, E, (int)stage, rsum, rmax);
    if (stage == 0) hipLaunchKernelGGL(k_ef_keep, grid, dim3(EF_T), 0, st, *h, E);
    else hipLaunchKernelGGL(k_ef_step, grid, dim3(EF_T), 0, st, *h, E);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int phgpu_ef_export(phgpu_handle h, double* x, double* y, double* obj, double* bound, int32_t* status,
                               int32_t* iters, double* z, void* stream) {
    EF_READY(h, "phgpu_ef_export", 0);
    if (!x || !obj || !bound || !status || !iters) return set_err(-1, "null argument");
    hipStream_t st = (hipStream_t)stream;
    const ef_store& E = *h->ef;
    hipLaunchKernelGGL(k_ef_export, dim3((unsigned)((h->S + EF_T - 1) / EF_T)), dim3(EF_T), 0, st, *h, E, x, y, obj, bound,
                       status, iters);
    HIPCHK(hipGetLastError());
    if (z) HIPCHK(hipMemcpyAsync(z, EF_Z(E, EZ_Z), (size_t)E.nn * sizeof(double), hipMemcpyDeviceToDevice, st));
    h->last_stats = nullptr;
    return 0;
}

// ------------------------------------------------------------------ bundles: the segmented form (ph_ef.inc)
// One extensive form per contiguous segment of the local scenarios (spbase.py:219-253,
// spopt.py:805-836), all solved at once.
struct bd_store {
    ef_store E;  // zd, C, ctl: G copies, segment-major
    ef_segs B;
    int32_t *seg_start, *seg_of;
    double* info8;  // [G][8]: the cores' own records
    int qp;
    double seq;  // records stored so far
};

static void bd_release(phgpu_state* h) {
    bd_store* D = h->bd;
    if (!D) return;
    ef_store* E = &D->E;
    dfree(h, &E->x); dfree(h, &E->zl); dfree(h, &E->zu); dfree(h, &E->dx); dfree(h, &E->dxa); dfree(h, &E->D);
    dfree(h, &E->w); dfree(h, &E->vl); dfree(h, &E->vu); dfree(h, &E->y); dfree(h, &E->dw); dfree(h, &E->dwa);
    dfree(h, &E->dy); dfree(h, &E->dya); dfree(h, &E->g); dfree(h, &E->wk); dfree(h, &E->rp); dfree(h, &E->E);
    dfree(h, &E->fac); dfree(h, &E->terms); dfree(h, &E->zd); dfree(h, &E->C); dfree(h, &E->ctl);
    dfree(h, &D->B.cprob); dfree(h, &D->B.ceff); dfree(h, &D->B.qeff); dfree(h, &D->B.rsum); dfree(h, &D->B.rmax);
    dfree(h, &D->seg_start); dfree(h, &D->seg_of); dfree(h, &D->info8);
    delete D;
    h->bd = nullptr;
}

// the lanes' view of the problem: conditional probabilities, the solve's cost and diagonal
static inline ph_data bd_view(const phgpu_state* h, const bd_store& D) {
    ph_data v = *h;
    v.prob = D.B.cprob;
    v.c = D.B.ceff;
    v.q = D.B.qeff;
    return v;
}

extern "C" int phgpu_bundle_init(phgpu_handle h, int32_t G, const int32_t* seg_start, const double* zlb, const double* zub,
                                 const double* ncomp, const double* cmax, double tol, double ztol, int32_t qp, void* stream) {
    if (!h) return set_err(-1, "null handle");
    if (!h->scen_set) return set_err(-1, "phgpu_bundle_init: no scenario data yet");
    if (h->shared) return set_err(-3, "phgpu_bundle_init: a shared-matrix handle is not served");
    if (h->depth != 1 || h->num_nodes != 1)
        return set_err(-3, "phgpu_bundle_init: two-stage handles only (depth %d, %d nodes)", h->depth, h->num_nodes);
    if (h->nn < 1 || h->nn > EF_NN_MAX || h->m < 1 || h->m > EF_M_MAX)
        return set_err(-1, "phgpu_bundle_init: nn %d (1..%d), m %d (1..%d)", h->nn, EF_NN_MAX, h->m, EF_M_MAX);
    if (!seg_start || !zlb || !zub || !ncomp || !cmax) return set_err(-1, "null argument");
    if (G < 1 || (int64_t)G > h->S || !(tol > 0.0) || !(ztol > 0.0))
        return set_err(-1, "phgpu_bundle_init: %d segments, tol %g, ztol %g", (int)G, tol, ztol);
    if (seg_start[0] != 0 || (int64_t)seg_start[G] != h->S)
        return set_err(-1, "phgpu_bundle_init: the segments span [%d, %d), not the %lld local scenarios", (int)seg_start[0],
                       (int)seg_start[G], (long long)h->S);
    const int nn = h->nn, m = h->m, n = h->n;
    for (int g = 0; g < G; ++g) {
        if (seg_start[g + 1] <= seg_start[g]) return set_err(-1, "phgpu_bundle_init: segment %d is empty", g);
        if (!(ncomp[g] >= 1.0) || !(cmax[g] >= 0.0))
            return set_err(-1, "phgpu_bundle_init: segment %d: ncomp %g, cmax %g", g, ncomp[g], cmax[g]);
        for (int k = 0; k < nn; ++k) {
            const double lo = zlb[(size_t)g * nn + k], hi = zub[(size_t)g * nn + k];
            if (!(lo < hi) || lo == INFINITY || hi == -INFINITY)
                return set_err(-1, "phgpu_bundle_init: segment %d: nonant %d has bounds [%g, %g] (no interior)", g, k, lo, hi);
        }
    }
    FLUSH_STEP(h);
    hipStream_t st = (hipStream_t)stream;
    if (h->bd) {
        HIPCHK(hipStreamSynchronize(st));  // (nothing of the old store may be in flight)
        bd_release(h);
    }
    bd_store* D = new (std::nothrow) bd_store();
    if (!D) return set_err(-3, "out of host memory");
    memset(D, 0, sizeof(*D));
    h->bd = D;
    ef_store* E = &D->E;
    E->nn = nn; E->m = m; E->n = n; E->ntri = nn * (nn + 1) / 2; E->ld = nn | 1;
    E->nplanes = ef_nsum0(*E) + 2;
    D->B.G = G;
    D->B.nsum0 = ef_nsum0(*E);
    D->qp = qp ? 1 : 0;
    const size_t S = (size_t)h->S;
    int rc = 0;
    for (double** p : {&E->x, &E->zl, &E->zu, &E->dx, &E->dxa, &E->D, &D->B.ceff, &D->B.qeff})
        if (!rc) rc = dalloc(h, p, (size_t)n * S);
    for (double** p : {&E->w, &E->vl, &E->vu, &E->y, &E->dw, &E->dwa, &E->dy, &E->dya, &E->g, &E->wk, &E->rp, &E->E})
        if (!rc) rc = dalloc(h, p, (size_t)m * S);
    if (!rc) rc = dalloc(h, &E->fac, (size_t)(m * (m + 1) / 2) * S);
    if (!rc) rc = dalloc(h, &E->terms, (size_t)E->nplanes * S);
    if (!rc) rc = dalloc(h, &E->C, (size_t)G * nn * E->ld);
    if (!rc) rc = dalloc(h, &D->B.rsum, (size_t)G * D->B.nsum0);
    if (!rc) rc = dalloc(h, &D->B.rmax, (size_t)G * 2);
    if (!rc) rc = dalloc(h, &D->info8, (size_t)G * 8);
    // per segment: the static part of zd (the bounds) and of ctl; the conditional probabilities
    std::vector<double> zd((size_t)G * EF_ZD_LEN(*E), 0.0), ctl((size_t)G * EF_CTL, 0.0), prob(S), cprob(S);
    std::vector<int32_t> seg_of(S);
    // (a failure from here on gives the half-built store back: no later entry may find it)
#define BD_CHK(call)                                                                                          \
    do {                                                                                                      \
        hipError_t e_ = (call);                                                                               \
        if (e_ != hipSuccess) {                                                                               \
            bd_release(h);                                                                                    \
            return set_err(-2, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__);  \
        }                                                                                                     \
    } while (0)
    if (!rc) BD_CHK(hipMemcpy(prob.data(), h->prob, S * sizeof(double), hipMemcpyDeviceToHost));
    for (int g = 0; g < G && !rc; ++g) {
        double* z = zd.data() + (size_t)g * EF_ZD_LEN(*E);
        for (int k = 0; k < nn; ++k) {
            z[(size_t)EZ_LB * nn + k] = zlb[(size_t)g * nn + k];
            z[(size_t)EZ_UB * nn + k] = zub[(size_t)g * nn + k];
        }
        double* c = ctl.data() + (size_t)g * EF_CTL;
        c[EC_NCOMP] = ncomp[g]; c[EC_CMAX] = cmax[g];
        c[EC_TOL] = -1.0;  // (the core's own test is off: ef_seg_test decides, after the predictor's dz)
        c[EC_SEG_TOL] = tol; c[EC_SEG_ZTOL] = ztol;
        double pb = 0.0;
        for (int32_t s = seg_start[g]; s < seg_start[g + 1]; ++s) pb += prob[s];
        if (!(pb > 0.0)) {
            bd_release(h);
            return set_err(-1, "phgpu_bundle_init: segment %d has probability %g", g, pb);
        }
        for (int32_t s = seg_start[g]; s < seg_start[g + 1]; ++s) {
            cprob[s] = prob[s] / pb;
            seg_of[s] = g;
        }
    }
    if (!rc) rc = ls_upload(h, &E->zd, zd.data(), zd.size());
    if (!rc) rc = ls_upload(h, &E->ctl, ctl.data(), ctl.size());
    if (!rc) rc = ls_upload(h, &D->B.cprob, cprob.data(), cprob.size());
    if (!rc) rc = ls_upload(h, &D->seg_start, seg_start, (size_t)G + 1);
    if (!rc) rc = ls_upload(h, &D->seg_of, seg_of.data(), seg_of.size());
    if (rc) {
        bd_release(h);
        return rc;
    }
    D->B.seg_start = D->seg_start;
    D->B.seg_of = D->seg_of;
    BD_CHK(hipMemsetAsync(E->terms, 0, (size_t)E->nplanes * S * sizeof(double), st));
    BD_CHK(hipMemsetAsync(D->B.rsum, 0, (size_t)G * D->B.nsum0 * sizeof(double), st));
    BD_CHK(hipMemsetAsync(D->B.rmax, 0, (size_t)G * 2 * sizeof(double), st));
    BD_CHK(hipMemsetAsync(D->info8, 0, (size_t)G * 8 * sizeof(double), st));
#undef BD_CHK
    return 0;
}

#define BD_READY(h, who, stage)                                                              \
    do {                                                                                     \
        if (!(h)) return set_err(-1, "null handle");                                         \
        if (!(h)->bd) return set_err(-1, who ": phgpu_bundle_init has not run");             \
        if ((stage) != 0 && (stage) != 1) return set_err(-1, who ": stage %d", (int)(stage)); \
        FLUSH_STEP(h);                                                                       \
    } while (0)
#define BD_GRID(h) dim3((unsigned)(((h)->S + EF_T - 1) / EF_T))
#define BD_SEG_GRID(D) dim3((unsigned)(((D).B.G + EF_T - 1) / EF_T))

// every solve is a cold start from the handle's W, rho, x̄ and its W_on / prox_on switches
extern "C" int phgpu_bundle_start(phgpu_handle h, void* stream) {
    BD_READY(h, "phgpu_bundle_start", 0);
    if ((h->W_on || h->prox_on) && (!h->W || !h->rho || !h->xbar))
        return set_err(-1, "phgpu_bundle_start: W_on / prox_on without phgpu_set_ph_state's arrays");
    hipStream_t st = (hipStream_t)stream;
    const bd_store& D = *h->bd;
    const ph_data v = bd_view(h, D);
    hipLaunchKernelGGL(k_bd_start, BD_GRID(h), dim3(EF_T), 0, st, v, D.E, D.B, (const double*)h->c, (const double*)h->q,
                       h->W, h->rho, h->xbar, h->W_on, h->prox_on);
    hipLaunchKernelGGL(k_bd_zstart, BD_SEG_GRID(D), dim3(EF_T), 0, st, v, D.E, D.B, (D.qp || h->prox_on) ? 1 : 0);
    HIPCHK(hipGetLastError());
    return 0;
}

static void bd_reduce(phgpu_state* h, const bd_store& D, int nsum, int nmax, hipStream_t st) {
    const int64_t nt = (int64_t)(nsum + nmax) * D.B.G;
    hipLaunchKernelGGL(k_bd_reduce, dim3((unsigned)((nt + GR_T - 1) / GR_T)), dim3(GR_T), 0, st, D.E, D.B, h->S, nsum, nmax);
}

extern "C" int phgpu_bundle_schur(phgpu_handle h, int32_t stage, double* rsum, double* rmax, double* terms, void* stream) {
    BD_READY(h, "phgpu_bundle_schur", stage);
    hipStream_t st = (hipStream_t)stream;
    const bd_store& D = *h->bd;
    hipLaunchKernelGGL(k_bd_schur, BD_GRID(h), dim3(EF_T), 0, st, bd_view(h, D), D.E, D.B, (int)stage);
    bd_reduce(h, D, stage == 0 ? D.B.nsum0 : D.E.nn, stage == 0 ? 2 : 0, st);
    HIPCHK(hipGetLastError());
    const size_t G = (size_t)D.B.G;
    if (rsum) HIPCHK(hipMemcpyAsync(rsum, D.B.rsum, G * D.B.nsum0 * sizeof(double), hipMemcpyDeviceToDevice, st));
    if (rmax) HIPCHK(hipMemcpyAsync(rmax, D.B.rmax, G * 2 * sizeof(double), hipMemcpyDeviceToDevice, st));
    if (terms)
        HIPCHK(hipMemcpyAsync(terms, D.E.terms, (size_t)D.E.nplanes * (size_t)h->S * sizeof(double), hipMemcpyDeviceToDevice, st));
    return 0;
}

extern "C" int phgpu_bundle_direction(phgpu_handle h, int32_t stage, double* info, void* stream) {
    BD_READY(h, "phgpu_bundle_direction", stage);
    if (stage == 0 && !info) return set_err(-1, "null argument");
    hipStream_t st = (hipStream_t)stream;
    bd_store& D = *h->bd;
    const size_t lds = (((size_t)D.E.nn * D.E.ld + D.E.nn + 1) * sizeof(double) + 15) & ~(size_t)15;
    hipLaunchKernelGGL(k_bd_solve, dim3((unsigned)D.B.G), dim3(WAVE), lds, st, D.E, D.B, (int)stage, D.info8);
    if (stage == 0) {
        D.seq += 1.0;
        hipLaunchKernelGGL(k_bd_record, dim3(1), dim3(GR_T), 0, st, D.E, D.B.G, D.seq, info);
    }
    hipLaunchKernelGGL(k_bd_direction, BD_GRID(h), dim3(EF_T), 0, st, bd_view(h, D), D.E, D.B, (int)stage);
    bd_reduce(h, D, 3, 2, st);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int phgpu_bundle_step(phgpu_handle h, int32_t stage, void* stream) {
    BD_READY(h, "phgpu_bundle_step", stage);
    hipStream_t st = (hipStream_t)stream;
    const bd_store& D = *h->bd;
    hipLaunchKernelGGL(k_bd_ctrl, BD_SEG_GRID(D), dim3(EF_T), 0, st, D.E, D.B, (int)stage);
    const ph_data v = bd_view(h, D);
    if (stage == 0) hipLaunchKernelGGL(k_bd_keep, BD_GRID(h), dim3(EF_T), 0, st, v, D.E, D.B);
    else hipLaunchKernelGGL(k_bd_step, BD_GRID(h), dim3(EF_T), 0, st, v, D.E, D.B);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int phgpu_bundle_export(phgpu_handle h, double* x, double* y, double* obj, double* bound, int32_t* status,
                                   int32_t* iters, void* stream) {
    BD_READY(h, "phgpu_bundle_export", 0);
    if (!x || !obj || !bound || !status || !iters) return set_err(-1, "null argument");
    hipStream_t st = (hipStream_t)stream;
    const bd_store& D = *h->bd;
    hipLaunchKernelGGL(k_bd_export, BD_GRID(h), dim3(EF_T), 0, st, bd_view(h, D), D.E, D.B, h->rho, h->xbar, h->prox_on, x, y,
                       obj, bound, status, iters);
    HIPCHK(hipGetLastError());
    h->last_stats = nullptr;  // (the statistics of this solve come from its status / iters outputs)
    h->last_status = status;
    h->last_iters = iters;
    return 0;
}

// ------------------------------------------------------------------ the multistage extensive form (ph_ef_tree.inc)
// One interior point over a scenario tree (mpisppy/opt/ef.py with all_nodenames, sputils.create_EF),
// its Schur complement eliminated along the tree.
struct eft_store {
    ef_store E;  // zd: G copies (one per deepest non-leaf node), C: ROOT's factor, ctl: one record
    eft_tree T;
    int32_t *depth, *child0, *nchild, *zoff, *path, *P, *seg_start, *seg_of;
    int block_reduce;            // the segmented sum by a block per (plane, segment)
    std::vector<int> lvl0;       // [D + 1]: the first node of each depth
    std::vector<int> Ph;         // [D]: P_d on the host
    // for phgpu_eft_fix: the z fields as uploaded (zn: [EZ_N + 1][Ztot], rz: ROOT's [EZ_N + 1][P0]),
    // each entry's node, the count of finite bounds, and where the solve stands
    std::vector<double> zn, rz;
    std::vector<int> znode;
    double ncomp;
    bool held, begun;
};

static void eft_release(phgpu_state* h) {
    eft_store* X = h->eft;
    if (!X) return;
    ef_store* E = &X->E;
    dfree(h, &E->x); dfree(h, &E->zl); dfree(h, &E->zu); dfree(h, &E->dx); dfree(h, &E->dxa); dfree(h, &E->D);
    dfree(h, &E->w); dfree(h, &E->vl); dfree(h, &E->vu); dfree(h, &E->y); dfree(h, &E->dw); dfree(h, &E->dwa);
    dfree(h, &E->dy); dfree(h, &E->dya); dfree(h, &E->g); dfree(h, &E->wk); dfree(h, &E->rp); dfree(h, &E->E);
    dfree(h, &E->fac); dfree(h, &E->terms); dfree(h, &E->zd); dfree(h, &E->C); dfree(h, &E->ctl);
    eft_tree* T = &X->T;
    dfree(h, &T->zn); dfree(h, &T->rootzd); dfree(h, &T->slot); dfree(h, &T->hv); dfree(h, &T->ty); dfree(h, &T->nsc);
    dfree(h, &T->segsum); dfree(h, &T->segmax); dfree(h, &T->rootsum); dfree(h, &T->rootmax); dfree(h, &T->lsum);
    dfree(h, &T->lmax); dfree(h, &T->dirsum); dfree(h, &T->dirmax);
    dfree(h, &X->depth); dfree(h, &X->child0); dfree(h, &X->nchild); dfree(h, &X->zoff); dfree(h, &X->path); dfree(h, &X->P);
    dfree(h, &X->seg_start); dfree(h, &X->seg_of);
    delete X;
    h->eft = nullptr;
}

// a segment at least this long on average is summed by a block per (plane, segment)
#define EFT_BLOCK_REDUCE_LEN GR_T

extern "C" int phgpu_eft_init(phgpu_handle h, int32_t D, const int32_t* nlens, int32_t Nn, const int32_t* node_depth,
                              const int32_t* node_parent, const int32_t* seg_start, const double* zlb, const double* zub,
                              const double* cz, const double* qz, double ncomp, double cmax, double tol, int32_t qp,
                              void* stream) {
    if (!h) return set_err(-1, "null handle");
    if (!h->scen_set) return set_err(-1, "phgpu_eft_init: no scenario data yet");
    if (h->shared) return set_err(-3, "phgpu_eft_init: a shared-matrix handle is not served");
    if (!nlens || !node_depth || !node_parent || !seg_start || !zlb || !zub || !cz || !qz) return set_err(-1, "null argument");
    if (D < 2 || D != h->depth) return set_err(-1, "phgpu_eft_init: depth %d (the handle's %d; at least 2)", (int)D, h->depth);
    if (h->nn < 1 || h->nn > EF_NN_MAX || h->m < 1 || h->m > EF_M_MAX)
        return set_err(-1, "phgpu_eft_init: nn %d (1..%d), m %d (1..%d)", h->nn, EF_NN_MAX, h->m, EF_M_MAX);
    if (!(ncomp >= 1.0) || !(cmax >= 0.0) || !(tol > 0.0))
        return set_err(-1, "phgpu_eft_init: ncomp %g, cmax %g, tol %g", ncomp, cmax, tol);
    const int nn = h->nn, m = h->m, n = h->n;
    std::vector<int32_t> P(D);
    for (int d = 0, a = 0; d < D; ++d) {
        if (nlens[d] < 1) return set_err(-1, "phgpu_eft_init: depth %d has %d nonants", d, (int)nlens[d]);
        P[d] = (a += nlens[d]);
    }
    if (P[D - 1] != nn) return set_err(-1, "phgpu_eft_init: nlens sum to %d, the handle's nn is %d", (int)P[D - 1], nn);
    // the nodes: depth by depth, ROOT first, children of one node adjacent and in their parents' order
    if (Nn < D || node_depth[0] != 0 || node_parent[0] != -1) return set_err(-1, "phgpu_eft_init: node 0 is not ROOT");
    std::vector<int32_t> child0(Nn, 0), nchild(Nn, 0), zoff(Nn, 0), path((size_t)Nn * nn, 0);
    std::vector<int> lvl0(D + 1, Nn);
    lvl0[0] = 0;
    int Ztot = P[0];
    for (int k = 0; k < P[0]; ++k) path[k] = k;
    for (int i = 1; i < Nn; ++i) {
        const int d = node_depth[i], p = node_parent[i];
        if (d < 1 || d >= D || d < node_depth[i - 1] || d > node_depth[i - 1] + 1 || p < 0 || p >= i || node_depth[p] != d - 1 ||
            (node_depth[i - 1] == d && p < node_parent[i - 1]))
            return set_err(-1, "phgpu_eft_init: node %d (depth %d, parent %d) is out of the depth-by-depth order", i, d, p);
        if (node_depth[i - 1] != d) lvl0[d] = i;
        if (nchild[p] == 0) child0[p] = i;
        else if (child0[p] + nchild[p] != i) return set_err(-1, "phgpu_eft_init: the children of node %d are not adjacent", p);
        ++nchild[p];
        zoff[i] = Ztot;
        for (int k = 0; k < P[d - 1]; ++k) path[(size_t)i * nn + k] = path[(size_t)p * nn + k];
        for (int k = P[d - 1]; k < P[d]; ++k) path[(size_t)i * nn + k] = Ztot + (k - P[d - 1]);
        Ztot += nlens[d];
    }
    if (node_depth[Nn - 1] != D - 1) return set_err(-1, "phgpu_eft_init: no node of depth %d", (int)D - 1);
    const int deep0 = lvl0[D - 1], G = Nn - deep0;
    for (int i = 0; i < deep0; ++i)
        if (nchild[i] == 0) return set_err(-1, "phgpu_eft_init: node %d of depth %d has no child", i, (int)node_depth[i]);
    if (seg_start[0] != 0 || (int64_t)seg_start[G] != h->S)
        return set_err(-1, "phgpu_eft_init: the %d segments span [%d, %d), not the %lld local scenarios", G, (int)seg_start[0],
                       (int)seg_start[G], (long long)h->S);
    for (int g = 0; g < G; ++g)
        if (seg_start[g + 1] <= seg_start[g]) return set_err(-1, "phgpu_eft_init: segment %d is empty", g);
    for (int k = 0; k < Ztot; ++k)
        if (!(zlb[k] < zub[k]) || zlb[k] == INFINITY || zub[k] == -INFINITY || !(qz[k] >= 0.0))
            return set_err(-1, "phgpu_eft_init: z entry %d has bounds [%g, %g] (no interior) or q %g", k, zlb[k], zub[k], qz[k]);
    FLUSH_STEP(h);
    hipStream_t st = (hipStream_t)stream;
    if (h->eft) {
        HIPCHK(hipStreamSynchronize(st));  // (nothing of the old store may be in flight)
        eft_release(h);
    }
    eft_store* X = new (std::nothrow) eft_store();
    if (!X) return set_err(-3, "out of host memory");
    h->eft = X;
    ef_store* E = &X->E;
    eft_tree* T = &X->T;
    memset(E, 0, sizeof(*E));
    memset(T, 0, sizeof(*T));
    X->lvl0 = lvl0;
    X->Ph.assign(P.begin(), P.end());
    E->nn = nn; E->m = m; E->n = n; E->ntri = nn * (nn + 1) / 2; E->ld = nn | 1;
    E->nplanes = ef_nsum0(*E) + 2;
    T->D = D; T->Nn = Nn; T->G = G; T->nn = nn; T->ld = nn | 1; T->Ztot = Ztot; T->P0 = P[0]; T->deep0 = deep0;
    T->nsum0 = ef_nsum0(*E);
    const size_t S = (size_t)h->S;
    X->block_reduce = S / (size_t)G >= (size_t)EFT_BLOCK_REDUCE_LEN;
    const int P0 = P[0], nsumR = P0 * (P0 + 1) / 2 + 2 * P0 + 2;
    int rc = 0;
    for (double** p : {&E->x, &E->zl, &E->zu, &E->dx, &E->dxa, &E->D})
        if (!rc) rc = dalloc(h, p, (size_t)n * S);
    for (double** p : {&E->w, &E->vl, &E->vu, &E->y, &E->dw, &E->dwa, &E->dy, &E->dya, &E->g, &E->wk, &E->rp, &E->E})
        if (!rc) rc = dalloc(h, p, (size_t)m * S);
    if (!rc) rc = dalloc(h, &E->fac, (size_t)(m * (m + 1) / 2) * S);
    if (!rc) rc = dalloc(h, &E->terms, (size_t)E->nplanes * S);
    if (!rc) rc = dalloc(h, &E->C, (size_t)P0 * (P0 | 1));
    if (!rc) rc = dalloc(h, &E->zd, (size_t)G * EF_ZD_LEN(*E));
    if (!rc) rc = dalloc(h, &T->slot, (size_t)Nn * nn * T->ld);
    if (!rc) rc = dalloc(h, &T->hv, (size_t)Nn * nn);
    if (!rc) rc = dalloc(h, &T->ty, (size_t)Nn * nn);
    if (!rc) rc = dalloc(h, &T->nsc, (size_t)Nn * 2);
    if (!rc) rc = dalloc(h, &T->segsum, (size_t)G * T->nsum0);
    if (!rc) rc = dalloc(h, &T->segmax, (size_t)G * 2);
    if (!rc) rc = dalloc(h, &T->rootsum, (size_t)nsumR);
    if (!rc) rc = dalloc(h, &T->rootmax, (size_t)2);
    if (!rc) rc = dalloc(h, &T->lsum, (size_t)3);
    if (!rc) rc = dalloc(h, &T->lmax, (size_t)2);
    if (!rc) rc = dalloc(h, &T->dirsum, (size_t)3);
    if (!rc) rc = dalloc(h, &T->dirmax, (size_t)2);
    // z's start, as phgpu_ef_init sets it: ROOT's fields in its own block, the other nodes' by z index
    std::vector<double> zn((size_t)(EZ_N + 1) * Ztot, 0.0), rz((size_t)(EZ_N + 1) * P0, 0.0), ctl(EF_CTL, 0.0);
    for (int k = 0; k < Ztot; ++k) {
        double* base = k < P0 ? rz.data() + k : zn.data() + k;
        const size_t ldz = k < P0 ? (size_t)P0 : (size_t)Ztot;
        base[EZ_LB * ldz] = zlb[k]; base[EZ_UB * ldz] = zub[k]; base[EZ_C * ldz] = cz[k]; base[EZ_Q * ldz] = qz[k];
        base[EZ_Z * ldz] = ef_inside(zlb[k], zub[k]);
        base[EZ_ZL * ldz] = isfinite(zlb[k]) ? 1.0 + fabs(cz[k]) : 0.0;
        base[EZ_ZU * ldz] = isfinite(zub[k]) ? 1.0 + fabs(cz[k]) : 0.0;
    }
    ctl[EC_NCOMP] = ncomp; ctl[EC_CMAX] = cmax; ctl[EC_TOL] = tol; ctl[EC_QP] = qp ? 1.0 : 0.0;
    std::vector<int32_t> seg_of(S), depth(node_depth, node_depth + Nn);
    for (int g = 0; g < G; ++g)
        for (int32_t s = seg_start[g]; s < seg_start[g + 1]; ++s) seg_of[s] = g;
    X->znode.resize(Ztot);
    for (int i = 0; i < Nn; ++i)
        for (int k = 0; k < nlens[node_depth[i]]; ++k) X->znode[zoff[i] + k] = i;
    X->zn = zn;
    X->rz = rz;
    X->ncomp = ncomp;
    X->held = X->begun = false;
    if (!rc) rc = ls_upload(h, &T->zn, zn.data(), zn.size());
    if (!rc) rc = ls_upload(h, &T->rootzd, rz.data(), rz.size());
    if (!rc) rc = ls_upload(h, &E->ctl, ctl.data(), ctl.size());
    if (!rc) rc = ls_upload(h, &X->depth, depth.data(), depth.size());
    if (!rc) rc = ls_upload(h, &X->child0, child0.data(), child0.size());
    if (!rc) rc = ls_upload(h, &X->nchild, nchild.data(), nchild.size());
    if (!rc) rc = ls_upload(h, &X->zoff, zoff.data(), zoff.size());
    if (!rc) rc = ls_upload(h, &X->path, path.data(), path.size());
    if (!rc) rc = ls_upload(h, &X->P, P.data(), P.size());
    if (!rc) rc = ls_upload(h, &X->seg_start, seg_start, (size_t)G + 1);
    if (!rc) rc = ls_upload(h, &X->seg_of, seg_of.data(), seg_of.size());
    if (rc) {
        eft_release(h);
        return rc;
    }
    T->depth = X->depth; T->child0 = X->child0; T->nchild = X->nchild; T->zoff = X->zoff; T->path = X->path; T->P = X->P;
    T->seg_start = X->seg_start; T->seg_of = X->seg_of;
#define EFT_CHK(call)                                                                                         \
    do {                                                                                                      \
        hipError_t e_ = (call);                                                                               \
        if (e_ != hipSuccess) {                                                                               \
            eft_release(h);                                                                                   \
            return set_err(-2, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__);  \
        }                                                                                                     \
    } while (0)
    EFT_CHK(hipMemsetAsync(E->terms, 0, (size_t)E->nplanes * S * sizeof(double), st));
    EFT_CHK(hipMemsetAsync(E->zd, 0, (size_t)G * EF_ZD_LEN(*E) * sizeof(double), st));
    EFT_CHK(hipMemsetAsync(T->slot, 0, (size_t)Nn * nn * T->ld * sizeof(double), st));
    EFT_CHK(hipMemsetAsync(T->hv, 0, (size_t)Nn * nn * sizeof(double), st));
    EFT_CHK(hipMemsetAsync(T->ty, 0, (size_t)Nn * nn * sizeof(double), st));
    EFT_CHK(hipMemsetAsync(T->nsc, 0, (size_t)Nn * 2 * sizeof(double), st));
    EFT_CHK(hipMemsetAsync(T->segsum, 0, (size_t)G * T->nsum0 * sizeof(double), st));
    EFT_CHK(hipMemsetAsync(T->segmax, 0, (size_t)G * 2 * sizeof(double), st));
    EFT_CHK(hipMemsetAsync(T->rootsum, 0, (size_t)nsumR * sizeof(double), st));
    EFT_CHK(hipMemsetAsync(T->rootmax, 0, 2 * sizeof(double), st));
#undef EFT_CHK
    hipLaunchKernelGGL(k_ef_start, dim3((unsigned)((h->S + EF_T - 1) / EF_T)), dim3(EF_T), 0, st, *h, *E);
    hipLaunchKernelGGL(k_eft_gather, dim3((unsigned)((G * nn + EF_T - 1) / EF_T)), dim3(EF_T), 0, st, *E, *T, (int)EZ_Z);
    HIPCHK(hipGetLastError());
    return 0;
}

#define EFT_READY(h, who, stage)                                                             \
    do {                                                                                     \
        if (!(h)) return set_err(-1, "null handle");                                         \
        if (!(h)->eft) return set_err(-1, who ": phgpu_eft_init has not run");               \
        if ((stage) != 0 && (stage) != 1) return set_err(-1, who ": stage %d", (int)(stage)); \
        FLUSH_STEP(h);                                                                       \
    } while (0)
#define EFT_GATHER(X, f, st) \
    hipLaunchKernelGGL(k_eft_gather, dim3((unsigned)(((X).T.G * (X).T.nn + EF_T - 1) / EF_T)), dim3(EF_T), 0, st, (X).E, (X).T, (int)(f))

// Entries of z held at values: the empty box (ef_held), the value, no duals; the
// fields go up again whole from the store's host copies, which live as long as the store.
extern "C" int phgpu_eft_fix(phgpu_handle h, const double* zfix, void* stream) {
    EFT_READY(h, "phgpu_eft_fix", 0);
    if (!zfix) return set_err(-1, "null argument");
    eft_store& X = *h->eft;
    const eft_tree& T = X.T;
    if (X.begun) return set_err(-1, "phgpu_eft_fix: an iteration has begun (it comes before the first phgpu_eft_schur)");
    if (X.held) return set_err(-1, "phgpu_eft_fix: called twice (phgpu_eft_init starts over)");
    const int Ztot = T.Ztot, P0 = T.P0;
    auto fld = [&](int f, int k) -> double& {
        return k < P0 ? X.rz[(size_t)f * P0 + k] : X.zn[(size_t)f * Ztot + k];
    };
    for (int k = 0; k < Ztot; ++k) {
        const double v = zfix[k];
        if (v != v) continue;
        if (isfinite(v) && v >= fld(EZ_LB, k) && v <= fld(EZ_UB, k)) continue;
        const int nd = X.znode[k];
        int e = 0;  // the entry's place in its node
        while (e < k && X.znode[k - e - 1] == nd) ++e;
        return set_err(-1, "phgpu_eft_fix: node %d entry %d: the value %.17g is outside its bounds [%g, %g]", nd, e, v,
                       fld(EZ_LB, k), fld(EZ_UB, k));
    }
    double ncomp = X.ncomp;
    for (int k = 0; k < Ztot; ++k) {
        const double v = zfix[k];
        if (v != v) continue;
        ncomp -= (isfinite(fld(EZ_LB, k)) ? 1.0 : 0.0) + (isfinite(fld(EZ_UB, k)) ? 1.0 : 0.0);
        fld(EZ_LB, k) = INFINITY;
        fld(EZ_UB, k) = -INFINITY;
        fld(EZ_Z, k) = v;
        fld(EZ_ZL, k) = fld(EZ_ZU, k) = 0.0;
    }
    X.ncomp = fmax(1.0, ncomp);
    X.held = true;
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipMemcpyAsync(T.zn, X.zn.data(), X.zn.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(T.rootzd, X.rz.data(), X.rz.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(X.E.ctl + EC_NCOMP, &X.ncomp, sizeof(double), hipMemcpyHostToDevice, st));
    EFT_GATHER(X, EZ_Z, st);
    HIPCHK(hipGetLastError());
    return 0;
}

// the scenario pass, its segmented sums, the elimination up the tree and ROOT's sums
extern "C" int phgpu_eft_schur(phgpu_handle h, int32_t stage, double* nodeA, double* nodeb, void* stream) {
    EFT_READY(h, "phgpu_eft_schur", stage);
    h->eft->begun = true;
    hipStream_t st = (hipStream_t)stream;
    const eft_store& X = *h->eft;
    const ef_store& E = X.E;
    eft_tree T = X.T;
    T.inspA = stage == 0 ? nodeA : nullptr;
    T.inspb = nodeb;
    hipLaunchKernelGGL(k_eft_schur, BD_GRID(h), dim3(EF_T), 0, st, *h, E, T, (int)stage);
    const int nsum = stage == 0 ? T.nsum0 : T.nn, nmax = stage == 0 ? 2 : 0;
    if (X.block_reduce) {
        hipLaunchKernelGGL(k_eft_reduce_b, dim3((unsigned)(nsum + nmax), (unsigned)T.G), dim3(GR_T), 0, st, E, T, h->S, nsum);
    } else {
        const int64_t nt = (int64_t)(nsum + nmax) * T.G;
        hipLaunchKernelGGL(k_eft_reduce_t, dim3((unsigned)((nt + GR_T - 1) / GR_T)), dim3(GR_T), 0, st, E, T, h->S, nsum, nmax);
    }
    for (int d = T.D - 1; d >= 1; --d) {
        const int n0 = X.lvl0[d], cnt = X.lvl0[d + 1] - n0;
        const int Pd = X.Ph[d];  // (the workspace of this depth: P_d rows of the odd leading dimension, b and T'y)
        const size_t lds = ((size_t)Pd * T.ld + 2 * (size_t)Pd) * sizeof(double);
        hipLaunchKernelGGL(k_eft_elim, dim3((unsigned)cnt), dim3(WAVE), lds, st, E, T, n0, (int)stage);
    }
    hipLaunchKernelGGL(k_eft_root, dim3(1), dim3(GR_T), 0, st, E, T, (int)stage);
    HIPCHK(hipGetLastError());
    return 0;
}

// ROOT's solve (ef_solve_core on its view), the back-substitution down the tree, the direction
// pass and its sums and maxima with the nodes' share
extern "C" int phgpu_eft_direction(phgpu_handle h, int32_t stage, double* info, void* stream) {
    EFT_READY(h, "phgpu_eft_direction", stage);
    if (!info) return set_err(-1, "null argument");
    hipStream_t st = (hipStream_t)stream;
    const eft_store& X = *h->eft;
    const ef_store& E = X.E;
    const eft_tree& T = X.T;
    const ef_store R = eft_root_view(E, T);
    const size_t lds = ((size_t)R.nn * R.ld + R.nn) * sizeof(double);
    hipLaunchKernelGGL(k_ef_solve, dim3(1), dim3(LS_T), lds, st, R, (int)stage, (const double*)T.rootsum,
                       (const double*)T.rootmax, info);
    for (int d = 1; d < T.D; ++d) {
        const int n0 = X.lvl0[d], cnt = X.lvl0[d + 1] - n0;
        hipLaunchKernelGGL(k_eft_back, dim3((unsigned)((cnt + EF_T - 1) / EF_T)), dim3(EF_T), 0, st, E, T, n0, cnt);
    }
    EFT_GATHER(X, EZ_DZ, st);
    hipLaunchKernelGGL(k_eft_direction, BD_GRID(h), dim3(EF_T), 0, st, *h, E, T, (int)stage);
    hipLaunchKernelGGL(k_ef_reduce, dim3(5), dim3(GR_T), 0, st, E, h->S, 3, T.lsum, T.lmax);
    hipLaunchKernelGGL(k_eft_dirsum, dim3(1), dim3(GR_T), 0, st, E, T, (int)stage);
    HIPCHK(hipGetLastError());
    return 0;
}

// the step lengths and sigma (stage 0), the step (stage 1): ef_ctrl_core on ROOT's view, then the
// other nodes' z entries and the lanes
extern "C" int phgpu_eft_step(phgpu_handle h, int32_t stage, void* stream) {
    EFT_READY(h, "phgpu_eft_step", stage);
    hipStream_t st = (hipStream_t)stream;
    const eft_store& X = *h->eft;
    const ef_store& E = X.E;
    const eft_tree& T = X.T;
    hipLaunchKernelGGL(k_ef_ctrl, dim3(1), dim3(WAVE), 0, st, eft_root_view(E, T), (int)stage, (const double*)T.dirsum,
                       (const double*)T.dirmax);
    hipLaunchKernelGGL(k_eft_zstep, dim3((unsigned)((T.Ztot - T.P0 + EF_T - 1) / EF_T)), dim3(EF_T), 0, st, E, T, (int)stage);
    if (stage == 0) {
        hipLaunchKernelGGL(k_ef_keep, BD_GRID(h), dim3(EF_T), 0, st, *h, E);
    } else {
        hipLaunchKernelGGL(k_ef_step, BD_GRID(h), dim3(EF_T), 0, st, *h, E);
        EFT_GATHER(X, EZ_Z, st);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int phgpu_eft_export(phgpu_handle h, double* x, double* y, double* obj, double* bound, int32_t* status,
                                int32_t* iters, double* z, void* stream) {
    EFT_READY(h, "phgpu_eft_export", 0);
    if (!x || !obj || !bound || !status || !iters) return set_err(-1, "null argument");
    hipStream_t st = (hipStream_t)stream;
    const eft_store& X = *h->eft;
    const eft_tree& T = X.T;
    hipLaunchKernelGGL(k_eft_export, BD_GRID(h), dim3(EF_T), 0, st, *h, X.E, T, x, y, obj, bound, status, iters);
    HIPCHK(hipGetLastError());
    if (z) {
        HIPCHK(hipMemcpyAsync(z, T.rootzd + (size_t)EZ_Z * T.P0, (size_t)T.P0 * sizeof(double), hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(z + T.P0, T.zn + (size_t)EZ_Z * T.Ztot + T.P0, (size_t)(T.Ztot - T.P0) * sizeof(double),
                              hipMemcpyDeviceToDevice, st));
    }
    h->last_stats = nullptr;
    return 0;
}

#include "comm_rccl.inc"

extern "C" int phgpu_destroy(phgpu_handle h) {
    if (!h) return 0;
    rccl_release(h);
    module_release(h->jit);
    module_release(h->ipm);
    module_release(h->ipm_loop);
    delete h->fw;  // (its device buffers are in allocs)
    delete h->ls;
    delete h->ef;
    delete h->bd;
    delete h->eft;
    phgpu_owner* o = owner_of(h);  // (a deferred step that never ran is dropped with it)
    for (const dev_alloc& a : o->allocs) (void)hipFree(a.p);
    delete o;
    return 0;
}

extern "C" int phgpu_last_error(char* buf, size_t len) {
    if (!buf || len == 0) return -1;
    strncpy(buf, g_err, len - 1);
    buf[len - 1] = 0;
    return 0;
}

extern "C" int64_t phgpu_workspace_bytes(phgpu_handle h) { return h ? h->ws_bytes : -1; }

// path 4 of the last solve (include/phgpu.h)
extern "C" int phgpu_stream_info(phgpu_handle h, int32_t* info) {
    if (!h || !info) return set_err(-1, "null argument");
    info[0] = h->last_path == 4 ? h->last_cluster : 0;
    info[1] = h->last_path == 4 ? 1 : 0;
    return 0;
}

extern "C" int phgpu_kernel_info(phgpu_handle h, int32_t* info) {
    if (!h || !info) return set_err(-1, "null argument");
    // info[0..9]: the register path (L <= 64); info[10..15]: the workgroup path; info[16]:
    // the path phgpu_solve takes by default (1 global, 2 register, 3 workgroup); info[17]:
    // queue mode of the last register-path solve (1 record mode, 0 scenario order, -1 none)
    for (int k = 0; k < 20; ++k) info[k] = 0;
    info[18] = jit_eligible(h) ? 1 : 0;
    info[19] = h->jit ? h->jit->wpe : 0;
    info[17] = h->last_rec;
    info[0] = h->reg_inst;
    info[1] = h->reg_inst >= 0 ? h->reg_L : 0;
    info[2] = h->reg_kc;
    info[3] = h->reg_zc;
    info[4] = h->reg_kr;
    info[5] = h->reg_zr;
    if (h->reg_inst >= 0) {
        const reg_instance& r = g_reg_instances[h->reg_inst];
        info[6] = r.KC;
        info[7] = r.ZC;
        info[8] = r.KR;
        info[9] = r.ZR;
    }
    info[10] = h->wg_inst;
    if (h->wg_inst >= 0) {
        const wg_instance& g = g_wg_instances[h->wg_inst];
        info[11] = g.WPS;
        info[12] = g.KC;
        info[13] = g.ZC;
        info[14] = g.KR;
        info[15] = g.ZR;
    }
    info[16] = h->scen_set && !h->shared ? default_path(h) : h->default_kernel;
    return 0;
}

extern "C" int64_t phgpu_ipm_prof(phgpu_handle h, unsigned long long* out, int64_t n) {
    if (!h) return set_err(-1, "null handle");
    if (!h->ipm_prof) return 0;
    const int64_t k = n < h->ipm_prof_n ? n : h->ipm_prof_n;
    if (out && k > 0 &&
        (hipDeviceSynchronize() != hipSuccess ||
         hipMemcpy(out, h->ipm_prof, k * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess))
        return set_err(-2, "phgpu_ipm_prof: copy failed");
    return h->ipm_prof_n;
}

extern "C" int phgpu_ipm_info(phgpu_handle h, double* info) {
    if (!h || !info) return set_err(-1, "null argument");
    for (int k = 0; k < 16; ++k) info[k] = 0.0;
    info[0] = ipm_eligible(h) ? 1.0 : 0.0;
    info[11] = (double)h->folded;
    info[1] = h->ipm_nf;
    info[2] = h->ipm_off;
    if (h->ipm) {
        info[3] = 1.0;
        info[4] = h->ipm->mr;
        info[5] = h->ipm->nf;
        info[6] = h->ipm->private_bytes;
        info[7] = h->ipm->compile_s;
        info[8] = h->ipm->fac_flops;
        info[9] = h->ipm->sol_flops;
        info[10] = h->ipm->L;
        info[12] = h->ipm->L == 1 ? 1 : (h->ipm->L < 64 ? 2 : (h->ipm->blk ? 4 : 3));
        info[15] = h->ipm->L == 1 && h->ipm_lds == 1 ? 1.0 : 0.0;
    }
    // the subtree kernel's jam statistics of the last path-6 solve (synchronous read)
    if (h->last_stats && h->ipm_stats && h->last_path == 6) {
        std::vector<unsigned long long> st(PHGPU_STATS_WORDS);
        // the solve may still run on a non-blocking stream (a torch side stream, the
        // speculative launch), which hipMemcpy does not wait for: finish it first
        if (hipDeviceSynchronize() == hipSuccess &&
            hipMemcpy(st.data(), h->last_stats, PHGPU_STATS_WORDS * sizeof(unsigned long long),
                      hipMemcpyDeviceToHost) == hipSuccess) {
            info[13] = (double)stats_word(st.data(), PHGPU_STATS_COPIES, 6);
            info[14] = (double)stats_word(st.data(), PHGPU_STATS_COPIES, 7);
        }
    }
    return 0;
}
