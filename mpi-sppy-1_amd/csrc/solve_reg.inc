// solve_reg.inc -- register-resident batched PDHG (included by phgpu.hip).
//
// Mapping (DESIGN.md section 3.3): a 64-lane wavefront holds G = 64 / L scenarios, each
// split over L consecutive lanes.  Lane l of a scenario owns
//   columns j = l + q L  (q < KC, compile-time slots) and
//   rows    i = l + r L  (r < KR, compile-time slots).
// What a PDHG iteration touches lives in VGPRs: the iterate and its Halpern anchor
// (x, x0, A^T y, its anchor, y, y0), the scaled cost, prox reciprocal and bounds, and
// each slot's CSC / CSR entries (ZC / ZR padded: value + 32-bit LDS address of the
// partner slot, so a gather is one ds_read_b64).  Only the two vectors that cross lanes
// go through LDS: the extrapolated primal x~ = 2 T(x) - x (written by column owners,
// gathered by row owners) and T(y) (written by row owners, gathered by column owners).
// What only the restart / KKT checks need -- per-scenario norms, objective constant,
// step size, primal weight, restart residuals, and per-slot quadratic / scaling factors
// -- is parked in LDS next to the exchange vectors, so it costs no VGPRs in the loop.
//
// Schedule: a wave runs CHUNKS of `restart_every` iterations.  The first iteration of a
// chunk also forms ||z - T(z)|| when a scenario has just (re)started; the middle ones
// are the bare PDHG + Halpern step; the last one is the check iteration (restart test,
// every check_every / restart_every chunks the KKT test, iteration cap).  Scenarios
// finish only at chunk ends, so refills (persistent work queue, one atomic per wave per
// refill) never interrupt a chunk.  HBM is touched only when a scenario is loaded and
// written back.

struct reg_plan {
    int L;                 // lanes per scenario (power of two <= 64)
    int kc, zc, kr, zr;    // actual per-lane maxima (<= the instance's template bounds)
    const int32_t* col_k;  // [L][kc][zc] CSR position of the column entry, -1 = pad
    const int32_t* col_r;  // [L][kc][zc] its row
    const int32_t* row_k;  // [L][kr][zr] CSR position of the row entry, -1 = pad
    const int32_t* row_c;  // [L][kr][zr] its column
    // record mode (template REC): scenarios come from the work queue in order[] (longest first
    // by the predicted iteration counts last_iters, k_reg_order) and are loaded from / written
    // back to their scenario-major record pk (phgpu.hip), so a group's loads and stores are
    // contiguous whatever scenarios its neighbours hold; x / y reach the caller's layout
    // by k_from_records after the launch.  Otherwise: scenario order, [k][S] arrays.
    const int32_t* order;  // [S] queue position -> scenario (REC)
    int32_t* last_iters;   // [S] predicted PDHG iterations of this solve (its queue order)
    int32_t* last_iters_w; // [S] the prediction for the next solve (== last_iters unless deferred)
    int ema;               // 1: last_iters <- 0.7 last_iters + 0.3 iterations (else: iterations)
};

typedef __attribute__((address_space(3))) double lds_double;

// cross-lane move of an fp64 value with a DPP pattern (two v_mov_b32_dpp, VALU only)
template <int CTRL>
__device__ __forceinline__ double dpp64(double v) {
    const long long b = __builtin_bit_cast(long long, v);
    const int lo = __builtin_amdgcn_mov_dpp((int)b, CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_mov_dpp((int)(b >> 32), CTRL, 0xF, 0xF, false);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);
}

// sum over the L lanes of a group (L a power of two, groups aligned).  Up to 16 lanes the
// exchange is DPP: quad_perm [1,0,3,2] and [2,3,0,1] make quad sums, row_half_mirror
// (i -> 7 - i) pairs the two quads of an 8-lane half-row, row_mirror (i -> 15 - i) the two
// halves of a row; wider groups continue with __shfl_xor.  Every lane of a group ends
// with the same bits (each step adds the same two operands, in either order), which the
// group's uniform restart / termination decisions rely on.
__device__ __forceinline__ double group_sum(double v, int L) {
    if (L >= 2) v += dpp64<0xB1>(v);
    if (L >= 4) v += dpp64<0x4E>(v);
    if (L >= 8) v += dpp64<0x141>(v);
    if (L >= 16) v += dpp64<0x140>(v);
    for (int o = 16; o < L; o <<= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}

// 1 / (k + 2) for the Halpern weights: the hardware reciprocal alone.  The weights need
// not be correctly rounded, only deterministic and in (0, 1/2]; a Newton step on top
// cost two fp64 instructions per iteration for no change in iteration counts.
__device__ __forceinline__ double halpern_a0(int k) {
    return __builtin_amdgcn_rcp(k + 2.0);
}

// a / b for b > 0 finite on the restart / check paths: reciprocal + one Newton step (4
// instructions instead of the ~10 of a correctly rounded fp64 division; deterministic)
__device__ __forceinline__ double fdiv(double a, double b) {
    double r = __builtin_amdgcn_rcp(b);
    r = fma(r, fma(-b, r, 1.0), r);
    return a * r;
}

// fp64 min / max as single instructions: the compiler otherwise re-canonicalises the
// loop-invariant bounds (an extra v_max_f64 per operand) inside the hot loop
__device__ __forceinline__ double vmax64(double a, double b) {
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ double vmin64(double a, double b) {
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ double vclamp(double v, double lo, double hi) { return vmin64(vmax64(v, lo), hi); }

// dual_prox (phgpu.hip) for rl <= ru in the form max(v + sig rl, min(v + sig ru, 0)):
// equal to it whenever rl <= ru (a = v + sig rl <= b = v + sig ru), two fewer
// instructions; srl / sru are sig * rlh / sig * ruh (+-inf allowed)
__device__ __forceinline__ double dual_prox_v(double v, double srl, double sru) {
    return vmax64(v + srl, vmin64(v + sru, 0.0));
}

__device__ __forceinline__ uint32_t lds_addr(const double* p) {
    return (uint32_t)(size_t)(lds_double*)p;
}

__device__ __forceinline__ double lds_ld(uint32_t a) { return *(lds_double*)(size_t)a; }
__device__ __forceinline__ void lds_st(uint32_t a, double v) { *(lds_double*)(size_t)a = v; }

// LDS hand-off between lanes of ONE wavefront (waves never share LDS data; no
// s_barrier).  The LDS executes one wave's DS instructions in issue order (the AMDGPU
// memory model makes wavefront-scope fences free for this reason), so a read issued
// after a write sees it: only the compiler must not move LDS accesses across the
// hand-off.  REG_LDS_WAIT=1 restores the explicit drain (s_waitcnt lgkmcnt(0)) between
// the writes and the reads.
#ifndef REG_LDS_WAIT
#define REG_LDS_WAIT 0
#endif
#if REG_LDS_WAIT
#define WSYNC() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
#else
#define WSYNC() asm volatile("" ::: "memory")
#endif

// per-group record in LDS (cold scalars, identical on the group's L lanes)
enum { GR_CNORM, GR_BNORM, GR_CTERM, GR_ETA, GR_OMEGA, GR_R0, GR_RLAST, GR_POBJ, GR_DOBJ, GR_N };

// doubles of LDS one wave needs (host and device agree on this)
__host__ __device__ inline size_t reg_wave_lds(int n, int m, int G, int KC, int KR) {
    return (size_t)G * (n + m + 2) + (size_t)G * GR_N + (size_t)(2 * KC + KR) * WAVE;
}

// A workgroup holds REG_WPB independent waves (they share nothing but the LDS
// allocation): multi-wave workgroups let the VGPR budget, not the per-CU workgroup-slot
// limit, set occupancy.
#define REG_WPB 4
#ifndef REG_WAVES_PER_EU
#define REG_WAVES_PER_EU 2
#endif

// wide-row instances (ZR > 8) serve few large scenarios (one per wave): they trade
// occupancy for the VGPRs their padded rows need
template <int ZR>
struct reg_waves { static constexpr int value = ZR > 8 ? 1 : REG_WAVES_PER_EU; };

template <int KC, int ZC, int KR, int ZR, bool REC>
__global__ void __launch_bounds__(WAVE * REG_WPB) __attribute__((amdgpu_waves_per_eu(reg_waves<ZR>::value)))
k_solve_reg(pdhg_view st, solve_params P, reg_plan pl, int* __restrict__ qhead, int64_t first_dyn,
            double* __restrict__ xout, double* __restrict__ yout, double* __restrict__ obj,
            double* __restrict__ bound, int32_t* __restrict__ status, int32_t* __restrict__ iters) {
    extern __shared__ double lds[];
    const int L = pl.L;
    const int G = WAVE / L;
    const int wv = threadIdx.x / WAVE;
    const int t = threadIdx.x - wv * WAVE;
    const int g = t / L;
    const int l = t - g * L;
    const int64_t S = st.S;
    const int n = st.n, m = st.m;
    double* wbase = lds + (size_t)wv * reg_wave_lds(n, m, G, KC, KR);
    double* xe_s = wbase + (size_t)g * (n + m + 2);       // [n + 1]  (slot n = pad)
    double* yt_s = xe_s + n + 1;                          // [m + 1]  (slot m = pad)
    double* gr = wbase + (size_t)G * (n + m + 2) + (size_t)g * GR_N;
    double* cold = wbase + (size_t)G * (n + m + 2) + (size_t)G * GR_N;
#define QH(q) cold[(q) * WAVE + t]
#define DC(q) cold[(KC + (q)) * WAVE + t]
#define DR(r) cold[(2 * KC + (r)) * WAVE + t]
    const double bs2 = P.bsuff * P.bsuff, bn2 = P.bnec * P.bnec;
    const int R = P.restart_every;
    const int kkt_every = P.check_every / P.restart_every;

    // hot per-lane state (VGPRs)
    uint32_t jadr[KC];                       // LDS address of x~_j (pad slot if not owned)
    double x[KC], x0[KC], aty[KC], aty0[KC], ch[KC], dinv[KC], lbh[KC], ubh[KC];
    double ac[KC][ZC];
    uint32_t rca[KC][ZC];                    // LDS addresses of T(y) partners
    uint32_t iadr[KR];                       // LDS address of T(y)_i
    double y[KR], y0[KR], rlh[KR], ruh[KR];
    double ar[KR][ZR];
    uint32_t cra[KR][ZR];                    // LDS addresses of x~ partners
    bool jown[KC], iown[KR];
    double tau = 0.0, sig = 0.0;
    int hk = 0, it = 0;

    int64_t s = ((int64_t)blockIdx.x * REG_WPB + wv) * G + g;  // static first queue position
    bool fresh = s < S, active = false, exhausted = !fresh && first_dyn >= S;
    if (REC && fresh) s = pl.order[s];
    const double* __restrict__ pk = st.pk;
    int chunk = 0;

    auto set_steps = [&](double omega) {
        const double eta = gr[GR_ETA];
        tau = fdiv(eta, omega);
        sig = eta * omega;
#pragma unroll
        for (int q = 0; q < KC; ++q) {
            const double qq = QH(q);
            dinv[q] = (qq != 0.0) ? fdiv(1.0, 1.0 + tau * qq) : 1.0;
        }
    };

    while (true) {
        // ---------------------------------------------- refill from the queue
        const bool need = !active && !fresh && !exhausted;
        const unsigned long long lead = __ballot(need && l == 0);
        if (lead) {
            int base = 0;
            if (t == 0) base = atomicAdd(qhead, __popcll(lead));
            base = __shfl(base, 0, WAVE);
            if (need) {
                const unsigned long long below = lead & ((1ull << (g * L)) - 1ull);
                const int64_t cand = first_dyn + base + __popcll(below);
                if (cand < S) {
                    s = REC ? (int64_t)pl.order[cand] : cand;
                    fresh = true;
                } else {
                    exhausted = true;
                }
            }
        }
        // ---------------------------------------------- load a scenario
        if (fresh) {
            double cn2 = 0.0, ct = 0.0, bn2v = 0.0;
            // element k of field f of this scenario: record pk[s][f + k] or array f[k][S]
            const double* rec = REC ? pk + (size_t)s * (size_t)st.pk_stride : nullptr;
#define LDF(arr, roff, k) (REC ? rec[(roff) + (k)] : (arr)[IX(k)])
#pragma unroll
            for (int q = 0; q < KC; ++q) {
                const int j = l + q * L;
                const bool own = q < pl.kc && j < n;
                jown[q] = own;
                jadr[q] = lds_addr(xe_s + (own ? j : n));
                x[q] = x0[q] = aty[q] = aty0[q] = 0.0;
                ch[q] = lbh[q] = ubh[q] = 0.0;
                double qq = 0.0, d = 1.0;
                if (own) {
                    double cj = LDF(st.c, st.pk_C, j);
                    double qj = LDF(st.q, st.pk_Q, j);
                    const int k = st.nonant_slot[j];
                    if (k >= 0) {
                        if (st.W_on) cj += LDF(st.W, st.pk_W, k);
                        if (st.prox_on) {
                            const double r = LDF(st.rho, st.pk_RHO, k), xb = LDF(st.xbar, st.pk_XB, k);
                            cj -= r * xb;
                            qj += r;
                            ct += 0.5 * r * xb * xb;
                        }
                    }
                    d = LDF(st.Dc, st.pk_DC, j);
                    ch[q] = d * cj;
                    qq = d * d * qj;
                    cn2 += cj * cj;
                    lbh[q] = LDF(st.lbh, st.pk_LB, j);
                    ubh[q] = LDF(st.ubh, st.pk_UB, j);
                    x[q] = clampd(P.warm ? LDF(st.x, st.pk_X, j) : 0.0, lbh[q], ubh[q]);
                    x0[q] = x[q];
                }
                QH(q) = qq;
                DC(q) = d;
#pragma unroll
                for (int z = 0; z < ZC; ++z) {
                    const int idx = (l * pl.kc + q) * pl.zc + z;
                    const int k = (own && z < pl.zc) ? pl.col_k[idx] : -1;
                    rca[q][z] = lds_addr(yt_s + ((k >= 0) ? pl.col_r[idx] : m));
                    ac[q][z] = (k >= 0) ? LDF(st.Ah_csr, st.pk_A, k) : 0.0;
                }
            }
#pragma unroll
            for (int r = 0; r < KR; ++r) {
                const int i = l + r * L;
                const bool own = r < pl.kr && i < m;
                iown[r] = own;
                iadr[r] = lds_addr(yt_s + (own ? i : m));
                y[r] = y0[r] = 0.0;
                rlh[r] = ruh[r] = 0.0;
                double d = 1.0;
                if (own) {
                    const double a = LDF(st.rl, st.pk_RL, i), b = LDF(st.ru, st.pk_RU, i);
                    if (isfinite(a)) bn2v += a * a;
                    if (isfinite(b) && b != a) bn2v += b * b;
                    d = LDF(st.Dr, st.pk_DR, i);
                    rlh[r] = LDF(st.rlh, st.pk_RLH, i);
                    ruh[r] = LDF(st.ruh, st.pk_RUH, i);
                    y[r] = y0[r] = P.warm ? LDF(st.y, st.pk_Y, i) : 0.0;
                }
                DR(r) = d;
#pragma unroll
                for (int z = 0; z < ZR; ++z) {
                    const int idx = (l * pl.kr + r) * pl.zr + z;
                    const int k = (own && z < pl.zr) ? pl.row_k[idx] : -1;
                    cra[r][z] = lds_addr(xe_s + ((k >= 0) ? pl.row_c[idx] : n));
                    ar[r][z] = (k >= 0) ? LDF(st.Ah_csr, st.pk_A, k) : 0.0;
                }
            }
#undef LDF
            const double cnorm = sqrt(group_sum(cn2, L));
            const double cterm = group_sum(ct, L) + st.objc[s];
            const double bnorm = sqrt(group_sum(bn2v, L));
            double omega = st.omega[s];
            if (!(P.keep_omega && P.warm) && P.omega0 > 0.0) omega = P.omega0;
            gr[GR_CNORM] = cnorm;
            gr[GR_BNORM] = bnorm;
            gr[GR_CTERM] = cterm;
            gr[GR_ETA] = P.eta_frac / st.normA[s];
            gr[GR_OMEGA] = omega;
            gr[GR_R0] = -1.0;
            gr[GR_RLAST] = INFINITY;
            // A^T y of the start point (y through this group's T(y) exchange slots)
#pragma unroll
            for (int r = 0; r < KR; ++r) lds_st(iadr[r], y[r]);
            if (l == 0) {
                xe_s[n] = 0.0;
                yt_s[m] = 0.0;
            }
            WSYNC();
#pragma unroll
            for (int q = 0; q < KC; ++q) {
                double a = 0.0;
#pragma unroll
                for (int z = 0; z < ZC; ++z) a += ac[q][z] * lds_ld(rca[q][z]);
                aty[q] = aty0[q] = a;
            }
            set_steps(omega);
            hk = 0;
            it = 0;
            active = true;
            fresh = false;
        }
        WSYNC();
        if (!__any(active)) break;

        // ---------------------------------------------- first iteration of the chunk:
        // the residual ||z - T(z)||^2 of a scenario that just (re)started
        const bool need_r0 = active && gr[GR_R0] < 0.0;
        const bool any_r0 = __any(need_r0);
        // ---------------------------------------------- R - 1 plain PDHG + Halpern steps
        for (int k = 0; k < R - 1; ++k) {
            const double a0 = halpern_a0(hk);
            double dx2 = 0.0, dy2 = 0.0;
            const bool norms = any_r0 && k == 0;
            // Halpern step z+ = (1 - a0) R(z) + a0 z0, written R + a0 (z0 - R)
#pragma unroll
            for (int q = 0; q < KC; ++q) {
                const double xj = x[q];
                const double v = vclamp((xj - tau * (ch[q] - aty[q])) * dinv[q], lbh[q], ubh[q]);
                // gamma = 1: the reflected point 2 T(x) - x is both x~ and the Halpern R(x)
                const double e = fma(2.0, v, -xj);
                lds_st(jadr[q], e);
                if (norms) {
                    const double d = v - xj;
                    dx2 += d * d;
                }
                x[q] = fma(a0, x0[q] - e, e);
            }
            WSYNC();
            double gx[KR][ZR];
#pragma unroll
            for (int r = 0; r < KR; ++r)
#pragma unroll
                for (int z = 0; z < ZR; ++z) gx[r][z] = lds_ld(cra[r][z]);
#pragma unroll
            for (int r = 0; r < KR; ++r) {
                double ax = 0.0;
#pragma unroll
                for (int z = 0; z < ZR; ++z) ax = fma(ar[r][z], gx[r][z], ax);
                const double yi = y[r];
                const double v = dual_prox_v(yi - sig * ax, sig * rlh[r], sig * ruh[r]);
                lds_st(iadr[r], v);
                if (norms) {
                    const double d = v - yi;
                    dy2 += d * d;
                }
                const double e = fma(2.0, v, -yi);
                y[r] = fma(a0, y0[r] - e, e);
            }
            WSYNC();
            double gy[KC][ZC];
#pragma unroll
            for (int q = 0; q < KC; ++q)
#pragma unroll
                for (int z = 0; z < ZC; ++z) gy[q][z] = lds_ld(rca[q][z]);
#pragma unroll
            for (int q = 0; q < KC; ++q) {
                double a = 0.0;
#pragma unroll
                for (int z = 0; z < ZC; ++z) a = fma(ac[q][z], gy[q][z], a);
                const double e = fma(2.0, a, -aty[q]);
                aty[q] = fma(a0, aty0[q] - e, e);
            }
            if (norms) {
                dx2 = group_sum(dx2, L);
                dy2 = group_sum(dy2, L);
                if (need_r0) {
                    const double om = gr[GR_OMEGA];
                    gr[GR_R0] = om * dx2 + fdiv(dy2, om);
                }
            }
            ++hk;
        }

        // ---------------------------------------------- check iteration
        double xt[KC], atyt[KC], yt[KR];
        double dx2 = 0.0, dy2 = 0.0;
        {
#pragma unroll
            for (int q = 0; q < KC; ++q) {
                const double xj = x[q];
                const double v = vclamp((xj - tau * (ch[q] - aty[q])) * dinv[q], lbh[q], ubh[q]);
                const double d = v - xj;
                lds_st(jadr[q], fma(2.0, v, -xj));
                dx2 += d * d;
                xt[q] = v;
            }
            WSYNC();
            double gx[KR][ZR];
#pragma unroll
            for (int r = 0; r < KR; ++r)
#pragma unroll
                for (int z = 0; z < ZR; ++z) gx[r][z] = lds_ld(cra[r][z]);
#pragma unroll
            for (int r = 0; r < KR; ++r) {
                double ax = 0.0;
#pragma unroll
                for (int z = 0; z < ZR; ++z) ax = fma(ar[r][z], gx[r][z], ax);
                const double v = dual_prox_v(y[r] - sig * ax, sig * rlh[r], sig * ruh[r]);
                lds_st(iadr[r], v);
                const double d = v - y[r];
                dy2 += d * d;
                yt[r] = v;
            }
            WSYNC();
            double gy[KC][ZC];
#pragma unroll
            for (int q = 0; q < KC; ++q)
#pragma unroll
                for (int z = 0; z < ZC; ++z) gy[q][z] = lds_ld(rca[q][z]);
#pragma unroll
            for (int q = 0; q < KC; ++q) {
                double a = 0.0;
#pragma unroll
                for (int z = 0; z < ZC; ++z) a = fma(ac[q][z], gy[q][z], a);
                atyt[q] = a;
            }
        }
        it += R;
        dx2 = group_sum(dx2, L);
        dy2 = group_sum(dy2, L);
        double omega = gr[GR_OMEGA];
        const double r2 = omega * dx2 + fdiv(dy2, omega);
        bool conv = false;
        int infeas = 0;  // PHGPU_PRIMAL_INFEASIBLE / PHGPU_DUAL_INFEASIBLE once certified
        double pobj = 0.0, dobj = 0.0;
        const bool kkt = (chunk % kkt_every) == kkt_every - 1;
        ++chunk;
        if (kkt) {
            // KKT test on T(z) in the original space; A T(x) needs T(x) in the x~ slots
#pragma unroll
            for (int q = 0; q < KC; ++q) lds_st(jadr[q], xt[q]);
            if (l == 0) xe_s[n] = 0.0;
            WSYNC();
            double pres2 = 0.0, dres2 = 0.0, pp = 0.0, dd = 0.0;
#pragma unroll
            for (int r = 0; r < KR; ++r) {
                double ax = 0.0;
#pragma unroll
                for (int z = 0; z < ZR; ++z) ax = fma(ar[r][z], lds_ld(cra[r][z]), ax);
                if (iown[r]) {
                    const double idr = fdiv(1.0, DR(r));
                    const double axo = ax * idr;
                    const double rl = rlh[r] * idr, ru = ruh[r] * idr;
                    const double v = axo - clampd(axo, rl, ru);
                    pres2 += v * v;
                    dd += row_dual_term(yt[r] * DR(r), rl, ru);
                }
            }
#pragma unroll
            for (int q = 0; q < KC; ++q) {
                if (jown[q]) {
                    const double d = DC(q);
                    const double id = fdiv(1.0, d);
                    const double xo = d * xt[q];
                    const double ce = ch[q] * id, qe = QH(q) * id * id;
                    const double at = atyt[q] * id;
                    const double lbj = lbh[q] * d, ubj = ubh[q] * d;
                    const double rcst = ce + qe * xo - at;
                    double lam;
                    if (isfinite(lbj) && isfinite(ubj)) lam = rcst;
                    else if (isfinite(lbj)) lam = fmax(rcst, 0.0);
                    else if (isfinite(ubj)) lam = fmin(rcst, 0.0);
                    else lam = 0.0;
                    dres2 += (rcst - lam) * (rcst - lam);
                    pp += ce * xo + 0.5 * qe * xo * xo;
                    dd += col_dual_term(ce - at, qe, lbj, ubj);
                }
            }
            const double cterm = gr[GR_CTERM];
            pres2 = group_sum(pres2, L);
            dres2 = group_sum(dres2, L);
            pp = group_sum(pp, L) + cterm;
            dd = group_sum(dd, L) + cterm;
            const double tp = P.eps_abs + P.eps_rel * (1.0 + gr[GR_BNORM]);
            const double td = P.eps_abs + P.eps_rel * (1.0 + gr[GR_CNORM]);
            conv = active && pres2 <= tp * tp && dres2 <= td * td &&
                   fabs(pp - dd) <= P.eps_abs + P.eps_rel * (1.0 + fabs(pp) + fabs(dd));
            pobj = pp;
            dobj = dd;
            // infeasibility certificates from d = T(z) - z (phgpu.hip, ray_*_terms); only
            // once some scenario of the wave has run infeas_start iterations
            if (P.infeas_start >= 0 && __any(active && !conv && it >= P.infeas_start)) {
                double po = 0.0, pv = 0.0, cdx = 0.0, dv = 0.0;
#pragma unroll
                for (int q = 0; q < KC; ++q) lds_st(jadr[q], xt[q] - x[q]);
                if (l == 0) xe_s[n] = 0.0;
                WSYNC();
#pragma unroll
                for (int r = 0; r < KR; ++r) {
                    double adx = 0.0;
#pragma unroll
                    for (int z = 0; z < ZR; ++z) adx = fma(ar[r][z], lds_ld(cra[r][z]), adx);
                    if (iown[r]) {
                        const double idr = fdiv(1.0, DR(r));
                        const double rl = rlh[r] * idr, ru = ruh[r] * idr;
                        ray_row_terms(DR(r) * (yt[r] - y[r]), rl, ru, po, pv);
                        dv += recession_viol2(adx * idr, rl, ru);
                    }
                }
#pragma unroll
                for (int q = 0; q < KC; ++q) {
                    if (jown[q]) {
                        const double d = DC(q);
                        const double id = fdiv(1.0, d);
                        const double lbj = lbh[q] * d, ubj = ubh[q] * d;
                        ray_col_terms(-(atyt[q] - aty[q]) * id, lbj, ubj, po, pv);
                        const double dxo = d * (xt[q] - x[q]);
                        const double qe = QH(q) * id * id;
                        cdx += ch[q] * id * dxo;
                        dv += recession_viol2(dxo, lbj, ubj) + (qe * dxo) * (qe * dxo);
                    }
                }
                po = group_sum(po, L);
                pv = group_sum(pv, L);
                cdx = group_sum(cdx, L);
                dv = group_sum(dv, L);
                if (active && !conv && it >= P.infeas_start) {
                    if (is_certificate(po, pv, P.eps_inf)) infeas = PHGPU_PRIMAL_INFEASIBLE;
                    else if (is_certificate(-cdx, dv, P.eps_inf)) infeas = PHGPU_DUAL_INFEASIBLE;
                }
            }
        }
        const bool finished = active && (conv || infeas != 0 || it >= P.max_iter);
        if (active && !finished) {
            double r02 = gr[GR_R0];
            if (r02 < 0.0) r02 = r2;       // restart_every == 1: no plain step set it
            const double rlast2 = gr[GR_RLAST];
            const bool restart = (r2 <= bs2 * r02) || (r2 <= bn2 * r02 && r2 > rlast2) ||
                                 (hk + 1 >= P.bart * it);
            gr[GR_RLAST] = r2;
            if (restart) {
                double ddx = 0.0, ddy = 0.0;
#pragma unroll
                for (int q = 0; q < KC; ++q) {
                    const double d = xt[q] - x0[q];
                    ddx += d * d;
                    x[q] = x0[q] = xt[q];
                    aty[q] = aty0[q] = atyt[q];
                }
#pragma unroll
                for (int r = 0; r < KR; ++r) {
                    const double d = yt[r] - y0[r];
                    ddy += d * d;
                    y[r] = y0[r] = yt[r];
                }
                ddx = group_sum(ddx, L);           // squared norms
                ddy = group_sum(ddy, L);
                if (ddx > 1e-20 && ddy > 1e-20) {
                    // geometric mean of omega and ||dy|| / ||dx||: exp(0.5 log(ddy/ddx) + 0.5 log(omega))
                    // as hardware square roots (fp64 exp / log / correctly rounded sqrt are long
                    // software sequences; the weight only has to be deterministic)
                    const double ratio = __builtin_amdgcn_sqrt(fdiv(ddy, ddx));
                    omega = clampd(__builtin_amdgcn_sqrt(omega * ratio), P.wmin, P.wmax);
                    gr[GR_OMEGA] = omega;
                    set_steps(omega);
                }
                hk = 0;
                gr[GR_R0] = -1.0;
                gr[GR_RLAST] = INFINITY;
            } else {
                const double a0 = halpern_a0(hk);
#pragma unroll
                for (int q = 0; q < KC; ++q) {
                    const double ex = fma(2.0, xt[q], -x[q]);
                    const double ea = fma(2.0, atyt[q], -aty[q]);
                    x[q] = fma(a0, x0[q] - ex, ex);
                    aty[q] = fma(a0, aty0[q] - ea, ea);
                }
#pragma unroll
                for (int r = 0; r < KR; ++r) {
                    const double ey = fma(2.0, yt[r], -y[r]);
                    y[r] = fma(a0, y0[r] - ey, ey);
                }
                ++hk;
            }
        }
        // ---------------------------------------------- write back finished scenarios
        if (__any(finished)) {
            double pp = 0.0, dd = 0.0;
            if (finished && !conv) {
                // iteration cap: the answer is T(z) of this iteration (box-feasible)
#pragma unroll
                for (int r = 0; r < KR; ++r)
                    if (iown[r]) dd += row_dual_term(yt[r] * DR(r), rlh[r] / DR(r), ruh[r] / DR(r));
#pragma unroll
                for (int q = 0; q < KC; ++q) {
                    if (jown[q]) {
                        const double d = DC(q);
                        const double xo = d * xt[q];
                        const double ce = ch[q] / d, qe = QH(q) / (d * d);
                        pp += ce * xo + 0.5 * qe * xo * xo;
                        dd += col_dual_term(ce - atyt[q] / d, qe, lbh[q] * d, ubh[q] * d);
                    }
                }
            }
            pp = group_sum(pp, L);
            dd = group_sum(dd, L);
            if (finished) {
                if (!conv) {
                    pobj = pp + gr[GR_CTERM];
                    dobj = dd + gr[GR_CTERM];
                }
                if (infeas == PHGPU_PRIMAL_INFEASIBLE) pobj = dobj = INFINITY;
                if (infeas == PHGPU_DUAL_INFEASIBLE) pobj = dobj = -INFINITY;
                if (REC) {
                    // scaled x / y into the record (the warm start); the caller's x / y
                    // come from k_from_records after the launch
                    double* rec = st.pk + (size_t)s * (size_t)st.pk_stride;
#pragma unroll
                    for (int q = 0; q < KC; ++q)
                        if (jown[q]) rec[st.pk_XW + l + q * L] = xt[q];
#pragma unroll
                    for (int r = 0; r < KR; ++r)
                        if (iown[r]) rec[st.pk_YW + l + r * L] = yt[r];
                } else {
#pragma unroll
                    for (int q = 0; q < KC; ++q) {
                        if (jown[q]) {
                            const int j = l + q * L;
                            xout[IX(j)] = DC(q) * xt[q];
                            st.xw[IX(j)] = xt[q];
                        }
                    }
#pragma unroll
                    for (int r = 0; r < KR; ++r) {
                        if (iown[r]) {
                            const int i = l + r * L;
                            if (yout) yout[IX(i)] = DR(r) * yt[r];
                            st.yw[IX(i)] = yt[r];
                        }
                    }
                }
                if (l == 0) {
                    st.omega_w[s] = gr[GR_OMEGA];
                    obj[s] = pobj;
                    bound[s] = dobj;
                    status[s] = conv ? PHGPU_OPTIMAL : (infeas ? infeas : PHGPU_ITER_LIMIT);
                    if (iters) iters[s] = it;
                    // the next solve's predictor: an exponential average of the counts
                    // (rank-correlates better with the next count than the last count alone:
                    // simulated makespan -18% instead of -9% vs scenario order,
                    // tools/sim_queue.py on profiles/r02/s2/iters_S65536.npy)
                    if (pl.last_iters) pl.last_iters_w[s] = pl.ema ? (7 * pl.last_iters[s] + 3 * it + 5) / 10 : it;
                }
                active = false;
            }
        }
    }
#undef QH
#undef DC
#undef DR
}

// ------------------------------------------------------------------ longest-first queue
// Record mode orders the work queue by a prediction of each scenario's PDHG iterations
// (pl.last_iters: an exponential average of its previous counts), longest first: a
// launch ends with the scenario that finishes last, and with the long ones
// started first the tail is made of short ones.  A counting sort in ORDER_BINS bins of
// restart_every iterations (the longest bin also takes everything above it); ties go in
// any order, since a scenario's solve is the same whichever lanes run it.
__device__ __forceinline__ int order_bin(int it, int R) {
    const int k = it / R;
    return ORDER_BINS - 1 - (k < ORDER_BINS - 1 ? k : ORDER_BINS - 1);
}

static_assert(ORDER_BINS == 256, "k_reg_prep / k_reg_order index the bins by thread");

// The histogram of the queue keys and this solve's PH-state transpose into the records
// (k_to_records_ph) in ONE launch (they are independent): blocks [0, nh) build the histogram, the next gx * gy
// blocks are transpose tiles -- one dependent launch less per PH iteration
__global__ void __launch_bounds__(256) k_reg_prep(const int32_t* __restrict__ its, int64_t S, int R,
                                                  int32_t* __restrict__ bins, int nh, int gx,
                                                  const double* __restrict__ W, const double* __restrict__ rho,
                                                  const double* __restrict__ xbar, int nn, double* __restrict__ pk,
                                                  int64_t stride, int off) {
    __shared__ double tile[TT][TT + 1];
    if ((int)blockIdx.x >= nh) {
        const int b = (int)blockIdx.x - nh;
        to_records_ph_tile(tile, b % gx, b / gx, W, rho, xbar, nn, S, pk, stride, off);
        return;
    }
    int* h = (int*)&tile[0][0];  // ORDER_BINS ints
    h[threadIdx.x] = 0;
    __syncthreads();
    const int64_t s = (int64_t)blockIdx.x * ORDER_BINS + threadIdx.x;
    if (s < S) atomicAdd(&h[order_bin(its[s], R)], 1);
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&bins[threadIdx.x], h[threadIdx.x]);
}

// bins[0..NB) = histogram (k_reg_prep), bins[NB..2NB) = fill counters, both zero on entry;
// `other` = the bins of the other parity, which the next solve uses: block 0 zeroes them
// (no device-wide fence needed: the next launches see them)
// (block 0 also resets the solve kernel's queue head: one launch less than a memset)
__global__ void __launch_bounds__(ORDER_BINS) k_reg_order(const int32_t* __restrict__ its, int64_t S, int R,
                                                          int32_t* __restrict__ bins, int32_t* __restrict__ other,
                                                          int32_t* __restrict__ order, int* __restrict__ qhead) {
    __shared__ int base[ORDER_BINS], h[ORDER_BINS], res[ORDER_BINS];
    const int t = threadIdx.x;
    base[t] = bins[t];
    h[t] = 0;
    if (blockIdx.x == 0) {
        other[t] = 0;
        other[ORDER_BINS + t] = 0;
        if (t == 0) *qhead = 0;
    }
    __syncthreads();
    for (int o = 1; o < ORDER_BINS; o <<= 1) {  // inclusive prefix (Hillis-Steele)
        const int v = t >= o ? base[t - o] : 0;
        __syncthreads();
        base[t] += v;
        __syncthreads();
    }
    const int64_t s = (int64_t)blockIdx.x * ORDER_BINS + t;
    int b = 0, r = 0;
    if (s < S) {
        b = order_bin(its[s], R);
        r = atomicAdd(&h[b], 1);
    }
    __syncthreads();
    if (h[t]) res[t] = atomicAdd(&bins[ORDER_BINS + t], h[t]);
    __syncthreads();
    if (s < S) order[(b ? base[b - 1] : 0) + res[b] + r] = (int32_t)s;
}

// ------------------------------------------------------------------ instances
typedef void (*reg_kernel_t)(pdhg_view, solve_params, reg_plan, int*, int64_t, double*, double*,
                             double*, double*, int32_t*, int32_t*);

struct reg_instance {
    int KC, ZC, KR, ZR;
    reg_kernel_t fn, fn_rec;  // scenario order / record mode
};

#define REG_INST(a, b, c, d) {a, b, c, d, k_solve_reg<a, b, c, d, false>, k_solve_reg<a, b, c, d, true>}
static const reg_instance g_reg_instances[] = {
    // exact widths for the farmer / aircond patterns (column degree <= 3, row degree <= 4)
    REG_INST(1, 3, 1, 4), REG_INST(2, 3, 1, 4), REG_INST(3, 3, 1, 4), REG_INST(3, 3, 2, 4),
    REG_INST(5, 3, 2, 4),
    REG_INST(1, 4, 1, 4), REG_INST(2, 4, 1, 4), REG_INST(3, 4, 1, 4), REG_INST(4, 4, 1, 4),
    REG_INST(2, 4, 2, 4), REG_INST(3, 4, 2, 4), REG_INST(4, 4, 2, 4), REG_INST(6, 4, 2, 4),
    REG_INST(8, 4, 4, 4), REG_INST(1, 4, 1, 8), REG_INST(2, 4, 1, 8), REG_INST(2, 4, 2, 8),
    REG_INST(4, 4, 2, 8), REG_INST(2, 8, 1, 8), REG_INST(4, 8, 2, 8),
    // one wide row per scenario at L = 64 (farmer cm <= 10: the acreage row has 3 cm
    // entries, every other row <= 4; config 2 is cm = 10, n = 120, m = 61)
    REG_INST(1, 3, 1, 32), REG_INST(2, 3, 1, 32),
};
#undef REG_INST
