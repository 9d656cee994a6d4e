// solve_wg.inc -- workgroup-per-scenario register-resident PDHG (included by phgpu.hip
// after solve_reg.inc).  For scenarios too large for the L <= 64 lane groups of
// k_solve_reg: farmer cm = 64 (n = 768, m = 385, an acreage row of 192 entries; the
// HBM-scale variant of config 3) and cm = 10 (config 2, a 30-entry acreage row).
//
// Mapping (DESIGN.md section 3.4): one workgroup of L = 64 * WPS lanes holds ONE scenario
// at a time (persistent grid, scenario queue).  A host plan (build_wg_plan) assigns
// every column to a (slot q, lane t) pair and every row to a (slot r, lane t) pair; each
// slot keeps, as in k_solve_reg, its iterate, Halpern anchor, bounds and its CSC / CSR
// entries (padded to ZC / ZR) in VGPRs.  A row with more than ZR entries is a LONG row:
// it gets a whole wave slot -- its entries spread over the 64 lanes of one wave, summed
// by a wave reduction, after which every lane of the slot holds the same row value and
// lane 0 (the head) publishes T(y)_i.  Long columns work the same way for A^T y.
// Cross-lane vectors go through LDS: x~ = 2 T(x) - x (written by column heads, gathered
// by row slots) and T(y) (written by row heads, gathered by column slots), with one
// workgroup barrier after each write phase; scenario norms are wave reductions plus a
// fixed-order sum over the WPS waves (every lane ends with the same bits, which the
// uniform restart / termination decisions rely on).  HBM is touched when a scenario is
// loaded and written back, never inside the solve.

struct wg_plan {
    int L;                     // lanes per scenario = 64 * WPS
    int kc, zc, kr, zr;        // actual maxima (<= the instance's template bounds)
    const int32_t* col_id;     // [kc][L] column held by (slot q, lane t), -1 = none
    const int32_t* row_id;     // [kr][L] row held by (slot r, lane t), -1 = none
    const int32_t* col_long;   // [kc][WPS] 1: slot q of wave w holds one long column
    const int32_t* row_long;   // [kr][WPS] 1: slot r of wave w holds one long row
    const int32_t* col_k;      // [kc][L][zc] CSR position of the entry, -1 = pad
    const int32_t* col_r;      // [kc][L][zc] its row
    const int32_t* row_k;      // [kr][L][zr] CSR position of the entry, -1 = pad
    const int32_t* row_c;      // [kr][L][zr] its column
};

// workgroup barrier for the LDS hand-offs: no global loads are in flight in the solve
// loop, so the wait is on the LDS counter only (a plain __syncthreads() also waits vmcnt).
// A one-wave workgroup (WPS = 1) needs neither: its DS instructions execute in issue
// order (the register path's hand-off, solve_reg.inc WSYNC), so only the compiler barrier
// stays.  Used inside templates with WPS in scope.
#define BSYNC()                                                        \
    do {                                                               \
        if (WPS > 1) {                                                 \
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");         \
            __builtin_amdgcn_s_barrier();                              \
        }                                                              \
        asm volatile("" ::: "memory");                                 \
    } while (0)

// doubles of LDS one workgroup needs (host and device agree on this)
__host__ __device__ inline size_t wg_lds_doubles(int n, int m, int KC, int KR, int WPS) {
    return (size_t)(n + 1) + (m + 1) + GR_N + 8 * WPS + 2 + (size_t)(2 * KC + KR) * WAVE * WPS;
}

// sum of NV values over the whole workgroup: wave sums (group_sum over 64 lanes), then
// the WPS wave partials added in wave order by every lane (identical bits everywhere).
// ``red`` holds two [4][WPS] halves used alternately: two consecutive calls never touch
// the same half, and a barrier separates a call's reads from the next-but-one's writes.
template <int WPS, int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV], double* red, int& parity, int wv, int lane) {
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = group_sum(v[i], WAVE);
    if (WPS == 1) return;
    double* r = red + parity * 4 * WPS;
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) r[i * WPS + wv] = v[i];
    }
    BSYNC();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        double a = 0.0;
#pragma unroll
        for (int w = 0; w < WPS; ++w) a += r[i * WPS + w];
        v[i] = a;
    }
    parity ^= 1;
}

#ifndef WG_WAVES_PER_EU
#define WG_WAVES_PER_EU 2
#endif

template <int KC, int ZC, int KR, int ZR, int WPS>
__global__ void __launch_bounds__(WAVE * WPS) __attribute__((amdgpu_waves_per_eu(WG_WAVES_PER_EU)))
k_solve_wg(pdhg_view st, solve_params P, wg_plan pl, int* __restrict__ qhead,
           double* __restrict__ xout, double* __restrict__ yout, double* __restrict__ obj,
           double* __restrict__ bound, int32_t* __restrict__ status, int32_t* __restrict__ iters) {
    extern __shared__ double lds[];
    constexpr int L = WAVE * WPS;
    const int t = threadIdx.x;
    const int wv = __builtin_amdgcn_readfirstlane(t / WAVE);
    const int lane = t & (WAVE - 1);
    const int64_t S = st.S;
    const int n = st.n, m = st.m;
    double* xe_s = lds;                          // [n + 1]  (slot n = pad)
    double* yt_s = xe_s + n + 1;                 // [m + 1]  (slot m = pad)
    double* gr = yt_s + m + 1;                   // [GR_N]   scenario record
    double* red = gr + GR_N;                     // [2][4][WPS] cross-wave sums
    double* bcast = red + 8 * WPS;               // [2]      scenario id hand-off
    double* cold = bcast + 2;                    // [2 KC + KR][L]
#define QH(q) cold[(q) * L + t]
#define DC(q) cold[(KC + (q)) * L + t]
#define DR(r) cold[(2 * KC + (r)) * L + t]
    const double bs2 = P.bsuff * P.bsuff, bn2 = P.bnec * P.bnec;
    const int R = P.restart_every;
    const int kkt_every = P.check_every / P.restart_every;
    int parity = 0;

    // slot ownership (fixed for the launch: the pattern is shared by all scenarios)
    int jcol[KC], irow[KR];
    bool jown[KC], iown[KR], clong[KC], rlong[KR];
    uint32_t jadr[KC], iadr[KR];
#pragma unroll
    for (int q = 0; q < KC; ++q) {
        const int j = q < pl.kc ? pl.col_id[q * L + t] : -1;
        clong[q] = q < pl.kc && pl.col_long[q * WPS + wv] != 0;
        jcol[q] = j;
        jown[q] = j >= 0 && (!clong[q] || lane == 0);
        jadr[q] = lds_addr(xe_s + (jown[q] ? j : n));
    }
#pragma unroll
    for (int r = 0; r < KR; ++r) {
        const int i = r < pl.kr ? pl.row_id[r * L + t] : -1;
        rlong[r] = r < pl.kr && pl.row_long[r * WPS + wv] != 0;
        irow[r] = i;
        iown[r] = i >= 0 && (!rlong[r] || lane == 0);
        iadr[r] = lds_addr(yt_s + (iown[r] ? i : m));
    }
    // partner addresses (LDS) of every slot entry, also launch-invariant
    uint32_t rca[KC][ZC], cra[KR][ZR];
#pragma unroll
    for (int q = 0; q < KC; ++q)
#pragma unroll
        for (int z = 0; z < ZC; ++z) {
            const int idx = (q * L + t) * pl.zc + z;
            const int k = (jcol[q] >= 0 && z < pl.zc) ? pl.col_k[idx] : -1;
            rca[q][z] = lds_addr(yt_s + ((k >= 0) ? pl.col_r[idx] : m));
        }
#pragma unroll
    for (int r = 0; r < KR; ++r)
#pragma unroll
        for (int z = 0; z < ZR; ++z) {
            const int idx = (r * L + t) * pl.zr + z;
            const int k = (irow[r] >= 0 && z < pl.zr) ? pl.row_k[idx] : -1;
            cra[r][z] = lds_addr(xe_s + ((k >= 0) ? pl.row_c[idx] : n));
        }

    // hot per-lane state (VGPRs)
    double x[KC], x0[KC], aty[KC], aty0[KC], ch[KC], dinv[KC], lbh[KC], ubh[KC];
    double ac[KC][ZC];
    double y[KR], y0[KR], rlh[KR], ruh[KR];
    double ar[KR][ZR];
    double tau = 0.0, sig = 0.0;

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

    int s = blockIdx.x;                        // scenario ids fit int (S < 2^31, checked at create)
    while (s < S) {
        // ------------------------------------------------------------ load scenario s
        // (one contiguous record per scenario: full-line loads, phgpu.hip pack_alloc)
        double* __restrict__ rec = st.pk + (size_t)s * (size_t)st.pk_stride;
        double nrm[3] = {0.0, 0.0, 0.0};   // ||c||^2, const term, ||b||^2 (heads only)
#pragma unroll
        for (int q = 0; q < KC; ++q) {
            const int j = jcol[q];
            x[q] = x0[q] = aty[q] = aty0[q] = 0.0;
            ch[q] = lbh[q] = ubh[q] = 0.0;
            double qq = 0.0, d = 1.0;
            if (j >= 0) {
                double cj = rec[st.pk_C + j];
                double qj = rec[st.pk_Q + j];
                const int k = st.nonant_slot[j];
                double ct = 0.0;
                if (k >= 0) {
                    if (st.W_on) cj += rec[st.pk_W + k];
                    if (st.prox_on) {
                        const double r = rec[st.pk_RHO + k], xb = rec[st.pk_XB + k];
                        cj -= r * xb;
                        qj += r;
                        ct = 0.5 * r * xb * xb;
                    }
                }
                d = rec[st.pk_DC + j];
                ch[q] = d * cj;
                qq = d * d * qj;
                if (jown[q]) {
                    nrm[0] += cj * cj;
                    nrm[1] += ct;
                }
                lbh[q] = rec[st.pk_LB + j];
                ubh[q] = rec[st.pk_UB + j];
                x[q] = x0[q] = clampd(P.warm ? rec[st.pk_X + j] : 0.0, lbh[q], ubh[q]);
            }
            QH(q) = qq;
            DC(q) = d;
#pragma unroll
            for (int z = 0; z < ZC; ++z) {
                const int k = (j >= 0 && z < pl.zc) ? pl.col_k[(q * L + t) * pl.zc + z] : -1;
                ac[q][z] = k >= 0 ? rec[st.pk_A + k] : 0.0;
            }
            // one slot's loads at a time: keeps the scheduler from hoisting every record
            // load of the scenario at once (register pressure of the load phase)
            asm volatile("" ::: "memory");
        }
#pragma unroll
        for (int r = 0; r < KR; ++r) {
            const int i = irow[r];
            y[r] = y0[r] = 0.0;
            rlh[r] = ruh[r] = 0.0;
            double d = 1.0;
            if (i >= 0) {
                const double a = rec[st.pk_RL + i], b = rec[st.pk_RU + i];
                if (iown[r]) {
                    if (isfinite(a)) nrm[2] += a * a;
                    if (isfinite(b) && b != a) nrm[2] += b * b;
                }
                d = rec[st.pk_DR + i];
                rlh[r] = rec[st.pk_RLH + i];
                ruh[r] = rec[st.pk_RUH + i];
                y[r] = y0[r] = P.warm ? rec[st.pk_Y + i] : 0.0;
            }
            DR(r) = d;
#pragma unroll
            for (int z = 0; z < ZR; ++z) {
                const int k = (i >= 0 && z < pl.zr) ? pl.row_k[(r * L + t) * pl.zr + z] : -1;
                ar[r][z] = k >= 0 ? rec[st.pk_A + k] : 0.0;
            }
            asm volatile("" ::: "memory");
        }
        block_sum<WPS, 3>(nrm, red, parity, wv, lane);
        double omega = st.omega[s];
        if (!(P.keep_omega && P.warm) && P.omega0 > 0.0) omega = P.omega0;
        if (t == 0) {
            gr[GR_CNORM] = sqrt(nrm[0]);
            gr[GR_CTERM] = nrm[1] + st.objc[s];
            gr[GR_BNORM] = sqrt(nrm[2]);
            gr[GR_ETA] = P.eta_frac / st.normA[s];
            gr[GR_OMEGA] = omega;
            gr[GR_R0] = -1.0;
            gr[GR_RLAST] = INFINITY;
            xe_s[n] = 0.0;
            yt_s[m] = 0.0;
        }
        // A^T y of the start point through the T(y) exchange slots
#pragma unroll
        for (int r = 0; r < KR; ++r) lds_st(iadr[r], y[r]);
        BSYNC();
        if (t == 0) yt_s[m] = 0.0;   // pad slot may have been written by non-head lanes
        BSYNC();
#pragma unroll
        for (int q = 0; q < KC; ++q) {
            double a = 0.0;
#pragma unroll
            for (int z = 0; z < ZC; ++z) a += ac[q][z] * lds_ld(rca[q][z]);
            if (clong[q]) a = group_sum(a, WAVE);
            aty[q] = aty0[q] = a;
        }
        set_steps(omega);
        int hk = 0, it = 0, chunk = 0;
        int stat = -1;
        double pobj = 0.0, dobj = 0.0;
        double xt[KC], atyt[KC], yt[KR];

        while (true) {
            // -------------------------------------------------- R - 1 plain steps
            const bool need_r0 = gr[GR_R0] < 0.0;
            for (int k = 0; k < R - 1; ++k) {
                const double a0 = halpern_a0(hk);
                double nx[2] = {0.0, 0.0};
                const bool norms = need_r0 && k == 0;
#pragma unroll
                for (int q = 0; q < KC; ++q) {
                    const double xj = x[q];
                    const double v = vclamp((xj - tau * (ch[q] - aty[q])) * dinv[q], lbh[q], ubh[q]);
                    const double e = fma(2.0, v, -xj);
                    lds_st(jadr[q], e);
                    if (norms && jown[q]) {
                        const double d = v - xj;
                        nx[0] += d * d;
                    }
                    x[q] = fma(a0, x0[q] - e, e);
                }
                BSYNC();
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
                    if (rlong[r]) ax = group_sum(ax, WAVE);
                    const double yi = y[r];
                    const double v = dual_prox_v(yi - sig * ax, sig * rlh[r], sig * ruh[r]);
                    lds_st(iadr[r], v);
                    if (norms && iown[r]) {
                        const double d = v - yi;
                        nx[1] += d * d;
                    }
                    const double e = fma(2.0, v, -yi);
                    y[r] = fma(a0, y0[r] - e, e);
                }
                BSYNC();
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
                    if (clong[q]) a = group_sum(a, WAVE);
                    const double e = fma(2.0, a, -aty[q]);
                    aty[q] = fma(a0, aty0[q] - e, e);
                }
                if (norms) {
                    block_sum<WPS, 2>(nx, red, parity, wv, lane);
                    const double om = gr[GR_OMEGA];
                    const double r0 = om * nx[0] + fdiv(nx[1], om);
                    BSYNC();                      // every lane has read GR_R0 / GR_OMEGA
                    if (t == 0) gr[GR_R0] = r0;
                }
                ++hk;
            }

            // -------------------------------------------------- check iteration
            double nx[2] = {0.0, 0.0};
#pragma unroll
            for (int q = 0; q < KC; ++q) {
                const double xj = x[q];
                const double v = vclamp((xj - tau * (ch[q] - aty[q])) * dinv[q], lbh[q], ubh[q]);
                lds_st(jadr[q], fma(2.0, v, -xj));
                if (jown[q]) {
                    const double d = v - xj;
                    nx[0] += d * d;
                }
                xt[q] = v;
            }
            BSYNC();
#pragma unroll
            for (int r = 0; r < KR; ++r) {
                double ax = 0.0;
#pragma unroll
                for (int z = 0; z < ZR; ++z) ax = fma(ar[r][z], lds_ld(cra[r][z]), ax);
                if (rlong[r]) ax = group_sum(ax, WAVE);
                const double v = dual_prox_v(y[r] - sig * ax, sig * rlh[r], sig * ruh[r]);
                lds_st(iadr[r], v);
                if (iown[r]) {
                    const double d = v - y[r];
                    nx[1] += d * d;
                }
                yt[r] = v;
            }
            BSYNC();
#pragma unroll
            for (int q = 0; q < KC; ++q) {
                double a = 0.0;
#pragma unroll
                for (int z = 0; z < ZC; ++z) a = fma(ac[q][z], lds_ld(rca[q][z]), a);
                if (clong[q]) a = group_sum(a, WAVE);
                atyt[q] = a;
            }
            it += R;
            block_sum<WPS, 2>(nx, red, parity, wv, lane);
            double om = gr[GR_OMEGA];
            const double r2 = om * nx[0] + fdiv(nx[1], om);
            bool conv = false;
            int infeas = 0;
            const bool kkt = (chunk % kkt_every) == kkt_every - 1;
            ++chunk;
            if (kkt) {
                // KKT test on T(z) in the original space; A T(x) through the x~ slots
                BSYNC();                              // all lanes done gathering T(y)
#pragma unroll
                for (int q = 0; q < KC; ++q) lds_st(jadr[q], xt[q]);
                if (t == 0) xe_s[n] = 0.0;
                BSYNC();
                double kv[4] = {0.0, 0.0, 0.0, 0.0};  // pres2, dres2, pobj, dobj
#pragma unroll
                for (int r = 0; r < KR; ++r) {
                    double ax = 0.0;
#pragma unroll
                    for (int z = 0; z < ZR; ++z) ax = fma(ar[r][z], lds_ld(cra[r][z]), ax);
                    if (rlong[r]) ax = group_sum(ax, WAVE);
                    if (iown[r]) {
                        const double idr = fdiv(1.0, DR(r));
                        const double axo = ax * idr;
                        const double rl = rlh[r] * idr, ru = ruh[r] * idr;
                        const double v = axo - clampd(axo, rl, ru);
                        kv[0] += v * v;
                        kv[3] += row_dual_term(yt[r] * DR(r), rl, ru);
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
                        kv[1] += (rcst - lam) * (rcst - lam);
                        kv[2] += ce * xo + 0.5 * qe * xo * xo;
                        kv[3] += col_dual_term(ce - at, qe, lbj, ubj);
                    }
                }
                block_sum<WPS, 4>(kv, red, parity, wv, lane);
                const double cterm = gr[GR_CTERM];
                const double pp = kv[2] + cterm, dd = kv[3] + cterm;
                const double tp = P.eps_abs + P.eps_rel * (1.0 + gr[GR_BNORM]);
                const double td = P.eps_abs + P.eps_rel * (1.0 + gr[GR_CNORM]);
                conv = kv[0] <= tp * tp && kv[1] <= td * td &&
                       fabs(pp - dd) <= P.eps_abs + P.eps_rel * (1.0 + fabs(pp) + fabs(dd));
                pobj = pp;
                dobj = dd;
                if (!conv && P.infeas_start >= 0 && it >= P.infeas_start) {
                    // certificates from d = T(z) - z (phgpu.hip, ray_*_terms)
                    BSYNC();
#pragma unroll
                    for (int q = 0; q < KC; ++q) lds_st(jadr[q], xt[q] - x[q]);
                    if (t == 0) xe_s[n] = 0.0;
                    BSYNC();
                    double iv[4] = {0.0, 0.0, 0.0, 0.0};  // ray obj, ray viol2, c'dx, dx viol2
#pragma unroll
                    for (int r = 0; r < KR; ++r) {
                        double adx = 0.0;
#pragma unroll
                        for (int z = 0; z < ZR; ++z) adx = fma(ar[r][z], lds_ld(cra[r][z]), adx);
                        if (rlong[r]) adx = group_sum(adx, WAVE);
                        if (iown[r]) {
                            const double idr = fdiv(1.0, DR(r));
                            const double rl = rlh[r] * idr, ru = ruh[r] * idr;
                            ray_row_terms(DR(r) * (yt[r] - y[r]), rl, ru, iv[0], iv[1]);
                            iv[3] += recession_viol2(adx * idr, rl, ru);
                        }
                    }
#pragma unroll
                    for (int q = 0; q < KC; ++q) {
                        if (jown[q]) {
                            const double d = DC(q);
                            const double id = fdiv(1.0, d);
                            const double lbj = lbh[q] * d, ubj = ubh[q] * d;
                            ray_col_terms(-(atyt[q] - aty[q]) * id, lbj, ubj, iv[0], iv[1]);
                            const double dxo = d * (xt[q] - x[q]);
                            const double qe = QH(q) * id * id;
                            iv[2] += ch[q] * id * dxo;
                            iv[3] += recession_viol2(dxo, lbj, ubj) + (qe * dxo) * (qe * dxo);
                        }
                    }
                    block_sum<WPS, 4>(iv, red, parity, wv, lane);
                    if (is_certificate(iv[0], iv[1], P.eps_inf)) infeas = PHGPU_PRIMAL_INFEASIBLE;
                    else if (is_certificate(-iv[2], iv[3], P.eps_inf)) infeas = PHGPU_DUAL_INFEASIBLE;
                }
            }
            if (conv || infeas != 0 || it >= P.max_iter) {
                stat = conv ? PHGPU_OPTIMAL : (infeas ? infeas : PHGPU_ITER_LIMIT);
                break;
            }
            // -------------------------------------------------- restart test / Halpern step
            double r02 = gr[GR_R0];
            if (r02 < 0.0) r02 = r2;
            const double rlast2 = gr[GR_RLAST];
            const bool restart = (r2 <= bs2 * r02) || (r2 <= bn2 * r02 && r2 > rlast2) ||
                                 (hk + 1 >= P.bart * it);
            BSYNC();                                  // every lane has read the record
            if (t == 0) gr[GR_RLAST] = r2;
            if (restart) {
                double dd2[2] = {0.0, 0.0};
#pragma unroll
                for (int q = 0; q < KC; ++q) {
                    const double d = xt[q] - x0[q];
                    if (jown[q]) dd2[0] += d * d;
                    x[q] = x0[q] = xt[q];
                    aty[q] = aty0[q] = atyt[q];
                }
#pragma unroll
                for (int r = 0; r < KR; ++r) {
                    const double d = yt[r] - y0[r];
                    if (iown[r]) dd2[1] += d * d;
                    y[r] = y0[r] = yt[r];
                }
                block_sum<WPS, 2>(dd2, red, parity, wv, lane);
                if (dd2[0] > 1e-20 && dd2[1] > 1e-20) {
                    const double ratio = __builtin_amdgcn_sqrt(fdiv(dd2[1], dd2[0]));
                    om = clampd(__builtin_amdgcn_sqrt(om * ratio), P.wmin, P.wmax);
                }
                BSYNC();
                if (t == 0) {
                    gr[GR_OMEGA] = om;
                    gr[GR_R0] = -1.0;
                    gr[GR_RLAST] = INFINITY;
                }
                set_steps(om);   // reads only GR_ETA (never written inside the solve)
                hk = 0;
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
            BSYNC();                                  // record updates visible to all lanes
        }

        // ------------------------------------------------------------ write back
        if (stat != PHGPU_OPTIMAL) {
            // iteration cap / certificate: the answer is T(z) of the last check (box-feasible)
            double pv[2] = {0.0, 0.0};
#pragma unroll
            for (int r = 0; r < KR; ++r)
                if (iown[r]) pv[1] += row_dual_term(yt[r] * DR(r), rlh[r] / DR(r), ruh[r] / DR(r));
#pragma unroll
            for (int q = 0; q < KC; ++q) {
                if (jown[q]) {
                    const double d = DC(q);
                    const double xo = d * xt[q];
                    const double ce = ch[q] / d, qe = QH(q) / (d * d);
                    pv[0] += ce * xo + 0.5 * qe * xo * xo;
                    pv[1] += col_dual_term(ce - atyt[q] / d, qe, lbh[q] * d, ubh[q] * d);
                }
            }
            block_sum<WPS, 2>(pv, red, parity, wv, lane);
            pobj = pv[0] + gr[GR_CTERM];
            dobj = pv[1] + gr[GR_CTERM];
            if (stat == PHGPU_PRIMAL_INFEASIBLE) pobj = dobj = INFINITY;
            if (stat == PHGPU_DUAL_INFEASIBLE) pobj = dobj = -INFINITY;
        }
#pragma unroll
        for (int q = 0; q < KC; ++q) {
            if (jown[q]) {
                rec[st.pk_XW + jcol[q]] = xt[q];  // x = Dc x^ goes out by k_from_records
            }
        }
#pragma unroll
        for (int r = 0; r < KR; ++r) {
            if (iown[r]) {
                rec[st.pk_YW + irow[r]] = yt[r];
            }
        }
        if (t == 0) {
            st.omega_w[s] = gr[GR_OMEGA];
            obj[s] = pobj;
            bound[s] = dobj;
            status[s] = stat;
            if (iters) iters[s] = it;
            bcast[0] = (double)(gridDim.x + atomicAdd(qhead, 1));   // next scenario
        }
        BSYNC();
        // wave-uniform (SGPR) scenario id: the record pointer then needs no VGPRs
        s = __builtin_amdgcn_readfirstlane((int)bcast[0]);
        BSYNC();                                      // bcast / record reads done before reuse
    }
#undef QH
#undef DC
#undef DR
}

// ------------------------------------------------------------------ instances
typedef void (*wg_kernel_t)(pdhg_view, solve_params, wg_plan, int*, double*, double*, double*, double*,
                            int32_t*, int32_t*);

struct wg_instance {
    int KC, ZC, KR, ZR, WPS;
    wg_kernel_t fn;
};

#define WG_INST(a, b, c, d, w) {a, b, c, d, w, k_solve_wg<a, b, c, d, w>}
static const wg_instance g_wg_instances[] = {
    // farmer: column degree <= 3, short rows <= 4 entries, one long (acreage) row
    WG_INST(2, 3, 2, 4, 1),   // cm = 10 (config 2): n = 120, m = 61, one wave per scenario
    WG_INST(3, 3, 2, 4, 1),
    WG_INST(2, 3, 2, 4, 2), WG_INST(3, 3, 2, 4, 2),
    WG_INST(2, 3, 2, 4, 4), WG_INST(3, 3, 2, 4, 4),   // cm = 64: n = 768, m = 385, L = 256
    WG_INST(2, 3, 2, 4, 8), WG_INST(3, 3, 2, 4, 8),
    // wider patterns (column degree <= 4, rows <= 8)
    WG_INST(2, 4, 2, 8, 4), WG_INST(2, 4, 2, 8, 8),
};
#undef WG_INST
