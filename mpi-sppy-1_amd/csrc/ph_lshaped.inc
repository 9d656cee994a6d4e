// The L-shaped method (mpisppy/opt/lshaped.py): Benders cuts of all local scenarios and the master
// LP, on the device (phgpu_lshaped_*, include/phgpu.h; DESIGN.md 3.19).  Included by phgpu.hip
// after ph_aph.inc.
//
// Master:  min sum_g eta_g  over z = (x in R^nn, eta in R^G)
//          xlb <= x <= xub,  rl <= R x <= ru (rl == ru: an equality),  eta >= etalb,
//          eta_{g(c)} - a_c . x >= b_c  for every cut c of the store.
// Every inequality is a row h_i . z >= beta_i with a slack s_i and a multiplier lam_i; their
// index space is fixed (LS_I_* below), rows that do not exist (an infinite side, an equality's
// two sides, a cut slot not filled) are inactive.
//
// The master's arithmetic (ls_master_core and what it calls) is written once for a workgroup of
// LS_T threads and for one host thread (LS_HOST: thread 0 of 1, barriers empty), so the same
// text can be compiled into a host program and checked there.
#define LS_NN_MAX 64
#define LS_G_MAX 32
#define LS_ROWS_MAX 64
#define LS_T 256        // threads of the master's workgroup
#define LS_ITER_CAP 200 // interior-point iterations at most, whatever the options say
#define LS_TILE 16      // dense rows staged in LDS per trip of the normal-matrix build

struct ls_store {
    int G, nn, N, ld, max_cuts, n_rows, ne, NI;
    int64_t s_off, S_total;  // global index of local scenario 0, scenarios of all ranks
    // the cuts: a [nn][max_cuts] (cut-fastest: a lane per cut reads coalesced), b, group, count
    double *cut_a, *cut_b;
    int32_t *cut_g, *ncuts;
    // first-stage rows (dense [n_rows][nn]) and which of them are equalities
    double *R, *rl, *ru;
    int32_t* eq;
    double *xlb, *xub, *etalb;
    // the master's warm state (its last solution) and work vectors [NI] / [N][ne]
    double* zw;
    int32_t* has_w;
    double *s, *lam, *rp, *ds, *dl, *t, *w;
    double* V;
    // per-scenario terms of the cut pass [(nn + 3)][S]
    double* terms;
};

// index space of the inequalities
#define LS_I_XL(L) 0
#define LS_I_XU(L) ((L).nn)
#define LS_I_EL(L) (2 * (L).nn)
#define LS_I_RL(L) (2 * (L).nn + (L).G)
#define LS_I_RU(L) (2 * (L).nn + (L).G + (L).n_rows)
#define LS_I_CUT(L) (2 * (L).nn + (L).G + 2 * (L).n_rows)

#ifdef LS_HOST
#define LS_FN static inline
#define LS_TID 0
#define LS_NT 1
#define LS_LANE 0
#define LS_NLANE 1
#define LS_WV 0
#define LS_NWV 1
#define LS_SYNC() ((void)0)
#else
#define LS_FN __device__ __forceinline__
#define LS_TID ((int)threadIdx.x)
#define LS_NT ((int)blockDim.x)
#define LS_LANE ((int)(threadIdx.x & (WAVE - 1)))
#define LS_NLANE WAVE
#define LS_WV ((int)(threadIdx.x / WAVE))
#define LS_NWV ((int)(blockDim.x / WAVE))
#define LS_SYNC() __syncthreads()
#endif

// op: 0 sum, 1 max, 2 min
LS_FN double ls_op(int op, double a, double b) { return op == 0 ? a + b : (op == 1 ? fmax(a, b) : fmin(a, b)); }

// the lanes' values combined over the wave, the same bits in every lane (a butterfly: each
// step adds the same two numbers in both partners)
LS_FN double ls_wave_all(int op, double v) {
#ifndef LS_HOST
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) v = ls_op(op, v, __shfl_xor(v, o, WAVE));
#endif
    return v;
}

// N values combined over the workgroup in a fixed order; the results in every thread.
// red: shared, N * (LS_T / WAVE) doubles.
template <int N>
LS_FN void ls_block_all(const int (&op)[N], double (&v)[N], double* red) {
#ifndef LS_HOST
#pragma unroll
    for (int j = 0; j < N; ++j) {
        v[j] = ls_wave_all(op[j], v[j]);
        if (LS_LANE == 0) red[j * (LS_T / WAVE) + LS_WV] = v[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < N; ++j) {
        double a = red[j * (LS_T / WAVE)];
        for (int u = 1; u < LS_NWV; ++u) a = ls_op(op[j], a, red[j * (LS_T / WAVE) + u]);
        v[j] = a;
    }
    __syncthreads();
#else
    (void)op; (void)v; (void)red;
#endif
}

// row i of the inequalities: false if it does not exist, else beta and h_i . z (z: N doubles)
LS_FN bool ls_row(const ls_store& L, int nc, int i, const double* z, double& beta, double& hz) {
    const int nn = L.nn;
    if (i < LS_I_XU(L)) {
        beta = L.xlb[i];
        hz = z[i];
        return isfinite(beta);
    }
    if (i < LS_I_EL(L)) {
        const int k = i - LS_I_XU(L);
        beta = -L.xub[k];
        hz = -z[k];
        return isfinite(beta);
    }
    if (i < LS_I_RL(L)) {
        const int g = i - LS_I_EL(L);
        beta = L.etalb[g];
        hz = z[nn + g];
        return true;
    }
    if (i < LS_I_CUT(L)) {
        const bool up = i >= LS_I_RU(L);
        const int r = i - (up ? LS_I_RU(L) : LS_I_RL(L));
        const double lo = L.rl[r], hi = L.ru[r];
        if (lo == hi) return false;
        double a = 0.0;
        for (int k = 0; k < nn; ++k) a += L.R[(size_t)r * nn + k] * z[k];
        beta = up ? -hi : lo;
        hz = up ? -a : a;
        return isfinite(beta);
    }
    const int c = i - LS_I_CUT(L);
    if (c >= nc) return false;
    double a = 0.0;
    for (int k = 0; k < nn; ++k) a += L.cut_a[(size_t)k * L.max_cuts + c] * z[k];
    beta = L.cut_b[c];
    hz = z[nn + L.cut_g[c]] - a;
    return true;
}

// out = H^T t (t zero on inactive rows): a wave per component, its lanes over the rows
LS_FN void ls_HTv(const ls_store& L, int nc, const double* t, double* out) {
    const int nn = L.nn;
    for (int j = LS_WV; j < L.N; j += LS_NWV) {
        double a = 0.0;
        if (j < nn) {
            for (int r = LS_LANE; r < L.n_rows; r += LS_NLANE)
                a += L.R[(size_t)r * nn + j] * (t[LS_I_RL(L) + r] - t[LS_I_RU(L) + r]);
            for (int c = LS_LANE; c < nc; c += LS_NLANE) a -= L.cut_a[(size_t)j * L.max_cuts + c] * t[LS_I_CUT(L) + c];
        } else {
            const int g = j - nn;
            for (int c = LS_LANE; c < nc; c += LS_NLANE)
                if (L.cut_g[c] == g) a += t[LS_I_CUT(L) + c];
        }
        a = ls_wave_all(0, a);
        if (LS_LANE == 0) {
            if (j < nn) a += t[LS_I_XL(L) + j] - t[LS_I_XU(L) + j];
            else a += t[LS_I_EL(L) + (j - nn)];
            out[j] = a;
        }
    }
    LS_SYNC();
}

// Cholesky factor of the n x n matrix M (lower triangle, leading dimension ld) in place.  A
// pivot at or below floor_ drops its direction (the factor gets a huge diagonal there).
LS_FN void ls_chol(double* M, int n, int ld, double floor_) {
    for (int j = 0; j < n; ++j) {
        LS_SYNC();
        if (LS_TID == 0) {
            const double d = M[j * ld + j];
            M[j * ld + j] = d > floor_ ? sqrt(d) : 1e64;
        }
        LS_SYNC();
        const double dj = M[j * ld + j];
        for (int i = j + 1 + LS_TID; i < n; i += LS_NT) M[i * ld + j] /= dj;
        LS_SYNC();
        const int m = n - j - 1;
        for (int e = LS_TID; e < m * m; e += LS_NT) {
            const int r = j + 1 + e / m, c = j + 1 + e % m;
            if (c <= r) M[r * ld + c] -= M[r * ld + j] * M[c * ld + j];
        }
    }
    LS_SYNC();
}

// v = L^-1 v, and with both: v = L^-T L^-1 v
LS_FN void ls_fwd(const double* M, int n, int ld, double* v) {
    for (int j = 0; j < n; ++j) {
        LS_SYNC();
        if (LS_TID == 0) v[j] /= M[j * ld + j];
        LS_SYNC();
        const double vj = v[j];
        for (int i = j + 1 + LS_TID; i < n; i += LS_NT) v[i] -= M[i * ld + j] * vj;
    }
    LS_SYNC();
}
LS_FN void ls_bwd(const double* M, int n, int ld, double* v) {
    for (int j = n - 1; j >= 0; --j) {
        LS_SYNC();
        if (LS_TID == 0) v[j] /= M[j * ld + j];
        LS_SYNC();
        const double vj = v[j];
        for (int i = LS_TID; i < j; i += LS_NT) v[i] -= M[j * ld + i] * vj;
    }
    LS_SYNC();
}

// the master's shared memory, carved from one block of doubles
struct ls_shared {
    double *M, *Sc, *tile, *tw;
    double *z, *dz, *rhs, *g;      // [N]
    double *nu, *dnu, *re, *q;     // [ne]
    double* red;                   // reductions
    double* sc;                    // scalars
};
static inline size_t ls_shared_doubles(int N, int ld, int ne) {  // (host)
    return (size_t)N * ld + (size_t)ne * (ne | 1) + (size_t)LS_TILE * N + LS_TILE + 4 * (size_t)N + 4 * (size_t)ne +
           8 * (LS_T / 64) + 16;
}
LS_FN void ls_carve(double* base, int N, int ld, int ne, ls_shared& sh) {
    double* p = base;
    sh.M = p; p += (size_t)N * ld;
    sh.Sc = p; p += (size_t)ne * (ne | 1);
    sh.tile = p; p += (size_t)LS_TILE * N;
    sh.tw = p; p += LS_TILE;
    sh.z = p; p += N;
    sh.dz = p; p += N;
    sh.rhs = p; p += N;
    sh.g = p; p += N;
    sh.nu = p; p += ne;
    sh.dnu = p; p += ne;
    sh.re = p; p += ne;
    sh.q = p; p += ne;
    sh.red = p; p += 8 * (LS_T / 64);
    sh.sc = p;
}

// dz, dnu of  (H^T W H + reg) dz - E^T dnu = rhs,  E dz = -re  from the factors: M = L L^T,
// V = L^-1 E^T, Sc = chol(V^T V).  rhs in sh.rhs (destroyed); dz to sh.dz, dnu to sh.dnu.
LS_FN void ls_kkt_solve(const ls_store& L, ls_shared& sh) {
    const int N = L.N, ld = L.ld, ne = L.ne, lds = ne | 1;
    ls_fwd(sh.M, N, ld, sh.rhs);  // u = L^-1 rhs
    if (ne > 0) {
        for (int e = LS_TID; e < ne; e += LS_NT) {
            double a = -sh.re[e];
            for (int j = 0; j < N; ++j) a -= L.V[(size_t)j * ne + e] * sh.rhs[j];
            sh.dnu[e] = a;
        }
        LS_SYNC();
        ls_fwd(sh.Sc, ne, lds, sh.dnu);
        ls_bwd(sh.Sc, ne, lds, sh.dnu);
        for (int j = LS_TID; j < N; j += LS_NT) {
            double a = sh.rhs[j];
            for (int e = 0; e < ne; ++e) a += L.V[(size_t)j * ne + e] * sh.dnu[e];
            sh.rhs[j] = a;
        }
        LS_SYNC();
    }
    ls_bwd(sh.M, N, ld, sh.rhs);
    for (int j = LS_TID; j < N; j += LS_NT) sh.dz[j] = sh.rhs[j];
    LS_SYNC();
}

// rhs = -c + E^T nu + H^T t   (c: 1 on the eta components)
LS_FN void ls_make_rhs(const ls_store& L, int nc, ls_shared& sh) {
    ls_HTv(L, nc, L.t, sh.rhs);
    for (int j = LS_TID; j < L.N; j += LS_NT) {
        double a = sh.rhs[j] - (j >= L.nn ? 1.0 : 0.0);
        if (j < L.nn)
            for (int e = 0; e < L.ne; ++e) a += L.R[(size_t)L.eq[e] * L.nn + j] * sh.nu[e];
        sh.rhs[j] = a;
    }
    LS_SYNC();
}

// The master LP by Mehrotra's predictor-corrector on the normal equations in z.
//   x0: the start of x, stride x0s (null: zero);  eps, eps_inf, max_it: tolerances and cap;
//   out: {objective, status, iterations, primal, dual, gap residual}; the solution in sh.z.
LS_FN void ls_master_core(const ls_store& L, ls_shared& sh, const double* x0, size_t x0s, double eps, double eps_inf,
                          int max_it, double* out) {
    const int N = L.N, nn = L.nn, G = L.G, ld = L.ld, ne = L.ne, NI = L.NI;
    const int nc = L.ncuts[0] < L.max_cuts ? L.ncuts[0] : L.max_cuts;
    const int op_sss[3] = {0, 0, 0}, op_m4[4] = {1, 1, 1, 1}, op_mm[2] = {2, 2}, op_s4[4] = {0, 0, 0, 0},
              op_sm[2] = {0, 2};
    // ---- the start: x0 pushed inside its bounds, eta above its cuts
    for (int k = LS_TID; k < nn; k += LS_NT) {
        double v = x0 ? x0[(size_t)k * x0s] : 0.0;
        const double lo = L.xlb[k], hi = L.xub[k];
        if (!isfinite(v)) v = 0.0;
        if (isfinite(lo) && isfinite(hi)) {
            const double m = 0.01 * (hi - lo);
            v = fmin(fmax(v, lo + m), hi - m);
        } else if (isfinite(lo)) v = fmax(v, lo + 1.0);
        else if (isfinite(hi)) v = fmin(v, hi - 1.0);
        sh.z[k] = v;
    }
    for (int g = LS_TID; g < G; g += LS_NT) sh.z[nn + g] = 0.0;
    for (int e = LS_TID; e < ne; e += LS_NT) sh.nu[e] = 0.0;
    LS_SYNC();
    for (int c = LS_TID; c < nc; c += LS_NT) {
        double beta, hz;
        ls_row(L, nc, LS_I_CUT(L) + c, sh.z, beta, hz);
        L.t[LS_I_CUT(L) + c] = beta - hz;  // what eta needs to be at least (eta is 0 in z)
    }
    LS_SYNC();
    for (int g = LS_TID; g < G; g += LS_NT) {
        double v = L.etalb[g];
        for (int c = 0; c < nc; ++c)
            if (L.cut_g[c] == g) v = fmax(v, L.t[LS_I_CUT(L) + c]);
        sh.z[nn + g] = v + 1.0 + 0.01 * fabs(v);
    }
    LS_SYNC();
    // slacks at least 1e-2 max(1, |beta|), multipliers centred: s_i lam_i = the slacks' mean
    double bmax = 0.0;
    {
        double ssum = 0.0, na = 0.0;
        for (int i = LS_TID; i < NI; i += LS_NT) {
            double beta = 0.0, hz = 0.0;
            const bool act = ls_row(L, nc, i, sh.z, beta, hz);
            const double fl = 1e-2 * fmax(1.0, fabs(beta));
            L.s[i] = act ? fmax(hz - beta, fl) : 1.0;
            L.lam[i] = act ? 1.0 : 0.0;
            if (act) {
                bmax = fmax(bmax, fabs(beta));
                ssum += L.s[i];
                na += 1.0;
            }
        }
        for (int e = LS_TID; e < ne; e += LS_NT) bmax = fmax(bmax, fabs(L.rl[L.eq[e]]));
        double v[4] = {bmax, 0.0, 0.0, 0.0};
        ls_block_all(op_m4, v, sh.red);
        bmax = v[0];
        double u[3] = {ssum, na, 0.0};
        ls_block_all(op_sss, u, sh.red);
        const double mu0 = u[0] / fmax(u[1], 1.0);
        for (int i = LS_TID; i < NI; i += LS_NT)
            if (L.lam[i] > 0.0) L.lam[i] = mu0 / L.s[i];
    }
    int status = PHGPU_ITER_LIMIT, it = 0;
    double pres = INFINITY, dres = INFINITY, gap = INFINITY, objv = 0.0, pres0 = 0.0;
    if (max_it > LS_ITER_CAP) max_it = LS_ITER_CAP;
    for (;; ++it) {
        // ---- residuals
        double mu_sum = 0.0, nact = 0.0, fobj = 0.0, rpm = 0.0, pmin = INFINITY;
        for (int i = LS_TID; i < NI; i += LS_NT) {
            double beta = 0.0, hz = 0.0;
            const bool act = ls_row(L, nc, i, sh.z, beta, hz);
            const double s = L.s[i], lam = L.lam[i];
            const double rp = act ? hz - s - beta : 0.0;
            L.rp[i] = rp;
            L.w[i] = act ? lam / s : 0.0;
            L.t[i] = act ? lam : 0.0;
            if (act) {
                mu_sum += s * lam;
                pmin = fmin(pmin, s * lam);
                nact += 1.0;
                fobj += beta * lam;
                rpm = fmax(rpm, fabs(rp));
            }
        }
        double rem = 0.0;
        for (int e = LS_TID; e < ne; e += LS_NT) {
            const int r = L.eq[e];
            double a = 0.0;
            for (int k = 0; k < nn; ++k) a += L.R[(size_t)r * nn + k] * sh.z[k];
            sh.re[e] = a - L.rl[r];
            rem = fmax(rem, fabs(sh.re[e]));
            fobj += L.rl[r] * sh.nu[e];
        }
        {
            double v[3] = {mu_sum, nact, fobj};
            ls_block_all(op_sss, v, sh.red);
            mu_sum = v[0]; nact = v[1]; fobj = v[2];
            double u[2] = {0.0, pmin};
            ls_block_all(op_sm, u, sh.red);
            pmin = u[1];
        }
        LS_SYNC();
        ls_HTv(L, nc, L.t, sh.g);  // H^T lam
        double rdm = 0.0, fvm = 0.0, zm = 0.0;
        objv = 0.0;
        for (int j = LS_TID; j < N; j += LS_NT) {
            double a = sh.g[j];
            if (j < nn)
                for (int e = 0; e < ne; ++e) a += L.R[(size_t)L.eq[e] * nn + j] * sh.nu[e];
            fvm = fmax(fvm, fabs(a));
            rdm = fmax(rdm, fabs((j >= nn ? 1.0 : 0.0) - a));
            zm = fmax(zm, fabs(sh.z[j]));
        }
        {
            double v[4] = {rpm, rem, rdm, fvm};
            ls_block_all(op_m4, v, sh.red);
            rpm = v[0]; rem = v[1]; rdm = v[2]; fvm = v[3];
            double u[4] = {zm, 0.0, 0.0, 0.0};
            ls_block_all(op_m4, u, sh.red);
            zm = u[0];
        }
        for (int g = 0; g < G; ++g) objv += sh.z[nn + g];
        const double mu = mu_sum / fmax(nact, 1.0);
        pres = fmax(rpm, rem) / (1.0 + bmax);
        dres = rdm / 2.0;
        gap = mu_sum / (1.0 + fabs(objv));
        if (pres <= eps && dres <= eps && gap <= eps) {
            status = PHGPU_OPTIMAL;
            break;
        }
        // a Farkas ray: (lam, nu) with H^T lam + E^T nu ~ 0 and beta . lam + e . nu > 0
        // (and a primal residual that has not come down: that of a feasible master falls with
        // every step, so a large dual objective alone is not taken for a ray)
        if (it == 0) pres0 = pres;
        if (it >= 5 && fobj > 0.0 && fvm * (1.0 + zm) <= eps_inf * fobj && pres > eps && pres >= 1e-2 * pres0) {
            status = PHGPU_PRIMAL_INFEASIBLE;
            break;
        }
        if (it >= max_it || !(mu_sum == mu_sum)) break;
        // ---- M = H^T W H + reg (lower triangle)
        for (int e = LS_TID; e < N * N; e += LS_NT) {
            const int i = e / N, j = e % N;
            if (j <= i) {
                double v = 0.0;
                if (i == j) v = i < nn ? L.w[LS_I_XL(L) + i] + L.w[LS_I_XU(L) + i] : L.w[LS_I_EL(L) + (i - nn)];
                sh.M[i * ld + j] = v;
            }
        }
        const int nd = L.n_rows + nc;
        for (int d0 = 0; d0 < nd; d0 += LS_TILE) {
            LS_SYNC();
            for (int e = LS_TID; e < LS_TILE * N; e += LS_NT) {
                const int u = e / N, j = e % N, d = d0 + u;
                double v = 0.0;
                if (d < L.n_rows) {
                    if (j < nn) v = L.R[(size_t)d * nn + j];
                } else if (d < nd) {
                    const int c = d - L.n_rows;
                    v = j < nn ? -L.cut_a[(size_t)j * L.max_cuts + c] : (L.cut_g[c] == j - nn ? 1.0 : 0.0);
                }
                sh.tile[u * N + j] = v;
            }
            for (int u = LS_TID; u < LS_TILE; u += LS_NT) {
                const int d = d0 + u;
                sh.tw[u] = d < L.n_rows ? L.w[LS_I_RL(L) + d] + L.w[LS_I_RU(L) + d]
                                        : (d < nd ? L.w[LS_I_CUT(L) + d - L.n_rows] : 0.0);
            }
            LS_SYNC();
            for (int e = LS_TID; e < N * N; e += LS_NT) {
                const int i = e / N, j = e % N;
                if (j <= i) {
                    double a = 0.0;
                    for (int u = 0; u < LS_TILE; ++u) a += sh.tw[u] * sh.tile[u * N + i] * sh.tile[u * N + j];
                    sh.M[i * ld + j] += a;
                }
            }
        }
        LS_SYNC();
        // the regularisation, relative to each column's own diagonal so that it does not damp
        // the directions along the optimal face (whose curvature is many orders below the
        // largest): 1e-13 of it, 1e-10 of it on an x column without a finite bound, plus
        // 1e-24 of the largest diagonal where a column has no row at all
        double dmax = 0.0;
        for (int j = LS_TID; j < N; j += LS_NT) dmax = fmax(dmax, sh.M[j * ld + j]);
        {
            double v[4] = {dmax, 0.0, 0.0, 0.0};
            ls_block_all(op_m4, v, sh.red);
            dmax = fmax(v[0], 1e-300);
        }
        for (int j = LS_TID; j < N; j += LS_NT) {
            const bool fr = j < nn && !isfinite(L.xlb[j]) && !isfinite(L.xub[j]);
            sh.M[j * ld + j] += (fr ? 1e-10 : 1e-13) * sh.M[j * ld + j] + 1e-24 * dmax;
        }
        ls_chol(sh.M, N, ld, 1e-40 * dmax);
        if (ne > 0) {
            const int lds = ne | 1;
            // V = L^-1 E^T, all columns together
            for (int e = LS_TID; e < N * ne; e += LS_NT) {
                const int j = e / ne, q = e % ne;
                L.V[e] = j < nn ? L.R[(size_t)L.eq[q] * nn + j] : 0.0;
            }
            for (int j = 0; j < N; ++j) {
                LS_SYNC();
                const double dj = sh.M[j * ld + j];
                for (int q = LS_TID; q < ne; q += LS_NT) L.V[(size_t)j * ne + q] /= dj;
                LS_SYNC();
                const int m = N - j - 1;
                for (int e = LS_TID; e < m * ne; e += LS_NT) {
                    const int i = j + 1 + e / ne, q = e % ne;
                    L.V[(size_t)i * ne + q] -= sh.M[i * ld + j] * L.V[(size_t)j * ne + q];
                }
            }
            LS_SYNC();
            double smax = 0.0;
            for (int e = LS_TID; e < ne * ne; e += LS_NT) {
                const int p = e / ne, q = e % ne;
                if (q <= p) {
                    double a = 0.0;
                    for (int j = 0; j < N; ++j) a += L.V[(size_t)j * ne + p] * L.V[(size_t)j * ne + q];
                    if (p == q) smax = fmax(smax, a);
                    sh.Sc[p * lds + q] = a;
                }
            }
            {
                double v[4] = {smax, 0.0, 0.0, 0.0};
                ls_block_all(op_m4, v, sh.red);
                smax = fmax(v[0], 1e-300);
            }
            for (int p = LS_TID; p < ne; p += LS_NT) sh.Sc[p * lds + p] += 1e-14 * smax;
            ls_chol(sh.Sc, ne, lds, 1e-30 * smax);
        }
        // ---- predictor: t = -lam rp / s
        for (int i = LS_TID; i < NI; i += LS_NT) L.t[i] = -L.w[i] * L.rp[i];
        LS_SYNC();
        ls_make_rhs(L, nc, sh);
        ls_kkt_solve(L, sh);
        double ap = 1.0, ad = 1.0;
        for (int i = LS_TID; i < NI; i += LS_NT) {
            double beta = 0.0, hd = 0.0;
            const bool act = ls_row(L, nc, i, sh.dz, beta, hd);
            if (!act) continue;
            const double s = L.s[i], lam = L.lam[i];
            const double ds = hd + L.rp[i], dl = -lam - L.w[i] * ds;
            L.ds[i] = ds;
            L.dl[i] = dl;
            if (ds < 0.0) ap = fmin(ap, -s / ds);
            if (dl < 0.0) ad = fmin(ad, -lam / dl);
        }
        {
            double v[2] = {ap, ad};
            ls_block_all(op_mm, v, sh.red);
            ap = v[0]; ad = v[1];
        }
        double mua = 0.0;
        for (int i = LS_TID; i < NI; i += LS_NT)
            if (L.w[i] > 0.0 || L.lam[i] > 0.0) mua += (L.s[i] + ap * L.ds[i]) * (L.lam[i] + ad * L.dl[i]);
        {
            double v[4] = {mua, 0.0, 0.0, 0.0};
            ls_block_all(op_s4, v, sh.red);
            mua = v[0] / fmax(nact, 1.0);
        }
        const double rat = mu > 0.0 ? fmin(1.0, fmax(0.0, mua / mu)) : 0.0;
        // the gap is already there and a residual is not: centre only (sigma = 1, no second-order
        // term), so that full steps take the residuals down at this mu
        // -- or the gap runs a factor ten ahead of the residuals: with lam / s of the active rows
        // at 1e10 the normal matrix no longer resolves a dual residual below about 1e-5
        const bool centre = gap <= 0.1 * eps || gap < 0.1 * fmax(pres, dres);
        const double sigma = centre ? 1.0 : rat * rat * rat;
        if (centre)
            for (int i = LS_TID; i < NI; i += LS_NT) L.ds[i] = 0.0;
        // ---- corrector: t = (sigma mu - ds_a dl_a - lam rp) / s
        for (int i = LS_TID; i < NI; i += LS_NT) {
            const bool act = L.lam[i] > 0.0;
            L.t[i] = act ? (sigma * mu - L.ds[i] * L.dl[i]) / L.s[i] - L.w[i] * L.rp[i] : 0.0;
        }
        LS_SYNC();
        ls_make_rhs(L, nc, sh);
        ls_kkt_solve(L, sh);
        ap = 1e30;
        ad = 1e30;
        for (int i = LS_TID; i < NI; i += LS_NT) {
            double beta = 0.0, hd = 0.0;
            const bool act = ls_row(L, nc, i, sh.dz, beta, hd);
            if (!act) continue;
            const double s = L.s[i], lam = L.lam[i];
            const double ds = hd + L.rp[i];
            // dl = (rc - lam ds) / s with rc = sigma mu - s lam - ds_a dl_a
            const double dl = (sigma * mu - L.ds[i] * L.dl[i]) / s - lam - L.w[i] * ds;
            L.ds[i] = ds;
            L.dl[i] = dl;
            if (ds < 0.0) ap = fmin(ap, -s / ds);
            if (dl < 0.0) ad = fmin(ad, -lam / dl);
        }
        {
            double v[2] = {ap, ad};
            ls_block_all(op_mm, v, sh.red);
            ap = fmin(1.0, 0.995 * v[0]);
            ad = fmin(1.0, 0.995 * v[1]);
        }
        // stay in the wide neighbourhood of the central path: no product s_i lam_i below 1e-4
        // of their new mean, or the steps are shortened (without it the multipliers of a
        // degenerate master jam at the boundary while the dual residual is still large)
        const double nbh = fmin(1e-4, 0.5 * pmin / fmax(mu, 1e-300));  // (never asks more than half of what holds now)
        for (int tr = 0; tr < 16; ++tr) {
            double v[2] = {0.0, INFINITY};
            for (int i = LS_TID; i < NI; i += LS_NT)
                if (L.lam[i] > 0.0) {
                    const double pr = (L.s[i] + ap * L.ds[i]) * (L.lam[i] + ad * L.dl[i]);
                    v[0] += pr;
                    v[1] = fmin(v[1], pr);
                }
            ls_block_all(op_sm, v, sh.red);
            if (v[1] >= nbh * v[0] / fmax(nact, 1.0)) break;
            ap *= 0.7;
            ad *= 0.7;
        }
        for (int i = LS_TID; i < NI; i += LS_NT)
            if (L.lam[i] > 0.0) {
                L.s[i] += ap * L.ds[i];
                L.lam[i] += ad * L.dl[i];
            }
        LS_SYNC();
        for (int j = LS_TID; j < N; j += LS_NT) sh.z[j] += ap * sh.dz[j];
        for (int e = LS_TID; e < ne; e += LS_NT) sh.nu[e] += ad * sh.dnu[e];
        LS_SYNC();
    }
    if (LS_TID == 0) {
        out[0] = objv;
        out[1] = (double)status;
        out[2] = (double)it;
        out[3] = pres;
        out[4] = dres;
        out[5] = gap;
    }
    LS_SYNC();
}

#ifndef LS_HOST
// ------------------------------------------------------------------ kernels
extern __shared__ double ls_dyn[];

// lshaped.py:600-630 (the root solve): the master as one workgroup.  The solution goes to
// xhat [nn][S] (every scenario the same, what phgpu_fix_nonants reads), eta [G], the store's
// warm state and info (6 doubles, device or host-mapped).
__global__ void __launch_bounds__(LS_T)
k_ls_master(ls_store L, int64_t S, double eps, double eps_inf, int max_it, double* __restrict__ xhat,
            double* __restrict__ eta, double* __restrict__ info) {
    ls_shared sh;
    ls_carve(ls_dyn, L.N, L.ld, L.ne, sh);
    const bool warm = L.has_w[0] != 0;
    ls_master_core(L, sh, warm ? L.zw : xhat, warm ? (size_t)1 : (size_t)S, eps, eps_inf, max_it, sh.sc);
    for (int j = threadIdx.x; j < L.N; j += LS_T) L.zw[j] = sh.z[j];
    for (int g = threadIdx.x; g < L.G; g += LS_T) eta[g] = sh.z[L.nn + g];
    if (threadIdx.x == 0) L.has_w[0] = 1;
    for (int k = 0; k < L.nn; ++k) {
        const double v = sh.z[k];
        for (int64_t s = threadIdx.x; s < S; s += LS_T) xhat[IX(k)] = v;
    }
    if (threadIdx.x < 6) info[threadIdx.x] = sh.sc[threadIdx.x];
}

// lshaped.py:477-520 (the cut of one scenario from its duals), all local scenarios: a lane per
// scenario, its probability-weighted terms to L.terms [(nn + 3)][S]:
//   d_k = c_k + q_k x_k - sum_i A_ik y_i  (the reduced cost of fixed column k),
//   planes 0 .. nn-1: p d_k,  nn: p (obj - d . x),  nn + 1: p obj,  nn + 2: 1 if not OPTIMAL
// (a scenario that is not OPTIMAL contributes that count only).
__global__ void __launch_bounds__(GR_T)
k_ls_terms(ph_data st, ls_store L, const double* __restrict__ x, const double* __restrict__ y,
           const double* __restrict__ obj, const int32_t* __restrict__ status) {
    const int64_t S = st.S;
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const int nn = st.nn;
    const bool ok = status[s] == PHGPU_OPTIMAL;
    const double p = st.prob[s];
    double dx = 0.0;
    for (int k = 0; k < nn; ++k) {
        const int j = st.nonant_col[k];
        const double xv = x[IX(j)];
        double d = st.c[IX(j)] + st.q[IX(j)] * xv;
        for (int kc = st.col_ptr[j]; kc < st.col_ptr[j + 1]; ++kc) d -= st.A[IX(st.perm[kc])] * y[IX(st.row_idx[kc])];
        L.terms[IX(k)] = ok ? p * d : 0.0;
        dx += d * xv;
    }
    const double o = obj[s];
    L.terms[IX(nn)] = ok ? p * (o - dx) : 0.0;
    L.terms[IX(nn + 1)] = ok ? p * o : 0.0;
    L.terms[IX(nn + 2)] = ok ? 0.0 : 1.0;
}

// the group sums: block b = g (nn + 2) + j adds plane j over the local scenarios of group g
// (global index s in [ceil(g S_total / G), ceil((g + 1) S_total / G))), the last block the
// not-OPTIMAL count over all of them.  Every thread adds its terms in index order, the block
// its threads in a fixed order.
__global__ void __launch_bounds__(GR_T)
k_ls_gsum(ls_store L, int64_t S, double* __restrict__ cutbuf) {
    __shared__ double red[GR_T / WAVE];
    const int nn = L.nn, P = nn + 2;
    const int b = blockIdx.x;
    int64_t lo = 0, hi = S;
    int j = nn + 2;
    if (b < L.G * P) {
        const int64_t g = b / P;
        j = b % P;
        lo = (g * L.S_total + L.G - 1) / L.G - L.s_off;
        hi = ((g + 1) * L.S_total + L.G - 1) / L.G - L.s_off;
        lo = lo < 0 ? 0 : (lo > S ? S : lo);
        hi = hi < 0 ? 0 : (hi > S ? S : hi);
    }
    double acc = 0.0;
    for (int64_t s = lo + threadIdx.x; s < hi; s += GR_T) acc += L.terms[IX(j)];
    const double t = block_sum_fixed(acc, red);
    if (threadIdx.x == 0) cutbuf[b] = t;
}

// lshaped.py:540-560 (add the cuts that cut off eta) after the ranks' sum of cutbuf: one wave.
// Group g gets a cut when Q_g - eta_g > tol max(1, |Q_g|); the cuts go to the store in group
// order.  info: {cuts added, sum_g Q_g, cuts held, scenarios not OPTIMAL, cuts wanted}, one store
// (wanted > added: the store was full and cuts were dropped).
__global__ void __launch_bounds__(WAVE)
k_ls_append(ls_store L, const double* __restrict__ cutbuf, const double* __restrict__ eta, double tol,
            double* __restrict__ info) {
    const int nn = L.nn, P = nn + 2, G = L.G;
    const int g = threadIdx.x;
    const double Q = g < G ? cutbuf[g * P + nn + 1] : 0.0;
    const bool want = g < G && Q - eta[g] > tol * fmax(1.0, fabs(Q));
    const unsigned long long m = __ballot(want);
    const int held = L.ncuts[0];
    const int room = L.max_cuts - held;
    const int pos = (int)__popcll(m & ((1ull << g) - 1ull));
    int added = (int)__popcll(m);
    if (added > room) added = room;
    double qs = 0.0;
    for (int u = 0; u < G; ++u) qs += cutbuf[u * P + nn + 1];
    for (int u = 0; u < G; ++u) {
        if (!((m >> u) & 1ull)) continue;
        const int pu = (int)__popcll(m & ((1ull << u) - 1ull));
        if (pu >= room) break;
        const int c = held + pu;
        for (int k = threadIdx.x; k < nn; k += WAVE) L.cut_a[(size_t)k * L.max_cuts + c] = cutbuf[u * P + k];
    }
    if (want && pos < room) {
        L.cut_b[held + pos] = cutbuf[g * P + nn];
        L.cut_g[held + pos] = g;
    }
    __syncthreads();
    if (threadIdx.x == 0) L.ncuts[0] = held + added;
    if (threadIdx.x < 5) {
        const int t = threadIdx.x;
        info[t] = t == 0 ? (double)added
                         : (t == 1 ? qs : (t == 2 ? (double)(held + added) : (t == 3 ? cutbuf[G * P] : (double)__popcll(m))));
    }
}
#endif  // !LS_HOST
