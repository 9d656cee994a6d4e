// The extensive form of a two-stage problem by one interior point over all scenarios, decomposed
// by a Schur complement in the first-stage variables (mpisppy/opt/ef.py, opt/sc.py; phgpu_ef_*,
// include/phgpu.h; DESIGN.md 3.21).  Included by phgpu.hip after ph_lshaped.inc, whose dense
// Cholesky (ls_chol, ls_fwd, ls_bwd) factors the Schur complement.
//
//   min sum_s p_s (c_s.x_s + 1/2 x_s.q_s x_s)   rl_s <= A_s x_s <= ru_s, lb_s <= x_s <= ub_s, x_s[N] = z
//
// with z substituted for the nonant columns N: A_s = [T_s | W_s].  Per scenario the other columns
// x (boxed, duals zl zu), the activities w of the rows with rl < ru (boxed, duals vl vu) and the
// row duals y; once, z (boxed, duals zlz zuz).  One Newton system per right-hand side:
//
//   N_s = W D W' + E,  C = Dz^-1 + sum_s T' N_s^-1 T,  C dz = -r_z + sum_s T' N_s^-1 g_s,
//   dy_s = N_s^-1 (g_s - T dz),  dx = D (W' dy - r_x),  dw = T dz + W dx + r_p
//
// One lane per scenario.  Everything a lane keeps between passes is in the store's [k][S]
// arrays (scenario-fastest, coalesced), the dense LDL' factor of N_s included.
#define EF_NN_MAX 64
#define EF_M_MAX 64
#define EF_T 128          // lanes per block of the scenario passes
#define EF_REG 1e-13      // diagonal regularisation, relative to each matrix's own diagonal
#define EF_CTL 32         // control scalars (ef_ctl)

enum ef_ctl {
    EC_IT = 0, EC_DONE, EC_MU, EC_SIGMU, EC_AP, EC_AD, EC_COMP, EC_NCOMP, EC_CMAX, EC_TOL, EC_QP, EC_PRES, EC_DRES,
    EC_GAP, EC_OBJ, EC_HIST /* 6 */, EC_END = EC_HIST + 6
};
// behind them, in a segment's record (bundles): the tolerances of the segment's own test (ef_seg_test)
#define EC_SEG_TOL EC_END
#define EC_SEG_ZTOL (EC_END + 1)
static_assert(EC_SEG_ZTOL < EF_CTL, "ef_ctl");

struct ef_store {
    int nn, m, n, ntri, ld, nplanes;
    // per scenario [k][S]
    double *x, *zl, *zu, *dx, *dxa, *D;                  // [n] (the nonant columns' entries are not used)
    double *w, *vl, *vu, *y, *dw, *dwa, *dy, *dya, *g, *wk, *rp, *E;  // [m]
    double* fac;                                         // [m (m + 1) / 2]: L below, 1 / d on the diagonal
    double* terms;                                       // [nplanes]: what the lanes give to a reduction
    // once: zlb zub cz qz z zlz zuz dz dza [nn each], the Cholesky factor of C, the control scalars
    double *zd, *C, *ctl;
};
#define EF_Z(E, f) ((E).zd + (size_t)(f) * (E).nn)
enum ef_zf { EZ_LB = 0, EZ_UB, EZ_C, EZ_Q, EZ_Z, EZ_ZL, EZ_ZU, EZ_DZ, EZ_DZA, EZ_N };

#if defined(__HIPCC__) || defined(EF_HOST)
#ifdef EF_HOST
#define EF_FN static inline
#define EF_MFN inline
#else
#define EF_FN __device__ __forceinline__
#define EF_MFN __device__ __forceinline__
#endif

// a point strictly inside [lo, hi] (the host sets z's start with it)
#ifndef EF_HOST
__host__
#endif
EF_FN double ef_inside(double lo, double hi) {
    const bool fl = isfinite(lo), fu = isfinite(hi);
    if (fl && fu) return 0.5 * (lo + hi);
    if (fl) return lo + fmax(1.0, 0.1 * fabs(lo));
    if (fu) return hi - fmax(1.0, 0.1 * fabs(hi));
    return 0.0;
}

// A z entry held at a value (phgpu_eft_fix; DESIGN.md 3.24) is stored with the empty box lo = +inf,
// hi = -inf: neither side is finite, so wherever a box is read it has no slack, no dual, no
// complementarity and no ratio, and this test tells it from a free entry.  Nothing else sets such a box.
EF_FN bool ef_held(double lo, double hi) { return lo > hi; }

// One boxed variable: value v in [lo, hi], duals zl zu, direction d.
struct ef_box {
    bool fl, fu;
    double sl, su, zl, zu;
};
EF_FN ef_box ef_mkbox(double v, double lo, double hi, double zl, double zu) {
    ef_box b;
    b.fl = isfinite(lo);
    b.fu = isfinite(hi);
    b.sl = b.fl ? v - lo : 1.0;
    b.su = b.fu ? hi - v : 1.0;
    b.zl = zl;
    b.zu = zu;
    return b;
}
EF_FN double ef_theta(const ef_box& b) { return b.zl / b.sl + b.zu / b.su; }
EF_FN double ef_push(const ef_box& b, double tl, double tu) { return (b.fl ? tl / b.sl : 0.0) - (b.fu ? tu / b.su : 0.0); }
// The duals' directions from the complementarity rows with targets tl, tu.  use_diff: dzl - dzu has
// to be diff for the stationarity row to hold exactly; the side with the larger z / s takes it from
// there (its complementarity row absorbs the rounding of d, which it can: an error e of d moves
// s z by z e, while through the other route it moves the dual residual by z e / s).
EF_FN void ef_dual_dirs(const ef_box& b, double d, double tl, double tu, bool use_diff, double diff, double& dzl,
                        double& dzu) {
    dzl = b.fl ? (tl - b.zl * d) / b.sl - b.zl : 0.0;
    dzu = b.fu ? (tu + b.zu * d) / b.su - b.zu : 0.0;
    if (use_diff) {
        const bool low = b.fl && (!b.fu || b.zl / b.sl >= b.zu / b.su);
        if (low) dzl = diff + dzu;
        else if (b.fu) dzu = dzl - diff;
    }
}
// the corrector's targets from the affine direction da (stage 0: none)
EF_FN void ef_targets(int stage, double sigmu, const ef_box& b, double da, bool use_diff, double diffa, double& tl,
                      double& tu) {
    tl = tu = 0.0;
    if (stage == 0) return;
    double al, au;
    ef_dual_dirs(b, da, 0.0, 0.0, use_diff, diffa, al, au);
    tl = sigmu - da * al;
    tu = sigmu + da * au;
}
// what a direction gives to the step lengths (the largest -ds / s, -dz / z) and to the affine mu
EF_FN void ef_ratios(const ef_box& b, double d, double dzl, double dzu, double& rp, double& rd, double (&ct)[3]) {
    if (b.fl) {
        rp = fmax(rp, -d / b.sl);
        rd = fmax(rd, -dzl / b.zl);
        ct[0] += b.sl * dzl;
        ct[1] += d * b.zl;
        ct[2] += d * dzl;
    }
    if (b.fu) {
        rp = fmax(rp, d / b.su);
        rd = fmax(rd, -dzu / b.zu);
        ct[0] += b.su * dzu;
        ct[1] -= d * b.zu;
        ct[2] -= d * dzu;
    }
}
#define EF_TRI(i, j) ((i) * ((i) + 1) / 2 + (j))  // j <= i

// the lane's scenario in the store: the solves on its factor
struct ef_lane {
    const ef_store& E;
    int64_t S, s;
    EF_MFN size_t ix(int k) const { return (size_t)k * (size_t)S + (size_t)s; }
    // wk = N^-1 wk from the LDL' factor
    EF_MFN void solve() const {
        const int m = E.m;
        for (int i = 0; i < m; ++i) {
            double a = E.wk[ix(i)];
            for (int k = 0; k < i; ++k) a -= E.fac[ix(EF_TRI(i, k))] * E.wk[ix(k)];
            E.wk[ix(i)] = a;
        }
        for (int i = 0; i < m; ++i) E.wk[ix(i)] *= E.fac[ix(EF_TRI(i, i))];
        for (int i = m - 1; i >= 0; --i) {
            double a = E.wk[ix(i)];
            for (int k = i + 1; k < m; ++k) a -= E.fac[ix(EF_TRI(k, i))] * E.wk[ix(k)];
            E.wk[ix(i)] = a;
        }
    }
};

// column j of the lane's matrix dotted with the row vector v [m][S]
EF_FN double ef_col_dot(const ph_data& st, int64_t S, int64_t s, int j, const double* v) {
    double a = 0.0;
    for (int kc = st.col_ptr[j]; kc < st.col_ptr[j + 1]; ++kc) a += st.A[IX(st.perm[kc])] * v[IX(st.row_idx[kc])];
    return a;
}

// ------------------------------------------------------------------ the start
EF_FN void ef_start_lane(const ph_data& st, const ef_store& E, int64_t s) {
    const int64_t S = st.S;
    const double p = st.prob[s];
    for (int j = 0; j < st.n; ++j) {
        const double lo = st.lb[IX(j)], hi = st.ub[IX(j)];
        const double sc = p * (1.0 + fabs(st.c[IX(j)]));
        E.x[IX(j)] = ef_inside(lo, hi);
        E.zl[IX(j)] = isfinite(lo) ? sc : 0.0;
        E.zu[IX(j)] = isfinite(hi) ? sc : 0.0;
        E.dx[IX(j)] = E.dxa[IX(j)] = E.D[IX(j)] = 0.0;
    }
    for (int i = 0; i < st.m; ++i) {
        const double lo = st.rl[IX(i)], hi = st.ru[IX(i)];
        const bool eq = lo == hi;
        E.w[IX(i)] = eq ? lo : ef_inside(lo, hi);
        const double a = (!eq && isfinite(lo)) ? p : 0.0, b = (!eq && isfinite(hi)) ? p : 0.0;
        E.vl[IX(i)] = a;
        E.vu[IX(i)] = b;
        E.y[IX(i)] = a - b;
        E.dw[IX(i)] = E.dwa[IX(i)] = E.dy[IX(i)] = E.dya[IX(i)] = 0.0;
    }
}

// ------------------------------------------------------------------ the scenario pass
// stage 0: residuals, D, E, N_s and its factor, T' N^-1 T, and the predictor's g; stage 1: the
// corrector's g on the same factor.  What the lane gives to the sums and maxima goes to E.terms:
//   stage 0  sums: C (ntri, lower triangle by rows) | T' N^-1 g (nn) | T' y (nn) | comp | obj
//            maxima: primal residual | dual residual
//   stage 1  sums: T' N^-1 g (nn)
EF_FN void ef_schur_lane(const ph_data& st, const ef_store& E, int64_t s, int stage) {
    const int64_t S = st.S;
    if (E.ctl[EC_DONE] != 0.0) return;
    const ef_lane L{E, S, s};
    const int n = st.n, m = st.m, nn = st.nn;
    const double p = st.prob[s], sigmu = E.ctl[EC_SIGMU];
    const double* z = EF_Z(E, EZ_Z);
    double comp = 0.0, obj = st.objc ? p * st.objc[s] : 0.0, pres = 0.0, dres = 0.0;
    // rows: r_p, E, r_w(t) -> E.g holds -r_p - E r_w for now
    for (int i = 0; i < m; ++i) {
        const double lo = st.rl[IX(i)], hi = st.ru[IX(i)];
        const bool eq = lo == hi;
        double e = 0.0, rw = 0.0, rp = E.rp[IX(i)];
        if (stage == 0) {
            double a = 0.0;
            for (int kk = st.row_ptr[i]; kk < st.row_ptr[i + 1]; ++kk) {
                const int j = st.col_idx[kk], k = st.nonant_slot[j];
                a += st.A[IX(kk)] * (k >= 0 ? z[k] : E.x[IX(j)]);
            }
            rp = a - (eq ? lo : E.w[IX(i)]);
            E.rp[IX(i)] = rp;
            pres = fmax(pres, fabs(rp) / (1.0 + fmax(isfinite(lo) ? fabs(lo) : 0.0, isfinite(hi) ? fabs(hi) : 0.0)));
        }
        if (!eq) {
            const ef_box b = ef_mkbox(E.w[IX(i)], lo, hi, E.vl[IX(i)], E.vu[IX(i)]);
            const double yv = E.y[IX(i)], rw0 = yv - b.zl + b.zu;
            double tl, tu;
            ef_targets(stage, sigmu, b, E.dwa[IX(i)], true, E.dya[IX(i)] + rw0, tl, tu);
            rw = yv - ef_push(b, tl, tu);
            if (stage == 0) {
                e = 1.0 / fmax(ef_theta(b), 1e-300);
                E.E[IX(i)] = e;
                dres = fmax(dres, fabs(rw0));
                comp += (b.fl ? b.sl * b.zl : 0.0) + (b.fu ? b.su * b.zu : 0.0);
            } else {
                e = E.E[IX(i)];
            }
        } else if (stage == 0) {
            E.E[IX(i)] = 0.0;
        }
        E.g[IX(i)] = -rp - e * rw;
    }
    // columns: D, u = D r_x(t) (kept in E.dx), the objective
    for (int j = 0; j < n; ++j) {
        const int k = st.nonant_slot[j];
        const double cj = st.c[IX(j)], qj = st.q ? st.q[IX(j)] : 0.0;
        if (k >= 0) {
            if (stage == 0) obj += p * (cj * z[k] + 0.5 * qj * z[k] * z[k]);
            continue;
        }
        const double xv = E.x[IX(j)];
        const ef_box b = ef_mkbox(xv, st.lb[IX(j)], st.ub[IX(j)], E.zl[IX(j)], E.zu[IX(j)]);
        const double lin = p * cj + p * qj * xv - ef_col_dot(st, S, s, j, E.y);
        double d = E.D[IX(j)];
        if (stage == 0) {
            d = 1.0 / (p * qj + ef_theta(b) + 1e-12 * p);
            E.D[IX(j)] = d;
            obj += p * (cj * xv + 0.5 * qj * xv * xv);
            dres = fmax(dres, fabs(lin - b.zl + b.zu));
            comp += (b.fl ? b.sl * b.zl : 0.0) + (b.fu ? b.su * b.zu : 0.0);
        }
        double tl, tu;
        ef_targets(stage, sigmu, b, E.dxa[IX(j)], false, 0.0, tl, tu);
        E.dx[IX(j)] = d * (lin - ef_push(b, tl, tu));
    }
    // g += W u
    for (int i = 0; i < m; ++i) {
        double a = E.g[IX(i)];
        for (int kk = st.row_ptr[i]; kk < st.row_ptr[i + 1]; ++kk) {
            const int j = st.col_idx[kk];
            if (st.nonant_slot[j] < 0) a += st.A[IX(kk)] * E.dx[IX(j)];
        }
        E.g[IX(i)] = a;
    }
    const int ntri = E.ntri;
    if (stage == 0) {
        // N = W D W' + E, regularised on its own diagonal, and its LDL' in place
        for (int e = 0; e < m * (m + 1) / 2; ++e) E.fac[IX(e)] = 0.0;
        for (int j = 0; j < n; ++j) {
            if (st.nonant_slot[j] >= 0) continue;
            const double d = E.D[IX(j)];
            for (int k1 = st.col_ptr[j]; k1 < st.col_ptr[j + 1]; ++k1) {
                const int r1 = st.row_idx[k1];
                const double a1 = d * st.A[IX(st.perm[k1])];
                for (int k2 = st.col_ptr[j]; k2 < st.col_ptr[j + 1]; ++k2) {
                    const int r2 = st.row_idx[k2];
                    if (r2 <= r1) E.fac[IX(EF_TRI(r1, r2))] += a1 * st.A[IX(st.perm[k2])];
                }
            }
        }
        double dmax = 0.0;
        for (int i = 0; i < m; ++i) {
            const double d = E.fac[IX(EF_TRI(i, i))] + E.E[IX(i)];
            E.fac[IX(EF_TRI(i, i))] = d + EF_REG * d;
            dmax = fmax(dmax, d);
        }
        for (int j = 0; j < m; ++j) {
            double d = E.fac[IX(EF_TRI(j, j))];
            for (int k = 0; k < j; ++k) {
                const double l = E.fac[IX(EF_TRI(j, k))];
                d -= l * l / E.fac[IX(EF_TRI(k, k))];
            }
            // a pivot that cancelled drops its direction (path 6's safeguard)
            const double id = (d > 1e-30 * dmax && isfinite(d)) ? 1.0 / d : 1e-128;
            E.fac[IX(EF_TRI(j, j))] = id;
            for (int i = j + 1; i < m; ++i) {
                double a = E.fac[IX(EF_TRI(i, j))];
                for (int k = 0; k < j; ++k)
                    a -= E.fac[IX(EF_TRI(i, k))] * E.fac[IX(EF_TRI(j, k))] / E.fac[IX(EF_TRI(k, k))];
                E.fac[IX(EF_TRI(i, j))] = a * id;
            }
        }
        // T' N^-1 T: one solve per nonant column
        for (int k = 0; k < nn; ++k) {
            const int j = st.nonant_col[k];
            for (int i = 0; i < m; ++i) E.wk[IX(i)] = 0.0;
            for (int kc = st.col_ptr[j]; kc < st.col_ptr[j + 1]; ++kc) E.wk[IX(st.row_idx[kc])] = st.A[IX(st.perm[kc])];
            L.solve();
            for (int l = 0; l <= k; ++l) E.terms[IX(EF_TRI(k, l))] = ef_col_dot(st, S, s, st.nonant_col[l], E.wk);
        }
        for (int k = 0; k < nn; ++k) E.terms[IX(ntri + nn + k)] = ef_col_dot(st, S, s, st.nonant_col[k], E.y);
        E.terms[IX(ntri + 2 * nn)] = comp;
        E.terms[IX(ntri + 2 * nn + 1)] = obj;
        E.terms[IX(ntri + 2 * nn + 2)] = pres;
        E.terms[IX(ntri + 2 * nn + 3)] = dres / p;
    }
    for (int i = 0; i < m; ++i) E.wk[IX(i)] = E.g[IX(i)];
    L.solve();
    const int base = stage == 0 ? ntri : 0;
    for (int k = 0; k < nn; ++k) E.terms[IX(base + k)] = ef_col_dot(st, S, s, st.nonant_col[k], E.wk);
}

// ------------------------------------------------------------------ the direction pass
// dy = N^-1 (g - T dz), dx, dw and the bound duals' directions; to E.terms the sums {s dz, ds z,
// ds dz} and the maxima {-ds / s, -dz / z}.  stage 0 keeps the direction as the affine one.
EF_FN void ef_direction_lane(const ph_data& st, const ef_store& E, int64_t s, int stage) {
    const int64_t S = st.S;
    if (E.ctl[EC_DONE] != 0.0) return;
    const ef_lane L{E, S, s};
    const int n = st.n, m = st.m;
    const double sigmu = E.ctl[EC_SIGMU];
    const double* dz = EF_Z(E, EZ_DZ);
    double rp = 0.0, rd = 0.0, ct[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < m; ++i) {
        double a = 0.0;
        for (int kk = st.row_ptr[i]; kk < st.row_ptr[i + 1]; ++kk) {
            const int k = st.nonant_slot[st.col_idx[kk]];
            if (k >= 0) a += st.A[IX(kk)] * dz[k];
        }
        E.dw[IX(i)] = a;  // (T dz, until dw is formed below)
        E.wk[IX(i)] = E.g[IX(i)] - a;
    }
    L.solve();
    for (int i = 0; i < m; ++i) E.dy[IX(i)] = E.wk[IX(i)];
    for (int j = 0; j < n; ++j) {
        if (st.nonant_slot[j] >= 0) continue;
        const double d = E.D[IX(j)] * ef_col_dot(st, S, s, j, E.dy) - E.dx[IX(j)];
        const ef_box b = ef_mkbox(E.x[IX(j)], st.lb[IX(j)], st.ub[IX(j)], E.zl[IX(j)], E.zu[IX(j)]);
        double tl, tu, dzl, dzu;
        ef_targets(stage, sigmu, b, E.dxa[IX(j)], false, 0.0, tl, tu);
        ef_dual_dirs(b, d, tl, tu, false, 0.0, dzl, dzu);
        ef_ratios(b, d, dzl, dzu, rp, rd, ct);
        E.dx[IX(j)] = d;
    }
    for (int i = 0; i < m; ++i) {
        const double lo = st.rl[IX(i)], hi = st.ru[IX(i)];
        if (lo == hi) {
            E.dw[IX(i)] = 0.0;
            continue;
        }
        double a = E.dw[IX(i)] + E.rp[IX(i)];
        for (int kk = st.row_ptr[i]; kk < st.row_ptr[i + 1]; ++kk) {
            const int j = st.col_idx[kk];
            if (st.nonant_slot[j] < 0) a += st.A[IX(kk)] * E.dx[IX(j)];
        }
        const ef_box b = ef_mkbox(E.w[IX(i)], lo, hi, E.vl[IX(i)], E.vu[IX(i)]);
        const double rw0 = E.y[IX(i)] - b.zl + b.zu;
        double tl, tu, dvl, dvu;
        ef_targets(stage, sigmu, b, E.dwa[IX(i)], true, E.dya[IX(i)] + rw0, tl, tu);
        ef_dual_dirs(b, a, tl, tu, true, E.dy[IX(i)] + rw0, dvl, dvu);
        ef_ratios(b, a, dvl, dvu, rp, rd, ct);
        E.dw[IX(i)] = a;
    }
    E.terms[IX(0)] = ct[0];
    E.terms[IX(1)] = ct[1];
    E.terms[IX(2)] = ct[2];
    E.terms[IX(3)] = rp;
    E.terms[IX(4)] = rd;
}

// the affine direction kept for the corrector's second-order term (after the affine step lengths
// have been taken from it: the stage-1 passes read dxa, dwa, dya)
EF_FN void ef_keep_lane(const ph_data& st, const ef_store& E, int64_t s) {
    const int64_t S = st.S;
    if (E.ctl[EC_DONE] != 0.0) return;
    for (int j = 0; j < st.n; ++j) E.dxa[IX(j)] = E.dx[IX(j)];
    for (int i = 0; i < st.m; ++i) {
        E.dwa[IX(i)] = E.dw[IX(i)];
        E.dya[IX(i)] = E.dy[IX(i)];
    }
}

// ------------------------------------------------------------------ the step
EF_FN void ef_step_lane(const ph_data& st, const ef_store& E, int64_t s) {
    const int64_t S = st.S;
    if (E.ctl[EC_DONE] != 0.0) return;
    const double sigmu = E.ctl[EC_SIGMU], ap = E.ctl[EC_AP], ad = E.ctl[EC_AD];
    for (int j = 0; j < st.n; ++j) {
        if (st.nonant_slot[j] >= 0) continue;
        const double d = E.dx[IX(j)];
        const ef_box b = ef_mkbox(E.x[IX(j)], st.lb[IX(j)], st.ub[IX(j)], E.zl[IX(j)], E.zu[IX(j)]);
        double tl, tu, dzl, dzu;
        ef_targets(1, sigmu, b, E.dxa[IX(j)], false, 0.0, tl, tu);
        ef_dual_dirs(b, d, tl, tu, false, 0.0, dzl, dzu);
        E.x[IX(j)] += ap * d;
        E.zl[IX(j)] += ad * dzl;
        E.zu[IX(j)] += ad * dzu;
    }
    for (int i = 0; i < st.m; ++i) {
        const double lo = st.rl[IX(i)], hi = st.ru[IX(i)];
        if (lo != hi) {
            const double d = E.dw[IX(i)];
            const ef_box b = ef_mkbox(E.w[IX(i)], lo, hi, E.vl[IX(i)], E.vu[IX(i)]);
            const double rw0 = E.y[IX(i)] - b.zl + b.zu;
            double tl, tu, dvl, dvu;
            ef_targets(1, sigmu, b, E.dwa[IX(i)], true, E.dya[IX(i)] + rw0, tl, tu);
            ef_dual_dirs(b, d, tl, tu, true, E.dy[IX(i)] + rw0, dvl, dvu);
            E.w[IX(i)] += ap * d;
            E.vl[IX(i)] += ad * dvl;
            E.vu[IX(i)] += ad * dvu;
        }
        E.y[IX(i)] += ad * E.dy[IX(i)];
    }
}

// ------------------------------------------------------------------ the Schur complement
// One workgroup, after the ranks' sums and maxima.  stage 0: the termination test of the iterate
// (info, 8 doubles, device or host-mapped: {iteration, mu, primal, dual, gap residual, objective,
// done: 0 no / 1 the iterate passes, iteration again}), then C = Dz^-1 + sum T' N^-1 T, its Cholesky
// factor (kept in E.C for stage 1) and the predictor's dz.  stage 1: the corrector's dz.
// (M: nn * ld + nn doubles and done: one int, both shared by the workgroup)
EF_FN void ef_solve_core(const ef_store& E, int stage, const double* rsum, const double* rmax, double* info, double* M,
                         int* done_) {
    const int nn = E.nn, ld = E.ld, ntri = E.ntri;
    double* rhs = M + (size_t)nn * ld;
    volatile int& done = *done_;
    const bool over = E.ctl[EC_DONE] != 0.0;
    LS_SYNC();  // (thread 0 sets the flag below: every thread has read it by now)
    if (over) return;
    const double *zlb = EF_Z(E, EZ_LB), *zub = EF_Z(E, EZ_UB), *cz = EF_Z(E, EZ_C), *qz = EF_Z(E, EZ_Q);
    double *z = EF_Z(E, EZ_Z), *zlz = EF_Z(E, EZ_ZL), *zuz = EF_Z(E, EZ_ZU), *dz = EF_Z(E, EZ_DZ), *dza = EF_Z(E, EZ_DZA);
    const double sigmu = E.ctl[EC_SIGMU];
    if (stage == 0) {
        if (LS_TID == 0) {
            const double* ty = rsum + ntri + nn;
            double comp = rsum[ntri + 2 * nn], rzm = 0.0;
            for (int k = 0; k < nn; ++k) {
                const ef_box b = ef_mkbox(z[k], zlb[k], zub[k], zlz[k], zuz[k]);
                comp += (b.fl ? b.sl * b.zl : 0.0) + (b.fu ? b.su * b.zu : 0.0);
                if (!ef_held(zlb[k], zub[k])) rzm = fmax(rzm, fabs(cz[k] + qz[k] * z[k] - ty[k] - zlz[k] + zuz[k]));
            }
            const double obj = rsum[ntri + 2 * nn + 1];
            const double mu = comp / E.ctl[EC_NCOMP];
            const double pres = rmax[0], dres = fmax(rmax[1], rzm) / (1.0 + E.ctl[EC_CMAX]);
            const double gap = comp / (1.0 + fabs(obj));
            const double tol = E.ctl[EC_TOL];
            done = (pres <= tol && dres <= tol && gap <= tol) ? 1 : 0;
            E.ctl[EC_MU] = mu;
            E.ctl[EC_COMP] = comp;
            E.ctl[EC_PRES] = pres;
            E.ctl[EC_DRES] = dres;
            E.ctl[EC_GAP] = gap;
            E.ctl[EC_OBJ] = obj;
            if (done) E.ctl[EC_DONE] = 1.0;
            info[1] = mu;
            info[2] = pres;
            info[3] = dres;
            info[4] = gap;
            info[5] = obj;
            info[6] = (double)done;
            info[7] = E.ctl[EC_IT];
            info[0] = E.ctl[EC_IT];
        }
        LS_SYNC();
        if (done) return;
        for (int e = LS_TID; e < nn * nn; e += LS_NT) {
            const int i = e / nn, j = e % nn;
            if (j <= i) M[i * ld + j] = rsum[EF_TRI(i, j)];
        }
        LS_SYNC();
        for (int k = LS_TID; k < nn; k += LS_NT) {
            if (ef_held(zlb[k], zub[k])) {  // its row and column: the identity's (off the diagonal, so no
                for (int j = 0; j < k; ++j) M[k * ld + j] = 0.0;       // other thread's entry; where two held
                for (int i = k + 1; i < nn; ++i) M[i * ld + k] = 0.0;  // entries meet both store the same 0)
                M[k * ld + k] = 1.0;
                continue;
            }
            const ef_box b = ef_mkbox(z[k], zlb[k], zub[k], zlz[k], zuz[k]);
            const double d = M[k * ld + k] + qz[k] + ef_theta(b);
            M[k * ld + k] = d + EF_REG * d;
        }
        LS_SYNC();
        double dmax = 0.0;
        for (int k = 0; k < nn; ++k) dmax = fmax(dmax, M[k * ld + k]);
        ls_chol(M, nn, ld, 1e-40 * dmax);
        for (int e = LS_TID; e < nn * ld; e += LS_NT) E.C[e] = M[e];
    } else {
        for (int e = LS_TID; e < nn * ld; e += LS_NT) M[e] = E.C[e];
    }
    const double* ng = rsum + (stage == 0 ? ntri : 0);
    const double* ty = EF_Z(E, EZ_N);  // (T' y of this iteration, kept behind the z fields by stage 0)
    for (int k = LS_TID; k < nn; k += LS_NT) {
        const ef_box b = ef_mkbox(z[k], zlb[k], zub[k], zlz[k], zuz[k]);
        double tl, tu;
        ef_targets(stage, sigmu, b, dza[k], false, 0.0, tl, tu);
        const double tyk = stage == 0 ? rsum[ntri + nn + k] : ty[k];
        if (stage == 0) EF_Z(E, EZ_N)[k] = tyk;
        rhs[k] = ef_held(zlb[k], zub[k]) ? 0.0 : -(cz[k] + qz[k] * z[k] - tyk - ef_push(b, tl, tu)) + ng[k];
    }
    LS_SYNC();
    ls_fwd(M, nn, ld, rhs);
    ls_bwd(M, nn, ld, rhs);
    for (int k = LS_TID; k < nn; k += LS_NT) dz[k] = ef_held(zlb[k], zub[k]) ? 0.0 : rhs[k];
}

// One wave, after the ranks' sums and maxima of a direction pass.  stage 0: the affine step
// lengths, the affine mu and sigma (Mehrotra's cube; once mu has not halved in five iterations at
// least 1/2); the affine dz is kept.  stage 1: the step lengths (0.995 of the way to the boundary, a common one for a
// QP), z's own step, the iteration count.
EF_FN void ef_ctrl_core(const ef_store& E, int stage, const double* rsum, const double* rmax) {
    if (E.ctl[EC_DONE] != 0.0) return;
    const int nn = E.nn;
    const double *zlb = EF_Z(E, EZ_LB), *zub = EF_Z(E, EZ_UB);
    double *z = EF_Z(E, EZ_Z), *zlz = EF_Z(E, EZ_ZL), *zuz = EF_Z(E, EZ_ZU), *dz = EF_Z(E, EZ_DZ), *dza = EF_Z(E, EZ_DZA);
    const double sigmu = E.ctl[EC_SIGMU];
    double rp = rmax[0], rd = rmax[1], ct[3] = {rsum[0], rsum[1], rsum[2]};
    for (int k = 0; k < nn; ++k) {
        const ef_box b = ef_mkbox(z[k], zlb[k], zub[k], zlz[k], zuz[k]);
        double tl, tu, dl, du;
        ef_targets(stage, sigmu, b, dza[k], false, 0.0, tl, tu);
        ef_dual_dirs(b, dz[k], tl, tu, false, 0.0, dl, du);
        ef_ratios(b, dz[k], dl, du, rp, rd, ct);
    }
    const double back = stage == 0 ? 1.0 : 0.995;
    double ap = fmin(1.0, back / fmax(rp, 1e-300)), ad = fmin(1.0, back / fmax(rd, 1e-300));
    if (E.ctl[EC_QP] != 0.0) ap = ad = fmin(ap, ad);
    if (stage == 0) {
        const double comp = E.ctl[EC_COMP], mu = E.ctl[EC_MU];
        const double mua = (comp + ad * ct[0] + ap * ct[1] + ap * ad * ct[2]) / E.ctl[EC_NCOMP];
        const double r = fmin(1.0, fmax(0.0, mua / fmax(mu, 1e-300)));
        double sigma = r * r * r;
        const int it = (int)E.ctl[EC_IT];
        if (it >= 5 && mu > 0.5 * E.ctl[EC_HIST + (it - 5) % 6]) sigma = fmax(sigma, 0.5);
        E.ctl[EC_HIST + it % 6] = mu;
        E.ctl[EC_SIGMU] = sigma * mu;
        for (int k = 0; k < nn; ++k) dza[k] = dz[k];
        return;
    }
    for (int k = 0; k < nn; ++k) {
        if (ef_held(zlb[k], zub[k])) continue;  // (z keeps its bits, a -0.0 included)
        const ef_box b = ef_mkbox(z[k], zlb[k], zub[k], zlz[k], zuz[k]);
        double tl, tu, dl, du;
        ef_targets(1, sigmu, b, dza[k], false, 0.0, tl, tu);
        ef_dual_dirs(b, dz[k], tl, tu, false, 0.0, dl, du);
        z[k] += ap * dz[k];
        zlz[k] += ad * dl;
        zuz[k] += ad * du;
    }
    E.ctl[EC_AP] = ap;
    E.ctl[EC_AD] = ad;
    E.ctl[EC_IT] += 1.0;
}

// ------------------------------------------------------------------ the solution
// z into every scenario's nonant columns (the same bits in every scenario), the other columns, the
// row duals per scenario (the extensive form's over p_s), each scenario's own objective
EF_FN void ef_export_lane(const ph_data& st, const ef_store& E, int64_t s, double* x, double* y, double* obj, double* bound,
                          int32_t* status, int32_t* iters) {
    const int64_t S = st.S;
    const double* z = EF_Z(E, EZ_Z);
    const double p = st.prob[s];
    double o = st.objc ? st.objc[s] : 0.0;
    for (int j = 0; j < st.n; ++j) {
        const int k = st.nonant_slot[j];
        const double v = k >= 0 ? z[k] : E.x[IX(j)];
        x[IX(j)] = v;
        o += st.c[IX(j)] * v + 0.5 * (st.q ? st.q[IX(j)] : 0.0) * v * v;
    }
    if (y)
        for (int i = 0; i < st.m; ++i) y[IX(i)] = E.y[IX(i)] / p;
    obj[s] = o;
    bound[s] = o;
    status[s] = E.ctl[EC_DONE] == 1.0 ? PHGPU_OPTIMAL : PHGPU_ITER_LIMIT;
    iters[s] = (int32_t)E.ctl[EC_IT];
}
// ------------------------------------------------------------------ segments (bundles; DESIGN.md 3.22)
// The local scenarios in G contiguous segments, each an extensive form of its own: G copies of
// the zd block, of C and of ctl, segment-major.  A segment's view of the store offsets the three;
// every function above then runs on it unchanged.  The ph_data the lanes get is a view too: prob
// is the conditional probability p_s / p_B, c and q carry the PH terms on the nonant columns.
#define EF_ZD_LEN(E) ((size_t)(EZ_N + 1) * (E).nn)
EF_FN ef_store ef_seg_view(const ef_store& E, int64_t g) {
    ef_store V = E;
    V.zd = E.zd + (size_t)g * EF_ZD_LEN(E);
    V.C = E.C + (size_t)g * E.nn * E.ld;
    V.ctl = E.ctl + (size_t)g * EF_CTL;
    return V;
}

// A segment's start (V its view, scenarios s0 .. s1 - 1): cz, qz summed in index order from the
// view's c, q and prob, z inside its bounds (zlb, zub stay as set at init), its duals, no
// direction; the control scalars zeroed but for the static ones (ncomp, cmax, tol).
EF_FN void ef_seg_start(const ph_data& st, const ef_store& V, int64_t s0, int64_t s1, bool qp) {
    const int64_t S = st.S;
    const int nn = V.nn;
    const double *zlb = EF_Z(V, EZ_LB), *zub = EF_Z(V, EZ_UB);
    bool anyq = qp;
    for (int k = 0; k < nn; ++k) {
        const int j = st.nonant_col[k];
        double cz = 0.0, qz = 0.0;
        for (int64_t s = s0; s < s1; ++s) {
            cz += st.prob[s] * st.c[IX(j)];
            qz += st.prob[s] * (st.q ? st.q[IX(j)] : 0.0);
        }
        anyq = anyq || qz != 0.0;
        EF_Z(V, EZ_C)[k] = cz;
        EF_Z(V, EZ_Q)[k] = qz;
        EF_Z(V, EZ_Z)[k] = ef_inside(zlb[k], zub[k]);
        EF_Z(V, EZ_ZL)[k] = isfinite(zlb[k]) ? 1.0 + fabs(cz) : 0.0;
        EF_Z(V, EZ_ZU)[k] = isfinite(zub[k]) ? 1.0 + fabs(cz) : 0.0;
        EF_Z(V, EZ_DZ)[k] = EF_Z(V, EZ_DZA)[k] = EF_Z(V, EZ_N)[k] = 0.0;
    }
    for (int e = 0; e < EF_CTL; ++e)
        if (e != EC_NCOMP && e != EC_CMAX && e != EC_TOL && e != EC_SEG_TOL && e != EC_SEG_ZTOL) V.ctl[e] = 0.0;
    V.ctl[EC_QP] = anyq ? 1.0 : 0.0;
}

// EC_DONE of a segment: 0 iterating, 1 its iterate passed the test, EF_SEG_STOPPED it was stopped
// because a number of its iteration is not finite (it keeps the iterate it had; not OPTIMAL)
#define EF_SEG_STOPPED 2.0
// A segment's own test, by one thread after ef_solve_core(stage 0) and ef_seg_refine.  The core's
// test is switched off (ctl[EC_TOL] < 0), so it has stored the residuals of the iterate and gone on
// to the predictor's dz.  The segment is over when the three residuals are at most tol AND the
// predictor's step of z is at most ztol (1 + max |z|): near the solution that Newton step is the
// distance of z from it, which the residuals do not bound (the gap bounds the objective, and z only
// by its square root; DESIGN.md 3.22).  A complementarity that is not finite stops the segment.
EF_FN void ef_seg_test(const ef_store& V) {
    if (V.ctl[EC_DONE] != 0.0) return;
    if (!isfinite(V.ctl[EC_MU])) {
        V.ctl[EC_DONE] = EF_SEG_STOPPED;
        return;
    }
    const double tol = V.ctl[EC_SEG_TOL];
    if (!(V.ctl[EC_PRES] <= tol && V.ctl[EC_DRES] <= tol && V.ctl[EC_GAP] <= tol)) return;
    const double *z = EF_Z(V, EZ_Z), *dz = EF_Z(V, EZ_DZ);
    double zm = 0.0, dm = 0.0;
    for (int k = 0; k < V.nn; ++k) {
        zm = fmax(zm, fabs(z[k]));
        dm = fmax(dm, fabs(dz[k]));
    }
    if (dm <= V.ctl[EC_SEG_ZTOL] * (1.0 + zm)) V.ctl[EC_DONE] = 1.0;
}
// After a segment's ef_solve_core (M: the Cholesky factor and behind it nn doubles, as the core
// leaves them): dz corrected for the regularisation of C.  The core solves (C + R) dz = rhs with
// R = EF_REG diag(C); the exact dz is dz + C^-1 R dz, to first order dz + (C + R)^-1 R dz: one more
// solve on the same factor, with diag(C + R) read off the factor's rows.  Without it R dz is left in
// z's stationarity row at every step; C grows like 1 / mu, and a bundle's dual residual then stalls
// above 1e-10 (1 + max |c|) (DESIGN.md 3.22).  A pivot the factorisation dropped takes no part.
EF_FN void ef_seg_refine(const ef_store& V, double* M) {
    if (V.ctl[EC_DONE] != 0.0) return;  // (the same for every thread: thread 0 stops a segment after this)
    const int nn = V.nn, ld = V.ld;
    double* r = M + (size_t)nn * ld;
    double* dz = EF_Z(V, EZ_DZ);
    LS_SYNC();
    for (int k = LS_TID; k < nn; k += LS_NT) {
        double d = 0.0;
        for (int j = 0; j <= k; ++j) d += M[k * ld + j] * M[k * ld + j];
        r[k] = M[k * ld + k] < 1e60 ? (EF_REG / (1.0 + EF_REG)) * d * dz[k] : 0.0;
    }
    LS_SYNC();
    ls_fwd(M, nn, ld, r);
    ls_bwd(M, nn, ld, r);
    for (int k = LS_TID; k < nn; k += LS_NT) dz[k] += r[k];
}
// a segment's control step: ef_ctrl_core unless the direction's sums or dz are not finite, which
// stops the segment before the step is taken (every later pass returns at its first instruction)
EF_FN void ef_seg_ctrl(const ef_store& V, int stage, const double* rsum, const double* rmax) {
    if (V.ctl[EC_DONE] != 0.0) return;
    bool ok = isfinite(rsum[0]) && isfinite(rsum[1]) && isfinite(rsum[2]) && isfinite(rmax[0]) && isfinite(rmax[1]);
    const double* dz = EF_Z(V, EZ_DZ);
    for (int k = 0; k < V.nn; ++k) ok = ok && isfinite(dz[k]);
    if (!ok) {
        V.ctl[EC_DONE] = EF_SEG_STOPPED;
        return;
    }
    ef_ctrl_core(V, stage, rsum, rmax);
}
#endif  // __HIPCC__ || EF_HOST

#if defined(__HIPCC__) && !defined(EF_HOST)
// ------------------------------------------------------------------ kernels
#define EF_LANE(call)                                                 \
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; \
    if (s < st.S) call
__global__ void __launch_bounds__(EF_T) k_ef_start(ph_data st, ef_store E) { EF_LANE(ef_start_lane(st, E, s)); }
__global__ void __launch_bounds__(EF_T) k_ef_schur(ph_data st, ef_store E, int stage) {
    EF_LANE(ef_schur_lane(st, E, s, stage));
}
__global__ void __launch_bounds__(EF_T) k_ef_direction(ph_data st, ef_store E, int stage) {
    EF_LANE(ef_direction_lane(st, E, s, stage));
}
__global__ void __launch_bounds__(EF_T) k_ef_keep(ph_data st, ef_store E) { EF_LANE(ef_keep_lane(st, E, s)); }
__global__ void __launch_bounds__(EF_T) k_ef_step(ph_data st, ef_store E) { EF_LANE(ef_step_lane(st, E, s)); }
__global__ void __launch_bounds__(EF_T)
k_ef_export(ph_data st, ef_store E, double* __restrict__ x, double* __restrict__ y, double* __restrict__ obj,
            double* __restrict__ bound, int32_t* __restrict__ status, int32_t* __restrict__ iters) {
    EF_LANE(ef_export_lane(st, E, s, x, y, obj, bound, status, iters));
}

// ------------------------------------------------------------------ the reduction
// block b: plane b of E.terms over the local scenarios, a sum (b < nsum) or a maximum of
// non-negative values.  Every thread takes its scenarios in index order, the block its threads in
// a fixed order: the same bits on every run.
__global__ void __launch_bounds__(GR_T)
k_ef_reduce(ef_store E, int64_t S, int nsum, double* __restrict__ osum, double* __restrict__ omax) {
    __shared__ double red[GR_T / WAVE];
    const int b = blockIdx.x;
    const bool mx = b >= nsum;
    double acc = 0.0;
    for (int64_t s = threadIdx.x; s < S; s += GR_T) {
        const double v = E.terms[IX(b)];
        acc = mx ? fmax(acc, v) : acc + v;
    }
    if (!mx) {
        const double t = block_sum_fixed(acc, red);
        if (threadIdx.x == 0) osum[b] = t;
        return;
    }
    acc = wave_max(acc);
    if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int u = 0; u < GR_T / WAVE; ++u) t = fmax(t, red[u]);
        omax[b - nsum] = t;
    }
}

extern __shared__ double ef_dyn[];
__global__ void __launch_bounds__(LS_T)
k_ef_solve(ef_store E, int stage, const double* __restrict__ rsum, const double* __restrict__ rmax,
           double* __restrict__ info) {
    __shared__ int done;
    ef_solve_core(E, stage, rsum, rmax, info, ef_dyn, &done);
}
__global__ void __launch_bounds__(WAVE)
k_ef_ctrl(ef_store E, int stage, const double* __restrict__ rsum, const double* __restrict__ rmax) {
    if (threadIdx.x == 0) ef_ctrl_core(E, stage, rsum, rmax);
}

// ------------------------------------------------------------------ segments: kernels (DESIGN.md 3.22)
// what the segmented kernels read besides the store: the segments, the per-solve copies of the
// cost and the diagonal with the PH terms, and each segment's sums and maxima
struct ef_segs {
    int G, nsum0;
    const int32_t *seg_start, *seg_of;  // [G + 1], [S]
    double *cprob, *ceff, *qeff;        // [S], [n][S], [n][S]
    double *rsum, *rmax;                // [G][nsum0], [G][2]
};
#define EF_SEG_LANE(call)                                             \
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; \
    if (s < st.S) {                                                   \
        const ef_store V = ef_seg_view(E, B.seg_of[s]);               \
        call;                                                         \
    }

// The solve's cost and diagonal per scenario (raw: the handle's own data; W, rho, xbar [nn][S]):
// c + W_on W - prox_on rho xbar and q + prox_on rho on the nonant columns; then the lane's start.
// st is the view (prob = B.cprob, c = B.ceff, q = B.qeff).
__global__ void __launch_bounds__(EF_T)
k_bd_start(ph_data st, ef_store E, ef_segs B, const double* __restrict__ c0, const double* __restrict__ q0,
           const double* __restrict__ W, const double* __restrict__ rho, const double* __restrict__ xbar, int W_on,
           int prox_on) {
    const int64_t S = st.S;
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    for (int j = 0; j < st.n; ++j) {
        const int k = st.nonant_slot[j];
        double c = c0[IX(j)], q = q0 ? q0[IX(j)] : 0.0;
        if (k >= 0) {
            if (W_on) c += W[IX(k)];
            if (prox_on) {
                c -= rho[IX(k)] * xbar[IX(k)];
                q += rho[IX(k)];
            }
        }
        B.ceff[IX(j)] = c;
        B.qeff[IX(j)] = q;
    }
    ef_start_lane(st, ef_seg_view(E, B.seg_of[s]), s);
}
// one thread per segment, after k_bd_start
__global__ void __launch_bounds__(EF_T) k_bd_zstart(ph_data st, ef_store E, ef_segs B, int qp) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < B.G) ef_seg_start(st, ef_seg_view(E, g), B.seg_start[g], B.seg_start[g + 1], qp != 0);
}
__global__ void __launch_bounds__(EF_T) k_bd_schur(ph_data st, ef_store E, ef_segs B, int stage) {
    EF_SEG_LANE(ef_schur_lane(st, V, s, stage));
}
__global__ void __launch_bounds__(EF_T) k_bd_direction(ph_data st, ef_store E, ef_segs B, int stage) {
    EF_SEG_LANE(ef_direction_lane(st, V, s, stage));
}
__global__ void __launch_bounds__(EF_T) k_bd_keep(ph_data st, ef_store E, ef_segs B) { EF_SEG_LANE(ef_keep_lane(st, V, s)); }
__global__ void __launch_bounds__(EF_T) k_bd_step(ph_data st, ef_store E, ef_segs B) { EF_SEG_LANE(ef_step_lane(st, V, s)); }

// The segmented reduction: one THREAD per (plane, segment), the segment fastest over the threads;
// it walks its segment's scenarios of its plane in index order, so the order of addition is fixed
// and there are no atomics.  A segment that is over is skipped.
__global__ void __launch_bounds__(GR_T) k_bd_reduce(ef_store E, ef_segs B, int64_t S, int nsum, int nmax) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)(nsum + nmax) * B.G) return;
    const int b = (int)(t / B.G), g = (int)(t % B.G);
    if (E.ctl[(size_t)g * EF_CTL + EC_DONE] != 0.0) return;
    const bool mx = b >= nsum;
    double acc = 0.0;
    for (int64_t s = B.seg_start[g]; s < B.seg_start[g + 1]; ++s) {
        const double v = E.terms[IX(b)];
        acc = mx ? fmax(acc, v) : acc + v;
    }
    if (mx) B.rmax[(size_t)g * 2 + (b - nsum)] = acc;
    else B.rsum[(size_t)g * B.nsum0 + b] = acc;
}

// One wave per segment: C in LDS (dynamic, the only shared memory of the kernel, so its base is
// aligned; the flag sits behind the matrix and the right-hand side).  info8 [G][8]: the cores'
// records, device memory.
__global__ void __launch_bounds__(WAVE) k_bd_solve(ef_store E, ef_segs B, int stage, double* __restrict__ info8) {
    const int g = blockIdx.x;
    const ef_store V = ef_seg_view(E, g);
    int* done = (int*)(ef_dyn + (size_t)E.nn * E.ld + E.nn);
    ef_solve_core(V, stage, B.rsum + (size_t)g * B.nsum0, B.rmax + (size_t)g * 2, info8 + (size_t)g * 8, ef_dyn, done);
    ef_seg_refine(V, ef_dyn);
    __syncthreads();  // (dz is whole before one thread reads it)
    if (stage == 0 && threadIdx.x == 0) ef_seg_test(V);
}
// one thread per segment
__global__ void __launch_bounds__(EF_T) k_bd_ctrl(ef_store E, ef_segs B, int stage) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < B.G) ef_seg_ctrl(ef_seg_view(E, g), stage, B.rsum + (size_t)g * B.nsum0, B.rmax + (size_t)g * 2);
}

// The host's record of an iteration (one workgroup, after the stage-0 solve; info: 8 doubles,
// host-mapped): {seq, segments still iterating, the worst primal, dual and gap residual among
// them, segments stopped on a number that is not finite, the largest iteration count, seq again
// (stored last)}.  The count by an integer atomic in LDS, the maxima in a fixed order.
__global__ void __launch_bounds__(GR_T) k_bd_record(ef_store E, int G, double seq, double* __restrict__ info) {
    __shared__ double red[4][GR_T / WAVE];
    __shared__ int cnt[2];
    if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
    __syncthreads();
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    int open = 0, stopped = 0;
    for (int g = threadIdx.x; g < G; g += GR_T) {
        const double* ctl = E.ctl + (size_t)g * EF_CTL;
        v[3] = fmax(v[3], ctl[EC_IT]);
        if (ctl[EC_DONE] == EF_SEG_STOPPED) ++stopped;
        if (ctl[EC_DONE] != 0.0) continue;
        ++open;
        v[0] = fmax(v[0], ctl[EC_PRES]);
        v[1] = fmax(v[1], ctl[EC_DRES]);
        v[2] = fmax(v[2], ctl[EC_GAP]);
    }
    if (open) atomicAdd(&cnt[0], open);
    if (stopped) atomicAdd(&cnt[1], stopped);
    for (int u = 0; u < 4; ++u) {
        const double w = wave_max(v[u]);
        if ((threadIdx.x & (WAVE - 1)) == 0) red[u][threadIdx.x / WAVE] = w;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int u = 0; u < 4; ++u) {
            double t = 0.0;
            for (int w = 0; w < GR_T / WAVE; ++w) t = fmax(t, red[u][w]);
            v[u] = t;
        }
        info[1] = (double)cnt[0];
        info[2] = v[0];
        info[3] = v[1];
        info[4] = v[2];
        info[5] = (double)cnt[1];
        info[6] = v[3];
        info[7] = seq;
        info[0] = seq;
    }
}

// The segments' iterates as a solve's outputs: ef_export_lane on the view (its c and q hold the PH
// terms), plus the prox term's constant; bound = obj, so that sum_s p_s bound[s] over a segment is
// p_B times the segment's objective.
__global__ void __launch_bounds__(EF_T)
k_bd_export(ph_data st, ef_store E, ef_segs B, const double* __restrict__ rho, const double* __restrict__ xbar,
            int prox_on, double* __restrict__ x, double* __restrict__ y, double* __restrict__ obj,
            double* __restrict__ bound, int32_t* __restrict__ status, int32_t* __restrict__ iters) {
    const int64_t S = st.S;
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    ef_export_lane(st, ef_seg_view(E, B.seg_of[s]), s, x, y, obj, bound, status, iters);
    double o = obj[s];
    if (prox_on)
        for (int k = 0; k < st.nn; ++k) o += 0.5 * rho[IX(k)] * xbar[IX(k)] * xbar[IX(k)];
    obj[s] = o;
    bound[s] = o;
}
#endif
