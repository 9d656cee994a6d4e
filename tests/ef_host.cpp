// The extensive form's interior point on the host: the lane functions and the Schur workgroup's
// core of csrc/ph_ef.inc compiled for one thread (EF_HOST, LS_HOST), driven as the library drives
// the kernels, behind a C entry that tests/test_ef.py loads with ctypes and compares with the numpy
// restatement (tests/ef_ref.py) and HiGHS.  Buffers are heap blocks of the exact size, so the same
// file, built as a stand-alone program with a sanitizer, sees every overrun (EF_HOST_MAIN).
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "phgpu.h"
#define LS_HOST
#define EF_HOST
#define WAVE 64
#define IX(k) ((size_t)(k) * (size_t)S + (size_t)s)
// what the lane functions read of the handle (csrc/ph_state.h ph_data), by the same names
struct ph_data {
    int64_t S;
    int n, m, nn;
    const int32_t *row_ptr, *col_idx, *col_ptr, *row_idx, *perm, *nonant_slot, *nonant_col;
    const double *A, *c, *q, *lb, *ub, *rl, *ru, *prob, *objc;
};
#include "ph_lshaped.inc"
#include "ph_ef.inc"

// Arrays are scenario-fastest ([k][S]); A in CSR order.  out_first [ntri + nn]: the first scenario
// pass's sums of T' N^-1 T and T' N^-1 g.  info [8]: the last test's record.  Returns the status.
extern "C" int ef_host_solve(int64_t S, int n, int m, int nnz, int nn, const int32_t* row_ptr, const int32_t* col_idx,
                             const int32_t* nonant_col, const double* A, const double* c, const double* q,
                             const double* lb, const double* ub, const double* rl, const double* ru, const double* prob,
                             const double* zlb, const double* zub, const double* cz, const double* qz, double ncomp,
                             double cmax, double tol, int qp, int max_iter, double* x, double* y, double* z,
                             double* out_first, double* info) {
    std::vector<int32_t> col_ptr(n + 1, 0), row_idx(nnz), perm(nnz), slot(n, -1);
    for (int k = 0; k < nnz; ++k) col_ptr[col_idx[k] + 1]++;
    for (int j = 0; j < n; ++j) col_ptr[j + 1] += col_ptr[j];
    {
        std::vector<int32_t> fill(col_ptr.begin(), col_ptr.end() - 1);
        for (int i = 0; i < m; ++i)
            for (int k = row_ptr[i]; k < row_ptr[i + 1]; ++k) {
                const int pos = fill[col_idx[k]]++;
                row_idx[pos] = i;
                perm[pos] = k;
            }
    }
    for (int k = 0; k < nn; ++k) slot[nonant_col[k]] = k;
    ph_data st;
    memset(&st, 0, sizeof(st));
    st.S = S; st.n = n; st.m = m; st.nn = nn;
    st.row_ptr = row_ptr; st.col_idx = col_idx; st.col_ptr = col_ptr.data(); st.row_idx = row_idx.data();
    st.perm = perm.data(); st.nonant_slot = slot.data(); st.nonant_col = nonant_col;
    st.A = A; st.c = c; st.q = q; st.lb = lb; st.ub = ub; st.rl = rl; st.ru = ru; st.prob = prob; st.objc = nullptr;
    ef_store E;
    memset(&E, 0, sizeof(E));
    E.nn = nn; E.m = m; E.n = n; E.ntri = nn * (nn + 1) / 2; E.ld = nn | 1;
    const int nsum0 = E.ntri + 2 * nn + 2;
    E.nplanes = nsum0 + 2;
    std::vector<double*> bufs;
    auto mk = [&](size_t cnt) {
        double* p = (double*)calloc(cnt ? cnt : 1, sizeof(double));
        bufs.push_back(p);
        return p;
    };
    for (double** p : {&E.x, &E.zl, &E.zu, &E.dx, &E.dxa, &E.D}) *p = mk((size_t)n * S);
    for (double** p : {&E.w, &E.vl, &E.vu, &E.y, &E.dw, &E.dwa, &E.dy, &E.dya, &E.g, &E.wk, &E.rp, &E.E}) *p = mk((size_t)m * S);
    E.fac = mk((size_t)(m * (m + 1) / 2) * S);
    E.terms = mk((size_t)E.nplanes * S);
    E.C = mk((size_t)nn * E.ld);
    E.ctl = mk(EF_CTL);
    E.zd = mk((size_t)(EZ_N + 1) * nn);
    for (int k = 0; k < nn; ++k) {
        EF_Z(E, EZ_LB)[k] = zlb[k]; EF_Z(E, EZ_UB)[k] = zub[k]; EF_Z(E, EZ_C)[k] = cz[k]; EF_Z(E, EZ_Q)[k] = qz[k];
        EF_Z(E, EZ_Z)[k] = ef_inside(zlb[k], zub[k]);
        EF_Z(E, EZ_ZL)[k] = isfinite(zlb[k]) ? 1.0 + fabs(cz[k]) : 0.0;
        EF_Z(E, EZ_ZU)[k] = isfinite(zub[k]) ? 1.0 + fabs(cz[k]) : 0.0;
    }
    E.ctl[EC_NCOMP] = ncomp; E.ctl[EC_CMAX] = cmax; E.ctl[EC_TOL] = tol; E.ctl[EC_QP] = qp ? 1.0 : 0.0;
    double* rsum = mk(nsum0);
    double* rmax = mk(2);
    double* M = mk((size_t)nn * E.ld + nn);
    auto reduce = [&](int nsum, int nmax) {
        for (int b = 0; b < nsum + nmax; ++b) {
            double acc = 0.0;
            for (int64_t s = 0; s < S; ++s) acc = b < nsum ? acc + E.terms[IX(b)] : fmax(acc, E.terms[IX(b)]);
            (b < nsum ? rsum[b] : rmax[b - nsum]) = acc;
        }
    };
    for (int64_t s = 0; s < S; ++s) ef_start_lane(st, E, s);
    int done = 0;
    for (int it = 0; it <= max_iter; ++it) {
        for (int stage = 0; stage < 2; ++stage) {
            for (int64_t s = 0; s < S; ++s) ef_schur_lane(st, E, s, stage);
            reduce(stage == 0 ? nsum0 : nn, stage == 0 ? 2 : 0);
            if (it == 0 && stage == 0 && out_first)
                for (int k = 0; k < E.ntri + nn; ++k) out_first[k] = rsum[k];
            ef_solve_core(E, stage, rsum, rmax, info, M, &done);
            if (it == max_iter) break;  // (the last trip only tests the iterate)
            for (int64_t s = 0; s < S; ++s) ef_direction_lane(st, E, s, stage);
            reduce(3, 2);
            ef_ctrl_core(E, stage, rsum, rmax);
            for (int64_t s = 0; s < S; ++s) stage == 0 ? ef_keep_lane(st, E, s) : ef_step_lane(st, E, s);
        }
        if (E.ctl[EC_DONE] != 0.0 || !(info[1] == info[1])) break;
    }
    std::vector<double> obj(S), bound(S);
    std::vector<int32_t> status(S), iters(S);
    for (int64_t s = 0; s < S; ++s) ef_export_lane(st, E, s, x, y, obj.data(), bound.data(), status.data(), iters.data());
    for (int k = 0; k < nn; ++k) z[k] = EF_Z(E, EZ_Z)[k];
    const int rc = status[0];
    for (double* p : bufs) free(p);
    return rc;
}

#ifdef EF_HOST_MAIN
#include <stdio.h>
// two scenarios, one nonant z in [0, 10], per scenario one other column x >= 0:
//   min sum_s p_s (z + 3 x_s)   s.t.  z + x_s >= d_s (d = 2, 6),  z - x_s <= 8 (ranged -inf..8)
// optimum z = 6 (cost 1 per unit of z against 3 p_s of each shortfall), x = 0: objective 6
int main() {
    const int64_t S = 2;
    const int n = 2, m = 2, nnz = 4, nn = 1;
    int32_t row_ptr[] = {0, 2, 4}, col_idx[] = {0, 1, 0, 1}, nonant_col[] = {0};
    double A[nnz * S] = {1, 1, 1, 1, 1, 1, -1, -1};
    double c[n * S] = {1, 1, 3, 3}, q[n * S] = {0, 0, 0, 0}, lb[n * S] = {0, 0, 0, 0}, ub[n * S] = {10, 10, INFINITY, INFINITY};
    double rl[m * S] = {2, 6, -INFINITY, -INFINITY}, ru[m * S] = {INFINITY, INFINITY, 8, 8}, prob[S] = {0.5, 0.5};
    double zlb[] = {0}, zub[] = {10}, cz[] = {1}, qz[] = {0};
    double x[n * S], y[m * S], z[nn], first[2], info[8];
    // finite bounds: x_s lower (2), row sides (4), z (2)
    const int st = ef_host_solve(S, n, m, nnz, nn, row_ptr, col_idx, nonant_col, A, c, q, lb, ub, rl, ru, prob, zlb, zub, cz, qz,
                                 8.0, 3.0, 1e-9, 0, 60, x, y, z, first, info);
    printf("status %d iterations %.0f z %.9f objective %.9f\n", st, info[0], z[0], info[5]);
    return (st == 0 && fabs(z[0] - 6.0) < 1e-6 && fabs(info[5] - 6.0) < 1e-6) ? 0 : 1;
}
#endif
