// The segmented extensive-form interior point (bundles) on the host: the lane
// functions, the cores and the segment helpers of csrc/ph_ef.inc compiled for one thread (EF_HOST,
// LS_HOST) and driven over several segments in the library's order, with plain-loop segmented
// sums, behind a C entry that tests/test_bundles.py loads with ctypes and compares with the numpy
// restatement (tests/ef_ref.py) bundle by bundle.  Buffers are heap blocks of the exact size, so
// the same file, built as a stand-alone program with a sanitizer, sees every overrun
// (BUNDLE_HOST_MAIN).
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

// Arrays are scenario-fastest ([k][S]); A in CSR order.  c, q: the solve's cost and diagonal (the
// PH terms on the nonant columns included); prob: p_s / p_B.  Per segment g: zlb, zub [G][nn],
// ncomp, cmax [G]; tol, ztol: the segments' test (ef_seg_test); out: z [G][nn], first [G][ntri + nn]
// (the first scenario pass's sums of T' N^-1 T and T' N^-1 g), objective, iterations, status [G].
// Returns the segments not OPTIMAL.
extern "C" int bundle_host_solve(int64_t S, int n, int m, int nnz, int nn, const int32_t* row_ptr, const int32_t* col_idx,
                                 const int32_t* nonant_col, const double* A, const double* c, const double* q,
                                 const double* lb, const double* ub, const double* rl, const double* ru, const double* prob,
                                 int G, const int32_t* seg_start, const double* zlb, const double* zub, const double* ncomp,
                                 const double* cmax, double tol, double ztol, int qp, int max_iter, double* x, double* y, double* z,
                                 double* out_first, double* out_obj, int32_t* out_iters, int32_t* out_status) {
    std::vector<int32_t> col_ptr(n + 1, 0), row_idx(nnz), perm(nnz), slot(n, -1), seg_of(S);
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
    for (int g = 0; g < G; ++g)
        for (int32_t s = seg_start[g]; s < seg_start[g + 1]; ++s) seg_of[s] = g;
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
    // segment-major: G copies of C, ctl and the zd block
    E.C = mk((size_t)G * nn * E.ld);
    E.ctl = mk((size_t)G * EF_CTL);
    E.zd = mk((size_t)G * EF_ZD_LEN(E));
    double* rsum = mk((size_t)G * nsum0);
    double* rmax = mk((size_t)G * 2);
    double* info = mk((size_t)G * 8);
    double* M = mk((size_t)nn * E.ld + nn);
    for (int g = 0; g < G; ++g) {
        const ef_store V = ef_seg_view(E, g);
        for (int k = 0; k < nn; ++k) {
            EF_Z(V, EZ_LB)[k] = zlb[(size_t)g * nn + k];
            EF_Z(V, EZ_UB)[k] = zub[(size_t)g * nn + k];
        }
        V.ctl[EC_NCOMP] = ncomp[g]; V.ctl[EC_CMAX] = cmax[g];
        V.ctl[EC_TOL] = -1.0;  // (the core's own test is off: ef_seg_test decides)
        V.ctl[EC_SEG_TOL] = tol; V.ctl[EC_SEG_ZTOL] = ztol;
    }
    // the segmented reduction: per (plane, segment) the segment's scenarios in index order
    auto reduce = [&](int nsum, int nmax) {
        for (int g = 0; g < G; ++g) {
            if (E.ctl[(size_t)g * EF_CTL + EC_DONE] != 0.0) continue;
            for (int b = 0; b < nsum + nmax; ++b) {
                double acc = 0.0;
                for (int64_t s = seg_start[g]; s < seg_start[g + 1]; ++s)
                    acc = b < nsum ? acc + E.terms[IX(b)] : fmax(acc, E.terms[IX(b)]);
                (b < nsum ? rsum[(size_t)g * nsum0 + b] : rmax[(size_t)g * 2 + b - nsum]) = acc;
            }
        }
    };
    auto view = [&](int64_t s) { return ef_seg_view(E, seg_of[s]); };
    // the start (phgpu_bundle_start)
    for (int64_t s = 0; s < S; ++s) ef_start_lane(st, view(s), s);
    for (int g = 0; g < G; ++g) ef_seg_start(st, ef_seg_view(E, g), seg_start[g], seg_start[g + 1], qp != 0);
    int done = 0;
    for (int it = 0; it <= max_iter; ++it) {
        for (int stage = 0; stage < 2; ++stage) {
            for (int64_t s = 0; s < S; ++s) ef_schur_lane(st, view(s), s, stage);
            reduce(stage == 0 ? nsum0 : nn, stage == 0 ? 2 : 0);
            if (it == 0 && stage == 0 && out_first)
                for (int g = 0; g < G; ++g)
                    for (int k = 0; k < E.ntri + nn; ++k) out_first[(size_t)g * (E.ntri + nn) + k] = rsum[(size_t)g * nsum0 + k];
            for (int g = 0; g < G; ++g) {
                const ef_store V = ef_seg_view(E, g);
                ef_solve_core(V, stage, rsum + (size_t)g * nsum0, rmax + (size_t)g * 2, info + (size_t)g * 8, M, &done);
                ef_seg_refine(V, M);
                if (stage == 0) ef_seg_test(V);
            }
            if (it == max_iter) break;  // (the last trip only tests the iterates)
            for (int64_t s = 0; s < S; ++s) ef_direction_lane(st, view(s), s, stage);
            reduce(3, 2);
            for (int g = 0; g < G; ++g) ef_seg_ctrl(ef_seg_view(E, g), stage, rsum + (size_t)g * nsum0, rmax + (size_t)g * 2);
            for (int64_t s = 0; s < S; ++s) stage == 0 ? ef_keep_lane(st, view(s), s) : ef_step_lane(st, view(s), s);
        }
        int open = 0;
        for (int g = 0; g < G; ++g) open += E.ctl[(size_t)g * EF_CTL + EC_DONE] == 0.0;
        if (!open) break;
    }
    std::vector<double> obj(S), bound(S);
    std::vector<int32_t> status(S), iters(S);
    for (int64_t s = 0; s < S; ++s) ef_export_lane(st, view(s), s, x, y, obj.data(), bound.data(), status.data(), iters.data());
    int bad = 0;
    for (int g = 0; g < G; ++g) {
        const ef_store V = ef_seg_view(E, g);
        for (int k = 0; k < nn; ++k) z[(size_t)g * nn + k] = EF_Z(V, EZ_Z)[k];
        out_obj[g] = V.ctl[EC_OBJ];
        out_iters[g] = iters[seg_start[g]];
        out_status[g] = status[seg_start[g]];
        bad += status[seg_start[g]] != 0;
    }
    for (double* p : bufs) free(p);
    return bad;
}

#ifdef BUNDLE_HOST_MAIN
#include <stdio.h>
// Five scenarios in two segments (3 + 2), one nonant z in [0, 10], per scenario one other column
// x >= 0:  min sum_s p_s (z + 3 x_s)  s.t.  z + x_s >= d_s,  z - x_s <= 8  per segment, p_s = 1 / |B|.
// A unit of z costs 1 and saves 3 p_s for each scenario whose demand is still above z: with
// d = (2, 6, 6 | 1, 4) that is 2 per unit up to z = 6 in the first segment and 1.5 up to z = 4 in the
// second, so z = 6 and z = 4, x = 0, objectives 6 and 4.
int main() {
    const int64_t S = 5;
    const int n = 2, m = 2, nnz = 4, nn = 1, G = 2;
    int32_t row_ptr[] = {0, 2, 4}, col_idx[] = {0, 1, 0, 1}, nonant_col[] = {0}, seg_start[] = {0, 3, 5};
    double A[nnz * S], c[n * S], q[n * S], lb[n * S], ub[n * S], rl[m * S], ru[m * S];
    const double d[S] = {2, 6, 6, 1, 4}, prob[S] = {1.0 / 3, 1.0 / 3, 1.0 / 3, 0.5, 0.5};
    for (int64_t s = 0; s < S; ++s) {
        A[0 * S + s] = 1; A[1 * S + s] = 1; A[2 * S + s] = 1; A[3 * S + s] = -1;
        c[0 * S + s] = 1; c[1 * S + s] = 3; q[0 * S + s] = q[1 * S + s] = 0;
        lb[0 * S + s] = lb[1 * S + s] = 0; ub[0 * S + s] = 10; ub[1 * S + s] = INFINITY;
        rl[0 * S + s] = d[s]; ru[0 * S + s] = INFINITY; rl[1 * S + s] = -INFINITY; ru[1 * S + s] = 8;
    }
    double zlb[G] = {0, 0}, zub[G] = {10, 10}, ncomp[G] = {3 + 6 + 2, 2 + 4 + 2}, cmax[G] = {3, 3};
    double x[n * S], y[m * S], z[G * nn], first[G * 2], obj[G];
    int32_t iters[G], status[G];
    const int bad = bundle_host_solve(S, n, m, nnz, nn, row_ptr, col_idx, nonant_col, A, c, q, lb, ub, rl, ru, prob, G, seg_start,
                                      zlb, zub, ncomp, cmax, 1e-9, 1e-8, 0, 60, x, y, z, first, obj, iters, status);
    printf("not optimal %d; z %.9f %.9f objectives %.9f %.9f iterations %d %d\n", bad, z[0], z[1], obj[0], obj[1], iters[0],
           iters[1]);
    return (bad == 0 && fabs(z[0] - 6.0) < 1e-6 && fabs(z[1] - 4.0) < 1e-6 && fabs(obj[0] - 6.0) < 1e-6 &&
            fabs(obj[1] - 4.0) < 1e-6)
               ? 0
               : 1;
}
#endif
