// The CONDITIONED multistage extensive form on the host (phgpu_eft_fix): z entries
// held at values.  tests/ef_tree_host.cpp's driver with the held entries set as phgpu_eft_fix sets
// them (the empty box, the value, no duals, their bounds out of ncomp), behind two C entries that
// tests/test_ef_cond.py loads with ctypes: the elimination and back-substitution alone on given
// systems with tree sparsity and held entries (through eft_elim_core, so the node's own z side is
// the kernels'), and the whole interior point.  Buffers are heap blocks of the exact size, so the
// same file, built as a stand-alone program with a sanitizer, sees every overrun (EF_COND_HOST_MAIN).
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
#include "ph_ef_tree.inc"

namespace {
// the tree as phgpu_eft_init lays it out, with every buffer of eft_tree on the heap
struct host_tree {
    eft_tree T;
    std::vector<int32_t> depth, child0, nchild, zoff, path, P, lvl0;
    std::vector<double*> bufs;
    double* mk(size_t cnt) {
        double* p = (double*)calloc(cnt ? cnt : 1, sizeof(double));
        bufs.push_back(p);
        return p;
    }
    ~host_tree() {
        for (double* p : bufs) free(p);
    }
    void build(int D, const int32_t* nlens, int Nn, const int32_t* nd, const int32_t* np, int nn) {
        memset(&T, 0, sizeof(T));
        P.assign(D, 0);
        for (int d = 0, a = 0; d < D; ++d) P[d] = (a += nlens[d]);
        depth.assign(nd, nd + Nn);
        child0.assign(Nn, 0);
        nchild.assign(Nn, 0);
        zoff.assign(Nn, 0);
        path.assign((size_t)Nn * nn, 0);
        lvl0.assign(D + 1, Nn);
        lvl0[0] = 0;
        int Ztot = P[0];
        for (int k = 0; k < P[0]; ++k) path[k] = k;
        for (int i = 1; i < Nn; ++i) {
            const int d = nd[i], p = np[i];
            if (nd[i - 1] != d) lvl0[d] = i;
            if (nchild[p] == 0) child0[p] = i;
            ++nchild[p];
            zoff[i] = Ztot;
            for (int k = 0; k < P[d - 1]; ++k) path[(size_t)i * nn + k] = path[(size_t)p * nn + k];
            for (int k = P[d - 1]; k < P[d]; ++k) path[(size_t)i * nn + k] = Ztot + (k - P[d - 1]);
            Ztot += nlens[d];
        }
        T.D = D; T.Nn = Nn; T.nn = nn; T.ld = nn | 1; T.Ztot = Ztot; T.P0 = P[0]; T.deep0 = lvl0[D - 1]; T.G = Nn - T.deep0;
        T.nsum0 = nn * (nn + 1) / 2 + 2 * nn + 2;
        T.depth = depth.data(); T.child0 = child0.data(); T.nchild = nchild.data(); T.zoff = zoff.data();
        T.path = path.data(); T.P = P.data();
        T.zn = mk((size_t)(EZ_N + 1) * Ztot);
        T.rootzd = mk((size_t)(EZ_N + 1) * P[0]);
        T.slot = mk((size_t)Nn * nn * T.ld);
        T.hv = mk((size_t)Nn * nn);
        T.ty = mk((size_t)Nn * nn);
        T.nsc = mk((size_t)Nn * 2);
        T.segsum = mk((size_t)T.G * T.nsum0);
        T.segmax = mk((size_t)T.G * 2);
        T.rootsum = mk((size_t)(P[0] * (P[0] + 1) / 2 + 2 * P[0] + 2));
        T.rootmax = mk(2);
        T.lsum = mk(3); T.lmax = mk(2); T.dirsum = mk(3); T.dirmax = mk(2);
    }
};
}  // namespace

// The elimination alone.  segA [G][nn * nn] (lower triangles, path order) and segb [G][nn]: what the
// deepest nodes' scenarios sum to; dd, rr [Ztot]: what every free z entry adds to its diagonal and its
// right-hand side (given to eft_node_zside as qz = dd, cz = -rr at z = 0 with no bounds); held [Ztot]:
// non-zero where the entry is held.  Out: nodeA [Nn][nn * nn], nodeb [Nn][nn] the per-node sums, dz
// [Ztot] the solution.  ROOT goes through the node functions too (its path is its own entries).
extern "C" int eft_cond_host_linear(int D, const int32_t* nlens, int Nn, const int32_t* node_depth, const int32_t* node_parent,
                                    const double* segA, const double* segb, const double* dd, const double* rr,
                                    const int32_t* held, double* nodeA, double* nodeb, double* dz) {
    int nn = 0;
    for (int d = 0; d < D; ++d) nn += nlens[d];
    host_tree H;
    H.build(D, nlens, Nn, node_depth, node_parent, nn);
    eft_tree& T = H.T;
    const int ntri = nn * (nn + 1) / 2;
    for (int g = 0; g < T.G; ++g) {
        double* r = T.segsum + (size_t)g * T.nsum0;
        for (int i = 0; i < nn; ++i) {
            for (int j = 0; j <= i; ++j) r[EF_TRI(i, j)] = segA[((size_t)g * nn + i) * nn + j];
            r[ntri + i] = segb[(size_t)g * nn + i];
        }
    }
    for (int k = 0; k < T.Ztot; ++k) {
        *eft_zp(T, EZ_LB, k) = held[k] ? INFINITY : -INFINITY;
        *eft_zp(T, EZ_UB, k) = held[k] ? -INFINITY : INFINITY;
        *eft_zp(T, EZ_C, k) = -rr[k];
        *eft_zp(T, EZ_Q, k) = dd[k];
        *eft_zp(T, EZ_DZ, k) = 7.0;  // (a held entry's has to be overwritten with 0)
    }
    T.inspA = nodeA;
    T.inspb = nodeb;
    double* W = H.mk((size_t)nn * T.ld + 2 * (size_t)nn);
    double* ctl = H.mk(EF_CTL);
    for (int d = D - 1; d >= 0; --d)
        for (int n = H.lvl0[d]; n < H.lvl0[d + 1]; ++n) eft_elim_core(T, ctl, n, 0, W);
    for (int d = 0; d < D; ++d)
        for (int n = H.lvl0[d]; n < H.lvl0[d + 1]; ++n) eft_node_back(T, n);
    for (int k = 0; k < T.Ztot; ++k) dz[k] = *eft_zp(T, EZ_DZ, k);
    return 0;
}

// The whole solve.  Arrays are scenario-fastest ([k][S]); A in CSR order; seg_start [G + 1]; zlb,
// zub, cz, qz [Ztot].  nodeA, nodeb: the first pass's per-node sums (ROOT's from its own sums).
// info [8]: the last test's record.  z [Ztot].  zfix [Ztot]: NaN = free, else the value the entry is
// held at (phgpu_eft_fix).  held_dz [1]: the largest |dz| of a held entry over every right-hand side
// of every iteration (0.0 exactly, or the elimination moved it).  Returns the status.
extern "C" int eft_cond_host_solve(int64_t S, int n, int m, int nnz, int nn, const int32_t* row_ptr, const int32_t* col_idx,
                              const int32_t* nonant_col, const double* A, const double* c, const double* q, const double* lb,
                              const double* ub, const double* rl, const double* ru, const double* prob, int D,
                              const int32_t* nlens, int Nn, const int32_t* node_depth, const int32_t* node_parent,
                              const int32_t* seg_start, const double* zlb, const double* zub, const double* cz,
                              const double* qz, double ncomp, double cmax, double tol, int qp, int max_iter, double* x,
                              double* y, double* z, double* nodeA, double* nodeb, double* info, const double* zfix, double* held_dz) {
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
    host_tree H;
    H.build(D, nlens, Nn, node_depth, node_parent, nn);
    eft_tree& T = H.T;
    const int G = T.G, P0 = T.P0, Ztot = T.Ztot;
    std::vector<int32_t> seg_of(S);
    for (int g = 0; g < G; ++g)
        for (int32_t s = seg_start[g]; s < seg_start[g + 1]; ++s) seg_of[s] = g;
    T.seg_start = seg_start;
    T.seg_of = seg_of.data();
    ef_store E;
    memset(&E, 0, sizeof(E));
    E.nn = nn; E.m = m; E.n = n; E.ntri = nn * (nn + 1) / 2; E.ld = nn | 1;
    E.nplanes = T.nsum0 + 2;
    auto mk = [&](size_t cnt) { return H.mk(cnt); };
    for (double** p : {&E.x, &E.zl, &E.zu, &E.dx, &E.dxa, &E.D}) *p = mk((size_t)n * S);
    for (double** p : {&E.w, &E.vl, &E.vu, &E.y, &E.dw, &E.dwa, &E.dy, &E.dya, &E.g, &E.wk, &E.rp, &E.E}) *p = mk((size_t)m * S);
    E.fac = mk((size_t)(m * (m + 1) / 2) * S);
    E.terms = mk((size_t)E.nplanes * S);
    E.C = mk((size_t)P0 * (P0 | 1));
    E.ctl = mk(EF_CTL);
    E.zd = mk((size_t)G * EF_ZD_LEN(E));
    for (int k = 0; k < Ztot; ++k) {
        *eft_zp(T, EZ_LB, k) = zlb[k]; *eft_zp(T, EZ_UB, k) = zub[k]; *eft_zp(T, EZ_C, k) = cz[k]; *eft_zp(T, EZ_Q, k) = qz[k];
        *eft_zp(T, EZ_Z, k) = ef_inside(zlb[k], zub[k]);
        *eft_zp(T, EZ_ZL, k) = isfinite(zlb[k]) ? 1.0 + fabs(cz[k]) : 0.0;
        *eft_zp(T, EZ_ZU, k) = isfinite(zub[k]) ? 1.0 + fabs(cz[k]) : 0.0;
    }
    for (int k = 0; k < Ztot; ++k) {  // phgpu_eft_fix
        if (zfix[k] != zfix[k]) continue;
        ncomp -= (isfinite(zlb[k]) ? 1.0 : 0.0) + (isfinite(zub[k]) ? 1.0 : 0.0);
        *eft_zp(T, EZ_LB, k) = INFINITY; *eft_zp(T, EZ_UB, k) = -INFINITY;
        *eft_zp(T, EZ_Z, k) = zfix[k];
        *eft_zp(T, EZ_ZL, k) = *eft_zp(T, EZ_ZU, k) = 0.0;
    }
    ncomp = fmax(1.0, ncomp);
    *held_dz = 0.0;
    E.ctl[EC_NCOMP] = ncomp; E.ctl[EC_CMAX] = cmax; E.ctl[EC_TOL] = tol; E.ctl[EC_QP] = qp ? 1.0 : 0.0;
    const ef_store R = eft_root_view(E, T);
    double* W = mk((size_t)nn * T.ld + 2 * (size_t)nn);
    double* M0 = mk((size_t)P0 * R.ld + P0);
    auto gather = [&](int f) {  // k_eft_gather
        for (int g = 0; g < G; ++g)
            for (int k = 0; k < nn; ++k)
                E.zd[(size_t)g * EF_ZD_LEN(E) + (size_t)f * nn + k] = *eft_zp(T, f, T.path[(size_t)(T.deep0 + g) * nn + k]);
    };
    auto reduce = [&](int nsum, int nmax) {  // k_eft_reduce_t
        if (E.ctl[EC_DONE] != 0.0) return;
        for (int b = 0; b < nsum + nmax; ++b)
            for (int g = 0; g < G; ++g) {
                double acc = 0.0;
                for (int64_t s = seg_start[g]; s < seg_start[g + 1]; ++s) acc = b < nsum ? acc + E.terms[IX(b)] : fmax(acc, E.terms[IX(b)]);
                if (b < nsum) T.segsum[(size_t)g * T.nsum0 + b] = acc;
                else T.segmax[(size_t)g * 2 + (b - nsum)] = acc;
            }
    };
    auto root = [&](int stage) {  // k_eft_root
        if (E.ctl[EC_DONE] != 0.0) return;
        const int ntri0 = R.ntri, ntri = E.ntri;
        if (stage == 1) {
            for (int k = 0; k < P0; ++k) T.rootsum[k] = eft_gather(T, 0, 1, 1, k, 0);
            return;
        }
        for (int i = 0; i < P0; ++i)
            for (int j = 0; j <= i; ++j) {
                T.rootsum[EF_TRI(i, j)] = eft_gather(T, 0, 0, 0, i, j);
                if (T.inspA) T.inspA[(size_t)i * nn + j] = T.rootsum[EF_TRI(i, j)];
            }
        for (int k = 0; k < P0; ++k) {
            T.rootsum[ntri0 + k] = eft_gather(T, 0, 0, 1, k, 0);
            if (T.inspb) T.inspb[k] = T.rootsum[ntri0 + k];
            T.rootsum[ntri0 + P0 + k] = eft_gather(T, 0, 0, 2, k, 0);
        }
        double comp = 0.0, obj = 0.0, mx[2] = {0.0, 0.0};
        for (int g = 0; g < G; ++g) {
            comp += T.segsum[(size_t)g * T.nsum0 + ntri + 2 * nn];
            obj += T.segsum[(size_t)g * T.nsum0 + ntri + 2 * nn + 1];
            mx[0] = fmax(mx[0], T.segmax[(size_t)g * 2]);
            mx[1] = fmax(mx[1], T.segmax[(size_t)g * 2 + 1]);
        }
        for (int i = 1; i < Nn; ++i) {
            comp += T.nsc[(size_t)i * 2];
            mx[1] = fmax(mx[1], T.nsc[(size_t)i * 2 + 1]);
        }
        T.rootsum[ntri0 + 2 * P0] = comp;
        T.rootsum[ntri0 + 2 * P0 + 1] = obj;
        T.rootmax[0] = mx[0];
        T.rootmax[1] = mx[1];
    };
    for (int64_t s = 0; s < S; ++s) ef_start_lane(st, E, s);
    gather(EZ_Z);
    int done = 0;
    for (int it = 0; it <= max_iter; ++it) {
        for (int stage = 0; stage < 2; ++stage) {
            T.inspA = (it == 0 && stage == 0) ? nodeA : nullptr;
            T.inspb = (it == 0 && stage == 0) ? nodeb : nullptr;
            for (int64_t s = 0; s < S; ++s) ef_schur_lane(st, eft_seg_view(E, seg_of[s]), s, stage);
            reduce(stage == 0 ? T.nsum0 : nn, stage == 0 ? 2 : 0);
            for (int d = D - 1; d >= 1; --d)
                for (int i = H.lvl0[d]; i < H.lvl0[d + 1]; ++i) eft_elim_core(T, E.ctl, i, stage, W);
            root(stage);
            ef_solve_core(R, stage, T.rootsum, T.rootmax, info, M0, &done);
            if (it == max_iter) break;  // (the last trip only tests the iterate)
            if (E.ctl[EC_DONE] == 0.0)
                for (int d = 1; d < D; ++d)
                    for (int i = H.lvl0[d]; i < H.lvl0[d + 1]; ++i) eft_node_back(T, i);
            if (E.ctl[EC_DONE] == 0.0)
                for (int k = 0; k < Ztot; ++k)
                    if (zfix[k] == zfix[k]) *held_dz = fmax(*held_dz, fabs(*eft_zp(T, EZ_DZ, k)));
            gather(EZ_DZ);
            for (int64_t s = 0; s < S; ++s) ef_direction_lane(st, eft_seg_view(E, seg_of[s]), s, stage);
            if (E.ctl[EC_DONE] == 0.0) {  // k_ef_reduce, k_eft_dirsum
                double rp = 0.0, rd = 0.0, ct[3] = {0.0, 0.0, 0.0};
                for (int zi = P0; zi < Ztot; ++zi) eft_z_ratios(T, E.ctl, stage, zi, rp, rd, ct);
                for (int b = 0; b < 5; ++b) {
                    double acc = 0.0;
                    for (int64_t s = 0; s < S; ++s) acc = b < 3 ? acc + E.terms[IX(b)] : fmax(acc, E.terms[IX(b)]);
                    if (b < 3) T.dirsum[b] = acc + ct[b];
                    else T.dirmax[b - 3] = fmax(acc, b == 3 ? rp : rd);
                }
            }
            ef_ctrl_core(R, stage, T.dirsum, T.dirmax);
            for (int zi = P0; zi < Ztot; ++zi) eft_z_step(T, E.ctl, stage, zi);
            for (int64_t s = 0; s < S; ++s) stage == 0 ? ef_keep_lane(st, E, s) : ef_step_lane(st, E, s);
            if (stage == 1) gather(EZ_Z);
        }
        if (E.ctl[EC_DONE] != 0.0 || !(info[1] == info[1])) break;
    }
    std::vector<double> obj(S), bound(S);
    std::vector<int32_t> status(S), iters(S);
    for (int64_t s = 0; s < S; ++s)
        ef_export_lane(st, eft_seg_view(E, seg_of[s]), s, x, y, obj.data(), bound.data(), status.data(), iters.data());
    for (int k = 0; k < Ztot; ++k) z[k] = *eft_zp(T, EZ_Z, k);
    return status[0];
}

#ifdef EF_COND_HOST_MAIN
#include <stdio.h>
// tests/ef_tree_host.cpp's program with z0 held at 4: four scenarios on a 2,2 tree; one nonant per
// non-leaf node (z0 at ROOT, z1 at the two nodes of depth 1), per scenario one other column x >= 0:
//   min sum_s p_s (z0 + 2 z1 + 5 x_s)   s.t.  z0 + z1 + x_s >= d_s,  z0 - z1 <= 8,  z in [0, 10];  d = (2, 4, 6, 9)
// With z0 = 4 node 1 (d = 2, 4) needs nothing more: z1 = 0.  Node 2 (d = 6, 9) pays 2 z1 p in both
// scenarios and 5 p per unit still short: z1 = 2 covers d = 6 and leaves x = 3 at d = 9 (node cost
// 0.5 * 2 * 2 + 0.25 * 15 = 5.75), every further unit of z1 costs 1 and saves 1.25, so z1 = 5 (node
// cost 5).  Objective 4 + 0 + 5 = 9.
int main() {
    const int64_t S = 4;
    const int n = 3, m = 2, nnz = 5, nn = 2, D = 2, Nn = 3;
    int32_t row_ptr[] = {0, 3, 5}, col_idx[] = {0, 1, 2, 0, 1}, nonant_col[] = {0, 1};
    int32_t nlens[] = {1, 1}, nd[] = {0, 1, 1}, np[] = {-1, 0, 0}, seg_start[] = {0, 2, 4};
    double A[nnz * S], c[n * S], q[n * S], lb[n * S], ub[n * S], rl[m * S], ru[m * S], prob[S];
    const double a0[nnz] = {1, 1, 1, 1, -1}, c0[n] = {1, 2, 5}, u0[n] = {10, 10, INFINITY}, d0[S] = {2, 4, 6, 9};
    for (int64_t s = 0; s < S; ++s) {
        for (int k = 0; k < nnz; ++k) A[IX(k)] = a0[k];
        for (int j = 0; j < n; ++j) {
            c[IX(j)] = c0[j]; q[IX(j)] = 0.0; lb[IX(j)] = 0.0; ub[IX(j)] = u0[j];
        }
        rl[IX(0)] = d0[s]; ru[IX(0)] = INFINITY;
        rl[IX(1)] = -INFINITY; ru[IX(1)] = 8.0;
        prob[s] = 0.25;
    }
    double zlb[] = {0, 0, 0}, zub[] = {10, 10, 10}, cz[] = {1, 1, 1}, qz[] = {0, 0, 0}, zfix[] = {4.0, NAN, NAN};
    double x[n * S], y[m * S], z[3], nodeA[Nn * nn * nn], nodeb[Nn * nn], info[8], held_dz = -1.0;
    const int st = eft_cond_host_solve(S, n, m, nnz, nn, row_ptr, col_idx, nonant_col, A, c, q, lb, ub, rl, ru, prob, D, nlens, Nn,
                                       nd, np, seg_start, zlb, zub, cz, qz, 18.0, 5.0, 1e-9, 0, 60, x, y, z, nodeA, nodeb, info,
                                       zfix, &held_dz);
    printf("status %d iterations %.0f z %.6f %.6f %.6f objective %.9f held dz %g\n", st, info[0], z[0], z[1], z[2], info[5],
           held_dz);
    return (st == 0 && fabs(info[5] - 9.0) < 1e-6 && z[0] == 4.0 && held_dz == 0.0) ? 0 : 1;
}
#endif
