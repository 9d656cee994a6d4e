// The extensive form of a multistage problem (mpisppy/opt/ef.py with all_nodenames; phgpu_eft_*,
// include/phgpu.h; DESIGN.md 3.23).  Included by phgpu.hip after ph_ef.inc, whose lane functions
// run here unchanged: a scenario's "linking variables" are the nn nonants of its whole path.
//
// z is the concatenation over the non-leaf nodes of nlens[depth] values each (Ztot in all), the
// nodes numbered depth by depth with siblings adjacent.  The Newton system in dz has a block
// (n, a) only where a is n or an ancestor of n; it is eliminated bottom-up.  With P_d = nlens[0] +
// ... + nlens[d], a node n of depth d holds a P_d x P_d matrix A_n over its path: at the deepest
// level the sum of T' N^-1 T over its scenarios (a contiguous segment, as in 3.22), above that the
// sum of its children's Schur complements.  Its own nl = nlens[d] variables are eliminated:
//
//   A_n = [A11 A21'; A21 A22],  A22 + Dz^-1 = L L',  K = L^-1 A21,  G_n = A11 - K'K,
//   v = L^-1 b2,  h_n = b1 - K'v;    back:  dz_n = L^-T (v - K dz_ancestors)
//
// In a node's workspace its own variables come FIRST (position i < nl is path entry P_{d-1} + i,
// position nl + a is the ancestors' path entry a): a right-looking Cholesky that stops after nl
// columns then leaves L and K' in those columns, G_n in the trailing block and (v | h_n) in the
// right-hand side.  The whole workspace is the node's slot: the corrector and the back-substitution
// read the columns, the parent reads the trailing block.
struct eft_tree {
    int D, Nn, G, nn, ld, Ztot, P0, deep0, nsum0;  // deep0: the first node of depth D - 1
    const int32_t *depth, *child0, *nchild;        // [Nn] (children: nodes; none at depth D - 1)
    const int32_t *zoff, *path;                    // [Nn], [Nn][nn]: z index of the node's path entry k < P_d
    const int32_t *P;                              // [D]
    const int32_t *seg_start, *seg_of;             // [G + 1], [S]: the scenarios of deepest node deep0 + g
    double* zn;                                    // [EZ_N + 1][Ztot]: the nodes' z fields (ROOT's live in rootzd)
    double* rootzd;                                // [EZ_N + 1][P0]: ROOT's, as ef_solve_core reads them
    double *slot, *hv, *ty;                        // [Nn][nn * ld], [Nn][nn], [Nn][nn]
    double* nsc;                                   // [Nn][2]: a node's own complementarity, its |r_z| maximum
    double *segsum, *segmax;                       // [G][nsum0], [G][2]
    double *rootsum, *rootmax;                     // ROOT's sums as ef_solve_core takes them, [2]
    double *lsum, *lmax, *dirsum, *dirmax;         // [3], [2]: the lanes' direction sums; with the nodes'
    double *inspA, *inspb;                         // [Nn][nn * nn], [Nn][nn] or NULL: A_n and b_n as summed
};
#define EFT_SLOT(T, n) ((T).slot + (size_t)(n) * (T).nn * (T).ld)

#if defined(__HIPCC__) || defined(EF_HOST)
// field f of z entry idx (ROOT's entries are 0 .. P0 - 1)
EF_FN double* eft_zp(const eft_tree& T, int f, int idx) {
    return idx < T.P0 ? T.rootzd + (size_t)f * T.P0 + idx : T.zn + (size_t)f * T.Ztot + idx;
}
// a node's workspace position of path entry k
EF_FN int eft_pos(int k, int Pp, int nl) { return k < Pp ? nl + k : k - Pp; }

// What node n's children (its segment, at the deepest level) give: entry (i, j), j <= i, of A_n
// (vec 0), entry i of the right-hand side (vec 1) or of T'y (vec 2), in path order; the children in
// index order.
EF_FN double eft_gather(const eft_tree& T, int n, int stage, int vec, int i, int j) {
    const int d = T.depth[n];
    if (d == T.D - 1) {
        const double* r = T.segsum + (size_t)(n - T.deep0) * T.nsum0;
        const int ntri = T.nn * (T.nn + 1) / 2;
        if (vec == 0) return r[EF_TRI(i, j)];
        if (vec == 1) return r[(stage == 0 ? ntri : 0) + i];
        return r[ntri + T.nn + i];
    }
    const int nlc = T.P[d + 1] - T.P[d];
    double a = 0.0;
    for (int c = T.child0[n]; c < T.child0[n] + T.nchild[n]; ++c) {
        if (vec == 0) a += EFT_SLOT(T, c)[(size_t)(nlc + i) * T.ld + nlc + j];
        else a += (vec == 1 ? T.hv : T.ty)[(size_t)c * T.nn + nlc + i];
    }
    return a;
}

// A_n (stage 0), b_n and T'y (stage 0) into the workspace M [P][ld], b [P], ty [P]
EF_FN void eft_node_load(const eft_tree& T, int n, int stage, double* M, double* b, double* ty) {
    const int d = T.depth[n], P = T.P[d], Pp = d ? T.P[d - 1] : 0, nl = P - Pp, ld = T.ld;
    if (stage == 0)
        for (int e = LS_TID; e < P * P; e += LS_NT) {
            const int i = e / P, j = e % P;
            if (j > i) continue;
            const double v = eft_gather(T, n, stage, 0, i, j);
            const int r = eft_pos(i, Pp, nl), c = eft_pos(j, Pp, nl);
            M[r >= c ? r * ld + c : c * ld + r] = v;
            if (T.inspA) T.inspA[(size_t)n * T.nn * T.nn + (size_t)i * T.nn + j] = v;
        }
    for (int k = LS_TID; k < P; k += LS_NT) {
        const double v = eft_gather(T, n, stage, 1, k, 0);
        b[eft_pos(k, Pp, nl)] = v;
        if (T.inspb) T.inspb[(size_t)n * T.nn + k] = v;
        if (stage == 0) ty[eft_pos(k, Pp, nl)] = eft_gather(T, n, stage, 2, k, 0);
    }
    LS_SYNC();
}

// The node's own z entries into its diagonal block and right-hand side (3.21's terms of z, per
// node): Dz^-1 = qz + zl / sl + zu / su, regularised on the block's own diagonal; -r_z with the
// stage's targets.  stage 0 keeps T'y of the entries and the node's complementarity and |r_z|.
EF_FN void eft_node_zside(const eft_tree& T, const double* ctl, int n, int stage, double* M, double* b, const double* ty) {
    const int d = T.depth[n], nl = T.P[d] - (d ? T.P[d - 1] : 0), ld = T.ld;
    const double sigmu = ctl[EC_SIGMU];
    const int P = T.P[d];
    for (int k = LS_TID; k < nl; k += LS_NT) {
        const int zi = T.zoff[n] + k;
        if (ef_held(*eft_zp(T, EZ_LB, zi), *eft_zp(T, EZ_UB, zi))) {
            // A held entry (3.24): its row and column of the node's own block are the identity's and
            // its right-hand side 0, in both stages; the trailing block and h_n then get nothing from it.
            // (Off the diagonal, so no other thread's entry; where two held entries meet both store the same 0.)
            if (stage == 0) {
                for (int j = 0; j < k; ++j) M[k * ld + j] = 0.0;
                for (int i = k + 1; i < P; ++i) M[i * ld + k] = 0.0;
                M[k * ld + k] = 1.0;
                *eft_zp(T, EZ_N, zi) = ty[k];
            }
            b[k] = 0.0;
            continue;
        }
        const double z = *eft_zp(T, EZ_Z, zi), cz = *eft_zp(T, EZ_C, zi), qz = *eft_zp(T, EZ_Q, zi);
        const ef_box bx = ef_mkbox(z, *eft_zp(T, EZ_LB, zi), *eft_zp(T, EZ_UB, zi), *eft_zp(T, EZ_ZL, zi), *eft_zp(T, EZ_ZU, zi));
        if (stage == 0) {
            const double dd = M[k * ld + k] + qz + ef_theta(bx);
            M[k * ld + k] = dd + EF_REG * dd;
            *eft_zp(T, EZ_N, zi) = ty[k];
        }
        const double tyk = *eft_zp(T, EZ_N, zi);
        double tl, tu;
        ef_targets(stage, sigmu, bx, *eft_zp(T, EZ_DZA, zi), false, 0.0, tl, tu);
        b[k] += -(cz + qz * z - tyk - ef_push(bx, tl, tu));
    }
    if (stage == 0 && LS_TID == 0) {
        double comp = 0.0, rzm = 0.0;
        for (int k = 0; k < nl; ++k) {
            const int zi = T.zoff[n] + k;
            const double z = *eft_zp(T, EZ_Z, zi), zl = *eft_zp(T, EZ_ZL, zi), zu = *eft_zp(T, EZ_ZU, zi);
            const ef_box bx = ef_mkbox(z, *eft_zp(T, EZ_LB, zi), *eft_zp(T, EZ_UB, zi), zl, zu);
            if (ef_held(*eft_zp(T, EZ_LB, zi), *eft_zp(T, EZ_UB, zi))) continue;
            comp += (bx.fl ? bx.sl * bx.zl : 0.0) + (bx.fu ? bx.su * bx.zu : 0.0);
            rzm = fmax(rzm, fabs(*eft_zp(T, EZ_C, zi) + *eft_zp(T, EZ_Q, zi) * z - ty[k] - zl + zu));
        }
        T.nsc[(size_t)n * 2] = comp;
        T.nsc[(size_t)n * 2 + 1] = rzm;
    }
    LS_SYNC();
}

// stage 0: the partial factorisation of the workspace (ls_chol's right-looking steps and its
// dropped pivot, stopped after the node's own nl columns; the right-hand side rides along as one
// more column), then the workspace into the node's slot.  stage 1: the stored columns applied to
// the new right-hand side.  Either way (v | h_n) is kept in hv.
EF_FN void eft_node_factor(const eft_tree& T, int n, int stage, double* M, double* b, const double* ty) {
    const int d = T.depth[n], P = T.P[d], nl = P - (d ? T.P[d - 1] : 0), ld = T.ld;
    double* slot = EFT_SLOT(T, n);
    if (stage == 0) {
        double dmax = 0.0;
        for (int k = 0; k < nl; ++k) dmax = fmax(dmax, M[k * ld + k]);
        const double floor_ = 1e-40 * dmax;
        for (int j = 0; j < nl; ++j) {
            LS_SYNC();
            if (LS_TID == 0) {
                const double p = M[j * ld + j];
                M[j * ld + j] = p > floor_ ? sqrt(p) : 1e64;
                b[j] /= M[j * ld + j];
            }
            LS_SYNC();
            const double dj = M[j * ld + j], bj = b[j];
            for (int i = j + 1 + LS_TID; i < P; i += LS_NT) {
                M[i * ld + j] /= dj;
                b[i] -= M[i * ld + j] * bj;
            }
            LS_SYNC();
            const int m = P - j - 1;
            for (int e = LS_TID; e < m * m; e += LS_NT) {
                const int r = j + 1 + e / m, c = j + 1 + e % m;
                if (c <= r) M[r * ld + c] -= M[r * ld + j] * M[c * ld + j];
            }
        }
        LS_SYNC();
        for (int e = LS_TID; e < P * P; e += LS_NT) {
            const int r = e / P, c = e % P;
            if (c <= r) slot[(size_t)r * ld + c] = M[r * ld + c];
        }
    } else {
        for (int j = 0; j < nl; ++j) {
            LS_SYNC();
            if (LS_TID == 0) b[j] /= slot[(size_t)j * ld + j];
            LS_SYNC();
            const double bj = b[j];
            for (int i = j + 1 + LS_TID; i < P; i += LS_NT) b[i] -= slot[(size_t)i * ld + j] * bj;
        }
        LS_SYNC();
    }
    for (int k = LS_TID; k < P; k += LS_NT) T.hv[(size_t)n * T.nn + k] = b[k];
    if (stage == 0)
        for (int k = LS_TID; k < P; k += LS_NT) T.ty[(size_t)n * T.nn + k] = ty[k];
}

// one node's elimination (W: P * ld + 2 P doubles shared by the node's threads)
EF_FN void eft_elim_core(const eft_tree& T, const double* ctl, int n, int stage, double* W) {
    if (ctl[EC_DONE] != 0.0) return;
    const int P = T.P[T.depth[n]];
    double *M = W, *b = W + (size_t)P * T.ld, *ty = b + P;
    eft_node_load(T, n, stage, M, b, ty);
    eft_node_zside(T, ctl, n, stage, M, b, ty);
    eft_node_factor(T, n, stage, M, b, ty);
}

// dz of the node's own entries from its stored columns, v and the ancestors' dz (one thread)
EF_FN void eft_node_back(const eft_tree& T, int n) {
    const int d = T.depth[n], P = T.P[d], Pp = d ? T.P[d - 1] : 0, nl = P - Pp, ld = T.ld;
    const double* slot = EFT_SLOT(T, n);
    double* dz = eft_zp(T, EZ_DZ, T.zoff[n]);
    for (int j = nl - 1; j >= 0; --j) {
        if (ef_held(*eft_zp(T, EZ_LB, T.zoff[n] + j), *eft_zp(T, EZ_UB, T.zoff[n] + j))) {
            dz[j] = 0.0;  // (exactly: its column is the identity's)
            continue;
        }
        double a = T.hv[(size_t)n * T.nn + j];
        for (int i = j + 1; i < nl; ++i) a -= slot[(size_t)i * ld + j] * dz[i];
        for (int k = 0; k < Pp; ++k) a -= slot[(size_t)(nl + k) * ld + j] * *eft_zp(T, EZ_DZ, T.path[(size_t)n * T.nn + k]);
        dz[j] = a / slot[(size_t)j * ld + j];
    }
}

// what z entry zi (not ROOT's) gives to the step lengths and the affine mu
EF_FN void eft_z_ratios(const eft_tree& T, const double* ctl, int stage, int zi, double& rp, double& rd, double (&ct)[3]) {
    if (ef_held(*eft_zp(T, EZ_LB, zi), *eft_zp(T, EZ_UB, zi))) return;
    const ef_box b = ef_mkbox(*eft_zp(T, EZ_Z, zi), *eft_zp(T, EZ_LB, zi), *eft_zp(T, EZ_UB, zi), *eft_zp(T, EZ_ZL, zi),
                              *eft_zp(T, EZ_ZU, zi));
    const double dz = *eft_zp(T, EZ_DZ, zi);
    double tl, tu, dl, du;
    ef_targets(stage, ctl[EC_SIGMU], b, *eft_zp(T, EZ_DZA, zi), false, 0.0, tl, tu);
    ef_dual_dirs(b, dz, tl, tu, false, 0.0, dl, du);
    ef_ratios(b, dz, dl, du, rp, rd, ct);
}
// z entry zi (not ROOT's) after ef_ctrl_core: stage 0 keeps the affine dz, stage 1 takes the step
EF_FN void eft_z_step(const eft_tree& T, const double* ctl, int stage, int zi) {
    if (ctl[EC_DONE] != 0.0 || ef_held(*eft_zp(T, EZ_LB, zi), *eft_zp(T, EZ_UB, zi))) return;  // (a held z keeps its bits)
    const double dz = *eft_zp(T, EZ_DZ, zi);
    if (stage == 0) {
        *eft_zp(T, EZ_DZA, zi) = dz;
        return;
    }
    const ef_box b = ef_mkbox(*eft_zp(T, EZ_Z, zi), *eft_zp(T, EZ_LB, zi), *eft_zp(T, EZ_UB, zi), *eft_zp(T, EZ_ZL, zi),
                              *eft_zp(T, EZ_ZU, zi));
    double tl, tu, dl, du;
    ef_targets(1, ctl[EC_SIGMU], b, *eft_zp(T, EZ_DZA, zi), false, 0.0, tl, tu);
    ef_dual_dirs(b, dz, tl, tu, false, 0.0, dl, du);
    *eft_zp(T, EZ_Z, zi) += ctl[EC_AP] * dz;
    *eft_zp(T, EZ_ZL, zi) += ctl[EC_AD] * dl;
    *eft_zp(T, EZ_ZU, zi) += ctl[EC_AD] * du;
}

// A deepest node's view of the store: its own zd block (a gathered copy of its path's z and dz);
// C is not read by the lanes and ctl is the ONE record of the tree (a bundle has its own).
EF_FN ef_store eft_seg_view(const ef_store& E, int64_t g) {
    ef_store V = E;
    V.zd = E.zd + (size_t)g * EF_ZD_LEN(E);
    return V;
}
// ROOT's view: the store as ef_solve_core and ef_ctrl_core take it, nn = P0 (the host builds it)
#ifndef EF_HOST
__host__
#endif
EF_FN ef_store eft_root_view(const ef_store& E, const eft_tree& T) {
    ef_store R = E;
    R.nn = T.P0;
    R.ntri = T.P0 * (T.P0 + 1) / 2;
    R.ld = T.P0 | 1;
    R.zd = T.rootzd;
    return R;
}
#endif  // __HIPCC__ || EF_HOST

#if defined(__HIPCC__) && !defined(EF_HOST)
// ------------------------------------------------------------------ kernels
#define EFT_LANE(call)                                                \
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; \
    if (s < st.S) {                                                   \
        const ef_store V = eft_seg_view(E, T.seg_of[s]);              \
        call;                                                         \
    }
__global__ void __launch_bounds__(EF_T) k_eft_schur(ph_data st, ef_store E, eft_tree T, int stage) {
    EFT_LANE(ef_schur_lane(st, V, s, stage));
}
__global__ void __launch_bounds__(EF_T) k_eft_direction(ph_data st, ef_store E, eft_tree T, int stage) {
    EFT_LANE(ef_direction_lane(st, V, s, stage));
}
__global__ void __launch_bounds__(EF_T)
k_eft_export(ph_data st, ef_store E, eft_tree T, double* __restrict__ x, double* __restrict__ y, double* __restrict__ obj,
             double* __restrict__ bound, int32_t* __restrict__ status, int32_t* __restrict__ iters) {
    EFT_LANE(ef_export_lane(st, V, s, x, y, obj, bound, status, iters));
}

// field f of every segment's path into its zd block: one thread per (segment, path entry)
__global__ void __launch_bounds__(EF_T) k_eft_gather(ef_store E, eft_tree T, int f) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T.G * T.nn) return;
    const int g = t / T.nn, k = t % T.nn;
    E.zd[(size_t)g * EF_ZD_LEN(E) + (size_t)f * T.nn + k] = *eft_zp(T, f, T.path[(size_t)(T.deep0 + g) * T.nn + k]);
}

// The segmented sum of the lanes' planes, fixed-order and without atomics, two ways.  Short
// segments: one THREAD per (plane, segment), the segment fastest (k_bd_reduce's shape).
__global__ void __launch_bounds__(GR_T) k_eft_reduce_t(ef_store E, eft_tree T, int64_t S, int nsum, int nmax) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)(nsum + nmax) * T.G || E.ctl[EC_DONE] != 0.0) return;
    const int b = (int)(t / T.G), g = (int)(t % T.G);
    const bool mx = b >= nsum;
    double acc = 0.0;
    for (int64_t s = T.seg_start[g]; s < T.seg_start[g + 1]; ++s) {
        const double v = E.terms[IX(b)];
        acc = mx ? fmax(acc, v) : acc + v;
    }
    if (mx) T.segmax[(size_t)g * 2 + (b - nsum)] = acc;
    else T.segsum[(size_t)g * T.nsum0 + b] = acc;
}
// Long segments: one BLOCK per (plane, segment) (k_ef_reduce's shape): every thread takes its
// scenarios of the segment in index order, the block its threads in a fixed order.
__global__ void __launch_bounds__(GR_T) k_eft_reduce_b(ef_store E, eft_tree T, int64_t S, int nsum) {
    __shared__ double red[GR_T / WAVE];
    if (E.ctl[EC_DONE] != 0.0) return;
    const int b = blockIdx.x, g = blockIdx.y;
    const bool mx = b >= nsum;
    double acc = 0.0;
    for (int64_t s = (int64_t)T.seg_start[g] + threadIdx.x; s < T.seg_start[g + 1]; s += GR_T) {
        const double v = E.terms[IX(b)];
        acc = mx ? fmax(acc, v) : acc + v;
    }
    if (!mx) {
        const double t = block_sum_fixed(acc, red);
        if (threadIdx.x == 0) T.segsum[(size_t)g * T.nsum0 + b] = t;
        return;
    }
    acc = wave_max(acc);
    if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int u = 0; u < GR_T / WAVE; ++u) t = fmax(t, red[u]);
        T.segmax[(size_t)g * 2 + (b - nsum)] = t;
    }
}

// One wave per node of one depth (n0: the depth's first node): the workspace in LDS (dynamic, the
// kernel's only shared memory; ld is odd, 3.19).
__global__ void __launch_bounds__(WAVE) k_eft_elim(ef_store E, eft_tree T, int n0, int stage) {
    eft_elim_core(T, E.ctl, n0 + (int)blockIdx.x, stage, ef_dyn);
}

// ROOT's sums as ef_solve_core takes them: {A_ROOT (lower triangle by rows) | b | T'y | comp | obj}
// and the maxima {primal, dual}; stage 1: {b}.  The scalars over the segments and then over the
// nodes, each thread its share in index order, the block in a fixed order.
__global__ void __launch_bounds__(GR_T) k_eft_root(ef_store E, eft_tree T, int stage) {
    __shared__ double red[GR_T / WAVE];
    if (E.ctl[EC_DONE] != 0.0) return;
    const int P0 = T.P0, ntri0 = P0 * (P0 + 1) / 2, ntri = T.nn * (T.nn + 1) / 2;
    if (stage == 1) {
        for (int k = threadIdx.x; k < P0; k += GR_T) {
            const double v = eft_gather(T, 0, 1, 1, k, 0);
            T.rootsum[k] = v;
            if (T.inspb) T.inspb[k] = v;
        }
        return;
    }
    for (int e = threadIdx.x; e < P0 * P0; e += GR_T) {
        const int i = e / P0, j = e % P0;
        if (j > i) continue;
        const double v = eft_gather(T, 0, 0, 0, i, j);
        T.rootsum[EF_TRI(i, j)] = v;
        if (T.inspA) T.inspA[(size_t)i * T.nn + j] = v;
    }
    for (int k = threadIdx.x; k < P0; k += GR_T) {
        const double v = eft_gather(T, 0, 0, 1, k, 0);
        T.rootsum[ntri0 + k] = v;
        if (T.inspb) T.inspb[k] = v;
        T.rootsum[ntri0 + P0 + k] = eft_gather(T, 0, 0, 2, k, 0);
    }
    double sc[2] = {0.0, 0.0}, mx[2] = {0.0, 0.0};
    for (int g = threadIdx.x; g < T.G; g += GR_T) {
        sc[0] += T.segsum[(size_t)g * T.nsum0 + ntri + 2 * T.nn];
        sc[1] += T.segsum[(size_t)g * T.nsum0 + ntri + 2 * T.nn + 1];
        mx[0] = fmax(mx[0], T.segmax[(size_t)g * 2]);
        mx[1] = fmax(mx[1], T.segmax[(size_t)g * 2 + 1]);
    }
    double nc = 0.0;
    for (int n = 1 + threadIdx.x; n < T.Nn; n += GR_T) {
        nc += T.nsc[(size_t)n * 2];
        mx[1] = fmax(mx[1], T.nsc[(size_t)n * 2 + 1]);
    }
    double comp = block_sum_fixed(sc[0], red);  // (thread 0's; red is reused: a barrier between the sums)
    __syncthreads();
    comp += block_sum_fixed(nc, red);
    __syncthreads();
    const double obj = block_sum_fixed(sc[1], red);
    for (int u = 0; u < 2; ++u) {
        __syncthreads();
        const double w = wave_max(mx[u]);
        if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = w;
        __syncthreads();
        if (threadIdx.x == 0) {
            double t = 0.0;
            for (int v = 0; v < GR_T / WAVE; ++v) t = fmax(t, red[v]);
            T.rootmax[u] = t;
        }
    }
    if (threadIdx.x == 0) {
        T.rootsum[ntri0 + 2 * P0] = comp;
        T.rootsum[ntri0 + 2 * P0 + 1] = obj;
    }
}

// one thread per node of one depth, top-down after ROOT's solve
__global__ void __launch_bounds__(EF_T) k_eft_back(ef_store E, eft_tree T, int n0, int cnt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < cnt && E.ctl[EC_DONE] == 0.0) eft_node_back(T, n0 + i);
}

// The nodes' share of a direction's sums and maxima (every z entry below ROOT; ROOT's own are
// ef_ctrl_core's), added to the lanes': one block, each thread its entries in index order.
__global__ void __launch_bounds__(GR_T) k_eft_dirsum(ef_store E, eft_tree T, int stage) {
    __shared__ double red[GR_T / WAVE];
    if (E.ctl[EC_DONE] != 0.0) return;
    double rp = 0.0, rd = 0.0, ct[3] = {0.0, 0.0, 0.0};
    for (int zi = T.P0 + threadIdx.x; zi < T.Ztot; zi += GR_T) eft_z_ratios(T, E.ctl, stage, zi, rp, rd, ct);
    double out[5];
    for (int u = 0; u < 3; ++u) {
        __syncthreads();  // (red is reused)
        out[u] = block_sum_fixed(ct[u], red);
    }
    for (int u = 0; u < 2; ++u) {
        __syncthreads();
        const double w = wave_max(u == 0 ? rp : rd);
        if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = w;
        __syncthreads();
        double t = 0.0;
        for (int v = 0; v < GR_T / WAVE; ++v) t = fmax(t, red[v]);
        out[3 + u] = t;
    }
    if (threadIdx.x == 0) {
        for (int u = 0; u < 3; ++u) T.dirsum[u] = T.lsum[u] + out[u];
        for (int u = 0; u < 2; ++u) T.dirmax[u] = fmax(T.lmax[u], out[3 + u]);
    }
}

// one thread per z entry below ROOT, after k_ef_ctrl on ROOT's view
__global__ void __launch_bounds__(EF_T) k_eft_zstep(ef_store E, eft_tree T, int stage) {
    const int zi = T.P0 + blockIdx.x * blockDim.x + threadIdx.x;
    if (zi < T.Ztot) eft_z_step(T, E.ctl, stage, zi);
}
#endif
