// solve_stream.inc -- the shared-matrix streaming path (path 4; DESIGN.md 3.5).
//
// For scenarios whose constraint matrix is the same in every scenario and too large for
// the register / workgroup-resident paths (the UC relaxation of config 5: n ~ 57k
// columns, m ~ 57k rows, nnz ~ 216k), one scaled copy of A (CSR + CSC values) serves all
// scenarios and stays hot in L2 / MALL, and one 1024-thread workgroup runs one
// scenario's PDHG with its iterates streamed through a scenario-major record in HBM:
//
//   record = X X0 U XT (n each) | Y Y0 YT (m each) | PC (8 per per-scenario column) |
//            PR (4 per per-scenario row)
//
// Columns whose cost / bounds differ between scenarios, and every nonant column (PH
// terms, fixing), are "per-scenario columns" P with their data in PC; all other columns
// read the shared base (scenario 0) in sh_col.  Rows likewise (R, PR / sh_row).
//
// One PDHG iteration is two passes with a workgroup barrier between them:
//   column pass  aty_j = sum_i A_ij Y_i (CSC gather of this scenario's Y), the primal
//                step xt, U = 2 xt - x, and the Halpern update of X in place;
//   row pass     ax_i = sum_j A_ij U_j (CSR gather), the dual step yt and the Halpern
//                update of Y in place.
// A^T y is recomputed each iteration instead of carried (k_solve carries it by the
// Halpern recurrence; the two agree up to rounding).  At restart-test iterations X / Y
// are left alone and T(z) goes to XT / YT; a fix-up pass then applies the restart or
// the Halpern step.  The KKT / infeasibility tests are two more passes every
// check_every iterations.  Algorithm, tests and constants are k_solve's.
#define SBLK 1024
#define SWAVES (SBLK / WAVE)
// the start index of a per-thread loop, hidden from the optimiser: otherwise every
// "base + tid * stride" start pointer of every loop is hoisted to the kernel entry and
// kept live (in VGPR pairs) across the whole solve, which costs more registers than the
// loops themselves
__device__ __forceinline__ int opq(int v) {
    asm volatile("" : "+v"(v));
    return v;
}

// sum of NV values over the workgroup (wave sums, then the wave partials in wave order:
// identical bits in every thread).  red: LDS [2][NV][SWAVES], halves used alternately.
template <int NV>
__device__ __forceinline__ void sblock_sum(double (&v)[NV], double* red, int& parity) {
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = wave_sum(v[i]);
    double* r = red + parity * NV * SWAVES;
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) r[i * SWAVES + wv] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        double a = 0.0;
#pragma unroll
        for (int w = 0; w < SWAVES; ++w) a += r[i * SWAVES + w];
        v[i] = a;
    }
    parity ^= 1;
}

// The split form (DESIGN.md 3.5): one scenario over a cluster of K workgroups of the
// cooperative grid -- the whole grid for the straggler scenarios of a large batch (one
// cluster), K = grid / S for a batch smaller than the GPU (a strong-scaling share: every
// scenario gets several CUs instead of one).  grid_sync is the cluster's barrier;
// grid_sum adds the workgroup totals in block order from a double-buffered partials array
// (8 per block): identical bits in every thread of every block of the cluster.
// The barrier is a counter per cluster that only grows during a launch (set to gbase before
// it): every block adds 1 with agent-scope release (its stores written back past its XCD's
// L2) and waits, with agent-scope acquire, until the count reaches the next multiple of K.
// A cooperative launch guarantees that every block is resident.
__device__ __forceinline__ void grid_sync(unsigned* __restrict__ bar, unsigned& target, int K) {
    __syncthreads();
    target += (unsigned)K;
    if (threadIdx.x == 0) {
        __hip_atomic_fetch_add(bar, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        // wrap-safe: the count may pass 2^32 over a long straggler (3+ barriers per PDHG
        // iteration); compare the signed distance, not the raw values
        while ((int)(__hip_atomic_load(bar, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) - target) < 0)
            __builtin_amdgcn_s_sleep(1);
    }
    __syncthreads();
}

template <int NV>
__device__ __forceinline__ void grid_sum(double (&v)[NV], double* red, int& parity, double* __restrict__ gpart,
                                         int& gpar, unsigned* __restrict__ bar, unsigned& target, int K, int cb) {
    sblock_sum<NV>(v, red, parity);
    double* gp = gpart + (size_t)gpar * K * 8;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) gp[cb * 8 + i] = v[i];
    }
    grid_sync(bar, target, K);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        double a = 0.0;
        for (int g = 0; g < K; ++g) a += gp[g * 8 + i];
        v[i] = a;
    }
    gpar ^= 1;
}

// sum_k val[e_k] * v[idx[e_k]] over the sliced-ELL entries of one slice member (lane):
// four entries per step, their index / value loads coalesced across the wave and their
// four gathers in flight together (entries in CSR / CSC order: the same sum as a plain
// CSR / CSC loop)
__device__ __forceinline__ double sell_dot(const int32_t* __restrict__ idx, const double* __restrict__ val, int base,
                                           int len, int lane, const double* __restrict__ v) {
    const int32_t* ip = idx + base + lane;
    const double* vp = val + base + lane;
    double a = 0.0;
    int k = 0;
    for (; k + 4 <= len; k += 4) {
        const int i0 = ip[0], i1 = ip[WAVE], i2 = ip[2 * WAVE], i3 = ip[3 * WAVE];
        const double c0 = vp[0], c1 = vp[WAVE], c2 = vp[2 * WAVE], c3 = vp[3 * WAVE];
#ifdef PHGPU_EXP_LOCAL_GATHER
        const double g0 = v[i0 & 1023], g1 = v[i1 & 1023], g2 = v[i2 & 1023], g3 = v[i3 & 1023];
#else
        const double g0 = v[i0], g1 = v[i1], g2 = v[i2], g3 = v[i3];
#endif
        a += c0 * g0;
        a += c1 * g1;
        a += c2 * g2;
        a += c3 * g3;
        ip += 4 * WAVE;
        vp += 4 * WAVE;
    }
    for (; k < len; ++k) {
        a += vp[0] * v[ip[0]];
        ip += WAVE;
        vp += WAVE;
    }
    return a;
}

// the same over the B scenario slots of a workgroup: one index / value load feeds the
// gathers of every active slot (the matrix is read once for B scenarios)
template <int B>
__device__ __forceinline__ void sell_dot_b(const int32_t* __restrict__ idx, const double* __restrict__ val, int base,
                                           int len, int lane, double* const (&v)[B], const bool (&act)[B],
                                           double (&out)[B]) {
    const int32_t* ip = idx + base + lane;
    const double* vp = val + base + lane;
#pragma unroll
    for (int b = 0; b < B; ++b) out[b] = 0.0;
    int k = 0;
    for (; k + 4 <= len; k += 4) {
        const int i0 = ip[0], i1 = ip[WAVE], i2 = ip[2 * WAVE], i3 = ip[3 * WAVE];
        const double c0 = vp[0], c1 = vp[WAVE], c2 = vp[2 * WAVE], c3 = vp[3 * WAVE];
#pragma unroll
        for (int b = 0; b < B; ++b) {
            if (!act[b]) continue;
            const double* __restrict__ w = v[b];
            const double g0 = w[i0], g1 = w[i1], g2 = w[i2], g3 = w[i3];
            double a = out[b];
            a += c0 * g0;
            a += c1 * g1;
            a += c2 * g2;
            a += c3 * g3;
            out[b] = a;
        }
        ip += 4 * WAVE;
        vp += 4 * WAVE;
    }
    for (; k < len; ++k) {
        const int i0 = ip[0];
        const double c0 = vp[0];
#pragma unroll
        for (int b = 0; b < B; ++b)
            if (act[b]) out[b] += c0 * v[b][i0];
        ip += WAVE;
        vp += WAVE;
    }
}

// One workgroup runs B scenarios ("slots") in lockstep: every PDHG iteration does one
// column pass and one row pass over the shared matrix for all active slots; each slot
// keeps its own iteration count, restart state, checks and termination, and a slot whose
// scenario finishes takes the next one from the queue while the others go on.  B = 1 is
// one scenario per workgroup.  The queue starts at position q0 (the ones before it went to
// the split form).
// SPLIT (B = 1, cooperative launch): the grid is ncl clusters of K = grid / ncl
// workgroups; cluster c runs the scenarios sk_order[c], sk_order[c + ncl], ... below q0 one
// after another -- every per-thread loop strides over the cluster, the slices of a pass go
// round-robin over the cluster's waves, the workgroup barriers become cluster barriers and
// the workgroup sums cluster sums; the control flow stays uniform over a cluster.
// Partials: gpart [ncl][2][K][8], then the clusters' barrier counters 128 B apart.
template <int B, bool SPLIT = false>
__global__ void __launch_bounds__(SBLK, B == 1 ? 8 : 4)
k_solve_stream(pdhg_view st, solve_params P, int* __restrict__ qhead, double* __restrict__ xout,
               double* __restrict__ yout, double* __restrict__ obj, double* __restrict__ bound,
               int32_t* __restrict__ status, int32_t* __restrict__ iters, int q0, double* __restrict__ gpart,
               unsigned gbase, int ncl) {
    static_assert(!SPLIT || B == 1, "the split form runs one scenario at a time");
    __shared__ double red[2 * 8 * SWAVES];
    __shared__ int s_next;
    const int n = st.n, m = st.m;
    const int S = (int)st.S;
    const int tid = threadIdx.x;
    const int32_t* __restrict__ row_ptr = st.row_ptr;
    const int32_t* __restrict__ col_idx = st.col_idx;
    const int32_t* __restrict__ col_ptr = st.col_ptr;
    const int32_t* __restrict__ row_idx = st.row_idx;
    const double* __restrict__ Ahr = st.Ah_csr;
    const double* __restrict__ Ahc = st.Ah_csc;
    const double g = P.gamma;
    const int32_t* __restrict__ cmap = st.cmap;
    const int32_t* __restrict__ rmap = st.rmap;
    const double* __restrict__ sh_col = st.sh_col;
    const double* __restrict__ sh_row = st.sh_row;
    const double* __restrict__ Dc = st.Dc;
    const double* __restrict__ Dr = st.Dr;
    const int32_t* __restrict__ cs_off = st.cs_off;
    const int32_t* __restrict__ cs_len = st.cs_len;
    const int32_t* __restrict__ cs_idx = st.cs_idx;
    const double* __restrict__ cs_val = st.cs_val;
    const int32_t* __restrict__ rs_off = st.rs_off;
    const int32_t* __restrict__ rs_len = st.rs_len;
    const int32_t* __restrict__ rs_idx = st.rs_idx;
    const double* __restrict__ rs_val = st.rs_val;
    const int32_t* __restrict__ cw_ptr = st.cw_ptr;
    const int32_t* __restrict__ cw_slc = st.cw_slc;
    const int32_t* __restrict__ rw_ptr = st.rw_ptr;
    const int32_t* __restrict__ rw_slc = st.rw_slc;
    const int wv = __builtin_amdgcn_readfirstlane(tid / WAVE), lane = tid % WAVE;
    int parity = 0, gpar = 0;
    // the split form's cluster: K workgroups, this one's index cb in it, cluster cid
    const int K = SPLIT ? (int)gridDim.x / ncl : 1;
    const int cid = SPLIT ? (int)blockIdx.x / K : 0;
    const int cb = SPLIT ? (int)blockIdx.x - cid * K : 0;
    unsigned gtarget = gbase;  // the cluster's barrier count (gbar: after the partials; starts at gbase)
    unsigned* __restrict__ gbar = SPLIT ? (unsigned*)(gpart + 2 * (size_t)gridDim.x * 8) + 32 * cid : nullptr;
    double* __restrict__ gpc = SPLIT ? gpart + (size_t)cid * 2 * K * 8 : nullptr;
    // per-thread loops: start and stride (the workgroup, or the cluster in the split form)
    const int gt = SPLIT ? cb * SBLK + tid : tid;
    const int gs = SPLIT ? K * SBLK : SBLK;
    auto sync = [&]() {
        if constexpr (SPLIT) grid_sync(gbar, gtarget, K);
        else __syncthreads();
    };
    auto bsum = [&](auto& v) {
        constexpr int NV = (int)(sizeof(v) / sizeof(v[0]));
        if constexpr (SPLIT) grid_sum<NV>(v, red, parity, gpc, gpar, gbar, gtarget, K, cb);
        else sblock_sum<NV>(v, red, parity);
    };
    int split_i = 0;  // the split form's position in the cluster's scenarios
    auto col_data = [=](const double* PC, int j, double& ch, double& qh, double& lo, double& hi) {
        const int p = cmap[j];
        const double* a = p < 0 ? sh_col + 4 * (size_t)j : PC + 8 * (size_t)p + 4;
        ch = a[0];
        qh = a[1];
        lo = a[2];
        hi = a[3];
    };
    auto row_data = [=](const double* PR, int i, double& rlh, double& ruh, double& rl, double& ru) {
        const int p = rmap[i];
        const double* a = p < 0 ? sh_row + 4 * (size_t)i : PR + 4 * (size_t)p;
        rlh = a[0];
        ruh = a[1];
        rl = a[2];
        ru = a[3];
    };
    auto rec_of = [&](int s) { return st.sk + (size_t)s * (size_t)st.sk_stride; };
    // KKT quantities of one scenario at (XT, YT) (original space), with ``inf`` also the
    // certificate sums from d = T(z) - z: o = {pres2, dres2, pobj, dobj, ray obj, ray
    // viol2, c'dx, dual viol2}; workgroup sum included
    auto kkt_sums = [&](const double* rec, bool inf, double (&o)[8]) {
        const double* X = rec + st.sk_X;
        const double* XT = rec + st.sk_XT;
        const double* Y = rec + st.sk_Y;
        const double* YT = rec + st.sk_YT;
        const double* PC = rec + st.sk_PC;
        const double* PR = rec + st.sk_PR;
        for (int k = 0; k < 8; ++k) o[k] = 0.0;
        for (int i = opq(gt); i < m; i += gs) {
            double ax = 0.0, adx = 0.0;
            const int k1 = row_ptr[i + 1];
            for (int k = row_ptr[i]; k < k1; ++k) {
                const int j = col_idx[k];
                const double a = Ahr[k];
                ax += a * XT[j];
                if (inf) adx += a * (XT[j] - X[j]);
            }
            const double dr = Dr[i];
            double rlh, ruh, rl, ru;
            row_data(PR, i, rlh, ruh, rl, ru);
            ax /= dr;
            const double v = ax - clampd(ax, rl, ru);
            o[0] += v * v;
            o[3] += row_dual_term(YT[i] * dr, rl, ru);
            if (inf) {
                ray_row_terms(dr * (YT[i] - Y[i]), rl, ru, o[4], o[5]);
                o[7] += recession_viol2(adx / dr, rl, ru);
            }
        }
        for (int j = opq(gt); j < n; j += gs) {
            double at = 0.0, aty = 0.0;
            const int k1 = col_ptr[j + 1];
            for (int kc = col_ptr[j]; kc < k1; ++kc) {
                const int i = row_idx[kc];
                const double a = Ahc[kc];
                at += a * YT[i];
                if (inf) aty += a * Y[i];
            }
            const double d = Dc[j];
            double ch, qh, lbh, ubh;
            col_data(PC, j, ch, qh, lbh, ubh);
            const double xo = d * XT[j];
            const double ce = ch / d, qe = qh / (d * d);
            const double lbj = lbh * d, ubj = ubh * d;
            const double atd = at / d;
            const double rc = ce + qe * xo - atd;
            double lam;
            if (isfinite(lbj) && isfinite(ubj)) lam = rc;
            else if (isfinite(lbj)) lam = fmax(rc, 0.0);
            else if (isfinite(ubj)) lam = fmin(rc, 0.0);
            else lam = 0.0;
            const double dr = rc - lam;
            o[1] += dr * dr;
            o[2] += ce * xo + 0.5 * qe * xo * xo;
            o[3] += col_dual_term(ce - atd, qe, lbj, ubj);
            if (inf) {
                ray_col_terms(-(at - aty) / d, lbj, ubj, o[4], o[5]);
                const double dxo = d * (XT[j] - X[j]);
                o[6] += ce * dxo;
                o[7] += recession_viol2(dxo, lbj, ubj) + (qe * dxo) * (qe * dxo);
            }
        }
        bsum(o);
    };

    // ---- slot state (workgroup-uniform)
    int sc[B], hk[B], itc[B], stat[B];
    double omega[B], r0[B], rlast[B], pobj[B], dobj[B], cnorm[B], bnorm[B], cterm[B], eta[B];
    bool ran_kkt[B];

    // start scenario s in slot b: effective objective of this solve on the per-scenario
    // columns (phbase.py:617-699), scaled; norms; start point (previous solution, clamped,
    // or 0)
    auto start = [&](int b, int s) {
        sc[b] = s;
        if (s >= S) return;
        double* rec = rec_of(s);
        double* X = rec + st.sk_X;
        double* X0 = rec + st.sk_X0;
        double* Y = rec + st.sk_Y;
        double* Y0 = rec + st.sk_Y0;
        double* PC = rec + st.sk_PC;
        const double* PR = rec + st.sk_PR;
        double nrm[3] = {0.0, 0.0, 0.0};
        for (int p = opq(gt); p < st.np; p += gs) {
            const int j = st.pcol[p];
            double* e = PC + 8 * (size_t)p;
            double cj = e[0], qj = e[1];
            const int k = st.nonant_slot[j];
            if (k >= 0) {
                const size_t ik = (size_t)k * (size_t)S + (size_t)s;
                if (st.W_on) cj += st.W[ik];
                if (st.prox_on) {
                    const double r = st.rho[ik], xb = st.xbar[ik];
                    cj -= r * xb;
                    qj += r;
                    nrm[1] += 0.5 * r * xb * xb;
                }
            }
            const double d = Dc[j];
            e[4] = d * cj;
            e[5] = d * d * qj;
            nrm[0] += cj * cj;
        }
        for (int p = opq(gt); p < st.nr; p += gs) {
            const double a = PR[4 * (size_t)p + 2], bb = PR[4 * (size_t)p + 3];
            if (isfinite(a)) nrm[2] += a * a;
            if (isfinite(bb) && bb != a) nrm[2] += bb * bb;
        }
        bsum(nrm);
        cnorm[b] = sqrt(nrm[0] + st.sh_norm[1]);
        bnorm[b] = sqrt(nrm[2] + st.sh_norm[2]);
        cterm[b] = nrm[1] + (st.objc ? st.objc[s] : 0.0);
        for (int j = opq(gt); j < n; j += gs) {
            double ch, qh, lo, hi;
            col_data(PC, j, ch, qh, lo, hi);
            const double v = clampd(P.warm ? X[j] : 0.0, lo, hi);
            X[j] = v;
            X0[j] = v;
        }
        for (int i = opq(gt); i < m; i += gs) {
            const double v = P.warm ? Y[i] : 0.0;
            Y[i] = v;
            Y0[i] = v;
        }
        sync();
        double om = st.omega[s];
        if (!(P.keep_omega && P.warm) && P.omega0 > 0.0) om = P.omega0;
        omega[b] = om;
        eta[b] = P.eta_frac / st.sh_norm[0];
        r0[b] = -1.0;
        rlast[b] = INFINITY;
        pobj[b] = dobj[b] = 0.0;
        hk[b] = 0;
        itc[b] = 0;
        stat[b] = PHGPU_ITER_LIMIT;
        ran_kkt[b] = false;
    };
    // the scenario of slot b is done: the answer is T(z) of its last (check) iteration;
    // outputs, warm start, then the next scenario of the queue into the slot
    auto finish = [&](int b) {
        const int s = sc[b];
        double* rec = rec_of(s);
        if (!ran_kkt[b]) {
            double o[8];
            kkt_sums(rec, false, o);
            pobj[b] = cterm[b] + o[2];
            dobj[b] = cterm[b] + o[3];
        }
        if (stat[b] == PHGPU_PRIMAL_INFEASIBLE) pobj[b] = dobj[b] = INFINITY;
        if (stat[b] == PHGPU_DUAL_INFEASIBLE) pobj[b] = dobj[b] = -INFINITY;
        double* X = rec + st.sk_X;
        const double* XT = rec + st.sk_XT;
        double* Y = rec + st.sk_Y;
        const double* YT = rec + st.sk_YT;
        for (int j = opq(gt); j < n; j += gs) {
            const double v = XT[j];
            X[j] = v;
            xout[(size_t)j * (size_t)S + (size_t)s] = Dc[j] * v;
        }
        for (int i = opq(gt); i < m; i += gs) {
            const double v = YT[i];
            Y[i] = v;
            if (yout) yout[(size_t)i * (size_t)S + (size_t)s] = Dr[i] * v;
        }
        if constexpr (SPLIT) {
            if (cb == 0 && tid == 0) {
                st.omega[s] = omega[b];
                obj[s] = pobj[b];
                bound[s] = dobj[b];
                status[s] = stat[b];
                const int used = (stat[b] == PHGPU_ITER_LIMIT) ? P.max_iter : itc[b];
                if (iters) iters[s] = used;
                st.sk_iters[s] = P.warm ? (7 * st.sk_iters[s] + 3 * used + 5) / 10 : used;
            }
            ++split_i;
            const int qn = cid + ncl * split_i;
            start(b, qn < q0 ? st.sk_order[qn] : S);
            return;
        }
        if (tid == 0) {
            st.omega[s] = omega[b];
            obj[s] = pobj[b];
            bound[s] = dobj[b];
            status[s] = stat[b];
            const int used = (stat[b] == PHGPU_ITER_LIMIT) ? P.max_iter : itc[b];
            if (iters) iters[s] = used;
            // the next solve's queue key: an exponential average of the counts once warm
            // (the register path's predictor, solve_reg.inc)
            st.sk_iters[s] = P.warm ? (7 * st.sk_iters[s] + 3 * used + 5) / 10 : used;
            const int qn = q0 + atomicAdd(qhead, 1) + (int)gridDim.x * B;
            s_next = qn < S ? st.sk_order[qn] : S;
        }
        __syncthreads();
        const int nxt = __builtin_amdgcn_readfirstlane(s_next);
        __syncthreads();
        start(b, nxt);
    };

#pragma unroll
    for (int b = 0; b < B; ++b) {
        const int qi = SPLIT ? cid : q0 + (int)blockIdx.x * B + b;
        start(b, qi < S && (!SPLIT || qi < q0) ? st.sk_order[qi] : S);
    }
    while (true) {
        bool act[B];
        bool any = false;
#pragma unroll
        for (int b = 0; b < B; ++b) {
            act[b] = sc[b] < S;
            any |= act[b];
        }
        if (!any) break;
        double* Xb[B];
        double* X0b[B];
        double* Ub[B];
        double* XTb[B];
        double* Yb[B];
        double* Y0b[B];
        double* YTb[B];
        double* PCb[B];
        double* PRb[B];
        bool check[B], kkt[B];
        double tau[B], sig[B], a1[B], a0[B];
        double d2[2 * B];
#pragma unroll
        for (int b = 0; b < B; ++b) {
            double* rec = rec_of(act[b] ? sc[b] : 0);
            Xb[b] = rec + st.sk_X;
            X0b[b] = rec + st.sk_X0;
            Ub[b] = rec + st.sk_U;
            XTb[b] = rec + st.sk_XT;
            Yb[b] = rec + st.sk_Y;
            Y0b[b] = rec + st.sk_Y0;
            YTb[b] = rec + st.sk_YT;
            PCb[b] = rec + st.sk_PC;
            PRb[b] = rec + st.sk_PR;
            const int it = itc[b];
            kkt[b] = (it % P.check_every) == 0;
            check[b] = kkt[b] || (it % P.restart_every) == 0 || it == P.max_iter - 1;
            tau[b] = eta[b] / omega[b];
            sig[b] = eta[b] * omega[b];
            a1[b] = (hk[b] + 1.0) / (hk[b] + 2.0);
            a0[b] = 1.0 / (hk[b] + 2.0);
            d2[2 * b] = d2[2 * b + 1] = 0.0;
        }
        // --- column pass: A^T y, primal step, reflected point, Halpern update of x, for
        // every active slot; the matrix slice is loaded once for all of them
        const int cq0 = SPLIT ? cb * SWAVES + wv : cw_ptr[wv];
        const int cq1 = SPLIT ? st.nsl_c : cw_ptr[wv + 1];
        const int qstep = SPLIT ? K * SWAVES : 1;
        for (int q = cq0; q < cq1; q += qstep) {
            const int sl = SPLIT ? q : cw_slc[q];
            const int j = sl * WAVE + lane;
            const int jj = j < n ? j : n - 1;
            const int p = cmap[jj];
            const double* sc4 = sh_col + 4 * (size_t)jj;
            const double ch0 = sc4[0], qh0 = sc4[1], lo0 = sc4[2], hi0 = sc4[3];
            double xj[B], x0j[B];
#pragma unroll
            for (int b = 0; b < B; ++b) {
                xj[b] = act[b] ? Xb[b][jj] : 0.0;
                x0j[b] = (act[b] && !check[b]) ? X0b[b][jj] : 0.0;
            }
            double a[B];
            sell_dot_b<B>(cs_idx, cs_val, cs_off[sl], cs_len[sl], lane, Yb, act, a);
            if (j >= n) continue;
#pragma unroll
            for (int b = 0; b < B; ++b) {
                if (!act[b]) continue;
                double ch = ch0, qh = qh0, lo = lo0, hi = hi0;
                if (p >= 0) {
                    const double* e = PCb[b] + 8 * (size_t)p + 4;
                    ch = e[0];
                    qh = e[1];
                    lo = e[2];
                    hi = e[3];
                }
                const double num = xj[b] - tau[b] * (ch - a[b]);
                const double xtj = clampd(qh != 0.0 ? num / (1.0 + tau[b] * qh) : num, lo, hi);
                Ub[b][j] = 2.0 * xtj - xj[b];
                const double d = xj[b] - xtj;
                d2[2 * b] += d * d;
                if (check[b]) XTb[b][j] = xtj;
                else Xb[b][j] = a1[b] * ((1.0 + g) * xtj - g * xj[b]) + a0[b] * x0j[b];
            }
        }
        sync();
        // --- row pass: A u, dual step, Halpern update of y
        const int rq0 = SPLIT ? cb * SWAVES + wv : rw_ptr[wv];
        const int rq1 = SPLIT ? st.nsl_r : rw_ptr[wv + 1];
        for (int q = rq0; q < rq1; q += qstep) {
            const int sl = SPLIT ? q : rw_slc[q];
            const int i = sl * WAVE + lane;
            const int ii = i < m ? i : m - 1;
            const int p = rmap[ii];
            const double* sr = sh_row + 4 * (size_t)ii;
            const double rlh0 = sr[0], ruh0 = sr[1];
            double yi[B], y0i[B];
#pragma unroll
            for (int b = 0; b < B; ++b) {
                yi[b] = act[b] ? Yb[b][ii] : 0.0;
                y0i[b] = (act[b] && !check[b]) ? Y0b[b][ii] : 0.0;
            }
            double ax[B];
            sell_dot_b<B>(rs_idx, rs_val, rs_off[sl], rs_len[sl], lane, Ub, act, ax);
            if (i >= m) continue;
#pragma unroll
            for (int b = 0; b < B; ++b) {
                if (!act[b]) continue;
                double rlh = rlh0, ruh = ruh0;
                if (p >= 0) {
                    rlh = PRb[b][4 * (size_t)p];
                    ruh = PRb[b][4 * (size_t)p + 1];
                }
                const double yti = dual_prox(yi[b] - sig[b] * ax[b], sig[b], rlh, ruh);
                const double d = yi[b] - yti;
                d2[2 * b + 1] += d * d;
                if (check[b]) YTb[b][i] = yti;
                else Yb[b][i] = a1[b] * ((1.0 + g) * yti - g * yi[b]) + a0[b] * y0i[b];
            }
        }
        bool need_any = false;
#pragma unroll
        for (int b = 0; b < B; ++b) need_any |= act[b] && (check[b] || r0[b] < 0.0);
        if (need_any) bsum(d2);
        else sync();
#pragma unroll
        for (int b = 0; b < B; ++b) {
            if (!act[b]) continue;
            if (!(check[b] || r0[b] < 0.0)) {
                ++hk[b];
                ++itc[b];
                continue;
            }
            const double r = sqrt(omega[b] * d2[2 * b] + d2[2 * b + 1] / omega[b]);
            if (r0[b] < 0.0) r0[b] = r;
            if (!check[b]) {
                ++hk[b];
                ++itc[b];
                continue;
            }
            double* rec = rec_of(sc[b]);
            // ---- KKT test on T(z) = (XT, YT)
            if (kkt[b]) {
                const bool inf = P.infeas_start >= 0 && itc[b] >= P.infeas_start;
                double o[8];
                kkt_sums(rec, inf, o);
                pobj[b] = cterm[b] + o[2];
                dobj[b] = cterm[b] + o[3];
                const bool conv =
                    sqrt(o[0]) <= P.eps_abs + P.eps_rel * (1.0 + bnorm[b]) &&
                    sqrt(o[1]) <= P.eps_abs + P.eps_rel * (1.0 + cnorm[b]) &&
                    fabs(pobj[b] - dobj[b]) <= P.eps_abs + P.eps_rel * (1.0 + fabs(pobj[b]) + fabs(dobj[b]));
                int fin = 0;
                if (conv) {
                    stat[b] = PHGPU_OPTIMAL;
                    ran_kkt[b] = true;
                    fin = 1;
                } else if (inf && is_certificate(o[4], o[5], P.eps_inf)) {
                    stat[b] = PHGPU_PRIMAL_INFEASIBLE;
                    fin = 1;
                } else if (inf && is_certificate(-o[6], o[7], P.eps_inf)) {
                    stat[b] = PHGPU_DUAL_INFEASIBLE;
                    fin = 1;
                }
                if (fin) {
                    finish(b);
                    continue;
                }
            }
            // ---- restart test (k_solve's rule), then restart or Halpern fix-up
            const int it = itc[b];
            const bool restart = (r <= P.bsuff * r0[b]) || (r <= P.bnec * r0[b] && r > rlast[b]) ||
                                 (it > 0 && hk[b] >= P.bart * it);
            rlast[b] = r;
            double* X = Xb[b];
            double* X0 = X0b[b];
            const double* XT = XTb[b];
            double* Y = Yb[b];
            double* Y0 = Y0b[b];
            const double* YT = YTb[b];
            if (restart) {
                double dd[2] = {0.0, 0.0};
                for (int j = opq(gt); j < n; j += gs) {
                    const double v = XT[j];
                    const double d = v - X0[j];
                    dd[0] += d * d;
                    X[j] = v;
                    X0[j] = v;
                }
                for (int i = opq(gt); i < m; i += gs) {
                    const double v = YT[i];
                    const double d = v - Y0[i];
                    dd[1] += d * d;
                    Y[i] = v;
                    Y0[i] = v;
                }
                bsum(dd);
                const double ddx = sqrt(dd[0]), ddy = sqrt(dd[1]);
                if (ddx > 1e-10 && ddy > 1e-10) omega[b] = clampd(sqrt(omega[b] * (ddy / ddx)), P.wmin, P.wmax);
                hk[b] = 0;
                r0[b] = -1.0;
                rlast[b] = INFINITY;
            } else {
                const double c1 = a1[b], c0 = a0[b];
                for (int j = opq(gt); j < n; j += gs) X[j] = c1 * ((1.0 + g) * XT[j] - g * X[j]) + c0 * X0[j];
                for (int i = opq(gt); i < m; i += gs) Y[i] = c1 * ((1.0 + g) * YT[i] - g * Y[i]) + c0 * Y0[i];
                sync();
                ++hk[b];
            }
            ++itc[b];
            if (itc[b] >= P.max_iter) finish(b);
        }
    }
}

// ------------------------------------------------------------------ shared-matrix setup
// One scaled copy of A for all scenarios: Ruiz (max) passes + one Pock-Chambolle (sum)
// pass, the CSC copy and ||A_scaled||_2 by power iteration (k_setup's algorithm, with
// rows / columns / nonzeros spread over threads instead of one lane per scenario).
__global__ void __launch_bounds__(256) k_sh_take0(const double* __restrict__ in, int64_t S, int K,
                                                  double* __restrict__ out) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < K) out[k] = in[(size_t)k * (size_t)S];
}

__global__ void __launch_bounds__(256) k_sh_init(ph_data st) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < st.nnz) st.Ah_csr[k] = st.A[k];
    if (k < st.m) st.Dr[k] = 1.0;
    if (k < st.n) st.Dc[k] = 1.0;
}

__global__ void __launch_bounds__(256) k_sh_rowfac(ph_data st, int pc, double* __restrict__ rf) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= st.m) return;
    double a = 0.0;
    for (int k = st.row_ptr[i]; k < st.row_ptr[i + 1]; ++k) {
        const double v = fabs(st.Ah_csr[k]);
        a = pc ? a + v : fmax(a, v);
    }
    rf[i] = a > 0.0 ? 1.0 / sqrt(a) : 1.0;
}

__global__ void __launch_bounds__(256) k_sh_colfac(ph_data st, int pc, double* __restrict__ cf) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= st.n) return;
    double a = 0.0;
    for (int kc = st.col_ptr[j]; kc < st.col_ptr[j + 1]; ++kc) {
        const double v = fabs(st.Ah_csr[st.perm[kc]]);
        a = pc ? a + v : fmax(a, v);
    }
    cf[j] = a > 0.0 ? 1.0 / sqrt(a) : 1.0;
}

__global__ void __launch_bounds__(256) k_sh_apply(ph_data st, const double* __restrict__ rf,
                                                  const double* __restrict__ cf) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < st.nnz) st.Ah_csr[k] *= rf[st.row_of[k]] * cf[st.col_idx[k]];
    if (k < st.m) st.Dr[k] *= rf[k];
    if (k < st.n) st.Dc[k] *= cf[k];
}

__global__ void __launch_bounds__(256) k_sh_csc(ph_data st) {
    const int kc = blockIdx.x * blockDim.x + threadIdx.x;
    if (kc < st.nnz) st.Ah_csc[kc] = st.Ah_csr[st.perm[kc]];
}

__global__ void __launch_bounds__(256) k_sh_vinit(ph_data st, double* __restrict__ v) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < st.n) v[j] = 1.0 + 0.5 * sin(1.7 * j);
}

__global__ void __launch_bounds__(256) k_sh_rowmv(ph_data st, const double* __restrict__ v,
                                                  double* __restrict__ w) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= st.m) return;
    double a = 0.0;
    for (int k = st.row_ptr[i]; k < st.row_ptr[i + 1]; ++k) a += st.Ah_csr[k] * v[st.col_idx[k]];
    w[i] = a;
}

// u = A^T w and per-block partial sums of u^2
__global__ void __launch_bounds__(256) k_sh_colmv(ph_data st, const double* __restrict__ w,
                                                  double* __restrict__ u, double* __restrict__ part) {
    __shared__ double sh[256];
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    double a = 0.0;
    if (j < st.n) {
        for (int kc = st.col_ptr[j]; kc < st.col_ptr[j + 1]; ++kc) a += st.Ah_csc[kc] * w[st.row_idx[kc]];
        u[j] = a;
    }
    sh[threadIdx.x] = a * a;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}

// out[0] = sqrt(sum part[0..nb))  (one block, fixed order)
__global__ void __launch_bounds__(256) k_sh_norm(const double* __restrict__ part, int nb, double* __restrict__ out) {
    __shared__ double sh[256];
    double a = 0.0;
    for (int b = threadIdx.x; b < nb; b += 256) a += part[b];
    sh[threadIdx.x] = a;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = sqrt(sh[0]);
}

__global__ void __launch_bounds__(256) k_sh_normalize(ph_data st, const double* __restrict__ u,
                                                      const double* __restrict__ nv, double* __restrict__ v) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const double inv = nv[0] > 0.0 ? 1.0 / nv[0] : 0.0;
    if (j < st.n) v[j] = u[j] * inv;
}

__global__ void k_sh_finish_norm(ph_data st) {
    // power iteration under-estimates ||A||_2: 1% margin (k_setup)
    const double lam = st.sh_norm[3];
    st.sh_norm[0] = lam > 0.0 ? 1.01 * sqrt(lam) : 1.0;
}

// shared base of the per-column / per-row data: scenario 0's values, scaled
__global__ void __launch_bounds__(256) k_sh_base(ph_data st, const double* __restrict__ c,
                                                 const double* __restrict__ q, const double* __restrict__ lb,
                                                 const double* __restrict__ ub, const double* __restrict__ rl,
                                                 const double* __restrict__ ru) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t S = (size_t)st.S;
    if (k < st.n) {
        const double d = st.Dc[k];
        const size_t o = (size_t)k * S;
        st.sh_col[4 * (size_t)k + 0] = d * c[o];
        st.sh_col[4 * (size_t)k + 1] = q ? d * d * q[o] : 0.0;
        st.sh_col[4 * (size_t)k + 2] = lb[o] / d;
        st.sh_col[4 * (size_t)k + 3] = ub[o] / d;
    }
    if (k < st.m) {
        const double d = st.Dr[k];
        const size_t o = (size_t)k * S;
        st.sh_row[4 * (size_t)k + 0] = rl[o] * d;
        st.sh_row[4 * (size_t)k + 1] = ru[o] * d;
        st.sh_row[4 * (size_t)k + 2] = rl[o];
        st.sh_row[4 * (size_t)k + 3] = ru[o];
    }
}

// flag[k] = 1 if any of the (up to 4) [K][S] arrays differs from scenario 0 at k; one
// wave per k, lanes over scenarios (coalesced)
__global__ void __launch_bounds__(256) k_sh_vary(const double* __restrict__ a, const double* __restrict__ b,
                                                 const double* __restrict__ c, const double* __restrict__ d,
                                                 int K, int64_t S, int32_t* __restrict__ flag) {
    const int k = blockIdx.x * (256 / WAVE) + threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    if (k >= K) return;
    const size_t o = (size_t)k * (size_t)S;
    const double* arr[4] = {a, b, c, d};
    int diff = 0;
    for (int t = 0; t < 4; ++t) {
        const double* p = arr[t];
        if (!p) continue;
        const double v0 = p[o];
        for (int64_t s = lane; s < S; s += WAVE)
            if (!(p[o + s] == v0)) diff = 1;
    }
    diff = __any(diff);
    if (lane == 0) flag[k] = diff;
}

// per-scenario column / row data into the records: PC = {c, q, lb, ub, ch, qh, lbh, ubh}
// (ch / qh are filled per solve), PR = {rlh, ruh, rl, ru}
__global__ void __launch_bounds__(256) k_sh_fill(ph_data st, const double* __restrict__ c,
                                                 const double* __restrict__ q, const double* __restrict__ lb,
                                                 const double* __restrict__ ub, const double* __restrict__ rl,
                                                 const double* __restrict__ ru) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t per = (int64_t)st.np + st.nr;
    if (per == 0 || t >= per * st.S) return;
    const int64_t s = t / per;
    const int p = (int)(t - s * per);
    const size_t S = (size_t)st.S;
    double* rec = st.sk + (size_t)s * (size_t)st.sk_stride;
    if (p < st.np) {
        const int j = st.pcol[p];
        const size_t o = (size_t)j * S + (size_t)s;
        const double d = st.Dc[j];
        double* e = rec + st.sk_PC + 8 * (size_t)p;
        e[0] = c[o];
        e[1] = q ? q[o] : 0.0;
        e[2] = lb[o];
        e[3] = ub[o];
        e[4] = d * c[o];
        e[5] = q ? d * d * q[o] : 0.0;
        e[6] = lb[o] / d;
        e[7] = ub[o] / d;
    } else {
        const int r = p - st.np;
        const int i = st.prow[r];
        const size_t o = (size_t)i * S + (size_t)s;
        const double d = st.Dr[i];
        double* e = rec + st.sk_PR + 4 * (size_t)r;
        e[0] = rl[o] * d;
        e[1] = ru[o] * d;
        e[2] = rl[o];
        e[3] = ru[o];
    }
}

// norms of the shared part: sh_norm[1] = sum over shared columns of c^2, sh_norm[2] =
// sum over shared rows of the finite row bounds squared (one block, fixed order)
__global__ void __launch_bounds__(256) k_sh_normbase(ph_data st, const double* __restrict__ c,
                                                     const double* __restrict__ rl, const double* __restrict__ ru) {
    __shared__ double sh[2][256];
    const size_t S = (size_t)st.S;
    double a = 0.0, b = 0.0;
    for (int j = threadIdx.x; j < st.n; j += 256)
        if (st.cmap[j] < 0) {
            const double v = c[(size_t)j * S];
            a += v * v;
        }
    for (int i = threadIdx.x; i < st.m; i += 256)
        if (st.rmap[i] < 0) {
            const double lo = rl[(size_t)i * S], hi = ru[(size_t)i * S];
            if (isfinite(lo)) b += lo * lo;
            if (isfinite(hi) && hi != lo) b += hi * hi;
        }
    sh[0][threadIdx.x] = a;
    sh[1][threadIdx.x] = b;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            sh[0][threadIdx.x] += sh[0][threadIdx.x + o];
            sh[1][threadIdx.x] += sh[1][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        st.sh_norm[1] = sh[0][0];
        st.sh_norm[2] = sh[1][0];
    }
}

__global__ void __launch_bounds__(256) k_sh_fill_omega(pdhg_view st) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s < st.S) st.omega[s] = 1.0;
}

// phgpu_fix_nonants on a shared-matrix handle: the working bounds live in PC
__global__ void __launch_bounds__(256) k_fix_nonants_sh(ph_data st, const double* __restrict__ xfix) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)st.nn * st.S) return;
    const int64_t s = t / st.nn;
    const int k = (int)(t - s * st.nn);
    const int j = st.nonant_col[k];
    const int p = st.cmap[j];
    double* e = st.sk + (size_t)s * (size_t)st.sk_stride + st.sk_PC + 8 * (size_t)p;
    const double d = st.Dc[j];
    const double xv = xfix ? xfix[(size_t)k * (size_t)st.S + (size_t)s] : NAN;
    if (!isnan(xv)) {
        const double v = fmin(fmax(xv, e[2]), e[3]);
        e[6] = v / d;
        e[7] = v / d;
    } else {
        e[6] = e[2] / d;
        e[7] = e[3] / d;
    }
}

// values of a sliced-ELL copy from the scaled CSR / CSC values (pads: 0)
__global__ void __launch_bounds__(256) k_sh_sell_vals(const int32_t* __restrict__ src, const double* __restrict__ a,
                                                      int tot, double* __restrict__ val) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < tot) val[e] = src[e] >= 0 ? a[src[e]] : 0.0;
}

// longest-first queue order for k_solve_stream: rank of scenario s by the previous
// solve's iterations (descending, ties by index) -- a permutation; O(S^2) compares, used
// up to STREAM_ORDER_MAX scenarios
#define STREAM_ORDER_MAX 16384
__global__ void __launch_bounds__(256) k_stream_order(pdhg_view st) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= st.S) return;
    const int S = (int)st.S;
    const int mine = st.sk_iters[s];
    int r = 0;
    for (int t = 0; t < S; ++t) {
        const int o = st.sk_iters[t];
        r += (o > mine) || (o == mine && t < s);
    }
    st.sk_order[r] = s;
}

__global__ void __launch_bounds__(256) k_stream_order_identity(pdhg_view st) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < st.S) st.sk_order[s] = s;
}
