// FWPH (mpisppy/fwph/fwph.py): the half of Boland et al.'s Algorithm 2 that is not an LP solve
// -- per scenario a growing set of columns and a small convex QP over their convex hull --
// for all local scenarios in one pass (phgpu_fwph_*, include/phgpu.h).  Included by phgpu.hip
// after ph_fixer.inc.
//
// The store is the handle's (fwph_store, allocated by phgpu_fwph_init): scenario-fastest like
// every per-scenario array, element (i, s) of an i-indexed quantity at [i * S + s].  One lane
// per scenario; everything a lane indexes dynamically (weights, gradient, the Gram matrix and
// its Cholesky factor) lives in the store, so the kernels keep scalars only and use no scratch.
//
// The QP of one scenario, with K columns X_j in R^nn of cost f_j:
//   min_a  1/2 a'G a + lin'a   on the simplex,   G = X' diag(rho) X,  lin_j = f_j + X_j.(W - rho xbar)
// G is singular whenever a column repeats or K > nn + 1, so the weights are not unique; x(a)
// and phi are.  It is solved by an active set on G in the manner of Wolfe's nearest-point
// method: the support P is kept affinely independent, so that H_PP = G_PP + mu 11' (the same
// problem on sum a = 1) has a Cholesky factor.  A column whose pivot vanishes lies in the affine
// hull of the support before it: weight moves along the null direction (x(a) fixed, the cost
// linear) until an entry leaves.  Finite, and exact up to rounding.
#define FW_T 64          // one wave per block: lanes of one wave diverge in the QP, waves do not wait for each other
#define FW_PIV 1e-11     // a pivot below this fraction of its diagonal: the column is affinely dependent
#define FW_GAP 1e-14     // the QP stops at gap <= FW_GAP * scale

struct fwph_store {
    int max_cols;
    double* X;                 // [max_cols][nn][S] columns (nonant values, the layout of W per column)
    double *f, *a;             // [max_cols][S] column costs c.x + obj_const, weights
    double *G, *L;             // [max_cols (max_cols + 1) / 2][S] packed lower: Gram matrix, Cholesky work
    double *lin, *u, *v;       // [max_cols][S] work vectors of the QP
    double* xq;                // [nn][S] the QP point
    double* phi;               // [S]
    int32_t *ncols, *active, *last, *nit;  // [S] columns held, active flag, newest column, inner iterations so far
    int32_t* acc;              // [4] {active, gamma < -tol, not OPTIMAL, ticket} of a pass in flight (zero between)
};

#define FWI(i) ((size_t)(i) * (size_t)S + (size_t)s)
#define FWP(i, j) ((size_t)((i) * ((i) + 1) / 2 + (j)) * (size_t)S + (size_t)s)
#define FWX(j, k) (((size_t)(j) * (size_t)nn + (size_t)(k)) * (size_t)S + (size_t)s)

// row j of the Gram matrix against columns 0..K-1 (and the diagonal), rho-weighted
__device__ __forceinline__ void fw_gram_row(const fwph_store& fw, const double* __restrict__ rho, int nn, int64_t S,
                                            int64_t s, int j, int K) {
    for (int i = 0; i < K; ++i) {
        double t = 0.0;
        for (int k = 0; k < nn; ++k) t += rho[FWI(k)] * fw.X[FWX(j, k)] * fw.X[FWX(i, k)];
        if (i <= j) fw.G[FWP(j, i)] = t;
        else fw.G[FWP(i, j)] = t;
    }
}

__device__ __forceinline__ double fw_G(const fwph_store& fw, int64_t S, int64_t s, int i, int j) {
    return i >= j ? fw.G[FWP(i, j)] : fw.G[FWP(j, i)];
}

// xq = sum a_j X_j, phi = sum a_j f_j over the K columns; xq also into the nonant columns of xqx
__device__ __forceinline__ void fw_point(const ph_tree& st, const fwph_store& fw, int64_t s, int K,
                                         double* __restrict__ xq_out, double* __restrict__ xqx) {
    const int64_t S = st.S;
    const int nn = st.nn;
    double phi = 0.0;
    for (int j = 0; j < K; ++j) phi += fw.a[FWI(j)] * fw.f[FWI(j)];
    fw.phi[s] = phi;
    for (int k = 0; k < nn; ++k) {
        double t = 0.0;
        for (int j = 0; j < K; ++j) {
            const double aj = fw.a[FWI(j)];
            if (aj != 0.0) t += aj * fw.X[FWX(j, k)];
        }
        fw.xq[FWI(k)] = t;
        if (xq_out) xq_out[FWI(k)] = t;
        if (xqx) xqx[FWI(st.nonant_col[k])] = t;
    }
}

// The simplex QP of scenario s over its K columns (G and lin in the store): the weights in
// fw.a, exactly 0 off the final support, summing to 1.  Cold start from the best single column,
// so the result depends on the columns only.
__device__ void fw_qp(const fwph_store& fw, int64_t S, int64_t s, int K) {
    // the linear term shifted by its minimum (a constant on the simplex) and the scales
    double lmin = INFINITY, mu = 0.0;
    for (int j = 0; j < K; ++j) {
        lmin = fmin(lmin, fw.lin[FWI(j)]);
        mu = fmax(mu, fw.G[FWP(j, j)]);
    }
    if (!(mu > 0.0)) mu = 1.0;
    int j0 = 0;
    double best = INFINITY;
    for (int j = 0; j < K; ++j) {
        const double l = fw.lin[FWI(j)] - lmin;
        fw.lin[FWI(j)] = l;
        fw.a[FWI(j)] = 0.0;
        const double q = l + 0.5 * fw.G[FWP(j, j)];
        if (q < best) {
            best = q;
            j0 = j;
        }
    }
    fw.a[FWI(j0)] = 1.0;
    const double tol = FW_GAP * fmax(1.0, fmax(fabs(lmin), mu));
    unsigned long long P = 1ull << j0;
    for (int major = 0; major < 4 * K + 16; ++major) {
        // g = G a + lin, the gap g.a - min g and the entering column
        double ga = 0.0, gmin = INFINITY;
        int js = 0;
        for (int j = 0; j < K; ++j) {
            double t = fw.lin[FWI(j)];
            for (unsigned long long m = P; m; m &= m - 1) {
                const int i = __builtin_ctzll(m);
                t += fw_G(fw, S, s, j, i) * fw.a[FWI(i)];
            }
            ga += fw.a[FWI(j)] * t;
            if (t < gmin) {
                gmin = t;
                js = j;
            }
        }
        if (ga - gmin <= tol || ((P >> js) & 1)) break;
        P |= 1ull << js;
        for (int minor = 0; minor < 2 * K + 8; ++minor) {
            // Cholesky of H_PP = G_PP + mu 11' in index order; dep: the first column whose pivot vanishes
            int dep = -1;
            for (unsigned long long mi = P; mi && dep < 0; mi &= mi - 1) {
                const int i = __builtin_ctzll(mi);
                const unsigned long long row = P & ((2ull << i) - 1);
                for (unsigned long long mj = row; mj; mj &= mj - 1) {
                    const int j = __builtin_ctzll(mj);
                    double t = fw_G(fw, S, s, i, j) + mu;
                    for (unsigned long long mk = P & ((1ull << j) - 1); mk; mk &= mk - 1) {
                        const int k = __builtin_ctzll(mk);
                        t -= fw.L[FWP(i, k)] * fw.L[FWP(j, k)];
                    }
                    if (j < i) fw.L[FWP(i, j)] = t / fw.L[FWP(j, j)];
                    else if (t <= FW_PIV * (fw.G[FWP(i, i)] + mu)) dep = i;
                    else fw.L[FWP(i, i)] = sqrt(t);
                }
            }
            int drop = -1;
            if (dep >= 0) {
                // X_dep = sum_B c_i X_i with sum c = 1 (B: the support below dep): L_BB' c = L(dep, B)
                const unsigned long long B = P & ((1ull << dep) - 1);
                double slope = fw.lin[FWI(dep)];
                for (unsigned long long mi = B; mi;) {
                    const int i = 63 - __builtin_clzll(mi);
                    mi &= ~(1ull << i);
                    double t = fw.L[FWP(dep, i)];
                    for (unsigned long long mk = B & ~((2ull << i) - 1); mk; mk &= mk - 1) {
                        const int k = __builtin_ctzll(mk);
                        t -= fw.L[FWP(k, i)] * fw.u[FWI(k)];
                    }
                    t /= fw.L[FWP(i, i)];
                    fw.u[FWI(i)] = t;
                    slope -= t * fw.lin[FWI(i)];
                }
                // weight to dep (slope < 0) or away from it, x(a) unchanged, until an entry reaches 0
                const double sg = slope < 0.0 ? 1.0 : -1.0;
                double tmax = sg > 0.0 ? INFINITY : fw.a[FWI(dep)];
                drop = sg > 0.0 ? -1 : dep;
                for (unsigned long long mi = B; mi; mi &= mi - 1) {
                    const int i = __builtin_ctzll(mi);
                    const double d = -sg * fw.u[FWI(i)];
                    if (d < 0.0) {
                        const double r = fw.a[FWI(i)] / -d;
                        if (r < tmax) {
                            tmax = r;
                            drop = i;
                        }
                    }
                }
                if (drop < 0) {  // (cannot happen: sum c = 1 has a positive entry)
                    drop = dep;
                    tmax = 0.0;
                }
                for (unsigned long long mi = B; mi; mi &= mi - 1) {
                    const int i = __builtin_ctzll(mi);
                    fw.a[FWI(i)] = fmax(0.0, fw.a[FWI(i)] - tmax * sg * fw.u[FWI(i)]);
                }
                fw.a[FWI(dep)] = fmax(0.0, fw.a[FWI(dep)] + tmax * sg);
            } else {
                // z = argmin on the affine hull of P: H u = 1, H v = lin, z = -v - lam u
                double su = 0.0, sv = 0.0;
                for (unsigned long long mi = P; mi; mi &= mi - 1) {
                    const int i = __builtin_ctzll(mi);
                    double tu = 1.0, tv = fw.lin[FWI(i)];
                    for (unsigned long long mk = P & ((1ull << i) - 1); mk; mk &= mk - 1) {
                        const int k = __builtin_ctzll(mk);
                        const double l = fw.L[FWP(i, k)];
                        tu -= l * fw.u[FWI(k)];
                        tv -= l * fw.v[FWI(k)];
                    }
                    const double d = fw.L[FWP(i, i)];
                    fw.u[FWI(i)] = tu / d;
                    fw.v[FWI(i)] = tv / d;
                }
                for (unsigned long long mi = P; mi;) {
                    const int i = 63 - __builtin_clzll(mi);
                    mi &= ~(1ull << i);
                    double tu = fw.u[FWI(i)], tv = fw.v[FWI(i)];
                    for (unsigned long long mk = P & ~((2ull << i) - 1); mk; mk &= mk - 1) {
                        const int k = __builtin_ctzll(mk);
                        const double l = fw.L[FWP(k, i)];
                        tu -= l * fw.u[FWI(k)];
                        tv -= l * fw.v[FWI(k)];
                    }
                    const double d = fw.L[FWP(i, i)];
                    tu /= d;
                    tv /= d;
                    fw.u[FWI(i)] = tu;
                    fw.v[FWI(i)] = tv;
                    su += tu;
                    sv += tv;
                }
                const double lam = -(1.0 + sv) / su;
                double theta = 1.0, zs = 0.0;
                for (unsigned long long mi = P; mi; mi &= mi - 1) {
                    const int i = __builtin_ctzll(mi);
                    const double z = -fw.v[FWI(i)] - lam * fw.u[FWI(i)];
                    fw.v[FWI(i)] = z;
                    zs += z;
                    if (!(z > 0.0)) {
                        const double ai = fw.a[FWI(i)];
                        const double r = ai / (ai - z);
                        if (!(r >= theta)) {  // (also a NaN ratio: 0 / 0)
                            theta = r == r ? r : 0.0;
                            drop = i;
                        }
                    }
                }
                if (drop < 0) {
                    for (unsigned long long mi = P; mi; mi &= mi - 1) {
                        const int i = __builtin_ctzll(mi);
                        fw.a[FWI(i)] = fw.v[FWI(i)] / zs;
                    }
                    break;
                }
                for (unsigned long long mi = P; mi; mi &= mi - 1) {
                    const int i = __builtin_ctzll(mi);
                    const double ai = fw.a[FWI(i)];
                    fw.a[FWI(i)] = fmax(0.0, ai + theta * (fw.v[FWI(i)] - ai));
                }
            }
            fw.a[FWI(drop)] = 0.0;
            P &= ~(1ull << drop);
        }
    }
    // exactly on the simplex
    double sa = 0.0;
    for (unsigned long long mi = P; mi; mi &= mi - 1) sa += fw.a[FWI(__builtin_ctzll(mi))];
    for (unsigned long long mi = P; mi; mi &= mi - 1) {
        const int i = __builtin_ctzll(mi);
        fw.a[FWI(i)] /= sa;
    }
}

// lin_j = f_j + X_j.(W - rho xbar) for the K columns of scenario s
__device__ __forceinline__ void fw_lin(const fwph_store& fw, int nn, int64_t S, int64_t s, int K,
                                       const double* __restrict__ W, const double* __restrict__ rho,
                                       const double* __restrict__ xbar) {
    for (int j = 0; j < K; ++j) {
        double t = fw.f[FWI(j)];
        for (int k = 0; k < nn; ++k) t += fw.X[FWX(j, k)] * (W[FWI(k)] - rho[FWI(k)] * xbar[FWI(k)]);
        fw.lin[FWI(j)] = t;
    }
}

// phgpu_fwph_load: the store of every scenario from K given columns, costs and weights
__global__ void __launch_bounds__(FW_T)
k_fw_load(ph_tree st, fwph_store fw, int K, const double* __restrict__ X, const double* __restrict__ f,
          const double* __restrict__ a, const double* __restrict__ rho, double* __restrict__ xq,
          double* __restrict__ xqx) {
    const int64_t S = st.S;
    const int nn = st.nn;
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    for (int j = 0; j < K; ++j) {
        for (int k = 0; k < nn; ++k) fw.X[FWX(j, k)] = X[FWX(j, k)];
        fw.f[FWI(j)] = f[FWI(j)];
        fw.a[FWI(j)] = a ? a[FWI(j)] : (j == 0 ? 1.0 : 0.0);
    }
    for (int j = 0; j < K; ++j) fw_gram_row(fw, rho, nn, S, s, j, j + 1);
    fw.ncols[s] = K;
    fw.active[s] = 1;
    fw.last[s] = K - 1;
    fw.nit[s] = 0;
    fw_point(st, fw, s, K, xq, xqx);
}

// phgpu_fwph_export: the store into the caller's arrays (each may be null)
__global__ void __launch_bounds__(FW_T)
k_fw_export(ph_tree st, fwph_store fw, double* __restrict__ X, double* __restrict__ f, double* __restrict__ a,
            int32_t* __restrict__ ncols, double* __restrict__ xq, double* __restrict__ phi,
            int32_t* __restrict__ active, int32_t* __restrict__ nit) {
    const int64_t S = st.S;
    const int nn = st.nn;
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const int K = fw.ncols[s];
    for (int j = 0; j < fw.max_cols; ++j) {
        const bool in = j < K;
        if (X)
            for (int k = 0; k < nn; ++k) X[FWX(j, k)] = in ? fw.X[FWX(j, k)] : 0.0;
        if (f) f[FWI(j)] = in ? fw.f[FWI(j)] : 0.0;
        if (a) a[FWI(j)] = in ? fw.a[FWI(j)] : 0.0;
    }
    if (ncols) ncols[s] = K;
    if (xq)
        for (int k = 0; k < nn; ++k) xq[FWI(k)] = fw.xq[FWI(k)];
    if (phi) phi[s] = fw.phi[s];
    if (active) active[s] = fw.active[s];
    if (nit) nit[s] = fw.nit[s];
}

// fwph.py:227-247: What = W + rho (src - xbar), src = (1 - alpha) xbar + alpha xq at t = 0, else
// xq; one nonant per grid row.  At t = 0 every scenario becomes active.
__global__ void __launch_bounds__(GR_T)
k_fw_direction(ph_tree st, fwph_store fw, int t0, double alpha, const double* __restrict__ W,
               const double* __restrict__ rho, const double* __restrict__ xbar, double* __restrict__ What) {
    const int64_t S = st.S;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int k = blockIdx.y; k < st.nn; k += gridDim.y) {
        for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < S; s += stride) {
            const double xb = xbar[FWI(k)], xqk = fw.xq[FWI(k)];
            const double src = t0 ? (1.0 - alpha) * xb + alpha * xqk : xqk;
            What[FWI(k)] = W[FWI(k)] + rho[FWI(k)] * (src - xb);
            if (t0 && k == 0) fw.active[s] = 1;
        }
    }
}

// fwph.py:256-292 for every active scenario: Gamma, the new column, the QP, the break test; and
// the three counts of the pass, stored last by the block with the last ticket.
__global__ void __launch_bounds__(FW_T)
k_fw_column(ph_tree st, fwph_store fw, phgpu_fwph_params prm, int t0, const double* __restrict__ x,
            const double* __restrict__ obj, const double* __restrict__ bound, const int32_t* __restrict__ status,
            const double* __restrict__ W, const double* __restrict__ What, const double* __restrict__ rho,
            const double* __restrict__ xbar, double* __restrict__ gamma, double* __restrict__ dual_bound,
            int32_t* __restrict__ ncols, double* __restrict__ xq, double* __restrict__ xqx,
            int32_t* __restrict__ counts) {
    const int64_t S = st.S;
    const int nn = st.nn;
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = s < S;
    const bool act = in && fw.active[s] != 0;
    const bool opt = act && status[s] == PHGPU_OPTIMAL;
    bool still = false, neg = false;
    if (act && t0) dual_bound[s] = bound[s];
    if (opt) {
        int K = fw.ncols[s];
        // val0 = the LP's objective, val1 = the same objective at the QP point before this QP
        double wx = 0.0, wq = 0.0;
        for (int k = 0; k < nn; ++k) {
            const double wh = What[FWI(k)];
            wx += wh * x[FWI(st.nonant_col[k])];
            wq += wh * fw.xq[FWI(k)];
        }
        const double val0 = obj[s], val1 = fw.phi[s] + wq;
        const double gm = fabs(val0) > 1e-9 ? (val1 - val0) / fabs(val0) : val1 - val0;
        // the column's slot: the next free one, or the smallest weight but the newest column's
        int j = K;
        if (K < fw.max_cols) {
            ++K;
        } else {
            const int newest = fw.last[s];
            double amin = INFINITY;
            for (int i = 0; i < K; ++i) {
                const double ai = fw.a[FWI(i)];
                if (i != newest && ai < amin) {
                    amin = ai;
                    j = i;
                }
            }
        }
        for (int k = 0; k < nn; ++k) fw.X[FWX(j, k)] = x[FWI(st.nonant_col[k])];
        fw.f[FWI(j)] = val0 - wx;
        fw.last[s] = j;
        fw.ncols[s] = K;
        fw.nit[s] += 1;
        fw_gram_row(fw, rho, nn, S, s, j, K);
        fw_lin(fw, nn, S, s, K, W, rho, xbar);
        fw_qp(fw, S, s, K);
        fw_point(st, fw, s, K, xq, xqx);
        gamma[s] = gm;
        ncols[s] = K;
        neg = gm < -prm.stop_check_tol;
        still = !(gm < prm.conv_thresh);
        fw.active[s] = still ? 1 : 0;
    } else if (act) {
        fw.active[s] = 0;  // no column, the QP point kept; the pass reports it
    }
    const int c0 = (int)__popcll(__ballot(still));
    const int c1 = (int)__popcll(__ballot(neg));
    const int c2 = (int)__popcll(__ballot(act && !opt));
    if (threadIdx.x == 0) {
        int o0 = c0 ? __hip_atomic_fetch_add(&fw.acc[0], c0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
        int o1 = c1 ? __hip_atomic_fetch_add(&fw.acc[1], c1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
        int o2 = c2 ? __hip_atomic_fetch_add(&fw.acc[2], c2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
        asm volatile("" ::"v"(o0), "v"(o1), "v"(o2) : "memory");
        const int tk = __hip_atomic_fetch_add(&fw.acc[3], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (tk == (int)gridDim.x - 1) {
            int4 r;
            r.x = __hip_atomic_exchange(&fw.acc[0], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            r.y = __hip_atomic_exchange(&fw.acc[1], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            r.z = __hip_atomic_exchange(&fw.acc[2], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            r.w = 0;
            ticket_reset(&fw.acc[3]);
            *reinterpret_cast<int4*>(counts) = r;  // one store: all four words or none
        }
    }
}

// fwph.py:528-547: out[0] = sum_s prob_s sum_k (xq - xbar)^2 over the local scenarios.  Every
// thread adds its scenarios in index order, every block its threads in a fixed order, the block
// with the last ticket the blocks' sums by a fixed tree (as k_w_diff): the same bits on every run.
__global__ void __launch_bounds__(GR_T)
k_fw_diff(ph_tree st, fwph_store fw, const double* __restrict__ xbar, double* __restrict__ bpart,
          int32_t* __restrict__ cnt, double* __restrict__ out) {
    __shared__ double red[GR_T / WAVE];
    __shared__ double fin[WD_BLOCKS];
    const int64_t S = st.S;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    double acc = 0.0;
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < S; s += stride) {
        double d = 0.0;
        for (int k = 0; k < st.nn; ++k) {
            const double e = fw.xq[FWI(k)] - xbar[FWI(k)];
            d += e * e;
        }
        acc += st.prob[s] * d;
    }
    const double b[1] = {block_sum_fixed(acc, red)};
    const int nblk = (int)gridDim.x;
    if (!last_block_publish(b, bpart, cnt, (int)blockIdx.x, nblk)) return;
    for (int u = threadIdx.x; u < WD_BLOCKS; u += blockDim.x) fin[u] = u < nblk ? agent_read(&bpart[u]) : 0.0;
    __syncthreads();
    for (int o = WD_BLOCKS / 2; o > 0; o >>= 1) {
        for (int u = threadIdx.x; u < o; u += blockDim.x) fin[u] += fin[u + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[0] = fin[0];
        ticket_reset(cnt);
    }
}
