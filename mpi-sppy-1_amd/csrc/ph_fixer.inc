// Fixer (mpisppy/extensions/fixer.py): the convergence counters, the decisions and the bound
// rewrite of every local (nonant, scenario) in one pass (phgpu_fixer_step, include/phgpu.h).
// Included by phgpu.hip after ph_reduce.inc.
//
// One nonant per grid row, lanes along the scenarios: count / fixval / lb / ub are coalesced,
// th and the lags are uniform per row.  A wave stays whole through the scenario loop (its
// trip count depends on the wave's first scenario only), so that it can vote: where all its
// scenarios share the node at the nonant's depth, the node index is taken from the first
// lane -- a wave-uniform value, so x̄ and E[x²] come by scalar loads -- and the wave adds its
// newly fixed entries to the node entry's count with one integer atomic (ballot + popcount);
// a wave that spans nodes loads and adds per lane.  Integer sums do not depend on the order:
// the same inputs give the same bits.  Stores happen only where something changed.
#define FX_T 256
#define FX_BLOCKS 1024  // blocks per nonant at most (a row's blocks stride over the scenarios)

// local scenarios of every node entry (nloc[num_nodes * nlen_max], cleared by the caller); the
// grid and the wave vote of k_fixer_step: one atomic per wave where its scenarios share a node
__global__ void __launch_bounds__(FX_T) k_fixer_nloc(ph_tree st, int32_t* __restrict__ nloc) {
    const int64_t S = st.S;
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int k = blockIdx.y; k < st.nn; k += gridDim.y) {
        const int d = st.nonant_depth[k], off = st.nonant_off[k];
        for (int64_t base = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x - lane); base < S; base += stride) {
            const int64_t s = base + lane;
            const bool act = s < S;
            const int g = st.node_of[(int64_t)d * S + (act ? s : S - 1)];
            const int gu = __builtin_amdgcn_readfirstlane(g);
            const unsigned long long m = __ballot(act);
            if (__all(g == gu)) {
                if (lane == 0) atomicAdd(&nloc[(int64_t)gu * st.nlen_max + off], (int)__popcll(m));
            } else if (act) {
                atomicAdd(&nloc[(int64_t)g * st.nlen_max + off], 1);
            }
        }
    }
}

// the rule for one entry (fixer.py:114-128 and 156-189 / 248-279): the new counter in c and
// true with the value to fix at in v.  The products are rounded on their own (no fused
// multiply-add), as the reference's xb * xb - xsq and tolval * tolval are.
__device__ __forceinline__ bool fixer_rule(bool iter0, double xb, double xsq, double th, int nb, int lbl, int ubl,
                                           double l, double u, double boundtol, int& c, double& v) {
    const double diff = __dmul_rn(xb, xb) - xsq;
    const double t2 = __dmul_rn(th, th);
    if (iter0) {
        // fixer.py:169: non-strict, the lags only tested for None, the counters left alone
        if (-diff > t2 || diff > t2) return false;
        if (nb >= 0) v = xb;
        else if (lbl >= 0 && xb - l < boundtol) v = l;
        else if (ubl >= 0 && u - xb < boundtol) v = u;
        else return false;
        return true;
    }
    c = (-diff < t2 && diff < t2) ? c + 1 : 0;  // fixer.py:124-128: strict
    if (c <= 0) return false;
    if (nb >= 0 && nb <= c) v = xb;
    else if (lbl >= 0 && lbl < c && xb - l < boundtol) v = l;
    else if (ubl >= 0 && ubl < c && u - xb < boundtol) v = u;
    else return false;
    return true;
}

template <bool SHARED>
__global__ void __launch_bounds__(FX_T)
k_fixer_step(ph_data st, phgpu_fixer_params prm, const double* __restrict__ node_buf,
             const double* __restrict__ th, const int32_t* __restrict__ nb, const int32_t* __restrict__ lbl,
             const int32_t* __restrict__ ubl, int32_t* __restrict__ count, double* __restrict__ fixval,
             int32_t* __restrict__ acc, unsigned long long* __restrict__ totals) {
    const int64_t S = st.S;
    const int nl = st.nlen_max;
    const int64_t half = (int64_t)st.num_nodes * nl;
    const int lane = threadIdx.x & (WAVE - 1);
    const bool iter0 = prm.iter0 != 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int arrived = 0;
    for (int k = blockIdx.y; k < st.nn; k += gridDim.y) {
        const int d = st.nonant_depth[k], off = st.nonant_off[k], j = st.nonant_col[k];
        const double thk = th[k];
        const int nbk = nb[k], lbk = lbl[k], ubk = ubl[k];
        for (int64_t base = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x - lane); base < S; base += stride) {
            const int64_t s = base + lane;
            const bool act = s < S;
            const int64_t sc = act ? s : S - 1;
            const size_t e = (size_t)k * (size_t)S + (size_t)sc;
            const int g = st.node_of[(int64_t)d * S + sc];
            const int gu = __builtin_amdgcn_readfirstlane(g);
            const bool uni = __all(g == gu);
            int c = count[e];
            const double fv = fixval[e];
            double l, u;
            double* pc = nullptr;
            if (SHARED) {
                pc = st.sk + (size_t)sc * (size_t)st.sk_stride + st.sk_PC + 8 * (size_t)st.cmap[j];
                l = pc[2];
                u = pc[3];
            } else {
                l = st.lb[(size_t)j * (size_t)S + (size_t)sc];
                u = st.ub[(size_t)j * (size_t)S + (size_t)sc];
            }
            double xb, xsq;
            if (uni) {
                const int64_t o = (int64_t)gu * nl + off;
                xb = node_buf[o];
                xsq = node_buf[half + o];
            } else {
                const int64_t o = (int64_t)g * nl + off;
                xb = node_buf[o];
                xsq = node_buf[half + o];
            }
            // fixed already (fixer.py:119, 164, 257 is_fixed; 199-203 fixed on arrival): skipped
            const bool skip = !act || !isnan(fv) || l == u;
            arrived += (act && skip && iter0) ? 1 : 0;
            const int c0 = c;
            double v = 0.0;
            const bool fix = !skip && fixer_rule(iter0, xb, xsq, thk, nbk, lbk, ubk, l, u, prm.boundtol, c, v);
            if (!skip && c != c0) count[e] = c;
            if (fix) {
                // as k_fix_nonants / k_fix_nonants_sh for this entry
                v = fmin(fmax(v, l), u);
                fixval[e] = v;
                if (SHARED) {
                    const double w = v / st.Dc[j];
                    pc[6] = w;
                    pc[7] = w;
                } else {
                    const size_t je = (size_t)j * (size_t)S + (size_t)sc;
                    const double w = v / st.Dc[je];
                    st.lbh[je] = w;
                    st.ubh[je] = w;
                    if (st.pk) {
                        double* rec = st.pk + (size_t)sc * (size_t)st.pk_stride;
                        rec[st.pk_LB + j] = w;
                        rec[st.pk_UB + j] = w;
                    }
                }
            }
            const unsigned long long m = __ballot(fix);
            if (uni) {
                if (lane == 0 && m) atomicAdd(&acc[(int64_t)gu * nl + off], (int)__popcll(m));
            } else if (fix) {
                atomicAdd(&acc[(int64_t)g * nl + off], 1);
            }
        }
    }
    if (iter0) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) arrived += __shfl_down(arrived, o, WAVE);
        if (lane == 0 && arrived) atomicAdd(&totals[1], (unsigned long long)arrived);
    }
}

// The counts of k_fixer_step (acc, the library's, zero between calls and cleared again here)
// into nfix, overwritten in full; totals[0] += the entries newly fixed; totals[2] += the node
// entries that fixed some but not all of their local scenarios (fixer.py:217-219, 302-304, per
// node entry).  One block.
__global__ void __launch_bounds__(FX_T)
k_fixer_totals(int32_t* __restrict__ acc, const int32_t* __restrict__ nloc, int64_t half,
               int32_t* __restrict__ nfix, long long* __restrict__ totals) {
    __shared__ long long sf[FX_T / WAVE], sv[FX_T / WAVE];
    long long f = 0, var = 0;
    for (int64_t o = threadIdx.x; o < half; o += FX_T) {
        const int a = acc[o];
        if (a) acc[o] = 0;
        nfix[o] = a;
        f += a;
        var += (a > 0 && a < nloc[o]) ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        f += __shfl_down(f, o, WAVE);
        var += __shfl_down(var, o, WAVE);
    }
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        sf[threadIdx.x / WAVE] = f;
        sv[threadIdx.x / WAVE] = var;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        long long tf = 0, tv = 0;
        for (int w = 0; w < FX_T / WAVE; ++w) {
            tf += sf[w];
            tv += sv[w];
        }
        if (tf) totals[0] += tf;
        if (tv) totals[2] += tv;
    }
}
