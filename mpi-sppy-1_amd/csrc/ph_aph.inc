// APH (mpisppy/opt/aph.py): everything of one iteration that is not a subproblem solve, for all
// local scenarios (phgpu_aph_*, phgpu_select_smallest, include/phgpu.h).  Included by phgpu.hip
// after ph_fwph.inc.
//
// Arrays are the caller's, k-major and scenario-fastest like W.  The three node planes of
// phgpu_aph_reduce go through the node-segmented sum of ph_reduce.inc; the probability-weighted
// scalars of the other two passes are summed per thread in index order, per block in a fixed
// order and over the blocks by the one with the last ticket (aph_total, as k_w_diff); the
// dispatch selection counts with integer histograms only.  The same bits on every run.
#define AP_NV 3  // planes: sum pcoef x, sum pcoef x^2, sum pcoef y

// Update_y (aph.py:151-181) and the local sums of Compute_Averages (:394-408), one nonant per
// grid row: y = 0 with first, else W_use + rho (x - z_use) where mask is set (null: everywhere),
// else kept; then the three sums per (wave, nonant) for k_node_final<0, 3>.
__global__ void __launch_bounds__(BLOCK)
k_aph_reduce_partial(ph_tree st, ph_ws ws, int first, const int32_t* __restrict__ mask,
                     const double* __restrict__ x, const double* __restrict__ Wu, const double* __restrict__ zu,
                     const double* __restrict__ rho, double* __restrict__ y, double* __restrict__ planes) {
    const int64_t S = st.S;
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool act = s < S;
    const int k = blockIdx.y;
    if (k >= st.nn) return;
    const int d = st.nonant_depth[k];
    const int gnode = act ? st.node_of[IX(d)] : -1;
    const double w = act ? (st.pvar ? st.pvar[IX(k)] : st.pcoef[IX(d)]) : 0.0;
    const double xv = act ? x[IX(st.nonant_col[k])] : 0.0;
    double yv = 0.0;
    if (act) {
        if (first) {
            y[IX(k)] = 0.0;
        } else if (!mask || mask[s] != 0) {
            yv = Wu[IX(k)] + rho[IX(k)] * (xv - zu[IX(k)]);
            y[IX(k)] = yv;
        } else {
            yv = y[IX(k)];
        }
    }
    node_partial<0, AP_NV, true>(st, s / WAVE, k, act, gnode, ws.part, ws.tag, planes, [&](double(&pv)[AP_NV]) {
        pv[0] = w * xv;  // (formed here: fused into the sums, see node_partial)
        pv[1] = w * xv * xv;
        pv[2] = w * yv;
    });
}

// The grid's sums of N per-thread accumulators: every block its threads in a fixed order, the
// block with the last ticket the blocks' sums by a fixed tree.  True in every thread of that
// block, with the totals in tot (shared memory); it resets the ticket.  The grid has at most
// WD_BLOCKS blocks of GR_T threads.
template <int N>
__device__ __forceinline__ bool aph_total(const double (&acc)[N], double* __restrict__ bpart,
                                          int32_t* __restrict__ cnt, double (&tot)[N]) {
    __shared__ double red[N][GR_T / WAVE];
    __shared__ double fin[N][WD_BLOCKS];
    double b[N];
#pragma unroll
    for (int j = 0; j < N; ++j) b[j] = block_sum_fixed(acc[j], red[j]);
    const int nblk = (int)gridDim.x;
    if (!last_block_publish(b, bpart, cnt, (int)blockIdx.x, nblk)) return false;
    for (int u = threadIdx.x; u < WD_BLOCKS; u += blockDim.x) {
#pragma unroll
        for (int j = 0; j < N; ++j) fin[j][u] = u < nblk ? agent_read(&bpart[N * u + j]) : 0.0;
    }
    __syncthreads();
    for (int o = WD_BLOCKS / 2; o > 0; o >>= 1) {
        for (int u = threadIdx.x; u < o; u += blockDim.x) {
#pragma unroll
            for (int j = 0; j < N; ++j) fin[j][u] += fin[j][u + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < N; ++j) tot[j] = fin[j][0];
        ticket_reset(cnt);
    }
    __syncthreads();
    return true;
}

// the four words of out by one store instruction (lanes 0..3 of the first wave)
__device__ __forceinline__ void aph_store4(double* __restrict__ out, const double (&v)[4]) {
    if (threadIdx.x < 4) {
        const int t = threadIdx.x;
        out[t] = t == 0 ? v[0] : (t == 1 ? v[1] : (t == 2 ? v[2] : v[3]));
    }
}

// the body of listener_side_gig (aph.py:254-310) after the ranks' sum of the planes: x̄
// scattered, u = x - x̄, phi_s = p_s sum_k (z - x)(W - y) (:185-195) and
// out = {sum p (|u|^2 + |ȳ|^2 / gamma), sum phi, sum p |u|^2, sum p |ȳ|^2}
__global__ void __launch_bounds__(GR_T)
k_aph_norms(ph_tree st, double gamma, const double* __restrict__ planes, const double* __restrict__ x,
            const double* __restrict__ y, const double* __restrict__ W, const double* __restrict__ z,
            double* __restrict__ xbar, double* __restrict__ u, double* __restrict__ phi,
            double* __restrict__ bpart, int32_t* __restrict__ cnt, double* __restrict__ out) {
    __shared__ double tot[4];
    const int64_t S = st.S;
    const int nn = st.nn, nl = st.nlen_max;
    const int64_t half = (int64_t)st.num_nodes * nl;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < S; s += stride) {
        double usq = 0.0, vsq = 0.0, ph = 0.0;
        for (int k = 0; k < nn; ++k) {
            const int64_t o = (int64_t)st.node_of[IX(st.nonant_depth[k])] * nl + st.nonant_off[k];
            const double xb = planes[o], yb = planes[2 * half + o];
            const double xv = x[IX(st.nonant_col[k])];
            const double uu = xv - xb;
            xbar[IX(k)] = xb;
            u[IX(k)] = uu;
            usq += uu * uu;
            vsq += yb * yb;
            ph += (z[IX(k)] - xv) * (W[IX(k)] - y[IX(k)]);
        }
        const double p = st.prob[s];
        phi[s] = p * ph;
        acc[0] += p * (usq + vsq / gamma);
        acc[1] += p * ph;
        acc[2] += p * usq;
        acc[3] += p * vsq;
    }
    if (!aph_total(acc, bpart, cnt, tot)) return;
    const double v[4] = {tot[0], tot[1], tot[2], tot[3]};
    aph_store4(out, v);
}

// Update_theta_zw (aph.py:453-496) after the ranks' sum of the four scalars (red = {tau, phi,
// ..}): theta, W += theta u, z = x̄ (first) or z + theta ȳ / gamma, the post-step phi (:756) and
// out = {sum p W^2, sum p z^2, theta, sum phi}
__global__ void __launch_bounds__(GR_T)
k_aph_update(ph_tree st, int first, double nu, double gamma, const double* __restrict__ red,
             const double* __restrict__ planes, const double* __restrict__ x, const double* __restrict__ y,
             const double* __restrict__ u, double* __restrict__ W, double* __restrict__ z,
             double* __restrict__ phi, double* __restrict__ bpart, int32_t* __restrict__ cnt,
             double* __restrict__ out) {
    __shared__ double tot[3];
    const int64_t S = st.S;
    const int nn = st.nn, nl = st.nlen_max;
    const int64_t half = (int64_t)st.num_nodes * nl;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const double tau = red[0], gphi = red[1];
    const double theta = (tau > 0.0 && gphi > 0.0) ? gphi * nu / tau : 0.0;
    double acc[3] = {0.0, 0.0, 0.0};
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < S; s += stride) {
        double pw = 0.0, pz = 0.0, ph = 0.0;
        for (int k = 0; k < nn; ++k) {
            const int64_t o = (int64_t)st.node_of[IX(st.nonant_depth[k])] * nl + st.nonant_off[k];
            const double wn = W[IX(k)] + theta * u[IX(k)];
            const double zn = first ? planes[o] : z[IX(k)] + theta * planes[2 * half + o] / gamma;
            W[IX(k)] = wn;
            z[IX(k)] = zn;
            pw += wn * wn;
            pz += zn * zn;
            ph += (zn - x[IX(st.nonant_col[k])]) * (wn - y[IX(k)]);
        }
        const double p = st.prob[s];
        phi[s] = p * ph;
        acc[0] += p * pw;
        acc[1] += p * pz;
        acc[2] += p * ph;
    }
    if (!aph_total(acc, bpart, cnt, tot)) return;
    const double v[4] = {tot[0], tot[1], theta, tot[2]};
    aph_store4(out, v);
}

// The dispatch bookkeeping of the marked scenarios (aph.py:646, _update_foropt :529-550) and
// every scenario's next first key: round robin (:610-611) last_iter, else (:626-629)
// -max(last_iter, shelf_life - 1), as the reference writes it.
__global__ void __launch_bounds__(GR_T)
k_aph_mark(ph_tree st, const int32_t* __restrict__ mask, int iter, int shelf_life, int round_robin,
           const double* __restrict__ phi, int32_t* __restrict__ last_iter, double* __restrict__ last_phi,
           double* __restrict__ k1, const double* __restrict__ W, const double* __restrict__ z,
           double* __restrict__ W_lag, double* __restrict__ z_lag) {
    const int64_t S = st.S;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < S; s += stride) {
        const bool m = mask[s] != 0;
        int li = last_iter[s];
        if (m) {
            li = iter;
            last_iter[s] = iter;
            last_phi[s] = phi[s];
            if (W_lag)
                for (int k = 0; k < st.nn; ++k) {
                    W_lag[IX(k)] = W[IX(k)];
                    z_lag[IX(k)] = z[IX(k)];
                }
        }
        const int sl = shelf_life - 1;
        k1[s] = round_robin ? (double)li : -(double)(li > sl ? li : sl);
    }
}

// ------------------------------------------------------------------ the smallest count by (k1, k2, s)
// A radix select on the order-preserving 64-bit image of the keys, most significant digit
// first: SEL_PASSES launches per key, each a histogram of one digit over the candidates (those
// that match the digits fixed so far) and, in the block with the last ticket, the digit in
// which the wanted count falls.  k1 first, k2 among k1's ties; what is left are exact ties in
// both keys, of which the first few in index order are taken (k_sel_count, k_sel_emit).
// Counters and histograms are integers: the same result on every run.
#define SEL_T 256
#define SEL_BLOCKS 64     // blocks of a histogram pass at most: each takes a ticket on one counter
#define SEL_BITS 11
#define SEL_BINS (1 << SEL_BITS)
#define SEL_PASSES 6      // 5 digits of 11 bits and one of 9
#define SEL_EMIT_BLOCKS 1024  // blocks of the final two passes at most (each sums the counts of those before it)

struct sel_state {             // the select's device workspace
    unsigned long long T[2];   // image of the threshold of k1, of k2 (digits fixed so far)
    int32_t r;                 // how many are still to take among the candidates
    int32_t ticket;            // last-block counter (0 between launches)
    uint32_t hist[SEL_BINS];   // the pass's histogram (0 between launches)
    int32_t blk[2 * SEL_EMIT_BLOCKS];  // per block of k_sel_count: {below the threshold, ties}
};

// Doubles compare as their images do as unsigned integers; -0.0 takes the image of 0.0 (they
// compare equal).  A null key array: every image 0.
__device__ __forceinline__ unsigned long long sel_image(const double* __restrict__ key, int64_t s) {
    if (!key) return 0ull;
    double d = key[s];
    if (d == 0.0) d = 0.0;
    const unsigned long long b = (unsigned long long)__double_as_longlong(d);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ int sel_shift(int pass) { return pass < 5 ? 53 - SEL_BITS * pass : 0; }
__device__ __forceinline__ int sel_width(int pass) { return pass < 5 ? SEL_BITS : 9; }

// pass `pass` (0 .. SEL_PASSES - 1) of key `which` (0: k1, 1: k2).  count > 0: the select's
// first launch, which starts from r = count and empty thresholds instead of reading them.
__global__ void __launch_bounds__(SEL_T)
k_sel_pass(int64_t S, const double* __restrict__ k1, const double* __restrict__ k2, int which, int pass, int count,
           sel_state* __restrict__ ss) {
    __shared__ uint32_t lh[SEL_BINS];
    __shared__ uint32_t wsum[SEL_T / WAVE];
    __shared__ int last;
    const int t = threadIdx.x;
    const unsigned long long T0 = count > 0 ? 0ull : ss->T[0];
    const unsigned long long T1 = (count > 0 || (which == 1 && pass == 0)) ? 0ull : ss->T[1];
    const int r = count > 0 ? count : ss->r;
    const int sh = sel_shift(pass), wd = sel_width(pass);
    const unsigned long long Tc = which ? T1 : T0;
    // digits above this one: they are fixed (none at pass 0)
    const unsigned long long hi = pass == 0 ? 0ull : ~0ull << (sh + wd);
    for (int b = t; b < SEL_BINS; b += SEL_T) lh[b] = 0u;
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + t; s < S; s += stride) {
        const unsigned long long a = sel_image(which ? k2 : k1, s);
        const bool cand = (!which || sel_image(k1, s) == T0) && ((a ^ Tc) & hi) == 0ull;
        if (cand) atomicAdd(&lh[(unsigned)((a >> sh) & ((1ull << wd) - 1ull))], 1u);
    }
    __syncthreads();
    // this block's counts into the grid's histogram; the adds have returned before the ticket
    for (int b = t; b < SEL_BINS; b += SEL_T) {
        const uint32_t c = lh[b];
        if (c) {
            const uint32_t old = __hip_atomic_fetch_add(&ss->hist[b], c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("" ::"v"(old) : "memory");
        }
    }
    __syncthreads();
    if (t == 0)
        last = __hip_atomic_fetch_add(&ss->ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)gridDim.x - 1;
    __syncthreads();
    if (!last) return;
    // the last block: the grid's histogram (read and zeroed for the next pass), SEL_BINS /
    // SEL_T consecutive bins per thread, and the bin in which the r-th smallest candidate falls
    constexpr int PER = SEL_BINS / SEL_T;
    uint32_t c[PER], mine = 0u;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        c[j] = __hip_atomic_exchange(&ss->hist[t * PER + j], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        mine += c[j];
    }
    // exclusive prefix of the threads' sums: inside the wave by shuffles, then over the waves
    uint32_t inc = mine;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const uint32_t v = __shfl_up(inc, o, WAVE);
        if ((t & (WAVE - 1)) >= o) inc += v;
    }
    if ((t & (WAVE - 1)) == WAVE - 1) wsum[t / WAVE] = inc;
    __syncthreads();
    uint32_t before = inc - mine;
    for (int w = 0; w < t / WAVE; ++w) before += wsum[w];
    // exactly one thread holds the bin (1 <= r <= the number of candidates)
    if (before < (uint32_t)r && (uint32_t)r <= before + mine) {
        uint32_t cb = before;
        int bin = 0;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            if (cb < (uint32_t)r && (uint32_t)r <= cb + c[j]) {
                bin = t * PER + j;
                break;
            }
            cb += c[j];
        }
        const unsigned long long Tn = (Tc & hi) | ((unsigned long long)bin << sh);
        if (count > 0) {
            ss->T[0] = which ? 0ull : Tn;
            ss->T[1] = which ? Tn : 0ull;
        } else {
            ss->T[which] = Tn;
        }
        ss->r = r - (int)cb;
    }
    if (t == 0) __hip_atomic_store(&ss->ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// 0: beyond the threshold, 1: below it (taken), 2: an exact tie in both keys
__device__ __forceinline__ int sel_class(const sel_state* __restrict__ ss, const double* __restrict__ k1,
                                         const double* __restrict__ k2, int64_t s) {
    const unsigned long long a = sel_image(k1, s), b = sel_image(k2, s);
    const unsigned long long T0 = ss->T[0], T1 = ss->T[1];
    if (a < T0 || (a == T0 && b < T1)) return 1;
    return (a == T0 && b == T1) ? 2 : 0;
}

// block b's chunk of `chunk` consecutive scenarios: how many are below the threshold, how many tie
__global__ void __launch_bounds__(SEL_T)
k_sel_count(int64_t S, int64_t chunk, const double* __restrict__ k1, const double* __restrict__ k2,
            sel_state* __restrict__ ss) {
    __shared__ int cb[2];
    if (threadIdx.x < 2) cb[threadIdx.x] = 0;
    __syncthreads();
    const int64_t s0 = (int64_t)blockIdx.x * chunk, s1 = s0 + chunk < S ? s0 + chunk : S;
    int nb = 0, nt = 0;
    for (int64_t s = s0 + threadIdx.x; s < s1; s += SEL_T) {
        const int c = sel_class(ss, k1, k2, s);
        nb += c == 1;
        nt += c == 2;
    }
    if (nb) atomicAdd(&cb[0], nb);
    if (nt) atomicAdd(&cb[1], nt);
    __syncthreads();
    if (threadIdx.x < 2) ss->blk[2 * blockIdx.x + threadIdx.x] = cb[threadIdx.x];
}

// mask and list: a scenario is taken if it is below the threshold, or a tie with fewer than r
// ties before it; its place in list is the number of taken scenarios before it
__global__ void __launch_bounds__(SEL_T)
k_sel_emit(int64_t S, int64_t chunk, int count, const double* __restrict__ k1, const double* __restrict__ k2,
           const sel_state* __restrict__ ss, int32_t* __restrict__ mask, int32_t* __restrict__ list) {
    __shared__ int base[2];
    __shared__ int wb[SEL_T / WAVE], wt[SEL_T / WAVE];
    const int t = threadIdx.x, lane = t & (WAVE - 1), wv = t / WAVE;
    if (t < 2) base[t] = 0;
    __syncthreads();
    {
        int nb = 0, nt = 0;
        for (int b = t; b < (int)blockIdx.x; b += SEL_T) {
            nb += ss->blk[2 * b];
            nt += ss->blk[2 * b + 1];
        }
        if (nb) atomicAdd(&base[0], nb);
        if (nt) atomicAdd(&base[1], nt);
    }
    __syncthreads();
    int below = base[0], ties = base[1];  // before this tile
    const int r = ss->r;
    const int64_t s0 = (int64_t)blockIdx.x * chunk, s1 = s0 + chunk < S ? s0 + chunk : S;
    for (int64_t a = s0; a < s1; a += SEL_T) {
        const int64_t s = a + t;
        const int c = s < s1 ? sel_class(ss, k1, k2, s) : 0;
        const unsigned long long mb = __ballot(c == 1), mt = __ballot(c == 2);
        const unsigned long long lt = (1ull << lane) - 1ull;
        __syncthreads();  // (the previous tile's wave counts have been read)
        if (lane == 0) {
            wb[wv] = (int)__popcll(mb);
            wt[wv] = (int)__popcll(mt);
        }
        __syncthreads();
        int nb = below + (int)__popcll(mb & lt), nt = ties + (int)__popcll(mt & lt), tb = 0, tt = 0;
        for (int w = 0; w < SEL_T / WAVE; ++w) {
            if (w < wv) {
                nb += wb[w];
                nt += wt[w];
            }
            tb += wb[w];
            tt += wt[w];
        }
        if (s < s1) {
            const bool take = c == 1 || (c == 2 && nt < r);
            mask[s] = take ? 1 : 0;
            const int pos = nb + (nt < r ? nt : r);
            if (take && pos < count) list[pos] = (int32_t)s;
        }
        below += tb;
        ties += tt;
    }
}
