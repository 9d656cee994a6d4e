// The PH-side device reductions of phgpu.hip (included there; the entry points that launch
// them are phgpu_ph_reduce .. phgpu_expectations): one node-segmented sum (node_partial,
// k_node_final, k_planes_clear), one last-block ticket (last_block_publish) and the map
// kernels on top of them.

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, WAVE));
    return v;
}

// ------------------------------------------------------------------ node-segmented sum
// NV values per (node, nonant) in NV planes of num_nodes * nlen_max entries each.  MAXMASK:
// bit j set = plane j is a maximum, not a sum (its identity is -inf, not 0).
template <int MAXMASK>
__device__ __forceinline__ double pl_id(int j) {
    return ((MAXMASK >> j) & 1) ? -INFINITY : 0.0;
}
template <int MAXMASK>
__device__ __forceinline__ double pl_op(int j, double a, double b) {
    return ((MAXMASK >> j) & 1) ? fmax(a, b) : a + b;
}
template <int MAXMASK>
__device__ __forceinline__ void pl_atomic(int j, double* p, double v) {
    if ((MAXMASK >> j) & 1) atomicMax(p, v);
    else atomicAdd(p, v);
}

// every plane to its identity (what an entry no local scenario reaches keeps), and extra
// [nextra] (may be null) to 0: one pass over the NV * half + nextra entries
template <int MAXMASK, int NV>
__global__ void __launch_bounds__(256) k_planes_clear(double* __restrict__ planes, int64_t half,
                                                      double* __restrict__ extra, int64_t nextra) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, np = NV * half;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < np + nextra; i += stride) {
        if (i < np) {
            double v = pl_id<MAXMASK>(NV - 1);
#pragma unroll
            for (int j = NV - 2; j >= 0; --j) v = i < (j + 1) * half ? pl_id<MAXMASK>(j) : v;
            planes[i] = v;
        } else {
            extra[i - np] = 0.0;
        }
    }
}

// The partial half, one lane per scenario: this lane's node (-1 past S) and its NV values of
// nonant k (the planes' identities past S), which vals(v) fills in.  A wave whose scenarios
// share one node reduces them and stores one partial per plane and the node as tag
// (deterministic); a mixed wave goes to the planes per lane by fp64 atomics (add / max) and
// stores tag -1.  vals runs inside either branch: a product it forms there is contracted
// with the wave sum's first add into one fused multiply-add, a product formed ahead of the
// call is not -- the bits of the sums depend on which, so a caller keeps to its choice.
// MIXED = false: the caller's waves are uniform by construction (a two-stage-only entry
// point): no test, no atomic route, planes unused.
template <int MAXMASK, int NV, bool MIXED, typename Vals>
__device__ __forceinline__ void node_partial(const ph_tree& st, int64_t wave, int k, bool act, int gnode,
                                             double* __restrict__ part, int32_t* __restrict__ tag,
                                             double* __restrict__ planes, Vals vals) {
    const bool lead = (threadIdx.x & (WAVE - 1)) == 0;
    const int g0 = __shfl(gnode, 0, WAVE);
    double v[NV];
    if (!MIXED || !__any(act && gnode != g0)) {
        vals(v);
#pragma unroll
        for (int j = 0; j < NV; ++j) v[j] = ((MAXMASK >> j) & 1) ? wave_max(v[j]) : wave_sum(v[j]);
        if (lead) {
#pragma unroll
            for (int j = 0; j < NV; ++j) part[(wave * st.nn + k) * NV + j] = v[j];
            tag[wave * st.nn + k] = g0;
        }
    } else {
        if (act) {
            vals(v);
            const int64_t half = (int64_t)st.num_nodes * st.nlen_max;
            const int64_t o = (int64_t)gnode * st.nlen_max + st.nonant_off[k];
#pragma unroll
            for (int j = 0; j < NV; ++j) pl_atomic<MAXMASK>(j, &planes[j * half + o], v[j]);
        }
        if (lead) tag[wave * st.nn + k] = -1;
    }
}

// x̄ partial of nonant k over chunk w recomputed from x (a chunk of the path-6 epilogue
// partials with a scenario the fallback solved; DESIGN.md 3.8), in scenario order
__device__ __forceinline__ void xp_recompute(const ph_tree& st, const double* __restrict__ x, int64_t w, int C,
                                             int k, double& a, double& b) {
    const int64_t S = st.S;
    const int d = st.nonant_depth[k], j = st.nonant_col[k];
    const int64_t s1 = (w + 1) * C < S ? (w + 1) * C : S;
    a = b = 0.0;
    for (int64_t s = w * C; s < s1; ++s) {
        const double p = st.pvar ? st.pvar[IX(k)] : st.pcoef[IX(d)], v = x[IX(j)];
        a += p * v;
        b += p * v * v;
    }
}

// The final half: ordered segmented reduction of the per-wave partials (part, tagged by node),
// one block per nonant, into the planes.  The local scenarios are in tree order, so each
// node's waves form ONE contiguous run.  A run inside one thread's chunk of waves is complete
// and is flushed by that thread; a run that crosses chunks is flushed once, by the thread
// where it starts, which adds the following chunks' pieces in thread order (deterministic for
// every wave-uniform node); a nonant whose waves all share one node takes the fixed-order
// tree sum.
// assign: the planes were not cleared (one tree node, every entry is some nonant's): the
// fixed-order sum is stored, not added (one launch less per call).
#define XF_THREADS 256
template <int MAXMASK, int NV>
__global__ void __launch_bounds__(XF_THREADS)
k_node_final(ph_tree st, const double* __restrict__ part, const int32_t* __restrict__ node,
             double* __restrict__ planes, int assign) {
    __shared__ int fnode[XF_THREADS], lnode[XF_THREADS];
    __shared__ double fv[NV][XF_THREADS], lv[NV][XF_THREADS];
    __shared__ int single;
    const int k = blockIdx.x;
    const int t = threadIdx.x;
    const int64_t half = (int64_t)st.num_nodes * st.nlen_max;
    const int off = st.nonant_off[k];
    const int64_t nw = st.nwaves;
    const int64_t C = (nw + XF_THREADS - 1) / XF_THREADS;
    const int64_t w0 = (int64_t)t * C, w1 = (w0 + C < nw) ? w0 + C : nw;
    int cur = -1, first = -1;
    double a[NV], a_first[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) a[j] = a_first[j] = pl_id<MAXMASK>(j);
    for (int64_t w = w0; w < w1; ++w) {
        const int gnode = node[w * st.nn + k];
        double p[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) p[j] = part[(w * st.nn + k) * NV + j];
        if (gnode < 0) continue;
        if (gnode != cur) {
            if (cur >= 0) {
                if (first < 0) {  // close the chunk's first run
                    first = cur;
#pragma unroll
                    for (int j = 0; j < NV; ++j) a_first[j] = a[j];
                } else {          // a complete middle run
#pragma unroll
                    for (int j = 0; j < NV; ++j) pl_atomic<MAXMASK>(j, &planes[j * half + cur * st.nlen_max + off], a[j]);
                }
            }
            cur = gnode;
#pragma unroll
            for (int j = 0; j < NV; ++j) a[j] = pl_id<MAXMASK>(j);
        }
#pragma unroll
        for (int j = 0; j < NV; ++j) a[j] = pl_op<MAXMASK>(j, a[j], p[j]);
    }
    if (t == 0) single = 1;
    if (first < 0) {  // zero or one run in this chunk: it is the first (and last) run
        fnode[t] = cur;
        lnode[t] = -1;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            fv[j][t] = a[j];
            lv[j][t] = pl_id<MAXMASK>(j);
        }
    } else {
        fnode[t] = first;
        lnode[t] = cur;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            fv[j][t] = a_first[j];
            lv[j][t] = a[j];
        }
    }
    __syncthreads();
    // fast path (every two-stage problem, and any nonant whose local scenarios share one
    // node): all runs belong to thread 0's node -> fixed-order tree sum
    {
        const int g0 = fnode[0] >= 0 ? fnode[0] : lnode[0];
        if ((fnode[t] >= 0 && fnode[t] != g0) || (lnode[t] >= 0 && lnode[t] != g0)) single = 0;
    }
    __syncthreads();
    if (single) {
#pragma unroll
        for (int j = 0; j < NV; ++j) fv[j][t] = pl_op<MAXMASK>(j, fv[j][t], lv[j][t]);
        __syncthreads();
        for (int o = XF_THREADS / 2; o > 0; o >>= 1) {
            if (t < o) {
#pragma unroll
                for (int j = 0; j < NV; ++j) fv[j][t] = pl_op<MAXMASK>(j, fv[j][t], fv[j][t + o]);
            }
            __syncthreads();
        }
        if (t == 0) {
            int g0 = -1;
            for (int u = 0; u < XF_THREADS && g0 < 0; ++u) g0 = fnode[u] >= 0 ? fnode[u] : lnode[u];
            if (g0 >= 0) {
#pragma unroll
                for (int j = 0; j < NV; ++j) {
                    double* q = &planes[j * half + g0 * st.nlen_max + off];
                    *q = assign ? fv[j][0] : pl_op<MAXMASK>(j, *q, fv[j][0]);
                }
            }
        }
        return;
    }
    // several nodes: every run is flushed once, by the thread where it starts (its owner),
    // which adds the continuation pieces of the following threads in thread order.  All
    // runs flush in parallel (a serial merge by one thread cost ~0.2 ms per launch on
    // 1,057 aircond nodes); one flush per node keeps tree-ordered sums deterministic.
    // (lnode[u] >= 0 implies fnode[u] >= 0: a chunk's runs are maximal and distinct.)
    for (int side = 0; side < 2; ++side) {
        const int g = side ? lnode[t] : fnode[t];
        if (g < 0) continue;
        if (side == 0) {  // does the first run continue the previous non-empty chunk's tail?
            int p = t - 1;
            while (p >= 0 && fnode[p] < 0) --p;
            if (p >= 0 && (lnode[p] >= 0 ? lnode[p] : fnode[p]) == g) continue;
        }
        double sv[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) sv[j] = side ? lv[j][t] : fv[j][t];
        if (side == 1 || lnode[t] < 0) {  // this run reaches the end of the chunk
            for (int u = t + 1; u < XF_THREADS; ++u) {
                if (fnode[u] < 0) continue;  // empty chunk
                if (fnode[u] != g) break;
#pragma unroll
                for (int j = 0; j < NV; ++j) sv[j] = pl_op<MAXMASK>(j, sv[j], fv[j][u]);
                if (lnode[u] >= 0) break;    // the run ends inside chunk u
            }
        }
#pragma unroll
        for (int j = 0; j < NV; ++j) pl_atomic<MAXMASK>(j, &planes[j * half + g * st.nlen_max + off], sv[j]);
    }
}

// k_node_final<0, 2> for x̄, kept as a body of its own: the two sums (st.part, tagged by
// st.part_node) into the halves of node_buf in the same orders, plus the recompute from x of a
// dirty chunk of the path-6 epilogue's partials (per chunk of xpC scenarios, st.nwaves chunks).
// The template's instance computed the same bits but traced 0.4-0.5 us slower on multistage
// trees (11.4 against 10.9 us at [8, 65, 64]) for a reason its assembly did not show, and this
// kernel is on every PH iteration's critical path.
// assign: node_buf was not cleared (one tree node, every entry is some nonant's): the fast
// path stores its sums instead of adding them (phgpu_ph_reduce: one launch less per step)
__global__ void __launch_bounds__(XF_THREADS) k_xbar_final(ph_tree st, double* __restrict__ node_buf,
                                                           const int32_t* __restrict__ dirty = nullptr,
                                                           int xpC = 0, const double* __restrict__ x = nullptr,
                                                           int assign = 0) {
    __shared__ int fnode[XF_THREADS], lnode[XF_THREADS];
    __shared__ double fa[XF_THREADS], fb[XF_THREADS], la[XF_THREADS], lb[XF_THREADS];
    const int k = blockIdx.x;
    const int t = threadIdx.x;
    const int half = st.num_nodes * st.nlen_max;
    const int off = st.nonant_off[k];
    const int64_t nw = st.nwaves;
    const int64_t C = (nw + XF_THREADS - 1) / XF_THREADS;
    const int64_t w0 = (int64_t)t * C, w1 = (w0 + C < nw) ? w0 + C : nw;
    int cur = -1, first = -1;
    double a = 0.0, b = 0.0, a_first = 0.0, b_first = 0.0;
    for (int64_t w = w0; w < w1; ++w) {
        // the chunk's node, dirty flag and partials in flight together (none gates another
        // load: one memory round trip per chunk instead of three on the x̄ critical path)
        const int gnode = st.part_node[w * st.nn + k];
        const int dw = dirty ? dirty[w] : 0;
        const double pa = st.part[(w * st.nn + k) * 2 + 0], pb = st.part[(w * st.nn + k) * 2 + 1];
        if (gnode < 0) continue;
        if (gnode != cur) {
            if (cur >= 0) {
                if (first < 0) {  // close the chunk's first run
                    first = cur;
                    a_first = a;
                    b_first = b;
                } else {          // a complete middle run
                    atomicAdd(&node_buf[cur * st.nlen_max + off], a);
                    atomicAdd(&node_buf[half + cur * st.nlen_max + off], b);
                }
            }
            cur = gnode;
            a = 0.0;
            b = 0.0;
        }
        if (dw) {
            double ra, rb;
            xp_recompute(st, x, w, xpC, k, ra, rb);
            a += ra;
            b += rb;
        } else {
            a += pa;
            b += pb;
        }
    }
    if (first < 0) {  // zero or one run in this chunk: it is the first (and last) run
        fnode[t] = cur;
        fa[t] = a;
        fb[t] = b;
        lnode[t] = -1;
        la[t] = lb[t] = 0.0;
    } else {
        fnode[t] = first;
        fa[t] = a_first;
        fb[t] = b_first;
        lnode[t] = cur;
        la[t] = a;
        lb[t] = b;
    }
    __syncthreads();
    // fast path (every two-stage problem, and any nonant whose local scenarios share one
    // node): all runs belong to thread 0's node -> fixed-order tree sum
    __shared__ int single;
    if (t == 0) single = 1;
    __syncthreads();
    {
        const int g0 = fnode[0] >= 0 ? fnode[0] : lnode[0];
        if ((fnode[t] >= 0 && fnode[t] != g0) || (lnode[t] >= 0 && lnode[t] != g0)) single = 0;
    }
    __syncthreads();
    if (single) {
        fa[t] += la[t];
        fb[t] += lb[t];
        __syncthreads();
        for (int off = XF_THREADS / 2; off > 0; off >>= 1) {
            if (t < off) {
                fa[t] += fa[t + off];
                fb[t] += fb[t + off];
            }
            __syncthreads();
        }
        if (t == 0) {
            int g0 = -1;
            for (int u = 0; u < XF_THREADS && g0 < 0; ++u) g0 = fnode[u] >= 0 ? fnode[u] : lnode[u];
            if (g0 >= 0 && assign) {
                node_buf[g0 * st.nlen_max + off] = fa[0];
                node_buf[half + g0 * st.nlen_max + off] = fb[0];
            } else if (g0 >= 0) {
                node_buf[g0 * st.nlen_max + off] += fa[0];
                node_buf[half + g0 * st.nlen_max + off] += fb[0];
            }
        }
        return;
    }
    // several nodes: every run is flushed once, by the thread where it starts (its owner),
    // which adds the continuation pieces of the following threads in thread order.  All
    // runs flush in parallel (a serial merge by one thread cost ~0.2 ms per launch on
    // 1,057 aircond nodes); one flush per node keeps tree-ordered sums deterministic.
    // (lnode[u] >= 0 implies fnode[u] >= 0: a chunk's runs are maximal and distinct.)
    for (int side = 0; side < 2; ++side) {
        const int g = side ? lnode[t] : fnode[t];
        if (g < 0) continue;
        if (side == 0) {  // does the first run continue the previous non-empty chunk's tail?
            int p = t - 1;
            while (p >= 0 && fnode[p] < 0) --p;
            if (p >= 0 && (lnode[p] >= 0 ? lnode[p] : fnode[p]) == g) continue;
        }
        double sa = side ? la[t] : fa[t];
        double sb = side ? lb[t] : fb[t];
        if (side == 1 || lnode[t] < 0) {  // this run reaches the end of the chunk
            for (int u = t + 1; u < XF_THREADS; ++u) {
                if (fnode[u] < 0) continue;  // empty chunk
                if (fnode[u] != g) break;
                sa += fa[u];
                sb += fb[u];
                if (lnode[u] >= 0) break;    // the run ends inside chunk u
            }
        }
        atomicAdd(&node_buf[g * st.nlen_max + off], sa);
        atomicAdd(&node_buf[half + g * st.nlen_max + off], sb);
    }
}

// ------------------------------------------------------------------ last-block ticket
// A grid-wide reduction without a second launch: every block swaps its N partials into
// bpart[N * bid ..], then takes a ticket on cnt (0 between launches); true in every thread of
// the block with the last ticket, which reads all partials with agent_read and resets the
// counter with ticket_reset.  All threads of the block call it; v is thread 0's.
// Every cross-block exchange is an agent-scope atomic read-modify-write, performed at the
// device's coherence point, so no block needs a release fence (an L2 writeback on gfx950,
// DESIGN.md 3.8).  The swaps have returned before the ticket is taken (the empty asm consumes
// their results, so the compiler waits for them).  Ordering rests on the hardware, not on
// the HIP memory model (all RMWs are relaxed): a returning agent-scope atomic has been
// performed at the device's coherence point when its value is back, so the last block's
// reads of bpart (agent-scope RMWs as well) see every partial whose ticket precedes its own.
// Release / acquire would make it formal at the price of an L2 writeback on every XCD (15-29
// us per launch, DESIGN.md 3.4).  tests/test_gpu_readback.py compares the conv made this way
// bit for bit with the ordered device reduction and would catch a reordering.
template <int N>
__device__ __forceinline__ bool last_block_publish(const double (&v)[N], double* __restrict__ bpart,
                                                   int32_t* __restrict__ cnt, int bid, int nblk) {
    __shared__ int last;
    if (threadIdx.x == 0) {
        double old[N];
#pragma unroll
        for (int j = 0; j < N; ++j)
            old[j] = __hip_atomic_exchange(&bpart[N * bid + j], v[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int j = 0; j < N; ++j) asm volatile("" ::"v"(old[j]) : "memory");
        last = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nblk - 1;
    }
    __syncthreads();
    return last;
}
__device__ __forceinline__ double agent_read(double* p) {
    return __hip_atomic_fetch_add(p, 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void ticket_reset(int32_t* cnt) {
    __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ------------------------------------------------------------------ x̄
// phbase.py:54-79: prob_coeff * x and prob_coeff * x^2 of each nonant, one nonant per grid
// row (blockIdx.y; see k_ph_update), into st.part / st.part_node for k_xbar_final.
__global__ void __launch_bounds__(BLOCK)
k_xbar_partial(ph_tree st, const double* __restrict__ x, double* __restrict__ node_buf, int clear) {
    const int64_t S = st.S;
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool act = s < S;
    // no wave spans two nodes (st.xbar_mixed == 0): this kernel does not touch node_buf
    // below, so it clears it for k_xbar_final (one launch less than a memset)
    if (clear && blockIdx.y == 0) {
        const int64_t nb = 2 * (int64_t)st.num_nodes * st.nlen_max;
        for (int64_t i = s; i < nb; i += (int64_t)gridDim.x * blockDim.x) node_buf[i] = 0.0;
    }
    if ((int)blockIdx.y < st.nn) {
        const int k = blockIdx.y;
        const int d = st.nonant_depth[k];
        const int gnode = act ? st.node_of[IX(d)] : -1;
        const double w = act ? (st.pvar ? st.pvar[IX(k)] : st.pcoef[IX(d)]) : 0.0;
        const double v = act ? x[IX(st.nonant_col[k])] : 0.0;
        node_partial<0, 2, true>(st, s / WAVE, k, act, gnode, st.part, st.part_node, node_buf, [&](double(&pv)[2]) {
            pv[0] = w * v;  // (formed here: fused into the sums, see node_partial)
            pv[1] = w * v * v;
        });
    }
}

// out[0] |= 1 if some wave of local scenarios spans two nodes at a nonant's depth (the
// test node_partial makes per wave)
// out[1] |= 1 if some local scenario's node at a nonant's depth differs from scenario 0's
__global__ void __launch_bounds__(BLOCK) k_xbar_mixed(ph_tree st, int32_t* __restrict__ out) {
    const int64_t S = st.S;
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool act = s < S;
    bool mixed = false, multi = false;
    for (int k = 0; k < st.nn; ++k) {
        const int d = st.nonant_depth[k];
        const int gnode = act ? st.node_of[IX(d)] : -1;
        const int g0 = __shfl(gnode, 0, WAVE);
        mixed |= __any(act && gnode != g0) != 0;
        multi |= __any(act && gnode != st.node_of[(int64_t)d * S]) != 0;
    }
    if (mixed && (threadIdx.x & (WAVE - 1)) == 0) atomicOr(out, 1);
    if (multi && (threadIdx.x & (WAVE - 1)) == 0) atomicOr(out + 1, 1);
}

// ------------------------------------------------------------------ adaptive rho
// The residual sums of NormRhoUpdater and the two convergers (include/phgpu.h
// phgpu_ph_residuals), four sums per (wave, nonant) in partials of their own (ws: the handle's rs).
#define RS_NV 4  // planes: prob |x - x̄|, pcoef |x - x̄|, rho, prob rho

// norm_rho_updater.py:73-83 (plane 0), primal_dual_converger.py:66-82 and 96-107 (planes 1,
// 2), norm_rho_converger.py:26 (plane 3), one nonant per grid row.  rho_last
// (norm_rho_updater.py:98-104, the last local scenario's rho at each node): the local
// scenarios are in tree order, so a node's scenarios are one run, and the lane at the end of a
// run stores its rho.
__global__ void __launch_bounds__(BLOCK)
k_resid_partial(ph_tree st, ph_ws ws, const double* __restrict__ x, const double* __restrict__ xbar,
                const double* __restrict__ rho, double* __restrict__ planes, double* __restrict__ rho_last) {
    const int64_t S = st.S;
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool act = s < S;
    const int k = blockIdx.y;
    if (k >= st.nn) return;
    const int d = st.nonant_depth[k];
    const int gnode = act ? st.node_of[IX(d)] : -1;
    const int gnext = (act && s + 1 < S) ? st.node_of[IX(d) + 1] : -1;
    const double r = act ? rho[IX(k)] : 0.0;
    const double ad = act ? fabs(x[IX(st.nonant_col[k])] - xbar[IX(k)]) : 0.0;
    const double pi = act ? st.prob[s] : 0.0;
    const double pc = act ? (st.pvar ? st.pvar[IX(k)] : st.pcoef[IX(d)]) : 0.0;
    // (the products formed here, ahead of node_partial, on purpose: not fused into the sums)
    const double v[RS_NV] = {pi * ad, pc * ad, r, pi * r};
    if (act && gnext != gnode) rho_last[gnode * st.nlen_max + st.nonant_off[k]] = r;
    node_partial<0, RS_NV, true>(st, s / WAVE, k, act, gnode, ws.part, ws.tag, planes, [&](double(&o)[RS_NV]) {
#pragma unroll
        for (int j = 0; j < RS_NV; ++j) o[j] = v[j];
    });
}

// NormRhoUpdater.miditer's rule (norm_rho_updater.py:128-143) for every local (k, s): one
// nonant per grid row, a row's blocks stride over the scenarios (the grid of k_ph_update).
// The residuals are per (node, nonant), so every rank and every scenario of a node takes the
// same branch.  counts (may be null): entries that took no action / increase / decrease /
// converged decrease, by integer atomics (one per wave and action).
#define NR_T 256
#define NR_U 4
__global__ void __launch_bounds__(NR_T)
k_norm_rho_update(ph_tree st, phgpu_norm_rho_params prm, const double* __restrict__ plane0,
                  const double* __restrict__ rho_last, const double* __restrict__ xbar_node,
                  const double* __restrict__ xbar_prev, double* __restrict__ rho,
                  unsigned long long* __restrict__ counts) {
    const int64_t S = st.S;
    const int k = blockIdx.y;
    int c[4] = {0, 0, 0, 0};
    if (k < st.nn) {
        const int d = st.nonant_depth[k];
        const int off = st.nonant_off[k], nl = st.nlen_max;
        const int64_t stride = (int64_t)gridDim.x * blockDim.x;
        for (int64_t s0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s0 < S; s0 += NR_U * stride) {
            double p[NR_U], dr[NR_U], r[NR_U];
#pragma unroll
            for (int u = 0; u < NR_U; ++u) {
                const int64_t s = s0 + u * stride;
                p[u] = dr[u] = r[u] = 0.0;
                if (s < S) {
                    const int o = st.node_of[(int64_t)d * S + s] * nl + off;
                    p[u] = plane0[o];
                    dr[u] = rho_last[o] * fabs(xbar_node[o] - xbar_prev[o]);
                    r[u] = rho[(int64_t)k * S + s];
                }
            }
#pragma unroll
            for (int u = 0; u < NR_U; ++u) {
                const int64_t s = s0 + u * stride;
                if (s < S) {
                    int act = 0;
                    if (p[u] > prm.f * dr[u] && p[u] > prm.tol) {
                        act = 1;
                        rho[(int64_t)k * S + s] = r[u] * prm.inc;
                    } else if (dr[u] > prm.f * p[u] && dr[u] > prm.tol) {
                        if (prm.allow_decrease) {
                            act = 2;
                            rho[(int64_t)k * S + s] = r[u] / prm.dec;
                        }
                    } else if (p[u] < prm.tol && dr[u] < prm.tol) {
                        act = 3;
                        rho[(int64_t)k * S + s] = r[u] / prm.conv_dec;
                    }
#pragma unroll
                    for (int a = 0; a < 4; ++a) c[a] += act == a;
                }
            }
        }
    }
    if (counts) {
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            int v = c[a];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, WAVE);
            if ((threadIdx.x & (WAVE - 1)) == 0 && v) atomicAdd(&counts[a], (unsigned long long)v);
        }
    }
}

// ------------------------------------------------------------------ xhat candidates
// Per-node statistics of a nonant array v[nn*S] (k-major, like W or a spoke's localnonants):
// the candidates of XhatXbar (extensions/xhatxbar.py:38-55: the node's x̄), the slam
// heuristics (cylinders/slam_heuristic.py:57-67, 84: the column-wise max / min) and the x̄ /
// x̄² XhatClosest measures against (extensions/xhatclosest.py:37-45): planes 0-1 are sums,
// planes 2-3 maxima (the minimum is stored negated, so that one MAX over the ranks serves
// both), for k_node_final<0xC, 4>.  One lane per scenario, NS_KU nonants per grid row.
#define NS_KU 4  // nonants per grid row: their loads are in flight together
__global__ void __launch_bounds__(BLOCK)
k_nstats_partial(ph_tree st, ph_ws ws, const double* __restrict__ v, double* __restrict__ planes) {
    const int64_t S = st.S;
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool act = s < S;
    const int k0 = blockIdx.y * NS_KU;
    double val[NS_KU], pc[NS_KU];
    int gn[NS_KU];
#pragma unroll
    for (int u = 0; u < NS_KU; ++u) {
        const int k = k0 + u;
        const bool on = act && k < st.nn;
        const int d = k < st.nn ? st.nonant_depth[k] : 0;
        gn[u] = on ? st.node_of[IX(d)] : -1;
        val[u] = on ? v[IX(k)] : 0.0;
        pc[u] = on ? (st.pvar ? st.pvar[IX(k)] : st.pcoef[IX(d)]) : 0.0;
    }
#pragma unroll
    for (int u = 0; u < NS_KU; ++u) {
        const int k = k0 + u;
        if (k >= st.nn) break;
        // (the products formed here, ahead of node_partial, on purpose: not fused into the sums)
        const double w[RS_NV] = {pc[u] * val[u], pc[u] * val[u] * val[u], act ? -val[u] : -INFINITY,
                                 act ? val[u] : -INFINITY};
        node_partial<0xC, RS_NV, true>(st, s / WAVE, k, act, gn[u], ws.part, ws.tag, planes, [&](double(&o)[RS_NV]) {
#pragma unroll
            for (int j = 0; j < RS_NV; ++j) o[j] = w[j];
        });
    }
}

// xhatclosest.py:37-51 for a two-stage handle: one lane per scenario sums, k ascending, the
// truncated z-scores min(3, |v - x̄| / sqrt(var)) of the nonants with var = x̄² - x̄ x̄ > 0
// (strict), NC_KU loads of v in flight.  The smallest distance and the lowest local index
// attaining it (the reference's strict < scan): (distance, index) pairs reduced per wave and
// per block, then over the blocks by the one with the last ticket (last_block_publish),
// which stores best.  The lexicographic minimum does not depend on the order.  The index
// travels as a double (exact below 2^53), as best[1] returns it.
#define NC_T 256
#define NC_KU 4
__device__ __forceinline__ void argmin_take(double& d, double& i, double od, double oi) {
    if (od < d || (od == d && oi < i)) {
        d = od;
        i = oi;
    }
}

// the block's lexicographic minimum of (d, i), in thread 0; rd, ri: one slot per wave
__device__ __forceinline__ void block_argmin(double& d, double& i, double* rd, double* ri) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        argmin_take(d, i, __shfl_down(d, off, WAVE), __shfl_down(i, off, WAVE));
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        rd[threadIdx.x / WAVE] = d;
        ri[threadIdx.x / WAVE] = i;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int u = 1; u < NC_T / WAVE; ++u) argmin_take(d, i, rd[u], ri[u]);
}

__global__ void __launch_bounds__(NC_T)
k_nonant_closest(ph_tree st, const double* __restrict__ v, const double* __restrict__ xbar_node,
                 const double* __restrict__ xsqbar_node, double* __restrict__ dist, double* __restrict__ bpart,
                 int32_t* __restrict__ cnt, double* __restrict__ best) {
    __shared__ double rd[NC_T / WAVE], ri[NC_T / WAVE];
    const int64_t S = st.S;
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool act = s < S;
    const int nn = st.nn;
    double acc = 0.0;
    for (int k0 = 0; k0 < nn; k0 += NC_KU) {
        double val[NC_KU];
#pragma unroll
        for (int u = 0; u < NC_KU; ++u) val[u] = (act && k0 + u < nn) ? v[IX(k0 + u)] : 0.0;
#pragma unroll
        for (int u = 0; u < NC_KU; ++u) {
            if (k0 + u >= nn) break;
            const int o = st.nonant_off[k0 + u];
            const double xb = xbar_node[o];
            const double var = xsqbar_node[o] - xb * xb;
            if (var > 0.0) acc += fmin(3.0, fabs(val[u] - xb) / sqrt(var));
        }
    }
    if (act && dist) dist[s] = acc;
    double d = act ? acc : INFINITY, i = act ? (double)s : INFINITY;
    block_argmin(d, i, rd, ri);
    const int nblk = (int)gridDim.x;
    const double pair[2] = {d, i};
    if (!last_block_publish(pair, bpart, cnt, (int)blockIdx.x, nblk)) return;
    d = INFINITY;
    i = INFINITY;
    for (int b = threadIdx.x; b < nblk; b += blockDim.x) {
        const double od = agent_read(&bpart[2 * b]), oi = agent_read(&bpart[2 * b + 1]);
        argmin_take(d, i, od, oi);
    }
    block_argmin(d, i, rd, ri);
    if (threadIdx.x == 0) {
        best[1] = i;
        best[0] = d;
        ticket_reset(cnt);
    }
}

// ------------------------------------------------------------------ gradient rho
// The cost-proportional rho of mpisppy/utils/gradient.py, find_rho.py and
// extensions/gradient_extension.py with the dual metric of utils/wtracker.py:134-157
// (include/phgpu.h phgpu_grad_cost .. phgpu_rho_from_stats): four single passes over at most
// nn * S doubles.
#define GR_T 256
#define GR_ROWS 65535  // grid rows at most (gridDim.y's limit): a kernel with a nonant per row strides over them

// c and q of column j of scenario s in original units: the library's copies, or on a
// shared-matrix handle words 0 and 1 of the column's per-scenario record (k_sh_fill; every
// nonant column has one)
__device__ __forceinline__ void obj_cq(const ph_data& st, int j, int64_t s, double& c, double& q) {
    if (st.shared) {
        const double* e = st.sk + (size_t)s * (size_t)st.sk_stride + st.sk_PC + 8 * (size_t)st.cmap[j];
        c = e[0];
        q = e[1];
    } else {
        c = st.c[(size_t)j * (size_t)st.S + (size_t)s];
        q = st.q[(size_t)j * (size_t)st.S + (size_t)s];
    }
}

// gradient.py:65-81 for f(x) = c.x + 1/2 x.diag(q).x: cost[k, s] = -(c + q xn[k, s]), one
// nonant per grid row
__global__ void __launch_bounds__(GR_T)
k_grad_cost(ph_data st, const double* __restrict__ xn, double* __restrict__ cost) {
    const int64_t S = st.S;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int k = blockIdx.y; k < st.nn; k += gridDim.y) {  // (more nonants than grid rows: strided)
        const int j = st.nonant_col[k];
        for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < S; s += stride) {
#pragma clang fp contract(off)  // two roundings, as numpy's c + q * x: no fused multiply-add
            double c, q;
            obj_cq(st, j, s, c, q);
            const double qx = q * xn[IX(k)];
            cost[IX(k)] = -(c + qx);
        }
    }
}

// A block's threads summed in a fixed order (wave shuffles, then the waves' sums in wave
// order); the result is thread 0's
__device__ __forceinline__ double block_sum_fixed(double v, double* red) {
    v = wave_sum(v);
    if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int u = 0; u < (int)(blockDim.x / WAVE); ++u) t += red[u];
    return t;
}

// wtracker.py:141-154: out[0] = scale x sum over the local (k, s) of |W - W_prev|, and W_prev
// = W in the same pass.  Every thread adds its elements in index order, every block its threads
// in a fixed order; the block with the last ticket (last_block_publish) adds the blocks' sums
// by a fixed tree and stores out: the same bits on every run.  The grid has at most WD_BLOCKS
// blocks.
#define WD_BLOCKS 256
__global__ void __launch_bounds__(GR_T)
k_w_diff(const double* __restrict__ W, double* __restrict__ W_prev, int64_t tot, double scale,
         double* __restrict__ bpart, int32_t* __restrict__ cnt, double* __restrict__ out) {
    __shared__ double red[GR_T / WAVE];
    __shared__ double fin[WD_BLOCKS];
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < tot; i += stride) {
        const double w = W[i];
        acc += fabs(w - W_prev[i]);
        W_prev[i] = w;
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
        out[0] = scale * fin[0];
        ticket_reset(cnt);
    }
}

// find_rho.py:170-203 up to the order statistic, for a two-stage handle: r[k, s] = |cost[k, s]|
// / denominator and, per nonant, the per-wave partials (ws: the handle's rr) of sum r, max(-r)
// and max(r) for k_node_final<0x6, 3>.  One lane per scenario.
//   gden == null: the scenario's own denominator, the largest over its nonants j of
//     max(|x_j - x̄_j|, 2 (x_j - x̄_j)^2): np.max((w_denom, prox_denom)) at find_rho.py:189
//     is ONE scalar per scenario (:78-115);
//   gden given:   gden[offset of k] for every scenario (_grad_denom, :118-147).
// IEEE division (numpy's): a zero denominator gives +inf (0 / 0 NaN, which fmax drops).
#define RR_NV 3  // planes: sum r, max(-r), max(r)
__global__ void __launch_bounds__(BLOCK)
k_rho_ratio_partial(ph_tree st, ph_ws ws, const double* __restrict__ cost, const double* __restrict__ x,
                    const double* __restrict__ xbar, const double* __restrict__ gden) {
    const int64_t S = st.S;
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool act = s < S;
    const int nn = st.nn;
    double d = 0.0;
    if (!gden && act) {
        for (int k = 0; k < nn; ++k) {
            const double dx = x[IX(st.nonant_col[k])] - xbar[IX(k)];
            d = fmax(d, fmax(fabs(dx), 2.0 * (dx * dx)));
        }
    }
    const int gnode = act ? st.node_of[s] : -1;
    for (int k = 0; k < nn; ++k) {
        double r = 0.0;
        if (act) r = fabs(cost[IX(k)]) / (gden ? gden[st.nonant_off[k]] : d);
        node_partial<0x6, RR_NV, false>(st, s / WAVE, k, act, gnode, ws.part, ws.tag, nullptr, [&](double(&v)[RR_NV]) {
            v[0] = r;
            v[1] = act ? -r : -INFINITY;
            v[2] = act ? r : -INFINITY;
        });
    }
}

// find_rho.py:150-168 (_order_stat) and the rho rewrite of gradient_extension.py:85-94 for a
// two-stage handle: every local rho[k, s] becomes the order statistic of nonant k's ratios,
// if the gate is open -- |(prev - cur) / prev| <= thr on gate = {prev, cur}, which NaN and
// inf fail (gradient_extension.py:65-68); a null gate is open.  Every thread evaluates the
// gate itself (two cached loads); a closed gate stores nothing to rho.  One nonant per grid
// row; applied (may be null) is stored by the grid's first thread.
__global__ void __launch_bounds__(GR_T)
k_rho_from_stats(ph_tree st, const double* __restrict__ planes, double s_total, double alpha,
                 const double* __restrict__ gate, double thr, double* __restrict__ rho,
                 int32_t* __restrict__ applied) {
    const int64_t S = st.S;
    bool open = true;
    if (gate) {
        const double prev = gate[0], cur = gate[1];
        open = fabs((prev - cur) / prev) <= thr;
    }
    if (applied && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *applied = open ? 1 : 0;
    if (!open) return;
    const int64_t half = (int64_t)st.num_nodes * st.nlen_max;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int k = blockIdx.y; k < st.nn; k += gridDim.y) {  // (more nonants than grid rows: strided)
        const int off = st.nonant_off[k];
        const double mean = planes[off] / s_total;
        const double mn = -planes[half + off], mx = planes[2 * half + off];
        double v;
        if (alpha == 0.5) v = mean;
        else if (alpha < 0.5) v = mn + alpha * 2.0 * (mean - mn);
        else v = (2.0 * mean - mx) + alpha * 2.0 * (mx - mean);
        for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < S; s += stride) rho[IX(k)] = v;
    }
}

// ------------------------------------------------------------------ PH update
// Where the update kernels leave conv (phbase.py:330-339) and the last solve's statistics
struct conv_sink {
    double* conv;                          // conv_local (pinned host or device memory)
    const unsigned long long* stats_src;   // the last solve's statistics (device), or null
    int stats_copies;                      // copies of them at stats_src (stats_word)
    int64_t* stats_dst;                    // where they go (pinned host or device), or null
    double scale;                          // 1 / (S nn)
    double* cpart;                         // [gridDim.x] block partials
    int32_t* cnt;                          // last-block counter (0 between launches)
};

// conv = scale x (sum over the grid of every thread's acc), without a second launch: each
// block reduces its threads in a fixed order; the block with the last ticket
// (last_block_publish) sums the block partials in block order (deterministic) and stores the
// statistics, then conv.  The host reads stats after it sees conv (phgpu_ph_update_ex).
__device__ __forceinline__ void conv_last_block(double acc, const conv_sink& o) {
    __shared__ double red[XL_T / WAVE];
    const int wv = threadIdx.x / WAVE, nwb = (int)(blockDim.x / WAVE);
    // the solve's statistics copies, loaded now by every block's first wave (the previous
    // launch wrote them: stream order) and reduced only by the last block -- their load is
    // off the exchange / ticket chain
    unsigned long long sv[6];
    {
        const int t = threadIdx.x;
#pragma unroll
        for (int k = 0; k < 6; ++k)
            sv[k] = (o.stats_dst && t < o.stats_copies) ? o.stats_src[t * PHGPU_STATS_STRIDE + k] : 0ull;
    }
    const int nblk = (int)(gridDim.x * gridDim.y), bid = (int)(blockIdx.y * gridDim.x + blockIdx.x);
    const double bsum[1] = {block_sum_fixed(acc, red)};
    if (!last_block_publish(bsum, o.cpart, o.cnt, bid, nblk)) return;
    double a = 0.0;
    for (int b = threadIdx.x; b < nblk; b += blockDim.x) a += agent_read(&o.cpart[b]);
    a = wave_sum(a);
    if ((threadIdx.x & (WAVE - 1)) == 0) red[wv] = a;
    __syncthreads();
    // lanes 0..5 store the statistics and lane 6 conv in one store instruction (no wait for
    // the host-memory acknowledgements: the host polls conv and the statistics' sentinels,
    // engine.convergence_wait)
    if (threadIdx.x < WAVE) {
        double t = 0.0;
        for (int u = 0; u < nwb; ++u) t += red[u];
        if (o.stats_dst) {
            unsigned long long v[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) v[k] = sv[k];
#pragma unroll
            for (int o2 = 32; o2 > 0; o2 >>= 1)
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    const unsigned long long u = __shfl_xor(v[k], o2, 64);
                    v[k] = k == 5 ? (u > v[k] ? u : v[k]) : v[k] + u;
                }
            unsigned long long w = v[0];
#pragma unroll
            for (int k = 1; k < 6; ++k) w = (int)threadIdx.x == k ? v[k] : w;
            if (threadIdx.x < 6) o.stats_dst[threadIdx.x] = (int64_t)w;
        }
        if (threadIdx.x == 6) *o.conv = t * o.scale;
        if (threadIdx.x == 0) ticket_reset(o.cnt);
    }
}

// phbase.py:90-103 (scatter x̄), 293-318 (W update), 330-339 (local |x - x̄| sum, reduced
// by the last block into conv_local).
#define UPD_T 256
#define UPD_BLOCKS 256  // at most about this many blocks: each takes a ticket on one counter
#define UPD_U 4         // scenarios per thread in flight per trip
__global__ void __launch_bounds__(UPD_T)
k_ph_update(ph_tree st, const double* __restrict__ x, const double* __restrict__ node_buf,
            double* __restrict__ xbar, double* __restrict__ W, const double* __restrict__ rho,
            int update_W, conv_sink o) {
    // one nonant per grid row (blockIdx.y): the per-nonant index loads of a scenario's
    // thread run in parallel instead of one dependent chain per nonant (config 2, 30
    // nonants: 27 us -> a few).  A row's blocks stride over the scenarios (UPD_U loads in
    // flight per thread), so that the grid stays near UPD_BLOCKS blocks: the last-block
    // ticket is one atomic counter, and config 4's 1,536 blocks (65,536 scenarios x 6
    // nonants) queued on it for about 20 us of a 27 us launch
    const int64_t S = st.S;
    const int k = blockIdx.y;
    double acc = 0.0;
    if (k < st.nn) {
        const int d = st.nonant_depth[k];
        const int off = st.nonant_off[k], col = st.nonant_col[k], nl = st.nlen_max;
        const int64_t stride = (int64_t)gridDim.x * blockDim.x;
        for (int64_t s0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s0 < S; s0 += UPD_U * stride) {
            double xb[UPD_U], xv[UPD_U], wo[UPD_U], rv[UPD_U];
            bool pz[UPD_U];
#pragma unroll
            for (int u = 0; u < UPD_U; ++u) {
                const int64_t s = s0 + u * stride;
                xb[u] = xv[u] = wo[u] = rv[u] = 0.0;
                pz[u] = false;
                if (s < S) {  // (a wave past S skips its loads: a small batch has one trip of one)
                    const int gnode = st.node_of[(int64_t)d * S + s];
                    xb[u] = node_buf[gnode * nl + off];
                    xv[u] = x[(int64_t)col * S + s];
                    wo[u] = update_W ? W[(int64_t)k * S + s] : 0.0;
                    rv[u] = update_W ? rho[(int64_t)k * S + s] : 0.0;
                    // (variable probabilities: W masked where the probability is 0, phbase.py:315-318)
                    pz[u] = update_W && st.pvar && st.pvar[(int64_t)k * S + s] == 0.0;
                }
            }
#pragma unroll
            for (int u = 0; u < UPD_U; ++u) {
                const int64_t s = s0 + u * stride;
                if (s < S) {
                    xbar[(int64_t)k * S + s] = xb[u];
                    if (update_W) W[(int64_t)k * S + s] = pz[u] ? 0.0 : wo[u] + rv[u] * (xv[u] - xb[u]);
                    acc += fabs(xv[u] - xb[u]);
                }
            }
        }
    }
    conv_last_block(acc, o);
}

// phgpu_ph_step_local (one rank, every nonant's scenarios on one node, nn <= XL_NN_MAX):
// the x̄ final sums and k_ph_update in one launch.  Every block sums the per-wave x̄ partials
// itself, in one fixed order (so every block gets the same bits), block 0 stores them in
// node_buf; then the scatter / W update / conv of k_ph_update (last-block reduction).  The
// partials are per wave (k_xbar_partial) or per chunk of the path-6 epilogue (st.part /
// st.nwaves then point at those; dirty chunks are recomputed from x).  Few, large blocks for
// a large batch (every block re-sums the partials), 256 threads for a small one.
__global__ void __launch_bounds__(XL_T)
k_ph_update_local(ph_tree st, const double* __restrict__ x, double* __restrict__ node_buf,
                  double* __restrict__ xbar, double* __restrict__ W, const double* __restrict__ rho,
                  int update_W, conv_sink o, const int32_t* __restrict__ dirty, int C) {
    __shared__ double sa[XL_T / WAVE][XL_NN_MAX], sb[XL_T / WAVE][XL_NN_MAX];
    __shared__ double xbs[XL_NN_MAX];
    const int64_t S = st.S;
    const int nn = st.nn;
    const int half = st.num_nodes * st.nlen_max;
    // every nonant at once: strided loads of the contiguous per-wave partials, wave sums,
    // then the block's waves in order (one barrier)
    // the scenario's own operands of the first XL_PF nonants, loaded ahead of the x̄ sums
    // (independent of them; the barrier below would keep them behind)
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t sc = s < S ? s : S - 1;
    double xv[XL_PF], wo[XL_PF], rv[XL_PF];
#pragma unroll
    for (int k = 0; k < XL_PF; ++k) {
        const int kk = k < nn ? k : 0;
        xv[k] = x[(int64_t)st.nonant_col[kk] * S + sc];
        wo[k] = update_W ? W[(int64_t)kk * S + sc] : 0.0;
        rv[k] = update_W ? rho[(int64_t)kk * S + sc] : 0.0;
    }
    double a[XL_NN_MAX], b[XL_NN_MAX];
#pragma unroll
    for (int k = 0; k < XL_NN_MAX; ++k) a[k] = b[k] = 0.0;
    for (int64_t w = threadIdx.x; w < st.nwaves; w += blockDim.x) {
        const double* pw = st.part + w * nn * 2;
        // the chunk's flag and partials in flight together (the flag gates the use only)
        const int dw = dirty ? dirty[w] : 0;
        double pa[XL_PF], pb[XL_PF];
#pragma unroll
        for (int k = 0; k < XL_PF; ++k) {
            pa[k] = k < nn ? pw[2 * k] : 0.0;
            pb[k] = k < nn ? pw[2 * k + 1] : 0.0;
        }
        if (dw) {  // a chunk with a fallback scenario (path-6 partials)
            for (int k = 0; k < nn; ++k) {
                double ra, rb;
                xp_recompute(st, x, w, C, k, ra, rb);
#pragma unroll
                for (int u = 0; u < XL_NN_MAX; ++u)
                    if (u == k) a[u] += ra, b[u] += rb;
            }
            continue;
        }
#pragma unroll
        for (int k = 0; k < XL_NN_MAX; ++k)
            if (k < nn) {
                a[k] += k < XL_PF ? pa[k < XL_PF ? k : 0] : pw[2 * k];
                b[k] += k < XL_PF ? pb[k < XL_PF ? k : 0] : pw[2 * k + 1];
            }
    }
    const int wv = threadIdx.x / WAVE;
#pragma unroll
    for (int k = 0; k < XL_NN_MAX; ++k)
        if (k < nn) {
            const double ta = wave_sum(a[k]), tb = wave_sum(b[k]);
            if ((threadIdx.x & (WAVE - 1)) == 0) {
                sa[wv][k] = ta;
                sb[wv][k] = tb;
            }
        }
    __syncthreads();
    if (threadIdx.x < nn) {
        const int k = threadIdx.x;
        double ta = 0.0, tb = 0.0;
        const int nwb = (int)(blockDim.x / WAVE);
        for (int u = 0; u < nwb; ++u) {
            ta += sa[u][k];
            tb += sb[u][k];
        }
        xbs[k] = ta;
        if (blockIdx.x == 0) {
            const int g0 = st.node_of[(int64_t)st.nonant_depth[k] * S];
            node_buf[g0 * st.nlen_max + st.nonant_off[k]] = ta;
            node_buf[half + g0 * st.nlen_max + st.nonant_off[k]] = tb;
        }
    }
    __syncthreads();
    double acc = 0.0;
    if (s < S) {
#pragma unroll
        for (int k = 0; k < XL_PF; ++k)
            if (k < nn) {
                const double xb = xbs[k];
                xbar[IX(k)] = xb;
                if (update_W) W[IX(k)] = wo[k] + rv[k] * (xv[k] - xb);
                acc += fabs(xv[k] - xb);
            }
        for (int k = XL_PF; k < nn; ++k) {
            const double xb = xbs[k];
            const double xw = x[IX(st.nonant_col[k])];
            xbar[IX(k)] = xb;
            if (update_W) W[IX(k)] += rho[IX(k)] * (xw - xb);
            acc += fabs(xw - xb);
        }
    }
    conv_last_block(acc, o);
}

// spopt.py:310-439 local sums: prob*obj, prob*bound, prob, prob*feasible, prob*optimal.
__global__ void __launch_bounds__(BLOCK)
k_expect_partial(ph_tree st, const double* __restrict__ obj, const double* __restrict__ bound,
                 const int32_t* __restrict__ status) {
    const int64_t S = st.S;
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (s < S) {
        const double p = st.prob[s];
        v[0] = p * obj[s];
        v[1] = p * bound[s];
        v[2] = p;
        v[3] = (status[s] == PHGPU_OPTIMAL || status[s] == PHGPU_ITER_LIMIT) ? p : 0.0;
        v[4] = (status[s] == PHGPU_OPTIMAL) ? p : 0.0;
    }
#pragma unroll
    for (int t = 0; t < 5; ++t) {
        const double a = wave_sum(v[t]);
        if ((threadIdx.x & (WAVE - 1)) == 0) st.part[(s / WAVE) * 5 + t] = a;
    }
}

// Deterministic ordered sum of K interleaved per-wave partials: out[k] = sum_w part[w*K+k].
// With stats_src / stats_dst (phgpu_ph_update_ex) block 0 also copies a solve's six
// statistics (a store to host memory here saves a copy launch per PH iteration).
__global__ void __launch_bounds__(256) k_sum_partials(const double* __restrict__ part, int64_t nw, int K,
                                                     double scale, double* __restrict__ out,
                                                     const unsigned long long* __restrict__ stats_src = nullptr,
                                                     int64_t* __restrict__ stats_dst = nullptr) {
    __shared__ double sh[256];
    const int k = blockIdx.x;
    if (stats_dst && k == 0 && threadIdx.x < 6) stats_dst[threadIdx.x] = (int64_t)stats_src[threadIdx.x];  // (one copy)
    double a = 0.0;
    for (int64_t w = threadIdx.x; w < nw; w += 256) a += part[w * K + k];
    sh[threadIdx.x] = a;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[k] = sh[0] * scale;
}
