// Host side of the PDHG solve paths 4, 3, 2 and 1: one launcher each (launch_stream, launch_wg,
// launch_reg, launch_global; paths 5 and 6 have jit_* and ipm_* next to their kernels), the
// pieces they share, and what phgpu_solve and phgpu_ph_loop share around a launch.  Included
// by phgpu.hip above solve_impl; host code only.

static solve_params make_solve_params(const phgpu_options& o, int warm) {
    solve_params P;
    P.eps_rel = o.eps_rel;
    P.eps_abs = o.eps_abs;
    P.gamma = o.gamma;
    P.bsuff = o.beta_sufficient;
    P.bnec = o.beta_necessary;
    P.bart = o.beta_artificial > 0.0 ? o.beta_artificial : 1e300;
    P.restart_every = o.restart_every;
    P.eta_frac = o.eta_frac;
    P.omega0 = o.omega0;
    P.max_iter = o.max_iter;
    P.check_every = o.check_every;
    P.warm = warm;
    P.keep_omega = o.keep_omega;
    P.infeas_start = o.infeas_start;
    P.eps_inf = o.eps_infeas;
    P.wmax = o.omega_clamp > 1.0 ? o.omega_clamp : 1e300;
    P.wmin = 1.0 / P.wmax;
    return P;
}

// The bookkeeping after a launched solve: the warm state it wrote (in the records if out_rec)
// is current now, or at phgpu_commit if deferred.
static void solve_done(phgpu_state* h, int path, int out_rec, int defer, const int32_t* status, const int32_t* iters) {
    const int wq = h->wq;
    h->last_status = status;
    h->last_iters = iters;
    if (path != 6) h->xp_C[wq] = 0;  // only path 6 writes x̄ partials with its outputs
    h->have_s[wq] = 1;
    h->warm_rec_s[wq] = out_rec;
    h->last_path = path;
    if (defer) h->pending = wq;
    else h->wslot = wq;
    h->wq = h->wslot;
    bind_slots(h);
}

// workgroups per CU of a solve kernel, at least 1 (queried once: occ_cache[slot])
static int occ_per_cu(phgpu_state* h, int slot, const void* fn, int threads, size_t lds, int* per_cu) {
    int& oc = h->occ_cache[slot];
    if (!oc) HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&oc, fn, threads, lds));
    *per_cu = oc < 1 ? 1 : oc;
    return 0;
}

// the records exist and hold the scaled problem
static int records_ready(phgpu_state* h, hipStream_t st) {
    if (h->pk) return 0;
    const int rc = pack_alloc(h);
    if (rc) return rc;
    if (h->scen_set) HIPCHK(pack_fill(h, st));
    return 0;
}

// a warm start left in x / y by another path into the records, and one left in the records out
static int warm_to_records(phgpu_state* h, const solve_params& P, hipStream_t st) {
    if (!P.warm || h->warm_rec) return 0;
    HIPCHK(to_records(h, h->x, h->n, h->pk_X, st));
    HIPCHK(to_records(h, h->y, h->m, h->pk_Y, st));
    return 0;
}
static int warm_from_records(phgpu_state* h, const solve_params& P, hipStream_t st) {
    if (!P.warm || !h->warm_rec) return 0;
    HIPCHK(from_records(h, h->pk_X, -1, h->n, h->x, st));
    HIPCHK(from_records(h, h->pk_Y, -1, h->m, h->y, st));
    return 0;
}

// outputs in the caller's scenario-fastest layout, unscaled
static int outputs_from_records(phgpu_state* h, double* x, double* y, hipStream_t st) {
    HIPCHK(from_records(h, h->pk_XW, h->pk_DC, h->n, x, st));
    if (y) HIPCHK(from_records(h, h->pk_YW, h->pk_DR, h->m, y, st));
    return 0;
}

// path 4 (solve_stream.inc): the streaming kernel of a shared-matrix handle
static int launch_stream(phgpu_state* h, const solve_params& P, double* x, double* y, double* obj, double* bound,
                         int32_t* status, int32_t* iters, hipStream_t st, int split_longest) {
    // B scenario slots per workgroup (PHGPU_STREAM_SLOTS=1|2, default 2)
    const char* env = getenv("PHGPU_STREAM_SLOTS");
    const int B = (env && atoi(env) == 1) ? 1 : 2;
    const void* fn = B == 1 ? (const void*)k_solve_stream<1> : (const void*)k_solve_stream<2>;
    int per_cu = 0;
    {
        const int rc = occ_per_cu(h, B == 1 ? 4 : 5, fn, SBLK, 0, &per_cu);
        if (rc) return rc;
    }
    // PHGPU_STREAM_PER_CU=k: launch k workgroups per CU whatever the occupancy query says
    // (the ones that do not fit wait for a free CU; the queue has no other dependency)
    const char* pce = getenv("PHGPU_STREAM_PER_CU");
    if (pce && atoi(pce) > 0) per_cu = std::min(atoi(pce), 8);
    int64_t nblk = (int64_t)per_cu * h->num_cus;
    if (nblk > (h->S + B - 1) / B) nblk = (h->S + B - 1) / B;
    // PHGPU_STREAM_SPLIT=T: the T longest scenarios of the previous solve run first, each
    // over the whole GPU (the split form of k_solve_stream, cooperative launch), then the
    // rest on the queue (DESIGN.md 3.5)
    const char* spe = getenv("PHGPU_STREAM_SPLIT");
    int T = split_longest > 0 ? split_longest : (spe ? atoi(spe) : 0);
    if (T < 0) T = 0;
    if (T > 16) T = 16;
    if (T > h->S) T = (int)h->S;
    HIPCHK(hipMemsetAsync(h->qhead, 0, sizeof(int), st));
    // queue order: longest first by the previous solve's iteration counts (the launch
    // ends with its slowest scenario; starting it first shortens the tail)
    if (!h->have_solution) HIPCHK(hipMemsetAsync(h->sk_iters, 0, (size_t)h->S * sizeof(int32_t), st));
    if (h->S <= STREAM_ORDER_MAX)
        hipLaunchKernelGGL(k_stream_order, dim3((unsigned)((h->S + 255) / 256)), dim3(256), 0, st, *h);
    else
        hipLaunchKernelGGL(k_stream_order_identity, dim3((unsigned)((h->S + 255) / 256)), dim3(256), 0, st, *h);
    int occ = 0;
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void*)k_solve_stream<1, true>, SBLK, 0));
    const int64_t cap = (int64_t)std::max(occ, 1) * h->num_cus;
    // enough waves for one slice each in the longer pass: no more workgroups per scenario
    const int kmax = std::max((std::max(h->nsl_c, h->nsl_r) + SWAVES - 1) / SWAVES, 1);
    // the cluster form for a batch smaller than the GPU (a rank's share of a strong-
    // scaling run): every scenario over K = capacity / S workgroups at once instead of
    // one scenario per workgroup on a few CUs (PHGPU_STREAM_CLUSTER=0: off, =K: that K)
    int Kc = 0;
    {
        const char* ce = getenv("PHGPU_STREAM_CLUSTER");
        const int ask = ce ? atoi(ce) : -1;
        if (ask != 0 && T == 0) {
            int64_t k = cap / std::max<int64_t>(h->S, 1);
            if (ask > 1) k = std::min<int64_t>(ask, k);
            k = std::min<int64_t>(k, kmax);
            if (k >= 2) Kc = (int)k;
        }
    }
    if (T > 0 || Kc >= 2) {
        // the split form: T stragglers over the whole grid (one cluster), or S clusters of Kc
        const int ncl = Kc >= 2 ? (int)h->S : 1;
        int G = Kc >= 2 ? (int)h->S * Kc : (int)std::min<int64_t>(kmax, cap);
        G = std::max(G, 1);
        const size_t need = (size_t)2 * G * 8 + (size_t)16 * ncl;  // partials, then 128-B barrier counters
        if (h->split_need < need) {
            dfree(h, &h->split_part);
            h->split_need = 0;
            const int rc = dalloc(h, &h->split_part, need, false);
            if (rc) return rc;
            h->split_need = need;
        }
        // the barrier counters start at gbase (PHGPU_SPLIT_BAR_BASE: a test starts them just
        // below 2^32 so that they wrap during the launch; the barrier compares wrap-safe)
        const char* bbe = getenv("PHGPU_SPLIT_BAR_BASE");
        unsigned gbase = bbe ? (unsigned)strtoul(bbe, nullptr, 0) : 0u;
        HIPCHK(hipMemsetD32Async((hipDeviceptr_t)(h->split_part + (size_t)2 * G * 8), (int)gbase, (size_t)32 * ncl, st));
        pdhg_view hv = *h;  // k_solve_stream's first parameter: the argument array passes addresses
        solve_params Pv = P;
        int32_t* qh = h->qhead;
        double* gp = h->split_part;
        int q0 = Kc >= 2 ? (int)h->S : T;
        int nc = ncl;
        void* args[] = {&hv, &Pv, &qh, &x, &y, &obj, &bound, &status, &iters, &q0, &gp, &gbase, &nc};
        HIPCHK(hipLaunchCooperativeKernel((const void*)k_solve_stream<1, true>, dim3((unsigned)G), dim3(SBLK), args,
                                          0, st));
        h->last_cluster = Kc >= 2 ? Kc : 0;
    } else {
        h->last_cluster = 0;
    }
    if (Kc < 2) {
        nblk = std::min<int64_t>(nblk, std::max<int64_t>((h->S - T + B - 1) / B, 1));
        if (B == 1)
            hipLaunchKernelGGL(k_solve_stream<1>, dim3((unsigned)nblk), dim3(SBLK), 0, st, *h, P, h->qhead, x, y, obj,
                               bound, status, iters, T, (double*)nullptr, 0u, 1);
        else
            hipLaunchKernelGGL(k_solve_stream<2>, dim3((unsigned)nblk), dim3(SBLK), 0, st, *h, P, h->qhead, x, y, obj,
                               bound, status, iters, T, (double*)nullptr, 0u, 1);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// path 3 (solve_wg.inc): one workgroup per scenario on the records
static int launch_wg(phgpu_state* h, const solve_params& P, double* x, double* y, double* obj, double* bound,
                     int32_t* status, int32_t* iters, hipStream_t st) {
    int rc = records_ready(h, st);
    if (rc) return rc;
    // this solve's PH state into the records; a warm start left by another path too
    HIPCHK(ph_to_records(h, st));
    rc = warm_to_records(h, P, st);
    if (rc) return rc;
    const wg_instance& gi = g_wg_instances[h->wg_inst];
    wg_plan pl;
    pl.L = WAVE * gi.WPS;
    pl.kc = gi.KC;
    pl.zc = gi.ZC;
    pl.kr = gi.KR;
    pl.zr = gi.ZR;
    pl.col_id = h->wg_col_id;
    pl.row_id = h->wg_row_id;
    pl.col_long = h->wg_col_long;
    pl.row_long = h->wg_row_long;
    pl.col_k = h->wg_col_k;
    pl.col_r = h->wg_col_r;
    pl.row_k = h->wg_row_k;
    pl.row_c = h->wg_row_c;
    const size_t lds = wg_lds_doubles(h->n, h->m, gi.KC, gi.KR, gi.WPS) * sizeof(double);
    int per_cu = 0;
    rc = occ_per_cu(h, 3, (const void*)gi.fn, pl.L, lds, &per_cu);
    if (rc) return rc;
    int64_t nblk = (int64_t)per_cu * h->num_cus;
    if (nblk > h->S) nblk = h->S;
    HIPCHK(hipMemsetAsync(h->qhead, 0, sizeof(int), st));
    hipLaunchKernelGGL(gi.fn, dim3((unsigned)nblk), dim3(pl.L), lds, st, *h, P, pl, h->qhead, x, y, obj, bound,
                       status, iters);
    HIPCHK(hipGetLastError());
    return outputs_from_records(h, x, y, st);
}

// path 2 (solve_reg.inc): the register-resident kernel, in scenario order or in record mode
// (h->last_rec says which it took)
static int launch_reg(phgpu_state* h, const solve_params& P, double* x, double* y, double* obj, double* bound,
                      int32_t* status, int32_t* iters, hipStream_t st) {
    const int G = WAVE / h->reg_L;
    const reg_instance& ri = g_reg_instances[h->reg_inst];
    const size_t lds = (size_t)REG_WPB * reg_wave_lds(h->n, h->m, G, ri.KC, ri.KR) * sizeof(double);
    // persistent grid: co-resident workgroups of REG_WPB independent waves (occupancy
    // x CUs), never more than there are scenario groups
    const int64_t need = (h->S + (int64_t)G * REG_WPB - 1) / ((int64_t)G * REG_WPB);
    int per_cu = 0;
    int rc = occ_per_cu(h, 2, (const void*)ri.fn, WAVE * REG_WPB, lds, &per_cu);
    if (rc) return rc;
    int64_t nblk = std::min<int64_t>((int64_t)per_cu * h->num_cus, need);
    // record mode (solve_reg.inc, template REC) when groups take more than one scenario
    // each: then the queue order matters (PHGPU_REG_REC=0|1 pins it)
    const char* env = getenv("PHGPU_REG_REC");
    const bool rec = env ? atoi(env) != 0 : nblk * REG_WPB * G < h->S;
    const reg_kernel_t fn = rec ? ri.fn_rec : ri.fn;
    if (rec) {
        rc = occ_per_cu(h, 6, (const void*)ri.fn_rec, WAVE * REG_WPB, lds, &per_cu);
        if (rc) return rc;
        nblk = std::min<int64_t>((int64_t)per_cu * h->num_cus, need);
    }
    const int64_t first_dyn = nblk * REG_WPB * G;
    if (rec) {
        rc = records_ready(h, st);
        if (!rc) rc = warm_to_records(h, P, st);
        if (rc) return rc;
        if (!h->have_solution) HIPCHK(hipMemsetAsync(h->sk_iters, 0, (size_t)h->S * sizeof(int32_t), st));
        const dim3 ob((unsigned)((h->S + ORDER_BINS - 1) / ORDER_BINS));
        int32_t* bins = h->sk_bins + 2 * ORDER_BINS * h->order_parity;
        int32_t* other = h->sk_bins + 2 * ORDER_BINS * (1 - h->order_parity);
        h->order_parity ^= 1;
        // histogram + this solve's PH state into the records, one launch (k_reg_prep)
        const bool ph = h->nn > 0 && (h->W_on || h->prox_on);
        const int nh = (int)ob.x;
        const int gx = (int)((h->S + TT - 1) / TT), gy = ph ? (3 * h->nn + TT - 1) / TT : 0;
        hipLaunchKernelGGL(k_reg_prep, dim3((unsigned)(nh + gx * gy)), dim3(256), 0, st, h->sk_iters, h->S,
                           P.restart_every, bins, nh, gx, h->W_on ? h->W : nullptr,
                           h->prox_on ? h->rho : nullptr, h->prox_on ? h->xbar : nullptr, h->nn, h->pk,
                           h->pk_stride, h->pk_W);
        hipLaunchKernelGGL(k_reg_order, ob, dim3(ORDER_BINS), 0, st, h->sk_iters, h->S, P.restart_every, bins,
                           other, h->sk_order, h->qhead);
    } else {
        rc = warm_from_records(h, P, st);
        if (rc) return rc;
    }
    reg_plan pl;
    pl.L = h->reg_L;
    pl.kc = h->reg_kc;
    pl.zc = h->reg_zc;
    pl.kr = h->reg_kr;
    pl.zr = h->reg_zr;
    pl.col_k = h->pl_col_k;
    pl.col_r = h->pl_col_r;
    pl.row_k = h->pl_row_k;
    pl.row_c = h->pl_row_c;
    pl.order = h->sk_order;
    pl.last_iters = h->sk_iters;
    pl.last_iters_w = h->its_w;
    pl.ema = h->have_solution ? 1 : 0;
    if (!rec) HIPCHK(hipMemsetAsync(h->qhead, 0, sizeof(int), st));  // record mode: k_reg_order did
    hipLaunchKernelGGL(fn, dim3((unsigned)nblk), dim3(WAVE * REG_WPB), lds, st, *h, P, pl, h->qhead, first_dyn,
                       x, y, obj, bound, status, iters);
    HIPCHK(hipGetLastError());
    if (rec) {
        rc = outputs_from_records(h, x, y, st);
        if (rc) return rc;
    }
    h->last_rec = rec ? 1 : 0;
    return 0;
}

// path 1: the global-memory kernel, one lane per scenario
static int launch_global(phgpu_state* h, const solve_params& P, double* x, double* y, double* obj, double* bound,
                         int32_t* status, int32_t* iters, hipStream_t st) {
    hipLaunchKernelGGL(k_solve, grid_for(h->S), dim3(BLOCK), 0, st, *h, P, x, y, obj, bound, status, iters);
    HIPCHK(hipGetLastError());
    return 0;
}
