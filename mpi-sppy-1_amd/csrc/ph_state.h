// ph_state.h -- the handle behind phgpu_handle: what the kernels see of it, what only the host
// keeps, and who owns its device memory.  Included by phgpu.hip after set_err.
//
// The handle is built in layers by single inheritance, so a field has one name everywhere
// (h->S on the host, st.S in a kernel).  A kernel declares the smallest device layer that holds
// what its family reads and the launcher passes *h, which slices to it:
//   ph_tree                 the scenario tree and the reduction partials (the PH-side kernels)
//   ph_data    : ph_tree    the problem as set up (the kernels that read or fill problem data)
//   pdhg_view  : ph_data    the iterates, PH terms and streaming tables of the PDHG solve kernels
//   phgpu_state : pdhg_view everything else, host only: no kernel or device function names it
// A buffer the device does not read goes in phgpu_state; one that a single kernel reads is
// passed to it as an argument; only what a whole family reads belongs in a device layer.
#pragma once
#include <type_traits>

// ------------------------------------------------------------------ state
struct jit_module;  // solve_jit.inc: the hipRTC-compiled path-5 kernel of a handle
struct ipm_module;  // solve_ipm.inc: the hipRTC-compiled path-6 module of a handle
struct fwph_store;  // ph_fwph.inc: the FWPH column store of a handle
struct sel_state;   // ph_aph.inc: the workspace of phgpu_select_smallest
struct ls_store;    // ph_lshaped.inc: the cut store and master of the L-shaped method
struct ef_store;    // ph_ef.inc: the iterate and work space of the extensive-form interior point
struct bd_store;    // phgpu.hip: the segmented form of it, one extensive form per bundle
struct eft_store;   // phgpu.hip: the multistage form of it, eliminated along the tree (ph_ef_tree.inc)
struct ph_ws {      // a reduction's device workspace: partials, and node tags or a ticket counter
    double* part;
    int32_t* tag;
};

// the scenario tree: sizes, the nonant maps, probabilities and the x̄ partials
struct ph_tree {
    int64_t S;
    int nn, depth, num_nodes, nlen_max;
    int32_t *nonant_col, *nonant_depth, *nonant_off, *nonant_slot;
    int32_t* node_of;
    double *prob, *pcoef;
    // per-nonant probability coefficients ([nn][S], caller-owned; null: the per-node pcoef),
    // the variable probabilities of spbase.py:394-424 (phgpu_set_nonant_probs)
    const double* pvar;
    // reductions
    double* part;       // [nwaves * max(2*nn, 5)]
    int32_t* part_node; // [nwaves * nn]
    int64_t nwaves;
};

// the problem as set up: the shared pattern, the scenarios' data and its scaled copies
struct ph_data : ph_tree {
    int n, m, nnz;
    // shared pattern
    int32_t *row_ptr, *col_idx, *col_ptr, *row_idx, *perm, *row_of;
    // per-scenario problem data (library copies)
    double *A, *c, *lb, *ub, *rl, *ru, *q, *objc;
    // scaling
    double *Ah_csr, *Ah_csc, *Dr, *Dc, *normA;
    double *lbh, *ubh, *rlh, *ruh;
    // shared-matrix handle (PHGPU_SHARED_MATRIX, path 4: solve_stream.inc): one scaled A
    // (A / Ah_csr / Ah_csc [nnz], Dr [m], Dc [n]) for all scenarios; the shared base of
    // the column / row data (sh_col: ch qh lbh ubh, sh_row: rlh ruh rl ru, scenario 0);
    // per-scenario columns P (cmap[j] = index or -1, pcol) and rows R (rmap, prow)
    int shared;
    int np, nr;
    int32_t *cmap, *rmap, *pcol, *prow;
    double *sh_col, *sh_row, *sh_norm;
    // scenario-major records of the workgroup path: one contiguous record
    // per scenario, so a workgroup loads / writes back its scenario in full lines; here the
    // offsets of the problem data in a record
    double* pk;
    int64_t pk_stride;
    int pk_A, pk_C, pk_Q, pk_DC, pk_LB, pk_UB, pk_RL, pk_RU, pk_DR, pk_RLH, pk_RUH;
    // stream records: X X0 U XT | Y Y0 YT | PC (8 per P column) | PR (4 per R row); here the
    // problem data's part
    double* sk;
    int64_t sk_stride, sk_PC, sk_PR;
};

// what the PDHG solve kernels (paths 1 to 4) and the setup kernels read besides
struct pdhg_view : ph_data {
    // per-solve effective objective (scaled) + iterates (scaled)
    double *ch, *qh;
    double *x, *x0, *xe, *xt, *aty, *aty0, *y, *y0, *yt;
    double* omega;
    // the iterates and PH terms in the records pk and the iterates in the records sk
    int pk_X, pk_Y, pk_W, pk_RHO, pk_XB;
    int64_t sk_X, sk_X0, sk_U, sk_XT, sk_Y, sk_Y0, sk_YT;
    // sliced-ELL copies of the scaled matrix for the two streaming passes: slice = 64
    // consecutive columns (rows), padded to its longest; entry k of slice member l at
    // off[slice] + 64 k + l (coalesced)
    int nsl_c, nsl_r;
    int32_t *cs_off, *cs_len, *cs_idx, *rs_off, *rs_len, *rs_idx;
    double *cs_val, *rs_val;
    // slices of each pass per wave of the streaming workgroup (balanced by entries):
    // wave w takes cw_slc[cw_ptr[w] .. cw_ptr[w+1]) (rw_* for rows)
    int32_t *cw_ptr, *cw_slc, *rw_ptr, *rw_slc;
    int32_t *sk_iters, *sk_order;  // PDHG iterations of the last solve / longest-first queue order
    // PH state (caller-owned)
    const double *W, *rho, *xbar;
    int W_on, prox_on;
    // where a solve writes its warm state (the warm-start slots of phgpu_state)
    double *xw, *yw, *omega_w;
    int pk_XW, pk_YW;
};

// Each bound is the layer's size rounded up to a multiple of 64: it bounds the kernel-argument
// segment a kernel taking that layer spends on it (4 KB per kernel at most).
static_assert(std::is_trivially_copyable<ph_tree>::value && sizeof(ph_tree) <= 128, "ph_tree is a kernel argument");
static_assert(std::is_trivially_copyable<ph_data>::value && sizeof(ph_data) <= 512, "ph_data is a kernel argument");
static_assert(std::is_trivially_copyable<pdhg_view>::value && sizeof(pdhg_view) <= 896,
              "pdhg_view is a kernel argument");

// the handle: the device layers and the host's bookkeeping
struct phgpu_state : pdhg_view {
    int device;
    void* rccl[2];                 // the library's RCCL communicators over the ranks (comm_rccl.inc), or null
    int64_t ws_bytes;
    // register-resident path (solve_reg.inc): lane plan, -1 instance = unavailable
    int reg_inst;
    int reg_L, reg_kc, reg_zc, reg_kr, reg_zr;
    int32_t *pl_col_k, *pl_col_r, *pl_row_k, *pl_row_c;
    // workgroup-per-scenario path (solve_wg.inc): -1 instance = unavailable
    int wg_inst, wg_long;
    int32_t *wg_col_id, *wg_row_id, *wg_col_long, *wg_row_long, *wg_col_k, *wg_col_r, *wg_row_k, *wg_row_c;
    int default_kernel;  // 1 global, 2 register (L <= 64), 3 workgroup per scenario
    int last_path;       // path of the last solve (whose layout holds the warm start)
    int scen_set;
    // 1 if some wave of local scenarios spans two nodes at a nonant's depth (its x̄
    // contributions go to node_buf by atomics, so node_buf is cleared by a memset first);
    // 0 if none does (k_xbar_partial clears node_buf itself); -1 not yet known
    int xbar_mixed;
    // 1 if every nonant's local scenarios share one node (two-stage problems): a single
    // rank's x̄ final sum can then be folded into the update kernel (phgpu_ph_step_local)
    int xbar_single;
    int* qhead;  // work-queue head of the persistent solve kernel
    int num_cus;
    int occ_cache[8];  // workgroups per CU of each solve kernel (0 = not queried yet)
    // shared-matrix handle: the power iteration's vectors and partials
    double *sh_v, *sh_u, *sh_w, *sh_part;
    // sliced-ELL copies: their entries, and the CSC / CSR position of each entry (-1 = pad)
    int nent_c, nent_r;
    int32_t *cs_src, *rs_src;
    double* split_part;            // grid-sum partials of the split streaming form ([ncl][2][K][8]) + barriers
    size_t split_need;             // its size in doubles
    int last_cluster;              // path 4: workgroups per scenario of the last solve's cluster form (0: none)
    int32_t* sk_bins;              // [2 parities][2][ORDER_BINS] counting-sort histogram / fill counters (path 2)
    int order_parity;              // which half of sk_bins the next register-path solve uses
    int warm_rec;                  // the warm start lives in the records pk (paths 2r, 3), else in x / y
    int last_rec;                  // queue mode of the last register-path solve (-1 none yet)
    int64_t sk_cap;
    int have_solution;
    // Warm-start slots (include/phgpu.h phgpu_solve_deferred / phgpu_commit).  The warm
    // state a solve starts from -- the iterate x / y ([k][S] arrays or the records' x^ / y^
    // fields), the primal weight omega and the queue predictor sk_iters -- lives in slot
    // wslot; the fields x, y, omega, sk_iters, pk_X, pk_Y, have_solution and warm_rec
    // are bound to it at the start of every solve.  A solve writes its warm state to the
    // *_w targets (xw, yw, omega_w, its_w, pk_XW, pk_YW): the same slot, or the other one for
    // a deferred (speculative) solve, which becomes current only at phgpu_commit.
    double *xs[2], *ys[2], *oms[2];
    int32_t* its_s[2];
    int pkXs[2], pkYs[2];
    int have_s[2], warm_rec_s[2];
    int wslot, wq;       // read slot / write slot of the current solve
    int pending;         // slot of an uncommitted deferred solve, -1 none
    int32_t* its_w;
    // path 5 (solve_jit.inc): the pattern-specialised module, and whether the column /
    // row kinds it was built for still describe the data (reset by phgpu_set_scenarios)
    jit_module* jit;
    int jit_kinds_valid;
    // path 6 (solve_ipm.inc): the interior-point module; whether the data flags it was
    // built for still hold (reset by phgpu_set_scenarios); factor entries of the pattern
    // (0: not eligible); 1 once a compiled module spilled (path 6 is then not the
    // default); the fallback list [S] and its counters {fail_n[2], qhead[2]} by parity
    ipm_module* ipm;
    // phgpu_ph_loop: the IPM_LOOP module (built on first use from the one-lane source) and its
    // buffers {gpart [blocks * 16], gpub [16], conv_hist [cap] | gsync [2], loop_out [2],
    // loop_its [PHGPU_STATS_WORDS]}
    ipm_module* ipm_loop;
    double* loop_dbl;
    int64_t loop_dbl_n;
    unsigned long long* loop_cnt;
    int ipm_flags_valid, ipm_nf, ipm_off, ipm_parity, ipm_spill1;
    // the one-lane module's slack reciprocals in LDS (IPM_LDS_ISL, solve_ipm.inc ipm_prepare):
    // 0 not tried, 1 on (its module spills less), -1 tried and not kept; with the spill
    // bytes of the register-only module it was compared with
    int ipm_lds, ipm_lds_ref;
    int ipm_wave;  // waves per scenario of the workgroup IPMs for medium scenarios (0: not eligible;
                   // jit_ipm_blk.hip.in for block-angular patterns, else jit_ipm_wave.hip.in)
    int32_t *ipm_list, *ipm_cnt;
    // solve statistics (phgpu_solve_stats): path 6 accumulates them in its kernels (by
    // parity, [2][8]); other paths get them from k_solve_stats over the last solve's
    // status / iters outputs into stats_gen[8].  last_stats: where the last solve's are
    // (null: compute on request)
    // ipm_stats: two parities of PHGPU_STATS_COPIES copies of the 8 statistics words (the
    // path-6 kernels spread their per-wave atomics over the copies, stats_word sums them)
    unsigned long long *ipm_stats, *stats_gen, *last_stats;
    unsigned long long* ipm_prof;  // PHGPU_IPM_PROF: per-wave timelines of IPM_PROF modules
    long long ipm_prof_n;
    const int32_t *last_status, *last_iters;
    // x̄ partial sums written by the path-6 kernels' epilogue, per warm slot:
    // [chunks * nn * 2] sums of pcoef x and pcoef x^2, node tags [chunks * nn], fallback
    // flags [chunks]; valid for the x buffer xp_x[slot] when xp_C[slot] (the chunk size) > 0
    double* xp[2];
    int32_t *xp_node[2], *xp_dirty[2];
    const double* xp_x[2];
    int xp_C[2];
    int64_t xp_n[2];
    // the update kernels' last-block reduction of conv: per-block partials and a counter
    double* cpart_blk;
    int32_t* blk_cnt;
    // a one-rank PH step deferred by phgpu_ph_step_defer: folded into the next path-6
    // deferred solve's prologue (jit_ph_step.hip.in) when it can be, else run by
    // phgpu_ph_step_local before that solve or before any other call
    struct ph_pending {
        int active;
        const double* x;
        double *node_buf, *xbar, *W;
        const double* rho;
        int update_W;
        double* conv;
        int64_t* stats;
        hipStream_t stream;
    } pend;
    int fuse_now;      // ipm_launch folds pend into this launch
    int64_t folded;    // PH steps folded into solve launches so far (phgpu_ipm_info)
    int32_t* nb_idx;   // [nn] node_buf index (node of the local scenarios, offset) of nonant k (two-stage)
    // Reduction workspaces, each its entry point's own and allocated at that entry's first call
    // (part / part_node may belong to a deferred step or to the path-6 epilogue; separate
    // allocations, so that calls on different streams may overlap); their kernels take them as
    // arguments.  Per-wave partials [nwaves * nn * planes] with node tags [nwaves * nn]: rs
    // phgpu_ph_residuals (4 planes), ns phgpu_nonant_stats (4), rr phgpu_rho_ratio_stats (3).
    // Per-block partials with a last-block counter as tag[0]: nc phgpu_nonant_closest
    // ((distance, index) pairs [2 * blocks]), wd phgpu_w_diff ([WD_BLOCKS]).
    ph_ws rs, ns, nc, wd, rr;
    // phgpu_fixer_step: the local scenarios of every node entry [num_nodes * nlen_max] and behind
    // them the newly fixed counts of a call in flight (zero between calls), allocated at its
    // first call; the former counted again after new scenario data (fx_valid 0)
    int32_t* fx_nloc;
    int fx_valid;
    // phgpu_fwph_*: the column store (host record of its device buffers; null until
    // phgpu_fwph_init) and the per-block partials and ticket of phgpu_fwph_diff
    fwph_store* fw;
    ph_ws fwd;
    // phgpu_aph_*: the per-wave partials of phgpu_aph_reduce (3 planes), the per-block partials
    // and tickets of phgpu_aph_norms and phgpu_aph_update; phgpu_select_smallest's workspace;
    // the list length of phgpu_solve_list on the device.  Each allocated at its entry's first call.
    ph_ws apr, apn, apu;
    sel_state* sel;
    int32_t* list_n;
    // phgpu_lshaped_*: the cut store, the master's data and work space (host record of its
    // device buffers; null until phgpu_lshaped_init)
    ls_store* ls;
    // phgpu_ef_*: the extensive-form interior point's iterate, factors and work space (host record
    // of its device buffers; null until phgpu_ef_init)
    ef_store* ef;
    // phgpu_bundle_*: the segmented extensive-form interior point (one segment per bundle; host
    // record of its device buffers; null until phgpu_bundle_init)
    bd_store* bd;
    // phgpu_eft_*: the multistage extensive-form interior point (host record of its device buffers;
    // null until phgpu_eft_init)
    eft_store* eft;
    // phgpu_gap_moments: two slots of GM_NV partials per wave (its head and its tail run) and
    // their segment tags [2 * nwaves], allocated at its first call
    ph_ws gm;
};

// ------------------------------------------------------------------ ownership (host)
// What phgpu_create2 allocates and phgpu_destroy deletes: the state and what only the host
// needs besides.  Every device buffer of the handle comes from dalloc and is in allocs until
// dfree or phgpu_destroy frees it; the counted ones make up phgpu_workspace_bytes (DESIGN.md
// 3.16).
struct dev_alloc {
    void* p;
    size_t bytes;
    bool counted;
};
struct phgpu_owner : phgpu_state {
    std::vector<dev_alloc> allocs;
    std::string ipm_tuning;  // phgpu_set_ipm_tuning's definitions, normalised ("" none)
};
static inline phgpu_owner* owner_of(phgpu_state* h) { return static_cast<phgpu_owner*>(h); }

template <typename T>
static int dalloc(phgpu_state* h, T** p, size_t count, bool counted = true) {
    *p = nullptr;
    if (count == 0) count = 1;
    const size_t bytes = count * sizeof(T);
    hipError_t e = hipMalloc((void**)p, bytes);
    if (e != hipSuccess) return set_err(-3, "hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
    owner_of(h)->allocs.push_back({(void*)*p, bytes, counted});
    if (counted) h->ws_bytes += (int64_t)bytes;
    return 0;
}

// free one buffer of the handle (null: nothing), give its bytes back if it was counted
template <typename T>
static void dfree(phgpu_state* h, T** p) {
    if (!*p) return;
    std::vector<dev_alloc>& v = owner_of(h)->allocs;
    for (size_t i = v.size(); i-- > 0;)
        if (v[i].p == (void*)*p) {
            if (v[i].counted) h->ws_bytes -= (int64_t)v[i].bytes;
            v[i] = v.back();
            v.pop_back();
            break;
        }
    (void)hipFree((void*)*p);
    *p = nullptr;
}

#define ALLOC(ptr, cnt)                         \
    do {                                        \
        int rc_ = dalloc(h, &(ptr), (size_t)(cnt)); \
        if (rc_) { phgpu_destroy(h); return rc_; } \
    } while (0)

// a host vector on the device: a (counted) buffer of the handle and the copy into it
template <typename T>
static int dupload(phgpu_state* h, T** d, const std::vector<T>& v, const char* what) {
    const int rc = dalloc(h, d, v.size());
    if (rc) return rc;
    const hipError_t e = v.empty() ? hipSuccess : hipMemcpy(*d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
    if (e != hipSuccess) return set_err(-2, "%s upload failed: %s", what, hipGetErrorString(e));
    return 0;
}

// a temporary device buffer of one call, freed by release() or on any other exit
template <typename T>
struct dev_tmp {
    T* p = nullptr;
    dev_tmp() = default;
    dev_tmp(const dev_tmp&) = delete;
    dev_tmp& operator=(const dev_tmp&) = delete;
    ~dev_tmp() { release(); }
    hipError_t alloc(size_t count) { return hipMalloc((void**)&p, count * sizeof(T)); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
    }
};

// unload a hipRTC module of the handle (jit_module, ipm_module) and delete its record
template <typename M>
static void module_release(M*& m) {
    if (!m) return;
    if (m->mod) (void)hipModuleUnload(m->mod);
    delete m;
    m = nullptr;
}
