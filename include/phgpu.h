/*
 * phgpu.h -- C-ABI of the MI355X-native progressive-hedging hot path.
 *
 * One handle holds one rank's local scenarios: a CSR sparsity pattern shared by all
 * of them and per-scenario coefficient / bound / objective arrays.  The library
 * replaces, for all local scenarios at once:
 *
 *   - SPOpt.solve_loop / solve_one        mpisppy/spopt.py:226-307 / 85-223
 *       (one LP/QP per scenario through Pyomo's SolverFactory plugin .solve(),
 *        spopt.py:165-172; results fields spopt.py:175-206)      -> phgpu_solve
 *   - PHBase.attach_PH_to_objective terms  mpisppy/phbase.py:617-699
 *       (W_on * W.x + prox_on * rho/2 (x - xbar)^2)                -> phgpu_set_ph_state
 *   - _Compute_Xbar local sums             mpisppy/phbase.py:27-87  -> phgpu_ph_reduce
 *   - Update_W + convergence_diff          mpisppy/phbase.py:293-343 -> phgpu_ph_update
 *   - SPOpt.Ebound / Eobjective / _update_E1 / feas_prob local sums
 *                                          mpisppy/spopt.py:310-439 -> phgpu_expectations
 *   - Fixer.miditer (counters, decisions, var.fix)
 *                                          mpisppy/extensions/fixer.py:114-304 -> phgpu_fixer_step
 *   - FWPH's column set and QP per scenario (SDM, _add_QP_column, _conv_diff)
 *                                          mpisppy/fwph/fwph.py:210-370, 528-547 -> phgpu_fwph_*
 *   - the L-shaped method's cuts and master LP
 *                                          mpisppy/opt/lshaped.py:477-560, 600-630 -> phgpu_lshaped_*
 *   - the extensive form's solve (ExtensiveForm.solve_extensive_form, SchurComplement.solve)
 *                                          mpisppy/opt/ef.py:60-140, opt/sc.py:60-105 -> phgpu_ef_*
 *   - bundles: the extensive form of each bundle's scenarios as a PH subproblem
 *                                          mpisppy/spbase.py:219-253, spopt.py:805-836 -> phgpu_bundle_*
 *   - the extensive form of a scenario tree (create_EF with all_nodenames), and of a sampled subtree
 *     whose ancestors' nonants are fixed (SampleSubtree fixing its Vars; every subtree of a stage in
 *     one conditioned tree)              mpisppy/confidence_intervals/sample_tree.py:79-158, 234-251
 *                                          -> phgpu_eft_*, phgpu_eft_fix
 *   - the per-batch moments of the MMW gap estimators and of zhat4xhat
 *                                          mpisppy/confidence_intervals/ciutils.py:400-415 -> phgpu_gap_moments
 *   - APH's projective step, dispatch and partial solve loop (Update_y, Compute_Averages,
 *     listener_side_gig, Update_theta_zw, _dispatch_list, APH_solve_loop)
 *                                          mpisppy/opt/aph.py:151-195, 254-310, 394-408, 453-496,
 *                                          602-668 -> phgpu_aph_*, phgpu_select_smallest,
 *                                          phgpu_solve_list
 *
 * The cross-rank sums (the per-node MPI Allreduce of phbase.py:83-87 and the
 * ROOT-comm Allreduce of phbase.py:341) are done by the caller (RCCL all-reduce of
 * the node buffer) between phgpu_ph_reduce and phgpu_ph_update.
 *
 * Conventions
 *   - Every function returns 0 on success and a negative code on error; the text of
 *     the last error of the calling thread is available from phgpu_last_error.
 *   - "host" pointers are read during the call only.  "device" pointers are HIP
 *     device pointers (e.g. torch.Tensor.data_ptr() of a cuda tensor) owned by the
 *     caller; the library owns only the workspace it allocates in phgpu_create and
 *     frees in phgpu_destroy.
 *   - Per-scenario arrays are scenario-fastest: element (k, s) of a k-indexed
 *     quantity lives at [k * S + s]  (coalesced: 64 lanes = 64 scenarios).
 *   - All work is ordered on the given hipStream_t (NULL = default stream); no call
 *     synchronises the device except phgpu_create / phgpu_destroy and
 *     phgpu_set_scenarios on a shared-matrix handle (it sizes its records from the data).
 *   - A handle is used by one host thread; it is not re-entrant; one process per GPU.
 *   - The problem is stored as a minimisation; a maximise model is negated by the
 *     caller (phbase.py:696-699 subtracts the PH term for max, which is the same).
 */
#ifndef PHGPU_H
#define PHGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct phgpu_state* phgpu_handle;

/* Per-scenario solve status (mapped to _mpisppy_data.scenario_feasible and the
 * termination_condition checks of spopt.py:175-194).  PRIMAL_INFEASIBLE: a dual ray
 * (Farkas certificate) was found, obj = bound = +inf; DUAL_INFEASIBLE: a primal ray of
 * descent was found (the subproblem is unbounded), obj = bound = -inf. */
enum {
    PHGPU_OPTIMAL = 0,
    PHGPU_ITER_LIMIT = 1,
    PHGPU_PRIMAL_INFEASIBLE = 2,
    PHGPU_DUAL_INFEASIBLE = 3
};

/* Solver options (the iter0_solver_options / iterk_solver_options dicts of
 * phbase.py:273-274 become these fields). */
typedef struct {
    double eps_rel;        /* relative KKT tolerance (primal, dual, gap)      [1e-9] */
    double eps_abs;        /* absolute KKT tolerance                          [1e-12] */
    int32_t max_iter;      /* PDHG iteration cap per scenario                 [100000] */
    int32_t check_every;   /* KKT / restart check period (iterations)         [64] */
    double gamma;          /* Halpern reflection coefficient in [0, 1]         [1.0]
                              (kernel 2 requires 1.0; kernel 0 uses kernel 1 otherwise) */
    double beta_sufficient;/* restart if r <= beta_suff * r_restart           [0.2] */
    double beta_necessary; /* ... or r <= beta_nec * r_restart and no progress [0.8] */
    double eta_frac;       /* step = eta_frac / ||A_scaled||_2                [0.998] */
    double omega0;         /* initial primal weight (<= 0: keep previous)     [1.0] */
    int32_t keep_omega;    /* 1: carry the primal weight across solves         [1] */
    int32_t restart_every; /* restart test period (iterations; divides check_every) [16] */
    double beta_artificial;/* restart when the Halpern run exceeds this fraction
                              of all iterations of the solve                  [0.36] */
    double omega_clamp;    /* primal weight kept in [1/clamp, clamp] (scaled) [1e4] */
    int32_t kernel;        /* 0 auto, 1 global-memory kernel, 2 register-resident
                              kernel (error if no compiled instance fits),
                              3 workgroup-per-scenario kernel (large scenarios),
                              4 shared-matrix streaming kernel (the only path, and
                              the automatic one, of a PHGPU_SHARED_MATRIX handle),
                              5 pattern-specialised kernel: one lane per scenario,
                              compiled with hipRTC for this handle's pattern at its
                              first path-5 solve (n, m <= 48, nnz <= 128; that solve
                              synchronises the stream once),
                              6 interior-point kernel (Mehrotra predictor-corrector,
                              one lane per scenario, compiled with hipRTC for this
                              handle's pattern and data at its first path-6 solve, which
                              synchronises once; n <= 40, m <= 32, nnz <= 128; the
                              automatic path wherever it applies, PHGPU_IPM=0 turns that
                              off; scenarios it does not finish go to the path-5 PDHG,
                              which certifies infeasibility)              [0] */
    int32_t infeas_start;  /* infeasibility certificates are tested at the KKT
                              checks from this iteration on (< 0: never)      [512] */
    double eps_infeas;     /* certificate tolerance: ray violation <= eps * |ray
                              objective| (PDLP-style)      [1e-8] */
    int32_t split_longest; /* path 4: the split_longest (<= 16) scenarios with the most
                              iterations in the previous solve run first, each over the
                              whole GPU (the split form); 0: the
                              PHGPU_STREAM_SPLIT environment variable, else none  [0] */
} phgpu_options;
/* max_iter must be a multiple of restart_every: the register-resident kernel counts
 * iterations in chunks of restart_every and stops exactly at max_iter (both kernels then
 * report iters == max_iter on ITER_LIMIT). */

/* Fill *opt with the defaults shown above. */
int phgpu_default_options(phgpu_options* opt);

/* Create a handle for S local scenarios sharing one CSR pattern.
 * Replaces: SPOpt._create_solvers / set_instance (spopt.py:839-903) and the
 * nonant index bookkeeping of SPBase._attach_nlens / _attach_nonant_indices
 * (spbase.py:293-320).
 *   row_ptr[m+1], col_idx[nnz]          host, the shared pattern
 *   nonant_col[nn]                      host, column of flat nonant k (node-list
 *                                       order then sorted index, scenario_tree.py:39)
 *   nonant_depth[nn], nonant_off[nn]    host, tree depth of k's node / offset in it
 *   depth                               number of non-leaf nodes per scenario
 *   num_nodes, nlen_max                 size of the node-indexed x̄ buffer
 *                                       (num_nodes * nlen_max entries per half) */
int phgpu_create(phgpu_handle* h, int device, int64_t S, int32_t n, int32_t m, int32_t nnz,
                 const int32_t* row_ptr, const int32_t* col_idx, int32_t nn,
                 const int32_t* nonant_col, const int32_t* nonant_depth,
                 const int32_t* nonant_off, int32_t depth, int32_t num_nodes,
                 int32_t nlen_max);

/* Flags of phgpu_create2.
 * PHGPU_SHARED_MATRIX: every scenario has the same constraint-matrix values (the UC
 *   relaxation: scenarios differ in bounds only).  phgpu_set_scenarios then takes
 *   A_val[nnz] (one copy), scales it once, and keeps per scenario only the iterates and
 *   the columns / rows whose data differ between scenarios (plus the nonant columns);
 *   solves run on path 4 (one workgroup streams one scenario).  Meant for
 *   scenarios too large for the register / workgroup-resident paths. */
#define PHGPU_SHARED_MATRIX 1u

/* phgpu_create with flags (phgpu_create(...) == phgpu_create2(..., 0)). */
int phgpu_create2(phgpu_handle* h, int device, int64_t S, int32_t n, int32_t m, int32_t nnz,
                  const int32_t* row_ptr, const int32_t* col_idx, int32_t nn,
                  const int32_t* nonant_col, const int32_t* nonant_depth,
                  const int32_t* nonant_off, int32_t depth, int32_t num_nodes,
                  int32_t nlen_max, uint32_t flags);

/* Upload per-scenario data (device pointers, scenario-fastest):
 *   A_val[nnz*S] (A_val[nnz] on a PHGPU_SHARED_MATRIX handle), c/lb/ub/q[n*S]
 *   (q may be NULL = 0), rl/ru[m*S] (+-inf allowed),
 *   obj_const[S] (may be NULL), prob[S], node_of[depth*S] (int32 global node id),
 *   prob_coeff[depth*S] (pi_s / pi_node, spbase.py:384-391).
 * Computes the diagonal (Ruiz + Pock-Chambolle) scaling and ||A_scaled||_2 per
 * scenario; replaces the per-scenario Pyomo model construction of
 * SPBase._create_scenarios (spbase.py:255-291). */
int phgpu_set_scenarios(phgpu_handle h, const double* A_val, const double* c,
                        const double* lb, const double* ub, const double* rl,
                        const double* ru, const double* q, const double* obj_const,
                        const double* prob, const int32_t* node_of,
                        const double* prob_coeff, void* stream);

/* Variable probabilities (spbase.py:394-424, phbase.py:54-79 and 315-318): pvar, device
 * [nn*S] (k-major like W), the probability coefficient of nonant k of scenario s in the x̄
 * sums in place of the per-node prob_coeff; Update_W then sets W[k,s] = 0 where pvar[k,s]
 * is 0 (prob0_mask).  Read at every reduce / update (not copied); NULL restores the per-node
 * coefficients.  While set, the PH step always runs as phgpu_ph_reduce + phgpu_ph_update
 * (no epilogue partials, no folded or fused step); partials of earlier solves are dropped. */
int phgpu_set_nonant_probs(phgpu_handle h, const double* pvar);

/* Interior-point tuning of this handle (path 6): defs = "IPM_NAME=number;..." -- the
 * compile-time constants of the generated interior-point modules (one table of defaults
 * for every kernel, jit_ipm_common.hip.in: IPM_SIG_MIN, IPM_WARM_T, ...; a kernel's own in
 * its jit_ipm*.hip.in) for the modules this handle builds; a model's measured
 * values (examples/aircond.py IPM_TUNING).  Only IPM_ names and numeric values; NULL or ""
 * clears.  Call before the first solve (-1 once the module is built).  The PHGPU_IPM_DEFS
 * environment variable (experiments) overrides it name by name. */
int phgpu_set_ipm_tuning(phgpu_handle h, const char* defs);

/* Bind the PH objective terms for the next solves (phbase.py:585-699):
 *   objective = f(x) + W_on * sum_k W[k,s] x_k + prox_on * sum_k rho[k,s]/2 (x_k - xbar[k,s])^2
 * W, rho, xbar: device [nn*S]; they are read at solve time (not copied). */
int phgpu_set_ph_state(phgpu_handle h, const double* W, const double* rho,
                       const double* xbar, int W_on, int prox_on);

/* Solve all local scenarios (SPOpt.solve_loop, spopt.py:226-307).
 *   warm_start   1: start from the previous solution (x, y) of this handle
 *   x[n*S]       device out: primal solution (all columns)
 *   y[m*S]       device out (may be NULL): row duals (positive = lower bound active)
 *   obj[S]       device out: augmented objective incl. PH terms (what
 *                Eobjective sums, spopt.py:332-333)
 *   bound[S]     device out: Lagrangian dual bound (results.Problem[0].Lower_bound,
 *                spopt.py:201-206)
 *   status[S]    device out: PHGPU_* code
 *   iters[S]     device out (may be NULL): iterations used (PDHG iterations; interior-
 *                point iterations for scenarios path 6 solved)
 * phgpu_solve_stats and phgpu_ph_update_ex(stats_out) read the status / iters outputs of
 * the last solve launched on the handle (paths without in-kernel statistics): those
 * buffers must stay alive until the next solve when statistics are requested.  A solve
 * rejected by validation leaves the previous solve's buffers in place.
 * Kernel 0 (automatic) on a pattern path 6 applies to: if its module cannot be compiled
 * or loaded, path 6 is turned off for the handle's data (phgpu_ipm_info off = 2), the
 * reason stays in phgpu_last_error and the solve runs on the handle's PDHG path;
 * kernel 6 asked for explicitly returns the error instead. */
int phgpu_solve(phgpu_handle h, const phgpu_options* opt, int warm_start, double* x,
                double* y, double* obj, double* bound, int32_t* status, int32_t* iters,
                void* stream);

/* Speculative solves.  PHBase.iterk_loop (phbase.py:909-957) decides after x̄ / W /
 * conv whether the next solve_loop runs; the engine launches it before that decision
 * and keeps it only if the loop goes on.  phgpu_solve_deferred is phgpu_solve except
 * that the warm-start state it leaves (the iterate the next warm solve starts from,
 * the primal weight, the work-queue predictor) goes to a second slot, which becomes the
 * handle's state only at phgpu_commit; any other solve before that drops it, so a
 * discarded speculative solve leaves the handle exactly as the last committed solve
 * did.  Its outputs (x, y, obj, bound, status, iters) are written as by phgpu_solve.
 * A PHGPU_SHARED_MATRIX handle (path 4) has one slot and rejects deferred solves. */
int phgpu_solve_deferred(phgpu_handle h, const phgpu_options* opt, int warm_start, double* x,
                         double* y, double* obj, double* bound, int32_t* status, int32_t* iters,
                         void* stream);

/* Make the warm-start state of the last phgpu_solve_deferred current (no-op if there is
 * none pending).  Host-side bookkeeping only: no device work, no synchronisation. */
int phgpu_commit(phgpu_handle h);

/* Local x̄ partial sums (phbase.py:54-79): node_buf[2*num_nodes*nlen_max] gets
 *   [g*nlen_max + o]                        sum_s prob_coeff * x
 *   [num_nodes*nlen_max + g*nlen_max + o]   sum_s prob_coeff * x^2
 * over the local scenarios whose depth-d node is g.  node_buf is overwritten. */
int phgpu_ph_reduce(phgpu_handle h, const double* x, double* node_buf, void* stream);

/* After the cross-rank sum of node_buf: scatter x̄ to every local scenario
 * (phbase.py:90-103), W += rho (x - x̄) if update_W (phbase.py:293-318), and
 * conv_local[0] = sum_{s,k} |x - x̄| / (S * nn)  (phbase.py:330-339; the caller
 * sums over ranks and divides by n_proc, phbase.py:341-343).
 *   xbar, W: device [nn*S] (xbar written, W updated in place). */
int phgpu_ph_update(phgpu_handle h, const double* x, const double* node_buf, double* xbar,
                    double* W, const double* rho, int update_W, double* conv_local,
                    void* stream);

/* phgpu_ph_update, plus: stats_out (int64[6], may be NULL) receives the statistics of
 * the handle's last solve launch as phgpu_solve_stats reports them, written by the same
 * kernel that writes conv_local.  conv_local and stats_out may be host-mapped pinned
 * memory (zero-copy), which saves the copy launches of the PH loop's convergence and gripe
 * readbacks (phbase.py:330-343, spopt.py:284-294): the host may read them after an event
 * recorded behind this call, or poll them -- they are written last, by one store
 * instruction, so a caller that set conv_local to NaN and stats_out to -1 before the call
 * has all seven values once none of them is a sentinel (the engine does that: no event
 * marker in the PH step).  The conv reduction over the grid is done by the kernel's last
 * block.  Clears no other state. */
int phgpu_ph_update_ex(phgpu_handle h, const double* x, const double* node_buf, double* xbar,
                       double* W, const double* rho, int update_W, double* conv_local,
                       int64_t* stats_out, void* stream);

/* phgpu_ph_reduce + phgpu_ph_update_ex for a single rank (no cross-rank sum of node_buf
 * between them), in fewer launches when every nonant's local scenarios share one node (a
 * two-stage problem) and nn <= 16: the x̄ final sum is folded into the update kernel.
 * Same outputs: node_buf (the local sums), xbar, W, conv_local, stats_out. */
int phgpu_ph_step_local(phgpu_handle h, const double* x, double* node_buf, double* xbar, double* W,
                        const double* rho, int update_W, double* conv_local, int64_t* stats_out,
                        void* stream);

/* phgpu_ph_step_local, deferred: the step is recorded and runs at the handle's next call.
 * If that call is a phgpu_solve_deferred that takes path 6 (the batched interior point),
 * writes other output buffers than x, and the previous solve was path 6 with its x̄
 * partials for x, the step is folded into the solve launch's prologue:
 * every block sums the previous solve's partials to x̄, each scenario updates its x̄ / W,
 * and the grid's last block stores conv_local; stats_out (the previous solve's statistics)
 * is stored by the same launch.  conv_local and stats_out are written a few microseconds
 * into the solve: a caller polling them (NaN / -1 sentinels, as phgpu_ph_update_ex
 * describes) learns the convergence metric while the solve runs.  Any other call on the
 * handle (or a solve that cannot fold it) first runs the step as phgpu_ph_step_local on
 * the stream given here.  PHGPU_FUSE_STEP=0 never folds (experiments). */
int phgpu_ph_step_defer(phgpu_handle h, const double* x, double* node_buf, double* xbar, double* W,
                        const double* rho, int update_W, double* conv_local, int64_t* stats_out,
                        void* stream);

/* Run a step deferred by phgpu_ph_step_defer now (no-op if none is pending). */
int phgpu_ph_step_flush(phgpu_handle h);

/* Adaptive rho (mpisppy/extensions/norm_rho_updater.py) and the residual sums of the
 * primal-dual and norm-rho convergers (mpisppy/convergers/), in two calls with the ranks'
 * sum of `planes` by the caller between them.  Both are ordered on the stream and do not
 * synchronise (the first use allocates their own workspace; phgpu_workspace_bytes grows
 * only then); both work on a PHGPU_SHARED_MATRIX handle.
 *
 * phgpu_ph_residuals: one pass over the local scenarios.  planes[4 * num_nodes * nlen_max],
 * four node-indexed planes laid out like one half of node_buf ([g * nlen_max + off]), the
 * sums over the local scenarios whose node at the nonant's depth is g of
 *   plane 0   prob_s |x - x̄|    prob_s the scenario's unconditional probability (not
 *             prob_coeff, with variable probabilities too): the primal residual of
 *             NormRhoUpdater._compute_primal_residual_norm, norm_rho_updater.py:73-83
 *             (its Allreduce, :85-89, is the caller's sum)
 *   plane 1   pcoef |x - x̄|     pcoef = prob_coeff, or pvar[k, s] with variable
 *             probabilities: summed over its entries, PrimalDualConverger's primal gap,
 *             primal_dual_converger.py:66-82
 *   plane 2   rho[k, s]          unweighted: sum of plane 2 x |x̄ - x̄_prev| is the
 *             converger's dual gap, primal_dual_converger.py:96-107
 *   plane 3   prob_s rho[k, s]   summed over its entries, NormRhoConverger's rho norm,
 *             norm_rho_converger.py:26
 * rho_last[num_nodes * nlen_max] (same indexing; rank-local, never summed over ranks):
 * rho[k, s] of the last local scenario (highest local index) of node g.
 * _compute_dual_residual_norm (norm_rho_updater.py:98-104) overwrites dual_resid[ndn_i]
 * scenario by scenario, so every rank's dual residual carries the rho of its own last
 * scenario at the node; it is taken here because phgpu_norm_rho_update rewrites rho.
 *   x[n*S], xbar[nn*S], rho[nn*S]: device, read.  Both outputs are overwritten in full
 *   (entries no local scenario reaches are 0).
 * Wave-uniform nodes are summed deterministically (per-wave partials, then an ordered
 * final sum, as phgpu_ph_reduce); a wave that spans nodes adds by fp64 atomics. */
int phgpu_ph_residuals(phgpu_handle h, const double* x, const double* xbar, const double* rho,
                       double* planes, double* rho_last, void* stream);

/* Constants of the rho rule (NormRhoUpdater's options, norm_rho_updater.py:12-31). */
typedef struct {
    double tol;              /* convergence_tolerance                              [1e-4] */
    double inc;              /* rho_increase_multiplier                            [2.0] */
    double dec;              /* rho_decrease_multiplier                            [2.0] */
    double conv_dec;         /* rho_converged_decrease_multiplier                  [1.1] */
    double f;                /* primal_dual_difference_factor                      [100.0] */
    int32_t allow_decrease;  /* the host's ph_iter >= iterations_converged_before_decrease */
} phgpu_norm_rho_params;

/* The rule of NormRhoUpdater.miditer (norm_rho_updater.py:128-143) for every local (k, s),
 * after the ranks' sum of planes.  With g the scenario's node at k's depth:
 *   p = planes[g * nlen_max + off]                                  (plane 0)
 *   d = rho_last[g * nlen_max + off] * |xbar_node[..] - xbar_prev[..]|
 *   if p > f d and p > tol:         rho[k, s] *= inc
 *   else if d > f p and d > tol:    rho[k, s] /= dec   only if allow_decrease
 *   else if p < tol and d < tol:    rho[k, s] /= conv_dec
 * (strict comparisons, as the reference; a decrease that is not allowed takes no action and
 * does not fall through to the third test).
 *   xbar_node: the first half of the reduced node_buf; xbar_prev: the caller's copy of it
 *   from the previous miditer (_prev_avg, norm_rho_updater.py:50-53); rho: device [nn*S],
 *   rewritten in place; counts: device int64[4] or NULL, the local (k, s) entries that took
 *   no action / increased / decreased / took the converged decrease. */
int phgpu_norm_rho_update(phgpu_handle h, const phgpu_norm_rho_params* prm, const double* planes,
                          const double* rho_last, const double* xbar_node, const double* xbar_prev,
                          double* rho, int64_t* counts, void* stream);

/* Inner-bound candidates that are functions of all scenarios: x̄ itself
 * (mpisppy/extensions/xhatxbar.py:38-55, cylinders/xhatxbar_bounder.py:96-104), the slam
 * heuristics' column-wise max / min (cylinders/slam_heuristic.py:57-67 and 84) and the scenario
 * closest to x̄ (extensions/xhatclosest.py:37-65).  Both entries are ordered on the stream and
 * do not synchronise (the first use allocates their own workspace; phgpu_workspace_bytes grows
 * only then); both work on a PHGPU_SHARED_MATRIX handle.  Inputs are finite: what a NaN in v
 * gives is unspecified.
 *
 * phgpu_nonant_stats: v, device [nn*S], nonant values k-major and scenario-fastest (the layout
 * of W and of a spoke's localnonants, not x[n*S]).  planes[4 * num_nodes * nlen_max], four
 * node-indexed planes laid out like one half of node_buf ([g * nlen_max + off]), each over the
 * local scenarios whose node at the nonant's depth is g:
 *   plane 0   sum pcoef v        pcoef = prob_coeff, or pvar[k, s] with variable probabilities
 *   plane 1   sum pcoef v^2      (the weights of phgpu_ph_reduce: xbars / xsqbars,
 *                                phbase.py:54-79, which xhatxbar.py:49-51 fixes the nonants at
 *                                and xhatclosest.py:40-42 measures against)
 *   plane 2   max(-v) = -min v   slam_heuristic.py:65 with np.amin, negated
 *   plane 3   max(v)             slam_heuristic.py:65 with np.amax
 * An entry no local scenario reaches is 0 in planes 0-1 and -inf in planes 2-3, so the caller
 * sums planes 0-1 over the ranks and takes ONE MAX all-reduce over planes 2-3 (the reference's
 * Allreduce with mpi.MAX / mpi.MIN, slam_heuristic.py:84).  planes is overwritten in full.
 * Planes 0-1 are deterministic wherever phgpu_ph_reduce is (wave-uniform nodes: per-wave
 * partials, then an ordered final sum; a wave that spans nodes adds by fp64 atomics); planes
 * 2-3 do not depend on the order. */
int phgpu_nonant_stats(phgpu_handle h, const double* v, double* planes, void* stream);

/* The local scenario closest to x̄ in truncated z-score (xhatclosest.py:37-51), two-stage
 * handles only (depth 1, one node; -3 and nothing launched otherwise, as the reference's
 * pre_iter0 refuses multistage, :91-93).  xbar_node, xsqbar_node: device [nlen_max] each, the
 * reduced planes 0 and 1 of phgpu_nonant_stats or the two halves of node_buf.  For every
 * local scenario s
 *   dist[s] = sum_k [var_k > 0] min(3, |v[k, s] - x̄_k| / sqrt(var_k)),  var_k = x̄²_k - x̄_k x̄_k
 * with k ascending and the test on var_k strict (:41-45).  dist: device [S] or NULL.
 * best: device double[2], written last: the smallest dist and the LOWEST local index attaining
 * it (the strict < scan of :46-51).  The ranks' agreement (MIN of the distance, then MAX of
 * the rank among those attaining it, :53-65) is the caller's. */
int phgpu_nonant_closest(phgpu_handle h, const double* v, const double* xbar_node,
                         const double* xsqbar_node, double* dist, double* best, void* stream);

/* Cost-proportional rho, rho_k ~ |cost_k| / |x_k - x̄_k|, set when the dual metric stalls:
 * mpisppy/utils/gradient.py (Find_Grad), utils/find_rho.py (Find_Rho), utils/wtracker.py
 * (WTracker.W_diff) and extensions/gradient_extension.py.  All four entries are ordered on the
 * stream and do not synchronise (the first use allocates their own workspace;
 * phgpu_workspace_bytes grows only then), work on a PHGPU_SHARED_MATRIX handle, and give the
 * same bits on every run.
 *
 * phgpu_grad_cost: cost[k, s] = -(c[col_k, s] + q[col_k, s] xn[k, s]) in original (unscaled)
 * units, the negated derivative of the stored objective c.x + 1/2 x.diag(q).x at the nonant
 * values xn: Find_Grad.compute_grad, gradient.py:65-81.  The reference fixes the nonants at
 * xhat, solves, unfixes and restores (:95-122) only to move pynumero's evaluation point; q is
 * diagonal here, so the nonants' derivative depends on xn alone and no solve is needed.
 * (compute_grad indexes the gradient, which is in NLP variable order, by nonant position, :78-80;
 * this entry gives the derivative with respect to the nonant itself.)
 *   xn, cost: device [nn*S], k-major and scenario-fastest (the layout of W). */
int phgpu_grad_cost(phgpu_handle h, const double* xn, double* cost, void* stream);

/* WTracker.W_diff, wtracker.py:141-154: out[0] = sum_{k,s} |W[k,s] - W_prev[k,s]| / (S nn) over
 * the local scenarios, and W_prev = W in the same pass.  The ranks' combination is the
 * caller's: the reference sums the ranks' means and divides by n_proc (:155-157, as for
 * conv_local); the engine weights every rank's mean by its share of the scenarios, which is the
 * same number for an even split and does not depend on the split otherwise.
 *   W: device [nn*S], read; W_prev: device [nn*S], rewritten; out: device double[1]. */
int phgpu_w_diff(phgpu_handle h, const double* W, double* W_prev, double* out, void* stream);

/* The ratios of Find_Rho.compute_rho (find_rho.py:170-203) reduced per nonant; two-stage
 * handles only (depth 1, one node; -3 and nothing launched otherwise: the reference asserts
 * node.name == "ROOT", :89, :109, :128).  r[k, s] = |cost[k, s]| / denominator, with
 *   gden == NULL   the scenario's own denominator d_s = max over its nonants j of
 *                  max(|x_j - x̄_j|, 2 (x_j - x̄_j)^2): np.max((w_denom, prox_denom)) at :189 is
 *                  one scalar per scenario (_w_denom :78-95, _prox_denom :98-115)
 *   gden given     gden[off_k], device [nlen_max]: _grad_denom (:118-147), i.e.
 *                  max(1 / rho_relative_bound, the ranks' sum of plane 1 of phgpu_ph_residuals)
 * planes[3 * num_nodes * nlen_max], laid out like phgpu_nonant_stats' planes:
 *   plane 0   sum_s r (unweighted)     plane 1   max(-r) = -min r     plane 2   max(r)
 * over the local scenarios; an entry without a nonant is 0 / -inf / -inf.  The caller takes one
 * SUM (plane 0) and one MAX (planes 1-2) all-reduce over the ranks.  Division is IEEE, as
 * numpy's: a zero denominator gives +inf; what 0 / 0 gives is unspecified.  Plane 0: per-wave
 * partials and an ordered final sum, as phgpu_ph_reduce.
 *   cost: device [nn*S]; x[n*S], xbar[nn*S]: device, read when gden is NULL. */
int phgpu_rho_ratio_stats(phgpu_handle h, const double* cost, const double* x, const double* xbar,
                          const double* gden, double* planes, void* stream);

/* Find_Rho._order_stat (find_rho.py:150-168) of every nonant's ratios, after the ranks'
 * reductions of planes, written to rho[k, s] of every local scenario (the rho_setter loop of
 * gradient_extension.py:85-94); two-stage handles only (-3).  With mean = plane 0 / S_total
 * (S_total: scenarios of all ranks), min = -plane 1, max = plane 2 and a = order_stat in [0, 1]:
 *   a == 0.5: mean;   a < 0.5: min + 2 a (mean - min);   a > 0.5: (2 mean - max) + 2 a (max - mean)
 * gate: device double[2] = {previous, current} dual metric (the ranks' W_diff), or NULL.  rho is
 * written only if |(previous - current) / previous| <= thr, which NaN and inf fail
 * (_update_rho_dual_based, gradient_extension.py:65-68, where thr is 0.05); NULL always writes.
 * With the gate closed no byte of rho is stored.  applied: device int32[1] or NULL, 1 if rho
 * was written, else 0. */
int phgpu_rho_from_stats(phgpu_handle h, const double* planes, int64_t S_total, double order_stat,
                         const double* gate, double thr, double* rho, int32_t* applied, void* stream);

/* Local probability-weighted sums (spopt.py:310-439) into out[5]:
 *   out[0] = sum_s prob_s * obj_s    out[1] = sum_s prob_s * bound_s
 *   out[2] = sum_s prob_s (E1)       out[3] = sum_{s feasible} prob_s, where feasible
 *   means status is OPTIMAL or ITER_LIMIT (a solution was loaded; spopt.py:175-194
 *   marks only infeasible / unbounded / no-solution results infeasible)
 *   out[4] = sum_{s OPTIMAL} prob_s (certified solves: the xhat inner bound,
 *   xhatbase.py:210-216, is only taken when this equals E1) */
int phgpu_expectations(phgpu_handle h, const double* obj, const double* bound,
                       const int32_t* status, double* out, void* stream);

/* Per-segment moments of two batched solves: what the Mak-Morton-Wood gap estimator
 * (confidence_intervals/ciutils.py:400-415) and zhat4xhat (zhat4xhat.py:94) take of the
 * per-scenario objectives, reduced on the device.
 *   f_hat, f_star: device [S], the objectives of the local scenarios in the two solves (at the
 *   candidate and at the sample problem's optimum); st_hat, st_star: their status outputs.
 *   f_star and st_star may both be NULL (no x* side: g and f_star count as 0, st_hat alone
 *   decides what is left out); exactly one of them NULL is an error.
 *   seg_ptr: device int64[nseg + 1], ascending, in GLOBAL scenario indices; local scenario k has
 *   the global index s_off + k.  A segment may begin before the local scenarios, end behind
 *   them, miss them or be empty; seg_ptr's contents are not validated.
 *   out: device [nseg][8].  With p the handle's scenario probabilities and g = f_hat - f_star,
 *   row j holds over the local scenarios of segment j
 *     {sum p, sum p^2, sum p g, sum p g^2, sum p f_hat, sum p f_star, scenarios left out, 0};
 *   a scenario that is not PHGPU_OPTIMAL in either solve is left out of the six sums and counted.
 * The sums are made in a fixed order without atomics (two calls give the same bits) and are not
 * normalised: the caller divides by sum p after summing the rows over the ranks.  The workspace
 * (two slots of 7 partials per wave) is allocated at the first call. */
int phgpu_gap_moments(phgpu_handle h, const double* f_hat, const int32_t* st_hat,
                      const double* f_star, const int32_t* st_star,
                      const int64_t* seg_ptr, int32_t nseg, int64_t s_off,
                      double* out, void* stream);

/* counts[c] = number of local scenarios whose status[s] == c, c = 0..3 (OPTIMAL,
 * ITER_LIMIT, PRIMAL_INFEASIBLE, DUAL_INFEASIBLE): the check behind SPOpt.solve_loop's
 * gripe (spopt.py:284-294) as one device reduction.  status: device [S] (phgpu_solve's
 * output), counts: device int32[4]. */
int phgpu_status_counts(phgpu_handle h, const int32_t* status, int32_t* counts, void* stream);

/* Statistics of the last solve (phgpu_solve / phgpu_solve_deferred on this handle),
 * enqueued on stream into out[6] (device or pinned host memory): the number of local
 * scenarios with status 0..3 (what phgpu_status_counts gives for its status output), the
 * sum and the maximum of its iters output.  Path 6 accumulates them inside its kernels
 * (then this is one 48-byte copy); for the other paths a one-block reduction over the
 * last solve's outputs computes them (iters may have been NULL: sum = max = 0). */
int phgpu_solve_stats(phgpu_handle h, int64_t* out, void* stream);

/* Fix the nonants of every local scenario (lb = ub = xfix[k*S + s], original units,
 * clipped to the model bounds) for the following solves, or restore the model bounds
 * when xfix is NULL.  A NaN entry leaves that nonant at its model bounds (partial
 * fixing: Xhat_Eval.fix_nonants_upto_stage, xhat_eval.py:326-362).  Replaces
 * SPOpt._fix_nonants / _restore_nonants as used by Xhat_Eval and XhatBase._try_one
 * (spopt.py:557-660, xhatbase.py:199-216).
 *   xfix: device [nn*S] (read during the call only) or NULL */
int phgpu_fix_nonants(phgpu_handle h, const double* xfix, void* stream);

/* Constants of the Fixer's rule (mpisppy/extensions/fixer.py:52-64). */
typedef struct {
    double boundtol;  /* fixeroptions["boundtol"]: xb within this of a bound sits on it */
    int32_t iter0;    /* 1: the rule of Fixer.iter0 (miditer at PH iteration 1), 0: of Fixer.iterk */
} phgpu_fixer_params;

/* Fixer.miditer (mpisppy/extensions/fixer.py:314-322) for every local (k, s) in one device
 * pass: the convergence counters (_update_fix_counts, :114-128), the decisions (iter0
 * :156-189, iterk :248-279) and the bound rewrite.  With g the scenario's node at k's depth
 * and o the nonant's offset in the node:
 *   xb   = node_buf[g * nlen_max + o]            (x̄, first half of the reduced node_buf)
 *   xsq  = node_buf[half + g * nlen_max + o]     (E[x²], half = num_nodes * nlen_max)
 *   diff = xb * xb - xsq                         (the product rounded on its own)
 *   l, u = the scenario's model bounds of the column (original units)
 * An entry that is fixed already is skipped and its counter left alone (is_fixed, :119, 164,
 * 257): fixval[k, s] is not NaN, or l == u in the model.
 *   iter0 != 0 (:169-189): converged iff !(-diff > th² || diff > th²) (non-strict); then the
 *     first of  nb not None -> xb;  lb not None and xb - l < boundtol -> l;
 *     ub not None and u - xb < boundtol -> u.  Counters are not touched.
 *   iter0 == 0: count = (-diff < th² && diff < th²) ? count + 1 : 0 (strict, :124-128); then
 *     if count > 0 the first of (:263-279)  nb not None and nb <= count -> xb;
 *     lb not None and lb < count and xb - l < boundtol -> l;
 *     ub not None and ub < count and u - xb < boundtol -> u.
 * A lag < 0 is the reference's None; 0 is a valid lag.  A nonant without a tuple is th = 0
 * with all lags None: never fixed, counter 0.  THIS DEPARTS FROM fixer.py in that the lags are
 * per nonant (there per nonant and scenario; thresholds are per nonant there too, :88-102).
 * The value is clipped to [l, u]; a newly fixed entry gets fixval[k, s] and the handle's
 * working bounds lb = ub = value exactly as phgpu_fix_nonants would write them for that entry
 * (the following solves of every path see it; phgpu_fix_nonants(NULL) would free it again --
 * pass fixval as its xfix instead).
 *   th: device double[nn]; nb, lb, ub: device int32[nn]; count: device int32[nn*S] and
 *   fixval: device double[nn*S] (NaN = free), both k-major and scenario-fastest like W,
 *   read and updated in place (stores only where something changed);
 *   nfix: device int32[num_nodes * nlen_max], overwritten in full: the local entries this call
 *   newly fixed, per node entry;
 *   totals: device int64[3], accumulated: [0] entries newly fixed, [1] entries found fixed on
 *   arrival (counted only when iter0, :199-203), [2] node entries with 0 < nfix < the node's
 *   local scenarios (the "Variation in fixing across scenarios" test of :217-219 and :302-304,
 *   made per node entry; never decreases).
 * Ordered on the stream, never synchronises; its workspace (two int32 per node entry: the
 * local scenarios, and the counts of a call in flight) is allocated at the first call
 * (phgpu_workspace_bytes grows only then).  Counts
 * are integer atomics (one per wave where the wave's scenarios share a node): the same inputs
 * give the same bits. */
int phgpu_fixer_step(phgpu_handle h, const phgpu_fixer_params* prm, const double* node_buf,
                     const double* th, const int32_t* nb, const int32_t* lb, const int32_t* ub,
                     int32_t* count, double* fixval, int32_t* nfix, int64_t* totals, void* stream);

/* FWPH (mpisppy/fwph/fwph.py), the half of Boland et al.'s Algorithm 2 that is not an LP solve:
 * per local scenario a set of columns X_j in R^nn (the nonant values of LP solutions, the layout
 * of W) with costs f_j = c.x + obj_const, weights a on the simplex, the QP point xq = sum a_j X_j
 * and phi = sum a_j f_j.  The reference keeps them in a second Pyomo model per scenario
 * (_initialize_QP_subproblems, fwph.py:685-771) and calls a QP solver per scenario and inner
 * iteration (:284-289); here one pass serves all local scenarios.  All entries are ordered on
 * the stream and never synchronise (phgpu_fwph_init does when it resizes an existing store), work
 * on a PHGPU_SHARED_MATRIX handle, for any nn and any tree, and give the same bits on every run.
 *
 * phgpu_fwph_init: allocate the store for max_cols columns per scenario (2 <= max_cols <= 64) and
 * empty it.  The store is the handle's: counted in phgpu_workspace_bytes from this call on,
 * freed by phgpu_destroy (or by an init with another max_cols).  Scenario-fastest; per scenario
 * max_cols (nn + 5) + max_cols (max_cols + 1) + nn + 1 doubles (columns, costs, weights, three
 * work vectors, the rho-weighted Gram matrix of the columns and its Cholesky work space, xq, phi)
 * and four int32 (columns held, active flag, newest column, inner iterations so far). */
int phgpu_fwph_init(phgpu_handle h, int32_t max_cols, void* stream);

/* Fill the store of every local scenario with K columns (_initialize_QP_var_values,
 * fwph.py:773-791: K = 1, Iter0's solution; the initial points of :744-755).
 *   X: device [K][nn][S], f: device [K][S], a: device [K][S] or NULL (a = e_0);
 *   rho: device [nn*S], the rho of every later call (the Gram matrix is kept up to date as
 *   columns arrive and never recomputed: rho must not change while the store is in use);
 *   xq: device [nn*S] or NULL and xqx: device [n*S] or NULL receive the QP point (xqx in its
 *   nonant columns only).  Every scenario becomes active with 0 inner iterations. */
int phgpu_fwph_load(phgpu_handle h, int32_t K, const double* X, const double* f, const double* a,
                    const double* rho, double* xq, double* xqx, void* stream);

/* Copy the store out (tests, _gather_weight_dict-style reporting); every pointer may be NULL.
 *   X: [max_cols][nn][S], f, a: [max_cols][S] (0 beyond a scenario's columns), ncols [S],
 *   xq [nn*S], phi [S], active [S], nit [S] (columns added since the load, replaced ones too). */
int phgpu_fwph_export(phgpu_handle h, double* X, double* f, double* a, int32_t* ncols, double* xq,
                      double* phi, int32_t* active, int32_t* nit, void* stream);

/* The LP's dual weights of one inner iteration (SDM, fwph.py:227-247), for every scenario:
 *   What = W + rho (src - xbar),  src = (1 - alpha) xbar + alpha xq if t0, else xq
 * What: device [nn*S], what phgpu_set_ph_state binds as W for the LP solve.  With t0 (the first
 * inner iteration of an outer one) every scenario is marked active. */
int phgpu_fwph_direction(phgpu_handle h, int t0, double alpha, const double* W, const double* rho,
                         const double* xbar, double* What, void* stream);

typedef struct {
    double conv_thresh;     /* FW_conv_thresh: a scenario with Gamma < this is done (fwph.py:291) */
    double stop_check_tol;  /* stop_check_tol: Gamma < -this is counted (the warning of :275-278) */
} phgpu_fwph_params;

/* One inner iteration of SDM after the LP solve (fwph.py:256-292, _add_QP_column :305-370), one
 * pass over the local scenarios.  x, obj, bound, status: the outputs of the solve with What
 * bound as W, W on and prox off.  For every active scenario whose status is OPTIMAL:
 *   val0 = obj, val1 = phi + What.xq (the QP point before this pass),
 *   Gamma = (val1 - val0) / |val0| if |val0| > 1e-9 else val1 - val0;
 *   the column (x's nonants, obj - What.x) is appended; a scenario that holds max_cols columns
 *   overwrites the one with the smallest weight, ties to the lowest index, never the newest
 *   (THIS DEPARTS FROM fwph.py, which never drops a column);
 *   min_a sum a_j f_j + W.x(a) + sum_k rho_k / 2 (x(a)_k - xbar_k)^2 on the simplex (W, not What)
 *   is solved by an active set on the Gram matrix (exact up to rounding; a is not unique, x(a)
 *   and phi are), from a cold start, so xq and phi depend on the columns only;
 *   the scenario stays active iff !(Gamma < conv_thresh) -- tested after the column and the QP.
 * An active scenario whose status is not OPTIMAL adds nothing, keeps its QP point and becomes
 * inactive (THIS DEPARTS FROM fwph.py:510-517, which raises).  Inactive scenarios are untouched.
 *   gamma [S], ncols [S], xq [nn*S], xqx [n*S] (nonant columns): written for the scenarios that
 *   added a column;  dual_bound [S]: = bound, written only with t0, for every active scenario;
 *   counts: int32[4], device or host-mapped pinned memory, written last by one 16-byte store:
 *   {scenarios still active, scenarios with Gamma < -stop_check_tol, active scenarios whose LP
 *   was not OPTIMAL, 0} of this pass. */
int phgpu_fwph_column(phgpu_handle h, const phgpu_fwph_params* prm, int t0, const double* x,
                      const double* obj, const double* bound, const int32_t* status, const double* W,
                      const double* What, const double* rho, const double* xbar, double* gamma,
                      double* dual_bound, int32_t* ncols, double* xq, double* xqx, int32_t* counts,
                      void* stream);

/* _conv_diff (fwph.py:528-547) without its Allreduce: out[0] = sum_s prob_s sum_k (xq - xbar)^2
 * over the local scenarios (xbar: device [nn*S], the OLD x̄).  Per-thread sums in index order,
 * per-block sums in a fixed order, the blocks' sums by a fixed tree in the block with the last
 * ticket (as phgpu_w_diff).  out: device double[1]. */
int phgpu_fwph_diff(phgpu_handle h, const double* xbar, double* out, void* stream);

/* APH (mpisppy/opt/aph.py): everything of one iteration around the subproblem solves, for all
 * local scenarios.  The reference walks its scenarios and nonants in Python four times per
 * iteration (Update_y, Compute_Averages, listener_side_gig, Update_theta_zw), sorts a Python list
 * for the dispatch (:602-632) and calls a solver per dispatched scenario (:642-657); here each is
 * one device pass.  y, z, u and the lagged copies are caller-owned device arrays [nn*S], k-major
 * and scenario-fastest like W; phi, k1, last_phi are [S] doubles; mask, list, last_iter [S] int32.
 * All entries are ordered on the stream and never synchronise, work for any tree and any nn and
 * on a PHGPU_SHARED_MATRIX handle (phgpu_solve_list excepted, see there), use the per-nonant
 * probabilities of phgpu_set_nonant_probs in the node sums where they are set (as
 * phgpu_nonant_stats), and give the same bits on every run.  Each allocates its own workspace at
 * its first call (phgpu_workspace_bytes grows only then).  A step deferred by phgpu_ph_step_defer
 * is run first.  The ranks' sums are the caller's.
 *
 * phgpu_aph_reduce: Update_y (aph.py:151-181) and the local sums of Compute_Averages (:394-408)
 * in one pass.  With first (the reference's _PHIter == 1) y = 0 everywhere; else
 *   y[k, s] = W_use[k, s] + rho[k, s] (x[col_k, s] - z_use[k, s])   where mask[s] != 0
 * (mask NULL: every scenario), and y is kept elsewhere.  W_use / z_use: W and z, or the lagged
 * copies under APHuse_lag (unused with first, may be NULL then).
 *   planes[3 * num_nodes * nlen_max]: three planes, each laid out like one half of node_buf,
 *   over the local scenarios:  sum pcoef x,  sum pcoef x^2,  sum pcoef y  (pcoef: prob_coeff of the
 *   nonant's node, or pvar).  An entry without a nonant is 0.  The node-segmented sum of
 *   phgpu_ph_reduce with three planes: per-wave partials and an ordered final sum where a wave's
 *   scenarios share a node (deterministic); waves that span nodes add by fp64 atomics, exactly
 *   as phgpu_ph_reduce documents. */
int phgpu_aph_reduce(phgpu_handle h, int first, const int32_t* mask, const double* x, const double* W_use,
                     const double* z_use, const double* rho, double* y, double* planes, void* stream);

/* The body of listener_side_gig (aph.py:254-310) after the ranks' sum of the three planes:
 *   xbar[k, s] = plane 0 at the scenario's node entry (scattered),  u[k, s] = x[col_k, s] - xbar[k, s],
 *   phi[s] = p_s sum_k (z - x)(W - y)          (compute_phis_summand, :185-195),
 *   out[4] = { sum_s p_s (|u_s|^2 + |ybar_s|^2 / gamma),  sum_s phi_s,  sum_s p_s |u_s|^2,
 *              sum_s p_s |ybar_s|^2 }          (tau's, phi's, pusqnorm's and pvsqnorm's summands)
 * with ybar_s plane 2 at the scenario's node entries and p_s the scenario's probability.  The sums
 * are per thread in index order, per block in a fixed order and over the blocks by the one with
 * the last ticket (as phgpu_w_diff).  out: device double[4] (or host-mapped), stored by one
 * instruction.  gamma > 0. */
int phgpu_aph_norms(phgpu_handle h, double gamma, const double* planes, const double* x, const double* y,
                    const double* W, const double* z, double* xbar, double* u, double* phi, double* out,
                    void* stream);

/* Update_theta_zw (aph.py:453-496) after the ranks' sum of phgpu_aph_norms' scalars.  red: device
 * double[>= 2] = {tau, phi} reduced; theta is computed on the device, no read-back:
 *   theta = phi nu / tau if tau > 0 and phi > 0, else 0;
 *   W += theta u;   z = xbar (plane 0) with first, else z += theta ybar / gamma;
 *   phi[s] = p_s sum_k (z - x)(W - y) with the new W and z: what the dispatch sorts by (:756);
 *   out[4] = { sum_s p_s |W_s|^2,  sum_s p_s |z_s|^2,  theta,  sum_s phi_s }.
 * out may be host-mapped pinned memory; it is written last, by one store instruction (the
 * contract of conv_local in phgpu_ph_update_ex).  Sums as in phgpu_aph_norms. */
int phgpu_aph_update(phgpu_handle h, int first, double nu, double gamma, const double* red,
                     const double* planes, const double* x, const double* y, const double* u, double* W,
                     double* z, double* phi, double* out, void* stream);

/* The dispatch bookkeeping of APH_solve_loop for the scenarios with mask[s] != 0 (aph.py:646:
 * dispatchrecord gets (iter, phi); _update_foropt :529-550), called after their solve:
 *   last_iter[s] = iter,  last_phi[s] = phi[s],  W_lag[., s] = W[., s],  z_lag[., s] = z[., s]
 * (W_lag and z_lag both NULL: no copies), and for EVERY scenario the first sort key of the next
 * dispatch, as the reference writes its two orders:
 *   round_robin == 0 (:626-629):  k1[s] = -max(last_iter[s], shelf_life - 1)   (second key: phi)
 *   round_robin != 0 (:610-611):  k1[s] = last_iter[s]                         (second key: last_phi)
 * The first of these prefers the scenarios dispatched most recently once iterations pass
 * shelf_life - 1; it is kept as written. */
int phgpu_aph_mark(phgpu_handle h, const int32_t* mask, int32_t iter, int32_t shelf_life, int round_robin,
                   const double* phi, int32_t* last_iter, double* last_phi, double* k1, const double* W,
                   const double* z, double* W_lag, double* z_lag, void* stream);

/* Mark the count local scenarios that are smallest by the lexicographic key (k1[s], k2[s], s):
 * what Python's stable sorted() over the reference's dict order takes first (aph.py:610-629).
 *   k1: device double[S] or NULL (all equal); k2: device double[S]; 1 <= count <= S < 2^31;
 *   mask: device int32[S], 1 for the taken scenarios and 0 for the others;
 *   list: device int32[count], the taken scenarios in ascending s.
 * Keys are finite doubles (-0.0 equals 0.0); what a NaN gives is unspecified (nothing is
 * written out of bounds).  No host read-back: a radix select on the order-preserving 64-bit image
 * of the keys, most significant digit first (6 histogram passes per key over a grid of at most 64
 * workgroups, k1 first, k2 among k1's ties), then a ballot / prefix compaction over the grid
 * that takes the first remaining exact ties in index order.  Histograms and counters are
 * integers: the same result on every run. */
int phgpu_select_smallest(phgpu_handle h, const double* k1, const double* k2, int32_t count, int32_t* mask,
                          int32_t* list, void* stream);

/* A warm solve of the listed scenarios only, in place (the partial APH_solve_loop, aph.py:642-657):
 * their entries of x, y, obj, bound, status, iters (the buffers of the previous phgpu_solve) and
 * their warm-start state are replaced; no other scenario's entry of the caller's buffers or of
 * the handle's warm state is touched.
 *   list: device int32[count], ascending and distinct; 0 <= count <= S.
 * It runs on a PDHG kernel with a list mode: path 5 of the handle's path-6 module where path 6 is
 * the default (the kernel that serves path 6's fallback list), the handle's path-5 module where
 * that is the default, else the global-memory kernel (path 1).  A warm state held in the records
 * (paths 2r, 3) is taken out first; the path-6 epilogue's x̄ partials are invalidated; an
 * uncommitted phgpu_solve_deferred is dropped; the solve is not deferrable.  A full dispatch
 * (count == S) is better served by phgpu_solve, which stays on the handle's default path.
 * Returns 0 and launches nothing for count == 0; -3 on a PHGPU_SHARED_MATRIX handle (the
 * streaming kernel has no list mode yet); -1 before any solve (there is no warm state). */
int phgpu_solve_list(phgpu_handle h, const phgpu_options* opt, const int32_t* list, int32_t count, double* x,
                     double* y, double* obj, double* bound, int32_t* status, int32_t* iters, void* stream);

/* The L-shaped method (mpisppy/opt/lshaped.py), two-stage problems, minimisation: Benders cuts
 * from the fixed solves of all local scenarios and the master LP, on the device.
 *
 *   master:  min sum_g eta_g  over x in R^nn (the ROOT nonants) and eta in R^G (one per cut group)
 *            xlb <= x <= xub,  rl <= R x <= ru,  eta >= etalb,  eta_g - a.x >= b for every cut
 *
 * eta_g models sum_{s in g} prob_s f_s(x), f_s the whole objective of scenario s at first stage x;
 * the scenario with global index s is in group s * G / S_total.  The reference keeps the master as
 * a Pyomo model with one eta per scenario and hands it to an LP solver (lshaped.py:84-230,
 * 600-630); it builds each cut from a scenario's duals in Python (:477-560).  All entries are
 * ordered on the stream and give the same bits on every run; -3 on a PHGPU_SHARED_MATRIX handle
 * and on a tree with more than two stages.
 *
 * phgpu_lshaped_init: allocate the cut store (max_cuts cuts of {group, a[nn], b}; the handle's,
 * counted in phgpu_workspace_bytes, freed by phgpu_destroy or by another init) and take the
 * master's data, all HOST arrays: R [n_rows][nn] dense first-stage rows with sides rl, ru (equal:
 * an equality row), xlb, xub [nn] (infinite sides allowed; xlb < xub, a fixed column is refused with -1), etalb [G] (finite).
 * s_off: the global index of local scenario 0; S_total: the scenarios of all ranks.
 * Limits: nn <= 64, G <= 32, n_rows <= 64; beyond them -1 with a message. */
int phgpu_lshaped_init(phgpu_handle h, int32_t G, int32_t max_cuts, int64_t s_off, int64_t S_total,
                       int32_t n_rows, const double* R, const double* rl, const double* ru,
                       const double* xlb, const double* xub, const double* etalb, void* stream);

/* The cuts of one iteration (lshaped.py:477-520 for every scenario, then the groups' sums),
 * before the ranks' sum.  x [n*S], y [m*S], obj [S], status [S]: the outputs of a solve with the
 * nonants fixed (phgpu_fix_nonants), W off and prox off.  One lane per scenario forms the reduced
 * cost of its fixed columns, d_k = c_k + q_k x_k - sum_i A_ik y_i; then one block per sum adds
 * the scenarios' terms in a fixed order:
 *   cutbuf [G * (nn + 2) + 1], device: per group a_g = sum p_s d_s [nn], b_g = sum p_s (obj_s -
 *   d_s . x_s), Q_g = sum p_s obj_s; last the number of local scenarios that are not OPTIMAL
 *   (they contribute nothing else).  All of it sums over the ranks (phgpu_allreduce_sum).
 * The test of a cut against eta is phgpu_lshaped_append's, after that sum. */
int phgpu_lshaped_cuts(phgpu_handle h, const double* x, const double* y, const double* obj,
                       const int32_t* status, double* cutbuf, void* stream);

/* Append the cuts that cut off eta (lshaped.py:540-560): group g gets {g, a_g, b_g} when
 * Q_g - eta_g > tol max(1, |Q_g|), in group order; a full store takes no more.  eta [G] device.
 *   info: double[5], device or host-mapped pinned memory, one store: {cuts added, sum_g Q_g (the
 *   expected cost at the candidate), cuts held, scenarios not OPTIMAL, cuts wanted}.  wanted >
 *   added means the store was full and cuts were dropped: the caller must not take "no cut
 *   added" for convergence then. */
int phgpu_lshaped_append(phgpu_handle h, const double* cutbuf, const double* eta, double tol,
                         double* info, void* stream);

/* Solve the master (the root solve of lshaped.py:600-630) as one workgroup: a dense fp64
 * primal-dual interior point (Mehrotra's predictor-corrector, steps kept in the wide
 * neighbourhood; the step only centres -- sigma = 1, no second-order term -- while the relative
 * gap is below a tenth of eps_rel or below a tenth of the larger relative residual, so that the
 * gap never runs ahead of the residuals) on the (nn + G)^2 normal matrix in LDS with a Cholesky factor; equality rows by a
 * Schur complement on that factor; diagonal regularisation 1e-13 of each column's own diagonal
 * (1e-10 on an x column without a finite bound).  At most 200 iterations.  opt: eps_rel (primal,
 * dual and gap, relative) and eps_infeas are read; NULL: the defaults.  It starts from the
 * previous master's solution (the store's warm state), the first time from xhat's scenario 0.
 *   xhat [nn*S] device: the solution broadcast to every local scenario (what phgpu_fix_nonants takes);
 *   eta [G] device;  info: double[6], device or host-mapped: {objective (the outer bound), status
 *   (PHGPU_OPTIMAL, PHGPU_ITER_LIMIT, PHGPU_PRIMAL_INFEASIBLE when a Farkas ray was found),
 *   iterations, primal, dual, gap residual}. */
int phgpu_lshaped_master(phgpu_handle h, const phgpu_options* opt, double* xhat, double* eta,
                         double* info, void* stream);

/* The store from and to HOST arrays (tests, checkpoints); both synchronise the stream.
 * load: K <= max_cuts cuts as group [K], a [K][nn], b [K]; it forgets the master's warm state.
 * export: *ncuts and, where not NULL, group, a, b of the cuts held (room for max_cuts). */
int phgpu_lshaped_load(phgpu_handle h, int32_t K, const int32_t* group, const double* a,
                       const double* b, void* stream);
int phgpu_lshaped_export(phgpu_handle h, int32_t* ncuts, int32_t* group, double* a, double* b,
                         void* stream);

/* The extensive form (mpisppy/opt/ef.py ExtensiveForm.solve_extensive_form, mpisppy/opt/sc.py
 * SchurComplement.solve), two-stage continuous problems, minimisation: ONE primal-dual interior
 * point (Mehrotra's predictor-corrector) on the whole extensive form, decomposed by a Schur
 * complement in the ROOT nonants z.  The reference builds one Pyomo model of all
 * scenarios and hands it to a solver (ef.py:60-140), or gives the scenarios' blocks to parapint's
 * Schur-complement linear solver over MPI (sc.py:60-105).  Here a lane per scenario factors
 * N_s = W D W' + E (dense LDL', kept in the store scenario-fastest), the lanes' T' N_s^-1 T and
 * T' N_s^-1 g are summed in a fixed order, one workgroup factors the nn x nn complement C and
 * solves for dz, and a second pass per scenario back-substitutes.  Step lengths, mu and sigma are
 * global.  An iteration is, per right-hand side (stage 0 the predictor, 1 the corrector),
 *
 *   phgpu_ef_schur -> [ranks: sum rsum, max rmax] -> phgpu_ef_direction -> [sum rsum[0:3], max
 *   rmax[0:2]] -> phgpu_ef_step
 *
 * and every rank then holds the same bits of z, of the step lengths and of the test's numbers.
 * All entries are ordered on the stream, none synchronises, the same input gives the same bits;
 * -3 on a PHGPU_SHARED_MATRIX handle and on a tree with more than two stages.
 *
 * phgpu_ef_init: allocate the store (the handle's, counted in phgpu_workspace_bytes, freed by
 * phgpu_destroy or by another init) and set the starting iterate.  HOST arrays [nn]: zlb < zub
 * the nonants' tightest bounds over the scenarios of all ranks (infinite sides allowed; a fixed
 * nonant is refused with -1), cz = sum_s p_s c_s[N], qz = sum_s p_s q_s[N] >= 0.  ncomp: the finite
 * bounds of the whole extensive form (other columns, sides of the rows with rl < ru, z) over all
 * ranks; cmax: max |c| over all ranks; tol: the relative KKT tolerance; qp: 1 takes a common
 * primal and dual step.  Limits: nn <= 64, m <= 64 (any n and nnz); beyond them -1 with a message. */
int phgpu_ef_init(phgpu_handle h, const double* zlb, const double* zub, const double* cz, const double* qz,
                  double ncomp, double cmax, double tol, int32_t qp, void* stream);

/* The scenario pass of one right-hand side and its sums over the local scenarios (device buffers).
 *   stage 0: residuals, N_s and its factor, and
 *     rsum [nn (nn + 1) / 2 + 2 nn + 2] = {sum_s T' N_s^-1 T (lower triangle by rows) | sum_s T' N_s^-1
 *     g_s | sum_s T' y_s | sum of the products slack x dual | sum_s p_s f_s},
 *     rmax [2] = {largest row residual over 1 + its sides, largest dual residual over p_s}
 *   stage 1: the corrector's g on the same factors, rsum [nn] = sum_s T' N_s^-1 g_s.
 * Several ranks sum rsum and take the maximum of rmax (stage 0) before phgpu_ef_direction. */
int phgpu_ef_schur(phgpu_handle h, int32_t stage, double* rsum, double* rmax, void* stream);

/* One workgroup: at stage 0 the test of the iterate, then C = Dz^-1 + rsum's triangle and its
 * Cholesky factor in LDS (kept for stage 1); the solve C dz = -r_z + rsum's right-hand side.  Then
 * the direction pass (dy_s = N_s^-1 (g_s - T dz), dx, dw, the bound duals) and its reductions:
 * rsum [3] = sums of {s dz, ds z, ds dz} (the affine mu is a polynomial in the step lengths),
 * rmax [2] = the largest -ds / s and -dz / z.  Several ranks sum and take the maximum again.
 *   info: double[8], device or host-mapped pinned memory, stored at stage 0 only: {iteration, mu,
 *   primal, dual, gap residual, objective sum_s p_s f_s, done (1: the iterate passes tol; every
 *   later call then leaves the iterate alone), iteration again (stored last)}. */
int phgpu_ef_direction(phgpu_handle h, int32_t stage, double* rsum, double* rmax, double* info, void* stream);

/* stage 0: the affine step lengths, sigma = (mu_aff / mu)^3 (at least 1/2 once mu has not halved in
 * five iterations), the affine direction kept for the second-order term.  stage 1: the step
 * lengths (0.995 of the way to the boundary; the minimum over all scenarios and z), the step. */
int phgpu_ef_step(phgpu_handle h, int32_t stage, const double* rsum, const double* rmax, void* stream);

/* The iterate as a solve's outputs (phgpu_solve's buffers): z in every scenario's nonant columns
 * (bitwise equal over the scenarios), y [m*S] the scenario's own row duals (the extensive form's
 * over p_s; may be NULL), obj = bound = the scenario's own objective, status PHGPU_OPTIMAL once the
 * test passed, else PHGPU_ITER_LIMIT, iters the interior-point iterations.  z [nn] device, may be NULL. */
int phgpu_ef_export(phgpu_handle h, double* x, double* y, double* obj, double* bound, int32_t* status,
                    int32_t* iters, double* z, void* stream);

/* Bundles (spbase.py:219-253, spopt.py:805-836): the local scenarios in G contiguous segments, each
 * the extensive form of its scenarios with the probabilities p_s / p_B, all solved at once by the
 * interior point above in a segmented form: every segment has its own z, Schur
 * complement, mu, step lengths and termination.  The PH terms enter through the nonants' cost and
 * diagonal; a solve reads the handle's W, rho, xbar and W_on / prox_on (phgpu_set_ph_state).  A
 * segment never spans two ranks, so nothing is reduced over the ranks.  All entries are ordered on
 * the stream, none synchronises, the same input gives the same bits.  An iteration is, per
 * right-hand side, phgpu_bundle_schur -> phgpu_bundle_direction -> phgpu_bundle_step.
 *
 * phgpu_bundle_init: allocate the store (the handle's; freed by phgpu_destroy or another init).
 * HOST arrays: seg_start [G + 1] (0 = seg_start[0] < ... < seg_start[G] = S), zlb < zub [G * nn] the
 * nonants' tightest bounds over each segment, ncomp [G] the finite bounds of each segment's
 * extensive form (z's included), cmax [G] its max |c|.  tol: the relative KKT tolerance; ztol: a
 * segment is over when its residuals are at most tol AND the predictor's step of z is at most
 * ztol (1 + max |z|) (the residuals bound the objective, not z: DESIGN.md 3.22); qp: 1 if
 * any q is set (a solve with prox_on takes a common step in any case).  The limits and refusals
 * of phgpu_ef_init hold (-3 shared-matrix handle or more than two stages; -1 nn or m > 64, a
 * segment's nonant without an interior). */
int phgpu_bundle_init(phgpu_handle h, int32_t G, const int32_t* seg_start, const double* zlb, const double* zub,
                      const double* ncomp, const double* cmax, double tol, double ztol, int32_t qp, void* stream);

/* A cold start of every segment: per scenario the solve's cost c + W_on W - prox_on rho xbar and
 * diagonal q + prox_on rho on the nonant columns, the lanes' starting iterate; per segment cz_B =
 * sum_s (p_s / p_B) of that cost, qz_B likewise (sums in index order), z inside its bounds, its
 * duals, and the control scalars zeroed. */
int phgpu_bundle_start(phgpu_handle h, void* stream);

/* The scenario pass (phgpu_ef_schur's) and the segmented reduction of its terms: one thread per
 * (value, segment) adds the segment's scenarios in index order -- no atomics, the same bits on
 * every run.  Optional device copies for inspection (NULL: none): rsum [G][nn (nn + 1) / 2 + 2 nn +
 * 2] and rmax [G][2] in phgpu_ef_schur's layout per segment, terms [values][S] what the lanes gave. */
int phgpu_bundle_schur(phgpu_handle h, int32_t stage, double* rsum, double* rmax, double* terms, void* stream);

/* One wave per segment: its Schur complement in LDS, its factor and the solve for dz, at stage 0
 * followed by the segment's test; then the direction pass and its segmented reduction.  A segment that has
 * passed its test is left alone by every later call; one whose mu or direction is not finite is
 * stopped with the iterate it had (status PHGPU_ITER_LIMIT).
 *   info: double[8], device or host-mapped pinned memory, stored at stage 0 only: {n, segments
 *   still iterating, the worst primal, dual and gap residual among them, segments stopped on a
 *   number that is not finite, the largest iteration count, n again (stored last)}, n counting the
 *   records since phgpu_bundle_init. */
int phgpu_bundle_direction(phgpu_handle h, int32_t stage, double* info, void* stream);

/* One thread per segment: phgpu_ef_step's control step; then the lanes keep the affine direction
 * (stage 0) or step (stage 1). */
int phgpu_bundle_step(phgpu_handle h, int32_t stage, void* stream);

/* The segments' iterates as a solve's outputs, with the meaning phgpu_solve gives them under the
 * same W_on / prox_on: x with the segment's z in the nonant columns (bitwise equal within a
 * segment), y [m*S] (may be NULL) the scenario's row duals over p_s / p_B, obj [S] the scenario's
 * objective with its PH terms, bound = obj (sum_s p_s bound[s] over a segment is p_B times the
 * segment's objective), status PHGPU_OPTIMAL where the segment passed its test, else
 * PHGPU_ITER_LIMIT, iters the segment's interior-point iterations. */
int phgpu_bundle_export(phgpu_handle h, double* x, double* y, double* obj, double* bound, int32_t* status,
                        int32_t* iters, void* stream);

/* The extensive form of a MULTISTAGE problem (mpisppy/opt/ef.py:39-64 with all_nodenames;
 * sputils.create_EF ties the nonants of every non-leaf node): the interior point of phgpu_ef_* with
 * x_s[N_d] = z_{node of s at depth d} for every depth d < D, one mu, one pair of step lengths, one
 * test.  z is the concatenation over the non-leaf nodes, in node order, of
 * nlens[depth] values each (Ztot in all).  The Schur complement in dz is block-sparse with the shape
 * of the tree and is eliminated bottom-up, a wave per node; ROOT's block is solved as phgpu_ef_*
 * solves C.  One rank; all entries are ordered on the stream, none synchronises, no floating-point
 * atomics: the same input gives the same bits.  An iteration is, per right-hand side,
 * phgpu_eft_schur -> phgpu_eft_direction -> phgpu_eft_step.  Between phgpu_eft_init and the first
 * phgpu_eft_schur, phgpu_eft_fix may hold any entries of z at given values: the CONDITIONED extensive
 * form, which with every node above a stage held is the forest of that stage's
 * subtrees in one solve.
 *
 * phgpu_eft_init: allocate the store (the handle's; freed by phgpu_destroy or another init) and set
 * the start.  HOST arrays: nlens [D] the nonants per depth (their sum is the handle's nn, whose
 * nonant slots are ordered by depth); node_depth, node_parent [Nn] the non-leaf nodes numbered depth
 * by depth, node 0 ROOT (parent -1), the children of a node adjacent and in their parents' order;
 * seg_start [G + 1] the contiguous scenario range of each node of depth D - 1, in node order (0 =
 * seg_start[0] < ... < seg_start[G] = S); zlb < zub, cz, qz >= 0 [Ztot] per z entry the tightest
 * bounds and the probability-weighted cost and diagonal over the node's scenarios; ncomp, cmax, tol,
 * qp as phgpu_ef_init.  -3: a shared-matrix handle; -1: D < 2 or not the handle's depth, nn or m >
 * 64, a tree out of that order, an entry of z without an interior. */
int phgpu_eft_init(phgpu_handle h, int32_t D, const int32_t* nlens, int32_t Nn, const int32_t* node_depth,
                   const int32_t* node_parent, const int32_t* seg_start, const double* zlb, const double* zub,
                   const double* cz, const double* qz, double ncomp, double cmax, double tol, int32_t qp, void* stream);

/* Hold entries of z at values (sample_tree.py: the extensive form of a subtree with its ancestors'
 * nonants fixed).  zfix: HOST [Ztot], NaN = the entry stays free.  Once, after phgpu_eft_init and
 * before the first phgpu_eft_schur (another phgpu_eft_init starts over).  A held entry keeps the
 * value's bits to the export: its dz is exactly 0 in both right-hand sides of every iteration, it has
 * no bound duals and takes no part in the complementarity (its finite bounds leave ncomp), in the dual
 * residual of the test, in the step lengths or in the affine mu.  In its node's elimination its row
 * and column are the identity's with right-hand side 0, so what the parent reads gets nothing from
 * it; ROOT's likewise.  Any subset may be held, all of z included (the scenarios then only share mu
 * and the step lengths).  A call with every entry NaN leaves the bits of a solve without it.
 * -1: no store, an iteration has begun, a second call, a value that is not finite or lies outside
 * the entry's [zlb, zub] (the message names the node and the entry). */
int phgpu_eft_fix(phgpu_handle h, const double* zfix, void* stream);

/* The scenario pass (phgpu_ef_schur's, on the scenario's whole path), the segmented sums of its
 * terms per deepest node (a thread or, for long segments, a block per value and segment; index
 * order), the elimination of depth D - 1 .. 1 and ROOT's sums.  Optional device copies for
 * inspection (NULL: none): nodeA [Nn][nn * nn] the lower triangle of every node's P_d x P_d matrix
 * as summed from its scenarios or children, before its own Dz^-1 (stage 0), nodeb [Nn][nn] its
 * right-hand side likewise (rows and columns in path order). */
int phgpu_eft_schur(phgpu_handle h, int32_t stage, double* nodeA, double* nodeb, void* stream);

/* ROOT's test (stage 0), factor and solve as phgpu_ef_direction's, the back-substitution depth 1 ..
 * D - 1, the direction pass and its sums and maxima over the scenarios and the nodes.
 *   info: phgpu_ef_direction's double[8], device or host-mapped pinned memory. */
int phgpu_eft_direction(phgpu_handle h, int32_t stage, double* info, void* stream);

/* phgpu_ef_step over the scenarios and every node's z entries. */
int phgpu_eft_step(phgpu_handle h, int32_t stage, void* stream);

/* phgpu_ef_export: every scenario's nonant columns hold its path's z (bitwise equal between the
 * scenarios that share the node).  z [Ztot] device, may be NULL. */
int phgpu_eft_export(phgpu_handle h, double* x, double* y, double* obj, double* bound, int32_t* status,
                     int32_t* iters, double* z, void* stream);

/* Free the workspace and the handle. */
int phgpu_destroy(phgpu_handle h);

/* Copy the calling thread's last error message (NUL-terminated) into buf. */
int phgpu_last_error(char* buf, size_t len);

/* Workspace bytes held by the handle (diagnostics / memory planning). */
int64_t phgpu_workspace_bytes(phgpu_handle h);

/* Solve-kernel selection of the handle (diagnostics): info[20] =
 * {register path (L <= 64 lanes per scenario): instance or -1, L, column slots / CSC
 *  entries per column / row slots / CSR entries per row needed, the instance's KC, ZC, KR,
 *  ZR;  workgroup path (one workgroup per scenario): instance or -1, waves per scenario,
 *  KC, ZC, KR, ZR;  the default path of phgpu_solve: 1 global, 2 register, 3 workgroup,
 *  4 shared-matrix streaming, 5 pattern-specialised, 6 interior point;  the queue mode of the last
 *  register-path solve: 1 record mode (longest-first queue, scenario-major records), 0
 *  scenario order, -1 none yet;  1 if path 5 applies to the pattern;  the waves per SIMD
 *  of the compiled path-5 kernel, 0 if none is compiled yet}. */
int phgpu_kernel_info(phgpu_handle h, int32_t* info);

/* The ranks' sums of the PH step through the library's own RCCL communicator
 * (comm_rccl.inc), in place of the node-communicator Allreduce of _Compute_Xbar and the
 * Allreduce of convergence_diff (phbase.py:83-87, 339-343; mpisppy/MPI.py's Allreduce over
 * mpi4py).  phgpu_comm_unique_id writes a 128-byte RCCL unique id (call it on one rank and
 * broadcast it); phgpu_comm_init joins the handle's communicator slot (0: the sums issued on
 * the launch stream, 1: those on a side stream -- one user stream per communicator) to the
 * communicator of nranks ranks as rank (collective: every rank calls it, one id per slot);
 * phgpu_allreduce_sum sums n doubles in place over the ranks on stream with the slot's
 * communicator.  RCCL is loaded at run time (the process's librccl.so.1 or the system's);
 * -2 when it is absent. */
int phgpu_comm_unique_id(char* id);
int phgpu_comm_init(phgpu_handle h, const char* id, int nranks, int rank, int slot);
int phgpu_allreduce_sum(phgpu_handle h, int slot, double* buf, int64_t n, void* stream);

/* Path 4 (shared matrix, PDHG) of the last solve: info[2] = {workgroups per scenario of its
 * cluster form (0: one workgroup per scenario slot on the queue; K >= 2: a batch smaller
 * than the GPU, every scenario over K co-resident workgroups with cluster barriers), 1 if
 * the last solve took path 4}.  No reference counterpart (diagnostics). */
int phgpu_stream_info(phgpu_handle h, int32_t* info);

/* Path-6 (interior point) diagnostics: info[16] = {1 if path 6 applies to the pattern,
 * factor entries of the pattern with every row active, 1 if a compiled module spilled
 * and 2 if the module failed to compile or load (path 6 is then not the automatic path
 * until new data arrives by phgpu_set_scenarios), 1 if a module is compiled, rows in its normal
 * equations, its factor entries, its scratch bytes per lane, its hipRTC compile seconds,
 * flops of one LDL' factorisation, flops of one forward + backward solve, lanes per
 * scenario of its IPM kernel (1, or a lane group of 2..16: more lanes for fewer local
 * scenarios, PHGPU_IPM_LANES pins it; 64..256: threads of a workgroup per scenario), PH
 * steps folded into solve launches so far (phgpu_ph_step_defer), the IPM kernel (0 none
 * compiled, 1 one lane, 2 lane groups, 3 workgroup, 4 subtree), and of the last path-6 solve
 * (synchronises): scenarios the subtree kernel found still jammed after its re-centrings
 * (handed to the PDHG fallback, never reported OPTIMAL), re-centrings, and 1 when the
 * one-lane module keeps its slack reciprocals in LDS (a module that spilled otherwise,
 * PHGPU_IPM_LDS=0 turns it off)}: 16 doubles. */
int phgpu_ipm_info(phgpu_handle h, double* info);

/* PHBase.iterk_loop (phbase.py:875-979) of one rank in one cooperative launch (no
 * extension, converger or spoke: the loop's only decision is conv < convthresh):
 *   for it = 1..max_iters: x̄ = the node's pcoef-weighted mean of the last solve's nonants,
 *   W += rho (x - x̄), conv = mean |x - x̄| (phbase.py:27-107, 293-343); stop if conv <
 *   convthresh; solve every local scenario's PH subproblem (path 6, warm-started)
 * with every scenario's data and iterate in registers and x̄ / conv by grid-wide steps.
 * x / y / obj / bound / status / iters as phgpu_solve (x also gives the nonants of the solve
 * before the loop); W and x̄ are the handle's PH state (phgpu_set_ph_state, updated in place);
 * node_buf receives the last step's node sums.  conv_hist (host, max_iters) gets each step's
 * conv; out (host, 4): [0] PH steps taken, [1] 0 limit / 1 conv < convthresh / 2 a solve
 * handed scenarios to the PDHG fallback (solved after the loop; the caller continues step by
 * step), [2] IPM iterations summed over the loop's solves.  Synchronises the stream.
 * Returns -3 (nothing launched) when the handle's state is not one it runs: several nodes
 * per nonant depth, variable probabilities, no prox term, a path other than the one-lane
 * interior point, or more workgroups than fit the GPU at once. */
int phgpu_ph_loop(phgpu_handle h, const phgpu_options* opt, int max_iters, double convthresh, double* x,
                  double* y, double* obj, double* bound, int32_t* status, int32_t* iters, double* node_buf,
                  double* conv_hist, int64_t* out, void* stream);

/* Diagnostics (no reference counterpart): the per-wave timelines of the last path-6 launch,
 * stored by modules compiled with IPM_PROF=1 (PHGPU_IPM_DEFS) on a handle created with
 * PHGPU_IPM_PROF=1 in the environment: 16 words per wave (wave = block * 4 + wave in block):
 * 100 MHz real-time stamps at entry, loop start, loop end, stores done, statistics done and
 * exit, the loop trips, and with IPM_PROF=2 (lane groups) words 8..15 the shader-clock
 * cycles of the loop's phases.  Copies min(n, available) words to out (synchronising the
 * device) and returns the words available (0: no buffer), < 0 on error. */
int64_t phgpu_ipm_prof(phgpu_handle h, unsigned long long* out, int64_t n);

/* The path-6 source the library generates for a pattern and its data flags (host code
 * only; tests and tools).  flags / v0 are per element of [A nnz | c n | q n | lb n | ub n |
 * rl m | ru m]: bit 0 the same value in every scenario, bit 1 finite in some scenario,
 * bit 2 finite in every scenario, bit 3 (rl elements) rl == ru in every scenario; v0 the
 * first scenario's value.  nonant_slot[n]: nonant index of each column or -1; lanes: lanes
 * per scenario of the IPM kernel (1, 2, 4, 8 or 16), or threads of a workgroup per scenario
 * (64, 128, 192 or 256: the subtree kernel for a block-angular pattern unless
 * PHGPU_IPM_BLK=0, else the workgroup kernel).  Writes the
 * NUL-terminated source to buf when len exceeds its length; returns the length + 1 (or a
 * negative error); info[4] (may be NULL) = {rows in the normal equations, factor entries,
 * factorisation flops, solve flops}. */
int phgpu_ipm_source(int32_t n, int32_t m, int32_t nnz, const int32_t* row_ptr, const int32_t* col_idx,
                     const int32_t* nonant_slot, const int32_t* flags, const double* v0, int32_t lanes, char* buf,
                     size_t len, int32_t* info);

#ifdef __cplusplus
}
#endif
#endif /* PHGPU_H */
