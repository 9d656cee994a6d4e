// ipm_args.h -- the argument blocks of the path-6 kernels, one text for host and device:
// solve_ipm.inc includes this file, and __graft_entry__.build embeds it (kIpmArgs) so the
// generator can place it in every path-6 module ahead of the kernel text.  Plain C++ that
// both compilers read alike: structs of scalars and pointers, no qualifiers, no default
// member initialisers, no includes (the host value-initialises, T a{}).  The members are
// written once, in three parts, and the blocks are layers of them: a kernel that takes a
// shorter block is launched with the base sub-object of the longer one, and p.A, p.S, p.ph
// read the same in every kernel.  solve_ipm.inc pins the sizes and a few offsets.

// The one-rank PH step folded into a path-6 solve launch (jit_ph_step.hip.in), on = 0: none
struct ph_step {
    int on, update_W;
    const double* xprev;    // x of the previous solve [n][S] (the one the partials belong to)
    const double* xp;       // its x̄ partials [(chunk NN + k) 2 + {0, 1}]
    const int* xp_dirty;    // chunks to recompute from xprev
    long long xp_n;         // chunks
    int C;                  // scenarios per chunk
    double* node_buf;       // node sums [2 nb_half] (block 0 stores them)
    const int* nb_idx;      // node_buf index of nonant k's (node, offset)
    long long nb_half;      // num_nodes * nlen_max
    double *W, *xbar;       // the PH state (updated in place; the solve then reads it)
    const double* rho;
    double* conv;           // conv_local (pinned host or device memory)
    long long* stats_dst;   // the previous solve's statistics (pinned host or device), or null
    double scale;           // 1 / (S nn)
    double* cpart;          // per-block conv partials
    int* cnt;               // last-block counter (0 between launches)
};

// (No comment here spells a kernel's name: the library and the tests tell a module's kernel
// by searching its source for the name.)

// part 1: the problem, the PH state and the results
struct ipm_params_ptrs {
    const double *A, *c, *q, *lb, *ub, *rl, *ru, *objc;
    const double *lbh, *ubh, *Dc, *Dr;  // working bounds of the nonant columns (fixing) and the scaling
    const double *W, *rho, *xbar;
    const double* omega_in;
    double *omega_out, *x_w, *y_w;  // the warm state the PDHG paths read next
    double *xout, *yout, *obj, *bound;
    int *status, *iters;
    int *fail_list, *fail_n, *zero3;  // fallback list of this solve; the other parity's 3 counters (zeroed)
};
// part 2: sizes, switches, tolerances, the warm state and the statistics
struct ipm_params_ctl {
    long long S;
    int W_on, prox_on;
    double eps_rel, eps_abs, eps_tight;
    int max_ipm;
    const double *x_in, *y_in;  // the warm state a failed scenario hands to the PDHG fallback (null: cold)
    unsigned long long *stats, *stats_zero;  // this solve's statistics; the other parity's (zeroed)
};

// part 3: the x̄ epilogue and the folded PH step
struct ipm_params_xp {
    // x̄ partial sums of this solve (null: none), one chunk = one wave of 64 scenarios (one
    // lane) or one block's 256 / ML_L scenarios (lane groups):
    // xp[(chunk NN + k) 2 + {0, 1}] = sum pcoef x, sum pcoef x^2 of nonant k over the chunk's
    // solved scenarios, xp_node its node, xp_dirty[chunk] = 1 if a scenario of the chunk
    // went to the fallback (the consumer recomputes that chunk from x); DESIGN.md 3.8
    double* xp;
    int *xp_node, *xp_dirty;
    const double* pcoef;
    const int* node_of;
    ph_step ph;
    unsigned long long* prof;  // IPM_PROF: per-wave timelines (phgpu_ipm_prof, jit_ipm_ml.hip.in), or null
};

// The blocks keep the names the kernels have always taken them by (the tests' host
// emulations call the kernels with ipmw_params / ipm_params).
// core: what every path-6 kernel takes, and the whole block of the workgroup kernels
// (jit_ipm_wave.hip.in, jit_ipm_blk.hip.in)
struct ipmw_params : ipm_params_ptrs, ipm_params_ctl {};
// step: core plus the epilogue and the folded step
struct ipm_step_params : ipmw_params, ipm_params_xp {};
// The lane-group kernel (jit_ipm_ml.hip.in) takes the step layer's members with one unused
// pointer after part 1, where its queue head was before its phases split.  The slot stays
// because the kernel's code depends on it: without it the compiler merges the argument loads
// differently and allocates other registers throughout (aircond, 4 lanes).  The host copies
// the three parts of its step block into this one.
struct ipml_params_pad {
    int* unused;
};
struct ipml_params : ipm_params_ptrs, ipml_params_pad, ipm_params_ctl, ipm_params_xp {};

// loop: step plus the PH loop's state -- the one-lane kernel (jit_ipm.hip.in, which ignores the
// tail, and its IPM_LOOP build, phgpu_ph_loop, one rank, two-stage): PHBase.iterk_loop's
// iterations in one cooperative launch -- x̄ / W / conv between the solves by grid-wide steps,
// every scenario's data and iterate kept in registers across the PH iterations
struct ipm_params : ipm_step_params {
    const double* xprev;           // x of the solve before the loop [n][S] (the first step's nonants)
    double *W_w, *xbar_w;          // W and x̄ as the loop leaves them
    double* node_buf;              // the last update's node sums (block 0)
    const int* nb_idx;             // node_buf index of nonant k
    long long nb_half;             // num_nodes * nlen_max
    double* conv_hist;             // conv of every PH step of the loop
    int* loop_out;                 // [0] PH steps, [1] end: 0 limit, 1 conv < thresh, 2 fallback, 3 abort
    unsigned long long* loop_its;  // IPM iterations over the loop's solves (statistics-copies layout)
    double* gpart;                 // [gridDim * 16] block partials (agent-scope atomic exchanges)
    double* gpub;                  // [16] the published grid totals
    unsigned* gsync;               // [2] ticket, publication count (zeroed before the launch)
    double conv_scale;             // 1 / (S nn)
    double convthresh;
    int loop_K;
};
