// jit_args.h -- the argument block of the path-5 kernel (k_solve_jit), one text for host and
// device: solve_jit.inc includes this file, and __graft_entry__.build embeds it (kJitArgs)
// ahead of the kernel text (jit_kernel.hip.in).  Plain C++: scalars and pointers only, no
// qualifiers, no default member initialisers, no includes.
struct jit_params {
    const double *A, *c, *q, *Dc, *lbh, *ubh, *Dr, *rlh, *ruh, *rl, *ru, *objc, *normA;
    const double *W, *rho, *xbar;
    const double *omega_in, *x_in, *y_in;
    double *omega_out, *x_w, *y_w;
    double *xout, *yout, *obj, *bound;
    int *status, *iters, *qhead;
    const int *list, *list_n;  // scenarios to solve (path 6's fallback list) or null: all
    unsigned long long* stats;  // path 6's solve statistics (counts by status, iteration sum / max) or null
    long long S, first_dyn;
    int W_on, prox_on;
    double eps_rel, eps_abs, bsuff, bnec, bart, eta_frac, omega0, wmin, wmax, eps_inf;
    int max_iter, check_every, restart_every, warm, keep_omega, infeas_start;
};
