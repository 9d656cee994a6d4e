// solve_jit.inc -- path 5: the pattern-specialised register kernel (included by phgpu.hip).
//
// jit_kernel.hip.in (embedded as kJitKernel by __graft_entry__.build) is the whole PDHG
// solve of solve_reg.inc with one lane per scenario; here the host specialises it to one
// handle's sparsity pattern and compiles it with hipRTC for gfx950 (DESIGN.md 3.6):
//
//   * the pattern becomes compile-time expressions (JIT_AX / JIT_ATY: each row's /
//     column's dot product with literal register indices), so A x~ and A^T y are
//     straight-line FMAs on registers -- no LDS hand-off, no padded slots;
//   * per column and row the "kind" -- which bound sides are finite in some scenario,
//     equality rows, which columns can carry a quadratic term -- taken from the data
//     (k_jit_kinds) drops the clamps / prox terms that can never act, and the registers
//     they would hold.
//
// The module is compiled at the first solve that takes path 5 and cached on the handle
// under a key of the pattern and the kinds (a new phgpu_set_scenarios whose kinds differ
// recompiles).  Compilation needs no GPU; loading does.
#include <hip/hiprtc.h>
#include <string>

// jit_params, the kernel's argument block: this very text (jit_args.h, embedded as kJitArgs)
// is what jit_source puts ahead of the kernel, so host and device cannot disagree on it.
// The asserts make a change of its layout a deliberate one.
#include "jit_args.h"
static_assert(sizeof(jit_params) == 384 && offsetof(jit_params, S) == 256 && offsetof(jit_params, eps_rel) == 280 &&
                  offsetof(jit_params, max_iter) == 360,
              "jit_params changed its layout");
#include "jit_args.inc"
#include "jit_kernel.inc"

// limits of the specialisation: the per-lane state must fit the register file
#ifndef JIT_MIN_S
#define JIT_MIN_S (1LL << 62)  // kernel 0 takes path 5 from this many scenarios (PHGPU_JIT=1: always)
#endif
#define JIT_MAX_N 48
#define JIT_MAX_M 48
#define JIT_MAX_NNZ 128

struct jit_module {
    std::string key;       // pattern + kinds the module was built for
    hipModule_t mod = nullptr;
    hipFunction_t fn = nullptr;
    int wpe = 1;           // waves per SIMD the register budget assumes
    int per_cu = 0;        // co-resident workgroups per CU
    double compile_s = 0;  // hipRTC wall time
};

static bool jit_eligible(const phgpu_state* h) {
    return !h->shared && h->n <= JIT_MAX_N && h->m <= JIT_MAX_M && h->nnz <= JIT_MAX_NNZ && h->m >= 1 &&
           (int64_t)std::max(h->nnz, std::max(h->n, h->m)) * h->S < (1LL << 31);
}

// kinds[j] (columns): bit 0 a finite lb in some scenario, bit 1 a finite ub, bit 2 a
// nonzero q; kinds[n + i] (rows): bit 0 a finite rl, bit 1 a finite ru, bit 2 rl != ru
__global__ void __launch_bounds__(256) k_jit_kinds(ph_data st, int32_t* __restrict__ kinds) {
    const int64_t S = st.S;
    const int e = blockIdx.x;
    int bits = 0;
    for (int64_t s = threadIdx.x; s < S; s += 256) {
        if (e < st.n) {
            if (isfinite(st.lb[IX(e)])) bits |= 1;
            if (isfinite(st.ub[IX(e)])) bits |= 2;
            if (st.q[IX(e)] != 0.0) bits |= 4;
        } else {
            const int i = e - st.n;
            const double a = st.rl[IX(i)], b = st.ru[IX(i)];
            if (isfinite(a)) bits |= 1;
            if (isfinite(b)) bits |= 2;
            if (a != b) bits |= 4;
        }
    }
    if (bits) atomicOr(&kinds[e], bits);
}

static std::string jit_chain(const char* var, const std::vector<std::string>& ex) {
    std::string out = ex.back();
    for (int k = (int)ex.size() - 2; k >= 0; --k)
        out = "(" + std::string(var) + " == " + std::to_string(k) + " ? (" + ex[k] + ") : " + out + ")";
    return out;
}

static std::string jit_dot(const std::vector<std::pair<int, int>>& terms, const char* V) {
    if (terms.empty()) return "0.0";
    std::string e = "a[" + std::to_string(terms[0].first) + "] * " + V + "[" + std::to_string(terms[0].second) + "]";
    for (size_t t = 1; t < terms.size(); ++t)
        e = "fma(a[" + std::to_string(terms[t].first) + "], " + V + "[" + std::to_string(terms[t].second) + "], " + e + ")";
    return e;
}

// the generated preamble: sizes, the dot-product expressions, nonant slots and kinds
static std::string jit_preamble(int n, int m, int nnz, const std::vector<int32_t>& rp, const std::vector<int32_t>& ci,
                                const std::vector<int32_t>& slot, const std::vector<int32_t>& kinds, int wpe) {
    std::vector<std::vector<std::pair<int, int>>> cols(n);
    std::vector<std::string> ax(m), aty(n), ns(n), qc(n), ck(n), rk(m);
    for (int i = 0; i < m; ++i) {
        std::vector<std::pair<int, int>> r;
        for (int k = rp[i]; k < rp[i + 1]; ++k) {
            r.push_back({k, ci[k]});
            cols[ci[k]].push_back({k, i});
        }
        ax[i] = jit_dot(r, "XV");
    }
    for (int j = 0; j < n; ++j) {
        aty[j] = jit_dot(cols[j], "YV");
        ns[j] = std::to_string(slot[j]);
        const bool nonant = slot[j] >= 0;
        qc[j] = (nonant || (kinds[j] & 4)) ? "true" : "false";
        // a nonant's bounds can be fixed (phgpu_fix_nonants): both sides are clamped
        ck[j] = std::to_string(nonant ? 3 : (kinds[j] & 3));
    }
    for (int i = 0; i < m; ++i) {
        const int b = kinds[n + i];
        int k = 4;                                   // free
        if ((b & 3) == 3) k = (b & 4) ? 0 : 1;       // ranged / equality
        else if (b & 2) k = 2;                       // upper side only
        else if (b & 1) k = 3;                       // lower side only
        rk[i] = std::to_string(k);
    }
    std::string s;
    s += "#define NC " + std::to_string(n) + "\n#define NR " + std::to_string(m) + "\n#define NZ " + std::to_string(nnz) +
         "\n#define WPE " + std::to_string(wpe) + "\n";
    s += "#define JIT_AX(XV, i) " + jit_chain("i", ax) + "\n";
    s += "#define JIT_ATY(YV, j) " + jit_chain("j", aty) + "\n";
    s += "#define JIT_NS(j) " + jit_chain("j", ns) + "\n";
    s += "#define JIT_QC(j) " + jit_chain("j", qc) + "\n";
    s += "#define JIT_CK(j) " + jit_chain("j", ck) + "\n";
    s += "#define JIT_RK(i) " + jit_chain("i", rk) + "\n";
    return s;
}

// a path-5 module's source: the generated preamble, the argument block, the kernel
static std::string jit_source(const std::string& pre) { return pre + kJitArgs + kJitKernel; }

static int jit_compile(const std::string& src, std::vector<char>& code, bool max_ilp = false) {
    hiprtcProgram prog;
    if (hiprtcCreateProgram(&prog, src.c_str(), "phgpu_jit.hip", 0, nullptr, nullptr) != HIPRTC_SUCCESS)
        return set_err(-2, "hiprtcCreateProgram failed");
    // PHGPU_JIT_OPTS: extra compiler options, space-separated (tuning experiments)
    std::vector<std::string> extra;
    if (const char* e = getenv("PHGPU_JIT_OPTS")) {
        std::string t(e);
        size_t a = 0;
        while (a < t.size()) {
            size_t b = t.find(' ', a);
            if (b == std::string::npos) b = t.size();
            if (b > a) extra.push_back(t.substr(a, b - a));
            a = b + 1;
        }
    }
    std::vector<const char*> opts = {"--gpu-architecture=gfx950", "-O3", "-std=c++17"};
    // the one-lane IPM kernel (one wave per SIMD, latency-bound): LLVM's max-ILP scheduler,
    // 2.5% shorter solves at config 3 (the lane-group kernel was 2% slower with it;
    // profiles/r03/u/)
    if (max_ilp) {
        opts.push_back("-mllvm");
        opts.push_back("-amdgpu-sched-strategy=max-ilp");
    }
    for (const auto& o : extra) opts.push_back(o.c_str());
    const hiprtcResult r = hiprtcCompileProgram(prog, (int)opts.size(), opts.data());
    if (r != HIPRTC_SUCCESS) {
        size_t ls = 0;
        hiprtcGetProgramLogSize(prog, &ls);
        std::string log(ls + 1, '\0');
        if (ls) hiprtcGetProgramLog(prog, &log[0]);
        hiprtcDestroyProgram(&prog);
        return set_err(-2, "hipRTC compile of the path-5 kernel failed: %.400s", log.c_str());
    }
    size_t sz = 0;
    hiprtcGetCodeSize(prog, &sz);
    code.resize(sz);
    hiprtcGetCode(prog, code.data());
    hiprtcDestroyProgram(&prog);
    return 0;
}

// the data-dependent kinds (one synchronisation), then the cached module or a new one
static int jit_prepare(phgpu_state* h, hipStream_t st) {
    const int n = h->n, m = h->m;
    if (h->jit && h->jit_kinds_valid) return 0;
    dev_tmp<int32_t> dk;
    HIPCHK(dk.alloc((size_t)(n + m)));
    HIPCHK(hipMemsetAsync(dk.p, 0, (size_t)(n + m) * sizeof(int32_t), st));
    hipLaunchKernelGGL(k_jit_kinds, dim3((unsigned)(n + m)), dim3(256), 0, st, *h, dk.p);
    std::vector<int32_t> kinds((size_t)(n + m)), slot((size_t)n), rp((size_t)m + 1), ci((size_t)std::max(h->nnz, 1));
    HIPCHK(hipMemcpyAsync(kinds.data(), dk.p, (size_t)(n + m) * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(slot.data(), h->nonant_slot, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(rp.data(), h->row_ptr, (size_t)(m + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (h->nnz)
        HIPCHK(hipMemcpyAsync(ci.data(), h->col_idx, (size_t)h->nnz * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    dk.release();
    const char* env = getenv("PHGPU_JIT_WPE");
    const int wpe = (env && atoi(env) >= 1 && atoi(env) <= 8) ? atoi(env) : 1;
    const std::string pre = jit_preamble(n, m, h->nnz, rp, ci, slot, kinds, wpe);
    if (h->jit && h->jit->key == pre) {
        h->jit_kinds_valid = 1;
        return 0;
    }
    std::vector<char> code;
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = jit_compile(jit_source(pre), code);
    if (rc) return rc;
    jit_module* jm = new jit_module();
    jm->compile_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    jm->key = pre;
    jm->wpe = wpe;
    hipError_t e = hipModuleLoadData(&jm->mod, code.data());
    if (e == hipSuccess) e = hipModuleGetFunction(&jm->fn, jm->mod, "k_solve_jit");
    if (e == hipSuccess) e = hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&jm->per_cu, jm->fn, 256, 0);
    if (e != hipSuccess) {
        module_release(jm);
        return set_err(-2, "loading the path-5 kernel failed: %s", hipGetErrorString(e));
    }
    module_release(h->jit);
    h->jit = jm;
    h->jit_kinds_valid = 1;
    return 0;
}

static int jit_launch(phgpu_state* h, const solve_params& P, double* x, double* y, double* obj, double* bound,
                      int32_t* status, int32_t* iters, hipStream_t st) {
    jit_module* jm = h->jit;
    const int64_t per = (int64_t)(jm->per_cu < 1 ? 1 : jm->per_cu) * h->num_cus * 256;
    int64_t nblk = (std::min<int64_t>(per, h->S) + 255) / 256;
    jit_params a{};
    a.A = h->Ah_csr; a.c = h->c; a.q = h->q; a.Dc = h->Dc; a.lbh = h->lbh; a.ubh = h->ubh; a.Dr = h->Dr;
    a.rlh = h->rlh; a.ruh = h->ruh; a.rl = h->rl; a.ru = h->ru; a.objc = h->objc; a.normA = h->normA;
    a.W = h->W; a.rho = h->rho; a.xbar = h->xbar;
    a.omega_in = h->omega; a.x_in = h->x; a.y_in = h->y;
    a.omega_out = h->omega_w; a.x_w = h->xw; a.y_w = h->yw;
    a.xout = x; a.yout = y; a.obj = obj; a.bound = bound;
    a.status = status; a.iters = iters; a.qhead = h->qhead;
    a.list = nullptr; a.list_n = nullptr; a.stats = nullptr;
    a.S = h->S;
    a.first_dyn = nblk * 256;
    a.W_on = h->W_on; a.prox_on = h->prox_on;
    a.eps_rel = P.eps_rel; a.eps_abs = P.eps_abs; a.bsuff = P.bsuff; a.bnec = P.bnec; a.bart = P.bart;
    a.eta_frac = P.eta_frac; a.omega0 = P.omega0; a.wmin = P.wmin; a.wmax = P.wmax; a.eps_inf = P.eps_inf;
    a.max_iter = P.max_iter; a.check_every = P.check_every; a.restart_every = P.restart_every; a.warm = P.warm;
    a.keep_omega = P.keep_omega; a.infeas_start = P.infeas_start;
    HIPCHK(hipMemsetAsync(h->qhead, 0, sizeof(int), st));
    void* args[] = {&a};
    HIPCHK(hipModuleLaunchKernel(jm->fn, (unsigned)nblk, 1, 1, 256, 1, 1, 0, st, args, nullptr));
    return 0;
}
