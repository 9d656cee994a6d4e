// solve_ipm.inc -- path 6: the batched interior-point solve (included by phgpu.hip after
// solve_jit.inc).
//
// jit_ipm.hip.in (embedded as kIpmKernel by __graft_entry__.build) is a Mehrotra
// predictor-corrector IPM with one lane per scenario.  Here the host specialises it to the
// handle's pattern and data and compiles it with hipRTC for gfx950 (DESIGN.md 3.7):
//
//   * data that is the same in every scenario (farmer: all but the 6 yield entries of A;
//     every bound and row side) becomes literal constants -- scalar registers, no loads,
//     no per-lane registers; only what differs is loaded per lane;
//   * the normal-equation matrix M = A D A' + E has the pattern of A A', fixed for the
//     handle: rows are ordered by minimum degree, the LDL' fill is computed symbolically,
//     and assembly, factorisation and the two triangular solves are emitted as
//     straight-line code over the factor's register entries;
//   * the same module holds the path-5 PDHG kernel (jit_kernel.hip.in), launched after
//     the IPM over the scenarios the IPM left on its fallback list (not converged within
//     max_ipm iterations, or an iterate that stopped being finite -- infeasible and
//     unbounded scenarios end there and get their certificates from the PDHG).
//
// What the kernel templates (jit_ipm.hip.in, jit_ipm_ml.hip.in, jit_ipm_wave.hip.in,
// jit_ipm_blk.hip.in) have in common is written once and emitted into every module ahead of
// them: the argument blocks (ipm_args.h, which this file includes too, so the host fills the
// very structs the kernels read -- ipm_fill_args) and the iteration's tunables, statistics
// and reciprocals (jit_ipm_common.hip.in).
//
// The module is compiled at the first path-6 solve (one synchronisation for the data
// flags) and cached under its source text; phgpu_set_scenarios invalidates the flags.
// Nonant bounds are always read per lane (phgpu_fix_nonants changes them without a
// recompile).
#include <map>
#include <set>

#include <array>

// The kernels' argument blocks -- ph_step, the layers ipmw_params < ipm_step_params <
// ipm_params, and the lane-group kernel's ipml_params -- are one text, ipm_args.h (the
// names are the kernels' own of old, which the tests' host emulations spell; their host
// twins are gone): included here for the host, and embedded
// (kIpmArgs) for ipm_source to put into every module, so the two sides cannot disagree.
// The asserts pin the layout the kernels were measured with: changing it is deliberate.
#include "ipm_args.h"
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winvalid-offsetof"  // (the derived layers are not standard-layout)
static_assert(sizeof(ph_step) == 136 && offsetof(ph_step, node_buf) == 48 && offsetof(ph_step, cnt) == 128,
              "ph_step changed its layout");
static_assert(sizeof(ipmw_params) == 304 && offsetof(ipmw_params, S) == 224 &&
                  offsetof(ipmw_params, x_in) == 272 && offsetof(ipmw_params, stats_zero) == 296,
              "ipmw_params changed its layout");
static_assert(sizeof(ipm_step_params) == 488 && offsetof(ipm_step_params, xp) == 304 &&
                  offsetof(ipm_step_params, ph) == 344 && offsetof(ipm_step_params, prof) == 480,
              "ipm_step_params changed its layout");
static_assert(sizeof(ipml_params) == 496 && offsetof(ipml_params, unused) == 224 && offsetof(ipml_params, S) == 232 &&
                  offsetof(ipml_params, xp) == 312 && offsetof(ipml_params, prof) == 488,
              "ipml_params changed its layout");
static_assert(sizeof(ipm_params) == 608 && offsetof(ipm_params, xprev) == 488 &&
                  offsetof(ipm_params, gsync) == 576 && offsetof(ipm_params, loop_K) == 600,
              "ipm_params changed its layout");
#pragma clang diagnostic pop

#include "ipm_args.inc"
#include "ipm_common.inc"
#include "ipm_kernel.inc"
#include "ipm_ml_kernel.inc"
#include "ph_step_kernel.inc"
#include "ipm_wave_kernel.inc"
#include "ipm_wg_common.inc"
#include "ipm_blk_kernel.inc"

#define IPM_MAX_N 40
#define IPM_MAX_M 32
#define IPM_MAX_NNZ 128
#define IPM_MAX_NF 320
#define IPM_SPILL_MAX 1024  // private-segment bytes above which path 6 is not the default
// (and above which a one-lane module gives way to lane groups: aircond at 65,536 scenarios
// spills 524 B per lane on one lane and still runs 0.315 ms per solve against 0.426 on
// lane groups of 4, profiles/r05/c/)
// (PHGPU_IPM_SPILL_MAX=<bytes> moves the threshold: tuning experiments)
// PHGPU_IPM_DEFS="NAME=VALUE;...": extra macro definitions for the generated module (the
// templates' tunables, e.g. IPM_WARM_T; tuning experiments)
// The handle's tuning (phgpu_set_ipm_tuning, same "NAME=VALUE;..." form) is set here while
// ipm_prepare generates that handle's modules; the environment's definitions win over it.
static thread_local const std::string* g_ipm_tuning = nullptr;
static void ipm_parse_defs(const std::string& d, std::vector<std::pair<std::string, std::string>>& out) {
    size_t a = 0;
    while (a < d.size()) {
        size_t b = d.find(';', a);
        if (b == std::string::npos) b = d.size();
        const std::string t = d.substr(a, b - a);
        const size_t q = t.find('=');
        if (!t.empty() && q != std::string::npos && q > 0) {
            const std::string k = t.substr(0, q), v = t.substr(q + 1);
            bool found = false;
            for (auto& kv : out)
                if (kv.first == k) kv.second = v, found = true;
            if (!found) out.emplace_back(k, v);
        }
        a = b + 1;
    }
}
static std::string ipm_env_defs() {
    std::vector<std::pair<std::string, std::string>> kv;
    if (g_ipm_tuning) ipm_parse_defs(*g_ipm_tuning, kv);
    if (const char* e = getenv("PHGPU_IPM_DEFS")) ipm_parse_defs(std::string(e), kv);
    std::string out;
    for (const auto& p : kv) out += "#define " + p.first + " " + p.second + "\n";
    return out;
}
static int ipm_spill_max() {
    const char* e = getenv("PHGPU_IPM_SPILL_MAX");
    return e ? atoi(e) : IPM_SPILL_MAX;
}
#ifndef IPM_MAXIT
#define IPM_MAXIT 80  // IPM iterations before a scenario goes to the PDHG fallback
#endif
#define IPM_ML_MAX_S 8192  // at most this many local scenarios: lane groups
#define IPM_ML_LANES 8
#define IPM_FALLBACK_BLOCKS 16  // workgroups of the fallback launch (4,096 lanes)
#define IPM_EPS_TIGHT 1e-13  // the IPM's own target (PHGPU_IPM_EPS), see jit_ipm.hip.in

struct ipm_module {
    std::string key;  // the generated source the module was built from
    int L = 1;        // lanes per scenario of its IPM kernel (1: k_solve_ipm, else k_solve_ipm_ml;
                      // >= 64: threads per scenario of k_solve_ipm_blk / k_solve_ipm_wave)
    bool blk = false;  // the subtree kernel (jit_ipm_blk.hip.in)
    int per_cu_ipm = 0;
    hipModule_t mod = nullptr;
    hipFunction_t fn_ipm = nullptr, fn_pdhg = nullptr;
    int per_cu_pdhg = 0;
    int private_bytes = 0;  // scratch per lane of the IPM kernel (spills)
    int vgprs = 0;
    double compile_s = 0;
    int mr = 0, nf = 0;  // rows in the normal equations, factor entries
    double fac_flops = 0, sol_flops = 0;  // one LDL' factorisation / one pair of triangular solves
};

// ---------------------------------------------------------------- symbolic analysis
// Rows of M = A D A' are adjacent when they share a column.  Minimum-degree order on the
// active rows, then the LDL' pattern: eliminating row r connects its remaining neighbours
// (the fill), and column r of L holds exactly those neighbours.
struct ipm_symbolic {
    std::vector<int> order;              // active rows in elimination order
    std::vector<int> rank;               // rank[row] (-1 inactive)
    std::vector<std::vector<int>> lcol;  // lcol[row]: rows below it in its L column (ascending rank)
    std::map<std::pair<int, int>, int> pos;  // (row, row') -> factor entry (rank(row) >= rank(row'))
    int nf = 0;
};

// (long_last: among rows of equal current degree eliminate the one with fewer entries of A
// first -- a long linking row goes to the top of the tree, the subtree plan's root)
static ipm_symbolic ipm_analyse(int n, int m, const int32_t* rp, const int32_t* ci, const std::vector<char>& active,
                                bool long_last = false) {
    ipm_symbolic sy;
    std::vector<std::vector<int>> colrows(n);
    for (int i = 0; i < m; ++i)
        if (active[i])
            for (int k = rp[i]; k < rp[i + 1]; ++k) colrows[ci[k]].push_back(i);
    std::vector<std::set<int>> adj(m);
    for (int j = 0; j < n; ++j)
        for (int a : colrows[j])
            for (int b : colrows[j])
                if (a != b) adj[a].insert(b);
    sy.rank.assign(m, -1);
    sy.lcol.assign(m, {});
    std::vector<char> done(m, 0);
    int na = 0;
    for (int i = 0; i < m; ++i) na += active[i] ? 1 : 0;
    for (int step = 0; step < na; ++step) {
        int best = -1;
        for (int i = 0; i < m; ++i)
            if (active[i] && !done[i] &&
                (best < 0 || adj[i].size() < adj[best].size() ||
                 (long_last && adj[i].size() == adj[best].size() && rp[i + 1] - rp[i] < rp[best + 1] - rp[best])))
                best = i;
        done[best] = 1;
        sy.rank[best] = step;
        sy.order.push_back(best);
        std::vector<int> nb(adj[best].begin(), adj[best].end());
        for (int a : nb) {
            adj[a].erase(best);
            for (int b : nb)
                if (a != b) adj[a].insert(b);
        }
        sy.lcol[best] = nb;
        adj[best].clear();
    }
    for (int r : sy.order) {
        std::sort(sy.lcol[r].begin(), sy.lcol[r].end(), [&](int a, int b) { return sy.rank[a] < sy.rank[b]; });
        sy.pos[{r, r}] = sy.nf++;
        for (int i : sy.lcol[r]) sy.pos[{i, r}] = sy.nf++;
    }
    return sy;
}

// the number of factor entries with every row active (create-time eligibility)
static int ipm_nf_bound(int n, int m, const int32_t* rp, const int32_t* ci) {
    if (n > IPM_MAX_N || m > IPM_MAX_M || rp[m] > IPM_MAX_NNZ || m < 1) return -1;
    return ipm_analyse(n, m, rp, ci, std::vector<char>(m, 1)).nf;
}

// ---------------------------------------------------------------- workgroup-IPM plan
// Path 6 for medium scenarios (jit_ipm_wave.hip.in, DESIGN.md 3.9): WT = 64 WPS threads per
// scenario; the elimination tree split into a dense root block and per-thread subtrees
// (tools/ipm_wave_proto.py states the same plan and checks it on the CPU).
#define WAVE_MAX_SLOTS 4     // columns / rows per thread at most
#define WAVE_RMAX 8          // rows of the dense root block at most
#define WAVE_ZR 12           // a row with more entries is a long row (workgroup sums)
#define WAVE_MAX_LR 4        // long rows at most
#define WAVE_MAX_ZC 16       // entries per column at most
#define WAVE_MAX_LDS 7680    // doubles of LDS per workgroup (60 KB)

struct wave_plan {
    bool ok = false;
    int WPS = 0, WT = 0, QC = 0, QR = 0, ZC = 1, ZR = 1, NLR = 0, NFL = 0, lds = 0;
    std::vector<int> lrw, rlng;
    std::vector<int> R, rpos;
    std::vector<int> EP, ER, EDIAG, ECP, ECU, ECF, ECR, EUP, EUT, EUA, EUB;
    std::vector<int> FTP, FTJ, FTK1, FTK2;
    std::vector<int> CRP, CRPP, CRK1, CRK2;
    std::vector<int> cer, cek, cel, rec, rek;
    ipm_symbolic root;  // the dense root block as a symbolic factor (ROOT_FACTOR / ROOT_SOLVE)
    long fac_flops = 0, sol_flops = 0;
    int rows = 0;
};

static wave_plan wave_build(int n, int m, int nnz, const int32_t* rp, const int32_t* ci, const std::vector<char>& active,
                            int want_wps = 0) {
    wave_plan w;
    if (n < 1 || m < 1 || n > 64 * 4 * WAVE_MAX_SLOTS || m > 64 * 4 * WAVE_MAX_SLOTS) return w;
    for (int wps : {1, 2, 3, 4}) {
        if (want_wps > 0 ? wps != want_wps : wps == 3) continue;
        const int wt = 64 * wps;
        if ((n + wt - 1) / wt <= WAVE_MAX_SLOTS && (m + wt - 1) / wt <= WAVE_MAX_SLOTS) {
            w.WPS = wps;
            w.WT = wt;
            break;
        }
    }
    if (!w.WPS) return w;
    const int WT = w.WT;
    w.QC = (n + WT - 1) / WT;
    w.QR = (m + WT - 1) / WT;
    // columns' CSC entries, rows' CSR entries; long rows
    std::vector<std::vector<std::pair<int, int>>> cols(n), rows(m);  // (row, k) / (col, k)
    for (int i = 0; i < m; ++i)
        for (int k = rp[i]; k < rp[i + 1]; ++k) {
            rows[i].push_back({ci[k], k});
            cols[ci[k]].push_back({i, k});
        }
    w.rlng.assign(m, -1);
    for (int i = 0; i < m; ++i)
        if ((int)rows[i].size() > WAVE_ZR) {
            w.rlng[i] = (int)w.lrw.size();
            w.lrw.push_back(i);
        }
    w.NLR = (int)w.lrw.size();
    if (w.NLR > WAVE_MAX_LR) return w;
    for (auto& c : cols) w.ZC = std::max(w.ZC, (int)c.size());
    for (int i = 0; i < m; ++i)
        if (w.rlng[i] < 0) w.ZR = std::max(w.ZR, (int)rows[i].size());
    if (w.ZC > WAVE_MAX_ZC) return w;
    w.cer.assign((size_t)n * w.ZC, m);
    w.cek.assign((size_t)n * w.ZC, -1);
    w.cel.assign((size_t)n * w.ZC, -1);
    for (int j = 0; j < n; ++j)
        for (size_t e = 0; e < cols[j].size(); ++e) {
            w.cer[j * w.ZC + e] = cols[j][e].first;
            w.cek[j * w.ZC + e] = cols[j][e].second;
            w.cel[j * w.ZC + e] = w.rlng[cols[j][e].first];
        }
    w.rec.assign((size_t)m * w.ZR, n);
    w.rek.assign((size_t)m * w.ZR, -1);
    for (int i = 0; i < m; ++i)
        if (w.rlng[i] < 0)
            for (size_t e = 0; e < rows[i].size(); ++e) {
                w.rec[i * w.ZR + e] = rows[i][e].first;
                w.rek[i * w.ZR + e] = rows[i][e].second;
            }
    // symbolic LDL' of the active rows, elimination tree, root set, subtrees -> threads
    const ipm_symbolic sy = ipm_analyse(n, m, rp, ci, active);
    w.rows = (int)sy.order.size();
    std::map<int, int> parent;
    std::map<int, std::vector<int>> kids;
    for (int r : sy.order) {
        parent[r] = sy.lcol[r].empty() ? -1 : sy.lcol[r][0];
        kids[r];
    }
    for (int r : sy.order)
        if (parent[r] >= 0) kids[parent[r]].push_back(r);
    std::map<int, long> cost;
    for (int r : sy.order) {  // rank order: children first
        const long c = (long)sy.lcol[r].size();
        long v = 1 + c + c * (c + 1) / 2;
        for (int k : kids[r]) v += cost[k];
        cost[r] = v;
    }
    std::vector<int> R, comps;
    for (int r : sy.order)
        if (parent[r] < 0) R.push_back(r);
    for (int r : R)
        for (int k : kids[r]) comps.push_back(k);
    while ((int)R.size() < WAVE_RMAX && !comps.empty()) {
        long total = 0;
        int big = comps[0];
        for (int c : comps) {
            total += cost[c];
            if (cost[c] > cost[big]) big = c;
        }
        if (2 * cost[big] > total || ((int)kids[big].size() >= 2 && (int)comps.size() < WT)) {
            R.push_back(big);
            comps.erase(std::find(comps.begin(), comps.end(), big));
            for (int k : kids[big]) comps.push_back(k);
        } else {
            break;
        }
    }
    if ((int)R.size() > WAVE_RMAX) return w;
    std::sort(R.begin(), R.end(), [&](int a, int b) { return sy.rank[a] < sy.rank[b]; });
    w.R = R;
    w.rpos.assign(m, -1);
    for (size_t a = 0; a < R.size(); ++a) w.rpos[R[a]] = (int)a;
    // longest-first packing of the subtrees onto the threads
    std::sort(comps.begin(), comps.end(), [&](int a, int b) { return cost[a] > cost[b] || (cost[a] == cost[b] && a < b); });
    std::vector<long> load(WT, 0);
    std::vector<std::vector<int>> trows(WT);
    for (int c : comps) {
        const int l = (int)(std::min_element(load.begin(), load.end()) - load.begin());
        load[l] += cost[c];
        std::vector<int> stack{c};
        while (!stack.empty()) {
            const int r = stack.back();
            stack.pop_back();
            trows[l].push_back(r);
            for (int k : kids[r]) stack.push_back(k);
        }
    }
    // FL numbering: each non-root row's diagonal then its L column, in rank order
    std::map<std::pair<int, int>, int> fpos;
    for (int r : sy.order) {
        if (w.rpos[r] >= 0) continue;
        fpos[{r, r}] = w.NFL++;
        for (int u : sy.lcol[r]) fpos[{u, r}] = w.NFL++;
    }
    auto pair_of = [](int a, int b) { return a * (a + 1) / 2 + b; };
    auto terms_of = [&](int u, int r, std::vector<int>& J, std::vector<int>& K1, std::vector<int>& K2) {
        for (auto& er : rows[r])
            for (auto& eu : rows[u])
                if (er.first == eu.first) {
                    J.push_back(er.first);
                    K1.push_back(eu.second);
                    K2.push_back(er.second);
                }
    };
    w.FTP.assign(w.NFL + 1, 0);
    {
        std::vector<std::vector<int>> tj(w.NFL), t1(w.NFL), t2(w.NFL);
        for (auto& kv : fpos) terms_of(kv.first.first, kv.first.second, tj[kv.second], t1[kv.second], t2[kv.second]);
        for (int f = 0; f < w.NFL; ++f) {
            w.FTP[f + 1] = w.FTP[f] + (int)tj[f].size();
            w.FTJ.insert(w.FTJ.end(), tj[f].begin(), tj[f].end());
            w.FTK1.insert(w.FTK1.end(), t1[f].begin(), t1[f].end());
            w.FTK2.insert(w.FTK2.end(), t2[f].begin(), t2[f].end());
        }
    }
    // each thread's rows in rank order: diagonal, L entries, Schur updates
    w.EP.assign(WT + 1, 0);
    w.ECP.push_back(0);
    w.EUP.push_back(0);
    for (int l = 0; l < WT; ++l) {
        std::sort(trows[l].begin(), trows[l].end(), [&](int a, int b) { return sy.rank[a] < sy.rank[b]; });
        for (int r : trows[l]) {
            w.ER.push_back(r);
            w.EDIAG.push_back(fpos.at({r, r}));
            const auto& lc = sy.lcol[r];
            for (int u : lc) {
                w.ECU.push_back(u);
                w.ECF.push_back(fpos.at({u, r}));
                w.ECR.push_back(w.rpos[u]);
            }
            w.ECP.push_back((int)w.ECU.size());
            for (size_t a = 0; a < lc.size(); ++a)
                for (size_t b = 0; b <= a; ++b) {  // lc is in rank order: rank(lc[a]) >= rank(lc[b])
                    const int u = lc[a], v = lc[b];
                    if (w.rpos[u] >= 0 && w.rpos[v] >= 0) w.EUT.push_back(-1 - pair_of(w.rpos[u], w.rpos[v]));
                    else w.EUT.push_back(fpos.at({u, v}));
                    w.EUA.push_back((int)a);
                    w.EUB.push_back((int)b);
                }
            w.EUP.push_back((int)w.EUT.size());
            const long c = (long)lc.size();
            w.fac_flops += 4 + c + 3 * c * (c + 1) / 2;
            w.sol_flops += 4 * c + 1;
        }
        w.EP[l + 1] = (int)w.ER.size();
    }
    // root-block assembly terms by column
    w.CRP.assign(n + 1, 0);
    for (int j = 0; j < n; ++j) {
        for (auto& ea : cols[j])
            for (auto& eb : cols[j]) {
                const int a = ea.first < m ? w.rpos[ea.first] : -1, b = eb.first < m ? w.rpos[eb.first] : -1;
                if (a < 0 || b < 0 || b > a) continue;
                w.CRPP.push_back(pair_of(a, b));
                w.CRK1.push_back(ea.second);
                w.CRK2.push_back(eb.second);
            }
        w.CRP[j + 1] = (int)w.CRPP.size();
    }
    // the dense root block as a symbolic factor
    const int nR = (int)R.size();
    w.root.rank.assign(std::max(nR, 1), -1);
    w.root.lcol.assign(std::max(nR, 1), {});
    for (int a = 0; a < nR; ++a) {
        w.root.order.push_back(a);
        w.root.rank[a] = a;
        for (int b = a + 1; b < nR; ++b) w.root.lcol[a].push_back(b);
    }
    for (int a = 0; a < nR; ++a)
        for (int b = 0; b <= a; ++b) w.root.pos[{a, b}] = pair_of(a, b);
    w.root.nf = nR * (nR + 1) / 2;
    for (int a = 0; a < nR; ++a) {
        const long c = nR - 1 - a;
        w.fac_flops += 4 + c + c * (c + 1);
        w.sol_flops += 4 * c + 1;
    }
    const int RRv = nR * (nR + 1) / 2, nred = std::max(RRv, 8);
    w.lds = nnz + (n + 2) + 2 * (m + 2) + (w.NFL + 1) + w.WPS * (nred + w.NLR + 4);
    if (w.lds > WAVE_MAX_LDS) return w;
    w.ok = true;
    return w;
}

// WPS of the workgroup IPM for the pattern with every row active (0: not eligible)
static int ipm_wave_bound(int n, int m, int nnz, const int32_t* rp, const int32_t* ci) {
    if (n > 64 * 4 * WAVE_MAX_SLOTS || m > 64 * 4 * WAVE_MAX_SLOTS) return 0;
    const wave_plan w = wave_build(n, m, nnz, rp, ci, std::vector<char>(m, 1));
    return w.ok ? w.WPS : 0;
}

// the one-lane / lane-group IPM applies (small scenarios with the path-5 fallback)
static bool ipm_small(const phgpu_state* h) { return h->ipm_nf > 0 && h->ipm_nf <= IPM_MAX_NF && jit_eligible(h); }

static bool ipm_eligible(const phgpu_state* h) {
    const char* we = getenv("PHGPU_IPM_WAVE");  // 0: no workgroup IPM (A/B experiments)
    return !h->shared && (ipm_small(h) || (h->ipm_wave > 0 && !(we && atoi(we) == 0)));
}

// ---------------------------------------------------------------- data flags
// Element e of [A nnz | c n | q n | lb n | ub n | rl m | ru m]: bit 0 the same bits in every
// scenario, bit 1 finite in some scenario, bit 2 finite in every scenario, bit 3 (rl
// entries) rl == ru in every scenario; v0[e] = scenario 0's value.
#define IPMF_UNI 1
#define IPMF_FIN_ANY 2
#define IPMF_FIN_ALL 4
#define IPMF_EQ 8

__global__ void __launch_bounds__(256) k_ipm_flags(ph_data st, int32_t* __restrict__ flags,
                                                   double* __restrict__ v0) {
    const int64_t S = st.S;
    const int n = st.n, m = st.m, nnz = st.nnz;
    int e = blockIdx.x, k = e;
    const double* arr;
    if (k < nnz) arr = st.A;
    else if ((k -= nnz) < n) arr = st.c;
    else if ((k -= n) < n) arr = st.q;
    else if ((k -= n) < n) arr = st.lb;
    else if ((k -= n) < n) arr = st.ub;
    else if ((k -= n) < m) arr = st.rl;
    else {
        k -= m;
        arr = st.ru;
    }
    const bool is_rl = arr == st.rl;
    __shared__ int any, all;
    if (threadIdx.x == 0) any = 0, all = IPMF_UNI | IPMF_FIN_ALL | (is_rl ? IPMF_EQ : 0);
    __syncthreads();
    const double first = arr[(size_t)k * S];
    int a = 0, b = IPMF_UNI | IPMF_FIN_ALL | (is_rl ? IPMF_EQ : 0);
    for (int64_t s = threadIdx.x; s < S; s += 256) {
        const double v = arr[(size_t)k * S + s];
        if (__double_as_longlong(v) != __double_as_longlong(first)) b &= ~IPMF_UNI;
        if (isfinite(v)) a |= IPMF_FIN_ANY;
        else b &= ~IPMF_FIN_ALL;
        if (is_rl && !(isfinite(v) && st.ru[(size_t)k * S + s] == v)) b &= ~IPMF_EQ;
    }
    if (a) atomicOr(&any, a);
    atomicAnd(&all, b);
    __syncthreads();
    if (threadIdx.x == 0) {
        flags[e] = any | all;
        v0[e] = first;
    }
}

// ---------------------------------------------------------------- code generation
static std::string ipm_lit(double v) {
    if (std::isinf(v)) return v > 0 ? "(__builtin_inf())" : "(-__builtin_inf())";
    char b[64];
    snprintf(b, sizeof b, "(%a)", v);
    return b;
}

static std::string ipm_chain(const char* var, const std::vector<std::string>& ex) {
    if (ex.empty()) return "0";
    return jit_chain(var, ex);
}

static std::string ipm_dot(const std::vector<std::pair<int, int>>& terms, const char* V) {
    return jit_dot(terms, V);
}

template <class T>
static std::string ipm_table(const char* type, const char* name, const std::vector<T>& v,
                             std::string (*fmt)(T)) {
    std::string s = std::string("static __device__ const ") + type + " " + name + "[] = {";
    if (v.empty()) s += fmt(T());
    for (size_t k = 0; k < v.size(); ++k) s += (k ? ", " : "") + fmt(v[k]);
    return s + "};\n";
}

// NN and the nonants' columns / depths for the x̄ partials of the IPM epilogues
// (nonant k is the column j with slot[j] == k; ndep[k] its tree depth, null = 0)
static std::string ipm_nonant_defs(int n, const int32_t* slot, const int32_t* ndep) {
    int nn = 0;
    for (int j = 0; j < n; ++j) nn = std::max(nn, slot[j] + 1);
    std::vector<std::string> col(std::max(nn, 1), "0"), dep(std::max(nn, 1), "0");
    std::vector<int> depv(std::max(nn, 1), 0);
    for (int j = 0; j < n; ++j)
        if (slot[j] >= 0) col[slot[j]] = std::to_string(j);
    for (int k = 0; k < nn; ++k) {
        depv[k] = ndep ? ndep[k] : 0;
        dep[k] = std::to_string(depv[k]);
    }
    std::vector<int> colv(std::max(nn, 1), 0);
    for (int j = 0; j < n; ++j)
        if (slot[j] >= 0) colv[slot[j]] = j;
    std::string s = "#define NN " + std::to_string(nn) + "\n";
    s += ipm_table<int>("int", "NDEP", depv, [](int v) { return std::to_string(v); });
    s += ipm_table<int>("int", "NCOLT", colv, [](int v) { return std::to_string(v); });
    return s + "#define INCOL(k) " + ipm_chain("k", col) + "\n#define INDEP(k) " + ipm_chain("k", dep) + "\n";
}

// the preamble of the IPM kernel (everything jit_ipm.hip.in expects); info[0] = active
// rows, info[1] = factor entries
static std::string ipm_preamble(int n, int m, int nnz, const int32_t* rp, const int32_t* ci, const int32_t* slot,
                                const int32_t* flags, const double* v0, int wpe, int* info) {
    const int oc = nnz, oq = nnz + n, olb = nnz + 2 * n, oub = nnz + 3 * n, orl = nnz + 4 * n, oru = nnz + 4 * n + m;
    auto kind = [&](int e) -> int {  // 0 never finite, 1 uniform finite, 2 per scenario
        if (!(flags[e] & IPMF_FIN_ANY)) return 0;
        return ((flags[e] & IPMF_UNI) && (flags[e] & IPMF_FIN_ALL)) ? 1 : 2;
    };
    std::vector<char> active(m);
    for (int i = 0; i < m; ++i) active[i] = (kind(orl + i) != 0 || kind(oru + i) != 0) ? 1 : 0;
    const ipm_symbolic sy = ipm_analyse(n, m, rp, ci, active);
    if (info) {
        info[0] = (int)sy.order.size(), info[1] = sy.nf;
        long fl = 0;
        for (int r : sy.order) {
            const long c = (long)sy.lcol[r].size();
            fl += 4 + c + c * (c + 1);  // pivot reciprocal, the column's scaling, its Schur update
        }
        info[2] = (int)fl;
        info[3] = 4 * (sy.nf - (int)sy.order.size()) + (int)sy.order.size();
    }

    std::vector<std::string> au(nnz), av(nnz), cu(n), cv(n), qk(n), qv(n), lk(n), lv(n), uk(n), uv(n), ns(n);
    std::vector<std::string> rlk(m), rlv(m), ruk(m), ruv(m), eq(m), act(m), ax(m), aty(n);
    std::vector<std::vector<std::pair<int, int>>> cols(n);
    for (int i = 0; i < m; ++i) {
        std::vector<std::pair<int, int>> r;
        for (int k = rp[i]; k < rp[i + 1]; ++k) {
            r.push_back({k, ci[k]});
            cols[ci[k]].push_back({k, i});
        }
        ax[i] = ipm_dot(r, "XV");
    }
    for (int k = 0; k < nnz; ++k) {
        au[k] = (flags[k] & IPMF_UNI) ? "true" : "false";
        av[k] = (flags[k] & IPMF_UNI) ? ipm_lit(v0[k]) : "0.0";
    }
    for (int j = 0; j < n; ++j) {
        aty[j] = ipm_dot(cols[j], "YV");
        ns[j] = std::to_string(slot[j]);
        const bool cu_ = (flags[oc + j] & IPMF_UNI) && std::isfinite(v0[oc + j]);
        cu[j] = cu_ ? "true" : "false";
        cv[j] = cu_ ? ipm_lit(v0[oc + j]) : "0.0";
        const bool qu = (flags[oq + j] & IPMF_UNI) && std::isfinite(v0[oq + j]);
        qk[j] = qu ? (v0[oq + j] == 0.0 ? "0" : "1") : "2";
        qv[j] = qu ? ipm_lit(v0[oq + j]) : "0.0";
        lk[j] = std::to_string(kind(olb + j));
        lv[j] = kind(olb + j) == 1 ? ipm_lit(v0[olb + j]) : "0.0";
        uk[j] = std::to_string(kind(oub + j));
        uv[j] = kind(oub + j) == 1 ? ipm_lit(v0[oub + j]) : "0.0";
    }
    for (int i = 0; i < m; ++i) {
        rlk[i] = std::to_string(kind(orl + i));
        rlv[i] = kind(orl + i) == 1 ? ipm_lit(v0[orl + i]) : "0.0";
        ruk[i] = std::to_string(kind(oru + i));
        ruv[i] = kind(oru + i) == 1 ? ipm_lit(v0[oru + i]) : "0.0";
        eq[i] = (flags[orl + i] & IPMF_EQ) ? "true" : "false";
        act[i] = active[i] ? "true" : "false";
    }
    // straight-line assembly / factorisation / solves over F[] (factor entries), DI[] / MD[] / R[] (rows)
    auto P = [&](int a, int b) { return sy.pos.at({a, b}); };
    std::string asmb, fac, sol;
    for (int f = 0; f < sy.nf; ++f) asmb += "F[" + std::to_string(f) + "] = 0.0; ";
    for (int j = 0; j < n; ++j) {
        std::vector<std::pair<int, int>> ent;  // (row, k) of the active rows
        for (auto& e : cols[j])
            if (active[e.second]) ent.push_back({e.second, e.first});
        if (ent.empty()) continue;
        asmb += "{ ";
        for (auto& e1 : ent) {
            asmb += "const double t" + std::to_string(e1.second) + " = a[" + std::to_string(e1.second) + "] * DX[" +
                    std::to_string(j) + "]; ";
            for (auto& e2 : ent) {
                if (sy.rank[e2.first] > sy.rank[e1.first]) continue;
                const std::string f = std::to_string(P(e1.first, e2.first));
                asmb += "F[" + f + "] = fma(t" + std::to_string(e1.second) + ", a[" + std::to_string(e2.second) +
                        "], F[" + f + "]); ";
            }
        }
        asmb += "} ";
    }
    for (int r : sy.order) {
        const std::string d = std::to_string(P(r, r)), rs = std::to_string(r);
        asmb += "F[" + d + "] += EI[" + rs + "]; MD[" + rs + "] = F[" + d + "]; ";
    }
    for (int r : sy.order) {
        const std::string d = std::to_string(P(r, r)), rs = std::to_string(r);
        fac += "{ double d_ = F[" + d + "]; d_ = (d_ > 1e-30 * MD[" + rs + "]) ? d_ : 1e128; const double id_ = i_rcpi(d_); DI[" +
               rs + "] = id_; ";
        const auto& lc = sy.lcol[r];
        for (size_t u = 0; u < lc.size(); ++u) {
            const std::string f = std::to_string(P(lc[u], r));
            fac += "const double u" + std::to_string(u) + " = F[" + f + "]; F[" + f + "] = u" + std::to_string(u) +
                   " * id_; ";
        }
        for (size_t u = 0; u < lc.size(); ++u)
            for (size_t v = 0; v <= u; ++v) {
                const std::string f = std::to_string(P(lc[u], lc[v]));
                fac += "F[" + f + "] = fma(-u" + std::to_string(u) + ", F[" + std::to_string(P(lc[v], r)) + "], F[" + f +
                       "]); ";
            }
        fac += "} ";
    }
    for (int r : sy.order)
        for (int i : sy.lcol[r])
            sol += "R[" + std::to_string(i) + "] = fma(-F[" + std::to_string(P(i, r)) + "], R[" + std::to_string(r) +
                   "], R[" + std::to_string(i) + "]); ";
    for (int r : sy.order) sol += "R[" + std::to_string(r) + "] *= DI[" + std::to_string(r) + "]; ";
    for (auto it = sy.order.rbegin(); it != sy.order.rend(); ++it)
        for (int i : sy.lcol[*it])
            sol += "R[" + std::to_string(*it) + "] = fma(-F[" + std::to_string(P(i, *it)) + "], R[" + std::to_string(i) +
                   "], R[" + std::to_string(*it) + "]); ";

    double gam = 1.0;
    for (int j = 0; j < n; ++j)
        if (std::isfinite(v0[oc + j])) gam = std::max(gam, std::fabs(v0[oc + j]));
    std::string s;
    s += "#define IPM_GAM " + ipm_lit(gam) + "\n";
    // PHGPU_IPM_MEHROTRA=1: predictor + corrector per iteration (fewer iterations, twice
    // the live registers); default one solve per iteration (DESIGN.md 3.7)
    const char* me = getenv("PHGPU_IPM_MEHROTRA");
    s += std::string("#define IPM_MEHROTRA ") + ((me && atoi(me) == 1) ? "1" : "0") + "\n";
    s += ipm_env_defs();
    s += "#define NC " + std::to_string(n) + "\n#define NR " + std::to_string(m) + "\n#define NZ " + std::to_string(nnz) +
         "\n#define NF " + std::to_string(std::max(sy.nf, 1)) + "\n#define IPM_WPE " + std::to_string(wpe) + "\n";
    s += "#define IA_U(k) " + ipm_chain("k", au) + "\n#define IA_V(k) " + ipm_chain("k", av) + "\n";
    s += "#define IC_U(j) " + ipm_chain("j", cu) + "\n#define IC_V(j) " + ipm_chain("j", cv) + "\n";
    s += "#define IQ_K(j) " + ipm_chain("j", qk) + "\n#define IQ_V(j) " + ipm_chain("j", qv) + "\n";
    s += "#define ILB_K(j) " + ipm_chain("j", lk) + "\n#define ILB_V(j) " + ipm_chain("j", lv) + "\n";
    s += "#define IUB_K(j) " + ipm_chain("j", uk) + "\n#define IUB_V(j) " + ipm_chain("j", uv) + "\n";
    s += "#define IRL_K(i) " + ipm_chain("i", rlk) + "\n#define IRL_V(i) " + ipm_chain("i", rlv) + "\n";
    s += "#define IRU_K(i) " + ipm_chain("i", ruk) + "\n#define IRU_V(i) " + ipm_chain("i", ruv) + "\n";
    s += "#define IEQ(i) " + ipm_chain("i", eq) + "\n#define IACT(i) " + ipm_chain("i", act) + "\n";
    s += "#define INS(j) " + ipm_chain("j", ns) + "\n";
    std::vector<std::string> rfix(m);
    for (int i = 0; i < m; ++i) {
        std::string e = "true";
        for (int k = rp[i]; k < rp[i + 1]; ++k) e += " && fx[" + std::to_string(ci[k]) + "]";
        rfix[i] = "(" + e + ")";
    }
    s += "#define IPM_ROWFIX(i) " + ipm_chain("i", rfix) + "\n";
    s += "#define IPM_AX(XV, i) " + ipm_chain("i", ax) + "\n#define IPM_ATY(YV, j) " + ipm_chain("j", aty) + "\n";
    s += "#define IPM_ASSEMBLE(F, DX, EI) do { " + asmb + "} while (0)\n";
    s += "#define IPM_FACTOR(F, DI, MD) do { " + fac + "} while (0)\n";
    s += "#define IPM_SOLVE(F, DI, R) do { " + sol + "} while (0)\n";
    return s;
}

// The factorisation / solve macros of a symbolic analysis (shared by both kernels)
static void ipm_fac_sol_text(const ipm_symbolic& sy, std::string& fac, std::string& sol) {
    auto P = [&](int a, int b) { return sy.pos.at({a, b}); };
    for (int r : sy.order) {
        const std::string d = std::to_string(P(r, r)), rs = std::to_string(r);
        fac += "{ double d_ = F[" + d + "]; d_ = (d_ > 1e-30 * MD[" + rs + "]) ? d_ : 1e128; const double id_ = i_rcpi(d_); DI[" +
               rs + "] = id_; ";
        const auto& lc = sy.lcol[r];
        for (size_t u = 0; u < lc.size(); ++u) {
            const std::string f = std::to_string(P(lc[u], r));
            fac += "const double u" + std::to_string(u) + " = F[" + f + "]; F[" + f + "] = u" + std::to_string(u) +
                   " * id_; ";
        }
        for (size_t u = 0; u < lc.size(); ++u)
            for (size_t v = 0; v <= u; ++v) {
                const std::string f = std::to_string(P(lc[u], lc[v]));
                fac += "F[" + f + "] = fma(-u" + std::to_string(u) + ", F[" + std::to_string(P(lc[v], r)) + "], F[" + f +
                       "]); ";
            }
        fac += "} ";
    }
    for (int r : sy.order)
        for (int i : sy.lcol[r])
            sol += "R[" + std::to_string(i) + "] = fma(-F[" + std::to_string(P(i, r)) + "], R[" + std::to_string(r) +
                   "], R[" + std::to_string(i) + "]); ";
    for (int r : sy.order) sol += "R[" + std::to_string(r) + "] *= DI[" + std::to_string(r) + "]; ";
    for (auto it = sy.order.rbegin(); it != sy.order.rend(); ++it)
        for (int i : sy.lcol[*it])
            sol += "R[" + std::to_string(*it) + "] = fma(-F[" + std::to_string(P(i, *it)) + "], R[" + std::to_string(i) +
                   "], R[" + std::to_string(*it) + "]); ";
}

static std::string ipm_fmt_i(int v) { return std::to_string(v); }
static std::string ipm_fmt_d(double v) { return std::isfinite(v) ? ipm_lit(v) : "0.0"; }

// The preamble of the multi-lane kernel (jit_ipm_ml.hip.in) for L lanes per scenario
static std::string ipm_ml_preamble(int n, int m, int nnz, const int32_t* rp, const int32_t* ci, const int32_t* slot,
                                   const int32_t* flags, const double* v0, int L, int* info) {
    const int oc = nnz, oq = nnz + n, olb = nnz + 2 * n, oub = nnz + 3 * n, orl = nnz + 4 * n, oru = nnz + 4 * n + m;
    auto kind = [&](int e) -> int {
        if (!(flags[e] & IPMF_FIN_ANY)) return 0;
        return ((flags[e] & IPMF_UNI) && (flags[e] & IPMF_FIN_ALL)) ? 1 : 2;
    };
    std::vector<char> active(m);
    for (int i = 0; i < m; ++i) active[i] = (kind(orl + i) != 0 || kind(oru + i) != 0) ? 1 : 0;
    const ipm_symbolic sy = ipm_analyse(n, m, rp, ci, active);
    if (info) {
        info[0] = (int)sy.order.size(), info[1] = sy.nf;
        long fl = 0;
        for (int r : sy.order) {
            const long c = (long)sy.lcol[r].size();
            fl += 4 + c + c * (c + 1);
        }
        info[2] = (int)fl;
        info[3] = 4 * (sy.nf - (int)sy.order.size()) + (int)sy.order.size();
    }
    const int NF = std::max(sy.nf, 1);
    const int QC = (n + L - 1) / L, QR = (m + L - 1) / L, QF = (NF + L - 1) / L;
    std::vector<std::vector<std::pair<int, int>>> cols(n), rows(m);  // (row, k) / (col, k)
    for (int i = 0; i < m; ++i)
        for (int k = rp[i]; k < rp[i + 1]; ++k) {
            rows[i].push_back({ci[k], k});
            cols[ci[k]].push_back({i, k});
        }
    int ZC = 1, ZR = 1;
    for (auto& c : cols) ZC = std::max(ZC, (int)c.size());
    for (auto& r : rows) ZR = std::max(ZR, (int)r.size());
    std::vector<int> tcj(QC * L), tri(QR * L), cer(n * ZC, m), cek(n * ZC, -1), rec(m * ZR, n), rek(m * ZR, -1);
    for (int k = 0; k < QC * L; ++k) tcj[k] = k < n ? k : -1;
    for (int k = 0; k < QR * L; ++k) tri[k] = k < m ? k : -1;
    for (int j = 0; j < n; ++j)
        for (size_t e = 0; e < cols[j].size(); ++e) cer[j * ZC + e] = cols[j][e].first, cek[j * ZC + e] = cols[j][e].second;
    for (int i = 0; i < m; ++i)
        for (size_t e = 0; e < rows[i].size(); ++e) rec[i * ZR + e] = rows[i][e].first, rek[i * ZR + e] = rows[i][e].second;
    // factor entries: index -> (row a, row b); terms over the common columns
    std::vector<std::pair<int, int>> ent(NF, {-1, -1});
    for (auto& kv : sy.pos) ent[kv.second] = kv.first;
    std::vector<std::vector<std::array<int, 3>>> terms(NF);
    int ZT = 1;
    for (int f = 0; f < sy.nf; ++f) {
        const int a = ent[f].first, b = ent[f].second;
        for (auto& ea : rows[a])
            for (auto& eb : rows[b])
                if (ea.first == eb.first) terms[f].push_back({ea.first, ea.second, eb.second});
        ZT = std::max(ZT, (int)terms[f].size());
    }
    std::vector<int> ftj(NF * ZT, n), ftk1(NF * ZT, -1), ftk2(NF * ZT, -1), fdr(NF, -1);
    for (int f = 0; f < sy.nf; ++f) {
        for (size_t t = 0; t < terms[f].size(); ++t)
            ftj[f * ZT + t] = terms[f][t][0], ftk1[f * ZT + t] = terms[f][t][1], ftk2[f * ZT + t] = terms[f][t][2];
        if (ent[f].first == ent[f].second) fdr[f] = ent[f].first;
    }
    std::vector<int> au(nnz), cu(n), qk(n), lk(n), uk(n), nsl(n), rlk(m), ruk(m), req(m), ract(m);
    std::vector<double> av(nnz), cv(n), qv(n), lv(n), uv(n), rlv(m), ruv(m);
    for (int k = 0; k < nnz; ++k) au[k] = (flags[k] & IPMF_UNI) ? 1 : 0, av[k] = au[k] ? v0[k] : 0.0;
    for (int j = 0; j < n; ++j) {
        cu[j] = ((flags[oc + j] & IPMF_UNI) && std::isfinite(v0[oc + j])) ? 1 : 0;
        cv[j] = cu[j] ? v0[oc + j] : 0.0;
        const bool qu = (flags[oq + j] & IPMF_UNI) && std::isfinite(v0[oq + j]);
        qk[j] = qu ? (v0[oq + j] == 0.0 ? 0 : 1) : 2;
        qv[j] = qu ? v0[oq + j] : 0.0;
        lk[j] = kind(olb + j), lv[j] = lk[j] == 1 ? v0[olb + j] : 0.0;
        uk[j] = kind(oub + j), uv[j] = uk[j] == 1 ? v0[oub + j] : 0.0;
        nsl[j] = slot[j];
    }
    for (int i = 0; i < m; ++i) {
        rlk[i] = kind(orl + i), rlv[i] = rlk[i] == 1 ? v0[orl + i] : 0.0;
        ruk[i] = kind(oru + i), ruv[i] = ruk[i] == 1 ? v0[oru + i] : 0.0;
        req[i] = (flags[orl + i] & IPMF_EQ) ? 1 : 0;
        ract[i] = active[i];
    }
    double gam = 1.0;
    for (int j = 0; j < n; ++j)
        if (std::isfinite(v0[oc + j])) gam = std::max(gam, std::fabs(v0[oc + j]));
    std::string fac, sol, diag;
    ipm_fac_sol_text(sy, fac, sol);
    for (int r : sy.order) diag += "MD[" + std::to_string(r) + "] = F[" + std::to_string(sy.pos.at({r, r})) + "]; ";
    std::vector<std::string> actr(m);
    for (int i = 0; i < m; ++i) actr[i] = sy.rank[i] >= 0 ? "true" : "false";
    std::string s;
    s += "#define IPM_GAM " + ipm_lit(gam) + "\n#define IPM_MEHROTRA 0\n";
    s += ipm_env_defs();
    s += "#define NC " + std::to_string(n) + "\n#define NR " + std::to_string(m) + "\n#define NZ " +
         std::to_string(std::max(nnz, 1)) + "\n#define NF " + std::to_string(NF) + "\n";
    s += "#define ML_L " + std::to_string(L) + "\n#define ML_QC " + std::to_string(QC) + "\n#define ML_QR " +
         std::to_string(QR) + "\n#define ML_QF " + std::to_string(QF) + "\n#define ML_ZC " + std::to_string(ZC) +
         "\n#define ML_ZR " + std::to_string(ZR) + "\n#define ML_ZT " + std::to_string(ZT) + "\n";
    s += "#define IPM_FACTOR(F, DI, MD) do { " + fac + "} while (0)\n";
    s += "#define IPM_SOLVE(F, DI, R) do { " + sol + "} while (0)\n";
    s += "#define ML_DIAG_COPY(F, MD) do { " + diag + "} while (0)\n";
    s += "#define ML_ACT_ROW(i) " + ipm_chain("i", actr) + "\n";
    s += ipm_table<int>("int", "TCJ", tcj, ipm_fmt_i) + ipm_table<int>("int", "TRI", tri, ipm_fmt_i);
    s += ipm_table<int>("int", "CER", cer, ipm_fmt_i) + ipm_table<int>("int", "CEK", cek, ipm_fmt_i);
    s += ipm_table<int>("int", "REC", rec, ipm_fmt_i) + ipm_table<int>("int", "REK", rek, ipm_fmt_i);
    s += ipm_table<int>("int", "FTJ", ftj, ipm_fmt_i) + ipm_table<int>("int", "FTK1", ftk1, ipm_fmt_i);
    s += ipm_table<int>("int", "FTK2", ftk2, ipm_fmt_i) + ipm_table<int>("int", "FDR", fdr, ipm_fmt_i);
    s += ipm_table<int>("int", "AU", au, ipm_fmt_i) + ipm_table<double>("double", "AV", av, ipm_fmt_d);
    s += ipm_table<int>("int", "CU", cu, ipm_fmt_i) + ipm_table<double>("double", "CV", cv, ipm_fmt_d);
    s += ipm_table<int>("int", "QK", qk, ipm_fmt_i) + ipm_table<double>("double", "QV", qv, ipm_fmt_d);
    s += ipm_table<int>("int", "LK", lk, ipm_fmt_i) + ipm_table<double>("double", "LV", lv, ipm_fmt_d);
    s += ipm_table<int>("int", "UK", uk, ipm_fmt_i) + ipm_table<double>("double", "UV", uv, ipm_fmt_d);
    s += ipm_table<int>("int", "NSL", nsl, ipm_fmt_i);
    s += ipm_table<int>("int", "RLK", rlk, ipm_fmt_i) + ipm_table<double>("double", "RLV", rlv, ipm_fmt_d);
    s += ipm_table<int>("int", "RUK", ruk, ipm_fmt_i) + ipm_table<double>("double", "RUV", ruv, ipm_fmt_d);
    s += ipm_table<int>("int", "REQ", req, ipm_fmt_i) + ipm_table<int>("int", "RACT", ract, ipm_fmt_i);
    return s;
}

// The preamble of the workgroup kernel (jit_ipm_wave.hip.in) for the data flags
static std::string ipm_wave_preamble(int n, int m, int nnz, const int32_t* rp, const int32_t* ci, const int32_t* slot,
                                     const int32_t* flags, const double* v0, int* info, bool* ok, int want_wps = 0) {
    const int oc = nnz, oq = nnz + n, olb = nnz + 2 * n, oub = nnz + 3 * n, orl = nnz + 4 * n, oru = nnz + 4 * n + m;
    auto kind = [&](int e) -> int {
        if (!(flags[e] & IPMF_FIN_ANY)) return 0;
        return ((flags[e] & IPMF_UNI) && (flags[e] & IPMF_FIN_ALL)) ? 1 : 2;
    };
    std::vector<char> active(m);
    for (int i = 0; i < m; ++i) active[i] = (kind(orl + i) != 0 || kind(oru + i) != 0) ? 1 : 0;
    const wave_plan w = wave_build(n, m, nnz, rp, ci, active, want_wps);
    if (ok) *ok = w.ok;
    if (!w.ok) return std::string();
    if (info) {
        info[0] = w.rows;
        info[1] = w.NFL + (int)(w.R.size() * (w.R.size() + 1) / 2);
        info[2] = (int)w.fac_flops;
        info[3] = (int)w.sol_flops;
    }
    std::vector<int> au(nnz), cu(n), qk(n), lk(n), uk(n), nsl(n), rlk(m), ruk(m), req(m), ract(m);
    std::vector<double> av(nnz), cv(n), qv(n), lv(n), uv(n), rlv(m), ruv(m);
    for (int k = 0; k < nnz; ++k) au[k] = (flags[k] & IPMF_UNI) ? 1 : 0, av[k] = au[k] ? v0[k] : 0.0;
    for (int j = 0; j < n; ++j) {
        cu[j] = ((flags[oc + j] & IPMF_UNI) && std::isfinite(v0[oc + j])) ? 1 : 0;
        cv[j] = cu[j] ? v0[oc + j] : 0.0;
        const bool qu = (flags[oq + j] & IPMF_UNI) && std::isfinite(v0[oq + j]);
        qk[j] = qu ? (v0[oq + j] == 0.0 ? 0 : 1) : 2;
        qv[j] = qu ? v0[oq + j] : 0.0;
        lk[j] = kind(olb + j), lv[j] = lk[j] == 1 ? v0[olb + j] : 0.0;
        uk[j] = kind(oub + j), uv[j] = uk[j] == 1 ? v0[oub + j] : 0.0;
        nsl[j] = slot[j];
    }
    for (int i = 0; i < m; ++i) {
        rlk[i] = kind(orl + i), rlv[i] = rlk[i] == 1 ? v0[orl + i] : 0.0;
        ruk[i] = kind(oru + i), ruv[i] = ruk[i] == 1 ? v0[oru + i] : 0.0;
        req[i] = (flags[orl + i] & IPMF_EQ) ? 1 : 0;
        ract[i] = active[i];
    }
    double gam = 1.0;
    for (int j = 0; j < n; ++j)
        if (std::isfinite(v0[oc + j])) gam = std::max(gam, std::fabs(v0[oc + j]));
    std::string fac, sol;
    ipm_fac_sol_text(w.root, fac, sol);
    const int nR = (int)w.R.size();
    std::vector<int> rrow(std::max(nR, 1), 0), lrw(std::max(w.NLR, 1), 0);
    for (int a = 0; a < nR; ++a) rrow[a] = w.R[a];
    for (int u = 0; u < w.NLR; ++u) lrw[u] = w.lrw[u];
    auto I = [](const char* nm, const std::vector<int>& v) { return ipm_table<int>("int", nm, v, ipm_fmt_i); };
    auto D = [](const char* nm, const std::vector<double>& v) { return ipm_table<double>("double", nm, v, ipm_fmt_d); };
    auto nz = [](std::vector<int> v) {
        if (v.empty()) v.push_back(0);
        return v;
    };
    std::string s;
    s += "#define IPM_GAM " + ipm_lit(gam) + "\n";
    s += ipm_env_defs();
    s += "#define NC " + std::to_string(n) + "\n#define NR " + std::to_string(m) + "\n#define NZ " +
         std::to_string(std::max(nnz, 1)) + "\n";
    s += "#define WPS " + std::to_string(w.WPS) + "\n#define WT " + std::to_string(w.WT) + "\n#define W_QC " +
         std::to_string(w.QC) + "\n#define W_QR " + std::to_string(w.QR) + "\n#define W_ZC " + std::to_string(w.ZC) +
         "\n#define W_ZR " + std::to_string(w.ZR) + "\n#define NLR " + std::to_string(w.NLR) + "\n#define NRT " +
         std::to_string(nR) + "\n#define NFL " + std::to_string(w.NFL) + "\n";
    s += "#define ROOT_FACTOR(F, DI, MD) do { " + fac + "} while (0)\n";
    s += "#define ROOT_SOLVE(F, DI, R) do { " + sol + "} while (0)\n";
    s += "#define RLONG(i) RLNG[i]\n";
    s += I("CER", w.cer) + I("CEK", w.cek) + I("CEL", w.cel) + I("REC", w.rec) + I("REK", w.rek);
    s += I("RLNG", w.rlng) + I("LRW", lrw) + I("RROW", rrow) + I("RPOS", w.rpos);
    s += I("EP", w.EP) + I("ER", nz(w.ER)) + I("EDIAG", nz(w.EDIAG)) + I("ECP", w.ECP) + I("ECU", nz(w.ECU)) +
         I("ECF", nz(w.ECF)) + I("ECR", nz(w.ECR)) + I("EUP", w.EUP) + I("EUT", nz(w.EUT)) + I("EUA", nz(w.EUA)) +
         I("EUB", nz(w.EUB));
    s += I("FTP", w.FTP) + I("FTJ", nz(w.FTJ)) + I("FTK1", nz(w.FTK1)) + I("FTK2", nz(w.FTK2));
    s += I("CRP", w.CRP) + I("CRPP", nz(w.CRPP)) + I("CRK1", nz(w.CRK1)) + I("CRK2", nz(w.CRK2));
    s += I("AU", au) + D("AV", av) + I("CU", cu) + D("CV", cv) + I("QK", qk) + D("QV", qv) + I("LK", lk) + D("LV", lv);
    s += I("UK", uk) + D("UV", uv) + I("NSL", nsl) + I("RLK", rlk) + D("RLV", rlv) + I("RUK", ruk) + D("RUV", ruv);
    s += I("REQ", req) + I("RACT", ract);
    return s;
}

#include "solve_blk.inc"

// waves per scenario of the workgroup IPMs (create time, every row active).  Automatic: the
// subtree kernel when the pattern is block-angular and its plan fits one wave (farmer cm = 10,
// config 2).  Multi-wave plans (cm = 64) and the workgroup kernel of 3.9 only with
// PHGPU_IPM_WAVE=1: measured, their PH subproblems jam on warm starts at cm = 64 and leave
// nonants 1e-3..1e-2 off (x̄ 2e-5 against the oracle's 1e-5 bar), and the workgroup kernel is
// slower than the workgroup PDHG on config 2 (DESIGN.md 3.9 / 3.10).  PHGPU_IPM_WAVE=0: none;
// PHGPU_IPM_BLK=0: not the subtree kernel.
static int ipm_wg_bound(int n, int m, int nnz, const int32_t* rp, const int32_t* ci) {
    if (n > 64 * 4 * WAVE_MAX_SLOTS || m > 64 * 4 * WAVE_MAX_SLOTS) return 0;
    const char* we = getenv("PHGPU_IPM_WAVE");
    if (we && atoi(we) == 0) return 0;
    const bool any = we && atoi(we) == 1;
    const char* be = getenv("PHGPU_IPM_BLK");
    if (!(be && atoi(be) == 0)) {
        const int wt = ipm_blk_bound(n, m, nnz, rp, ci);
        if (wt == 64 || (wt > 0 && any)) return wt / 64;
    }
    return any ? ipm_wave_bound(n, m, nnz, rp, ci) : 0;
}

// The whole source of a handle's path-6 module: the path-5 preamble and kernel (the
// fallback) followed by the IPM preamble and kernel; for the workgroup kernel (L >= 64 =
// its threads per scenario) the IPM alone (its fallback is k_solve over the list).  Every
// IPM preamble starts with its #define IPM_GAM line and carries the tuning definitions
// (ipm_env_defs); after it come, once each, the argument blocks (ipm_args.h), the folded PH
// step (one lane / lane groups), the shared defaults and helpers (jit_ipm_common.hip.in,
// all #ifndef: the tuning comes first) and the kernel template, whose first line is its
// "// <file> --" banner (the host emulations and tools cut the source at those two marks).
// Pure host code (no GPU).
static std::string ipm_source_body(int n, int m, int nnz, const int32_t* rp, const int32_t* ci, const int32_t* slot,
                                   const int32_t* kinds, const int32_t* flags, const double* v0, int* info,
                                   int L, const int32_t* ndep);
static std::string ipm_source(int n, int m, int nnz, const int32_t* rp, const int32_t* ci, const int32_t* slot,
                              const int32_t* kinds, const int32_t* flags, const double* v0, int* info /* [4] */,
                              int L = 1, const int32_t* ndep = nullptr) {
    // the statistics layout every path-6 kernel shares with the host (phgpu.hip stats_word):
    // IPM_SC copies of IPM_SS words (the templates' IPM_STAT picks a wave's copy)
    const std::string body = ipm_source_body(n, m, nnz, rp, ci, slot, kinds, flags, v0, info, L, ndep);
    if (body.empty()) return body;
    return "#define IPM_SC " + std::to_string(PHGPU_STATS_COPIES) + "\n#define IPM_SS " +
           std::to_string(PHGPU_STATS_STRIDE) + "\n" + body;
}
static std::string ipm_source_body(int n, int m, int nnz, const int32_t* rp, const int32_t* ci, const int32_t* slot,
                                   const int32_t* kinds, const int32_t* flags, const double* v0, int* info,
                                   int L, const int32_t* ndep) {
    if (L >= 64) {
        // the subtree kernel when the pattern is block-angular, else the workgroup kernel;
        // both with WT = L threads per scenario
        bool ok = false;
        const char* be = getenv("PHGPU_IPM_BLK");
        if (!(be && atoi(be) == 0)) {
            const std::string pre = ipm_blk_preamble(n, m, nnz, rp, ci, slot, flags, v0, info, L, &ok);
            if (ok) return pre + kIpmArgs + kIpmCommon + kIpmWgCommon + kIpmBlkKernel;
        }
        const std::string pre = ipm_wave_preamble(n, m, nnz, rp, ci, slot, flags, v0, info, &ok, L / 64);
        return ok ? pre + kIpmArgs + kIpmCommon + kIpmWgCommon + kIpmWaveKernel : std::string();
    }
    std::vector<int32_t> rpv(rp, rp + m + 1), civ(ci, ci + std::max(nnz, 1)), sv(slot, slot + n), kv(kinds, kinds + n + m);
    if (!nnz) civ.assign(1, 0);
    std::string src = jit_source(jit_preamble(n, m, nnz, rpv, civ, sv, kv, 1));
    src += "\n#undef NC\n#undef NR\n#undef NZ\n";
    src += L <= 1 ? ipm_preamble(n, m, nnz, rp, ci, slot, flags, v0, 1, info)
                  : ipm_ml_preamble(n, m, nnz, rp, ci, slot, flags, v0, L, info);
    src += ipm_nonant_defs(n, slot, ndep);
    src += kIpmArgs;
    src += kPhStep;
    src += kIpmCommon;
    src += L <= 1 ? kIpmKernel : kIpmMlKernel;
    return src;
}

// path-5 kinds from the path-6 flags (same meaning as k_jit_kinds)
static void ipm_kinds_from_flags(int n, int m, int nnz, const int32_t* flags, const double* v0, std::vector<int32_t>& kinds) {
    const int oq = nnz + n, olb = nnz + 2 * n, oub = nnz + 3 * n, orl = nnz + 4 * n, oru = nnz + 4 * n + m;
    kinds.assign((size_t)(n + m), 0);
    for (int j = 0; j < n; ++j) {
        int b = 0;
        if (flags[olb + j] & IPMF_FIN_ANY) b |= 1;
        if (flags[oub + j] & IPMF_FIN_ANY) b |= 2;
        if (!((flags[oq + j] & IPMF_UNI) && v0[oq + j] == 0.0)) b |= 4;
        kinds[j] = b;
    }
    for (int i = 0; i < m; ++i) {
        int b = 0;
        if (flags[orl + i] & IPMF_FIN_ANY) b |= 1;
        if (flags[oru + i] & IPMF_FIN_ANY) b |= 2;
        if (!(flags[orl + i] & IPMF_EQ)) b |= 4;
        kinds[n + i] = b;
    }
}

// C-ABI: the generated path-6 source for a pattern and data flags (tests / tools; no GPU)
extern "C" int phgpu_ipm_source(int32_t n, int32_t m, int32_t nnz, const int32_t* row_ptr, const int32_t* col_idx,
                                const int32_t* nonant_slot, const int32_t* flags, const double* v0, int32_t lanes,
                                char* buf, size_t len, int32_t* info) {
    if (n <= 0 || m < 1 || nnz < 0 || !row_ptr || (nnz && !col_idx) || !nonant_slot || !flags || !v0)
        return set_err(-1, "phgpu_ipm_source: bad arguments");
    std::vector<int32_t> kinds;
    ipm_kinds_from_flags(n, m, nnz, flags, v0, kinds);
    int inf[4] = {0, 0, 0, 0};
    if (!(lanes == 1 || lanes == 2 || lanes == 4 || lanes == 8 || lanes == 16 || lanes == 64 || lanes == 128 ||
          lanes == 192 || lanes == 256))
        return set_err(-1, "phgpu_ipm_source: lanes must be 1, 2, 4, 8, 16 or 64 / 128 / 192 / 256 (workgroup kernels)");
    const std::string src = ipm_source(n, m, nnz, row_ptr, col_idx, nonant_slot, kinds.data(), flags, v0, inf, lanes);
    if (src.empty()) return set_err(-1, "phgpu_ipm_source: the workgroup plan does not fit this pattern");
    if (info)
        for (int k = 0; k < 4; ++k) info[k] = inf[k];
    if (buf && len > src.size()) memcpy(buf, src.c_str(), src.size() + 1);
    return (int)std::min<size_t>(src.size() + 1, (size_t)INT32_MAX);
}

// Lanes per scenario of the IPM kernel: lane groups while one lane per scenario would leave
// most SIMDs idle (the per-rank share of a strong-scaling run; a launch is latency-bound,
// one scenario's iteration chain).  Measured with the load / iterate / store kernel
// (profiles/r03/p/, farmer): 8,192 scenarios L = 8 0.072 ms per solve (L = 4 0.081, L = 16
// 0.104); 16,384 L = 4 0.094 (L = 1 0.102, L = 8 0.112); 32,768 L = 1 0.103 (L = 4 0.165);
// L = 2 modules spill.  A pattern whose one-lane module spills more than IPM_SPILL_MAX takes
// L = 4 above 8,192 (aircond 65,536: L = 4 0.355 ms, L = 8 0.415, L = 16 0.677 in round 3;
// round 5: its one-lane module's 524 B of spills cost less than lane groups, 0.315 vs 0.426
// ms).  PHGPU_IPM_LANES = 1 | 2 | 4 | 8 | 16 pins it.
static int ipm_lanes(const phgpu_state* h) {
    if (!ipm_small(h)) return 64 * h->ipm_wave;  // the workgroup kernel (threads per scenario)
    const char* env = getenv("PHGPU_IPM_LANES");
    if (env) {
        const int v = atoi(env);
        if (v == 1 || v == 2 || v == 4 || v == 8 || v == 16) return v;
    }
    if (h->S <= IPM_ML_MAX_S) return IPM_ML_LANES;      // <= 8,192: 8 lanes
    if (h->S <= 2 * IPM_ML_MAX_S || h->ipm_spill1) return 4;  // <= 16,384, or one lane spills
    return 1;
}

// Compile a path-6 source and load it: the IPM kernel `fname` (L lanes / threads per
// scenario) with its occupancy and resources and, when want_pdhg, the module's path-5 kernel
// (the fallback).  *out is the new module (key = src); mr / nf / flops are the caller's.
static int ipm_module_load(const std::string& src, int L, const char* fname, bool want_pdhg, const char* what,
                           ipm_module** out) {
    std::vector<char> code;
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = jit_compile(src, code, L == 1);
    if (rc) return rc;
    ipm_module* im = new ipm_module();
    im->compile_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    im->key = src;
    im->L = L;
    hipError_t e = hipModuleLoadData(&im->mod, code.data());
    if (e == hipSuccess) e = hipModuleGetFunction(&im->fn_ipm, im->mod, fname);
    if (e == hipSuccess)
        e = hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&im->per_cu_ipm, im->fn_ipm, L < 64 ? 256 : L, 0);
    if (want_pdhg) {
        if (e == hipSuccess) e = hipModuleGetFunction(&im->fn_pdhg, im->mod, "k_solve_jit");
        if (e == hipSuccess) e = hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&im->per_cu_pdhg, im->fn_pdhg, 256, 0);
    }
    if (e == hipSuccess) e = hipFuncGetAttribute(&im->private_bytes, HIP_FUNC_ATTRIBUTE_LOCAL_SIZE_BYTES, im->fn_ipm);
    if (e == hipSuccess) e = hipFuncGetAttribute(&im->vgprs, HIP_FUNC_ATTRIBUTE_NUM_REGS, im->fn_ipm);
    if (e != hipSuccess) {
        module_release(im);
        return set_err(-2, "loading the %s module failed: %s", what, hipGetErrorString(e));
    }
    *out = im;
    return 0;
}

// flags (one synchronisation), then the cached module or a new one
static int ipm_prepare(phgpu_state* h, hipStream_t st) {
    if (h->ipm && h->ipm_flags_valid && h->ipm->L == ipm_lanes(h)) return 0;
    struct tuning_scope {  // the handle's phgpu_set_ipm_tuning definitions, for ipm_source
        explicit tuning_scope(phgpu_state* hh) {
            const std::string& t = owner_of(hh)->ipm_tuning;
            g_ipm_tuning = t.empty() ? nullptr : &t;
        }
        ~tuning_scope() { g_ipm_tuning = nullptr; }
    } tuning(h);
    const int n = h->n, m = h->m, nnz = h->nnz;
    const int E = nnz + 4 * n + 2 * m;
    // temporary device buffers of the flag pass, freed on every exit path
    dev_tmp<int32_t> df;
    dev_tmp<double> dv;
    HIPCHK(df.alloc((size_t)E));
    HIPCHK(dv.alloc((size_t)E));
    hipLaunchKernelGGL(k_ipm_flags, dim3((unsigned)E), dim3(256), 0, st, *h, df.p, dv.p);
    std::vector<int32_t> flags((size_t)E), slot((size_t)n), rp((size_t)m + 1), ci((size_t)std::max(nnz, 1));
    std::vector<double> v0((size_t)E);
    HIPCHK(hipMemcpyAsync(flags.data(), df.p, (size_t)E * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(v0.data(), dv.p, (size_t)E * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(slot.data(), h->nonant_slot, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(rp.data(), h->row_ptr, (size_t)(m + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (nnz) HIPCHK(hipMemcpyAsync(ci.data(), h->col_idx, (size_t)nnz * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    std::vector<int32_t> ndep((size_t)std::max(h->nn, 1), 0);
    if (h->nn)
        HIPCHK(hipMemcpyAsync(ndep.data(), h->nonant_depth, (size_t)h->nn * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    std::vector<int32_t> kinds;
    ipm_kinds_from_flags(n, m, nnz, flags.data(), v0.data(), kinds);
    int inf[4] = {0, 0, 0, 0};
    const int L = ipm_lanes(h);
    std::string src = ipm_source(n, m, nnz, rp.data(), ci.data(), slot.data(), kinds.data(), flags.data(),
                                 v0.data(), inf, L, ndep.data());
    if (src.empty()) return set_err(-2, "path 6: the workgroup plan does not fit this data (flags)");
    if (L == 1 && h->ipm_lds == 1) src = "#define IPM_LDS_ISL 1\n" + src;
    if (h->ipm && h->ipm->key == src) {
        h->ipm_flags_valid = 1;
        return 0;
    }
    const bool blk = L >= 64 && src.find("k_solve_ipm_blk") != std::string::npos;
    const char* fname = L == 1 ? "k_solve_ipm" : (L < 64 ? "k_solve_ipm_ml" : (blk ? "k_solve_ipm_blk" : "k_solve_ipm_wave"));
    ipm_module* im = nullptr;
    // (the workgroup kernels' fallback is k_solve of the library, not the module's path 5)
    const int rc = ipm_module_load(src, L, fname, L < 64, "path-6", &im);
    if (rc) return rc;
    im->blk = blk;
    im->mr = inf[0];
    im->nf = inf[1];
    im->fac_flops = inf[2];
    im->sol_flops = inf[3];
    module_release(h->ipm);
    h->ipm = im;
    h->ipm_flags_valid = 1;
    // a one-lane kernel that spills: its slack reciprocals (2 (n + m) doubles per lane, written
    // once per IPM iteration and read several times) in LDS instead, kept when that module
    // spills less.  Config 4 (aircond 32x32x64, n = 20, m = 8): 516 -> 132 B of scratch per
    // lane, 0.372 -> 0.292-0.297 ms per PH iteration (profiles/r06/hh/).  114 KB of LDS per
    // workgroup, within the one workgroup per CU a 512-register module has anyway.
    // PHGPU_IPM_LDS=0 turns it off.
    const char* le = getenv("PHGPU_IPM_LDS");
    if (L == 1 && h->ipm_lds == 0 && im->private_bytes > 0 && (2 * n + 2 * m) * 256 * 8 <= 150 * 1024 &&
        !(le && atoi(le) == 0)) {
        h->ipm_lds = 1;
        h->ipm_lds_ref = (int)im->private_bytes;
        h->ipm_flags_valid = 0;
        return ipm_prepare(h, st);
    }
    if (L == 1 && h->ipm_lds == 1 && (int)im->private_bytes >= h->ipm_lds_ref) {
        h->ipm_lds = -1;  // no better: back to the register-only module
        h->ipm_flags_valid = 0;
        return ipm_prepare(h, st);
    }
    // a one-lane kernel that spills: lane groups of 4 instead (aircond, config 4: 0.355 ms
    // per solve at 65,536 scenarios vs 0.622 on the register PDHG, profiles/r03/r/; the
    // queue-based lane-group kernel of before was slower, 0.86 ms, profiles/r03/j/)
    if (L == 1 && im->private_bytes > ipm_spill_max() && !getenv("PHGPU_IPM_LANES")) {
        h->ipm_spill1 = 1;
        return ipm_prepare(h, st);
    }
    return 0;
}

// the PDHG fallback over a path-6 launch's list (path 5 of the same module): a persistent
// grid that drains the device-side count
static int ipm_fallback_launch(phgpu_state* h, ipm_module* im, const solve_params& P, double* x, double* y,
                               double* obj, double* bound, int32_t* status, int32_t* iters, int32_t* qhead,
                               int32_t* fail_n, unsigned long long* stats, hipStream_t st) {
    jit_params b{};
    b.A = h->Ah_csr; b.c = h->c; b.q = h->q; b.Dc = h->Dc; b.lbh = h->lbh; b.ubh = h->ubh; b.Dr = h->Dr;
    b.rlh = h->rlh; b.ruh = h->ruh; b.rl = h->rl; b.ru = h->ru; b.objc = h->objc; b.normA = h->normA;
    b.W = h->W; b.rho = h->rho; b.xbar = h->xbar;
    b.omega_in = h->omega_w; b.x_in = h->xw; b.y_in = h->yw;  // what the IPM handed over
    b.omega_out = h->omega_w; b.x_w = h->xw; b.y_w = h->yw;
    b.xout = x; b.yout = y; b.obj = obj; b.bound = bound;
    b.status = status; b.iters = iters; b.qhead = qhead;
    b.list = h->ipm_list; b.list_n = fail_n; b.stats = stats;
    b.S = h->S;
    b.first_dyn = 0;
    b.W_on = h->W_on; b.prox_on = h->prox_on;
    b.eps_rel = P.eps_rel; b.eps_abs = P.eps_abs; b.bsuff = P.bsuff; b.bnec = P.bnec; b.bart = P.bart;
    b.eta_frac = P.eta_frac; b.omega0 = P.omega0; b.wmin = P.wmin; b.wmax = P.wmax; b.eps_inf = P.eps_inf;
    b.max_iter = P.max_iter; b.check_every = P.check_every; b.restart_every = P.restart_every; b.warm = 1;
    b.keep_omega = P.keep_omega; b.infeas_start = P.infeas_start;
    void* bargs[] = {&b};
    // a small persistent grid: the list is usually empty (this launch then only costs its
    // dispatch, which grows with the grid of a kernel with a private segment), and short
    const int64_t per = (int64_t)(im->per_cu_pdhg < 1 ? 1 : im->per_cu_pdhg) * h->num_cus;
    int64_t fb_max = IPM_FALLBACK_BLOCKS;
    if (const char* e = getenv("PHGPU_IPM_FB_BLOCKS")) fb_max = std::max(1, atoi(e));  // (experiments)
    const unsigned fblk = (unsigned)std::min<int64_t>(std::min<int64_t>(per, fb_max),
                                                      std::max<int64_t>(1, (h->S + 255) / 256));
    HIPCHK(hipModuleLaunchKernel(im->fn_pdhg, fblk, 1, 1, 256, 1, 1, 0, st, bargs, nullptr));
    return 0;
}

// The core of a path-6 launch's argument block (and prof) for the solve of parity par, the
// one place that reads PHGPU_IPM_EPS / PHGPU_IPM_MAXIT and does the parity arithmetic: this
// solve's counters {fallback count, fallback queue head, spare} and statistics are those of
// its parity, zeroed by the previous path-6 launch (the other parity) or at create; the
// kernel zeroes the other parity's for the next.  Sets h->last_stats.
static void ipm_fill_args(phgpu_state* h, const solve_params& P, int par, double* x, double* y, double* obj,
                          double* bound, int32_t* status, int32_t* iters, ipm_step_params& a) {
    a.A = h->A; a.c = h->c; a.q = h->q; a.lb = h->lb; a.ub = h->ub; a.rl = h->rl; a.ru = h->ru; a.objc = h->objc;
    a.lbh = h->lbh; a.ubh = h->ubh; a.Dc = h->Dc; a.Dr = h->Dr;
    a.W = h->W; a.rho = h->rho; a.xbar = h->xbar;
    a.omega_in = h->omega;
    a.omega_out = h->omega_w; a.x_w = h->xw; a.y_w = h->yw;
    a.xout = x; a.yout = y; a.obj = obj; a.bound = bound;
    a.status = status; a.iters = iters;
    a.fail_list = h->ipm_list; a.fail_n = h->ipm_cnt + 3 * par;
    a.zero3 = h->ipm_cnt + 3 * (1 - par);
    a.stats = h->ipm_stats + PHGPU_STATS_WORDS * par; a.stats_zero = h->ipm_stats + PHGPU_STATS_WORDS * (1 - par);
    a.prof = h->ipm_prof;  // IPM_PROF modules only (phgpu_ipm_prof), null unless PHGPU_IPM_PROF
    h->last_stats = a.stats;  // phgpu_solve_stats copies these
    a.S = h->S;
    a.W_on = h->W_on; a.prox_on = h->prox_on;
    a.eps_rel = P.eps_rel; a.eps_abs = P.eps_abs;
    const char* et = getenv("PHGPU_IPM_EPS");
    a.eps_tight = (et && atof(et) > 0.0) ? atof(et) : IPM_EPS_TIGHT;
    a.x_in = P.warm ? h->x : nullptr;  // a failed scenario's PDHG start without a finite iterate
    a.y_in = P.warm ? h->y : nullptr;
    const char* env = getenv("PHGPU_IPM_MAXIT");
    a.max_ipm = (env && atoi(env) >= 0) ? atoi(env) : IPM_MAXIT;
}

static int ipm_launch(phgpu_state* h, const solve_params& P, double* x, double* y, double* obj, double* bound,
                      int32_t* status, int32_t* iters, hipStream_t st) {
    ipm_module* im = h->ipm;
    const int par = h->ipm_parity;
    h->ipm_parity ^= 1;
    // every path-6 launch is filled as this one block: the one-lane kernel reads all of it
    // (and ignores the loop's tail), the workgroup kernels take its core layer, the lane-group
    // kernel a copy of its step layer's parts
    ipm_params a{};
    ipm_fill_args(h, P, par, x, y, obj, bound, status, iters, a);
    int32_t* qhead = a.fail_n + 1;  // the fallback's queue head
    if (im->L >= 64) {
        // the workgroup kernels (one scenario per workgroup of L threads) take the core layer
        h->xp_C[h->wq] = 0;
        ipmw_params& core = a;
        void* args[] = {&core};
        HIPCHK(hipModuleLaunchKernel(im->fn_ipm, (unsigned)h->S, 1, 1, (unsigned)im->L, 1, 1, 0, st, args, nullptr));
        // the fallback: the global-memory PDHG (path 1) over the list, warm-started from the
        // IPM's hand-over (x_w / y_w / omega_w), adding its scenarios' statistics
        pdhg_view v = *h;
        v.x = h->xw;
        v.y = h->yw;
        v.omega = h->omega_w;
        solve_params Q = P;
        Q.warm = 1;
        hipLaunchKernelGGL(k_solve, dim3((unsigned)((h->S + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, v, Q, x, y, obj,
                           bound, status, iters,
                           (const int32_t*)h->ipm_list, (const int32_t*)a.fail_n, a.stats);
        HIPCHK(hipGetLastError());
        return 0;
    }
    // x̄ partials from the epilogue (DESIGN.md 3.8): when every wave of local scenarios is
    // on one node per nonant depth (xbar_mixed == 0, known after the first phgpu_ph_reduce)
    // and a chunk is at most a wave; PHGPU_XP=0 turns them off (A/B experiments)
    const int C = im->L == 1 ? WAVE : 256 / im->L;
    const char* xe = getenv("PHGPU_XP");
    // (variable probabilities: the epilogue weights by node, so no partials there)
    const bool xp_on = h->xbar_mixed == 0 && h->nn > 0 && h->nn <= XL_NN_MAX && C <= WAVE && !(xe && atoi(xe) == 0) &&
                       !h->pvar;
    const int wq = h->wq;
    a.xp = xp_on ? h->xp[wq] : nullptr;
    a.xp_node = h->xp_node[wq];
    a.xp_dirty = h->xp_dirty[wq];
    a.pcoef = h->pcoef;
    a.node_of = h->node_of;
    if (h->fuse_now) {  // the pending one-rank PH step, folded into this launch (jit_ph_step.hip.in)
        const int r = h->wslot;
        const phgpu_state::ph_pending& q = h->pend;
        a.ph.on = 1;
        a.ph.update_W = q.update_W;
        a.ph.xprev = q.x;
        a.ph.xp = h->xp[r];
        a.ph.xp_dirty = h->xp_dirty[r];
        a.ph.xp_n = h->xp_n[r];
        a.ph.C = h->xp_C[r];
        a.ph.node_buf = q.node_buf;
        a.ph.nb_idx = h->nb_idx;
        a.ph.nb_half = (long long)h->num_nodes * h->nlen_max;
        a.ph.W = q.W;
        a.ph.xbar = q.xbar;
        a.ph.rho = q.rho;
        a.ph.conv = q.conv;
        a.ph.stats_dst = (long long*)q.stats;
        a.ph.scale = 1.0 / ((double)h->S * (double)h->nn);
        a.ph.cpart = h->cpart_blk;
        a.ph.cnt = h->blk_cnt;
        h->fuse_now = 0;
        h->pend.active = 0;
    }
    h->xp_C[wq] = xp_on ? C : 0;
    h->xp_x[wq] = x;
    h->xp_n[wq] = (h->S + C - 1) / C;
    // one lane: a scenario per lane; lane groups: one scenario per group, S * L lanes
    ipml_params ml{};
    static_cast<ipm_params_ptrs&>(ml) = a;
    static_cast<ipm_params_ctl&>(ml) = a;
    static_cast<ipm_params_xp&>(ml) = a;
    void* args[] = {im->L == 1 ? (void*)&a : (void*)&ml};
    const unsigned nblk = (unsigned)((h->S * im->L + 255) / 256);
    HIPCHK(hipModuleLaunchKernel(im->fn_ipm, nblk, 1, 1, 256, 1, 1, 0, st, args, nullptr));
    return ipm_fallback_launch(h, im, P, x, y, obj, bound, status, iters, qhead, a.fail_n, a.stats, st);
}

// ---------------------------------------------------------------- the PH loop (IPM_LOOP)
// The IPM_LOOP build of the handle's one-lane module (jit_ipm.hip.in, k_ph_loop_ipm), made on
// first use from the regular module's source.
static int ipm_loop_prepare(phgpu_state* h) {
    const std::string src = "#define IPM_LOOP 1\n" + h->ipm->key;
    if (h->ipm_loop && h->ipm_loop->key == src) return 0;
    ipm_module* im = nullptr;
    const int rc = ipm_module_load(src, 1, "k_ph_loop_ipm", true, "PH-loop", &im);
    if (rc) return rc;
    im->mr = h->ipm->mr;
    im->nf = h->ipm->nf;
    im->fac_flops = h->ipm->fac_flops;
    im->sol_flops = h->ipm->sol_flops;
    module_release(h->ipm_loop);
    h->ipm_loop = im;
    return 0;
}

// Is the handle's state one phgpu_ph_loop runs (include/phgpu.h)?  0 yes, else a reason.
static int ph_loop_eligible(phgpu_state* h) {
    if (h->shared) return 1;
    if (!(h->nn > 0 && 2 * h->nn + 1 <= 16)) return 2;
    if (!h->nb_idx || !h->xbar_single || h->xbar_mixed != 0) return 3;  // two-stage, x̄ known after one reduce
    if (h->pvar) return 4;
    if (!h->W || !h->rho || !h->xbar || !h->prox_on) return 5;
    if (!ipm_eligible(h) || h->ipm_off || ipm_lanes(h) != 1) return 6;
    return 0;
}

// Interior-point tuning of one handle (include/phgpu.h): "IPM_NAME=number;..." definitions
// for the modules this handle generates next (a model's measured constants, e.g. the aircond
// example's IPM_TUNING); only IPM_ names and numeric values are accepted.
extern "C" int phgpu_set_ipm_tuning(phgpu_handle h, const char* defs) {
    if (!h) return set_err(-1, "null handle");
    std::vector<std::pair<std::string, std::string>> kv;
    if (defs) ipm_parse_defs(std::string(defs), kv);
    std::string norm;
    for (const auto& p : kv) {
        if (p.first.compare(0, 4, "IPM_") != 0) return set_err(-1, "phgpu_set_ipm_tuning: %s is not an IPM_ constant", p.first.c_str());
        for (char ch : p.first)
            if (!(std::isalnum((unsigned char)ch) || ch == '_')) return set_err(-1, "phgpu_set_ipm_tuning: bad name %s", p.first.c_str());
        char* end = nullptr;
        (void)strtod(p.second.c_str(), &end);
        if (p.second.empty() || !end || *end != '\0')
            return set_err(-1, "phgpu_set_ipm_tuning: %s=%s is not a number", p.first.c_str(), p.second.c_str());
        norm += p.first + "=" + p.second + ";";
    }
    if (h->ipm) return set_err(-1, "phgpu_set_ipm_tuning: the interior-point module is already built (call it before the first solve)");
    owner_of(h)->ipm_tuning = norm;
    return 0;
}
