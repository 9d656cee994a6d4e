// The master LP of the L-shaped method on the host: csrc/ph_lshaped.inc's ls_master_core compiled
// for one thread (LS_HOST), behind a C entry that tests/test_lshaped_host.py loads with ctypes and
// compares with HiGHS.  Buffers are heap blocks of the exact size, so the same file, built as a
// stand-alone program with a sanitizer, sees every overrun (define LS_HOST_MAIN for its main).
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "phgpu.h"
#define LS_HOST
#define WAVE 64
#include "ph_lshaped.inc"

extern "C" int ls_host_master(int nn, int G, int max_cuts, int K, const int32_t* group, const double* a,
                              const double* b, int n_rows, const double* R, const double* rl, const double* ru,
                              const double* xlb, const double* xub, const double* etalb, const double* x0, double eps,
                              double* z, double* info) {
    ls_store L;
    memset(&L, 0, sizeof(L));
    L.G = G; L.nn = nn; L.N = nn + G; L.ld = (nn + G) | 1; L.max_cuts = max_cuts; L.n_rows = n_rows;
    std::vector<int32_t> eq;
    for (int r = 0; r < n_rows; ++r) if (rl[r] == ru[r]) eq.push_back(r);
    L.ne = (int)eq.size();
    L.NI = 2 * nn + G + 2 * n_rows + max_cuts;
    std::vector<double> at((size_t)nn * max_cuts, 0.0), cb(max_cuts, 0.0);
    std::vector<int32_t> cg(max_cuts, 0);
    for (int c = 0; c < K; ++c) {
        for (int k = 0; k < nn; ++k) at[(size_t)k * max_cuts + c] = a[(size_t)c * nn + k];
        cb[c] = b[c]; cg[c] = group[c];
    }
    int32_t nc = K;
    L.cut_a = at.data(); L.cut_b = cb.data(); L.cut_g = cg.data(); L.ncuts = &nc;
    L.R = (double*)R; L.rl = (double*)rl; L.ru = (double*)ru; L.eq = eq.data();
    L.xlb = (double*)xlb; L.xub = (double*)xub; L.etalb = (double*)etalb;
    // exact-size heap buffers so that a sanitizer sees every overrun
    std::vector<double*> bufs;
    auto mk = [&](size_t n) { double* p = (double*)malloc((n ? n : 1) * sizeof(double)); bufs.push_back(p); return p; };
    L.s = mk(L.NI); L.lam = mk(L.NI); L.rp = mk(L.NI); L.ds = mk(L.NI); L.dl = mk(L.NI); L.t = mk(L.NI); L.w = mk(L.NI);
    L.V = mk((size_t)L.N * (L.ne ? L.ne : 1));
    double* shm = mk(ls_shared_doubles(L.N, L.ld, L.ne));
    ls_shared sh;
    ls_carve(shm, L.N, L.ld, L.ne, sh);
    ls_master_core(L, sh, x0, 1, eps, 1e-8, LS_ITER_CAP, info);
    for (int j = 0; j < L.N; ++j) z[j] = sh.z[j];
    for (double* p : bufs) free(p);
    return 0;
}

#ifdef LS_HOST_MAIN
#include <stdio.h>
int main() {
    // nn = 3, G = 2, an equality row, a ranged row, a free column, 7 cuts in a store of 7
    const int nn = 3, G = 2, K = 7, mc = 7, nr = 2;
    int32_t grp[K] = {0, 1, 0, 1, 0, 1, 0};
    double a[K * nn], b[K];
    unsigned s = 12345;
    auto rnd = [&] { s = s * 1103515245u + 12345u; return ((s >> 8) & 0xffff) / 65536.0 * 2.0 - 1.0; };
    for (int i = 0; i < K * nn; ++i) a[i] = rnd();
    for (int i = 0; i < K; ++i) b[i] = 5.0 * rnd();
    double R[nr * nn] = {1, 1, 1, 1, -1, 0}, rl[nr] = {7, -2}, ru[nr] = {7, 3};
    double xlb[nn] = {0, -INFINITY, 0}, xub[nn] = {10, INFINITY, 10}, etalb[G] = {-100, -100}, x0[nn] = {0, 0, 0};
    double z[nn + G], info[6];
    ls_host_master(nn, G, mc, K, grp, a, b, nr, R, rl, ru, xlb, xub, etalb, x0, 1e-9, z, info);
    printf("objective %.10f status %.0f iterations %.0f\n", info[0], info[1], info[2]);
    if (info[1] != 0) return 1;
    double R2[nr * nn] = {1, 1, 1, 1, 1, 1}, rl2[nr] = {-INFINITY, 2}, ru2[nr] = {1, INFINITY};
    ls_host_master(nn, G, mc, K, grp, a, b, nr, R2, rl2, ru2, xlb, xub, etalb, x0, 1e-9, z, info);
    printf("contradictory rows: status %.0f iterations %.0f\n", info[1], info[2]);
    return info[1] == 2 ? 0 : 1;
}
#endif
