// tests/hostsim/sim_fol_reduce_dd.cpp -- the settle tier of the reduction kinds on the CPU, one lane:
// ValInterp<dd, 3, kFolMaxD, dd> (pdeval_point.h) and red_point_dd (pdeval_fol_reduce.h) as a stand-alone
// program.  Reads int32 {n, m, min_points, n_words}, double {omega2, tau, grid[8]}, int64 offsets[n + 1],
// int32 ops[n_words]; prints per row "kind n_finite bad[3] qmax[3]", then per sample point "fin bad[3]
// X[3] as hi lo, S[3]" (doubles in hexadecimal).  Test infrastructure only (test_fol_reduce_dd_host.py).
#include <cstdio>
#include <vector>
#include "../../include/pdeval.h"
#include "../../pde-engine_amd/csrc/pdeval_point.h"
#include "../../pde-engine_amd/csrc/pdeval_fol_reduce.h"
using namespace pd;

int main(int argc, char** argv) {
    FILE* f = argc == 2 ? fopen(argv[1], "rb") : nullptr;
    int32_t h[4];
    double prm[10];
    if (!f || fread(h, sizeof h, 1, f) != 1 || fread(prm, sizeof prm, 1, f) != 1 || h[0] < 0 || h[1] < 1 || h[3] < 1) return 2;
    const int n = h[0], mm = h[1] * h[1];
    std::vector<int64_t> off((size_t)n + 1);
    std::vector<int32_t> ops((size_t)h[3]);
    if (fread(off.data(), 8, off.size(), f) != off.size() || fread(ops.data(), 4, ops.size(), f) != ops.size()) return 2;
    fclose(f);
    using VI = ValInterp<dd, 3, kFolMaxD, dd>;
    using STK = PrivVStack<dd, nc(3), kFolMaxD - 1>;
    const FolGrid g = fol_grid(prm + 2, h[1]);
    for (int row = 0; row < n; ++row) {
        const FolProg pr = fol_program(ops.data(), (int64_t)ops.size(), off.data(), n, nullptr, row);
        std::vector<RedPointDD> pts((size_t)mm, RedPointDD{});
        bool ok = pr.ok;
        for (int p = 0; p < mm && ok; ++p) {
            double x, y;
            fol_point_xy(g, p, x, y);
            STK stk;
            VI::J u;
            ok = VI::run<STK, false>(pr.words, 1, pr.len, dd_from(x), dd_from(y), u, stk, PrmTab<dd>{}) == RUN_OK;
            if (ok) pts[(size_t)p] = red_point_dd(u.c, x, prm[0], prm[1]);
        }
        if (!ok) pts.assign((size_t)mm, RedPointDD{});   // (a row that does not run counts nothing)
        RedCount c{0, {0, 0, 0}};
        double q[3] = {0.0, 0.0, 0.0};
        for (const RedPointDD& t : pts)
            for (int k = 0; k < 3; ++k) {
                c.n_fin += k == 0 && t.fin;
                c.bad[k] += t.bad[k];
                if (t.fin) q[k] = fmax(q[k], red_q(t, k));
            }
        printf("%d %d %d %d %d %a %a %a\n", red_kind_of(c, h[2]), c.n_fin, c.bad[0], c.bad[1], c.bad[2], q[0], q[1], q[2]);
        for (const RedPointDD& t : pts)
            printf("%d %d %d %d %a %a %a %a %a %a %a %a %a\n", t.fin, t.bad[0], t.bad[1], t.bad[2], t.X[0].hi, t.X[0].lo,
                   t.X[1].hi, t.X[1].lo, t.X[2].hi, t.X[2].lo, t.S[0], t.S[1], t.S[2]);
    }
    return 0;
}
