// tests/hostsim/sim_fol_reduce.cpp -- the per-point and per-row rule of the reduction kinds
// (pdeval_fol_reduce.h: red_point, red_q, red_coefs, red_kind_of) built for the CPU as a stand-alone
// program.  Reads one binary file -- int32 {rows, mm, min_points, pad}, double {omega2, tau}, then
// rho[mm] and the order-3 jets [rows][mm][10] -- and prints per row "kind n_finite bad_LA bad_LB
// bad_W" and the three row maxima of |X| / S_X as hexadecimal doubles, then per point kappa and G.
// Test infrastructure only (tests/test_fol_reduce_host.py); the product is built by hipcc for gfx950.
#include <cstdio>
#include <vector>
#include "../../include/pdeval.h"
#include "../../pde-engine_amd/csrc/pdeval_fol_reduce.h"
using namespace pd;

int main(int argc, char** argv) {
    FILE* f = argc == 2 ? fopen(argv[1], "rb") : nullptr;
    int32_t h[4];
    double prm[2];
    if (!f || fread(h, sizeof h, 1, f) != 1 || fread(prm, sizeof prm, 1, f) != 1 || h[0] < 0 || h[1] < 1) return 2;
    const int rows = h[0], mm = h[1];
    std::vector<double> x((size_t)mm), c((size_t)rows * mm * 10);
    if (fread(x.data(), sizeof(double), x.size(), f) != x.size()) return 2;
    if (!c.empty() && fread(c.data(), sizeof(double), c.size(), f) != c.size()) return 2;
    fclose(f);
    for (int r = 0; r < rows; ++r) {
        RedCount n{0, {0, 0, 0}};
        double q[3] = {0.0, 0.0, 0.0};
        std::vector<double> kg((size_t)2 * mm);
        for (int p = 0; p < mm; ++p) {
            const RedPoint t = red_point(&c[((size_t)r * mm + p) * 10], x[(size_t)p], prm[0], prm[1]);
            n.n_fin += t.fin;
            for (int k = 0; k < 3; ++k) {
                n.bad[k] += t.bad[k];
                if (t.fin) q[k] = fmax(q[k], red_q(t, k));
            }
            red_coefs(t, kg[(size_t)p], kg[(size_t)mm + p]);
        }
        printf("%d %d %d %d %d %a %a %a\n", red_kind_of(n, h[2]), n.n_fin, n.bad[0], n.bad[1], n.bad[2], q[0], q[1], q[2]);
        for (double v : kg) printf("%a ", v);
        printf("\n");
    }
    return 0;
}
