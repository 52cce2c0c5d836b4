// tests/hostsim/sim_fol_reduce_cplx.cpp -- red_point_cplx (pdeval_fol_reduce.h) built for the CPU as a stand-alone
// program.  Reads int32 {rows, mm}, double {omega2, tau}, rho[mm], the order-3 complex jets [rows][mm][10] as (re, im)
// pairs; prints per point "fin bad_LA bad_LB bad_W".  Test infrastructure only (tests/test_fol_reduce_cplx_host.py).
#include <cstdio>
#include <vector>
#include "../../include/pdeval.h"
#include "../../pde-engine_amd/csrc/pdeval_fol_reduce.h"
using namespace pd;

int main(int argc, char** argv) {
    FILE* f = argc == 2 ? fopen(argv[1], "rb") : nullptr;
    int32_t h[2];
    double prm[2];
    if (!f || fread(h, sizeof h, 1, f) != 1 || fread(prm, sizeof prm, 1, f) != 1 || h[0] < 0 || h[1] < 1) return 2;
    const size_t rows = (size_t)h[0], mm = (size_t)h[1];
    std::vector<double> x(mm);
    std::vector<cplx> c(rows * mm * 10);
    if (fread(x.data(), sizeof(double), mm, f) != mm) return 2;
    if (!c.empty() && fread(c.data(), sizeof(cplx), c.size(), f) != c.size()) return 2;
    fclose(f);
    for (size_t i = 0; i < rows * mm; ++i) {
        const RedPointCplx t = red_point_cplx(&c[i * 10], x[i % mm], prm[0], prm[1]);
        printf("%d %d %d %d\n", t.fin, t.bad[0], t.bad[1], t.bad[2]);
    }
    return 0;
}
