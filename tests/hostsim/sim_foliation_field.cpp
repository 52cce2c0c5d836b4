// tests/hostsim/sim_foliation_field.cpp -- the per-point code of the gradient field kernel
// (pdeval_foliation.h: the program guard, the sample point, the order-1 interpretation and the
// finite rule) built for the CPU, one lane.  Test infrastructure only
// (tests/test_foliation_field_host.py); the product is built by hipcc for gfx950.
#include <vector>
#include "../../include/pdeval.h"
#include "../../pde-engine_amd/csrc/pdeval_foliation.h"
using namespace pd;

// The fields of n_list list rows as fol_field_kernel writes them: field [n_list][2][m^2],
// n_finite [n_list].  grid: the context's 8 doubles.  Returns the number of rows the guard or
// the interpreter declined (all NaN).
extern "C" int sim_fol_fields(const int32_t* ops, int64_t n_words, const int64_t* offsets, int64_t n,
                              const int64_t* list, int64_t n_list, const double* grid, int m, double* field,
                              int32_t* n_finite) {
    const FolGrid g = fol_grid(grid, m);
    const int mm = m * m, n_chunk = (mm + 63) / 64;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    std::vector<double> stk((size_t)kFolStackDoubles);
    const PrmTab<double> P{};   // (force-free: no constants of the problem)
    int declined = 0;
    for (int64_t row = 0; row < n_list; ++row) {
        const FolProg pr = fol_program(ops, n_words, offsets, n, list, row);
        double* out = field + row * 2 * (int64_t)mm;
        int nf = 0;
        bool row_ok = pr.ok;
        for (int chunk = 0; chunk < n_chunk; ++chunk)
            for (int lane = 0; lane < 64; ++lane) {   // (one lane at a time: stack column 0)
                const int p = chunk * 64 + lane;
                const bool active = p < mm;
                FolField f{nan, nan, false, RUN_BAD};
                if (pr.ok) {
                    f = fol_field_point(pr, g, active ? p : mm - 1, stk.data(), 0, P);
                    if (f.rc != RUN_OK) f = FolField{nan, nan, false, f.rc};
                }
                row_ok = row_ok && f.rc == RUN_OK;
                if (active) {
                    out[p] = f.a;
                    out[mm + p] = f.b;
                    nf += f.fin;
                }
            }
        n_finite[row] = nf;
        declined += !row_ok;
    }
    return declined;
}

// the sample point p of the m x m grid (the coordinates the kernel evaluates at)
extern "C" void sim_fol_point(const double* grid, int m, int p, double* xy) {
    fol_point_xy(fol_grid(grid, m), p, xy[0], xy[1]);
}
