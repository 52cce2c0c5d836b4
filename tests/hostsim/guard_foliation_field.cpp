// tests/hostsim/guard_foliation_field.cpp -- a stand-alone check of the field code's bounds guard
// (pdeval_foliation.h fol_program), built with -fsanitize=address,undefined by
// tests/test_foliation_field_host.py: every array is a heap block of its exact size, so a read
// of a program word, an offset or a list entry outside it ends the run.  Rows whose offsets fall
// outside [0, n_words] or whose list entry lies outside [0, n) must come back all NaN with
// n_finite 0; the good rows must not.  Test infrastructure only.
#include <cmath>
#include <cstdio>
#include <memory>

#include "sim_foliation_field.cpp"

int main() {
    const int m = 5, mm = m * m;
    // two good programs: u = rho, and u = rho * z
    const int32_t prog[] = {(int32_t)(1u << 8), PDOP_PUSH_X, (int32_t)(1u << 8), PDOP_PUSH_X, PDOP_MUL_Y};
    const int64_t n_words = 5;
    std::unique_ptr<int32_t[]> ops(new int32_t[n_words]);
    for (int i = 0; i < n_words; ++i) ops[i] = prog[i];
    // candidates: 0 good, 1 good, 2 end past n_words, 3 negative begin, 4 end < begin, 5 empty,
    // 6 begin far past n_words
    const int64_t n = 7;
    const int64_t offs[2 * 7] = {0, 2, 2, 5, 2, 6, -3, 2, 4, 1, 3, 3, (int64_t)1 << 40, ((int64_t)1 << 40) + 2};
    const double grid[8] = {0.05, 3.0, 64, -2.0, 2.0, 64, 0.37, 0.41};
    int failures = 0;
    for (int64_t c = 0; c < n; ++c) {
        // offsets[c], offsets[c + 1] of candidate c alone: the guard reads exactly these two
        std::unique_ptr<int64_t[]> off(new int64_t[2]);
        off[0] = offs[2 * c];
        off[1] = offs[2 * c + 1];
        const int64_t lists[4] = {0, -1, 1, (int64_t)1 << 33};   // list entries: only 0 is inside [0, 1)
        for (int l = 0; l < 4; ++l) {
            std::unique_ptr<int64_t[]> list(new int64_t[1]);
            list[0] = lists[l];
            std::unique_ptr<double[]> field(new double[2 * mm]);
            std::unique_ptr<int32_t[]> nfin(new int32_t[1]);
            const int declined = sim_fol_fields(ops.get(), n_words, off.get(), 1, list.get(), 1, grid, m, field.get(),
                                                nfin.get());
            const bool good = c < 2 && l == 0;
            int nan = 0;
            for (int p = 0; p < 2 * mm; ++p) nan += std::isnan(field[p]);
            const bool ok = good ? (declined == 0 && nan == 0 && nfin[0] == mm) : (declined == 1 && nan == 2 * mm && nfin[0] == 0);
            if (!ok) {
                std::printf("candidate %d list %d: declined %d nan %d n_finite %d\n", (int)c, l, declined, nan, nfin[0]);
                ++failures;
            }
        }
    }
    std::printf("guard: %d failures\n", failures);
    return failures ? 1 : 0;
}
