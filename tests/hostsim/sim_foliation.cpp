// tests/hostsim/sim_foliation.cpp -- the per-point code of the Jacobian match kernel
// (pdeval_foliation.h: the point test, the leader round) built for the CPU, one lane.  Test
// infrastructure only (tests/test_foliation_host.py); the product is built by hipcc for gfx950.
#include <vector>
#include "../../include/pdeval.h"
#include "../../pde-engine_amd/csrc/pdeval_foliation.h"
using namespace pd;

// One row field against one probe field (2 mm doubles each), as fol_match_kernel counts.
// Returns 1 on a match.
extern "C" int sim_fol_match(const double* row, const double* probe, int mm, double tau, int min_points,
                             int* n_used, int* n_bad, double* qmax) {
    int nu = 0, nb = 0;
    double q = 0.0;
    for (int p = 0; p < mm; ++p) {
        const FolPoint t = fol_point_test(row[p], row[mm + p], probe[p], probe[mm + p], tau);
        nu += t.used;
        nb += t.bad;
        if (t.used) q = fmax(q, fol_q(t));
    }
    if (n_used) *n_used = nu;
    if (n_bad) *n_bad = nb;
    if (qmax) *qmax = q;
    return nu >= min_points && nb == 0;
}

// The grouping on host fields: rounds of up to 32 probes, fol_round assigning.
// leader[i]: the leader's row, or -1 with fewer than min_points finite points.  Returns the
// number of classes; *rounds the number of rounds.
extern "C" int sim_fol_classes(const double* fields, int n, int mm, double tau, int min_points, int64_t* leader,
                               int* rounds) {
    std::vector<int64_t> un, next;
    for (int i = 0; i < n; ++i) {
        leader[i] = -1;
        int nfin = 0;
        for (int p = 0; p < mm; ++p) nfin += fields[(size_t)i * 2 * mm + p] == fields[(size_t)i * 2 * mm + p];
        if (nfin >= min_points) un.push_back(i);
    }
    int classes = 0, nr = 0;
    std::vector<uint32_t> mask;
    while (!un.empty()) {
        const int64_t nu = (int64_t)un.size();
        const int np = (int)std::min<int64_t>(PDEVAL_FOL_MAX_PROBES, nu);
        mask.assign((size_t)nu, 0u);
        for (int64_t r = 0; r < nu; ++r)
            for (int k = 0; k < np; ++k)
                if (sim_fol_match(fields + (size_t)un[r] * 2 * mm, fields + (size_t)un[k] * 2 * mm, mm, tau,
                                  min_points, nullptr, nullptr, nullptr))
                    mask[(size_t)r] |= 1u << k;
        classes += fol_round(mask.data(), un.data(), nu, np, nullptr, leader, next);
        un.swap(next);
        ++nr;
    }
    if (rounds) *rounds = nr;
    return classes;
}
