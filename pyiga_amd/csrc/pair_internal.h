// What pair.hip (assembly over two spline spaces) and solve_saddle.hip (the saddle-point solver that takes a pair's values) share:
// the test-space tables of a pair on the device and the pair object itself.
#pragma once
#include "igx_internal.h"

#include <vector>

namespace igx {

// test space of a pair on the device: tables at the PATCH's Gauss nodes and the rectangular column ranges
struct PairAxisDev {
    int P, N, S;              // p + 1, test dofs, number of 1D (test i, trial j) pairs with overlapping support
    const double *V;          // [G][P][2] (value, derivative) of the P active test functions
    const int *fa;            // [n]   first active test dof of span s
    const int *mslo, *mshi;   // [N]   mesh-span support of test dof i
    const int *jlo, *jhi;     // [N]   trial column range of test row i
    const int *rp;            // [N+1] exclusive prefix sum of (jhi - jlo)
};
struct PairDev { PairAxisDev t[3]; };

} // namespace igx

struct igx_pair {
    igx_patch *pt = nullptr;                  // trial space, geometry, Gauss grid, form fields (not owned)
    igx_ctx *ctx = nullptr;                   // the patch's context (igx_pair_destroy does not touch the patch)
    int dim = 0;
    igx::Axis tax[3];                         // test space: host tables of setup_axis (its pair tables are square ones and unused)
    std::vector<int> jlo[3], jhi[3], rp[3];   // rectangular column ranges per axis
    double *d_kv[3] = {nullptr, nullptr, nullptr}, *d_V[3] = {nullptr, nullptr, nullptr};
    int *d_ints[3] = {nullptr, nullptr, nullptr};   // one allocation per axis: fa | mslo | mshi | jlo | jhi | rp
    igx::PairDev dev{};
    long long nrows = 0, ncols = 0, nnz = 0;
    int maxrow = 1;                           // longest row
    double *d_data = nullptr;
    int32_t *d_indptr = nullptr, *d_indices = nullptr;
    bool have_pattern = false;
    size_t *d_ws_ij = nullptr; double *d_ws_out = nullptr;      // grow-only workspaces of igx_pair_entries
    size_t ws_cap = 0;
    igx_timing timing{};
};
