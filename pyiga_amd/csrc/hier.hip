// Hierarchical (HB / THB) spline spaces: the level-coupling contraction (include/igx.h igx_hier_contract_d; host planning in
// pyiga_amd/hierarchical.py).
//
// Every value of the HB matrix is a short weighted sum of entries of ONE tensor-product level matrix A_k:
//     A[a, b] = sum_i W[i, a] A_k[i, b]        (a active on level la <= k, b active on level k, row = test function)
//     A[b, a] = sum_i A_k[b, i] W[i, a]
// with W the Kronecker product of the composite 1D two-scale matrices la -> k and i over the children of a on level k whose
// support overlaps that of b: at most 2p+1 per axis, 49 terms in 2D p = 3, 343 in 3D p = 3.  The entries of the needed rows of
// A_k are resident (igx_entries_d wrote them, row slot by row slot, each row its tensor-product stencil), so a term is found by
// arithmetic on small per-axis tables -- no list of (source, weight) per term exists anywhere.
//
// Shape: a group of G lanes (16 or 64, chosen by the host from the largest term count of the block) owns one output entry.
// Lane l takes the terms l, l + G, .. in ascending order, then the G partial sums are added by a shuffle tree of fixed shape.
// One lane writes the value to its final CSR position (and its mirror position): no atomics, and the value does not depend on
// the grid.  The kernel is a gather: per term one 8-byte entry at an address that follows the slot map (neighbouring lanes of a
// group read neighbouring stencil columns or neighbouring rows, i.e. mostly the same or adjacent 128-byte lines) plus table
// reads that stay in L2; per item 16 bytes of indices in and 8 or 16 bytes out.  It is judged against memory traffic, not FP64
// issue: two FMAs per 8-byte gather.
#include "igx_internal.h"
#include <climits>

namespace igx {

struct HierAxis {
    const int *clo, *ccnt;
    const double *w;
    const int *first, *cnt;
    int wmax, n_coarse, n_fine, box_lo, box_n;
};

struct HierArgs {
    int dim, symmetric;
    HierAxis ax[3];
    const int *slot;
    const long long *rowptr;
    const double *E;
    long long n_entries;
    const int *ia, *ib, *pos, *pos2;
    long long n_items, nnz;
    double *vals;
};

template <int G>
__global__ void __launch_bounds__(256) k_hier_contract(const HierArgs H)
{
    const int lane = threadIdx.x % G;
    const long long ngroups = (long long)gridDim.x * (256 / G);
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    for (long long it = (long long)blockIdx.x * (256 / G) + threadIdx.x / G; it < H.n_items; it += ngroups) {
        int ra = H.ia[it], rb = H.ib[it];
        int a[3], b[3], lo[3], n[3], clo[3];
        int T = 1;
        bool ok = true;
        for (int x = H.dim - 1; x >= 0; --x) {
            const HierAxis &A = H.ax[x];
            a[x] = ra % A.n_coarse; ra /= A.n_coarse;
            b[x] = rb % A.n_fine;   rb /= A.n_fine;
            clo[x] = A.clo[a[x]];
            const int chi = clo[x] + A.ccnt[a[x]];
            const int f = A.first[b[x]], l = f + A.cnt[b[x]];
            lo[x] = clo[x] > f ? clo[x] : f;
            const int hi = chi < l ? chi : l;
            n[x] = hi > lo[x] ? hi - lo[x] : 0;
            T *= n[x];
        }
        // the row of b (the other orientation reads its stencil)
        long long rowb = -1;
        if (!H.symmetric) {
            long long bi = 0;
            for (int x = 0; x < H.dim; ++x) {
                const int o = b[x] - H.ax[x].box_lo;
                ok = ok && o >= 0 && o < H.ax[x].box_n;
                bi = bi * H.ax[x].box_n + o;
            }
            const int s = ok ? H.slot[bi] : -1;
            ok = ok && s >= 0;
            rowb = ok ? H.rowptr[s] : -1;
        }
        double fwd = 0.0, bwd = 0.0;
        for (int t = lane; t < T; t += G) {
            int rem = t;
            int i[3];
            for (int x = H.dim - 1; x >= 0; --x) {
                i[x] = lo[x] + rem % n[x];
                rem /= n[x];
            }
            double w = 1.0;
            long long bi = 0, cf = 0, cb = 0;
            bool in = true;
            for (int x = 0; x < H.dim; ++x) {
                const HierAxis &A = H.ax[x];
                w *= A.w[(long long)a[x] * A.wmax + (i[x] - clo[x])];
                const int o = i[x] - A.box_lo;
                in = in && o >= 0 && o < A.box_n;
                bi = bi * A.box_n + o;
                cf = cf * A.cnt[i[x]] + (b[x] - A.first[i[x]]);
                cb = cb * A.cnt[b[x]] + (i[x] - A.first[b[x]]);
            }
            const int s = in ? H.slot[bi] : -1;
            const long long ef = s >= 0 ? H.rowptr[s] + cf : -1;
            fwd += (ef >= 0 && ef < H.n_entries) ? w * H.E[ef] : nan;
            if (!H.symmetric) {
                const long long eb = rowb >= 0 ? rowb + cb : -1;
                bwd += (eb >= 0 && eb < H.n_entries) ? H.E[eb] * w : nan;
            }
        }
#pragma unroll
        for (int o = G / 2; o > 0; o >>= 1) {
            fwd += __shfl_down(fwd, o, G);
            bwd += __shfl_down(bwd, o, G);
        }
        if (lane == 0) {
            const int p1 = H.pos[it], p2 = H.pos2[it];
            if (p1 >= 0 && p1 < H.nnz) H.vals[p1] = fwd;
            if (p2 >= 0 && p2 < H.nnz) H.vals[p2] = H.symmetric ? fwd : bwd;
        }
    }
}

__global__ void __launch_bounds__(256) k_hier_gather(const double *src, long long n_src, const long long *idx, long long n, double *dst)
{
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < n; t += (long long)gridDim.x * 256) {
        const long long s = idx[t];
        dst[t] = (s >= 0 && s < n_src) ? src[s] : nan;
    }
}

} // namespace igx

using namespace igx;

extern "C" {

int igx_hier_contract_d(igx_ctx *ctx, const igx_hier_block *blk, double *d_values, int64_t nnz, float *ms)
{
    if (!ctx || !blk || !d_values) { set_error("igx_hier_contract_d: null argument"); return IGX_ERR_ARG; }
    if (blk->dim < 2 || blk->dim > IGX_MAX_DIM) { set_error("igx_hier_contract_d: dim %d (2 or 3)", blk->dim); return IGX_ERR_ARG; }
    if (blk->group != 16 && blk->group != 64) { set_error("igx_hier_contract_d: group of %d lanes (16 or 64)", blk->group); return IGX_ERR_ARG; }
    if (blk->n_items < 0 || nnz < 0 || nnz > INT_MAX || blk->n_entries < 0 || blk->max_blocks < 0) {
        set_error("igx_hier_contract_d: negative size / more than 2^31-1 values"); return IGX_ERR_ARG;
    }
    if (ms) *ms = 0.0f;
    if (blk->n_items == 0) return IGX_OK;
    if (!blk->d_slot || !blk->d_rowptr || !blk->d_entries || !blk->d_ia || !blk->d_ib || !blk->d_pos || !blk->d_pos2) {
        set_error("igx_hier_contract_d: null device pointer in the block"); return IGX_ERR_ARG;
    }
    HierArgs H{};
    H.dim = blk->dim; H.symmetric = blk->symmetric ? 1 : 0;
    long long box = 1;
    for (int x = 0; x < blk->dim; ++x) {
        const igx_hier_axis &A = blk->ax[x];
        if (!A.d_clo || !A.d_ccnt || !A.d_w || !A.d_first || !A.d_cnt || A.wmax < 1 || A.n_coarse < 1 || A.n_fine < 1 || A.box_n < 1 || A.box_lo < 0) {
            set_error("igx_hier_contract_d: axis %d: null table or empty range", x); return IGX_ERR_ARG;
        }
        H.ax[x] = HierAxis{A.d_clo, A.d_ccnt, A.d_w, A.d_first, A.d_cnt, A.wmax, A.n_coarse, A.n_fine, A.box_lo, A.box_n};
        box *= A.box_n;
    }
    if (box >= (1LL << 40)) { set_error("igx_hier_contract_d: slot map too large"); return IGX_ERR_ARG; }
    H.slot = blk->d_slot; H.rowptr = (const long long *)blk->d_rowptr; H.E = blk->d_entries; H.n_entries = blk->n_entries;
    H.ia = blk->d_ia; H.ib = blk->d_ib; H.pos = blk->d_pos; H.pos2 = blk->d_pos2;
    H.n_items = blk->n_items; H.nnz = nnz; H.vals = d_values;
    IGX_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int per_block = 256 / blk->group;
    long long blocks = (blk->n_items + per_block - 1) / per_block;
    const long long cap = blk->max_blocks > 0 ? blk->max_blocks : (long long)ctx->ncu * 8;      // (8 blocks of 256 threads per CU: from the block size, occupancy not measured)
    if (blocks > cap) blocks = cap;
    // (timed: two events around the launch and a wait; they are destroyed on every path)
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t err = hipSuccess;
    if (ms) {
        err = hipEventCreate(&e0);
        if (err == hipSuccess) err = hipEventCreate(&e1);
        if (err == hipSuccess) err = hipEventRecord(e0, st);
    }
    if (err == hipSuccess) {
        if (blk->group == 64) k_hier_contract<64><<<dim3((unsigned)blocks), dim3(256), 0, st>>>(H);
        else k_hier_contract<16><<<dim3((unsigned)blocks), dim3(256), 0, st>>>(H);
        err = hipGetLastError();
    }
    if (ms && err == hipSuccess) {
        err = hipEventRecord(e1, st);
        if (err == hipSuccess) err = hipEventSynchronize(e1);
        if (err == hipSuccess) err = hipEventElapsedTime(ms, e0, e1);
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (err != hipSuccess) {
        set_error("igx_hier_contract_d: %s", hipGetErrorString(err));
        return IGX_ERR_HIP;
    }
    return IGX_OK;
}

int igx_hier_gather_d(igx_ctx *ctx, const double *d_src, int64_t n_src, const int64_t *d_idx, int64_t n_idx, double *d_dst)
{
    if (!ctx || n_idx < 0 || n_src < 0) { set_error("igx_hier_gather_d: null context / negative size"); return IGX_ERR_ARG; }
    if (n_idx == 0) return IGX_OK;
    if (!d_src || !d_idx || !d_dst) { set_error("igx_hier_gather_d: null device pointer"); return IGX_ERR_ARG; }
    IGX_HIP(hipSetDevice(ctx->device));
    long long blocks = (n_idx + 255) / 256;
    if (blocks > (long long)ctx->ncu * 8) blocks = (long long)ctx->ncu * 8;
    k_hier_gather<<<dim3((unsigned)blocks), dim3(256), 0, ctx->stream>>>(d_src, n_src, (const long long *)d_idx, n_idx, d_dst);
    IGX_HIP(hipGetLastError());
    return IGX_OK;
}

} // extern "C"
