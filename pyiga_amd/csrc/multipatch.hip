// Multipatch: the global CSR of  sum_p X_p A_p X_p^T  on the device (igx_multipatch_*, include/igx.h).
//
// Replaces the host step of the reference's Multipatch.assemble_system (pyiga/assemble.py:1340-1370), which forms
// X_p @ A_p @ X_p.T and adds it to the global matrix with scipy, once per patch.  Here
//   create:  the global pattern is built once from the device patterns of the patches and the local-to-global maps
//            (count -> scan -> fill -> per-row sort / de-duplicate -> scan -> compact), then the global position of every
//            local entry is found (binary search in its global row) and each local row is classified for the scatter;
//   scatter: one stream-ordered pass per patch, vals_global[pos_p(k)] (+)= vals_p[k], reading the patch's device values.
// Scatter classes of a local row i of patch p, global row r = l2g_p[i] (DESIGN.md section 11 has the byte budget):
//   DIRECT  r is reached by this row only and its global row is the local row, entry for entry:  pos = k + delta.
//           A store, and no position array.
//   STORE   r is reached by this row only, columns permuted (a shared column sorts to the end):  out[pos[k]] = v.
//   RMW     r is reached by several rows (an interface dof):  out[pos[k]] += v  -- plain read-add-write; the passes of the
//           patches are ordered on the stream, so the sum is ((0 + a_0) + a_1) + ..., the reference's order.
//   ATOMIC  the map of the patch is not injective (two of its local dofs share a global one): entries of one pass may
//           collide, atomicAdd; the sum is then correct to rounding only.
#include "igx_internal.h"

#include <algorithm>
#include <climits>
#include <new>
#include <vector>

using namespace igx;

namespace {

constexpr int WAVE = 64;
constexpr int SORT_TILE = 1024;          // longest raw global row sorted in the LDS of one wave; longer rows: k_sort_long


__device__ __forceinline__ unsigned long long lanemask_lt(int lane) { return (1ull << lane) - 1ull; }

// ---------------------------------------------------------------------------------------------
// exclusive scan, int64 output with the total in out[n]
constexpr int SCAN_BLOCK = 256, SCAN_ITEMS = 4, SCAN_TILE = SCAN_BLOCK * SCAN_ITEMS;

template <typename T>
__global__ void k_scan_tiles(const T *in, long long n, long long *out, long long *tile_sums)
{
    __shared__ long long s[SCAN_BLOCK];
    const long long base = (long long)blockIdx.x * SCAN_TILE + (long long)threadIdx.x * SCAN_ITEMS;
    long long v[SCAN_ITEMS], sum = 0;
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        v[k] = base + k < n ? (long long)in[base + k] : 0;
        sum += v[k];
    }
    s[threadIdx.x] = sum;
    __syncthreads();
    for (int off = 1; off < SCAN_BLOCK; off <<= 1) {           // inclusive Hillis-Steele over the thread sums
        long long t = threadIdx.x >= (unsigned)off ? s[threadIdx.x - off] : 0;
        __syncthreads();
        s[threadIdx.x] += t;
        __syncthreads();
    }
    long long run = s[threadIdx.x] - sum;
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        if (base + k < n) out[base + k] = run;
        run += v[k];
    }
    if (threadIdx.x == SCAN_BLOCK - 1) tile_sums[blockIdx.x] = s[threadIdx.x];
}

__global__ void k_scan_sums(long long *sums, long long nt)      // one block: exclusive scan of the tile sums in place
{
    __shared__ long long s[SCAN_BLOCK];
    __shared__ long long carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (long long c0 = 0; c0 < nt; c0 += SCAN_BLOCK) {
        const long long i = c0 + threadIdx.x;
        const long long v = i < nt ? sums[i] : 0;
        s[threadIdx.x] = v;
        __syncthreads();
        for (int off = 1; off < SCAN_BLOCK; off <<= 1) {
            long long t = threadIdx.x >= (unsigned)off ? s[threadIdx.x - off] : 0;
            __syncthreads();
            s[threadIdx.x] += t;
            __syncthreads();
        }
        if (i < nt) sums[i] = carry + s[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == SCAN_BLOCK - 1) carry += s[threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x == 0) sums[nt] = carry;
}

__global__ void k_scan_add(long long *out, long long n, const long long *tile_sums, long long nt)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] += tile_sums[i / SCAN_TILE];
    if (i == 0) out[n] = tile_sums[nt];
}

template <typename T>
int scan_exclusive(hipStream_t st, const T *d_in, long long n, long long *d_out, long long *d_tiles)
{
    const long long nt = std::max(1LL, (n + SCAN_TILE - 1) / SCAN_TILE);
    k_scan_tiles<T><<<(unsigned)nt, SCAN_BLOCK, 0, st>>>(d_in, n, d_out, d_tiles);
    k_scan_sums<<<1, SCAN_BLOCK, 0, st>>>(d_tiles, nt);
    k_scan_add<<<(unsigned)((n + 255) / 256 + 1), 256, 0, st>>>(d_out, n, d_tiles, nt);
    IGX_HIP(hipGetLastError());
    return IGX_OK;
}

// ---------------------------------------------------------------------------------------------
// pattern build
__global__ void k_count(const int32_t *l2g, const int32_t *indptr, int n, int32_t *cnt, int32_t *contrib)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int r = l2g[i];
    atomicAdd(&cnt[r], indptr[i + 1] - indptr[i]);
    atomicAdd(&contrib[r], 1);
}

// one wave per local row: reserve a slot range in global row r, write the mapped columns
__global__ void k_fill(const int32_t *l2g, const int32_t *indptr, const int32_t *indices, int n,
                       const long long *upoff, int32_t *cursor, int32_t *upper)
{
    const int lane = threadIdx.x % WAVE;
    const long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
    if (i >= n) return;
    const int r = l2g[i];
    const int k0 = indptr[i], len = indptr[i + 1] - k0;
    int slot = 0;
    if (lane == 0) slot = atomicAdd(&cursor[r], len);
    slot = __shfl(slot, 0);
    int32_t *dst = upper + upoff[r] + slot;
    for (int t = lane; t < len; t += WAVE) dst[t] = l2g[indices[k0 + t]];
}

// one wave per global row: sort + de-duplicate in place (LDS bitonic sort); the unique count to ucnt[r].  A row reached by
// one local row whose mapped columns already increase strictly is left as it is.  Rows longer than SORT_TILE are listed for
// k_sort_long.
__global__ void __launch_bounds__(WAVE) k_sort_rows(const long long *upoff, const int32_t *cnt, const int32_t *contrib, long long nrows,
                                                    int32_t *upper, int32_t *ucnt, int32_t *long_rows, int32_t *n_long)
{
    __shared__ int32_t s[SORT_TILE];
    const int lane = threadIdx.x;
    const long long r = blockIdx.x;
    if (r >= nrows) return;
    const int L = cnt[r];
    int32_t *row = upper + upoff[r];
    if (contrib[r] == 1) {
        bool bad = false;
        for (int t = lane; t + 1 < L; t += WAVE) bad |= row[t] >= row[t + 1];
        if (!__any(bad)) {
            if (lane == 0) ucnt[r] = L;
            return;
        }
    }
    if (L > SORT_TILE) {
        if (lane == 0) { ucnt[r] = 0; long_rows[atomicAdd(n_long, 1)] = (int32_t)r; }
        return;
    }
    int n = 1;
    while (n < L) n <<= 1;
    for (int t = lane; t < n; t += WAVE) s[t] = t < L ? row[t] : INT_MAX;
    __syncthreads();
    for (int k = 2; k <= n; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = lane; t < n; t += WAVE) {
                const int u = t ^ j;
                if (u > t) {
                    const int32_t a = s[t], b = s[u];
                    if ((a > b) == ((t & k) == 0)) { s[t] = b; s[u] = a; }
                }
            }
            __syncthreads();
        }
    int u = 0;
    for (int b0 = 0; b0 < L; b0 += WAVE) {
        const int t = b0 + lane;
        const bool keep = t < L && (t == 0 || s[t] != s[t - 1]);
        const unsigned long long m = __ballot(keep);
        if (keep) row[u + __popcll(m & lanemask_lt(lane))] = s[t];
        u += __popcll(m);
    }
    if (lane == 0) ucnt[r] = u;
}

// rows longer than SORT_TILE (a dof where many patches meet, in 3D): rank sort into tmp, then one thread de-duplicates
__global__ void k_sort_long(const long long *upoff, const int32_t *cnt, const int32_t *long_rows, int32_t *upper, int32_t *tmp, int32_t *ucnt)
{
    const int r = long_rows[blockIdx.x];
    const int L = cnt[r];
    int32_t *row = upper + upoff[r], *dst = tmp + upoff[r];
    for (int a = threadIdx.x; a < L; a += blockDim.x) {
        const int32_t v = row[a];
        int rank = 0;
        for (int b = 0; b < L; ++b) {
            const int32_t w = row[b];
            rank += (w < v) || (w == v && b < a);
        }
        dst[rank] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int u = 0;
        for (int a = 0; a < L; ++a)
            if (a == 0 || dst[a] != dst[a - 1]) row[u++] = dst[a];
        ucnt[r] = u;
    }
}

__global__ void k_compact(const long long *upoff, const int32_t *upper, const int32_t *ucnt, const long long *gptr, long long nrows,
                          int32_t *indptr, int32_t *indices)
{
    const int lane = threadIdx.x % WAVE;
    const long long r = ((long long)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
    if (r > nrows) return;
    if (lane == 0) indptr[r] = (int32_t)gptr[r];
    if (r == nrows) return;
    const int32_t *src = upper + upoff[r];
    int32_t *dst = indices + gptr[r];
    for (int t = lane; t < ucnt[r]; t += WAVE) dst[t] = src[t];
}

// one wave per local row: global position of every local entry (binary search in the sorted global row) and the row's class
__global__ void k_positions(const int32_t *l2g, const int32_t *indptr, const int32_t *indices, int n, bool injective,
                            const int32_t *gindptr, const int32_t *gindices, const int32_t *contrib,
                            int32_t *pos, RowInfo *info, int32_t *ndlen, int32_t *err)
{
    const int lane = threadIdx.x % WAVE;
    const long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
    if (i >= n) return;
    const int r = l2g[i];
    const int k0 = indptr[i], len = indptr[i + 1] - k0;
    const int g0 = gindptr[r], glen = gindptr[r + 1] - g0;
    const int32_t *grow = gindices + g0;
    bool shifted = false;
    for (int t = lane; t < len; t += WAVE) {
        const int32_t c = l2g[indices[k0 + t]];
        int lo = 0, hi = glen;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (grow[mid] < c) lo = mid + 1; else hi = mid;
        }
        if (lo >= glen || grow[lo] != c) { atomicExch(err, 1); lo = 0; }
        pos[k0 + t] = g0 + lo;
        shifted |= lo != t;
    }
    const bool direct = injective && contrib[r] == 1 && glen == len && !__any(shifted);
    if (lane == 0) {
        RowInfo ri;
        ri.kstart = k0;
        ri.len = len;
        ri.mode = !injective ? MODE_ATOMIC : direct ? MODE_DIRECT : contrib[r] == 1 ? MODE_STORE : MODE_RMW;
        ri.base = direct ? g0 - k0 : 0;                          // (position-array offset of the other classes: k_compact_pos)
        info[i] = ri;
        ndlen[i] = direct ? 0 : len;
    }
}

__global__ void k_compact_pos(const int32_t *pos, int n, const long long *ndofs, RowInfo *info, int32_t *cpos)
{
    const int lane = threadIdx.x % WAVE;
    const long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
    if (i >= n) return;
    RowInfo ri = info[i];
    if (ri.mode == MODE_DIRECT) return;
    const long long o = ndofs[i];
    for (int t = lane; t < ri.len; t += WAVE) cpos[o + t] = pos[ri.kstart + t];
    if (lane == 0) info[i].base = (int32_t)o;
}

// ---------------------------------------------------------------------------------------------
// scatter: one wave per local row
__global__ void k_scatter(const RowInfo *info, const int32_t *cpos, int n, const double *vals, double *out)
{
    const int lane = threadIdx.x % WAVE;
    const long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
    if (i >= n) return;
    const RowInfo ri = info[i];
    const double *v = vals + ri.kstart;
    if (ri.mode == MODE_DIRECT) {
        double *o = out + (long long)ri.kstart + ri.base;
        for (int t = lane; t < ri.len; t += WAVE) o[t] = v[t];
        return;
    }
    const int32_t *q = cpos + ri.base;
    if (ri.mode == MODE_STORE)
        for (int t = lane; t < ri.len; t += WAVE) out[q[t]] = v[t];
    else if (ri.mode == MODE_RMW)
        for (int t = lane; t < ri.len; t += WAVE) out[q[t]] += v[t];
    else
        for (int t = lane; t < ri.len; t += WAVE) atomicAdd(&out[q[t]], v[t]);
}

__global__ void k_scatter_vec(const int32_t *l2g, int n, const int32_t *contrib, bool injective, const double *b, double *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int g = l2g[i];
    if (!injective) atomicAdd(&out[g], b[i]);
    else if (contrib[g] == 1) out[g] = b[i];
    else out[g] += b[i];
}

unsigned waves_grid(long long nwaves, int block = 256) { return (unsigned)((nwaves * WAVE + block - 1) / block); }

} // namespace


namespace {

void mp_free(igx_multipatch *mp)
{
    (void)hipSetDevice(mp->ctx->device);
    (void)hipStreamSynchronize(mp->ctx->stream);
    for (auto &p : mp->pp) { (void)hipFree(p.d_l2g); (void)hipFree(p.d_info); (void)hipFree(p.d_cpos); (void)hipFree(p.d_tab); }
    (void)hipFree(mp->d_indptr); (void)hipFree(mp->d_indices); (void)hipFree(mp->d_contrib);
    (void)hipFree(mp->d_vals); (void)hipFree(mp->d_vec); (void)hipFree(mp->d_stage);
    delete mp;
}

// device scratch freed on every exit of the build
struct Scratch {
    std::vector<void *> ptrs;
    ~Scratch() { for (void *p : ptrs) (void)hipFree(p); }
    template <typename T> hipError_t alloc(T **p, size_t n)
    {
        hipError_t e = hipMalloc((void **)p, std::max<size_t>(1, n) * sizeof(T));
        if (e == hipSuccess) ptrs.push_back(*p); else *p = nullptr;
        return e;
    }
};

#define MP_ALLOC(S, ptr, n, what)                                                                              \
    do {                                                                                                      \
        if ((S).alloc(&(ptr), (n)) != hipSuccess) {                                                           \
            (void)hipGetLastError();                                                                          \
            set_error("igx_multipatch_create: hipMalloc of %.3f GB (%s) failed", (double)(n) * sizeof(*(ptr)) / 1e9, what); \
            return IGX_ERR_NOMEM;                                                                             \
        }                                                                                                     \
    } while (0)

#define MP_KEEP(ptr, n, what)                                                                                  \
    do {                                                                                                      \
        if (hipMalloc((void **)&(ptr), std::max<size_t>(1, (size_t)(n)) * sizeof(*(ptr))) != hipSuccess) {     \
            (void)hipGetLastError(); ptr = nullptr;                                                           \
            set_error("igx_multipatch_create: hipMalloc of %.3f GB (%s) failed", (double)(n) * sizeof(*(ptr)) / 1e9, what); \
            return IGX_ERR_NOMEM;                                                                             \
        }                                                                                                     \
    } while (0)

int mp_build(igx_multipatch *mp, igx_patch *const *patches, const int32_t *const *l2g)
{
    hipStream_t st = mp->ctx->stream;
    const long long G = mp->nglobal;
    Scratch S;
    int32_t *d_cnt, *d_cursor, *d_upper, *d_ucnt, *d_long, *d_nlong, *d_err;
    long long *d_upoff, *d_gptr, *d_tiles;
    MP_ALLOC(S, d_cnt, G, "row counts");
    MP_ALLOC(S, d_cursor, G, "row cursors");
    MP_ALLOC(S, d_ucnt, G, "unique counts");
    MP_ALLOC(S, d_upoff, G + 1, "row offsets");
    MP_ALLOC(S, d_gptr, G + 1, "row pointers");
    long long max_n = G;
    for (int p = 0; p < mp->np; ++p) max_n = std::max<long long>(max_n, mp->pp[p].n);
    MP_ALLOC(S, d_tiles, max_n / SCAN_TILE + 2, "scan tiles");
    MP_ALLOC(S, d_nlong, 2, "counters");
    d_err = d_nlong + 1;
    MP_KEEP(mp->d_contrib, G, "contributions per row");
    MP_KEEP(mp->d_indptr, G + 1, "global indptr");
    IGX_HIP(hipMemsetAsync(d_cnt, 0, G * sizeof(int32_t), st));
    IGX_HIP(hipMemsetAsync(d_cursor, 0, G * sizeof(int32_t), st));
    IGX_HIP(hipMemsetAsync(mp->d_contrib, 0, G * sizeof(int32_t), st));
    IGX_HIP(hipMemsetAsync(d_nlong, 0, 2 * sizeof(int32_t), st));
    // count
    for (int p = 0; p < mp->np; ++p) {
        auto &P = mp->pp[p];
        MP_KEEP(P.d_l2g, P.n, "local-to-global map");
        IGX_HIP(hipMemcpyAsync(P.d_l2g, l2g[p], P.n * sizeof(int32_t), hipMemcpyHostToDevice, st));
        k_count<<<(P.n + 255) / 256, 256, 0, st>>>(P.d_l2g, patches[p]->d_indptr, P.n, d_cnt, mp->d_contrib);
    }
    IGX_HIP(hipGetLastError());
    // scan -> fill
    if (int rc = scan_exclusive(st, d_cnt, G, d_upoff, d_tiles)) return rc;
    long long raw = 0;
    IGX_HIP(hipMemcpyAsync(&raw, d_upoff + G, sizeof(long long), hipMemcpyDeviceToHost, st));
    IGX_HIP(hipStreamSynchronize(st));
    MP_ALLOC(S, d_upper, raw, "unsorted global rows");
    for (int p = 0; p < mp->np; ++p) {
        auto &P = mp->pp[p];
        k_fill<<<waves_grid(P.n), 256, 0, st>>>(P.d_l2g, patches[p]->d_indptr, patches[p]->d_indices, P.n, d_upoff, d_cursor, d_upper);
    }
    IGX_HIP(hipGetLastError());
    // sort / de-duplicate per row
    MP_ALLOC(S, d_long, G, "long-row list");
    if (G) k_sort_rows<<<(unsigned)G, WAVE, 0, st>>>(d_upoff, d_cnt, mp->d_contrib, G, d_upper, d_ucnt, d_long, d_nlong);
    IGX_HIP(hipGetLastError());
    int nlong = 0;
    IGX_HIP(hipMemcpyAsync(&nlong, d_nlong, sizeof(int), hipMemcpyDeviceToHost, st));
    IGX_HIP(hipStreamSynchronize(st));
    if (nlong) {
        int32_t *d_tmp;
        MP_ALLOC(S, d_tmp, raw, "sort scratch of long rows");
        k_sort_long<<<nlong, 256, 0, st>>>(d_upoff, d_cnt, d_long, d_upper, d_tmp, d_ucnt);
        IGX_HIP(hipGetLastError());
    }
    // scan of the unique counts -> global indptr, indices
    if (int rc = scan_exclusive(st, d_ucnt, G, d_gptr, d_tiles)) return rc;
    long long nnz = 0;
    IGX_HIP(hipMemcpyAsync(&nnz, d_gptr + G, sizeof(long long), hipMemcpyDeviceToHost, st));
    IGX_HIP(hipStreamSynchronize(st));
    if (nnz >= (1LL << 31)) {
        set_error("igx_multipatch_create: the global pattern has %lld >= 2^31 entries (CSR indices are int32)", nnz);
        return IGX_ERR_UNSUPPORTED;
    }
    mp->nnz = nnz;
    MP_KEEP(mp->d_indices, nnz, "global indices");
    k_compact<<<waves_grid(G + 1), 256, 0, st>>>(d_upoff, d_upper, d_ucnt, d_gptr, G, mp->d_indptr, mp->d_indices);
    IGX_HIP(hipGetLastError());
    // positions and scatter classes per patch
    IGX_HIP(hipMemsetAsync(d_err, 0, sizeof(int32_t), st));
    for (int p = 0; p < mp->np; ++p) {
        auto &P = mp->pp[p];
        int32_t *d_pos, *d_ndlen;
        long long *d_ndofs;
        MP_ALLOC(S, d_pos, P.nnz, "local positions");
        MP_ALLOC(S, d_ndlen, P.n, "row lengths");
        MP_ALLOC(S, d_ndofs, P.n + 1, "row offsets");
        MP_KEEP(P.d_info, P.n, "row plans");
        k_positions<<<waves_grid(P.n), 256, 0, st>>>(P.d_l2g, patches[p]->d_indptr, patches[p]->d_indices, P.n, mp->injective,
                                                    mp->d_indptr, mp->d_indices, mp->d_contrib, d_pos, P.d_info, d_ndlen, d_err);
        IGX_HIP(hipGetLastError());
        if (int rc = scan_exclusive(st, d_ndlen, P.n, d_ndofs, d_tiles)) return rc;
        long long ncpos = 0;
        IGX_HIP(hipMemcpyAsync(&ncpos, d_ndofs + P.n, sizeof(long long), hipMemcpyDeviceToHost, st));
        IGX_HIP(hipStreamSynchronize(st));
        MP_KEEP(P.d_cpos, ncpos, "position array");
        k_compact_pos<<<waves_grid(P.n), 256, 0, st>>>(d_pos, P.n, d_ndofs, P.d_info, P.d_cpos);
        IGX_HIP(hipGetLastError());
        std::vector<RowInfo> h(P.n);
        IGX_HIP(hipMemcpyAsync(h.data(), P.d_info, P.n * sizeof(RowInfo), hipMemcpyDeviceToHost, st));
        IGX_HIP(hipStreamSynchronize(st));
        for (const RowInfo &ri : h) mp->counts[ri.mode] += ri.len;
    }
    int err = 0;
    IGX_HIP(hipMemcpyAsync(&err, d_err, sizeof(int), hipMemcpyDeviceToHost, st));
    // the rows more than one local row reaches: where the zeroing of a new sum has to start
    std::vector<int32_t> contrib(G), gptr32(G + 1);
    IGX_HIP(hipMemcpyAsync(contrib.data(), mp->d_contrib, G * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    IGX_HIP(hipMemcpyAsync(gptr32.data(), mp->d_indptr, (G + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    IGX_HIP(hipStreamSynchronize(st));
    if (err) { set_error("igx_multipatch_create: a local entry is missing from the global pattern (internal error)"); return IGX_ERR_HIP; }
    long long first_multi = G;
    for (long long r = 0; r < G; ++r)
        if (contrib[r] != 1) { first_multi = r; break; }
    bool tail = true;
    for (long long r = first_multi; r < G && tail; ++r) tail = contrib[r] != 1;
    if (!mp->injective || !tail) first_multi = 0;
    mp->vzero_from = first_multi;
    mp->zero_from = gptr32[first_multi];
    for (long long r = 0; r < G; ++r) mp->max_row = std::max(mp->max_row, gptr32[r + 1] - gptr32[r]);
    MP_KEEP(mp->d_vals, nnz, "global values");
    MP_KEEP(mp->d_vec, G, "global vector");
    IGX_HIP(hipMemsetAsync(mp->d_vals, 0, std::max<long long>(1, nnz) * sizeof(double), st));
    IGX_HIP(hipMemsetAsync(mp->d_vec, 0, std::max<long long>(1, G) * sizeof(double), st));
    IGX_HIP(hipStreamSynchronize(st));
    return IGX_OK;
}

int stage(igx_multipatch *mp, const double *h, size_t n)
{
    hipStream_t st = mp->ctx->stream;
    if (mp->stage_len < n) {
        (void)hipStreamSynchronize(st);
        (void)hipFree(mp->d_stage);
        mp->d_stage = nullptr;
        mp->stage_len = 0;
        if (hipMalloc((void **)&mp->d_stage, std::max<size_t>(1, n) * sizeof(double)) != hipSuccess) {
            (void)hipGetLastError();
            set_error("igx_multipatch: hipMalloc of %.3f GB for host values failed", n * 8.0 / 1e9);
            return IGX_ERR_NOMEM;
        }
        mp->stage_len = n;
    }
    IGX_HIP(hipMemcpyAsync(mp->d_stage, h, n * sizeof(double), hipMemcpyHostToDevice, st));
    return IGX_OK;
}

int run_scatter(igx_multipatch *mp, int p, const double *d_src)
{
    hipStream_t st = mp->ctx->stream;
    const auto &P = mp->pp[p];
    if (P.n) k_scatter<<<waves_grid(P.n), 256, 0, st>>>(P.d_info, P.d_cpos, P.n, d_src, mp->d_vals);
    IGX_HIP(hipGetLastError());
    IGX_HIP(hipStreamSynchronize(st));     // (host staging buffer and the source patch may be reused / freed after the call)
    mp->scattered = mp->generation;
    mp->pp[p].scattered = mp->generation;
    return IGX_OK;
}

} // namespace

extern "C" {

igx_multipatch *igx_multipatch_create(igx_ctx *ctx, int npatches, igx_patch *const *patches, const int32_t *const *l2g, int64_t nglobal)
{
    if (!ctx || npatches < 1 || !patches || !l2g) { set_error("igx_multipatch_create: null argument / no patches"); return nullptr; }
    if (nglobal < 1 || nglobal >= INT_MAX) { set_error("igx_multipatch_create: %lld global dofs (1 .. 2^31-2)", (long long)nglobal); return nullptr; }
    for (int p = 0; p < npatches; ++p) {
        const igx_patch *pt = patches[p];
        if (!pt || !l2g[p]) { set_error("igx_multipatch_create: patch %d: null argument", p); return nullptr; }
        if (pt->ctx != ctx) { set_error("igx_multipatch_create: patch %d lives on another context", p); return nullptr; }
        if (pt->boxed || pt->row_lo != 0 || pt->row_hi != pt->nrows_total) {
            set_error("igx_multipatch_create: patch %d is not a whole patch (row slab / span box)", p); return nullptr;
        }
        if (pt->nnz >= (1LL << 31) || pt->nrows_total >= INT_MAX) { set_error("igx_multipatch_create: patch %d too large for int32 CSR", p); return nullptr; }
    }
    if (hipSetDevice(ctx->device) != hipSuccess) { set_error("hipSetDevice failed"); return nullptr; }
    igx_multipatch *mp = new (std::nothrow) igx_multipatch();
    if (!mp) { set_error("igx_multipatch_create: out of host memory"); return nullptr; }
    mp->ctx = ctx;
    mp->np = npatches;
    mp->nglobal = nglobal;
    mp->pp.resize(npatches);
    for (int p = 0; p < npatches; ++p) {
        auto &P = mp->pp[p];
        P.n = (int)patches[p]->nrows_total;
        P.nnz = patches[p]->nnz;
        P.dim = patches[p]->dim;
        for (int k = 0; k < P.dim; ++k) {
            const igx::Axis &A = patches[p]->ax[k];
            P.N[k] = A.N; P.p[k] = A.p;
            P.jlo[k] = A.jlo; P.jhi[k] = A.jhi; P.rp[k] = A.rp;
        }
        std::vector<int32_t> s(l2g[p], l2g[p] + P.n);
        for (int32_t g : s)
            if (g < 0 || g >= nglobal) { set_error("igx_multipatch_create: patch %d maps a dof to %d, outside [0, %lld)", p, g, (long long)nglobal); delete mp; return nullptr; }
        std::sort(s.begin(), s.end());
        if (std::adjacent_find(s.begin(), s.end()) != s.end()) mp->injective = false;
    }
    for (int p = 0; p < npatches; ++p)
        if (igx_pattern(patches[p], nullptr, nullptr)) { mp_free(mp); return nullptr; }
    if (mp_build(mp, patches, l2g)) { (void)hipGetLastError(); mp_free(mp); return nullptr; }
    return mp;
}

void igx_multipatch_destroy(igx_multipatch *mp)
{
    if (mp) mp_free(mp);
}

int igx_multipatch_get_info(const igx_multipatch *mp, igx_multipatch_info *info)
{
    if (!mp || !info) { set_error("igx_multipatch_get_info: null argument"); return IGX_ERR_ARG; }
    info->npatches = mp->np;
    info->injective = mp->injective ? 1 : 0;
    info->nrows = mp->nglobal;
    info->nnz = mp->nnz;
    for (int k = 0; k < 4; ++k) info->entries[k] = mp->counts[k];
    info->zero_from = mp->zero_from;
    return IGX_OK;
}

int igx_multipatch_pattern(const igx_multipatch *mp, int32_t *indptr, int32_t *indices)
{
    if (!mp) { set_error("igx_multipatch_pattern: null handle"); return IGX_ERR_ARG; }
    IGX_HIP(hipSetDevice(mp->ctx->device));
    hipStream_t st = mp->ctx->stream;
    if (indptr) IGX_HIP(hipMemcpyAsync(indptr, mp->d_indptr, (mp->nglobal + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (indices) IGX_HIP(hipMemcpyAsync(indices, mp->d_indices, mp->nnz * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    IGX_HIP(hipStreamSynchronize(st));
    return IGX_OK;
}

int igx_multipatch_zero(igx_multipatch *mp)
{
    if (!mp) { set_error("igx_multipatch_zero: null handle"); return IGX_ERR_ARG; }
    IGX_HIP(hipSetDevice(mp->ctx->device));
    hipStream_t st = mp->ctx->stream;
    ++mp->generation;
    // rows one local row reaches are overwritten by every scatter; only the sums need a zero to start from
    if (mp->nnz > mp->zero_from)
        IGX_HIP(hipMemsetAsync(mp->d_vals + mp->zero_from, 0, (mp->nnz - mp->zero_from) * sizeof(double), st));
    if (mp->nglobal > mp->vzero_from)
        IGX_HIP(hipMemsetAsync(mp->d_vec + mp->vzero_from, 0, (mp->nglobal - mp->vzero_from) * sizeof(double), st));
    return IGX_OK;
}

int igx_multipatch_scatter_patch(igx_multipatch *mp, int p, const igx_patch *src)
{
    if (!mp || !src) { set_error("igx_multipatch_scatter_patch: null argument"); return IGX_ERR_ARG; }
    if (p < 0 || p >= mp->np) { set_error("igx_multipatch_scatter_patch: patch %d out of range", p); return IGX_ERR_ARG; }
    const auto &P = mp->pp[p];
    if (src->ctx != mp->ctx || src->boxed || src->row_lo != 0 || src->nrows_total != P.n || src->row_hi != P.n || src->nnz != P.nnz) {
        set_error("igx_multipatch_scatter_patch: the source patch does not have the shape and nnz of patch %d (%d rows, %lld nnz)", p, P.n, P.nnz);
        return IGX_ERR_ARG;
    }
    if (!src->d_data) { set_error("igx_multipatch_scatter_patch: the source patch holds no assembled values"); return IGX_ERR_ARG; }
    IGX_HIP(hipSetDevice(mp->ctx->device));
    return run_scatter(mp, p, src->d_data);
}

int igx_multipatch_scatter_host(igx_multipatch *mp, int p, const double *vals)
{
    if (!mp || !vals) { set_error("igx_multipatch_scatter_host: null argument"); return IGX_ERR_ARG; }
    if (p < 0 || p >= mp->np) { set_error("igx_multipatch_scatter_host: patch %d out of range", p); return IGX_ERR_ARG; }
    IGX_HIP(hipSetDevice(mp->ctx->device));
    if (int rc = stage(mp, vals, (size_t)mp->pp[p].nnz)) return rc;
    return run_scatter(mp, p, mp->d_stage);
}

int igx_multipatch_scatter_vector(igx_multipatch *mp, int p, const double *b)
{
    if (!mp || !b) { set_error("igx_multipatch_scatter_vector: null argument"); return IGX_ERR_ARG; }
    if (p < 0 || p >= mp->np) { set_error("igx_multipatch_scatter_vector: patch %d out of range", p); return IGX_ERR_ARG; }
    IGX_HIP(hipSetDevice(mp->ctx->device));
    const auto &P = mp->pp[p];
    if (int rc = stage(mp, b, (size_t)P.n)) return rc;
    hipStream_t st = mp->ctx->stream;
    if (P.n) k_scatter_vec<<<(P.n + 255) / 256, 256, 0, st>>>(P.d_l2g, P.n, mp->d_contrib, mp->injective, mp->d_stage, mp->d_vec);
    IGX_HIP(hipGetLastError());
    IGX_HIP(hipStreamSynchronize(st));
    return IGX_OK;
}

int igx_multipatch_download(const igx_multipatch *mp, double *vals, double *vec)
{
    if (!mp) { set_error("igx_multipatch_download: null handle"); return IGX_ERR_ARG; }
    IGX_HIP(hipSetDevice(mp->ctx->device));
    hipStream_t st = mp->ctx->stream;
    if (vals) IGX_HIP(hipMemcpyAsync(vals, mp->d_vals, mp->nnz * sizeof(double), hipMemcpyDeviceToHost, st));
    if (vec) IGX_HIP(hipMemcpyAsync(vec, mp->d_vec, mp->nglobal * sizeof(double), hipMemcpyDeviceToHost, st));
    IGX_HIP(hipStreamSynchronize(st));
    {
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) { set_error("igx_multipatch_download: kernel failure: %s", hipGetErrorString(e)); return IGX_ERR_HIP; }
    }
    return IGX_OK;
}

int igx_multipatch_values_d(const igx_multipatch *mp, double *d_out)
{
    if (!mp || !d_out) { set_error("igx_multipatch_values_d: null argument"); return IGX_ERR_ARG; }
    IGX_HIP(hipSetDevice(mp->ctx->device));
    hipStream_t st = mp->ctx->stream;
    IGX_HIP(hipMemcpyAsync(d_out, mp->d_vals, mp->nnz * sizeof(double), hipMemcpyDeviceToDevice, st));
    IGX_HIP(hipStreamSynchronize(st));
    {
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) { set_error("igx_multipatch_values_d: kernel failure: %s", hipGetErrorString(e)); return IGX_ERR_HIP; }
    }
    return IGX_OK;
}

} // extern "C"
