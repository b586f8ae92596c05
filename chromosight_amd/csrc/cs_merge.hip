// cs_merge.hip -- the pixel-wise sum of resident pixel tables over the same bins (include/chromosight_hip.h cs_merge_count /
// cs_merge_fill): what `cooler merge` writes, restated.  The merged table holds one pixel for every (bin1, bin2) stored in at least
// one source, its count the sum of the sources' counts there; a pixel whose sum is 0 is not stored (cs_coarsen's rule).  Nothing
// is mirrored.
//
// Row r of the result is the union of up to kMaxSources sorted runs: row r of every source.  That is the shape of a coarse row in
// cs_coarsen.hip (the fine rows under it) with the identity as the column map, but the runs live in arrays of their own, with a
// value type of their own, and there are never more of them than a wave has lanes:
//
//   host                a device table of per-source descriptors (row pointers, columns, counts, dtype)
//   mg_rows_kernel<0>   one workgroup per row.  A tile is kTile columns from the smallest one any run has left (empty stretches are
//                       never visited).  One thread per source finds its run's pixels of the tile (the run's cursor, a lower bound
//                       for the tile's end); wave 0 scans the lengths; the workgroup then walks the concatenated ranges -- a long
//                       run is spread over all lanes -- and adds every count to the int64 accumulator of its column (integer LDS
//                       atomics: exact, so order-independent).  The accumulators that are not zero are the tile's pixels, counted
//                       through wave ballots (emit_tile, cs_table_rows.h: shared with cs_coarsen.hip).  The same pass checks every
//                       count (finite, non-negative, integer, below 2^53) and column (inside the table, not decreasing along a
//                       row) and reduces the grand total and the largest sum per workgroup (co_stats_kernel adds the workgroups
//                       up: no same-address global atomics).
//   exclusive scan      of the rows' pixel counts into the new row pointers (cs_merge_count ends here: the caller allocates the
//                       columns and counts at their exact size)
//   mg_rows_kernel<1>   the same walk; the ballots' prefix sums give every nonzero accumulator its place, in column order:
//                       consecutive lanes store to increasing, mostly consecutive addresses.  No store goes beyond the row's end in
//                       the caller's row pointers or the table's pixel count.
//
// Every output value is an exact integer sum written by one thread at a place fixed by the tables alone: the result is bitwise the
// same for any launch shape, order of the sources, context or device.  No float atomics.
#include <hipcub/hipcub.hpp>

#include "cs_api_internal.h"
#include "cs_table_rows.h"

using namespace csapi;

namespace {

constexpr int kMaxSources = 64;             // one lane of wave 0 per source
constexpr int kTile = 2048;                 // columns of an LDS tile: 16 KiB of accumulators + 5 KiB of tables, 7 workgroups per CU
constexpr int kWords = kTile / 64;          // ballot words of a tile

struct MgSource {
    const long long* indptr;
    const int* indices;
    const void* data;
    int dtype;                              // CS_F32 / CS_F64
    int reserved;
};

template <typename TO, bool WRITE>
__global__ __launch_bounds__(kCoThreads) void mg_rows_kernel(const MgSource* __restrict__ sources, int n_src, int n,
                                                              long long* __restrict__ row_count, const long long* __restrict__ out_indptr,
                                                              long long out_nnz, int* __restrict__ out_indices, TO* __restrict__ out_data,
                                                              CoStats* __restrict__ stats)
{
    __shared__ unsigned long long s_acc[kTile];
    __shared__ unsigned long long s_words[kWords];
    __shared__ MgSource s_src[kMaxSources];
    __shared__ long long s_cur[kMaxSources], s_end[kMaxSources];      // the runs' cursors and ends in the row at hand
    __shared__ long long s_lo[kMaxSources];
    __shared__ long long s_pre[kMaxSources + 1];
    __shared__ int s_wpre[kWords];
    __shared__ int s_next, s_maxc, s_total;
    const int tid = threadIdx.x, lane = tid & 63;
    unsigned long long bad = 0, sum_hi = 0, sum_lo = 0, vmax = 0;

    if (tid < n_src) s_src[tid] = sources[tid];
    for (int R = blockIdx.x; R < n; R += gridDim.x) {
        __syncthreads();
        if (tid == 0) s_next = kNoColumn;
        __syncthreads();
        if (tid < n_src) {
            const long long rs = s_src[tid].indptr[R], re = s_src[tid].indptr[R + 1];
            s_cur[tid] = rs;
            s_end[tid] = re;
            if (rs < re) atomicMin(&s_next, min(max(s_src[tid].indices[rs], 0), n - 1));
        }
        __syncthreads();
        int base = s_next;
        if (base == kNoColumn) {                               // the row is empty in every source
            if (!WRITE && tid == 0) row_count[R] = 0;
            continue;
        }
        const long long row_out = WRITE ? out_indptr[R] : 0;
        const long long row_end = WRITE ? min(out_indptr[R + 1], out_nnz) : 0;
        long long written = 0;
        while (base < n) {
            const int top = min(base + kTile, n);
            __syncthreads();
            if (tid == 0) {
                s_next = kNoColumn;
                s_maxc = base;
            }
            __syncthreads();
            // wave 0: every run's pixels of the tile, and the exclusive scan of their numbers
            if (tid < 64) {
                long long len = 0;
                if (tid < n_src) {
                    const int* __restrict__ indices = s_src[tid].indices;
                    const long long lo = s_cur[tid], re = s_end[tid];
                    long long hi = re;
                    if (lo < re) {
                        if (indices[re - 1] >= top) hi = lower_bound(indices, lo, re, top);
                        if (hi < re) atomicMin(&s_next, min(max(indices[hi], 0), n - 1));
                        if (hi > lo) atomicMax(&s_maxc, min(max(indices[hi - 1], 0), n - 1));
                    }
                    s_lo[tid] = lo;
                    s_cur[tid] = hi;
                    len = hi - lo;
                }
                long long inc = len;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const long long y = __shfl_up(inc, d);
                    if (lane >= d) inc += y;
                }
                s_pre[tid] = inc - len;
                if (tid == 63) s_pre[64] = inc;
            }
            __syncthreads();
            // only the columns the tile's pixels reach are cleared
            const int span = min(max(s_maxc - base + 1, 1), top - base);
            for (int c = tid; c < span; c += kCoThreads) s_acc[c] = 0;
            __syncthreads();
            const long long total = s_pre[64];
            for (long long p = tid; p < total; p += kCoThreads) {
                int a = 0, b = kMaxSources - 1;                // the last run whose range starts at or before p
                while (a < b) {
                    const int mid = (a + b + 1) >> 1;
                    if (s_pre[mid] <= p) a = mid;
                    else b = mid - 1;
                }
                const long long first = s_lo[a];
                const long long k = first + (p - s_pre[a]);
                const int* __restrict__ indices = s_src[a].indices;
                const int col = indices[k];
                // the value type is one per source: uniform over a run's stretch of the walk
                const double v = s_src[a].dtype == CS_F64 ? ((const double*)s_src[a].data)[k] : (double)((const float*)s_src[a].data)[k];
                const bool ok = v >= 0.0 && v < kMaxTotal && v == floor(v);
                const unsigned long long u = ok ? (unsigned long long)v : 0ull;
                const int c = col - base;
                if (!WRITE) {
                    if (!ok) bad |= 1;
                    if (k > first && indices[k - 1] > col) bad |= 2;
                    sum_hi += u >> 32;
                    sum_lo += u & 0xffffffffull;
                }
                if ((unsigned)col >= (unsigned)n || (unsigned)c >= (unsigned)span) {
                    bad |= 2;
                    continue;
                }
                if (u) atomicAdd(&s_acc[c], u);
            }
            __syncthreads();
            const int next = s_next;
            // the nonzero accumulators, in column order; no store beyond the row's end in the caller's row pointers
            written += emit_tile<kTile, TO, WRITE>(s_acc, s_words, s_wpre, &s_total, span, base, row_out + written, row_end, out_indices,
                                                   out_data, vmax);
            if (next < top) bad |= 2;                          // a row that is not sorted by column
            base = max(next, top);
        }
        if (!WRITE && tid == 0) row_count[R] = written;
    }
    if (!WRITE) {                                              // this workgroup's statistics: one plain store, no atomics
        __syncthreads();
        block_stats(bad, sum_hi, sum_lo, vmax, s_acc, &stats[blockIdx.x]);
    }
}

// the checks of both entries: the tables as descriptors, their common number of rows and whether any holds a pixel
int check_tables(cs_ctx* ctx, const char* who, const cs_csr* const* tables, int32_t n_tables, std::vector<MgSource>& src, int* n_rows,
                 bool* any)
{
    if (!tables) return fail(ctx, CS_ERR_INVALID, "%s: null argument", who);
    if (n_tables < 1) return fail(ctx, CS_ERR_INVALID, "%s: at least one table is needed, got %d", who, (int)n_tables);
    if (n_tables > kMaxSources) return fail(ctx, CS_ERR_UNSUPPORTED, "%s: more than %d tables in one call (%d)", who, kMaxSources, (int)n_tables);
    src.clear();
    *any = false;
    for (int s = 0; s < n_tables; ++s) {
        const cs_csr* g = tables[s];
        if (!g) return fail(ctx, CS_ERR_INVALID, "%s: null table %d", who, s);
        if (g->dtype != CS_F32 && g->dtype != CS_F64) return fail(ctx, CS_ERR_INVALID, "%s: bad dtype of table %d", who, s);
        if (g->n_rows < 0 || g->n_rows != g->n_cols || g->col0 != 0 || g->d_row_end || g->d_row_weight || g->d_col_weight)
            return fail(ctx, CS_ERR_INVALID, "%s takes whole-genome pixel tables (square, plain row pointers, no weights): table %d is not", who, s);
        if (g->n_rows != tables[0]->n_rows)
            return fail(ctx, CS_ERR_INVALID, "%s: table %d has %d bins, table 0 has %d", who, s, (int)g->n_rows, (int)tables[0]->n_rows);
        if (!g->d_indptr || g->nnz < 0 || (g->nnz > 0 && (!g->d_indices || !g->d_data)))
            return fail(ctx, CS_ERR_INVALID, "%s: null arrays of table %d", who, s);
        if (g->nnz >= (int64_t)std::numeric_limits<int>::max())
            return fail(ctx, CS_ERR_UNSUPPORTED, "%s: tables of 2^31 - 1 pixels or more", who);
        if (g->nnz > 0) *any = true;
        src.push_back(MgSource{(const long long*)g->d_indptr, g->d_indices, g->d_data, g->dtype, 0});
    }
    *n_rows = tables[0]->n_rows;
    return CS_OK;
}

int launch_grid(const cs_ctx* ctx, int n) { return (int)std::max(1LL, std::min<long long>(n, 32LL * std::max(ctx->n_cu, 1))); }

template <typename TO, bool WRITE>
void launch_rows(int grid, hipStream_t stream, const MgSource* d_src, int n_src, int n, long long* row_count, const long long* out_indptr,
                 long long out_nnz, void* out_indices, void* out_data, CoStats* stats)
{
    hipLaunchKernelGGL((mg_rows_kernel<TO, WRITE>), dim3(grid), dim3(kCoThreads), 0, stream, d_src, n_src, n, row_count, out_indptr,
                       out_nnz, (int*)out_indices, (TO*)out_data, stats);
}

}  // namespace

extern "C" {

int32_t cs_merge_tile_columns(void) { return kTile; }

int cs_merge_count(cs_ctx* ctx, void* stream_, const cs_csr* const* tables, int32_t n_tables, int64_t* d_out_indptr, int64_t* h_out_nnz,
                   int32_t* h_out_dtype)
{
    CS_ENTER(ctx);
    hipStream_t stream = (hipStream_t)stream_;
    if (!d_out_indptr || !h_out_nnz || !h_out_dtype) return fail(ctx, CS_ERR_INVALID, "cs_merge_count: null argument");
    std::vector<MgSource> src;
    int n = 0;
    bool any = false;
    if (int rc = check_tables(ctx, "cs_merge_count", tables, n_tables, src, &n, &any)) return rc;
    *h_out_nnz = 0;
    *h_out_dtype = CS_F32;
    if (!any) {
        CS_HIP(ctx, hipMemsetAsync(d_out_indptr, 0, ((size_t)n + 1) * sizeof(long long), stream));
        CS_HIP(ctx, hipStreamSynchronize(stream));
        return CS_OK;
    }

    CallBuffers Bf;
    MgSource* d_src = nullptr;
    long long* d_count = nullptr;
    CoStats* d_stats = nullptr;
    unsigned char* tmp = nullptr;
    size_t tmp_bytes = 0;
    CS_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, (const long long*)nullptr, (long long*)nullptr, n + 1, stream));
    CS_HIP(ctx, Bf.get(&tmp, tmp_bytes));
    CS_HIP(ctx, Bf.get(&d_src, src.size()));
    CS_HIP(ctx, Bf.get(&d_count, (size_t)n + 1));
    const int grid = launch_grid(ctx, n);
    CS_HIP(ctx, Bf.get(&d_stats, (size_t)grid + 1));         // one entry per workgroup of the count pass, then their reduction
    CS_HIP(ctx, hipMemcpyAsync(d_src, src.data(), src.size() * sizeof(MgSource), hipMemcpyHostToDevice, stream));
    CS_HIP(ctx, hipMemsetAsync(d_count + n, 0, sizeof(long long), stream));

    // 1. pixels per row, the validity of the counts and columns, the grand total and the largest sum
    launch_rows<double, false>(grid, stream, d_src, n_tables, n, d_count, nullptr, 0, nullptr, nullptr, d_stats);
    CS_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(co_stats_kernel, dim3(1), dim3(kCoThreads), 0, stream, d_stats, grid);
    CS_HIP(ctx, hipGetLastError());
    CoStats st;
    CS_HIP(ctx, hipMemcpyAsync(&st, d_stats + grid, sizeof(st), hipMemcpyDeviceToHost, stream));
    CS_HIP(ctx, hipStreamSynchronize(stream));
    if (st.bad & 2) return fail(ctx, CS_ERR_INVALID, "cs_merge: column bins must lie inside the table and be sorted within every row");
    if (st.bad & 1) return fail(ctx, CS_ERR_INVALID, "cs_merge: counts must be finite, non-negative integers");
    const unsigned __int128 total = ((unsigned __int128)st.sum_hi << 32) + st.sum_lo;
    if (total >= ((unsigned __int128)1 << 53)) return fail(ctx, CS_ERR_INVALID, "cs_merge: the counts sum to 2^53 or more");

    // 2. row pointers
    size_t bytes = tmp_bytes;
    CS_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(tmp, bytes, d_count, (long long*)d_out_indptr, n + 1, stream));
    long long h_nnz = 0;
    CS_HIP(ctx, hipMemcpyAsync(&h_nnz, (const long long*)d_out_indptr + n, sizeof(long long), hipMemcpyDeviceToHost, stream));
    CS_HIP(ctx, hipStreamSynchronize(stream));
    if (h_nnz < 0) return fail(ctx, CS_ERR_HIP, "cs_merge_count: %lld merged pixels", h_nnz);
    if (h_nnz >= (long long)std::numeric_limits<int>::max())
        return fail(ctx, CS_ERR_UNSUPPORTED, "cs_merge: a merged table of 2^31 - 1 pixels or more");
    *h_out_nnz = h_nnz;
    // float32 when every sum is below 2^24 (pipeline.DeviceCool's rule), else float64
    *h_out_dtype = st.vmax < (1ull << 24) ? CS_F32 : CS_F64;
    return CS_OK;
}

int cs_merge_fill(cs_ctx* ctx, void* stream_, const cs_csr* const* tables, int32_t n_tables, cs_csr* out)
{
    CS_ENTER(ctx);
    hipStream_t stream = (hipStream_t)stream_;
    if (!out) return fail(ctx, CS_ERR_INVALID, "cs_merge_fill: null argument");
    std::vector<MgSource> src;
    int n = 0;
    bool any = false;
    if (int rc = check_tables(ctx, "cs_merge_fill", tables, n_tables, src, &n, &any)) return rc;
    if (out->dtype != CS_F32 && out->dtype != CS_F64) return fail(ctx, CS_ERR_INVALID, "cs_merge_fill: bad output dtype");
    if (out->n_rows != n || out->n_cols != n || out->col0 != 0 || out->d_row_end || out->d_row_weight || out->d_col_weight)
        return fail(ctx, CS_ERR_INVALID, "cs_merge_fill: the output must be a plain table of the sources' %d bins", n);
    if (!out->d_indptr || out->nnz < 0 || (out->nnz > 0 && (!out->d_indices || !out->d_data)))
        return fail(ctx, CS_ERR_INVALID, "cs_merge_fill: null output arrays");
    if (out->nnz >= (int64_t)std::numeric_limits<int>::max())
        return fail(ctx, CS_ERR_UNSUPPORTED, "cs_merge: a merged table of 2^31 - 1 pixels or more");
    // the row pointers must be those of cs_merge_count for an output of this size
    long long h_nnz = -1;
    CS_HIP(ctx, hipMemcpyAsync(&h_nnz, (const long long*)out->d_indptr + n, sizeof(long long), hipMemcpyDeviceToHost, stream));
    CS_HIP(ctx, hipStreamSynchronize(stream));
    if (h_nnz != out->nnz)
        return fail(ctx, CS_ERR_INVALID, "cs_merge_fill: the row pointers end at %lld, the output holds %lld pixels", h_nnz, (long long)out->nnz);
    if (out->nnz == 0) return CS_OK;

    CallBuffers Bf;
    MgSource* d_src = nullptr;
    CS_HIP(ctx, Bf.get(&d_src, src.size()));
    CS_HIP(ctx, hipMemcpyAsync(d_src, src.data(), src.size() * sizeof(MgSource), hipMemcpyHostToDevice, stream));
    const int grid = launch_grid(ctx, n);
    if (out->dtype == CS_F32)
        launch_rows<float, true>(grid, stream, d_src, n_tables, n, nullptr, (const long long*)out->d_indptr, out->nnz, (void*)out->d_indices,
                                 (void*)out->d_data, nullptr);
    else
        launch_rows<double, true>(grid, stream, d_src, n_tables, n, nullptr, (const long long*)out->d_indptr, out->nnz, (void*)out->d_indices,
                                  (void*)out->d_data, nullptr);
    CS_HIP(ctx, hipGetLastError());
    CS_HIP(ctx, hipStreamSynchronize(stream));
    return CS_OK;
}

}  // extern "C"
