// cs_coarsen.hip -- coarsening of the resident pixel table on the device (include/chromosight_hip.h cs_coarsen): what
// `cooler coarsen -k factor` writes, restated.  Every chromosome's bins are regrouped `factor` at a time on their own
// (coarse(b) = off'[c] + (b - off[c]) / factor, the last coarse bin of a chromosome may be short), the stored pixels are grouped by
// (coarse(bin1), coarse(bin2)) and their counts summed.  Nothing is mirrored: an upper-triangle table stays one.
//
// A coarse row is the merge of the (at most `factor`) fine rows under it, which are one contiguous segment of the input table.
// coarse() is monotone, so every fine row is a sorted run of coarse columns; the runs are merged through LDS, a column tile at a
// time:
//
//   host                two small tables: fine bin -> coarse bin, coarse bin -> its first fine bin
//   co_rows_kernel<0>   one workgroup per coarse row.  A tile is kTile coarse columns from the smallest one any run has left (empty
//                       stretches are never visited).  One thread per fine row finds the row's pixels of the tile (a lower bound on
//                       either side; two loads when the row ends inside the tile); the workgroup then walks the concatenated ranges
//                       -- a heavy row is spread over all its lanes -- and adds every count to the int64 accumulator of its column
//                       (integer LDS atomics: exact, so order-independent).  The accumulators that are not zero are the tile's coarse
//                       pixels (counts are non-negative: no presence bits needed), counted through wave ballots.  The same pass
//                       checks every count (finite, non-negative, integer, below 2^53) and reduces the grand total and the largest sum
//                       per workgroup (co_stats_kernel adds the workgroups up: same-address global atomics would serialise).
//   exclusive scan      of the rows' pixel counts into the new row pointers
//   co_rows_kernel<1>   the same walk; the ballots' prefix sums give every nonzero accumulator its place, in column order:
//                       consecutive lanes store to increasing, mostly consecutive addresses.
//
// Every output value is an exact integer sum written by one thread at a place fixed by the table alone: the result is bitwise the
// same for any launch shape, context or device.  No float atomics.
#include <hipcub/hipcub.hpp>

#include "cs_api_internal.h"
#include "cs_table_rows.h"

using namespace csapi;

namespace {

constexpr int kTile = 2048;                 // coarse columns of an LDS tile: 16 KiB of accumulators, 7 workgroups per CU
constexpr int kRowChunk = kCoThreads;       // fine rows whose ranges are looked up at a time (one per thread)
constexpr int kWords = kTile / 64;          // ballot words of a tile

// coarse bin of a column (clamped: a column outside the table is reported by the count pass, never used as an index)
__device__ __forceinline__ int coarse_of(const int* __restrict__ cmap, int n, int col)
{
    return cmap[min(max(col, 0), n - 1)];
}

template <typename TV, typename TO, bool WRITE>
__global__ __launch_bounds__(kCoThreads) void co_rows_kernel(const long long* __restrict__ indptr, const int* __restrict__ indices,
                                                              const TV* __restrict__ data, int n, const int* __restrict__ cmap,
                                                              const int* __restrict__ cfirst, int n_coarse,
                                                              long long* __restrict__ row_count, const long long* __restrict__ out_indptr,
                                                              int* __restrict__ out_indices, TO* __restrict__ out_data,
                                                              CoStats* __restrict__ stats)
{
    __shared__ unsigned long long s_acc[kTile];
    __shared__ unsigned long long s_words[kWords];
    __shared__ long long s_lo[kRowChunk];
    __shared__ int s_len[kRowChunk];
    __shared__ int s_pre[kRowChunk + 1];
    __shared__ int s_wpre[kWords];
    __shared__ int s_next, s_maxc, s_total;
    const int tid = threadIdx.x;
    unsigned long long bad = 0, sum_hi = 0, sum_lo = 0, vmax = 0;

    for (int R = blockIdx.x; R < n_coarse; R += gridDim.x) {
        const int r0 = cfirst[R], r1 = cfirst[R + 1];
        if (indptr[r0] == indptr[r1]) {                    // no pixel under this coarse row
            if (!WRITE && tid == 0) row_count[R] = 0;
            continue;
        }
        const bool multi = r1 - r0 > kRowChunk;
        const long long row_out = WRITE ? out_indptr[R] : 0;
        long long written = 0;
        __syncthreads();
        if (tid == 0) s_next = kNoColumn;
        __syncthreads();
        for (int r = r0 + tid; r < r1; r += kCoThreads) {
            const long long rs = indptr[r];
            if (rs < indptr[r + 1]) atomicMin(&s_next, coarse_of(cmap, n, indices[rs]));
        }
        __syncthreads();
        int base = s_next;
        while (base < n_coarse) {
            const int top = min(base + kTile, n_coarse);
            const int f_lo = cfirst[base], f_hi = cfirst[top];
            __syncthreads();
            if (tid == 0) {
                s_next = kNoColumn;
                s_maxc = multi ? top - 1 : base;
            }
            // more fine rows than threads: their ranges come in chunks, the whole tile is cleared first
            if (multi)
                for (int c = tid; c < kTile; c += kCoThreads) s_acc[c] = 0;
            __syncthreads();
            int span = top - base;
            for (int c0 = r0; c0 < r1; c0 += kRowChunk) {
                const int m = min(kRowChunk, r1 - c0);
                int len = 0;
                if (tid < m) {
                    const long long rs = indptr[c0 + tid], re = indptr[c0 + tid + 1];
                    long long lo = rs, hi = re;
                    if (rs < re) {
                        if (indices[rs] < f_lo) lo = lower_bound(indices, rs, re, f_lo);
                        if (indices[re - 1] >= f_hi) hi = lower_bound(indices, lo, re, f_hi);
                        if (hi < re) atomicMin(&s_next, coarse_of(cmap, n, indices[hi]));
                        if (hi > lo) atomicMax(&s_maxc, coarse_of(cmap, n, indices[hi - 1]));
                    }
                    s_lo[tid] = lo;
                    len = (int)(hi - lo);
                }
                s_len[tid] = len;
                __syncthreads();
                if (tid < m) {
                    int before = 0;
                    for (int j = 0; j < tid; ++j) before += s_len[j];
                    s_pre[tid] = before;
                    if (tid == m - 1) s_pre[m] = before + len;
                }
                __syncthreads();
                if (!multi) {                              // one chunk: only the columns the tile's pixels reach are cleared
                    span = min(max(s_maxc - base + 1, 1), top - base);
                    for (int c = tid; c < span; c += kCoThreads) s_acc[c] = 0;
                    __syncthreads();
                }
                const int total = s_pre[m];
                for (int p = tid; p < total; p += kCoThreads) {
                    int a = 0, b = m - 1;                  // the last row whose range starts at or before p
                    while (a < b) {
                        const int mid = (a + b + 1) >> 1;
                        if (s_pre[mid] <= p) a = mid;
                        else b = mid - 1;
                    }
                    const long long k = s_lo[a] + (p - s_pre[a]);
                    const int col = indices[k];
                    const double v = (double)data[k];
                    const bool ok = v >= 0.0 && v < kMaxTotal && v == floor(v);
                    const unsigned long long u = ok ? (unsigned long long)v : 0ull;
                    const int c = coarse_of(cmap, n, col) - base;
                    if (!WRITE) {
                        if (!ok) bad |= 1;
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
            }
            const int next = s_next;
            // the nonzero accumulators, in column order (the output has room for every input pixel)
            written += emit_tile<kTile, TO, WRITE>(s_acc, s_words, s_wpre, &s_total, span, base, row_out + written, kNoLimit,
                                                   out_indices, out_data, vmax);
            if (next < top) bad |= 2;                      // a row that is not sorted by column
            base = max(next, top);
        }
        if (!WRITE && tid == 0) row_count[R] = written;
    }
    if (!WRITE) {                                          // this workgroup's statistics: one plain store, no atomics
        __syncthreads();
        block_stats(bad, sum_hi, sum_lo, vmax, s_acc, &stats[blockIdx.x]);
    }
}

template <typename TV, typename TO, bool WRITE>
void launch_rows(int grid, hipStream_t stream, const cs_csr* g, const int* cmap, const int* cfirst, int n_coarse, long long* row_count,
                 const cs_csr* out, CoStats* stats)
{
    hipLaunchKernelGGL((co_rows_kernel<TV, TO, WRITE>), dim3(grid), dim3(kCoThreads), 0, stream, (const long long*)g->d_indptr,
                       g->d_indices, (const TV*)g->d_data, g->n_rows, cmap, cfirst, n_coarse, row_count,
                       (const long long*)out->d_indptr, (int*)out->d_indices, (TO*)out->d_data, stats);
}

}  // namespace

extern "C" {

int cs_coarsen(cs_ctx* ctx, void* stream_, const cs_csr* g, const int64_t* chrom_offsets, int32_t n_chrom, int32_t factor, cs_csr* out,
               int64_t* h_out_nnz)
{
    CS_ENTER(ctx);
    hipStream_t stream = (hipStream_t)stream_;
    if (!g || !out || !h_out_nnz || !chrom_offsets) return fail(ctx, CS_ERR_INVALID, "cs_coarsen: null argument");
    if (factor < 1) return fail(ctx, CS_ERR_INVALID, "cs_coarsen: factor must be at least 1, got %d", (int)factor);
    if (g->dtype != CS_F32 && g->dtype != CS_F64) return fail(ctx, CS_ERR_INVALID, "cs_coarsen: bad table dtype");
    if (g->n_rows < 0 || g->n_rows != g->n_cols || g->col0 != 0 || g->d_row_end || g->d_row_weight || g->d_col_weight)
        return fail(ctx, CS_ERR_INVALID, "cs_coarsen takes the whole-genome pixel table (square, plain row pointers, no weights)");
    if (!g->d_indptr || g->nnz < 0 || (g->nnz > 0 && (!g->d_indices || !g->d_data)))
        return fail(ctx, CS_ERR_INVALID, "cs_coarsen: null table arrays");
    if (!out->d_indptr || (g->nnz > 0 && (!out->d_indices || !out->d_data)))
        return fail(ctx, CS_ERR_INVALID, "cs_coarsen: null output arrays");
    if (g->nnz >= (int64_t)std::numeric_limits<int>::max())
        return fail(ctx, CS_ERR_UNSUPPORTED, "cs_coarsen: tables of 2^31 - 1 pixels or more");
    const int n = g->n_rows;
    if (n_chrom < 1 || chrom_offsets[0] != 0 || chrom_offsets[n_chrom] != n)
        return fail(ctx, CS_ERR_INVALID, "cs_coarsen: %d chromosome offsets must run from 0 to the %d bins", (int)n_chrom + 1, n);
    for (int c = 0; c < n_chrom; ++c)
        if (chrom_offsets[c + 1] < chrom_offsets[c]) return fail(ctx, CS_ERR_INVALID, "cs_coarsen: decreasing chromosome offsets");
    // fine bin -> coarse bin, coarse bin -> its first fine bin (one more entry: n)
    const long long k = factor;
    std::vector<int> cmap((size_t)n), cfirst;
    cfirst.reserve((size_t)(n / k) + (size_t)n_chrom + 1);
    for (int c = 0; c < n_chrom; ++c) {
        const long long s = chrom_offsets[c], m = chrom_offsets[c + 1] - s;
        const int at = (int)cfirst.size();
        for (long long b = 0; b < m; ++b) cmap[(size_t)(s + b)] = at + (int)(b / k);
        for (long long b = 0; b < m; b += k) cfirst.push_back((int)(s + b));
    }
    const int nc = (int)cfirst.size();
    cfirst.push_back(n);
    out->n_rows = out->n_cols = nc;
    out->col0 = 0;
    out->d_row_end = nullptr;
    out->d_row_weight = out->d_col_weight = nullptr;
    out->nnz = 0;
    out->dtype = CS_F32;
    *h_out_nnz = 0;
    const long long nnz = g->nnz;
    if (nnz == 0) {
        CS_HIP(ctx, hipMemsetAsync((void*)out->d_indptr, 0, ((size_t)nc + 1) * sizeof(long long), stream));
        CS_HIP(ctx, hipStreamSynchronize(stream));
        return CS_OK;
    }

    CallBuffers Bf;
    int *d_cmap = nullptr, *d_cfirst = nullptr;
    long long* d_count = nullptr;
    CoStats* d_stats = nullptr;
    unsigned char* tmp = nullptr;
    size_t tmp_bytes = 0;
    CS_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, (const long long*)nullptr, (long long*)nullptr, nc + 1, stream));
    CS_HIP(ctx, Bf.get(&tmp, tmp_bytes));
    CS_HIP(ctx, Bf.get(&d_cmap, (size_t)n));
    CS_HIP(ctx, Bf.get(&d_cfirst, (size_t)nc + 1));
    CS_HIP(ctx, Bf.get(&d_count, (size_t)nc + 1));
    const int grid = (int)std::max(1LL, std::min<long long>(nc, 32LL * std::max(ctx->n_cu, 1)));
    CS_HIP(ctx, Bf.get(&d_stats, (size_t)grid + 1));         // one entry per workgroup of the count pass, then their reduction
    CS_HIP(ctx, hipMemcpyAsync(d_cmap, cmap.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, stream));
    CS_HIP(ctx, hipMemcpyAsync(d_cfirst, cfirst.data(), ((size_t)nc + 1) * sizeof(int), hipMemcpyHostToDevice, stream));
    CS_HIP(ctx, hipMemsetAsync(d_count + nc, 0, sizeof(long long), stream));

    // 1. pixels per coarse row, the validity of the counts, their total and the largest sum
    if (g->dtype == CS_F64) launch_rows<double, double, false>(grid, stream, g, d_cmap, d_cfirst, nc, d_count, out, d_stats);
    else launch_rows<float, double, false>(grid, stream, g, d_cmap, d_cfirst, nc, d_count, out, d_stats);
    CS_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(co_stats_kernel, dim3(1), dim3(kCoThreads), 0, stream, d_stats, grid);
    CS_HIP(ctx, hipGetLastError());
    CoStats st;
    CS_HIP(ctx, hipMemcpyAsync(&st, d_stats + grid, sizeof(st), hipMemcpyDeviceToHost, stream));
    CS_HIP(ctx, hipStreamSynchronize(stream));
    if (st.bad & 2) return fail(ctx, CS_ERR_INVALID, "cs_coarsen: column bins must lie inside the table and be sorted within every row");
    if (st.bad & 1) return fail(ctx, CS_ERR_INVALID, "cs_coarsen: counts must be finite, non-negative integers");
    const unsigned __int128 total = ((unsigned __int128)st.sum_hi << 32) + st.sum_lo;
    if (total >= ((unsigned __int128)1 << 53)) return fail(ctx, CS_ERR_INVALID, "cs_coarsen: the counts sum to 2^53 or more");

    // 2. row pointers
    size_t bytes = tmp_bytes;
    CS_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(tmp, bytes, d_count, (long long*)out->d_indptr, nc + 1, stream));
    long long h_nnz = 0;
    CS_HIP(ctx, hipMemcpyAsync(&h_nnz, (const long long*)out->d_indptr + nc, sizeof(long long), hipMemcpyDeviceToHost, stream));
    CS_HIP(ctx, hipStreamSynchronize(stream));
    if (h_nnz < 0 || h_nnz > nnz) return fail(ctx, CS_ERR_HIP, "cs_coarsen: %lld coarse pixels from %lld", h_nnz, nnz);

    // 3. the coarse pixels: float32 when every sum is below 2^24 (pipeline.DeviceCool's rule), else float64
    const int dtype = st.vmax < (1ull << 24) ? CS_F32 : CS_F64;
    if (g->dtype == CS_F64) {
        if (dtype == CS_F32) launch_rows<double, float, true>(grid, stream, g, d_cmap, d_cfirst, nc, d_count, out, d_stats);
        else launch_rows<double, double, true>(grid, stream, g, d_cmap, d_cfirst, nc, d_count, out, d_stats);
    } else {
        if (dtype == CS_F32) launch_rows<float, float, true>(grid, stream, g, d_cmap, d_cfirst, nc, d_count, out, d_stats);
        else launch_rows<float, double, true>(grid, stream, g, d_cmap, d_cfirst, nc, d_count, out, d_stats);
    }
    CS_HIP(ctx, hipGetLastError());
    CS_HIP(ctx, hipStreamSynchronize(stream));
    out->nnz = h_nnz;
    out->dtype = dtype;
    *h_out_nnz = h_nnz;
    return CS_OK;
}

}  // extern "C"
