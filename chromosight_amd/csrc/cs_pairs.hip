// cs_pairs.hip -- read pairs binned into a pixel table on the device (include/chromosight_hip.h cs_pairs_count / cs_pairs_fill):
// what `cooler cload pairs` writes, restated.  A pair is (chromosome id, position) twice; a side whose id is -1 (a chromosome that
// is not part of the genome) drops the pair, an id outside [-1, n_chrom) or a position outside its chromosome refuses the whole
// chunk.  The genome bin of a side is chrom_offset[c] + pos0 / binsize; a pair whose bin1 > bin2 is reflected; the table holds one
// pixel per distinct (bin1, bin2), its count the number of pairs there.
//
//   pr_bin_kernel       one thread per pair: validates, bins and reflects it and writes the packed key (bin1 << b) | bin2, with
//                       b = bits(n_bins - 1); a dropped pair gets 1 << 2b, which sorts behind every pixel.  The division by the bin
//                       size is a multiplication by its float64 reciprocal with one correction step either way (a quotient below 2^31
//                       is never further off), no 64-bit hardware division.  Dropped and refused pairs are counted per lane, reduced
//                       per wave and added with one integer atomic per wave; the first refused index is an atomic minimum.
//   radix sort          of the keys (hipcub::DeviceRadixSort), over the 2b + 1 bits in use
//   pr_runs_kernel<0>   a workgroup covers kBlockPairs sorted keys, a wave kWavePairs consecutive ones, 64 at a time: the heads of the
//                       runs (a key that differs from the one before it) as wave ballots, kept in scalar registers.  Per workgroup:
//                       its number of heads and the position of its last one.
//   two scans           over the workgroups: heads in front of each (the pixels in front of it), the last head in front of each
//   pr_runs_kernel<1>   the same ballots; a lane's pixel is the heads at or before it, its run's start the last head at or before it
//                       (the carries of the scans, then popcount / leading zeros of the ballot): the last pair of a run knows the run's
//                       length -- the largest decides the dtype (one integer atomic maximum per workgroup) -- and the last pair of a row
//                       stores the pixels up to and including its row at mark[row + 1].  An inclusive maximum scan over the marks
//                       (rows without pixels hold 0) gives the row pointers.  cs_pairs_count ends here.
//   pr_runs_kernel<2>   cs_pairs_fill: the same walk; the last pair of a run stores the run's column bin and length at the run's
//                       pixel, nothing at or beyond out->nnz.
//
// Every stored value is an integer fixed by the multiset of the pairs alone, written by one thread at a place fixed by the sorted
// keys: the table is bitwise the same for every order of the pairs, launch shape, context and device.  Integer atomics only.
#include <hipcub/hipcub.hpp>

#include "cs_api_internal.h"
#include "cs_table_rows.h"

using namespace csapi;

namespace {

constexpr int kPrThreads = 256;
constexpr int kPrIters = 8;                                     // stretches of 64 keys per wave
constexpr int kWavePairs = 64 * kPrIters;
constexpr int kBlockPairs = (kPrThreads / 64) * kWavePairs;      // 2048: cs_pairs_block_pairs()
constexpr unsigned long long kNoIndex = ~0ull;

struct PairStats {
    unsigned long long dropped, refused, first_refused;       // pr_bin_kernel
    unsigned long long longest;                               // pr_runs_kernel<1>: the largest count
};

// bits(n - 1): the width of a bin in a key
int key_bits(long long n_bins)
{
    int b = 0;
    while (b < 63 && (1LL << b) < n_bins) ++b;
    return b;
}

enum { kSideBinned = 0, kSideDropped = 1, kSideRefused = 2 };

// one side of a pair: its genome bin.  u < len and len / binsize < 2^31, so the float64 estimate of the quotient (relative error of a
// few 2^-53) is off by at most one after truncation.
__device__ __forceinline__ int side_bin(int c, long long pos, int n_chrom, const long long* __restrict__ chrom_off,
                                        const long long* __restrict__ chrom_len, long long binsize, double inv, unsigned long long shift,
                                        long long* bin)
{
    if (c == -1) return kSideDropped;
    if (c < -1 || c >= n_chrom) return kSideRefused;
    const unsigned long long u = (unsigned long long)pos - shift;           // a position below the first wraps to a huge one
    if (u >= (unsigned long long)chrom_len[c]) return kSideRefused;
    long long q = (long long)((double)u * inv);
    const long long r = (long long)u - q * binsize;
    if (r < 0) --q;
    else if (r >= binsize) ++q;
    *bin = chrom_off[c] + q;
    return kSideBinned;
}

__global__ __launch_bounds__(kPrThreads) void pr_bin_kernel(const int* __restrict__ chrom1, const long long* __restrict__ pos1,
                                                            const int* __restrict__ chrom2, const long long* __restrict__ pos2, long long n,
                                                            const long long* __restrict__ chrom_off, const long long* __restrict__ chrom_len,
                                                            int n_chrom, long long binsize, double inv, unsigned long long shift, int b,
                                                            unsigned long long* __restrict__ keys, PairStats* __restrict__ stats)
{
    const unsigned long long drop_key = 1ull << (2 * b);
    unsigned long long dropped = 0, refused = 0, first = kNoIndex;
    const long long stride = (long long)gridDim.x * kPrThreads;
    for (long long i = (long long)blockIdx.x * kPrThreads + threadIdx.x; i < n; i += stride) {
        long long b1 = 0, b2 = 0;
        const int s1 = side_bin(chrom1[i], pos1[i], n_chrom, chrom_off, chrom_len, binsize, inv, shift, &b1);
        const int s2 = side_bin(chrom2[i], pos2[i], n_chrom, chrom_off, chrom_len, binsize, inv, shift, &b2);
        unsigned long long key = drop_key;
        if (s1 == kSideRefused || s2 == kSideRefused) {
            ++refused;
            first = min(first, (unsigned long long)i);
        } else if (s1 == kSideDropped || s2 == kSideDropped) {
            ++dropped;
        } else {
            key = ((unsigned long long)min(b1, b2) << b) | (unsigned long long)max(b1, b2);
        }
        keys[i] = key;
    }
    // one atomic per wave and counter, and only where there is something to report
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        dropped += __shfl_down(dropped, d);
        refused += __shfl_down(refused, d);
        first = min(first, __shfl_down(first, d));
    }
    if ((threadIdx.x & 63) == 0) {
        if (dropped) atomicAdd(&stats->dropped, dropped);
        if (refused) {
            atomicAdd(&stats->refused, refused);
            atomicMin(&stats->first_refused, first);
        }
    }
}

// MODE 0: blk_heads / blk_last receive the workgroup's number of heads and the position of its last head (-1: none).
// MODE 1, 2: they hold the exclusive scans of those (sum; maximum from -1).
template <int MODE, typename TO>
__global__ __launch_bounds__(kPrThreads) void pr_runs_kernel(const unsigned long long* __restrict__ keys, long long n, int b, long long n_bins,
                                                             long long* __restrict__ blk_heads, long long* __restrict__ blk_last,
                                                             long long* __restrict__ mark, PairStats* __restrict__ stats, long long out_nnz,
                                                             int* __restrict__ out_indices, TO* __restrict__ out_data)
{
    __shared__ long long s_heads[kPrThreads / 64], s_last[kPrThreads / 64];
    __shared__ unsigned long long s_longest[kPrThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long drop_key = 1ull << (2 * b);
    const long long seg = (long long)blockIdx.x * kBlockPairs + (long long)wave * kWavePairs;
    unsigned long long key[kPrIters];
    unsigned long long heads[kPrIters], tails[kPrIters], row_ends[kPrIters];      // ballots: the same in every lane
    long long w_heads = 0, w_last = -1;
#pragma unroll
    for (int j = 0; j < kPrIters; ++j) {
        const long long i = seg + 64 * j + lane;
        const unsigned long long k = i < n ? keys[i] : drop_key;
        unsigned long long before = __shfl_up(k, 1);
        if (lane == 0) before = (i > 0 && i - 1 < n) ? keys[i - 1] : drop_key;
        const bool valid = k < drop_key;
        heads[j] = __ballot(valid && (i == 0 || before != k));
        key[j] = k;
        if (MODE != 0) {
            unsigned long long after = __shfl_down(k, 1);
            if (lane == 63) after = i + 1 < n ? keys[i + 1] : drop_key;
            const bool tail = valid && after != k;
            tails[j] = __ballot(tail);
            row_ends[j] = __ballot(tail && (after >= drop_key || (after >> b) != (k >> b)));
        }
        w_heads += __popcll(heads[j]);
        if (heads[j]) w_last = seg + 64 * j + 63 - __clzll((long long)heads[j]);
    }
    if (lane == 0) {
        s_heads[wave] = w_heads;
        s_last[wave] = w_last;
    }
    __syncthreads();
    if (MODE == 0) {
        if (threadIdx.x == 0) {
            long long total = 0, last = -1;
            for (int w = 0; w < kPrThreads / 64; ++w) {
                total += s_heads[w];
                last = max(last, s_last[w]);
            }
            blk_heads[blockIdx.x] = total;
            blk_last[blockIdx.x] = last;
        }
        return;
    }
    long long rank = blk_heads[blockIdx.x], start = blk_last[blockIdx.x];          // the heads, and the last head, before this wave
    for (int w = 0; w < wave; ++w) {
        rank += s_heads[w];
        start = max(start, s_last[w]);
    }
    const unsigned long long col_mask = (1ull << b) - 1ull;
    unsigned long long longest = 0;
#pragma unroll
    for (int j = 0; j < kPrIters; ++j) {
        const long long i = seg + 64 * j + lane;
        const unsigned long long upto = heads[j] & (~0ull >> (63 - lane));          // the heads at or before this lane
        if ((tails[j] >> lane) & 1ull) {
            const long long pixels = rank + __popcll(upto);                         // ... up to and including this run
            const long long from = upto ? seg + 64 * j + 63 - __clzll((long long)upto) : start;
            const unsigned long long len = (unsigned long long)(i - from + 1);
            if (MODE == 1) {
                longest = max(longest, len);
                const unsigned long long row = key[j] >> b;
                if (((row_ends[j] >> lane) & 1ull) && row < (unsigned long long)n_bins) mark[row + 1] = pixels;
            } else {
                const long long at = pixels - 1;
                if (at >= 0 && at < out_nnz) {
                    out_indices[at] = (int)(key[j] & col_mask);
                    out_data[at] = (TO)len;
                }
            }
        }
        rank += __popcll(heads[j]);
        if (heads[j]) start = seg + 64 * j + 63 - __clzll((long long)heads[j]);
    }
    if (MODE == 1) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) longest = max(longest, __shfl_down(longest, d));
        if (lane == 0) s_longest[wave] = longest;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < kPrThreads / 64; ++w) longest = max(longest, s_longest[w]);
            if (longest) atomicMax(&stats->longest, longest);
        }
    }
}

// the first pass over the sorted keys and the scans over its workgroups: on return d_heads / d_last are what pr_runs_kernel<1, 2> read
// and *h_pixels is the number of runs
int run_carries(cs_ctx* ctx, hipStream_t stream, CallBuffers& Bf, const unsigned long long* d_keys, long long n, int b, long long n_bins,
                int blocks, long long** d_heads, long long** d_last, long long* h_pixels)
{
    long long *tot_heads = nullptr, *tot_last = nullptr;
    unsigned char* tmp = nullptr;
    size_t sum_bytes = 0, max_bytes = 0;
    CS_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, sum_bytes, (const long long*)nullptr, (long long*)nullptr, blocks + 1, stream));
    CS_HIP(ctx, hipcub::DeviceScan::ExclusiveScan(nullptr, max_bytes, (const long long*)nullptr, (long long*)nullptr, hipcub::Max(), (long long)-1,
                                                  blocks, stream));
    size_t tmp_bytes = std::max(sum_bytes, max_bytes);
    CS_HIP(ctx, Bf.get(&tmp, tmp_bytes));
    CS_HIP(ctx, Bf.get(&tot_heads, (size_t)blocks + 1));
    CS_HIP(ctx, Bf.get(&tot_last, (size_t)blocks));
    CS_HIP(ctx, Bf.get(d_heads, (size_t)blocks + 1));
    CS_HIP(ctx, Bf.get(d_last, (size_t)blocks));
    CS_HIP(ctx, hipMemsetAsync(tot_heads + blocks, 0, sizeof(long long), stream));
    hipLaunchKernelGGL((pr_runs_kernel<0, float>), dim3(blocks), dim3(kPrThreads), 0, stream, d_keys, n, b, n_bins, tot_heads, tot_last, nullptr,
                       nullptr, 0, nullptr, nullptr);
    CS_HIP(ctx, hipGetLastError());
    size_t bytes = tmp_bytes;
    CS_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(tmp, bytes, tot_heads, *d_heads, blocks + 1, stream));
    bytes = tmp_bytes;
    CS_HIP(ctx, hipcub::DeviceScan::ExclusiveScan(tmp, bytes, tot_last, *d_last, hipcub::Max(), (long long)-1, blocks, stream));
    CS_HIP(ctx, hipMemcpyAsync(h_pixels, *d_heads + blocks, sizeof(long long), hipMemcpyDeviceToHost, stream));
    CS_HIP(ctx, hipStreamSynchronize(stream));
    return CS_OK;
}

int check_count(cs_ctx* ctx, const char* who, long long n)
{
    if (n < 0) return fail(ctx, CS_ERR_INVALID, "%s: %lld pairs", who, n);
    if (n >= (long long)std::numeric_limits<int>::max()) return fail(ctx, CS_ERR_UNSUPPORTED, "%s: chunks of 2^31 - 1 pairs or more (%lld)", who, n);
    return CS_OK;
}

}  // namespace

extern "C" {

int32_t cs_pairs_block_pairs(void) { return kBlockPairs; }

int cs_pairs_count(cs_ctx* ctx, void* stream_, const int32_t* d_chrom1, const int64_t* d_pos1, const int32_t* d_chrom2, const int64_t* d_pos2,
                   int64_t n_pairs, const int64_t* h_chrom_offsets, const int64_t* h_chrom_lengths, int32_t n_chrom, int64_t binsize,
                   int32_t zero_based, int64_t* d_keys, int64_t* d_out_indptr, int64_t* h_out_nnz, int32_t* h_out_dtype, int64_t* h_out_dropped)
{
    CS_ENTER(ctx);
    hipStream_t stream = (hipStream_t)stream_;
    if (!h_chrom_offsets || !h_chrom_lengths || !d_out_indptr || !h_out_nnz || !h_out_dtype || !h_out_dropped)
        return fail(ctx, CS_ERR_INVALID, "cs_pairs_count: null argument");
    if (int rc = check_count(ctx, "cs_pairs_count", n_pairs)) return rc;
    if (n_pairs > 0 && (!d_chrom1 || !d_pos1 || !d_chrom2 || !d_pos2 || !d_keys)) return fail(ctx, CS_ERR_INVALID, "cs_pairs_count: null argument");
    if (n_chrom < 0 || binsize < 1) return fail(ctx, CS_ERR_INVALID, "cs_pairs_count: %d chromosomes, bins of %lld bp", (int)n_chrom, (long long)binsize);
    if (h_chrom_offsets[0] != 0) return fail(ctx, CS_ERR_INVALID, "cs_pairs_count: chromosome offsets must start at 0");
    for (int c = 0; c < n_chrom; ++c) {
        const long long len = h_chrom_lengths[c];
        if (len < 1) return fail(ctx, CS_ERR_INVALID, "cs_pairs_count: chromosome %d is %lld bp long", c, len);
        const long long bins = len / binsize + (len % binsize != 0);
        if (h_chrom_offsets[c + 1] - h_chrom_offsets[c] != bins)
            return fail(ctx, CS_ERR_INVALID, "cs_pairs_count: chromosome %d of %lld bp has %lld bins of %lld bp, its offsets say %lld", c, len, bins,
                        (long long)binsize, (long long)(h_chrom_offsets[c + 1] - h_chrom_offsets[c]));
        if (h_chrom_offsets[c + 1] >= (long long)std::numeric_limits<int>::max())
            return fail(ctx, CS_ERR_UNSUPPORTED, "cs_pairs_count: genomes of 2^31 - 1 bins or more");
    }
    const long long n_bins = h_chrom_offsets[n_chrom];
    const int b = key_bits(n_bins);
    *h_out_nnz = 0;
    *h_out_dtype = CS_F32;
    *h_out_dropped = 0;
    if (n_pairs == 0) {
        CS_HIP(ctx, hipMemsetAsync(d_out_indptr, 0, ((size_t)n_bins + 1) * sizeof(long long), stream));
        CS_HIP(ctx, hipStreamSynchronize(stream));
        return CS_OK;
    }

    CallBuffers Bf;
    PairStats* d_stats = nullptr;
    CS_HIP(ctx, Bf.get(&d_stats, 1));
    PairStats st = {0, 0, kNoIndex, 0};
    CS_HIP(ctx, hipMemcpyAsync(d_stats, &st, sizeof(st), hipMemcpyHostToDevice, stream));
    unsigned long long* keys = (unsigned long long*)d_keys;
    {
        // 1. keys, unsorted, in a buffer of this step; 2. sorted into the caller's
        CallBuffers Sort;
        long long* d_geo = nullptr;
        unsigned long long* d_raw = nullptr;
        unsigned char* tmp = nullptr;
        size_t tmp_bytes = 0;
        CS_HIP(ctx, hipcub::DeviceRadixSort::SortKeys(nullptr, tmp_bytes, (const unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                                      (int)n_pairs, 0, 2 * b + 1, stream));
        CS_HIP(ctx, Sort.get(&d_geo, 2 * (size_t)n_chrom + 1));
        CS_HIP(ctx, Sort.get(&d_raw, (size_t)n_pairs));
        CS_HIP(ctx, Sort.get(&tmp, tmp_bytes));
        CS_HIP(ctx, hipMemcpyAsync(d_geo, h_chrom_offsets, ((size_t)n_chrom + 1) * sizeof(long long), hipMemcpyHostToDevice, stream));
        if (n_chrom > 0)
            CS_HIP(ctx, hipMemcpyAsync(d_geo + n_chrom + 1, h_chrom_lengths, (size_t)n_chrom * sizeof(long long), hipMemcpyHostToDevice, stream));
        const int grid = (int)std::max(1LL, std::min<long long>((n_pairs + kPrThreads - 1) / kPrThreads, 8LL * std::max(ctx->n_cu, 1)));
        hipLaunchKernelGGL(pr_bin_kernel, dim3(grid), dim3(kPrThreads), 0, stream, d_chrom1, (const long long*)d_pos1, d_chrom2,
                           (const long long*)d_pos2, (long long)n_pairs, d_geo, d_geo + n_chrom + 1, (int)n_chrom, (long long)binsize,
                           1.0 / (double)binsize, zero_based ? 0ull : 1ull, b, d_raw, d_stats);
        CS_HIP(ctx, hipGetLastError());
        CS_HIP(ctx, hipMemcpyAsync(&st, d_stats, sizeof(st), hipMemcpyDeviceToHost, stream));
        CS_HIP(ctx, hipStreamSynchronize(stream));
        if (st.refused)
            return fail(ctx, CS_ERR_INVALID,
                        "cs_pairs_count: %llu of %lld pairs refused (a chromosome id outside [-1, %d) or a position outside its chromosome); "
                        "the first is pair %llu of the chunk",
                        st.refused, (long long)n_pairs, (int)n_chrom, st.first_refused);
        CS_HIP(ctx, hipcub::DeviceRadixSort::SortKeys(tmp, tmp_bytes, d_raw, keys, (int)n_pairs, 0, 2 * b + 1, stream));
        CS_HIP(ctx, hipStreamSynchronize(stream));
    }

    // 3. runs: their number, the longest, the rows' ends
    const int blocks = (int)((n_pairs + kBlockPairs - 1) / kBlockPairs);
    long long *d_heads = nullptr, *d_last = nullptr, *d_mark = nullptr;
    long long pixels = 0;
    if (int rc = run_carries(ctx, stream, Bf, keys, n_pairs, b, n_bins, blocks, &d_heads, &d_last, &pixels)) return rc;
    unsigned char* tmp = nullptr;
    size_t tmp_bytes = 0;
    CS_HIP(ctx, hipcub::DeviceScan::InclusiveScan(nullptr, tmp_bytes, (const long long*)nullptr, (long long*)nullptr, hipcub::Max(),
                                                  (int)(n_bins + 1), stream));
    CS_HIP(ctx, Bf.get(&tmp, tmp_bytes));
    CS_HIP(ctx, Bf.get(&d_mark, (size_t)n_bins + 1));
    CS_HIP(ctx, hipMemsetAsync(d_mark, 0, ((size_t)n_bins + 1) * sizeof(long long), stream));
    hipLaunchKernelGGL((pr_runs_kernel<1, float>), dim3(blocks), dim3(kPrThreads), 0, stream, keys, (long long)n_pairs, b, n_bins, d_heads, d_last,
                       d_mark, d_stats, 0, nullptr, nullptr);
    CS_HIP(ctx, hipGetLastError());
    // 4. row pointers: a row without pixels ends where the one before it does
    CS_HIP(ctx, hipcub::DeviceScan::InclusiveScan(tmp, tmp_bytes, d_mark, (long long*)d_out_indptr, hipcub::Max(), (int)(n_bins + 1), stream));
    CS_HIP(ctx, hipMemcpyAsync(&st, d_stats, sizeof(st), hipMemcpyDeviceToHost, stream));
    CS_HIP(ctx, hipStreamSynchronize(stream));
    if (pixels < 0 || pixels > n_pairs) return fail(ctx, CS_ERR_HIP, "cs_pairs_count: %lld pixels from %lld pairs", pixels, (long long)n_pairs);
    *h_out_nnz = pixels;
    *h_out_dtype = st.longest < (1ull << 24) ? CS_F32 : CS_F64;      // pipeline.DeviceCool's rule
    *h_out_dropped = (int64_t)st.dropped;
    return CS_OK;
}

int cs_pairs_fill(cs_ctx* ctx, void* stream_, const int64_t* d_keys, int64_t n_pairs, cs_csr* out)
{
    CS_ENTER(ctx);
    hipStream_t stream = (hipStream_t)stream_;
    if (!out) return fail(ctx, CS_ERR_INVALID, "cs_pairs_fill: null argument");
    if (int rc = check_count(ctx, "cs_pairs_fill", n_pairs)) return rc;
    if (out->dtype != CS_F32 && out->dtype != CS_F64) return fail(ctx, CS_ERR_INVALID, "cs_pairs_fill: bad output dtype");
    if (out->n_rows < 0 || out->n_cols != out->n_rows || out->col0 != 0 || out->d_row_end || out->d_row_weight || out->d_col_weight)
        return fail(ctx, CS_ERR_INVALID, "cs_pairs_fill: the output must be a plain square table");
    if (!out->d_indptr || out->nnz < 0 || (out->nnz > 0 && (!out->d_indices || !out->d_data || !d_keys)))
        return fail(ctx, CS_ERR_INVALID, "cs_pairs_fill: null arrays");
    const long long n_bins = out->n_rows;
    // the row pointers must be those of cs_pairs_count for an output of this size
    long long h_nnz = -1;
    CS_HIP(ctx, hipMemcpyAsync(&h_nnz, (const long long*)out->d_indptr + n_bins, sizeof(long long), hipMemcpyDeviceToHost, stream));
    CS_HIP(ctx, hipStreamSynchronize(stream));
    if (h_nnz != out->nnz)
        return fail(ctx, CS_ERR_INVALID, "cs_pairs_fill: the row pointers end at %lld, the output holds %lld pixels", h_nnz, (long long)out->nnz);
    if (out->nnz > n_pairs) return fail(ctx, CS_ERR_INVALID, "cs_pairs_fill: %lld pixels from %lld pairs", (long long)out->nnz, (long long)n_pairs);
    if (out->nnz == 0) return CS_OK;

    CallBuffers Bf;
    const int b = key_bits(n_bins);
    const unsigned long long* keys = (const unsigned long long*)d_keys;
    const int blocks = (int)((n_pairs + kBlockPairs - 1) / kBlockPairs);
    long long *d_heads = nullptr, *d_last = nullptr;
    long long pixels = 0;
    if (int rc = run_carries(ctx, stream, Bf, keys, n_pairs, b, n_bins, blocks, &d_heads, &d_last, &pixels)) return rc;
    if (pixels != out->nnz)
        return fail(ctx, CS_ERR_INVALID, "cs_pairs_fill: the keys hold %lld pixels, the output %lld", pixels, (long long)out->nnz);
    if (out->dtype == CS_F32)
        hipLaunchKernelGGL((pr_runs_kernel<2, float>), dim3(blocks), dim3(kPrThreads), 0, stream, keys, (long long)n_pairs, b, n_bins, d_heads,
                           d_last, nullptr, nullptr, (long long)out->nnz, (int*)out->d_indices, (float*)out->d_data);
    else
        hipLaunchKernelGGL((pr_runs_kernel<2, double>), dim3(blocks), dim3(kPrThreads), 0, stream, keys, (long long)n_pairs, b, n_bins, d_heads,
                           d_last, nullptr, nullptr, (long long)out->nnz, (int*)out->d_indices, (double*)out->d_data);
    CS_HIP(ctx, hipGetLastError());
    CS_HIP(ctx, hipStreamSynchronize(stream));
    return CS_OK;
}

}  // extern "C"
