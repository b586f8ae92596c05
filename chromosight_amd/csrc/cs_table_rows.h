// cs_table_rows.h -- what the kernels that rebuild the resident pixel table row by row share (cs_coarsen.hip: the fine rows under a
// coarse row; cs_merge.hip: row r of every source): the workgroup size, the tail of a column tile (its nonzero accumulators counted and placed
// through wave ballots), the statistics of the count pass and their reduction, the lower bound on a row's sorted columns and the
// device allocations of one call.  Everything here has internal linkage: every
// translation unit that includes it gets its own copy.
#pragma once
#include "cs_api_internal.h"

namespace {

constexpr int kCoThreads = 256;
constexpr double kMaxTotal = 9007199254740992.0;        // 2^53
constexpr int kNoColumn = std::numeric_limits<int>::max();
constexpr long long kNoLimit = std::numeric_limits<long long>::max();      // emit_tile: the output has room for whatever is placed

struct CoStats {
    unsigned long long bad;                 // bit 0: a count that is not a finite non-negative integer below 2^53; bit 1: a column
                                            // outside the table or out of order
    unsigned long long sum_hi, sum_lo;      // the grand total, as the sums of the counts' high and low 32 bits
    unsigned long long vmax;                // the largest summed count
};

// the first position of [lo, hi) whose column is >= key
__device__ __forceinline__ long long lower_bound(const int* __restrict__ indices, long long lo, long long hi, int key)
{
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (indices[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the statistics of a workgroup's threads into *out (s_red: 4 words per wave of LDS that nobody else is using)
__device__ __forceinline__ void block_stats(unsigned long long bad, unsigned long long sum_hi, unsigned long long sum_lo,
                                            unsigned long long vmax, unsigned long long* s_red, CoStats* __restrict__ out)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        bad |= __shfl_down(bad, d);
        sum_hi += __shfl_down(sum_hi, d);
        sum_lo += __shfl_down(sum_lo, d);
        vmax = max(vmax, __shfl_down(vmax, d));
    }
    if (lane == 0) {
        s_red[4 * wave] = bad;
        s_red[4 * wave + 1] = sum_hi;
        s_red[4 * wave + 2] = sum_lo;
        s_red[4 * wave + 3] = vmax;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        CoStats t = {0, 0, 0, 0};
        for (int w = 0; w < kCoThreads / 64; ++w) {
            t.bad |= s_red[4 * w];
            t.sum_hi += s_red[4 * w + 1];
            t.sum_lo += s_red[4 * w + 2];
            t.vmax = max(t.vmax, s_red[4 * w + 3]);
        }
        *out = t;
    }
}

// The tail of a column tile: the accumulators s_acc[0 .. span) that are not zero are the tile's pixels (counts are non-negative: no
// presence bits needed).  Wave ballots give 64-bit words (s_words), wave 0 scans their popcounts (s_wpre, *s_total); in the write
// pass every nonzero column stores its bin (base + c) and its sum at `at` + prefix + popcount(bits below) -- consecutive lanes
// store to increasing, mostly consecutive addresses -- and nothing at or beyond `limit` (kNoLimit: the check folds away); the count pass takes the largest sum.
// Called by the whole workgroup after the barrier behind the walk; returns the tile's pixels.  TILE: the tile's columns.
template <int TILE, typename TO, bool WRITE>
__device__ __forceinline__ int emit_tile(const unsigned long long* s_acc, unsigned long long* s_words, int* s_wpre, int* s_total,
                                         int span, int base, long long at, long long limit, int* __restrict__ out_indices,
                                         TO* __restrict__ out_data, unsigned long long& vmax)
{
    const int tid = threadIdx.x, lane = tid & 63;
    const int nw = (span + 63) >> 6;
    for (int c = tid; c < nw * 64; c += kCoThreads) {
        const unsigned long long a = c < span ? s_acc[c] : 0ull;
        const unsigned long long mask = __ballot(a != 0);
        if (lane == 0) s_words[c >> 6] = mask;
    }
    __syncthreads();
    if (tid < 64) {
        const int x = tid < nw ? __popcll(s_words[tid]) : 0;
        int inc = x;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int y = __shfl_up(inc, d);
            if (lane >= d) inc += y;
        }
        if (tid < TILE / 64) s_wpre[tid] = inc - x;
        if (tid == 63) *s_total = inc;
    }
    __syncthreads();
    for (int c = tid; c < span; c += kCoThreads) {
        const unsigned long long a = s_acc[c];
        if (!a) continue;
        if (WRITE) {
            const int w = c >> 6;
            const long long to = at + s_wpre[w] + __popcll(s_words[w] & ((1ull << lane) - 1ull));
            if (limit == kNoLimit || (unsigned long long)to < (unsigned long long)limit) {
                out_indices[to] = base + c;
                out_data[to] = (TO)a;
            }
        } else {
            vmax = max(vmax, a);
        }
    }
    return *s_total;
}

// the workgroups' statistics (parts[0 .. n_parts)) into parts[n_parts]; one workgroup
__global__ __launch_bounds__(kCoThreads) void co_stats_kernel(CoStats* __restrict__ parts, int n_parts)
{
    __shared__ unsigned long long s_red[4 * (kCoThreads / 64)];
    unsigned long long bad = 0, sum_hi = 0, sum_lo = 0, vmax = 0;
    for (int i = threadIdx.x; i < n_parts; i += kCoThreads) {
        const CoStats p = parts[i];
        bad |= p.bad;
        sum_hi += p.sum_hi;
        sum_lo += p.sum_lo;
        vmax = max(vmax, p.vmax);
    }
    block_stats(bad, sum_hi, sum_lo, vmax, s_red, &parts[n_parts]);
}

// device allocations of one call, freed on every way out (hipFree waits for the work that uses them)
struct CallBuffers {
    std::vector<void*> p;
    ~CallBuffers()
    {
        for (void* q : p) (void)hipFree(q);
    }
    template <typename T>
    hipError_t get(T** out, size_t count)
    {
        void* q = nullptr;
        hipError_t e = hipMalloc(&q, std::max<size_t>(count * sizeof(T), 1));
        if (e == hipSuccess) p.push_back(q);
        *out = (T*)q;
        return e;
    }
};

}  // namespace
