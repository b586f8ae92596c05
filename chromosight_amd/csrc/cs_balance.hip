// cs_balance.hip -- ICE balancing of the resident genome pixel table (cooler.balance_cooler; the reference's
// HicGenome.normalize runs it on a file without weights, contacts_map.py:203-221).  cs_api_balance.cpp drives it:
//
//   once per call   ice_rowid_kernel + a stable radix sort of the column indices + ice_csc_kernel + ice_colptr_kernel:
//                   a CSC permutation of the upper table (column c: its pixels (r <= c, c) by increasing r, the values
//                   already filtered), so that the column half of a marginal is a gather-free row walk like the other half;
//                   ice_marg_kernel<INIT>: the filtered count and nonzero marginals (the host takes the filter medians)
//   per iteration   ice_marg_kernel: m[i] = sum over the kept pixels of bin i (row side from the CSR, column side from the
//                   CSC) of count * b[bin1] * b[bin2], float64, and (count, sum, M2) of the nonzero m of every chunk of 64 bins;
//                   ice_span_kernel: per span, the chunks' partials combined in a fixed order (Chan et al.) -> mean, var,
//                   convergence; ice_update_kernel: b[i] /= m[i] / mean (m = 0: unchanged) for the spans of this iteration
//   at the end      ice_finish_kernel: 0 -> NaN, / sqrt(scale)
//
// A pixel adds to the marginal of both of its bins (a diagonal pixel twice).  With cis_only the spans are the chromosomes,
// which share no pixel: they iterate side by side, and a span that has stopped is frozen (its chunks return at once) --
// the result of the reference's chromosome-by-chromosome loop.  Every reduction has a fixed shape (wave butterflies, per-chunk
// slots, per-span sequential combination): no float atomics, the weights are bitwise reproducible.  The only atomic is the
// integer count of spans still running; when it reaches 0, the launches queued for the remaining iterations return at once.
#include <hipcub/hipcub.hpp>

#include "cs_launch_aux.h"

namespace cs {

namespace {

constexpr int kIceThreads = 256;
constexpr int kIceWaves = kIceThreads / 64;
static_assert(kIceChunk == 64, "the chunk statistics give one bin to each lane of a wave");

__device__ __forceinline__ double ice_wave_sum(double x)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

__global__ __launch_bounds__(kIceThreads) void ice_rowid_kernel(const long long* __restrict__ indptr, int n, int* __restrict__ rowid,
                                                                 int* __restrict__ iota)
{
    const int lane = threadIdx.x & 63;
    for (int r = blockIdx.x * kIceWaves + (threadIdx.x >> 6); r < n; r += gridDim.x * kIceWaves) {
        const long long k1 = indptr[r + 1];
        for (long long k = indptr[r] + lane; k < k1; k += 64) {
            rowid[k] = r;
            iota[k] = (int)k;
        }
    }
}

// column-sorted entry j: row, and the value when the pixel survives the filters (0 otherwise); *bad = 1 for a pixel below the
// diagonal
template <typename TV>
__global__ __launch_bounds__(kIceThreads) void ice_csc_kernel(const int* __restrict__ col_sorted, const int* __restrict__ perm,
                                                              const int* __restrict__ rowid, const TV* __restrict__ data,
                                                              const int* __restrict__ bin_lim, int ignore_diags, long long nnz,
                                                              int* __restrict__ csc_row, TV* __restrict__ csc_val, int* __restrict__ bad)
{
    for (long long j = blockIdx.x * (long long)kIceThreads + threadIdx.x; j < nnz; j += (long long)gridDim.x * kIceThreads) {
        const int k = perm[j];
        const int r = rowid[k];
        const int c = col_sorted[j];
        if (c < r) *bad = 1;
        const bool keep = (long long)c - r >= ignore_diags && c < bin_lim[r];
        csc_row[j] = r;
        csc_val[j] = keep ? data[k] : TV(0);
    }
}

__global__ __launch_bounds__(kIceThreads) void ice_colptr_kernel(const int* __restrict__ col_sorted, long long nnz, int n,
                                                                 long long* __restrict__ colptr)
{
    for (int c = blockIdx.x * kIceThreads + threadIdx.x; c <= n; c += gridDim.x * kIceThreads) {
        long long lo = 0, hi = nnz;                     // first entry with column >= c
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (col_sorted[mid] < c) lo = mid + 1;
            else hi = mid;
        }
        colptr[c] = lo;
    }
}

// one workgroup per chunk (64 bins of one chromosome), one wave per bin.  INIT: bias all ones, out = filtered count marginal,
// out_nnz = marginal of (count != 0).  Otherwise out = the bias-weighted marginal and part[chunk] = its nonzero statistics.
template <typename TV, bool INIT>
__global__ __launch_bounds__(kIceThreads) void ice_marg_kernel(IceDev D, const TV* __restrict__ data, const TV* __restrict__ csc_val)
{
    const IceChunk ch = D.chunks[blockIdx.x];
    if (!INIT && (D.ctl[0] == 0 || D.st[ch.span].done)) return;          // (workgroup-uniform)
    __shared__ double sm[kIceChunk];
    const int lane = threadIdx.x & 63;
    for (int i = ch.lo + (threadIdx.x >> 6); i < ch.hi; i += kIceWaves) {
        const double bi = INIT ? 1.0 : D.bias[i];
        double acc = 0.0, nz = 0.0;
        if (bi != 0.0) {                                  // (a zero weight: every term is 0)
            const long long cmin = (long long)i + D.ignore_diags;
            const long long k1 = D.indptr[i + 1];
            for (long long k = D.indptr[i] + lane; k < k1; k += 64) {
                const int c = D.indices[k];
                if (c >= cmin && c < ch.lim) {
                    const double v = (double)data[k];
                    if (INIT) {
                        acc += v;
                        nz += v != 0.0 ? 1.0 : 0.0;
                    } else {
                        acc += (v * bi) * D.bias[c];
                    }
                }
            }
            const long long j1 = D.colptr[i + 1];
            for (long long j = D.colptr[i] + lane; j < j1; j += 64) {
                const double v = (double)csc_val[j];
                if (INIT) {
                    acc += v;
                    nz += v != 0.0 ? 1.0 : 0.0;
                } else {
                    acc += (v * D.bias[D.csc_row[j]]) * bi;
                }
            }
        }
        acc = ice_wave_sum(acc);
        if (INIT) nz = ice_wave_sum(nz);
        if (lane == 0) {
            D.marg[i] = acc;
            if (INIT) D.marg_nnz[i] = nz;
            else sm[i - ch.lo] = acc;
        }
    }
    if (INIT) return;
    __syncthreads();
    if (threadIdx.x >= 64) return;
    const double x = lane < ch.hi - ch.lo ? sm[lane] : 0.0;
    const bool on = x != 0.0;
    const double cnt = (double)__popcll(__ballot(on));
    const double sum = ice_wave_sum(x);
    const double mean = cnt > 0.0 ? sum / cnt : 0.0;
    const double m2 = ice_wave_sum(on ? (x - mean) * (x - mean) : 0.0);
    if (lane == 0) {
        D.part[3 * blockIdx.x] = cnt;
        D.part[3 * blockIdx.x + 1] = sum;
        D.part[3 * blockIdx.x + 2] = m2;
    }
}

struct IceMoments {
    double n, sum, m2;
};

__device__ __forceinline__ IceMoments ice_combine(IceMoments a, IceMoments b)
{
    if (b.n == 0.0) return a;
    if (a.n == 0.0) return b;
    const double n = a.n + b.n;
    const double d = b.sum / b.n - a.sum / a.n;
    return {n, a.sum + b.sum, a.m2 + b.m2 + d * d * (a.n * b.n / n)};
}

// one workgroup per span: mean and variance of its nonzero marginals, then the stopping rules of cooler's loop
__global__ __launch_bounds__(kIceThreads) void ice_span_kernel(IceDev D, int it)
{
    const int s = blockIdx.x;
    if (D.ctl[0] == 0 || D.st[s].done) return;
    __shared__ IceMoments red[kIceThreads];
    IceMoments acc = {0.0, 0.0, 0.0};
    const int c1 = D.span_chunk0[s + 1];
    for (int c = D.span_chunk0[s] + threadIdx.x; c < c1; c += kIceThreads)
        acc = ice_combine(acc, {D.part[3 * c], D.part[3 * c + 1], D.part[3 * c + 2]});
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = kIceThreads / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] = ice_combine(red[threadIdx.x], red[threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const IceMoments t = red[0];
    IceSpanState& S = D.st[s];
    S.iters += 1;
    S.last_iter = it;
    if (t.n == 0.0) {                                   // no nonzero marginal: weights NaN, scale NaN, var 0
        S.empty = 1;
        S.converged = 1;
        S.var = 0.0;
        S.mean = __builtin_nan("");
        S.done = 1;
    } else {
        S.mean = t.sum / t.n;
        S.var = t.m2 / t.n;
        if (S.var < D.tol) S.converged = 1;
        S.done = S.converged || S.iters >= D.max_iters;
    }
    D.ctl[1] = it;                                      // (every writer stores the same value)
    if (S.done) atomicSub(&D.ctl[0], 1);
}

// b[i] /= m[i] / mean for the spans that iterated in `it` (cooler: marg /= nzmarg.mean(); marg[marg == 0] = 1; bias /= marg)
__global__ __launch_bounds__(kIceChunk) void ice_update_kernel(IceDev D, int it)
{
    if (D.ctl[1] != it) return;
    const IceChunk ch = D.chunks[blockIdx.x];
    const IceSpanState& S = D.st[ch.span];
    if (S.last_iter != it || S.empty) return;
    const int i = ch.lo + (int)threadIdx.x;
    if (i >= ch.hi) return;
    double q = D.marg[i] / S.mean;
    if (q == 0.0) q = 1.0;
    D.bias[i] = D.bias[i] / q;
}

__global__ __launch_bounds__(kIceChunk) void ice_finish_kernel(IceDev D)
{
    const IceChunk ch = D.chunks[blockIdx.x];
    const IceSpanState& S = D.st[ch.span];
    const int i = ch.lo + (int)threadIdx.x;
    if (i >= ch.hi) return;
    double b = D.bias[i];
    if (S.empty || b == 0.0) b = __builtin_nan("");
    else if (D.rescale) b = b / sqrt(S.mean);
    D.bias[i] = b;
}

inline int grid_for(long long items, int per_block, int n_cu)
{
    return (int)std::max<long long>(1, std::min<long long>((items + per_block - 1) / per_block, 8LL * n_cu));
}

}  // namespace

size_t ice_sort_scratch_bytes(long long nnz, int end_bit)
{
    size_t bytes = 0;
    if (nnz <= 0) return 0;
    if (hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, (const int*)nullptr, (int*)nullptr, (const int*)nullptr, (int*)nullptr,
                                           (int)nnz, 0, end_bit, (hipStream_t)0) != hipSuccess)
        return 0;
    return bytes;
}

int ice_prepare(const IceDev& D, const void* data, int data_is_f64, void* csc_val, const int* bin_lim, int* rowid, int* iota,
                int* col_sorted, int* perm, void* sort_tmp, size_t sort_bytes, int end_bit, int* bad, int n_cu, hipStream_t stream)
{
    const int n = D.n;
    const long long nnz = D.nnz;
    if (nnz > 0) {
        hipLaunchKernelGGL(ice_rowid_kernel, dim3(grid_for(n, kIceWaves, n_cu)), dim3(kIceThreads), 0, stream, D.indptr, n, rowid, iota);
        hipError_t e = hipcub::DeviceRadixSort::SortPairs(sort_tmp, sort_bytes, D.indices, col_sorted, (const int*)iota, perm, (int)nnz, 0,
                                                          end_bit, stream);
        if (e != hipSuccess) return (int)e;
        const dim3 g(grid_for(nnz, kIceThreads, n_cu));
        if (data_is_f64)
            hipLaunchKernelGGL(ice_csc_kernel<double>, g, dim3(kIceThreads), 0, stream, col_sorted, perm, rowid, (const double*)data,
                               bin_lim, D.ignore_diags, nnz, D.csc_row, (double*)csc_val, bad);
        else
            hipLaunchKernelGGL(ice_csc_kernel<float>, g, dim3(kIceThreads), 0, stream, col_sorted, perm, rowid, (const float*)data,
                               bin_lim, D.ignore_diags, nnz, D.csc_row, (float*)csc_val, bad);
    }
    hipLaunchKernelGGL(ice_colptr_kernel, dim3(grid_for((long long)n + 1, kIceThreads, n_cu)), dim3(kIceThreads), 0, stream,
                       col_sorted, nnz, n, D.colptr);
    if (D.n_chunks > 0) {
        if (data_is_f64)
            hipLaunchKernelGGL((ice_marg_kernel<double, true>), dim3(D.n_chunks), dim3(kIceThreads), 0, stream, D, (const double*)data,
                               (const double*)csc_val);
        else
            hipLaunchKernelGGL((ice_marg_kernel<float, true>), dim3(D.n_chunks), dim3(kIceThreads), 0, stream, D, (const float*)data,
                               (const float*)csc_val);
    }
    return (int)hipGetLastError();
}

int ice_iterate(const IceDev& D, const void* data, int data_is_f64, const void* csc_val, int max_iters, hipStream_t stream)
{
    if (D.n_chunks > 0 || D.n_spans > 0) {
        for (int it = 0; it < max_iters; ++it) {
            if (D.n_chunks > 0) {
                if (data_is_f64)
                    hipLaunchKernelGGL((ice_marg_kernel<double, false>), dim3(D.n_chunks), dim3(kIceThreads), 0, stream, D,
                                       (const double*)data, (const double*)csc_val);
                else
                    hipLaunchKernelGGL((ice_marg_kernel<float, false>), dim3(D.n_chunks), dim3(kIceThreads), 0, stream, D,
                                       (const float*)data, (const float*)csc_val);
            }
            hipLaunchKernelGGL(ice_span_kernel, dim3(D.n_spans), dim3(kIceThreads), 0, stream, D, it);
            if (D.n_chunks > 0) hipLaunchKernelGGL(ice_update_kernel, dim3(D.n_chunks), dim3(kIceChunk), 0, stream, D, it);
        }
        if (D.n_chunks > 0) hipLaunchKernelGGL(ice_finish_kernel, dim3(D.n_chunks), dim3(kIceChunk), 0, stream, D);
    }
    return (int)hipGetLastError();
}

}  // namespace cs
