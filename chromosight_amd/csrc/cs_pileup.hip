// cs_pileup.hip -- the pileup of the windows of a pixel list, reduced on the device (cs_pileup_blocks).
//
// `detect --iterations` replaces a template by the pixel-wise mean of the windows it just detected, NaN ignored (reference
// cli/chromosight.py:732, 791; detection.py:158-174, np.nanmean over the stack).  The windows are a pure function of the staged
// maps and the pixel list (cs_launch_aux.h window_frame / window_pixel, the code the detect and quantify chains write their
// windows with), so they are summed where they are built instead of crossing the link: 2 km kn numbers leave the device.
//
// THE ORDER OF THE SUMS IS FIXED (include/chromosight_hip.h, cs_pileup_blocks): no floating-point atomics, nothing that depends
// on the grid or the device.
//
//   pileup_chunks_kernel  one wave per chunk of S = pileup_chunk(n) consecutive records.  Lane l owns the pixels e = l, l + 64, ...
//                         of the window, kPileupStrip of them at a time in registers (an 81 x 81 template has 103 pixels per
//                         lane: they are taken in strips, the chunk's records walked once per strip); a pixel's sum starts at
//                         +0.0 and takes the non-NaN values of the chunk's records in record order, its count beside it.
//                         Lazily evaluated bands: the window gathered into the wave's LDS slots per record, as
//                         window_stats_batch_kernel does.
//   pileup_reduce_kernel  one thread per pixel: the chunks' partial sums added from +0.0 in chunk order, the counts likewise.
#include "cs_launch_aux.h"

namespace cs {

namespace {

constexpr int kPileupThreads = 256;
constexpr int kPileupStrip = 8;         // pixels a lane accumulates at a time: 512 per wave >= kLazyWinMax, so a gathered window
                                        // is one strip (and gathered once)
static_assert(64 * kPileupStrip >= kLazyWinMax, "a gathered window must be a single strip");

__global__ __launch_bounds__(kPileupThreads) void pileup_chunks_kernel(const CorrArgs<double>* __restrict__ tab,
                                                                       const int* __restrict__ blk_inter, const int* __restrict__ blk,
                                                                       const int* __restrict__ rows, const int* __restrict__ cols,
                                                                       long long n, long long chunk, long long n_chunks, int kk,
                                                                       double* __restrict__ part_sum, long long* __restrict__ part_cnt,
                                                                       bool fast_windows)
{
    __shared__ double lazy_win[kPileupThreads >> 6][kLazyWinMax];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long c = (long long)blockIdx.x * (kPileupThreads >> 6) + wv;
    if (c >= n_chunks) return;
    const long long t0 = c * chunk, t1 = min(t0 + chunk, n);
    double* win = lazy_win[wv];
    for (int e0 = 0; e0 < kk; e0 += 64 * kPileupStrip) {
        double acc[kPileupStrip];
        int cnt[kPileupStrip];
#pragma unroll
        for (int j = 0; j < kPileupStrip; ++j) {
            acc[j] = 0.0;
            cnt[j] = 0;
        }
        for (long long t = t0; t < t1; ++t) {
            const int b = blk[t];
            const CorrArgs<double>& A = tab[b];
            const WindowFrame F = window_frame(A, blk_inter[b], rows[t], cols[t], lane, win, fast_windows);
            if (F.inside) {                                          // wave-uniform; a window that leaves the map is all NaN
#pragma unroll
                for (int j = 0; j < kPileupStrip; ++j) {
                    const int e = e0 + lane + 64 * j;
                    if (e < kk) {
                        const double v = window_pixel(A, F, e, win);
                        if (v == v) {
                            acc[j] += v;
                            cnt[j] += 1;
                        }
                    }
                }
            }
            if (F.gathered) {
                // (the next record's gather overwrites the window: every lane is done reading it)
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
        }
#pragma unroll
        for (int j = 0; j < kPileupStrip; ++j) {
            const int e = e0 + lane + 64 * j;
            if (e < kk) {
                part_sum[c * kk + e] = acc[j];
                part_cnt[c * kk + e] = cnt[j];
            }
        }
    }
}

__global__ __launch_bounds__(kPileupThreads) void pileup_reduce_kernel(const double* __restrict__ part_sum,
                                                                       const long long* __restrict__ part_cnt, long long n_chunks, int kk,
                                                                       double* __restrict__ sum, long long* __restrict__ cnt)
{
    const int e = blockIdx.x * kPileupThreads + threadIdx.x;
    if (e >= kk) return;
    double s = 0.0;
    long long k = 0;
    for (long long c = 0; c < n_chunks; ++c) {
        s += part_sum[c * kk + e];
        k += part_cnt[c * kk + e];
    }
    sum[e] = s;
    cnt[e] = k;
}

}  // namespace

int enqueue_pileup_batch(const CorrArgs<double>* d_tab, const int* d_inter, const int* d_blk, const int* d_rows, const int* d_cols,
                         long long n, int kk, double* d_part_sum, long long* d_part_cnt, double* d_sum, long long* d_cnt,
                         hipStream_t stream)
{
    if (n <= 0 || kk <= 0) return 0;
    const long long chunk = pileup_chunk(n), n_chunks = pileup_chunks(n);
    const int waves = kPileupThreads >> 6;
    hipLaunchKernelGGL(pileup_chunks_kernel, dim3((unsigned)((n_chunks + waves - 1) / waves)), dim3(kPileupThreads), 0, stream, d_tab,
                       d_inter, d_blk, d_rows, d_cols, n, chunk, n_chunks, kk, d_part_sum, d_part_cnt, fast_windows_on());
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(pileup_reduce_kernel, dim3((unsigned)((kk + kPileupThreads - 1) / kPileupThreads)), dim3(kPileupThreads), 0, stream,
                       d_part_sum, d_part_cnt, n_chunks, kk, d_sum, d_cnt);
    return (int)hipGetLastError();
}

}  // namespace cs
