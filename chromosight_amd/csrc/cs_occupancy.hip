// cs_occupancy.hip -- which 64 x 64 output tiles of a dense (inter-chromosomal) map can hold a candidate (cs_csr_tile_occupancy).
//
// A window without a stored pixel that survives staging is all zeros after staging (NaN -> 0): its coefficient is 0
// (cs_pearson_body.inc: num = 0, den = 0 -> 0, and NaN -> 0), and the candidate rules drop exact zeros whatever the
// threshold (flag_keep_kernel, the reference's eliminate_zeros).  A tile of the tile kernel can therefore only produce
// candidates if its windows, dilated by the template, reach such a pixel.  Here:
//
//   occ_mark_kernel     one wave per CSR row of the view: every pixel with count > 0 and finite weights sets the bits of
//                       the (at most 2 x 2 up to 65, 3 x 3 up to 81) output tiles whose windows reach it -- integer atomicOr only
//   occ_compact_kernel  one workgroup: per 32-bit word a popcount, an exclusive scan in word order, and the set bits
//                       written as tile indices by * tiles_x + bx -- the list is in increasing order, the same every run
//
// Pixels of missing bins come with NaN weights and do not mark anything; a stored pixel whose weights are finite is kept even
// when its balanced value rounds to 0 (conservative).
#include "cs_launch_aux.h"

namespace cs {

namespace {

constexpr int kOccThreads = 256;
constexpr int kOccScan = 1024;

struct OccArgs {
    CsrView M;
    int row_off;             // block row of the view's first row
    int km, kn;
    int row_begin, row_end;  // output rows of the tile grid (tile row ty starts at row_begin + 64 ty)
    int tiles_x, tiles_y;
    unsigned* bits;
};

template <typename TV>
__global__ __launch_bounds__(kOccThreads) void occ_mark_kernel(const OccArgs P)
{
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * kOccThreads + threadIdx.x) >> 6;
    const int n_waves = (gridDim.x * kOccThreads) >> 6;
    const TV* __restrict__ data = reinterpret_cast<const TV*>(P.M.data);
    const int kh = (P.km - 1) / 2, kw = (P.kn - 1) / 2;
    const int up = P.km - 1 - kh, left = P.kn - 1 - kw;     // output pixel (i, j) reads rows i - kh .. i + up, columns j - kw .. j + left
    for (int r = wave; r < P.M.n_rows; r += n_waves) {
        const int p = P.row_off + r;
        // output rows whose windows reach row p, inside the grid
        const int i_lo = max(p - up, P.row_begin), i_hi = min(p + kh, P.row_end - 1);
        if (i_lo > i_hi) continue;
        if (P.M.row_w && !(fabs(P.M.row_w[r]) <= 1.7976931348623157e308)) continue;     // NaN / inf weight: staged as 0
        const int ty0 = (i_lo - P.row_begin) >> 6, ty1 = (i_hi - P.row_begin) >> 6;
        const long long k0 = P.M.indptr[r], k1 = P.M.row_end[r];
        for (long long k = k0 + lane; k < k1; k += 64) {
            const int q = P.M.indices[k] - P.M.col0;
            if (q < 0 || q >= P.M.n_cols) continue;
            if (!((double)data[k] > 0.0)) continue;
            if (P.M.col_w && !(fabs(P.M.col_w[q]) <= 1.7976931348623157e308)) continue;
            const int j_lo = max(q - left, 0), j_hi = min(q + kw, P.M.n_cols - 1);
            const int tx0 = j_lo >> 6, tx1 = j_hi >> 6;
            for (int ty = ty0; ty <= ty1; ++ty)
                for (int tx = tx0; tx <= tx1; ++tx) {
                    const long long t = (long long)ty * P.tiles_x + tx;
                    atomicOr(P.bits + (t >> 5), 1u << (t & 31));
                }
        }
    }
}

// one workgroup: the set bits of n_words words, in order, as tile indices; *count = their number (entries beyond cap are not
// written)
__global__ __launch_bounds__(kOccScan) void occ_compact_kernel(const unsigned* __restrict__ bits, long long n_words, int* __restrict__ out,
                                                                long long cap, long long* __restrict__ count)
{
    __shared__ long long part[kOccScan / 64];
    __shared__ long long carry_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (long long base = 0; base < n_words; base += kOccScan) {
        const long long w = base + tid;
        const unsigned word = w < n_words ? bits[w] : 0u;
        const int c = __popc(word);
        // inclusive scan of c over the wave, then over the waves
        long long v = c;
        for (int d = 1; d < 64; d <<= 1) {
            const long long o = __shfl_up(v, d, 64);
            if (lane >= d) v += o;
        }
        if (lane == 63) part[wave] = v;
        __syncthreads();
        long long before = carry_s;
        for (int k = 0; k < wave; ++k) before += part[k];
        long long at = before + v - c;          // exclusive position of this word's first tile
        for (unsigned b = word; b; b &= b - 1, ++at)
            if (at < cap) out[at] = (int)(w * 32 + __builtin_ctz(b));
        __syncthreads();                        // every thread has read carry_s and part[]
        if (tid == kOccScan - 1) carry_s = before + v;
        __syncthreads();
    }
    if (tid == 0) *count = carry_s;
}

}  // namespace

int launch_tile_occupancy(const CsrView& M, int row_off, int km, int kn, int row_begin, int row_end, unsigned* bits, int* out,
                          long long cap, long long* d_count, int n_cu, hipStream_t stream)
{
    OccArgs P;
    P.M = M;
    P.row_off = row_off;
    P.km = km;
    P.kn = kn;
    P.row_begin = row_begin;
    P.row_end = row_end;
    P.tiles_x = (M.n_cols + 63) / 64;
    P.tiles_y = (row_end - row_begin + 63) / 64;
    P.bits = bits;
    const long long n_tiles = (long long)P.tiles_x * P.tiles_y;
    const long long n_words = (n_tiles + 31) / 32;
    hipError_t e = hipMemsetAsync(bits, 0, 4 * (size_t)std::max(n_words, 1LL), stream);
    if (e != hipSuccess) return (int)e;
    if (M.n_rows > 0) {
        const int waves = kOccThreads / 64;
        const int grid = (int)std::max(1LL, std::min<long long>(((long long)M.n_rows + waves - 1) / waves, 16LL * n_cu));
        if (M.is_f64) hipLaunchKernelGGL(occ_mark_kernel<double>, dim3(grid), dim3(kOccThreads), 0, stream, P);
        else hipLaunchKernelGGL(occ_mark_kernel<float>, dim3(grid), dim3(kOccThreads), 0, stream, P);
        e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(occ_compact_kernel, dim3(1), dim3(kOccScan), 0, stream, bits, n_words, out, cap, d_count);
    return (int)hipGetLastError();
}

}  // namespace cs
