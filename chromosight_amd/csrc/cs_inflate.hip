// cs_inflate.hip -- the pixel columns of a .cool decoded on the device (include/chromosight_hip.h cs_inflate_chunks,
// cs_table_from_columns_count / _fill): what hdf5_lite.File.dataset and the constructor of pipeline.DeviceCool do on the host, chunk
// by chunk and column by column, restated for a file whose bytes are in HBM.
//
//   inflate_kernel      one wave (a workgroup of 64) per chunk, chunks taken round robin.  The stored chunk goes through the dataset's
//                       filters backwards: a Fletcher-32 tail is cut off (not verified, as on the host), the zlib stream is decoded
//                       into LDS by csz::inflate_stream (cs_inflate_core.h: stored, fixed and dynamic blocks, Adler-32 from LDS as
//                       a reduction over the lanes), and the decoded chunk leaves LDS through the inverse shuffle -- byte plane p of
//                       element e at p * chunk_elems + e -- as one typed store per element into the column at the chunk's start,
//                       consecutive lanes to consecutive elements, clipped to the column's length (the last chunk is padded).  A
//                       filter the chunk's mask skips is left out.  A chunk that fails stores its status and nothing else.
//                       LDS: the tables (csz::Tables, 3.6 KB) and the chunk, so a 15 KB chunk runs eight waves per CU.
//   bgzf_inflate_kernel one wave per member of a BGZF file (cs_bgzf_inflate), members taken round robin: the raw deflate body is decoded
//                       into LDS by csz::inflate_member, which holds it to the member's ISIZE and CRC-32 (a byte table in LDS, every
//                       lane the remainder of a contiguous share, shifted to the end and xor-reduced), and leaves LDS for
//                       text[out_offset .. out_offset + isize) at any byte offset: byte stores in front of and behind the 16-byte
//                       lines of the text buffer, one 16-byte store per whole line, never a read of it -- the neighbouring bytes of a
//                       line belong to another wave.  The offset of the block's last '\n' goes into one int64 by atomicMax.  A
//                       member that fails stores its status and nothing else.  LDS: tables, CRC table and 64 KiB of text, 69 KiB:
//                       two waves per CU.
//   table_check_kernel  one thread per pixel over bin1_id / bin2_id / count as stored (int32 / int64): ids in [0, n_bins), strictly
//                       behind the pixel before it, on or above the diagonal; smallest and largest count; the column bin narrowed to
//                       int32; and the row pointers: a pixel whose row r differs from the row q of the one before it is the first of
//                       every row in (q, r], the end of the table that of every row behind the last.  For a sorted bin1_id these are
//                       the values of searchsorted(bin1_id, arange(n_bins + 1)).  Flags and extrema are reduced per wave; one
//                       integer atomic per wave and statistic, no float atomics.
//   table_fill_kernel   the counts as float32 or float64 (round to nearest even, as numpy's astype).
#include "cs_inflate.h"
#include "cs_inflate_core.h"

namespace csz {

namespace {

constexpr int kWave = 64;
constexpr uint32_t kTableBytes = (uint32_t)((sizeof(Tables) + 15u) & ~15u);
constexpr int kTabThreads = 256;

struct WaveCoop {
    __device__ __forceinline__ int lane() const { return (int)threadIdx.x; }
    __device__ __forceinline__ int lanes() const { return kWave; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
    __device__ __forceinline__ uint32_t uni(uint32_t v) const { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
    __device__ __forceinline__ uint64_t sum(uint64_t v) const
    {
#pragma unroll
        for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_xor((unsigned long long)v, d);
        return v;
    }
    __device__ __forceinline__ uint32_t xor_all(uint32_t v) const
    {
#pragma unroll
        for (int d = kWave / 2; d > 0; d >>= 1) v ^= (uint32_t)__shfl_xor((int)v, d);
        return v;
    }
};

template <typename UT>
__device__ __forceinline__ void store_elements(const uint8_t* buf, bool shuffled, uint32_t chunk_elems, uint32_t m, UT* __restrict__ to)
{
    constexpr uint32_t ES = sizeof(UT);
    for (uint32_t e = threadIdx.x; e < m; e += kWave) {
        UT v = 0;
#pragma unroll
        for (uint32_t p = 0; p < ES; ++p) v |= (UT)((UT)buf[shuffled ? p * chunk_elems + e : e * ES + p] << (8u * p));
        to[e] = v;
    }
}

__global__ __launch_bounds__(kWave) void inflate_kernel(InflateArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    Tables* T = (Tables*)lds;
    uint8_t* buf = lds + kTableBytes;
    const uint32_t chunk_bytes = A.chunk_elems * (uint32_t)A.esize;
    WaveCoop co;
    for (int c = blockIdx.x; c < A.n_chunks; c += gridDim.x) {
        const ChunkDesc d = A.chunks[c];
        const uint8_t* in = A.file + d.offset;
        uint64_t nb = d.nbytes;
        const bool fletcher = A.bit_fletcher >= 0 && !((d.mask >> A.bit_fletcher) & 1u);
        const bool deflate = A.bit_deflate >= 0 && !((d.mask >> A.bit_deflate) & 1u);
        const bool shuffled = A.bit_shuffle >= 0 && !((d.mask >> A.bit_shuffle) & 1u);
        int status = kOk;
        if (fletcher) {
            if (nb < 4) status = kInputEnd;
            else nb -= 4;
        }
        if (status == kOk) {
            if (deflate) {
                status = inflate_stream(in, nb, buf, chunk_bytes, T, co);
            } else if (nb != chunk_bytes) {
                status = kBadChunk;
            } else {
                for (uint32_t i = threadIdx.x; i < chunk_bytes; i += kWave) buf[i] = in[i];
            }
        }
        __syncthreads();
        if (status == kOk && d.start < A.n_elems) {
            const unsigned long long left = A.n_elems - d.start;
            const uint32_t m = left < A.chunk_elems ? (uint32_t)left : A.chunk_elems;
            if (A.esize == 8) store_elements(buf, shuffled, A.chunk_elems, m, (uint64_t*)A.out + d.start);
            else if (A.esize == 4) store_elements(buf, shuffled, A.chunk_elems, m, (uint32_t*)A.out + d.start);
            else if (A.esize == 2) store_elements(buf, shuffled, A.chunk_elems, m, (uint16_t*)A.out + d.start);
            else store_elements(buf, shuffled, A.chunk_elems, m, (uint8_t*)A.out + d.start);
        }
        if (threadIdx.x == 0) A.status[c] = status;
        __syncthreads();                                         // the next chunk overwrites buf
    }
}

constexpr uint32_t kCrcTableBytes = 256u * sizeof(uint32_t);
constexpr uint32_t kBgzfTextBytes = kMaxBgzfBlockBytes + 16u;      // a line more than a block: the copy-out reads whole words
constexpr uint32_t kBgzfLds = kTableBytes + kCrcTableBytes + kBgzfTextBytes;

__global__ __launch_bounds__(kWave) void bgzf_inflate_kernel(BgzfArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    Tables* T = (Tables*)lds;
    uint32_t* crc_table = (uint32_t*)(lds + kTableBytes);
    uint8_t* buf = lds + kTableBytes + kCrcTableBytes;
    const uint32_t lane = threadIdx.x;
    WaveCoop co;
    for (int b = blockIdx.x; b < A.n_blocks; b += gridDim.x) {
        const BgzfDesc d = A.blocks[b];
        const uint8_t* in = A.file + d.offset;
        uint32_t crc = 0;
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) crc |= (uint32_t)in[(uint64_t)d.nbytes + i] << (8u * i);
        const int status = inflate_member(in, d.nbytes, buf, d.isize, co.uni(crc), T, crc_table, co);
        __syncthreads();
        const uint32_t n = d.isize;
        if (status == kOk && n != 0) {
            // to[0 .. n) = buf[0 .. n): the bytes in front of the first 16-byte line of `to` and behind its last whole one as byte
            // stores, the lines between as one store each, their words put together from the aligned words of buf
            uint8_t* to = A.text + d.out_offset;
            uint32_t head = (uint32_t)((0u - (uintptr_t)to) & 15u);
            if (head > n) head = n;
            const uint32_t lines = (n - head) / 16u, tail = head + 16u * lines;
            if (lane < head) to[lane] = buf[lane];
            const uint32_t shift = 8u * (head & 3u);
            const uint32_t* words = (const uint32_t*)(buf + (head & ~3u));
            for (uint32_t k = lane; k < lines; k += kWave) {
                uint32_t w[5];
#pragma unroll
                for (int j = 0; j < 5; ++j) w[j] = words[4u * k + j];            // (w[4]: at most 4 bytes behind buf[n), inside buf)
                uint4 v;
                v.x = (uint32_t)((((uint64_t)w[1] << 32) | w[0]) >> shift);
                v.y = (uint32_t)((((uint64_t)w[2] << 32) | w[1]) >> shift);
                v.z = (uint32_t)((((uint64_t)w[3] << 32) | w[2]) >> shift);
                v.w = (uint32_t)((((uint64_t)w[4] << 32) | w[3]) >> shift);
                *(uint4*)(to + head + 16u * k) = v;
            }
            if (lane < n - tail) to[tail + lane] = buf[tail + lane];
            // the last '\n' of the block, looked for from its end, 64 bytes at a time: lane 0 has the last byte
            for (uint32_t end = n;; end -= kWave) {
                const bool hit = lane < end && buf[end - 1u - lane] == (uint8_t)'\n';
                const unsigned long long hits = __ballot(hit);
                if (hits != 0ull) {
                    if (lane == 0) atomicMax(A.last_newline, (long long)(d.out_offset + end - (uint32_t)__ffsll(hits)));
                    break;
                }
                if (end <= (uint32_t)kWave) break;
            }
        }
        if (lane == 0) A.status[b] = status;
        __syncthreads();                                         // the next block overwrites buf
    }
}

template <typename TI, typename TC>
__global__ __launch_bounds__(kTabThreads) void table_check_kernel(const TI* __restrict__ bin1, const TI* __restrict__ bin2, const TC* __restrict__ count,
                                                                  long long n, long long n_bins, long long* __restrict__ indptr,
                                                                  int* __restrict__ indices, TableStats* __restrict__ stats)
{
    unsigned long long flags = 0;
    long long mn = 0x7FFFFFFFFFFFFFFFll, mx = -0x7FFFFFFFFFFFFFFFll - 1;
    const long long stride = (long long)gridDim.x * kTabThreads;
    for (long long i = (long long)blockIdx.x * kTabThreads + threadIdx.x; i < n; i += stride) {
        const long long r = bin1[i], c = bin2[i], v = count[i];
        const bool inside = r >= 0 && r < n_bins && c >= 0 && c < n_bins;
        if (!inside) flags |= 1ull;
        long long q = -1;                                        // the row of the pixel before
        if (i > 0) {
            q = bin1[i - 1];
            const long long qc = bin2[i - 1];
            if (!(q < r || (q == r && qc < c))) flags |= 2ull;
        }
        if (c < r) flags |= 4ull;
        indices[i] = (int)c;
        mn = min(mn, v);
        mx = max(mx, v);
        if (inside && q >= -1 && q < r)
            for (long long row = q + 1; row <= r; ++row) indptr[row] = i;
        if (i == n - 1 && inside)
            for (long long row = r + 1; row <= n_bins; ++row) indptr[row] = n;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        flags |= __shfl_down(flags, d);
        mn = min(mn, __shfl_down(mn, d));
        mx = max(mx, __shfl_down(mx, d));
    }
    if ((threadIdx.x & 63) == 0) {
        if (flags) atomicOr(&stats->flags, flags);
        if (mn <= mx) {
            atomicMin(&stats->count_min, mn);
            atomicMax(&stats->count_max, mx);
        }
    }
}

template <typename TC, typename TO>
__global__ __launch_bounds__(kTabThreads) void table_fill_kernel(const TC* __restrict__ count, long long n, TO* __restrict__ data)
{
    const long long stride = (long long)gridDim.x * kTabThreads;
    for (long long i = (long long)blockIdx.x * kTabThreads + threadIdx.x; i < n; i += stride) data[i] = (TO)count[i];
}

int table_grid(long long n, int n_cu)
{
    const long long want = (n + kTabThreads - 1) / kTabThreads, cap = 8LL * (n_cu > 0 ? n_cu : 1);
    return (int)(want < 1 ? 1 : want < cap ? want : cap);
}

}  // namespace

hipError_t launch_inflate(const InflateArgs& A, int n_cu, hipStream_t stream)
{
    if (A.n_chunks <= 0) return hipSuccess;
    const size_t chunk_bytes = (size_t)A.chunk_elems * (size_t)A.esize;
    const size_t lds = kTableBytes + ((chunk_bytes + 15u) & ~(size_t)15u);
    // more dynamic LDS than a launch gets by default: a per-function, per-device attribute (cheap; set on every call)
    hipError_t e = hipFuncSetAttribute((const void*)inflate_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    // as many workgroups as the LDS lets a CU hold at once (at most 32 waves), each taking chunks round robin
    const long long per_cu = (long long)(160 * 1024) / (long long)lds;
    const long long resident = (long long)(n_cu > 0 ? n_cu : 1) * (per_cu < 1 ? 1 : per_cu > 32 ? 32 : per_cu);
    const int grid = (int)(A.n_chunks < resident ? A.n_chunks : resident);
    hipLaunchKernelGGL(inflate_kernel, dim3(grid), dim3(kWave), lds, stream, A);
    return hipGetLastError();
}

hipError_t launch_bgzf_inflate(const BgzfArgs& A, int n_cu, hipStream_t stream)
{
    if (A.n_blocks <= 0) return hipSuccess;
    hipError_t e = hipFuncSetAttribute((const void*)bgzf_inflate_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    const long long resident = (long long)(n_cu > 0 ? n_cu : 1) * (long long)((160u * 1024u) / kBgzfLds);      // two workgroups per CU
    const int grid = (int)(A.n_blocks < resident ? A.n_blocks : resident);
    hipLaunchKernelGGL(bgzf_inflate_kernel, dim3(grid), dim3(kWave), kBgzfLds, stream, A);
    return hipGetLastError();
}

hipError_t launch_table_check(const void* bin1, const void* bin2, int id_bytes, const void* count, int count_bytes, long long n, long long n_bins,
                              long long* indptr, int* indices, TableStats* stats, int n_cu, hipStream_t stream)
{
    const int grid = table_grid(n, n_cu);
#define CS_TAB_CHECK(TI, TC)                                                                                                             \
    hipLaunchKernelGGL((table_check_kernel<TI, TC>), dim3(grid), dim3(kTabThreads), 0, stream, (const TI*)bin1, (const TI*)bin2,          \
                       (const TC*)count, n, n_bins, indptr, indices, stats)
    if (id_bytes == 8 && count_bytes == 8) CS_TAB_CHECK(long long, long long);
    else if (id_bytes == 8) CS_TAB_CHECK(long long, int);
    else if (count_bytes == 8) CS_TAB_CHECK(int, long long);
    else CS_TAB_CHECK(int, int);
#undef CS_TAB_CHECK
    return hipGetLastError();
}

hipError_t launch_table_fill(const void* count, int count_bytes, long long n, void* data, int f64, int n_cu, hipStream_t stream)
{
    const int grid = table_grid(n, n_cu);
#define CS_TAB_FILL(TC, TO) \
    hipLaunchKernelGGL((table_fill_kernel<TC, TO>), dim3(grid), dim3(kTabThreads), 0, stream, (const TC*)count, n, (TO*)data)
    if (count_bytes == 8 && f64) CS_TAB_FILL(long long, double);
    else if (count_bytes == 8) CS_TAB_FILL(long long, float);
    else if (f64) CS_TAB_FILL(int, double);
    else CS_TAB_FILL(int, float);
#undef CS_TAB_FILL
    return hipGetLastError();
}

}  // namespace csz
