// cs_pairs_text.hip -- the body text of a 4DN .pairs file parsed on the device into the four columns cs_pairs_count takes
// (include/chromosight_hip.h cs_pairs_text_count / cs_pairs_text_parse).  The text is cut into tiles of kTileBytes; a line belongs to
// the tile that holds its first byte: byte 0, and every byte behind a '\n' (so a last line without '\n' is a line, and a trailing '\n'
// opens none).
//
//   pt_count_kernel     one workgroup per tile, one 16-byte load per thread: the line starts of the tile.
//   exclusive sum       over the tiles (hipcub::DeviceScan): the index of the first line that starts in each tile; the entry behind
//                       the last tile is the number of lines.
//   pt_parse_kernel     one workgroup per tile.  The tile goes to LDS with the same 16-byte loads; every thread ranks the starts
//                       among its 16 bytes behind those of the threads before it (wave prefix through shuffles, the four waves
//                       through LDS) and lists them in LDS;
//                       then the lines of the tile are parsed 256 at a time, one per lane, by cspt::parse_line (cs_pairs_text_core.h):
//                       the head of a line is read from LDS, whatever lies past the tile's end from global memory.  Consecutive
//                       lanes hold consecutive lines and store consecutive column entries.  A flagged line's (index << 8 | reason)
//                       is reduced to a minimum per wave and merged with one integer atomic minimum, so the report names the first
//                       flagged line whatever the order of the workgroups.
//
// Bounds.  The text is read at offsets below nbytes only: the 16-byte load of a thread after its last byte was checked against nbytes
// (byte by byte otherwise), the byte in front of a thread's 16 when the first of them exists and is not byte 0, and a line's tail
// through cspt::parse_line, which reads no byte at or beyond the `avail` = nbytes - start it is given.  A tile of kTileBytes bytes has at most kTileBytes line starts,
// which is what the list in LDS holds.  A column entry is stored at a line index below the n_lines the caller allocated (the entry
// has checked that the text holds exactly that many before the kernel runs).  The text is never written.
#include <hipcub/hipcub.hpp>

#include "cs_api_internal.h"
#include "cs_pairs_text_core.h"
#include "cs_table_rows.h"

using namespace csapi;

namespace {

constexpr int kPtThreads = 256;
constexpr int kTileBytes = 16 * kPtThreads;          // 4096: cs_pairs_text_tile_bytes()
constexpr unsigned long long kNoFlag = ~0ull;

// the 16 bytes of thread `tid` of the tile at `base`: bytes at or beyond nbytes read as 0
__device__ __forceinline__ uint4 load_16(const unsigned char* __restrict__ text, long long base, long long nbytes)
{
    if (base + 16 <= nbytes) return *reinterpret_cast<const uint4*>(text + base);       // (text is 16-byte aligned, base a multiple of 16)
    unsigned int w[4] = {0, 0, 0, 0};
    for (int j = 0; j < 16; ++j)
        if (base + j < nbytes) w[j >> 2] |= (unsigned int)text[base + j] << (8 * (j & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// bit j set: byte j of the 16 is '\n'
__device__ __forceinline__ unsigned int newline_bits(uint4 v)
{
    const unsigned int w[4] = {v.x, v.y, v.z, v.w};
    unsigned int bits = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) bits |= (unsigned int)(((w[j >> 2] >> (8 * (j & 3))) & 0xffu) == 0x0au) << j;
    return bits;
}

// bit j set: byte base + j of the text starts a line -- it exists, and the byte before it is '\n' (byte 0: always).  v: load_16 at base.
__device__ __forceinline__ unsigned int start_bits(const unsigned char* __restrict__ text, uint4 v, long long base, long long nbytes)
{
    const long long left = nbytes - base;           // my bytes that exist
    if (left <= 0) return 0u;
    unsigned int bits = (newline_bits(v) << 1) & 0xffffu;
    bits |= (unsigned int)(base == 0 || text[base - 1] == '\n');
    return left >= 16 ? bits : bits & ((1u << left) - 1u);
}

__global__ __launch_bounds__(kPtThreads) void pt_count_kernel(const unsigned char* __restrict__ text, long long nbytes,
                                                              long long* __restrict__ tile_lines)
{
    __shared__ int s_wave[kPtThreads / 64];
    const long long base = (long long)blockIdx.x * kTileBytes + 16 * (long long)threadIdx.x;
    int n = __popc(start_bits(text, load_16(text, base, nbytes), base, nbytes));
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) n += __shfl_down(n, d);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int w = 0; w < kPtThreads / 64; ++w) t += s_wave[w];
        tile_lines[blockIdx.x] = t;
    }
}

// the bytes of a line that starts at `start` of the text: below tile_end from the tile in LDS, the rest from global memory
struct TileBytes {
    const unsigned char* s_tile;        // the tile, byte 0 = byte tile_begin of the text
    const unsigned char* text;
    long long start, tile_begin, tile_end;
    __device__ __forceinline__ uint8_t operator()(uint64_t i) const
    {
        const long long g = start + (long long)i;
        return g < tile_end ? s_tile[g - tile_begin] : text[g];
    }
};

__global__ __launch_bounds__(kPtThreads) void pt_parse_kernel(const unsigned char* __restrict__ text, long long nbytes,
                                                              const long long* __restrict__ tile_first, cspt::Format F,
                                                              int* __restrict__ chrom1, long long* __restrict__ pos1,
                                                              int* __restrict__ chrom2, long long* __restrict__ pos2, long long n_lines,
                                                              unsigned long long* __restrict__ flag)
{
    __shared__ __attribute__((aligned(16))) unsigned char s_tile[kTileBytes];
    __shared__ unsigned short s_starts[kTileBytes];
    __shared__ int s_wave[kPtThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long tile_begin = (long long)blockIdx.x * kTileBytes;
    const long long base = tile_begin + 16 * (long long)tid;
    const uint4 v = load_16(text, base, nbytes);
    *reinterpret_cast<uint4*>(s_tile + 16 * tid) = v;
    const unsigned int starts = start_bits(text, v, base, nbytes);
    const int mine = __popc(starts);
    int inc = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(inc, d);
        if (lane >= d) inc += y;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    int rank = inc - mine, total = 0;
    for (int w = 0; w < kPtThreads / 64; ++w) {
        if (w < wave) rank += s_wave[w];
        total += s_wave[w];
    }
    for (unsigned int m = starts; m; m &= m - 1) s_starts[rank++] = (unsigned short)(16 * tid + __ffs(m) - 1);      // rank < kTileBytes
    __syncthreads();

    const long long first = tile_first[blockIdx.x];
    unsigned long long worst = kNoFlag;
    for (int l = tid; l < total; l += kPtThreads) {
        const long long line = first + l;
        TileBytes at = {s_tile, text, tile_begin + s_starts[l], tile_begin, tile_begin + kTileBytes};
        cspt::Pair p = {0, 0, 0, 0};
        const int reason = cspt::parse_line(at, (uint64_t)(nbytes - at.start), F, &p);
        if (reason != cspt::kOk) {
            worst = min(worst, ((unsigned long long)line << 8) | (unsigned long long)reason);
        } else if (line < n_lines) {
            chrom1[line] = p.chrom1;
            pos1[line] = p.pos1;
            chrom2[line] = p.chrom2;
            pos2[line] = p.pos2;
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) worst = min(worst, __shfl_down(worst, d));
    if (lane == 0 && worst != kNoFlag) atomicMin(flag, worst);
}

int check_text(cs_ctx* ctx, const char* who, const void* d_text, long long nbytes)
{
    if (nbytes < 0) return fail(ctx, CS_ERR_INVALID, "%s: %lld bytes", who, nbytes);
    if (nbytes > 0 && !d_text) return fail(ctx, CS_ERR_INVALID, "%s: null argument", who);
    if (((uintptr_t)d_text & 15u) != 0) return fail(ctx, CS_ERR_INVALID, "%s: the text must start at a multiple of 16 bytes", who);
    if (nbytes >= (1LL << 40)) return fail(ctx, CS_ERR_UNSUPPORTED, "%s: texts of 2^40 bytes or more (%lld)", who, nbytes);
    return CS_OK;
}

// the line starts of every tile, their exclusive sum (*d_first: tiles + 1 entries) and the lines of the text
int count_lines(cs_ctx* ctx, hipStream_t stream, CallBuffers& Bf, const unsigned char* text, long long nbytes, int tiles, long long** d_first,
                long long* h_lines)
{
    long long* d_lines = nullptr;
    unsigned char* tmp = nullptr;
    size_t tmp_bytes = 0;
    CS_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, (const long long*)nullptr, (long long*)nullptr, tiles + 1, stream));
    CS_HIP(ctx, Bf.get(&tmp, tmp_bytes));
    CS_HIP(ctx, Bf.get(&d_lines, (size_t)tiles + 1));
    CS_HIP(ctx, Bf.get(d_first, (size_t)tiles + 1));
    CS_HIP(ctx, hipMemsetAsync(d_lines + tiles, 0, sizeof(long long), stream));
    hipLaunchKernelGGL(pt_count_kernel, dim3(tiles), dim3(kPtThreads), 0, stream, text, nbytes, d_lines);
    CS_HIP(ctx, hipGetLastError());
    CS_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, d_lines, *d_first, tiles + 1, stream));
    CS_HIP(ctx, hipMemcpyAsync(h_lines, *d_first + tiles, sizeof(long long), hipMemcpyDeviceToHost, stream));
    CS_HIP(ctx, hipStreamSynchronize(stream));
    if (*h_lines < 1 || *h_lines > nbytes) return fail(ctx, CS_ERR_HIP, "cs_pairs_text: %lld lines in %lld bytes", *h_lines, nbytes);
    return CS_OK;
}

}  // namespace

extern "C" {

int32_t cs_pairs_text_tile_bytes(void) { return kTileBytes; }
int32_t cs_pairs_text_max_line_bytes(void) { return (int32_t)cspt::kMaxLineBytes; }

int32_t cs_pairs_text_name_slot(const uint8_t* name, int64_t len, int64_t n_names)
{
    if (!name || len < 0 || n_names < 0 || n_names >= (1LL << 30)) return -1;
    return (int32_t)(cspt::hash_name(name, len) & (cspt::table_slots(n_names) - 1));
}

int cs_pairs_text_count(cs_ctx* ctx, void* stream_, const void* d_text, int64_t nbytes, int64_t* h_n_lines)
{
    CS_ENTER(ctx);
    hipStream_t stream = (hipStream_t)stream_;
    if (!h_n_lines) return fail(ctx, CS_ERR_INVALID, "cs_pairs_text_count: null argument");
    if (int rc = check_text(ctx, "cs_pairs_text_count", d_text, nbytes)) return rc;
    *h_n_lines = 0;
    if (nbytes == 0) return CS_OK;
    CallBuffers Bf;
    long long* d_first = nullptr;
    long long lines = 0;
    const int tiles = (int)((nbytes + kTileBytes - 1) / kTileBytes);
    if (int rc = count_lines(ctx, stream, Bf, (const unsigned char*)d_text, nbytes, tiles, &d_first, &lines)) return rc;
    *h_n_lines = lines;
    return CS_OK;
}

int cs_pairs_text_parse(cs_ctx* ctx, void* stream_, const void* d_text, int64_t nbytes, const cs_pairs_text_format* fmt, int32_t* d_chrom1,
                        int64_t* d_pos1, int32_t* d_chrom2, int64_t* d_pos2, int64_t n_lines, cs_pairs_text_report* h_report)
{
    CS_ENTER(ctx);
    hipStream_t stream = (hipStream_t)stream_;
    if (!fmt || !h_report) return fail(ctx, CS_ERR_INVALID, "cs_pairs_text_parse: null argument");
    if (int rc = check_text(ctx, "cs_pairs_text_parse", d_text, nbytes)) return rc;
    if (n_lines < 0 || (n_lines > 0 && (!d_chrom1 || !d_pos1 || !d_chrom2 || !d_pos2)))
        return fail(ctx, CS_ERR_INVALID, "cs_pairs_text_parse: %lld lines, or null columns", (long long)n_lines);
    if (n_lines >= (long long)std::numeric_limits<int>::max())
        return fail(ctx, CS_ERR_UNSUPPORTED, "cs_pairs_text_parse: 2^31 - 1 lines or more in one call (%lld)", (long long)n_lines);
    const int32_t cols[4] = {fmt->col_chrom1, fmt->col_pos1, fmt->col_chrom2, fmt->col_pos2};
    int32_t need = 0;
    for (int a = 0; a < 4; ++a) {
        if (cols[a] < 0 || cols[a] >= fmt->width)
            return fail(ctx, CS_ERR_INVALID, "cs_pairs_text_parse: column %d of lines of at most %d fields", (int)cols[a], (int)fmt->width);
        for (int b = 0; b < a; ++b)
            if (cols[a] == cols[b]) return fail(ctx, CS_ERR_INVALID, "cs_pairs_text_parse: field %d is named twice", (int)cols[a]);
        need = std::max(need, cols[a] + 1);
    }
    const int64_t n_names = fmt->n_names;
    if (n_names < 0 || n_names >= (1LL << 30) || !fmt->h_name_offsets || (n_names > 0 && fmt->h_name_offsets[n_names] > 0 && !fmt->h_name_bytes))
        return fail(ctx, CS_ERR_INVALID, "cs_pairs_text_parse: %lld names, or null name arrays", (long long)n_names);
    const uint32_t n_slots = cspt::table_slots(n_names);
    std::vector<int32_t> slots(n_slots), off32((size_t)n_names + 1);
    int64_t twice = -1;
    if (int bad = cspt::build_name_table(fmt->h_name_bytes, fmt->h_name_offsets, n_names, slots.data(), off32.data(), &twice))
        return bad == 2 ? fail(ctx, CS_ERR_INVALID, "cs_pairs_text_parse: name %lld is given twice", (long long)twice)
                        : fail(ctx, CS_ERR_INVALID, "cs_pairs_text_parse: the name offsets do not start at 0, decrease or reach 2^31");
    h_report->n_lines = 0;
    h_report->first_flagged = -1;
    h_report->reason = 0;
    h_report->reserved = 0;
    if (nbytes == 0) {
        if (n_lines != 0) return fail(ctx, CS_ERR_INVALID, "cs_pairs_text_parse: an empty text holds no line, not %lld", (long long)n_lines);
        return CS_OK;
    }

    CallBuffers Bf;
    const unsigned char* text = (const unsigned char*)d_text;
    const int tiles = (int)((nbytes + kTileBytes - 1) / kTileBytes);
    long long* d_first = nullptr;
    long long lines = 0;
    if (int rc = count_lines(ctx, stream, Bf, text, nbytes, tiles, &d_first, &lines)) return rc;
    h_report->n_lines = lines;
    if (lines != n_lines)
        return fail(ctx, CS_ERR_INVALID, "cs_pairs_text_parse: the text holds %lld lines, the columns %lld", lines, (long long)n_lines);
    const size_t name_bytes = (size_t)off32[(size_t)n_names];
    int32_t *d_slots = nullptr, *d_off = nullptr;
    unsigned char* d_names = nullptr;
    unsigned long long* d_flag = nullptr;
    CS_HIP(ctx, Bf.get(&d_slots, (size_t)n_slots));
    CS_HIP(ctx, Bf.get(&d_off, (size_t)n_names + 1));
    CS_HIP(ctx, Bf.get(&d_names, name_bytes));
    CS_HIP(ctx, Bf.get(&d_flag, 1));
    CS_HIP(ctx, hipMemcpyAsync(d_slots, slots.data(), (size_t)n_slots * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    CS_HIP(ctx, hipMemcpyAsync(d_off, off32.data(), ((size_t)n_names + 1) * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    if (name_bytes) CS_HIP(ctx, hipMemcpyAsync(d_names, fmt->h_name_bytes, name_bytes, hipMemcpyHostToDevice, stream));
    CS_HIP(ctx, hipMemsetAsync(d_flag, 0xff, sizeof(unsigned long long), stream));
    cspt::Format F;
    for (int a = 0; a < 4; ++a) F.col[a] = cols[a];
    F.width = fmt->width;
    F.need = need;
    F.slot_mask = n_slots - 1;
    F.slots = d_slots;
    F.name_off = d_off;
    F.name_bytes = d_names;
    hipLaunchKernelGGL(pt_parse_kernel, dim3(tiles), dim3(kPtThreads), 0, stream, text, (long long)nbytes, (const long long*)d_first, F, (int*)d_chrom1,
                       (long long*)d_pos1, (int*)d_chrom2, (long long*)d_pos2, (long long)n_lines, d_flag);
    CS_HIP(ctx, hipGetLastError());
    unsigned long long flagged = kNoFlag;
    CS_HIP(ctx, hipMemcpyAsync(&flagged, d_flag, sizeof(flagged), hipMemcpyDeviceToHost, stream));
    CS_HIP(ctx, hipStreamSynchronize(stream));
    if (flagged != kNoFlag) {
        h_report->first_flagged = (int64_t)(flagged >> 8);
        h_report->reason = (int32_t)(flagged & 0xffu);
    }
    return CS_OK;
}

}  // extern "C"
