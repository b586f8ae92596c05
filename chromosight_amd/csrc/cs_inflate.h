// cs_inflate.h -- what cs_inflate.hip (the kernels) and cs_api_inflate.cpp (their entries, include/chromosight_hip.h cs_inflate_chunks /
// cs_table_from_columns_*) share: the argument blocks and the launchers.  Internal to the library.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace csz {

constexpr uint32_t kMaxChunkBytes = 128u * 1024u;      // cs_inflate_max_chunk_bytes(): a chunk and the decode tables fit a CU's LDS

struct ChunkDesc {
    uint64_t offset;       // of the stored chunk in the buffer of file bytes
    uint64_t start;        // its first element in the column
    uint32_t nbytes;       // stored size
    uint32_t mask;         // filter mask: bit k set = filter k of the dataset's list was not applied
};

struct InflateArgs {
    const uint8_t* file;
    const ChunkDesc* chunks;
    int32_t* status;               // per chunk: csz::Status
    void* out;                     // the column, n_elems elements of esize bytes
    unsigned long long n_elems;
    uint32_t chunk_elems;
    int n_chunks;
    int esize;                     // 1, 2, 4, 8
    int bit_shuffle, bit_deflate, bit_fletcher;      // the filters' positions in the dataset's list (their mask bits), -1 = not in it
};

hipError_t launch_inflate(const InflateArgs& A, int n_cu, hipStream_t stream);

constexpr uint32_t kMaxBgzfBlockBytes = 64u * 1024u;   // cs_bgzf_max_block_bytes(): the most text a BGZF member holds

struct BgzfDesc {
    uint64_t offset;       // of the member's deflate body in the buffer of file bytes; its CRC-32 stands in the 4 bytes behind the body
    uint64_t out_offset;   // of its text in the text buffer
    uint32_t nbytes;       // of the body
    uint32_t isize;        // of its text
};

struct BgzfArgs {
    const uint8_t* file;
    const BgzfDesc* blocks;
    int32_t* status;               // per block: csz::Status
    uint8_t* text;
    long long* last_newline;       // the largest offset in text of a '\n' written, by atomicMax (the caller stores -1 first)
    int n_blocks;
};

hipError_t launch_bgzf_inflate(const BgzfArgs& A, int n_cu, hipStream_t stream);

struct TableStats {
    unsigned long long flags;      // bit 0: an id outside [0, n_bins); bit 1: a pixel not behind the one before it; bit 2: a pixel below the diagonal
    long long count_min, count_max;
};

// the check pass of the finish: statistics, row pointers (zeroed by the caller), column bins.  id_bytes / count_bytes: 4 or 8.
hipError_t launch_table_check(const void* bin1, const void* bin2, int id_bytes, const void* count, int count_bytes, long long n, long long n_bins,
                              long long* indptr, int* indices, TableStats* stats, int n_cu, hipStream_t stream);
// the counts as float32 (f64 = 0) or float64
hipError_t launch_table_fill(const void* count, int count_bytes, long long n, void* data, int f64, int n_cu, hipStream_t stream);

}  // namespace csz
