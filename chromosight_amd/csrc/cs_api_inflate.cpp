// cs_api_inflate.cpp -- the entries over cs_inflate.hip (include/chromosight_hip.h): cs_inflate_chunks, cs_inflate_max_chunk_bytes,
// cs_table_from_columns_count / cs_table_from_columns_fill.  Everything a chunk index could get wrong is refused here, on the host,
// before anything is launched; what a stream could get wrong is the decoder's business (cs_inflate_core.h) and comes back per chunk.
#include "cs_api_internal.h"
#include "cs_inflate.h"
#include "cs_inflate_core.h"
#include "cs_table_rows.h"

using namespace csapi;

namespace {

const char* status_name(int s)
{
    switch (s) {
    case csz::kOk: return "ok";
    case csz::kBadHeader: return "bad zlib header";
    case csz::kBadBlockType: return "reserved block type";
    case csz::kBadStored: return "stored block whose lengths disagree";
    case csz::kBadCodes: return "bad code set or code";
    case csz::kBadDistance: return "distance before the start of the output";
    case csz::kTooLong: return "more output than the chunk holds";
    case csz::kTooShort: return "less output than the chunk holds";
    case csz::kInputEnd: return "input exhausted";
    case csz::kBadChecksum: return "Adler-32 mismatch";
    case csz::kBadChunk: return "unfiltered chunk of the wrong size";
    case csz::kTrailing: return "bytes behind the end of the stream";
    }
    return "unknown status";
}

}  // namespace

extern "C" {

int64_t cs_inflate_max_chunk_bytes(void) { return (int64_t)csz::kMaxChunkBytes; }

int cs_inflate_chunks(cs_ctx* ctx, void* stream_, const void* d_file, int64_t file_bytes, const int64_t* h_offsets, const int64_t* h_nbytes,
                      const int64_t* h_starts, const uint32_t* h_masks, int64_t n_chunks, int32_t elem_bytes, int64_t chunk_elems,
                      int64_t n_elems, const int32_t* h_filters, int32_t n_filters, void* d_out, int32_t* h_status)
{
    CS_ENTER(ctx);
    hipStream_t stream = (hipStream_t)stream_;
    if (n_chunks < 0 || n_elems < 0 || file_bytes < 0 || n_filters < 0) return fail(ctx, CS_ERR_INVALID, "cs_inflate_chunks: negative size");
    if (n_filters > 0 && !h_filters) return fail(ctx, CS_ERR_INVALID, "cs_inflate_chunks: null argument");
    if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4 && elem_bytes != 8)
        return fail(ctx, CS_ERR_UNSUPPORTED, "cs_inflate_chunks: elements of %d bytes", (int)elem_bytes);
    if (chunk_elems < 1) return fail(ctx, CS_ERR_INVALID, "cs_inflate_chunks: chunks of %lld elements", (long long)chunk_elems);
    if (chunk_elems > (int64_t)csz::kMaxChunkBytes / elem_bytes)
        return fail(ctx, CS_ERR_UNSUPPORTED, "cs_inflate_chunks: chunks of %lld bytes decoded, the limit is %u (cs_inflate_max_chunk_bytes)",
                    (long long)chunk_elems * elem_bytes, csz::kMaxChunkBytes);
    if (n_chunks >= (int64_t)std::numeric_limits<int>::max()) return fail(ctx, CS_ERR_UNSUPPORTED, "cs_inflate_chunks: 2^31 - 1 chunks or more");
    // the filters: shuffle (2), gzip (1), Fletcher-32 (3), each at most once and in that order -- the only one a writer can mean
    int bit_shuffle = -1, bit_deflate = -1, bit_fletcher = -1, stage = 0;
    for (int k = 0; k < n_filters; ++k) {
        const int id = h_filters[k];
        const int at = id == 2 ? 1 : id == 1 ? 2 : id == 3 ? 3 : 0;
        if (at == 0) return fail(ctx, CS_ERR_UNSUPPORTED, "cs_inflate_chunks: filter %d", id);
        if (at <= stage || k >= 32) return fail(ctx, CS_ERR_UNSUPPORTED, "cs_inflate_chunks: filters not in the order shuffle, gzip, Fletcher-32");
        stage = at;
        (id == 2 ? bit_shuffle : id == 1 ? bit_deflate : bit_fletcher) = k;
    }
    if (n_chunks == 0) return CS_OK;
    if (!d_file || !h_offsets || !h_nbytes || !h_starts || !h_masks || !d_out || !h_status)
        return fail(ctx, CS_ERR_INVALID, "cs_inflate_chunks: null argument");
    std::vector<csz::ChunkDesc> desc((size_t)n_chunks);
    for (int64_t c = 0; c < n_chunks; ++c) {
        const int64_t off = h_offsets[c], nb = h_nbytes[c], start = h_starts[c];
        if (off < 0 || nb < 0 || nb > (int64_t)std::numeric_limits<uint32_t>::max() || off > file_bytes || nb > file_bytes - off)
            return fail(ctx, CS_ERR_INVALID, "cs_inflate_chunks: chunk %lld (offset %lld, %lld bytes) leaves the buffer of %lld bytes", (long long)c,
                        (long long)off, (long long)nb, (long long)file_bytes);
        if (start < 0 || start >= n_elems)
            return fail(ctx, CS_ERR_INVALID, "cs_inflate_chunks: chunk %lld starts at element %lld of a column of %lld", (long long)c, (long long)start,
                        (long long)n_elems);
        desc[(size_t)c] = {(uint64_t)off, (uint64_t)start, (uint32_t)nb, h_masks[c]};
        h_status[c] = csz::kOk;
    }

    CallBuffers Bf;
    csz::ChunkDesc* d_desc = nullptr;
    int32_t* d_status = nullptr;
    CS_HIP(ctx, Bf.get(&d_desc, (size_t)n_chunks));
    CS_HIP(ctx, Bf.get(&d_status, (size_t)n_chunks));
    CS_HIP(ctx, hipMemcpyAsync(d_desc, desc.data(), (size_t)n_chunks * sizeof(csz::ChunkDesc), hipMemcpyHostToDevice, stream));
    csz::InflateArgs A = {};
    A.file = (const uint8_t*)d_file;
    A.chunks = d_desc;
    A.status = d_status;
    A.out = d_out;
    A.n_elems = (unsigned long long)n_elems;
    A.chunk_elems = (uint32_t)chunk_elems;
    A.n_chunks = (int)n_chunks;
    A.esize = elem_bytes;
    A.bit_shuffle = bit_shuffle, A.bit_deflate = bit_deflate, A.bit_fletcher = bit_fletcher;
    CS_HIP(ctx, csz::launch_inflate(A, ctx->n_cu, stream));
    CS_HIP(ctx, hipMemcpyAsync(h_status, d_status, (size_t)n_chunks * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    CS_HIP(ctx, hipStreamSynchronize(stream));
    int64_t failed = 0, first = -1;
    for (int64_t c = 0; c < n_chunks; ++c)
        if (h_status[c] != csz::kOk) {
            if (first < 0) first = c;
            ++failed;
        }
    if (failed)
        return fail(ctx, CS_ERR_CORRUPT, "cs_inflate_chunks: %lld of %lld chunks failed; the first is chunk %lld (%s)", (long long)failed,
                    (long long)n_chunks, (long long)first, status_name(h_status[first]));
    return CS_OK;
}

int64_t cs_bgzf_max_block_bytes(void) { return (int64_t)csz::kMaxBgzfBlockBytes; }

int cs_bgzf_inflate(cs_ctx* ctx, void* stream_, const void* d_file, int64_t file_bytes, const int64_t* h_offsets, const int64_t* h_nbytes,
                    const int64_t* h_out_offsets, const int64_t* h_isizes, int64_t n_blocks, void* d_text, int64_t text_bytes, int32_t* h_status,
                    int64_t* h_last_newline)
{
    CS_ENTER(ctx);
    hipStream_t stream = (hipStream_t)stream_;
    if (n_blocks < 0 || file_bytes < 0 || text_bytes < 0) return fail(ctx, CS_ERR_INVALID, "cs_bgzf_inflate: negative size");
    if (!h_last_newline) return fail(ctx, CS_ERR_INVALID, "cs_bgzf_inflate: null argument");
    if (n_blocks >= (int64_t)std::numeric_limits<int>::max()) return fail(ctx, CS_ERR_UNSUPPORTED, "cs_bgzf_inflate: 2^31 - 1 blocks or more");
    *h_last_newline = -1;
    if (n_blocks == 0) return CS_OK;
    if (!d_file || !h_offsets || !h_nbytes || !h_out_offsets || !h_isizes || !h_status || (!d_text && text_bytes > 0))
        return fail(ctx, CS_ERR_INVALID, "cs_bgzf_inflate: null argument");
    std::vector<csz::BgzfDesc> desc((size_t)n_blocks);
    std::vector<std::pair<int64_t, int64_t>> spans;              // (start, end) of every block's text that is not empty
    spans.reserve((size_t)n_blocks);
    for (int64_t b = 0; b < n_blocks; ++b) {
        const int64_t off = h_offsets[b], nb = h_nbytes[b], out = h_out_offsets[b], isize = h_isizes[b];
        // the body and the four bytes of its CRC-32 behind it
        if (off < 0 || nb < 0 || nb > (int64_t)std::numeric_limits<uint32_t>::max() || off > file_bytes || nb + 4 > file_bytes - off)
            return fail(ctx, CS_ERR_INVALID, "cs_bgzf_inflate: block %lld (offset %lld, %lld bytes and its CRC-32) leaves the buffer of %lld bytes",
                        (long long)b, (long long)off, (long long)nb, (long long)file_bytes);
        if (isize < 0) return fail(ctx, CS_ERR_INVALID, "cs_bgzf_inflate: block %lld holds %lld bytes", (long long)b, (long long)isize);
        if (isize > (int64_t)csz::kMaxBgzfBlockBytes)
            return fail(ctx, CS_ERR_UNSUPPORTED, "cs_bgzf_inflate: block %lld holds %lld bytes, the limit is %u (cs_bgzf_max_block_bytes)", (long long)b,
                        (long long)isize, csz::kMaxBgzfBlockBytes);
        if (out < 0 || out > text_bytes || isize > text_bytes - out)
            return fail(ctx, CS_ERR_INVALID, "cs_bgzf_inflate: block %lld (text offset %lld, %lld bytes) leaves the text buffer of %lld bytes",
                        (long long)b, (long long)out, (long long)isize, (long long)text_bytes);
        if (isize > 0) spans.emplace_back(out, out + isize);
        desc[(size_t)b] = {(uint64_t)off, (uint64_t)out, (uint32_t)nb, (uint32_t)isize};
        h_status[b] = csz::kOk;
    }
    std::sort(spans.begin(), spans.end());
    for (size_t i = 1; i < spans.size(); ++i)
        if (spans[i].first < spans[i - 1].second)
            return fail(ctx, CS_ERR_INVALID, "cs_bgzf_inflate: the texts of two blocks overlap at offset %lld", (long long)spans[i].first);

    CallBuffers Bf;
    csz::BgzfDesc* d_desc = nullptr;
    int32_t* d_status = nullptr;
    long long* d_last = nullptr;
    CS_HIP(ctx, Bf.get(&d_desc, (size_t)n_blocks));
    CS_HIP(ctx, Bf.get(&d_status, (size_t)n_blocks));
    CS_HIP(ctx, Bf.get(&d_last, 1));
    long long last = -1;
    CS_HIP(ctx, hipMemcpyAsync(d_desc, desc.data(), (size_t)n_blocks * sizeof(csz::BgzfDesc), hipMemcpyHostToDevice, stream));
    CS_HIP(ctx, hipMemcpyAsync(d_last, &last, sizeof(last), hipMemcpyHostToDevice, stream));
    csz::BgzfArgs A = {};
    A.file = (const uint8_t*)d_file;
    A.blocks = d_desc;
    A.status = d_status;
    A.text = (uint8_t*)d_text;
    A.last_newline = d_last;
    A.n_blocks = (int)n_blocks;
    CS_HIP(ctx, csz::launch_bgzf_inflate(A, ctx->n_cu, stream));
    CS_HIP(ctx, hipMemcpyAsync(h_status, d_status, (size_t)n_blocks * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    CS_HIP(ctx, hipMemcpyAsync(&last, d_last, sizeof(last), hipMemcpyDeviceToHost, stream));
    CS_HIP(ctx, hipStreamSynchronize(stream));
    *h_last_newline = (int64_t)last;
    int64_t failed = 0, first = -1;
    for (int64_t b = 0; b < n_blocks; ++b)
        if (h_status[b] != csz::kOk) {
            if (first < 0) first = b;
            ++failed;
        }
    if (failed)
        return fail(ctx, CS_ERR_CORRUPT, "cs_bgzf_inflate: %lld of %lld blocks failed; the first is block %lld (%s)", (long long)failed,
                    (long long)n_blocks, (long long)first, h_status[first] == csz::kBadChecksum ? "CRC-32 mismatch" : status_name(h_status[first]));
    return CS_OK;
}

int cs_table_from_columns_count(cs_ctx* ctx, void* stream_, const void* d_bin1, const void* d_bin2, int32_t id_bytes, const void* d_count,
                                int32_t count_bytes, int64_t nnz, int64_t n_bins, int64_t* d_out_indptr, int32_t* d_out_indices,
                                cs_table_report* h_report)
{
    CS_ENTER(ctx);
    hipStream_t stream = (hipStream_t)stream_;
    if (!d_out_indptr || !h_report) return fail(ctx, CS_ERR_INVALID, "cs_table_from_columns_count: null argument");
    if ((id_bytes != 4 && id_bytes != 8) || (count_bytes != 4 && count_bytes != 8))
        return fail(ctx, CS_ERR_UNSUPPORTED, "cs_table_from_columns_count: ids of %d bytes, counts of %d (int32 / int64 columns only)", (int)id_bytes,
                    (int)count_bytes);
    if (nnz < 0 || n_bins < 0) return fail(ctx, CS_ERR_INVALID, "cs_table_from_columns_count: %lld pixels, %lld bins", (long long)nnz, (long long)n_bins);
    if (n_bins >= (int64_t)std::numeric_limits<int>::max()) return fail(ctx, CS_ERR_UNSUPPORTED, "cs_table_from_columns_count: genomes of 2^31 - 1 bins or more");
    if (nnz > 0 && (!d_bin1 || !d_bin2 || !d_count || !d_out_indices)) return fail(ctx, CS_ERR_INVALID, "cs_table_from_columns_count: null argument");
    cs_table_report rep = {};
    rep.nnz = nnz;
    rep.ids_ok = rep.sorted = rep.upper = 1;
    rep.dtype = CS_F32;
    CS_HIP(ctx, hipMemsetAsync(d_out_indptr, 0, ((size_t)n_bins + 1) * sizeof(long long), stream));
    if (nnz > 0) {
        CallBuffers Bf;
        csz::TableStats* d_stats = nullptr;
        CS_HIP(ctx, Bf.get(&d_stats, 1));
        csz::TableStats st = {0ull, std::numeric_limits<long long>::max(), std::numeric_limits<long long>::min()};
        CS_HIP(ctx, hipMemcpyAsync(d_stats, &st, sizeof(st), hipMemcpyHostToDevice, stream));
        CS_HIP(ctx, csz::launch_table_check(d_bin1, d_bin2, id_bytes, d_count, count_bytes, (long long)nnz, (long long)n_bins, (long long*)d_out_indptr,
                                              d_out_indices, d_stats, ctx->n_cu, stream));
        CS_HIP(ctx, hipMemcpyAsync(&st, d_stats, sizeof(st), hipMemcpyDeviceToHost, stream));
        CS_HIP(ctx, hipStreamSynchronize(stream));
        rep.ids_ok = !(st.flags & 1ull);
        rep.sorted = !(st.flags & 2ull);
        rep.upper = !(st.flags & 4ull);
        rep.count_min = st.count_min;
        rep.count_max = st.count_max;
        rep.dtype = st.count_max < (1ll << 24) ? CS_F32 : CS_F64;      // pipeline.DeviceCool's rule
    } else {
        CS_HIP(ctx, hipStreamSynchronize(stream));
    }
    *h_report = rep;
    return CS_OK;
}

int cs_table_from_columns_fill(cs_ctx* ctx, void* stream_, const void* d_count, int32_t count_bytes, int64_t nnz, void* d_out_data, int32_t dtype)
{
    CS_ENTER(ctx);
    hipStream_t stream = (hipStream_t)stream_;
    if (count_bytes != 4 && count_bytes != 8) return fail(ctx, CS_ERR_UNSUPPORTED, "cs_table_from_columns_fill: counts of %d bytes", (int)count_bytes);
    if (dtype != CS_F32 && dtype != CS_F64) return fail(ctx, CS_ERR_INVALID, "cs_table_from_columns_fill: bad output dtype");
    if (nnz < 0) return fail(ctx, CS_ERR_INVALID, "cs_table_from_columns_fill: %lld pixels", (long long)nnz);
    if (nnz == 0) return CS_OK;
    if (!d_count || !d_out_data) return fail(ctx, CS_ERR_INVALID, "cs_table_from_columns_fill: null argument");
    CS_HIP(ctx, csz::launch_table_fill(d_count, count_bytes, (long long)nnz, d_out_data, dtype == CS_F64, ctx->n_cu, stream));
    CS_HIP(ctx, hipStreamSynchronize(stream));
    return CS_OK;
}

}  // extern "C"
