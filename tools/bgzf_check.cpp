// bgzf_check -- the BGZF member decoder of cs_inflate.hip (chromosight_amd/csrc/cs_inflate_core.h: inflate_member and the CRC-32 it
// checks) as a host program: the same control flow as on the device with one "lane", built with -fsanitize=address,undefined (make -C
// chromosight_amd/csrc bgzf_check) so that a body which would make the kernel read outside its span or write outside its text is
// reported here, on the CPU, before it ever reaches a GPU.  tests/test_bgzf_host.py writes the records and judges the verdicts.
//
//   bgzf_check FILE
//
// FILE: "CSBZ", uint32 count, then per record uint32 nbytes, uint32 isize, uint32 crc, int32 expected_len (-1: no expected bytes), the
// body (nbytes) and the expected bytes (expected_len); then uint32 buffer_len, the buffer, uint32 n_splits, and per split uint32 n (a
// prefix of the buffer), uint32 want (zlib.crc32 of that prefix), uint32 n_spans and n_spans uint32 span lengths that add up to n --
// n_spans = 0: the shares crc32_share_start gives 64 lanes.  All little-endian.  Per record one line on stdout, "<status> <equal>":
// status as csz::Status, equal = 1 when the status is 0 and the isize output bytes are the expected ones.  Per split one line, "crc <ok>":
// ok = 1 when the remainders of the spans (crc32_span), each shifted by the bytes behind it (crc32_shift) and xor-ed together with the
// shifted initial value, give `want` after the final inversion.  Bodies, outputs and spans are heap blocks of exactly their size, so
// that the address sanitizer sees the first byte on either side.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../chromosight_amd/csrc/cs_inflate_core.h"

namespace {

struct OneLane {
    int lane() const { return 0; }
    int lanes() const { return 1; }
    void sync() const {}
    uint32_t uni(uint32_t v) const { return v; }
    uint64_t sum(uint64_t v) const { return v; }
    uint32_t xor_all(uint32_t v) const { return v; }
};

bool read_exact(FILE* f, void* to, size_t n) { return n == 0 || fread(to, 1, n, f) == n; }

int damaged(const char* path, const char* what, uint32_t r)
{
    fprintf(stderr, "%s: %s %u is damaged\n", path, what, r);
    return 2;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: bgzf_check FILE\n");
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    char magic[4];
    uint32_t count = 0;
    if (!read_exact(f, magic, 4) || memcmp(magic, "CSBZ", 4) != 0 || !read_exact(f, &count, 4)) {
        fprintf(stderr, "%s: not a records file\n", argv[1]);
        return 2;
    }
    csz::Tables* tables = new csz::Tables;
    uint32_t* crc_table = new uint32_t[256];
    for (uint32_t r = 0; r < count; ++r) {
        uint32_t nbytes = 0, isize = 0, crc = 0;
        int32_t expected_len = 0;
        if (!read_exact(f, &nbytes, 4) || !read_exact(f, &isize, 4) || !read_exact(f, &crc, 4) || !read_exact(f, &expected_len, 4) ||
            isize >= (1u << 24))
            return damaged(argv[1], "record", r);
        uint8_t* in = new uint8_t[nbytes];
        uint8_t* out = new uint8_t[isize];
        std::vector<uint8_t> expected(expected_len > 0 ? (size_t)expected_len : 0);
        if (!read_exact(f, in, nbytes) || !read_exact(f, expected.data(), expected.size())) return damaged(argv[1], "record", r);
        memset(out, 0xA5, isize);
        memset(tables, 0xA5, sizeof(*tables));
        memset(crc_table, 0xA5, 256 * sizeof(uint32_t));
        OneLane co;
        const int status = csz::inflate_member(in, nbytes, out, isize, crc, tables, crc_table, co);
        const int equal = status == csz::kOk && expected_len >= 0 && (uint32_t)expected_len == isize &&
                          (isize == 0 || memcmp(out, expected.data(), isize) == 0);
        printf("%d %d\n", status, equal);
        delete[] in;
        delete[] out;
    }
    delete tables;

    uint32_t buffer_len = 0, n_splits = 0;
    if (!read_exact(f, &buffer_len, 4)) return damaged(argv[1], "buffer", 0);
    std::vector<uint8_t> buffer(buffer_len);
    if (!read_exact(f, buffer.data(), buffer_len) || !read_exact(f, &n_splits, 4)) return damaged(argv[1], "buffer", 0);
    for (uint32_t i = 0; i < 256; ++i) crc_table[i] = csz::crc32_table_entry(i);
    for (uint32_t s = 0; s < n_splits; ++s) {
        uint32_t n = 0, want = 0, n_spans = 0;
        if (!read_exact(f, &n, 4) || !read_exact(f, &want, 4) || !read_exact(f, &n_spans, 4) || n > buffer_len) return damaged(argv[1], "split", s);
        std::vector<uint32_t> lens(n_spans);
        if (!read_exact(f, lens.data(), 4 * (size_t)n_spans)) return damaged(argv[1], "split", s);
        if (n_spans == 0)
            for (int lane = 0; lane < 64; ++lane) lens.push_back(csz::crc32_share_start(n, lane + 1, 64) - csz::crc32_share_start(n, lane, 64));
        uint64_t total = 0;
        for (uint32_t len : lens) total += len;
        if (total != n) return damaged(argv[1], "split", s);
        uint32_t acc = csz::crc32_shift(0xFFFFFFFFu, n), at = 0;
        for (uint32_t len : lens) {
            uint8_t* span = new uint8_t[len];                    // a block of its own: a read past the span is seen
            if (len) memcpy(span, buffer.data() + at, len);
            acc ^= csz::crc32_shift(csz::crc32_span(crc_table, span, len), n - at - len);
            delete[] span;
            at += len;
        }
        printf("crc %d\n", (uint32_t)~acc == want);
    }
    delete[] crc_table;
    fclose(f);
    return 0;
}
