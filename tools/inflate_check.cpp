// inflate_check -- the decoder core of cs_inflate.hip (chromosight_amd/csrc/cs_inflate_core.h) as a host program: the same
// control flow as on the device with one "lane", built with -fsanitize=address,undefined (make -C chromosight_amd/csrc
// inflate_check) so that a stream which would make the kernel read outside its input or write outside its output is reported here,
// on the CPU, before it ever reaches a GPU.  tests/test_inflate_host.py writes the streams and judges the verdicts.
//
//   inflate_check FILE
//
// FILE: "CSIF", uint32 count, then per record uint32 nbytes, uint32 cap, int32 expected_len (-1: no expected bytes), the stream
// (nbytes) and the expected bytes (expected_len).  All little-endian.  Per record one line on stdout: "<status> <equal>", status as
// csz::Status, equal = 1 when the status is 0 and the cap output bytes are the expected ones.  The stream and the output are heap
// blocks of exactly nbytes and cap bytes, so that the address sanitizer sees the first byte on either side.
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
};

bool read_exact(FILE* f, void* to, size_t n) { return n == 0 || fread(to, 1, n, f) == n; }

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: inflate_check FILE\n");
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    char magic[4];
    uint32_t count = 0;
    if (!read_exact(f, magic, 4) || memcmp(magic, "CSIF", 4) != 0 || !read_exact(f, &count, 4)) {
        fprintf(stderr, "%s: not a stream file\n", argv[1]);
        return 2;
    }
    csz::Tables* tables = new csz::Tables;
    for (uint32_t r = 0; r < count; ++r) {
        uint32_t nbytes = 0, cap = 0;
        int32_t expected_len = 0;
        if (!read_exact(f, &nbytes, 4) || !read_exact(f, &cap, 4) || !read_exact(f, &expected_len, 4) || cap >= (1u << 24)) {
            fprintf(stderr, "%s: record %u is damaged\n", argv[1], r);
            return 2;
        }
        uint8_t* in = new uint8_t[nbytes];
        uint8_t* out = new uint8_t[cap];
        std::vector<uint8_t> expected(expected_len > 0 ? (size_t)expected_len : 0);
        if (!read_exact(f, in, nbytes) || !read_exact(f, expected.data(), expected.size())) {
            fprintf(stderr, "%s: record %u is cut short\n", argv[1], r);
            return 2;
        }
        memset(out, 0xA5, cap);
        memset(tables, 0xA5, sizeof(*tables));
        OneLane co;
        const int status = csz::inflate_stream(in, nbytes, out, cap, tables, co);
        const int equal = status == csz::kOk && expected_len >= 0 && (uint32_t)expected_len == cap && memcmp(out, expected.data(), cap) == 0;
        printf("%d %d\n", status, equal);
        delete[] in;
        delete[] out;
    }
    delete tables;
    fclose(f);
    return 0;
}
