// pairs_text_check -- the line parser of cs_pairs_text.hip and the builder of its name table (chromosight_amd/csrc/
// cs_pairs_text_core.h) as a host program: the function a lane runs on the device, here over every line of a text in turn, built with
// -fsanitize=address,undefined (make -C chromosight_amd/csrc pairs_text_check) so that a line which would make the kernel read
// outside the text or the name table is reported here, on the CPU, before it ever reaches a GPU.  tests/test_pairs_text_host.py
// writes the records and judges the verdicts.
//
//   pairs_text_check FILE
//
// FILE: "CSPT", uint32 count, then per record: int32 col[4], int32 width, uint32 n_names, per name uint32 length + its bytes,
// uint32 nbytes + the text, int64 expected lines, int64 expected first flagged line (-1: none), int32 expected reason, and, when no
// line is expected to be flagged, the expected columns: chrom1 (int32 per line), pos1 (int64), chrom2 (int32), pos2 (int64).  All
// little-endian.  Per record one line on stdout: "<lines> <first flagged> <reason> <equal>", equal = 1 when all three are the
// expected ones and, without a flagged line, so are the columns.  The text, the names and the tables are heap blocks of exactly their
// size, so that the address sanitizer sees the first byte on either side; lines are cut as the kernel cuts them (a line starts at
// byte 0 and behind every '\n').
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../chromosight_amd/csrc/cs_pairs_text_core.h"

namespace {

bool read_exact(FILE* f, void* to, size_t n) { return n == 0 || fread(to, 1, n, f) == n; }

template <typename T>
bool read_column(FILE* f, std::vector<T>& to, size_t n)
{
    to.resize(n);
    return read_exact(f, to.data(), n * sizeof(T));
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: pairs_text_check FILE\n");
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    char magic[4];
    uint32_t count = 0;
    if (!read_exact(f, magic, 4) || memcmp(magic, "CSPT", 4) != 0 || !read_exact(f, &count, 4)) {
        fprintf(stderr, "%s: not a record file\n", argv[1]);
        return 2;
    }
    for (uint32_t r = 0; r < count; ++r) {
        int32_t head[5];
        uint32_t n_names = 0, nbytes = 0;
        if (!read_exact(f, head, sizeof(head)) || !read_exact(f, &n_names, 4) || n_names >= (1u << 24)) {
            fprintf(stderr, "%s: record %u is damaged\n", argv[1], r);
            return 2;
        }
        std::vector<uint8_t> gathered;
        std::vector<int64_t> offsets(1, 0);
        for (uint32_t k = 0; k < n_names; ++k) {
            uint32_t len = 0;
            if (!read_exact(f, &len, 4) || len >= (1u << 24)) return 2;
            gathered.resize(gathered.size() + len);
            if (!read_exact(f, gathered.data() + gathered.size() - len, len)) return 2;
            offsets.push_back((int64_t)gathered.size());
        }
        if (!read_exact(f, &nbytes, 4) || nbytes >= (1u << 28)) return 2;
        uint8_t* text = new uint8_t[nbytes];
        uint8_t* name_bytes = new uint8_t[gathered.size()];
        if (!gathered.empty()) memcpy(name_bytes, gathered.data(), gathered.size());
        int64_t want_lines = 0, want_flagged = 0;
        int32_t want_reason = 0;
        if (!read_exact(f, text, nbytes) || !read_exact(f, &want_lines, 8) || !read_exact(f, &want_flagged, 8) || !read_exact(f, &want_reason, 4) ||
            want_lines < 0 || want_lines > (int64_t)nbytes) {
            fprintf(stderr, "%s: record %u is cut short\n", argv[1], r);
            return 2;
        }
        std::vector<int32_t> want_c1, want_c2;
        std::vector<int64_t> want_p1, want_p2;
        if (want_flagged < 0 && (!read_column(f, want_c1, (size_t)want_lines) || !read_column(f, want_p1, (size_t)want_lines) ||
                                 !read_column(f, want_c2, (size_t)want_lines) || !read_column(f, want_p2, (size_t)want_lines))) {
            fprintf(stderr, "%s: record %u is cut short\n", argv[1], r);
            return 2;
        }
        const uint32_t n_slots = cspt::table_slots(n_names);
        int32_t* slots = new int32_t[n_slots];
        int32_t* off32 = new int32_t[n_names + 1];
        if (cspt::build_name_table(name_bytes, offsets.data(), n_names, slots, off32, nullptr) != 0) {
            fprintf(stderr, "%s: record %u names a chromosome twice\n", argv[1], r);
            return 2;
        }
        cspt::Format F;
        int32_t need = 0;
        for (int k = 0; k < 4; ++k) {
            F.col[k] = head[k];
            if (head[k] + 1 > need) need = head[k] + 1;
        }
        F.width = head[4];
        F.need = need;
        F.slot_mask = n_slots - 1;
        F.slots = slots;
        F.name_off = off32;
        F.name_bytes = name_bytes;

        int64_t lines = 0, flagged = -1;
        int32_t reason = 0;
        bool equal = true;
        for (uint32_t start = 0; start < nbytes;) {
            cspt::PlainBytes at = {text + start};
            cspt::Pair p = {0, 0, 0, 0};
            const int32_t verdict = cspt::parse_line(at, (uint64_t)(nbytes - start), F, &p);
            if (verdict != cspt::kOk) {
                if (flagged < 0) flagged = lines, reason = verdict;
            } else if (want_flagged < 0 && lines < want_lines) {
                equal = equal && p.chrom1 == want_c1[lines] && p.pos1 == want_p1[lines] && p.chrom2 == want_c2[lines] && p.pos2 == want_p2[lines];
            }
            ++lines;
            const void* nl = memchr(text + start, '\n', nbytes - start);
            if (!nl) break;
            start = (uint32_t)((const uint8_t*)nl - text) + 1;
        }
        equal = equal && lines == want_lines && flagged == want_flagged && reason == want_reason;
        printf("%lld %lld %d %d\n", (long long)lines, (long long)flagged, (int)reason, (int)equal);
        delete[] text;
        delete[] name_bytes;
        delete[] slots;
        delete[] off32;
    }
    fclose(f);
    return 0;
}
