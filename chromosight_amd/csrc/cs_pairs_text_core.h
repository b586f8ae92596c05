// cs_pairs_text_core.h -- the per-line parser of cs_pairs_text.hip (one body line of a 4DN .pairs file -> chrom1, pos1, chrom2, pos2
// or a reason why not) as one __host__ __device__ function over plain pointers and sizes, and the host-side builder of the name table
// it looks chromosome names up in.  The same function serves a lane on the device (cs_pairs_text.hip: one line per lane, the head of
// the line in LDS) and one thread on the host (tools/pairs_text_check.cpp, built with the sanitizers); where a byte of the line comes
// from goes through a small trait,
//
//   struct Bytes { uint8_t operator()(uint64_t i) const; };          // byte i of the line, for 0 <= i < avail
//
// The grammar (include/chromosight_hip.h states it for callers): the line ends at '\n' or at the end of the text; one '\r' directly
// before the '\n' is dropped; fields are split at '\t'; the line has more fields than its largest column and at most `width`; a
// position is 1 to 18 ASCII digits; a name is not empty and is compared bytewise.  Everything else is flagged with the first
// defect met from the left (field counts and empty fields are met where the field or the line ends).
//
// Bounds.  The line is read through Bytes only, at i < avail and i <= kMaxLineBytes + 1: the scan reads byte i after both were
// checked, the look-ahead behind a '\r' reads byte i + 1 after i + 1 < avail, and the name comparison re-reads bytes of a field the
// scan has passed.  The name table is read at a slot masked to its size (a power of two with at least one empty slot, so a probe
// ends), the offsets at an id the table holds (below n_names, checked when built) and id + 1, the name bytes between two offsets.
// Nothing is written but *out.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CS_PT_HD __host__ __device__ __forceinline__
#else
#define CS_PT_HD inline
#endif

namespace cspt {

enum Reason : int32_t {
    kOk = 0,
    kEmptyLine = 1,         // no byte in front of the terminator
    kTooFewFields = 2,      // fewer than max(columns) + 1
    kTooManyFields = 3,     // more than width
    kEmptyField = 4,        // a name or a position without a byte
    kBadPosition = 5,       // a position that is not 1 to 18 ASCII digits: a sign, a space, '_', a letter, a 19th digit
    kLoneCR = 6,            // a '\r' that does not stand directly before '\n'
    kNulByte = 7,
    kHighByte = 8,          // a byte >= 0x80
    kTooLong = 9            // more than kMaxLineBytes bytes in front of the terminator
};

constexpr uint32_t kMaxLineBytes = 65536;       // cs_pairs_text_max_line_bytes()
constexpr int kMaxDigits = 18;                  // 10^18 - 1 < 2^63
constexpr uint32_t kHashBasis = 2166136261u, kHashPrime = 16777619u;        // FNV-1a over the bytes of a name

struct Format {
    int32_t col[4];                 // the 0-based fields of chr1, pos1, chr2, pos2: distinct, each below width
    int32_t width;                  // the most fields a line may have
    int32_t need;                   // max(col) + 1
    uint32_t slot_mask;             // slots - 1, slots a power of two above n_names
    const int32_t* slots;           // per slot: a name's id, or -1
    const int32_t* name_off;        // n_names + 1 offsets into name_bytes
    const uint8_t* name_bytes;
};

struct Pair {
    int32_t chrom1, chrom2;
    int64_t pos1, pos2;
};

CS_PT_HD uint32_t hash_step(uint32_t h, uint8_t b) { return (h ^ b) * kHashPrime; }

// the id of the name in bytes [start, start + len) of the line, whose hash is h; -1 when the table does not hold it
template <typename Bytes>
CS_PT_HD int32_t lookup_name(const Bytes& at, uint64_t start, uint32_t len, uint32_t h, const Format& F)
{
    for (uint32_t s = h & F.slot_mask;; s = (s + 1) & F.slot_mask) {
        const int32_t id = F.slots[s];
        if (id < 0) return -1;
        const int32_t a = F.name_off[id], b = F.name_off[id + 1];
        if ((uint32_t)(b - a) != len) continue;
        uint32_t j = 0;
        while (j < len && F.name_bytes[a + j] == at(start + j)) ++j;
        if (j == len) return id;
    }
}

// One line: its bytes are at(0 .. ), `avail` of them up to the end of the text (>= 1 for a line that exists; 0 gives kEmptyLine).
// Returns kOk and the pair in *out, or the reason the line is flagged (*out is then unspecified).
template <typename Bytes>
CS_PT_HD int32_t parse_line(const Bytes& at, uint64_t avail, const Format& F, Pair* out)
{
    int32_t field = 0;
    int role = -1;                  // 0 .. 3: the field at hand is col[role]; -1: a field that is only looked through
    for (int k = 0; k < 4; ++k)
        if (F.col[k] == 0) role = k;
    uint64_t start = 0, value = 0;  // of the field at hand: its first byte, its digits so far
    uint32_t len = 0, hash = kHashBasis;
    for (uint64_t i = 0;; ++i) {
        if (i > kMaxLineBytes) return kTooLong;
        bool line_ends = i == avail, field_ends = line_ends;
        if (!line_ends) {
            const uint8_t b = at(i);
            if (b == '\n') {
                line_ends = field_ends = true;
            } else if (b == '\r') {
                if (i + 1 < avail && at(i + 1) == '\n') line_ends = field_ends = true;
                else return kLoneCR;
            } else if (b == '\t') {
                field_ends = true;
            } else if (b == 0) {
                return kNulByte;
            } else if (b >= 0x80) {
                return kHighByte;
            } else {
                if (role == 1 || role == 3) {
                    if (b < '0' || b > '9' || len >= (uint32_t)kMaxDigits) return kBadPosition;
                    value = value * 10 + (uint64_t)(b - '0');
                } else if (role >= 0) {
                    hash = hash_step(hash, b);
                }
                ++len;
            }
        }
        if (!field_ends) continue;
        if (line_ends && i == 0) return kEmptyLine;
        if (role >= 0) {
            if (len == 0) return kEmptyField;
            if (role == 0) out->chrom1 = lookup_name(at, start, len, hash, F);
            else if (role == 1) out->pos1 = (int64_t)value;
            else if (role == 2) out->chrom2 = lookup_name(at, start, len, hash, F);
            else out->pos2 = (int64_t)value;
        }
        ++field;
        if (line_ends) return field < F.need ? kTooFewFields : kOk;
        if (field >= F.width) return kTooManyFields;
        role = -1;
        for (int k = 0; k < 4; ++k)
            if (F.col[k] == field) role = k;
        start = i + 1, value = 0, len = 0, hash = kHashBasis;
    }
}

// the trait over a plain pointer (the host program; the device reads the head of a line from LDS)
struct PlainBytes {
    const uint8_t* p;
    CS_PT_HD uint8_t operator()(uint64_t i) const { return p[i]; }
};

// ---- the name table, built on the host ---------------------------------------------------------------------------------------------
// slots of a table over n_names names: the power of two above twice their number (half of the slots stay empty at the least)
inline uint32_t table_slots(int64_t n_names)
{
    uint32_t s = 16;
    while ((int64_t)s < 2 * n_names + 1) s <<= 1;
    return s;
}

inline uint32_t hash_name(const uint8_t* name, int64_t len)
{
    uint32_t h = kHashBasis;
    for (int64_t j = 0; j < len; ++j) h = hash_step(h, name[j]);
    return h;
}

// Fills slots[0 .. table_slots(n_names)) from n_names names (offsets: n_names + 1 non-decreasing values from 0; name k is bytes
// [offsets[k], offsets[k + 1])) and off32[0 .. n_names].  Returns 0, or 1 for offsets that are not such a list or reach 2^31, 2 for
// a name given twice (the id of the second in *twice).  n_names below 2^30.
inline int build_name_table(const uint8_t* bytes, const int64_t* offsets, int64_t n_names, int32_t* slots, int32_t* off32, int64_t* twice)
{
    const uint32_t n_slots = table_slots(n_names), mask = n_slots - 1;
    for (uint32_t s = 0; s < n_slots; ++s) slots[s] = -1;
    if (offsets[0] != 0) return 1;
    off32[0] = 0;
    for (int64_t k = 0; k < n_names; ++k) {
        if (offsets[k + 1] < offsets[k] || offsets[k + 1] >= ((int64_t)1 << 31)) return 1;
        off32[k + 1] = (int32_t)offsets[k + 1];
    }
    for (int64_t k = 0; k < n_names; ++k) {
        const int64_t a = offsets[k], len = offsets[k + 1] - a;
        uint32_t s = hash_name(bytes + a, len) & mask;
        for (; slots[s] >= 0; s = (s + 1) & mask) {
            const int64_t c = offsets[slots[s]], clen = offsets[slots[s] + 1] - c;
            bool same = clen == len;
            for (int64_t j = 0; same && j < len; ++j) same = bytes[c + j] == bytes[a + j];
            if (same) {
                if (twice) *twice = k;
                return 2;
            }
        }
        slots[s] = (int32_t)k;
    }
    return 0;
}

}  // namespace cspt
