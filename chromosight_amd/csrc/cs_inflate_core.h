// cs_inflate_core.h -- the decoders of cs_inflate.hip as __host__ __device__ functions over plain pointers and sizes: inflate_raw (the
// blocks of RFC 1951), inflate_stream (a zlib stream: RFC 1950 header, that body, Adler-32 trailer) and inflate_member (the body of a
// BGZF member against its ISIZE and CRC-32).  The same control flow serves a wave on the device (cs_inflate.hip:
// the stream's output and the decode tables live in LDS) and one thread on the host (tools/inflate_check.cpp and tools/bgzf_check.cpp, built with the
// sanitizers): whatever is done by "the lanes" goes through a small trait,
//
//   struct Coop { int lane(); int lanes(); void sync(); uint32_t uni(uint32_t); uint64_t sum(uint64_t); uint32_t xor_all(uint32_t); };
//
// lane / lanes: who I am among the lanes that run this call together; sync: everything the lanes have stored is visible to all of
// them; uni: a value that is the same in every lane, said so (the device takes it from the first lane, which lets the compiler keep
// the bit reader in scalar registers); sum / xor_all: the sum / the exclusive or of a value over the lanes, in every lane.
//
// Every lane runs the symbol loop with the same values, so every branch is uniform and every sync is reached by all lanes.  Lane 0
// stores literals and table heads; match copies, stored blocks, table fills and the checksum are spread over the lanes.
//
// Bounds.  The input is read in two places only: BitReader::refill, at pos < nbytes, and the stored-block copy, after
// pos + len <= nbytes was checked.  The output is written in three: a literal after at < cap, a match after at + len <= cap, a stored
// block after at + len <= cap; a match reads [at - dist, at) after dist <= at.  The tables are indexed by a symbol below the size of
// its set (checked where sets are declared), by a length of at most 15 and by table bits of an integer masked to the table's size.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define CS_INF_HD __host__ __device__ __forceinline__
#else
#define CS_INF_HD inline
#endif

namespace csz {

enum Status : int32_t {
    kOk = 0,
    kBadHeader = 1,        // the two bytes of RFC 1950: method, window, check bits, preset dictionary
    kBadBlockType = 2,     // block type 3
    kBadStored = 3,        // LEN != ~NLEN
    kBadCodes = 4,         // a code set zlib refuses (counts, repeats, over-subscribed, incomplete, no end-of-block) or a code outside it
    kBadDistance = 5,      // a distance reaching before the start of the output
    kTooLong = 6,          // more than chunk_bytes of output
    kTooShort = 7,         // the stream ended with less
    kInputEnd = 8,         // the input ended inside the stream
    kBadChecksum = 9,      // Adler-32 (a zlib stream), CRC-32 (a BGZF member)
    kBadChunk = 10,        // cs_inflate.hip: a chunk without gzip whose stored size is not chunk_bytes
    kTrailing = 11         // a BGZF member: bytes of the body span behind the end of the stream
};

constexpr int kLitBits = 10, kDistBits = 8;      // index bits of the two one-step tables
constexpr int kMaxLit = 288, kMaxDist = 32, kMaxBits = 15;

// the decode tables of the block in flight (device: LDS).  fast[]: (symbol << 4) | length for every index whose low `length` bits
// are the code, bit-reversed; 0 where the code is longer than the table's bits (or no code: an incomplete set) -- the canonical
// walk over cnt / sym then decides.
struct Tables {
    uint16_t lit_fast[1 << kLitBits];
    uint16_t dist_fast[1 << kDistBits];
    uint16_t lit_sym[kMaxLit], dist_sym[kMaxDist];
    uint16_t lit_cnt[16], dist_cnt[16];
    uint16_t offs[16], first[16], next[16];     // of the set being built: start of a length's symbols in sym, its first code
    uint8_t lens[kMaxLit + kMaxDist];
    int32_t verdict;                   // of lane 0's part of a build
};

struct BitReader {
    const uint8_t* in;
    uint64_t nbytes, pos;
    uint64_t hold;
    int bits;

    // more than 32 bits in hold, or the rest of the input
    template <typename Coop>
    CS_INF_HD void refill(Coop& co)
    {
        if (bits > 32) return;
        if (pos + 4 <= nbytes) {
            uint32_t w;
            memcpy(&w, in + pos, 4);
            hold |= (uint64_t)co.uni(w) << bits;
            pos += 4;
            bits += 32;
        } else {
            while (bits <= 56 && pos < nbytes) {
                hold |= (uint64_t)co.uni(in[pos++]) << bits;
                bits += 8;
            }
        }
    }
    CS_INF_HD uint32_t peek(int n) const { return (uint32_t)hold & ((1u << n) - 1u); }
    CS_INF_HD void drop(int n)
    {
        hold >>= n;
        bits -= n;
    }
};

// n <= 16 bits into *v; false when the input ends first
template <typename Coop>
CS_INF_HD bool take(BitReader& br, Coop& co, int n, uint32_t* v)
{
    br.refill(co);
    if (br.bits < n) return false;
    *v = br.peek(n);
    br.drop(n);
    return true;
}

CS_INF_HD uint32_t reverse_bits(uint32_t code, int len)
{
    uint32_t r = 0;
    for (int i = 0; i < len; ++i) r |= ((code >> i) & 1u) << (len - 1 - i);
    return r;
}

// The canonical code of lens[0 .. n) into cnt / sym / fast (table of `tbits` index bits).  zlib's rules (inftrees.c): an
// over-subscribed set is refused; an incomplete one too, unless it is a single code of length 1 (`strict`: not even then -- the
// code-length code); a set without any code is taken and decodes nothing.
template <typename Coop>
CS_INF_HD int build_codes(Tables* T, Coop& co, const uint8_t* lens, int n, uint16_t* cnt, uint16_t* sym, uint16_t* fast, int tbits, bool strict)
{
    co.sync();                                                   // lens are stored, the tables of the previous block are done with
    if (co.lane() == 0) {
        for (int l = 0; l <= kMaxBits; ++l) cnt[l] = 0;
        for (int s = 0; s < n; ++s) cnt[lens[s]]++;
        int verdict = kOk, left = 1, maxlen = 0;
        for (int l = 1; l <= kMaxBits; ++l) {
            left = (left << 1) - (int)cnt[l];
            if (left < 0) {
                verdict = kBadCodes;
                break;
            }
            if (cnt[l]) maxlen = l;
        }
        if (verdict == kOk && left > 0 && maxlen != 0 && (strict || maxlen != 1)) verdict = kBadCodes;
        if (verdict == kOk) {
            uint32_t off = 0, code = 0;
            for (int l = 1; l <= kMaxBits; ++l) {
                T->offs[l] = (uint16_t)off;
                T->first[l] = (uint16_t)code;
                off += cnt[l];
                code = (code + cnt[l]) << 1;
            }
            for (int l = 1; l <= kMaxBits; ++l) T->next[l] = T->offs[l];
            for (int s = 0; s < n; ++s)
                if (lens[s]) sym[T->next[lens[s]]++] = (uint16_t)s;
        }
        cnt[0] = 0;                                              // (symbols without a code are no length of the walk)
        T->verdict = verdict;
    }
    for (int i = co.lane(); i < (1 << tbits); i += co.lanes()) fast[i] = 0;
    co.sync();
    const int verdict = (int)co.uni((uint32_t)T->verdict);
    if (verdict != kOk) return verdict;
    int total = 0;
    for (int l = 1; l <= kMaxBits; ++l) total += (int)co.uni(cnt[l]);
    for (int i = co.lane(); i < total; i += co.lanes()) {
        const int s = sym[i], l = lens[s];
        if (l > tbits) continue;
        const uint32_t code = (uint32_t)T->first[l] + (uint32_t)(i - (int)T->offs[l]);
        const uint16_t entry = (uint16_t)((s << 4) | l);
        for (uint32_t j = reverse_bits(code, l); j < (1u << tbits); j += 1u << l) fast[j] = entry;
    }
    co.sync();
    return kOk;
}

// one symbol: >= 0, or -kBadCodes / -kInputEnd
template <typename Coop>
CS_INF_HD int decode_symbol(BitReader& br, Coop& co, const uint16_t* cnt, const uint16_t* sym, const uint16_t* fast, int tbits)
{
    br.refill(co);
    const uint32_t e = co.uni(fast[br.peek(tbits)]);
    const int l = (int)(e & 15u);
    if (l != 0) {
        if (l > br.bits) return -kInputEnd;
        br.drop(l);
        return (int)(e >> 4);
    }
    // the canonical walk, a bit at a time: codes beyond the table's bits, and the verdict on bits that are no code
    int code = 0, first = 0, index = 0;
    for (int len = 1; len <= kMaxBits; ++len) {
        if (len > br.bits) return -kInputEnd;
        code |= (int)((br.hold >> (len - 1)) & 1u);
        const int count = (int)co.uni(cnt[len]);
        if (code - count < first) {
            br.drop(len);
            return (int)co.uni(sym[index + (code - first)]);
        }
        index += count;
        first += count;
        first <<= 1;
        code <<= 1;
    }
    return -kBadCodes;
}

// the order in which the lengths of the code-length code are stored, 5 bits each
CS_INF_HD int code_length_slot(int i)
{
    // 16 17 18 0 8 7 9 6 10 5 11 4 | 12 3 13 2 14 1 15
    const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 |
                        5ull << 45 | 11ull << 50 | 4ull << 55;
    const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return (int)((i < 12 ? lo >> (5 * i) : hi >> (5 * (i - 12))) & 31u);
}

// Adler-32 of out[0 .. n): s1 = 1 + sum d_i, s2 = n + sum (n - i) d_i, both mod 65521.  Every lane sums a strided share, four bytes
// at a time (out is 4-byte aligned), the lanes' sums are added and reduced once: n < 2^24, so a term is below 2^32 and a sum below 2^56.
template <typename Coop>
CS_INF_HD uint32_t adler32(Coop& co, const uint8_t* out, uint32_t n)
{
    uint64_t a = 0, b = 0;
    const uint32_t whole = n & ~3u;
    for (uint32_t i = 4u * (uint32_t)co.lane(); i < whole; i += 4u * (uint32_t)co.lanes()) {
        uint32_t w;
        memcpy(&w, out + i, 4);
        const uint32_t d0 = w & 255u, d1 = (w >> 8) & 255u, d2 = (w >> 16) & 255u, d3 = w >> 24;
        a += d0 + d1 + d2 + d3;
        b += (uint64_t)(n - i) * d0 + (uint64_t)(n - i - 1) * d1 + (uint64_t)(n - i - 2) * d2 + (uint64_t)(n - i - 3) * d3;
    }
    for (uint32_t i = whole + (uint32_t)co.lane(); i < n; i += (uint32_t)co.lanes()) {
        a += out[i];
        b += (uint64_t)(n - i) * out[i];
    }
    a = co.sum(a);
    b = co.sum(b);
    const uint32_t s1 = (uint32_t)((1u + a) % 65521u), s2 = (uint32_t)((n + b) % 65521u);
    return (s2 << 16) | s1;
}

// The blocks of one raw deflate stream (RFC 1951) from the reader's place into out[0 .. cap): kOk with the bytes decoded in *n_out and
// the reader behind the last bit of the final block, or a status (kTooLong: the stream holds more than cap bytes).  cap < 2^24.
template <typename Coop>
CS_INF_HD int inflate_raw(BitReader& br, uint8_t* out, uint32_t cap, uint32_t* n_out, Tables* T, Coop& co)
{
    const uint8_t* in = br.in;
    const uint64_t nbytes = br.nbytes;
    uint32_t v = 0;
    uint32_t at = 0;
    for (bool last = false; !last;) {
        if (!take(br, co, 3, &v)) return kInputEnd;
        last = v & 1u;
        const uint32_t type = v >> 1;
        if (type == 3) return kBadBlockType;
        if (type == 0) {
            br.drop(br.bits & 7);
            if (!take(br, co, 16, &v)) return kInputEnd;
            uint32_t nlen = 0;
            if (!take(br, co, 16, &nlen)) return kInputEnd;
            if ((v ^ 0xFFFFu) != nlen) return kBadStored;
            // whole bytes the reader holds go back to the input
            br.pos -= (uint64_t)(br.bits >> 3);
            br.bits = 0;
            br.hold = 0;
            if (br.pos + v > nbytes) return kInputEnd;
            if (v > cap - at) return kTooLong;
            for (uint32_t i = (uint32_t)co.lane(); i < v; i += (uint32_t)co.lanes()) out[at + i] = in[br.pos + i];
            br.pos += v;
            at += v;
            continue;
        }
        if (type == 1) {
            for (int s = co.lane(); s < kMaxLit + kMaxDist; s += co.lanes())
                T->lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < kMaxLit ? 8 : 5);
            if (int rc = build_codes(T, co, T->lens, kMaxLit, T->lit_cnt, T->lit_sym, T->lit_fast, kLitBits, false)) return rc;
            if (int rc = build_codes(T, co, T->lens + kMaxLit, kMaxDist, T->dist_cnt, T->dist_sym, T->dist_fast, kDistBits, false)) return rc;
        } else {
            if (!take(br, co, 14, &v)) return kInputEnd;
            const int nlen = (int)(v & 31u) + 257, ndist = (int)((v >> 5) & 31u) + 1, ncode = (int)(v >> 10) + 4;
            if (nlen > 286 || ndist > 30) return kBadCodes;
            // the code-length code borrows the distance set's places: its 19 lengths at lens[kMaxLit ..), its tables (codes of at most
            // 7 bits) in dist_cnt / dist_sym / dist_fast
            for (int i = 0; i < 19; ++i) {
                uint32_t l = 0;
                if (i < ncode && !take(br, co, 3, &l)) return kInputEnd;
                if (co.lane() == 0) T->lens[kMaxLit + code_length_slot(i)] = (uint8_t)l;
            }
            if (int rc = build_codes(T, co, T->lens + kMaxLit, 19, T->dist_cnt, T->dist_sym, T->dist_fast, kDistBits, true)) return rc;
            int have = 0, prev = 0;
            while (have < nlen + ndist) {
                const int s = decode_symbol(br, co, T->dist_cnt, T->dist_sym, T->dist_fast, kDistBits);
                if (s < 0) return -s;
                int rep = 1, len = s;
                if (s >= 16) {
                    if (s == 16) {
                        if (have == 0) return kBadCodes;
                        if (!take(br, co, 2, &v)) return kInputEnd;
                        len = prev, rep = 3 + (int)v;
                    } else if (s == 17) {
                        if (!take(br, co, 3, &v)) return kInputEnd;
                        len = 0, rep = 3 + (int)v;
                    } else {
                        if (!take(br, co, 7, &v)) return kInputEnd;
                        len = 0, rep = 11 + (int)v;
                    }
                    if (have + rep > nlen + ndist) return kBadCodes;
                }
                // both sets' lengths behind each other at lens[0 .. nlen + ndist) (at most 316 of the 320; the code-length code's own
                // lengths, which this may reach, went into its tables)
                if (co.lane() == 0)
                    for (int r = 0; r < rep; ++r) T->lens[have + r] = (uint8_t)len;
                have += rep;
                prev = len;
            }
            co.sync();
            if (co.uni(T->lens[256]) == 0) return kBadCodes;                             // no end-of-block code
            // the distance lengths move up to their own place, lens[kMaxLit ..) (nlen <= 286 < kMaxLit): one lane, from the top, so
            // that where the two ranges overlap a length is read before it is overwritten
            if (co.lane() == 0)
                for (int i = ndist - 1; i >= 0; --i) T->lens[kMaxLit + i] = T->lens[nlen + i];
            if (int rc = build_codes(T, co, T->lens, nlen, T->lit_cnt, T->lit_sym, T->lit_fast, kLitBits, false)) return rc;
            if (int rc = build_codes(T, co, T->lens + kMaxLit, ndist, T->dist_cnt, T->dist_sym, T->dist_fast, kDistBits, false)) return rc;
        }
        // the symbols of the block
        for (;;) {
            int s = decode_symbol(br, co, T->lit_cnt, T->lit_sym, T->lit_fast, kLitBits);
            if (s < 0) return -s;
            if (s < 256) {
                if (at >= cap) return kTooLong;
                if (co.lane() == 0) out[at] = (uint8_t)s;
                ++at;
                continue;
            }
            if (s == 256) break;
            if (s > 285) return kBadCodes;
            uint32_t len;
            if (s < 265) len = (uint32_t)s - 254u;
            else if (s == 285) len = 258u;
            else {
                const int e = (s - 261) >> 2;
                if (!take(br, co, e, &v)) return kInputEnd;
                len = 3u + ((4u + (uint32_t)((s - 261) & 3)) << e) + v;
            }
            const int d = decode_symbol(br, co, T->dist_cnt, T->dist_sym, T->dist_fast, kDistBits);
            if (d < 0) return -d;
            if (d > 29) return kBadCodes;
            uint32_t dist;
            if (d < 4) dist = (uint32_t)d + 1u;
            else {
                const int e = (d >> 1) - 1;
                if (!take(br, co, e, &v)) return kInputEnd;
                dist = 1u + ((2u + (uint32_t)(d & 1)) << e) + v;
            }
            if (dist > at) return kBadDistance;
            if (len > cap - at) return kTooLong;
            co.sync();                                           // the literals and matches so far are in place
            const uint8_t* from = out + (at - dist);
            if (dist >= len) {
                for (uint32_t i = (uint32_t)co.lane(); i < len; i += (uint32_t)co.lanes()) out[at + i] = from[i];
            } else {
                // the overlapping copy repeats the `dist` bytes in front of the match: every source lies before it
                for (uint32_t i = (uint32_t)co.lane(); i < len; i += (uint32_t)co.lanes()) out[at + i] = from[i % dist];
            }
            at += len;
        }
    }
    *n_out = at;
    return kOk;
}

// One zlib stream in[0 .. nbytes) into out[0 .. cap): exactly cap bytes, or a status.  Bytes behind the trailer are not looked at
// (zlib.decompress does not either).  cap < 2^24.
template <typename Coop>
CS_INF_HD int inflate_stream(const uint8_t* in, uint64_t nbytes, uint8_t* out, uint32_t cap, Tables* T, Coop& co)
{
    BitReader br = {in, nbytes, 0, 0, 0};
    uint32_t v = 0;
    if (!take(br, co, 16, &v)) return kInputEnd;
    const uint32_t cmf = v & 255u, flg = v >> 8;
    if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u != 0u || (flg & 32u)) return kBadHeader;
    uint32_t at = 0;
    if (int rc = inflate_raw(br, out, cap, &at, T, co)) return rc;
    if (at != cap) return kTooShort;
    // the trailer: byte-aligned, big-endian
    br.drop(br.bits & 7);
    uint32_t want = 0;
    for (int i = 0; i < 4; ++i) {
        if (!take(br, co, 8, &v)) return kInputEnd;
        want = (want << 8) | v;
    }
    co.sync();
    return adler32(co, out, cap) == want ? kOk : kBadChecksum;
}

// ---- CRC-32 (IEEE 802.3, reflected: zlib.crc32) in two parts that combine ---------------------------------------------------------------
// A register value is a polynomial over GF(2) modulo P with bit 31 the coefficient of x^0 (the reflected form).  The remainder of
// a span is what the byte-table loop leaves in a register that started at zero, without the final inversion: linear in the bytes,
// so the remainder of A followed by B is (remainder of A) * x^(8 |B|) + (remainder of B).
constexpr uint32_t kCrcPoly = 0xEDB88320u;

// entry i of the byte table
CS_INF_HD uint32_t crc32_table_entry(uint32_t i)
{
    uint32_t r = i;
    for (int k = 0; k < 8; ++k) r = (r >> 1) ^ (kCrcPoly & (0u - (r & 1u)));
    return r;
}

// the remainder of p[0 .. n) through the 256-entry table
CS_INF_HD uint32_t crc32_span(const uint32_t* table, const uint8_t* p, uint32_t n)
{
    uint32_t r = 0;
    for (uint32_t i = 0; i < n; ++i) r = table[(r ^ p[i]) & 255u] ^ (r >> 8);
    return r;
}

// a * b mod P
CS_INF_HD uint32_t crc32_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int k = 31; k >= 0; --k) {                              // the coefficient of x^(31 - k) of a
        p ^= b & (0u - ((a >> k) & 1u));
        b = (b >> 1) ^ (kCrcPoly & (0u - (b & 1u)));             // b * x
    }
    return p;
}

// r * x^(8 n) mod P: the remainder r of a span once n more bytes stand behind it.  Square and multiply over the bits of n.
CS_INF_HD uint32_t crc32_shift(uint32_t r, uint32_t n)
{
    uint32_t power = 0x00800000u;                                // x^8
    for (; n != 0; n >>= 1) {
        if (n & 1u) r = crc32_mul(r, power);
        if (n > 1u) power = crc32_mul(power, power);
    }
    return r;
}

// where lane `lane` of `lanes` starts in n bytes cut into contiguous shares: a whole number of 4-byte words each, an odd number of
// them (the lanes' reads of their k-th word then fall into different banks of the LDS), the last share that is not empty shorter
CS_INF_HD uint32_t crc32_share_start(uint32_t n, int lane, int lanes)
{
    const uint32_t words = ((n + (uint32_t)lanes - 1u) / (uint32_t)lanes + 3u) / 4u;
    const uint64_t at = (uint64_t)(words | 1u) * 4u * (uint32_t)lane;
    return at < n ? (uint32_t)at : n;
}

// CRC-32 of out[0 .. n) as zlib.crc32 gives it; table: room for 256 entries, built here by the lanes
template <typename Coop>
CS_INF_HD uint32_t crc32(Coop& co, uint32_t* table, const uint8_t* out, uint32_t n)
{
    for (int i = co.lane(); i < 256; i += co.lanes()) table[i] = crc32_table_entry((uint32_t)i);
    co.sync();
    const uint32_t lo = crc32_share_start(n, co.lane(), co.lanes()), hi = crc32_share_start(n, co.lane() + 1, co.lanes());
    uint32_t r = crc32_shift(crc32_span(table, out + lo, hi - lo), n - hi);
    if (co.lane() == 0) r ^= crc32_shift(0xFFFFFFFFu, n);        // the initial value, n bytes on
    return ~co.xor_all(r);
}

// One member of a BGZF file: the raw deflate body in[0 .. nbytes) into out[0 .. isize).  kOk when the body decodes to exactly isize
// bytes, its final block ends inside the last byte of the span and the CRC-32 of the output is `crc`; kTooLong / kTooShort against
// isize, kTrailing for whole bytes of the span behind the end of the stream, kBadChecksum for the CRC.  isize < 2^24.
template <typename Coop>
CS_INF_HD int inflate_member(const uint8_t* in, uint64_t nbytes, uint8_t* out, uint32_t isize, uint32_t crc, Tables* T, uint32_t* crc_table,
                             Coop& co)
{
    BitReader br = {in, nbytes, 0, 0, 0};
    uint32_t at = 0;
    if (int rc = inflate_raw(br, out, isize, &at, T, co)) return rc;
    if (at != isize) return kTooShort;
    if (br.pos - (uint64_t)(br.bits >> 3) != nbytes) return kTrailing;          // (whole bytes the reader holds were not used)
    co.sync();
    return crc32(co, crc_table, out, isize) == crc ? kOk : kBadChecksum;
}
}  // namespace csz
