// cs_subsample.hip -- `--subsample` on the device (include/chromosight_hip.h cs_subsample): every sub-matrix of the resident pixel
// table keeps a multivariate hypergeometric sample of int(sample * total) of its contacts, drawn without replacement, and the kept
// pixels become a new CSR in HBM.  The pools are those of pipeline.DeviceCool.subsampled (the reference's
// preprocessing.py:359-401 subsample_contacts on every block of contacts_map.py:555-596):
//
//   intra block (a, a)   the upper-triangle pixels, diagonal included, plus a mirror copy of every off-diagonal pixel (the
//                        symmetric matrix the reference sees); only the upper copy's share is stored
//   trans block (a < b)  its pixels (inter = 1 only; with inter = 0 trans pixels are dropped)
//
// The draw of a block is a binary split tree over its pixels in table order.  Node (L, j) covers the block positions
// [(j n) >> L, ((j + 1) n) >> L) and, holding k contacts, gives k_left ~ Hypergeometric(N_left, N_right, k) to its left half
// (N = the pool weights under each half: the count on the diagonal and in trans blocks, twice the count off it).  A pixel whose
// leaf holds t contacts and that has a mirror copy keeps Hypergeometric(c, c, t) of them.  Every draw takes its uniforms from
// Philox4x32-10 keyed by the seed and counting over (chrom a, chrom b, node or pixel, draw): the result is a pure function of the
// seed and the table -- the same for any launch shape, context, device, and whichever other blocks are sampled.
//
//   ss_key_kernel       per pixel: truncated int64 count (invalid counts flagged), block id, pool multiplicity
//   radix sort          (block id, table index) pairs: each block's pixels become one run, in table order
//   ss_weight_kernel    pool weights in block order, then an int64 exclusive scan: N of any node is a difference of two entries
//   ss_bounds_kernel    first / last position of every block; ss_total_kernel: the pool total of every block  -> host: keep
//   ss_level_kernel     one launch per level: every node wider than kLeaf pixels splits (nodes keep their k in out[lo])
//   ss_leaf_kernel      one thread per subtree of at most kLeaf pixels finishes it, level by level, in place
//   ss_mirror_kernel    per pixel: the upper / mirror split, the new count, the kept flag
//   exclusive scan of the kept flags, ss_rowptr_kernel, ss_write_kernel: the ordered compaction into the new CSR
//
// No atomics at all: every value is written by exactly one thread, and the scans and the sort are integer ones.
#include <hipcub/hipcub.hpp>

#include "cs_api_internal.h"

using namespace csapi;

namespace {

constexpr int kSsThreads = 256;
constexpr int kLeaf = 32;                   // a subtree of at most kLeaf pixels is finished by one thread
constexpr int kMaxTries = 1 << 16;          // HRUA needs < 2 tries on average; a draw that never accepts is reported, not looped on
constexpr unsigned long long kMirrorBit = 1ull << 62;
constexpr double kMaxCount = 4611686018427387904.0;      // 2^62: counts at or above it are refused (their flag bit)

struct SsBlock {
    long long base, n, keep;                // block positions [base, base + n) of the sorted order; contacts to keep
    int ca, cb;
    int lb;                                 // levels split by ss_level_kernel (nodes of level lb have at most kLeaf pixels)
    int pad;
};

// ---- Philox4x32-10 (Salmon et al., SC'11) -------------------------------------------------------------------------------
struct Philox {
    unsigned k0, k1;                        // the seed
    unsigned c1, c2, c3;                    // node (or pixel) and block; c0 counts the draws

    __device__ __forceinline__ void pair(unsigned c0, double& u, double& v) const
    {
        unsigned x0 = c0, x1 = c1, x2 = c2, x3 = c3, a = k0, b = k1;
#pragma unroll
        for (int r = 0; r < 10; ++r) {
            const unsigned lo0 = 0xD2511F53u * x0, hi0 = __umulhi(0xD2511F53u, x0);
            const unsigned lo1 = 0xCD9E8D57u * x2, hi1 = __umulhi(0xCD9E8D57u, x2);
            x0 = hi1 ^ x1 ^ a;
            x1 = lo1;
            x2 = hi0 ^ x3 ^ b;
            x3 = lo0;
            a += 0x9E3779B9u;
            b += 0xBB67AE85u;
        }
        const unsigned long long p = ((unsigned long long)x0 << 32) | x1, q = ((unsigned long long)x2 << 32) | x3;
        u = (double)((p >> 11) + 1) * 0x1.0p-53;      // (0, 1]
        v = (double)(q >> 11) * 0x1.0p-53;            // [0, 1)
    }
};

__device__ __forceinline__ Philox make_rng(unsigned long long seed, unsigned long long node, int ca, int cb)
{
    Philox r;
    r.k0 = (unsigned)seed;
    r.k1 = (unsigned)(seed >> 32);
    r.c1 = (unsigned)node;
    r.c2 = (unsigned)ca;
    r.c3 = (unsigned)cb;
    return r;
}

// ---- exact hypergeometric draws ----------------------------------------------------------------------------------------
// a * b < c * d for non-negative 64-bit integers, exactly
__device__ __forceinline__ bool prod_less(unsigned long long a, unsigned long long b, unsigned long long c, unsigned long long d)
{
    const unsigned long long h1 = __umul64hi(a, b), h2 = __umul64hi(c, d);
    return h1 < h2 || (h1 == h2 && a * b < c * d);
}

// log(n!) for n < 16
__constant__ double kLogFact[16] = {0.0, 0.0, 0.693147180559945, 1.7917594692280554, 3.178053830347945, 4.787491742782047, 6.579251212010102, 8.525161361065415, 10.604602902745249, 12.801827480081467, 15.104412573075514, 17.502307845873887, 19.987214495661885, 22.55216385312342, 25.191221182738683, 27.89927138384089};

__device__ __forceinline__ double stirling_tail(double z)       // lgamma(z) - ((z - 1/2) log z - z + log(2 pi) / 2), z >= 17: |error| < 2e-12
{
    const double iz = 1.0 / z, iz2 = iz * iz;
    return iz * (1.0 / 12 - iz2 * (1.0 / 360 - iz2 * (1.0 / 1260)));
}

// log(n!), n a non-negative integer below 2^53: a table, else the Stirling series
__device__ __forceinline__ double log_fact(double n)
{
    if (n < 16.0) return kLogFact[(int)n];
    const double z = n + 1.0;
    return (z - 0.5) * log(z) - z + 0.91893853320467274178 + stirling_tail(z);
}

// log((x + d)!) - log(x!), x and x + d non-negative integers below 2^53.  When both are large the difference of the two Stirling
// series is written so that nothing of the size of log(x!) is ever formed: at x ~ 1e12, log(x!) ~ 3e13 keeps only ~4e-3 of
// absolute precision, this form ~1e-8
__device__ __forceinline__ double lf_diff(double x, double d)
{
    const double y = x + d;
    if (fmin(x, y) < 16.0) return log_fact(y) - log_fact(x);
    const double z = x + 1.0, w = y + 1.0;
    return d * log(z) + (w - 0.5) * log1p(d / z) - d + (stirling_tail(w) - stirling_tail(z));
}

// number of "good" among m draws without replacement from g good and b bad, g <= b, 0 < m <= (g + b) / 2
// inversion: min(g, m) < 10, at most 10 steps
__device__ long long hyper_inversion(long long g, long long b, long long m, const Philox& rng)
{
    const double N = (double)(g + b);
    double p = 1.0;
    if (m <= g)
        for (long long i = 0; i < m; ++i) p *= (double)(b - i) / (N - (double)i);
    else
        for (long long i = 0; i < g; ++i) p *= (N - (double)(m + i)) / (N - (double)i);
    double u, unused;
    rng.pair(0, u, unused);
    const long long xmax = min(g, m);
    long long x = 0;
    while (x < xmax && u > p) {
        u -= p;
        p *= (double)(g - x) * (double)(m - x) / ((double)(x + 1) * (double)(b - m + x + 1));
        ++x;
    }
    return x;
}

// HRUA, the ratio-of-uniforms sampler of Stadlober (1989/1990), with an exact integer mode and log-factorial differences in float64
__device__ long long hyper_hrua(long long g, long long b, long long m, const Philox& rng, int* failed)
{
    const double N = (double)(g + b), dg = (double)g, db = (double)b, dm = (double)m;
    const double p = dg / N, q = db / N;
    const double a = dm * p + 0.5;
    const double c = sqrt((N - dm) * dm * p * q / (N - 1.0) + 0.5);
    const double h = 1.7155277699214135 * c + 0.8989161620588988;
    // the mode: floor((m + 1)(g + 1) / (N + 2)), corrected exactly (f(M + 1) >= f(M) <=> (g - M)(m - M) >= (M + 1)(b - m + M + 1))
    long long M = (long long)floor((dm + 1.0) * (dg + 1.0) / (N + 2.0));
    const long long top = min(g, m);
    M = max(0LL, min(M, top));
    while (M < top && !prod_less(g - M, m - M, M + 1, b - m + M + 1)) ++M;
    while (M > 0 && prod_less(g - M + 1, m - M + 1, M, b - m + M)) --M;
    const double dM = (double)M;
    const double bound = fmin((double)top + 1.0, floor(a + 16.0 * c));
    for (unsigned t = 0; t < (unsigned)kMaxTries; ++t) {
        double U, V;
        rng.pair(t, U, V);
        const double X = a + h * (V - 0.5) / U;
        if (!(X >= 0.0) || X >= bound) continue;
        const double K = floor(X), d = K - dM;
        // T = log f(K) - log f(M) <= 0
        double T = 0.0;
#pragma nounroll
        for (int i = 0; i < 4; ++i) {           // one lf_diff body in the code
            const double x = i == 0 ? dM : i == 1 ? dg - dM : i == 2 ? dm - dM : db - dm + dM;
            T -= lf_diff(x, (i == 0 || i == 3) ? d : -d);
        }
        if (U * (4.0 - U) - 3.0 <= T) return (long long)K;
        if (U * (U - T) >= 1.0) continue;
        if (2.0 * log(U) <= T) return (long long)K;
    }
    *failed = 1;
    return M;
}

// Hypergeometric(good, bad, k): good contacts among k drawn without replacement from good + bad
__device__ long long hypergeometric(long long good, long long bad, long long k, const Philox& rng, int* failed)
{
    const long long N = good + bad;
    if (k <= 0 || good <= 0) return 0;
    if (bad <= 0) return k;
    if (k >= N) return good;
    const bool flip = k > N - k;                 // draw the contacts left behind instead
    const long long m = flip ? N - k : k;
    const bool swap = good > bad;
    const long long g = swap ? bad : good, b = swap ? good : bad;
    long long x = min(g, m) < 10 ? hyper_inversion(g, b, m, rng) : hyper_hrua(g, b, m, rng, failed);
    if (swap) x = m - x;
    if (flip) x = good - x;
    return x;
}

// ---- kernels -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int chrom_of(const long long* __restrict__ off, int n_chrom, long long bin)
{
    int lo = 0, hi = n_chrom - 1;               // the last chromosome whose first bin is <= bin
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= bin) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ int block_id(int ca, int cb, int n_chrom, int inter, int n_blocks)
{
    if (cb < ca || (cb > ca && !inter)) return n_blocks;
    if (!inter) return ca;
    return (int)((long long)ca * n_chrom - (long long)ca * (ca - 1) / 2 + (cb - ca));
}

// one wave per row; cnt[k] = truncated count | kMirrorBit for a pixel of an intra block with a mirror copy
template <typename TV>
__global__ __launch_bounds__(kSsThreads) void ss_key_kernel(const long long* __restrict__ indptr, const int* __restrict__ indices,
                                                             const TV* __restrict__ data, int n, const long long* __restrict__ off,
                                                             int n_chrom, int inter, int n_blocks, unsigned long long* __restrict__ cnt,
                                                             int* __restrict__ key, int* __restrict__ iota, int* __restrict__ bad)
{
    const int lane = threadIdx.x & 63;
    const int waves = kSsThreads / 64;
    for (int r = blockIdx.x * waves + (threadIdx.x >> 6); r < n; r += gridDim.x * waves) {
        const int ca = chrom_of(off, n_chrom, r);
        const long long k1 = indptr[r + 1];
        for (long long k = indptr[r] + lane; k < k1; k += 64) {
            const int col = indices[k];
            const double v = (double)data[k];
            if (!(v > -1.0 && v < kMaxCount)) *bad = 1;          // NaN, inf, negative after truncation, or too large
            const unsigned long long c = (v > -1.0 && v < kMaxCount) ? (unsigned long long)(long long)v : 0ull;
            const int cb = (col >= 0 && col < n) ? chrom_of(off, n_chrom, col) : -1;
            const int id = cb < 0 ? n_blocks : block_id(ca, cb, n_chrom, inter, n_blocks);
            cnt[k] = c | ((ca == cb && col != r) ? kMirrorBit : 0ull);
            key[k] = id;
            iota[k] = (int)k;
        }
    }
}

// pool weight of sorted position p (w[nnz] = 0 closes the scan)
__global__ __launch_bounds__(kSsThreads) void ss_weight_kernel(const int* __restrict__ perm, const unsigned long long* __restrict__ cnt,
                                                                long long nnz, long long* __restrict__ w)
{
    for (long long p = blockIdx.x * (long long)kSsThreads + threadIdx.x; p <= nnz; p += (long long)gridDim.x * kSsThreads) {
        if (p == nnz) {
            w[p] = 0;
            continue;
        }
        const unsigned long long c = cnt[perm[p]];
        const long long x = (long long)(c & (kMirrorBit - 1));
        w[p] = (c & kMirrorBit) ? 2 * x : x;
    }
}

// first / end position of every block id (zeroed beforehand: an empty block keeps [0, 0))
__global__ __launch_bounds__(kSsThreads) void ss_bounds_kernel(const int* __restrict__ skey, long long nnz, long long* __restrict__ bstart,
                                                                long long* __restrict__ bend)
{
    for (long long p = blockIdx.x * (long long)kSsThreads + threadIdx.x; p < nnz; p += (long long)gridDim.x * kSsThreads) {
        const int id = skey[p];
        if (p == 0 || skey[p - 1] != id) bstart[id] = p;
        if (p == nnz - 1 || skey[p + 1] != id) bend[id] = p + 1;
    }
}

__global__ __launch_bounds__(kSsThreads) void ss_total_kernel(const long long* __restrict__ E, const long long* __restrict__ bstart,
                                                               const long long* __restrict__ bend, int n_blocks, long long* __restrict__ tot)
{
    for (int b = blockIdx.x * kSsThreads + threadIdx.x; b < n_blocks; b += gridDim.x * kSsThreads)
        tot[b] = E[bend[b]] - E[bstart[b]];
}

__global__ __launch_bounds__(kSsThreads) void ss_root_kernel(const SsBlock* __restrict__ blocks, int n_blocks, long long* __restrict__ out)
{
    for (int b = blockIdx.x * kSsThreads + threadIdx.x; b < n_blocks; b += gridDim.x * kSsThreads)
        if (blocks[b].n > 0) out[blocks[b].base] = blocks[b].keep;
}

// node (L, j) of a block: out[base + lo] holds its k; the left half keeps its share there, the right half's goes to out[base + mid]
__device__ __forceinline__ void split_node(const SsBlock& B, int L, long long j, const long long* __restrict__ E, long long* __restrict__ out,
                                           unsigned long long seed, int* failed)
{
    const long long n = B.n;
    const long long lo = (j * n) >> L, hi = ((j + 1) * n) >> L;
    if (hi - lo < 2) return;
    const long long mid = ((2 * j + 1) * n) >> (L + 1);
    const long long* e = E + B.base;
    const long long nl = e[mid] - e[lo], nr = e[hi] - e[mid];
    const long long k = out[B.base + lo];
    const Philox rng = make_rng(seed, (1ull << L) + (unsigned long long)j, B.ca, B.cb);
    const long long kl = hypergeometric(nl, nr, k, rng, failed);
    out[B.base + lo] = kl;
    out[B.base + mid] = k - kl;
}

// level L of the blocks listed in `active` (all of them have 2^L nodes at this level, each wider than kLeaf pixels)
__global__ __launch_bounds__(kSsThreads) void ss_level_kernel(const SsBlock* __restrict__ blocks, const int* __restrict__ active,
                                                               long long n_threads, int L, const long long* __restrict__ E,
                                                               long long* __restrict__ out, unsigned long long seed, int* __restrict__ failed)
{
    for (long long t = blockIdx.x * (long long)kSsThreads + threadIdx.x; t < n_threads; t += (long long)gridDim.x * kSsThreads) {
        const SsBlock B = blocks[active[t >> L]];
        split_node(B, L, t & ((1LL << L) - 1), E, out, seed, failed);
    }
}

// one thread per node of level lb of every non-empty block (leaf_off: prefix of 2^lb over leaf_blocks): the whole subtree, a level
// at a time (nodes of a level are disjoint; a level whose nodes all hold at most one pixel ends the subtree)
__global__ __launch_bounds__(kSsThreads) void ss_leaf_kernel(const SsBlock* __restrict__ blocks, const int* __restrict__ leaf_blocks,
                                                              const long long* __restrict__ leaf_off, int n_leaf_blocks,
                                                              const long long* __restrict__ E, long long* __restrict__ out,
                                                              unsigned long long seed, int* __restrict__ failed)
{
    const long long n_threads = leaf_off[n_leaf_blocks];
    for (long long t = blockIdx.x * (long long)kSsThreads + threadIdx.x; t < n_threads; t += (long long)gridDim.x * kSsThreads) {
        int lo = 0, hi = n_leaf_blocks - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (leaf_off[mid] <= t) lo = mid;
            else hi = mid - 1;
        }
        const SsBlock B = blocks[leaf_blocks[lo]];
        const long long j0 = t - leaf_off[lo];
        for (int L = B.lb; L < 62; ++L) {
            const int depth = L - B.lb;
            // node sizes of a level differ by at most one: the widest is ceil(n / 2^L)
            if (((B.n + (1LL << L) - 1) >> L) < 2) break;
            for (long long j = j0 << depth; j < (j0 + 1) << depth; ++j) split_node(B, L, j, E, out, seed, failed);
        }
    }
}

// sorted position p: t = the pixel's share of the pool draw; a pixel with a mirror copy keeps Hypergeometric(c, c, t) of it
__global__ __launch_bounds__(kSsThreads) void ss_mirror_kernel(const int* __restrict__ skey, const int* __restrict__ perm,
                                                                const unsigned long long* __restrict__ cnt, const SsBlock* __restrict__ blocks,
                                                                const long long* __restrict__ out, long long n_sampled, unsigned long long seed,
                                                                long long* __restrict__ fresh, int* __restrict__ kept, long long* __restrict__ drawn,
                                                                int* __restrict__ failed)
{
    for (long long p = blockIdx.x * (long long)kSsThreads + threadIdx.x; p < n_sampled; p += (long long)gridDim.x * kSsThreads) {
        const int k = perm[p];
        const unsigned long long c = cnt[k];
        const long long t = out[p];
        long long x = t;
        if ((c & kMirrorBit) && t > 0) {
            const SsBlock B = blocks[skey[p]];
            const long long cc = (long long)(c & (kMirrorBit - 1));
            // pixel draws count over the block position, node draws over the heap index: the top bit of c2 keeps them apart
            const Philox rng = make_rng(seed, (unsigned long long)(p - B.base), (int)((unsigned)B.ca | 0x80000000u), B.cb);
            x = hypergeometric(cc, cc, t, rng, failed);
        }
        fresh[k] = x;
        kept[k] = x > 0;
        if (drawn) drawn[k] = t;
    }
}

__global__ __launch_bounds__(kSsThreads) void ss_rowptr_kernel(const long long* __restrict__ indptr, const int* __restrict__ pos, int n,
                                                                long long* __restrict__ out_indptr)
{
    for (int r = blockIdx.x * kSsThreads + threadIdx.x; r <= n; r += gridDim.x * kSsThreads) out_indptr[r] = pos[indptr[r]];
}

template <typename TO>
__global__ __launch_bounds__(kSsThreads) void ss_write_kernel(const int* __restrict__ indices, const long long* __restrict__ fresh,
                                                               const int* __restrict__ kept, const int* __restrict__ pos, long long nnz,
                                                               int* __restrict__ out_indices, TO* __restrict__ out_data)
{
    for (long long k = blockIdx.x * (long long)kSsThreads + threadIdx.x; k < nnz; k += (long long)gridDim.x * kSsThreads) {
        if (!kept[k]) continue;
        const int at = pos[k];
        out_indices[at] = indices[k];
        out_data[at] = (TO)fresh[k];
    }
}

// device allocations of one call, freed on every way out (hipFree waits for the work that uses them)
struct CallBuffers {
    std::vector<void*> p;
    ~CallBuffers()
    {
        for (void* q : p) (void)hipFree(q);
    }
    template <typename T>
    hipError_t get(T** out, size_t count)
    {
        void* q = nullptr;
        hipError_t e = hipMalloc(&q, std::max<size_t>(count * sizeof(T), 1));
        if (e == hipSuccess) p.push_back(q);
        *out = (T*)q;
        return e;
    }
};

int grid_for(long long items, int n_cu)
{
    return (int)std::max(1LL, std::min<long long>((items + kSsThreads - 1) / kSsThreads, 32LL * std::max(n_cu, 1)));
}

}  // namespace

extern "C" {

int cs_subsample(cs_ctx* ctx, void* stream_, const cs_csr* g, const int64_t* chrom_offsets, int32_t n_chrom, const cs_subsample_params* p,
                 cs_csr* out, int64_t* h_out_nnz, cs_subsample_block* h_blocks, int64_t* d_drawn)
{
    CS_ENTER(ctx);
    hipStream_t stream = (hipStream_t)stream_;
    if (!g || !p || !out || !h_out_nnz || !h_blocks || !chrom_offsets) return fail(ctx, CS_ERR_INVALID, "cs_subsample: null argument");
    if (g->dtype != CS_F32 && g->dtype != CS_F64) return fail(ctx, CS_ERR_INVALID, "cs_subsample: bad table dtype");
    if (g->n_rows < 0 || g->n_rows != g->n_cols || g->col0 != 0 || g->d_row_end || g->d_row_weight || g->d_col_weight)
        return fail(ctx, CS_ERR_INVALID, "cs_subsample takes the whole-genome pixel table (square, plain row pointers, no weights)");
    if (!g->d_indptr || g->nnz < 0 || (g->nnz > 0 && (!g->d_indices || !g->d_data)))
        return fail(ctx, CS_ERR_INVALID, "cs_subsample: null table arrays");
    if (!out->d_indptr || (g->nnz > 0 && (!out->d_indices || !out->d_data)))
        return fail(ctx, CS_ERR_INVALID, "cs_subsample: null output arrays");
    if (g->nnz >= (int64_t)std::numeric_limits<int>::max())
        return fail(ctx, CS_ERR_UNSUPPORTED, "cs_subsample: tables of 2^31 - 1 pixels or more");
    if (!(p->sample >= 0.0)) return fail(ctx, CS_ERR_INVALID, "Subsample must be strictly positive.");
    if (!(p->sample <= 1.0)) return fail(ctx, CS_ERR_INVALID, "Subsample cannot be above 1");
    if (p->reserved != 0) return fail(ctx, CS_ERR_INVALID, "cs_subsample: reserved must be 0");
    const int n = g->n_rows;
    if (n_chrom < 1 || chrom_offsets[0] != 0 || chrom_offsets[n_chrom] != n)
        return fail(ctx, CS_ERR_INVALID, "cs_subsample: %d chromosome offsets must run from 0 to the %d bins", (int)n_chrom + 1, n);
    for (int c = 0; c < n_chrom; ++c)
        if (chrom_offsets[c + 1] < chrom_offsets[c]) return fail(ctx, CS_ERR_INVALID, "cs_subsample: decreasing chromosome offsets");
    const bool inter = p->inter != 0;
    const long long n_blocks_ll = inter ? (long long)n_chrom * (n_chrom + 1) / 2 : n_chrom;
    if (n_blocks_ll >= (long long)std::numeric_limits<int>::max() / 2)
        return fail(ctx, CS_ERR_UNSUPPORTED, "cs_subsample: too many sub-matrices (%lld)", n_blocks_ll);
    const int n_blocks = (int)n_blocks_ll;
    const long long nnz = g->nnz;
    const unsigned long long seed = p->seed;
    // block list in (chrom1, chrom2) row-major order
    for (int ca = 0, b = 0; ca < n_chrom; ++ca)
        for (int cb = ca; cb < (inter ? n_chrom : ca + 1); ++cb, ++b) h_blocks[b] = cs_subsample_block{ca, cb, 0, 0};
    out->n_rows = out->n_cols = n;
    out->col0 = 0;
    out->d_row_end = nullptr;
    out->d_row_weight = out->d_col_weight = nullptr;
    if (nnz == 0) {
        CS_HIP(ctx, hipMemsetAsync((void*)out->d_indptr, 0, ((size_t)n + 1) * sizeof(long long), stream));
        CS_HIP(ctx, hipStreamSynchronize(stream));
        out->nnz = 0;
        out->dtype = CS_F32;
        *h_out_nnz = 0;
        return CS_OK;
    }

    CallBuffers Bf;
    long long *d_off = nullptr, *E = nullptr, *bstart = nullptr, *bend = nullptr, *tot = nullptr, *outk = nullptr, *fresh = nullptr,
              *d_max = nullptr;
    unsigned long long* cnt = nullptr;
    int *key = nullptr, *iota = nullptr, *skey = nullptr, *perm = nullptr, *flags = nullptr, *bad = nullptr;
    int end_bit = 1;
    while (end_bit < 31 && (1LL << end_bit) <= n_blocks) ++end_bit;
    // hipcub scratch: the largest of the four queries
    size_t b_sort = 0, b_scan64 = 0, b_scan32 = 0, b_max = 0;
    CS_HIP(ctx, hipcub::DeviceRadixSort::SortPairs(nullptr, b_sort, (const int*)nullptr, (int*)nullptr, (const int*)nullptr, (int*)nullptr,
                                                   (int)nnz, 0, end_bit, stream));
    CS_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, b_scan64, (const long long*)nullptr, (long long*)nullptr, (int)nnz + 1, stream));
    CS_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, b_scan32, (const int*)nullptr, (int*)nullptr, (int)nnz + 1, stream));
    CS_HIP(ctx, hipcub::DeviceReduce::Max(nullptr, b_max, (const long long*)nullptr, (long long*)nullptr, (int)nnz, stream));
    const size_t tmp_bytes = std::max(std::max(b_sort, b_scan64), std::max(b_scan32, b_max));
    unsigned char* tmp = nullptr;
    CS_HIP(ctx, Bf.get(&tmp, tmp_bytes));
    CS_HIP(ctx, Bf.get(&d_off, (size_t)n_chrom + 1));
    CS_HIP(ctx, Bf.get(&cnt, (size_t)nnz));
    CS_HIP(ctx, Bf.get(&key, (size_t)nnz));
    CS_HIP(ctx, Bf.get(&iota, (size_t)nnz));
    CS_HIP(ctx, Bf.get(&skey, (size_t)nnz));
    CS_HIP(ctx, Bf.get(&perm, (size_t)nnz));
    CS_HIP(ctx, Bf.get(&E, (size_t)nnz + 1));
    CS_HIP(ctx, Bf.get(&outk, (size_t)nnz + 1));
    CS_HIP(ctx, Bf.get(&bstart, (size_t)n_blocks + 1));
    CS_HIP(ctx, Bf.get(&bend, (size_t)n_blocks + 1));
    CS_HIP(ctx, Bf.get(&tot, (size_t)n_blocks));
    CS_HIP(ctx, Bf.get(&bad, 2));
    CS_HIP(ctx, Bf.get(&d_max, 1));
    const int n_cu = ctx->n_cu;
    CS_HIP(ctx, hipMemcpyAsync(d_off, chrom_offsets, ((size_t)n_chrom + 1) * sizeof(long long), hipMemcpyHostToDevice, stream));
    CS_HIP(ctx, hipMemsetAsync(bad, 0, 2 * sizeof(int), stream));
    CS_HIP(ctx, hipMemsetAsync(bstart, 0, ((size_t)n_blocks + 1) * sizeof(long long), stream));
    CS_HIP(ctx, hipMemsetAsync(bend, 0, ((size_t)n_blocks + 1) * sizeof(long long), stream));

    // 1. counts, block ids, sort into block runs, pool prefix sums, block totals
    {
        const int grid = (int)std::max(1LL, std::min<long long>(((long long)n + 3) / 4, 32LL * std::max(n_cu, 1)));
        if (g->dtype == CS_F64)
            hipLaunchKernelGGL(ss_key_kernel<double>, dim3(grid), dim3(kSsThreads), 0, stream, (const long long*)g->d_indptr, g->d_indices,
                               (const double*)g->d_data, n, d_off, (int)n_chrom, (int)inter, n_blocks, cnt, key, iota, bad);
        else
            hipLaunchKernelGGL(ss_key_kernel<float>, dim3(grid), dim3(kSsThreads), 0, stream, (const long long*)g->d_indptr, g->d_indices,
                               (const float*)g->d_data, n, d_off, (int)n_chrom, (int)inter, n_blocks, cnt, key, iota, bad);
        CS_HIP(ctx, hipGetLastError());
    }
    size_t bytes = tmp_bytes;
    CS_HIP(ctx, hipcub::DeviceRadixSort::SortPairs(tmp, bytes, key, skey, iota, perm, (int)nnz, 0, end_bit, stream));
    hipLaunchKernelGGL(ss_weight_kernel, dim3(grid_for(nnz + 1, n_cu)), dim3(kSsThreads), 0, stream, perm, cnt, nnz, outk);
    CS_HIP(ctx, hipGetLastError());
    bytes = tmp_bytes;
    CS_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(tmp, bytes, outk, E, (int)nnz + 1, stream));
    hipLaunchKernelGGL(ss_bounds_kernel, dim3(grid_for(nnz, n_cu)), dim3(kSsThreads), 0, stream, skey, nnz, bstart, bend);
    CS_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(ss_total_kernel, dim3(grid_for(n_blocks, n_cu)), dim3(kSsThreads), 0, stream, E, bstart, bend, n_blocks, tot);
    CS_HIP(ctx, hipGetLastError());
    std::vector<long long> h_start((size_t)n_blocks + 1), h_end((size_t)n_blocks + 1), h_tot((size_t)n_blocks);
    int h_bad[2] = {0, 0};
    CS_HIP(ctx, hipMemcpyAsync(h_start.data(), bstart, h_start.size() * sizeof(long long), hipMemcpyDeviceToHost, stream));
    CS_HIP(ctx, hipMemcpyAsync(h_end.data(), bend, h_end.size() * sizeof(long long), hipMemcpyDeviceToHost, stream));
    CS_HIP(ctx, hipMemcpyAsync(h_tot.data(), tot, h_tot.size() * sizeof(long long), hipMemcpyDeviceToHost, stream));
    CS_HIP(ctx, hipMemcpyAsync(h_bad, bad, sizeof(h_bad), hipMemcpyDeviceToHost, stream));
    CS_HIP(ctx, hipStreamSynchronize(stream));
    if (h_bad[0]) return fail(ctx, CS_ERR_INVALID, "cs_subsample: counts must be finite, non-negative and below 2^62");

    // 2. keep = int(sample * total) per block (the host path's float64 product), the level lists and the subtrees
    std::vector<SsBlock> blk((size_t)n_blocks);
    std::vector<std::vector<int>> levels;
    std::vector<int> leaf_blocks;
    std::vector<long long> leaf_off(1, 0);
    long long n_sampled = 0;
    for (int b = 0; b < n_blocks; ++b) {
        SsBlock& B = blk[(size_t)b];
        B.base = h_start[(size_t)b];
        B.n = h_end[(size_t)b] - h_start[(size_t)b];
        const long long total = h_tot[(size_t)b];
        const long long keep = (long long)(p->sample * (double)total);
        B.keep = std::min(std::max(keep, 0LL), total);
        B.ca = h_blocks[b].chrom1;
        B.cb = h_blocks[b].chrom2;
        B.pad = 0;
        h_blocks[b].total = total;
        h_blocks[b].keep = B.keep;
        int lb = 0;
        while (((B.n + (1LL << lb) - 1) >> lb) > kLeaf) ++lb;
        B.lb = lb;
        n_sampled = std::max(n_sampled, h_end[(size_t)b]);
        if (B.n == 0) continue;
        if ((int)levels.size() < lb) levels.resize((size_t)lb);
        for (int L = 0; L < lb; ++L) levels[(size_t)L].push_back(b);
        leaf_blocks.push_back(b);
        leaf_off.push_back(leaf_off.back() + (1LL << lb));
    }
    std::vector<int> level_flat;
    std::vector<size_t> level_at;
    for (auto& v : levels) {
        level_at.push_back(level_flat.size());
        level_flat.insert(level_flat.end(), v.begin(), v.end());
    }
    SsBlock* d_blk = nullptr;
    int *d_levels = nullptr, *d_leaf_blocks = nullptr;
    long long* d_leaf_off = nullptr;
    CS_HIP(ctx, Bf.get(&d_blk, blk.size()));
    CS_HIP(ctx, Bf.get(&d_levels, level_flat.size()));
    CS_HIP(ctx, Bf.get(&d_leaf_blocks, leaf_blocks.size()));
    CS_HIP(ctx, Bf.get(&d_leaf_off, leaf_off.size()));
    CS_HIP(ctx, hipMemcpyAsync(d_blk, blk.data(), blk.size() * sizeof(SsBlock), hipMemcpyHostToDevice, stream));
    if (!level_flat.empty())
        CS_HIP(ctx, hipMemcpyAsync(d_levels, level_flat.data(), level_flat.size() * sizeof(int), hipMemcpyHostToDevice, stream));
    if (!leaf_blocks.empty()) {
        CS_HIP(ctx, hipMemcpyAsync(d_leaf_blocks, leaf_blocks.data(), leaf_blocks.size() * sizeof(int), hipMemcpyHostToDevice, stream));
    }
    CS_HIP(ctx, hipMemcpyAsync(d_leaf_off, leaf_off.data(), leaf_off.size() * sizeof(long long), hipMemcpyHostToDevice, stream));

    // 3. the split trees: the levels of the wide nodes, then the subtrees
    hipLaunchKernelGGL(ss_root_kernel, dim3(grid_for(n_blocks, n_cu)), dim3(kSsThreads), 0, stream, d_blk, n_blocks, outk);
    CS_HIP(ctx, hipGetLastError());
    for (size_t L = 0; L < levels.size(); ++L) {
        const long long n_threads = (long long)levels[L].size() << L;
        hipLaunchKernelGGL(ss_level_kernel, dim3(grid_for(n_threads, n_cu)), dim3(kSsThreads), 0, stream, d_blk, d_levels + level_at[L],
                           n_threads, (int)L, E, outk, seed, bad + 1);
        CS_HIP(ctx, hipGetLastError());
    }
    if (!leaf_blocks.empty()) {
        hipLaunchKernelGGL(ss_leaf_kernel, dim3(grid_for(leaf_off.back(), n_cu)), dim3(kSsThreads), 0, stream, d_blk, d_leaf_blocks,
                           d_leaf_off, (int)leaf_blocks.size(), E, outk, seed, bad + 1);
        CS_HIP(ctx, hipGetLastError());
    }

    // 4. upper / mirror split, kept flags (table order), ordered compaction
    CS_HIP(ctx, Bf.get(&fresh, (size_t)nnz));
    CS_HIP(ctx, Bf.get(&flags, (size_t)nnz + 1));
    int* pos = nullptr;
    CS_HIP(ctx, Bf.get(&pos, (size_t)nnz + 1));
    CS_HIP(ctx, hipMemsetAsync(fresh, 0, (size_t)nnz * sizeof(long long), stream));
    CS_HIP(ctx, hipMemsetAsync(flags, 0, ((size_t)nnz + 1) * sizeof(int), stream));
    if (d_drawn) CS_HIP(ctx, hipMemsetAsync(d_drawn, 0, (size_t)nnz * sizeof(long long), stream));
    if (n_sampled > 0) {
        hipLaunchKernelGGL(ss_mirror_kernel, dim3(grid_for(n_sampled, n_cu)), dim3(kSsThreads), 0, stream, skey, perm, cnt, d_blk, outk,
                           n_sampled, seed, fresh, flags, (long long*)d_drawn, bad + 1);
        CS_HIP(ctx, hipGetLastError());
    }
    bytes = tmp_bytes;
    CS_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(tmp, bytes, flags, pos, (int)nnz + 1, stream));
    bytes = tmp_bytes;
    CS_HIP(ctx, hipcub::DeviceReduce::Max(tmp, bytes, fresh, d_max, (int)nnz, stream));
    long long* out_indptr = (long long*)out->d_indptr;
    hipLaunchKernelGGL(ss_rowptr_kernel, dim3(grid_for((long long)n + 1, n_cu)), dim3(kSsThreads), 0, stream, (const long long*)g->d_indptr,
                       pos, n, out_indptr);
    CS_HIP(ctx, hipGetLastError());
    int h_kept = 0;
    long long h_max = 0;
    CS_HIP(ctx, hipMemcpyAsync(&h_kept, pos + nnz, sizeof(int), hipMemcpyDeviceToHost, stream));
    CS_HIP(ctx, hipMemcpyAsync(&h_max, d_max, sizeof(long long), hipMemcpyDeviceToHost, stream));
    CS_HIP(ctx, hipMemcpyAsync(h_bad, bad, sizeof(h_bad), hipMemcpyDeviceToHost, stream));
    CS_HIP(ctx, hipStreamSynchronize(stream));
    if (h_bad[1]) return fail(ctx, CS_ERR_HIP, "cs_subsample: a hypergeometric draw did not accept in %d tries", kMaxTries);

    // 5. the kept pixels, in table order: float32 when every count is below 2^24 (pipeline.DeviceCool's rule), else float64
    const int dtype = h_max < (1LL << 24) ? CS_F32 : CS_F64;
    if (dtype == CS_F32)
        hipLaunchKernelGGL(ss_write_kernel<float>, dim3(grid_for(nnz, n_cu)), dim3(kSsThreads), 0, stream, g->d_indices, fresh, flags, pos, nnz,
                           (int*)out->d_indices, (float*)out->d_data);
    else
        hipLaunchKernelGGL(ss_write_kernel<double>, dim3(grid_for(nnz, n_cu)), dim3(kSsThreads), 0, stream, g->d_indices, fresh, flags, pos,
                           nnz, (int*)out->d_indices, (double*)out->d_data);
    CS_HIP(ctx, hipGetLastError());
    CS_HIP(ctx, hipStreamSynchronize(stream));
    out->nnz = h_kept;
    out->dtype = dtype;
    *h_out_nnz = h_kept;
    return CS_OK;
}

}  // extern "C"
