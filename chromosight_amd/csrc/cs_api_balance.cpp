// cs_api_balance.cpp -- the C ABI of ICE balancing (include/chromosight_hip.h cs_ice_balance): validation, the chunk / span
// tables, the filters that need medians (on the host: n_bins doubles down once, the initial weights up once) and the launch
// chain of cs_balance.hip.  Two host synchronisations per call, whatever the number of iterations.
#include "cs_api_internal.h"

using namespace csapi;

namespace {

// np.median: the mean of the two middle values for an even count, NaN for none
double median_of(std::vector<double> v)
{
    if (v.empty()) return std::numeric_limits<double>::quiet_NaN();
    const size_t h = v.size() / 2;
    std::nth_element(v.begin(), v.begin() + h, v.end());
    const double hi = v[h];
    if (v.size() & 1) return hi;
    const double lo = *std::max_element(v.begin(), v.begin() + h);
    return (lo + hi) / 2.0;
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

}  // namespace

extern "C" {

int cs_ice_balance(cs_ctx* ctx, void* stream_, const cs_csr* g, const int64_t* chrom_offsets, int32_t n_chrom,
                   const cs_ice_params* p, double* d_bias, cs_ice_span_stats* h_stats)
{
    CS_ENTER(ctx);
    hipStream_t stream = (hipStream_t)stream_;
    if (!g || !p || !d_bias || !h_stats || !chrom_offsets) return fail(ctx, CS_ERR_INVALID, "cs_ice_balance: null argument");
    if (g->dtype != CS_F32 && g->dtype != CS_F64) return fail(ctx, CS_ERR_INVALID, "cs_ice_balance: bad table dtype");
    if (g->n_rows < 0 || g->n_rows != g->n_cols || g->col0 != 0 || g->d_row_end || g->d_row_weight || g->d_col_weight)
        return fail(ctx, CS_ERR_INVALID, "cs_ice_balance takes the whole-genome pixel table (square, plain row pointers, no weights)");
    if (!g->d_indptr || (g->nnz > 0 && (!g->d_indices || !g->d_data)) || g->nnz < 0)
        return fail(ctx, CS_ERR_INVALID, "cs_ice_balance: null table arrays");
    if (g->nnz > (int64_t)std::numeric_limits<int>::max())
        return fail(ctx, CS_ERR_UNSUPPORTED, "cs_ice_balance: tables of 2^31 pixels or more");
    const int n = g->n_rows;
    if (n_chrom < 1 || chrom_offsets[0] != 0 || chrom_offsets[n_chrom] != n)
        return fail(ctx, CS_ERR_INVALID, "cs_ice_balance: %d chromosome offsets must run from 0 to the %d bins", (int)n_chrom + 1, n);
    for (int c = 0; c < n_chrom; ++c)
        if (chrom_offsets[c + 1] < chrom_offsets[c]) return fail(ctx, CS_ERR_INVALID, "cs_ice_balance: decreasing chromosome offsets");
    if (!(p->tol > 0.0)) return fail(ctx, CS_ERR_INVALID, "cs_ice_balance: tol must be > 0");
    if (p->max_iters < 1) return fail(ctx, CS_ERR_INVALID, "cs_ice_balance: max_iters must be >= 1");
    if (p->ignore_diags < 0 || p->min_nnz < 0 || !(p->min_count >= 0.0) || !(p->mad_max >= 0.0))
        return fail(ctx, CS_ERR_INVALID, "cs_ice_balance: ignore_diags, min_nnz, min_count and mad_max must be >= 0");
    if (p->reserved != 0) return fail(ctx, CS_ERR_INVALID, "cs_ice_balance: reserved must be 0");
    const bool cis = p->cis_only != 0;
    const int n_spans = cis ? n_chrom : 1;
    const long long nnz = g->nnz;
    const size_t vbytes = g->dtype == CS_F64 ? 8 : 4;

    // chunks of at most kIceChunk bins inside one chromosome; the columns a row keeps end with its chromosome (cis_only)
    std::vector<cs::IceChunk> chunks;
    std::vector<int> span_chunk0(1, 0), bin_lim((size_t)std::max(n, 1));
    for (int c = 0; c < n_chrom; ++c) {
        const int lo = (int)chrom_offsets[c], hi = (int)chrom_offsets[c + 1];
        const int lim = cis ? hi : n;
        for (int b = lo; b < hi; b += cs::kIceChunk) chunks.push_back({b, std::min(hi, b + cs::kIceChunk), cis ? c : 0, lim});
        for (int b = lo; b < hi; ++b) bin_lim[(size_t)b] = lim;
        if (cis) span_chunk0.push_back((int)chunks.size());
    }
    if (!cis) span_chunk0.push_back((int)chunks.size());
    int end_bit = 1;
    while (end_bit < 31 && (1LL << end_bit) <= n) ++end_bit;

    CallBuffers B;
    cs::IceDev D{};
    D.n = n;
    D.n_chunks = (int)chunks.size();
    D.n_spans = n_spans;
    D.ignore_diags = p->ignore_diags;
    D.nnz = nnz;
    D.indptr = (const long long*)g->d_indptr;
    D.indices = g->d_indices;
    D.bias = d_bias;
    D.tol = p->tol;
    D.max_iters = p->max_iters;
    D.rescale = p->rescale_marginals != 0;
    cs::IceChunk* d_chunks = nullptr;
    int *d_span0 = nullptr, *d_lim = nullptr, *rowid = nullptr, *iota = nullptr, *col_sorted = nullptr, *perm = nullptr, *bad = nullptr;
    unsigned char* csc_val = nullptr;
    void* sort_tmp = nullptr;
    const size_t sort_bytes = cs::ice_sort_scratch_bytes(nnz, end_bit);
    if (nnz > 0 && sort_bytes == 0) return fail(ctx, CS_ERR_HIP, "cs_ice_balance: radix sort size query failed");
    CS_HIP(ctx, B.get(&d_chunks, chunks.size()));
    CS_HIP(ctx, B.get(&d_span0, span_chunk0.size()));
    CS_HIP(ctx, B.get(&d_lim, bin_lim.size()));
    CS_HIP(ctx, B.get(&D.colptr, (size_t)n + 1));
    CS_HIP(ctx, B.get(&D.csc_row, (size_t)nnz));
    CS_HIP(ctx, B.get(&csc_val, (size_t)nnz * vbytes));
    CS_HIP(ctx, B.get(&rowid, (size_t)nnz));
    CS_HIP(ctx, B.get(&iota, (size_t)nnz));
    CS_HIP(ctx, B.get(&col_sorted, (size_t)nnz));
    CS_HIP(ctx, B.get(&perm, (size_t)nnz));
    CS_HIP(ctx, B.get((unsigned char**)&sort_tmp, sort_bytes));
    CS_HIP(ctx, B.get(&D.marg, (size_t)n));
    CS_HIP(ctx, B.get(&D.marg_nnz, (size_t)n));
    CS_HIP(ctx, B.get(&D.part, 3 * chunks.size()));
    CS_HIP(ctx, B.get(&D.st, (size_t)n_spans));
    CS_HIP(ctx, B.get(&D.ctl, 2));
    CS_HIP(ctx, B.get(&bad, 1));
    D.chunks = d_chunks;
    D.span_chunk0 = d_span0;
    CS_HIP(ctx, hipMemcpyAsync(d_chunks, chunks.data(), chunks.size() * sizeof(cs::IceChunk), hipMemcpyHostToDevice, stream));
    CS_HIP(ctx, hipMemcpyAsync(d_span0, span_chunk0.data(), span_chunk0.size() * sizeof(int), hipMemcpyHostToDevice, stream));
    CS_HIP(ctx, hipMemcpyAsync(d_lim, bin_lim.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, stream));
    CS_HIP(ctx, hipMemsetAsync(bad, 0, sizeof(int), stream));

    // 1. CSC permutation and the filtered marginals (no weights)
    int rc = cs::ice_prepare(D, g->d_data, g->dtype == CS_F64, csc_val, d_lim, rowid, iota, col_sorted, perm, sort_tmp, sort_bytes,
                             end_bit, bad, ctx->n_cu, stream);
    if (rc) return fail(ctx, CS_ERR_HIP, "cs_ice_balance: preparation launches failed: %s", hipGetErrorString((hipError_t)rc));
    std::vector<double> marg((size_t)n), nnzm((size_t)n);
    int h_bad = 0;
    CS_HIP(ctx, hipMemcpyAsync(marg.data(), D.marg, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, stream));
    CS_HIP(ctx, hipMemcpyAsync(nnzm.data(), D.marg_nnz, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, stream));
    CS_HIP(ctx, hipMemcpyAsync(&h_bad, bad, sizeof(int), hipMemcpyDeviceToHost, stream));
    CS_HIP(ctx, hipStreamSynchronize(stream));
    if (h_bad) return fail(ctx, CS_ERR_INVALID, "cs_ice_balance: the table holds pixels below the diagonal (an upper-triangle table is required)");

    // 2. the filters of balance_cooler: min_nnz, min_count, then the MAD of the log marginals, each chromosome scaled by the median
    // of its positive marginals (a chromosome without any: NaN, never filtered)
    std::vector<double> bias((size_t)n, 1.0);
    if (p->min_nnz > 0)
        for (int i = 0; i < n; ++i)
            if (nnzm[(size_t)i] < p->min_nnz) bias[(size_t)i] = 0.0;
    if (p->min_count > 0.0)
        for (int i = 0; i < n; ++i)
            if (marg[(size_t)i] < p->min_count) bias[(size_t)i] = 0.0;
    if (p->mad_max > 0.0) {
        std::vector<double> scaled((size_t)n), logs;
        for (int c = 0; c < n_chrom; ++c) {
            const int lo = (int)chrom_offsets[c], hi = (int)chrom_offsets[c + 1];
            std::vector<double> pos;
            for (int i = lo; i < hi; ++i)
                if (marg[(size_t)i] > 0.0) pos.push_back(marg[(size_t)i]);
            const double med = median_of(std::move(pos));
            for (int i = lo; i < hi; ++i) scaled[(size_t)i] = marg[(size_t)i] / med;
        }
        for (int i = 0; i < n; ++i)
            if (scaled[(size_t)i] > 0.0) logs.push_back(std::log(scaled[(size_t)i]));
        const double med = median_of(logs);
        for (double& x : logs) x = std::fabs(x - med);
        const double dev = median_of(std::move(logs));
        const double cutoff = std::exp(med - p->mad_max * dev);
        for (int i = 0; i < n; ++i)
            if (scaled[(size_t)i] < cutoff) bias[(size_t)i] = 0.0;
    }
    std::vector<cs::IceSpanState> st((size_t)n_spans);
    for (auto& s : st) s = cs::IceSpanState{0, 0, 0, 0, -1, 0, 0.0, 0.0};
    const int ctl[2] = {n_spans, -1};
    CS_HIP(ctx, hipMemcpyAsync(d_bias, bias.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, stream));
    CS_HIP(ctx, hipMemcpyAsync(D.st, st.data(), st.size() * sizeof(cs::IceSpanState), hipMemcpyHostToDevice, stream));
    CS_HIP(ctx, hipMemcpyAsync(D.ctl, ctl, sizeof(ctl), hipMemcpyHostToDevice, stream));

    // 3. the iterations, queued; launches behind the last running span return at once
    rc = cs::ice_iterate(D, g->d_data, g->dtype == CS_F64, csc_val, p->max_iters, stream);
    if (rc) return fail(ctx, CS_ERR_HIP, "cs_ice_balance: iteration launches failed: %s", hipGetErrorString((hipError_t)rc));
    CS_HIP(ctx, hipMemcpyAsync(st.data(), D.st, st.size() * sizeof(cs::IceSpanState), hipMemcpyDeviceToHost, stream));
    CS_HIP(ctx, hipStreamSynchronize(stream));
    for (int s = 0; s < n_spans; ++s) {
        h_stats[s].iterations = st[(size_t)s].iters;
        h_stats[s].converged = st[(size_t)s].converged;
        h_stats[s].var = st[(size_t)s].var;
        h_stats[s].scale = st[(size_t)s].mean;
    }
    return CS_OK;
}

}  // extern "C"
