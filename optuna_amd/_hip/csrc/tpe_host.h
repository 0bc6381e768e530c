// Host side of the TPE hot path: the stateless fit-and-score entry point and
// the device-resident history. Kernels: tpe_kernels.h, tpe_fused_kernels.h.
#pragma once

#include "hip_common.h"
#include "tpe_below_host.h"
#include "tpe_draw_bind.h"
#include "tpe_fused_kernels.h"
#include "tpe_kernels.h"

// d_scratch must hold 2 * mix_n_chunks(K) * S doubles (may alias nothing else).
static void launch_mix_logpdf(hipStream_t st, const double* d_x,
                              const double* d_xedges, const double* d_c1,
                              const double* d_c2, const double* d_c3,
                              const double* d_logw, const double* d_steps,
                              const double* d_nchoices, double cat_base,
                              int64_t K, int64_t D, int64_t S, double* d_out,
                              double* d_scratch) {
    const int block = 256;
    const size_t shmem = (4 * (size_t)D + 2 * block) * sizeof(double);
    const int64_t n_chunks = mix_n_chunks(K);
    if (n_chunks <= 1) {
        hipLaunchKernelGGL(k_mix_logpdf, dim3((unsigned)S), dim3(block), shmem, st,
                           d_x, d_xedges, d_c1, d_c2, d_c3, d_logw, d_steps,
                           d_nchoices, cat_base, K, D, d_out);
        return;
    }
    double* d_part_m = d_scratch;
    double* d_part_s = d_scratch + (size_t)n_chunks * S;
    hipLaunchKernelGGL(k_mix_logpdf_partial, dim3((unsigned)S, (unsigned)n_chunks),
                       dim3(block), shmem, st, d_x, d_xedges, d_c1, d_c2, d_c3,
                       d_logw, d_steps, d_nchoices, cat_base, K, D, MIX_CHUNK,
                       d_part_m, d_part_s);
    hipLaunchKernelGGL(k_mix_logpdf_merge, dim3((unsigned)S), dim3(64), 0, st,
                       d_part_m, d_part_s, n_chunks, S, d_out);
}

// End of a scoring call: copy the result (shape.prod() doubles at d_src) into a
// fresh array, drain the stream and surface any launch error.
static py::array_t<double> download_f64(hipStream_t st, const double* d_src,
                                        std::vector<py::ssize_t> shape) {
    py::array_t<double> out(std::move(shape));
    HIP_CHECK(hipMemcpyAsync(out.mutable_data(), d_src, (size_t)out.size() * 8,
                             hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipGetLastError());
    return out;
}

// Full fused path: fit one KDE on device and evaluate candidates.
//   obs        (N, D)   observations, KDE domain
//   sorted_pos (N, D)   column-wise ranks (row index of r-th smallest per dim)
//   logw       (N+1,)   log mixture weights (prior last)
//   alow/ahigh (D,)     KDE-domain truncation bounds
//   x          (S, D)   candidates, KDE domain
// returns (S,) log mixture pdf.
py::array_t<double> kde_logpdf(const arr_f64& obs, const arr_i64& sorted_pos,
                               const arr_f64& logw, const arr_f64& alow,
                               const arr_f64& ahigh, const arr_f64& steps,
                               const arr_f64& n_choices, double prior_weight,
                               const arr_f64& x, const arr_f64& xedges,
                               bool consider_endpoints, bool magic_clip) {
    if (obs.ndim() != 2 || x.ndim() != 2) throw std::runtime_error("obs/x must be 2-D");
    const int64_t N = obs.shape(0);
    const int64_t D = obs.shape(1);
    const int64_t S = x.shape(0);
    const int64_t K = N + 1;
    if (x.shape(1) != D || (int64_t)logw.size() != K ||
        (int64_t)alow.size() != D || (int64_t)ahigh.size() != D ||
        (int64_t)steps.size() != D || (int64_t)xedges.size() != 2 * S * D ||
        sorted_pos.shape(0) != N || (N > 0 && sorted_pos.shape(1) != D))
        throw std::runtime_error("shape mismatch in kde_logpdf");

    hipStream_t st = g_ws.get_stream();

    const size_t n_obs = (size_t)N * D;
    const size_t n_c = (size_t)K * D;
    WsLayout L;
    const auto s_obs = L.add<double>(n_obs);
    const auto s_c1 = L.add<double>(n_c), s_c2 = L.add<double>(n_c),
               s_c3 = L.add<double>(n_c);
    const auto s_logw = L.add<double>(K);
    const auto s_alow = L.add<double>(D), s_ahigh = L.add<double>(D),
               s_steps = L.add<double>(D), s_nchoices = L.add<double>(D);
    const auto s_x = L.add<double>((size_t)S * D);
    const auto s_xedges = L.add<double>(2 * (size_t)S * D);
    const auto s_out = L.add<double>(S);
    const auto s_scratch = L.add<double>(2 * (size_t)mix_n_chunks(K) * S);
    const auto s_sorted = L.add<int64_t>(n_obs);
    char* base = g_ws.ensure_bytes(L.bytes());
    double *d_obs = s_obs.in(base), *d_c1 = s_c1.in(base), *d_c2 = s_c2.in(base),
           *d_c3 = s_c3.in(base), *d_logw = s_logw.in(base),
           *d_alow = s_alow.in(base), *d_ahigh = s_ahigh.in(base),
           *d_steps = s_steps.in(base), *d_nchoices = s_nchoices.in(base),
           *d_x = s_x.in(base), *d_xedges = s_xedges.in(base),
           *d_out = s_out.in(base), *d_scratch = s_scratch.in(base);
    int64_t* d_sorted = s_sorted.in(base);

    g_ws.begin_uploads();
    if (N > 0) {
        g_ws.h2d(d_obs, obs.data(), n_obs * 8, st);
        g_ws.h2d(d_sorted, sorted_pos.data(), n_obs * 8, st);
    }
    g_ws.h2d(d_logw, logw.data(), K * 8, st);
    g_ws.h2d(d_alow, alow.data(), D * 8, st);
    g_ws.h2d(d_ahigh, ahigh.data(), D * 8, st);
    g_ws.h2d(d_steps, steps.data(), D * 8, st);
    g_ws.h2d(d_nchoices, n_choices.data(), D * 8, st);
    g_ws.h2d(d_x, x.data(), (size_t)S * D * 8, st);
    g_ws.h2d(d_xedges, xedges.data(), 2 * (size_t)S * D * 8, st);

    const double cat_base = prior_weight / (double)K;
    {
        const int block = 256;
        const int gx = (int)((K + block - 1) / block);
        hipLaunchKernelGGL(k_parzen_fit, dim3(gx, (unsigned)D), dim3(block), 0, st,
                           d_obs, d_sorted, d_alow, d_ahigh, d_steps, d_nchoices,
                           N, D, consider_endpoints ? 1 : 0, magic_clip ? 1 : 0,
                           d_c1, d_c2, d_c3);
    }
    launch_mix_logpdf(st, d_x, d_xedges, d_c1, d_c2, d_c3, d_logw, d_steps,
                      d_nchoices, cat_base, K, D, S, d_out, d_scratch);
    return download_f64(st, d_out, {S});
}

// Below estimator of a fused suggest, fitted on the host in one call (see
// tpe_below_host.h): no device work. The arrays are taken as they are, so a
// wrong dtype or a non-contiguous view is an error, not a silent copy.
//   obs (n, D) f64, alow/ahigh (D,) f64, active (S,) i64 in [0, n]
// returns (mus, sigmas (n + 1, D); a, b, loc, scale (S, D)).
static const double* below_f64(const py::array& arr, const char* name) {
    if (!py::isinstance<py::array_t<double>>(arr) ||
        !(arr.flags() & py::array::c_style))
        throw std::runtime_error(std::string("tpe_below_kernels: ") + name +
                                 " must be a C-contiguous float64 array");
    return static_cast<const double*>(arr.data());
}

py::tuple tpe_below_kernels(const py::array& obs, const py::array& alow,
                            const py::array& ahigh, bool consider_endpoints,
                            bool consider_magic_clip, const py::array& active) {
    const double* p_obs = below_f64(obs, "obs");
    const double* p_alow = below_f64(alow, "alow");
    const double* p_ahigh = below_f64(ahigh, "ahigh");
    if (!py::isinstance<py::array_t<int64_t>>(active) ||
        !(active.flags() & py::array::c_style))
        throw std::runtime_error(
            "tpe_below_kernels: active must be a C-contiguous int64 array");
    if (obs.ndim() != 2 || alow.ndim() != 1 || ahigh.ndim() != 1 ||
        active.ndim() != 1 || obs.shape(1) < 1 || alow.shape(0) != obs.shape(1) ||
        ahigh.shape(0) != obs.shape(1))
        throw std::runtime_error("tpe_below_kernels: shape mismatch");
    const int64_t n = obs.shape(0), D = obs.shape(1), S = active.shape(0);
    if (n + 1 > FUSED_MAX_BELOW)
        throw std::runtime_error("tpe_below_kernels: too many below kernels");
    const int64_t* p_active = static_cast<const int64_t*>(active.data());
    for (int64_t s = 0; s < S; ++s)
        if (p_active[s] < 0 || p_active[s] > n)
            throw std::runtime_error("tpe_below_kernels: active out of range");

    py::array_t<double> mus({n + 1, D}), sigmas({n + 1, D});
    py::array_t<double> a({S, D}), b({S, D}), loc({S, D}), scale({S, D});
    tpe_below::fit_and_gather(p_obs, (size_t)n, (size_t)D, p_alow, p_ahigh,
                              consider_endpoints, consider_magic_clip, p_active,
                              (size_t)S, mus.mutable_data(), sigmas.mutable_data(),
                              a.mutable_data(), b.mutable_data(),
                              loc.mutable_data(), scale.mutable_data());
    return py::make_tuple(mus, sigmas, a, b, loc, scale);
}

// ---------------------------------------------------------------------------
// Device-resident TPE history (one per (study, search-space) on the Python side).
//
// The parameter table lives in HBM and grows append-only, mirroring the host
// history (_history.py). The per-dim global sorted order (i32) is resident too:
// upload_sorted seeds it and insert_sorted_by_value grows it on the device
// (score also accepts explicit columns, uploaded for that call only). A suggest
// uploads only the subset position map, the domain, mixture weights and
// candidates — the big fp64 observation matrix never crosses PCIe again after
// its append.
//
// score() pipeline (all on one stream):
//   1. k_compact_{count,scan,write}: per dim, order-preserving compaction of
//      the global sorted order down to the "above" subset (tiled 3-phase scan).
//   2. k_parzen_fit_table: K1 fit reading mus from the resident table.
//   3. k_mix_logpdf: K2 scoring.
// ---------------------------------------------------------------------------

class TpeDeviceHistory {
  public:
    explicit TpeDeviceHistory(int64_t D) : D_(D) {}

    int64_t n_rows() const { return n_; }

    void append(const arr_f64& block) {
        if (block.ndim() != 2 || block.shape(1) != D_)
            throw std::runtime_error("append: block must be (n_new, D)");
        const int64_t n_new = block.shape(0);
        if (n_new == 0) return;
        prep_.valid = false;
        hipStream_t st = g_ws.get_stream();
        if (n_ + n_new > capacity_) {
            const int64_t new_cap = std::max<int64_t>(1024, (n_ + n_new) * 2);
            params_.grow_preserving((size_t)new_cap * D_, 1, (size_t)n_ * D_, st);
            capacity_ = new_cap;
        }
        g_ws.begin_uploads();
        g_ws.h2d(params_.ptr + (size_t)n_ * D_, block.data(),
                 (size_t)n_new * D_ * sizeof(double), st);
        // No stream sync: the table write is stream-ordered before any later
        // kernel on this stream; staging reuse is guarded by the upload event.
        g_ws.end_uploads_async(st);
        n_ += n_new;
    }

    py::array_t<double> score(const std::vector<arr_i32>& sorted_cols,  // D × (Nv,)
                              const arr_i32& pos,  // (n_rows,)
                              int64_t n_above,
                              const arr_f64& logw,  // (n_above + L + 1,)
                              const arr_f64& alow, const arr_f64& ahigh,
                              const arr_f64& steps,   // (D,) 0 = continuous
                              const arr_f64& n_choices,  // (D,) 0 = numerical
                              double prior_weight,
                              const arr_f64& x,       // (S, D) KDE domain
                              const arr_f64& xedges,  // (S, 2D) cell lo|hi
                              bool consider_endpoints, bool magic_clip,
                              const arr_f64& extras_raw,         // (L, D) or empty
                              const arr_f64& extras_sorted,      // (D, L)
                              const arr_i32& extras_sorted_idx,  // (D, L)
                              bool per_dim)
    {
        const bool resident_sorted = sorted_cols.empty() && sorted_valid_;
        const int64_t Nv =
            resident_sorted ? n_sorted_
                            : (sorted_cols.empty() ? 0
                                                   : (int64_t)sorted_cols[0].size());
        const int64_t S = x.shape(0);
        const int64_t Na = n_above;
        const int64_t L = extras_raw.ndim() == 2 ? extras_raw.shape(0) : 0;
        const int64_t Nk = Na + L;  // mixture kernels excluding the prior
        const int64_t K = Nk + 1;
        if ((int64_t)pos.size() != n_ || x.shape(1) != D_ ||
            (!resident_sorted && Nv > 0 && (int64_t)sorted_cols.size() != D_) ||
            (int64_t)logw.size() != K)
            throw std::runtime_error("score: shape mismatch");
        if (Na < 0 || Na > Nv)
            throw std::runtime_error("score: n_above exceeds the sorted index");
        if (L > 0 && ((int64_t)extras_sorted.size() != L * D_ ||
                      (int64_t)extras_sorted_idx.size() != L * D_ ||
                      extras_raw.shape(1) != D_))
            throw std::runtime_error("score: extras shape mismatch");
        for (const auto& col : sorted_cols)
            if ((int64_t)col.size() != Nv)
                throw std::runtime_error("score: ragged sorted columns");

        hipStream_t st = g_ws.get_stream();
        const size_t n_c = (size_t)K * D_;
        const int64_t n_tiles = (Nv + 255) / 256;
        const int64_t mstride = Nv + L;  // merged subset stride
        const size_t n_sd = (size_t)S * D_, n_ld = (size_t)L * D_;
        const size_t n_vd = (size_t)Nv * D_, n_md = (size_t)mstride * D_;
        WsLayout W;
        const auto s_c1 = W.add<double>(n_c), s_c2 = W.add<double>(n_c),
                   s_c3 = W.add<double>(n_c);
        const auto s_logw = W.add<double>(K);
        const auto s_alow = W.add<double>(D_), s_ahigh = W.add<double>(D_),
                   s_steps = W.add<double>(D_), s_nchoices = W.add<double>(D_);
        const auto s_x = W.add<double>(n_sd), s_xedges = W.add<double>(2 * n_sd);
        const auto s_out = W.add<double>(per_dim ? n_sd : (size_t)S);
        const auto s_scratch = W.add<double>(2 * (size_t)mix_n_chunks(K) * S);
        const auto s_extras_raw = W.add<double>(n_ld),
                   s_extras_sorted = W.add<double>(n_ld);
        const auto s_sorted = W.add<int32_t>(n_vd);
        const auto s_pos = W.add<int32_t>(n_);
        const auto s_sub_rows = W.add<int32_t>(n_vd), s_sub_k = W.add<int32_t>(n_vd);
        const auto s_merged_rows = W.add<int32_t>(n_md),
                   s_merged_k = W.add<int32_t>(n_md);
        const auto s_extra_idx = W.add<int32_t>(n_ld);
        const auto s_counts = W.add<int32_t>((size_t)n_tiles * D_);
        char* base = g_ws.ensure_bytes(W.bytes());
        double *d_c1 = s_c1.in(base), *d_c2 = s_c2.in(base), *d_c3 = s_c3.in(base),
               *d_logw = s_logw.in(base), *d_alow = s_alow.in(base),
               *d_ahigh = s_ahigh.in(base), *d_steps = s_steps.in(base),
               *d_nchoices = s_nchoices.in(base), *d_x = s_x.in(base),
               *d_xedges = s_xedges.in(base), *d_out = s_out.in(base),
               *d_scratch = s_scratch.in(base),
               *d_extras_raw = s_extras_raw.in(base),
               *d_extras_sorted = s_extras_sorted.in(base);
        int32_t *d_sorted = s_sorted.in(base), *d_pos = s_pos.in(base),
                *d_sub_rows = s_sub_rows.in(base), *d_sub_k = s_sub_k.in(base),
                *d_merged_rows = s_merged_rows.in(base),
                *d_merged_k = s_merged_k.in(base),
                *d_extra_idx = s_extra_idx.in(base), *d_counts = s_counts.in(base);

        g_ws.begin_uploads();
        if (!resident_sorted)
            for (int64_t d = 0; d < (int64_t)sorted_cols.size() && Nv > 0; ++d)
                g_ws.h2d(d_sorted + d * Nv, sorted_cols[d].data(), (size_t)Nv * 4,
                         st);
        if (n_ > 0) g_ws.h2d(d_pos, pos.data(), (size_t)n_ * 4, st);
        g_ws.h2d(d_logw, logw.data(), K * 8, st);
        g_ws.h2d(d_alow, alow.data(), D_ * 8, st);
        g_ws.h2d(d_ahigh, ahigh.data(), D_ * 8, st);
        g_ws.h2d(d_steps, steps.data(), D_ * 8, st);
        g_ws.h2d(d_nchoices, n_choices.data(), D_ * 8, st);
        g_ws.h2d(d_x, x.data(), (size_t)S * D_ * 8, st);
        g_ws.h2d(d_xedges, xedges.data(), 2 * (size_t)S * D_ * 8, st);
        if (L > 0) {
            g_ws.h2d(d_extras_raw, extras_raw.data(), (size_t)L * D_ * 8, st);
            g_ws.h2d(d_extras_sorted, extras_sorted.data(), (size_t)L * D_ * 8, st);
            g_ws.h2d(d_extra_idx, extras_sorted_idx.data(), (size_t)L * D_ * 4, st);
        }

        if (Na > 0 && Nv > 0) {
            const int32_t* s_src = resident_sorted ? sorted_.ptr : d_sorted;
            const int64_t s_stride = resident_sorted ? sorted_cap_ : Nv;
            const dim3 grid((unsigned)n_tiles, (unsigned)D_);
            hipLaunchKernelGGL(k_compact_count, grid, dim3(256), 0, st, s_src,
                               d_pos, Nv, s_stride, D_, d_counts);
            hipLaunchKernelGGL(k_compact_scan, dim3((unsigned)D_), dim3(64), 0, st,
                               d_counts, n_tiles);
            hipLaunchKernelGGL(k_compact_write, grid, dim3(256), 0, st, s_src,
                               d_pos, Nv, s_stride, D_, d_counts, d_sub_rows,
                               d_sub_k);
        }
        const int32_t* fit_rows = d_sub_rows;
        const int32_t* fit_k = d_sub_k;
        int64_t fit_stride = Nv;
        if (L > 0) {
            const int block = 256;
            const int gx = (int)((Na + L + block - 1) / block);
            hipLaunchKernelGGL(k_merge_extras, dim3(gx, (unsigned)D_), dim3(block),
                               0, st, d_sub_rows, d_sub_k, Nv, Na, params_.ptr, n_,
                               D_, d_extras_sorted, d_extra_idx, L,
                               d_merged_rows, d_merged_k, mstride);
            fit_rows = d_merged_rows;
            fit_k = d_merged_k;
            fit_stride = mstride;
        }
        {
            const int block = 256;
            const int gx = (int)((K + block - 1) / block);
            hipLaunchKernelGGL(k_parzen_fit_table, dim3(gx, (unsigned)D_),
                               dim3(block), 0, st, params_.ptr,
                               L > 0 ? d_extras_raw : nullptr, n_, fit_rows,
                               fit_k, fit_stride, d_alow, d_ahigh, d_steps,
                               d_nchoices, Nk, D_, consider_endpoints ? 1 : 0,
                               magic_clip ? 1 : 0, d_c1, d_c2, d_c3);
        }
        const double cat_base = prior_weight / (double)K;
        if (per_dim) {
            hipLaunchKernelGGL(k_mix_logpdf_perdim,
                               dim3((unsigned)S, (unsigned)D_), dim3(256), 0, st,
                               d_x, d_xedges, d_c1, d_c2, d_c3, d_logw, d_steps,
                               d_nchoices, cat_base, K, D_, d_out);
            return download_f64(st, d_out, {S, D_});
        }
        launch_mix_logpdf(st, d_x, d_xedges, d_c1, d_c2, d_c3, d_logw, d_steps,
                          d_nchoices, cat_base, K, D_, S, d_out, d_scratch);
        return download_f64(st, d_out, {S});
    }

    // ---- device-resident per-dim sorted index ------------------------------

    void upload_sorted(const std::vector<arr_i32>& cols) {
        const int64_t Nv = cols.empty() ? 0 : (int64_t)cols[0].size();
        if ((int64_t)cols.size() != D_ && Nv > 0)
            throw std::runtime_error("upload_sorted: wrong number of columns");
        prep_.valid = false;
        hipStream_t st = g_ws.get_stream();
        ensure_sorted_capacity(Nv, st);
        g_ws.begin_uploads();
        for (int64_t d = 0; d < (int64_t)cols.size() && Nv > 0; ++d)
            g_ws.h2d(sorted_.ptr + d * sorted_cap_, cols[d].data(), (size_t)Nv * 4, st);
        g_ws.end_uploads_async(st);
        n_sorted_ = Nv;
        sorted_valid_ = true;
    }

    int64_t n_sorted() const { return sorted_valid_ ? n_sorted_ : -1; }

    // Insert table rows [first_row, first_row + n_new) into the resident index
    // by value (see k_sorted_insert_by_value). No upload, no sync.
    void insert_sorted_by_value(int64_t first_row, int64_t n_new) {
        if (!sorted_valid_)
            throw std::runtime_error("insert_sorted_by_value before upload");
        if (n_new <= 0) return;
        prep_.valid = false;
        if (first_row < 0 || first_row + n_new > n_)
            throw std::runtime_error("insert_sorted_by_value: rows not in table");
        hipStream_t st = g_ws.get_stream();
        ensure_sorted_capacity(n_sorted_ + n_new, st);
        hipLaunchKernelGGL(k_sorted_insert_by_value, dim3((unsigned)D_),
                           dim3(256), 0, st, sorted_.ptr, sorted_cap_, n_sorted_,
                           params_.ptr, D_, first_row, n_new);
        HIP_CHECK(hipGetLastError());
        n_sorted_ += n_new;
    }

    // Debug/test accessor: the resident sorted index as a (D, n_sorted) array.
    py::array_t<int32_t> sorted_index() {
        if (!sorted_valid_) throw std::runtime_error("sorted_index before upload");
        py::array_t<int32_t> out({D_, n_sorted_});
        hipStream_t st = g_ws.get_stream();
        if (n_sorted_ > 0)
            HIP_CHECK(hipMemcpy2DAsync(out.mutable_data(), (size_t)n_sorted_ * 4,
                                       sorted_.ptr, (size_t)sorted_cap_ * 4,
                                       (size_t)n_sorted_ * 4, (size_t)D_,
                                       hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        return out;
    }

    // Per-space constants (KDE-domain bounds, steps, category counts): they
    // never change for a (study, search-space), so they are uploaded once.
    void set_domain(const arr_f64& alow, const arr_f64& ahigh,
                    const arr_f64& steps, const arr_f64& n_choices) {
        if ((int64_t)alow.size() != D_ || (int64_t)ahigh.size() != D_ ||
            (int64_t)steps.size() != D_ || (int64_t)n_choices.size() != D_)
            throw std::runtime_error("set_domain: shape mismatch");
        prep_.valid = false;
        std::vector<double> host(4 * (size_t)D_);
        std::copy(alow.data(), alow.data() + D_, host.begin());
        std::copy(ahigh.data(), ahigh.data() + D_, host.begin() + D_);
        std::copy(steps.data(), steps.data() + D_, host.begin() + 2 * D_);
        std::copy(n_choices.data(), n_choices.data() + D_, host.begin() + 3 * D_);
        hipStream_t st = g_ws.get_stream();
        domain_.reserve(host.size());
        // Earlier launches may still read the old values.
        HIP_CHECK(hipStreamSynchronize(st));
        HIP_CHECK(hipMemcpy(domain_.ptr, host.data(), host.size() * sizeof(double),
                            hipMemcpyHostToDevice));
        has_steps_ = false;
        has_categorical_ = false;
        for (int64_t d = 0; d < D_; ++d) {
            has_steps_ |= steps.data()[d] > 0.0;
            has_categorical_ |= n_choices.data()[d] > 0.0;
        }
    }

    // Fused suggest, in two native calls that share one stream:
    //   fused_prepare  uploads the exclusion list (and custom log-weights) and
    //                  launches the above-set fit into this history's own
    //                  coefficient buffer; returns without synchronising.
    //   fused_score    one packed upload (candidates + below estimator),
    //                  k_fused_score, k_fused_merge (which writes the result
    //                  into pinned host memory: no download). It reuses
    //                  the prepared fit when that is still valid for its
    //                  arguments and otherwise runs the fit itself first.
    //   fused_draw_score  the same device half behind the host draw of the
    //                  candidates, with the arg-max behind it: the one call
    //                  of the sampler's native draw route.
    //   excl     sorted table rows NOT in the above set (below + invalid rows)
    //   n_above  size of the above set (= resident index rows not in excl)
    //   x/xedges candidates (KDE domain); xedges only read for stepped dims
    //   bmu/bsig/bw  below estimator kernels (Kb, D) and mixture weights (Kb,)
    //   logw     custom above log-weights (n_above + 1,), or empty for the
    //            default ramp, which the device writes itself from
    //            (w_num, w_start, w_step, log_total)
    void fused_prepare(const arr_i32& excl, int64_t n_above, const arr_f64& logw,
                       int64_t w_num, double w_start, double w_step,
                       double log_total, double prior_weight,
                       bool consider_endpoints, bool magic_clip) {
        check_fit_args("fused_prepare", excl, n_above, logw);
        g_ws.begin_uploads();
        launch_fit(excl, n_above, logw, w_num, w_start, w_step, log_total,
                   prior_weight, consider_endpoints, magic_clip,
                   /*guard_staging=*/true);
    }

    // Returns (S,) log l - log g, or with return_parts the test/debug form
    // ((3, S) [ei | log g | log l], (K,) above logw).
    py::object fused_score(const arr_i32& excl, int64_t n_above,
                                    const arr_f64& x, const arr_f64& xedges,
                                    const arr_f64& bmu, const arr_f64& bsig,
                                    const arr_f64& bw, const arr_f64& logw,
                                    int64_t w_num, double w_start,
                                    double w_step, double log_total,
                                    double prior_weight,
                                    bool consider_endpoints, bool magic_clip,
                                    bool return_parts) {
        check_fit_args("fused_score", excl, n_above, logw);
        if (x.ndim() != 2 || x.shape(1) != D_ || bmu.ndim() != 2 ||
            bmu.shape(1) != D_ || bsig.ndim() != 2 || bsig.shape(1) != D_)
            throw std::runtime_error("fused_score: shape mismatch");
        const int64_t S = x.shape(0);
        const int64_t Kb = bmu.shape(0);
        const int64_t K = n_above + 1;
        if (S < 1 || Kb < 1 || Kb > FUSED_MAX_BELOW || bsig.shape(0) != Kb ||
            (int64_t)bw.size() != Kb ||
            (has_steps_ && (int64_t)xedges.size() != 2 * S * D_))
            throw std::runtime_error("fused_score: shape mismatch");

        // The results are allocated ahead of the call, under the device work.
        py::array_t<double> lw(return_parts ? K : 0);
        py::array_t<double> out(return_parts ? 0 : S);
        const double* h_out = score_candidates(
            excl, n_above, x.data(), xedges.data(), bmu.data(), bsig.data(),
            bw.data(), S, Kb, logw, w_num, w_start, w_step, log_total,
            prior_weight, consider_endpoints, magic_clip,
            return_parts ? lw.mutable_data() : nullptr);
        if (return_parts) {
            py::array_t<double> parts({(int64_t)3, S});
            memcpy(parts.mutable_data(), h_out, 3 * (size_t)S * 8);
            return py::make_tuple(parts, lw);
        }
        memcpy(out.mutable_data(), h_out, (size_t)S * 8);
        return out;
    }

    // Second half of a fused suggest in one call: the host draw of
    // tpe_draw_bind.h (below fit, kernel choice, quantile, candidates and
    // their scoring inputs), then the device half of fused_score, then the
    // arg-max. Fit arguments as for fused_score; the estimator flags serve
    // the below fit too. Returns (best index, x_raw (S, D), (S,) log l - log g).
    py::tuple fused_draw_score(const arr_i32& excl, int64_t n_above,
                               const py::array& table, const py::array& valid,
                               const py::array& below_rows, const py::array& bw,
                               const py::array& u, const py::array& q,
                               const py::array& alow, const py::array& ahigh,
                               const py::array& kinds, const py::array& lows,
                               const py::array& highs, const py::array& steps,
                               const arr_f64& logw, int64_t w_num,
                               double w_start, double w_step, double log_total,
                               double prior_weight, bool consider_endpoints,
                               bool magic_clip) {
        check_fit_args("fused_draw_score", excl, n_above, logw);
        if (table.ndim() != 2 || table.shape(1) != D_)
            throw std::runtime_error("fused_draw_score: shape mismatch");
        tpe_draw_py::HostDraw& H = draw_;
        tpe_draw_py::draw(H, table, valid, below_rows, bw, u, q, alow, ahigh,
                          kinds, lows, highs, steps, consider_endpoints,
                          magic_clip, has_steps_, (size_t)FUSED_MAX_BELOW);
        const int64_t S = (int64_t)H.S;
        py::array_t<double> out(S);
        py::array_t<double> x_raw = tpe_draw_py::copy_out(H.x_raw, H.S, H.D);
        const double* h_out = score_candidates(
            excl, n_above, H.x_kde.data(), H.xedges.data(), H.mus.data(),
            H.sigmas.data(), static_cast<const double*>(bw.data()), S,
            (int64_t)H.Kb(), logw, w_num, w_start, w_step, log_total,
            prior_weight, consider_endpoints, magic_clip, nullptr);
        memcpy(out.mutable_data(), h_out, (size_t)S * 8);
        const size_t best = tpe_draw::argmax(h_out, (size_t)S);
        return py::make_tuple(best, x_raw, out);
    }

  private:
    // What the coefficients in coef_ were fitted from. They stay usable only
    // while the table, the index, the domain and every fit argument are the
    // same; every mutator of those clears `valid`.
    struct PreparedFit {
        bool valid = false;
        int64_t n = 0, n_sorted = 0, Na = 0, w_num = 0;
        double w_start = 0.0, w_step = 0.0, log_total = 0.0, prior_weight = 0.0;
        bool consider_endpoints = false, magic_clip = false;
        std::vector<int32_t> excl;
        std::vector<double> logw;  // custom log-weights, empty for the ramp
    };

    void check_fit_args(const char* who, const arr_i32& excl, int64_t Na,
                        const arr_f64& logw) const {
        const std::string w(who);
        if (!sorted_valid_) throw std::runtime_error(w + " before upload_sorted");
        if (!domain_.ptr) throw std::runtime_error(w + " before set_domain");
        if (has_categorical_)
            throw std::runtime_error(w + ": categorical dims unsupported");
        const int64_t E = excl.size();
        const int64_t Nv = n_sorted_;
        if (E > FUSED_MAX_EXCL || Na < 0 || Na > Nv || Na + E < Nv ||
            (logw.size() > 0 && (int64_t)logw.size() != Na + 1))
            throw std::runtime_error(w + ": shape mismatch");
        // Strictly ascending in-table rows: keeps row - lower_bound(excl, row)
        // inside [0, n_above) for every member row.
        const int32_t* ex = excl.data();
        for (int64_t e = 0; e < E; ++e)
            if (ex[e] < 0 || ex[e] >= n_ || (e > 0 && ex[e] <= ex[e - 1]))
                throw std::runtime_error(w + ": excl must be sorted table rows");
    }

    // Device half of a fused suggest on checked arguments: the fall-back fit,
    // the packed upload, k_fused_score, k_fused_merge and the stream
    // synchronise. Returns the merge's (3, S) result [ei | log g | log l] in
    // pinned host memory, good until the next upload batch; lw_out, if given,
    // receives the (K,) above log-weights.
    const double* score_candidates(const arr_i32& excl, int64_t n_above,
                                   const double* x, const double* xedges,
                                   const double* bmu, const double* bsig,
                                   const double* bw, int64_t S, int64_t Kb,
                                   const arr_f64& logw, int64_t w_num,
                                   double w_start, double w_step,
                                   double log_total, double prior_weight,
                                   bool consider_endpoints, bool magic_clip,
                                   double* lw_out) {
        const int64_t K = n_above + 1;
        hipStream_t st = g_ws.get_stream();
        g_ws.begin_uploads();
        if (!prepared_matches(excl, n_above, logw, w_num, w_start, w_step,
                              log_total, prior_weight, consider_endpoints,
                              magic_clip))
            launch_fit(excl, n_above, logw, w_num, w_start, w_step, log_total,
                       prior_weight, consider_endpoints, magic_clip,
                       /*guard_staging=*/false);

        // Packed region (one pinned slice, one DMA, same layout on device):
        //   x | bmu | bsig | bw | [xedges]
        const size_t n_x = (size_t)S * D_;
        const size_t n_b = (size_t)Kb * D_;
        const int64_t n_as = (K + SCORE_SLICE - 1) / SCORE_SLICE;
        // Below slices: as many kernels as give each of the block's threads
        // at most one (kernel, dim) coefficient to build per pass over dims.
        const int64_t pass_dims = std::min<int64_t>(D_, SCORE_DC);
        const int below_slice = (int)std::max<int64_t>(
            1, std::min<int64_t>(SCORE_SLICE, SCORE_SLICE * SCORE_WAVES / pass_dims));
        const int64_t n_bs = (Kb + below_slice - 1) / below_slice;
        const size_t n_part = (size_t)(n_as + n_bs) * S;
        WsLayout L;
        const auto s_x = L.add<double>(n_x);
        const auto s_bmu = L.add<double>(n_b), s_bsig = L.add<double>(n_b);
        const auto s_bw = L.add<double>(Kb);
        const auto s_xedges = L.add<double>(has_steps_ ? 2 * n_x : 0);
        const size_t up_bytes = L.bytes();  // the packed region ends here
        const auto s_part_m = L.add<double>(n_part), s_part_s = L.add<double>(n_part);
        char* base = g_ws.ensure_bytes(L.bytes());
        double *d_x = s_x.in(base), *d_bmu = s_bmu.in(base),
               *d_bsig = s_bsig.in(base), *d_bw = s_bw.in(base),
               *d_xedges = s_xedges.in(base), *d_part_m = s_part_m.in(base),
               *d_part_s = s_part_s.in(base);
        {
            char* h = g_ws.stage(up_bytes, st);
            memcpy(s_x.in(h), x, n_x * 8);
            memcpy(s_bmu.in(h), bmu, n_b * 8);
            memcpy(s_bsig.in(h), bsig, n_b * 8);
            memcpy(s_bw.in(h), bw, (size_t)Kb * 8);
            if (has_steps_) memcpy(s_xedges.in(h), xedges, 2 * n_x * 8);
            HIP_CHECK(hipMemcpyAsync(base, h, up_bytes, hipMemcpyHostToDevice, st));
        }

        const CoefLayout C(K, D_, excl.size());
        const double* d_logw = C.logw.in(coef_.ptr);
        const int64_t n_groups = (S + SCORE_CAND - 1) / SCORE_CAND;
        hipLaunchKernelGGL(k_fused_score,
                           dim3((unsigned)(n_as + n_bs), (unsigned)n_groups),
                           dim3(SCORE_SLICE * SCORE_WAVES), 0, st, d_x, d_xedges,
                           C.c1.in(coef_.ptr), C.c2.in(coef_.ptr),
                           C.c3.in(coef_.ptr), d_logw, K, n_as,
                           d_bmu, d_bsig, d_bw, Kb, below_slice, domain_.ptr,
                           has_steps_ ? 1 : 0,
                           D_, S, d_part_m, d_part_s);
        // The merge writes its (3, S) result straight into a pinned host slot
        // (kernels can address hipHostMalloc memory), which saves the
        // download's own dispatch on the serial chain. The slot belongs to
        // this upload batch and is read after the stream sync below, so it is
        // not reused before the kernel has finished.
        const double* h_out =
            reinterpret_cast<const double*>(g_ws.stage(3 * (size_t)S * 8, st));
        hipLaunchKernelGGL(k_fused_merge, dim3((unsigned)S), dim3(64), 0, st,
                           d_part_m, d_part_s, n_as, n_bs, S,
                           const_cast<double*>(h_out));
        if (lw_out != nullptr)
            HIP_CHECK(hipMemcpyAsync(lw_out, d_logw, (size_t)K * 8,
                                     hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        HIP_CHECK(hipGetLastError());
        return h_out;
    }

    // Bit-wise comparisons throughout: equal arguments give the same fit.
    bool prepared_matches(const arr_i32& excl, int64_t Na, const arr_f64& logw,
                          int64_t w_num, double w_start, double w_step,
                          double log_total, double prior_weight,
                          bool consider_endpoints, bool magic_clip) const {
        const PreparedFit& p = prep_;
        const double a[4] = {w_start, w_step, log_total, prior_weight};
        const double b[4] = {p.w_start, p.w_step, p.log_total, p.prior_weight};
        return p.valid && p.n == n_ && p.n_sorted == n_sorted_ && p.Na == Na &&
               p.w_num == w_num && memcmp(a, b, sizeof(a)) == 0 &&
               p.consider_endpoints == consider_endpoints &&
               p.magic_clip == magic_clip &&
               p.excl.size() == (size_t)excl.size() &&
               (p.excl.empty() ||
                memcmp(p.excl.data(), excl.data(), p.excl.size() * 4) == 0) &&
               p.logw.size() == (size_t)logw.size() &&
               (p.logw.empty() ||
                memcmp(p.logw.data(), logw.data(), p.logw.size() * 8) == 0);
    }

    // coef_ = c1 | c2 | c3 (D, K each, k-major) | logw (K) | excl (E, i32).
    // logw and excl are adjacent, so one DMA uploads both.
    struct CoefLayout {
        WsLayout L;
        WsSlot<double> c1, c2, c3, logw;
        WsSlot<int32_t> excl;
        CoefLayout(int64_t K, int64_t D, int64_t E)
            : c1(L.add<double>((size_t)K * D)), c2(L.add<double>((size_t)K * D)),
              c3(L.add<double>((size_t)K * D)), logw(L.add<double>(K)),
              excl(L.add<int32_t>(E)) {}
    };

    // Upload [logw] | excl into coef_ and launch the fit behind it. The caller
    // has opened the upload batch; with guard_staging the batch is closed with
    // the event guard right behind the DMA (the caller does not synchronise).
    void launch_fit(const arr_i32& excl, int64_t Na, const arr_f64& logw,
                    int64_t w_num, double w_start, double w_step,
                    double log_total, double prior_weight,
                    bool consider_endpoints, bool magic_clip, bool guard_staging) {
        prep_.valid = false;
        hipStream_t st = g_ws.get_stream();
        const int64_t E = excl.size();
        const int64_t K = Na + 1;
        const int64_t Nv = n_sorted_;
        const bool custom_w = logw.size() > 0;
        const CoefLayout C(K, D_, E);
        // Geometric growth, at least 4096 doubles.
        if (C.L.bytes() > coef_.capacity)
            coef_.reserve(std::max(4096 * sizeof(double), 2 * C.L.bytes()));
        double* d_logw = C.logw.in(coef_.ptr);
        int32_t* d_excl = C.excl.in(coef_.ptr);
        // The upload is the tail of the coefficient layout, from logw (custom
        // weights) or from excl on; U names the same regions in the staging
        // slice.
        WsLayout U;
        const auto u_logw = U.add<double>(custom_w ? K : 0);
        const auto u_excl = U.add<int32_t>(E);
        if (U.bytes()) {
            char* h = g_ws.stage(U.bytes(), st);
            if (custom_w) memcpy(u_logw.in(h), logw.data(), (size_t)K * 8);
            // For odd E the slot's padding word is uploaded too: define it.
            if (E & 1) u_excl.in(h)[E] = 0;
            memcpy(u_excl.in(h), excl.data(), (size_t)E * 4);
            HIP_CHECK(hipMemcpyAsync(custom_w ? (void*)d_logw : (void*)d_excl, h,
                                     U.bytes(), hipMemcpyHostToDevice, st));
            if (guard_staging) g_ws.end_uploads_async(st);
        }
        const int64_t n_tiles = std::max<int64_t>(1, (Nv + FUSED_TILE - 1) / FUSED_TILE);
        hipLaunchKernelGGL(k_fused_fit, dim3((unsigned)n_tiles, (unsigned)D_),
                           dim3(FUSED_TILE), 0, st, params_.ptr, sorted_.ptr,
                           sorted_cap_, Nv, d_excl, (int)E, domain_.ptr, Na, D_,
                           consider_endpoints ? 1 : 0, magic_clip ? 1 : 0,
                           C.c1.in(coef_.ptr), C.c2.in(coef_.ptr),
                           C.c3.in(coef_.ptr),
                           custom_w ? nullptr : d_logw, w_num, w_start, w_step,
                           log_total, prior_weight);
        HIP_CHECK(hipGetLastError());
        prep_.n = n_;
        prep_.n_sorted = n_sorted_;
        prep_.Na = Na;
        prep_.w_num = w_num;
        prep_.w_start = w_start;
        prep_.w_step = w_step;
        prep_.log_total = log_total;
        prep_.prior_weight = prior_weight;
        prep_.consider_endpoints = consider_endpoints;
        prep_.magic_clip = magic_clip;
        prep_.excl.assign(excl.data(), excl.data() + E);
        prep_.logw.assign(logw.data(), logw.data() + logw.size());
        prep_.valid = true;
    }

    void ensure_sorted_capacity(int64_t need, hipStream_t st) {
        if (need <= sorted_cap_) return;
        const int64_t new_cap = std::max<int64_t>(1024, need * 2);
        // D_ columns, each new_cap wide.
        sorted_.grow_preserving((size_t)new_cap * D_, D_, n_sorted_, st);
        sorted_cap_ = new_cap;
    }

    int64_t D_;
    int64_t n_ = 0;
    int64_t capacity_ = 0;          // rows params_ can hold
    DeviceBuffer<double> params_;   // (capacity_, D)
    DeviceBuffer<int32_t> sorted_;  // (D, sorted_cap_)
    int64_t n_sorted_ = 0;
    int64_t sorted_cap_ = 0;
    bool sorted_valid_ = false;
    DeviceBuffer<double> domain_;  // alow | ahigh | steps | n_choices
    bool has_steps_ = false;
    bool has_categorical_ = false;
    // Above-set coefficients of the fused suggest (see CoefLayout): owned by
    // the history (the shared workspace is laid over by every other entry
    // point), grown geometrically.
    DeviceBuffer<char> coef_;
    PreparedFit prep_;
    tpe_draw_py::HostDraw draw_;  // host half of fused_draw_score
};
