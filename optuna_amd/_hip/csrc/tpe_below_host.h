// Host fit of the TPE "below" estimator and the gather for its candidate
// draw: what parzen.py's _numerical_kernels_batched and the head of
// _sample_array compute through some 25 numpy calls, in one pass. Every
// operation is the IEEE add, subtract, divide, max or min that numpy performs,
// in the same order, so the outputs equal numpy's bit for bit.
//
// Plain C++17 on pointers and sizes: no HIP, no pybind (see
// tests/cpp/tpe_below_check.cpp for the stand-alone check).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <numeric>
#include <vector>

// No a * b + c may become an FMA. The pragma goes inside the function bodies:
// at file scope it would reach whatever is included after this header.
#if defined(__clang__)
#define TPE_BELOW_FP_CONTRACT_OFF _Pragma("clang fp contract(off)")
#elif defined(__GNUC__)
// GCC ignores the STDC pragma; contraction is switched off around the
// functions with push_options below.
#define TPE_BELOW_FP_CONTRACT_OFF
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#else
#define TPE_BELOW_FP_CONTRACT_OFF _Pragma("STDC FP_CONTRACT OFF")
#endif

namespace tpe_below {

// numpy's maximum / minimum on doubles (a NaN operand wins).
inline double np_max(double x, double y) { return (x >= y || x != x) ? x : y; }
inline double np_min(double x, double y) { return (x <= y || x != x) ? x : y; }

// numpy's sort order on doubles: ascending, NaN last.
inline bool np_less(double x, double y) { return x < y || (y != y && x == x); }

// Fit and gather.
//   obs     (n, D)    valid below rows in trial-number order, KDE domain
//   alow, ahigh (D,)  adapted bounds
//   active  (S,)      kernel indices in [0, n] (checked by the caller)
//   mus, sigmas (n + 1, D)  kernels, the prior kernel last
//   a, b, loc, scale (S, D) loc = mus[active], scale = sigmas[active],
//                           a = (alow - loc) / scale, b = (ahigh - loc) / scale
// Per dim the sigmas are the larger gap to the neighbours in a stable sort of
// the column (ties keep row order) padded with alow / ahigh; without
// consider_endpoints and with n >= 2 the first and last sorted kernels take
// their inner gap. Sigmas are clipped to [minsig, range], minsig =
// range / min(100, 1 + (n + 1)) with the magic clip and 1e-12 without. The
// prior kernel is (0.5 * (alow + ahigh), range).
inline void fit_and_gather(const double* obs, size_t n, size_t D,
                           const double* alow, const double* ahigh,
                           bool consider_endpoints, bool consider_magic_clip,
                           const int64_t* active, size_t S, double* mus,
                           double* sigmas, double* a, double* b, double* loc,
                           double* scale) {
    TPE_BELOW_FP_CONTRACT_OFF
    std::vector<double> col(n), padded(n + 2), sorted_sigma(n);
    std::vector<size_t> order(n);
    const double clip_div = std::min(100.0, 1.0 + (double)(n + 1));
    for (size_t c = 0; c < D; ++c) {
        const double lo = alow[c], hi = ahigh[c];
        const double range = hi - lo;
        for (size_t k = 0; k < n; ++k) {
            col[k] = obs[k * D + c];
            mus[k * D + c] = col[k];
        }
        mus[n * D + c] = 0.5 * (lo + hi);
        sigmas[n * D + c] = range;
        if (n == 0) continue;

        std::iota(order.begin(), order.end(), (size_t)0);
        std::stable_sort(order.begin(), order.end(), [&](size_t i, size_t j) {
            return np_less(col[i], col[j]);
        });
        padded[0] = lo;
        for (size_t i = 0; i < n; ++i) padded[i + 1] = col[order[i]];
        padded[n + 1] = hi;
        for (size_t i = 0; i < n; ++i)
            sorted_sigma[i] = np_max(padded[i + 1] - padded[i],
                                     padded[i + 2] - padded[i + 1]);
        if (!consider_endpoints && n >= 2) {
            sorted_sigma[0] = padded[2] - padded[1];
            sorted_sigma[n - 1] = padded[n] - padded[n - 1];
        }
        const double minsig = consider_magic_clip ? range / clip_div : 1e-12;
        for (size_t i = 0; i < n; ++i)
            sigmas[order[i] * D + c] =
                np_min(np_max(sorted_sigma[i], minsig), range);
    }
    for (size_t s = 0; s < S; ++s) {
        const size_t k = (size_t)active[s];
        for (size_t c = 0; c < D; ++c) {
            const double m = mus[k * D + c], sg = sigmas[k * D + c];
            loc[s * D + c] = m;
            scale[s * D + c] = sg;
            a[s * D + c] = (alow[c] - m) / sg;
            b[s * D + c] = (ahigh[c] - m) / sg;
        }
    }
}

}  // namespace tpe_below

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC pop_options
#endif
#undef TPE_BELOW_FP_CONTRACT_OFF
