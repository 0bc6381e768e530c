// Host half of the fused TPE suggest between the below fit and the chosen
// candidate: the kernel choice from uniforms, the truncated-normal quantile
// (_truncnorm_np.ppf with _log_gauss_mass), the transform to the parameter
// domain, the scoring inputs that _device.score_fused derives from the draws,
// and the arg-max. The outputs equal the numpy/scipy expressions bit for bit.
//
// Plain C++17 on pointers and sizes: no HIP, no pybind (see
// tests/cpp/tpe_draw_check.cpp for the stand-alone check). The special
// functions come in through Ops:
//   * scipy's scalar ndtr / log_ndtr / ndtri_exp are called per element;
//   * log, log1p, exp and logaddexp are numpy's own loops, whose last bit
//     differs from libm's. They give the same value for an element wherever it
//     stands in a contiguous array, so each is called once per stage on a
//     packed array of every element that needs it.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <vector>

// No a * b + c may become an FMA (ppf * scale + loc, lo + round(..) * st).
// The pragma goes inside the function bodies: at file scope it would reach
// whatever is included after this header.
#if defined(__clang__)
#define TPE_DRAW_FP_CONTRACT_OFF _Pragma("clang fp contract(off)")
#elif defined(__GNUC__)
// GCC ignores the STDC pragma; contraction is switched off around the
// functions with push_options below.
#define TPE_DRAW_FP_CONTRACT_OFF
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#else
#define TPE_DRAW_FP_CONTRACT_OFF _Pragma("STDC FP_CONTRACT OFF")
#endif

namespace tpe_draw {

// Dimension kinds (parzen.py KIND_*).
constexpr int8_t KIND_CONT = 0, KIND_LOG = 1, KIND_DISC = 2, KIND_LOG_DISC = 3;

struct Ops {
    // scipy.special.cython_special: double f(double, int skip_dispatch).
    double (*ndtr)(double, int) = nullptr;
    double (*log_ndtr)(double, int) = nullptr;
    double (*ndtri_exp)(double, int) = nullptr;
    // numpy's elementwise loops over n contiguous doubles (in != out).
    void (*log)(void* ctx, const double* in, double* out, size_t n) = nullptr;
    void (*log1p)(void* ctx, const double* in, double* out, size_t n) = nullptr;
    void (*exp)(void* ctx, const double* in, double* out, size_t n) = nullptr;
    void (*logaddexp)(void* ctx, const double* x, const double* y, double* out,
                      size_t n) = nullptr;
    void* ctx = nullptr;
};

// Reusable temporaries: a suggest allocates nothing once they have grown.
struct Workspace {
    std::vector<double> f[9];
    std::vector<uint32_t> at[3];
    double* get(int i, size_t n) {
        if (f[i].size() < n) f[i].resize(n);
        return f[i].data();
    }
    uint32_t* idx(int i, size_t n) {
        if (at[i].size() < n) at[i].resize(n);
        return at[i].data();
    }
};

// numpy's clip on doubles: a NaN x stays, otherwise comparisons pick (so
// clip(-0.0, 0.0, hi) is +0.0 and a NaN bound comes through).
inline double np_clip(double x, double lo, double hi) {
    if (x != x) return x;
    const double t = x > lo ? x : lo;
    if (t != t) return t;
    return t < hi ? t : hi;
}

// RandomState.choice(n, p=w, size=S) after its argument checks, given its
// one random_sample(S) draw u: cdf = cumsum(w) (sequential), cdf /= cdf[-1],
// searchsorted(cdf, u, side="right"). Indices lie in [0, n].
inline void choose(const double* w, size_t n, const double* u, size_t S,
                   int64_t* active, Workspace& ws) {
    TPE_DRAW_FP_CONTRACT_OFF
    if (n == 0) return;
    double* cdf = ws.get(0, n);
    cdf[0] = w[0];
    for (size_t i = 1; i < n; ++i) cdf[i] = cdf[i - 1] + w[i];
    const double total = cdf[n - 1];
    for (size_t i = 0; i < n; ++i) cdf[i] /= total;
    for (size_t s = 0; s < S; ++s)
        active[s] = (int64_t)(std::upper_bound(cdf, cdf + n, u[s]) - cdf);
}

// Quantile of the standard normal truncated to [a, b] at q, n elements each:
// _truncnorm_np.ppf. Per element
//   mass = -inf                                         where !(a < b)
//        = lb + log1p(-exp(log_ndtr(-b) - lb)), lb = log_ndtr(-a)  where a > 0
//        = lb + log1p(-exp(log_ndtr(a) - lb)),  lb = log_ndtr(b)   where b <= 0
//        = log1p(-ndtr(a) - ndtr(-b))                              otherwise
//   out  =  ndtri_exp(logaddexp(log_ndtr(a),  log(q)    + mass))   where a < 0
//        = -ndtri_exp(logaddexp(log_ndtr(-b), log1p(-q) + mass))   otherwise
// clipped to [a, b], NaN where a >= b. A scalar that two of these terms share
// (same function, same argument) is evaluated once.
inline void ppf(const Ops& op, const double* q, const double* a, const double* b,
                size_t n, double* out, Workspace& ws) {
    TPE_DRAW_FP_CONTRACT_OFF
    if (n == 0) return;
    const double ninf = -std::numeric_limits<double>::infinity();
    double* lx = ws.get(0, n);    // first operand of logaddexp
    double* ly = ws.get(1, n);    // second operand, then its result
    double* mass = ws.get(2, n);  // lb until the log1p term is added
    double* e_in = ws.get(3, n);
    double* e_out = ws.get(4, n);
    // log1p batch: central mass terms | tail mass terms | -q of a >= 0.
    double* p_in = ws.get(5, 2 * n);
    double* p_out = ws.get(6, 2 * n);
    double* g_in = ws.get(7, n);  // log batch: q of a < 0
    double* g_out = ws.get(8, n);
    uint32_t* e_at = ws.idx(0, n);
    uint32_t* p_at = ws.idx(1, 2 * n);
    uint32_t* g_at = ws.idx(2, n);
    size_t ne = 0, np = 0, ng = 0;

    for (size_t i = 0; i < n; ++i) {
        const double ai = a[i], bi = b[i];
        const bool left = ai < 0;
        if (left) {
            g_in[ng] = q[i];
            g_at[ng++] = (uint32_t)i;
        }
        if (!(ai < bi)) {
            mass[i] = ninf;
            lx[i] = left ? op.log_ndtr(ai, 0) : op.log_ndtr(-bi, 0);
        } else if (ai > 0) {
            const double lb = op.log_ndtr(-ai, 0);
            const double t = op.log_ndtr(-bi, 0);
            e_in[ne] = t - lb;
            e_at[ne++] = (uint32_t)i;
            mass[i] = lb;
            lx[i] = t;
        } else if (bi <= 0) {
            const double lb = op.log_ndtr(bi, 0);
            const double t = op.log_ndtr(ai, 0);
            e_in[ne] = t - lb;
            e_at[ne++] = (uint32_t)i;
            mass[i] = lb;
            lx[i] = t;
        } else {
            p_in[np] = -op.ndtr(ai, 0) - op.ndtr(-bi, 0);
            p_at[np++] = (uint32_t)i;
            lx[i] = left ? op.log_ndtr(ai, 0) : op.log_ndtr(-bi, 0);
        }
    }
    const size_t n_central = np;
    if (ne) op.exp(op.ctx, e_in, e_out, ne);
    for (size_t k = 0; k < ne; ++k) {
        p_in[np] = -e_out[k];
        p_at[np++] = e_at[k];
    }
    const size_t n_mass = np;
    for (size_t i = 0; i < n; ++i)
        if (!(a[i] < 0)) {
            p_in[np] = -q[i];
            p_at[np++] = (uint32_t)i;
        }
    if (np) op.log1p(op.ctx, p_in, p_out, np);
    if (ng) op.log(op.ctx, g_in, g_out, ng);
    for (size_t k = 0; k < n_central; ++k) mass[p_at[k]] = p_out[k];
    for (size_t k = n_central; k < n_mass; ++k)
        mass[p_at[k]] = mass[p_at[k]] + p_out[k];
    for (size_t k = n_mass; k < np; ++k) ly[p_at[k]] = p_out[k] + mass[p_at[k]];
    for (size_t k = 0; k < ng; ++k) ly[g_at[k]] = g_out[k] + mass[g_at[k]];
    double* r = e_in;  // free again
    op.logaddexp(op.ctx, lx, ly, r, n);
    for (size_t i = 0; i < n; ++i) {
        const double ai = a[i], bi = b[i];
        const double v = ai < 0 ? op.ndtri_exp(r[i], 0) : -op.ndtri_exp(r[i], 0);
        out[i] = ai >= bi ? std::numeric_limits<double>::quiet_NaN()
                          : np_clip(v, ai, bi);
    }
}

// Below observations to the KDE domain, in place: the log of the log dims
// (the head of _device.draw_below_native).
inline void log_observations(const Ops& op, double* obs, size_t n, size_t D,
                             const int8_t* kinds, Workspace& ws) {
    size_t n_log = 0;
    for (size_t c = 0; c < D; ++c)
        n_log += kinds[c] == KIND_LOG || kinds[c] == KIND_LOG_DISC;
    if (n_log == 0 || n == 0) return;
    double* in = ws.get(0, n * n_log);
    double* out = ws.get(1, n * n_log);
    size_t k = 0;
    for (size_t r = 0; r < n; ++r)
        for (size_t c = 0; c < D; ++c)
            if (kinds[c] == KIND_LOG || kinds[c] == KIND_LOG_DISC)
                in[k++] = obs[r * D + c];
    op.log(op.ctx, in, out, k);
    k = 0;
    for (size_t r = 0; r < n; ++r)
        for (size_t c = 0; c < D; ++c)
            if (kinds[c] == KIND_LOG || kinds[c] == KIND_LOG_DISC)
                obs[r * D + c] = out[k++];
}

// From the quantiles to the candidates and the scoring inputs.
//   p, loc, scale (S, D)   quantiles and the drawn kernels
//   x_raw (S, D)   p * scale + loc through parzen.py's _to_param_domain: exp
//                  for log dims, clip(lo + rint((x - lo) / st) * st, lo, hi)
//                  for stepped dims
//   x_kde (S, D)   x_raw with the log dims logged (what score_fused uploads)
//   xedges (S, 2D) _device._cell_edges: x_raw -/+ step / 2 for stepped dims,
//                  logged for log dims, zeros elsewhere; nullptr to skip
inline void to_candidates(const Ops& op, const double* p, const double* loc,
                          const double* scale, size_t S, size_t D,
                          const int8_t* kinds, const double* lows,
                          const double* highs, const double* steps,
                          double* x_raw, double* x_kde, double* xedges,
                          Workspace& ws) {
    TPE_DRAW_FP_CONTRACT_OFF
    const size_t n = S * D;
    size_t n_log = 0, n_log_step = 0;
    for (size_t c = 0; c < D; ++c) {
        const bool is_log = kinds[c] == KIND_LOG || kinds[c] == KIND_LOG_DISC;
        n_log += is_log;
        n_log_step += is_log && steps[c] > 0 && xedges != nullptr;
    }
    for (size_t i = 0; i < n; ++i) x_raw[i] = p[i] * scale[i] + loc[i];
    const auto is_log = [&](size_t c) {
        return kinds[c] == KIND_LOG || kinds[c] == KIND_LOG_DISC;
    };
    double* in = ws.get(0, S * (n_log + 2 * n_log_step));
    double* out = ws.get(1, S * (n_log + 2 * n_log_step));
    if (n_log) {
        size_t k = 0;
        for (size_t s = 0; s < S; ++s)
            for (size_t c = 0; c < D; ++c)
                if (is_log(c)) in[k++] = x_raw[s * D + c];
        op.exp(op.ctx, in, out, k);
        k = 0;
        for (size_t s = 0; s < S; ++s)
            for (size_t c = 0; c < D; ++c)
                if (is_log(c)) x_raw[s * D + c] = out[k++];
    }
    for (size_t c = 0; c < D; ++c) {
        if (!(steps[c] > 0)) continue;
        const double lo = lows[c], hi = highs[c], st = steps[c];
        for (size_t s = 0; s < S; ++s) {
            const double v = x_raw[s * D + c];
            x_raw[s * D + c] =
                np_clip(lo + std::nearbyint((v - lo) / st) * st, lo, hi);
        }
    }
    for (size_t i = 0; i < n; ++i) x_kde[i] = x_raw[i];
    if (xedges != nullptr) {
        for (size_t i = 0; i < 2 * n; ++i) xedges[i] = 0.0;
        for (size_t c = 0; c < D; ++c) {
            if (!(steps[c] > 0)) continue;
            const double half = steps[c] / 2;
            for (size_t s = 0; s < S; ++s) {
                xedges[s * 2 * D + c] = x_raw[s * D + c] - half;
                xedges[s * 2 * D + D + c] = x_raw[s * D + c] + half;
            }
        }
    }
    if (n_log) {
        // One log call: x of the log dims, then the cell edges of the
        // log-stepped dims.
        size_t k = 0;
        for (size_t s = 0; s < S; ++s)
            for (size_t c = 0; c < D; ++c)
                if (is_log(c)) in[k++] = x_raw[s * D + c];
        if (n_log_step)
            for (size_t s = 0; s < S; ++s)
                for (size_t c = 0; c < D; ++c)
                    if (is_log(c) && steps[c] > 0) {
                        in[k++] = xedges[s * 2 * D + c];
                        in[k++] = xedges[s * 2 * D + D + c];
                    }
        op.log(op.ctx, in, out, k);
        k = 0;
        for (size_t s = 0; s < S; ++s)
            for (size_t c = 0; c < D; ++c)
                if (is_log(c)) x_kde[s * D + c] = out[k++];
        if (n_log_step)
            for (size_t s = 0; s < S; ++s)
                for (size_t c = 0; c < D; ++c)
                    if (is_log(c) && steps[c] > 0) {
                        xedges[s * 2 * D + c] = out[k++];
                        xedges[s * 2 * D + D + c] = out[k++];
                    }
    }
}

// np.argmax on doubles: the first NaN if there is one, else the first maximum.
inline size_t argmax(const double* v, size_t n) {
    size_t best = 0;
    for (size_t i = 0; i < n; ++i) {
        if (v[i] != v[i]) return i;
        if (v[i] > v[best]) best = i;
    }
    return best;
}

}  // namespace tpe_draw

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC pop_options
#endif
#undef TPE_DRAW_FP_CONTRACT_OFF
