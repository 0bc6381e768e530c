// Stand-alone driver for optuna_amd/_hip/csrc/tpe_draw_host.h, compiled and
// run by tests/test_tpe_draw_native.py (once plain, once with
// -fsanitize=address,undefined):  tpe_draw_check
//
// The callbacks are libm stand-ins, so the values are only approximately
// scipy's and numpy's: this program checks memory safety and structure over
// the edge shapes (every finite quantile inside [a, b], NaN where a >= b,
// indices in range, stepped values on their grid). Bit equality with the
// Python code is the pybind test's job.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "tpe_draw_host.h"

static double s_ndtr(double x, int) { return 0.5 * std::erfc(-x / std::sqrt(2.0)); }

static double s_log_ndtr(double x, int) {
    if (x < -20.0)  // leading term of the asymptotic series
        return -0.5 * x * x - std::log(-x) - 0.5 * std::log(2.0 * M_PI);
    return std::log(s_ndtr(x, 0));
}

static double s_ndtri_exp(double y, int) {
    if (y != y) return y;
    if (y >= 0) return std::numeric_limits<double>::infinity();
    double lo = -1e4, hi = 40.0;
    for (int it = 0; it < 200; ++it) {
        const double mid = 0.5 * (lo + hi);
        (s_log_ndtr(mid, 0) < y ? lo : hi) = mid;
    }
    return 0.5 * (lo + hi);
}

static void v_log(void*, const double* in, double* out, size_t n) {
    for (size_t i = 0; i < n; ++i) out[i] = std::log(in[i]);
}
static void v_log1p(void*, const double* in, double* out, size_t n) {
    for (size_t i = 0; i < n; ++i) out[i] = std::log1p(in[i]);
}
static void v_exp(void*, const double* in, double* out, size_t n) {
    for (size_t i = 0; i < n; ++i) out[i] = std::exp(in[i]);
}
static void v_logaddexp(void*, const double* x, const double* y, double* out, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        const double a = x[i], b = y[i];
        if (a == b) out[i] = a + std::log(2.0);
        else if (a - b > 0) out[i] = a + std::log1p(std::exp(b - a));
        else if (a - b <= 0) out[i] = b + std::log1p(std::exp(a - b));
        else out[i] = a - b;  // NaN
    }
}

static uint64_t g_state = 88172645463325252ull;
static double unif() {  // xorshift64, [0, 1)
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return (double)(g_state >> 11) / 9007199254740992.0;
}

static int fail(const char* what, size_t n, size_t i) {
    std::printf("tpe_draw: %s (n = %zu, element %zu)\n", what, n, i);
    return 1;
}

int main() {
    tpe_draw::Ops op;
    op.ndtr = s_ndtr;
    op.log_ndtr = s_log_ndtr;
    op.ndtri_exp = s_ndtri_exp;
    op.log = v_log;
    op.log1p = v_log1p;
    op.exp = v_exp;
    op.logaddexp = v_logaddexp;
    tpe_draw::Workspace ws;

    // Quantile over the edge shapes; the interval kinds rotate per element.
    const size_t sizes[] = {1, 20, 24, 21, 480, 481};
    for (size_t n : sizes) {
        std::vector<double> q(n), a(n), b(n), out(n, -1.0);
        for (size_t i = 0; i < n; ++i) {
            const double w = 0.01 + 10.0 * unif();
            switch (i % 8) {
                case 0: a[i] = -3.0 * unif() - 0.1; b[i] = a[i] + w; break;  // a < 0
                case 1: a[i] = -50.0 - unif(); b[i] = a[i] + w; break;       // far left
                case 2: a[i] = 0.1 + 3.0 * unif(); b[i] = a[i] + w; break;   // right
                case 3: a[i] = 38.0 + unif(); b[i] = a[i] + w; break;        // far right
                case 4: a[i] = -w; b[i] = w; break;                          // straddling
                case 5: a[i] = 0.0; b[i] = w; break;                         // a == 0
                case 6: a[i] = b[i] = unif() - 0.5; break;                   // a == b
                default: a[i] = 1.0; b[i] = -1.0; break;                     // a > b
            }
            q[i] = i % 5 == 0 ? 0.0 : (i % 7 == 0 ? 1.0 : unif());
        }
        tpe_draw::ppf(op, q.data(), a.data(), b.data(), n, out.data(), ws);
        for (size_t i = 0; i < n; ++i) {
            if (a[i] >= b[i]) {
                if (out[i] == out[i]) return fail("a >= b must give NaN", n, i);
            } else if (std::isfinite(out[i]) && (out[i] < a[i] || out[i] > b[i])) {
                return fail("quantile outside [a, b]", n, i);
            } else if (out[i] != out[i]) {
                return fail("NaN inside a proper interval", n, i);
            }
        }
    }

    // Kernel choice.
    const size_t kernels[] = {1, 2, 26, 1025};
    for (size_t n : kernels) {
        std::vector<double> w(n), u(24);
        double total = 0.0;
        for (size_t i = 0; i < n; ++i) total += w[i] = i % 3 == 1 ? 0.0 : unif();
        if (total == 0.0) w[0] = total = 1.0;
        for (double& v : w) v /= total;
        for (double& v : u) v = unif();
        u[0] = 0.0;
        std::vector<int64_t> active(u.size(), -1);
        tpe_draw::choose(w.data(), n, u.data(), u.size(), active.data(), ws);
        for (size_t s = 0; s < u.size(); ++s)
            if (active[s] < 0 || (size_t)active[s] >= n || w[(size_t)active[s]] == 0.0)
                return fail("choice out of range or of a zero weight", n, s);
    }

    // Candidates: one dim of every kind, odd candidate count.
    {
        const size_t S = 7, D = 4;
        const int8_t kinds[D] = {tpe_draw::KIND_CONT, tpe_draw::KIND_LOG,
                                 tpe_draw::KIND_DISC, tpe_draw::KIND_LOG_DISC};
        const double lows[D] = {-5.0, 1e-3, -5.0, 1.0};
        const double highs[D] = {5.0, 10.0, 5.0, 64.0};
        const double steps[D] = {0.0, 0.0, 0.5, 1.0};
        std::vector<double> p(S * D), loc(S * D), scale(S * D, 1.0);
        for (size_t i = 0; i < S * D; ++i) {
            p[i] = 2.0 * unif() - 1.0;
            loc[i] = i % D == 1 ? -2.0 : (i % D == 3 ? 2.0 : 0.0);
        }
        std::vector<double> x_raw(S * D), x_kde(S * D), xedges(2 * S * D, -1.0);
        tpe_draw::to_candidates(op, p.data(), loc.data(), scale.data(), S, D, kinds,
                                lows, highs, steps, x_raw.data(), x_kde.data(),
                                xedges.data(), ws);
        for (size_t s = 0; s < S; ++s)
            for (size_t c = 0; c < D; ++c) {
                const double v = x_raw[s * D + c];
                if (steps[c] > 0) {
                    const double cells = (v - lows[c]) / steps[c];
                    if (v < lows[c] || v > highs[c] || cells != std::nearbyint(cells))
                        return fail("stepped value off its grid", S, s * D + c);
                    if (!(xedges[s * 2 * D + c] < xedges[s * 2 * D + D + c]))
                        return fail("cell edges out of order", S, s * D + c);
                } else if (xedges[s * 2 * D + c] != 0.0 || xedges[s * 2 * D + D + c] != 0.0) {
                    return fail("edges of a continuous dim must be zero", S, s * D + c);
                }
            }
        // Without edges (no stepped dim on the device side).
        tpe_draw::to_candidates(op, p.data(), loc.data(), scale.data(), S, D, kinds,
                                lows, highs, steps, x_raw.data(), x_kde.data(),
                                nullptr, ws);
        std::vector<double> obs = {1e-3, 10.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0};
        tpe_draw::log_observations(op, obs.data(), 2, D, kinds, ws);
        if (obs[0] != 1e-3 || obs[1] != std::log(10.0) || obs[7] != std::log(6.0))
            return fail("log of the log dims only", 2, 0);
    }

    // Arg-max.
    {
        const double inf = std::numeric_limits<double>::infinity();
        const double nan = std::numeric_limits<double>::quiet_NaN();
        const double ties[] = {1.0, 3.0, 3.0, 2.0}, ninf[] = {-inf, -inf, -inf};
        const double with_nan[] = {1.0, 5.0, nan, 9.0, nan};
        if (tpe_draw::argmax(ties, 4) != 1 || tpe_draw::argmax(ninf, 3) != 0 ||
            tpe_draw::argmax(with_nan, 5) != 2)
            return fail("arg-max rule", 0, 0);
    }
    std::printf("tpe_draw: ok\n");
    return 0;
}
