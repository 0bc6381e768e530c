// Host driver for optuna_amd/_hip/csrc/tpe_below_host.h, compiled and run by
// tests/test_tpe_below_native.py:  tpe_below_check CASES_IN RESULTS_OUT
//
// CASES_IN (native endianness): int64 n_cases, then per case
//   int64 n, D, S, consider_endpoints, consider_magic_clip
//   double obs[n * D], alow[D], ahigh[D];  int64 active[S]
// RESULTS_OUT: per case, double mus[(n + 1) * D], sigmas[(n + 1) * D],
//   a[S * D], b[S * D], loc[S * D], scale[S * D].
// The comparison with the Python estimator is done by the test.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "tpe_below_host.h"

template <typename T>
static bool read_n(std::FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

static bool write_n(std::FILE* f, const std::vector<double>& v) {
    return v.empty() || std::fwrite(v.data(), sizeof(double), v.size(), f) == v.size();
}

int main(int argc, char** argv) {
    if (argc != 3) {
        std::printf("usage: %s CASES_IN RESULTS_OUT\n", argv[0]);
        return 2;
    }
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) {
        std::printf("cannot open the case or the result file\n");
        return 2;
    }
    std::vector<int64_t> head, active;
    std::vector<double> obs, alow, ahigh;
    if (!read_n(in, head, 1) || head[0] < 0) {
        std::printf("bad case file header\n");
        return 2;
    }
    const int64_t n_cases = head[0];
    for (int64_t i = 0; i < n_cases; ++i) {
        if (!read_n(in, head, 5) || head[0] < 0 || head[1] < 1 || head[2] < 0) {
            std::printf("case %lld: bad header\n", (long long)i);
            return 2;
        }
        const size_t n = (size_t)head[0], D = (size_t)head[1], S = (size_t)head[2];
        if (!read_n(in, obs, n * D) || !read_n(in, alow, D) || !read_n(in, ahigh, D) ||
            !read_n(in, active, S)) {
            std::printf("case %lld: truncated\n", (long long)i);
            return 2;
        }
        for (size_t s = 0; s < S; ++s)
            if (active[s] < 0 || (size_t)active[s] > n) {
                std::printf("case %lld: active out of range\n", (long long)i);
                return 2;
            }
        std::vector<double> mus((n + 1) * D), sigmas((n + 1) * D);
        std::vector<double> a(S * D), b(S * D), loc(S * D), scale(S * D);
        tpe_below::fit_and_gather(obs.data(), n, D, alow.data(), ahigh.data(),
                                  head[3] != 0, head[4] != 0, active.data(), S,
                                  mus.data(), sigmas.data(), a.data(), b.data(),
                                  loc.data(), scale.data());
        if (!write_n(out, mus) || !write_n(out, sigmas) || !write_n(out, a) ||
            !write_n(out, b) || !write_n(out, loc) || !write_n(out, scale)) {
            std::printf("case %lld: write failed\n", (long long)i);
            return 2;
        }
    }
    std::fclose(in);
    if (std::fclose(out) != 0) {
        std::printf("closing the result file failed\n");
        return 2;
    }
    std::printf("tpe_below: %lld cases written\n", (long long)n_cases);
    return 0;
}
