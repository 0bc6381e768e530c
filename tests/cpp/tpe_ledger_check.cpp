// Stand-alone check of optuna_amd/_hip/csrc/tpe_ledger_host.h, built with the
// host compiler by tests/test_tpe_ledger_native.py (plain, and under the
// address and undefined-behaviour sanitizers). Every case inserts keys in
// arrival order and compares the ledger with a stable sort of the whole
// column (the comparison with numpy goes through tpe_ledger_module.cpp).
#include <cmath>
#include <cstdio>
#include <limits>
#include <numeric>
#include <string>

#include "tpe_ledger_host.h"

namespace {

int g_failures = 0;

void fail(const std::string& name, const char* what) {
    std::printf("FAIL %s: %s\n", name.c_str(), what);
    ++g_failures;
}

// Deterministic 64-bit generator (splitmix64).
uint64_t next_u64(uint64_t& s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// `batch` > 0 feeds the keys through insert_many in batches of that size.
void run_case(const std::string& name, const std::vector<double>& keys,
              size_t batch = 0) {
    const size_t n = keys.size();
    tpe_ledger::TpeSplitLedger L;
    if (batch == 0) {
        for (size_t r = 0; r < n; ++r) L.insert((int64_t)r, keys[r]);
    } else {
        std::vector<int64_t> rows(n);
        std::iota(rows.begin(), rows.end(), (int64_t)0);
        for (size_t at = 0; at < n; at += batch) {
            const size_t m = std::min(batch, n - at);
            L.insert_many(rows.data() + at, keys.data() + at, m);
        }
    }
    if (L.size() != n) fail(name, "size");
    if (n > 0 && L.capacity() < n) fail(name, "capacity");

    std::vector<int64_t> want(n);
    std::iota(want.begin(), want.end(), (int64_t)0);
    std::stable_sort(want.begin(), want.end(),
                     [&](int64_t a, int64_t b) { return keys[a] < keys[b]; });
    for (size_t i = 0; i < n; ++i) {
        if (L.rows()[i] != want[i]) {
            fail(name, "rows differ from the stable sort");
            break;
        }
        if (std::memcmp(&L.keys()[i], &keys[want[i]], sizeof(double)) != 0) {
            fail(name, "keys do not travel with their rows");
            break;
        }
    }

    const size_t ks[] = {0, 1, n / 10, n / 2, n > 0 ? n - 1 : 0, n, n + 1, n + 1000};
    for (size_t k : ks) {
        std::vector<int64_t> got(std::min(k, n) + 1, -7);
        const size_t m = L.below(k, got.data());
        if (m != std::min(k, n) || got[m] != -7) {
            fail(name, "below: length");
            continue;
        }
        std::vector<int64_t> exp(want.begin(), want.begin() + m);
        std::sort(exp.begin(), exp.end());
        if (!std::equal(exp.begin(), exp.end(), got.begin()))
            fail(name, "below: rows");
    }
}

void check_exclusion() {
    const int64_t below[] = {1, 5, 9, 70000};
    const int32_t invalid[] = {0, 5, 12};
    int32_t out[7];
    const int32_t want[] = {0, 1, 5, 9, 12, 70000};
    size_t E = tpe_ledger::exclusion_list(below, 4, invalid, 3, out);
    if (E != 6 || !std::equal(want, want + 6, out)) fail("exclusion", "union");
    E = tpe_ledger::exclusion_list(below, 0, invalid, 3, out);
    if (E != 3 || !std::equal(invalid, invalid + 3, out)) fail("exclusion", "no below");
    E = tpe_ledger::exclusion_list(below, 4, invalid, 0, out);
    if (E != 4 || out[3] != 70000) fail("exclusion", "no invalid");
    E = tpe_ledger::exclusion_list(below, 0, invalid, 0, out);
    if (E != 0) fail("exclusion", "empty");
}

void check_ramp() {
    auto r = tpe_ledger::default_weight_ramp(0, 1.0);
    if (r.num != 0 || r.start != 1.0 || r.step != 0.0 || r.log_total != 0.0)
        fail("ramp", "n = 0");
    r = tpe_ledger::default_weight_ramp(24, 1.0);
    if (r.num != 0 || r.log_total != std::log(25.0)) fail("ramp", "n = 24");
    r = tpe_ledger::default_weight_ramp(26, 1.0);
    if (r.num != 1 || r.step != 0.0 || r.start != 1.0 / 26.0) fail("ramp", "n = 26");
    r = tpe_ledger::default_weight_ramp(1000, 0.5);
    if (r.num != 975 || r.step != (1.0 - 0.001) / 974.0) fail("ramp", "n = 1000");
}

}  // namespace

int main() {
    const double inf = std::numeric_limits<double>::infinity();

    run_case("empty", {});
    run_case("one", {3.5});
    run_case("all_equal", std::vector<double>(100, 2.0));
    {
        std::vector<double> up(300), down(300);
        for (size_t i = 0; i < 300; ++i) {
            up[i] = (double)i * 0.25;
            down[i] = 1e3 - (double)i;
        }
        run_case("ascending", up);
        run_case("descending", down);
        for (double& v : up) v = -v;  // a maximize study's keys
        run_case("maximize", up);
    }
    run_case("signed_zeros", {0.0, -0.0, 1.0, -0.0, 0.0, -1.0, 0.0, 1.0, -0.0});
    run_case("infinities", {inf, 1.0, -inf, inf, 0.0, -inf, 1.0, inf, -inf, 2.0});
    // Growth across the first capacities (64, 128, 256).
    for (size_t n : {63, 64, 65, 127, 128, 129, 257}) {
        std::vector<double> v(n);
        uint64_t s = 17 * n;
        for (double& x : v) x = (double)(next_u64(s) % 50);
        run_case("capacity_" + std::to_string(n), v);
    }
    {
        // 2000 random inserts, about 10 % of them ties of an earlier key.
        std::vector<double> v(2000);
        uint64_t s = 42;
        for (size_t i = 0; i < v.size(); ++i) {
            const double u = (double)(next_u64(s) >> 11) * 0x1.0p-53;
            v[i] = (i > 0 && next_u64(s) % 10 == 0) ? v[next_u64(s) % i] : u;
        }
        run_case("random_2000", v);
        run_case("random_2000_batches_of_1", v, 1);
        run_case("random_2000_batches_of_7", v, 7);
        run_case("random_2000_batches_of_300", v, 300);
        run_case("random_2000_one_batch", v, 2000);
    }
    {
        tpe_ledger::TpeSplitLedger L;
        L.insert(0, 1.0);
        bool threw = false;
        try {
            L.insert(1, std::nan(""));
        } catch (const std::invalid_argument&) {
            threw = true;
        }
        const int64_t rows[] = {1, 2, 3, 4, 5};
        const double keys[] = {0.0, 1.0, std::nan(""), 2.0, 3.0};
        bool threw_many = false;
        try {
            L.insert_many(rows, keys, 5);
        } catch (const std::invalid_argument&) {
            threw_many = true;
        }
        if (!threw || !threw_many || L.size() != 1) fail("nan", "NaN key accepted");
    }
    check_exclusion();
    check_ramp();

    if (g_failures) {
        std::printf("%d failures\n", g_failures);
        return 1;
    }
    std::printf("tpe_ledger_check ok\n");
    return 0;
}
