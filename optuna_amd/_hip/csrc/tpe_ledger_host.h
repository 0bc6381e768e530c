// Split ledger of the fused TPE suggest: the feasible complete rows of one
// study's history, kept sorted by objective value, and the host arithmetic
// that stands between a tell and the above-set fit (the below rows, the
// exclusion list, the default weight ramp). It replaces O(N) numpy work per
// step (_history.py's np.insert pair and split's masks) by a binary search, a
// memmove and O(n_below) work.
//
// Plain C++17 on pointers and sizes: no HIP, no pybind (see
// tests/cpp/tpe_ledger_check.cpp for the stand-alone check).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <utility>
#include <vector>

namespace tpe_ledger {

// Value-sorted list of (key, row) in two capacity-doubled parallel arrays.
// The key is the objective value of a minimize study and its negation for a
// maximize study (the caller applies the sign). Entries with equal keys stay
// in arrival order (-0.0 and 0.0 compare equal), so when rows arrive in
// ascending order the list equals np.argsort(keys, kind="stable") over the
// whole column. NaN keys have no place in that order and are refused.
class TpeSplitLedger {
  public:
    size_t size() const { return n_; }
    size_t capacity() const { return cap_; }
    const double* keys() const { return keys_.get(); }
    const int64_t* rows() const { return rows_.get(); }

    // Behind every entry with an equal or smaller key (upper_bound).
    void insert(int64_t row, double key) {
        if (key != key) throw std::invalid_argument("TpeSplitLedger: NaN key");
        reserve(n_ + 1);
        double* k = keys_.get();
        int64_t* r = rows_.get();
        const size_t i = (size_t)(std::upper_bound(k, k + n_, key) - k);
        std::memmove(k + i + 1, k + i, (n_ - i) * sizeof(double));
        std::memmove(r + i + 1, r + i, (n_ - i) * sizeof(int64_t));
        k[i] = key;
        r[i] = row;
        ++n_;
    }

    // m entries at once, equal to m inserts in the given order: the batch is
    // sorted stably and merged from the back (O(n + m log m), for the first
    // fill of a long history).
    void insert_many(const int64_t* rows, const double* keys, size_t m) {
        for (size_t j = 0; j < m; ++j)
            if (keys[j] != keys[j])
                throw std::invalid_argument("TpeSplitLedger: NaN key");
        if (m <= 4) {
            for (size_t j = 0; j < m; ++j) insert(rows[j], keys[j]);
            return;
        }
        std::vector<std::pair<double, int64_t>> batch(m);
        for (size_t j = 0; j < m; ++j) batch[j] = {keys[j], rows[j]};
        std::stable_sort(batch.begin(), batch.end(),
                         [](const auto& a, const auto& b) { return a.first < b.first; });
        reserve(n_ + m);
        double* k = keys_.get();
        int64_t* r = rows_.get();
        size_t i = n_, j = m, o = n_ + m;
        while (j > 0) {
            // An old entry moves up only past strictly smaller new keys, so
            // equal keys keep the old entries in front.
            if (i > 0 && k[i - 1] > batch[j - 1].first) {
                --i, --o;
                k[o] = k[i];
                r[o] = r[i];
            } else {
                --j, --o;
                k[o] = batch[j].first;
                r[o] = batch[j].second;
            }
        }
        n_ += m;
    }

    // The rows of the first min(k, n) entries, ascending by row, written to
    // out (room for min(k, n) values); returns their number. With rows in
    // trial-number order this is below[np.argsort(numbers[below], "stable")].
    size_t below(size_t k, int64_t* out) const {
        const size_t m = std::min(k, n_);
        std::copy(rows_.get(), rows_.get() + m, out);
        std::sort(out, out + m);
        return m;
    }

  private:
    void reserve(size_t need) {
        if (need <= cap_) return;
        const size_t cap = std::max<size_t>({64, 2 * cap_, need});
        std::unique_ptr<double[]> k(new double[cap]);
        std::unique_ptr<int64_t[]> r(new int64_t[cap]);
        if (n_) {
            std::memcpy(k.get(), keys_.get(), n_ * sizeof(double));
            std::memcpy(r.get(), rows_.get(), n_ * sizeof(int64_t));
        }
        keys_ = std::move(k);
        rows_ = std::move(r);
        cap_ = cap;
    }

    std::unique_ptr<double[]> keys_;
    std::unique_ptr<int64_t[]> rows_;
    size_t n_ = 0, cap_ = 0;
};

// Sorted union of the ascending below rows and the ascending invalid rows as
// int32 table rows, written to out (room for n_below + n_invalid values);
// returns its length. What _SpaceCache.excluded_rows builds with np.union1d.
inline size_t exclusion_list(const int64_t* below, size_t n_below,
                             const int32_t* invalid, size_t n_invalid,
                             int32_t* out) {
    size_t i = 0, j = 0, o = 0;
    while (i < n_below || j < n_invalid) {
        int32_t v;
        if (j == n_invalid || (i < n_below && below[i] <= (int64_t)invalid[j])) {
            v = (int32_t)below[i];
            if (j < n_invalid && (int64_t)invalid[j] == below[i]) ++j;
            ++i;
        } else {
            v = invalid[j++];
        }
        out[o++] = v;
    }
    return o;
}

// _device.default_weight_ramp(n, prior_weight) in the same expression order,
// math.log being libm's log: the same bits.
struct WeightRamp {
    int64_t num;
    double start, step, log_total;
};

inline WeightRamp default_weight_ramp(int64_t n, double prior_weight) {
    if (n < 25)
        return {0, 1.0, 0.0, n ? std::log((double)n + prior_weight) : 0.0};
    const int64_t num = n - 25;
    const double start = 1.0 / (double)n;
    const double step = num > 1 ? (1.0 - start) / (double)(num - 1) : 0.0;
    const double ramp_sum =
        num > 1 ? (double)num * (start + 1.0) / 2.0 : start * (double)num;
    return {num, start, step, std::log(ramp_sum + 25.0 + prior_weight)};
}

}  // namespace tpe_ledger
