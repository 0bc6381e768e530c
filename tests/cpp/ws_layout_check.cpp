// Host check of optuna_amd/_hip/csrc/ws_layout.h, compiled and run by
// tests/test_ws_layout.py. Prints one line per failed check; exit status 1 if
// any failed.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "ws_layout.h"

static int g_failed = 0;

#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);    \
            ++g_failed;                                              \
        }                                                            \
    } while (0)

struct Region {
    size_t offset, bytes;
};

// In order, disjoint, 8-aligned and inside total. A zero-length region may
// share its offset with its successor.
static void check_regions(const std::vector<Region>& r, size_t total) {
    size_t end = 0;
    for (const Region& x : r) {
        CHECK(x.offset % 8 == 0);
        CHECK(x.offset >= end);
        end = x.offset + x.bytes;
        CHECK(end <= total);
    }
}

template <typename T>
static void odd_count_then_double(size_t n) {
    WsLayout L;
    const auto a = L.add<T>(n);
    const auto b = L.add<double>(2);
    check_regions({{a.offset, n * sizeof(T)}, {b.offset, 16}}, L.bytes());
    // Fill both through typed pointers and read both back: a write of the
    // last odd element must not reach the next slot.
    std::vector<char> buf(L.bytes());
    double* pb = b.in(buf.data());
    pb[0] = 1.5;
    pb[1] = -2.5;
    T* pa = a.in(buf.data());
    for (size_t i = 0; i < n; ++i) pa[i] = (T)(i + 1);
    CHECK(pb[0] == 1.5 && pb[1] == -2.5);
    for (size_t i = 0; i < n; ++i) CHECK(pa[i] == (T)(i + 1));
}

int main() {
    {  // mixed types, odd counts
        WsLayout L;
        const auto d = L.add<double>(3);
        const auto i32 = L.add<int32_t>(5);
        const auto i64 = L.add<int64_t>(2);
        const auto u8 = L.add<uint8_t>(7);
        const auto d2 = L.add<double>(1);
        check_regions({{d.offset, 24}, {i32.offset, 20}, {i64.offset, 16},
                       {u8.offset, 7}, {d2.offset, 8}},
                      L.bytes());
        CHECK(d.offset == 0);
        CHECK(L.bytes() == 24 + 24 + 16 + 8 + 8);
        char base[80];
        CHECK(reinterpret_cast<char*>(i32.in(base)) == base + i32.offset);
        CHECK(reinterpret_cast<char*>(u8.in(base)) == base + u8.offset);
    }
    for (size_t n : {1, 3, 257}) {
        odd_count_then_double<int32_t>(n);
        odd_count_then_double<uint8_t>(n);
    }
    {  // zero-length slots: legal, take no room, share the next offset
        WsLayout L;
        const auto z0 = L.add<double>(0);
        const auto a = L.add<int32_t>(3);
        const auto z1 = L.add<uint8_t>(0);
        const auto b = L.add<double>(2);
        const auto z2 = L.add<int64_t>(0);
        CHECK(z0.offset == 0 && a.offset == 0);
        CHECK(z1.offset == 16 && b.offset == 16);
        CHECK(z2.offset == 32 && L.bytes() == 32);
        check_regions({{z0.offset, 0}, {a.offset, 12}, {z1.offset, 0},
                       {b.offset, 16}, {z2.offset, 0}},
                      L.bytes());
        WsLayout empty;
        CHECK(empty.bytes() == 0);
        CHECK(empty.add<double>(0).offset == 0 && empty.bytes() == 0);
    }
    {  // all-double layouts are densely packed
        WsLayout L;
        const size_t ns[] = {1, 0, 7, 257, 2, 1000003};
        size_t sum = 0;
        for (size_t n : ns) {
            CHECK(L.add<double>(n).offset == 8 * sum);
            sum += n;
        }
        CHECK(L.bytes() == 8 * sum);
    }
    {  // one slot list addresses two bases
        WsLayout L;
        const auto a = L.add<double>(2);
        const auto b = L.add<int32_t>(3);
        std::vector<char> host(L.bytes()), dev(L.bytes());
        b.in(host.data())[2] = 42;
        std::memcpy(dev.data(), host.data(), L.bytes());
        CHECK(b.in(dev.data())[2] == 42);
        CHECK(reinterpret_cast<char*>(b.in(dev.data())) - dev.data() ==
              reinterpret_cast<char*>(b.in(host.data())) - host.data());
        (void)a;
    }
    {  // overflow throws and leaves the layout unchanged
        auto throws = [](auto add) {
            try {
                add();
            } catch (const std::overflow_error&) {
                return true;
            }
            return false;
        };
        WsLayout L;
        L.add<double>(4);
        CHECK(throws([&] { L.add<double>(SIZE_MAX / 8 + 1); }));   // n * 8 wraps
        CHECK(throws([&] { L.add<double>(SIZE_MAX / 8); }));       // padding/sum wraps
        CHECK(throws([&] { L.add<uint8_t>(SIZE_MAX - 8); }));      // + bytes() wraps
        CHECK(throws([&] { L.add<uint8_t>(SIZE_MAX - 38); }));     // rounding wraps
        CHECK(throws([&] { L.add<int32_t>((size_t)1 << 62); }));
        CHECK(L.bytes() == 32);
        CHECK(!throws([&] { L.add<uint8_t>(SIZE_MAX - 39); }));    // largest that fits
        CHECK(L.bytes() == SIZE_MAX - 7);
        CHECK(!throws([&] { L.add<double>(0); }));
        CHECK(throws([&] { L.add<uint8_t>(1); }));
    }
    if (g_failed == 0) std::printf("ws_layout: all checks passed\n");
    return g_failed == 0 ? 0 : 1;
}
