// Shared host plumbing of the _hipcore extension: error check, numpy array
// typedefs, the process-wide workspace and an owning device buffer.
#pragma once

#include <hip/hip_runtime.h>
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "ws_layout.h"

namespace py = pybind11;

#define HIP_CHECK(expr)                                                          \
    do {                                                                         \
        hipError_t _e = (expr);                                                  \
        if (_e != hipSuccess) {                                                  \
            throw std::runtime_error(std::string("HIP error: ") +                \
                                     hipGetErrorString(_e) + " at " __FILE__ ":" + \
                                     std::to_string(__LINE__));                  \
        }                                                                        \
    } while (0)

using arr_f64 = py::array_t<double, py::array::c_style | py::array::forcecast>;
using arr_i64 = py::array_t<int64_t, py::array::c_style | py::array::forcecast>;
using arr_i32 = py::array_t<int32_t, py::array::c_style | py::array::forcecast>;

// ---------------------------------------------------------------------------
// Host-side workspace: grown lazily, reused across calls (no per-suggest
// hipMalloc). One workspace per process; calls are serialized by the GIL.
// Every entry point lays its own WsLayout over it, so nothing in it survives
// from one native call to the next.
// ---------------------------------------------------------------------------

struct Workspace {
    char* buf = nullptr;
    size_t capacity = 0;  // bytes
    hipStream_t stream = nullptr;
    // Pinned host staging: pageable hipMemcpyAsync silently degrades to a slow
    // synchronous staged copy; all H2D goes through this buffer instead.
    char* pinned = nullptr;
    size_t pinned_capacity = 0;
    size_t pinned_cursor = 0;

    char* ensure_bytes(size_t n_bytes) {
        if (n_bytes > capacity) {
            if (buf) (void)hipFree(buf);
            buf = nullptr;
            capacity = 0;
            const size_t grown = n_bytes + n_bytes / 2;
            HIP_CHECK(hipMalloc(&buf, grown));
            capacity = grown;
        }
        return buf;
    }
    void ensure_pinned(size_t n_bytes) {
        if (n_bytes > pinned_capacity) {
            if (pinned) (void)hipHostFree(pinned);
            pinned_capacity = n_bytes + n_bytes / 2;
            HIP_CHECK(hipHostMalloc(&pinned, pinned_capacity));
        }
    }
    // Event guard: an upload batch that ends without a stream sync (append's
    // fast path) records this event; the next begin_uploads waits on it before
    // reusing the staging buffer.
    hipEvent_t uploads_done = nullptr;
    bool uploads_pending = false;

    void end_uploads_async(hipStream_t st) {
        if (!uploads_done)
            HIP_CHECK(hipEventCreateWithFlags(&uploads_done, hipEventDisableTiming));
        HIP_CHECK(hipEventRecord(uploads_done, st));
        uploads_pending = true;
    }
    void begin_uploads() {
        if (uploads_pending) {
            HIP_CHECK(hipEventSynchronize(uploads_done));
            uploads_pending = false;
        }
        pinned_cursor = 0;
    }
    // Reserve a fresh pinned slice (the caller fills it and issues the DMA).
    char* stage(size_t bytes, hipStream_t st) {
        size_t aligned = (bytes + 255) & ~size_t(255);
        if (pinned_cursor + aligned > pinned_capacity) {
            // Grow: must drain in-flight DMAs that read the old buffer first.
            HIP_CHECK(hipStreamSynchronize(st));
            ensure_pinned(pinned_cursor + aligned);
            pinned_cursor = 0;
        }
        char* slot = pinned + pinned_cursor;
        pinned_cursor += aligned;
        return slot;
    }
    // memcpy into a fresh pinned slice, then a true-async DMA on the stream.
    void h2d(void* dst, const void* src, size_t bytes, hipStream_t st) {
        if (bytes == 0) return;
        char* slot = stage(bytes, st);
        memcpy(slot, src, bytes);
        HIP_CHECK(hipMemcpyAsync(dst, slot, bytes, hipMemcpyHostToDevice, st));
    }
    hipStream_t get_stream() {
        if (!stream) HIP_CHECK(hipStreamCreate(&stream));
        return stream;
    }
};

static Workspace g_ws;

// Owning device allocation of `capacity` elements: move-only, freed with the
// object.
template <typename T>
struct DeviceBuffer {
    T* ptr = nullptr;
    size_t capacity = 0;

    DeviceBuffer() = default;
    DeviceBuffer(DeviceBuffer&& o) noexcept
        : ptr(std::exchange(o.ptr, nullptr)), capacity(std::exchange(o.capacity, 0)) {}
    DeviceBuffer& operator=(DeviceBuffer&& o) noexcept {
        std::swap(ptr, o.ptr);
        std::swap(capacity, o.capacity);
        return *this;
    }
    ~DeviceBuffer() {
        if (ptr) (void)hipFree(ptr);
    }

    // At least n elements; the contents are NOT kept. The old buffer is freed
    // first (hipFree waits for the launches that still read it).
    void reserve(size_t n) {
        if (n <= capacity) return;
        if (ptr) HIP_CHECK(hipFree(ptr));
        ptr = nullptr;
        capacity = 0;
        HIP_CHECK(hipMalloc(&ptr, n * sizeof(T)));
        capacity = n;
    }

    // Grow to new_capacity elements and keep the contents, seen as `rows` rows
    // that each fill an equal share of the buffer (the pitch, which grows with
    // it) and hold `width` live elements. rows == 1 is the flat case. The
    // stream is drained before the old buffer is freed.
    void grow_preserving(size_t new_capacity, size_t rows, size_t width,
                         hipStream_t st) {
        DeviceBuffer grown;
        grown.reserve(new_capacity);
        if (ptr && width > 0) {
            if (rows == 1)
                HIP_CHECK(hipMemcpyAsync(grown.ptr, ptr, width * sizeof(T),
                                         hipMemcpyDeviceToDevice, st));
            else
                HIP_CHECK(hipMemcpy2DAsync(grown.ptr, new_capacity / rows * sizeof(T),
                                           ptr, capacity / rows * sizeof(T),
                                           width * sizeof(T), rows,
                                           hipMemcpyDeviceToDevice, st));
            HIP_CHECK(hipStreamSynchronize(st));
        }
        *this = std::move(grown);  // the old allocation dies with `grown`
    }
};

static bool g_available_checked = false;
static bool g_available = false;

static bool device_available() {
    if (!g_available_checked) {
        int n = 0;
        g_available = (hipGetDeviceCount(&n) == hipSuccess) && n > 0;
        g_available_checked = true;
    }
    return g_available;
}

bool available() { return device_available(); }

int device_count() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
