// Buffer layouts: a call site names each region once and gets the total size
// and every typed pointer from that one list, so the two cannot disagree.
//
// A slot is a typed byte offset, not a pointer: the same slots address any
// base the layout is carved from (the device workspace and, for a packed
// upload, the pinned host slice that mirrors it). Every slot starts on an
// 8-byte boundary and its padding belongs to it, so an all-double layout is
// densely packed and a zero-length slot is legal (it shares its offset with
// the next one). Plain C++17: no HIP, no pybind.
#pragma once

#include <cstddef>
#include <cstdint>
#include <stdexcept>

template <typename T>
struct WsSlot {
    size_t offset = 0;  // bytes from the base, a multiple of 8
    T* in(void* base) const {
        return reinterpret_cast<T*>(static_cast<char*>(base) + offset);
    }
};

class WsLayout {
  public:
    template <typename T>
    WsSlot<T> add(size_t n) {
        // bytes_ is a multiple of 8, so SIZE_MAX - 7 - bytes_ cannot wrap.
        if (n > (SIZE_MAX - 7 - bytes_) / sizeof(T))
            throw std::overflow_error("WsLayout: size overflow");
        const WsSlot<T> slot{bytes_};
        bytes_ += (n * sizeof(T) + 7) & ~size_t(7);
        return slot;
    }
    size_t bytes() const { return bytes_; }

  private:
    size_t bytes_ = 0;
};
