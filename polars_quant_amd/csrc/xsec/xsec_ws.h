// xsec/xsec_ws.h -- the workspace carver of the cross-sectional entry points.  A call describes its scratch memory once, as spans taken in
// order, each a typed pointer and a count; on a null base the description measures the bytes to reserve, on the reserved block it binds the
// pointers (xs_ws_carve, xsec_dev.h).  Every span starts on a 256-byte boundary and they follow each other in the order taken; a count of 0 (or
// 0 rows) takes no room; bytes that would wrap size_t take nothing and mark the carver `bad`.  No HIP header (tests/host/xs_ws_check.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

inline size_t xs_al(size_t x) { return (x + 255) / 256 * 256; }
struct XsWs {
    unsigned char *base;   // null: a measuring run, every span is null
    size_t off = 0;        // the next span's start = the bytes taken so far
    bool bad = false;
    template <class T> static size_t pitch(size_t count) { return xs_al(count * sizeof(T)) / sizeof(T); }   // elements from row to row
    // p <- the start of `rows` rows of `count` T each, pitch<T>(count) elements apart; chains
    template <class T> XsWs &take(T *&p, size_t count, size_t rows = 1) {
        const size_t room = SIZE_MAX - 255 - off;   // what xs_al can still round up without wrapping
        const bool fits = count == 0 || rows == 0 || (count <= room / sizeof(T) && rows <= room / xs_al(count * sizeof(T)));
        p = base && fits ? (T *)(base + off) : nullptr;
        if (fits && count) off += rows * xs_al(count * sizeof(T));
        bad = bad || !fits;
        return *this;
    }
};
