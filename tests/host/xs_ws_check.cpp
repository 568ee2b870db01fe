// tests/host/xs_ws_check.cpp -- the workspace carver of csrc/xsec/xsec_ws.h on the host, built with -fsanitize=address,undefined by
// tests/test_xsec_ws.py: a measuring run, then a binding run over a malloc of exactly the measured size, for mixes of element types
// and counts; every byte of every span is written, so a span that left the block would be an AddressSanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "xsec_ws.h"

static int failures = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            failures++;                                    \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                      \
            std::printf("\n");                             \
        }                                                  \
    } while (0)

struct Span { unsigned char *p; size_t bytes, off_before, off_after; };

enum Type { F64, I32, U16, U8 };
static const size_t SIZE_OF[] = {8, 4, 2, 1};

// takes (type, count) pairs in order; records each span
static std::vector<Span> carve(XsWs &w, const std::vector<std::pair<Type, size_t>> &plan) {
    std::vector<Span> out;
    for (const auto &[type, count] : plan) {
        Span s{nullptr, count * SIZE_OF[type], w.off, 0};
        double *f64;
        int32_t *i32;
        uint16_t *u16;
        switch (type) {
        case F64: w.take(f64, count); s.p = (unsigned char *)f64; break;
        case I32: w.take(i32, count); s.p = (unsigned char *)i32; break;
        case U16: w.take(u16, count); s.p = (unsigned char *)u16; break;
        case U8: w.take(s.p, count); break;
        }
        s.off_after = w.off;
        out.push_back(s);
    }
    return out;
}

static void check_plan(const std::vector<std::pair<Type, size_t>> &plan) {
    XsWs measure{nullptr};
    const std::vector<Span> m = carve(measure, plan);
    CHECK(!measure.bad, "a plan that fits was refused");
    for (const Span &s : m) CHECK(s.p == nullptr, "a measuring run handed out a pointer");
    const size_t total = measure.off;
    unsigned char *block = (unsigned char *)std::malloc(total ? total : 1);
    XsWs bind{block};
    const std::vector<Span> b = carve(bind, plan);
    CHECK(!bind.bad && bind.off == total, "the binding run took %zu bytes, the measuring run %zu", bind.off, total);
    size_t end = 0;   // the end of the last non-empty span so far: spans in taking order, pairwise disjoint
    for (size_t i = 0; i < b.size(); i++) {
        const Span &s = b[i];
        CHECK(s.off_before == m[i].off_before && s.off_after == m[i].off_after, "span %zu: the two runs disagree", i);
        const size_t off = (size_t)(s.p - block);
        CHECK(off == s.off_before, "span %zu does not start at the running offset", i);
        if (s.bytes == 0) {
            CHECK(s.off_after == s.off_before, "span %zu: a zero count moved the offset", i);
            continue;
        }
        CHECK(off % 256 == 0, "span %zu starts at %zu, not on a 256-byte boundary", i, off);
        CHECK(off >= end, "span %zu overlaps the span before it", i);
        CHECK(off + s.bytes <= total, "span %zu ends at %zu, beyond the block of %zu", i, off + s.bytes, total);
        CHECK(s.off_after >= off + s.bytes && s.off_after - (off + s.bytes) < 256, "span %zu: the offset after it is %zu", i, s.off_after);
        std::memset(s.p, (int)(i + 1), s.bytes);   // inside the malloc, or AddressSanitizer reports
        end = off + s.bytes;
    }
    CHECK(total == (end + 255) / 256 * 256, "the measured size %zu is not the aligned end %zu of the last span", total, end);
    for (size_t i = 0; i < b.size(); i++)   // disjoint: every span still holds its own fill
        for (size_t k = 0; k < b[i].bytes; k += (b[i].bytes > 4096 ? 257 : 1))
            if (b[i].p[k] != (unsigned char)(i + 1)) { CHECK(false, "span %zu was overwritten at byte %zu", i, k); break; }
    std::free(block);
}

int main() {
    const size_t counts[] = {0, 1, 31, 32, 33, (size_t)1 << 20};
    const Type types[] = {F64, I32, U16, U8};
    // every (type, count) alone, then every ordered pair of them, then one plan with all of them in a scrambled order
    std::vector<std::pair<Type, size_t>> all;
    for (Type t : types)
        for (size_t c : counts) all.push_back({t, c});
    for (const auto &a : all) check_plan({a});
    for (const auto &a : all)
        for (const auto &b : all)
            if (a.second + b.second <= ((size_t)1 << 20) + 33) check_plan({a, b});
    std::vector<std::pair<Type, size_t>> mixed;
    for (size_t i = 0; i < all.size(); i++) mixed.push_back(all[(i * 7 + 3) % all.size()]);
    check_plan(mixed);
    check_plan({});

    // rows: `rows` spans of one count, pitch<T>(count) elements apart; 0 rows take nothing
    {
        XsWs w{nullptr};
        double *f64;
        int32_t *i32;
        w.take(f64, 33, 3);
        CHECK(w.off == 3 * 512 && XsWs::pitch<double>(33) == 64, "3 rows of 33 doubles took %zu bytes", w.off);
        w.take(i32, 5, 0);
        CHECK(w.off == 3 * 512 && !w.bad, "0 rows moved the offset");
        w.take(f64, 1).take(i32, 1).take(f64, 0).take(i32, 65);   // chained takes are takes in order
        CHECK(w.off == 3 * 512 + 256 + 256 + 512, "chained takes took %zu bytes", w.off);
    }
    // a count whose byte size wraps size_t is refused: nothing is taken, the carver is marked, and later spans do not clear the mark
    {
        unsigned char block[512], *u8;
        double *f64 = nullptr;
        int32_t *i32;
        XsWs w{block};
        w.take(u8, 100);
        const size_t before = w.off;
        w.take(f64, SIZE_MAX / 8 + 2);
        CHECK(f64 == nullptr && w.bad && w.off == before, "a wrapping f64 count was not refused");
        w.take(i32, 4);
        CHECK(w.bad && (unsigned char *)i32 == block + 256, "a later span cleared the refusal, or did not follow the last good one");
        XsWs u{nullptr};
        u.take(u8, SIZE_MAX - 100);                      // the bytes fit, their 256-byte round-up does not
        CHECK(u.bad && u.off == 0, "a count whose round-up wraps was not refused");
        XsWs v{nullptr};
        v.take(f64, (size_t)1 << 40, (size_t)1 << 40);   // rows * row bytes wraps
        CHECK(v.bad && v.off == 0, "rows whose total wraps were not refused");
        XsWs s{nullptr};
        s.take(f64, (size_t)1 << 40).take(u8, SIZE_MAX - ((size_t)1 << 43) - 10);   // fits alone, not behind the first span
        CHECK(s.bad && s.off == ((size_t)1 << 43), "a span that wraps the running offset was not refused");
    }
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("xs_ws_check OK\n");
    return 0;
}
