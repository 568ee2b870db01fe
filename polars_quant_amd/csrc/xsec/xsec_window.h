// xsec/xsec_window.h -- the window stage of the kernels that walk a window along the days of every symbol: rolling.hip (D-21) and
// rolling_regress.hip (D-28).  Both launch one workgroup of XW_TILE threads per (symbol, tile of XW_TILE days), walked with a grid
// stride; a workgroup stages its tile and a halo of window - 1 earlier days in LDS, M = XW_TILE + window - 1 entries, and beside them
// last[l] = l where entry l is unusable, -1 where it is usable.  From here:
//  * job:   xw_job splits a job index into the symbol, the tile's first day and the day of staged entry 0.
//  * scan:  xw_last_scan turns last[] into "the last unusable entry at or before l" (a max-scan: every thread scans a short run, the
//           runs are joined by a wave scan), so "is the whole window of a row usable" is one compare: e - last[e] >= w at its entry e.
//  * host:  xw_grid is the launch shape; XwSpan / xw_disjoint refuse an output that overlaps an input (a workgroup reads a halo of days
//           that another workgroup writes).
// What is staged, and what a row computes from its window, stay in each kernel.
#pragma once
#include "xsec_dev.h"

namespace {

constexpr int XW_TILE = 256;            // days per workgroup = threads per workgroup

// job = symbol s, tile of days [t0, t0 + XW_TILE); staged entry l is day g0 + l, row t0 + i is entry i + w - 1 and its window is entries
// [i, i + w)
struct XwJob { int64_t s, t0, g0; };
__device__ __forceinline__ XwJob xw_job(int64_t job, int64_t chunks, int w) {
    const int64_t s = job / chunks, t0 = (job - s * chunks) * XW_TILE;
    return XwJob{s, t0, t0 - (w - 1)};
}

// last[0 .. M) <- the running maximum of the staged marks, by all XW_TILE threads; wave_last is XW_TILE / 64 ints of LDS.  Begins with
// the barrier behind the staging loop and ends with the one in front of the rows.
__device__ __forceinline__ void xw_last_scan(int *last, int M, int *wave_last) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int C = (M + XW_TILE - 1) / XW_TILE, lo = tid * C < M ? tid * C : M, hi = lo + C < M ? lo + C : M;
    __syncthreads();
    int m = -1;                                                 // the marks grow with l, so the maximum is the last one
    for (int l = lo; l < hi; l++) m = last[l] > m ? last[l] : m;
    int inc = m;
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(inc, o, 64);
        if (lane >= o && u > inc) inc = u;
    }
    if (lane == 63) wave_last[wave] = inc;
    __syncthreads();
    int carry = __shfl_up(inc, 1, 64);
    if (lane == 0) carry = -1;
    for (int k = 0; k < wave; k++) carry = wave_last[k] > carry ? wave_last[k] : carry;
    for (int l = lo; l < hi; l++) {
        carry = last[l] > carry ? last[l] : carry;
        last[l] = carry;
    }
    __syncthreads();
}

// ---------------------------------------------------------------- host
struct XwGrid { int64_t chunks, total; dim3 grid; };   // tiles per symbol, jobs, workgroups (at most 2^20: the kernels stride)
inline XwGrid xw_grid(const Dims &d) {
    const int64_t chunks = (d.len + XW_TILE - 1) / XW_TILE, total = chunks * d.n;
    return XwGrid{chunks, total, dim3((unsigned)(total < (int64_t)1 << 20 ? total : (int64_t)1 << 20))};
}

struct XwSpan { uintptr_t lo, hi; };
inline XwSpan xw_span(const void *p, uintptr_t bytes) { return XwSpan{(uintptr_t)p, (uintptr_t)p + bytes}; }
inline bool xw_disjoint(const XwSpan &a, const XwSpan &b) { return a.hi <= b.lo || b.hi <= a.lo; }

} // namespace
