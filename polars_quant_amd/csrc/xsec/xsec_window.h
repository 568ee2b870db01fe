// xsec/xsec_window.h -- the window walk of the kernels that evaluate a window along the days of every symbol: rolling.hip (D-21),
// rolling_regress.hip (D-28), tsops.hip (D-29) and combine.hip's weights (D-30: one "symbol" of K IC series).  All launch one workgroup of XW_TILE threads per (symbol, tile of XW_TILE days), walked
// with a grid stride.
//  stage:   a workgroup stages its tile and a halo of window - 1 earlier days in LDS, M = XW_TILE + window - 1 entries per column, loads
//           coalesced along days, and beside them last[l] = l where entry l is unusable, -1 where it is usable.
//  scan:    xw_last_scan turns last[] into "the last unusable entry at or before l" (a max-scan: every thread scans a short run, the
//           runs are joined by a wave scan), so "is the whole window of a row usable" is one compare: e - last[e] >= w at its entry e.
//  rows:    each thread evaluates its own row's window directly out of LDS: consecutive threads read consecutive 8-byte words at every
//           step (no bank conflict), and every sum starts at 0.0 and adds in ascending day order, which is the definition's order; a
//           sliding sum would not keep it.
//  walk:    xw_walk is the three steps above with their barriers, around a kernel's own load and row; xw_rows is the job loop and the
//           row guard alone, for the kernels that stage nothing.  xw_sum / xw_mean / xw_mean_q2 are the row sums that several ops share.
//  host:    xw_prepare is what every entry point does after its own argument checks, down to the launch shape; xw_no_overlap refuses
//           an output that overlaps an input or another output.
// What is staged, the LDS it is staged in, and what a row computes from its window stay in each kernel.
#pragma once
#include "xsec_dev.h"

namespace {

constexpr int XW_TILE = 256;                                    // days per workgroup = threads per workgroup
constexpr int XW_MAX_W = PQ_FACTOR_ROLLING_MAX_WINDOW;
constexpr int XW_STAGE = XW_TILE + XW_MAX_W - 1;                // staged entries at the widest window: 10 KiB of f64 + 5 KiB of i32

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

// The walk of a windowed kernel over its jobs, by all XW_TILE threads.  LDS is the kernel's: val holds NC columns of M entries (column c
// at val + c * M), last M ints, wave_last XW_TILE / 64.
//  load(s, g, v) -> bool    writes the NC values of day g of symbol s into v (any g, also outside [0, len)); is the entry usable?
//  row(s, t, win, M, usable)  the result(s) of row t of symbol s from win[c * M + k], k = 0 .. w-1 (oldest to newest), and their store(s);
//                             usable: the whole window is
template <int NC, class Load, class Row>
__device__ __forceinline__ void xw_walk(double *val, int *last, int *wave_last, const Dims &d, int w, int64_t chunks, int64_t total, Load load,
                                        Row row) {
    const int tid = threadIdx.x, M = XW_TILE + w - 1;
    for (int64_t job = blockIdx.x; job < total; job += gridDim.x) {
        const auto [s, t0, g0] = xw_job(job, chunks, w);
        for (int l = tid; l < M; l += XW_TILE) {
            double v[NC];
            const bool ok = load(s, g0 + l, v);
#pragma unroll
            for (int c = 0; c < NC; c++) val[c * M + l] = v[c];
            last[l] = ok ? -1 : l;
        }
        xw_last_scan(last, M, wave_last);
        const int64_t t = t0 + tid;
        if (t < d.len) {
            const int e = tid + w - 1;
            row(s, t, val + tid, M, e - last[e] >= w);
        }
        __syncthreads();                                        // the next tile restages val / last
    }
}

// f(s, t) for every row of the same jobs, nothing staged: no halo, no barrier
template <class F> __device__ __forceinline__ void xw_rows(const Dims &d, int64_t chunks, int64_t total, F f) {
    for (int64_t job = blockIdx.x; job < total; job += gridDim.x) {
        const XwJob j = xw_job(job, chunks, 1);
        const int64_t t = j.t0 + threadIdx.x;
        if (t < d.len) f(j.s, t);
    }
}

// the sums of one column of a window that several ops share; each starts at 0.0 and adds win[0 .. w) in ascending order
__device__ __forceinline__ double xw_sum(const double *win, int w) {
    double sum = 0.0;
    for (int k = 0; k < w; k++) sum += win[k];
    return sum;
}
__device__ __forceinline__ double xw_mean(const double *win, int w) { return xw_sum(win, w) / (double)w; }
struct XwMeanQ2 { double mean, q2; };                           // q2 = sum of (win[k] - mean)^2
__device__ __forceinline__ XwMeanQ2 xw_mean_q2(const double *win, int w) {
    const double mean = xw_mean(win, w);
    double q2 = 0.0;
    for (int k = 0; k < w; k++) {
        const double dv = win[k] - mean;
        q2 += dv * dv;
    }
    return XwMeanQ2{mean, q2};
}

// ---------------------------------------------------------------- host
struct XwGrid { Dims d; int64_t chunks, total; dim3 grid; };    // tiles per symbol, jobs, workgroups (at most 2^20: the kernels stride)

// What an entry point does after its own argument checks: it refuses a recording context and a ragged batch with the caller's texts
// (and the caller's status for the latter), then fills *g.  g->total == 0: an empty batch, nothing to launch.
inline pq_status xw_prepare(pq_ctx *ctx, const pq_batch *b, const char *recorded, const char *ragged, pq_status ragged_status, XwGrid *g) {
    if (ctx->rec) { pq_set_error("%s", recorded); return PQ_ERR_UNSUPPORTED; }
    if (b->offsets) { pq_set_error("%s", ragged); return ragged_status; }
    const Dims d = dims_of(b);
    const int64_t chunks = (d.len + XW_TILE - 1) / XW_TILE, total = chunks * d.n;
    *g = XwGrid{d, chunks, total, dim3((unsigned)(total < (int64_t)1 << 20 ? total : (int64_t)1 << 20))};
    return PQ_OK;
}

struct XwSpan { uintptr_t lo, hi; };
inline XwSpan xw_span(const void *p, uintptr_t bytes) { return XwSpan{(uintptr_t)p, (uintptr_t)p + bytes}; }
inline bool xw_disjoint(const XwSpan &a, const XwSpan &b) { return a.hi <= b.lo || b.hi <= a.lo; }
inline uintptr_t xw_plane_bytes(const Dims &d) { return (uintptr_t)d.n * (uintptr_t)d.stride * 8; }   // one [n_series][stride] column

// A workgroup reads a halo of days that another workgroup writes, so no output may overlap an input (else: the text vs_in) or an
// earlier output (vs_out)
inline pq_status xw_no_overlap(const XwSpan *outs, int n_out, const XwSpan *ins, int n_in, const char *vs_in, const char *vs_out) {
    for (int i = 0; i < n_out; i++) {
        for (int j = 0; j < n_in; j++) PQ_REQUIRE(xw_disjoint(outs[i], ins[j]), vs_in);
        for (int j = 0; j < i; j++) PQ_REQUIRE(xw_disjoint(outs[i], outs[j]), vs_out);
    }
    return PQ_OK;
}

} // namespace
