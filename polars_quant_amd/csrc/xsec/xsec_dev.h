// xsec/xsec_dev.h -- device helpers shared by the cross-sectional kernels (sorts.hip: D-15, clean.hip: D-16, regress.hip: D-17): the
// summation block, the LDS bitonic sort of one day's keys, the segment offsets of rocPRIM's segmented sort, the sequential summaries.
#pragma once
#include "../pq_dev.h"

namespace {

constexpr int XS_BLOCK = 256;      // D-12 / D-15 summation block (symbols)
constexpr int XS_LDS_MAX = 16384;  // widest cross-section sorted in LDS: 16 384 f64 keys = 128 KiB of the CU's 160 KiB
constexpr int XS_CHUNK = 2048;     // days staged in LDS per step of the sequential summaries

__device__ __forceinline__ double xs_inf() { return __longlong_as_double(0x7FF0000000000000LL); }
__device__ __forceinline__ bool xs_valid(double v) { return !pq_isnull(v) && isfinite(v); }

// LDS rows carry one pad slot per 16 keys, so that the 16-key chunks of consecutive lanes start on different banks
__device__ __forceinline__ int xs_phys(int i) { return i + (i >> 4); }

// All-ascending bitonic network over S[0 .. P) (P = 2^p >= 16): the first stage of the merge of size k pairs i with its mirror
// i ^ (k-1), the later stages are half-cleaners i, i + j.  S[n .. P) holds +inf and keeps it (the larger key always goes to the
// larger index), so a pair or a 16-key chunk that only touches indices >= n changes nothing and is skipped.  Every stage whose pairs
// lie inside one aligned 16-key chunk runs in registers -- merges of 2 .. 16 keys entirely, and the last four stages (j = 8 .. 1) of
// every larger merge -- so a workgroup barrier is paid for each stage with j >= 16 and once per merge for the register pass: 65
// barriers instead of 105 at P = 16 384.
__device__ __forceinline__ void xs_cx(double &a, double &b) { // a <= b afterwards (keys are never NaN)
    const bool sw = b < a;
    const double lo = sw ? b : a, hi = sw ? a : b;
    a = lo; b = hi;
}
template <bool FULL> __device__ __forceinline__ void xs_chunk(double *S, int c) {
    double r[16];
#pragma unroll
    for (int m = 0; m < 16; m++) r[m] = S[xs_phys(c * 16 + m)];
    if (FULL) {
#pragma unroll
        for (int k = 2; k <= 16; k <<= 1) {
#pragma unroll
            for (int m = 0; m < 16; m++)
                if (!(m & (k >> 1))) xs_cx(r[m], r[m ^ (k - 1)]);
#pragma unroll
            for (int j = k >> 2; j > 0; j >>= 1)
#pragma unroll
                for (int m = 0; m < 16; m++)
                    if (!(m & j)) xs_cx(r[m], r[m | j]);
        }
    } else {
#pragma unroll
        for (int j = 8; j > 0; j >>= 1)
#pragma unroll
            for (int m = 0; m < 16; m++)
                if (!(m & j)) xs_cx(r[m], r[m | j]);
    }
#pragma unroll
    for (int m = 0; m < 16; m++) S[xs_phys(c * 16 + m)] = r[m];
}
__device__ __forceinline__ void xs_sort_lds(double *S, int P, int n, int tid, int nthr) {
    const int nchunk = P >> 4;
    for (int c = tid; c < nchunk && c * 16 < n; c += nthr) xs_chunk<true>(S, c);
    __syncthreads();
    for (int k = 32; k <= P; k <<= 1) {
        for (int j = k >> 1; j >= 16; j >>= 1) {
            const bool mirror = j == (k >> 1);
            for (int q = tid; q < (P >> 1); q += nthr) {
                const int i = ((q & ~(j - 1)) << 1) | (q & (j - 1)); // grows with q
                if (i >= n) break;
                const int p = mirror ? (i ^ (k - 1)) : (i + j);
                if (p < n) {
                    const int pi = xs_phys(i), pp = xs_phys(p);
                    const double a = S[pi], b = S[pp];
                    if (b < a) { S[pi] = b; S[pp] = a; }
                }
            }
            __syncthreads();
        }
        for (int c = tid; c < nchunk && c * 16 < n; c += nthr) xs_chunk<false>(S, c);
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void xs_offsets_kernel(unsigned *off, int64_t segs, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i <= segs) off[i] = (unsigned)(i * n);
}

// Sequential statistics of a series x[0 .. len) over its non-NaN entries, in ascending order from 0.0.  SQ = false: count, sum and
// count of entries > 0; SQ = true: sum of (x - center)^2.  The 64 lanes stage XS_CHUNK terms at a time in LDS -- the entry (or its
// square deviation), +0.0 for a NaN entry -- and count in parallel (integers: any order); lane 0 adds the staged terms in order.
// A +0.0 term leaves the sum unchanged: it starts at +0.0, and a round-to-nearest sum that starts there is never -0.0.  Sum and
// counts are returned in every lane.
template <bool SQ>
__device__ void xs_seq(const double *x, int64_t len, double center, double *buf, double &acc, int64_t &n, int64_t &pos) {
    acc = 0.0;
    long long cn = 0, cp = 0;
    for (int64_t c0 = 0; c0 < len; c0 += XS_CHUNK) {
        const int64_t m = len - c0 < XS_CHUNK ? len - c0 : XS_CHUNK, m8 = (m + 7) & ~7LL;
        for (int64_t i0 = threadIdx.x; i0 < m8; i0 += 64 * 8) { // eight global loads in flight per lane
            double v[8];
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int64_t i = i0 + k * 64;
                v[k] = i < m ? x[c0 + i] : __longlong_as_double(0x7FF8000000000000LL);
            }
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const bool ok = v[k] == v[k];
                cn += ok;
                if (!SQ) cp += v[k] > 0.0;
                const double dv = v[k] - center;
                if (i0 + k * 64 < m8) buf[i0 + k * 64] = ok ? (SQ ? dv * dv : v[k]) : 0.0;
            }
        }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int64_t i = 0; i < m8; i += 8) {
                double v[8];
#pragma unroll
                for (int k = 0; k < 8; k++) v[k] = buf[i + k];
#pragma unroll
                for (int k = 0; k < 8; k++) acc += v[k];
            }
        __syncthreads();
    }
    for (int o = 32; o > 0; o >>= 1) { cn += __shfl_xor(cn, o, 64); cp += __shfl_xor(cp, o, 64); }
    n = cn; pos = cp;
    acc = __shfl(acc, 0, 64); // the next pass centres on the mean in every lane
}

inline size_t xs_al(size_t x) { return (x + 255) / 256 * 256; }

} // namespace
