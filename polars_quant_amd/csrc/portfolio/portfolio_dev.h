// portfolio/portfolio_dev.h -- what the two portfolio engines share: portfolio.hip (D-27, groups of labels with weights normalised inside a
// group) and weights.hip (D-35, given signed weights with a cash remainder).  The usable test, the held price, the argument block with the
// `days` / `seg` tables, the host's day check and table, and the chain over the rebalance days.
#pragma once
#include <vector>

#include "../xsec/xsec_dev.h"

namespace {

// a price that can be held, a weight that counts: non-null, finite and > 0
__device__ __forceinline__ bool pf_usable(double v) { return xs_valid(v) && v > 0.0; }

struct PfArgs {
    const uint8_t *labels;  // [n][stride]
    const double *price;    // [n][stride]
    const double *weight;   // [n][stride] or null: equal weights
    const int32_t *days;    // [R], ascending
    const int32_t *seg;     // [len]: the rebalance index whose holdings day t values (d_k < t <= d_{k+1}), -1 up to d_0
    const double *A;        // [ng][R]: sum of the members' weights
    const double *G;        // [ng][len]: growth of the group since the rebalance that owns the day
    const int32_t *count;   // [ng][R]
    Dims d;
    int64_t R;
    int lag, ng;
};

// h(s, t): the price on the latest day in [dk, t] on which it is usable (price[s][dk] is, for a member); p = price[s][t]
__device__ __forceinline__ double pf_held(const double *row, double p, int64_t t, int64_t dk) {
    while (!pf_usable(p) && t > dk) p = row[--t];
    return p;
}

// the chain, one 64-lane workgroup per group: P_0 = capital, P_k = B_{k-1} G(g, d_k), B_k = P_k (1 - cost_rate tau_k).  The lanes stage
// PF_CHAIN steps at a time in LDS -- G(g, d_k) and 1 - cost_rate tau_k, which do not depend on the chain --, lane 0 walks them (two
// dependent multiplications a step, no global load in between) and leaves B_k in the place of G, and the lanes store the B_k
constexpr int PF_CHAIN = 1024;
__global__ __launch_bounds__(64) void pf_chain_kernel(PfArgs q, const double *tau, double cost_rate, double capital, double *Bout) {
    __shared__ double grow[PF_CHAIN], keep[PF_CHAIN];
    const int64_t g = blockIdx.x;
    double B = capital;
    for (int64_t k0 = 0; k0 < q.R; k0 += PF_CHAIN) {
        const int m = (int)(q.R - k0 < PF_CHAIN ? q.R - k0 : PF_CHAIN);
        for (int i = threadIdx.x; i < m; i += 64) {
            grow[i] = q.G[g * q.d.len + q.days[k0 + i]];
            keep[i] = 1.0 - cost_rate * tau[g * q.R + k0 + i];
        }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int i = 0; i < m; i++) {
                const double P = k0 + i == 0 ? capital : B * grow[i];
                B = P * keep[i];
                grow[i] = B;
            }
        __syncthreads();
        for (int i = threadIdx.x; i < m; i += 64) Bout[g * q.R + k0 + i] = grow[i];
        __syncthreads();
    }
}

inline dim3 pf_grid(int64_t threads, int64_t y = 1) { return dim3((unsigned)((threads + 63) / 64), (unsigned)y); }

// the rebalance days of a call: strictly ascending, each in [first, len); the message names the entry `what` and the lower bound `lo_name`
inline pq_status pf_check_days(const char *what, const int32_t *rebalance_days, int64_t R, int64_t first, const char *lo_name, int64_t len) {
    for (int64_t k = 0; k < R; k++) {
        const int64_t dk = rebalance_days[k];
        if (dk < first || dk >= len) {
            pq_set_error("%s: rebalance day %lld (entry %lld) is outside [%s, len) = [%d, %lld)", what, (long long)dk, (long long)k, lo_name,
                         (int)first, (long long)len);
            return PQ_ERR_ARG;
        }
        if (k > 0 && dk <= rebalance_days[k - 1]) {
            pq_set_error("%s: the rebalance days must be strictly ascending (entry %lld)", what, (long long)k);
            return PQ_ERR_ARG;
        }
    }
    return PQ_OK;
}

// the day table and, behind it, the segment table: seg[t] = k for d_k < t <= d_{k+1} (the last segment runs to len - 1), -1 up to d_0
inline std::vector<int32_t> pf_day_tables(const int32_t *rebalance_days, int64_t R, int64_t len) {
    std::vector<int32_t> host((size_t)(R + len));
    for (int64_t k = 0; k < R; k++) host[(size_t)k] = rebalance_days[k];
    for (int64_t t = 0, k = -1; t < len; t++) {
        host[(size_t)(R + t)] = (int32_t)k;
        if (k + 1 < R && t == rebalance_days[k + 1]) k++; // day d_{k+1} itself still belongs to segment k
    }
    return host;
}

} // namespace
