// seq/sequential.hip -- SequentialBacktester (src/backtest/sequential.rs:48-171, :257-336; decision D-23): the
// reference's shared-cash portfolio engine replayed from order tapes.  The reference calls a Python callback once per period; the
// callback sees an OrderContext and the period index and nothing of the engine's state, so its orders can be recorded first and
// matched afterwards.  The data-parallel axis is the tape.
//
//  sq_tape_kernel: one wavefront per tape, up to four tapes per workgroup.  pos / entry / board of the tape live in LDS (24 bytes per
//                  asset).  Cash, the trade counters and the order being matched are wave-uniform: every lane computes the same fill.
//                  Orders are loaded 64 at a time, one per lane, with the following 64 already in flight, and walked by uniform lane
//                  reads; pos[a] and entry[a] are read by all lanes from one LDS address and written by lane 0, with a wavefront fence
//                  between.  The waves of a workgroup walk different tapes with different trip counts: there is NO workgroup barrier.
//                  After a period that touched the board lane k forms partial k of D-22's summation order from LDS and the wave folds
//                  them; an untouched period reuses the valuation.  equity and cash are kept one period per lane and stored 64 periods
//                  (512 contiguous bytes) at a time.  Lane 0 writes the summary from the stored row (bt_summary_from_row).
#include "../ops_backtest.h"

namespace {

constexpr int SQ_MAX_WAVES = 4;                                 // tapes per workgroup
constexpr int SQ_ASSET_BYTES = 24;                              // pos, entry, board
constexpr int SQ_MAX_ASSETS = PQ_SEQ_MAX_ASSETS;                // 147 456 B of the CU's 160 KiB for one wave
constexpr int SQ_LDS_PLAIN = 64 * 1024;                         // what a launch gets without raising the attribute
constexpr int64_t SQ_NO_CHUNK = -(1LL << 60);

struct SqArgs {
    const int64_t *off;                                         // [n_tapes][T + 1]
    const int32_t *asset;
    const double *qty, *price;
    int64_t n_orders;
    const double *bench;                                        // [T] or nullptr
    const pq_seq_params *prm_dev;                               // [n_tapes], or nullptr: prm for every tape
    pq_seq_params prm;
    double *equity, *cash, *position;
    int64_t *counts;
    double *summary;
    int64_t n_tapes, T;
    int32_t A;
};

// only the order of the wave's own LDS and global accesses matters: lane 0 writes what every lane reads next
__device__ __forceinline__ void sq_fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); }

// uniform lane reads (j is the same in every lane): the value lands in scalar registers, no LDS round trip
__device__ __forceinline__ int sq_rd(int v, int j) { return __builtin_amdgcn_readlane(v, j); }
__device__ __forceinline__ long long sq_rd(long long v, int j) {
    const int lo = __builtin_amdgcn_readlane((int)v, j), hi = __builtin_amdgcn_readlane((int)(v >> 32), j);
    return ((long long)hi << 32) | (long long)(unsigned)lo;
}
__device__ __forceinline__ double sq_rd(double v, int j) { return __longlong_as_double(sq_rd(__double_as_longlong(v), j)); }

// D-22's fold of the 64 partials (report.hip rp_fold)
__device__ __forceinline__ double sq_fold(double p) {
    for (int s = 32; s > 0; s >>= 1) p += __shfl_down(p, s, 64);
    return __shfl(p, 0, 64);
}

struct SqChunk { int a; double q, p; };                          // 64 orders, one per lane
__device__ __forceinline__ void sq_load(SqChunk &c, const SqArgs &g, int64_t base, int lane) {
    const int64_t i = base + lane;
    const bool ok = i >= 0 && i < g.n_orders;
    c.a = ok ? g.asset[i] : -1;
    c.q = ok ? g.qty[i] : 0.0;
    c.p = ok ? g.price[i] : 0.0;
}

__device__ __forceinline__ int64_t sq_clamp(int64_t v, int64_t hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__global__ __launch_bounds__(SQ_MAX_WAVES * 64) void sq_tape_kernel(SqArgs g) {
    extern __shared__ __align__(16) unsigned char sq_lds[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t tape = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
    if (tape >= g.n_tapes) return;                              // an idle tail wave: nobody waits for it
    const int A = g.A;
    const int64_t T = g.T;
    double *pos = reinterpret_cast<double *>(sq_lds) + (size_t)wave * 3 * A, *entry = pos + A, *board = entry + A;
    for (int a = lane; a < 3 * A; a += 64) pos[a] = 0.0;
    sq_fence();
    const pq_seq_params prm = g.prm_dev ? g.prm_dev[tape] : g.prm;
    const int64_t *off = g.off + tape * (T + 1);
    double *eq_row = g.equity + tape * T, *cash_row = g.cash ? g.cash + tape * T : nullptr;

    double cash = prm.initial_capital, V = 0.0, eq_buf = 0.0, cash_buf = 0.0;
    int64_t trades = 0, wins = 0;
    SqChunk cur{-1, 0.0, 0.0}, nxt{-1, 0.0, 0.0};
    int64_t cb = SQ_NO_CHUNK;                                   // cur holds orders [cb, cb + 64), nxt [cb + 64, cb + 128)
    long long o_lo = 0, o_hi = 0;                               // lane k: the clamped slice of period t0 + k
    for (int64_t t = 0; t < T; t++) {
        const int slot = (int)(t & 63);
        if (slot == 0) {                                        // the offsets of 64 periods, coalesced
            const int64_t k = t + lane < T ? t + lane : T - 1;
            o_lo = sq_clamp(off[k], g.n_orders);
            o_hi = sq_clamp(off[k + 1], g.n_orders);
        }
        const int64_t lo = sq_rd(o_lo, slot), hi = sq_rd(o_hi, slot);   // hi < lo: an empty period
        bool dirty = false;
        for (int64_t i = lo; i < hi; i++) {
            if (i < cb || i >= cb + 64) {                       // wave-uniform
                if (i >= cb + 64 && i < cb + 128) { cur = nxt; cb += 64; }
                else { cb = i; sq_load(cur, g, cb, lane); }
                sq_load(nxt, g, cb + 64, lane);
            }
            const int j = (int)(i - cb);
            const int a = sq_rd(cur.a, j);
            const double q = sq_rd(cur.q, j), p = sq_rd(cur.p, j);
            if (!(p > 0.0) || q != q || q == 0.0 || a < 0 || a >= A) continue;   // not an order (sequential.rs:185-204), or no such asset
            dirty = true;
            if (lane == 0) board[a] = p;                        // :298, filled or not
            if (q > 0.0) {                                      // :56-73, :129-135
                const double fp = p + prm.buy_slippage;
                const double cost = q * fp;
                const double com = fmax(cost * prm.buy_commission_rate, prm.minimum_commission_fee);
                const double due = cost + com;
                if (cash >= due) {
                    const double have = pos[a];
                    cash -= due;
                    if (lane == 0) { pos[a] = have + q; entry[a] = fp; }
                    trades += 1;
                }
            } else {                                            // :74-92, :136-156
                const double aq = fabs(q), have = pos[a];
                if (have >= aq) {
                    const double fp = p - prm.sell_slippage;
                    const double rev = aq * fp;
                    const double com = fmax(rev * prm.sell_commission_rate, prm.minimum_commission_fee);
                    const double net = rev - com;
                    cash += net;
                    double left = have + q;
                    if (net > aq * entry[a]) wins += 1;
                    if (left <= 1e-8) left = 0.0;               // the map entry is removed; entry[a] is rewritten before it is read again
                    if (lane == 0) pos[a] = left;
                }
            }
            sq_fence();
        }
        if (dirty) {                                            // calculate_equity (:161-171) in D-22's order
            double part = 0.0;
#pragma unroll 4
            for (int a = lane; a < A; a += 64) {
                const double h = pos[a], b = board[a];
                part += h > 0.0 ? h * b : 0.0;                  // selected, not multiplied: 0 * inf
            }
            V = sq_fold(part);
        }
        if (lane == slot) { eq_buf = cash + V; cash_buf = cash; }
        if (slot == 63 || t == T - 1) {                         // 64 periods, 512 contiguous bytes
            const int64_t t0 = t - slot;
            if (lane <= slot) {
                eq_row[t0 + lane] = eq_buf;
                if (cash_row) cash_row[t0 + lane] = cash_buf;
            }
        }
    }
    if (g.position)
        for (int a = lane; a < A; a += 64) g.position[tape * A + a] = pos[a];
    if (lane == 0) { g.counts[tape * 2] = trades; g.counts[tape * 2 + 1] = wins; }
    if (g.summary) {
        // lane 0 reads the row that all lanes stored: one wait for the wave's own stores, after the walk
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        if (lane == 0) bt_summary_from_row(eq_row, T, prm.initial_capital, trades, wins, g.bench, g.summary + tape * PQ_SUMMARY_COLS);
    }
}

} // namespace

extern "C" {

pq_status pq_backtest_sequential(pq_ctx *ctx, int64_t n_tapes, int64_t n_periods, int32_t n_assets, const int64_t *period_offsets,
                                 const int32_t *asset, const double *quantity, const double *price, int64_t n_orders,
                                 const double *benchmark, const pq_seq_params *params, int64_t n_params, double *equity, double *cash,
                                 double *position, int64_t *counts, double *summary) {
    PQ_REQUIRE(ctx, "pq_backtest_sequential: null context");
    PQ_REQUIRE(n_tapes >= 0 && n_periods >= 0 && n_assets >= 0 && n_orders >= 0, "pq_backtest_sequential: negative size");
    if (n_assets > SQ_MAX_ASSETS) {
        pq_set_error("pq_backtest_sequential: n_assets = %d exceeds %d (pos / entry / board of one tape must fit the LDS of a compute unit)",
                     (int)n_assets, SQ_MAX_ASSETS);
        return PQ_ERR_ARG;
    }
    PQ_REQUIRE(params && (n_params == 1 || n_params == n_tapes), "pq_backtest_sequential: params must hold 1 or n_tapes entries");
    PQ_REQUIRE(n_orders == 0 || (asset && quantity && price), "pq_backtest_sequential: null order array");
    if (ctx->rec) { pq_set_error("pq_backtest_sequential cannot be recorded into a suite"); return PQ_ERR_UNSUPPORTED; }
    if (n_tapes == 0 || n_periods == 0) return PQ_OK;
    PQ_REQUIRE(period_offsets && equity && counts, "pq_backtest_sequential: null pointer");
    const size_t per_wave = (size_t)n_assets * SQ_ASSET_BYTES;
    int waves = per_wave ? (int)(SQ_LDS_PLAIN / per_wave) : SQ_MAX_WAVES;
    waves = waves < 1 ? 1 : (waves > SQ_MAX_WAVES ? SQ_MAX_WAVES : waves);
    if ((int64_t)waves > n_tapes) waves = (int)n_tapes;
    const size_t lds = per_wave * (size_t)waves;
    const int64_t blocks = (n_tapes + waves - 1) / waves;
    PQ_REQUIRE(blocks <= 0x7FFFFFFFLL, "pq_backtest_sequential: too many tapes for one launch");
    PQ_HIP_TRY(hipSetDevice(ctx->device));
    SqArgs g{};
    g.off = period_offsets; g.asset = asset; g.qty = quantity; g.price = price; g.n_orders = n_orders; g.bench = benchmark;
    g.prm = params[0];
    if (n_params > 1) {                                         // the host array may go once this call returns
        PQ_TRY(pq_ws_reserve(ctx, (size_t)n_params * sizeof(pq_seq_params)));
        PQ_HIP_TRY(hipMemcpyAsync(ctx->ws, params, (size_t)n_params * sizeof(pq_seq_params), hipMemcpyHostToDevice, ctx->stream));
        PQ_HIP_TRY(hipStreamSynchronize(ctx->stream));
        g.prm_dev = (const pq_seq_params *)ctx->ws;
    }
    g.equity = equity; g.cash = cash; g.position = position; g.counts = counts; g.summary = summary;
    g.n_tapes = n_tapes; g.T = n_periods; g.A = n_assets;
    if (lds > (size_t)SQ_LDS_PLAIN)
        PQ_HIP_TRY(hipFuncSetAttribute((const void *)sq_tape_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(sq_tape_kernel, dim3((unsigned)blocks), dim3((unsigned)waves * 64), lds, ctx->stream, g);
    PQ_HIP_TRY(hipGetLastError());
    return PQ_OK;
}

} // extern "C"
