// sweep.hip -- ParameterSweep (decision D-25 in DESIGN.md): one launch backtests a grid of strategy parameter sets over every symbol.
// The parameter set is the parallel axis: one lane is one parameter set, one wavefront is one symbol x 64 consecutive parameter sets,
// the (up to four) wavefronts of a workgroup share the symbol.  A parameter set names a rule over candidate indicator columns ("lines"):
//   rule 0  cross(lines[a], lines[b])   (oracle/backtest.c:263-270)      rule 1  band(lines[a], k0, k1)   (oracle/backtest.c:271-278)
// and the lane runs the reference's scan (vectorized.rs:124-194) and summary (metrics.rs:7-152) on the signals without ever writing a
// signal, position, cash or equity value to memory.  The price and the benchmark return of a row are the same for the whole workgroup;
// only the two line values differ per lane, and they come from LDS: the symbol's rows of every line (plus the price row and the
// benchmark-return row) are staged in tiles of R rows, R sized from the number of lines, double buffered -- the loads of the next tile
// are issued into registers before the current tile is walked and stored to the other buffer after it, so they are in flight during
// the walk.  The LDS pitch of a line is R itself, which is odd: lanes of one 32-lane group that read different lines at the same row
// then read different 8-byte banks (address (a R + t) mod 32 is a permutation of a for odd R).
// calculate_summary sums left to right and needs the mean before the variance and the covariance: the lane walks its rows twice, running
// the same deterministic state machine both times (walk 1: sum of returns, peak, drawdown, trades, wins; walk 2: the squared deviations
// and the covariance in the same row order).  A one-pass sum of squares would cancel.  Only pow differs from the host.
#include "../pq_dev.h"
#include <vector>

namespace {
constexpr int SW_BLOCK = 256;                // up to four wavefronts share a symbol
constexpr int SW_PRE = 16;                   // tile elements a thread carries from global memory to LDS
constexpr int SW_TILE = SW_BLOCK * SW_PRE;   // doubles in one tile buffer: two buffers = 64 KB of LDS at the most
constexpr int SW_MAX_R = 51;                 // rows of a tile at the most: up to 18 lines one wavefront carries a whole tile (20 x 51 <= 64 x 16)
constexpr int SW_MIN_R = 7;

// rows of a tile for n_lines lines: every line, the price and the benchmark return get one row of R values; odd (the bank spread above)
int sw_row_tile(int n_lines) {
    if (n_lines < 1 || n_lines > PQ_SWEEP_MAX_LINES) return 0;
    int r = SW_TILE / (n_lines + 2);
    if (r > SW_MAX_R) r = SW_MAX_R;
    if (r % 2 == 0) r -= 1;
    return r >= SW_MIN_R ? r : 0;
}
// wavefronts of a workgroup: one per 64 parameter sets, and enough threads to carry a tile (SW_PRE elements each); a wavefront without
// a parameter set only helps with the staging
int sw_waves(int n_lines, int R, int64_t n_params) {
    const int64_t by_params = (n_params + 63) / 64;
    const int by_tile = ((n_lines + 2) * R + 64 * SW_PRE - 1) / (64 * SW_PRE);
    const int64_t w = by_params > by_tile ? by_params : by_tile;
    return (int)(w < SW_BLOCK / 64 ? w : SW_BLOCK / 64);
}

struct SwArgs {
    const double *price;          // [n_series][stride]
    const double *const *lines;   // device table of n_lines columns, each [n_series][stride]
    const pq_sweep_param *params; // device, [n_params]
    const double *bench;          // nullable; series s at bench + s * bench_stride
    double *summary;              // [n_series][n_params][8]
    pq_bt_params prm;
    int64_t len, stride, bench_stride, n_params;
    int32_t n_lines, R, pblocks;
    uint32_t magic; // (e * magic) >> 20 == e / R for e < SW_TILE
};

struct SwLane { // the scan's state (vectorized.rs:124-194) and the rule's row t - 1
    double pa, pb, pos, avail, entry_cost, prev_eq;
    int32_t trades, wins;
    __device__ void reset(double capital) {
        pa = pb = __longlong_as_double(0x7FF8000000000000LL); // row 0 never signals: a NaN compares false
        pos = 0.0; avail = capital; entry_cost = 0.0; prev_eq = capital; trades = 0; wins = 0;
    }
};
struct SwAcc { // calculate_summary's running values (metrics.rs:21-67, :86-116)
    double max_eq, max_dd, ret_sum, bsum; // walk 1
    double mean, bmean, vs, bv, cv;       // walk 2
};

// where element e of a tile lives in global memory: row e / R of the tile is a line, the price or the benchmark; column e % R
struct SwSrc {
    const double *p; // row t of that series at p[t]
    int c;           // the element's row offset inside the tile
    int kind;        // 0: a line or the price (copied), 1: the benchmark (turned into its daily return), -1: beyond the tile
};
template <bool BENCH>
__device__ __forceinline__ SwSrc sw_src(const SwArgs &g, int64_t s, int e) {
    SwSrc r{nullptr, 0, -1};
    const int rows = g.n_lines + (BENCH ? 2 : 1);
    if (e >= rows * g.R) return r;
    const int row = (int)(((uint32_t)e * g.magic) >> 20);
    r.c = e - row * g.R;
    if (row < g.n_lines) { r.p = g.lines[row] + s * g.stride; r.kind = 0; }
    else if (row == g.n_lines) { r.p = g.price + s * g.stride; r.kind = 0; }
    else { r.p = g.bench + s * g.bench_stride; r.kind = 1; }
    return r;
}

// global memory -> registers: rows [t0, t0 + R) of every staged column.  A thread holds at most one benchmark element (R < 64),
// whose predecessor row comes along in bprev (metrics.rs:91-98: the return of row 0 is taken against row 0 itself).
template <bool BENCH>
__device__ __forceinline__ void sw_fetch(const SwArgs &g, int64_t s, int64_t t0, double (&pre)[SW_PRE], double &bprev) {
#pragma unroll
    for (int k = 0; k < SW_PRE; k++) {
        const SwSrc src = sw_src<BENCH>(g, s, k * (int)blockDim.x + (int)threadIdx.x);
        const int64_t t = t0 + src.c;
        pre[k] = 0.0; // an element beyond the tile or the series is stored at the most, never walked
        if (src.kind < 0 || t >= g.len) continue;
        pre[k] = src.p[t];
        if (BENCH && src.kind == 1) bprev = src.p[t > 0 ? t - 1 : 0];
    }
}
// registers -> LDS (element e at tile[e]: the pitch of a row is R)
template <bool BENCH>
__device__ __forceinline__ void sw_store(const SwArgs &g, int64_t t0, const double (&pre)[SW_PRE], double bprev, double *tile) {
    const int rows = g.n_lines + (BENCH ? 2 : 1), bench0 = (g.n_lines + 1) * g.R, n = rows * g.R;
#pragma unroll
    for (int k = 0; k < SW_PRE; k++) {
        const int e = k * (int)blockDim.x + (int)threadIdx.x;
        if (e >= n) continue;
        double v = pre[k];
        if (BENCH && e >= bench0) v = (bprev > 0.0) ? (v - bprev) / bprev : 0.0;
        tile[e] = v;
    }
}

// n rows of one tile for one lane.  The rule is two comparisons on the lane's two line values (a NULL is a NaN: it compares false);
// a buy or a sell is rare, so the event arithmetic stays behind the branch.
template <int PASS, bool BENCH>
__device__ __forceinline__ void sw_walk(const double *tile, int n, int ia, int ib, int ipx, int ibr, bool band, double k0, double k1,
                                        const pq_bt_params &prm, SwLane &st, SwAcc &acc) {
    for (int c = 0; c < n; c++) {
        const double xa = tile[ia + c], xb = tile[ib + c], px = tile[ipx + c];
        const bool buy = band ? (st.pa < k0 && xa >= k0) : (st.pa <= st.pb && xa > xb);
        const bool sell = band ? (st.pa > k1 && xa <= k1) : (st.pa >= st.pb && xa < xb);
        st.pa = xa; st.pb = xb;
        const bool do_buy = buy && st.pos == 0.0, do_sell = sell && st.pos > 0.0;
        if (px > 0.0 && (do_buy || do_sell)) { // a NaN (or NULL) or non-positive price leaves the state untouched (:141-144)
            if (do_buy) {                      // :146-161
                const double exec = px + prm.buy_slippage;
                const double cur_eq = st.avail + st.pos * px;
                const double deploy = cur_eq * prm.position_size;
                const double qty = floor(deploy / exec);
                if (qty > 0.0) {
                    const double cost = qty * exec;
                    const double fee = fmax(cost * prm.buy_commission_rate, prm.min_commission);
                    st.pos += qty;
                    st.avail -= cost + fee;
                    st.entry_cost = st.pos * px;
                    if (PASS == 1) st.trades += 1;
                }
            } else {                           // :162-175
                const double exec = px - prm.sell_slippage;
                const double revenue = st.pos * exec;
                const double fee = fmax(revenue * prm.sell_commission_rate, prm.min_commission);
                const double net = revenue - fee;
                if (PASS == 1 && net > st.entry_cost) st.wins += 1;
                st.avail += net;
                st.pos = 0.0;
            }
        }
        const double eq = st.avail + st.pos * px; // :177, and :142 on an untouched row
        const double r = (st.prev_eq > 0.0) ? (eq - st.prev_eq) / st.prev_eq : 0.0;
        st.prev_eq = eq;
        if (PASS == 1) { // metrics.rs:26-49
            if (eq > acc.max_eq) acc.max_eq = eq;
            const double dd = (acc.max_eq > 0.0) ? (acc.max_eq - eq) / acc.max_eq : 0.0;
            if (dd > acc.max_dd) acc.max_dd = dd;
            acc.ret_sum += r;
            if (BENCH) acc.bsum += tile[ibr + c];
        } else {         // metrics.rs:63-67, :100-116
            const double d = r - acc.mean;
            acc.vs += d * d;
            if (BENCH) {
                const double db = tile[ibr + c] - acc.bmean;
                acc.bv += db * db;
                acc.cv += d * db;
            }
        }
    }
}

// one walk over all rows; `again`: the other walk follows, so the tile after the last one is tile 0
template <int PASS, bool BENCH>
__device__ __forceinline__ void sw_pass(const SwArgs &g, int64_t s, double *lds, int &cur, bool wave_live, bool again, int ia, int ib,
                                        bool band, double k0, double k1, SwLane &st, SwAcc &acc) {
    const int R = g.R, tile_elems = (g.n_lines + (BENCH ? 2 : 1)) * R;
    const int ipx = g.n_lines * R, ibr = (g.n_lines + 1) * R;
    for (int64_t t0 = 0; t0 < g.len; t0 += R) {
        const bool last = t0 + R >= g.len, more = !last || again;
        const int64_t tn = last ? 0 : t0 + R;
        double pre[SW_PRE], bprev = 0.0;
        if (more) sw_fetch<BENCH>(g, s, tn, pre, bprev); // in flight during the walk
        const int n = (int)(last ? g.len - t0 : R);
        if (wave_live) sw_walk<PASS, BENCH>(lds + cur * tile_elems, n, ia, ib, ipx, ibr, band, k0, k1, g.prm, st, acc);
        if (more) sw_store<BENCH>(g, tn, pre, bprev, lds + (cur ^ 1) * tile_elems);
        __syncthreads(); // the next tile is complete, and nobody reads this one any more
        cur ^= 1;
    }
}

template <bool BENCH>
__global__ __launch_bounds__(SW_BLOCK) void sweep_kernel(SwArgs g) {
    extern __shared__ double sw_lds[];
    const int tid = (int)threadIdx.x;
    const int64_t s = (int64_t)(blockIdx.x / (unsigned)g.pblocks);
    const int64_t p0 = (int64_t)(blockIdx.x % (unsigned)g.pblocks) * blockDim.x;
    const int64_t p = p0 + tid;
    const bool live = p < g.n_params;
    const bool wave_live = p0 + (tid & ~63) < g.n_params; // a wavefront without a parameter set only helps with the staging
    int ia = 0, ib = 0;
    bool band = false;
    double k0 = 0.0, k1 = 0.0;
    if (live) { // a and b were checked against n_lines on the host before the launch
        const pq_sweep_param q = g.params[p];
        band = q.rule == 1;
        ia = q.a * g.R;
        ib = band ? ia : q.b * g.R;
        k0 = q.k0; k1 = q.k1;
    }
    const double capital = g.prm.initial_capital;
    SwLane st;
    SwAcc acc{};
    st.reset(capital);
    acc.max_eq = capital;
    int cur = 0;
    {
        double pre[SW_PRE], bprev = 0.0;
        sw_fetch<BENCH>(g, s, 0, pre, bprev);
        sw_store<BENCH>(g, 0, pre, bprev, sw_lds);
        __syncthreads();
    }
    sw_pass<1, BENCH>(g, s, sw_lds, cur, wave_live, true, ia, ib, band, k0, k1, st, acc);
    const double T = (double)g.len;
    const double last_eq = st.prev_eq;
    const int32_t trades = st.trades, wins = st.wins;
    acc.mean = acc.ret_sum / T;  // metrics.rs:60
    acc.bmean = acc.bsum / T;
    st.reset(capital);
    sw_pass<2, BENCH>(g, s, sw_lds, cur, wave_live, false, ia, ib, band, k0, k1, st, acc);
    if (!live) return;
    const double DAYS = 252.0, RF = 0.03;
    const double total_return = (last_eq - capital) / capital;                                                  // :52
    const double ann = (total_return > -1.0) ? pow(1.0 + total_return, DAYS / T) - 1.0 : -1.0;                  // :54-58
    const double dof = fmax(T - 1.0, 1.0);                                                                      // :61
    const double vol = sqrt(acc.vs / dof) * sqrt(DAYS);                                                         // :69
    const double sharpe = (vol > 0.0) ? (ann - RF) / vol : 0.0;                                                 // :71-75
    const double win_rate = (trades > 0) ? (double)wins / (double)trades : 0.0;
    double alpha = 0.0, beta = 0.0;
    if (BENCH) {                                                                                                // :86-140
        const double *bm = g.bench + s * g.bench_stride;
        const double bvar = acc.bv / dof, cov = acc.cv / dof;
        if (bvar > 0.0) beta = cov / bvar;
        const double b0 = bm[0], b1 = bm[g.len - 1];
        const double btr = (b0 > 0.0) ? (b1 - b0) / b0 : 0.0;
        const double bann = (btr > -1.0) ? pow(1.0 + btr, DAYS / T) - 1.0 : -1.0;
        alpha = ann - (RF + beta * (bann - RF));
    }
    double *sm = g.summary + (s * g.n_params + p) * PQ_SUMMARY_COLS; // a wavefront's 64 rows are one contiguous 4 KB piece
    sm[0] = ann; sm[1] = acc.max_dd; sm[2] = alpha; sm[3] = beta; sm[4] = sharpe;
    sm[5] = fmax(total_return, 0.0); sm[6] = win_rate; sm[7] = (double)trades;                                  // :142-149
}
} // namespace

extern "C" {

int32_t pq_sweep_row_tile(int32_t n_lines) { return sw_row_tile(n_lines); }

pq_status pq_backtest_sweep(pq_ctx *ctx, const pq_batch *b, const double *price, const double *const *lines, int32_t n_lines,
                            const pq_sweep_param *params, int64_t n_params, const double *benchmark, int64_t bench_series_stride,
                            const pq_bt_params *bt, double *summary) {
    PQ_TRY(pq_check(ctx, b));
    if (ctx->rec) { pq_set_error("pq_backtest_sweep cannot be recorded into a suite"); return PQ_ERR_UNSUPPORTED; }
    PQ_NO_RAGGED(b, "pq_backtest_sweep");
    PQ_REQUIRE(n_params >= 0, "pq_backtest_sweep: negative n_params");
    const int R = sw_row_tile(n_lines);
    if (R == 0) { pq_set_error("pq_backtest_sweep: n_lines must be in [1, %d], not %d", PQ_SWEEP_MAX_LINES, (int)n_lines); return PQ_ERR_ARG; }
    PQ_REQUIRE(bt, "pq_backtest_sweep: null parameters");
    if (n_params == 0 || b->n_series == 0) return PQ_OK;
    PQ_REQUIRE(params && summary && (b->len == 0 || (price && lines)), "pq_backtest_sweep: null pointer");
    for (int j = 0; j < n_lines && b->len > 0; j++) PQ_REQUIRE(lines[j], "pq_backtest_sweep: null line pointer");
    PQ_REQUIRE(!benchmark || bench_series_stride == 0 || bench_series_stride >= b->len, "pq_backtest_sweep: bench_series_stride must be 0 or >= len");
    const int waves = sw_waves(n_lines, R, n_params);
    const int64_t pblocks = (n_params + 64 * waves - 1) / (64 * waves);
    PQ_REQUIRE(b->len <= 0x7fffffffLL && n_params <= 0x7fffffffLL && pblocks * b->n_series <= 0x7fffffffLL, "pq_backtest_sweep: batch or grid too large");
    // the table is checked on the host before anything is launched: the kernel indexes LDS with a and b
    std::vector<pq_sweep_param> host((size_t)n_params);
    PQ_HIP_TRY(hipMemcpyAsync(host.data(), params, sizeof(pq_sweep_param) * (size_t)n_params, hipMemcpyDeviceToHost, ctx->stream));
    PQ_HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (int64_t i = 0; i < n_params; i++) {
        const pq_sweep_param &q = host[(size_t)i];
        if (q.rule != 0 && q.rule != 1) { pq_set_error("pq_backtest_sweep: parameter set %lld: unknown rule %d (0 cross, 1 band)", (long long)i, (int)q.rule); return PQ_ERR_ARG; }
        if (q.a < 0 || q.a >= n_lines || (q.rule == 0 && (q.b < 0 || q.b >= n_lines))) {
            pq_set_error("pq_backtest_sweep: parameter set %lld: line a=%d b=%d outside [0, %d)", (long long)i, (int)q.a, (int)q.b, (int)n_lines);
            return PQ_ERR_ARG;
        }
    }
    if (b->len == 0) { // calculate_summary on no rows: all zeros (metrics.rs:17-19)
        PQ_HIP_TRY(hipMemsetAsync(summary, 0, sizeof(double) * PQ_SUMMARY_COLS * (size_t)b->n_series * (size_t)n_params, ctx->stream));
        return PQ_OK;
    }
    PQ_TRY(pq_ws_reserve(ctx, sizeof(double *) * (size_t)n_lines));
    PQ_HIP_TRY(hipMemcpyAsync(ctx->ws, lines, sizeof(double *) * (size_t)n_lines, hipMemcpyHostToDevice, ctx->stream));
    PQ_HIP_TRY(hipStreamSynchronize(ctx->stream)); // the caller's table may go away after the call
    SwArgs g{};
    g.price = price; g.lines = (const double *const *)ctx->ws; g.params = params; g.bench = benchmark; g.summary = summary; g.prm = *bt;
    g.len = b->len; g.stride = b->stride; g.bench_stride = bench_series_stride; g.n_params = n_params;
    g.n_lines = n_lines; g.R = R; g.pblocks = (int32_t)pblocks;
    g.magic = ((1u << 20) + (uint32_t)R - 1u) / (uint32_t)R;
    const size_t lds = sizeof(double) * 2 * (size_t)(n_lines + 2) * (size_t)R; // <= 2 * SW_TILE doubles = 64 KB
    const dim3 grid((unsigned)(pblocks * b->n_series));
    if (benchmark) hipLaunchKernelGGL(sweep_kernel<true>, grid, dim3(64 * waves), lds, ctx->stream, g);
    else hipLaunchKernelGGL(sweep_kernel<false>, grid, dim3(64 * waves), lds, ctx->stream, g);
    PQ_HIP_TRY(hipGetLastError());
    return PQ_OK;
}

} // extern "C"
