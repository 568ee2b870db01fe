// sweep.hip -- ParameterSweep (decision D-25 in DESIGN.md): one launch backtests a grid of strategy parameter sets over every symbol.
// The parameter set is the parallel axis: one lane is one parameter set, one wavefront is one symbol x 64 consecutive parameter sets,
// the (up to four) wavefronts of a workgroup share the symbol.  A parameter set names a rule over candidate indicator columns ("lines");
// col[c] is lines[c], or the price where c = -1:
//   rule 0  cross(lines[a], lines[b])   (oracle/backtest.c:263-270)      rule 1  band(lines[a], k0, k1)   (oracle/backtest.c:271-278)
//   rule 2  channel, reversion: col[c] against lo = lines[a], hi = lines[b]   (pq_channel_signals mode 0, oracle/backtest.c:279-294)
//   rule 3  channel, breakout: col[c] against row t - 1 of lo and hi          (pq_channel_signals mode 1)
//   rule 4  rule 2 with lo = lines[a] k0, hi = lines[a] k1                    (pq_scale_band + pq_channel_signals mode 0)
//   rule 5  cross(lines[a], lines[b]), buys while col[c] < k0, sells while col[c] > k1   (pq_cross_signals + pq_gate_signals mode 0)
//   rule 6  cross(lines[a], lines[b]), both while col[c] > k0                            (pq_cross_signals + pq_gate_signals mode 1)
// and the lane runs the reference's scan (vectorized.rs:124-194) and summary (metrics.rs:7-152) on the signals without ever writing a
// signal, position, cash or equity value to memory.  A table with one rule throughout runs the kernel instantiated for that rule, which
// keeps only the LDS reads and row t - 1 registers of that rule; a mixed table runs the generic instantiation (RULE = -1), whose lanes
// dispatch on their own rule.  The price and the benchmark return of a row are the same for the whole workgroup;
// only the (up to three) column values differ per lane, and they come from LDS: the symbol's rows of every line (plus the price row and the
// benchmark-return row) are staged in tiles of R rows, R sized from the number of lines, double buffered -- the loads of the next tile
// are issued into registers before the current tile is walked and stored to the other buffer after it, so they are in flight during
// the walk.  The LDS pitch of a line is R itself, which is odd: lanes of one 32-lane group that read different lines at the same row
// then read different 8-byte banks (address (a R + t) mod 32 is a permutation of a for odd R).
// calculate_summary sums left to right and needs the mean before the variance and the covariance: the lane walks its rows twice, running
// the same deterministic state machine both times (walk 1: sum of returns, peak, drawdown, trades, wins; walk 2: the squared deviations
// and the covariance in the same row order).  A one-pass sum of squares would cancel.  Only pow differs from the host.
#include "../pq_dev.h"
#include "../bt_core.h"
#include "../wave_util.h"
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
    const pq_sweep_rule *params;  // device, [n_params]
    const double *bench;          // nullable; series s at bench + s * bench_stride
    double *summary;              // [n_series][n_params][8]
    pq_bt_params prm;
    int64_t len, stride, bench_stride, n_params;
    int32_t n_lines, R, pblocks;
    uint32_t magic; // (e * magic) >> 20 == e / R for e < SW_TILE
};

static_assert(sizeof(pq_sweep_rule) == 32 && sizeof(pq_sweep_param) == 32, "one table layout for both entry points");
constexpr int SW_GENERIC = -1; // the instantiation whose lanes dispatch on their own rule
// what a rule reads besides lines[a] (SW_GENERIC: both): RULE is a template argument, so an instantiation carries only its own reads
// and registers
constexpr bool sw_uses_b(int rule) { return rule != PQ_SWEEP_RULE_BAND && rule != PQ_SWEEP_RULE_SCALED_CHANNEL; }
constexpr bool sw_uses_c(int rule) { return rule != PQ_SWEEP_RULE_CROSS && rule != PQ_SWEEP_RULE_BAND; }

struct SwRule { // a lane's parameter set: the LDS offsets of its columns (an unused one repeats ia)
    int ia, ib, ic, rule;
    double k0, k1;
};
struct SwLane { // the scan's state (vectorized.rs:124-194) and the rule's row t - 1
    double pa, pb, pc, prev_eq;
    BtPool pl;
    int32_t trades, wins;
    __device__ void reset(double capital) {
        pa = pb = pc = __longlong_as_double(0x7FF8000000000000LL); // row 0 never signals: a NaN (not the NULL) compares false
        pl.reset(capital); prev_eq = capital; trades = 0; wins = 0;
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

// global memory -> registers: rows [t0, t0 + R) of every staged column, of the rows [lo, hi) that the walk covers (the whole series, or
// one window of it).  A thread holds at most one benchmark element (R < 64), whose predecessor row comes along in bprev
// (metrics.rs:91-98: the return of the first row is taken against that row itself).
template <bool BENCH>
__device__ __forceinline__ void sw_fetch(const SwArgs &g, int64_t s, int64_t t0, int64_t lo, int64_t hi, double (&pre)[SW_PRE],
                                         double &bprev) {
#pragma unroll
    for (int k = 0; k < SW_PRE; k++) {
        const SwSrc src = sw_src<BENCH>(g, s, k * (int)blockDim.x + (int)threadIdx.x);
        const int64_t t = t0 + src.c;
        pre[k] = 0.0; // an element beyond the tile or the series is stored at the most, never walked
        if (src.kind < 0 || t >= hi) continue;
        pre[k] = src.p[t];
        if (BENCH && src.kind == 1) bprev = src.p[t > lo ? t - 1 : lo];
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

// the lane's rule on row t (xa, xb, xc) and row t - 1 (st.pa, st.pb, st.pc).  Cross, band and the gates are comparisons a NaN fails, and
// a NULL is a NaN.  A channel side is refused when the OTHER side's column is NULL but not when it is a non-NULL NaN (ChannelSigOp,
// ops_backtest.h), so rules 2-4 test for the NULL itself.
template <int RULE>
__device__ __forceinline__ void sw_signal(const SwRule &q, double xa, double xb, double xc, SwLane &st, bool &buy, bool &sell) {
    const int rule = RULE == SW_GENERIC ? q.rule : RULE;
    double na = xa, nb = xb; // what row t leaves behind as row t - 1
    switch (rule) {
    case PQ_SWEEP_RULE_BAND:
        buy = st.pa < q.k0 && xa >= q.k0;
        sell = st.pa > q.k1 && xa <= q.k1;
        break;
    case PQ_SWEEP_RULE_SCALED_CHANNEL: { // ScaleBandOp (strategy.hip): one rounded multiply each, NULL where the base is
        const bool null = pq_isnull(xa);
        na = null ? xa : xa * q.k0;
        nb = null ? xa : xa * q.k1;
    }
        [[fallthrough]]; // then the channel on lo = na, hi = nb
    case PQ_SWEEP_RULE_CHANNEL: {
        const bool ok = !pq_isnull(xc) && !pq_isnull(st.pc) && !pq_isnull(na) && !pq_isnull(nb) && !pq_isnull(st.pa) && !pq_isnull(st.pb);
        buy = ok && xc < na && st.pc >= st.pa;
        sell = ok && xc > nb && st.pc <= st.pb;
    } break;
    case PQ_SWEEP_RULE_BREAKOUT: {
        const bool ok = !pq_isnull(xc) && !pq_isnull(st.pa) && !pq_isnull(st.pb);
        buy = ok && xc > st.pb;
        sell = ok && xc < st.pa;
    } break;
    default: { // cross, alone or behind a gate on col[c] of row t
        buy = st.pa <= st.pb && xa > xb;
        sell = st.pa >= st.pb && xa < xb;
        if (rule == PQ_SWEEP_RULE_CROSS_ZONES) { buy = buy && xc < q.k0; sell = sell && xc > q.k1; }
        if (rule == PQ_SWEEP_RULE_CROSS_STRENGTH) { const bool gate = xc > q.k0; buy = buy && gate; sell = sell && gate; }
    } break;
    }
    st.pa = na; st.pb = nb; st.pc = xc;
}

// n rows of one tile for one lane.  A buy or a sell is rare, so the event arithmetic stays behind the branch.
template <int RULE, int PASS, bool BENCH>
__device__ __forceinline__ void sw_walk(const double *tile, int n, const SwRule &q, int ipx, int ibr, const pq_bt_params &prm, SwLane &st,
                                        SwAcc &acc) {
    for (int c = 0; c < n; c++) {
        const double xa = tile[q.ia + c], px = tile[ipx + c];
        const double xb = sw_uses_b(RULE) ? tile[q.ib + c] : xa;
        const double xc = sw_uses_c(RULE) ? tile[q.ic + c] : xa;
        bool buy, sell;
        sw_signal<RULE>(q, xa, xb, xc, st, buy, sell);
        const bool do_buy = buy && st.pl.pos == 0.0, do_sell = sell && st.pl.pos > 0.0;
        if (px > 0.0 && (do_buy || do_sell)) { // a NaN (or NULL) or non-positive price leaves the state untouched (:141-144)
            if (do_buy) {
                const bool opened = bt_buy(st.pl, px, prm);
                if (PASS == 1 && opened) st.trades += 1;
            } else {
                const bool win = bt_sell(st.pl, px, prm);
                if (PASS == 1 && win) st.wins += 1;
            }
        }
        const double eq = st.pl.equity(px);
        const double r = bt_ret(st.prev_eq, eq);
        st.prev_eq = eq;
        if (PASS == 1) { // metrics.rs:26-49 (BtRun::add, with prev_eq among the lane's registers of both walks)
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

// one walk over the rows [lo, hi); `again`: the other walk follows, so the tile after the last one is the first one
template <int RULE, int PASS, bool BENCH>
__device__ __forceinline__ void sw_pass(const SwArgs &g, int64_t s, int64_t lo, int64_t hi, double *lds, int &cur, bool wave_live, bool again,
                                        const SwRule &q, SwLane &st, SwAcc &acc) {
    const int R = g.R, tile_elems = (g.n_lines + (BENCH ? 2 : 1)) * R;
    const int ipx = g.n_lines * R, ibr = (g.n_lines + 1) * R;
    for (int64_t t0 = lo; t0 < hi; t0 += R) {
        const bool last = t0 + R >= hi, more = !last || again;
        const int64_t tn = last ? lo : t0 + R;
        double pre[SW_PRE], bprev = 0.0;
        if (more) sw_fetch<BENCH>(g, s, tn, lo, hi, pre, bprev); // in flight during the walk
        const int n = (int)(last ? hi - t0 : R);
        if (wave_live) sw_walk<RULE, PASS, BENCH>(lds + cur * tile_elems, n, q, ipx, ibr, g.prm, st, acc);
        if (more) sw_store<BENCH>(g, tn, pre, bprev, lds + (cur ^ 1) * tile_elems);
        __syncthreads(); // the next tile is complete, and nobody reads this one any more
        cur ^= 1;
    }
}

// a lane's parameter set p of the table (a lane beyond the table walks a cross of column 0 with itself and writes nothing)
template <int RULE>
__device__ __forceinline__ SwRule sw_rule(const SwArgs &g, int64_t p, bool live) {
    SwRule q{0, 0, 0, RULE == SW_GENERIC ? PQ_SWEEP_RULE_CROSS : RULE, 0.0, 0.0};
    if (live) { // the rule and the columns it uses were checked against n_lines on the host before the launch
        const pq_sweep_rule in = g.params[p];
        if (RULE == SW_GENERIC) q.rule = in.rule;
        q.ia = in.a * g.R;
        q.ib = (RULE == SW_GENERIC ? sw_uses_b(in.rule) : sw_uses_b(RULE)) ? in.b * g.R : q.ia;
        q.ic = (RULE == SW_GENERIC ? sw_uses_c(in.rule) : sw_uses_c(RULE)) ? (in.c < 0 ? g.n_lines : in.c) * g.R : q.ia; // -1: the price row
        q.k0 = in.k0; q.k1 = in.k1;
    }
    return q;
}
// the lane's eight values after both walks over the rows [lo, hi); a wavefront's 64 rows of `sm` are one contiguous 4 KB piece
template <bool BENCH>
__device__ __forceinline__ void sw_close(const SwArgs &g, int64_t s, int64_t lo, int64_t hi, double last_eq, int32_t trades, int32_t wins,
                                         const SwAcc &acc, double *sm) {
    const double *bm = g.bench + s * g.bench_stride;
    bt_summary_close((double)(hi - lo), g.prm.initial_capital, last_eq, acc.max_dd, acc.vs, acc.bv, acc.cv, trades, wins, BENCH,
                     BENCH ? bm[lo] : 0.0, BENCH ? bm[hi - 1] : 0.0, sm);
}

// RULE: the one rule of the whole table, or SW_GENERIC.  The lane set-up (sw_rule), the two walks (sw_pass) and the close (sw_close) are
// shared with sweep_windows_kernel below; the two bodies that string them together stay apart (see there), and the bit-for-bit tests of
// tests/test_sweep_windows_gpu.py compare the two.
template <int RULE, bool BENCH>
__global__ __launch_bounds__(SW_BLOCK) void sweep_kernel(SwArgs g) {
    extern __shared__ double sw_lds[];
    const int tid = (int)threadIdx.x;
    const int64_t s = (int64_t)(blockIdx.x / (unsigned)g.pblocks);
    const int64_t p0 = (int64_t)(blockIdx.x % (unsigned)g.pblocks) * blockDim.x;
    const int64_t p = p0 + tid;
    const bool live = p < g.n_params;
    const bool wave_live = p0 + (tid & ~63) < g.n_params; // a wavefront without a parameter set only helps with the staging
    const SwRule q = sw_rule<RULE>(g, p, live);
    const double capital = g.prm.initial_capital;
    SwLane st;
    SwAcc acc{};
    st.reset(capital);
    acc.max_eq = capital;
    int cur = 0;
    {
        double pre[SW_PRE], bprev = 0.0;
        sw_fetch<BENCH>(g, s, 0, 0, g.len, pre, bprev);
        sw_store<BENCH>(g, 0, pre, bprev, sw_lds);
        __syncthreads();
    }
    sw_pass<RULE, 1, BENCH>(g, s, 0, g.len, sw_lds, cur, wave_live, true, q, st, acc);
    const double T = (double)g.len;
    const double last_eq = st.prev_eq;
    const int32_t trades = st.trades, wins = st.wins;
    acc.mean = acc.ret_sum / T;  // metrics.rs:60
    acc.bmean = acc.bsum / T;
    st.reset(capital);
    sw_pass<RULE, 2, BENCH>(g, s, 0, g.len, sw_lds, cur, wave_live, false, q, st, acc);
    if (!live) return;
    sw_close<BENCH>(g, s, 0, g.len, last_eq, trades, wins, acc, g.summary + (s * g.n_params + p) * PQ_SUMMARY_COLS);
}

// D-26: the sweep with one more grid axis, the window.  Block ((w N + s) pblocks + pb) -- window-major, the order of the loop of sweeps
// it replaces: with the windows of one symbol as neighbours, ((s W + w) pblocks + pb), the same launch took 57.7 ms against 37.3 ms
// (config 3, 32 windows, one run each) -- runs rows
// [t0_w, t1_w) exactly as sweep_kernel runs a series of that length: the
// lane state and the rule's row t - 1 start afresh at t0 (row t0 never signals, row t0 - 1 is never read), T = t1 - t0, the benchmark
// return of row t0 is taken against row t0, alpha spans bm[t0] .. bm[t1 - 1].  summary is [W][N][P][8]; an empty window's cells are 0
// (metrics.rs:17-19).  Only the grid decode, the first tile and the order of the calls are written twice: sweep_kernel written through
// one shared body with lo = 0 is allocated ~25 more VGPRs by the compiler, and its figures are pinned (tests/test_sweep_rules_ref.py).
struct SwWinArgs {
    SwArgs g;
    const pq_sweep_window *windows; // device, [n_windows]; checked against len on the host
    int64_t n_series;
};
template <int RULE, bool BENCH>
__global__ __launch_bounds__(SW_BLOCK) void sweep_windows_kernel(SwWinArgs a) {
    extern __shared__ double sw_lds[];
    const SwArgs &g = a.g;
    const unsigned sw = blockIdx.x / (unsigned)g.pblocks;
    const int64_t p0 = (int64_t)(blockIdx.x % (unsigned)g.pblocks) * blockDim.x;
    const int64_t w = (int64_t)(sw / (unsigned)a.n_series), s = (int64_t)(sw % (unsigned)a.n_series);
    const pq_sweep_window win = a.windows[w]; // uniform over the workgroup
    double *sm_rows = g.summary + (w * a.n_series + s) * g.n_params * PQ_SUMMARY_COLS;
    const int tid = (int)threadIdx.x;
    const int64_t p = p0 + tid;
    const bool live = p < g.n_params;
    if (win.t0 >= win.t1) {
        if (live) bt_summary_zero(sm_rows + p * PQ_SUMMARY_COLS);
        return;
    }
    const int64_t lo = win.t0, hi = win.t1;
    const bool wave_live = p0 + (tid & ~63) < g.n_params; // a wavefront without a parameter set only helps with the staging
    const SwRule q = sw_rule<RULE>(g, p, live);
    const double capital = g.prm.initial_capital;
    SwLane st;
    SwAcc acc{};
    st.reset(capital);
    acc.max_eq = capital;
    int cur = 0;
    {
        double pre[SW_PRE], bprev = 0.0;
        sw_fetch<BENCH>(g, s, lo, lo, hi, pre, bprev);
        sw_store<BENCH>(g, lo, pre, bprev, sw_lds);
        __syncthreads();
    }
    sw_pass<RULE, 1, BENCH>(g, s, lo, hi, sw_lds, cur, wave_live, true, q, st, acc);
    const double T = (double)(hi - lo);
    const double last_eq = st.prev_eq;
    const int32_t trades = st.trades, wins = st.wins;
    acc.mean = acc.ret_sum / T;  // metrics.rs:60
    acc.bmean = acc.bsum / T;
    st.reset(capital);
    sw_pass<RULE, 2, BENCH>(g, s, lo, hi, sw_lds, cur, wave_live, false, q, st, acc);
    if (!live) return;
    sw_close<BENCH>(g, s, lo, hi, last_eq, trades, wins, acc, sm_rows + p * PQ_SUMMARY_COLS);
}

// D-26, selection: one wavefront per (fold f, symbol s).  Lanes stride over the parameter sets of summary[train[f]][s] and keep their
// best metric value with a strict comparison (a NaN ranks as the worst value), the wave reduces on (value, index) -- the lower index
// wins a tie, so an all-NaN column gives 0, like SweepResult.best() -- and the chosen set's eight values are copied from the train and
// the test window.
struct SwSelArgs {
    const double *summary; // [W][N][P][8]
    const int32_t *train, *test; // device, [F]
    int32_t *chosen;
    double *in_sample, *out_sample;
    int64_t n_series, n_params;
    int32_t col, maximize;
};
__global__ __launch_bounds__(64) void sweep_select_kernel(SwSelArgs a) {
    const int lane = (int)threadIdx.x;
    const int64_t f = (int64_t)(blockIdx.x / (unsigned)a.n_series), s = (int64_t)(blockIdx.x % (unsigned)a.n_series);
    const double *tr = a.summary + ((int64_t)a.train[f] * a.n_series + s) * a.n_params * PQ_SUMMARY_COLS;
    const double *te = a.summary + ((int64_t)a.test[f] * a.n_series + s) * a.n_params * PQ_SUMMARY_COLS;
    const bool mx = a.maximize != 0;
    const double worst = mx ? -__builtin_huge_val() : __builtin_huge_val();
    const int NONE = 0x7fffffff; // a lane without a parameter set loses every tie
    auto key = [&](int64_t p) { const double v = tr[p * PQ_SUMMARY_COLS + a.col]; return v != v ? worst : v; };
    double bv = worst;
    int bi = NONE;
    if (lane < a.n_params) { // the lane's first set, then only a strictly better one
        bv = key(lane);
        bi = lane;
        for (int64_t p = lane + 64; p < a.n_params; p += 64) {
            const double v = key(p);
            if (mx ? v > bv : v < bv) { bv = v; bi = (int)p; }
        }
    }
#define SW_BEST(CTRL, RM) { const double tv = btw_dpp<CTRL, RM>(worst, bv); const int ti = btw_dpp<CTRL, RM>(NONE, bi);   \
                            if ((mx ? tv > bv : tv < bv) || (tv == bv && ti < bi)) { bv = tv; bi = ti; } }
    BTW_SCAN_STEPS(SW_BEST) // an inclusive scan: lane 63 holds the best of the wave
#undef SW_BEST
    const int64_t best = __builtin_amdgcn_readlane(bi, 63);
    const int64_t cell = f * a.n_series + s;
    if (lane == 0) a.chosen[cell] = (int32_t)best;
    if (lane < PQ_SUMMARY_COLS) a.in_sample[cell * PQ_SUMMARY_COLS + lane] = tr[best * PQ_SUMMARY_COLS + lane];
    else if (lane < 2 * PQ_SUMMARY_COLS) a.out_sample[cell * PQ_SUMMARY_COLS + lane - PQ_SUMMARY_COLS] = te[best * PQ_SUMMARY_COLS + lane - PQ_SUMMARY_COLS];
}

using SwKernel = void (*)(SwArgs);
template <bool BENCH>
SwKernel sw_kernel_for(int rule) {
    switch (rule) {
    case PQ_SWEEP_RULE_CROSS: return sweep_kernel<PQ_SWEEP_RULE_CROSS, BENCH>;
    case PQ_SWEEP_RULE_BAND: return sweep_kernel<PQ_SWEEP_RULE_BAND, BENCH>;
    case PQ_SWEEP_RULE_CHANNEL: return sweep_kernel<PQ_SWEEP_RULE_CHANNEL, BENCH>;
    case PQ_SWEEP_RULE_BREAKOUT: return sweep_kernel<PQ_SWEEP_RULE_BREAKOUT, BENCH>;
    case PQ_SWEEP_RULE_SCALED_CHANNEL: return sweep_kernel<PQ_SWEEP_RULE_SCALED_CHANNEL, BENCH>;
    case PQ_SWEEP_RULE_CROSS_ZONES: return sweep_kernel<PQ_SWEEP_RULE_CROSS_ZONES, BENCH>;
    case PQ_SWEEP_RULE_CROSS_STRENGTH: return sweep_kernel<PQ_SWEEP_RULE_CROSS_STRENGTH, BENCH>;
    default: return sweep_kernel<SW_GENERIC, BENCH>;
    }
}

using SwWinKernel = void (*)(SwWinArgs);
template <bool BENCH>
SwWinKernel sw_win_kernel_for(int rule) {
    switch (rule) {
    case PQ_SWEEP_RULE_CROSS: return sweep_windows_kernel<PQ_SWEEP_RULE_CROSS, BENCH>;
    case PQ_SWEEP_RULE_BAND: return sweep_windows_kernel<PQ_SWEEP_RULE_BAND, BENCH>;
    case PQ_SWEEP_RULE_CHANNEL: return sweep_windows_kernel<PQ_SWEEP_RULE_CHANNEL, BENCH>;
    case PQ_SWEEP_RULE_BREAKOUT: return sweep_windows_kernel<PQ_SWEEP_RULE_BREAKOUT, BENCH>;
    case PQ_SWEEP_RULE_SCALED_CHANNEL: return sweep_windows_kernel<PQ_SWEEP_RULE_SCALED_CHANNEL, BENCH>;
    case PQ_SWEEP_RULE_CROSS_ZONES: return sweep_windows_kernel<PQ_SWEEP_RULE_CROSS_ZONES, BENCH>;
    case PQ_SWEEP_RULE_CROSS_STRENGTH: return sweep_windows_kernel<PQ_SWEEP_RULE_CROSS_STRENGTH, BENCH>;
    default: return sweep_windows_kernel<SW_GENERIC, BENCH>;
    }
}

// every entry point: `who` names the caller in the messages, max_rule is the last rule it accepts.  windowed: `windows` is a HOST table
// of n_windows row ranges and summary is [n_windows][n_series][n_rules][8]; otherwise the one range is the whole series
pq_status sw_run(const char *who, int max_rule, pq_ctx *ctx, const pq_batch *b, const double *price, const double *const *lines,
                 int32_t n_lines, const pq_sweep_rule *rules, int64_t n_rules, const double *benchmark, int64_t bench_series_stride,
                 const pq_bt_params *bt, double *summary, bool windowed = false, const pq_sweep_window *windows = nullptr,
                 int64_t n_windows = 1) {
    PQ_TRY(pq_check(ctx, b));
    if (ctx->rec) { pq_set_error("%s cannot be recorded into a suite", who); return PQ_ERR_UNSUPPORTED; }
    if (b->offsets) { pq_set_error("%s: ragged batches are not supported", who); return PQ_ERR_UNSUPPORTED; }
    if (n_rules < 0) { pq_set_error("%s: negative n_params", who); return PQ_ERR_ARG; }
    const int R = sw_row_tile(n_lines);
    if (R == 0) { pq_set_error("%s: n_lines must be in [1, %d], not %d", who, PQ_SWEEP_MAX_LINES, (int)n_lines); return PQ_ERR_ARG; }
    if (!bt) { pq_set_error("%s: null parameters", who); return PQ_ERR_ARG; }
    if (n_windows < 0) { pq_set_error("%s: negative n_windows", who); return PQ_ERR_ARG; }
    if (n_rules == 0 || b->n_series == 0) return PQ_OK;
    if (!(rules && summary && (b->len == 0 || (price && lines)))) { pq_set_error("%s: null pointer", who); return PQ_ERR_ARG; }
    for (int j = 0; j < n_lines && b->len > 0; j++)
        if (!lines[j]) { pq_set_error("%s: null line pointer", who); return PQ_ERR_ARG; }
    if (benchmark && bench_series_stride != 0 && bench_series_stride < b->len) { pq_set_error("%s: bench_series_stride must be 0 or >= len", who); return PQ_ERR_ARG; }
    const int waves = sw_waves(n_lines, R, n_rules);
    const int64_t pblocks = (n_rules + 64 * waves - 1) / (64 * waves);
    if (!(b->len <= 0x7fffffffLL && n_rules <= 0x7fffffffLL && pblocks * b->n_series <= 0x7fffffffLL)) { pq_set_error("%s: batch or grid too large", who); return PQ_ERR_ARG; }
    if (windowed) { // the size of the grid first: the table is read only once it is known to be of a sane length
        if (n_windows > 0x7fffffffLL / (pblocks * b->n_series)) {
            pq_set_error("%s: %lld windows make a grid of more than 2^31 - 1 blocks", who, (long long)n_windows);
            return PQ_ERR_ARG;
        }
        if (n_windows > 0 && !windows) { pq_set_error("%s: null window table", who); return PQ_ERR_ARG; }
        for (int64_t w = 0; w < n_windows; w++)
            if (windows[w].t0 < 0 || windows[w].t1 > b->len || windows[w].t0 > windows[w].t1) {
                pq_set_error("%s: window %lld: rows [%lld, %lld) are not a range inside [0, %lld)", who, (long long)w, (long long)windows[w].t0,
                             (long long)windows[w].t1, (long long)b->len);
                return PQ_ERR_ARG;
            }
        if (n_windows == 0) return PQ_OK;
    }
    // the table is checked on the host before anything is launched: the kernel indexes LDS with a, b and c
    std::vector<pq_sweep_rule> host((size_t)n_rules);
    PQ_HIP_TRY(hipMemcpyAsync(host.data(), rules, sizeof(pq_sweep_rule) * (size_t)n_rules, hipMemcpyDeviceToHost, ctx->stream));
    PQ_HIP_TRY(hipStreamSynchronize(ctx->stream));
    int one_rule = host[0].rule; // the rule of every set, or SW_GENERIC
    for (int64_t i = 0; i < n_rules; i++) {
        const pq_sweep_rule &q = host[(size_t)i];
        if (q.rule < 0 || q.rule > max_rule) { pq_set_error("%s: parameter set %lld: unknown rule %d (the rules are 0 .. %d)", who, (long long)i, (int)q.rule, max_rule); return PQ_ERR_ARG; }
        if (q.a < 0 || q.a >= n_lines || (sw_uses_b(q.rule) && (q.b < 0 || q.b >= n_lines))) {
            pq_set_error("%s: parameter set %lld: line a=%d b=%d outside [0, %d)", who, (long long)i, (int)q.a, (int)q.b, (int)n_lines);
            return PQ_ERR_ARG;
        }
        if (sw_uses_c(q.rule) && (q.c < -1 || q.c >= n_lines)) {
            pq_set_error("%s: parameter set %lld: column c=%d outside [-1, %d) (-1 is the price)", who, (long long)i, (int)q.c, (int)n_lines);
            return PQ_ERR_ARG;
        }
        if (q.rule != one_rule) one_rule = SW_GENERIC;
    }
    if (b->len == 0) { // calculate_summary on no rows: all zeros (metrics.rs:17-19); n_windows is 1 where the call is not windowed
        PQ_HIP_TRY(hipMemsetAsync(summary, 0, sizeof(double) * PQ_SUMMARY_COLS * (size_t)n_windows * (size_t)b->n_series * (size_t)n_rules, ctx->stream));
        return PQ_OK;
    }
    const size_t line_bytes = sizeof(double *) * (size_t)n_lines; // the window table lies behind the line pointers
    PQ_TRY(pq_ws_reserve(ctx, line_bytes + (windowed ? sizeof(pq_sweep_window) * (size_t)n_windows : 0)));
    PQ_HIP_TRY(hipMemcpyAsync(ctx->ws, lines, line_bytes, hipMemcpyHostToDevice, ctx->stream));
    pq_sweep_window *dwin = reinterpret_cast<pq_sweep_window *>(static_cast<unsigned char *>(ctx->ws) + line_bytes);
    if (windowed) PQ_HIP_TRY(hipMemcpyAsync(dwin, windows, sizeof(pq_sweep_window) * (size_t)n_windows, hipMemcpyHostToDevice, ctx->stream));
    PQ_HIP_TRY(hipStreamSynchronize(ctx->stream)); // the caller's tables may go away after the call
    SwArgs g{};
    g.price = price; g.lines = (const double *const *)ctx->ws; g.params = rules; g.bench = benchmark; g.summary = summary; g.prm = *bt;
    g.len = b->len; g.stride = b->stride; g.bench_stride = bench_series_stride; g.n_params = n_rules;
    g.n_lines = n_lines; g.R = R; g.pblocks = (int32_t)pblocks;
    g.magic = ((1u << 20) + (uint32_t)R - 1u) / (uint32_t)R;
    const size_t lds = sizeof(double) * 2 * (size_t)(n_lines + 2) * (size_t)R; // <= 2 * SW_TILE doubles = 64 KB
    if (windowed) {
        SwWinArgs a{g, dwin, b->n_series};
        const SwWinKernel kernel = benchmark ? sw_win_kernel_for<true>(one_rule) : sw_win_kernel_for<false>(one_rule);
        hipLaunchKernelGGL(kernel, dim3((unsigned)(pblocks * b->n_series * n_windows)), dim3(64 * waves), lds, ctx->stream, a);
        PQ_HIP_TRY(hipGetLastError());
        return PQ_OK;
    }
    const dim3 grid((unsigned)(pblocks * b->n_series));
    const SwKernel kernel = benchmark ? sw_kernel_for<true>(one_rule) : sw_kernel_for<false>(one_rule);
    hipLaunchKernelGGL(kernel, grid, dim3(64 * waves), lds, ctx->stream, g);
    PQ_HIP_TRY(hipGetLastError());
    return PQ_OK;
}
} // namespace

extern "C" {

int32_t pq_sweep_row_tile(int32_t n_lines) { return sw_row_tile(n_lines); }

pq_status pq_backtest_sweep(pq_ctx *ctx, const pq_batch *b, const double *price, const double *const *lines, int32_t n_lines,
                            const pq_sweep_param *params, int64_t n_params, const double *benchmark, int64_t bench_series_stride,
                            const pq_bt_params *bt, double *summary) {
    // the same 32 bytes; rules 0 and 1 never look at _pad / c
    return sw_run("pq_backtest_sweep", PQ_SWEEP_RULE_BAND, ctx, b, price, lines, n_lines, reinterpret_cast<const pq_sweep_rule *>(params), n_params,
                  benchmark, bench_series_stride, bt, summary);
}

pq_status pq_backtest_sweep_rules(pq_ctx *ctx, const pq_batch *b, const double *price, const double *const *lines, int32_t n_lines,
                                  const pq_sweep_rule *rules, int64_t n_rules, const double *benchmark, int64_t bench_series_stride,
                                  const pq_bt_params *bt, double *summary) {
    return sw_run("pq_backtest_sweep_rules", PQ_SWEEP_RULE_CROSS_STRENGTH, ctx, b, price, lines, n_lines, rules, n_rules, benchmark,
                  bench_series_stride, bt, summary);
}

pq_status pq_backtest_sweep_windows(pq_ctx *ctx, const pq_batch *b, const double *price, const double *const *lines, int32_t n_lines,
                                    const pq_sweep_rule *rules, int64_t n_rules, const pq_sweep_window *windows, int64_t n_windows,
                                    const double *benchmark, int64_t bench_series_stride, const pq_bt_params *bt, double *summary) {
    return sw_run("pq_backtest_sweep_windows", PQ_SWEEP_RULE_CROSS_STRENGTH, ctx, b, price, lines, n_lines, rules, n_rules, benchmark,
                  bench_series_stride, bt, summary, true, windows, n_windows);
}

pq_status pq_sweep_select(pq_ctx *ctx, const double *summary, int64_t n_windows, int64_t n_series, int64_t n_params, const int32_t *train,
                          const int32_t *test, int64_t n_folds, int32_t metric_col, int32_t maximize, int32_t *chosen, double *in_sample,
                          double *out_sample) {
    const char *who = "pq_sweep_select";
    if (!ctx) { pq_set_error("%s: null context", who); return PQ_ERR_ARG; }
    if (ctx->rec) { pq_set_error("%s cannot be recorded into a suite", who); return PQ_ERR_UNSUPPORTED; }
    if (n_windows < 0 || n_series < 0 || n_params < 0 || n_folds < 0) { pq_set_error("%s: negative size", who); return PQ_ERR_ARG; }
    if (metric_col < 0 || metric_col >= PQ_SUMMARY_COLS) { pq_set_error("%s: metric_col %d outside [0, %d)", who, (int)metric_col, PQ_SUMMARY_COLS); return PQ_ERR_ARG; }
    if (n_folds > 0 && !(train && test)) { pq_set_error("%s: null fold table", who); return PQ_ERR_ARG; }
    for (int64_t f = 0; f < n_folds; f++)
        if (train[f] < 0 || train[f] >= n_windows || test[f] < 0 || test[f] >= n_windows) {
            pq_set_error("%s: fold %lld: train window %d or test window %d outside [0, %lld)", who, (long long)f, (int)train[f], (int)test[f], (long long)n_windows);
            return PQ_ERR_ARG;
        }
    if (n_folds == 0 || n_series == 0) return PQ_OK;
    if (n_params < 1) { pq_set_error("%s: no parameter set to choose from", who); return PQ_ERR_ARG; }
    if (!(summary && chosen && in_sample && out_sample)) { pq_set_error("%s: null pointer", who); return PQ_ERR_ARG; }
    if (n_params > 0x7fffffffLL || n_series > 0x7fffffffLL || n_folds > 0x7fffffffLL / n_series) { pq_set_error("%s: grid too large", who); return PQ_ERR_ARG; }
    PQ_TRY(pq_ws_reserve(ctx, 2 * sizeof(int32_t) * (size_t)n_folds));
    int32_t *dfold = static_cast<int32_t *>(ctx->ws);
    PQ_HIP_TRY(hipMemcpyAsync(dfold, train, sizeof(int32_t) * (size_t)n_folds, hipMemcpyHostToDevice, ctx->stream));
    PQ_HIP_TRY(hipMemcpyAsync(dfold + n_folds, test, sizeof(int32_t) * (size_t)n_folds, hipMemcpyHostToDevice, ctx->stream));
    PQ_HIP_TRY(hipStreamSynchronize(ctx->stream)); // the caller's tables may go away after the call
    SwSelArgs a{summary, dfold, dfold + n_folds, chosen, in_sample, out_sample, n_series, n_params, metric_col, maximize};
    hipLaunchKernelGGL(sweep_select_kernel, dim3((unsigned)(n_folds * n_series)), dim3(64), 0, ctx->stream, a);
    PQ_HIP_TRY(hipGetLastError());
    return PQ_OK;
}

} // extern "C"
