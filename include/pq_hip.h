/*
 * pq_hip.h -- C ABI of libpolars_quant_hip.so: the MI355X (gfx950) execution path for the
 * polars-quant technical-indicator + per-symbol backtest hot path.
 *
 * This header is the drop-in boundary.  Each entry point replaces one `#[polars_expr]` plugin
 * function / PyO3 method of the reference (file:line cited per function, paths relative to the
 * reference repo) with a BATCHED call over n_series independent series (symbols): one call here
 * replaces the N per-group plugin calls Polars makes under `.over("symbol")`.
 *
 * Conventions
 *   - all data pointers are DEVICE pointers (hipMalloc'd or torch CUDA tensors); plain C types only
 *   - a column is symbol-major: element (s, t) lives at ptr[s * stride + t], 0 <= t < len
 *   - f64 NULL rows are the NaN bit pattern PQ_NULL_BITS (in and out); int32 outputs that can be
 *     null (ht_trendmode) use PQ_NULL_I32.  pq_nulls_from_arrow / pq_validity_to_arrow convert
 *     from / to Arrow validity bitmaps.
 *   - every call is asynchronous on the context's HIP stream; pq_ctx_sync waits for it
 *   - return value: PQ_OK or an error code; pq_last_error() gives a thread-local message
 *   - parameters whose reference handling would panic (timeperiod == 0 underflow, momentum.rs:52)
 *     yield all-null output instead of aborting
 */
#ifndef PQ_HIP_H
#define PQ_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PQ_NULL_BITS 0x7FF80000504E554CULL
#define PQ_NULL_I32 ((int32_t)0x80000000)

typedef int32_t pq_status;
enum {
    PQ_OK = 0,
    PQ_ERR_ARG = 1,     /* bad argument (null pointer, negative size, stride < len) */
    PQ_ERR_HIP = 2,     /* a HIP runtime call failed */
    PQ_ERR_NULLS = 3,   /* input has nulls and the reference function rejects them (N-B family) */
    PQ_ERR_NOMEM = 4,
    PQ_ERR_UNSUPPORTED = 5,
    PQ_WARN_SLOW_LAYOUT = 100 /* pq_layout_check only: not an error -- results are identical, the kernels take their 8-byte / per-lane forms */
};

typedef struct pq_ctx pq_ctx; /* device + stream + scratch workspace; one per host thread/stream.  A pq_ctx is NOT re-entrant: calls grow its
                               * workspaces on demand, so two host threads must not use one context concurrently (create one each: contexts
                               * are cheap; the Polars plugin symbols keep one per calling thread) */

/* n_series series of `len` rows; consecutive series start `stride` elements apart (stride >= len).
 * RAGGED batches (offsets != NULL): what the reference sees under `.over("symbol")` -- one plugin call per group of whatever
 * length the group has (python/polars_quant/talib/momentum.py:13-16, is_elementwise=False).  The columns are the LONG columns
 * sorted by symbol; `offsets` is a DEVICE array of n_series + 1 row indices, series s = rows [offsets[s], offsets[s + 1]);
 * `len` = the longest series, `stride` = the total row count offsets[n_series].  Every series is computed as if it were
 * passed alone (a series shorter than a warm-up is all-null, as in the reference); output columns have the same long layout.
 * Accepted by every indicator / pattern entry point, pq_backtest_vectorized, pq_backtest_macd_cross, pq_macd_cross_signals, the
 * signal rules and pq_returns; the cross-sectional calls (pq_factor_ic, pq_portfolio_metrics, pq_backtest_leveraged with a
 * benchmark) and suite recording return PQ_ERR_UNSUPPORTED. */
typedef struct {
    int64_t n_series;
    int64_t len;
    int64_t stride;
    const int64_t *offsets; /* NULL: the regular [n_series][stride] layout */
} pq_batch;

/* ---- layout advice (no reference counterpart: Polars hands over dense Arrow buffers) ----
 * Every kernel moves [64 series][8 or 16 rows] tiles with 16-byte accesses when the rows of a column are 16-byte aligned
 * (stride even AND every column base a multiple of 16 B), and is fastest when the row pitch is a multiple of 128 B: every 64 / 128-byte
 * piece of a tile is then one aligned cache line.  Measured on the full suite at 5 000 x 2 520: pitch 2 528
 * 3.9 ms per step, dense even pitch 2 520 4.1 ms, ODD pitch 2 521 5.8 ms (the 8-byte forms: every piece straddles two cache lines).
 *   pq_recommended_stride(len)  the smallest multiple of 16 elements (128 B) >= len: the pitch to allocate [n_series][stride] columns
 *                               with (pq_memcpy_h2d_pitched places a dense host column there)
 *   pq_layout_check(b, cols, n) PQ_OK if the n column bases and the batch's stride take the fast forms, PQ_WARN_SLOW_LAYOUT if the
 *                               call will run the 8-byte forms (odd stride, or a base 8 bytes off) or the per-lane gather forms (a
 *                               base not even 8-byte aligned); pq_last_error() then says which.  Ragged batches (offsets != NULL)
 *                               always return PQ_OK: their groups start at arbitrary rows by construction.  Advisory only: every
 *                               entry point accepts every layout and returns the same values.
 * The library's own allocations follow the advice: the Polars plugin's device copies of a balanced `_over` panel, loader.DeviceFrame
 * and polars_quant_amd.Suite (which also re-houses inputs handed over at a slow pitch once, at record time). */
int64_t pq_recommended_stride(int64_t len);
pq_status pq_layout_check(const pq_batch *b, const void *const *cols, int32_t n_cols);

/* ---- runtime ---- */
int32_t pq_abi_version(void);
const char *pq_last_error(void);
pq_status pq_device_count(int32_t *count);
/* hip_stream: the hipStream_t every call launches on (e.g. torch's current stream); NULL = the default stream */
pq_status pq_ctx_create(int32_t device, void *hip_stream, pq_ctx **out);
pq_status pq_ctx_destroy(pq_ctx *ctx);
pq_status pq_ctx_set_stream(pq_ctx *ctx, void *hip_stream);
pq_status pq_ctx_sync(pq_ctx *ctx);
pq_status pq_malloc(pq_ctx *ctx, size_t bytes, void **dptr);
pq_status pq_free(pq_ctx *ctx, void *dptr);
/* pin / unpin a host buffer (an Arrow data buffer) so that the two copies below DMA straight from / to it */
pq_status pq_host_register(void *host_ptr, size_t bytes);
pq_status pq_host_unregister(void *host_ptr);
pq_status pq_memcpy_h2d(pq_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
pq_status pq_memcpy_d2h(pq_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);
/* The same for `rows` rows of `width_bytes` each with different row pitches on the two sides: a dense host column
 * ([n_series][len], what Arrow hands over) to / from a device column whose pitch is a multiple of 128 B (pq_batch.stride > len:
 * every 64 / 128-byte tile piece is then one aligned cache line, which the suite replay rewards with ~8 %). */
pq_status pq_memcpy_h2d_pitched(pq_ctx *ctx, void *dst_dev, size_t dst_pitch_bytes, const void *src_host, size_t src_pitch_bytes,
                                size_t width_bytes, size_t rows);
pq_status pq_memcpy_d2h_pitched(pq_ctx *ctx, void *dst_host, size_t dst_pitch_bytes, const void *src_dev, size_t src_pitch_bytes,
                                size_t width_bytes, size_t rows);
/* Arrow validity bitmap (LSB-first, bit i = row i of the long column, starting at bit `bit_offset`)
 * -> overwrite null rows of `col` (n contiguous rows) with PQ_NULL_BITS */
pq_status pq_nulls_from_arrow(pq_ctx *ctx, double *col, const uint8_t *validity_bits, int64_t bit_offset, int64_t n);
/* PQ_NULL_BITS rows of `col` -> Arrow validity bitmap (ceil(n/8) bytes) + null count (device int64) */
pq_status pq_validity_to_arrow(pq_ctx *ctx, const double *col, int64_t n, uint8_t *validity_bits, int64_t *null_count);
pq_status pq_count_nulls(pq_ctx *ctx, const pq_batch *b, const double *col, int64_t *host_count);

/* ---- overlap studies (src/talib/overlap.rs) ---- */
pq_status pq_sma(pq_ctx *, const pq_batch *, const double *real, int64_t timeperiod, double *out);              /* :494 */
pq_status pq_ema(pq_ctx *, const pq_batch *, const double *real, int64_t timeperiod, double *out);              /* :128 */
pq_status pq_bbands(pq_ctx *, const pq_batch *, const double *real, int64_t timeperiod, double nbdevup,
                    double nbdevdn, double *bb_upper, double *bb_middle, double *bb_lower);                     /* :47 */
pq_status pq_dema(pq_ctx *, const pq_batch *, const double *real, int64_t timeperiod, double *out);             /* :119 */
pq_status pq_tema(pq_ctx *, const pq_batch *, const double *real, int64_t timeperiod, double *out);             /* :513 */
pq_status pq_t3(pq_ctx *, const pq_batch *, const double *real, int64_t timeperiod, double vfactor, double *out); /* :503 */
pq_status pq_trima(pq_ctx *, const pq_batch *, const double *real, int64_t timeperiod, double *out);            /* :522 */
pq_status pq_wma(pq_ctx *, const pq_batch *, const double *real, int64_t timeperiod, double *out);              /* :531 */
pq_status pq_kama(pq_ctx *, const pq_batch *, const double *real, int64_t timeperiod, double *out);             /* :137 */
pq_status pq_ma(pq_ctx *, const pq_batch *, const double *real, int64_t timeperiod, int64_t matype, double *out); /* :146 */
pq_status pq_midpoint(pq_ctx *, const pq_batch *, const double *real, int64_t timeperiod, double *out);         /* :180 */
pq_status pq_midprice(pq_ctx *, const pq_batch *, const double *high, const double *low, int64_t timeperiod,
                      double *out);                                                                             /* :281 */
pq_status pq_mama(pq_ctx *, const pq_batch *, const double *real, double fastlimit, double slowlimit,
                  double *mama, double *fama);                                                                  /* :156 */
pq_status pq_mavp(pq_ctx *, const pq_batch *, const double *real, const double *periods, int64_t minperiod,
                  int64_t maxperiod, int64_t matype, double *out);                                              /* :407 */
pq_status pq_sar(pq_ctx *, const pq_batch *, const double *high, const double *low, double acceleration,
                 double maximum, double *out);                                                                  /* :437 */
pq_status pq_sarext(pq_ctx *, const pq_batch *, const double *high, const double *low, double startvalue,
                    double offsetonreverse, double accelerationinitlong, double accelerationlong,
                    double accelerationmaxlong, double accelerationinitshort, double accelerationshort,
                    double accelerationmaxshort, double *out);                                                  /* :457 */

/* ---- momentum (src/talib/momentum.rs; composites python/polars_quant/talib/momentum.py) ---- */
pq_status pq_adx(pq_ctx *, const pq_batch *, const double *high, const double *low, const double *close,
                 int64_t timeperiod, double *out);                                                              /* :11 */
pq_status pq_adxr(pq_ctx *, const pq_batch *, const double *high, const double *low, const double *close,
                  int64_t timeperiod, double *out);                                                             /* :32 */
pq_status pq_dx(pq_ctx *, const pq_batch *, const double *high, const double *low, const double *close,
                int64_t timeperiod, double *out);                                                               /* :226 */
pq_status pq_plus_di(pq_ctx *, const pq_batch *, const double *high, const double *low, const double *close,
                     int64_t timeperiod, double *out);                                                          /* :400 */
pq_status pq_minus_di(pq_ctx *, const pq_batch *, const double *high, const double *low, const double *close,
                      int64_t timeperiod, double *out);                                                         /* :345 */
pq_status pq_plus_dm(pq_ctx *, const pq_batch *, const double *high, const double *low, int64_t timeperiod,
                     double *out);                                                                              /* :414 */
pq_status pq_minus_dm(pq_ctx *, const pq_batch *, const double *high, const double *low, int64_t timeperiod,
                      double *out);                                                                             /* :359 */
pq_status pq_aroon(pq_ctx *, const pq_batch *, const double *high, const double *low, int64_t timeperiod,
                   double *aroon_up, double *aroon_down);                                                       /* :70 */
pq_status pq_aroonosc(pq_ctx *, const pq_batch *, const double *high, const double *low, int64_t timeperiod,
                      double *out);                                                             /* momentum.py:40 */
/* Multi-output forms: several reference functions over the same inputs evaluated as ONE job (one in-tile, one walk); every
 * output column is bit-identical to the single function's.  A DataFrame query that asks for several of them
 * (df.with_columns([EMA, DEMA, TEMA, TRIX, ...])) maps onto these like common-subexpression elimination. */
pq_status pq_ema_all(pq_ctx *, const pq_batch *, const double *real, int64_t timeperiod, double *ema, double *dema, double *tema,
                     double *trix);
pq_status pq_atr_all(pq_ctx *, const pq_batch *, const double *high, const double *low, const double *close, int64_t timeperiod,
                     double *atr, double *natr);
pq_status pq_dm_pair(pq_ctx *, const pq_batch *, const double *high, const double *low, int64_t timeperiod, double *plus_dm,
                     double *minus_dm);
pq_status pq_ad_all(pq_ctx *, const pq_batch *, const double *high, const double *low, const double *close, const double *volume,
                    int64_t fastperiod, int64_t slowperiod, double *ad, double *adosc);
pq_status pq_macd_pair(pq_ctx *, const pq_batch *, const double *real, int64_t fastperiod, int64_t slowperiod, int64_t signalperiod,
                       int64_t macdfix_signalperiod, double *macd, double *macdsignal, double *macdhist, double *fix_macd,
                       double *fix_signal, double *fix_hist);
/* Wilder's directional system over (high, low, close): DX, +DI, -DI, ADX, ADXR and ATR, NATR of one timeperiod as one job */
pq_status pq_dm_system_all(pq_ctx *, const pq_batch *, const double *high, const double *low, const double *close, int64_t timeperiod,
                           double *dx, double *plus_di, double *minus_di, double *adx, double *adxr, double *atr, double *natr);
/* SMA(timeperiod) and MA(timeperiod, matype 0) are the same walk (overlap.rs:857-869: `ma` dispatches to calc_sma): one job, both columns */
pq_status pq_sma_ma(pq_ctx *, const pq_batch *, const double *real, int64_t timeperiod, double *sma, double *ma);
/* the two up/down-move oscillators of one timeperiod as one job */
pq_status pq_cmo_rsi(pq_ctx *, const pq_batch *, const double *real, int64_t timeperiod, double *cmo, double *rsi);
/* the volume family over (high, low, close, volume): MFI + AD + ADOSC + OBV as one job (4 in / 4 out: MFI's own LDS need) */
pq_status pq_volume_all(pq_ctx *, const pq_batch *, const double *high, const double *low, const double *close, const double *volume,
                        int64_t mfi_timeperiod, int64_t adosc_fastperiod, int64_t adosc_slowperiod, double *mfi, double *ad,
                        double *adosc, double *obv);
pq_status pq_sar_pair(pq_ctx *, const pq_batch *, const double *high, const double *low, double acceleration, double maximum,
                      double startvalue, double offsetonreverse, double accelerationinitlong, double accelerationlong,
                      double accelerationmaxlong, double accelerationinitshort, double accelerationshort,
                      double accelerationmaxshort, double *sar, double *sarext);
/* STOCH + STOCHF of one fastk_period: the rolling extrema are evaluated once */
pq_status pq_stoch_all(pq_ctx *, const pq_batch *, const double *high, const double *low, const double *close, int64_t fastk_period,
                       int64_t slowk_period, int64_t slowk_matype, int64_t slowd_period, int64_t slowd_matype, int64_t fastd_period,
                       int64_t fastd_matype, double *slowk, double *slowd, double *fastk, double *fastd);
pq_status pq_apo_ppo(pq_ctx *, const pq_batch *, const double *real, int64_t fastperiod, int64_t slowperiod, int64_t matype,
                     double *apo, double *ppo);
/* AROON and AROONOSC of the same timeperiod from one window scan (multi-output form, like pq_dmi_all) */
pq_status pq_aroon_all(pq_ctx *, const pq_batch *, const double *high, const double *low, int64_t timeperiod,
                       double *aroon_up, double *aroon_down, double *aroonosc);
pq_status pq_bop(pq_ctx *, const pq_batch *, const double *open, const double *high, const double *low,
                 const double *close, double *out);                                                             /* :113 */
pq_status pq_cci(pq_ctx *, const pq_batch *, const double *high, const double *low, const double *close,
                 int64_t timeperiod, double *out);                                                              /* :138 */
pq_status pq_cmo(pq_ctx *, const pq_batch *, const double *real, int64_t timeperiod, double *out);              /* :181 */
pq_status pq_macd(pq_ctx *, const pq_batch *, const double *real, int64_t fastperiod, int64_t slowperiod,
                  int64_t signalperiod, double *macd, double *macd_signal, double *macd_hist);                  /* :250 */
pq_status pq_macdext(pq_ctx *, const pq_batch *, const double *real, int64_t fastperiod, int64_t fastmatype,
                     int64_t slowperiod, int64_t slowmatype, int64_t signalperiod, int64_t signalmatype,
                     double *macd_dif, double *macd_dea, double *macd_hist);                    /* momentum.py:83 */
pq_status pq_macdfix(pq_ctx *, const pq_batch *, const double *real, int64_t signalperiod, double *macd,
                     double *macd_signal, double *macd_hist);                                   /* momentum.py:90 */
pq_status pq_mfi(pq_ctx *, const pq_batch *, const double *high, const double *low, const double *close,
                 const double *volume, int64_t timeperiod, double *out);                                        /* :286 */
pq_status pq_mom(pq_ctx *, const pq_batch *, const double *real, int64_t timeperiod, double *out);              /* :384 */
pq_status pq_roc(pq_ctx *, const pq_batch *, const double *real, int64_t timeperiod, double *out);              /* :439 */
pq_status pq_rocp(pq_ctx *, const pq_batch *, const double *real, int64_t timeperiod, double *out);             /* :456 */
pq_status pq_rocr(pq_ctx *, const pq_batch *, const double *real, int64_t timeperiod, double *out);             /* :473 */
pq_status pq_rocr100(pq_ctx *, const pq_batch *, const double *real, int64_t timeperiod, double *out);          /* :490 */
pq_status pq_rsi(pq_ctx *, const pq_batch *, const double *real, int64_t timeperiod, double *out);              /* :507 */
pq_status pq_trix(pq_ctx *, const pq_batch *, const double *real, int64_t timeperiod, double *out);             /* :544 */
pq_status pq_ultosc(pq_ctx *, const pq_batch *, const double *high, const double *low, const double *close,
                    int64_t timeperiod1, int64_t timeperiod2, int64_t timeperiod3, double *out);                /* :572 */
pq_status pq_willr(pq_ctx *, const pq_batch *, const double *high, const double *low, const double *close,
                   int64_t timeperiod, double *out);                                                            /* :630 */
pq_status pq_apo(pq_ctx *, const pq_batch *, const double *real, int64_t fastperiod, int64_t slowperiod,
                 int64_t matype, double *out);                                                  /* momentum.py:25 */
pq_status pq_ppo(pq_ctx *, const pq_batch *, const double *real, int64_t fastperiod, int64_t slowperiod,
                 int64_t matype, double *out);                                                 /* momentum.py:136 */
pq_status pq_stoch(pq_ctx *, const pq_batch *, const double *high, const double *low, const double *close,
                   int64_t fastk_period, int64_t slowk_period, int64_t slowk_matype, int64_t slowd_period,
                   int64_t slowd_matype, double *slowk, double *slowd);                        /* momentum.py:178 */
pq_status pq_stochf(pq_ctx *, const pq_batch *, const double *high, const double *low, const double *close,
                    int64_t fastk_period, int64_t fastd_period, int64_t fastd_matype, double *fastk,
                    double *fastd);                                                            /* momentum.py:188 */
pq_status pq_stochrsi(pq_ctx *, const pq_batch *, const double *real, int64_t timeperiod, int64_t fastk_period,
                      int64_t fastd_period, int64_t fastd_matype, double *fastk, double *fastd); /* momentum.py:197 */

/* fused multi-output forms: the shared core is evaluated once (bit-identical to the single-output calls) */
pq_status pq_dmi_all(pq_ctx *, const pq_batch *, const double *high, const double *low, const double *close,
                     int64_t timeperiod, double *dx, double *plus_di, double *minus_di, double *adx,
                     double *adxr);                                                    /* momentum.rs:668-727 calc_dm */
pq_status pq_ht_all(pq_ctx *, const pq_batch *, const double *real, double *ht_dcperiod, double *ht_dcphase,
                    double *inphase, double *quadrature, double *sine, double *leadsine);    /* cycle.rs:27-63 */

/* ---- volatility / volume / price (src/talib/{volatility,volume,price}.rs) ---- */
pq_status pq_trange(pq_ctx *, const pq_batch *, const double *high, const double *low, const double *close,
                    double *out);                                                              /* volatility.rs:51 */
pq_status pq_atr(pq_ctx *, const pq_batch *, const double *high, const double *low, const double *close,
                 int64_t timeperiod, double *out);                                             /* volatility.rs:18 */
pq_status pq_natr(pq_ctx *, const pq_batch *, const double *high, const double *low, const double *close,
                  int64_t timeperiod, double *out);                                            /* volatility.rs:34 */
pq_status pq_ad(pq_ctx *, const pq_batch *, const double *high, const double *low, const double *close,
                const double *volume, double *out);                                                /* volume.rs:19 */
pq_status pq_adosc(pq_ctx *, const pq_batch *, const double *high, const double *low, const double *close,
                   const double *volume, int64_t fastperiod, int64_t slowperiod, double *out);     /* volume.rs:34 */
pq_status pq_obv(pq_ctx *, const pq_batch *, const double *close, const double *volume, double *out); /* volume.rs:70 */
pq_status pq_avgprice(pq_ctx *, const pq_batch *, const double *open, const double *high, const double *low,
                      const double *close, double *out);                                            /* price.rs:10 */
pq_status pq_medprice(pq_ctx *, const pq_batch *, const double *high, const double *low, double *out); /* price.rs:34 */
pq_status pq_typprice(pq_ctx *, const pq_batch *, const double *high, const double *low, const double *close,
                      double *out);                                                                 /* price.rs:53 */
pq_status pq_wclprice(pq_ctx *, const pq_batch *, const double *high, const double *low, const double *close,
                      double *out);                                                                 /* price.rs:74 */

/* ---- returns (README.md:46-75 `returns(df, price_col, period, method, return_col)`; README-only, decision D-13) ----
 * method 0 "simple": (p[t] - p[t-period]) / p[t-period];  1 "log": ln(p[t] / p[t-period]).  Null for t < period and where
 * either price is null; period <= 0 or another method: all null.  Pinned by the reference-held vector README.md:75. */
pq_status pq_returns(pq_ctx *, const pq_batch *, const double *price, int64_t period, int64_t method, double *out);

/* rolling maximum / minimum over the last `window` rows, null until the frame holds `window` non-null rows (the Polars
 * rolling_max / rolling_min of momentum.py:181-183): channel bounds for the README's breakout strategy (README.md:947) */
pq_status pq_rolling_max(pq_ctx *, const pq_batch *, const double *x, int64_t window, double *out);
pq_status pq_rolling_min(pq_ctx *, const pq_batch *, const double *x, int64_t window, double *out);

/* ---- cycle (src/talib/cycle.rs) ---- */
pq_status pq_ht_dcperiod(pq_ctx *, const pq_batch *, const double *real, double *out);                          /* :10 */
pq_status pq_ht_dcphase(pq_ctx *, const pq_batch *, const double *real, double *out);                           /* :75 */
pq_status pq_ht_phasor(pq_ctx *, const pq_batch *, const double *real, double *inphase, double *quadrature);    /* :159 */
pq_status pq_ht_sine(pq_ctx *, const pq_batch *, const double *real, double *sine, double *leadsine);           /* :236 */
pq_status pq_ht_trendline(pq_ctx *, const pq_batch *, const double *real, double *out);                         /* :310 */
pq_status pq_ht_trendmode(pq_ctx *, const pq_batch *, const double *real, int32_t *out);                        /* :377 */

/* ---- candlestick patterns (src/talib/pattern.rs:10-2062) ---- */
#define PQ_N_PATTERNS 61
/* names in id order, lower-case plugin names ("cdl2crows", ...) */
const char *pq_pattern_name(int32_t id);
int32_t pq_pattern_id(const char *name);
/* one recogniser; penetration is used by ids 14,19,20,42,43,45 (pattern.rs:529,675,713,1426,1464,1529) */
pq_status pq_cdl(pq_ctx *, const pq_batch *, int32_t pattern_id, const double *open, const double *high,
                 const double *low, const double *close, double penetration, int32_t *out);
/* all 61 in one pass over OHLC: outs[id] may be NULL to skip a pattern; penetrations[id] per pattern */
pq_status pq_cdl_all(pq_ctx *, const pq_batch *, const double *open, const double *high, const double *low,
                     const double *close, const double *penetrations /* host, 61 */, int32_t *const *outs /* host, 61 device ptrs */);

/* ---- backtest (src/backtest/vectorized.rs:69-224, src/backtest/metrics.rs:7-152) ---- */
typedef struct {
    double initial_capital, buy_slippage, sell_slippage, buy_commission_rate, sell_commission_rate,
        min_commission, position_size;
} pq_bt_params; /* vectorized.rs:38 defaults: 1e5, 0, 0, 3e-4, 3e-4, 5, 1 */
#define PQ_SUMMARY_COLS 8 /* annualized_return, max_drawdown, alpha, beta, sharpe_ratio, max_profit, win_rate, total_trades */
/* buy/sell: uint8 0/1 per row (null -> 0, vectorized.rs:80-98); price null -> NaN (:70-78);
 * EVERY column (price, buy, sell, benchmark, position, cash, equity) is [n_series][stride]: element (s, t) at
 * ptr[s * stride + t] -- a benchmark shared by all series must be replicated per series by the caller;
 * benchmark may be NULL; position/cash/equity may be NULL (summary only); summary is [n_series][8] */
pq_status pq_backtest_vectorized(pq_ctx *, const pq_batch *, const double *price, const uint8_t *buy,
                                 const uint8_t *sell, const double *benchmark, const pq_bt_params *params,
                                 double *position, double *cash, double *equity, double *summary);
/* fused strategy + backtest: MACD(fast,slow,signal) cross signals generated on the fly
 * (buy: macd crosses above signal; sell: crosses below), then the same scan + summary */
pq_status pq_backtest_macd_cross(pq_ctx *, const pq_batch *, const double *close, int64_t fastperiod,
                                 int64_t slowperiod, int64_t signalperiod, const pq_bt_params *params,
                                 double *position, double *cash, double *equity, double *summary);
pq_status pq_macd_cross_signals(pq_ctx *, const pq_batch *, const double *close, int64_t fastperiod,
                                int64_t slowperiod, int64_t signalperiod, uint8_t *buy, uint8_t *sell);
/* Both backtests run ONE SYMBOL PER WAVEFRONT for len <= 8192 (csrc/ops_backtest_wave.h): the MACD state machine is run in
 * 64 speculative row chunks per symbol whose hand-over states are compared bit for bit (a chunk that fails is re-run from
 * its predecessor's state, so results are exact either way).  out3 (host): [0] symbols processed that way since the last
 * reset, [1] chunks that failed the bit test, [2] chunk re-runs.  Synchronises the context's stream. */
pq_status pq_backtest_wave_stats(pq_ctx *, int64_t *out3, int32_t reset);
/* The contractive recurrences of the indicator suite -- calc_ema (overlap.rs:660-730) and its cascades DEMA / TEMA / TRIX, MACD
 * (momentum.rs:250-283), Wilder's calc_rma behind RSI (momentum.rs:507-541), +DM / -DM, DX / DI / ADX / ADXR (momentum.rs:668-727),
 * ATR / NATR (volatility.rs:18-48) -- and the extrema of MIDPOINT have a ONE-SYMBOL-PER-WAVEFRONT form (csrc/wt_dev.h): 64 row chunks
 * per symbol, started from prefix-scanned seeds, whose hand-over states are compared bit for bit (a chunk that fails is re-run from
 * its predecessor's state: results are the serial walk's either way).  DIRECT calls (not recorded into a suite) take it on regular
 * batches with 1 024 <= len <= 4 096 where it beats the lane-per-symbol kernel of the function (EMA, TRIX, RSI, +DM / -DM, ATR / NATR,
 * MIDPOINT, pq_ema_all, pq_macd_pair, pq_dm_pair, pq_atr_all), and on RAGGED batches whose groups average >= 1 024 rows (every function
 * named above).  A symbol / group with a NULL or NaN input is left to the lane-per-symbol kernel of the same function, launched gated
 * behind.  out4 (host): [0] symbols computed that way since the last reset, [1] chunks that failed the bit test, [2] chunk re-runs,
 * [3] symbols handed to the gated general path.  Synchronises the context's stream. */
pq_status pq_wt_stats(pq_ctx *, int64_t *out4, int32_t reset);
/* Ragged batches whose groups are of similar length (n_series x pq_recommended_stride(longest) <= 1.5 x total rows, >= 16 groups,
 * >= 16 384 rows) do not run the per-lane gather forms of the sequential kernels: every function here is causal in time, so the groups
 * are re-housed as the rows of a regular padded batch (one streaming copy per input column), the tiled kernel of the same function
 * walks it -- told every group's own length, so short groups see the reference's short-series rules -- and the groups' rows of every
 * output are copied back (csrc/pq_dev.h launch_seq, csrc/runtime.hip rg_pack / rg_unpack).  Bit-identical to the gather forms, 2-10 x
 * faster on `.over("symbol")`-shaped batches (profiles/r05_bench_ragged.json).  *calls: launches that took this path on the context
 * since the last reset.  PQ_NO_RG_PACK=1 in the environment keeps the gather forms (A/B runs and tests). */
pq_status pq_ragged_rehouse_stats(pq_ctx *, int64_t *calls, int32_t reset);

/* ---- multi-GPU: symbols are split statically over the ranks -- rank r of G owns [floor(N r / G), floor(N (r + 1) / G)),
 * a contiguous byte range of every symbol-major column -- and every rank runs the calls above on its own shard with no
 * communication.  The one exchange is the per-symbol summary table (reference: the dict of vectorized.rs:204-223 per symbol):
 *   pq_comm_unique_id   rank 0 makes the 128-byte rendezvous id; the HOST ships it to the other ranks (its own channel)
 *   pq_comm_init        collective over the `world` ranks (one process per GPU); RCCL is bound at run time (dlopen)
 *   pq_gather_summaries local [n_local][8] (this rank's shard, device) -> all [n_symbols][8] (device, symbol order) on every
 *                       rank, on the context's stream: one ncclAllGather when the shards are equal, else one grouped broadcast
 *                       per rank */
#define PQ_COMM_ID_BYTES 128
pq_status pq_comm_unique_id(void *id128);
pq_status pq_comm_init(pq_ctx *, int32_t rank, int32_t world, const void *id128);
pq_status pq_comm_destroy(pq_ctx *);
pq_status pq_shard_range(int64_t n_symbols, int32_t rank, int32_t world, int64_t *lo, int64_t *hi);
pq_status pq_gather_summaries(pq_ctx *, const double *local, int64_t n_symbols, double *all);
/* The same exchange OFF the step's critical path (round 5): at 8 GPUs a 625-symbol backtest step is ~50 us and an all-gather tens of
 * us, so a gather in series behind every step would cost a third of the throughput.
 *   pq_gather_summaries_begin  marks everything enqueued on the context's stream so far (the step that produced `local`) with an
 *                              event; the communicator's OWN stream (created on first use, highest priority) waits for it and takes
 *                              the collective.  Returns at once: the context's stream is free for the next step.  slot = 0 / 1.
 *   pq_gather_summaries_end    the context's stream waits -- on the device, the host does not block -- for that slot's collective:
 *                              work enqueued afterwards may read `all` and overwrite `local`.  A no-op on an idle slot.
 * Double-buffer `local` / `all` by slot and call _end(slot) just before the step that rewrites local[slot]: one exchange is then in
 * flight beside the next step's kernels (polars_quant_amd/distributed.py: OverlappedGather; bench.py --gpus N times it).  No
 * reference counterpart (single process). */
pq_status pq_gather_summaries_begin(pq_ctx *, const double *local, int64_t n_symbols, double *all, int32_t slot);
pq_status pq_gather_summaries_end(pq_ctx *, int32_t slot);
/* host-side wait for the communicator's own stream (e.g. to bound the FIRST exchange from a helper thread: a collective that never
 * returns then blocks that thread, not the context's stream) */
pq_status pq_comm_sync(pq_ctx *);

/* ---- the README's `Strategy` signal rules (README.md:862-994; README-only, decision D-11 in
 * oracle/backtest.c): indicator columns -> uint8 buy / sell columns for the backtests above.  Row-parallel.
 *   cross:   buy = a[i-1] <= b[i-1] && a[i] > b[i];  sell mirrored            (MA / MACD / STOCH / trend strategies)
 *   band:    buy = x[i-1] < lower && x[i] >= lower;  sell = x[i-1] > upper && x[i] <= upper      (RSI / CCI / STOCH)
 *   channel: mode 0 reversion (BBANDS): buy = price crosses below `lo`, sell = crosses above `hi`;
 *            mode 1 breakout (Donchian): buy = price[i] > hi[i-1], sell = price[i] < lo[i-1]
 * a rule is false where any value it reads is null, and on row 0 */
pq_status pq_cross_signals(pq_ctx *, const pq_batch *, const double *a, const double *b, uint8_t *buy, uint8_t *sell);
pq_status pq_band_signals(pq_ctx *, const pq_batch *, const double *x, double lower, double upper, uint8_t *buy, uint8_t *sell);
pq_status pq_channel_signals(pq_ctx *, const pq_batch *, const double *price, const double *lo, const double *hi, int32_t mode,
                             uint8_t *buy, uint8_t *sell);

/* The remaining comparisons of the README's fourteen `Strategy` generators (README.md:942-956; definitions = decision D-11b),
 * row-parallel and recordable into a suite in front of pq_backtest_vectorized.  A NULL compares false everywhere.
 *   pq_gate_signals   (buy_in, sell_in) -> (buy, sell), in place allowed; mode 0 zones: buy &= a < k0, sell &= a > k1 (stoch);
 *                     1 strength: both &= a > k0 (adx); 2: buy &= a > c (ma trend filter); 3: buy &= a[i] > a[i-1] (slope filter);
 *                     4: buy &= (a - c) > |c| * k0 (distance filter)
 *   pq_zscore         z = (price - mid) / (upper - mid), NULL where upper is (reversion: then pq_band_signals on z)
 *   pq_scale_band     lo = base * f_lo, hi = base * f_hi, NULL where base is (grid: then pq_channel_signals mode 0)
 *   pq_volume_surge_signals  surge = volume > multiplier * avg_volume; buy = surge on an up close, sell = surge on a down close
 *   pq_gap_signals    buy = open[i] > high[i-1] * f_up, sell = open[i] < low[i-1] * f_dn
 *   pq_pattern_any_signals   buy = any of <= 16 recogniser columns == +100, sell = any of <= 16 == -100 (host arrays of device pointers)
 *   pq_ma_stack_signals      buy = first bar where mas[0] > mas[1] > ... holds, sell = first bar of the reverse order (2..16 columns) */
pq_status pq_gate_signals(pq_ctx *, const pq_batch *, const double *a, const double *c, int32_t mode, double k0, double k1,
                          const uint8_t *buy_in, const uint8_t *sell_in, uint8_t *buy, uint8_t *sell);
pq_status pq_zscore(pq_ctx *, const pq_batch *, const double *price, const double *upper, const double *mid, double *z);
pq_status pq_scale_band(pq_ctx *, const pq_batch *, const double *base, double f_lo, double f_hi, double *lo, double *hi);
pq_status pq_volume_surge_signals(pq_ctx *, const pq_batch *, const double *volume, const double *avg_volume, const double *close,
                                  double multiplier, uint8_t *buy, uint8_t *sell);
pq_status pq_gap_signals(pq_ctx *, const pq_batch *, const double *open, const double *high, const double *low, double f_up, double f_dn,
                         uint8_t *buy, uint8_t *sell);
pq_status pq_pattern_any_signals(pq_ctx *, const pq_batch *, const int32_t *const *bullish, int32_t n_bullish,
                                 const int32_t *const *bearish, int32_t n_bearish, uint8_t *buy, uint8_t *sell);
pq_status pq_ma_stack_signals(pq_ctx *, const pq_batch *, const double *const *mas, int32_t n, uint8_t *buy, uint8_t *sell);

/* ---- the README's multi-symbol `Backtest` (README.md:346-640; README-only, no source).
 * Semantics = decision D-10 (oracle/backtest.c): independent capital pool per symbol, 100-share lots, leverage
 * with daily compounding interest on the debt, margin call (forced sale), commission with a minimum, proportional
 * slippage.  One symbol per lane; every column is [n_series][stride].
 *   cash_net = cash - debt, stock_value, total_value: daily records (get_daily_records), all required.
 *   trade records (get_position_records): the first max_trades closed trades per symbol in [n_series][max_trades] arrays,
 *   all eight arrays or none (NULL); trade_count [n_series] counts every closed trade.  reason: 1 signal, 2 margin call.
 *   benchmark: ONE series of b->len rows shared by all symbols, or NULL; summary [n_series][8] as pq_backtest_vectorized. */
typedef struct {
    double initial_capital, position_size, leverage, margin_call_threshold, interest_rate, commission_rate,
        min_commission, slippage;
} pq_lev_params; /* README.md:356-365 defaults: 1e5, 1, 1, 0.3, 0.06, 3e-4, 5, 0 */
pq_status pq_backtest_leveraged(pq_ctx *, const pq_batch *, const double *price, const uint8_t *buy, const uint8_t *sell,
                                const double *benchmark, const pq_lev_params *params, double *cash_net,
                                double *stock_value, double *total_value, int32_t max_trades, int32_t *trade_count,
                                int32_t *entry_day, int32_t *exit_day, double *entry_price, double *exit_price,
                                double *quantity, double *pnl, double *pnl_pct, int32_t *reason, double *summary);
#define PQ_PORTFOLIO_COLS 10 /* portfolio_value, daily_pnl, daily_return_pct, cumulative_pnl, cumulative_return_pct,
                                benchmark_return_pct, alpha_pct, relative_return_pct, beta, (reserved 0) */
/* get_performance_metrics (README.md:455-477): per-day sums over the symbols of this batch (blocks of 256 symbols, ascending
 * inside a block, block sums added in ascending order), then the
 * day-to-day metrics; out is [b->len][PQ_PORTFOLIO_COLS]; benchmark: one series of b->len rows or NULL */
pq_status pq_portfolio_metrics(pq_ctx *, const pq_batch *, const double *total_value, double initial_total,
                               const double *benchmark, double *out);

/* ---- rank 1, continued: the statistics report of `Backtest` (README.md:511-548, :627-640; README-only, decision D-22 in DESIGN.md).
 * One row of PQ_REPORT_COLS f64 per symbol (names: _spec.REPORT_COLS), from its total_value row [n_series][stride], the initial capital,
 * the first min(trade_count, max_trades) records of pq_backtest_leveraged and ONE shared benchmark series (or NULL):
 *   0-14  the curve: final value, P&L, total / annualized / mean daily return, max drawdown and its longest run of under-water days,
 *         daily / annualized volatility, Sharpe, Sortino, Calmar, positive / negative days, daily win rate
 *   15-37 the trades: counts, win rate, gross profit / loss, profit factor, average / largest win and loss, holding days, the longest
 *         winning / losing streak, turnover, fees (the engine's own, bit for bit), fee ratio, average trade amount, capital use,
 *         margin calls
 *   38-44 the benchmark: its return, excess return, daily alpha, beta, information ratio, days ahead and their rate
 *   45-47 carriers of the portfolio row: hold days of winners, of losers, and the summed entry amount
 * Sums run in ONE order: 64 partials (partial k adds x[k], x[k + 64], ... from +0.0), folded p[k] += p[k + s], s = 32 .. 1.  A count is
 * stored as f64, a missing value (a ratio over 0, an empty maximum) is PQ_NULL_BITS.  A NULL or non-finite total_value makes 0-14 and
 * 38-44 NULL, a NULL or non-finite benchmark 38-44; trade_count > max_trades (records cut short) or no record arrays make 16-37 NULL;
 * without trade_count 15 is NULL too.  The seven record arrays are all passed or all NULL; params is read for commission_rate and
 * min_commission.  initial_capital must be positive and finite.  Ragged batches: PQ_ERR_UNSUPPORTED. */
#define PQ_REPORT_COLS 48
pq_status pq_backtest_report(pq_ctx *, const pq_batch *, const double *total_value, double initial_capital, const double *benchmark,
                             const pq_lev_params *params, int32_t max_trades, const int32_t *trade_count, const int32_t *entry_day,
                             const int32_t *exit_day, const double *entry_price, const double *exit_price, const double *quantity,
                             const double *pnl, const int32_t *reason, double *report);
/* The portfolio row (D-22) from the [n_symbols][PQ_REPORT_COLS] rows: 0-14 and 38-44 are copied from curve_row, the report row of the
 * portfolio_value series (pq_portfolio_metrics column 0 with initial_capital * n_symbols as its capital); trade counts are integer sums,
 * the trade sums are added in D-10's order (blocks of 256 symbols, ascending), the ratios are formed from the sums (capital use over the
 * per-symbol initial_capital), extrema and streaks are the extremes over the symbols; 45 / 46: index of the best / worst symbol by total
 * return (ties: the lowest index; a NULL return is skipped), 47: symbols with total_trades > 0.  One symbol with NULL trade columns
 * makes 16-37 NULL.  out: PQ_REPORT_COLS values. */
pq_status pq_report_portfolio(pq_ctx *, int64_t n_symbols, const double *report, const double *curve_row, double initial_capital,
                              double *out);

/* ---- SequentialBacktester (src/backtest/sequential.rs:48-171, :207-336; decision D-23 in DESIGN.md): the shared-cash portfolio engine,
 * replayed from order tapes.  The reference's callback sees an OrderContext and the period index only (:291-294), so its orders do not
 * depend on the engine's state: they are recorded first and matched here, one wavefront per tape.
 *   A tape has n_periods periods over the assets 0 .. n_assets - 1.  Orders (asset, quantity, price) lie in callback order; quantity is
 *   signed (buy > 0, sell < 0).  period_offsets [n_tapes][n_periods + 1] holds ABSOLUTE indices into the order arrays: period t of tape b
 *   owns orders [off[b][t], off[b][t + 1]).  Two tapes may point at the same orders (one tape under many parameter sets).  An offset is
 *   clamped into [0, n_orders], a decreasing pair is an empty period, an order whose asset is outside [0, n_assets) is skipped.
 *   An order takes part iff price is not NaN and > 0 and quantity is not NaN and not 0 (:185-204); it then sets board[asset] = price
 *   whether it fills or not (:298).  Buy (:56-73, :129-135): fp = price + buy_slippage, cost = q fp, com = max(cost buy_rate, min_fee),
 *   fills iff cash >= cost + com; cash -= cost + com, pos += q, entry = fp (overwritten, not averaged), trades += 1.  Sell (:74-92,
 *   :136-156): fills iff pos >= |q|; fp = price - sell_slippage, rev = |q| fp, com = max(rev sell_rate, min_fee), cash += rev - com,
 *   pos += q, wins += 1 iff rev - com > |q| entry, pos <= 1e-8 becomes 0; a sell is not counted in trades.
 *   equity[t] = cash + V (:161-171), V = the sum of pos[a] board[a] over the held assets (pos > 0) in D-22's order over a: 64 partials
 *   (partial k adds a = k, k + 64, ... from +0.0; an asset not held adds +0.0), folded p[k] += p[k + s], s = 32 .. 1.
 * params: HOST array of n_params = 1 or n_tapes entries.  benchmark: ONE device series of n_periods rows or NULL.  equity [n_tapes]
 * [n_periods]; cash the same or NULL; position [n_tapes][n_assets] (the final holdings) or NULL; counts [n_tapes][2] = trades, wins;
 * summary [n_tapes][PQ_SUMMARY_COLS] (calculate_summary of the equity row, metrics.rs:7-152) or NULL.  n_assets > 6144 (24 bytes of LDS
 * per asset and tape) is PQ_ERR_ARG and launches nothing; n_tapes = 0 or n_periods = 0 launches nothing.  Uses the context workspace for
 * the parameters when n_params > 1.  Suite recording is refused. */
typedef struct {
    double initial_capital, buy_slippage, sell_slippage, buy_commission_rate, sell_commission_rate, minimum_commission_fee;
} pq_seq_params; /* sequential.rs:232 defaults: 1e5, 0, 0, 3e-4, 3e-4, 5 */
#define PQ_SEQ_MAX_ASSETS 6144
pq_status pq_backtest_sequential(pq_ctx *, int64_t n_tapes, int64_t n_periods, int32_t n_assets, const int64_t *period_offsets,
                                 const int32_t *asset, const double *quantity, const double *price, int64_t n_orders,
                                 const double *benchmark, const pq_seq_params *params, int64_t n_params, double *equity, double *cash,
                                 double *position, int64_t *counts, double *summary);

/* ---- ParameterSweep (decision D-25 in DESIGN.md): a grid of strategy parameter sets backtested in ONE launch, one lane per parameter
 * set, one wavefront per symbol and 64 consecutive parameter sets.  lines: HOST array of n_lines device columns, each [n_series][stride]
 * like price (candidate indicator columns: every distinct moving average once, ...).  params: DEVICE table; set i trades
 *   rule 0  cross(lines[a], lines[b])  buy = a[t-1] <= b[t-1] && a[t] > b[t], sell = a[t-1] >= b[t-1] && a[t] < b[t]  (oracle/backtest.c:263-270)
 *   rule 1  band(lines[a], k0, k1)     buy = a[t-1] < k0 && a[t] >= k0,       sell = a[t-1] > k1 && a[t] <= k1        (oracle/backtest.c:271-278; b unused)
 * (a NULL or NaN compares false, row 0 never signals) through the scan of pq_backtest_vectorized (vectorized.rs:124-194: a null price
 * is a NaN, a NaN or non-positive price leaves the state untouched, quantity = floor(deploy / exec), fee = max(cost * rate, min_commission),
 * a buy that cannot afford one share is no trade) into calculate_summary (metrics.rs:7-152) in the reference's left-to-right order.
 * summary [n_series][n_params][PQ_SUMMARY_COLS] is the ONLY output: no signal, position, cash or equity value is written to memory.
 * max_drawdown, max_profit, win_rate and total_trades equal the reference bit for bit, the others up to the device pow.
 * benchmark: NULL, or one [len] series shared by all symbols (bench_series_stride = 0), or series s at benchmark + s * bench_series_stride.
 * Before anything is launched the table is copied to the host and checked (synchronises the stream): an unknown rule, a outside
 * [0, n_lines), or b outside it under rule 0 is PQ_ERR_ARG, as is n_lines outside [1, PQ_SWEEP_MAX_LINES].  n_params = 0 or n_series = 0
 * launches nothing; len = 0 writes zeros (metrics.rs:17-19).  Ragged batches and suite recording: PQ_ERR_UNSUPPORTED.  Uses the context
 * workspace for the line table.  pq_sweep_row_tile: the rows of one LDS tile for n_lines lines (0: n_lines is out of range). */
typedef struct { int32_t rule, a, b, _pad; double k0, k1; } pq_sweep_param;
#define PQ_SWEEP_MAX_LINES 512
pq_status pq_backtest_sweep(pq_ctx *, const pq_batch *, const double *price, const double *const *lines, int32_t n_lines,
                            const pq_sweep_param *params /* device */, int64_t n_params,
                            const double *benchmark, int64_t bench_series_stride /* 0: one [len] series shared by all */,
                            const pq_bt_params *bt, double *summary /* [n_series][n_params][8] */);
int32_t pq_sweep_row_tile(int32_t n_lines);
/* pq_backtest_sweep_rules: the same launch with a third column index c and every line-based rule of `Strategy`.  pq_sweep_rule has the
 * layout of pq_sweep_param with _pad read as c; col[c] is lines[c], or the price where c = -1.  Row i against row i - 1, row 0 never signals:
 *   0 PQ_SWEEP_RULE_CROSS, 1 PQ_SWEEP_RULE_BAND   as above                                  (Strategy.ma / macd; rsi / cci / reversion)
 *   2 PQ_SWEEP_RULE_CHANNEL         p = col[c], lo = lines[a], hi = lines[b]: buy = p[i] < lo[i] && p[i-1] >= lo[i-1], sell = p[i] > hi[i] &&
 *                                   p[i-1] <= hi[i-1]; both false unless all six values are non-NULL   (pq_channel_signals mode 0; bband)
 *   3 PQ_SWEEP_RULE_BREAKOUT        buy = p[i] > hi[i-1], sell = p[i] < lo[i-1]; both false if p[i], lo[i-1] or hi[i-1] is NULL
 *                                                                                            (pq_channel_signals mode 1; breakout)
 *   4 PQ_SWEEP_RULE_SCALED_CHANNEL  rule 2 with lo = lines[a] * k0, hi = lines[a] * k1 (one rounded multiply each, NULL where lines[a]
 *                                   is; b unused)                                            (pq_scale_band + pq_channel_signals mode 0; grid)
 *   5 PQ_SWEEP_RULE_CROSS_ZONES     cross(lines[a], lines[b]); buys need col[c][i] < k0, sells col[c][i] > k1   (pq_gate_signals mode 0; stoch)
 *   6 PQ_SWEEP_RULE_CROSS_STRENGTH  cross(lines[a], lines[b]); both need col[c][i] > k0                        (pq_gate_signals mode 1; adx)
 * Every rule takes the same buy / sell decision on every row as the rule kernels it names, NULL and non-NULL NaN values included (rules
 * 2-4 test the other side's columns for the NULL itself, like pq_channel_signals: a non-NULL NaN there does not refuse the signal).
 * Limits, refusals and empty shapes are pq_backtest_sweep's.  The table is checked on the host before anything is launched: rule in
 * [0, 6], a in [0, n_lines), b in [0, n_lines) under rules 0, 2, 3, 5, 6, c in [-1, n_lines) under rules 2-6; a field that a rule does not
 * use is ignored.  A table with one rule throughout runs a kernel instantiated for that rule, a mixed one the generic kernel. */
#define PQ_SWEEP_RULE_CROSS 0
#define PQ_SWEEP_RULE_BAND 1
#define PQ_SWEEP_RULE_CHANNEL 2
#define PQ_SWEEP_RULE_BREAKOUT 3
#define PQ_SWEEP_RULE_SCALED_CHANNEL 4
#define PQ_SWEEP_RULE_CROSS_ZONES 5
#define PQ_SWEEP_RULE_CROSS_STRENGTH 6
typedef struct { int32_t rule, a, b, c; double k0, k1; } pq_sweep_rule;
pq_status pq_backtest_sweep_rules(pq_ctx *, const pq_batch *, const double *price, const double *const *lines, int32_t n_lines,
                                  const pq_sweep_rule *rules /* device */, int64_t n_rules,
                                  const double *benchmark, int64_t bench_series_stride /* 0: one [len] series shared by all */,
                                  const pq_bt_params *bt, double *summary /* [n_series][n_rules][8] */);
/* ---- walk-forward windows (decision D-26 in DESIGN.md).  pq_backtest_sweep_windows: pq_backtest_sweep_rules with one more grid axis, the
 * window -- a HOST table of n_windows row ranges [t0, t1) of the same columns, which may overlap or repeat.  summary is
 * [n_windows][n_series][n_rules][8], and summary[w] is bit for bit what pq_backtest_sweep_rules writes for the rows [t0, t1) alone: the
 * scan starts flat with initial_capital at t0, row t0 never signals (row t0 - 1 of a line is never read, under rule 3 as well), the
 * number of rows in the summary is t1 - t0, the benchmark return of row t0 is taken against row t0 and alpha spans benchmark[t0] ..
 * benchmark[t1 - 1].  The lines are NOT restarted: a window of a causal indicator computed over the whole history is a warmed-up
 * indicator.  t0 == t1: that window's cells are 0 (metrics.rs:17-19).  PQ_ERR_ARG (naming the window): t0 < 0, t1 > len, t0 > t1;
 * also n_windows < 0 and a grid beyond 2^31 - 1 blocks.  n_windows = 0 writes nothing.  Everything else -- the table check, limits, ragged
 * batches, recording -- is pq_backtest_sweep_rules's; the window table is copied into the context workspace behind the line pointers.
 * pq_sweep_select: per fold f and symbol s the parameter set with the largest (maximize != 0) or smallest summary[train[f]][s][.][metric_col]
 * -- a NaN ranks last, the lowest index wins a tie, an all-NaN column gives 0 -- as chosen [n_folds][n_series], and that set's eight
 * values in the train window (in_sample) and in the test window (out_sample), both [n_folds][n_series][8].  train / test: HOST tables
 * of window indices.  PQ_ERR_ARG: metric_col outside [0, 8), an index outside [0, n_windows), n_params < 1 with n_folds n_series > 0. */
typedef struct { int64_t t0, t1; } pq_sweep_window; /* rows [t0, t1) */
pq_status pq_backtest_sweep_windows(pq_ctx *, const pq_batch *, const double *price, const double *const *lines, int32_t n_lines,
                                    const pq_sweep_rule *rules /* device */, int64_t n_rules,
                                    const pq_sweep_window *windows /* HOST */, int64_t n_windows,
                                    const double *benchmark, int64_t bench_series_stride /* 0: one [len] series shared by all */,
                                    const pq_bt_params *bt, double *summary /* [n_windows][n_series][n_rules][8] */);
pq_status pq_sweep_select(pq_ctx *, const double *summary /* [n_windows][n_series][n_params][8] */, int64_t n_windows, int64_t n_series,
                          int64_t n_params, const int32_t *train /* HOST [n_folds] */, const int32_t *test /* HOST [n_folds] */,
                          int64_t n_folds, int32_t metric_col, int32_t maximize, int32_t *chosen /* [n_folds][n_series] */,
                          double *in_sample /* [n_folds][n_series][8] */, double *out_sample /* [n_folds][n_series][8] */);

/* ---- cross-sectional factor evaluation, Factor.ic / rank_ic / rolling_ic (README.md:1429-1430,
 * :1480-1482, :1626-1634; README-only, decision D-12 in oracle/backtest.c).  factor / fwd_return: [n_series][stride];
 * per day the cross-section = symbols where both values are non-null and finite.  method 0: Pearson IC (sums over
 * blocks of 256 symbols in ascending order), 1: Spearman Rank-IC (average ranks; n_series <= 100000, n_series*len < 2^32; uses the
 * context workspace, ~52 bytes per cell).  ic: [len] (null where fewer than 2 pairs or zero variance); n_valid: [len] or NULL */
pq_status pq_factor_ic(pq_ctx *, const pq_batch *, const double *factor, const double *fwd_return, int32_t method, double *ic,
                       int32_t *n_valid);
/* rolling mean of ic over `window` rows (null unless all of them are non-null) and mean / sample std (IR) */
pq_status pq_rolling_ic(pq_ctx *, const double *ic, int64_t len, int64_t window, double *rolling_ic, double *rolling_ir);

/* ---- rank 3, continued: quantile sorts, long-short legs, turnover, coverage and IC statistics, Factor.quantile / portfolio_sorts /
 * long_short / factor_mimicking_portfolio / turnover / coverage / ir / ic_win_rate (README.md:1479-1487, :1535-1545, :1589-1599;
 * README-only, decision D-15 in DESIGN.md section 2).  factor / fwd_return: [n_series][stride], the cross-section as in D-12.  A
 * symbol whose factor value occupies the tie run [a, b) of the day's ascending sort has m = a + b; labels are uint8 [n_series][stride]
 * (the inputs' layout; NULL: not written): quantiles floor(m Q / 2n), long / short 1 (long) / 0 (short) / PQ_LABEL_MID, and
 * PQ_LABEL_OUT outside the cross-section or on a day with n < Q (quantiles) / n < 2 (long / short).  Per group and day (dense
 * [groups][len]): mean_return (sums over blocks of 256 symbols as in D-12; null where count is 0), count, turnover (new members / count;
 * null on day 0 and where either day's count is 0); spread / ls_return [len] = top group - bottom group; summary [groups + 1]
 * [PQ_GROUP_SUMMARY_COLS] = n_days, mean_return, std_return (ddof 1), sharpe (x sqrt(252)), mean_turnover over the non-null days, the
 * last row for the spread.  n_series <= 100000; above 16384, n_series * len < 2^32.  Uses the context workspace (~10 bytes per cell, ~18
 * above 16384 series). */
#define PQ_LABEL_OUT 255
#define PQ_LABEL_MID 254
#define PQ_GROUP_SUMMARY_COLS 5
/* n_quantiles in [2, 20]; mean_return / count / turnover: [n_quantiles][len]; summary: [n_quantiles + 1][5] */
pq_status pq_factor_quantiles(pq_ctx *, const pq_batch *, const double *factor, const double *fwd_return, int32_t n_quantiles,
                              uint8_t *labels, double *mean_return, int32_t *count, double *turnover, double *spread, double *summary);
/* 0 < top_pct, 0 < bottom_pct, top_pct + bottom_pct <= 1; groups 0 = short, 1 = long: mean_return / count / turnover [2][len];
 * ls_return [len] = long - short; summary [3][5] */
pq_status pq_factor_long_short(pq_ctx *, const pq_batch *, const double *factor, const double *fwd_return, double top_pct,
                               double bottom_pct, uint8_t *labels, double *mean_return, int32_t *count, double *turnover,
                               double *ls_return, double *summary);
/* coverage [len] = symbols with a non-null finite factor value / n_series */
pq_status pq_factor_coverage(pq_ctx *, const pq_batch *, const double *factor, double *coverage);
/* statistics of an IC series over its non-NaN days: out[5] = n_days, mean, std (ddof 1), ir = mean / std (not annualised),
 * win_rate = #(ic > 0) / n_days; all but n_days null below 2 days, ir null where std is 0 */
pq_status pq_ic_stats(pq_ctx *, const double *ic, int64_t len, double *out);
/* two-way (double) sort, Factor.double_sort (beyond the README; decision D-31 in DESIGN.md section 2): control (A) and factor (B) sorted
 * into n_control x n_quantiles cells, both in [2, 10]; mode 0 independent, 1 dependent (B sorted inside each control bucket).  The day's
 * sample = the symbols where control, factor and return are all non-null and finite, n its size; m of a key in a set = a + b of its tie
 * run in that set's ascending sort, as above.  la = floor(m_A Qa / 2n) over the sample; independent: lb = floor(m_B Qb / 2n) over the
 * sample, the day PQ_LABEL_OUT where n < max(Qa, Qb); dependent: the day PQ_LABEL_OUT where n < Qa, else inside control bucket a of n_a
 * members lb = floor(m_{B|a} Qb / 2 n_a) with the tie runs taken among the bucket's members, and a bucket with n_a < Qb puts its members
 * in no cell (PQ_LABEL_MID).  labels: uint8 la * Qb + lb (PQ_LABEL_OUT outside the sample), [n_series][stride], NULL: not written.  With
 * C = Qa Qb cells: mean_return / count / turnover [C][len] by the rules above; spread_factor [Qa + 1][len]: row a = mean[a][Qb - 1] -
 * mean[a][0] (null where either is), row Qa = the rows summed in ascending a from 0.0 and divided by Qa (null where any row is);
 * spread_control [Qb + 1][len]: mean[Qa - 1][b] - mean[0][b] and its average over b; summary [C + Qa + Qb + 2][5]: the cells (with
 * mean_turnover), then the spread_factor rows, then the spread_control rows (mean_turnover null).  The limits of pq_factor_quantiles;
 * uses the context workspace (~18 bytes per cell, ~26 above 16384 series, and 16 bytes per cell of the grid, day and block of 256
 * symbols).  No ragged batches, not recordable; len == 0 returns PQ_OK. */
pq_status pq_factor_double_sort(pq_ctx *, const pq_batch *, const double *control, const double *factor, const double *fwd_return,
                                int32_t n_control, int32_t n_quantiles, int32_t mode, uint8_t *labels /* NULL: not written */,
                                double *mean_return, int32_t *count, double *turnover, double *spread_factor, double *spread_control,
                                double *summary);

/* ---- rank 3, continued: the group portfolios of D-15's labels held between rebalance days, with weights, drift and a fee on the
 * traded value, Factor.portfolio_backtest (beyond the README; decision D-27 in DESIGN.md section 2).  labels: uint8 [n_series][stride]
 * (the pitch of the batch, as D-15 writes them); price / weight: f64 on the batch's pitch, weight NULL = equal weights;
 * rebalance_days d_0 < ... < d_{R-1}: a HOST array, each in [label_lag, len), copied into the context workspace.
 *   usable       a price (a weight) that is non-null, finite and > 0
 *   members      M_k(g) = the symbols with labels[s][d_k - label_lag] == g, a usable price[s][d_k] and, where weight is given, a usable
 *                weight[s][d_k]; a label >= n_groups (PQ_LABEL_MID, PQ_LABEL_OUT) belongs to no group; count[g][k] = |M_k(g)|
 *   weights      a_s = weight[s][d_k] (1.0 without weight), A_k(g) = the sum of a_s over M_k(g) in D-12's order (blocks of 256 symbols,
 *                ascending symbols inside a block from 0.0, blocks added in ascending order from 0.0), w_s = a_s / A_k(g)
 *   held price   h(s, t), t >= d_k: the price on the latest day in [d_k, t] with a usable price (a suspended stock keeps its last price)
 *   ownership    day t > d_0 belongs to the segment k with d_k < t <= d_{k+1}; the last segment runs to len - 1
 *   growth       G(g, t) = the sum over M_k(g) of w_s * (h(s, t) / price[s][d_k]) in D-12's order; 1.0 where M_k(g) is empty (cash)
 *   turnover     traded value over portfolio value, buys and sells both counted: turnover[g][k] = the sum over ALL symbols, in D-12's
 *                order, of |w_new - w_old|; w_new = w_s of rebalance k (0 for a non-member); w_old = 0 at k = 0, else for s in
 *                M_{k-1}(g) its weight drifted to d_k, w_s * (h(s, d_k) / price[s][d_{k-1}]) / G(g, d_k) (0 for a symbol not held)
 *   value        P_0 = initial_capital, P_k = B_{k-1} * G(g, d_k), B_k = P_k * (1 - cost_rate * turnover[g][k]), a sequential product
 *                over k; value[g][t] = initial_capital for t < d_0, B_k at t = d_k, B_k * G(g, t) for d_k < t <= d_{k+1}
 * Plain IEEE f64; value holds no NULL, a non-finite result stays as it is.  n_groups in [1, 20], label_lag >= 0, cost_rate in [0, 1),
 * initial_capital > 0 and finite, n_rebalance >= 0 (0: every value cell is initial_capital); len == 0 returns PQ_OK.  value:
 * [n_groups][len], turnover / count: [n_groups][n_rebalance].  No ragged batches, not recordable.  Uses the context workspace
 * (8 bytes per group, day and block of 256 symbols). */
pq_status pq_factor_portfolio(pq_ctx *, const pq_batch *, const uint8_t *labels, int32_t n_groups, int32_t label_lag,
                              const double *price, const double *weight /* NULL: equal weights */,
                              const int32_t *rebalance_days /* HOST, n_rebalance entries */, int64_t n_rebalance,
                              double cost_rate, double initial_capital,
                              double *value /* [n_groups][len] */, double *turnover /* [n_groups][n_rebalance] */,
                              int32_t *count /* [n_groups][n_rebalance] */);

/* ---- rank 3, continued: per-day factor cleaning, clean(...) (README.md:244-345; README-only, decision D-16 in DESIGN.md section 2).
 * factor / cap_z: f64 [n_series][stride], industry: int32 [n_series][stride], all on the batch's row pitch.  Per day, the cross-section is
 * every symbol with a non-null finite factor, a non-null finite cap_z (size neutralization on) and an industry code in [0, n_industries)
 * (industry neutralization on).  In the README's order: winsorize (clip to bounds from the day's cross-section), the OLS residual on cap_z
 * with an intercept, minus the mean of the symbol's industry, standardize (mean 0, sample std 1).  The log of the cap is the caller's:
 * cap_z is regressed on as given.  NULL outside the cross-section, on days with fewer than 2 members, and (standardize) on days whose std
 * is 0.  out may be factor itself (in place); cap_z and industry must not overlap out.  mad / percentile: n_series <= 100000, and above
 * 16384, n_series * len < 2^32.  Uses the context workspace (~8 bytes per cell for mad / percentile, ~16 above 16384 series, plus
 * ~10 * n_industries bytes per (day, block of 256 symbols)). */
/* D-16. winsorize: 0 none, 1 mad (winsorize_n MADs x 1.4826), 2 sigma (winsorize_n stds), 3 percentile (winsorize_n %, 0 <= p < 50);
 * cap_z / industry NULL = that neutralization off; industry codes outside [0, n_industries) are unclassified; n_industries in [1, 256];
 * standardize 0 / 1; out [n_series][stride], NULL outside the cross-section */
pq_status pq_factor_clean(pq_ctx *, const pq_batch *, const double *factor, int32_t winsorize, double winsorize_n,
                          const double *cap_z, const int32_t *industry, int32_t n_industries, int32_t standardize, double *out);

/* ---- rank 3, continued: OLS with t-tests, ic_test / factor_return / fama_macbeth / time_series_regression (README.md:1521-1600;
 * README-only, decision D-17 in DESIGN.md section 2).  Model r = a + sum_j b_j f_j, 1 <= k <= PQ_REGRESS_MAX_K.  factors is a HOST array
 * of k device pointers, each on the batch's row pitch ([n_series][stride]).  A sample is every index where the return and all k factors
 * are non-null and finite; sums over blocks of 256 indices as in D-12, centred normal equations solved by C = L D L^T in D-17's order,
 * so coef / t / R^2 / n are bit-exact; p-values (two-sided Student t) are accurate to ~1e-13 relative.  NULL (coef, t, p, R^2) where
 * n < k + 2 or a pivot D_j <= 1e-12 C[j][j]; t and p NULL where se == 0; R^2 NULL where the centred sum of squares of r is 0.  Ragged
 * batches and suite recording are refused.  Uses the context workspace (~8 (k + 1)(k + 2) / 2 bytes per (unit, block of 256)). */
#define PQ_REGRESS_MAX_K 8
#define PQ_REGRESS_SUMMARY_COLS 5 /* n_days, mean_coef, std_coef (ddof 1), t = mean / (std / sqrt(n_days)), p on n_days - 1 */
/* per-day cross-sectional regression over the symbols.  coef / t_stat / p_value: [k + 1][len] (row k = the intercept); r2 / n_obs:
 * [len]; summary (Fama-MacBeth, NULL: not written): [k + 1][PQ_REGRESS_SUMMARY_COLS] over the days with a solution */
pq_status pq_xsec_regress(pq_ctx *, const pq_batch *, const double *const *factors, int32_t k, const double *fwd_return, double *coef,
                          double *t_stat, double *p_value, double *r2, int32_t *n_obs, double *summary);
/* D-32: the weighted per-day cross-sectional regression on k factors AND n_groups industry dummies, r_i = g_ind(i) + sum_j b_j f_ij + e_i
 * minimising sum_i w_i e_i^2 -- the pure factor returns, the industry returns and the specific (residual) returns.  No separate
 * intercept (the dummies span it); group NULL puts every symbol in group 0 (n_groups must be 1), whose row is the intercept.  weight: f64
 * on the batch's row pitch, NULL = 1.0; group: int32 codes, [n_series] (group_stride 0) or [n_series][group_stride] (group_stride >=
 * len).  A day's sample: return and all k factors non-null and finite, the weight non-null, finite and > 0, the code in [0, n_groups).
 * The dummies are eliminated exactly (weighted demeaning within each industry), the k x k system is D-17's; every sum is D-12's blocked
 * sum, so coef / t / R^2 / n / resid are bit-exact (DESIGN.md D-32 has the order; with weights of 1.0 and one group the results are
 * pq_xsec_regress's bit for bit).  coef / t_stat / p_value: [k + n_groups][len], the factors, then the industries; r2: [2][len], total
 * (against the day's weighted mean return) and within (against the industry means); n_obs: the sample; n_groups_present: the industries
 * with a member; resid (NULL: not written): [n_series][stride], e on the sample's cells of solved days, NULL elsewhere; summary (NULL:
 * not written): [k + n_groups][PQ_REGRESS_SUMMARY_COLS], D-17's Fama-MacBeth row of every coefficient row.  No solution (every output
 * but n_obs and n_groups_present NULL) where a pivot is singular or n < k + n_groups_present + 1; an industry's rows are NULL on a day it
 * has no member; p on n - k - n_groups_present degrees of freedom; t and p NULL where se == 0, each R^2 where its denominator is 0.
 * len = 0 launches nothing; n_series = 0 is allowed.  Ragged batches and suite recording are refused.  Uses the context workspace (~8
 * (k + 3) n_groups bytes per day, plus at most 8 * 128 bytes (8 n_groups above 128 groups) per (day, block of 256 symbols)). */
pq_status pq_xsec_regress_wls(pq_ctx *, const pq_batch *, const double *const *factors, int32_t k, const double *fwd_return,
                              const double *weight, const int32_t *group, int64_t group_stride, int32_t n_groups, double *coef,
                              double *t_stat, double *p_value, double *r2, int32_t *n_obs, int32_t *n_groups_present, double *resid,
                              double *summary);
/* per-symbol time-series regression over the days.  Bit j of series_mask: factors[j] is one [len] series shared by every symbol (e.g. a
 * market return).  coef / t_stat / p_value: [n_series][k + 1] (column k = the intercept); r2 / n_obs: [n_series] */
pq_status pq_ts_regress(pq_ctx *, const pq_batch *, const double *const *factors, int32_t k, uint32_t series_mask, const double *ret,
                        double *coef, double *t_stat, double *p_value, double *r2, int32_t *n_obs);
/* correlation t-test: t = corr sqrt((n - 2) / (1 - corr corr)), p on n - 2; NULL where corr is NaN, n < 3 or 1 - corr^2 == 0 */
pq_status pq_corr_t_test(pq_ctx *, const double *corr, const int32_t *n_valid, int64_t len, double *t_stat, double *p_value);

/* ---- linear regression, linear(df, x_cols, y_col, pred_col, resid_col, return_stats) (README.md:165-240; README-only, decision D-24
 * in DESIGN.md section 2): ONE pooled fit y = a + sum_j b_j x_j, 1 <= k <= PQ_REGRESS_MAX_K, over all rows of the columns.  x is a HOST
 * array of k device pointers; x[j], y, pred and resid are f64 [n_series][stride] on the batch's row pitch (a flat column is n_series = 1),
 * and the logical row index is s * len + t.  A member is a row where y and all k regressors are non-null and finite.  D-17's three passes
 * and its C = L D L^T solve; the sums run over tiles of PQ_LINEAR_TILE logical rows and then over the tile partials, PQ_LINEAR_STAGE2 per
 * step, each folded in a fixed tree (D-24), so coef / t / R^2 / n / pred / resid are bit-exact and do not depend on the row pitch.
 * pred = a + sum_j b_j x_j wherever all k regressors are valid (also where y is not), resid = y - pred on the members, NULL elsewhere;
 * both may be NULL pointers together (statistics only).  coef / t_stat / p_value: [k + 1], slopes first and the intercept last, p on
 * n - k - 1 degrees of freedom; r2 = 1 - sum resid^2 / Syy; n: the members.  These scalars are ALWAYS written, an empty batch included
 * (n = 0), unlike D-17's per-unit arrays: coef, t, p, R^2 -- and every pred / resid cell -- are NULL where n < k + 2 or a pivot
 * D_j <= 1e-12 C[j][j]; t and p NULL where se == 0; R^2 NULL where Syy == 0.  Ragged batches and suite recording are refused.  Uses the
 * context workspace (~8 (k + 1)(k + 2) / 2 bytes per tile). */
#define PQ_LINEAR_TILE 4096
#define PQ_LINEAR_STAGE2 256
pq_status pq_linear(pq_ctx *, const pq_batch *, const double *const *x, int32_t k, const double *y, double *coef, double *t_stat,
                    double *p_value, double *r2, int64_t *n, double *pred, double *resid);

/* ---- rank 3, continued: multi-factor orthogonalization and neutralization, Factor().clean(factors, method) (README.md:1495-1519;
 * README-only, decision D-19 in DESIGN.md section 2).  factors is a HOST array of k device pointers, 2 <= k <= PQ_REGRESS_MAX_K, and out
 * a HOST array of k - 1, all on the batch's row pitch.  Per day, the sample is every symbol whose k factors are all non-null and finite.
 * out[j] (j = 0 .. k - 2) is the residual of factors[j + 1]: mode 0 (orthogonalize, sequential Gram-Schmidt) on factors[0 .. j], mode
 * 1 (neutralize) on factors[0] alone, each with an intercept and bit-identical to the e of pq_xsec_regress's D-17 order (one
 * C = L D L^T per day serves every level).  NULL outside the sample and where D-17 would NULL that regression's coefficients
 * (n < regressors + 2 or a singular pivot; in mode 0 a singular block NULLs every later residual).  out[j] may be factors[j + 1] (in
 * place).  Ragged batches and suite recording are refused.  Uses the context workspace (~4 k (k + 1) bytes per (day, block of 256)). */
pq_status pq_factor_orthogonalize(pq_ctx *, const pq_batch *, const double *const *factors, int32_t k, int32_t mode, double *const *out);

/* ---- rank 3, continued: IC decay, sub-period and sub-group robustness tests, ic_decay / subsample_test / subgroup_test
 * (README.md:1556-1565, :1607-1624; README-only, decision D-18 in DESIGN.md section 2).  factor / fwd_return: [n_series][stride]; the
 * cross-section, the blocked sums (Pearson) and the average ranks (Rank-IC) are D-12's, so every daily IC is bit-identical to
 * pq_factor_ic on the shifted or masked inputs.  method 0 Pearson IC, 1 Spearman Rank-IC (n_series <= 100000).  summary rows
 * [PQ_IC_SUMMARY_COLS] = n_days, mean, std (ddof 1), t = mean / (std / sqrt(n_days)), p on n_days - 1 over the non-null days, as
 * pq_xsec_regress's Fama-MacBeth summary.  Ragged batches and suite recording are refused.  Use the context workspace (Pearson ~24 bytes
 * per (row, day, block of 256 symbols); Rank-IC ~8 bytes per cell, ~12 for sub-groups). */
#define PQ_IC_DECAY_MAX_LAG 256
#define PQ_IC_MAX_GROUPS 256
#define PQ_IC_SUMMARY_COLS 5
/* IC decay: row l - 1 (l = 1 .. max_lag) is the IC of the factor of day t against the return of day t + l - 1, NULL with n_valid 0 for
 * t > len - l.  ic / n_valid: [max_lag][len]; summary: [max_lag][PQ_IC_SUMMARY_COLS] */
pq_status pq_ic_decay(pq_ctx *, const pq_batch *, const double *factor, const double *fwd_return, int32_t method, int32_t max_lag,
                      double *ic, int32_t *n_valid, double *summary);
/* sub-group IC: row g is the IC over the day's cross-section restricted to the symbols whose code is g.  group: int32 codes, [n_series]
 * (group_stride 0) or [n_series][group_stride] (group_stride >= len); codes outside [0, n_groups) are unclassified; n_groups in [1, 256].
 * ic / n_valid: [n_groups][len]; summary: [n_groups][PQ_IC_SUMMARY_COLS] */
pq_status pq_ic_subgroup(pq_ctx *, const pq_batch *, const double *factor, const double *fwd_return, const int32_t *group,
                         int64_t group_stride, int32_t n_groups, int32_t method, double *ic, int32_t *n_valid, double *summary);
/* sub-period summaries of a series x [len]: the periods are numpy.array_split(range(len), n_splits) (contiguous, the first len % n_splits
 * one day longer), 1 <= n_splits <= len; summary: [n_splits][PQ_IC_SUMMARY_COLS] */
pq_status pq_series_split_summary(pq_ctx *, const double *x, int64_t len, int32_t n_splits, double *summary);

/* ---- rank 3, continued: the general factor calculations, Factor.rank / normalize / weighted / ratio / diff (README.md:1416-1421,
 * :1438-1470; README-only, decision D-20 in DESIGN.md section 2).  Every column is f64 [n_series][stride] on the batch's row pitch, and
 * so is out, which may be one of the inputs (in place).  "Valid" is non-null and finite.  Ragged batches and suite recording are refused;
 * n_series = 0 or len = 0 launches nothing.  Normalize's zscore is pq_factor_clean(winsorize 0, standardize 1). */
/* Factor.rank and normalize("quantile") (README.md:1420-1421, :1456-1460).  Per day over the n valid symbols: a symbol whose key (-0 ties
 * with +0) occupies the tie run [a, b) of the ascending sort has rank = ((a + 1) + b) / 2; descending: n + 1 - rank.  mode 0: that rank,
 * 1: rank / n (pct), 2: (rank - 0.5) / n, the mid-rank position in (0, 1) (descending must be 0).  NULL outside the sample.
 * n_series <= 100000; above 16384, n_series * len < 2^32.  Uses the context workspace (~8 bytes per cell, ~16 above 16384 series). */
pq_status pq_factor_rank(pq_ctx *, const pq_batch *, const double *factor, int32_t mode, int32_t descending, double *out);
/* normalize("minmax") (README.md:1420, :1454-1456): (x - min) / (max - min) over the day's valid symbols, -0 read as +0; the whole day
 * NULL where max == min.  Uses the context workspace (~16 bytes per (day, block of 256 symbols)). */
pq_status pq_factor_minmax(pq_ctx *, const pq_batch *, const double *factor, double *out);
/* Factor.weighted (README.md:1419, :1449-1451): (x w) / W per day over the symbols whose factor and weight are both valid and (group not
 * NULL) whose code lies in [0, n_groups); W = the sum of w over the day's sample, or over the symbol's group on that day, in D-12's
 * blocked order (blocks of 256 symbols, ascending from 0.0, block sums in ascending order).  group: int32 codes, [n_series]
 * (group_stride 0) or [n_series][group_stride] (group_stride >= len); n_groups in [1, 256].  NULL outside the sample and where W == 0.
 * Uses the context workspace (~8 * max(n_groups, 1) bytes per (day, block of 256 symbols)). */
pq_status pq_factor_weighted(pq_ctx *, const pq_batch *, const double *factor, const double *weight, const int32_t *group,
                             int64_t group_stride, int32_t n_groups, double *out);
/* Factor.ratio / diff (README.md:1417-1418, :1441-1447): op 0: a / b, 1: a - b, 2: (a - b) / |b|.  NULL where either input is NULL,
 * otherwise plain IEEE-754 (a zero divisor gives inf or NaN). */
pq_status pq_factor_binary(pq_ctx *, const pq_batch *, const double *a, const double *b, int32_t op, double *out);

/* ---- rank 3, continued: the common technical factors, Factor.moving_average / momentum / volatility / skewness / relative_strength
 * (README.md:1423-1426, :1472-1477; README-only, decision D-21 in DESIGN.md section 2).  x: f64 [n_series][stride], usually a price; out:
 * f64 [n_series][stride] on the same pitch.  Everything runs along the days of one symbol.  valid(j): 0 <= j and x[j] non-null and
 * finite; r[j] = (x[j] - x[j-1]) / x[j-1] and d[j] = x[j] - x[j-1] where j-1 and j are valid; w = window; every sum starts at 0.0 and adds
 * in ascending j.
 *   op 0 mean:              valid(t-w+1 .. t): (sum of x[j]) / w
 *   op 1 momentum:          valid(t-skip) and valid(t-skip-w): (a - b) / b, a = x[t-skip], b = x[t-skip-w]
 *   op 2 volatility:        valid(t-w .. t) and r[t-w+1 .. t] finite, w >= 2: m = (sum r) / w, sqrt((sum (r-m)(r-m)) / (w-1))
 *   op 3 skewness:          the same sample, w >= 3: e = r-m, m2 = (sum e e) / w, m3 = (sum (e e) e) / w, m3 / (m2 sqrt(m2)); NULL at m2 == 0
 *   op 4 relative strength: valid(t-w .. t): G = sum of the d[j] > 0, L = sum of -d[j] over the d[j] < 0, (100 G) / (G + L); NULL at G + L == 0
 * A row whose sample is incomplete is NULL, and so is a result that comes out NaN (+-inf passes).  1 <= window <= 1024 and at least the
 * op's minimum; skip >= 0, and 0 except for momentum; anything else is PQ_ERR_ARG.  out must NOT overlap x (PQ_ERR_ARG): unlike the
 * elementwise calls above, a workgroup reads a halo of days that another workgroup writes.  Ragged batches and suite recording are
 * refused; n_series = 0 or len = 0 launches nothing.  No workspace. */
#define PQ_FACTOR_ROLLING_MAX_WINDOW 1024
/* op 0 mean, 1 momentum, 2 volatility, 3 skewness, 4 relative strength (decision D-21) */
pq_status pq_factor_rolling(pq_ctx *, const pq_batch *, const double *x, int32_t op, int64_t window, int64_t skip, double *out);

/* ---- rank 3, continued: rolling-window OLS, Factor.rolling_regression / rolling_beta / idiosyncratic_volatility (the README computes
 * one whole-history beta to the market with `linear`, README.md:231; one value per (symbol, day) is decision D-28 in DESIGN.md section
 * 2).  Model y = a + sum_j b_j x_j over the days t-w+1 .. t of one symbol, w = window, K = n_x, 1 <= K <= PQ_ROLLING_REGRESS_MAX_K.  x is
 * a HOST array of K device pointers; y and x[j] are f64 [n_series][stride] on the batch's row pitch, except that bit j of series_mask
 * makes x[j] one [len] series shared by every symbol (e.g. a market return), as in pq_ts_regress.  A row has a result only if
 * t >= w - 1 and all K + 1 values are non-null and finite on every day of its window (D-21's rule; no min_periods).  The arithmetic is
 * D-17's with n = w, every sum a plain sum over the window in ascending day order from 0.0, evaluated directly (no sliding sums), so
 * every output is bit-exact: the K + 1 means; the centred products and C = L D L^T in D-17's order with its singular rule (a pivot
 * D_j <= 1e-12 C[j][j], a NaN pivot, anything behind one); alpha = ybar - sum_j b_j xbar_j; e = d_y - sum_j b_j d_j, sse = sum e e.
 *   beta      [n_x][n_series][stride]   b_j
 *   alpha     [n_series][stride]        a
 *   resid_std [n_series][stride]        sqrt(sse / (w - K - 1))
 *   r_squared [n_series][stride]        1 - sse / Syy; NULL where Syy == 0 (the other outputs stay)
 *   resid     [n_series][stride]        the e of the window's last day t
 * Each output may be a NULL pointer: it is not written.  A row without its sample, with a singular window or with a result that comes
 * out NaN is NULL in every output.  K + 2 <= window <= PQ_FACTOR_ROLLING_MAX_WINDOW, n_x outside 1 .. 4, a series_mask bit beyond n_x,
 * a ragged batch, and an output that overlaps an input or another output (a workgroup reads a halo of days that another workgroup
 * writes) are PQ_ERR_ARG; suite recording is refused (PQ_ERR_UNSUPPORTED); n_series = 0 or len = 0 launches nothing.  No workspace. */
#define PQ_ROLLING_REGRESS_MAX_K 4
pq_status pq_factor_rolling_regress(pq_ctx *, const pq_batch *, const double *const *x, int32_t n_x, uint32_t series_mask,
                                    const double *y, int64_t window, double *beta /* [n_x][n_series][stride] */, double *alpha,
                                    double *resid_std, double *r_squared, double *resid);

/* ---- rank 3, continued: the time-series operators of factor construction, Factor.ts_sum / ts_std / ts_zscore / ts_min / ts_max /
 * ts_argmin / ts_argmax / ts_rank / decay_linear / delay / delta and ts_cov / ts_corr (beyond the README: the windowed operators that
 * formulaic alphas are written in; decision D-29 in DESIGN.md section 2).  x, y: f64 [n_series][stride]; out: f64 [n_series][stride] on
 * the same pitch.  Everything runs along the days of one symbol.  w = window, dw = (double)w; win[0 .. w) = x[t-w+1 .. t], oldest to
 * newest; D-21's rule: a row is NULL unless t >= w - 1 and every value of its window is non-null and finite; every sum starts at 0.0
 * and adds in ascending k, evaluated directly (no sliding sums), so every output is bit-exact.
 *   op 0 sum:           sum of win[k]
 *   op 1 std:           w >= 2: mean = sum / dw, q2 = sum of (win[k] - mean)^2, sqrt(q2 / (w - 1))   (volatility's order)
 *   op 2 zscore:        w >= 2: (win[w-1] - mean) / std; NULL at q2 == 0
 *   op 3 min, 4 max:    the window's extreme (of equal extremes the oldest: -0 ties with +0)
 *   op 5 argmin, 6 argmax: the 0-based offset of the extreme from the window's OLDEST day, 0 .. w-1, as f64; compares are < and >, so
 *                       ties go to the oldest day (numpy.argmin / argmax of the window)
 *   op 7 rank:          of win[w-1] within the window: (2 #less + #equal + 1) / 2 with #equal counting the day itself, compares < and
 *                       ==; mode 0: that rank in 1 .. w, mode 1: the rank / dw
 *   op 8 decay_linear:  (sum of (k + 1) win[k]) / (w (w + 1) / 2)
 *   op 9 delay:         x[t-w] where t >= w and it is non-null and not NaN (+-inf passes), else NULL
 *   op 10 delta:        x[t] - x[t-w] where t >= w and both are non-null and finite, else NULL
 * A result that comes out NaN is NULL (+-inf passes).  1 <= window <= PQ_FACTOR_ROLLING_MAX_WINDOW and at least the op's minimum; mode
 * is rank's alone, 0 for every other op; anything else is PQ_ERR_ARG.  out must NOT overlap x (PQ_ERR_ARG): a workgroup reads a halo of
 * days that another workgroup writes.  Ragged batches and suite recording are refused; n_series = 0 or len = 0 launches nothing.  No
 * workspace. */
pq_status pq_factor_ts(pq_ctx *, const pq_batch *, const double *x, int32_t op, int64_t window, int32_t mode, double *out);
/* the two-column operators on the same sample rule applied to both columns: mx = (sum x) / dw, my = (sum y) / dw, then in one ascending
 * pass sxy = sum (x - mx)(y - my), sxx = sum (x - mx)^2, syy = sum (y - my)^2.
 *   op 0 cov:   sxy / (w - 1)
 *   op 1 corr:  sxy / (sqrt(sxx) sqrt(syy)); NULL at sxx == 0 or syy == 0
 * 2 <= window <= PQ_FACTOR_ROLLING_MAX_WINDOW; out must overlap neither x nor y; otherwise as pq_factor_ts. */
pq_status pq_factor_ts_pair(pq_ctx *, const pq_batch *, const double *x, const double *y, int32_t op, int64_t window, double *out);

/* ---- rank 3, continued: K tested factors into one composite score, Factor.combine (beyond the README: the step between the factor
 * tests and portfolio_backtest; decision D-30 in DESIGN.md section 2).
 * Weights: ic is a DEVICE array [k][len], row j the IC series of factor j (pq_factor_ic's), 1 <= k <= PQ_REGRESS_MAX_K; weights [k][len].
 * w = window; the window of day t is the days t-lag-w+1 .. t-lag, so with lag >= 1 a weight never sees the IC of its own day.  Row t is
 * NULL in all k weights unless the whole window lies in [0, len) and all k w values are non-NULL (pq_rolling_ic's rule, across the
 * factors).  Every sum starts at 0.0 and adds the window in ascending day order, evaluated directly.
 *   method 0 PQ_COMBINE_IC:       w_j = m_j = (sum ic_j) / w                                                   w >= 1
 *   method 1 PQ_COMBINE_ICIR:     w_j = m_j / sd_j, sd_j = sqrt((sum (ic_j - m_j)^2) / (w - 1)); the row NULL unless every sd_j > 0    w >= 2
 *   method 2 PQ_COMBINE_MAX_ICIR: w = C^-1 m, C[j][l] = (sum (ic_j - m_j)(ic_l - m_l)) / (w - 1), solved as C = L D L^T in D-17's order
 *                                 without an intercept; the row NULL where a pivot D_j <= 1e-12 C[j][j]         w >= k + 1
 * A weight that comes out NaN makes the row NULL.  Methods 0 and 1 are pq_rolling_ic(ic_j, w)'s rolling_ic and rolling_ir read at day
 * t - lag, bit for bit.  window <= PQ_FACTOR_ROLLING_MAX_WINDOW, 0 <= lag <= PQ_FACTOR_ROLLING_MAX_WINDOW; k, method, window or lag out
 * of range, a null pointer and weights overlapping ic are PQ_ERR_ARG; suite recording is refused; len = 0 launches nothing.
 * Composite: factors is a HOST array of k device pointers, each [n_series][stride] on the batch's row pitch, as out; weights is the
 * DEVICE array [k][len].  Per cell acc = sum_j weights[j][t] * factors[j][s][t] (j ascending from 0.0, product and sum rounded
 * separately); normalize != 0 stores acc / D[t], D[t] = sum_j |weights[j][t]| (j ascending from 0.0), normalize == 0 stores acc.  NULL
 * unless all k cells are non-null and finite (D-19's common sample), and where a weight of the day is NULL or NaN, where normalize is
 * set and D[t] == 0, and where the result is NaN.  The factors are taken as given: standardise them first.  k out of range, a null
 * pointer and out overlapping a factor or the weights are PQ_ERR_ARG; ragged batches and suite recording are refused
 * (PQ_ERR_UNSUPPORTED); n_series = 0 or len = 0 launches nothing.  No workspace. */
#define PQ_COMBINE_IC 0
#define PQ_COMBINE_ICIR 1
#define PQ_COMBINE_MAX_ICIR 2
pq_status pq_factor_combine_weights(pq_ctx *, const double *ic /* device [k][len] */, int32_t k, int64_t len, int32_t method,
                                    int64_t window, int64_t lag, double *weights /* [k][len] */);
pq_status pq_factor_combine(pq_ctx *, const pq_batch *, const double *const *factors, int32_t k, const double *weights /* device [k][len] */,
                            int32_t normalize, double *out);

/* ---- rank 3, continued: the risk model on the series of pq_xsec_regress_wls, Factor.risk_model / Factor.portfolio_risk (beyond the
 * README; decision D-33 in DESIGN.md section 2).  Everything is evaluated on `count` AS-OF days t_d = day0 + d * step, d = 0 .. count - 1
 * (day0 >= 0, step >= 1, count >= 0, day0 + (count - 1) * step < len, else PQ_ERR_ARG); the model of day t reads the rows t-w+1 .. t of its
 * inputs and nothing later.
 * The one arithmetic, rk_wcov(a, b) of two windows a[0 .. w), b[0 .. w) (oldest to newest) under the weights omega[0 .. w) (omega[w-1]
 * weights the as-of day): the sample P is every k whose day t-w+1+k >= 0, whose a[k] and b[k] are both non-null and finite and whose
 * omega[k] > 0; n = |P|.  Over P in ascending k from 0.0, every product rounded before it is added: W = sum omega, W2 = sum (omega omega),
 * Sa = sum (omega a), Sb = sum (omega b), ma = Sa / W, mb = Sb / W, C = sum (omega (a - ma)) (b - mb).  cov = C / (W - W2 / W) when
 * unbiased (reliability weights; n - 1 for equal weights), C / W otherwise.  NULL where n < min_periods, where unbiased and n < 2, where
 * the denominator is not > 0 and where the result is NaN (+-inf passes).  With every omega 1.0, unbiased, min_periods = w and a full
 * window this is pq_factor_ts_pair's op 0 bit for bit; doubling every omega changes no bit; cov(a, b) and cov(b, a) are bit-identical where omega (a - ma) is exact (equal weights) and may
 * differ in the last bit otherwise, which is why the matrix is written from one evaluation per unordered pair.
 * omega is a DEVICE array of `window` doubles that the entry points do not read (finite, >= 0 and not all 0 is the caller's to check).
 * 1 <= window <= PQ_FACTOR_ROLLING_MAX_WINDOW, 1 <= min_periods <= window, min_periods >= 2 when unbiased; a null required pointer and an
 * output that overlaps an input or another output are PQ_ERR_ARG; ragged batches and suite recording are refused (PQ_ERR_UNSUPPORTED);
 * count = 0, len = 0 or n_series = 0 launches nothing.  No workspace.
 *   pq_risk_factor_cov:   the batch is the M = n_series series [M][stride] (D-32's coef block), 1 <= M <= PQ_RISK_MAX_SERIES.  cov_out
 *                         [count][M][M]: entry [d][j][l], l <= j, is rk_wcov(f_j, f_l), mirrored to [d][l][j] (one evaluation per unordered
 *                         pair: exactly symmetric).  n_out (NULL: not written) [count][M]: the n of the diagonal.
 *   pq_risk_specific_var: the batch is [n_series][stride]; var_out[s * out_stride + d] = rk_wcov(x_s, x_s), out_stride >= count; n_out
 *                         (NULL: not written) on the same layout. */
#define PQ_RISK_MAX_SERIES (PQ_REGRESS_MAX_K + PQ_IC_MAX_GROUPS)
pq_status pq_risk_factor_cov(pq_ctx *, const pq_batch *, const double *f, const double *omega /* device [window] */, int64_t window,
                             int64_t min_periods, int32_t unbiased, int64_t day0, int64_t step, int64_t count,
                             double *cov_out /* [count][M][M] */, int32_t *n_out /* [count][M] */);
pq_status pq_risk_specific_var(pq_ctx *, const pq_batch *, const double *x, const double *omega /* device [window] */, int64_t window,
                               int64_t min_periods, int32_t unbiased, int64_t day0, int64_t step, int64_t count, double *var_out,
                               int64_t out_stride, int32_t *n_out);
/* The predicted risk of the holdings [n_series][stride] on the as-of days.  exposures is a HOST array of 0 <= k <= PQ_REGRESS_MAX_K device
 * pointers on the batch's row pitch; industry / group_stride / n_groups = G are pq_xsec_regress_wls's (NULL: G = 1 and every symbol in
 * group 0, so row k is the net weight); cov [count][M][M] with M = k + G and specific_var [n_series][sv_stride] (sv_stride >= count) are
 * the two calls' outputs, indexed by d.  Per as-of day: the held set H is every symbol whose holding h is non-null, finite and != 0;
 * a held symbol is UNCOVERED where an exposure is null or not finite, a given code lies outside [0, G), or its specific variance is not
 * >= 0 (NULL, NaN or negative).  n_out [2][count]: |H| and the uncovered count.  With |H| = 0 or anything uncovered every f64 output of
 * the day is NULL.  X[j] = sum_H (h x_j), X[k + g] = sum over H in g of h, S = sum_H (h h) s^2, each D-12's blocked sum (blocks of 256 symbol
 * indices, ascending from 0.0, block sums in ascending order).  For every row j with X[j] != 0: v_j = sum_l cov[j][l] X[l] over ascending l
 * with X[l] != 0 from 0.0, c_j = X[j] v_j; c_j = 0.0 where X[j] == 0; a NULL cov[j][l] that a sum needs makes the day NULL.  factor_var =
 * sum_j c_j (ascending from 0.0), total = factor_var + S, vol = sqrt(total), NULL where total < 0 (pairwise-complete covariances need
 * not be positive semi-definite).  A value that comes out NaN is NULL.  exposure_out / contribution_out: [M][count]; risk_out
 * [4][count]: factor_var, specific_var, total_var, volatility.  k, n_groups, group_stride, sv_stride or the as-of days out of range and a
 * null pointer are PQ_ERR_ARG; ragged batches and suite recording are refused; count = 0 launches nothing.  Uses the context workspace
 * (~8 (M + 1) bytes per (as-of day, block of 256 symbols)). */
pq_status pq_risk_portfolio(pq_ctx *, const pq_batch *, const double *holdings, const double *const *exposures, int32_t k,
                            const int32_t *industry, int64_t group_stride, int32_t n_groups, const double *cov, const double *specific_var,
                            int64_t sv_stride, int64_t day0, int64_t step, int64_t count, double *exposure_out, double *contribution_out,
                            double *risk_out, int32_t *n_out);
/* Portfolio construction from the risk model (api.risk_solve, Factor.optimal_portfolio; decision D-34 in DESIGN.md section 2): on every
 * as-of day y_r = Sigma^-1 v_r for n_rhs = R right-hand sides at once, Sigma = B F B^T + diag(s^2) (never built), and the matrix
 * v_r^T Sigma^-1 v_q.  rhs is a HOST array of 1 <= R <= PQ_RISK_SOLVE_MAX_RHS device pointers [n_series][stride] on the batch's pitch,
 * read at day t_d; a NULL entry is the vector of ones.  exposures / k, industry / group_stride / n_groups = G, cov [count][M][M] (M = k + G),
 * specific_var / sv_stride and the as-of days are pq_risk_portfolio's; 1 <= M <= PQ_RISK_SOLVE_MAX_M (a larger M: PQ_ERR_UNSUPPORTED).
 * The universe U of a day: every given rhs non-null and finite, every exposure non-null and finite, a given code in [0, G), and s^2 > 0
 * (NULL, NaN, zero or negative fails).  n_out [2][count]: |U|, and the symbols whose rhs are all valid but that fail another condition
 * (uncovered): such a symbol is outside U and its y is NULL, the day goes on.  With q_i = 1.0 / s^2_i, every product rounded before it is
 * added and every sum D-12's blocked sum (blocks of 256 symbol indices, ascending from 0.0, block sums in ascending order):
 * A[j][l] = sum_U (q x_j) x_l for l <= j < k, mirrored; A[k+g][j] = A[j][k+g] = sum over U in g of q x_j; A[k+g][k+g] = sum over U in g
 * of q; other industry-industry entries exactly 0.0; p_r[j] = sum_U (q x_j) v_r, p_r[k+g] = sum over U in g of q v_r.  Active rows
 * J = {j: A[j][j] > 0} ascending (an industry without a member, a factor that is 0 on all of U take no part); a NULL cov[j][l] with j and l
 * in J makes the day NULL, one outside does not.  Compacted to m = |J|: S[a][b] = sum_c F[a][c] A[c][b] over ascending c from 0.0, then
 * + 1.0 on the diagonal; c_r[a] = sum_c F[a][c] p_r[c]: (I + F A) u = F p, which needs neither F^-1 nor a positive semi-definite F.
 * In-place LU with partial pivoting on [S | c_0 .. c_{R-1}]: at column c the pivot is the first row >= c with the largest |S[.][c]| (a NaN
 * never displaces an entry), swapped in; for i > c: mu = S[i][c] / S[c][c], S[i][l] = S[i][l] - mu S[c][l] for l > c and on every rhs;
 * then u[a] = (c[a] - sum_{b>a} S[a][b] u[b]) / S[a][a], the sum over ascending b from 0.0.  A pivot that is 0, NaN or infinite, a u that
 * is not finite and |U| = 0 make the day NULL.  For i in U: y_r,i = q_i (v_r,i - e), e = sum over j < k in J of x_ij u_r[j] (ascending
 * from 0.0), then + u_r[k + g_i].  y is NULL outside U and on NULL days; a NaN result is NULL.  y_out: a HOST array of R device pointers
 * [n_series][out_stride], out_stride >= count, indexed by d (specific_var's layout).  quad_out [R][R][count]: entry [r][q], q <= r, is the
 * blocked sum over U of v_r y_q, mirrored to [q][r] (one evaluation per unordered pair: exactly symmetric), NULL on NULL days.
 * PQ_ERR_ARG: a null required pointer, k, n_rhs, n_groups, group_stride, sv_stride, out_stride or the as-of days out of range, an output
 * that overlaps an input or another output; ragged batches and suite recording are refused (PQ_ERR_UNSUPPORTED); count = 0, len = 0 or
 * n_series = 0 launches nothing.  Uses the context workspace (block partials of at most k (k + 1) / 2 + k R + 128 cells per (as-of day,
 * block of 256 symbols), and (1 + k + R) G + R M cells per as-of day). */
#define PQ_RISK_SOLVE_MAX_RHS 4
#define PQ_RISK_SOLVE_MAX_M 128
pq_status pq_risk_solve(pq_ctx *, const pq_batch *, const double *const *rhs, int32_t n_rhs, const double *const *exposures, int32_t k,
                        const int32_t *industry, int64_t group_stride, int32_t n_groups, const double *cov, const double *specific_var,
                        int64_t sv_stride, int64_t day0, int64_t step, int64_t count, double *const *y_out, int64_t out_stride,
                        double *quad_out, int32_t *n_out);

/* ---- rank 3, continued: the backtest of GIVEN target weights, signed and with cash (api.factor_weights, Factor.weights_backtest; decision
 * D-35 in DESIGN.md section 2): what pq_risk_solve's y_out / Factor.optimal_portfolio's weights, a composite's or the caller's own weights
 * would have earned, for P = n_portfolios portfolios at once (the price plane is read once for all of them).  Everything not said here is
 * pq_factor_portfolio's: usable, the held price h(s, t), the ownership of days, the chain.  weights: a HOST array of P device pointers
 * [n_series][w_stride], column k = rebalance k (pq_risk_solve's y_out layout), w_stride >= n_rebalance; price on the batch's pitch;
 * rebalance_days d_0 < ... < d_{R-1}: a HOST array, each in [0, len).  Every sum is D-12's blocked sum (blocks of 256 symbols, ascending
 * from 0.0, block sums ascending from 0.0), every product is rounded before it is added.  For portfolio p and rebalance k:
 *   target       w = weights[p][s][k] non-null, finite and != 0.0 (NULL, NaN and +-inf are silently not held: NULL is what D-34 writes
 *                outside its universe)
 *   member       a target whose price[s][d_k] is usable: M_k; a target without one is DROPPED: counted, it contributes nothing and its
 *                weight stays in cash.  count [3][P][R]: members with w > 0, members with w < 0, dropped
 *   exposure     [2][P][R]: net W_k = sum over M_k of w, gross = sum over M_k of |w|; cash c_k = 1.0 - W_k (negative under leverage)
 *   growth       for d_k < t <= d_{k+1} (the last segment runs to len - 1): L = sum over M_k of w * (h(s, t) / price[s][d_k]),
 *                G(p, t) = c_k + L; an empty M_k gives L = 0.0 and G = 1.0
 *   turnover     [P][R]: the sum over ALL symbols of |w_new - w_old|; w_new = the member's w, 0.0 for a non-member; w_old = 0.0 at k = 0,
 *                else for s in M_{k-1}: (w * (h(s, d_k) / price[s][d_{k-1}])) / G(p, d_k), 0.0 for a symbol not held.  The cash leg is
 *                not counted
 *   value        [P][len]: P_0 = initial_capital, P_k = B_{k-1} * G(p, d_k), B_k = P_k * (1 - cost_rate * turnover[p][k]); value[p][t] =
 *                initial_capital for t < d_0, B_k at t = d_k, B_k * G(p, t) for d_k < t <= d_{k+1}.  Plain IEEE f64, no NULL is written;
 *                a non-finite or negative result stays as it is
 *   first_nonpositive [P]: the smallest t whose value[p][t] is not > 0.0 (<= 0 or NaN), -1 if there is none: a signed, levered book can
 *                be ruined, and the curve after that day means nothing
 *   holdings     of portfolio holdings_of, holdings_out[s][t] on the batch's pitch (what pq_risk_portfolio reads): 0.0 for t < d_0 and for
 *                a non-member; at t = d_k the member's w itself; for d_k < t < d_{k+1} (to len - 1 in the last segment)
 *                (w * (h(s, t) / price[s][d_k])) / G(p, t)
 * With 2^m members, clean prices and equal weights 1 / 2^m, W_k is exactly 1.0, c_k exactly 0.0 and value and turnover are
 * pq_factor_portfolio's (one group, equal weights) bit for bit.  1 <= P <= PQ_WEIGHTS_MAX_PORTFOLIOS, cost_rate in [0, 1), initial_capital
 * > 0 and finite, holdings_of in [-1, P) and set exactly when holdings_out is; a null required pointer and an output that overlaps an
 * input or another output are PQ_ERR_ARG; ragged batches and suite recording are refused (PQ_ERR_UNSUPPORTED); len == 0 or n_series == 0
 * returns PQ_OK with nothing launched; n_rebalance == 0 gives every value cell initial_capital, first_nonpositive -1 and holdings 0.0.
 * Uses the context workspace (8 bytes per portfolio, day and block of 256 symbols). */
#define PQ_WEIGHTS_MAX_PORTFOLIOS 8
pq_status pq_factor_weights(pq_ctx *, const pq_batch *, const double *const *weights, int32_t n_portfolios, int64_t w_stride,
                            const double *price, const int32_t *rebalance_days /* HOST, n_rebalance entries */, int64_t n_rebalance,
                            double cost_rate, double initial_capital, double *value /* [P][len] */, double *turnover /* [P][R] */,
                            double *exposure /* [2][P][R]: net, gross */, int32_t *count /* [3][P][R]: long, short, dropped */,
                            int32_t *first_nonpositive /* [P] */, int32_t holdings_of /* portfolio index, or -1 */,
                            double *holdings_out /* [n_series][stride], or NULL */);

/* ---- rank 3, continued: the return attribution of holdings through the factor model (api.return_attribution, Factor.return_attribution;
 * decision D-36 in DESIGN.md section 2): how much of every day's return of a book came from each style factor, each industry and the
 * specific returns of pq_xsec_regress_wls (D-32), and how much the model cannot see.  Where something is not said here, pq_risk_portfolio's
 * rules hold.  holdings [n_series][stride] on the batch's pitch (what pq_factor_weights writes); benchmark_holdings optional, same layout;
 * exposures a HOST array of 0 <= k <= PQ_REGRESS_MAX_K device pointers; industry / group_stride / n_groups = G are pq_xsec_regress_wls's
 * (NULL: G = 1, every symbol in group 0); factor_return [M][fr_stride], M = k + G, fr_stride >= len: the k style rows, then the G industry
 * rows or the intercept (D-32's coef block); specific_return [n_series][stride] (D-32's resid); next_return optional, same layout.  The
 * call covers EVERY day t in [0, len).
 *   books        P = 1: the holdings h.  With a benchmark b, P = 3: h, b and the active book a, a_i = h_i - b_i per symbol, where a holding
 *                that is NULL or not finite counts as 0.0.  A symbol is HELD in a book when its value there is non-null, finite and != 0.0
 *   covered      every exposure non-null and finite, a given code in [0, G), specific_return[s][t] non-null and finite: membership of
 *                D-32's sample of the day.  A held symbol that is not covered is UNCOVERED -- the day goes on --, and MISSING when
 *                next_return is also absent or not valid there.  n_out [3][P][len]: held, uncovered, missing
 *   sums         each D-12's blocked sum (blocks of 256 symbol indices ascending from 0.0, block sums ascending from 0.0), every product
 *                rounded before it is added: X[j] = sum over covered of h x_j, X[k + g] = sum over covered in g of h, spec = sum over
 *                covered of h u, unexplained = sum over uncovered with a valid r of h r, realized = sum over held with a valid r of h r
 *   contribution c_j = X[j] f_j(t) where X[j] != 0 and 0.0 where X[j] == 0 (D-32 writes NULL for an empty industry: it does not matter);
 *                a NULL or non-finite f_j(t) with X[j] != 0 and a day on which nothing is held make every f64 output of the book's day NULL
 *   outputs      exposure_out / contribution_out [P][M][len]; totals_out [P][6][len]: style = sum_{j<k} c_j and industry = sum_g c_{k+g}
 *                (each ascending from 0.0), specific, unexplained, total = ((style + industry) + specific) + unexplained, and realized
 *                (NULL without next_return).  A value that comes out NaN is NULL
 *   aggregates   the series of a book are its M contribution rows, then its 6 totals.  summary_out [P][M + 6][5]: pq_xsec_regress's
 *                Fama-MacBeth row (n_days, mean, std, t_stat, p_value) over the series' non-NULL days.  With period_bounds, a HOST array
 *                of n_periods + 1 day indices strictly ascending in [0, len] (period k = the days [bounds[k], bounds[k + 1])):
 *                period_sum_out [P][M + 6][S], the sum over the period's non-NULL days ascending from 0.0, and period_days_out [P][S], the
 *                period's days whose total is not NULL.  The sums are arithmetic, not geometrically linked
 * On a day without uncovered symbols total equals realized up to rounding; doubling the holdings doubles every f64 output bit for bit.
 * PQ_ERR_ARG: a null required pointer, k, n_groups, group_stride, fr_stride or the bounds out of range, period_bounds without n_periods
 * > 0 or the reverse, an output that overlaps an input or another output; ragged batches and suite recording are refused
 * (PQ_ERR_UNSUPPORTED); len == 0 or n_series == 0 launches nothing.  Uses the context workspace (8 P (M + 3) + 12 P bytes per (day, block
 * of 256 symbols)). */
#define PQ_ATTRIBUTION_TOTALS 6
pq_status pq_return_attribution(pq_ctx *, const pq_batch *, const double *holdings, const double *benchmark_holdings /* or NULL */,
                                const double *const *exposures, int32_t k, const int32_t *industry, int64_t group_stride, int32_t n_groups,
                                const double *factor_return /* [M][fr_stride] */, int64_t fr_stride, const double *specific_return,
                                const double *next_return /* or NULL */, const int64_t *period_bounds /* HOST, n_periods + 1, or NULL */,
                                int64_t n_periods, double *exposure_out /* [P][M][len] */, double *contribution_out /* [P][M][len] */,
                                double *totals_out /* [P][6][len] */, int32_t *n_out /* [3][P][len] */,
                                double *summary_out /* [P][M + 6][5] */, double *period_sum_out /* [P][M + 6][S], or NULL */,
                                int32_t *period_days_out /* [P][S], or NULL */);

/* ---- suites: record many calls, replay them as a few chip-filling grids ----
 * One indicator over N symbols is only N/64 wavefronts -- far too few for 256 CUs -- but a DataFrame query asks
 * for many indicators at once (df.with_columns([...]) in the reference; Polars then calls the plugin once per
 * expression and group).  Between pq_suite_begin and pq_suite_end every pq_* compute call on `ctx` is RECORDED
 * instead of launched (same batch shape for all; pointers must stay valid for the suite's lifetime);
 * pq_suite_run replays the whole set: per dependency phase ONE grid runs all sequential jobs
 * (blockIdx.y = job) and the row-parallel launches follow.  Results are bit-identical to the direct calls. */
typedef struct pq_suite pq_suite;
pq_status pq_suite_begin(pq_ctx *ctx, const pq_batch *b);
pq_status pq_suite_end(pq_ctx *ctx, pq_suite **out);
pq_status pq_suite_abort(pq_ctx *ctx);
pq_status pq_suite_run(pq_ctx *ctx, pq_suite *suite);
pq_status pq_suite_destroy(pq_ctx *ctx, pq_suite *suite);
pq_status pq_suite_info(const pq_suite *suite, int32_t *n_phases, int32_t *n_seq_jobs, int32_t *n_row_launches);
/* measurement: HIP events around every sequential-job grid, on the stream it is launched on */
pq_status pq_suite_set_timing(pq_suite *suite, int32_t on);
pq_status pq_suite_grid_stats(pq_suite *suite, int32_t grid, double *avg_ms, double *algorithmic_bytes, int32_t *n_jobs,
                              int32_t *lds_bytes, int32_t *runs);
/* which kernel a grid launches: 0 = seq_jobs_kernel<0> (tiled bodies), 1 = seq_jobs_kernel<1> (register-heavy ops),
 * 2 = seq_jobs_kernel<2> (gather bodies) */
pq_status pq_suite_grid_variant(pq_suite *suite, int32_t grid, int32_t *variant);
/* the launches of one kernel overlap inside a step: mean (latest end - earliest start) over the grids launching kernel
 * `variant`, and the sum of their algorithmic bytes */
pq_status pq_suite_span_stats(pq_suite *suite, int32_t variant, double *avg_span_ms, double *algorithmic_bytes);

#ifdef __cplusplus
}
#endif
#endif
