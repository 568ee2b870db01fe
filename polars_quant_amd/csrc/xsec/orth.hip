// xsec/orth.hip -- multi-factor orthogonalization and neutralization, Factor.clean(factors, method) (README.md:1495-1519; README-only
// => decision D-19).
//
// Columns are symbol-major [n_series][stride]; a day's cross-section is a strided column.  The sample of a day is every symbol whose K
// factors are all non-null and finite.  orthogonalize: e_k (k = 1 .. K-1) is D-17's residual of f_k on f_0 .. f_{k-1} with an
// intercept (sequential Gram-Schmidt); neutralize: e_k is D-17's residual of f_k on f_0 alone.  The last level of orthogonalize(K) is
// regress(K - 1) with r = f_{K-1}; the combine, the means, the factorization and the substitutions are D-17's own code, in xsec_ols.h:
//  1. passes:  one thread per (day, block of 256 symbols), consecutive threads on consecutive days (coalesced), sums its block in
//              ascending symbol order from 0.0, members only: pass 1 n and sum f_j; pass 2 the centred cross-products C[j][m]
//              (m <= j; neutralize: column 0 only).  This file's own kernel, as regress.hip has its own (xsec_ols.h says why).
//  2. combine: one thread per day adds the block sums in ascending block order from 0.0 (xo_combine, xo_means_kernel).  After pass 2
//              it factorises C = L D L^T once by rows (xo_ldl; prefix-consistent: the leading k x k block is what D-17 factorises for
//              k regressors) and solves the K - 1 nested systems, level k on row k of the triangle by xo_forward then xo_back as
//              D-17 solves on its row K (neutralize: b = C[k][0] / C[0][0]).
//  3. write:   the pass body once more: e = (f_k - fbar_k) - fit, fit = 0.0; fit += b_j (f_j - fbar_j) for ascending j.  A thread reads
//              all K inputs of a symbol before it writes that symbol's residuals, so out[j] may be factors[j + 1].
// Every operation is D-17's, in its order (restated in tests/xsec_orth_ref.py), so the residuals are bit-identical to the e of D-17's pass 3.
#include "xsec_ols.h"

namespace {

enum OrPass { OR_P1 = 1, OR_P2 = 2, OR_P3 = 3 };

template <int K, bool NEUT> struct OrNa {
    static constexpr int P1 = K;                               // sum f_j
    static constexpr int P2 = NEUT ? K : K * (K + 1) / 2;      // C[j][0] (neutralize) or C[j][m], m <= j, at j (j + 1) / 2 + m
    static constexpr int NB = NEUT ? K - 1 : K * (K - 1) / 2;  // coefficients: level k at k - 1 (neutralize) or k (k - 1) / 2 + j
};

struct OrIn {
    const double *f[XO_MAX_K];
    double *out[XO_MAX_K - 1];
    Dims d;
};

// per-day state: [rows][len] rows
struct OrDay {
    int32_t *n;
    int32_t *nok;      // levels 1 .. nok have a solution (residuals written); the rest are NULL
    double *mean;      // [K]: fbar_0 .. fbar_{K-1}
    double *b;         // [NB]
};

__device__ __forceinline__ int or_boff(bool neut, int k) { return neut ? k - 1 : k * (k - 1) / 2; }

template <int K, bool NEUT, int P>
__global__ __launch_bounds__(64) void or_pass_kernel(OrIn in, OrDay day, double *ps, int32_t *pcnt) {
    constexpr int NA = P == OR_P1 ? OrNa<K, NEUT>::P1 : (P == OR_P2 ? OrNa<K, NEUT>::P2 : 1);
    constexpr int NB = OrNa<K, NEUT>::NB;
    const Dims d = in.d;
    const int64_t units = d.len;
    const int64_t u = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (u >= units) return;
    double fbar[K], b[NB > 0 ? NB : 1];
    int nok = 0;
#pragma unroll
    for (int j = 0; j < K; j++) fbar[j] = 0.0;
    if (P >= OR_P2) {
#pragma unroll
        for (int j = 0; j < K; j++) fbar[j] = day.mean[(int64_t)j * units + u];
    }
    if (P == OR_P3) {
        nok = day.nok[u];
#pragma unroll
        for (int q = 0; q < NB; q++) b[q] = day.b[(int64_t)q * units + u];
    }
    double acc[NA];
#pragma unroll
    for (int q = 0; q < NA; q++) acc[q] = 0.0;
    int cnt = 0;
    const int64_t i_lo = (int64_t)blockIdx.y * XS_BLOCK, i_hi = i_lo + XS_BLOCK < d.n ? i_lo + XS_BLOCK : d.n;
    constexpr int B = xo_ahead(K);
    for (int64_t i0 = i_lo; i0 < i_hi; i0 += B) {
        double fv[B][K];
#pragma unroll
        for (int k = 0; k < B; k++) {
            const int64_t i = i0 + k < i_hi ? i0 + k : i_hi - 1;
            const int64_t o = i * d.stride + u;
#pragma unroll
            for (int j = 0; j < K; j++) fv[k][j] = in.f[j][o];
        }
#pragma unroll
        for (int k = 0; k < B; k++) {
            if (i0 + k >= i_hi) break;
            bool mem = true;
#pragma unroll
            for (int j = 0; j < K; j++) mem = mem && xs_valid(fv[k][j]);
            if (P == OR_P3) {
                const int64_t o = (i0 + k) * d.stride + u;
                double df[K];
#pragma unroll
                for (int j = 0; j < K; j++) df[j] = fv[k][j] - fbar[j];
#pragma unroll
                for (int l = 1; l < K; l++) {
                    double fit = 0.0;
                    if (NEUT) {
                        fit += b[l - 1] * df[0];
                    } else {
#pragma unroll
                        for (int j = 0; j < l; j++) fit += b[l * (l - 1) / 2 + j] * df[j];
                    }
                    const double e = df[l] - fit;
                    in.out[l - 1][o] = mem && l <= nok ? e : pq_null();
                }
                continue;
            }
            if (!mem) continue;
            cnt += 1;
            if (P == OR_P1) {
#pragma unroll
                for (int j = 0; j < K; j++) acc[j] += fv[k][j];
                continue;
            }
            double df[K];
#pragma unroll
            for (int j = 0; j < K; j++) df[j] = fv[k][j] - fbar[j];
            if (NEUT) {
#pragma unroll
                for (int j = 0; j < K; j++) acc[j] += df[j] * df[0];
            } else {
#pragma unroll
                for (int j = 0; j < K; j++)
#pragma unroll
                    for (int m = 0; m <= j; m++) acc[j * (j + 1) / 2 + m] += df[j] * df[m];
            }
        }
    }
    if (P == OR_P3) return;
#pragma unroll
    for (int q = 0; q < NA; q++) ps[((int64_t)blockIdx.y * NA + q) * units + u] = acc[q];
    if (P == OR_P1) pcnt[(int64_t)blockIdx.y * units + u] = cnt;
}

// after pass 2: the coefficients of every level.  orthogonalize: C[0:K-1, 0:K-1] = L D L^T by rows once; level k (regressors
// f_0 .. f_{k-1}) is solved on the leading k x k block as D-17 solves it: z_m = c_m - sum_{i < m} L[m][i] z_i, then
// b_j = z_j / D_j - sum_{m > j} L[m][j] b_m (sums ascending from 0.0), c = C[k][0:k].  It has a solution while n >= k + 2 and every pivot
// D_j (j < k) > 1e-12 C[j][j].  neutralize: level k is D-17 at one regressor, b = C[k][0] / C[0][0], solved while n >= 3 and
// C[0][0] > 1e-12 C[0][0].
template <int K, bool NEUT>
__global__ __launch_bounds__(64) void or_solve_kernel(const double *ps, int64_t nblk, int64_t units, OrDay day) {
    const int64_t u = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (u >= units) return;
    constexpr int NA = OrNa<K, NEUT>::P2;
    double s[NA];
    xo_combine<NA>(ps, nblk, units, u, s);
    const int32_t n = day.n[u];
    if (NEUT) {
        const bool ok = n >= 3 && s[0] > XO_SINGULAR * s[0];
        day.nok[u] = ok ? K - 1 : 0;
#pragma unroll
        for (int k = 1; k < K; k++) day.b[(int64_t)(k - 1) * units + u] = s[k] / s[0];
        return;
    }
    constexpr int R = K - 1;   // regressor rows: f_{K-1} is never a regressor
    double L[R][R], D[R];
    const int npiv = xo_ldl<R>(s, L, D), nok = npiv < n - 2 ? npiv : n - 2;   // level k also needs n >= k + 2
    day.nok[u] = nok > 0 ? nok : 0;
#pragma unroll
    for (int k = 1; k < K; k++) {
        double z[R], b[R];
        xo_forward<R>(L, s + xo_tri(k), k, z);   // row k of the triangle, as D-17 solves on its row K
        xo_back<R>(L, D, z, k, b);
#pragma unroll
        for (int j = 0; j < k; j++) day.b[(int64_t)(k * (k - 1) / 2 + j) * units + u] = b[j];
    }
}

template <int K, bool NEUT>
pq_status or_run(pq_ctx *ctx, const OrIn &in) {
    const Dims d = in.d;
    const int64_t units = d.len;
    const int64_t nblk = xs_nblk(d.n);
    XoWs w;
    PQ_TRY(xo_workspace(ctx, "factor orthogonalization", units, nblk, K, K + OrNa<K, NEUT>::NB, OrNa<K, NEUT>::P2, &w));   // own rows: b [NB]
    const OrDay day{w.n, w.flag, w.mean, w.own};
    double *ps = w.ps;
    int32_t *pc = w.pcnt;
    const dim3 gp((unsigned)((units + 63) / 64), (unsigned)nblk), gu((unsigned)((units + 63) / 64));
    hipStream_t st = ctx->stream;
    hipLaunchKernelGGL((or_pass_kernel<K, NEUT, OR_P1>), gp, dim3(64), 0, st, in, day, ps, pc);
    hipLaunchKernelGGL(xo_means_kernel<K>, gu, dim3(64), 0, st, (const double *)ps, (const int32_t *)pc, nblk, units, day.n, day.mean);
    hipLaunchKernelGGL((or_pass_kernel<K, NEUT, OR_P2>), gp, dim3(64), 0, st, in, day, ps, pc);
    hipLaunchKernelGGL((or_solve_kernel<K, NEUT>), gu, dim3(64), 0, st, (const double *)ps, nblk, units, day);
    hipLaunchKernelGGL((or_pass_kernel<K, NEUT, OR_P3>), gp, dim3(64), 0, st, in, day, ps, pc);
    PQ_HIP_TRY(hipGetLastError());
    return PQ_OK;
}

template <bool NEUT>
pq_status or_dispatch(pq_ctx *ctx, int k, const OrIn &in) {
    switch (k) {
    case 2: return or_run<2, NEUT>(ctx, in);
    case 3: return or_run<3, NEUT>(ctx, in);
    case 4: return or_run<4, NEUT>(ctx, in);
    case 5: return or_run<5, NEUT>(ctx, in);
    case 6: return or_run<6, NEUT>(ctx, in);
    case 7: return or_run<7, NEUT>(ctx, in);
    default: return or_run<8, NEUT>(ctx, in);
    }
}

} // namespace

extern "C" {

pq_status pq_factor_orthogonalize(pq_ctx *ctx, const pq_batch *b, const double *const *factors, int32_t k, int32_t mode,
                                  double *const *out) {
    const char *what = "pq_factor_orthogonalize";
    PQ_TRY(pq_check(ctx, b));
    if (k < 2 || k > XO_MAX_K) { pq_set_error("%s: k must be in [2, 8]", what); return PQ_ERR_ARG; }
    if (mode != 0 && mode != 1) { pq_set_error("%s: mode must be 0 (orthogonalize) or 1 (neutralize)", what); return PQ_ERR_ARG; }
    if (ctx->rec) { pq_set_error("%s cannot be recorded into a suite", what); return PQ_ERR_UNSUPPORTED; }
    if (b->offsets) { pq_set_error("%s: ragged batches are not supported", what); return PQ_ERR_UNSUPPORTED; }
    if (b->n_series == 0 || b->len == 0) return PQ_OK;
    if (!factors || !out) { pq_set_error("%s: null pointer", what); return PQ_ERR_ARG; }
    OrIn in{};
    in.d = dims_of(b);
    for (int j = 0; j < k; j++) {
        if (!factors[j]) { pq_set_error("%s: null factor pointer", what); return PQ_ERR_ARG; }
        in.f[j] = factors[j];
    }
    for (int j = 0; j < k - 1; j++) {
        if (!out[j]) { pq_set_error("%s: null output pointer", what); return PQ_ERR_ARG; }
        in.out[j] = out[j];
    }
    return mode == 1 ? or_dispatch<true>(ctx, k, in) : or_dispatch<false>(ctx, k, in);
}

} // extern "C"
