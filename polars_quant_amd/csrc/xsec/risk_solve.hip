// xsec/risk_solve.hip -- y = Sigma^-1 v under the factor risk model of D-33, Sigma = B F B^T + diag(s^2), on every as-of day and for up to four
// right-hand sides at once, with the small matrix v_r^T Sigma^-1 v_q (api.risk_solve, Factor.optimal_portfolio); decision D-34, DESIGN.md
// section 2.  Sigma is never built: with q_i = 1 / s^2_i, A = B^T diag(q) B and p = B^T diag(q) v (one pass over the symbols),
// (I + F A) u = F p is an M x M system per day (M = K + G; it needs neither F^-1 nor a positive semi-definite F), and
// y_i = q_i (v_i - b_i^T u) is one more pass (Woodbury).
//  1. moments: 64 lanes = 64 consecutive as-of days, blockIdx.y = the block of 256 symbols (risk.hip's portfolio pass 1, wls.hip's pass 1).
//              The sums without an industry index -- the triangle (q x_j) x_l and (q x_j) v_r -- sit in registers under static indices
//              (guarded unrolled loops); the per-industry columns q, q x_j, q v_r sit [column][g][lane] in LDS and run over chunks of
//              rs_chunk columns where all of them do not fit (wls.hip's rule); the registers and the counts belong to the first chunk.
//              Block partials go to the workspace, one thread per (day, cell) adds them in ascending block order from 0.0 (D-12).
//  2. solve:   one workgroup per as-of day.  The day's moments are staged in LDS in their structure (K x K, K x G, G: the industry block of
//              A is diagonal), the active rows J compacted, [S | c] = [I + F A | F p] built in dynamic LDS, then LU with partial pivoting:
//              per column wave 0 finds the pivot, swaps the row permutation (no row moves) and divides the multipliers, all threads update
//              the trailing block; two barriers per column.  Back substitution: one wave per right-hand side, its lane 0 in series (the
//              sum of row a starts with the u just computed, so the order of D-34 leaves nothing to share out).
//  3. output:  pass 1's shape again: y along d (coalesced), and the block partials of v_r y_q for q <= r; one thread per (day, pair) adds
//              them and mirrors the entry.
// The operation order is D-34's, restated in tests/xsec_solve_ref.py.
#include "xsec_window.h"

namespace {

constexpr int RS_MAX_K = PQ_REGRESS_MAX_K;
constexpr int RS_MAX_R = PQ_RISK_SOLVE_MAX_RHS;
constexpr int RS_MAX_M = PQ_RISK_SOLVE_MAX_M;
constexpr int RS_TRI = RS_MAX_K * (RS_MAX_K + 1) / 2;
constexpr int RS_PAIRS = RS_MAX_R * (RS_MAX_R + 1) / 2;
constexpr int RS_LDS_CELLS = 128;    // (column, industry) pairs of [64]-lane f64 accumulators per moments workgroup: 64 KiB (wls.hip's WL_LDS_CELLS)
constexpr int RS_THREADS = 256;      // the solve's workgroup: four waves, one per right-hand side in the back substitution
static_assert(RS_THREADS / 64 >= RS_MAX_R, "one wave per right-hand side");

// columns of the moments pass per chunk: as many of the ncol as keep chunk * G within RS_LDS_CELLS, at least one (wl_chunk's rule; G <= 128 here)
inline int rs_chunk(int ncol, int G) {
    const int c = RS_LDS_CELLS / G;
    return c < 1 ? 1 : (c > ncol ? ncol : c);
}
__host__ __device__ __forceinline__ constexpr int rs_tri(int j) { return j * (j + 1) / 2; }

struct RsIn {
    const double *v[RS_MAX_R];   // null: the vector of ones
    const double *x[RS_MAX_K];
    int32_t R, K;
    XsGroups grp;                // null codes: every symbol in group 0 (G = 1)
    const double *sv;            // [n_series][sv_stride], by as-of day
    int64_t sv_stride;
    Dims d;
    RkDays a;
};

// one symbol of one as-of day: its cells, and whether it is in the universe U or uncovered
struct RsCell {
    double v[RS_MAX_R], x[RS_MAX_K], s2;
    int32_t g;
    bool given, in_u;            // every given rhs valid; and covered
    __device__ __forceinline__ void load(const RsIn &in, int64_t s, int64_t t, int64_t dd) {
        const int64_t o = s * in.d.stride + t;
#pragma unroll
        for (int r = 0; r < RS_MAX_R; r++) v[r] = r < in.R && in.v[r] ? in.v[r][o] : 1.0;
#pragma unroll
        for (int j = 0; j < RS_MAX_K; j++) x[j] = j < in.K ? in.x[j][o] : 0.0;
        s2 = in.sv[s * in.sv_stride + dd];
        g = in.grp.codes ? in.grp.at(s, t) : 0;
        given = true;
#pragma unroll
        for (int r = 0; r < RS_MAX_R; r++) given = given && xs_valid(v[r]);
        bool cov = s2 > 0.0 && in.grp.has(g);                   // a NULL (or NaN) variance fails the compare
#pragma unroll
        for (int j = 0; j < RS_MAX_K; j++) cov = cov && xs_valid(x[j]);
        in_u = given && cov;
    }
};

// ---------------------------------------------------------------- 1. moments
// The cells of a day: [0, tri(K)) the triangle (q x_j) x_l at tri(j) + l, then K R cells (q x_j) v_r at j R + r (together NT), then the
// 1 + K + R industry columns q | q x_j | q v_r, G cells each.  This launch: the columns [c0, c1); FIRST also the NT register cells and the
// counts.  Block partials ps[block][(FIRST ? NT : 0) + (c1 - c0) G][count], counts pc[block][2][count] (|U|, uncovered).
template <bool FIRST>
__global__ __launch_bounds__(64) void rs_moments_kernel(RsIn in, int c0, int c1, double *ps, int32_t *pc) {
    extern __shared__ __align__(16) unsigned char rs_lds[];
    double *acc = (double *)rs_lds;
    const int lane = threadIdx.x;
    const int64_t D = in.a.count, dd = (int64_t)blockIdx.x * 64 + lane;
    if (dd >= D) return;
    const int K = in.K, R = in.R, G = in.grp.G, nq = (c1 - c0) * G, NT = rs_tri(K) + K * R;
    for (int q = 0; q < nq; q++) acc[q * 64 + lane] = 0.0;
    double tri[FIRST ? RS_TRI : 1], pr[FIRST ? RS_MAX_K * RS_MAX_R : 1];
    if (FIRST) {
#pragma unroll
        for (int q = 0; q < RS_TRI; q++) tri[q] = 0.0;
#pragma unroll
        for (int q = 0; q < RS_MAX_K * RS_MAX_R; q++) pr[q] = 0.0;
    }
    const int64_t t = in.a.day0 + dd * in.a.step;
    const int64_t s_lo = (int64_t)blockIdx.y * XS_BLOCK, s_hi = s_lo + XS_BLOCK < in.d.n ? s_lo + XS_BLOCK : in.d.n;
    int32_t nu = 0, nx = 0;
    for (int64_t s = s_lo; s < s_hi; s++) {
        RsCell c;
        c.load(in, s, t, dd);
        if (!c.given) continue;
        if (!c.in_u) { nx++; continue; }
        nu++;
        const double q = 1.0 / c.s2;
        double qx[RS_MAX_K];
#pragma unroll
        for (int j = 0; j < RS_MAX_K; j++) qx[j] = q * c.x[j];
        if (FIRST) {
#pragma unroll
            for (int j = 0; j < RS_MAX_K; j++) {
                if (j >= K) continue;
#pragma unroll
                for (int l = 0; l <= j; l++) tri[rs_tri(j) + l] += qx[j] * c.x[l];
#pragma unroll
                for (int r = 0; r < RS_MAX_R; r++)
                    if (r < R) pr[j * RS_MAX_R + r] += qx[j] * c.v[r];
            }
        }
#pragma unroll
        for (int col = 0; col < 1 + RS_MAX_K + RS_MAX_R; col++) {
            // column `col` of the widest layout is q (0), q x_j (1 + j) or q v_r (1 + RS_MAX_K + r); its place among this call's 1 + K + R
            const int at = col <= RS_MAX_K ? col : col - RS_MAX_K + K;
            if ((col > K && col <= RS_MAX_K) || col - 1 - RS_MAX_K >= R || at < c0 || at >= c1) continue;
            const double val = col == 0 ? q : (col <= RS_MAX_K ? qx[col >= 1 ? col - 1 : 0] : q * c.v[col > RS_MAX_K ? col - 1 - RS_MAX_K : 0]);
            acc[((at - c0) * G + c.g) * 64 + lane] += val;
        }
    }
    const int nreg = FIRST ? NT : 0, np = nreg + nq;
    double *out = ps + ((int64_t)blockIdx.y * np) * D + dd;
    if (FIRST) {
#pragma unroll
        for (int j = 0; j < RS_MAX_K; j++) {
            if (j >= K) continue;
#pragma unroll
            for (int l = 0; l <= j; l++) out[(int64_t)(rs_tri(j) + l) * D] = tri[rs_tri(j) + l];
#pragma unroll
            for (int r = 0; r < RS_MAX_R; r++)
                if (r < R) out[(int64_t)(rs_tri(K) + j * R + r) * D] = pr[j * RS_MAX_R + r];
        }
        pc[((int64_t)blockIdx.y * 2 + 0) * D + dd] = nu;
        pc[((int64_t)blockIdx.y * 2 + 1) * D + dd] = nx;
    }
    for (int q = 0; q < nq; q++) out[(int64_t)(nreg + q) * D] = acc[q * 64 + lane];
}

// one thread per (as-of day, cell q of a launch's np): the block sums in ascending block order from 0.0 -> mom[cell][count], the first
// nreg cells to themselves and the others behind cell `base`; with pc, cell 0's threads also add the counts -> n_out[2][count]
__global__ __launch_bounds__(64) void rs_sum_kernel(const double *ps, const int32_t *pc, int64_t nblk, int64_t D, int np, int nreg, int base,
                                                    double *mom, int32_t *n_out) {
    const int64_t dd = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const int q = blockIdx.y;
    if (dd >= D) return;
    if (q < np) {
        double s = 0.0;
        for (int64_t k = 0; k < nblk; k++) s += ps[(k * np + q) * D + dd];
        mom[(int64_t)(q < nreg ? q : base + q - nreg) * D + dd] = s;
    }
    if (q == 0 && pc) {
        int32_t nu = 0, nx = 0;
        for (int64_t k = 0; k < nblk; k++) {
            nu += pc[(k * 2 + 0) * D + dd];
            nx += pc[(k * 2 + 1) * D + dd];
        }
        n_out[dd] = nu;
        n_out[D + dd] = nx;
    }
}

// ---------------------------------------------------------------- 2. solve
struct RsSolve {
    const double *mom, *cov;
    const int32_t *n_out;
    int64_t D;
    int32_t K, G, R;
    double *u;      // [R][M][count]: u_r on the rows of J, 0.0 on the others
    int32_t *ok;    // [count]: 0 on a NULL day
};

// the day's A in its structure: kk [K][K] (mirrored), kg [K][G], gg [G] (the diagonal of the industry block, whose other entries are 0.0)
struct RsA {
    const double *kk, *kg, *gg;
    int K, G;
    __device__ __forceinline__ double diag(int j) const { return j < K ? kk[j * K + j] : gg[j - K]; }
    __device__ __forceinline__ double at(int c, int b) const {
        if (c < K) return b < K ? kk[c * K + b] : kg[c * G + b - K];
        return b < K ? kg[b * G + c - K] : (c == b ? gg[c - K] : 0.0);
    }
};

// dynamic LDS (host: rs_solve_lds): S [M][M + R] | kk | kg | gg | p [R][M] (later u on all M rows) | J [M] | perm [M] | st [4]: m and the
// NULL flags of the day's inputs (nothing in U, a missing covariance), of a pivot and of a non-finite u
inline size_t rs_solve_lds(int K, int G, int R) {
    const size_t M = (size_t)(K + G);
    return (M * (M + R) + (size_t)K * K + (size_t)K * G + G + (size_t)R * M) * 8 + (2 * M + 4) * 4;
}

__global__ __launch_bounds__(RS_THREADS) void rs_solve_kernel(RsSolve a) {
    extern __shared__ __align__(16) unsigned char rs_lds[];
    const int tid = threadIdx.x, K = a.K, G = a.G, R = a.R, M = K + G, NT = rs_tri(K) + K * R;
    const int64_t D = a.D, dd = blockIdx.x;
    double *S = (double *)rs_lds, *kk = S + M * (M + R), *kg = kk + K * K, *gg = kg + K * G, *P = gg + G;
    int *J = (int *)(P + R * M), *perm = J + M, *st = perm + M;
    const double *mom = a.mom + dd;                             // cell q of the day: mom[q * D]
    for (int e = tid; e < K * K; e += RS_THREADS) {
        const int j = e / K, l = e - j * K;
        kk[e] = mom[(int64_t)(j >= l ? rs_tri(j) + l : rs_tri(l) + j) * D];
    }
    for (int e = tid; e < K * G; e += RS_THREADS) kg[e] = mom[(int64_t)(NT + G + e) * D];
    for (int e = tid; e < G; e += RS_THREADS) gg[e] = mom[(int64_t)(NT + e) * D];
    for (int e = tid; e < R * M; e += RS_THREADS) {
        const int r = e / M, j = e - r * M;
        P[e] = mom[(int64_t)(j < K ? rs_tri(K) + j * R + r : NT + (1 + K + r) * G + j - K) * D];
    }
    __syncthreads();
    const RsA A{kk, kg, gg, K, G};
    if (tid == 0) {
        int m = 0;
        for (int j = 0; j < M; j++)
            if (A.diag(j) > 0.0) { J[m] = j; perm[m] = m; m++; }
        st[0] = m;
        st[1] = a.n_out[dd] == 0;
        st[2] = st[3] = 0;
    }
    __syncthreads();
    const int m = st[0], W = m + R;
    // [S | c]: row a of the compacted system, over the active c in ascending order from 0.0
    const double *F = a.cov + dd * M * M;
    bool missing = false;
    for (int e = tid; e < m * W; e += RS_THREADS) {
        const int ia = e / W, ib = e - ia * W;
        const double *row = F + (int64_t)J[ia] * M;
        double s = 0.0;
        if (ib < m) {
            const int jb = J[ib];
            for (int c = 0; c < m; c++) {
                const int jc = J[c];
                const double f = row[jc];
                missing = missing || pq_isnull(f);
                s += f * A.at(jc, jb);
            }
            if (ia == ib) s = s + 1.0;
        } else {
            const double *p = P + (ib - m) * M;
            for (int c = 0; c < m; c++) {
                const int jc = J[c];
                const double f = row[jc];
                missing = missing || pq_isnull(f);
                s += f * p[jc];
            }
        }
        S[e] = s;
    }
    if (missing) st[1] = 1;                                     // (every writer stores the same 1)
    __syncthreads();
    // st[1] is final here; st[2] is written by wave 0 before a column's first barrier and read behind it only
    for (int c = 0; c < m && !st[1]; c++) {
        if (tid < 64) {
            // the first position >= c with the largest |S[.][c]|; a NaN never displaces another entry, and a NaN at position c stays
            double best = -2.0;
            int bi = c;
            for (int i = c + tid; i < m; i += 64) {
                const double v = fabs(S[perm[i] * W + c]), key = v == v ? v : -1.0;
                if (key > best) { best = key; bi = i; }
            }
            for (int o = 32; o > 0; o >>= 1) {
                const double ob = __shfl_xor(best, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
            }
            const int pc_ = perm[c];
            const double own = S[pc_ * W + c];
            if (own != own) bi = c;
            const int pp = perm[bi];
            const double piv = S[pp * W + c];
            const bool bad = !(piv != 0.0 && isfinite(piv));
            for (int i = c + 1 + tid; i < m && !bad; i += 64) {
                const int row = i == bi ? pc_ : perm[i];        // the permutation after the swap
                S[row * W + c] = S[row * W + c] / piv;
            }
            if (tid == 0) {
                perm[c] = pp;
                perm[bi] = pc_;
                if (bad) st[2] = 1;
            }
        }
        __syncthreads();
        if (st[2]) break;
        const int prow = perm[c], nr = m - c - 1, nc = W - c - 1;
        for (int e = tid; e < nr * nc; e += RS_THREADS) {
            const int i = e / nc, l = c + 1 + e - i * nc, row = perm[c + 1 + i];
            S[row * W + l] = S[row * W + l] - S[row * W + c] * S[prow * W + l];
        }
        __syncthreads();
    }
    // back substitution, one wave per rhs: u over the rhs column
    if (!st[1] && !st[2] && (tid & 63) == 0 && (tid >> 6) < R) {
        const int col = m + (tid >> 6);
        bool finite = true;
        for (int ia = m - 1; ia >= 0; ia--) {
            const int row = perm[ia];
            double s = 0.0;
            for (int b = ia + 1; b < m; b++) s += S[row * W + b] * S[perm[b] * W + col];
            const double u = (S[row * W + col] - s) / S[row * W + ia];
            finite = finite && isfinite(u);
            S[row * W + col] = u;
        }
        if (!finite) st[3] = 1;
    }
    for (int e = tid; e < R * M; e += RS_THREADS) P[e] = 0.0;
    __syncthreads();
    const bool ok = !(st[1] | st[2] | st[3]);
    for (int e = tid; e < R * m && ok; e += RS_THREADS) {
        const int r = e / m, ia = e - r * m;
        P[r * M + J[ia]] = S[perm[ia] * W + m + r];
    }
    __syncthreads();
    for (int e = tid; e < R * M; e += RS_THREADS) a.u[(int64_t)e * D + dd] = P[e];
    if (tid == 0) a.ok[dd] = ok ? 1 : 0;
}

// ---------------------------------------------------------------- 3. output
struct RsOut {
    double *y[RS_MAX_R];
    int64_t stride;
};

// y_r,i = q_i (v_r,i - e) on the universe of a solved day, NULL elsewhere; block partials pq[block][pair tri(r) + q][count] of v_r y_q
__global__ __launch_bounds__(64) void rs_output_kernel(RsIn in, const double *mom, const double *u, const int32_t *okf, RsOut out, double *pq) {
    const int lane = threadIdx.x;
    const int64_t D = in.a.count, dd = (int64_t)blockIdx.x * 64 + lane;
    if (dd >= D) return;
    const int K = in.K, R = in.R, M = K + in.grp.G;
    const bool ok = okf[dd] != 0;
    double uk[RS_MAX_K][RS_MAX_R], acc[RS_PAIRS];
    bool act[RS_MAX_K];
#pragma unroll
    for (int j = 0; j < RS_MAX_K; j++) {
        act[j] = j < K && mom[(int64_t)(rs_tri(j) + j) * D + dd] > 0.0;
#pragma unroll
        for (int r = 0; r < RS_MAX_R; r++) uk[j][r] = ok && act[j] && r < R ? u[((int64_t)r * M + j) * D + dd] : 0.0;
    }
#pragma unroll
    for (int p = 0; p < RS_PAIRS; p++) acc[p] = 0.0;
    const int64_t t = in.a.day0 + dd * in.a.step;
    const int64_t s_lo = (int64_t)blockIdx.y * XS_BLOCK, s_hi = s_lo + XS_BLOCK < in.d.n ? s_lo + XS_BLOCK : in.d.n;
    for (int64_t s = s_lo; s < s_hi; s++) {
        RsCell c;
        c.load(in, s, t, dd);
        const bool live = ok && c.in_u;
        const double q = 1.0 / c.s2;
        double y[RS_MAX_R];
#pragma unroll
        for (int r = 0; r < RS_MAX_R; r++) {
            if (r >= R) continue;
            y[r] = pq_null();
            if (live) {
                double e = 0.0;
#pragma unroll
                for (int j = 0; j < RS_MAX_K; j++)
                    if (act[j]) e += c.x[j] * uk[j][r];
                e = e + u[((int64_t)r * M + K + c.g) * D + dd];
                y[r] = q * (c.v[r] - e);
            }
            out.y[r][s * out.stride + dd] = rk_nan_null(y[r]);
        }
        if (!live) continue;
#pragma unroll
        for (int r = 0; r < RS_MAX_R; r++)
#pragma unroll
            for (int l = 0; l <= r; l++)
                if (r < R) acc[rs_tri(r) + l] += c.v[r] * y[l];
    }
    const int NP = rs_tri(R);
#pragma unroll
    for (int p = 0; p < RS_PAIRS; p++)
        if (p < NP) pq[((int64_t)blockIdx.y * NP + p) * D + dd] = acc[p];
}

// one thread per (as-of day, pair r >= q): the block sums in ascending block order from 0.0 -> quad[r][q][count], mirrored to [q][r]
__global__ __launch_bounds__(64) void rs_quad_kernel(const double *pq, const int32_t *okf, int64_t nblk, int64_t D, int R, double *quad) {
    const int64_t dd = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const int p = blockIdx.y, NP = rs_tri(R);
    if (dd >= D) return;
    int r = 0;
    while (rs_tri(r + 1) <= p) r++;
    const int q = p - rs_tri(r);
    double s = 0.0;
    for (int64_t k = 0; k < nblk; k++) s += pq[(k * NP + p) * D + dd];
    const double v = okf[dd] ? rk_nan_null(s) : pq_null();
    quad[((int64_t)r * R + q) * D + dd] = v;
    quad[((int64_t)q * R + r) * D + dd] = v;
}

} // namespace

extern "C" {

pq_status pq_risk_solve(pq_ctx *ctx, const pq_batch *b, const double *const *rhs, int32_t n_rhs, const double *const *exposures, int32_t k,
                        const int32_t *industry, int64_t group_stride, int32_t n_groups, const double *cov, const double *specific_var,
                        int64_t sv_stride, int64_t day0, int64_t step, int64_t count, double *const *y_out, int64_t out_stride,
                        double *quad_out, int32_t *n_out) {
    const char *what = "pq_risk_solve";
    auto refuse = [&](const char *text, pq_status s) { pq_set_error("%s: %s", what, text); return s; };
    PQ_TRY(pq_check(ctx, b));
    if (n_rhs < 1 || n_rhs > RS_MAX_R) return refuse("n_rhs must be in [1, 4]", PQ_ERR_ARG);
    if (k < 0 || k > RS_MAX_K) return refuse("k must be in [0, 8]", PQ_ERR_ARG);
    RsIn in{};
    PQ_TRY(xs_groups_arg(what, b, industry, group_stride, n_groups, XsGroupsPolicy{XS_G_ALWAYS, "n_groups", "industry"}, &in.grp));
    if (k + n_groups > RS_MAX_M) return refuse("k + n_groups must be <= 128 (PQ_RISK_SOLVE_MAX_M): the system is solved in LDS", PQ_ERR_UNSUPPORTED);
    if (ctx->rec) return refuse("cannot be recorded into a suite", PQ_ERR_UNSUPPORTED);
    if (b->offsets) return refuse("ragged batches are not supported", PQ_ERR_UNSUPPORTED);
    PQ_TRY(xs_groups_stride(what, b, industry != nullptr, group_stride));
    PQ_TRY(rk_days(what, b->len, day0, step, count, &in.a));
    if (sv_stride < count) return refuse("sv_stride must be >= count", PQ_ERR_ARG);
    if (out_stride < count) return refuse("out_stride must be >= count", PQ_ERR_ARG);
    if (count == 0 || b->len == 0 || b->n_series == 0) return PQ_OK;
    if (!(rhs && cov && specific_var && y_out && quad_out && n_out && (k == 0 || exposures))) return refuse("null pointer", PQ_ERR_ARG);
    in.d = dims_of(b);
    const int R = n_rhs, G = n_groups, M = k + G;
    const uintptr_t plane = xw_plane_bytes(in.d), yb = (uintptr_t)in.d.n * (uintptr_t)out_stride * 8;
    XwSpan ins[RS_MAX_R + RS_MAX_K + 3], outs[RS_MAX_R + 2];
    int ni = 0, no = 0;
    RsOut out{};
    for (int r = 0; r < R; r++) {
        if (!y_out[r]) return refuse("null output pointer", PQ_ERR_ARG);
        in.v[r] = rhs[r];
        out.y[r] = y_out[r];
        if (rhs[r]) ins[ni++] = xw_span(rhs[r], plane);
        outs[no++] = xw_span(y_out[r], yb);
    }
    for (int j = 0; j < k; j++) {
        if (!exposures[j]) return refuse("null exposure pointer", PQ_ERR_ARG);
        in.x[j] = exposures[j];
        ins[ni++] = xw_span(exposures[j], plane);
    }
    if (industry) ins[ni++] = xw_span(industry, (group_stride ? (uintptr_t)in.d.n * (uintptr_t)group_stride : (uintptr_t)in.d.n) * 4);
    ins[ni++] = xw_span(cov, (uintptr_t)count * M * M * 8);
    ins[ni++] = xw_span(specific_var, (uintptr_t)in.d.n * (uintptr_t)sv_stride * 8);
    outs[no++] = xw_span(quad_out, (uintptr_t)R * R * (uintptr_t)count * 8);
    outs[no++] = xw_span(n_out, (uintptr_t)2 * (uintptr_t)count * 4);
    PQ_TRY(xw_no_overlap(outs, no, ins, ni, "pq_risk_solve: an output must not overlap an input",
                         "pq_risk_solve: the outputs must not overlap each other"));
    in.R = R;
    in.K = k;
    in.sv = specific_var;
    in.sv_stride = sv_stride;
    out.stride = out_stride;
    const int NT = rs_tri(k) + k * R, NCOL = 1 + k + R, NC = NT + NCOL * G, NP = rs_tri(R), chunk = rs_chunk(NCOL, G);
    const int64_t D = count, nblk = xs_nblk(in.d.n);
    // workspace: block partials ps (f64): the larger of a moments launch [nblk][NT + chunk G][D] and the output pass's [nblk][NP][D] | the
    // moments mom [NC][D] | u [R][M][D] | block counts pc [nblk][2][D] (i32) | ok [D] (i32)
    const size_t part = (size_t)nblk * D, p1 = part * (size_t)(NT + chunk * G), p3 = part * (size_t)NP;
    double *ps, *mom, *u;
    int32_t *pc, *ok;
    PQ_TRY(xs_ws_carve(ctx, what, [&](XsWs &w) {
        w.take(ps, p1 > p3 ? p1 : p3).take(mom, (size_t)NC * D).take(u, (size_t)R * M * D).take(pc, part * 2).take(ok, (size_t)D);
    }));
    const dim3 gd((unsigned)((D + 63) / 64)), gp(gd.x, (unsigned)nblk);
    hipStream_t st = ctx->stream;
    const size_t lds1 = (size_t)chunk * G * 64 * 8, lds2 = rs_solve_lds(k, G, R);
    PQ_HIP_TRY(hipFuncSetAttribute((const void *)rs_moments_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds1));
    PQ_HIP_TRY(hipFuncSetAttribute((const void *)rs_moments_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds1));
    PQ_HIP_TRY(hipFuncSetAttribute((const void *)rs_solve_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2));
    for (int c0 = 0; c0 < NCOL; c0 += chunk) {
        const int c1 = c0 + chunk < NCOL ? c0 + chunk : NCOL, nreg = c0 == 0 ? NT : 0, np = nreg + (c1 - c0) * G;
        if (c0 == 0) hipLaunchKernelGGL(rs_moments_kernel<true>, gp, dim3(64), (size_t)(c1 - c0) * G * 64 * 8, st, in, c0, c1, ps, pc);
        else hipLaunchKernelGGL(rs_moments_kernel<false>, gp, dim3(64), (size_t)(c1 - c0) * G * 64 * 8, st, in, c0, c1, ps, pc);
        hipLaunchKernelGGL(rs_sum_kernel, dim3(gd.x, (unsigned)np), dim3(64), 0, st, (const double *)ps, c0 == 0 ? (const int32_t *)pc : nullptr,
                           nblk, D, np, nreg, NT + c0 * G, mom, n_out);
    }
    const RsSolve sa{mom, cov, n_out, D, k, G, R, u, ok};
    hipLaunchKernelGGL(rs_solve_kernel, dim3((unsigned)D), dim3(RS_THREADS), lds2, st, sa);
    hipLaunchKernelGGL(rs_output_kernel, gp, dim3(64), 0, st, in, (const double *)mom, (const double *)u, (const int32_t *)ok, out, ps);
    hipLaunchKernelGGL(rs_quad_kernel, dim3(gd.x, (unsigned)NP), dim3(64), 0, st, (const double *)ps, (const int32_t *)ok, nblk, D, R, quad_out);
    PQ_HIP_TRY(hipGetLastError());
    return PQ_OK;
}

} // extern "C"
