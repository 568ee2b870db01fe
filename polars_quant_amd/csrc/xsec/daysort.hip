// xsec/daysort.hip -- the wide half of the day-sort stage (D-15): cross-sections above XS_LDS_MAX symbols are sorted by rocPRIM's segmented
// radix sort (keys only) in global memory, one segment per day.  The only xsec file that includes rocPRIM; sorts.hip, double_sort.hip,
// clean.hip and build.hip plan the sort and lay the tail out at the end of their own workspace; the consumer on the sorted rows is
// xs_sort_wide_kernel<Op> (xsec_dev.h: sorts.hip, double_sort.hip, build.hip) or the caller's own (clean.hip).  The LDS half of the
// stage is in xsec_dev.h; robust.hip uses that half alone and has no wide sort (above XS_LDS_MAX it calls pq_factor_ic).
#include "xsec_dev.h"
#include <rocprim/rocprim.hpp>

namespace {

__global__ __launch_bounds__(256) void xs_offsets_kernel(unsigned *off, int64_t segs, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i <= segs) off[i] = (unsigned)(i * n);
}

// workspace: the wide tail -- sorted keys (f64, day-major) | segment offsets (u32) [len + 1] | rocPRIM temp
struct XsDayTail { double *srt; unsigned *off; unsigned char *tmp; };
void xs_day_tail(XsWs &w, const Dims &d, size_t tmp, XsDayTail &t) { w.take(t.srt, (size_t)d.len * d.n).take(t.off, d.len + 1).take(t.tmp, tmp); }

} // namespace

pq_status xs_day_sort_plan(pq_ctx *ctx, const Dims &d, const char *who, XsDaySort *plan) {
    *plan = XsDaySort{d.n > XS_LDS_MAX, 0, 0};
    if (!plan->wide) return PQ_OK;
    const size_t cells = (size_t)d.len * (size_t)d.n;
    if (d.n > 100000) { pq_set_error("%s: at most 100000 series are supported", who); return PQ_ERR_ARG; }
    if (cells >= (1ull << 32)) { pq_set_error("%s: n_series * len must be < 2^32 above 16384 series", who); return PQ_ERR_ARG; }
    PQ_HIP_TRY(rocprim::segmented_radix_sort_keys(nullptr, plan->tmp_bytes, (double *)nullptr, (double *)nullptr, (unsigned)cells,
                                                  (unsigned)d.len, (unsigned *)nullptr, (unsigned *)nullptr, 0, 64, ctx->stream));
    XsWs measure{nullptr};
    XsDayTail t;
    xs_day_tail(measure, d, plan->tmp_bytes, t);
    if (measure.bad) { pq_set_error("%s: the sort's workspace does not fit size_t", who); return PQ_ERR_ARG; }
    plan->bytes = measure.off;
    return PQ_OK;
}

pq_status xs_day_sort_wide(pq_ctx *ctx, const Dims &d, const XsDaySort &plan, unsigned char *tail, const double *key, const double **sorted) {
    XsWs w{tail};
    XsDayTail t;
    xs_day_tail(w, d, plan.tmp_bytes, t);
    size_t tmp_bytes = plan.tmp_bytes;
    hipLaunchKernelGGL(xs_offsets_kernel, dim3((unsigned)((d.len + 256) / 256)), dim3(256), 0, ctx->stream, t.off, d.len, d.n);
    PQ_HIP_TRY(rocprim::segmented_radix_sort_keys(t.tmp, tmp_bytes, key, t.srt, (unsigned)((size_t)d.len * (size_t)d.n),
                                                  (unsigned)d.len, t.off, t.off + 1, 0, 64, ctx->stream));
    *sorted = t.srt;
    return PQ_OK;
}
