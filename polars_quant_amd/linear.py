"""`linear(df, x_cols, y_col, pred_col, resid_col, return_stats)` -- README.md:165-240 of the reference (README-only, no source in the
tree; semantics = decision D-24).  One pooled ordinary least squares fit of `y_col` on `x_cols` with an intercept over all rows; the
arithmetic runs in pq_linear (HIP), this module only moves columns and puts the intercept first.

`df` may be a polars DataFrame (returned with the two new columns, nulls in and nulls out, as the README shows), a pyarrow Table, or a
dict of columns ([M] or [N, T], host or device; a new dict with two more entries comes back, in the container kind of the y column).
With return_stats=True the result is `(df, (coefficients, r_squared))`: coefficients = [b0, b1, ..., bK] with the intercept b0 FIRST,
r_squared a float; both are nan where the fit has no solution (fewer than K + 2 complete rows, or collinear / constant regressors).
"""
from __future__ import annotations

from . import api


def linear(df, x_cols, y_col, pred_col: str = "pred", resid_col: str = "resid", return_stats: bool = False):
    x_cols = [x_cols] if isinstance(x_cols, str) else list(x_cols)
    mod = type(df).__module__.split(".")[0]
    table = mod == "pyarrow" and hasattr(df, "append_column")
    if not (mod == "polars" or table or isinstance(df, dict)):
        raise TypeError(f"df must be a polars DataFrame, a pyarrow Table or a dict of columns, not {type(df).__name__}")
    col = df.column if table else df.__getitem__
    ty, kind, squeeze = api._to_device(col(y_col))
    txs = [api._to_device(col(c))[0] for c in x_cols]
    fit = api.linear([t[0] for t in txs] if squeeze else txs, ty[0] if squeeze else ty)
    pred, resid = (api._from_device(fit[k], kind, False, name) for k, name in (("pred", pred_col), ("resid", resid_col)))
    if mod == "polars":
        out = df.with_columns(pred, resid)
    elif table:
        out = df.append_column(pred_col, pred).append_column(resid_col, resid)
    else:
        out = dict(df)
        out[pred_col], out[resid_col] = pred, resid
    if not return_stats:
        return out
    coef = fit["coef"].cpu().tolist()
    return out, ([coef[-1]] + coef[:-1], float(fit["r_squared"].cpu()))
