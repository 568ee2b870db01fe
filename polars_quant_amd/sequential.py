"""SequentialBacktester -- the reference's shared-cash portfolio engine (src/backtest/sequential.rs:207-336) with the same constructor
arguments, callback protocol and result shape, backed by the order-tape HIP kernel (decision D-23).

The reference calls `strategy_callback(ctx, t)` once per period and matches the orders the callback committed through `ctx.buy` /
`ctx.sell`.  The callback sees nothing of the engine's state (no cash, positions, fills or equity), so its orders do not depend on the
matching: `OrderTape.record` runs every callback on the host first, and one kernel launch then replays the tapes, one wavefront per
tape.  `run_many` replays many tapes -- a sweep over strategies, or one strategy under many capital and cost settings -- in one launch.
"""
from __future__ import annotations

import numpy as np

from ._spec import SEQ_DEFAULTS, SUMMARY_KEYS


class OrderContext:
    """What the callback receives (sequential.rs:175-205): `buy` / `sell` commit a pending order; an order with a NaN or non-positive
    price, or a NaN or non-positive quantity, is dropped."""

    def __init__(self):
        self.pending_orders = []            # (target_asset, signed quantity, execution_price)

    def buy(self, target_asset, target_quantity, execution_price):
        q, p = float(target_quantity), float(execution_price)
        if not np.isnan(p) and p > 0.0 and q > 0.0:
            self.pending_orders.append((target_asset, q, p))

    def sell(self, target_asset, target_quantity, execution_price):
        q, p = float(target_quantity), float(execution_price)
        if not np.isnan(p) and p > 0.0 and q > 0.0:
            self.pending_orders.append((target_asset, -q, p))


class OrderTape:
    """The orders of one strategy over `n_periods` periods: `assets` (the names, id = index), `period_offsets` [T + 1] int64 and the
    order arrays `asset` int32 / `quantity` (signed) / `price` in callback order; period t owns orders
    [period_offsets[t], period_offsets[t + 1]).  Construction raises ValueError unless the offsets start at 0, never decrease and end at
    the order count, and every asset id is in range."""

    def __init__(self, assets, period_offsets, asset, quantity, price):
        self.assets = list(assets)
        self.period_offsets = np.ascontiguousarray(period_offsets, dtype=np.int64).reshape(-1)
        self.asset = np.ascontiguousarray(asset, dtype=np.int32).reshape(-1)
        self.quantity = np.ascontiguousarray(quantity, dtype=np.float64).reshape(-1)
        self.price = np.ascontiguousarray(price, dtype=np.float64).reshape(-1)
        n = self.asset.size
        if self.quantity.size != n or self.price.size != n:
            raise ValueError("asset, quantity and price must have one entry per order")
        off = self.period_offsets
        if off.size < 1 or off[0] != 0 or off[-1] != n or (np.diff(off) < 0).any():
            raise ValueError("period_offsets must start at 0, never decrease and end at the number of orders")
        if n and (self.asset.min() < 0 or self.asset.max() >= len(self.assets)):
            raise ValueError(f"asset ids must lie in [0, {len(self.assets)})")

    @property
    def n_periods(self) -> int:
        return self.period_offsets.size - 1

    @property
    def n_orders(self) -> int:
        return self.asset.size

    @classmethod
    def record(cls, callback, n_periods: int, assets=None) -> "OrderTape":
        """Calls `callback(ctx, t)` for t = 0 .. n_periods - 1, each with a fresh OrderContext, and keeps the orders it committed.
        Assets are numbered in first-seen order unless `assets` lists them (an order for an asset outside the list then raises
        ValueError).  Like the reference (sequential.rs:294, `let _ =`), an exception raised by the callback is swallowed: the orders
        committed before it in that period are kept and the run goes on with the next period."""
        fixed = assets is not None
        names = list(assets) if fixed else []
        ids = {a: k for k, a in enumerate(names)}
        off, aa, qq, pp = [0], [], [], []
        for t in range(int(n_periods)):
            ctx = OrderContext()
            try:
                callback(ctx, t)
            except Exception:  # noqa: BLE001 -- the reference discards the callback's result, an error included
                pass
            for name, q, p in ctx.pending_orders:
                k = ids.get(name)
                if k is None:
                    if fixed:
                        raise ValueError(f"order for {name!r}, which is not among the given assets")
                    k = ids[name] = len(names)
                    names.append(name)
                aa.append(k); qq.append(q); pp.append(p)
            off.append(len(aa))
        return cls(names, off, aa, qq, pp)


def _table(cols: dict):
    try:
        import polars as pl  # optional
        return pl.DataFrame(cols)
    except ImportError:
        return cols


class SequentialBacktester:
    def __init__(self, historical_data, benchmark=None, initial_capital=100_000.0, buy_slippage=0.0, sell_slippage=0.0,
                 buy_commission_rate=0.0003, sell_commission_rate=0.0003, minimum_commission_fee=5.0):
        self.historical_data, self.benchmark = historical_data, benchmark
        self.n_periods = int(historical_data.height) if hasattr(historical_data, "height") else len(historical_data)
        self.params = dict(initial_capital=initial_capital, buy_slippage=buy_slippage, sell_slippage=sell_slippage,
                           buy_commission_rate=buy_commission_rate, sell_commission_rate=sell_commission_rate,
                           minimum_commission_fee=minimum_commission_fee)

    def _benchmark(self):
        """the first column of the benchmark as f64 when it has exactly one row per period, else None (sequential.rs:264-276,
        metrics.rs:86: a benchmark of another length is not used)"""
        b = self.benchmark
        if b is None:
            return None
        if hasattr(b, "columns"):                                # polars / pandas frame
            b = b[list(b.columns)[0]]
        elif isinstance(b, dict):
            b = b[next(iter(b))]
        if hasattr(b, "to_numpy"):
            b = b.to_numpy()
        elif hasattr(b, "cpu"):
            b = b.cpu().numpy()
        b = np.ascontiguousarray(b, dtype=np.float64).reshape(-1)
        return b if b.size == self.n_periods else None

    def _tape(self, x) -> OrderTape:
        tape = x if isinstance(x, OrderTape) else OrderTape.record(x, self.n_periods)
        if tape.n_periods != self.n_periods:
            raise ValueError(f"a tape of {tape.n_periods} periods for {self.n_periods} rows of historical_data")
        return tape

    def run_many(self, callbacks_or_tapes, params=None) -> dict:
        """Replays callbacks and / or OrderTapes in ONE launch.  The tapes' assets are renumbered into one universe, the union in
        first-seen order.  params: optional list with one dict per tape that overrides the constructor's six values.
        -> {"equity", "cash": [B, T], "position": [B, A], "trades", "wins": [B], "summary": list of B dicts, "assets": the universe}
        (numpy arrays)."""
        from . import api as _api
        tapes = [self._tape(x) for x in callbacks_or_tapes]
        B, T = len(tapes), self.n_periods
        if params is not None and len(params) != B:
            raise ValueError(f"params must hold one dict per tape ({B}), got {len(params)}")
        plist = [{**self.params, **(params[k] if params is not None else {})} for k in range(B)]
        for d in plist:
            unknown = set(d) - set(SEQ_DEFAULTS)
            if unknown:
                raise ValueError(f"unknown parameters {sorted(unknown)}")
        universe, ids = [], {}
        offs, aa, qq, pp, base = [], [], [], [], 0
        for tape in tapes:
            remap = np.empty(len(tape.assets), dtype=np.int32)
            for k, name in enumerate(tape.assets):
                if name not in ids:
                    ids[name] = len(universe)
                    universe.append(name)
                remap[k] = ids[name]
            offs.append(tape.period_offsets + base)
            aa.append(remap[tape.asset] if tape.n_orders else tape.asset)
            qq.append(tape.quantity); pp.append(tape.price)
            base += tape.n_orders
        A = len(universe)
        empty = dict(equity=np.zeros((B, T)), cash=np.zeros((B, T)), position=np.zeros((B, A)), trades=np.zeros(B, np.int64),
                     wins=np.zeros(B, np.int64), summary=[{} for _ in range(B)], assets=universe)
        if B == 0 or T == 0:
            return empty
        cat = lambda xs, dt: np.concatenate(xs).astype(dt, copy=False) if xs else np.zeros(0, dt)
        r = _api.backtest_sequential(np.stack(offs), cat(aa, np.int32), cat(qq, np.float64), cat(pp, np.float64), A,
                                     self._benchmark(), plist)
        host = {k: v.cpu().numpy() for k, v in r.items()}
        return dict(equity=host["equity"], cash=host["cash"], position=host["position"], trades=host["counts"][:, 0].copy(),
                    wins=host["counts"][:, 1].copy(),
                    summary=[dict(zip(SUMMARY_KEYS, (float(v) for v in row))) for row in host["summary"]], assets=universe)

    def run(self, strategy_callback):
        """-> (positions, capital {"equity": [T]}, summary dict) as the reference returns them (sequential.rs:324-335): positions is
        an empty table; with polars installed both tables are pl.DataFrame, otherwise dicts of arrays."""
        r = self.run_many([strategy_callback])
        return _table({}), _table({"equity": r["equity"][0]}), r["summary"][0]
