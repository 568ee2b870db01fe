"""Two restatements of decision D-23 (the SequentialBacktester engine on an order tape), written from its text in
plain Python floats (IEEE doubles, one rounding per operation, no contraction).

run_literal  the reference's shape: dicts for positions, entries and the price board; the valuation is summed in ascending asset id
             (the reference sums in HashMap iteration order, which is unspecified, so ascending id stands for "some other order").
run_lanes    the same fills; the valuation in D-22's order: 64 partials from +0.0 (partial k adds a = k, k + 64, ...), folded
             p[k] += p[k + s] for s = 32 .. 1.  This is what the kernel must reproduce bit for bit.

Both return {"equity", "cash": [T], "position": [A], "trades", "wins", "outcomes": {"buy_filled", "buy_rejected", "sell_filled",
"sell_rejected"}} and apply the C ABI's defensive rules (an offset is clamped into [0, n_orders], a decreasing pair is an empty period,
an asset id outside [0, A) is skipped)."""
import math

import numpy as np

DEFAULTS = dict(initial_capital=100000.0, buy_slippage=0.0, sell_slippage=0.0, buy_commission_rate=0.0003,
                sell_commission_rate=0.0003, minimum_commission_fee=5.0)


def rs_max(a, b):
    """f64::max: the other operand when one is NaN"""
    if a != a:
        return b
    if b != b:
        return a
    return a if a > b else b


def sum_lanes(terms):
    """D-22's summation order over a list of terms"""
    p = [0.0] * 64
    for k, x in enumerate(terms):
        p[k % 64] += x
    s = 32
    while s:
        for k in range(s):
            p[k] += p[k + s]
        s //= 2
    return p[0]


def _run(period_offsets, asset, quantity, price, n_assets, params, lanes):
    prm = {**DEFAULTS, **(params or {})}
    off = [int(v) for v in np.asarray(period_offsets).reshape(-1)]
    asset = [int(v) for v in np.asarray(asset).reshape(-1)]
    quantity = [float(v) for v in np.asarray(quantity, dtype=np.float64).reshape(-1)]
    price = [float(v) for v in np.asarray(price, dtype=np.float64).reshape(-1)]
    n, T, A = len(asset), len(off) - 1, int(n_assets)
    clamp = lambda v: 0 if v < 0 else (n if v > n else v)
    cash = float(prm["initial_capital"])
    pos, entry, board = {}, {}, {}                      # membership in pos = held
    trades = wins = 0
    out = dict(buy_filled=0, buy_rejected=0, sell_filled=0, sell_rejected=0)
    equity, cash_row = [], []
    for t in range(T):
        for i in range(clamp(off[t]), clamp(off[t + 1])):
            a, q, p = asset[i], quantity[i], price[i]
            if p != p or not p > 0.0 or q != q or q == 0.0:
                continue
            if a < 0 or a >= A:
                continue
            board[a] = p
            have = pos.get(a, 0.0)
            if q > 0.0:
                fp = p + prm["buy_slippage"]
                cost = q * fp
                com = rs_max(cost * prm["buy_commission_rate"], prm["minimum_commission_fee"])
                due = cost + com
                if cash >= due:
                    cash -= due
                    pos[a] = have + q
                    entry[a] = fp
                    trades += 1
                    out["buy_filled"] += 1
                else:
                    out["buy_rejected"] += 1
            else:
                aq = abs(q)
                if have >= aq:
                    fp = p - prm["sell_slippage"]
                    rev = aq * fp
                    com = rs_max(rev * prm["sell_commission_rate"], prm["minimum_commission_fee"])
                    net = rev - com
                    cash += net
                    pos[a] = have + q
                    if net > aq * entry[a]:
                        wins += 1
                    if pos[a] <= 1e-8:
                        del pos[a]
                        del entry[a]
                    out["sell_filled"] += 1
                else:
                    out["sell_rejected"] += 1
        if lanes:
            v = sum_lanes([pos[a] * board[a] if a in pos else 0.0 for a in range(A)])
        else:
            v = 0.0
            for a in sorted(pos):
                v += pos[a] * board[a]
        equity.append(cash + v)
        cash_row.append(cash)
    position = np.zeros(A)
    for a, h in pos.items():
        position[a] = h
    return dict(equity=np.array(equity, dtype=np.float64), cash=np.array(cash_row, dtype=np.float64), position=position,
                trades=trades, wins=wins, outcomes=out)


def run_literal(period_offsets, asset, quantity, price, n_assets, params=None):
    return _run(period_offsets, asset, quantity, price, n_assets, params, lanes=False)


def run_lanes(period_offsets, asset, quantity, price, n_assets, params=None):
    return _run(period_offsets, asset, quantity, price, n_assets, params, lanes=True)


def random_tape(seed, T, A, orders_per_period, exact=False, c0=100000.0, shuffle_ids=False):
    """A tape on which every outcome occurs: buys of small lots (a few per cent of c0), a few too large for the cash left; sells drawn
    from the assets bought earlier in the tape, some for more than is held.  orders_per_period: an int (Poisson mean) or a list of
    per-period counts.  exact: prices are multiples of 1/64 and quantities integers <= 400, so that every product and sum of the walk
    is exact when the slippages are multiples of 1/64, the rates 2^-12 and the fee 5.  -> (period_offsets [T + 1], asset, quantity,
    price)"""
    rng = np.random.default_rng(seed)
    counts = rng.poisson(orders_per_period, T) if np.isscalar(orders_per_period) else np.asarray(orders_per_period)
    ids = rng.permutation(A) if shuffle_ids else np.arange(A)
    base = rng.uniform(5.0, 60.0, A)
    bought = []
    aa, qq, pp = [], [], []
    for t in range(T):
        for _ in range(int(counts[t])):
            sell = bought and rng.random() < 0.45
            a = int(bought[rng.integers(len(bought))]) if sell else int(rng.integers(A))
            p = base[a] * (1.0 + 0.3 * math.sin(0.37 * t + a) + 0.05 * rng.standard_normal())
            p = max(p, 0.5)
            r = rng.random()
            if sell:
                q = -float(rng.integers(1, 400)) if r < 0.7 else -float(rng.integers(300, 2000))
            else:
                q = float(rng.integers(1, 400)) if r < 0.8 else float(rng.integers(3000, 40000)) * c0 / 1e5
                if q <= 400.0:
                    bought.append(a)
            if exact:
                p = max(round(p * 64.0), 32.0) / 64.0
                q = float(np.clip(round(q), -400, 400)) if abs(q) <= 400 else q
                if abs(q) > 400:
                    q = 400.0 if q > 0 else -400.0
            else:
                q = q + (rng.random() * 0.5 if rng.random() < 0.3 else 0.0) * (1 if q > 0 else -1)
            aa.append(int(ids[a])); qq.append(q); pp.append(p)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return off, np.array(aa, dtype=np.int32), np.array(qq, dtype=np.float64), np.array(pp, dtype=np.float64)


def tape_of(periods):
    """[[(asset, signed quantity, price), ...] per period] -> (period_offsets, asset, quantity, price)"""
    off, aa, qq, pp = [0], [], [], []
    for orders in periods:
        for a, q, p in orders:
            aa.append(a); qq.append(q); pp.append(p)
        off.append(len(aa))
    return (np.array(off, dtype=np.int64), np.array(aa, dtype=np.int32), np.array(qq, dtype=np.float64),
            np.array(pp, dtype=np.float64))


_R10 = dict(buy_commission_rate=2.0 ** -10, sell_commission_rate=2.0 ** -10)
_TINY, _SMALL = 1.0 - 5e-9, 1.0 - 2e-8                   # sells that leave 5e-9 (dropped) and 2e-8 (kept) of one share

# Known answers derived by hand from D-23's text: name -> (periods, n_assets, params, expected).  Every number below is exactly
# representable or written as the one rounded operation the text prescribes.
KATS = {
    # cost 995 <= cash 999 < cost + fee 1000: rejected although the cost alone is covered; the board moves, nothing is held
    "buy_rejected_by_less_than_the_commission": (
        [[(0, 10.0, 99.5)]], 1, dict(initial_capital=999.0),
        dict(equity=[999.0], cash=[999.0], position=[0.0], trades=0, wins=0)),
    "buy_filled_with_the_last_cent": (
        [[(0, 10.0, 99.5)]], 1, dict(initial_capital=1000.0),
        dict(equity=[995.0], cash=[0.0], position=[10.0], trades=1, wins=0)),
    # 11 > 10 held: rejected, but its price 60 marks the 10 shares: 99495 + 600
    "sell_rejected_for_position": (
        [[(0, 10.0, 50.0)], [(0, -11.0, 60.0)]], 1, {},
        dict(equity=[99995.0, 100095.0], cash=[99495.0, 99495.0], position=[10.0], trades=1, wins=0)),
    # a buy far beyond the cash moves the board to 55; the empty period after it keeps the valuation
    "unfilled_order_moves_the_board": (
        [[(1, 10.0, 50.0)], [(1, 1e6, 55.0)], []], 2, {},
        dict(equity=[99995.0, 100045.0, 100045.0], cash=[99495.0] * 3, position=[0.0, 10.0], trades=1, wins=0)),
    # entry is overwritten, not averaged: net 645 against 10 * 70 is no win (against the average 60 or the first 50 it would be)
    "second_buy_overwrites_the_entry_no_win": (
        [[(0, 10.0, 50.0)], [(0, 10.0, 70.0)], [(0, -10.0, 65.0)]], 1, {},
        dict(equity=[99995.0, 100190.0, 100085.0], cash=[99495.0, 98790.0, 99435.0], position=[10.0], trades=2, wins=0)),
    # the same orders with the buys swapped: entry 50, net 645 > 500 wins; the sell is not a trade
    "second_buy_overwrites_the_entry_win": (
        [[(0, 10.0, 70.0)], [(0, 10.0, 50.0)], [(0, -10.0, 65.0)]], 1, {},
        dict(equity=[99995.0, 99790.0, 100085.0], cash=[99295.0, 98790.0, 99435.0], position=[10.0], trades=2, wins=1)),
    # 1 - (1 - 5e-9) <= 1e-8: the remainder is dropped, equity is the cash alone
    "remainder_dropped": (
        [[(0, 1.0, 100.0)], [(0, -_TINY, 100.0)]], 1, {},
        dict(equity=[99995.0, 99895.0 + (_TINY * 100.0 - 5.0)], cash=[99895.0, 99895.0 + (_TINY * 100.0 - 5.0)], position=[0.0],
             trades=1, wins=0)),
    # 1 - (1 - 2e-8) > 1e-8: kept and valued
    "remainder_kept": (
        [[(0, 1.0, 100.0)], [(0, -_SMALL, 100.0)]], 1, {},
        dict(equity=[99995.0, (99895.0 + (_SMALL * 100.0 - 5.0)) + (1.0 - _SMALL) * 100.0],
             cash=[99895.0, 99895.0 + (_SMALL * 100.0 - 5.0)], position=[1.0 - _SMALL], trades=1, wins=0)),
    # rate 2^-10: 500 -> 0.49 < 5 takes the fee; 51200 -> 50 and 61440 -> 60 take the rate; 600 -> 0.59 takes the fee.  Asset 0 stays
    # marked at 50 until its own sell: 109625 + 10 * 50
    "commission_takes_each_branch": (
        [[(0, 10.0, 50.0)], [(1, 1024.0, 50.0)], [(1, -1024.0, 60.0)], [(0, -10.0, 60.0)]], 2, _R10,
        dict(equity=[99995.0, 99945.0, 110125.0, 110220.0], cash=[99495.0, 48245.0, 109625.0, 110220.0], position=[0.0, 0.0],
             trades=2, wins=2)),
    # three orders for one asset in one period: 10 @ 50, 5 @ 52 (entry 52), sell 12 @ 51: net 607 < 12 * 52, 3 left at 51
    "same_asset_three_times_in_one_period": (
        [[(0, 10.0, 50.0), (0, 5.0, 52.0), (0, -12.0, 51.0)]], 1, {},
        dict(equity=[99990.0], cash=[99837.0], position=[3.0], trades=2, wins=0)),
    # slippage: buy at 50 + 0.5, sell at 60 - 0.25
    "slippage_moves_the_fill_price_not_the_board": (
        [[(0, 10.0, 50.0)], [(0, -4.0, 60.0)]], 1, dict(buy_slippage=0.5, sell_slippage=0.25),
        dict(equity=[99990.0, 100084.0], cash=[99490.0, 99724.0], position=[6.0], trades=1, wins=1)),
}
