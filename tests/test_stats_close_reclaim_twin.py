"""The reclaiming stats close (`StatsAggState.close_due`,
`close_below`, `close_all`) on the CPU twin.

The rule under test, for a close at `horizon`: cells of windows in
``[closed_horizon, horizon)`` are emitted, cells at or above `horizon`
stay, and everything below `horizon` is forgotten.  The reference is an
exact int64 numpy group-by; nothing has a tolerance.
"""

from datetime import datetime, timezone

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from bytewax_amd.gpu import RecordBatch, _ms  # noqa: E402
from bytewax_amd.gpu.state import StatsAggState  # noqa: E402

ALIGN_MS = _ms(datetime(2024, 1, 1, tzinfo=timezone.utc))
LEN_MS = 60_000
CPU = torch.device("cpu")
COLS = ("keys", "wins", "cnt", "sum", "min", "max")


def _ref_stats(keys, x, vals):
    """{(key, window): (count, sum mod 2^64, min, max)} of events given
    as offsets `x` >= 0 from the alignment."""
    keys = np.asarray(keys, dtype=np.int64)
    x = np.asarray(x, dtype=np.int64)
    vals = np.asarray(vals, dtype=np.int64)
    assert (x >= 0).all()
    if keys.size == 0:
        return {}
    wins = x // LEN_MS
    order = np.lexsort((wins, keys))
    k, w, v = keys[order], wins[order], vals[order]
    first = np.flatnonzero(
        np.r_[True, (k[1:] != k[:-1]) | (w[1:] != w[:-1])]
    )
    cnt = np.diff(np.r_[first, k.size])
    with np.errstate(over="ignore"):
        s = np.add.reduceat(v, first)
    mn = np.minimum.reduceat(v, first)
    mx = np.maximum.reduceat(v, first)
    return {
        (int(a), int(b)): (int(c), int(d), int(e), int(f))
        for a, b, c, d, e, f in zip(k[first], w[first], cnt, s, mn, mx)
    }


def _got(out, into=None):
    """Rows of one close as a dict; no cell twice, also across the
    closes collected in `into`."""
    got = {} if into is None else into
    if out is None:
        return got
    for k, w, c, s, mn, mx in zip(*(out[n].tolist() for n in COLS)):
        assert (k, w) not in got, f"cell {(k, w)} emitted twice"
        got[(k, w)] = (c, s, mn, mx)
    return got


def _cat(batches):
    return tuple(np.concatenate([b[i] for b in batches]) for i in range(3))


def _window_batch(win, n, seed, n_keys=40):
    """`n` events inside window `win`."""
    rng = np.random.default_rng(seed)
    keys = rng.integers(-n_keys // 2, n_keys // 2, n).astype(np.int32)
    x = win * LEN_MS + rng.integers(0, LEN_MS, n)
    vals = rng.integers(-(1 << 40), 1 << 40, n)
    return keys, x, vals


def _insert(st, batch):
    keys, x, vals = batch
    x = np.asarray(x, dtype=np.int64)
    st.insert(
        RecordBatch(
            torch.from_numpy(np.asarray(keys, dtype=np.int32)),
            torch.from_numpy(ALIGN_MS + x),
            torch.from_numpy(np.asarray(vals, dtype=np.int64)),
            max_ts=int(ALIGN_MS + x.max()),
        )
    )


def _state(**kw):
    return StatsAggState(CPU, ALIGN_MS, LEN_MS, **kw)


def test_successive_closes_and_close_all_equal_the_reference():
    st = _state()
    batches, got = [], {}
    for w in range(6):
        # Each batch also reaches one window ahead, so every close
        # leaves live cells behind.
        b = _cat([_window_batch(w, 300, 10 + w), _window_batch(w + 1, 50, 90 + w)])
        batches.append(b)
        _insert(st, b)
        out = st.close_due(0)
        rows = _got(out)
        assert all(cell[1] < st.closed_horizon for cell in rows)
        _got(out, got)
        assert all(cell[1] >= st.closed_horizon for cell in st._table)
    assert st.closed_horizon == 6
    _got(st.close_all(), got)
    assert got == _ref_stats(*_cat(batches))
    assert st.close_all() is None


def test_close_due_is_none_until_the_horizon_advances():
    st = _state()
    assert st.close_due(0) is None
    _insert(st, _window_batch(2, 100, 1))
    first = st.close_due(0)
    assert first is None and st.closed_horizon == 2  # nothing below 2
    _insert(st, _window_batch(2, 100, 2))
    assert st.close_due(0) is None  # same horizon
    assert st.closed_horizon == 2
    # A wait holds the horizon back: window 2 is not due yet.
    _insert(st, _window_batch(3, 100, 3))
    assert st.close_due(LEN_MS) is None
    assert st.close_below(2) is None and st.close_below(-5) is None
    out = _got(st.close_due(0))
    assert out and {w for _k, w in out} == {2}
    assert st.closed_horizon == 3


def test_default_wait_is_the_constructors():
    st = _state(wait_ms=2 * LEN_MS)
    _insert(st, _cat([_window_batch(w, 50, w) for w in range(5)]))
    got = _got(st.close_due())
    assert {w for _k, w in got} == {0, 1}
    assert st.closed_horizon == 2


def test_cell_below_closed_horizon_is_dropped():
    st = _state()
    b0 = _cat([_window_batch(0, 200, 1), _window_batch(1, 200, 2)])
    _insert(st, b0)
    got = _got(st.close_due(0))  # closes window 0
    assert st.closed_horizon == 1
    # An event behind the watermark, in the window already emitted,
    # under a key of its own.
    stale = (np.array([9_999], dtype=np.int32), np.array([5]), np.array([7]))
    _insert(st, stale)
    assert (9_999, 0) in st._table
    # It shows in no extract ...
    assert (9_999, 0) not in _got(st.extract(clear=False))
    assert st.snapshot_to_host()["n"] == len(_ref_stats(*_window_batch(1, 200, 2)))
    # ... and the next close forgets it.
    b2 = _window_batch(2, 200, 3)
    _insert(st, b2)
    _got(st.close_due(0), got)
    assert (9_999, 0) not in st._table
    assert all(w >= 2 for _k, w in st._table)
    _got(st.close_all(), got)
    assert got == _ref_stats(*_cat([b0, b2]))


def test_close_below_skips_ahead_and_forgets_everything_under_it():
    st = _state()
    b = _cat([_window_batch(w, 100, w) for w in range(5)])
    _insert(st, b)
    ref = _ref_stats(*b)
    got = _got(st.close_below(3))
    assert got == {c: v for c, v in ref.items() if c[1] < 3}
    assert {w for _k, w in st._table} == {3, 4}
    assert _got(st.close_all()) == {c: v for c, v in ref.items() if c[1] >= 3}


def test_snapshot_restore_and_insert_between_closes():
    st = _state()
    batches, got = [], {}
    for w in range(3):
        b = _cat([_window_batch(w, 200, 20 + w), _window_batch(w + 1, 40, 30 + w)])
        batches.append(b)
        _insert(st, b)
        _got(st.close_due(0), got)
    snap = st.snapshot_to_host()
    assert snap["closed_horizon"] == 3
    assert {int(w) for w in snap["wins"]} == {3}
    st2 = _state()
    st2.restore_from_host(snap)
    assert st2.closed_horizon == 3 and st2.max_ts_host == st.max_ts_host
    for w in range(3, 6):
        b = _cat([_window_batch(w, 200, 40 + w), _window_batch(w + 1, 40, 50 + w)])
        batches.append(b)
        _insert(st2, b)
        _got(st2.close_due(0), got)
    _got(st2.close_all(), got)
    assert got == _ref_stats(*_cat(batches))


def test_merge_rows_into_a_state_that_has_closed():
    st = _state()
    b0 = _cat([_window_batch(0, 100, 1), _window_batch(1, 100, 2)])
    _insert(st, b0)
    got = _got(st.close_due(0))
    donor = _state()
    d = _cat([_window_batch(1, 100, 3), _window_batch(2, 100, 4)])
    _insert(donor, d)
    st.merge_rows(donor.snapshot_to_host())
    _got(st.close_below(2), got)
    _got(st.close_all(), got)
    assert got == _ref_stats(*_cat([b0, d]))


def test_late_rows_come_out_once_with_closes_in_between():
    st = _state(track_late=True, wait_ms=0)
    batches, got, late = [], {}, []
    for w in range(4):
        b = _window_batch(w, 200, 60 + w)
        batches.append(b)
        if w >= 2:
            # Events two windows back: below the watermark of the
            # earlier batches, so late.
            lb = _window_batch(w - 2, 30, 70 + w)
            late.append(lb)
            b = _cat([b, lb])
        _insert(st, b)
        _got(st.close_due(), got)
    drained = st.take_late()
    assert st.take_late() is None
    _got(st.close_all(), got)
    assert got == _ref_stats(*_cat(batches))
    want = _cat(late)
    rows = sorted(
        zip(
            drained.keys.tolist(),
            (drained.ts - ALIGN_MS).tolist(),
            drained.vals.tolist(),
        )
    )
    assert rows == sorted(zip(*(a.tolist() for a in want)))
