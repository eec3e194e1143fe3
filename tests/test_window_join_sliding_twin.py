"""The sliding windowed join of the columnar path on the CPU: the dict
twin of `SlidingWindowJoinState` and `window_join(offset=...)` on
``device="cpu"``.

The twin is pinned to the host `join_window` (EventClock,
SlidingWindower, ``ordered=True``, "final" emit), run over the same
events as Python objects, and to a small oracle that knows nothing of
panes: per (key, window, side) it picks the maximum ("last") or minimum
("first") of ``(ts, global arrival index)`` over the events the window
covers.  Every comparison is exact equality of the full set of
(key, window id, v0-or-None, v1-or-None) rows over the whole stream,
EOF included, and no (key, window) may come out twice across the closes
of a run.
"""

from datetime import datetime, timedelta, timezone

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import bytewax_amd.operators as op  # noqa: E402
import bytewax_amd.operators.windowing as win  # noqa: E402
from bytewax_amd.dataflow import Dataflow  # noqa: E402
from bytewax_amd.gpu import RecordBatch, _ms  # noqa: E402
from bytewax_amd.gpu.operators import window_join  # noqa: E402
from bytewax_amd.gpu.state import (  # noqa: E402
    SlidingWindowJoinState,
    WindowJoinState,
)
from bytewax_amd.testing import TestingSink, TestingSource, run_main  # noqa: E402

ALIGN = datetime(2024, 1, 1, tzinfo=timezone.utc)
ALIGN_MS = _ms(ALIGN)
CPU = torch.device("cpu")
MODES = ("first", "last")
#: (length, offset) in ms: L=3 o=1; g=5 L=12 o=5; L=64 o=1; L=1.
GEOMS = ((30, 10), (60, 25), (64, 1), (20, 20))


def _step(len_ms, off_ms):
    """Time a stream advances per step; `_stream` needs a wait of two."""
    return max(off_ms, len_ms // 4)


def _windows(x, len_ms, off_ms):
    """The window ids that cover offset `x` from the alignment."""
    return range((x - len_ms) // off_ms + 1, x // off_ms + 1)


def _oracle(batches, mode, len_ms, off_ms):
    """{(key, window): (v0 or None, v1 or None)} of `batches`, a list
    of (side, keys, x, vals) in arrival order with `x` the offsets from
    the alignment."""
    best = {}
    arrival = 0
    for side, keys, x, vals in batches:
        for k, t, v in zip(
            np.asarray(keys).tolist(),
            np.asarray(x).tolist(),
            np.asarray(vals).tolist(),
        ):
            cand = ((t, arrival), v)
            for w in _windows(t, len_ms, off_ms):
                cur = best.get((k, w, side))
                if (
                    cur is None
                    or (mode == "last" and cand[0] > cur[0])
                    or (mode == "first" and cand[0] < cur[0])
                ):
                    best[(k, w, side)] = cand
            arrival += 1
    rows = {}
    for (k, w, side), (_rank, v) in best.items():
        row = list(rows.get((k, w), (None, None)))
        row[side] = v
        rows[(k, w)] = tuple(row)
    return rows


def _host(batches, mode, len_ms, off_ms):
    """The same rows from the host `join_window` over the events as
    Python objects, each side in its arrival order; the clock waits
    longer than the stream lasts, so nothing is late."""

    def items(side):
        return [
            (str(k), (ALIGN + timedelta(milliseconds=t), v))
            for s, keys, x, vals in batches
            if s == side
            for k, t, v in zip(
                np.asarray(keys).tolist(),
                np.asarray(x).tolist(),
                np.asarray(vals).tolist(),
            )
        ]

    down, late = [], []
    flow = Dataflow("host_join")
    a = op.input("a", flow, TestingSource(items(0)))
    b = op.input("b", flow, TestingSource(items(1)))
    clock = win.EventClock(
        ts_getter=lambda x: x[0],
        wait_for_system_duration=timedelta(days=1),
    )
    windower = win.SlidingWindower(
        align_to=ALIGN,
        length=timedelta(milliseconds=len_ms),
        offset=timedelta(milliseconds=off_ms),
    )
    wo = win.join_window(
        "jw", clock, windower, a, b,
        insert_mode=mode, emit_mode="final", ordered=True,
    )
    op.output("down", wo.down, TestingSink(down))
    op.output("late", wo.late, TestingSink(late))
    run_main(flow)
    assert late == []
    rows = {}
    for k, (w, (l, r)) in down:
        assert (int(k), w) not in rows
        rows[(int(k), w)] = (
            None if l is None else l[1],
            None if r is None else r[1],
        )
    return rows


def _batch(keys, x, vals, device=CPU):
    x = np.asarray(x, dtype=np.int64)
    return RecordBatch(
        torch.from_numpy(np.asarray(keys, dtype=np.int32)).to(device),
        torch.from_numpy(ALIGN_MS + x).to(device),
        torch.from_numpy(np.asarray(vals, dtype=np.int64)).to(device),
        max_ts=int(ALIGN_MS + x.max()) if x.size else None,
    )


def _rows(out, into):
    """Add the rows of one close to `into`; no (key, window) twice."""
    if out is None:
        return into
    cols = (out[c].cpu().tolist() for c in ("keys", "wins", "mask", "v0", "v1"))
    for k, w, m, v0, v1 in zip(*cols):
        assert (k, w) not in into, f"cell {(k, w)} emitted twice"
        assert m in (1, 2, 3)
        into[(k, w)] = (v0 if m & 1 else None, v1 if m & 2 else None)
    return into


def _stream(seed, len_ms, off_ms, steps=12, n_keys=10, per_batch=30):
    """`2 * steps` batches, the sides in turn.  Step `i` of either side
    draws its timestamps from a few values in ``[i * step, (i + 2) *
    step)``: consecutive steps overlap, so batches are disordered by up
    to two steps (what the wait has to cover), and ties within a batch,
    across the batches of a side and across the sides abound.  Step 0
    holds the very first millisecond, whose windows reach back before
    the alignment."""
    rng = np.random.default_rng(seed)
    step = _step(len_ms, off_ms)
    batches = []
    for i in range(steps):
        marks = i * step + rng.choice(2 * step, min(6, 2 * step), replace=False)
        if i == 0:
            marks[0] = 0
        for side in (0, 1):
            # Side 1 never sees key 0, side 0 never key 1.
            keys = rng.integers(0, n_keys, per_batch)
            keys = keys[keys != (1 - side)]
            x = rng.choice(marks, keys.size)
            if i == 0:
                x[0] = 0
            batches.append(
                (
                    side,
                    keys.astype(np.int32),
                    x,
                    rng.integers(-(1 << 62), 1 << 62, keys.size),
                )
            )
    return batches


def _state(mode, len_ms, off_ms, wait_ms=None, **kw):
    if wait_ms is None:
        wait_ms = 2 * _step(len_ms, off_ms)
    return SlidingWindowJoinState(
        CPU, ALIGN_MS, len_ms, off_ms, mode, wait_ms=wait_ms, **kw
    )


def _drive(st, batches, start=0, rows=None):
    """Insert `batches[start:]` with a `close_due` after each, then
    close at EOF; the union of the rows."""
    rows = {} if rows is None else rows
    for side, keys, x, vals in batches[start:]:
        st.insert(side, _batch(keys, x, vals))
        _rows(st.close_due(), rows)
    _rows(st.close_eof(), rows)
    return rows


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("geom", GEOMS)
def test_twin_matches_host_join_window(mode, geom):
    """A disordered stream with ties, one-sided keys and events in the
    first pane, closed along the way with a wait that covers the
    disorder: the host's rows."""
    len_ms, off_ms = geom
    batches = _stream(7, len_ms, off_ms)
    st = _state(mode, len_ms, off_ms)
    rows = {}
    closes = 0
    for side, keys, x, vals in batches:
        st.insert(side, _batch(keys, x, vals))
        out = st.close_due()
        closes += out is not None
        _rows(out, rows)
    _rows(st.close_eof(), rows)
    assert closes >= 5  # closed along the way, not only at EOF
    assert rows == _host(batches, mode, len_ms, off_ms)
    assert rows == _oracle(batches, mode, len_ms, off_ms)
    assert {(a is None, b is None) for a, b in rows.values()} == {
        (False, False), (False, True), (True, False),
    }
    # The first millisecond lies in windows that open before `align`.
    assert min(w for _k, w in rows) == -len_ms // off_ms + 1
    assert (st.panes_per_window, st.panes_per_offset) == {
        (30, 10): (3, 1), (60, 25): (12, 5), (64, 1): (64, 1), (20, 20): (1, 1),
    }[geom]


@pytest.mark.parametrize("mode", MODES)
def test_one_pane_per_window_is_the_tumbling_join(mode):
    """20 ms every 20 ms: every close returns the rows of
    `WindowJoinState`, row for row."""
    batches = _stream(3, 20, 20)
    sl = _state(mode, 20, 20)
    tb = WindowJoinState(CPU, ALIGN_MS, 20, mode, wait_ms=sl.wait_ms)

    def norm(out):
        if out is None:
            return None
        cols = [out[c].tolist() for c in ("keys", "wins", "mask", "v0", "v1")]
        return sorted(zip(*cols))

    some = 0
    for side, keys, x, vals in batches:
        sl.insert(side, _batch(keys, x, vals))
        tb.insert(side, _batch(keys, x, vals))
        a, b = norm(sl.close_due()), norm(tb.close_due())
        assert a == b
        some += a is not None
        assert (sl.win_horizon, sl.closed_horizon) == (
            tb.closed_horizon, tb.closed_horizon,
        )
    assert some >= 5
    assert norm(sl.close_eof()) == norm(tb.close_eof())


@pytest.mark.parametrize("mode", MODES)
def test_sides_in_different_panes(mode):
    """Key 1 has its left side in pane 0 and its right side in pane 2:
    they meet in window 0 (panes 0..2) alone.  Key 2 has two left
    events in different panes of window 0."""
    batches = [
        (0, [1, 2, 2], [3, 4, 25], [10, 20, 21]),
        (1, [1], [27], [30]),
    ]
    st = _state(mode, 30, 10, wait_ms=0)
    got = _drive(st, batches)
    assert got == _oracle(batches, mode, 30, 10)
    assert got == _host(batches, mode, 30, 10)
    assert got[(1, 0)] == (10, 30)
    assert got[(1, -1)] == (10, None) and got[(1, 1)] == (None, 30)
    assert got[(2, 0)] == ((21 if mode == "last" else 20), None)
    assert got[(2, 1)] == (21, None)


@pytest.mark.parametrize("mode", MODES)
def test_ties_within_and_across_batches(mode):
    """Equal timestamps in one batch and in two, next to an event in
    another pane of the same window that does or does not beat them."""
    t = 12
    batches = [
        (0, [1, 1, 1, 2], [t, t, t, t], [10, 11, 12, 20]),
        (0, [1, 2, 2], [t, t - 10, t + 10], [13, 21, 22]),
        (1, [1, 1], [t, t], [30, 31]),
        (1, [1], [t], [32]),
    ]
    st = _state(mode, 30, 10, wait_ms=30)
    got = _drive(st, batches)
    assert got == _oracle(batches, mode, 30, 10)
    assert got == _host(batches, mode, 30, 10)
    # Window 1 is [10, 40): key 1 holds the tie alone; key 2 has the
    # tie and a later event.
    assert got[(1, 1)] == ((13, 32) if mode == "last" else (10, 30))
    assert got[(2, 1)] == ((22 if mode == "last" else 20), None)
    # Window 0 is [0, 30): key 2 has an earlier event and the tie.
    assert got[(2, 0)] == ((22 if mode == "last" else 21), None)


def _late_stream(seed, len_ms, off_ms, wait_ms):
    """A stream whose every third step reaches back past the wait."""
    rng = np.random.default_rng(seed)
    batches = _stream(seed, len_ms, off_ms, steps=10)
    out = []
    for i, (side, keys, x, vals) in enumerate(batches):
        x = x.copy()
        if i >= 6 and i % 3 == 0:
            back = rng.integers(0, x.size, 5)
            x[back] = np.maximum(x[back] - wait_ms - 2 * len_ms, 0)
        out.append((side, keys, x, vals))
    return out


def _split_late(batches, wait_ms):
    """The batch-granular late rule: an event is late iff it lies below
    the greatest timestamp of the earlier batches (of either side)
    minus the wait.  Returns the accepted batches and the late
    (key, x, val) rows per side."""
    accepted, late = [], ([], [])
    seen = None
    for side, keys, x, vals in batches:
        keys, x, vals = (np.asarray(c) for c in (keys, x, vals))
        is_late = (
            np.zeros(x.size, bool) if seen is None else x < seen - wait_ms
        )
        late[side].extend(
            zip(keys[is_late].tolist(), x[is_late].tolist(), vals[is_late].tolist())
        )
        accepted.append((side, keys[~is_late], x[~is_late], vals[~is_late]))
        if x.size:
            seen = int(x.max()) if seen is None else max(seen, int(x.max()))
    return accepted, late


def _take_late(st, side, into):
    lb = st.take_late(side)
    if lb is not None:
        into[side].extend(
            zip(
                lb.keys.tolist(),
                (lb.ts.to(torch.int64) + lb.ts_base - ALIGN_MS).tolist(),
                lb.vals.tolist(),
            )
        )


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("geom", [(30, 10), (60, 25)])
def test_track_late(mode, geom):
    """With late tracking the late rows come out once, per side, and
    the windows are the host's over the accepted events."""
    len_ms, off_ms = geom
    wait_ms = 2 * _step(len_ms, off_ms)
    batches = _late_stream(5, len_ms, off_ms, wait_ms)
    accepted, want_late = _split_late(batches, wait_ms)
    assert want_late[0] and want_late[1]
    st = _state(mode, len_ms, off_ms, track_late=True)
    rows, late = {}, ([], [])
    for side, keys, x, vals in batches:
        st.insert(side, _batch(keys, x, vals))
        _take_late(st, side, late)
        _rows(st.close_due(), rows)
    _rows(st.close_eof(), rows)
    for side in (0, 1):
        _take_late(st, side, late)
        assert sorted(late[side]) == sorted(want_late[side])
    assert rows == _oracle(accepted, mode, len_ms, off_ms)
    assert rows == _host(accepted, mode, len_ms, off_ms)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("geom", [(30, 10), (60, 25)])
def test_close_eof_then_continue_and_restore(mode, geom):
    """`close_eof` reports every window still owed and moves nothing:
    the stream continues, in the same state or in one restored from a
    snapshot taken after it, as if it had not been called."""
    len_ms, off_ms = geom
    batches = _stream(13, len_ms, off_ms)
    want = _oracle(batches, mode, len_ms, off_ms)
    k = 11
    st = _state(mode, len_ms, off_ms)
    rows = {}
    for side, keys, x, vals in batches[:k]:
        st.insert(side, _batch(keys, x, vals))
        _rows(st.close_due(), rows)
    horizons = (st.win_horizon, st.closed_horizon)
    live = dict(st._table)
    at_eof = _rows(st.close_eof(), {})
    so_far = _oracle(batches[:k], mode, len_ms, off_ms)
    assert at_eof == {
        kw: v for kw, v in so_far.items() if kw[1] >= st.win_horizon
    }
    assert at_eof and not set(at_eof) & set(rows)
    assert (st.win_horizon, st.closed_horizon) == horizons
    assert st._table == live
    snap = st.snapshot_to_host()
    assert snap["n"] == len(live)
    assert (snap["win_horizon"], snap["win_len_ms"], snap["off_ms"]) == (
        horizons[0], len_ms, off_ms,
    )

    assert _drive(st, batches, start=k, rows=dict(rows)) == want
    st2 = _state(mode, len_ms, off_ms)
    st2.restore_from_host(snap)
    assert (st2.win_horizon, st2.closed_horizon) == horizons
    assert _drive(st2, batches, start=k, rows=dict(rows)) == want


@pytest.mark.parametrize("mode", MODES)
def test_close_all(mode):
    batches = _stream(2, 30, 10, steps=4)
    st = _state(mode, 30, 10)
    rows = {}
    for side, keys, x, vals in batches:
        st.insert(side, _batch(keys, x, vals))
        _rows(st.close_due(), rows)
    _rows(st.close_all(), rows)
    assert rows == _oracle(batches, mode, 30, 10)
    assert st._table == {}
    assert st.close_all() is None


def test_refused_snapshots():
    batches = _stream(1, 30, 10, steps=3)
    st = _state("last", 30, 10)
    for side, keys, x, vals in batches:
        st.insert(side, _batch(keys, x, vals))
    snap = st.snapshot_to_host()
    # Another geometry, also one with the same pane width.
    for len_ms, off_ms in ((60, 10), (30, 15), (40, 10)):
        with pytest.raises(ValueError, match="cannot restore a state of"):
            _state("last", len_ms, off_ms).restore_from_host(snap)
    with pytest.raises(ValueError, match="cannot restore"):
        _state("first", 30, 10).restore_from_host(snap)
    # Sliding into tumbling, also where the pane is the tumbling length.
    for len_ms in (30, 10):
        tb = WindowJoinState(CPU, ALIGN_MS, len_ms, "last")
        with pytest.raises(
            ValueError, match="sliding window join .* cannot restore a tumbling"
        ):
            tb.restore_from_host(snap)
    # Tumbling into sliding.
    tb = WindowJoinState(CPU, ALIGN_MS, 10, "last")
    tb.insert(0, _batch([1], [5], [1]))
    with pytest.raises(
        ValueError, match="tumbling window join cannot restore a sliding"
    ):
        _state("last", 30, 10).restore_from_host(tb.snapshot_to_host())


def test_value_errors():
    def build(len_ms, off_ms):
        return SlidingWindowJoinState(CPU, ALIGN_MS, len_ms, off_ms)

    with pytest.raises(ValueError, match="`off_ms` must be positive"):
        build(30, 0)
    with pytest.raises(ValueError, match="`off_ms` must be positive"):
        build(30, -10)
    with pytest.raises(ValueError, match="can't be longer than `len_ms`"):
        build(30, 40)
    with pytest.raises(ValueError, match="needs 65 panes of 1 ms"):
        build(65, 64)
    with pytest.raises(ValueError, match="at most 64 are supported"):
        build(130, 2)
    with pytest.raises(ValueError, match="not supported"):
        SlidingWindowJoinState(CPU, ALIGN_MS, 30, 10, "product")
    st = build(128, 2)
    assert (st.panes_per_window, st.panes_per_offset, st.len_ms) == (64, 1, 2)
    assert st.MAX_PANES == 64


def _run_operator(batches, mode, len_ms, off_ms, device="cpu", **kw):
    out = []
    flow = Dataflow("wj")
    dev = torch.device(device)
    left = op.input(
        "l", flow,
        TestingSource([_batch(*b[1:], dev) for b in batches if b[0] == 0]),
    )
    right = op.input(
        "r", flow,
        TestingSource([_batch(*b[1:], dev) for b in batches if b[0] == 1]),
    )
    joined = window_join(
        "join", left, right, ALIGN, timedelta(milliseconds=len_ms),
        wait=timedelta(milliseconds=2 * _step(len_ms, off_ms)),
        insert_mode=mode, device=device,
        offset=timedelta(milliseconds=off_ms), **kw,
    )
    op.output("out", joined, TestingSink(out))
    run_main(flow)
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("geom", [(30, 10), (60, 25)])
def test_operator_cpu(mode, geom):
    """`window_join(offset=...)` on ``device="cpu"`` through `run_main`
    equals the host `join_window`."""
    len_ms, off_ms = geom
    batches = _stream(17, len_ms, off_ms)
    out = _run_operator(batches, mode, len_ms, off_ms)
    rows = {}
    for d in out:
        _rows(d, rows)
    assert len(out) > 2  # closed along the way, not only at EOF
    assert rows == _host(batches, mode, len_ms, off_ms)


def test_operator_offset_equal_to_length_tumbles():
    batches = _stream(19, 20, 20)
    rows = {}
    for d in _run_operator(batches, "last", 20, 20):
        _rows(d, rows)
    assert rows == _drive(
        WindowJoinState(CPU, ALIGN_MS, 20, "last", wait_ms=40), batches
    )


def test_operator_build_time_errors():
    def build(length, offset):
        flow = Dataflow("wj_err")
        left = op.input("l", flow, TestingSource([]))
        right = op.input("r", flow, TestingSource([]))
        window_join(
            "join", left, right, ALIGN, length, device="cpu", offset=offset,
            fold_slots_pow=8,
        )

    ms = timedelta(milliseconds=1)
    build(30 * ms, 10 * ms)
    build(30 * ms, 30 * ms)
    with pytest.raises(ValueError, match="must be positive"):
        build(30 * ms, 0 * ms)
    with pytest.raises(ValueError, match="can't be longer"):
        build(30 * ms, 31 * ms)
    with pytest.raises(ValueError, match="needs 65 panes"):
        build(65 * ms, 64 * ms)
