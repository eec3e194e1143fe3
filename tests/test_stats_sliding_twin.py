"""Sliding stats windows (`SlidingStatsAggState`,
`keyed_stats_agg(offset=...)`) on the CPU twin.

Events are aggregated into panes of ``gcd(length, offset)`` and a close
folds the panes of every due window.  The oracle is a brute-force
group-by over `_SlidingWindowerLogic.intersects`, the host windower;
sums wrap mod 2^64.  Every test checks that no (key, window) comes out
twice, that the closes plus `close_all` equal the oracle, and that each
close returns exactly the windows in ``[old horizon, new horizon)``.
Nothing has a tolerance.
"""

import math
from datetime import datetime, timedelta, timezone

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import bytewax_amd.operators as op  # noqa: E402
import bytewax_amd.operators.windowing as win  # noqa: E402
from bytewax_amd.dataflow import Dataflow  # noqa: E402
from bytewax_amd.gpu import RecordBatch, _ms  # noqa: E402
from bytewax_amd.gpu.operators import keyed_stats_agg  # noqa: E402
from bytewax_amd.gpu.state import (  # noqa: E402
    SlidingStatsAggState,
    StatsAggState,
)
from bytewax_amd.operators.windowing import (  # noqa: E402
    _SlidingWindowerLogic,
    _SlidingWindowerState,
)
from bytewax_amd.testing import TestingSink, TestingSource, run_main  # noqa: E402

ALIGN = datetime(2024, 1, 1, tzinfo=timezone.utc)
ALIGN_MS = _ms(ALIGN)
CPU = torch.device("cpu")
COLS = ("keys", "wins", "cnt", "sum", "min", "max")
#: (len_ms, off_ms): g = 20 s, L = 3, o = 1; g = 5 s, L = 12, o = 5
#: (the offset does not divide the length); tumbling.
GEOMS = [(60_000, 20_000), (60_000, 25_000), (60_000, 60_000)]
OVERLAPPING = GEOMS[:2]


def _wrap64(x):
    return ((x + (1 << 63)) & ((1 << 64) - 1)) - (1 << 63)


def _oracle(len_ms, off_ms, keys, x, vals):
    """{(key, window): (count, sum mod 2^64, min, max)} of events given
    as offsets `x` from the alignment, by the host windower."""
    logic = _SlidingWindowerLogic(
        timedelta(milliseconds=len_ms),
        timedelta(milliseconds=off_ms),
        ALIGN,
        _SlidingWindowerState(),
    )
    ref = {}
    memo = {}
    for k, xi, v in zip(
        np.asarray(keys).tolist(), np.asarray(x).tolist(), np.asarray(vals).tolist()
    ):
        wins = memo.get(xi)
        if wins is None:
            wins = memo[xi] = logic.intersects(
                ALIGN + timedelta(milliseconds=xi)
            )
        for w in wins:
            c, s, mn, mx = ref.get((k, w), (0, 0, v, v))
            ref[(k, w)] = (c + 1, _wrap64(s + v), min(mn, v), max(mx, v))
    return ref


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


def _span_batch(lo_ms, hi_ms, n, seed, n_keys=12):
    """`n` events with offsets in [lo_ms, hi_ms)."""
    rng = np.random.default_rng(seed)
    keys = rng.integers(-n_keys // 2, n_keys // 2, n).astype(np.int32)
    x = rng.integers(lo_ms, hi_ms, n)
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


def _close_checked(st, out_fn, got):
    """Run one close; its rows are exactly the windows between the old
    and the new horizon, and afterwards no dead pane is left."""
    old = st.win_horizon
    out = out_fn()
    rows = _got(out)
    assert all(old <= w < st.win_horizon for _k, w in rows)
    _got(out, got)
    pane_keep = st.win_horizon * st.panes_per_offset
    assert st.closed_horizon == pane_keep or st.win_horizon == old
    assert all(p >= pane_keep for _k, p in st._table)
    return rows


@pytest.mark.parametrize("len_ms,off_ms", GEOMS)
def test_successive_closes_and_close_all_equal_the_oracle(len_ms, off_ms):
    st = SlidingStatsAggState(CPU, ALIGN_MS, len_ms, off_ms)
    assert st.len_ms == math.gcd(len_ms, off_ms)
    batches, got = [], {}
    step = 35_000  # not a multiple of any pane width in GEOMS
    for i in range(12):
        b = _span_batch(i * step, (i + 1) * step, 300, 10 + i)
        batches.append(b)
        _insert(st, b)
        _close_checked(st, lambda: st.close_due(0), got)
        # The due windows are the ones that end at or below the
        # watermark, by the host's own rule.
        wm = st.max_ts_host - ALIGN_MS
        assert st.win_horizon * off_ms + len_ms > wm
        assert (st.win_horizon - 1) * off_ms + len_ms <= wm
    assert len({w for _k, w in got}) >= 6  # many windows were closed
    _close_checked(st, st.close_all, got)
    assert got == _oracle(len_ms, off_ms, *_cat(batches))
    assert st.close_all() is None and not st._table


def test_tumbling_geometry_equals_stats_agg_state_row_for_row():
    a = SlidingStatsAggState(CPU, ALIGN_MS, 60_000, 60_000)
    b = StatsAggState(CPU, ALIGN_MS, 60_000)
    for i in range(6):
        batch = _span_batch(i * 45_000, (i + 1) * 45_000, 250, 40 + i)
        _insert(a, batch)
        _insert(b, batch)
        assert a.horizon_for(a.max_ts_host) == b.horizon_for(b.max_ts_host)
        assert _got(a.close_due(0)) == _got(b.close_due(0))
        assert a.win_horizon == a.closed_horizon == b.closed_horizon
    assert _got(a.close_all()) == _got(b.close_all())


@pytest.mark.parametrize("len_ms,off_ms", OVERLAPPING)
def test_first_panes_open_windows_before_the_alignment(len_ms, off_ms):
    st = SlidingStatsAggState(CPU, ALIGN_MS, len_ms, off_ms)
    b = (np.array([-1, 5], dtype=np.int32), np.array([0, 1]), np.array([7, 9]))
    _insert(st, b)
    got = _got(st.close_all())
    assert got == _oracle(len_ms, off_ms, *b)
    n_back = -(-len_ms // off_ms) - 1  # windows that opened before `align`
    assert {w for _k, w in got} == set(range(-n_back, 1))


@pytest.mark.parametrize("len_ms,off_ms", OVERLAPPING)
def test_close_below_is_none_until_the_horizon_advances(len_ms, off_ms):
    st = SlidingStatsAggState(CPU, ALIGN_MS, len_ms, off_ms)
    assert st.close_due(0) is None
    b = _span_batch(3 * len_ms, 3 * len_ms + 1_000, 50, 3)
    _insert(st, b)
    before = dict(st._table)
    h = st.horizon_for(st.max_ts_host, 0)
    # Nothing is due: every pane lies in open windows only.
    assert st.close_due(0) is None and st.win_horizon == h
    assert st._table == before
    assert st.close_below(h) is None and st.close_below(h - 3) is None
    # A wait holds the horizon back.
    assert st.horizon_for(st.max_ts_host, off_ms) == h - 1
    assert _got(st.close_all()) == _oracle(len_ms, off_ms, *b)


def test_default_wait_is_the_constructors():
    st = SlidingStatsAggState(CPU, ALIGN_MS, 60_000, 20_000, wait_ms=40_000)
    b = _span_batch(0, 200_000, 400, 5)
    _insert(st, b)
    assert st.horizon_for(st.max_ts_host) == st.horizon_for(st.max_ts_host, 40_000)
    got = _got(st.close_due())
    assert st.win_horizon == st.horizon_for(st.max_ts_host, 0) - 2
    assert got and max(w for _k, w in got) == st.win_horizon - 1


@pytest.mark.parametrize("len_ms,off_ms", OVERLAPPING)
def test_snapshot_restore_continues_to_the_same_result(len_ms, off_ms):
    st = SlidingStatsAggState(CPU, ALIGN_MS, len_ms, off_ms)
    batches, got = [], {}
    for i in range(4):
        b = _span_batch(i * 50_000, (i + 1) * 50_000, 200, 20 + i)
        batches.append(b)
        _insert(st, b)
        _close_checked(st, lambda: st.close_due(0), got)
    snap = st.snapshot_to_host()
    assert snap["win_horizon"] == st.win_horizon
    assert (snap["win_len_ms"], snap["off_ms"]) == (len_ms, off_ms)
    assert snap["closed_horizon"] == st.win_horizon * st.panes_per_offset
    st2 = SlidingStatsAggState(CPU, ALIGN_MS, len_ms, off_ms)
    st2.restore_from_host(snap)
    assert st2.win_horizon == st.win_horizon
    assert st2.closed_horizon == st.closed_horizon
    assert st2.max_ts_host == st.max_ts_host and st2._table == st._table
    for i in range(4, 8):
        b = _span_batch(i * 50_000, (i + 1) * 50_000, 200, 20 + i)
        batches.append(b)
        _insert(st2, b)
        _close_checked(st2, lambda: st2.close_due(0), got)
    _close_checked(st2, st2.close_all, got)
    assert got == _oracle(len_ms, off_ms, *_cat(batches))


@pytest.mark.parametrize("len_ms,off_ms", OVERLAPPING)
def test_merge_rows_of_two_donors_with_duplicate_panes(len_ms, off_ms):
    """The pane rows of one stream split across two donors, both
    holding cells of the same (key, pane), merge to the whole."""
    whole = _span_batch(0, 150_000, 600, 7)
    halves = [tuple(a[i::2] for a in whole) for i in range(2)]
    donors = []
    for h in halves:
        d = SlidingStatsAggState(CPU, ALIGN_MS, len_ms, off_ms)
        _insert(d, h)
        donors.append(d.snapshot_to_host())
    assert set(zip(donors[0]["keys"], donors[0]["wins"])) & set(
        zip(donors[1]["keys"], donors[1]["wins"])
    )
    st = SlidingStatsAggState(CPU, ALIGN_MS, len_ms, off_ms)
    st.merge_rows(
        {c: np.concatenate([d[c] for d in donors]) for c in COLS}
    )
    st.max_ts_host = max(d["max_ts"] for d in donors)
    got = {}
    _close_checked(st, lambda: st.close_due(0), got)
    _close_checked(st, st.close_all, got)
    assert got == _oracle(len_ms, off_ms, *whole)


@pytest.mark.parametrize("len_ms,off_ms", OVERLAPPING)
def test_late_rows_come_out_once_and_join_no_window(len_ms, off_ms):
    st = SlidingStatsAggState(
        CPU, ALIGN_MS, len_ms, off_ms, track_late=True, wait_ms=0
    )
    batches, got, late = [], {}, []
    step = 40_000
    for i in range(6):
        b = _span_batch(i * step, (i + 1) * step, 200, 60 + i)
        batches.append(b)
        if i >= 2:
            # Below every event of the batch before, so below the
            # watermark the earlier batches set.
            lb = _span_batch((i - 2) * step, (i - 1) * step, 30, 70 + i)
            late.append(lb)
            # Disordered within the batch as well.
            b = tuple(a[::-1].copy() for a in _cat([b, lb]))
        _insert(st, b)
        _close_checked(st, st.close_due, got)
    drained = st.take_late()
    assert st.take_late() is None
    _close_checked(st, st.close_all, got)
    assert got == _oracle(len_ms, off_ms, *_cat(batches))
    rows = sorted(
        zip(
            drained.keys.tolist(),
            (drained.ts - ALIGN_MS).tolist(),
            drained.vals.tolist(),
        )
    )
    assert rows == sorted(zip(*(a.tolist() for a in _cat(late))))


def test_constructor_rejects_bad_geometries():
    with pytest.raises(ValueError, match="positive"):
        SlidingStatsAggState(CPU, ALIGN_MS, 60_000, 0)
    with pytest.raises(ValueError, match="positive"):
        SlidingStatsAggState(CPU, ALIGN_MS, 60_000, -20_000)
    with pytest.raises(ValueError, match="longer"):
        SlidingStatsAggState(CPU, ALIGN_MS, 60_000, 60_001)
    # gcd 1 s: 65 panes per window.
    with pytest.raises(ValueError, match="65 panes"):
        SlidingStatsAggState(CPU, ALIGN_MS, 65_000, 64_000)
    st = SlidingStatsAggState(CPU, ALIGN_MS, 64_000, 63_000)
    assert st.panes_per_window == 64 and st.panes_per_offset == 63


def test_restore_rejects_another_geometry():
    st = SlidingStatsAggState(CPU, ALIGN_MS, 60_000, 20_000)
    _insert(st, _span_batch(0, 100_000, 100, 1))
    snap = st.snapshot_to_host()
    # Same pane width, another window.
    other = SlidingStatsAggState(CPU, ALIGN_MS, 80_000, 20_000)
    with pytest.raises(ValueError, match="cannot restore"):
        other.restore_from_host(snap)
    assert not other._table
    tumbling = StatsAggState(CPU, ALIGN_MS, 20_000)
    with pytest.raises(ValueError, match="cannot restore"):
        st.restore_from_host(tumbling.snapshot_to_host())
    # The other direction: the rows of a sliding snapshot are panes,
    # which a tumbling state must not take for windows.
    with pytest.raises(ValueError, match="cannot restore"):
        tumbling.restore_from_host(snap)
    assert not tumbling._table


# -- end of input -----------------------------------------------------------


@pytest.mark.parametrize("len_ms,off_ms", OVERLAPPING)
def test_close_eof_leaves_a_state_that_resumes(len_ms, off_ms):
    """`close_eof` returns every window from the horizon up, the
    unfinished ones included, and moves nothing: a snapshot taken after
    it continues the stream, and the windows that were unfinished come
    out again, complete."""
    st = SlidingStatsAggState(CPU, ALIGN_MS, len_ms, off_ms)
    batches, got = [], {}
    for i in range(3):
        b = _span_batch(i * 50_000, (i + 1) * 50_000, 200, 80 + i)
        batches.append(b)
        _insert(st, b)
        _close_checked(st, lambda: st.close_due(0), got)
    horizons = (st.win_horizon, st.closed_horizon)
    table = dict(st._table)
    ref_so_far = _oracle(len_ms, off_ms, *_cat(batches))
    eof = _got(st.close_eof())
    assert eof == {c: v for c, v in ref_so_far.items() if c[1] >= horizons[0]}
    assert (st.win_horizon, st.closed_horizon) == horizons
    assert st._table == table
    assert _got(st.close_eof()) == eof  # and again: nothing moved
    st2 = SlidingStatsAggState(CPU, ALIGN_MS, len_ms, off_ms)
    st2.restore_from_host(st.snapshot_to_host())
    for i in range(3, 6):
        b = _span_batch(i * 50_000, (i + 1) * 50_000, 200, 80 + i)
        batches.append(b)
        _insert(st2, b)
        _close_checked(st2, lambda: st2.close_due(0), got)
    _got(st2.close_eof(), got)
    assert got == _oracle(len_ms, off_ms, *_cat(batches))


# -- rescale ----------------------------------------------------------------


def _rescaled_logic(donor_snaps, len_ms, off_ms):
    """A fresh active shard that merges `donor_snaps` as a change of
    the worker count does."""
    from types import SimpleNamespace

    from bytewax_amd.gpu.operators import _DeviceStatsLogic

    rt = SimpleNamespace(
        rescale_rows=[{"snap": s, "consumed": False} for s in donor_snaps]
    )
    return _DeviceStatsLogic(
        SlidingStatsAggState(CPU, ALIGN_MS, len_ms, off_ms),
        0, False, None, shard="shard-0", world=1, registry=rt,
    )


def _record_batch(batch):
    keys, x, vals = batch
    x = np.asarray(x, dtype=np.int64)
    return RecordBatch(
        torch.from_numpy(np.asarray(keys, dtype=np.int32)),
        torch.from_numpy(ALIGN_MS + x),
        torch.from_numpy(np.asarray(vals, dtype=np.int64)),
        max_ts=int(ALIGN_MS + x.max()),
    )


def test_rescale_does_not_emit_a_closed_window_again():
    """One key, an event every 20 s: after a rescale the panes of
    closed windows that open windows still need must not rebuild the
    closed ones."""
    len_ms, off_ms = 60_000, 20_000
    x = np.arange(5_000, 110_000, 20_000)
    first = (np.zeros(x.size, dtype=np.int32), x, np.ones(x.size, dtype=np.int64))
    st = SlidingStatsAggState(CPU, ALIGN_MS, len_ms, off_ms)
    _insert(st, first)
    got = _got(st.close_due(0))
    assert {w for _k, w in got} == {-2, -1, 0, 1, 2} and st.win_horizon == 3
    logic = _rescaled_logic([st.snapshot_to_host()], len_ms, off_ms)
    more = (np.zeros(1, dtype=np.int32), np.array([125_000]), np.ones(1, dtype=np.int64))
    out, _ = logic.on_batch([_record_batch(more)])
    assert logic.state.win_horizon == 4
    for o in out:
        _got(o, got)  # raises on a window that comes out twice
    for o in logic.on_eof()[0]:
        _got(o, got)
    assert got == _oracle(len_ms, off_ms, *_cat([first, more]))


@pytest.mark.parametrize("len_ms,off_ms", OVERLAPPING)
def test_rescale_of_two_donors_with_different_horizons(len_ms, off_ms):
    """Two old shards with keys of their own, one a few windows behind
    the other: the merged shard adopts the furthest horizon, emits the
    windows the slower donor still owed at once, and continues to the
    oracle with no (key, window) twice."""
    whole = [_span_batch(i * 50_000, (i + 1) * 50_000, 300, 90 + i) for i in range(6)]
    got, snaps, fed = {}, [], []
    for parity, n_fed in ((0, 4), (1, 2)):
        d = SlidingStatsAggState(CPU, ALIGN_MS, len_ms, off_ms)
        for b in whole[:n_fed]:
            mine = tuple(a[b[0] % 2 == parity] for a in b)
            fed.append(mine)
            _insert(d, mine)
            _close_checked(d, lambda: d.close_due(0), got)
        snaps.append(d.snapshot_to_host())
    assert snaps[0]["win_horizon"] > snaps[1]["win_horizon"]
    logic = _rescaled_logic(snaps, len_ms, off_ms)
    for b in whole[4:]:
        fed.append(b)
        out, _ = logic.on_batch([_record_batch(b)])
        for o in out:
            _got(o, got)
        assert logic.state.win_horizon >= snaps[0]["win_horizon"]
    for o in logic.on_eof()[0]:
        _got(o, got)
    assert got == _oracle(len_ms, off_ms, *_cat(fed))


def test_rescale_refuses_a_donor_of_another_geometry():
    st = SlidingStatsAggState(CPU, ALIGN_MS, 80_000, 20_000)
    _insert(st, _span_batch(0, 100_000, 100, 1))
    logic = _rescaled_logic([st.snapshot_to_host()], 60_000, 20_000)
    with pytest.raises(ValueError, match="cannot restore"):
        logic.on_eof()


# -- the operator ---------------------------------------------------------


def _flow_events(n=3_000, n_keys=5, span_ms=400_000, seed=11):
    """Time-ordered events, so the host windower sees none late."""
    rng = np.random.default_rng(seed)
    keys = rng.integers(0, n_keys, n).astype(np.int32)
    x = np.sort(rng.integers(0, span_ms, n))
    vals = rng.integers(-1_000, 1_000, n)
    return keys, x, vals


def _run_device(events, n_batches, **kw):
    keys, x, vals = events
    batches = []
    for ks, xs, vs in zip(
        np.array_split(keys, n_batches),
        np.array_split(x, n_batches),
        np.array_split(vals, n_batches),
    ):
        batches.append(
            RecordBatch(
                torch.from_numpy(ks),
                torch.from_numpy(ALIGN_MS + xs),
                torch.from_numpy(vs.astype(np.int64)),
                max_ts=int(ALIGN_MS + xs.max()),
            )
        )
    out = []
    flow = Dataflow("sliding_stats")
    s = op.input("inp", flow, TestingSource(batches, batch_size=1))
    agg = keyed_stats_agg(
        "stats", s, align_to=ALIGN, device="cpu", slots_pow=12, **kw
    )
    op.output("out", agg, TestingSink(out))
    run_main(flow)
    got = {}
    for o in out:
        _got(o, got)
    return got, out


def _run_host(events, length, offset):
    """min, max and mean per (key, window) through host `fold_window`
    with a `SlidingWindower`."""
    keys, x, vals = events
    items = [
        (str(k), (ALIGN + timedelta(milliseconds=xi), v))
        for k, xi, v in zip(keys.tolist(), x.tolist(), vals.tolist())
    ]
    out = []
    flow = Dataflow("sliding_host")
    s = op.input("inp", flow, TestingSource(items))
    wo = win.fold_window(
        "fold",
        s,
        # A frozen system clock: the watermark is the largest event
        # time alone, as on the device path.
        win.EventClock(
            lambda item: item[0],
            wait_for_system_duration=timedelta(0),
            now_getter=lambda: ALIGN,
            to_system_utc=lambda _t: None,
        ),
        win.SlidingWindower(length=length, offset=offset, align_to=ALIGN),
        lambda: None,
        lambda acc, item: (
            (1, item[1], item[1], item[1])
            if acc is None
            else (
                acc[0] + 1,
                acc[1] + item[1],
                min(acc[2], item[1]),
                max(acc[3], item[1]),
            )
        ),
        lambda a, b: (a[0] + b[0], a[1] + b[1], min(a[2], b[2]), max(a[3], b[3])),
    )
    op.output("out", wo.down, TestingSink(out))
    run_main(flow)
    host = {}
    for k, (w, acc) in out:
        assert (int(k), w) not in host
        host[(int(k), w)] = acc
    return host


@pytest.mark.parametrize("len_ms,off_ms", OVERLAPPING)
def test_operator_matches_host_fold_window(len_ms, off_ms):
    events = _flow_events()
    length = timedelta(milliseconds=len_ms)
    offset = timedelta(milliseconds=off_ms)
    got, out = _run_device(events, 20, length=length, offset=offset)
    assert len(out) > 3  # windows closed while the stream ran
    host = _run_host(events, length, offset)
    assert set(got) == set(host)
    for cell, (c, s, mn, mx) in got.items():
        hc, hs, hmn, hmx = host[cell]
        assert (mn, mx) == (hmn, hmx)
        assert (c, s) == (hc, hs) and s / c == hs / hc  # the mean
    assert got == _oracle(len_ms, off_ms, *events)


def test_operator_without_offset_is_todays_tumbling_output():
    events = _flow_events(seed=12)
    length = timedelta(seconds=60)
    plain, plain_out = _run_device(events, 20, length=length)
    same, same_out = _run_device(events, 20, length=length, offset=length)
    assert plain == same == _oracle(60_000, 60_000, *events)
    # Batch by batch what the tumbling state gives when it is driven
    # by hand, as the operator drove it before.
    st = StatsAggState(CPU, ALIGN_MS, 60_000, slots_pow=12)
    by_hand = []
    keys, x, vals = events
    for ks, xs, vs in zip(*(np.array_split(a, 20) for a in (keys, x, vals))):
        _insert(st, (ks, xs, vs))
        horizon = (st.max_ts_host - ALIGN_MS) // 60_000
        if horizon > st.closed_horizon:
            closed = st.close_below(horizon)
            if closed is not None:
                by_hand.append(closed)
    tail = st.extract(None, clear=True)
    if tail is not None:
        by_hand.append(tail)
    assert len(plain_out) == len(by_hand) == len(same_out)
    for a, b, c in zip(plain_out, by_hand, same_out):
        for col in COLS:
            assert a[col].tolist() == b[col].tolist() == c[col].tolist()
