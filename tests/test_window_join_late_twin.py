"""Late events on the windowed join's CPU twin:
`WindowJoinState(cpu, track_late=True)` against the host classes.

The oracle is the project's own host logic, driven directly: one
`_WindowLogic` over an `EventClock`, a `TumblingWindower` and
`_JoinWindowLogic` per key, fed `(side, value)` items in the fixture's
arrival order (so nothing depends on how the engine interleaves two
inputs).

The host keeps one watermark per key and moves it item by item; the
state keeps one per shard and moves it batch by batch.  The fixture is
built by the three rules of
`tests/windowing/test_columnar_window_late_lowering.py`, with which
the two select the same late set:

- each batch is sorted ascending (stable: duplicates keep their order);
- a batch that advances the maximum ends with one event per key at
  that maximum, on that batch's side;
- an accepted item has `ts >= cutoff >=` the end of every closed
  window, so it can never reach an emitted window.

All comparisons are exact equality of full row sets; late rows are
compared as multisets.
"""

import functools
from collections import Counter
from datetime import datetime, timedelta, timezone

import pytest

torch = pytest.importorskip("torch")

from bytewax_amd.gpu import RecordBatch  # noqa: E402
from bytewax_amd.gpu.state import WindowJoinState  # noqa: E402
from bytewax_amd.operators import _JoinState  # noqa: E402
from bytewax_amd.operators.windowing import (  # noqa: E402
    EventClock,
    TumblingWindower,
    _JoinWindowLogic,
    _WindowLogic,
)

ALIGN = datetime(2024, 1, 1, tzinfo=timezone.utc)
ALIGN_MS = int(ALIGN.timestamp() * 1000)
EPOCH = datetime(1970, 1, 1, tzinfo=timezone.utc)
MS = timedelta(milliseconds=1)
LEN_MS = 60_000
KEYS = 4
WAITS = (0, 30_000)
MODES = ("first", "last")
CPU = torch.device("cpu")

# (side, ((key, seconds after ALIGN), ...)) per batch.  A batch whose
# listed events advance the maximum gets one event per key just above
# it appended (rule two).
_SHAPE = (
    # no late events
    (0, ((0, 3), (1, 10), (2, 18), (3, 25), (1, 44), (0, 50))),
    # no late events; maximum 130 closes window 0 (and 1 under wait 0);
    # the (1, 118) twins tie inside the batch
    (1, ((2, 61), (0, 75), (1, 118), (1, 118), (3, 125), (2, 130))),
    # same side, key and timestamp as an event of the batch before:
    # late with its window open (wait 0), a tie across batches (30 s)
    (1, ((3, 125),)),
    # mixed: 10/45 hit emitted cells, 95..125 are late under wait 0 and
    # 125's window is still open; 105/125 are accepted under wait 30 s
    # although older than 130
    (0, ((1, 10), (2, 45), (3, 95), (0, 105), (1, 125), (2, 131), (0, 180))),
    # right side into window 3 ...
    (1, ((3, 183), (1, 186))),
    # ... then the left side moves the maximum past those stamps while
    # window 3 stays open: the restore pitfall (snapshot after this)
    (0, ((2, 190), (3, 200))),
    # entirely late under both waits (watermark 200)
    (1, ((0, 20), (1, 70), (3, 150), (2, 160), (1, 169))),
    # late + new
    (1, ((2, 100), (0, 165), (1, 205), (3, 260), (0, 300))),
    # late on the left again, and a last window
    (0, ((1, 200), (2, 310), (3, 365))),
)
SNAP_AT = 6  # batches inserted before the mid-stream snapshot


@functools.lru_cache(maxsize=None)
def _batches():
    """Tuple of (side, ((key, abs ts ms, val), ...)), each batch sorted
    ascending by ts; vals are distinct."""
    out, val, wm = [], 1, -1
    for side, shape in _SHAPE:
        events = []
        for k, sec in shape:
            events.append((k, ALIGN_MS + sec * 1000 + 7 * k, val))
            val += 1
        top = max(t for _k, t, _v in events)
        if top > wm:
            top += 50
            for k in range(KEYS):
                events.append((k, top, val))
                val += 1
            wm = top
        out.append((side, tuple(sorted(events, key=lambda e: e[1]))))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _split(wait):
    """Brute force of the batch-granular rule -> (accepted batches,
    late (side, key, ts, val) rows, per-batch late counts, cutoffs)."""
    wm, acc, late, per_batch, cutoffs = 0, [], [], [], []
    for side, batch in _batches():
        cutoff = wm - wait
        cutoffs.append(cutoff)
        keep = tuple(e for e in batch if e[1] >= cutoff)
        late.extend((side,) + e for e in batch if e[1] < cutoff)
        per_batch.append(len(batch) - len(keep))
        acc.append((side, keep))
        wm = max(wm, max(t for _k, t, _v in batch))
    return tuple(acc), tuple(late), tuple(per_batch), tuple(cutoffs)


def _win(t):
    return (t - ALIGN_MS) // LEN_MS


@pytest.mark.parametrize("wait", WAITS)
def test_fixture_has_the_cases(wait):
    batches = _batches()
    _acc, late, per_batch, cutoffs = _split(wait)
    emitted_hit = open_window = old_accepted = False
    cells = set()
    wm = 0
    for (side, batch), cutoff in zip(batches, cutoffs):
        closed = {
            (k, wn) for k, wn in cells
            if wn * LEN_MS + ALIGN_MS + LEN_MS <= cutoff
        }
        for k, t, _v in batch:
            if t < cutoff:
                # a late event whose cell was already emitted
                emitted_hit |= (k, _win(t)) in closed
                # a late event whose window is still open
                open_window |= _win(t) * LEN_MS + ALIGN_MS + LEN_MS > cutoff
            else:
                # accepted, older than an earlier batch's maximum
                old_accepted |= t < wm
                cells.add((k, _win(t)))
        wm = max(wm, max(t for _k, t, _v in batch))
    assert emitted_hit and open_window
    # Needs room between cutoff and watermark.
    assert old_accepted == (wait > 0)
    assert 0 in per_batch
    assert any(n == len(b) for n, (_s, b) in zip(per_batch, batches))
    assert {row[0] for row in late} == {0, 1}
    # Ties: inside one batch, and across two batches of one side.
    s1, b1 = batches[1]
    assert len({(k, t) for k, t, _v in b1}) < len(b1)
    s2, b2 = batches[2]
    assert s1 == s2 and {(k, t) for k, t, _v in b2} <= {
        (k, t) for k, t, _v in b1
    }


@functools.lru_cache(maxsize=None)
def _host(mode, wait):
    """(down rows, late rows) of the host logic: down as sorted
    (key, window, mask, v0, v1), late as a Counter of
    (side, key, ts, val)."""
    clock = EventClock(
        ts_getter=lambda side_item: side_item[1][0],
        wait_for_system_duration=wait * MS,
        # A frozen system clock: the watermark moves with event time.
        now_getter=lambda: ALIGN,
    )
    windower = TumblingWindower(align_to=ALIGN, length=LEN_MS * MS)

    def builder(_resume):
        return _JoinWindowLogic(mode, "final", _JoinState.for_side_count(2))

    logics = {
        k: _WindowLogic(
            clock.build(None), windower.build(None), builder, ordered=True
        )
        for k in range(KEYS)
    }
    events = {k: [] for k in range(KEYS)}
    for side, batch in _batches():
        for k in range(KEYS):
            items = [
                (side, (EPOCH + t * MS, kk, v)) for kk, t, v in batch if kk == k
            ]
            if items:
                events[k].extend(logics[k].on_batch(items)[0])
    for k in range(KEYS):
        events[k].extend(logics[k].on_eof()[0])
    down, late = [], Counter()
    for k, evs in events.items():
        for wid, typ, obj in evs:
            if typ == "E":
                i0, i1 = obj
                down.append(
                    (
                        k,
                        wid,
                        (i0 is not None) | 2 * (i1 is not None),
                        i0[2] if i0 is not None else 0,
                        i1[2] if i1 is not None else 0,
                    )
                )
            elif typ == "L":
                side, item = obj
                late[(side, k, (item[0] - EPOCH) // MS, item[2])] += 1
    return sorted(down), late


def _rb(batch):
    return RecordBatch(
        torch.tensor([k for k, _t, _v in batch], dtype=torch.int32),
        torch.tensor([t for _k, t, _v in batch], dtype=torch.int64),
        torch.tensor([v for _k, _t, v in batch], dtype=torch.int64),
    )


def _state(mode, wait, **kw):
    return WindowJoinState(
        CPU, ALIGN_MS, LEN_MS, mode, slots_pow=10, out_cap=1 << 10,
        wait_ms=wait, **kw
    )


def _rows(out, into):
    if out is not None:
        into.extend(
            zip(*(out[c].tolist() for c in ("keys", "wins", "mask", "v0", "v1")))
        )


def _late_rows(st, into):
    for side in (0, 1):
        rb = st.take_late(side)
        if rb is None:
            continue
        assert rb.ts.dtype == torch.int64 and rb.ts_base == 0
        into.update(
            (side, k, t, v)
            for k, t, v in zip(
                rb.keys.tolist(), rb.ts.tolist(), rb.vals.tolist()
            )
        )


def _drive(st, batches, rows, late):
    for side, batch in batches:
        st.insert(side, _rb(batch))
        _rows(st.close_due(), rows)
        _late_rows(st, late)


def _finish(st, rows, late):
    _rows(st.close_eof(), rows)
    _late_rows(st, late)
    cells = [r[:2] for r in rows]
    assert len(set(cells)) == len(cells), "a cell came out twice"
    return sorted(rows), late


@pytest.mark.parametrize("wait", WAITS)
@pytest.mark.parametrize("mode", MODES)
def test_twin_matches_host(mode, wait):
    st = _state(mode, wait, track_late=True)
    rows, late = [], Counter()
    _drive(st, _batches(), rows, late)
    rows, late = _finish(st, rows, late)
    h_rows, h_late = _host(mode, wait)
    assert len(h_rows) > 10 and sum(h_late.values()) > 5
    assert rows == h_rows
    assert late == h_late
    # And the brute force of the rule.
    _acc, o_late, _pb, _cut = _split(wait)
    assert late == Counter(o_late)
    assert st.take_late(0) is None and st.take_late(1) is None


def test_without_track_late_nothing_is_reported():
    st = _state("last", 0)
    assert st.track_late is False
    for side, batch in _batches()[:4]:
        st.insert(side, _rb(batch))
    assert st.take_late(0) is None and st.take_late(1) is None
    assert not st.late_drained()


@pytest.mark.parametrize("wait", WAITS)
@pytest.mark.parametrize("mode", MODES)
def test_snapshot_restore_midstream(mode, wait):
    """The snapshot holds a right-side stamp of an open window below
    ``max_ts - wait``: a restore that classified would call it late."""
    batches = _batches()
    whole = _state(mode, wait, track_late=True)
    rows, late = [], Counter()
    _drive(whole, batches, rows, late)
    ref = _finish(whole, rows, late)

    first = _state(mode, wait, track_late=True)
    rows, late = [], Counter()
    _drive(first, batches[:SNAP_AT], rows, late)
    snap = first.snapshot_to_host()
    assert snap["track_late"] is True
    horizon = first.horizon_for(snap["max_ts"])
    assert any(
        (m & 2) and t1 < snap["max_ts"] - wait and w >= horizon
        for m, t1, w in zip(
            snap["mask"].tolist(), snap["t1"].tolist(), snap["wins"].tolist()
        )
    )
    resumed = _state(mode, wait, track_late=True)
    resumed.restore_from_host(snap)
    assert resumed.take_late(0) is None and resumed.take_late(1) is None
    assert resumed.snapshot_to_host()["n"] == snap["n"]
    _drive(resumed, batches[SNAP_AT:], rows, late)
    assert _finish(resumed, rows, late) == ref
    assert ref == _host(mode, wait)


def test_track_late_mismatch():
    tracked = _state("last", 0, track_late=True)
    plain = _state("last", 0)
    for side, batch in _batches()[:2]:
        tracked.insert(side, _rb(batch))
        plain.insert(side, _rb(batch))
    # A snapshot taken with late tracking needs a state that tracks.
    with pytest.raises(ValueError, match="track_late"):
        _state("last", 0).restore_from_host(tracked.snapshot_to_host())
    # One taken without restores into either kind.
    snap = plain.snapshot_to_host()
    assert snap["track_late"] is False
    for kw in ({}, {"track_late": True}):
        st = _state("last", 0, **kw)
        st.restore_from_host(snap)
        assert st.snapshot_to_host()["n"] == snap["n"] > 0
    # So does one from before the field existed.
    del snap["track_late"]
    _state("last", 0).restore_from_host(snap)
