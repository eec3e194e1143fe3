"""The columnar lowering of `win.join_window`: two sides of
RecordBatches, `EventClock`, `TumblingWindower`, "first"/"last"
insert, "final" emit, ordered -> `WindowJoinState(track_late=True)`.

The late set of two interleaved inputs depends on their arrival order,
so the end-to-end stream is made invariant under any interleaving
that keeps the sides within one step of each other.  With
``wait = 2 * length``, step `i`'s on-time events in window `i` and its
late events in windows `<= i - 4`:

- before batch `i` of a side, that side's batch `i - 1` has been seen,
  so the cutoff is `>= (i - 1) * length - wait = (i - 3) * length`:
  every event of a window `<= i - 4` is late;
- the newest batch that can have been seen is the other side's step
  `i + 1`, so the cutoff is `< (i + 2) * length - wait = i * length`:
  every event of window `i` is accepted.

All comparisons are exact equality of full row sets; late rows are
compared as multisets.
"""

import functools
from collections import Counter
from datetime import datetime, timedelta, timezone

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import bytewax_amd.operators as op  # noqa: E402
import bytewax_amd.operators.windowing as win  # noqa: E402
from bytewax_amd.dataflow import Dataflow  # noqa: E402
from bytewax_amd.gpu import RecordBatch  # noqa: E402
from bytewax_amd.operators.windowing import (  # noqa: E402
    COLUMNAR_WINDOW_ID,
    EventClock,
    SessionWindower,
    SlidingWindower,
    SystemClock,
    TumblingWindower,
    _ColumnarJoinLogic,
    _ColumnarJoinSpec,
    _ColumnarSpec,
    _join_device_mode,
)
from bytewax_amd.testing import TestingSink, TestingSource, run_main  # noqa: E402

ALIGN = datetime(2024, 1, 1, tzinfo=timezone.utc)
ALIGN_MS = int(ALIGN.timestamp() * 1000)
MS = timedelta(milliseconds=1)
LEN_MS = 60_000
WAIT_MS = 2 * LEN_MS
STEPS, KEYS = 9, 6
MODES = ("first", "last")


@functools.lru_cache(maxsize=None)
def _stream():
    """Per side, `STEPS` batches of (keys, offsets from ALIGN, vals,
    late flags) as numpy arrays.  Timestamps come from a few marks per
    window, so ties within and across batches abound; vals are
    distinct."""
    rng = np.random.default_rng(11)
    sides = ([], [])
    val = 1
    for i in range(STEPS):
        marks = i * LEN_MS + rng.choice(LEN_MS, 5, replace=False)
        for side in (0, 1):
            n = 20
            keys = rng.integers(0, KEYS, n)
            x = rng.choice(marks, n)
            is_late = np.zeros(n, dtype=bool)
            if i >= 4:
                # Windows <= i - 4: emitted ones, and (i - 4) whose
                # close may or may not have run yet.
                m = 3 + (i + side) % 3
                lw = rng.integers(0, i - 3, m)
                keys = np.r_[keys, rng.integers(0, KEYS, m)]
                x = np.r_[x, lw * LEN_MS + rng.integers(0, LEN_MS, m)]
                is_late = np.r_[is_late, np.ones(m, dtype=bool)]
                order = rng.permutation(keys.size)
                keys, x, is_late = keys[order], x[order], is_late[order]
            vals = np.arange(val, val + keys.size)
            val += keys.size
            sides[side].append((keys, x, vals, is_late))
    return sides


@functools.lru_cache(maxsize=None)
def _expected(mode):
    """(rows, late) by brute force: the accepted events' winners per
    (key, window, side) by (ts, arrival within the side), as sorted
    (key, window, mask, v0, v1); late as a Counter of
    (side, key, abs ts, val)."""
    best, late = {}, Counter()
    for side, batches in enumerate(_stream()):
        arrival = 0
        for keys, x, vals, is_late in batches:
            for k, t, v, lt in zip(
                keys.tolist(), x.tolist(), vals.tolist(), is_late.tolist()
            ):
                arrival += 1
                if lt:
                    late[(side, k, ALIGN_MS + t, v)] += 1
                    continue
                cell = (k, t // LEN_MS, side)
                cand = ((t, arrival), v)
                cur = best.get(cell)
                if (
                    cur is None
                    or (mode == "last" and cand[0] > cur[0])
                    or (mode == "first" and cand[0] < cur[0])
                ):
                    best[cell] = cand
    cells = {}
    for (k, w, side), (_rank, v) in best.items():
        m, v0, v1 = cells.get((k, w), (0, 0, 0))
        cells[(k, w)] = (
            m | (1 << side), v if side == 0 else v0, v if side == 1 else v1
        )
    return sorted((k, w) + c for (k, w), c in cells.items()), late


def _rb(keys, x, vals, device):
    return RecordBatch(
        torch.from_numpy(keys.astype(np.int32)).to(device),
        torch.from_numpy(ALIGN_MS + x.astype(np.int64)).to(device),
        torch.from_numpy(vals.astype(np.int64)).to(device),
    )


def _clock(wait_ms=WAIT_MS):
    return EventClock(
        ts_getter=lambda it: it,
        wait_for_system_duration=wait_ms * MS,
        now_getter=lambda: ALIGN,
    )


def _tumbling():
    return TumblingWindower(align_to=ALIGN, length=LEN_MS * MS)


def _down_rows(cols, device, into):
    assert sorted(cols) == ["keys", "mask", "v0", "v1", "wins"]
    for t in cols.values():
        assert t.device.type == torch.device(device).type
    into.extend(
        zip(*(cols[c].cpu().tolist() for c in ("keys", "wins", "mask", "v0", "v1")))
    )


def _late_rows(side_rb, device, into):
    side, rb = side_rb
    assert side in (0, 1)
    assert rb.ts.dtype == torch.int64 and rb.ts_base == 0
    if device is not None:
        assert rb.keys.device.type == torch.device(device).type
    into.update(
        (side, k, t, v)
        for k, t, v in zip(
            rb.keys.cpu().tolist(), rb.ts.cpu().tolist(), rb.vals.cpu().tolist()
        )
    )


def _end_to_end(mode, device):
    down, late, meta = [], [], []
    flow = Dataflow("join_window_columnar")
    keyed = []
    for side, batches in enumerate(_stream()):
        s = op.input(
            f"in{side}",
            flow,
            TestingSource([_rb(k, x, v, device) for k, x, v, _l in batches]),
        )
        keyed.append(op.key_on(f"k{side}", s, lambda _b: "shard-0"))
    wo = win.join_window(
        "jw", _clock(), _tumbling(), *keyed, insert_mode=mode
    )
    op.output("down", wo.down, TestingSink(down))
    op.output("late", wo.late, TestingSink(late))
    op.output("meta", wo.meta, TestingSink(meta))
    run_main(flow)
    rows, late_rows = [], Counter()
    for key, (wid, cols) in down:
        assert key == "shard-0" and wid == COLUMNAR_WINDOW_ID
        _down_rows(cols, device, rows)
    for key, (wid, side_rb) in late:
        assert key == "shard-0" and wid == COLUMNAR_WINDOW_ID
        _late_rows(side_rb, device, late_rows)
    assert meta == []
    cells = [r[:2] for r in rows]
    assert len(set(cells)) == len(cells), "a cell came out twice"
    want_rows, want_late = _expected(mode)
    assert len(want_rows) > 40 and sum(want_late.values()) > 30
    assert {s for s, *_r in want_late} == {0, 1}
    assert sorted(rows) == want_rows
    assert late_rows == want_late


@pytest.mark.parametrize("mode", MODES)
def test_end_to_end_cpu_twin(mode):
    _end_to_end(mode, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_end_to_end_gpu(mode):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _end_to_end(mode, "cuda:0")


# -- dispatch ---------------------------------------------------------------


@pytest.mark.parametrize("mode", MODES)
def test_resolve_gives_a_join_spec(mode):
    device_mode = _join_device_mode(2, _clock(), mode, "final", True)
    assert device_mode == f"join_{mode}"
    spec = _ColumnarSpec.resolve(device_mode, _clock(), _tumbling())
    assert spec == _ColumnarJoinSpec(mode, ALIGN_MS, LEN_MS, WAIT_MS)
    assert isinstance(spec.build(None), _ColumnarJoinLogic)


def _resolve(
    sides=2, clock=None, windower=None, insert="last", emit="final",
    ordered=True,
):
    clock = _clock() if clock is None else clock
    windower = _tumbling() if windower is None else windower
    return _ColumnarSpec.resolve(
        _join_device_mode(sides, clock, insert, emit, ordered), clock, windower
    )


@pytest.mark.parametrize(
    "excluded",
    [
        {"sides": 1},
        {"sides": 3},
        {"clock": SystemClock()},
        {"windower": SlidingWindower(
            align_to=ALIGN, length=LEN_MS * MS, offset=LEN_MS // 2 * MS)},
        {"windower": SessionWindower(gap=LEN_MS * MS)},
        {"insert": "product"},
        {"emit": "complete"},
        {"emit": "running"},
        {"ordered": False},
    ],
    ids=lambda kw: "-".join(
        f"{k}={type(v).__name__ if k in ('clock', 'windower') else v}"
        for k, v in kw.items()
    ),
)
def test_resolve_excludes(excluded):
    assert _resolve() is not None
    assert _resolve(**excluded) is None


def test_python_objects_take_the_host_path():
    """The docstring example of `join_window`: a lowerable
    configuration over Python objects runs on the host as before."""
    names = [(ALIGN + timedelta(seconds=1), ("1", "alice"))]
    mails = [(ALIGN + timedelta(seconds=2), ("1", "a@x.io"))]
    flow = Dataflow("join_window_eg")
    n = op.input("n", flow, TestingSource(names))
    m = op.input("m", flow, TestingSource(mails))
    clock = EventClock(
        ts_getter=lambda ts_kv: ts_kv[0],
        wait_for_system_duration=timedelta(0),
    )
    n_keyed = op.map("nk", n, lambda ts_kv: (ts_kv[1][0], ts_kv))
    m_keyed = op.map("mk", m, lambda ts_kv: (ts_kv[1][0], ts_kv))
    wo = win.join_window(
        "join",
        clock,
        TumblingWindower(align_to=ALIGN, length=timedelta(minutes=1)),
        n_keyed,
        m_keyed,
    )
    out, meta = [], []
    op.output("out", wo.down, TestingSink(out))
    op.output("meta", wo.meta, TestingSink(meta))
    run_main(flow)
    got = [(k, (wid, tuple(v[1][1] for v in vals))) for k, (wid, vals) in out]
    assert got == [("1", (0, ("alice", "a@x.io")))]
    # The host path, window metadata included.
    assert [(k, wid) for k, (wid, _m) in meta] == [("1", 0)]


# -- recovery through the logic ---------------------------------------------


def _values(device):
    """The stream as `(side, RecordBatch)` values, the sides in turn,
    with an entirely late batch of each side after step 6: it moves no
    watermark, so no close runs and its rows sit undrained."""
    sides = _stream()
    values = []
    for i in range(STEPS):
        for side in (0, 1):
            k, x, v, _l = sides[side][i]
            values.append((side, _rb(k, x, v, device)))
        if i == 6:
            for side in (0, 1):
                n = 7 + side
                values.append(
                    (
                        side,
                        _rb(
                            np.arange(n) % KEYS,
                            np.arange(n) * 1000 + side,
                            10_000 * (side + 1) + np.arange(n),
                            device,
                        ),
                    )
                )
    return values


SNAP_AT = 2 * 7 + 2  # values before the snapshot: the late pair is last
# Late rows per side that no close has drained by then: the left side's
# step 6 advanced the horizon (a close ran after it), the right side's
# did not.
_UNDRAINED = [7, 8 + int(_stream()[1][6][3].sum())]


def _drive(logic, values, events):
    for v in values:
        out, done = logic.on_batch([v])
        assert not done
        events.extend(out)


def _emitted(events, device):
    rows, late = [], Counter()
    for wid, typ, obj in events:
        assert wid == COLUMNAR_WINDOW_ID
        assert typ in ("E", "L")  # no metadata on this lowering
        if typ == "E":
            _down_rows(obj, device, rows)
        else:
            # Rows that went through a snapshot come back as host
            # tensors, so the device of late rows is not pinned here.
            _late_rows(obj, None, late)
    cells = [r[:2] for r in rows]
    assert len(set(cells)) == len(cells), "a cell came out twice"
    return sorted(rows), late


def _recovery(mode, device):
    spec = _ColumnarSpec.resolve(f"join_{mode}", _clock(), _tumbling())
    values = _values(device)
    whole = spec.build(None)
    ref = []
    _drive(whole, values, ref)
    ref.extend(whole.on_eof()[0])
    ref_rows, ref_late = _emitted(ref, device)
    want_rows, want_late = _expected(mode)
    assert ref_rows == want_rows
    extra = sum(ref_late.values()) - sum(want_late.values())
    assert extra == 7 + 8 and not want_late - ref_late

    first = spec.build(None)
    before = []
    _drive(first, values[:SNAP_AT], before)
    n_before = sum(_emitted(before, device)[1].values())
    snap = first.snapshot()["__columnar__"]
    assert snap["track_late"] is True
    # The late pair was undrained: the snapshot carries it, per side
    # (with the late rows of the right side's step 6, after which no
    # close ran either).
    assert [len(s["keys"]) for s in snap["__late__"]] == _UNDRAINED
    assert n_before < sum(ref_late.values()) - 15

    resumed = spec.build(snap)
    after = []
    _drive(resumed, values[SNAP_AT:], after)
    after.extend(resumed.on_eof()[0])
    assert _emitted(before + after, device) == (ref_rows, ref_late)
    # The snapshotted logic may carry on as well: each late row once.
    cont = []
    _drive(first, values[SNAP_AT:], cont)
    cont.extend(first.on_eof()[0])
    assert _emitted(before + cont, device) == (ref_rows, ref_late)


@pytest.mark.parametrize("mode", MODES)
def test_recovery_through_the_logic_cpu_twin(mode):
    _recovery(mode, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_recovery_through_the_logic_gpu(mode):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _recovery(mode, "cuda:0")


def test_resumed_without_batches_still_emits_late():
    spec = _ColumnarSpec.resolve("join_last", _clock(), _tumbling())
    first = spec.build(None)
    _drive(first, _values("cpu")[:SNAP_AT], [])
    snap = first.snapshot()["__columnar__"]
    again = spec.build(snap).snapshot()["__columnar__"]
    assert [len(s["keys"]) for s in again["__late__"]] == _UNDRAINED
    events, done = spec.build(again).on_eof()
    assert done
    assert sorted(side for _w, _t, (side, _rb_) in events) == [0, 1]
    assert sum(_emitted(events, "cpu")[1].values()) == sum(_UNDRAINED)
