"""The windowed join of the columnar path on the CPU: the dict twin of
`WindowJoinState`, the `window_join` operator on ``device="cpu"`` and
the example.

The twin is pinned to the host `join_window` (EventClock,
TumblingWindower, ``ordered=True``, "final" emit) and to a small
oracle that picks, per (key, window, side), the maximum ("last") or
minimum ("first") of ``(ts, global arrival index)``.  Every comparison
is exact equality of the full set of rows, and no cell may come out
twice across the closes of a run.
"""

import subprocess
import sys
from datetime import datetime, timedelta, timezone
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import bytewax_amd.operators as op  # noqa: E402
import bytewax_amd.operators.windowing as win  # noqa: E402
from bytewax_amd.dataflow import Dataflow  # noqa: E402
from bytewax_amd.gpu import RecordBatch, _ms  # noqa: E402
from bytewax_amd.gpu.operators import window_join  # noqa: E402
from bytewax_amd.gpu.state import WindowJoinState  # noqa: E402
from bytewax_amd.testing import TestingSink, TestingSource, run_main  # noqa: E402

ALIGN = datetime(2024, 1, 1, tzinfo=timezone.utc)
ALIGN_MS = _ms(ALIGN)
LEN_MS = 60_000
CPU = torch.device("cpu")
MODES = ("first", "last")
REPO = Path(__file__).resolve().parent.parent


def _oracle(batches, mode):
    """{(key, window): (mask, v0, v1)} of `batches`, a list of
    (side, keys, x, vals) in arrival order with `x` the offsets from
    the alignment.  A side's winner is the max ("last") or min
    ("first") of (ts, global arrival index); a missing side reads 0."""
    best = {}
    arrival = 0
    for side, keys, x, vals in batches:
        for k, t, v in zip(
            np.asarray(keys).tolist(),
            np.asarray(x).tolist(),
            np.asarray(vals).tolist(),
        ):
            cell = (k, t // LEN_MS, side)
            cand = ((t, arrival), v)
            cur = best.get(cell)
            if (
                cur is None
                or (mode == "last" and cand[0] > cur[0])
                or (mode == "first" and cand[0] < cur[0])
            ):
                best[cell] = cand
            arrival += 1
    rows = {}
    for (k, w, side), (_rank, v) in best.items():
        m, v0, v1 = rows.get((k, w), (0, 0, 0))
        rows[(k, w)] = (m | (1 << side), v if side == 0 else v0,
                        v if side == 1 else v1)
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
    """Add the rows of one close to `into`; no cell twice."""
    if out is None:
        return into
    cols = (out[c].cpu().tolist() for c in ("keys", "wins", "mask", "v0", "v1"))
    for k, w, m, v0, v1 in zip(*cols):
        assert (k, w) not in into, f"cell {(k, w)} emitted twice"
        assert m in (1, 2, 3)
        into[(k, w)] = (m, v0, v1)
    return into


def _stream(seed, steps=15, n_keys=12, per_batch=40):
    """`2 * steps` batches, the sides in turn; step `i` of either side
    lies in window `i`, so with ``wait = LEN_MS`` every batch is at or
    after the earlier batches' watermark minus the wait.  Timestamps
    come from a few values per window: ties within and across batches
    (both sides of a step, and the halves of a side's step) abound."""
    rng = np.random.default_rng(seed)
    batches = []
    for i in range(steps):
        marks = i * LEN_MS + rng.choice(LEN_MS, 6, replace=False)
        for side in (0, 1):
            # Side 1 never sees key 0, side 0 never key 1.
            keys = rng.integers(0, n_keys, per_batch)
            keys = keys[keys != (1 - side)]
            batches.append(
                (
                    side,
                    keys.astype(np.int32),
                    rng.choice(marks, keys.size),
                    rng.integers(-(1 << 62), 1 << 62, keys.size),
                )
            )
    return batches


def _drive(st, batches, start=0, rows=None, device=CPU):
    """Insert `batches[start:]` with a `close_due` after each, then
    close at EOF; the union of the rows."""
    rows = {} if rows is None else rows
    for side, keys, x, vals in batches[start:]:
        st.insert(side, _batch(keys, x, vals, device))
        _rows(st.close_due(), rows)
    _rows(st.close_eof(), rows)
    return rows


def _state(mode, len_ms=LEN_MS, wait_ms=LEN_MS):
    return WindowJoinState(CPU, ALIGN_MS, len_ms, mode, wait_ms=wait_ms)


@pytest.mark.parametrize("mode", MODES)
def test_twin_matches_host_join_window(mode):
    """The semantics are the host's: a few hundred events over 20 keys
    and 5 windows on two sides, timestamps unique per (key, side), keys
    18 and 19 on one side only."""
    rng = np.random.default_rng(7)
    span = 5 * LEN_MS
    sides = []
    for side in (0, 1):
        n = 200
        keys = rng.integers(0, 18, n)
        keys[:10] = 18 + side  # one-sided keys
        # Unique per side, hence per (key, side).
        x = rng.choice(span, n, replace=False)
        vals = rng.integers(-(1 << 62), 1 << 62, n)
        sides.append((keys, x, vals))

    def items(side):
        keys, x, vals = sides[side]
        return [
            (str(k), (ALIGN + timedelta(milliseconds=t), v))
            for k, t, v in zip(keys.tolist(), x.tolist(), vals.tolist())
        ]

    down, late = [], []
    flow = Dataflow("host_join")
    a = op.input("a", flow, TestingSource(items(0)))
    b = op.input("b", flow, TestingSource(items(1)))
    clock = win.EventClock(
        ts_getter=lambda x: x[0],
        wait_for_system_duration=timedelta(milliseconds=2 * span),
    )
    windower = win.TumblingWindower(
        align_to=ALIGN, length=timedelta(milliseconds=LEN_MS)
    )
    wo = win.join_window(
        "jw", clock, windower, a, b,
        insert_mode=mode, emit_mode="final", ordered=True,
    )
    op.output("down", wo.down, TestingSink(down))
    op.output("late", wo.late, TestingSink(late))
    run_main(flow)
    assert late == []
    host = {}
    for k, (w, (l, r)) in down:
        assert (int(k), w) not in host
        host[(int(k), w)] = (
            (l is not None) | ((r is not None) << 1),
            0 if l is None else l[1],
            0 if r is None else r[1],
        )
    assert {m for m, *_v in host.values()} == {1, 2, 3}

    # The twin sees the same events in four batches per side.
    st = _state(mode, wait_ms=2 * span)
    batches = []
    for part in range(4):
        for side in (0, 1):
            keys, x, vals = (c[part * 50:(part + 1) * 50] for c in sides[side])
            batches.append((side, keys, x, vals))
    got = _drive(st, batches)
    assert got == host
    assert got == _oracle(batches, mode)


@pytest.mark.parametrize("mode", MODES)
def test_tie_rule(mode):
    """Equal timestamps within a batch and across batches: the oracle's
    (ts, arrival) order decides."""
    t = 5_000
    batches = [
        # Within one batch: rows 0..3 of key 1 tie at `t`.
        (0, [1, 1, 1, 1, 2], [t, t, t, t, t + 1], [10, 11, 12, 13, 20]),
        # Across batches: the same timestamp again, and a tie at t + 1.
        (0, [1, 2, 2], [t, t + 1, t + 1], [14, 21, 22]),
        (1, [1, 1], [t, t], [30, 31]),
        # A later batch that neither raises nor lowers the stamp.
        (0, [1, 1], [t - 1, t + 1], [15, 16]),
        (1, [1], [t], [32]),
    ]
    st = _state(mode)
    got = _drive(st, batches)
    assert got == _oracle(batches, mode)
    if mode == "last":
        assert got == {(1, 0): (3, 16, 32), (2, 0): (1, 22, 0)}
    else:
        assert got == {(1, 0): (3, 15, 30), (2, 0): (1, 20, 0)}


@pytest.mark.parametrize("mode", MODES)
def test_streaming_closes(mode):
    """30 batches through 15 windows with a close after each: every
    cell once, and the table only ever holds the open windows."""
    batches = _stream(11)
    st = _state(mode)
    rows = {}
    closes = 0
    for side, keys, x, vals in batches:
        st.insert(side, _batch(keys, x, vals))
        out = st.close_due()
        closes += out is not None
        _rows(out, rows)
        assert len({w for _k, w in st._table}) <= 2
    _rows(st.close_eof(), rows)
    assert closes >= 13
    assert rows == _oracle(batches, mode)
    assert {m for m, *_v in rows.values()} == {1, 2, 3}


@pytest.mark.parametrize("mode", MODES)
def test_snapshot_restore(mode):
    batches = _stream(13)
    want = _drive(_state(mode), batches)
    k = 13
    st = _state(mode)
    rows = {}
    for side, keys, x, vals in batches[:k]:
        st.insert(side, _batch(keys, x, vals))
        _rows(st.close_due(), rows)
    snap = st.snapshot_to_host()
    assert snap["n"] > 0
    st2 = _state(mode)
    st2.restore_from_host(snap)
    assert _drive(st2, batches, start=k, rows=rows) == want

    with pytest.raises(ValueError, match="cannot restore"):
        _state(mode, len_ms=LEN_MS // 2).restore_from_host(snap)
    other = "first" if mode == "last" else "last"
    with pytest.raises(ValueError, match="cannot restore"):
        _state(other).restore_from_host(snap)


@pytest.mark.parametrize("mode", MODES)
def test_operator_cpu(mode):
    """`window_join` on ``device="cpu"`` through `run_main` equals the
    state driven directly."""
    batches = _stream(17)
    out = []
    flow = Dataflow("wj")
    left = op.input(
        "l", flow,
        TestingSource([_batch(*b[1:]) for b in batches if b[0] == 0]),
    )
    right = op.input(
        "r", flow,
        TestingSource([_batch(*b[1:]) for b in batches if b[0] == 1]),
    )
    joined = window_join(
        "join", left, right, ALIGN, timedelta(milliseconds=LEN_MS),
        wait=timedelta(milliseconds=LEN_MS), insert_mode=mode,
        device="cpu",
    )
    op.output("out", joined, TestingSink(out))
    run_main(flow)
    rows = {}
    for d in out:
        _rows(d, rows)
    assert len(out) > 2  # closed along the way, not only at EOF
    assert rows == _drive(_state(mode), batches)


def test_build_time_errors():
    def build(**kw):
        flow = Dataflow("wj_err")
        left = op.input("l", flow, TestingSource([]))
        right = op.input("r", flow, TestingSource([]))
        window_join(
            "join", left, right, ALIGN, timedelta(minutes=1),
            device="cpu", **kw,
        )

    build()
    for kw in (
        {"emit_mode": "complete"},
        {"emit_mode": "running"},
        {"insert_mode": "product"},
    ):
        with pytest.raises(ValueError, match="not supported"):
            build(**kw)
    with pytest.raises(NotImplementedError, match="collectives ordered"):
        build(exchange=True)


def test_example_runs_on_cpu():
    res = subprocess.run(
        [
            sys.executable,
            str(REPO / "examples" / "window_join_gpu.py"),
            "--device", "cpu", "--rows", "20000",
        ],
        capture_output=True,
        text=True,
        timeout=120,
    )
    assert res.returncode == 0, res.stderr
    assert "events/s" in res.stdout
