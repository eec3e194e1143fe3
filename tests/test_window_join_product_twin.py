"""The windowed product join of the columnar path on the CPU: the dict
twin of `WindowJoinProductState` and the `window_join_product`
operator on ``device="cpu"``.

The twin is pinned to the host `join_window` (EventClock,
TumblingWindower, ``insert_mode="product"``, "final" emit,
``ordered=True``) run on the same events.  Row order is not part of
the contract, so every comparison is exact equality of
`collections.Counter`s of ``(key, win, v0 | None, v1 | None)``, and no
cell may come out of two closes.
"""

import itertools
import subprocess
import sys
from collections import Counter
from datetime import datetime, timedelta, timezone
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import bytewax_amd.operators as op  # noqa: E402
import bytewax_amd.operators.windowing as win  # noqa: E402
from bytewax_amd.dataflow import Dataflow  # noqa: E402
from bytewax_amd.gpu import RecordBatch, _ms  # noqa: E402
from bytewax_amd.gpu.operators import (  # noqa: E402
    window_join,
    window_join_product,
)
from bytewax_amd.gpu.state import (  # noqa: E402
    SlidingWindowJoinState,
    WindowJoinProductState,
    WindowJoinState,
)
from bytewax_amd.testing import TestingSink, TestingSource, run_main  # noqa: E402

ALIGN = datetime(2024, 1, 1, tzinfo=timezone.utc)
ALIGN_MS = _ms(ALIGN)
LEN_MS = 60_000
CPU = torch.device("cpu")
VALUES = np.array([-(1 << 62), -1, 7, 1 << 62])
REPO = Path(__file__).resolve().parent.parent


def _stream(seed, steps=15, n_keys=12, per_batch=40):
    """`2 * steps` batches (side, keys, x, vals), the sides in turn;
    step `i` of either side lies in window `i`, so with ``wait =
    LEN_MS`` every batch is at or after the earlier batches' watermark
    minus the wait.  Side 1 never sees key 0 and side 0 never key 1, so
    one-sided cells exist; values come from 4 numbers, so equal values
    and equal pairs occur."""
    rng = np.random.default_rng(seed)
    batches = []
    for i in range(steps):
        for side in (0, 1):
            keys = rng.integers(0, n_keys, per_batch)
            keys = keys[keys != (1 - side)]
            batches.append(
                (
                    side,
                    keys.astype(np.int32),
                    i * LEN_MS + rng.integers(0, LEN_MS, keys.size),
                    rng.choice(VALUES, keys.size),
                )
            )
    return batches


def _batch(keys, x, vals, device=CPU):
    x = np.asarray(x, dtype=np.int64)
    return RecordBatch(
        torch.from_numpy(np.asarray(keys, dtype=np.int32)).to(device),
        torch.from_numpy(ALIGN_MS + x).to(device),
        torch.from_numpy(np.asarray(vals, dtype=np.int64)).to(device),
        max_ts=int(ALIGN_MS + x.max()) if x.size else None,
    )


def _oracle(batches):
    """Counter of (key, win, v0 | None, v1 | None): the values per
    (key, window, side), then `itertools.product` per cell with
    ``[None]`` for an empty side."""
    cells = {}
    for side, keys, x, vals in batches:
        for k, t, v in zip(
            np.asarray(keys).tolist(),
            np.asarray(x).tolist(),
            np.asarray(vals).tolist(),
        ):
            cells.setdefault((k, t // LEN_MS), ([], []))[side].append(v)
    rows = Counter()
    for (k, w), (a, b) in cells.items():
        for v0, v1 in itertools.product(a or [None], b or [None]):
            rows[(k, w, v0, v1)] += 1
    return rows


def _rows(out, into, seen):
    """Add the rows of one close to the Counter `into`; `seen` holds
    the cells of earlier closes, none of which may come again."""
    if out is None:
        return into
    cols = [out[c].cpu().tolist() for c in ("keys", "wins", "mask", "v0", "v1")]
    cells = set()
    for k, w, m, v0, v1 in zip(*cols):
        assert m in (1, 2, 3)
        assert (m & 1) or v0 == 0
        assert (m & 2) or v1 == 0
        cells.add((k, w))
        into[(k, w, v0 if m & 1 else None, v1 if m & 2 else None)] += 1
    assert not (cells & seen), f"cells {sorted(cells & seen)} emitted twice"
    seen |= cells
    return into


def _state(len_ms=LEN_MS, wait_ms=LEN_MS, **kw):
    return WindowJoinProductState(CPU, ALIGN_MS, len_ms, wait_ms=wait_ms, **kw)


def _drive(st, batches, start=0, rows=None, seen=None):
    """Insert `batches[start:]` with a `close_due` after each, then
    close at EOF; the Counter of all rows."""
    rows = Counter() if rows is None else rows
    seen = set() if seen is None else seen
    for side, keys, x, vals in batches[start:]:
        st.insert(side, _batch(keys, x, vals, st.device))
        _rows(st.close_due(), rows, seen)
    _rows(st.close_eof(), rows, seen)
    return rows


def _host(batches):
    """The host `join_window` over the same events, as a Counter."""

    def items(side):
        return [
            (str(k), (ALIGN + timedelta(milliseconds=t), v))
            for s, keys, x, vals in batches
            if s == side
            for k, t, v in zip(keys.tolist(), x.tolist(), vals.tolist())
        ]

    span = (max(int(b[2].max()) for b in batches) // LEN_MS + 1) * LEN_MS
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
        insert_mode="product", emit_mode="final", ordered=True,
    )
    op.output("down", wo.down, TestingSink(down))
    op.output("late", wo.late, TestingSink(late))
    run_main(flow)
    assert late == []
    return Counter(
        (int(k), w, None if l is None else l[1], None if r is None else r[1])
        for k, (w, (l, r)) in down
    )


def test_twin_matches_host_join_window():
    batches = _stream(7)
    host = _host(batches)
    # One-sided cells, paired cells, and rows that occur more than once.
    assert any(v0 is None for _k, _w, v0, _v1 in host)
    assert any(v1 is None for _k, _w, _v0, v1 in host)
    assert max(host.values()) > 1
    assert len({(k, w) for k, w, *_v in host}) > 100
    got = _drive(_state(), batches)
    assert got == host
    assert got == _oracle(batches)


def test_each_cell_in_one_close():
    """30 batches through 15 windows with a close after each: a cell's
    rows all come out of one close (`_rows` refuses a second), and the
    table only ever holds the open windows."""
    batches = _stream(11)
    st = _state()
    rows, seen = Counter(), set()
    closes = 0
    for side, keys, x, vals in batches:
        st.insert(side, _batch(keys, x, vals))
        out = st.close_due()
        closes += out is not None
        _rows(out, rows, seen)
        assert len({w for _k, w in st._table}) <= 2
    _rows(st.close_eof(), rows, seen)
    assert closes >= 13
    assert rows == _oracle(batches)
    assert st._table == {}
    assert st.live_counts == (0, 0)
    assert st.close_eof() is None


def test_operator_cpu():
    """`window_join_product` on ``device="cpu"`` through `run_main`
    equals the host `join_window`."""
    batches = _stream(17)
    out = []
    flow = Dataflow("wjp")
    left = op.input(
        "l", flow,
        TestingSource([_batch(*b[1:]) for b in batches if b[0] == 0]),
    )
    right = op.input(
        "r", flow,
        TestingSource([_batch(*b[1:]) for b in batches if b[0] == 1]),
    )
    joined = window_join_product(
        "join", left, right, ALIGN, timedelta(milliseconds=LEN_MS),
        wait=timedelta(milliseconds=LEN_MS), device="cpu",
    )
    op.output("out", joined, TestingSink(out))
    run_main(flow)
    rows, seen = Counter(), set()
    for d in out:
        assert set(d) == {"keys", "wins", "v0", "v1", "mask"}
        assert d["keys"].dtype == d["wins"].dtype == d["mask"].dtype == torch.int32
        assert d["v0"].dtype == d["v1"].dtype == torch.int64
        _rows(d, rows, seen)
    assert len(out) > 2  # closed along the way, not only at EOF
    assert rows == _host(batches)


def test_build_time_errors():
    def build(**kw):
        flow = Dataflow("wjp_err")
        left = op.input("l", flow, TestingSource([]))
        right = op.input("r", flow, TestingSource([]))
        kw.setdefault("length", timedelta(minutes=1))
        window_join_product("join", left, right, ALIGN, device="cpu", **kw)

    build()
    with pytest.raises(NotImplementedError, match="collectives ordered"):
        build(exchange=True)
    for length in (timedelta(0), timedelta(minutes=-1)):
        with pytest.raises(ValueError, match="length must be positive"):
            build(length=length)
    with pytest.raises(ValueError, match="length must be positive"):
        WindowJoinProductState(CPU, ALIGN_MS, 0)
    # `window_join` still refuses the mode, and says where to go.
    flow = Dataflow("wj_err")
    left = op.input("l", flow, TestingSource([]))
    right = op.input("r", flow, TestingSource([]))
    with pytest.raises(ValueError, match="not supported.*window_join_product"):
        window_join(
            "join", left, right, ALIGN, timedelta(minutes=1),
            insert_mode="product", device="cpu",
        )


def test_snapshot_restore():
    """Snapshot after batch 11 of 30 into a fresh state, then the
    remaining batches: the uninterrupted run's rows."""
    batches = _stream(13)
    assert len(batches) == 30
    want = _drive(_state(), batches)
    k = 11
    st = _state()
    rows, seen = Counter(), set()
    for side, keys, x, vals in batches[:k]:
        st.insert(side, _batch(keys, x, vals))
        _rows(st.close_due(), rows, seen)
    snap = st.snapshot_to_host()
    assert snap["n"] == sum(st.live_counts) > 0
    assert set(snap["sides"].tolist()) == {0, 1}
    st2 = _state()
    st2.restore_from_host(snap)
    assert st2.live_counts == st.live_counts
    assert _drive(st2, batches, start=k, rows=rows, seen=seen) == want

    with pytest.raises(ValueError, match="cannot restore"):
        _state(len_ms=LEN_MS // 2).restore_from_host(snap)
    with pytest.raises(ValueError, match="cannot restore"):
        WindowJoinProductState(CPU, ALIGN_MS + 1, LEN_MS).restore_from_host(snap)


def test_operator_logic_world_tag():
    """The logic class tags its snapshot with the world size and
    refuses one of another, as the window join's does."""
    from bytewax_amd.gpu.operators import _DeviceWindowJoinProductLogic

    side, keys, x, vals = _stream(3)[0]
    logic = _DeviceWindowJoinProductLogic(_state(), LEN_MS)
    logic.on_batch([(side, _batch(keys, x, vals))])
    snap = logic.snapshot()
    assert snap["__world__"] == 1 and snap["n"] == keys.size
    again = _DeviceWindowJoinProductLogic(_state(), LEN_MS, snap)
    assert again.state.live_counts == (keys.size, 0)
    with pytest.raises(ValueError, match="does not rescale"):
        _DeviceWindowJoinProductLogic(
            _state(), LEN_MS, {**snap, "__world__": 2}
        )


def test_cross_kind_snapshots_refused():
    side, keys, x, vals = _stream(5)[0]
    prod = _state()
    prod.insert(side, _batch(keys, x, vals))
    psnap = prod.snapshot_to_host()
    tumbling = WindowJoinState(CPU, ALIGN_MS, LEN_MS, "last", wait_ms=LEN_MS)
    tumbling.insert(side, _batch(keys, x, vals))
    sliding = SlidingWindowJoinState(
        CPU, ALIGN_MS, LEN_MS, LEN_MS // 2, "last", wait_ms=LEN_MS
    )
    sliding.insert(side, _batch(keys, x, vals))
    for other in (tumbling, sliding):
        with pytest.raises(ValueError, match="cannot restore"):
            other.restore_from_host(psnap)
        with pytest.raises(ValueError, match="cannot restore"):
            _state().restore_from_host(other.snapshot_to_host())


@pytest.mark.parametrize("skew", [(), ("--hot-keys", "2", "--hot-frac", "0.05")])
def test_example_runs_on_cpu(skew):
    res = subprocess.run(
        [
            sys.executable,
            str(REPO / "examples" / "window_join_product_gpu.py"),
            "--device", "cpu", "--rows", "8000", "--rows-per-batch", "1000",
            "--keys", "1000", *skew,
        ],
        capture_output=True,
        text=True,
        timeout=120,
    )
    assert res.returncode == 0, res.stderr
    assert "events/s" in res.stdout and "pairs/s" in res.stdout


def test_out_cap_raises_before_anything_is_reclaimed():
    """40 x 30 = 1,200 rows of one cell against ``out_cap=1000``: the
    close raises with the exact total and the state keeps every
    event."""
    st = _state(wait_ms=0, out_cap=1000)
    st.insert(0, _batch(np.full(40, 3), np.arange(40), np.arange(40)))
    st.insert(1, _batch(np.full(30, 3), np.arange(30), np.arange(30) + 100))
    st.insert(0, _batch([9], [LEN_MS], [1]))
    before = st.closed_horizon
    # At EOF the one-row cell of window 1 is due too.
    for close, total in (
        (st.close_due, 1200), (st.close_eof, 1201), (st.close_all, 1201)
    ):
        with pytest.raises(RuntimeError, match=rf"\b{total} rows > out_cap"):
            close()
        assert st.closed_horizon == before
        snap = st.snapshot_to_host()
        assert snap["n"] == 71
        assert sorted(snap["vals"].tolist()) == sorted(
            [*range(40), *range(100, 130), 1]
        )
    # A state with room takes the snapshot and emits the product.
    st2 = _state(wait_ms=0)
    st2.restore_from_host(snap)
    rows = _rows(st2.close_due(), Counter(), set())
    assert rows == Counter(
        (3, 0, a, b) for a in range(40) for b in range(100, 130)
    )
    assert _rows(st2.close_all(), Counter(), set()) == Counter([(9, 1, 1, None)])
