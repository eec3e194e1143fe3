"""The windowed product join on the device: `k_wjprod_insert`,
`k_wjprod_plan`, `k_wjprod_gather` and `k_wjprod_expand` behind
`WindowJoinProductState`, and the `window_join_product` operator.

The device is compared with the CPU twin and with a direct oracle that
groups the values per (key, window, side) and takes
`itertools.product` per cell, ``[None]`` standing for an empty side.
Row order is not part of the contract, so every comparison is exact
equality of `collections.Counter`s of ``(key, win, v0 | None, v1 |
None)``, and no cell may come out of two closes.

The plan walks the table in chunks of 2,048 slots (256 threads x 8),
so the stream cases use tables of half a chunk, one chunk and four
chunks.
"""

import itertools
from collections import Counter
from datetime import datetime, timedelta, timezone

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import bytewax_amd.operators as op  # noqa: E402
from bytewax_amd.dataflow import Dataflow  # noqa: E402
from bytewax_amd.gpu import RecordBatch, _ms  # noqa: E402
from bytewax_amd.gpu.operators import window_join_product  # noqa: E402
from bytewax_amd.gpu.state import WindowJoinProductState  # noqa: E402
from bytewax_amd.testing import TestingSink, TestingSource, run_main  # noqa: E402

pytestmark = pytest.mark.gpu

ALIGN = datetime(2024, 1, 1, tzinfo=timezone.utc)
ALIGN_MS = _ms(ALIGN)
LEN_MS = 60_000
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
VALUES = np.array([I64_MIN, -1, 7, I64_MAX])
SLOTS_POWS = (10, 11, 13)  # half a plan chunk, one chunk, four chunks
CPU = torch.device("cpu")


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _oracle(batches):
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


def _batch(keys, x, vals, device, ts_form="abs"):
    keys = np.asarray(keys, dtype=np.int32)
    x = np.asarray(x, dtype=np.int64)
    if ts_form == "abs" or x.size == 0:
        ts, base = torch.from_numpy(ALIGN_MS + x), 0
    else:
        # int32 deltas against a base inside the batch's range.
        mid = int(np.sort(x)[x.size // 2])
        ts, base = torch.from_numpy((x - mid).astype(np.int32)), ALIGN_MS + mid
    return RecordBatch(
        torch.from_numpy(keys).to(device),
        ts.to(device),
        torch.from_numpy(np.asarray(vals, dtype=np.int64)).to(device),
        max_ts=int(ALIGN_MS + x.max()) if x.size else None,
        ts_base=base,
    )


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


def _state(dev, slots_pow=10, out_cap=1 << 14, wait_ms=LEN_MS, log_cap=1 << 10):
    return WindowJoinProductState(
        dev, ALIGN_MS, LEN_MS, slots_pow=slots_pow, out_cap=out_cap,
        wait_ms=wait_ms, log_cap=log_cap,
    )


def _drive(st, batches, start=0, rows=None, seen=None, ts_form="abs"):
    """Insert `batches[start:]` with a `close_due` after each, then
    close at EOF; the Counter of all rows."""
    rows = Counter() if rows is None else rows
    seen = set() if seen is None else seen
    for side, keys, x, vals in batches[start:]:
        st.insert(side, _batch(keys, x, vals, st.device, ts_form))
        _rows(st.close_due(), rows, seen)
    _rows(st.close_eof(), rows, seen)
    return rows


def _stream(seed, steps=15, n_keys=12, per_batch=40):
    """`2 * steps` batches, the sides in turn; step `i` of either side
    lies in window `i`.  Side 1 never sees key 0, side 0 never key 1;
    values come from 4 numbers, so equal values and pairs occur."""
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


_SHARED = {}


def _stream_want():
    """One stream and its two references, computed once."""
    if not _SHARED:
        batches = _stream(21)
        want = _oracle(batches)
        assert _drive(_state(CPU), batches) == want
        _SHARED["stream"] = (batches, want)
    return _SHARED["stream"]


@pytest.mark.parametrize("ts_form", ["abs", "delta"])
@pytest.mark.parametrize("slots_pow", SLOTS_POWS)
def test_stream_matches_twin_and_oracle(slots_pow, ts_form):
    dev = _gpu()
    batches, want = _stream_want()
    got = _drive(_state(dev, slots_pow), batches, ts_form=ts_form)
    assert got == want
    assert max(got.values()) > 1
    assert any(v0 is None for _k, _w, v0, _v1 in got)
    assert any(v1 is None for _k, _w, _v0, v1 in got)


def test_cell_shapes_and_hot_cell():
    """One close over cells of (n0, n1) = (1,0), (0,1), (1,1), (1,7),
    (7,1), (64,65) and one of 300 x 200 = 60,000 rows among 500
    single-row cells: rows of many cells share a wave of the expand
    and the hot cell spans many blocks."""
    dev = _gpu()
    rng = np.random.default_rng(1)
    shapes = [(1, 0), (0, 1), (1, 1), (1, 7), (7, 1), (64, 65), (300, 200)]
    hot = len(shapes) - 1
    keys = [[], []]
    for key, ns in enumerate(shapes):
        for side in (0, 1):
            keys[side] += [key] * ns[side]
    # 500 single-row cells, 250 per side, keys 1000..1499.
    keys[0] += range(1000, 1250)
    keys[1] += range(1250, 1500)
    batches = []
    for side in (0, 1):
        k = rng.permutation(np.array(keys[side]))
        # Values from a small range: duplicates inside the hot lists.
        batches.append(
            (side, k, rng.integers(0, LEN_MS, k.size), rng.integers(0, 90, k.size))
        )
    st = _state(dev, slots_pow=11, out_cap=1 << 17, wait_ms=0)
    for side, k, x, v in batches:
        st.insert(side, _batch(k, x, v, dev))
    assert st.close_due() is None  # window 0 is still open
    st.insert(0, _batch([7], [LEN_MS], [1], dev))
    out = st.close_due()
    total = sum(max(a, 1) * max(b, 1) for a, b in shapes) + 500
    assert len(out["keys"]) == total
    got = _rows(out, Counter(), set())
    assert got == _oracle(batches)
    # The hot cell is exactly the product of its lists, with
    # multiplicity.
    lists = [
        Counter(v[k == hot].tolist()) for _side, k, _x, v in batches
    ]
    assert sum(lists[0].values()) == 300 and sum(lists[1].values()) == 200
    assert max(lists[0].values()) > 1
    hot_rows = {r[2:]: n for r, n in got.items() if r[0] == hot}
    assert sum(hot_rows.values()) == 60_000
    assert hot_rows == {
        (a, b): na * nb
        for a, na in lists[0].items()
        for b, nb in lists[1].items()
    }
    assert st.live_counts == (1, 0)
    assert _rows(st.close_eof(), Counter(), set()) == Counter([(7, 1, 1, None)])


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_batch_sizes(n):
    """Around one wave and past one block of the log append; an empty
    batch changes nothing."""
    dev = _gpu()
    rng = np.random.default_rng(n)
    batches = [
        (
            side,
            rng.integers(0, 40, n),
            rng.choice(np.arange(0, 2 * LEN_MS, 7_000), n),
            rng.choice(VALUES, n),
        )
        for side in (0, 1, 0, 1)
    ]
    st = _state(dev)
    got = _drive(st, batches)
    assert got == _oracle(batches)
    assert got == _drive(_state(CPU), batches)
    assert (len(got) == 0) == (n == 0)
    if n == 0:
        assert st.live_counts == (0, 0)
        assert st.snapshot_to_host()["n"] == 0


def test_reclaim_bounds_table_and_logs():
    """40 windows of 200 events per side over about 100 keys each, a
    wait of one window, 1,024 slots and logs that start at 64 entries:
    4,000 cells pass through the table, and a log never holds more
    than the open windows (one that never compacts would need 8,000
    entries)."""
    dev = _gpu()
    rng = np.random.default_rng(4)
    batches = []
    for w in range(40):
        for side in (0, 1):
            batches.append(
                (
                    side,
                    rng.integers(0, 100, 200),
                    w * LEN_MS + rng.integers(0, LEN_MS, 200),
                    rng.choice(VALUES, 200),
                )
            )
    assert 3500 < len({(k, w) for k, w, *_v in _oracle(batches)}) <= 4000
    st = _state(dev, slots_pow=10, out_cap=1 << 12, log_cap=64)
    rows, seen = Counter(), set()
    need = [0, 0]
    for side, keys, x, vals in batches:
        need[side] = max(need[side], st.live_counts[side] + len(keys))
        st.insert(side, _batch(keys, x, vals, dev))
        _rows(st.close_due(), rows, seen)
    _rows(st.close_eof(), rows, seen)
    assert rows == _oracle(batches)
    for side in (0, 1):
        print(f"side {side}: log cap {st.log_caps[side]}, need {need[side]}")
        assert need[side] <= 3 * 200  # at most three windows in flight
        assert need[side] <= st.log_caps[side] <= 2 * need[side]
    assert st.live_counts == (0, 0)


def test_row_total_is_64_bit():
    """One cell of 50,000 x 50,000 events is 2.5e9 rows, past 2^31:
    the close refuses with the exact total and keeps every event.  No
    row is materialised."""
    dev = _gpu()
    n = 50_000
    st = _state(dev, wait_ms=0, log_cap=1 << 16)
    for side in (0, 1):
        st.insert(side, _batch(np.full(n, 3), np.arange(n) % LEN_MS, np.arange(n), dev))
    with pytest.raises(RuntimeError, match=r"\b2500000000\b"):
        st.close_all()
    snap = st.snapshot_to_host()
    assert snap["n"] == 2 * n
    assert st.live_counts == (n, n)
    for side in (0, 1):
        assert sorted(snap["vals"][snap["sides"] == side].tolist()) == list(range(n))
    assert set(snap["keys"].tolist()) == {3} and set(snap["wins"].tolist()) == {0}


def test_table_overflow_raises():
    """600 distinct cells into 512 slots."""
    dev = _gpu()
    keys, x = np.arange(600), np.full(600, 5)
    cpu = _state(CPU)
    cpu.insert(0, _batch(keys, x, keys, CPU))
    assert len(cpu._table) == 600
    st = _state(dev, slots_pow=9)
    st.insert(0, _batch(keys, x, keys, dev))
    with pytest.raises(RuntimeError, match="overflowed; increase slots_pow"):
        st.close_due()


def test_event_behind_the_horizon_is_dropped():
    """An event of a window that has been emitted appears in no
    output, whether the next close has rows or not."""
    dev = _gpu()
    late_val = 666
    # (side, key, window, value), then the horizon to close below.
    steps = [
        ((0, 1, 3, 1), 2),  # nothing is due
        ((1, 9, 0, late_val), 3),  # behind the horizon; nothing is due
        ((1, 1, 3, 3), None),
        ((0, 1, 3, 2), None),
        ((0, 8, 1, late_val), 4),  # behind the horizon; window 3 closes
        ((0, 3, 4, 6), None),
        ((1, 3, 4, 7), 4),
    ]
    outs = []
    for st in (_state(dev, wait_ms=0), _state(CPU, wait_ms=0)):
        rows, seen = Counter(), set()
        for (side, key, w, val), horizon in steps:
            st.insert(side, _batch([key], [w * LEN_MS + 5], [val], st.device))
            if horizon is not None:
                _rows(st.close_below(horizon), rows, seen)
        assert rows == Counter([(1, 3, 1, 3), (1, 3, 2, 3)])
        snap = st.snapshot_to_host()
        assert sorted(snap["vals"].tolist()) == [6, 7]
        _rows(st.close_all(), rows, seen)
        assert st.close_all() is None
        outs.append(rows)
    assert outs[0] == outs[1]
    assert outs[0] == Counter([(1, 3, 1, 3), (1, 3, 2, 3), (3, 4, 6, 7)])


def test_snapshot_restore():
    """Snapshot on the device mid-stream, restore into a fresh device
    state and into a CPU state: the rest of the run is the same."""
    dev = _gpu()
    batches, want = _stream_want()
    k = 11
    st = _state(dev)
    rows, seen = Counter(), set()
    for side, keys, x, vals in batches[:k]:
        st.insert(side, _batch(keys, x, vals, dev))
        _rows(st.close_due(), rows, seen)
    snap = st.snapshot_to_host()
    assert snap["n"] == sum(st.live_counts) > 0
    assert snap["kind"] == "window_join_product"
    for target in (_state(dev, slots_pow=11, log_cap=16), _state(CPU)):
        target.restore_from_host(snap)
        assert target.live_counts == st.live_counts
        got = _drive(target, batches, start=k, rows=Counter(rows), seen=set(seen))
        assert got == want
    # The CPU twin's snapshot holds the same events.
    cpu = _state(CPU)
    for side, keys, x, vals in batches[:k]:
        cpu.insert(side, _batch(keys, x, vals, CPU))
        cpu.close_due()
    csnap = cpu.snapshot_to_host()
    cols = ("keys", "wins", "sides", "vals")
    assert sorted(zip(*(snap[c].tolist() for c in cols))) == sorted(
        zip(*(csnap[c].tolist() for c in cols))
    )
    for c in cols:
        assert snap[c].dtype == csnap[c].dtype
    with pytest.raises(ValueError, match="cannot restore"):
        WindowJoinProductState(dev, ALIGN_MS, 2 * LEN_MS).restore_from_host(snap)


def _run_operator(batches, device):
    out = []
    flow = Dataflow("wjp")
    dev = torch.device(device)
    left = op.input(
        "l", flow,
        TestingSource([_batch(*b[1:], dev) for b in batches if b[0] == 0]),
    )
    right = op.input(
        "r", flow,
        TestingSource([_batch(*b[1:], dev) for b in batches if b[0] == 1]),
    )
    joined = window_join_product(
        "join", left, right, ALIGN, timedelta(milliseconds=LEN_MS),
        wait=timedelta(milliseconds=LEN_MS), slots_pow=10, out_cap=1 << 12,
        log_cap=64, device=device,
    )
    op.output("out", joined, TestingSink(out))
    run_main(flow)
    return out


def test_operator_on_device():
    _gpu()
    batches, want = _stream_want()
    got = []
    for device in ("cuda:0", "cpu"):
        out = _run_operator(batches, device)
        assert len(out) > 2  # closed along the way, not only at EOF
        rows, seen = Counter(), set()
        for d in out:
            assert d["keys"].device.type == torch.device(device).type
            assert d["keys"].dtype == d["wins"].dtype == d["mask"].dtype == torch.int32
            assert d["v0"].dtype == d["v1"].dtype == torch.int64
            _rows(d, rows, seen)
        got.append(rows)
    assert got[0] == got[1] == want
