"""Late tracking of the windowed join on the device: the `LATE`
instantiation of `k_wjoin_stamp` behind
`WindowJoinState(track_late=True)`, and the lowered `win.join_window`.

The device is compared with the CPU twin and with a brute force of the
batch-granular rule (an event is late iff its timestamp lies below the
maximum of all earlier batches, hints included, minus the wait)
followed by the oracle of `tests/test_gpu_window_join.py` over the
accepted events.  Every comparison is exact equality of the full set
of rows, no cell may come out twice, and late rows are compared as
multisets: their order in the buffer is not defined.
"""

import importlib.util
from collections import Counter
from datetime import datetime, timezone
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from bytewax_amd.gpu import RecordBatch, _ms  # noqa: E402
from bytewax_amd.gpu.state import WindowJoinState  # noqa: E402

pytestmark = pytest.mark.gpu

ALIGN = datetime(2024, 1, 1, tzinfo=timezone.utc)
ALIGN_MS = _ms(ALIGN)
LEN_MS = 60_000
MODES = ("first", "last")
COLS = ("keys", "wins", "mask", "v0", "v1", "t0", "t1")


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _split(batches, wait_ms):
    """Brute force of the rule over (side, keys, x, vals[, hint])
    batches, `x` the offsets from the alignment: (accepted batches,
    Counter of late (side, key, abs ts, val))."""
    wm, acc, late = 0, [], Counter()
    for side, keys, x, vals, *hint in batches:
        keys, x, vals = (np.asarray(a) for a in (keys, x, vals))
        is_late = ALIGN_MS + x < wm - wait_ms
        late.update(
            (side, k, ALIGN_MS + t, v)
            for k, t, v in zip(
                keys[is_late].tolist(), x[is_late].tolist(),
                vals[is_late].tolist(),
            )
        )
        acc.append((side, keys[~is_late], x[~is_late], vals[~is_late]))
        top = hint[0] if hint else (x.max() if x.size else None)
        if top is not None:
            wm = max(wm, ALIGN_MS + int(top))
    return acc, late


def _oracle(batches, mode):
    """{(key, window): (mask, v0, v1)}: per side the max ("last") or
    min ("first") of (ts, global arrival index); a missing side reads
    0."""
    best = {}
    arrival = 0
    for side, keys, x, vals in batches:
        for k, t, v in zip(keys.tolist(), x.tolist(), vals.tolist()):
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


def _batch(keys, x, vals, device, ts_form="abs", hint=None):
    """`hint` (an offset like `x`) overrides the batch maximum as the
    `max_ts` hint."""
    keys = np.asarray(keys, dtype=np.int32)
    x = np.asarray(x, dtype=np.int64)
    if ts_form == "abs" or x.size == 0:
        ts, base = torch.from_numpy(ALIGN_MS + x), 0
    else:
        # int32 deltas against a base inside the batch's range.
        mid = int(np.sort(x)[x.size // 2])
        ts, base = torch.from_numpy((x - mid).astype(np.int32)), ALIGN_MS + mid
    if hint is None and x.size:
        hint = x.max()
    return RecordBatch(
        torch.from_numpy(keys).to(device),
        ts.to(device),
        torch.from_numpy(np.asarray(vals, dtype=np.int64)).to(device),
        max_ts=None if hint is None else int(ALIGN_MS + hint),
        ts_base=base,
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


def _late(st, into):
    for side in (0, 1):
        rb = st.take_late(side)
        if rb is None:
            continue
        assert rb.ts.dtype == torch.int64 and rb.ts_base == 0
        assert rb.keys.device == st.device
        into.update(
            (side, k, t, v)
            for k, t, v in zip(
                rb.keys.cpu().tolist(), rb.ts.cpu().tolist(),
                rb.vals.cpu().tolist(),
            )
        )
    return into


def _state(dev, mode, slots_pow=10, out_cap=1 << 14, wait_ms=0, late_cap=0):
    return WindowJoinState(
        dev, ALIGN_MS, LEN_MS, mode, slots_pow=slots_pow, out_cap=out_cap,
        wait_ms=wait_ms, track_late=True, late_cap=late_cap,
    )


def _drive(st, batches, ts_form="abs"):
    """Insert with a `close_due` after each batch, close at EOF:
    (rows, late multiset)."""
    rows, late = {}, Counter()
    for side, keys, x, vals, *hint in batches:
        st.insert(side, _batch(keys, x, vals, st.device, ts_form, *hint))
        _rows(st.close_due(), rows)
    _rows(st.close_eof(), rows)
    return rows, _late(st, late)


def _table(st):
    snap = st.snapshot_to_host()
    if not snap["n"]:
        return []
    return sorted(zip(*(snap[c].tolist() for c in COLS)))


def _check(dev, mode, batches, wait_ms=0, ts_form="abs", **kw):
    """Device rows and late rows == brute force + oracle == CPU twin."""
    got = _drive(_state(dev, mode, wait_ms=wait_ms, **kw), batches, ts_form)
    acc, late = _split(batches, wait_ms)
    assert got[0] == _oracle(acc, mode)
    assert got[1] == late
    cpu = _state(torch.device("cpu"), mode, wait_ms=wait_ms)
    assert got == _drive(cpu, batches)
    return got


# Watermark set by the priming batch: the middle of window 1.
WM = LEN_MS + LEN_MS // 2

PATTERNS = {
    "none": lambda i: np.zeros(i.size, dtype=bool),
    "all": lambda i: np.ones(i.size, dtype=bool),
    "alternating": lambda i: i % 2 == 1,
    "lane0": lambda i: i % 64 == 0,
    "lane63": lambda i: i % 64 == 63,
}


@pytest.mark.parametrize("pattern", sorted(PATTERNS))
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_batch_sizes(n, pattern):
    """Around one wave and just past one block; late lanes by pattern.
    Late rows lie in window 0 and in window 1, which is still open for
    the first of the four batches; the accepted rows of a batch start
    where the batch before ended."""
    dev = _gpu()
    rng = np.random.default_rng(n)
    is_late = PATTERNS[pattern](np.arange(n))
    batches = [(0, [7, 8], [WM - 5, WM], [1, 2])]
    for j, side in enumerate((0, 1, 1, 0)):
        x = np.where(
            is_late,
            rng.choice(np.arange(0, WM, 6_000), n),
            WM + j * LEN_MS + rng.choice(np.arange(0, LEN_MS, 7_000), n),
        )
        batches.append(
            (side, rng.integers(0, 40, n), x, rng.integers(-(1 << 62), 1 << 62, n))
        )
    for mode in MODES:
        for ts_form in ("abs", "delta"):
            rows, late = _check(dev, mode, batches, ts_form=ts_form)
            assert sum(late.values()) == 4 * int(is_late.sum())
            assert len(rows) >= 2


@pytest.mark.parametrize("half", [False, True], ids=["all_late", "first_half"])
@pytest.mark.parametrize("mode", MODES)
def test_stale_scratch(mode, half):
    """`ev_slot` keeps the slots of the batch before.  A late row whose
    key and timestamp equal a cell of the table must leave that cell
    alone: under "last" a stale slot would win the election (equal
    stamp, later arrival) and commit the late value."""
    dev = _gpu()
    n = 512
    keys = np.arange(n)
    x = LEN_MS + (np.arange(n) * 97) % LEN_MS
    hint = 2 * LEN_MS - 1  # above every stamp: the same rows are late next
    first = (0, keys, x, np.arange(n) + 1, hint)
    if half:
        # Rows 256.. are new cells of window 2, accepted.
        k2 = np.r_[keys[:256], keys[256:] + 1000]
        x2 = np.r_[x[:256], 2 * LEN_MS + x[256:] - LEN_MS]
    else:
        k2, x2 = keys, x
    second = (0, k2, x2, np.arange(n) + 1_000_000)
    n_late = 256 if half else n

    def run(device):
        st = _state(device, mode, slots_pow=11)
        st.insert(0, _batch(*first[1:4], device, hint=hint))
        before = _table(st)
        assert len(before) == n
        st.insert(0, _batch(*second[1:], device))
        late = _late(st, Counter())
        return st, before, _table(st), late

    st, before, after, late = run(dev)
    _acc, want_late = _split([first, second], 0)
    assert sum(want_late.values()) == n_late
    assert late == want_late
    if half:
        assert after[:n] == before and len(after) == n + 256
    else:
        assert after == before
    _st, c_before, c_after, c_late = run(torch.device("cpu"))
    assert (before, after, late) == (c_before, c_after, c_late)
    # The right side of the same cells: late as well, and absent.
    st.insert(1, _batch(keys, x, np.arange(n) - 5, dev))
    assert _table(st) == after
    assert sum(_late(st, Counter()).values()) == n


@pytest.mark.parametrize("mode", MODES)
def test_one_hot_late_cell(mode):
    """4,096 late events with one key and one timestamp, in an open
    window: all come out, none is in the table."""
    dev = _gpu()
    n = 4096
    st = _state(dev, mode)
    st.insert(0, _batch([5], [WM], [1], dev))
    st.insert(0, _batch(np.full(n, 5), np.full(n, WM - 1), np.arange(n) + 10, dev))
    st.insert(1, _batch(np.full(n, 5), np.full(n, WM - 1), np.arange(n) - n, dev))
    late = _late(st, Counter())
    want = Counter(
        (side, 5, ALIGN_MS + WM - 1, v)
        for side, vals in ((0, np.arange(n) + 10), (1, np.arange(n) - n))
        for v in vals.tolist()
    )
    assert late == want and sum(late.values()) == 2 * n
    assert _table(st) == [(5, 1, 1, 1, 0, ALIGN_MS + WM, 0)]
    assert _rows(st.close_eof(), {}) == {(5, 1): (1, 1, 0)}


def test_late_buffer_bound():
    """`late_cap=64` and five all-late batches of 64: the state drains
    the buffer into the host carry before each insert that could pass
    it, so every row comes out and nothing overflows."""
    dev = _gpu()
    st = _state(dev, "last", late_cap=64)
    st.insert(0, _batch([1], [WM], [0], dev))
    assert not st.late_drained()
    want = Counter()
    for b in range(5):
        keys = np.arange(64) + 100 * b
        x = np.arange(64) * 11 + b
        vals = np.arange(64) + 1000 * b
        st.insert(1, _batch(keys, x, vals, dev))
        want.update(
            (1, k, ALIGN_MS + t, v)
            for k, t, v in zip(keys.tolist(), x.tolist(), vals.tolist())
        )
    assert st.late_drained()
    assert st._late[1].cap == 64
    late = _late(st, Counter())
    assert late == want and sum(late.values()) == 320
    assert not st.late_drained()
    # The error flag is read here: no overflow of either kind.
    assert _rows(st.close_eof(), {}) == {(1, 1): (1, 0, 0)}


@pytest.mark.parametrize("mode", MODES)
def test_reclaim_with_late_traffic(mode):
    """The reclaim shape of `test_gpu_window_join.py` at 1,024 slots
    (400 keys per window over 20 windows, 0..299 left and 100..399
    right), with 50 events from three windows back appended to every
    batch and ``wait_ms=0``.

    With no wait a batch must not lie below the batch before it, so
    the left side takes the first half of each window and the right
    side the second; and the stream starts at window 3, so that window
    `w - 3` exists.  The appended events are late in every batch but
    the stream's first, before which there is no watermark: there they
    are accepted into window 0 and come out as cells of their own."""
    dev = _gpu()
    rng = np.random.default_rng(10)
    half = LEN_MS // 2
    batches = []
    for w in range(3, 23):
        for side, lo in ((0, 0), (1, 100)):
            keys = np.r_[
                np.arange(lo, lo + 300),
                rng.integers(lo, lo + 300, 50),
                rng.integers(0, 400, 50),
            ]
            x = np.r_[
                w * LEN_MS + side * half + rng.integers(0, half, 350),
                (w - 3) * LEN_MS + rng.integers(0, LEN_MS, 50),
            ]
            order = rng.permutation(keys.size)
            batches.append(
                (
                    side,
                    keys[order],
                    x[order],
                    rng.integers(-(1 << 62), 1 << 62, keys.size),
                )
            )
    acc, want_late = _split(batches, 0)
    assert sum(want_late.values()) == 50 * 39
    st = _state(dev, mode, slots_pow=10)
    rows, late = {}, Counter()
    for side, keys, x, vals in batches:
        st.insert(side, _batch(keys, x, vals, dev))
        _rows(st.close_due(), rows)  # raises if the table overflowed
    _rows(st.close_eof(), rows)
    _late(st, late)
    assert late == want_late
    assert rows == _oracle(acc, mode)
    live = {kw for kw in rows if kw[1] >= 3}
    assert live == {(k, w) for w in range(3, 23) for k in range(400)}
    assert len(live) == 8000 and len(rows) - len(live) <= 50


@pytest.mark.parametrize("mode", MODES)
def test_determinism(mode):
    """The same disordered input twice: identical rows, bit for bit,
    and identical late multisets."""
    dev = _gpu()
    rng = np.random.default_rng(5)
    n = 4096
    marks = rng.choice(6 * LEN_MS, 16, replace=False)
    batches = [
        (
            side,
            rng.integers(0, 50, n),
            rng.choice(marks, n),
            rng.integers(-(1 << 63), (1 << 63) - 1, n),
        )
        for side in (0, 1, 0, 1, 1, 0)
    ]
    runs = []
    for _ in range(2):
        rows, late = _drive(_state(dev, mode, wait_ms=LEN_MS), batches)
        runs.append((sorted(rows.items()), late))
    assert runs[0] == runs[1]
    acc, want_late = _split(batches, LEN_MS)
    assert 0 < sum(want_late.values()) < 6 * n
    assert runs[0][1] == want_late
    assert dict(runs[0][0]) == _oracle(acc, mode)


@pytest.mark.parametrize("mode", MODES)
def test_operator_on_device(mode):
    """The end-to-end case of the lowering tests with `cuda:0`
    tensors: `win.join_window` over two RecordBatch sources; rows and
    late rows stay on the device."""
    _gpu()
    path = (
        Path(__file__).parent / "windowing"
        / "test_columnar_join_window_lowering.py"
    )
    spec = importlib.util.spec_from_file_location("_join_lowering_case", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod._end_to_end(mode, "cuda:0")
