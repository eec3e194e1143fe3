"""`count_window` / `fold_window(device_sum)` with a `SessionWindower`
over RecordBatch streams lower onto `SessionAggState(ordered=False)`:
`down`, `meta` and `late` all carry data and agree with the host path
fed the same events as Python items, and with a brute-force oracle.

The host path keeps one watermark per key and moves it item by item;
the columnar path keeps one per shard and moves it batch by batch.
The stream makes the two judge lateness alike: each batch is sorted by
timestamp (an item is never late because of an earlier item of its own
batch) and ends with one event per key at the batch's max timestamp
(every key's watermark is the shard's).
"""

import functools
import random
from collections import defaultdict
from datetime import datetime, timedelta, timezone

import pytest

torch = pytest.importorskip("torch")

import bytewax_amd.operators as op  # noqa: E402
import bytewax_amd.operators.windowing as w  # noqa: E402
from bytewax_amd.dataflow import Dataflow  # noqa: E402
from bytewax_amd.gpu import RecordBatch  # noqa: E402
from bytewax_amd.operators.windowing import (  # noqa: E402
    COLUMNAR_WINDOW_ID,
    LATE_SESSION_ID,
    EventClock,
    SessionWindower,
)
from bytewax_amd.testing import TestingSink, TestingSource, run_main  # noqa: E402

ALIGN = datetime(2024, 1, 1, tzinfo=timezone.utc)
ALIGN_MS = int(ALIGN.timestamp() * 1000)
G, W, KEYS = 120, 600, 20
MS =timedelta(milliseconds=1)


@functools.lru_cache(maxsize=None)
def _batches():
    r = random.Random(11)
    out = []
    for b in range(6):
        events = [
            (
                r.randrange(KEYS),
                ALIGN_MS + max(0, b * 400 + r.randrange(-900, 400)),
                r.randrange(1, 50),
            )
            for _ in range(200)
        ]
        # Every key sees the batch's max timestamp.
        events.extend(
            (k, ALIGN_MS + b * 400 + 400, r.randrange(1, 50))
            for k in range(KEYS)
        )
        out.append(tuple(sorted(events, key=lambda e: e[1])))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _oracle(mode):
    """Brute force from the semantics -> (sessions, late)."""
    wm = 0
    per_key, late = defaultdict(list), []
    for batch in _batches():
        for k, t, v in batch:
            if t < wm - W:
                late.append((k, t, v))
            else:
                per_key[k].append((t, v if mode == "sum" else 1))
        wm = max(wm, max(t for _k, t, _v in batch))
    sessions = []
    for k, evs in per_key.items():
        evs.sort()
        start, last, acc = evs[0][0], evs[0][0], 0
        for t, v in evs:
            if t - last > G:
                sessions.append((k, start, last, acc))
                start, acc = t, 0
            last = t
            acc += v
        sessions.append((k, start, last, acc))
    return sorted(sessions), sorted(late)


def _clock(ts_getter):
    # A frozen system clock: the watermark moves with event time only.
    return EventClock(
        ts_getter=ts_getter,
        wait_for_system_duration=W * MS,
        now_getter=lambda: ALIGN,
    )


def _flow(name, items, mode, ts_getter, key_fn):
    """The ONE flow definition, run over items or RecordBatches."""
    down, meta, late = [], [], []
    flow = Dataflow(name)
    s = op.input("inp", flow, TestingSource(items))
    windower = SessionWindower(gap=G * MS)
    if mode == "count":
        wo = w.count_window("cw", s, _clock(ts_getter), windower, key=key_fn)
    else:
        keyed = op.key_on("k", s, key_fn)
        wo = w.fold_window(
            "fw", keyed, _clock(ts_getter), windower, int,
            w.device_sum(lambda it: it[2]), lambda a, b: a + b,
        )
    op.output("down", wo.down, TestingSink(down))
    op.output("meta", wo.meta, TestingSink(meta))
    op.output("late", wo.late, TestingSink(late))
    run_main(flow)
    return down, meta, late


@functools.lru_cache(maxsize=None)
def _host(mode):
    items = [
        (datetime.fromtimestamp(t / 1000, tz=timezone.utc), k, v)
        for batch in _batches()
        for k, t, v in batch
    ]
    down, meta, late = _flow(
        "host", items, mode, lambda it: it[0], lambda it: str(it[1])
    )

    def ms(t):
        return (t - datetime(1970, 1, 1, tzinfo=timezone.utc)) // MS

    accs = {(key, wid): acc for key, (wid, acc) in down}
    assert len(accs) == len(down) == len(meta)
    sessions = sorted(
        (int(key), ms(m.open_time), ms(m.close_time), accs[(key, wid)])
        for key, (wid, m) in meta
    )
    lates = []
    for key, (wid, it) in late:
        assert wid == LATE_SESSION_ID
        lates.append((int(key), ms(it[0]), it[2]))
    return sessions, sorted(lates)


def _rb_rows(out):
    rows = []
    for _key, (wid, rb) in out:
        assert wid == COLUMNAR_WINDOW_ID
        ts = rb.ts.cpu().to(torch.int64) + rb.ts_base
        rows.extend(
            zip(rb.keys.cpu().tolist(), ts.tolist(), rb.vals.cpu().tolist())
        )
    return rows


def _columnar(mode, device):
    batches = [
        RecordBatch(
            torch.tensor([k for k, _t, _v in b], dtype=torch.int32,
                         device=device),
            torch.tensor([t for _k, t, _v in b], dtype=torch.int64,
                         device=device),
            torch.tensor([v for _k, _t, v in b], dtype=torch.int64,
                         device=device),
        )
        for b in _batches()
    ]
    down, meta, late = _flow(
        "columnar", batches, mode, lambda it: it, lambda b: "shard-0"
    )
    accs = {(k, start): acc for k, start, acc in _rb_rows(down)}
    ends = _rb_rows(meta)
    assert len(accs) == len(ends) > 0
    sessions = sorted(
        (k, start, end, accs[(k, start)]) for k, start, end in ends
    )
    return sessions, sorted(_rb_rows(late))


def _check(mode, device):
    sessions, late = _columnar(mode, device)
    o_sessions, o_late = _oracle(mode)
    assert len(o_late) > 50 and len(o_sessions) > 50
    assert sessions == o_sessions
    assert late == o_late
    h_sessions, h_late = _host(mode)
    assert sessions == h_sessions
    assert late == h_late


@pytest.mark.parametrize("mode", ["count", "sum"])
def test_session_lowering_cpu_twin(mode):
    _check(mode, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["count", "sum"])
def test_session_lowering_gpu(mode):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _check(mode, "cuda:0")


def test_session_resolve():
    from bytewax_amd.operators.windowing import (
        _ColumnarSessionLogic,
        _ColumnarSpec,
    )

    windower = SessionWindower(gap=G * MS)
    clock = _clock(lambda it: it)
    spec = _ColumnarSpec.resolve("sum", clock, windower)
    assert (spec.gap_ms, spec.wait_ms) == (G, W)
    logic = spec.build(None)
    assert isinstance(logic, _ColumnarSessionLogic)
    # min/max/mean over sessions stay on the host path.
    for mode in ("min", "max", "mean"):
        assert _ColumnarSpec.resolve(mode, clock, windower) is None
