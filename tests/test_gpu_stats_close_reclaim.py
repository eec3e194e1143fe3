"""The reclaiming stats close on the device: `k_stats_close_migrate`
behind `StatsAggState.close_due` / `close_below`, and the two public
paths that close through it.

A close at `horizon` emits the cells of windows in
``[closed_horizon, horizon)``, rebuilds the cells at or above `horizon`
in a fresh table and forgets everything below `horizon`.  Every oracle
is an exact int64 numpy group-by.

The kernel walks the table in chunks of 2,048 slots (256 threads x 8),
so the shape cases use tables of half a chunk, one chunk and four
chunks.
"""

from datetime import datetime, timedelta, timezone

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from bytewax_amd.gpu import RecordBatch, _ms  # noqa: E402
from bytewax_amd.gpu.state import StatsAggState  # noqa: E402

pytestmark = pytest.mark.gpu

ALIGN = datetime(2024, 1, 1, tzinfo=timezone.utc)
ALIGN_MS = _ms(ALIGN)
LEN_MS = 60_000
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
COLS = ("keys", "wins", "cnt", "sum", "min", "max")
FILLS = (-1, 0, 0, I64_MAX, I64_MIN)  # an empty slot of the five arrays


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


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
        s = np.add.reduceat(v, first)  # wraps mod 2^64 like the device
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
    for k, w, c, s, mn, mx in zip(*(out[n].cpu().tolist() for n in COLS)):
        assert (k, w) not in got, f"cell {(k, w)} emitted twice"
        got[(k, w)] = (c, s, mn, mx)
    return got


def _cat(batches):
    return tuple(np.concatenate([b[i] for b in batches]) for i in range(3))


def _insert(st, batch, ts_form="abs"):
    keys, x, vals = batch
    x = np.asarray(x, dtype=np.int64)
    if ts_form == "abs":
        ts, base = torch.from_numpy(ALIGN_MS + x), 0
    else:
        # int32 deltas against a base inside the batch's range.
        mid = int(np.sort(x)[x.size // 2])
        ts, base = torch.from_numpy((x - mid).astype(np.int32)), ALIGN_MS + mid
    dev = st.device
    st.insert(
        RecordBatch(
            torch.from_numpy(np.asarray(keys, dtype=np.int32)).to(dev),
            ts.to(dev),
            torch.from_numpy(np.asarray(vals, dtype=np.int64)).to(dev),
            max_ts=int(ALIGN_MS + x.max()),
            ts_base=base,
        )
    )


def _window_batch(win, n_keys, n_extra, seed):
    """Every key of `arange(n_keys)` once plus `n_extra` random
    repeats, all inside window `win`."""
    rng = np.random.default_rng(seed)
    keys = np.r_[np.arange(n_keys), rng.integers(0, n_keys, n_extra)]
    x = win * LEN_MS + rng.integers(0, LEN_MS, keys.size)
    vals = rng.integers(-(1 << 40), 1 << 40, keys.size)
    return keys.astype(np.int32), x, vals


def _cells(n_cells, wins, seed):
    """`n_cells` one- or two-event cells spread evenly over `wins`."""
    rng = np.random.default_rng(seed)
    per = -(-n_cells // len(wins))
    keys = np.concatenate([np.arange(per) for _ in wins])[:n_cells]
    w = np.repeat(np.asarray(wins), per)[:n_cells]
    dup = rng.random(n_cells) < 0.3
    keys = np.r_[keys, keys[dup]]
    w = np.r_[w, w[dup]]
    x = w * LEN_MS + rng.integers(0, LEN_MS, keys.size)
    vals = rng.integers(-(1 << 40), 1 << 40, keys.size)
    return keys.astype(np.int32), x, vals


def _direct(dev, slots_pow, **kw):
    kw.setdefault("out_cap", 1 << 13)
    st = StatsAggState(
        dev, ALIGN_MS, LEN_MS, radix=False, slots_pow=slots_pow, **kw
    )
    assert st.nslots == 1 << slots_pow
    return st


def _occupied(st):
    return int((st.tkeys != -1).sum().item())


def _assert_retired_is_fresh(st):
    assert st.tables_alt is not None
    for t, fill in zip(st.tables_alt, FILLS):
        assert t.numel() == st.nslots
        assert bool((t == fill).all().item())


def _check_survivors(st, want):
    """The live table holds exactly `want`: by extract, and by the raw
    count of occupied slots (a dropped cell shows in no extract)."""
    assert _got(st.extract(clear=False)) == want
    assert _occupied(st) == len(want)
    assert int(st.error_flag.item()) == 0


# -- streams longer than the table --------------------------------------


def _direct_stream():
    return [_window_batch(w, 200, 400, 1000 + w) for w in range(40)]


def test_stream_longer_than_table_direct():
    dev = _gpu()
    batches = _direct_stream()
    ref = _ref_stats(*_cat(batches))
    assert len(ref) == 8_000
    st = _direct(dev, 10, out_cap=1 << 12)
    got = {}
    for b in batches:
        _insert(st, b)
        assert _occupied(st) <= 400
        _got(st.close_due(0), got)
    assert st.closed_horizon == 39
    _got(st.close_all(), got)
    assert int(st.error_flag.item()) == 0
    assert got == ref


def test_stream_longer_than_table_overflows_without_reclaim():
    """The control: the same stream closed by `extract(horizon)` plus a
    `closed_horizon` bump, which never gives a slot back."""
    dev = _gpu()
    st = _direct(dev, 10, out_cap=1 << 12)
    with pytest.raises(RuntimeError, match="overflowed"):
        for b in _direct_stream():
            _insert(st, b)
            horizon = (st.max_ts_host - ALIGN_MS) // LEN_MS
            st.extract(horizon)
            st.closed_horizon = horizon
    assert st.tables_alt is None


@pytest.mark.parametrize("ts_form", ["abs", "delta"])
def test_stream_longer_than_table_radix(ts_form):
    dev = _gpu()
    batches = [_window_batch(w, 3_000, 5_193, 2000 + w) for w in range(30)]
    assert all(b[0].size == 8_193 for b in batches)
    ref = _ref_stats(*_cat(batches))
    assert len(ref) == 90_000
    st = StatsAggState(
        dev, ALIGN_MS, LEN_MS, slots_pow=10, region_bits=4, out_cap=1 << 13
    )
    assert st.radix and st.nslots == 1 << 14
    got = {}
    for b in batches:
        _insert(st, b, ts_form)
        _got(st.close_due(0), got)
    _got(st.close_all(), got)
    assert int(st.error_flag.item()) == 0
    assert got == ref


# -- kernel shapes -------------------------------------------------------

# Half a chunk, one chunk, four chunks.
SHAPES = [(10, 500), (11, 1_000), (13, 4_000)]
N_WIN = 8


def _primed(dev, slots_pow):
    """A state whose second table exists: until a close has had rows
    to emit, a close that finds nothing due launches no migration.
    One cell in window 0, closed; the table is empty again."""
    st = _direct(dev, slots_pow)
    _insert(st, (np.array([-5], dtype=np.int32), np.array([3]), np.array([1])))
    assert _got(st.close_below(1)) == {(-5, 0): (1, 1, 1, 1)}
    assert st.tables_alt is not None and _occupied(st) == 0
    return st


@pytest.mark.parametrize("slots_pow,n_cells", SHAPES)
@pytest.mark.parametrize("take", ["nothing", "everything", "half"])
def test_close_shapes(slots_pow, n_cells, take):
    dev = _gpu()
    lo = 2  # windows 2 .. 9: a close at 2 runs and takes nothing
    batch = _cells(n_cells, range(lo, lo + N_WIN), 3000 + slots_pow)
    ref = _ref_stats(*batch)
    assert len(ref) == n_cells
    st = _primed(dev, slots_pow)
    _insert(st, batch)
    horizon = lo + {"nothing": 0, "everything": N_WIN, "half": N_WIN // 2}[take]
    retired = st.tkeys.data_ptr()
    out = st.close_below(horizon)
    assert st.closed_horizon == horizon
    # The tables were swapped: the kernel ran, also for `nothing`.
    assert st.tables_alt[0].data_ptr() == retired != st.tkeys.data_ptr()
    assert _got(out) == {c: v for c, v in ref.items() if c[1] < horizon}
    assert (out is None) == (take == "nothing")
    _check_survivors(st, {c: v for c, v in ref.items() if c[1] >= horizon})
    _assert_retired_is_fresh(st)


@pytest.mark.parametrize("slots_pow,n_cells", SHAPES)
def test_close_every_second_window_drops_the_rest(slots_pow, n_cells):
    """One pass that meets all three classes, window by window: with
    `closed_horizon` moved to h - 1, a close at h emits window h - 1,
    drops window h - 2 (below the closed horizon, as a cell made by an
    event behind the watermark is) and migrates the rest."""
    dev = _gpu()
    batch = _cells(n_cells, range(N_WIN), 3100 + slots_pow)
    ref = _ref_stats(*batch)
    st = _direct(dev, slots_pow, out_cap=1 << 13)
    _insert(st, batch)
    got = {}
    for h in range(2, N_WIN + 1, 2):
        st.closed_horizon = h - 1
        rows = _got(st.close_below(h))
        assert rows == {c: v for c, v in ref.items() if c[1] == h - 1}
        got.update(rows)
        _check_survivors(st, {c: v for c, v in ref.items() if c[1] >= h})
        _assert_retired_is_fresh(st)
    assert got == {c: v for c, v in ref.items() if c[1] % 2 == 1}
    assert _occupied(st) == 0


def test_probe_chains_survive_the_rebuild():
    """70 % load: 716 cells in 1,024 slots, half due and half live.
    Events inserted into the survivors afterwards must find their
    cells; a broken chain would claim a second slot for one."""
    dev = _gpu()
    first = _cells(716, [0, 1], 3200)
    assert len(_ref_stats(*first)) == 716
    st = _direct(dev, 10)
    _insert(st, first)
    assert _occupied(st) == 716
    ref = _ref_stats(*first)
    assert _got(st.close_below(1)) == {
        c: v for c, v in ref.items() if c[1] == 0
    }
    more = _cells(358, [1], 3201)
    fresh = _cells(300, [2], 3202)
    _insert(st, _cat([more, fresh]))
    want = _ref_stats(*_cat([first, more, fresh]))
    _check_survivors(st, {c: v for c, v in want.items() if c[1] >= 1})


def test_edge_values_through_close_and_migration():
    dev = _gpu()
    keys = [-2, I32_MIN, I32_MAX, 0]
    rows = []
    for w in (0, 1):
        # one-event cells at the extremes
        rows += [(-2, w, I64_MIN), (I32_MIN, w, I64_MAX)]
        # sums that wrap, in both directions
        rows += [(I32_MAX, w, I64_MAX), (I32_MAX, w, I64_MAX), (I32_MAX, w, 2)]
        rows += [(0, w, I64_MIN), (0, w, I64_MIN), (0, w, -1)]
    batch = (
        np.array([r[0] for r in rows], dtype=np.int32),
        np.array([r[1] * LEN_MS + 7 for r in rows]),
        np.array([r[2] for r in rows], dtype=np.int64),
    )
    ref = _ref_stats(*batch)
    assert {c[0] for c in ref} == set(keys) and len(ref) == 8
    assert ref[(I32_MAX, 0)] == (3, 0, 2, I64_MAX)
    assert ref[(0, 1)] == (3, -1, I64_MIN, -1)
    assert ref[(-2, 0)] == (1, I64_MIN, I64_MIN, I64_MIN)
    st = _direct(dev, 10)
    _insert(st, batch)
    assert _got(st.close_below(1)) == {
        c: v for c, v in ref.items() if c[1] == 0
    }
    _check_survivors(st, {c: v for c, v in ref.items() if c[1] == 1})
    assert _got(st.close_all()) == {c: v for c, v in ref.items() if c[1] == 1}


def test_out_cap_is_reported():
    dev = _gpu()
    st = _direct(dev, 10, out_cap=64)
    _insert(st, _cells(100, [0], 3300))
    with pytest.raises(RuntimeError, match="out_cap"):
        st.close_below(1)


# -- state life cycle across closes --------------------------------------


def _lifecycle_batch(w, seed):
    # Reaches one window ahead, so every close leaves live cells.
    return _cat([_window_batch(w, 150, 150, seed), _window_batch(w + 1, 40, 0, seed + 500)])


def test_snapshot_restore_across_closes():
    dev = _gpu()
    st = _direct(dev, 10)
    batches, got = [], {}
    for w in range(2):
        batches.append(_lifecycle_batch(w, 4000 + w))
        _insert(st, batches[-1])
        _got(st.close_due(0), got)
    assert st.closed_horizon == 2
    snap = st.snapshot_to_host()
    assert snap["closed_horizon"] == 2
    assert {int(w) for w in snap["wins"]} == {2}
    st2 = _direct(dev, 10)
    st2.restore_from_host(snap)
    assert st2.tables_alt is None
    for w in range(2, 5):
        batches.append(_lifecycle_batch(w, 4000 + w))
        _insert(st2, batches[-1])
        _got(st2.close_due(0), got)
    _got(st2.close_all(), got)
    assert int(st2.error_flag.item()) == 0
    assert got == _ref_stats(*_cat(batches))


def test_merge_rows_into_a_state_that_has_closed():
    dev = _gpu()
    st = _direct(dev, 10)
    b0 = _cat([_window_batch(0, 100, 50, 4100), _window_batch(1, 100, 50, 4101)])
    _insert(st, b0)
    got = _got(st.close_due(0))
    donor = _direct(dev, 10)
    d = _cat([_window_batch(1, 120, 50, 4102), _window_batch(2, 120, 50, 4103)])
    _insert(donor, d)
    st.merge_rows(donor.snapshot_to_host())
    _got(st.close_below(2), got)
    _got(st.close_all(), got)
    assert int(st.error_flag.item()) == 0
    assert got == _ref_stats(*_cat([b0, d]))


@pytest.mark.parametrize("radix", [False, True])
def test_late_rows_once_with_closes_in_between(radix):
    dev = _gpu()
    st = StatsAggState(
        dev, ALIGN_MS, LEN_MS, slots_pow=10, region_bits=4, radix=radix,
        track_late=True, wait_ms=0,
    )
    batches, late, got, drained = [], [], {}, []
    for w in range(5):
        b = _window_batch(w, 150, 150, 4200 + w)
        batches.append(b)
        if w >= 2:
            # Two windows back: below the watermark the earlier
            # batches set, so late.
            lb = _window_batch(w - 2, 30, 10, 4300 + w)
            late.append(lb)
            b = _cat([b, lb])
        _insert(st, b)
        _got(st.close_due(), got)
        if w == 3:
            drained.append(st.take_late())
    drained.append(st.take_late())
    assert st.take_late() is None
    _got(st.close_all(), got)
    assert int(st.error_flag.item()) == 0
    assert got == _ref_stats(*_cat(batches))
    rows = sorted(
        row
        for d in drained
        if d is not None
        for row in zip(
            d.keys.cpu().tolist(),
            (d.ts.cpu() - ALIGN_MS).tolist(),
            d.vals.cpu().tolist(),
        )
    )
    assert rows == sorted(zip(*(a.tolist() for a in _cat(late))))


def test_alternate_table_is_lazy():
    dev = _gpu()
    st = _direct(dev, 10)
    b = _cat([_window_batch(0, 100, 0, 4400), _window_batch(1, 100, 0, 4401)])
    _insert(st, b)
    st.extract(1)
    st.closed_horizon = 1
    st.extract(clear=False)
    st.snapshot_to_host()
    assert st.tables_alt is None
    st.close_below(2)
    _assert_retired_is_fresh(st)
    # Nor does a close with nothing due: the whole-stream operator asks
    # once for the windows below its only one.
    whole = _direct(dev, 10)
    _insert(whole, _window_batch(5, 100, 50, 4402))
    assert whole.close_due(0) is None
    assert whole.closed_horizon == 5 and whole.tables_alt is None
    assert whole.close_due(0) is None
    _insert(whole, _window_batch(6, 100, 50, 4403))
    assert _got(whole.close_due(0)) == _ref_stats(*_window_batch(5, 100, 50, 4402))
    _assert_retired_is_fresh(whole)


# -- through the public lowering -----------------------------------------


def test_max_window_lowering_runs_past_the_table():
    """4.48M cumulative cells through the lowering's 2^22-slot table,
    at most 140k of them live.  One event per cell, so the oracle is
    the value itself."""
    dev = _gpu()
    import bytewax_amd.operators as op
    import bytewax_amd.operators.windowing as w
    from bytewax_amd.dataflow import Dataflow
    from bytewax_amd.operators.windowing import (
        COLUMNAR_WINDOW_ID,
        EventClock,
        TumblingWindower,
    )
    from bytewax_amd.testing import TestingSink, TestingSource, run_main

    n_keys, n_win = 70_000, 64
    gen = torch.Generator(device="cpu").manual_seed(5)
    vals = torch.randint(
        -(1 << 40), 1 << 40, (n_win, n_keys), generator=gen, dtype=torch.int64
    ).to(dev)
    offs = torch.randint(
        0, LEN_MS, (n_win, n_keys), generator=gen, dtype=torch.int64
    )
    batches = []
    for i in range(n_win):
        perm = torch.randperm(n_keys, generator=gen)
        ts = ALIGN_MS + i * LEN_MS + offs[i]
        batches.append(
            RecordBatch(
                perm.to(torch.int32).to(dev),
                ts.to(dev),
                vals[i][perm.to(dev)],
                max_ts=int(ts.max().item()),
            )
        )
    out = []
    flow = Dataflow("reclaim")
    s = op.input("inp", flow, TestingSource(batches))
    keyed = op.key_on("k", s, lambda b: "shard-0")
    clock = EventClock(
        ts_getter=lambda it: it, wait_for_system_duration=timedelta(0)
    )
    wo = w.fold_window(
        "fw", keyed, clock,
        TumblingWindower(align_to=ALIGN, length=timedelta(milliseconds=LEN_MS)),
        lambda: -1, w.device_max(lambda it: it), max,
    )
    op.output("out", wo.down, TestingSink(out))
    run_main(flow)
    assert all(wid == COLUMNAR_WINDOW_ID for _k, (wid, _rb) in out)
    keys = torch.cat([rb.keys for _k, (_w, rb) in out]).to(torch.int64)
    ts = torch.cat([rb.ts for _k, (_w, rb) in out])
    got = torch.cat([rb.vals for _k, (_w, rb) in out])
    assert keys.numel() == n_keys * n_win
    assert bool(((ts - ALIGN_MS) % LEN_MS == 0).all().item())
    win = (ts - ALIGN_MS) // LEN_MS
    cell = win * n_keys + keys
    assert bool(((keys >= 0) & (keys < n_keys)).all().item())
    assert bool(((win >= 0) & (win < n_win)).all().item())
    # Every cell exactly once ...
    assert torch.unique(cell).numel() == n_keys * n_win
    # ... with its own value.
    assert torch.equal(got, vals.reshape(-1)[cell])
