"""Sliding stats windows on the device: `k_stats_pane_close` behind
`SlidingStatsAggState.close_due` / `close_below` / `close_all`, and
`keyed_stats_agg(offset=...)`.

Events are aggregated into panes of ``g = gcd(length, offset)`` by the
tumbling insert kernels; a close folds the panes of every due window
into a fold table, rebuilds the panes that an open window still needs
in a fresh table and forgets the rest.  The oracle is a brute-force
group-by over `_SlidingWindowerLogic.intersects`, the host windower;
sums wrap mod 2^64 and nothing has a tolerance.  Every test checks that
no (key, window) comes out twice, that the closes plus `close_all`
equal the oracle, and that each close returns exactly the windows in
``[old horizon, new horizon)``.

The kernel walks the table in chunks of 2,048 slots (256 threads x 8),
so the shape cases use tables of half a chunk, one chunk and four
chunks.
"""

import functools
from datetime import datetime, timedelta, timezone

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import bytewax_amd.operators as op  # noqa: E402
from bytewax_amd.dataflow import Dataflow  # noqa: E402
from bytewax_amd.gpu import RecordBatch, _ms  # noqa: E402
from bytewax_amd.gpu.operators import keyed_stats_agg  # noqa: E402
from bytewax_amd.gpu.state import SlidingStatsAggState  # noqa: E402
from bytewax_amd.operators.windowing import (  # noqa: E402
    _SlidingWindowerLogic,
    _SlidingWindowerState,
)
from bytewax_amd.testing import TestingSink, TestingSource, run_main  # noqa: E402

pytestmark = pytest.mark.gpu

ALIGN = datetime(2024, 1, 1, tzinfo=timezone.utc)
ALIGN_MS = _ms(ALIGN)
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
COLS = ("keys", "wins", "cnt", "sum", "min", "max")
FILLS = (-1, 0, 0, I64_MAX, I64_MIN)  # an empty slot of the five arrays
#: (len_ms, off_ms): g = 20 s, L = 3, o = 1, and g = 5 s, L = 12,
#: o = 5, where the offset does not divide the length.
GEOMS = [(60_000, 20_000), (60_000, 25_000)]


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


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
    ref, memo = {}, {}
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


def _pane_oracle(g, keys, x, vals):
    """The (key, pane) cells of the same events: tumbling windows of
    the pane width, by the same windower."""
    return _oracle(g, g, keys, x, vals)


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


def _direct(dev, len_ms, off_ms, slots_pow, **kw):
    kw.setdefault("out_cap", 1 << 13)
    st = SlidingStatsAggState(
        dev, ALIGN_MS, len_ms, off_ms, radix=False, slots_pow=slots_pow, **kw
    )
    assert st.nslots == 1 << slots_pow
    return st


def _table_cells(st):
    """The live table read back from its five arrays."""
    arrays = [
        t.cpu().numpy() for t in (st.tkeys, st.tcnt, st.tsum, st.tmin, st.tmax)
    ]
    used = np.flatnonzero(arrays[0] != -1)
    cells = {}
    for i in used.tolist():
        packed = int(arrays[0][i]) & ((1 << 64) - 1)
        key = (packed & 0xFFFFFFFF) - ((packed & 0x80000000) << 1)
        pane = (packed >> 32) - ((packed >> 32 & 0x80000000) << 1)
        assert (key, pane) not in cells
        cells[(key, pane)] = tuple(int(a[i]) for a in arrays[1:])
    return cells


def _assert_fresh(tables, nslots):
    assert tables is not None
    for t, fill in zip(tables, FILLS):
        assert t.numel() == nslots
        assert bool((t == fill).all().item())


def _close_checked(st, horizon, ref, panes, got):
    """One `close_below` (`close_all` if `horizon` is None): its rows
    are the oracle's windows in [old horizon, new horizon); afterwards
    the live table holds exactly the panes at or above `pane_keep`
    with their four values, and the fold table and the retired table
    are back to the empty fills."""
    old = st.win_horizon
    out = st.close_all() if horizon is None else st.close_below(horizon)
    new = st.win_horizon
    assert new == ((1 << 40) if horizon is None else max(old, horizon))
    rows = _got(out)
    assert rows == {c: v for c, v in ref.items() if old <= c[1] < new}
    assert (out is None) == (not rows)
    _got(out, got)
    pane_keep = new * st.panes_per_offset
    if new > old:
        assert st.closed_horizon == pane_keep
    assert _table_cells(st) == {
        c: v for c, v in panes.items() if c[1] >= pane_keep
    }
    assert int(st.error_flag.item()) == 0
    if st.tables_alt is not None:
        _assert_fresh(st.tables_alt, st.nslots)
        _assert_fresh(st.fold, st.fold_slots)
    return rows


# -- close-kernel shapes -------------------------------------------------

SPAN_MS = 200_000


@functools.lru_cache(maxsize=None)
def _shape_case(len_ms, off_ms, slots_pow):
    """Events that fill every (key, pane) cell of `SPAN_MS`, the table
    at most half full, with the window and the pane oracle."""
    g = int(np.gcd(len_ms, off_ms))
    n_panes = SPAN_MS // g
    n_keys = (1 << slots_pow) // (2 * n_panes)
    rng = np.random.default_rng(slots_pow * 100 + n_panes)
    keys = np.repeat(np.arange(n_keys), n_panes)
    pane = np.tile(np.arange(n_panes), n_keys)
    extra = rng.integers(0, keys.size, keys.size // 2)
    keys = np.r_[keys, keys[extra]].astype(np.int32)
    pane = np.r_[pane, pane[extra]]
    x = pane * g + rng.integers(0, g, keys.size)
    vals = rng.integers(-(1 << 40), 1 << 40, keys.size)
    events = (keys, x, vals)
    panes = _pane_oracle(g, *events)
    assert len(panes) == n_keys * n_panes <= (1 << slots_pow) // 2
    return events, _oracle(len_ms, off_ms, *events), panes


@pytest.mark.parametrize("slots_pow", [10, 11, 13])
@pytest.mark.parametrize("len_ms,off_ms", GEOMS)
def test_close_sequence_shapes(len_ms, off_ms, slots_pow):
    """Nothing due; a due window that shares panes with an open one;
    the horizon moved by one window, then by many; everything due."""
    dev = _gpu()
    events, ref, panes = _shape_case(len_ms, off_ms, slots_pow)
    st = _direct(dev, len_ms, off_ms, slots_pow)
    _insert(st, events)
    assert _table_cells(st) == panes
    n_w, n_o = st.panes_per_window, st.panes_per_offset
    first_w = min(w for _k, w in ref)
    assert first_w == 1 - (-(-len_ms // off_ms))  # opened before `align`
    got = {}
    # Nothing due: no window ends below the first one.  Nothing is
    # allocated and the table is unchanged.
    assert _close_checked(st, first_w, ref, panes, got) == {}
    assert st.tables_alt is None and st.fold is None
    # Windows up to 1 close; window 2 stays open and shares panes with
    # them.  Both sides of `pane_keep` hold cells.
    rows = _close_checked(st, 2, ref, panes, got)
    assert {w for _k, w in rows} == set(range(first_w, 2))
    pane_keep = 2 * n_o
    assert (0, pane_keep) in panes and (0, pane_keep - 1) in panes
    live = _table_cells(st)
    assert (0, pane_keep) in live and (0, pane_keep - 1) not in live
    assert any(
        2 * n_o <= p < 1 * n_o + n_w for _k, p in live
    ), "a pane of closed window 1 is still needed by open window 2"
    # The same horizon again, and one below it: nothing happens.
    assert _close_checked(st, 2, ref, panes, got) == {}
    assert _close_checked(st, 0, ref, panes, got) == {}
    # By one window, then by many.
    rows = _close_checked(st, 3, ref, panes, got)
    assert {w for _k, w in rows} == {2}
    rows = _close_checked(st, 6, ref, panes, got)
    assert {w for _k, w in rows} == {3, 4, 5}
    # Everything that is left.
    rows = _close_checked(st, None, ref, panes, got)
    assert rows and min(w for _k, w in rows) == 6
    assert got == ref
    assert st.close_all() is None


@pytest.mark.parametrize("slots_pow", [10, 11, 13])
@pytest.mark.parametrize("len_ms,off_ms", GEOMS)
def test_every_pane_due_in_the_first_close(len_ms, off_ms, slots_pow):
    dev = _gpu()
    events, ref, panes = _shape_case(len_ms, off_ms, slots_pow)
    st = _direct(dev, len_ms, off_ms, slots_pow)
    _insert(st, events)
    got = {}
    _close_checked(st, None, ref, panes, got)
    assert got == ref
    assert int((st.tkeys != -1).sum().item()) == 0


@pytest.mark.parametrize("len_ms,off_ms", GEOMS)
def test_nothing_due_after_the_tables_exist(len_ms, off_ms):
    """A horizon that advances past no pane's last window: None, and
    the rebuilt table holds what the old one held."""
    dev = _gpu()
    g = int(np.gcd(len_ms, off_ms))
    early = (np.arange(20, dtype=np.int32), np.arange(20) * 7, np.arange(20) - 9)
    far = (np.arange(20, dtype=np.int32), 40 * len_ms + np.arange(20), np.arange(20))
    ref = _oracle(len_ms, off_ms, *_cat([early, far]))
    st = _direct(dev, len_ms, off_ms, 10)
    _insert(st, early)
    _insert(st, far)
    got = {}
    _close_checked(st, 10, ref, _pane_oracle(g, *_cat([early, far])), got)
    assert st.tables_alt is not None
    far_panes = _pane_oracle(g, *far)
    # Windows 10 .. 19 hold no event.
    assert _close_checked(st, 20, ref, far_panes, got) == {}
    assert _table_cells(st) == far_panes
    _close_checked(st, None, ref, far_panes, got)
    assert got == ref


# -- edges ---------------------------------------------------------------


@pytest.mark.parametrize("len_ms,off_ms", GEOMS)
def test_edge_keys_values_and_windows_before_the_alignment(len_ms, off_ms):
    """Key -1 in the first pane folds into window -1, whose plain
    packing would be the empty-slot sentinel; extreme keys and values;
    a sum that wraps; a key with a single pane."""
    dev = _gpu()
    g = int(np.gcd(len_ms, off_ms))
    keys = np.array(
        [-1, -1, I32_MIN, I32_MAX, 7, 7, 8, 8, 9, -1], dtype=np.int32
    )
    x = np.array([0, 1, 0, g - 1, 3, 4, 5, 6, 3 * len_ms + 1, 2 * len_ms])
    vals = np.array(
        [5, -6, I64_MIN, I64_MAX, I64_MAX, I64_MAX, I64_MIN, I64_MIN, 11, 1]
    )
    events = (keys, x, vals)
    ref = _oracle(len_ms, off_ms, *events)
    panes = _pane_oracle(g, *events)
    n_back = -(-len_ms // off_ms) - 1
    assert {w for k, w in ref if k == -1 and w <= 0} == set(range(-n_back, 1))
    assert ref[(7, 0)][1] == -2 and ref[(8, 0)][1] == 0  # wrapped sums
    assert sum(1 for k, _p in panes if k == 9) == 1  # one pane only
    st = _direct(dev, len_ms, off_ms, 10)
    _insert(st, events)
    got = {}
    rows = _close_checked(st, 1, ref, panes, got)
    assert (-1, -1) in rows and (I32_MIN, -n_back) in rows
    assert rows[(I32_MAX, 0)] == (1, I64_MAX, I64_MAX, I64_MAX)
    _close_checked(st, None, ref, panes, got)
    assert got == ref


# -- fold-table overflow -------------------------------------------------


def test_fold_table_overflow_raises():
    dev = _gpu()
    events, ref, _panes = _shape_case(60_000, 20_000, 10)
    st = _direct(dev, 60_000, 20_000, 10, fold_slots_pow=4)
    assert st.fold_slots == 16 < len(ref)
    _insert(st, events)
    with pytest.raises(RuntimeError, match="overflowed"):
        st.close_all()


# -- radix insert --------------------------------------------------------

STEP_MS = 150_000


@functools.lru_cache(maxsize=None)
def _radix_stream():
    """Four watermark-ordered batches, about 50k events, and per batch
    a few late rows that lie below every event of the batch before."""
    batches, late = [], []
    for i in range(4):
        rng = np.random.default_rng(500 + i)
        n = 12_500
        keys = rng.integers(-300, 300, n).astype(np.int32)
        x = rng.integers(i * STEP_MS, (i + 1) * STEP_MS, n)
        vals = rng.integers(-(1 << 40), 1 << 40, n)
        batches.append((keys, x, vals))
        if i >= 2:
            lk = rng.integers(-300, 300, 200).astype(np.int32)
            lx = rng.integers((i - 2) * STEP_MS, (i - 1) * STEP_MS, 200)
            lv = rng.integers(-(1 << 40), 1 << 40, 200)
            late.append((lk, lx, lv))
        else:
            late.append(None)
    return batches, late


@functools.lru_cache(maxsize=None)
def _radix_ref(len_ms, off_ms):
    return _oracle(len_ms, off_ms, *_cat(_radix_stream()[0]))


@pytest.mark.parametrize("track_late", [False, True])
@pytest.mark.parametrize("ts_form", ["abs", "delta32"])
@pytest.mark.parametrize("len_ms,off_ms", GEOMS)
def test_radix_insert_three_closes(len_ms, off_ms, ts_form, track_late):
    dev = _gpu()
    batches, late = _radix_stream()
    ref = _radix_ref(len_ms, off_ms)
    st = SlidingStatsAggState(
        dev, ALIGN_MS, len_ms, off_ms, slots_pow=20, radix=True,
        track_late=track_late, wait_ms=0,
    )
    got, closes = {}, 0
    for i, b in enumerate(batches):
        if track_late and late[i] is not None:
            b = tuple(a[::-1].copy() for a in _cat([b, late[i]]))
        _insert(st, b, ts_form)
        if i == 0:
            continue
        old = st.win_horizon
        out = st.close_due(0)
        rows = _got(out)
        assert rows and all(old <= w < st.win_horizon for _k, w in rows)
        _got(out, got)
        closes += 1
    assert closes == 3
    if track_late:
        drained = st.take_late()
        assert st.take_late() is None
        rows = sorted(
            zip(
                drained.keys.cpu().tolist(),
                (drained.ts.cpu() - ALIGN_MS).tolist(),
                drained.vals.cpu().tolist(),
            )
        )
        want = _cat([lb for lb in late if lb is not None])
        assert rows == sorted(zip(*(a.tolist() for a in want)))
    _got(st.close_all(), got)
    assert got == ref
    assert int((st.tkeys != -1).sum().item()) == 0


# -- snapshot, operator, determinism ----------------------------------------


@pytest.mark.parametrize("len_ms,off_ms", GEOMS)
def test_snapshot_round_trip(len_ms, off_ms):
    dev = _gpu()
    batches, _late = _radix_stream()
    batches = [tuple(a[:3_000] for a in b) for b in batches]
    ref = _oracle(len_ms, off_ms, *_cat(batches))
    st = _direct(dev, len_ms, off_ms, 15, out_cap=1 << 15)
    got = {}
    for b in batches[:2]:
        _insert(st, b)
        _got(st.close_due(0), got)
    snap = st.snapshot_to_host()
    assert (snap["win_len_ms"], snap["off_ms"]) == (len_ms, off_ms)
    assert snap["win_horizon"] == st.win_horizon
    assert snap["n"] == len(_table_cells(st)) > 0
    st2 = _direct(dev, len_ms, off_ms, 15, out_cap=1 << 15)
    st2.restore_from_host(snap)
    assert st2.win_horizon == st.win_horizon
    assert st2.closed_horizon == st.closed_horizon
    assert _table_cells(st2) == _table_cells(st)
    for b in batches[2:]:
        _insert(st2, b)
        old = st2.win_horizon
        out = st2.close_due(0)
        assert all(old <= w < st2.win_horizon for _k, w in _got(out))
        _got(out, got)
    _got(st2.close_all(), got)
    assert got == ref
    other = _direct(dev, 2 * len_ms, off_ms, 15)
    with pytest.raises(ValueError, match="cannot restore"):
        other.restore_from_host(snap)


def _run_operator(dev, events, n_batches, len_ms, off_ms):
    keys, x, vals = events
    batches = [
        RecordBatch(
            torch.from_numpy(ks).to(dev),
            torch.from_numpy(ALIGN_MS + xs).to(dev),
            torch.from_numpy(vs).to(dev),
            max_ts=int(ALIGN_MS + xs.max()),
        )
        for ks, xs, vs in zip(
            *(np.array_split(a, n_batches) for a in (keys, x, vals))
        )
    ]
    out = []
    flow = Dataflow("sliding_stats_gpu")
    s = op.input("inp", flow, TestingSource(batches))
    agg = keyed_stats_agg(
        "stats",
        s,
        align_to=ALIGN,
        length=timedelta(milliseconds=len_ms),
        offset=timedelta(milliseconds=off_ms),
        device=str(dev),
        exchange=False,
    )
    op.output("out", agg, TestingSink(out))
    run_main(flow)
    got = {}
    for o in out:
        assert o["keys"].device.type == "cuda"
        _got(o, got)
    return got, len(out)


@functools.lru_cache(maxsize=None)
def _operator_events():
    rng = np.random.default_rng(77)
    n = 20_000
    keys = rng.integers(-100, 100, n).astype(np.int32)
    x = np.sort(rng.integers(0, 600_000, n))
    vals = rng.integers(-(1 << 40), 1 << 40, n)
    return keys, x, vals


@pytest.mark.parametrize("len_ms,off_ms", GEOMS)
def test_operator_against_the_oracle(len_ms, off_ms):
    dev = _gpu()
    events = _operator_events()
    got, n_out = _run_operator(dev, events, 10, len_ms, off_ms)
    assert n_out > 3  # windows closed while the stream ran
    assert got == _oracle(len_ms, off_ms, *events)


def test_two_runs_give_identical_rows():
    dev = _gpu()
    batches, _late = _radix_stream()

    def run():
        st = SlidingStatsAggState(
            dev, ALIGN_MS, 60_000, 25_000, slots_pow=20, radix=True
        )
        rows = []
        for b in batches:
            _insert(st, b)
            out = st.close_due(0)
            if out is not None:
                rows += list(zip(*(out[n].cpu().tolist() for n in COLS)))
        out = st.close_all()
        rows += list(zip(*(out[n].cpu().tolist() for n in COLS)))
        return sorted(rows)

    a, b = run(), run()
    assert a == b and len(a) == len(_radix_ref(60_000, 25_000))


# -- first close, end of input, rescale ---------------------------------------


def test_first_close_counts_due_panes_without_the_row_buffers():
    """The first close only asks whether any pane is due.  There are
    up to L due panes per key, more than `out_cap` here, while the
    window rows of the close fit."""
    dev = _gpu()
    len_ms, off_ms = 60_000, 25_000
    events, ref, panes = _shape_case(len_ms, off_ms, 11)
    due_panes = sum(1 for _k, p in panes if p < 12)
    rows = sum(1 for _k, w in ref if w < 1)
    assert rows <= 128 < due_panes
    st = _direct(dev, len_ms, off_ms, 11, out_cap=128)
    _insert(st, events)
    _close_checked(st, 1, ref, panes, {})


@pytest.mark.parametrize("len_ms,off_ms", GEOMS)
def test_close_eof_leaves_a_state_that_resumes(len_ms, off_ms):
    """`close_eof` returns every window from the horizon up and moves
    neither horizon nor any live pane; a snapshot taken after it
    continues the stream."""
    dev = _gpu()
    batches, _late = _radix_stream()
    batches = [tuple(a[:3_000] for a in b) for b in batches]
    st = _direct(dev, len_ms, off_ms, 15, out_cap=1 << 15)
    got = {}
    for b in batches[:2]:
        _insert(st, b)
        _got(st.close_due(0), got)
    horizons = (st.win_horizon, st.closed_horizon)
    table = _table_cells(st)
    so_far = _oracle(len_ms, off_ms, *_cat(batches[:2]))
    eof = _got(st.close_eof())
    assert eof == {c: v for c, v in so_far.items() if c[1] >= horizons[0]}
    assert (st.win_horizon, st.closed_horizon) == horizons
    assert _table_cells(st) == table
    _assert_fresh(st.fold, st.fold_slots)
    st2 = _direct(dev, len_ms, off_ms, 15, out_cap=1 << 15)
    st2.restore_from_host(st.snapshot_to_host())
    for b in batches[2:]:
        _insert(st2, b)
        _got(st2.close_due(0), got)
    _got(st2.close_eof(), got)
    assert got == _oracle(len_ms, off_ms, *_cat(batches))


@pytest.mark.parametrize("len_ms,off_ms", GEOMS)
def test_rescale_of_two_donors_with_different_horizons(len_ms, off_ms):
    """`merge_donors` on the device: the merged state adopts the
    furthest horizon, closes the donor that is behind up to it in a
    scratch state and continues with no (key, window) twice."""
    dev = _gpu()
    batches, _late = _radix_stream()
    batches = [tuple(a[:3_000] for a in b) for b in batches]
    got, parts, fed = {}, [], []
    for parity, n_fed in ((0, 3), (1, 2)):
        d = _direct(dev, len_ms, off_ms, 15, out_cap=1 << 15)
        for b in batches[:n_fed]:
            mine = tuple(a[b[0] % 2 == parity] for a in b)
            fed.append(mine)
            _insert(d, mine)
            _got(d.close_due(0), got)
        snap = d.snapshot_to_host()
        part = {c: snap[c] for c in COLS}
        part["meta"] = d.donor_meta(snap)
        parts.append(part)
    assert parts[0]["meta"]["win_horizon"] > parts[1]["meta"]["win_horizon"]
    st = _direct(dev, len_ms, off_ms, 15, out_cap=1 << 15)
    owed = st.merge_donors(parts)
    assert owed and st.win_horizon == parts[0]["meta"]["win_horizon"]
    assert st.closed_horizon == st.win_horizon * st.panes_per_offset
    for o in owed:
        _got(o, got)
    st.max_ts_host = int(ALIGN_MS + batches[2][1].max())
    fed.append(batches[3])
    _insert(st, batches[3])
    _got(st.close_due(0), got)
    _got(st.close_all(), got)
    assert got == _oracle(len_ms, off_ms, *_cat(fed))
    other = _direct(dev, 2 * len_ms, off_ms, 10)
    with pytest.raises(ValueError, match="cannot restore"):
        other.donor_meta(snap)
