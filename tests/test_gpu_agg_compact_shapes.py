"""COUNT segment aggregation with compact LDS cells, at the shapes where
it can go wrong.

The compact kernel keeps ``key | window delta (4 bits) | count`` in one
8-byte LDS cell, takes the delta against a per-segment base and sends
entries outside the delta range straight to the global table.  These
cases pin: vector head/tail peeling and pads, the small-table launch,
window ranges inside, at the edge of and far beyond the delta range,
keys whose bits look like the empty marker, same-address LDS atomics
with a spilling segment, a nearly full and an overfull table, and the
split scatter/aggregate calls on alternating buffers.

Every case runs under ``BYTEWAX_AGG`` unset (compact cells) and
``BYTEWAX_AGG=wide`` (16-byte cells), compares each result exactly
against a plain-Python ``Counter`` and requires the two to be equal.
"""

from collections import Counter
from datetime import datetime, timezone

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

ALIGN = datetime(2024, 1, 1, tzinfo=timezone.utc)
KNOBS = [None, "wide"]
SIZES = [1, 7, 8, 9, 4_095, 100_003]
INT32_MIN = -(1 << 31)
INT32_MAX = (1 << 31) - 1


def _skip_no_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _align_ms():
    from bytewax_amd.gpu import _ms

    return _ms(ALIGN)


def _ref(keys, ts, align_ms, len_ms):
    c = Counter()
    for k, t in zip(keys.tolist(), ts.tolist()):
        c[(k, (t - align_ms) // len_ms)] += 1
    return c


def _rows_to_counter(batch, state):
    if batch is None:
        return Counter()
    keys = batch.keys.cpu().tolist()
    wins = ((batch.ts.cpu() - state.align_ms) // state.off_ms).tolist()
    vals = batch.vals.cpu().tolist()
    got = Counter()
    for k, w, v in zip(keys, wins, vals):
        assert (k, w) not in got, "cell emitted twice"
        got[(k, w)] = v
    return got


def _set_knob(monkeypatch, knob):
    if knob is None:
        monkeypatch.delenv("BYTEWAX_AGG", raising=False)
    else:
        monkeypatch.setenv("BYTEWAX_AGG", knob)


def _insert_close(keys, ts, len_ms, max_batch=None, **state_kw):
    """One insert into a fresh COUNT state, then close everything.
    Returns (rows, error_flag, spilled entries)."""
    from bytewax_amd.gpu import AGG_COUNT, RecordBatch, WindowAggState

    kw = dict(slots_pow=18, region_bits=11)
    kw.update(state_kw)
    state = WindowAggState(
        torch.device("cuda:0"), _align_ms(), len_ms, AGG_COUNT, radix=True,
        max_batch=max_batch or int(keys.numel()), **kw,
    )
    state.insert(RecordBatch(keys.cuda(), ts.cuda()))
    spilled = int(state.rx_ov_cursor.item())
    got = _rows_to_counter(state.close_all(), state)
    return got, int(state.error_flag.item()), spilled, state


def _check_both(monkeypatch, keys, ts, len_ms, **kw):
    """Run under both knob values; each equals the reference and they
    equal each other.  Returns the per-knob (spilled, state)."""
    ref = _ref(keys, ts, _align_ms(), len_ms)
    results, extra = [], []
    for knob in KNOBS:
        _set_knob(monkeypatch, knob)
        got, err, spilled, state = _insert_close(keys, ts, len_ms, **kw)
        assert err == 0, f"error_flag set (BYTEWAX_AGG={knob})"
        assert got == ref, f"BYTEWAX_AGG={knob}"
        results.append(got)
        extra.append((spilled, state))
    assert results[0] == results[1]
    return ref, extra


def _uniform(n, seed, n_keys=20_000, span_ms=300_000):
    g = torch.Generator().manual_seed(seed)
    keys = torch.randint(0, n_keys, (n,), dtype=torch.int32, generator=g)
    ts = _align_ms() + torch.randint(
        0, span_ms, (n,), dtype=torch.int64, generator=g
    )
    return keys, ts


def _odd_cap_max_batch(n, n_regions):
    """Smallest max_batch >= n whose fixed-layout capacity is odd (same
    arithmetic as WindowAggState._alloc_rx)."""
    mb = max(n, 1)
    while True:
        per_region = max(32, -(-mb * 5 // 2) // n_regions + 1)
        if per_region % 2 == 1:
            return mb, per_region
        mb += 1


@pytest.mark.parametrize("n", SIZES)
def test_staged_sizes(n, monkeypatch):
    """Staged layout, 2^13-slot segments: counts shorter than one
    vector / one chunk, granule pads."""
    _skip_no_gpu()
    monkeypatch.delenv("BYTEWAX_SCATTER", raising=False)
    keys, ts = _uniform(n, 1_000 + n)
    _check_both(monkeypatch, keys, ts, 60_000)


@pytest.mark.parametrize("n", SIZES)
def test_fixed_layout_odd_capacity_sizes(n, monkeypatch):
    """Fixed layout with an odd per-segment capacity: every other
    segment starts only 8-byte aligned (head peeling), 2^11-slot
    segments (256-thread launch)."""
    _skip_no_gpu()
    monkeypatch.setenv("BYTEWAX_SCATTER", "fixed")
    n_regions = (1 << 18) >> 11
    mb, per_region = _odd_cap_max_batch(n, n_regions)
    assert per_region % 2 == 1
    keys, ts = _uniform(n, 2_000 + n)
    _, extra = _check_both(monkeypatch, keys, ts, 60_000, max_batch=mb)
    for _, state in extra:
        assert state.rx_packed.numel() == per_region * n_regions


@pytest.mark.parametrize("layout", ["staged", "fixed"])
@pytest.mark.parametrize("region_bits", [8, 10])
def test_small_tables(layout, region_bits, monkeypatch):
    """LDS tables of 2^8, 2^10 (fixed layout: one region per segment)
    and 2^10, 2^12 slots (staged: four regions per segment)."""
    _skip_no_gpu()
    monkeypatch.setenv("BYTEWAX_SCATTER", layout)
    keys, ts = _uniform(6_001, 3_000 + region_bits, n_keys=1_000)
    _check_both(
        monkeypatch, keys, ts, 60_000, slots_pow=14, region_bits=region_bits
    )


def test_forty_windows_in_one_batch(monkeypatch):
    """Timestamps spanning 40 windows: most entries are outside any
    15-window delta range and take the direct path."""
    _skip_no_gpu()
    monkeypatch.delenv("BYTEWAX_SCATTER", raising=False)
    keys, ts = _uniform(50_000, 41, n_keys=500, span_ms=40_000)
    ref, _ = _check_both(monkeypatch, keys, ts, 1_000)
    assert len({w for _, w in ref}) == 40


@pytest.mark.parametrize("n_windows", [15, 16])
def test_delta_range_edge(n_windows, monkeypatch):
    """Exactly 15 and exactly 16 distinct consecutive windows: the
    largest set a cell's delta can cover, and one more."""
    _skip_no_gpu()
    monkeypatch.delenv("BYTEWAX_SCATTER", raising=False)
    keys, ts = _uniform(30_000, 50 + n_windows, n_keys=300,
                        span_ms=n_windows * 1_000)
    # Every window present, ascending at the front of the batch.
    ts[:n_windows] = _align_ms() + torch.arange(n_windows) * 1_000
    ref, _ = _check_both(monkeypatch, keys, ts, 1_000)
    assert sorted({w for _, w in ref}) == list(range(n_windows))


def test_windows_below_first_entry(monkeypatch):
    """The first entry carries the highest window of the batch; all
    others lie up to 12 windows below it."""
    _skip_no_gpu()
    monkeypatch.delenv("BYTEWAX_SCATTER", raising=False)
    g = torch.Generator().manual_seed(61)
    n = 30_000
    # One key, so every entry shares the first entry's segment.
    keys = torch.full((n,), 77, dtype=torch.int32)
    ts = _align_ms() + 100_000 + torch.randint(
        0, 12_000, (n,), dtype=torch.int64, generator=g
    )
    ts[0] = _align_ms() + 100_000 + 12_500
    ref, _ = _check_both(monkeypatch, keys, ts, 1_000)
    assert len(ref) == 13
    # Several keys: segments whose first entry is anywhere in the range.
    keys = torch.randint(0, 200, (n,), dtype=torch.int32, generator=g)
    _check_both(monkeypatch, keys, ts, 1_000)


def test_keys_that_look_like_the_empty_marker(monkeypatch):
    """Keys -1, INT32_MIN, INT32_MAX and 0 across 20 windows."""
    _skip_no_gpu()
    monkeypatch.delenv("BYTEWAX_SCATTER", raising=False)
    g = torch.Generator().manual_seed(71)
    n = 10_000
    pool = torch.tensor([-1, INT32_MIN, INT32_MAX, 0], dtype=torch.int32)
    keys = pool[torch.randint(0, 4, (n,), generator=g)]
    ts = _align_ms() + torch.randint(
        0, 20_000, (n,), dtype=torch.int64, generator=g
    )
    ref, _ = _check_both(monkeypatch, keys, ts, 1_000)
    assert len(ref) == 80


@pytest.mark.parametrize("n_hot", [1, 3])
def test_hot_keys(n_hot, monkeypatch):
    """100k events on one or three keys: same-address LDS atomics, a
    segment past its capacity, entries in the spill."""
    _skip_no_gpu()
    monkeypatch.delenv("BYTEWAX_SCATTER", raising=False)
    n = 100_000
    keys = (torch.arange(n, dtype=torch.int64) % n_hot * 7_919 + 5).to(
        torch.int32
    )
    ts = torch.full((n,), _align_ms() + 1_234, dtype=torch.int64)
    ref, extra = _check_both(monkeypatch, keys, ts, 60_000)
    assert len(ref) == n_hot
    for spilled, _ in extra:
        assert spilled > 0


def test_nearly_full_table(monkeypatch):
    """Distinct keys at about 90 % of a 2^14-slot table."""
    _skip_no_gpu()
    monkeypatch.delenv("BYTEWAX_SCATTER", raising=False)
    n = (1 << 14) * 9 // 10
    keys = (torch.randperm(n, generator=torch.Generator().manual_seed(81))
            .to(torch.int32))
    ts = torch.full((n,), _align_ms() + 5, dtype=torch.int64)
    ref, _ = _check_both(monkeypatch, keys, ts, 60_000, slots_pow=14)
    assert len(ref) == n


def test_overfull_table_sets_error_flag(monkeypatch):
    """More distinct cells than slots: the error flag is raised,
    whichever kernel runs."""
    _skip_no_gpu()
    monkeypatch.delenv("BYTEWAX_SCATTER", raising=False)
    n = 20_000
    keys = torch.arange(n, dtype=torch.int32)
    ts = torch.full((n,), _align_ms() + 5, dtype=torch.int64)
    for knob in KNOBS:
        _set_knob(monkeypatch, knob)
        from bytewax_amd.gpu import AGG_COUNT, RecordBatch, WindowAggState

        state = WindowAggState(
            torch.device("cuda:0"), _align_ms(), 60_000, AGG_COUNT,
            slots_pow=14, radix=True, region_bits=11, max_batch=n,
        )
        state.insert(RecordBatch(keys.cuda(), ts.cuda()))
        assert int(state.error_flag.item()) != 0, f"BYTEWAX_AGG={knob}"


def test_split_calls_on_alternating_buffers(monkeypatch):
    """Two inserts through radix_scatter_only / radix_agg_only, one on
    each buffer set, with a watermark close in between."""
    _skip_no_gpu()
    from bytewax_amd.gpu import AGG_COUNT, WindowAggState

    monkeypatch.delenv("BYTEWAX_SCATTER", raising=False)
    align_ms = _align_ms()
    len_ms, step_ms = 1_000, 5_000
    sizes = [60_001, 9]
    g = torch.Generator().manual_seed(91)
    batches = []
    ref = Counter()
    for i, n in enumerate(sizes):
        keys = torch.randint(0, 3_000, (n,), dtype=torch.int32, generator=g)
        ts = torch.randint(0, step_ms, (n,), dtype=torch.int64, generator=g)
        base = align_ms + i * step_ms
        ref.update(_ref(keys, ts + base, align_ms, len_ms))
        batches.append((keys, ts, base))
    results = []
    for knob in KNOBS:
        _set_knob(monkeypatch, knob)
        state = WindowAggState(
            torch.device("cuda:0"), align_ms, len_ms, AGG_COUNT,
            slots_pow=18, radix=True, region_bits=11, max_batch=max(sizes),
        )
        got = Counter()
        for i, (keys, ts, base) in enumerate(batches):
            state.insert_pipelined(
                keys.cuda(), ts.cuda(), None, base, [], [],
                base + step_ms - 1,
            )
            if i == 0:
                closed = _rows_to_counter(state.close_due(), state)
                assert len(closed) > 0
                got.update(closed)
        tail = _rows_to_counter(state.close_all(), state)
        assert not (set(tail) & set(got)), "cell closed twice"
        got.update(tail)
        assert int(state.error_flag.item()) == 0
        assert got == ref, f"BYTEWAX_AGG={knob}"
        results.append(got)
    assert results[0] == results[1]
