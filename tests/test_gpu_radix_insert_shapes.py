"""Radix insert (scatter + segment aggregation) at awkward shapes.

The segment aggregation streams each scatter segment with 16-byte
vector loads in unrolled chunks.  These cases pin the places where
such code can go wrong: counts shorter than one vector / one chunk,
8-byte-aligned segment starts (fixed layout, odd capacity), sentinel
pads, capacity overflow into the spill, and the alternating buffer
parities of the pipelined insert.  The window-delta cases (window ids
far from the batch base, timestamps below it, several bases in one
call) guard any scatter that encodes the window relative to a base
instead of carrying it whole.  Every result is compared exactly
against the plain-Python ``Counter`` reference.
"""

from collections import Counter
from datetime import datetime, timezone

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

ALIGN = datetime(2024, 1, 1, tzinfo=timezone.utc)

SIZES = [1, 7, 8, 9, 4_095, 100_003]


def _skip_no_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _ref(keys, ts, vals, align_ms, len_ms):
    c = Counter()
    if vals is None:
        for k, t in zip(keys.tolist(), ts.tolist()):
            c[(k, (t - align_ms) // len_ms)] += 1
    else:
        for k, t, v in zip(keys.tolist(), ts.tolist(), vals.tolist()):
            c[(k, (t - align_ms) // len_ms)] += v
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


def _data(n, seed, n_keys=20_000, span_ms=300_000):
    from bytewax_amd.gpu import _ms

    g = torch.Generator().manual_seed(seed)
    align_ms = _ms(ALIGN)
    keys = torch.randint(0, n_keys, (n,), dtype=torch.int32, generator=g)
    ts = align_ms + torch.randint(
        0, span_ms, (n,), dtype=torch.int64, generator=g
    )
    vals = torch.randint(0, 100, (n,), dtype=torch.int64, generator=g)
    return align_ms, keys, ts, vals


def _odd_cap_max_batch(n, n_regions):
    """Smallest max_batch >= n whose fixed-layout capacity is odd (same
    arithmetic as WindowAggState._alloc_rx)."""
    mb = max(n, 1)
    while True:
        per_region = max(32, -(-mb * 5 // 2) // n_regions + 1)
        if per_region % 2 == 1:
            return mb, per_region
        mb += 1


def _run_one(mode_name, n, seed, max_batch):
    from bytewax_amd.gpu import AGG_COUNT, AGG_SUM, RecordBatch, WindowAggState

    align_ms, keys, ts, vals = _data(n, seed)
    len_ms = 60_000  # 300 s span: five windows
    mode = AGG_COUNT if mode_name == "count" else AGG_SUM
    ref = _ref(keys, ts, vals if mode == AGG_SUM else None, align_ms, len_ms)
    state = WindowAggState(
        torch.device("cuda:0"), align_ms, len_ms, mode,
        slots_pow=18, radix=True, region_bits=11, max_batch=max_batch,
    )
    state.insert(RecordBatch(keys.cuda(), ts.cuda(), vals.cuda()))
    got = _rows_to_counter(state.close_all(), state)
    assert int(state.error_flag.item()) == 0
    assert got == ref
    return state


@pytest.mark.parametrize("mode_name", ["count", "sum"])
@pytest.mark.parametrize("n", SIZES)
def test_staged_small_and_odd_sizes(mode_name, n, monkeypatch):
    """Granule padding, EMPTY_SLOT pads, tails shorter than one vector
    and shorter than one unrolled chunk."""
    _skip_no_gpu()
    monkeypatch.delenv("BYTEWAX_SCATTER", raising=False)
    _run_one(mode_name, n, 100 + n, max_batch=n)


@pytest.mark.parametrize("mode_name", ["count", "sum"])
@pytest.mark.parametrize("n", SIZES)
def test_fixed_layout_odd_capacity(mode_name, n, monkeypatch):
    """Fixed layout with an odd per-segment capacity: every other
    segment starts only 8-byte aligned and counts are arbitrary."""
    _skip_no_gpu()
    monkeypatch.setenv("BYTEWAX_SCATTER", "fixed")
    n_regions = (1 << 18) >> 11
    mb, per_region = _odd_cap_max_batch(n, n_regions)
    assert per_region % 2 == 1
    state = _run_one(mode_name, n, 200 + n, max_batch=mb)
    assert state.rx_packed.numel() == per_region * n_regions


@pytest.mark.parametrize("mode_name", ["count", "sum"])
@pytest.mark.parametrize("n", [1, 7, 50])
def test_tiny_buffer_falls_back_to_fixed(mode_name, n, monkeypatch):
    """Scatter buffers so small that the granule-rounded staged capacity
    is zero: the insert switches to the fixed layout on its own (one
    slot per segment here; the rest goes through the spill)."""
    _skip_no_gpu()
    from bytewax_amd.gpu import AGG_COUNT, AGG_SUM, RecordBatch, WindowAggState

    monkeypatch.delenv("BYTEWAX_SCATTER", raising=False)
    align_ms, keys, ts, vals = _data(n, 300 + n)
    len_ms = 60_000
    mode = AGG_COUNT if mode_name == "count" else AGG_SUM
    ref = _ref(keys, ts, vals if mode == AGG_SUM else None, align_ms, len_ms)
    dev = torch.device("cuda:0")
    state = WindowAggState(
        dev, align_ms, len_ms, mode,
        slots_pow=18, radix=True, region_bits=11, max_batch=64,
    )
    # 32 staged segments x 7 < one granule each; 128 fixed segments x 1.
    state.rx_packed = torch.empty(250, dtype=torch.int64, device=dev)
    if mode == AGG_SUM:
        state.rx_vals = torch.empty(250, dtype=torch.int64, device=dev)
    state.insert(RecordBatch(keys.cuda(), ts.cuda(), vals.cuda()))
    got = _rows_to_counter(state.close_all(), state)
    assert int(state.error_flag.item()) == 0
    assert got == ref


@pytest.mark.parametrize("layout", ["staged", "fixed"])
@pytest.mark.parametrize("n_hot", [1, 2])
def test_hot_key_overflows_segment(layout, n_hot, monkeypatch):
    """All events on one or two keys: the segment overflows its
    capacity, so the spill and the count clamp both run."""
    _skip_no_gpu()
    from bytewax_amd.gpu import AGG_COUNT, RecordBatch, WindowAggState, _ms

    monkeypatch.setenv("BYTEWAX_SCATTER", layout)
    n = 100_000
    align_ms = _ms(ALIGN)
    len_ms = 60_000
    keys = (torch.arange(n, dtype=torch.int64) % n_hot * 7_919 + 5).to(
        torch.int32
    )
    ts = torch.full((n,), align_ms + 1_234, dtype=torch.int64)
    ref = _ref(keys, ts, None, align_ms, len_ms)
    assert len(ref) == n_hot
    state = WindowAggState(
        torch.device("cuda:0"), align_ms, len_ms, AGG_COUNT,
        slots_pow=18, radix=True, region_bits=11, max_batch=n,
    )
    state.insert(RecordBatch(keys.cuda(), ts.cuda()))
    # More events than any one segment holds went to the spill.
    assert int(state.rx_ov_cursor.item()) > 0
    got = _rows_to_counter(state.close_all(), state)
    assert int(state.error_flag.item()) == 0
    assert got == ref


def _escape_data():
    """1 ms windows over a 100 000 ms span: ~100 000 distinct window ids
    relative to any one base."""
    from bytewax_amd.gpu import _ms

    g = torch.Generator().manual_seed(77)
    n = 100_000
    align_ms = _ms(ALIGN)
    keys = torch.randint(0, 50, (n,), dtype=torch.int32, generator=g)
    ts = align_ms + torch.randint(
        0, 100_000, (n,), dtype=torch.int64, generator=g
    )
    return n, align_ms, keys, ts


@pytest.fixture(scope="module")
def escape_case():
    n, align_ms, keys, ts = _escape_data()
    return n, align_ms, keys, ts, _ref(keys, ts, None, align_ms, 1)


def test_window_delta_escape_int64_absolute(escape_case, monkeypatch):
    _skip_no_gpu()
    from bytewax_amd.gpu import AGG_COUNT, RecordBatch, WindowAggState

    monkeypatch.delenv("BYTEWAX_SCATTER", raising=False)
    n, align_ms, keys, ts, ref = escape_case
    state = WindowAggState(
        torch.device("cuda:0"), align_ms, 1, AGG_COUNT,
        slots_pow=18, radix=True, region_bits=11, max_batch=n,
    )
    state.insert(RecordBatch(keys.cuda(), ts.cuda()))
    assert int(state.max_ts_dev.item()) == int(ts.max())
    got = _rows_to_counter(state.close_all(), state)
    assert int(state.error_flag.item()) == 0
    assert got == ref


def test_window_delta_escape_int32_segments(escape_case, monkeypatch):
    """Segmented int32-delta form: two segments with different bases in
    one call, one base ABOVE most of its timestamps (negative deltas),
    the other far below its own (deltas up to the whole span)."""
    _skip_no_gpu()
    from bytewax_amd.gpu import AGG_COUNT, WindowAggState, _LazyTsBatch

    monkeypatch.delenv("BYTEWAX_SCATTER", raising=False)
    n, align_ms, keys, ts, ref = escape_case
    seg_counts = [n // 3, n - n // 3]
    seg_bases = [align_ms + 90_000, align_ms - 1_000_000]
    ts32 = torch.empty(n, dtype=torch.int32)
    off = 0
    for cnt, base in zip(seg_counts, seg_bases):
        ts32[off : off + cnt] = (ts[off : off + cnt] - base).to(torch.int32)
        off += cnt
    assert int(ts32[: seg_counts[0]].min()) < 0
    lz = _LazyTsBatch(
        keys.cuda(), ts32.cuda(), seg_counts, seg_bases, None, int(ts.max())
    )
    state = WindowAggState(
        torch.device("cuda:0"), align_ms, 1, AGG_COUNT,
        slots_pow=18, radix=True, region_bits=11, max_batch=n,
    )
    state.insert_lazy(lz)
    assert int(state.max_ts_dev.item()) == int(ts.max())
    got = _rows_to_counter(state.close_all(), state)
    assert int(state.error_flag.item()) == 0
    assert got == ref


def test_window_delta_escape_int32_single_base(escape_case, monkeypatch):
    """Plain int32 deltas against one ts_base in the middle of the
    span (the bench's timestamp form), half of them below the base."""
    _skip_no_gpu()
    from bytewax_amd.gpu import AGG_COUNT, RecordBatch, WindowAggState

    monkeypatch.delenv("BYTEWAX_SCATTER", raising=False)
    n, align_ms, keys, ts, ref = escape_case
    base = align_ms + 50_000
    ts32 = (ts - base).to(torch.int32)
    assert int(ts32.min()) < 0 < int(ts32.max())
    state = WindowAggState(
        torch.device("cuda:0"), align_ms, 1, AGG_COUNT,
        slots_pow=18, radix=True, region_bits=11, max_batch=n,
    )
    state.insert(
        RecordBatch(keys.cuda(), ts32.cuda(), None, ts_base=base)
    )
    got = _rows_to_counter(state.close_all(), state)
    assert int(state.error_flag.item()) == 0
    assert got == ref


@pytest.mark.parametrize("mode_name", ["count", "sum"])
def test_pipelined_accumulation_both_parities(mode_name, monkeypatch):
    """Six batches through insert_pipelined (each buffer parity used
    three times) with a watermark close after the third: closed rows
    plus close_all() must equal the reference."""
    _skip_no_gpu()
    from bytewax_amd.gpu import AGG_COUNT, AGG_SUM, WindowAggState, _ms

    monkeypatch.delenv("BYTEWAX_SCATTER", raising=False)
    align_ms = _ms(ALIGN)
    len_ms = 1_000
    step_ms = 5_000
    mode = AGG_COUNT if mode_name == "count" else AGG_SUM
    dev = torch.device("cuda:0")
    # Shrinking and odd sizes: a stale cursor from a bigger batch on the
    # same parity would over-read.
    sizes = [60_001, 50_000, 40_003, 9, 30_000, 1]
    g = torch.Generator().manual_seed(5)
    ref = Counter()
    state = WindowAggState(
        dev, align_ms, len_ms, mode,
        slots_pow=18, radix=True, region_bits=11, max_batch=max(sizes),
    )
    got = Counter()
    for i, n in enumerate(sizes):
        keys = torch.randint(0, 3_000, (n,), dtype=torch.int32, generator=g)
        ts = torch.randint(0, step_ms, (n,), dtype=torch.int64, generator=g)
        vals = torch.randint(0, 100, (n,), dtype=torch.int64, generator=g)
        base = align_ms + i * step_ms
        ref.update(
            _ref(keys, ts + base, vals if mode == AGG_SUM else None,
                 align_ms, len_ms)
        )
        state.insert_pipelined(
            keys.cuda(), ts.cuda(),
            vals.cuda() if mode == AGG_SUM else None,
            base, [], [], base + step_ms - 1,
        )
        if i == 2:
            closed = _rows_to_counter(state.close_due(), state)
            assert len(closed) > 0
            got.update(closed)
    tail = _rows_to_counter(state.close_all(), state)
    assert not (set(tail) & set(got)), "cell closed twice"
    got.update(tail)
    assert int(state.error_flag.item()) == 0
    assert got == ref


def test_sliding_windows_on_radix_path(monkeypatch):
    """60 s / 20 s sliding windows keep the expanding scatter body."""
    _skip_no_gpu()
    from bytewax_amd.gpu import AGG_COUNT, RecordBatch, WindowAggState, _ms

    monkeypatch.delenv("BYTEWAX_SCATTER", raising=False)
    g = torch.Generator().manual_seed(13)
    n = 50_000
    align_ms = _ms(ALIGN)
    len_ms, off_ms = 60_000, 20_000
    keys = torch.randint(0, 2_000, (n,), dtype=torch.int32, generator=g)
    # Start one full length after align so every overlapped window id is
    # non-negative.
    ts = align_ms + len_ms + torch.randint(
        0, 200_000, (n,), dtype=torch.int64, generator=g
    )
    ref = Counter()
    for k, t in zip(keys.tolist(), ts.tolist()):
        hi = (t - align_ms) // off_ms
        lo = (t - align_ms - len_ms) // off_ms + 1
        for wn in range(lo, hi + 1):
            ref[(k, wn)] += 1
    state = WindowAggState(
        torch.device("cuda:0"), align_ms, len_ms, AGG_COUNT,
        slots_pow=18, radix=True, region_bits=11, max_batch=n,
        off_ms=off_ms,
    )
    state.insert(RecordBatch(keys.cuda(), ts.cuda()))
    got = _rows_to_counter(state.close_all(), state)
    assert int(state.error_flag.item()) == 0
    assert got == ref
