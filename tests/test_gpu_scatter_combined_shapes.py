"""Write-combined staged scatter (``BYTEWAX_SCATTER=staged2``) at the
shapes where its LDS staging can go wrong.

The kernel stages a tile's granted entries per segment in LDS and
copies them out in 16-byte pieces; what is left (< 8 per segment) rides
along as residual and leaves through the sentinel-padded final flush.
The cases pin: sizes around one granule and one tile, a whole tile in
one segment, a tile in which nothing is granted, the bench geometry
(512 segments) over several tiles, one- and two-segment tables,
granules beyond the segment capacity (spill), the fallback where the
LDS does not fit, the timestamp forms, both buffer parities of the
pipelined insert, and the modes that must keep the plain kernel.
Every case runs under ``staged2`` and under the default, and compares
exactly against a plain-Python ``Counter``.
"""

from collections import Counter
from datetime import datetime, timezone

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

ALIGN = datetime(2024, 1, 1, tzinfo=timezone.utc)
LEN_MS = 60_000
T = 8192  # events per tile: 512 threads x 16
SEG_BITS = 13  # region_bits 11 + two coarse bits
M64 = (1 << 64) - 1

VARIANTS = ["staged2", "default"]


def _skip_no_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _select(monkeypatch, variant):
    if variant == "default":
        monkeypatch.delenv("BYTEWAX_SCATTER", raising=False)
    else:
        monkeypatch.setenv("BYTEWAX_SCATTER", variant)
    for knob in ("BYTEWAX_SCATTER_U", "BYTEWAX_SCATTER_THREADS",
                 "BYTEWAX_SCATTER_BLOCKS", "BYTEWAX_SCATTER_COARSE_BITS"):
        monkeypatch.delenv(knob, raising=False)


def _align_ms():
    from bytewax_amd.gpu import _ms

    return _ms(ALIGN)


def _mix64(x):
    x ^= x >> 33
    x = (x * 0xFF51AFD7ED558CCD) & M64
    x ^= x >> 33
    x = (x * 0xC4CEB9FE1A85EC53) & M64
    x ^= x >> 33
    return x


def _segment(key, win, slots_pow):
    packed = ((win & 0xFFFFFFFF) << 32) | (key & 0xFFFFFFFF)
    return (_mix64(packed) & ((1 << slots_pow) - 1)) >> SEG_BITS


def _ref(keys, ts, align_ms, len_ms, vals=None):
    c = Counter()
    if vals is None:
        for k, t in zip(keys.tolist(), ts.tolist()):
            c[(k, (t - align_ms) // len_ms)] += 1
    else:
        for k, t, v in zip(keys.tolist(), ts.tolist(), vals.tolist()):
            c[(k, (t - align_ms) // len_ms)] += v
    return c


def _rows(batch, state):
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


def _uniform(n, seed, n_keys=20_000, span_ms=300_000):
    g = torch.Generator().manual_seed(seed)
    align_ms = _align_ms()
    keys = torch.randint(0, n_keys, (n,), dtype=torch.int32, generator=g)
    ts = align_ms + torch.randint(
        0, span_ms, (n,), dtype=torch.int64, generator=g
    )
    return align_ms, keys, ts


def _state(align_ms, slots_pow, max_batch, **kw):
    from bytewax_amd.gpu import AGG_COUNT, WindowAggState

    kw.setdefault("mode", AGG_COUNT)
    return WindowAggState(
        torch.device("cuda:0"), align_ms, kw.pop("len_ms", LEN_MS),
        slots_pow=slots_pow, radix=True, region_bits=11,
        max_batch=max_batch, **kw,
    )


def _insert_and_check(state, keys, ts, ref, ts_base=0):
    from bytewax_amd.gpu import RecordBatch

    state.insert(RecordBatch(keys.cuda(), ts.cuda(), None, ts_base=ts_base))
    got = _rows(state.close_all(), state)
    assert int(state.error_flag.item()) == 0
    assert got == ref


# The references depend on the case only, not on the variant.
_REFS = {}


def _cached(name, build):
    if name not in _REFS:
        _REFS[name] = build()
    return _REFS[name]


@pytest.mark.parametrize("variant", VARIANTS + ["staged"])
@pytest.mark.parametrize(
    "n", [1, 7, 8, 9, 63, 65, T - 1, T, T + 1, 2 * T + 5]
)
def test_sizes_around_granule_and_tile(n, variant, monkeypatch):
    _skip_no_gpu()
    _select(monkeypatch, variant)

    def build():
        align_ms, keys, ts = _uniform(n, 1_000 + n)
        return align_ms, keys, ts, _ref(keys, ts, align_ms, LEN_MS)

    align_ms, keys, ts, ref = _cached(("sizes", n), build)
    state = _state(align_ms, 18, n)
    _insert_and_check(state, keys, ts, ref)
    assert int(state.max_ts_dev.item()) == int(ts.max())


@pytest.mark.parametrize("variant", VARIANTS)
def test_one_hot_cell_three_tiles(variant, monkeypatch):
    """One (key, window) cell: every tile lands in one segment whole and
    its residual carries into the next tile."""
    _skip_no_gpu()
    _select(monkeypatch, variant)
    n = 3 * T + 3
    align_ms = _align_ms()
    keys = torch.full((n,), 4_242, dtype=torch.int32)
    ts = torch.full((n,), align_ms + 1_234, dtype=torch.int64)
    # Capacity for the whole run in one segment: no spill here.
    state = _state(align_ms, 18, 32 * n)
    _insert_and_check(state, keys, ts, Counter({(4_242, 0): n}))
    assert int(state.rx_ov_cursor.item()) == 0


@pytest.mark.parametrize("variant", VARIANTS)
def test_nothing_granted(variant, monkeypatch):
    """Five events in each of the 512 segments: no segment reaches a
    granule, everything leaves through the padded final flush."""
    _skip_no_gpu()
    _select(monkeypatch, variant)
    slots_pow = 22
    nseg = (1 << slots_pow) >> SEG_BITS

    def build():
        per = [0] * nseg
        picked = []
        key = 0
        while len(picked) < 5 * nseg:
            s = _segment(key, 0, slots_pow)
            if per[s] < 5:
                per[s] += 1
                picked.append(key)
            key += 1
        return torch.tensor(picked, dtype=torch.int32)

    keys = _cached("nothing_granted", build)
    n = keys.numel()
    assert n == 5 * nseg < T
    align_ms = _align_ms()
    ts = torch.full((n,), align_ms + 1_234, dtype=torch.int64)
    state = _state(align_ms, slots_pow, n)
    from bytewax_amd.gpu import RecordBatch

    state.insert(RecordBatch(keys.cuda(), ts.cuda()))
    cursors = state.rx_gcursors[:nseg].cpu()
    assert cursors.tolist() == [8] * nseg, "one padded granule per segment"
    got = _rows(state.close_all(), state)
    assert int(state.error_flag.item()) == 0
    assert got == Counter({(k, 0): 1 for k in keys.tolist()})


@pytest.mark.parametrize("variant", VARIANTS)
def test_bench_geometry_three_tiles(variant, monkeypatch):
    """2^22 slots (512 segments), uniform keys, three tiles: each tile
    mixes granted granules with residual in nearly every segment."""
    _skip_no_gpu()
    _select(monkeypatch, variant)
    n = 3 * T

    def build():
        align_ms, keys, ts = _uniform(n, 31, n_keys=1_000_000, span_ms=5_000)
        return align_ms, keys, ts, _ref(keys, ts, align_ms, LEN_MS)

    align_ms, keys, ts, ref = _cached("bench_geometry", build)
    _insert_and_check(_state(align_ms, 22, n), keys, ts, ref)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("slots_pow", [13, 14])
def test_one_and_two_segment_tables(slots_pow, variant, monkeypatch):
    _skip_no_gpu()
    _select(monkeypatch, variant)
    n = T + 77

    def build():
        align_ms, keys, ts = _uniform(n, 50 + slots_pow, n_keys=1_500)
        return align_ms, keys, ts, _ref(keys, ts, align_ms, 300_000)

    align_ms, keys, ts, ref = _cached(("small_table", slots_pow), build)
    state = _state(align_ms, slots_pow, n, len_ms=300_000)
    assert (1 << slots_pow) >> SEG_BITS == slots_pow - 12
    _insert_and_check(state, keys, ts, ref)


@pytest.mark.parametrize("variant", VARIANTS)
def test_hot_key_beyond_capacity_spills(variant, monkeypatch):
    """One hot key on top of uniform traffic: its segment outgrows its
    capacity, so whole granules take the spill path."""
    _skip_no_gpu()
    _select(monkeypatch, variant)
    n = 50_000

    def build():
        align_ms, keys, ts = _uniform(n, 61)
        keys = keys.clone()
        keys[::2] = 12_345
        ts = ts.clone()
        ts[::2] = align_ms + 1_234
        return align_ms, keys, ts, _ref(keys, ts, align_ms, LEN_MS)

    align_ms, keys, ts, ref = _cached("spill", build)
    state = _state(align_ms, 18, n)
    from bytewax_amd.gpu import RecordBatch

    state.insert(RecordBatch(keys.cuda(), ts.cuda()))
    assert int(state.rx_ov_cursor.item()) > 0
    got = _rows(state.close_all(), state)
    assert int(state.error_flag.item()) == 0
    assert got == ref


@pytest.mark.parametrize("variant", VARIANTS)
def test_table_too_large_for_lds_falls_back(variant, monkeypatch):
    """2^24 slots make 2048 segments: the staging does not fit a CU and
    the insert falls back to the plain staged kernel."""
    _skip_no_gpu()
    _select(monkeypatch, variant)
    n = T + 5

    def build():
        align_ms, keys, ts = _uniform(n, 71)
        return align_ms, keys, ts, _ref(keys, ts, align_ms, LEN_MS)

    align_ms, keys, ts, ref = _cached("fallback", build)
    _insert_and_check(_state(align_ms, 24, n), keys, ts, ref)


@pytest.mark.parametrize("variant", VARIANTS)
def test_int32_timestamps_single_base(variant, monkeypatch):
    _skip_no_gpu()
    _select(monkeypatch, variant)
    n = 2 * T + 5

    def build():
        align_ms, keys, ts = _uniform(n, 81)
        return align_ms, keys, ts, _ref(keys, ts, align_ms, LEN_MS)

    align_ms, keys, ts, ref = _cached("ts32", build)
    base = align_ms + 150_000
    ts32 = (ts - base).to(torch.int32)
    assert int(ts32.min()) < 0 < int(ts32.max())
    _insert_and_check(_state(align_ms, 18, n), keys, ts32, ref, ts_base=base)


@pytest.mark.parametrize("variant", VARIANTS)
def test_seg32_several_bases(variant, monkeypatch):
    """One call, three int32 segments with their own bases (one of them
    above most of its timestamps, one odd length so the next segment's
    pointers start only 4-byte aligned)."""
    _skip_no_gpu()
    _select(monkeypatch, variant)
    from bytewax_amd.gpu import _LazyTsBatch

    n = 2 * T + 5

    def build():
        align_ms, keys, ts = _uniform(n, 91)
        return align_ms, keys, ts, _ref(keys, ts, align_ms, LEN_MS)

    align_ms, keys, ts, ref = _cached("seg32", build)
    seg_counts = [T + 1, 333, n - T - 334]
    seg_bases = [align_ms + 250_000, align_ms, align_ms - 1_000_000]
    ts32 = torch.empty(n, dtype=torch.int32)
    off = 0
    for cnt, base in zip(seg_counts, seg_bases):
        ts32[off : off + cnt] = (ts[off : off + cnt] - base).to(torch.int32)
        off += cnt
    lz = _LazyTsBatch(
        keys.cuda(), ts32.cuda(), seg_counts, seg_bases, None, int(ts.max())
    )
    state = _state(align_ms, 18, n)
    state.insert_lazy(lz)
    assert int(state.max_ts_dev.item()) == int(ts.max())
    got = _rows(state.close_all(), state)
    assert int(state.error_flag.item()) == 0
    assert got == ref


@pytest.mark.parametrize("variant", VARIANTS)
def test_pipelined_both_parities(variant, monkeypatch):
    """Four batches through insert_pipelined (radix_scatter_only +
    radix_agg_only), each buffer parity used twice, shrinking sizes."""
    _skip_no_gpu()
    _select(monkeypatch, variant)
    align_ms = _align_ms()
    len_ms, step_ms = 1_000, 5_000
    sizes = [T + 9, T, 9, 1]

    def build():
        g = torch.Generator().manual_seed(7)
        batches, ref = [], Counter()
        for i, n in enumerate(sizes):
            keys = torch.randint(0, 3_000, (n,), dtype=torch.int32,
                                 generator=g)
            ts = torch.randint(0, step_ms, (n,), dtype=torch.int64,
                               generator=g)
            base = align_ms + i * step_ms
            ref.update(_ref(keys, ts + base, align_ms, len_ms))
            batches.append((keys, ts, base))
        return batches, ref

    batches, ref = _cached("pipelined", build)
    state = _state(align_ms, 18, max(sizes), len_ms=len_ms)
    for keys, ts, base in batches:
        state.insert_pipelined(
            keys.cuda(), ts.cuda(), None, base, [], [], base + step_ms - 1
        )
    got = _rows(state.close_all(), state)
    assert int(state.error_flag.item()) == 0
    assert got == ref


def test_sliding_keeps_plain_kernel(monkeypatch):
    _skip_no_gpu()
    _select(monkeypatch, "staged2")
    g = torch.Generator().manual_seed(13)
    n = T + 100
    align_ms = _align_ms()
    len_ms, off_ms = 60_000, 20_000
    keys = torch.randint(0, 2_000, (n,), dtype=torch.int32, generator=g)
    ts = align_ms + len_ms + torch.randint(
        0, 200_000, (n,), dtype=torch.int64, generator=g
    )
    ref = Counter()
    for k, t in zip(keys.tolist(), ts.tolist()):
        hi = (t - align_ms) // off_ms
        lo = (t - align_ms - len_ms) // off_ms + 1
        for wn in range(lo, hi + 1):
            ref[(k, wn)] += 1
    state = _state(align_ms, 18, n, len_ms=len_ms, off_ms=off_ms)
    _insert_and_check(state, keys, ts, ref)


def test_sum_keeps_plain_kernel(monkeypatch):
    _skip_no_gpu()
    _select(monkeypatch, "staged2")
    from bytewax_amd.gpu import AGG_SUM, RecordBatch

    n = T + 100
    align_ms, keys, ts = _uniform(n, 17)
    g = torch.Generator().manual_seed(18)
    vals = torch.randint(0, 100, (n,), dtype=torch.int64, generator=g)
    ref = _ref(keys, ts, align_ms, LEN_MS, vals)
    state = _state(align_ms, 18, n, mode=AGG_SUM)
    state.insert(RecordBatch(keys.cuda(), ts.cuda(), vals.cuda()))
    got = _rows(state.close_all(), state)
    assert int(state.error_flag.item()) == 0
    assert got == ref


def test_late_tracking_keeps_plain_kernel(monkeypatch):
    """Second batch holds events below the watermark of the first: they
    come back from take_late() and join no window."""
    _skip_no_gpu()
    _select(monkeypatch, "staged2")
    from bytewax_amd.gpu import RecordBatch

    n = T + 100
    align_ms, keys, ts = _uniform(n, 19, span_ms=100_000)
    ts1 = ts + 100_000  # [100 s, 200 s)
    wm = int(ts1.max())
    _a, keys2, ts2 = _uniform(n, 20, span_ms=200_000)
    ts2 = ts2 + 50_000  # [50 s, 250 s): part of it below the watermark
    late = ts2 < wm
    assert 0 < int(late.sum()) < n
    ref = _ref(keys, ts1, align_ms, LEN_MS)
    ref.update(_ref(keys2[~late], ts2[~late], align_ms, LEN_MS))
    state = _state(align_ms, 18, n, track_late=True, wait_ms=0)
    state.insert(RecordBatch(keys.cuda(), ts1.cuda(), None, max_ts=wm))
    state.insert(
        RecordBatch(keys2.cuda(), ts2.cuda(), None, max_ts=int(ts2.max()))
    )
    rb = state.take_late()
    got_late = Counter(zip(rb.keys.cpu().tolist(), rb.ts.cpu().tolist()))
    assert got_late == Counter(
        zip(keys2[late].tolist(), ts2[late].tolist())
    )
    got = _rows(state.close_all(), state)
    assert int(state.error_flag.item()) == 0
    assert got == ref
