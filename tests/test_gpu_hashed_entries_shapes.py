"""Hashed scatter entries, at the shapes where they can go wrong.

For batches of int32 timestamp deltas the write-combined COUNT scatter
hands the aggregation entries of the form ``key | window delta (19 bits)
| LDS slot (13 bits)``, the delta taken against a per-call entry base;
what does not fit goes to the overflow spill as a classic ``window |
key`` word.  These cases pin: both sides of 2,000 consecutive window
edges for four lengths and two kinds of base, deltas beyond the 19-bit
range, segmented batches with several bases under one entry base, a
length of 2^31 ms or more (classic entries), every pairing of scatter
and aggregation kernel, the per-parity entry base of the pipelined path,
and segments whose first entry stands alone or that hold only pads.

Expected rows come from a numpy group-by.  ``seg_bits`` (``region_bits``
+ 2) is 8, 12 or 13, which covers both thread-block sizes of the
aggregation.
"""

from datetime import datetime, timezone

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

ALIGN = datetime(2024, 1, 1, tzinfo=timezone.utc)
CLASSIC = -(1 << 63)  # what radix_scatter_only returns for classic entries
KNOBS = ("BYTEWAX_AGG", "BYTEWAX_SCATTER", "BYTEWAX_ENTRIES",
         "BYTEWAX_SCATTER_THREADS", "BYTEWAX_SCATTER_U")
# (slots_pow, region_bits): seg_bits 13, 12 and 8.
SHAPES = {13: (16, 11), 12: (16, 10), 8: (14, 6)}


def _skip_no_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _align_ms():
    from bytewax_amd.gpu import _ms

    return _ms(ALIGN)


def _clear_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _ref(keys, abs_ts, len_ms):
    """{(key, window): count} by a numpy group-by (events at or after
    the alignment only, where floor and truncation agree)."""
    keys = np.asarray(keys, dtype=np.int64)
    x = np.asarray(abs_ts, dtype=np.int64) - _align_ms()
    assert (x >= 0).all()
    pairs = np.stack([keys, x // len_ms], axis=1)
    uniq, counts = np.unique(pairs, axis=0, return_counts=True)
    return {(int(k), int(w)): int(c) for (k, w), c in zip(uniq, counts)}


def _rows(batch, state):
    if batch is None:
        return {}
    keys = batch.keys.cpu().tolist()
    wins = ((batch.ts.cpu() - state.align_ms) // state.off_ms).tolist()
    vals = batch.vals.cpu().tolist()
    got = {}
    for k, w, v in zip(keys, wins, vals):
        assert (k, w) not in got, "cell emitted twice"
        got[(k, w)] = v
    return got


def _state(len_ms, seg_bits, max_batch):
    from bytewax_amd.gpu import AGG_COUNT, WindowAggState

    slots_pow, region_bits = SHAPES[seg_bits]
    return WindowAggState(
        torch.device("cuda:0"), _align_ms(), len_ms, AGG_COUNT,
        slots_pow=slots_pow, radix=True, region_bits=region_bits,
        max_batch=max_batch,
    )


def _split_insert(state, keys, ts, base, seg_counts=(), seg_bases=()):
    """One insert through the split calls; returns what the scatter said
    about its entries."""
    par = getattr(state, "_pipe_parity", 0)
    state.insert_pipelined(
        keys.cuda(), ts.cuda(), None, base, list(seg_counts),
        list(seg_bases), None,
    )
    return state._ev_w[par]


def _edge_events(len_ms, first_k, n_keys):
    """Absolute offsets from the alignment on both sides of 2,000
    consecutive window edges."""
    k = np.arange(first_k, first_k + 2_000, dtype=np.int64)
    x = np.concatenate([k * len_ms - 1, k * len_ms])
    x = x[x >= 0]
    keys = (np.arange(x.size) % n_keys * 7_919 + 3).astype(np.int32)
    return keys, x


@pytest.mark.parametrize("base_kind", ["middle", "near_align"])
@pytest.mark.parametrize(
    "len_ms,seg_bits", [(60_000, 13), (4_096, 12), (1_000, 8), (7, 13)]
)
def test_window_edges(len_ms, seg_bits, base_kind, monkeypatch):
    """k*len - 1 and k*len for 2,000 consecutive k, as int32 deltas on
    both sides of a base in the middle of them, and from a base three
    milliseconds after the alignment (first window 0)."""
    _skip_no_gpu()
    _clear_knobs(monkeypatch)
    from bytewax_amd.gpu import RecordBatch

    n_keys = 1 if seg_bits == 8 else 5
    if base_kind == "middle":
        keys, x = _edge_events(len_ms, 5_000, n_keys)
        base = _align_ms() + 6_000 * len_ms + 1
    else:
        keys, x = _edge_events(len_ms, 0, n_keys)
        base = _align_ms() + 3
    abs_ts = x + _align_ms()
    d = abs_ts - base
    assert d.min() < 0 < d.max()
    ts32 = torch.from_numpy(d.astype(np.int32))
    tkeys = torch.from_numpy(keys)
    ref = _ref(keys, abs_ts, len_ms)
    # Fused call.
    state = _state(len_ms, seg_bits, len(keys))
    state.insert(RecordBatch(tkeys.cuda(), ts32.cuda(), ts_base=int(base)))
    assert _rows(state.close_all(), state) == ref
    assert int(state.error_flag.item()) == 0
    assert int(state.max_ts_dev.item()) == int(abs_ts.max())
    # Split calls, which also say that the entries were hashed.
    state = _state(len_ms, seg_bits, len(keys))
    w = _split_insert(state, tkeys, ts32, int(base))
    assert w != CLASSIC
    assert _rows(state.close_all(), state) == ref
    assert int(state.error_flag.item()) == 0


def test_delta_overflow_spills(monkeypatch):
    """len 7 ms, deltas over more than 2^19 windows on each side of the
    base: what does not fit the entry delta is spilled and counted."""
    _skip_no_gpu()
    _clear_knobs(monkeypatch)
    g = np.random.default_rng(11)
    n, len_ms = 6_000, 7
    span = 7 * (1 << 20)
    base = _align_ms() + 2 * span
    d = g.integers(-span, span, n)
    d[:4] = [-span, span - 1, -7 * (1 << 18), 7 * (1 << 18)]
    keys = g.integers(0, 50, n).astype(np.int32)
    ref = _ref(keys, d + base, len_ms)
    state = _state(len_ms, 13, n)
    w = _split_insert(
        state, torch.from_numpy(keys), torch.from_numpy(d.astype(np.int32)),
        int(base),
    )
    assert w != CLASSIC
    spilled = int(state.rx_ov_cursor.item())
    assert 0 < spilled < n
    assert _rows(state.close_all(), state) == ref
    assert int(state.error_flag.item()) == 0


@pytest.mark.parametrize("fused", [True, False])
def test_seg32_several_bases(fused, monkeypatch):
    """Wire-format segments: an empty one first, three whose bases lie
    20 windows apart, one more than 2^19 windows away; one entry base
    (from the second segment) serves them all."""
    _skip_no_gpu()
    _clear_knobs(monkeypatch)
    from bytewax_amd.gpu import _LazyTsBatch

    g = np.random.default_rng(21)
    len_ms = 1_000
    b0 = _align_ms() + 50_000 * len_ms + 17
    bases = [b0 - 999, b0, b0 + 20 * len_ms, b0 + 40 * len_ms,
             b0 + 600_000 * len_ms]
    counts = [0, 2_001, 1_500, 9, 700]
    n = sum(counts)
    d = g.integers(-3_000, 3_000, n)
    keys = g.integers(0, 300, n).astype(np.int32)
    abs_ts = d + np.repeat(np.array(bases, dtype=np.int64), counts)
    ref = _ref(keys, abs_ts, len_ms)
    tkeys = torch.from_numpy(keys)
    ts32 = torch.from_numpy(d.astype(np.int32))
    state = _state(len_ms, 13, n)
    if fused:
        state.insert_lazy(
            _LazyTsBatch(tkeys.cuda(), ts32.cuda(), counts, bases, None, None)
        )
    else:
        w = _split_insert(state, tkeys, ts32, 0, counts, bases)
        assert w != CLASSIC
    # The far segment does not fit the entry delta.
    assert int(state.rx_ov_cursor.item()) >= counts[-1]
    assert _rows(state.close_all(), state) == ref
    assert int(state.error_flag.item()) == 0
    assert int(state.max_ts_dev.item()) == int(abs_ts.max())


@pytest.mark.parametrize("len_ms", [1 << 31, (1 << 31) + 12_345])
def test_length_without_a_32_bit_path(len_ms, monkeypatch):
    """A window length of 2^31 ms or more: classic entries, same rows."""
    _skip_no_gpu()
    _clear_knobs(monkeypatch)
    g = np.random.default_rng(31)
    n = 5_000
    base = _align_ms() + 3 * len_ms
    d = g.integers(-(1 << 31), 1 << 31, n)
    d[:2] = [-(1 << 31), (1 << 31) - 1]
    keys = g.integers(0, 400, n).astype(np.int32)
    ref = _ref(keys, d + base, len_ms)
    state = _state(len_ms, 13, n)
    w = _split_insert(
        state, torch.from_numpy(keys), torch.from_numpy(d.astype(np.int32)),
        int(base),
    )
    assert w == CLASSIC
    assert _rows(state.close_all(), state) == ref
    assert int(state.error_flag.item()) == 0


def test_full_int32_delta_domain(monkeypatch):
    """Deltas at both ends of int32 and around zero, one-minute
    windows: about 71,000 windows apart, all inside the entry delta."""
    _skip_no_gpu()
    _clear_knobs(monkeypatch)
    len_ms = 60_000
    base = _align_ms() + (1 << 32) + 59_999
    top = (1 << 31) - 1
    d = np.concatenate([
        np.arange(-(1 << 31), -(1 << 31) + 1_500),
        np.arange(top - 1_500, top + 1),
        np.arange(-700, 700),
    ])
    keys = (np.arange(d.size) % 7).astype(np.int32)
    ref = _ref(keys, d + base, len_ms)
    state = _state(len_ms, 13, d.size)
    w = _split_insert(
        state, torch.from_numpy(keys), torch.from_numpy(d.astype(np.int32)),
        int(base),
    )
    assert w != CLASSIC
    assert _rows(state.close_all(), state) == ref
    assert int(state.error_flag.item()) == 0


@pytest.mark.parametrize("seg_bits", [8, 12, 13])
def test_pairing(seg_bits, monkeypatch):
    """Every scatter / aggregation pairing closes the same rows as the
    default on the same input."""
    _skip_no_gpu()
    from bytewax_amd.gpu import RecordBatch

    g = np.random.default_rng(41 + seg_bits)
    n, len_ms = 9_001, 1_000
    base = _align_ms() + 777_777
    d = g.integers(-20_000, 20_000, n)
    keys = g.integers(0, 40 if seg_bits == 8 else 2_000, n).astype(np.int32)
    ref = _ref(keys, d + base, len_ms)
    tkeys = torch.from_numpy(keys).cuda()
    ts32 = torch.from_numpy(d.astype(np.int32)).cuda()
    ts64 = torch.from_numpy(d + base).cuda()

    def run(env, int64_ts=False):
        _clear_knobs(monkeypatch)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        state = _state(len_ms, seg_bits, n)
        if int64_ts:
            state.insert(RecordBatch(tkeys, ts64))
        else:
            state.insert(RecordBatch(tkeys, ts32, ts_base=int(base)))
        got = _rows(state.close_all(), state)
        assert int(state.error_flag.item()) == 0, env
        return got

    default = run({})
    assert default == ref
    assert run({"BYTEWAX_AGG": "wide"}) == default
    assert run({"BYTEWAX_SCATTER": "staged"}) == default
    assert run({"BYTEWAX_ENTRIES": "classic"}) == default
    assert run({}, int64_ts=True) == default


def test_pairing_reports_the_format(monkeypatch):
    """The split scatter says "classic" under every knob that rules the
    hashed format out, and for int64 timestamps."""
    _skip_no_gpu()
    n, len_ms = 500, 1_000
    base = _align_ms() + 10_000
    keys = torch.arange(n, dtype=torch.int32)
    ts32 = torch.arange(n, dtype=torch.int32)
    for env, ts, want_classic in [
        ({}, ts32, False),
        ({"BYTEWAX_AGG": "wide"}, ts32, True),
        ({"BYTEWAX_SCATTER": "staged"}, ts32, True),
        ({"BYTEWAX_ENTRIES": "classic"}, ts32, True),
        ({}, ts32.to(torch.int64) + base, True),
    ]:
        _clear_knobs(monkeypatch)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        state = _state(len_ms, 13, n)
        b = 0 if ts.dtype == torch.int64 else int(base)
        w = _split_insert(state, keys, ts, b)
        assert (w == CLASSIC) == want_classic, env
        got = _rows(state.close_all(), state)
        assert sum(got.values()) == n and len(got) == n
        assert int(state.error_flag.item()) == 0


def test_pipelined_parities(monkeypatch):
    """Four batches through insert_pipelined, a different base and so a
    different entry base each, a watermark close in between; each buffer
    parity is used twice."""
    _skip_no_gpu()
    _clear_knobs(monkeypatch)
    g = np.random.default_rng(51)
    len_ms, step_ms = 1_000, 5_000
    sizes = [20_001, 9, 8_192, 3_000]
    state = _state(len_ms, 13, max(sizes))
    ref, got, seen_w = {}, {}, []
    for i, n in enumerate(sizes):
        base = _align_ms() + 1_000_000 + i * step_ms
        d = g.integers(0, step_ms, n)
        keys = g.integers(0, 3_000, n).astype(np.int32)
        for cell, c in _ref(keys, d + base, len_ms).items():
            ref[cell] = ref.get(cell, 0) + c
        par = state._pipe_parity if hasattr(state, "_pipe_parity") else 0
        assert par == i % 2
        state.insert_pipelined(
            torch.from_numpy(keys).cuda(),
            torch.from_numpy(d.astype(np.int32)).cuda(), None, int(base),
            [], [], int(base + step_ms - 1),
        )
        seen_w.append(state._ev_w[par])
        if i == 1:
            closed = _rows(state.close_due(), state)
            assert len(closed) > 0
            got.update(closed)
    assert CLASSIC not in seen_w and len(set(seen_w)) == 4
    tail = _rows(state.close_all(), state)
    assert not (set(tail) & set(got)), "cell closed twice"
    got.update(tail)
    assert got == ref
    assert int(state.error_flag.item()) == 0


def test_first_entry_alone_in_its_window(monkeypatch):
    """One key, so one segment; its first entry is the only event of a
    window 100 windows ahead of all others: the cell base comes from it
    and every other entry is rebuilt and takes the direct path."""
    _skip_no_gpu()
    _clear_knobs(monkeypatch)
    from bytewax_amd.gpu import RecordBatch

    n, len_ms = 4_000, 1_000
    base = _align_ms() + 3_000_000
    d = np.arange(n) % 3_000  # three windows
    d[0] = 100 * len_ms + 5
    keys = np.full(n, 77, dtype=np.int32)
    ref = _ref(keys, d + base, len_ms)
    assert ref[(77, 3_100)] == 1
    state = _state(len_ms, 13, n)
    state.insert(RecordBatch(
        torch.from_numpy(keys).cuda(),
        torch.from_numpy(d.astype(np.int32)).cuda(), ts_base=int(base),
    ))
    assert _rows(state.close_all(), state) == ref
    assert int(state.error_flag.item()) == 0


@pytest.mark.parametrize("seg_bits", [8, 13])
def test_segment_of_only_pads(seg_bits, monkeypatch):
    """The aggregation alone over segments that hold nothing but pads,
    told that the entries are hashed: no rows, no error."""
    _skip_no_gpu()
    _clear_knobs(monkeypatch)
    state = _state(1_000, seg_bits, 4_096)
    state.rx_packed.fill_(-1)
    state.rx_gcursors.zero_()
    state.rx_gcursors[:3] = torch.tensor([8, 16, 24], dtype=torch.int32)
    state.rx_ov_cursor.zero_()
    state.k.radix_agg_only(
        state.tkeys, state.tvals, state.error_flag, state.rx_gcursors,
        state.rx_packed, state.rx_vals, state.rx_ov_cursor,
        state.rx_ov_packed, state.rx_ov_vals, state.mode, state.region_bits,
        123_456,
    )
    assert _rows(state.close_all(), state) == {}
    assert int(state.error_flag.item()) == 0
    assert int((state.tkeys != -1).sum().item()) == 0
