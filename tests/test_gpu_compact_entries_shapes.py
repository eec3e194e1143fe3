"""Compact (4-byte) scatter entries, at the shapes where they can go wrong.

With at least 128 segments the write-combined COUNT scatter hands the
aggregation 4-byte entries: the low 31 bits of an invertible hash of
``key32 | window delta << 32``, whose top bits are the segment index.
The delta has D = log2(segments) - 1 bits against an entry base that lies
2^(D-1) windows before the window of the call's first ``ts_base``; what
does not fit goes to the overflow spill as a classic ``window | key``
word.  Expected rows come from a numpy group-by, entry buffers are
decoded with the numpy twin of the mixer.

Shapes (slots_pow, region_bits): 128 segments of 2^13 slots, 512 of
2^13 (the benchmark's), 128 of 2^8.
"""

from datetime import datetime, timezone

import numpy as np
import pytest
from test_compact_entries_twin import decode, encode

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

ALIGN = datetime(2024, 1, 1, tzinfo=timezone.utc)
CLASSIC = -(1 << 63)
FMT_CLASSIC, FMT_HASHED, FMT_COMPACT = 0, 1, 2
KNOBS = ("BYTEWAX_AGG", "BYTEWAX_SCATTER", "BYTEWAX_ENTRIES",
         "BYTEWAX_SCATTER_THREADS", "BYTEWAX_SCATTER_U",
         "BYTEWAX_SCATTER_BLOCKS", "BYTEWAX_AGG_R")
# name -> (slots_pow, region_bits, segments, D, seg_bits)
SHAPES = {
    "s128": (20, 11, 128, 6, 13),
    "s512": (22, 11, 512, 8, 13),
    "s128x8": (15, 6, 128, 6, 8),
}
EXTREME = [0, -1, -(1 << 31), (1 << 31) - 1]
LEN = 60_000


def _prep(monkeypatch, **env):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _align_ms():
    from bytewax_amd.gpu import _ms

    return _ms(ALIGN)


def _ref(keys, abs_ts, len_ms):
    keys = np.asarray(keys, dtype=np.int64)
    x = np.asarray(abs_ts, dtype=np.int64) - _align_ms()
    assert (x >= 0).all()
    if keys.size == 0:
        return {}
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


def _state(shape, max_batch, len_ms=LEN):
    from bytewax_amd.gpu import AGG_COUNT, WindowAggState

    slots_pow, region_bits = SHAPES[shape][:2]
    return WindowAggState(
        torch.device("cuda:0"), _align_ms(), len_ms, AGG_COUNT,
        slots_pow=slots_pow, radix=True, region_bits=region_bits,
        max_batch=max(max_batch, 1),
    )


def _bufs(st):
    return (st.rx_gcursors, st.rx_packed, st.rx_vals, st.rx_ov_cursor,
            st.rx_ov_packed, st.rx_ov_vals)


def _scatter(st, keys, d, base, compact=True):
    args = (
        torch.from_numpy(np.asarray(keys, dtype=np.int32)).cuda(),
        torch.from_numpy(np.asarray(d).astype(np.int32)).cuda(), None,
        st.max_ts_dev, st.error_flag, *_bufs(st), st.nslots, st.align_ms,
        st.len_ms, st.mode, int(base), st.region_bits, st.off_ms, [], [],
    )
    out = st.k.radix_scatter_only(*args, True) if compact else (
        st.k.radix_scatter_only(*args))
    torch.cuda.synchronize()
    return out


def _agg(st, w, fmt):
    st.k.radix_agg_only(
        st.tkeys, st.tvals, st.error_flag, *_bufs(st), st.mode,
        st.region_bits, w, fmt,
    )
    torch.cuda.synchronize()


def _cap(st, shape):
    return (st.rx_packed.numel() // SHAPES[shape][2]) & ~15


def _fused(st, keys, d, base):
    from bytewax_amd.gpu import RecordBatch

    st.insert(RecordBatch(
        torch.from_numpy(np.asarray(keys, dtype=np.int32)).cuda(),
        torch.from_numpy(np.asarray(d).astype(np.int32)).cuda(),
        ts_base=int(base),
    ))
    torch.cuda.synchronize()


def _check_closed(st, keys, d, base, len_ms=LEN):
    abs_ts = np.asarray(d, dtype=np.int64) + base
    assert _rows(st.close_all(), st) == _ref(keys, abs_ts, len_ms)
    assert int(st.error_flag.item()) == 0
    if len(abs_ts):
        assert int(st.max_ts_dev.item()) == int(abs_ts.max())


def _base(len_ms=LEN):
    return _align_ms() + 10_000 * len_ms + 17


def _entry_base(base, D, len_ms=LEN):
    return (base - _align_ms()) // len_ms - (1 << (D - 1))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_decode(shape, monkeypatch):
    """Every entry of the buffer, inverted with the numpy twin and its
    segment index, and every spilled word: the multiset is the input."""
    _prep(monkeypatch)
    nseg, D = SHAPES[shape][2:4]
    g = np.random.default_rng(5)
    n = 20_011
    keys = g.integers(-(1 << 31), 1 << 31, n).astype(np.int32)
    keys[:4] = EXTREME
    keys[4:2_000] = g.integers(0, 50, 1_996)
    base = _base()
    # Windows on both sides of the reach.
    d = g.integers(-(1 << D) * LEN, (1 << D) * LEN, n)
    st = _state(shape, n)
    w, fmt = _scatter(st, keys, d, base)
    assert fmt == FMT_COMPACT and w == _entry_base(base, D)
    cap = _cap(st, shape)
    cur = st.rx_gcursors[:nseg].cpu().numpy()
    assert (cur % 16 == 0).all() and (cur <= cap).all()
    ev = st.rx_packed.view(torch.int32).cpu().numpy().view(np.uint32)
    segs, ents = [], []
    for b in range(nseg):
        e = ev[b * cap:b * cap + cur[b]]
        e = e[e != 0xFFFFFFFF]
        assert (e >> 31 == 0).all()
        ents.append(e)
        segs.append(np.full(e.size, b))
    k2, d2 = decode(np.concatenate(segs), np.concatenate(ents), 32 + D)
    assert d2.min() >= 0 and d2.max() < (1 << D)
    got = [(int(a), int(w + b)) for a, b in zip(k2, d2)]
    nov = int(st.rx_ov_cursor.item())
    ov = st.rx_ov_packed[:nov].cpu().numpy().view(np.uint64)
    win = (d + base - _align_ms()) // LEN
    fits = (win - w >= 0) & (win - w < (1 << D))
    assert nov == int((~fits).sum()) and 0 < nov < n
    ovk = (ov & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
    got += list(zip(ovk.tolist(), (ov >> np.uint64(32)).tolist()))
    want = sorted(zip(keys.tolist(), win.tolist()))
    assert sorted(got) == want
    # What the twin says about segments is what the device did.
    s2, _ = encode(keys[fits], (win - w)[fits], 32 + D)
    assert (np.bincount(s2, minlength=nseg) <= cur).all()
    _agg(st, w, fmt)
    _check_closed(st, keys, d, base)


@pytest.mark.parametrize("one_key", [True, False])
@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 8191, 8192, 8193])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_sizes(shape, n, one_key, monkeypatch):
    """A line never filled, exactly filled, one over (one key and one
    window: one segment), and both sides of the 8192-event tile."""
    _prep(monkeypatch)
    g = np.random.default_rng(n)
    keys = np.full(n, 4_242) if one_key else g.integers(0, 3_000, n)
    d = np.full(n, 5) if one_key else g.integers(0, 3 * LEN, n)
    st = _state(shape, n)
    _fused(st, keys, d, _base())
    if one_key and 0 < n <= 17:
        cur = st.rx_gcursors[:SHAPES[shape][2]].cpu().numpy()
        assert sorted(cur[cur > 0].tolist()) == [16 * -(-n // 16)]
    _check_closed(st, keys, d, _base())


@pytest.mark.parametrize("shape", list(SHAPES))
def test_one_block_walks_several_tiles(shape, monkeypatch):
    """One block, three tiles and five events: residuals are carried
    from tile to tile."""
    _prep(monkeypatch, BYTEWAX_SCATTER_BLOCKS="1")
    g = np.random.default_rng(9)
    n = 3 * 8192 + 5
    keys = g.integers(0, 700, n)
    d = g.integers(0, 2 * LEN, n)
    st = _state(shape, n)
    w, fmt = _scatter(st, keys, d, _base())
    assert fmt == FMT_COMPACT
    _agg(st, w, fmt)
    _check_closed(st, keys, d, _base())


@pytest.mark.parametrize("shape", ["s128", "s512"])
def test_one_key_crosses_cap(shape, monkeypatch):
    """One key and one window: one segment takes everything, fills to
    `cap`, and whole 16-entry granules go to the spill, rebuilt.  One
    block, so that no other block's padded final flush takes room below
    `cap` and the spill count is exact."""
    _prep(monkeypatch, BYTEWAX_SCATTER_BLOCKS="1")
    n = 30_000
    keys = np.full(n, -123_456_789)
    d = np.full(n, 42)
    st = _state(shape, n)
    cap = _cap(st, shape)
    assert 16 <= cap < n
    w, fmt = _scatter(st, keys, d, _base())
    assert fmt == FMT_COMPACT
    assert int(st.rx_ov_cursor.item()) == n - cap
    ov = st.rx_ov_packed[:n - cap].cpu().numpy().view(np.uint64)
    win = (_base() + 42 - _align_ms()) // LEN
    assert (ov == np.uint64((win << 32) | (-123_456_789 & 0xFFFFFFFF))).all()
    _agg(st, w, fmt)
    _check_closed(st, keys, d, _base())


@pytest.mark.parametrize("shape", list(SHAPES))
def test_extreme_keys(shape, monkeypatch):
    _prep(monkeypatch)
    D = SHAPES[shape][3]
    keys = np.repeat(np.array(EXTREME), 40)
    d = (np.arange(keys.size) % (1 << D) - (1 << (D - 1))) * LEN + 3
    st = _state(shape, keys.size)
    _fused(st, keys, d, _base())
    assert int(st.rx_ov_cursor.item()) == 0
    _check_closed(st, keys, d, _base())


@pytest.mark.parametrize("shape", list(SHAPES))
def test_reach_edges(shape, monkeypatch):
    """Deltas 0 and 2^D - 1 from the entry base stay in the buffer,
    -1 and 2^D spill: the exact spill count."""
    _prep(monkeypatch)
    D = SHAPES[shape][3]
    base = _base()
    wb = _entry_base(base, D)
    counts = {wb - 1: 7, wb: 11, wb + (1 << D) - 1: 13, wb + (1 << D): 5}
    wins = np.repeat(np.array(list(counts)), list(counts.values()))
    # Both edges of each window.
    x = wins * LEN + np.where(np.arange(wins.size) % 2 == 0, 0, LEN - 1)
    d = x + _align_ms() - base
    keys = np.arange(wins.size) % 3
    st = _state(shape, wins.size)
    w, fmt = _scatter(st, keys, d, base)
    assert (w, fmt) == (wb, FMT_COMPACT)
    assert int(st.rx_ov_cursor.item()) == 7 + 5
    assert int(st.rx_gcursors.sum().item()) >= 11 + 13
    _agg(st, w, fmt)
    _check_closed(st, keys, d, base)


@pytest.mark.parametrize("len_ms", [60_000, 7])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_window_edges_inside_the_reach(shape, len_ms, monkeypatch):
    """k * len - 1 and k * len for consecutive k inside the reach: 100
    of them where the reach has 256 windows, the 62 that fit where it
    has 64.  Nothing spills."""
    _prep(monkeypatch)
    D = SHAPES[shape][3]
    base = _base(len_ms)
    wb = _entry_base(base, D, len_ms)
    nk = min(100, (1 << D) - 2)
    k = np.arange(wb + 1, wb + 1 + nk, dtype=np.int64)
    x = np.concatenate([k * len_ms - 1, k * len_ms])
    d = x + _align_ms() - base
    keys = np.arange(x.size) % 5 * 7_919 + 3
    st = _state(shape, x.size, len_ms)
    _fused(st, keys, d, base)
    assert int(st.rx_ov_cursor.item()) == 0
    _check_closed(st, keys, d, base, len_ms)


@pytest.mark.parametrize("shape", ["s128", "s128x8"])
def test_segment_of_only_pads(shape, monkeypatch):
    _prep(monkeypatch)
    st = _state(shape, 4_096)
    st.rx_packed.fill_(-1)
    st.rx_gcursors.zero_()
    st.rx_gcursors[:3] = torch.tensor([16, 32, 48], dtype=torch.int32)
    st.rx_ov_cursor.zero_()
    _agg(st, 123_456, FMT_COMPACT)
    assert _rows(st.close_all(), st) == {}
    assert int(st.error_flag.item()) == 0
    assert int((st.tkeys != -1).sum().item()) == 0


@pytest.mark.parametrize("shape", list(SHAPES))
def test_first_entry_alone_in_its_window(shape, monkeypatch):
    """One key, three windows of 400 events and one event alone 20
    windows ahead, first in the batch; room for a cell's 400 entries in
    a segment, so nothing spills."""
    _prep(monkeypatch)
    n = 1_201
    d = np.arange(n) % 3 * LEN + np.arange(n) % 1_000
    d[0] = 20 * LEN + 5
    keys = np.full(n, 77)
    st = _state(shape, 100_000)
    assert _cap(st, shape) >= 400 + 16
    _fused(st, keys, d, _base())
    assert int(st.rx_ov_cursor.item()) == 0
    _check_closed(st, keys, d, _base())


def test_lds_table_full_escape(monkeypatch):
    """More distinct cells in a segment than its 256 LDS slots.  The
    table of this shape has 32,768 slots in regions of 64 and cannot
    hold 60,000 cells, so of 60,000 distinct candidate cells the test
    keeps those that the twin puts into segments 0..7: about 470 cells
    for each of them, 230 past a full LDS table."""
    _prep(monkeypatch)
    shape = "s128x8"
    D = SHAPES[shape][3]
    base = _base()
    wb = _entry_base(base, D)
    ck = np.repeat(np.arange(60_000 // 20), 20)
    cd = np.tile(np.arange(20), 60_000 // 20) + 10
    seg, _ = encode(ck, cd, 32 + D)
    keep = seg < 8
    per_seg = np.bincount(seg[keep], minlength=8)
    assert per_seg.min() > 256 + 100
    keys = np.tile(ck[keep], 3)
    d = (np.tile(cd[keep], 3) + wb) * LEN + _align_ms() - base + 1
    st = _state(shape, 100_000)  # room for 1,400 entries in a segment
    assert _cap(st, shape) > 3 * per_seg.max() + 16
    w, fmt = _scatter(st, keys, d, base)
    assert (w, fmt) == (wb, FMT_COMPACT)
    assert int(st.rx_ov_cursor.item()) == 0
    cur = st.rx_gcursors[:128].cpu().numpy()
    assert (cur[:8] >= 3 * per_seg).all() and (cur[8:] == 0).all()
    _agg(st, w, fmt)
    _check_closed(st, keys, d, base)


@pytest.mark.parametrize("shape", ["s128", "s128x8"])
def test_head_and_tail_peeling(shape, monkeypatch):
    """Segments that hold 1 .. 7 entries, written by hand: vector body
    of 0 or 1 and a tail of 0 .. 3."""
    _prep(monkeypatch)
    nseg, D = SHAPES[shape][2:4]
    st = _state(shape, 4_096)
    cap = _cap(st, shape)
    ck = np.arange(20_000)
    cd = ck % 4
    seg, ent = encode(ck, cd, 32 + D)
    buf = np.full(st.rx_packed.numel() * 2, 0xFFFFFFFF, dtype=np.uint32)
    cur = np.zeros(st.rx_gcursors.numel(), dtype=np.int32)
    wb, want = 9_000, {}
    for b in range(1, 8):
        pick = np.flatnonzero(seg == b)[:b]
        assert pick.size == b
        buf[b * cap:b * cap + b] = ent[pick]
        cur[b] = b
        for i in pick:
            want[(int(ck[i]), wb + int(cd[i]))] = 1
    st.rx_packed.copy_(torch.from_numpy(buf.view(np.int64)).cuda())
    st.rx_gcursors.copy_(torch.from_numpy(cur).cuda())
    st.rx_ov_cursor.zero_()
    _agg(st, wb, FMT_COMPACT)
    assert _rows(st.close_all(), st) == want
    assert int(st.error_flag.item()) == 0


@pytest.mark.parametrize("shape", list(SHAPES))
def test_formats_close_identical_rows(shape, monkeypatch):
    """The same batches under each BYTEWAX_ENTRIES close the same rows,
    and the split calls report the format."""
    D = SHAPES[shape][3]
    g = np.random.default_rng(61)
    n = 9_001
    keys = g.integers(0, 2_000, n)
    d = g.integers(-(1 << D) * LEN, (1 << D) * LEN, n)
    base = _base()
    got = {}
    for env, want_fmt in [({}, FMT_COMPACT),
                          ({"BYTEWAX_ENTRIES": "hashed"}, FMT_HASHED),
                          ({"BYTEWAX_ENTRIES": "classic"}, FMT_CLASSIC)]:
        _prep(monkeypatch, **env)
        st = _state(shape, n)
        w, fmt = _scatter(st, keys, d, base)
        assert fmt == want_fmt
        assert (w == CLASSIC) == (fmt == FMT_CLASSIC)
        _agg(st, w, fmt)
        got[want_fmt] = _rows(st.close_all(), st)
        assert int(st.error_flag.item()) == 0
        # The fused call plans the same way.
        st = _state(shape, n)
        _fused(st, keys, d, base)
        assert _rows(st.close_all(), st) == got[want_fmt]
    assert got[FMT_COMPACT] == _ref(keys, d + base, LEN)
    assert got[FMT_HASHED] == got[FMT_COMPACT] == got[FMT_CLASSIC]


def test_split_call_without_the_format_argument(monkeypatch):
    """A caller that does not ask for compact entries gets a plain entry
    base and hashed entries, and the aggregation needs no format."""
    _prep(monkeypatch)
    n = 5_000
    keys = np.arange(n) % 900
    d = np.arange(n) * 37 % (4 * LEN)
    st = _state("s512", n)
    w = _scatter(st, keys, d, _base(), compact=False)
    assert isinstance(w, int) and w != CLASSIC
    assert w != _entry_base(_base(), 8)  # the hashed base lies 2^18 back
    st.k.radix_agg_only(
        st.tkeys, st.tvals, st.error_flag, *_bufs(st), st.mode,
        st.region_bits, w,
    )
    _check_closed(st, keys, d, _base())


def test_pipelined_parities(monkeypatch):
    """Four batches through insert_pipelined, a different base each, a
    watermark close in between; each parity keeps its own entry base
    and format."""
    _prep(monkeypatch)
    g = np.random.default_rng(51)
    step_ms = 5 * LEN
    sizes = [20_001, 9, 8_192, 3_000]
    st = _state("s512", max(sizes))
    ref, got, seen = {}, {}, []
    for i, n in enumerate(sizes):
        base = _base() + i * step_ms
        d = g.integers(0, step_ms, n)
        keys = g.integers(0, 3_000, n).astype(np.int32)
        for cell, c in _ref(keys, d + base, LEN).items():
            ref[cell] = ref.get(cell, 0) + c
        par = getattr(st, "_pipe_parity", 0)
        assert par == i % 2
        st.insert_pipelined(
            torch.from_numpy(keys).cuda(),
            torch.from_numpy(d.astype(np.int32)).cuda(), None, int(base),
            [], [], int(base + step_ms - 1),
        )
        assert st._ev_fmt[par] == FMT_COMPACT
        assert st._ev_w[par] == _entry_base(base, 8)
        seen.append(st._ev_w[par])
        if i == 1:
            assert st._ev_w[0] != st._ev_w[1]
            closed = _rows(st.close_due(), st)
            assert len(closed) > 0
            got.update(closed)
    assert len(set(seen)) == 4
    tail = _rows(st.close_all(), st)
    assert not (set(tail) & set(got)), "cell closed twice"
    got.update(tail)
    assert got == ref
    assert int(st.error_flag.item()) == 0


def _stream(shape, span_windows, pipelined, monkeypatch):
    """Three batches whose events span `span_windows` windows from each
    batch's base, a watermark close after each, then the rest; returns
    the state, its format after every batch, and whether rows are
    exact."""
    from bytewax_amd.gpu import RecordBatch

    g = np.random.default_rng(71)
    n = 6_000
    st = _state(shape, n)
    ref, got, compact_ok, fmts = {}, {}, [], []
    for i in range(3):
        base = _base() + i * span_windows * LEN
        d = g.integers(0, span_windows * LEN, n)
        keys = g.integers(0, 500, n).astype(np.int32)
        for cell, c in _ref(keys, d + base, LEN).items():
            ref[cell] = ref.get(cell, 0) + c
        tk = torch.from_numpy(keys).cuda()
        tt = torch.from_numpy(d.astype(np.int32)).cuda()
        # The watermark stays one span behind, so every batch leaves
        # open windows for the next one to add to.
        wm = int(base - 1)
        if pipelined:
            st.insert_pipelined(tk, tt, None, int(base), [], [], wm)
            fmts.append(st._ev_fmt[i % 2])
        else:
            st.insert(RecordBatch(tk, tt, max_ts=wm, ts_base=int(base)))
        closed = _rows(st.close_due(), st)
        assert not (set(closed) & set(got)), "cell closed twice"
        got.update(closed)
        compact_ok.append(st.compact_ok)
    tail = _rows(st.close_all(), st)
    assert not (set(tail) & set(got)), "cell closed twice"
    got.update(tail)
    assert int(st.error_flag.item()) == 0
    return st, compact_ok, fmts, got == ref


@pytest.mark.parametrize("pipelined", [False, True])
@pytest.mark.parametrize("shape", ["s128", "s512"])
def test_wide_stream_demotes_at_its_first_close(shape, pipelined, monkeypatch):
    """Batches that span 4 x 2^D windows: most of each batch is spilled,
    the first close sees it and the state keeps hashed entries from the
    second batch on.  Rows are exact before and after."""
    _prep(monkeypatch)
    D = SHAPES[shape][3]
    st, compact_ok, fmts, exact = _stream(
        shape, 4 << D, pipelined, monkeypatch)
    assert exact
    assert compact_ok == [False, False, False]
    assert int(st.spill_total.item()) > 6_000 // 2
    if pipelined:
        assert fmts == [FMT_COMPACT, FMT_HASHED, FMT_HASHED]


@pytest.mark.parametrize("pipelined", [False, True])
def test_stream_inside_the_reach_never_demotes(pipelined, monkeypatch):
    _prep(monkeypatch)
    st, compact_ok, fmts, exact = _stream("s512", 100, pipelined, monkeypatch)
    assert exact
    assert compact_ok == [True, True, True]
    assert fmts == ([FMT_COMPACT] * 3 if pipelined else [])
    assert int(st.spill_total.item()) == 0
