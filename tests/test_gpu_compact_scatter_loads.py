"""The compact scatter's column loads and its event-to-lane mapping.

A lane of ``k_radix_scatter_compact`` holds four consecutive events at a
time (slot ``u = 4q + j`` of lane ``tid`` is event ``(q * 512 + tid) * 4
+ j`` of an 8192-event tile), full tiles are loaded 16 bytes at a time
when both columns are 16-byte aligned, and the last, partial tile is
loaded in clamped dwords.  These tests walk the sizes around a vector, a
wave's worth of vectors and a tile, columns that start 4, 8 and 12 bytes
off alignment, and the events that leave the fast path (beyond the entry
reach, before ``align_to``) at chosen places of that mapping.

Expected rows come from a numpy group-by, expected entries from the
numpy twin of the mixer; shapes are ``s128`` (2^20 slots, n = 38) and
``s512`` (2^22 slots, n = 40, the benchmark's).
"""

from datetime import datetime, timezone

import numpy as np
import pytest
from test_compact_entries_twin import decode, encode

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

ALIGN = datetime(2024, 1, 1, tzinfo=timezone.utc)
FMT_COMPACT = 2
KNOBS = ("BYTEWAX_AGG", "BYTEWAX_SCATTER", "BYTEWAX_ENTRIES",
         "BYTEWAX_SCATTER_THREADS", "BYTEWAX_SCATTER_U",
         "BYTEWAX_SCATTER_BLOCKS", "BYTEWAX_AGG_R")
# name -> (slots_pow, region_bits, segments, D)
SHAPES = {"s128": (20, 11, 128, 6), "s512": (22, 11, 512, 8)}
EXTREME = [0, -1, -(1 << 31), (1 << 31) - 1]
LEN = 60_000
TILE = 8192
SIZES = [1, 3, 4, 5, 2047, 2048, 2049, 8191, 8192, 8193, 3 * 8192 + 7]
BLOCKS = ["default", "1"]


def _prep(monkeypatch, blocks="default"):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    if blocks != "default":
        monkeypatch.setenv("BYTEWAX_SCATTER_BLOCKS", blocks)


def _align_ms():
    from bytewax_amd.gpu import _ms

    return _ms(ALIGN)


def _base():
    return _align_ms() + 10_000 * LEN + 17


def _entry_base(D):
    return (_base() - _align_ms()) // LEN - (1 << (D - 1))


def _windows(d):
    """Window of each delta from `_base()`; towards zero before
    `align_to`, as the generic window code divides."""
    x = np.asarray(d, dtype=np.int64) + _base() - _align_ms()
    return np.where(x >= 0, x // LEN, -((-x) // LEN))


def _group(keys, wins):
    pairs = np.stack([np.asarray(keys, dtype=np.int64), wins], axis=1)
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


def _columns(keys, d, koff, toff):
    """The two columns on the device, each a view `off` elements into a
    larger tensor (allocations are at least 16-byte aligned)."""
    out = []
    for col, off in ((keys, koff), (d, toff)):
        big = torch.zeros(len(col) + 4, dtype=torch.int32, device="cuda")
        assert big.data_ptr() % 16 == 0
        view = big[off:off + len(col)]
        view.copy_(torch.from_numpy(np.asarray(col).astype(np.int32)))
        assert view.data_ptr() % 16 == 4 * off
        out.append(view)
    return out


def _run(shape, keys, d, koff=0, toff=0):
    """Scatter alone, read the buffers, aggregate, close.  Returns the
    sorted `segment << 31 | entry` words, the sorted spill words, the
    closed rows and max_ts."""
    from bytewax_amd.gpu import AGG_COUNT, WindowAggState

    slots_pow, region_bits, nseg, D = SHAPES[shape]
    st = WindowAggState(
        torch.device("cuda:0"), _align_ms(), LEN, AGG_COUNT,
        slots_pow=slots_pow, radix=True, region_bits=region_bits,
        # Room for every segment's share and each block's padded final
        # flush below `cap`, so that nothing spills for want of room.
        max_batch=max(len(keys), 100_000),
    )
    bufs = (st.rx_gcursors, st.rx_packed, st.rx_vals, st.rx_ov_cursor,
            st.rx_ov_packed, st.rx_ov_vals)
    tk, tt = _columns(keys, d, koff, toff)
    w, fmt = st.k.radix_scatter_only(
        tk, tt, None, st.max_ts_dev, st.error_flag, *bufs, st.nslots,
        st.align_ms, st.len_ms, st.mode, int(_base()), st.region_bits,
        st.off_ms, [], [], True,
    )
    torch.cuda.synchronize()
    assert (w, fmt) == (_entry_base(D), FMT_COMPACT)
    cap = (st.rx_packed.numel() // nseg) & ~15
    cur = st.rx_gcursors[:nseg].cpu().numpy()
    assert cap >= 256
    assert (cur % 16 == 0).all() and (cur <= cap).all()
    ev = st.rx_packed.view(torch.int32).cpu().numpy().view(np.uint32)
    words = []
    for b in np.flatnonzero(cur):
        e = ev[b * cap:b * cap + cur[b]]
        e = e[e != 0xFFFFFFFF]
        assert (e >> 31 == 0).all()
        words.append((np.uint64(b) << np.uint64(31)) | e.astype(np.uint64))
    words = np.sort(np.concatenate(words)) if words else np.zeros(0, np.uint64)
    nov = int(st.rx_ov_cursor.item())
    spill = np.sort(st.rx_ov_packed[:nov].cpu().numpy().view(np.uint64))
    st.k.radix_agg_only(st.tkeys, st.tvals, st.error_flag, *bufs, st.mode,
                        st.region_bits, w, fmt)
    torch.cuda.synchronize()
    rows = _rows(st.close_all(), st)
    assert int(st.error_flag.item()) == 0
    return words, spill, rows, int(st.max_ts_dev.item())


def _want_words(keys, d, D):
    """What the twin says the buffer holds when every event fits."""
    delta = _windows(d) - _entry_base(D)
    assert delta.min() >= 0 and delta.max() < (1 << D)
    seg, ent = encode(np.asarray(keys), delta, 32 + D)
    return np.sort((seg.astype(np.uint64) << np.uint64(31)) |
                   ent.astype(np.uint64))


def _check(shape, keys, d, **kw):
    D = SHAPES[shape][3]
    words, spill, rows, max_ts = _run(shape, keys, d, **kw)
    assert np.array_equal(words, _want_words(keys, d, D))
    assert spill.size == 0
    assert rows == _group(keys, _windows(d))
    assert max_ts == int(np.max(d)) + _base()
    return words, rows, max_ts


@pytest.mark.parametrize("blocks", BLOCKS)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_tile_and_vector_edges(shape, n, blocks, monkeypatch):
    """Both sides of one vector, of a wave's vectors (2048 events) and
    of a tile, and three tiles and seven events; with one block the full
    -tile loads, the prefetch and the partial last tile all run.  The
    maximum sits at the last event, then at event 0."""
    _prep(monkeypatch, blocks)
    g = np.random.default_rng(n)
    keys = g.integers(-(1 << 31), 1 << 31, n)
    keys[: n // 2] = g.integers(0, 300, n // 2)
    for at in (n - 1, 0):
        d = g.integers(-LEN, 2 * LEN, n)
        d[at] = 2 * LEN + 7
        _check(shape, keys, d)


_ALIGNED = {}


def _aligned(shape):
    """One batch of a tile and five events, and what an aligned copy of
    it scatters to; computed once for each shape."""
    if shape not in _ALIGNED:
        g = np.random.default_rng(77)
        n = TILE + 5
        keys = g.integers(-(1 << 31), 1 << 31, n)
        d = g.integers(-LEN, 2 * LEN, n)
        _ALIGNED[shape] = (keys, d, _check(shape, keys, d))
    return _ALIGNED[shape]


@pytest.mark.parametrize("blocks", BLOCKS)
@pytest.mark.parametrize(
    "koff,toff", [(0, 0), (1, 0), (2, 0), (3, 0), (0, 1), (0, 2), (0, 3),
                  (3, 1)])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_unaligned_columns(shape, koff, toff, blocks, monkeypatch):
    """Columns that start 1, 2 and 3 elements into a tensor, each column
    on its own, give what a fresh aligned copy gives."""
    _prep(monkeypatch)
    keys, d, (words, rows, max_ts) = _aligned(shape)
    _prep(monkeypatch, blocks)
    got = _check(shape, keys, d, koff=koff, toff=toff)
    assert np.array_equal(got[0], words)
    assert got[1:] == (rows, max_ts)


@pytest.mark.parametrize("blocks", BLOCKS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_rare_events_under_the_mapping(shape, blocks, monkeypatch):
    """Events that leave the fast path at chosen slots: the four slots
    of lane 0, the last slot of the first quarter's last lane, both
    sides of the tile edge, the last event of the partial tile, and
    lane 100 once for each j (q = j).  Every other one is beyond the
    entry reach, the rest lie before `align_to`.  Exactly these are in
    the spill, with their own key and window."""
    _prep(monkeypatch, blocks)
    D = SHAPES[shape][3]
    g = np.random.default_rng(13)
    n = TILE + 77
    chosen = [0, 1, 2, 3, 4 * 511 + 3, 8191, 8192, n - 1]
    chosen += [(j * 512 + 100) * 4 + j for j in range(4)]
    chosen = np.array(chosen)
    keys = g.integers(0, 5_000, n)
    d = g.integers(-LEN, 2 * LEN, n)
    keys[chosen] = 1_000_000 + chosen
    far = (1 << D) * LEN + 11                   # 2^(D-1) windows past the reach
    early = _align_ms() - _base() - 5           # 5 ms before align_to
    d[chosen] = np.where(np.arange(chosen.size) % 2 == 0, far, early)
    wins = _windows(d)
    assert (wins[chosen[1::2]] == 0).all()
    rest = np.ones(n, dtype=bool)
    rest[chosen] = False
    words, spill, rows, max_ts = _run(shape, keys, d)
    want_spill = np.sort(
        (wins[chosen].astype(np.uint64) << np.uint64(32)) |
        keys[chosen].astype(np.uint64))
    assert np.array_equal(spill, want_spill)
    assert np.array_equal(words, _want_words(keys[rest], d[rest], D))
    assert rows == _group(keys, wins)
    assert max_ts == far + _base()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_extreme_keys_at_both_ends_of_the_delta(shape, monkeypatch):
    """0, -1, -2^31 and 2^31 - 1 under delta 0 and under 2^D - 1."""
    _prep(monkeypatch)
    D = SHAPES[shape][3]
    keys = np.tile(np.array(EXTREME), 2)
    delta = np.repeat(np.array([0, (1 << D) - 1]), len(EXTREME))
    d = (delta + _entry_base(D)) * LEN + _align_ms() - _base() + 3
    words, _, _ = _check(shape, keys, d)
    seg = (words >> np.uint64(31)).astype(np.int64)
    ent = (words & np.uint64(0x7FFFFFFF)).astype(np.uint32)
    k2, d2 = decode(seg, ent, 32 + D)
    assert sorted(zip(k2.tolist(), d2.tolist())) == sorted(
        zip(keys.tolist(), delta.tolist()))
