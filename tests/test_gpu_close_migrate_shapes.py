"""Window close with reclamation (``k_close_migrate``) at awkward
shapes.

The kernel walks the table in 2048-slot chunks, reserves the output
rows of a chunk with one atomic, and rebuilds the live cells in a fresh
table.  The cases pin: tables smaller than, equal to and larger than a
chunk (down to the one-slot table), closes that take nothing,
everything and half of the cells, probe chains that must survive the
rebuild, and an output buffer smaller than the rows due.  Every result
is compared exactly against a plain-Python ``Counter``.
"""

from collections import Counter
from datetime import datetime, timezone

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

ALIGN = datetime(2024, 1, 1, tzinfo=timezone.utc)
LEN_MS = 1_000


def _skip_no_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _align_ms():
    from bytewax_amd.gpu import _ms

    return _ms(ALIGN)


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


def _state(slots_pow, out_cap=1 << 16, max_batch=1 << 16):
    from bytewax_amd.gpu import AGG_COUNT, WindowAggState

    # The region layout from 2^14 slots up, whole-table probing below.
    radix = slots_pow >= 14
    return WindowAggState(
        torch.device("cuda:0"), _align_ms(), LEN_MS, AGG_COUNT,
        slots_pow=slots_pow, out_cap=out_cap, radix=radix, region_bits=11,
        max_batch=max_batch,
    )


def _events(n_cells, seed, windows=(0, 1)):
    """Events over `n_cells` distinct (key, window) cells, alternating
    between the windows, one to three events per cell."""
    g = torch.Generator().manual_seed(seed)
    align_ms = _align_ms()
    cell_keys = torch.randperm(1 << 20, generator=g)[:n_cells].to(torch.int32)
    cell_wins = torch.tensor(windows, dtype=torch.int64)[
        torch.arange(n_cells) % len(windows)
    ]
    reps = torch.randint(1, 4, (n_cells,), generator=g)
    keys = torch.repeat_interleave(cell_keys, reps)
    wins = torch.repeat_interleave(cell_wins, reps)
    ts = align_ms + wins * LEN_MS + torch.randint(
        0, LEN_MS, (keys.numel(),), dtype=torch.int64, generator=g
    )
    ref = Counter()
    for k, w in zip(keys.tolist(), wins.tolist()):
        ref[(k, w)] += 1
    return keys, ts, ref


# (slots_pow, cells): the one-slot table, one power of two below a
# chunk, exactly one chunk, 2^14 and 2^18 in the region layout.
TABLES = [(0, 1), (10, 512), (11, 1_000), (14, 6_000), (18, 30_000)]
_CASES = {}


def _case(slots_pow, n_cells):
    if slots_pow not in _CASES:
        _CASES[slots_pow] = _events(n_cells, 40 + slots_pow)
    return _CASES[slots_pow]


@pytest.mark.parametrize("due", ["none", "half", "all"])
@pytest.mark.parametrize("slots_pow,n_cells", TABLES)
def test_close_due_coverage(slots_pow, n_cells, due, monkeypatch):
    _skip_no_gpu()
    monkeypatch.delenv("BYTEWAX_SCATTER", raising=False)
    from bytewax_amd.gpu import RecordBatch

    keys, ts, ref = _case(slots_pow, n_cells)
    align_ms = _align_ms()
    # Watermark at the end of window 0 / 1 / 2: windows wholly below it
    # are due.
    n_due_windows = {"none": 0, "half": 1, "all": 2}[due]
    wm = align_ms + (n_due_windows + 1) * LEN_MS - 1
    state = _state(slots_pow)
    state.insert(RecordBatch(keys.cuda(), ts.cuda(), None, max_ts=wm))
    closed = _rows(state.close_due(), state)
    want_closed = Counter(
        {c: v for c, v in ref.items() if c[1] < n_due_windows}
    )
    assert closed == want_closed
    # The rebuilt table holds exactly the rest.
    rest = _rows(state.close_all(), state)
    assert int(state.error_flag.item()) == 0
    assert rest == Counter(
        {c: v for c, v in ref.items() if c[1] >= n_due_windows}
    )
    # The retired table was reset for the next close.
    assert bool((state.tkeys_alt == -1).all())
    assert int(state.tvals_alt.abs().sum()) == 0


@pytest.mark.parametrize("slots_pow,n_cells", [(11, 1_000), (14, 8_000)])
def test_probe_chains_survive_rebuild(slots_pow, n_cells, monkeypatch):
    """Insert, close half, insert the live keys again (and a new
    window), close_all: a migrated cell that a later insert could not
    find again would show up twice."""
    _skip_no_gpu()
    monkeypatch.delenv("BYTEWAX_SCATTER", raising=False)
    from bytewax_amd.gpu import RecordBatch

    align_ms = _align_ms()
    keys, ts, ref = _events(n_cells, 7)
    state = _state(slots_pow)
    wm = align_ms + 2 * LEN_MS - 1
    state.insert(RecordBatch(keys.cuda(), ts.cuda(), None, max_ts=wm))
    closed = _rows(state.close_due(), state)
    assert closed == Counter({c: v for c, v in ref.items() if c[1] == 0})
    # Same keys again: window 1 (live, migrated) and window 2 (new).
    live = ts >= align_ms + LEN_MS
    keys2 = torch.cat([keys[live], keys[live]])
    ts2 = torch.cat([ts[live], ts[live] + LEN_MS])
    state.insert(RecordBatch(keys2.cuda(), ts2.cuda()))
    want = Counter()
    for (k, w), v in ref.items():
        if w == 1:
            want[(k, 1)] = 2 * v
            want[(k, 2)] = v
    rest = _rows(state.close_all(), state)
    assert int(state.error_flag.item()) == 0
    assert rest == want


def test_two_closes_in_a_row(monkeypatch):
    """Close, then close again one window later: the second close reads
    the table the first one built."""
    _skip_no_gpu()
    monkeypatch.delenv("BYTEWAX_SCATTER", raising=False)
    from bytewax_amd.gpu import RecordBatch

    align_ms = _align_ms()
    keys, ts, ref = _events(9_000, 11, windows=(0, 1, 2))
    state = _state(14)
    state.insert(
        RecordBatch(keys.cuda(), ts.cuda(), None,
                    max_ts=align_ms + 2 * LEN_MS - 1)
    )
    got = _rows(state.close_due(), state)
    assert set(w for _k, w in got) == {0}
    state.max_ts_host = align_ms + 3 * LEN_MS - 1
    second = _rows(state.close_due(), state)
    assert set(w for _k, w in second) == {1}
    got.update(second)
    tail = _rows(state.close_all(), state)
    assert set(w for _k, w in tail) == {2}
    got.update(tail)
    assert int(state.error_flag.item()) == 0
    assert got == ref


def test_out_cap_smaller_than_rows_due(monkeypatch):
    """More rows due than the output holds: the count is still the
    total, and nothing is written past the capacity."""
    _skip_no_gpu()
    monkeypatch.delenv("BYTEWAX_SCATTER", raising=False)
    from bytewax_amd.gpu import RecordBatch

    align_ms = _align_ms()
    keys, ts, ref = _events(5_000, 3, windows=(0,))
    cap = 100
    state = _state(14, out_cap=cap)
    dev = state.out_keys.device
    guard = 4_096
    big_k = torch.full((cap + guard,), -7, dtype=torch.int32, device=dev)
    big_w = torch.full((cap + guard,), -7, dtype=torch.int32, device=dev)
    big_v = torch.full((cap + guard,), -7, dtype=torch.int64, device=dev)
    state.out_keys, state.out_wins, state.out_vals = (
        big_k[:cap], big_w[:cap], big_v[:cap]
    )
    state.insert(
        RecordBatch(keys.cuda(), ts.cuda(), None,
                    max_ts=align_ms + 2 * LEN_MS - 1)
    )
    with pytest.raises(RuntimeError, match=f"produced {len(ref)} rows"):
        state.close_due()
    assert int(state.out_n.item()) == len(ref)
    for big in (big_k, big_w, big_v):
        assert bool((big[cap:] == -7).all()), "write past out_cap"
    # The rows that fit are real cells of the due window.
    for k, w, v in zip(big_k[:cap].tolist(), big_w[:cap].tolist(),
                       big_v[:cap].tolist()):
        assert ref[(k, w)] == v
