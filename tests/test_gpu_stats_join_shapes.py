"""Keyed stats and stream join state, at the shapes and edges where
their partition -> LDS collapse -> flush pipelines can go wrong.

Both references are plain numpy / Python and exact (everything is
int64, so nothing has a tolerance):

- stats: ``{(key, window): (count, sum mod 2^64, min, max)}`` by a
  group-by, for events at or after the alignment only;
- join: `JoinModel`, a per-key model of "last" insert / "complete"
  emit with one side per call.  It carries the set of flag states the
  documented semantics allow per key, checks the exact number of rows
  per key per drain, that every value is one the key could hold, and
  `snapshot_to_host()` against the allowed live cells.

Both run against the CPU twins in the unmarked tests, so the models
are themselves checked where there is no GPU.  The device tests reuse
the same case bodies.

Every device case first asserts, from `_mix64` (the host port of the
kernels' hash) and from host copies of the launchers' sizing formulas
(`_stats_plan`, `_join_plan`, `_rx_totals`), that its inputs have the
property that takes the kernel down the path in question:

====================  =============================================
path                  case / host-side condition
====================  =============================================
k_radix_agg_stats     `lds_full`: > 2^seg_bits distinct cells in
LDS-full fall-        one segment, segment load <= cap (nothing of
through, pad skip,    it spills); `clamp_cap`: `hot` (cursor > cap);
clamp_cap, 256/1024   pads: every staged batch that is no multiple
threads               of 8 per segment; block size: `rb4*` (256)
                      and `rb10*` (1024)
k_overflow_agg_stats  `hot`: 20,000 events of a cell > cap; the
                      sizes below the staged threshold (cap 1)
scatter ladder        `rb10`: seg_bits 12 > 11 -> one coarse bit
(stats)               less; `rb10_c4`: three rounds of the loop;
                      `rb4_fixed`; sizes with cap < SC_GRAN
scatter choice        `order pairs`: first batch below / above the
(join)                size at which cap reaches SC_GRAN; small
                      after large (staged, large cap); `lds160`:
                      staged LDS > 160 KiB -> fixed; `fixed`;
                      `one_segment_table`: nb < 1 (16 slots)
k_join_region_lds     `t256` / `t512` / default threads; `lds_full`
                      (seg_bits 13 > 12: > 4,096 distinct keys in
                      one segment, none spilled); lcnt >= 2 re-arm:
                      duplicated keys of `accumulate` whose segment
                      neither spills nor fills its LDS must end at
                      exactly ``1 << side``
k_join_region         `nolds`
k_join_overflow       `hot`: 20,000 events of a key > cap
keys and values       `edges`: keys -1, -2, INT32_MIN, INT32_MAX,
                      0; values INT64_MIN, INT64_MAX, 0, -1; sums
                      that wrap; one-value min/max cells
extract(horizon)      `horizon`; `out_cap` and table-overflow
                      errors in `errors`
max_ts_dev            `max_ts`, int64 and int32-delta timestamps
join snapshot         `snapshot`: side-0-only, side-1-only and
                      completed keys
====================  =============================================

No case asserts which duplicate's value a row carries; singleton keys
are used wherever an exact value is wanted.
"""

from datetime import datetime, timezone

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from bytewax_amd.gpu import RecordBatch, _ms  # noqa: E402
from bytewax_amd.gpu.state import HashJoinState, StatsAggState  # noqa: E402

ALIGN_MS = _ms(datetime(2024, 1, 1, tzinfo=timezone.utc))
LEN_MS = 60_000
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
SC_GRAN = 8  # events per cursor reservation of the staged scatter
TILE = 8192  # events per staged-scatter block iteration (512 x 16)
SIZES = [1, 63, 64, 65, 255, 256, 257, 8191, 8192, 8193, 3 * 8192 + 1]
KNOBS = (
    "BYTEWAX_SCATTER", "BYTEWAX_SCATTER_DIRECT",
    "BYTEWAX_SCATTER_COARSE_BITS", "BYTEWAX_SCATTER_U",
    "BYTEWAX_SCATTER_THREADS", "BYTEWAX_SCATTER_BLOCKS",
    "BYTEWAX_JOIN_COARSE", "BYTEWAX_JOIN_LDS", "BYTEWAX_JOIN_THREADS",
    "BYTEWAX_JOIN_RADIX",
)
CPU = torch.device("cpu")


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _select(monkeypatch, env):
    """Set the knobs of one variant and clear every other one."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# -- host hash ---------------------------------------------------------


def _mix64(x):
    """The kernels' `mix64` (splitmix64 finalizer) on a uint64 array."""
    x = np.atleast_1d(np.asarray(x)).astype(np.uint64)
    x = x ^ (x >> np.uint64(33))
    x = x * np.uint64(0xFF51AFD7ED558CCD)
    x = x ^ (x >> np.uint64(33))
    x = x * np.uint64(0xC4CEB9FE1A85EC53)
    x = x ^ (x >> np.uint64(33))
    return x


def _packed(keys, wins=None):
    """`window << 32 | (uint32)key`; the join packs the bare key."""
    k = np.atleast_1d(np.asarray(keys)).astype(np.int64) & 0xFFFFFFFF
    if wins is None:
        return k.astype(np.uint64)
    w = np.atleast_1d(np.asarray(wins)).astype(np.int64) & 0xFFFFFFFF
    return ((w << 32) | k).astype(np.uint64)


def _segment(packed, slots_pow, bits):
    """`(mix64(packed) & mask) >> bits`: scatter segment or table
    region of an event."""
    mask = np.uint64((1 << slots_pow) - 1)
    return ((_mix64(packed) & mask) >> np.uint64(bits)).astype(np.int64)


def test_mix64_port_matches_scalar_form():
    m64 = (1 << 64) - 1

    def scalar(x):
        x ^= x >> 33
        x = (x * 0xFF51AFD7ED558CCD) & m64
        x ^= x >> 33
        x = (x * 0xC4CEB9FE1A85EC53) & m64
        x ^= x >> 33
        return x

    xs = [0, 1, 7, 0xFFFFFFFF, (5 << 32) | 0xFFFFFFFE, m64 - 1, 1 << 63]
    assert [int(v) for v in _mix64(np.array(xs, dtype=np.uint64))] == [
        scalar(x) for x in xs
    ]
    # Keys are packed as uint32: -1 is 0xFFFFFFFF, never all ones.
    assert int(_packed(-1)[0]) == 0xFFFFFFFF
    assert int(_packed(-1, 2)[0]) == (2 << 32) | 0xFFFFFFFF
    assert int(_segment(_packed(3, 1), 14, 6)[0]) == (
        (scalar((1 << 32) | 3) & ((1 << 14) - 1)) >> 6
    )


# -- host copies of the sizing formulas --------------------------------


def _rx_totals(sizes, n_regions):
    """Scatter-buffer length at each insert of a state that saw
    batches of `sizes` in this order (`insert` of both states)."""
    out, max_batch, total = [], 0, 1
    for n in sizes:
        if n > max_batch:
            max_batch = n * 5 // 4
            total = (-(-max_batch * 5 // 2) // n_regions + 1) * n_regions
        out.append(total)
    return out


def _staged_lds(nseg):
    return nseg * SC_GRAN * 8 * 2 + 4 * nseg * 4


def _stats_plan(total, slots_pow, region_bits, env):
    """(kind, seg_bits, nseg, cap) as `radix_stats_insert_impl`
    decides them."""
    nslots = 1 << slots_pow
    kind = "fixed" if env.get("BYTEWAX_SCATTER") == "fixed" else "staged"
    coarse = int(
        env.get("BYTEWAX_SCATTER_COARSE_BITS", 2 if kind == "staged" else 0)
    )
    seg_bits = region_bits + coarse
    nseg = nslots >> seg_bits
    while kind == "staged" and (
        nseg < 1 or _staged_lds(nseg) > 160 * 1024 or seg_bits > 11
    ):
        if coarse > 0 and seg_bits > 11:
            coarse -= 1
        else:
            kind, coarse = "fixed", 0
        seg_bits = region_bits + coarse
        nseg = nslots >> seg_bits
    if seg_bits > 11:
        seg_bits = region_bits
        nseg = nslots >> seg_bits
    cap = total // nseg
    if kind == "staged":
        cap &= ~(SC_GRAN - 1)
        if cap < SC_GRAN:
            kind, seg_bits = "fixed", region_bits
            nseg = nslots >> seg_bits
            cap = total // nseg
    return kind, seg_bits, nseg, cap


def _join_plan(total, slots_pow, region_bits, env):
    """(kind, seg_bits, nseg, cap, lds_slots) as `radix_join_insert`
    decides them."""
    nslots = 1 << slots_pow
    seg_bits = region_bits + int(env.get("BYTEWAX_JOIN_COARSE", 1))
    nseg = nslots >> seg_bits
    if nseg < 1:
        nseg, seg_bits = 1, slots_pow
    cap = total // nseg
    kind = "fixed" if env.get("BYTEWAX_SCATTER") == "fixed" else "staged"
    if kind == "staged":
        cap &= ~(SC_GRAN - 1)
        if cap < SC_GRAN or _staged_lds(nseg) > 160 * 1024:
            kind, cap = "fixed", total // nseg
    lds_bits = min(max(seg_bits + 1, 6), 12)
    return kind, seg_bits, nseg, cap, 1 << lds_bits


def _cursor_bound(kind, n, load):
    """Upper bound of the segment cursors after a batch of `n` events
    that puts `load` of them into the segments: every block of the
    staged scatter pads its last granule of a segment."""
    load = np.asarray(load)
    if kind == "fixed":
        return load
    blocks = min(max(-(-n // TILE), 1), 1024)
    if blocks == 1:
        return -(-load // SC_GRAN) * SC_GRAN
    return load + (SC_GRAN - 1) * blocks


# -- stats reference ---------------------------------------------------


def _ref_stats(keys, x, vals):
    """Group-by over events given as offsets `x` from the alignment.
    Floor (here) and the kernels' truncation agree only for x >= 0."""
    keys = np.asarray(keys, dtype=np.int64)
    x = np.asarray(x, dtype=np.int64)
    vals = np.asarray(vals, dtype=np.int64)
    assert (x >= 0).all(), "events before the alignment are out of scope"
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


def test_ref_stats_wraps_and_rejects_early_events():
    ref = _ref_stats([5, 5, 5, -1], [0, 1, 2, LEN_MS], [I64_MAX, I64_MAX, 1, 9])
    assert ref == {
        (5, 0): (3, -1, 1, I64_MAX),
        (-1, 1): (1, 9, 9, 9),
    }
    with pytest.raises(AssertionError):
        _ref_stats([1], [-1], [0])


def _cat(batches):
    return tuple(np.concatenate([b[i] for b in batches]) for i in range(3))


def _got_stats(out):
    if out is None:
        return {}
    cols = [
        out[name].cpu().tolist()
        for name in ("keys", "wins", "cnt", "sum", "min", "max")
    ]
    got = {}
    for k, w, c, s, mn, mx in zip(*cols):
        assert (k, w) not in got, f"cell {(k, w)} emitted twice"
        got[(k, w)] = (c, s, mn, mx)
    return got


# name -> (constructor arguments, knobs, expected nslots, seg_bits of a
# batch large enough for the staged scatter)
STATS_GEOMS = {
    "rb4": (dict(region_bits=4), {}, 1 << 14, 6),
    "rb4_fixed": (
        dict(region_bits=4), {"BYTEWAX_SCATTER": "fixed"}, 1 << 14, 4,
    ),
    "rb10": (dict(region_bits=10), {}, 1 << 20, 11),
    "rb10_c4": (
        dict(region_bits=10), {"BYTEWAX_SCATTER_COARSE_BITS": "4"},
        1 << 20, 11,
    ),
    "direct": (dict(radix=False, slots_pow=14), {}, 1 << 14, None),
}


def _stats_state(dev, geom, monkeypatch, out_cap=1 << 15):
    kw, env, nslots, _seg = STATS_GEOMS[geom]
    _select(monkeypatch, env)
    # slots_pow=10 for the radix geometries: the constructor raises it
    # to region_bits + 10, which is what the cases are sized for.
    args = dict(slots_pow=10, out_cap=out_cap)
    args.update(kw)
    st = StatsAggState(dev, ALIGN_MS, LEN_MS, **args)
    if not st.cpu:
        assert st.nslots == nslots
    return st


def _plan_for(geom, sizes):
    """Plans of every insert of `sizes` into a fresh state of `geom`."""
    kw, env, nslots, _seg = STATS_GEOMS[geom]
    slots_pow = nslots.bit_length() - 1
    rb = kw["region_bits"]
    return [
        _stats_plan(t, slots_pow, rb, env)
        for t in _rx_totals(sizes, nslots >> rb)
    ]


def _stats_insert(st, batch, ts_form="abs"):
    keys, x, vals = batch
    k = torch.from_numpy(np.asarray(keys, dtype=np.int32))
    v = torch.from_numpy(np.asarray(vals, dtype=np.int64))
    x = np.asarray(x, dtype=np.int64)
    if ts_form == "abs":
        ts, base = torch.from_numpy(ALIGN_MS + x), 0
    else:
        # int32 deltas against a base inside the batch's range, so
        # there are negative deltas too.
        mid = int(np.sort(x)[x.size // 2])
        ts, base = torch.from_numpy((x - mid).astype(np.int32)), ALIGN_MS + mid
    dev = st.device
    st.insert(RecordBatch(k.to(dev), ts.to(dev), v.to(dev), ts_base=base))


def _stats_check(st, ref):
    got = _got_stats(st.extract(clear=False))
    if not st.cpu:
        assert int(st.error_flag.item()) == 0
    assert got == ref


def _uniform_stats(n, seed, n_keys=300, n_win=3, lo=-(1 << 40), hi=1 << 40):
    rng = np.random.default_rng(seed)
    keys = rng.integers(-n_keys // 2, n_keys // 2, n).astype(np.int32)
    x = rng.integers(0, n_win * LEN_MS, n)
    vals = rng.integers(lo, hi, n)
    return keys, x, vals


_CACHE = {}


def _cached(name, build):
    """Inputs and references depend on the case, not on the variant."""
    if name not in _CACHE:
        _CACHE[name] = build()
    return _CACHE[name]


# -- stats case bodies (run on the CPU twin and on the device) ---------


def _stats_sizes_inputs():
    out = {}
    for n in SIZES:
        b = _uniform_stats(n, seed=100 + n % 97)
        out[n] = (b, _ref_stats(*b))
    return out


def _case_stats_sizes(dev, geom, ts_form, monkeypatch):
    inputs = _cached("stats_sizes", _stats_sizes_inputs)
    if geom != "direct":
        plans = [_plan_for(geom, [n])[0] for n in SIZES]
        kinds = {p[0] for p in plans}
        if "fixed" not in STATS_GEOMS[geom][1].values():
            # cap < SC_GRAN for the small sizes, staged for the large.
            assert kinds == {"fixed", "staged"}
            assert plans[0][3] < SC_GRAN
        assert plans[-1][1] == STATS_GEOMS[geom][3]
    for n in SIZES:
        batch, ref = inputs[n]
        st = _stats_state(dev, geom, monkeypatch)
        _stats_insert(st, batch, ts_form)
        _stats_check(st, ref)
        if not st.cpu:
            assert int(st.max_ts_dev.item()) == ALIGN_MS + int(batch[1].max())


def _accumulate_inputs():
    batches = [_uniform_stats(3_000, seed=200 + i) for i in range(5)]
    return batches, _ref_stats(*_cat(batches))


def _case_stats_accumulate(dev, geom, monkeypatch):
    batches, ref = _cached("stats_acc", _accumulate_inputs)
    st = _stats_state(dev, geom, monkeypatch)
    for i, b in enumerate(batches):
        _stats_insert(st, b, "abs" if i % 2 == 0 else "delta")
    _stats_check(st, ref)


def _hot_batch(n_cells, seed):
    rng = np.random.default_rng(seed)
    hot_k = np.array([7, -3, 1234][:n_cells], dtype=np.int32)
    hot_w = np.array([1, 0, 2][:n_cells])
    pick = rng.integers(0, n_cells, 20_000)
    uk, ux, uv = _uniform_stats(2_000, seed + 1)
    keys = np.concatenate([hot_k[pick], uk])
    x = np.concatenate([hot_w[pick] * LEN_MS + rng.integers(0, LEN_MS, 20_000), ux])
    vals = np.concatenate([rng.integers(-(1 << 50), 1 << 50, 20_000), uv])
    perm = rng.permutation(keys.size)
    return keys[perm], x[perm], vals[perm]


def _case_stats_hot(dev, geom, n_cells, monkeypatch):
    batch, ref = _cached(
        f"stats_hot{n_cells}",
        lambda: (lambda b: (b, _ref_stats(*b)))(_hot_batch(n_cells, 300)),
    )
    if geom != "direct":
        _kind, seg_bits, _nseg, cap = _plan_for(geom, [batch[0].size])[0]
        slots_pow = STATS_GEOMS[geom][2].bit_length() - 1
        seg = _segment(_packed(batch[0], batch[1] // LEN_MS), slots_pow, seg_bits)
        # The hot cells overflow their segments into the spill.
        assert np.bincount(seg).max() > cap + 5_000
    st = _stats_state(dev, geom, monkeypatch)
    _stats_insert(st, batch)
    _stats_check(st, ref)
    return st


def _lds_full_batch():
    """>= 200 distinct cells of one seg_bits-6 segment of a 2^14-slot
    table, each hit three times with different values, in 250,000
    uniform events that make the per-segment capacity large enough for
    none of them to spill."""
    rng = np.random.default_rng(400)
    ck = np.tile(np.arange(40_000, dtype=np.int64), 2)
    cw = np.repeat(np.arange(2), 40_000)
    seg6 = _segment(_packed(ck, cw), 14, 6)
    target = int(_segment(_packed(12_345, 0), 14, 6)[0])
    hit = np.flatnonzero(seg6 == target)[:230]
    assert hit.size >= 200
    fk = np.repeat(ck[hit], 3).astype(np.int32)
    fx = np.repeat(cw[hit], 3) * LEN_MS + rng.integers(0, LEN_MS, fk.size)
    fv = rng.integers(-(1 << 45), 1 << 45, fk.size)
    uk, ux, uv = _uniform_stats(250_000, 401, n_keys=1_500, n_win=2)
    keys = np.concatenate([fk, uk])
    x = np.concatenate([fx, ux])
    vals = np.concatenate([fv, uv])
    perm = rng.permutation(keys.size)
    return keys[perm], x[perm], vals[perm]


def _case_stats_lds_full(dev, geom, monkeypatch):
    batch, ref = _cached(
        "stats_lds_full",
        lambda: (lambda b: (b, _ref_stats(*b)))(_lds_full_batch()),
    )
    assert len(ref) < (1 << 14) // 2  # the table as a whole has room
    if geom in ("rb4", "rb4_fixed"):
        kind, seg_bits, nseg, cap = _plan_for(geom, [batch[0].size])[0]
        assert seg_bits == STATS_GEOMS[geom][3]
        wins = batch[1] // LEN_MS
        seg = _segment(_packed(batch[0], wins), 14, seg_bits)
        cells = np.unique(
            np.stack([seg, batch[0].astype(np.int64), wins], axis=1), axis=0
        )
        distinct = np.bincount(cells[:, 0], minlength=nseg)
        load = np.bincount(seg, minlength=nseg)
        full = distinct > (1 << seg_bits)
        # Some segment holds more distinct cells than LDS slots, and
        # all its events fit the segment, so they reach the LDS loop.
        assert full.any()
        assert (_cursor_bound(kind, batch[0].size, load[full]) <= cap).all()
    st = _stats_state(dev, geom, monkeypatch)
    _stats_insert(st, batch)
    _stats_check(st, ref)


def _edge_batch():
    rng = np.random.default_rng(500)
    cells = [
        # (key, window, values)
        (-1, 0, [I64_MIN]),
        (-2, 0, [I64_MAX]),
        (I32_MIN, 1, [0]),
        (I32_MAX, 1, [-1]),
        (0, 0, [I64_MIN, I64_MAX, 0, -1, 7]),
        (5, 2, [I64_MAX, I64_MAX, 1]),  # sum wraps upwards
        (6, 2, [I64_MIN, I64_MIN, -1]),  # and downwards
        (-1, 2, [3, -4, 0]),
        (I32_MIN, 0, [I64_MAX, I64_MIN]),
        (I32_MAX, 2, [I64_MIN, 1]),
        (0, 2, [0, 0]),
        (9, 1, [12]),  # min == max == the one value
    ]
    keys, x, vals = [], [], []
    for k, w, vs in cells:
        for v in vs:
            keys.append(k)
            x.append(w * LEN_MS + int(rng.integers(0, LEN_MS)))
            vals.append(v)
    uk, ux, uv = _uniform_stats(500, 501, n_keys=40)
    uk = uk + 1_000  # ordinary cells, apart from the ones above
    keys = np.concatenate([np.array(keys, dtype=np.int32), uk])
    x = np.concatenate([np.array(x, dtype=np.int64), ux])
    vals = np.concatenate([np.array(vals, dtype=np.int64), uv])
    perm = rng.permutation(keys.size)
    return keys[perm], x[perm], vals[perm]


def _case_stats_edges(dev, geom, ts_form, monkeypatch):
    batch, ref = _cached(
        "stats_edges", lambda: (lambda b: (b, _ref_stats(*b)))(_edge_batch())
    )
    assert ref[(5, 2)][1] == -1  # 2^64 - 1, wrapped
    assert ref[(6, 2)][1] == -1  # -2^64 - 1, wrapped
    assert ref[(-2, 0)] == (1, I64_MAX, I64_MAX, I64_MAX)
    assert ref[(-1, 0)] == (1, I64_MIN, I64_MIN, I64_MIN)
    assert ref[(9, 1)] == (1, 12, 12, 12)
    st = _stats_state(dev, geom, monkeypatch)
    _stats_insert(st, batch, ts_form)
    _stats_check(st, ref)
    return st


def _horizon_inputs():
    rng = np.random.default_rng(600)
    first = _uniform_stats(6_000, 601, n_keys=200, n_win=6)
    k2, _x, v2 = _uniform_stats(4_000, 602, n_keys=200)
    x2 = rng.integers(3 * LEN_MS, 8 * LEN_MS, 4_000)
    return first, (k2, x2, v2)


def _case_stats_horizon(dev, geom, monkeypatch):
    first, second = _cached("stats_horizon", _horizon_inputs)
    ref1 = _ref_stats(*first)
    ref_all = _ref_stats(*_cat([first, second]))
    st = _stats_state(dev, geom, monkeypatch)
    _stats_insert(st, first)
    closed = _got_stats(st.extract(horizon=3, clear=False))
    assert closed == {c: v for c, v in ref1.items() if c[1] < 3}
    # Extraction does not mutate the table.
    assert _got_stats(st.extract(horizon=3, clear=False)) == closed
    st.closed_horizon = 3
    _stats_insert(st, second, "delta")
    rest = _got_stats(st.extract(clear=False))
    assert rest == {c: v for c, v in ref_all.items() if c[1] >= 3}
    assert _got_stats(st.extract(clear=False)) == rest
    assert not set(closed) & set(rest)
    union = dict(closed)
    union.update(rest)
    assert union == ref_all  # nothing lost either
    if not st.cpu:
        assert int(st.error_flag.item()) == 0


def _case_stats_snapshot(dev, monkeypatch):
    """A radix state that took the hot and the edge inputs, restored
    into a fresh radix and a fresh direct state; all three go on."""
    hot = _cached("stats_hot3_b", lambda: _hot_batch(3, 300))
    edge = _cached("stats_edge_b", _edge_batch)
    more = _cached("stats_more_b", lambda: _uniform_stats(5_000, 700, n_keys=60))
    ref = _ref_stats(*_cat([hot, edge, more]))
    a = _stats_state(dev, "rb4", monkeypatch)
    _stats_insert(a, hot)
    _stats_insert(a, edge, "delta")
    snap = a.snapshot_to_host()
    assert snap["n"] == len(_ref_stats(*_cat([hot, edge])))
    for geom in ("rb4", "direct"):
        b = _stats_state(dev, geom, monkeypatch)
        b.restore_from_host(snap)
        _stats_insert(b, more)
        _stats_check(b, ref)
    _select(monkeypatch, {})
    _stats_insert(a, more)
    _stats_check(a, ref)


def _rows_of(ref):
    cells = list(ref.items())
    return {
        "keys": np.array([c[0] for c, _ in cells], dtype=np.int32),
        "wins": np.array([c[1] for c, _ in cells], dtype=np.int32),
        "cnt": np.array([v[0] for _, v in cells], dtype=np.int64),
        "sum": np.array([v[1] for _, v in cells], dtype=np.int64),
        "min": np.array([v[2] for _, v in cells], dtype=np.int64),
        "max": np.array([v[3] for _, v in cells], dtype=np.int64),
    }


def _case_stats_merge_rows(dev, geom, monkeypatch):
    """Rows of two donors that share cells with each other (the same
    cell twice in one call) and with the occupied table."""
    live = _uniform_stats(3_000, 800, n_keys=50)
    d1 = _uniform_stats(2_000, 801, n_keys=70)
    d2 = _cached("stats_edge_b", _edge_batch)
    d3 = _uniform_stats(2_000, 803, n_keys=70)
    rows = [_rows_of(_ref_stats(*d)) for d in (d1, d2, d3)]
    snap = {name: np.concatenate([r[name] for r in rows]) for name in rows[0]}
    cells = list(zip(snap["keys"].tolist(), snap["wins"].tolist()))
    assert len(set(cells)) < len(cells)  # duplicate rows
    assert set(cells) & set(_ref_stats(*live))  # occupied cells
    st = _stats_state(dev, geom, monkeypatch)
    _stats_insert(st, live)
    st.merge_rows(snap)
    _stats_check(st, _ref_stats(*_cat([live, d1, d2, d3])))


# -- stats: the CPU twin against the reference -------------------------


@pytest.mark.parametrize("ts_form", ["abs", "delta"])
def test_stats_twin_sizes(ts_form, monkeypatch):
    _case_stats_sizes(CPU, "rb4", ts_form, monkeypatch)


def test_stats_twin_cases(monkeypatch):
    _case_stats_accumulate(CPU, "rb4", monkeypatch)
    _case_stats_hot(CPU, "rb4", 1, monkeypatch)
    _case_stats_hot(CPU, "rb4_fixed", 3, monkeypatch)
    _case_stats_lds_full(CPU, "rb4", monkeypatch)
    _case_stats_lds_full(CPU, "rb4_fixed", monkeypatch)
    _case_stats_edges(CPU, "rb4", "abs", monkeypatch)
    _case_stats_edges(CPU, "rb4", "delta", monkeypatch)
    _case_stats_horizon(CPU, "rb4", monkeypatch)
    _case_stats_snapshot(CPU, monkeypatch)
    _case_stats_merge_rows(CPU, "rb4", monkeypatch)


def test_stats_plans_of_the_geometries():
    """The ladder of `radix_stats_insert_impl`, from the host copy: what
    each geometry is meant to reach for a batch of 8,192 events."""
    big = {g: _plan_for(g, [8_192])[0] for g in STATS_GEOMS if g != "direct"}
    assert big["rb4"][:3] == ("staged", 6, 256)
    assert big["rb4_fixed"][:3] == ("fixed", 4, 1024)
    # seg_bits 12 and 14 come down to 11 one coarse bit at a time.
    assert big["rb10"][:3] == ("staged", 11, 512)
    assert big["rb10_c4"][:3] == ("staged", 11, 512)
    assert all(p[3] >= SC_GRAN for p in big.values())
    # One event: the buffers give fewer than SC_GRAN entries per segment.
    assert _plan_for("rb4", [1])[0] == ("fixed", 4, 1024, 1)
    assert _plan_for("rb10", [1])[0] == ("fixed", 10, 1024, 1)


# -- stats: device -----------------------------------------------------

GEOMS = list(STATS_GEOMS)


@pytest.mark.gpu
@pytest.mark.parametrize("ts_form", ["abs", "delta"])
@pytest.mark.parametrize("geom", GEOMS)
def test_stats_sizes(geom, ts_form, monkeypatch):
    _case_stats_sizes(_gpu(), geom, ts_form, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("geom", GEOMS)
def test_stats_accumulate(geom, monkeypatch):
    _case_stats_accumulate(_gpu(), geom, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("n_cells", [1, 3])
@pytest.mark.parametrize("geom", GEOMS)
def test_stats_hot_cells(geom, n_cells, monkeypatch):
    _case_stats_hot(_gpu(), geom, n_cells, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("geom", GEOMS)
def test_stats_lds_full(geom, monkeypatch):
    _case_stats_lds_full(_gpu(), geom, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("ts_form", ["abs", "delta"])
@pytest.mark.parametrize("geom", GEOMS)
def test_stats_edges(geom, ts_form, monkeypatch):
    _case_stats_edges(_gpu(), geom, ts_form, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("geom", GEOMS)
def test_stats_horizon(geom, monkeypatch):
    _case_stats_horizon(_gpu(), geom, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("ts_form", ["abs", "delta"])
@pytest.mark.parametrize("geom", GEOMS)
def test_stats_max_ts(geom, ts_form, monkeypatch):
    """`max_ts_dev` is the batch maximum after the first insert and
    the running maximum afterwards."""
    st = _stats_state(_gpu(), geom, monkeypatch)
    k, x, v = _uniform_stats(5_000, 900)
    running = 0
    for lo, hi in ((LEN_MS, 2 * LEN_MS), (0, LEN_MS), (2 * LEN_MS, 3 * LEN_MS)):
        xb = lo + x % (hi - lo)
        _stats_insert(st, (k, xb, v), ts_form)
        running = max(running, ALIGN_MS + int(xb.max()))
        assert int(st.max_ts_dev.item()) == running
    assert int(st.error_flag.item()) == 0


@pytest.mark.gpu
def test_stats_snapshot_restore(monkeypatch):
    _case_stats_snapshot(_gpu(), monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("geom", ["rb4", "direct"])
def test_stats_merge_rows(geom, monkeypatch):
    _case_stats_merge_rows(_gpu(), geom, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("geom", ["rb4", "direct"])
def test_stats_out_cap_is_reported(geom, monkeypatch):
    batch = _uniform_stats(3_000, 1_000)
    assert len(_ref_stats(*batch)) > 64
    st = _stats_state(_gpu(), geom, monkeypatch, out_cap=64)
    _stats_insert(st, batch)
    with pytest.raises(RuntimeError, match="out_cap"):
        st.extract()


@pytest.mark.gpu
def test_stats_table_overflow_is_reported(monkeypatch):
    _select(monkeypatch, {})
    batch = _uniform_stats(6_000, 1_001, n_keys=2_000)
    assert len(_ref_stats(*batch)) > 1 << 10
    st = StatsAggState(
        _gpu(), ALIGN_MS, LEN_MS, slots_pow=10, out_cap=1 << 12, radix=False
    )
    assert st.nslots == 1 << 10
    _stats_insert(st, batch)
    with pytest.raises(RuntimeError, match="overflowed"):
        st.extract()


# -- join model --------------------------------------------------------


def _groups(keys, vals):
    """{key: (count, set of values)} of one batch."""
    keys = np.asarray(keys, dtype=np.int64)
    vals = np.asarray(vals, dtype=np.int64)
    order = np.argsort(keys, kind="stable")
    k, v = keys[order], vals[order]
    first = np.flatnonzero(np.r_[True, k[1:] != k[:-1]])
    ends = np.r_[first[1:], k.size]
    return {
        int(k[a]): (int(b - a), set(v[a:b].tolist()))
        for a, b in zip(first, ends)
    }


class JoinModel:
    """Per key: the flag states the documented semantics allow, each
    with the number of rows emitted since the last drain, and the
    values each side's cell may hold.

    One `insert` call on side `s` with `c` events of a key in state
    `f`: when `f` has the other side, exactly one row comes out and
    the flags end at 0 (`c == 1`), at ``1 << s`` (`c >= 2`, kernel
    that collapses the key's events before the table) or at either of
    the two (`c >= 2`, per-event kernels, where the race between the
    clearing event and its duplicates is unspecified); otherwise the
    flags become ``f | 1 << s``.
    """

    def __init__(self):
        self.hyps = {}  # key -> {(flags, rows since drain)}
        self.vals = {}  # key -> [values side 0 may hold, side 1]
        self.pend = {}  # key -> [(v0 set, v1 set)] of possible rows

    def insert(self, side, keys, vals, exact=lambda key: True):
        for key, (c, vs) in _groups(keys, vals).items():
            cell = self.vals.setdefault(key, [set(), set()])
            cell[side] = vs
            new = set()
            may_emit = False
            for f, r in self.hyps.get(key, {(0, 0)}):
                if f & (2 >> side):
                    may_emit = True
                    if c == 1:
                        new.add((0, r + 1))
                    else:
                        new.add((1 << side, r + 1))
                        if not exact(key):
                            new.add((0, r + 1))
                else:
                    new.add((f | 1 << side, r))
            self.hyps[key] = new
            if may_emit:
                self.pend.setdefault(key, []).append(
                    (set(cell[0]), set(cell[1]))
                )

    def check_rows(self, rows):
        """`rows`: every (key, v0, v1) drained since the last call."""
        by_key = {}
        for k, v0, v1 in rows:
            by_key.setdefault(k, []).append((v0, v1))
        assert set(by_key) <= set(self.hyps), "row for a key never inserted"
        for key, hyps in self.hyps.items():
            got = by_key.get(key, [])
            keep = {(f, 0) for f, r in hyps if r == len(got)}
            assert keep, (
                f"key {key}: {len(got)} rows, allowed "
                f"{sorted({r for _f, r in hyps})}"
            )
            self.hyps[key] = keep
            pend = self.pend.pop(key, [])
            assert len(got) <= len(pend)
            if len(got) == len(pend):
                # Every possible row came: they match one to one (at
                # most three per key per drain in these cases).
                assert _matches(got, pend), f"key {key}: rows {got}"
            else:
                for v0, v1 in got:
                    assert any(v0 in a and v1 in b for a, b in pend)

    def check_snapshot(self, snap):
        """Exactly the live half-pairs, with an allowed flag value and
        a value the set side may hold.  Narrows the model to what the
        snapshot shows."""
        assert not any(r for h in self.hyps.values() for _f, r in h), (
            "drain before a snapshot"
        )
        keys = snap["keys"].tolist()
        assert len(set(keys)) == len(keys), "key twice in the snapshot"
        seen = dict(
            zip(
                keys,
                zip(
                    snap["flags"].tolist(),
                    snap["v0"].tolist(),
                    snap["v1"].tolist(),
                ),
            )
        )
        assert set(seen) <= set(self.hyps)
        for key, hyps in self.hyps.items():
            flags, v0, v1 = seen.get(key, (0, None, None))
            assert (flags, 0) in hyps, (
                f"key {key}: flags {flags}, allowed {sorted(hyps)}"
            )
            self.hyps[key] = {(flags, 0)}
            if flags & 1:
                assert v0 in self.vals[key][0]
            if flags & 2:
                assert v1 in self.vals[key][1]

    def live(self):
        """{key: flags} where the model is certain."""
        out = {}
        for key, hyps in self.hyps.items():
            assert len(hyps) == 1
            ((f, _r),) = hyps
            if f:
                out[key] = f
        return out


def _matches(rows, pend):
    if not rows:
        return True
    v0, v1 = rows[0]
    return any(
        v0 in a and v1 in b and _matches(rows[1:], pend[:i] + pend[i + 1:])
        for i, (a, b) in enumerate(pend)
    )


def _drain(st):
    out = st.take_joined()
    if out is None:
        return []
    k, v0, v1 = (t.cpu().tolist() for t in out)
    return list(zip(k, v0, v1))


# name -> (constructor arguments, knobs, collapses duplicates in LDS)
JOIN_VARIANTS = {
    "coarse0": (dict(region_bits=4), {"BYTEWAX_JOIN_COARSE": "0"}, True),
    "default": (dict(region_bits=4), {}, True),
    "coarse3": (dict(region_bits=4), {"BYTEWAX_JOIN_COARSE": "3"}, True),
    "fixed": (dict(region_bits=4), {"BYTEWAX_SCATTER": "fixed"}, True),
    "nolds": (dict(region_bits=4), {"BYTEWAX_JOIN_LDS": "0"}, False),
    "t256": (dict(region_bits=4), {"BYTEWAX_JOIN_THREADS": "256"}, True),
    "t512": (dict(region_bits=4), {"BYTEWAX_JOIN_THREADS": "512"}, True),
    "direct": (dict(radix=False, slots_pow=14), {}, False),
    "lds160": (
        dict(region_bits=4, slots_pow=16), {"BYTEWAX_JOIN_COARSE": "0"}, True,
    ),
    "lds_full": (
        dict(region_bits=11), {"BYTEWAX_JOIN_COARSE": "2"}, True,
    ),
}
SMALL_VARIANTS = [v for v in JOIN_VARIANTS if v not in ("lds160", "lds_full")]


def _variant_geom(variant):
    kw, env, lds = JOIN_VARIANTS[variant]
    radix = kw.get("radix", True)
    rb = kw.get("region_bits", 11)
    slots_pow = kw.get("slots_pow", 10)
    if radix:
        slots_pow = max(slots_pow, rb + 10)
    return radix, rb, slots_pow, env, lds


class JoinRun:
    """One state and its model, fed the same calls.  Before each
    device insert the host hash shows that no region overfills and
    says which keys the LDS kernel collapses exactly."""

    def __init__(self, dev, variant, monkeypatch, out_cap=1 << 15):
        kw, env, _lds = JOIN_VARIANTS[variant]
        _select(monkeypatch, env)
        args = dict(slots_pow=10, out_cap=out_cap, radix=True)
        args.update(kw)
        self.st = HashJoinState(dev, **args)
        self.variant = variant
        self.model = JoinModel()
        self.sizes = []
        self.plans = []
        self.exact_dups = 0  # duplicated keys held to the exact rule
        self.all_keys = np.zeros(0, dtype=np.int64)
        radix, rb, slots_pow, _env, _l = _variant_geom(variant)
        if not self.st.cpu:
            assert self.st.nslots == 1 << slots_pow

    def _exact(self, keys):
        """Keys whose events all reach one LDS table with room: their
        segment neither spills nor holds more distinct keys than LDS
        slots.  On the CPU twin (sequential) every key is exact."""
        if self.st.cpu:
            return lambda key: True
        radix, rb, slots_pow, env, lds = _variant_geom(self.variant)
        keys = np.asarray(keys, dtype=np.int64)
        self.all_keys = np.union1d(self.all_keys, keys)
        if not radix:
            # Whole-table probing: the table as a whole has room.
            assert self.all_keys.size <= (1 << slots_pow) // 2
            self.plans.append(None)
            return lambda key: False
        region = _segment(_packed(self.all_keys), slots_pow, rb)
        assert np.bincount(region).max() <= 1 << rb, "region overfull"
        self.sizes.append(keys.size)
        total = _rx_totals(self.sizes, (1 << slots_pow) >> rb)[-1]
        plan = _join_plan(total, slots_pow, rb, env)
        self.plans.append(plan)
        kind, seg_bits, nseg, cap, lds_slots = plan
        if not lds:
            return lambda key: False
        seg = _segment(_packed(keys), slots_pow, seg_bits)
        load = np.bincount(seg, minlength=nseg)
        useg = _segment(_packed(np.unique(keys)), slots_pow, seg_bits)
        distinct = np.bincount(useg, minlength=nseg)
        ok = (_cursor_bound(kind, keys.size, load) <= cap) & (
            distinct <= lds_slots
        )
        return lambda key: bool(
            ok[int(_segment(_packed(key), slots_pow, seg_bits)[0])]
        )

    def insert(self, side, keys, vals):
        exact = self._exact(keys)
        uniq, counts = np.unique(keys, return_counts=True)
        self.exact_dups += sum(exact(int(k)) for k in uniq[counts >= 2])
        self.model.insert(side, keys, vals, exact)
        dev = self.st.device
        self.st.insert(
            side,
            torch.from_numpy(np.asarray(keys, dtype=np.int32)).to(dev),
            torch.from_numpy(np.asarray(vals, dtype=np.int64)).to(dev),
        )

    def drain(self):
        rows = _drain(self.st)
        self.model.check_rows(rows)
        return rows

    def snapshot(self):
        snap = self.st.snapshot_to_host()
        self.model.check_snapshot(snap)
        if not self.st.cpu:
            assert int(self.st.error_flag.item()) == 0
        return snap


def _vocab(slots_pow, rb, n, seed, per_region=10):
    """`n` distinct keys, negative ones among them, at most
    `per_region` to a table region."""
    rng = np.random.default_rng(seed)
    cand = rng.permutation(np.arange(-30_000, 30_000, dtype=np.int64))
    region = _segment(_packed(cand), slots_pow, rb)
    order = np.argsort(region, kind="stable")
    sr = region[order]
    first = np.flatnonzero(np.r_[True, sr[1:] != sr[:-1]])
    rank = np.arange(sr.size) - np.repeat(first, np.diff(np.r_[first, sr.size]))
    keep = np.sort(order[rank < per_region])
    out = cand[keep][:n]
    assert out.size == n
    return out


def _vocab_for(variant, n, seed=1):
    radix, rb, slots_pow, _env, _lds = _variant_geom(variant)
    return _vocab(slots_pow, rb if radix else 4, n, seed)


def _draw(vocab, n, rng):
    """`n` events over `vocab`: every key once while they last, the
    rest duplicates."""
    head = rng.permutation(vocab)[: min(n, vocab.size)]
    tail = vocab[rng.integers(0, vocab.size, n - head.size)]
    keys = rng.permutation(np.concatenate([head, tail]))
    return keys, rng.integers(-(1 << 60), 1 << 60, n)


# -- join case bodies --------------------------------------------------


def _case_join_sizes(dev, variant, monkeypatch):
    vocab = _vocab_for(variant, 4_000)
    for n in SIZES:
        rng = np.random.default_rng(1_100 + n % 89)
        run = JoinRun(dev, variant, monkeypatch)
        run.insert(0, *_draw(vocab, n, rng))
        assert run.drain() == []
        run.insert(1, *_draw(vocab, n, rng))
        run.drain()
        run.snapshot()


def _staged_threshold(variant):
    """Smallest first batch whose buffers give every segment SC_GRAN
    entries, from the sizing formula of `HashJoinState.insert`."""
    _radix, rb, slots_pow, env, _lds = _variant_geom(variant)
    n_regions = (1 << slots_pow) >> rb
    n = 1
    while _join_plan(_rx_totals([n], n_regions)[0], slots_pow, rb, env)[0] != "staged":
        n += 1
    return n


def _case_join_order(dev, variant, small_first, monkeypatch):
    vocab = _vocab_for(variant, 3_000)
    thr = _staged_threshold(variant)
    assert 500 < thr < 4_000  # roughly 1,000 events at 512 segments
    small, large = thr - 1, 8 * thr
    sizes = [small, large] if small_first else [large, small]
    rng = np.random.default_rng(1_200)
    run = JoinRun(dev, variant, monkeypatch)
    for i, n in enumerate(sizes + sizes):
        run.insert(i % 2, *_draw(vocab, n, rng))
        run.drain()
    run.snapshot()
    if dev.type != "cpu":
        kinds = [p[0] for p in run.plans[:2]]
        caps = [p[3] for p in run.plans[:2]]
        if small_first:
            # Below the threshold the fixed scatter, above it staged.
            assert kinds == ["fixed", "staged"]
        else:
            # The small batch inherits the large one's buffers.
            assert kinds == ["staged", "staged"]
            assert caps[1] == caps[0] >= 4 * SC_GRAN


def _case_join_accumulate(dev, variant, take_each, monkeypatch):
    """Five calls, alternating sides, singleton and duplicated keys,
    drained after every call or only once at the end."""
    vocab = _vocab_for(variant, 2_500)
    rng = np.random.default_rng(1_300)
    run = JoinRun(dev, variant, monkeypatch)
    for i in range(5):
        single = rng.permutation(vocab)[:1_400]
        dup = np.repeat(
            rng.permutation(vocab[:300])[:120], np.arange(120) % 2 + 2
        )
        dup = dup[~np.isin(dup, single)]
        keys = rng.permutation(np.concatenate([single, dup]))
        run.insert(i % 2, keys, rng.integers(-(1 << 60), 1 << 60, keys.size))
        if take_each:
            run.drain()
    rows = run.drain()
    assert take_each or rows
    run.snapshot()
    if dev.type != "cpu" and JOIN_VARIANTS[variant][2]:
        # Duplicated keys whose segment neither spilled nor filled its
        # LDS were held to exactly `1 << side` (the lcnt >= 2 re-arm).
        assert run.exact_dups > 50


def _case_join_hot(dev, variant, n_hot, monkeypatch):
    """Side 0, side 1, side 0 with hot keys of 20,000 events per call
    among 2,000 singleton bystanders."""
    vocab = _vocab_for(variant, 2_000 + n_hot, seed=2)
    hot, by = vocab[:n_hot], vocab[n_hot:]
    rng = np.random.default_rng(1_400)
    run = JoinRun(dev, variant, monkeypatch)
    for side in (0, 1, 0):
        keys = rng.permutation(
            np.concatenate([hot[rng.integers(0, n_hot, 20_000)], by])
        )
        run.insert(side, keys, rng.integers(-(1 << 60), 1 << 60, keys.size))
        if dev.type != "cpu" and run.plans[-1] is not None:
            _kind, seg_bits, nseg, cap, _l = run.plans[-1]
            slots_pow = _variant_geom(variant)[2]
            load = np.bincount(_segment(_packed(keys), slots_pow, seg_bits))
            assert load.max() > cap + 1_000  # the hot keys spill
        rows = run.drain()
        if side == 1:
            # Every bystander completes exactly once, every hot key too.
            assert sorted(k for k, _a, _b in rows) == sorted(vocab.tolist())
    run.snapshot()


def _case_join_edges(dev, variant, monkeypatch):
    """Key and value edges as singletons, so rows are exact."""
    keys = np.array([-1, -2, I32_MIN, I32_MAX, 0, 11, 12, 13, 14, 15])
    v0 = np.array([I64_MIN, I64_MAX, 0, -1, I64_MAX, 0, 5, I64_MIN, -1, 0])
    v1 = np.array([I64_MAX, I64_MIN, -1, 0, 0, 0, I64_MIN, I64_MAX, 7, -1])
    radix, rb, slots_pow, _env, _lds = _variant_geom(variant)
    run = JoinRun(dev, variant, monkeypatch)
    run.insert(0, keys, v0)
    assert run.drain() == []
    snap = run.snapshot()
    assert sorted(snap["keys"].tolist()) == sorted(keys.tolist())
    assert (snap["flags"] == 1).all()
    assert dict(zip(snap["keys"].tolist(), snap["v0"].tolist())) == dict(
        zip(keys.tolist(), v0.tolist())
    )
    # Complete all but key 11, whose stored 0 stays a live half-pair.
    done = keys != 11
    run.insert(1, keys[done], v1[done])
    rows = run.drain()
    assert sorted(rows) == sorted(
        zip(keys[done].tolist(), v0[done].tolist(), v1[done].tolist())
    )
    snap = run.snapshot()
    assert (snap["keys"].tolist(), snap["v0"].tolist()) == ([11], [0])
    assert snap["flags"].tolist() == [1]
    # The same through a restore: nothing on restore, then (11, 0, 0).
    run2 = JoinRun(dev, variant, monkeypatch)
    run2.st.restore_from_host(snap)
    assert _drain(run2.st) == []
    run2.st.insert(
        1,
        torch.tensor([11], dtype=torch.int32).to(dev),
        torch.tensor([0], dtype=torch.int64).to(dev),
    )
    assert _drain(run2.st) == [(11, 0, 0)]
    assert run2.st.snapshot_to_host()["keys"].tolist() == []


def _case_join_snapshot(dev, variant, monkeypatch):
    """Side-0-only, side-1-only and just-completed keys."""
    vocab = _vocab_for(variant, 900, seed=3)
    a, b, c = vocab[:300], vocab[300:600], vocab[600:]
    rng = np.random.default_rng(1_500)
    val = lambda n: rng.integers(-(1 << 60), 1 << 60, n)  # noqa: E731
    run = JoinRun(dev, variant, monkeypatch)
    va, vb = val(300), val(300)
    run.insert(0, np.concatenate([a, c]), np.concatenate([va, val(300)]))
    run.insert(1, np.concatenate([b, c]), np.concatenate([vb, val(300)]))
    rows = run.drain()
    assert sorted(k for k, _x, _y in rows) == sorted(c.tolist())
    snap = run.snapshot()
    live = dict(zip(snap["keys"].tolist(), snap["flags"].tolist()))
    assert live == {**{int(k): 1 for k in a}, **{int(k): 2 for k in b}}
    cols = [snap[name].tolist() for name in ("keys", "flags", "v0", "v1")]
    got0 = {k: v0 for k, f, v0, _v1 in zip(*cols) if f == 1}
    got1 = {k: v1 for k, f, _v0, v1 in zip(*cols) if f == 2}
    assert got0 == dict(zip(a.tolist(), va.tolist()))
    assert got1 == dict(zip(b.tolist(), vb.tolist()))

    run2 = JoinRun(dev, variant, monkeypatch)
    run2.st.restore_from_host(snap)
    assert _drain(run2.st) == []  # a restore emits nothing
    run2.model = run.model  # the restored state continues the model
    if not run2.st.cpu:
        # The restore was one insert per side.
        run2.sizes = [a.size, b.size]
        run2.all_keys = np.union1d(a, b)
    wa, wb = val(300), val(300)
    run2.insert(1, np.concatenate([a, c]), np.concatenate([wa, val(300)]))
    run2.insert(0, b, wb)
    rows = run2.drain()
    assert sorted(rows) == sorted(
        list(zip(a.tolist(), va.tolist(), wa.tolist()))
        + list(zip(b.tolist(), wb.tolist(), vb.tolist()))
    )
    # ... and exactly once: the same calls again only re-open halves.
    run2.insert(1, a, wa)
    assert run2.drain() == []
    snap2 = run2.snapshot()
    assert sorted(snap2["keys"].tolist()) == sorted(a.tolist() + c.tolist())


# -- join: the CPU twin against the model ------------------------------


def test_join_model_documented_example():
    """The model on the sequences of `stream_join`'s documentation."""
    m = JoinModel()
    m.insert(0, [1, 2], [10, 20])
    m.check_rows([])
    m.insert(1, [2, 3], [200, 300])
    m.check_rows([(2, 20, 200)])
    with pytest.raises(AssertionError):
        m.check_rows([(2, 20, 200)])  # a pair completes once
    m.insert(0, [2], [21])
    m.check_rows([])
    assert m.live() == {1: 1, 2: 1, 3: 2}
    m.insert(1, [2, 2], [5, 6], exact=lambda k: True)
    m.check_rows([(2, 21, 6)])
    assert m.live()[2] == 2  # re-armed by the duplicate
    m.insert(0, [2], [1])
    with pytest.raises(AssertionError):
        m.check_rows([(2, 1, 7)])  # 7 was never stored for side 1


def test_join_twin_sizes(monkeypatch):
    _case_join_sizes(CPU, "default", monkeypatch)


@pytest.mark.parametrize("small_first", [True, False])
def test_join_twin_order(small_first, monkeypatch):
    _case_join_order(CPU, "default", small_first, monkeypatch)


@pytest.mark.parametrize("take_each", [True, False])
def test_join_twin_accumulate(take_each, monkeypatch):
    """`take_each=False` is the order in which a twin that completes
    pairs only when drained differs from the device."""
    _case_join_accumulate(CPU, "default", take_each, monkeypatch)


def test_join_twin_cases(monkeypatch):
    _case_join_hot(CPU, "default", 1, monkeypatch)
    _case_join_hot(CPU, "default", 3, monkeypatch)
    _case_join_edges(CPU, "default", monkeypatch)
    _case_join_snapshot(CPU, "default", monkeypatch)


def test_join_twin_several_inserts_before_one_drain():
    st = HashJoinState(CPU)
    t = lambda xs, dt: torch.tensor(xs, dtype=dt)  # noqa: E731
    st.insert(0, t([4], torch.int32), t([1], torch.int64))
    st.insert(1, t([4], torch.int32), t([2], torch.int64))  # completes
    st.insert(0, t([4], torch.int32), t([3], torch.int64))  # a new half
    assert _drain(st) == [(4, 1, 2)]
    snap = st.snapshot_to_host()
    assert (snap["keys"].tolist(), snap["v0"].tolist()) == ([4], [3])
    assert snap["flags"].tolist() == [1]


def _lds_full_inputs():
    """>= 4,500 distinct keys of one seg_bits-13 segment of the 2^21
    table plus 300 duplicates among them, and the duplicate-heavy
    warm-up batch that sizes the scatter buffers (their capacity
    follows the largest batch seen) so that none of them spills."""
    cand = np.arange(1, 1_400_000, dtype=np.int64)
    seg = _segment(_packed(cand), 21, 13)
    target = int(seg[0])
    focus = cand[seg == target][:4_600]
    assert focus.size >= 4_500
    warm = cand[seg != target][:1_000]
    return focus, warm


def _case_join_lds_full(dev, monkeypatch):
    focus, warm = _cached("join_lds_full", _lds_full_inputs)
    rng = np.random.default_rng(1_600)
    run = JoinRun(dev, "lds_full", monkeypatch)
    val = lambda n: rng.integers(-(1 << 60), 1 << 60, n)  # noqa: E731
    run.insert(0, np.tile(warm, 420), val(420_000))
    assert run.drain() == []
    for side in (0, 1):
        keys = rng.permutation(np.concatenate([focus, focus[:300]]))
        run.insert(side, keys, val(keys.size))
        if dev.type != "cpu":
            kind, seg_bits, nseg, cap, lds_slots = run.plans[-1]
            assert (kind, seg_bits, lds_slots) == ("staged", 13, 4_096)
            # One segment: more distinct keys than LDS slots, all of
            # its events within capacity, each region with room.
            assert np.unique(_segment(_packed(keys), 21, 13)).size == 1
            assert focus.size > lds_slots
            assert _cursor_bound(kind, keys.size, keys.size) <= cap
            assert np.bincount(_segment(_packed(focus), 21, 11)).max() <= 2_048
        rows = run.drain()
        if side == 1:
            assert sorted(k for k, _a, _b in rows) == sorted(focus.tolist())
    run.snapshot()


def test_join_twin_lds_full(monkeypatch):
    _case_join_lds_full(CPU, monkeypatch)


def test_join_plans_of_the_variants():
    """The scatter choice of `radix_join_insert`, from the host copy."""
    def plan(variant, n):
        _r, rb, slots_pow, env, _l = _variant_geom(variant)
        total = _rx_totals([n], (1 << slots_pow) >> rb)[0]
        return _join_plan(total, slots_pow, rb, env)

    assert plan("default", 8_192)[:3] == ("staged", 5, 512)
    assert plan("coarse0", 8_192)[:3] == ("staged", 4, 1_024)
    assert plan("coarse3", 8_192)[:3] == ("staged", 7, 128)
    assert plan("fixed", 8_192)[0] == "fixed"
    assert plan("default", 64)[0] == "fixed"  # cap < SC_GRAN
    # 4,096 segments: the staged scatter's LDS exceeds 160 KiB.
    assert _staged_lds(4_096) > 160 * 1024
    assert plan("lds160", 3 * 8_192 + 1)[:3] == ("fixed", 4, 4_096)
    assert plan("lds_full", 420_000)[:3] == ("staged", 13, 256)
    assert plan("lds_full", 420_000)[4] == 4_096  # the 12-bit clamp


# -- join: device ------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("variant", SMALL_VARIANTS + ["lds160"])
def test_join_sizes(variant, monkeypatch):
    _case_join_sizes(_gpu(), variant, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("small_first", [True, False])
@pytest.mark.parametrize("variant", ["default", "coarse0", "nolds", "t256"])
def test_join_order(variant, small_first, monkeypatch):
    _case_join_order(_gpu(), variant, small_first, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("take_each", [True, False])
@pytest.mark.parametrize("variant", SMALL_VARIANTS + ["lds160"])
def test_join_accumulate(variant, take_each, monkeypatch):
    _case_join_accumulate(_gpu(), variant, take_each, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("n_hot", [1, 3])
@pytest.mark.parametrize("variant", SMALL_VARIANTS)
def test_join_hot_keys(variant, n_hot, monkeypatch):
    _case_join_hot(_gpu(), variant, n_hot, monkeypatch)


@pytest.mark.gpu
def test_join_lds_full(monkeypatch):
    _case_join_lds_full(_gpu(), monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", SMALL_VARIANTS + ["lds160"])
def test_join_edges(variant, monkeypatch):
    _case_join_edges(_gpu(), variant, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", SMALL_VARIANTS)
def test_join_snapshot_restore(variant, monkeypatch):
    _case_join_snapshot(_gpu(), variant, monkeypatch)


@pytest.mark.gpu
def test_join_one_segment_table(monkeypatch):
    """`nb < 1` in `radix_join_insert`: a table smaller than one
    scatter segment.  `HashJoinState` never builds one (it raises
    `slots_pow` to `region_bits + 10`), so the launcher is called on a
    16-slot table directly: region_bits 4 + coarse 1 > 4 bits."""
    dev = _gpu()
    _select(monkeypatch, {})
    st = HashJoinState(dev, slots_pow=10, out_cap=64, radix=True, region_bits=4)
    assert _join_plan(64, 4, 4, {})[1:3] == (4, 1)
    st.nslots = 16
    st.n_regions = 1
    st.tkeys = st.tkeys[:16].clone()
    st.tval0 = st.tval0[:16].clone()
    st.tval1 = st.tval1[:16].clone()
    st.tflags = st.tflags[:16].clone()
    st.rx_gcursors = st.rx_gcursors[:1].clone()
    keys = np.array([-1, 0, 3, 9, I32_MIN, 77, 78, 79, 80, 81, 82, 83])
    model = JoinModel()
    rng = np.random.default_rng(1_700)
    for side, sel in ((0, slice(0, 9)), (1, slice(3, 12)), (0, slice(0, 12))):
        k = np.concatenate([keys[sel], keys[sel][:2]])  # two duplicated
        v = rng.integers(-(1 << 60), 1 << 60, k.size)
        model.insert(side, k, v)
        st.insert(
            side,
            torch.from_numpy(k.astype(np.int32)).to(dev),
            torch.from_numpy(v).to(dev),
        )
        model.check_rows(_drain(st))
    model.check_snapshot(st.snapshot_to_host())
    assert int(st.error_flag.item()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["default", "nolds"])
def test_join_overfull_region_is_reported(variant, monkeypatch):
    cand = np.arange(0, 40_000, dtype=np.int64)
    region = _segment(_packed(cand), 14, 4)
    worst = int(np.bincount(region).argmax())
    keys = cand[region == worst][:24]
    assert keys.size > 16  # more distinct keys than the region's slots
    kw, env, _lds = JOIN_VARIANTS[variant]
    _select(monkeypatch, env)
    st = HashJoinState(_gpu(), slots_pow=10, out_cap=1 << 10, **kw)
    assert st.nslots == 1 << 14
    dev = st.device
    st.insert(
        0,
        torch.from_numpy(keys.astype(np.int32)).to(dev),
        torch.zeros(keys.size, dtype=torch.int64, device=dev),
    )
    with pytest.raises(RuntimeError, match="overflowed"):
        st.take_joined()


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["default", "direct"])
def test_join_out_cap_is_reported(variant, monkeypatch):
    vocab = _vocab_for(variant, 50)
    run = JoinRun(_gpu(), variant, monkeypatch, out_cap=8)
    vals = np.arange(50, dtype=np.int64)
    run.insert(0, vocab, vals)
    run.insert(1, vocab, vals)
    with pytest.raises(RuntimeError, match="out_cap"):
        run.st.take_joined()
