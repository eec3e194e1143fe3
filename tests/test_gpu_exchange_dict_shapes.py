"""Keyed exchange, filter compaction, the string dictionary and the
string exchange, at the shapes and edges where their kernels and host
twins can go wrong.

Every reference is exact (everything is integer, nothing has a
tolerance) and lives in this file: `_mix64`, `_fnv_rows` / `_fnv_bytes`
and `_hash128` are plain numpy / Python ports of the kernels' `mix64`
and `str_hash128`, checked against published FNV-1a vectors and a
pure-Python-integer form, and never imported from the package.  The
case bodies run unmarked against the CPU twins (`key_owner`,
`_bucket_cpu`, `StringDict(cpu)`, `_str_bucket_cpu`, `str_owner_cpu`)
and `gpu`-marked against the kernels.

The launchers use 256-thread blocks and at most 2,048 of them, so a
kernel's grid-stride loop runs a second time only above 524,288
elements: BIG is 524,288 + 321 (blocks 0 and 1 go round again, the
last wave holds one element).  The CPU twins have no such path; their
big cases are there for the batch shapes (one id, all ids distinct),
and `_str_bucket_cpu`, a Python loop per byte, stops at 5,000.

Rows are identified by their timestamp wherever a kernel may reorder
them: `ts` is a shifted `arange`, so "output row j is input row
`ts[j] - base` and carries its key / value / bytes, it sits in the
segment of that row's owner, and every input row occurs once" is the
per-segment multiset equality.  The keyed-exchange cases, whose `ts`
is random, compare sorted `(segment, key, ts, val)` rows instead.
The three checkers are themselves tested without a GPU: each takes a
twin's (for the filter, a numpy model's) output and must reject it
once rows are misrouted, reordered within a wave, lost, doubled or
altered, or a tail is written.

============================  =====================================
path                          case / host-side condition
============================  =====================================
`key_owner`, `_bucket_cpu`    `_owner_keys`: 0, 1, -1, -2, INT32_MIN,
(zero extension, unsigned     INT32_MAX and 4,096 random int32, about
modulo, multiplier)           half negative (asserted); worlds 1, 2,
                              3, 5, 7, 8, 13, 257
k_bucket_hist LDS init /      world 257 > 256 threads: the
flush loops                   `w += blockDim.x` loops run twice
k_bucket_hist /               BIG; `skew`: one key, one destination
k_bucket_scatter grid         (asserted from the port), every atomic
stride, atomics               of the batch on one counter
k_bucket_scatter<int32_t>     `ts32`
`vals == nullptr`             `vals=False` (zero-length `out_vals`)
launch skipped                n == 0: prefilled outputs untouched
k_filter_compact `i - lane    BIG: 524,609 % 64 == 1 (asserted), the
< n`, `i < n`                 last wave has one live lane; sizes 1,
                              63, 65, 255, 257
ballot / rank / leader        `lane0` (leader is lane 0, rank 0),
                              `lane63` (leader is lane 63, `(1 <<
                              63) - 1` rank mask), `one` (all 64
                              bits), `zero` (`ball == 0` skip),
                              `single0` / `single63` (one survivor)
mask != 0                     uint8 masks holding 2 and 255; bool
k_dict_insert / lookup CAS    BIG copies of one string: one id, one
contention                    slot, every thread on one CAS word
k_dict_insert new-id          BIG distinct strings: BIG claims, ids a
readback                      permutation of 0..BIG-1
str_hash128 lengths           "", embedded NUL, trailing NUL,
                              prefixes, multi-byte UTF-8, 70,000 bytes
probe wrap at the last slot   `full table`: two strings whose home is
                              slot 2^p - 1 (asserted from the port);
                              the second lands in slot 0 (asserted on
                              the table)
DICT_ERR_FULL / MISS /        `full table` + 1; `new_cap` + 1;
NEWCAP, priority              restore of 2^p + 1 strings
k_dict_insert_pinned          restore of exactly 2^p strings;
                              non-identity id permutation
`_encode_dev`                 device tensors in, both orders
k_str_bucket_hist /           BIG fixed-width strings; all strings
meta_scatter / byte_gather    identical (one destination, asserted);
                              all empty (zero bytes, null `bytes`);
                              70,000-byte strings among empty ones;
                              padded outputs keep their tails
============================  =====================================
"""

import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from bytewax_amd.gpu import RecordBatch, _bucket_cpu  # noqa: E402
from bytewax_amd.gpu.strings import (  # noqa: E402
    StringDict,
    _str_bucket_cpu,
    str_owner_cpu,
)

CPU = torch.device("cpu")
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
M64 = (1 << 64) - 1
BLOCK, MAX_BLOCKS, WAVE = 256, 2048, 64
BIG = BLOCK * MAX_BLOCKS + 321
SMALL = [0, 1, 63, 64, 65, 255, 256, 257]
WORLDS = [1, 2, 3, 5, 7, 8, 13, 257]
STR_WORLDS = [1, 2, 3, 5, 7, 8]
# Prefills of output buffers: a tail that still holds them was not
# written.
S32, S64, S8 = -1515870811, -6510615555426900571, 0xA5
PAD = 5
TS_BASE = 1_704_067_200_000


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _ext():
    from bytewax_amd.gpu import ext

    return ext()


# -- host hash ports ----------------------------------------------------


def _mix64(x):
    """The kernels' `mix64` (splitmix64 finalizer) on a uint64 array."""
    x = np.atleast_1d(np.asarray(x)).astype(np.uint64)
    x = x ^ (x >> np.uint64(33))
    x = x * np.uint64(0xFF51AFD7ED558CCD)
    x = x ^ (x >> np.uint64(33))
    x = x * np.uint64(0xC4CEB9FE1A85EC53)
    x = x ^ (x >> np.uint64(33))
    return x


def _owner(keys, world):
    """`mix64((uint32_t)key) % (uint64_t)world` of int32 keys."""
    k = np.ascontiguousarray(keys, dtype=np.int32).view(np.uint32)
    return (_mix64(k.astype(np.uint64)) % np.uint64(world)).astype(np.int64)


FNV_OFFSET, FNV_PRIME = 0xCBF29CE484222325, 0x100000001B3


def _fnv_bytes(b):
    """FNV-1a 64 of one byte string (Python integers)."""
    h = FNV_OFFSET
    for c in b:
        h = ((h ^ c) * FNV_PRIME) & M64
    return h


def _fnv_rows(mat):
    """FNV-1a 64 of every row of an (n, width) uint8 matrix."""
    h = np.full(mat.shape[0], FNV_OFFSET, dtype=np.uint64)
    for j in range(mat.shape[1]):
        h = (h ^ mat[:, j].astype(np.uint64)) * np.uint64(FNV_PRIME)
    return h


def _hash128(fnv):
    """`str_hash128` from the FNV state: (lo, hi) uint64 arrays."""
    fnv = np.atleast_1d(np.asarray(fnv, dtype=np.uint64))
    lo = _mix64(fnv ^ np.uint64(0x9E3779B97F4A7C15))
    lo = np.where(lo == np.uint64(M64), np.uint64(0), lo)
    hi = _mix64(fnv + np.uint64(0x2545F4914F6CDD1D))
    return lo, hi


def _hash128_list(bs):
    return _hash128(np.array([_fnv_bytes(b) for b in bs], dtype=np.uint64))


def _str_owner(hi, world):
    return (hi % np.uint64(world)).astype(np.int64)


def test_hash_ports_match_scalar_forms():
    def scalar(x):
        x ^= x >> 33
        x = (x * 0xFF51AFD7ED558CCD) & M64
        x ^= x >> 33
        x = (x * 0xC4CEB9FE1A85EC53) & M64
        x ^= x >> 33
        return x

    xs = [0, 1, 7, 0xFFFFFFFF, 0x80000000, M64 - 1, 1 << 63]
    assert [int(v) for v in _mix64(np.array(xs, dtype=np.uint64))] == [
        scalar(x) for x in xs
    ]
    assert scalar(1) == 12994781566227106604
    # Keys hash as uint32: -1 is 0xFFFFFFFF, INT32_MIN is 0x80000000.
    for key, u in ((-1, 0xFFFFFFFF), (I32_MIN, 0x80000000), (-2, 0xFFFFFFFE)):
        for world in (3, 8, 257):
            assert int(_owner([key], world)[0]) == scalar(u) % world
    # Published FNV-1a 64 vectors.
    assert _fnv_bytes(b"") == 0xCBF29CE484222325
    assert _fnv_bytes(b"a") == 0xAF63DC4C8601EC8C
    assert _fnv_bytes(b"foobar") == 0x85944171F73967E8
    mat = np.frombuffer(b"foobarfoobaz", dtype=np.uint8).reshape(2, 6)
    assert [int(v) for v in _fnv_rows(mat)] == [
        _fnv_bytes(b"foobar"), _fnv_bytes(b"foobaz"),
    ]
    h = _fnv_bytes(b"foobar")
    lo, hi = _hash128([h])
    assert int(lo[0]) == scalar(h ^ 0x9E3779B97F4A7C15)
    assert int(hi[0]) == scalar((h + 0x2545F4914F6CDD1D) & M64)


# -- shared inputs (computed once, read-only) ---------------------------


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _owner_keys():
    rng = np.random.default_rng(20240521)
    rnd = rng.integers(I32_MIN, I32_MAX + 1, size=4096, dtype=np.int64)
    edges = np.array([0, 1, -1, -2, I32_MIN, I32_MAX], dtype=np.int64)
    return _frozen(np.concatenate([edges, rnd]).astype(np.int32))


@functools.lru_cache(maxsize=None)
def _columns(n, seed=7):
    """(keys, ts64, ts32, vals) of a keyed batch: full-range keys with
    the edge keys first, random timestamps and extreme values."""
    rng = np.random.default_rng(seed + n)
    keys = rng.integers(I32_MIN, I32_MAX + 1, size=n, dtype=np.int64)
    edges = [0, 1, -1, -2, I32_MIN, I32_MAX]
    keys[: min(n, len(edges))] = edges[:n]
    ts32 = rng.integers(0, 1 << 20, size=n, dtype=np.int64).astype(np.int32)
    ts64 = TS_BASE + ts32.astype(np.int64)
    vals = rng.integers(-(1 << 62), 1 << 62, size=n, dtype=np.int64)
    ext = [-(1 << 63), (1 << 63) - 1, 0, -1]
    vals[: min(n, len(ext))] = ext[:n]
    return tuple(
        _frozen(a) for a in (keys.astype(np.int32), ts64, ts32, vals)
    )


@functools.lru_cache(maxsize=None)
def _fixed_mat(n, width=8):
    """n distinct fixed-width strings: row i spells i in base 16 with
    the letters a..p, lowest digit first."""
    idx = np.arange(n, dtype=np.int64)
    mat = np.empty((n, width), dtype=np.uint8)
    for j in range(width):
        mat[:, j] = 97 + ((idx >> (4 * j)) & 15)
    return _frozen(mat)


def _pack_bytes(bs):
    offs = np.zeros(len(bs) + 1, dtype=np.int64)
    if bs:
        np.cumsum([len(b) for b in bs], out=offs[1:])
    data = np.frombuffer(b"".join(bs), dtype=np.uint8).copy()
    return data, offs


def _pack_mat(mat):
    n, w = mat.shape
    return mat.reshape(-1).copy(), np.arange(n + 1, dtype=np.int64) * w


LONG = "z" * 69_999 + "y"  # 70,000 bytes
CONTENT = [
    "", "a", "ab", "abc", "a\x00", "a\x00\x00", "\x00", "\x00\x00",
    "x\x00y", "x\x00", "x", "é", "éé", "日本", "日本語", "😀", "e\u0301",
    LONG, LONG[:-1], LONG + "\x00",
]


def test_content_strings_are_what_the_table_says():
    assert len(set(CONTENT)) == len(CONTENT)
    assert len(LONG.encode()) == 70_000
    enc = [s.encode() for s in CONTENT]
    assert b"" in enc and b"a\x00" in enc and b"a" in enc
    assert any(len(s) < len(b) for s, b in zip(CONTENT, enc))  # multi-byte
    lo, hi = _hash128_list(enc)
    assert len(set(lo.tolist())) == len(enc)
    assert len(set(hi.tolist())) == len(enc)


# -- key owner ----------------------------------------------------------


@pytest.mark.parametrize("world", WORLDS)
def test_key_owner_matches_device_hash_port(world):
    from bytewax_amd.gpu import key_owner

    keys = _owner_keys()
    assert 1500 < int((keys < 0).sum()) < 2600
    got = key_owner(torch.from_numpy(keys.copy()), world)
    assert got.dtype == torch.int64 and got.shape == (len(keys),)
    ref = _owner(keys, world)
    diff = int((got.numpy() != ref).sum())
    nonneg = int((got.numpy() != ref)[keys >= 0].sum())
    assert diff == 0, (
        f"world {world}: {diff} of {len(keys)} owners differ from "
        f"mix64((uint32)k) % world ({nonneg} of them non-negative keys)"
    )
    assert int(ref.min()) >= 0 and int(ref.max()) < world


def test_key_owner_rejects_what_it_cannot_hash():
    from bytewax_amd.gpu import key_owner

    with pytest.raises(ValueError):
        key_owner(torch.zeros(3, dtype=torch.int32), 0)
    with pytest.raises(TypeError):
        key_owner(torch.zeros(3, dtype=torch.int64), 2)
    assert key_owner(torch.zeros(0, dtype=torch.int32), 3).numel() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("world", WORLDS)
def test_key_owner_is_where_bucket_hist_counts(world):
    from bytewax_amd.gpu import key_owner

    dev = _gpu()
    keys = torch.from_numpy(_owner_keys().copy())
    counts = torch.zeros(world, dtype=torch.int32, device=dev)
    _ext().bucket_hist(keys.to(dev), world, counts)
    own = key_owner(keys, world)
    assert torch.equal(own, key_owner(keys.to(dev), world))
    assert counts.cpu().tolist() == torch.bincount(
        own, minlength=world
    ).tolist()


# -- keyed exchange -----------------------------------------------------


def _sorted_rows(cols):
    cols = [np.asarray(c).astype(np.int64) for c in cols]
    order = np.lexsort(cols[::-1])
    return np.stack([c[order] for c in cols])


def _check_buckets(keys, ts, vals, world, got):
    """`got`: (counts, send_keys, send_ts, send_vals) as numpy."""
    counts, skeys, sts, svals = got
    own = _owner(keys, world)
    ref_counts = np.bincount(own, minlength=world)
    assert counts.tolist() == ref_counts.tolist()
    assert len(skeys) == len(sts) == len(keys)
    seg = np.repeat(np.arange(world), ref_counts)
    ref, out = [own, keys, ts], [seg, skeys, sts]
    if vals is not None:
        assert len(svals) == len(keys)
        ref.append(vals)
        out.append(svals)
    else:
        assert svals is None or len(svals) == 0
    assert np.array_equal(_sorted_rows(ref), _sorted_rows(out))


def _bucket_twin(keys, ts, vals, world):
    t = torch.from_numpy
    batch = RecordBatch(
        t(keys.copy()), t(ts.copy()),
        t(vals.copy()) if vals is not None else None,
    )
    counts, sk, st, sv = _bucket_cpu(batch, world)
    assert counts.dtype == torch.int32 and st.dtype == batch.ts.dtype
    return (
        counts.numpy(), sk.numpy(), st.numpy(),
        sv.numpy() if sv is not None else None,
    )


def _bucket_device(keys, ts, vals, world):
    dev, k = _gpu(), _ext()
    n = len(keys)
    d_keys = torch.from_numpy(keys.copy()).to(dev)
    d_ts = torch.from_numpy(ts.copy()).to(dev)
    d_vals = torch.from_numpy(vals.copy()).to(dev) if vals is not None else None
    counts = torch.zeros(world, dtype=torch.int32, device=dev)
    k.bucket_hist(d_keys, world, counts)
    cursors = (torch.cumsum(counts, 0, dtype=torch.int32) - counts).clone()
    out_keys = torch.full((n + PAD,), S32, dtype=torch.int32, device=dev)
    out_ts = torch.full(
        (n + PAD,), S32 if ts.dtype == np.int32 else S64,
        dtype=d_ts.dtype, device=dev,
    )
    out_vals = torch.full(
        (n + PAD if vals is not None else 0,), S64,
        dtype=torch.int64, device=dev,
    )
    k.bucket_scatter(
        d_keys, d_ts, d_vals, world, cursors, out_keys, out_ts, out_vals
    )
    c = counts.cpu().numpy()
    # Every cursor ends where the next segment begins.
    assert cursors.cpu().tolist() == np.cumsum(c).tolist()
    assert bool((out_keys[n:] == S32).all())
    assert bool((out_ts[n:] == out_ts[-1]).all()) and int(out_ts[-1]) in (
        S32, S64,
    )
    if vals is not None:
        assert bool((out_vals[n:] == S64).all())
    return (
        c, out_keys[:n].cpu().numpy(), out_ts[:n].cpu().numpy(),
        out_vals[:n].cpu().numpy() if vals is not None else None,
    )


def _bucket_case(run, n, world, has_vals, ts32):
    keys, ts64, t32, vals = _columns(n)
    ts = t32 if ts32 else ts64
    v = vals if has_vals else None
    _check_buckets(keys, ts, v, world, run(keys, ts, v, world))


COMBOS = [(True, False), (False, True), (True, True), (False, False)]


@pytest.mark.parametrize("world", WORLDS)
def test_bucket_twin_segments(world):
    for n in [*SMALL, 5000]:
        for has_vals, ts32 in COMBOS:
            _bucket_case(_bucket_twin, n, world, has_vals, ts32)


@pytest.mark.gpu
@pytest.mark.parametrize("world", WORLDS)
def test_bucket_kernels_small(world):
    for n in SMALL[1:]:
        for has_vals, ts32 in COMBOS:
            _bucket_case(_bucket_device, n, world, has_vals, ts32)


@pytest.mark.gpu
@pytest.mark.parametrize("world", WORLDS)
def test_bucket_kernels_big(world):
    assert BIG > BLOCK * MAX_BLOCKS  # the grid-stride loops go round
    for has_vals, ts32 in COMBOS[:2]:
        _bucket_case(_bucket_device, BIG, world, has_vals, ts32)


def test_bucket_checker_rejects_misrouted_and_altered_rows():
    world, n = 3, 257
    keys, ts, _t, vals = _columns(n)
    counts, sk, st, sv = _bucket_twin(keys, ts, vals, world)
    _check_buckets(keys, ts, vals, world, (counts, sk, st, sv))
    assert counts.min() > 0

    def rejected(*got):
        with pytest.raises(AssertionError):
            _check_buckets(keys, ts, vals, world, got)

    a, b = 0, n - 1  # rows of the first and the last segment, swapped
    mis = [x.copy() for x in (sk, st, sv)]
    for x in mis:
        x[[a, b]] = x[[b, a]]
    rejected(counts, *mis)
    v2 = sv.copy()
    v2[[a, a + 1]] = v2[[a + 1, a]]  # values of two rows exchanged
    assert v2[a] != sv[a]
    rejected(counts, sk, st, v2)
    t2 = st.copy()
    t2[5] = t2[6]  # one row lost, one doubled
    rejected(counts, sk, t2, sv)
    c2 = counts.copy()
    c2[0] += 1
    c2[1] -= 1
    rejected(c2, sk, st, sv)


def _skew(n):
    _k, ts64, _t, vals = _columns(n)
    return np.full(n, -1, dtype=np.int32), ts64, vals


@pytest.mark.parametrize("world", [1, 3, 257])
def test_bucket_twin_skew(world):
    keys, ts, vals = _skew(5000)
    assert len(set(_owner(keys, world).tolist())) == 1
    _check_buckets(keys, ts, vals, world, _bucket_twin(keys, ts, vals, world))


@pytest.mark.gpu
@pytest.mark.parametrize("world", [1, 3, 257])
def test_bucket_kernels_skew(world):
    keys, ts, vals = _skew(BIG)
    assert len(set(_owner(keys, world).tolist())) == 1
    _check_buckets(
        keys, ts, vals, world, _bucket_device(keys, ts, vals, world)
    )
    _check_buckets(
        keys, ts, None, world, _bucket_device(keys, ts, None, world)
    )


@pytest.mark.gpu
def test_bucket_kernels_empty_batch_touches_nothing():
    dev, k = _gpu(), _ext()
    world = 5
    keys = torch.zeros(0, dtype=torch.int32, device=dev)
    ts = torch.zeros(0, dtype=torch.int64, device=dev)
    vals = torch.zeros(0, dtype=torch.int64, device=dev)
    counts = torch.full((world,), 7, dtype=torch.int32, device=dev)
    cursors = torch.full((world,), 9, dtype=torch.int32, device=dev)
    out_keys = torch.full((PAD,), S32, dtype=torch.int32, device=dev)
    out_ts = torch.full((PAD,), S64, dtype=torch.int64, device=dev)
    out_vals = torch.full((PAD,), S64, dtype=torch.int64, device=dev)
    k.bucket_hist(keys, world, counts)
    k.bucket_scatter(keys, ts, vals, world, cursors, out_keys, out_ts, out_vals)
    assert counts.cpu().tolist() == [7] * world
    assert cursors.cpu().tolist() == [9] * world
    assert out_keys.cpu().tolist() == [S32] * PAD
    assert out_ts.cpu().tolist() == [S64] * PAD
    assert out_vals.cpu().tolist() == [S64] * PAD


# -- filter compaction --------------------------------------------------

MASKS = ["zero", "one", "random", "lane0", "lane63", "single0", "single63"]


def _mask(kind, n):
    m = np.zeros(n, dtype=bool)
    if kind == "one":
        m[:] = True
    elif kind == "random":
        m = np.random.default_rng(n + 3).random(n) < 0.5
    elif kind == "lane0":
        m[0::WAVE] = True
    elif kind == "lane63":
        m[WAVE - 1 :: WAVE] = True
    elif kind == "single0" and n:
        m[(n - 1) // WAVE * WAVE] = True  # lane 0 of the last wave
    elif kind == "single63" and n >= WAVE:
        m[n // WAVE * WAVE - 1] = True  # lane 63 of the last full wave
    return m


def test_filter_masks_are_what_their_names_say():
    for n in [*SMALL, BIG]:
        lane = np.arange(n) % WAVE
        assert set(lane[_mask("lane0", n)].tolist()) <= {0}
        assert set(lane[_mask("lane63", n)].tolist()) <= {63}
        assert int(_mask("single0", n).sum()) == (1 if n else 0)
        assert int(_mask("single63", n).sum()) == (1 if n >= WAVE else 0)
        assert set(lane[_mask("single0", n)].tolist()) <= {0}
        assert set(lane[_mask("single63", n)].tolist()) <= {63}
        assert not _mask("zero", n).any() and _mask("one", n).all()
    assert BIG % WAVE == 1  # the last wave of BIG has one live lane


def _check_filter(keys, vals, m, kept, out_keys, out_ts, out_vals):
    """Outputs as numpy, `PAD` longer than the input and prefilled;
    the input's `ts` is ``arange(n)``."""
    assert kept == int(m.sum())
    src = out_ts[:kept]
    # Every survivor once, with its own key and value; nothing else.
    assert np.array_equal(np.sort(src), np.flatnonzero(m))
    assert np.array_equal(out_keys[:kept], keys[src])
    assert (out_keys[kept:] == S32).all() and len(out_keys) == len(m) + PAD
    assert (out_ts[kept:] == S64).all() and len(out_ts) == len(m) + PAD
    if vals is not None:
        assert np.array_equal(out_vals[:kept], vals[src])
        assert (out_vals[kept:] == S64).all()
        assert len(out_vals) == len(m) + PAD
    else:
        assert len(out_vals) == 0
    if kept > 1:
        # The documented order: the survivors of a 64-aligned input
        # chunk are contiguous in the output and in input order.
        chunk = src // WAVE
        change = chunk[1:] != chunk[:-1]
        assert int(change.sum()) + 1 == len(np.unique(chunk))
        assert bool((np.diff(src)[~change] > 0).all())


def _filter_model(keys, vals, m, wave_order):
    """What the kernel may produce: waves reserve their output ranges
    in any order, each wave writes its survivors in lane order."""
    n = len(m)
    out_keys = np.full(n + PAD, S32, dtype=np.int32)
    out_ts = np.full(n + PAD, S64, dtype=np.int64)
    out_vals = np.full(n + PAD if vals is not None else 0, S64, dtype=np.int64)
    o = 0
    for w in wave_order:
        idx = np.flatnonzero(m[w * WAVE : (w + 1) * WAVE]) + w * WAVE
        out_keys[o : o + len(idx)] = keys[idx]
        out_ts[o : o + len(idx)] = idx
        if vals is not None:
            out_vals[o : o + len(idx)] = vals[idx]
        o += len(idx)
    return o, out_keys, out_ts, out_vals


def test_filter_checker_takes_any_wave_order_and_nothing_else():
    n = 5 * WAVE + 7
    keys, _ts, _t, vals = _columns(n)
    m = _mask("random", n)
    order = [3, 0, 5, 1, 4, 2]
    for v in (vals, None):
        _check_filter(keys, v, m, *_filter_model(keys, v, m, range(6)))
        _check_filter(keys, v, m, *_filter_model(keys, v, m, order))
    kept, ok, ot, ov = _filter_model(keys, vals, m, order)

    def rejected(kept, ok, ot, ov):
        with pytest.raises(AssertionError):
            _check_filter(keys, vals, m, kept, ok, ot, ov)

    swapped = ot.copy()  # two survivors of one wave out of input order
    swapped[[0, 1]] = swapped[[1, 0]]
    k2 = ok.copy()
    k2[[0, 1]] = k2[[1, 0]]
    v2 = ov.copy()
    v2[[0, 1]] = v2[[1, 0]]
    assert swapped[0] // WAVE == swapped[1] // WAVE
    rejected(kept, k2, swapped, v2)
    perm = np.argsort(ot[:kept] % WAVE, kind="stable")  # waves interleaved
    rejected(
        kept,
        np.concatenate([ok[:kept][perm], ok[kept:]]),
        np.concatenate([ot[:kept][perm], ot[kept:]]),
        np.concatenate([ov[:kept][perm], ov[kept:]]),
    )
    rejected(kept - 1, ok, ot, ov)  # a survivor dropped from the count
    dup = ot.copy()
    dup[1] = dup[0]
    rejected(kept, ok, dup, ov)  # one survivor twice, one lost
    wrong = ov.copy()
    wrong[kept - 1] ^= 1
    rejected(kept, ok, ot, wrong)  # another row's value
    spill = ok.copy()
    spill[kept] = 0
    rejected(kept, spill, ot, ov)  # a write past out_n


def _filter_case(n, kind, dtype, has_vals):
    dev, k = _gpu(), _ext()
    keys, _ts, _t, vals = _columns(n)
    m = _mask(kind, n)
    if dtype == "bool":
        d_mask = torch.from_numpy(m.copy()).to(dev)
    else:
        # "Kept" is any non-zero byte: 2 has bit 0 clear, 255 is -1.
        odd = np.arange(n) % 2 == 1
        d_mask = torch.from_numpy(
            np.where(m, np.where(odd, 255, 2), 0).astype(np.uint8)
        ).to(dev)
    d_keys = torch.from_numpy(keys.copy()).to(dev)
    d_ts = torch.arange(n, dtype=torch.int64, device=dev)
    d_vals = torch.from_numpy(vals.copy()).to(dev) if has_vals else None
    out_keys = torch.full((n + PAD,), S32, dtype=torch.int32, device=dev)
    out_ts = torch.full((n + PAD,), S64, dtype=torch.int64, device=dev)
    out_vals = torch.full(
        (n + PAD if has_vals else 0,), S64, dtype=torch.int64, device=dev
    )
    out_n = torch.zeros(1, dtype=torch.int32, device=dev)
    k.filter_compact(
        d_keys, d_ts, d_vals, d_mask, out_keys, out_ts, out_vals, out_n
    )
    _check_filter(
        keys, vals if has_vals else None, m, int(out_n.item()),
        out_keys.cpu().numpy(), out_ts.cpu().numpy(), out_vals.cpu().numpy(),
    )


@pytest.mark.gpu
@pytest.mark.parametrize("kind", MASKS)
def test_filter_compact_small(kind):
    for n in SMALL:
        for dtype in ("bool", "u8"):
            for has_vals in (False, True):
                _filter_case(n, kind, dtype, has_vals)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", MASKS)
def test_filter_compact_big(kind):
    _filter_case(BIG, kind, "bool", True)
    _filter_case(BIG, kind, "u8", False)


# -- string dictionary --------------------------------------------------


def _check_encode(d, batch, ids, seen):
    """The properties of one `encode`: ids of earlier batches are
    stable, all ids are dense 0..len-1, decode inverts encode.
    `seen` (str -> id) is carried across batches."""
    first_new = len(seen)
    got = ids.cpu().tolist()
    assert len(got) == len(batch)
    for s, i in zip(batch, got):
        if seen.setdefault(s, i) != i:
            msg = f"{s[:20]!r} had id {seen[s]}, now {i}"
            raise AssertionError(msg)
    assert sorted(seen.values()) == list(range(len(seen)))
    assert len(d) == len(seen)
    assert d.decode(ids) == list(batch)
    new = {i for s, i in seen.items() if i >= first_new}
    assert new == set(range(first_new, len(seen)))


def _dict_content_case(dev):
    d = StringDict(dev, slots_pow=10, new_cap=64)
    seen = {}
    one = ["solo\x00"]
    _check_encode(d, one, d.encode(one), seen)  # a batch of one
    assert seen == {"solo\x00": 0}
    batch = CONTENT + CONTENT[::-1] + ["", LONG]
    _check_encode(d, batch, d.encode(batch), seen)
    later = ["new", "a\x00\x00\x00", *CONTENT[::3], "solo", "solo\x00"]
    _check_encode(d, later, d.encode(later), seen)
    assert len(d) == len(CONTENT) + 4
    _check_encode(d, batch, d.encode(batch), seen)
    return d, seen


def test_dict_twin_content():
    _dict_content_case(CPU)


@pytest.mark.gpu
def test_dict_kernels_content():
    _dict_content_case(_gpu())


def _dict_big_repeat_case(dev):
    # Into an empty table: BIG threads race for one slot and one id.
    d = StringDict(dev, slots_pow=10, new_cap=64)
    s = "hot\x00key-é"
    ids = d.encode([s] * BIG)
    assert len(d) == 1 and d.id2str == [s]
    assert ids.shape == (BIG,) and bool((ids == 0).all())
    seen = {s: 0}
    later = ["cold", s, "colder"]
    _check_encode(d, later, d.encode(later), seen)
    # And again behind other ids: still one new id for the whole batch.
    t = "hot\x00key-é\x00"
    ids = d.encode([t] * BIG)
    assert len(d) == 4 and d.id2str[3] == t
    assert bool((ids == 3).all())
    seen[t] = 3
    _check_encode(d, [t, s, *later], d.encode([t, s, *later]), seen)


def test_dict_twin_big_batch_of_one_string():
    _dict_big_repeat_case(CPU)


@pytest.mark.gpu
def test_dict_kernels_big_batch_of_one_string():
    _dict_big_repeat_case(_gpu())


def _dict_big_distinct_case(dev):
    mat = _fixed_mat(BIG)
    d = StringDict(dev, slots_pow=21, new_cap=1 << 20)
    ids = d.encode(_pack_mat(mat)).cpu().numpy()
    assert len(d) == BIG
    assert np.array_equal(np.sort(ids), np.arange(BIG))
    # decode(encode(x)) == x for all of them at once: id2str, laid out
    # as a matrix and gathered by id, is the input.
    table = np.frombuffer(
        "".join(d.id2str).encode(), dtype=np.uint8
    ).reshape(BIG, mat.shape[1])
    assert np.array_equal(table[ids], mat)
    # Stable in a later batch (a slice, reversed, with one new string).
    sub = mat[::-1][: 3 * BLOCK + 1]
    strs = [bytes(r).decode() for r in sub] + ["brand new"]
    ids2 = d.encode(strs).cpu().numpy()
    assert np.array_equal(ids2[:-1], ids[::-1][: len(sub)])
    assert int(ids2[-1]) == BIG and len(d) == BIG + 1
    assert d.decode(ids2[-3:]) == strs[-3:]


def test_dict_twin_big_batch_of_distinct_strings():
    _dict_big_distinct_case(CPU)


@pytest.mark.gpu
def test_dict_kernels_big_batch_of_distinct_strings():
    _dict_big_distinct_case(_gpu())


def _dict_restore_case(dev):
    snap = {"strings": ["", "a\x00", "a", "日本", LONG]}
    d = StringDict(dev, slots_pow=6, new_cap=16)
    d.restore(snap)
    assert len(d) == 5
    seen = {s: i for i, s in enumerate(snap["strings"])}
    batch = ["new1", "a", "new2", "", LONG, "new1", "a\x00"]
    ids = d.encode(batch)
    _check_encode(d, batch, ids, seen)
    # New strings get ids from len(snapshot) on.
    assert {seen["new1"], seen["new2"]} == {5, 6}
    assert ids.cpu().tolist()[1] == 2 and ids.cpu().tolist()[4] == 4
    assert d.snapshot() == {"strings": d.id2str}
    with pytest.raises(RuntimeError, match="empty dictionary"):
        d.restore(snap)


def test_dict_twin_restore_then_new_ids():
    _dict_restore_case(CPU)


@pytest.mark.gpu
def test_dict_kernels_restore_then_new_ids():
    _dict_restore_case(_gpu())


@pytest.mark.gpu
def test_dict_device_tensor_input_matches_host_list_input():
    dev = _gpu()
    strs = [*CONTENT, *(f"w{i % 300}" for i in range(1000))]
    data, offs = _pack_bytes([s.encode() for s in strs])
    on_dev = (torch.from_numpy(data).to(dev), torch.from_numpy(offs).to(dev))
    # Host list first: the device-tensor batch adds nothing.
    d = StringDict(dev, slots_pow=12, new_cap=512)
    seen = {}
    ids_list = d.encode(strs)
    _check_encode(d, strs, ids_list, seen)
    assert torch.equal(d.encode(on_dev), ids_list)
    assert len(d) == len(seen)
    # Device tensors first: the new ids' strings come back from the
    # device bytes.
    d2 = StringDict(dev, slots_pow=12, new_cap=512)
    seen2 = {}
    ids_dev = d2.encode(on_dev)
    _check_encode(d2, strs, ids_dev, seen2)
    assert torch.equal(d2.encode(strs), ids_dev)
    # An empty device batch.
    empty = (
        torch.zeros(0, dtype=torch.uint8, device=dev),
        torch.zeros(1, dtype=torch.int64, device=dev),
    )
    assert d2.encode(empty).numel() == 0 and len(d2) == len(seen2)


def _full_table_strings(slots_pow):
    """2^p distinct strings, the first two with the last slot as home,
    and one more; plus the (lo, home) of each from the port."""
    nslots = 1 << slots_pow
    cand = [f"k{i}" for i in range(4000)]
    lo, _hi = _hash128_list([c.encode() for c in cand])
    assert len(set(lo.tolist())) == len(cand)
    home = (lo & np.uint64(nslots - 1)).astype(np.int64)
    last = [i for i in range(len(cand)) if home[i] == nslots - 1]
    assert len(last) >= 2
    rest = [i for i in range(len(cand)) if i not in last[:2]]
    pick = [*last[:2], *rest[: nslots - 1]]
    return [cand[i] for i in pick], lo[pick], home[pick]


@pytest.mark.gpu
@pytest.mark.parametrize("slots_pow", [4, 5, 6])
def test_dict_kernels_full_table_wraps_then_reports_full(slots_pow):
    dev = _gpu()
    nslots = 1 << slots_pow
    strs, lo, home = _full_table_strings(slots_pow)
    assert len(strs) == nslots + 1
    # The property this case is about, from the hash port: the second
    # string's home is the last slot, which the first one holds.
    assert home[0] == home[1] == nslots - 1 and lo[0] != lo[1]
    d = StringDict(dev, slots_pow=slots_pow, new_cap=nslots)
    seen = {}
    _check_encode(d, strs[:1], d.encode(strs[:1]), seen)
    _check_encode(d, strs[1:2], d.encode(strs[1:2]), seen)
    table = d.dlo.cpu().numpy().view(np.uint64)
    assert int(table[nslots - 1]) == int(lo[0])
    assert int(table[0]) == int(lo[1])  # wrapped
    assert int((table != np.uint64(M64)).sum()) == 2
    # Fill to exactly 100% in one batch, then resolve everything.
    fill = strs[2:nslots]
    _check_encode(d, fill, d.encode(fill), seen)
    table = d.dlo.cpu().numpy().view(np.uint64)
    assert sorted(table.tolist()) == sorted(lo[:nslots].tolist())
    every = strs[:nslots][::-1]
    _check_encode(d, every, d.encode(every), seen)
    assert len(d) == nslots
    with pytest.raises(RuntimeError, match="table full"):
        d.encode([strs[1], strs[nslots]])


@pytest.mark.gpu
def test_dict_kernels_new_cap_is_per_batch_and_reported():
    dev = _gpu()
    cap = 8
    d = StringDict(dev, slots_pow=10, new_cap=cap)
    seen = {}
    a = [f"a{i}" for i in range(cap)]
    _check_encode(d, a + a, d.encode(a + a), seen)
    b = [f"b{i}" for i in range(cap)]
    _check_encode(d, b + a, d.encode(b + a), seen)  # cap new ids again
    assert len(d) == 2 * cap
    d2 = StringDict(dev, slots_pow=10, new_cap=cap)
    with pytest.raises(RuntimeError, match="new_cap"):
        d2.encode([*a, "one too many"])


@pytest.mark.gpu
@pytest.mark.parametrize("slots_pow", [4, 6])
def test_dict_kernels_restore_to_the_last_slot(slots_pow):
    dev = _gpu()
    nslots = 1 << slots_pow
    strs, _lo, home = _full_table_strings(slots_pow)
    assert home[0] == home[1] == nslots - 1  # the restore wraps too
    d = StringDict(dev, slots_pow=slots_pow, new_cap=nslots)
    d.restore({"strings": strs[:nslots]})
    table = d.dlo.cpu().numpy().view(np.uint64)
    assert int((table == np.uint64(M64)).sum()) == 0
    order = list(range(nslots))[::-1]
    ids = d.encode([strs[i] for i in order])
    assert ids.cpu().tolist() == order  # the pinned ids
    assert len(d) == nslots
    d2 = StringDict(dev, slots_pow=slots_pow, new_cap=nslots)
    with pytest.raises(RuntimeError, match="table full"):
        d2.restore({"strings": strs})


@pytest.mark.gpu
def test_dict_restore_kernel_honours_an_id_permutation():
    dev = _gpu()
    strs = [*CONTENT, *(f"p{i}" for i in range(300))]
    n = len(strs)
    perm = np.random.default_rng(5).permutation(n).astype(np.int32)
    assert not np.array_equal(perm, np.arange(n))
    d = StringDict(dev, slots_pow=10, new_cap=64)
    data, offs = _pack_bytes([s.encode() for s in strs])
    d.k.dict_restore(
        torch.from_numpy(data).to(dev), torch.from_numpy(offs).to(dev),
        torch.from_numpy(perm).to(dev), d.dlo, d.dhi, d.dids, d.error_flag,
    )
    d.counter.fill_(n)
    d.id2str = [""] * n
    for s, i in zip(strs, perm.tolist()):
        d.id2str[i] = s
    assert int(d.error_flag.item()) == 0
    ids = d.encode(strs[::-1] + ["fresh"])
    assert ids.cpu().tolist() == [*perm[::-1].tolist(), n]
    assert d.decode(ids) == strs[::-1] + ["fresh"]


# -- string exchange ----------------------------------------------------


def _check_str_pack(data, offs, owner, vals, world, got, pad):
    """`got`: (counts, byte_counts, send_lens, send_ts, send_vals,
    send_bytes) as numpy, the send buffers `pad` longer than needed.
    The input's `ts` is ``TS_BASE + arange(n)``."""
    counts, bcounts, slens, sts, svals, sbytes = got
    n, total = len(offs) - 1, len(data)
    lens = np.diff(offs)
    ref_counts = np.bincount(owner, minlength=world)
    ref_bytes = np.zeros(world, dtype=np.int64)
    np.add.at(ref_bytes, owner, lens)
    assert counts.tolist() == ref_counts.tolist()
    assert bcounts.tolist() == ref_bytes.tolist()
    src = sts[:n] - TS_BASE
    assert np.array_equal(np.sort(src), np.arange(n))
    seg = np.repeat(np.arange(world), ref_counts)
    assert np.array_equal(owner[src], seg)
    assert np.array_equal(slens[:n], lens[src])
    seg_bytes = np.zeros(world, dtype=np.int64)
    np.add.at(seg_bytes, seg, slens[:n].astype(np.int64))
    assert seg_bytes.tolist() == bcounts.tolist()
    if vals is not None:
        assert np.array_equal(svals[:n], vals[src])
    # Wire byte b of row j is input byte offs[src[j]] + (b - start_j).
    starts = np.cumsum(slens[:n].astype(np.int64)) - slens[:n]
    where = np.arange(total) + np.repeat(offs[:-1][src] - starts, lens[src])
    assert np.array_equal(sbytes[:total], data[where])
    if pad:
        assert (slens[n:] == S32).all() and len(slens) == n + pad
        assert (sts[n:] == S64).all() and len(sts) == n + pad
        assert (sbytes[total:] == S8).all() and len(sbytes) == total + pad
        if vals is not None:
            assert (svals[n:] == S64).all() and len(svals) == n + pad


def _str_twin(data, offs, ts, vals, world):
    out = _str_bucket_cpu(data, offs, ts, vals, world)
    assert out[0].dtype == torch.int32 and out[1].dtype == torch.int64
    return tuple(o.numpy() if o is not None else None for o in out)


def _str_device(data, offs, ts, vals, world):
    dev, k = _gpu(), _ext()
    n, total = len(offs) - 1, len(data)
    full = functools.partial(torch.full, device=dev)
    counts = full((world,), 9, dtype=torch.int32)  # zeroed by the pack
    bcounts = full((world,), 9, dtype=torch.int64)
    slens = full((n + PAD,), S32, dtype=torch.int32)
    sts = full((n + PAD,), S64, dtype=torch.int64)
    svals = full((n + PAD if vals is not None else 0,), S64, dtype=torch.int64)
    sbytes = full((total + PAD,), S8, dtype=torch.uint8)
    k.str_exchange_pack(
        torch.from_numpy(data).to(dev), torch.from_numpy(offs).to(dev),
        torch.from_numpy(ts).to(dev),
        torch.from_numpy(vals).to(dev) if vals is not None else None,
        world, counts, bcounts, slens, sts, svals, sbytes,
    )
    return tuple(
        t.cpu().numpy() for t in (counts, bcounts, slens, sts, svals, sbytes)
    )


def _str_inputs(mix, n):
    """(data, offs, owner hashes hi) of one input mix."""
    if mix == "fixed":
        mat = _fixed_mat(n)
        return (*_pack_mat(mat), _hash128(_fnv_rows(mat))[1])
    if mix == "empty":
        bs = [b""] * n
    elif mix == "same":
        bs = ["all the sáme\x00".encode()] * n
    else:  # "long": 70,000-byte strings among empty and short ones
        long_a = LONG.encode()
        long_b = b"\xff" + long_a[1:]
        kinds = [b"", long_a, b"\x00", b"ab", b"", long_b, b"a\x00", "é".encode()]
        bs = [kinds[i % len(kinds)] for i in range(n)]
    uniq = {b: int(_hash128([_fnv_bytes(b)])[1][0]) for b in set(bs)}
    hi = np.array([uniq[b] for b in bs], dtype=np.uint64)
    return (*_pack_bytes(bs), hi)


def _str_case(run, mix, n, world, has_vals, pad):
    data, offs, hi = _str_inputs(mix, n)
    owner = _str_owner(hi, world)
    if mix in ("empty", "same") and n:
        assert len(set(owner.tolist())) == 1  # one rank gets everything
    if mix == "empty":
        assert len(data) == 0
    if mix == "long" and n >= 2:
        assert int(np.diff(offs).max()) == 70_000
    ts = TS_BASE + np.arange(n, dtype=np.int64)
    vals = _columns(n)[3].copy() if has_vals else None
    got = run(data, offs, ts, vals, world)
    _check_str_pack(data, offs, owner, vals, world, got, pad)


def test_str_checker_rejects_misrouted_and_altered_rows():
    world, n = 3, 65
    data, offs, hi = _str_inputs("fixed", n)
    owner = _str_owner(hi, world)
    ts = TS_BASE + np.arange(n, dtype=np.int64)
    vals = _columns(n)[3].copy()
    got = _str_twin(data, offs, ts, vals, world)
    _check_str_pack(data, offs, owner, vals, world, got, 0)
    counts, bcounts, slens, sts, svals, sbytes = got
    assert counts.min() > 0

    def rejected(*g):
        with pytest.raises(AssertionError):
            _check_str_pack(data, offs, owner, vals, world, g, 0)

    w = int(slens[0])
    b2 = sbytes.copy()  # bytes of two rows exchanged, metadata kept
    b2[:w], b2[w : 2 * w] = sbytes[w : 2 * w], sbytes[:w]
    rejected(counts, bcounts, slens, sts, svals, b2)
    t2, v2 = sts.copy(), svals.copy()  # first and last segment's rows
    t2[[0, n - 1]] = t2[[n - 1, 0]]
    v2[[0, n - 1]] = v2[[n - 1, 0]]
    b3 = sbytes.copy()
    b3[:w], b3[-w:] = sbytes[-w:], sbytes[:w]
    rejected(counts, bcounts, slens, t2, v2, b3)
    v3 = svals.copy()
    v3[3] ^= 1
    rejected(counts, bcounts, slens, sts, v3, sbytes)
    l2 = slens.copy()
    l2[0] -= 1
    rejected(counts, bcounts, l2, sts, svals, sbytes)
    bc = bcounts.copy()
    bc[0] += 1
    rejected(counts, bc, slens, sts, svals, sbytes)


@pytest.mark.parametrize("world", STR_WORLDS)
def test_str_owner_twin_matches_hash_port(world):
    rng = np.random.default_rng(world)
    bs = [s.encode() for s in CONTENT]
    bs += [bytes(rng.integers(0, 256, size=k).tolist()) for k in range(200)]
    _lo, hi = _hash128_list(bs)
    ref = _str_owner(hi, world).tolist()
    assert [str_owner_cpu(b, world) for b in bs] == ref


@pytest.mark.parametrize("world", STR_WORLDS)
def test_str_bucket_twin(world):
    for mix, sizes in (
        ("fixed", [*SMALL, 5000]),
        ("empty", [1, 257]),
        ("same", [1, 257]),
        ("long", [1, 2, 17]),
    ):
        for n in sizes:
            for has_vals in (False, True):
                _str_case(_str_twin, mix, n, world, has_vals, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("world", STR_WORLDS)
def test_str_exchange_pack_small(world):
    for mix, sizes in (
        ("fixed", SMALL),
        ("empty", [1, 64, 257]),
        ("same", [1, 65, 257]),
        ("long", [1, 2, 65, 257]),
    ):
        for n in sizes:
            for has_vals in (False, True):
                _str_case(_str_device, mix, n, world, has_vals, PAD)


@pytest.mark.gpu
@pytest.mark.parametrize("world", STR_WORLDS)
def test_str_exchange_pack_big(world):
    _str_case(_str_device, "fixed", BIG, world, world % 2 == 0, PAD)


@pytest.mark.gpu
@pytest.mark.parametrize("mix", ["empty", "same"])
def test_str_exchange_pack_big_one_destination(mix):
    _str_case(_str_device, mix, BIG, 3, mix == "same", PAD)
