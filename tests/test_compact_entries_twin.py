"""A numpy twin of the compact-entry mixer and its inverse (CPU only).

Compact scatter entries are the low 31 bits of ``y = mixn(x, n)`` with
``x = key32 | delta << 32`` an n = 32 + D bit word and the segment the
top D + 1 bits of ``y``; the aggregation and the spill paths recover the
key and the window delta with ``mixn_inv``.  The twin mirrors the device
functions in ``stream_kernels.hip`` line for line, and the GPU shape
tests decode real entry buffers with it.
"""

import numpy as np
import pytest

C = (0xFF51AFD7ED558CCD, 0xC4CEB9FE1A85EC53, 0x9E3779B97F4A7C15)
U = np.uint64


def mixn(x, n):
    m, s = U((1 << n) - 1), U((n + 1) // 2)
    x = np.asarray(x, dtype=np.uint64) & m
    for c in C:
        x = x ^ (x >> s)
        x = (x * U(c)) & m
    return x ^ (x >> s)


def mixn_inv(y, n):
    m, s = U((1 << n) - 1), U((n + 1) // 2)
    y = np.asarray(y, dtype=np.uint64) & m
    for c in reversed(C):
        y = y ^ (y >> s)
        y = (y * U(pow(c, -1, 1 << 64))) & m
    return y ^ (y >> s)


def encode(keys, deltas, n):
    """(segment, entry) of events, as the scatter computes them."""
    x = (np.asarray(keys).astype(np.int64).astype(np.uint64) & U(0xFFFFFFFF)) | (
        np.asarray(deltas, dtype=np.uint64) << U(32)
    )
    y = mixn(x, n)
    return (y >> U(31)).astype(np.int64), (y & U(0x7FFFFFFF)).astype(np.uint32)


def decode(seg, entry, n):
    """(key as int32, delta) of entries of segment `seg`."""
    y = (np.asarray(seg, dtype=np.uint64) << U(31)) | np.asarray(
        entry, dtype=np.uint64
    )
    x = mixn_inv(y, n)
    key = (x & U(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
    return key, (x >> U(32)).astype(np.int64)


EXTREME = [0, -1, -(1 << 31), (1 << 31) - 1]


@pytest.mark.parametrize("n", [38, 39, 40, 41])
def test_round_trip(n):
    d_bits = n - 32
    g = np.random.default_rng(n)
    # The extreme keys and a few others under every delta.
    keys = np.array(EXTREME + [1, 77, 123_456_789, -987_654], dtype=np.int64)
    kk, dd = np.meshgrid(keys, np.arange(1 << d_bits), indexing="ij")
    words = (kk.ravel().astype(np.uint64) & U(0xFFFFFFFF)) | (
        dd.ravel().astype(np.uint64) << U(32)
    )
    words = np.concatenate([words, g.integers(0, 1 << n, 100_000, dtype=np.uint64)])
    y = mixn(words, n)
    assert (y >> U(n) == 0).all()
    assert (mixn_inv(y, n) == words).all()
    # And through the (segment, entry) split.
    keys32 = (words & U(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
    deltas = (words >> U(32)).astype(np.int64)
    seg, entry = encode(keys32, deltas, n)
    assert seg.min() >= 0 and seg.max() < (2 << d_bits)
    k2, d2 = decode(seg, entry, n)
    assert (k2 == keys32).all() and (d2 == deltas).all()


@pytest.mark.parametrize("n", [38, 39, 40, 41])
def test_no_valid_entry_has_bit_31(n):
    g = np.random.default_rng(100 + n)
    keys = np.concatenate([np.array(EXTREME), g.integers(-(1 << 31), 1 << 31, 50_000)])
    deltas = g.integers(0, 1 << (n - 32), keys.size)
    _, entry = encode(keys, deltas, n)
    assert entry.dtype == np.uint32
    assert (entry >> np.uint32(31) == 0).all()
    assert (entry != np.uint32(0xFFFFFFFF)).all()


def test_mixer_is_a_bijection_on_a_small_word():
    """Exhaustive at n = 16: every value is hit exactly once."""
    y = mixn(np.arange(1 << 16, dtype=np.uint64), 16)
    assert np.unique(y).size == 1 << 16
