"""Loader of the built kernel library (no GPU, no compiler needed)."""

import os

from bytewax_amd.gpu import _ext


def test_load_built_missing_or_stale_is_none(tmp_path, monkeypatch):
    src = tmp_path / "k.hip"
    src.write_text("// source")
    monkeypatch.setattr(_ext, "_BUILD_DIR", tmp_path / "build")
    monkeypatch.setattr(_ext, "_SOURCES", [src])
    # Nothing built yet: leave it to the JIT builder.
    assert _ext.load_built() is None
    # A library older than its source must be rebuilt, never imported.
    (tmp_path / "build").mkdir()
    so = tmp_path / "build" / f"{_ext._NAME}.so"
    so.write_bytes(b"not a library")
    old = src.stat().st_mtime - 100
    os.utime(so, (old, old))
    assert _ext.load_built() is None
