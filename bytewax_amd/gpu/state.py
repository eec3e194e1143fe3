"""Additional HBM-resident keyed state: running stats and hash join.

Device twins of `reduce_final`-style keyed aggregations and the
`join` operator for the columnar path:

- :class:`StatsAggState` — 1BRC-style count/sum/min/max per
  (key, window) in one fused pass (BASELINE config 5);
- :class:`HashJoinState` — stream-stream join with HBM-resident
  open-address state, "last" insert / "complete" emit (config 4);
- :class:`WindowJoinState` — the same join per tumbling event-time
  window, "first" or "last" insert / "final" emit, with a close that
  reclaims the closed cells;
- :class:`SlidingWindowJoinState` — that join over sliding windows:
  one insert per event into panes, folded per window at close;
- :class:`WindowJoinProductState` — the tumbling windowed join with
  "product" insert: every left value of a cell with every right one.

All support pinned-host snapshot spill for recovery and have CPU
twins for GPU-less test runs.
"""

from typing import Any, Dict, List, Optional, Tuple

from . import AGG_COUNT, AGG_SUM, RecordBatch, _ms  # noqa: F401
from . import _check_error_flag, _LateTracker, _split_late_cpu
from ._ext import ext

_I64_MAX = (1 << 63) - 1
_I64_MIN = -(1 << 63)
_STATS_COLS = ("keys", "wins", "cnt", "sum", "min", "max")


def _wrap64(x: int) -> int:
    """Two's-complement int64 wrap, as the device's 64-bit adds do."""
    return ((x + (1 << 63)) & ((1 << 64) - 1)) - (1 << 63)


class StatsAggState:
    """Keyed (windowed) running count/sum/min/max on device.

    With ``track_late=True`` disordered batches are accepted and late
    events reported, with the semantics (and the sync-free `max_ts`
    hint) documented on `WindowAggState`: an event with absolute
    ``ts < watermark_of_earlier_batches - wait_ms`` joins no cell and
    comes out of :meth:`take_late` exactly once.
    """

    def __init__(
        self,
        device,
        align_ms: int,
        len_ms: int,
        slots_pow: int = 20,
        out_cap: int = 1 << 20,
        radix: bool = True,
        region_bits: int = 10,
        track_late: bool = False,
        wait_ms: int = 0,
        late_cap: int = 0,
    ):
        import torch

        self.track_late = track_late
        self.wait_ms = wait_ms
        self._late = (
            _LateTracker(device, wait_ms, True, late_cap)
            if track_late
            else None
        )
        self.device = device
        self.align_ms = align_ms
        self.len_ms = len_ms
        self.max_ts_host = 0
        self.closed_horizon = -(1 << 62)
        #: The second table (keys, cnt, sum, min, max) that a
        #: reclaiming close rebuilds the live cells into.  None until
        #: a close has rows to emit: a whole-stream state never pays
        #: for it.
        self.tables_alt: Optional[Tuple[Any, ...]] = None
        self.cpu = device.type == "cpu"
        if self.cpu:
            self._table: Dict[Tuple[int, int], Tuple[int, int, int, int]] = {}
            return
        self.k = ext()
        # The radix path needs enough regions for parallelism; keep at
        # least 1024 workgroups' worth.
        if radix:
            slots_pow = max(slots_pow, region_bits + 10)
        self.radix = radix
        self.region_bits = region_bits
        self.nslots = 1 << slots_pow
        if radix:
            self.n_regions = self.nslots >> region_bits
            self.rx_gcursors = torch.zeros(
                self.n_regions, dtype=torch.int32, device=device
            )
            self.rx_ov_cursor = torch.zeros(
                1, dtype=torch.int32, device=device
            )
            self.rx_max_batch = 0
            self.rx_packed = torch.empty(1, dtype=torch.int64, device=device)
            self.rx_vals = torch.empty(1, dtype=torch.int64, device=device)
            self.rx_ov_packed = torch.empty(
                1, dtype=torch.int64, device=device
            )
            self.rx_ov_vals = torch.empty(1, dtype=torch.int64, device=device)
        self.tkeys = torch.full(
            (self.nslots,), -1, dtype=torch.int64, device=device
        )
        self.tcnt = torch.zeros(self.nslots, dtype=torch.int64, device=device)
        self.tsum = torch.zeros(self.nslots, dtype=torch.int64, device=device)
        self.tmin = torch.full(
            (self.nslots,), _I64_MAX, dtype=torch.int64, device=device
        )
        self.tmax = torch.full(
            (self.nslots,), _I64_MIN, dtype=torch.int64, device=device
        )
        self.max_ts_dev = torch.zeros(1, dtype=torch.int64, device=device)
        self.error_flag = torch.zeros(1, dtype=torch.int32, device=device)
        self.out_cap = out_cap
        self.out_keys = torch.empty(out_cap, dtype=torch.int32, device=device)
        self.out_wins = torch.empty(out_cap, dtype=torch.int32, device=device)
        self.out = {
            name: torch.empty(out_cap, dtype=torch.int64, device=device)
            for name in ("cnt", "sum", "min", "max")
        }
        self.out_n = torch.zeros(1, dtype=torch.int32, device=device)

    def insert(self, batch: RecordBatch) -> None:
        import torch

        if batch.vals is None:
            msg = "stats aggregation requires a `vals` column"
            raise ValueError(msg)
        if (
            not self.cpu
            and not self.radix
            and batch.ts.dtype != torch.int64
        ):
            # The plain (non-radix) stats kernel takes absolute int64
            # timestamps; the radix scatter consumes int32 templates
            # natively.
            batch = RecordBatch(
                batch.keys,
                batch.ts.to(torch.int64),
                batch.vals,
                max_ts=batch.max_ts,
                ts_base=batch.ts_base,
            )
        late_args = ()
        if self.track_late and not self.cpu:
            lt = self._late
            lt.reserve(len(batch), self.error_flag)
            late_args = (
                self.max_ts_host - self.wait_ms, lt.keys, lt.ts, lt.vals, lt.n
            )
        if self.cpu:
            self._insert_cpu(batch)
        elif self.radix:
            import torch

            if len(batch) > self.rx_max_batch:
                mb = int(len(batch) * 5 // 4)
                self.rx_max_batch = mb
                per_region = -(-mb * 5 // 2) // self.n_regions + 1
                total = per_region * self.n_regions
                self.rx_packed = torch.empty(
                    total, dtype=torch.int64, device=self.device
                )
                self.rx_vals = torch.empty(
                    total, dtype=torch.int64, device=self.device
                )
                ov = max(1 << 20, mb)
                self.rx_ov_packed = torch.empty(
                    ov, dtype=torch.int64, device=self.device
                )
                self.rx_ov_vals = torch.empty(
                    ov, dtype=torch.int64, device=self.device
                )
            fn = (
                self.k.radix_stats_insert_late
                if late_args
                else self.k.radix_stats_insert
            )
            fn(
                batch.keys,
                batch.ts,
                batch.vals,
                self.tkeys,
                self.tcnt,
                self.tsum,
                self.tmin,
                self.tmax,
                self.max_ts_dev,
                self.error_flag,
                self.rx_gcursors,
                self.rx_packed,
                self.rx_vals,
                self.rx_ov_cursor,
                self.rx_ov_packed,
                self.rx_ov_vals,
                self.align_ms,
                self.len_ms,
                batch.ts_base,
                self.region_bits,
                *late_args,
            )
        else:
            fn = self.k.stats_insert_late if late_args else self.k.stats_insert
            fn(
                batch.keys,
                batch.ts,
                batch.vals,
                self.tkeys,
                self.tcnt,
                self.tsum,
                self.tmin,
                self.tmax,
                self.max_ts_dev,
                self.error_flag,
                self.align_ms,
                self.len_ms,
                batch.ts_base,
                *late_args,
            )
        if late_args:
            self._late.inserted()
        if batch.max_ts is not None:
            if batch.max_ts > self.max_ts_host:
                self.max_ts_host = batch.max_ts
        elif late_args:
            # The next cutoff needs this batch's maximum: without the
            # hint it has to come back from the device.
            dev_max = int(self.max_ts_dev.item())
            if dev_max > self.max_ts_host:
                self.max_ts_host = dev_max

    def take_late(self) -> Optional[RecordBatch]:
        """Drain the late events accumulated since the last call
        (`track_late` only): `keys`, absolute int64 `ts` (``ts_base``
        0) and `vals`, one row per late event.  Synchronises with the
        device."""
        if self._late is None:
            return None
        return self._late.take(None if self.cpu else self.error_flag)

    def late_drained(self) -> bool:
        """True when :meth:`insert` had to drain late rows into the
        host-side carry (see `WindowAggState.late_drained`)."""
        return self._late is not None and bool(self._late.carry)

    def _insert_cpu(self, batch: RecordBatch) -> None:
        if self.track_late:
            # The rule of the LATE kernels (see WindowAggState).
            batch = _split_late_cpu(
                batch, self.max_ts_host - self.wait_ms, self._late
            )
        keys = batch.keys.tolist()
        import torch

        wins = (
            (batch.ts.to(torch.int64) + batch.ts_base - self.align_ms)
            // self.len_ms
        ).tolist()
        vals = batch.vals.tolist()
        for k, w, v in zip(keys, wins, vals):
            cnt, s, mn, mx = self._table.get(
                (k, w), (0, 0, _I64_MAX, _I64_MIN)
            )
            self._table[(k, w)] = (
                cnt + 1, _wrap64(s + v), min(mn, v), max(mx, v)
            )
        if len(batch):
            mx_ts = int(batch.ts.max().item()) + batch.ts_base
            if mx_ts > self.max_ts_host:
                self.max_ts_host = mx_ts

    def extract(
        self, horizon: Optional[int] = None, clear: bool = True
    ) -> Optional[Dict[str, Any]]:
        """Extract (key, window) stats in [closed_horizon, horizon)
        (up to +inf if None).  On device the table is never mutated —
        already-emitted cells are excluded by the horizon range (no
        in-place deletion: it would corrupt probe chains); callers
        advance `closed_horizon` after a closing extract.  This call
        reclaims nothing: a stream that closes windows through it
        alone needs `slots_pow` sized for its total distinct
        (key, window) cells (1BRC-style whole-stream aggregation has
        exactly one window).  Close through :meth:`close_due` /
        :meth:`close_below` instead and `slots_pow` only has to hold
        the live working set: the cells of the windows still open."""
        import torch

        if horizon is None:
            horizon = 1 << 40
        win_lo = self.closed_horizon
        if win_lo < -(1 << 39):
            win_lo = -(1 << 39)
        if self.cpu:
            hit = [
                (k, w, v)
                for (k, w), v in self._table.items()
                if win_lo <= w < horizon
            ]
            if not hit:
                return None
            if clear:
                for k, w, _v in hit:
                    del self._table[(k, w)]
            return {
                "keys": torch.tensor([k for k, _w, _v in hit], dtype=torch.int32),
                "wins": torch.tensor([w for _k, w, _v in hit], dtype=torch.int32),
                "cnt": torch.tensor([v[0] for *_x, v in hit], dtype=torch.int64),
                "sum": torch.tensor([v[1] for *_x, v in hit], dtype=torch.int64),
                "min": torch.tensor([v[2] for *_x, v in hit], dtype=torch.int64),
                "max": torch.tensor([v[3] for *_x, v in hit], dtype=torch.int64),
            }
        self.out_n.zero_()
        self.k.stats_extract(
            self.tkeys,
            self.tcnt,
            self.tsum,
            self.tmin,
            self.tmax,
            win_lo,
            horizon,
            self.out_keys,
            self.out_wins,
            self.out["cnt"],
            self.out["sum"],
            self.out["min"],
            self.out["max"],
            self.out_n,
        )
        n = int(self.out_n.item())
        if n == 0:
            return None
        if n > self.out_cap:
            msg = f"stats extract produced {n} rows > out_cap"
            raise RuntimeError(msg)
        _check_error_flag(int(self.error_flag.item()), "stats table")
        return {
            "keys": self.out_keys[:n].clone(),
            "wins": self.out_wins[:n].clone(),
            "cnt": self.out["cnt"][:n].clone(),
            "sum": self.out["sum"][:n].clone(),
            "min": self.out["min"][:n].clone(),
            "max": self.out["max"][:n].clone(),
        }

    def close_due(
        self, wait_ms: Optional[int] = None
    ) -> Optional[Dict[str, Any]]:
        """Emit every window fully below the watermark (`max_ts_host`
        minus `wait_ms`, the constructor's by default) and reclaim its
        space; None when the horizon has not advanced.  See
        :meth:`close_below`."""
        return self.close_below(self.horizon_for(self.max_ts_host, wait_ms))

    def horizon_for(
        self, watermark_ms: int, wait_ms: Optional[int] = None
    ) -> int:
        """The window horizon of a watermark: every window below it
        ends at or before `watermark_ms` minus `wait_ms` (the
        constructor's by default).  What :meth:`close_below` takes."""
        if wait_ms is None:
            wait_ms = self.wait_ms
        return (watermark_ms - wait_ms - self.align_ms) // self.len_ms

    def close_eof(self) -> Optional[Dict[str, Any]]:
        """End of input, as the operator closes it: every cell at or
        above the closed horizon, with the horizon left where it is."""
        return self.extract(None, clear=True)

    def close_below(self, horizon: int) -> Optional[Dict[str, Any]]:
        """Close with reclamation: return the cells of windows in
        [closed_horizon, horizon) as :meth:`extract` does, keep the
        cells at or above `horizon`, forget everything below it and
        advance `closed_horizon` to `horizon`.

        On device the live cells are rebuilt in a second table (see
        k_stats_close_migrate), the tables are swapped and the retired
        one is reset on the stream, so the table only ever holds the
        open windows.  The second table is allocated by the first
        close that has rows to emit.  A cell below `closed_horizon`
        (an event behind the watermark that no late tracking caught)
        was never going to be emitted; it is dropped here."""
        import torch

        if horizon <= self.closed_horizon:
            return None
        win_lo = self.closed_horizon
        if win_lo < -(1 << 39):
            win_lo = -(1 << 39)
        if self.cpu:
            hit = [
                (k, w, v)
                for (k, w), v in self._table.items()
                if win_lo <= w < horizon
            ]
            for kw in [kw for kw in self._table if kw[1] < horizon]:
                del self._table[kw]
            self.closed_horizon = horizon
            if not hit:
                return None
            return {
                "keys": torch.tensor([k for k, _w, _v in hit], dtype=torch.int32),
                "wins": torch.tensor([w for _k, w, _v in hit], dtype=torch.int32),
                "cnt": torch.tensor([v[0] for *_x, v in hit], dtype=torch.int64),
                "sum": torch.tensor([v[1] for *_x, v in hit], dtype=torch.int64),
                "min": torch.tensor([v[2] for *_x, v in hit], dtype=torch.int64),
                "max": torch.tensor([v[3] for *_x, v in hit], dtype=torch.int64),
            }
        if self.tables_alt is None:
            # Until something is due there is nothing to reclaim: a
            # whole-stream state, whose operator asks once for the
            # windows below its only one, never pays for the second
            # table.  The stream's first close with rows scans twice.
            if self.extract(horizon, clear=False) is None:
                self.closed_horizon = horizon
                return None
            self.tables_alt = tuple(
                torch.full(
                    (self.nslots,), fill, dtype=torch.int64, device=self.device
                )
                for fill in (-1, 0, 0, _I64_MAX, _I64_MIN)
            )
        live = (self.tkeys, self.tcnt, self.tsum, self.tmin, self.tmax)
        self.out_n.zero_()
        self.k.stats_close_migrate(
            *live,
            *self.tables_alt,
            win_lo,
            min(horizon, 1 << 40),
            self.out_keys,
            self.out_wins,
            self.out["cnt"],
            self.out["sum"],
            self.out["min"],
            self.out["max"],
            self.out_n,
            self.error_flag,
        )
        (
            self.tkeys, self.tcnt, self.tsum, self.tmin, self.tmax
        ) = self.tables_alt
        self.tables_alt = live
        # Reset the retired table asynchronously for the next close.
        for t, fill in zip(live, (-1, 0, 0, _I64_MAX, _I64_MIN)):
            t.fill_(fill)
        n = int(self.out_n.item())
        if n > self.out_cap:
            msg = f"stats extract produced {n} rows > out_cap"
            raise RuntimeError(msg)
        _check_error_flag(int(self.error_flag.item()), "stats table")
        self.closed_horizon = horizon
        if n == 0:
            return None
        return {
            "keys": self.out_keys[:n].clone(),
            "wins": self.out_wins[:n].clone(),
            "cnt": self.out["cnt"][:n].clone(),
            "sum": self.out["sum"][:n].clone(),
            "min": self.out["min"][:n].clone(),
            "max": self.out["max"][:n].clone(),
        }

    def close_all(self) -> Optional[Dict[str, Any]]:
        """EOF: every cell at or above the closed horizon, read without
        mutating the device table."""
        out = self.extract(None, clear=True)
        self.closed_horizon = 1 << 40
        return out

    def snapshot_to_host(self) -> Dict[str, Any]:
        import torch

        snap = self.extract(None, clear=False)
        out: Dict[str, Any] = {
            "max_ts": self.max_ts_host,
            "closed_horizon": self.closed_horizon,
        }
        if snap is None:
            out["n"] = 0
            return out
        for name, t in snap.items():
            out[name] = t.cpu().numpy().copy()
        out["n"] = len(out["keys"])
        return out

    def _check_geometry(self, snap: Dict[str, Any]) -> None:
        """Refuse a snapshot of another window shape: a sliding
        state's rows are panes, not windows."""
        if "win_len_ms" in snap or "off_ms" in snap:
            msg = (
                "snapshot of sliding stats windows (length, offset) = "
                f"{(snap.get('win_len_ms'), snap.get('off_ms'))} ms cannot "
                "restore a tumbling stats state"
            )
            raise ValueError(msg)

    def restore_from_host(self, snap: Dict[str, Any]) -> None:
        self._check_geometry(snap)
        self.max_ts_host = snap["max_ts"]
        self.closed_horizon = snap["closed_horizon"]
        if snap["n"] == 0:
            return
        self.merge_rows(snap)

    def donor_meta(self, snap: Dict[str, Any]) -> Optional[Dict[str, Any]]:
        """Rescale: what of a donor shard's snapshot has to travel
        with its rows (checked against this state's window shape).
        Nothing for tumbling windows: no cell of an emitted window is
        ever kept."""
        self._check_geometry(snap)
        return None

    def merge_donors(self, parts) -> List[Dict[str, Any]]:
        """Rescale: merge the rows of donor shards, each a dict of the
        six columns plus ``"meta"`` from :meth:`donor_meta`.  Returns
        rows that have to be emitted at once (none here)."""
        import numpy as np

        parts = [p for p in parts if len(p["keys"])]
        if parts:
            self.merge_rows(
                {
                    c: np.concatenate([np.asarray(p[c]) for p in parts])
                    for c in _STATS_COLS
                }
            )
        return []

    def merge_rows(self, snap: Dict[str, Any]) -> None:
        """Additively merge saved stats rows into the live table
        (count/sum add, min/max observe).  Correct for occupied cells
        and duplicate rows, so rescale can concatenate multiple donor
        shards' spills before merging."""
        import torch

        if len(snap.get("keys", ())) == 0:
            return
        if self.cpu:
            for k, w, c, s, mn, mx in zip(
                snap["keys"].tolist(),
                snap["wins"].tolist(),
                snap["cnt"].tolist(),
                snap["sum"].tolist(),
                snap["min"].tolist(),
                snap["max"].tolist(),
            ):
                kw = (int(k), int(w))
                cur = self._table.get(kw)
                if cur is None:
                    self._table[kw] = (c, s, mn, mx)
                else:
                    self._table[kw] = (
                        cur[0] + c,
                        _wrap64(cur[1] + s),
                        min(cur[2], mn),
                        max(cur[3], mx),
                    )
            return
        wins = torch.as_tensor(snap["wins"]).to(torch.int64)
        ts = (wins * self.len_ms + self.align_ms).to(self.device)
        keys = torch.as_tensor(snap["keys"]).to(self.device)
        # Rebuild slots: count/sum re-add; min/max re-observe.  Use the
        # insert kernel once per stat via synthetic value columns would
        # be wrong for cnt/sum, so write slots directly through a
        # one-event-per-row insert of each stat:
        #   cnt: add (cnt-1) extra via sum of ones is wasteful; instead
        #   insert value=min (sets min), value=max (sets max), then fix
        #   cnt/sum arithmetically with a second pass.
        mn = torch.as_tensor(snap["min"]).to(self.device)
        mx = torch.as_tensor(snap["max"]).to(self.device)
        # Window starts, not event times: kept off the watermark
        # scalar (the late-tracking insert reads it back).
        no_wm = torch.zeros_like(self.max_ts_dev)
        self.k.stats_insert(
            keys, ts, mn, self.tkeys, self.tcnt, self.tsum, self.tmin,
            self.tmax, no_wm, self.error_flag,
            self.align_ms, self.len_ms, 0,
        )
        self.k.stats_insert(
            keys, ts, mx, self.tkeys, self.tcnt, self.tsum, self.tmin,
            self.tmax, no_wm, self.error_flag,
            self.align_ms, self.len_ms, 0,
        )
        # Correct cnt/sum: current slots have cnt=2, sum=min+max; the
        # delta columns below restore the snapshotted values exactly.
        cnt_fix = torch.as_tensor(snap["cnt"]).to(self.device) - 2
        sum_fix = (
            torch.as_tensor(snap["sum"]).to(self.device)
            - mn
            - mx
        )
        self.k.stats_fixup(
            keys, ts, cnt_fix, sum_fix, self.tkeys, self.tcnt, self.tsum,
            self.align_ms, self.len_ms,
        )


_STATS_FILLS = (-1, 0, 0, _I64_MAX, _I64_MIN)


def _stats_rows(hit) -> Dict[str, Any]:
    """The six-column dict of a list of (key, win, (cnt, sum, min, max))."""
    import torch

    return {
        "keys": torch.tensor([k for k, _w, _v in hit], dtype=torch.int32),
        "wins": torch.tensor([w for _k, w, _v in hit], dtype=torch.int32),
        "cnt": torch.tensor([v[0] for *_x, v in hit], dtype=torch.int64),
        "sum": torch.tensor([v[1] for *_x, v in hit], dtype=torch.int64),
        "min": torch.tensor([v[2] for *_x, v in hit], dtype=torch.int64),
        "max": torch.tensor([v[3] for *_x, v in hit], dtype=torch.int64),
    }


class SlidingStatsAggState(StatsAggState):
    """Keyed count/sum/min/max over sliding windows on device.

    Window `w` spans ``[align + w * off, align + w * off + len)``, the
    ids of `SlidingWindower`.  Events are aggregated once, by the
    parent's insert kernels, into non-overlapping *panes* of width
    ``g = gcd(len_ms, off_ms)``: the table holds (key, pane) cells and
    an insert costs what a tumbling window of length `g` costs.  A
    window is the ``L = len_ms / g`` panes ``[w * o, w * o + L)`` with
    ``o = off_ms / g``; count and sum add and min and max observe, so a
    close folds the panes of every due window into a separate fold
    table (k_stats_pane_close), reads the rows out of it and drops the
    panes that no open window contains.  An event that is not late
    lies in no closed window, so the result is the host windower's.

    `insert`, `take_late`, `snapshot_to_host`, `restore_from_host`,
    `merge_rows` and `extract` work on pane cells (the parent's
    `len_ms` is `g` and its `closed_horizon` the pane floor); the
    closing calls return windows.

    A pane outlives the windows that have closed over it for as long
    as an open window contains it, so pane rows alone do not say which
    windows are still owed: the window horizon travels with them, in
    snapshots and through a rescale (:meth:`merge_donors`).

    Limits:

    - ``L <= 64``.  The table holds up to `L` live cells per key, so
      size `slots_pow` for ``keys x (L + panes per watermark lag)``;
      the cap keeps that growth, and the ``w + L`` the fold table
      stores, small.
    - The fold table (`fold_slots_pow`, the table's size by default)
      has to hold the (key, window) rows of one close, kept under half
      full.  Reading the rows out and refilling it costs time in
      proportion to its size, so a stream that closes one window per
      close does best with a fold table sized for ``2 x keys``.
    - Event times must not precede `align_ms` (the stats kernels
      truncate towards zero), and pane ids ``(t - align_ms) / g`` must
      fit in int32.
    """

    MAX_PANES = 64

    def __init__(
        self,
        device,
        align_ms: int,
        len_ms: int,
        off_ms: int,
        slots_pow: int = 20,
        out_cap: int = 1 << 20,
        radix: bool = True,
        region_bits: int = 10,
        track_late: bool = False,
        wait_ms: int = 0,
        late_cap: int = 0,
        fold_slots_pow: Optional[int] = None,
    ):
        import math

        if off_ms <= 0:
            msg = "sliding stats `off_ms` must be positive"
            raise ValueError(msg)
        if off_ms > len_ms:
            msg = (
                "sliding stats `off_ms` can't be longer than `len_ms`; "
                "there would be gaps between windows"
            )
            raise ValueError(msg)
        g = math.gcd(len_ms, off_ms)
        if len_ms // g > self.MAX_PANES:
            msg = (
                f"sliding stats window of {len_ms} ms every {off_ms} ms "
                f"needs {len_ms // g} panes of {g} ms per window; at "
                f"most {self.MAX_PANES} are supported"
            )
            raise ValueError(msg)
        super().__init__(
            device, align_ms, g, slots_pow=slots_pow, out_cap=out_cap,
            radix=radix, region_bits=region_bits, track_late=track_late,
            wait_ms=wait_ms, late_cap=late_cap,
        )
        self.win_len_ms = len_ms
        self.off_ms = off_ms
        self.panes_per_window = len_ms // g
        self.panes_per_offset = off_ms // g
        #: Windows below this id have been emitted.
        self.win_horizon = -(1 << 62)
        #: The fold table (keys, cnt, sum, min, max); None until a
        #: close has windows to build.
        self.fold: Optional[Tuple[Any, ...]] = None
        if not self.cpu:
            self.fold_slots = (
                self.nslots if fold_slots_pow is None else 1 << fold_slots_pow
            )

    def horizon_for(
        self, watermark_ms: int, wait_ms: Optional[int] = None
    ) -> int:
        """Window `w` is due once ``w * off + len`` is at or below the
        watermark minus `wait_ms`; the windows below the returned id
        are."""
        if wait_ms is None:
            wait_ms = self.wait_ms
        rel = watermark_ms - wait_ms - self.align_ms
        return (rel - self.win_len_ms) // self.off_ms + 1

    def close_below(self, horizon: int) -> Optional[Dict[str, Any]]:
        """Return the windows in [win_horizon, horizon), folded from
        their panes, forget the panes that lie in no window at or above
        `horizon`, and advance `win_horizon` to `horizon` and the pane
        floor `closed_horizon` to ``horizon * o``.

        On device one kernel folds and migrates (k_stats_pane_close);
        the rows are then extracted from the fold table, which is
        refilled for the next close, all on the one stream.  The fold
        table and the second table are allocated by the first close
        that has a window to build."""
        if horizon <= self.win_horizon:
            return None
        win_hi = min(horizon, 1 << 40)
        pane_keep = win_hi * self.panes_per_offset
        out = self._fold(win_hi, pane_keep)
        self.win_horizon = horizon
        self.closed_horizon = pane_keep
        return out

    def _fold(self, win_hi: int, pane_keep: int) -> Optional[Dict[str, Any]]:
        """The rows of the windows in [win_horizon, win_hi); panes
        below `pane_keep` are forgotten.  Moves no horizon."""
        import torch

        n_w, n_o = self.panes_per_window, self.panes_per_offset
        win_lo = max(self.win_horizon, -(1 << 39))
        if self.cpu:
            folded: Dict[Tuple[int, int], Tuple[int, int, int, int]] = {}
            for (k, p), v in self._table.items():
                w_first = (p - n_w) // n_o + 1
                w_last = p // n_o
                for w in range(max(w_first, win_lo), min(w_last, win_hi - 1) + 1):
                    cur = folded.get((k, w), (0, 0, _I64_MAX, _I64_MIN))
                    folded[(k, w)] = (
                        cur[0] + v[0],
                        _wrap64(cur[1] + v[1]),
                        min(cur[2], v[2]),
                        max(cur[3], v[3]),
                    )
            for kp in [kp for kp in self._table if kp[1] < pane_keep]:
                del self._table[kp]
            if not folded:
                return None
            return _stats_rows([(k, w, v) for (k, w), v in folded.items()])
        if self.tables_alt is None:
            # A pane lies in a window below `win_hi` iff it is below
            # (win_hi - 1) * o + L, and a pane is dropped iff it is
            # below `pane_keep`: with no pane under the larger of the
            # two there is nothing to fold or to drop.
            bound = max((win_hi - 1) * n_o + n_w, pane_keep)
            if not self._any_pane_below(bound):
                return None
            self.tables_alt = tuple(
                torch.full(
                    (self.nslots,), fill, dtype=torch.int64, device=self.device
                )
                for fill in _STATS_FILLS
            )
        if self.fold is None:
            self.fold = tuple(
                torch.full(
                    (self.fold_slots,), fill, dtype=torch.int64,
                    device=self.device,
                )
                for fill in _STATS_FILLS
            )
        live = (self.tkeys, self.tcnt, self.tsum, self.tmin, self.tmax)
        self.k.stats_pane_close(
            *live,
            *self.tables_alt,
            *self.fold,
            win_lo,
            win_hi,
            pane_keep,
            n_w,
            n_o,
            self.error_flag,
        )
        (
            self.tkeys, self.tcnt, self.tsum, self.tmin, self.tmax
        ) = self.tables_alt
        self.tables_alt = live
        for t, fill in zip(live, _STATS_FILLS):
            t.fill_(fill)
        # Every occupied fold cell is a row; its window column holds
        # w + L (see the kernel).
        self.out_n.zero_()
        self.k.stats_extract(
            *self.fold,
            0,
            1 << 40,
            self.out_keys,
            self.out_wins,
            self.out["cnt"],
            self.out["sum"],
            self.out["min"],
            self.out["max"],
            self.out_n,
        )
        for t, fill in zip(self.fold, _STATS_FILLS):
            t.fill_(fill)
        n = int(self.out_n.item())
        if n > self.out_cap:
            msg = f"stats extract produced {n} rows > out_cap"
            raise RuntimeError(msg)
        _check_error_flag(int(self.error_flag.item()), "stats table")
        if n == 0:
            return None
        return {
            "keys": self.out_keys[:n].clone(),
            "wins": self.out_wins[:n] - n_w,
            "cnt": self.out["cnt"][:n].clone(),
            "sum": self.out["sum"][:n].clone(),
            "min": self.out["min"][:n].clone(),
            "max": self.out["max"][:n].clone(),
        }

    def _any_pane_below(self, bound: int) -> bool:
        """Whether the table holds a pane in [closed_horizon, bound).
        `k_stats_extract` counts the rows past the buffers' capacity
        without writing them, so the count alone is read."""
        self.out_n.zero_()
        self.k.stats_extract(
            self.tkeys,
            self.tcnt,
            self.tsum,
            self.tmin,
            self.tmax,
            max(self.closed_horizon, -(1 << 39)),
            bound,
            self.out_keys,
            self.out_wins,
            self.out["cnt"],
            self.out["sum"],
            self.out["min"],
            self.out["max"],
            self.out_n,
        )
        return int(self.out_n.item()) > 0

    def close_all(self) -> Optional[Dict[str, Any]]:
        """Every window that still holds a pane, the unfinished ones
        included; :meth:`close_below` with an unbounded horizon.  The
        state takes no further input afterwards."""
        return self.close_below(1 << 40)

    def close_eof(self) -> Optional[Dict[str, Any]]:
        """End of input, as the operator closes it: the rows of every
        window at or above `win_horizon`, the unfinished ones included,
        with both horizons and every live pane left where they are, as
        the tumbling :meth:`StatsAggState.close_eof` leaves its table.
        A snapshot taken afterwards resumes exactly: an execution that
        continues the stream emits the windows that were unfinished
        here again, complete, when they fall due."""
        return self._fold(1 << 40, self.closed_horizon)

    def snapshot_to_host(self) -> Dict[str, Any]:
        out = super().snapshot_to_host()
        out["win_horizon"] = self.win_horizon
        out["win_len_ms"] = self.win_len_ms
        out["off_ms"] = self.off_ms
        return out

    def _check_geometry(self, snap: Dict[str, Any]) -> None:
        geom = (snap.get("win_len_ms"), snap.get("off_ms"))
        if geom != (self.win_len_ms, self.off_ms):
            msg = (
                f"snapshot of sliding stats windows (length, offset) = "
                f"{geom} ms cannot restore a state of "
                f"{(self.win_len_ms, self.off_ms)} ms"
            )
            raise ValueError(msg)

    def restore_from_host(self, snap: Dict[str, Any]) -> None:
        super().restore_from_host(snap)
        self.win_horizon = snap["win_horizon"]

    def donor_meta(self, snap: Dict[str, Any]) -> Optional[Dict[str, Any]]:
        self._check_geometry(snap)
        return {"win_horizon": snap["win_horizon"]}

    def merge_donors(self, parts) -> List[Dict[str, Any]]:
        """Rescale: adopt the furthest window horizon among the donors
        (the merged state adopts the furthest watermark as well).  A
        pane row of a donor may lie in windows that donor has already
        emitted, so the horizon has to come along, or those windows
        would come out again, built from the panes that are left.  A
        donor that is behind is first closed up to the adopted horizon
        in a scratch state of its own; the rows of that close are
        returned for the operator to emit.  Exact as long as no key
        has rows in two donors with different horizons."""
        import numpy as np

        parts = [p for p in parts if len(p["keys"])]
        if not parts:
            return []
        n_o = self.panes_per_offset
        horizon = max(p["meta"]["win_horizon"] for p in parts)
        if self.win_horizon > horizon:
            horizon = self.win_horizon
        out = []
        for p in parts:
            rows = {c: p[c] for c in _STATS_COLS}
            behind = p["meta"]["win_horizon"]
            if behind < horizon:
                tmp = self._scratch_like(len(rows["keys"]))
                tmp.win_horizon = behind
                tmp.closed_horizon = max(behind, -(1 << 39)) * n_o
                tmp.merge_rows(rows)
                closed = tmp.close_below(horizon)
                if closed is not None:
                    out.append(closed)
                left = tmp.snapshot_to_host()
                if left["n"] == 0:
                    continue
                rows = {c: np.asarray(left[c]) for c in _STATS_COLS}
            self.merge_rows(rows)
        if horizon > self.win_horizon:
            self.win_horizon = horizon
            self.closed_horizon = horizon * n_o
        return out

    def _scratch_like(self, n_rows: int) -> "SlidingStatsAggState":
        """An empty state of this geometry, sized for `n_rows` cells."""
        if self.cpu:
            return SlidingStatsAggState(
                self.device, self.align_ms, self.win_len_ms, self.off_ms
            )
        slots_pow = max(10, (2 * n_rows - 1).bit_length())
        return SlidingStatsAggState(
            self.device, self.align_ms, self.win_len_ms, self.off_ms,
            slots_pow=slots_pow, out_cap=self.out_cap, radix=False,
        )


class HashJoinState:
    """Two-sided stream join state on device ("last"/"complete").

    With ``radix=True`` (default) each side's batch is partitioned
    into table-region segments first, so the exchange of flags/values
    stays L2-local per workgroup instead of random across the table.
    """

    N_SIDES = 2

    def __init__(
        self,
        device,
        slots_pow: int = 20,
        out_cap: int = 1 << 20,
        radix: Optional[bool] = None,
        region_bits: int = 11,
    ):
        import os

        import torch

        if radix is None:
            # Radix default: the LDS-deduped region join measures
            # 1.6x the direct atomics at 1M keys (r02 call 29/30,
            # profiles/); BYTEWAX_JOIN_RADIX=0 restores direct.
            radix = os.environ.get("BYTEWAX_JOIN_RADIX", "1") == "1"
        self.device = device
        self.cpu = device.type == "cpu"
        if self.cpu:
            self._table: Dict[int, list] = {}
            self._rows: List[Tuple[int, int, int]] = []
            return
        self.k = ext()
        if radix:
            slots_pow = max(slots_pow, region_bits + 10)
        self.radix = radix
        self.region_bits = region_bits
        self.nslots = 1 << slots_pow
        if radix:
            self.n_regions = self.nslots >> region_bits
            self.rx_gcursors = torch.zeros(
                self.n_regions, dtype=torch.int32, device=device
            )
            self.rx_ov_cursor = torch.zeros(1, dtype=torch.int32, device=device)
            self.rx_max_batch = 0
            self.rx_packed = torch.empty(1, dtype=torch.int64, device=device)
            self.rx_vals = torch.empty(1, dtype=torch.int64, device=device)
            self.rx_ov_packed = torch.empty(1, dtype=torch.int64, device=device)
            self.rx_ov_vals = torch.empty(1, dtype=torch.int64, device=device)
            self.rx_zeros = torch.zeros(1, dtype=torch.int64, device=device)
            self.rx_maxts = torch.zeros(1, dtype=torch.int64, device=device)
        self.tkeys = torch.full(
            (self.nslots,), -1, dtype=torch.int64, device=device
        )
        self.tval0 = torch.zeros(self.nslots, dtype=torch.int64, device=device)
        self.tval1 = torch.zeros(self.nslots, dtype=torch.int64, device=device)
        self.tflags = torch.zeros(self.nslots, dtype=torch.int32, device=device)
        self.error_flag = torch.zeros(1, dtype=torch.int32, device=device)
        self.out_cap = out_cap
        self.out_keys = torch.empty(out_cap, dtype=torch.int32, device=device)
        self.out_v0 = torch.empty(out_cap, dtype=torch.int64, device=device)
        self.out_v1 = torch.empty(out_cap, dtype=torch.int64, device=device)
        self.out_n = torch.zeros(1, dtype=torch.int32, device=device)
        self._pending = 0

    def insert(self, side: int, keys, vals) -> None:
        """Insert one side's (keys, vals) columns; completed pairs
        accumulate in the output buffer until `take_joined`."""
        if self.cpu:
            # Per-event twin of `join_apply`: the event that makes both
            # sides present emits the row and clears the flags, so a
            # later duplicate of the key in the same batch re-arms its
            # side.  Completing here, not in `take_joined`, keeps
            # several inserts before one drain equal to the device.
            for k, v in zip(keys.tolist(), vals.tolist()):
                ent = self._table.setdefault(int(k), [None, None, 0])
                ent[side] = int(v)
                ent[2] |= 1 << side
                if ent[2] == 3:
                    self._rows.append((int(k), ent[0], ent[1]))
                    ent[2] = 0
            return
        if self.radix:
            import torch

            n = int(keys.numel())
            if n > self.rx_max_batch:
                mb = int(n * 5 // 4)
                self.rx_max_batch = mb
                per_region = -(-mb * 5 // 2) // self.n_regions + 1
                total = per_region * self.n_regions
                self.rx_packed = torch.empty(
                    total, dtype=torch.int64, device=self.device
                )
                self.rx_vals = torch.empty(
                    total, dtype=torch.int64, device=self.device
                )
                ov = max(1 << 20, mb)
                self.rx_ov_packed = torch.empty(
                    ov, dtype=torch.int64, device=self.device
                )
                self.rx_ov_vals = torch.empty(
                    ov, dtype=torch.int64, device=self.device
                )
                self.rx_zeros = torch.zeros(
                    mb, dtype=torch.int64, device=self.device
                )
            self.k.radix_join_insert(
                keys,
                self.rx_zeros,
                vals,
                side,
                self.N_SIDES,
                self.tkeys,
                self.tval0,
                self.tval1,
                self.tflags,
                self.rx_gcursors,
                self.rx_packed,
                self.rx_vals,
                self.rx_ov_cursor,
                self.rx_ov_packed,
                self.rx_ov_vals,
                self.out_keys,
                self.out_v0,
                self.out_v1,
                self.out_n,
                self.rx_maxts,
                self.error_flag,
                self.region_bits,
            )
            return
        self.k.join_insert(
            keys,
            vals,
            side,
            self.N_SIDES,
            self.tkeys,
            self.tval0,
            self.tval1,
            self.tflags,
            self.out_keys,
            self.out_v0,
            self.out_v1,
            self.out_n,
            self.error_flag,
        )

    def snapshot_to_host(self) -> Dict[str, Any]:
        """Spill live (single-side) cells to host for recovery.

        Completed pairs reset their flags on emission
        (k_join_insert), so the live state is exactly the cells with
        a nonzero side mask.  Reuses the (drained) output buffers as
        extraction scratch."""
        import numpy as np
        import torch

        if self.cpu:
            rows = [
                (k, e[0] or 0, e[1] or 0, e[2])
                for k, e in self._table.items()
                if e[2]
            ]
            return {
                "keys": np.array([r[0] for r in rows], dtype="int32"),
                "v0": np.array([r[1] for r in rows], dtype="int64"),
                "v1": np.array([r[2] for r in rows], dtype="int64"),
                "flags": np.array([r[3] for r in rows], dtype="int32"),
            }
        if not hasattr(self, "_snap_flags"):
            self._snap_flags = torch.empty(
                self.out_cap, dtype=torch.int32, device=self.device
            )
            self._snap_n = torch.zeros(
                1, dtype=torch.int32, device=self.device
            )
        self._snap_n.zero_()
        self.k.join_extract(
            self.tkeys,
            self.tval0,
            self.tval1,
            self.tflags,
            self.out_keys,
            self.out_v0,
            self.out_v1,
            self._snap_flags,
            self._snap_n,
        )
        n = int(self._snap_n.item())
        if n > self.out_cap:
            msg = f"join snapshot produced {n} rows > out_cap"
            raise RuntimeError(msg)
        return {
            "keys": self.out_keys[:n].cpu().numpy().copy(),
            "v0": self.out_v0[:n].cpu().numpy().copy(),
            "v1": self.out_v1[:n].cpu().numpy().copy(),
            "flags": self._snap_flags[:n].cpu().numpy().copy(),
        }

    def restore_from_host(self, snap: Dict[str, Any]) -> None:
        """Re-insert each spilled side presence.  Single-side cells
        cannot re-complete, so nothing re-emits."""
        import torch

        flags = snap["flags"]
        for side, col in ((0, "v0"), (1, "v1")):
            m = (flags & (1 << side)) != 0
            if m.any():
                keys = torch.as_tensor(snap["keys"][m]).to(self.device)
                vals = torch.as_tensor(snap[col][m]).to(self.device)
                self.insert(side, keys, vals)

    def take_joined(self):
        """Drain completed (key, v0, v1) rows."""
        import torch

        if self.cpu:
            out, self._rows = self._rows, []
            if not out:
                return None
            return (
                torch.tensor([k for k, *_v in out], dtype=torch.int32),
                torch.tensor([v0 for _k, v0, _v1 in out], dtype=torch.int64),
                torch.tensor([v1 for *_kv, v1 in out], dtype=torch.int64),
            )
        # One D2H fetch for (count, error) — two .item() calls would
        # sync the stream twice per drained batch.
        n, err = torch.cat((self.out_n, self.error_flag)).cpu().tolist()
        if err != 0:
            msg = "join table overflowed; increase slots_pow"
            raise RuntimeError(msg)
        if n == 0:
            return None
        if n > self.out_cap:
            msg = f"join produced {n} rows > out_cap"
            raise RuntimeError(msg)
        out = (
            self.out_keys[:n].clone(),
            self.out_v0[:n].clone(),
            self.out_v1[:n].clone(),
        )
        self.out_n.zero_()
        return out


_WJOIN_COLS = ("keys", "wins", "v0", "v1", "mask")
_WJOIN_MODES = ("first", "last")
#: Kind tag of a `WindowJoinProductState` snapshot.
_WJPROD_KIND = "window_join_product"


def _wjoin_rows(hit) -> Optional[Dict[str, Any]]:
    """The five-column dict of a list of (key, win, [t0, v0, t1, v1])
    cells, None standing for an absent side."""
    import torch

    if not hit:
        return None
    return {
        "keys": torch.tensor([k for k, _w, _c in hit], dtype=torch.int32),
        "wins": torch.tensor([w for _k, w, _c in hit], dtype=torch.int32),
        "v0": torch.tensor(
            [0 if c[0] is None else c[1] for *_x, c in hit], dtype=torch.int64
        ),
        "v1": torch.tensor(
            [0 if c[2] is None else c[3] for *_x, c in hit], dtype=torch.int64
        ),
        "mask": torch.tensor(
            [
                (c[0] is not None) | ((c[2] is not None) << 1)
                for *_x, c in hit
            ],
            dtype=torch.int32,
        ),
    }


class WindowJoinState:
    """Two-sided join over tumbling event-time windows on device:
    "first" or "last" insert, "final" emit (the device twin of the
    host `join_window` with an `EventClock`, a `TumblingWindower` and
    ``ordered=True``).

    One cell per (key, window) holds, per side, a value and the
    timestamp of the event that won it.  Under "last" the event with
    the greatest timestamp holds a side, and among equal timestamps
    the latest arrival (a later batch beats an earlier one, within a
    batch the greater row index); under "first" the smallest timestamp
    and the earliest arrival.  That is what a stable sort by timestamp
    followed by the host's `on_value` gives, and it is exact for every
    input, run after run.

    A close emits each cell of a due window once, as columns `keys`,
    `wins`, `v0`, `v1` and `mask` (bit ``s`` set: side ``s`` present; a
    missing side's value column reads 0), and reclaims its slot.
    Values are arbitrary int64; timestamps lie strictly inside the
    int64 range.

    Without ``track_late`` (the default) nothing checks the ordering:
    see `window_join` for the contract.  With ``track_late=True``
    disordered batches are accepted and late events reported by the
    batch-granular rule of `WindowAggState`: an event of side ``s``
    with absolute ``ts < max_ts_host - wait_ms``, taken as it stands
    before its batch, joins no cell, whether its window is still open
    or not, and comes out of ``take_late(s)`` exactly once.  One late
    buffer per side says where a row came from (`late_cap` bounds each;
    0 sizes it from the batches).  An accepted event then has
    ``ts >= watermark - wait_ms``, so its window is at or above
    ``horizon_for(watermark)``: no cell is ever made behind the closed
    horizon and the drop arm of the close is unreachable.
    """

    def __init__(
        self,
        device,
        align_ms: int,
        len_ms: int,
        insert_mode: str = "last",
        slots_pow: int = 20,
        out_cap: int = 1 << 20,
        wait_ms: int = 0,
        track_late: bool = False,
        late_cap: int = 0,
    ):
        import torch

        if insert_mode not in _WJOIN_MODES:
            msg = (
                f"window join insert mode {insert_mode!r} is not "
                "supported on the device path: use 'first' or 'last'"
            )
            raise ValueError(msg)
        if len_ms <= 0:
            msg = "window length must be positive"
            raise ValueError(msg)
        self.device = device
        self.align_ms = align_ms
        self.len_ms = len_ms
        self.insert_mode = insert_mode
        self.first = insert_mode == "first"
        self.wait_ms = wait_ms
        self.track_late = track_late
        #: One tracker per side: a late row has to say which side it
        #: came from, and one insert call handles one side.
        self._late = (
            tuple(
                _LateTracker(device, wait_ms, True, late_cap)
                for _side in (0, 1)
            )
            if track_late
            else None
        )
        self.max_ts_host = 0
        self.closed_horizon = -(1 << 62)
        #: The second table (keys, ts0, ts1, v0, v1, elect) that a
        #: reclaiming close rebuilds the live cells into.  None until
        #: a close has rows to emit.
        self.tables_alt: Optional[Tuple[Any, ...]] = None
        self.cpu = device.type == "cpu"
        if self.cpu:
            #: (key, win) -> [ts0, v0, ts1, v1]; None = side absent.
            self._table: Dict[Tuple[int, int], List[Optional[int]]] = {}
            return
        self.k = ext()
        self.nslots = 1 << slots_pow
        #: Stamp of an absent side and idle election word (see
        #: k_wjoin_stamp).
        self.ts_none = _I64_MAX if self.first else _I64_MIN
        self._fills = (
            -1, self.ts_none, self.ts_none, 0, 0,
            0x7FFFFFFF if self.first else -1,
        )
        (
            self.tkeys, self.tts0, self.tts1, self.tv0, self.tv1,
            self.telect,
        ) = self._new_table()
        self.ev_slot = torch.empty(0, dtype=torch.int32, device=device)
        self.max_ts_dev = torch.zeros(1, dtype=torch.int64, device=device)
        self.error_flag = torch.zeros(1, dtype=torch.int32, device=device)
        self.out_cap = out_cap
        self.out = {
            name: torch.empty(
                out_cap,
                dtype=torch.int64 if name[0] in "vt" else torch.int32,
                device=device,
            )
            for name in ("keys", "wins", "v0", "v1", "t0", "t1", "mask")
        }
        self.out_n = torch.zeros(1, dtype=torch.int32, device=device)

    def _new_table(self) -> Tuple[Any, ...]:
        import torch

        return tuple(
            torch.full(
                (self.nslots,),
                fill,
                dtype=torch.int32 if i == 5 else torch.int64,
                device=self.device,
            )
            for i, fill in enumerate(self._fills)
        )

    def insert(self, side: int, batch: RecordBatch) -> None:
        """Insert one side's batch (`side` 0 = left, 1 = right).  With
        `track_late` the events below ``max_ts_host - wait_ms``, as it
        stands before this batch, go to the side's late rows."""
        self._insert(side, batch, self.track_late)

    def _insert(self, side: int, batch: RecordBatch, classify: bool) -> None:
        import torch

        if side not in (0, 1):
            msg = f"window join side must be 0 or 1, not {side!r}"
            raise ValueError(msg)
        if batch.vals is None:
            msg = "window join requires a `vals` column"
            raise ValueError(msg)
        n = len(batch)
        if self.cpu:
            self._insert_cpu(side, batch, classify)
            return
        if n:
            if self.ev_slot.numel() < n:
                self.ev_slot = torch.empty(
                    n * 5 // 4, dtype=torch.int32, device=self.device
                )
            late_args = ()
            if classify:
                lt = self._late[side]
                lt.reserve(n, self.error_flag)
                late_args = (
                    self.max_ts_host - self.wait_ms,
                    lt.keys, lt.ts, lt.vals, lt.n,
                )
            fn = self.k.wjoin_insert_late if classify else self.k.wjoin_insert
            fn(
                batch.keys,
                batch.ts,
                batch.vals,
                self.tkeys,
                self.tts1 if side else self.tts0,
                self.tv1 if side else self.tv0,
                self.telect,
                self.ev_slot,
                self.max_ts_dev,
                self.error_flag,
                self.align_ms,
                self.len_ms,
                batch.ts_base,
                self.first,
                *late_args,
            )
            if classify:
                self._late[side].inserted()
        if batch.max_ts is not None:
            if batch.max_ts > self.max_ts_host:
                self.max_ts_host = batch.max_ts
        elif n:
            # No host-side hint: the watermark (and with `track_late`
            # the next cutoff) has to come back from the device.
            dev_max = int(self.max_ts_dev.item())
            if dev_max > self.max_ts_host:
                self.max_ts_host = dev_max

    def take_late(self, side: int) -> Optional[RecordBatch]:
        """Drain the late events of `side` accumulated since the last
        call (`track_late` only): `keys`, absolute int64 `ts`
        (``ts_base`` 0) and `vals`, one row per late event, in no
        defined order.  Synchronises with the device."""
        if side not in (0, 1):
            msg = f"window join side must be 0 or 1, not {side!r}"
            raise ValueError(msg)
        if self._late is None:
            return None
        return self._late[side].take(None if self.cpu else self.error_flag)

    def late_drained(self) -> bool:
        """True when :meth:`insert` had to drain late rows of either
        side into the host-side carry (see
        `WindowAggState.late_drained`)."""
        return self._late is not None and any(
            bool(lt.carry) for lt in self._late
        )

    def _insert_cpu(
        self, side: int, batch: RecordBatch, classify: bool = False
    ) -> None:
        import torch

        if classify:
            # The rule of the LATE stamp pass (see WindowAggState).
            batch = _split_late_cpu(
                batch, self.max_ts_host - self.wait_ms, self._late[side]
            )
        keys = batch.keys.tolist()
        ts = (batch.ts.to(torch.int64) + batch.ts_base).tolist()
        vals = batch.vals.tolist()
        # Rows in arrival order: ">=" lets the later of equals take a
        # "last" side, "<" keeps the earlier of equals on a "first" one.
        for k, t, v in zip(keys, ts, vals):
            kw = (k, (t - self.align_ms) // self.len_ms)
            cell = self._table.get(kw)
            if cell is None:
                cell = self._table[kw] = [None, None, None, None]
            cur = cell[2 * side]
            if cur is None or (t < cur if self.first else t >= cur):
                cell[2 * side] = t
                cell[2 * side + 1] = v
        mx_ts = batch.max_ts
        if mx_ts is None and ts:
            mx_ts = max(ts)
        if mx_ts is not None and mx_ts > self.max_ts_host:
            self.max_ts_host = mx_ts

    def _win_lo(self) -> int:
        return max(self.closed_horizon, -(1 << 39))

    def _take(self, n: int, cols) -> Dict[str, Any]:
        return {name: self.out[name][:n].clone() for name in cols}

    def _check(self, n: int) -> None:
        if n > self.out_cap:
            msg = f"window join extract produced {n} rows > out_cap"
            raise RuntimeError(msg)
        _check_error_flag(int(self.error_flag.item()), "window join table")

    def extract(
        self,
        horizon: Optional[int] = None,
        clear: bool = True,
        stamps: bool = False,
    ) -> Optional[Dict[str, Any]]:
        """The cells of windows in [closed_horizon, horizon) (up to
        +inf if None) without reclaiming anything; the device table is
        not mutated (`clear` drops the rows from the CPU twin only, as
        `StatsAggState.extract` does).  With `stamps` the winning
        timestamps come along as `t0` and `t1`."""
        import torch

        if horizon is None:
            horizon = 1 << 40
        win_lo = self._win_lo()
        cols = _WJOIN_COLS + (("t0", "t1") if stamps else ())
        if self.cpu:
            hit = [
                (k, w, c)
                for (k, w), c in self._table.items()
                if win_lo <= w < horizon
            ]
            if clear:
                for k, w, _c in hit:
                    del self._table[(k, w)]
            rows = _wjoin_rows(hit)
            if rows is not None and stamps:
                for name, j in (("t0", 0), ("t1", 2)):
                    rows[name] = torch.tensor(
                        [0 if c[j] is None else c[j] for *_x, c in hit],
                        dtype=torch.int64,
                    )
            return rows
        self.out_n.zero_()
        self.k.wjoin_extract(
            self.tkeys, self.tts0, self.tts1, self.tv0, self.tv1,
            win_lo, horizon, self.ts_none,
            *(self.out[c] for c in ("keys", "wins", "v0", "v1", "t0", "t1")),
            self.out["mask"], self.out_n,
        )
        n = int(self.out_n.item())
        self._check(n)
        if n == 0:
            return None
        return self._take(n, cols)

    def close_due(
        self, wait_ms: Optional[int] = None
    ) -> Optional[Dict[str, Any]]:
        """Emit every window fully below the watermark (`max_ts_host`
        minus `wait_ms`, the constructor's by default) and reclaim its
        space; None when nothing was due.  See :meth:`close_below`."""
        return self.close_below(self.horizon_for(self.max_ts_host, wait_ms))

    def horizon_for(
        self, watermark_ms: int, wait_ms: Optional[int] = None
    ) -> int:
        """The window horizon of a watermark: every window below it
        ends at or before `watermark_ms` minus `wait_ms` (the
        constructor's by default).  What :meth:`close_below` takes."""
        if wait_ms is None:
            wait_ms = self.wait_ms
        return (watermark_ms - wait_ms - self.align_ms) // self.len_ms

    def close_eof(self) -> Optional[Dict[str, Any]]:
        """End of input, as the operator closes it: every cell at or
        above the closed horizon, with the horizon left where it is."""
        return self.extract(None, clear=True)

    def close_all(self) -> Optional[Dict[str, Any]]:
        """EOF: every cell at or above the closed horizon, read without
        mutating the device table; nothing is emitted after it."""
        out = self.extract(None, clear=True)
        self.closed_horizon = 1 << 40
        return out

    def close_below(self, horizon: int) -> Optional[Dict[str, Any]]:
        """Close with reclamation: return the cells of windows in
        [closed_horizon, horizon), each exactly once, keep the cells at
        or above `horizon`, forget everything below it and advance
        `closed_horizon` to `horizon`.

        On device the live cells are rebuilt in a second table (see
        k_wjoin_close_migrate), the tables are swapped and the retired
        one is reset on the stream, so the table only ever holds the
        open windows.  The second table is allocated by the first
        close that has rows to emit.  A cell below `closed_horizon`
        (an event behind the watermark) was never going to be emitted;
        it is dropped here.  Only a state without `track_late` can hold
        one: with it such an event went to the late rows instead."""
        if horizon <= self.closed_horizon:
            return None
        win_lo = self._win_lo()
        if self.cpu:
            hit = [
                (k, w, c)
                for (k, w), c in self._table.items()
                if win_lo <= w < horizon
            ]
            for kw in [kw for kw in self._table if kw[1] < horizon]:
                del self._table[kw]
            self.closed_horizon = horizon
            return _wjoin_rows(hit)
        if self.tables_alt is None:
            # Until something is due there is nothing to reclaim.  The
            # stream's first close with rows scans twice.
            if self.extract(horizon, clear=False) is None:
                self.closed_horizon = horizon
                return None
            self.tables_alt = self._new_table()
        live = (
            self.tkeys, self.tts0, self.tts1, self.tv0, self.tv1,
            self.telect,
        )
        self.out_n.zero_()
        self.k.wjoin_close_migrate(
            *live[:5],
            *self.tables_alt[:5],
            win_lo,
            min(horizon, 1 << 40),
            self.ts_none,
            *(self.out[c] for c in _WJOIN_COLS),
            self.out_n,
            self.error_flag,
        )
        (
            self.tkeys, self.tts0, self.tts1, self.tv0, self.tv1,
            self.telect,
        ) = self.tables_alt
        self.tables_alt = live
        # Reset the retired table asynchronously for the next close.
        # Its election words are idle already: every insert leaves
        # them so.
        for t, fill in zip(live[:5], self._fills):
            t.fill_(fill)
        n = int(self.out_n.item())
        self._check(n)
        self.closed_horizon = horizon
        if n == 0:
            return None
        return self._take(n, _WJOIN_COLS)

    def snapshot_to_host(self) -> Dict[str, Any]:
        """Spill the live cells with their winning timestamps, the
        closed horizon, the window geometry, the insert mode and
        `track_late`.  Late rows not yet taken are not part of it: the
        caller drains them through :meth:`take_late` and persists them
        itself (as `_ColumnarJoinLogic` does)."""
        out: Dict[str, Any] = {
            "max_ts": self.max_ts_host,
            "closed_horizon": self.closed_horizon,
            "align_ms": self.align_ms,
            "len_ms": self.len_ms,
            "insert_mode": self.insert_mode,
            "track_late": self.track_late,
            "n": 0,
        }
        snap = self.extract(None, clear=False, stamps=True)
        if snap is not None:
            for name, t in snap.items():
                out[name] = t.cpu().numpy().copy()
            out["n"] = len(out["keys"])
        return out

    def restore_from_host(self, snap: Dict[str, Any]) -> None:
        """Re-insert each present side as the event (key, winning
        timestamp, value) through the insert without late tracking:
        the timestamp lies in the cell's window and wins an empty side
        again.  Restore never classifies: once side 0 is in with the
        snapshot's `max_ts`, a side-1 stamp of a still open window may
        lie below ``max_ts - wait_ms``, and it was accepted when it
        arrived.  A snapshot taken with `track_late` restores only into
        a state that has it too (its stream may be disordered); one
        taken without restores into either kind."""
        import torch

        if snap.get("kind") == _WJPROD_KIND:
            msg = (
                "snapshot of a window product join holds value lists and "
                "cannot restore a 'first' / 'last' window join"
            )
            raise ValueError(msg)
        self._check_kind(snap)
        theirs = (
            snap.get("align_ms"), snap.get("len_ms"), snap.get("insert_mode")
        )
        mine = (self.align_ms, self.len_ms, self.insert_mode)
        if theirs != mine:
            msg = (
                "snapshot of a window join with (align_ms, len_ms, "
                f"insert_mode) = {theirs} cannot restore one with {mine}"
            )
            raise ValueError(msg)
        if snap.get("track_late", False) and not self.track_late:
            msg = (
                "snapshot of a window join with track_late=True cannot "
                "restore one without late tracking"
            )
            raise ValueError(msg)
        if snap["n"]:
            for side in (0, 1):
                m = (snap["mask"] & (1 << side)) != 0
                if not m.any():
                    continue
                self._insert(
                    side,
                    RecordBatch(
                        torch.as_tensor(snap["keys"][m]).to(self.device),
                        torch.as_tensor(snap[f"t{side}"][m]).to(self.device),
                        torch.as_tensor(snap[f"v{side}"][m]).to(self.device),
                        max_ts=snap["max_ts"],
                    ),
                    False,
                )
        self.max_ts_host = snap["max_ts"]
        self.closed_horizon = snap["closed_horizon"]

    def _check_kind(self, snap: Dict[str, Any]) -> None:
        """Refuse a snapshot of the other window kind: the cells of a
        sliding join are panes, and its window horizon would be lost."""
        if "win_len_ms" in snap:
            geom = (snap.get("win_len_ms"), snap.get("off_ms"))
            msg = (
                f"snapshot of a sliding window join (length, offset) = "
                f"{geom} ms cannot restore a tumbling window join"
            )
            raise ValueError(msg)


def _sliding_join_geometry(len_ms: int, off_ms: int) -> Tuple[int, int, int]:
    """Pane width and panes per window and per offset of a sliding
    join, or the `ValueError` of a geometry it does not support."""
    import math

    if off_ms <= 0:
        msg = "sliding window join `off_ms` must be positive"
        raise ValueError(msg)
    if off_ms > len_ms:
        msg = (
            "sliding window join `off_ms` can't be longer than `len_ms`; "
            "there would be gaps between windows"
        )
        raise ValueError(msg)
    g = math.gcd(len_ms, off_ms)
    if len_ms // g > SlidingWindowJoinState.MAX_PANES:
        msg = (
            f"sliding window join of {len_ms} ms every {off_ms} ms "
            f"needs {len_ms // g} panes of {g} ms per window; at "
            f"most {SlidingWindowJoinState.MAX_PANES} are supported"
        )
        raise ValueError(msg)
    return g, len_ms // g, off_ms // g


class SlidingWindowJoinState(WindowJoinState):
    """Two-sided "first"/"last" join over sliding event-time windows on
    device, "final" emit (the device twin of the host `join_window`
    with an `EventClock`, a `SlidingWindower` and ``ordered=True``).

    Window `w` spans ``[align + w * off, align + w * off + len)``, the
    ids of `SlidingWindower`.  Events are inserted once, by the
    parent's three insert kernels, into non-overlapping *panes* of
    width ``g = gcd(len_ms, off_ms)``: the table holds (key, pane)
    cells and an insert costs what a tumbling join of length `g`
    costs.  A window is the ``L = len_ms / g`` panes
    ``[w * o, w * o + L)`` with ``o = off_ms / g``.  The panes of a
    window are disjoint in time, so the winner of a side over the
    window is the winner of the pane with the greatest ("last") or
    smallest ("first") stamp; a close folds the panes of every due
    window that way into a separate fold table (k_wjoin_pane_stamp,
    k_wjoin_pane_commit), reads the rows out of it and drops the panes
    that no open window contains.

    `insert`, `take_late`, `late_drained`, `extract`,
    `snapshot_to_host` and `restore_from_host` work on pane cells (the
    parent's `len_ms` is `g` and its `closed_horizon` the pane floor);
    the closing calls return windows.  Late tracking is the parent's,
    unchanged: an accepted event has ``ts >= watermark - wait``, and
    window `w` is closed only when ``align + w * off + len <=
    watermark - wait``, so an accepted event lies in no emitted window.

    A pane outlives the windows that have closed over it for as long
    as an open window contains it, so pane cells alone do not say
    which windows are still owed: `win_horizon` travels with them in
    snapshots.

    Limits:

    - ``L <= 64``.  The table holds up to `L` live cells per key, so
      size `slots_pow` for ``keys x (L + panes the wait spans)``.
    - The fold table (`fold_slots_pow`, the table's size by default)
      has to hold the (key, window) rows of one close, kept under half
      full.  Reading the rows out and refilling it costs time in
      proportion to its size, so a stream that closes one window per
      close does best with a fold table sized for ``2 x keys``.
    - Event times must not precede `align_ms` (a window below
      ``1 - L`` is not built), and pane ids ``(t - align_ms) / g``
      must fit in int32.
    """

    MAX_PANES = 64

    def __init__(
        self,
        device,
        align_ms: int,
        len_ms: int,
        off_ms: int,
        insert_mode: str = "last",
        slots_pow: int = 20,
        out_cap: int = 1 << 20,
        wait_ms: int = 0,
        track_late: bool = False,
        late_cap: int = 0,
        fold_slots_pow: Optional[int] = None,
    ):
        g, n_w, n_o = _sliding_join_geometry(len_ms, off_ms)
        super().__init__(
            device, align_ms, g, insert_mode=insert_mode,
            slots_pow=slots_pow, out_cap=out_cap, wait_ms=wait_ms,
            track_late=track_late, late_cap=late_cap,
        )
        self.win_len_ms = len_ms
        self.off_ms = off_ms
        self.panes_per_window = n_w
        self.panes_per_offset = n_o
        #: Windows below this id have been emitted.
        self.win_horizon = -(1 << 62)
        #: The fold table (keys, ts0, ts1, v0, v1); None until a close
        #: has a pane to fold or drop.
        self.fold: Optional[Tuple[Any, ...]] = None
        #: Most blocks the two close passes launch (0: the launcher's
        #: cap); fewer blocks than 2,048-slot chunks makes each block
        #: stride over several.
        self.close_blocks = 0
        if not self.cpu:
            self.fold_slots = (
                self.nslots if fold_slots_pow is None else 1 << fold_slots_pow
            )

    def horizon_for(
        self, watermark_ms: int, wait_ms: Optional[int] = None
    ) -> int:
        """Window `w` is due once ``w * off + len`` is at or below the
        watermark minus `wait_ms`; the windows below the returned id
        are."""
        if wait_ms is None:
            wait_ms = self.wait_ms
        rel = watermark_ms - wait_ms - self.align_ms
        return (rel - self.win_len_ms) // self.off_ms + 1

    def close_below(self, horizon: int) -> Optional[Dict[str, Any]]:
        """Return the windows in [win_horizon, horizon), folded from
        their panes, forget the panes that lie in no window at or above
        `horizon`, and advance `win_horizon` to `horizon` and the pane
        floor `closed_horizon` to ``horizon * o``.

        On device two launches fold and migrate (k_wjoin_pane_stamp,
        k_wjoin_pane_commit); the rows are then extracted from the fold
        table, which is refilled for the next close, all on the one
        stream.  The fold table and the second pane table are allocated
        by the first close that has a pane to fold or drop."""
        if horizon <= self.win_horizon:
            return None
        win_hi = min(horizon, 1 << 40)
        pane_keep = win_hi * self.panes_per_offset
        out = self._fold(win_hi, pane_keep)
        self.win_horizon = horizon
        self.closed_horizon = pane_keep
        return out

    def _fold(self, win_hi: int, pane_keep: int) -> Optional[Dict[str, Any]]:
        """The rows of the windows in [win_horizon, win_hi); panes
        below `pane_keep` are forgotten.  Moves no horizon."""
        n_w, n_o = self.panes_per_window, self.panes_per_offset
        win_lo = max(self.win_horizon, -(1 << 39))
        if self.cpu:
            # Per (key, window) and side the pane with the greatest
            # ("last") / smallest ("first") stamp; stamps of different
            # panes never tie.
            folded: Dict[Tuple[int, int], List[Optional[int]]] = {}
            for (k, p), c in self._table.items():
                w_first = max((p - n_w) // n_o + 1, win_lo, 1 - n_w)
                w_last = min(p // n_o, win_hi - 1)
                for w in range(w_first, w_last + 1):
                    cur = folded.setdefault((k, w), [None, None, None, None])
                    for j in (0, 2):
                        t = c[j]
                        if t is None:
                            continue
                        if cur[j] is None or (
                            t < cur[j] if self.first else t > cur[j]
                        ):
                            cur[j] = t
                            cur[j + 1] = c[j + 1]
            for kp in [kp for kp in self._table if kp[1] < pane_keep]:
                del self._table[kp]
            return _wjoin_rows([(k, w, c) for (k, w), c in folded.items()])
        if self.tables_alt is None:
            # A pane lies in a window below `win_hi` iff it is below
            # (win_hi - 1) * o + L, and a pane is dropped iff it is
            # below `pane_keep`: with no pane under the larger of the
            # two there is nothing to fold or to drop.
            bound = max((win_hi - 1) * n_o + n_w, pane_keep)
            if not self._any_pane_below(bound):
                return None
            self.tables_alt = self._new_table()
        if self.fold is None:
            import torch

            self.fold = tuple(
                torch.full(
                    (self.fold_slots,), fill, dtype=torch.int64,
                    device=self.device,
                )
                for fill in self._fills[:5]
            )
        live = (
            self.tkeys, self.tts0, self.tts1, self.tv0, self.tv1,
            self.telect,
        )
        self.k.wjoin_pane_stamp(
            *live[:5],
            *self.tables_alt[:5],
            *self.fold,
            win_lo,
            win_hi,
            pane_keep,
            n_w,
            n_o,
            self.first,
            self.error_flag,
            self.close_blocks,
        )
        # The old pane table is still intact: the commit reads it.
        self.k.wjoin_pane_commit(
            *live[:5],
            *self.fold,
            win_lo,
            win_hi,
            n_w,
            n_o,
            self.first,
            self.error_flag,
            self.close_blocks,
        )
        (
            self.tkeys, self.tts0, self.tts1, self.tv0, self.tv1,
            self.telect,
        ) = self.tables_alt
        self.tables_alt = live
        # Election words are idle between inserts (see close_below of
        # the parent).
        for t, fill in zip(live[:5], self._fills):
            t.fill_(fill)
        # Every fold cell with a side is a row; its window column holds
        # w + L (see the kernel).
        self.out_n.zero_()
        self.k.wjoin_extract(
            *self.fold,
            0,
            1 << 40,
            self.ts_none,
            *(self.out[c] for c in ("keys", "wins", "v0", "v1", "t0", "t1")),
            self.out["mask"],
            self.out_n,
        )
        for t, fill in zip(self.fold, self._fills):
            t.fill_(fill)
        n = int(self.out_n.item())
        self._check(n)
        if n == 0:
            return None
        out = self._take(n, _WJOIN_COLS)
        out["wins"] -= n_w
        return out

    def _any_pane_below(self, bound: int) -> bool:
        """Whether the table holds a pane in [closed_horizon, bound).
        `k_wjoin_extract` counts the rows past the buffers' capacity
        without writing them, so the count alone is read."""
        self.out_n.zero_()
        self.k.wjoin_extract(
            self.tkeys, self.tts0, self.tts1, self.tv0, self.tv1,
            self._win_lo(), bound, self.ts_none,
            *(self.out[c] for c in ("keys", "wins", "v0", "v1", "t0", "t1")),
            self.out["mask"], self.out_n,
        )
        return int(self.out_n.item()) > 0

    def close_all(self) -> Optional[Dict[str, Any]]:
        """Every window that still holds a pane, the unfinished ones
        included; :meth:`close_below` with an unbounded horizon.  The
        state takes no further input afterwards."""
        return self.close_below(1 << 40)

    def close_eof(self) -> Optional[Dict[str, Any]]:
        """End of input, as the operator closes it: the rows of every
        window at or above `win_horizon`, the unfinished ones included,
        with both horizons and every live pane left where they are.  A
        snapshot taken afterwards resumes exactly: an execution that
        continues the stream emits the windows that were unfinished
        here again, complete, when they fall due."""
        return self._fold(1 << 40, self.closed_horizon)

    def snapshot_to_host(self) -> Dict[str, Any]:
        out = super().snapshot_to_host()
        out["win_horizon"] = self.win_horizon
        out["win_len_ms"] = self.win_len_ms
        out["off_ms"] = self.off_ms
        return out

    def _check_kind(self, snap: Dict[str, Any]) -> None:
        if "win_len_ms" not in snap:
            msg = (
                "snapshot of a tumbling window join cannot restore a "
                "sliding window join"
            )
            raise ValueError(msg)
        geom = (snap.get("win_len_ms"), snap.get("off_ms"))
        if geom != (self.win_len_ms, self.off_ms):
            msg = (
                f"snapshot of a sliding window join (length, offset) = "
                f"{geom} ms cannot restore a state of "
                f"{(self.win_len_ms, self.off_ms)} ms"
            )
            raise ValueError(msg)

    def restore_from_host(self, snap: Dict[str, Any]) -> None:
        """The parent's restore of the pane cells, then the window
        horizon.  A snapshot of another (length, offset), or of a
        tumbling join, is refused."""
        super().restore_from_host(snap)
        self.win_horizon = snap["win_horizon"]


#: Error-flag bit of the product join's device guards (a log, arena or
#: segment position out of range): the host's bookkeeping is wrong.
_ERR_WJPROD_BOUND = 4


class WindowJoinProductState:
    """Two-sided join over tumbling event-time windows on device with
    "product" insert and "final" emit: the device twin of the host
    `join_window` with an `EventClock`, a `TumblingWindower`,
    ``insert_mode="product"`` and ``ordered=True``.

    Each (key, window) cell keeps every value of each side, duplicates
    included.  A close emits each cell of a due window once, as the
    rows of the product of its two value lists, an empty side counting
    as one absent value: a cell with n0 left and n1 right values gives
    ``max(n0, 1) * max(n1, 1)`` rows of the columns `keys`, `wins`,
    `v0`, `v1` and `mask` (bit ``s`` set: side ``s`` present; an absent
    side's value column reads 0).  All rows of a cell come out of one
    close.  The order of the rows is not defined, within a cell or
    across cells, and may differ from run to run: the contract is the
    multiset of ``(key, win, v0-or-absent, v1-or-absent)``.

    On device the state is a (window << 32 | key) table with a count
    per side and slot, and one append log per side of (cell, value)
    entries.  A close plans the due cells, gathers their values from
    the logs into an arena while it compacts the live entries into a
    fresh table and fresh logs, and expands the arena into rows (see
    k_wjprod_plan, k_wjprod_gather and k_wjprod_expand).  So table and
    logs only ever hold the open windows.  `log_cap` is the initial
    capacity of each side's log in entries; a log grows by doubling
    before an insert that could pass it, from a host-side bound on the
    live entries (`live_counts`), so it never overflows.

    The ordering contract is `WindowJoinState`'s without late
    tracking: nothing checks the order, and an event behind the closed
    horizon is dropped by the next close that has rows.  Timestamps
    only choose the window and move the watermark.

    A close whose row total exceeds `out_cap` raises `RuntimeError`
    with the exact total before anything is emitted or reclaimed: the
    state then holds what it held before.
    """

    def __init__(
        self,
        device,
        align_ms: int,
        len_ms: int,
        slots_pow: int = 20,
        out_cap: int = 1 << 20,
        wait_ms: int = 0,
        log_cap: int = 1 << 20,
    ):
        import torch

        if len_ms <= 0:
            msg = "window length must be positive"
            raise ValueError(msg)
        self.device = device
        self.align_ms = align_ms
        self.len_ms = len_ms
        self.wait_ms = wait_ms
        self.out_cap = out_cap
        self.max_ts_host = 0
        self.closed_horizon = -(1 << 62)
        self._log_caps = [max(1, log_cap)] * 2
        self.cpu = device.type == "cpu"
        if self.cpu:
            #: (key, win) -> [left values, right values].
            self._table: Dict[Tuple[int, int], List[List[int]]] = {}
            return
        self.k = ext()
        self.nslots = 1 << slots_pow
        self.tkeys, self.tcnt = self._new_table()
        #: The second table and logs that a close rebuilds the live
        #: entries into.  None until a close has rows to emit.
        self.table_alt: Optional[Tuple[Any, Any]] = None
        self.logs = [self._new_log(side) for side in (0, 1)]
        self.logs_alt: List[Any] = [None, None]
        #: Device cursors of the two logs: entries appended so far.
        self.log_n = torch.zeros(2, dtype=torch.int32, device=device)
        self.log_n_alt = torch.zeros(2, dtype=torch.int32, device=device)
        #: Upper bound on each log's entries: the cursor read back at
        #: the last close, less what that close took, plus the batch
        #: lengths inserted since.
        self._live = [0, 0]
        #: The plan's due-cell list and per-slot scratch, allocated by
        #: the first close.
        self._plan: Optional[Tuple[Any, Any, Any]] = None
        self.cells_n = torch.zeros(1, dtype=torch.int32, device=device)
        self.max_ts_dev = torch.zeros(1, dtype=torch.int64, device=device)
        self.error_flag = torch.zeros(1, dtype=torch.int32, device=device)

    def _new_table(self) -> Tuple[Any, Any]:
        import torch

        return (
            torch.full(
                (self.nslots,), -1, dtype=torch.int64, device=self.device
            ),
            torch.zeros(2 * self.nslots, dtype=torch.int32, device=self.device),
        )

    def _new_log(self, side: int):
        import torch

        return torch.empty(
            2 * self._log_caps[side], dtype=torch.int64, device=self.device
        )

    @property
    def log_caps(self) -> Tuple[int, int]:
        """Current capacity of each side's log, in entries."""
        return (self._log_caps[0], self._log_caps[1])

    @property
    def live_counts(self) -> Tuple[int, int]:
        """Entries each side holds.  On device this is the host's
        bound, without a synchronisation: exact unless the last close
        dropped events behind the closed horizon, and never too low."""
        if self.cpu:
            return (
                sum(len(c[0]) for c in self._table.values()),
                sum(len(c[1]) for c in self._table.values()),
            )
        return (self._live[0], self._live[1])

    def _reserve(self, side: int, n: int) -> None:
        """Room for `n` more entries in the side's log: grow it by
        doubling, copying the live prefix on the stream."""
        need = self._live[side] + n
        cap = self._log_caps[side]
        if need <= cap:
            return
        while cap < need:
            cap *= 2
        old = self.logs[side]
        self._log_caps[side] = cap
        self.logs[side] = self._new_log(side)
        live = 2 * self._live[side]
        self.logs[side][:live].copy_(old[:live])
        # The spare log is empty between closes: the next close makes
        # one of the new size.
        self.logs_alt[side] = None

    def insert(self, side: int, batch: RecordBatch) -> None:
        """Insert one side's batch (`side` 0 = left, 1 = right)."""
        if side not in (0, 1):
            msg = f"window join side must be 0 or 1, not {side!r}"
            raise ValueError(msg)
        if batch.vals is None:
            msg = "window join requires a `vals` column"
            raise ValueError(msg)
        n = len(batch)
        if self.cpu:
            self._insert_cpu(side, batch)
            return
        if n:
            self._reserve(side, n)
            self.k.wjprod_insert(
                batch.keys,
                batch.ts,
                batch.vals,
                self.tkeys,
                self.tcnt,
                self.logs[side],
                self.log_n,
                side,
                self.max_ts_dev,
                self.error_flag,
                self.align_ms,
                self.len_ms,
                batch.ts_base,
            )
            self._live[side] += n
        if batch.max_ts is not None:
            if batch.max_ts > self.max_ts_host:
                self.max_ts_host = batch.max_ts
        elif n:
            # No host-side hint: the watermark has to come back from
            # the device.
            dev_max = int(self.max_ts_dev.item())
            if dev_max > self.max_ts_host:
                self.max_ts_host = dev_max

    def _insert_cpu(self, side: int, batch: RecordBatch) -> None:
        import torch

        keys = batch.keys.tolist()
        ts = (batch.ts.to(torch.int64) + batch.ts_base).tolist()
        vals = batch.vals.tolist()
        for k, t, v in zip(keys, ts, vals):
            kw = (k, (t - self.align_ms) // self.len_ms)
            cell = self._table.get(kw)
            if cell is None:
                cell = self._table[kw] = [[], []]
            cell[side].append(v)
        mx_ts = batch.max_ts
        if mx_ts is None and ts:
            mx_ts = max(ts)
        if mx_ts is not None and mx_ts > self.max_ts_host:
            self.max_ts_host = mx_ts

    def _win_lo(self) -> int:
        return max(self.closed_horizon, -(1 << 39))

    def _too_many(self, rows: int) -> None:
        if rows > self.out_cap:
            msg = (
                f"window product join close has {rows} rows > out_cap "
                f"{self.out_cap}; nothing was emitted or reclaimed"
            )
            raise RuntimeError(msg)

    def close_due(
        self, wait_ms: Optional[int] = None
    ) -> Optional[Dict[str, Any]]:
        """Emit every window fully below the watermark (`max_ts_host`
        minus `wait_ms`, the constructor's by default) and reclaim its
        space; None when nothing was due.  See :meth:`close_below`."""
        return self.close_below(self.horizon_for(self.max_ts_host, wait_ms))

    def horizon_for(
        self, watermark_ms: int, wait_ms: Optional[int] = None
    ) -> int:
        """The window horizon of a watermark: every window below it
        ends at or before `watermark_ms` minus `wait_ms` (the
        constructor's by default).  What :meth:`close_below` takes."""
        if wait_ms is None:
            wait_ms = self.wait_ms
        return (watermark_ms - wait_ms - self.align_ms) // self.len_ms

    def close_eof(self) -> Optional[Dict[str, Any]]:
        """End of input, as the operator closes it: the rows of every
        cell at or above the closed horizon, with the horizon left
        where it is and the state left empty."""
        return self._close(self._win_lo(), 1 << 40)

    def close_all(self) -> Optional[Dict[str, Any]]:
        """EOF: the rows of every cell at or above the closed horizon;
        the state is left empty and nothing is emitted after it."""
        out = self._close(self._win_lo(), 1 << 40)
        self.closed_horizon = 1 << 40
        return out

    def close_below(self, horizon: int) -> Optional[Dict[str, Any]]:
        """Close with reclamation: return the rows of the cells of
        windows in [closed_horizon, horizon), each cell exactly once
        and whole, keep the events at or above `horizon`, forget
        everything below it and advance `closed_horizon` to `horizon`.
        An event below `closed_horizon` (one behind the watermark) was
        never going to be emitted; it is dropped here, on device by
        the next close that has rows."""
        if horizon <= self.closed_horizon:
            return None
        out = self._close(self._win_lo(), min(horizon, 1 << 40))
        self.closed_horizon = horizon
        return out

    def _close(self, win_lo: int, win_hi: int) -> Optional[Dict[str, Any]]:
        import torch

        if self.cpu:
            return self._close_cpu(win_lo, win_hi)
        if self._plan is None:
            self._plan = (
                torch.empty(self.nslots, dtype=torch.int64, device=self.device),
                torch.empty(
                    2 * self.nslots, dtype=torch.int32, device=self.device
                ),
                torch.empty(self.nslots, dtype=torch.int32, device=self.device),
            )
        cell_pk, cell_n, slot_cell = self._plan
        self.cells_n.zero_()
        self.k.wjprod_plan(
            self.tkeys, self.tcnt, win_lo, win_hi,
            cell_pk, cell_n, slot_cell, self.cells_n,
        )
        # A cell holds at least one entry, so the list is no longer
        # than the host's bound on the entries; rows past the list's
        # end hold earlier closes' cells and count for nothing.
        ub = max(1, min(self.nslots, self._live[0] + self._live[1]))
        nn = cell_n[: 2 * ub].view(ub, 2).to(torch.int64)
        listed = (
            torch.arange(ub, device=self.device) < self.cells_n
        ).to(torch.int64)
        n0, n1 = nn[:, 0] * listed, nn[:, 1] * listed
        val_end = torch.cumsum(n0 + n1, 0)
        row_end = torch.cumsum(
            n0.clamp(min=1) * n1.clamp(min=1) * listed, 0
        )
        # The one readback of a close: list length, row and value
        # totals, the error flag and both log cursors.
        ncells, rows, nvals, due0, flag, cur0, cur1 = torch.cat(
            [
                self.cells_n.to(torch.int64),
                row_end[-1:],
                val_end[-1:],
                n0.sum().reshape(1),
                self.error_flag.to(torch.int64),
                self.log_n.to(torch.int64),
            ]
        ).tolist()
        if flag & _ERR_WJPROD_BOUND:
            msg = (
                "window product join wrote past a log or arena bound on "
                "device; this is a bug in the host-side bound"
            )
            raise RuntimeError(msg)
        _check_error_flag(flag, "window product join table")
        if ncells > ub:
            msg = "window product join: more due cells than live entries"
            raise RuntimeError(msg)
        self._too_many(rows)
        self._live = [cur0, cur1]
        if ncells == 0:
            # Nothing due, so nothing to reclaim yet.
            return None
        if self.table_alt is None:
            self.table_alt = self._new_table()
        for side in (0, 1):
            if self.logs_alt[side] is None:
                self.logs_alt[side] = self._new_log(side)
        arena = torch.empty(nvals, dtype=torch.int64, device=self.device)
        for side, cur in ((0, cur0), (1, cur1)):
            self.k.wjprod_gather(
                self.logs[side], cur, side, self.tkeys, self.tcnt,
                self.log_n, win_lo, win_hi, slot_cell, cell_n, val_end,
                ncells, arena, *self.table_alt, self.logs_alt[side],
                self.log_n_alt, self.error_flag,
            )
        out = {
            name: torch.empty(
                rows,
                dtype=torch.int64 if name[0] == "v" else torch.int32,
                device=self.device,
            )
            for name in _WJOIN_COLS
        }
        self.k.wjprod_expand(
            rows, ncells, row_end, val_end, cell_pk, cell_n, arena,
            *(out[c] for c in _WJOIN_COLS),
        )
        retired = (self.tkeys, self.tcnt)
        self.tkeys, self.tcnt = self.table_alt
        self.table_alt = retired
        self.logs, self.logs_alt = self.logs_alt, self.logs
        self.log_n, self.log_n_alt = self.log_n_alt, self.log_n
        # Reset the retired table and cursors on the stream for the
        # next close; the retired logs need none.
        retired[0].fill_(-1)
        retired[1].zero_()
        self.log_n_alt.zero_()
        self._live = [cur0 - due0, cur1 - (nvals - due0)]
        return out

    def _close_cpu(self, win_lo: int, win_hi: int) -> Optional[Dict[str, Any]]:
        import torch

        hit = [
            (k, w, c)
            for (k, w), c in self._table.items()
            if win_lo <= w < win_hi
        ]
        self._too_many(
            sum(max(len(c[0]), 1) * max(len(c[1]), 1) for *_x, c in hit)
        )
        for kw in [kw for kw in self._table if kw[1] < win_hi]:
            del self._table[kw]
        if not hit:
            return None
        rows = [
            (k, w, a, b)
            for k, w, c in hit
            for a in (c[0] or [None])
            for b in (c[1] or [None])
        ]
        return {
            "keys": torch.tensor([r[0] for r in rows], dtype=torch.int32),
            "wins": torch.tensor([r[1] for r in rows], dtype=torch.int32),
            "v0": torch.tensor(
                [0 if r[2] is None else r[2] for r in rows], dtype=torch.int64
            ),
            "v1": torch.tensor(
                [0 if r[3] is None else r[3] for r in rows], dtype=torch.int64
            ),
            "mask": torch.tensor(
                [(r[2] is not None) | ((r[3] is not None) << 1) for r in rows],
                dtype=torch.int32,
            ),
        }

    def snapshot_to_host(self) -> Dict[str, Any]:
        """Spill the live events of windows at or above the closed
        horizon as columns `keys`, `wins`, `sides` and `vals`, with
        the watermark, the closed horizon, the window geometry and a
        kind tag.  Nothing on the device is changed."""
        import numpy as np

        if self.cpu:
            ev = [
                (k, w, side, v)
                for (k, w), c in self._table.items()
                if w >= self.closed_horizon
                for side in (0, 1)
                for v in c[side]
            ]
            cols = [
                np.array([e[j] for e in ev], dtype=dt)
                for j, dt in enumerate((np.int32, np.int32, np.int32, np.int64))
            ]
        else:
            cur = self.log_n.tolist()
            _check_error_flag(
                int(self.error_flag.item()), "window product join table"
            )
            parts = []
            for side in (0, 1):
                log = self.logs[side][: 2 * cur[side]].cpu().numpy()
                packed, vals = log[0::2], log[1::2]
                wins = (packed >> 32).astype(np.int32)
                keys = (packed & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
                live = wins.astype(np.int64) >= self.closed_horizon
                parts.append(
                    (
                        keys[live],
                        wins[live],
                        np.full(int(live.sum()), side, dtype=np.int32),
                        vals[live].copy(),
                    )
                )
            cols = [np.concatenate(c) for c in zip(*parts)]
        return {
            "kind": _WJPROD_KIND,
            "max_ts": self.max_ts_host,
            "closed_horizon": self.closed_horizon,
            "align_ms": self.align_ms,
            "len_ms": self.len_ms,
            "n": len(cols[0]),
            "keys": cols[0],
            "wins": cols[1],
            "sides": cols[2],
            "vals": cols[3],
        }

    def restore_from_host(self, snap: Dict[str, Any]) -> None:
        """Re-insert the live events, each at the start of its window:
        the timestamp of an event only ever chose its window.  A
        snapshot of another geometry, or of a "first" / "last" or
        sliding window join, is refused."""
        import torch

        if snap.get("kind") != _WJPROD_KIND:
            msg = (
                "snapshot of another kind of window join cannot restore a "
                "window product join"
            )
            raise ValueError(msg)
        theirs = (snap.get("align_ms"), snap.get("len_ms"))
        mine = (self.align_ms, self.len_ms)
        if theirs != mine:
            msg = (
                "snapshot of a window product join with (align_ms, len_ms) "
                f"= {theirs} cannot restore one with {mine}"
            )
            raise ValueError(msg)
        if snap["n"]:
            for side in (0, 1):
                m = snap["sides"] == side
                if not m.any():
                    continue
                ts = self.align_ms + snap["wins"][m].astype("int64") * self.len_ms
                self.insert(
                    side,
                    RecordBatch(
                        torch.as_tensor(snap["keys"][m]).to(self.device),
                        torch.as_tensor(ts).to(self.device),
                        torch.as_tensor(snap["vals"][m]).to(self.device),
                        max_ts=snap["max_ts"],
                    ),
                )
        self.max_ts_host = snap["max_ts"]
        self.closed_horizon = snap["closed_horizon"]


class SessionAggState:
    """Gap-based session aggregation state on device.

    One cell per key: (session_start, last_ts, accumulator).  Batches
    are sorted by (key, ts) on insert and one thread walks each key's
    segment in order (parallelism = distinct keys — built for
    high-cardinality streams; low-cardinality session streams belong
    on the host path's `SessionWindower`).  A gap > ``gap_ms`` closes
    the running session; the watermark close emits sessions idle past
    ``watermark - gap``.  Role parity: reference
    windowing.py _SessionWindowerLogic under watermark-ordered input
    (in-order ingestion makes merges degenerate to extension).

    ``ordered=False`` drops the ordering assumption: a key's cell
    holds up to ``max_open`` (4, 8, 16 or 32) open sessions sorted by
    start, a batch is collapsed into gap-separated runs in parallel
    over events and merged into the cell, so an event may extend a
    session backwards or bridge two of them.  The watermark is the
    max event ts over all earlier batches; an event older than
    ``watermark - wait_ms`` is late and `insert` hands it back instead
    of applying it.  Insert never closes a session on this path; only
    `close_due` (sessions with ``last < watermark - wait_ms - gap``)
    and `close_all` do.  A key that would need more than ``max_open``
    sessions raises on the next drain.
    """

    def __init__(
        self,
        device,
        gap_ms: int,
        mode: int = AGG_COUNT,
        slots_pow: int = 20,
        out_cap: int = 1 << 20,
        ordered: bool = True,
        max_open: int = 8,
        wait_ms: int = 0,
    ):
        import torch

        if max_open not in (4, 8, 16, 32):
            msg = f"max_open must be 4, 8, 16 or 32; got {max_open!r}"
            raise ValueError(msg)
        self.device = device
        self.cpu = device.type == "cpu"
        self.gap_ms = gap_ms
        self.mode = mode
        self.max_ts_host = 0
        self.ordered = ordered
        self.max_open = max_open
        #: Lateness allowance of the unordered path (ordered mode takes
        #: it per `close_due` call, as before).
        self.wait_ms = wait_ms
        if not ordered:
            self._init_unordered(slots_pow, out_cap)
            return
        if self.cpu:
            self._table: Dict[int, Tuple[int, int, int]] = {}
            self._closed: List[Tuple[int, int, int, int]] = []
            return
        self.k = ext()
        self.nslots = 1 << slots_pow
        mk = lambda fill: torch.full(  # noqa: E731
            (self.nslots,), fill, dtype=torch.int64, device=device
        )
        self.skeys, self.sstart = mk(-1), mk(0)
        self.slast, self.sacc = mk(-1), mk(0)
        self.skeys_alt, self.sstart_alt = mk(-1), mk(0)
        self.slast_alt, self.sacc_alt = mk(-1), mk(0)
        self.out_cap = out_cap
        self.out_keys = torch.empty(out_cap, dtype=torch.int32, device=device)
        self.out_start = torch.empty(out_cap, dtype=torch.int64, device=device)
        self.out_end = torch.empty(out_cap, dtype=torch.int64, device=device)
        self.out_vals = torch.empty(out_cap, dtype=torch.int64, device=device)
        self.out_n = torch.zeros(1, dtype=torch.int32, device=device)
        self.max_ts_dev = torch.zeros(1, dtype=torch.int64, device=device)
        self.error_flag = torch.zeros(1, dtype=torch.int32, device=device)

    def _sort(self, batch: RecordBatch):
        import torch

        order = torch.argsort(batch.ts, stable=True)
        k1 = batch.keys[order]
        order2 = torch.argsort(k1.to(torch.int64), stable=True)
        perm = order[order2]
        keys = batch.keys[perm]
        ts = batch.ts[perm].to(torch.int64) + batch.ts_base
        vals = batch.vals[perm] if batch.vals is not None else None
        return keys, ts, vals

    def _insert_cpu(self, batch: RecordBatch) -> None:
        keys, ts, vals = self._sort(batch)
        it = zip(
            keys.tolist(),
            ts.tolist(),
            vals.tolist() if vals is not None else [1] * len(keys),
        )
        for k, t, v in it:
            if self.mode == AGG_COUNT:
                v = 1
            cur = self._table.get(k)
            if cur is not None and t - cur[1] > self.gap_ms:
                self._closed.append((k, cur[0], cur[1], cur[2]))
                cur = None
            if cur is None:
                self._table[k] = (t, t, v)
            else:
                self._table[k] = (cur[0], t, cur[2] + v)
            if t > self.max_ts_host:
                self.max_ts_host = t

    def _insert_batch_fast(self, batch: RecordBatch) -> None:
        """Batch-level fast path (COUNT, gap >= batch span): no
        session boundary can fall inside the batch, so each key's
        per-batch (count, min_ts, max_ts) merges as one unit — fused
        into ONE radix pass: AGG_TS scatter partitions (key, t) pairs
        into segments, one block LDS-aggregates each segment and
        merges its distinct keys straight into the session table
        (round-2 rework: replaces the stats-table round trip and its
        five per-batch table clears)."""
        import torch

        n = len(batch)
        if not hasattr(self, "rx_gcursors"):
            # Segment count ~nslots/2^seg_bits; LDS staging in the agg
            # covers up to 2^12 distinct keys per segment.
            self.seg_bits = max(self.nslots.bit_length() - 1 - 10, 1)
            nseg = self.nslots >> self.seg_bits
            self.rx_gcursors = torch.zeros(
                nseg, dtype=torch.int32, device=self.device
            )
            self.rx_ov_cursor = torch.zeros(
                1, dtype=torch.int32, device=self.device
            )
            self.rx_max_batch = 0
            self.rx_packed = torch.empty(1, dtype=torch.int64, device=self.device)
            self.rx_vals = torch.empty(1, dtype=torch.int64, device=self.device)
            self.rx_ov_packed = torch.empty(
                1, dtype=torch.int64, device=self.device
            )
            self.rx_ov_vals = torch.empty(
                1, dtype=torch.int64, device=self.device
            )
        if n > self.rx_max_batch:
            mb = int(n * 5 // 4)
            self.rx_max_batch = mb
            nseg = self.nslots >> self.seg_bits
            per_seg = max(64, -(-mb * 5 // 2) // nseg + 1)
            total = per_seg * nseg
            self.rx_packed = torch.empty(
                total, dtype=torch.int64, device=self.device
            )
            self.rx_vals = torch.empty(
                total, dtype=torch.int64, device=self.device
            )
            ov = max(1 << 20, mb)
            self.rx_ov_packed = torch.empty(
                ov, dtype=torch.int64, device=self.device
            )
            self.rx_ov_vals = torch.empty(
                ov, dtype=torch.int64, device=self.device
            )
        self.k.session_radix_insert(
            batch.keys,
            batch.ts,
            batch.ts_base,
            self.gap_ms,
            self.skeys, self.sstart, self.slast, self.sacc,
            self.rx_gcursors, self.rx_packed, self.rx_vals,
            self.rx_ov_cursor, self.rx_ov_packed, self.rx_ov_vals,
            self.out_keys, self.out_start, self.out_end, self.out_vals,
            self.out_n, self.max_ts_dev, self.error_flag,
            self.seg_bits,
        )
        if batch.max_ts is not None and batch.max_ts > self.max_ts_host:
            self.max_ts_host = batch.max_ts

    def insert(self, batch: RecordBatch) -> Optional[RecordBatch]:
        """Apply one batch.  Returns the batch's late events on the
        unordered path (None if there are none); always None in
        ordered mode."""
        import torch

        if len(batch) == 0:
            return None
        if not self.ordered:
            return self._insert_unordered(batch)
        if self.cpu:
            self._insert_cpu(batch)
            if (
                batch.max_ts is not None
                and batch.max_ts > self.max_ts_host
            ):
                self.max_ts_host = batch.max_ts
            return
        if (
            self.mode == AGG_COUNT
            and batch.ts_base != 0
            and batch.max_ts is not None
            and self.gap_ms >= (batch.max_ts - batch.ts_base)
        ):
            # Producers shipping a zero-based template guarantee
            # ts in [0, max_ts - ts_base]; with the gap at least that
            # span, the batch-level merge is exact.
            self._insert_batch_fast(batch)
            return
        keys, ts, vals = self._sort(batch)
        neq = keys[1:] != keys[:-1]
        idx = torch.nonzero(neq).flatten() + 1
        zero = torch.zeros(1, dtype=torch.int64, device=self.device)
        seg_start = torch.cat([zero, idx])
        n = torch.full((1,), len(keys), dtype=torch.int64, device=self.device)
        seg_end = torch.cat([idx, n])
        self.k.session_insert(
            keys, ts, vals, seg_start, seg_end,
            self.skeys, self.sstart, self.slast, self.sacc,
            self.out_keys, self.out_start, self.out_end, self.out_vals,
            self.out_n, self.max_ts_dev, self.error_flag,
            self.gap_ms, self.mode,
        )
        if batch.max_ts is not None and batch.max_ts > self.max_ts_host:
            self.max_ts_host = batch.max_ts

    def _drain_out(self) -> Optional[Dict[str, Any]]:
        if not self.ordered:
            self._check_max_open()
        if self.cpu:
            if not self._closed:
                return None
            import torch

            rows = self._closed
            self._closed = []
            return {
                "keys": torch.tensor([r[0] for r in rows], dtype=torch.int32),
                "start": torch.tensor([r[1] for r in rows], dtype=torch.int64),
                "end": torch.tensor([r[2] for r in rows], dtype=torch.int64),
                "vals": torch.tensor([r[3] for r in rows], dtype=torch.int64),
            }
        n = int(self.out_n.item())
        if int(self.error_flag.item()) != 0:
            msg = "session state overflow; increase slots_pow/out_cap"
            raise RuntimeError(msg)
        if hasattr(self, "_bs") and int(self._bs.error_flag.item()) != 0:
            msg = "session batch-stats overflow; increase slots_pow"
            raise RuntimeError(msg)
        if n == 0:
            return None
        out = {
            "keys": self.out_keys[:n].clone(),
            "start": self.out_start[:n].clone(),
            "end": self.out_end[:n].clone(),
            "vals": self.out_vals[:n].clone(),
        }
        self.out_n.zero_()
        return out

    def close_due(
        self, wait_ms: Optional[int] = None
    ) -> Optional[Dict[str, Any]]:
        """Emit sessions idle past watermark - gap (plus any closed by
        gaps during inserts since the last drain).  The unordered path
        closes with the allowance it was built with."""
        if not self.ordered:
            if wait_ms is not None and wait_ms != self.wait_ms:
                msg = (
                    "unordered session state closes with its own "
                    f"wait_ms={self.wait_ms}; got {wait_ms}"
                )
                raise ValueError(msg)
            return self._close_unordered(
                self.max_ts_host - self.gap_ms - self.wait_ms
            )
        if wait_ms is None:
            wait_ms = 0
        horizon = self.max_ts_host - self.gap_ms - wait_ms
        if self.cpu:
            for k in list(self._table):
                s, last, acc = self._table[k]
                if last < horizon:
                    self._closed.append((k, s, last, acc))
                    del self._table[k]
            return self._drain_out()
        self.k.session_close_migrate(
            self.skeys, self.sstart, self.slast, self.sacc,
            self.skeys_alt, self.sstart_alt, self.slast_alt, self.sacc_alt,
            self.out_keys, self.out_start, self.out_end, self.out_vals,
            self.out_n, self.error_flag, horizon,
        )
        self._swap_reset()
        return self._drain_out()

    def _swap_reset(self) -> None:
        self.skeys, self.skeys_alt = self.skeys_alt, self.skeys
        self.sstart, self.sstart_alt = self.sstart_alt, self.sstart
        self.slast, self.slast_alt = self.slast_alt, self.slast
        self.sacc, self.sacc_alt = self.sacc_alt, self.sacc
        self.skeys_alt.fill_(-1)
        self.slast_alt.fill_(-1)
        self.sstart_alt.zero_()
        self.sacc_alt.zero_()

    def close_all(self) -> Optional[Dict[str, Any]]:
        if not self.ordered:
            return self._close_unordered(1 << 60)
        if self.cpu:
            for k in list(self._table):
                s, last, acc = self._table[k]
                self._closed.append((k, s, last, acc))
            self._table.clear()
            return self._drain_out()
        self.k.session_close_migrate(
            self.skeys, self.sstart, self.slast, self.sacc,
            self.skeys_alt, self.sstart_alt, self.slast_alt, self.sacc_alt,
            self.out_keys, self.out_start, self.out_end, self.out_vals,
            self.out_n, self.error_flag, 1 << 60,
        )
        self._swap_reset()
        return self._drain_out()

    def snapshot_to_host(self) -> Dict[str, Any]:
        import numpy as np

        if not self.ordered:
            return self._snapshot_unordered()
        if self.cpu:
            items = list(self._table.items())
            return {
                "keys": np.array([k for k, _ in items], dtype="int32"),
                "start": np.array([v[0] for _, v in items], dtype="int64"),
                "last": np.array([v[1] for _, v in items], dtype="int64"),
                "acc": np.array([v[2] for _, v in items], dtype="int64"),
                "max_ts": self.max_ts_host,
                "pending": list(self._closed),
            }
        live = (self.skeys >= 0) & (self.slast >= 0)
        # Sessions closed by gaps during insert() but not yet drained
        # sit in the out buffer; persist them (without draining — a
        # snapshot must not mutate) so a restore re-emits them exactly
        # once, mirroring the CPU twin's `_closed` list.
        pend_n = int(self.out_n.item())
        pending = [
            (int(k), int(s), int(e), int(v))
            for k, s, e, v in zip(
                self.out_keys[:pend_n].cpu().tolist(),
                self.out_start[:pend_n].cpu().tolist(),
                self.out_end[:pend_n].cpu().tolist(),
                self.out_vals[:pend_n].cpu().tolist(),
            )
        ]
        return {
            "keys": self.skeys[live].to("cpu").numpy().astype("int32"),
            "start": self.sstart[live].cpu().numpy().copy(),
            "last": self.slast[live].cpu().numpy().copy(),
            "acc": self.sacc[live].cpu().numpy().copy(),
            "max_ts": self.max_ts_host,
            "pending": pending,
        }

    def restore_from_host(self, snap: Dict[str, Any]) -> None:
        import torch

        if bool(snap.get("ordered", True)) != self.ordered:
            msg = (
                "session snapshot was taken with ordered="
                f"{bool(snap.get('ordered', True))}; this state has "
                f"ordered={self.ordered}"
            )
            raise ValueError(msg)
        if not self.ordered:
            self._restore_unordered(snap)
            return
        self.max_ts_host = snap["max_ts"]
        if self.cpu:
            for k, s, last, acc in zip(
                snap["keys"].tolist(), snap["start"].tolist(),
                snap["last"].tolist(), snap["acc"].tolist(),
            ):
                self._table[int(k)] = (int(s), int(last), int(acc))
            self._closed.extend(
                tuple(r) for r in snap.get("pending", [])
            )
            return
        pending = snap.get("pending", [])
        if pending:
            # Re-stage snapshotted closed-but-undrained sessions into
            # the out buffer; the next drain re-emits them.
            n0 = int(self.out_n.item())
            n1 = n0 + len(pending)
            if n1 > self.out_cap:
                msg = "session restore overflows out_cap"
                raise RuntimeError(msg)
            self.out_keys[n0:n1] = torch.tensor(
                [r[0] for r in pending], dtype=torch.int32
            ).to(self.device)
            self.out_start[n0:n1] = torch.tensor(
                [r[1] for r in pending], dtype=torch.int64
            ).to(self.device)
            self.out_end[n0:n1] = torch.tensor(
                [r[2] for r in pending], dtype=torch.int64
            ).to(self.device)
            self.out_vals[n0:n1] = torch.tensor(
                [r[3] for r in pending], dtype=torch.int64
            ).to(self.device)
            self.out_n.fill_(n1)
        if len(snap["keys"]) == 0:
            return
        self.k.session_restore(
            torch.as_tensor(snap["keys"]).to(self.device),
            torch.as_tensor(snap["start"]).to(self.device),
            torch.as_tensor(snap["last"]).to(self.device),
            torch.as_tensor(snap["acc"]).to(self.device),
            self.skeys, self.sstart, self.slast, self.sacc,
            self.error_flag,
        )

    # -- ordered=False: several open sessions per key -------------------

    def _init_unordered(self, slots_pow: int, out_cap: int) -> None:
        import torch

        self._max_open_hit = False
        if self.cpu:
            # key -> [[start, last, acc], ...] sorted by start, any two
            # neighbours more than the gap apart.
            self._open: Dict[int, List[List[int]]] = {}
            self._closed: List[Tuple[int, int, int, int]] = []
            return
        device = self.device
        self.k = ext()
        self.nslots = 1 << slots_pow

        def table():
            return (
                torch.full(
                    (self.nslots,), -1, dtype=torch.int64, device=device
                ),
                torch.zeros(self.nslots, dtype=torch.int32, device=device),
            ) + tuple(
                torch.zeros(
                    (self.nslots, self.max_open),
                    dtype=torch.int64,
                    device=device,
                )
                for _ in range(3)
            )

        (
            self.skeys, self.scnt, self.sstart, self.slast, self.sacc,
        ) = table()
        (
            self.skeys_alt, self.scnt_alt, self.sstart_alt,
            self.slast_alt, self.sacc_alt,
        ) = table()
        self.out_cap = out_cap
        self.out_keys = torch.empty(out_cap, dtype=torch.int32, device=device)
        self.out_start = torch.empty(out_cap, dtype=torch.int64, device=device)
        self.out_end = torch.empty(out_cap, dtype=torch.int64, device=device)
        self.out_vals = torch.empty(out_cap, dtype=torch.int64, device=device)
        self.out_n = torch.zeros(1, dtype=torch.int32, device=device)
        self.max_ts_dev = torch.zeros(1, dtype=torch.int64, device=device)
        self.error_flag = torch.zeros(1, dtype=torch.int32, device=device)

    def _check_max_open(self) -> None:
        hit = self._max_open_hit
        if not self.cpu:
            hit = (int(self.error_flag.item()) & 2) != 0
        if hit:
            msg = (
                "a key holds more simultaneously open sessions than "
                f"max_open={self.max_open}; increase max_open"
            )
            raise RuntimeError(msg)

    def _split_late(self, batch: RecordBatch):
        """(accepted, late) by the batch-granular watermark: the max
        event ts over all EARLIER batches, so a batch's own events
        never make each other late."""
        import torch

        cutoff = self.max_ts_host - self.wait_ms
        if cutoff <= 0:
            # Timestamps are >= 0: nothing can be late yet.
            return batch, None
        late = batch.ts < (cutoff - batch.ts_base)
        n_late = int(late.sum().item())
        if n_late == 0:
            return batch, None
        n = len(batch)

        def part(keys, ts, vals):
            return RecordBatch(
                keys, ts, vals, max_ts=None, ts_base=batch.ts_base
            )

        if self.cpu:
            keep = ~late
            pick = lambda m: part(  # noqa: E731
                batch.keys[m],
                batch.ts[m],
                batch.vals[m] if batch.vals is not None else None,
            )
            return (pick(keep) if n_late < n else None), pick(late)
        ts = batch.ts.to(torch.int64)
        out = []
        for mask, kept in ((~late, n - n_late), (late, n_late)):
            if kept == 0:
                out.append(None)
                continue
            keys_o = torch.empty(kept, dtype=torch.int32, device=self.device)
            ts_o = torch.empty(kept, dtype=torch.int64, device=self.device)
            vals_o = torch.empty(
                kept if batch.vals is not None else 0,
                dtype=torch.int64,
                device=self.device,
            )
            out_n = torch.zeros(1, dtype=torch.int32, device=self.device)
            self.k.filter_compact(
                batch.keys, ts, batch.vals, mask.to(torch.uint8),
                keys_o, ts_o, vals_o, out_n,
            )
            out.append(
                part(keys_o, ts_o, vals_o if batch.vals is not None else None)
            )
        return out[0], out[1]

    def _insert_unordered(self, batch: RecordBatch) -> Optional[RecordBatch]:
        if self.mode == AGG_SUM and batch.vals is None:
            msg = "sum sessions require a `vals` column"
            raise ValueError(msg)
        bmax = batch.max_ts
        if bmax is None:
            bmax = int(batch.ts.max().item()) + batch.ts_base
        accepted, late = self._split_late(batch)
        if accepted is not None:
            keys, ts, vals = self._sort(accepted)
            if self.cpu:
                self._merge_sorted_cpu(keys, ts, vals)
            else:
                runs = self.k.session_run_collapse(
                    keys.contiguous(), ts.contiguous(),
                    vals.contiguous() if self.mode == AGG_SUM else None,
                    self.gap_ms, self.mode,
                )
                self.k.session_run_merge(
                    *runs,
                    self.skeys, self.scnt, self.sstart, self.slast,
                    self.sacc, self.max_ts_dev, self.error_flag,
                    self.gap_ms, self.max_open,
                )
        if bmax > self.max_ts_host:
            self.max_ts_host = bmax
        return late

    def _merge_sorted_cpu(self, keys, ts, vals) -> None:
        """Twin of run collapse + run merge: the executable spec."""
        ks, tl = keys.tolist(), ts.tolist()
        vl = vals.tolist() if self.mode == AGG_SUM else [1] * len(ks)
        per_key: Dict[int, List[List[int]]] = {}
        prev_k = prev_t = None
        for k, t, v in zip(ks, tl, vl):
            if k != prev_k or t - prev_t > self.gap_ms:
                per_key.setdefault(k, []).append([t, t, v])
            else:
                run = per_key[k][-1]
                run[1] = t
                run[2] += v
            prev_k, prev_t = k, t
        for k, runs in per_key.items():
            self._merge_runs_cpu(k, runs)

    def _merge_runs_cpu(self, k: int, runs: List[List[int]]) -> None:
        cell = self._open.get(k, [])
        merged: List[List[int]] = []
        # Stable sort keeps cell sessions ahead of equal-start runs,
        # like the kernel's two-pointer merge.
        for s, last, acc in sorted(cell + runs, key=lambda r: r[0]):
            if merged and s - merged[-1][1] <= self.gap_ms:
                cur = merged[-1]
                cur[1] = max(cur[1], last)
                cur[2] += acc
            else:
                merged.append([s, last, acc])
        if len(merged) > self.max_open:
            self._max_open_hit = True  # cell left as it was
            return
        self._open[k] = merged

    def _close_unordered(self, horizon: int) -> Optional[Dict[str, Any]]:
        if self.cpu:
            for k in list(self._open):
                cell = self._open[k]
                p = 0
                while p < len(cell) and cell[p][1] < horizon:
                    s, last, acc = cell[p]
                    self._closed.append((k, s, last, acc))
                    p += 1
                if p == len(cell):
                    del self._open[k]
                elif p:
                    self._open[k] = cell[p:]
            return self._drain_out()
        self.k.session_multi_close_migrate(
            self.skeys, self.scnt, self.sstart, self.slast, self.sacc,
            self.skeys_alt, self.scnt_alt, self.sstart_alt,
            self.slast_alt, self.sacc_alt,
            self.out_keys, self.out_start, self.out_end, self.out_vals,
            self.out_n, self.error_flag, horizon, self.max_open,
        )
        for name in ("skeys", "scnt", "sstart", "slast", "sacc"):
            cur, alt = getattr(self, name), getattr(self, name + "_alt")
            setattr(self, name, alt)
            setattr(self, name + "_alt", cur)
        # The count gates every read of a cell's sessions.
        self.skeys_alt.fill_(-1)
        self.scnt_alt.zero_()
        return self._drain_out()

    def _snapshot_unordered(self) -> Dict[str, Any]:
        import numpy as np
        import torch

        if self.cpu:
            rows = [
                (k, s, last, acc)
                for k, cell in self._open.items()
                for s, last, acc in cell
            ]
        else:
            live = (self.skeys >= 0)[:, None] & (
                torch.arange(self.max_open, device=self.device)[None, :]
                < self.scnt[:, None]
            )
            keys = self.skeys[:, None].expand(-1, self.max_open)[live]
            rows = list(
                zip(
                    keys.cpu().tolist(),
                    self.sstart[live].cpu().tolist(),
                    self.slast[live].cpu().tolist(),
                    self.sacc[live].cpu().tolist(),
                )
            )
        rows.sort()
        return {
            "keys": np.array([r[0] for r in rows], dtype="int32"),
            "start": np.array([r[1] for r in rows], dtype="int64"),
            "last": np.array([r[2] for r in rows], dtype="int64"),
            "acc": np.array([r[3] for r in rows], dtype="int64"),
            "max_ts": self.max_ts_host,
            # Insert never closes here, so nothing waits undrained.
            "pending": [],
            "ordered": False,
        }

    def _restore_unordered(self, snap: Dict[str, Any]) -> None:
        import numpy as np
        import torch

        self.max_ts_host = snap["max_ts"]
        n = len(snap["keys"])
        if n == 0:
            return
        # Rows are runs already: sorted by (key, start) they merge
        # into the table exactly like a collapsed batch.
        order = np.lexsort((snap["start"], snap["keys"]))
        cols = [
            np.asarray(snap[name])[order]
            for name in ("keys", "start", "last", "acc")
        ]
        if self.cpu:
            per_key: Dict[int, List[List[int]]] = {}
            for k, s, last, acc in zip(*(c.tolist() for c in cols)):
                per_key.setdefault(int(k), []).append([s, last, acc])
            for k, runs in per_key.items():
                self._merge_runs_cpu(k, runs)
            return
        dev = [torch.as_tensor(c).to(self.device) for c in cols]
        self.k.session_run_merge(
            dev[0].to(torch.int32), dev[1], dev[2], dev[3],
            torch.full((1,), n, dtype=torch.int64, device=self.device),
            self.skeys, self.scnt, self.sstart, self.slast, self.sacc,
            self.max_ts_dev, self.error_flag,
            self.gap_ms, self.max_open,
        )
