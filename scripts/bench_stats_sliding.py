"""Cost of sliding stats windows built from panes.

Three measurements, all in one process, the sides alternating call by
call:

    python scripts/bench_stats_sliding.py close   [--reps 60]
    python scripts/bench_stats_sliding.py insert  [--reps 5]
    python scripts/bench_stats_sliding.py sustain [--reps 3]

`close`: a 2^22-slot pane table of a 60 s / 20 s `SlidingStatsAggState`
(panes of 20 s, three per window) with 10 % and 40 % of the slots
occupied, the cells spread evenly over panes 0 .. 5.  Closes window 0:
panes 0 .. 2, half of the cells, fold into it, pane 0 dies and panes
1 .. 5 migrate.  Times `stats_pane_close`, the `stats_extract` over
the fold table and the five fills that reset it, against
`stats_close_migrate` of pane 0 on the same table, and prints the
bytes each must move, computed from the shapes, and the fold atomics.

`insert`: insert time per batch of the sliding state against a
tumbling `StatsAggState` of the pane width on the same batches, with a
second tumbling state as the measure of the run's own spread.

`sustain`: events per second of `keyed_stats_agg` through `run_main`,
60 s windows every 20 s beside tumbling 20 s windows (host clock
around the run, which ends in a device synchronise).

Each mode prints one JSON line; `--out FILE` also writes it there.
"""

import argparse
import json
import statistics
import sys
import time
from datetime import datetime, timedelta, timezone
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from bytewax_amd.gpu import RecordBatch  # noqa: E402
from bytewax_amd.gpu._ext import ext  # noqa: E402
from bytewax_amd.gpu.state import (  # noqa: E402
    SlidingStatsAggState,
    StatsAggState,
)

p = argparse.ArgumentParser()
p.add_argument("mode", choices=["close", "insert", "sustain"])
p.add_argument("--reps", type=int, default=None)
p.add_argument("--warmup", type=int, default=10)
p.add_argument("--out", default=None)
args = p.parse_args()

k = ext()
dev = torch.device("cuda:0")
ALIGN = datetime(2024, 1, 1, tzinfo=timezone.utc)
ALIGN_MS, LEN, OFF, PANE = 1_704_067_200_000, 60_000, 20_000, 20_000
SLOTS_POW = 22
NSLOTS = 1 << SLOTS_POW
FILLS = (-1, 0, 0, (1 << 63) - 1, -(1 << 63))
N_PANES = 6


def events():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(
        enable_timing=True
    )


def summary(ms):
    q = statistics.quantiles(ms, n=10)
    return {
        "median_ms": round(statistics.median(ms), 4),
        "min_ms": round(min(ms), 4),
        "p10_ms": round(q[0], 4),
        "p90_ms": round(q[-1], 4),
        "n": len(ms),
    }


def fill_panes(st, cells_per_pane, chunk=1 << 20):
    g = torch.Generator(device=dev).manual_seed(7)
    for pane in range(N_PANES):
        t = ALIGN_MS + pane * PANE + 5
        for lo in range(0, cells_per_pane, chunk):
            n = min(chunk, cells_per_pane - lo)
            keys = torch.arange(lo, lo + n, dtype=torch.int32, device=dev)
            ts = torch.full((n,), t, dtype=torch.int64, device=dev)
            vals = torch.randint(
                -(1 << 40), 1 << 40, (n,), generator=g, device=dev
            )
            st.insert(RecordBatch(keys, ts, vals, max_ts=t))


def close_cost(load, reps, warmup):
    per_pane = int(NSLOTS * load) // N_PANES
    occupied = per_pane * N_PANES
    st = SlidingStatsAggState(
        dev, ALIGN_MS, LEN, OFF, slots_pow=SLOTS_POW, out_cap=1 << 21
    )
    assert st.nslots == NSLOTS and st.fold_slots == NSLOTS
    fill_panes(st, per_pane)
    assert int((st.tkeys != -1).sum().item()) == occupied
    assert int(st.error_flag.item()) == 0
    table = (st.tkeys, st.tcnt, st.tsum, st.tmin, st.tmax)
    alt, fold = (
        tuple(
            torch.full((NSLOTS,), f, dtype=torch.int64, device=dev)
            for f in FILLS
        )
        for _ in range(2)
    )
    outs = (
        st.out_keys, st.out_wins, st.out["cnt"], st.out["sum"],
        st.out["min"], st.out["max"], st.out_n,
    )
    n_w, n_o = st.panes_per_window, st.panes_per_offset
    folded = n_w * per_pane  # panes 0 .. 2 into window 0
    rows = per_pane  # one row per key
    live = (N_PANES - 1) * per_pane
    t_mig, t_pane, t_ext, t_rst = [], [], [], []
    for i in range(warmup + reps):
        # The tumbling close of pane 0 on the same table.
        st.out_n.zero_()
        a0, a1 = events()
        a0.record()
        k.stats_close_migrate(*table, *alt, 0, 1, *outs, st.error_flag)
        a1.record()
        n_mig = st.out_n.clone()
        for t, f in zip(alt, FILLS):
            t.fill_(f)
        # The sliding close of window 0.
        b0, b1 = events()
        b0.record()
        k.stats_pane_close(
            *table, *alt, *fold, 0, 1, n_o, n_w, n_o, st.error_flag
        )
        b1.record()
        st.out_n.zero_()
        c0, c1 = events()
        c0.record()
        k.stats_extract(*fold, 0, 1 << 40, *outs)
        c1.record()
        n_fold = st.out_n.clone()
        d0, d1 = events()
        d0.record()
        for t, f in zip(fold, FILLS):
            t.fill_(f)
        d1.record()
        for t, f in zip(alt, FILLS):
            t.fill_(f)
        torch.cuda.synchronize()
        assert int(n_mig.item()) == per_pane and int(n_fold.item()) == rows
        if i >= warmup:
            t_mig.append(a0.elapsed_time(a1))
            t_pane.append(b0.elapsed_time(b1))
            t_ext.append(c0.elapsed_time(c1))
            t_rst.append(d0.elapsed_time(d1))
    assert int(st.error_flag.item()) == 0
    # Bytes from the shapes.  A migrated cell is a probe read and a
    # 40 B cell written; a row is 40 B (two int32, four int64 columns).
    b_mig = 8 * NSLOTS + 32 * occupied + (8 + 40) * live + 40 * per_pane
    # Keys of every slot, values of every occupied slot (each is folded
    # or migrated), per fold a probe read and four 8 B atomics, and the
    # migrated cells.
    b_pane = 8 * NSLOTS + 32 * occupied + (8 + 32) * folded + (8 + 40) * live
    b_ext = 8 * NSLOTS + 32 * rows + 40 * rows
    b_rst = 40 * NSLOTS
    t_sum = [a + b + c for a, b, c in zip(t_pane, t_ext, t_rst)]

    def rate(nbytes, ms):
        return round(nbytes / (statistics.median(ms) * 1e-3) / 1e9, 1)

    def ratio(ms):
        return round(statistics.median(ms) / statistics.median(t_mig), 2)

    return {
        "load": load,
        "occupied": occupied,
        "cells_per_pane": per_pane,
        "folded_cells": folded,
        "fold_atomics": 4 * folded,
        "rows": rows,
        "migrated_cells": live,
        "close_migrate": summary(t_mig),
        "pane_close": summary(t_pane),
        "fold_extract": summary(t_ext),
        "fold_reset_fills": summary(t_rst),
        "sliding_total": summary(t_sum),
        "bytes": {"close_migrate": b_mig, "pane_close": b_pane,
                  "fold_extract": b_ext, "fold_reset_fills": b_rst},
        "GB_per_s": {
            "close_migrate": rate(b_mig, t_mig),
            "pane_close": rate(b_pane, t_pane),
            "fold_extract": rate(b_ext, t_ext),
            "fold_reset_fills": rate(b_rst, t_rst),
        },
        "time_ratio_over_close_migrate": {
            "pane_close": ratio(t_pane),
            "fold_extract": ratio(t_ext),
            "fold_reset_fills": ratio(t_rst),
            "sliding_total": ratio(t_sum),
        },
    }


def insert_parity(reps, n_keys=100_000, n_steps=30, per_batch=200_000):
    g = torch.Generator(device=dev).manual_seed(11)
    keys = torch.cat(
        [
            torch.arange(n_keys, dtype=torch.int32, device=dev),
            torch.randint(
                0, n_keys, (per_batch - n_keys,), dtype=torch.int32,
                generator=g, device=dev,
            ),
        ]
    )
    offs = torch.randint(0, PANE, (per_batch,), generator=g, device=dev)
    vals = torch.randint(
        -(1 << 40), 1 << 40, (per_batch,), generator=g, device=dev
    )
    batches = [
        RecordBatch(
            keys, ALIGN_MS + s * PANE + offs, vals,
            max_ts=ALIGN_MS + (s + 1) * PANE - 1,
        )
        for s in range(n_steps)
    ]
    kw = dict(slots_pow=SLOTS_POW, out_cap=1 << 22)

    def one_pass():
        sides = [
            StatsAggState(dev, ALIGN_MS, PANE, **kw),
            SlidingStatsAggState(dev, ALIGN_MS, LEN, OFF, **kw),
            StatsAggState(dev, ALIGN_MS, PANE, **kw),
        ]
        times = [[] for _ in sides]
        for b in batches:
            evs = []
            for st in sides:
                e0, e1 = events()
                e0.record()
                st.insert(b)
                e1.record()
                evs.append((e0, e1))
                st.close_due(0)  # keeps the table at its working set
            torch.cuda.synchronize()
            for t, (e0, e1) in zip(times, evs):
                t.append(e0.elapsed_time(e1))
        loads = [int((st.tkeys != -1).sum().item()) / NSLOTS for st in sides]
        return times, loads

    one_pass()  # warm-up: code objects, allocator
    runs = [one_pass() for _ in range(reps)]
    # Steady state: the sliding table holds its three live panes from
    # the fourth step on.
    skip = 4

    def med(side):
        return [
            round(statistics.median(r[0][side][skip:]), 4) for r in runs
        ]

    tum_a, sliding, tum_b = med(0), med(1), med(2)
    return {
        "n_keys": n_keys,
        "steps": n_steps,
        "events_per_batch": per_batch,
        "reps": reps,
        "final_load": {
            "tumbling": round(runs[-1][1][0], 3),
            "sliding": round(runs[-1][1][1], 3),
        },
        "insert_median_ms_per_rep": {
            "tumbling_a": tum_a, "sliding": sliding, "tumbling_b": tum_b,
        },
        "ratio_sliding_over_tumbling_a": [
            round(s / a, 3) for s, a in zip(sliding, tum_a)
        ],
        "ratio_tumbling_b_over_tumbling_a": [
            round(b / a, 3) for b, a in zip(tum_b, tum_a)
        ],
    }


def sustain(reps, per_batch=1_000_000, n_batches=2000, vocab=100_000):
    import bytewax_amd.operators as op
    from bytewax_amd.dataflow import Dataflow
    from bytewax_amd.gpu.operators import (
        SyntheticEventSource,
        keyed_stats_agg,
    )
    from bytewax_amd.outputs import DynamicSink, StatelessSinkPartition
    from bytewax_amd.testing import run_main

    class _Count(StatelessSinkPartition):
        def __init__(self, tally):
            self.tally = tally

        def write_batch(self, items):
            for d in items:
                self.tally[0] += len(d["keys"])

    class CountSink(DynamicSink):
        def __init__(self, tally):
            self.tally = tally

        def build(self, step_id, worker_index, worker_count):
            return _Count(self.tally)

    def run(offset):
        tally = [0]
        flow = Dataflow("stats_sliding_bench")
        s = op.input(
            "inp",
            flow,
            SyntheticEventSource(
                events_per_batch=per_batch,
                n_batches=n_batches,
                vocab=vocab,
                align_to=ALIGN,
                sim_ms_per_batch=1000,
                with_vals=True,
            ),
        )
        agg = keyed_stats_agg(
            "stats",
            s,
            align_to=ALIGN,
            length=timedelta(milliseconds=LEN if offset else PANE),
            offset=offset,
            slots_pow=SLOTS_POW,
            out_cap=1 << 22,
            exchange=False,
        )
        op.output("out", agg, CountSink(tally))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run_main(flow)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return per_batch * n_batches / dt, tally[0]

    off = timedelta(milliseconds=OFF)
    run(None), run(off)  # warm-up
    tum, sli, rows = [], [], None
    for _ in range(reps):
        r, _n = run(None)
        tum.append(r)
        r, rows = run(off)
        sli.append(r)
    return {
        "events_per_batch": per_batch,
        "batches": n_batches,
        "vocab": vocab,
        "reps": reps,
        "sliding_rows": rows,
        "events_per_s_tumbling_20s": [round(r) for r in tum],
        "events_per_s_sliding_60s_20s": [round(r) for r in sli],
        "ratio_sliding_over_tumbling": round(
            statistics.median(sli) / statistics.median(tum), 3
        ),
    }


if args.mode == "close":
    reps = args.reps or 60
    result = {
        "mode": "close",
        "nslots": NSLOTS,
        "cases": [close_cost(load, reps, args.warmup) for load in (0.1, 0.4)],
    }
elif args.mode == "insert":
    result = {"mode": "insert", **insert_parity(args.reps or 5)}
else:
    result = {"mode": "sustain", **sustain(args.reps or 3)}
line = json.dumps(result)
print(line)
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")
