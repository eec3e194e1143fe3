"""Cost of the sliding windowed join built from panes.

Two measurements, each in one process, the sides alternating call by
call:

    python scripts/bench_window_join_sliding.py close  [--reps 40]
    python scripts/bench_window_join_sliding.py insert [--reps 3]

`close`: the pane table of a 60 s / 10 s `SlidingWindowJoinState`
(panes of 10 s, six per window) with `--keys` keys (1M), both sides
present in each of the panes 0 .. 6: the table as it stands when window
0 falls due.  Closes window 0: panes 0 .. 5 fold into it, pane 0 dies
and panes 1 .. 6 migrate.  Times the stamp pass, the commit pass, the
`wjoin_extract` over the fold table, the five fills that reset the fold
table and the five that reset the retired pane table, each between its
own pair of device events, against the tumbling `wjoin_close_migrate`
of pane 0 on the same table (which emits as many rows and migrates the
same cells), once with the fold table at its default size (the pane
table's) and once at 2 x keys slots.

`insert`: insert time per batch of the sliding state against a
tumbling `WindowJoinState` of the pane width on the same batches (both
sides, `--batch` events each, int32 timestamp deltas), with a second
tumbling state as the measure of the run's own spread and a third that
closes 50 s late, so that its table holds the six panes the sliding
one holds (the same kernels at the same load).

Each mode prints one JSON line; `--out FILE` also writes it there.
"""

import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from bytewax_amd.gpu import RecordBatch  # noqa: E402
from bytewax_amd.gpu._ext import ext  # noqa: E402
from bytewax_amd.gpu.state import (  # noqa: E402
    SlidingWindowJoinState,
    WindowJoinState,
)

p = argparse.ArgumentParser()
p.add_argument("mode", choices=["close", "insert"])
p.add_argument("--reps", type=int, default=None)
p.add_argument("--warmup", type=int, default=5)
p.add_argument("--keys", type=int, default=1_000_000)
p.add_argument("--batch", type=int, default=16_000_000)
p.add_argument("--slots-pow", type=int, default=24)
p.add_argument("--insert-mode", default="last", choices=["first", "last"])
p.add_argument("--out", default=None)
args = p.parse_args()

k = ext()
dev = torch.device("cuda:0")
ALIGN_MS, LEN, OFF, PANE = 1_704_067_200_000, 60_000, 10_000, 10_000
N_PANES = 7
FIRST = args.insert_mode == "first"


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


def timed(fn):
    e0, e1 = events()
    e0.record()
    fn()
    e1.record()
    return e0, e1


def fill_panes(st, n_keys, chunk=1 << 20):
    g = torch.Generator(device=dev).manual_seed(7)
    for pane in range(N_PANES):
        for side in (0, 1):
            t = ALIGN_MS + pane * PANE + 5 + side
            for lo in range(0, n_keys, chunk):
                n = min(chunk, n_keys - lo)
                keys = torch.arange(lo, lo + n, dtype=torch.int32, device=dev)
                ts = torch.full((n,), t, dtype=torch.int64, device=dev)
                vals = torch.randint(
                    -(1 << 40), 1 << 40, (n,), generator=g, device=dev
                )
                st.insert(side, RecordBatch(keys, ts, vals, max_ts=t))


def close_cost(fold_slots_pow, reps, warmup):
    n_keys = args.keys
    st = SlidingWindowJoinState(
        dev, ALIGN_MS, LEN, OFF, args.insert_mode, slots_pow=args.slots_pow,
        out_cap=1 << 21, fold_slots_pow=fold_slots_pow,
    )
    nslots, fslots = st.nslots, st.fold_slots
    fill_panes(st, n_keys)
    occupied = N_PANES * n_keys
    assert int((st.tkeys != -1).sum().item()) == occupied
    assert int(st.error_flag.item()) == 0
    fills = st._fills[:5]
    table = (st.tkeys, st.tts0, st.tts1, st.tv0, st.tv1)
    alt = tuple(
        torch.full((nslots,), f, dtype=torch.int64, device=dev) for f in fills
    )
    fold = tuple(
        torch.full((fslots,), f, dtype=torch.int64, device=dev) for f in fills
    )
    o = st.out
    cm_outs = (o["keys"], o["wins"], o["v0"], o["v1"], o["mask"], st.out_n)
    ex_outs = (
        o["keys"], o["wins"], o["v0"], o["v1"], o["t0"], o["t1"], o["mask"],
        st.out_n,
    )
    n_w, n_o = st.panes_per_window, st.panes_per_offset
    names = ("close_migrate", "pane_stamp", "pane_commit", "fold_extract",
             "fold_reset_fills", "table_reset_fills")
    times = {name: [] for name in names}

    def refill(tables):
        for t, f in zip(tables, fills):
            t.fill_(f)

    for i in range(warmup + reps):
        ev = {}
        # The tumbling close of pane 0 on the same table.
        st.out_n.zero_()
        ev["close_migrate"] = timed(
            lambda: k.wjoin_close_migrate(
                *table, *alt, 0, 1, st.ts_none, *cm_outs, st.error_flag
            )
        )
        n_mig = st.out_n.clone()
        ev["table_reset_fills"] = timed(lambda: refill(alt))
        # The sliding close of window 0.
        ev["pane_stamp"] = timed(
            lambda: k.wjoin_pane_stamp(
                *table, *alt, *fold, 0, 1, n_o, n_w, n_o, FIRST,
                st.error_flag, 0,
            )
        )
        ev["pane_commit"] = timed(
            lambda: k.wjoin_pane_commit(
                *table, *fold, 0, 1, n_w, n_o, FIRST, st.error_flag, 0
            )
        )
        st.out_n.zero_()
        ev["fold_extract"] = timed(
            lambda: k.wjoin_extract(*fold, 0, 1 << 40, st.ts_none, *ex_outs)
        )
        n_fold = st.out_n.clone()
        ev["fold_reset_fills"] = timed(lambda: refill(fold))
        migrated = int((alt[0] != -1).sum().item())
        refill(alt)
        torch.cuda.synchronize()
        assert int(n_mig.item()) == n_keys and int(n_fold.item()) == n_keys
        assert migrated == occupied - n_keys
        if i >= warmup:
            for name, (e0, e1) in ev.items():
                times[name].append(e0.elapsed_time(e1))
    assert int(st.error_flag.item()) == 0
    folded = n_w * n_keys  # panes 0 .. 5 into window 0
    live = occupied - n_keys
    # Bytes from the shapes.  A cell is 40 B (key, two stamps, two
    # values); a migrated cell is a probe read and a cell written; a
    # close_migrate row is 28 B, an extract row 44 B.
    nbytes = {
        "close_migrate": 8 * nslots + 32 * live + 16 * n_keys
        + (8 + 40) * live + 28 * n_keys + 16 * n_keys,
        # Keys of every slot, stamps of every occupied slot, per fold a
        # probe read and two 8 B atomics, values of the migrated cells
        # and the cells written.
        "pane_stamp": 8 * nslots + 16 * occupied + (8 + 16) * folded
        + 16 * live + (8 + 40) * live,
        # Keys of every slot, stamps and values of the folded cells,
        # per fold a probe read and two stamps read; one winner per
        # row and side stores 8 B.
        "pane_commit": 8 * nslots + 32 * folded + (8 + 16) * folded
        + 16 * n_keys,
        "fold_extract": 8 * fslots + 32 * n_keys + 44 * n_keys,
        "fold_reset_fills": 40 * fslots,
        "table_reset_fills": 40 * nslots,
    }
    total = [
        sum(v)
        for v in zip(
            *(times[n] for n in names if n != "close_migrate")
        )
    ]
    tumbling = [
        a + b
        for a, b in zip(times["close_migrate"], times["table_reset_fills"])
    ]
    med = statistics.median
    return {
        "nslots": nslots,
        "fold_slots": fslots,
        "keys": n_keys,
        "occupied": occupied,
        "load": round(occupied / nslots, 3),
        "folded_cells": folded,
        "fold_stamp_atomics": 2 * folded,
        "rows": n_keys,
        "migrated_cells": live,
        **{name: summary(times[name]) for name in names},
        "sliding_total": summary(total),
        "tumbling_total": summary(tumbling),
        "bytes": nbytes,
        "GB_per_s": {
            name: round(nbytes[name] / (med(times[name]) * 1e-3) / 1e9, 1)
            for name in names
        },
        "time_ratio_over_close_migrate": {
            name: round(med(times[name]) / med(times["close_migrate"]), 2)
            for name in names
        },
        "sliding_total_over_tumbling_total": round(med(total) / med(tumbling), 2),
    }


def insert_parity(reps, n_steps=12):
    n_keys, per_batch = args.keys, args.batch
    g = torch.Generator(device=dev).manual_seed(11)
    sides = []
    for _side in (0, 1):
        keys = torch.randint(
            0, n_keys, (per_batch,), dtype=torch.int32, generator=g, device=dev
        )
        offs = torch.randint(
            0, PANE, (per_batch,), dtype=torch.int32, generator=g, device=dev
        )
        vals = torch.randint(
            -(1 << 40), 1 << 40, (per_batch,), generator=g, device=dev
        )
        sides.append((keys, offs, vals))
    batches = [
        [
            RecordBatch(
                keys, offs, vals, max_ts=ALIGN_MS + (s + 1) * PANE - 1,
                ts_base=ALIGN_MS + s * PANE,
            )
            for keys, offs, vals in sides
        ]
        for s in range(n_steps)
    ]
    kw = dict(slots_pow=args.slots_pow, out_cap=1 << 21)
    mode = args.insert_mode

    def one_pass():
        states = [
            WindowJoinState(dev, ALIGN_MS, PANE, mode, **kw),
            SlidingWindowJoinState(
                dev, ALIGN_MS, LEN, OFF, mode, fold_slots_pow=21, **kw
            ),
            WindowJoinState(dev, ALIGN_MS, PANE, mode, **kw),
            WindowJoinState(dev, ALIGN_MS, PANE, mode, **kw),
        ]
        waits = [0, 0, 0, LEN - PANE]
        times = [[] for _ in states]
        for pair in batches:
            evs = []
            for st, wait in zip(states, waits):
                e0, e1 = events()
                e0.record()
                for side, b in enumerate(pair):
                    st.insert(side, b)
                e1.record()
                evs.append((e0, e1))
                st.close_due(wait)  # keeps the table at its working set
            torch.cuda.synchronize()
            for t, (e0, e1) in zip(times, evs):
                t.append(e0.elapsed_time(e1))
        loads = [
            round(int((st.tkeys != -1).sum().item()) / st.nslots, 3)
            for st in states
        ]
        for st in states:
            assert int(st.error_flag.item()) == 0
        return times, loads

    one_pass()  # warm-up: code objects, allocator
    runs = [one_pass() for _ in range(reps)]
    # Steady state: the sliding table holds its six live panes from the
    # seventh step on.
    skip = 7

    def med(side):
        return [round(statistics.median(r[0][side][skip:]), 4) for r in runs]

    tum_a, sliding, tum_b, tum_late = med(0), med(1), med(2), med(3)
    return {
        "n_keys": n_keys,
        "steps": n_steps,
        "events_per_batch_and_side": per_batch,
        "nslots": 1 << args.slots_pow,
        "reps": reps,
        "final_load": dict(
            zip(
                ("tumbling_a", "sliding", "tumbling_b", "tumbling_six_panes"),
                runs[-1][1],
            )
        ),
        "insert_both_sides_median_ms_per_rep": {
            "tumbling_a": tum_a, "sliding": sliding, "tumbling_b": tum_b,
            "tumbling_six_panes": tum_late,
        },
        "ratio_sliding_over_tumbling_a": [
            round(s / a, 3) for s, a in zip(sliding, tum_a)
        ],
        "ratio_sliding_over_tumbling_six_panes": [
            round(s / a, 3) for s, a in zip(sliding, tum_late)
        ],
        "ratio_tumbling_b_over_tumbling_a": [
            round(b / a, 3) for b, a in zip(tum_b, tum_a)
        ],
    }


if args.mode == "close":
    reps = args.reps or 40
    result = {
        "mode": "close",
        "insert_mode": args.insert_mode,
        "cases": [
            close_cost(fp, reps, args.warmup)
            for fp in (None, (2 * args.keys - 1).bit_length())
        ],
    }
else:
    result = {
        "mode": "insert",
        "insert_mode": args.insert_mode,
        **insert_parity(args.reps or 3),
    }
line = json.dumps(result)
print(line)
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")
