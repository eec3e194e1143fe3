"""Cost of the reclaiming stats close, and what it buys the insert.

Two measurements, both with device events in one process, the two
sides alternating call by call:

    python scripts/bench_stats_close.py close   [--reps 60]
    python scripts/bench_stats_close.py sustain [--reps 3]

`close`: a 2^22-slot `StatsAggState` table with 10 % and 40 % of the
slots occupied, half of the cells in the due window.  Times the
non-reclaiming `stats_extract` of the due window, the
`stats_close_migrate` kernel, and the five fills that reset the
retired table, and prints the bytes each must move, computed from the
shapes, with the achieved bytes per second.

`sustain`: the geometry the `fold_window` lowering builds (2^22 slots,
late tracking on), 100k keys, 35 one-window batches of 200k events.
One state closes as the operators did before (`extract(horizon)` and a
`closed_horizon` bump, which keeps every cell), the other through
`close_below`.  Prints the insert time per window of both.

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
from bytewax_amd.gpu.state import StatsAggState  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("mode", choices=["close", "sustain"])
p.add_argument("--reps", type=int, default=None)
p.add_argument("--warmup", type=int, default=10)
p.add_argument("--out", default=None)
args = p.parse_args()

k = ext()
dev = torch.device("cuda:0")
ALIGN_MS, LEN = 1_704_067_200_000, 60_000
SLOTS_POW = 22
NSLOTS = 1 << SLOTS_POW
FILLS = (-1, 0, 0, (1 << 63) - 1, -(1 << 63))


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


def fill_table(st, cells_per_window, windows, chunk=1 << 20):
    g = torch.Generator(device=dev).manual_seed(7)
    for w in windows:
        for lo in range(0, cells_per_window, chunk):
            n = min(chunk, cells_per_window - lo)
            keys = torch.arange(lo, lo + n, dtype=torch.int32, device=dev)
            ts = torch.full(
                (n,), ALIGN_MS + w * LEN + 5, dtype=torch.int64, device=dev
            )
            vals = torch.randint(
                -(1 << 40), 1 << 40, (n,), generator=g, device=dev
            )
            st.insert(
                RecordBatch(keys, ts, vals, max_ts=ALIGN_MS + w * LEN + 5)
            )


def close_cost(load, reps, warmup):
    occupied = int(NSLOTS * load) // 2 * 2
    due = live = occupied // 2
    st = StatsAggState(dev, ALIGN_MS, LEN, slots_pow=SLOTS_POW, out_cap=1 << 21)
    assert st.nslots == NSLOTS
    fill_table(st, due, (0, 1))
    assert int((st.tkeys != -1).sum().item()) == occupied
    assert int(st.error_flag.item()) == 0
    table = (st.tkeys, st.tcnt, st.tsum, st.tmin, st.tmax)
    alt = tuple(
        torch.full((NSLOTS,), f, dtype=torch.int64, device=dev) for f in FILLS
    )
    outs = (
        st.out_keys, st.out_wins, st.out["cnt"], st.out["sum"],
        st.out["min"], st.out["max"], st.out_n,
    )
    t_ext, t_mig, t_rst = [], [], []
    for i in range(warmup + reps):
        st.out_n.zero_()
        a0, a1 = events()
        a0.record()
        k.stats_extract(*table, 0, 1, *outs)
        a1.record()
        n_ext = st.out_n.clone()
        st.out_n.zero_()
        b0, b1 = events()
        b0.record()
        k.stats_close_migrate(*table, *alt, 0, 1, *outs, st.error_flag)
        b1.record()
        n_mig = st.out_n.clone()
        c0, c1 = events()
        c0.record()
        for t, f in zip(alt, FILLS):
            t.fill_(f)
        c1.record()
        torch.cuda.synchronize()
        assert int(n_ext.item()) == due and int(n_mig.item()) == due
        if i >= warmup:
            t_ext.append(a0.elapsed_time(a1))
            t_mig.append(b0.elapsed_time(b1))
            t_rst.append(c0.elapsed_time(c1))
    assert int(st.error_flag.item()) == 0
    # Bytes from the shapes.  Rows written are 40 B each on both sides
    # (two int32 and four int64 columns).
    b_ext = 8 * NSLOTS + 32 * due + 40 * due
    # Keys of every slot, values of every occupied slot that is due or
    # live, a probe read and a 40 B cell written per migrated cell, and
    # the rows.
    b_mig = 8 * NSLOTS + 32 * occupied + (8 + 40) * live + 40 * due
    b_rst = 40 * NSLOTS
    t_close = [m + r for m, r in zip(t_mig, t_rst)]

    def rate(nbytes, ms):
        return round(nbytes / (statistics.median(ms) * 1e-3) / 1e9, 1)

    return {
        "load": load,
        "occupied": occupied,
        "due": due,
        "extract": summary(t_ext),
        "migrate_kernel": summary(t_mig),
        "reset_fills": summary(t_rst),
        "close_total": summary(t_close),
        "bytes": {"extract": b_ext, "migrate_kernel": b_mig,
                  "reset_fills": b_rst, "close_total": b_mig + b_rst},
        "GB_per_s": {
            "extract": rate(b_ext, t_ext),
            "migrate_kernel": rate(b_mig, t_mig),
            "reset_fills": rate(b_rst, t_rst),
            "close_total": rate(b_mig + b_rst, t_close),
        },
        "time_ratio_close_over_extract": round(
            statistics.median(t_close) / statistics.median(t_ext), 2
        ),
        "byte_ratio_close_over_extract": round((b_mig + b_rst) / b_ext, 2),
    }


def sustain(reps, n_keys=100_000, n_win=35, per_batch=200_000):
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
    offs = torch.randint(0, LEN, (per_batch,), generator=g, device=dev)
    vals = torch.randint(
        -(1 << 40), 1 << 40, (per_batch,), generator=g, device=dev
    )
    batches = [
        RecordBatch(
            keys, ALIGN_MS + w * LEN + offs, vals,
            max_ts=ALIGN_MS + (w + 1) * LEN - 1,
        )
        for w in range(n_win)
    ]

    def mk():
        return StatsAggState(
            dev, ALIGN_MS, LEN, slots_pow=SLOTS_POW, out_cap=1 << 22,
            track_late=True, wait_ms=0,
        )

    def one_pass():
        old, new = mk(), mk()
        t_old, t_new, rows_old, rows_new = [], [], 0, 0
        for w, b in enumerate(batches):
            a0, a1 = events()
            a0.record()
            old.insert(b)
            a1.record()
            out = old.extract(w)
            old.closed_horizon = w
            rows_old += 0 if out is None else len(out["keys"])
            b0, b1 = events()
            b0.record()
            new.insert(b)
            b1.record()
            out = new.close_below(w)
            rows_new += 0 if out is None else len(out["keys"])
            torch.cuda.synchronize()
            t_old.append(a0.elapsed_time(a1))
            t_new.append(b0.elapsed_time(b1))
        assert rows_old == rows_new == n_keys * (n_win - 1)
        load_old = int((old.tkeys != -1).sum().item()) / NSLOTS
        load_new = int((new.tkeys != -1).sum().item()) / NSLOTS
        return t_old, t_new, load_old, load_new

    one_pass()  # warm-up: code objects, allocator
    runs = [one_pass() for _ in range(reps)]

    def per_window(side):
        return [
            round(statistics.median(r[side][w] for r in runs), 4)
            for w in range(n_win)
        ]

    old_ms, new_ms = per_window(0), per_window(1)
    return {
        "n_keys": n_keys,
        "windows": n_win,
        "events_per_batch": per_batch,
        "reps": reps,
        "final_load_extract_only": round(runs[-1][2], 3),
        "final_load_reclaiming": round(runs[-1][3], 3),
        "insert_ms_extract_only": old_ms,
        "insert_ms_reclaiming": new_ms,
        "first3_vs_last3_extract_only": [
            round(statistics.mean(old_ms[1:4]), 4),
            round(statistics.mean(old_ms[-3:]), 4),
        ],
        "first3_vs_last3_reclaiming": [
            round(statistics.mean(new_ms[1:4]), 4),
            round(statistics.mean(new_ms[-3:]), 4),
        ],
        "spread_last_window_ms": {
            "extract_only": [round(r[0][-1], 4) for r in runs],
            "reclaiming": [round(r[1][-1], 4) for r in runs],
        },
    }


if args.mode == "close":
    reps = args.reps or 60
    result = {
        "mode": "close",
        "nslots": NSLOTS,
        "cases": [close_cost(load, reps, args.warmup) for load in (0.1, 0.4)],
    }
else:
    result = {"mode": "sustain", **sustain(args.reps or 3)}
line = json.dumps(result)
print(line)
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")
