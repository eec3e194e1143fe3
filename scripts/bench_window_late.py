"""Cost of late tracking on the tumbling radix insert.

Times `WindowAggState.insert` + `close_due` over identical in-order
batches that carry `max_ts` hints (bench.py's workload scaled down:
1M keys, 60 s windows, 5 s of simulated time per batch, COUNT, int32
timestamp deltas), in one of three configurations:

    python scripts/bench_window_late.py                  # ordered-only
    python scripts/bench_window_late.py --track-late
    python scripts/bench_window_late.py --track-late --late-pct 1

Without `--track-late` the script uses nothing newer than the plain
`WindowAggState` constructor, so the same file measures the commit
before late tracking (the yardstick).  With `--late-pct P`, P % of
each batch (every 100/P-th event) is moved 10 minutes back, far below
the cutoff; late rows are drained at every close.
"""

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from bytewax_amd.gpu import AGG_COUNT, RecordBatch, WindowAggState  # noqa: E402
from bytewax_amd.gpu._ext import ext  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--track-late", action="store_true")
p.add_argument("--late-pct", type=float, default=0.0)
p.add_argument("--repeats", type=int, default=7)
p.add_argument("--batches", type=int, default=48)
p.add_argument("--events-per-batch", type=int, default=16_000_000)
args = p.parse_args()
if args.late_pct and not args.track_late:
    p.error("--late-pct needs --track-late")

ext()
dev = torch.device("cuda:0")
N, VOCAB, LEN, SIM, PER_CLOSE = args.events_per_batch, 1_000_000, 60_000, 5_000, 4
ALIGN_MS = 1_704_067_200_000
g = torch.Generator(device=dev).manual_seed(1)
pool = [
    torch.randint(0, VOCAB, (N,), dtype=torch.int32, generator=g, device=dev)
    for _ in range(4)
]
tmpl = ((torch.arange(N, dtype=torch.int64, device=dev) * SIM) // N).to(
    torch.int32
)
n_late = 0
if args.late_pct:
    every = int(round(100 / args.late_pct))
    tmpl[::every] -= 600_000
    n_late = len(range(0, N, every))


def batch(i):
    # Far enough from the alignment that the moved-back events stay
    # above it.
    start = ALIGN_MS + (i + 200) * SIM
    return RecordBatch(
        pool[i % 4], tmpl, None, max_ts=start + SIM - 1, ts_base=start
    )


def run(n_batches):
    extra = {"track_late": True, "wait_ms": 0} if args.track_late else {}
    st = WindowAggState(
        dev, ALIGN_MS, LEN, AGG_COUNT, slots_pow=22, out_cap=1 << 21,
        radix=True, region_bits=11, max_batch=N, **extra,
    )
    batches = [batch(i) for i in range(n_batches)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    events = late = 0
    for i, b in enumerate(batches):
        st.insert(b)
        if (i + 1) % PER_CLOSE == 0:
            out = st.close_due(0)
            if out is not None:
                events += int(out.vals.sum())
            if args.track_late:
                rows = st.take_late()
                late += len(rows) if rows is not None else 0
    out = st.close_all()
    if out is not None:
        events += int(out.vals.sum())
    if args.track_late:
        rows = st.take_late()
        late += len(rows) if rows is not None else 0
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    # The first batch has no earlier watermark: nothing in it is late.
    want_late = n_late * (n_batches - 1)
    assert late == want_late, (late, want_late)
    assert events + late == N * n_batches, (events, late)
    return dt


run(8)  # warm-up
rates = [N * args.batches / run(args.batches) for _ in range(args.repeats)]
print(
    json.dumps(
        {
            "track_late": args.track_late,
            "late_pct": args.late_pct,
            "events_per_s_median": statistics.median(rates),
            "events_per_s_min": min(rates),
            "events_per_s_max": max(rates),
            "repeats": args.repeats,
            "config": dict(
                events_per_batch=N, keys=VOCAB, window_ms=LEN,
                sim_ms_per_batch=SIM, batches=args.batches,
                batches_per_close=PER_CLOSE,
            ),
        }
    )
)
