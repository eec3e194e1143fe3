"""Windowed stream-stream join on MI355X.

Two synthetic keyed streams joined per (key, tumbling window) with
HBM-resident open-address state ("last" insert / "final" emit): each
window close emits its cells once and gives their slots back.

    python examples/window_join_gpu.py
    python examples/window_join_gpu.py --device cpu --rows 20000

With ``--track-late`` the same two streams go through the public
`win.join_window`, which lowers onto the same kernels with late
tracking and reports late events on `WindowOut.late` (none here: the
synthetic sides are ordered).  That lowering sizes its own table
(2^22 slots on a GPU), so the default there is 500,000 keys.

    python examples/window_join_gpu.py --track-late
"""

import argparse
import sys
import time
from datetime import datetime, timedelta, timezone
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import bytewax_amd.operators as op
import bytewax_amd.operators.windowing as win
from bytewax_amd.dataflow import Dataflow
from bytewax_amd.gpu import _ms
from bytewax_amd.gpu.operators import _SyntheticPartition, window_join
from bytewax_amd.inputs import DynamicSource
from bytewax_amd.outputs import DynamicSink, StatelessSinkPartition
from bytewax_amd.testing import run_main

ALIGN = datetime(2024, 1, 1, tzinfo=timezone.utc)
SIM_MS = 1000  # simulated time per batch
# A window spans two batches of each side.
LENGTH = timedelta(milliseconds=2 * SIM_MS)
# The sides are polled in turn, so one may run a batch or two ahead of
# the other: wait one window before closing.
WAIT = LENGTH


class _CountRows(DynamicSink):
    """Counts emitted rows and complete pairs without keeping them."""

    def __init__(self, totals):
        self.totals = totals

    def build(self, step_id, worker_index, worker_count):
        totals = self.totals

        class _Part(StatelessSinkPartition):
            def write_batch(self, items):
                for rows in items:
                    totals[0] += int(rows["keys"].numel())
                    totals[1] += int((rows["mask"] == 3).sum().item())

        return _Part()


class _CountLate(DynamicSink):
    """Counts the late events of `WindowOut.late`."""

    def __init__(self, totals):
        self.totals = totals

    def build(self, step_id, worker_index, worker_count):
        totals = self.totals

        class _Part(StatelessSinkPartition):
            def write_batch(self, items):
                for _key, (_wid, (_side, late)) in items:
                    totals[2] += len(late)

        return _Part()


def _prebuilt(part):
    class _Pre(DynamicSource):
        def build(self, step_id, worker_index, worker_count):
            return part

    return _Pre()


def _flow(device, per_batch, n_batches, keys, totals, track_late=False):
    import torch

    # Both sides are generated on the device before the run starts:
    # the join measures the hash-state kernels, not torch.randint.
    parts = [
        _SyntheticPartition(
            torch.device(device), per_batch, n_batches, keys, SIM_MS,
            _ms(ALIGN), seed, vals=True,
        )
        for seed in (1, 2)
    ]
    # About three windows are open at once (the one being filled plus
    # the wait); keep their (key, window) cells under half the table.
    slots_pow = max(10, (6 * min(keys, 4 * per_batch) - 1).bit_length())
    out_cap = 1 << max(10, (4 * keys - 1).bit_length())
    flow = Dataflow("window_join")
    left = op.input("left", flow, _prebuilt(parts[0]))
    right = op.input("right", flow, _prebuilt(parts[1]))
    if track_late:
        # The public operator: RecordBatch values under one shard key
        # lower onto the device join with late tracking.
        wo = win.join_window(
            "join",
            win.EventClock(
                ts_getter=lambda batch: batch, wait_for_system_duration=WAIT
            ),
            win.TumblingWindower(align_to=ALIGN, length=LENGTH),
            op.key_on("key_l", left, lambda _b: "shard-0"),
            op.key_on("key_r", right, lambda _b: "shard-0"),
        )
        rows = op.map("rows", wo.down, lambda k_wid_rows: k_wid_rows[1][1])
        op.output("out", rows, _CountRows(totals))
        op.output("late", wo.late, _CountLate(totals))
        return flow
    joined = window_join(
        "join", left, right, ALIGN, LENGTH, wait=WAIT,
        slots_pow=slots_pow, out_cap=out_cap, device=device,
    )
    op.output("out", joined, _CountRows(totals))
    return flow


def main():
    import torch

    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rows", type=int, default=160_000_000,
                    help="events per side")
    ap.add_argument("--rows-per-batch", type=int, default=16_000_000)
    ap.add_argument("--keys", type=int, default=None,
                    help="default 1,000,000 (500,000 with --track-late)")
    ap.add_argument("--device", default=None)
    ap.add_argument("--track-late", action="store_true",
                    help="run through win.join_window, which tracks late "
                    "events")
    args = ap.parse_args()
    if args.keys is None:
        args.keys = 500_000 if args.track_late else 1_000_000
    device = args.device or ("cuda" if torch.cuda.is_available() else "cpu")
    per_batch = max(1, min(args.rows_per_batch, args.rows))
    n_batches = max(1, args.rows // per_batch)
    on_gpu = device.startswith("cuda")

    def sync():
        if on_gpu:
            torch.cuda.synchronize()

    # Warm up outside the timed region: load the HIP extension and run
    # two batches per side through every kernel of the operator.
    run_main(
        _flow(
            device, min(per_batch, 4096), 2, args.keys, [0, 0, 0],
            args.track_late,
        ),
        epoch_interval=timedelta(days=365),
    )
    totals = [0, 0, 0]
    flow = _flow(
        device, per_batch, n_batches, args.keys, totals, args.track_late
    )
    sync()

    t0 = time.perf_counter()
    run_main(flow, epoch_interval=timedelta(days=365))
    sync()
    dt = time.perf_counter() - t0
    total = 2 * per_batch * n_batches
    print(
        f"window-joined {total} events -> {totals[0]} cells "
        f"({totals[1]} with both sides) in {dt:.3f}s = "
        f"{total / dt:.3e} events/s"
        + (f", {totals[2]} late events" if args.track_late else "")
    )


if __name__ == "__main__":
    main()
