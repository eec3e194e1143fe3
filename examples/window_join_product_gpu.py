"""Windowed product join of two streams on MI355X.

Two synthetic keyed streams joined per (key, tumbling window) with
"product" insert and "final" emit: each window close emits, for every
key, every left event of the window paired with every right one, and
gives the space back.

    python examples/window_join_product_gpu.py
    python examples/window_join_product_gpu.py --device cpu --rows 20000 \
        --rows-per-batch 2000 --keys 2000

By default every batch has as many events as there are keys, so a cell
holds about two events per side and the pairs are a small multiple of
the cells.  ``--hot-keys H --hot-frac F`` sends the fraction F of each
side's events to H keys: a few hot cells whose pairs grow with the
square of their events.

    python examples/window_join_product_gpu.py --hot-keys 4 --hot-frac 0.001
"""

import argparse
import math
import sys
import time
from datetime import datetime, timedelta, timezone
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import bytewax_amd.operators as op
from bytewax_amd.dataflow import Dataflow
from bytewax_amd.gpu import _ms
from bytewax_amd.gpu.operators import _SyntheticPartition, window_join_product
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


def _prebuilt(part):
    class _Pre(DynamicSource):
        def build(self, step_id, worker_index, worker_count):
            return part

    return _Pre()


def _skew(part, hot_keys, hot_frac, seed):
    """Send the fraction `hot_frac` of the pooled events to the keys
    below `hot_keys`."""
    import torch

    g = torch.Generator(device=part.device).manual_seed(seed)
    for i, keys in enumerate(part.key_pool):
        hot = (
            torch.rand(keys.shape, generator=g, device=part.device) < hot_frac
        )
        part.key_pool[i] = torch.where(hot, keys % hot_keys, keys)


def _rows_per_close(per_batch, keys, hot_keys, hot_frac):
    """Expected rows of one window: cells with Poisson-many events per
    side, plus the hot cells' squares."""
    per_window = 2 * per_batch
    lam = per_window * (1 - hot_frac) / keys
    rows = keys * (lam + math.exp(-lam)) ** 2
    if hot_keys:
        rows += hot_keys * (per_window * hot_frac / hot_keys + lam) ** 2
    return rows


def _flow(device, per_batch, n_batches, keys, totals, hot_keys, hot_frac):
    import torch

    # Both sides are generated on the device before the run starts:
    # the join measures its own kernels, not torch.randint.
    parts = [
        _SyntheticPartition(
            torch.device(device), per_batch, n_batches, keys, SIM_MS,
            _ms(ALIGN), seed, vals=True,
        )
        for seed in (1, 2)
    ]
    if hot_keys:
        for seed, part in enumerate(parts):
            _skew(part, hot_keys, hot_frac, 10 + seed)
    # About three windows are open at once (the one being filled plus
    # the wait); keep their (key, window) cells under half the table.
    slots_pow = max(10, (6 * min(keys, 4 * per_batch) - 1).bit_length())
    # Twice the expected rows of a window; a close with more raises.
    expect = _rows_per_close(per_batch, keys, hot_keys, hot_frac)
    out_cap = 1 << max(10, (int(2 * expect) - 1).bit_length())
    flow = Dataflow("window_join_product")
    left = op.input("left", flow, _prebuilt(parts[0]))
    right = op.input("right", flow, _prebuilt(parts[1]))
    joined = window_join_product(
        "join", left, right, ALIGN, LENGTH, wait=WAIT,
        slots_pow=slots_pow, out_cap=out_cap, log_cap=8 * per_batch,
        device=device,
    )
    op.output("out", joined, _CountRows(totals))
    return flow


def main():
    import torch

    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rows", type=int, default=200_000_000,
                    help="events per side")
    ap.add_argument("--rows-per-batch", type=int, default=1_000_000)
    ap.add_argument("--keys", type=int, default=1_000_000)
    ap.add_argument("--hot-keys", type=int, default=0,
                    help="keys that take --hot-frac of the events")
    ap.add_argument("--hot-frac", type=float, default=0.001)
    ap.add_argument("--device", default=None)
    args = ap.parse_args()
    device = args.device or ("cuda" if torch.cuda.is_available() else "cpu")
    per_batch = max(1, min(args.rows_per_batch, args.rows))
    n_batches = max(1, args.rows // per_batch)
    hot = (args.hot_keys, args.hot_frac if args.hot_keys else 0.0)
    on_gpu = device.startswith("cuda")

    def sync():
        if on_gpu:
            torch.cuda.synchronize()

    # Warm up outside the timed region: load the HIP extension and run
    # four batches per side through every kernel of the operator.
    run_main(
        _flow(device, min(per_batch, 4096), 4, args.keys, [0, 0], 0, 0.0),
        epoch_interval=timedelta(days=365),
    )
    totals = [0, 0]
    flow = _flow(device, per_batch, n_batches, args.keys, totals, *hot)
    sync()

    t0 = time.perf_counter()
    run_main(flow, epoch_interval=timedelta(days=365))
    sync()
    dt = time.perf_counter() - t0
    total = 2 * per_batch * n_batches
    print(
        f"product-joined {total} events -> {totals[0]} rows "
        f"({totals[1]} pairs with both sides) in {dt:.3f}s = "
        f"{total / dt:.3e} events/s, {totals[0] / dt:.3e} pairs/s"
    )


if __name__ == "__main__":
    main()
