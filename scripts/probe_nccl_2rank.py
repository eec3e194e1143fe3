"""Probe: can RCCL run 2 ranks on one physical MI355X?

Functional validation of the exchange code path (bucketing kernel +
all_to_all_single over the real NCCL/RCCL backend) without an 8-GPU
node: both ranks map to cuda:0.  Prints per-rank checksums of the
exchanged batch so correctness can be compared against the
single-process expectation.
"""

import os
import sys
from pathlib import Path

import torch
import torch.multiprocessing as mp

REPO = str(Path(__file__).resolve().parent.parent)
# Spawned workers re-import this module; make the package importable
# in them regardless of how the parent was launched.
os.environ["PYTHONPATH"] = REPO + os.pathsep + os.environ.get("PYTHONPATH", "")
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def expected(world: int):
    """What every rank together should hold after the exchange."""
    from bytewax_amd.gpu import key_owner

    per = {}
    for rank in range(world):
        g = torch.Generator().manual_seed(1234 + rank)
        keys = torch.randint(0, 1000, (4096,), dtype=torch.int32, generator=g)
        ts = torch.arange(4096, dtype=torch.int64) + rank
        dst = key_owner(keys, world)
        for d in range(world):
            m = dst == d
            k, t = keys[m], ts[m]
            s = per.setdefault(d, [0, 0, 0])
            s[0] += int(k.numel())
            s[1] += int(k.to(torch.int64).sum())
            s[2] += int(t.sum())
    return per


def worker(rank: int, world: int):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = "29571"
    os.environ["RANK"] = str(rank)
    os.environ["WORLD_SIZE"] = str(world)
    torch.cuda.set_device(0)
    import torch.distributed as dist

    dist.init_process_group("nccl", rank=rank, world_size=world)
    from bytewax_amd.gpu import RecordBatch, exchange_by_key

    g = torch.Generator().manual_seed(1234 + rank)
    keys = torch.randint(0, 1000, (4096,), dtype=torch.int32, generator=g)
    ts = torch.arange(4096, dtype=torch.int64) + rank
    batch = RecordBatch(
        keys.to("cuda:0"), ts.to("cuda:0"), max_ts=int(ts.max())
    )
    out = exchange_by_key(batch)
    n = len(out)
    ksum = int(out.keys.to(torch.int64).sum().item())
    tsum = int(out.ts.sum().item())
    exp = expected(world)[rank]
    ok = [n, ksum, tsum] == exp
    print(
        f"RANK {rank}: n={n} ksum={ksum} tsum={tsum} "
        f"expected={exp} OK={ok}",
        flush=True,
    )
    dist.barrier()
    dist.destroy_process_group()
    if not ok:
        sys.exit(1)


def single_rank_nccl():
    """Fallback when RCCL refuses 2 ranks on one device ("Duplicate
    GPU detected"): run the full exchange path (bucketing kernels +
    all_to_all_single over a real 1-rank NCCL/RCCL group; self-copy)
    and verify the roundtrip is the identity on the key multiset."""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = "29573"
    torch.cuda.set_device(0)
    import torch.distributed as dist

    dist.init_process_group("nccl", rank=0, world_size=1)
    from bytewax_amd.gpu import RecordBatch, exchange_by_key

    g = torch.Generator().manual_seed(99)
    keys = torch.randint(0, 1000, (8192,), dtype=torch.int32, generator=g)
    ts = torch.arange(8192, dtype=torch.int64)
    batch = RecordBatch(
        keys.to("cuda:0"), ts.to("cuda:0"), max_ts=int(ts.max())
    )
    out = exchange_by_key(batch, force=True)
    ok = (
        len(out) == 8192
        and int(out.keys.to(torch.int64).sum()) == int(keys.to(torch.int64).sum())
        and int(out.ts.sum()) == int(ts.sum())
    )
    print(f"1-rank NCCL exchange roundtrip OK={ok}", flush=True)
    dist.destroy_process_group()
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    world = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    try:
        mp.spawn(worker, args=(world,), nprocs=world, join=True)
        print("PROBE_2RANK_RESULT: PASS", flush=True)
    except Exception as ex:  # noqa: BLE001
        if "Duplicate GPU" not in str(ex):
            raise
        # This RCCL build refuses N ranks on one device; validate the
        # collective wiring with a single NCCL-initialized rank.
        print(
            "2 ranks per device refused by RCCL (Duplicate GPU); "
            "falling back to the 1-rank NCCL exchange",
            flush=True,
        )
        single_rank_nccl()
        print("PROBE_2RANK_RESULT: PASS (1-rank fallback)", flush=True)
