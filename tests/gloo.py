"""One process per rank over gloo (test infrastructure): the environment, the import path and the
process group around a test's own worker body."""
import json
import os
import socket
import sys
from pathlib import Path

import torch.multiprocessing as mp


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank(rank, world, port, out_path, worker_body, args):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    root = Path(__file__).resolve().parent.parent
    sys.path[:0] = [str(root / "raft-simulation_amd"), str(root / "tests"), str(root / "oracle")]
    import torch.distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world)
    result = worker_body(rank, world, *args)
    if rank == 0:
        Path(out_path).write_text(json.dumps(result))
    dist.destroy_process_group()


def spawn(worker_body, world, out_path, *args):
    """Run worker_body(rank, world, *args) on `world` ranks inside one gloo process group; rank
    0's result is written to out_path as JSON, and returned. worker_body is pickled: a
    module-level function."""
    mp.spawn(_rank, args=(world, free_port(), str(out_path), worker_body, args), nprocs=world,
             join=True)
    return json.loads(Path(out_path).read_text())
