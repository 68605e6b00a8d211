"""The one launcher of the multi-process tests: `world` spawned ranks, a process group among them, one result per rank.

A rank that raises or dies ends the wait at once, with its traceback or exit code in the AssertionError; no way out of
run_ranks() leaves a child running (a GPU rank would go on holding the device, blocked in a collective)."""
import datetime
import os
import queue
import socket
import sys
import time
import traceback

import torch
import torch.multiprocessing as mp

ANSWER_S = 150        # for every rank's result to arrive
JOIN_S = 120          # for every rank to leave after the last result
POLL_S = 0.2          # one look at the queue; between two looks, one at every child's exit code
KILL_GRACE_S = 10     # for the children killed on the way out to be gone


class _Failure:
    def __init__(self, text):
        self.text = text


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _child(worker, backend, rank, world, port, q, args):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    try:
        if backend is not None:
            import torch.distributed as dist
            group = dict(rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
            if backend == "nccl":
                torch.cuda.set_device(0)
                group["device_id"] = torch.device("cuda", 0)
            dist.init_process_group(backend, **group)
        result = worker(rank, world, *args)
    except BaseException:
        q.put((rank, _Failure(traceback.format_exc())))
        q.close()
        q.join_thread()          # (the traceback is in the pipe before this process leaves)
        sys.exit(1)
    q.put((rank, result))
    if backend is not None:
        dist.barrier()
        dist.destroy_process_group()


def _take(q, procs, results, timeout):
    """One answer from the queue into `results`, if one comes within `timeout`; a reported failure raises."""
    try:
        rank, result = q.get(timeout=timeout)
    except queue.Empty:
        return False
    if isinstance(result, _Failure):
        procs[rank].join(KILL_GRACE_S)
        raise AssertionError(f"rank {rank} failed (exit code {procs[rank].exitcode}):\n{result.text}")
    results[rank] = result
    return True


def run_ranks(worker, world, *args, backend="gloo", answer_s=ANSWER_S, join_s=JOIN_S):
    """worker(rank, world, *args), a module-level function, in `world` spawned processes joined in a `backend` process group
    (None: no group); returns the workers' results, indexed by rank."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_child, args=(worker, backend, r, world, port, q, args)) for r in range(world)]
    results = {}
    try:
        for p in procs:
            p.start()
        deadline = time.monotonic() + answer_s
        while len(results) < world:
            _take(q, procs, results, POLL_S)
            for r, p in enumerate(procs):
                if p.exitcode is not None and (p.exitcode != 0 or r not in results):
                    while _take(q, procs, results, POLL_S):          # (what it said last may still be on its way)
                        pass
                    if p.exitcode != 0 or r not in results:
                        raise AssertionError(f"rank {r} left with exit code {p.exitcode} " + ("after" if r in results else "without") + " its answer")
            if len(results) < world and time.monotonic() > deadline:
                silent = [r for r in range(world) if r not in results]
                raise AssertionError(f"no answer within {answer_s} s from rank(s) {silent}")
        for r, p in enumerate(procs):
            p.join(timeout=join_s)
            assert p.exitcode == 0, f"rank {r} left with exit code {p.exitcode} after its answer"
        return [results[r] for r in range(world)]
    finally:
        started = [p for p in procs if p.pid is not None]
        for p in started:
            if p.is_alive():
                p.kill()
        for p in started:
            p.join(KILL_GRACE_S)
