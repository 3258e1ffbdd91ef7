"""The one multi-process launcher of the suite: run_ranks(target, world, *args) runs target(rank, world, *args) in `world` spawned
processes that form a process group, and returns what they returned, in rank order.

A rank that raises or dies ends the call at once, with its traceback or exit code in the message; nothing the call started outlives
it.  Rendezvous ports are picked per call (free_port), so neither a straggler nor anybody else's job on the machine can hold one."""
import os
import queue
import socket
import time
import traceback

import torch.multiprocessing as mp

POLL_S = 0.2            # one look at the result queue; the children's exit codes are checked between two looks
JOIN_S = 120.0          # ranks that have delivered their results leave the barrier and exit within this
GRACE_S = 1.0           # what is still alive when the call ends gets this long to exit by itself, then terminate(), then kill()
# what a launcher (torch.distributed.run) puts in a rank's environment: a test that starts one of its own removes these first
LAUNCHER_ENV = ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "GROUP_RANK", "ROLE_RANK",
                "TORCHELASTIC_RUN_ID")


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _child(rank, world, port, backend, target, args, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    grouped = False
    try:
        try:
            if world > 1:                     # (a one-rank run has no group, but still its own process: what it patches stays there)
                dist.init_process_group(backend, rank=rank, world_size=world)
                grouped = True
            result = target(rank, world, *args)
        except Exception:
            q.put((rank, "error", traceback.format_exc()))
            return
        q.put((rank, "ok", result))
        if grouped:
            dist.barrier()
    finally:
        if grouped:
            dist.destroy_process_group()


def _reap(procs):
    end = time.monotonic() + GRACE_S
    for p in procs:
        if p.pid is not None:
            p.join(max(0.0, end - time.monotonic()))
    for stop in ("terminate", "kill"):
        alive = [p for p in procs if p.pid is not None and p.exitcode is None]
        for p in alive:
            getattr(p, stop)()
        for p in alive:
            p.join(GRACE_S)


def run_ranks(target, world, *args, timeout=300.0, backend="gloo"):
    """`target` is a module-level function (spawn pickles it by name) that RETURNS its result."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_child, args=(r, world, port, backend, target, args, q)) for r in range(world)]
    results, errors = {}, {}
    end = time.monotonic() + timeout

    def failure():
        """every rank that failed, not the first one heard of: the rank that lost its peer often reports before the one that died"""
        gone = [f"rank {r} of {world} exited with code {p.exitcode} without a result"
                for r, p in enumerate(procs) if r not in results and r not in errors and p.exitcode is not None]
        return RuntimeError("\n".join(gone + [f"rank {r} of {world} raised:\n{errors[r]}" for r in sorted(errors)]))
    try:
        for p in procs:
            p.start()
        while len(results) + len(errors) < world:     # results first, join afterwards: a child cannot exit before its result has been read
            # looked at BEFORE the queue: a child that has exited has flushed what it put, so an empty queue after this is final
            gone = any(r not in results and r not in errors and p.exitcode is not None for r, p in enumerate(procs))
            try:
                rank, kind, payload = q.get(timeout=POLL_S)
            except queue.Empty:
                if errors or gone:
                    raise failure()
                if time.monotonic() > end:
                    raise TimeoutError(f"{world - len(results)} of {world} ranks gave no result within {timeout} s")
                continue
            (results if kind == "ok" else errors)[rank] = payload
        if errors:
            raise failure()
        for p in procs:
            p.join(JOIN_S)
        codes = [p.exitcode for p in procs]
        assert codes == [0] * world, codes
        return [results[r] for r in range(world)]
    finally:
        _reap(procs)
        q.close()
