"""CPU, gloo: the multi-process launcher of the suite itself (tests/ranks.py).  A failing rank must end the call within seconds, with
its traceback or exit code in the message, and leave no process behind -- not leave the parent waiting for the deadline while the
surviving rank sits in a collective.  The workers touch neither the package nor a device."""
import multiprocessing
import os
import time

import pytest

from tests.ranks import run_ranks


def _all_reduce(value):
    import torch
    import torch.distributed as dist
    t = torch.tensor([value], dtype=torch.int64)
    dist.all_reduce(t)
    return int(t[0])


def _sum_worker(rank, world):
    return _all_reduce(rank + 1)


def _raising_worker(rank, world):
    if rank == 1:
        raise ValueError("boom")
    return _all_reduce(1)                # rank 0 waits here for a rank that never comes


def _dying_worker(rank, world):
    if rank == 1:
        os._exit(3)
    return _all_reduce(1)


def _sleeping_worker(rank, world):
    time.sleep(60)


def test_results_come_back_in_rank_order():
    assert run_ranks(_sum_worker, 2) == [3, 3]
    assert multiprocessing.active_children() == []


def _fails_at_once(worker, *words):
    """120 s is the deadline a waiting parent would sit out; the poll interval and the grace period of the harness are constants
    of a few seconds, so is the spawn: a quarter of the deadline is ample."""
    t0 = time.monotonic()
    with pytest.raises(RuntimeError) as e:
        run_ranks(worker, 2, timeout=120)
    assert time.monotonic() - t0 < 120 / 4
    assert all(w in str(e.value) for w in words), str(e.value)
    assert multiprocessing.active_children() == []


def test_a_raising_rank_ends_the_call_at_once_with_its_traceback():
    _fails_at_once(_raising_worker, "boom", "ValueError")


def test_a_rank_that_dies_silently_ends_the_call_at_once_with_its_exit_code():
    _fails_at_once(_dying_worker, "rank 1", "code 3")


def test_a_deadline_raises_timeout_error_and_leaves_no_process():
    with pytest.raises(TimeoutError):
        run_ranks(_sleeping_worker, 2, timeout=5)
    assert multiprocessing.active_children() == []
