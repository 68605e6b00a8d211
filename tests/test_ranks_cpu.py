"""tests/ranks.py itself: results in rank order; a rank that raises, dies or never answers fails the test at once, with what it
left behind in the message, and no child outlives run_ranks().  Host processes only: they sleep, raise or exit."""
import atexit
import multiprocessing
import os
import time

import pytest
import torch

from tests import ranks
from tests.ranks import run_ranks


def _sum_worker(rank, world):
    import torch.distributed as dist
    t = torch.full((4,), float(rank + 1))
    dist.all_reduce(t)
    return rank, t.tolist()


def test_both_ranks_answer_in_rank_order():
    assert run_ranks(_sum_worker, 2, answer_s=120, join_s=60) == [(0, [3.0] * 4), (1, [3.0] * 4)]


def _raise_or_sleep(rank, world):
    if rank == 1:
        raise ValueError("boom")
    time.sleep(600)          # (a rank stuck in a collective)


def _die_or_sleep(rank, world):
    if rank == 1:
        os._exit(3)
    time.sleep(600)


@pytest.mark.parametrize("worker,words", [(_raise_or_sleep, ("ValueError", "boom")), (_die_or_sleep, ("exit code 3",))], ids=["raises", "dies"])
def test_a_rank_that_fails_ends_the_wait_and_its_peer(worker, words):
    t0 = time.monotonic()
    with pytest.raises(AssertionError) as e:
        run_ranks(worker, 2, backend=None, answer_s=60)
    assert time.monotonic() - t0 < 60
    assert all(w in str(e.value) for w in ("rank 1",) + words), str(e.value)
    assert multiprocessing.active_children() == []


def _sleep(rank, world):
    time.sleep(600)


def test_ranks_that_never_answer_are_named_and_killed():
    t0 = time.monotonic()
    with pytest.raises(AssertionError, match=r"rank\(s\) \[0, 1\]"):
        run_ranks(_sleep, 2, backend=None, answer_s=3)
    assert time.monotonic() - t0 < 3 + ranks.KILL_GRACE_S
    assert multiprocessing.active_children() == []


def _answer_then_exit_badly(rank, world):
    atexit.register(os._exit, 1)
    return rank


def test_a_clean_answer_with_a_bad_exit_fails():
    with pytest.raises(AssertionError, match="rank 0 left with exit code 1 after its answer"):
        run_ranks(_answer_then_exit_badly, 1, backend=None, answer_s=60)
    assert multiprocessing.active_children() == []
