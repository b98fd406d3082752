"""The owner of every device block on the CPU: csrc/mrs_tg_block.hpp (Block, ensure, ensure_filled, ensure_both) compiled by g++
into tests/host/block_harness.cpp over a counting allocator that fails on request.  What it checks are the states behind a failed
allocation, a failed fill and a failed synchronise, which a GPU test must not provoke: a block is held or empty, a pair is held
or empty together, a fill that failed runs again, a failed idle step is reported, and nothing is live at the end.  No GPU."""
import pytest

from tests import host_harness as hh

CHECKS = [
    "ensure_allocates_once_and_grows_behind_idle",
    "caller_idle_step_and_headroom",
    "failed_allocation_leaves_the_block_empty",
    "pair_both_held_or_both_empty",
    "filled_once_fill_failure_empties_the_block",
    "failing_idle_is_returned_old_block_freed_nothing_allocated",
    "request_of_zero_is_a_request_of_one",
    "reset_gives_back_once",
]


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_block_states_over_a_failing_allocator(tmp_path, sanitize):
    exe = hh.build("block_harness.cpp", tmp_path, sanitize=sanitize)
    env = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1") if sanitize else None
    assert hh.run(exe, [], len(CHECKS), env=env) == ["ok " + c for c in CHECKS]
