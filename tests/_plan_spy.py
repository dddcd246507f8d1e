"""The one plan spy of the scheduler tests: the plans the allocate action
hands to the torch runner.  A plain module: no fixtures, no collection
hooks."""

import contextlib

import volcano_amd.scheduler.actions.allocate as alloc


@contextlib.contextmanager
def spying():
    """Collect every plan allocate runs while the block is open.  The
    action looks ``run_plan_torch`` up in its module at call time; whatever
    was installed there keeps running underneath."""
    seen = []
    real = alloc.run_plan_torch

    def spy(plan):
        seen.append(plan)
        return real(plan)

    alloc.run_plan_torch = spy
    try:
        yield seen
    finally:
        alloc.run_plan_torch = real


def plans_of(sched):
    """Run one cycle, returning the plans the torch runner was given."""
    with spying() as seen:
        sched.run_once()
    return seen
