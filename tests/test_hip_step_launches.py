"""GPU: every way to run a step issues the launches it issued before the host layer was folded into one chain, one recorder
and one run loop -- by name, in order, from construction to the end of the run.  The expectation
(tests/golden/step_launches.json) was written by tools/step_launch_trace.py on the commit BEFORE that change, through the
``_lib.TIMER`` hook that ``_lib.call`` consults for every launch; it is never regenerated from the code under test."""
import json
import os

import pytest

from tools import step_launch_trace as T

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_launches.json")) as _fh:
    GOLDEN = json.load(_fh)


@pytest.fixture(scope="module")
def arithmetic():
    """The arithmetic the stored traces were taken in, and one untraced step (what the process builds once)."""
    from gotennet_amd import engine
    old = engine.GEMM_MODE
    yield T.prepare(GOLDEN["arithmetic"])
    engine.GEMM_MODE = old


def test_every_mode_has_a_stored_trace():
    assert set(GOLDEN["launches"]) == set(T.MODES)


@pytest.mark.parametrize("mode", sorted(T.MODES))
def test_launches_are_the_parent_commits(arithmetic, mode):
    want = T.unfold(GOLDEN["launches"][mode])
    got, _ = T.run_mode(mode, arithmetic)
    first = next((k for k, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    assert got == want, (f"{mode}: {len(got)} launches, {len(want)} stored; the first difference is at launch {first}: "
                         f"{got[first:first + 3]} against {want[first:first + 3]}")
