"""The kernel-library calls of the HIP step program against a recorded trace (GPU only).

``tests/golden/launch_trace.json`` holds, per case of ``scripts/launch_trace.py``'s grid,
the name and a digest of the normalised arguments of every library call made while the
engine is constructed, in the first two training steps and in one prediction.  A change
to the program that is meant to launch what it launched before (a refactor of the
lowering, the planners or the step) must reproduce every call; a change that is meant to
launch something else records the file again with ``scripts/launch_trace.py --write``.
"""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("launch_trace", os.path.join(_ROOT, "scripts", "launch_trace.py"))
LT = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(LT)

with open(os.path.join(_ROOT, "tests", "golden", "launch_trace.json")) as _f:
    GOLDEN = LT.unpack(json.load(_f))
GRID = LT.grid()


def test_fixture_covers_the_grid():
    assert sorted(GOLDEN) == sorted(GRID)


@pytest.mark.parametrize("name", list(GRID))
def test_launch_trace_matches_recorded(name):
    diff = LT.first_difference(LT.trace(GRID[name]), GOLDEN[name])
    if diff is not None:
        print(f"{name}: {diff}")
    assert diff is None, f"{name}: {diff}"
