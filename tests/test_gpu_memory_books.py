"""The engine's books (Engine.memory(), tw_debug_memory) over the tour of tools/memory_books.py, step by step, against
tests/golden/memory_books_parent.json: what the library reported at every step of the same tour before its buffers got
owning types that enter each allocation in the books when it is made (profiles/engine_buffers.md).  The recorded report
derived every allocation's size again from the engine's parameters, slack included, so the equality ties the running
totals to the sizes that are allocated: a buffer that misses the books, or enters them with another size, moves the step
that creates it.  Sums of allocation sizes: no tolerance."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import memory_books as MB  # noqa: E402

pytestmark = pytest.mark.gpu


def test_the_books_equal_the_parents_at_every_step(twflow):
    with open(os.path.join(ROOT, "tests", "golden", "memory_books_parent.json")) as f:
        want = json.load(f)
    got = MB.tour(twflow)
    assert [name for name, _ in got] == [name for name, _ in want]
    for (name, mine), (_, parents) in zip(got, want):
        assert mine == parents, name
