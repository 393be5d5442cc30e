"""build.py lists every HIP source once, and the contraction rule holds for every includer (CPU).

The device bodies of pgf_step_dev.h and the sums of pgf_reduce_dev.h are bit-exact with numpy
expressions and with each other only when no multiply-add is fused behind their back: every
translation unit that includes one of them, directly or through project headers, must be compiled
with -ffp-contract=off.
"""

import os
import re

from pygradflow_amd import build

NO_CONTRACT_HEADERS = {"pgf_step_dev.h", "pgf_reduce_dev.h"}


def _project_includes(name, seen=None):
    """Every pgf_* header `name` includes, textually and transitively."""
    seen = set() if seen is None else seen
    text = open(os.path.join(build.CSRC, name)).read()
    for inc in re.findall(r'^\s*#\s*include\s+"(pgf_[^"]+)"', text, flags=re.M):
        if inc not in seen:
            seen.add(inc)
            _project_includes(inc, seen)
    return seen


def test_every_source_listed_once_and_present():
    listed = [src for src, _ in build.SOURCES]
    on_disk = sorted(f for f in os.listdir(build.CSRC) if f.endswith(".hip"))
    assert sorted(listed) == on_disk
    assert len(set(listed)) == len(listed)
    assert sorted(build.NO_CONTRACT + build.CONTRACT) == sorted(listed)
    assert not set(build.NO_CONTRACT) & set(build.CONTRACT)
    for src, extra in build.SOURCES:
        assert ("-ffp-contract=off" in extra) == (src in build.NO_CONTRACT), src


def test_includers_of_the_step_bodies_are_compiled_without_contraction():
    includers = [src for src, _ in build.SOURCES if _project_includes(src) & NO_CONTRACT_HEADERS]
    # the three step-kernel files, the line search and the unsymmetric step at the least
    assert {"pgf_kernels.hip", "pgf_guard_kernels.hip", "pgf_batch_kernels.hip", "pgf_line_search.hip",
            "pgf_unsym.hip"} <= set(includers)
    for src in includers:
        assert src in build.NO_CONTRACT, src
