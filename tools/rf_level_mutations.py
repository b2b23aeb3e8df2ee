#!/usr/bin/env python3
"""Do the level tests have teeth?  Flips one detail of tests/rf_level_model.py at a time -- the squared-error tail summed
before the chain, equal feature values in descending r (what an unstable sort may leave), searchsorted 'right' -- and lists
the cases of tests/test_gpu_rf_levels.py that notice (needs an MI355X).  Every mutation must fail at least one case; the
unmutated restatement must fail none.
Usage: python tools/rf_level_mutations.py"""
import contextlib
import functools
import io
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import rf_level_model as lm  # noqa: E402

MUTATIONS = (("none", {}), ("squared-error tail before the chain", {"tail_first": True}),
             ("equal values in descending r", {"stable": False}), ("searchsorted right", {"side": "right"}))


class Collect:
    def __init__(self):
        self.failed, self.passed = [], []

    def pytest_runtest_logreport(self, report):
        if report.when == "call":
            (self.failed if report.failed else self.passed).append(report.nodeid.split("::")[-1])


def main():
    grow, bad = lm.grow, 0
    for name, kw in MUTATIONS:
        lm.grow = functools.partial(grow, **kw)
        c = Collect()
        with contextlib.redirect_stdout(io.StringIO()):
            pytest.main([os.path.join(ROOT, "tests", "test_gpu_rf_levels.py"), "-q", "-m", "gpu", "-p", "no:cacheprovider", "--tb=no"], plugins=[c])
        print("%s: %d failed, %d passed; failed: %s" % (name, len(c.failed), len(c.passed), ", ".join(c.failed)), flush=True)
        bad += int((len(c.failed) == 0) != (not kw) or not (c.failed or c.passed))
    lm.grow = grow
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
