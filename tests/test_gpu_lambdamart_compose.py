"""Randomised soak of LambdaMART training with every training key drawn at once (tools/fuzz_lambdamart.py --compose,
--objective, --rank-objective; DESIGN.md section 11, "Randomised soak"): each run is a fresh child process that checks
every stage of every case against tests/lambdamart_composed_model.py.  tests/test_lambdamart_compose_host.py shows with
--dry, before any device is involved, that the same seeds draw and bind every key."""
import json
import os
import subprocess
import sys

import pytest

from tests import lambdamart_composed_model as cm

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("soak", sorted(cm.SOAKS))
def test_randomised_composed_soak(soak):
    flags, seed, iters = cm.SOAKS[soak]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz_lambdamart.py"), "--iters", str(iters), "--seed", str(seed)] + flags,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    print(out.stdout[-3000:])
    assert out.returncode == 0, out.stdout[-3000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["iters"] == iters and res["mismatches"] == 0 and res["ended_at_iter"] is None and res["both_error"] * 10 <= res["iters"]
    assert res["growers"].get("exact", 0) >= 1 and res["growers"].get("histogram", 0) >= 1
    assert res["sampled_views"] >= 1 and res["file_loaded"] >= 1
    assert sorted(res["bound"]) == sorted(cm.soak_bound_keys(flags))
    assert all(count >= 1 for count in res["bound"].values()), res["bound"]
