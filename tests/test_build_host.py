"""The build's staleness bookkeeping (fastrank_amd/_build.py), without a compiler: every unit depends on exactly the files its
source includes, and a change to any of them changes that unit's digest and no other unit's."""
import os
import re
import shutil

from fastrank_amd import _build


def include_closure(csrc, src):
    """The quoted includes reachable from `src`, as normalised paths relative to `csrc` (restated here, not taken from _build)."""
    found, stack = set(), [src]
    while stack:
        cur = stack.pop()
        text = open(os.path.join(csrc, cur)).read()
        for line in text.splitlines():
            m = re.match(r'\s*#\s*include\s*"(.+?)"', line)
            if m is None:
                continue
            name = os.path.normpath(os.path.join(os.path.dirname(cur), m.group(1)))
            if name not in found:
                found.add(name)
                stack.append(name)
    return found


def test_every_unit_depends_on_the_closure_of_its_includes():
    units = _build.units()
    assert [u[0] for u in units[:3]] == ["device.o", "capi.o", "explain.o"] and len(units) == 3 + _build.fv_parts()
    for obj, src, _, deps in units:
        assert len(deps) == len(set(deps)) and src not in deps, obj
        assert set(deps) == include_closure(_build.CSRC, src), obj
        assert all(os.path.isfile(os.path.join(_build.CSRC, d)) for d in deps), obj
    assert [u[3] for u in units] == [u[3] for u in _build.units()], "the order is deterministic"
    by_obj = {u[0]: set(u[3]) for u in units}
    assert {"dataset_build.inc", "train_rf.inc", "train_lambda.inc", "train_dart.inc", "train_hist.inc", "device_dataset.inc",
            "score_trees.inc", "forest_pack.hpp",
            "kernels_fillnet.inc"} <= by_obj["device.o"]  # (kernels_fillnet.inc: through kernels_verify.inc only)
    assert "forest_pack.hpp" in by_obj["capi.o"]
    assert os.path.join("..", "..", "include", "fastrank.h") in by_obj["capi.o"]
    assert "dataset_layout.hpp" in by_obj["fullverify_0.o"]  # (through device.hpp)


def test_a_byte_in_any_dependency_changes_the_digest_of_the_units_that_include_it(tmp_path, monkeypatch):
    root = os.path.dirname(os.path.dirname(_build.CSRC))
    csrc = str(tmp_path / "fastrank_amd" / "csrc")
    shutil.copytree(_build.CSRC, csrc)
    shutil.copytree(os.path.join(root, "include"), str(tmp_path / "include"))
    monkeypatch.setattr(_build, "CSRC", csrc)
    units = _build.units()
    before = {obj: _build._digest(src, extra, deps) for obj, src, extra, deps in units}
    assert len(set(before.values())) == len(units)
    files = set()
    for _, src, _, deps in units:
        files |= {src} | set(deps)
    assert len(files) > 30
    for name in sorted(files):
        path = os.path.join(csrc, name)
        size = os.path.getsize(path)
        with open(path, "ab") as fh:
            fh.write(b" ")
        for obj, src, extra, deps in units:
            changed = _build._digest(src, extra, deps) != before[obj]
            assert changed == (name == src or name in deps), (name, obj)
        os.truncate(path, size)
    assert {obj: _build._digest(src, extra, deps) for obj, src, extra, deps in units} == before
