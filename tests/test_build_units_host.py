"""The units the build gained after tests/test_build_host.py pinned its list (fastrank_amd/_build.py: feature_units, all_units),
held to the same rules without a compiler: each depends on exactly the files its source includes, a byte in any of them
changes that unit's digest and the library's, and the pinned units' digests do not depend on the new sources."""
import os
import shutil

from fastrank_amd import _build
from tests.test_build_host import include_closure


def test_all_units_are_the_pinned_ones_then_the_feature_units():
    extra = _build.feature_units()
    assert [u[0] for u in extra] == ["normalize.o"] and _build.all_units() == _build.units() + extra
    assert len({u[0] for u in _build.all_units()}) == len(_build.all_units())
    for obj, src, _, deps in extra:
        assert len(deps) == len(set(deps)) and src not in deps, obj
        assert set(deps) == include_closure(_build.CSRC, src), obj
        assert all(os.path.isfile(os.path.join(_build.CSRC, d)) for d in deps), obj
    assert set(extra[0][3]) == {"normalize.hpp"}  # no HIP-free host header, none of device.o's sources
    by_obj = {u[0]: set(u[3]) for u in _build.units()}
    assert {"normalize_host.hpp", "normalize.hpp"} <= by_obj["capi.o"]
    for obj in by_obj:
        if obj != "capi.o":
            assert not {"normalize.hip", "normalize.hpp", "normalize_host.hpp"} & by_obj[obj], obj


def test_a_byte_in_the_new_sources_changes_their_unit_and_the_library(tmp_path, monkeypatch):
    root = os.path.dirname(os.path.dirname(_build.CSRC))
    csrc = str(tmp_path / "fastrank_amd" / "csrc")
    shutil.copytree(_build.CSRC, csrc)
    shutil.copytree(os.path.join(root, "include"), str(tmp_path / "include"))
    monkeypatch.setattr(_build, "CSRC", csrc)
    units = _build.all_units()
    before = {obj: _build._digest(src, extra, deps) for obj, src, extra, deps in units}
    lib_before = _build._lib_digest()
    assert len(set(before.values())) == len(units)
    for name in ("normalize.hip", "normalize.hpp", "normalize_host.hpp"):
        path = os.path.join(csrc, name)
        size = os.path.getsize(path)
        with open(path, "ab") as fh:
            fh.write(b" ")
        for obj, src, extra, deps in units:
            changed = _build._digest(src, extra, deps) != before[obj]
            assert changed == (name == src or name in deps), (name, obj)
        assert _build._lib_digest() != lib_before, name
        os.truncate(path, size)
    assert _build._lib_digest() == lib_before
