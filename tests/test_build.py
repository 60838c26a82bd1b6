"""build.py's source list: what it names exists, what csrc/ holds is named, and a missing source is refused instead of left out."""
import os

import pytest

from conftest import pkg


def test_every_source_is_listed_and_exists():
    b = pkg("build")
    assert all(os.path.exists(os.path.join(b.CSRC, s)) for s in b.SOURCES)
    own_programs = {"pyngp.cpp", "ngp_main.cpp"}  # build_pyngp and build_main compile these against the library
    on_disk = {f for f in os.listdir(b.CSRC) if f.endswith((".cpp", ".hip"))} - own_programs
    assert on_disk == set(b.SOURCES) and len(set(b.SOURCES)) == len(b.SOURCES)


def test_a_missing_source_is_refused(monkeypatch):
    b = pkg("build")
    monkeypatch.setattr(b, "SOURCES", b.SOURCES + ["no_such_unit.cpp"])
    with pytest.raises(RuntimeError, match="no_such_unit.cpp"):  # (before any compiler runs: the library on disk is left alone)
        b.build(force=True)
