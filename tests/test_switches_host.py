"""CPU: the library's environment switches have one reader (spc_switch in spc_common.h), every one of them is set by something
in the tree and listed in docs/DESIGN_NOTES.md (8b), and the arithmetic of the masked
spatial stencil is a setting of the calling thread (spc_set_masked_spatial_form) behind ops.masked_spatial_arithmetic: it
nests, no other thread sees it, an exception restores it and the process environment is never written."""
import glob
import os
import re
import threading

import pytest

from conftest import REPO
from spectral_cube_amd import _lib, ops

ENV, SPLIT, RING = _lib.SPATIAL_FORM_ENV, _lib.SPATIAL_FORM_SPLIT, _lib.SPATIAL_FORM_RING


def _form():
    return _lib.load().spc_get_masked_spatial_form()


def _in_thread(body, timeout=5.0):
    """run *body* in a fresh thread (whose setting is the initial one) and hand back what it returns; a body that blocks -
    the lock the scope used to take was not reentrant - fails the test instead of hanging the suite"""
    box = {}

    def run():
        try:
            box["value"] = body()
        except BaseException as exc:           # noqa: B902 - handed to the caller's thread
            box["error"] = exc

    t = threading.Thread(target=run, daemon=True)
    t.start()
    t.join(timeout)
    assert not t.is_alive(), "the thread did not finish within %g s" % timeout
    if "error" in box:
        raise box["error"]
    return box["value"]


def test_the_constants_are_the_headers():
    hdr = open(os.path.join(REPO, "include", "spcube_hip.h")).read()
    for name, value in (("ENV", ENV), ("SPLIT", SPLIT), ("RING", RING)):
        assert "#define SPC_SPATIAL_FORM_%s" % name in hdr
        line = [ln for ln in hdr.splitlines() if ln.startswith("#define SPC_SPATIAL_FORM_%s" % name)][0]
        assert int(line.split()[2].strip("()")) == value
    assert ops.MASKED_SPATIAL_ARITHMETIC == ("f16-split", "f32")


def test_scopes_nest_on_one_thread():
    def body():
        seen = [_form()]
        with ops.masked_spatial_arithmetic("f32"):
            seen.append(_form())
            with ops.masked_spatial_arithmetic("f16-split"):
                seen.append(_form())
                with ops.masked_spatial_arithmetic("f16-split"):      # the same name again: the old lock stopped here
                    seen.append(_form())
                with ops.masked_spatial_arithmetic(None):             # no name: nothing changes
                    seen.append(_form())
            seen.append(_form())
        seen.append(_form())
        return seen

    assert _in_thread(body) == [ENV, RING, SPLIT, SPLIT, SPLIT, RING, ENV]


def test_a_scope_is_seen_by_its_own_thread_only_and_never_touches_the_environment(monkeypatch):
    monkeypatch.delenv("SPC_SPATIAL_RING", raising=False)
    before = _form()
    assert before == ENV and "SPC_SPATIAL_RING" not in os.environ
    with ops.masked_spatial_arithmetic("f32"):
        assert _form() == RING
        assert _in_thread(_form) == ENV                               # a thread starts with "follow the environment"

        def other():
            with ops.masked_spatial_arithmetic("f16-split"):
                return _form()

        assert _in_thread(other) == SPLIT and _form() == RING         # and its own scope does not reach this thread
        assert "SPC_SPATIAL_RING" not in os.environ
    assert _form() == ENV and "SPC_SPATIAL_RING" not in os.environ


def test_an_exception_inside_the_scope_restores_the_previous_value():
    def body():
        with ops.masked_spatial_arithmetic("f16-split"):
            with pytest.raises(RuntimeError, match="inside"):
                with ops.masked_spatial_arithmetic("f32"):
                    assert _form() == RING
                    raise RuntimeError("inside")
            inner = _form()
        return inner, _form()

    assert _in_thread(body) == (SPLIT, ENV)


def test_the_setter_returns_the_previous_value_and_ignores_what_is_no_form():
    def body():
        lib = _lib.load()
        out = [lib.spc_set_masked_spatial_form(RING), lib.spc_set_masked_spatial_form(7), lib.spc_get_masked_spatial_form(),
               lib.spc_set_masked_spatial_form(-2), lib.spc_set_masked_spatial_form(SPLIT), lib.spc_set_masked_spatial_form(ENV)]
        return out + [lib.spc_get_masked_spatial_form()]

    assert _in_thread(body) == [ENV, RING, RING, RING, RING, SPLIT, ENV]


def test_validation_and_messages_of_the_scope_are_unchanged():
    with pytest.raises(ValueError) as exc:
        ops.masked_spatial_arithmetic("f64")
    assert str(exc.value) == "arithmetic must be one of ('f16-split', 'f32'), got 'f64'"
    with ops.masked_spatial_arithmetic(None) as scope:
        assert scope.name is None and _form() == ENV


def test_the_environment_is_read_in_one_place():
    """every switch goes through spc_switch (spc_common.h): the C library's environment lookup is named once in csrc/"""
    hits = []
    for path in sorted(glob.glob(os.path.join(REPO, "spectral_cube_amd", "csrc", "*"))):      # whatever the suffix
        if not os.path.isfile(path):
            continue
        for i, line in enumerate(open(path, errors="replace"), 1):
            if "getenv" in line:
                hits.append((os.path.basename(path), i))
    assert len(hits) == 1 and hits[0][0] == "spc_common.h", hits


# ---- no switch without a setter -------------------------------------------------------------------------------------
# A switch of the library stays only while something in the tree gives it a value: a test, a tool, bench.py or the Python
# package.  The ones below are read and set by nothing, each for a reason:
UNSET_ON_PURPOSE = {
    "SPC_POOL_POISON": "a documented debugging feature of the buffer pool (include/spcube_hip.h), for whole-suite runs by hand",
    "SPC_MOMENTS_VEC": "spc_moments_workspace_bytes reads it beside SPC_MOMENTS_NSPLIT: the moment kernel's tuning set stays whole",
}
_READ = re.compile(r"""spc_switch(?:_text)?\(\s*"(SPC_[A-Z0-9_]+)\"""")
# set or forwarded: the name as a whole string literal (setenv, os.environ[...], os.environ.get, an env dict's key, a
# (name, value) pair) or as a keyword of dict(os.environ, NAME=...).  Prose that mentions NAME=0 sets nothing.
_SET = re.compile(r"""["'](SPC_[A-Z0-9_]+)["']|\b(SPC_[A-Z0-9_]+)\s*=\s*["']""")


def _switches_read():
    names = set()
    for path in sorted(glob.glob(os.path.join(REPO, "spectral_cube_amd", "csrc", "*"))):
        if os.path.isfile(path):
            names.update(_READ.findall(open(path, errors="replace").read()))
    return names


def _switches_set():
    paths = [os.path.join(REPO, "bench.py")] + glob.glob(os.path.join(REPO, "spectral_cube_amd", "*.py"))
    for top in ("tests", "tools"):
        for root, _dirs, files in os.walk(os.path.join(REPO, top)):
            paths += [os.path.join(root, f) for f in files if f.endswith((".py", ".sh"))]
    names = set()
    for path in paths:
        if os.path.abspath(path) == os.path.abspath(__file__):
            continue                                                   # the allow-list above sets nothing
        for quoted, keyword in _SET.findall(open(path, errors="replace").read()):
            names.add(quoted or keyword)
    return names


def test_every_switch_the_library_reads_is_set_by_something_in_the_tree():
    read, given = _switches_read(), _switches_set()
    assert len(read) > 20, "the search for spc_switch sites found too little: %s" % sorted(read)
    assert not (read - given - set(UNSET_ON_PURPOSE)), "read in csrc/ and set by nothing: %s" % sorted(read - given - set(UNSET_ON_PURPOSE))
    # (and the allow-list holds nothing that has gone or that something sets by now)
    assert set(UNSET_ON_PURPOSE) <= read - given, sorted(set(UNSET_ON_PURPOSE) - (read - given))


def test_the_design_notes_list_exactly_the_switches_that_are_read():
    notes = open(os.path.join(REPO, "docs", "DESIGN_NOTES.md")).read()
    table = notes.split("### The switches the library reads", 1)[1].split("\n## ", 1)[0]
    listed = re.findall(r"^\| `(SPC_[A-Z0-9_]+)` \|", table, flags=re.M)
    assert len(listed) == len(set(listed)), "a switch is listed twice"
    assert set(listed) == _switches_read()
