"""CPU: the library's environment switches have one reader (spc_switch in spc_common.h), and the arithmetic of the masked
spatial stencil is a setting of the calling thread (spc_set_masked_spatial_form) behind ops.masked_spatial_arithmetic: it
nests, no other thread sees it, an exception restores it and the process environment is never written."""
import glob
import os
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
