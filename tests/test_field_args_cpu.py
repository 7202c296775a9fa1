"""The argument checks of the six field-domain entries and their four wrappers, without a GPU: return code and message, byte for byte and in
the precedence that the commit before csrc/field_lattice.h had (tests/golden/field_args_errors.json, written from that commit by
tests/golden/make_golden_field_args.py).  Section "c" calls the built library with made-up pointers -- every case is rejected by a check or
has n == 0 -- so it runs only where no device is visible: with one, a case whose check had gone missing would launch on those addresses;
without one it fails with PWS_EHIP, and this test with it."""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import field_args  # noqa: E402

with open(os.path.join(ROOT, "tests", "golden", "field_args_errors.json")) as _f:
    FIXTURE = json.load(_f)
C, PY = FIXTURE["c"], FIXTURE["python_cpu"]

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="made-up pointers: only where no device is visible")


@pytest.fixture(scope="module")
def lib():
    from pwstablenet_amd import build, hipabi
    build.build(verbose=False)
    return hipabi.lib()


def test_the_fixture_covers_every_entry():
    entries = {c["entry"] for c in C}
    assert entries == {"pws_field_zoom", "pws_field_compose", "pws_field_compose_rows", "pws_field_rigid", "pws_field_wobble", "pws_field_reach"}
    for e in entries:
        rows = [c for c in C if c["entry"] == e]
        assert any(c["rc"] == 0 and c["args"][1] == 0 for c in rows), e      # the n == 0 return
        assert len({c["message"] for c in rows if c["rc"] != 0}) >= 7, e       # (pws_field_zoom has seven checks, the others more)
    assert {c["rc"] for c in C} == {0, -22}
    assert {p["fn"] for p in PY} == {"zoom_fields", "compose_fields", "rigid_fields", "wobble_fields"}


@pytest.mark.parametrize("k", range(len(C)), ids=lambda k: "%s-%d" % (C[k]["entry"], k))
def test_c_code_and_message(lib, k):
    rc, message = field_args.call_c(lib, C[k])
    assert (rc, message) == (C[k]["rc"], C[k]["message"])


@pytest.mark.parametrize("k", range(len(PY)), ids=lambda k: "%s-%d" % (PY[k]["fn"], k))
def test_python_type_and_message(k):
    from pwstablenet_amd import functional as PF
    assert field_args.call_python(PF, PY[k], "cpu") == (PY[k]["exc"], PY[k]["message"])
