"""The argument checks of zoom_fields, compose_fields, rigid_fields and wobble_fields that look at device tensors: exception type and message,
word for word and in the precedence that the commit before csrc/field_lattice.h had (section "python_device" of
tests/golden/field_args_errors.json, recorded on an MI355X from that commit's package by tests/golden/make_golden_field_args.py --device).
Fields of 1 x 2 x 2 x 2; every case is a rejection, so no kernel is launched."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import field_args  # noqa: E402

with open(os.path.join(ROOT, "tests", "golden", "field_args_errors.json")) as _f:
    PY = json.load(_f)["python_device"]

pytestmark = pytest.mark.gpu


def test_the_fixture_covers_every_wrapper():
    for fn in ("zoom_fields", "compose_fields", "rigid_fields", "wobble_fields"):
        assert len({p["message"] for p in PY if p["fn"] == fn}) >= 8, fn


@pytest.mark.parametrize("k", range(len(PY)), ids=lambda k: "%s-%d" % (PY[k]["fn"], k))
def test_python_type_and_message(k):
    from pwstablenet_amd import functional as PF
    assert field_args.call_python(PF, PY[k], "cuda") == (PY[k]["exc"], PY[k]["message"])
