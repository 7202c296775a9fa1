"""What tests/golden/make_golden_field_args.py (which records, at the commit before csrc/field_lattice.h) and the two tests that replay its
fixture share: how a recorded case becomes a call.

Section "c": {"entry", "args", "rc", "message"} -- ``args`` as ctypes takes them: integers for pointers (made up: every case is rejected by a
check or has n == 0, so no address is used), null for NULL, numbers.
Section "python": {"fn", "args", "kwargs", "exc", "message"[, "device"]} -- a tensor is written {"t": shape, "dtype": name} with optional
"host": true (it stays on the CPU), "strided": true (every other element of a tensor twice as wide: not contiguous), "alias": name (the
transposed view of that argument's memory: same address, not contiguous) or "same": name (that argument itself)."""
import torch


def call_c(lib, case):
    """(rc, message) of one recorded C call."""
    rc = getattr(lib, case["entry"])(*case["args"])
    return rc, (lib.pws_last_error().decode() if rc != 0 else "")


def _tensor(spec, device):
    shape = list(spec["t"])
    dev = "cpu" if spec.get("host") else device
    if spec.get("strided"):
        return torch.zeros(shape[:-1] + [2 * shape[-1]], dtype=getattr(torch, spec["dtype"]), device=dev)[..., ::2]
    return torch.zeros(shape, dtype=getattr(torch, spec["dtype"]), device=dev)


def call_python(PF, case, device):
    """(exception's type name, message) of one recorded wrapper call on ``device``; (None, None) if it returns."""
    named = dict(zip(case["names"], case["args"]))
    named.update(case["kwargs"])
    built = {k: _tensor(v, device) for k, v in named.items() if isinstance(v, dict) and "t" in v}
    for k, v in named.items():
        if isinstance(v, dict) and "alias" in v:
            built[k] = built[v["alias"]].transpose(1, 2)
        elif isinstance(v, dict) and "same" in v:
            built[k] = built[v["same"]]
    value = {k: built.get(k, v) for k, v in named.items()}
    try:
        getattr(PF, case["fn"])(*[value[k] for k in case["names"]], **{k: value[k] for k in case["kwargs"]})
    except Exception as e:   # (recorded by type: the wrappers raise ValueError, hipabi.require_cuda RuntimeError)
        return type(e).__name__, str(e)
    return None, None
