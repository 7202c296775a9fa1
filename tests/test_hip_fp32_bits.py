"""The fp32 generator forward of bench.py's configs[1] holds its bits: batch 8, ngf 64, on the synth weights W1 and W2 and the
inputs of tests/test_hip_timed_path.py, eager and as a graph replay.  The SHA-256 of the field's bytes must equal digests recorded
on an MI355X.

Kernel changes that only reshape the work (unit sizes, workgroups per CU, schedules) keep every product and every sum in its order and
must leave these digests alone.  A change to the fp32 arithmetic order (K order, split-K, another matrix instruction, another
Winograd transform) changes them by design: then regenerate them on an MI355X with

    python tests/test_hip_fp32_bits.py

which prints the table below, and say in the commit why the order changed (tools/parity_budget.py gives the parity it costs).
"""
import hashlib
import os
import sys

import pytest

# (weights, mode) -> sha256 of the field tensor's bytes (float32, [8, 256, 256, 2]); recorded on an MI355X from the commit before
# the stride-2 ring kernel's half workgroups
DIGESTS = {
    ("W1", "eager"): "38035ee53cbe847bfec5c3dfde172929ee89e31930fdb96fcf988bfb060a921a",
    ("W1", "graph"): "38035ee53cbe847bfec5c3dfde172929ee89e31930fdb96fcf988bfb060a921a",
    ("W2", "eager"): "91db8595c4ba153aac5eb1bed925591777a2857c30d2a71614680752db13e574",
    ("W2", "graph"): "91db8595c4ba153aac5eb1bed925591777a2857c30d2a71614680752db13e574",
}


def field_digests(kind):
    import torch

    from pwstablenet_amd import synth
    from pwstablenet_amd.lib.networks_cascading import define_G
    net = define_G(31, 2, 64, "normal", 0.02)
    net.load_state_dict({"module." + k: torch.from_numpy(v) for k, v in synth.make_weights(kind, seed=123, ngf=64)})
    net = net.cuda()
    x = torch.from_numpy(synth.noise_window(8, 31, 256, seed=123)).cuda()
    with torch.no_grad():
        eager = net(x, False).clone()
        net.module.enable_graph(True)
        net(x, False)              # capture + first replay
        graph = net(x, False)      # replay
    torch.cuda.synchronize()
    assert net.module._graph is not None
    sha = lambda t: hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()   # noqa: E731
    return {(kind, "eager"): sha(eager), (kind, "graph"): sha(graph)}


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["W1", "W2"])
def test_fp32_forward_field_bits(hip, kind):
    assert hip.lib().pws_get_option(hip.OPT_TWO_QUEUES) == 1   # the product default, what the bench times
    got = field_digests(kind)
    for key, digest in got.items():
        assert digest == DIGESTS[key], ("fp32 field bits changed for %s %s: %s (recorded %s); see the module docstring" % (key + (digest, DIGESTS[key])))


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    out = {}
    for k in ("W1", "W2"):
        out.update(field_digests(k))
    for key in sorted(out):
        print("    %r: %r," % (key, out[key]))
