"""The PWS_OPT_EXPERIMENT registry (pwstablenet_amd/csrc/experiments.h): named, disjoint ids, read only through the registry, mirrored by
hipabi.Exp, and never set from tests or tools as a bare number."""
import ast
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pwstablenet_amd", "csrc")
ENTRY = re.compile(r"^\s+EXP_(\w+) = (\d+),\s*//\s*(?:\[(\d+)\])?")


def _registry():
    """{name: (id, span)} from enum Exp."""
    out = {}
    with open(os.path.join(CSRC, "experiments.h")) as f:
        for line in f:
            m = ENTRY.match(line)
            if m:
                out[m.group(1)] = (int(m.group(2)), int(m.group(3) or 1))
    return out


def test_registry_ids_and_ranges_are_disjoint():
    reg = _registry()
    assert len(reg) > 40
    spans = sorted((v, v + n, name) for name, (v, n) in reg.items())
    assert spans[0][0] > 0, "0 is the product"
    for (a0, a1, an), (b0, b1, bn) in zip(spans, spans[1:]):
        assert a1 <= b0, "%s [%d, %d) overlaps %s [%d, %d)" % (an, a0, a1, bn, b0, b1)


def test_range_reads_use_the_registry_span():
    reg = _registry()
    for fn in sorted(os.listdir(CSRC)):
        if fn == "experiments.h" or not fn.endswith((".h", ".hip", ".cpp")):
            continue
        with open(os.path.join(CSRC, fn)) as f:
            src = f.read()
        for name, n in re.findall(r"exp_(?:in|mask)\(EXP_(\w+), (\d+)\)", src):
            assert reg[name][1] == int(n), (fn, name, n, reg[name])
        for name in re.findall(r"exp_is\(EXP_(\w+)\)", src):
            assert reg[name][1] == 1, (fn, name, "is a range")


def test_only_the_registry_and_the_abi_name_g_experiment():
    users = sorted(fn for fn in os.listdir(CSRC) if os.path.isfile(os.path.join(CSRC, fn)) and "g_experiment" in open(os.path.join(CSRC, fn)).read())
    assert users == ["abi.cpp", "experiments.h"], users


def test_hipabi_exp_mirrors_the_header():
    from pwstablenet_amd import hipabi
    mirror = {k: v for k, v in vars(hipabi.Exp).items() if not k.startswith("_")}
    assert mirror == {name: v for name, (v, _) in _registry().items()}


def _literal_experiment_sets(path):
    """(line, literals) of every pws_set_option(<experiment key>, ...) and experiment(...) call in a Python file whose id is written
    with a nonzero integer literal."""
    with open(path) as f:
        tree = ast.parse(f.read(), path)
    out = []
    for node in ast.walk(tree):
        if not isinstance(node, ast.Call):
            continue
        name = node.func.attr if isinstance(node.func, ast.Attribute) else getattr(node.func, "id", None)
        if name == "pws_set_option" and len(node.args) == 2:
            key, val = node.args
            if not ((isinstance(key, ast.Constant) and key.value == 100) or (isinstance(key, ast.Attribute) and key.attr == "OPT_EXPERIMENT")):
                continue
        elif name == "experiment" and len(node.args) == 1:
            val = node.args[0]
        else:
            continue
        literal = [n.value for n in ast.walk(val) if isinstance(n, ast.Constant) and isinstance(n.value, int) and n.value != 0]
        if literal:
            out.append((node.lineno, literal))
    return out


def test_tests_and_tools_set_experiments_by_name():
    files = [os.path.join(ROOT, "tests", f) for f in os.listdir(os.path.join(ROOT, "tests")) if f.endswith(".py")]
    for d in ("tools", os.path.join("tools", "probes")):
        files += [os.path.join(ROOT, d, f) for f in os.listdir(os.path.join(ROOT, d)) if f.endswith(".py")]
    bad = {os.path.relpath(p, ROOT): hits for p in sorted(files) for hits in [_literal_experiment_sets(p)] if hits}
    assert not bad, bad
