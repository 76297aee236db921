"""oracle/golden/registry.py against tests/golden/, on the CPU and without the reference: every fixture file has exactly one generator that claims it, every
claimed file is in the tree, every `needs` entry is some generator's output, the generators can be ordered, and listing the registry (or importing any module of
the package) loads neither torch nor the reference, so that nothing of it can reach a machine where only the fixtures exist."""
import os
import subprocess
import sys
from collections import Counter

import pytest

from oracle.golden import registry

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = [o for g in registry.GENERATORS for o in g.outputs]


def test_every_fixture_has_one_generator():
    tree = sorted(f"tests/golden/{f}" for f in os.listdir(os.path.join(REPO, "tests", "golden")))
    claims = Counter(OUTPUTS)
    assert [f for f in tree if claims[f] != 1] == []


def test_outputs_exist_and_are_claimed_once():
    assert [o for o in OUTPUTS if not os.path.isfile(os.path.join(REPO, o))] == []
    assert [o for o, n in Counter(OUTPUTS).items() if n > 1] == []
    assert len({g.name for g in registry.GENERATORS}) == len(registry.GENERATORS)
    assert all(callable(g.run) for g in registry.GENERATORS)


def test_needs_are_outputs_and_the_graph_has_an_order():
    assert [(g.name, n) for g in registry.GENERATORS for n in g.needs if n not in OUTPUTS] == []
    order = registry.ordered()
    assert sorted(g.name for g in order) == sorted(g.name for g in registry.GENERATORS)
    seen = set()
    for g in order:
        assert set(g.needs) <= seen, g.name
        seen |= set(g.outputs)
    # a subset keeps the order among its members; a need outside it is read from the tree
    assert [g.name for g in registry.ordered(["acq", "consts"])] == ["consts", "acq"]
    assert [g.name for g in registry.ordered(["dec_loss"])] == ["dec_loss"]


def test_a_cycle_is_reported(monkeypatch):
    a = registry.Generator("a", ("tests/golden/a.npz",), ("tests/golden/b.npz",), print)
    b = registry.Generator("b", ("tests/golden/b.npz",), ("tests/golden/a.npz",), print)
    monkeypatch.setattr(registry, "GENERATORS", (a, b))
    monkeypatch.setattr(registry, "BY_NAME", {"a": a, "b": b})
    with pytest.raises(ValueError, match="cycle"):
        registry.ordered()


def test_list_and_import_need_no_reference(tmp_path):
    env = dict(os.environ, RADAE_REFERENCE=str(tmp_path / "absent"))
    r = subprocess.run([sys.executable, "-m", "oracle.golden", "--list"], cwd=REPO, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert all(g.name in r.stdout for g in registry.GENERATORS) and all(o in r.stdout for o in OUTPUTS)
    mods = sorted(f[:-3] for f in os.listdir(os.path.join(REPO, "oracle", "golden")) if f.endswith(".py") and f != "__init__.py")
    code = ("import os, sys, importlib; cwd = os.getcwd(); import oracle.golden\n"
            f"for m in {mods!r}: importlib.import_module('oracle.golden.' + m)\n"
            "import numpy\n"
            "bad = [m for m in ('torch', 'radae', 'matplotlib') if m in sys.modules]\n"
            "assert not bad and os.getcwd() == cwd and numpy.random.randint.__name__ == 'randint', bad")
    r = subprocess.run([sys.executable, "-c", code], cwd=REPO, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
