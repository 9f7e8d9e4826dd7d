"""cenet_amd.ops re-exports exactly what its modules list in `__all__`; every `ops.<name>` the tree spells resolves."""
import glob
import importlib
import os
import re
import types

from cenet_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODULES = ("infra", "linear", "norm", "depthwise", "attention", "glue", "decoder_fused", "gates", "dseb_loss")


def test_every_module_lists_names_it_defines():
    seen = {}
    for m in MODULES:
        mod = importlib.import_module(f"cenet_amd.ops.{m}")
        assert isinstance(mod.__all__, list) and len(set(mod.__all__)) == len(mod.__all__), m
        for n in mod.__all__:
            obj = mod.__dict__[n]
            assert not isinstance(obj, types.ModuleType), (m, n)
            if isinstance(obj, (type, types.FunctionType)):
                assert obj.__module__ == mod.__name__, f"{m}.__all__ lists {n}, which {obj.__module__} defines"
            assert seen.setdefault(n, m) == m, f"{n} is listed by {seen[n]} and {m}"
        src = open(mod.__file__).read()
        assert not re.search(r"^from \.\w* import \*", src, flags=re.M), f"{m} star-imports"


def test_package_exports_no_modules():
    assert sorted(ops.__all__) == sorted(n for m in MODULES for n in importlib.import_module(f"cenet_amd.ops.{m}").__all__)
    for n in ops.__all__:
        assert not isinstance(getattr(ops, n), types.ModuleType), n
    for n in ("torch", "os", "math", "contextlib", "kern", "Function", "Optional"):
        assert n not in ops.__all__


def test_every_spelled_ops_name_resolves():
    files = [os.path.join(ROOT, "bench.py")]
    for d in ("tests", "tools", "cenet_amd"):
        files += glob.glob(os.path.join(ROOT, d, "**", "*.py"), recursive=True)
    names = {}
    for f in files:
        for n in re.findall(r"(?<![\w./])ops\.([A-Za-z_]\w*)", open(f).read()):  # (not torch.ops.aten, not a path)
            names.setdefault(n, os.path.relpath(f, ROOT))
    assert len(names) >= 90
    for n in ("_ZeroWs", "_WgradCfg", "_wgrad_side", "_prescaled_put", "_WG", "_zeros", "_WgradState", "_OffsetView"):
        assert n in names, n
    missing = {n: f for n, f in names.items() if not hasattr(ops, n)}
    assert not missing, f"spelled as ops.<name> but not on cenet_amd.ops: {missing}"
