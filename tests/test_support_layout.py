"""The layout of the test tree: what two test modules share lives in a support module next to them (devtest, cshim, dev_append,
dev_take, dev_batch, cpu_batch, cpu_take, decode_harness, the *_cases modules), so that collecting one test file never imports
another with its fixtures and caches."""
import ast
import glob
import os

from conftest import ROOT


def test_no_test_module_imports_a_test_module():
    bad = []
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "test_*.py"))):
        for node in ast.walk(ast.parse(open(path).read())):
            if isinstance(node, ast.Import):
                names = [a.name for a in node.names]
            else:
                names = [node.module or ""] if isinstance(node, ast.ImportFrom) else []
            bad += [(os.path.basename(path), n) for n in names if n.split(".")[-1].startswith("test_")]
    assert not bad, bad
