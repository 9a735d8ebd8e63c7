"""The layout of the suite itself: shared scaffolding lives in plain modules (gpu_support.py, *_cases.py, output_checks.py),
never in a test module that another imports, and each of the small helpers the GPU suites once copied has one definition."""
import ast
import glob
import os

HERE = os.path.dirname(os.path.abspath(__file__))
ONE_DEFINITION = ["api", "host_crc", "oracle_bytes", "controls", "cut", "ints", "write_wav", "run_cli", "dev", "sync", "cur_stream"]


def test_no_module_imports_a_test_module_and_shared_helpers_are_defined_once():
    defined = {name: [] for name in ONE_DEFINITION}
    for path in sorted(glob.glob(os.path.join(HERE, "*.py"))):
        module = os.path.basename(path)
        tree = ast.parse(open(path).read(), path)
        for node in ast.walk(tree):
            names = [a.name for a in node.names] if isinstance(node, ast.Import) else [node.module or ""] if isinstance(node, ast.ImportFrom) else []
            bad = [n for n in names if n.split(".")[-1].startswith("test_")]
            assert not bad, "%s imports the test module %s: what it needs belongs in a cases or support module" % (module, bad[0])
        for node in tree.body:
            if isinstance(node, (ast.FunctionDef, ast.ClassDef)) and node.name in defined:
                defined[node.name].append(module)
    many = {name: where for name, where in defined.items() if len(where) > 1}
    assert not many, "defined at top level in more than one module: %s" % many
