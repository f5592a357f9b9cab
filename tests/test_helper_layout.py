"""Where the tests' helpers live: no test module imports another, no helper is defined twice in the test modules,
and the helper modules hold no tests.  `ast` work over tests/*.py; no GPU and nothing is imported."""
import ast
import collections
import glob
import os

HERE = os.path.dirname(os.path.abspath(__file__))
TREES = {os.path.basename(p)[:-3]: ast.parse(open(p).read()) for p in sorted(glob.glob(os.path.join(HERE, "*.py")))}
TESTS = {name: tree for name, tree in TREES.items() if name.startswith("test_")}
DEFS = (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)


def _is_test_module(name):
    return name.startswith(("tests.test_", "test_"))


def test_no_test_module_imports_another():
    """at any depth: an import inside a function counts"""
    found = []
    for name, tree in TESTS.items():
        for node in ast.walk(tree):
            if isinstance(node, ast.Import):
                found += ["%s: import %s" % (name, a.name) for a in node.names if _is_test_module(a.name)]
            elif isinstance(node, ast.ImportFrom):
                module = node.module or ""
                found += ["%s: from %s import %s" % (name, module, a.name) for a in node.names if _is_test_module(module) or _is_test_module(a.name)]
    assert not found, "\n".join(found)


def _body(node):
    """a definition as text, its docstring aside"""
    body = node.body[1:] if ast.get_docstring(node, clean=False) is not None else node.body
    return ast.dump(type(node)(**dict(ast.iter_fields(node), body=body)))


def test_no_helper_is_defined_in_two_test_modules():
    where = collections.defaultdict(list)
    for name, tree in TESTS.items():
        for node in tree.body:
            if isinstance(node, DEFS) and not node.name.startswith("test_"):
                where[_body(node)].append("%s.%s" % (name, node.name))
    twice = sorted(", ".join(v) for v in where.values() if len(v) > 1)
    assert not twice, "\n".join(twice)


def test_helper_modules_define_no_tests():
    found = []
    for name, tree in TREES.items():
        for node in ast.walk(tree) if name not in TESTS else ():
            names = [node.name] if isinstance(node, DEFS) else [t.id for t in node.targets if isinstance(t, ast.Name)] if isinstance(node, ast.Assign) else []
            found += ["%s.%s" % (name, n) for n in names if n.startswith("test_")]
    assert not found, "\n".join(found)
