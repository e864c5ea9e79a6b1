"""tests/test_gpu_lane_forms.py leaves out the setting combinations that feature tests run, by
three maps that name those tests.  Every test named there must exist, with the parameters the
name carries: a renamed or removed feature test must not silently take a combination's only
test with it.  No GPU: the files are parsed, not run."""
import ast
import importlib.util
import re
from pathlib import Path

HERE = Path(__file__).resolve().parent


def lane_forms():
    spec = importlib.util.spec_from_file_location("lane_forms_tables", HERE / "test_gpu_lane_forms.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def parametrize_values(fn):
    """The literal values of a test function's pytest.mark.parametrize decorators, as strings."""
    vals = set()
    for d in fn.decorator_list:
        if isinstance(d, ast.Call) and ast.unparse(d.func).endswith("parametrize"):
            for v in ast.walk(d.args[1]):
                if isinstance(v, ast.Constant):
                    vals.add(str(v.value))
    return vals


def test_every_named_test_exists():
    t = lane_forms()
    named = list(t.COVERED.values()) + list(t.RAW_COVERED.values()) + list(t.PREPARED_COVERED.values())
    assert len(named) == 18 + 9 + 4
    trees = {}
    for name in named:
        m = re.fullmatch(r"(test_\w+)::(test_\w+)(?:\[(.*)\])?", name)
        assert m, name
        module, test, params = m.groups()
        path = HERE / (module + ".py")
        assert path.exists(), name
        if module not in trees:
            trees[module] = {n.name: n for n in ast.parse(path.read_text()).body
                             if isinstance(n, ast.FunctionDef)}
        assert test in trees[module], name
        if params:
            have = parametrize_values(trees[module][test])
            for p in params.split("-"):
                assert p in have, (name, p)


def test_the_cases_are_the_complement():
    t = lane_forms()
    assert len(t.CASES) + len(t.COVERED) == 96
    assert len(t.RAW_CASES) + len(t.RAW_COVERED) == 24
    assert len(t.PREPARED_CASES) + len(t.PREPARED_COVERED) == 8
