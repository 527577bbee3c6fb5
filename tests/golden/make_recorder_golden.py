#!/usr/bin/env python3
"""Generate tests/golden/recorder_kats.json: the known answers of the reference's interpolation tests
(tests/test_interpolation.py: every `interp(t) == value`, `interp(t) is interp.no_value`, `interp(t) is None` and
`np.allclose(interp(t), value)` after a `timestream = [...]` and an `interp = interpolator.<Class>(timestream, **kw)`), the
eleven recorded property names and the two interpolator tables of recorder/__init__.py, all extracted with `ast` as
make_golden.py extracts the render known answers.  Data only; runs where the reference checkout is mounted."""
import ast
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, REF  # noqa: E402


def _value(node):
    """A literal, or np.eye(n) / np.array(literal), as plain JSON data."""
    if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "eye":
        n = ast.literal_eval(node.args[0])
        return [[1.0 if i == j else 0.0 for j in range(n)] for i in range(n)]
    if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "array":
        return _value(node.args[0])
    if isinstance(node, (ast.List, ast.Tuple)):
        return [_value(e) for e in node.elts]
    return ast.literal_eval(node)


def _interp_call(node):
    """t of `interp(t)`, else None"""
    if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == "interp" and len(node.args) == 1:
        try:
            return ast.literal_eval(node.args[0])
        except ValueError:
            return None
    return None


def interpolation_cases(path):
    cases = []
    for fn in [n for n in ast.parse(open(path).read()).body if isinstance(n, ast.FunctionDef)]:
        case = {"test": fn.name, "checks": []}
        for stmt in fn.body:
            if isinstance(stmt, ast.Assign) and isinstance(stmt.targets[0], ast.Name):
                name = stmt.targets[0].id
                if name == "timestream":
                    case["timestream"] = _value(stmt.value)
                elif name == "interp":
                    case["class"] = stmt.value.func.attr
                    case["kwargs"] = {k.arg: ast.literal_eval(k.value) for k in stmt.value.keywords}
            elif isinstance(stmt, ast.Assert):
                test = stmt.test
                if isinstance(test, ast.Compare) and len(test.ops) == 1 and _interp_call(test.left) is not None:
                    t, op, right = _interp_call(test.left), test.ops[0], test.comparators[0]
                    if isinstance(op, ast.Eq):
                        case["checks"].append({"t": t, "kind": "eq", "value": _value(right)})
                    elif isinstance(op, ast.Is) and isinstance(right, ast.Attribute) and right.attr == "no_value":
                        case["checks"].append({"t": t, "kind": "no_value"})
                    elif isinstance(op, ast.Is) and isinstance(right, ast.Constant) and right.value is None:
                        case["checks"].append({"t": t, "kind": "is_none"})
                elif (isinstance(test, ast.Call) and isinstance(test.func, ast.Attribute) and test.func.attr == "allclose"
                      and _interp_call(test.args[0]) is not None):
                    case["checks"].append({"t": _interp_call(test.args[0]), "kind": "allclose", "value": _value(test.args[1])})
        if "timestream" in case and "class" in case:
            cases.append(case)
    return cases


def recorder_tables(path):
    """The class attributes _record_properties and the two _record_interpolation_class_* lists (names only)."""
    out = {}
    for cls in [n for n in ast.walk(ast.parse(open(path).read())) if isinstance(n, ast.ClassDef)]:
        for stmt in cls.body:
            if isinstance(stmt, ast.Assign) and isinstance(stmt.targets[0], ast.Name):
                name = stmt.targets[0].id
                if name == "_record_properties":
                    out["properties"] = ast.literal_eval(stmt.value)
                elif name.startswith("_record_interpolation_class_"):
                    out[name[len("_record_interpolation_class_"):]] = [e.id for e in stmt.value.elts]
    return out


def main():
    data = {"interpolation": interpolation_cases(os.path.join(REF, "tests", "test_interpolation.py"))}
    data.update(recorder_tables(os.path.join(REF, "src", "topsy", "recorder", "__init__.py")))
    with open(os.path.join(OUT, "recorder_kats.json"), "w") as f:
        json.dump(data, f, indent=1)
        f.write("\n")
    print({c["test"]: len(c["checks"]) for c in data["interpolation"]}, len(data["properties"]), "properties")


if __name__ == "__main__":
    main()
