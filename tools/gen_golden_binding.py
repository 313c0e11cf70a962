#!/usr/bin/env python3
"""TEST INFRASTRUCTURE (fixture generator; needs a checkout of the reference, whose path is the one argument).
Writes tests/golden/reference_binding.json: the binding surface of the reference's L1 Python wrappers, as data — which attribute
names of `cuda_corr`, `cuda_ba` and `lietorch_backends` each wrapper file reads (devo/altcorr/correlation.py, devo/fastba/ba.py,
devo/lietorch/group_ops.py), the module-level aliases fastba/ba.py binds at import, the (forward_op, backward_op) pair of every
GroupOp subclass and the group_id of every group class (devo/lietorch/groups.py).  Only names are extracted (Python's ast); no
source text is kept.  tests/test_reference_binding.py checks the installed modules against it.

    python tools/gen_golden_binding.py <reference checkout>
"""
import ast
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BACKENDS = ("cuda_corr", "cuda_ba", "lietorch_backends")
WRAPPERS = ("devo/altcorr/correlation.py", "devo/fastba/ba.py", "devo/lietorch/group_ops.py")


def backend_attr(node):
    """'module.name' for an expression `module.name` with module one of BACKENDS, else None."""
    if isinstance(node, ast.Attribute) and isinstance(node.value, ast.Name) and node.value.id in BACKENDS:
        return f"{node.value.id}.{node.attr}"
    return None


def main(ref):
    out = {"source": "tum-vision/DEVO: " + ", ".join(WRAPPERS) + ", devo/lietorch/groups.py",
           "reads": {}, "aliases": {}, "group_ops": {}, "group_ids": {}}
    for rel in WRAPPERS:
        with open(os.path.join(ref, rel)) as f:
            tree = ast.parse(f.read())
        reads = sorted({a for node in ast.walk(tree) for a in [backend_attr(node)] if a})
        out["reads"][rel] = reads
        for node in tree.body:                                       # module-level `name = backend.attr` (bound at import)
            if isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name) and backend_attr(node.value):
                out["aliases"].setdefault(rel, {})[node.targets[0].id] = backend_attr(node.value)
        for cls in (n for n in tree.body if isinstance(n, ast.ClassDef)):
            for node in cls.body:                                    # `forward_op, backward_op = lietorch_backends.x, lietorch_backends.y | None`
                if (isinstance(node, ast.Assign) and isinstance(node.targets[0], ast.Tuple) and isinstance(node.value, ast.Tuple)
                        and [t.id for t in node.targets[0].elts if isinstance(t, ast.Name)] == ["forward_op", "backward_op"]):
                    fwd, bwd = (backend_attr(v) for v in node.value.elts)
                    out["group_ops"][cls.name] = [fwd.split(".", 1)[1], bwd.split(".", 1)[1] if bwd else None]
    with open(os.path.join(ref, "devo/lietorch/groups.py")) as f:
        tree = ast.parse(f.read())
    for cls in (n for n in tree.body if isinstance(n, ast.ClassDef)):
        for node in cls.body:
            if (isinstance(node, ast.Assign) and isinstance(node.targets[0], ast.Name) and node.targets[0].id == "group_id"
                    and isinstance(node.value, ast.Constant)):
                out["group_ids"][cls.name] = node.value.value
    dst = os.path.join(ROOT, "tests", "golden", "reference_binding.json")
    with open(dst, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", dst)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
