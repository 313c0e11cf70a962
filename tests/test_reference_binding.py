"""The drop-in boundary, checked against the binding surface of the reference's OWN Python wrappers.  After devo_amd.backends.install()
the reference's L1 modules — which bind attribute names of `cuda_corr`, `cuda_ba` and `lietorch_backends` at import time
(devo/altcorr/correlation.py:2,11,28,40,47; devo/fastba/ba.py:2-8; devo/lietorch/group_ops.py:1,28-66) — must find every name they read,
every GroupOp must resolve its backend functions, and a CPU call made the way the wrappers make it must raise the no-fallback error
instead of computing anything.  The names come from tests/golden/reference_binding.json (tools/gen_golden_binding.py extracts them
from a reference checkout), so the test needs nothing outside the repository."""
import json
import os
import sys
import pytest
import torch

# the names the reference's GroupOp subclasses bind (group_ops.py:28-66): forward ops and the backward ops that exist
FORWARD = ["expm", "logm", "inv", "mul", "adj", "adjT", "act", "act4", "Jinv", "as_matrix"]
BACKWARD = ["expm_backward", "logm_backward", "inv_backward", "mul_backward", "adj_backward", "adjT_backward", "act_backward", "act4_backward"]
NAMES = ("cuda_corr", "cuda_ba", "lietorch_backends")


@pytest.fixture()
def reference_package(golden_dir):
    """install() under the names the reference imports (restored afterwards) + the reference's binding surface (golden)."""
    import devo_amd.backends as b
    saved = {k: sys.modules.get(k) for k in NAMES}
    for k in saved:
        sys.modules.pop(k, None)
    mods = b.install()
    with open(os.path.join(golden_dir, "reference_binding.json")) as f:
        surface = json.load(f)
    try:
        yield mods, surface
    finally:
        for k, v in saved.items():
            sys.modules.pop(k, None)
            if v is not None:
                sys.modules[k] = v


def _resolve(dotted):
    """'cuda_ba.neighbors' -> the attribute of the module the reference's `import cuda_ba` finds."""
    mod, name = dotted.split(".", 1)
    return getattr(sys.modules[mod], name)


def test_reference_wrappers_bind_to_the_installed_modules(reference_package):
    (cuda_corr, cuda_ba, lietorch_backends), surface = reference_package
    # the reference's `import cuda_corr` / `import cuda_ba` / `import lietorch_backends` find the installed modules
    assert sys.modules["cuda_corr"] is cuda_corr and sys.modules["cuda_ba"] is cuda_ba and sys.modules["lietorch_backends"] is lietorch_backends
    assert set(surface["reads"]) == {"devo/altcorr/correlation.py", "devo/fastba/ba.py", "devo/lietorch/group_ops.py"}

    # every GroupOp subclass resolves its forward / backward op to the HIP-backed module's function: 10 + 8 names (+ projector below)
    ops = surface["group_ops"]
    want = {"Exp": ("expm", "expm_backward"), "Log": ("logm", "logm_backward"), "Inv": ("inv", "inv_backward"), "Mul": ("mul", "mul_backward"),
            "Adj": ("adj", "adj_backward"), "AdjT": ("adjT", "adjT_backward"), "Act3": ("act", "act_backward"), "Act4": ("act4", "act4_backward"),
            "Jinv": ("Jinv", None), "ToMatrix": ("as_matrix", None)}
    assert set(ops) == set(want)
    assert sorted(f for f, _ in want.values()) == sorted(FORWARD) and sorted(b_ for _, b_ in want.values() if b_) == sorted(BACKWARD)
    for name, (fwd, bwd) in want.items():
        assert tuple(ops[name]) == (fwd, bwd), name
        assert callable(getattr(lietorch_backends, fwd)), name
        assert bwd is None or callable(getattr(lietorch_backends, bwd)), name
    assert callable(lietorch_backends.projector)                     # lietorch.cpp:313 (19th name; not on the hot path)

    # altcorr / fastba / lietorch: every backend attribute a wrapper reads, and the aliases fastba/ba.py binds at import
    for rel, reads in surface["reads"].items():
        assert reads, rel
        for dotted in reads:
            assert callable(_resolve(dotted)), f"{rel}: {dotted}"
    assert {"cuda_corr.forward", "cuda_corr.backward", "cuda_corr.patchify_forward", "cuda_corr.patchify_backward"} <= set(surface["reads"]["devo/altcorr/correlation.py"])
    assert {"cuda_ba.forward", "cuda_ba.neighbors", "cuda_ba.reproject"} <= set(surface["reads"]["devo/fastba/ba.py"])
    aliases = surface["aliases"]["devo/fastba/ba.py"]
    assert aliases == {"neighbors": "cuda_ba.neighbors", "reproject": "cuda_ba.reproject"}
    assert _resolve(aliases["neighbors"]) is cuda_ba.neighbors and _resolve(aliases["reproject"]) is cuda_ba.reproject


def test_a_cpu_call_through_the_reference_wrappers_raises_instead_of_falling_back(reference_package):
    (cuda_corr, cuda_ba, lietorch_backends), surface = reference_package
    # SE3.Identity(1).inv(): groups.py apply_op -> Inv.apply(group_id, data) -> lietorch_backends.inv(group_id, data)
    X = torch.tensor([[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]])
    with pytest.raises(RuntimeError, match="GPU"):
        _resolve("lietorch_backends." + surface["group_ops"]["Inv"][0])(surface["group_ids"]["SE3"], X)
    # altcorr.corr: CorrLayer.forward -> cuda_corr.forward(fmap1, fmap2, coords, ii, jj, radius)
    with pytest.raises(RuntimeError, match="GPU"):
        _resolve("cuda_corr.forward")(torch.zeros(1, 2, 8, 3, 3), torch.zeros(1, 2, 8, 4, 4), torch.zeros(1, 3, 2, 3, 3),
                                      torch.zeros(3, dtype=torch.long), torch.zeros(3, dtype=torch.long), 3)
    # fastba.neighbors: the alias of cuda_ba.neighbors bound at import
    with pytest.raises(RuntimeError, match="GPU"):
        _resolve(surface["aliases"]["devo/fastba/ba.py"]["neighbors"])(torch.zeros(4, dtype=torch.long), torch.zeros(4, dtype=torch.long))
