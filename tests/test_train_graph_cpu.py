"""The training graph without a GPU: the restatement (tests/train_graph_ref.py) against the reference-generated fixture, the host's size
model (devo_amd.train_graph.GraphSizes: a presence matrix of frame pairs) against the restatement at every iteration of six schedules,
and the refusals that come before anything touches a device."""
import os
import sys
import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_graph_ref as R                                    # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_graph.npz")

# (N, M, init, warmup, steps, drops)
SCHEDULES = [(15, 80, 8, 8, 18, ()), (15, 80, 8, 8, 18, (8, 9, 10, 12, 15)), (11, 3, 8, 8, 14, (9, 12)), (8, 3, 5, 2, 8, (2, 3, 4)), (4, 6, 2, 2, 6, (2, 3)),
             (6, 2, 3, 1, 6, (1, 2, 3))]


def test_restatement_equals_the_reference_fixture():
    z = np.load(GOLDEN)
    N, M, P, steps, drops = int(z["N"]), int(z["M"]), int(z["P"]), int(z["steps"]), tuple(int(d) for d in z["drops"])
    out, _ = R.drive(N, M, 8, 8, steps, drops, P=P, poses=torch.from_numpy(z["poses0"]), patches=torch.from_numpy(z["patches0"]))
    grew = 0
    for t, rec in enumerate(out):
        for name in ("ii", "jj", "kk", "close", "far"):
            assert np.array_equal(rec[name].numpy(), z[f"{name}{t}"]), (name, t)
        assert rec["n"] == int(z[f"n{t}"]), t
        assert np.array_equal(rec["pose"].numpy(), z[f"pose{t}"]) and np.array_equal(rec["depths"].numpy(), z[f"depths{t}"]), t
        grew += t > 0 and rec["n"] != out[t - 1]["n"]
    assert grew == 3 and out[-1]["n"] == N


@pytest.mark.parametrize("sched", SCHEDULES, ids=lambda s: "N%d-M%d-init%d-warm%d-steps%d-drops%s" % (s[:5] + ("_".join(map(str, s[5])) or "none",)))
def test_size_model_equals_the_restatement(sched):
    from devo_amd.train_graph import GraphSizes
    N, M, init, warmup, steps, drops = sched
    out, _ = R.drive(N, M, init, warmup, steps, drops, P=1)
    m = GraphSizes(N, M, init, warmup)
    for t, rec in enumerate(out):
        if m.grows(t):
            m.grow(drop=t in drops)
        assert (m.E, m.n_close, m.n_far, m.n) == (rec["ii"].numel(), rec["close"].numel(), rec["far"].numel(), rec["n"]), t
        assert m.n == int(rec["ii"].max()) + 1
        E_cap, c_cap, f_cap = m.capacities(m.n)
        assert m.E <= E_cap and m.n_close <= c_cap and m.n_far <= f_cap


def test_refusals_come_before_any_device_work():
    from devo_amd.train_graph import TrainGraph
    with pytest.raises(ValueError, match="n_frames"):
        TrainGraph(65, 2)
    with pytest.raises(ValueError, match="init_frames"):
        TrainGraph(4, 2, init_frames=5)
    with pytest.raises(ValueError, match="median"):
        TrainGraph(9, 1821, P=3)                               # 2 * 1821 * 9 = 32 778 > 32 768
    TrainGraph(9, 1820, P=3)                                   # 32 760: fits; nothing is allocated or launched by the constructor
    with pytest.raises(ValueError, match="multiple of 8"):
        TrainGraph(9, 2, dim=12)
    g = TrainGraph(4, 2, dim=8, init_frames=2, warmup=0, device="cpu")
    poses, patches = torch.zeros(1, 4, 7), torch.zeros(1, 8, 3, 3, 3)
    with pytest.raises(ValueError, match="net of shape"):
        g.step(0, torch.zeros(1, 7, 8), poses, patches)        # E = 8
    with pytest.raises(ValueError, match="net of shape"):
        g.step(0, torch.zeros(1, 8, 16), poses, patches)
    with pytest.raises(ValueError, match="fp16 or fp32"):
        g.step(0, torch.zeros(1, 8, 8, dtype=torch.float64), poses, patches)
    with pytest.raises(ValueError, match="poses of 4 rows"):
        g.step(0, torch.zeros(1, 8, 8), torch.zeros(1, 5, 7), patches)
    with pytest.raises(RuntimeError, match="GPU"):              # well-formed, but there is no CPU path
        g.step(0, torch.zeros(1, 8, 8), poses, patches)
    assert (g.n, len(g)) == (2, 8)                              # unchanged by every refusal
    net = torch.zeros(1, 8, 8)
    g2 = TrainGraph(4, 2, dim=8, init_frames=2, warmup=3, device="cpu")
    assert g2.step(0, net, poses, patches) == (net, poses, patches) and g2.step(2, net, poses, patches)[0] is net      # before the warm-up: inputs back, nothing launched


def test_schedule_argument_is_checked():
    from devo_amd.training import TrainNet
    assert TrainNet.SCHEDULES == ("full", "reference")
    import inspect
    sig = inspect.signature(TrainNet.forward)
    assert sig.parameters["schedule"].default == "full" and sig.parameters["warmup"].default == 8 and sig.parameters["init_frames"].default is None
