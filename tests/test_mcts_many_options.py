"""The ValueErrors of `solve(..., mcts_leaves=K, virtual_loss=v)` and `synth`: each is raised before any handle is built, so none of this
needs a GPU -- a gym object does (it creates an env), so a stand-in with the two things the checks read takes its place.  The searches
themselves are in tests/test_gpu_mcts_many_search.py."""
from types import SimpleNamespace

import pytest

torch = pytest.importorskip("torch")

from util import line_gateset  # noqa: E402


def synthesis():
    from qiskit_gym_amd.synthesis import BatchedSynthesis

    gs = line_gateset("clifford", 3)
    gym = SimpleNamespace(env_kind="clifford", config={"gateset": gs, "num_qubits": 3, "max_depth": 6})
    return BatchedSynthesis(gym, torch.nn.Linear(36, len(gs))), [[0] * 36]


DET = dict(deterministic=True, num_mcts_searches=8)
SMP = dict(mcts_sampled=True, num_searches=2, num_mcts_searches=8)
BAD = [
    (dict(DET, mcts_leaves=0), "mcts_leaves"),
    (dict(DET, mcts_leaves=-3), "mcts_leaves"),
    (dict(DET, mcts_leaves=65), "mcts_leaves"),
    (dict(SMP, mcts_leaves=65, num_mcts_searches=100), "mcts_leaves"),
    (dict(deterministic=True, mcts_leaves=2), "num_mcts_searches"),  # no tree search to batch
    (dict(mcts_leaves=4), "num_mcts_searches"),
    (dict(deterministic=True, num_mcts_searches=0, mcts_leaves=2), "num_mcts_searches"),
    (dict(DET, mcts_leaves=9), "num_mcts_searches"),  # more leaves than simulations
    (dict(SMP, mcts_leaves=64), "num_mcts_searches"),
    (dict(DET, reuse_tree=True, mcts_leaves=9), "num_mcts_searches"),
    (dict(DET, mcts_leaves=4, virtual_loss=-0.5), "virtual_loss"),
    (dict(DET, mcts_leaves=4, virtual_loss=float("inf")), "virtual_loss"),
    (dict(DET, mcts_leaves=4, virtual_loss=float("nan")), "virtual_loss"),
    (dict(DET, virtual_loss=0.5), "virtual_loss"),  # one leaf per round leaves no virtual visits
    (dict(DET, mcts_leaves=1, virtual_loss=1.0), "virtual_loss"),
    (dict(deterministic=True, virtual_loss=0.5), "virtual_loss"),
    (dict(virtual_loss=-1.0), "virtual_loss"),
    # ... and what the tree search refuses, it refuses in rounds as well
    (dict(DET, mcts_leaves=4, beam_width=2), "beam_width"),
    (dict(DET, mcts_leaves=4, twists=2), "twists"),
    (dict(DET, mcts_leaves=4, max_expand_depth=2), "max_expand_depth"),
    (dict(DET, mcts_leaves=4, deterministic=False), "deterministic"),
    (dict(SMP, mcts_leaves=4, deterministic=True), "deterministic"),
    (dict(DET, mcts_leaves=4, mcts_nodes=20), "mcts_nodes"),
    (dict(DET, mcts_leaves=4, reuse_tree=True, mcts_nodes=8), "mcts_nodes"),
    (dict(DET, mcts_leaves=4, C=0.0), "C"),
]


@pytest.mark.parametrize("kw,word", BAD, ids=[",".join(f"{k}={v}" for k, v in kw.items()) for kw, _ in BAD])
def test_value_errors(kw, word):
    syn, states = synthesis()
    with pytest.raises(ValueError, match=word):
        syn.solve(states, **kw)
    with pytest.raises(ValueError, match=word):
        syn.solve([], **kw)  # checked without a target too
    assert not syn._held  # refused before any handle was built


def test_synth_passes_the_keywords_on():
    import inspect

    from qiskit_gym_amd.synthesis import BatchedSynthesis

    for fn in (BatchedSynthesis.solve, BatchedSynthesis.synth):
        p = inspect.signature(fn).parameters
        assert p["mcts_leaves"].default == 1 and p["virtual_loss"].default == 0.0
    syn, _ = synthesis()
    with pytest.raises(ValueError, match="mcts_leaves"):
        syn.synth([], deterministic=True, num_mcts_searches=8, mcts_leaves=65)
    with pytest.raises(ValueError, match="virtual_loss"):
        syn.synth([], deterministic=True, num_mcts_searches=8, virtual_loss=0.5)


def test_the_defaults_are_no_tree_search_and_no_error():
    syn, _ = synthesis()
    assert syn.solve([], mcts_leaves=1, virtual_loss=0.0) == [] and syn.solve([], deterministic=True, num_mcts_searches=8, mcts_leaves=8, virtual_loss=1.0) == []
