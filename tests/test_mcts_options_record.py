"""The record `BatchedSynthesis._check_mcts` resolves a tree search into: the handle kind and the batch shapes of every combination of
deterministic / sampled x plain / `reuse_tree` x one / several leaves, for `solve` and under `self_play`'s prefix, against the table written
out below.  No handle is built, so none of this needs a GPU; the stand-in gym is that of tests/test_mcts_many_options.py."""
import pytest

torch = pytest.importorskip("torch")

from test_mcts_many_options import synthesis  # noqa: E402

N, TREES = 6, 3  # one target, three trees

# (sampled, reuse, K, prefix, mcts_nodes) -> (kind, batches); K = 1: the leaf batch has one env per tree; the default capacity is 2 N + 1 = 13
TABLE = {
    (False, False, 1, None, None): ("mcts", (3, 21, 3)),
    (True, False, 1, None, None): ("mcts-sampled", (3, 21, 3)),
    (False, True, 1, None, None): ("mcts-reuse", (3, 39, 39, 3)),
    (False, True, 1, None, 7): ("mcts-reuse", (3, 21, 21, 3)),
    (True, True, 1, None, None): ("mcts-sampled-reuse", (3, 39, 39, 3)),
    (True, True, 1, None, 7): ("mcts-sampled-reuse", (3, 21, 21, 3)),
    (False, False, 4, None, None): ("mcts-many", (12, 21, 3)),
    (True, False, 4, None, None): ("mcts-sampled-many", (12, 21, 3)),
    (False, True, 4, None, None): ("mcts-reuse-many", (12, 39, 39, 3)),
    (False, True, 4, None, 7): ("mcts-reuse-many", (12, 21, 21, 3)),
    (True, True, 4, None, None): ("mcts-sampled-reuse-many", (12, 39, 39, 3)),
    (True, True, 4, None, 7): ("mcts-sampled-reuse-many", (12, 21, 21, 3)),
    (False, False, 1, "self-play", None): ("self-play", (3, 21, 3)),
    (True, False, 1, "self-play", None): ("self-play", (3, 21, 3)),
    (False, True, 1, "self-play", None): ("self-play-reuse", (3, 39, 39, 3)),
    (False, True, 1, "self-play", 7): ("self-play-reuse", (3, 21, 21, 3)),
    (True, True, 1, "self-play", None): ("self-play-reuse", (3, 39, 39, 3)),
    (True, True, 1, "self-play", 7): ("self-play-reuse", (3, 21, 21, 3)),
    (False, False, 4, "self-play", None): ("self-play-many", (12, 21, 3)),
    (True, False, 4, "self-play", None): ("self-play-many", (12, 21, 3)),
    (False, True, 4, "self-play", None): ("self-play-reuse-many", (12, 39, 39, 3)),
    (False, True, 4, "self-play", 7): ("self-play-reuse-many", (12, 21, 21, 3)),
    (True, True, 4, "self-play", None): ("self-play-reuse-many", (12, 39, 39, 3)),
    (True, True, 4, "self-play", 7): ("self-play-reuse-many", (12, 21, 21, 3)),
}


def test_the_table_has_all_sixteen_combinations():
    assert {k[:4] for k in TABLE} == {(s, r, K, p) for s in (False, True) for r in (False, True) for K in (1, 4) for p in (None, "self-play")}
    assert all((k[:4] + (7,) in TABLE) == k[1] for k in TABLE)  # mcts_nodes goes with reuse_tree, and every reuse row has both


@pytest.mark.parametrize("case", TABLE, ids=["-".join(str(x) for x in k) for k in TABLE])
def test_kind_and_batches(case):
    sampled, reuse, K, prefix, nodes = case
    syn, _ = synthesis()
    opts = syn._check_mcts(TREES, N, 2 ** 0.5, deterministic=not sampled, searches=TREES if sampled else None, reuse_tree=reuse, mcts_nodes=nodes,
                           mcts_leaves=K, virtual_loss=0.5 if K > 1 else 0.0)
    assert (opts.N, opts.C, opts.S, opts.K, opts.virtual_loss) == (N, 2 ** 0.5, TREES if sampled else None, K, 0.5 if K > 1 else 0.0)
    assert opts.cap == ((nodes or 13) if reuse else None)
    assert (opts.kind(prefix), opts.batches(TREES)) == TABLE[case]
    with pytest.raises(Exception):  # frozen
        opts.N = 7
    assert not syn._held  # no handle was built


def test_no_simulations_is_no_tree_search():
    syn, _ = synthesis()
    assert syn._check_mcts(TREES, 0, 2 ** 0.5) is None and syn._check_mcts(TREES, 0, -1.0, max_expand_depth=3, deterministic=True) is None
    assert syn._check_mcts(0, N, 2 ** 0.5, deterministic=True).batches(0) == (0, 0, 0)
    assert not syn._held


@pytest.mark.parametrize("K", (1, 4))
def test_a_search_is_freed_when_its_last_reference_goes(K):
    """The search object owns the forest and the per-decision buffers, and the pair of kernels it chose is kept on it: nothing kept there may
    refer back to it, or all of that lives until the cyclic collector comes by.  Built on stand-in handles (the setup reads their sizes only)."""
    import gc
    import weakref
    from types import SimpleNamespace

    from qiskit_gym_amd.synthesis import _MctsOptions, _TreeSearch

    def vec(batch):
        return SimpleNamespace(batch=batch, device=torch.device("cpu"), num_actions=lambda: 5, _cfg=SimpleNamespace(max_depth=6))

    for cap in (None, 13):
        opts = _MctsOptions(N, 2 ** 0.5, None, cap, K, 0.0)
        held = SimpleNamespace(vecs=tuple(vec(b) for b in opts.batches(TREES)))
        gc.collect()
        gc.disable()
        try:
            search = _TreeSearch(opts, held, seed=1)
            alive = [weakref.ref(search), weakref.ref(search.forest)]
            del search
            assert [r() for r in alive] == [None, None]
        finally:
            gc.enable()
