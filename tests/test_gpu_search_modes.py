"""`BatchedSynthesis.solve` mode after mode on one instance: what an instance carries from one call to the next -- the handles of each
kind, the first layers packed through them, the snapshot of the packed weights, the view list -- changes no result.  Every call returns
the solutions and `last_stats` of a fresh instance, on the same policy object and seed, that makes this one call.  One sequence per
first-layer route: the resident state (TILE layout), the views' words at an odd row count (pad word, byte-word observation), and the
packed observation words (PauliGym).  And the one path of a beam search's bookkeeping: `beam_advance` once per step, with or without a bound."""
import pytest

from test_gpu_beam import pauli_case
from test_gpu_synthesis import make, targets

pytestmark = pytest.mark.gpu


def each_call_as_on_a_fresh_instance(syn, tg, calls):
    from qiskit_gym_amd.synthesis import BatchedSynthesis

    for kw in calls:
        sols = syn.solve(tg, **kw)
        stats = dict(syn.last_stats)
        fresh = BatchedSynthesis(syn.env, syn._policy, seed=syn.seed)
        assert fresh.solve(tg, **kw) == sols, kw
        assert fresh.last_stats == stats, kw
        assert len(sols) == len(tg) and stats["targets"] == len(tg)


def one_beam_advance_per_step(monkeypatch, syn, tg, calls):
    """A beam search without a bound does its step's bookkeeping where the bounded ones do: with `synthesis.beam_advance` behind a counting
    stand-in, every call goes through it once per step, in mode None, and returns what it returns without the stand-in."""
    import inspect

    from qiskit_gym_amd import synthesis

    real = synthesis.beam_advance
    for kw in calls:
        plain = syn.solve(tg, **kw)
        modes = []

        def counting(*a, **k):
            call = inspect.signature(real).bind(*a, **k)
            call.apply_defaults()
            modes.append(call.arguments["mode"])
            return real(*a, **k)

        with monkeypatch.context() as m:
            m.setattr(synthesis, "beam_advance", counting)
            assert syn.solve(tg, **kw) == plain, kw
        assert syn.last_stats["steps"] > 0 and modes == [None] * syn.last_stats["steps"], (kw, modes)
        assert "bound" not in syn.last_stats and "bounded" not in syn.last_stats


def test_every_beam_search_advances_through_the_kernel(monkeypatch):
    """Widths 1 and 64, alone, under two views and with the merge; PauliGym (no twists, no merge) alone."""
    from qiskit_gym_amd.synthesis import BatchedSynthesis

    kind, cfg, gateset, syn = make("clifford_3q_custom")
    one_beam_advance_per_step(monkeypatch, syn, targets(kind, cfg, gateset, 5, 24, 2),
                              [dict(beam_width=W, **kw) for W in (1, 64) for kw in ({}, dict(twists=2), dict(merge_duplicates=True))])
    gym, policy, states, _ = pauli_case()
    one_beam_advance_per_step(monkeypatch, BatchedSynthesis(gym, policy, seed=1), states, [dict(beam_width=W) for W in (1, 64)])


def test_state_route_nine_modes_in_a_row():
    kind, cfg, gateset, syn = make("clifford_3q_custom")
    tg = targets(kind, cfg, gateset, 16, 24, 2)
    each_call_as_on_a_fresh_instance(syn, tg, [
        dict(num_searches=4),
        dict(deterministic=True),
        dict(deterministic=True, fast=True),
        dict(beam_width=2),
        dict(beam_width=2, fast=True),
        dict(beam_width=2, merge_duplicates=True, fast=True),
        dict(deterministic=True, twists=2),
        dict(deterministic=True, twists=2, twist_kernels=True),
        dict(num_searches=4, fast=True),
    ])
    assert syn.last_stats["kernels"] is True and syn.last_stats["solved"] > 0


def test_view_words_route_at_five_rows():
    kind, cfg, gateset, syn = make("lf_5_line")
    tg = targets(kind, cfg, gateset, 16, 20, 31)
    each_call_as_on_a_fresh_instance(syn, tg, [dict(twists=2, twist_kernels=True, **kw) for kw in
                                               (dict(deterministic=True), dict(beam_width=2), dict(num_searches=4))])
    assert syn.last_stats["kernels"] is True and syn.last_stats["views"] == 2 and syn.last_stats["solved"] > 0


def test_words_route_on_pauli():
    from qiskit_gym_amd.synthesis import BatchedSynthesis

    gym, policy, states, _ = pauli_case()
    syn = BatchedSynthesis(gym, policy, seed=1)
    each_call_as_on_a_fresh_instance(syn, states, [dict(num_searches=4, fast=True), dict(beam_width=2, fast=True)])
    assert syn.last_stats["kernels"] is True and syn._beam.first[syn._beam.vecs[0]].route == "words"
