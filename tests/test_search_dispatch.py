"""The launch geometry of the search kernels, pinned: which shape reaches which bracket.  `qg_search_plan_query` (include/qgym.h) answers
from the functions the launchers of kernels_mcts.hip and kernels_search.hip themselves call (qiskit_gym_amd/csrc/qgym_plan.hpp) and needs no
GPU.  No result depends on the geometry, so a threshold edited there would leave every GPU test green while its cases slid into a bracket
that is covered already; here it turns a CPU test red.  Every shape that tests/test_gpu_mcts_geometry.py, tests/test_gpu_mcts_reuse.py,
tests/test_gpu_beam.py and tests/test_gpu_beammerge.py run for the sake of a bracket is named below with the bracket it is there for."""
import pytest

from qiskit_gym_amd import _lib

MCTS_TREES, REBASE_SLICES, REBASE_ROWS, BEAM_SELECT_WAVES, BEAM_MERGE_WAVES = range(5)


def ask(op, a, b=0, c=0):
    return _lib.load().qg_search_plan_query(op, a, b, c)


# cap -> trees (waves) per workgroup of mcts_select and mcts_rebase: min(4, 65536 / (8 cap))
TREES = [(2, 4), (130, 4), (300, 4), (2048, 4), (2049, 3), (2730, 3), (2731, 2), (4096, 2), (4097, 1), (8192, 1)]
# the (cap, M) of tests/test_gpu_mcts_geometry.py: the last workgroup of every launch is partly filled
GEOMETRY_LAUNCHES = [(2048, 5, 4), (2049, 7, 3), (2730, 7, 3), (2731, 5, 2), (4096, 5, 2), (4097, 3, 1), (8192, 3, 1)]
# num_actions -> K slices of 64 actions and 16 / K rows per trip of mcts_rebase_kernel<K>
SLICES = [(1, 1, 16), (5, 1, 16), (64, 1, 16), (65, 2, 8), (71, 2, 8), (128, 2, 8), (129, 3, 5), (137, 3, 5), (170, 3, 5), (192, 3, 5), (193, 4, 4),
          (256, 4, 4)]
# (W, A) -> waves of beam_select: 1, 2, 4, 8 for n = W A <= 1024, <= 2048, <= 6144, above
SELECT = [(16, 64, 1), (25, 41, 2), (16, 100, 2), (64, 32, 2), (10, 205, 4), (32, 192, 4), (29, 212, 8), (64, 224, 8),
          # ... and the cases tests/test_gpu_beam.py had before
          (1, 3, 1), (1, 170, 1), (2, 3, 1), (2, 222, 1), (16, 3, 1), (16, 170, 4), (16, 222, 4), (64, 3, 1), (64, 170, 8), (64, 222, 8)]
# (W, words_per_env, seen_cap) -> waves of beam_merge: 1 where W n <= 512 and seen_cap <= 512, else 4
MERGE = [(8, 64, 24, 1), (9, 57, 27, 4), (8, 6, 512, 1), (8, 6, 513, 4), (8, 64, 512, 1), (8, 64, 513, 4), (8, 6, 0, 1), (9, 57, 0, 4),
         # ... and the cases tests/test_gpu_beammerge.py had before
         (1, 1, 3, 1), (8, 6, 24, 1), (16, 9, 48, 1), (33, 32, 99, 4), (64, 64, 192, 4), (64, 256, 192, 4), (8, 6, 3, 1)]


@pytest.mark.parametrize("cap,trees", TREES)
def test_trees_per_workgroup(cap, trees):
    assert ask(MCTS_TREES, cap) == trees
    assert trees * cap * 8 <= 65536 and (trees == 4 or (trees + 1) * cap * 8 > 65536)  # as many as fit, four at the most


def test_every_break_of_the_trees_per_workgroup_has_both_sides():
    got = [ask(MCTS_TREES, cap) for cap in range(2, 8193)]
    breaks = [cap for cap, (a, b) in zip(range(3, 8193), zip(got, got[1:])) if a != b]
    assert breaks == [2049, 2731, 4097] and got[0] == 4 and got[-1] == 1 and sorted(set(got)) == [1, 2, 3, 4]
    caps = {cap for cap, _ in TREES}
    assert all(b in caps and b - 1 in caps for b in breaks)


@pytest.mark.parametrize("cap,M,trees", GEOMETRY_LAUNCHES)
def test_the_geometry_launches_end_on_a_partly_filled_workgroup(cap, M, trees):
    assert ask(MCTS_TREES, cap) == trees
    assert M > trees  # more than one workgroup: the tree index is blockIdx.x * trees + wave ...
    assert M % trees != 0 or trees == 1  # ... and waves past the last tree (a workgroup of one wave has none)


@pytest.mark.parametrize("A,K,rows", SLICES)
def test_rebase_slices_and_rows(A, K, rows):
    assert ask(REBASE_SLICES, A) == K and ask(REBASE_ROWS, A) == rows == 16 // K


def test_every_break_of_the_rebase_slices_has_both_sides():
    got = [ask(REBASE_SLICES, A) for A in range(1, 257)]
    breaks = [A for A, (a, b) in zip(range(2, 257), zip(got, got[1:])) if a != b]
    assert breaks == [65, 129, 193]
    actions = {A for A, _, _ in SLICES}
    assert all(b in actions and b - 1 in actions for b in breaks)


@pytest.mark.parametrize("W,A,waves", SELECT)
def test_beam_select_waves(W, A, waves):
    assert ask(BEAM_SELECT_WAVES, W, A) == waves


def test_every_break_of_the_beam_select_waves_has_both_sides():
    def reachable(n):  # as a product of a width <= 64 and at most 256 actions, the most a tree search takes
        return any(n % W == 0 and n // W <= 256 for W in range(1, 65))

    by_n = {W * A: waves for W, A, waves in SELECT}
    for below, above, lo, hi in ((1024, 1025, 1, 2), (2048, 2050, 2, 4), (6144, 6148, 4, 8)):
        assert by_n[below] == lo and by_n[above] == hi
        assert not any(reachable(n) for n in range(below + 1, above))  # the smallest product above the break
    assert by_n[14336] == 8 and ask(BEAM_SELECT_WAVES, 64, 225) == -3  # the maximum


@pytest.mark.parametrize("W,n,cap,waves", MERGE)
def test_beam_merge_waves(W, n, cap, waves):
    assert ask(BEAM_MERGE_WAVES, W, n, cap) == waves


def test_beyond_the_limits_and_unknown_questions():
    assert ask(MCTS_TREES, 8193) == -3 and ask(MCTS_TREES, 1) == -1 and ask(MCTS_TREES, 0) == -1
    assert ask(REBASE_SLICES, 257) == -3 and ask(REBASE_ROWS, 257) == -3 and ask(REBASE_SLICES, 0) == -1
    assert ask(BEAM_SELECT_WAVES, 65, 3) == -3 and ask(BEAM_SELECT_WAVES, 0, 3) == -1 and ask(BEAM_SELECT_WAVES, 3, 0) == -1
    assert ask(BEAM_MERGE_WAVES, 65, 3) == -3 and ask(BEAM_MERGE_WAVES, 0, 3) == -1 and ask(BEAM_MERGE_WAVES, 3, 0) == -1
    assert ask(5, 1) == -1 and ask(-1, 1) == -1
    assert b"unknown search plan op" in _lib.load().qg_last_error()
