"""The sampling specification against its own statistics (collect_ref.py, CPU only): the thresholds the GPU tests hold the kernels to
are attainable by the numpy restatement itself, and every committed logit case leaves at most 1 % of its envs under the key margin."""
import warnings

import numpy as np
import pytest

from collect_ref import categorical_ref, chi2_quantile, log_softmax, race_keys, race_winner, sample_uniforms
from sampling_cases import JOINT_ROW, PEAKED_ROW, SHAPE_A, SHAPE_B, cases, entry_kind, expected_winner, shape_case


def draw(row, seed, batch, counter, env_base=0):
    u = sample_uniforms(seed, batch, counter, row.size, env_base)
    return race_keys(np.broadcast_to(row, (batch, row.size)), u).argmin(axis=1)


def test_chi2_quantile_is_the_1e5_tail():
    assert 82.0 < chi2_quantile(35) < 84.5  # about 83
    assert 29.0 < chi2_quantile(5) < 32.0


def test_categorical_ref_conventions():
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # no NaN is formed on the way
        x = np.array([[0.0, -np.inf, 1.0], [-np.inf, -np.inf, -np.inf], [-np.inf, 2.0, -np.inf], [1e4, 1e4 - 1.0, -1e4]])
        lsm, ent = categorical_ref(x)
        masked, ment = categorical_ref(np.array([[0.0, 5.0, 1.0]]), np.array([[1, 0, 1]]))
        none = log_softmax(np.zeros((1, 3)), np.zeros((1, 3)))
    p = np.exp([0.0, 1.0]) / np.exp([0.0, 1.0]).sum()
    np.testing.assert_allclose(lsm[0, [0, 2]], np.log(p), rtol=1e-14)
    assert lsm[0, 1] == -np.inf and np.isclose(ent[0], -(p * np.log(p)).sum(), rtol=1e-14)
    assert (lsm[1] == 0).all() and ent[1] == 0  # no live action: (0, 0)
    assert lsm[2, 1] == 0.0 and ent[2] == 0.0  # one live action: exactly (0, 0)
    np.testing.assert_array_equal(masked, lsm[:1])  # a mask and -inf are the same thing
    assert ment[0] == ent[0] and (none == 0).all()
    q = 1.0 / (1.0 + np.exp(-1.0))
    assert np.isclose(lsm[3, 0], np.log(q), rtol=1e-12) and lsm[3, 2] < -1.9e4  # shift invariance at 1e4
    assert np.isfinite(ent).all()


@pytest.mark.parametrize("pair", ["counters", "envs", "seeds"])
def test_reference_draws_are_jointly_independent(pair):
    """6 x 6 table of two draws from the same row, 200 000 envs, 35 dof, against the product of the marginals."""
    B = 200_000
    if pair == "counters":
        a, b = draw(JOINT_ROW, 42, B, 3), draw(JOINT_ROW, 42, B, 4)
    elif pair == "envs":
        d = draw(JOINT_ROW, 42, B + 1, 3)
        a, b = d[:-1], d[1:]
    else:
        a, b = draw(JOINT_ROW, 42, B, 3), draw(JOINT_ROW, 43, B, 3)
    p = np.exp(log_softmax(JOINT_ROW[None])[0])
    want = B * np.outer(p, p)
    got = np.bincount(a * 6 + b, minlength=36).reshape(6, 6)
    chi2 = ((got - want) ** 2 / want).sum()
    print(pair, chi2)
    assert chi2 < chi2_quantile(35), (pair, chi2)


def test_reference_peaked_row():
    """10^6 draws from a row whose tail is dead: chi-square over the cells with expectation >= 5, the dead cells stay empty."""
    B = 1_000_000
    counts = np.bincount(draw(PEAKED_ROW, 7, B, 0), minlength=7)
    want = B * np.exp(log_softmax(PEAKED_ROW[None])[0])
    big = want >= 5
    chi2 = ((counts[big] - want[big]) ** 2 / want[big]).sum()
    print(counts, want, chi2)
    assert big.sum() == 5 and chi2 < chi2_quantile(int(big.sum()) - 1), (chi2, counts)
    assert (counts[~big] == 0).all()
    np.testing.assert_array_equal(counts, [980921, 18068, 905, 96, 10, 0, 0])


def test_reference_has_no_ties_in_the_smallest_u():
    """100 000 rows x 222 actions: the smallest u of a row is unique (23-bit u: a tie of the extreme pair is a 2.6e-5 event per row)."""
    u = sample_uniforms(1, 100_000, 0, 222)
    srt = np.partition(u, 1, axis=1)
    assert (srt[:, 0] < srt[:, 1]).all()


ENTRIES = ("sample_f32", "sample_bf16", "sample_f16", "head", "mid_small", "mid_big")


@pytest.mark.parametrize("entry", ENTRIES)
def test_committed_cases_leave_at_most_one_percent_under_the_margin(entry):
    """What test_gpu_sampling_edges.py excludes from the winner comparison, counted on the reference alone: keys closer than 1e-4
    (1e-3 through head_sample) on at most 1 % of a case's envs, none at all in the small shape batches; the tie cases exclude nothing
    but adjacent-float u."""
    for case in cases():
        if entry_kind(entry) in case.kinds:
            unclear = expected_winner(case, entry)[1]
            assert unclear.mean() <= 0.01, (case.name, entry, unclear.mean())
    for A in SHAPE_A + ((1000, 4097) if entry.startswith("sample") else ()):
        assert expected_winner(shape_case(A, 4097), entry)[1].mean() <= 0.01, (A, entry)
        for B in SHAPE_B:
            if A <= 222 or B == 41:
                unclear = expected_winner(shape_case(A, B), entry)[1]  # mid_big runs B + 8 192 envs
                assert unclear.mean() <= 0.01 if entry == "mid_big" else not unclear.any(), (A, B, entry)
