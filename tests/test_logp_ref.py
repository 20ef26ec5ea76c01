"""logp_ref.py on hand-made rows: the reference of test_gpu_head_logp.py has to be right on its own (CPU)."""
import numpy as np

from logp_ref import HEAD_MASKED, logp_ref, logsumexp_rows


def test_tied_maximum_takes_the_lowest_index():
    row = np.full(10, -1.0)
    row[[3, 7]] = 2.5
    rows, act, best, ent = logp_ref(row[None])
    assert act[0] == 3
    assert rows[0, 3] == rows[0, 7] == best[0]
    np.testing.assert_allclose(np.exp(rows[0]).sum(), 1.0, rtol=1e-14)


def test_uniform_row():
    rows, act, best, ent = logp_ref(np.zeros((2, 8)))
    np.testing.assert_allclose(rows, -np.log(8.0), rtol=1e-15)
    assert (act == 0).all()
    np.testing.assert_allclose(ent, np.log(8.0), rtol=1e-14)


def test_one_live_action():
    for masked in (-np.inf, -1.0e30, float(np.finfo(np.float32).min)):
        row = np.full(6, masked)
        row[4] = -3.0
        rows, act, best, ent = logp_ref(row[None])
        assert act[0] == 4 and best[0] == 0.0 and ent[0] == 0.0
        assert rows[0, 4] == 0.0 and np.isneginf(np.delete(rows[0], 4)).all()


def test_all_masked_row():
    L = np.array([[-np.inf] * 5, [-1.0e30, -2.0e30, -np.inf, -5.0e29, -1.0e30], [0.0, 1.0, 2.0, 3.0, 4.0]])
    rows, act, best, ent = logp_ref(L)
    assert act.tolist() == [0, 0, 4]
    assert best[0] == 0.0 and best[1] == 0.0 and ent[0] == 0.0 and ent[1] == 0.0
    assert np.isneginf(rows[:2]).all() and np.isfinite(rows[2]).all()
    assert np.isneginf(logsumexp_rows(rows)[:2]).all()


def test_an_action_90_below_the_maximum_stays_finite():
    row = np.array([0.0, -90.0, -200.0, -np.inf, -0.5])
    rows, act, best, ent = logp_ref(row[None])
    lse = np.log(1.0 + np.exp(-0.5))  # the far entries add less than 1e-39
    np.testing.assert_allclose(rows[0, [0, 1, 2, 4]], np.array([0.0, -90.0, -200.0, -0.5]) - lse, rtol=1e-14)
    assert np.isneginf(rows[0, 3]) and act[0] == 0
    assert abs(logsumexp_rows(rows)[0]) < 1e-15


def test_threshold_and_last_maximum():
    row = np.array([HEAD_MASKED * 1.0001, -5.0, HEAD_MASKED, 7.0])  # just below the threshold: masked; at it: live
    rows, act, best, ent = logp_ref(row[None])
    assert np.isneginf(rows[0, 0]) and np.isfinite(rows[0, 2]) and act[0] == 3


def test_entropy_matches_the_definition():
    rng = np.random.default_rng(0)
    L = rng.normal(size=(5, 33)) * 3
    L[1, ::3] = -np.inf
    rows, act, best, ent = logp_ref(L)
    p = np.exp(rows)
    want = -(np.where(p > 0, p * np.where(np.isfinite(rows), rows, 0.0), 0.0)).sum(axis=1)
    np.testing.assert_allclose(ent, want, rtol=1e-13)
    np.testing.assert_allclose(logsumexp_rows(rows), 0.0, atol=1e-14)
    np.testing.assert_array_equal(act, np.where(np.isfinite(L), L, -np.inf).argmax(axis=1))


def test_random_weights_seed_stays_within_the_unclear_cap():
    """The random-weights case of test_gpu_head_logp.py leaves out rows whose two largest logits are closer than 5e-2: at most 20 % of them."""
    from logp_cases import RANDOM_MAX_UNCLEAR, random_reference, random_weights

    full, clear = random_reference(*random_weights())
    print("unclear rows:", 1.0 - clear.mean())
    assert 1.0 - clear.mean() <= RANDOM_MAX_UNCLEAR
