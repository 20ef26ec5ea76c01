"""Operands shared by test_logp_ref.py (CPU: the reference alone must meet the cap on unclear rows) and test_gpu_head_logp.py.  numpy only."""
import numpy as np

from sampling_cases import to_bf16

RANDOM_SEED, RANDOM_A, RANDOM_K1, RANDOM_F, RANDOM_B = 3, 170, 512, 256, 300
RANDOM_GAP = 5e-2       # rows whose two largest logits are closer are left out of the arg-max comparison (test_gpu_collect_ops.py)
RANDOM_MAX_UNCLEAR = 0.2


def random_weights():
    """bf16-valued operands of the random-weights case as f32 arrays: h1 [B, K1], w2 [F, K1], b2 [F], w3 [A + 1, F], b3 [A + 1]."""
    rng = np.random.default_rng(RANDOM_SEED)
    A, K1, F, B = RANDOM_A, RANDOM_K1, RANDOM_F, RANDOM_B
    h1 = to_bf16(np.maximum(rng.standard_normal((B, K1)), 0.0).astype(np.float32))
    w2 = to_bf16((rng.standard_normal((F, K1)) * (2.0 / K1) ** 0.5).astype(np.float32))
    b2 = to_bf16((rng.standard_normal(F) * 0.1).astype(np.float32))
    w3 = to_bf16((rng.standard_normal((A + 1, F)) * 2.0 * (2.0 / F) ** 0.5).astype(np.float32))
    b3 = to_bf16((rng.standard_normal(A + 1) * 0.1).astype(np.float32))
    return h1, w2, b2, w3, b3


def random_reference(h1, w2, b2, w3, b3):
    """f64 logits [B, A + 1] (column A: the value) with h2 rounded to bf16 as the kernel rounds it, and which rows are clear."""
    h2 = np.maximum(h1.astype(np.float64) @ w2.astype(np.float64).T + b2.astype(np.float64), 0.0)
    h2 = to_bf16(h2.astype(np.float32)).astype(np.float64)
    full = h2 @ w3.astype(np.float64).T + b3.astype(np.float64)
    top = np.sort(full[:, :RANDOM_A], axis=1)
    clear = (top[:, -1] - top[:, -2]) > RANDOM_GAP
    return full, clear
