"""numpy restatements of the collector kernels (kernels_collect.hip), used only by the tests."""
import numpy as np

from util import rng_draw

SAMPLE_STREAM = 0x73616D70


def sample_uniforms(seed: int, batch: int, counter: int, num_actions: int, env_base: int = 0) -> np.ndarray:
    """u[e, a] exactly as qg_sample_actions builds it (f32), for envs env_base .. env_base + batch - 1."""
    env = np.arange(batch, dtype=np.uint64) + np.uint64(env_base)
    base = rng_draw((seed ^ SAMPLE_STREAM) & (2**64 - 1), env, counter)
    hi = (base >> np.uint64(32)).astype(np.uint32)[:, None]
    lo = (base & np.uint64(0xFFFFFFFF)).astype(np.uint32)[:, None]
    a = np.arange(num_actions, dtype=np.uint32)[None, :]
    with np.errstate(over="ignore"):
        x = hi + a * np.uint32(0x9E3779B9)
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x7FEB352D)
        x ^= lo
        x ^= x >> np.uint32(15)
        x *= np.uint32(0x846CA68B)
        x ^= x >> np.uint32(16)
    return ((x >> np.uint32(9)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 8388608.0)


def race_keys(logits: np.ndarray, u: np.ndarray, mask=None) -> np.ndarray:
    """log of the exponential-race times, f64: the sampled action is the argmin."""
    x = logits.astype(np.float64)
    with np.errstate(invalid="ignore"):
        m = np.where(np.isfinite(x), x, -np.inf).max(axis=1, keepdims=True)
    x = x - np.where(np.isfinite(m), m, 0.0)  # the race is shift-invariant: keep the f64 digits for the gaps, not for the offset
    keys = np.log(-np.log(u.astype(np.float64))) - x
    if mask is not None:
        keys = np.where(mask.astype(bool), keys, np.inf)
    return keys


def categorical_ref(logits: np.ndarray, mask=None):
    """(log_softmax [B, A], entropy [B]) of the categorical distribution over each row, f64.  A masked action and a -inf logit are the
    same thing (probability 0, log-prob -inf, p log p = 0).  A row without any live action gives log_softmax = 0 everywhere and
    entropy 0: with action 0 that is the `none` branch of sample_kernel (kernels_collect.hip)."""
    x = np.asarray(logits).astype(np.float64)
    if mask is not None:
        x = np.where(np.asarray(mask).astype(bool), x, -np.inf)
    some = np.isfinite(x.max(axis=1, keepdims=True))
    m = np.where(some, x.max(axis=1, keepdims=True), 0.0)
    d = np.where(some, x, 0.0) - m  # (-inf) - finite = -inf: no NaN is formed
    ex = np.exp(d)
    s = ex.sum(axis=1, keepdims=True)
    lsm = np.where(some, d - np.log(s), 0.0)
    p = ex / s
    plogp = np.where(p > 0, p * np.where(p > 0, lsm, 0.0), 0.0)
    entropy = np.where(some[:, 0], -plogp.sum(axis=1), 0.0)
    return lsm, entropy


def log_softmax(logits: np.ndarray, mask=None) -> np.ndarray:
    return categorical_ref(logits, mask)[0]


def race_winner(keys: np.ndarray):
    """(action, margin) of the race: the lowest index among the smallest keys, 0 where every key is +inf (no live action); margin =
    second smallest key - smallest, +inf where fewer than two actions are live."""
    srt = np.sort(keys, axis=1)
    live = np.isfinite(srt[:, 0])
    action = np.where(live, keys.argmin(axis=1), 0)
    if keys.shape[1] == 1:
        return action, np.full(keys.shape[0], np.inf)
    with np.errstate(invalid="ignore"):
        margin = np.where(np.isfinite(srt[:, 1]), srt[:, 1] - srt[:, 0], np.inf)
    return action, margin


def chi2_quantile(dof: int, tail: float = 1e-5) -> float:
    """The 1 - tail quantile of chi-square with `dof` degrees of freedom: scipy where it imports, else Wilson-Hilferty."""
    try:
        from scipy.stats import chi2
        return float(chi2.ppf(1.0 - tail, dof))
    except ImportError:
        from statistics import NormalDist
        z = NormalDist().inv_cdf(1.0 - tail)
        return dof * (1.0 - 2.0 / (9.0 * dof) + z * (2.0 / (9.0 * dof)) ** 0.5) ** 3


def gae_f32(rewards, values, dones, last_values, gamma, lam):
    """Same f32 operation order as gae_kernel (no FMA)."""
    T, B = rewards.shape
    f = np.float32
    g, gl = f(gamma), f(gamma) * f(lam)
    adv = np.zeros((T, B), dtype=f)
    ret = np.zeros((T, B), dtype=f)
    next_v = np.zeros(B, dtype=f) if last_values is None else last_values.astype(f)
    acc = np.zeros(B, dtype=f)
    for t in range(T - 1, -1, -1):
        nd = np.where(dones[t] != 0, f(0), f(1)).astype(f)
        v = values[t].astype(f)
        delta = (rewards[t].astype(f) + (g * next_v) * nd) - v
        acc = delta + (gl * nd) * acc
        adv[t] = acc
        ret[t] = acc + v
        next_v = v
    return adv, ret
