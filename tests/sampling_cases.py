"""Prescribed logit matrices for the sampling kernels, shared by test_collect_ref.py (the reference alone must meet the margin cap) and
test_gpu_sampling_edges.py (the kernels against the reference).  numpy only.

A case is a few distinct rows tiled over the batch, L[e] = rows[e % J] + bias: that is what a one-hot activation through a linear head
can produce exactly, so all four entry points see the same matrix.  `kind` names the number format the entry point takes the logits in:
"f32" / "bf16" / "f16" (qg_sample_actions' dtypes) or "head" (bf16 weights times a pair of ones, plus a bias carried as two bf16 terms)."""
from dataclasses import dataclass
from typing import Optional

import numpy as np

KINDS = ("f32", "bf16", "f16", "head")
HEAD_MASKED = -1.0e29  # qgym.h: a head logit below this is a masked action


def to_bf16(x) -> np.ndarray:
    """Round f32 to bf16 (nearest even), returned as f32."""
    b = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    out = (r & 0xFFFFFFFF).astype(np.uint32).view(np.float32)
    return np.where(np.isfinite(np.asarray(x, dtype=np.float32)), out, np.asarray(x, dtype=np.float32))


def two_bf16(x):
    """(hi, lo): the two bf16 terms pack_head carries a bias as, and the weights pair a test spreads a logit over."""
    x = np.asarray(x, dtype=np.float32)
    hi = to_bf16(x)
    with np.errstate(invalid="ignore"):
        lo = to_bf16(np.where(np.isfinite(x), x - hi, 0.0).astype(np.float32))
    return hi, lo


def quantise(x, kind: str) -> np.ndarray:
    """The nearest value the entry point can be handed, f64."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore"):
        if kind == "f32":
            return x.astype(np.float32).astype(np.float64)
        if kind == "f16":
            return x.astype(np.float16).astype(np.float64)
        if kind == "bf16":
            return to_bf16(x.astype(np.float32)).astype(np.float64)
    hi, lo = two_bf16(x.astype(np.float32))
    return hi.astype(np.float64) + lo.astype(np.float64)


@dataclass
class Case:
    name: str
    rows: np.ndarray            # [J, A] f64, finite
    bias: Optional[np.ndarray]  # [A] f64 (-inf = masked by value) or None
    batch: int
    seed: int
    counter: int
    large_d: bool = False       # |logit - max| is large: log-prob / entropy tolerances take the relative term
    ties: bool = False          # the live logits of a row are equal or flushed: the winner is the largest u, no margin exclusion
    kinds: tuple = KINDS

    @property
    def num_actions(self) -> int:
        return self.rows.shape[1]


def case_parts(case: Case, kind: str):
    """(rows, bias) as the entry point is handed them (f64; bias None for the dtype kinds, where it is folded into the rows)."""
    if kind != "head":
        full = case.rows + (case.bias if case.bias is not None else 0.0)
        return quantise(full, kind), None
    rows = quantise(case.rows, "head")
    if case.bias is None:
        return rows, None
    bias = np.where(np.isfinite(case.bias), quantise(np.where(np.isfinite(case.bias), case.bias, 0.0), "head"), case.bias)
    # rows + bias must not depend on the order the MFMA adds its four terms in: multiples of 1/64 below 2^17 are exact in f32
    fin = np.isfinite(bias) & (bias != 0) & (bias > HEAD_MASKED)
    if fin.any():
        terms = np.concatenate([rows[:, fin].ravel(), bias[fin]])
        assert np.all(terms * 64 == np.round(terms * 64)) and np.abs(rows[:, fin]).max() + np.abs(bias[fin]).max() < 2.0**17, case.name
    return rows, bias


def case_logits(case: Case, kind: str, batch: Optional[int] = None) -> np.ndarray:
    """L[batch, A] f64 as the kernel sees it; a head logit at or below HEAD_MASKED is -inf."""
    rows, bias = case_parts(case, kind)
    full = rows if bias is None else rows + bias
    if kind == "head":
        full = np.where(full < HEAD_MASKED, -np.inf, full)
    return full[np.arange(case.batch if batch is None else batch) % full.shape[0]]


SMALL_KERNEL_MAX = 8192


def entry_kind(entry: str) -> str:
    """The logit format of an entry point: sample_f32 / sample_bf16 / sample_f16 / head / mid_small / mid_big."""
    return entry[7:] if entry.startswith("sample_") else "head"


def entry_batch(entry: str, case: Case) -> int:
    """mid_head_sample_kernel is reached beyond 8 192 envs only."""
    return case.batch + SMALL_KERNEL_MAX if entry == "mid_big" else case.batch


def entry_threshold(entry: str) -> float:
    """Key margins below which f32 against f64 may reorder a race (test_gpu_collect_ops.py)."""
    return 1e-3 if entry == "head" else 1e-4


def expected_winner(case: Case, entry: str, batch: Optional[int] = None):
    """(action [B], unclear [B]) by the f64 reference.  Ordinary cases: the race winner, unclear where the two best keys are closer than
    the entry's threshold.  Tie cases: the live logits of a row are equal, so the winner is the largest u among them (lowest index where
    u ties as well), unclear only where the two largest are adjacent floats."""
    from collect_ref import race_keys, race_winner, sample_uniforms

    kind = entry_kind(entry) if entry not in KINDS else entry
    B = (entry_batch(entry, case) if entry not in KINDS else case.batch) if batch is None else batch
    L = case_logits(case, kind, B)
    u = sample_uniforms(case.seed, B, case.counter, case.num_actions)
    if not case.ties:
        want, margin = race_winner(race_keys(L, u))
        return want, margin <= entry_threshold(entry)
    live = np.where(L > L.max(axis=1, keepdims=True) - 100.0, u, np.float32(0)).astype(np.float32)
    top = np.sort(live, axis=1)[:, -2:] if L.shape[1] > 1 else np.stack([np.zeros(B, np.float32), live[:, 0]], axis=1)
    unclear = (top[:, 0] > 0) & (top[:, 0] != top[:, 1]) & (np.nextafter(top[:, 0], np.float32(2)) >= top[:, 1])
    return live.argmax(axis=1), unclear


def _rest(rng, n, lo, hi):
    """n random multiples of 1/8 in [lo, hi]."""
    return rng.integers(int(lo * 8), int(hi * 8) + 1, size=n) / 8.0


GAPS = (20.0, 80.0, 87.3, 88.0, 104.0, 150.0, 1.0e3, 1.0e4)


def peaked_rows(A: int, rng, grid: float = 0.0) -> np.ndarray:
    """Two rows per gap: the runner-up at the gap below the winner, and the runner-up tied with the winner; everything else at or below
    the gap.  grid > 0 rounds the gaps to multiples of it."""
    rows = []
    for g in GAPS:
        g = round(g / grid) * grid if grid else g
        for tied in (False, True):
            r = -g - _rest(rng, A, 0, 8)
            w, s = rng.choice(A, size=2, replace=False)
            r[w] = 0.0
            r[s] = 0.0 if tied else -g
            rows.append(r)
    return np.array(rows)


def cases():
    rng = np.random.default_rng(20240)
    out = []
    A = 37
    out.append(Case("peaked", peaked_rows(A, rng), None, 4097, 21, 2, large_d=True))
    for sign in (1.0, -1.0):
        out.append(Case(f"peaked_shift_{'up' if sign > 0 else 'down'}", peaked_rows(A, rng, 1 / 64), np.full(A, sign * 1.0e4), 4097, 22, 5, large_d=True))
    # dtype extremes (qg_sample_actions): the largest finite value of the format against its negative and against 0
    for kind, big in (("f16", 65504.0), ("bf16", float(np.float32(3.3895313892515355e38))), ("f32", float(np.finfo(np.float32).max))):
        r = np.zeros((4, 19))
        r[0, :] = -big; r[0, 3] = big
        r[1, :] = -big; r[1, 3] = big; r[1, 17] = big
        r[2, :] = -big; r[2, 5] = 0.0; r[2, 6] = -1.0
        r[3, :] = _rest(rng, 19, -2, 2); r[3, 0] = big
        out.append(Case(f"extreme_{kind}", r, None, 1025, 23, 1, large_d=True, kinds=(kind,)))
    # (b) -inf entries: one, many, all but one, all
    A = 40
    base = _rest(rng, 8 * A, -4, 4).reshape(8, A)
    for name, dead in (("one", [11]), ("many", sorted(rng.choice(A, size=23, replace=False).tolist())), ("all_but_one", [i for i in range(A) if i != 26]),
                       ("all", list(range(A)))):
        b = np.zeros(A)
        b[dead] = -np.inf
        out.append(Case(f"neginf_{name}", base, b, 2049, 24, 7))
    # (c) ties: all logits equal
    for A in (2, 16, 17, 32, 33, 222):
        out.append(Case(f"all_equal_{A}", np.full((1, A), 1.5), None, 4097, 25 + A, 3, ties=True))
    # (c) exact ties at the top, everything else flushed (exp(-200) = 0 in f32): the winner is the largest u among the tied
    A = 222
    places = [(3, 19),        # one lane of sample_kernel (a % 16)
              (3, 4),         # two lanes of one 16-lane group
              (0, 1),         # one lane of the head kernels
              (2, 6),         # the two lane halves of the head kernels (a, a + 4)
              (5, 69),        # two action tiles, two waves of mid_head_small_kernel (tile % 4)
              (10, 138),      # two action tiles of one wave there (tiles 0 and 4)
              (7, 11, 200), (0, 32, 64), (31, 63, 221)]
    r = np.full((len(places), A), -200.0)
    for j, p in enumerate(places):
        r[j, list(p)] = 0.0
    out.append(Case("top_ties", r, None, 4099, 26, 4, ties=True, large_d=True))
    # the same placements with a live tail two below the top: ordinary margins apply
    r2 = np.tile(-2.0 - _rest(rng, A, 0, 4), (len(places), 1))
    for j, p in enumerate(places):
        r2[j, list(p)] = 0.0
    out.append(Case("top_ties_live_tail", r2, None, 4099, 27, 4))
    return out


SHAPE_A = (1, 15, 16, 17, 31, 32, 33, 221, 222)
SHAPE_B = (1, 3, 5, 41)


def shape_case(A: int, B: int) -> Case:
    """Random multiples of 1/8 in [-6, 6].  The seed offset is one for which the REFERENCE has no key margin under 1e-3 in any of the
    small batches (a single such row would be more than 1 % of 41 envs); test_collect_ref.py keeps that checked."""
    rng = np.random.default_rng(A * 1000 + B)
    return Case(f"shape_{A}_{B}", _rest(rng, min(B, 32) * A, -6, 6).reshape(min(B, 32), A), None, B, 31 + A, B)


PEAKED_ROW = np.array([0.0, -4.0, -7.0, -9.2, -11.5, -60.0, -200.0])
JOINT_ROW = np.array([0.3, -1.2, 2.0, 0.0, 1.1, -3.0])
