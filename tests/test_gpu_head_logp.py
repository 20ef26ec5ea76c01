"""qg_policy_head_logp / qg_policy_mid_head_logp -- the deterministic epilogue of head_sample_kernel, mid_head_small_kernel and
mid_head_sample_kernel -- on prescribed logits: the arg-max with its tie rule, the rows of log-probabilities against the f64 reference
(logp_ref.py), bit-identity with what the sampling entry points report on the same operands, masks, guards, NULL outputs and limits.
The logits are prescribed exactly with the two-bf16 split of test_gpu_sampling_edges.py::head_operands (restated here): h W^T + b equals
the chosen f32 rows bit for bit, and a 0/1 selection W2 passes h1 through the middle layer."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from logp_cases import RANDOM_A, RANDOM_F, RANDOM_MAX_UNCLEAR, random_reference, random_weights  # noqa: E402
from logp_ref import logp_ref, logsumexp_rows  # noqa: E402
from sampling_cases import two_bf16  # noqa: E402

ENTRIES = ("head", "mid_small", "mid_big")
TOL = {"head": 2e-4, "mid_small": 3e-5, "mid_big": 3e-5}  # log-prob tolerances of test_gpu_sampling_edges.py (TOL)
TOL_ENT = {"head": 2e-4, "mid_small": 1e-4, "mid_big": 1e-4}  # ... and their entropy tolerances
GUARD = 16
MID_F, HEAD_K = 256, 128
K1_OF = {"mid_small": 128, "mid_big": 96}  # 96 is no multiple of 128: mid_head_sample_kernel at every batch size
SMALL_KERNEL_MAX = 8192
SENT = -1234.5
SHAPE_A = (1, 31, 32, 33, 170, 222)
SHAPE_B = (1, 33, 300)
J_ROWS = 40  # distinct logit rows of a case: 2 * J_ROWS <= 96


def head_operands(rows, bias, B, K, mask_value=-np.inf, values=None):
    """h [B, K] bf16 and W [A + 1, K], b [A + 1] f32 with h W^T + b = rows[e % J] + bias exactly: the logit is spread over two bf16
    weights (hi, lo) that a pair of ones in h adds up; row A is the value head (values[e % J], bf16-exact, or 0).  -inf in `bias` is
    handed over as `mask_value`."""
    J, A = rows.shape
    assert 2 * J <= K
    hi, lo = two_bf16(rows)
    w = np.zeros((A + 1, K), dtype=np.float32)
    w[:A, 0:2 * J:2] = hi.T
    w[:A, 1:2 * J:2] = lo.T
    if values is not None:
        w[A, 0:2 * J:2] = values
    h = torch.zeros((B, K), dtype=torch.bfloat16, device="cuda")
    e = torch.arange(B, device="cuda")
    h[e, 2 * (e % J)] = 1.0
    h[e, 2 * (e % J) + 1] = 1.0
    b = None
    if bias is not None:
        b = np.zeros(A + 1, dtype=np.float32)
        b[:A] = np.where(np.isneginf(bias), mask_value, bias).astype(np.float32)
        b = torch.from_numpy(b).cuda()
    return h, torch.from_numpy(w).cuda(), b


_SELECT = {}


def mid_select(K1):
    """W2 = a 0/1 selection: h2 = relu(h1 W2^T) = h1 exactly (features K1.. stay 0)."""
    if K1 not in _SELECT:
        from qiskit_gym_amd.collector import pack_mid
        w2 = torch.zeros((MID_F, K1), device="cuda")
        w2[torch.arange(K1), torch.arange(K1)] = 1.0
        _SELECT[K1] = pack_mid(w2, None)
    return _SELECT[K1]


class Ops:
    """The operands of one entry point for L[e] = rows[e % J] + bias, value[e] = values[e % J]."""

    def __init__(self, entry, rows, bias, B, mask_value=-np.inf, values=None, K1=None):
        from qiskit_gym_amd.collector import pack_head
        self.entry, self.B, self.A = entry, B, rows.shape[1]
        A = self.A
        if entry == "head":
            self.h, w, b = head_operands(rows, bias, B, HEAD_K, mask_value, values)
            self.head, self.mid = pack_head(w, b, A, A), None
        else:
            K1 = K1 or K1_OF[entry]
            assert (B <= SMALL_KERNEL_MAX and K1 % 128 == 0) if entry == "mid_small" else (B > SMALL_KERNEL_MAX or K1 % 128 != 0)
            self.h, w3, b = head_operands(rows, bias, B, K1, mask_value, values)
            w = torch.zeros((A + 1, MID_F), device="cuda")
            w[:, :K1] = w3
            self.head, self.mid = pack_head(w, b, A, A, after_mid=True), mid_select(K1)

    def logp(self, **kw):
        from qiskit_gym_amd.collector import head_logp, mid_head_logp
        if self.mid is None:
            return head_logp(self.h, self.head, self.A, **kw)
        return mid_head_logp(self.h, self.mid, MID_F, self.head, self.A, **kw)

    def sample(self, seed, counter, **kw):
        from qiskit_gym_amd.collector import head_sample, mid_head_sample
        if self.mid is None:
            return head_sample(self.h, self.head, self.A, seed, counter, **kw)
        return mid_head_sample(self.h, self.mid, MID_F, self.head, self.A, seed, counter, **kw)

    def raw(self, rows_ptr, ld, act_ptr, best_ptr, ent_ptr, val_ptr, A=None, in_features=None):
        """The C entry point itself; returns its status."""
        from qiskit_gym_amd import _lib
        L, h, A = _lib.load(), self.h, self.A if A is None else A
        K = h.shape[1] if in_features is None else in_features
        if self.mid is None:
            return L.qg_policy_head_logp(h.data_ptr(), h.stride(0), self.B, K, self.head.data_ptr(), A, rows_ptr, ld, act_ptr, _lib.ACT_I64, best_ptr, ent_ptr,
                                         val_ptr, None)
        return L.qg_policy_mid_head_logp(h.data_ptr(), h.stride(0), self.B, K, self.mid.data_ptr(), MID_F, self.head.data_ptr(), A, rows_ptr, ld, act_ptr,
                                         _lib.ACT_I64, best_ptr, ent_ptr, val_ptr, None)


class Out:
    """Output buffers with guard elements behind them; the rows live in a flat sentinel-filled buffer at element offset `off` with row
    stride `ld` (off = 1: a row base misaligned by 4 bytes)."""

    def __init__(self, B, A, int32=False, ld=None, off=0):
        self.B, self.A, self.ld, self.off = B, A, ld or (A + 3) // 4 * 4, off
        self.flat = torch.full((off + (B + GUARD) * self.ld,), SENT, dtype=torch.float32, device="cuda")
        self.act = torch.full((B + GUARD,), -77, dtype=torch.int32 if int32 else torch.int64, device="cuda")
        self.f = [torch.full((B + GUARD,), SENT, dtype=torch.float32, device="cuda") for _ in range(3)]

    def rows_view(self):
        return self.flat[self.off:].view(self.B + GUARD, self.ld)[:self.B]

    def kwargs(self):
        return dict(logp_rows=self.rows_view(), actions=self.act[:self.B], best_logp=self.f[0][:self.B], entropy=self.f[1][:self.B], values=self.f[2][:self.B])

    def check_guards(self):
        assert (self.act[self.B:] == -77).all()
        for t in self.f:
            assert (t[self.B:] == SENT).all()
        full = self.flat[self.off:].view(self.B + GUARD, self.ld)
        assert (full[self.B:] == SENT).all() and (full[:, self.A:] == SENT).all() and (self.flat[:self.off] == SENT).all()

    def numpy(self):
        return (self.rows_view()[:, :self.A].cpu().numpy(), self.act[:self.B].cpu().numpy(), *(t[:self.B].cpu().numpy() for t in self.f))


def grid_rows(A, seed=0):
    """J_ROWS logit rows on a grid of 1/8 in [-4, 4] (exact in bf16), the first ones hand-made: exact ties of the maximum inside one lane
    (actions a, a + 1), across the two lane halves (a, a + 4), across action tiles (a, a + 32: another wave of mid_head_small_kernel),
    the maximum on the last action, an action 90 below the maximum, everything else far below."""
    rng = np.random.default_rng(seed + A)
    rows = rng.integers(-32, 25, size=(J_ROWS, A)) / 8.0  # random rows: maxima of 3.0 are tied often
    top = 5.0

    def tie(j, *idx):
        for i in idx:
            if i < A:
                rows[j, i] = top
    tie(0, 1, 2)
    tie(1, 2, 6)
    tie(2, 3, 35)
    tie(3, A - 1)
    tie(4, A - 1, 0)
    tie(5, 9, 13, 41, 141)
    tie(6, 7, 3)          # rows[6, 3] == rows[6, 7]: the lower index wins
    rows[7, :] = -86.0
    tie(7, A // 2)
    if A > 1:
        rows[7, 0] = top - 90.0
    tie(8, 100, 68, 36)
    tie(9, 31, 32)
    return rows.astype(np.float64)


def reference(rows, bias, B):
    L = rows[np.arange(B) % rows.shape[0]]
    return L if bias is None else L + bias


def check(entry, out, L, exact_rows=None):
    """One launch against logp_ref on the matrix the kernel saw."""
    rows, act, best, ent, val = out.numpy()
    B, A = L.shape
    want_rows, want_act, want_best, want_ent = logp_ref(L)
    np.testing.assert_array_equal(act, want_act)
    assert np.array_equal(np.isneginf(rows), np.isneginf(want_rows)) and not np.isnan(rows).any() and not np.isposinf(rows).any()
    fin = np.isfinite(want_rows)
    err = np.abs(rows[fin] - want_rows[fin]).max() if fin.any() else 0.0
    live = fin.any(axis=1)
    lse = np.abs(logsumexp_rows(rows)[live]).max() if live.any() else 0.0
    print(f"{entry} A={A} B={B}: max log-prob error {err:.3e}, max |logsumexp(row)| {lse:.3e} (tol {TOL[entry]:.0e})")
    assert err <= TOL[entry] and lse <= TOL[entry]
    assert rows[np.arange(B), act].tobytes() == np.where(live, best, rows[np.arange(B), act]).astype(np.float32).tobytes()
    assert (best[~live] == 0).all() and (ent[~live] == 0).all() and (act[~live] == 0).all()
    assert np.abs(best - want_best).max() <= TOL[entry]
    assert np.abs(ent - want_ent).max() <= TOL_ENT[entry]


VALUES = (np.arange(J_ROWS) - 7.0) / 4.0  # bf16-exact value-head outputs, one per logit row


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("A", SHAPE_A)
def test_rows_argmax_and_agreement_with_the_sampling_entry(A, entry):
    """Arg-max (ties inside a lane, across lane halves, across tiles, maximum on the last action), rows against the f64 reference,
    rows[e, action] == best_logp, and on the same operands the sampling entry's log-prob / entropy / values bit for bit; int32 and int64
    actions, guards behind every output."""
    rows = grid_rows(A)
    for B in SHAPE_B:
        ops = Ops(entry, rows, None, B, values=VALUES)
        L = reference(rows, None, B)
        for int32 in (False, True):
            out = Out(B, A, int32)
            ops.logp(**out.kwargs())
            torch.cuda.synchronize()
            out.check_guards()
            check(entry, out, L)
        got_rows, act, best, ent, val = out.numpy()
        np.testing.assert_array_equal(val, VALUES[np.arange(B) % J_ROWS].astype(np.float32))
        for seed, counter in ((5, 0), (6, 3)):
            s_act, s_logp, s_ent, s_val = (t.cpu().numpy() for t in ops.sample(seed, counter))
            assert got_rows[np.arange(B), s_act].tobytes() == s_logp.tobytes()
            assert ent.tobytes() == s_ent.tobytes() and val.tobytes() == s_val.tobytes()


def test_mid_big_natural_route():
    """mid_head_sample_kernel where qg_policy_mid_head_sample takes it by itself: in_features = 128, more than 8 192 envs."""
    A, B = 170, SMALL_KERNEL_MAX + 32
    rows = grid_rows(A)
    ops = Ops("mid_big", rows, None, B, values=VALUES, K1=128)
    out = Out(B, A)
    ops.logp(**out.kwargs())
    torch.cuda.synchronize()
    out.check_guards()
    check("mid_big", out, reference(rows, None, B))
    s_act, s_logp, s_ent, s_val = (t.cpu().numpy() for t in ops.sample(5, 1))
    got_rows, act, best, ent, val = out.numpy()
    assert got_rows[np.arange(B), s_act].tobytes() == s_logp.tobytes() and ent.tobytes() == s_ent.tobytes() and val.tobytes() == s_val.tobytes()


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("mask_value", [-np.inf, float(np.finfo(np.float32).min)])
def test_masked_columns_and_rows(entry, mask_value):
    """A bias of -inf or at the dtype's lowest gives -inf in that column; with every column masked: action 0, best log-prob 0, entropy 0 and
    a row of -inf."""
    A, B = 33, 70
    rows = grid_rows(A)
    for masked in (np.arange(A) % 3 == 1, np.arange(A) != 32, np.arange(A) != 5, np.ones(A, dtype=bool)):
        bias = np.where(masked, -np.inf, 0.0)
        out = Out(B, A)
        Ops(entry, rows, bias, B, mask_value=mask_value).logp(**out.kwargs())
        torch.cuda.synchronize()
        out.check_guards()
        check(entry, out, reference(rows, bias, B))
        got = out.numpy()
        assert np.isneginf(got[0][:, masked]).all()
        if masked.all():
            assert (got[1] == 0).all() and (got[2] == 0).all() and (got[3] == 0).all()


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("A", [33, 170])
def test_row_layouts(entry, A):
    """ld_logp = A + 3 with sentinel columns, and a row base misaligned by 4 bytes (a view buf[1:] of a flat buffer): the narrow-store path
    writes the bits of the 16-byte path and nothing else."""
    B = 33
    rows = grid_rows(A)
    ops = Ops(entry, rows, None, B)
    ref = Out(B, A)
    ops.logp(**ref.kwargs())
    for ld, off in ((A + 3, 0), ((A + 3) // 4 * 4, 1), (A, 0), (A + 3, 3)):
        out = Out(B, A, ld=ld, off=off)
        ops.logp(**out.kwargs())
        torch.cuda.synchronize()
        out.check_guards()
        for x, y in zip(out.numpy(), ref.numpy()):
            assert x.tobytes() == y.tobytes(), (ld, off)
    check(entry, ref, reference(rows, None, B))


@pytest.mark.parametrize("entry", ENTRIES)
def test_null_outputs_and_limits(entry):
    """want_rows=False writes no row; every NULL combination but the empty one is QG_OK and leaves the other outputs' bits alone; all NULL
    and ld_logp < A are QG_ERR_INVALID; limits beyond the fused head are QG_ERR_UNSUPPORTED, as for the sampling entry."""
    from qiskit_gym_amd import _lib
    A, B = 37, 33
    rows = grid_rows(A)
    ops = Ops(entry, rows, None, B)
    full = Out(B, A)
    ops.logp(**full.kwargs())
    out = Out(B, A)
    kw = out.kwargs()
    untouched = kw.pop("logp_rows")
    res = ops.logp(want_rows=False, **kw)
    torch.cuda.synchronize()
    assert res[0] is None and (untouched == SENT).all() and (out.flat == SENT).all()
    for x, y in zip(out.numpy()[1:], full.numpy()[1:]):
        assert x.tobytes() == y.tobytes()
    want = full.numpy()
    for combo in range(32):
        o = Out(B, A)
        ptrs = [o.rows_view().data_ptr(), o.act.data_ptr(), o.f[0].data_ptr(), o.f[1].data_ptr(), o.f[2].data_ptr()]
        ptrs = [p if combo >> i & 1 else None for i, p in enumerate(ptrs)]
        rc = ops.raw(ptrs[0], o.ld, *ptrs[1:])
        torch.cuda.synchronize()
        assert rc == (_lib.QG_OK if combo else -1), (combo, rc)  # QG_ERR_INVALID = -1
        o.check_guards()
        for i, (x, y) in enumerate(zip(o.numpy(), want)):
            if combo >> i & 1:
                assert x.tobytes() == y.tobytes(), (combo, i)
            else:
                assert (x == (SENT if i != 1 else -77)).all(), (combo, i)
    o = Out(B, A)
    ptrs = (o.act.data_ptr(), o.f[0].data_ptr(), o.f[1].data_ptr(), o.f[2].data_ptr())
    assert ops.raw(o.rows_view().data_ptr(), A - 1, *ptrs) == -1                      # ld_logp < num_actions: QG_ERR_INVALID
    wide = Out(B, 1000)  # rows that would hold such a call's output
    assert ops.raw(wide.rows_view().data_ptr(), wide.ld, *ptrs, A=224) == -3          # more action tiles than the fused head has: QG_ERR_UNSUPPORTED
    assert ops.raw(wide.rows_view().data_ptr(), wide.ld, *ptrs, A=1000) == -3
    assert ops.raw(o.rows_view().data_ptr(), o.ld, *ptrs, in_features=100) == -3      # in_features the kernels do not take
    with pytest.raises(_lib.QGymError):
        _lib.check(ops.raw(None, 0, None, None, None, None))
    torch.cuda.synchronize()
    assert (o.flat == SENT).all() and (wide.flat == SENT).all()


def test_random_bf16_weights():
    """Random bf16 weights (A = 170, K1 = 512, B = 300) against the f64 reference that rounds h2 to bf16 like the kernel: tolerance and
    the rule for unclear rows of test_gpu_collect_ops.py::test_mid_head_sample_random_weights; at most 20 % of the rows are left out of
    the arg-max comparison (test_logp_ref.py checks the seed on the CPU)."""
    from qiskit_gym_amd.collector import mid_head_logp, pack_head, pack_mid
    A, F = RANDOM_A, RANDOM_F
    h1, w2, b2, w3, b3 = random_weights()
    full, clear = random_reference(h1, w2, b2, w3, b3)
    assert 1.0 - clear.mean() <= RANDOM_MAX_UNCLEAR
    t = lambda x: torch.from_numpy(x).cuda().to(torch.bfloat16)  # noqa: E731
    rows, act, best, ent, val = mid_head_logp(t(h1), pack_mid(t(w2), t(b2)), F, pack_head(t(w3), t(b3), A, A, after_mid=True), A)
    torch.cuda.synchronize()
    want_rows, want_act, want_best, want_ent = logp_ref(full[:, :A])
    got = act.cpu().numpy()
    np.testing.assert_array_equal(got[clear], want_act[clear])
    err = np.abs(rows.cpu().numpy() - want_rows).max()
    print(f"random weights: unclear {1 - clear.mean():.3f}, max log-prob error {err:.3e}")
    assert err <= 2e-2
    np.testing.assert_allclose(val.cpu().numpy(), full[:, A], rtol=0, atol=2e-2)
    assert rows.cpu().numpy()[np.arange(len(got)), got].tobytes() == best.cpu().numpy().tobytes()


def test_small_and_big_kernels_agree():
    """mid_head_small_kernel on 300 envs and mid_head_sample_kernel on the same 300 rows inside a batch of 8 224 (K1 = 128): identical
    rows and actions.  The two kernels add the same softmax terms in different orders (per wave and then over the waves, against down
    the lane), so bit-identity is a fair demand only where that sum is exact, and the operands are chosen so: k tied maxima (terms of
    exactly 1, k from 1 to all unmasked actions, at random places: the tie rule across lanes, halves, tiles and waves decides the action) above actions
    110 to 130 below them (terms of exactly 0: 2^-158 is below the smallest f32) or masked ones.  On general rows the two differ in the
    last bits of logf(sum), as their sampling twins do."""
    A, B = 170, 300
    rng = np.random.default_rng(11)
    rows = -(110.0 + rng.integers(0, 161, size=(J_ROWS, A)) / 8.0)
    bias = np.where(np.arange(A) % 11 == 3, -np.inf, 0.0)
    free = np.flatnonzero(np.isfinite(bias))  # the maxima sit on unmasked actions
    for j in range(J_ROWS):
        k = (1 + (j * 5) % free.size) if j else free.size
        rows[j, rng.choice(free, size=k, replace=False)] = 2.0
    small, big = Out(B, A), Out(SMALL_KERNEL_MAX + 32, A)
    Ops("mid_small", rows, bias, B, values=VALUES).logp(**small.kwargs())
    Ops("mid_big", rows, bias, big.B, values=VALUES, K1=128).logp(**big.kwargs())
    torch.cuda.synchronize()
    check("mid_small", small, reference(rows, bias, B))
    for x, y in zip(small.numpy(), big.numpy()):
        assert x.tobytes() == y[:B].tobytes()


def test_graph_capture_and_replay():
    """One capture and replay of mid_head_logp gives the eager result."""
    A, B = 170, 300
    rows = grid_rows(A)
    ops = Ops("mid_small", rows, None, B, values=VALUES)
    eager, out = Out(B, A), Out(B, A)
    ops.logp(**eager.kwargs())
    kw = out.kwargs()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.logp(**kw)
    torch.cuda.synchronize()
    assert (out.flat == SENT).all()  # recorded, not run
    graph.replay()
    torch.cuda.synchronize()
    out.check_guards()
    for x, y in zip(out.numpy(), eager.numpy()):
        assert x.tobytes() == y.tobytes()
