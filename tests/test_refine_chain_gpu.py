"""qmax_refine2_kernel (csrc/xq_refine.hip.h) after its loads were regrouped into four dependent levels — `pytest -m gpu`.

The kernel's arithmetic did not change, so every check is an equality: the TD work riding in the refine blocks against the same step
kernel by kernel (td_delta_kernel), the two forms of the whole-group pass against each other, and the screened maximum against the full
product within the bound the existing screening tests use (2e-6).

The candidate scan has two paths, chosen by the geometry the screening pass hands over (screen_geometry, xq_screen.hip.h; `_geometry`
below restates it for a 256-CU device and a 256-wide last hidden layer):
  * at most 16 row ranges of at most 16 lane groups: both ranges of a thread (phase p owns ranges p and p + 8) are decided from maxima
    kept in registers and their P1 / P2 loads share round trips.  With 256 CUs that is n = 7681 .. 8192 (16 panels of 512 samples,
    16 ranges of 512 rows = 16 groups): the bench's shape.  Sizes here: 7681 = 240 whole blocks of 32 samples + a block with ONE live
    sample (every load of its other 31 lanes is clamped), and 8192 (whole blocks only) for the two-candidate case;
  * anything else re-reads the maxima range by range.  Sizes here: 897, the smallest batch the screen takes (64 x ceil(n / 128) >= 512
    tiles; 127 ranges of 2 groups; 28 whole blocks + one live sample), and 928 (whole blocks only).
Common to all: actions -1 and >= 96 (no Q(s,a), no view row: the unconditional row loads read a stand-in row whose value must not
leak), terminal samples, rewards of both signs.  Two candidates per sample: rows 10 and 4100 — in the 16-range geometry ranges 0 and 8,
both owned by phase 0, so ONE thread has both of its ranges above the threshold; in the 127-range geometry ranges 0 and 64, again one
thread (phase 0), in two trips of its loop.  Every group of every range a candidate, as whole groups: all output rows equal.
"""
import numpy as np
import pytest

from test_dqn_gpu import CFG2_NET, make_net

pytestmark = pytest.mark.gpu

N_RAGGED, N_WHOLE = 897, 928            # re-reading path
N_TWO_RAGGED, N_TWO_WHOLE = 7681, 8192  # two-range path
NOUT, HL = CFG2_NET[-1], CFG2_NET[-2]


def _geometry(n, ncu=256):
    """(row ranges, lane groups per range) of the screening pass for a 256-wide last hidden layer: screen_geometry + qmax_screened"""
    nchunks = (NOUT + 63) // 64
    panels = (n + 511) // 512
    ranges = min(max(ncu // panels, 1), nchunks)
    cpr = (nchunks + ranges - 1) // ranges
    return (nchunks + cpr - 1) // cpr, 2 * cpr


def test_sizes_reach_both_paths_of_the_scan():
    for n in (N_TWO_RAGGED, N_TWO_WHOLE):
        ranges, gpr = _geometry(n)
        assert (ranges, gpr) == (16, 16)                       # two-range path; rows 10 / 4100 in ranges 0 / 8 (512 rows each): phase 0
        assert 10 // (32 * gpr) == 0 and 4100 // (32 * gpr) == 8
    for n in (N_RAGGED, N_WHOLE):
        ranges, gpr = _geometry(n)
        assert (ranges, gpr) == (127, 2)                       # re-reading path; rows 10 / 4100 in ranges 0 / 64: phase 0 again
        assert 10 // (32 * gpr) % 8 == 0 and 4100 // (32 * gpr) % 8 == 0


@pytest.fixture(scope="module")
def xq():
    import cn_chess_ai_amd as m
    assert m._capi.device_count() > 0
    return m


@pytest.fixture(scope="module")
def batch(xq):
    """8192 transitions of a short random self-play (every size takes the first n of them); built once, never written to."""
    n = N_TWO_WHOLE
    env = xq.VecEnv(n, seed=17)
    for _ in range(9):
        env.selfplay_step(None)
    S, _ = env.get_state()
    res = env.selfplay_step(None)
    S2, _ = env.get_state()
    env.close()
    rng = np.random.default_rng(23)
    A = (res["action"] % 90).astype(np.int32)
    A[3::11] = -1                                              # no action: no Q(s,a), delta 0
    A[5::13] = 96 + rng.integers(0, NOUT - 96, size=len(A[5::13]))   # outside the trained rows: the same
    A[0] = NOUT - 1
    for m in (N_RAGGED, N_TWO_RAGGED):
        assert 0 <= A[m - 1] < 90                              # the lone live sample of the last block at a ragged size has a Q(s,a)
    R = rng.uniform(-1.0, 1.0, size=n).astype(np.float32)
    D = res["done"].copy()
    D[::7] = 1
    for a in (S, S2, A, R, D):
        a.setflags(write=False)
    return S, S2, A, R, D


def _cut(batch, n):
    return tuple(a[:n] for a in batch)


def _step(d, batch, n, lr, td_net=0):
    S, S2, A, R, D = _cut(batch, n)
    return d.td_update(S, S2, A, R, D, td_net=td_net, mode=0, learning_rate=lr, grad_scale=1.0 / n)


@pytest.mark.parametrize("loss", ["squared", "huber"])
@pytest.mark.parametrize("n", [N_RAGGED, N_WHOLE, N_TWO_RAGGED])
def test_td_in_the_refine_blocks_equals_the_step_kernel_by_kernel(xq, batch, n, loss):
    """set_td_tail(True): target, delta, loss and top hidden delta come out of the refine kernel; (False): out of td_delta_kernel behind
    it.  One step with a learning rate: Q(s,a), y, the loss and every parameter bit for bit, and the screen did run."""
    from cn_chess_ai_amd import _capi
    out = {}
    for tail in (True, False):
        d, w, b = make_net(xq, CFG2_NET, seed=41)
        d.set_qmax_mode(_capi.QMAX_SCREENED)
        d.set_td_tail(tail)
        if loss == "huber":
            d.set_td_loss("huber", 0.5)                        # errors reach ~2 here: both branches of the clamp
        before = d.qmax_stats()[0]
        q, y = _step(d, batch, n, lr=0.05)
        assert d.qmax_stats()[0] == before + 1                 # not the full product
        out[tail] = (q.copy(), y.copy(), d.last_loss(), d.get_params())
        d.close()
    (q1, y1, l1, (w1, b1)), (q0, y0, l0, (w0, b0)) = out[True], out[False]
    assert np.array_equal(q1, q0) and np.array_equal(y1, y0) and l1 == l0
    assert np.array_equal(w1, w0) and np.array_equal(b1, b0)
    assert np.abs(w1 - w).max() > 0                            # the step moved the weights
    A = batch[2][:n]
    assert not q1[(A < 0) | (A >= 96)].any() and np.abs(q1[(A >= 0) & (A < 96)]).min() > 0


def _lifted(w, b, rows, src, lift):
    """the net with W_out[rows] = W_out[src] (bias too), their biases raised by `lift`"""
    w, b = w.copy(), b.copy()
    wo, bo = w[-NOUT * HL:].reshape(NOUT, HL), b[-NOUT:]
    wo[rows] = wo[src]
    bo[rows] = bo[src] + lift
    return w, b


@pytest.mark.parametrize("n", [N_RAGGED, N_WHOLE, N_TWO_RAGGED, N_TWO_WHOLE])
def test_candidates_in_both_ranges_of_one_thread(xq, batch, n):
    """Rows 10 and 4100 carry the same weights and the same raised bias: both lead for every sample, in the two ranges that phase 0 owns
    (ranges 0 and 8 at n = 7681 / 8192, where their loads share one round trip; ranges 0 and 64 at n = 897 / 928)."""
    from cn_chess_ai_amd import _capi
    d, w, b = make_net(xq, CFG2_NET, seed=43)
    d.set_params(*_lifted(w, b, [10, 4100], 10, 1.5))
    d.set_qmax_mode(_capi.QMAX_FULL)
    _, y_full = _step(d, batch, n, lr=0.0)
    d.set_qmax_mode(_capi.QMAX_SCREENED)
    ys, qs = {}, {}
    pairs0 = d.qmax_stats()[2]
    for tail in (True, False):
        d.set_td_tail(tail)
        qs[tail], ys[tail] = (a.copy() for a in _step(d, batch, n, lr=0.0))
    steps, samples, pairs, _ = d.qmax_stats()
    assert steps == 2 and samples == 2 * n
    assert pairs - pairs0 >= 2 * 2 * n, (pairs, pairs0)        # two candidate pairs per sample and step
    assert np.abs(ys[True] - y_full).max() < 2e-6
    assert np.array_equal(ys[True], ys[False]) and np.array_equal(qs[True], qs[False])
    d.close()


@pytest.mark.parametrize("n", [N_RAGGED, N_TWO_RAGGED])
def test_every_group_of_every_range_as_whole_groups(xq, batch, n):
    """All output rows equal: both screened values of every lane group reach the threshold, so every group of every range of every sample
    is re-evaluated whole — from global memory (stage 0) and through LDS (stage 1), with the same bits."""
    from cn_chess_ai_amd import _capi
    d, w, b = make_net(xq, CFG2_NET, seed=47)
    d.set_params(*_lifted(w, b, slice(None), 7, 0.0))
    d.set_qmax_mode(_capi.QMAX_FULL)
    _, y_full = _step(d, batch, n, lr=0.0)
    d.set_qmax_mode(_capi.QMAX_SCREENED)
    ys = {}
    for stage in (0, 1):
        d.set_refine_stage(stage)
        ys[stage] = _step(d, batch, n, lr=0.0)[1].copy()
    steps, samples, pairs, whole = d.qmax_stats()
    assert steps == 2 and samples == 2 * n
    assert whole >= 2 * 200 * n, (pairs, whole)                # >= 200 whole groups per sample and step (254 lane groups)
    assert np.array_equal(ys[0], ys[1])
    assert np.abs(ys[1] - y_full).max() < 2e-6
    d.close()
