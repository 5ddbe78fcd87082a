"""fp64 restatement of the Huber TD loss (xq_dqn_set_td_loss, DESIGN.md section 4 "TD loss") on top of tests/batch_ref.py.  Test
infrastructure only: tests import it, the product path never does.

With e = Q(s,a) - y the Huber step replaces e by clamp(e, -kappa, kappa) in the output delta and in nothing else, so it IS the
squared step with every sample's weight multiplied by clamp(e) / e (1 where e = 0):

    bk = batch_ref.backward(net, f, mode, precision, weights=weights(f, kappa, w), y=y)

The gradient sums (batch_ref.accumulate) and the element-wise error budget of batch_ref.check_update then carry over unchanged.
tests/test_huber_ref_cpu.py pins this to torch.nn.functional.huber_loss and its autograd gradient.
"""
import numpy as np


def clamp(e, kappa):
    return np.minimum(np.maximum(e, -kappa), kappa)


def factor(e, kappa):
    """clamp(e, +-kappa) / e, 1 where e = 0 (and wherever |e| <= kappa: exactly 1, so kappa = inf gives today's weights)"""
    e = np.asarray(e, dtype=np.float64)
    out = np.ones_like(e)
    lin = np.abs(e) > kappa
    out[lin] = kappa / np.abs(e[lin])
    return out


def weights(f, kappa, w=None, y=None):
    """per-sample weights for batch_ref.backward: w (importance weights; None = 1) times the Huber factor of the reference's own error"""
    y = f.y if y is None else np.asarray(y, dtype=np.float64)
    om = np.ones(f.n) if w is None else np.asarray(w, dtype=np.float64).reshape(f.n)
    return om * factor(f.q - y, kappa)


def loss_of(e, kappa):
    a = np.abs(np.asarray(e, dtype=np.float64))
    with np.errstate(invalid="ignore"):
        return np.where(a <= kappa, 0.5 * a * a, kappa * (a - 0.5 * kappa))


def loss(f, kappa, y=None, q=None):
    """xq_dqn_last_loss under huber(kappa): the sum over the live samples (unweighted)"""
    y = f.y if y is None else np.asarray(y, dtype=np.float64)
    q = f.q if q is None else np.asarray(q, dtype=np.float64)
    return float(np.sum(loss_of(q - y, kappa)[f.live]))


def stats(q, y, live, kappa):
    """xq_dqn_td_error_stats of device values: e = fl32(q - y) as the step forms it, then everything in fp64; kappa = (float)kappa of
    the handle, inf under the squared loss"""
    q, y = np.asarray(q, dtype=np.float32), np.asarray(y, dtype=np.float32)
    live = np.asarray(live, dtype=bool)
    k = float(np.float32(kappa))
    e = (q - y)[live].astype(np.float64)
    n = int(live.sum())
    a = np.abs(e)
    return dict(live=n, mean_abs=float(a.sum() / n) if n else 0.0, max_abs=float(a.max()) if n else 0.0,
                mean_loss=float(loss_of(e, k).sum() / n) if n else 0.0, linear=int((a > k).sum()))


def copy_with(f, q, y):
    """a shallow copy of a batch_ref.Forward with other Q(s,a) and y (e.g. the device's), for batch_ref.loss / priorities"""
    import copy
    g = copy.copy(f)
    g.q, g.y = q, y
    return g
