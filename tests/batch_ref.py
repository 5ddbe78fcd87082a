"""Batched fp64 restatement of the TD step defined by the CPU oracle (oracle/xq_oracle.c: xqo_td_target + xqo_nn_accum_grad;
oracle/xq_oracle_ext.c: xqo_ext_td_accum), over a whole minibatch with numpy.  Test infrastructure only, like refnn.py: tests
import it, the product path never does.

The oracle works one sample at a time in scalar C; this module does the same arithmetic as dense fp64 products over chunks of at
most CHUNK samples, so that a TD step of 8192 or 16384 samples can be checked element by element in seconds.
tests/test_batch_ref_cpu.py pins it to the oracle to 1e-12 on every combination of net, backprop mode, TD rule, precision and
importance weights the oracle defines.

    fwd = forward(net, boards, next_boards, A, R, D, gamma, td_rule, precision)    # Q(s,a), y, a*, candidate set
    bwd = backward(net, fwd, mode, precision, weights)                              # per-sample deltas
    upd = accumulate(net, fwd, bwd, precision)                                      # gradient sums + error-scale sums
    worst = check_update(net, upd, new_w, new_b, lr, scale, precision, fwd.boards)  # the bound of TOLERANCES below
    q = q_rows(net, boards_or_dense, n_out)                                         # what the inference entry points return

Parameters are flat float64 arrays in the reference layout (dqn.cu:112-140): layer l's weights are an (L[l+1], L[l]) row-major
block at offset wo[l], its biases a block of L[l+1] at bo[l].
"""
import numpy as np

CHUNK = 2048                        # samples per dense block: an 8100-wide fp64 block of s' is then <= 133 MB

PRECISION_F32, PRECISION_BF16, PRECISION_BF16_FULL = 0, 1, 2

# Error budget of one device update against this reference, per precision:
#   |dgot - dref| <= lr * scale * sum_i (|a_ik| (tau * |delta_ij| + eta_l * w_i) + eps_a * |delta_ij|)  +  ulp32(new_jk)
# tau: relative error of the fp32 sums (summation order, rounding of the products);
# eta[l]: absolute budget on the per-sample delta of layer l (hidden layers 0, 1, 2 — a deeper hidden layer takes the third's — then
# the output layer): the error of the
# device's forward pass carried into the delta, e.g. where Q(s,a) ~ y.  Set from MI355X runs of tests/test_td_full_size_gpu.py so
# that the largest observed err / bound is <= 0.5 (the fp32 store alone can reach 0.5: half an ulp against a whole one).  In the
# bf16 modes the output layer's budget is the Q error of the bf16 forward itself (BF16_QTOL's scale, incl. Double DQN arg-max
# near-ties that move y by less than BF16_QTOL); the hidden layers stay tight.
# eps_a: ABSOLUTE error of a device activation a_ik (layers >= 1; the one-hot input of layer 0 is exact).  tau covers an error of a_ik
# in proportion to |a_ik|, which is what the rounding of the product delta * a is; but the activation itself is tanh of an fp32 sum whose
# terms cancel, and its error does not shrink with it: |a_ik| = 2.8e-4 came back 2.2e-8 off (8e-5 of its value) on a step of 65 samples
# on 1260-64-64-8100, and the sample's delta of 0.12 carried that into its W_out element — 8.5 bounds, with the per-sample delta itself
# 4e-8 from the reference (tests/test_td_shape_edges_gpu.py, profiles/NOTES.md).  At 8192 samples ~90 samples share a W_out row and
# the eta term, which grows with the row's sample count, hides it; a row that one sample owns shows it.  The budget is the one the suite
# already holds the device's hidden tanh to, 3e-7 absolute (tests/test_dqn_gpu.py::test_hidden_tanh_accuracy; 5 ulps of an activation
# near 1, where fp32 itself stops).  bf16 nets: reference and device round every activation to the same bf16 grid, so none.
TOLERANCES = {
    PRECISION_F32: dict(tau=2.0 ** -17, eta=(2e-7, 2e-7, 2e-7, 2e-7), eps_a=3e-7),
    PRECISION_BF16: dict(tau=2.0 ** -12, eta=(1e-4, 4e-6, 4e-6, 3.5e-2), eps_a=0.0),
    PRECISION_BF16_FULL: dict(tau=2.0 ** -12, eta=(1e-4, 4e-6, 4e-6, 3.5e-2), eps_a=0.0),
}
QTOL = 1e-4                         # fp32: Q(s,a) absolute, y relative to max(1, |y|)
BF16_QTOL = 1e-2                    # bf16 Q-net (one bf16 ulp of a hidden activation is 2^-8 relative)
LOSS_RTOL = {PRECISION_F32: 1e-4, PRECISION_BF16: 2e-2, PRECISION_BF16_FULL: 2e-2}
CAND_MARGIN = {PRECISION_F32: 2e-6, PRECISION_BF16: 5e-3, PRECISION_BF16_FULL: 5e-3}     # near-maximal online z (Double DQN)
MAX_FLIP_FRACTION = {PRECISION_F32: 0.01, PRECISION_BF16: 0.1, PRECISION_BF16_FULL: 0.1}


class UndefinedTopology(ValueError):
    """Mode 0 (the hidden delta as written) reads out of bounds for this topology: the oracle returns -1 there."""


def offsets(sizes):
    wo, bo, tw, tb = [], [], 0, 0
    for i, o in zip(sizes[:-1], sizes[1:]):
        wo.append(tw); bo.append(tb)
        tw += i * o; tb += o
    return wo, bo, tw, tb


def bf16_round(x):
    """xqo_bf16_round on every element: through fp32, round to nearest even on 8 significant bits, inf / nan unchanged."""
    f = np.ascontiguousarray(np.asarray(x, dtype=np.float64).astype(np.float32))
    u = f.view(np.uint32)
    fin = (u & np.uint32(0x7F800000)) != np.uint32(0x7F800000)
    r = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return np.where(fin, r, u).astype(np.uint32).view(np.float32).astype(np.float64)


def one_hot(boards):
    """xo.state_repr of packed 90-byte boards: input s*14 + piece-1 is 1 for every occupied square s.  A float array is taken as
    the dense inputs themselves (nets whose input is not a board)."""
    if np.asarray(boards).dtype.kind == "f":
        return np.asarray(boards, dtype=np.float64)
    boards = np.asarray(boards, dtype=np.uint8).reshape(-1, 90)
    x = np.zeros((len(boards), 90 * 14))
    r, s = np.nonzero(boards)
    x[r, s * 14 + boards[r, s].astype(np.int64) - 1] = 1.0
    return x


def _inputs(x):
    x = np.asarray(x)
    return x if x.dtype.kind == "f" else np.asarray(x, dtype=np.uint8).reshape(-1, 90)


class Net:
    """One parameter set: its layers as matrices, and the operands of the forward pass in the given precision."""

    def __init__(self, sizes, w, b, precision=PRECISION_F32):
        self.sizes = [int(s) for s in sizes]
        self.nl = len(self.sizes) - 1
        self.w = np.asarray(w, dtype=np.float64)
        self.b = np.asarray(b, dtype=np.float64)
        self.wo, self.bo, nw, nb = offsets(self.sizes)
        assert self.w.size == nw and self.b.size == nb
        L = self.sizes
        self.W = [self.w[self.wo[l]:self.wo[l] + L[l] * L[l + 1]].reshape(L[l + 1], L[l]) for l in range(self.nl)]
        self.B = [self.b[self.bo[l]:self.bo[l] + L[l + 1]] for l in range(self.nl)]
        bf = precision != PRECISION_F32
        self.Wf = [bf16_round(W) if bf else W for W in self.W]          # forward operands (xq_oracle_ext.c ext_forward)
        self.Bf = [B.astype(np.float32).astype(np.float64) if bf else B for B in self.B]
        self.bf = bf

    def hidden(self, x):
        """hidden activations a_1 .. a_{nl-1} of a block of inputs (bias first, tanh, bf16-rounded in the bf16 modes)"""
        acts, cur = [], x
        for l in range(self.nl - 1):
            a = np.tanh(self.Bf[l] + cur @ self.Wf[l].T)
            if self.bf:
                a = bf16_round(a)
            acts.append(a)
            cur = a
        return acts

    def z_out(self, a_last):
        return self.Bf[-1] + a_last @ self.Wf[-1].T


def q_rows(net, boards_or_dense, n_out, chunk=CHUNK):
    """Q(s)[0 .. n_out) of every row, what the inference entry points return: tanh of the first n_out outputs behind the last hidden
    layer (xo.nn_forward; xo.ext_forward's z through tanh in the bf16 arithmetic, where Net rounds operands and activations)."""
    x = _inputs(boards_or_dense)
    q = np.empty((len(x), n_out))
    for c0 in range(0, len(x), chunk):
        a_last = net.hidden(one_hot(x[c0:c0 + chunk]))[-1]
        q[c0:c0 + chunk] = np.tanh(net.Bf[-1][:n_out] + a_last @ net.Wf[-1][:n_out].T)     # = z_out(a_last)[:, :n_out], only those rows
    return q


class Forward:
    """Per-sample results of the forward half: q = Q(s,a), y, a* (-1 where not defined), hidden activations of s, and for Double
    DQN the target-net values y could take at the near-maximal online outputs (cand_y)."""


def forward(net, boards, next_boards, A, R, D, gamma, td_rule, precision=PRECISION_F32, target=None, chunk=CHUNK):
    """Q(s,a) and the TD target of every sample.  td_rule 0: y = r + gamma max_k Q_online(s')  (chessai.cpp:126)
    1: the target net's maximum (dqn.cpp:166);  2: Double DQN, the target net's tanh at the first strict maximum of the online z.
    Terminal samples take y = r.  `target` is the target net's Net (rules 1, 2)."""
    boards, next_boards = _inputs(boards), _inputs(next_boards)
    n = len(boards)
    A = np.asarray(A, dtype=np.int64).reshape(n)
    R = np.asarray(R, dtype=np.float64).reshape(n)
    D = np.asarray(D).reshape(n).astype(bool)
    assert (A < net.sizes[-1]).all()
    tnet = target if target is not None else net
    f = Forward()
    f.live = A >= 0                                                     # action -1: an empty slot, no gradient (xq_td.hip.h)
    A = np.maximum(A, 0)
    f.n, f.boards, f.A, f.R, f.D, f.td_rule, f.precision = n, boards, A, R, D, td_rule, precision
    f.acts = [np.empty((n, h)) for h in net.sizes[1:-1]]
    f.q, f.y = np.empty(n), R.copy()
    f.astar = np.full(n, -1, np.int64)
    f.cand_y = [None] * n
    margin = CAND_MARGIN[precision]
    for c0 in range(0, n, chunk):
        c1 = min(n, c0 + chunk)
        acts = net.hidden(one_hot(boards[c0:c1]))
        for l, a in enumerate(acts):
            f.acts[l][c0:c1] = a
        a_last, rows = acts[-1], A[c0:c1]
        f.q[c0:c1] = np.tanh(net.Bf[-1][rows] + np.einsum("ij,ij->i", a_last, net.Wf[-1][rows]))
        live = np.nonzero(~D[c0:c1])[0]
        if len(live) == 0:
            continue
        x2 = one_hot(next_boards[c0:c1][live])
        zn = net.z_out(net.hidden(x2)[-1]) if td_rule in (0, 2) else None
        zt = tnet.z_out(tnet.hidden(x2)[-1]) if td_rule in (1, 2) else None
        sel = zt if td_rule == 1 else zn
        star = np.argmax(sel, axis=1)                                   # first maximum (dqn.cpp:48)
        val = zn if td_rule == 0 else zt
        gi = c0 + live
        f.astar[gi] = star
        f.y[gi] = R[gi] + gamma * np.tanh(val[np.arange(len(live)), star])
        if td_rule == 2:
            zmax = sel[np.arange(len(live)), star]
            for k in range(len(live)):
                cand = np.nonzero(sel[k] >= zmax[k] - margin)[0]
                f.cand_y[gi[k]] = R[gi[k]] + gamma * np.tanh(zt[k, cand])
        del zn, zt, sel, val
    return f


class Backward:
    """Per-sample deltas: dout (n,) the single non-zero output delta (x importance weight), d[l] (n, L[l+1]) of hidden layer l."""


def _bf16_layers(net, precision, layers):
    """the hidden layers whose backward product takes bf16 operands: `layers`, or every one under PRECISION_BF16_FULL (the oracle)"""
    if layers is None:
        return set(range(net.nl - 1)) if precision == PRECISION_BF16_FULL else set()
    assert precision == PRECISION_BF16_FULL or not layers, "bf16 backward operands belong to PRECISION_BF16_FULL"
    return set(layers)


def backward(net, f, mode, precision=PRECISION_F32, weights=None, y=None, bf16_layers=None):
    """Deltas of every sample.  mode 0: the hidden delta as written (dqn.cu:406-427, the shifted view of the flat weight array,
    compute_deltas in xq_oracle.c), mode 1: textbook backprop.  `y` replaces the forward's targets (e.g. the device's y where a
    Double DQN arg-max flipped).  bf16_layers: the hidden layers l whose delta product (delta_{l+1} x weight view) takes bf16-rounded
    operands; None: every layer under PRECISION_BF16_FULL, as the oracle does.  The device rounds where the product's shape fits its
    bf16 tiles ("XQ_PRECISION_BF16_FULL"), so a test of other shapes names the layers."""
    L, nl, n = net.sizes, net.nl, f.n
    y = f.y if y is None else np.asarray(y, dtype=np.float64)
    om = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64).reshape(n)
    bk = Backward()
    bk.weights = om * f.live
    bk.dout = (f.q - y) * (1.0 - f.q * f.q) * bk.weights
    rounded = _bf16_layers(net, precision, bf16_layers)
    d = [None] * (nl - 1)
    nw = net.w.size
    for l in range(nl - 2, -1, -1):
        rnd = bf16_round if l in rounded else (lambda v: v)
        if mode == 0:
            inp, outp = L[l + 1], L[l]
            if L[l + 2] < inp or outp < L[l + 1] or net.wo[l + 1] + (inp - 1) * outp + (L[l + 1] - 1) >= nw:
                raise UndefinedTopology(f"mode 0 reads out of bounds at hidden layer {l} of {L}")
            V = net.w[net.wo[l + 1]:net.wo[l + 1] + inp * outp].reshape(inp, outp)[:, :L[l + 1]]   # V[i, idx] = Wflat[wo + i*L[l] + idx]
            if l == nl - 2:
                s = np.zeros((n, L[l + 1]))
                ok = f.A < inp
                s[ok] = V[f.A[ok]] * bk.dout[ok, None]
            else:
                s = rnd(d[l + 1][:, :inp]) @ rnd(V)
        else:
            if l == nl - 2:
                s = net.W[l + 1][f.A] * bk.dout[:, None]
            else:
                s = rnd(d[l + 1]) @ rnd(net.W[l + 1])
        a = f.acts[l]
        d[l] = s * (1.0 - a * a)
    bk.d = d
    return bk


class Update:
    """Gradient sums gW[l], gB[l] and the error-scale sums of the bound: T = sum_i |a_ik| |delta_ij|, U = sum_i w_i |a_ik| (for
    hidden layers U does not depend on j: one row), bias: sum_i |delta_ij| and sum_i w_i.  The output layer keeps rows 0 .. rows-1
    (every action a sample takes); its other rows have no gradient."""


def accumulate(net, f, bk, precision=PRECISION_F32, mask=None, chunk=CHUNK, bf16_layers=None):
    """Sums over the samples (all, or those where mask is True).  bf16_layers: the hidden layers l >= 1 whose weight-gradient product
    (delta_l^T a_l) takes the bf16-rounded delta; None: every one under PRECISION_BF16_FULL, as the oracle does (see backward)."""
    L, nl, n = net.sizes, net.nl, f.n
    keep = np.ones(n, bool) if mask is None else np.asarray(mask, bool)
    u = Update()
    rounded = _bf16_layers(net, precision, bf16_layers)
    rows = int(f.A.max()) + 1
    u.rows = rows
    u.gW = [np.zeros((L[l + 1], L[l])) for l in range(nl - 1)] + [np.zeros((rows, L[nl - 1]))]
    u.gB = [np.zeros(L[l + 1]) for l in range(nl - 1)] + [np.zeros(rows)]
    u.T = [np.zeros_like(g) for g in u.gW]
    u.U = [np.zeros(L[l]) for l in range(nl - 1)] + [np.zeros((rows, L[nl - 1]))]
    u.TB = [np.zeros_like(g) for g in u.gB]
    u.UB = [np.zeros(L[l + 1]) for l in range(nl - 1)] + [np.zeros(rows)]
    for c0 in range(0, n, chunk):
        c1 = min(n, c0 + chunk)
        k = keep[c0:c1]
        om = bk.weights[c0:c1] * k
        acts = [one_hot(f.boards[c0:c1])] + [a[c0:c1] for a in f.acts]
        # output layer: the single non-zero delta at action.to
        dout = bk.dout[c0:c1] * k
        M = np.zeros((c1 - c0, rows))
        M[np.arange(c1 - c0), f.A[c0:c1]] = 1.0
        al = acts[nl - 1]
        u.gW[-1] += M.T @ (dout[:, None] * al)
        u.gB[-1] += M.T @ dout
        u.T[-1] += M.T @ (np.abs(dout)[:, None] * np.abs(al))
        u.U[-1] += M.T @ (om[:, None] * np.abs(al))
        u.TB[-1] += M.T @ np.abs(dout)
        u.UB[-1] += M.T @ om
        for l in range(nl - 1):
            dl = bk.d[l][c0:c1] * k[:, None]
            dw = bf16_round(dl) if l in rounded and l >= 1 else dl     # layer 0 sums the fp32 delta rows
            u.gW[l] += dw.T @ acts[l]
            u.gB[l] += dl.sum(axis=0)
            u.T[l] += np.abs(dw).T @ np.abs(acts[l])
            u.U[l] += om @ np.abs(acts[l])
            u.TB[l] += np.abs(dl).sum(axis=0)
            u.UB[l] += om.sum()
    return u


def td_step(sizes, w, b, boards, next_boards, A, R, D, gamma=0.99, td_rule=0, mode=0, precision=PRECISION_F32, weights=None,
            wt=None, bt=None):
    """forward + backward + accumulate in one call (wt, bt: the target net for rules 1 and 2)."""
    net = Net(sizes, w, b, precision)
    tnet = Net(sizes, wt, bt, precision) if wt is not None else None
    f = forward(net, boards, next_boards, A, R, D, gamma, td_rule, precision, target=tnet)
    bk = backward(net, f, mode, precision, weights)
    return net, f, bk, accumulate(net, f, bk, precision)


def flat_grads(net, u):
    """(gw, gb) as flat arrays in the reference layout (rows >= u.rows of the output layer: zero)."""
    gw, gb = np.zeros_like(net.w), np.zeros_like(net.b)
    for l in range(net.nl):
        L0, L1 = net.sizes[l], net.sizes[l + 1]
        blk = gw[net.wo[l]:net.wo[l] + L0 * L1].reshape(L1, L0)
        blk[:u.gW[l].shape[0]] = u.gW[l]
        gb[net.bo[l]:net.bo[l] + u.gB[l].shape[0]] = u.gB[l]
    return gw, gb


def loss(f, y=None):
    """xq_dqn_last_loss: sum over the samples of 0.5 (Q(s,a) - y)^2 (unweighted)."""
    y = f.y if y is None else y
    return float(0.5 * np.sum(((f.q - y) ** 2)[f.live]))


def priorities(f, eps, alpha, y=None):
    """new PER priorities (|Q(s,a) - y| + eps)^alpha of the sampled transitions (xqo_per_priority)."""
    y = f.y if y is None else y
    return (np.abs(f.q - y) + eps) ** alpha


def _ulp32(v):
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64).astype(np.float32))).astype(np.float64)


def update_ratios(net, u, new_w, new_b, lr, scale, precision, tol=None):
    """max over the elements of each layer of |dgot - dref| / bound, weights and biases apart: {"w0": r, "b0": r, ...}.
    net holds the parameters before the step (what the device started from, fp32 values), new_* what it left."""
    tol = TOLERANCES[precision] if tol is None else tol
    tau, eta, eps_a, sigma = tol["tau"], tol["eta"], tol.get("eps_a", 0.0), tol.get("sigma", 0.0)
    new_w = np.asarray(new_w, dtype=np.float64)
    new_b = np.asarray(new_b, dtype=np.float64)
    ls = lr * scale
    out = {}
    for l in range(net.nl):
        e = eta[min(l, len(eta) - 2)] if l < net.nl - 1 else eta[-1]      # hidden layers past the third: the third's budget
        L0, L1 = net.sizes[l], net.sizes[l + 1]
        r = u.gW[l].shape[0]
        got = new_w[net.wo[l]:net.wo[l] + L0 * L1].reshape(L1, L0)[:r]
        old = net.W[l][:r]
        err = np.abs((got - old) + ls * u.gW[l])
        U = u.U[l] if u.U[l].ndim == 2 else u.U[l][None, :]
        bound = ls * (tau * u.T[l] + e * U + (eps_a if l >= 1 else 0.0) * u.TB[l][:, None]) + _ulp32(got)
        gotb = new_b[net.bo[l]:net.bo[l] + L1][:r]
        errb = np.abs((gotb - net.B[l][:r]) + ls * u.gB[l])
        boundb = ls * (tau * u.TB[l] + e * u.UB[l]) + _ulp32(gotb)
        if sigma:                                   # dense_ref.DENSE_TOLERANCES alone: the hidden deltas' own summation error (u.S, u.SB)
            bound = bound + ls * sigma * u.S[l]
            boundb = boundb + ls * sigma * u.SB[l]
        out[f"w{l}"] = float((err / bound).max())
        out[f"b{l}"] = float((errb / boundb).max())
    return out


def untouched_masks(net, f, mask=None):
    """(W0 columns of (square, piece) pairs on no board s, output actions that no sample takes) — parameters that must not move."""
    keep = (np.ones(f.n, bool) if mask is None else mask) & f.live
    seen = one_hot(f.boards[keep]).any(axis=0)
    taken = np.zeros(net.sizes[-1], bool)
    taken[f.A[keep]] = True
    return ~seen, ~taken


def check_update(net, u, f, new_w, new_b, lr, scale, precision, tol=None):
    """The comparison of a device update with the reference update: every weight and bias within the bound (TOLERANCES), and
    bit-identical where the step must not write: rows >= 96 of W_out, the output rows / biases of actions no sample takes, the
    W0 columns of (square, piece) pairs that appear on no board of the minibatch.  Returns update_ratios."""
    new_w = np.asarray(new_w, dtype=np.float64)
    new_b = np.asarray(new_b, dtype=np.float64)
    L, nl = net.sizes, net.nl
    cols0, untaken = untouched_masks(net, f)
    W0 = new_w[:L[0] * L[1]].reshape(L[1], L[0])
    assert np.array_equal(W0[:, cols0], net.W[0][:, cols0]), "a W0 column of an absent (square, piece) pair moved"
    Wout = new_w[net.wo[-1]:].reshape(L[-1], L[-2])
    Bout = new_b[net.bo[-1]:]
    assert untaken[90:96].all()
    assert np.array_equal(Wout[96:], net.W[-1][96:]), "rows >= 96 of W_out moved"
    assert np.array_equal(Wout[untaken], net.W[-1][untaken]), "a W_out row of an action no sample takes moved"
    assert np.array_equal(Bout[untaken], net.B[-1][untaken]), "an output bias of an action no sample takes moved"
    ratios = update_ratios(net, u, new_w, new_b, lr, scale, precision, tol)
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, f"update outside the bound: {bad} (all: {ratios})"
    return ratios


def check_q_y(f, q_dev, y_dev, precision):
    """Q(s,a) and y of every sample.  Double DQN: a sample whose y differs must have the device's y among the target values of
    the near-maximal online outputs, and at most MAX_FLIP_FRACTION of the samples may differ so.  Returns (flipped sample
    indices, the y the reference gradient takes: the device's at the flipped samples)."""
    q_dev = np.asarray(q_dev, dtype=np.float64)
    y_dev = np.asarray(y_dev, dtype=np.float64)
    bf = precision != PRECISION_F32
    qtol = BF16_QTOL if bf else QTOL
    q_dev = np.where(f.live, q_dev, f.q)
    y_dev = np.where(f.live, y_dev, f.y)
    assert np.abs(q_dev - f.q).max() < qtol, ("Q(s,a)", float(np.abs(q_dev - f.q).max()), int(np.abs(q_dev - f.q).argmax()))
    yerr = np.abs(y_dev - f.y) / (1.0 if bf else np.maximum(1.0, np.abs(f.y)))
    off = yerr >= qtol
    flipped = np.nonzero(off)[0]
    if f.td_rule == 2:
        for i in flipped:
            assert f.cand_y[i] is not None and np.abs(f.cand_y[i] - y_dev[i]).min() < qtol * max(1.0, abs(y_dev[i])), ("y", i)
        assert len(flipped) <= MAX_FLIP_FRACTION[precision] * f.n, (len(flipped), f.n)
    else:
        assert len(flipped) == 0, ("y", float(yerr.max()), int(yerr.argmax()))
    y_use = f.y.copy()
    y_use[flipped] = y_dev[flipped]
    return flipped, y_use
