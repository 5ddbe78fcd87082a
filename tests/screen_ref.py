"""The screened max pass of a TD step (xq_dqn_set_qmax_mode(XQ_QMAX_SCREENED)) as a plain numpy model, and the inputs that push the true
maximum to the edge of its candidate window.  Test infrastructure only: nothing is imported from the library.

The model restates the header of cn_chess_ai_amd/csrc/xq_refine.hip.h.  With u = 2^-8 (bf16, round to nearest even):
    z~_j  = sum_k bf16(W_jk) bf16(a_k) + b_j                     the screened value (here in fp64 from the rounded operands: the fp32
                                                                 accumulation and the 5-bit position tag move it by < 2^-13 of B)
    B     = kScreenEps ||a|| max_j ||W_j|| + kScreenBiasEps max_j |b_j|
    thr   = m~ - 2 B (1 + 2^-5) - 2^-16 (|m~| + 2 B),   m~ = max_j z~_j
    every 32-row group (screen_row) whose largest z~ reaches thr is a candidate: its largest row alone, or all of its rows when its second
    value reaches thr too; the result is the largest fp32-evaluated z over the candidate rows (here: the fp64 z).
||a|| is taken from the bf16 activations where screen_top2_kernel runs (256- and 512-wide last hidden layers, qmax_refine2_kernel) and from
the fp32 ones otherwise (qmax_refine_kernel); max_j ||W_j|| and max_j |b_j| are kept for rows 0..95 (written again every step) and for rows
>= 96 (kept while the net stands) and the larger of the two is used.

`damage` switches break the model one rule at a time, for the negative controls of tests/test_screen_ref_cpu.py:
    "half_window"  threshold m~ - B instead of m~ - 2B          "eps_0.8"     kScreenEps * 0.8 (any "eps_<factor>")
    "neighbour"    ||a|| of sample i ^ 1                        "static_only" row-norm / bias maxima over rows >= 96 only
    "no_whole"     a group's largest row only, whatever its second value

The construction (build) is described at its builder below and in DESIGN.md §2.
"""
from collections import namedtuple

import numpy as np

K_SCREEN_EPS = 2.0 ** -7 * 1.0625          # kScreenEps, xq_refine.hip.h
K_SCREEN_BIAS_EPS = 2.0 ** -9              # kScreenBiasEps, xq_refine.hip.h
THR_REEVAL = 1.0 + 2.0 ** -5               # the share of the window reserved for the rounding of the fp32 re-evaluation
THR_TAG = 2.0 ** -16                       # the 5-bit position tag at both ends
DYN_ROWS = 96                              # rows 0..95: the dynamic slots wm[parity], wm[2 + parity]; the rest: wm[4], wm[5]
TANH_HIDDEN_REL = 6e-6                     # relative error of tanh_hidden as its comment in xq_gemm.hip.h documents it
GAMMA = float(np.float32(0.99))            # the discount the handles of the tests are made with, as the device holds it
Y_BAR = 2e-6                               # |y_screened - y_full|: the bar of the screen tests of tests/test_dqn_gpu.py
NO = 8100
T_EDGE = 1.0 / 64                          # distance of the constructed operands from the bf16 rounding midpoint, in half-ulps


def bf16_rne(x):
    """x -> fp32 -> bf16 (round to nearest even), as float64: what screen_shadow_block and the activation producers store"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32).astype(np.float64).reshape(np.shape(x))


def f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def screen_row(g, code):
    """row of position `code` (0..31) of group g: the inverse of the CM_TOP2 position code (screen_row, xq_refine.hip.h)"""
    q = code & 15
    return (g >> 2) * 128 + ((g >> 1) & 1) * 64 + 4 * (g & 1) + (code >> 4) * 32 + (q & 3) + 8 * (q >> 2)


def group_rows(no):
    """[G][32] rows of every group that holds a real row (G = 2 * ceil(no / 64)); entries >= no are padding"""
    G = 2 * ((no + 63) // 64)
    g, c = np.meshgrid(np.arange(G), np.arange(32), indexing="ij")
    return screen_row(g, c)


def group_of(row):
    rows = group_rows(row + 1)
    return int(np.nonzero((rows == row).any(axis=1))[0][0])


Screened = namedtuple("Screened", "zmax kept pairs whole B m thr zt z")


def screen(W, b, A, na_bf16, damage=None):
    """The screened maximum of every sample.  W [NO][K], b [NO]: the output layer as the device holds it (fp32 values); A [m][K]: the
    last hidden activations (fp32 values).  Returns Screened: zmax [m] the fp64 maximum over the candidate rows, kept [m] lists of
    candidate rows, pairs / whole [m] candidate groups and those among them taken whole, B, m~, thr [m], zt / z [m][NO]."""
    W, b, A = f32(W), f32(b), f32(A)
    no = W.shape[0]
    z = A @ W.T + b
    zt = bf16_rne(A) @ bf16_rne(W).T + b
    rows = group_rows(no)
    pad = rows >= no
    v = np.where(pad[None], -np.inf, zt[:, np.minimum(rows, no - 1)])             # [m][G][32]
    order = np.argsort(-v, axis=2, kind="stable")
    top = np.take_along_axis(v, order[:, :, :2], axis=2)
    p1, p2, first = top[:, :, 0], top[:, :, 1], order[:, :, 0]
    eps = K_SCREEN_EPS * (float(damage[4:]) if damage and damage.startswith("eps_") else 1.0)
    wn = np.sqrt((W * W).sum(axis=1))
    lo = 0 if damage != "static_only" else DYN_ROWS
    wmx, bmx = wn[lo:].max(initial=0.0), np.abs(b[lo:]).max(initial=0.0)
    na = np.sqrt(((bf16_rne(A) if na_bf16 else A) ** 2).sum(axis=1))
    if damage == "neighbour":
        na = na[np.minimum(np.arange(len(na)) ^ 1, len(na) - 1)]
    B = eps * na * wmx + K_SCREEN_BIAS_EPS * bmx
    m = p1.max(axis=1)
    window = B if damage == "half_window" else 2.0 * B
    thr = m - window * THR_REEVAL - THR_TAG * (np.abs(m) + window)
    zmax, kept, pairs, whole = [], [], [], []
    for i in range(len(A)):
        cand = p1[i] >= thr[i]
        wh = cand & (p2[i] >= thr[i]) if damage != "no_whole" else np.zeros_like(cand)
        ks = [int(rows[g, first[i, g]]) for g in np.nonzero(cand & ~wh)[0]]
        for g in np.nonzero(wh)[0]:
            ks += [int(r) for r in rows[g] if r < no]
        kept.append(ks)
        zmax.append(z[i, ks].max())
        pairs.append(int(cand.sum()))
        whole.append(int(wh.sum()))
    return Screened(np.array(zmax), kept, np.array(pairs), np.array(whole), B, m, thr, zt, z)


# ---- the construction ---------------------------------------------------------------------------------------------------------------------
# A case: the last hidden width, the batch, how the bf16 activation operand is produced ("gather": 1260-Hl-8100, the layer-0 gather writes it;
# "product": 1260-64-Hl-8100, the hidden product's epilogue does), the rows of the true maximum and of its rival, the selecting net, the
# switches of the handle (tail: the TD arithmetic rides in the refine blocks; huber), and the two variants of the output layer.
Case = namedtuple("Case", "family Hl n net jstar rival td_net tail huber biased low_static")

N_CLASSES = 8
GENERALS = ((4, 1), (85, 8))               # (square, piece code): the two generals every board holds; their rows of W0 are zero


def marker(q):
    """(square, piece code) of class q's marker"""
    return 30 + 3 * q, 5 if q < 4 else 12


def class_scale(q):
    return 2.0 ** -(q % 4)


def class_of_sample(n):
    """classes alternate sample by sample: every 32-sample MFMA tile and every 32-sample refine block holds all of them"""
    return np.arange(n) % N_CLASSES


def sizes_of(c):
    return [1260, c.Hl, NO] if c.net == "gather" else [1260, 64, c.Hl, NO]


Built = namedtuple("Built", "sizes w b w_decoy boards cls a W bout z wa")


def pattern(K):
    """Class 0's activations a0 [K] and the weight magnitudes wmag [K] (times 2^-4 in the main family), sgn [K] the signs of row j*.
    Columns 2p (half A) and 2p + 1 (half B) share the exponent e = 2 + (p & 1); the last two columns are the exact ones.
    Half A: a = 2^-e (1 + 2^-8 (1 - t)) rounds DOWN to bf16 by (1 - t) half-ulps, half B: 2^-e (1 + 2^-8 (1 + t)) rounds UP by as much;
    the weight magnitudes are 2^-4 times the same numbers, so every operand of half A shrinks and every one of half B grows.  Row j* = +|w|
    on A, -|w| on B: every term of its screened value errs DOWN by ~2u |w a|; the rival is its negative: every term errs UP."""
    assert K % 2 == 0 and K >= 8
    k = np.arange(K - 2)
    e = 2 + ((k // 2) & 1)
    halfB = (k & 1) == 1
    mant = 1.0 + 2.0 ** -8 * np.where(halfB, 1.0 + T_EDGE, 1.0 - T_EDGE)
    a0 = np.concatenate([2.0 ** -e * mant, [0.25, 0.25]])
    wmag = np.concatenate([2.0 ** -e * mant, [0.0, 0.0]])
    sgn = np.concatenate([np.where(halfB, -1.0, 1.0), [0.0, 0.0]])
    return a0, wmag, sgn


_built = {}


def build(c):
    """Parameter vectors (reference flat layout: layer l's weights [L[l+1]][L[l]] row-major, then the biases layer by layer) of the case's
    net and of a decoy for the net that does NOT select (the same net with the output weights halved), the boards, and per class the
    intended activations a [8][K], the fp64 pre-activations z [8][NO] of the output layer on them and wa [8] = sum_k |W_j*k a_k|."""
    key = (c.Hl, c.net, c.jstar, c.rival, c.biased, c.low_static)
    if key in _built:
        sizes, w, b, w_decoy, a, W, bout, z, wa = _built[key]
    else:
        K = c.Hl
        a0, wmag, sgn = pattern(K)
        wscale = 1.0 if c.biased else 2.0 ** -4          # (biased: larger weights, so that the bias term stays a few per cent of B)
        rng = np.random.default_rng(K * 131 + c.jstar)
        f = rng.uniform(0.3, 0.5, NO)                     # every other row: -f |a|-aligned, at most half the norm, z clearly negative
        W = -f[:, None] * (wscale * wmag)[None, :]
        if c.low_static:
            W[DYN_ROWS:] *= 0.1                           # rows >= 96 at a tenth of the norm: the dynamic slot alone carries the bound
        W[c.jstar] = wscale * wmag * sgn
        W[c.rival] = -wscale * wmag * sgn
        bout = np.zeros(NO)
        if c.biased:
            bout = -rng.uniform(0.01, 0.06, NO)
            bout[rng.integers(0, NO)] = -0.06
            bout[c.jstar] = bout[c.rival] = 0.05
        # the lift of j* over the rival through the exact columns: z_j* - z_J = 0.1 B_w on class 0 (B_w: the weight part of B)
        Bw = K_SCREEN_EPS * np.linalg.norm(a0) * np.linalg.norm(W[c.jstar])
        need = (0.1 * Bw - 2.0 * (W[c.jstar] @ a0)) / 0.25
        g1 = float(bf16_rne(need / 2))
        W[c.jstar, K - 2], W[c.jstar, K - 1] = g1, float(bf16_rne(need - g1))
        W = f32(W)
        bout = f32(bout)
        a = np.stack([a0 * class_scale(q) for q in range(N_CLASSES)])
        z = a @ W.T + bout
        wa = np.abs(W[c.jstar][None, :] * a).sum(axis=1)
        pre = np.arctanh(a)                               # the hidden pre-activations that produce a
        if c.net == "gather":
            sizes = [1260, K, NO]
            W0 = np.zeros((K, 1260))
            for q in range(N_CLASSES):
                sq, pc = marker(q)
                W0[:, sq * 14 + pc - 1] = pre[q]
            hidden_w, nb = [W0.ravel()], K
        else:
            sizes = [1260, 64, K, NO]
            W0 = np.zeros((64, 1260))
            W1 = np.zeros((K, 64))
            for q in range(N_CLASSES):
                sq, pc = marker(q)
                W0[q, sq * 14 + pc - 1] = 20.0            # tanh_hidden(20) = 1.0f, tanh_hidden(0) = 0: an exact one-hot of the class
                W1[:, q] = pre[q]
            hidden_w, nb = [W0.ravel(), W1.ravel()], 64 + K
        w = np.concatenate(hidden_w + [W.ravel()])
        w_decoy = np.concatenate(hidden_w + [0.5 * W.ravel()])
        b = np.concatenate([np.zeros(nb), bout])
        _built.clear()                                    # (one net at a time: 8100 x 1024 doubles each)
        _built[key] = (sizes, w, b, w_decoy, a, W, bout, z, wa)
    cls = class_of_sample(c.n)
    boards = np.zeros((c.n, 90), np.uint8)
    for sq, pc in GENERALS:
        boards[:, sq] = pc
    for q in range(N_CLASSES):
        sq, pc = marker(q)
        boards[cls == q, sq] = pc
    return Built(sizes, w, b, w_decoy, boards, cls, a, W, bout, z, wa)


def na_from_bf16(c):
    """screen_top2_kernel (Hl = 256, 512) hands the refine kernel the norm of the bf16 activations"""
    return c.Hl in (256, 512)


def jittered(a, seed):
    """the activations the device may hold instead of the intended ones: tanh_hidden's documented error"""
    return a * (1.0 + np.random.default_rng(seed).uniform(-TANH_HIDDEN_REL, TANH_HIDDEN_REL, a.shape))


def depth(c, seed=None, bt=None):
    """(m~ - z~_j*) / (2 B) per class: how far down the candidate window the true maximum sits; > 1 + 2^-5 and it is lost"""
    bt = bt or build(c)
    A = bt.a if seed is None else jittered(bt.a, seed)
    s = screen(bt.W, bt.bout, A, na_from_bf16(c))
    return (s.m - s.zt[:, c.jstar]) / (2.0 * s.B)


def y_bar(bt):
    """per class: the bar on |y - (r + gamma tanh z_max)| against fp64: the bar of the screen tests plus tanh_hidden's documented error
    carried through the winning row"""
    return Y_BAR + GAMMA * TANH_HIDDEN_REL * bt.wa
