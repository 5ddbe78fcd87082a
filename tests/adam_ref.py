"""fp64 restatement of the Adam step of xq_dqn_apply_grads (include/xq_capi.h, xq_dqn_set_optimizer; DESIGN.md section 4 "Optimizer")
and the error bounds the device is held to.  Test infrastructure only, like batch_ref.py: tests import it, the product never does.

The rule is torch.optim.Adam's (amsgrad off, no weight decay), at the t-th apply since the state was reset (t starts at 1):

    g' = grad_scale * g
    m  = beta1 m + (1 - beta1) g'
    v  = beta2 v + (1 - beta2) g'^2
    p  = p - (lr / (1 - beta1^t)) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)

tests/test_adam_ref_cpu.py pins step() to torch.optim.Adam (float64) to 1e-12 over 50 steps.

Rounding bound of ONE device step (one_step_bound) started from the device's own read-back state (p0, m0, v0) and an exactly known fp32
gradient, with u = 2^-24, to first order in u:

    |dm| <= K u (beta1 |m0| + (1 - beta1) |g'|)
    |dv| <= K u (beta2 v0 + (1 - beta2) g'^2)
    |dp| <= a (|dm| / den + |m| |dden| / den^2) + K u |step| + ulp32(p) / 2
            a = lr / (1 - beta1^t),  den = sqrt(v) / sqrt(1 - beta2^t) + eps,  |dden| = |dv| carried through the square root

K = 8 covers the operation count: at most 8 rounded fp32 operations or constants on any chain (grad_scale, g' , 1 - beta, the product,
beta, the fused multiply-add; a, the quotient, the final fused multiply-add), square root and division correctly rounded (hipcc's
default for HIP, and the Makefile passes nothing that relaxes it).

That model, fl(x op y) = (x op y)(1 + d) with |d| <= u, holds while no result underflows.  The gradients the tests inject reach down
to the subnormal range on purpose, and there fp32 rounds to a multiple of 2^-149 instead: |fl(x op y) - x op y| <= 2^-150 absolutely
(the standard model with underflow, Higham, "Accuracy and Stability of Numerical Algorithms", section 2.2).  So |dm| and |dv| each get
K * 2^-150 added, a property of the number format, not of the code under test; it is below 1e-44 and vanishes against the relative
terms for every value above ~1e-37.  |dp| takes it through |dm| and |dden| and gets none of its own (p is O(1e-2)).
"""
import numpy as np

U32 = 2.0 ** -24                 # unit roundoff of fp32
ETA32 = 2.0 ** -150              # half the spacing of the fp32 subnormals
K = 8
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8


def step(p, m, v, g, t, lr, grad_scale=1.0, beta1=BETA1, beta2=BETA2, eps=EPS, bias_correction=True, eps_inside_sqrt=False):
    """(p, m, v) after the t-th step, all float64.  The two switches exist for the negative controls only."""
    p, m, v, g = (np.asarray(x, dtype=np.float64) for x in (p, m, v, g))
    gp = grad_scale * g
    m = beta1 * m + (1.0 - beta1) * gp
    v = beta2 * v + (1.0 - beta2) * gp * gp
    bc1 = 1.0 - beta1 ** t if bias_correction else 1.0
    bc2 = 1.0 - beta2 ** t if bias_correction else 1.0
    if eps_inside_sqrt:
        den = np.sqrt(v / bc2 + eps)
    else:
        den = np.sqrt(v) / np.sqrt(bc2) + eps
    return p - (lr / bc1) * m / den, m, v


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64).astype(np.float32))).astype(np.float64)


def one_step_bound(p0, m0, v0, g, t, lr, grad_scale=1.0, beta1=BETA1, beta2=BETA2, eps=EPS):
    """((p, m, v) of the fp64 step, (bound_p, bound_m, bound_v)) for one device step from (p0, m0, v0) with the fp32 gradient g."""
    p0, m0, v0, g = (np.asarray(x, dtype=np.float64) for x in (p0, m0, v0, g))
    p, m, v = step(p0, m0, v0, g, t, lr, grad_scale, beta1, beta2, eps)
    gp = grad_scale * g
    bm = K * U32 * (beta1 * np.abs(m0) + (1.0 - beta1) * np.abs(gp)) + K * ETA32
    bv = K * U32 * (beta2 * v0 + (1.0 - beta2) * gp * gp) + K * ETA32
    a = lr / (1.0 - beta1 ** t)
    rbc2 = 1.0 / np.sqrt(1.0 - beta2 ** t)
    sq = np.sqrt(v)
    # |sqrt(v + dv) - sqrt(v)|: dv / (2 sqrt v) to first order, and never more than sqrt(|dv|)
    with np.errstate(divide="ignore", invalid="ignore"):
        dsq = np.minimum(np.sqrt(bv), np.where(sq > 0, bv / (2.0 * sq), np.inf))
    den = sq * rbc2 + eps
    dden = rbc2 * dsq
    st = a * m / den
    bp = a * (bm / den + np.abs(m) * dden / (den * den)) + K * U32 * np.abs(st) + 0.5 * ulp32(p)
    return (p, m, v), (bp, bm, bv)


def gradient_error_bound(m0, v0, gp_ref, E, t, lr, beta1=BETA1, beta2=BETA2, eps=EPS):
    """How far the step S(g') = a m / den moves when the scaled gradient is only known to |g' - gp_ref| <= E (E >= 0, per element):

        |dS| <= a E ((1 - beta1) / den_min + |m|_max sqrt((1 - beta2) / (1 - beta2^t)) / den_min^2)

    dm/dg' = 1 - beta1.  dden/dg' = (1 - beta2) g' / (sqrt(v) sqrt(1 - beta2^t)), and v >= (1 - beta2) g'^2 gives
    |dden/dg'| <= sqrt((1 - beta2) / (1 - beta2^t)).  den_min and |m|_max are taken over the whole interval: den is smallest where
    |g'| is (max(0, |gp_ref| - E)), |m| is at most beta1 |m0| + (1 - beta1)(|gp_ref| + E)."""
    m0, v0, gp_ref, E = (np.asarray(x, dtype=np.float64) for x in (m0, v0, gp_ref, E))
    a = lr / (1.0 - beta1 ** t)
    bc2 = 1.0 - beta2 ** t
    g_lo = np.maximum(0.0, np.abs(gp_ref) - E)
    den_min = np.sqrt(beta2 * v0 + (1.0 - beta2) * g_lo * g_lo) / np.sqrt(bc2) + eps
    m_max = beta1 * np.abs(m0) + (1.0 - beta1) * (np.abs(gp_ref) + E)
    return a * E * ((1.0 - beta1) / den_min + m_max * np.sqrt((1.0 - beta2) / bc2) / (den_min * den_min))


# ---- the layout of the gradient buffer / the two state buffers (xq_dqn.hip layout_td_grads) -------------------------------------
def layout(sizes):
    """dict of offsets into the compact buffer: gW0^T [L0][L1], hidden gW_l [out][in], gW_out rows 0..95, gb_out[96], hidden biases."""
    L, nl = list(sizes), len(sizes) - 1
    off, lay = 0, {}
    lay["w0"] = off; off += L[0] * L[1]
    lay["wh"] = {}
    for l in range(1, nl - 1):
        lay["wh"][l] = off; off += L[l] * L[l + 1]
    lay["wout"] = off; off += 96 * L[nl - 1]
    lay["bout"] = off; off += 96
    lay["bh"] = off; off += sum(L[1:nl])
    lay["n"] = off
    return lay


def to_reference(sizes, buf, fill=0.0):
    """A compact buffer as (weights, biases) in the reference flat layout (row-major [out][in] per layer); what it does not cover
    (output rows >= 96) is `fill`."""
    L, nl = list(sizes), len(sizes) - 1
    lay = layout(sizes)
    buf = np.asarray(buf)
    assert buf.size == lay["n"]
    nw = sum(L[l] * L[l + 1] for l in range(nl))
    nb = sum(L[1:])
    w, b = np.full(nw, fill, dtype=buf.dtype), np.full(nb, fill, dtype=buf.dtype)
    o = L[0] * L[1]
    w[:o] = buf[:o].reshape(L[0], L[1]).T.reshape(-1)
    for l in range(1, nl - 1):
        k = L[l] * L[l + 1]
        w[o:o + k] = buf[lay["wh"][l]:lay["wh"][l] + k]
        o += k
    w[o:o + 96 * L[nl - 1]] = buf[lay["wout"]:lay["wout"] + 96 * L[nl - 1]]
    nh = sum(L[1:nl])
    b[:nh] = buf[lay["bh"]:lay["bh"] + nh]
    b[nh:nh + 96] = buf[lay["bout"]:lay["bout"] + 96]
    return w, b


def covered(sizes):
    """(mask over weights, mask over biases): the parameters the compact buffer covers."""
    w, b = to_reference(sizes, np.ones(layout(sizes)["n"], dtype=np.float64))
    return w > 0, b > 0
