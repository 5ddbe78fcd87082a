"""fp64 restatement of the gradient clipping of xq_dqn_apply_grads (include/xq_capi.h, xq_dqn_set_grad_clip; DESIGN.md section 4
"Gradient clipping") and the error bounds the device is held to.  Test infrastructure only, like adam_ref.py: tests import it, the
product never does.

With g the summed gradient about to be applied (every entry of the gradient buffer's layout):

    S    = sum_i g_i^2                                   (exactly rounded here: math.fsum of fp64 squares)
    norm = |grad_scale| sqrt(S)
    c    = min(1, max_norm / (norm + 1e-6))              torch.nn.utils.clip_grad_norm_'s coefficient
    SGD : p -= lr grad_scale c g
    Adam: adam_ref.step with the gradient scale grad_scale c

tests/test_clip_ref_cpu.py pins this to clip_grad_norm_ + torch.optim.SGD / Adam in float64.

One device step, u = 2^-24.  SGD computes p - fl32(fl32(lr grad_scale) fl32(c)) g: c rounded to fp32, the product alpha c, the product
with g and the subtraction are four roundings, the first three relative to the step, the last at most one ulp of the larger of p
before and after:

    |p_dev - (p0 - step)| <= 4 u |step| + ulp32(max(|p0|, |p1|)),     step = lr grad_scale c g in fp64

Adam: adam_ref.one_step_bound with the gradient scale grad_scale c covers everything but the two extra roundings of that scale (c to
fp32, the product grad_scale c): g' is off by at most E = 2 u |g'| more, which moves m by (1 - beta1) E, v by (1 - beta2)(2 |g'| E + E^2)
and the step by adam_ref.gradient_error_bound(E); the three are added to the bounds.
"""
import math

import numpy as np

import adam_ref as ar

U32 = ar.U32
EPS_NORM = 1e-6


def norm(g, grad_scale=1.0):
    g = np.asarray(g, dtype=np.float64).reshape(-1)
    return abs(float(grad_scale)) * math.sqrt(math.fsum((g * g).tolist()))


def coef_of_norm(nrm, max_norm):
    return min(1.0, float(max_norm) / (nrm + EPS_NORM))


def coef(g, max_norm, grad_scale=1.0):
    return coef_of_norm(norm(g, grad_scale), max_norm)


def sgd_step(p, g, lr, grad_scale, c):
    return np.asarray(p, dtype=np.float64) - lr * grad_scale * c * np.asarray(g, dtype=np.float64)


def adam_step(p, m, v, g, t, lr, grad_scale, c, **kw):
    return ar.step(p, m, v, g, t, lr, grad_scale * c, **kw)


def sgd_one_step_bound(p0, g, lr, grad_scale, c):
    """(p of the fp64 step, bound) for one device SGD step from p0 with the fp32 gradient g and the fp64 coefficient c."""
    p0, g = np.asarray(p0, dtype=np.float64), np.asarray(g, dtype=np.float64)
    step = lr * grad_scale * c * g
    p1 = p0 - step
    return p1, 4.0 * U32 * np.abs(step) + ar.ulp32(np.maximum(np.abs(p0), np.abs(p1)))


def adam_one_step_bound(p0, m0, v0, g, t, lr, grad_scale, c, beta1=ar.BETA1, beta2=ar.BETA2, eps=ar.EPS):
    """((p, m, v) of the fp64 step, (bound_p, bound_m, bound_v)): adam_ref's bound at the scale grad_scale c, widened by that scale's
    two extra roundings."""
    gs = grad_scale * c
    ref, (bp, bm, bv) = ar.one_step_bound(p0, m0, v0, g, t, lr, gs, beta1, beta2, eps)
    gp = np.abs(gs * np.asarray(g, dtype=np.float64))
    E = 2.0 * U32 * (1.0 + U32) * gp
    bp = bp + ar.gradient_error_bound(m0, v0, gp, E, t, lr, beta1, beta2, eps)
    bm = bm + (1.0 - beta1) * E
    bv = bv + (1.0 - beta2) * (2.0 * gp * E + E * E)
    return ref, (bp, bm, bv)
