"""fp64 restatement of the soft (Polyak) target update and the rounding bound of the device's fp32 step (DESIGN.md section 4
"Soft target update").

Device, per parameter, with tau32 = float32(tau), p the online value the apply has just produced and t the target value, all fp32:
    d  = fl32(p - t)
    t' = fma(tau32, d, t)                          one rounding
Reference: t'_ref = t + tau32 (p - t), evaluated in fp64 from the fp32 inputs (torch.lerp's formula for weights below 0.5).

One-step bound (derived, not measured).  With u = 2^-24 the unit roundoff of fp32, d = (p - t)(1 + e1) and
t' = (tau32 d + t)(1 + e2), |e1|, |e2| <= u, so
    t' - t'_ref = tau32 (p - t) e1 + (t'_ref + tau32 (p - t) e1) e2
    |t' - t'_ref| <= u (tau32 |p - t| + |t'_ref|) + u^2 tau32 |p - t|.
The factor (1 + 2^-20) covers the second-order term and the rounding of the fp64 evaluation itself; one fp32 subnormal (2^-149) covers a
result in the subnormal range, where the fma's error is absolute (half a subnormal spacing) instead of relative.  A difference p - t in
the subnormal range is exact.  p == t gives d = 0 and t' == t: the bound is then u |t| although the error is 0.  (In bits too, with one
exception that is none in value: t = p = -0 gives d = +0 and t' = +0.)

K steps: the recursion is linear in t with factor (1 - tau32) in [0, 1], so an error already made is never amplified; the device's error
after step k is at most the sum of the one-step bounds of steps 1..k, each taken at the target value the device itself started that step
from (`budget`).
"""
import numpy as np

U = 2.0 ** -24
SUBNORMAL = 2.0 ** -149


def tau32(tau):
    return np.float32(tau)


def _f64_of_f32(x):
    a = np.asarray(x)
    assert a.dtype == np.float32 or np.array_equal(a.astype(np.float32).astype(np.float64), a.astype(np.float64)), "inputs must be fp32 values"
    return a.astype(np.float64)


def step(t, p, tau_32):
    """t + tau32 (p - t) in fp64; t, p: fp32 values (as float32 or as float64 arrays that hold fp32 values)"""
    assert isinstance(tau_32, np.float32)
    t, p = _f64_of_f32(t), _f64_of_f32(p)
    return t + float(tau_32) * (p - t)


def one_step_bound(t, p, tau_32):
    """(t'_ref, bound): |t'_dev - t'_ref| <= bound for the device's fp32 step from (t, p)"""
    ref = step(t, p, tau_32)
    t, p = _f64_of_f32(t), _f64_of_f32(p)
    bound = U * (float(tau_32) * np.abs(p - t) + np.abs(ref)) * (1.0 + 2.0 ** -20) + SUBNORMAL
    return ref, bound


def fp32_step(t, p, tau_32):
    """numpy emulation of the device step: the difference rounded to fp32, then the fma (its product is exact in fp64, the sum is rounded
    to fp64 and then to fp32: within 2^-29 relative of the singly rounded fma)"""
    t32, p32 = np.asarray(t, dtype=np.float32), np.asarray(p, dtype=np.float32)
    with np.errstate(under="ignore"):
        d = (p32 - t32).astype(np.float32)
        return (float(tau_32) * d.astype(np.float64) + t32.astype(np.float64)).astype(np.float32)


class Budget:
    """K-step budget: ref follows the fp64 recursion over the online snapshots, bound accumulates the one-step bounds taken at the
    device's own target values."""

    def __init__(self, t0):
        self.ref = _f64_of_f32(t0).copy()
        self.bound = np.zeros_like(self.ref)

    def advance(self, t_dev_before, p_new, tau_32):
        self.ref = step_f64(self.ref, p_new, tau_32)
        self.bound = self.bound + one_step_bound(t_dev_before, p_new, tau_32)[1]
        return self.ref, self.bound


def step_f64(t_ref, p, tau_32):
    """the fp64 recursion itself: t_ref is a running fp64 value (not an fp32 one), p an fp32 snapshot"""
    return np.asarray(t_ref, dtype=np.float64) + float(tau_32) * (_f64_of_f32(p) - np.asarray(t_ref, dtype=np.float64))
