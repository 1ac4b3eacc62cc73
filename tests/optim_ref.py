"""Plain numpy restatements of one AdamW step, for tests/test_hip_optim.py.  No torch, no device code.

Both work on 1-D arrays in STORAGE order (the optimizer is elementwise, so the memory layout of a tensor does not matter):

``scalars`` + ``step32``   csrc/optim.hip restated operation for operation: the seven float32 scalars the host binding
                           ``t2h_adamw_flat_step`` derives (double arithmetic, rounded once), then the five lines of
                           ``adam_one``, one numpy float32 operation per device operation in the same order.  numpy's float32
                           ``+ - * / sqrt`` are correctly rounded and keep subnormals, which is what the kernel's header
                           promises (``__f*_rn``, no contraction), so the kernel is held to this BIT FOR BIT.
``step64``                 torch/optim/adam.py ``_single_tensor_adam`` (decoupled decay, amsgrad = maximize = False) in
                           float64 with nothing rounded to float32 in between; the caller carries float64 state over steps.
"""
import math

import numpy as np

F32 = np.float32


def scalars(lr, beta1, beta2, eps, weight_decay, step):
    """(decay, 1 - beta1, beta2, 1 - beta2, -(lr / bc1), sqrt(bc2), eps) as float32, the fields of ``AdamScalars``."""
    lr, beta1, beta2, eps, weight_decay = float(lr), float(beta1), float(beta2), float(eps), float(weight_decay)
    bc1 = 1.0 - math.pow(beta1, float(step))
    bc2 = 1.0 - math.pow(beta2, float(step))
    return (F32(1.0 - lr * weight_decay), F32(1.0 - beta1), F32(beta2), F32(1.0 - beta2), F32(-(lr / bc1)),
            F32(math.sqrt(bc2)), F32(eps))


def step32(p, g, m, v, scalars):
    """One step on float32 arrays; returns new (p, m, v).  The inputs are left unchanged."""
    decay, one_minus_beta1, beta2, one_minus_beta2, neg_step_size, bc2_sqrt, eps = (F32(s) for s in scalars)
    p, g, m, v = (np.asarray(a, dtype=F32) for a in (p, g, m, v))
    with np.errstate(all="ignore"):
        p = p * decay
        m = m + one_minus_beta1 * (g - m)
        v = v * beta2 + (one_minus_beta2 * g) * g
        denom = np.sqrt(v) / bc2_sqrt + eps
        p = p + neg_step_size * (m / denom)
    assert p.dtype == F32 and m.dtype == F32 and v.dtype == F32
    return p, m, v


def step64(p, g, m, v, lr, betas, eps, wd, step):
    """One step in float64; returns new (p, m, v) as float64 arrays."""
    beta1, beta2 = betas
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    with np.errstate(all="ignore"):
        p = p * (1 - lr * wd)
        m = m + (1 - beta1) * (g - m)                       # Tensor.lerp_, weight < 0.5
        v = v * beta2 + (1 - beta2) * g * g                 # mul_ then addcmul_
        step_size = lr / (1 - beta1 ** step)
        bc2_sqrt = (1 - beta2 ** step) ** 0.5
        denom = np.sqrt(v) / bc2_sqrt + eps
        p = p + (-step_size) * (m / denom)                  # addcdiv_
    return p, m, v


def same_floats(a, b):
    """Byte equality of two float32 arrays, except that a NaN only has to meet a NaN (payload and sign are free)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != F32 or b.dtype != F32 or a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def first_mismatches(a, b, k=8):
    """Storage positions of the first elements that ``same_floats`` objects to (for assertion messages)."""
    na, nb = np.isnan(a), np.isnan(b)
    bad = (na != nb) | (~na & ~nb & (a.view(np.uint32) != b.view(np.uint32)))
    idx = np.nonzero(bad)[0]
    return [(int(i), float(a[i]), float(b[i])) for i in idx[:k]], int(idx.size)
