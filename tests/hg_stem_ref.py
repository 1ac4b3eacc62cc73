"""The stride-2 convolution's two adjoints restated in plain torch, their derived error bars, and the cases of the stem-gradient
fixture (tests/golden/make_golden_hourglass_stem_grad.py -> tests/golden/hourglass_stem_grad*.npz).

Adjoints (include/t2h_hg.h: t2h_hg_conv_s2_dgrad / t2h_hg_conv_s2_wgrad).  ``dgrad_by_parity`` writes the data gradient the way the
kernel computes it: the input pixels are cut into four classes by the parities (py, px) of (iy + pad, ix + pad); a pixel of
class (py, px) with q = (iy + pad) // 2 meets only the kernel rows ky = py + 2 a, at the output row q - a -- a stride-1
convolution of gy with every second tap.  ``wgrad_by_taps`` sums x over the strided window of each tap.

Bars.  Any summation order of n rounded products (or of fused multiply-adds) stays within gamma_n sum|terms| of the exact sum,
gamma_n = n u / (1 - n u) <= (n + 1) u with u = 2^-24 while n (n + 1) u <= 1 (n <= 4095): ``bars`` evaluates that elementwise in
float64.  With an addend the sum has one more term and one more rounding: (m + 2) u (sum|gy| |w| + |addend|).
"""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

import hg_grad_ref
import hg_ref

U = 2.0 ** -24

# (B, Cin, H, W, Cout, K, pad): the smallest shapes that exercise every seam of the two kernels
KERNEL_SHAPES = (
    (2, 3, 18, 22, 64, 7, 3),          # the stem: OH x OW = 9 x 11, two partly filled 8 x 8 output tiles each way
    (2, 3, 17, 16, 64, 7, 3),          # odd H; W + 2 pad - K odd: the last column meets only some taps
    (2, 128, 10, 6, 128, 3, 1),        # down_conv2: lanes over channels, two 64-channel tiles both ways
    (2, 128, 16, 16, 128, 3, 1),
    (1, 5, 7, 9, 64, 3, 0),            # ragged Cin, no padding
    (1, 5, 8, 10, 64, 3, 0),           # ... and a last row and column that no tap reaches
    (2, 8, 5, 6, 64, 1, 0),            # K = 1
    (1, 20, 9, 8, 64, 5, 2),           # K = 5: a ragged 64-channel tile (20 of 64), input-channel chunks of 6, 6, 6, 2
    (1, 4, 34, 6, 64, 3, 1),           # OH = 17: three slabs of 8 output rows per sample
)
BAD_ARGUMENTS = (                      # (B, Cin, H, W, Cout, K, pad) outside the domain of t2h_hg_conv_s2_fwd
    (1, 3, 8, 8, 64, 4, 1), (1, 3, 8, 8, 64, 9, 4), (1, 3, 8, 8, 64, 3, 2), (1, 3, 8, 8, 60, 3, 1), (1, 3, 8, 8, 32, 3, 1),
    (1, 0, 8, 8, 64, 3, 1), (1, 3, 2, 8, 64, 7, 2), (0, 3, 8, 8, 64, 3, 1), (1, 3, 8, 8, 64, 3, -1),
)


def out_size(n, k, pad):
    return (n + 2 * pad - k) // 2 + 1


def kernel_case(shape, seed=0):
    """(x, weight [Cout, Cin, K, K], bias, gy, addend) of a kernel shape, float32, seeded by the shape."""
    b, cin, h, w, cout, k, pad = shape
    g = torch.Generator().manual_seed((zlib.crc32(repr(shape).encode()) + seed) % (2 ** 31))
    x = torch.randn(b, cin, h, w, generator=g)
    weight = torch.randn(cout, cin, k, k, generator=g) / (k * k * cin) ** 0.5
    bias = torch.randn(cout, generator=g)
    gy = torch.randn(b, cout, out_size(h, k, pad), out_size(w, k, pad), generator=g)
    addend = torch.randn(b, cin, h, w, generator=g)
    return x, weight, bias, gy, addend


def autograd_adjoints(x, weight, gy, pad, dtype):
    """(dx, dw, dbias) of sum(F.conv2d(x, weight, bias, stride=2, padding=pad) * gy) in ``dtype`` by torch's autograd on the host."""
    x, weight = (t.detach().to(dtype).clone().requires_grad_(True) for t in (x, weight))
    bias = torch.zeros(weight.shape[0], dtype=dtype, requires_grad=True)
    (F.conv2d(x, weight, bias, stride=2, padding=pad) * gy.to(dtype)).sum().backward()
    return x.grad, weight.grad, bias.grad


def dgrad_by_parity(gy, weight, h, w, pad):
    """dx [B, Cin, H, W] from gy [B, Cout, OH, OW] and weight [Cout, Cin, K, K], class by class."""
    b, cout, oh, ow = gy.shape
    cin, k = weight.shape[1], weight.shape[2]
    a_n = (k + 1) // 2
    nqy, nqx = (h + pad - 1) // 2 + 1, (w + pad - 1) // 2 + 1
    g = gy.new_zeros(b, cout, nqy + a_n - 1, nqx + a_n - 1)          # gy with a_n - 1 zeros in front and zeros behind: row q - a + a_n - 1
    g[:, :, a_n - 1:a_n - 1 + oh, a_n - 1:a_n - 1 + ow] = gy
    dx = gy.new_zeros(b, cin, h, w)
    for py in (0, 1):
        qy = [q for q in range(nqy) if 0 <= 2 * q + py - pad < h]
        for px in (0, 1):
            qx = [q for q in range(nqx) if 0 <= 2 * q + px - pad < w]
            if not qy or not qx:
                continue
            acc = gy.new_zeros(b, cin, len(qy), len(qx))
            for a in range(a_n):
                for c in range(a_n):
                    ky, kx = py + 2 * a, px + 2 * c
                    if ky >= k or kx >= k:
                        continue
                    rows = torch.tensor([q - a + a_n - 1 for q in qy])
                    cols = torch.tensor([q - c + a_n - 1 for q in qx])
                    acc += torch.einsum("bohw,oi->bihw", g[:, :, rows][:, :, :, cols], weight[:, :, ky, kx])
            iy, ix = torch.tensor([2 * q + py - pad for q in qy]), torch.tensor([2 * q + px - pad for q in qx])
            dx[:, :, iy[:, None], ix[None, :]] = acc
    return dx


def wgrad_by_taps(x, gy, k, pad):
    """(dw [Cout, Cin, K, K], dbias [Cout]) from x [B, Cin, H, W] and gy [B, Cout, OH, OW], tap by tap over the zero-padded input."""
    oh, ow = gy.shape[2:]
    xp = F.pad(x, (pad, pad, pad, pad))
    dw = x.new_zeros(gy.shape[1], x.shape[1], k, k)
    for ky in range(k):
        for kx in range(k):
            dw[:, :, ky, kx] = torch.einsum("bihw,bohw->oi", xp[:, :, ky:ky + 2 * oh - 1:2, kx:kx + 2 * ow - 1:2], gy)
    return dw, gy.sum(dim=(0, 2, 3))


def bars(x, weight, gy, pad, addend=None):
    """Elementwise float64 bars (dx, dw, dbias, terms of every dx element) for float32 sums in any order (module docstring)."""
    ax, aw, ag = x.double().abs(), weight.double().abs(), gy.double().abs()
    sdx, sdw, sdb = autograd_adjoints(ax, aw, ag, pad, torch.float64)
    m, _, _ = autograd_adjoints(torch.ones_like(ax), torch.ones_like(aw), torch.ones_like(ag), pad, torch.float64)
    n = gy.shape[0] * gy.shape[2] * gy.shape[3]
    assert float(m.max()) <= 4095 and n <= 4095
    bar_dx = (m + 1) * U * sdx if addend is None else (m + 2) * U * (sdx + addend.double().abs())
    return bar_dx, (n + 1) * U * sdw, n * U * sdb, m


# ------------------------------------------------------------------------------------------------ the stem fixture
FIXTURE = "hourglass_stem_grad"
CASES = {"stem_ave": "ave_pool", "stem_c128": "conv128"}          # name -> hg_down
SHAPE, OUT_SHAPE = (2, 3, 16, 16), (2, 32, 4, 4)
KWARGS = dict(in_channel=3, feature_dim=32, num_hourglass=1, num_stack=1)
STEM = ("conv1", "bn1", "conv2", "down_conv2")
DEPTH = dict(num_hourglass=1, num_stack=1)


def build(namespace, name, **kwargs):
    """``HGFilter(3, 32, num_hourglass=1, num_stack=1, hg_down=...)`` of ``namespace`` (the reference's module or this package's)."""
    return namespace.HGFilter(**KWARGS, hg_down=CASES[name], **kwargs)


def case_input(name, seed):
    return hg_grad_ref._randn("grad-input", name, seed, SHAPE)


def case_cotangent(name, seed):
    return hg_grad_ref._randn("grad-cotangent", name, seed, OUT_SHAPE)


def is_stem(key):
    return key == "input" or key.split(".")[0] in STEM


def restated_grads(name, module, seed, dtype):
    """{name: gradient} of the case on ``module``'s parameters from tests/hg_ref.py under autograd (input and every parameter)."""
    return hg_grad_ref.grads_of("filter", module, case_input(name, seed), case_cotangent(name, seed), dtype,
                                dict(DEPTH, hg_down=CASES[name]), True)


def restated_margin(name, module, seed):
    return hg_grad_ref.relu_margin("filter", module, case_input(name, seed), dict(DEPTH, hg_down=CASES[name]))


def worst(a, ref):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(ref, np.float64)).max())
