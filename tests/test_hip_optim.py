"""FlatAdamW (one HIP launch over the flat gradient bucket) against torch.optim.AdamW -- the optimizer the reference
builds at train.py:97 -- and the CyclicLR schedule of conf/model/tomosar2height.yaml:46-55 driving both.

The second half holds the launch to tests/optim_ref.py: BYTE EQUALITY with ``step32``, the numpy float32 restatement of
csrc/optim.hip's ``adam_one`` (chunk seams and tails, the scalar path of unaligned pointers, channels_last layouts, special
values, hyper-parameter edges, re-planning, the Trainer's GradBucket), and 4 x E32 against the float64 restatement ``step64``,
E32 being CPU torch.optim.AdamW's own float32 - float64 gap on the same 6-step CyclicLR run over SIZES.  Measured:

    state array    E32 (torch CPU - step64)    step32 - step64    device - step64
    params         1.431e-07                   1.431e-07          1.431e-07
    exp_avg        7.447e-08                   7.572e-08          7.572e-08
    exp_avg_sq     6.115e-09                   6.115e-09          6.115e-09

No operand class is excepted from byte equality (subnormal gradients, moments and intermediates included)."""
import copy
import functools
import math
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np
import pytest
import torch

import optim_ref
from tomosar2height_amd.config import berlin_config


def _net(dev):
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Conv2d(8, 16, 3, padding=1), torch.nn.Conv2d(16, 1, 1), torch.nn.Linear(37, 5),
                              torch.nn.Linear(5, 3, bias=False)).to(dev)
    net[0].weight.data = net[0].weight.data.contiguous(memory_format=torch.channels_last)     # dense, non-contiguous
    return net


def _grads(net, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    for p in net.parameters():
        gr = torch.randn(p.shape, generator=g).to(p.device)
        p.grad = gr.contiguous(memory_format=torch.channels_last) if p.dim() == 4 and p.stride() != p.contiguous().stride() else gr


def test_cyclic_lr_schedule_is_the_reference_one():
    from tomosar2height_amd.optim import cyclic_lr
    cfg = berlin_config()
    opt = torch.optim.AdamW(torch.nn.Linear(2, 2).parameters(), lr=cfg.training.learning_rate)
    sched = cyclic_lr(opt, cfg)
    lrs = []
    for _ in range(2001):
        lrs.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    # triangular2, 500 up / 500 down, 1e-4 .. 5e-4, amplitude halves every cycle (train.py:98-104)
    assert lrs[0] == pytest.approx(1e-4) and lrs[500] == pytest.approx(5e-4) and lrs[1000] == pytest.approx(1e-4)
    assert lrs[250] == pytest.approx(3e-4) and lrs[1500] == pytest.approx(3e-4) and lrs[2000] == pytest.approx(1e-4)
    assert opt.param_groups[0]["betas"] == (0.9, 0.999)                 # cycle_momentum: false


@pytest.mark.gpu
def test_flat_adamw_matches_torch_adamw_under_cyclic_lr():
    from tomosar2height_amd.optim import FlatAdamW, cyclic_lr
    dev = torch.device("cuda:0")
    cfg = berlin_config()
    a, b = _net(dev), _net(dev)
    oa = FlatAdamW(a.parameters(), lr=cfg.training.learning_rate)
    ob = torch.optim.AdamW(b.parameters(), lr=cfg.training.learning_rate)
    sa, sb = cyclic_lr(oa, cfg), cyclic_lr(ob, cfg)
    for step in range(6):
        _grads(a, step); _grads(b, step)
        oa.step(); ob.step()
        sa.step(); sb.step()
    for pa, pb in zip(a.parameters(), b.parameters()):
        np.testing.assert_allclose(pa.detach().cpu().numpy(), pb.detach().cpu().numpy(), rtol=2e-6, atol=1e-9)
        np.testing.assert_allclose(oa.state[pa]["exp_avg_sq"].cpu().numpy(), ob.state[pb]["exp_avg_sq"].cpu().numpy(), rtol=2e-6, atol=1e-12)
        assert float(oa.state[pa]["step"]) == 6.0


@pytest.mark.gpu
def test_flat_adamw_state_dict_round_trip_and_zero_grad():
    from tomosar2height_amd.optim import FlatAdamW
    dev = torch.device("cuda:0")
    a = _net(dev)
    oa = FlatAdamW(a.parameters(), lr=1e-3)
    for step in range(2):
        _grads(a, step)
        oa.step()
    sd = copy.deepcopy(oa.state_dict())
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}       # torch.optim.AdamW's checkpoint format
    b = _net(dev)
    b.load_state_dict(a.state_dict())
    ob = FlatAdamW(b.parameters(), lr=1e-3)
    ob.load_state_dict(sd)
    tb = torch.optim.AdamW(_net(dev).parameters(), lr=1e-3)
    tb.load_state_dict(copy.deepcopy(sd))                                  # and torch's own optimizer accepts it
    _grads(a, 9); _grads(b, 9)
    oa.step(); ob.step(zero_grad=True)
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert torch.equal(pa, pb)
        assert not pb.grad.any()


# ------------------------------------------------------------------------------------------------------------------------
# FlatAdamW against tests/optim_ref.py: byte equality with the float32 restatement of csrc/optim.hip (step32), and
# 4 x E32 against float64 (step64), where E32 is CPU torch.optim.AdamW's own float32 - float64 gap on the same run.

SIZES = (1, 2, 3, 4, 5, 4095, 4096, 4097, 8191, 8192, 8195, 12289 + 2)     # chunk = 4096: seams, partial chunks, n % 4 tails
CHUNK = 4096
CANARY = np.float32(-12345.678)
HYPER = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)      # torch.optim.AdamW's defaults


def _dev():
    return torch.device("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_same(got, want, what):
    if not optim_ref.same_floats(got, want):
        bad, n_bad = optim_ref.first_mismatches(got, want)
        raise AssertionError(f"{what}: {n_bad} of {want.size} elements differ from the float32 restatement; "
                             f"(position, device, step32) {bad}")


def _storage(t):
    """Host copy of the numel() floats a dense tensor occupies, in STORAGE order (no .contiguous(): the bytes as they lie)."""
    return torch.as_strided(t.detach(), (t.numel(),), (1,), t.storage_offset()).cpu().numpy().copy()


def _pack(arrays, dev, shift=0):
    """One canary-filled device buffer holding every array as a view ``shift`` floats past a 16-byte boundary, with at least
    four canary floats between neighbours and at both ends.  Returns (buffer, views, mask of the floats no view owns)."""
    offs, off = [], 4
    for a in arrays:
        offs.append(off + shift)
        off += -(-(a.size + shift) // 4) * 4 + 4
    host = np.full(off, CANARY, np.float32)
    free = np.ones(off, bool)
    for o, a in zip(offs, arrays):
        host[o:o + a.size] = a
        free[o:o + a.size] = False
    base = torch.from_numpy(host).to(dev)
    assert base.data_ptr() % 16 == 0
    return base, [base[o:o + a.size] for o, a in zip(offs, arrays)], free


def _canaries_intact(base, free):
    return bool((_bits(base.cpu().numpy())[free] == _bits(CANARY)).all())


class _Mirror:
    """Host mirror of an optimizer: ``step()`` first advances float32 host copies of every live parameter's storage with
    optim_ref.step32 (state carried on the host from the first step on), then steps the optimizer and requires p, exp_avg and
    exp_avg_sq to hold the same bytes."""

    def __init__(self, opt):
        self.opt, self.host = opt, {}

    def _entry(self, p):
        h = self.host.get(p)
        if h is None:
            st = self.opt.state.get(p) or {}
            if "exp_avg" in st:                                                # loaded from a state_dict
                m, v = (_storage(torch.empty_like(p).copy_(st[k])) for k in ("exp_avg", "exp_avg_sq"))
                h = [_storage(p), m, v, int(float(st["step"]))]
            else:
                h = [_storage(p), np.zeros(p.numel(), np.float32), np.zeros(p.numel(), np.float32), 0]
            self.host[p] = h
        return h

    def predict(self):
        for group in self.opt.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                h = self._entry(p)
                s = optim_ref.scalars(group["lr"], *group["betas"], group["eps"], group["weight_decay"], h[3] + 1)
                h[0], h[1], h[2] = optim_ref.step32(h[0], _storage(p.grad), h[1], h[2], s)
                h[3] += 1

    def check(self, tag=""):
        for i, (p, h) in enumerate(self.host.items()):
            st = self.opt.state[p]
            where = f"{tag} tensor {i} (n = {p.numel()}, step {h[3]})"
            assert float(st["step"]) == h[3], where
            _assert_same(_storage(p), h[0], where + " p")
            _assert_same(_storage(st["exp_avg"]), h[1], where + " exp_avg")
            _assert_same(_storage(st["exp_avg_sq"]), h[2], where + " exp_avg_sq")

    def step(self, zero_grad=False, tag=""):
        self.predict()
        self.opt.step(zero_grad=zero_grad)
        self.check(tag)


def _params(views):
    return [torch.nn.Parameter(v) for v in views]


def _set_grads(params, grads):
    """Write values into the existing gradient tensors (same data_ptr: no re-plan), or attach them the first time."""
    for p, g in zip(params, grads):
        if p.grad is None:
            p.grad = g
        else:
            p.grad.copy_(g)


def _grads_are_plus_zero(params):
    return all(not _bits(_storage(p.grad)).any() for p in params)


@functools.lru_cache(maxsize=None)
def _cyclic_reference():
    """Computed once on the CPU, never changed: 6 steps under cyclic_lr over SIZES by CPU torch.optim.AdamW (float32, the
    single-tensor form), by step32 and by step64, all on the same seeded values; E32[x] = max |torch_cpu - step64|."""
    from tomosar2height_amd.optim import cyclic_lr
    cfg = berlin_config()
    rng = np.random.default_rng(20240607)
    p0 = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in SIZES]
    grads = [[rng.standard_normal(n).astype(np.float32) for n in SIZES] for _ in range(6)]
    params = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in p0]
    opt = torch.optim.AdamW(params, lr=cfg.training.learning_rate, foreach=False, fused=False)
    sched = cyclic_lr(opt, cfg)
    r32 = [[p.copy(), np.zeros_like(p), np.zeros_like(p)] for p in p0]
    r64 = [[p.astype(np.float64), np.zeros(p.size), np.zeros(p.size)] for p in p0]
    lrs = []
    for k in range(6):
        group = opt.param_groups[0]
        lr = group["lr"]
        lrs.append(lr)
        for p, g in zip(params, grads[k]):
            p.grad = torch.from_numpy(g.copy())
        opt.step()
        sched.step()
        s = optim_ref.scalars(lr, *group["betas"], group["eps"], group["weight_decay"], k + 1)
        for i, g in enumerate(grads[k]):
            r32[i] = list(optim_ref.step32(r32[i][0], g, r32[i][1], r32[i][2], s))
            r64[i] = list(optim_ref.step64(r64[i][0], g, r64[i][1], r64[i][2], lr, group["betas"], group["eps"],
                                           group["weight_decay"], k + 1))
    t32 = [[p.detach().numpy(), opt.state[p]["exp_avg"].numpy(), opt.state[p]["exp_avg_sq"].numpy()] for p in params]
    e32 = [max(float(np.abs(t[x].astype(np.float64) - r[x]).max()) for t, r in zip(t32, r64)) for x in range(3)]
    return dict(cfg=cfg, p0=p0, grads=grads, lrs=lrs, r32=r32, r64=r64, e32=e32)


STATE_NAMES = ("params", "exp_avg", "exp_avg_sq")


def test_restatements_against_cpu_torch_adamw():
    """step32 stays within 4 x E32 of step64 for every state array, where E32 is CPU torch.optim.AdamW's own distance from
    step64 on the same 6-step cyclic-LR run (so step64 is torch's formula, and step32 is as good a float32 AdamW as torch's).
    Measured (this test prints them): E32 = 1.431e-07 (params), 7.447e-08 (exp_avg), 6.115e-09 (exp_avg_sq); step32's own
    gaps are 1.431e-07, 7.572e-08 and 6.115e-09."""
    ref = _cyclic_reference()
    for x, name in enumerate(STATE_NAMES):
        e32 = ref["e32"][x]
        err = max(float(np.abs(r[x].astype(np.float64) - w[x]).max()) for r, w in zip(ref["r32"], ref["r64"]))
        print(f"{name}: E32 = {e32:.3e}, max|step32 - step64| = {err:.3e}")
        assert e32 > 0.0                                   # a float32 run that met float64 exactly would make the bound void
        assert err <= 4 * e32, (name, err, e32)


def _round_f32(x):
    """A rational rounded ONCE to float32 (nearest, ties to even); normal range."""
    x = Fraction(x)
    if x == 0:
        return np.float32(0.0)
    sign, x = (-1, -x) if x < 0 else (1, x)
    e = math.floor(math.log2(x))
    while Fraction(2) ** e > x:
        e -= 1
    while Fraction(2) ** (e + 1) <= x:
        e += 1
    assert -126 <= e <= 127
    q = round(x / Fraction(2) ** (e - 23))                 # Fraction.__round__: ties to even; 2^23 <= q <= 2^24
    return np.float32(sign * q * 2.0 ** (e - 23))


def _scalars_independent(lr, beta1, beta2, eps, weight_decay, step):
    """The seven scalars from the exact values of the double arguments in 200-digit decimal arithmetic, rounded once."""
    ctx = getcontext().copy()
    ctx.prec = 200
    d = [Decimal(float(x)) for x in (lr, beta1, beta2, eps, weight_decay)]          # exact
    lr, beta1, beta2, eps, weight_decay = d
    bc1 = ctx.subtract(1, ctx.power(beta1, step))
    bc2 = ctx.subtract(1, ctx.power(beta2, step))
    vals = (ctx.subtract(1, ctx.multiply(lr, weight_decay)), ctx.subtract(1, beta1), beta2, ctx.subtract(1, beta2),
            -ctx.divide(lr, bc1), ctx.sqrt(bc2), eps)
    return tuple(_round_f32(Fraction(v)) for v in vals)


@functools.lru_cache(maxsize=None)
def _cyclic_lrs(n):
    from tomosar2height_amd.optim import cyclic_lr
    cfg = berlin_config()
    opt = torch.optim.SGD(torch.nn.Linear(1, 1).parameters(), lr=cfg.training.learning_rate)
    sched = cyclic_lr(opt, cfg)
    lrs = []
    for _ in range(n):
        lrs.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    return lrs


def test_scalars_against_independent_arithmetic():
    """optim_ref.scalars (double arithmetic as in t2h_adamw_flat_step, rounded once) against 200-digit decimal arithmetic on
    the same double arguments rounded once: step 1; steps 2000 and 2001 (the learning rates on both sides of the CyclicLR
    trough at scheduler step 2000); step 100 000, where beta^step has left the range that matters (0.9^1e5 underflows,
    0.999^1e5 = 3.5e-44 is far below half an ulp of 1, so both bias corrections are 1.0 already in double)."""
    lrs = _cyclic_lrs(2001)
    assert lrs[2000] < lrs[1999] and lrs[2000] == pytest.approx(1e-4)
    cases = [(1e-4, 1), (lrs[0], 1), (lrs[1999], 2000), (lrs[2000], 2001), (lrs[1001], 1002), (1e-3, 100000), (lrs[1999], 100000)]
    for lr, step in cases:
        for betas, eps, wd in (((0.9, 0.999), 1e-8, 1e-2), ((0.0, 0.999), 0.0, 0.0), ((0.8, 0.99), 1e-6, 0.1)):
            got = optim_ref.scalars(lr, betas[0], betas[1], eps, wd, step)
            want = _scalars_independent(lr, betas[0], betas[1], eps, wd, step)
            assert all(g.dtype == np.float32 for g in got)
            assert [float(g) for g in got] == [float(w) for w in want], (lr, step, betas, eps, wd, got, want)
    s = optim_ref.scalars(1e-3, 0.9, 0.999, 1e-8, 1e-2, 100000)
    assert s[4] == np.float32(-1e-3) and s[5] == np.float32(1.0)
    s = optim_ref.scalars(1e-3, 0.9, 0.999, 1e-8, 1e-2, 1)
    assert s[4] == _round_f32(-Fraction(1e-3) / (1 - Fraction(0.9))) and s[5] == _round_f32(Fraction(math.sqrt(1 - 0.999)))


def test_step32_is_one_rounding_per_operation():
    """step32 on hand-checked operands (exact rationals rounded after every operation) -- the restatement must not be
    computing in a wider type and rounding at the end."""
    s = optim_ref.scalars(1e-3, 0.9, 0.999, 1e-8, 1e-2, 3)
    rng = np.random.default_rng(5)
    p, g = (rng.standard_normal(64).astype(np.float32) for _ in range(2))
    m, v = (0.1 * rng.standard_normal(64)).astype(np.float32), (0.01 * rng.random(64)).astype(np.float32)
    got = optim_ref.step32(p, g, m, v, s)
    F = Fraction
    r = lambda x: F(float(_round_f32(x)))                                     # one float32 rounding, as an exact rational
    decay, omb1, b2, omb2, nss, bc2s, eps = (F(float(x)) for x in s)
    for i in range(64):
        pi, gi, mi, vi = (F(float(a[i])) for a in (p, g, m, v))
        pi = r(pi * decay)
        mi = r(mi + r(omb1 * r(gi - mi)))
        vi = r(r(vi * b2) + r(r(omb2 * gi) * gi))
        sq = F(float(np.sqrt(np.float32(float(vi)))))                         # the correctly rounded root: vi lies between the
        lo, hi = (F(float(np.nextafter(np.float32(float(sq)), np.float32(t)))) for t in (0.0, np.inf))  # squared midpoints
        assert ((sq + lo) / 2) ** 2 <= vi <= ((sq + hi) / 2) ** 2
        pi = r(pi + r(nss * r(mi / r(r(sq / bc2s) + eps))))
        assert (F(float(got[0][i])), F(float(got[1][i])), F(float(got[2][i]))) == (pi, mi, vi), i


# ------------------------------------------------------------------------------------------------------------------------ a
def _moment_offsets(params):
    offs, off = [], 0
    for p in params:
        offs.append(off)
        off += -(-p.numel() // 4) * 4
    return offs


@pytest.mark.gpu
def test_flat_adamw_chunk_seams_and_tails_are_bit_exact():
    """(a) One parameter per size in SIZES in one optimizer: a second and third chunk (begin > 0), the clamp on a last partial
    chunk, a float4 body followed by an n % 4 tail inside a later chunk, odd sizes shifting every later moment offset by the
    4-float padding.  3 steps, then one with zero_grad=True; canaries between the tensors of the buffers this test owns."""
    from tomosar2height_amd.optim import FlatAdamW
    ref = _cyclic_reference()
    pbase, pviews, pfree = _pack(ref["p0"], _dev())
    gbase, gviews, gfree = _pack(ref["grads"][0], _dev())
    params = _params(pviews)
    opt = FlatAdamW(params, **HYPER)
    mir = _Mirror(opt)
    for k in range(4):
        if k == 0:
            _set_grads(params, gviews)
        else:
            _set_grads(params, [torch.from_numpy(g).to(_dev()) for g in ref["grads"][k]])
        mir.step(zero_grad=(k == 3), tag=f"step {k + 1}")
        assert _canaries_intact(pbase, pfree) and _canaries_intact(gbase, gfree), f"step {k + 1} wrote outside a tensor"
        if k < 3:
            for p, g in zip(params, ref["grads"][k]):
                assert np.array_equal(_bits(_storage(p.grad)), _bits(g))        # gradients are read-only without zero_grad
    assert _grads_are_plus_zero(params)
    assert all(p.grad.data_ptr() == g.data_ptr() for p, g in zip(params, gviews))
    plan = opt._plans[0]
    assert plan["n_chunks"] == sum(-(-n // CHUNK) for n in SIZES)
    # the moments: one flat buffer each, every tensor on a 16-byte boundary (4-float padding), padding floats still zero
    offs = _moment_offsets(params)
    used = np.zeros(plan["m"].numel(), bool)
    for p, off in zip(params, offs):
        for key, flat in (("exp_avg", plan["m"]), ("exp_avg_sq", plan["v"])):
            t = opt.state[p][key]
            assert t.data_ptr() == flat.data_ptr() + 4 * off and t.data_ptr() % 16 == 0
        used[off:off + p.numel()] = True
    assert used.size == offs[-1] + -(-SIZES[-1] // 4) * 4
    assert not _bits(plan["m"].cpu().numpy())[~used].any() and not _bits(plan["v"].cpu().numpy())[~used].any()


# ------------------------------------------------------------------------------------------------------------------------ b
@pytest.mark.gpu
@pytest.mark.parametrize("n", [5, 4097, 8195])
def test_flat_adamw_scalar_path_is_bit_identical_to_the_float4_path(n):
    """(b) Parameters and / or gradients one float past a 16-byte boundary take the kernel's scalar branch: the same bytes as
    the aligned run of the same values, nothing written outside the views, gradients cleared by zero_grad there too."""
    from tomosar2height_amd.optim import FlatAdamW
    rng = np.random.default_rng(n)
    p0 = (0.1 * rng.standard_normal(n)).astype(np.float32)
    grads = [rng.standard_normal(n).astype(np.float32) for _ in range(3)]
    results = {}
    for case, (pshift, gshift) in dict(aligned=(0, 0), p_off=(1, 0), g_off=(0, 1), both_off=(1, 1)).items():
        pbase, (pv,), pfree = _pack([p0], _dev(), shift=pshift)
        gbase, (gv,), gfree = _pack([grads[0]], _dev(), shift=gshift)
        p = torch.nn.Parameter(pv)
        p.grad = gv
        assert p.data_ptr() % 16 == 4 * pshift and p.grad.data_ptr() % 16 == 4 * gshift
        opt = FlatAdamW([p], **HYPER)
        mir = _Mirror(opt)
        for k in range(3):
            p.grad.copy_(torch.from_numpy(grads[k]).to(_dev()))
            mir.step(zero_grad=(k == 2), tag=f"{case} step {k + 1}")
            assert _canaries_intact(pbase, pfree) and _canaries_intact(gbase, gfree), (case, k)
            if k < 2:
                assert np.array_equal(_bits(_storage(p.grad)), _bits(grads[k]))
        assert p.grad.data_ptr() == gv.data_ptr() and _grads_are_plus_zero([p]), case
        results[case] = [_storage(p), _storage(opt.state[p]["exp_avg"]), _storage(opt.state[p]["exp_avg_sq"])]
    for case in ("p_off", "g_off", "both_off"):
        for got, want in zip(results[case], results["aligned"]):
            assert np.array_equal(_bits(got), _bits(want)), case


# ------------------------------------------------------------------------------------------------------------------------ c
@pytest.mark.gpu
def test_flat_adamw_channels_last_weights_across_chunks():
    """(c) Dense non-contiguous tensors longer than a chunk: a channels_last Conv2d(32, 32, 3) weight (9216 elements, three
    chunks) and a channels_last ConvTranspose2d(48, 32, 2) weight (6144: one full chunk and a partial one), gradients with the
    same strides.  Storage order byte for byte, and the moments READ THROUGH THEIR STRIDED VIEWS against the reference of the
    logical elements (a moment view with other strides than its parameter would pass the first and fail the second)."""
    from tomosar2height_amd.optim import FlatAdamW
    torch.manual_seed(11)
    mods = [torch.nn.Conv2d(32, 32, 3), torch.nn.ConvTranspose2d(48, 32, 2, stride=2), torch.nn.Conv2d(8, 16, 3)]
    params = []
    for mod in mods:
        mod.weight.data = mod.weight.data.to(_dev()).contiguous(memory_format=torch.channels_last)
        assert not mod.weight.is_contiguous()
        params.append(mod.weight)
    assert [p.numel() for p in params] == [9216, 6144, 1152]
    opt = FlatAdamW(params, **HYPER)
    mir = _Mirror(opt)
    gen = torch.Generator().manual_seed(12)
    logical = [[p.detach().cpu().numpy().ravel().copy(), np.zeros(p.numel(), np.float32), np.zeros(p.numel(), np.float32)]
               for p in params]
    for k in range(3):
        gs = [torch.randn(p.shape, generator=gen) for p in params]
        for p, g in zip(params, gs):
            p.grad = torch.empty_like(p).copy_(g.to(_dev()))
            assert p.grad.stride() == p.stride()
        mir.step(zero_grad=(k == 2), tag=f"step {k + 1}")
        s = optim_ref.scalars(HYPER["lr"], *HYPER["betas"], HYPER["eps"], HYPER["weight_decay"], k + 1)
        for i, (p, g) in enumerate(zip(params, gs)):
            logical[i] = list(optim_ref.step32(logical[i][0], g.numpy().ravel(), logical[i][1], logical[i][2], s))
            st = opt.state[p]
            assert st["exp_avg"].shape == p.shape and st["exp_avg"].stride() == p.stride()
            _assert_same(p.detach().cpu().numpy().ravel(), logical[i][0], f"logical p {i}")
            _assert_same(st["exp_avg"].cpu().numpy().ravel(), logical[i][1], f"logical exp_avg {i}")
            _assert_same(st["exp_avg_sq"].cpu().numpy().ravel(), logical[i][2], f"logical exp_avg_sq {i}")
    assert _grads_are_plus_zero(params)


# ------------------------------------------------------------------------------------------------------------------------ d
N_VAL = 8195                                             # chunks [0, 4096), [4096, 8192), [8192, 8195): the last is all tail
# chunk position 0, the last float4 of a chunk (4092..4095), both sides of both seams, the tail
POS = np.array([0, 4092, 4093, 4095, 4096, 8191, 8192, 8194])
FLT_MAX = float(np.finfo(np.float32).max)
DENORM = 1e-40                                           # subnormal in float32
TINY = float(np.finfo(np.float32).smallest_subnormal)


@functools.lru_cache(maxsize=None)
def _value_base():
    rng = np.random.default_rng(77)
    p0 = (0.1 * rng.standard_normal(N_VAL)).astype(np.float32)
    grads = [rng.standard_normal(N_VAL).astype(np.float32) for _ in range(2)]
    return p0, grads


def _value_run(p_val, g_vals):
    """Two steps on the 8195-element tensor with ``p_val`` (or the base value) at POS in p and ``g_vals[k]`` (or the base value)
    at POS in the gradient of step k; returns the mirror's expectation and the device's storage after each step."""
    from tomosar2height_amd.optim import FlatAdamW
    p0, grads = _value_base()
    p0 = p0.copy()
    if p_val is not None:
        p0[POS] = np.float32(p_val)
    p = torch.nn.Parameter(torch.from_numpy(p0).to(_dev()))
    opt = FlatAdamW([p], **HYPER)
    mir = _Mirror(opt)
    out = []
    for k in range(2):
        g = grads[k].copy()
        if g_vals[k] is not None:
            g[POS] = np.float32(g_vals[k])
        p.grad = torch.from_numpy(g).to(_dev())
        mir.predict()
        opt.step()
        st = opt.state[p]
        out.append(dict(want=[a.copy() for a in mir.host[p][:3]], p0=p0,
                        got=[_storage(p), _storage(st["exp_avg"]), _storage(st["exp_avg_sq"])]))
    return out


@functools.lru_cache(maxsize=None)
def _clean_value_run():
    return _value_run(None, (None, None))


VALUE_CASES = {
    # name: (p at POS, gradient at POS in step 1, in step 2)
    "g_zero": (None, 0.0, 0.0), "g_neg_zero": (None, -0.0, -0.0),
    "g_inf": (None, np.inf, None), "g_neg_inf": (None, -np.inf, None), "g_nan": (None, np.nan, None),
    "g_nan_late": (None, None, np.nan), "g_inf_late": (None, None, np.inf),
    "g_1e20": (None, 1e20, 1e20), "g_neg_1e20": (None, -1e20, -1e20),
    "g_1e25": (None, 1e25, 1e25), "g_neg_1e25": (None, -1e25, -1e25),
    "g_1e-30": (None, 1e-30, 1e-30), "g_neg_1e-30": (None, -1e-30, -1e-30),
    "g_denormal": (None, DENORM, DENORM), "g_neg_denormal": (None, -DENORM, -DENORM), "g_smallest": (None, TINY, -TINY),
    "g_1e-20_then_denormal": (None, 1e-20, DENORM),
    "p_zero": (0.0, None, None), "p_neg_zero": (-0.0, None, None), "p_flt_max": (FLT_MAX, None, None),
    "p_neg_flt_max_g_zero": (-FLT_MAX, 0.0, 0.0), "p_neg_zero_g_zero": (-0.0, 0.0, 0.0),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(VALUE_CASES))
def test_flat_adamw_special_values(case):
    """(d) Special operands at chunk position 0, in the last float4 of a chunk, on both sides of both chunk seams and in the
    tail of an 8195-element tensor, over two steps (zero moments, then the moments the first step left): every element byte
    equal to step32 (NaN where step32 has NaN), and every OTHER element bit-identical to the run without the special values.
    Subnormal operands and intermediates (g = 1e-40, 1.4e-45; g = 1e-20, whose v = 1e-43 is subnormal under the square root;
    m / denom with a subnormal m) are held to byte equality like the rest: the device's division and square root keep them."""
    p_val, g1, g2 = VALUE_CASES[case]
    runs, clean = _value_run(p_val, (g1, g2)), _clean_value_run()
    others = np.ones(N_VAL, bool)
    others[POS] = False
    for k, (run, ref) in enumerate(zip(runs, clean)):
        for x, name in enumerate(STATE_NAMES):
            _assert_same(run["got"][x], run["want"][x], f"{case} step {k + 1} {name}")
            assert np.array_equal(_bits(run["got"][x])[others], _bits(ref["got"][x])[others]), \
                f"{case} step {k + 1}: a neighbour's {name} differs from the run without the special values"
    p_after, m_after, v_after = (a[POS] for a in runs[0]["got"])
    p_before = runs[0]["p0"][POS]
    decay = optim_ref.scalars(HYPER["lr"], *HYPER["betas"], HYPER["eps"], HYPER["weight_decay"], 1)[0]
    with np.errstate(all="ignore"):
        decayed = p_before * decay
    if case in ("g_zero", "g_neg_zero", "p_neg_flt_max_g_zero", "p_neg_zero_g_zero"):
        # zero gradient on zero moments: the update is exactly 0, p only decays (and keeps its sign bit), moments stay 0
        assert np.array_equal(_bits(p_after), _bits(decayed)) and not m_after.any() and not _bits(v_after).any()
        assert np.array_equal(_bits(runs[1]["got"][0][POS]), _bits(decayed * optim_ref.scalars(
            HYPER["lr"], *HYPER["betas"], HYPER["eps"], HYPER["weight_decay"], 2)[0]))
    if case in ("g_1e20", "g_neg_1e20"):
        # g * g = 1e40 overflows, but the kernel (like torch's CPU addcmul) forms ((1 - beta2) * g) * g = 1e37: v stays finite
        # and the step is an ordinary one.  (1 - beta2) * (g * g) -- the order of torch's device addcmul -- would give inf.
        assert np.isfinite(v_after).all() and np.isfinite(p_after).all() and not np.array_equal(_bits(p_after), _bits(decayed))
    if case in ("g_1e25", "g_neg_1e25"):
        # the second moment overflows in either order: v = inf, denom = inf, m / denom = 0, so p only decays
        assert np.isinf(v_after).all() and np.isfinite(m_after).all() and np.array_equal(_bits(p_after), _bits(decayed))
    if case in ("g_inf", "g_neg_inf", "g_nan"):
        assert np.isnan(p_after).all() and np.isnan(runs[1]["got"][0][POS]).all()
    if case in ("g_1e-30", "g_neg_1e-30", "g_denormal", "g_neg_denormal", "g_smallest"):
        assert not _bits(v_after).any()                        # g * g underflows to +0
        assert m_after.all() or case == "g_smallest"           # m = 0.1 g survives, as a subnormal for g = 1e-40
    if case == "p_flt_max":
        assert np.isfinite(p_after).all()


# ------------------------------------------------------------------------------------------------------------------------ e
@pytest.mark.gpu
@pytest.mark.parametrize("name, hyper", [("lr_zero", dict(lr=0.0)), ("weight_decay_zero", dict(weight_decay=0.0)),
                                         ("beta1_zero", dict(betas=(0.0, 0.999))), ("eps_zero", dict(eps=0.0)),
                                         ("beta2_zero", dict(betas=(0.9, 0.0)))])
def test_flat_adamw_hyper_parameter_edges(name, hyper):
    """(e) lr = 0, weight_decay = 0, beta1 = 0, eps = 0 (non-zero gradients), over step 1 and step 2."""
    from tomosar2height_amd.optim import FlatAdamW
    p0, grads = _value_base()
    assert grads[0].all() and grads[1].all()
    p = torch.nn.Parameter(torch.from_numpy(p0.copy()).to(_dev()))
    opt = FlatAdamW([p], **{**HYPER, **hyper})
    mir = _Mirror(opt)
    for k in range(2):
        p.grad = torch.from_numpy(grads[k]).to(_dev())
        mir.step(tag=f"{name} step {k + 1}")
        if name == "lr_zero":
            # decay = 1 - 0 * wd = 1 and the step size is -0: p changes by its decay only, which is by nothing
            assert np.array_equal(_bits(_storage(p)), _bits(p0))
        if name == "beta1_zero" and k == 0:                  # m = 0 + 1 * (g - 0); later, m + (g - m) rounds twice
            assert np.array_equal(_bits(_storage(opt.state[p]["exp_avg"])), _bits(grads[k]))


@pytest.mark.gpu
def test_flat_adamw_step_100000_from_a_state_dict():
    """(e) step 100 000: a state_dict with step = 99 999 and non-trivial moments, one step; byte equal to step32, and within the
    module's rtol = 2e-6 of device torch.optim.AdamW loaded from the same dict."""
    from tomosar2height_amd.optim import FlatAdamW
    rng = np.random.default_rng(99)
    n = 8195
    p0 = (0.1 * rng.standard_normal(n)).astype(np.float32)
    g = rng.standard_normal(n).astype(np.float32)
    m0 = (0.3 * rng.standard_normal(n)).astype(np.float32)
    v0 = (rng.standard_normal(n).astype(np.float32) ** 2 * np.float32(0.7) + np.float32(1e-3)).astype(np.float32)
    pa, pb = (torch.nn.Parameter(torch.from_numpy(p0.copy()).to(_dev())) for _ in range(2))
    oa, ob = FlatAdamW([pa], **HYPER), torch.optim.AdamW([pb], **HYPER)
    sd = dict(state={0: dict(step=torch.tensor(99999.0), exp_avg=torch.from_numpy(m0), exp_avg_sq=torch.from_numpy(v0))},
              param_groups=oa.state_dict()["param_groups"])
    oa.load_state_dict(copy.deepcopy(sd))
    ob.load_state_dict(copy.deepcopy(sd))
    pa.grad, pb.grad = (torch.from_numpy(g).to(_dev()) for _ in range(2))
    mir = _Mirror(oa)
    mir.predict()
    assert mir.host[pa][3] == 100000 and np.array_equal(_bits(_storage(oa.state[pa]["exp_avg"].to(_dev()))), _bits(m0))
    oa.step()
    ob.step()
    mir.check("step 100000")
    assert float(oa.state[pa]["step"]) == 100000.0 == float(ob.state[pb]["step"])
    assert not np.array_equal(_storage(pa), p0)
    np.testing.assert_allclose(_storage(pa), pb.detach().cpu().numpy(), rtol=2e-6, atol=1e-9)
    np.testing.assert_allclose(_storage(oa.state[pa]["exp_avg_sq"]), ob.state[pb]["exp_avg_sq"].cpu().numpy(), rtol=2e-6,
                               atol=1e-12)


@pytest.mark.gpu
def test_flat_adamw_two_param_groups():
    """(e) Two groups with their own lr and weight_decay, each with a tensor longer than a chunk: one launch per group, each
    with its own scalars."""
    from tomosar2height_amd.optim import FlatAdamW
    rng = np.random.default_rng(31)
    sizes = ((4097, 3), (8195,))
    groups = [[torch.nn.Parameter(torch.from_numpy((0.1 * rng.standard_normal(n)).astype(np.float32)).to(_dev())) for n in ns]
              for ns in sizes]
    opt = FlatAdamW([dict(params=groups[0], lr=1e-3, weight_decay=0.0), dict(params=groups[1], lr=3e-4, weight_decay=0.1)])
    mir = _Mirror(opt)
    for k in range(3):
        for p in groups[0] + groups[1]:
            p.grad = torch.from_numpy(rng.standard_normal(p.numel()).astype(np.float32)).to(_dev())
        mir.step(zero_grad=(k == 2), tag=f"step {k + 1}")
    assert [opt._plans[i]["n_chunks"] for i in range(2)] == [3, 3]
    assert _grads_are_plus_zero(groups[0] + groups[1])


# ------------------------------------------------------------------------------------------------------------------------ f
def _fresh(sizes, seed):
    rng = np.random.default_rng(seed)
    return [torch.nn.Parameter(torch.from_numpy((0.1 * rng.standard_normal(n)).astype(np.float32)).to(_dev())) for n in sizes]


def _snapshot(opt, params):
    return [[_storage(p)] + [_storage(opt.state[p][k]) for k in ("exp_avg", "exp_avg_sq") if k in opt.state.get(p, {})]
            for p in params]


@pytest.mark.gpu
def test_flat_adamw_replanning_carries_the_moments_over():
    """(f) After 2 steps every p.grad is REPLACED by a new tensor (new data_ptr): the optimizer re-plans, copies the moments
    into new flat buffers, and step 3 leaves the same bytes as in an optimizer whose gradients were updated in place."""
    from tomosar2height_amd.optim import FlatAdamW
    sizes = (5, 4097, 8195, 2)
    rng = np.random.default_rng(41)
    grads = [[rng.standard_normal(n).astype(np.float32) for n in sizes] for _ in range(3)]
    pa, pb = _fresh(sizes, 40), _fresh(sizes, 40)
    oa, ob = FlatAdamW(pa, **HYPER), FlatAdamW(pb, **HYPER)
    ma, mb = _Mirror(oa), _Mirror(ob)
    for k in range(2):
        for params, mir in ((pa, ma), (pb, mb)):
            _set_grads(params, [torch.from_numpy(g).to(_dev()) for g in grads[k]])
            mir.step(tag=f"step {k + 1}")
    plan_a, plan_b = oa._plans[0], ob._plans[0]
    old = [p.grad for p in pa]                                # kept alive: the allocator cannot hand the same blocks out again
    for p, g in zip(pa, grads[2]):
        p.grad = torch.from_numpy(g).to(_dev())
    assert all(p.grad.data_ptr() != o.data_ptr() for p, o in zip(pa, old))
    _set_grads(pb, [torch.from_numpy(g).to(_dev()) for g in grads[2]])
    ma.step(tag="step 3, re-planned")
    mb.step(tag="step 3, same plan")
    assert oa._plans[0] is not plan_a and ob._plans[0] is plan_b
    for a, b in zip(_snapshot(oa, pa), _snapshot(ob, pb)):
        assert len(a) == len(b) == 3 and all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


@pytest.mark.gpu
def test_flat_adamw_skips_parameters_without_gradient_and_refuses_mixed_step_counts():
    """(f) A parameter whose grad is None is left untouched and gets no state, as in torch.  When it becomes live after the
    others have stepped, step() raises -- before any parameter or moment has changed."""
    from tomosar2height_amd.optim import FlatAdamW
    sizes = (4097, 4099, 6)
    rng = np.random.default_rng(51)
    params = _fresh(sizes, 50)
    idle = params[1]
    idle_before = _storage(idle)
    opt = FlatAdamW(params, **HYPER)
    mir = _Mirror(opt)
    for p in (params[0], params[2]):
        p.grad = torch.from_numpy(rng.standard_normal(p.numel()).astype(np.float32)).to(_dev())
    mir.step(tag="step 1")
    assert idle not in opt.state and idle.grad is None and np.array_equal(_bits(_storage(idle)), _bits(idle_before))
    assert opt._plans[0]["n_chunks"] == 3 and set(mir.host) == {params[0], params[2]}
    idle.grad = torch.from_numpy(rng.standard_normal(idle.numel()).astype(np.float32)).to(_dev())
    before = _snapshot(opt, params)
    with pytest.raises(RuntimeError, match="share their step count"):
        opt.step()
    after = _snapshot(opt, params)
    for b, a in zip(before, after):
        assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(b, a))   # parameters and the moments that existed
    assert [float(opt.state[p]["step"]) for p in (params[0], params[2])] == [1.0, 1.0]
    mir.check("after the refusal")


@pytest.mark.gpu
def test_flat_adamw_refuses_float64_and_foreign_gradient_layouts():
    """(f) The documented errors: a float64 parameter; a gradient with other strides than its parameter."""
    from tomosar2height_amd.optim import FlatAdamW
    p = torch.nn.Parameter(torch.zeros(8, dtype=torch.float64, device=_dev()))
    p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError, match="fp32 parameters on the MI355X only"):
        FlatAdamW([p]).step()
    assert not p.detach().any()
    w = torch.nn.Parameter(torch.zeros(4, 6, 3, 3, device=_dev()))
    w.grad = torch.ones(4, 6, 3, 3, device=_dev()).contiguous(memory_format=torch.channels_last)
    assert w.grad.stride() != w.stride()
    with pytest.raises(RuntimeError, match="share its parameter's dense memory layout"):
        FlatAdamW([w]).step()
    assert not w.detach().any()


# ------------------------------------------------------------------------------------------------------------------------ g
@pytest.mark.gpu
def test_flat_adamw_against_float64_under_cyclic_lr():
    """(g) The 6-step cyclic-LR run over SIZES on the device: within 4 x E32 of step64 for every state array (E32: CPU
    torch.optim.AdamW's own distance from step64, computed in _cyclic_reference), so that a mistake shared by step32 and the
    kernel cannot hide behind their byte equality -- which is asserted on the same run."""
    from tomosar2height_amd.optim import FlatAdamW, cyclic_lr
    ref = _cyclic_reference()
    params = [torch.nn.Parameter(torch.from_numpy(p.copy()).to(_dev())) for p in ref["p0"]]
    opt = FlatAdamW(params, lr=ref["cfg"].training.learning_rate)
    sched = cyclic_lr(opt, ref["cfg"])
    for k in range(6):
        assert opt.param_groups[0]["lr"] == ref["lrs"][k]
        _set_grads(params, [torch.from_numpy(g).to(_dev()) for g in ref["grads"][k]])
        opt.step()
        sched.step()
    got = [[_storage(p), _storage(opt.state[p]["exp_avg"]), _storage(opt.state[p]["exp_avg_sq"])] for p in params]
    for x, name in enumerate(STATE_NAMES):
        err = max(float(np.abs(g[x].astype(np.float64) - w[x]).max()) for g, w in zip(got, ref["r64"]))
        print(f"{name}: E32 = {ref['e32'][x]:.3e}, max|device - step64| = {err:.3e}")
        assert err <= 4 * ref["e32"][x], (name, err, ref["e32"][x])
        for i, (g, w) in enumerate(zip(got, ref["r32"])):
            _assert_same(g[x], w[x], f"{name} of tensor {i} (n = {SIZES[i]})")


# ------------------------------------------------------------------------------------------------------------------------ h
@pytest.mark.gpu
def test_flat_adamw_on_the_trainers_gradient_bucket():
    """(h) The layout the Trainer steps: every parameter of TomoSAR2Height (U-Net depth 4, channels_last), gradients living in
    trainer.GradBucket's 4-float-padded views of one flat buffer.  3 steps, the last with zero_grad=True: every parameter and
    moment byte equal to step32, the bucket's padding floats untouched while zero_grad is off, the whole bucket +0.0 after."""
    from detinit import det_init_
    from tomosar2height_amd import TomoSAR2Height
    from tomosar2height_amd.optim import FlatAdamW
    from tomosar2height_amd.trainer import GradBucket
    cfg = berlin_config()
    cfg.model.encoder_kwargs.unet_kwargs.depth = 4
    model = det_init_(TomoSAR2Height(cfg), seed=21).to(_dev())
    model.set_channels_last(True)
    params = list(model.parameters())
    assert any(not p.is_contiguous() for p in params) and any(p.numel() % 4 for p in params)
    gen = torch.Generator().manual_seed(8)

    def fill(first):
        for p in params:
            g = torch.empty_like(p).copy_(torch.randn(p.shape, generator=gen).to(_dev()))
            if first:
                p.grad = g
            else:
                p.grad.copy_(g)

    fill(True)
    bucket = GradBucket(params)
    assert len(bucket.params) == len(params)
    pad = np.ones(bucket.flat.numel(), bool)
    off = 0
    for p in bucket.params:
        assert p.grad.data_ptr() == bucket.flat.data_ptr() + 4 * off and p.grad.stride() == p.stride()
        pad[off:off + p.numel()] = False
        off += -(-p.numel() // 4) * 4
    assert off == pad.size and pad.any()
    pad_dev = torch.from_numpy(pad).to(_dev())
    bucket.flat[pad_dev] = float(CANARY)
    opt = FlatAdamW(params, **HYPER)
    mir = _Mirror(opt)
    for k in range(2):
        if k:
            fill(False)
        mir.step(tag=f"step {k + 1}")
        assert (_bits(bucket.flat.cpu().numpy())[pad] == _bits(CANARY)).all(), "a padding float of the bucket was written"
    bucket.flat[pad_dev] = 0.0                               # as the Trainer's bucket has them
    fill(False)
    assert bucket.flat.count_nonzero().item() > 0.99 * (~pad).sum()
    mir.step(zero_grad=True, tag="step 3")
    assert not _bits(bucket.flat.cpu().numpy()).any()
    assert opt._plans[0]["n_chunks"] == sum(-(-p.numel() // CHUNK) for p in params)
