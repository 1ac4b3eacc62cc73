"""-m gpu: the 1-tap split products (csrc/conv_bx3.hip, ``t2h_gemm_bx3``) on a compact matrix, whose workgroups are ordered over the
row tiles IN USE instead of over the dense grid.  Only which workgroup computes which tile changes, so with a row count the product
must equal, bit for bit over the rows in use, the same entry point's dense product of a matrix whose rows behind the count are zero
(the last partial tile stages them as zeros, and a staged value takes part in the tile's fp16 block scale).

Cases: M = 1024 rows (eight 128-row tiles), K = 64, N = 64 (one column tile: the plain form) and N = 576 (nine 64-wide column tiles:
the persistent form under the fp16 two-way split, the plain form under the bf16 three-way split -- the recorded kernel symbols are
asserted), as ``linear_fwd`` (weight [N, K], with a bias) and as ``linear_dgrad`` (weight [K, N]), row counts 0, 1, 127, 128, 129, 511,
1023, 1024.  The operand rows behind the count are NaN and every output starts as NaN: a tile nobody computed, or a row staged from
behind the count, shows.  Output rows behind the last partial 128-row tile must keep their NaN; inside that tile the kernel may leave
anything.

``large``: M = 262 144, K = N = 64 with 69 % of the rows in use -- 1024 tiles of 256 rows (the 8-row form takes over at this size), the
large-grid index arithmetic.  ``uneven``: M = 65 536, N = 704 -- 512 row tiles, so the persistent form walks its eleven column tiles in
four groups of 3, 3, 3 and 2.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

LIMITS = (0, 1, 127, 128, 129, 511, 1023, 1024)


def _dev():
    return torch.device("cuda:0")


@pytest.fixture
def precision():
    from tomosar2height_amd import grid

    def use(name):
        grid.set_conv_precision(name)
    yield use
    grid.set_conv_precision(None)


def _operands(m, k, n, form, seed):
    """x [m, k], the weight as the form stores it, a bias for the forward form."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(m, k, generator=g) * torch.exp2(torch.randint(-3, 4, (m, 1), generator=g).float())      # rows of unlike size
    w = torch.randn((n, k) if form == "fwd" else (k, n), generator=g) / 8
    bias = torch.randn(n, generator=g) if form == "fwd" else None
    return x.to(_dev()), w.to(_dev()), None if bias is None else bias.to(_dev())


def _product(x, w, bias, form, n, row_limit=None):
    from tomosar2height_amd import mlp
    y = torch.full((x.shape[0], n), float("nan"), device=_dev())
    return mlp._gemm_bx3(x, w, form == "dgrad", bias, None, y, False, False, f"t2h_linear_{form}[test]", row_limit)


def _check(x, w, bias, form, n, lim, tile_rows):
    """The product with the row count ``lim`` against the dense product of the zero-padded matrix."""
    m = x.shape[0]
    x_c, x_d = x.clone(), x.clone()
    x_c[lim:] = float("nan")
    x_d[lim:] = 0.0
    count = torch.tensor([lim], dtype=torch.int32, device=_dev())
    got = _product(x_c, w, bias, form, n, count.data_ptr())
    ref = _product(x_d, w, bias, form, n)
    torch.cuda.synchronize()
    assert torch.isfinite(ref).all()
    assert torch.equal(got[:lim], ref[:lim]), f"rows in use differ at row count {lim}"
    behind = -(-lim // tile_rows) * tile_rows
    assert torch.isnan(got[min(behind, m):]).all(), f"a tile behind the rows in use was written at row count {lim}"


@pytest.mark.parametrize("n", [64, 576])
@pytest.mark.parametrize("form", ["fwd", "dgrad"])
@pytest.mark.parametrize("prec,npl", [("f16x2", 2), ("bf16x3", 3)])
def test_rows_in_use_bit_identical(prec, npl, form, n, precision):
    from tomosar2height_amd import _lib
    precision(prec)
    x, w, bias = _operands(1024, 64, n, form, seed=n + npl)
    with _lib.KernelTimeline() as tl:
        for lim in LIMITS:
            _check(x, w, bias, form, n, lim, 128)
    symbols = {rec[5] for rec in tl.records if rec[0].startswith("t2h_linear_")}
    persist = npl == 2 and n == 576
    assert symbols == {f"bx3_rows_kernel<4,64,4,1,64,{npl},1,0,{'true' if persist else 'false'}>"}, symbols


def test_rows_in_use_large_grid(precision):
    """M = 262 144: the tile index of the last tile in use is far from the first workgroups' -- 64-bit and unsigned arithmetic."""
    from tomosar2height_amd import _lib
    precision("f16x2")
    m = 262144
    x, w, bias = _operands(m, 64, 64, "fwd", seed=1)
    with _lib.KernelTimeline() as tl:
        _check(x, w, bias, "fwd", 64, int(0.69 * m), 256)
    assert {rec[5] for rec in tl.records if rec[0].startswith("t2h_linear_")} == {"bx3_rows_kernel<8,64,4,1,32,2,1,0,false>"}


def test_rows_in_use_uneven_column_groups(precision):
    """M = 65 536, N = 704 (eleven 64-wide column tiles): the persistent form with column groups of 3, 3, 3 and 2 tiles."""
    from tomosar2height_amd import _lib
    precision("f16x2")
    m = 65536
    x, w, bias = _operands(m, 64, 704, "fwd", seed=2)
    with _lib.KernelTimeline() as tl:
        _check(x, w, bias, "fwd", 704, int(0.69 * m), 128)
    assert {rec[5] for rec in tl.records if rec[0].startswith("t2h_linear_")} == {"bx3_rows_kernel<4,64,4,1,64,2,1,0,true>"}
