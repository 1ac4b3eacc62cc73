"""-m gpu: every grid-side launch of the benchmarked step, replayed alone against float64.

The headline number is ``Trainer.train_step`` on the cloud-only Berlin network with four tiles coalesced per forward / backward.
Which kernel a layer runs on is decided by host code from (B, H, W, Cin, Cout) -- ``bx3_rows_plan`` / ``launch_rows`` /
``bx3_wgrad_plan`` of csrc/conv_bx3.hip, the GEMM dispatch of csrc/gemm.hip -- and the hand-picked shapes of the per-kernel float64
tests do not reach the plans the benchmark runs (8-row tiles, the persistent column-group form, 2^20-pixel reductions, B = 4).

``ROWS_B4`` / ``ROWS_B1`` below list every grid-side launch of one benchmarked window (four tiles per pass) and of one strict
``T2H_COALESCE_TILES=1`` step: (family, shape, epilogue of the call site, what the call site's inputs look like, kernel symbol as
``_lib.KernelTimeline`` records it).  They were written down from a live window of this tree.

  * ``test_row``                 one launch per row, called the way grid.py / mlp.py call it, under a KernelTimeline: the recorded symbol is
                                 the row's, and the whole result is compared with the same operation in float64.
  * ``test_window_launches...``  builds the benchmarked trainer, records a window and asserts that its grid-side launches ARE the table
                                 (both directions); prints the point-side (tag, symbol) list, about which nothing is asserted here.

Inputs: seeded randn, weights scaled by 1 / sqrt(fan_in); image b of a batch is scaled by 2^(-6 b) and judged against its OWN norm (a
halo read from the neighbouring image, or a block scale taken across an image border, then fails); call sites behind a ReLU get
relu(randn), masked gradients randn times a 0/1 mask, masks both signs and exact zeros.

Bounds, both must hold:
  (a) the max-norm bounds of the per-kernel files: 2e-5 forward / data gradient (tests/test_hip_conv.py, tests/test_hip_gemm.py),
      1e-4 for the convolution weight / bias gradients (as test_conv3x3_at_bench_sizes judges 2^18-pixel reductions), 3e-5 for the
      linear weight gradients (tests/test_hip_gemm.py);
  (b) per output |got - ref64| <= c S, S = the same operation on |a|, |b| in float64, c = max(floor, 4 e32) where e32 is the largest
      |ref32 - ref64| / S of torch's CPU fp32 evaluation of the same row (an independent fp32 accumulation in another order; the factor
      4 covers two fp32 summation orders) and floor = 2^-21 (the documented contract of the fp16 two-way split, test_f16x2_block_scales)
      or 4e-7 for the exact bf16 three-way split (test_conv3x3_bx3_error_is_fp32_grade).  The code under test never sets its bound.
The bf16 arithmetic (BASELINE configs[2]) is judged as test_conv3x3_bf16_mode judges it: 1e-2 of the max-norm, and more than 2e-5.

The float64 reference of a row above ``CPU64_MAX_FLOPS`` is evaluated with torch's float64 matmul on the device (torch's own library,
which the product never calls); the smallest row of every family runs BOTH and asserts that they agree to 1e-12 of the max-norm.

What the rows found: on the exact three-way bf16 split seven 3 x 3 rows (reductions of 9 * 128 .. 9 * 512 terms) reached 4.3 .. 5.6e-7 of
sum |a b| against the floor 4e-7, where torch's CPU fp32 run of the same rows has 0.8e-7: all six piece products of a step went through
the running accumulator, six roundings per step at its size.  csrc/conv_bx3.hip now sums a step's pieces in a fresh accumulator and
joins it with one addition (3 x 3 form): the same rows measure <= 1.7e-7.

Notes.  e32 is taken per row (finer than per family and reduction length); it is the maximum over all outputs of ONE CPU fp32 run, so c
follows that run's worst output (up to 1.8e-6 on linear rows).  The input kinds of a row (post-ReLU input, masked gradient) were read
off the live window's tensors when the table was written; the closure test checks shapes, epilogues and symbols, not those.  The weight
gradients pass defer=True as grid.py / mlp.py do; the benchmarked trainer runs them on its side streams, where no ``_lib.reduce_capture``
is active (trainer.py: batched reductions only without side streams), so the flag stays clear in the window as in the replay -- the
table carries defer=False and both tests assert it.  ``bx3_wgrad_kernel`` and the 1-tap forms are not run in bf16x3 by any row.

``t2h_head1x1_bwd`` is checked for its VALUES here; the byte model grid.py reports for it to the roofline table is not.
"""
import math
import zlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (family, dims, epilogue of the call site, inputs of the call site, kernel symbol)
#   conv3x3_* / upconv2x2_*: dims = (B, H, W, Cin, Cout) of the layer (H, W: the INPUT plane of the transposed convolution)
#   linear_fwd:   (M, K, N, ldx, ldy)     y [M, N]  = x [M, K] w[N, K]^T
#   linear_dgrad: (M, N, K, lddy, lddx)   dx [M, K] = dy [M, N] w[N, K]
#   linear_wgrad: (M, K, N, lddy, ldx)    dw [N, K] = dy [M, N]^T x [M, K]
#   ``addend`` on a linear_fwd row: the launch is grid._Conv1x1's (t2h_linear_fwd_add; addend=False: that entry without an addend)
ROWS_B4 = [
    ("conv3x3_dgrad", (4, 128, 128, 128, 128), dict(accumulate=False, mask=True, rank1=False), dict(g_sparse=True), "bx3_rows_kernel<4,128,2,2,32,2,9,0,false>"),
    ("conv3x3_dgrad", (4, 128, 128, 256, 128), dict(accumulate=False, mask=False, rank1=False), dict(g_sparse=True), "bx3_rows_kernel<4,128,2,2,32,2,9,0,false>"),
    ("conv3x3_dgrad", (4, 128, 128, 64, 128), dict(accumulate=False, mask=False, rank1=False), dict(g_sparse=True), "bx3_rows_kernel<4,64,4,1,32,2,9,0,false>"),
    ("conv3x3_dgrad", (4, 256, 256, 128, 64), dict(accumulate=False, mask=False, rank1=False), dict(g_sparse=True), "bx3_rows_kernel<8,128,2,2,16,2,9,0,false>"),
    ("conv3x3_dgrad", (4, 256, 256, 32, 32), dict(accumulate=False, mask=False, rank1=False), dict(g_sparse=True), "bx3_rows_kernel<8,32,4,1,16,2,9,0,false>"),
    ("conv3x3_dgrad", (4, 256, 256, 32, 32), dict(accumulate=False, mask=True, rank1=False), dict(g_sparse=True), "bx3_rows_kernel<8,32,4,1,16,2,9,0,false>"),
    ("conv3x3_dgrad", (4, 256, 256, 32, 64), dict(accumulate=False, mask=False, rank1=False), dict(g_sparse=True), "bx3_rows_kernel<8,32,4,1,16,2,9,0,false>"),
    ("conv3x3_dgrad", (4, 256, 256, 64, 32), dict(accumulate=False, mask=False, rank1=False), dict(g_sparse=True), "bx3_rows_kernel<8,64,4,1,16,2,9,0,false>"),
    ("conv3x3_dgrad", (4, 256, 256, 64, 64), dict(accumulate=False, mask=True, rank1=False), dict(g_sparse=True), "bx3_rows_kernel<8,64,4,1,16,2,9,0,false>"),
    ("conv3x3_dgrad", (4, 32, 32, 256, 512), dict(accumulate=False, mask=False, rank1=False), dict(g_sparse=True), "bx3_rows_kernel<4,128,2,2,32,2,9,0,false>"),
    ("conv3x3_dgrad", (4, 32, 32, 512, 512), dict(accumulate=False, mask=True, rank1=False), dict(g_sparse=True), "bx3_rows_kernel<4,128,2,2,32,2,9,0,false>"),
    ("conv3x3_dgrad", (4, 512, 512, 128, 64), dict(accumulate=False, mask=True, rank1=True), dict(g_sparse=True), "bx3_rows_kernel<8,128,2,2,16,2,9,0,false>"),
    ("conv3x3_dgrad", (4, 512, 512, 32, 64), dict(accumulate=False, mask=False, rank1=True), dict(g_sparse=True), "bx3_rows_kernel<8,32,4,1,16,2,9,0,false>"),
    ("conv3x3_dgrad", (4, 512, 512, 64, 128), dict(accumulate=False, mask=True, rank1=True), dict(g_sparse=True), "bx3_rows_kernel<8,64,4,1,16,2,9,0,false>"),
    ("conv3x3_dgrad", (4, 64, 64, 128, 256), dict(accumulate=False, mask=False, rank1=False), dict(g_sparse=True), "bx3_rows_kernel<4,128,2,2,32,2,9,0,false>"),
    ("conv3x3_dgrad", (4, 64, 64, 256, 256), dict(accumulate=False, mask=True, rank1=False), dict(g_sparse=True), "bx3_rows_kernel<4,128,2,2,32,2,9,0,false>"),
    ("conv3x3_dgrad", (4, 64, 64, 512, 256), dict(accumulate=False, mask=False, rank1=False), dict(g_sparse=True), "bx3_rows_kernel<4,128,2,2,32,2,9,0,false>"),
    ("conv3x3_fwd", (4, 128, 128, 128, 128), dict(accumulate=False, bias=True, relu=True), dict(x_relu=True), "bx3_rows_kernel<4,128,2,2,32,2,9,0,false>"),
    ("conv3x3_fwd", (4, 128, 128, 256, 128), dict(accumulate=False, bias=True, relu=True), dict(x_relu=False), "bx3_rows_kernel<4,128,2,2,32,2,9,0,false>"),
    ("conv3x3_fwd", (4, 128, 128, 64, 128), dict(accumulate=False, bias=True, relu=True), dict(x_relu=False), "bx3_rows_kernel<4,128,2,2,32,2,9,0,false>"),
    ("conv3x3_fwd", (4, 256, 256, 128, 64), dict(accumulate=False, bias=True, relu=True), dict(x_relu=False), "bx3_rows_kernel<8,64,4,1,16,2,9,0,false>"),
    ("conv3x3_fwd", (4, 256, 256, 32, 32), dict(accumulate=False, bias=True, relu=True), dict(x_relu=True), "bx3_rows_kernel<8,32,4,1,16,2,9,0,false>"),
    ("conv3x3_fwd", (4, 256, 256, 32, 64), dict(accumulate=False, bias=True, relu=True), dict(x_relu=False), "bx3_rows_kernel<8,64,4,1,16,2,9,0,false>"),
    ("conv3x3_fwd", (4, 256, 256, 64, 32), dict(accumulate=False, bias=True, relu=True), dict(x_relu=False), "bx3_rows_kernel<8,32,4,1,16,2,9,0,false>"),
    ("conv3x3_fwd", (4, 256, 256, 64, 64), dict(accumulate=False, bias=True, relu=True), dict(x_relu=True), "bx3_rows_kernel<8,64,4,1,16,2,9,0,false>"),
    ("conv3x3_fwd", (4, 32, 32, 256, 512), dict(accumulate=False, bias=True, relu=True), dict(x_relu=False), "bx3_rows_kernel<4,128,2,2,32,2,9,0,false>"),
    ("conv3x3_fwd", (4, 32, 32, 512, 512), dict(accumulate=False, bias=True, relu=True), dict(x_relu=True), "bx3_rows_kernel<4,128,2,2,32,2,9,0,false>"),
    ("conv3x3_fwd", (4, 512, 512, 128, 64), dict(accumulate=False, bias=True, relu=True), dict(x_relu=True), "bx3_rows_kernel<8,64,4,1,16,2,9,0,false>"),
    ("conv3x3_fwd", (4, 512, 512, 32, 64), dict(accumulate=False, bias=True, relu=True), dict(x_relu=False), "bx3_rows_kernel<8,64,4,1,16,2,9,0,false>"),
    ("conv3x3_fwd", (4, 512, 512, 64, 128), dict(accumulate=False, bias=True, relu=True), dict(x_relu=True), "bx3_rows_kernel<8,128,2,2,16,2,9,0,false>"),
    ("conv3x3_fwd", (4, 64, 64, 128, 256), dict(accumulate=False, bias=True, relu=True), dict(x_relu=False), "bx3_rows_kernel<4,128,2,2,32,2,9,0,false>"),
    ("conv3x3_fwd", (4, 64, 64, 256, 256), dict(accumulate=False, bias=True, relu=True), dict(x_relu=True), "bx3_rows_kernel<4,128,2,2,32,2,9,0,false>"),
    ("conv3x3_fwd", (4, 64, 64, 512, 256), dict(accumulate=False, bias=True, relu=True), dict(x_relu=False), "bx3_rows_kernel<4,128,2,2,32,2,9,0,false>"),
    ("conv3x3_wgrad", (4, 128, 128, 128, 128), dict(accumulate=True, db=True, defer=False), dict(g_sparse=True, x_relu=True), "bx3_wgrad_kernel<4,2,false,0>"),
    ("conv3x3_wgrad", (4, 128, 128, 256, 128), dict(accumulate=True, db=True, defer=False), dict(g_sparse=True, x_relu=False), "bx3_wgrad_kernel<4,2,false,0>"),
    ("conv3x3_wgrad", (4, 128, 128, 64, 128), dict(accumulate=True, db=True, defer=False), dict(g_sparse=True, x_relu=False), "bx3_wgrad_kernel<4,2,false,0>"),
    ("conv3x3_wgrad", (4, 256, 256, 128, 64), dict(accumulate=True, db=True, defer=False), dict(g_sparse=True, x_relu=False), "bx3_wgrad_kernel<2,2,false,0>"),
    ("conv3x3_wgrad", (4, 256, 256, 32, 32), dict(accumulate=True, db=True, defer=False), dict(g_sparse=True, x_relu=True), "bx3_wgrad_kernel<1,2,false,0>"),
    ("conv3x3_wgrad", (4, 256, 256, 32, 64), dict(accumulate=True, db=True, defer=False), dict(g_sparse=True, x_relu=False), "bx3_wgrad_kernel<2,2,false,0>"),
    ("conv3x3_wgrad", (4, 256, 256, 64, 32), dict(accumulate=True, db=True, defer=False), dict(g_sparse=True, x_relu=False), "bx3_wgrad_kernel<1,2,false,0>"),
    ("conv3x3_wgrad", (4, 256, 256, 64, 64), dict(accumulate=True, db=True, defer=False), dict(g_sparse=True, x_relu=True), "bx3_wgrad_kernel<2,2,false,0>"),
    ("conv3x3_wgrad", (4, 32, 32, 256, 512), dict(accumulate=True, db=True, defer=False), dict(g_sparse=True, x_relu=False), "bx3_wgrad_kernel<4,2,false,0>"),
    ("conv3x3_wgrad", (4, 32, 32, 512, 512), dict(accumulate=True, db=True, defer=False), dict(g_sparse=True, x_relu=True), "bx3_wgrad_kernel<4,2,false,0>"),
    ("conv3x3_wgrad", (4, 512, 512, 128, 64), dict(accumulate=True, db=True, defer=False), dict(g_sparse=True, x_relu=True), "bx3_wgrad_kernel<2,2,false,0>"),
    ("conv3x3_wgrad", (4, 512, 512, 32, 64), dict(accumulate=True, db=True, defer=False), dict(g_sparse=True, x_relu=False), "bx3_wgrad_kernel<2,2,false,0>"),
    ("conv3x3_wgrad", (4, 512, 512, 64, 128), dict(accumulate=True, db=True, defer=False), dict(g_sparse=True, x_relu=True), "bx3_wgrad_kernel<4,2,false,0>"),
    ("conv3x3_wgrad", (4, 64, 64, 128, 256), dict(accumulate=True, db=True, defer=False), dict(g_sparse=True, x_relu=False), "bx3_wgrad_kernel<4,2,false,0>"),
    ("conv3x3_wgrad", (4, 64, 64, 256, 256), dict(accumulate=True, db=True, defer=False), dict(g_sparse=True, x_relu=True), "bx3_wgrad_kernel<4,2,false,0>"),
    ("conv3x3_wgrad", (4, 64, 64, 512, 256), dict(accumulate=True, db=True, defer=False), dict(g_sparse=True, x_relu=False), "bx3_wgrad_kernel<4,2,false,0>"),
    ("head1x1_bwd", (1048576,), dict(flags=3586), dict(), "t2h_head1x1_bwd"),
    ("head1x1_fwd", (1048576,), dict(bias=True), dict(), "t2h_head1x1_fwd"),
    ("linear_dgrad", (16384, 2368, 256, 2752, 256), dict(accumulate=False, bias=False, bx3=True, ldm=0, mask=False, relu_out=False), dict(x_relu=False), "bx3_rows_kernel<4,128,2,2,64,2,1,0,false>"),
    ("linear_dgrad", (16384, 256, 128, 256, 128), dict(accumulate=False, bx3=False, ldm=0, mask=False), dict(g_sparse=False), "gemm_kernel<64,64,2,2,true,false,32,true,1,0>"),
    ("linear_dgrad", (16384, 512, 256, 512, 256), dict(accumulate=True, bx3=False, ldm=0, mask=False), dict(g_sparse=True), "gemm_dma_nn_kernel"),
    ("linear_dgrad", (16384, 832, 256, 2752, 256), dict(accumulate=False, bias=False, bx3=True, ldm=0, mask=False, relu_out=False), dict(x_relu=False), "bx3_rows_kernel<4,128,2,2,64,2,1,0,false>"),
    ("linear_dgrad", (262144, 128, 64, 128, 64), dict(accumulate=True, bx3=False, ldm=0, mask=False), dict(g_sparse=True), "gemm_kernel<128,64,2,2,true,false,16,true,1,0>"),
    ("linear_dgrad", (262144, 2752, 64, 2752, 64), dict(accumulate=False, bias=False, bx3=True, ldm=0, mask=False, relu_out=False), dict(x_relu=False), "bx3_rows_kernel<8,64,4,1,32,2,1,0,false>"),
    ("linear_dgrad", (262144, 32, 32, 32, 32), dict(accumulate=False, bx3=False, ldm=0, mask=False), dict(g_sparse=False), "gemm_kernel<128,32,4,1,true,false,16,true,1,0>"),
    ("linear_dgrad", (262144, 32, 64, 32, 64), dict(accumulate=False, bx3=False, ldm=0, mask=False), dict(g_sparse=False), "gemm_kernel<128,64,2,2,true,false,16,true,1,0>"),
    ("linear_dgrad", (262144, 32, 64, 64, 64), dict(accumulate=False, bx3=False, ldm=0, mask=False), dict(g_sparse=False), "gemm_kernel<128,64,2,2,true,false,16,true,1,0>"),
    ("linear_dgrad", (262144, 64, 32, 64, 32), dict(accumulate=False, bx3=False, ldm=0, mask=False), dict(g_sparse=False), "gemm_kernel<128,32,4,1,true,false,16,true,1,0>"),
    ("linear_dgrad", (4096, 1024, 512, 1024, 512), dict(accumulate=True, bx3=False, ldm=0, mask=False), dict(g_sparse=True), "gemm_kernel<64,64,2,2,true,false,32,true,1,0>"),
    ("linear_dgrad", (4096, 1856, 512, 2752, 512), dict(accumulate=False, bias=False, bx3=True, ldm=0, mask=False, relu_out=False), dict(x_relu=False), "bx3_rows_kernel<4,128,2,2,64,2,1,0,false>"),
    ("linear_dgrad", (4096, 512, 256, 512, 256), dict(accumulate=False, bx3=False, ldm=0, mask=False), dict(g_sparse=False), "gemm_kwaves_kernel<true,false>"),
    ("linear_dgrad", (524288, 128, 64, 128, 64), dict(accumulate=False, bx3=False, ldm=0, mask=False), dict(g_sparse=True), "gemm_kernel<128,64,2,2,true,false,16,true,1,0>"),
    ("linear_dgrad", (524288, 32, 32, 32, 32), dict(accumulate=False, bx3=False, ldm=0, mask=False), dict(g_sparse=False), "gemm_kernel<128,32,4,1,true,false,16,true,1,0>"),
    ("linear_dgrad", (524288, 32, 64, 32, 64), dict(accumulate=False, bx3=False, ldm=64, mask=True), dict(g_sparse=False), "gemm_kernel<128,64,2,2,true,false,16,true,1,0>"),
    ("linear_dgrad", (524288, 64, 128, 64, 128), dict(accumulate=False, bx3=False, ldm=128, mask=True), dict(g_sparse=False), "gemm_dma_nn_kernel"),
    ("linear_dgrad", (524288, 64, 32, 64, 32), dict(accumulate=False, bx3=False, ldm=0, mask=False), dict(g_sparse=True), "gemm_kernel<128,32,4,1,true,false,16,true,1,0>"),
    ("linear_dgrad", (65536, 128, 64, 128, 64), dict(accumulate=False, bx3=False, ldm=0, mask=False), dict(g_sparse=False), "gemm_kernel<128,64,2,2,true,false,16,true,1,0>"),
    ("linear_dgrad", (65536, 256, 128, 256, 128), dict(accumulate=True, bx3=False, ldm=0, mask=False), dict(g_sparse=True), "gemm_dma_nn_kernel"),
    ("linear_dgrad", (65536, 2624, 128, 2752, 128), dict(accumulate=False, bias=False, bx3=True, ldm=0, mask=False, relu_out=False), dict(x_relu=False), "bx3_rows_kernel<4,128,2,2,64,2,1,0,false>"),
    ("linear_dgrad", (65536, 320, 128, 2752, 128), dict(accumulate=False, bias=False, bx3=True, ldm=0, mask=False, relu_out=False), dict(x_relu=False), "bx3_rows_kernel<4,128,2,2,64,2,1,0,false>"),
    ("linear_fwd", (16384, 128, 256, 128, 256), dict(accumulate=False, addend=True, bias=True, bx3=False, relu_in=False, relu_out=False), dict(x_relu=False), "gemm_dma_kernel"),
    ("linear_fwd", (16384, 256, 2368, 256, 2752), dict(accumulate=False, bias=False, bx3=True, ldm=0, mask=False, relu_out=False), dict(x_relu=False), "bx3_rows_kernel<8,64,4,1,32,2,1,0,false>"),
    ("linear_fwd", (16384, 256, 512, 256, 512), dict(accumulate=False, bias=True, bx3=False, relu_in=False, relu_out=False), dict(x_relu=False), "gemm_dma_kernel"),
    ("linear_fwd", (16384, 256, 832, 256, 2752), dict(accumulate=True, bias=False, bx3=True, ldm=0, mask=False, relu_out=False), dict(x_relu=False), "bx3_rows_kernel<4,64,4,1,64,2,1,0,false>"),
    ("linear_fwd", (262144, 32, 32, 32, 32), dict(accumulate=False, addend=False, bias=True, bx3=False, relu_in=False, relu_out=False), dict(x_relu=False), "gemm_kernel<128,32,4,1,true,true,16,true,1,0>"),
    ("linear_fwd", (262144, 32, 64, 32, 64), dict(accumulate=False, addend=True, bias=True, bx3=False, relu_in=False, relu_out=False), dict(x_relu=True), "gemm_kernel<128,64,2,2,true,true,16,true,1,0>"),
    ("linear_fwd", (262144, 64, 128, 64, 128), dict(accumulate=False, bias=True, bx3=False, relu_in=False, relu_out=False), dict(x_relu=False), "gemm_dma_kernel"),
    ("linear_fwd", (262144, 64, 2752, 64, 2752), dict(accumulate=False, bias=False, bx3=True, ldm=0, mask=False, relu_out=False), dict(x_relu=False), "bx3_rows_kernel<4,64,4,1,64,2,1,0,true>"),
    ("linear_fwd", (262144, 64, 32, 64, 32), dict(accumulate=False, addend=False, bias=True, bx3=False, relu_in=False, relu_out=False), dict(x_relu=False), "gemm_kernel<128,32,4,1,true,true,16,true,1,0>"),
    ("linear_fwd", (262144, 64, 32, 64, 32), dict(accumulate=False, addend=True, bias=True, bx3=False, relu_in=False, relu_out=False), dict(x_relu=False), "gemm_kernel<128,32,4,1,true,true,16,true,1,0>"),
    ("linear_fwd", (4096, 256, 512, 256, 512), dict(accumulate=False, addend=True, bias=True, bx3=False, relu_in=False, relu_out=False), dict(x_relu=False), "gemm_kernel<64,64,2,2,true,true,32,true,1,0>"),
    ("linear_fwd", (4096, 512, 1024, 512, 1024), dict(accumulate=False, bias=True, bx3=False, relu_in=False, relu_out=False), dict(x_relu=False), "gemm_dma_kernel"),
    ("linear_fwd", (4096, 512, 1856, 512, 2752), dict(accumulate=False, bias=False, bx3=True, ldm=0, mask=False, relu_out=False), dict(x_relu=False), "bx3_rows_kernel<4,64,4,1,64,2,1,0,false>"),
    ("linear_fwd", (524288, 128, 64, 128, 64), dict(accumulate=False, bias=True, bx3=False, relu_in=False, relu_out=False), dict(x_relu=True), "gemm_kernel<128,64,2,2,true,true,16,true,1,0>"),
    ("linear_fwd", (524288, 32, 32, 32, 32), dict(accumulate=True, bias=True, bx3=False, relu_in=False, relu_out=False), dict(x_relu=False), "gemm_kernel<128,32,4,1,true,true,16,true,1,0>"),
    ("linear_fwd", (524288, 32, 64, 32, 64), dict(accumulate=False, bias=True, bx3=False, relu_in=False, relu_out=True), dict(x_relu=True), "gemm_kernel<128,64,2,2,true,true,16,true,1,0>"),
    ("linear_fwd", (524288, 32, 64, 32, 64), dict(accumulate=True, bias=True, bx3=False, relu_in=False, relu_out=False), dict(x_relu=False), "gemm_kernel<128,64,2,2,true,true,16,true,1,0>"),
    ("linear_fwd", (524288, 64, 128, 64, 128), dict(accumulate=False, bias=True, bx3=False, relu_in=False, relu_out=True), dict(x_relu=False), "gemm_dma_kernel"),
    ("linear_fwd", (524288, 64, 32, 64, 32), dict(accumulate=False, bias=True, bx3=False, relu_in=False, relu_out=False), dict(x_relu=True), "gemm_kernel<128,32,4,1,true,true,16,true,1,0>"),
    ("linear_fwd", (65536, 128, 256, 128, 256), dict(accumulate=False, bias=True, bx3=False, relu_in=False, relu_out=False), dict(x_relu=False), "gemm_dma_kernel"),
    ("linear_fwd", (65536, 128, 2624, 128, 2752), dict(accumulate=False, bias=False, bx3=True, ldm=0, mask=False, relu_out=False), dict(x_relu=False), "bx3_rows_kernel<8,64,4,1,32,2,1,0,false>"),
    ("linear_fwd", (65536, 128, 320, 128, 2752), dict(accumulate=True, bias=False, bx3=True, ldm=0, mask=False, relu_out=False), dict(x_relu=False), "bx3_rows_kernel<8,64,4,1,32,2,1,0,false>"),
    ("linear_fwd", (65536, 64, 128, 64, 128), dict(accumulate=False, addend=True, bias=True, bx3=False, relu_in=False, relu_out=False), dict(x_relu=False), "gemm_dma_kernel"),
    ("linear_wgrad", (16384, 128, 256, 256, 128), dict(accumulate=True, db=True, defer=False, relu_in=False), dict(x_relu=False), "gemm_dma_tn_kernel"),
    ("linear_wgrad", (16384, 256, 2368, 2752, 256), dict(accumulate=True, db=False, defer=False, relu_in=False), dict(x_relu=False), "gemm_dma_tn_kernel"),
    ("linear_wgrad", (16384, 256, 512, 512, 256), dict(accumulate=True, db=True, defer=False, relu_in=False), dict(x_relu=False), "gemm_dma_tn_kernel"),
    ("linear_wgrad", (16384, 256, 832, 2752, 256), dict(accumulate=True, db=False, defer=False, relu_in=False), dict(x_relu=False), "gemm_dma_tn_kernel"),
    ("linear_wgrad", (262144, 32, 32, 32, 32), dict(accumulate=True, db=True, defer=False, relu_in=False), dict(x_relu=False), "gemm_kernel<32,32,1,1,false,false,16,true,1,0>"),
    ("linear_wgrad", (262144, 32, 64, 64, 32), dict(accumulate=True, db=True, defer=False, relu_in=False), dict(x_relu=False), "gemm_kernel<64,32,2,1,false,false,16,true,1,0>"),
    ("linear_wgrad", (262144, 64, 128, 128, 64), dict(accumulate=True, db=True, defer=False, relu_in=False), dict(x_relu=False), "gemm_kernel<128,64,2,2,false,false,16,true,1,0>"),
    ("linear_wgrad", (262144, 64, 2752, 2752, 64), dict(accumulate=True, db=False, defer=False, relu_in=False), dict(x_relu=False), "gemm_kernel<128,64,2,2,false,false,16,true,1,0>"),
    ("linear_wgrad", (262144, 64, 32, 32, 64), dict(accumulate=True, db=True, defer=False, relu_in=False), dict(x_relu=False), "gemm_kernel<32,64,1,2,false,false,16,true,1,0>"),
    ("linear_wgrad", (262144, 64, 32, 64, 64), dict(accumulate=True, db=True, defer=False, relu_in=False), dict(x_relu=False), "gemm_kernel<32,64,1,2,false,false,16,true,1,0>"),
    ("linear_wgrad", (4096, 256, 512, 512, 256), dict(accumulate=True, db=True, defer=False, relu_in=False), dict(x_relu=False), "gemm_dma_tn_kernel"),
    ("linear_wgrad", (4096, 512, 1024, 1024, 512), dict(accumulate=True, db=True, defer=False, relu_in=False), dict(x_relu=False), "gemm_dma_tn_kernel"),
    ("linear_wgrad", (4096, 512, 1856, 2752, 512), dict(accumulate=True, db=False, defer=False, relu_in=False), dict(x_relu=False), "gemm_dma_tn_kernel"),
    ("linear_wgrad", (524288, 128, 64, 64, 128), dict(accumulate=True, db=True, defer=False, relu_in=False), dict(x_relu=True), "gemm_kernel<64,128,2,2,false,false,16,true,1,0>"),
    ("linear_wgrad", (524288, 32, 32, 32, 32), dict(accumulate=True, db=True, defer=False, relu_in=False), dict(x_relu=False), "gemm_kernel<32,32,1,1,false,false,16,true,1,0>"),
    ("linear_wgrad", (524288, 32, 64, 64, 32), dict(accumulate=True, db=True, defer=False, relu_in=False), dict(x_relu=True), "gemm_kernel<64,32,2,1,false,false,16,true,1,0>"),
    ("linear_wgrad", (524288, 64, 128, 128, 64), dict(accumulate=True, db=True, defer=False, relu_in=False), dict(x_relu=False), "gemm_kernel<128,64,2,2,false,false,16,true,1,0>"),
    ("linear_wgrad", (524288, 64, 32, 32, 64), dict(accumulate=True, db=True, defer=False, relu_in=False), dict(x_relu=True), "gemm_kernel<32,64,1,2,false,false,16,true,1,0>"),
    ("linear_wgrad", (65536, 128, 256, 256, 128), dict(accumulate=True, db=True, defer=False, relu_in=False), dict(x_relu=False), "gemm_dma_tn_kernel"),
    ("linear_wgrad", (65536, 128, 2624, 2752, 128), dict(accumulate=True, db=False, defer=False, relu_in=False), dict(x_relu=False), "gemm_dma_tn_kernel"),
    ("linear_wgrad", (65536, 128, 320, 2752, 128), dict(accumulate=True, db=False, defer=False, relu_in=False), dict(x_relu=False), "gemm_dma_tn_kernel"),
    ("linear_wgrad", (65536, 64, 128, 128, 64), dict(accumulate=True, db=True, defer=False, relu_in=False), dict(x_relu=False), "gemm_kernel<128,64,2,2,false,false,16,true,1,0>"),
    ("maxpool_bwd", (4, 128, 128, 128), dict(), dict(), "t2h_maxpool2x2_nhwc_bwd"),
    ("maxpool_bwd", (4, 256, 256, 64), dict(), dict(), "t2h_maxpool2x2_nhwc_bwd"),
    ("maxpool_bwd", (4, 64, 64, 256), dict(), dict(), "t2h_maxpool2x2_nhwc_bwd"),
    ("maxpool_bwd_add", (4, 128, 128, 128), dict(addend=True, ld=256), dict(), "t2h_maxpool2x2_nhwc_bwd_add"),
    ("maxpool_bwd_add", (4, 256, 256, 64), dict(addend=True, ld=128), dict(), "t2h_maxpool2x2_nhwc_bwd_add"),
    ("maxpool_bwd_add", (4, 64, 64, 256), dict(addend=True, ld=512), dict(), "t2h_maxpool2x2_nhwc_bwd_add"),
    ("maxpool_fwd", (4, 128, 128, 128), dict(), dict(), "t2h_maxpool2x2_nhwc_fwd"),
    ("maxpool_fwd", (4, 256, 256, 64), dict(), dict(), "t2h_maxpool2x2_nhwc_fwd"),
    ("maxpool_fwd", (4, 64, 64, 256), dict(), dict(), "t2h_maxpool2x2_nhwc_fwd"),
    ("relu_mask", (16777216,), dict(), dict(), "t2h_relu_mask"),
    ("relu_mask", (2097152,), dict(), dict(), "t2h_relu_mask"),
    ("relu_mask", (4194304,), dict(), dict(), "t2h_relu_mask"),
    ("relu_mask", (8388608,), dict(), dict(), "t2h_relu_mask"),
    ("upconv2x2_dgrad", (4, 128, 128, 128, 64), dict(lddy=128), dict(g_sparse=False), "bx3_rows_kernel<4,128,2,2,64,2,1,2,false>"),
    ("upconv2x2_dgrad", (4, 128, 128, 128, 64), dict(lddy=64), dict(g_sparse=False), "bx3_rows_kernel<4,128,2,2,64,2,1,2,false>"),
    ("upconv2x2_dgrad", (4, 32, 32, 512, 256), dict(lddy=256), dict(g_sparse=False), "bx3_rows_kernel<4,128,2,2,64,2,1,2,false>"),
    ("upconv2x2_dgrad", (4, 32, 32, 512, 256), dict(lddy=512), dict(g_sparse=False), "bx3_rows_kernel<4,128,2,2,64,2,1,2,false>"),
    ("upconv2x2_dgrad", (4, 64, 64, 256, 128), dict(lddy=128), dict(g_sparse=False), "bx3_rows_kernel<4,128,2,2,64,2,1,2,false>"),
    ("upconv2x2_dgrad", (4, 64, 64, 256, 128), dict(lddy=256), dict(g_sparse=False), "bx3_rows_kernel<4,128,2,2,64,2,1,2,false>"),
    ("upconv2x2_fwd", (4, 128, 128, 128, 64), dict(addend=False, bias=True), dict(x_relu=False), "bx3_rows_kernel<4,128,2,2,64,2,1,1,false>"),
    ("upconv2x2_fwd", (4, 128, 128, 128, 64), dict(addend=True, bias=True), dict(x_relu=False), "bx3_rows_kernel<4,128,2,2,64,2,1,1,false>"),
    ("upconv2x2_fwd", (4, 32, 32, 512, 256), dict(addend=False, bias=True), dict(x_relu=False), "bx3_rows_kernel<4,128,2,2,64,2,1,1,false>"),
    ("upconv2x2_fwd", (4, 32, 32, 512, 256), dict(addend=True, bias=True), dict(x_relu=False), "bx3_rows_kernel<4,128,2,2,64,2,1,1,false>"),
    ("upconv2x2_fwd", (4, 64, 64, 256, 128), dict(addend=False, bias=True), dict(x_relu=False), "bx3_rows_kernel<4,128,2,2,64,2,1,1,false>"),
    ("upconv2x2_fwd", (4, 64, 64, 256, 128), dict(addend=True, bias=True), dict(x_relu=False), "bx3_rows_kernel<4,128,2,2,64,2,1,1,false>"),
    ("upconv2x2_wgrad", (4, 128, 128, 128, 64), dict(accumulate=True, db=True, defer=False, lddy=128), dict(), "bx3_wgrad_kernel<4,2,true,0>"),
    ("upconv2x2_wgrad", (4, 128, 128, 128, 64), dict(accumulate=True, db=True, defer=False, lddy=64), dict(), "bx3_wgrad_kernel<4,2,true,0>"),
    ("upconv2x2_wgrad", (4, 32, 32, 512, 256), dict(accumulate=True, db=True, defer=False, lddy=256), dict(), "bx3_wgrad_kernel<4,2,true,0>"),
    ("upconv2x2_wgrad", (4, 32, 32, 512, 256), dict(accumulate=True, db=True, defer=False, lddy=512), dict(), "bx3_wgrad_kernel<4,2,true,0>"),
    ("upconv2x2_wgrad", (4, 64, 64, 256, 128), dict(accumulate=True, db=True, defer=False, lddy=128), dict(), "bx3_wgrad_kernel<4,2,true,0>"),
    ("upconv2x2_wgrad", (4, 64, 64, 256, 128), dict(accumulate=True, db=True, defer=False, lddy=256), dict(), "bx3_wgrad_kernel<4,2,true,0>"),
    ("upsample_bwd", (4, 32, 256, 256, 512, 512), dict(), dict(), "t2h_upsample_bilinear_nhwc_bwd"),
    ("upsample_fwd", (4, 32, 256, 256, 512, 512), dict(addend=False), dict(), "t2h_upsample_bilinear_nhwc_fwd"),
]

ROWS_B1 = [
    ("conv3x3_dgrad", (1, 128, 128, 128, 128), dict(accumulate=False, mask=True, rank1=False), dict(g_sparse=True), "bx3_rows_kernel<4,64,4,1,32,2,9,0,false>"),
    ("conv3x3_dgrad", (1, 128, 128, 256, 128), dict(accumulate=False, mask=False, rank1=False), dict(g_sparse=True), "bx3_rows_kernel<4,128,2,2,32,2,9,0,false>"),
    ("conv3x3_dgrad", (1, 128, 128, 64, 128), dict(accumulate=False, mask=False, rank1=False), dict(g_sparse=True), "bx3_rows_kernel<4,64,4,1,32,2,9,0,false>"),
    ("conv3x3_dgrad", (1, 256, 256, 128, 64), dict(accumulate=False, mask=False, rank1=False), dict(g_sparse=True), "bx3_rows_kernel<4,128,2,2,32,2,9,0,false>"),
    ("conv3x3_dgrad", (1, 256, 256, 32, 32), dict(accumulate=False, mask=False, rank1=False), dict(g_sparse=True), "bx3_rows_kernel<4,32,4,1,32,2,9,0,false>"),
    ("conv3x3_dgrad", (1, 256, 256, 32, 32), dict(accumulate=False, mask=True, rank1=False), dict(g_sparse=True), "bx3_rows_kernel<4,32,4,1,32,2,9,0,false>"),
    ("conv3x3_dgrad", (1, 256, 256, 32, 64), dict(accumulate=False, mask=False, rank1=False), dict(g_sparse=True), "bx3_rows_kernel<4,32,4,1,32,2,9,0,false>"),
    ("conv3x3_dgrad", (1, 256, 256, 64, 32), dict(accumulate=False, mask=False, rank1=False), dict(g_sparse=True), "bx3_rows_kernel<4,64,4,1,32,2,9,0,false>"),
    ("conv3x3_dgrad", (1, 256, 256, 64, 64), dict(accumulate=False, mask=True, rank1=False), dict(g_sparse=True), "bx3_rows_kernel<4,64,4,1,32,2,9,0,false>"),
    ("conv3x3_dgrad", (1, 32, 32, 256, 512), dict(accumulate=False, mask=False, rank1=False), dict(g_sparse=True), "bx3_rows_kernel<4,128,2,2,32,2,9,0,false>"),
    ("conv3x3_dgrad", (1, 32, 32, 512, 512), dict(accumulate=False, mask=True, rank1=False), dict(g_sparse=True), "bx3_rows_kernel<4,128,2,2,32,2,9,0,false>"),
    ("conv3x3_dgrad", (1, 512, 512, 128, 64), dict(accumulate=False, mask=True, rank1=True), dict(g_sparse=True), "bx3_rows_kernel<8,128,2,2,16,2,9,0,false>"),
    ("conv3x3_dgrad", (1, 512, 512, 32, 64), dict(accumulate=False, mask=False, rank1=True), dict(g_sparse=True), "bx3_rows_kernel<8,32,4,1,16,2,9,0,false>"),
    ("conv3x3_dgrad", (1, 512, 512, 64, 128), dict(accumulate=False, mask=True, rank1=True), dict(g_sparse=True), "bx3_rows_kernel<8,64,4,1,16,2,9,0,false>"),
    ("conv3x3_dgrad", (1, 64, 64, 128, 256), dict(accumulate=False, mask=False, rank1=False), dict(g_sparse=True), "bx3_rows_kernel<4,128,2,2,32,2,9,0,false>"),
    ("conv3x3_dgrad", (1, 64, 64, 256, 256), dict(accumulate=False, mask=True, rank1=False), dict(g_sparse=True), "bx3_rows_kernel<4,128,2,2,32,2,9,0,false>"),
    ("conv3x3_dgrad", (1, 64, 64, 512, 256), dict(accumulate=False, mask=False, rank1=False), dict(g_sparse=True), "bx3_rows_kernel<4,128,2,2,32,2,9,0,false>"),
    ("conv3x3_fwd", (1, 128, 128, 128, 128), dict(accumulate=False, bias=True, relu=True), dict(x_relu=True), "bx3_rows_kernel<4,64,4,1,32,2,9,0,false>"),
    ("conv3x3_fwd", (1, 128, 128, 256, 128), dict(accumulate=False, bias=True, relu=True), dict(x_relu=False), "bx3_rows_kernel<4,128,2,2,32,2,9,0,false>"),
    ("conv3x3_fwd", (1, 128, 128, 64, 128), dict(accumulate=False, bias=True, relu=True), dict(x_relu=False), "bx3_rows_kernel<4,64,4,1,32,2,9,0,false>"),
    ("conv3x3_fwd", (1, 256, 256, 128, 64), dict(accumulate=False, bias=True, relu=True), dict(x_relu=False), "bx3_rows_kernel<4,64,4,1,32,2,9,0,false>"),
    ("conv3x3_fwd", (1, 256, 256, 32, 32), dict(accumulate=False, bias=True, relu=True), dict(x_relu=True), "bx3_rows_kernel<4,32,4,1,32,2,9,0,false>"),
    ("conv3x3_fwd", (1, 256, 256, 32, 64), dict(accumulate=False, bias=True, relu=True), dict(x_relu=False), "bx3_rows_kernel<4,64,4,1,32,2,9,0,false>"),
    ("conv3x3_fwd", (1, 256, 256, 64, 32), dict(accumulate=False, bias=True, relu=True), dict(x_relu=False), "bx3_rows_kernel<4,32,4,1,32,2,9,0,false>"),
    ("conv3x3_fwd", (1, 256, 256, 64, 64), dict(accumulate=False, bias=True, relu=True), dict(x_relu=True), "bx3_rows_kernel<4,64,4,1,32,2,9,0,false>"),
    ("conv3x3_fwd", (1, 32, 32, 256, 512), dict(accumulate=False, bias=True, relu=True), dict(x_relu=False), "bx3_rows_kernel<4,128,2,2,32,2,9,0,false>"),
    ("conv3x3_fwd", (1, 32, 32, 512, 512), dict(accumulate=False, bias=True, relu=True), dict(x_relu=True), "bx3_rows_kernel<4,128,2,2,32,2,9,0,false>"),
    ("conv3x3_fwd", (1, 512, 512, 128, 64), dict(accumulate=False, bias=True, relu=True), dict(x_relu=True), "bx3_rows_kernel<8,64,4,1,16,2,9,0,false>"),
    ("conv3x3_fwd", (1, 512, 512, 32, 64), dict(accumulate=False, bias=True, relu=True), dict(x_relu=False), "bx3_rows_kernel<8,64,4,1,16,2,9,0,false>"),
    ("conv3x3_fwd", (1, 512, 512, 64, 128), dict(accumulate=False, bias=True, relu=True), dict(x_relu=True), "bx3_rows_kernel<8,128,2,2,16,2,9,0,false>"),
    ("conv3x3_fwd", (1, 64, 64, 128, 256), dict(accumulate=False, bias=True, relu=True), dict(x_relu=False), "bx3_rows_kernel<4,64,4,1,32,2,9,0,false>"),
    ("conv3x3_fwd", (1, 64, 64, 256, 256), dict(accumulate=False, bias=True, relu=True), dict(x_relu=True), "bx3_rows_kernel<4,128,2,2,32,2,9,0,false>"),
    ("conv3x3_fwd", (1, 64, 64, 512, 256), dict(accumulate=False, bias=True, relu=True), dict(x_relu=False), "bx3_rows_kernel<4,128,2,2,32,2,9,0,false>"),
    ("conv3x3_wgrad", (1, 128, 128, 128, 128), dict(accumulate=True, db=True, defer=False), dict(g_sparse=True, x_relu=True), "bx3_wgrad_kernel<4,2,false,0>"),
    ("conv3x3_wgrad", (1, 128, 128, 256, 128), dict(accumulate=True, db=True, defer=False), dict(g_sparse=True, x_relu=False), "bx3_wgrad_kernel<4,2,false,0>"),
    ("conv3x3_wgrad", (1, 128, 128, 64, 128), dict(accumulate=True, db=True, defer=False), dict(g_sparse=True, x_relu=False), "bx3_wgrad_kernel<4,2,false,0>"),
    ("conv3x3_wgrad", (1, 256, 256, 128, 64), dict(accumulate=True, db=True, defer=False), dict(g_sparse=True, x_relu=False), "bx3_wgrad_kernel<2,2,false,0>"),
    ("conv3x3_wgrad", (1, 256, 256, 32, 32), dict(accumulate=True, db=True, defer=False), dict(g_sparse=True, x_relu=True), "bx3_wgrad_kernel<1,2,false,0>"),
    ("conv3x3_wgrad", (1, 256, 256, 32, 64), dict(accumulate=True, db=True, defer=False), dict(g_sparse=True, x_relu=False), "bx3_wgrad_kernel<2,2,false,0>"),
    ("conv3x3_wgrad", (1, 256, 256, 64, 32), dict(accumulate=True, db=True, defer=False), dict(g_sparse=True, x_relu=False), "bx3_wgrad_kernel<1,2,false,0>"),
    ("conv3x3_wgrad", (1, 256, 256, 64, 64), dict(accumulate=True, db=True, defer=False), dict(g_sparse=True, x_relu=True), "bx3_wgrad_kernel<2,2,false,0>"),
    ("conv3x3_wgrad", (1, 32, 32, 256, 512), dict(accumulate=True, db=True, defer=False), dict(g_sparse=True, x_relu=False), "bx3_wgrad_kernel<4,2,false,0>"),
    ("conv3x3_wgrad", (1, 32, 32, 512, 512), dict(accumulate=True, db=True, defer=False), dict(g_sparse=True, x_relu=True), "bx3_wgrad_kernel<4,2,false,0>"),
    ("conv3x3_wgrad", (1, 512, 512, 128, 64), dict(accumulate=True, db=True, defer=False), dict(g_sparse=True, x_relu=True), "bx3_wgrad_kernel<2,2,false,0>"),
    ("conv3x3_wgrad", (1, 512, 512, 32, 64), dict(accumulate=True, db=True, defer=False), dict(g_sparse=True, x_relu=False), "bx3_wgrad_kernel<2,2,false,0>"),
    ("conv3x3_wgrad", (1, 512, 512, 64, 128), dict(accumulate=True, db=True, defer=False), dict(g_sparse=True, x_relu=True), "bx3_wgrad_kernel<4,2,false,0>"),
    ("conv3x3_wgrad", (1, 64, 64, 128, 256), dict(accumulate=True, db=True, defer=False), dict(g_sparse=True, x_relu=False), "bx3_wgrad_kernel<4,2,false,0>"),
    ("conv3x3_wgrad", (1, 64, 64, 256, 256), dict(accumulate=True, db=True, defer=False), dict(g_sparse=True, x_relu=True), "bx3_wgrad_kernel<4,2,false,0>"),
    ("conv3x3_wgrad", (1, 64, 64, 512, 256), dict(accumulate=True, db=True, defer=False), dict(g_sparse=True, x_relu=False), "bx3_wgrad_kernel<4,2,false,0>"),
    ("head1x1_bwd", (262144,), dict(flags=3586), dict(), "t2h_head1x1_bwd"),
    ("head1x1_fwd", (262144,), dict(bias=True), dict(), "t2h_head1x1_fwd"),
    ("linear_dgrad", (1024, 1024, 512, 1024, 512), dict(accumulate=True, bx3=False, ldm=0, mask=False), dict(g_sparse=True), "gemm_kwaves_kernel<true,false>"),
    ("linear_dgrad", (1024, 1856, 512, 2752, 512), dict(accumulate=False, bx3=False, ldm=0, mask=False), dict(g_sparse=True), "gemm_kwaves_kernel<true,false>"),
    ("linear_dgrad", (1024, 512, 256, 512, 256), dict(accumulate=False, bx3=False, ldm=0, mask=False), dict(g_sparse=False), "gemm_kwaves_kernel<true,false>"),
    ("linear_dgrad", (131072, 128, 64, 128, 64), dict(accumulate=False, bx3=False, ldm=0, mask=False), dict(g_sparse=True), "gemm_kernel<128,64,2,2,true,false,16,true,1,0>"),
    ("linear_dgrad", (131072, 32, 32, 32, 32), dict(accumulate=False, bx3=False, ldm=0, mask=False), dict(g_sparse=False), "gemm_kernel<128,32,4,1,true,false,16,true,1,0>"),
    ("linear_dgrad", (131072, 32, 64, 32, 64), dict(accumulate=False, bx3=False, ldm=64, mask=True), dict(g_sparse=False), "gemm_kernel<128,64,2,2,true,false,16,true,1,0>"),
    ("linear_dgrad", (131072, 64, 128, 64, 128), dict(accumulate=False, bx3=False, ldm=128, mask=True), dict(g_sparse=False), "gemm_dma_nn_kernel"),
    ("linear_dgrad", (131072, 64, 32, 64, 32), dict(accumulate=False, bx3=False, ldm=0, mask=False), dict(g_sparse=True), "gemm_kernel<128,32,4,1,true,false,16,true,1,0>"),
    ("linear_dgrad", (16384, 128, 64, 128, 64), dict(accumulate=False, bx3=False, ldm=0, mask=False), dict(g_sparse=False), "gemm_kernel<128,64,2,2,true,false,16,true,1,0>"),
    ("linear_dgrad", (16384, 256, 128, 256, 128), dict(accumulate=True, bx3=False, ldm=0, mask=False), dict(g_sparse=True), "gemm_kernel<64,64,2,2,true,false,32,true,1,0>"),
    ("linear_dgrad", (16384, 2624, 128, 2752, 128), dict(accumulate=False, bias=False, bx3=True, ldm=0, mask=False, relu_out=False), dict(x_relu=False), "bx3_rows_kernel<4,128,2,2,64,2,1,0,false>"),
    ("linear_dgrad", (16384, 320, 128, 2752, 128), dict(accumulate=False, bias=False, bx3=True, ldm=0, mask=False, relu_out=False), dict(x_relu=False), "bx3_rows_kernel<4,128,2,2,64,2,1,0,false>"),
    ("linear_dgrad", (4096, 2368, 256, 2752, 256), dict(accumulate=False, bias=False, bx3=True, ldm=0, mask=False, relu_out=False), dict(x_relu=False), "bx3_rows_kernel<4,128,2,2,64,2,1,0,false>"),
    ("linear_dgrad", (4096, 256, 128, 256, 128), dict(accumulate=False, bx3=False, ldm=0, mask=False), dict(g_sparse=False), "gemm_kwaves_kernel<true,false>"),
    ("linear_dgrad", (4096, 512, 256, 512, 256), dict(accumulate=True, bx3=False, ldm=0, mask=False), dict(g_sparse=True), "gemm_kwaves_kernel<true,false>"),
    ("linear_dgrad", (4096, 832, 256, 2752, 256), dict(accumulate=False, bias=False, bx3=True, ldm=0, mask=False, relu_out=False), dict(x_relu=False), "bx3_rows_kernel<4,128,2,2,64,2,1,0,false>"),
    ("linear_dgrad", (65536, 128, 64, 128, 64), dict(accumulate=True, bx3=False, ldm=0, mask=False), dict(g_sparse=True), "gemm_kernel<128,64,2,2,true,false,16,true,1,0>"),
    ("linear_dgrad", (65536, 2752, 64, 2752, 64), dict(accumulate=False, bias=False, bx3=True, ldm=0, mask=False, relu_out=False), dict(x_relu=False), "bx3_rows_kernel<4,64,4,1,64,2,1,0,false>"),
    ("linear_dgrad", (65536, 32, 32, 32, 32), dict(accumulate=False, bx3=False, ldm=0, mask=False), dict(g_sparse=False), "gemm_kernel<128,32,4,1,true,false,16,true,1,0>"),
    ("linear_dgrad", (65536, 32, 64, 32, 64), dict(accumulate=False, bx3=False, ldm=0, mask=False), dict(g_sparse=False), "gemm_kernel<128,64,2,2,true,false,16,true,1,0>"),
    ("linear_dgrad", (65536, 32, 64, 64, 64), dict(accumulate=False, bx3=False, ldm=0, mask=False), dict(g_sparse=False), "gemm_kernel<128,64,2,2,true,false,16,true,1,0>"),
    ("linear_dgrad", (65536, 64, 32, 64, 32), dict(accumulate=False, bx3=False, ldm=0, mask=False), dict(g_sparse=False), "gemm_kernel<128,32,4,1,true,false,16,true,1,0>"),
    ("linear_fwd", (1024, 256, 512, 256, 512), dict(accumulate=False, addend=True, bias=True, bx3=False, relu_in=False, relu_out=False), dict(x_relu=False), "gemm_kwaves_kernel<true,true>"),
    ("linear_fwd", (1024, 512, 1024, 512, 1024), dict(accumulate=False, bias=True, bx3=False, relu_in=False, relu_out=False), dict(x_relu=False), "gemm_kwaves_kernel<true,true>"),
    ("linear_fwd", (1024, 512, 1856, 512, 2752), dict(accumulate=False, bias=False, bx3=False, relu_in=False, relu_out=False), dict(x_relu=False), "gemm_kernel<64,64,2,2,true,true,32,true,1,0>"),
    ("linear_fwd", (131072, 128, 64, 128, 64), dict(accumulate=False, bias=True, bx3=False, relu_in=False, relu_out=False), dict(x_relu=True), "gemm_kernel<128,64,2,2,true,true,16,true,1,0>"),
    ("linear_fwd", (131072, 32, 32, 32, 32), dict(accumulate=True, bias=True, bx3=False, relu_in=False, relu_out=False), dict(x_relu=False), "gemm_kernel<128,32,4,1,true,true,16,true,1,0>"),
    ("linear_fwd", (131072, 32, 64, 32, 64), dict(accumulate=False, bias=True, bx3=False, relu_in=False, relu_out=True), dict(x_relu=True), "gemm_kernel<128,64,2,2,true,true,16,true,1,0>"),
    ("linear_fwd", (131072, 32, 64, 32, 64), dict(accumulate=True, bias=True, bx3=False, relu_in=False, relu_out=False), dict(x_relu=False), "gemm_kernel<128,64,2,2,true,true,16,true,1,0>"),
    ("linear_fwd", (131072, 64, 128, 64, 128), dict(accumulate=False, bias=True, bx3=False, relu_in=False, relu_out=True), dict(x_relu=False), "gemm_dma_kernel"),
    ("linear_fwd", (131072, 64, 32, 64, 32), dict(accumulate=False, bias=True, bx3=False, relu_in=False, relu_out=False), dict(x_relu=True), "gemm_kernel<128,32,4,1,true,true,16,true,1,0>"),
    ("linear_fwd", (16384, 128, 256, 128, 256), dict(accumulate=False, bias=True, bx3=False, relu_in=False, relu_out=False), dict(x_relu=False), "gemm_dma_kernel"),
    ("linear_fwd", (16384, 128, 2624, 128, 2752), dict(accumulate=False, bias=False, bx3=True, ldm=0, mask=False, relu_out=False), dict(x_relu=False), "bx3_rows_kernel<8,64,4,1,32,2,1,0,false>"),
    ("linear_fwd", (16384, 128, 320, 128, 2752), dict(accumulate=True, bias=False, bx3=True, ldm=0, mask=False, relu_out=False), dict(x_relu=False), "bx3_rows_kernel<4,64,4,1,64,2,1,0,false>"),
    ("linear_fwd", (16384, 64, 128, 64, 128), dict(accumulate=False, addend=True, bias=True, bx3=False, relu_in=False, relu_out=False), dict(x_relu=False), "gemm_kernel<64,64,2,2,true,true,32,true,1,0>"),
    ("linear_fwd", (4096, 128, 256, 128, 256), dict(accumulate=False, addend=True, bias=True, bx3=False, relu_in=False, relu_out=False), dict(x_relu=False), "gemm_kernel<64,64,2,2,true,true,32,true,1,0>"),
    ("linear_fwd", (4096, 256, 2368, 256, 2752), dict(accumulate=False, bias=False, bx3=True, ldm=0, mask=False, relu_out=False), dict(x_relu=False), "bx3_rows_kernel<4,64,4,1,64,2,1,0,false>"),
    ("linear_fwd", (4096, 256, 512, 256, 512), dict(accumulate=False, bias=True, bx3=False, relu_in=False, relu_out=False), dict(x_relu=False), "gemm_kernel<64,64,2,2,true,true,32,true,1,0>"),
    ("linear_fwd", (4096, 256, 832, 256, 2752), dict(accumulate=True, bias=False, bx3=True, ldm=0, mask=False, relu_out=False), dict(x_relu=False), "bx3_rows_kernel<4,64,4,1,64,2,1,0,false>"),
    ("linear_fwd", (65536, 32, 32, 32, 32), dict(accumulate=False, addend=False, bias=True, bx3=False, relu_in=False, relu_out=False), dict(x_relu=False), "gemm_kernel<128,32,4,1,true,true,16,true,1,0>"),
    ("linear_fwd", (65536, 32, 64, 32, 64), dict(accumulate=False, addend=True, bias=True, bx3=False, relu_in=False, relu_out=False), dict(x_relu=True), "gemm_kernel<128,64,2,2,true,true,16,true,1,0>"),
    ("linear_fwd", (65536, 64, 128, 64, 128), dict(accumulate=False, bias=True, bx3=False, relu_in=False, relu_out=False), dict(x_relu=False), "gemm_dma_kernel"),
    ("linear_fwd", (65536, 64, 2752, 64, 2752), dict(accumulate=False, bias=False, bx3=True, ldm=0, mask=False, relu_out=False), dict(x_relu=False), "bx3_rows_kernel<4,64,4,1,64,2,1,0,true>"),
    ("linear_fwd", (65536, 64, 32, 64, 32), dict(accumulate=False, addend=False, bias=True, bx3=False, relu_in=False, relu_out=False), dict(x_relu=False), "gemm_kernel<128,32,4,1,true,true,16,true,1,0>"),
    ("linear_fwd", (65536, 64, 32, 64, 32), dict(accumulate=False, addend=True, bias=True, bx3=False, relu_in=False, relu_out=False), dict(x_relu=False), "gemm_kernel<128,32,4,1,true,true,16,true,1,0>"),
    ("linear_wgrad", (1024, 256, 512, 512, 256), dict(accumulate=True, db=True, defer=False, relu_in=False), dict(x_relu=False), "gemm_dma_tn_kernel"),
    ("linear_wgrad", (1024, 512, 1024, 1024, 512), dict(accumulate=True, db=True, defer=False, relu_in=False), dict(x_relu=False), "gemm_dma_tn_kernel"),
    ("linear_wgrad", (1024, 512, 1856, 2752, 512), dict(accumulate=True, db=False, defer=False, relu_in=False), dict(x_relu=False), "gemm_kwaves_kernel<false,false>"),
    ("linear_wgrad", (131072, 128, 64, 64, 128), dict(accumulate=True, db=True, defer=False, relu_in=False), dict(x_relu=True), "gemm_kernel<64,128,2,2,false,false,16,true,1,0>"),
    ("linear_wgrad", (131072, 32, 32, 32, 32), dict(accumulate=True, db=True, defer=False, relu_in=False), dict(x_relu=False), "gemm_kernel<32,32,1,1,false,false,16,true,1,0>"),
    ("linear_wgrad", (131072, 32, 64, 64, 32), dict(accumulate=True, db=True, defer=False, relu_in=False), dict(x_relu=True), "gemm_kernel<64,32,2,1,false,false,16,true,1,0>"),
    ("linear_wgrad", (131072, 64, 128, 128, 64), dict(accumulate=True, db=True, defer=False, relu_in=False), dict(x_relu=False), "gemm_kernel<128,64,2,2,false,false,16,true,1,0>"),
    ("linear_wgrad", (131072, 64, 32, 32, 64), dict(accumulate=True, db=True, defer=False, relu_in=False), dict(x_relu=True), "gemm_kernel<32,64,1,2,false,false,16,true,1,0>"),
    ("linear_wgrad", (16384, 128, 256, 256, 128), dict(accumulate=True, db=True, defer=False, relu_in=False), dict(x_relu=False), "gemm_dma_tn_kernel"),
    ("linear_wgrad", (16384, 128, 2624, 2752, 128), dict(accumulate=True, db=False, defer=False, relu_in=False), dict(x_relu=False), "gemm_dma_tn_kernel"),
    ("linear_wgrad", (16384, 128, 320, 2752, 128), dict(accumulate=True, db=False, defer=False, relu_in=False), dict(x_relu=False), "gemm_dma_tn_kernel"),
    ("linear_wgrad", (16384, 64, 128, 128, 64), dict(accumulate=True, db=True, defer=False, relu_in=False), dict(x_relu=False), "gemm_kernel<128,64,2,2,false,false,16,true,1,0>"),
    ("linear_wgrad", (4096, 128, 256, 256, 128), dict(accumulate=True, db=True, defer=False, relu_in=False), dict(x_relu=False), "gemm_dma_tn_kernel"),
    ("linear_wgrad", (4096, 256, 2368, 2752, 256), dict(accumulate=True, db=False, defer=False, relu_in=False), dict(x_relu=False), "gemm_dma_tn_kernel"),
    ("linear_wgrad", (4096, 256, 512, 512, 256), dict(accumulate=True, db=True, defer=False, relu_in=False), dict(x_relu=False), "gemm_dma_tn_kernel"),
    ("linear_wgrad", (4096, 256, 832, 2752, 256), dict(accumulate=True, db=False, defer=False, relu_in=False), dict(x_relu=False), "gemm_dma_tn_kernel"),
    ("linear_wgrad", (65536, 32, 32, 32, 32), dict(accumulate=True, db=True, defer=False, relu_in=False), dict(x_relu=False), "gemm_kernel<32,32,1,1,false,false,16,true,1,0>"),
    ("linear_wgrad", (65536, 32, 64, 64, 32), dict(accumulate=True, db=True, defer=False, relu_in=False), dict(x_relu=False), "gemm_kernel<64,32,2,1,false,false,16,true,1,0>"),
    ("linear_wgrad", (65536, 64, 128, 128, 64), dict(accumulate=True, db=True, defer=False, relu_in=False), dict(x_relu=False), "gemm_kernel<128,64,2,2,false,false,16,true,1,0>"),
    ("linear_wgrad", (65536, 64, 2752, 2752, 64), dict(accumulate=True, db=False, defer=False, relu_in=False), dict(x_relu=False), "gemm_kernel<128,64,2,2,false,false,16,true,1,0>"),
    ("linear_wgrad", (65536, 64, 32, 32, 64), dict(accumulate=True, db=True, defer=False, relu_in=False), dict(x_relu=False), "gemm_kernel<32,64,1,2,false,false,16,true,1,0>"),
    ("linear_wgrad", (65536, 64, 32, 64, 64), dict(accumulate=True, db=True, defer=False, relu_in=False), dict(x_relu=False), "gemm_kernel<32,64,1,2,false,false,16,true,1,0>"),
    ("maxpool_bwd", (1, 128, 128, 128), dict(), dict(), "t2h_maxpool2x2_nhwc_bwd"),
    ("maxpool_bwd", (1, 256, 256, 64), dict(), dict(), "t2h_maxpool2x2_nhwc_bwd"),
    ("maxpool_bwd", (1, 64, 64, 256), dict(), dict(), "t2h_maxpool2x2_nhwc_bwd"),
    ("maxpool_bwd_add", (1, 128, 128, 128), dict(addend=True, ld=256), dict(), "t2h_maxpool2x2_nhwc_bwd_add"),
    ("maxpool_bwd_add", (1, 256, 256, 64), dict(addend=True, ld=128), dict(), "t2h_maxpool2x2_nhwc_bwd_add"),
    ("maxpool_bwd_add", (1, 64, 64, 256), dict(addend=True, ld=512), dict(), "t2h_maxpool2x2_nhwc_bwd_add"),
    ("maxpool_fwd", (1, 128, 128, 128), dict(), dict(), "t2h_maxpool2x2_nhwc_fwd"),
    ("maxpool_fwd", (1, 256, 256, 64), dict(), dict(), "t2h_maxpool2x2_nhwc_fwd"),
    ("maxpool_fwd", (1, 64, 64, 256), dict(), dict(), "t2h_maxpool2x2_nhwc_fwd"),
    ("relu_mask", (1048576,), dict(), dict(), "t2h_relu_mask"),
    ("relu_mask", (2097152,), dict(), dict(), "t2h_relu_mask"),
    ("relu_mask", (4194304,), dict(), dict(), "t2h_relu_mask"),
    ("relu_mask", (524288,), dict(), dict(), "t2h_relu_mask"),
    ("upconv2x2_dgrad", (1, 128, 128, 128, 64), dict(lddy=128), dict(g_sparse=False), "bx3_rows_kernel<4,128,2,2,64,2,1,2,false>"),
    ("upconv2x2_dgrad", (1, 128, 128, 128, 64), dict(lddy=64), dict(g_sparse=False), "bx3_rows_kernel<4,128,2,2,64,2,1,2,false>"),
    ("upconv2x2_dgrad", (1, 32, 32, 512, 256), dict(lddy=256), dict(g_sparse=False), "bx3_rows_kernel<4,128,2,2,64,2,1,2,false>"),
    ("upconv2x2_dgrad", (1, 32, 32, 512, 256), dict(lddy=512), dict(g_sparse=False), "bx3_rows_kernel<4,128,2,2,64,2,1,2,false>"),
    ("upconv2x2_dgrad", (1, 64, 64, 256, 128), dict(lddy=128), dict(g_sparse=False), "bx3_rows_kernel<4,128,2,2,64,2,1,2,false>"),
    ("upconv2x2_dgrad", (1, 64, 64, 256, 128), dict(lddy=256), dict(g_sparse=False), "bx3_rows_kernel<4,128,2,2,64,2,1,2,false>"),
    ("upconv2x2_fwd", (1, 128, 128, 128, 64), dict(addend=False, bias=True), dict(x_relu=False), "bx3_rows_kernel<4,128,2,2,64,2,1,1,false>"),
    ("upconv2x2_fwd", (1, 128, 128, 128, 64), dict(addend=True, bias=True), dict(x_relu=False), "bx3_rows_kernel<4,128,2,2,64,2,1,1,false>"),
    ("upconv2x2_fwd", (1, 32, 32, 512, 256), dict(addend=False, bias=True), dict(x_relu=False), "bx3_rows_kernel<4,32,4,1,64,2,1,1,false>"),
    ("upconv2x2_fwd", (1, 32, 32, 512, 256), dict(addend=True, bias=True), dict(x_relu=False), "bx3_rows_kernel<4,32,4,1,64,2,1,1,false>"),
    ("upconv2x2_fwd", (1, 64, 64, 256, 128), dict(addend=False, bias=True), dict(x_relu=False), "bx3_rows_kernel<4,64,4,1,64,2,1,1,false>"),
    ("upconv2x2_fwd", (1, 64, 64, 256, 128), dict(addend=True, bias=True), dict(x_relu=False), "bx3_rows_kernel<4,64,4,1,64,2,1,1,false>"),
    ("upconv2x2_wgrad", (1, 128, 128, 128, 64), dict(accumulate=True, db=True, defer=False, lddy=128), dict(), "bx3_wgrad_kernel<4,2,true,0>"),
    ("upconv2x2_wgrad", (1, 128, 128, 128, 64), dict(accumulate=True, db=True, defer=False, lddy=64), dict(), "bx3_wgrad_kernel<4,2,true,0>"),
    ("upconv2x2_wgrad", (1, 32, 32, 512, 256), dict(accumulate=True, db=True, defer=False, lddy=256), dict(), "bx3_wgrad_kernel<4,2,true,0>"),
    ("upconv2x2_wgrad", (1, 32, 32, 512, 256), dict(accumulate=True, db=True, defer=False, lddy=512), dict(), "bx3_wgrad_kernel<4,2,true,0>"),
    ("upconv2x2_wgrad", (1, 64, 64, 256, 128), dict(accumulate=True, db=True, defer=False, lddy=128), dict(), "bx3_wgrad_kernel<4,2,true,0>"),
    ("upconv2x2_wgrad", (1, 64, 64, 256, 128), dict(accumulate=True, db=True, defer=False, lddy=256), dict(), "bx3_wgrad_kernel<4,2,true,0>"),
    ("upsample_bwd", (1, 32, 256, 256, 512, 512), dict(), dict(), "t2h_upsample_bilinear_nhwc_bwd"),
    ("upsample_fwd", (1, 32, 256, 256, 512, 512), dict(addend=False), dict(), "t2h_upsample_bilinear_nhwc_fwd"),
]


ROWS = [("b4",) + r for r in ROWS_B4] + [("b1",) + r for r in ROWS_B1]
CPU64_MAX_FLOPS = 2e10
F16X2_FLOOR, BF16X3_FLOOR = 2.0 ** -21, 4e-7


def _dev():
    return torch.device("cuda:0")


def _flops(row):
    _, fam, d = row[:3]
    if fam.startswith("conv3x3"):
        return 18.0 * d[0] * d[1] * d[2] * d[3] * d[4]
    if fam.startswith("upconv"):
        return 8.0 * d[0] * d[1] * d[2] * d[3] * d[4]
    if fam.startswith("linear"):
        return 2.0 * d[0] * d[1] * d[2]
    return 0.0


def _smallest(rows):
    best = {}
    for r in rows:
        if _flops(r) > 0 and (r[1] not in best or _flops(r) < _flops(best[r[1]])):
            best[r[1]] = r
    return {id(r) for r in best.values()}


_BOTH = _smallest(ROWS)


def _modes(row):
    """The 8-row kernels and the 4-row / 128-column plan also run in the two other reported arithmetics."""
    fam, sym = row[1], row[5]
    if fam in ("conv3x3_fwd", "conv3x3_dgrad") and (sym.startswith("bx3_rows_kernel<8,") or sym.startswith("bx3_rows_kernel<4,128,")):
        return ("f16x2", "bf16x3", "bf16")
    return ("f16x2",)


def _symbol_in(sym, mode):
    """bx3_rows_kernel's sixth template argument is the number of operand planes: 2 (fp16 two-way), 3 (bf16 three-way), 1 (bf16)."""
    if mode == "f16x2":
        return sym
    head, args = sym.split("<")
    args = args.split(",")
    args[5] = {"bf16x3": "3", "bf16": "1"}[mode]
    return head + "<" + ",".join(args)


def _id(row, mode):
    t, fam, d, epi = row[:4]
    e = "".join("+" + k for k, v in sorted(epi.items()) if v is True) + "".join(f"+{k}{v}" for k, v in sorted(epi.items())
                                                                               if type(v) is int and k.startswith("ld"))
    return f"{t}-{fam}-{'x'.join(map(str, d))}{e}" + ("" if mode == "f16x2" else "-" + mode)


CASES = [(r, m) for r in ROWS for m in _modes(r)]


# ------------------------------------------------------------------------------------------------ inputs
def _gen(row):
    return torch.Generator().manual_seed(zlib.crc32(repr((row[1], row[2], sorted(row[3].items()))).encode()) % (2 ** 31))


def _imgscale(n):
    return torch.tensor([2.0 ** (-6 * i) for i in range(n)])


def _plane(g, b, c, h, w, relu=False, sparse=False, scale=True):
    """NCHW fp32 plane on the CPU, image i scaled by 2^(-6 i)."""
    t = torch.randn(b, c, h, w, generator=g)
    if relu:
        t = t.clamp_(min=0)
    if sparse:
        t = t * (torch.rand(b, c, h, w, generator=g) < 0.5)
    return t * _imgscale(b).view(b, 1, 1, 1) if scale else t


def _mask(g, *shape):
    """Both signs and exact zeros."""
    return torch.randn(*shape, generator=g) * (torch.rand(*shape, generator=g) < 0.7)


def _rows(g, m, c, nblk, ld=None, relu=False, sparse=False):
    """[M, c] fp32 rows (a column slice of a [M, ld] buffer), row block i of ``nblk`` scaled by 2^(-6 i)."""
    t = torch.randn(m, c, generator=g)
    if relu:
        t = t.clamp_(min=0)
    if sparse:
        t = t * (torch.rand(m, c, generator=g) < 0.5)
    return t * _imgscale(nblk).repeat_interleave(m // nblk).view(m, 1)


def _cl(t):
    return t.to(_dev()).contiguous(memory_format=torch.channels_last)


def _wide(t, ld):
    """The [M, c] rows ``t`` on the device as a column slice of a [M, ld] buffer."""
    if ld == t.shape[1]:
        return t.to(_dev()).contiguous()
    buf = torch.full((t.shape[0], ld), 7.0, device=_dev())
    buf[:, :t.shape[1]] = t.to(_dev())
    return buf[:, :t.shape[1]]


def _wide_cl(t, ld):
    """The NCHW plane ``t`` on the device as a channel slice of an NHWC tensor with ``ld`` channels."""
    if ld == t.shape[1]:
        return _cl(t)
    b, c, h, w = t.shape
    buf = torch.full((b, ld, h, w), 7.0, device=_dev()).contiguous(memory_format=torch.channels_last)
    buf[:, :c] = t.to(_dev())
    return buf[:, :c]


# ------------------------------------------------------------------------------------------------ the same operations, three ways
class _Ops:
    """The reference arithmetic on one backend.  'cpu32' / 'cpu64': torch's CPU convolutions and matmul; 'dev64': float64 matmul
    on the device (shifted products for the convolutions).  Planes are NCHW in, NCHW out."""

    def __init__(self, backend):
        self.backend = backend
        self.dtype = torch.float32 if backend == "cpu32" else torch.float64
        self.device = _dev() if backend == "dev64" else torch.device("cpu")

    def t(self, x):
        return None if x is None else x.detach().to(self.device, self.dtype)

    def conv3(self, x, w):
        if self.backend != "dev64":
            return F.conv2d(x, w, None, padding=1)
        b, ci, h, wd = x.shape
        xp = F.pad(x.permute(0, 2, 3, 1), (0, 0, 1, 1, 1, 1))
        y = None
        for ky in range(3):
            for kx in range(3):
                t = xp[:, ky:ky + h, kx:kx + wd, :].reshape(-1, ci) @ w[:, :, ky, kx].t()
                y = t if y is None else y.add_(t)
        return y.view(b, h, wd, -1).permute(0, 3, 1, 2)

    def conv3_dgrad(self, gy, w):
        return self.conv3(gy, w.flip(2, 3).transpose(0, 1).contiguous())

    def conv3_wgrad(self, gy, x, wshape):
        if self.backend != "dev64":
            return torch.nn.grad.conv2d_weight(x, wshape, gy, padding=1)
        b, ci, h, wd = x.shape
        xp = F.pad(x.permute(0, 2, 3, 1), (0, 0, 1, 1, 1, 1))
        g2 = gy.permute(0, 2, 3, 1).reshape(-1, gy.shape[1]).t().contiguous()
        dw = torch.empty(wshape, dtype=self.dtype, device=self.device)
        for ky in range(3):
            for kx in range(3):
                dw[:, :, ky, kx] = g2 @ xp[:, ky:ky + h, kx:kx + wd, :].reshape(-1, ci)
        return dw

    def up(self, x, w):
        """ConvTranspose2d(2, stride 2), w [Cin, Cout, 2, 2]."""
        if self.backend != "dev64":
            return F.conv_transpose2d(x, w, None, stride=2)
        b, ci, h, wd = x.shape
        co = w.shape[1]
        y = x.permute(0, 2, 3, 1).reshape(-1, ci) @ w.permute(0, 2, 3, 1).reshape(ci, 4 * co)
        return y.view(b, h, wd, 2, 2, co).permute(0, 5, 1, 3, 2, 4).reshape(b, co, 2 * h, 2 * wd)

    def _taps(self, g):
        b, co, h2, w2 = g.shape
        return g.view(b, co, h2 // 2, 2, w2 // 2, 2).permute(0, 2, 4, 3, 5, 1).reshape(-1, 4 * co)     # [pixels, (dy, dx, co)]

    def up_dgrad(self, g, w):
        if self.backend != "dev64":
            return F.conv2d(g, w, None, stride=2)
        b, co, h2, w2 = g.shape
        ci = w.shape[0]
        dx = self._taps(g) @ w.permute(0, 2, 3, 1).reshape(ci, 4 * co).t()
        return dx.view(b, h2 // 2, w2 // 2, ci).permute(0, 3, 1, 2)

    def up_wgrad(self, g, x, wshape):
        ci, co = wshape[0], wshape[1]
        dw = x.permute(0, 2, 3, 1).reshape(-1, ci).t() @ self._taps(g)
        return dw.view(ci, 2, 2, co).permute(0, 3, 1, 2)


def _refs(fn, both):
    """ref64, S, ref32 (dicts of fp64 device tensors) of ``fn(ops, absolute)``; ``both``: float64 on the CPU AND on the device,
    asserted equal to 1e-12 of the max-norm."""
    def on(backend, absolute):
        return {k: v.to(_dev(), torch.float64) for k, v in fn(_Ops(backend), absolute).items()}
    flops = fn.flops
    first = "cpu64" if (flops <= CPU64_MAX_FLOPS or both) else "dev64"
    ref = on(first, False)
    if both:
        other = on("dev64", False)
        for k in ref:
            d = (ref[k] - other[k]).abs().max().item()
            assert d <= 1e-12 * ref[k].abs().max().item(), f"{k}: CPU float64 and device float64 references differ by {d:.3e}"
    mag = on(first if flops <= CPU64_MAX_FLOPS else "dev64", True)
    ref32 = on("cpu32", False)
    return ref, mag, ref32


def _judge(what, got, ref, mag, ref32, bound_a, floor, nimg, report, bf16=False):
    """Bounds (a) and (b) of the module docstring on one result; the leading dimension holds ``nimg`` images (or row blocks)."""
    got = got.detach().to(torch.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    err = (got - ref).abs()
    if nimg > 1:
        rel = max((err[i].max() / ref[i].abs().max().clamp_min(1e-300)).item() for i in range(nimg))
    else:
        rel = (err.max() / ref.abs().max().clamp_min(1e-300)).item()
    pos = mag > 0
    e32 = ((ref32 - ref).abs()[pos] / mag[pos]).max().item()
    own = (err[pos] / mag[pos]).max().item()
    c = max(floor, 4.0 * e32)
    report.append(f"{what}: max-norm {rel:.3e} (bound {bound_a:.0e}); |err|/S kernel {own:.3e}, e32 {e32:.3e}, c {c:.3e}")
    print("[census] " + report[-1])
    if bf16:
        assert 2e-5 < rel <= 1e-2, report[-1]
        return
    assert rel <= bound_a, report[-1]
    assert float((err - c * mag).max()) <= 0.0, report[-1]


# ------------------------------------------------------------------------------------------------ one launch per family
def _launch_conv3x3(row):
    from tomosar2height_amd import grid, _lib
    _, fam, (b, h, wd, cin, cout), epi, inp, _ = row
    g = _gen(row)
    w = torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin)
    wdv = _cl(w)
    both = id(row) in _BOTH
    sc = _imgscale(b).view(b, 1, 1, 1)
    if fam == "conv3x3_fwd":
        x = _plane(g, b, cin, h, wd, relu=inp.get("x_relu"))
        bias = torch.randn(cout, generator=g) * 0.1 if epi["bias"] else None
        y0 = _plane(g, b, cout, h, wd) if epi["accumulate"] else None

        def fn(ops, absolute):
            A = (lambda t: t.abs()) if absolute else (lambda t: t)
            y = ops.conv3(A(ops.t(x)), A(ops.t(w)))
            if bias is not None:
                y = y + A(ops.t(bias)).view(1, -1, 1, 1)
            if epi["relu"] and not absolute:
                y = y.clamp_(min=0)
            return {"y": y if y0 is None else y + A(ops.t(y0))}
        y = _cl(y0) if y0 is not None else grid._empty_cl(b, cout, h, wd, _dev())
        with _lib.KernelTimeline() as tl:
            grid.conv3x3_fwd_(_cl(x), wdv, None if bias is None else bias.to(_dev()), y, relu=epi["relu"], accumulate=epi["accumulate"])
        outs, bounds = {"y": y}, {"y": 2e-5}
    elif fam == "conv3x3_dgrad":
        gy = _plane(g, b, cout, h, wd, sparse=inp.get("g_sparse"))
        mask = _mask(g, b, cin, h, wd) if epi["mask"] else None
        dx0 = _plane(g, b, cin, h, wd) if epi["accumulate"] else None
        g1 = (torch.randn(b, 1, h, wd, generator=g) * sc) if epi["rank1"] else None
        w1 = torch.randn(cin, generator=g) / math.sqrt(cin) if epi["rank1"] else None

        def fn(ops, absolute):
            A = (lambda t: t.abs()) if absolute else (lambda t: t)
            dx = ops.conv3_dgrad(A(ops.t(gy)), A(ops.t(w)))
            if g1 is not None:
                dx = dx + A(ops.t(g1)) * A(ops.t(w1)).view(1, -1, 1, 1)
            if mask is not None:
                dx = dx * (ops.t(mask) > 0)
            return {"dx": dx if dx0 is None else dx + A(ops.t(dx0))}
        dx = _cl(dx0) if dx0 is not None else grid._empty_cl(b, cin, h, wd, _dev())
        with _lib.KernelTimeline() as tl:
            if epi["rank1"]:
                assert grid.dgrad_rank1_ok(_cl(gy), wdv)
                grid.conv3x3_dgrad_rank1_(_cl(gy), wdv, dx, None if mask is None else _cl(mask), g1.to(_dev()).contiguous(), w1.to(_dev()))
            else:
                grid.conv3x3_dgrad_(_cl(gy), wdv, dx, mask=None if mask is None else _cl(mask), accumulate=epi["accumulate"])
        outs, bounds = {"dx": dx}, {"dx": 2e-5}
    else:
        # a sum over the images: x scaled down and dy scaled UP by the same power of two, so that every image carries an equal share
        x = _plane(g, b, cin, h, wd, relu=inp.get("x_relu"))
        gy = _plane(g, b, cout, h, wd, sparse=inp.get("g_sparse"), scale=False) / sc
        dw0 = torch.randn(cout, cin, 3, 3, generator=g)
        db0 = torch.randn(cout, generator=g)

        def fn(ops, absolute):
            A = (lambda t: t.abs()) if absolute else (lambda t: t)
            dw = ops.conv3_wgrad(A(ops.t(gy)), A(ops.t(x)), w.shape) + A(ops.t(dw0))
            return {"dw": dw, "db": A(ops.t(gy)).sum((0, 2, 3)) + A(ops.t(db0))}
        dw, db = _cl(dw0), db0.to(_dev())
        assert epi["accumulate"] and epi["db"]
        with _lib.KernelTimeline() as tl:
            grid.conv3x3_wgrad_(_cl(gy), _cl(x), dw, db, accumulate=True, defer=True)
        outs, bounds = {"dw": dw, "db": db}, {"dw": 1e-4, "db": 1e-4}
    torch.cuda.synchronize()
    fn.flops = _flops(row)
    return tl, outs, bounds, fn, both, (b if fam != "conv3x3_wgrad" else 1)


def _launch_upconv(row):
    from tomosar2height_amd import grid, mlp, _lib
    _, fam, (b, h, wd, cin, cout), epi, inp, _ = row
    g = _gen(row)
    x = _plane(g, b, cin, h, wd)
    w = torch.randn(cin, cout, 2, 2, generator=g) / math.sqrt(cin)
    bias = torch.randn(cout, generator=g) * 0.1
    addend = _plane(g, b, cout, 2 * h, 2 * wd) if epi.get("addend") else None
    sc = _imgscale(b).view(b, 1, 1, 1)
    gy = _plane(g, b, cout, 2 * h, 2 * wd)
    if fam == "upconv2x2_wgrad":
        gy = gy / sc / sc                                                    # equal shares of the images in the sum (see conv3x3_wgrad)
    dw0, db0 = torch.randn(cin, cout, 2, 2, generator=g), torch.randn(cout, generator=g)

    def fn(ops, absolute):
        A = (lambda t: t.abs()) if absolute else (lambda t: t)
        if fam == "upconv2x2_fwd":
            y = ops.up(A(ops.t(x)), A(ops.t(w))) + A(ops.t(bias)).view(1, -1, 1, 1)
            return {"y": y if addend is None else y + A(ops.t(addend))}
        if fam == "upconv2x2_dgrad":
            return {"dx": ops.up_dgrad(A(ops.t(gy)), A(ops.t(w)))}
        return {"dw": ops.up_wgrad(A(ops.t(gy)), A(ops.t(x)), w.shape) + A(ops.t(dw0)),
                "db": A(ops.t(gy)).sum((0, 2, 3)) + A(ops.t(db0))}
    wp = torch.nn.Parameter(_cl(w))
    bp = torch.nn.Parameter(bias.to(_dev()))
    wp.grad, bp.grad = _cl(dw0), db0.to(_dev())
    xd = _cl(x).requires_grad_(True)
    with _lib.KernelTimeline() as tl:
        y = grid._UpConv2x2.apply(xd, wp, bp, None if addend is None else _cl(addend))
        if fam != "upconv2x2_fwd":
            with mlp.direct_grad_accumulation(True):
                y.backward(_wide_cl(gy, epi["lddy"]))
    torch.cuda.synchronize()
    want = {"upconv2x2_fwd": "t2h_upconv2x2_bx3_fwd", "upconv2x2_dgrad": "t2h_upconv2x2_bx3_dgrad", "upconv2x2_wgrad": "t2h_upconv2x2_bx3_wgrad"}[fam]
    tl.records = [r for r in tl.records if r[0].startswith(want)]
    if fam == "upconv2x2_fwd":
        outs, bounds = {"y": y}, {"y": 2e-5}
    elif fam == "upconv2x2_dgrad":
        outs, bounds = {"dx": xd.grad}, {"dx": 2e-5}
    else:
        outs, bounds = {"dw": wp.grad, "db": bp.grad}, {"dw": 1e-4, "db": 1e-4}
    fn.flops = _flops(row)
    return tl, outs, bounds, fn, id(row) in _BOTH, (1 if fam == "upconv2x2_wgrad" else b)


def _launch_linear(row):
    from tomosar2height_amd import grid, mlp, _lib
    table, fam, d, epi, inp, _ = row
    nblk = 4 if table == "b4" else 1
    g = _gen(row)
    if fam == "linear_fwd":
        m, k, n, ldx, ldy = d
        x = _rows(g, m, k, nblk, relu=inp.get("x_relu"))
        w = torch.randn(n, k, generator=g) / math.sqrt(k)
        bias = torch.randn(n, generator=g) * 0.1 if epi["bias"] else None
        y0 = _rows(g, m, n, nblk) if (epi["accumulate"] or epi.get("addend")) else None

        def fn(ops, absolute):
            A = (lambda t: t.abs()) if absolute else (lambda t: t)
            y = A(ops.t(x)) @ A(ops.t(w)).t()
            if bias is not None:
                y = y + A(ops.t(bias))
            if epi["relu_out"] and not absolute:
                y = y.clamp_(min=0)
            return {"y": y if y0 is None else y + A(ops.t(y0))}
        if "addend" in epi:                                                  # grid._Conv1x1: the rows are the pixels of an NHWC plane
            side = math.isqrt(m // nblk)
            assert nblk * side * side == m and ldx == k and ldy == n
            as_plane = lambda t, c: t.view(nblk, side, side, c).permute(0, 3, 1, 2).to(_dev())
            with _lib.KernelTimeline() as tl:
                y = grid._Conv1x1.apply(as_plane(x, k), w.view(n, k, 1, 1).to(_dev()), None if bias is None else bias.to(_dev()),
                                        as_plane(y0, n) if epi["addend"] else None)
            y = y.permute(0, 2, 3, 1).reshape(m, n)
        else:
            y = _wide(y0 if y0 is not None else torch.zeros(m, n), ldy)
            with _lib.KernelTimeline() as tl:
                mlp.linear_fwd_(_wide(x, ldx), w.to(_dev()), None if bias is None else bias.to(_dev()), y, relu_out=epi["relu_out"],
                                accumulate=epi["accumulate"], bx3=epi["bx3"])
        outs, bounds = {"y": y}, {"y": 2e-5}
    elif fam == "linear_dgrad":
        m, n, k, lddy, lddx = d
        dy = _rows(g, m, n, nblk, sparse=inp.get("g_sparse"))
        w = torch.randn(n, k, generator=g) / math.sqrt(n)
        mask = _mask(g, m, k) if epi["mask"] else None
        dx0 = _rows(g, m, k, nblk) if epi["accumulate"] else None

        def fn(ops, absolute):
            A = (lambda t: t.abs()) if absolute else (lambda t: t)
            dx = A(ops.t(dy)) @ A(ops.t(w))
            if mask is not None:
                dx = dx * (ops.t(mask) > 0)
            return {"dx": dx if dx0 is None else dx + A(ops.t(dx0))}
        dx = _wide(dx0 if dx0 is not None else torch.zeros(m, k), lddx)
        with _lib.KernelTimeline() as tl:
            mlp.linear_dgrad_(_wide(dy, lddy), w.to(_dev()), dx, mask=None if mask is None else _wide(mask, epi["ldm"]),
                              accumulate=epi["accumulate"], bx3=epi["bx3"])
        outs, bounds = {"dx": dx}, {"dx": 2e-5}
    else:
        m, k, n, lddy, ldx = d
        sc = _imgscale(nblk).repeat_interleave(m // nblk).view(m, 1)
        dy = _rows(g, m, n, nblk) / sc / sc                                  # equal shares of the row blocks in the sum
        x = _rows(g, m, k, nblk, relu=inp.get("x_relu"))
        dw0, db0 = torch.randn(n, k, generator=g), (torch.randn(n, generator=g) if epi["db"] else None)
        assert epi["accumulate"] and not epi["relu_in"]

        def fn(ops, absolute):
            A = (lambda t: t.abs()) if absolute else (lambda t: t)
            out = {"dw": A(ops.t(dy)).t() @ A(ops.t(x)) + A(ops.t(dw0))}
            if db0 is not None:
                out["db"] = A(ops.t(dy)).sum(0) + A(ops.t(db0))
            return out
        dw, db = dw0.to(_dev()), (None if db0 is None else db0.to(_dev()))
        with _lib.KernelTimeline() as tl:
            mlp.linear_wgrad_(_wide(dy, lddy), _wide(x, ldx), dw, db, accumulate=True, defer=True)
        outs, bounds = {"dw": dw}, {"dw": 3e-5}
        if db is not None:
            outs["db"], bounds["db"] = db, 3e-5
    torch.cuda.synchronize()
    fn.flops = _flops(row)
    return tl, outs, bounds, fn, id(row) in _BOTH, (1 if fam == "linear_wgrad" else nblk)


def _blocks(t, n):
    """Leading dimension = images / row blocks."""
    return t if n == 1 or t.shape[0] == n else t.reshape(n, t.shape[0] // n, *t.shape[1:])


def _matrix_row(row, mode, monkeypatch):
    from tomosar2height_amd import grid
    fam = row[1]
    monkeypatch.setattr(grid, "CONV_PRECISION", mode)
    floor = BF16X3_FLOOR if mode == "bf16x3" else F16X2_FLOOR
    report = []
    launch = _launch_conv3x3 if fam.startswith("conv3x3") else (_launch_upconv if fam.startswith("upconv") else _launch_linear)
    tl, outs, bounds, fn, both, nimg = launch(row)
    ref, mag, ref32 = _refs(fn, both)
    for k, got in outs.items():
        bf = mode == "bf16" and k != "db"
        _judge(f"{_id(row, mode)} {k}", _blocks(got, nimg), _blocks(ref[k], nimg), _blocks(mag[k], nimg), _blocks(ref32[k], nimg),
               bounds[k], floor, nimg, report, bf16=bf)
    # (after the values: a changed plan shows as a failed symbol on a row whose values were judged first)
    syms = [r[5] for r in tl.records if "_prepare" not in r[0]]            # (the weight split of a fresh weight: not part of a warm step)
    assert syms == [_symbol_in(row[5], mode)], f"{_id(row, mode)}: launched {syms}, the table says {_symbol_in(row[5], mode)}"


# ------------------------------------------------------------------------------------------------ the launches that are no products
def _other_row(row):
    from tomosar2height_amd import grid, mlp, _lib
    _, fam, d, epi, inp, sym = row
    g = _gen(row)
    with _lib.KernelTimeline() as tl:
        if fam in ("head1x1_fwd", "head1x1_bwd"):
            b = 4 if row[0] == "b4" else 1
            side = math.isqrt(d[0] // b)
            chans = (32, 64, 128, 64)                                        # ConvDecoder: x, x1, x2, x3 (pixel.py:20-32)
            xs = [_plane(g, b, c, side, side, relu=i > 0) for i, c in enumerate(chans)]
            w4 = torch.randn(1, sum(chans), 1, 1, generator=g) / math.sqrt(sum(chans))
            b4 = torch.randn(1, generator=g)
            xd = [_cl(x) for x in xs]
            cat = torch.cat(xs, 1).double()
            if fam == "head1x1_fwd":
                out = grid._head_fwd(xd, w4.to(_dev()), b4.to(_dev()))
                checks = [(out, F.conv2d(cat, w4.double(), b4.double()), 2e-5)]
            else:
                gout = torch.randn(b, 1, side, side, generator=g) / _imgscale(b).view(b, 1, 1, 1)      # x scaled down, g UP: equal shares in dw
                wp, bp = torch.nn.Parameter(w4.to(_dev())), torch.nn.Parameter(b4.to(_dev()))
                dw0, db0 = torch.randn(1, sum(chans), 1, 1, generator=g), torch.randn(1, generator=g)
                wp.grad, bp.grad = dw0.to(_dev()), db0.to(_dev())
                d3 = torch.empty_like(xd[3], memory_format=torch.channels_last)
                # the decoder's backward: the three data gradients with the rank-1 epilogue form their own share, the head writes x3's
                with mlp.direct_grad_accumulation(True):
                    assert grid._head_bwd(xd, [None, None, None, d3], wp, bp, _cl(gout).contiguous(), relu_inputs=(1, 2, 3)) == (None, None)
                checks = [(d3[i:i + 1], (gout[i:i + 1].double() * w4[:, 224:].double().view(1, -1, 1, 1)) * (xs[3][i:i + 1] > 0), 2e-5)
                          for i in range(b)]
                checks += [(wp.grad, dw0.double() + (cat * gout.double()).sum((0, 2, 3)).view(1, -1, 1, 1), 1e-4),
                           (bp.grad, db0.double() + gout.double().sum(), 1e-4)]
        elif fam.startswith("maxpool"):
            b, h, w, c = d
            x = torch.randint(-2, 3, (b, c, h, w), generator=g).float()      # few distinct values: ties in most windows
            x[:, :, : h // 2] *= (torch.rand(b, c, h // 2, w, generator=g) < 0.5)
            gout = _plane(g, b, c, h // 2, w // 2)
            xr = x.clone().requires_grad_(True)
            yr = F.max_pool2d(xr, 2, 2)
            yr.backward(gout)
            xg = _cl(x).requires_grad_(True)
            if fam == "maxpool_bwd_add":
                thru = _plane(g, b, c, h, w)
                y, skip = grid.maxpool2x2_thru(xg, torch.nn.MaxPool2d(2, 2))
                torch.autograd.backward([y, skip], [_cl(gout), _wide_cl(thru, epi["ld"])])
                checks = [(xg.grad, (xr.grad + thru).double(), 0.0)]
            else:
                y = grid.maxpool2x2(xg, torch.nn.MaxPool2d(2, 2))
                y.backward(_cl(gout))
                checks = [(y.detach(), yr.detach().double(), 0.0)] if fam == "maxpool_fwd" else [(xg.grad, xr.grad.double(), 0.0)]
            want = {"maxpool_fwd": "t2h_maxpool2x2_fwd", "maxpool_bwd": "t2h_maxpool2x2_bwd", "maxpool_bwd_add": "t2h_maxpool2x2_bwd"}[fam]
            tl.records = [r for r in tl.records if r[0] == want]
        elif fam.startswith("upsample"):
            b, c, h, w, size, _ = d
            x = _plane(g, b, c, h, w)
            gout = _plane(g, b, c, size, size)
            from oracle import c_oracle
            xg = _cl(x).requires_grad_(True)
            y = grid.upsample_bilinear_cl(xg, size)
            y.backward(_cl(gout))
            # the reference and the bounds of tests/test_hip_grid.py::test_upsample_cl_vs_oracle (|d| <= atol + rtol |want|, 1e-6 forward,
            # 1e-5 backward), the absolute term scaled with the image like its input
            if fam == "upsample_fwd":
                got, want, tol = y.detach(), torch.from_numpy(c_oracle.upsample_bilinear_fwd(x.numpy(), size)), 1e-6
            else:
                got, want, tol = xg.grad, torch.from_numpy(c_oracle.upsample_bilinear_bwd(gout.numpy(), h, w)), 1e-5
            for i in range(b):
                dlt = (got[i].cpu().double() - want[i].double()).abs()
                assert bool((dlt <= tol * 2.0 ** (-6 * i) + tol * want[i].double().abs()).all()), (fam, i, float(dlt.max()))
            checks = []
            tl.records = [r for r in tl.records if r[0] == {"upsample_fwd": "t2h_upsample_bilinear_fwd", "upsample_bwd": "t2h_upsample_bilinear_bwd"}[fam]]
        else:
            n = d[0]
            gr, y = torch.randn(n, generator=g), _mask(g, n)
            out, grd, yd = torch.empty(n, device=_dev()), gr.to(_dev()), y.to(_dev())
            _lib.call("t2h_relu_mask", _lib.ptr(grd), _lib.ptr(yd), _lib.ptr(out), n, _lib.stream(), nbytes=12 * n)
            checks = [(out, (gr * (y > 0)).double(), 0.0)]
    torch.cuda.synchronize()
    assert [r[5] for r in tl.records] == [sym], ([r[5] for r in tl.records], sym)
    for i, (got, want, tol) in enumerate(checks):
        err = float((got.double().cpu() - want).abs().max()) / max(float(want.abs().max()), 1e-300)
        print(f"[census] {_id(row, 'f16x2')} result {i}: max-norm error {err:.3e} (bound {tol:.0e})")
        assert err <= tol, (fam, i, err, tol)


@pytest.mark.parametrize("row,mode", CASES, ids=[_id(r, m) for r, m in CASES])
def test_row(row, mode, monkeypatch):
    from tomosar2height_amd import _lib
    made, orig = [], _lib.call

    def recording(name, *a, **k):
        orig(name, *a, **k)
        if _lib._timeline is not None:
            rec = _lib._timeline.records[-1]
            r = _row_of_call(name, a, rec[0], rec[5])
            if r is not None and r[0] == row[1]:
                made.append(_key(*r))
    monkeypatch.setattr(_lib, "call", recording)
    if _flops(row) > 0:
        _matrix_row(row, mode, monkeypatch)
    else:
        _other_row(row)
    # the replay made the table's call: same shape arguments, same epilogue (flags, optional pointers, leading dimensions), same kernel
    assert made == [_key(row[1], row[2], row[3], _symbol_in(row[5], mode))], (made, row)


# ------------------------------------------------------------------------------------------------ closure
def _row_of_call(name, a, tag, sym):
    """(family, dims, epilogue, symbol) of one recorded C-ABI call, None for the point-side entry points.  ``a``: the call's arguments."""
    P = lambda i: a[i] is not None
    if name == "t2h_conv3x3_bx3_fwd" or name == "t2h_conv3x3_fwd":
        return ("conv3x3_fwd", tuple(a[4:9]), dict(bias=P(2), relu=bool(a[9] & 2), accumulate=bool(a[9] & 4)), sym)
    if name == "t2h_conv3x3_bx3_dgrad" or name == "t2h_conv3x3_dgrad":
        return ("conv3x3_dgrad", tuple(a[4:9]), dict(mask=P(3), accumulate=bool(a[9] & 4), rank1=False), sym)
    if name == "t2h_conv3x3_bx3_dgrad_rank1":
        return ("conv3x3_dgrad", tuple(a[6:11]), dict(mask=P(3), accumulate=False, rank1=True), sym)
    if name == "t2h_conv3x3_bx3_wgrad" or name == "t2h_conv3x3_wgrad":
        return ("conv3x3_wgrad", tuple(a[4:9]), dict(db=P(3), accumulate=bool(a[9] & 4), defer=bool(a[9] & 32)), sym)
    if name == "t2h_upconv2x2_bx3_fwd" or name == "t2h_upconv2x2_fwd_add":
        return ("upconv2x2_fwd", tuple(a[5:10]), dict(bias=P(2), addend=P(3)), sym)
    if name == "t2h_upconv2x2_bx3_dgrad":
        return ("upconv2x2_dgrad", tuple(a[4:9]), dict(lddy=a[1]), sym)
    if name == "t2h_upconv2x2_dgrad":
        return ("upconv2x2_dgrad", tuple(a[3:8]), dict(lddy=None), sym)
    if name == "t2h_upconv2x2_bx3_wgrad":
        return ("upconv2x2_wgrad", tuple(a[5:10]), dict(lddy=a[1], db=P(4), accumulate=bool(a[10] & 4), defer=bool(a[10] & 32)), sym)
    if name == "t2h_upconv2x2_wgrad_bias":
        return ("upconv2x2_wgrad", tuple(a[4:9]), dict(lddy=None, db=P(3), accumulate=bool(a[9] & 4), defer=bool(a[9] & 32)), sym)
    if name == "t2h_linear_fwd":
        return ("linear_fwd", (a[6], a[7], a[8], a[1], a[5]), dict(bias=P(3), relu_in=bool(a[9] & 1), relu_out=bool(a[9] & 2),
                                                                  accumulate=bool(a[9] & 4), bx3=False), sym)
    if name == "t2h_linear_fwd_add":
        return ("linear_fwd", (a[8], a[9], a[10], a[1], a[7]), dict(bias=P(3), addend=P(4), relu_in=bool(a[11] & 1), relu_out=bool(a[11] & 2),
                                                                    accumulate=bool(a[11] & 4), bx3=False), sym)
    if name == "t2h_gemm_bx3":
        return ("linear_fwd" if "fwd" in tag else "linear_dgrad", (a[8], a[9], a[10], a[1], a[7]),
                dict(bias=P(3), mask=P(4), ldm=a[5], relu_out=bool(a[11] & 2), accumulate=bool(a[11] & 4), bx3=True), sym)
    if name == "t2h_linear_dgrad":
        return ("linear_dgrad", (a[5], a[7], a[6], a[1], a[4]), dict(mask=P(8), ldm=a[9], accumulate=bool(a[10] & 4), bx3=False), sym)
    if name == "t2h_linear_wgrad":
        return ("linear_wgrad", (a[4], a[5], a[6], a[1], a[3]), dict(db=P(9), relu_in=bool(a[7] & 1), accumulate=bool(a[7] & 4), defer=bool(a[7] & 32)), sym)
    if name == "t2h_gemm_bx3_wgrad":
        return ("linear_wgrad", (a[4], a[5], a[6], a[1], a[3]), dict(bx3=True), sym)
    if name == "t2h_head1x1_fwd":
        return ("head1x1_fwd", (a[5],), dict(bias=P(4)), sym)
    if name == "t2h_head1x1_bwd":
        return ("head1x1_bwd", (a[6],), dict(flags=a[7]), sym)
    if name == "t2h_maxpool2x2_nhwc_fwd":
        return ("maxpool_fwd", tuple(a[1:5]), {}, sym)
    if name == "t2h_maxpool2x2_nhwc_bwd":
        return ("maxpool_bwd", tuple(a[2:6]), {}, sym)
    if name == "t2h_maxpool2x2_nhwc_bwd_add":
        return ("maxpool_bwd_add", tuple(a[2:6]), dict(addend=P(6), ld=a[7]), sym)
    if name == "t2h_upsample_bilinear_nhwc_fwd":
        return ("upsample_fwd", tuple(a[2:8]), dict(addend=P(1)), sym)
    if name == "t2h_upsample_bilinear_nhwc_bwd":
        return ("upsample_bwd", tuple(a[1:7]), {}, sym)
    if name == "t2h_relu_mask":
        return ("relu_mask", (a[3],), {}, sym)
    return None


def _key(fam, dims, epi, sym):
    # (the linear_dgrad rows of the split kernels carry mask / bias of the shared entry point: keep what the table keeps)
    return (fam, tuple(dims), tuple(sorted(epi.items())), sym)


@pytest.mark.parametrize("coalesce,table", [(4, "b4"), (1, "b1")])
def test_window_launches_are_the_table(coalesce, table, monkeypatch):
    """The benchmarked configuration itself (bench.py: berlin_config() cloud-only, N = 131 072, Trainer with all defaults, four
    equal-N synthetic tiles): one warm window, then one window under a KernelTimeline with ``_lib.call`` wrapped; every grid-side
    launch is a row of the table and every row of the table occurs.  ``coalesce`` = 1: the strict B = 1 step."""
    from tomosar2height_amd import TomoSAR2Height, _lib
    from tomosar2height_amd.config import berlin_config
    from tomosar2height_amd.optim import FlatAdamW
    from tomosar2height_amd.synthetic import berlin_tile
    from tomosar2height_amd.trainer import Trainer
    monkeypatch.setenv("T2H_COALESCE_TILES", str(coalesce))
    dev = _dev()
    cfg = berlin_config()
    torch.manual_seed(0)
    model = TomoSAR2Height(cfg).to(dev)
    model.set_mlp_precision("fp32")
    model.set_channels_last(True)
    trainer = Trainer(model, FlatAdamW(model.parameters(), lr=cfg.training.learning_rate), device=dev, optimize_every=64, use_cloud=True,
                      use_image=False)
    assert trainer.coalesce_tiles == coalesce
    tiles = []
    for i in range(4):
        t = berlin_tile(seed=i, n_points=131072, clustered=True)
        tiles.append({k: t[k].to(dev) for k in ("inputs", "dsm")})
    for t in tiles:
        trainer.train_step(t)
    trainer.flush_pipeline()
    torch.cuda.synchronize()
    seen, point_side = set(), set()
    orig = _lib.call

    def recording(name, *a, **k):
        orig(name, *a, **k)
        rec = _lib._timeline.records[-1]
        row = _row_of_call(name, a, rec[0], rec[5])
        if row is None:
            point_side.add((rec[0], rec[5]))
        else:
            seen.add(_key(*row))
    monkeypatch.setattr(_lib, "call", recording)
    with _lib.KernelTimeline():
        for t in (tiles if coalesce > 1 else tiles[:1]):
            trainer.train_step(t)
        trainer.flush_pipeline()
        torch.cuda.synchronize()
    monkeypatch.setattr(_lib, "call", orig)
    print(f"[census] point-side launches of the window ({len(point_side)}; nothing asserted about them):")
    for tag, sym in sorted(point_side):
        print(f"[census]   {tag}  {sym}")
    rows = {_key(r[1], r[2], r[3], r[5]) for r in ROWS if r[0] == table}
    extra, missing = sorted(seen - rows, key=repr), sorted(rows - seen, key=repr)
    assert not extra and not missing, ("launched by the window but not in the table:\n  " + "\n  ".join(map(repr, extra))
                                       + "\nin the table but not launched by the window:\n  " + "\n  ".join(map(repr, missing)))
