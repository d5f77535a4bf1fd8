"""The shapes that reach each main loop of kvq_gemm_bf16 / kvq_conv_implicit, as a table of literals.

tests/test_gemm_choice_cpu.py asserts every row against ``kernels.gemm_kernel_choice`` (no GPU needed) and that the rows cover every
code the query can return; tests/test_gpu_gemm_variants.py and tests/test_gpu_bounds.py run the rows and assert the code again before
each launch, so a re-tuned dispatch fails here first and cannot move a case onto another kernel unnoticed.

A code is MI*1000 + NI*100 + BK of the ring kernel's 64 MI x 64 NI x BK tile, 22264 for the 128 x 128 x 64 QKV tile on its 2-slice
ring, 4464 for the 256 x 256 x 64 eight-phase kernel.  ``mode`` is the tile mode the case sets (-1 by shape, 0 never the wide
tile); ``split``: whether the launch cuts K (split-K partial tiles + the reduce launch).  Every shape is ragged in M (no multiple
of its tile's rows; but for 8960 x 1152 x 384, the shape of tests/test_gpu_kernels.py that the wide tile takes by shape, ragged in N
there) and several are in N; M*N*K stays below 7e9 so that the fp64 reference takes under a second."""
from collections import namedtuple

Gemm = namedtuple("Gemm", "name M N K mode nH code split")
Conv = namedtuple("Conv", "name shape Cout kernel pad Kpad code split")

# plain GEMMs, every epilogue but QKV (nH = 0)
GEMM = [
    Gemm("64x64x32", 517, 520, 128, -1, 0, 1132, False),
    Gemm("128x128x64", 1479, 1024, 1024, -1, 0, 2264, False),
    Gemm("128x128x32", 1479, 1024, 1056, -1, 0, 2232, False),
    Gemm("128x128x32-mode0", 8960, 1152, 384, 0, 0, 2232, False),      # by shape this one is the eight-phase kernel's
    Gemm("128x64x32", 1479, 936, 1056, -1, 0, 2132, False),
    Gemm("192x128x64", 3000, 1408, 1024, -1, 0, 3264, False),
    Gemm("128x256x64", 2500, 2520, 1024, -1, 0, 2464, False),
    Gemm("splitk-128x128x32", 1479, 1024, 1568, -1, 0, 2232, True),
    Gemm("splitk-128x64x32", 12200, 64, 1568, -1, 0, 2132, True),
    Gemm("256x256x64", 8960, 1152, 384, -1, 0, 4464, False),
]
# the QKV epilogue (N = 96 nH; never split)
QKV = [
    Gemm("qkv-128x256x64", 2000, 3072, 1024, -1, 32, 2464, False),
    Gemm("qkv-128x64x32", 17030, 288, 96, -1, 3, 2132, False),
    Gemm("qkv-ring2", 17100, 384, 128, -1, 4, 22264, False),
]
# implicit-GEMM convolutions: channels-last input (B, D, H, W, C), stride 1; M = B*Do*Ho*Wo, K = Kpad
CONV = [
    Conv("conv-128x128", (1, 2, 80, 80, 128), 128, (1, 3, 3), (0, 1, 1), 1152, 2232, False),
    Conv("conv-128x64", (1, 2, 80, 80, 160), 64, (1, 3, 3), (0, 1, 1), 1440, 2132, False),
    Conv("conv-splitk-128x128", (1, 2, 61, 100, 64), 64, (1, 5, 5), (0, 2, 2), 1600, 2232, True),   # the plain GEMM of this shape stays whole
    Conv("conv-128x128-table", (1, 2, 80, 81, 120), 72, (1, 3, 3), (0, 1, 1), 1088, 2232, False),   # C % 32 != 0: tap table only, 8 columns of K padding
    Conv("conv-64x64", (2, 3, 13, 10, 32), 64, (1, 3, 3), (0, 1, 1), 288, 1132, False),
]
BY_NAME = {c.name: c for c in GEMM + QKV + CONV}


def conv_rows(c):
    """GEMM rows of a CONV case (stride 1)"""
    B, D, H, W, _ = c.shape
    return B * (D + 2 * c.pad[0] - c.kernel[0] + 1) * (H + 2 * c.pad[1] - c.kernel[1] + 1) * (W + 2 * c.pad[2] - c.kernel[2] + 1)
