"""CPU: which main loop each shape of tests/gemm_forms.py reaches, asked of the library (kvq_gemm_kernel_choice is host-only, and the
launchers of csrc/gemm.hip switch on the value it returns) and held against the table's literals — not against a copy of the
dispatch rule.  A re-tuned dispatch fails here and forces new shapes, instead of silently moving the GPU tests' coverage."""
import itertools

import pytest

import kvq_amd  # noqa: F401
from gemm_forms import CONV, GEMM, QKV, conv_rows
from kvq_amd import _abi, kernels


@pytest.fixture
def tile_mode_restored():
    prev = kernels.gemm_tile_mode(-2)          # reads only
    yield
    kernels.gemm_tile_mode(prev)


def _choice(M, N, K, mode, epi, conv=False):
    kernels.gemm_tile_mode(mode)
    return kernels.gemm_kernel_choice(M, N, K, epi, conv)


@pytest.mark.parametrize("c", GEMM + QKV, ids=lambda c: c.name)
def test_gemm_shape_reaches_its_form(c, tile_mode_restored):
    epis = [_abi.EPI_QKV_BF16] if c.nH else [_abi.EPI_BIAS_BF16, _abi.EPI_GELU_BF16, _abi.EPI_RESID_F32, _abi.EPI_STORE_F32, _abi.EPI_RELU_BF16,
                                            _abi.EPI_QGELU_BF16, _abi.EPI_RESID_SCALE_F32]
    assert not c.nH or c.N == 96 * c.nH
    for e in epis:
        assert _choice(c.M, c.N, c.K, c.mode, e) == c.code, (c.name, e)
    S = _abi.lib().kvq_gemm_splitk_factor(c.M, c.N, c.K)
    assert (S > 1) == c.split, (c.name, S)
    assert (_abi.lib().kvq_gemm_splitk_bytes(c.M, c.N, c.K) >= S * c.M * c.N * 4) if c.split else S == 1
    assert c.M * c.N * c.K <= 7e9 and c.K <= 1600            # the integer operands of the GPU tests stay exact in fp32
    rows = 256 if c.code == 4464 else 64 * (c.code // 1000 % 10)
    assert c.M % rows or c.M == 8960, "M must leave a ragged last row tile"


@pytest.mark.parametrize("c", CONV, ids=lambda c: c.name)
def test_conv_shape_reaches_its_form(c, tile_mode_restored):
    M = conv_rows(c)
    taps = c.kernel[0] * c.kernel[1] * c.kernel[2] * c.shape[-1]
    assert c.Kpad == -(-taps // 32) * 32
    for mode in (-1, 0, 1):                                   # the convolution has no wide tile: the mode does not move it
        assert _choice(M, c.Cout, c.Kpad, mode, _abi.EPI_RELU_BF16, True) == c.code, (c.name, mode)
    # no export names the conv front end's own factor; the scratch size covers the larger of the two front ends' factors
    S_plain, nbytes = _abi.lib().kvq_gemm_splitk_factor(M, c.Cout, c.Kpad), _abi.lib().kvq_gemm_splitk_bytes(M, c.Cout, c.Kpad)
    assert (nbytes > 0) == c.split, (c.name, nbytes)
    if c.split:
        assert S_plain == 1 and nbytes == 2 * M * c.Cout * 4      # the conv front end cuts K in two where the plain GEMM stays whole
    assert M * c.Cout * c.Kpad <= 7e9 and c.Kpad <= 1600


def test_expected_codes_are_literals():
    """the table as this test was written: an edit of tests/gemm_forms.py that follows a re-tuned dispatch shows up here as well"""
    assert {c.name: c.code for c in GEMM + QKV + CONV} == {
        "64x64x32": 1132, "128x128x64": 2264, "128x128x32": 2232, "128x128x32-mode0": 2232, "128x64x32": 2132, "192x128x64": 3264,
        "128x256x64": 2464, "splitk-128x128x32": 2232, "splitk-128x64x32": 2132, "256x256x64": 4464,
        "qkv-128x256x64": 2464, "qkv-128x64x32": 2132, "qkv-ring2": 22264,
        "conv-128x128": 2232, "conv-128x64": 2132, "conv-splitk-128x128": 2232, "conv-128x128-table": 2232, "conv-64x64": 1132}
    assert kernels.GEMM_8P == 4464 and kernels.GEMM_QKV_RING2 == 22264


def test_table_covers_every_code_the_query_returns(tile_mode_restored):
    """Every (front end, code) the query returns over a wide sweep of shapes, the QKV epilogue and the three modes is reached by a
    row of the table; and each big 32-deep ring tile is also reached under split-K (the 64-deep ones never split)."""
    Ms = [1, 64, 200, 1000, 1479, 2500, 3000, 6000, 8960, 12200, 17100, 40000, 131072]
    Ns = [8, 64, 96, 192, 264, 288, 384, 520, 768, 936, 1024, 1152, 1408, 2304, 2520, 3072, 4096]
    Ks = [32, 96, 128, 256, 384, 768, 1024, 1056, 1536, 1568, 3072, 4096]
    seen = set()
    for mode in (-1, 0, 1):
        kernels.gemm_tile_mode(mode)
        for M, N, K in itertools.product(Ms, Ns, Ks):
            seen.add((False, kernels.gemm_kernel_choice(M, N, K, _abi.EPI_BIAS_BF16)))
            seen.add((True, kernels.gemm_kernel_choice(M, N, K, _abi.EPI_RELU_BF16, True)))
            if N % 96 == 0:
                seen.add((False, kernels.gemm_kernel_choice(M, N, K, _abi.EPI_QKV_BF16)))
    reached = {(False, c.code) for c in GEMM + QKV} | {(True, c.code) for c in CONV}
    assert seen == reached, sorted(seen ^ reached)
    assert {c.code for c in GEMM if c.split} == {2232, 2132} and any(c.split and c.code == 2232 for c in CONV)


def test_query_refuses_what_the_launch_refuses(tile_mode_restored):
    for M, N, K in [(0, 64, 64), (64, 0, 64), (64, 64, 0), (64, 60, 64), (64, 64, 48), (-5, 64, 64)]:
        assert kernels.gemm_kernel_choice(M, N, K) == 0 and kernels.gemm_kernel_choice(M, N, K, conv=True) == 0
