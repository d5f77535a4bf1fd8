"""CPU: the region order of shifted windows and the key-block ranges attention32 runs against (host functions of libkvq_hip:
kvq_attn32_row_order, kvq_attn32_key_ranges) against the oracle's restatement of compute_mask (oracle/swin3d_oracle.py shift_mask)."""
import numpy as np
import pytest

import kvq_amd  # noqa: F401
import attn_ranges_ref as AR
from kvq_amd import kernels
from oracle import swin3d_oracle as O

WINDOW, SHIFT = (8, 7, 7), (4, 3, 3)
# token grids of the C2 trunk (Swin-T, 32 x 224 x 224 clip, (2,4,4) patches) at stages 0-2, and one grid whose depth the window clamps
# (D = 8: no depth shift, H / W regions only)
GRIDS = {"stage0": (16, 56, 56), "stage1": (16, 28, 28), "stage2": (16, 14, 14), "clamped_d": (8, 28, 14)}
KB = 13


def descriptors(lay, window=WINDOW):
    """[nW*N, 2] int32 descriptors in raster order, as the plan builds them"""
    N, nW = lay["N"], lay["nW"]
    _, Wh, Ww = window
    n = np.arange(N)
    code = (n // (Wh * Ww)) * (2 * Wh - 1) * (2 * Ww - 1) + ((n // Ww) % Wh) * (2 * Ww - 1) + n % Ww
    desc = lay["frag"][:, 0] | (lay["frag"][:, 1] << 8) | (lay["region"] << 16)
    return np.stack([np.tile(code, nW), desc], -1).astype(np.int32)


_cache = {}


def ordered(name):
    """(layout, order [nW, N], ranges [nW, 13, 2], un-masked [nW, N, N] bool in the region order) of a shifted grid, computed once"""
    if name not in _cache:
        lay = O.window_layout(*GRIDS[name], WINDOW, SHIFT)
        N, nW = lay["N"], lay["nW"]
        tok = descriptors(lay)
        order = kernels.attn32_row_order(tok, nW, N)
        tok_o = tok.reshape(nW, N, 2)[np.arange(nW)[:, None], order]
        ranges = kernels.attn32_key_ranges(tok_o, nW, N, True)
        open_ = O.shift_mask(lay) == 0.0
        open_ = open_[np.arange(nW)[:, None, None], order[:, :, None], order[:, None, :]]
        _cache[name] = (lay, order, ranges, open_)
    return _cache[name]


def needed_blocks(open_w, N):
    """brute force from the mask of one window: per 32-query block the bool [13] of 32-key blocks that hold an un-masked key"""
    out = np.zeros((KB, KB), bool)
    for qb in range(-(-N // 32)):
        keys = np.nonzero(open_w[32 * qb:32 * qb + 32].any(0))[0]
        out[qb, np.unique(keys >> 5)] = True
    return out


@pytest.mark.parametrize("name", list(GRIDS))
def test_no_unmasked_pair_lies_outside_the_range(name):
    lay, order, ranges, open_ = ordered(name)
    N, nW, nqb = lay["N"], lay["nW"], -(-lay["N"] // 32)
    regions = lay["region"].reshape(nW, N)
    shortened = 0
    for w in range(nW):
        need = needed_blocks(open_[w], N)
        for qb in range(nqb):
            first, last = int(ranges[w, qb, 0]), int(ranges[w, qb, 1])
            blocks = np.nonzero(need[qb])[0]
            assert 0 <= first <= last < nqb
            assert first <= blocks.min() and blocks.max() <= last, (name, w, qb, first, last, blocks)
            assert (first, last) == (blocks.min(), blocks.max())        # and no wider than the rule says
            shortened += last - first + 1 < nqb
        if len(np.unique(regions[w])) == 1:                              # a window the shift leaves whole
            assert (ranges[w, :, 0] == 0).all() and (ranges[w, :, 1] == nqb - 1).all()
    assert shortened > 0


def test_unshifted_partition_gets_the_full_range():
    lay = O.window_layout(16, 14, 14, WINDOW, (0, 0, 0))
    N, nW = lay["N"], lay["nW"]
    tok = descriptors(lay)
    assert np.array_equal(kernels.attn32_row_order(tok, nW, N), np.tile(np.arange(N, dtype=np.int32), (nW, 1)))
    ranges = kernels.attn32_key_ranges(tok, nW, N, False)
    assert (ranges[:, :, 0] == 0).all() and (ranges[:, :, 1] == KB - 1).all()
    # a small window: the range ends at the last block that holds a key
    ranges = kernels.attn32_key_ranges(tok[:200], 2, 100, False)
    assert (ranges[:, :, 0] == 0).all() and (ranges[:, :, 1] == 3).all()


@pytest.mark.parametrize("name", list(GRIDS))
def test_row_order_is_a_permutation_with_contiguous_regions(name):
    lay, order, _, _ = ordered(name)
    N, nW = lay["N"], lay["nW"]
    regions = lay["region"].reshape(nW, N)
    for w in range(nW):
        assert np.array_equal(np.sort(order[w]), np.arange(N))
        r = regions[w][order[w]]
        assert (np.diff(r) >= 0).all()                                   # sorted by region: every region one run of rows
        for v in np.unique(r):
            assert (np.diff(order[w][r == v]) > 0).all()                 # stable: raster order inside a region


def test_tile_totals_per_launch_of_swin_t_32x224x224(capsys):
    """Score tiles per shifted attention launch ((window, head) units x tiles) of Swin-T at 32 x 224 x 224: the ranges' totals equal a
    brute-force count from the mask (span of the needed key blocks of every q-block), and what the kernel runs after widening to its body
    lengths stays below the depth split alone.  The printed totals are the ones profiles/attn_ranges_ab.txt records."""
    expect_run = {}
    for name, grid in (("stage0", GRIDS["stage0"]), ("stage1", GRIDS["stage1"]), ("stage2", GRIDS["stage2"]), ("stage3", (16, 7, 7))):
        if name == "stage3":
            lay = O.window_layout(*grid, WINDOW, SHIFT)
            N, nW = lay["N"], lay["nW"]
            tok = descriptors(lay)
            order = kernels.attn32_row_order(tok, nW, N)
            assert np.array_equal(order, np.tile(np.arange(N, dtype=np.int32), (nW, 1)))     # depth regions are in raster order already
            ranges = kernels.attn32_key_ranges(tok, nW, N, True)
            open_ = O.shift_mask(lay) == 0.0
        else:
            lay, order, ranges, open_ = ordered(name)
            N, nW = lay["N"], lay["nW"]
        table = run = brute = 0
        for w in range(nW):
            need = needed_blocks(open_[w], N)
            for qb in range(KB):
                blocks = np.nonzero(need[qb])[0]
                brute += blocks.max() - blocks.min() + 1
                table += int(ranges[w, qb, 1]) - int(ranges[w, qb, 0]) + 1
                run += AR.widened(int(ranges[w, qb, 0]), int(ranges[w, qb, 1]))[1]
        slabs = lay["Dp"] // 8
        today = (nW - nW // slabs) * 169 + (nW // slabs) * 97                # all 13 x 13 tiles; the last depth slab depth-split
        expect_run[name] = (today / nW, table / nW, run / nW)
        with capsys.disabled():
            print(f"\n{name}: {nW} windows, tiles per (window, head): depth split only {today / nW:.2f}, ranges {table / nW:.2f}, "
                  f"as run (4 | 7 | 13 bodies) {run / nW:.2f}")
        assert table == brute
        assert table <= run <= today
    assert expect_run["stage3"][1] == expect_run["stage3"][2] == expect_run["stage3"][0] == 133.0      # the depth split falls out of the table
    for name in ("stage0", "stage1", "stage2"):                      # H / W edges: strictly fewer tiles, and more so the smaller the grid
        assert expect_run[name][2] < expect_run[name][0]
    assert expect_run["stage2"][2] < expect_run["stage1"][2] < expect_run["stage0"][2]
