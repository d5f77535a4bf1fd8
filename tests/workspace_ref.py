"""What the Swin trunk's forward needs of each workspace region, restated from the geometry alone.

``kvq_swin3d_plan_create`` (csrc/plan.hip) carves the caller's workspace into x0 | x1 | ln | big | o | sk.  ``region_needs`` lists,
per stage, the largest number of bytes ANY launch of ANY schedule of ``swin_run`` writes to or reads from each region — fused or
un-fused embedding, tails and merges, fp32 or fp16 streams (the fp32 form is the larger), padded or un-padded partitions, whole
forward or stage split — without looking at the plan.  L, Lp and N come from ``oracle.swin3d_oracle.window_layout``, the merged
grid from this module's own ceil-halving.

    x0, x1   the residual stream of a stage, B L C fp32; the patch merge writes the next stage's, B Ln 2C fp32, into the other one
    ln       16-bit LayerNorm rows: norm1 in window order (B Lp C) or token order (B L C), norm2 (B L C), and the un-fused
             merge's LayerNorm over the 4 gathered neighbours, B Ln 4C — more than B L C whenever H or W is odd
    big      16-bit: the im2col rows of the un-fused embedding (B L0 K0), q | k | v (B Lp 3C), the MLP hidden rows (B L mlp C)
    o        16-bit attention output in window order, B Lp C
    sk       nothing: the trunk's GEMMs run without split-K (their result must not depend on the batch)

``check_regions`` compares a reported layout with these needs and returns the list of defects.
"""
from oracle.swin3d_oracle import window_layout

REGIONS = ("x0", "x1", "ln", "big", "o", "sk")
ALIGN = 256


def ceil_div(a, b):
    return -(-a // b)


def stage_grids(T, H, W, patch, num_stages):
    """[(D, H, W)] of the token grid of every stage: the patch grid, halved (rounding up) in H and W by every merge"""
    d, h, w = ceil_div(T, patch[0]), ceil_div(H, patch[1]), ceil_div(W, patch[2])
    out = []
    for _ in range(num_stages):
        out.append((d, h, w))
        h, w = ceil_div(h, 2), ceil_div(w, 2)
    return out


def region_needs(B, T, H, W, embed_dim=96, num_stages=4, window=(8, 7, 7), patch=(2, 4, 4), in_chans=3, mlp_ratio=4, adaptive=None):
    """{region: [bytes needed by stage i]}"""
    need = {r: [] for r in REGIONS}
    grids = stage_grids(T, H, W, patch, num_stages)
    K0 = in_chans * patch[0] * patch[1] * patch[2]
    for i, (d, h, w) in enumerate(grids):
        C = embed_dim << i
        lay = window_layout(d, h, w, window, tuple(x // 2 for x in window), adaptive)
        L, Lp = d * h * w, lay["nW"] * lay["N"]
        assert Lp >= L
        last = i == num_stages - 1
        Ln = 0 if last else d * ceil_div(h, 2) * ceil_div(w, 2)
        stream = max(B * L * C * 4, B * Ln * 2 * C * 4)
        need["x0"].append(stream)
        need["x1"].append(stream)
        need["ln"].append(2 * max(B * Lp * C, B * L * C, B * Ln * 4 * C))
        need["big"].append(2 * max(B * L * K0 if i == 0 else 0, B * Lp * 3 * C, B * L * mlp_ratio * C))
        need["o"].append(2 * B * Lp * C)
        need["sk"].append(0)
    return need


def check_regions(regions, total_bytes, needs):
    """``regions``: {name: (offset, bytes)} as kvq_swin3d_workspace_regions reports them -> the list of defects"""
    problems = []
    end = 0
    for name in REGIONS:
        off, nb = regions[name]
        if off % ALIGN:
            problems.append(f"{name} starts at {off}, not a multiple of {ALIGN}")
        if off < end:
            problems.append(f"{name} starts at {off}, inside the region in front of it (which ends at {end})")
        end = off + nb
        if end > total_bytes:
            problems.append(f"{name} ends at {end}, past the workspace of {total_bytes} bytes")
        for stage, n in enumerate(needs[name]):
            if n > nb:
                problems.append(f"{name} holds {nb} bytes, stage {stage} needs {n}: short by {n - nb}")
    return problems
