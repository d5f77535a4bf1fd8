"""CPU: the two independent checkers of the plan workspaces name each defect they are there to find (tests/plan_layout_check.py,
tests/workspace_ref.py) and pass layouts without one.  tests/test_gpu_workspace.py runs them on the plans of the library."""
import pytest

import plan_layout_check as P
import workspace_ref as R


def _op(lane, reads=(), writes=(), wait=-1):
    return {"lane": lane, "reads": list(reads), "writes": list(writes), "wait": wait}


def _layout(slots, ops, ws_bytes=4096, scratch=((3072, 1024),)):
    return {"ws_bytes": ws_bytes, "scratch": list(scratch), "slots": [tuple(s) for s in slots], "ops": ops}


INPUT = (0, 0, 0)        # slot 0 of every layout below: the caller's input pointer, not in the workspace


def test_a_clean_one_lane_layout_with_a_recycled_slot_passes():
    # slot 3 takes slot 1's bytes after slot 1's last reader
    lay = _layout([INPUT, (0, 512, 1), (512, 512, 1), (0, 256, 1)],
                  [_op(0, [0], [1]), _op(0, [1], [2]), _op(0, [2], [3]), _op(0, [3])])
    assert P.check(lay) == []
    assert P.live_intervals(lay) == {1: (0, 1), 2: (1, 2), 3: (2, 3)}


def test_two_live_slots_sharing_bytes_are_named():
    lay = _layout([INPUT, (0, 512, 1), (256, 512, 1)], [_op(0, [0], [1]), _op(0, [0], [2]), _op(0, [1, 2])])
    got = P.check(lay)
    assert got == ["slots 1 and 2 share bytes while both are live (ops 0..2 and 1..2)"]
    # recycled one op too early: slot 2 is written by the op that still reads slot 1
    lay = _layout([INPUT, (0, 512, 1), (0, 512, 1)], [_op(0, [0], [1]), _op(0, [1], [2]), _op(0, [2])])
    assert P.check(lay) == ["slots 1 and 2 share bytes while both are live (ops 0..1 and 1..2)"]


def test_a_slot_reaching_into_the_scratch_or_past_the_workspace_is_named():
    lay = _layout([INPUT, (2816, 512, 1)], [_op(0, [0], [1]), _op(0, [1])])
    assert P.check(lay) == ["slot 1 [2816, 3328) reaches into the scratch of lane 0 [3072, 4096)"]
    lay = _layout([INPUT, (0, 512, 1)], [_op(0, [0], [1]), _op(0, [1])], ws_bytes=4096, scratch=((3584, 1024),))
    assert P.check(lay) == ["scratch of lane 0 [3584, 4608) ends past the workspace of 4096 bytes"]
    lay = _layout([INPUT, (0, 512, 1)], [_op(0, [0], [1]), _op(1, [0], [])], scratch=((2048, 1024), (2816, 1024)))
    assert P.check(lay) == ["scratch of lane 0 overlaps the scratch of lane 1"]


def test_a_read_of_a_slot_nobody_wrote_is_named():
    lay = _layout([INPUT, (0, 512, 1), (512, 512, 1)], [_op(0, [1], [2]), _op(0, [0], [1])])
    assert "op 0 reads slot 1 before any op has written it" in P.check(lay)


TWO = ((2048, 1024), (3072, 1024))


def test_a_cross_lane_write_and_read_without_an_edge_is_named():
    lay = _layout([INPUT, (0, 512, 1)], [_op(0, [0], [1]), _op(1, [1])], scratch=TWO)
    assert P.check(lay) == ["op 0 (lane 0, slot 1) and op 1 (lane 1, slot 1) touch the same bytes, one of them writing, with no "
                            "ordering between the lanes"]
    # bytes recycled across lanes: the live intervals are disjoint in program order (check 2 is content), but the other lane's
    # write may run beside the write of slot 1 and beside its reader, which writes slot 2
    lay = _layout([INPUT, (0, 512, 1), (512, 512, 1), (256, 512, 1)],
                  [_op(0, [0], [1]), _op(0, [1], [2]), _op(1, [0], [3])], scratch=TWO)
    got = P.check(lay)
    assert len(got) == 2 and all("no ordering between the lanes" in g for g in got) and "op 0 " in got[0] and "op 1 " in got[1], got
    # with the edge it passes; two reads need none
    lay = _layout([INPUT, (0, 512, 1)], [_op(0, [0], [1]), _op(1, [1], wait=0), _op(0, [1])], scratch=TWO)
    assert P.check(lay) == []
    # an edge to an op enqueued later orders nothing
    lay = _layout([INPUT, (0, 512, 1)], [_op(0, [0], [1]), _op(1, [1], wait=2), _op(0, [1])], scratch=TWO)
    got = P.check(lay)
    assert "op 1 waits for op 2, which is not enqueued before it" in got and any("no ordering between the lanes" in g for g in got)


def test_a_conflict_ordered_only_transitively_passes():
    # op 0 writes A, op 1 (same lane) writes B, op 2 (other lane) waits for op 1, op 3 (same lane as 2) reads A with no wait of its own
    lay = _layout([INPUT, (0, 512, 1), (512, 512, 1)],
                  [_op(0, [0], [1]), _op(0, [0], [2]), _op(1, [2], wait=1), _op(1, [1])], scratch=TWO)
    assert P.check(lay) == []
    anc = P.happens_before(lay)
    assert anc[3] == 0b0111 and anc[2] == 0b0011
    # the wait one op too early (for op 0 instead of op 1) leaves op 1 -> op 2 open
    lay["ops"][2]["wait"] = 0
    assert P.check(lay) == ["op 1 (lane 0, slot 2) and op 2 (lane 1, slot 2) touch the same bytes, one of them writing, with no "
                            "ordering between the lanes"]


# ---- the Swin regions -----------------------------------------------------------------------------------------------------
def _carve(sizes):
    regions, off = {}, 0
    for name in R.REGIONS:
        regions[name] = (off, sizes[name])
        off += -(-sizes[name] // R.ALIGN) * R.ALIGN
    return regions, off


def _sizes(needs, ln_without_merge_rows=False, B=1, geometry=None):
    sizes = {name: max(v) for name, v in needs.items()}
    if ln_without_merge_rows:           # ln sized for the norm1 / norm2 rows only: max(B Lp C, B L C) 16-bit elements
        T, H, W = geometry
        rows = []
        for i, (d, h, w) in enumerate(R.stage_grids(T, H, W, (2, 4, 4), 4)):
            lay = R.window_layout(d, h, w, (8, 7, 7), (4, 3, 3))
            rows.append(2 * B * max(lay["nW"] * lay["N"], d * h * w) * (96 << i))
        sizes["ln"] = max(rows)
    return sizes


def test_stage_grids_halve_rounding_up():
    assert R.stage_grids(16, 84, 84, (2, 4, 4), 4) == [(8, 21, 21), (8, 11, 11), (8, 6, 6), (8, 3, 3)]
    assert R.stage_grids(10, 50, 70, (2, 4, 4), 4) == [(5, 13, 18), (5, 7, 9), (5, 4, 5), (5, 2, 3)]


@pytest.mark.parametrize("geometry,B,short", [((16, 84, 84), 1, 66048), ((16, 28, 28), 1, 23040), ((16, 140, 140), 1, 109056),
                                              ((16, 84, 84), 2, 132096)])
def test_region_check_names_an_ln_region_without_the_merge_rows(geometry, B, short):
    """Swin-T, window (8,7,7): an odd token grid whose extent is a multiple of the window (or no larger than it) has 4 Ln > L and
    Lp == L, so an ``ln`` sized for the norm1 / norm2 rows alone is short of the un-fused merge's LayerNorm rows by these amounts."""
    needs = R.region_needs(B, *geometry)
    regions, total = _carve(_sizes(needs, True, B, geometry))
    got = R.check_regions(regions, total, needs)
    assert len(got) == 1 and got[0].startswith("ln holds ") and got[0].endswith(f": short by {short}"), got
    regions, total = _carve(_sizes(needs))
    assert R.check_regions(regions, total, needs) == []


def test_region_check_names_overlap_misalignment_and_overrun():
    needs = R.region_needs(1, 16, 64, 64)
    regions, total = _carve(_sizes(needs))
    assert R.check_regions(regions, total, needs) == []          # even grids: 4 Ln == L, nothing to add
    assert _sizes(needs, True, 1, (16, 64, 64))["ln"] == _sizes(needs)["ln"]
    bad = dict(regions)
    bad["big"] = (regions["big"][0] - 256, regions["big"][1])
    assert any(g.startswith("big starts at") and "inside the region in front of it" in g for g in R.check_regions(bad, total, needs))
    bad = dict(regions)
    bad["o"] = (regions["o"][0] + 16, regions["o"][1])
    assert any("not a multiple of 256" in g for g in R.check_regions(bad, total, needs))
    assert any(g.startswith("sk ends at") or g.startswith("o ends at") for g in R.check_regions(regions, regions["o"][0] + 256, needs))
