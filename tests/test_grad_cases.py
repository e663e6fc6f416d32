"""CPU guard of the recipe-geometry backward cases (tests/grad_cases.py): every case marked "multi-tile" / "thin" must still
reach the loop it was written for.  The counts come from the launcher's own arithmetic through the C ABI (the library loads
without a device), so if someone retunes the pixel split of m4d_conv3x3_wgrad this test names the cases that went blind."""
import pytest

from grad_cases import CONV_BACKWARD_RECIPE_CASES, conv_case_id

TILE_H, TILE_W = 8, 16       # kTH, kTW of csrc/m4d_wgrad.hip:25 (the output-pixel tile of one staging round)
THIN_WAVES = 2048            # csrc/m4d_wgrad.hip:419: at most 512 workgroups of 4 waves
THIN_ITEM = 8                # csrc/m4d_wgrad.hip:284-285: an item is 8 output pixels of a row


def _is_thin(c):
    return c.cin < 8 or (c.cin == 16 and c.cout <= 32)       # the dispatch of csrc/m4d_wgrad.hip:416


def tiles_and_slices(c, lib):
    """(tiles, slices) of conv3x3_wgrad_kernel's launch (csrc/m4d_wgrad.hip:433-437)."""
    oh, ow = -(-c.h // c.stride), -(-c.w // c.stride)
    block = 9 * 32 * -(-c.cout // 32) * 32 * -(-c.cin // 32)
    ws = int(lib.m4d_conv3x3_wgrad_workspace_floats(c.b, c.h, c.w, c.cin, c.cout, c.stride))
    assert ws > 0 and ws % block == 0, (ws, block)
    tiles = c.b * -(-oh // TILE_H) * -(-ow // TILE_W)
    return tiles, min(ws // block, tiles)


def thin_items(c):
    oh, ow = -(-c.h // c.stride), -(-c.w // c.stride)
    return c.b * oh * -(-ow // THIN_ITEM)


@pytest.mark.parametrize("case", CONV_BACKWARD_RECIPE_CASES, ids=conv_case_id)
def test_recipe_cases_reach_the_loops_they_are_listed_for(case):
    from m4depth_amd._lib import lib
    assert case.kind in ("multi-tile", "thin"), case
    if case.kind == "thin":
        assert _is_thin(case), f"{case}: not dispatched to wgrad_thin_kernel"
        items = thin_items(case)
        assert items > THIN_WAVES, f"{case}: {items} items on {THIN_WAVES} waves -- no wave takes a second item"
    else:
        assert not _is_thin(case), f"{case}: dispatched to wgrad_thin_kernel"
        tiles, slices = tiles_and_slices(case, lib)
        assert tiles > slices, f"{case}: {tiles} tiles on {slices} slices -- every workgroup stages one tile only"


def test_the_table_covers_every_staging_variant():
    """The 16-byte prefetching kernel, the 8-byte one (Cin even, not a multiple of 4), stride 2, and all three thin kernels."""
    multi = [c for c in CONV_BACKWARD_RECIPE_CASES if c.kind == "multi-tile"]
    thin = [c for c in CONV_BACKWARD_RECIPE_CASES if c.kind == "thin"]
    assert any(c.stride == 1 and c.cin % 4 == 0 and c.cout % 4 == 0 for c in multi)
    assert any(c.stride == 1 and c.cin % 4 == 2 for c in multi)
    assert any(c.stride == 2 for c in multi)
    assert {(c.cin, c.stride) for c in thin} == {(3, 1), (16, 1), (16, 2)}
    assert any(c.cout == 5 for c in thin)
