"""The geometries at which the training backward kernels are held to their references: one table for the GPU tests
(tests/test_gpu_grad.py) and for the CPU guard that keeps the table honest (tests/test_grad_cases.py).

The recipe: batch 3, 4 frames, 384 x 384 crops, 6 levels (``--mode=train``), then 256 x 768 KITTI frames (``finetune_kitti``).
Not all 78 layer calls of a step are listed -- only the ones that change which code of csrc/m4d_wgrad.hip runs.

``kind`` says which loop of the weight-gradient launcher a case is there for, and tests/test_grad_cases.py recomputes from the
launcher's own arithmetic that it still reaches it:

  "multi-tile"  conv3x3_wgrad_kernel with more 8 x 16-pixel tiles than pixel slices: a workgroup walks several tiles, so the
                slice striding, the ``stage(nxt)`` refill and -- on the 16-byte stride-1 path -- the prefetch / commit pair run;
  "thin"        wgrad_thin_kernel (Cin = 3, or Cin = 16 with Cout <= 32) with more items of 8 pixels than its 2048 waves: both
                operand sets of the ping-pong and the loads in flight are used.
"""
from collections import namedtuple

ConvCase = namedtuple("ConvCase", "b h w cin cout stride kind note")

CONV_BACKWARD_RECIPE_CASES = [
    # ---- level 1 of the recipe (192 x 192 maps): 864 tiles
    ConvCase(3, 192, 192, 128, 128, 1, "multi-tile", "864 tiles on 48 slices: 18 per workgroup"),
    ConvCase(3, 192, 192, 128, 96, 1, "multi-tile", "64 slices: 13.5 per workgroup (ragged)"),
    ConvCase(3, 192, 192, 96, 64, 1, "multi-tile", "128 slices: 6.75 per workgroup (ragged)"),
    ConvCase(3, 192, 192, 64, 32, 1, "multi-tile", "the 256-slice cap: 3.375 per workgroup"),
    ConvCase(3, 192, 192, 32, 16, 1, "multi-tile", "the 256-slice cap, half-empty Cout block"),
    ConvCase(3, 192, 192, 64, 128, 1, "multi-tile", "first refiner layer of level 1: 96 slices, 9 per workgroup"),
    # ---- level 2 (96 x 96): 216 tiles
    ConvCase(3, 96, 96, 122, 128, 1, "multi-tile", "Cin = 122: the 8-byte staging kernel <1, 4, 2>, no prefetch; 4.5 per workgroup"),
    ConvCase(3, 96, 96, 128, 128, 1, "multi-tile", "48 slices: 4.5 per workgroup"),
    ConvCase(3, 96, 96, 96, 64, 1, "multi-tile", "128 slices: 1.69 per workgroup"),
    # ---- level 3 (48 x 48): 54 tiles on 48 slices, 6 workgroups take a second tile
    ConvCase(3, 48, 48, 128, 128, 1, "multi-tile", "1.125 per workgroup"),
    # ---- the thin kernel
    ConvCase(3, 384, 384, 3, 16, 1, "thin", "the image layer: 55296 items, 27 per wave"),
    ConvCase(3, 384, 384, 16, 16, 2, "thin", "encoder level 0, stride 2: 6.75 per wave"),
    ConvCase(3, 192, 192, 16, 32, 1, "thin", "wgrad_thin_kernel<16, 1>: 6.75 per wave"),
    ConvCase(3, 192, 192, 16, 5, 1, "thin", "last refiner layer: 27 of 32 MFMA rows empty"),
    # ---- stride 2 with more than one tile per workgroup: the KITTI finetuning geometry (3 x 256 x 768) and one synthetic case
    ConvCase(3, 128, 384, 32, 32, 2, "multi-tile", "KITTI encoder level 1: 288 tiles on 256 slices"),
    ConvCase(3, 256, 768, 16, 16, 2, "thin", "KITTI encoder level 0: 18432 items on 2048 waves"),
    ConvCase(3, 192, 192, 128, 128, 2, "multi-tile", "synthetic (no such layer in the model): 216 tiles on 48 slices, stride 2"),
    # ---- odd-sized large maps: ragged edge tiles and several tiles per workgroup meet
    ConvCase(2, 101, 203, 96, 64, 1, "multi-tile", "338 tiles on 128 slices"),
    ConvCase(2, 101, 203, 128, 128, 2, "multi-tile", "98 tiles on 48 slices"),
]


def conv_case_id(c):
    return f"{c.b}x{c.h}x{c.w}-{c.cin}to{c.cout}-s{c.stride}"


# (h, w, C, cuts) of the cost volumes at the six levels of a 384 x 384 crop, and level 1 of a 256 x 768 KITTI frame
CV_RECIPE_LEVELS = [(192, 192, 16, 1), (96, 96, 32, 2), (48, 48, 64, 2), (24, 24, 96, 4), (12, 12, 128, 4), (6, 6, 192, 8),
                    (128, 384, 16, 1)]
