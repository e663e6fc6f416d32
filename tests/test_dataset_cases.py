"""CPU guard of the dataset geometries (tests/dataset_cases.py): the sizes come from the loaders, and every fact
tests/test_gpu_datasets.py rests on -- which kernel a level of a dataset's pyramid runs at batch 1, 3 and 8 -- is recomputed
from ``_Conv3x3SameTF.plan`` (``network_ops.lat_config`` inside it) and ``DepthEstimatorLevel._front_by_size`` /
``wants_prenormalized``.  The library loads without a device.  If a threshold moves, the message names the case that lost
its reason."""
import pytest

import dataset_cases as DC
from m4depth_amd import network as N

DIRECT = "conv3x3_bias_act"
LAT = {"f16x2": "conv3x3_lat_f16", "bf16x3": "conv3x3_lat"}
WINO = {"f16x2": ("conv3x3_wino6_bias_act", "winof16"), "bf16x3": ("conv3x3_wino6_bias_act", "wino6")}


def _level(name, b, depth):
    return DC.level_rows(*DC.network_size(name), b)[depth - 1][1:4]


def _wrappers(name, b, depth, callers=("level", "refiner")):
    """The wrapper of every layer call of the level (both callers: the model's loop and ``DispRefiner.forward``)."""
    return [DC.conv_row(c)[0] for c in DC.refiner_calls(depth, *_level(name, b, depth)) if set(c.callers) & set(callers)]


def test_sizes_are_the_loaders_defaults():
    want = {"kitti": (256, 768), "midair": (384, 384), "tartanair": (384, 512)}
    for name in DC.DATASETS:
        assert DC.network_size(name) == want[name], f"{name}: the loader's default network size is {DC.network_size(name)}"
    coarsest = {name: DC.level_rows(*DC.network_size(name), 1)[-1][2:4] for name in DC.DATASETS}
    assert coarsest == {"kitti": (4, 12), "midair": (6, 6), "tartanair": (6, 8)}, coarsest
    assert DC.EVAL_BATCHES == (1, 3, 8)


def test_cameras_are_the_loaders_own():
    """KITTI: the csv ratios times the size; Mid-Air: f = c = half the size; TartanAir: fy = 2/3 H -- none is ``camera_np``'s
    for KITTI and TartanAir."""
    k, m, t = (DC.camera_np(n, 2) for n in DC.DATASETS)
    assert k["f"].shape == (2, 2) and k["f"][1].tolist() == pytest.approx([0.58 * 768, 1.92 * 256], rel=1e-6)
    assert k["c"][0].tolist() == pytest.approx([0.49 * 768, 0.51 * 256], rel=1e-6)
    assert m["f"][0].tolist() == [192.0, 192.0] and m["c"][0].tolist() == [192.0, 192.0]
    assert t["f"][0].tolist() == [256.0, 256.0] and t["c"][0].tolist() == [256.0, 192.0]


def test_the_gpu_cases_are_the_datasets_maps():
    """Every map of the GPU cases is a level of one of the three pyramids, with that level's channels and cuts."""
    maps = {(d, h, w): (C, k) for name in DC.DATASETS for d, _, h, w, C, k in DC.level_rows(*DC.network_size(name), 1)}
    for h, w, C, k in DC.CV_CASES:
        assert any((d, h, w) in maps and maps[(d, h, w)] == (C, k) for d in range(1, 7)), (h, w, C, k)
    for d, _, h, w, _, _ in DC.FRONT_SMALL_CASES + DC.FRONT_FUSED_CASES:
        assert (d, h, w) in maps, (d, h, w)
    for d, h, w in DC.LEVEL_MAPS:
        assert (d, h, w) in maps, (d, h, w)
    for d in (4, 5, 6):                                    # every coarse map of every dataset is a level-step case
        for name in DC.DATASETS:
            assert (d, *_level(name, 1, d)[1:]) in DC.LEVEL_MAPS, (name, d)
    assert set(DC.MODEL_SEEDS) == set(DC.DATASETS)


@pytest.mark.parametrize("arith", DC.ARITHS)
def test_front_forms(arith):
    """Levels 1-3 open with the fused front at every batch; levels 5 and 6 with the small front; level 4 with the small front
    at batch 1 and 3, at batch 8 with the fused front for KITTI and TartanAir (6144 pixels) and the small one for Mid-Air."""
    with N.conv_arithmetic(arith):
        for name in DC.DATASETS:
            for b in DC.EVAL_BATCHES:
                forms = "".join(DC.front_form(d, *_level(name, b, d)) for d in range(1, 7))
                want = "FFFFss" if b == 8 and name != "midair" else "FFFsss"
                assert forms == want, f"{name} batch {b}: fronts {forms}, the GPU cases assume {want}"
        for d, b, h, w, _, _ in DC.FRONT_SMALL_CASES:
            assert DC.front_form(d, b, h, w) == "s", f"small-front case {(d, b, h, w)} no longer takes the small front"
        for d, b, h, w, form in DC.level_step_cases():
            assert form != "small" or DC.front_form(d, b, h, w) == "s", (d, b, h, w)
        # (the fused-front cases force the fused front on their maps: only the batch-8 KITTI one takes it by size)
        assert DC.front_form(4, 8, 16, 48) == "F"
        assert (4, 8, 16, 48, True, "fp32_round") in DC.FRONT_FUSED_CASES


@pytest.mark.parametrize("arith", DC.ARITHS)
def test_level_3_at_batch_1_is_all_direct(arith):
    with N.conv_arithmetic(arith):
        for name in DC.DATASETS:
            got = set(_wrappers(name, 1, 3))
            assert got == {DIRECT}, f"{name} level 3 at batch 1 {_level(name, 1, 3)}: runs {sorted(got)}, not the direct kernel alone"


@pytest.mark.parametrize("arith", DC.ARITHS)
def test_level_4_at_batch_3_is_direct_but_for_midair(arith):
    """3 x 768 pixels > 2048: KITTI and TartanAir leave the latency-first / one-launch kernels for the direct split-K kernel;
    Mid-Air's 3 x 576 pixels stay."""
    with N.conv_arithmetic(arith):
        for name in ("kitti", "tartanair"):
            got = set(_wrappers(name, 3, 4))
            assert got == {DIRECT}, f"{name} level 4 at batch 3 {_level(name, 3, 4)}: runs {sorted(got)}, not the direct kernel alone"
        stays = LAT.get(arith, "conv3x3_small_bias_act")
        got = set(_wrappers("midair", 3, 4))
        assert got == {stays}, f"midair level 4 at batch 3: runs {sorted(got)}, not {stays} alone"
        for name in DC.DATASETS:                           # ... and at batch 1 every dataset's level 4 is on that kernel
            assert set(_wrappers(name, 1, 4)) == {stays}, (name, _wrappers(name, 1, 4))


@pytest.mark.parametrize("arith", ["f16x2", "bf16x3"])
def test_level_4_at_batch_8_is_winograd(arith):
    """The third path level 4 takes: the 16-bit-split Winograd kernel on its wide layers (behind the fused front for KITTI and
    TartanAir, behind the small front for Mid-Air)."""
    with N.conv_arithmetic(arith):
        for name in DC.DATASETS:
            rows = [DC.conv_row(c)[:2] for c in DC.refiner_calls(4, *_level(name, 8, 4)) if "level" in c.callers]
            assert rows[:3] == [WINO[arith]] * 3, f"{name} level 4 at batch 8: layers 0-2 run {rows[:3]}"


@pytest.mark.parametrize("arith", ["f16x2", "bf16x3"])
def test_levels_5_and_6_are_latency_kernels_that_hand_slabs_on(arith):
    with N.conv_arithmetic(arith):
        for name in DC.DATASETS:
            for b in DC.EVAL_BATCHES:
                for d in (5, 6):
                    rows = [DC.conv_row(c) for c in DC.refiner_calls(d, *_level(name, b, d)) if c.ci < 5]
                    what = f"{name} batch {b} level {d} {_level(name, b, d)}"
                    assert {r[0] for r in rows} == {LAT[arith]}, f"{what}: runs {sorted({r[0] for r in rows})}"
                    assert any(r[2][2] > 1 for r in rows), f"{what}: no layer hands partial-sum slabs on ({[r[2] for r in rows]})"
        # the configurations the issue names, with the M-tile counts of their maps (8 x 4 pixels per M-tile)
        first = {c.ci: DC.conv_row(c) for c in DC.refiner_calls(6, 1, 6, 8) if "level" in c.callers}
        assert first[0][2] == (1, 4, 4) and [c.cin for c in DC.refiner_calls(6, 1, 6, 8)][0] == 472
        assert DC.conv_row(DC.LayerCall(6, 4, 1, 4, 12, 64, 32, True, ("level",)))[2] == (1, 4, 1)
        for h, w in ((4, 12), (6, 6), (6, 8)):
            assert 2 <= -(-h // 4) * -(-w // 8) <= 3


def test_f32_levels_5_and_6_never_take_the_latency_kernels():
    with N.conv_arithmetic("f32"):
        for name in DC.DATASETS:
            for b in DC.EVAL_BATCHES:
                for d in (5, 6):
                    assert not set(_wrappers(name, b, d)) & set(LAT.values()), (name, b, d)


def test_every_kernel_the_datasets_run_is_reached_by_a_gpu_case():
    """Every distinct (wrapper, layout, lat_config, front form) of the model's refiner layers over the three datasets and batches
    1, 3 and 8, under the default arithmetic, is run by a teacher-forced level case or a whole-model case of
    tests/test_gpu_datasets.py."""
    with N.conv_arithmetic("f16x2"):
        covered = DC.gpu_covered()
        for (name, b, d), rows in sorted(DC.dataset_dispatch().items()):
            missing = rows - covered
            assert not missing, f"{name} batch {b} level {d} {_level(name, b, d)}: no GPU case runs {sorted(missing, key=str)}"


@pytest.mark.parametrize("arith", DC.REFINER_ARITHS)
def test_the_refiner_chain_cases_reach_the_slab_hand_over_and_the_direct_kernel(arith):
    """``DispRefiner.forward`` on the coarse maps: latency kernels with partial-sum slabs between layers 3-5 on levels 5 and 6,
    the direct kernel on level 3 and on the 768-pixel level-4 maps at batch 3."""
    with N.conv_arithmetic(arith):
        seen = set()
        for d, b, h, w in DC.refiner_cases():
            for c in DC.refiner_calls(d, b, h, w):
                if "refiner" in c.callers:
                    wrapper, _, cfg = DC.conv_row(c)
                    seen.add((wrapper, cfg is not None and cfg[2] > 1))
        assert (LAT[arith], True) in seen and (LAT[arith], False) in seen and (DIRECT, False) in seen, seen
