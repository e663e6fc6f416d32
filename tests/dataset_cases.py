"""The geometries the network evaluates the datasets at: one table for the GPU tests (tests/test_gpu_datasets.py) and for the
CPU guard that keeps the table honest (tests/test_dataset_cases.py).

Sizes: each loader's default network size (``_set_output_size`` without an argument) -- KITTI 256 x 768, Mid-Air 384 x 384,
TartanAir 384 x 512 -- with six levels: pyramids that end in 4 x 12, 6 x 6 and 6 x 8 maps.  Batches: 1 (plain streaming
evaluation and predict), 3 (the README's validation / evaluation recipe), 8 (``--eval_streams 8``).

From these, per level, ``(b, h, w, C, cuts)`` and every refiner layer call ``(b, h, w, cin, cout, final)`` -- built the way
``test_conv_dispatch.layer_calls`` builds them (refiner input padded to a multiple of 8 channels, the ``final`` flag of each
caller) -- and ``dispatch`` = what the model runs there, computed on the CPU from ``_Conv3x3SameTF.plan``,
``network_ops.lat_config`` (inside ``plan``) and ``DepthEstimatorLevel._front_by_size`` / ``wants_prenormalized``.

The GPU cases of tests/test_gpu_datasets.py are listed here as well, so that the guard can say which of the kernels the
datasets run no GPU case reaches."""
from collections import namedtuple

import numpy as np

from m4depth_amd.synthetic import ENCODER_CHANNELS, REFINER_CHANNELS, nbre_cuts_for

LEVELS = 6
EVAL_BATCHES = (1, 3, 8)
ARITHS = ("f16x2", "bf16x3", "f32")
DATASETS = ("kitti", "midair", "tartanair")
# the intrinsics row of a KITTI trajectory file, normalised by the image size (the ratios helpers.make_fake_dataset writes)
KITTI_ROW = {"fx": 0.58, "fy": 1.92, "cx": 0.49, "cy": 0.51}


def _loader(name):
    from m4depth_amd import dataloaders as D
    loader = D.get_loader({"kitti": "kitti-raw"}.get(name, name))
    loader._set_output_size()                       # the default: what ``get_dataset`` does without an ``out_size``
    return loader


def network_size(name):
    """(H, W) the loader resizes to by default."""
    return tuple(int(v) for v in _loader(name).out_size)


def camera_np(name, b):
    """The loader's own intrinsics at its default size, for a batch of ``b``: {"f", "c"} [b, 2] float32."""
    f, c = _loader(name)._camera(KITTI_ROW)
    return {"f": np.tile(np.array([f], np.float32), [b, 1]), "c": np.tile(np.array([c], np.float32), [b, 1])}


def level_map(H, W, depth):
    return -(-H // 2 ** depth), -(-W // 2 ** depth)


def level_rows(H, W, b):
    """(depth, b, h, w, C, cuts) of the six levels."""
    return [(d, b, *level_map(H, W, d), ENCODER_CHANNELS[d - 1], nbre_cuts_for(d)) for d in range(1, LEVELS + 1)]


_MODEL = []


def model():
    from m4depth_amd import network as N
    if not _MODEL:
        _MODEL.append(N.M4Depth(nbre_levels=LEVELS))
    return _MODEL[0]


LayerCall = namedtuple("LayerCall", "depth ci b h w cin cout final callers")


def refiner_calls(depth, b, h, w):
    """Every call of the level's seven refiner layers on a [b, h, w] map, as ``test_conv_dispatch.layer_calls`` lists them.
    ``callers``: "level" = the loop of ``DepthEstimatorLevel.forward`` in front of the fused tail (layers 0-4, what the model
    runs), "refiner" = ``DispRefiner.forward`` (all seven)."""
    lvl = model().d_estimator.levels[depth - 1]
    widths = [(lvl.f_in + 7) // 8 * 8] + list(REFINER_CHANNELS[:-1])
    out = []
    for ci in range(7):
        callers = {}
        callers.setdefault(ci < 3 or ci == 6, []).append("refiner")
        if ci < 5:
            callers.setdefault(ci == 4, []).append("level")
        for final in sorted(callers):
            out.append(LayerCall(depth, ci, b, h, w, widths[ci], REFINER_CHANNELS[ci], final, tuple(callers[final])))
    return out


def conv_of(call):
    lvl = model().d_estimator.levels[call.depth - 1]
    return (list(lvl.disp_refiner.prep_conv_layers) + list(lvl.disp_refiner.est_d_conv_layers))[call.ci]


def conv_row(call):
    """(wrapper, layout, lat_config) of a layer call under the arithmetic in force."""
    from m4depth_amd import network as N
    p = conv_of(call).plan(call.b, call.h, call.w, call.cin, call.final)
    return N._CONV_LAUNCH[p.kernel][0], p.layout, None if p.lat_config is None else tuple(int(v) for v in p.lat_config)


def front_form(depth, b, h, w):
    """"F" = the big-tile fused front (m4d_level_front_r), "s" = the one-launch small front on prenormalised features
    (m4d_level_front_small), "-" = neither (level_pre, then the cost volumes)."""
    lvl = model().d_estimator.levels[depth - 1]
    shape = (b, h, w, ENCODER_CHANNELS[depth - 1])
    if lvl._front_by_size(*shape):
        return "F"
    return "s" if lvl.wants_prenormalized(*shape) else "-"


def level_dispatch(depth, b, h, w, callers=("level",)):
    """{(wrapper, layout, lat_config, front form)} of the level's layer calls made by ``callers``."""
    form = front_form(depth, b, h, w)
    return {conv_row(c) + (form,) for c in refiner_calls(depth, b, h, w) if set(c.callers) & set(callers)}


def dataset_dispatch(callers=("level",)):
    """{(dataset, batch, depth): {(wrapper, layout, lat_config, front form)}} over the three datasets and batches."""
    out = {}
    for name in DATASETS:
        H, W = network_size(name)
        for b in EVAL_BATCHES:
            for d, _, h, w, _, _ in level_rows(H, W, b):
                out[(name, b, d)] = level_dispatch(d, b, h, w, callers)
    return out


# ------------------------------------------------------------------------------- the GPU cases of tests/test_gpu_datasets.py
# (a) cost volumes: (h, w, C, cuts), each at batch 1 and 3
CV_CASES = [(4, 12, 192, 8), (6, 6, 192, 8), (6, 8, 192, 8), (8, 24, 128, 4), (12, 12, 128, 4), (12, 16, 128, 4), (16, 48, 96, 4)]
CV_BATCHES = (1, 3)
CV_VARIANT_MAPS = [(4, 12), (6, 6)]                # every DSCV variant and the merged entry on these

# (b) level fronts: (depth, b, h, w, quat, cv_accum)
FRONT_SMALL_CASES = [(6, 1, 4, 12, True, "fp32_round"), (6, 3, 6, 6, False, "fp16_seq"), (6, 1, 6, 8, True, "fp16_seq"),
                     (5, 1, 8, 24, False, "fp32_round"), (5, 3, 12, 12, True, "fp32_round"), (4, 1, 16, 48, True, "fp16_seq")]
FRONT_FUSED_CASES = [(4, 8, 16, 48, True, "fp32_round"), (3, 1, 32, 96, False, "fp16_seq")]

# (c) one whole level, teacher-forced: (depth, h, w) -- the level-3 map in the default form only
LEVEL_MAPS = [(6, 4, 12), (6, 6, 6), (6, 6, 8), (5, 8, 24), (5, 12, 12), (5, 12, 16), (4, 16, 48), (4, 24, 24), (4, 24, 32),
              (3, 32, 96)]


def level_step_cases():
    """(depth, b, h, w, form).  ``form`` False = the level called without prenormalised features: the fused front where the map
    takes it by size, ``level_pre`` + the merged cost-volume launch elsewhere; "small" = the one-launch small front on
    prenormalised features, what the model runs on a coarse map of at most 6000 pixels.  At batch 8 the 16 x 48 and 24 x 32
    maps have 6144 pixels: the small front does not exist there (``wants_prenormalized`` is False), so these two have the
    default form only."""
    out = []
    for depth, h, w in LEVEL_MAPS:
        for b in (1, 3) + ((8,) if depth == 4 else ()):
            out.append((depth, b, h, w, False))
            if depth > 3 and front_form(depth, b, h, w) == "s":
                out.append((depth, b, h, w, "small"))
    return out


# (d) the refiner chain on its own: every map of (c) at batch 1 and 3, under the default arithmetic and "bf16x3"
REFINER_ARITHS = ("f16x2", "bf16x3")


def refiner_cases():
    return [(depth, b, h, w) for depth, h, w in LEVEL_MAPS for b in (1, 3)]


# (e) the whole model: every dataset's size, six levels, batch 1
MODEL_BATCH = 1
MODEL_FRAMES = 3
# seeds of S.make_sequence(..., motion="lateral"): chosen so that the float32 oracle alone meets check_depth_and_parallax's
# ``frac_ok`` against the float64 oracle at every level, checked on the CPU before the seeds were settled (for KITTI, whose
# float64 oracle the GPU test pays for anyway, tests/test_gpu_datasets.py asserts it again)
MODEL_SEEDS = {"kitti": 2561, "midair": 3841, "tartanair": 3842}


def gpu_covered():
    """{(wrapper, layout, lat_config, front form)} the GPU cases (c) and (e) run through ``DepthEstimatorLevel.forward`` under the
    arithmetic in force.  A default-form case on a map without the fused front opens with neither one-launch front ("-")."""
    got = set()
    for depth, b, h, w, form in level_step_cases():
        rows = level_dispatch(depth, b, h, w)
        got |= rows if form == "small" or front_form(depth, b, h, w) == "F" else {r[:3] + ("-",) for r in rows}
    for name in DATASETS:
        for d, b, h, w, _, _ in level_rows(*network_size(name), MODEL_BATCH):
            got |= level_dispatch(d, b, h, w)
    return got
