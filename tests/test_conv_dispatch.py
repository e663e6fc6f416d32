"""The convolution dispatch against a recorded snapshot (CPU only: the library loads without a device).

``tests/golden/conv_dispatch_snapshot.json`` was recorded from ``_Conv3x3SameTF.forward`` itself -- the ``network_ops.conv3x3_*``
launch wrappers replaced by recorders, the input a shape-only stand-in -- at commit 60d4868, BEFORE the dispatch rules moved
into ``_Conv3x3SameTF.plan``: the expected values come from that code path, not from ``plan``.  Per row: the wrapper called,
the packed layout it read, ``cout_pad``, the latency-kernel configuration, the Winograd kernel argument, the stagger, and
whether the result is a ``PartialAct``."""
import json
import os

import torch

from m4depth_amd import network as N
from m4depth_amd import network_ops as nops
from m4depth_amd.synthetic import ENCODER_CHANNELS, REFINER_CHANNELS

SNAPSHOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_dispatch_snapshot.json")
ARITHS = ("f16x2", "bf16x3", "f32")
# name: (H, W, levels, sequence batch, frames stacked per encoder launch).  A 4-frame step under the default encoder split
# encodes two batches of two frames; a streamed frame is encoded alone.
WORKLOADS = {
    "128x256_L3_b1": (128, 256, 3, 1, 2),
    "384x1280_L6_b1": (384, 1280, 6, 1, 2),
    "384x1280_L6_b8": (384, 1280, 6, 8, 2),
    "384x1280_L6_b32": (384, 1280, 6, 32, 2),
    "768x2560_L6_b1": (768, 2560, 6, 1, 2),
    "stream_384x1280_L6_b4": (384, 1280, 6, 4, 1),
}
_MODELS = {}


def model_for(levels):
    if levels not in _MODELS:
        torch.manual_seed(0)
        _MODELS[levels] = N.M4Depth(nbre_levels=levels)
    return _MODELS[levels]


def layer_calls(model, H, W, b, stack):
    """Every ``(tag, layer, input shape, final)`` call of the convolution layers in one step of the workload: the encoder on
    ``stack`` frames of a batch-``b`` sequence, every refiner layer on its level's map with the refiner input padded to a
    multiple of 8 channels, with the ``final`` flag of each caller (the fused-tail loop of ``DepthEstimatorLevel.forward``
    and ``DispRefiner.forward``)."""
    enc = model.encoder
    enc.set_sequence_batch(b)
    cin = [3] + list(enc.out_sizes[:-1])
    for i, (s1, s2) in enumerate(zip(enc.conv_layers_s1, enc.conv_layers_s2)):
        h, w = -(-H // 2 ** i), -(-W // 2 ** i)
        yield f"enc.s1.{i}", s1, (stack * b, h, w, cin[i]), True
        yield f"enc.s2.{i}", s2, (stack * b, h, w, enc.out_sizes[i]), True
    for lvl in model.d_estimator.levels:
        d = lvl.lvl_depth
        h, w = -(-H // 2 ** d), -(-W // 2 ** d)
        convs = list(lvl.disp_refiner.prep_conv_layers) + list(lvl.disp_refiner.est_d_conv_layers)
        widths = [(lvl.f_in + 7) // 8 * 8] + list(REFINER_CHANNELS[:-1])
        for ci, conv in enumerate(convs):
            finals = {ci < 3 or ci == 6}                       # DispRefiner.forward
            if ci < 5:
                finals.add(ci == 4)                            # the loop in front of the fused tail
            for final in sorted(finals):
                yield f"lvl{d}.conv{ci}", conv, (b, h, w, widths[ci]), final


def front_rows(model, H, W, b):
    """[level depth, _front_by_size, wants_prenormalized] per level on its encoder map."""
    rows = []
    for lvl in model.d_estimator.levels:
        d = lvl.lvl_depth
        shape = (b, -(-H // 2 ** d), -(-W // 2 ** d), ENCODER_CHANNELS[d - 1])
        rows.append([d, bool(lvl._front_by_size(*shape)), bool(lvl.wants_prenormalized(*shape))])
    return rows


class ShapeOnly:
    """What ``forward`` looks at before it launches."""
    is_cuda = True
    device = torch.device("cpu")

    def __init__(self, shape):
        self.shape = tuple(shape)


def record_forward(conv, shape, final, layout_of):
    """The row ``forward`` produces for this call, through recorders in place of the launch wrappers.  ``layout_of(tensor)`` =
    (layout key, cin_pad) of a packed tensor."""
    seen = []

    def recorder(name):
        def rec(x, wts, bias, cout, *args, **kw):
            has_pad = name not in ("conv3x3_lat", "conv3x3_lat_f16")
            cfg = kw.get("config")
            seen.append([name, layout_of(wts)[0], int(args[0]) if has_pad else None,
                         None if cfg is None else [int(v) for v in cfg], kw.get("kernel"), kw.get("stagger_us"),
                         bool(cfg is not None and cfg[2] > 1)])
        return rec
    names = [n for n in dir(nops) if n.startswith("conv3x3_") and callable(getattr(nops, n))]
    old = {n: getattr(nops, n) for n in names}
    try:
        for n in names:
            setattr(nops, n, recorder(n))
        conv.forward(ShapeOnly(shape), slope=0.1, final=final)
    finally:
        for n, f in old.items():
            setattr(nops, n, f)
    assert len(seen) == 1, seen
    return seen[0]


def snapshot(row_of):
    """The whole snapshot, ``row_of(conv, shape, final)`` giving a row's recorded part."""
    out = {"columns": ["layer", "b", "h", "w", "cin", "final", "wrapper", "layout", "cout_pad", "lat_config", "wino6_kernel",
                       "stagger_us", "partial"],
           "front_columns": ["level", "front_by_size", "wants_prenormalized"], "rows": {}, "fronts": {}}
    for name, (H, W, L, b, stack) in WORKLOADS.items():
        model = model_for(L)
        out["fronts"][name] = front_rows(model, H, W, b)
        for arith in ARITHS:
            with N.conv_arithmetic(arith):
                out["rows"].setdefault(arith, {})[name] = [
                    [tag, *shape, int(final)] + row_of(conv, shape, final) for tag, conv, shape, final in
                    layer_calls(model, H, W, b, stack)]
    return out


def _load():
    with open(SNAPSHOT) as fh:
        return json.load(fh)


def _plan_row(conv, shape, final):
    p = conv.plan(*shape, final)
    is_lat = p.kernel in ("lat", "lat_f16")
    cout_pad = None if is_lat else -(-conv.out_channels // (64 if p.layout in ("wino6", "winof16") else 32)) * (
        64 if p.layout in ("wino6", "winof16") else 32)
    return [N._CONV_LAUNCH[p.kernel][0], p.layout, cout_pad, None if p.lat_config is None else list(p.lat_config),
            p.wino6_kernel, p.stagger_us, bool(is_lat and p.lat_config[2] > 1)]


def test_plan_reproduces_the_recorded_dispatch():
    want = _load()
    got = snapshot(_plan_row)
    assert got["fronts"] == want["fronts"]
    for arith in ARITHS:
        for name in WORKLOADS:
            assert len(got["rows"][arith][name]) == len(want["rows"][arith][name])
            for g, w in zip(got["rows"][arith][name], want["rows"][arith][name]):
                assert g == w, (arith, name, g, w)


def test_forward_launches_what_plan_says():
    """``forward`` through recorders (how the snapshot was taken) gives the recorded rows too, ``cout_pad`` from the packed
    weights themselves."""
    want = _load()
    layouts = {}
    old = N._Conv3x3SameTF.packed

    def packed(conv, layout, cin_pad=None):
        res = old(conv, layout, cin_pad)
        layouts[id(res[0] if isinstance(res, tuple) else res)] = (layout, cin_pad)
        return res
    N._Conv3x3SameTF.packed = packed
    try:
        got = snapshot(lambda conv, shape, final: record_forward(conv, shape, final, lambda t: layouts[id(t)]))
    finally:
        N._Conv3x3SameTF.packed = old
    assert got == want


def test_prepack_builds_every_layout_the_dispatch_names():
    """For every recorded row, the layout ``plan`` names satisfies the layer's static condition -- the condition ``prepack``
    builds from -- at the row's channel padding, and ``prepack`` visits that (layer, padding) pair."""
    for name, (H, W, L, b, stack) in WORKLOADS.items():
        model = model_for(L)
        built = {(id(conv), cin_pad): set(layouts) for conv, cin_pad, layouts in model.prepack_jobs()}
        for arith in ARITHS:
            with N.conv_arithmetic(arith):
                for tag, conv, shape, final in layer_calls(model, H, W, b, stack):
                    p = conv.plan(*shape, final)
                    assert conv.can_use(p.layout, shape[3]), (name, arith, tag, p)
                    assert p.layout in built[(id(conv), shape[3])], (name, arith, tag, p)
