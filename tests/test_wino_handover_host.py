"""Which layers of the 384x1280 six-level pyramid at batch 1 write and which read pixel maxima (``_Conv3x3SameTF.plan``,
``network.wino_handover``), and what ``forward`` hands its launch wrapper -- on the CPU: plans are pure, and the wrappers are
replaced by recorders over shape-only stand-ins.

Levels 1 and 2 hand maxima on; level 3 (30 tiles) does not: ``network._WINO_HANDOVER_MIN_TILES`` keeps the hand-over to maps of at
least 100 tiles, because tests/test_level_dispatch.py holds ``forward`` on maps of up to 30 tiles to launch rows recorded before the
hand-over existed (49 of its 53 cases run chained fp16 Winograd layers).  With the threshold lifted the plans are the full table
-- levels 1-3: conv1 writes, conv2-conv4 read and write, conv5 reads -- which the second test checks."""
import pytest
import torch

from m4depth_amd import network as N
from m4depth_amd import network_ops as nops
from m4depth_amd.synthetic import REFINER_CHANNELS

H, W, LEVELS, B = 384, 1280, 6, 1


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    m = N.M4Depth(nbre_levels=LEVELS)
    m.encoder.set_sequence_batch(B)
    return m


def _refiner_chain(lvl):
    """[(conv, input shape, final)] of the five layers in front of the fused tail, as ``DepthEstimatorLevel.forward`` calls them."""
    d = lvl.lvl_depth
    h, w = -(-H // 2 ** d), -(-W // 2 ** d)
    convs = (list(lvl.disp_refiner.prep_conv_layers) + list(lvl.disp_refiner.est_d_conv_layers))[:5]
    widths = [(lvl.f_in + 7) // 8 * 8] + list(REFINER_CHANNELS[:4])
    return [(conv, (B, h, w, widths[ci]), ci == 4) for ci, conv in enumerate(convs)]


def _walk(lvl):
    """[(reads, writes)] per layer, the maxima following the chain."""
    rows, maxima = [], False
    for conv, shape, final in _refiner_chain(lvl):
        p = conv.plan(*shape, final, maxima)
        rows.append((p.reads_maxima, p.writes_maxima))
        maxima = p.writes_maxima
    return rows


@pytest.mark.parametrize("min_tiles,levels", [(None, (1, 2)), (1, (1, 2, 3))])
def test_which_layers_write_and_read_maxima(model, monkeypatch, min_tiles, levels):
    monkeypatch.setattr(N, "wino_handover", True)
    if min_tiles is not None:
        monkeypatch.setattr(N, "_WINO_HANDOVER_MIN_TILES", min_tiles)
    with N.conv_arithmetic("f16x2"):
        for lvl in model.d_estimator.levels:
            rows = _walk(lvl)
            if lvl.lvl_depth in levels:
                assert rows == [(False, True)] + [(True, True)] * 3 + [(True, False)], (lvl.lvl_depth, rows)
                assert all(conv.plan(*shape, final).layout == "winof16" for conv, shape, final in _refiner_chain(lvl))
            else:
                assert rows == [(False, False)] * 5, (lvl.lvl_depth, rows)
        enc = model.encoder
        cin = [3] + list(enc.out_sizes[:-1])
        for i, (s1, s2) in enumerate(zip(enc.conv_layers_s1, enc.conv_layers_s2)):
            h, w = -(-H // 2 ** i), -(-W // 2 ** i)
            for conv, c in ((s1, cin[i]), (s2, enc.out_sizes[i])):
                p = conv.plan(2 * B, h, w, c, True)           # every encoder call is final and reads a plain tensor
                assert not p.reads_maxima and not p.writes_maxima, (i, p)


def test_switch_off_and_other_arithmetics_hand_nothing_on(model, monkeypatch):
    lvl = model.d_estimator.levels[0]
    monkeypatch.setattr(N, "wino_handover", False)
    with N.conv_arithmetic("f16x2"):
        assert _walk(lvl) == [(False, False)] * 5
    monkeypatch.setattr(N, "wino_handover", True)
    for arith in ("bf16x3", "f32"):
        with N.conv_arithmetic(arith):
            assert _walk(lvl) == [(False, False)] * 5, arith


class ShapeOnly:
    """What ``forward`` looks at before it launches."""
    is_cuda = True
    device = torch.device("cpu")

    def __init__(self, shape):
        self.shape = tuple(shape)

    def dense(self):
        return self


def _forward_through_recorders(conv, x, final):
    """(first argument, keyword arguments) of the one launch wrapper ``forward`` calls."""
    seen = []
    names = [n for n in dir(nops) if n.startswith("conv3x3_") and callable(getattr(nops, n))]
    old = {n: getattr(nops, n) for n in names}
    try:
        for n in names:
            setattr(nops, n, lambda x, *args, _n=n, **kw: seen.append((_n, x, kw)))
        conv.forward(x, slope=0.1, final=final)
    finally:
        for n, f in old.items():
            setattr(nops, n, f)
    assert len(seen) == 1, seen
    return seen[0]


def test_forward_hands_maxima_only_to_the_layer_that_reads_them(model, monkeypatch):
    """A padded input and a ``PartialAct`` never carry maxima into a launch; a layer on another kernel gets the plain tensor."""
    monkeypatch.setattr(N, "wino_handover", True)
    with N.conv_arithmetic("f16x2"):
        chain1 = _refiner_chain(model.d_estimator.levels[0])
        conv2, shape2, _ = chain1[1]
        act = nops.ActMaxima(ShapeOnly(shape2), ShapeOnly(shape2[:3] + (2,)))
        name, x, kw = _forward_through_recorders(conv2, act, False)
        assert name == "conv3x3_wino6_bias_act" and x is act and kw["want_maxima"] is True and kw["arith"] == "f16x2"
        name, x, kw = _forward_through_recorders(conv2, ShapeOnly(shape2), True)                   # a plain tensor, a last layer
        assert isinstance(x, ShapeOnly) and kw["want_maxima"] is False
        # level 2's conv1 reads the refiner input padded from 122 to 128 channels: maxima beside such a tensor are not its input's
        conv1, shape1, _ = _refiner_chain(model.d_estimator.levels[1])[0]
        assert shape1[3] != conv1.weight.shape[1]
        assert not conv1.plan(*shape1, False, True).reads_maxima
        padded = nops.ActMaxima(ShapeOnly(shape1), ShapeOnly(shape1[:3] + (2,)))
        name, x, kw = _forward_through_recorders(conv1, padded, False)
        assert x is padded.tensor and kw["want_maxima"] is True
        # a layer on the latency-first kernel takes the tensor itself
        conv4, shape4, _ = _refiner_chain(model.d_estimator.levels[3])[1]
        lone = nops.ActMaxima(ShapeOnly(shape4), ShapeOnly(shape4[:3] + (2,)))
        name, x, kw = _forward_through_recorders(conv4, lone, False)
        assert name == "conv3x3_lat_f16" and x is lone.tensor and "want_maxima" not in kw
        # a PartialAct is not an ActMaxima: the plan is made without maxima
        part = nops.PartialAct(ShapeOnly((2,) + shape4), None, 0.1)
        name, x, kw = _forward_through_recorders(conv4, part, False)
        assert x is part and not conv4.plan(*shape4, False).reads_maxima


def test_act_maxima_is_the_tensor_for_every_other_consumer():
    t, m = torch.zeros(1, 4, 4, 64), torch.zeros(1, 4, 4, 1, dtype=torch.int32)
    act = nops.ActMaxima(t, m)
    assert act.dense() is t and act.shape == t.shape and act.device == t.device and not act.is_cuda
