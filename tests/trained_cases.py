"""The trained encoder of the reference's legacy model as a test case: all 24 tensors of its ``features`` bundle
(tests/golden/tf_legacy: the head file and the byte ranges beside it, put back end to end and read through
``tf_checkpoint.CheckpointReader`` with TensorFlow's own checksums), and the activations these weights produce.

Unlike He-initialised weights on Gaussian inputs -- what every other convolution test draws -- the trained kernels have dead
output channels (|w| < 1e-4 beside channels of 0.3: per-channel exponents up to 32 in the fp16 two-term packers, ``lo`` terms
in fp16's subnormal range), dead input channels, and activations that are post-leaky-ReLU, not zero-mean, constant in the
dead channels and 2^15 and more apart between the channels of one map.  tests/test_trained_cases.py pins those facts;
tests/test_gpu_trained.py runs the kernels on them."""
import glob
import os
import tempfile

import numpy as np

F = np.float32
LEGACY = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tf_legacy")
HEAD = os.path.join(LEGACY, "features.data-00000-of-00001")
DATA_BYTES = 4088640                                    # the size of the data file TensorFlow wrote (test_tf_checkpoint.py)
ENCODER_CHANNELS = [16, 32, 64, 96, 128, 192]
LAYERS = [(l, c) for l in range(1, 7) for c in (1, 2)]  # (level, conv): conv2d_1 = stride 1, conv2d_2 = stride 2
DEAD = 1e-4                                             # a channel whose largest |weight| is below this is dead
ACTIVATION_CASE = (384, 640, 1)                         # height, width, seed of synthetic.make_sequence (see trained_activations)

_cache = {}


def layer_shape(level, conv):
    """HWIO shape of FeaturePyramid's layer (m4depth_amd.network.FeaturePyramid: conv_layers_s1 / conv_layers_s2)."""
    cout = ENCODER_CHANNELS[level - 1]
    cin = cout if conv == 2 else ([3] + ENCODER_CHANNELS)[level - 1]
    return (3, 3, cin, cout)


def data_parts():
    """[(offset, path)] of the committed byte ranges of the features data file, the head first."""
    parts = [(0, HEAD)]
    for p in sorted(glob.glob(HEAD + ".at-*")):
        parts.append((int(p.rsplit("-", 1)[1]), p))
    return sorted(parts)


def read_bundle(parts=None):
    """{tensor name: array} of all 24 tensors, every one checked against the masked crc32c TensorFlow stored for it.
    ``parts``: [(offset, path)] in place of the committed byte ranges."""
    from m4depth_amd import tf_checkpoint as TC
    parts = data_parts() if parts is None else parts
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "features.data-%05d-of-%05d")
        pos = 0
        with open(path % (0, 1), "wb") as out:
            for off, p in parts:
                if off != pos:
                    raise ValueError(f"{p}: starts at byte {off}, the ranges before it end at {pos}")
                with open(p, "rb") as fh:
                    raw = fh.read()
                out.write(raw)
                pos += len(raw)
        if pos != DATA_BYTES:
            raise ValueError(f"the byte ranges end at {pos}, the data file TensorFlow wrote at {DATA_BYTES}")
        reader = TC.CheckpointReader(os.path.join(LEGACY, "features"), verify=True, data_path=path)
        return {k: reader.tensor(k) for k in reader.keys()}


def trained_encoder_weights():
    """{(level, conv, "kernel" | "bias"): float32 array}: level 1..6, conv 1 (stride 1) and 2 (stride 2).  Read once."""
    if "weights" not in _cache:
        t = read_bundle()
        assert len(t) == 24
        _cache["weights"] = {(l, c, p): t[f"feature_pyramid/layer_{l}/conv2d_{c}/{p}"] for l, c in LAYERS for p in ("kernel", "bias")}
    return {k: v.copy() for k, v in _cache["weights"].items()}


def encoder_weight_dict(levels=6):
    """The trained encoder under the names of synthetic.init_weights (``enc.s1.<i>``, ``enc.s2.<i>``), DINL scale 1 and bias 0
    (the legacy bundle holds no DINL variables)."""
    tw = trained_encoder_weights()
    W = {}
    for i in range(levels):
        for c, nm in ((1, "s1"), (2, "s2")):
            W[f"enc.{nm}.{i}.kernel"] = tw[i + 1, c, "kernel"]
            W[f"enc.{nm}.{i}.bias"] = tw[i + 1, c, "bias"]
    W["enc.dn.0.scale"] = np.ones([16], F)
    W["enc.dn.0.bias"] = np.zeros([16], F)
    return W


def model_weights(levels=6, seed=42):
    """synthetic.init_weights with its encoder replaced by the trained one (the legacy model has no refiner of this shape)."""
    from m4depth_amd import synthetic
    W = synthetic.init_weights(levels, seed=seed)
    W.update(encoder_weight_dict(levels))
    return W


def he_init_like(kernel, seed=0):
    """The kernel every other convolution test draws, in the shape of ``kernel``."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(kernel.shape) * np.sqrt(2.0 / (9 * kernel.shape[2]))).astype(F)


def pyramid_with_inputs(image, W, levels=6):
    """oracle.feature_pyramid's loop (the same calls in the same order) keeping every layer's input:
    ({(level, conv): input map}, [level outputs])."""
    from oracle import m4depth_oracle as O
    fm, inputs, outs = O._f32(image), {}, []
    for i in range(levels):
        inputs[i + 1, 1] = fm
        t = O.conv2d_same(fm, W[f"enc.s1.{i}.kernel"], W[f"enc.s1.{i}.bias"], 1)
        if i == 0:
            t = O.domain_normalization(t, W["enc.dn.0.scale"], W["enc.dn.0.bias"])
        t = O.leaky_relu(t, 0.1)
        inputs[i + 1, 2] = t
        fm = O.leaky_relu(O.conv2d_same(t, W[f"enc.s2.{i}.kernel"], W[f"enc.s2.{i}.bias"], 2), 0.1)
        outs.append(fm)
    return inputs, outs


def trained_activations():
    """{(level, conv): float32 [1,h,w,cin]}: the input of each of the 12 trained layers when the float32 oracle encodes frame 0
    of synthetic.make_sequence(1, 1, 384, 640, seed) -- 384x640x3 down to 12x20x192.  Computed once per session; read-only.
    The first seed tried, 20261, spread the channel maxima of level 6's input over 2^14.95, short of the 2^15
    test_trained_cases.py asks for (level 5: 2^17.9); seed 1, the second tried, gives 2^15.1 and 2^18.1 (seeds 2 to 6:
    2^15.0 to 2^15.4 -- the spread is set by the dead channels' biases, the frame only moves the largest channel)."""
    if "acts" not in _cache:
        from m4depth_amd import synthetic
        h, w, seed = ACTIVATION_CASE
        samples, _ = synthetic.make_sequence(1, 1, h, w, seed=seed)
        inputs, outs = pyramid_with_inputs(samples[0]["RGB_im"], encoder_weight_dict())
        for v in inputs.values():
            v.setflags(write=False)
        _cache["acts"], _cache["pyramid"] = inputs, outs
    return _cache["acts"]


def two_term_split(kernel):
    """The fp16 two-term split of a float32 HWIO kernel, restated: per output channel t = 15 - (exponent of the channel's
    largest |w|), hi = fp16(2^t w), lo = fp16(2^t w - hi).  -> (t [Cout], |(hi + lo) 2^-t - w| [3,3,Cin,Cout], in float64)."""
    w = np.asarray(kernel, np.float64)
    amax = np.abs(w).max(axis=(0, 1, 2))
    t = np.where(amax > 0, 15 - np.frexp(amax)[1], 0)
    s = w * np.ldexp(1.0, t)
    hi = s.astype(np.float16).astype(np.float64)
    lo = (s - hi).astype(np.float16).astype(np.float64)
    return t, np.abs((hi + lo) * np.ldexp(1.0, -t) - w)


def kernel_facts(kernel):
    """What the table of test_trained_cases.py lists for one kernel."""
    w = np.abs(np.asarray(kernel, np.float64))
    t, err = two_term_split(kernel)
    over = err > 2.0 ** -22 * w
    return dict(t_min=int(t.min()), t_max=int(t.max()), share=float(over.mean()),
                worst=float((err[over] / w[over]).max()) if over.any() else 0.0,
                dead_out=int((w.max(axis=(0, 1, 2)) < DEAD).sum()), dead_in=int((w.max(axis=(0, 1, 3)) < DEAD).sum()),
                smallest=float(w[w > 0].min()))
