"""Prediction export (m4d_depth_export, network_ops.depth_export, export.PredictionWriter, main.py --save_dir) against a numpy
restatement of the formulas in include/m4depth_hip.h.  All arithmetic is + - * / rint and one float16 conversion on float32,
one rounding per operation: the comparison is bit for bit on every output."""
import functools
import os

import numpy as np
import pytest
import torch

from helpers import F, npy, make_fake_dataset

pytestmark = pytest.mark.gpu

NEAR, FAR, ERR_MAX = F(1.0), F(80.0), F(0.5)


# ---- the restatement -----------------------------------------------------------------------------------------------------
def valid(d):
    return np.isfinite(d) & (d > 0)


def encode_depth16(d, fmt):
    """float32 depth -> the uint16 codes of 'kitti16' / 'midair16'."""
    d = np.asarray(d, F)
    with np.errstate(all="ignore"):
        if fmt == "kitti16":
            v = np.minimum(np.maximum(np.rint(d * F(256.0)), F(1.0)), F(65535.0))
            return np.where(valid(d), v, F(0.0)).astype(np.uint16)
        bits = (F(512.0) / d).astype(np.float16).view(np.uint16)            # round to nearest even; overflow -> +Inf = 0x7C00
    return np.where(valid(d), bits, np.uint16(0x7C00)).astype(np.uint16)


def decode_depth16(bits, fmt):
    """The loaders' arithmetic: value / 256, 512 / float16(bits)."""
    if fmt == "kitti16":
        return bits.astype(F) / F(256.0)
    with np.errstate(divide="ignore"):
        return F(512.0) / bits.view(np.float16).astype(F)


def depth_index(d, near=NEAR, far=FAR):
    d = np.asarray(d, F)
    with np.errstate(all="ignore"):
        t = (F(1.0) / d - F(1.0) / far) / (F(1.0) / near - F(1.0) / far)
        i = np.rint(np.minimum(np.maximum(t, F(0.0)), F(1.0)) * F(255.0))
    return np.where(valid(d), i, F(256.0)).astype(np.int64)


def error_index(est, gt, err_max=ERR_MAX):
    est, gt = np.asarray(est, F), np.asarray(gt, F)
    with np.errstate(all="ignore"):
        r = (np.abs(est - gt) / gt) / err_max
        i = np.rint(np.minimum(r, F(1.0)) * F(255.0))
    return np.where(valid(est) & valid(gt), i, F(256.0)).astype(np.int64)


def rgb_bytes(v):
    v = np.asarray(v, F)
    v = np.where(np.isnan(v), F(0.0), v)
    return np.rint(np.minimum(np.maximum(v, F(0.0)), F(1.0)) * F(255.0)).astype(np.uint8)


def render_panels(kinds, est, gt, rgb, lut):
    """[b, len(kinds)*h, w, 3] uint8; est, gt [b,h,w], rgb [b,h,w,3]."""
    one = {"rgb": lambda: rgb_bytes(rgb), "est": lambda: lut[depth_index(est)], "gt": lambda: lut[depth_index(gt)],
           "err": lambda: lut[error_index(est, gt)]}
    return np.concatenate([one[k]() for k in kinds], axis=1)


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def half_tie_depths():
    """Depths d for which float32 512 / d lies exactly between two neighbouring float16 values (even and odd lower
    neighbours, normal and subnormal).  The quotients sit just above a power of two, where consecutive float32 depths step
    the quotient by half an ulp, so every one of them is the quotient of some depth."""
    out = []
    for lower in (0x3C00, 0x3C01, 0x4000, 0x4001, 0x5402, 0x2C03, 0x0004):
        pair = np.array([lower, lower + 1], np.uint16).view(np.float16).astype(F)
        tie = F((pair[0] + pair[1]) / F(2.0))                                   # exact: 12 significant bits
        d = F(512.0) / tie
        for _ in range(8):                                                      # a few float32 neighbours of 512 / tie
            if F(512.0) / d == tie:
                out.append(d)
                break
            d = np.nextafter(d, F(0.0) if F(512.0) / d < tie else F(np.inf))
    assert len(out) == 7, out
    return out


def planted_depths():
    ties256 = [F((k + 0.5) / 256.0) for k in (2, 3, 512, 513, 20480, 20481)]    # rintf ties of kitti16: exact in float32
    return np.array([0.0, -1.0, np.nan, np.inf, 1e-4, 3e38, NEAR, FAR] + ties256 + half_tie_depths(), F)


@functools.lru_cache(maxsize=None)
def case(b, h, w):
    """Host inputs of one shape, made once: est, gt [b,h,w], rgb [b,h,w,3]."""
    rng = np.random.default_rng(b * 1000003 + h * 1009 + w)
    n = b * h * w
    est = np.exp(rng.uniform(np.log(0.05), np.log(2000.0), n)).astype(F)
    planted = planted_depths()
    where = rng.permutation(n)[:len(planted)]
    est[where] = planted[:len(where)]
    if n >= 4 * len(planted):                                                   # the last pixels of a row: the guarded tail
        est.reshape(b * h, w)[-1, -min(w, 3):] = planted[2:2 + min(w, 3)]
    u = rng.random(n)
    gt = np.exp(rng.uniform(np.log(0.05), np.log(2000.0), n)).astype(F)
    gt = np.where(u < 1 / 3, F(0.0), np.where(u < 0.5, est, gt)).astype(F)      # KITTI's sparse maps; gt == est
    gt[rng.permutation(n)[:3]] = np.array([np.nan, -2.0, np.inf], F)[:min(n, 3)]
    rgb = rng.uniform(-0.2, 1.2, n * 3).astype(F)
    rgb[rng.permutation(n * 3)[:4]] = np.array([np.nan, -5.0, 7.0, 0.5], F)[:min(n * 3, 4)]
    for a in (est, gt, rgb):
        a.setflags(write=False)
    return est.reshape(b, h, w), gt.reshape(b, h, w), rgb.reshape(b, h, w, 3)


def on_device(a, dev, c, strided):
    """[b,h,w(,c)] host array -> [b,h,w,c] device tensor; ``strided``: the [:, :h] view of a taller buffer."""
    b, h, w = a.shape[:3]
    t = torch.from_numpy(np.array(a, F).reshape(b, h, w, c)).to(dev)                  # a copy: the cached case stays read-only
    if not strided:
        return t
    tall = torch.full((b, h + 3, w, c), float("nan"), dtype=torch.float32, device=dev)
    tall[:, :h] = t
    return tall[:, :h]


GUARD = 16                                                                      # elements before and after every output


def guarded(shape, dtype, dev):
    n = int(np.prod(shape))
    pattern = 0x5A if dtype == torch.uint8 else 0x5A5A
    flat = torch.full((n + 2 * GUARD,), pattern, dtype=dtype, device=dev)
    return flat, flat[GUARD:GUARD + n].view(shape), pattern


def assert_guards(flat, pattern, what):
    host = npy(flat)
    assert (host[:GUARD] == pattern).all() and (host[-GUARD:] == pattern).all(), f"{what}: guard elements overwritten"


def lut_pair(dev):
    from m4depth_amd.export import default_lut
    lut = default_lut()
    return lut, torch.from_numpy(lut).to(dev)


SHAPES = [(1, 1, 1), (3, 5, 7), (2, 37, 53), (1, 64, 130), (2, 16, 128)]
STRIDED = {(3, 5, 7), (2, 37, 53)}                                              # (2,16,128): dense and fully aligned
PANEL_LISTS = [(), ("est",), ("rgb", "est", "gt", "err"), ("err", "rgb")]


# ---- 1. the kernel against the restatement --------------------------------------------------------------------------------
@pytest.mark.parametrize("kinds", PANEL_LISTS, ids=lambda k: "+".join(k) or "none")
@pytest.mark.parametrize("fmt", ["kitti16", "midair16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_export_matches_the_restatement_bit_for_bit(dev, shape, fmt, kinds):
    from m4depth_amd import network_ops as nops
    b, h, w = shape
    est, gt, rgb = case(*shape)
    strided = shape in STRIDED
    lut, lut_d = lut_pair(dev)
    est_d, gt_d, rgb_d = on_device(est, dev, 1, strided), on_device(gt, dev, 1, strided), on_device(rgb, dev, 3, strided)
    assert est_d.is_contiguous() == (not strided)
    d_flat, d_out, d_pat = guarded((b, h, w), torch.int16, dev)
    p_flat, p_out, p_pat = guarded((b, max(len(kinds), 1) * h, w, 3), torch.uint8, dev)
    got_d, got_p = nops.depth_export(est_d, fmt, kinds, gt=gt_d, rgb=rgb_d, lut=lut_d, near=float(NEAR), far=float(FAR),
                                     err_max=float(ERR_MAX), depth16=d_out, panels_out=p_out if kinds else None)
    torch.cuda.synchronize()
    want_d = encode_depth16(est, fmt)
    bad = np.argwhere(npy(got_d).view(np.uint16) != want_d)
    assert len(bad) == 0, f"{fmt}: {len(bad)} codes differ; first at {bad[0]}: est {est[tuple(bad[0])]!r}"
    assert_guards(d_flat, d_pat, "depth16")
    if kinds:
        want_p = render_panels(kinds, est, gt, rgb, lut)
        bad = np.argwhere(npy(got_p) != want_p)
        assert len(bad) == 0, f"panels {kinds}: {len(bad)} bytes differ; first at {bad[0]}"
    else:
        assert got_p is None
    assert_guards(p_flat, p_pat, "panels")


def test_export_without_a_format_writes_panels_only(dev):
    from m4depth_amd import network_ops as nops
    est, gt, rgb = case(3, 5, 7)
    lut, lut_d = lut_pair(dev)
    got_d, got_p = nops.depth_export(on_device(est, dev, 1, False), None, ("gt", "est"), gt=on_device(gt, dev, 1, False),
                                     lut=lut_d, near=float(NEAR), far=float(FAR))
    assert got_d is None and np.array_equal(npy(got_p), render_panels(("gt", "est"), est, gt, rgb, lut))
    with pytest.raises(ValueError, match="need gt"):
        nops.depth_export(on_device(est, dev, 1, False), "kitti16", ("err",), lut=lut_d)


# ---- 2. round trip through the project's decoders ---------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,kind", [("kitti16", 1), ("midair16", 0)])
def test_round_trip_through_the_dataset_decoders(dev, fmt, kind):
    """export -> m4d_decode_depth_resize at equal size.  The bounds follow from the formats: kitti16 rounds d * 256 to an
    integer (half a code = 1/512 m; below 1/512 m the code is clamped to 1, which is why the inputs start at 0.05 m);
    midair16 keeps 11 significant bits of 512 / d (2^-11 = 4.883e-4, plus two float32 roundings) while the quotient is a
    normal, finite float16, i.e. 0.0079 <= d <= 8e6."""
    from m4depth_amd import network_ops as nops
    from m4depth_amd._lib import lib, dptr, stream_ptr, check
    b, h, w = 2, 37, 53
    rng = np.random.default_rng(5)
    est = np.exp(rng.uniform(np.log(0.05), np.log(2000.0), (b, h, w))).astype(F)
    est.reshape(-1)[rng.permutation(est.size)[:8]] = np.array([0.0, -1.0, np.nan, np.inf, -np.inf, NEAR, FAR, 255.998], F)
    codes, _ = nops.depth_export(on_device(est, dev, 1, False), fmt)
    out = torch.empty((b, h, w, 1), dtype=torch.float32, device=dev)
    check(lib.m4d_decode_depth_resize(dptr(codes, "codes", torch.int16), kind, b, h, w, h, w, None, None, dptr(out),
                                      stream_ptr()), "m4d_decode_depth_resize")
    dec = npy(out)[..., 0]
    ok = valid(est)
    assert (dec[~ok] == 0).all()
    if fmt == "kitti16":
        sel = ok & (est <= F(65535.0 / 256.0))
        err = np.abs(dec[sel].astype(np.float64) - est[sel])
        print(f"kitti16 round trip: max |error| {err.max():.4e} m over {sel.sum()} pixels")
        assert sel.sum() > 1000 and err.max() <= 1.0 / 512.0
    else:
        sel = ok & (est >= F(0.0079)) & (est <= F(8e6))
        rel = np.abs(dec[sel].astype(np.float64) - est[sel]) / est[sel]
        print(f"midair16 round trip: max relative error {rel.max():.4e} over {sel.sum()} pixels")
        assert sel.sum() > 1000 and rel.max() <= 4.9e-4


# ---- 3. inside a captured graph ---------------------------------------------------------------------------------------------
def test_export_replays_from_a_captured_graph(dev):
    from m4depth_amd import network_ops as nops
    shape, kinds = (2, 37, 53), ("rgb", "est", "gt", "err")
    b, h, w = shape
    est, gt, rgb = case(*shape)
    lut, lut_d = lut_pair(dev)
    est_d, gt_d, rgb_d = on_device(est, dev, 1, True), on_device(gt, dev, 1, True), on_device(rgb, dev, 3, False)
    d_out = torch.zeros((b, h, w), dtype=torch.int16, device=dev)
    p_out = torch.zeros((b, len(kinds) * h, w, 3), dtype=torch.uint8, device=dev)
    kw = dict(gt=gt_d, rgb=rgb_d, lut=lut_d, near=float(NEAR), far=float(FAR), err_max=float(ERR_MAX))
    eager_d, eager_p = nops.depth_export(est_d, "midair16", kinds, **kw)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        nops.depth_export(est_d, "midair16", kinds, depth16=d_out, panels_out=p_out, **kw)
    d_out.zero_()
    p_out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(d_out, eager_d) and torch.equal(p_out, eager_p)
    assert np.array_equal(npy(d_out).view(np.uint16), encode_depth16(est, "midair16"))


# ---- 4. the writer --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["kitti16", "midair16"])
def test_prediction_writer_files_equal_the_export(dev, tmp_path, fmt):
    from PIL import Image
    from m4depth_amd import network_ops as nops
    from m4depth_amd.export import PredictionWriter, FrameNamer, read_depth_png
    b, h, w, steps, kinds = 3, 24, 40, 7, ("rgb", "est", "gt", "err")
    rng = np.random.default_rng(11)
    lut, lut_d = lut_pair(dev)
    namer, want = FrameNamer(b), {}
    out = str(tmp_path / "out")
    with PredictionWriter(out, fmt, kinds, near=float(NEAR), far=float(FAR), err_max=float(ERR_MAX), slots=2) as writer:
        for step in range(steps):
            est = torch.from_numpy(np.exp(rng.uniform(np.log(0.05), np.log(2000.0), (b, h, w, 1))).astype(F)).to(dev)
            gt = torch.from_numpy(np.where(rng.random((b, h, w, 1)) < 0.3, 0.0, rng.uniform(1, 90, (b, h, w, 1))).astype(F)).to(dev)
            rgb = torch.from_numpy(rng.random((b, h, w, 3)).astype(F)).to(dev)
            names = namer([step == 0, step in (0, 3), step in (0, 5)])
            writer.submit(est, names, gt=gt, rgb=rgb)
            d16, pan = nops.depth_export(est, fmt, kinds, gt=gt, rgb=rgb, lut=lut_d, near=float(NEAR), far=float(FAR),
                                         err_max=float(ERR_MAX))
            for s, name in enumerate(names):
                want[name] = (npy(d16[s]).view(np.uint16), npy(pan[s]))
    assert writer.frames == 21 and len(want) == 21
    found = sorted(os.path.relpath(os.path.join(r, f), out) for r, _, fs in os.walk(out) for f in fs)
    assert found == sorted(n + s for n in want for s in ("_depth.png", "_panels.png")) and len(found) == 42
    assert "s01_t0001/000003_depth.png" in found and "s00_t0000/000006_panels.png" in found
    for name, (d16, pan) in want.items():
        with Image.open(os.path.join(out, name + "_depth.png")) as im:
            assert im.mode == "I;16" and np.array_equal(np.asarray(im, np.uint16), d16), name
        with Image.open(os.path.join(out, name + "_panels.png")) as im:
            assert im.mode == "RGB" and np.array_equal(np.asarray(im), pan), name
        assert np.array_equal(read_depth_png(os.path.join(out, name + "_depth.png"), fmt), decode_depth16(d16, fmt))


def test_prediction_writer_errors_and_dry_runs(dev, tmp_path):
    from m4depth_amd.export import PredictionWriter, FrameNamer
    b, h, w = 3, 24, 40
    est = torch.rand((b, h, w, 1), device=dev) * 50 + 1
    blocked = tmp_path / "taken"
    blocked.write_text("a file where the output directory should be")
    writer = PredictionWriter(str(blocked), "kitti16", slots=2)
    namer = FrameNamer(b)
    for _ in range(3):
        writer.submit(est, namer([False] * b))                                 # the failing workers still free their slots
    with pytest.raises(OSError):
        writer.close()
    dry = tmp_path / "dry"
    with PredictionWriter(str(dry), "midair16", ("est",), slots=2, encode=False) as writer:
        namer = FrameNamer(b)
        for _ in range(5):
            writer.submit(est, namer([False] * b))
    assert writer.frames == 15 and not dry.exists()


# ---- 5. the driver --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [[], ["--stream"], ["--stream", "--graph"]], ids=["frames", "stream", "stream-graph"])
def test_driver_saves_what_it_predicts(dev, tmp_path, mode):
    import json
    from PIL import Image
    from m4depth_amd import main as MAIN
    from m4depth_amd.export import read_depth_png
    db, rec = make_fake_dataset(str(tmp_path), "midair", n_traj=2, n_frames=8, size=(64, 64))
    cfg = os.path.join(str(tmp_path), "datasets_location.json")
    with open(cfg, "w") as fh:
        json.dump({"midair": "./db"}, fh)
    ck, ck2, out = (os.path.join(str(tmp_path), d) for d in ("ckpt", "ckpt2", "saved"))
    common = ["--mode", "predict", "--dataset", "midair", "--db_path_config", cfg, "--records_path", rec, "--arch_depth", "2",
              "--height", "64", "--width", "64"] + mode
    assert MAIN.main(common + ["--ckpt_dir", ck]) == 0
    preds = np.load(os.path.join(ck, "predictions.npy"))
    assert preds.shape == (16, 64, 64, 1)
    assert MAIN.main(common + ["--ckpt_dir", ck2, "--save_dir", out, "--save_format", "midair16",
                               "--save_panels", "rgb,est,gt,err"]) == 0
    assert not os.path.exists(os.path.join(ck2, "predictions.npy"))
    assert sorted(os.listdir(out)) == ["s00_t0000", "s00_t0001"]
    files = sorted(os.path.join(d, f) for d in sorted(os.listdir(out)) for f in os.listdir(os.path.join(out, d)))
    depth_files = [f for f in files if f.endswith("_depth.png")]
    assert len(depth_files) == 16 and len(files) == 32
    for i, f in enumerate(depth_files):
        want = decode_depth16(encode_depth16(preds[i, ..., 0], "midair16"), "midair16")
        got = read_depth_png(os.path.join(out, f), "midair16")
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), f
    with Image.open(os.path.join(out, files[1])) as im:
        assert files[1].endswith("_panels.png") and im.size == (64, 4 * 64) and im.mode == "RGB"
