"""The options of ``m4depth_amd.main`` (and, extended, of ``m4depth_amd.finetune_kitti``): the parser and every refusal that
needs no GPU.  ``check_args`` runs all of them in the driver's order; every option's default lives in ``build_parser`` or, for
the options that are None when not given, in the one place that reads them."""
from __future__ import annotations

import argparse
import os

from .fusion import MAP_COMPANIONS, VOLUME_COMPANIONS
from .network import M4depthAblationParameters


def build_parser():
    p = argparse.ArgumentParser(description="M4Depth (MI355X native) train / eval / predict driver")
    p.add_argument("--mode", default="eval", choices=["train", "finetune", "eval", "validation", "predict"])
    p.add_argument("--dataset", default="synthetic", choices=["synthetic", "midair", "tartanair", "kitti-raw", "recording"],
                   help="a dataset of the reference (m4depth_options.py:11-14), the seeded synthetic one, or your own recording "
                        "(--records_path = a recording directory or a directory of them, dataloaders/recording.py; needs "
                        "--height and --width, no --db_path_config)")
    p.add_argument("--db_path_config", default=None, help="json file with the dataset roots (m4depth_options.py:27-29)")
    p.add_argument("--records_path", default=None, help="directory of trajectory csv files (m4depth_options.py:33-35)")
    p.add_argument("--rec_stride", type=int, default=None, metavar="N",
                   help="--dataset=recording: take every N-th frame of a trajectory (default 1)")
    p.add_argument("--rec_min_baseline", type=float, default=None, metavar="METRES",
                   help="--dataset=recording: of those, keep a frame when the camera centre has moved at least this far since "
                        "the last kept frame (default 0)")
    p.add_argument("--rec_max_gap", type=float, default=None, metavar="SECONDS",
                   help="--dataset=recording: drop a frame whose bracketing poses are further apart than this; the next kept "
                        "frame starts a new trajectory (default 0.5)")
    p.add_argument("--no_augmentation", action="store_true")
    p.add_argument("--epochs", type=int, default=1, help="train on a real dataset: passes over the records")
    p.add_argument("--arch_depth", type=int, default=6, help="number of pyramid levels (m4depth_options.py:64)")
    p.add_argument("--seq_len", type=int, default=4)
    p.add_argument("--db_seq_len", type=int, default=None)
    p.add_argument("--batch_size", type=int, default=1, help="GLOBAL batch (sharded over ranks)")
    p.add_argument("--n_batches", type=int, default=2, help="synthetic dataset: batches to generate")
    p.add_argument("--height", type=int, default=None, help="frame height (default: 384 synthetic, else the dataset's)")
    p.add_argument("--width", type=int, default=None)
    p.add_argument("--ckpt_dir", default="ckpt")
    p.add_argument("--tf_checkpoint", default=None,
                   help="TensorFlow checkpoint of the reference model (prefix, or a directory holding a 'checkpoint' state "
                        "file, e.g. pretrained_weights/midair): used instead of <ckpt_dir>/train for the initial weights")
    p.add_argument("--seed", type=int, default=1234)
    p.add_argument("--graph", action="store_true", help="replay the sequence forward from a hipGraph")
    p.add_argument("--stream", action="store_true",
                   help="predict: run the frames as B independent streams with per-sample trajectory resets (M4Depth.stream_step; "
                        "with --graph replayed from network.GraphedStream)")
    p.add_argument("--eval_streams", type=int, default=0, metavar="N",
                   help="eval / validation on a dataset's whole trajectories (no --db_seq_len): run N trajectories side by side "
                        "as the samples of M4Depth.stream_step (with --graph replayed from network.GraphedStream), score each "
                        "sample on the device and fold the scores in the sequential run's order -- the same perfs file as the "
                        "one-frame-at-a-time loop.  0 = that loop")
    p.add_argument("--eval_streams_policy", default="lpt", choices=["lpt", "arrival"],
                   help="--eval_streams: the order trajectories are dealt to free slots (lpt = longest first, arrival = csv order)")
    p.add_argument("--consistency", action="store_true",
                   help="--eval_streams: also score every frame without ground truth -- the previous frame reprojected with the "
                        "estimated depth against the current one (photo: SSIM + L1, the criterion) and the estimate against the "
                        "previous frame's (geo, a diagnostic); m4depth_amd.consistency.  Writes perfs-consistency-<dataset>.txt "
                        "and consistency-frames-<dataset>.txt; a set without ground truth (a recording without depth.txt) is then "
                        "accepted and the seven metrics are skipped")
    p.add_argument("--refine_pose", action="store_true",
                   help="--eval_streams / predict --stream: before every step, align the frame's motion to the images -- "
                        "Gauss-Newton direct alignment of the current frame against the previous frame and its estimated depth, "
                        "per sample on the GPU, started from the given motion (m4depth_amd.pose_refine; the defaults are "
                        "untuned).  The network, --consistency and --save_cloud then see the refined motion; --eval_streams "
                        "writes pose-refine-frames-<dataset>.txt")
    p.add_argument("--refine_pose_strides", default=None, metavar="LIST",
                   help="--refine_pose: comma list of pyramid strides, coarse to fine, powers of two (default 8,4,2)")
    p.add_argument("--refine_pose_iters", type=int, default=None, metavar="N",
                   help="--refine_pose: Gauss-Newton iterations per stride (default 4)")
    p.add_argument("--refine_pose_prior", type=float, nargs=2, default=None, metavar=("LT", "LR"),
                   help="--refine_pose: weights of the prior towards the given motion, per m^2 and per rad^2 (default 0 0: off)")
    p.add_argument("--refine_pose_max", type=float, nargs=2, default=None, metavar=("METRES", "DEGREES"),
                   help="--refine_pose: a correction larger than this is rejected and the given motion kept (default 0.05 0.5)")
    p.add_argument("--host_input", action="store_true",
                   help="synthetic eval: hand every batch over from pinned HOST memory (the PCIe copy is part of the step) and "
                        "print the frames/s of the loop -- the PCIe-inclusive rate, next to bench.py's HBM-resident one")
    p.add_argument("--save_dir", default=None, metavar="DIR",
                   help="predict: write every frame to DIR/s<slot>_t<trajectory>/<frame>_depth.png (16-bit, --save_format), "
                        "encoded on the GPU and compressed in host threads (m4depth_amd.export), instead of predictions.npy")
    p.add_argument("--save_format", default=None, choices=["kitti16", "midair16"],
                   help="--save_dir: uint16 = depth * 256 (kitti16, the default) or float16 bits of 512 / depth (midair16)")
    p.add_argument("--save_panels", default=None, metavar="LIST",
                   help="--save_dir: comma list of rgb,est,gt,err -- also write <frame>_panels.png with these panels stacked "
                        "vertically (default: none)")
    p.add_argument("--save_range", type=float, nargs=2, default=None, metavar=("NEAR", "FAR"),
                   help="--save_panels: the depths the colour scale of est / gt spans, linear in inverse depth (default 1 80)")
    p.add_argument("--save_err_max", type=float, default=None,
                   help="--save_panels: the relative error the colour scale of err saturates at (default 0.5)")
    p.add_argument("--save_cloud", action="store_true",
                   help="--save_dir: also write <frame>_cloud.ply, the estimate as coloured 3-D points (depths within "
                        "--save_range), back-projected, posed and compacted on the GPU")
    p.add_argument("--cloud_stride", type=int, default=None, metavar="N",
                   help="--save_cloud: keep every N-th pixel of every N-th row (default 2)")
    p.add_argument("--cloud_frame", default=None, choices=["world", "camera"],
                   help="--save_cloud: coordinates in the frame of the trajectory's first camera (world, the default; the "
                        "frame-to-frame motions are chained on the GPU) or of each frame's own camera")
    # the four options of the multi-view check are absent from the namespace until given (SUPPRESS): check_save_args fills in
    # their defaults, and a parse without them yields exactly the destinations it yielded before they existed
    p.add_argument("--cloud_views", type=int, default=argparse.SUPPRESS, metavar="K",
                   help="--save_cloud: keep a pixel only if earlier frames of its trajectory confirm it -- its 3-D point, seen "
                        "from up to K (1..8) earlier frames, lands on a surface they estimated too and projects back onto the "
                        "pixel (default 0 = off).  Strict: the first --cloud_min_views frames of a trajectory give empty clouds")
    p.add_argument("--cloud_min_views", type=int, default=argparse.SUPPRESS, metavar="N",
                   help="--cloud_views: confirming frames a pixel needs, 1..K (default min(2, K))")
    p.add_argument("--cloud_tol", type=float, nargs=2, default=argparse.SUPPRESS, metavar=("PX", "REL"),
                   help="--cloud_views: a frame confirms within PX pixels of reprojection error and REL relative depth "
                        "difference (default 1.0 0.01: MVSNet's fusion thresholds, untuned for this network)")
    p.add_argument("--save_conf", action="store_true", default=argparse.SUPPRESS,
                   help="--cloud_views: also write <frame>_conf.png, 8-bit grey = confirming frames * 255 // K")
    # like the multi-view options above: absent from the namespace until given
    p.add_argument("--save_map", type=float, default=argparse.SUPPRESS, metavar="VOXEL",
                   help="--save_dir: also write DIR/s<slot>_t<trajectory>/map.ply, ONE fused map per trajectory -- the vertices "
                        "of its clouds (as --cloud_stride, --save_range and --cloud_views make them, with or without "
                        "--save_cloud) merged on the GPU into one vertex per occupied voxel of VOXEL metres: mean position, "
                        "mean colour, alpha = frames that saw it.  --cloud_views is the recommended companion: without it "
                        "every depth-edge pixel lands in the map")
    p.add_argument("--map_min_frames", type=int, default=argparse.SUPPRESS, metavar="N",
                   help="--save_map: a voxel is written only if at least N frames of the trajectory put a point in it (default 2)")
    p.add_argument("--map_slots_log2", type=int, default=argparse.SUPPRESS, metavar="L",
                   help="--save_map: 2^L hash-table slots per sample, 16..26 (default 21: 168 MB per sample; a map stops "
                        "taking new voxels at 3/4 of them, and the closing line of the run counts what was dropped)")
    # like the map's: absent from the namespace until given
    p.add_argument("--save_mesh", type=float, default=argparse.SUPPRESS, metavar="VOXEL",
                   help="--save_dir: also write DIR/s<slot>_t<trajectory>/mesh.ply, ONE triangle mesh per trajectory -- the "
                        "estimates (as --save_range and --cloud_views make them; --cloud_stride does not apply, every pixel "
                        "counts) fused on the GPU into a truncated signed distance field on a hashed grid of VOXEL metres and "
                        "extracted by naive surface nets.  Independent of --save_cloud and --save_map.  --cloud_views is the "
                        "recommended companion.  VOXEL, --mesh_trunc and --mesh_min_frames are untuned")
    p.add_argument("--mesh_trunc", type=int, default=argparse.SUPPRESS, metavar="K",
                   help="--save_mesh: the truncation distance in voxels, 2..8 (default 4)")
    p.add_argument("--mesh_min_frames", type=int, default=argparse.SUPPRESS, metavar="N",
                   help="--save_mesh: a voxel takes part in the surface only if at least N frames updated it (default 2)")
    p.add_argument("--mesh_slots_log2", type=int, default=argparse.SUPPRESS, metavar="L",
                   help="--save_mesh: 2^L hash-table slots per sample, 16..26 (default 22: 134 MB per sample; a volume stops "
                        "taking new voxels at 3/4 of them, and the closing line of the run counts what was dropped)")
    # like the mesh's: absent from the namespace until given
    p.add_argument("--fused", type=float, default=argparse.SUPPRESS, metavar="VOXEL",
                   help="--eval_streams: also score the FUSED depth of every frame -- the estimates of the trajectory so far fused "
                        "on the GPU into a truncated signed distance field on a hashed grid of VOXEL metres (as --save_mesh does) "
                        "and rendered back into the frame by ray marching over 1..80 m; where the volume has no surface the raw "
                        "estimate stays.  Writes perfs-fused-<dataset>.txt (the seven metrics of the fused depth, next to the "
                        "unchanged perfs-<dataset>.txt) and fused-frames-<dataset>.txt.  Needs ground truth")
    p.add_argument("--fused_trunc", type=int, default=argparse.SUPPRESS, metavar="K",
                   help="--fused: the truncation distance in voxels, 2..8 (default 4)")
    p.add_argument("--fused_min_frames", type=int, default=argparse.SUPPRESS, metavar="N",
                   help="--fused: a voxel is rendered only if at least N frames updated it (default 2)")
    p.add_argument("--fused_slots_log2", type=int, default=argparse.SUPPRESS, metavar="L",
                   help="--fused: 2^L hash-table slots per sample, 16..26 (default 22: 134 MB per sample; the closing line counts "
                        "what a full table dropped)")
    p.add_argument("--fused_window", type=int, default=argparse.SUPPRESS, metavar="W",
                   help="--fused / --save_fused: march only W >= 1 truncation distances around the raw estimate of each pixel "
                        "instead of the whole range (several times fewer probes; a surface further from the estimate is missed)")
    p.add_argument("--fused_interp", choices=["nearest", "trilinear"], default=argparse.SUPPRESS,
                   help="--fused / --save_fused: how the march samples the field (default nearest: the value of the voxel a "
                        "sample falls in; trilinear: the blend of the eight voxels around it where all are known -- no half-voxel "
                        "staircase in the rendered depth, eight table probes per sample instead of one)")
    p.add_argument("--save_fused", action="store_true", default=argparse.SUPPRESS,
                   help="--save_mesh: also write <frame>_fused.png, the mesh's volume rendered into the frame (--save_format; "
                        "a pixel without a surface is written as a non-finite estimate is: 0 in kitti16, 0x7C00 in midair16)")
    p.add_argument("--save_fused_view", action="store_true", default=argparse.SUPPRESS,
                   help="--save_fused: also write <frame>_fused_view.png, an RGB8 picture of the rendered surface -- the volume's "
                        "colour under a headlight along the interpolated field's normal; black where there is no surface")
    p.add_argument("--learning_rate", type=float, default=1e-4, help="Adam step size (main.py:88)")
    p.add_argument("--loss", default="supervised", choices=["supervised", "photometric"],
                   help="train: supervised = the reference's log-depth L1 against ground truth; photometric = the reprojection "
                        "loss between neighbouring frames (SSIM + L1, auto-masking, edge-aware smoothness), which needs poses "
                        "but no ground-truth depth -- the way to finetune on a --dataset=recording without depth.txt")
    p.add_argument("--photo_smooth", type=float, default=None,
                   help="--loss=photometric: weight of the edge-aware smoothness term (default 1e-3, Monodepth2's value; not "
                        "tuned for this network)")
    p.add_argument("--no_photo_automask", action="store_true",
                   help="--loss=photometric: keep the pixels whose unwarped previous frame already matches better (auto-masking off)")
    p.add_argument("--photo_scale", default=None, choices=["level", "full"],
                   help="--loss=photometric: level (default) = each term at its level's resolution against the image pyramid; "
                        "full = every level's depth upsampled to the input resolution and compared there (Monodepth2's form)")
    p.add_argument("--photo_sources", default=None, choices=["prev", "both"],
                   help="--loss=photometric: prev (default) = frame t-1 only; both = the per-pixel minimum over frame t-1 and frame "
                        "t+1, which drops pixels one neighbour does not see (needs quaternion rotations)")
    p.add_argument("--save_every", type=int, default=0, help="train: checkpoint every N steps (0 = at the end)")
    p.add_argument("--summary_interval", type=int, default=1200,
                   help="train --graph: read the device-side step log every N steps (m4depth_options.py:47-49); it is also "
                        "read at every epoch end and before every checkpoint")
    p.add_argument("--log_dir", default=None, metavar="DIR",
                   help="train: write a TensorBoard event file to DIR (m4depth_options.py:43; m4depth_amd.summaries): loss and "
                        "RMSE_log of every step, and every --summary_interval steps the images of the reference's train_step "
                        "(RGB_im, camera_prev_t_reproj, depth_gt, depth_lvl_i), converted on the GPU and compressed in host "
                        "threads.  Rank 0 only")
    p.add_argument("--max_keep", type=int, default=0,
                   help="train: keep only the newest N checkpoints of <ckpt_dir>/train (0 = keep all)")
    p.add_argument("--enable_validation", action="store_true",
                   help="train: checkpoint at every epoch end and validate that checkpoint in-process (--mode=validation on "
                        "--val_dataset / --val_records_path, seq_len 4 / db_seq_len 4), keeping the best-N in <ckpt_dir>/best")
    p.add_argument("--val_records_path", default=None, help="--enable_validation: trajectory csv files of the validation set")
    p.add_argument("--val_dataset", default="kitti-raw", choices=["midair", "tartanair", "kitti-raw", "recording"],
                   help="--enable_validation: the validation set's dataset")
    p.add_argument("--val_consistency", action="store_true",
                   help="--enable_validation: validate as --eval_streams <batch_size> --consistency on whole trajectories instead "
                        "of the 4-frame sequence batches, appending a line to validation-consistency.txt; required for a "
                        "validation set without ground truth, where best-N is then judged on photo alone (lower is better)")
    p.add_argument("--keep_top_n", type=int, default=1,
                   help="validation: how many best checkpoints <ckpt_dir>/best keeps (callbacks.py:173-240)")
    # ablation flags, spelled as in m4depth_options.py:67-84
    for flag in ("DINL", "SNCV", "time_recurr", "feature_normalization", "feature_subdivision", "level_memory"):
        p.add_argument(f"--no_{flag}", action="store_true")
    return p


def ablation_from_args(args):
    return M4depthAblationParameters(not args.no_DINL, not args.no_SNCV, not args.no_time_recurr,
                                     not args.no_feature_normalization, not args.no_feature_subdivision,
                                     not args.no_level_memory)                  # m4depth_options.py:96-98


def records_have_depth(args):
    """Whether the trajectory files of ``--records_path`` name a ground-truth map (the loader's depth column): known on the
    host before anything is loaded."""
    import glob
    from . import dataloaders as dl
    if args.dataset == "recording":
        return dl.get_loader("recording").has_depth(args.records_path)
    col = dl.get_loader(args.dataset)._depth_column()
    files = sorted(glob.glob(os.path.join(args.records_path, "**/*.csv"), recursive=True))
    if not files:
        return False
    with open(files[0], newline="") as fh:
        return col in fh.readline().rstrip("\r\n").split("\t")


def check_stream_args(parser, args):
    if args.stream and args.mode != "predict":
        parser.error("--stream is a --mode=predict option")


def _check_eval_streams(parser, args):
    if args.eval_streams < 0:
        parser.error("--eval_streams must be >= 0")
    if args.consistency and (not args.eval_streams or args.mode not in ("eval", "validation")):
        parser.error("--consistency needs --eval_streams B (with or without --graph) in --mode=eval / --mode=validation: it scores "
                     "whole trajectories, each frame against the one before it")
    if not args.eval_streams:
        return
    if args.mode not in ("eval", "validation"):
        parser.error("--eval_streams is a --mode=eval / --mode=validation option")
    if args.dataset == "synthetic":
        parser.error("--eval_streams runs the trajectories of a real dataset (--dataset midair | tartanair | kitti-raw | recording)")
    if args.db_seq_len is not None:
        parser.error("--eval_streams evaluates whole trajectories: it excludes --db_seq_len")


def check_train_args(parser, args, world=None):
    """Refusals of the training workflow's options.  ``world``: the number of ranks (default: WORLD_SIZE of the environment,
    what dist.init_from_env will see)."""
    if world is None:
        world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.summary_interval < 1:
        parser.error("--summary_interval must be >= 1")
    if args.log_dir is not None and args.mode not in ("train", "finetune"):
        parser.error("--log_dir is a --mode=train / --mode=finetune option")
    if args.max_keep < 0:
        parser.error("--max_keep must be >= 0")
    if args.keep_top_n < 1:
        parser.error("--keep_top_n must be >= 1")
    if args.enable_validation:
        if args.val_records_path is None:
            parser.error("--enable_validation needs --val_records_path (the validation set's trajectory csv files)")
        if args.db_path_config is None:
            parser.error("--enable_validation needs --db_path_config (the validation set's dataset root)")
        if world > 1:
            parser.error("--enable_validation runs in-process on one GPU: it is refused with several ranks")
    elif args.val_consistency:
        parser.error("--val_consistency needs --enable_validation (it chooses how that validation scores)")
    photo_opts = [f for f, on in (("photo_smooth", args.photo_smooth is not None), ("no_photo_automask", args.no_photo_automask),
                                      ("photo_scale", args.photo_scale is not None), ("photo_sources", args.photo_sources is not None)) if on]
    if args.loss != "supervised" and args.mode != "train":
        parser.error("--loss=%s is a --mode=train option" % args.loss)
    if photo_opts and args.loss != "photometric":
        parser.error("--%s needs --loss=photometric" % photo_opts[0])
    if args.photo_smooth is not None and not args.photo_smooth >= 0:
        parser.error("--photo_smooth must be >= 0")
    if args.mode == "train" and args.loss == "supervised" and args.dataset == "recording" and args.records_path is not None:
        try:
            if not records_have_depth(args):
                parser.error("--mode=train on a recording without depth.txt needs --loss=photometric (the supervised loss reads "
                             "ground-truth depth)")
        except ValueError:
            pass                                   # a malformed --records_path: check_recording_args reports it
    if args.enable_validation and args.val_dataset == "recording" and args.val_records_path is not None:
        from . import dataloaders as dl
        try:
            scored = dl.get_loader("recording").has_depth(args.val_records_path)
        except ValueError as e:
            parser.error("--val_records_path %s" % e)
        if not scored and not args.val_consistency:
            parser.error("--enable_validation: a recording of --val_records_path has no depth.txt -- validation scores against "
                         "ground truth, which such a recording does not have")
    if args.graph and args.mode in ("train", "finetune") and world > 1:
        parser.error("--graph training is refused with several ranks (RCCL inside a captured training step is not supported)")


def check_recording_args(parser, args):
    """Refusals around ``--dataset=recording``: its ``--rec_*`` options belong to it alone, and a recording has no default
    network size."""
    given = [f for f in ("rec_stride", "rec_min_baseline", "rec_max_gap") if getattr(args, f) is not None]
    if args.dataset != "recording":
        if given:
            parser.error("--%s is a --dataset=recording option" % given[0])
        return
    if args.height is None or args.width is None:
        parser.error("--dataset=recording needs --height and --width (the size the frames are undistorted and resized to)")
    if args.records_path is not None:
        from .dataloaders.recording import find_recordings
        try:
            find_recordings(args.records_path)
        except ValueError as e:
            parser.error("--records_path %s" % e)
    unit = 2 ** args.arch_depth
    if args.height < unit or args.width < unit or args.height % unit or args.width % unit:
        parser.error("--dataset=recording: --height and --width must be positive multiples of 2**arch_depth = %d" % unit)
    if args.rec_stride is not None and args.rec_stride < 1:
        parser.error("--rec_stride must be >= 1")
    if args.rec_min_baseline is not None and not args.rec_min_baseline >= 0:
        parser.error("--rec_min_baseline must be >= 0")
    if args.rec_max_gap is not None and not args.rec_max_gap > 0:
        parser.error("--rec_max_gap must be > 0")


CLI_SLOTS_LOG2_MIN = 16      # the command line's floor for every --*_slots_log2; the Python API takes smaller tables


def _cli_companions(prefix, companions):                # the chain's table (fusion.py) under the options' prefix, with that floor
    return tuple((prefix + name, default, max(lo, CLI_SLOTS_LOG2_MIN) if name == "slots_log2" else lo, hi)
                 for name, default, lo, hi in companions)


# the per-trajectory products of --save_dir: flag, its companions (option, default, lowest, highest or None) and why the camera
# frame is refused.  The voxel map runs on the clouds' vertices, so the clouds' options serve it too; the TSDF mesh reads the
# estimate itself, so of the clouds' options only --cloud_frame concerns it
_TRAJECTORY_PRODUCTS = (
    ("save_map", _cli_companions("map_", MAP_COMPANIONS), "a map merges the frames of a trajectory in one frame"),
    ("save_mesh", _cli_companions("mesh_", VOLUME_COMPANIONS), "a mesh fuses the frames of a trajectory in one frame"))


def _check_companions(parser, args, companions):
    """The ranges of the companions that were given, and the defaults of the others."""
    for f, default, lo, hi in companions:
        v = getattr(args, f)
        if v is not None and (v < lo or (hi is not None and v > hi)):
            parser.error("--%s must be %s" % (f, ">= %d" % lo if hi is None else "in %d..%d" % (lo, hi)))
        setattr(args, f, default if v is None else v)


def _check_trajectory_product(parser, args, flag, companions, reason):
    """The refusals and defaults of one of them (its options are absent from the namespace until given); whether it is on."""
    for f in (flag,) + tuple(c[0] for c in companions):
        setattr(args, f, getattr(args, f, None))
    voxel = getattr(args, flag)
    given = [c[0] for c in companions if getattr(args, c[0]) is not None]
    if given and voxel is None:
        parser.error("--%s needs --%s" % (given[0], flag))
    if voxel is None:
        return False
    if not (0 < voxel < float("inf")):
        parser.error("--%s VOXEL needs a finite edge length > 0" % flag)
    if args.cloud_frame == "camera":
        parser.error("--%s needs --cloud_frame world: %s" % (flag, reason))
    _check_companions(parser, args, companions)
    return True


def check_save_args(parser, args):
    """Refusals of the ``--save_*`` options; fills in their defaults and parses ``--save_panels`` into a tuple."""
    from .export import PANELS
    others = [f for f in ("save_format", "save_panels", "save_range", "save_err_max") if getattr(args, f) is not None]
    others += [f for f in ("save_cloud",) if args.save_cloud]
    for product in _TRAJECTORY_PRODUCTS:
        if _check_trajectory_product(parser, args, *product):
            others.append(product[0])
    geometry = args.save_cloud or args.save_map is not None or args.save_mesh is not None
    cloud_others = [f for f in ("cloud_stride", "cloud_frame") if getattr(args, f) is not None]
    if args.save_dir is not None and cloud_others and not geometry:
        parser.error("--%s needs --save_cloud" % cloud_others[0])
    others += cloud_others
    if args.cloud_stride is not None and args.cloud_stride < 1:
        parser.error("--cloud_stride must be >= 1")
    args.cloud_stride = 2 if args.cloud_stride is None else args.cloud_stride
    args.cloud_frame = args.cloud_frame or "world"
    # the multi-view check runs on the clouds' pose chain: every option of it needs --save_cloud or --save_map (and so --save_dir)
    for f in ("cloud_views", "cloud_min_views", "cloud_tol"):
        setattr(args, f, getattr(args, f, None))
    args.save_conf = bool(getattr(args, "save_conf", False))
    view_others = [f for f in ("cloud_views", "cloud_min_views", "cloud_tol") if getattr(args, f) is not None]
    view_others += [f for f in ("save_conf",) if args.save_conf]
    if view_others and not geometry:
        parser.error("--%s needs --save_cloud" % view_others[0])
    if args.cloud_views is not None and not 0 <= args.cloud_views <= 8:
        parser.error("--cloud_views must be 0 (off) or 1..8")
    args.cloud_views = args.cloud_views or 0
    dependents = [f for f in view_others if f != "cloud_views"]
    if dependents and not args.cloud_views:
        parser.error("--%s needs --cloud_views" % dependents[0])
    if args.cloud_min_views is not None and not 1 <= args.cloud_min_views <= args.cloud_views:
        parser.error("--cloud_min_views must be in 1..%d (--cloud_views)" % args.cloud_views)
    if args.cloud_views and args.cloud_min_views is None:
        args.cloud_min_views = min(2, args.cloud_views)
    args.cloud_tol = tuple(args.cloud_tol) if args.cloud_tol is not None else (1.0, 0.01)
    if not (args.cloud_tol[0] > 0 and args.cloud_tol[1] > 0):
        parser.error("--cloud_tol PX REL needs PX > 0 and REL > 0")
    if args.save_dir is None:
        if others:
            parser.error("--%s needs --save_dir" % others[0])
        return
    if args.mode != "predict":
        parser.error("--save_dir is a --mode=predict option")
    args.save_format = args.save_format or "kitti16"
    panels = tuple(p for p in (args.save_panels or "").split(",") if p)
    if len(panels) > 4 or any(p not in PANELS for p in panels):
        parser.error("--save_panels: a comma list of up to four of %s, got %r" % (",".join(PANELS), args.save_panels))
    args.save_panels = panels
    args.save_range = tuple(args.save_range) if args.save_range is not None else (1.0, 80.0)
    args.save_err_max = 0.5 if args.save_err_max is None else args.save_err_max
    if not (0 < args.save_range[0] < args.save_range[1]):
        parser.error("--save_range NEAR FAR needs 0 < NEAR < FAR")
    if not args.save_err_max > 0:
        parser.error("--save_err_max must be > 0")
    if any(p in ("gt", "err") for p in panels) and args.dataset != "synthetic" and args.records_path is not None \
            and not records_have_depth(args):
        parser.error("--save_panels %s: the records of --records_path name no ground-truth map" % ",".join(panels))


def check_refine_args(parser, args):
    """Refusals of ``--refine_pose`` and its options; fills in their defaults (``pose_refine.DEFAULTS``) and parses
    ``--refine_pose_strides`` into a tuple."""
    import math
    others = [f for f in ("refine_pose_strides", "refine_pose_iters", "refine_pose_prior", "refine_pose_max")
              if getattr(args, f) is not None]
    if not args.refine_pose:
        if others:
            parser.error("--%s needs --refine_pose" % others[0])
        return
    streams = args.mode in ("eval", "validation") and args.eval_streams > 0
    if not streams and not (args.mode == "predict" and args.stream):
        parser.error("--refine_pose needs --eval_streams B in --mode=eval / --mode=validation or --stream in --mode=predict (with "
                     "or without --graph): it aligns each frame of a trajectory against the one before it")
    from .pose_refine import DEFAULTS
    if args.refine_pose_strides is None:
        args.refine_pose_strides = DEFAULTS["strides"]
    else:
        try:
            strides = tuple(int(v) for v in args.refine_pose_strides.split(","))
        except ValueError:
            strides = ()
        if not strides or any(v < 1 or v & (v - 1) for v in strides):
            parser.error("--refine_pose_strides: a comma list of powers of two, got %r" % args.refine_pose_strides)
        args.refine_pose_strides = strides
    if args.refine_pose_iters is None:
        args.refine_pose_iters = DEFAULTS["iters"]
    if args.refine_pose_iters < 1:
        parser.error("--refine_pose_iters must be >= 1")
    args.refine_pose_prior = tuple(args.refine_pose_prior) if args.refine_pose_prior is not None else DEFAULTS["prior"]
    if not (args.refine_pose_prior[0] >= 0 and args.refine_pose_prior[1] >= 0):
        parser.error("--refine_pose_prior LT LR must be >= 0")
    args.refine_pose_max = tuple(args.refine_pose_max) if args.refine_pose_max is not None \
        else (DEFAULTS["caps"][0], math.degrees(DEFAULTS["caps"][1]))
    if not (args.refine_pose_max[0] >= 0 and args.refine_pose_max[1] >= 0):
        parser.error("--refine_pose_max METRES DEGREES must be >= 0")
    if args.height is not None and args.width is not None:
        top = max(args.refine_pose_strides)
        if args.height % top or args.width % top or args.height // top < 3 or args.width // top < 3:
            parser.error("--refine_pose_strides: --height and --width must be multiples of the largest stride, at least 3 of them")


# --fused VOXEL renders the volume --save_mesh builds: its companions are the same table under its own prefix;
# --fused_window (no default: absent = the whole range) and --fused_interp (absent = nearest) also serve --save_fused
_FUSED_COMPANIONS = _cli_companions("fused_", VOLUME_COMPANIONS)


def check_fused_args(parser, args):
    """Refusals of ``--fused`` / ``--save_fused`` and their options (absent from the namespace until given); fills in the defaults.
    Runs after ``check_save_args``."""
    for f in ("fused", "fused_window") + tuple(c[0] for c in _FUSED_COMPANIONS):
        setattr(args, f, getattr(args, f, None))
    args.save_fused = bool(getattr(args, "save_fused", False))
    args.save_fused_view = bool(getattr(args, "save_fused_view", False))
    given = [c[0] for c in _FUSED_COMPANIONS if getattr(args, c[0]) is not None]
    if given and args.fused is None:
        parser.error("--%s needs --fused" % given[0])
    if hasattr(args, "fused_interp") and args.fused is None and not args.save_fused:
        parser.error("--fused_interp needs --fused or --save_fused")
    args.fused_interp = getattr(args, "fused_interp", "nearest")
    if args.save_fused_view and not args.save_fused:
        parser.error("--save_fused_view needs --save_fused: it is the same rendering's picture")
    if args.fused_window is not None and args.fused is None and not args.save_fused:
        parser.error("--fused_window needs --fused or --save_fused")
    if args.fused_window is not None and args.fused_window < 1:
        parser.error("--fused_window must be >= 1")
    if args.save_fused and args.save_mesh is None:
        parser.error("--save_fused needs --save_mesh: it renders the mesh's volume")
    if args.fused is None:
        return
    if not (args.eval_streams and args.mode == "eval"):
        parser.error("--fused needs --eval_streams B (with or without --graph) in --mode=eval: it fuses whole trajectories, frame "
                     "by frame")
    if not (0 < args.fused < float("inf")):
        parser.error("--fused VOXEL needs a finite edge length > 0")
    _check_companions(parser, args, _FUSED_COMPANIONS)
    if args.consistency and args.records_path is not None and not records_have_depth(args):
        parser.error("--fused scores against ground truth: the records of --records_path name no ground-truth map")


def check_args(parser, args, world=None):
    """Every refusal of ``m4depth_amd.main``, in the order they win."""
    check_stream_args(parser, args)
    _check_eval_streams(parser, args)
    check_refine_args(parser, args)
    check_train_args(parser, args, world)
    check_recording_args(parser, args)
    check_save_args(parser, args)
    check_fused_args(parser, args)
