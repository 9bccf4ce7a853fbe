"""`python -m dsrg_amd.train`: the two training runs of run.sh, fed from files.

  --stage s  <-> training/tools/train.py --solver solver-s.prototxt   (DSRG training: train-s.prototxt; DSRGTrainer + TrainSInput)
  --stage f  <-> training/tools/train.py --solver solver-f.prototxt   (retraining on the pseudo labels: train-f.prototxt;
                                                                      RetrainTrainer + TrainFInput)

Stage s reads --list ('name.jpg <id>' lines, the reference's list/input_list.txt), the images under --root and the localisation
cues of --cues; stage f reads --list ('image_path label_path' lines, list/train.txt) with --root prefixed to both paths.  The
defaults are the solver files' values (STAGE_DEFAULTS).  --class N (1..96, default 21; 81: the reference's COCO variant) sets the
outputs of the network's classifiers in both stages and reaches the loader and the validator.  Stage s with --cue-maps is fed as
AnnotationLayerCOCO feeds the 81-class runs (pylayers.py:432-512; TrainSCueMapInput): --list then holds 'image_path cue_path'
lines with --root prefixed to both, a cue file is a 41 x 41 one-channel image of classes with 255 = no cue, --cues is absent and
the images are zoomed to 321 x 321; --channel-order rgb feeds the net R G B as that layer does (the default, bgr, is what this
project's predict and validate — and the reference's test-coco.py — feed).  Stage f's --scale-factors (not the reference's; DeepLab's augmentation for
--backbone resnet101 --crop 513, where no VOC image leaves the crop any slack) rescales each image by a drawn factor before the crop.  Stage f's --loss-at label (not the reference's either) takes the softmax loss at label
resolution — the logits zoomed to the label map, every label pixel judged, one fused HIP call (retrain.seg_softmax_loss_zoom) — and
adds the pixel accuracy of the display window to the display line; the default, map, is the reference's step.  Stage f's
--msc-scales 0.75,0.5 (DeepLab-v2's multi-scale inputs with max fusion, not the reference's either) runs the network on the crop and
on the crop zoomed by every scale, fuses the score maps by their maximum and judges the fused map and every scale's own map
(retrain.seg_softmax_loss_msc, one fused HIP call); the display line then reads loss, loss-fusion, loss-res1, loss-res<scale>...
and the fused head's pixel accuracy.  Batches are assembled on the GPU (dsrg_amd/input.py) while the step
before runs.  Every --display steps the mean of the last --display losses is printed with the learning rate; snapshots
(<prefix>_iter_N.caffemodel + .solverstate.pt) are written every --snapshot-every steps and at the end; --snapshot resumes at the
snapshot's iteration count.  Under a launcher (torch.distributed.run: RANK / WORLD_SIZE set) every rank takes its shard of each
epoch and --batch / WORLD_SIZE images per step.

--val-list ('image_path label_path' lines, --val-root prefixed to both; ground-truth label PNGs) turns on validation: every
--val-every steps (default: whenever a snapshot is written) and at the last iteration the network is scored over the list by
dsrg_amd.validate.Validator — single scale, every image padded to --val-crop, no CRF — and rank 0 prints the mean IoU and the pixel
accuracy (and rewrites --val-result in evaluate's three-line format).  Every rank scores its share of the list; the pass is
collective and leaves the run's weights, momentum and random streams as it found them: a run with validation ends with the
weights of the same run without.
"""
import argparse
import os
import sys

# solver-s.prototxt / train-s.prototxt:14-21 and solver-f.prototxt / train-f.prototxt:11
STAGE_DEFAULTS = {
    "s": dict(iters=8000, snapshot_every=8000, display=10, prefix="models/model-s", batch=20),
    "f": dict(iters=20000, snapshot_every=10000, display=20, prefix="models/model-f", batch=10),
}
F_DEFAULTS = dict(crop=321, mean=(104.0, 117.0, 123.0))
VAL_CROP = 513                                   # no VOC image is larger


def val_batch(a, world):
    """validation images per forward on one rank: --val-batch, else the per-rank training batch"""
    return a.val_batch if a.val_batch is not None else a.batch // world


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="python -m dsrg_amd.train", description="train stage s (DSRG) or stage f (retrain) from files")
    p.add_argument("--stage", choices=("s", "f"), required=True, help="s: solver-s.prototxt (DSRG training); f: solver-f.prototxt (retrain)")
    p.add_argument("--list", required=True, help="s: 'name.jpg <id>' lines; f: 'image_path label_path' lines")
    p.add_argument("--root", required=True, help="s: directory of the images; f: prefix of both paths of a list line")
    p.add_argument("--weights", default=None, help="initial weights (.caffemodel, .npz or torch file), copied by layer name")
    p.add_argument("--snapshot", default=None, help="a .solverstate.pt written by an earlier run: resume there")
    p.add_argument("--prefix", default=None, help="snapshot prefix (s: models/model-s, f: models/model-f)")
    p.add_argument("--iters", type=int, default=None, help="last iteration (s: 8000, f: 20000)")
    p.add_argument("--snapshot-every", type=int, default=None, help="snapshot interval (s: 8000, f: 10000)")
    p.add_argument("--batch", type=int, default=None, help="images per step over all ranks (s: 20, f: 10)")
    p.add_argument("--seed", type=int, default=0, help="weights, dropout, shuffle and augmentation draws (solver: random_seed 0)")
    p.add_argument("--display", type=int, default=None, help="print the mean loss every N steps (s: 10, f: 20)")
    p.add_argument("--workers", type=int, default=8, help="decoding threads")
    p.add_argument("--cues", default=None, help="s: the localisation-cue pickle")
    p.add_argument("--class", dest="num_classes", type=int, default=21, metavar="N",
                   help="outputs of the classifiers, labels 0..N-1 (1..96; default 21, the reference's COCO variant has 81)")
    p.add_argument("--cue-maps", action="store_true",
                   help="s: --list holds 'image_path cue_path' lines (--root prefixed to both); a cue file is a 41 x 41 map of classes, "
                        "255 = no cue (AnnotationLayerCOCO's format); --cues is then absent")
    p.add_argument("--channel-order", choices=("bgr", "rgb"), default=None,
                   help="s with --cue-maps: the network input's channel order (default bgr, as predict and validate feed; rgb is "
                        "AnnotationLayerCOCO's own)")
    p.add_argument("--backbone", choices=("vgg16", "resnet101"), default=None, help="f: the network (default vgg16)")
    p.add_argument("--crop", type=int, default=None, help="f: crop size (321)")
    p.add_argument("--mean", default=None, help="f: B,G,R mean (104,117,123)")
    p.add_argument("--no-mirror", action="store_true", help="f: no random mirror")
    p.add_argument("--scale-factors", default=None,
                   help="f: rescale every image by one of these factors, drawn per image, before the crop, e.g. 0.5,0.75,1,1.25,1.5 "
                        "(bilinear for the image, nearest neighbour for the label, done on the GPU; default: none)")
    p.add_argument("--loss-at", choices=("map", "label"), default=None,
                   help="f: where the softmax loss is taken.  map (default): on the network's output map against the labels shrunk "
                        "by 8, as the reference does; label: the logits are zoomed to the label map and every label pixel is judged "
                        "(one fused HIP call), and the display line gains the pixel accuracy.  Not stored in snapshots: a resumed "
                        "run names it again")
    p.add_argument("--msc-scales", default=None,
                   help="f: DeepLab-v2's multi-scale inputs with max fusion, e.g. 0.75,0.5 (up to 3 extra scales, distinct, each > 0, <= 2 and not 1): "
                        "every step runs the network on the crop and on the crop zoomed by each scale, fuses the score maps by their "
                        "maximum and judges the fused map and every scale's own map (one fused HIP call); the display line names "
                        "the losses and gains the fused map's pixel accuracy.  Not stored in snapshots; not with --loss-at label")
    p.add_argument("--val-list", default=None, help="validate on these 'image_path label_path' lines (ground-truth label PNGs)")
    p.add_argument("--val-root", default=None, help="prefix of both paths of a --val-list line (default: --root)")
    p.add_argument("--val-every", type=int, default=None, help="validate every N steps (default: whenever a snapshot is written)")
    p.add_argument("--val-crop", type=int, default=None, help="every validation image is padded to this size (513)")
    p.add_argument("--val-batch", type=int, default=None, help="validation images per forward and rank (default: the per-rank batch)")
    p.add_argument("--val-result", default=None, help="file rewritten at each validation: meanIOU / per-class IoU / matrix")
    a = p.parse_args(argv)
    for key, value in STAGE_DEFAULTS[a.stage].items():
        if getattr(a, key) is None:
            setattr(a, key, value)
    if a.val_list is None:
        given = [o for o in ("val_root", "val_every", "val_crop", "val_batch", "val_result") if getattr(a, o) is not None]
        if given:
            p.error("%s need%s --val-list" % (", ".join("--" + o.replace("_", "-") for o in given), "s" if len(given) == 1 else ""))
    else:
        a.val_root = a.root if a.val_root is None else a.val_root
        a.val_every = a.snapshot_every if a.val_every is None else a.val_every
        a.val_crop = VAL_CROP if a.val_crop is None else a.val_crop
        if min(a.val_every, a.val_crop) < 1 or (a.val_batch is not None and not 1 <= a.val_batch <= 32):
            p.error("--val-every and --val-crop must be >= 1, --val-batch 1..32")
    from .input import MAX_CLASSES
    if not 1 <= a.num_classes <= MAX_CLASSES:
        p.error("--class takes 1..%d, got %d" % (MAX_CLASSES, a.num_classes))
    if a.cue_maps and a.stage != "s":
        p.error("--cue-maps is for --stage s")
    if a.channel_order is not None and not a.cue_maps:
        p.error("--channel-order needs --cue-maps")
    a.channel_order = a.channel_order or "bgr"
    if a.stage == "s":
        if a.cue_maps and a.cues:
            p.error("--cue-maps reads the cues from the files of --list: --cues must be absent")
        if not a.cues and not a.cue_maps:
            p.error("--stage s needs --cues (the localisation-cue pickle) or --cue-maps")
        if a.cues and a.num_classes != 21:
            p.error("--class %d: the cue pickle of --cues describes 21 classes; other class counts are fed by --cue-maps" % a.num_classes)
        if a.backbone or a.crop is not None or a.mean is not None or a.no_mirror or a.scale_factors is not None:
            p.error("--backbone, --crop, --mean, --no-mirror and --scale-factors are for --stage f")
        if a.loss_at is not None:
            p.error("--loss-at is for --stage f")
        if a.msc_scales is not None:
            p.error("--msc-scales is for --stage f")
    else:
        a.loss_at = a.loss_at or "map"
        if a.cues:
            p.error("--cues is for --stage s")
        a.backbone = a.backbone or "vgg16"
        a.crop = F_DEFAULTS["crop"] if a.crop is None else a.crop
        a.mean = F_DEFAULTS["mean"] if a.mean is None else tuple(float(v) for v in a.mean.split(","))
        if len(a.mean) != 3:
            p.error("--mean takes three values: B,G,R")
        if a.scale_factors is None:
            a.scale_factors = ()
        else:
            try:
                a.scale_factors = tuple(float(v) for v in a.scale_factors.split(","))
            except ValueError:
                p.error("--scale-factors takes numbers separated by commas, got %r" % a.scale_factors)
            if not all(0.0 < s < float("inf") for s in a.scale_factors):
                p.error("--scale-factors must be finite and > 0, got %r" % (a.scale_factors,))
        if a.msc_scales is None:
            a.msc_scales = ()
        else:
            if a.loss_at == "label":
                p.error("--msc-scales and --loss-at label do not combine")
            from .retrain import check_msc_scales
            try:
                a.msc_scales = check_msc_scales(a.msc_scales.split(","), a.crop)
            except ValueError as e:
                p.error("--msc-scales: %s" % e)
            if not a.msc_scales:
                p.error("--msc-scales takes numbers separated by commas")
    if min(a.iters, a.snapshot_every, a.batch, a.display, a.workers) < 1:
        p.error("--iters, --snapshot-every, --batch, --display and --workers must be >= 1")
    return a


def _process_group(torch):
    """(rank, world size, local rank); under a launcher the group is initialised here, one GPU per rank"""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size(), int(os.environ.get("LOCAL_RANK", torch.cuda.current_device()))
    if os.environ.get("RANK") is None:
        return 0, 1, torch.cuda.current_device()
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local_rank)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))        # nccl == RCCL on ROCm
    return dist.get_rank(), dist.get_world_size(), local_rank


def main(argv=None):
    a = parse_args(argv)
    import torch
    from ._lib import require_gpu
    from .input import TrainFInput, TrainSCueMapInput, TrainSInput
    from .trainer import DSRGTrainer, params_checksum

    require_gpu()
    rank, world, local_rank = _process_group(torch)
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    if a.batch % world:
        raise SystemExit("--batch %d is not a multiple of the %d ranks" % (a.batch, world))
    batch = a.batch // world
    say = print if rank == 0 else (lambda *args, **kw: None)

    if a.stage == "s":
        trainer = DSRGTrainer(device, world_size=world, seed=a.seed, weights=a.weights, snapshot=a.snapshot, num_classes=a.num_classes)
        if a.cue_maps:
            loader = TrainSCueMapInput(a.list, a.root, a.num_classes, batch_size=batch, size=321, mean=TrainSInput.mean,
                                       bgr=a.channel_order == "bgr", seed=a.seed, workers=a.workers, rank=rank, world_size=world,
                                       device=device)
        else:
            loader = TrainSInput(a.list, a.root, a.cues, batch_size=batch, seed=a.seed, workers=a.workers, rank=rank,
                                 world_size=world, device=device)
        names = ("loss-Seed", "loss-Constrain")
        rate = trainer.opt.lr
    else:
        from .retrain import RetrainTrainer, poly_lr
        trainer = RetrainTrainer(device, world_size=world, backbone=a.backbone, max_iter=a.iters, seed=a.seed, weights=a.weights,
                                 snapshot=a.snapshot, num_classes=a.num_classes, loss_at=a.loss_at, msc_scales=a.msc_scales)
        loader = TrainFInput(dict(source=a.list, root_folder=a.root, batch_size=batch, crop_size=(a.crop, a.crop), mean=a.mean,
                                  mirror=not a.no_mirror, scale_factors=a.scale_factors), seed=a.seed, workers=a.workers, rank=rank, world_size=world, device=device)
        names = ("loss",)
        if a.msc_scales:                                                 # (DeepLab's names: the fused head, the crop, every scale)
            names = ("loss", "loss-fusion", "loss-res1") + tuple("loss-res%g" % s for s in a.msc_scales)
        rate = lambda: poly_lr(trainer.base_lr, trainer.opt.iter, trainer.max_iter)      # noqa: E731
    if trainer.opt.iter:
        say("resumed from %s at iteration %d" % (a.snapshot, trainer.opt.iter), flush=True)

    validator = None
    if a.val_list is not None:
        from .validate import Validator, write_result
        validator = Validator(trainer.net, a.val_list, a.val_root, crop=a.val_crop, batch=val_batch(a, world),
                              mean=a.mean if a.stage == "f" else TrainSInput.mean, num_classes=a.num_classes, device=device, rank=rank, world_size=world,
                              amp_dtype=trainer.amp_dtype, workers=a.workers)

    # --loss-at label: the step adds to trainer.loss_counters on the device; they are read where the display step reads the losses
    counters = getattr(trainer, "loss_counters", None)
    seen = [0, 0, 0]                                                     # the counters at the last display line

    def accuracy_words():
        """', accuracy = ...' over the display window, summed over the ranks (and a warning line for invalid labels), or ''"""
        if counters is None:
            return ""
        import torch.distributed as dist
        now = counters.clone()
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dist.all_reduce(now, op=dist.ReduceOp.SUM)
        now = now.tolist()
        valid, correct, invalid = (n - s for n, s in zip(now, seen))
        seen[:] = now
        if invalid:
            say("warning: %d label pixels are neither a class below %d nor 255: they were left out of the loss" % (invalid, a.num_classes),
                flush=True)
        return ", accuracy = %.6f" % (correct / max(valid, 1))

    window, saved_at = [], None
    with loader:
        while trainer.opt.iter < a.iters:
            lr = rate()
            window.append(trainer.step(*next(loader)).detach().reshape(-1))
            it = trainer.opt.iter
            if it % a.display == 0 or it == a.iters:
                mean = DSRGTrainer.reduce_losses(trainer, torch.stack(window).mean(0)).tolist()
                tail = accuracy_words()
                say("Iteration %d, lr = %g, %s%s" % (it, lr, ", ".join("%s = %.6f" % nv for nv in zip(names, mean)), tail), flush=True)
                window = []
            if it % a.snapshot_every == 0 or it == a.iters:
                paths = trainer.save(a.prefix)                           # (collective: every rank calls it)
                saved_at = it
                say("snapshot %s %s" % paths, flush=True)
            if validator is not None and (it % a.val_every == 0 or it == a.iters):
                res = validator.run()                                    # (collective: every rank scores its share of the list)
                say("Iteration %d, validation: meanIOU = %.6f, pixel accuracy = %.6f (%d images)"
                    % (it, res["miou"], res["pixel_accuracy"], res["images"]), flush=True)
                if a.val_result and rank == 0:
                    write_result(a.val_result, res)
    if saved_at != trainer.opt.iter:                                     # (a run that had nothing left to do still leaves its model)
        say("snapshot %s %s" % trainer.save(a.prefix), flush=True)
    words = params_checksum(list(trainer.net.parameters()) + [b for g in trainer.opt.groups for b in g["bufs"]])
    say("done: iteration %d weights_checksum %d %d" % ((trainer.opt.iter,) + tuple(int(v) for v in words.cpu())), flush=True)
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and os.environ.get("RANK") is not None:
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
