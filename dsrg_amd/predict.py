"""`python -m dsrg_amd.predict`: the test runs of run.sh on a list of images, writing one label PNG per image.

  --mode ms    <-> training/tools/test-ms.py    (absolute sizes, default 241,321,401; pseudo labels)
  --mode ms-f  <-> training/tools/test-ms-f.py  (sizes relative to each image, default 0.75,1,1.25; the final test)
  --mode ms --scales 481 --class 81  <-> training/tools/test-coco.py:108-135 (single-scale COCO test).  Channel order: that script
               reads with pylab.imread (RGB) and swaps [2, 1, 0] (test-coco.py:101, 110), so it feeds B G R, as every mode here
               does.  The reference's COCO TRAINING layer feeds the other order (AnnotationLayerCOCO, pylayers.py:456, 489:
               cv2.imread gives BGR, the same swap makes it RGB).  `python -m dsrg_amd.train --stage s --cue-maps --class 81`
               feeds B G R by default, so a model trained here matches this command; one trained with --channel-order rgb (the
               layer's own order) would need RGB here, which this command does not offer
  --mode gt --cues PICKLE  <-> training/tools/generate_train_gt.py (one size, default 321; labels restricted to background + the
               image-level labels '<id>_labels' of the cue pickle; --images holds the reference's input_list.txt lines "name.jpg <id>")
  --mode gt-ms --cues PICKLE  (no counterpart in the reference) --mode gt as a probability ensemble over several sizes (default
               241,321,401; at most 8), with --flip each also on the mirror image: the zoomed softmax maps are averaged before the
               clamp (inference.predict_train_gt_ms_many).  One size without --flip is --mode gt

Reads DIR/JPEGImages/<id>.jpg for every id of --images, writes OUT/<id>.png: 8-bit grayscale class ids, what
training/tools/evaluate.py reads (and `python -m dsrg_amd.evaluate`).  The network is VGG16-ASPP (--backbone resnet101: the DeepLab-v2
ResNet-101 of the stage-2 trainer, run through resnet_test.ResNetTestNet: fused HIP stem, weights packed once) with the weights of --model
(checkpoint.load_weights: .caffemodel, .npz or a torch file), run under bf16 autocast (--fp32: float32, the reference's
precision); forwards replay from captured HIP graphs (inference.GraphedForward, bounded for the relative scales) while the
CRFs of earlier images are in flight (inference.predict_masks_ms_many / predict_masks_ms_f_many).  --mode ms --forward-batch N
takes the images N at a time through batch-N forwards (the absolute sizes are the same for every image); so do --mode gt and
--mode gt-ms (one generator, inference.predict_train_gt_ms_many).
--mode ms-f --same-size-batch N collects same-sized images (up to N, out of a window of
--window images) into batch-n forwards (inference.plan_size_groups); the masks are still written per image, in input order.
--flip (ms, ms-f, gt-ms; no counterpart in the reference): mirrored test-time augmentation, every scale runs on the image and on its
mirror image and all the score maps are summed before the softmax (gt-ms: the probabilities averaged) (at most 4 scales, batches of at most 8
images).

--gt DIR (all four modes) <-> the loop of training/tools/test-coco.py:138-173, run.sh steps 4 and 5 as one command: the label maps
stay on the device (masks="device" of the generators) and are scored there against DIR/<id>.png, 16 images per launch
(inference.MaskScorer, dsrg_score_labels_batch), under the rule of `python -m dsrg_amd.evaluate` (ground truth < --class kept).
--save_path FILE: the three-line result file evaluate writes; --score-every N (default 100): '<n> images, meanIOU = <v>' with one
synchronisation per N images (test-coco.py:150-157); the last line printed is 'meanIOU: <v>'.  The mean IoU in all three is
evaluate.py's (ConfusionMatrix.jaccard: the classes with a non-zero diagonal only), not test-coco.py's own tp / max(1, pos + res - tp)
averaged over all classes.  --output is optional with --gt: without it only the ground truth goes up and the counters come down,
with it the PNGs are written from the scorer's uint8 masks.  A ground truth whose size differs from its image's stops the run with an
error that names the id.  Without --gt everything runs as before.  --image-subdir NAME: the folder under --dir that holds the images
(default JPEGImages; test-coco.py reads images/val2014).
"""
import argparse
import os
import sys


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="multi-scale test: label PNGs for a list of images")
    p.add_argument("--mode", choices=("ms", "ms-f", "gt", "gt-ms"), required=True,
                   help="ms: absolute sizes (test-ms.py); ms-f: sizes relative to each image (test-ms-f.py); "
                        "gt: pseudo labels restricted to the image-level labels (generate_train_gt.py); gt-ms: gt as a "
                        "probability ensemble over several sizes (and their mirrors with --flip)")
    p.add_argument("--model", required=True, help="weights (.caffemodel, .npz or torch file)")
    p.add_argument("--images", required=True, help="list of image ids, one per line (gt: lines 'name.jpg <id>')")
    p.add_argument("--cues", default=None, help="gt, gt-ms: the localisation-cue pickle holding '<id>_labels' for every image")
    p.add_argument("--dir", required=True, help="dataset root holding the image folder (--image-subdir)")
    p.add_argument("--image-subdir", default="JPEGImages",
                   help="the folder under --dir that holds <id>.jpg (default JPEGImages; test-coco.py reads images/val2014)")
    p.add_argument("--output", default=None, help="directory for the <id>.png label maps (optional with --gt)")
    p.add_argument("--gt", default=None,
                   help="directory of ground-truth label PNGs <id>.png: score the label maps against them on the GPU as they are made "
                        "(all four modes; ground truth < --class is kept, as `python -m dsrg_amd.evaluate` keeps it) and print "
                        "'meanIOU: <v>'.  The mean IoU is evaluate.py's (ConfusionMatrix.jaccard): the mean over the classes with a "
                        "non-zero diagonal only — NOT test-coco.py's own tp / max(1, pos + res - tp) averaged over all classes")
    p.add_argument("--save_path", default=None, help="with --gt: the three-line result file `python -m dsrg_amd.evaluate` writes")
    p.add_argument("--score-every", type=int, default=None,
                   help="with --gt: print '<n> images, meanIOU = <v>' (the same mean IoU) every N images, one synchronisation each "
                        "(default 100; at least 1)")
    p.add_argument("--smooth", action="store_true", help="dense-CRF post-processing (as the reference's --smooth)")
    p.add_argument("--scales", default=None,
                   help="comma-separated: sizes in pixels (ms; default 241,321,401) or factors (ms-f; default 0.75,1,1.25); "
                        "gt: one size (default 321); gt-ms: up to 8 sizes (default 241,321,401)")
    p.add_argument("--class", dest="num_classes", type=int, default=21, help="number of classes including background")
    p.add_argument("--fp32", action="store_true", help="float32 forwards instead of bf16 autocast")
    p.add_argument("--backbone", choices=("vgg16", "resnet101"), default="vgg16",
                   help="the network of --model: vgg16 (VGG16-ASPP, the default) or resnet101 (DeepLab-v2 ResNet-101, the model of "
                        "`python -m dsrg_amd.train --stage f --backbone resnet101`)")
    p.add_argument("--in-flight", type=int, default=3, help="CRFs in flight under the next image's forwards")
    p.add_argument("--max-graphs", type=int, default=12, help="ms-f: captured forward graphs kept (least recently used dropped)")
    p.add_argument("--forward-batch", type=int, default=1,
                   help="ms, gt, gt-ms: images per batched forward (1..16; default 1: one image per forward)")
    p.add_argument("--same-size-batch", type=int, default=1,
                   help="ms-f: same-sized images per batched forward (1..16; default 1: one image per forward)")
    p.add_argument("--window", type=int, default=64,
                   help="ms-f with --same-size-batch: an image waits for at most N - 1 later images for its group (default 64)")
    p.add_argument("--flip", action="store_true",
                   help="ms, ms-f, gt-ms: mirrored test-time augmentation: every scale also runs on the mirror image, whose scores are "
                        "mirrored back and summed with the others (at most 4 scales; --forward-batch / --same-size-batch at most 8)")
    a = p.parse_args(argv)
    if a.gt is None:
        if a.output is None:
            p.error("--output is required without --gt")
        if a.save_path is not None or a.score_every is not None:
            p.error("--save_path and --score-every go with --gt")
    else:
        if a.score_every is None:
            a.score_every = 100
        if a.score_every < 1:
            p.error("--score-every must be at least 1")
    if a.mode in ("gt", "gt-ms"):
        if not a.cues:
            p.error("--mode %s needs --cues (the pickle with the image-level labels)" % a.mode)
        if a.mode == "gt" and a.scales is not None and len(a.scales.split(",")) != 1:
            p.error("--mode gt takes one size in --scales")
        if a.mode == "gt-ms" and a.scales is not None and len(a.scales.split(",")) > 8:
            p.error("--mode gt-ms takes at most 8 sizes in --scales")
    elif a.cues:
        p.error("--cues is for --mode gt and --mode gt-ms only")
    if a.mode == "ms-f" and a.forward_batch != 1:
        p.error("--forward-batch is for --mode ms only: the relative scales of ms-f give every image size its own input shapes")
    if not 1 <= a.forward_batch <= 16:
        p.error("--forward-batch must be 1..16")
    if a.mode != "ms-f" and (a.same_size_batch != 1 or a.window != 64):
        p.error("--same-size-batch and --window are for --mode ms-f only")
    if not 1 <= a.same_size_batch <= 16:
        p.error("--same-size-batch must be 1..16")
    if a.window < 1:
        p.error("--window must be at least 1")
    if a.flip:
        if a.mode == "gt":
            p.error("--flip is for --mode ms and --mode ms-f only: the softmax-before-zoom tail of --mode gt has no mirror form")
        if a.forward_batch > 8 or a.same_size_batch > 8:
            p.error("--flip takes --forward-batch / --same-size-batch of at most 8: every image fills two slots of a batch")
        if a.scales is not None and len(a.scales.split(",")) > 4:
            p.error("--flip takes at most 4 scales: every scale runs twice")
    return a


def read_ids(path):
    return [l.strip() for l in open(path) if l.strip()]


def read_gt_list(path):
    """the lines of the reference's input_list.txt, 'name.jpg <id>' (generate_train_gt.py:117-122) -> [(name without extension, id)]"""
    out = []
    for line in open(path):
        parts = line.strip().split()
        if parts:
            if len(parts) < 2:
                raise ValueError("%s: expected 'name.jpg <id>', got %r" % (path, line.strip()))
            out.append((os.path.splitext(parts[0])[0], int(parts[1])))
    return out


def read_image(path):
    """(H,W,3) RGB uint8, as pylab.imread gives a JPEG"""
    import numpy as np
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"))


def write_mask(path, mask):
    import numpy as np
    from PIL import Image
    Image.fromarray(np.asarray(mask).astype(np.uint8), mode="L").save(path)


def score_masks(a, ids, masks, device):
    """--gt: the loop of test-coco.py:138-173 with the label maps left on the device.  masks: a generator of (H,W) int32 CUDA label
    maps (masks="device") in the order of ids.  They are collected 16 at a time (and whenever a progress line is due) and scored
    against GT/<id>.png by inference.MaskScorer under evaluate's rule; with --output the PNGs are written from the scorer's uint8
    masks.  -> (images, the result dict of validate.result_from_counts)"""
    from . import inference as I
    from .evaluate import read_label_png
    scorer = I.MaskScorer(a.num_classes, device, rule_lt=True, want_masks=a.output is not None)
    held, n = [], 0                                         # (id, label map, ground truth) of the open group

    def flush():
        if not held:
            return
        narrowed = scorer.add([lab for _, lab, _ in held], [gt for _, _, gt in held])
        for (img_id, _, _), mask in zip(held, narrowed or ()):
            write_mask(os.path.join(a.output, img_id + ".png"), mask)
        del held[:]

    for img_id, lab in zip(ids, masks):
        gt = read_label_png(os.path.join(a.gt, img_id + ".png"))
        if tuple(gt.shape) != tuple(lab.shape):
            raise ValueError("%s: the ground truth is %d x %d, the image %d x %d" % ((img_id,) + tuple(gt.shape) + tuple(lab.shape)))
        held.append((img_id, lab, gt))
        n += 1
        due = n % a.score_every == 0
        if due or len(held) == I.MAX_SCORE_GROUP:
            flush()
        if due:                                             # (test-coco.py:150-157; one synchronisation)
            print("%d images, meanIOU = %s" % (n, scorer.result(n)["miou"]), flush=True)
    flush()
    return n, scorer.result(n)


def main(argv=None, net=None):
    """net (tools): a network of --backbone / --class already on the device in eval mode, used instead of loading --model"""
    a = parse_args(argv)
    import torch
    from . import inference as I
    from .backbone import VGG16ASPP
    from .checkpoint import load_weights
    from ._lib import require_gpu

    require_gpu()
    if a.mode in ("gt", "gt-ms"):
        from .layers import _open_cue_file
        cues = _open_cue_file(os.path.abspath(a.cues))
    if a.mode == "gt":
        scales = (int(a.scales),) if a.scales else (321,)
    elif a.mode in ("ms", "gt-ms"):
        scales = tuple(int(s) for s in a.scales.split(",")) if a.scales else (241, 321, 401)
    else:
        scales = tuple(float(s) for s in a.scales.split(",")) if a.scales else (0.75, 1.0, 1.25)
    dev = torch.device("cuda", torch.cuda.current_device())
    if net is not None:
        pass
    elif a.backbone == "resnet101":
        from .retrain import ResNet101DeepLab
        net = ResNet101DeepLab(num_classes=a.num_classes).to(dev).to(memory_format=torch.channels_last).eval()
        load_weights(net, a.model)
        if not a.fp32:                                      # the packed test-time path is bf16 by contract; float32 runs the module itself
            from .resnet_test import ResNetTestNet
            net = ResNetTestNet(net)                        # packs the loaded weights once
    else:
        net = VGG16ASPP(num_classes=a.num_classes).to(dev).to(memory_format=torch.channels_last).eval()
        load_weights(net, a.model)
    if a.mode in ("gt", "gt-ms"):
        entries = read_gt_list(a.images)
        ids = [name for name, _ in entries]
        gt_labels = [cues['%i_labels' % num] for _, num in entries]
    else:
        ids = read_ids(a.images)
    if a.output is not None:
        os.makedirs(a.output, exist_ok=True)
    images = (read_image(os.path.join(a.dir, a.image_subdir, i + ".jpg")) for i in ids)
    how = {} if a.gt is None else {"masks": "device"}       # scored: the label maps stay on the device

    if a.mode in ("ms", "gt", "gt-ms"):
        fwd = I.GraphedForward(net)                         # one graph per fixed size
    else:                                                   # every image size has its own shapes: keep the common ones
        fwd = I.GraphedForward(net, max_shapes=a.max_graphs, capture_after=2)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=not a.fp32):
        if a.mode in ("gt", "gt-ms"):                       # gt: its one size, no flip (what predict_train_gt_many is)
            masks = I.predict_train_gt_ms_many(net, zip(images, gt_labels), sizes=scales, flip=a.flip, smooth=a.smooth, device=dev,
                                               forward=fwd, in_flight=a.in_flight, forward_batch=a.forward_batch, **how)
        elif a.mode == "ms":
            masks = I.predict_masks_ms_many(net, images, sizes=scales, device=dev, forward=fwd, in_flight=a.in_flight,
                                            forward_batch=a.forward_batch, flip=a.flip, smooth=a.smooth, **how)
        else:
            from .crf import MAX_BATCH
            masks = I.predict_masks_ms_f_many(net, images, scales=scales, device=dev, forward=fwd, in_flight=a.in_flight,
                                              batch=min(a.same_size_batch, MAX_BATCH), same_size_batch=a.same_size_batch,
                                              window=a.window, smooth=a.smooth, flip=a.flip, **how)
        if a.gt is not None:
            try:
                n, result = score_masks(a, ids, masks, dev)
            finally:
                masks.close()                               # (a run stopped by an error: the CRF workers end before it is reported)
            if a.save_path is not None:
                from .validate import write_result
                write_result(a.save_path, result)
            if a.output is not None:
                print("wrote %d masks to %s" % (n, a.output))
            print("meanIOU: %s" % float(result["miou"]))
            return 0
        n = 0
        for img_id, mask in zip(ids, masks):
            write_mask(os.path.join(a.output, img_id + ".png"), mask)
            n += 1
            if n % 100 == 0:
                print("%d %s" % (n, img_id), flush=True)
    print("wrote %d masks to %s" % (n, a.output))
    return 0


if __name__ == "__main__":
    sys.exit(main())
