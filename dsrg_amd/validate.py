"""Validation against ground truth: one single-scale, padded pass over a list of image / label pairs, scored on the GPU.

  ValInput   one ordered pass over 'image_path label_path' lines (the format of list/train.txt): every image at the top left
             corner of a crop x crop window, labels `ignore_label` off the image — no mirror, no shuffle, no rescaling, no random
             draw; built on input._StagedLoader and ops.train_f_input_batch
  Validator  net -> {miou, iou, pixel_accuracy, images, matrix}: each batch is forwarded once and its scores go to
             ops.eval_confusion_batch (dsrg_eval_confusion_batch: zoom to the crop, argmax and confusion counters in one launch);
             nothing but the nclass*nclass + 1 counters is written, and the host waits once, at the end
  `python -m dsrg_amd.validate --model M --list L --root R --save_path FILE`: that pass as a command, written in the three-line
             format of `python -m dsrg_amd.evaluate` (training/tools/evaluate.py:151-157)

The pixels kept are those whose ground truth is < num_classes (ConfusionMatrix.generateM, the rule of evaluate.py's main): VOC's
255 border and everything off the image are dropped.  The prediction of a pixel is the first maximum of the score maps zoomed to
the crop with the arithmetic of ops.multiscale_unary at one scale.  This is NOT the multi-scale test with the CRF of run.sh (`python
-m dsrg_amd.predict` + `python -m dsrg_amd.evaluate`): it is the number a run can afford every few thousand iterations.

`python -m dsrg_amd.train --val-list ...` runs a Validator on the trainer's own network between two steps.  The pass draws from no
random generator (eval mode: Dropout is the identity), runs under torch.no_grad(), touches no gradient, momentum buffer or
parameter, and restores the network's training mode.
"""
import argparse
import sys

import numpy as np
import torch

from .input import _PairLoader, _StagedLoader, image_size, read_list


def read_val_list(path):
    """'image_path label_path' lines -> [(image_path, label_path)]"""
    return read_list(path, "image_path label_path", "image / label pair")


class ValInput(_PairLoader):
    """Iterator of (data (n,3,crop,crop), label (n,1,crop,crop)) float32 device tensors, n = batch_size but for a shorter last
    batch: ONE pass over this rank's share — items rank, rank + world_size, ... — of list_file, in list order.  Every listed image
    is returned exactly once over the ranks, whatever the batch and world sizes.  An image lies at top = left = 0 of its window,
    unmirrored and unscaled; data is 0 and label is ignore_label off it.  An image larger than the crop raises ValueError naming
    the file when its batch is planned (the size comes from the label file's header), before anything is decoded or uploaded.
    The tensors of a batch are valid until the __next__ call after next (_StagedLoader)."""

    def __init__(self, list_file, root, crop=513, batch_size=10, mean=(104.0, 117.0, 123.0), ignore_label=255, workers=8, rank=0,
                 world_size=1, device=None):
        _StagedLoader.__init__(self, batch_size, workers, device)
        self.crop = (int(crop), int(crop))
        if self.crop[0] < 1:
            raise ValueError("crop %r" % (crop,))
        if not 0 <= rank < world_size:
            raise ValueError("rank %d outside world size %d" % (rank, world_size))
        self.mean = tuple(float(np.float32(m)) for m in mean)
        self.ignore_label = ignore_label
        self.entries = [(root + i, root + l) for i, l in read_val_list(list_file)]
        self.items = self.entries[rank::world_size]          # (a rank beyond the end of a short list has nothing to score)
        self._planned = 0

    def plan_batch(self):
        """the next batch's items, [] once the pass is over"""
        plan = []
        for image_path, label_path in self.items[self._planned:self._planned + self.batch_size]:
            H, W = image_size(label_path)
            if H > self.crop[0] or W > self.crop[1]:
                raise ValueError("%s is %d x %d: larger than the %d x %d validation crop" % ((label_path, H, W) + self.crop))
            plan.append(dict(image=image_path, label=label_path, top=0, left=0, mirror=False))
        self._planned += len(plan)
        return plan

    def _assemble(self, slot):
        from . import ops
        n = slot.count                                       # a short last batch fills the first n slices of the slot's tensors
        return ops.train_f_input_batch(slot.dev, slot.desc, self.crop, self.mean, 1.0, self.ignore_label,
                                       out=(slot.outputs[0][:n], slot.outputs[1][:n]), nbytes=slot.nbytes)


def reduce_counts(hist):
    """the sum of an integer tensor over the ranks of the default process group (one all_reduce; CPU tensors under gloo, device
    tensors under nccl); outside a group, or in a group of one, the tensor itself.  Collective: every rank calls it."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return hist
    out = hist.detach().clone()
    dist.all_reduce(out, op=dist.ReduceOp.SUM)
    return out


def result_from_counts(counts, num_classes, images):
    """nclass*nclass + 1 counters -> the dict Validator.run returns"""
    from .inference import ConfusionMatrix
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    cm = ConfusionMatrix(num_classes)
    cm.add_counts(counts)
    with np.errstate(divide="ignore", invalid="ignore"):
        miou, per, M = cm.jaccard()
        acc = float(np.trace(M) / np.sum(M))
    return dict(miou=float(miou), iou=[float(j) for j in per], pixel_accuracy=acc, images=int(images), matrix=M, counts=counts)


def write_result(path, result):
    """the reference's three-line result file (evaluate.py:151-157), as dsrg_amd.evaluate writes it"""
    with open(path, "w") as f:
        f.write("meanIOU: " + str(float(result["miou"])) + "\n")
        f.write(str([float(j) for j in result["iou"]]) + "\n")
        f.write(str(result["matrix"]) + "\n")


class Validator(object):
    """run() -> dict(miou, iou, pixel_accuracy, images, matrix, counts) of `net` over list_file ('image_path label_path' lines, root
    prefixed to both): miou / iou / matrix as ConfusionMatrix.jaccard returns them, counts the nclass*nclass + 1 integer counters.
    Rank r of world_size scores items r, r + world_size, ...; with a process group initialised the counters are summed over the
    ranks (one all_reduce), so every rank returns the whole list's result and run() is collective."""

    def __init__(self, net, list_file, root, crop=513, batch=10, mean=(104.0, 117.0, 123.0), num_classes=21, device=None, rank=0,
                 world_size=1, amp_dtype=torch.bfloat16, ignore_label=255, workers=8):
        self.net, self.list_file, self.root = net, list_file, root
        self.crop, self.batch, self.mean, self.num_classes = int(crop), int(batch), tuple(mean), int(num_classes)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.rank, self.world_size = int(rank), int(world_size)
        self.amp_dtype = amp_dtype                           # None: float32 forwards
        self.ignore_label, self.workers = ignore_label, int(workers)

    def loader(self):
        return ValInput(self.list_file, self.root, crop=self.crop, batch_size=self.batch, mean=self.mean,
                        ignore_label=self.ignore_label, workers=self.workers, rank=self.rank, world_size=self.world_size,
                        device=self.device)

    def run(self):
        from . import ops
        C = self.num_classes
        net = self.net
        was_training = net.training
        net.eval()
        images = 0
        try:
            with torch.cuda.device(self.device), torch.no_grad():
                hist = torch.zeros(C * C + 1, dtype=torch.int64, device=self.device)
                with self.loader() as loader, torch.autocast("cuda", dtype=self.amp_dtype, enabled=self.amp_dtype is not None):
                    for data, label in loader:
                        scores = net(data.contiguous(memory_format=torch.channels_last)).float().contiguous()
                        # generateM's rule, the one of evaluate.py's main: ground truth < C is kept
                        ops.eval_confusion_batch(scores, label, C, self.ignore_label, rule_lt=True, hist=hist)
                        images += data.shape[0]
                packed = torch.cat([hist, torch.tensor([images], dtype=torch.int64, device=self.device)])
                torch.cuda.synchronize(self.device)
        finally:
            net.train(was_training)
        packed = reduce_counts(packed).cpu().numpy()
        return result_from_counts(packed[:-1], C, packed[-1])


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="python -m dsrg_amd.validate",
                                description="single-scale padded evaluation of a model against ground truth, scored on the GPU")
    p.add_argument("--model", required=True, help="weights (.caffemodel, .npz or torch file)")
    p.add_argument("--list", required=True, help="'image_path label_path' lines")
    p.add_argument("--root", required=True, help="prefix of both paths of a list line")
    p.add_argument("--backbone", choices=("vgg16", "resnet101"), default="vgg16", help="the network of --model")
    p.add_argument("--class", dest="num_classes", type=int, default=21, help="number of classes including background")
    p.add_argument("--crop", type=int, default=513, help="every image is padded to crop x crop (no image may be larger)")
    p.add_argument("--batch", type=int, default=10, help="images per forward")
    p.add_argument("--fp32", action="store_true", help="float32 forwards instead of bf16 autocast")
    p.add_argument("--save_path", required=True, help="result file path")
    a = p.parse_args(argv)
    if a.crop < 1 or a.batch < 1 or a.num_classes < 1:
        p.error("--crop, --batch and --class must be >= 1")
    return a


def main(argv=None):
    a = parse_args(argv)
    from ._lib import require_gpu
    from .checkpoint import load_weights

    require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    if a.backbone == "resnet101":
        from .retrain import ResNet101DeepLab
        net = ResNet101DeepLab(num_classes=a.num_classes).to(dev).to(memory_format=torch.channels_last).eval()
        load_weights(net, a.model)
        if not a.fp32:                                      # (as predict.py: the packed test-time path is bf16 by contract)
            from .resnet_test import ResNetTestNet
            net = ResNetTestNet(net)
    else:
        from .backbone import VGG16ASPP
        net = VGG16ASPP(num_classes=a.num_classes).to(dev).to(memory_format=torch.channels_last).eval()
        load_weights(net, a.model)
    result = Validator(net, a.list, a.root, crop=a.crop, batch=a.batch, num_classes=a.num_classes, device=dev,
                       amp_dtype=None if a.fp32 else torch.bfloat16).run()
    write_result(a.save_path, result)
    print("meanIOU: %s" % float(result["miou"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
