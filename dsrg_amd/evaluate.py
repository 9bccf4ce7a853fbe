"""`python -m dsrg_amd.evaluate` <-> training/tools/evaluate.py:132-162: the confusion matrix of a folder of predicted label PNGs
against the ground-truth PNGs (ConfusionMatrix.generateM per image: ground truth < class_num kept), and the mean IoU written in
the reference's three-line format (meanIOU: <v> / per-class IoU list / matrix).  CPU only.

PNGs are read as 8-bit label maps: a grayscale or palette PNG gives its stored values (the class ids; a palette PNG as in VOC's
SegmentationClass gives its indices), any other mode is converted to grayscale first.
"""
import argparse
import os
import sys


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="evaluate segmentation result")
    p.add_argument("--pred", dest="pred_dir", required=True, help="prediction result dir")
    p.add_argument("--gt", dest="gt_dir", required=True, help="ground truth dir")
    p.add_argument("--test_ids", required=True, help="test ids file path")
    p.add_argument("--save_path", required=True, help="result file path")
    p.add_argument("--class_num", type=int, default=21, help="class number include bg")
    return p.parse_args(argv)


def read_label_png(path):
    import numpy as np
    from PIL import Image
    with Image.open(path) as im:
        if im.mode not in ("L", "P"):
            im = im.convert("L")
        return np.array(im, dtype=np.uint8)


def evaluate(pred_dir, gt_dir, ids, class_num):
    """-> (mean IoU, per-class IoU list, matrix) of inference.ConfusionMatrix.jaccard"""
    from .inference import ConfusionMatrix
    cm = ConfusionMatrix(class_num)
    for index, img_id in enumerate(ids):
        if index % 100 == 0:
            print("%d processd" % index)
        gt = read_label_png(os.path.join(gt_dir, img_id + ".png"))
        pred = read_label_png(os.path.join(pred_dir, img_id + ".png"))
        cm.addM(cm.generateM((gt.flatten(), pred.flatten())))
    return cm.jaccard()


def main(argv=None):
    a = parse_args(argv)
    ids = [i.strip() for i in open(a.test_ids) if i.strip()]
    aveJ, j_list, M = evaluate(a.pred_dir, a.gt_dir, ids, a.class_num)
    with open(a.save_path, "w") as f:
        f.write("meanIOU: " + str(float(aveJ)) + "\n")
        f.write(str([float(j) for j in j_list]) + "\n")
        f.write(str(M) + "\n")
    print("meanIOU: %s" % float(aveJ))
    return 0


if __name__ == "__main__":
    sys.exit(main())
