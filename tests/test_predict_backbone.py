"""`python -m dsrg_amd.predict --backbone {vgg16,resnet101}`: the option's parsing (no GPU), and the command itself on a seeded
ResNet-101 in a child process: label PNGs of the images' sizes, the same bytes from a second run."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

gpu = pytest.mark.gpu
COMMON = ["--model", "m.pth", "--images", "ids.txt", "--dir", "d", "--output", "o"]


@pytest.mark.parametrize("mode", ["ms", "ms-f", "gt"])
def test_backbone_option_in_every_mode(mode):
    from dsrg_amd.predict import parse_args
    extra = ["--cues", "cues.pickle"] if mode == "gt" else []
    assert parse_args(["--mode", mode] + COMMON + extra).backbone == "vgg16"                       # the default
    assert parse_args(["--mode", mode, "--backbone", "resnet101"] + COMMON + extra).backbone == "resnet101"
    assert parse_args(["--mode", mode, "--backbone", "vgg16"] + COMMON + extra).backbone == "vgg16"


def test_backbone_option_rejects_other_values(capsys):
    from dsrg_amd.predict import parse_args
    for bad in ("resnet50", "ResNet101", ""):
        with pytest.raises(SystemExit):
            parse_args(["--mode", "ms", "--backbone", bad] + COMMON)
    assert "--backbone" in capsys.readouterr().err


@gpu
def test_predict_command_runs_a_resnet_model(tmp_path):
    import torch
    from PIL import Image
    from dsrg_amd.retrain import ResNet101DeepLab
    torch.manual_seed(3)
    net = ResNet101DeepLab(num_classes=21)
    with torch.no_grad():
        for m in net.aspp:                                       # scores that differ between classes
            m.weight.normal_(0, 0.05)
            m.bias.normal_(0, 1.0)
    model = str(tmp_path / "model-f.pth")
    torch.save({k: v.detach().cpu() for k, v in net.state_dict().items()}, model)
    os.makedirs(str(tmp_path / "JPEGImages"))
    rng = np.random.default_rng(0)
    sizes = {"a": (64, 48), "b": (48, 64)}                       # width x height
    for name, (wd, ht) in sizes.items():
        yy, xx = np.mgrid[0:ht, 0:wd]
        img = np.stack([(yy * 5) % 256, (xx * 4) % 256, ((yy + 2 * xx) * 3) % 256], -1) + rng.integers(-8, 9, (ht, wd, 3))
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(str(tmp_path / "JPEGImages" / (name + ".jpg")), quality=95)
    ids = str(tmp_path / "ids.txt")
    with open(ids, "w") as f:
        f.write("a\nb\n")

    def run(out):
        cmd = [sys.executable, "-m", "dsrg_amd.predict", "--mode", "ms", "--backbone", "resnet101", "--model", model, "--images", ids,
               "--dir", str(tmp_path), "--output", out, "--scales", "65,97", "--smooth"]
        r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
        assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
        got = {}
        for name, (wd, ht) in sizes.items():
            path = os.path.join(out, name + ".png")
            with Image.open(path) as im:
                assert im.mode == "L" and im.size == (wd, ht)
                assert np.asarray(im).max() < 21
            got[name] = open(path, "rb").read()
        return got
    first = run(str(tmp_path / "out1"))
    assert run(str(tmp_path / "out2")) == first
