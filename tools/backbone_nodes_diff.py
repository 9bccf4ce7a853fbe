"""Do the backbone's autograd nodes (dsrg_amd/backbone.py, dsrg_amd/retrain.py) compute the same bits in two trees?

    python tools/backbone_nodes_diff.py dump DIR                      # in each tree, a fresh process per dump
    python tools/backbone_nodes_diff.py compare DIR_A DIR_B [--rerun DIR_A2] [--out FILE]

dump: with fixed seeds, one forward + backward per configuration; scores, loss, input gradient (where the input takes one) and every
parameter gradient go to DIR/<configuration>.pt:
  a  VGG16ASPP, train mode with Dropout, bf16 autocast, 4 x 3 x 161 x 161      b  a with _FUSE_CHAIN = False
  c  a with _IGEMM = False                                                      d  a in float32 without autocast, batch 1
  e  one eval forward, batch 1, bf16 autocast
  f  three retrain._Bottleneck blocks in a row (a projection block, two identity blocks), bf16, 2 x 512 x 33 x 33
  g1..g4  the 3x3 GemmConv2d chains of tests/test_gpu_igemm.py, fused and separate
compare: every array of DIR_B against DIR_A with torch.equal.  --rerun names a second dump of tree A: an array that differs between
A's own two runs is listed with that difference, and B is held to it for that array only.  Exit status 1 if anything else differs."""
import argparse
import os
import sys

os.environ.setdefault("MIOPEN_FIND_MODE", "2")        # as tests/conftest.py: MIOpen's heuristic pick, no ~50 s search per new shape

import torch                                           # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CL = torch.channels_last


def _step(net, x, amp, seed=11, train=True):
    """-> {name: CPU tensor} of one forward (+ backward when train) of net on x"""
    net.zero_grad(set_to_none=True)
    x.grad = None
    torch.manual_seed(seed)                                              # Dropout: the seeds come from torch's generators
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp), torch.set_grad_enabled(train):
        y = net(x)
    out = {"scores": y.detach()}
    if train:
        gout = torch.randn(y.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed + 1)).to(y.dtype)
        loss = (y.float() * gout.float()).sum()
        loss.backward()
        out["loss"] = loss.detach()
        if x.grad is not None:
            out["grad.input"] = x.grad
        out.update({"grad." + n: p.grad for n, p in net.named_parameters() if p.grad is not None})
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in out.items()}


def _configurations():
    """yields (name, arrays)"""
    from dsrg_amd import backbone, retrain
    torch.manual_seed(5)
    net = backbone.VGG16ASPP(dropout=0.5).cuda().to(memory_format=CL).train()
    x = torch.randn(4, 3, 161, 161, device="cuda").contiguous(memory_format=CL)
    yield "a", _step(net, x, True)
    try:
        backbone._FUSE_CHAIN = False
        yield "b", _step(net, x, True)
    finally:
        backbone._FUSE_CHAIN = True
    try:
        backbone._IGEMM = False
        yield "c", _step(net, x, True)
    finally:
        backbone._IGEMM = True
    yield "d", _step(net, x[:1].contiguous(memory_format=CL), False)
    yield "e", _step(net.eval(), x[:1].contiguous(memory_format=CL), True, train=False)
    del net

    torch.manual_seed(6)
    blocks = torch.nn.Sequential(retrain._Bottleneck(512, 256, 1, 2, down=True, train_bn_affine=False),
                                 retrain._Bottleneck(1024, 256, 1, 2, down=False, train_bn_affine=False),
                                 retrain._Bottleneck(1024, 256, 1, 2, down=False, train_bn_affine=False))
    with torch.no_grad():
        for m in blocks.modules():
            if isinstance(m, retrain._FrozenBN):                         # a frozen map that is not the identity
                m.weight.uniform_(0.5, 1.5); m.bias.normal_(0.0, 0.1); m.running_mean.normal_(0.0, 0.1); m.running_var.uniform_(0.5, 1.5)
    blocks = blocks.cuda().to(memory_format=CL).train()
    xb = torch.randn(2, 512, 33, 33, device="cuda").bfloat16().contiguous(memory_format=CL).requires_grad_(True)
    yield "f", _step(blocks, xb, True)
    del blocks

    G = backbone.GemmConv2d
    for i, (widths, size) in enumerate([((256, 256, 512, 256), 41), ((64, 64, 64), 97), ((64, 128, 128), 50), ((128, 128, 64, 64), 33)]):
        torch.manual_seed(5)
        wide = widths[0] >= 256                                          # implicit-GEMM route (dilation on the middle layer) / direct kernels
        chain = torch.nn.Sequential(*[G(a, b, 3, padding=2 if (wide and j == 1) else 1, dilation=2 if (wide and j == 1) else 1,
                                        fuse_relu=True, chain_input=j > 0)
                                      for j, (a, b) in enumerate(zip(widths[:-1], widths[1:]))]).cuda().to(memory_format=CL)
        xc = torch.randn(4, widths[0], size, size, device="cuda").contiguous(memory_format=CL).requires_grad_(True)
        try:
            for tag, on in (("fused", True), ("separate", False)):
                backbone._FUSE_CHAIN = on
                yield "g%d.%s" % (i + 1, tag), _step(chain, xc, True)
        finally:
            backbone._FUSE_CHAIN = True


def dump(directory):
    os.makedirs(directory, exist_ok=True)
    for name, arrays in _configurations():
        torch.save(arrays, os.path.join(directory, name + ".pt"))
        print("dumped %-12s %3d arrays" % (name, len(arrays)), flush=True)


def _distance(a, b):
    """None where torch.equal, else a description of the difference"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return "%s %s against %s %s" % (a.dtype, tuple(a.shape), b.dtype, tuple(b.shape))
    if torch.equal(a, b):
        return None
    return float((a.double() - b.double()).abs().max())                  # (nan where either holds one)


def compare(dir_a, dir_b, rerun, out):
    lines, bad, noisy = [], 0, 0
    names = sorted(set(os.listdir(dir_a)) | set(os.listdir(dir_b)))
    for f in names:
        if not (os.path.exists(os.path.join(dir_a, f)) and os.path.exists(os.path.join(dir_b, f))):
            lines.append("MISSING   %s in one of the two dumps" % f)
            bad += 1
            continue
        a, b = torch.load(os.path.join(dir_a, f)), torch.load(os.path.join(dir_b, f))
        a2 = torch.load(os.path.join(rerun, f)) if rerun else None
        for key in sorted(set(a) | set(b)):
            what = "%s:%s" % (f[:-3], key)
            if key not in a or key not in b:
                lines.append("MISSING   %s in one of the two dumps" % what)
                bad += 1
                continue
            d = _distance(a[key], b[key])
            own = _distance(a[key], a2[key]) if a2 is not None else None
            shape = "%s %s" % (str(a[key].dtype).replace("torch.", ""), tuple(a[key].shape))
            if own is not None:
                noisy += 1
                within = d is None or (isinstance(d, float) and isinstance(own, float) and d <= own)
                lines.append("%s %-52s %s  A's two runs differ by %s, B from A by %s" % ("noisy    " if within else "DIFFERENT", what, shape, own, d))
                bad += 0 if within else 1
            elif d is not None:
                lines.append("DIFFERENT %-52s %s  max |A - B| = %s" % (what, shape, d))
                bad += 1
            else:
                lines.append("identical %-52s %s" % (what, shape))
    lines.append("# %d arrays, %d differ beyond A's own run-to-run difference, %d differ between A's two runs" % (
        sum(1 for ln in lines if not ln.startswith("MISSING")), bad, noisy))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if out:
        with open(out, "w") as fh:
            fh.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="mode", required=True)
    sub.add_parser("dump").add_argument("dir")
    c = sub.add_parser("compare")
    c.add_argument("dir_a")
    c.add_argument("dir_b")
    c.add_argument("--rerun", default=None)
    c.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.exit(dump(args.dir) if args.mode == "dump" else compare(args.dir_a, args.dir_b, args.rerun, args.out))
