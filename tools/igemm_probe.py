#!/usr/bin/env python
"""A/B on one box: the implicit-GEMM convolution (csrc/conv_igemm.hip) against the route it replaces (NHWC im2col kernel +
hipBLASLt GEMM with fused bias / ReLU, solutions picked by TunableOp) for the wide layers of the backbone at batch 16.
Prints one line per layer: microseconds (median of the rounds; variants interleaved inside every round) and TFLOP/s.

  python tools/igemm_probe.py [--rounds 5] [--iters 10] [--batch 16]
  python tools/igemm_probe.py --ab A B [--rounds 7]     two debug variants (ops.set_igemm_variant; -1 = the default) of the layer table and
                                                        then of the weight-gradient table, interleaved in every round (after --warm seconds of
                                                        both): every round's time, each arm's spread, each table summed
  python tools/igemm_probe.py --ab 4 -1 --backward-groups   the whole backward of fc6 x4 and fc7 x4 (ops.conv_igemm_backward_groups: data
                                                        gradient + weight gradient + reductions per arm), two launches against the merged grid
"""
import argparse
import os
import sys
import time

os.environ.setdefault("PYTORCH_TUNABLEOP_ENABLED", "1")
os.environ.setdefault("PYTORCH_TUNABLEOP_FILENAME", "/tmp/dsrg_tunableop_probe.csv")
os.environ.setdefault("PYTORCH_TUNABLEOP_VERBOSE", "0")

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dsrg_amd import ops                                                           # noqa: E402
from dsrg_amd.backbone import _im2col_gemm                                         # noqa: E402

CL = torch.channels_last


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--ab", type=int, nargs=2, metavar=("A", "B"), default=None)
    ap.add_argument("--warm", type=float, default=1.0, help="--ab: seconds of alternating launches per layer before the timed rounds")
    ap.add_argument("--wgrad-only", action="store_true", help="--ab: the weight-gradient table alone")
    ap.add_argument("--backward-groups", action="store_true", help="--ab: the grouped whole-backward table alone (fc6 x4, fc7 x4)")
    ap.add_argument("--force-order", type=int, default=0, help="--backward-groups: 1 / 2 = the data / weight gradient's blocks first in a merged grid")
    args = ap.parse_args()
    B = args.batch
    layers = [  # name, H, W, cin, cout, k, dilations (len = groups)
        ("conv4_2 512->512 d1", 41, 41, 512, 512, 3, [1]),
        ("conv5_1 512->512 d2", 41, 41, 512, 512, 3, [2]),
        ("conv4_1 256->512 d1", 41, 41, 256, 512, 3, [1]),
        ("conv4_1 dgrad 512->256", 41, 41, 512, 256, 3, [1]),
        ("fc6 512->1024 d12", 41, 41, 512, 1024, 3, [12]),
        ("fc6 x4 (one launch)", 41, 41, 512, 1024, 3, [6, 12, 18, 24]),
        ("fc6 dgrad 1024->512 d12", 41, 41, 1024, 512, 3, [12]),
        ("fc6 dgrad x4", 41, 41, 1024, 512, 3, [6, 12, 18, 24]),
        ("fc7 1024->1024 1x1", 41, 41, 1024, 1024, 1, [1]),
        ("fc7 x4 (one launch)", 41, 41, 1024, 1024, 1, [1, 1, 1, 1]),
        ("conv3_2 256->256 81x81", 81, 81, 256, 256, 3, [1]),
        ("conv3_1 128->256 81x81", 81, 81, 128, 256, 3, [1]),
    ]
    if args.ab and args.backward_groups:
        return variant_ab(BWD_GROUP_LAYERS, B, args.ab, args.rounds, args.iters, args.warm, bwd=True, order=args.force_order)
    if args.ab:
        if not args.wgrad_only:
            variant_ab(layers, B, args.ab, args.rounds, args.iters, args.warm)
        return variant_ab(WGRAD_LAYERS, B, args.ab, args.rounds, args.iters, args.warm, wgrad=True)
    print("%-28s %9s %9s %9s %9s | %8s %8s | %s" % ("layer", "variant", "default", "im2col+mm", "mm only", "TF/s ig", "TF/s old", "max err"))
    for name, H, W, cin, cout, k, dils in layers:
        n = len(dils)
        torch.manual_seed(1)
        xs = [torch.randn(B, cin, H, W, device="cuda").bfloat16().contiguous(memory_format=CL) for _ in range(n)]
        ws = [(torch.randn(cout, cin, k, k, device="cuda") * (2.0 / (cin * k * k)) ** 0.5).bfloat16() for _ in range(n)]
        bs = [torch.randn(cout, device="cuda") for _ in range(n)]
        packed = [ops.pack_conv_weight(w) for w in ws]
        bsb = [b.bfloat16() for b in bs]

        sk = [True]

        def run_ig():
            return ops.conv_igemm(xs, packed, bs, dils, k, True, stream_k=sk[0])

        def run_old():
            return [_im2col_gemm(xs[g], ws[g], bsb[g], dils[g], True) for g in range(n)]

        cols = [ops.im2col3x3_nhwc(xs[g].permute(0, 2, 3, 1), dils[g]) if k == 3 else xs[g].permute(0, 2, 3, 1).reshape(-1, cin) for g in range(n)]
        wm = [ws[g].permute(2, 3, 1, 0).reshape(k * k * cin, cout) for g in range(n)]
        outs = [torch.empty(B * H * W, cout, device="cuda", dtype=torch.bfloat16) for _ in range(n)]

        def run_mm():
            for g in range(n):
                torch._addmm_activation(bsb[g], cols[g], wm[g], out=outs[g])

        # correctness of the first group against fp32 torch (bias rounded as the old route rounds it: bf16)
        want = torch.relu(F.conv2d(xs[0].float(), ws[0].float(), bs[0], padding=dils[0] * (k // 2), dilation=dils[0]))
        got = run_ig()[0]
        err = float((got.float() - want).abs().max() / want.abs().max())
        for fn in (run_ig, run_old, run_mm):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        t = {"ig1": [], "ig0": [], "old": [], "mm": []}
        for _ in range(args.rounds):
            sk[0] = False
            ops.set_igemm_variant(int(os.environ.get("PROBE_VARIANT", "4")))     # 4: stream-K wherever legal (needs the scratch)
            sk[0] = os.environ.get("PROBE_VARIANT", "4") == "4"
            t["ig1"].append(timed(run_ig, args.iters))
            ops.set_igemm_variant(-1)
            sk[0] = False
            t["ig0"].append(timed(run_ig, args.iters))
            t["old"].append(timed(run_old, args.iters))
            t["mm"].append(timed(run_mm, args.iters))
        ops.set_igemm_variant(-1)
        med = {k_: float(np.median(v)) for k_, v in t.items()}
        flops = 2.0 * B * H * W * cin * k * k * cout * n
        print("%-28s %9.1f %9.1f %9.1f %9.1f | %8.0f %8.0f | %.2e" % (
            name, med["ig1"], med["ig0"], med["old"], med["mm"], flops / min(med["ig1"], med["ig0"]) / 1e6,
            flops / med["old"] / 1e6, err), flush=True)
    wgrad_probe(B, args.rounds, args.iters)
    absorb_probe(B, args.rounds, args.iters)


def variant_ab(layers, B, ab, rounds, iters, warm_s, wgrad=False, bwd=False, order=0):
    """two variants of every layer of the table on random operands, alternating inside every round (A B A B ..), stream-K where the
    launcher picks it (as the train step runs them); wgrad: the weight gradient (ops.conv_igemm_wgrad, float32) of the table
    instead of the forward; bwd: the whole backward of the table's grouped layers (ops.conv_igemm_backward_groups; a 1x1 layer with
    masks, Dropout scale and bias gradients as fc7_k runs it).  Per layer: every round of both arms, medians, max - min of each arm; then the
    table summed per round — the figure a decision between the two is taken on: the gain of the summed medians against twice the
    spread of arm A's own rounds"""
    arms = ("A = variant %d" % ab[0], "B = variant %d" % ab[1])
    print("%s%s, %s; batch %d, %.1f s of warm-up per layer, %d rounds of %d launches each; microseconds per launch" % (
        ("whole backward: " if bwd else "weight gradients: " if wgrad else "",) + arms + (B, warm_s, rounds, iters)))
    tot = np.zeros((2, rounds))
    for name, H, W, cin, cout, k, dils in layers:
        n = len(dils)
        torch.manual_seed(1)
        xs = [torch.randn(B, cin, H, W, device="cuda").bfloat16().contiguous(memory_format=CL) for _ in range(n)]
        packed = [ops.pack_conv_weight((torch.randn(cout, cin, k, k, device="cuda") * (2.0 / (cin * k * k)) ** 0.5).bfloat16()) for _ in range(n)]
        bs = [torch.randn(cout, device="cuda") for _ in range(n)]

        gs = [torch.randn(B, cout, H, W, device="cuda").bfloat16().contiguous(memory_format=CL) for _ in range(n)] if (wgrad or bwd) else None
        if bwd:
            xs = [x.relu() for x in xs]                   # the layer's inputs as masks: ReLU outputs
            packs_d = [ops.pack_conv_weight(torch.randn(cout, cin, k, k, device="cuda") * (2.0 / (cin * k * k)) ** 0.5, for_dgrad=True) for _ in range(n)]
            print("%-28s plan A %s" % (name, _plan_of(ab[0], n, B, H, W, cin, cout, k, dils, order)))
            print("%-28s plan B %s" % ("", _plan_of(ab[1], n, B, H, W, cin, cout, k, dils, order)))

        def run():
            if bwd:
                gx, gw, gb = ops.conv_igemm_backward_groups(gs, packs_d, xs, dils, k, xs if k == 1 else None, 2.0 if k == 1 else 1.0, force_order=order)
                return list(gx) + list(gw) + list(gb or [])
            if wgrad:
                return ops.conv_igemm_wgrad(xs, gs, dils, k)
            return ops.conv_igemm(xs, packed, bs, dils, k, True, stream_k=True)
        t = np.zeros((2, rounds))
        try:
            outs = []
            for v in ab:
                ops.set_igemm_variant(v)
                for _ in range(3):
                    outs.append(run())
            torch.cuda.synchronize()
            diff = max(float((a_.float() - b_.float()).abs().max()) for a_, b_ in zip(outs[0], outs[-1]))
            t0 = time.time()
            while time.time() - t0 < warm_s:              # to the clock the chip holds under this load: the first milliseconds run faster
                for v in ab:
                    ops.set_igemm_variant(v)
                    timed(run, iters)
            for r in range(rounds):
                for i, v in enumerate(ab):
                    ops.set_igemm_variant(v)
                    t[i, r] = timed(run, iters)
        finally:
            ops.set_igemm_variant(-1)
        tot += t
        med = np.median(t, axis=1)
        print("%-28s A %s | med %7.1f spread %5.1f" % (name, " ".join("%7.1f" % v for v in t[0]), med[0], t[0].max() - t[0].min()))
        print("%-28s B %s | med %7.1f spread %5.1f | B/A %.4f  max |A - B| %.3g" % ("", " ".join("%7.1f" % v for v in t[1]), med[1], t[1].max() - t[1].min(),
                                                                                  med[1] / med[0], diff), flush=True)
    med = np.median(tot, axis=1)
    print("%-28s A %s | med %7.1f spread %5.1f" % ("sum of the table", " ".join("%7.1f" % v for v in tot[0]), med[0], tot[0].max() - tot[0].min()))
    print("%-28s B %s | med %7.1f spread %5.1f | B/A %.4f" % ("", " ".join("%7.1f" % v for v in tot[1]), med[1], tot[1].max() - tot[1].min(), med[1] / med[0]))
    print("gain of the summed medians %.1f us; twice the spread of A's rounds %.1f us" % (med[0] - med[1], 2.0 * (tot[0].max() - tot[0].min())))


def _plan_of(variant, n, B, H, W, cin, cout, k, dils, order=0):
    ops.set_igemm_variant(variant)
    try:
        return ops.conv_igemm_backward_groups_plan(n, B, H, W, cin, cout, k, dils, with_mask=k == 1, force_order=order)
    finally:
        ops.set_igemm_variant(-1)


def absorb_probe(B, rounds, iters):
    """the data gradient with the ReLU (+ Dropout) backward and bias gradient of the layer below in its store against the plain
    data gradient followed by ops.relu_bwd_bias"""
    layers = [("conv4_3 -> conv4_2 out", 41, 41, 512, 512, 3, [1]), ("conv3_3 -> conv3_2 out", 81, 81, 256, 256, 3, [1]),
              ("fc7 x4 -> fc6 out", 41, 41, 1024, 1024, 1, [1] * 4)]
    print("%-28s %9s %9s %9s" % ("fused backward", "fused", "separate", "dgrad only"))
    for name, H, W, cf, cb, k, dils in layers:
        n = len(dils)
        torch.manual_seed(3)
        gs = [torch.randn(B, cf, H, W, device="cuda").bfloat16().contiguous(memory_format=CL) for _ in range(n)]
        ys = [torch.relu(torch.randn(B, cb, H, W, device="cuda")).bfloat16().contiguous(memory_format=CL) for _ in range(n)]
        packs = [ops.pack_conv_weight((torch.randn(cf, cb, k, k, device="cuda") * 0.02), for_dgrad=True) for _ in range(n)]

        def fused():
            return ops.conv_igemm_dgrad(gs, packs, ys, dils, k, 2.0)

        def plain():
            return ops.conv_igemm(gs, packs, None, dils, k, False, stream_k=False)

        def separate():
            return [ops.relu_bwd_bias(g, y, 2.0) for g, y in zip(plain(), ys)]
        for fn in (fused, separate, plain):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        t = {"f": [], "s": [], "p": []}
        for _ in range(rounds):
            t["f"].append(timed(fused, iters)); t["s"].append(timed(separate, iters)); t["p"].append(timed(plain, iters))
        print("%-28s %9.1f %9.1f %9.1f" % (name, np.median(t["f"]), np.median(t["s"]), np.median(t["p"])), flush=True)


WGRAD_LAYERS = [("conv4_2 512->512", 41, 41, 512, 512, 3, [1]), ("conv4_1 256->512", 41, 41, 256, 512, 3, [1]),
                ("fc6 512->1024 d12", 41, 41, 512, 1024, 3, [12]), ("fc6 x4 (one launch)", 41, 41, 512, 1024, 3, [6, 12, 18, 24]),
                ("fc7 1024->1024 1x1", 41, 41, 1024, 1024, 1, [1]), ("fc7 x4 (one launch)", 41, 41, 1024, 1024, 1, [1] * 4),
                ("conv3_2 256->256 81x81", 81, 81, 256, 256, 3, [1])]


BWD_GROUP_LAYERS = [("fc6 x4 backward", 41, 41, 512, 1024, 3, [6, 12, 18, 24]), ("fc7 x4 backward", 41, 41, 1024, 1024, 1, [1] * 4)]


def wgrad_probe(B, rounds, iters):
    """the implicit weight gradient against im2col + g^T @ cols (what backbone._ConvFn.backward runs today)"""
    layers = WGRAD_LAYERS
    print("%-28s %9s %9s %9s | %8s %8s | %s" % ("weight gradient", "igemm", "im2col+mm", "mm only", "TF/s ig", "TF/s old", "max err"))
    for name, H, W, cin, cout, k, dils in layers:
        n = len(dils)
        torch.manual_seed(2)
        xs = [torch.randn(B, cin, H, W, device="cuda").bfloat16().contiguous(memory_format=CL) for _ in range(n)]
        gs = [torch.randn(B, cout, H, W, device="cuda").bfloat16().contiguous(memory_format=CL) for _ in range(n)]

        def run_ig():
            return ops.conv_igemm_wgrad(xs, gs, dils, k)

        def cols_of(g_):
            return ops.im2col3x3_nhwc(xs[g_].permute(0, 2, 3, 1), dils[g_]) if k == 3 else xs[g_].permute(0, 2, 3, 1).reshape(-1, cin)

        def run_old():
            return [torch.mm(gs[g_].permute(0, 2, 3, 1).reshape(-1, cout).t(), cols_of(g_)) for g_ in range(n)]
        cols = [cols_of(g_) for g_ in range(n)]

        def run_mm():
            return [torch.mm(gs[g_].permute(0, 2, 3, 1).reshape(-1, cout).t(), cols[g_]) for g_ in range(n)]
        want = run_old()[0].float().view(cout, k, k, cin).permute(0, 3, 1, 2)
        got = run_ig()[0]
        err = float((got - want).abs().max() / want.abs().max())
        for fn in (run_ig, run_old, run_mm):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        t = {"ig": [], "ig3": [], "old": [], "mm": []}
        for _ in range(rounds):
            ops.set_igemm_variant(3)
            t["ig3"].append(timed(run_ig, iters))
            ops.set_igemm_variant(1)
            t["ig"].append(timed(run_ig, iters))
            t["old"].append(timed(run_old, iters))
            t["mm"].append(timed(run_mm, iters))
        med = {k_: float(np.median(v)) for k_, v in t.items()}
        flops = 2.0 * B * H * W * cin * k * k * cout * n
        print("%-28s %9.1f %9.1f %9.1f | %8.0f %8.0f | %.2e  (staggered %.1f)" % (name, med["ig"], med["old"], med["mm"], flops / med["ig"] / 1e6,
                                                                  flops / med["old"] / 1e6, err, med["ig3"]), flush=True)


if __name__ == "__main__":
    main()
