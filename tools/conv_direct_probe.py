#!/usr/bin/env python
"""microseconds of the narrow 3x3 layers at batch 16 (conv1_2 64 -> 64 at 321x321; conv2_1 64 -> 128, conv2_2 128 -> 128 and
the data gradient of conv2_1, 128 -> 64, at 161x161): the direct HIP kernel against MIOpen through F.conv2d; then the two masked
data gradients of the train step (conv1_2 and conv2_2, ops.conv3x3_direct_dgrad).  --direct-only: only the direct forward and
data-gradient kernels, five timings of 50 launches each (median, min, max).  Every direct line ends with a checksum of the output it timed
(the sum of its raw 16-bit words), so that two builds (DSRG_LIB) can be compared for equality on the same seeded data"""
import os, sys
import torch
import torch.nn.functional as F
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dsrg_amd import ops
cl = torch.channels_last
DIRECT_ONLY = "--direct-only" in sys.argv[1:]
torch.manual_seed(0)
def checksum(y):
    return int(y.contiguous(memory_format=cl).view(torch.int16).to(torch.int64).bitwise_and(0xffff).sum())
def t5(f):
    v = sorted(t(f, 50) for _ in range(5))
    return v[2], v[0], v[4]
def t(f, it=10):
    for _ in range(3): f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(it): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / it * 1e3
for cin, cout, hw in [(64, 64, 321), (64, 128, 161), (128, 128, 161), (128, 64, 161)]:
    x = torch.randn(16, cin, hw, hw, device="cuda").bfloat16().contiguous(memory_format=cl)
    w = (torch.randn(cout, cin, 3, 3, device="cuda") * 0.05).bfloat16().contiguous(memory_format=cl)
    b = torch.randn(cout, device="cuda")
    flops = 2 * 16 * hw * hw * cout * 9 * cin
    byts = 16 * hw * hw * (cin + cout) * 2
    us, lo, hi = t5(lambda: ops.conv3x3_direct(x, w, b, True))
    print("%3d -> %3d @ %d: direct kernel  %.1f us (min %.1f max %.1f)  %.0f TFLOP/s  %.2f TB/s of in+out  checksum %d" % (
        cin, cout, hw, us, lo, hi, flops / us / 1e6, byts / us / 1e6, checksum(ops.conv3x3_direct(x, w, b, True))), flush=True)
    if DIRECT_ONLY: continue
    us = t(lambda: torch.relu_(F.conv2d(x, w, b.bfloat16(), padding=1)))
    print("%3d -> %3d @ %d: F.conv2d+relu  %.1f us  %.0f TFLOP/s" % (cin, cout, hw, us, flops / us / 1e6))
for c, hw in [(64, 321), (128, 161)]:
    g = torch.randn(16, c, hw, hw, device="cuda").bfloat16().contiguous(memory_format=cl)
    y = torch.relu(torch.randn(16, c, hw, hw, device="cuda")).bfloat16().contiguous(memory_format=cl)
    wt = (torch.randn(c, c, 3, 3, device="cuda") * 0.05).bfloat16().contiguous(memory_format=cl)
    us, lo, hi = t5(lambda: ops.conv3x3_direct_dgrad(g, wt, y))
    print("%3d -> %3d @ %d: masked dgrad   %.1f us (min %.1f max %.1f)  %.2f TB/s of in+out+mask  checksum %d" % (
        c, c, hw, us, lo, hi, 16 * hw * hw * 3 * c * 2 / us / 1e6, checksum(ops.conv3x3_direct_dgrad(g, wt, y)[0])), flush=True)
if DIRECT_ONLY: sys.exit(0)
print("weight gradients")
for cin, cout, hw in [(64, 64, 321), (64, 128, 161), (128, 128, 161)]:
    x = torch.randn(16, cin, hw, hw, device="cuda").bfloat16().contiguous(memory_format=cl)
    g = torch.randn(16, cout, hw, hw, device="cuda").bfloat16().contiguous(memory_format=cl)
    w = (torch.randn(cout, cin, 3, 3, device="cuda") * 0.05).bfloat16().contiguous(memory_format=cl)
    flops = 2 * 16 * hw * hw * cout * 9 * cin
    us = t(lambda: ops.conv3x3_wgrad(x, g))
    print("%3d -> %3d @ %d: direct wgrad  %.1f us  %.0f TFLOP/s  %.2f TB/s of x+g" % (cin, cout, hw, us, flops / us / 1e6, 16 * hw * hw * (cin + cout) * 2 / us / 1e6))
    us = t(lambda: torch.ops.aten.convolution_backward(g, x, w, None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1, [False, True, False]))
    print("%3d -> %3d @ %d: MIOpen wrw    %.1f us  %.0f TFLOP/s" % (cin, cout, hw, us, flops / us / 1e6))
x = torch.randn(16, 3, 321, 321, device="cuda").bfloat16().contiguous(memory_format=cl)
w = (torch.randn(64, 3, 3, 3, device="cuda") * 0.05).bfloat16().contiguous(memory_format=cl)
b = torch.randn(64, device="cuda")
g = torch.randn(16, 64, 321, 321, device="cuda").bfloat16().contiguous(memory_format=cl)
print("  3 ->  64 @ 321: direct kernel %.1f us, F.conv2d + bias + relu %.1f us; direct wgrad %.1f us, MIOpen wrw %.1f us" % (
    t(lambda: ops.conv3x3_direct(x, w, b, True)), t(lambda: torch.relu_(F.conv2d(x, w, b.bfloat16(), padding=1))),
    t(lambda: ops.conv3x3_wgrad(x, g)),
    t(lambda: torch.ops.aten.convolution_backward(g, x, w, None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1, [False, True, False]))))
