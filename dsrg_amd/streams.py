"""The side streams of the test-time loops, kept apart from the stream HIP graphs are captured on.

torch hands out side streams from a pool of 32 per device, in turn: the 33rd torch.cuda.Stream() of a process IS the first one
again.  The *_many generators of inference.py capture a new input shape's graph (backbone.GraphedForward) on the forward thread
while the CRF workers of crf.CRF_device_many launch and synchronise on streams of their own; capture_error_mode="thread_local"
lets the workers do that on OTHER streams, but a worker whose stream is the capturing stream itself launches into the open capture
and synchronises on it, which invalidates the capture (the next launch inside it fails: `miopenStatusUnknownError`, then `capturing
stream has unjoined work`).  Whether the pool lines up that way depends on how many streams the process made before.  So captures
run on capture_stream(), one stream per device made once, and every stream that may be busy during a capture comes from
side_stream(), which skips it."""
import torch

_capture = {}


def _index(device):
    if device is None:
        return torch.cuda.current_device()
    if isinstance(device, int):
        return device
    index = torch.device(device).index
    return torch.cuda.current_device() if index is None else index


def capture_stream(device=None):
    """the stream backbone.GraphedForward captures on: one per device, made at the first call"""
    index = _index(device)
    s = _capture.get(index)
    if s is None:
        s = _capture[index] = torch.cuda.Stream(device=index)
    return s


def side_stream(device=None):
    """torch.cuda.Stream(device) that is not capture_stream(device)"""
    index = _index(device)
    avoid = capture_stream(index).cuda_stream
    while True:
        s = torch.cuda.Stream(device=index)
        if s.cuda_stream != avoid:
            return s
