#!/usr/bin/env python
"""bench.py — images/s of a full DSRG train-s step on N MI355X (BASELINE.json metric).

A step = VGG16-ASPP forward (bf16 autocast) -> supervision hot path in libdsrg_hip.so (Softmax, dense-CRF mean field,
seeded region growing, seed + constrain losses, backward) -> backbone backward -> Caffe-style SGD, on one synthetic batch of
16 images per GPU (BASELINE.json configs[2]; configs[3] at N=8).  Synthetic inputs are resident in HBM before the timed region.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--batch B] [--mode train|supervision|infer|crf-fullres|test-ms|train-f]
                  [--full] [--dump-outputs DIR]
  N>1: python bench.py --gpus N starts `python -m torch.distributed.run --nnodes=1 --nproc-per-node N
       --master-addr 127.0.0.1 ... bench.py --gpus N ...` as a child process (one rank per GPU over RCCL) and exits with its
       status; started under that launcher already (WORLD_SIZE set) it runs as a rank.  Fewer than N GPUs visible: one line
       saying so, exit status 1.

Rank 0 prints ONE JSON line.  A plain run of --mode train or train-f sets up, warms up, times the K steps and prints the
contract fields (`value`, `ms_per_step`, ...) with the figures that follow from the timed steps alone (backbone TFLOP/s).
--dump-outputs DIR then also writes what the last timed step computed as DIR/<name>.npy (float32 / float64): the losses the
step returns and the trainable parameters it updated (each whole up to PARAM_SAMPLE elements, a larger one at PARAM_SAMPLE
fixed, seeded positions); the other modes write their own results (supervision: losses and the gradient to the logits;
infer: seeds; crf-fullres: marginals; test-ms: mask).  The inputs are seeded: the same arguments give the same inputs.

--full adds, for --mode train on one rank, what the headline does not need (the --no-* switches still drop single parts):
  roofline      — the dominant hot-path kernel (mean-field filter = permutohedral splat/blur/slice): modelled LDS bytes per
                  launch / HIP-event time per launch, measured in a separate untimed pass (the event brackets cost ~5 us each)
  cpu_baseline  — the CPU oracle (a port of the reference's CPU path) timed on this box's host cores on a bounded sample of
                  the same workload (rank 0, N=1 only)
  legs          — the bf16-autocast leg (= value) and the float32-backbone leg (the reference's Caffe precision), same steps;
                  grad_cosine_min / loss_gap_300_steps: how close the two legs' gradients and 300-step trajectories are
  modes         — (N=1, --mode train) bounded sub-records of the other quoted configurations, each with its own roofline and
                  cpu_baseline: supervision (hot path alone, 16 images), supervision_b1, infer_b1 (BASELINE.json configs[1]),
                  crf_fullres, train_f (the reference's stage 2: VGG16-ASPP 321x321, batch 16), train_f_resnet101_513
                  (BASELINE.json configs[4] on one GPU, batch 10)
  also          — other_rooflines (region growing), supervision_ms_per_step and the weight checksum of a single process (a
                  run under a process group always all-gathers the checksums: its figure stands on the replicas agreeing)
"""
import argparse
import json
import os
import sys
import time

# hipBLASLt solution selection by PyTorch's own online tuner (TunableOp): each GEMM shape of the backbone is timed once
# during the warm-up steps and the fastest solution kept (+1.3 % measured); set PYTORCH_TUNABLEOP_ENABLED=0 to opt out
# (not for --mode test-ms: three input sizes at batch 1 are ~60 GEMM shapes, each tuned for seconds the first time it is seen — a
# one-off cost a 10 582-image run amortises, but one that would BE that bounded record)
os.environ.setdefault("PYTORCH_TUNABLEOP_ENABLED", "0" if "test-ms" in sys.argv else "1")
os.environ.setdefault("PYTORCH_TUNABLEOP_FILENAME", "/tmp/dsrg_tunableop_%s.csv" % os.environ.get("LOCAL_RANK", "0"))   # one file per rank
os.environ.setdefault("PYTORCH_TUNABLEOP_VERBOSE", "0")
# dmabuf IPC between the ranks of a node (the image exports this already; RCCL's intra-node transport fails with
# `hipIpcGetMemHandle: invalid argument` without it): set before the HIP runtime starts, inherited by the ranks bench.py launches
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.3 TB/s achievable)


def filter_bytes(d, M, C, N):
    """stage-streamed traffic of one splat/blur/slice over C label planes."""
    return 8 * C * N + 16 * (d + 1) * N + 8 * C * M + (d + 1) * (16 * C * M + 8 * M)


# MI355X_MICROARCH.md, LDS table: bytes per clock per CU by instruction, x 256 CUs x 2.4 GHz
LDS_RATE_GBS = {"read_b128": 256 * 256 * 2.4, "read_b64": 256 * 256 * 2.4, "read_b32": 128 * 256 * 2.4,
                "write_b128": 79 * 256 * 2.4, "write_b64": 85 * 256 * 2.4, "write_b32": 64 * 256 * 2.4}


def lds_filter_traffic(d, M, X, N, cpw):
    """LDS bytes one workgroup of mf_filter_kernel moves for one lattice (dsrg_amd/csrc/meanfield.hip, filter_lattice), cpw
    label planes of 4 bytes interleaved per element (8-byte accesses at cpw = 2, 16-byte at cpw = 4):
    reads  = first splat term of every vertex (M gathers of the input planes) + products of the X further entries (X gathers)
             + ordered row sums over those products (X) + blur (2 gathers per vertex and axis) + slice (d+1 per pixel);
    writes = input planes (N) + products (X) + lattice values (M) + blur (M per axis).
    A pixel-local Gaussian lattice (training scale) is evaluated in registers by the update kernel: no LDS bytes."""
    reads = (M + 2 * X + 2 * (d + 1) * M + (d + 1) * N) * 4 * cpw
    writes = (N + X + M + (d + 1) * M) * 4 * cpw
    return reads, writes


def lds_filter_instructions(d, M, X, N, vpt=10, wg=1024):
    """wave-level LDS instructions of the same workgroup as ISSUED (what SQ_INSTS_LDS counts): vertex slots come in batches
    of (5, 4, 1) x 1024 and a batch is issued when its first vertex exists, pixels in ceil(N / 1024) rounds, entries in
    rounds of 1024 — the check of the byte model against the counter (profiles/r03_lds_counters.json)"""
    waves = wg // 64
    bounds = [0, min(5, vpt), min(9, vpt), vpt]
    slots = sum(bounds[i + 1] - bounds[i] for i in range(3) if bounds[i] * wg < M)
    xs = -(-X // wg) if X else 0
    xs = min(vpt, -(-xs // 5) * 5) if xs else 0
    ppt = -(-N // wg)
    reads = slots + xs + 2 * (d + 1) * slots + (d + 1) * ppt            # first terms, extra products, blur, slice
    writes = ppt + xs + -(-M // wg) + (d + 1) * -(-M // wg) + 1          # input planes, products, values, blur (+ sentinel)
    # the ordered row sums are data-dependent loops (one read per further entry of the longest row of a wave's 64): not modelled
    return (reads + writes) * waves


def cpu_baseline(batch_np, target_s=12.0):
    """Time the CPU oracle on the supervision path of the same synthetic images (single thread)."""
    from oracle import oracle as O
    B = batch_np["logits"].shape[0]
    n_done, t0 = 0, time.perf_counter()
    while True:
        for b in range(B):
            sl = slice(b, b + 1)
            logits = batch_np["logits"][sl]
            probs = O.softmax_forward(logits)
            refined, logq = O.crf_refine_batch(probs, batch_np["images"][sl], 12.0, 10)
            seeds = O.srg_grow_batch(batch_np["labels"][sl], batch_np["cues"][sl], refined)
            _, g1 = O.seed_loss(probs, seeds)
            _, g2, g3 = O.constrain_loss(probs, logq)
            O.softmax_backward(logits, g1 + g2 + O.crf_layer_backward(refined, g3))
            n_done += 1
            if time.perf_counter() - t0 > target_s:
                break
        if time.perf_counter() - t0 > target_s:
            break
    dt = time.perf_counter() - t0
    return {"value": n_done / dt, "unit": "images/s (supervision path only: softmax+CRF+SRG+losses+backward)",
            "cores": 1, "kind": "port",
            "sample": "%d images of the bench batch, %.1f s, oracle/dsrg_oracle.c single-threaded; the "
                      "reference runs exactly this part on the CPU (its convolutions run in Caffe on a GPU)" % (n_done, dt)}


def cpu_baseline_all_cores(seconds=6.0, max_workers=None, timeout_s=150.0):
    """the same port, image-parallel over the host's logical CPUs as the reference's multiprocessing.Pool() does it (one worker
    per CPU, BASELINE.md §3: nproc): independent `oracle/baseline_worker.py` processes (they never touch the GPU), every wait
    bounded by a timeout; `cores` in the record is the number of workers that finished"""
    import subprocess
    workers = max(1, min(os.cpu_count() or 1, max_workers or (os.cpu_count() or 1)))
    t0 = time.perf_counter()
    env = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "oracle", "baseline_worker.py"), str(5000 + w), str(seconds)],
                              stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, env=env) for w in range(workers)]
    n, span, failed = 0, 0.0, 0
    for p in procs:
        try:
            out, _ = p.communicate(timeout=max(1.0, timeout_s - (time.perf_counter() - t0)))
            a, b = out.decode().split()[:2]
            n += int(a)
            span = max(span, float(b))
        except Exception:
            p.kill()
            failed += 1
    if n == 0:
        return {"error": "no worker finished within %.0f s" % timeout_s}
    return {"value": n / span, "unit": "images/s (supervision path only)", "cores": workers - failed, "kind": "port",
            "sample": "%d images over %d processes in %.1f s of work each (%.1f s with process start-up), host has %d "
                      "logical CPUs" % (n, workers - failed, span, time.perf_counter() - t0, os.cpu_count() or 0)}


def event_overhead_ms(stream=None):
    """a HIP-event bracket also times the event signalling itself: the cost of an empty bracket on the same stream, to be
    taken off so that a per-launch figure is the kernel's duration as rocprofv3 --kernel-trace sees it"""
    st = stream or torch.cuda.current_stream()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(64)]
    for _ in range(2):
        for a, b in pairs:
            a.record(st)
            b.record(st)
        torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in pairs]))


def _load_json(name):
    try:
        return json.load(open(os.path.join(ROOT, "profiles", name)))
    except Exception:
        return None


def _counter_file(stem, kernel):
    """the newest profiles/rNN_<stem>.json and whether it still describes `kernel`: the PMC passes run outside bench.py
    (tools/gpu_pmc.sh) and their figures are replayed here — only while the kernel's sources hash to what the file was
    collected against (dsrg_amd/provenance.py); -> (record or None, provenance dict for the bench line)"""
    from dsrg_amd import provenance
    for rnd in ("r06", "r05", "r04", "r03"):
        rec = _load_json("%s_%s.json" % (rnd, stem))
        if rec is not None:
            src = provenance.check(rec, kernel)
            src["file"] = "profiles/%s_%s.json" % (rnd, stem)
            return (rec if src["match"] else None), src
    return None, {"file": None, "match": False}


PARAM_SAMPLE = 65536                    # elements kept of each trainable parameter in --dump-outputs (VGG16-ASPP: 5.3 MB in all)
DUMP_LIMIT_BYTES = 64 << 20


def param_sample(net):
    """the trainable parameters as the last step left them: each whole up to PARAM_SAMPLE elements, a larger one at PARAM_SAMPLE
    positions drawn by a generator seeded with the parameter's index (the same elements in every run and every build)"""
    out = {}
    for i, (name, p) in enumerate(n_p for n_p in net.named_parameters() if n_p[1].requires_grad):
        flat = p.detach().reshape(-1)
        if flat.numel() > PARAM_SAMPLE:
            idx = np.sort(np.random.default_rng(i).choice(flat.numel(), PARAM_SAMPLE, replace=False))
            flat = flat[torch.from_numpy(idx).to(flat.device)]
        out["param." + name] = flat
    return out


def write_outputs(path, arrays):
    """--dump-outputs: every array as <path>/<name>.npy, float64 kept, everything else as float32"""
    host = {}
    for name, a in arrays.items():
        a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
        host[name] = np.ascontiguousarray(a, dtype=np.float64 if a.dtype == np.float64 else np.float32)
    total = sum(a.nbytes for a in host.values())
    if total > DUMP_LIMIT_BYTES:
        raise SystemExit("bench.py --dump-outputs: %d bytes of outputs, over the %d-byte limit" % (total, DUMP_LIMIT_BYTES))
    os.makedirs(path, exist_ok=True)
    for name, a in host.items():
        np.save(os.path.join(path, name + ".npy"), a)


def crf_fullres_record(device, steps, warmup, cpu=True, size=321, dump=None):
    """SURVEY 8f-1, training/tools/test-ms.py:84-111: the test-time dense CRF at image resolution — log-probability unaries,
    scale_factor 1, 21 labels, 10 iterations — through krahenbuhl2013's object API with device pointers (dsrg_amd.crf.DenseCRF;
    what CRF_device does per call).  One step = one image: unary + pairwise set-up (both lattices are built) + inference.
    This is the path where HBM/L2 bandwidth is the bound: lattice values live in HBM and one launch streams them per blur axis."""
    from dsrg_amd import synthetic as S
    from dsrg_amd.crf import DenseCRF
    C, out_sizes = 21, []
    sizes = [(321, 321), (375, 500)] if size == 321 else [(size, size)]
    for (H, W) in sizes:
        rng = np.random.default_rng(3000 + H)
        img = S.make_images(rng, 1, size=max(H, W))[0, :, :H, :W] + S.MEAN_PIXEL[:, None, None]
        im_np = np.ascontiguousarray(np.transpose(img, (1, 2, 0))).astype(np.uint8)
        logits = S.make_logits(rng, 1, C, H, W, gain=12.0, sigma=12.0)[0]
        e = np.exp(logits - logits.max(0, keepdims=True))
        un_np = np.log(np.maximum(e / e.sum(0, keepdims=True), 1e-5)).transpose(1, 2, 0).astype(np.float32)   # test-ms.py:102-106
        im, neg = torch.from_numpy(im_np).to(device), (-torch.from_numpy(np.ascontiguousarray(un_np)).to(device)).contiguous()
        out = torch.empty((H, W, C), dtype=torch.float32, device=device)
        crf = DenseCRF(W, H, C)

        def one():
            crf.set_unary_energy(neg)
            crf.add_pairwise_energy(10, 80.0, 80.0, 13, 13, 13, 3, 3.0, 3.0, im)
            crf.inference(10, out=out)
        for _ in range(warmup):
            one()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            one()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        nprof = max(2, min(steps, 5))
        crf.profile_start(nprof * 10 + 8)                   # the dominant kernel, bracketed in a separate untimed pass
        for _ in range(nprof):
            one()
        torch.cuda.synchronize()
        blur_ms, blur_n = crf.profile_stop()
        mg, mb = crf.lattice_size(0), crf.lattice_size(1)
        N = H * W
        # SURVEY 8d, the splat stage of filter(d, M) for both lattices in one launch: the input planes in = Q * norm of each
        # kernel (two arrays of 4 C N, each read once — the update kernel forms them, lattice_large.hip), the (pixel, weight)
        # pair of every (pixel, corner) entry (8 (d+1) N per lattice), the lattice rows out (4 C M per lattice)
        alg_per_launch = 2 * 4 * C * N + 8 * (6 + 3) * N + 4 * C * (mb + mg)
        out_sizes.append(dict(H=H, W=W, images_per_s=steps / dt, ms_per_image=dt / steps * 1e3, M_gauss=mg, M_bil=mb,
                              splat_us_per_launch_event_bracket=blur_ms / max(blur_n, 1) * 1e3, splat_launches=blur_n,
                              alg_bytes_per_splat_launch=alg_per_launch,
                              crf_alg_bytes=10 * (filter_bytes(2, mg, C, N) + filter_bytes(5, mb, C, N) + 8 * C * N),
                              q=out.cpu().numpy(), im=im_np, un=un_np, dt=dt))
    # the same images with four of them in flight (one object + stream each: dsrg_amd.crf.CRF_device_many) — how the test-time
    # loop over 10 582 images runs; arg-max labels out
    from dsrg_amd.crf import CRF_device_many
    head = out_sizes[0]
    im0 = torch.from_numpy(head["im"]).to(device)
    un0 = torch.from_numpy(np.ascontiguousarray(head["un"])).to(device)
    npipe = max(8, steps)
    for _ in CRF_device_many([(im0, un0)] * 8, scale_factor=1.0, in_flight=4):
        pass
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in CRF_device_many([(im0, un0)] * npipe, scale_factor=1.0, in_flight=4):
        pass
    torch.cuda.synchronize()
    pipelined = npipe / (time.perf_counter() - t0)
    # ... and batched (round 5, dsrg_crf_create_batch): eight same-sized images per call — every launch of the build and of the
    # mean-field loop carries all of them — alone and with two such calls in flight
    from dsrg_amd.crf import CRF_device_batch, DenseCRF as _DenseCRF
    nb = 8
    ims8, uns8 = torch.stack([im0] * nb), torch.stack([un0] * nb)
    for _ in range(2):
        CRF_device_batch(ims8, uns8, scale_factor=1.0, want="map")
    torch.cuda.synchronize()
    reps = max(2, steps // 4)
    t0 = time.perf_counter()
    for _ in range(reps):
        CRF_device_batch(ims8, uns8, scale_factor=1.0, want="map")
    torch.cuda.synchronize()
    batched = nb * reps / (time.perf_counter() - t0)
    for _ in CRF_device_many([(im0, un0)] * (4 * nb), scale_factor=1.0, in_flight=2, batch=nb):
        pass
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in CRF_device_many([(im0, un0)] * (8 * nb), scale_factor=1.0, in_flight=2, batch=nb):
        pass
    torch.cuda.synchronize()
    batched_pipelined = 8 * nb / (time.perf_counter() - t0)
    # the batched object's splat launch, bracketed like the single-image one: the same algorithmic bytes per image, x nb per launch
    bcrf = _DenseCRF(head["W"], head["H"], C, nimages=nb)
    bout = torch.empty((nb, head["H"], head["W"], C), dtype=torch.float32, device=device)

    def one_batch():
        bcrf.set_unary_energy((-uns8).contiguous())
        bcrf.add_pairwise_energy(10, 80.0, 80.0, 13, 13, 13, 3, 3.0, 3.0, ims8)
        bcrf.inference(10, out=bout)
    one_batch()
    bcrf.profile_start(3 * 10 + 8)
    for _ in range(3):
        one_batch()
    torch.cuda.synchronize()
    bsplat_ms, bsplat_n = bcrf.profile_stop()
    batch_same = bool(torch.equal(bout[0], bout[nb - 1]))                   # eight copies of one image: eight equal results
    ev_us = event_overhead_ms(torch.cuda.default_stream()) * 1e3
    per_launch_s = max(head["splat_us_per_launch_event_bracket"] - ev_us, 1e-3) * 1e-6
    tj, traffic_src = _counter_file("pmc_traffic_fullres", "fullres")
    traffic = (tj or {}).get("lg_splat2_kernel_bytes_per_launch")
    achieved = head["alg_bytes_per_splat_launch"] / per_launch_s / 1e9
    roofline = {"kernel": "lg_splat2_kernel (+ lg_combine_kernel for rows beyond 4 096 entries) — permutohedral splat of both lattices: one "
                          "ordered sum per vertex over its gather list, in the reference's order; values in HBM/L2.  One image per launch: "
                          "the longest row sets the launch's duration; modes.crf_fullres.batch8_splat is the throughput form",
                "bound": "hbm",
                "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS, "traffic": traffic,
                "traffic_source": traffic_src,
                "alg_bytes_per_launch": head["alg_bytes_per_splat_launch"], "us_per_launch": per_launch_s * 1e6,
                "us_per_launch_event_bracket": head["splat_us_per_launch_event_bracket"], "event_bracket_overhead_us": ev_us,
                "launches": head["splat_launches"], "lattice_M_gauss": head["M_gauss"], "lattice_M_bilateral": head["M_bil"],
                "hbm_gbs_from_pmc_traffic": (traffic / per_launch_s / 1e9) if traffic else None,
                "whole_crf_alg_gbs": head["crf_alg_bytes"] / (head["ms_per_image"] * 1e-3) / 1e9}
    rec = {"metric": "images/sec full-resolution dense CRF (test-ms.py:84-111; %dx%d, 21 labels, 10 iterations, lattices built "
                     "per image)" % (head["H"], head["W"]),
           "value": head["images_per_s"], "unit": "images/s", "n_gpus": 1, "steps": steps, "warmup": warmup,
           "ms_per_step": head["ms_per_image"], "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
           "dtype": "f32", "data": "synthetic",
           "config": {"workload": "krahenbuhl2013.CRF on device tensors, log-prob unaries, scale_factor 1, maxiter 10"},
           "images_per_s_four_in_flight": pipelined,
           "images_per_s_batch8": batched, "ms_per_image_batch8": 1e3 / batched,
           "images_per_s_batch8_two_in_flight": batched_pipelined,
           "batch8_splat": {"us_per_launch": (bsplat_ms / max(bsplat_n, 1)) * 1e3 - ev_us, "launches": bsplat_n,
                            "alg_bytes_per_launch": nb * head["alg_bytes_per_splat_launch"],
                            "hbm_gbs": nb * head["alg_bytes_per_splat_launch"] / max((bsplat_ms / max(bsplat_n, 1)) * 1e-3 - ev_us * 1e-6, 1e-9) / 1e9,
                            "frac_of_8TBs": nb * head["alg_bytes_per_splat_launch"] / max((bsplat_ms / max(bsplat_n, 1)) * 1e-3 - ev_us * 1e-6, 1e-9) / 1e9 / HBM_PEAK_GBS,
                            "eight_copies_equal": batch_same},
           "sizes": [{k: v for k, v in o.items() if k not in ("q", "im", "un", "dt")} for o in out_sizes],
           "roofline": roofline}
    if dump is not None:
        dump.update({"q_%dx%d" % (o["H"], o["W"]): o["q"] for o in out_sizes})      # each size's last timed call
    if cpu:
        from oracle import oracle as O
        t0 = time.perf_counter()
        want = O.CRF(head["im"], head["un"], scale_factor=1.0)
        t_cpu = time.perf_counter() - t0
        rec["cpu_baseline"] = {"value": 1.0 / t_cpu, "unit": "images/s", "cores": 1, "kind": "port",
                               "sample": "1 image %dx%d, oracle/dsrg_oracle.c single-threaded, %.2f s" % (head["H"], head["W"], t_cpu)}
        rec["max_abs_dq_vs_oracle"] = float(np.abs(head["q"] - want).max())
    return rec


def test_ms_record(device, steps, warmup, cpu=True, dump=None):
    """the reference's test-time loop end to end for one image per step (training/tools/test-ms.py:84-111, run.sh:6,10): three forwards at
    241 / 321 / 401, each score map zoomed to the image, summed, softmax, clip, log, full-resolution dense CRF (10 iterations, scale 1),
    arg-max — inference.predict_mask_ms on synthetic VOC-sized images (375 x 500), random-init VGG16-ASPP in eval mode.  Only the
    (H, W) mask crosses PCIe.  CPU side: the reference runs its forwards in Caffe on a GPU and ONLY the CRF on the CPU
    (krahenbuhl2013.CRF); the baseline is the oracle's CRF on the log-probabilities of the same pipeline."""
    from dsrg_amd import synthetic as S
    from dsrg_amd.backbone import VGG16ASPP, count_flops_per_image
    from dsrg_amd import inference as I
    # (no online GEMM tuning here: three input sizes at batch 1 are ~60 GEMM shapes, each tuned for seconds the first time it is
    # seen — a one-off cost a 10 582-image run amortises, but one that would BE this bounded record; hipBLASLt's own heuristic
    # picks the solutions instead)
    try:
        torch.cuda.tunable.enable(False)
        torch.cuda.tunable.tuning_enable(False)
    except Exception:
        pass
    torch.manual_seed(0)
    net = VGG16ASPP().to(device).to(memory_format=torch.channels_last).eval()
    H, W = 375, 500
    rng = np.random.default_rng(4242)
    imgs = []
    for k in range(4):
        img = S.make_images(rng, 1, size=max(H, W), kind=["smooth", "noise", "dark_corner", "smooth"][k])[0, :, :H, :W] + S.MEAN_PIXEL[:, None, None]
        imgs.append(np.ascontiguousarray(np.transpose(img, (1, 2, 0))[:, :, ::-1]).clip(0, 255).astype(np.uint8))     # RGB uint8, as PIL hands it over

    # the three forwards as captured HIP graphs (inference.GraphedForward: their input shapes are fixed by test-ms.py's resize);
    # DSRG_TEST_MS_GRAPH=0: launch by launch, as before (1.4 ms per forward whatever the size: host-bound)
    graphed = os.environ.get("DSRG_TEST_MS_GRAPH", "1") != "0"
    fwd = I.GraphedForward(net) if graphed else None

    def one(i):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            return I.predict_mask_ms(net, imgs[i % len(imgs)], smooth=True, device=device, forward=fwd)
    for i in range(warmup):
        one(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        mask = one(i)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if dump is not None:
        dump["mask"] = np.asarray(mask)
    # the same loop with the CRFs of earlier images in flight under the next image's forwards (inference.predict_masks_ms_many): how
    # a whole split (1 449 / 10 582 images) is run
    npipe = max(64, steps)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        n_fl, n_b = int(os.environ.get("DSRG_TEST_MS_INFLIGHT", "3")), int(os.environ.get("DSRG_TEST_MS_BATCH", "1"))       # tools: A/B
        for _ in I.predict_masks_ms_many(net, [imgs[i % len(imgs)] for i in range(8)], device=device, forward=fwd, in_flight=n_fl, batch=n_b):
            pass
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in I.predict_masks_ms_many(net, [imgs[i % len(imgs)] for i in range(npipe)], device=device, forward=fwd, in_flight=n_fl, batch=n_b):
            pass
        torch.cuda.synchronize()
        pipelined = npipe / (time.perf_counter() - t0)
    # the parts, each timed on its own (events): the three forwards + zooms + softmax, and the CRF + arg-max
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        e[0].record()
        for i in range(5):
            probs = I._probs_from_scores(I.multiscale_scores(net, imgs[i % len(imgs)], device=device, forward=fwd))
        e[1].record()
        unary = torch.log(probs).permute(1, 2, 0).contiguous()
        img_t = torch.as_tensor(imgs[0], device=device)
        from dsrg_amd.crf import CRF_device
        for i in range(5):
            CRF_device(img_t, unary, scale_factor=1.0, want="map")
        e[2].record()
    torch.cuda.synchronize()
    fwd_ms, crf_ms = e[0].elapsed_time(e[1]) / 5, e[1].elapsed_time(e[2]) / 5
    flops = sum(count_flops_per_image(sz) for sz in (241, 321, 401))
    rec = {"metric": "images/sec multi-scale test-time prediction (test-ms.py:84-111: 3 forwards + zoom + sum + softmax + full-resolution "
                     "dense CRF + arg-max, %dx%d image, 21 labels)" % (H, W),
           "value": steps / dt, "unit": "images/s", "n_gpus": 1, "steps": steps, "warmup": warmup, "ms_per_step": dt / steps * 1e3,
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
           "dtype": "bf16 backbone forwards (fp32 heads), f64 zoom, f32 CRF", "data": "synthetic",
           "config": {"workload": "inference.predict_mask_ms: scales 241/321/401, CRF scale_factor 1, maxiter 10, one image per step"},
           "forwards_zoom_softmax_ms": fwd_ms, "crf_argmax_ms": crf_ms, "forwards_as_hip_graphs": graphed,
           "images_per_s_crfs_in_flight": pipelined,
           "roofline": {"kernel": "the three VGG16-ASPP forwards (batch 1: 18-55 pixel tiles per layer; replayed as HIP graphs, tile-quantisation-bound)",
                        "bound": "mfma", "achieved": flops / (fwd_ms * 1e-3) / 1e12, "peak": 2500.0, "unit": "TFLOP/s",
                        "frac": flops / (fwd_ms * 1e-3) / 1e12 / 2500.0, "traffic": None,
                        "note": "the CRF half has its own record and roofline: modes.crf_fullres"},
           "labels_in_mask": int(len(np.unique(mask)))}
    if cpu:
        from oracle import oracle as O
        un_np = unary.float().cpu().numpy()
        t0 = time.perf_counter()
        want = O.CRF(imgs[0], un_np, scale_factor=1.0)
        t_cpu = time.perf_counter() - t0
        got = CRF_device(img_t, unary, scale_factor=1.0).cpu().numpy()
        rec["cpu_baseline"] = {"value": 1.0 / t_cpu, "unit": "images/s (the CRF alone: the reference's forwards run in Caffe on a GPU)",
                               "cores": 1, "kind": "port",
                               "sample": "1 image %dx%d, oracle/dsrg_oracle.c CRF single-threaded, %.2f s" % (H, W, t_cpu)}
        rec["max_abs_dq_vs_oracle"] = float(np.abs(got - want).max())
    del net
    return rec


def infer_record(device, rank, B, steps, warmup, use_graph=True, dump=None):
    """BASELINE.json configs[1]: VGG16-ASPP forward (bf16 autocast, fp32 heads, eval mode) + Softmax + dense CRF + seeded
    region growing on the network's own scores, no losses, no backward — the inference-only supervision path."""
    from dsrg_amd import ops, synthetic as S
    from dsrg_amd.backbone import VGG16ASPP, count_flops_per_image
    batch_np = S.make_batch(1000 + rank, B)
    images = torch.from_numpy(batch_np["images"]).to(device)
    labels = torch.from_numpy(batch_np["labels"]).to(device)
    cues = torch.from_numpy(batch_np["cues"]).to(device)
    torch.manual_seed(0)
    net = VGG16ASPP().to(device).to(memory_format=torch.channels_last).eval()
    ctx = ops.get_context(B, 21, 41, 41)
    x = images.contiguous(memory_format=torch.channels_last)
    side = torch.cuda.Stream(device=device)

    # The forward at batch 1 is ~150 launches of 3-30 us: launch-bound.  Its shapes, weights and input buffer are static, so it
    # is captured once into a hipGraph (torch.cuda.CUDAGraph: the HIP kernels take torch's current stream, which is the
    # capture stream) and replayed per image; --no-graph keeps the eager launches.  Eager warm-up first: TunableOp picks its
    # GEMM solutions and the kernels reserve their LDS outside the capture.
    graph, graph_note = None, "eager"
    if use_graph:
        try:
            from dsrg_amd.backbone import GraphedForward
            graph = GraphedForward(net, x)
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                same = torch.equal(graph(x), net(x).contiguous())                # eval mode: the replay must reproduce the eager scores
            if not same:
                raise RuntimeError("replayed scores differ from the eager forward")
            graph_note = "hipGraph replay of the backbone forward (scores bit-identical to the eager launches)"
        except Exception as e:                                   # noqa: BLE001 - report and fall back to eager launches
            graph, graph_note = None, "eager (capture failed: %s)" % str(e)[:120]

    @torch.no_grad()
    def one(replay_forward=True):
        # the bilateral lattices depend only on the image: built on a side stream underneath the backbone forward
        main = torch.cuda.current_stream()
        side.wait_stream(main)
        with torch.cuda.stream(side):
            ops.crf_prepare(images, 21, 41, 41, ctx=ctx)
        if graph is not None and replay_forward:
            scores = graph(x)
        else:
            with torch.autocast("cuda", dtype=torch.bfloat16):
                scores = net(x)
        probs = ops.softmax_forward(scores.contiguous())
        main.wait_stream(side)
        refined, _ = ops.crf_refine(probs, images, ctx=ctx, want_log=False, prepared=True)
        return ops.srg_grow(labels, cues, refined)
    for _ in range(warmup):
        one()
    torch.cuda.synchronize()
    # the WHOLE step as one graph (forward replay + lattice build on the side stream + softmax + mean field + region growing: the
    # supervision path sizes everything for the worst case and never asks the host anything, so it captures as it is): tried when
    # DSRG_INFER_STEP_GRAPH=1 (tools: A/B); the results must equal the launch-by-launch step's
    step_graph = None
    if use_graph and os.environ.get("DSRG_INFER_STEP_GRAPH", "0") == "1":
        try:
            want = one().clone()
            torch.cuda.synchronize()
            g2 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g2):
                out2 = one(replay_forward=False)                 # (a graph cannot replay another while it is being captured: the forward is captured again, in line)
            g2.replay()
            torch.cuda.synchronize()
            if not torch.equal(out2, want):
                raise RuntimeError("replayed step differs")
            step_graph = g2
            graph_note += "; whole step (lattice build, softmax, CRF, SRG) replayed as one graph too"
        except Exception as e:                                   # noqa: BLE001
            graph_note += "; whole-step capture failed: %s" % str(e)[:160]
    if step_graph is not None:
        def one(replay_forward=True):                            # noqa: F811
            step_graph.replay()
            return out2
    t0 = time.perf_counter()
    for _ in range(steps):
        seeds = one()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if dump is not None:
        dump["seeds"] = seeds.float()                            # a copy: the context's buffers are reused below
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    lg = torch.from_numpy(batch_np["logits"]).to(device)
    e0.record()
    for _ in range(10):
        probs = ops.softmax_forward(lg)
        refined, _ = ops.crf_refine(probs, images, ctx=ctx, want_log=False)
        ops.srg_grow(labels, cues, refined)
    e1.record()
    torch.cuda.synchronize()
    del net, graph
    return {"metric": "images/sec VGG16-ASPP forward + Softmax + dense CRF + SRG (inference-only supervision path, 321x321, 21-class)",
            "value": B * steps / dt, "unit": "images/s", "n_gpus": 1, "steps": steps, "warmup": warmup,
            "ms_per_step": dt / steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "bf16 backbone forward (fp32 heads) + f32/f64 CRF and SRG", "data": "synthetic",
            "config": {"workload": "BASELINE.json configs[1]: backbone forward + CRF (10 it, scale 12) + SRG, batch %d" % B,
                       "per_gpu_batch": B},
            "backbone_launch": graph_note,
            "supervision_only_ms": e0.elapsed_time(e1) / 10,
            "backbone_forward_tflops": count_flops_per_image() * B * steps / dt / 1e12,
            "grown_seed_pixels": int(seeds.sum().item() - cues.sum().item())}


def filter_roofline(ctx, B, C, N, filt_ms, filt_n, ev_overhead_ms):
    """roofline object of mf_filter_kernel from a HIP-event-bracketed pass (dsrg_ctx_profile_start/stop).  The lattice values
    never leave LDS between splat and slice, so the roof that binds this kernel is LDS bandwidth, not HBM: bytes through LDS
    per launch from the instruction mix (lds_filter_traffic, measured M and X per image) against the per-instruction rates of
    MI355X_MICROARCH.md (reads and writes have different rates: the peak is the byte-weighted blend)."""
    mg, mb = ctx.lattice_sizes(B)
    xg, xb = ctx.lattice_extras(B)
    gflags_local = mg == 3 * N and xg == 0                      # pixel-local at training scale (M = 3 N private vertices)
    raw_launch_us = filt_ms / filt_n * 1e3
    per_launch_s = (filt_ms / filt_n - ev_overhead_ms) * 1e-3
    alg_bytes = sum(filter_bytes(2, mg, C, N) + filter_bytes(5, m, C, N) for m in mb)   # SURVEY 8d, one filter launch
    cpw_b, cpw_g, plan_wgs, plan_lds = ctx.filter_plan(B)      # what the launcher does, not a copy of its rules
    groups_b, groups_g = (C + cpw_b - 1) // cpw_b, (C + cpw_g - 1) // cpw_g
    rd = sum(lds_filter_traffic(5, m, x, N, cpw_b)[0] for m, x in zip(mb, xb)) * groups_b
    wr = sum(lds_filter_traffic(5, m, x, N, cpw_b)[1] for m, x in zip(mb, xb)) * groups_b
    insts = sum(lds_filter_instructions(5, m, x, N) for m, x in zip(mb, xb)) * groups_b
    rate_r = LDS_RATE_GBS["read_b64" if cpw_b == 2 else "read_b32"]
    rate_w = LDS_RATE_GBS["write_b64" if cpw_b == 2 else "write_b32"]
    t_peak = rd / rate_r + wr / rate_w
    gauss_rd = gauss_wr = 0
    if not gflags_local:                                        # the Gaussian workgroups ride in the same launch
        g_r, g_w = lds_filter_traffic(2, mg, xg, N, cpw_g)
        gauss_rd, gauss_wr = g_r * groups_g * B, g_w * groups_g * B
        t_peak += gauss_rd / LDS_RATE_GBS["read_b128" if cpw_g == 4 else "read_b64"] + \
            gauss_wr / LDS_RATE_GBS["write_b128" if cpw_g == 4 else "write_b64"]
        insts += lds_filter_instructions(2, mg, xg, N, vpt=5) * groups_g * B
    total = rd + wr + gauss_rd + gauss_wr
    lds_peak = total / t_peak
    lds_achieved = total / per_launch_s / 1e9
    tj, traffic_src = _counter_file("pmc_traffic", "mf_filter_kernel")
    traffic = (tj or {}).get("mf_filter_kernel_bytes_per_launch")       # None when the kernel changed after the PMC pass
    counters = None
    cj, counters_src = _counter_file("lds_counters", "mf_filter_kernel")
    if cj and int(cj.get("batch", 16)) != B:
        # the PMC pass ran the 16-image step: its per-launch counters say nothing about a launch over B images
        cj, counters_src = None, dict(counters_src or {}, dropped="counters collected at batch %d, this record is batch %d" % (int(cj.get("batch", 16)), B))
    if cj:
        ck = sorted((v for k, v in cj.get("kernels", {}).items() if "mf_filter_kernel" in k),
                    key=lambda v: -v.get("launches", 0))          # the loop's instantiation, not the build's norm pass
        if ck:
            counters = {k: ck[0].get(k) for k in ("SQ_LDS_IDX_ACTIVE", "SQ_LDS_BANK_CONFLICT", "SQ_INSTS_LDS", "SQ_WAIT_INST_LDS",
                                                  "SQ_WAVE_CYCLES", "lds_conflict_share", "avg_duration_us_under_pmc")}
            counters["collected_at_commit"] = cj.get("commit")
            if counters.get("SQ_LDS_IDX_ACTIVE") and counters.get("avg_duration_us_under_pmc"):
                counters["lds_array_busy_frac_at_2.4GHz"] = counters["SQ_LDS_IDX_ACTIVE"] / (
                    256 * counters["avg_duration_us_under_pmc"] * 1e-6 * 2.4e9)
            if counters.get("SQ_INSTS_LDS"):
                counters["model_insts_over_counter"] = insts / counters["SQ_INSTS_LDS"]
    return {"kernel": "mf_filter_kernel (permutohedral splat/blur/slice: %d bilateral lattices x %d label planes%s)" % (
                B, C, "; the pixel-local Gaussian lattice is evaluated by the update kernel" if gflags_local
                else " + the Gaussian lattice x %d planes x %d images" % (C, B)),
            "bound": "lds", "achieved": lds_achieved, "peak": lds_peak, "unit": "GB/s",
            "frac": lds_achieved / lds_peak, "traffic": traffic, "traffic_source": traffic_src,
            "lds_counters_source": counters_src,
            "lds_read_bytes_per_launch": rd + gauss_rd, "lds_write_bytes_per_launch": wr + gauss_wr,
            "lds_bytes_gaussian_workgroups": gauss_rd + gauss_wr,
            "lds_wave_instructions_model": insts,
            "lds_peak_read_gbs": rate_r, "lds_peak_write_gbs": rate_w,
            "us_per_launch": per_launch_s * 1e6, "launches": filt_n,
            "us_per_launch_event_bracket": raw_launch_us, "event_bracket_overhead_us": ev_overhead_ms * 1e3,
            "workgroups_with_lds_work": groups_b * B + (0 if gflags_local else groups_g * B), "cus": 256,
            "launch_plan": {"planes_per_bilateral_workgroup": cpw_b, "planes_per_gaussian_workgroup": cpw_g,
                            "workgroups_in_grid": plan_wgs, "dynamic_lds_bytes": plan_lds},
            "lds_counters_per_launch": counters,
            "hbm_model": {"alg_bytes_per_launch": alg_bytes, "gbs": alg_bytes / per_launch_s / 1e9,
                          "frac_of_8TBs": alg_bytes / per_launch_s / 1e9 / HBM_PEAK_GBS,
                          "note": "SURVEY 8d stage-streamed bytes / time: a labelled secondary, NOT a roofline — "
                                  "the values stay in LDS, so this ratio exceeds 1"},
            "hbm_gbs_from_pmc_traffic": (traffic / per_launch_s / 1e9) if traffic else None,
            "lattice_M_gauss": mg, "lattice_M_bilateral_mean": float(np.mean(mb)), "splat_extras_bilateral_mean": float(np.mean(xb)),
            "note": "achieved = modelled LDS bytes per launch / HIP-event time per launch (events on the launch stream, "
                    "empty-bracket cost subtracted); traffic = HBM bytes per launch from the FETCH_SIZE/WRITE_SIZE passes"}


def srg_roofline(ops, B, C, N, logits, images, labels, cues, ctx):
    """the region-growing kernels on their own (north_star asks for their HBM rate too): one bracket around 20 calls"""
    refined, _ = ops.crf_refine(ops.softmax_forward(logits), images, ctx=ctx, want_log=False)
    for _ in range(3):
        ops.srg_grow(labels, cues, refined)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        ops.srg_grow(labels, cues, refined)
    e1.record()
    torch.cuda.synchronize()
    srg_us = e0.elapsed_time(e1) / 20 * 1e3
    pj, srg_src = _counter_file("pmc_traffic", "srg")
    pmc = (pj or {}).get("kernels", {})
    srg_bytes = 16 * C * N * B                  # cues + fp64 marginals in, seeds out, per image
    tr = sum(v.get("hbm_bytes_per_launch", 0) for k, v in pmc.items() if "srg_" in k) or None
    return {"kernel": "srg_classify_kernel + srg_grow_kernel (seeded region growing, %d images)" % B, "bound": "hbm",
            "achieved": srg_bytes / (srg_us * 1e-6) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": srg_bytes / (srg_us * 1e-6) / 1e9 / HBM_PEAK_GBS, "traffic": tr, "traffic_source": srg_src,
            "alg_bytes_per_launch": srg_bytes, "us_per_launch": srg_us,
            "note": "two dependent launches (pixel-parallel classification over the batch, then one workgroup per image for the "
                    "growth): the time is two kernel boundaries plus one memory round trip each, not bandwidth"}


def supervision_record(device, rank, B, steps, warmup, cpu=True, cpu_target_s=10.0, size=321, dump=None):
    """the supervision path on fixed fc8 logits: Softmax -> CRF -> SRG -> losses -> backward (dsrg_supervision_step); size = the
    input images' side: 321 -> 41 x 41 score maps (train-s), 513 -> 65 x 65 (the ResNet-101 / 513 configuration's map size)"""
    from dsrg_amd import ops, synthetic as S
    C = 21
    H = W = (size - 1) // 8 + 1
    N = H * W
    batch_np = S.make_batch(1000 + rank, B, C, H, W, size=size)
    d = lambda a: torch.from_numpy(a).to(device)                 # noqa: E731
    logits, images, labels, cues = d(batch_np["logits"]), d(batch_np["images"]), d(batch_np["labels"]), d(batch_np["cues"])
    ctx = ops.get_context(B, C, H, W)
    for _ in range(warmup):
        ops.supervision_step(logits, images, labels, cues, ctx=ctx)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        losses, grad, _ = ops.supervision_step(logits, images, labels, cues, ctx=ctx)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if dump is not None:
        dump.update(losses=losses.clone(), grad_logits=grad.clone())      # copies: the profiling pass below reuses the buffers
    nprof = max(3, min(steps, 20))
    ctx.profile_start(nprof * 10 + 16)                           # the filter launches bracketed in a separate, untimed pass
    for _ in range(nprof):
        ops.supervision_step(logits, images, labels, cues, ctx=ctx)
    torch.cuda.synchronize()
    filt_ms, filt_n = ctx.profile_stop()
    rec = {"metric": "images/sec DSRG supervision path only (softmax+CRF+SRG+losses+backward)",
           "value": B * steps / dt, "unit": "images/s", "n_gpus": 1, "steps": steps, "warmup": warmup,
           "ms_per_step": dt / steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
           "dtype": "f32 (thresholds and marginals f64)", "data": "synthetic",
           "config": {"workload": "supervision path on fixed fc8 logits, %dx%dx21, CRF 10 iterations scale 12" % (H, W), "per_gpu_batch": B},
           "losses": [float(x) for x in losses.detach().cpu()],
           "roofline": filter_roofline(ctx, B, C, N, filt_ms, filt_n, event_overhead_ms()) if filt_n else None,
           "other_rooflines": [srg_roofline(ops, B, C, N, logits, images, labels, cues, ctx)]}
    if cpu:
        rec["cpu_baseline"] = cpu_baseline(batch_np, target_s=cpu_target_s)
    return rec


def fp32_leg(device, images, labels, cues, steps, warmup=3):
    """the same train-s step with the backbone in float32 (the reference's Caffe arithmetic, train-s.prototxt:41-744):
    ms per step at this batch size, timed like the headline (synchronised brackets)"""
    from dsrg_amd.trainer import DSRGTrainer
    tr = DSRGTrainer(device, amp_dtype=None)
    for _ in range(warmup):
        tr.step(images, labels, cues)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        losses = tr.step(images, labels, cues)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    del tr
    return dt, [float(x) for x in losses]


def loss_trajectories(device, images, labels, cues, steps=300):
    """bf16-autocast backbone vs float32 backbone: same initial weights, same batch, `steps` steps of the solver, Dropout off (the
    bf16 leg draws its masks inside the convolutions' epilogues from a counter-based generator, the float32 leg from torch's: with
    Dropout on the two trajectories would differ by their masks, not by their arithmetic; tools/overfit_probe.py prints both);
    -> (bf16 totals, fp32 totals, relative gaps of the total loss per step)"""
    from dsrg_amd.backbone import VGG16ASPP
    from dsrg_amd.trainer import DSRGTrainer
    out = []
    for amp in (torch.bfloat16, None):
        torch.manual_seed(123)
        tr = DSRGTrainer(device, amp_dtype=amp, seed=123, net=VGG16ASPP(dropout=0.0))
        tot = [tr.step(images, labels, cues).detach() for _ in range(steps)]
        out.append(torch.stack(tot).sum(1).cpu().numpy().astype(np.float64))
        del tr
        torch.cuda.empty_cache()
    a, b = out
    return a, b, np.abs(a - b) / np.maximum(np.abs(b), 1e-12)


def precision_legs(device, images, labels, cues, B):
    """what `legs` says about the bf16 step against the reference's float32 step, beyond their speeds (round-4 review item 2):
    grad_cosine_min — the smallest per-parameter cosine between the bf16 route's gradient and the float32 backbone's, at an
      ImageNet-scale initialisation, on this batch size, same score gradient fed to both (dsrg_amd/fidelity.py), with the
      yardstick beside it: the same float32 gradient after the weights alone were rounded to bf16 once;
    loss_gap_300_steps — both legs trained for 300 solver steps from the same weights on the same batch, Dropout off: the
      largest and the final relative gap of the total loss, and both trajectories sampled every 20 steps."""
    from dsrg_amd.fidelity import gradient_fidelity
    rec = {}
    r = gradient_fidelity(B, ("bf16", "f32,w16"))
    worst = min(r["cos"]["bf16"], key=r["cos"]["bf16"].get)
    rec["grad_cosine_min"] = r["cos"]["bf16"][worst]
    rec["grad_cosine_min_parameter"] = worst
    rec["grad_cosine_whole_gradient"] = r["cos_all"]["bf16"]
    rec["grad_cosine_min_f32_with_bf16_rounded_weights"] = min(r["cos"]["f32,w16"].values())
    rec["grad_cosine_note"] = ("per-parameter cosine to the float32 backbone's gradient, Kaiming-scale init, batch %d, Dropout off; "
                               "the yardstick leg is float32 arithmetic with the weights rounded to bf16 once" % B)
    torch.cuda.empty_cache()
    t16, t32, gap = loss_trajectories(device, images, labels, cues)
    rec["loss_gap_300_steps"] = {"max": float(gap.max()), "final": float(gap[-1]), "mean_last_30": float(gap[-30:].mean())}
    rec["loss_trajectory_bf16"] = [float(v) for v in t16[::20]] + [float(t16[-1])]
    rec["loss_trajectory_fp32"] = [float(v) for v in t32[::20]] + [float(t32[-1])]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=None, help="images per GPU (weak scaling); default 16, 1 for --mode infer")
    ap.add_argument("--mode", choices=["train", "supervision", "train-f", "crf-fullres", "infer", "test-ms"], default="train",
                    help="train = seed_mc train-s step (the headline metric; on one GPU the line also carries bounded "
                         "sub-records of the other quoted configurations under `modes`); supervision = hot path on fixed "
                         "logits; infer = BASELINE.json configs[1]; crf-fullres = test-time CRF at image resolution; "
                         "train-f = stage-2 retrain step (no SRG/CRF inside; BASELINE.json configs[4] with "
                         "--backbone resnet101 --size 513)")
    ap.add_argument("--backbone", choices=["vgg16", "resnet101"], default="vgg16")
    ap.add_argument("--size", type=int, default=321)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-fp32", action="store_true", help="skip the float32-backbone leg and the bf16/fp32 loss trajectories")
    ap.add_argument("--no-modes", action="store_true", help="--mode train: skip the sub-records of the other configurations")
    ap.add_argument("--no-graph", action="store_true", help="--mode infer: launch the backbone forward eagerly instead of replaying a hipGraph")
    ap.add_argument("--no-profile", action="store_true", help="do not bracket filter launches with HIP events")
    ap.add_argument("--sub", action="store_true", help="(internal) a sub-record of the --full run: short CPU baseline, one core only")
    ap.add_argument("--full", action="store_true",
                    help="--mode train: also the filter roofline pass, the float32 leg and precision comparison, the CPU baselines, "
                         "the sub-records of the other configurations and the weight checksum of a single process (a plain "
                         "run times the headline only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed as DIR/<name>.npy (rank 0)")
    args = ap.parse_args()

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X; there is no CPU fallback for the hot path")
    # torch sizes its intra-op pool by the machine's cores (128 on the GPU boxes); the idle spin of those threads after any host-side
    # parallel op counts against a container's CPU quota (cgroup cpu.max) and the launch thread is then throttled for up to 100 ms
    # (measured: test-time prediction 7 ms -> 95 ms per image).  Nothing on the timed paths needs host parallelism.
    torch.set_num_threads(min(torch.get_num_threads(), 8))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # started as plain `python bench.py --gpus N`: become the launcher — one rank per GPU under torch.distributed.run
        # (what the driver's own N>1 launch line does), same arguments, rendezvous on the loopback address
        visible = torch.cuda.device_count()
        if visible < args.gpus:
            raise SystemExit("bench.py --gpus %d: only %d GPU(s) visible on this node" % (args.gpus, visible))
        import socket
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        sys.stdout.flush()
        import subprocess
        raise SystemExit(subprocess.call(cmd))            # a child process: this one has the HIP runtime up already
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world and (args.gpus > 1 or world > 1):
        raise SystemExit("bench.py --gpus %d under a launcher with WORLD_SIZE=%d: start it with --nproc-per-node %d" % (
            args.gpus, world, args.gpus))
    if local_rank >= torch.cuda.device_count():
        raise SystemExit("bench.py: rank %d has no GPU (%d visible)" % (local_rank, torch.cuda.device_count()))
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    dist = None
    # under torch.distributed.run (RANK set) the process group and the gradient reducer (dsrg_amd/reducer.py) are set up even for one
    # rank, so the single-GPU run of the driver's launch line goes through the code the 8-GPU run goes through (at one rank the
    # bucket all-reduces themselves are skipped — nothing to reduce; barrier, timing gather and the weight checksums use RCCL)
    use_dist = world > 1 or (os.environ.get("RANK") is not None and os.environ.get("DSRG_BENCH_NO_DDP") is None)
    if use_dist:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=device)      # nccl == RCCL on ROCm

    def finish():
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()

    cpu = not args.no_cpu_baseline and world == 1
    if args.batch is None:
        args.batch = 1 if args.mode == "infer" else 16
    dump = {} if args.dump_outputs and rank == 0 else None
    if args.mode == "crf-fullres":
        rec = crf_fullres_record(device, args.steps, args.warmup, cpu=cpu, size=args.size, dump=dump)
        if rank == 0:
            if dump is not None:
                write_outputs(args.dump_outputs, dump)
            print(json.dumps(rec))
        return finish()
    if args.mode == "test-ms":
        rec = test_ms_record(device, args.steps, args.warmup, cpu=cpu, dump=dump)
        if rank == 0:
            if dump is not None:
                write_outputs(args.dump_outputs, dump)
            print(json.dumps(rec))
        return finish()
    if args.mode == "infer":
        rec = infer_record(device, rank, args.batch, args.steps, args.warmup, use_graph=not args.no_graph, dump=dump)
        if rank == 0:
            if dump is not None:
                write_outputs(args.dump_outputs, dump)
            print(json.dumps(rec))
        return finish()
    if args.mode == "supervision":
        rec = supervision_record(device, rank, args.batch, args.steps, args.warmup, cpu=cpu, cpu_target_s=5.0 if args.sub else 10.0,
                                 size=args.size, dump=dump)
        if rank == 0:
            if dump is not None:
                write_outputs(args.dump_outputs, dump)
            if cpu and not args.sub:
                try:
                    rec["cpu_baseline_all_cores"] = cpu_baseline_all_cores()
                except Exception as e:                   # never let the extra baseline cost the bench line
                    rec["cpu_baseline_all_cores"] = {"error": str(e)[:200]}
            print(json.dumps(rec))
        return finish()

    from dsrg_amd import ops, synthetic as S
    from dsrg_amd.backbone import count_flops_per_image
    from dsrg_amd.trainer import DSRGTrainer

    B, C, H, W = args.batch, 21, 41, 41
    N = H * W
    batch_np = S.make_batch(1000 + rank, B)                     # each rank its own shard of the global batch
    images = torch.from_numpy(batch_np["images"]).to(device)
    labels = torch.from_numpy(batch_np["labels"]).to(device)
    cues = torch.from_numpy(batch_np["cues"]).to(device)
    logits_fixed = torch.from_numpy(batch_np["logits"]).to(device)
    ctx = ops.get_context(B, C, H, W)

    trainer = DSRGTrainer(device, world_size=world, ddp=use_dist) if args.mode == "train" else None
    retrainer = None
    if args.mode == "train-f":
        from dsrg_amd.retrain import RetrainTrainer
        retrainer = RetrainTrainer(device, world_size=world, ddp=use_dist, backbone=args.backbone)
        g = torch.Generator(device="cpu").manual_seed(2000 + rank)
        f_images = torch.randn(B, 3, args.size, args.size, generator=g).to(device)
        f_label = torch.randint(0, 21, (B, 1, args.size, args.size), generator=g).float().to(device)

    def one_step():
        if retrainer is not None:
            return retrainer.step(f_images, f_label).reshape(1)
        return trainer.step(images, labels, cues)

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        one_step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        losses = one_step()
    barrier()
    dt = time.perf_counter() - t0
    rank_ms = [dt / args.steps * 1e3]
    if dist is not None:
        ts = [torch.zeros(1, dtype=torch.float64, device=device) for _ in range(world)]
        dist.all_gather(ts, torch.tensor([dt], dtype=torch.float64, device=device))
        rank_ms = [float(t.item()) / args.steps * 1e3 for t in ts]
        dt = max(float(t.item()) for t in ts)                     # the job's time is its slowest rank's

    # what the last timed step computed, before any further step moves the weights: its losses and the parameters it updated
    if dump is not None:
        dump["losses" if retrainer is None else "loss"] = losses.float()
        dump.update(param_sample((retrainer or trainer).net))
        write_outputs(args.dump_outputs, dump)

    # replicas in lock step?  every rank all-gathers a 64-bit checksum pair of its parameters and momentum buffers (a
    # data-parallel number is only a number if the ranks still hold the same weights); outside the timed region.  A single process
    # has nothing to compare: there the checksum is one of the --full extras
    weights_equal, weight_words = None, None
    if trainer is not None and (dist is not None or args.full):
        weights_equal, weight_words = trainer.weights_equal_across_ranks()

    # the dominant hot-path kernel inside the train step: a separate, untimed pass with every filter launch bracketed by HIP
    # events on its launch stream (the brackets cost ~5 us each: they must not sit in the timed region)
    filt_ms, filt_n, ev_overhead = 0.0, 0, 0.0
    if args.mode == "train" and args.full and not args.no_profile:
        nprof = max(3, min(args.steps, 10))
        ctx.profile_start(nprof * 10 + 16)
        for _ in range(nprof):
            one_step()
        torch.cuda.synchronize()
        filt_ms, filt_n = ctx.profile_stop()
        ev_overhead = event_overhead_ms()

    # supervision-only time per step on this rank (same inputs; untimed region)
    sup_ms = None
    if args.mode == "train" and args.full:
        for _ in range(3):
            ops.supervision_step(logits_fixed, images, labels, cues, ctx=ctx)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            ops.supervision_step(logits_fixed, images, labels, cues, ctx=ctx)
        e1.record()
        torch.cuda.synchronize()
        sup_ms = e0.elapsed_time(e1) / 10

    if rank == 0:
        total_images = B * world * args.steps
        other = []
        if args.mode == "train":
            if args.full:
                other.append(srg_roofline(ops, B, C, N, logits_fixed, images, labels, cues, ctx))
            tf = count_flops_per_image() * 3 * B * world * args.steps / dt / 1e12 / world
            other.append({"kernel": "backbone convolutions (hipBLASLt / MIOpen / CK / own direct kernels, MFMA bf16), whole step per GPU",
                          "bound": "mfma", "achieved": tf, "peak": 2500.0, "unit": "TFLOP/s", "frac": tf / 2500.0,
                          "traffic": None, "note": "3 x forward flops of the conv stack / step time (supervision, "
                                                   "pooling, optimizer included in the time)"})
        if args.mode == "train-f":
            from dsrg_amd.retrain import count_flops_per_image_resnet101
            fl = count_flops_per_image(args.size) if args.backbone == "vgg16" else count_flops_per_image_resnet101(args.size)
            tf = fl * 3 * B * world * args.steps / dt / 1e12 / world
            trainf_roofline = {"kernel": "backbone convolutions of the train-f step (implicit-GEMM / direct MFMA kernels of this repo; "
                                         "%s), whole step per GPU" % ("every convolution" if args.backbone == "vgg16" else
                                                                      "every stride-1 bottleneck convolution and the ASPP head, shortcut "
                                                                      "adds and ReLU backward in the convolutions' stores, data + weight "
                                                                      "gradient in one grid; the 7x7 stem, res3's two stride-2 layers and "
                                                                      "their gradients stay on MIOpen"),
                               "bound": "mfma", "achieved": tf, "peak": 2500.0, "unit": "TFLOP/s", "frac": tf / 2500.0, "traffic": None,
                               "flops_per_image_forward": fl,
                               "note": "3 x forward flops of the conv stack / step time (loss, pooling, residual adds, optimizer "
                                       "included in the time); per-kernel times: profiles/r06_train_f_*_kernel_stats.txt"}
        out = {
            "metric": "images/sec DSRG train step (VGG16 321x321, 21-class)" if args.mode == "train"
                      else "images/sec train-f retrain step (%s %dx%d, softmax loss on pseudo-labels)" % (args.backbone, args.size, args.size),
            "value": total_images / dt, "unit": "images/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None,
            "dtype": ("bf16 backbone (fp32 master weights) + f32/f64 supervision path" if args.mode == "train" else
                      "bf16 backbone (fp32 master weights), f32 loss"),
            "data": "synthetic",
            "config": {"workload": ("full seed_mc train-s step: VGG16-ASPP fwd+bwd + Softmax/CRF(10 it, scale 12)/"
                                    "SRG/BalancedSeedLoss/ConstrainLoss + SGD, 321x321 -> 41x41x21"
                                    if args.mode == "train" else
                                    "train-f step: %s fwd+bwd + Interp(1/8) + SoftmaxWithLoss + SGD(poly), %dx%d" % (
                                        args.backbone, args.size, args.size)),
                       "per_gpu_batch": B, "global_batch": B * world, "parallelism": "dp%d" % world,
                       "baseline_config": "configs[2] (batch 16 on 1 GPU); configs[3] at 8 GPUs"},
            "rccl_ranks": dist.get_world_size() if dist is not None else 0,     # 0: no process group (plain single-GPU run)
            "weights_equal_across_ranks": weights_equal,                         # checksums all-gathered after the timed steps
            "weights_checksum_rank0": ("%016x" % (weight_words[0][0] & (2 ** 64 - 1))) if weight_words else None,
            "ms_per_step_ranks": {"min": min(rank_ms), "max": max(rank_ms)},
            "losses": [float(x) for x in losses.detach().cpu()],
            "supervision_ms_per_step": sup_ms,
            "backbone_tflops": (count_flops_per_image() * 3 * B * world * args.steps / dt / 1e12) if args.mode == "train" else None,
            "roofline": (filter_roofline(ctx, B, C, N, filt_ms, filt_n, ev_overhead) if filt_n else None) if args.mode == "train" else trainf_roofline,
            "other_rooflines": other,
        }
        if args.mode == "train-f":
            out["config"]["baseline_config"] = ("configs[4] (ResNet-101 DeepLab-v2, 513x513, train-f) on one GPU" if args.backbone == "resnet101"
                                                else "the reference's own stage 2: train-f.prototxt:3-14,721-755 + solver-f.prototxt:1-17 (VGG16-ASPP, 321x321)")
            out["cpu_baseline"] = None
            out["cpu_baseline_note"] = ("no CPU leg: the reference runs this step entirely inside Caffe on a GPU (no Python layer on "
                                        "the path, train-f.prototxt) — there is no reference CPU path to time")
        if args.mode == "train" and world == 1:
            out["legs"] = {"bf16": {"value": out["value"], "ms_per_step": out["ms_per_step"], "steps": args.steps,
                                    "dtype": out["dtype"], "backbone_tflops": out["backbone_tflops"],
                                    "mfma_peak_tflops": 2500.0, "mfma_frac": out["backbone_tflops"] / 2500.0}}
        if args.mode == "train" and world == 1 and args.full and not args.no_fp32:
            # the reference's backbone arithmetic is Caffe float32: the same step with a float32 backbone, for the SAME number
            # of timed steps, and how far the two loss trajectories drift apart
            del trainer
            torch.cuda.empty_cache()
            dt32, l32 = fp32_leg(device, images, labels, cues, args.steps)
            tf32 = count_flops_per_image() * 3 * B / dt32 / 1e12
            out["value_fp32"] = B / dt32
            out["ms_per_step_fp32"] = dt32 * 1e3
            # the reference's backbone precision is float32 (Caffe): the figure any comparison WITH THE REFERENCE quotes, kept in
            # fields the driver's record keeps (it drops keys it does not know)
            out["config"]["fp32_backbone_images_per_s"] = B / dt32
            out["config"]["fp32_backbone_ms_per_step"] = dt32 * 1e3
            out["dtype"] += "; float32-backbone leg (the reference's precision) %.1f images/s" % (B / dt32)
            out["legs"]["fp32"] = {"value": B / dt32, "ms_per_step": dt32 * 1e3, "steps": args.steps, "losses": l32,
                                   "dtype": "f32 backbone + f32/f64 supervision path", "backbone_tflops": tf32,
                                   "mfma_peak_tflops": 157.3, "mfma_frac": tf32 / 157.3,
                                   "note": "float32 is the reference's backbone precision (Caffe): any comparison with the "
                                           "reference quotes this leg; `value` is the bf16-autocast (fp32 master weights, fp32 "
                                           "classifier heads) leg — the MI355X-native configuration"}
            try:
                out["legs"].update(precision_legs(device, images, labels, cues, B))
                # (kept where the driver's record keeps it)
                out["config"]["bf16_vs_fp32_grad_cosine_min"] = out["legs"]["grad_cosine_min"]
                out["config"]["bf16_vs_fp32_loss_gap_300_steps_max"] = out["legs"]["loss_gap_300_steps"]["max"]
            except Exception as e:                       # never let the comparison cost the bench line
                out["legs"]["precision_legs_error"] = str(e)[:200]
        if args.mode == "train" and world == 1 and args.full and cpu:
            out["cpu_baseline"] = cpu_baseline(batch_np)
            try:
                out["cpu_baseline_all_cores"] = cpu_baseline_all_cores()
            except Exception as e:                       # never let the extra baseline cost the bench line
                out["cpu_baseline_all_cores"] = {"error": str(e)[:200]}
        else:
            out["cpu_baseline"] = None
        if args.mode == "train" and world == 1 and args.full and not args.no_modes:
            # the other quoted configurations, bounded, each with its own roofline and CPU baseline: driver-timed alongside
            # the headline (BASELINE.json configs[1]; the hot path alone at 16 images and at one).  Each runs
            # in a fresh process (this one keeps its GPU context but is idle): measured inside this process, after the
            # float32 leg, the launch-bound batch-1 inference came out 13 % slower than on its own.
            import subprocess
            trainer = None
            torch.cuda.empty_cache()
            modes = {}
            base = [sys.executable, os.path.abspath(__file__)]
            nocpu = [] if cpu else ["--no-cpu-baseline"]
            for name, argv in (("supervision", ["--mode", "supervision", "--batch", "16", "--steps", "200", "--warmup", "20", "--no-cpu-baseline"]),
                               ("supervision_b1", ["--mode", "supervision", "--batch", "1", "--steps", "200", "--warmup", "20", "--sub"] + nocpu),
                               ("supervision_65", ["--mode", "supervision", "--batch", "10", "--size", "513", "--steps", "100", "--warmup", "10",
                                                   "--no-cpu-baseline"]),
                               ("infer_b1", ["--mode", "infer", "--batch", "1", "--steps", "300", "--warmup", "30"]),
                               ("crf_fullres", ["--mode", "crf-fullres", "--steps", "20", "--warmup", "5"] + nocpu),
                               ("test_ms", ["--mode", "test-ms", "--steps", "30", "--warmup", "6"] + nocpu),
                               ("train_f", ["--mode", "train-f", "--backbone", "vgg16", "--size", "321", "--batch", "16", "--steps", "20",
                                            "--warmup", "6", "--no-cpu-baseline"]),
                               ("train_f_resnet101_513", ["--mode", "train-f", "--backbone", "resnet101", "--size", "513", "--batch", "10",
                                                          "--steps", "10", "--warmup", "5", "--no-cpu-baseline"])):
                try:
                    r = subprocess.run(base + argv, capture_output=True, text=True, timeout=420)
                    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
                    if r.returncode != 0 or not lines:
                        raise RuntimeError("rc %d: %s" % (r.returncode, r.stderr[-300:]))
                    modes[name] = json.loads(lines[-1])
                except Exception as e:                   # a sub-record must never cost the headline line
                    modes[name] = {"error": "%s: %s" % (type(e).__name__, str(e)[:300])}
            if "error" not in modes["supervision"] and isinstance(out.get("cpu_baseline"), dict):
                modes["supervision"]["cpu_baseline"] = out["cpu_baseline"]      # same workload: the port on the same batch
            out["modes"] = modes
        print(json.dumps(out))
    finish()
    if weights_equal is False:
        # every rank leaves with the same status: a scaling number from replicas that drifted apart is not a measurement
        raise SystemExit("bench.py: the ranks' weights differ after %d steps (checksums %s)" % (
            args.warmup + args.steps, ["%016x" % (w[0] & (2 ** 64 - 1)) for w in weight_words]))


if __name__ == "__main__":
    main()
