#!/usr/bin/env python
"""bench.py — pages/sec of the vision hot path on N MI355X (one process per GPU).

Metric (BASELINE.json): pages/sec (detect+segment+inpaint+upscale) 1024x1536 @1/2/4/8 MI355X.
A "step" is one synthetic 1024x1536 page through every stage of the hot path:
  detect   YOLOv8m-seg @imgsz 1600: letterbox -> network -> decode -> NMS -> retina masks
  segment  SAM-2.1 Hiera-L: antialiased resize -> image encoder -> 8 box prompts -> mask decoder -> masks
  inpaint  R=1 outside-text region: crop geometry + EDT feather (host) -> FLUX.1-Kontext, 20 Euler steps bf16
           at the snapped ~1 MP resolution (VAE encode, 57-block MMDiT x steps, VAE decode) -> LANCZOS -> composite
  upscale  2x RCAN (10 groups x 20 RCAB x 64 feats) on the whole page
`config.stages` names the stages that ran inside the timed region.  Pages are resident in HBM before the
timed region (image decode/encode excluded).  Pages are independent units: rank r processes
its own pages, no data-path collective; the only collective is the start-up weight broadcast over RCCL
(outside the timed region).  Weights are seeded random (no checkpoints offline) with the real architectures.

Launch:  python bench.py --gpus 1 --steps K --warmup W [--dump-outputs DIR] [--full]
         python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...
"""
import argparse
import json
import os
import sys
import time
from pathlib import Path



def _early_hw_queues(argv):
    """ROCm maps HIP streams onto GPU_MAX_HW_QUEUES hardware queues per device (default 4); streams that share a queue run their work one
    after the other.  A page's detect stage keeps five model streams busy at once (hip/plan.py AsyncLane: four detectors + the SAM encoder),
    so with four queues two of its graphs always wait for each other: measured on an MI355X (profiles/r03_hw_queues_ab.log), BASELINE
    config 2 29.1 -> 31.4 pages/s and config 1 46.5 -> 49.2 with eight queues; with the detect stages of TWO pages in flight on two sets of
    model instances (round 4, profiles/r04_visit_e_front_replicas.log) eight queues LOSE (config 2: 28.1) and sixteen win (33.2; config 1:
    51.3 -> 56.7).  More queues LOSE where the back half of the page
    pipeline saturates the chip with big kernels (config 5, two pages in flight: 1.20 -> 1.10 pages/s on boxes of the same clock class —
    detector kernels that truly run beside the 256-workgroup GEMM / conv waves cost those waves a second round), so it is chosen here only
    for the stage sets without diffusion / upscaling, and reported in the line (config.hw_queues).  It has to be in the environment
    before the HIP runtime starts, hence this look at argv ahead of `import torch`; a value the caller exported wins."""
    def opt(name, default):
        for i, a in enumerate(argv):
            if a == name and i + 1 < len(argv):
                return argv[i + 1]
            if a.startswith(name + "="):
                return a.split("=", 1)[1]
        return default
    stages = opt("--stages", None)
    if stages in (None, "all"):
        stages = {"1": "detect,clean", "2": "detect,segment"}.get(opt("--config", "4"), "detect,segment,inpaint,upscale")
    if not ({"inpaint", "upscale"} & {x.strip() for x in stages.split(",")}):
        os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")      # round 4: two pages' detect stages in flight (--front-replicas 2) = ten model streams


_early_hw_queues(sys.argv[1:])

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
MFMA_PEAK_TFLOPS = 2500.0    # dense bf16/f16 (no sparsity)
FP8_PEAK_TFLOPS = 5000.0     # dense fp8 on the MX-scaled K = 64 / 128 matrix instructions (no sparsity)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--width", type=int, default=None)
    ap.add_argument("--height", type=int, default=None)
    ap.add_argument("--stages", default=None, help="comma list of: detect,segment,inpaint,upscale,clean (default: what --config names)")
    ap.add_argument("--config", type=int, default=4, choices=[1, 2, 3, 4, 5],
                    help="BASELINE.json configs (1-based): 1 = YOLO detect + OpenCV-style clean, 2 = YOLO + SAM-2.1 segment only, 3 = + FLUX.1-Kontext "
                         "inpaint (20 steps bf16), 4 = full pipeline + 2x upscale (the headline metric, default), 5 = 2048x3072 pages, FLUX.2-Klein fp8 "
                         "inpaint + upscale")
    ap.add_argument("--inpainter", default=None, choices=["kontext", "klein_4b", "klein_9b"], help="default: kontext (configs 3, 4), klein_4b (config 5)")
    ap.add_argument("--bubble-detector", default="yolo_2", choices=["yolo_1", "yolo_2"],
                    help="primary bubble detector of the detect stage: yolo_2 = the reference's default (core/config.py:18; a YOLO11-seg, run here at "
                         "the m scale) or yolo_1 = YOLOv8m-seg")
    ap.add_argument("--no-aux-detectors", action="store_true",
                    help="leave out the panel (YOLO11-L @640) and outside-text (YOLO12x @640) detectors that the reference runs on every page by "
                         "default (core/config.py:20-21); RT-DETR-v2 always runs")
    ap.add_argument("--serial-detectors", action="store_true",
                    help="call the page's detectors one after the other, each returning finished results (the reference's order of calls); default: "
                         "submit all of them, then collect — their graphs run side by side on their own streams")
    ap.add_argument("--no-lanes", action="store_true", help="FLUX.1: keep the text stream's ops in line with the image stream's (one lane)")
    ap.add_argument("--no-fused-quant", action="store_true",
                    help="Klein fp8: separate quantiser passes behind the norms and SwiGLU (round 2's form) instead of producers that write the fp8 operands themselves")
    ap.add_argument("--no-fp8", action="store_true", help="Klein: keep the block linears in bf16 instead of the MX-fp8 matrix path")
    ap.add_argument("--no-overlap", action="store_true",
                    help="run the stages of a page strictly one after another; default: two pages in flight — detect / segment / OSB prepare of "
                         "page i+1 on a worker thread while the main thread runs inpaint / upscale / clean of page i (same work per page)")
    ap.add_argument("--launch-check", action="store_true",
                    help="bring the process group up, report the ranks the collective library sees and one broadcast, then exit (no GPU work; "
                         "with --backend gloo this runs on a CPU-only host)")
    ap.add_argument("--boxes", type=int, default=8, help="bubbles per page (SAM prompts; generator ground truth, SURVEY.md §8d)")
    ap.add_argument("--regions", type=int, default=1, help="FLUX-inpainted outside-text regions per page (R in SURVEY.md §8d)")
    ap.add_argument("--inpaint-steps", type=int, default=None, help="default: 20 (Kontext, BASELINE config 3), 8 (Klein: the reference's flux_num_inference_steps default)")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend for N > 1 (nccl = RCCL; gloo only for dry runs)")
    ap.add_argument("--upscale-model", default="model", choices=["model", "model_lite"])
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--with-traffic", action="store_true", help=argparse.SUPPRESS)       # (round 3's opt-in; the counter child now runs by default)
    ap.add_argument("--sam-precision", choices=("fast", "high"), default=None,
                    help="SAM-2.1 arithmetic: high = hi + lo trunk weights, fp32 residual stream and an fp32 mask decoder (core/ml/sam2.py); fast = 16-bit "
                         "storage throughout.  Default: the product's rule (core/pipeline.py resolve_sam_precision) — high for every stage set since round 6")
    ap.add_argument("--no-traffic", action="store_true",
                    help="skip the counter child that fills roofline.traffic: after the timed region rank 0 (at --gpus 1) re-executes this command's inpaint "
                         "(or upscale) stage under `rocprofv3 --pmc FETCH_SIZE` and `--pmc WRITE_SIZE` (two passes, --kernel-trace only) on a DiT cut to "
                         "2 + 4 blocks (same kernels, shapes and launch mix: bytes per launch do not depend on depth) with one denoising step, ~60 s")
    ap.add_argument("--traffic-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--batch-io", type=int, default=0,
                    help="after the timed region: N pages through `batch_process_images` WITH image I/O — PNG files decoded from disk, uploaded, "
                         "run through the same stages, results downloaded, PNG-encoded and written (SURVEY.md §8d: decode / encode reported "
                         "separately, never part of `value`); reported under config.batch_io")
    ap.add_argument("--io-threads", type=int, default=None, help="decoder / encoder threads of the batch harness per rank (default: host cores / ranks / 4, 2..8)")
    ap.add_argument("--no-glu-epilogue", action="store_true",
                    help="FLUX.2-Klein fp8 path, for A/Bs: separate SwiGLU / attention-output quantiser launches instead of the epilogue fusions "
                         "(mtx_gemm_args.glu_*, mtx_attn_args.q8) that are the default since round 4")
    ap.add_argument("--no-attn-pv-f8", action="store_true",
                    help="FLUX.2-Klein fp8 path, for A/Bs: 16-bit P V in the joint attention instead of the fp8 path's default since round 6 (values as e4m3 V^T, "
                         "probabilities rounded to e4m3: Flux2DiTHip(attn_pv_f8=True), mtx_attn_args.v_f8t); reported in config.attn_pv_f8")
    ap.add_argument("--no-attn-qk-f8", action="store_true",
                    help="FLUX.2-Klein fp8 path, for A/Bs: 16-bit attention scores instead of the scores from e4m3 q and k on the fp8 matrix instruction "
                         "(Flux2DiTHip(attn_qk_f8=True), mtx_attn_args.q_f8 / k_f8) that are the fp8 path's default since round 6; reported in config.attn_qk_f8")
    ap.add_argument("--detector-batch", type=int, default=0,
                    help="pages per graph replay of the panel / outside-text detectors (imgsz 640): > 1 shares ONE batching wrapper per detector between the "
                         "front halves that run side by side; 1 = a detector instance per front half; 0 (default) = as many as there are front halves")
    ap.add_argument("--no-rtdetr-batch", action="store_true", help="for A/Bs: keep an RT-DETR instance per front half while the 640-px YOLO detectors share batches")
    ap.add_argument("--front-replicas", type=int, default=None,
                    help="instances of the detect-stage models (detectors + SAM) per rank; with N > 1 the front halves of N pages run at once, "
                         "each on its own instance (a model's plan has one set of buffers).  Default: 2 for the stage sets without diffusion / "
                         "upscaling (BASELINE configs 1 and 2: the 640-pixel graphs of ONE page do not fill 256 CUs), else 1")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--kontext-backend", default="sdnq", choices=["sdnq", "nunchaku", "sdcpp"],
                    help="the reference's Kontext backend name the OSB stage is configured with: sdnq (default; every step runs every block — the headline) "
                         "or nunchaku, whose loader wraps the pipeline in the first-block cache (reference model_manager.py:1159-1162) with --residual-diff-threshold")
    ap.add_argument("--residual-diff-threshold", type=float, default=0.15, help="first-block cache threshold (reference core/config.py:150), used with --kontext-backend nunchaku")
    ap.add_argument("--no-extra", action="store_true",
                    help="--full on the default command only (config 4, one GPU): skip the child runs that put BASELINE configs 5 and 2 and the first-block-cache figure "
                         "under `extra` of the same JSON line (after the timed region; ~2 minutes)")
    ap.add_argument("--extra-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--time-ops", default="auto", choices=["auto", "difference", "stamp"],
                    help="in-context kernel timing of the roofline objects: hipGraph with minus hipGraph without the ops (HIP events), "
                         "or device wall-clock stamps around the ops inside one graph (mtx_plan_time_ops, MTX_TIME_OPS=stamp); auto = "
                         "both, stamps reported when they pass a sanity band around the difference figure")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also take everything that is not the headline figure: the stage-by-stage wall clock of one more page, "
                         "per-stage GPU times, rooflines, the counter child (unless --no-traffic), the other BASELINE configs under `extra` (unless "
                         "--no-extra) and the CPU baseline (unless --no-cpu-baseline).  Default: set up, warm up, time --steps pages, print the line")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write what the timed path returned for its last step as DIR/<name>.npy (float32; arrays above a fixed size as a fixed, "
                         "seeded sample of their elements; 64 MB at most in all)")
    a = ap.parse_args()
    preset = {1: "detect,clean", 2: "detect,segment", 3: "detect,segment,inpaint", 4: "detect,segment,inpaint,upscale", 5: "detect,segment,inpaint,upscale"}
    if a.stages is None or a.stages == "all":
        a.stages = preset[a.config]
    if a.width is None:
        a.width = 2048 if a.config == 5 else 1024
    if a.height is None:
        a.height = 3072 if a.config == 5 else 1536
    if a.inpainter is None:
        a.inpainter = "klein_4b" if a.config == 5 else "kontext"
    if a.inpaint_steps is None:
        a.inpaint_steps = 20 if a.inpainter == "kontext" else 8
    a.sam_precision_rule = a.sam_precision is None
    if a.sam_precision is None:
        a.sam_precision = "high"                      # the product's rule since round 6: every batch, segment-only ones included
    return a


def self_launch(args) -> int:
    """`python bench.py --gpus N` with N > 1 and no launcher around it: re-run this very command under torch.distributed.run, one rank per
    GPU (nccl = RCCL), rendezvous on 127.0.0.1 — so `--gpus 8` can never silently measure one GPU eight times."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, MTX_BENCH_SELF_LAUNCHED="1")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), str(Path(__file__).resolve())] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def launch_check(args, rank, world):
    """process-group smoke test: world size as the collective library reports it, every rank's id gathered, one 64 MB broadcast timed"""
    import torch.distributed as dist
    use_gpu = args.backend == "nccl"
    if use_gpu:
        local = 0 if os.environ.get("MTX_BENCH_ONE_DEVICE") == "1" else int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(local)
        dist.init_process_group("nccl", device_id=torch.device(f"cuda:{local}"))
    else:
        dist.init_process_group(args.backend)
    dev = torch.device("cuda", torch.cuda.current_device()) if use_gpu else torch.device("cpu")
    ids = [None] * dist.get_world_size()
    dist.all_gather_object(ids, dist.get_rank())
    buf = torch.full((16 << 20,), float(rank == 0), device=dev)
    dist.barrier()
    t0 = time.perf_counter()
    dist.broadcast(buf, src=0)
    if use_gpu:
        torch.cuda.synchronize()
    dist.barrier()
    dt = time.perf_counter() - t0
    ok = bool(buf.min().item() == 1.0)
    if rank == 0:
        print(json.dumps({"launch_check": True, "n_gpus": args.gpus, "world_size": dist.get_world_size(), "ranks": sorted(ids), "backend": dist.get_backend(),
                          "self_launched": os.environ.get("MTX_BENCH_SELF_LAUNCHED") == "1", "broadcast_64MB_ms": 1e3 * dt, "broadcast_ok": ok}))
    dist.destroy_process_group()


def broadcast_state_dict(sd, rank, world, device):
    """Rank 0 owns the checkpoint; one flat RCCL broadcast over xGMI hands it to every rank."""
    import torch.distributed as dist
    keys = sorted(sd.keys())
    shapes = [tuple(sd[k].shape) for k in keys]
    sizes = [int(np.prod(s)) if len(s) else 1 for s in shapes]
    cdev = device if dist.get_backend() == "nccl" else torch.device("cpu")       # gloo (dry runs of the N > 1 path) moves host tensors
    flat = torch.empty(sum(sizes), dtype=torch.float32, device=cdev)
    if rank == 0:
        flat.copy_(torch.cat([sd[k].float().reshape(-1) for k in keys]).to(cdev))
    dist.broadcast(flat, src=0)
    out, off = {}, 0
    flat = flat.cpu()
    for k, s, n in zip(keys, shapes, sizes):
        out[k] = flat[off:off + n].view(s).clone()
        off += n
    return out


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(self_launch(args))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if args.launch_check:
        if world > 1:
            launch_check(args, rank, world)
        else:
            print(json.dumps({"launch_check": True, "n_gpus": 1, "world_size": 1, "ranks": [0], "self_launched": False}))
        return
    assert torch.cuda.is_available(), "bench.py needs a GPU (the HIP path has no CPU fallback)"
    if os.environ.get("MTX_BENCH_ONE_DEVICE") == "1":     # dry run of the N > 1 code path on a one-GPU box (with --backend gloo)
        local_rank = 0
        os.environ["LOCAL_RANK"] = "0"                     # ... for everything that derives its device from it (ModelManager: core/device.py)
    torch.cuda.set_device(local_rank)
    device = torch.device(f"cuda:{local_rank}")
    # host hygiene for N ranks on one node: every rank runs a stage-A worker thread plus numpy / PIL / torch-CPU work (NMS, EDT feather,
    # LANCZOS, contour code); with the default thread counts 8 ranks would each claim every core.  One share of the cores per rank.
    # Counted on the cores this process may actually run on (a container's affinity mask, not the machine's core count: setting the
    # latter on a 32-core slice of a 256-core host made every small torch op 40 ms — measured, r03 visit E), and capped: the host ops
    # here are small, more than 16 threads each only adds fork / join time.
    # With several ranks each one first moves to the CPUs of its GPU's NUMA node (its share of them when GPUs share a node):
    # core/device.py pin_host_threads_to_gpu — worker threads and codec pools started later inherit the mask.
    placement = {"pinned": False, "reason": "one rank"}
    if world > 1 and os.environ.get("MTX_BENCH_ONE_DEVICE") != "1":
        from mangatranslator_amd.core.device import pin_host_threads_to_gpu
        placement = pin_host_threads_to_gpu(local_rank, n_devices=torch.cuda.device_count())
    try:
        usable = len(os.sched_getaffinity(0))
    except AttributeError:
        usable = os.cpu_count() or 8
    host_threads = max(1, min(16, usable if placement.get("pinned") else usable // world, torch.get_num_threads()))
    torch.set_num_threads(host_threads)
    dist = None
    if world > 1:
        import torch.distributed as dist
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=device)
        else:
            dist.init_process_group(args.backend)

    from PIL import Image
    from mangatranslator_amd.hip.lib import get_library
    from mangatranslator_amd.utils.synthetic_pages import make_page

    lib = get_library()
    lib.init(local_rank)
    graph = not args.no_graph
    want = [x.strip() for x in args.stages.split(",")]
    stages = [st for st in ("detect", "segment", "inpaint", "upscale", "clean") if st in want]
    # front halves in flight (page i uses model set i % N): decided here because the batching wrapper of the 640-px detectors is sized by it
    n_front = args.front_replicas
    if n_front is None:
        # (measured with the front halves sharing detector batches, profiles/r06_visit_r_...log: config 2 — SAM in the front half — 34.8 pages/s with 2 front
        # halves and no batches (round 5's arrangement), 35.7 with 2 + batches of 2, 41.3-42.4 with 3 + 3, 40.1-40.3 with 4 + 4; config 1: 68.6 -> 77.6-78.4 with 4 + 4)
        light_back = "detect" in stages and "inpaint" not in stages and "upscale" not in stages and not args.no_overlap and not args.serial_detectors
        # (with RT-DETR behind the batching wrapper as well — profiles/r06_visit_u_...log, three alternating rounds — config 2: 38.7-41.8 with 3 front halves,
        # 47.6-48.2 with 4, 43.3-43.8 with 5; config 1: 67 / 80 / 85 with 2 / 3 / 4)
        n_front = 4 if light_back else 1
    n_front = max(1, n_front)
    if args.detector_batch <= 0:
        args.detector_batch = n_front
    t_load0 = time.perf_counter()
    first = rank == 0 or world == 1

    # ---- models: rank 0 "reads" (seeds) the checkpoints, every other rank receives them over RCCL ---------
    upscaler, rcan_sd, rcan_cfg = None, None, None
    if "upscale" in want:
        from mangatranslator_amd.core.ml.rcan import RCANUpscaler
        from mangatranslator_amd.utils.synthetic_checkpoints import rcan_state_dict as make_state_dict   # seeded stand-in checkpoint (no real weights offline)
        if args.upscale_model == "model_lite":   # assumed Fast_RCAN_PU shape; real hyper-parameters come from the file
            rcan_cfg = dict(n_feats=64, n_resgroups=4, n_resblocks=8, unshuffle=2)
        else:                                    # canonical RCAN: 10 groups x 20 RCAB x 64 feats
            rcan_cfg = dict(n_feats=64, n_resgroups=10, n_resblocks=20, unshuffle=1)
        rcan_sd = make_state_dict(seed=7 if first else 0, **rcan_cfg)
        if world > 1:
            rcan_sd = broadcast_state_dict(rcan_sd, rank, world, device)
        upscaler = RCANUpscaler(rcan_sd, device=device, lib=lib, graph=graph)
    yolo = rtdetr = None
    aux_detectors, make_aux = [], []
    make_yolo = make_rtdetr = make_sam = None
    if "detect" in want:
        from mangatranslator_amd.core.ml.yolo import YoloSegHip
        from mangatranslator_amd.utils import synthetic_checkpoints as synth
        # seeded YOLOv8m-seg (the reference's yolo_1 geometry) from its parameter inventory; the random head is tamed so NMS sees a
        # realistic number of candidates
        v8_shapes, v8_head = synth.yolov8_seg_shapes("m", 1)
        ysd = synth.seeded_detector(v8_shapes, v8_head, seed=3 if first else 0, class_bias=-1.0, class_gain=0.05, box_gain=0.1)
        if world > 1:
            ysd = broadcast_state_dict(ysd, rank, world, device)
        make_yolo = lambda: YoloSegHip(ysd, device=device, lib=lib, graph=graph)
        yolo = make_yolo()
        if args.bubble_detector == "yolo_2" or not args.no_aux_detectors:
            from mangatranslator_amd.core.ml.yolo11 import Yolo11Hip

            def seeded_y11(family, scale, seg, seed):
                """seeded network of the published architecture (parameter inventory), head tamed like the YOLOv8 one above: scores ~ 0.12,
                below every threshold used here"""
                shapes_, head_ = synth.yolo11_shapes(family, scale, 1, seg)
                sd_ = synth.seeded_detector(shapes_, head_, seed=seed if first else 0, class_bias=-2.0, class_gain=0.05, box_gain=0.1)
                if world > 1:
                    sd_ = broadcast_state_dict(sd_, rank, world, device)
                return lambda: Yolo11Hip(sd_, device=device, lib=lib, graph=graph)
            if args.bubble_detector == "yolo_2":
                make_yolo = seeded_y11("11", "m", True, 13)     # manga109-segmentation-bubble: a YOLO11-seg (its scale is not stated upstream: m assumed)
                yolo = make_yolo()
            if not args.no_aux_detectors:
                make_aux = [("panel", seeded_y11("11", "l", False, 17), 0.25), ("osb_text", seeded_y11("12", "x", False, 19), 0.4)]
                aux_detectors = [(n_, mk_(), c_) for n_, mk_, c_ in make_aux]
                if args.detector_batch > 1 and not args.serial_detectors:
                    # one batching wrapper per 640-px detector, SHARED by every front half (core/ml/detector_batch.py): the pages whose front
                    # halves run side by side go through one graph replay; their results are the one-page call's, byte for byte
                    from mangatranslator_amd.core.ml.detector_batch import DetectorBatcher
                    aux_detectors = [(n_, DetectorBatcher(d_, args.detector_batch), c_) for n_, d_, c_ in aux_detectors]
                    make_aux = [(n_, (lambda w_=d_: w_), c_) for n_, d_, c_ in aux_detectors]
        # secondary detector of the same stage: RT-DETR-v2 R50 @640 (reference detection.py:1401-1407, on by default)
        from mangatranslator_amd.core.ml.rtdetr import RTDetrHip
        rcfg = synth.rtdetr_r50_config()
        rsd = synth.rtdetr_state_dict(rcfg, seed=5 if first else 0)
        if world > 1:
            rsd = broadcast_state_dict(rsd, rank, world, device)
        make_rtdetr = lambda: RTDetrHip(rsd, rcfg, device=device, lib=lib, graph=graph, names={0: "bubble", 1: "text_bubble", 2: "text_free"})
        rtdetr = make_rtdetr()
        if args.detector_batch > 1 and not args.serial_detectors and not args.no_rtdetr_batch:
            # the secondary detector too: ONE instance behind a batching wrapper shared by the front halves (backbone + encoder once per batch, the
            # decoder image by image: core/ml/detector_batch.py RTDetrBatcher)
            from mangatranslator_amd.core.ml.detector_batch import RTDetrBatcher
            rtdetr = RTDetrBatcher(rtdetr, args.detector_batch)
            make_rtdetr = (lambda w_=rtdetr: w_)
    sam = None
    if "segment" in want:
        from mangatranslator_amd.core.ml.sam2 import Sam2Hip
        from mangatranslator_amd.hip.abi import F16 as abi_f16
        from mangatranslator_amd.utils import synthetic_checkpoints as synth_sam
        sam_cfg = synth_sam.sam2_hiera_large_config()           # facebook/sam2.1-hiera-large geometry, seeded weights
        if first:
            sam_sd = synth_sam.sam2_state_dict(sam_cfg, seed=11)
        else:
            sam_sd = {k: torch.empty(shp) for k, shp in synth_sam.sam2_shapes(sam_cfg).items()}
        if world > 1:
            sam_sd = broadcast_state_dict(sam_sd, rank, world, device)
        # f16 storage: what ModelManager.load_sam2 serves (bf16 only when a checkpoint leaves the f16 range)
        make_sam = lambda: Sam2Hip(sam_sd, sam_cfg, device=device, lib=lib, graph=graph, dtype=abi_f16, precision=args.sam_precision)
        sam = make_sam()
    inpainter, flux = None, None
    klein = args.inpainter.startswith("klein")
    if "inpaint" in want:
        from mangatranslator_amd.core.ml.model_manager import ModelType, get_model_manager
        if klein:
            # FLUX.2-Klein (the reference's default inpainter; BASELINE config 5): 3.9 B / 9.1 B-parameter Flux2 MMDiT + 84 M-parameter VAE, seeded
            # on rank 0's GPU and broadcast tensor by tensor; block linears quantised to MX fp8 at load unless --no-fp8
            from mangatranslator_amd.core.image.inpainting import FluxKleinInpainter
            from mangatranslator_amd.core.ml import flux as fx
            from mangatranslator_amd.core.ml import flux2 as f2
            dcfg = f2.KLEIN_9B_DIT_CFG if args.inpainter == "klein_9b" else f2.KLEIN_4B_DIT_CFG
            if args.traffic_child:      # counter pass: same kernels, shapes and double : single launch mix on a fraction of the depth
                dcfg = dict(dcfg, layers=max(1, dcfg["layers"] // 5), single_layers=max(1, dcfg["single_layers"] // 5))
            dit = f2.Flux2DiTHip(fx.synthetic_provider(f2.dit_param_shapes(dcfg), device, 21, broadcast=world > 1), dcfg, device, lib=lib,
                                  fp8=not args.no_fp8, fused_quant=not args.no_fused_quant, glu_epilogue=not args.no_glu_epilogue, attn_q8=not args.no_glu_epilogue,
                                  attn_qk_f8=not args.no_attn_qk_f8, attn_pv_f8=not args.no_attn_pv_f8)
            vae = f2.Flux2VAEHip(fx.synthetic_provider(f2.vae_param_shapes(f2.KLEIN_VAE_CFG), device, 22, broadcast=world > 1), f2.KLEIN_VAE_CFG, device, lib=lib)
            flux = f2.Flux2KleinHip(dit, vae, graph=graph)
            flux.set_prompt_embeds(torch.randn(512, dcfg["joint_dim"], generator=torch.Generator().manual_seed(23)))     # cached Qwen3 states (stand-ins)
            mt = ModelType.FLUX_KLEIN_9B_PIPELINE if args.inpainter == "klein_9b" else ModelType.FLUX_KLEIN_4B_PIPELINE
            method = "flux_" + args.inpainter
        else:
            from mangatranslator_amd.core.image.inpainting import FluxKontextInpainter
            from mangatranslator_amd.core.ml import flux as fx
            # 11.9 B-parameter MMDiT + 84 M-parameter VAE, bf16, seeded on rank 0's GPU and broadcast tensor by tensor
            kcfg = fx.KONTEXT_DIT_CFG
            if args.traffic_child:      # counter pass: 2 + 4 of the 19 + 38 blocks (the same 1 : 2 launch mix; bytes per launch do not depend on depth)
                kcfg = dict(kcfg, layers=2, single_layers=4)
            dit = fx.FluxDiTHip(fx.synthetic_provider(fx.dit_param_shapes(kcfg), device, 21, broadcast=world > 1), kcfg, device, lib=lib,
                                text_stream_on_side_lane=not args.no_lanes)
            vae = fx.FluxVAEHip(fx.synthetic_provider(fx.vae_param_shapes(fx.KONTEXT_VAE_CFG), device, 22, broadcast=world > 1), fx.KONTEXT_VAE_CFG, device, lib=lib)
            flux = fx.FluxKontextHip(dit, vae, graph=graph)
            g = torch.Generator().manual_seed(23)     # cached T5 / CLIP embeddings of "Remove all text." (random stand-ins)
            flux.set_prompt_embeds(torch.randn(512, 4096, generator=g), torch.randn(768, generator=g))
            mt, method = ModelType.FLUX_KONTEXT_SDNQ_PIPELINE, "flux_kontext"
        inpainter = True
        # the OSB stage (core/outside_text_processor.py) builds its own inpainter and asks the manager for the pipeline
        from mangatranslator_amd.core.batch_coordinator import BatchRequestCoordinator
        from mangatranslator_amd.core import outside_text_processor as otp
        import types as _types
        get_model_manager().models[mt] = flux
        osb_cfg = _types.SimpleNamespace(
            device=device, yolo_model_path=None, request_coordinator=BatchRequestCoordinator(1),
            detection=_types.SimpleNamespace(conjoined_confidence=0.35, bubble_detector_model="yolo_2"),
            outside_text=_types.SimpleNamespace(      # the reference's OutsideTextConfig defaults (core/config.py:126-173), Kontext selected
                enabled=True, enable_page_number_filtering=False, min_area_ignore_ratio=0.0, seed=1, huggingface_token="",
                inpainting_method=method, flux_backend=args.kontext_backend, flux_low_vram=False, flux_num_inference_steps=args.inpaint_steps,
                flux_luminance_correction=True, flux_upscale_small_crops=True, flux_sdcpp_cache_mode="none", flux_sdcpp_diffusion_quant="",
                flux_sdcpp_text_encoder_quant="",
                flux_group_regions=False, flux_residual_diff_threshold=args.residual_diff_threshold, osb_confidence=0.5, osb_text_free_only=False,
                bbox_expansion_percent_width=0.1, bbox_expansion_percent_height=0.1, osb_render_expansion_narrow_multiplier=1.0,
                osb_render_expansion_tiny_multiplier=1.0, osb_render_expansion_aspect_ratio_threshold=0.4,
                osb_render_expansion_area_ratio_threshold=0.005, text_box_proximity_ratio=0.02))

    load_s = time.perf_counter() - t_load0          # model set-up incl. the start-up weight broadcast (outside the timed region)

    # ---- synthetic pages, resident in HBM -----------------------------------------------------------------
    W_, H_ = args.width, args.height
    pool = 2
    pages, page_boxes, page_pil, page_masks, page_text_boxes = [], [], [], [], []
    for i in range(pool):
        pg, boxes, regions = make_page(rank * 1000 + i, W_, H_, bubbles=args.boxes, osb_regions=args.regions)
        pages.append(torch.from_numpy(pg).to(device))
        page_boxes.append(boxes)
        page_pil.append(Image.fromarray(pg))
        ms_ = []
        for (x0, y0, x1, y1) in regions:
            m_ = np.zeros((H_, W_), bool); m_[y0:y1, x0:x1] = True
            ms_.append(m_)
        page_masks.append(ms_)
        # the outside-text detections of the page: the text inside each gradient block (block inset by 10 px, so the 2 px ring the
        # solid-border test samples lies on the gradient and the region goes to FLUX)
        page_text_boxes.append([[x0 + 10.0, y0 + 10.0, x1 - 10.0, y1 - 10.0] for (x0, y0, x1, y1) in regions])
    torch.cuda.synchronize()

    page_outs = {}           # page index -> that page's stage results: two front halves may be in flight, nothing is shared between pages
    page_bgr = [pg.flip(-1).contiguous().cpu().numpy() for pg in pages]   # the detector's input is BGR (cv2 layout)
    yolo_conf = 0.6
    if yolo is not None:     # untimed calibration: seeded weights have arbitrary scores; let ~3x boxes anchors pass
        yolo(page_bgr[0], conf=0.0, imgsz=1600, max_det=1)
        plan0, _ = yolo._plans[(H_, W_, 1600)]
        sc = plan0.decoded[:, 4].float().sort(descending=True).values
        yolo_conf = float(sc[min(3 * args.boxes, len(sc) - 1)])

    clean_args = None
    if "clean" in want:      # bubble cleaning (reference core/image/cleaning.py:210-521) on the page's ground-truth bubble masks
        from mangatranslator_amd.core.image import cleaning as cl
        yy, xx = np.mgrid[0:H_, 0:W_]
        sc_ = (W_ * H_ / 1e6) ** 0.5
        ckw = dict(dilation_kernel=cl.structuring_element(cl.scale_kernel(cl.DILATION_KERNEL_SIZE, sc_)),
                   constraint_erosion_kernel=cl.structuring_element(cl.scale_kernel(cl.EROSION_KERNEL_SIZE, sc_)),
                   min_contour_area=cl.scale_area(50, sc_, minimum=50, maximum=5000), processing_scale=sc_, device=device, lib=lib)
        shrink_ = float(cl.scale_scalar(5, sc_, minimum=0.0, maximum=64.0))
        clean_args = []
        for k_ in range(pool):
            bm = []
            for x0, y0, x1, y1 in page_boxes[k_]:
                cx, cy, a_, b_ = (x0 + x1) / 2, (y0 + y1) / 2, (x1 - x0) / 2 - 4, (y1 - y0) / 2 - 4
                bm.append((((xx - cx) / a_) ** 2 + ((yy - cy) / b_) ** 2 <= 1.0).astype(np.uint8) * 255)
            clean_args.append((torch.from_numpy(np.stack(bm)).to(device), [tuple(int(v) for v in b_) for b_ in page_boxes[k_]]))

    # ---- instances of the front half's models: page i uses set i % N, so N pages' detect stages can be in flight at once --------------
    front_sets = [dict(yolo=yolo, aux=aux_detectors, rtdetr=rtdetr, sam=sam)]
    for _ in range(1, n_front):
        front_sets.append(dict(yolo=make_yolo() if make_yolo else None, aux=[(n_, mk_(), c_) for n_, mk_, c_ in make_aux],
                               rtdetr=make_rtdetr() if make_rtdetr else None, sam=make_sam() if make_sam else None))

    stage_wall = {}

    def lap(name, t_prev):      # only when a stage-by-stage wall-clock breakdown is being taken (one extra page after the timed region)
        if stage_wall is not None and stage_wall.get("_on"):
            torch.cuda.synchronize()
            now = time.perf_counter()
            stage_wall[name] = stage_wall.get(name, 0.0) + 1e3 * (now - t_prev)
            return now
        return t_prev

    from mangatranslator_amd.core.caching import get_cache
    stage_memo = get_cache()

    # BASELINE config 2 (detect + segment, nothing behind them): the two stages are the two halves of the page pipeline — the SAM mask decoder of
    # page i (its encoder already ran beside the detectors) beside the detectors of page i + 1
    seg_in_b = (yolo is not None and sam is not None and inpainter is None and upscaler is None and clean_args is None
                and not args.no_overlap and not args.serial_detectors)

    import threading as _threading
    harness_slot = _threading.local()       # set by the batch harness (front_context): the instance set this thread's front half holds

    def front_set_of(i):
        slot = getattr(harness_slot, "slot", None)
        return slot if slot is not None else i % n_front

    def stage_a(i):
        """front half of page i: the stages whose host share is large (NMS, prompt handling, OSB region logic)"""
        if world > 1:       # may run on a worker thread: an operator that asks the manager for an unstaged optional model must not enter a collective from here
            from mangatranslator_amd.core.ml.model_manager import get_model_manager as _gmm
            with _gmm().thread_local_reads():
                return stage_a_body(i)
        return stage_a_body(i)

    def stage_a_body(i):
        k = i % pool
        outs = page_outs.setdefault(i, {})
        fs = front_sets[front_set_of(i)]
        yolo, aux_detectors, rtdetr, sam = fs["yolo"], fs["aux"], fs["rtdetr"], fs["sam"]
        stage_memo.reset()        # the operators remember results per (pixels, settings); the pool repeats pages, and no step may be served from memory
        tl = time.perf_counter()
        work_ = None
        sam_ticket = None
        if yolo is not None and args.serial_detectors:
            outs["detect"] = yolo(page_bgr[k], conf=yolo_conf, imgsz=1600)[0]
            outs["detect2"] = rtdetr(page_bgr[k], conf=0.35, imgsz=640)[0]
            for name_, det_, conf_ in aux_detectors:             # panel / outside-text detectors: imgsz 640 (reference detection.py:1867-1873, 144-150)
                outs["detect_" + name_] = det_(page_bgr[k], conf=conf_, imgsz=640)[0]
            tl = lap("detect", tl)
        elif yolo is not None:
            # every detector of the page is SUBMITTED first — each queues its upload and graph replay on its own HIP stream — and
            # collected afterwards: the four graphs share the chip (none of the 640-pixel networks fills 256 CUs alone) and one
            # detector's NMS / result objects run on the host while the others' kernels still execute (hip/plan.py AsyncLane)
            # The YOLO family reads the page where it already lies in HBM (one upload per page, not one per detector); RT-DETR — whose
            # pre-processing is the image processor's host-side resize — is submitted last, so that resize runs beside the others' kernels.
            bgr_dev = pages[k].flip(-1)
            tickets = [("detect", yolo, yolo.submit(bgr_dev, conf=yolo_conf, imgsz=1600))]
            tickets += [("detect_" + name_, det_, det_.submit(bgr_dev, conf=conf_, imgsz=640)) for name_, det_, conf_ in aux_detectors]
            tickets.append(("detect2", rtdetr, rtdetr.submit(page_bgr[k], conf=0.35, imgsz=640)))
            if sam is not None:          # the image encoder does not depend on the boxes: it runs beside the detectors, the mask decoder follows the boxes
                sam_ticket = sam.submit_image(pages[k])
            for name_, det_, tk_ in tickets:
                outs[name_] = det_.collect(tk_)[0]
            tl = lap("detect", tl)
        if sam is not None and seg_in_b:          # detect + segment only: the mask decoder of this page runs beside the next page's detectors
            return ("segment", sam_ticket)
        if sam is not None:      # prompts: the generator's ground-truth boxes (fixed unit count)
            outs["segment"] = sam.segment(pages[k], page_boxes[k], ticket=sam_ticket)
            tl = lap("segment", tl)
        if inpainter is not None:
            # the reference's OSB stage end to end (prepare + finish): the bubbles guard the fills, the text boxes arrive as text_free
            # detections, each region is classified by its border ring and the non-solid ones run through FLUX in waves.  Bubbles
            # and text boxes are the generator's ground truth, like the SAM prompts (seeded-random SAM weights give arbitrary
            # masks that may swallow the text block, so the masks of the segment stage are not fed forward here)
            bubbles_ = [{"bbox": tuple(float(v) for v in b)} for b in page_boxes[k]]
            work_ = otp.prepare_outside_text_work(page_pil[k], osb_cfg, "page.png", "PNG", bubble_data=bubbles_,      # == process_outside_text
                                                  text_free_boxes=page_text_boxes[k])
            tl = lap("inpaint_prepare", tl)
        return work_

    def stage_b(i, work_):
        """back half of page i: GPU-bound; returns the page's stage results"""
        k = i % pool
        outs = page_outs.pop(i, None) or {}
        tl = time.perf_counter()
        if seg_in_b:
            outs["segment"] = front_sets[front_set_of(i)]["sam"].segment(pages[k], page_boxes[k], ticket=work_[1])
            tl = lap("segment", tl)
            return outs
        if inpainter is not None:
            outs["inpaint"], _ = otp.finish_outside_text_work(work_) if work_ is not None else (page_pil[k], [])
            tl = lap("inpaint_finish", tl)
        if upscaler is not None:
            # chained like the page flow (core/pipeline.py process_page_vision): the upscaler takes the page the inpaint stage produced
            # (a host image, as the operator API hands it over: one more upload), not the original
            src = pages[k]
            if inpainter is not None and outs.get("inpaint") is not None:
                src = torch.from_numpy(np.asarray(outs["inpaint"] if outs["inpaint"].mode == "RGB" else outs["inpaint"].convert("RGB"))).to(device)
            outs["upscale"] = upscaler.upscale_u8(src)
            tl = lap("upscale", tl)
        if clean_args is not None:
            dm_, bbs_ = clean_args[k]
            outs["clean"] = cl.process_bubbles(page_bgr[k], dm_, bbs_, 200, False, shrink_, **ckw)
            tl = lap("clean", tl)
        return outs

    def step(i):
        return stage_b(i, stage_a(i))

    overlap = not args.no_overlap and (yolo is not None or sam is not None) and (inpainter is not None or upscaler is not None or clean_args is not None)
    overlap = overlap or seg_in_b

    def run_steps(n):
        """n pages; with overlap, page i+1's front half runs on a worker thread beside page i's back half (a page still goes through its
        stages in order, and every page does all of its work inside the region that is timed).  Returns the last page's stage results."""
        last = None
        if not overlap or n < 2:
            for i in range(n):
                last = step(i)
            return last
        from collections import deque
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=n_front) as ex:
            futs = deque(ex.submit(stage_a, j) for j in range(min(n_front, n)))      # n_front front halves in flight, each on its own model instances
            nxt = len(futs)
            for i in range(n):
                work_ = futs.popleft().result()
                if nxt < n:
                    futs.append(ex.submit(stage_a, nxt))
                    nxt += 1
                last = stage_b(i, work_)
        return last

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    setup_pages = max(pool, n_front)
    for k in range(setup_pages):            # set-up, like model loading: every page of the pool once (on every model instance), so each stage's plans / hipGraphs for the
        step(k)                      # shapes it will meet (the FLUX crop resolution depends on where the text block sits) exist
    run_steps(args.warmup)
    barrier()
    t0, cpu0 = time.perf_counter(), time.process_time()
    last_outs = run_steps(args.steps)
    barrier()
    dt = time.perf_counter() - t0
    host_cpu_ms_per_page = 1e3 * (time.process_time() - cpu0) / max(1, args.steps)      # CPU time of every thread of this process over the timed region
    if flux is not None:          # every page sent its R regions through FLUX (none classified as solid, none dropped)
        want_calls = (setup_pages + args.warmup + args.steps) * args.regions
        assert flux.calls == want_calls, f"expected {want_calls} FLUX calls, saw {flux.calls}"
        assert flux.completed == want_calls, f"{want_calls - flux.completed} of {want_calls} FLUX calls raised (the OSB stage turns those into flat fills)"
    if args.dump_outputs and rank == 0:
        dump_outputs(last_outs, Path(args.dump_outputs))
    if rank == 0 and args.full:     # informational: wall clock of each stage of one more page, synchronised stage by stage
        stage_wall["_on"] = True
        step(0)
        stage_wall.pop("_on")
    batch_io = None
    if args.batch_io > 0:
        # ---- the batch harness end to end, image I/O included (row f2; not the metric) ----------------------------------------------
        import shutil
        import tempfile
        import types as _t
        from mangatranslator_amd.core.caching import UnifiedCache
        from mangatranslator_amd.core.pipeline import batch_process_images
        names = [tempfile.mkdtemp(prefix="mtx_batch_io_") if rank == 0 else None]
        if dist is not None:
            dist.broadcast_object_list(names, src=0)
        tmp = Path(names[0])
        n_io = args.batch_io * world
        if rank == 0:
            (tmp / "in").mkdir()
            for i in range(n_io):
                page_pil[i % pool].save(tmp / "in" / f"page_{i:04d}.png", compress_level=1)
        barrier()
        io_threads = args.io_threads or max(2, min(8, (os.cpu_count() or 8) // max(1, world) // 4))

        def io_front(page, path):
            i = int(path.stem.split("_")[1])
            k = i % pool
            rgb = page.convert("RGB")
            arr = np.asarray(rgb)
            pages[k].copy_(torch.from_numpy(arr))          # the decoded page replaces the resident one: upload inside the harness's clock
            page_bgr[k] = np.ascontiguousarray(arr[..., ::-1])
            page_pil[k] = rgb
            return i, page, stage_a(i)

        def io_front_whole(page, path):          # detect + segment only: the product's front half holds both stages (core/pipeline.py
            i, page, work_ = io_front(page, path)       # process_page_vision_front), pages overlap through front_workers instead
            stage_b(i, work_)
            return i, page, None

        def io_back(state):
            i, page, work_ = state
            outs = stage_b(i, work_) if not seg_in_b else {}
            if "upscale" in outs:
                return Image.fromarray(outs["upscale"].cpu().numpy())
            if "inpaint" in outs:
                return outs["inpaint"]
            return page

        # two pages in flight inside the harness too (core/pipeline.py, round 4) when the plain line runs that way and the pool has a slot per page in flight
        import contextlib

        @contextlib.contextmanager
        def io_slot(slot):
            harness_slot.slot = slot
            try:
                yield
            finally:
                harness_slot.slot = None

        io_pipelined = overlap and pool >= 2
        io_kw = (dict(process_front=io_front_whole if seg_in_b else io_front, process_back=io_back, front_workers=n_front, front_context=io_slot) if io_pipelined
                 else dict(process_image=lambda page, path: io_back((io_front_whole if seg_in_b else io_front)(page, path))))

        io_cfg = _t.SimpleNamespace(verbose=False, output=_t.SimpleNamespace(output_format="png", jpeg_quality=95, png_compression=2))
        h0, c0 = UnifiedCache.hash_seconds, UnifiedCache.hash_calls
        barrier()
        t_io = time.perf_counter()
        res_io = batch_process_images(tmp / "in", io_cfg, tmp / "out", io_threads=io_threads, **io_kw)
        barrier()
        dt_io = time.perf_counter() - t_io
        io_ = res_io.get("io", {})
        out_bytes = sum(f.stat().st_size for f in (tmp / "out").glob("*.png")) if rank == 0 else 0
        batch_io = {"pages": n_io, "wall_s": round(dt_io, 3), "pages_per_s_with_io": n_io / dt_io, "pages_in_flight": io_.get("pages_in_flight", 1), "succeeded": res_io["success_count"], "failed": res_io["error_count"],
                    "io_threads_per_rank": io_threads, "decode_ms_per_page": round(io_.get("decode_ms_per_page", 0.0), 2),
                    "encode_ms_per_page": round(io_.get("encode_ms_per_page", 0.0), 2), "process_ms_per_page": round(io_.get("process_ms_per_page", 0.0), 2),
                    "hash_ms_per_page": round(1e3 * (UnifiedCache.hash_seconds - h0) / max(1, args.batch_io), 2), "hash_calls_per_page": (UnifiedCache.hash_calls - c0) / max(1, args.batch_io),
                    "gpu_wait_for_decode_ms_per_page": round(1e3 * io_.get("gpu_wait_for_decode_s", 0.0) / max(1, n_io), 2),
                    "wait_for_save_slot_ms_per_page": round(1e3 * io_.get("wait_for_save_slot_s", 0.0) / max(1, n_io), 2), "max_pending_saves": io_.get("max_pending_saves"),
                    "input": f"{n_io} PNG files ({W_}x{H_}, compress_level 1)", "output": f"PNG, native writer (csrc/host_png.cpp: reductions + per-row filters + {io_threads and 8}-stripe parallel deflate, zlib level 6; oxipng absent), {out_bytes / max(1, n_io) / 1e6:.2f} MB per page",
                    "front_workers": n_front if io_pipelined else 1,
                    "note": (f"{io_.get('pages_in_flight', 2)} pages in flight inside the harness (core/pipeline.py batch_process_images(process_front=, process_back=, "
                             f"front_workers={n_front}))" if io_pipelined else "pages go through the stages one at a time here")}
        if rank == 0:
            shutil.rmtree(tmp, ignore_errors=True)
    if dist is not None:
        t = torch.tensor([dt], device=device if dist.get_backend() == "nccl" else "cpu", dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    pages_per_s = world * args.steps / dt

    if flux is None:
        inp_desc = None
    elif klein:
        c_ = flux.transformer.cfg
        inp_desc = (f"FLUX.2-Klein-{args.inpainter[-2:].upper()} geometry ({c_['layers']} double + {c_['single_layers']} single blocks, d={c_['d']}, {c_['heads']} heads), "
                    f"block linears {'MX fp8 e4m3 (v_mfma_scale_f32_32x32x64_f8f6f4)' if flux.transformer.fp8 else 'bf16'}, rest bf16, seeded random weights")
    else:
        inp_desc = "FLUX.1-Kontext-dev geometry (19 double + 38 single blocks, d=3072, 24 heads), bf16, seeded random weights"
    stage_names = "+".join(st for st in stages)
    headline = stages == ["detect", "segment", "inpaint", "upscale"] and (W_, H_) == (1024, 1536) and not klein
    result = {
        "metric": "pages/sec (detect+segment+inpaint+upscale) 1024x1536" if headline else f"pages/sec ({stage_names}) {W_}x{H_}",
        "value": pages_per_s, "unit": "pages/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": 1000.0 * dt / args.steps, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": dtype_string(stages, klein and flux is not None and flux.transformer.fp8,
                                                     fp8_attention=(klein and flux is not None and (getattr(flux.transformer, "attn_qk_f8", False), getattr(flux.transformer, "attn_pv_f8", False)))),
        "data": "synthetic",
        "config": {"workload": f"{W_}x{H_} synthetic pages, BASELINE.json configs[{args.config - 1}] per GPU ({stage_names}): one page per step per GPU, "
                               f"{args.boxes} bubbles" + (f", {args.regions} FLUX region(s) x {args.inpaint_steps} steps" if flux is not None else "")
                               + (", 2x upscale" if upscaler is not None else "") + "; HBM-resident input",
                   "baseline_config": args.config,
                   "stages": stages, "stage_memo": "cleared before every page (no cached outputs in the timed region)",
                   "dtypes": {"detect": "f16", "segment": "bf16", "inpaint": "bf16 (fp32 latents / Euler update)" + (" with MX-fp8 block linears" if klein and flux is not None and flux.transformer.fp8 else ""), "upscale": "f16"},
                   "detector": (("YOLO11m-seg (yolo_2, the reference's default)" if args.bubble_detector == "yolo_2" else "YOLOv8m-seg (yolo_1)")
                                + " @imgsz 1600 + RT-DETR-v2 R50 @640 (secondary)"
                                + (" + YOLO11-L panel detector @640 + YOLO12x outside-text detector @640" if aux_detectors else "") + ", seeded random weights") if yolo is not None else None,
                   "segmenter": (f"SAM-2.1 Hiera-L (HF Sam2Model layout), seeded random weights, precision {args.sam_precision!r}"
                                 + (" (the product's rule for this stage set)" if args.sam_precision_rule else " (--sam-precision)")) if sam is not None else None,
                   "inpainter": inp_desc,
                   "upscaler": ({"arch": "RCAN", **rcan_cfg, "weights": "seeded random"} if upscaler is not None else None),
                   "detector_calls": ("one after the other" if args.serial_detectors else "submitted together, one HIP stream per model, collected afterwards") if yolo is not None else None,
                   "front_replicas": n_front,
                   "host_cpu_ms_per_page": round(host_cpu_ms_per_page, 2),      # all threads; near ms_per_step = the Python side of the page loop is what the pages wait for

                   "detector_batch": ({"pages_per_replay_max": args.detector_batch,
                                       **{n_: {"pages": d_.stats["pages"], "graph_replays": d_.stats["launches"]} for n_, d_, _c in (aux_detectors or []) if hasattr(d_, "stats")},
                                       **({"rtdetr": {"pages": rtdetr.stats["pages"], "graph_replays": rtdetr.stats["launches"]}} if hasattr(rtdetr, "stats") else {})}
                                      if args.detector_batch > 1 and aux_detectors else None),
                   "stage_wall_ms_one_page": {k_: round(v_, 2) for k_, v_ in stage_wall.items()},
                   "page_pipeline": ("two pages in flight: detectors (+ SAM encoder) of page i+1 on a worker thread beside the SAM mask decoder of page i" if seg_in_b else
                                     "two pages in flight: detect / segment / OSB prepare of page i+1 on a worker thread beside inpaint / upscale / clean of page i"
                                     if overlap else "stages strictly in order, one page at a time"),
                   "parallelism": f"page-sharded x{world}, weights broadcast once over RCCL",
                   "host_threads_per_rank": host_threads, "host_placement": placement, "hw_queues": os.environ.get("GPU_MAX_HW_QUEUES", "runtime default (4)"),
                   "launch": {"world_size_seen_by_collectives": (dist.get_world_size() if dist is not None else 1), "backend": (dist.get_backend() if dist is not None else None),
                              "self_launched": os.environ.get("MTX_BENCH_SELF_LAUNCHED") == "1", "model_setup_and_weight_broadcast_s": round(load_s, 2)}},
    }
    cfg = result["config"]
    if batch_io is not None:
        cfg["batch_io"] = batch_io
    if klein and flux is not None:
        cfg["attn_pv_f8"] = bool(getattr(flux.transformer, "attn_pv_f8", False))      # P V on the fp8 instruction too (fp8 path only; 41.8 dB against the bf16 pipeline)
        cfg["attn_qk_f8"] = bool(getattr(flux.transformer, "attn_qk_f8", False))      # scores from e4m3 q / k (fp8 path only; 41.9 dB against the bf16 pipeline, tests/test_flux2_gpu.py)
    if flux is not None and not klein:
        st_ = getattr(flux, "cache_stats", {"steps": 0, "skipped": 0})
        on_ = args.kontext_backend == "nunchaku" and args.residual_diff_threshold > 0
        cfg["first_block_cache"] = ({"state": f"on (backend nunchaku, residual_diff_threshold {args.residual_diff_threshold}; reference model_manager.py:1159-1162)",
                                     "denoising_steps": st_["steps"], "steps_skipped": st_["skipped"],
                                     "steps_skipped_per_page": st_["skipped"] / max(1, flux.calls) * args.regions,
                                     "note": "seeded random weights: how often the probe passes says nothing about a trained model; parity with nunchaku unpinned"} if on_
                                    else {"state": f"off (backend {args.kontext_backend}: every step runs every block)", "steps_skipped": st_["skipped"]})

    if rank == 0 and args.full:
        # ---- per-stage GPU time (HIP events on the launch stream), outside the timed region ---------------
        if sam is not None:
            pre, enc, dec, post = sam.plans(args.boxes, H_, W_)
            cfg["segment_ms"] = {"preprocess": pre.time(5), "encoder": enc.time(5), "decoder": dec.time(5), "upsample_threshold": post.time(5)}
        if yolo is not None:
            cfg["detect_net_ms"] = yolo._plans[(H_, W_, 1600)][0].time(5)
            # (a batching wrapper: one replay of its batched graph, divided by the pages it carries when full — what a page costs in a full batch)
            cfg["detect_aux_ms"] = {name_: (det_._sets[(H_, W_, 640)][0].plan.time(5) / det_.batch if hasattr(det_, "_sets") else det_._plans[(H_, W_, 640)][0].time(5))
                                    for name_, det_, _ in aux_detectors}
            if hasattr(rtdetr, "_sets"):          # batching wrapper: the batched encoder replay divided by its pages, the decoder per page as it runs
                set0 = rtdetr._sets[(640, 640, "rtdetr")][0]
                cfg["detect_rtdetr_ms"] = {"backbone_encoder": set0.enc.time(5) / rtdetr.batch, "decoder": set0.dec.time(5)}
            else:
                ra, rb = rtdetr.plans(640, 640)
                cfg["detect_rtdetr_ms"] = {"backbone_encoder": ra.time(5), "decoder": rb.time(5)}
        # wall clock of a stage (one page, synchronised) against the GPU time of its graphs: what is left is host work (NMS, prompt set-up,
        # downloads) — the share the page pipeline hides behind the next page's GPU work
        split = {}
        if yolo is not None and "detect" in stage_wall:
            gpu_ = cfg["detect_net_ms"] + sum(cfg["detect_rtdetr_ms"].values()) + sum(cfg["detect_aux_ms"].values())
            split["detect"] = {"wall_ms": round(stage_wall["detect"], 2), "gpu_graph_ms": round(gpu_, 2), "host_ms": round(stage_wall["detect"] - gpu_, 2)}
        if sam is not None and "segment" in stage_wall:
            gpu_ = sum(cfg["segment_ms"].values())
            split["segment"] = {"wall_ms": round(stage_wall["segment"], 2), "gpu_graph_ms": round(gpu_, 2), "host_ms": round(stage_wall["segment"] - gpu_, 2)}
        cfg["host_gpu_split_one_page"] = split
        # not part of the metric, reported for reference: the OpenCV-style cleaning chain on the page's 8 bubbles
        try:
            if clean_args is not None:
                raise RuntimeError("timed as a stage of this run")
            from mangatranslator_amd.core.image import cleaning as cl
            yy, xx = np.mgrid[0:H_, 0:W_]
            bm = []
            for x0, y0, x1, y1 in page_boxes[0]:
                cx, cy, a_, b_ = (x0 + x1) / 2, (y0 + y1) / 2, (x1 - x0) / 2 - 4, (y1 - y0) / 2 - 4
                bm.append((((xx - cx) / a_) ** 2 + ((yy - cy) / b_) ** 2 <= 1.0).astype(np.uint8) * 255)
            dm = torch.from_numpy(np.stack(bm)).to(device)
            sc = (W_ * H_ / 1e6) ** 0.5
            kw = dict(dilation_kernel=cl.structuring_element(cl.scale_kernel(cl.DILATION_KERNEL_SIZE, sc)),
                      constraint_erosion_kernel=cl.structuring_element(cl.scale_kernel(cl.EROSION_KERNEL_SIZE, sc)),
                      min_contour_area=cl.scale_area(50, sc, minimum=50, maximum=5000), processing_scale=sc, device=device, lib=lib)
            bbs = [tuple(int(v) for v in b_) for b_ in page_boxes[0]]
            cl.process_bubbles(page_bgr[0], dm, bbs, 200, False, float(cl.scale_scalar(5, sc, minimum=0.0, maximum=64.0)), **kw)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(3):
                cl.process_bubbles(page_bgr[0], dm, bbs, 200, False, float(cl.scale_scalar(5, sc, minimum=0.0, maximum=64.0)), **kw)
            torch.cuda.synchronize()
            cfg["clean_ms_not_in_metric"] = (time.perf_counter() - t0) / 3 * 1e3
        except Exception as e:      # informational only
            cfg["clean_ms_not_in_metric"] = f"failed: {e}"
        if upscaler is not None:
            cfg["upscale_ms"] = upscaler.plan_for(1, H_, W_).time(3)
        if flux is not None and not args.traffic_child:      # (the counter child only needs the page's own launches: no timing replays)
            key, plan = next(iter(flux.transformer._plans.items()))
            t_txt, h2, w2 = key[0], key[1], key[2]
            fl = flux.transformer.flops_per_step(*key[:3]) if not klein else flux.transformer.flops_per_step(*key)
            # With the first-block cache on, a step is TWO graphs — the head (embedders, double block 0, the probe) and, when the step is
            # computed, the body (the other 56 blocks): `plan` is the head and carries the body.  A computed step is what is timed and priced here
            # (dividing the whole step's flops by the head's time read 23x the chip's peak).
            parts_ = [plan] + ([plan.body] if hasattr(plan, "body") else [])
            for p_ in parts_:
                p_.time(6 if len(parts_) == 1 else 3, graph=True)   # ~1 s of sustained load first: the chip boosts for the first few steps after an idle phase and
            part_ms = [p_.time(4, graph=True) for p_ in parts_]    # then settles (rocprof: 0.71 ms vs 0.83 ms per attention launch); the steady state is what a page
            step_ms = sum(part_ms)
            # sees.  Timed as the hipGraph replay the pipeline runs (with the text stream on its side lane), not as eager launches
            cfg["dit_step_ms_one_lane_eager"] = sum(p_.time(2) for p_ in parts_)
            rh2, rw2 = (key[3], key[4]) if klein else (h2, w2)
            cfg["inpaint"] = {"resolution": [w2 * 16, h2 * 16], "tokens": fl["tokens"], "dit_step_ms": step_ms,
                              "dit_tflops": (fl["gemm"] + fl["attention"]) / step_ms / 1e9,
                              "vae_encode_ms": flux.vae.encoder_plan(rh2 * 16, rw2 * 16).time(2), "vae_decode_ms": flux.vae.decoder_plan(h2 * 2, w2 * 2).time(2)}
            if len(parts_) > 1:
                cfg["inpaint"]["dit_step_parts_ms"] = {"head (embedders + block 0 + probe)": part_ms[0], "body (56 blocks + projection)": part_ms[1]}
            # ---- in-context time of every MFMA-bound launch of one denoising step, grouped by kernel and problem shape -----------------------
            # (hipGraph replay of the whole step; per group: device wall-clock stamps around its ops, or graph with minus graph without them)
            import ctypes as C_
            from mangatranslator_amd.hip import abi as abi_
            groups = {}
            for pi_, p_ in enumerate(parts_):
                for i_, lab in enumerate(p_.labels):
                    op_ = p_.ops[i_] if hasattr(p_, "ops") else None
                    if lab.endswith(".attn"):
                        groups.setdefault(("attention", fl["tokens"], fl["tokens"], flux.transformer.cfg["d"]), {}).setdefault(pi_, []).append(i_)
                    elif op_ is not None and op_.kind == abi_.OP_GEMM and lab.split(".")[0][:3] in ("sgl", "dbl"):
                        g_ = op_.u.gemm
                        groups.setdefault(("gemm_fp8" if g_.in_dtype == abi_.F8 else "gemm_bf16", int(g_.m), int(g_.n), int(g_.k)), {}).setdefault(pi_, []).append(i_)
            rows, tot = [], {}
            for (kind_, m_, n_, k_), by_part in sorted(groups.items(), key=lambda kv: -sum(len(v_) for v_ in kv[1].values())):
                flops_ = (4.0 * m_ * n_ * k_) if kind_ == "attention" else (2.0 * m_ * n_ * k_)        # attention: M = N = T, K = d_model: 4 T^2 D
                ms_, how_, info_, n_l = 0.0, set(), {}, 0
                for pi_, idx_ in by_part.items():
                    m1, h1, i1 = in_context_ms(parts_[pi_], idx_, 3, args.time_ops, replay_ms=part_ms[pi_])
                    ms_ += m1; how_.add(h1); n_l += len(idx_)
                    info_ = i1 if len(by_part) == 1 else {**info_, f"part{pi_}": i1}
                how_ = "+".join(sorted(how_))
                idx_ = range(n_l)
                peak_ = FP8_PEAK_TFLOPS if kind_ == "gemm_fp8" else MFMA_PEAK_TFLOPS
                if kind_ == "attention" and getattr(flux.transformer, "attn_qk_f8", False):
                    peak_ = 2.0 / (1.0 / FP8_PEAK_TFLOPS + 1.0 / MFMA_PEAK_TFLOPS)      # Q K^T on the fp8 instruction, P V on the 16-bit one (see roofline_attention)
                    if getattr(flux.transformer, "attn_pv_f8", False):
                        peak_ = FP8_PEAK_TFLOPS
                rows.append({"kernel": kind_, "m": m_, "n": n_, "k": k_, "launches_per_step": len(idx_), "mean_ms": ms_ / len(idx_), "timing": how_,
                             "timing_detail": info_, "tflops": flops_ * len(idx_) / ms_ / 1e9, "frac_of_peak": flops_ * len(idx_) / ms_ / 1e9 / peak_})
                t_ = tot.setdefault(kind_, [0.0, 0.0, 0])
                t_[0] += flops_ * len(idx_); t_[1] += ms_; t_[2] += len(idx_)
            cfg["inpaint"]["mfma_launch_groups"] = rows
            cfg["inpaint"]["step_ms_accounted_by_groups"] = sum(r_["mean_ms"] * r_["launches_per_step"] for r_ in rows)
            n_attn = len(flux.transformer.blocks) + len(flux.transformer.singles)

            def roof(kind_, kernel_name, peak_):
                f_, ms_, n_ = tot[kind_]
                return {"kernel": kernel_name, "bound": "mfma", "achieved": f_ / ms_ / 1e9, "peak": peak_, "unit": "TFLOP/s", "frac": f_ / ms_ / 1e9 / peak_,
                        "traffic": None, "avg_launch_ms": ms_ / n_, "timing": "in-context (see config.inpaint.mfma_launch_groups)",
                        "launches_per_page": n_ * args.inpaint_steps * args.regions, "algorithmic_flops_per_launch": f_ / n_,
                        "share_of_step_ms": ms_ / step_ms}
            roofs = {}
            if "attention" in tot:
                if getattr(flux.transformer, "attn_qk_f8", False):
                    # half of the flops (Q K^T) run on the fp8 matrix instruction at FP8_PEAK, half (P V) on the 16-bit one: the launch's ideal time is
                    # F/2 / FP8_PEAK + F/2 / MFMA_PEAK, i.e. the peak it is priced against is the harmonic mix (3 333 TFLOP/s), not 2 500
                    mix_ = 2.0 / (1.0 / FP8_PEAK_TFLOPS + 1.0 / MFMA_PEAK_TFLOPS)
                    if getattr(flux.transformer, "attn_pv_f8", False):      # P V on the fp8 instruction too: every flop at the fp8 rate
                        mix_ = FP8_PEAK_TFLOPS
                    roofs["attention"] = roof("attention", (f"attn_mma32_k8v8q_kernel<bf16, 128> (scores from e4m3 q / k AND P V from e4m3 p / v on v_mfma_scale_f32_32x32x64_f8f6f4) " if getattr(flux.transformer, "attn_pv_f8", False) else
                                                            f"attn_mma32_k8q_kernel<bf16, 128> (scores from e4m3 q / k on v_mfma_scale_f32_32x32x64_f8f6f4, P V 16-bit) ") + 
                                                           f"{flux.transformer.cfg['heads']} heads, {fl['tokens']}x{fl['tokens']} tokens (MMDiT joint attention)", mix_)
                    roofs["attention"]["peak_note"] = ("the fp8 dense peak (both products)" if getattr(flux.transformer, "attn_pv_f8", False)
                                                       else "harmonic mix of the fp8 (Q K^T) and 16-bit (P V) dense peaks")
                else:
                    roofs["attention"] = roof("attention", f"attn_mma32_kernel<bf16, 128> {flux.transformer.cfg['heads']} heads, {fl['tokens']}x{fl['tokens']} tokens (MMDiT joint attention)", MFMA_PEAK_TFLOPS)
            if "gemm_bf16" in tot:
                roofs["gemm_bf16"] = roof("gemm_bf16", "gemm256_kernel<bf16> (256x256x64 LDS-DMA tiles) + 128-tile kernel, block linears of one MMDiT step", MFMA_PEAK_TFLOPS)
            if "gemm_fp8" in tot:
                roofs["gemm_fp8"] = roof("gemm_fp8", "gemm256_f8_kernel (256x256x128 LDS-DMA tiles, v_mfma_scale_f32_32x32x64_f8f6f4, MX e4m3), block linears of one MMDiT step", FP8_PEAK_TFLOPS)
            # `roofline` = the group with the largest share of the step's time; the others ride along under their own keys
            dom = max(roofs, key=lambda k_: roofs[k_]["share_of_step_ms"])
            result["roofline"] = roofs.pop(dom)
            for k_, v_ in roofs.items():
                result["roofline_" + k_] = v_
        if upscaler is not None and not args.traffic_child:
            # ---- the HBM-bound kernel the north star names: RCAN 3x3 conv 64->64 at page resolution -------
            u = upscaler.hp["unshuffle"]
            plan = upscaler.plan_for(1, H_, W_)
            # an RCAB's two launches of it: conv1 (+ ReLU + channel sums) moves in + out; conv2 (+ attention factors + residual) also reads
            # the block's input as its residual — 1.5x the bytes.  The figure is the pair's bytes over the pair's time.
            work = upscaler.work(H_, W_)
            act_bytes = work["conv64_bytes"] - 9 * 64 * 64 * 2
            pair, pair_bytes = {}, 0.0
            for nm_, extra_ in (("g0b0.conv1", 0.0), ("g0b0.conv2", act_bytes / 2 if getattr(upscaler, "pool_before_conv", False) else 0.0)):
                idx = plan.labels.index(nm_)
                plan.time_range(idx, idx, 3)
                pair[nm_] = {"ms": plan.time_range(idx, idx, 20), "algorithmic_bytes": work["conv64_bytes"] + extra_}
                pair_bytes += pair[nm_]["algorithmic_bytes"]
            ms = sum(v_["ms"] for v_ in pair.values()) / 2
            gbs = pair_bytes / 2 / (ms * 1e-3) / 1e9
            tfs = work["conv64_flops"] / (ms * 1e-3) / 1e12
            conv_roof = {
                "kernel": "conv3x3_c64_kernel<f16> 64->64 @%dx%d, the two convs of an RCAB" % (W_ // u, H_ // u), "per_conv": pair,
                "bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS,
                "traffic": None,          # PMC bytes are taken in separate rocprofv3 --pmc passes of this command (profiles/), never copied into the line
                "avg_launch_ms": ms, "timing": "event pair around 20 eager launches", "launches_per_page": work["n_conv64"],
                "algorithmic_bytes_per_launch": pair_bytes / 2, "mfma_tflops": tfs, "mfma_frac": tfs / MFMA_PEAK_TFLOPS,
            }
            if "roofline" in result:
                result["roofline_upscale_conv"] = conv_roof
            else:
                result["roofline"] = conv_roof
        if not args.no_traffic and not args.traffic_child and world == 1 and "roofline" in result:
            result["roofline"]["traffic"], result["roofline"]["traffic_detail"] = measure_traffic(result["roofline"]["kernel"])
        if (world == 1 and headline and not args.no_extra and not args.extra_child and not args.traffic_child
                and args.kontext_backend == "sdnq" and args.sam_precision_rule):
            result["extra"] = run_extra_children()
        if not args.no_cpu_baseline and world == 1:          # the CPU leg is a single-GPU-run item (rank 0 at N = 1 only)
            result["cpu_baseline"] = cpu_baseline(stages, rcan_sd, W_, H_, args, cfg.get("inpaint"), flux.transformer.cfg if (klein and flux is not None) else None)
    if rank == 0:
        print(json.dumps(result))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


def run_extra_children():
    """The other BASELINE configurations under the driver's clock: after the timed region of the default command, this very
    script is run again as child processes — the GPU is idle by then; each child loads its own models, times its own region with the same
    barrier discipline and prints its own JSON line, of which the figures are kept:
      config5  8 pages at 2048x3072, FLUX.2-Klein-4B with MX-fp8 block linears, 8 steps, + 2x upscale (BASELINE configs[4]; the reference's DEFAULT inpainter)
      config2  64 pages, detect + segment only (BASELINE configs[1]), two front halves in flight on sixteen hardware queues
      first_block_cache  3 pages of config 3 with the OSB stage configured for the reference's nunchaku backend (first-block cache on)
      upscale_model_lite_assumed_shape  the upscale stage alone with the reference's CLI-default upscaler, shape assumed (VERDICT r05 missing #3)"""
    import subprocess
    me = [sys.executable, str(Path(__file__).resolve()), "--full", "--no-cpu-baseline", "--no-traffic", "--extra-child"]
    jobs = {"config5": ["--config", "5", "--steps", "8", "--warmup", "2"],
            "config2": ["--config", "2", "--steps", "64", "--warmup", "4"],
            "first_block_cache": ["--config", "3", "--steps", "3", "--warmup", "1", "--kontext-backend", "nunchaku"],
            # the reference's CLI-default upscaler (core/config.py:185 image_upscale_model = "model_lite", the Fast_RCAN_PU file): ASSUMED shape
            # (4 groups x 8 blocks x 64 features, pixel-unshuffle 2) — the real hyper-parameters come from the checkpoint's header, which is not here
            "upscale_model_lite_assumed_shape": ["--stages", "upscale", "--upscale-model", "model_lite", "--steps", "10", "--warmup", "3"]}
    out = {}
    env = {k: v for k, v in os.environ.items() if k != "GPU_MAX_HW_QUEUES"}          # each child picks its own queue count (see _early_hw_queues)
    for name, extra_args in jobs.items():
        t0 = time.perf_counter()
        try:
            r = subprocess.run(me + extra_args, capture_output=True, text=True, timeout=420, env=env)
            line = next((l for l in reversed(r.stdout.splitlines()) if l.startswith("{")), None)
            if r.returncode != 0 or line is None:
                out[name] = {"error": f"rc {r.returncode}: {(r.stderr or r.stdout)[-300:]}"}
                continue
            d = json.loads(line)
            c = d.get("config", {})
            keep = {"command": "python bench.py " + " ".join(extra_args), "metric": d["metric"], "value": d["value"], "unit": d["unit"], "steps": d["steps"], "warmup": d["warmup"],
                    "ms_per_step": d["ms_per_step"], "dtype": d["dtype"], "workload": c.get("workload"), "wall_s_incl_model_setup": round(time.perf_counter() - t0, 1)}
            for k in ("roofline", "roofline_attention", "roofline_gemm_fp8", "roofline_gemm_bf16", "roofline_upscale_conv"):
                if k in d:
                    keep[k] = {kk: vv for kk, vv in d[k].items() if kk not in ("traffic_detail", "per_conv")}
            for k in ("stage_wall_ms_one_page", "front_replicas", "hw_queues", "segment_ms", "detect_net_ms", "upscale_ms", "first_block_cache", "inpainter", "segmenter", "upscaler"):
                if k in c:
                    keep[k] = c[k]
            if "inpaint" in c:
                keep["inpaint"] = {kk: c["inpaint"][kk] for kk in ("resolution", "tokens", "dit_step_ms", "dit_tflops", "vae_encode_ms", "vae_decode_ms") if kk in c["inpaint"]}
            out[name] = keep
        except subprocess.TimeoutExpired:
            out[name] = {"error": "did not finish in 420 s"}
        except Exception as e:      # noqa: BLE001 — an extra must never cost the headline line
            out[name] = {"error": str(e)[:300]}
    return out


def measure_traffic(kernel_desc: str):
    """HBM-side bytes per launch of the dominant kernel group, from counter passes over this very bench command (one page, nothing else
    changed): `rocprofv3 --pmc FETCH_SIZE --kernel-trace` and a second pass with WRITE_SIZE (they do not fit one pass on gfx950; counters
    only, never combined with sys / hip trace domains).  FETCH_SIZE and WRITE_SIZE are in KB; FETCH_SIZE counts 128-byte requests at 64 B
    on gfx950 and is doubled (MI355X_MICROARCH.md, HBM).  Infinity-Cache hits are counted, so this is fabric-side traffic."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    if shutil.which("rocprofv3") is None:
        return None, {"error": "rocprofv3 not on PATH"}
    want = "attn_mma32" if kernel_desc.startswith("attn") else ("conv3x3_c64" if kernel_desc.startswith("conv") else "gemm256")
    base = [a_ for a_ in sys.argv[1:] if a_ not in ("--with-traffic", "--no-traffic") and not a_.startswith("--dump-outputs=")]
    for flag in ("--steps", "--warmup", "--stages", "--inpaint-steps", "--batch-io", "--dump-outputs"):
        if flag in base:
            i_ = base.index(flag)
            del base[i_:i_ + 2]
    # only the stage that owns the kernel, and ONE denoising step: every launch of a group moves the same bytes, and a counter pass costs
    # tens of milliseconds per dispatch (a whole 20-step page under --pmc ran past 25 minutes, r03)
    base += ["--stages", "upscale"] if want == "conv3x3_c64" else ["--stages", "inpaint", "--inpaint-steps", "1"]
    # eager launches: rocprofv3's counter mode segfaulted on hipGraph replays (r03); the kernels and their arguments are the same
    child = [sys.executable, str(Path(__file__).resolve())] + base + ["--steps", "1", "--warmup", "0", "--no-cpu-baseline", "--no-overlap", "--no-graph", "--traffic-child"]
    per = {}
    import types as types_
    detail = {"command": "rocprofv3 --pmc <FETCH_SIZE | WRITE_SIZE> --kernel-trace --output-format csv -- python bench.py " + " ".join(child[2:]), "kernels": {}}
    for counter in ("FETCH_SIZE", "WRITE_SIZE"):
        tmp = tempfile.mkdtemp(prefix="mtx_pmc_")
        try:
            import signal
            proc = subprocess.Popen(["rocprofv3", "--pmc", counter, "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "t", "--"] + child,
                                    cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True)
            try:
                _, err_ = proc.communicate(timeout=150)
            except subprocess.TimeoutExpired:
                os.killpg(proc.pid, signal.SIGKILL)          # the profiler AND the bench process under it (its own process group)
                proc.communicate()
                return None, {"error": f"{counter} pass did not finish in 150 s"}
            r = types_.SimpleNamespace(returncode=proc.returncode, stderr=err_)
            files = glob.glob(tmp + "/**/*counter_collection.csv", recursive=True)
            if r.returncode != 0 or not files:
                return None, {"error": f"{counter} pass failed (rc {r.returncode}): {r.stderr[-300:]}"}
            tot, n = {}, {}
            for fn in files:
                for row in csv.DictReader(open(fn)):
                    if row["Counter_Name"] == counter and want in row["Kernel_Name"]:
                        k_ = row["Kernel_Name"][:90]
                        tot[k_] = tot.get(k_, 0.0) + float(row["Counter_Value"]); n[k_] = n.get(k_, 0) + 1
            per[counter] = (tot, n)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    rd_t, rd_n = per["FETCH_SIZE"]
    wr_t, wr_n = per["WRITE_SIZE"]
    launches = sum(rd_n.values())
    if launches == 0:
        return None, {"error": f"no '{want}' dispatches in the counter pass"}
    rd = 2.0 * 1024.0 * sum(rd_t.values()) / launches
    wr = 1024.0 * sum(wr_t.values()) / max(1, sum(wr_n.values()))
    for k_ in rd_t:
        detail["kernels"][k_] = {"launches": rd_n[k_], "read_bytes_per_launch": round(2.0 * 1024.0 * rd_t[k_] / rd_n[k_]),
                                 "write_bytes_per_launch": round(1024.0 * wr_t.get(k_, 0.0) / max(1, wr_n.get(k_, 1)))}
    detail.update(launches=launches, read_bytes_per_launch=round(rd), write_bytes_per_launch=round(wr),
                  note="fabric-side bytes (Infinity-Cache hits counted), mean over every launch of the group in one page")
    return rd + wr, detail


DUMP_BUDGET_BYTES = 64 << 20
DUMP_MAX_ELEMS = 1 << 20       # larger arrays are stored as this many elements at fixed, seeded positions (the same ones for the same size)


def _output_arrays(obj, name, out):
    """flatten a stage result into named arrays: tensors, numpy arrays, PIL images, numbers, and the detector results' boxes / masks"""
    from PIL import Image
    if obj is None:
        return
    if isinstance(obj, torch.Tensor):
        out[name] = obj.detach().float().cpu().numpy()
    elif isinstance(obj, np.ndarray):
        out[name] = obj
    elif isinstance(obj, Image.Image):
        out[name] = np.asarray(obj)
    elif isinstance(obj, (bool, int, float, np.number)) or (isinstance(obj, (list, tuple)) and obj and all(isinstance(v, (bool, int, float, np.number)) for v in obj)):
        out[name] = np.asarray(obj)          # a number, or a colour / box given as a tuple of numbers
    elif isinstance(obj, (list, tuple)):      # e.g. the cleaning stage: one tuple (or None) per bubble
        for i, v in enumerate(obj):
            _output_arrays(v, f"{name}_{i}", out)
    elif hasattr(obj, "boxes"):          # a detector's Results: (N, 6) rows of x0, y0, x1, y1, conf, cls, and the instance masks where there are any
        b = obj.boxes                    # (None when nothing passed the threshold)
        out[name + "_boxes"] = (np.zeros((0, 6)) if b is None else
                                torch.cat([b.xyxy.float().reshape(-1, 4), b.conf.float().reshape(-1, 1), b.cls.float().reshape(-1, 1)], 1).cpu().numpy())
        if getattr(obj, "masks", None) is not None:
            out[name + "_masks"] = obj.masks.data.float().cpu().numpy()


def dump_outputs(outs, out_dir: Path):
    """DIR/<stage>[_<part>].npy, float32, of one page's stage results; an array of more than DUMP_MAX_ELEMS elements keeps a sorted, seeded
    sample of them (seed and positions depend only on the array's size, so two runs / builds sample the same elements).  A result with no
    elements (a detector that found nothing on the page) has nothing to compare and is not written."""
    arrays = {}
    for k in sorted(outs or {}):
        _output_arrays(outs[k], k, arrays)
    arrays = {name: a for name, a in arrays.items() if np.asarray(a).size > 0}
    out_dir.mkdir(parents=True, exist_ok=True)
    cap = max(1, min(DUMP_MAX_ELEMS, (DUMP_BUDGET_BYTES // max(1, len(arrays)) - 1024) // 4))      # (1 KB per file for the .npy header)
    for name, a in arrays.items():
        a = np.asarray(a, dtype=np.float32)
        if a.size > cap:
            idx = np.sort(np.random.default_rng(a.size).choice(a.size, cap, replace=False))
            a = a.reshape(-1)[idx]
        np.save(out_dir / f"{name}.npy", a)


def dtype_string(stages, fp8_linears, fp8_attention=None):
    """The arithmetic the timed stages compute in, by stage — the storage types narrower than the reference's fp32 are named in the top-level
    field, not only in `config.dtypes`: the detectors and the RCAN upscaler store f16 where the reference runs fp32."""
    parts = []
    if "inpaint" in stages:
        attn = ""
        if fp8_linears and fp8_attention and fp8_attention[0]:          # the fp8 path's attention: e4m3 q / k (and p / v) on the fp8 matrix instruction
            attn = " + e4m3 attention " + ("scores and P V" if fp8_attention[1] else "scores")
        parts.append("fp8 (e4m3, MX block scales) block linears" + attn + " + bf16 DiT / VAE" if fp8_linears else "bf16 DiT / VAE")
    if "detect" in stages:
        parts.append("f16 detectors")
    if "segment" in stages:
        parts.append("bf16 / f16 SAM trunk")
    if "upscale" in stages:
        parts.append("f16 upscaler")
    if "clean" in stages:
        parts.append("u8 cleaning")
    return ", ".join(parts) + "; fp32 accumulation throughout"


def in_context_ms(plan, idx, iters, mode, replay_ms=None):
    """Duration (ms per plan replay) of the ops `idx` inside the replayed plan.  "difference": hipGraph with minus hipGraph without the
    ops, HIP events around each replay — an upper bound on a power-limited chip, where the graph without the ops also clocks higher
    (run 20).  "stamp": device wall-clock stamps before and after each op inside ONE replay graph.  "auto": both; the
    stamps are reported when they land in a sanity band around the difference figure (0.6x .. 1.25x: a wrong clock rate would be far
    outside it), else the difference is.  A group that is a small share of the replay (< 15 % of `replay_ms`) has no usable
    difference figure — two replays of a 160 ms graph differ by more than such a group lasts (r02 visit D: 19 text-stream GEMMs,
    1.7 ms stamped, read 12.7 ms by difference) — so its stamps are taken as they are."""
    os.environ.pop("MTX_TIME_OPS", None)
    plan.time_ops(idx, 1)
    diff = plan.time_ops(idx, iters) / iters
    info = {"difference_ms_per_launch": diff / len(idx)}
    if mode == "difference":
        return diff, "difference", info
    stamped = None
    try:
        os.environ["MTX_TIME_OPS"] = "stamp"
        plan.time_ops(idx, 1)
        stamped = plan.time_ops(idx, iters) / iters
        info["stamp_ms_per_launch"] = stamped / len(idx)
    except Exception as e:                                    # a HIP error in the stamped replay: keep the difference figure
        info["stamp_error"] = str(e)[:160]
    finally:
        os.environ.pop("MTX_TIME_OPS", None)
    small = replay_ms is not None and max(diff, stamped or 0.0) < 0.15 * replay_ms
    if stamped is not None and stamped > 0 and (mode == "stamp" or small or 0.6 * diff <= stamped <= 1.25 * diff):
        return stamped, "stamp", info
    return diff, "difference", info


def cpu_baseline(stages, rcan_sd, W_, H_, args, inpaint_info, klein_cfg=None):
    """The oracle (CPU restatement, fp32 torch) timed on bounded samples of the same page; each stage's
    sample is scaled to the full page by its unit count (stated in `sample`)."""
    from mangatranslator_amd.utils.synthetic_pages import make_page
    cores = min(os.cpu_count() or 1, 32)     # the oracle's small convolutions stop scaling (and thrash) beyond this
    torch.set_num_threads(cores)
    pg, boxes, _ = make_page(0, W_, H_, bubbles=args.boxes)
    parts, total, spent = [], 0.0, 0.0

    def timed(fn):
        t0 = time.perf_counter()
        with torch.no_grad():
            fn()
        return time.perf_counter() - t0

    if "detect" in stages:
        from oracle import yolo_ref
        bgr = np.ascontiguousarray(pg[..., ::-1])
        if args.bubble_detector == "yolo_2":
            from oracle import yolo11_ref as y11p
            net = y11p.make_model("11", "m", 1, True, seed=3)
            t = timed(lambda: y11p.predict(net, bgr, imgsz=1600, conf=0.99))
            parts.append(f"detect: oracle YOLO11m-seg on the whole page {t:.2f} s"); total += t; spent += t
        else:
            net = yolo_ref.make_model("m", 1, seed=3)
            t = timed(lambda: yolo_ref.predict(net, bgr, imgsz=1600, conf=0.99))
            parts.append(f"detect: oracle YOLOv8m-seg on the whole page {t:.2f} s"); total += t; spent += t
        del net
        if not args.no_aux_detectors:
            from oracle import yolo11_ref as y11
            for nm_, fam_, sc_ in (("panel YOLO11-L", "11", "l"), ("outside-text YOLO12x", "12", "x")):
                n_ = y11.make_model(fam_, sc_, 1, False, seed=3)
                t = timed(lambda: y11.predict(n_, bgr, imgsz=640, conf=0.99))
                parts.append(f"{nm_} @640 {t:.2f} s"); total += t; spent += t
                del n_
    if "segment" in stages:
        from oracle import sam2_ref
        m, _ = sam2_ref.make_model("hiera_large", seed=11)
        t = timed(lambda: sam2_ref.run(m, pg, boxes))
        parts.append(f"segment: oracle SAM-2.1 Hiera-L on the whole page, {len(boxes)} boxes {t:.2f} s"); total += t; spent += t
        del m
    if "inpaint" in stages and inpaint_info is not None and klein_cfg is not None:
        from oracle import flux2_ref as f2r
        from oracle import flux_ref as fr
        T, t_txt, D, Hh = inpaint_info["tokens"], 512, klein_cfg["d"], klein_cfg["heads"]
        torch.manual_seed(0)
        dbl, sgl = f2r.DoubleBlock(D, Hh, klein_cfg["mlp_ratio"]).eval(), f2r.SingleBlock(D, Hh, klein_cfg["mlp_ratio"]).eval()
        ids = torch.zeros(T, 4); ids[:, 1] = torch.arange(T) % 64; ids[:, 2] = torch.arange(T) // 64
        cos, sin = fr.rope_tables(ids, klein_cfg["axes_dim"], theta=klein_cfg["rope_theta"])
        x = torch.randn(T, D)
        mod2 = [tuple(0.1 * torch.randn(D) for _ in range(3)) for _ in range(2)]
        td = timed(lambda: dbl(x[t_txt:], x[:t_txt], mod2, mod2, cos, sin))
        ts = timed(lambda: sgl(x, mod2[0], cos, sin))
        t = args.regions * args.inpaint_steps * (klein_cfg["layers"] * td + klein_cfg["single_layers"] * ts)
        parts.append(f"inpaint: oracle Flux2 MMDiT blocks at full width and T={T}: 1 double {td:.2f} s + 1 single {ts:.2f} s, "
                     f"x({klein_cfg['layers']}, {klein_cfg['single_layers']}) blocks x {args.inpaint_steps} steps x {args.regions} region (VAE and host math not counted)")
        total += t; spent += td + ts
        del dbl, sgl
    elif "inpaint" in stages and inpaint_info is not None:
        from oracle import flux_ref as fr
        T = inpaint_info["tokens"]
        t_txt = 512
        w2, h2 = inpaint_info["resolution"][0] // 16, inpaint_info["resolution"][1] // 16
        torch.manual_seed(0)
        dbl, sgl = fr.DoubleBlock(3072, 24).eval(), fr.SingleBlock(3072, 24).eval()
        ids = torch.cat([torch.zeros(t_txt, 3), fr.image_ids(h2, w2, 0), fr.image_ids(h2, w2, 1)])
        cos, sin = fr.rope_tables(ids, (16, 56, 56))
        x, temb = torch.randn(T, 3072), torch.randn(3072)
        td = timed(lambda: dbl(x[t_txt:], x[:t_txt], temb, cos, sin))
        ts = timed(lambda: sgl(x, temb, cos, sin))
        t = args.regions * args.inpaint_steps * (19 * td + 38 * ts)
        parts.append(f"inpaint: oracle MMDiT blocks at full width and T={T}: 1 double {td:.2f} s + 1 single {ts:.2f} s, "
                     f"x(19, 38) blocks x {args.inpaint_steps} steps x {args.regions} region (VAE and host math not counted)")
        total += t; spent += td + ts
        del dbl, sgl
    if "upscale" in stages:
        from oracle.rcan_ref import load_ref
        ref = load_ref(rcan_sd)
        ch, cw = 256, 192
        x = torch.from_numpy(pg[:ch, :cw].copy()).permute(2, 0, 1)[None].float() / 255.0
        ref(x[:, :, :16, :16])
        t = timed(lambda: ref(x))
        frac = (ch * cw) / float(W_ * H_)
        parts.append(f"upscale: oracle RCAN on a {cw}x{ch} crop = {frac:.4f} page {t:.2f} s"); total += t / frac; spent += t
    if "clean" in stages:
        from oracle import cleaning_ref as cr
        from mangatranslator_amd.core.image import cleaning as cl
        sc = (W_ * H_ / 1e6) ** 0.5
        dk, ek = cr.ellipse_kernel(cl.scale_kernel(cl.DILATION_KERNEL_SIZE, sc)), cr.ellipse_kernel(cl.scale_kernel(cl.EROSION_KERNEL_SIZE, sc))
        x0, y0, x1, y1 = (int(v) for v in boxes[0])
        yy, xx = np.mgrid[0:H_, 0:W_]
        bm = ((((xx - (x0 + x1) / 2) / ((x1 - x0) / 2 - 4)) ** 2 + ((yy - (y0 + y1) / 2) / ((y1 - y0) / 2 - 4)) ** 2) <= 1.0).astype(np.uint8) * 255
        gray = cr.bgr_to_gray(np.ascontiguousarray(pg[..., ::-1]))
        t = timed(lambda: cr.process_single_bubble(bm, gray, 200, False, float(cl.scale_scalar(5, sc, minimum=0.0, maximum=64.0)), (x0, y0, x1, y1), dk, ek,
                                                   cl.scale_area(50, sc, minimum=50, maximum=5000), False, None, sc, np.ascontiguousarray(pg[..., ::-1])))
        parts.append(f"clean: oracle cleaning chain on 1 of {len(boxes)} bubbles {t:.2f} s"); total += t * len(boxes); spent += t
    return {"value": 1.0 / total, "unit": "pages/s", "cores": cores, "kind": "port",
            "sample": f"{spent:.1f} s of CPU work, extrapolated to {total:.0f} s/page — " + "; ".join(parts)}


if __name__ == "__main__":
    main()
