"""Reference-exact preprocessing timing on one GPU (DeformableDetrDeviceFeatureExtractor, csrc/preprocess.hip).
Prints one JSON line; per shape ("eval": 450 x 750 uint8 -> 600 x 1000 at size 600 / max_size 1000, the bench model's
input; "vg": 375 x 500 -> 800 x 1066 at 800 / 1333):
  host_images_s          the reference's host path in this process: PIL BILINEAR resize + the 4.18 float32 rescale /
                         normalise in numpy + the collate's pad, one image at a time
  device_images_s_bs{1,8}  the extractor from uint8 numpy images (pinned staging + one H2D copy + the launch), device
                         events around --iters batches after warm-up
  launch_us_bs{1,8}      stream time per launch of a prepared batch (events around back-to-back launches)
  roofline_us_bs{1,8}    algorithmic bytes (uint8 in, fp32 out, int64 mask) / HBM_PEAK_GBS; roofline_fraction =
                         roofline_us / launch_us
and, at the eval shape:
  calculate_fps_images_s / evaluate_fp32_images_s / evaluate_uint8_images_s: runtime.calculate_fps, and
                         evaluation.evaluate(single=True) fed the pre-made fp32 tensors of tools/eval_loop_bench.py or
                         uint8 images through the extractor (one call per batch, bs 1)
The per-kernel times come from a rocprofv3 --kernel-trace --stats run of this tool (--no-model keeps that run short).

    python tools/preprocess_bench.py [--iters 50] [--batches 200] [--warmup 5] [--no-model]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_PEAK_GBS = 8000.0
SHAPES = {"eval": ((450, 750), 600, 1000), "vg": ((375, 500), 800, 1333)}


def images(shape, n, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, shape + (3,), dtype=np.uint8) for _ in range(n)]


def host_reference(imgs, size, max_size):
    """The reference's per-image path (PIL + numpy, float32) and the host pad, images per second."""
    from PIL import Image
    from egtr_amd.feature_extraction import _target_size
    mean = np.array((0.485, 0.456, 0.406)).astype(np.float32)[:, None, None]
    std = np.array((0.229, 0.224, 0.225)).astype(np.float32)[:, None, None]
    t0 = time.perf_counter()
    outs = []
    for a in imgs:
        oh, ow = _target_size(a.shape[0], a.shape[1], size, max_size)
        v = np.array(Image.fromarray(a).resize((ow, oh), Image.BILINEAR)).astype(np.float32) * (1 / 255.0)
        outs.append((v.transpose(2, 0, 1) - mean) / std)
    H, W = max(o.shape[1] for o in outs), max(o.shape[2] for o in outs)
    pv = np.zeros((len(outs), 3, H, W), np.float32)
    pm = np.zeros((len(outs), H, W), np.int64)
    for i, o in enumerate(outs):
        pv[i, :, :o.shape[1], :o.shape[2]] = o
        pm[i, :o.shape[1], :o.shape[2]] = 1
    return len(imgs) / (time.perf_counter() - t0)


def event_time(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters      # us per call


def shape_bench(name, iters, dev):
    from egtr_amd.feature_extraction import DeformableDetrDeviceFeatureExtractor
    shape, size, max_size = SHAPES[name]
    fe = DeformableDetrDeviceFeatureExtractor(size=size, max_size=max_size)
    pool = images(shape, 16, seed=1)
    out = {"host_images_s": round(host_reference(pool[:8], size, max_size), 2)}
    for bs in (1, 8):
        k = [0]

        def call():
            k[0] = (k[0] + 1) % (len(pool) // bs)
            fe(pool[k[0] * bs:(k[0] + 1) * bs], device=dev)
        us = event_time(call, iters)
        batch = fe.prepare(pool[:bs], dev)
        enc = batch.run()
        pv, pm = enc["pixel_values"], enc["pixel_mask"]
        launch = event_time(lambda: batch.run(pv, pm), iters * 4)
        nbytes = sum(a.size for a in pool[:bs]) + pv.numel() * 4 + pm.numel() * 8
        roof = nbytes / (HBM_PEAK_GBS * 1e9) * 1e6
        out.update({f"device_images_s_bs{bs}": round(bs * 1e6 / us, 1), f"launch_us_bs{bs}": round(launch, 2),
                    f"roofline_us_bs{bs}": round(roof, 2), f"roofline_fraction_bs{bs}": round(roof / launch, 3),
                    f"bytes_bs{bs}": int(nbytes)})
    out["out_shape"] = list(pv.shape[-2:])
    return out


def model_bench(args, dev):
    import bench
    from eval_loop_bench import synthetic_targets
    from egtr_amd.evaluation import evaluate
    from egtr_amd.feature_extraction import DeformableDetrDeviceFeatureExtractor
    from egtr_amd.runtime import GraphedForward, calculate_fps

    model, cfg, _ = bench.build_model(dev)
    C, R = cfg.num_labels, cfg.num_rel_labels
    pv = torch.randn(1, 3, bench.H_IMG, bench.W_IMG)
    pm = torch.ones(1, bench.H_IMG, bench.W_IMG, dtype=torch.long)
    targets = synthetic_targets(args.batches, C, R, seed=3)
    batches = [{"pixel_values": pv, "pixel_mask": pm, "labels": [t]} for t in targets]
    shape, size, max_size = SHAPES["eval"]
    fe = DeformableDetrDeviceFeatureExtractor(size=size, max_size=max_size)
    pool = images(shape, 16, seed=2)
    assert fe.output_size(*shape) == (bench.H_IMG, bench.W_IMG)

    def uint8_batches(n):
        for i, t in enumerate(targets[:n]):
            enc = fe([pool[i % len(pool)]], device=dev)
            yield {"pixel_values": enc["pixel_values"], "pixel_mask": enc["pixel_mask"], "labels": [t]}

    fwd = GraphedForward(model, enabled=True, strict=True)
    try:
        fwd(pv.to(dev), pm.to(dev))      # capture outside every timed region
        fps = calculate_fps(model, batches, warmup=args.warmup, forward=fwd)

        def timed(feed):
            evaluate(model, feed(args.warmup), C, R, forward=fwd, single=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            evaluate(model, feed(len(batches)), C, R, forward=fwd, single=True)
            return len(batches) / (time.perf_counter() - t0)
        ev_f32 = timed(lambda n: batches[:n])
        ev_u8 = timed(uint8_batches)
        ev_f32_again = timed(lambda n: batches[:n])
    finally:
        fwd.close()
    return {"calculate_fps_images_s": round(fps, 2), "evaluate_fp32_images_s": round(ev_f32, 2),
            "evaluate_fp32_again_images_s": round(ev_f32_again, 2), "evaluate_uint8_images_s": round(ev_u8, 2),
            "uint8_vs_fp32": round(ev_u8 / max(ev_f32, ev_f32_again), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-model", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("preprocess_bench needs a GPU")
    dev = torch.device("cuda:0")
    res = {"tool": "preprocess_bench", "hbm_peak_gbs": HBM_PEAK_GBS}
    for name in SHAPES:
        res[name] = shape_bench(name, args.iters, dev)
    if not args.no_model:
        res.update(model_bench(args, dev))
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
