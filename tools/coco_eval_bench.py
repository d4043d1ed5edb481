"""COCO box-detection evaluation timing on one GPU: the bench model (600 x 1000, 150 object classes, bs 1, fp32,
graphed, seeded random weights, synthetic targets).  Prints one JSON line:
  calculate_fps_images_s      runtime.calculate_fps (forward only) on the same batches
  evaluate_coco_images_s      evaluation.evaluate(single=True, coco=True) -- forward + the single-predicate SGG
                              evaluator + post_process + CocoDetectionMetrics.update per batch, compute() at the end
  evaluate_single_images_s    evaluation.evaluate(single=True) on the same batches, for reference
  update_stream_us            stream time per CocoDetectionMetrics.update at bs 1 (GT packing + copy + egtr_coco_match_f32)
  post_process_update_us      stream time per post_process + update at bs 1
  compute_ms / records        one device compute() over synthetic records at the VG test scale (25k images x 100
                              detections, 150 classes): record sort + egtr_coco_accumulate_f64 + summarize + one sync
  host_compute_ms             the host path's compute() over the same records
The per-kernel times come from a rocprofv3 --kernel-trace --stats run of this tool.

    python tools/coco_eval_bench.py [--batches 200] [--warmup 5] [--images 25000]"""
import argparse
import json
import os
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def synthetic_records(ev, n_images, K, dev, seed, chunk=250):
    """Fill ``ev`` through update() with n_images images of 100 random detections and 5-25 random GTs each."""
    g = torch.Generator().manual_seed(seed)
    for i0 in range(0, n_images, chunk):
        B = min(chunk, n_images - i0)
        xy = torch.rand(B, 100, 2, generator=g) * 800
        wh = torch.rand(B, 100, 2, generator=g) * 200 + 1
        boxes = torch.cat([xy, xy + wh], -1).to(dev)
        scores = torch.rand(B, 100, generator=g).to(dev)
        labels = torch.randint(0, K + 1, (B, 100), generator=g).to(dev)
        results = [{"scores": scores[b], "labels": labels[b], "boxes": boxes[b]} for b in range(B)]
        gts = []
        for b in range(B):
            G = int(torch.randint(5, 26, (1,), generator=g))
            j = torch.randint(0, 100, (G,), generator=g)
            gb = torch.cat([xy[b, j], wh[b, j] * (0.8 + 0.4 * torch.rand(G, 2, generator=g))], -1).double()
            gts.append({"boxes": gb, "area": gb[:, 2] * gb[:, 3], "iscrowd": (torch.rand(G, generator=g) < 0.05).to(
                torch.uint8), "labels": labels[b, j].cpu().clamp(max=K - 1)})
        ev.update(results, gts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--images", type=int, default=25000)
    args = ap.parse_args()
    import bench
    from eval_loop_bench import synthetic_targets
    from egtr_amd.evaluation import CocoDetectionMetrics, coco_gt_entry, evaluate
    from egtr_amd.feature_extraction import DeformableDetrFeatureExtractor
    from egtr_amd.runtime import GraphedForward, calculate_fps

    dev = torch.device("cuda:0")
    model, cfg, _ = bench.build_model(dev)
    C, R = cfg.num_labels, cfg.num_rel_labels
    pv = torch.randn(1, 3, bench.H_IMG, bench.W_IMG)
    pm = torch.ones(1, bench.H_IMG, bench.W_IMG, dtype=torch.long)
    targets = synthetic_targets(args.batches, C, R, seed=3)
    batches = [{"pixel_values": pv, "pixel_mask": pm, "labels": [t]} for t in targets]
    fe = DeformableDetrFeatureExtractor()
    fwd = GraphedForward(model, enabled=True, strict=True)
    try:
        fwd(pv.to(dev), pm.to(dev))      # capture outside every timed region
        fps = calculate_fps(model, batches, warmup=args.warmup, forward=fwd)
        evaluate(model, batches[:args.warmup], C, R, forward=fwd, single=True, coco=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        evaluate(model, batches, C, R, forward=fwd, single=True)
        ev_single = len(batches) / (time.perf_counter() - t0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        metrics = evaluate(model, batches, C, R, forward=fwd, single=True, coco=True)   # ends with compute()
        ev_coco = len(batches) / (time.perf_counter() - t0)

        out = fwd(pv.to(dev), pm.to(dev))
        sizes = torch.tensor([[600, 1000]], device=dev)
        boxes_out = types.SimpleNamespace(logits=out["logits"], pred_boxes=out["pred_boxes"])
        res = fe.post_process(boxes_out, sizes)
        gts = [coco_gt_entry(t) for t in targets]
        ev = CocoDetectionMetrics(C)
        for t in gts[:10]:
            ev.update(res, [t])
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n = 100
        e0.record()
        for i in range(n):
            ev.update(res, [gts[i % len(gts)]])
        e1.record()
        e1.synchronize()
        update_us = e0.elapsed_time(e1) * 1e3 / n
        e0.record()
        for i in range(n):
            ev.update(fe.post_process(boxes_out, sizes), [gts[i % len(gts)]])
        e1.record()
        e1.synchronize()
        pp_update_us = e0.elapsed_time(e1) * 1e3 / n
    finally:
        fwd.close()

    big = CocoDetectionMetrics(C)
    synthetic_records(big, args.images, C, dev, seed=7)
    big.compute()                        # warm the sort and the kernel
    big._result = None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    big_stats = big.compute()
    compute_ms = (time.perf_counter() - t0) * 1e3
    records = int(sum(b[0].numel() for b in big._batches))
    host = CocoDetectionMetrics(C)
    host.npig = big.npig.cpu()
    host._batches = [tuple(x.cpu() for x in b) for b in big._batches]
    host._n_images = big.n_images
    t0 = time.perf_counter()
    host_stats = host.compute()
    host_ms = (time.perf_counter() - t0) * 1e3
    assert torch.equal(host.precision, big.precision.cpu()) and torch.equal(host.recall, big.recall.cpu())
    print(json.dumps({"tool": "coco_eval_bench", "shape": [1, 3, bench.H_IMG, bench.W_IMG],
                      "num_queries": cfg.num_queries, "num_labels": C, "batches": len(batches),
                      "calculate_fps_images_s": round(fps, 2), "evaluate_coco_images_s": round(ev_coco, 2),
                      "evaluate_single_images_s": round(ev_single, 2), "coco_ratio": round(ev_coco / fps, 3),
                      "update_stream_us": round(update_us, 1), "post_process_update_us": round(pp_update_us, 1),
                      "records": records, "compute_ms": round(compute_ms, 2), "host_compute_ms": round(host_ms, 1),
                      "AP50": round(metrics["AP50"], 6),
                      "synthetic_stats_max_abs_diff": max(abs(big_stats[k] - host_stats[k]) for k in big_stats),
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
