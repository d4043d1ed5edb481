"""Open Images evaluation loop timing on one GPU: BASELINE configs[3] shape (600 x 1000, N = 200, 601 object classes,
30 predicates, bs 1, fp32, graphed, seeded random weights, synthetic targets).  Prints one JSON line:
  calculate_fps_images_s      runtime.calculate_fps (forward only) on the same batches
  evaluate_oi_images_s        evaluation.evaluate(single=False, oi=True) -- forward + triplet_candidates(mode="oi") +
                              OpenImagesRelationMetrics.update per batch, compute() at the end
  update_stream_us            stream time per OpenImagesRelationMetrics.update (host GT packing + copy + the four
                              per-batch kernels), HIP events around 100 updates on fixed candidates
  compute_ms                  one compute() over those 110 images' records (record sort + oi_ap + one synchronisation)
The per-kernel times come from a rocprofv3 --kernel-trace --stats run of this tool.

    python tools/oi_eval_bench.py [--batches 200] [--warmup 5]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import bench
    from eval_loop_bench import synthetic_targets
    from egtr_amd.evaluation import OpenImagesRelationMetrics, evaluate
    from egtr_amd.runtime import GraphedForward, calculate_fps, triplet_candidates

    dev = torch.device("cuda:0")
    model, cfg, _ = bench.build_model(dev, dict(num_labels=601, num_rel_labels=30))
    C, R = cfg.num_labels, cfg.num_rel_labels
    pv = torch.randn(1, 3, bench.H_IMG, bench.W_IMG)
    pm = torch.ones(1, bench.H_IMG, bench.W_IMG, dtype=torch.long)
    targets = synthetic_targets(args.batches, C, R, seed=3)
    batches = [{"pixel_values": pv, "pixel_mask": pm, "labels": [t]} for t in targets]
    fwd = GraphedForward(model, enabled=True, strict=True)
    try:
        fwd(pv.to(dev), pm.to(dev))      # capture outside every timed region
        fps = calculate_fps(model, batches, warmup=args.warmup, forward=fwd)
        evaluate(model, batches[:args.warmup], C, R, forward=fwd, single=False, oi=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        metrics = evaluate(model, batches, C, R, forward=fwd, single=False, oi=True)   # ends with compute()
        ev_oi = len(batches) / (time.perf_counter() - t0)

        out = fwd(pv.to(dev), pm.to(dev))
        sizes = torch.tensor([[600, 1000]], device=dev)
        cands = triplet_candidates(out, C, sizes, 100, mode="oi")
        ev = OpenImagesRelationMetrics(R)
        for t in targets[:10]:
            ev.update(cands, [t])
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n = 100
        e0.record()
        for i in range(n):
            ev.update(cands, [targets[i % len(targets)]])
        e1.record()
        e1.synchronize()
        update_us = e0.elapsed_time(e1) * 1e3 / n
        t0 = time.perf_counter()
        ev.compute()
        compute_ms = (time.perf_counter() - t0) * 1e3
    finally:
        fwd.close()
    print(json.dumps({"tool": "oi_eval_bench", "shape": [1, 3, bench.H_IMG, bench.W_IMG],
                      "num_queries": cfg.num_queries, "num_labels": C, "num_rel_labels": R, "batches": len(batches),
                      "calculate_fps_images_s": round(fps, 2), "evaluate_oi_images_s": round(ev_oi, 2),
                      "oi_ratio": round(ev_oi / fps, 3), "update_stream_us": round(update_us, 1),
                      "compute_ms": round(compute_ms, 2),
                      "metrics": {k: round(v, 6) for k, v in metrics.items()},
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
