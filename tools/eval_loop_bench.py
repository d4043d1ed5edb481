"""Evaluation loop timing on one GPU: VG inference shape (600 x 1000, N = 200, 50 predicates, bs 1, fp32, graphed, seeded
random weights, synthetic targets).  Prints one JSON line:
  calculate_fps_images_s      runtime.calculate_fps (forward only)
  evaluate_single_images_s    evaluation.evaluate(single=True) -- forward + triplet_candidates + R@K / mR@K
  evaluate_both_images_s      evaluation.evaluate(single=True, multiple=True)
  sgg_eval_kernels_us         device time per batch (bs 1) of the two sgg_eval kernels (match + fold), HIP events around
                              100 back-to-back launches on staged inputs (an upper bound: launch-issue bound)
  update_stream_us            stream time per SceneGraphRecall.update (host packing + GT copy + kernels), HIP events
                              around 100 updates on fixed candidates

    python tools/eval_loop_bench.py [--batches 200] [--warmup 5]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic_targets(n, C, R, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        G = int(torch.randint(10, 25, (1,), generator=g))
        boxes = torch.cat([torch.rand(G, 2, generator=g) * 0.6 + 0.2, torch.rand(G, 2, generator=g) * 0.2 + 0.05], 1)
        rel = torch.zeros(G, G, R)
        T = int(torch.randint(5, 21, (1,), generator=g))
        idx = torch.randint(0, G, (T, 2), generator=g)
        rel[idx[:, 0], idx[:, 1], torch.randint(0, R, (T,), generator=g)] = 1
        out.append({"class_labels": torch.randint(0, C, (G,), generator=g), "boxes": boxes, "rel": rel,
                    "orig_size": torch.tensor([600, 1000])})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import bench
    from egtr_amd.evaluation import SceneGraphRecall, evaluate
    from egtr_amd.runtime import GraphedForward, calculate_fps, triplet_candidates

    dev = torch.device("cuda:0")
    model, cfg, _ = bench.build_model(dev)
    C, R = cfg.num_labels, cfg.num_rel_labels
    pv = torch.randn(1, 3, bench.H_IMG, bench.W_IMG)
    pm = torch.ones(1, bench.H_IMG, bench.W_IMG, dtype=torch.long)
    targets = synthetic_targets(args.batches, C, R, seed=3)
    batches = [{"pixel_values": pv, "pixel_mask": pm, "labels": [t]} for t in targets]
    fwd = GraphedForward(model, enabled=True, strict=True)
    try:
        fwd(pv.to(dev), pm.to(dev))      # capture outside every timed region
        fps = calculate_fps(model, batches, warmup=args.warmup, forward=fwd)

        def timed_eval(**kw):
            evaluate(model, batches[:args.warmup], C, R, forward=fwd, **kw)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            evaluate(model, batches, C, R, forward=fwd, **kw)     # ends with compute(): one synchronisation
            return len(batches) / (time.perf_counter() - t0)

        ev_single = timed_eval(single=True, multiple=False)
        ev_both = timed_eval(single=True, multiple=True)

        out = fwd(pv.to(dev), pm.to(dev))
        sizes = torch.tensor([[600, 1000]], device=dev)
        res, kern = {}, {}
        for mode in ("single", "multiple"):
            cands = triplet_candidates(out, C, sizes, 100, mode=mode)
            ev = SceneGraphRecall(R, multiple_preds=(mode == "multiple"))
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
            res[mode] = e0.elapsed_time(e1) * 1e3 / n
            torch.cuda.synchronize()
            e0.record()
            for i in range(n):
                ev._launch(ev.acc)
            e1.record()
            e1.synchronize()
            kern[mode] = e0.elapsed_time(e1) * 1e3 / n
    finally:
        fwd.close()
    print(json.dumps({"tool": "eval_loop_bench", "shape": [1, 3, bench.H_IMG, bench.W_IMG], "num_queries": cfg.num_queries,
                      "num_rel_labels": R, "batches": len(batches), "calculate_fps_images_s": round(fps, 2),
                      "evaluate_single_images_s": round(ev_single, 2), "evaluate_both_images_s": round(ev_both, 2),
                      "single_ratio": round(ev_single / fps, 3), "both_ratio": round(ev_both / fps, 3),
                      "sgg_eval_kernels_us": {k: round(v, 1) for k, v in kern.items()},
                      "update_stream_us": {k: round(v, 1) for k, v in res.items()},
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
