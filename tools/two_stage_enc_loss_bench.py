#!/usr/bin/env python
"""A/B of the two-stage variant's ``*_enc`` loss terms (labels + cardinality + boxes of the per-token proposal set against the
class-agnostic targets): the tensor composition -- what the parent of this change does for the proposal set, and what is still
done outside the large entry's domain -- against the one-pass route (egtr_detection_loss_large_f32, csrc/loss.hip).

    python tools/two_stage_enc_loss_bench.py [--rounds 3] [--iters 20] [--train-steps 8] > profiles/two_stage_enc_loss_ab.txt

Every measurement runs in a FRESH process and the two routes alternate (composition, kernel, composition, kernel, ...), so
drift of the shared host lands on both.  ``--route composition`` takes the route decision away (``ops.detection_loss_large_route``
answers False); the code that then runs -- ``get_loss`` per term on the zero-label copies of the targets -- is the parent's,
line for line.

  terms     the ``*_enc`` terms alone on device-matched indices (the matcher runs once, outside the timed region): forward,
            the weighted total, backward to the logits and boxes, ending in a device synchronise (median wall time over
            --iters calls after 3 warm-up calls); peak memory held by the term (``torch.cuda.max_memory_allocated`` over the
            call minus what was allocated before it); the kernel route also reports its two launches by HIP events
  train     ms per bs-4 two-stage train step at 600x1000 through DataParallelTrainer (ResNet-50, 6 enc / 6 dec, N = 200,
            proposals = every encoder token), mean over --train-steps steps after 3 warm-up steps

Settings (targets per image: fixed lists):  600x1000  B = 4  S = 12 537  T = 26/13/13/18;  800x1333  B = 16  S = 22 223
T = 5 .. 93.  C = 150.  Traffic floor of the arithmetic (one read of the logits, one write of their gradient) at 8 TB/s:
7.5 us and 53 us.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETTINGS = {"600x1000": dict(B=4, S=12537, T=[26, 13, 13, 18]),
            "800x1333": dict(B=16, S=22223, T=[5, 93, 11, 40, 26, 13, 62, 18, 7, 33, 50, 21, 9, 77, 15, 29])}
C = 150
WEIGHTS = {"loss_ce": 2.0, "loss_bbox": 5.0, "loss_giou": 2.0}
HBM_BYTES_PER_S = 8e12


def force_composition():
    from egtr_amd import ops
    from egtr_amd.kernels import heads
    heads.detection_loss_large_route = ops.detection_loss_large_route = lambda num_query: False


def term_inputs(setting, dev):
    import numpy as np
    import torch
    s = SETTINGS[setting]
    rng = np.random.RandomState(12 + s["S"])
    g = torch.Generator().manual_seed(s["S"])
    B, S = s["B"], s["S"]
    logits = (torch.randn(B, S, C, generator=g) * 2 - 3).to(dev)
    boxes = torch.cat([torch.rand(B, S, 2, generator=g) * 0.8 + 0.1, torch.rand(B, S, 2, generator=g) * 0.4 + 0.02], -1).to(dev)
    targets = []
    for T in s["T"]:
        bx = np.concatenate([rng.uniform(0.2, 0.8, (T, 2)), rng.uniform(0.05, 0.25, (T, 2))], 1).astype(np.float32)
        targets.append({"class_labels": torch.from_numpy(rng.randint(0, C, T)).to(dev), "boxes": torch.from_numpy(bx).to(dev)})
    return logits, boxes, targets


def child_terms(args):
    import torch
    from egtr_amd import _lib, ops
    from egtr_amd.deformable_detr import DeformableDetrHungarianMatcher
    from egtr_amd.egtr import SceneGraphGenerationLoss
    if not torch.cuda.is_available():
        raise SystemExit("two_stage_enc_loss_bench: no GPU -- nothing is measured without one")
    dev = "cuda:0"
    if args.route == "composition":
        force_composition()
    logits, boxes, targets = term_inputs(args.setting, dev)
    m = DeformableDetrHungarianMatcher(class_cost=2.0, bbox_cost=5.0, giou_cost=2.0, smoothing=1e-14)
    crit = SceneGraphGenerationLoss(
        matcher=m, num_object_queries=200, num_classes=C, num_rel_labels=50, eos_coef=0.1,
        losses=["labels", "boxes", "cardinality"], smoothing=1e-14, rel_sample_negatives=80, rel_sample_nonmatching=80,
        model_training=True, focal_alpha=0.25, rel_sample_negatives_largest=True, rel_sample_nonmatching_largest=True).to(dev)
    num_boxes = float(sum(len(t["class_labels"]) for t in targets))
    bin_targets = [dict(t, class_labels=torch.zeros_like(t["class_labels"])) for t in targets]
    lg, bx = logits.requires_grad_(True), boxes.requires_grad_(True)
    enc = {"logits": lg, "pred_boxes": bx}
    indices, costs = m(enc, bin_targets)
    packed = ops.pack_detection_targets(targets, dev)      # the step's own: built for the main output set in any case
    m.raise_if_invalid()
    events = []
    real_launch = _lib.launch

    def launch(name, *a, **k):          # HIP events around the entry's two launches
        if name != "egtr_detection_loss_large_f32":
            return real_launch(name, *a, **k)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        real_launch(name, *a, **k)
        e1.record()
        events.append((e0, e1))
    _lib.launch = launch

    def terms():
        if ops.detection_loss_large_route(lg.shape[1]):
            return ops.detection_losses_large(lg, bx, indices.flat, packed, 0.25, num_boxes, class_agnostic=True)
        d = {}
        for loss in ("labels", "boxes", "cardinality"):
            d.update(crit.get_loss(loss, enc, bin_targets, indices, costs, num_boxes))
        return d

    wall, peak = [], []
    for it in range(3 + args.iters):
        lg.grad = bx.grad = None
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        d = terms()
        sum(d[k] * w for k, w in WEIGHTS.items()).backward()
        torch.cuda.synchronize()
        if it >= 3:
            wall.append((time.perf_counter() - t0) * 1e3)
            peak.append(torch.cuda.max_memory_allocated() - before)
    assert bool(events) == (args.route == "kernel"), (len(events), args.route)
    kern = [a.elapsed_time(b) for a, b in events[3:]]
    res = {"kind": "terms", "setting": args.setting, "route": args.route,
           "wall_ms": round(statistics.median(wall), 3), "wall_ms_min": round(min(wall), 3),
           "kernel_ms": round(statistics.median(kern), 4) if kern else None,
           "peak_mb": round(max(peak) / 2 ** 20, 1),
           "terms": {k: float(d[k]) for k in sorted(d)},
           "grad_logits_abs_sum": float(lg.grad.abs().sum()), "grad_boxes_abs_sum": float(bx.grad.abs().sum())}
    print(json.dumps(res))


def child_train(args):
    import numpy as np
    import torch
    import bench
    from egtr_amd.deformable_detr import DeformableDetrConfig
    from egtr_amd.egtr import DetrForSceneGraphGeneration
    from egtr_amd.runtime import DataParallelTrainer, configure_optimizers
    if not torch.cuda.is_available():
        raise SystemExit("two_stage_enc_loss_bench: no GPU -- nothing is measured without one")
    dev = torch.device("cuda:0")
    if args.route == "composition":
        force_composition()
    c = dict(bench.CFG)
    c.update(dropout=0.1, two_stage=True, with_box_refine=True, two_stage_num_proposals=bench.CFG["num_queries"])
    base = ("num_queries", "encoder_layers", "decoder_layers", "dropout", "auxiliary_loss", "two_stage", "with_box_refine",
            "two_stage_num_proposals")
    cfg = DeformableDetrConfig(**{k: c[k] for k in base})
    for k, v in c.items():
        if k not in base:
            setattr(cfg, k, v)
    fg = np.random.RandomState(0).randint(0, 5, (cfg.num_labels + 1, cfg.num_labels + 1, cfg.num_rel_labels))
    torch.manual_seed(0)
    model = DetrForSceneGraphGeneration(cfg, fg_matrix=fg.astype(np.float64)).to(dev).train()
    opt = configure_optimizers(model, lr=2e-6, lr_backbone=2e-7, lr_initialized=None, weight_decay=1e-4)
    tr = DataParallelTrainer(model, optimizer=opt, accumulate=1, clip=0.1)
    torch.manual_seed(100)
    b = {"pixel_values": torch.randn(4, 3, bench.H_IMG, bench.W_IMG, device=dev),
         "pixel_mask": torch.ones(4, bench.H_IMG, bench.W_IMG, dtype=torch.long, device=dev),
         "labels": bench.make_targets(4, cfg, dev, 7)}
    for _ in range(3):
        tr.training_step(b)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.train_steps):
        loss, loss_dict, _ = tr.training_step(b)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / args.train_steps
    tr.finalize()
    print(json.dumps({"kind": "train", "setting": "600x1000", "route": args.route, "ms_per_step": round(ms, 3),
                      "loss": float(loss), "enc_terms": {k: float(v) for k, v in sorted(loss_dict.items()) if k.endswith("_enc")}}))


def run_child(kind, route, setting, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, "--route", route, "--setting", setting,
           "--iters", str(args.iters), "--train-steps", str(args.train_steps)]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.child_timeout)
    except subprocess.TimeoutExpired:
        return {"kind": kind, "setting": setting, "route": route, "failed": f"no result within {args.child_timeout} s"}, True
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not lines:
        tail = (p.stderr.strip().splitlines() or ["?"])[-1]
        return {"kind": kind, "setting": setting, "route": route, "failed": f"exit {p.returncode}: {tail}"}, True
    return json.loads(lines[-1]), False


def spread(v):
    return f"{statistics.median(v):.3f} (rounds {min(v):.3f} .. {max(v):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--train-steps", type=int, default=8)
    ap.add_argument("--no-train", action="store_true")
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--child", choices=["terms", "train"])
    ap.add_argument("--route", choices=["composition", "kernel"], default="kernel")
    ap.add_argument("--setting", choices=sorted(SETTINGS), default="600x1000")
    args = ap.parse_args()
    if args.child == "terms":
        return child_terms(args)
    if args.child == "train":
        return child_train(args)
    print("# two-stage *_enc loss terms: the tensor composition (the parent's code) against egtr_detection_loss_large_f32, "
          "alternating fresh processes")
    print(f"# rounds {args.rounds}, calls per process {args.iters}, train steps per process {args.train_steps}")
    jobs = [("terms", s) for s in sorted(SETTINGS)] + ([] if args.no_train else [("train", "600x1000")])
    for kind, setting in jobs:
        rows = {"composition": [], "kernel": []}
        for rnd in range(args.rounds):
            for route in ("composition", "kernel"):
                res, stop = run_child(kind, route, setting, args)
                print(json.dumps(res), flush=True)
                if stop:      # a child that failed, was killed or timed out: nothing more is started on the device
                    print("# stopped: a measurement process did not end normally")
                    return 1
                rows[route].append(res)
        key = "wall_ms" if kind == "terms" else "ms_per_step"
        comp, kern = [r[key] for r in rows["composition"]], [r[key] for r in rows["kernel"]]
        line = f"# {kind} {setting}: composition {spread(comp)} ms, kernel {spread(kern)} ms"
        if kind == "terms":
            s = SETTINGS[setting]
            floor_us = 2 * 4 * s["B"] * s["S"] * C / HBM_BYTES_PER_S * 1e6
            k = [r["kernel_ms"] for r in rows["kernel"]]
            line += (f"; the entry's two launches by HIP events {spread(k)} ms = {floor_us / (statistics.median(k) * 1e3):.0%} of "
                     f"the HBM roofline (derived floor {floor_us:.1f} us at 8 TB/s); peak memory held by the term: composition "
                     f"{max(r['peak_mb'] for r in rows['composition'])} MB, kernel {max(r['peak_mb'] for r in rows['kernel'])} MB")
        print(line, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
