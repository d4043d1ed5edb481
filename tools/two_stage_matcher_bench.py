#!/usr/bin/env python
"""A/B of the two-stage variant's proposal matcher: the host route (cost matrix on the device, copy, scipy per image --
what the parent of this change does for every query set beyond 1024, and what is still done outside the large kernel's
domain) against the device route (egtr_hungarian_match_large_f32, csrc/matcher.hip).

    python tools/two_stage_matcher_bench.py [--rounds 3] [--iters 20] [--train-steps 8] > profiles/two_stage_matcher_ab.txt
    python tools/two_stage_matcher_bench.py --referee >> profiles/two_stage_matcher_ab.txt

Every measurement runs in a FRESH process and the two routes alternate (host, device, host, device, ...), so drift of
the shared host lands on both.  ``--route host`` takes the route decision away from the large kernel
(``ops.hungarian_match_route`` answers None where it would answer "large"); the code that then runs -- the else-branch of
``DeformableDetrHungarianMatcher.prepare`` and the scipy loop of ``finish`` -- is the parent's, line for line.

  matcher   wall time of one ``matcher(outputs, targets)`` call per batch, ending in a device synchronise (median over
            --iters calls after 3 warm-up calls); the device route also reports the launch's own time by HIP events
  train     ms per bs-4 two-stage train step at 600x1000 through DataParallelTrainer (ResNet-50, 6 enc / 6 dec, N = 200,
            proposals = every encoder token), mean over --train-steps steps after 3 warm-up steps

Settings (targets per image: a seeded draw):  600x1000  B = 4  N = 12 537  T in 5..40;  800x1333  B = 16  N = 22 223
T in 5..100.  The logits have one column per class (150); the class-agnostic targets read column 0, as in the criterion.
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

SETTINGS = {"600x1000": dict(B=4, N=12537, tmin=5, tmax=40), "800x1333": dict(B=16, N=22223, tmin=5, tmax=100)}


def force_host_route():
    from egtr_amd import ops
    from egtr_amd.kernels import heads
    real = heads.hungarian_match_route

    def route(num_query, max_targets):
        r = real(num_query, max_targets)
        return None if r == "large" else r
    heads.hungarian_match_route = ops.hungarian_match_route = route


def matcher_inputs(setting, dev):
    import numpy as np
    import torch
    s = SETTINGS[setting]
    rng = np.random.RandomState(12 + s["N"])
    g = torch.Generator().manual_seed(s["N"])
    B, N, K = s["B"], s["N"], 150
    logits = (torch.randn(B, N, K, generator=g) * 2 - 3).to(dev)
    boxes = torch.cat([torch.rand(B, N, 2, generator=g) * 0.8 + 0.1, torch.rand(B, N, 2, generator=g) * 0.4 + 0.02], -1).to(dev)
    targets = []
    for _ in range(B):
        T = int(rng.randint(s["tmin"], s["tmax"] + 1))
        bx = np.concatenate([rng.uniform(0.2, 0.8, (T, 2)), rng.uniform(0.05, 0.25, (T, 2))], 1).astype(np.float32)
        targets.append({"class_labels": torch.zeros(T, dtype=torch.int64, device=dev), "boxes": torch.from_numpy(bx).to(dev)})
    return {"logits": logits, "pred_boxes": boxes}, targets


def child_matcher(args):
    import torch
    from egtr_amd import _lib
    from egtr_amd.deformable_detr import DeformableDetrHungarianMatcher
    if not torch.cuda.is_available():
        raise SystemExit("two_stage_matcher_bench: no GPU -- nothing is measured without one")
    dev = "cuda:0"
    if args.route == "host":
        force_host_route()
    out, targets = matcher_inputs(args.setting, dev)
    m = DeformableDetrHungarianMatcher(class_cost=2.0, bbox_cost=5.0, giou_cost=2.0, smoothing=1e-14)
    events = []
    real_launch = _lib.launch

    def launch(name, *a, **k):          # HIP events around the matcher's own launch
        if name != "egtr_hungarian_match_large_f32":
            return real_launch(name, *a, **k)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        real_launch(name, *a, **k)
        e1.record()
        events.append((e0, e1))
    _lib.launch = launch
    wall = []
    for it in range(3 + args.iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pending = m.prepare(out, targets)
        idx, costs = m.finish(pending)
        torch.cuda.synchronize()
        if it >= 3:
            wall.append((time.perf_counter() - t0) * 1e3)
    assert pending[0] == args.route, (pending[0], args.route)
    m.raise_if_invalid()
    kern = [a.elapsed_time(b) for a, b in events[3:]]
    checksum = int(sum(int(a.sum()) for a, _ in idx))
    res = {"kind": "matcher", "setting": args.setting, "route": args.route,
           "wall_ms": round(statistics.median(wall), 3), "wall_ms_min": round(min(wall), 3),
           "kernel_ms": round(statistics.median(kern), 3) if kern else None,
           "targets": [int(t["boxes"].shape[0]) for t in targets], "index_sum": checksum}
    if args.route == "device":
        res.update(device_result_checks(m, out, targets, idx))
    print(json.dumps(res))


def device_result_checks(m, out, targets, idx):
    """Outside the timed region: (a) scipy on the DEVICE's own cost blocks must give the kernel's indices, image for image;
    (b) against the host route's tensor composition of the same costs (another evaluation of exp / log, so near-ties may
    fall the other way at these sizes): how far the two cost matrices are apart, how many images differ in an index, and
    how much dearer the host's assignment is than the device's ON THE DEVICE'S MATRIX (float64 sums; never negative if
    the device's assignment is optimal there)."""
    import numpy as np
    from scipy.optimize import linear_sum_assignment as sp
    from egtr_amd import ops
    cm, iss = m._smoothing_scalars()
    pi, ti, mc, n_out, blocks = ops.hungarian_match(out["logits"], out["pred_boxes"], targets, m.class_cost, m.bbox_cost,
                                                    m.giou_cost, float(cm), float(iss), want_cost=True)
    blocks = [b.cpu().numpy() for b in blocks]
    pi, ti = pi.cpu().numpy(), ti.cpu().numpy()
    equal, o = 0, 0
    for blk, n, (a, b) in zip(blocks, n_out, idx):
        sa, sb = sp(blk)
        equal += int(np.array_equal(pi[o:o + n], sa) and np.array_equal(ti[o:o + n], sb)
                     and np.array_equal(a.cpu().numpy(), sa) and np.array_equal(b.cpu().numpy(), sb))
        o += n
    force_host_route()
    pending = m.prepare(out, targets)
    assert pending[0] == "host"
    hidx, _ = m.finish(pending)
    differ, excess, apart = 0, 0.0, 0.0
    for i, (blk, (a, b), (ha, hb)) in enumerate(zip(blocks, idx, hidx)):
        host_blk = (pending[1][i].split(pending[2], -1)[i] - cm + iss).numpy()
        apart = max(apart, float(np.abs(host_blk - blk).max()))
        a, b, ha, hb = a.cpu().numpy(), b.cpu().numpy(), ha.numpy(), hb.numpy()
        if not (np.array_equal(a, ha) and np.array_equal(b, hb)):
            differ += 1
            excess = max(excess, float(blk[ha, hb].astype(np.float64).sum() - blk[a, b].astype(np.float64).sum()))
    return {"scipy_on_device_costs_equal": f"{equal}/{len(blocks)}", "images_differing_from_host_composition": differ,
            "max_cost_difference_vs_host_composition": apart, "host_assignment_excess_on_device_costs": excess}


def referee(args):
    """``--referee``: where the device's cost blocks and the host route's composition disagree, which one is right?  The
    referee is the same composition on CPU tensors, one image at a time (the reference's own path at a size every test
    covers).  Prints, per setting, the largest distance of (a) the kernel's blocks, (b) the host route's batch-wide
    composition on the device, (c) the same composition on the device for one image at a time, from the referee, and
    (d) ``torch.cdist(p=1)`` of the whole batch from the broadcast |a - b| sum on the same device tensors."""
    import torch
    from egtr_amd import ops
    from egtr_amd.deformable_detr import DeformableDetrHungarianMatcher
    if not torch.cuda.is_available():
        raise SystemExit("two_stage_matcher_bench: no GPU -- nothing is measured without one")
    m = DeformableDetrHungarianMatcher(class_cost=2.0, bbox_cost=5.0, giou_cost=2.0, smoothing=1e-14)
    cm, iss = m._smoothing_scalars()
    real = ops.hungarian_match_route
    print("# referee: the tensor composition on CPU tensors, one image at a time; largest |difference| over all images")
    for setting in sorted(SETTINGS):
        out, targets = matcher_inputs(setting, "cuda:0")
        blocks = ops.hungarian_match(out["logits"], out["pred_boxes"], targets, 2.0, 5.0, 2.0, float(cm), float(iss),
                                     want_cost=True)[4]
        force_host_route()
        pend = m.prepare(out, targets)
        worst = [0.0, 0.0, 0.0]
        for i, t in enumerate(targets):
            ref = m.prepare({"logits": out["logits"][i:i + 1].cpu(), "pred_boxes": out["pred_boxes"][i:i + 1].cpu()},
                            [{k: v.cpu() for k, v in t.items()}])[1][0]
            one = m.prepare({"logits": out["logits"][i:i + 1], "pred_boxes": out["pred_boxes"][i:i + 1]}, [t])[1][0]
            got = (blocks[i].cpu() - iss + cm, pend[1][i].split(pend[2], -1)[i], one)
            worst = [max(w, float((g - ref).abs().max())) for w, g in zip(worst, got)]
        from egtr_amd.kernels import heads
        heads.hungarian_match_route = ops.hungarian_match_route = real
        ob, tb = out["pred_boxes"].flatten(0, 1), torch.cat([t["boxes"] for t in targets])
        cd = float((torch.cdist(ob, tb, p=1) - (ob[:, None, :] - tb[None, :, :]).abs().sum(-1)).abs().max())
        print(f"# referee {setting} (B = {len(targets)}, {ob.shape[0]} x {tb.shape[0]} pairs): device kernel {worst[0]:.2e}, "
              f"host route on the batch {worst[1]:.2e}, host route image by image {worst[2]:.2e}; "
              f"torch.cdist(p=1) of the batch against the broadcast sum {cd:.2e}", flush=True)
    return 0


def child_train(args):
    import numpy as np
    import torch
    import bench
    from egtr_amd.deformable_detr import DeformableDetrConfig
    from egtr_amd.egtr import DetrForSceneGraphGeneration
    from egtr_amd.runtime import DataParallelTrainer, configure_optimizers
    if not torch.cuda.is_available():
        raise SystemExit("two_stage_matcher_bench: no GPU -- nothing is measured without one")
    dev = torch.device("cuda:0")
    if args.route == "host":
        force_host_route()
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
                      "loss": float(loss), "enc_terms": sorted(k for k in loss_dict if k.endswith("_enc"))}))


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
        return {"kind": kind, "setting": setting, "route": route, "failed": f"exit {p.returncode}: {tail}"}, p.returncode < 0
    return json.loads(lines[-1]), False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--train-steps", type=int, default=8)
    ap.add_argument("--no-train", action="store_true")
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--child", choices=["matcher", "train"])
    ap.add_argument("--route", choices=["host", "device"], default="device")
    ap.add_argument("--setting", choices=sorted(SETTINGS), default="600x1000")
    ap.add_argument("--referee", action="store_true", help="only: which cost matrix is right where the two routes disagree")
    args = ap.parse_args()
    if args.referee:
        return referee(args)
    if args.child == "matcher":
        return child_matcher(args)
    if args.child == "train":
        return child_train(args)
    print("# two-stage proposal matcher: host route (the parent's code) against the device route, alternating fresh processes")
    print(f"# rounds {args.rounds}, matcher calls per process {args.iters}, train steps per process {args.train_steps}")
    jobs = [("matcher", s) for s in sorted(SETTINGS)] + ([] if args.no_train else [("train", "600x1000")])
    for kind, setting in jobs:
        rows = {"host": [], "device": []}
        for rnd in range(args.rounds):
            for route in ("host", "device"):
                res, stop = run_child(kind, route, setting, args)
                print(json.dumps(res), flush=True)
                if stop:      # a child that was killed or timed out: nothing more is started on the device
                    print("# stopped: a measurement process did not end normally")
                    return 1
                if "failed" not in res:
                    rows[route].append(res)
        key = "wall_ms" if kind == "matcher" else "ms_per_step"
        if rows["host"] and rows["device"]:
            h, d = [r[key] for r in rows["host"]], [r[key] for r in rows["device"]]
            line = (f"# {kind} {setting}: host {statistics.median(h):.3f} ms (rounds {min(h):.3f} .. {max(h):.3f}), "
                    f"device {statistics.median(d):.3f} ms (rounds {min(d):.3f} .. {max(d):.3f})")
            if kind == "matcher":
                k = [r["kernel_ms"] for r in rows["device"] if r["kernel_ms"] is not None]
                same = {r["index_sum"] for r in rows["host"]} == {r["index_sum"] for r in rows["device"]}
                last = rows["device"][-1]
                line += (f", launch by HIP events {statistics.median(k):.3f} ms; scipy on the device's own costs gives the "
                         f"kernel's indices in {last['scipy_on_device_costs_equal']} images; index sum equal to the host "
                         f"composition's: {same} ({last['images_differing_from_host_composition']} images differ, the two cost "
                         f"evaluations are {last['max_cost_difference_vs_host_composition']:.2e} apart, the host's assignment "
                         f"is {last['host_assignment_excess_on_device_costs']:.2e} dearer on the device's costs)")
            print(line, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
