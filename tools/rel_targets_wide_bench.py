"""Triplet-list relation targets above 64 predicates: wide packed words against per-step dense materialisation,
on one GPU.  Prints a table, and writes it with --out.

At B = 4, N = 200 and R = 100 and 256, ~30 triplets per image, the criterion's relation terms (``relations`` + ``uncertainty``,
matcher outputs given) of ``SceneGraphGenerationLoss`` are timed on ``rel_triplets`` targets by two routes in ONE process:
  wide     the criterion as it is: the triplets packed into [B, N, N, ceil(R / 64)] words once per call, the loss kernels read bits
  dense    what the criterion did for such targets before the wide words existed: ``targets.dense_targets`` materialises one fp32
           [N, N, R] tensor per image (``materialize_relations``: zero fill + indexed write) in EVERY call, and the dense loss
           entries read it
in two configurations:
  train    training mode, 80 / 80 sampling, value and gradient (forward + backward of loss_rel + loss_connectivity)
  valid    evaluation mode under no_grad: the un-sampled, value-only pass over all B N N R elements
Host clock around --iters calls that end in a synchronise (a step pays the host work too), the two routes in alternating rounds,
median with min and max over --rounds rounds; peak ``torch.cuda.max_memory_allocated`` of a call above what is resident before it
(logits, matcher outputs).  The terms of the two routes are compared bit for bit.

    python tools/rel_targets_wide_bench.py [--iters 20] [--rounds 7] [--out profiles/rel_targets_wide_ab.txt]"""
import argparse
import os
import statistics
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, N, K_PER_IMAGE, T_PER_IMAGE, SAMPLE = 4, 200, 30, 12, 80


def inputs(R, dev):
    g = torch.Generator().manual_seed(17 + R)
    trips, indices, costs = [], [], []
    for _ in range(B):
        so = torch.stack([torch.randint(0, T_PER_IMAGE, (K_PER_IMAGE,), generator=g),
                          torch.randint(0, T_PER_IMAGE, (K_PER_IMAGE,), generator=g)], 1)
        trips.append(torch.cat([so, torch.randint(0, R, (K_PER_IMAGE, 1), generator=g)], 1))
        indices.append((torch.randperm(N, generator=g)[:T_PER_IMAGE].sort()[0].to(dev), torch.randperm(T_PER_IMAGE, generator=g).to(dev)))
        costs.append((torch.randn(T_PER_IMAGE, generator=g) * 3).to(dev))
    pred_rel = torch.randn(B, N, N, R, generator=g).to(dev)
    pred_conn = torch.randn(B, N, N, 1, generator=g).to(dev)
    labels = torch.zeros(T_PER_IMAGE, dtype=torch.int64, device=dev)
    targets = [{"class_labels": labels, "rel_triplets": t} for t in trips]               # host triplets, as a loader gives them
    return targets, indices, costs, pred_rel, pred_conn


def criterion(R, training, dev):
    from egtr_amd.egtr import SceneGraphGenerationLoss
    matcher = types.SimpleNamespace(class_cost=2.0, bbox_cost=5.0, giou_cost=2.0)
    return SceneGraphGenerationLoss(matcher=matcher, num_object_queries=N, num_classes=150, num_rel_labels=R, eos_coef=0.1,
                                    losses=["relations", "uncertainty"], smoothing=1e-14, rel_sample_negatives=SAMPLE,
                                    rel_sample_nonmatching=SAMPLE, model_training=training, focal_alpha=0.25,
                                    rel_sample_negatives_largest=True, rel_sample_nonmatching_largest=True).to(dev)


def measure(R, training, iters, rounds, dev):
    from egtr_amd import targets as T
    trip, indices, costs, pred_rel, pred_conn = inputs(R, dev)
    crit = criterion(R, training, dev)
    matched = (indices, costs)

    def call(route):
        tg = trip if route == "wide" else T.dense_targets(trip, N, R, dev)     # the dense route materialises in every call
        if training:
            pr, pc = pred_rel.detach().requires_grad_(True), pred_conn.detach().requires_grad_(True)
            out = crit({"pred_rel": pr, "pred_connectivity": pc}, tg, matched=matched)
            (out["loss_rel"] + out["loss_connectivity"]).backward()
            return out, pr.grad, pc.grad
        with torch.no_grad():
            return crit({"pred_rel": pred_rel, "pred_connectivity": pred_conn}, tg, matched=matched), None, None

    res = {}
    for route in ("wide", "dense"):        # warm, the terms for the comparison, the peak of one call
        for _ in range(3):
            call(route)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = call(route)
        torch.cuda.synchronize()
        res[route] = dict(out=out, peak=torch.cuda.max_memory_allocated() - before, us=[])
        del out
    a, b = res["wide"]["out"], res["dense"]["out"]
    same = all(torch.equal(a[0][k], b[0][k]) or bool(torch.isnan(a[0][k]) & torch.isnan(b[0][k])) for k in a[0])
    same = same and set(a[0]) == set(b[0]) and all(x is None or torch.equal(x, y) for x, y in zip(a[1:], b[1:]))
    for r in res.values():
        del r["out"]
    for _ in range(rounds):                # alternating rounds: drift of the machine falls on both routes alike
        for route in ("wide", "dense"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                call(route)
            torch.cuda.synchronize()
            res[route]["us"].append((time.perf_counter() - t0) * 1e6 / iters)
    return res, same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rel_targets_wide_bench needs a GPU: nothing is measured without one")
    if args.rounds < 5:
        raise SystemExit("--rounds must be at least 5")
    dev = torch.device("cuda:0")
    lines = [f"{torch.cuda.get_device_name(0)}: B = {B}, N = {N}, {K_PER_IMAGE} triplets and {T_PER_IMAGE} matched targets per image; "
             f"{args.iters} calls per round, {args.rounds} alternating rounds; us per call (host clock, synchronised)",
             f"{'R':>4} {'config':>6} {'route':>6} {'median':>9} {'min':>9} {'max':>9} {'peak MB':>9} {'target MB':>10}  terms equal"]
    for R in (100, 256):
        W = (R + 63) // 64
        for training in (True, False):
            res, same = measure(R, training, args.iters, args.rounds, dev)
            for route in ("wide", "dense"):
                us = res[route]["us"]
                target = B * N * N * (W * 8 if route == "wide" else R * 4)
                lines.append(f"{R:>4} {'train' if training else 'valid':>6} {route:>6} {statistics.median(us):>9.1f} {min(us):>9.1f} "
                             f"{max(us):>9.1f} {res[route]['peak'] / 1e6:>9.2f} {target / 1e6:>10.2f}  {same}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
