#!/usr/bin/env python3
"""A/B timing of the relation loss's sampling routes: the six relation-loss calls of one training batch --
the main output set and five auxiliary ones -- forward and backward, B = 4, N = 200, R = 50, about 20 objects and 25 relations
per image, ``rel_triplets`` targets.

For each configuration the policy kernels (egtr_relation_loss_f32 with a policy other than `largest`) against the route the
criterion took for the SAME configuration before they existed:

  random / random, 80 / 80   device sampler           vs  the reference's composition (nonzero() lists + random.sample)
  largest / None (whole)     policy kernels           vs  _loss_relations_device (masked topk, one host wait)
  random / random, 80 / 80   policy kernels           vs  largest / largest on the existing sampled entries (same passes + key)

Alternating rounds (A, B, A, B, ...), medians over the rounds, spread = max - min.  Two clocks per round: HIP events around the six
calls, and the host clock from before the first call to after a device synchronise -- the compositions' cost is mostly host waits,
which events on an idle stream under-count.  Needs a GPU; writes the table to --out.

  python tools/relation_sampling_bench.py --rounds 5 --out profiles/relation_sampling_ab.txt"""
import argparse
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETS = 6


def make_batch(B, N, R, objects, relations, seed, dev):
    """(per-set logits, targets, indices, costs): the same matching and targets for the six output sets, own logits each."""
    rng = np.random.default_rng(seed)
    targets, indices, costs = [], [], []
    for _ in range(B):
        T = int(rng.integers(objects - 4, objects + 5))
        pairs = rng.choice(T * T, size=min(relations, T * T), replace=False)
        trips = np.stack([pairs // T, pairs % T, rng.integers(0, R, len(pairs))], 1).astype(np.int64)
        targets.append({"rel_triplets": torch.as_tensor(trips).to(dev)})
        indices.append((torch.as_tensor(np.sort(rng.choice(N, T, replace=False))).to(dev),
                        torch.as_tensor(rng.permutation(T)).to(dev)))
        costs.append(torch.as_tensor((rng.standard_normal(T) * 3).astype(np.float32)).to(dev))
    g = torch.Generator(device="cpu").manual_seed(seed)
    logits = [(torch.randn(B, N, N, R, generator=g) * 2 - 3).to(dev) for _ in range(SETS)]
    conn = [torch.randn(B, N, N, 1, generator=g).to(dev) for _ in range(SETS)]
    return logits, conn, targets, indices, costs


def criterion(N, R, neg, nm, neg_largest, nm_largest, dev):
    from egtr_amd.egtr import SceneGraphGenerationLoss
    matcher = types.SimpleNamespace(class_cost=2.0, bbox_cost=5.0, giou_cost=2.0)
    return SceneGraphGenerationLoss(matcher=matcher, num_object_queries=N, num_classes=150, num_rel_labels=R, eos_coef=0.1,
                                    losses=["relations"], smoothing=1e-14, rel_sample_negatives=neg, rel_sample_nonmatching=nm,
                                    model_training=True, focal_alpha=0.25, rel_sample_negatives_largest=neg_largest,
                                    rel_sample_nonmatching_largest=nm_largest).to(dev)


def six_calls(fn, logits, conn):
    """forward + backward of the six sets' relation losses through ``fn(outputs) -> loss dict``; returns the summed loss."""
    total = None
    for pr, pc in zip(logits, conn):
        pr, pc = pr.detach().requires_grad_(True), pc.detach().requires_grad_(True)
        out = fn({"pred_rel": pr, "pred_connectivity": pc})
        term = out["loss_rel"] + out["loss_connectivity"]
        total = term if total is None else total + term
    total.backward()
    return total.detach()


def timed(run):
    """(event ms, host ms) of one round of ``run``; the host clock ends after a device synchronise."""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3


def ab(name_a, run_a, name_b, run_b, rounds, warmup):
    for _ in range(warmup):
        run_a()
        run_b()
    res = {name_a: [], name_b: []}
    for _ in range(rounds):
        res[name_a].append(timed(run_a))
        res[name_b].append(timed(run_b))
    lines = []
    for name, rows in res.items():
        ev, host = [r[0] for r in rows], [r[1] for r in rows]
        lines.append(f"  {name:58s} events {statistics.median(ev):9.3f} ms (spread {max(ev) - min(ev):8.3f})   "
                     f"host+sync {statistics.median(host):9.3f} ms (spread {max(host) - min(host):8.3f})")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--queries", type=int, default=200)
    ap.add_argument("--rel", type=int, default=50)
    ap.add_argument("--objects", type=int, default=20)
    ap.add_argument("--relations", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rounds < 3:
        ap.error("--rounds must be at least 3 (medians)")
    if not torch.cuda.is_available():
        sys.exit("relation_sampling_bench.py measures on a GPU; none is available")
    from egtr_amd import ops
    dev = torch.device("cuda:0")
    B, N, R = a.batch, a.queries, a.rel
    logits, conn, targets, indices, costs = make_batch(B, N, R, a.objects, a.relations, 0, dev)

    def through(crit):
        return lambda outputs: crit.loss_relations(outputs, targets, indices, costs, 1.0)

    lines = [f"Relation loss sampling routes: six relation-loss calls (forward + backward) of one batch, B = {B}, N = {N}, R = {R}, "
             f"~{a.objects} objects and {a.relations} relations per image, triplet targets; {a.rounds} alternating rounds after "
             f"{a.warmup} warm-up rounds, medians, spread = max - min; {torch.cuda.get_device_name(0)}", ""]

    rr = criterion(N, R, 80, 80, False, False, dev)

    def rr_device():
        with ops.relation_sampler_mode("device"):
            six_calls(through(rr), logits, conn)

    def rr_python():
        with ops.relation_sampler_mode("python"):
            six_calls(through(rr), logits, conn)

    lines.append("random / random, 80 / 80:")
    lines += ab("policy kernels, device sampler (this change)", rr_device,
                "reference composition, random.sample (before)", rr_python, a.rounds, a.warmup)

    ln = criterion(N, R, 80, None, True, True, dev)

    def ln_before(outputs):   # what loss_relations did with one count None: dense targets, then the tensor composition
        return ln._loss_relations_device(outputs, ln._dense_targets(targets, dev), indices, costs)

    lines += ["", "largest 80 / whole non-matching class (rel_sample_nonmatching = None):"]
    lines += ab("policy kernels (this change)", lambda: six_calls(through(ln), logits, conn),
                "_loss_relations_device (before)", lambda: six_calls(ln_before, logits, conn), a.rounds, a.warmup)

    ll = criterion(N, R, 80, 80, True, True, dev)
    lines += ["", "random / random against largest / largest, 80 / 80, both on the device:"]
    lines += ab("policy kernels, random / random", rr_device,
                "existing sampled entries, largest / largest", lambda: six_calls(through(ll), logits, conn), a.rounds, a.warmup)
    if ops.FALLBACKS:
        lines += ["", f"FALLBACKS: {ops.FALLBACKS}"]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
