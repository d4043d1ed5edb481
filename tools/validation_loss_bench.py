"""The relation losses of a validation batch, kernel route against the tensor composition, on one GPU.

In evaluation mode the criterion's relation loss is un-sampled: BCE over all N N R elements.  ``ops.RELATION_LOSS_ALL`` selects
between one HIP pipeline per output set (egtr_relation_loss_all_f32 on packed words, value-only under no_grad) and the per-image tensor
composition of the reference (dense target, permuting gathers, ``torch.nonzero``).  Two legs in ONE process, alternating, at
B = 4, N = 200, R = 50, six output sets, ``rel_triplets`` targets (the words are packed once per call, as the criterion's forward
does):
  criterion   the six ``loss_relations`` calls of a batch under no_grad: stream time between two device events around them, and
              the host clock from the first call to the end of a synchronise (the composition's cost is largely host waits)
  step        ``DataParallelTrainer.validation_step`` of the bench model (600 x 1000, batch 4, auxiliary losses on: six output
              sets), host clock around --steps steps ending in a synchronise; skipped with --no-step
Prints the table, and writes it to --out with the sha256 of csrc/loss.hip.

    python tools/validation_loss_bench.py [--rounds 7] [--iters 5] [--steps 3] [--no-step] [--out profiles/validation_loss_ab.txt]"""
import argparse
import os
import statistics
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

B, N, R, SETS, K_PER_IMAGE, T_PER_IMAGE = 4, 200, 50, 6, 20, 12


def criterion_inputs(dev):
    g = torch.Generator().manual_seed(12)
    targets, indices, costs = [], [], []
    for _ in range(B):
        so = torch.randint(0, T_PER_IMAGE, (K_PER_IMAGE, 2), generator=g)
        targets.append({"rel_triplets": torch.cat([so, torch.randint(0, R, (K_PER_IMAGE, 1), generator=g)], 1)})
        indices.append((torch.randperm(N, generator=g)[:T_PER_IMAGE].sort()[0].to(dev), torch.randperm(T_PER_IMAGE, generator=g).to(dev)))
        costs.append((torch.randn(T_PER_IMAGE, generator=g) * 3).to(dev))
    outputs = [{"pred_rel": torch.randn(B, N, N, R, generator=g).to(dev), "pred_connectivity": torch.randn(B, N, N, 1, generator=g).to(dev)}
               for _ in range(SETS)]
    return outputs, targets, indices, costs


def make_criterion(dev):
    from egtr_amd.egtr import SceneGraphGenerationLoss
    matcher = types.SimpleNamespace(class_cost=2.0, bbox_cost=5.0, giou_cost=2.0)
    return SceneGraphGenerationLoss(matcher=matcher, num_object_queries=N, num_classes=150, num_rel_labels=R, eos_coef=0.1,
                                    losses=["relations"], smoothing=1e-14, rel_sample_negatives=80, rel_sample_nonmatching=80,
                                    model_training=False, focal_alpha=0.25, rel_sample_negatives_largest=True,
                                    rel_sample_nonmatching_largest=True).to(dev)


def spread(v):
    return max(v) - min(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5, help="criterion leg: calls per round")
    ap.add_argument("--steps", type=int, default=3, help="step leg: validation steps per round")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("validation_loss_bench needs a GPU: nothing is measured without one")
    if args.rounds < 5:
        raise SystemExit("--rounds must be at least 5")
    from egtr_amd import ops
    from egtr_amd import targets as T
    from kernel_source_hash import source_hash
    dev = torch.device("cuda:0")
    outputs, targets, indices, costs = criterion_inputs(dev)
    crit = make_criterion(dev)

    def batch_losses():
        crit._rel_bits_cache = (targets, dev, T.pack_relations(targets, N, R, dev))
        try:
            with torch.no_grad():
                return [crit.loss_relations(o, targets, indices, costs, 1.0) for o in outputs]
        finally:
            crit._rel_bits_cache = None

    def criterion_round():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        for _ in range(args.iters):
            batch_losses()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / args.iters, (time.perf_counter() - t0) * 1e6 / args.iters

    legs = {"kernel": True, "composition": False}
    values = {}
    for name, on in legs.items():      # warm both, and compare what they compute
        ops.RELATION_LOSS_ALL = on
        for _ in range(2):
            values[name] = batch_losses()
    worst = max(abs(float(a[k]) - float(b[k])) / abs(float(b[k])) for a, b in zip(values["kernel"], values["composition"]) for k in a)
    crit_us = {name: [] for name in legs}
    for _ in range(args.rounds):       # alternating: drift of the box falls on both legs alike
        for name, on in legs.items():
            ops.RELATION_LOSS_ALL = on
            crit_us[name].append(criterion_round())

    step_ms = {name: [] for name in legs}
    if not args.no_step:
        import bench
        from egtr_amd.runtime import DataParallelTrainer
        model, cfg, _ = bench.build_model(dev, {"auxiliary_loss": True})
        tr = DataParallelTrainer(model, optimizer=torch.optim.SGD(model.parameters(), lr=0.0), accumulate=1)
        labels = []
        for t in bench.make_targets(B, cfg, dev, 7):
            labels.append({"class_labels": t["class_labels"], "boxes": t["boxes"], "rel_triplets": t["rel"].nonzero()})
        batch = {"pixel_values": torch.randn(B, 3, bench.H_IMG, bench.W_IMG, device=dev),
                 "pixel_mask": torch.ones(B, bench.H_IMG, bench.W_IMG, dtype=torch.long, device=dev), "labels": labels}
        for name, on in legs.items():
            ops.RELATION_LOSS_ALL = on
            for _ in range(3):
                tr.validation_step(batch)
        for _ in range(args.rounds):
            for name, on in legs.items():
                ops.RELATION_LOSS_ALL = on
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    tr.validation_step(batch)
                torch.cuda.synchronize()
                step_ms[name].append((time.perf_counter() - t0) * 1e3 / args.steps)
    ops.RELATION_LOSS_ALL = True

    def row(label, unit, k, c):
        fmt = lambda v: " ".join(f"{x:9.1f}" for x in v)  # noqa: E731
        gain = statistics.median(c) - statistics.median(k)
        verdict = "gain exceeds the slower leg's spread" if gain > spread(c) else "within the slower leg's spread: no claim"
        return [f"{label} ({unit} per {'batch' if unit == 'us' else 'step'}), rounds in order",
                f"    kernel route   median {statistics.median(k):9.1f}   spread {spread(k):8.1f}   | {fmt(k)}",
                f"    composition    median {statistics.median(c):9.1f}   spread {spread(c):8.1f}   | {fmt(c)}",
                f"    difference of medians {gain:9.1f} {unit}: {verdict}"]

    lines = [f"validation_loss_bench: relation losses of a validation batch, ops.RELATION_LOSS_ALL on (kernel route) / off (composition)",
             f"device {torch.cuda.get_device_name(0)}; B = {B}, N = {N}, R = {R}, {SETS} output sets, {K_PER_IMAGE} triplets and "
             f"{T_PER_IMAGE} matches per image; {args.rounds} alternating rounds, {args.iters} batches / {args.steps} steps per round",
             f"source_sha256 csrc/loss.hip {source_hash('rel_loss')}",
             f"largest relative difference of a loss term between the legs: {worst:.2e}", ""]
    lines += row("criterion, stream time between device events", "us", [x[0] for x in crit_us["kernel"]], [x[0] for x in crit_us["composition"]])
    lines += row("criterion, host clock to the end of a synchronise", "us", [x[1] for x in crit_us["kernel"]], [x[1] for x in crit_us["composition"]])
    if not args.no_step:
        lines += row("validation_step end to end, 600 x 1000, batch 4, host clock", "ms", step_ms["kernel"], step_ms["composition"])
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
