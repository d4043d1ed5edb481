"""Same-box A/B of ``ops.set_matmul_precision``: "fp32" (six-term split-bf16 products, the default) against "bf16" (operands
rounded once, one product), alternating the two in ONE process.  HIP events around every timed window.

  (a) the training-size launches, M = 50 148 rows (bs 4 at 600x1000): forward, data gradient and weight gradient of the
      256 -> 256, 256 -> 384, 256 -> 1024 and 1024 -> 256 linears, through the ``terms=`` bindings;
  (b) the bs-4 train step of BASELINE.json configs[2] (bench.py's model, batch and optimizer), one trainer, the global
      setting switched between blocks of steps;
  (c) the relative deviation of the total loss and of the global gradient norm between the two modes on the inputs of the
      tests/golden/sgg_full_train.npz fixture (600x1000, bs 2, auxiliary losses, dropout 0), next to the deviation between two
      "fp32" runs (the atomics of the MSDA backward make the gradient norm of one mode vary from run to run);
  (d) the relation head at B = 4, N = 200, T = 7, R = 50: the training forward launch alone, RelationHeadFunction forward +
      backward, and inside the backward the two data-gradient launches against torch.mm + column_sum and the two weight
      gradients with ``terms`` 1 against 6 (profiles/matmul_precision_rel_head_ab.txt).

    python tools/matmul_precision_bench.py [--rounds 3] [--iters 50] [--steps 10] [--out profiles/matmul_precision_ab.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def time_us(fn, iters):
    for _ in range(5):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def launches(rounds, iters):
    from egtr_amd import ops
    M = 50148
    g = torch.Generator().manual_seed(0)
    say(f"(a) launches at M = {M}: median of {rounds} alternating rounds x {iters} launches, us (TFLOP/s); six-term | one-term | ratio")
    total = {6: 0.0, 1: 0.0}
    for K, N in ((256, 256), (256, 384), (256, 1024), (1024, 256)):
        x = torch.randn(M, K, generator=g).to(DEV)
        gy = torch.randn(M, N, generator=g).to(DEV)
        w = (torch.randn(N, K, generator=g) / 16).to(DEV)
        b = torch.zeros(N, device=DEV)
        y, gx = torch.empty(M, N, device=DEV), torch.empty(M, K, device=DEV)
        fns = {}
        for t in (6, 1):
            wt, wtT = ops.gemm_split_tile(w, terms=t), ops.gemm_split_tile(w, transposed=True, terms=t)
            fns[t] = {"forward": lambda t=t, wt=wt: ops.linear_split_bf16(x, wt, b, N, out=y, terms=t),
                      "data gradient": lambda t=t, wtT=wtT: ops.linear_split_bf16(gy, wtT, None, K, out=gx, terms=t)}
            if N % 128 == 0 and K % 128 == 0:
                fns[t]["weight gradient"] = lambda t=t: ops.linear_split_bf16_wgrad(gy, x, terms=t)
        flop = 2.0 * M * N * K
        for name in fns[6]:
            got = {6: [], 1: []}
            for _ in range(rounds):
                for t in (6, 1):
                    got[t].append(time_us(fns[t][name], iters))
            m6, m1 = statistics.median(got[6]), statistics.median(got[1])
            total[6] += m6
            total[1] += m1
            say(f"  {K:4d} -> {N:4d} {name:16s} {m6:8.1f} ({flop / m6 * 1e-6:6.1f}) | {m1:8.1f} ({flop / m1 * 1e-6:6.1f}) | "
                f"{m6 / m1:5.2f}x   rounds {['%.1f' % v for v in got[6]]} | {['%.1f' % v for v in got[1]]}")
    say(f"  sum of the twelve launches: {total[6]:.1f} | {total[1]:.1f} us")


def train_step(rounds, steps):
    import bench
    from egtr_amd import ops
    from egtr_amd.runtime import DataParallelTrainer, configure_optimizers
    model, cfg, _ = bench.build_model(torch.device(DEV), {"dropout": 0.1})
    model.train()
    opt = configure_optimizers(model, lr=2e-6, lr_backbone=2e-7, lr_initialized=None, weight_decay=1e-4)
    tr = DataParallelTrainer(model, optimizer=opt, accumulate=1, clip=0.1)
    torch.manual_seed(100)
    batch = {"pixel_values": torch.randn(4, 3, bench.H_IMG, bench.W_IMG, device=DEV),
             "pixel_mask": torch.ones(4, bench.H_IMG, bench.W_IMG, dtype=torch.long, device=DEV),
             "labels": bench.make_targets(4, cfg, DEV, 7)}
    got = {"fp32": [], "bf16": []}
    for mode in ("fp32", "bf16"):          # every shape and route warm before the first timed window
        with ops.matmul_precision_mode(mode):
            for _ in range(3):
                tr.training_step(batch)
    for _ in range(rounds):
        for mode in ("fp32", "bf16"):
            with ops.matmul_precision_mode(mode):
                tr.training_step(batch)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                for _ in range(steps):
                    loss, _, _ = tr.training_step(batch)
                b.record()
                torch.cuda.synchronize()
                assert torch.isfinite(loss).item()
                got[mode].append(a.elapsed_time(b) / steps)
    tr.finalize()
    m32, m16 = statistics.median(got["fp32"]), statistics.median(got["bf16"])
    say(f"(b) bs-4 train step (600x1000, N = 200, dropout 0.1, AdamW): median of {rounds} alternating rounds x {steps} steps")
    say(f"  fp32 {m32:.2f} ms/step ({4e3 / m32:.1f} images/s)   rounds {['%.2f' % v for v in got['fp32']]}")
    say(f"  bf16 {m16:.2f} ms/step ({4e3 / m16:.1f} images/s)   rounds {['%.2f' % v for v in got['bf16']]}")
    say(f"  fp32 / bf16 = {m32 / m16:.3f}")
    del tr, opt, model
    torch.cuda.empty_cache()


def deviation():
    import json
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import helpers as Hh
    import weights as W
    from egtr_amd import ops
    g = Hh.load_golden(os.path.join(ROOT, "tests", "golden"), "sgg_full_train.npz")
    cfg_dict, shapes = json.loads(str(g["cfg"])), json.loads(str(g["shapes"]))
    model, cfg, sd = Hh.build_product_model(cfg_dict, shapes, int(g["seed"]))
    model.load_state_dict(sd)
    model = model.to(DEV).train()
    pv, pm = Hh.padded_inputs(g, 2)
    pv, pm = pv.to(DEV), pm.to(DEV)
    targets = [{k: t.to(DEV) for k, t in d.items()}
               for d in W.make_targets(int(g["target_seed"]), 2, cfg.num_queries, cfg.num_labels, cfg.num_rel_labels,
                                       tmin=5, tmax=30)]

    def run(mode):
        model.zero_grad(set_to_none=True)
        with ops.matmul_precision_mode(mode):
            out = model(pixel_values=pv, pixel_mask=pm, labels=targets, output_attention_states=True)
            out.loss.backward()
        sq = sum(p.grad.double().pow(2).sum() for p in model.parameters() if p.grad is not None)
        return float(out.loss.detach()), float(sq.sqrt())

    l32, n32 = run("fp32")
    l32b, n32b = run("fp32")
    l16, n16 = run("bf16")
    say("(c) sgg_full_train inputs (600x1000, bs 2, auxiliary losses, dropout 0), one forward + backward per mode")
    say(f"  total loss     fp32 {l32:.6f}   bf16 {l16:.6f}   relative deviation {abs(l16 - l32) / abs(l32):.3e}   "
        f"(fp32 run to run {abs(l32b - l32) / abs(l32):.1e})")
    say(f"  gradient norm  fp32 {n32:.6f}   bf16 {n16:.6f}   relative deviation {abs(n16 - n32) / abs(n32):.3e}   "
        f"(fp32 run to run {abs(n32b - n32) / abs(n32):.1e})")


def rel_head(rounds, iters):
    """(d) the relation head at B = 4, N = 200, T = 7, R = 50 (160 000 pairs): per piece, "fp32" against "bf16", alternating.  A
    piece stays routed under the mode only if its "bf16" median is below its "fp32" median by more than the spread (max - min)
    of the "fp32" rounds of this run: the verdict is printed per piece."""
    from egtr_amd import ops
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from test_gpu_kernels import _head_inputs
    B, N, T, R = 4, 200, 7, 50
    d, trip, node = _head_inputs(1, B, N, T, R, 150)
    dd = [v.to(DEV) for v in d.values()]
    trip, node = trip.to(DEV), node.to(DEV)
    w2r, w3r, w2c = dd[5], dd[7], dd[9]
    P_, Hd = B * N * N, 256
    g = torch.Generator().manual_seed(2)
    g_rel, g_conn = torch.randn(B, N, N, R, generator=g).to(DEV), torch.randn(B, N, N, 1, generator=g).to(DEV)
    say(f"(d) relation head, B = {B}, N = {N}, T = {T}, R = {R}: median of {rounds} alternating rounds x {iters} calls, us; "
        "fp32 | bf16 | ratio | fp32 spread | verdict")

    def ab(name, fns):
        got = {"fp32": [], "bf16": []}
        for _ in range(rounds):
            for mode in ("fp32", "bf16"):
                got[mode].append(time_us(fns[mode], iters))
        m32, m16 = statistics.median(got["fp32"]), statistics.median(got["bf16"])
        spread = max(got["fp32"]) - min(got["fp32"])
        say(f"  {name:44s} {m32:8.1f} | {m16:8.1f} | {m32 / m16:5.2f}x | {spread:6.1f} | "
            f"{'faster beyond the spread: routed' if m32 - m16 > spread else 'NOT faster beyond the spread'}"
            f"   rounds {['%.1f' % v for v in got['fp32']]} | {['%.1f' % v for v in got['bf16']]}")

    streams = {t: ops.rel_head_streams(w2r, w3r, w2c, terms=t) for t in (6, 1)}
    fwd = lambda t: ops.relation_head_train_forward(*dd, trip, node, True, t, streams=streams[t])   # noqa: E731
    ab("training forward launch", {"fp32": lambda: fwd(6), "bf16": lambda: fwd(1)})

    leaves = [v.clone().requires_grad_(True) for v in dd]

    def step(mode):
        for t in leaves:
            t.grad = None
        with ops.matmul_precision_mode(mode):
            rel, conn, _ = ops.RelationHeadFunction.apply(*leaves, trip, node, True)
            torch.autograd.backward([rel, conn], [g_rel, g_conn])

    ab("RelationHeadFunction forward + backward", {"fp32": lambda: step("fp32"), "bf16": lambda: step("bf16")})

    _, _, _, h1s, h2s = fwd(6)
    del h2s
    dh2 = torch.randn(P_, Hd, generator=g).to(DEV)
    dh1 = torch.empty(2, P_, Hd, device=DEV)
    colp = torch.empty(2, (P_ + 31) // 32, Hd, device=DEV)

    def dgrad_fp32():
        for i, w2 in enumerate((w2r, w2c)):
            torch.mm(dh2, w2, out=dh1[i])
            ops.column_sum(dh1[i], relu_output=h1s[i], inplace=True)

    def dgrad_bf16():
        for i, w2 in enumerate((w2r, w2c)):
            ops.linear_split_ex([dict(x=dh2, wt=ops.gemm_split_tile(w2, transposed=True, terms=1), N=Hd, relu_ref=h1s[i],
                                      colpart=colp[i], out=dh1[i])], P_, Hd, terms=1)
            ops.column_sum(colp[i])

    ab("two data gradients + masks + b1 column sums", {"fp32": dgrad_fp32, "bf16": dgrad_bf16})
    ab("two weight gradients (terms 6 | 1)",
       {"fp32": lambda: [ops.linear_split_bf16_wgrad(dh2, h1s[i], terms=6) for i in range(2)],
        "bf16": lambda: [ops.linear_split_bf16_wgrad(dh2, h1s[i], terms=1) for i in range(2)]})
    del h1s, dh1, dh2, colp, leaves
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--skip", default="", help="comma-separated parts to leave out: a, b, c, d")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a timing from anywhere else says nothing"
    from egtr_amd import _lib
    say(f"device {torch.cuda.get_device_name(0)}; library {os.path.relpath(_lib.LIB_PATH, ROOT)}")
    skip = set(args.skip.split(","))
    if "a" not in skip:
        launches(args.rounds, args.iters)
    if "b" not in skip:
        train_step(args.rounds, args.steps)
    if "c" not in skip:
        deviation()
    if "d" not in skip:
        rel_head(args.rounds, args.iters)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
