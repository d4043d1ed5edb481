"""Relation targets, dense against bit-packed, on one GPU.  Prints one JSON line.

At N = 200, R = 50, B = 4 with 20 triplets per image (the training shape of bench.py), in one process:
  dense_us / packed_us   stream time of one call of egtr_relation_loss_f32 with target format 0 (dense) / 1 (packed words) on
                         the same logits, matcher outputs and targets: device events around --iters back-to-back calls, warm,
                         the two forms in alternating blocks, median over --blocks blocks (and every block's figure)
  parent_dense_us        the same for egtr_relation_loss_f32 of ANOTHER build of the library (--parent-lib: an ABI-6 build,
                         where the dense form was an entry of its own), in the same alternation: the yardstick of "nothing
                         got slower"
  launch_host_us         host time of one ``ops.relation_loss_launch`` call (allocations, argument marshalling and the
                         entry's launches, not waited for), median and range over --blocks x --iters calls
  pack_us                one egtr_pack_relations_u64 call (memset + launch) on triplets already on the device
  h2d_*_us               the host -> device copy of the batch's triplets + offsets (one buffer) against the copy of four
                         dense [N, N, R] fp32 targets, from pinned and from pageable memory: host clock around copies that
                         end in a synchronise, median of --blocks
  results_identical      loss_out, grad_rel and grad_conn of the two forms compared bit for bit on these inputs

    python tools/rel_targets_bench.py [--iters 50] [--blocks 7] [--parent-lib PATH] [--out profiles/rel_targets_bench.json]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, N, R, K_PER_IMAGE, T_PER_IMAGE, SAMPLE = 4, 200, 50, 20, 12, 80


def inputs(dev):
    g = torch.Generator().manual_seed(11)
    trips, indices, costs = [], [], []
    for _ in range(B):
        so = torch.stack([torch.randint(0, T_PER_IMAGE, (K_PER_IMAGE,), generator=g),
                          torch.randint(0, T_PER_IMAGE, (K_PER_IMAGE,), generator=g)], 1)
        trips.append(torch.cat([so, torch.randint(0, R, (K_PER_IMAGE, 1), generator=g)], 1))
        indices.append((torch.randperm(N, generator=g)[:T_PER_IMAGE].sort()[0], torch.randperm(T_PER_IMAGE, generator=g)))
        costs.append(torch.randn(T_PER_IMAGE, generator=g) * 3)
    n = B * N * N * R
    pred_rel = (((torch.randperm(n, generator=g).float() + 0.5) / n - 0.5) * 8.0).view(B, N, N, R)   # no two logits equal
    pred_conn = torch.randn(B, N, N, 1, generator=g)
    dense = []
    for t in trips:
        rel = torch.zeros(N, N, R)
        rel[t[:, 0], t[:, 1], t[:, 2]] = 1.0
        dense.append(rel)
    return trips, dense, indices, costs, pred_rel.to(dev), pred_conn.to(dev)


def event_us(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters


def host_us(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rel_targets_bench needs a GPU: nothing is measured without one")
    if args.blocks < 5:
        raise SystemExit("--blocks must be at least 5")
    from egtr_amd import _lib, ops
    from egtr_amd import targets as T
    dev = torch.device("cuda:0")
    trips, dense, indices, costs, pred_rel, pred_conn = inputs(dev)
    offs = [0]
    for a, _ in indices:
        offs.append(offs[-1] + int(a.shape[0]))
    pi = torch.cat([a for a, _ in indices]).to(dev)
    ti = torch.cat([b for _, b in indices]).to(dev)
    mc = torch.cat(costs).to(dev)
    off = torch.tensor(offs, dtype=torch.int32).to(dev)
    rels = [d.to(dev) for d in dense]
    ptrs = torch.tensor([r.data_ptr() for r in rels], dtype=torch.int64).to(dev)
    bits = T.pack_relations([{"rel_triplets": t} for t in trips], N, R, dev)
    nm = 60.0

    h = _lib.lib()
    loss = torch.empty(2, device=dev)
    grad_rel, grad_conn = torch.empty_like(pred_rel), torch.empty_like(pred_conn)
    ws = torch.empty(int(h.egtr_relation_loss_workspace_bytes(B, N)), dtype=torch.uint8, device=dev)

    def entry(fn, target, *form):
        """``form``: what this build's entry takes between the target and the matcher's outputs (the target format) and
        after the workspace (both policies `largest`, seed, stream, arrival-order ties); nothing for the ABI-6 prototype"""
        head, tail = form[:1], form[1:]

        def call():
            st = fn(_lib._stream(), pred_rel.data_ptr(), pred_conn.data_ptr(), target.data_ptr(), *head, pi.data_ptr(),
                    ti.data_ptr(), mc.data_ptr(), off.data_ptr(), B, N, R, nm, SAMPLE, SAMPLE, loss.data_ptr(),
                    grad_rel.data_ptr(), grad_conn.data_ptr(), ws.data_ptr(), *tail)
            if st != 0:
                raise RuntimeError(f"status {st}")
        return call

    runs = {"dense_us": entry(h.egtr_relation_loss_f32, ptrs, 0, 0, 0, 0, 0, 0),
            "packed_us": entry(h.egtr_relation_loss_f32, bits, 1, 0, 0, 0, 0, 0)}
    if args.parent_lib:   # the parent is by definition the OLD interface: its prototype is written out, not borrowed
        parent = ctypes.CDLL(args.parent_lib)
        vp, ci = ctypes.c_void_p, ctypes.c_int
        parent.egtr_relation_loss_f32.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ctypes.c_float, ci, ci, vp, vp,
                                                  vp, vp]
        parent.egtr_relation_loss_f32.restype = ci
        runs["parent_dense_us"] = entry(parent.egtr_relation_loss_f32, ptrs)

    d = ops.relation_loss_launch(pred_rel, pred_conn, ptrs, False, pi, ti, mc, off, nm, SAMPLE, SAMPLE)
    p = ops.relation_loss_launch(pred_rel, pred_conn, bits, True, pi, ti, mc, off, nm, SAMPLE, SAMPLE)
    identical = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(d, p))

    trip_d = torch.cat(trips).to(dev)
    off_k = torch.tensor([K_PER_IMAGE * i for i in range(B + 1)], dtype=torch.int32).to(dev)
    runs["pack_us"] = lambda: ops.pack_relation_bits(trip_d, off_k, B, B * K_PER_IMAGE, N, R)

    for fn in runs.values():       # warm every timed shape
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    blocks = {k: [] for k in runs}
    for _ in range(args.blocks):    # alternating blocks: drift of the box falls on every entry alike
        for k, fn in runs.items():
            blocks[k].append(event_us(fn, args.iters))
    res = {"tool": "rel_targets_bench", "device": torch.cuda.get_device_name(0), "B": B, "N": N, "R": R,
           "triplets_per_image": K_PER_IMAGE, "matched_per_image": T_PER_IMAGE, "iters": args.iters, "blocks": args.blocks,
           "results_identical": bool(identical)}
    for k, v in blocks.items():
        res[k] = round(statistics.median(v), 2)
        res[k + "_blocks"] = [round(x, 2) for x in v]

    # host time of the binding: the clock around one call that is not waited for, the queue empty before it
    def launch_host_us():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ops.relation_loss_launch(pred_rel, pred_conn, ptrs, False, pi, ti, mc, off, nm, SAMPLE, SAMPLE)
        return (time.perf_counter() - t0) * 1e6
    host = sorted(launch_host_us() for _ in range(args.blocks * args.iters))
    res["launch_host_us"] = round(statistics.median(host), 2)
    res["launch_host_us_range"] = [round(host[0], 2), round(host[-1], 2)]

    # host -> device copies: triplets + offsets in one buffer against four dense targets
    n_trip = 2 * ((B + 4) // 4) + 3 * B * K_PER_IMAGE
    small_pageable = torch.zeros(n_trip, dtype=torch.int64)
    small_pinned = small_pageable.pin_memory()
    dense_pageable = [x.clone() for x in dense]
    dense_pinned = [x.pin_memory() for x in dense]
    copies = {"h2d_triplets_pinned_us": lambda: small_pinned.to(dev, non_blocking=True),
              "h2d_triplets_pageable_us": lambda: small_pageable.to(dev, non_blocking=True),
              "h2d_dense_pinned_us": lambda: [x.to(dev, non_blocking=True) for x in dense_pinned],
              "h2d_dense_pageable_us": lambda: [x.to(dev, non_blocking=True) for x in dense_pageable]}
    for fn in copies.values():
        fn()
    for k, fn in copies.items():
        res[k] = round(statistics.median(host_us(fn) for _ in range(args.blocks)), 1)
    res["bytes_triplets"] = n_trip * 8
    res["bytes_dense"] = B * N * N * R * 4
    res["bytes_words"] = B * N * N * 8
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
