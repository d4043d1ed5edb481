#!/usr/bin/env python3
"""bench.py -- EGTR end-to-end scene-graph-generation throughput on MI355X.

Workload (BASELINE.json configs[1], the reference's FPS path, evaluate_egtr.py:26-36): one 600x1000 image per
step, ResNet-50 backbone, 6 encoder / 6 decoder layers, N = 200 object queries, 150 object classes, 50
predicates, fp32, synthetic input (randn pixels, all-ones mask), random-init weights of that architecture.
A "step" = one forward pass of one batch; inputs are resident in HBM before the timed region.

    python bench.py                       # 1 GPU, defaults finish in about a minute
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

Multi-GPU: images are independent, so each rank runs its own replica on its own images (weak scaling, no
data-path collective); the timed region is bracketed by a barrier + synchronize and the MAX over ranks is used.

`python bench.py --gpus N` with N > 1 and no torchrun environment starts the N ranks itself (a child
`torch.distributed.run`, spawned BEFORE this process touches the GPU); rank 0 reports `n_gpus` = the world size and
`rccl_ranks` = the result of a real all-reduce over RCCL.

Prints ONE JSON line on rank 0 with the driver's contract (metric, value, unit, higher_is_better, dtype, ms_per_step,
...).  A plain run does only that: set up, warm up, time --steps forwards, print.  Everything else the benchmark measures
is behind --full (off by default), which adds to the same line
  "roofline":     the encoder MSDA kernel (dominant hand-written kernel): algorithmic bytes per launch / its
                  average duration measured with HIP events on the launch stream, against the 8 TB/s HBM peak;
  "roofline_kernels": the same entry plus the matrix-core kernels; the split-bf16 ("x6") ones are priced against the unit
                  they run on (executed bf16 FLOPs / time against the 2.5 PFLOP/s dense bf16 peak; the fp32-equivalent
                  rate is kept as `achieved_fp32_equiv`, the matrix-pipe busy counter as `mfma_busy`);
  "cpu_baseline": the CPU oracle (the reference's pure-PyTorch fallback semantics) timed on the host cores on a
                  bounded sample of the same workload (rank 0, N = 1 only), with the logit parity against it;
and the other workloads (`eager`, `mixed_shapes`, `batched_bs8`, `train_step`, `stress_bf16`, `train_step_ddp`).

--dump-outputs DIR writes what the timed path handed its caller in the last timed step as DIR/<name>.npy (see
dump_outputs); inputs and weights are seeded, so two builds run with the same arguments can be compared output for output.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

CFG = dict(num_queries=200, encoder_layers=6, decoder_layers=6, dropout=0.1, auxiliary_loss=False, num_labels=150,
           num_rel_labels=50, ce_loss_coefficient=2.0, rel_loss_coefficient=15.0, connectivity_loss_coefficient=30.0,
           smoothing=1e-14, rel_sample_negatives=80, rel_sample_nonmatching=80, rel_sample_negatives_largest=True,
           rel_sample_nonmatching_largest=True, use_freq_bias=True, use_log_softmax=False, freq_bias_eps=1e-12,
           logit_adjustment=False, logit_adj_tau=0.3)
H_IMG, W_IMG = 600, 1000
HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec


def build_model(device, cfg_over=None):
    import numpy as np
    from egtr_amd.deformable_detr import DeformableDetrConfig
    from egtr_amd.egtr import DetrForSceneGraphGeneration
    c = dict(CFG)
    c.update(cfg_over or {})
    base = ("num_queries", "encoder_layers", "decoder_layers", "dropout", "auxiliary_loss")
    cfg = DeformableDetrConfig(**{k: c[k] for k in base})
    for k, v in c.items():
        if k not in base:
            setattr(cfg, k, v)
    fg = np.random.RandomState(0).randint(0, 5, (cfg.num_labels + 1, cfg.num_labels + 1, cfg.num_rel_labels))
    torch.manual_seed(0)
    model = DetrForSceneGraphGeneration(cfg, fg_matrix=fg.astype(np.float64))
    return model.to(device).eval(), cfg, c


DUMP_BYTES = 60_000_000   # --dump-outputs: at most this many bytes of array data in all


def output_arrays(obj, name=""):
    """[(name, tensor)] of every tensor in a model output / loss dict, nested tuples and lists as name.<i>, in order."""
    if torch.is_tensor(obj):
        return [(name, obj)]
    if isinstance(obj, (int, float)) and not isinstance(obj, bool):
        return [(name, torch.tensor(float(obj), dtype=torch.float64))]
    if isinstance(obj, dict):
        items = obj.items()
    elif isinstance(obj, (list, tuple)):
        items = ((str(i), v) for i, v in enumerate(obj))
    else:
        return []
    return [a for k, v in items for a in output_arrays(v, f"{name}.{k}" if name else str(k))]


def dump_outputs(path, arrays):
    """Write ``arrays`` ([(name, tensor)]) as path/<name>.npy: float64 for float64 and integer / boolean tensors, float32 for
    the rest.  DUMP_BYTES is shared out smallest array first: an array that fits its equal share of what is left is written
    whole, a larger one as a fixed sample of its flattened elements (seeded positions that depend only on the element count
    and the shapes of the other arrays, so every run with the same arguments samples the same positions), as a 1-D array."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    dtypes = [torch.float32 if t.is_floating_point() and t.dtype != torch.float64 else torch.float64 for _, t in arrays]
    size = [8 if d == torch.float64 else 4 for d in dtypes]
    keep, left = [0] * len(arrays), DUMP_BYTES
    order = sorted(range(len(arrays)), key=lambda i: arrays[i][1].numel() * size[i])
    for n, i in enumerate(order):
        keep[i] = min(arrays[i][1].numel(), left // (len(order) - n) // size[i])
        left -= keep[i] * size[i]
    perms, sampled = {}, []
    for (name, t), dtype, k in zip(arrays, dtypes, keep):
        t = t.detach()
        if t.numel() > k:
            if t.numel() not in perms:
                perms[t.numel()] = torch.randperm(t.numel(), generator=torch.Generator().manual_seed(0))
            pick = perms[t.numel()][:k].sort().values
            t = t.reshape(-1)[pick.to(t.device)]
            sampled.append(name)
        np.save(os.path.join(path, name + ".npy"), t.to(dtype).cpu().numpy())
    print(f"[bench] --dump-outputs: {len(arrays)} arrays in {path}"
          + (f" ({len(sampled)} as fixed samples: {', '.join(sampled)})" if sampled else ""), file=sys.stderr)


class MsdaProbe:
    """Remembers the operands of the most recent encoder-shaped (Lq == S) MSDA forward launch: the inference path calls
    the fused entry (softmax + sampling locations inside the kernel), the training path the plain one."""

    def __init__(self):
        self.args = None
        self.fused = False
        self.keep_bits = None      # the bit-packed padding mask the model handed to the fused entry (explicit argument)
        from egtr_amd import ops
        self._ops = ops
        self._orig = ops.MultiScaleDeformableAttentionFunction.forward
        self._orig_fused = ops.msda_forward_fused

    def __enter__(self):
        probe = self
        orig, orig_fused = self._orig, self._orig_fused

        def fwd(ctx, value, shapes, lsi, loc, attn, step):
            if loc.shape[1] == value.shape[1]:
                probe.args, probe.fused = (value, shapes, lsi, loc, attn, step), False
            return orig(ctx, value, shapes, lsi, loc, attn, step)

        def fwd_fused(value, shapes, lsi, off, logits, ref, want_weights=False, keep_mask=None, **kw):
            if off.shape[1] == value.shape[1]:
                probe.args, probe.fused = (value, shapes, lsi, off, logits, ref, False, keep_mask), True
                probe.keep_bits = kw.get("keep_bits")
            return orig_fused(value, shapes, lsi, off, logits, ref, want_weights, keep_mask, **kw)

        self._ops.MultiScaleDeformableAttentionFunction.forward = staticmethod(fwd)
        self._ops.msda_forward_fused = fwd_fused
        return self

    def __exit__(self, *a):
        self._ops.MultiScaleDeformableAttentionFunction.forward = staticmethod(self._orig)
        self._ops.msda_forward_fused = self._orig_fused


class RelHeadProbe:
    """Remembers the operands of the most recent relation-head launch (egtr_amd.ops.relation_head)."""

    def __init__(self):
        from egtr_amd import ops
        self._ops, self._orig, self.args = ops, ops.relation_head, None

    def __enter__(self):
        probe, orig = self, self._orig

        def rel(*a, **kw):
            probe.args = (a, kw)
            return orig(*a, **kw)

        self._ops.relation_head = rel
        return self

    def __exit__(self, *a):
        self._ops.relation_head = self._orig


MFMA_F32_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md: fp32-input MFMA = the fp32 vector peak
MFMA_BF16_PEAK_TFLOPS = 2500.0  # MI355X_MICROARCH.md: dense bf16 MFMA peak (what the split-bf16 "x6" kernels run on)


def time_rel_head_kernel(args, iters=100):
    """Average duration of the fused relation-head forward (one launch = one image batch) and its algorithmic FLOPs:
    per (i, j) pair the gated first layer (T slots x 2*Hd outputs, FMA), two Hd x Hd second layers, and the R + 1
    third-layer outputs: 2 * B * N^2 * (T * 2Hd + 2 * Hd * Hd + Hd * (R + 1))  (DESIGN.md 4.4)."""
    from egtr_amd import ops
    a, kw = args
    def fn():
        with torch.no_grad():  # as in the timed forward: the inference kernel, nothing saved for a backward
            return ops.relation_head(*a, **kw)

    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / iters
    gate_q, w2r, w3r = a[0], a[5], a[7]
    B, N, T = gate_q.shape
    Hd, R = w2r.shape[1], w3r.shape[0]
    flops = 2.0 * B * N * N * (T * 2 * Hd + 2 * Hd * Hd + Hd * (R + 1))
    return us, flops


def time_encoder_tail(dev, iters=100):
    """One encoder layer's tail at S = 12 537 rows -- output projection + LayerNorm + FFN block (256 -> 1024 -> 256) +
    LayerNorm (as the model runs it: no position output) -- through egtr_encoder_tail_x6_f32 (csrc/ffn_x6.hip, one launch); algorithmic FLOPs =
    2 M (256 * 256 + 2 * 256 * 1024)."""
    from egtr_amd import ops
    M, D, F = 12537, 256, 1024
    g = torch.Generator(device="cpu").manual_seed(0)
    mods = [torch.nn.Linear(D, D), torch.nn.LayerNorm(D), torch.nn.Linear(D, F), torch.nn.Linear(F, D), torch.nn.LayerNorm(D)]
    mods = [m.to(dev) for m in mods]
    ctx, hid = (torch.randn(M, D, generator=g).to(dev) for _ in range(2))
    with torch.no_grad():
        if not ops.encoder_tail_fused_supported(ctx, *mods):
            return None, None
        for _ in range(5):
            ops.encoder_tail_fused(ctx, hid, *mods)
        torch.cuda.synchronize()
        best = None     # the median of three batches: one batch was once seen 5x slower than its neighbours (a box hiccup)
        times = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(max(1, iters // 3)):
                ops.encoder_tail_fused(ctx, hid, *mods)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3 / max(1, iters // 3))
        best = sorted(times)[1]
    return best, 2.0 * M * (D * D + 2 * D * F)


def _time_us(fn, iters=60):
    """Median of three event-timed batches of `fn` on the current stream (us per call)."""
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(max(1, iters // 3)):
            fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / max(1, iters // 3))
    return sorted(times)[1]


def time_backbone_kernels(dev):
    """The hand-written backbone kernels of the fp32 channels-last route at the bench shapes (600x1000, bs 1), stand-alone:
    [(kernel, launch description, us, algorithmic flops, algorithmic bytes)] -- the 3x3 convolution of a layer-3 bottleneck
    (38x63, C = 256; csrc/conv3x3_x6.hip), the tail of a layer-1 bottleneck (37 500 rows, 64 -> 256; csrc/conv_tail_x6.hip)
    and the fused stem (csrc/stem_x6.hip)."""
    from egtr_amd import ops
    out = []
    with torch.no_grad():
        g = torch.Generator(device="cpu").manual_seed(0)
        x = torch.randn(1, 256, 38, 63, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
        w = (torch.randn(256, 256, 3, 3, generator=g) / 48.0).to(dev)
        if ops.conv3x3_supported(x, 256):
            wxs = ops.conv3x3_weights(w)
            us = _time_us(lambda: ops.conv3x3(x, wxs, 256))
            out.append(("conv3x3_x6_ksplit_kernel<256, 128, 1>", "3x3 convolution of a layer-3 bottleneck: 38x63 pixels, 256 -> 256 "
                        "channels (5 such launches per forward; 16 own 3x3 convolutions in all)", us,
                        2.0 * 38 * 63 * 9 * 256 * 256, 4.0 * (2 * 38 * 63 * 256 + 9 * 256 * 256)))
        M, K, N = 37500, 64, 256
        a, sc = torch.randn(M, K, generator=g).to(dev), torch.randn(M, N, generator=g).to(dev)
        w3 = (torch.randn(N, K, generator=g) / 8.0).to(dev)
        b2, b3 = torch.randn(K, generator=g).to(dev), torch.randn(N, generator=g).to(dev)
        if ops.conv1x1_tail_supported(a, N):
            w3xs = ops.xs_split(w3, weights=True)
            us = _time_us(lambda: ops.conv1x1_tail(a, b2, w3xs, b3, sc, N))
            out.append(("conv_tail_x6_kernel<32, 1, 4, 4>", "tail of a layer-1 bottleneck: shift + ReLU, 1x1 convolution 64 -> 256, "
                        "shift + shortcut + ReLU over 37 500 pixel rows (3 such launches per forward; 16 tails in all)", us,
                        2.0 * M * K * N, 4.0 * M * (K + 2 * N)))
        xs_ = torch.randn(1, 3, H_IMG, W_IMG, generator=g).to(dev)
        ws = (torch.randn(64, 3, 7, 7, generator=g) / 12.0).to(dev)
        bs = torch.randn(64, generator=g).to(dev)
        if ops.stem_fused_supported(xs_, ws):
            wsx = ops.stem_weights(ws)
            us = _time_us(lambda: ops.stem_fused(xs_, wsx, bs))
            out.append(("stem_x6_kernel", "stem: 7x7/2 convolution 3 -> 64 + shift + ReLU + 3x3/2 max-pool, 600x1000 -> 150x250x64 "
                        "channels-last (1 launch per forward)", us, 2.0 * 300 * 500 * 147 * 64,
                        4.0 * (3 * H_IMG * W_IMG + 150 * 250 * 64)))
    return out


def time_split_gemm(dev, iters=100):
    """The split-bf16 tile GEMM as the encoder layer launches it since round 3 (csrc/gemm_split.hip, one grouped launch):
    value projection 256 -> 256 of the layer input and sampling-offset / attention-weight projection 256 -> 384 of
    (input + position rows, added on load), S = 12 537 rows; algorithmic FLOPs = 2 M K (256 + 384)."""
    from egtr_amd import ops
    M, K = 12537, 256
    g = torch.Generator(device="cpu").manual_seed(0)
    x, pos = torch.randn(M, K, generator=g).to(dev), torch.randn(M, K, generator=g).to(dev)
    ws = [(torch.randn(n, K, generator=g) / K ** 0.5).to(dev) for n in (256, 384)]
    bs = [torch.randn(n, generator=g).to(dev) for n in (256, 384)]
    wts = [ops.gemm_split_weights(w) for w in ws]
    outs = [torch.empty(M, n, device=dev) for n in (256, 384)]

    def fn():
        ops.linear_split_bf16_grouped([dict(x=x, wt=wts[0], N=256, b=bs[0], out=outs[0]),
                                       dict(x=x, wt=wts[1], N=384, b=bs[1], out=outs[1], pos=pos)])

    with torch.no_grad():
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters, 2.0 * M * K * (256 + 384)


def time_msda_kernel(args, fused, iters=200, keep_bits=None):
    """Average duration of the encoder MSDA kernel: `iters` back-to-back launches through the C ABI on torch's
    current stream, bracketed by HIP events recorded on that same stream."""
    from egtr_amd.load_custom import load_hip_kernels
    k = load_hip_kernels()
    value, loc = args[0], args[3]
    if fused and value.dtype == torch.bfloat16:
        fn = lambda: k.ms_deform_attn_forward_fused_bf16(*args[:6], args[7], keep_bits=keep_bits)  # noqa: E731
    else:
        fn = ((lambda: k.ms_deform_attn_forward_fused(*args, keep_bits=keep_bits)) if fused
              else (lambda: k.ms_deform_attn_forward(*args)))
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / iters
    B, S, M, D = value.shape
    Lq = loc.shape[1]
    e = value.element_size()
    el, ea = loc.element_size(), args[4].element_size()
    # value S*256*e (capped by the gathered bytes) + loc Lq*256*e_loc + attn Lq*128*e_attn + out Lq*256*e
    # (the fused entry reads raw offsets / logits of exactly the loc / attn sizes -- bf16 in the bf16 model: until round 5
    # this line priced them at 4 bytes and overstated the bf16 launch's bytes by 43 %; its reference points, Lq*L*8 B, are
    # not counted)
    alg = B * (min(S * M * D * e, Lq * M * 16 * 4 * D * e) + Lq * M * 32 * el + Lq * M * 16 * ea + Lq * M * D * e)
    return us, alg


def time_decoder_layer(model, pv, pm, forwards=20):
    """Average duration of one egtr_decoder_layer_f32 launch (csrc/dec_layer.hip): HIP events on torch's current stream
    around every launch of `forwards` eager forwards; (us, launches per forward) or (None, 0) when the cluster path is off."""
    from egtr_amd import _lib
    lib = _lib.lib()
    raw = lib.egtr_decoder_layer_f32
    evs = []

    def wrapped(stream, a):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        st = raw(stream, a)
        e1.record()
        evs.append((e0, e1))
        return st

    lib.egtr_decoder_layer_f32 = wrapped
    try:
        with torch.no_grad():
            for _ in range(forwards):
                model(pixel_values=pv, pixel_mask=pm, output_attentions=False, output_attention_states=True)
        torch.cuda.synchronize()
    finally:
        lib.egtr_decoder_layer_f32 = raw
    if not evs:
        return None, 0
    ts = sorted(a.elapsed_time(b) * 1e3 for a, b in evs[len(evs) // 4:])
    return ts[len(ts) // 2], len(evs) // forwards


def time_lib_entries(names, run, forwards=3):
    """Median duration (us) of the launches of the C entries `names` during `forwards` eager calls of `run()`: HIP events on
    torch's current stream around every call; {name: (us, launches per forward)} for the entries that were called."""
    from egtr_amd import _lib
    lib = _lib.lib()
    raws, evs = {}, {n: [] for n in names}

    def wrap(name, raw):
        def wrapped(*a):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            st = raw(*a)
            e1.record()
            evs[name].append((e0, e1))
            return st
        return wrapped

    for n in names:
        raws[n] = getattr(lib, n)
        setattr(lib, n, wrap(n, raws[n]))
    try:
        with torch.no_grad():
            for _ in range(forwards):
                run()
        torch.cuda.synchronize()
    finally:
        for n, r in raws.items():
            setattr(lib, n, r)
    out = {}
    for n, ev in evs.items():
        if ev:
            ts = sorted(a.elapsed_time(b) * 1e3 for a, b in ev[len(ev) // 3:])
            out[n] = (ts[len(ts) // 2], len(ev) // forwards)
    return out


def time_l1_gather_ceiling(iters=2000, reps=3):
    """The vector-L1 gather ceiling of THIS GPU in THIS run (GB/s): csrc/probe_l1.hip through the test ABI
    (include/egtr_hip_test.h) -- 512 workgroups, every 8-lane group of a wave reading a different L1-resident 128-byte line
    with 16 B per lane, i.e. the MSDA gather's access shape with every miss removed; HIP events on the launch stream."""
    import ctypes
    from egtr_amd import _lib
    from egtr_amd.load_custom import _stream
    h = _lib.lib()
    h.egtr_test_l1_gather_buffer_bytes.argtypes, h.egtr_test_l1_gather_buffer_bytes.restype = [ctypes.c_int], ctypes.c_longlong
    h.egtr_test_l1_gather_bandwidth.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                ctypes.c_void_p]
    h.egtr_test_l1_gather_bandwidth.restype = ctypes.c_int
    blocks = 512
    buf = torch.zeros(h.egtr_test_l1_gather_buffer_bytes(blocks) // 4, dtype=torch.float32, device="cuda")
    out = torch.zeros(256, dtype=torch.float32, device="cuda")
    moved = ctypes.c_longlong(0)
    best = None
    for _ in range(reps + 1):     # first launch: warm-up
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(h.egtr_test_l1_gather_bandwidth(_stream(), buf.data_ptr(), out.data_ptr(), iters, blocks,
                                                   ctypes.byref(moved)), "egtr_test_l1_gather_bandwidth")
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        best = ms if best is None else min(best, ms)
    return moved.value / (best * 1e-3) / 1e9


def msda_kernel_name(fused):
    from egtr_amd import ops
    name = getattr(ops, "MSDA_ENCODER_KERNEL", "msda_fwd_q64_f32")
    return name + ("<fused prologue>" if fused else "")


def logit_parity(model, ref, pv, pm):
    """max |product - oracle| on class logits, boxes and the PRE-sigmoid relation / connectivity logits (egtr:402-416).
    The frequency bias (a table lookup by argmax class, -29 for unseen triplets) is removed from both sides with each
    side's own argmax, so a class near-tie cannot masquerade as a relation-logit error."""
    with torch.no_grad():
        outputs = model.model(pv, pixel_mask=pm, output_attentions=False, output_hidden_states=True,
                              output_attention_states=True, return_dict=True)
        logits, boxes, _, _, rel, conn, _, _ = model._heads(outputs, want_gate_mean=False)

    def unbias(rel_, logits_, table):
        node = logits_.argmax(-1)
        return rel_ - torch.stack([table[n][:, n] for n in node])

    td = model.triplet_dist
    got_rel = unbias(rel, logits, td).cpu() if model.config.use_freq_bias else rel.cpu()
    ref_rel = unbias(ref["rel_logits"], ref["logits"], td.cpu()) if model.config.use_freq_bias else ref["rel_logits"]
    return {"class_logits": float((logits.cpu() - ref["logits"]).abs().max()),
            "boxes": float((boxes.cpu() - ref["pred_boxes"]).abs().max()),
            "rel_logits": float((got_rel - ref_rel).abs().max()),
            "conn_logits": float((conn.cpu() - ref["conn_logits"]).abs().max())}


def _train_switch(name):
    return os.environ.get(name, "1") != "0"


def usable_cores():
    """Cores this process may actually use: affinity mask, capped by the cgroup CPU quota if one is set
    (os.cpu_count() reports the whole machine and badly oversubscribes inside a container)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(float(quota) / float(period))))
    except Exception:
        pass
    return max(1, n)


def cpu_baseline(model, cfg_dict, budget_s=20.0, max_images=8):
    """The CPU oracle (reference fallback semantics: per-level F.grid_sample MSDA, materialised relation_source)
    on the host cores, same workload, bounded sample: one warm-up image, then as many images as fit in
    ~budget_s seconds (at least 1, at most max_images)."""
    from oracle import detr as O
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    cfg = dict(d_model=256, num_feature_levels=4, encoder_attention_heads=8)
    cfg.update(cfg_dict)
    torch.manual_seed(1)
    pv = torch.randn(1, 3, H_IMG, W_IMG)
    pm = torch.ones(1, H_IMG, W_IMG, dtype=torch.long)
    with torch.no_grad():
        t0 = time.perf_counter()
        out = O.sgg_forward(sd, cfg, pv, pm, backbone=O.resnet50_backbone)  # warm-up (also sizes the sample)
        warm = time.perf_counter() - t0
        n = int(min(max_images, max(1, budget_s // max(warm, 1e-3))))
        t0 = time.perf_counter()
        for _ in range(n):
            out = O.sgg_forward(sd, cfg, pv, pm, backbone=O.resnet50_backbone)
        dt = time.perf_counter() - t0
    return n / dt, n, out, pv, pm


def make_targets(batch, cfg, dev, seed):
    """Synthetic SGG labels: T ~ U{5..30} boxes per image, 3T random relations in the dense [N,N,R]."""
    import numpy as np
    rng = np.random.RandomState(seed)
    N, C, R = cfg.num_queries, cfg.num_labels, cfg.num_rel_labels
    out = []
    for _ in range(batch):
        T = int(rng.randint(5, 31))
        boxes = np.concatenate([rng.uniform(0.2, 0.8, (T, 2)), rng.uniform(0.05, 0.25, (T, 2))], 1).astype(np.float32)
        rel = np.zeros((N, N, R), dtype=np.float32)
        so = rng.randint(0, T, (3 * T, 2))
        pr = rng.randint(0, R, (3 * T,))
        keep = so[:, 0] != so[:, 1]
        rel[so[keep, 0], so[keep, 1], pr[keep]] = 1.0
        out.append({"class_labels": torch.from_numpy(rng.randint(0, C, (T,)).astype(np.int64)).to(dev),
                    "boxes": torch.from_numpy(boxes).to(dev), "rel": torch.from_numpy(rel).to(dev)})
    return out


class MsdaBwdProbe:
    """Remembers the operands of the most recent encoder-shaped (Lq == S) MSDA backward launch."""

    def __init__(self):
        from egtr_amd import load_custom
        self._cls = load_custom._MultiScaleDeformableAttention
        self._orig = self._cls.ms_deform_attn_backward
        self.args = None

    def __enter__(self):
        probe, orig = self, self._orig

        def bwd(value, shapes, lsi, loc, attn, grad_out, step):
            if loc.shape[1] == value.shape[1]:
                probe.args = (value, shapes, lsi, loc, attn, grad_out, step)
            return orig(value, shapes, lsi, loc, attn, grad_out, step)

        self._cls.ms_deform_attn_backward = staticmethod(bwd)
        return self

    def __exit__(self, *a):
        self._cls.ms_deform_attn_backward = staticmethod(self._orig)


def time_msda_backward(args, iters=50):
    """Average duration of the encoder-shaped MSDA backward (both kernels: grad_loc / grad_attn by the wave-per-query
    kernel, grad_value by the matrix-core tile kernel; the zero-fill of grad_value is part of the call) and its algorithmic
    bytes: forward reads + grad_out + 2 x grad_value (zero-init + accumulate) + grad_loc + grad_attn."""
    from egtr_amd.load_custom import load_hip_kernels
    k = load_hip_kernels()
    for _ in range(5):
        k.ms_deform_attn_backward(*args)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        k.ms_deform_attn_backward(*args)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / iters
    value, loc = args[0], args[3]
    B, S, M, D = value.shape
    Lq = loc.shape[1]
    fwd = min(S * M * D * 4, Lq * M * 16 * 4 * D * 4) + Lq * M * 32 * 4 + Lq * M * 16 * 4
    alg = B * (fwd + Lq * M * D * 4 + 2 * S * M * D * 4 + Lq * M * 32 * 4 + Lq * M * 16 * 4)
    return us, alg


def cpu_train_baseline(model, cfg_dict, labels_cpu, budget_s=25.0):
    """The CPU oracle's train step on the host cores: forward (reference fallback semantics) + Hungarian matching + SGG
    loss + autograd backward of ONE 600x1000 image per iteration (bounded sample of the bs = 4 step)."""
    from oracle import detr as O
    from oracle import loss as OL
    sd = {k: v.detach().cpu().clone().requires_grad_(v.is_floating_point()) for k, v in model.state_dict().items()}
    cfg = dict(d_model=256, num_feature_levels=4, encoder_attention_heads=8, bbox_cost=5, giou_cost=2,
               bbox_loss_coefficient=5, giou_loss_coefficient=2, focal_alpha=0.25)
    cfg.update(cfg_dict)
    cfg["dropout"] = 0.0
    torch.manual_seed(1)
    pv = torch.randn(1, 3, H_IMG, W_IMG)
    pm = torch.ones(1, H_IMG, W_IMG, dtype=torch.long)
    n, t0 = 0, time.perf_counter()
    while True:
        out = O.sgg_forward(sd, cfg, pv, pm, backbone=O.resnet50_backbone)
        total, _, _, _ = OL.sgg_loss(out, labels_cpu[:1], cfg, training=True)
        total.backward()
        n += 1
        dt = time.perf_counter() - t0
        if dt > budget_s or n >= 4:
            break
    return n / dt, n


def train_bench(args, world, rank, dev, dist, emit=True):
    """Train-step throughput (BASELINE configs[2] shape: 600x1000, N=200, VG heads, fp32, batch 4/GPU, DDP over
    RCCL when world > 1, accumulate 1 so every step carries the gradient all-reduce).  Secondary metric."""
    from egtr_amd.runtime import DataParallelTrainer, configure_optimizers
    batch = args.batch if args.batch > 1 else 4
    model, cfg, cfg_dict = build_model(dev, {"dropout": 0.1})
    model.train()
    opt = configure_optimizers(model, lr=2e-6, lr_backbone=2e-7, lr_initialized=None, weight_decay=1e-4)
    tr = DataParallelTrainer(model, optimizer=opt, accumulate=1, clip=0.1, graph=bool(args.train_graph))
    torch.manual_seed(100 + rank)
    b = {"pixel_values": torch.randn(batch, 3, H_IMG, W_IMG, device=dev),
         "pixel_mask": torch.ones(batch, H_IMG, W_IMG, dtype=torch.long, device=dev),
         "labels": make_targets(batch, cfg, dev, 7 + rank)}
    with MsdaBwdProbe() as bprobe:
        for _ in range(args.warmup):
            tr.training_step(b)
        bwd_args = bprobe.args
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss, loss_dict, _ = tr.training_step(b)
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    tr.finalize()   # a cost matrix the device matcher refused in the last step would surface here (ValueError)
    dt, spread = rank_times(dt, args.steps, dist, dev, world)
    if emit and rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, output_arrays({"loss": loss, "loss_dict": loss_dict}))
    result = None
    if rank == 0:
        result = {
            "metric": "images/sec SGG train step (fwd + loss + bwd + grad all-reduce + AdamW), 600x1000, N=200",
            "value": round(world * batch * args.steps / dt, 3), "unit": "images/sec", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "final_loss": float(loss), "rccl_ranks": args.rccl_ranks, "rank_ms_per_step": spread,
            "config": {"workload": f"VG train step: ResNet-50, N=200, 6 enc/6 dec, bs={batch}/GPU fp32, DDP x{world} "
                                   "(BASELINE configs[2] shape)", "parallelism": f"dp{world}",
                       "token_linears": ("fp32 via bf16x6 operand split (forward, data and weight gradients)"
                                         if _train_switch("EGTR_TOKEN_LINEAR") and _train_switch("EGTR_GEMM_SPLIT_BF16")
                                         else "vendor fp32 GEMM"),
                       "training_nodes": ("round-4 autograd nodes: encoder layer, decoder value projections, dropout + add + "
                                          "LayerNorm, level geometry" if _train_switch("EGTR_ENCODER_TRAIN_FUSED")
                                          else "per-op composition (EGTR_ENCODER_TRAIN_FUSED=0)"),
                       "gemm_tuning": bool(args.tune_gemm), "miopen_find": bool(torch.backends.cudnn.benchmark)}}
        if args.full and bwd_args is not None and not args.no_kernel_probes:
            us, alg = time_msda_backward(bwd_args)
            ach = alg / (us * 1e-6) / 1e9
            bwd_kernel = "msda_bwd_q64_f32<no atomics> + msda_bwd_value_tile_f32"
            # HBM bytes of the pair from separate --pmc passes over the train command (tools/pmc_train.sh), batch 4
            bp, bp_src = newest_pmc("r*_msda_bwd_pmc.json", bwd_kernel) if batch == 4 else ({}, None)
            result["roofline"] = {"bound": "hbm", "kernel": bwd_kernel,
                                  "launch": f"encoder layer backward, B={batch}, Lq = S = 12537",
                                  "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                  "frac": round(ach / HBM_PEAK_GBS, 4), "traffic": bp.get("hbm_bytes_per_launch"),
                                  "traffic_source": bp_src, "l2_hit": bp.get("l2_hit"),
                                  "algorithmic_bytes_per_launch": alg, "avg_launch_us": round(us, 2)}
        if args.full and world == 1 and not args.no_cpu_baseline:
            ncores = usable_cores()
            torch.set_num_threads(ncores)
            labels_cpu = [{k: v.cpu() for k, v in t.items()} for t in b["labels"]]
            ips, nimg = cpu_train_baseline(model, cfg_dict, labels_cpu, args.cpu_budget)
            result["cpu_baseline"] = {"value": round(ips, 4), "unit": "images/sec", "cores": torch.get_num_threads(),
                                      "kind": "port", "sample": f"{nimg} single-image train iterations (oracle forward "
                                      "+ matcher + SGG loss + autograd backward, incl. ResNet-50) at 600x1000 / N=200"}
        if emit:
            print(json.dumps(result))
    if dist is not None and emit:
        dist.destroy_process_group()
    return result if rank == 0 else None


def stress_bench(dev, steps, warmup, batch=16):
    """BASELINE configs[4] shape on ONE GPU: 800x1333, N = 300 queries, 8 decoder layers, bf16 weights and activations,
    `batch` images per step (HIP-graph replay).  Returns the extra-key dict of the default bench line."""
    from egtr_amd.runtime import GraphedForward
    model, cfg, _ = build_model(dev, {"num_queries": 300, "decoder_layers": 8})
    model = model.to(torch.bfloat16).eval()
    torch.manual_seed(300)
    pv = torch.randn(batch, 3, 800, 1333, device=dev, dtype=torch.bfloat16)
    pm = torch.ones(batch, 800, 1333, dtype=torch.long, device=dev)
    fwd = GraphedForward(model, enabled=True, strict=True)
    with MsdaProbe() as probe, torch.no_grad():
        model(pixel_values=pv, pixel_mask=pm, output_attentions=False, output_attention_states=True,
              output_hidden_states=True)
        msda_args, fused, msda_bits = probe.args, probe.fused, probe.keep_bits
    with torch.no_grad():
        for _ in range(warmup):
            fwd(pv, pm)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fwd(pv, pm)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    out = {"metric": "images/sec end-to-end SGG forward, stress shape", "value": round(batch * steps / dt, 2),
           "unit": "images/sec", "ms_per_step": round(dt / steps * 1e3, 3), "steps": steps, "warmup": warmup,
           "dtype": "bf16", "n_gpus": 1,
           "config": {"workload": f"Stress: ResNet-50, 800x1333, N=300, 6 enc/8 dec, bf16, bs={batch}/GPU "
                                  "(BASELINE configs[4] shape on one GPU)", "hip_graph": bool(fwd.graphed),
                      "miopen_find": bool(torch.backends.cudnn.benchmark)}}
    if msda_args is not None:
        us, alg = time_msda_kernel(msda_args, fused, iters=50, keep_bits=msda_bits)
        ach = alg / (us * 1e-6) / 1e9
        out["roofline"] = {"bound": "hbm", "kernel": "msda_fwd_q32_bf16<fused prologue>" if fused else "msda_fwd_q32_bf16",
                           "launch": f"encoder layer, B={batch}, Lq = S = 22223, bf16 values",
                           "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                           "frac": round(ach / HBM_PEAK_GBS, 4), "traffic": None,
                           "algorithmic_bytes_per_launch": alg, "avg_launch_us": round(us, 2)}
        # memory counters of this launch from the newest separate rocprofv3 --pmc run over tools/stress_bench.py
        # (tools/profile_r05_all.sh): HBM-side bytes, L2 hit rate, bytes moved through the vector L1
        sp, sp_src = newest_pmc("r*_msda_bf16_pmc.json", out["roofline"]["kernel"])
        if sp:
            out["roofline"].update(traffic=sp.get("hbm_bytes_per_launch"), l2_hit=sp.get("l2_hit"),
                                   l1_gather_bytes=sp.get("l1_gather_bytes"), traffic_source=sp_src)
    # the bf16 matrix kernels of this forward, timed live (eager forwards, HIP events around each launch), priced against the
    # dense bf16 MFMA peak on their ALGORITHMIC flops; matrix-pipe busy from the newest profiles/r*_stress_mfma_pmc.json
    S = msda_args[0].shape[1] if msda_args is not None else 0
    times = time_lib_entries(["egtr_ffn_layernorm_bf16", "egtr_rel_head_forward_bf16p"],
                             lambda: model(pixel_values=pv, pixel_mask=pm, output_attentions=False,
                                           output_attention_states=True, output_hidden_states=False))
    busy = {}
    try:
        import glob
        paths = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_stress_mfma_pmc.json")), key=os.path.getmtime)
        if paths:
            busy = json.load(open(paths[-1]))
            busy["_src"] = "profiles/" + os.path.basename(paths[-1])
    except Exception:
        busy = {}
    kernels = []
    nq, T, R = cfg.num_queries, cfg.decoder_layers + 1, cfg.num_rel_labels if hasattr(cfg, "num_rel_labels") else 50
    specs = {
        "egtr_ffn_layernorm_bf16": ("ffn_bf16_kernel", f"encoder layer: fc1 + ReLU + fc2 + residual + LayerNorm (+ position rows), "
                                    f"M = {batch} x {S} rows, 256 -> {cfg.encoder_ffn_dim} -> 256",
                                    2.0 * batch * S * 256 * cfg.encoder_ffn_dim * 2),
        "egtr_rel_head_forward_bf16p": ("rel_head_fwd_bf16p", f"relation + connectivity heads, B = {batch}, N = {nq}, T = {T} slots",
                                        2.0 * batch * nq * nq * (2 * T * 512 + 2 * 256 * 256 + 256 * (R + 1))),
    }
    for entry, (kname, launch, flops) in specs.items():
        if entry in times:
            us, n = times[entry]
            tf = flops / (us * 1e-6) / 1e12
            e = {"bound": "mfma", "kernel": kname, "launch": f"{launch}; {n} launches per forward", "achieved": round(tf, 1),
                 "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(tf / MFMA_BF16_PEAK_TFLOPS, 4), "traffic": None,
                 "algorithmic_flops_per_launch": flops, "avg_launch_us": round(us, 1)}
            b = busy.get("kernels", {}).get(kname) if isinstance(busy, dict) else None
            if isinstance(b, dict) and b.get("source_sha256") is not None and b.get("source_sha256") == _source_hash(kname):
                e["mfma_busy"] = b.get("mfma_busy")
                e["mfma_busy_source"] = busy.get("_src")
            kernels.append(e)
    if kernels:
        out["roofline_kernels"] = ([out["roofline"]] if "roofline" in out else []) + kernels
    del fwd, model
    torch.cuda.empty_cache()
    return out


def _source_hash(kernel):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from kernel_source_hash import source_hash
        return source_hash(kernel)
    except Exception:
        return None


def newest_pmc(pattern, kernel):
    """The most recent profiles/<pattern> (rocprofv3 --pmc passes over this command, tools/pmc_passes.sh + tools/*_pmc.py)
    whose `kernel` field names the kernel that was just timed AND whose `source_sha256` equals the hash of that kernel's
    source files as they are in the tree now (tools/kernel_source_hash.py): a profile taken from an older version of the
    kernel is refused, whatever its label or file time says.  (dict, "file name (mtime, sources verified)") or ({}, None).
    Counters are collected in separate profiler runs, never inside the timed run, so the line says which file they come
    from."""
    import glob
    best = None
    want = _source_hash(kernel)
    for path in glob.glob(os.path.join(ROOT, "profiles", pattern)):
        try:
            d = json.load(open(path))
        except Exception:
            continue
        if d.get("kernel") != kernel:
            continue
        if want is None or d.get("source_sha256") != want:
            continue    # stale (or pre-round-6, unhashed) profile: not quoted
        m = os.path.getmtime(path)
        if best is None or m > best[0]:
            best = (m, path, d)
    if best is None:
        return {}, None
    return best[2], (f"profiles/{os.path.basename(best[1])} (mtime {time.strftime('%Y-%m-%d %H:%M', time.gmtime(best[0]))} UTC, "
                     f"kernel sources sha256 {want[:12]} verified)")


def mixed_shape_set(n_shapes=12, seed=0, min_size=600, max_size=1000):
    """Image shapes (H, W) as the reference's evaluation resize produces them (evaluate_egtr.py:165-175 ``--min_size 600
    --max_size 1000``: short side -> 600 unless the long side would exceed 1000, then long side = 1000): aspect ratios
    drawn with a fixed seed from U(1, 2), a quarter of them portrait; the bench's own 600x1000 is always in the set."""
    import numpy as np
    rng = np.random.RandomState(seed)
    shapes = [(H_IMG, W_IMG)]
    while len(shapes) < n_shapes:
        r = float(rng.uniform(1.0, 2.0))
        short, long_ = min_size, int(round(min_size * r))
        if long_ > max_size:
            short, long_ = int(round(max_size / r)), max_size
        hw = (long_, short) if rng.uniform() < 0.25 else (short, long_)
        if hw not in shapes:
            shapes.append(hw)
    return shapes


def mixed_shapes_leg(model, dev, fixed_value, n_shapes=12, stream=96, seed=0, tune_first_pass=True):
    """The reference's FPS loop on a stream of differently sized images (evaluate_egtr.py:26-36 over a dataloader), bs = 1:
    every distinct shape is captured once into its own HIP graph (egtr_amd.runtime.GraphedForward, LRU of 16) in an untimed
    first pass, then `stream` images (shapes drawn with a fixed seed, inputs resident in HBM) are timed as one region.
    ``tune_first_pass``: MIOpen find mode / TunableOp tuning stay as the headline run set them during the (untimed) first
    pass -- a new shape gets its convolution solvers and GEMM solutions picked once, like cudnn.benchmark does in the
    reference's loop -- and are switched off for the timed stream; False: off for the first pass too (heuristic picks)."""
    import numpy as np
    from egtr_amd.runtime import GraphedForward
    shapes = mixed_shape_set(n_shapes, seed)
    rng = np.random.RandomState(seed + 1)
    order = [int(i) for i in rng.randint(0, len(shapes), stream)]
    g = torch.Generator(device="cpu").manual_seed(seed + 2)
    inputs = [(torch.randn(1, 3, h, w, generator=g).to(dev), torch.ones(1, h, w, dtype=torch.long, device=dev))
              for (h, w) in shapes]
    bench_find = torch.backends.cudnn.benchmark
    tun = None
    try:
        import torch.cuda.tunable as tun
        tuning_was = tun.tuning_is_enabled()
        tun.tuning_enable(False)
    except Exception:
        tun = None
    torch.backends.cudnn.benchmark = bench_find and tune_first_pass
    budget = None
    if tun is not None and tune_first_pass:
        tun.tuning_enable(tuning_was)
        try:    # a third of TunableOp's default budget per candidate (30 ms / 100 iterations): eleven new image shapes x ~25
            # GEMM shapes each are tuned in this pass, and the default bench run has to stay within minutes
            budget = (tun.get_max_tuning_duration(), tun.get_max_tuning_iterations())
            tun.set_max_tuning_duration(10)
            tun.set_max_tuning_iterations(20)
        except Exception:
            budget = None
    try:
        fwd = GraphedForward(model, enabled=True, strict=True, max_graphs=16)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            for pv, pm in inputs:          # first pass: two eager warm-up runs + capture per shape
                fwd(pv, pm)
        torch.cuda.synchronize()
        first_pass_s = time.perf_counter() - t0
        torch.backends.cudnn.benchmark = False
        if tun is not None:
            tun.tuning_enable(False)
            if budget is not None:
                tun.set_max_tuning_duration(budget[0])
                tun.set_max_tuning_iterations(budget[1])
        captures = fwd.captures
        with torch.no_grad():
            for i in order[:8]:
                fwd(*inputs[i])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in order:
                fwd(*inputs[i])
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
    finally:
        torch.backends.cudnn.benchmark = bench_find
        if tun is not None:
            tun.tuning_enable(tuning_was)
    pixels = sum(shapes[i][0] * shapes[i][1] for i in order) / len(order)
    value = len(order) / dt
    return {"metric": "images/sec end-to-end SGG, bs=1, stream of differently sized images (HIP graph per shape)",
            "value": round(value, 2), "unit": "images/sec", "ms_per_image": round(dt / len(order) * 1e3, 4),
            "images": len(order), "distinct_shapes": len(shapes), "shapes_hw": [list(hw) for hw in shapes],
            "graphs_captured": captures, "recaptures_in_timed_region": fwd.captures - captures,
            "first_pass_s": round(first_pass_s, 3), "mean_pixels_vs_600x1000": round(pixels / (H_IMG * W_IMG), 4),
            "vs_fixed_shape": round(value / fixed_value, 4) if fixed_value else None,
            "tuning": ("first pass: MIOpen find / TunableOp as in the headline run; timed stream: off" if tune_first_pass
                       else "MIOpen find / TunableOp tuning off for the new shapes")}


def eager_leg(model, pv, pm, iters=30):
    """The same bs = 1 forward WITHOUT graph replay (what a caller gets from a plain ``model(...)`` call, and what every new
    shape costs before its graph exists): eager launches, synchronised at both ends."""
    with torch.no_grad():
        for _ in range(5):
            model(pixel_values=pv, pixel_mask=pm, output_attentions=False, output_attention_states=True,
                  output_hidden_states=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            model(pixel_values=pv, pixel_mask=pm, output_attentions=False, output_attention_states=True,
                  output_hidden_states=True)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    return {"value": round(pv.shape[0] * iters / dt, 2), "unit": "images/sec", "ms_per_step": round(dt / iters * 1e3, 4),
            "iters": iters, "launch": "eager (no HIP graph), 600x1000, bs=%d" % pv.shape[0]}


def batched_leg(model, dev, batch=8, steps=10, warmup=3, find=True):
    """The same fp32 model in THROUGHPUT mode: `batch` 600x1000 images per forward (HIP-graph replay).  Not the headline -- the
    reference's FPS path is bs = 1 (evaluate_egtr.py:26-36, BASELINE configs[1]) -- but what one GPU delivers when latency is
    not the constraint: the MSDA launch is long enough to sit at its L1 floor, the token GEMMs fill their last tile round."""
    from egtr_amd.runtime import GraphedForward
    torch.manual_seed(200)
    pv = torch.randn(batch, 3, H_IMG, W_IMG, device=dev)
    pm = torch.ones(batch, H_IMG, W_IMG, dtype=torch.long, device=dev)
    fwd = GraphedForward(model, enabled=True, strict=True)
    # MIOpen find mode for the batched convolution shapes (`find`; the heuristic picks vary from run to run and cost up to 3 ms
    # of the 17.4: profiles/r06_batched_bs8_breakdown_find{0,1}.txt), heuristic GEMM picks (TunableOp tuning of the batched shapes
    # cost ~60 s of the default run for 3 %)
    find_was = torch.backends.cudnn.benchmark
    torch.backends.cudnn.benchmark = bool(find)
    tun = None
    try:
        import torch.cuda.tunable as tun
        tuning_was = tun.tuning_is_enabled()
        tun.tuning_enable(False)
    except Exception:
        tun = None
    try:
        with torch.no_grad():
            for _ in range(warmup):
                fwd(pv, pm)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                fwd(pv, pm)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
    finally:
        torch.backends.cudnn.benchmark = find_was
        if tun is not None:
            tun.tuning_enable(tuning_was)
    return {"metric": "images/sec end-to-end SGG, 600x1000, fp32, throughput mode", "value": round(batch * steps / dt, 2),
            "unit": "images/sec", "images_per_step": batch, "ms_per_step": round(dt / steps * 1e3, 3), "steps": steps,
            "warmup": warmup, "miopen_find": bool(find),
            "note": "extra information; the headline stays bs = 1 (the reference's FPS path); heuristic GEMM picks"}


GRAD_BYTES_FP32 = 165 * 1000 * 1000   # ~165 MB of fp32 gradients per optimizer step (42.5 M parameters)


def time_allreduce(dist, dev, nbytes=GRAD_BYTES_FP32, iters=10):
    """A bare all-reduce of `nbytes` of fp32 over the process group (RCCL over xGMI on GPUs; gloo in the CPU launch test),
    average ms per call -- device events on the GPU, wall clock on the CPU.  The per-link floor for 165 MB on an 8-GPU ring
    is ~1.9 ms; DDP overlaps its buckets with backward, so the step pays less than this."""
    t = torch.ones(nbytes // 4, dtype=torch.float32, device=dev)
    for _ in range(2):
        dist.all_reduce(t)
    if dev.type == "cuda":
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        dist.barrier()
        e0.record()
        for _ in range(iters):
            dist.all_reduce(t)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters
    dist.barrier()
    t0 = time.perf_counter()
    for _ in range(iters):
        dist.all_reduce(t)
    return (time.perf_counter() - t0) / iters * 1e3


def ddp_train_leg(args, world, rank, dev, dist):
    """world > 1: a short DDP train loop (BASELINE configs[2]: bs 4 per GPU, accumulate 1 so that EVERY step carries the
    bucketed gradient all-reduce over RCCL) on all ranks, plus the bare 165 MB all-reduce beside it.  Rank 0 gets the dict
    that goes into the JSON line as `train_step_ddp` (schema: DESIGN.md 5); the other ranks get None."""
    import copy
    targs = copy.copy(args)
    targs.mode, targs.batch, targs.steps, targs.warmup = "train", 4, max(2, args.extra_steps), 5
    targs.no_cpu_baseline, targs.no_kernel_probes = True, True
    find_was = torch.backends.cudnn.benchmark
    torch.backends.cudnn.benchmark = False      # MIOpen find mode: no gain for the train step
    try:
        leg = train_bench(targs, world, rank, dev, dist, emit=False)
    finally:
        torch.backends.cudnn.benchmark = find_was
    ar_ms = time_allreduce(dist, dev)
    if rank != 0 or leg is None:
        return None
    keep = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "scaling", "dtype", "final_loss",
            "rccl_ranks", "rank_ms_per_step")
    out = {k: leg[k] for k in keep if k in leg}
    out["config"] = leg.get("config")
    out["allreduce_ms"] = round(ar_ms, 4)
    out["allreduce_bytes"] = GRAD_BYTES_FP32
    out["allreduce_busbw_GBs"] = round(2 * (world - 1) / world * GRAD_BYTES_FP32 / (ar_ms * 1e-3) / 1e9, 2)
    return out


def rank_times(dt, steps, dist, dev, world):
    """(max-over-ranks seconds, {"per_rank_ms_per_step": [...], "min", "max", "slowest_rank"}): every rank's own time for the
    timed region -- `value` uses the MAX (the contract), the spread shows a straggler that the one number would hide."""
    if dist is None:
        ms = dt / steps * 1e3
        return dt, {"per_rank_ms_per_step": [round(ms, 4)], "min": round(ms, 4), "max": round(ms, 4), "slowest_rank": 0}
    t = torch.tensor([dt], device=dev, dtype=torch.float64)
    all_t = [torch.zeros_like(t) for _ in range(world)]
    dist.all_gather(all_t, t)
    per = [float(x.item()) / steps * 1e3 for x in all_t]
    return max(float(x.item()) for x in all_t), {"per_rank_ms_per_step": [round(v, 4) for v in per], "min": round(min(per), 4),
                                                  "max": round(max(per), 4), "slowest_rank": per.index(max(per))}


def newest_mfma_busy():
    """{kernel name: matrix-pipe busy fraction} from the most recent profiles/r*_x6_mfma_pmc.json (tools/mfma_busy.py over
    separate rocprofv3 --pmc passes: SQ_VALU_MFMA_BUSY_CYCLES / (4 SIMDs x SQ_BUSY_CU_CYCLES)), and its provenance string."""
    import glob
    best = None
    for path in glob.glob(os.path.join(ROOT, "profiles", "r*_x6_mfma_pmc.json")):
        try:
            d = json.load(open(path))
        except Exception:
            continue
        m = os.path.getmtime(path)
        if best is None or m > best[0]:
            best = (m, path, d)
    if best is None:
        return {}, None
    return ({k: v.get("mfma_busy") for k, v in best[2].get("kernels", {}).items()
             if v.get("source_sha256") is not None and v.get("source_sha256") == _source_hash(k)},   # stale entries dropped
            f"profiles/{os.path.basename(best[1])} (mtime {time.strftime('%Y-%m-%d %H:%M', time.gmtime(best[0]))} UTC)")


def _free_port():
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def launch_ranks(n):
    """`python bench.py --gpus N` without a torchrun environment: start N ranks (one process per GPU) as a CHILD
    `torch.distributed.run` -- the reference's Trainer(gpus=N, strategy=DDPStrategy(...)) (train_egtr.py:770-779) in
    launcher form.  Called before this process has made any GPU call (a process that has initialised the GPU must
    never be replaced or forked into workers); the parent only waits and returns the child's exit code."""
    import subprocess
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // n)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def rccl_world_check(dist, dev):
    """A real all-reduce over the process group: every rank contributes 1, so the sum is the number of ranks that
    actually took part in a collective (RCCL on GPUs, gloo in the CPU launch test)."""
    t = torch.ones(1, device=dev)
    dist.all_reduce(t)
    return int(t.item())


def launch_check(args):
    """--launch-check: rendezvous + one all-reduce + the JSON line, without the model (tests/test_distributed_cpu.py
    runs `bench.py --gpus 2 --launch-check` on CPU under gloo; on a GPU box it exercises RCCL)."""
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    n_dev = torch.cuda.device_count()
    backend = "nccl" if n_dev >= world and n_dev > 0 else "gloo"
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    if backend == "nccl":
        lr = int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(lr)
        dev = torch.device("cuda", lr)
        dist.init_process_group("nccl", device_id=dev)
    else:
        dev = torch.device("cpu")
        dist.init_process_group("gloo")
    ranks = rccl_world_check(dist, dev)
    dist.barrier()
    # the bare all-reduce timer of the world > 1 DDP leg (`train_step_ddp.allreduce_ms`), on a small buffer under gloo
    nbytes = GRAD_BYTES_FP32 if backend == "nccl" else 4 * 1000 * 1000
    ar_ms = time_allreduce(dist, dev, nbytes=nbytes, iters=3)
    if rank == 0:
        print(json.dumps({"launch_check": True, "n_gpus": dist.get_world_size(), "rccl_ranks": ranks,
                          "backend": backend, "requested_gpus": args.gpus,
                          "train_step_ddp": {"allreduce_ms": round(ar_ms, 4), "allreduce_bytes": nbytes,
                                             "note": "launch check: collective only, no model"}}))
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=1, help="images per step per GPU (reference FPS path: 1)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline and parity check")
    ap.add_argument("--no-kernel-probes", action="store_true",
                    help="--full --mode train: skip the stand-alone timing loop of the MSDA backward after the timed steps (used "
                         "for rocprofv3 traces of the steady-state step)")
    ap.add_argument("--cpu-budget", type=float, default=20.0, help="--full: seconds of CPU-baseline work (bounded sample)")
    ap.add_argument("--graph", type=int, default=1, help="replay the forward from a HIP graph (0 = eager launches)")
    ap.add_argument("--train-graph", type=int, default=0,
                    help="--mode train, one GPU: replay forward / backward of the static part of the step from HIP "
                         "graphs (measured slower than eager launches: the step is GPU-bound, DESIGN.md 4.7)")
    ap.add_argument("--tune-gemm", type=int, default=1,
                    help="1 = PyTorch TunableOp picks the fastest rocBLAS / hipBLASLt solution per GEMM shape during "
                         "warm-up (egtr_amd.runtime.enable_gemm_tuning)")
    ap.add_argument("--miopen-find", type=int, default=-1,
                    help="1 = torch.backends.cudnn.benchmark (MIOpen find mode for the backbone convolutions during "
                         "warm-up: 250 -> 261 images/s); -1 = on for --mode infer, off for --mode train (no gain there)")
    ap.add_argument("--mode", default="infer", choices=["infer", "train"],
                    help="infer = BASELINE configs[1] (default, the headline metric); train = configs[2]-style train "
                         "step (forward + SGG loss + backward + DDP all-reduce + AdamW), batch 4/GPU unless --batch")
    ap.add_argument("--extras", type=int, default=1,
                    help="--full --mode infer on one GPU: after the timed region also run a short bs = 4 train loop and the bf16 "
                         "stress forward and append them to the JSON line as `train_step` / `stress_bf16` (0 = skip)")
    ap.add_argument("--extra-steps", type=int, default=8, help="--full: timed steps of each extra workload")
    ap.add_argument("--mixed-tune", type=int, default=1,
                    help="mixed_shapes leg: 1 = the untimed first pass keeps MIOpen find / TunableOp tuning on for the new "
                         "shapes (what the reference's cudnn autotuning does on a new shape), 0 = heuristic picks")
    ap.add_argument("--strict-fast-path", type=int, default=1,
                    help="1: raise when a call falls off a HIP fast path (egtr_amd.ops.FALLBACKS); 0: count and warn")
    ap.add_argument("--launch-check", action="store_true",
                    help="only rendezvous, all-reduce and print n_gpus / rccl_ranks (launcher self-test, runs on CPU)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline also run the kernel roofline probes, the CPU baseline + parity check and the "
                         "other workloads (--extras); a plain run only times the --steps steps")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the outputs of the last timed step as DIR/<name>.npy (float32 / float64, <= 60 MB in all)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(launch_ranks(args.gpus))  # nothing above this line touches the GPU
    if args.launch_check:
        return launch_check(args)
    from egtr_amd.runtime import private_miopen_db
    private_miopen_db()   # N ranks: one MIOpen user database / kernel cache directory per rank (no-op for one rank)
    if args.miopen_find == 1 or (args.miopen_find < 0 and args.mode == "infer"):
        from egtr_amd.runtime import enable_conv_tuning
        enable_conv_tuning()
    if args.tune_gemm:
        from egtr_amd.runtime import enable_gemm_tuning
        enable_gemm_tuning()

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the HIP path has no CPU fallback)")
    # EGTR_BENCH_BACKEND=gloo: the whole world > 1 code path (replica inference, DDP train leg, all-reduce timer) on a box with
    # FEWER GPUs than ranks -- ranks share devices (local_rank % device_count) and the collectives go through gloo.  A
    # self-test of the bench's own plumbing (this pool hands out one-GPU boxes), never a performance number: the line says so.
    backend = os.environ.get("EGTR_BENCH_BACKEND", "nccl")
    local_rank = local_rank % max(1, torch.cuda.device_count()) if backend != "nccl" else local_rank
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)  # RCCL on ROCm
        else:
            dist.init_process_group(backend)
    if rank == 0 and world != args.gpus:
        print(f"[bench] --gpus {args.gpus} but the launcher started WORLD_SIZE = {world}: reporting n_gpus = {world}",
              file=sys.stderr)
    args.rccl_ranks = rccl_world_check(dist, dev) if dist is not None else 1
    # a call that leaves a hand-written kernel for an ATen composition is an ERROR here (egtr_amd.ops.note_fallback): a
    # benchmark number must not come from a silently deoptimised path.  --strict-fast-path 0: count and warn instead.
    from egtr_amd import ops as _ops
    _ops.STRICT_FAST_PATH = bool(args.strict_fast_path)

    if args.mode == "train":
        return train_bench(args, world, rank, dev, dist)
    model, cfg, cfg_dict = build_model(dev)
    torch.manual_seed(100 + rank)
    pv = torch.randn(args.batch, 3, H_IMG, W_IMG, device=dev)
    pm = torch.ones(args.batch, H_IMG, W_IMG, dtype=torch.long, device=dev)

    from egtr_amd.runtime import GraphedForward
    # a failed capture is fatal (strict): an eager run would report ~half the throughput with rc = 0
    fwd = GraphedForward(model, enabled=bool(args.graph), strict=True)

    with MsdaProbe() as probe, RelHeadProbe() as rprobe, torch.no_grad():
        out = model(pixel_values=pv, pixel_mask=pm, output_attentions=False, output_attention_states=True,
                    output_hidden_states=True)  # eager once: fills the probe, loads MIOpen / rocBLAS kernels
        msda_args, rel_args = probe.args, rprobe.args
    with torch.no_grad():
        for _ in range(args.warmup):
            out = fwd(pv, pm)
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            out = fwd(pv, pm)
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    dt, spread = rank_times(dt, args.steps, dist, dev, world)
    value = world * args.batch * args.steps / dt
    if args.graph and not fwd.graphed:
        raise SystemExit("[bench] HIP-graph capture did not happen (pass --graph 0 to time eager launches)")
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, output_arrays(out))   # before anything else replays the graph into `out`

    result = {
        "metric": "images/sec end-to-end SGG, 600x1000 input, N=200 queries",
        "value": round(value, 3), "unit": "images/sec", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(dt / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": "VG inference: ResNet-50, N=200, 6 enc/6 dec, 150 classes, 50 predicates, "
                               f"600x1000, bs={args.batch}/GPU fp32 (BASELINE configs[1])",
                   "images_per_step_per_gpu": args.batch, "hip_graph": bool(args.graph) and fwd.graphed, "gemm_tuning": bool(args.tune_gemm),
                   "miopen_find": bool(torch.backends.cudnn.benchmark),
                   "parallelism": f"replicas x{world} (independent images, no collective)"},
        "rccl_ranks": args.rccl_ranks, "rank_ms_per_step": spread,
    }
    if world > 1 and backend != "nccl":
        result["config"]["collective_backend"] = f"{backend} (plumbing self-test: ranks share GPUs; not a performance number)"
    from egtr_amd import ops as _ops
    if not args.full:
        result["config"]["fast_path"] = {"strict": bool(_ops.STRICT_FAST_PATH), "fallbacks": dict(_ops.FALLBACKS)}
        if rank == 0:
            print(json.dumps(result))
        if dist is not None:
            dist.destroy_process_group()
        return

    msda_us, alg_bytes = time_msda_kernel(msda_args, probe.fused, keep_bits=probe.keep_bits)
    achieved = alg_bytes / (msda_us * 1e-6) / 1e9
    rel_us, rel_flops = time_rel_head_kernel(rel_args)
    rel_tflops = rel_flops / (rel_us * 1e-6) / 1e12
    msda_kernel = msda_kernel_name(probe.fused)
    l1_ceiling_gbs = time_l1_gather_ceiling()
    # HBM bytes / cache behaviour per launch come from separate rocprofv3 --pmc passes over THIS command
    # (tools/pmc_passes.sh + tools/msda_pmc.py -> profiles/r02_msda_pmc.json); used only if they were collected for
    # the kernel that was just timed, otherwise null.
    pmc, pmc_src = newest_pmc("r*_msda_pmc.json", msda_kernel)
    traffic = pmc.get("hbm_bytes_per_launch")
    result["roofline"] = {
        "bound": "hbm", "kernel": msda_kernel, "launch": "encoder layer, Lq = S = 12537, fused softmax + "
        "sampling locations" if probe.fused else "encoder layer, Lq = S = 12537",
        "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
        "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic,
        "algorithmic_bytes_per_launch": alg_bytes, "avg_launch_us": round(msda_us, 3),
        "traffic_source": pmc_src,
        "l2_hit": pmc.get("l2_hit"), "l1_gather_bytes": pmc.get("l1_gather_bytes"),
        # the vector-L1 return path is what bounds this kernel: its ceiling is MEASURED in this
        # run (csrc/probe_l1.hip); the gathered bytes per launch are 4 corners x 16 samples x 128 B per (query,
        # head) by construction, the counter figure (incl. the prologue's reads) comes from the PMC file
        "l1_gather_ceiling_gbs": round(l1_ceiling_gbs, 1),
        "l1_gather_bytes_by_construction": int(msda_args[0].shape[0] * msda_args[3].shape[1] * 8 * 64 * 128),
        "frac_of_l1_gather_ceiling": round(
            (pmc.get("l1_gather_bytes") or msda_args[0].shape[0] * msda_args[3].shape[1] * 8 * 64 * 128)
            / (msda_us * 1e-6) / 1e9 / l1_ceiling_gbs, 3)}
    split = bool(_ops.REL_HEAD_SPLIT_BF16) and rel_args[1].get("owner") is not None
    busy, busy_src = newest_mfma_busy()

    def x6_entry(kernel, launch, us, alg_flops, executed_flops, busy_key):
        """A kernel that computes fp32 results on the bf16 matrix cores (exact three-way operand splits, six cross terms per
        product on v_mfma_f32_32x32x16_bf16, fp32 accumulation): priced against the unit it RUNS on -- `achieved` = executed
        bf16 FLOPs / time, `peak` = the dense bf16 MFMA peak; the algorithmic fp32 rate is `achieved_fp32_equiv`."""
        e = {"bound": "mfma", "kernel": kernel, "launch": launch,
             "achieved": round(executed_flops / (us * 1e-6) / 1e12, 2), "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s",
             "frac": round(executed_flops / (us * 1e-6) / 1e12 / MFMA_BF16_PEAK_TFLOPS, 4), "traffic": None,
             "algorithmic_flops_per_launch": alg_flops, "bf16_mfma_flops_executed": executed_flops,
             "achieved_fp32_equiv": round(alg_flops / (us * 1e-6) / 1e12, 2), "avg_launch_us": round(us, 3),
             "arithmetic": "fp32 via bf16x6 operand split, fp32 accumulate"}
        if busy.get(busy_key) is not None:     # matrix pipe busy fraction from separate --pmc passes (tools/mfma_busy.py)
            e["mfma_busy"], e["mfma_busy_source"] = busy[busy_key], busy_src
        return e

    if split:
        # accuracy vs float64: tests/test_gpu_kernels.py::test_relation_head_split_bf16_is_fp32_accurate; the matrix cores
        # execute 6x the layer-2 / layer-3 products (layer 1 and the gates run on the vector ALUs)
        n2 = args.batch * 200 * 200
        rel_entry = x6_entry("rel_head_fwd_x6", f"B={args.batch}, N=200, T=7, R=50", rel_us, rel_flops,
                             2.0 * n2 * 6 * (2 * 256 * 256 + 256 * 64), "rel_head_fwd_x6")
    else:
        rel_entry = {"bound": "mfma", "kernel": "rel_head_fwd_f32", "launch": f"B={args.batch}, N=200, T=7, R=50",
                     "achieved": round(rel_tflops, 2), "peak": MFMA_F32_PEAK_TFLOPS, "unit": "TFLOP/s",
                     "frac": round(rel_tflops / MFMA_F32_PEAK_TFLOPS, 4), "traffic": None,
                     "algorithmic_flops_per_launch": rel_flops, "avg_launch_us": round(rel_us, 3)}
    rp, rp_src = newest_pmc("r*_rel_head_pmc.json", rel_entry["kernel"])   # same provenance as the MSDA counters above
    if rp:
        rel_entry["traffic"] = rp.get("hbm_bytes_per_launch")
        rel_entry["l2_hit"] = rp.get("l2_hit")
        rel_entry["traffic_source"] = rp_src
    result["roofline_kernels"] = [result["roofline"], rel_entry]
    if _ops.GEMM_SPLIT_BF16:
        g_us, g_flops = time_split_gemm(dev)
        # (until round 3 this key timed the 256 -> 1024 + ReLU product; since the FFN moved into the row-panel kernel the
        # model's only stand-alone launch of this kernel is the grouped one named here -- not comparable across that change)
        result["roofline_kernels"].append(x6_entry(
            "gemm_split_bf16_f32<grouped: value + offsets/weights>",
            "encoder layer: value (256->256) + offsets/weights (256->384, + position rows on load), M=12537, one launch",
            g_us, g_flops, 6 * g_flops, "gemm_split_bf16_f32"))
        result["config"]["encoder_linears"] = "fp32 via bf16x6 operand split, fp32 accumulate"
        import egtr_amd.backbone as _bb
        result["config"]["backbone"] = ("ResNet-50, frozen BN folded, channels-last; 3x3 convolutions of layers 1-3 "
                                        + ("own split-bf16 implicit GEMM (fp32 accumulate)" if _bb.CONV2_X6 else "MIOpen")
                                        + ", bottleneck tails " + ("own fused kernel" if _bb.CONV3_FUSED else "vendor GEMM + passes")
                                        + ", the rest MIOpen / hipBLASLt")
        t_us, t_flops = time_encoder_tail(dev)
        if t_us is not None:
            tail_entry = x6_entry(
                "ffn_x6_kernel<true>",
                "encoder layer tail: output projection + LayerNorm + FFN 256-1024-256 + LayerNorm, M=12537",
                t_us, t_flops, 6 * t_flops, "ffn_x6_kernel")
            tp, tp_src = newest_pmc("r*_ffn_x6_pmc.json", tail_entry["kernel"])
            if tp:
                tail_entry["traffic"] = tp.get("hbm_bytes_per_launch")
                tail_entry["l2_hit"] = tp.get("l2_hit")
                tail_entry["traffic_source"] = tp_src
            result["roofline_kernels"].append(tail_entry)
    result["config"]["relation_head"] = rel_entry.get("arithmetic", "exact-f32 MFMA")
    d_us, d_n = time_decoder_layer(model, pv, pm)
    if d_us is not None:
        # algorithmic bytes of one layer launch at N = 200, B = batch: the layer's weights once (3.80 MB fp32), states in / out,
        # q / k / v in and out (7 x N x 1 KiB), and the gathered value lines, at most N x 8 heads x 64 corners x 128 B
        nq = cfg.num_queries * args.batch
        d_alg = 3801088 + 8 * nq * 1024 + nq * 8 * 64 * 128
        d_entry = {"bound": "hbm", "kernel": "decoder_layer_cluster_f32",
                   "launch": f"one decoder layer (self-attention, MSDA cross-attention, FFN, next q/k/v), N={cfg.num_queries}, "
                             f"{d_n} launches per forward; latency-bound: 3 L2 barriers + 4 dependent phases per launch",
                   "achieved": round(d_alg / (d_us * 1e-6) / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                   "frac": round(d_alg / (d_us * 1e-6) / 1e9 / HBM_PEAK_GBS, 4), "algorithmic_bytes_per_launch": d_alg,
                   "avg_launch_us": round(d_us, 2), "traffic": None}
        dp, dp_src = newest_pmc("r*_dec_layer_pmc.json", "decoder_layer_cluster_f32")
        if dp:
            d_entry.update(traffic=dp.get("hbm_bytes_per_launch"), l2_hit=dp.get("l2_hit"), traffic_source=dp_src)
        result["roofline_kernels"].append(d_entry)
    try:
        for kname, launch, us, flops, nbytes in time_backbone_kernels(dev):
            e = x6_entry(kname, launch, us, flops, 6 * flops, kname.split("<")[0])
            # (the stem executes more than 6x its algorithmic flops: K padded 147 -> 224, overlapping pool windows)
            e["algorithmic_bytes_per_launch"] = int(nbytes)
            e["frac_of_hbm_roofline"] = round(nbytes / (us * 1e-6) / 1e9 / HBM_PEAK_GBS, 4)
            pat = {"conv_tail_x6_kernel": "r*_conv_tail_x6_pmc.json", "conv3x3_x6_ksplit_kernel": "r*_conv3x3_x6_pmc.json",
                   "stem_x6_kernel": "r*_stem_x6_pmc.json"}.get(kname.split("<")[0])
            tp, tp_src = newest_pmc(pat, kname) if pat else ({}, None)
            if tp:
                e.update(traffic=tp.get("hbm_bytes_per_launch"), l2_hit=tp.get("l2_hit"), traffic_source=tp_src)
            result["roofline_kernels"].append(e)
    except Exception as exc:  # the headline stays valid
        result["roofline_kernels"].append({"kernel": "backbone kernels", "error": f"{type(exc).__name__}: {exc}"})
    if rank == 0 and world == 1 and args.extras:
        # the FPS loop as the reference runs it (evaluate_egtr.py:26-36): differently sized images, and the eager number
        try:
            result["eager"] = eager_leg(model, pv, pm)
            result["mixed_shapes"] = mixed_shapes_leg(model, dev, value, tune_first_pass=bool(args.mixed_tune))
            result["batched_bs8"] = batched_leg(model, dev)
        except Exception as e:  # the headline stays valid; the failure is visible
            result["mixed_shapes"] = {"error": f"{type(e).__name__}: {e}"}
    result["config"]["fast_path"] = {"strict": bool(_ops.STRICT_FAST_PATH), "fallbacks": dict(_ops.FALLBACKS)}
    if world > 1 and args.extras:
        # BASELINE configs[2] ("RCCL grad all-reduce over xGMI"): every rank takes part; rank 0 reports
        try:
            ddp = ddp_train_leg(args, world, rank, dev, dist)
        except Exception as e:
            ddp = {"error": f"{type(e).__name__}: {e}"}
        if rank == 0:
            result["train_step_ddp"] = ddp
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        ncores = usable_cores()
        torch.set_num_threads(ncores)
        print(f"[bench] cpu baseline on {ncores} usable cores (os.cpu_count() = {os.cpu_count()})", file=sys.stderr)
        ips, nimg, ref, cpv, cpm = cpu_baseline(model, cfg_dict, args.cpu_budget)
        par = logit_parity(model, ref, cpv.to(dev), cpm.to(dev))
        print("[bench] parity vs CPU oracle on the bench workload (PRE-sigmoid logits, north-star bar 1e-3): "
              + ", ".join(f"max|d {k}| = {v:.2e}" for k, v in par.items()), file=sys.stderr)
        result["parity_vs_oracle"] = {k: float(f"{v:.3e}") for k, v in par.items()}
        if max(par.values()) >= 1e-3:
            print(json.dumps(result))
            raise SystemExit("[bench] parity against the CPU oracle FAILED (>= 1e-3 on a logit tensor)")
        result["cpu_baseline"] = {"value": round(ips, 4), "unit": "images/sec", "cores": torch.get_num_threads(),
                                  "kind": "port",
                                  "sample": f"{nimg} images after 1 warm-up, same 600x1000 / N=200 "
                                            "workload incl. ResNet-50, oracle = reference's pure-PyTorch "
                                            "grid_sample MSDA fallback semantics, torch CPU threads = cores"}
    if rank == 0 and world == 1 and args.extras:
        # The reference's other two workloads, driver-visible in the SAME line (bounded: a few steps each): the train step
        # (train_egtr.py:303-319, 770-779; BASELINE configs[2] shape on this GPU) and the stress shape (configs[4]).
        del fwd, out
        torch.cuda.empty_cache()
        import copy
        targs = copy.copy(args)
        # 10 warm-up steps as in `--mode train`: TunableOp picks and the caching allocator's pool settle over the first steps
        targs.mode, targs.batch, targs.steps, targs.warmup = "train", 4, 2 * args.extra_steps, 10
        targs.no_cpu_baseline, targs.no_kernel_probes = True, False
        find_was = torch.backends.cudnn.benchmark
        torch.backends.cudnn.benchmark = False      # MIOpen find mode: no gain for the train step
        try:
            result["train_step"] = train_bench(targs, 1, 0, dev, None, emit=False)
        except Exception as e:  # the headline stays valid; the failure is visible
            result["train_step"] = {"error": f"{type(e).__name__}: {e}"}
        torch.cuda.empty_cache()
        # ... and a large one for the bf16 stress forward: MIOpen's heuristic pick for the layer-1 3x3 convolutions at bs 16 is a
        # 400 us kernel where the search finds a 147 us one (tools/miopen_solver_ab.sh: 690 -> 771 images/s).  Until round 6
        # this leg inherited the train leg's "off".
        torch.backends.cudnn.benchmark = find_was
        try:
            result["stress_bf16"] = stress_bench(dev, steps=args.extra_steps, warmup=3)
        except Exception as e:
            result["stress_bf16"] = {"error": f"{type(e).__name__}: {e}"}
    if rank == 0:
        print(json.dumps(result))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
