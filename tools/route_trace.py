#!/usr/bin/env python
"""Route trace of the host model: which library entries and ATen operators one forward (or one train step) runs, in order.

    python tools/route_trace.py --out DIR [--dump DIR] [--device cpu] [--list] [CONFIG ...]

For every named configuration the tool builds the model from the test fixtures (stub backbone, seeded weights: tests/helpers.py,
tests/golden/weights.py), runs one warm-up pass (derived weights are cached on first use) and then records ONE pass:

  * every entry name that goes through ``egtr_amd._lib.launch`` (the attribute is wrapped for the pass),
  * every ATen operator dispatched (a ``TorchDispatchMode``),
  * ``dict(ops.FALLBACKS)`` at the end.

It writes ``DIR/<config>.txt``.  With ``--dump`` it also saves the outputs as ``<config>.pt``; training configurations run
forward + loss + backward under ``ops.deterministic()`` and save the loss and every parameter gradient.  ``--device cpu`` swaps
the three HIP operators the host-logic tests swap (tests/cpu_kernels.py); the trace then holds ATen operators only.

The tool uses public entry points only, so the same file runs in a checkout of any other commit: two directories of traces
(and dumps) are compared with ``--compare A B``, which is how a refactor of the forward passes is shown to change nothing.
tests/test_gpu_routes.py pins the library-entry column of the main configurations."""
import argparse
import contextlib
import json
import os
import sys

import torch
from torch.utils._python_dispatch import TorchDispatchMode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

SWITCHES = {"FFN_FUSED": ("ops", "FFN_FUSED"), "ENCODER_TAIL_FUSED": ("ops", "ENCODER_TAIL_FUSED"), "LAZY_POS": ("ops", "LAZY_POS"),
            "DEFER_LAYERNORM": ("ops", "DEFER_LAYERNORM"), "GEMM_SPLIT_BF16": ("ops", "GEMM_SPLIT_BF16"),
            "DECODER_CLUSTER": ("decoder_fused", "ENABLED")}
T_SIZE = (448, 448)      # stub backbone, strides 8 / 16 / 32 + the extra level: 56^2 + 28^2 + 14^2 + 7^2 = 4 165 tokens > 4 096


def _cfg(fixture="sgg_small.npz", size=None, batch=2, dtype="fp32", train=False, grad=False, attn=False, off=(), real=False):
    return dict(fixture=fixture, size=size, batch=batch, dtype=dtype, train=train, grad=grad, attn=attn, off=tuple(off), real=real)


CONFIGS = {"T": _cfg(size=T_SIZE, batch=1)}
for _s in SWITCHES:
    CONFIGS["T-no-" + _s] = _cfg(size=T_SIZE, batch=1, off=(_s,))
CONFIGS.update({
    "T-all-off": _cfg(size=T_SIZE, batch=1, off=tuple(SWITCHES)),
    "T2": _cfg(size=T_SIZE, batch=2),
    "T-nchw": _cfg(size=T_SIZE, batch=1, off=("NHWC_F32",)),
    "T-attn": _cfg(size=T_SIZE, batch=1, attn=True),
    "T-train": _cfg(size=T_SIZE, batch=1, train=True),
    "T-train-unfused": _cfg(size=T_SIZE, batch=1, train=True, off=("ENCODER_TRAIN_FUSED",)),
    "S": _cfg(),
    "S-bf16": _cfg(dtype="bf16"),
    "S-attn": _cfg(attn=True),
    "S-grad": _cfg(grad=True),
    "S-train": _cfg(train=True),
    "S-train-unfused": _cfg(train=True, off=("ENCODER_TRAIN_FUSED",)),
    "refine": _cfg("sgg_small_refine.npz"),
    "refine-train": _cfg("sgg_small_refine.npz", train=True),
    "two-stage": _cfg("sgg_small_two_stage.npz"),
    "two-stage-train": _cfg("sgg_small_two_stage.npz", train=True),
    # the in-repo ResNet-50 hands out channels-last maps: the grouped x6 input projection, and per-level mm without it
    "R": _cfg(size=(128, 160), batch=2, real=True),
    "R-no-GEMM_SPLIT_BF16": _cfg(size=(128, 160), batch=2, real=True, off=("GEMM_SPLIT_BF16",)),
})
CPU_CONFIGS = ("S", "S-attn", "S-grad", "S-train", "refine", "refine-train", "two-stage", "two-stage-train")
PINNED = ("T",) + tuple("T-no-" + s for s in SWITCHES) + ("S", "S-train")


class _Record(TorchDispatchMode):
    def __init__(self, lines):
        super().__init__()
        self.lines = lines

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.lines.append("aten " + str(func))
        return func(*args, **(kwargs or {}))


@contextlib.contextmanager
def _switched_off(names):
    from egtr_amd import backbone, decoder_fused, ops
    mods = dict(ops=ops, decoder_fused=decoder_fused, backbone=backbone)
    table = dict(SWITCHES, NHWC_F32=("backbone", "NHWC_F32"), ENCODER_TRAIN_FUSED=("ops", "ENCODER_TRAIN_FUSED"))
    saved = [(mods[table[n][0]], table[n][1], getattr(mods[table[n][0]], table[n][1])) for n in names]
    enabled = decoder_fused.ENABLED      # (a device that refuses the cluster kernel clears it: not carried to the next configuration)
    try:
        for mod, attr, _ in saved:
            setattr(mod, attr, False)
        yield
    finally:
        for mod, attr, value in saved:
            setattr(mod, attr, value)
        decoder_fused.ENABLED = enabled


@contextlib.contextmanager
def _cpu_stand_ins():
    import cpu_kernels as ck
    from egtr_amd import ops
    saved = (ops._msda, ops.decoder_self_attention, ops.relation_head)
    ops._msda, ops.decoder_self_attention, ops.relation_head = (lambda: ck.OracleMSDA), ck.decoder_self_attention, ck.relation_head
    try:
        yield
    finally:
        ops._msda, ops.decoder_self_attention, ops.relation_head = saved


def _build(spec, device):
    import helpers as Hh
    import weights as W
    g = Hh.load_golden(os.path.join(ROOT, "tests", "golden"), spec["fixture"])
    cfg_dict, shapes = json.loads(str(g["cfg"])), json.loads(str(g["shapes"]))
    if spec["real"]:
        from egtr_amd.egtr import DetrForSceneGraphGeneration
        cfg = Hh.product_config(cfg_dict)
        torch.manual_seed(5)
        model = DetrForSceneGraphGeneration(cfg, fg_matrix=W.fg_matrix(cfg.num_labels, cfg.num_rel_labels, seed=0))
    else:
        model, cfg, sd = Hh.build_product_model(cfg_dict, shapes, int(g["seed"]))
        model.load_state_dict(sd)
    B = spec["batch"]
    H, Wd = spec["size"] or (int(g["H"]), int(g["W"]))
    pv = torch.from_numpy(W.rng_inputs(int(g["input_seed"])).standard_normal((B, 3, H, Wd))).float()
    pm = torch.ones(B, H, Wd, dtype=torch.long)
    if B > 1:     # the second image is padded, in the fixture's proportions
        vh, vw = (int(v) * s // f for v, s, f in zip(g["valid1"], (H, Wd), (int(g["H"]), int(g["W"]))))
        pm[1, vh:, :] = 0
        pm[1, :, vw:] = 0
        pv[1] = pv[1] * pm[1][None].float()
    targets = None
    if spec["train"]:
        targets = [{k: t.to(device) for k, t in d.items()}
                   for d in W.make_targets(int(g["target_seed"]), B, cfg.num_queries, cfg.num_labels, cfg.num_rel_labels)]
    model = model.to(device).train(spec["train"])
    if spec["dtype"] == "bf16":
        model, pv = model.to(torch.bfloat16), pv.to(torch.bfloat16)
    if spec["grad"]:
        for p in model.parameters():
            p.requires_grad_(False)
    return model, pv.to(device), pm.to(device), targets


def _one_pass(model, pv, pm, targets, spec):
    from egtr_amd import ops
    if spec["train"]:
        model.zero_grad(set_to_none=True)
        with ops.deterministic():
            out = model(pixel_values=pv, pixel_mask=pm, labels=targets, output_attention_states=True)
            out.loss.backward()
        res = {"loss": out.loss.detach()}
        res.update({"grad::" + n: p.grad for n, p in model.named_parameters() if p.grad is not None})
        return res
    with (torch.enable_grad() if spec["grad"] else torch.no_grad()):
        out = model(pixel_values=pv, pixel_mask=pm, output_attentions=spec["attn"], output_attention_states=True,
                    output_hidden_states=True)
    res = {}
    for k, v in out.items():
        if torch.is_tensor(v):
            res[k] = v.detach()
        elif isinstance(v, (tuple, list)):
            res.update({f"{k}.{i}": t.detach() for i, t in enumerate(v) if torch.is_tensor(t)})
    return res


def trace(name, device="cuda"):
    """(lines, dump) of configuration ``name``: the ordered record of one pass, and its tensors on the host."""
    from egtr_amd import _lib, ops
    spec = CONFIGS[name]
    lines = []
    with contextlib.ExitStack() as stack:
        stack.enter_context(_switched_off(spec["off"]))
        if device == "cpu":
            stack.enter_context(_cpu_stand_ins())
        model, pv, pm, targets = _build(spec, device)
        _one_pass(model, pv, pm, targets, spec)        # warm-up: derived weights, geometry cache, the cluster kernel's first-run check
        ops.FALLBACKS.clear()
        real_launch = _lib.launch

        def launch(entry, *args, **kwargs):
            lines.append("lib " + entry)
            return real_launch(entry, *args, **kwargs)

        _lib.launch = launch
        try:
            with _Record(lines):
                res = _one_pass(model, pv, pm, targets, spec)
        finally:
            _lib.launch = real_launch
        lines.append("fallbacks " + json.dumps(dict(ops.FALLBACKS), sort_keys=True))
    return lines, {k: v.cpu() for k, v in res.items()}


def library_entries(lines):
    """The library-entry column of a trace, runs of a repeated name folded to ``(name, count)``."""
    out = []
    for line in lines:
        if not line.startswith("lib "):
            continue
        entry = line[4:]
        if out and (out[-1] == entry or (isinstance(out[-1], tuple) and out[-1][0] == entry)):
            out[-1] = (entry, out[-1][1] + 1 if isinstance(out[-1], tuple) else 2)
        else:
            out.append(entry)
    return out


def compare(a, b):
    """Compare two output directories of this tool; returns the list of differences (empty: identical)."""
    bad = []
    names = sorted(set(os.listdir(a)) | set(os.listdir(b)))
    for n in names:
        pa, pb = os.path.join(a, n), os.path.join(b, n)
        if not (os.path.exists(pa) and os.path.exists(pb)):
            bad.append(f"{n}: only in one directory")
        elif n.endswith(".txt"):
            if open(pa, "rb").read() != open(pb, "rb").read():
                la, lb = open(pa).read().split("\n"), open(pb).read().split("\n")
                i = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), min(len(la), len(lb)))
                bad.append(f"{n}: traces differ at line {i + 1}: {la[i:i + 1]} / {lb[i:i + 1]}")
        elif n.endswith(".pt"):
            da, db = torch.load(pa), torch.load(pb)
            if set(da) != set(db):
                bad.append(f"{n}: tensor names differ: {sorted(set(da) ^ set(db))}")
            bad += [f"{n}: {k} differs (max abs {float((da[k].double() - db[k].double()).abs().max()):.3g})"
                    for k in sorted(set(da) & set(db)) if not torch.equal(da[k], db[k])]
    return bad


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("configs", nargs="*")
    ap.add_argument("--out", help="directory of the trace files")
    ap.add_argument("--dump", help="directory of the saved outputs (default: none)")
    ap.add_argument("--device", default="cuda", choices=["cuda", "cpu"])
    ap.add_argument("--entries", action="store_true", help="print the folded library-entry sequence of each configuration")
    ap.add_argument("--list", action="store_true")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    args = ap.parse_args()
    if args.list:
        print("\n".join(CONFIGS))
        return 0
    if args.compare:
        bad = compare(*args.compare)
        print("\n".join(bad) if bad else f"identical: {len(os.listdir(args.compare[0]))} files")
        return 1 if bad else 0
    names = args.configs or (list(CPU_CONFIGS) if args.device == "cpu" else list(CONFIGS))
    torch.backends.cudnn.deterministic = True   # vendor convolution picks that differ between two processes hide real differences
    for d in (args.out, args.dump):
        if d:
            os.makedirs(d, exist_ok=True)
    for name in names:
        lines, dump = trace(name, args.device)
        if args.out:
            with open(os.path.join(args.out, name + ".txt"), "w") as f:
                f.write("\n".join(lines) + "\n")
        if args.dump:
            torch.save(dump, os.path.join(args.dump, name + ".pt"))
        if args.entries:
            print(f"{name!r}: {library_entries(lines)!r},")
        print(f"{name}: {sum(l.startswith('lib ') for l in lines)} library entries, "
              f"{sum(l.startswith('aten ') for l in lines)} ATen operators, {lines[-1]}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
