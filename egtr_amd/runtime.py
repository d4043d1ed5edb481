"""Run-time helpers around the model: HIP-graph replay of the inference forward, the reference's optimizer
grouping, and one-process-per-GPU data parallelism over RCCL (``torch.distributed`` backend "nccl" on ROCm).

The reference drives training through pytorch-lightning (train_egtr.py:770-783: DDPStrategy, accumulate 2,
clip 0.1) and measures FPS with a bare loop (evaluate_egtr.py:26-36).  Lightning is not part of the hot path and
is absent on the GPU box; these helpers reproduce exactly the pieces that touch it.
"""
import collections
import contextlib
import gc
import os

import torch
import torch.distributed as dist


@contextlib.contextmanager
def _collector_off():
    """Around a stream capture: Python's cycle collector must not run while the stream captures.  A dead cycle that holds GPU
    objects -- a dropped GraphedForward is one (model -> load_state_dict hook -> self -> its graphs and their pools) -- would be
    torn down in the middle of the capture, where that is an illegal call and aborts the process.  torch.cuda.graph() collected
    before every capture up to torch 2.9 and no longer does: collect first, then keep the collector off until the end."""
    gc.collect()
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was_enabled:
            gc.enable()


class _GraphEntry:
    """One captured forward: the graph, its static input buffers and static outputs, and the weight epoch it was captured at."""
    __slots__ = ("graph", "static_in", "static_out", "epoch", "replays")

    def __init__(self, graph, static_in, static_out, epoch):
        self.graph, self.static_in, self.static_out, self.epoch, self.replays = graph, static_in, static_out, epoch, 0


class GraphedForward:
    """Replay ``model(pixel_values, pixel_mask, output_attention_states=True, output_hidden_states=True)`` from captured
    HIP graphs.  At bs = 1 the forward is ~150 short kernels, i.e. launch-bound when issued eagerly
    (MI355X_MICROARCH.md: eager launch ~3.3-3.8 us host time each); a graph replay issues them back-to-back.
    Inputs are copied into static buffers; outputs are the graph's static tensors (valid until the next call).

    **Variable image sizes** (the reference's FPS loop runs over a dataloader whose images are resized to a short side of
    ``--min_size`` / long side <= ``--max_size``, evaluate_egtr.py:26-36, 165-175, so almost every batch has its own shape):
    the object keeps an LRU of up to ``max_graphs`` captured graphs keyed by (pixel shape, mask shape, dtypes, device).  A
    shape seen before replays its own graph -- own static inputs, own outputs, own private memory pool (a 600x1000 fp32
    forward holds < 0.5 GB; sixteen of them are noise in 288 GB of HBM) -- and only a NEW shape pays the two eager
    warm-up runs + capture (the warm-up runs are also what lets MIOpen / TunableOp pick their kernels for the new
    convolution / GEMM shapes outside the capture).  The least recently used graph is dropped when the table is full;
    ``capture_after = k`` defers a shape's capture until it is seen for the k-th time (eager launches before that).

    **Weights.**  A captured graph bakes in pointers to DERIVED tensors built at capture time (folded-BN backbone weights,
    stacked / concatenated projection weights, query tables).  The table is therefore tagged with a weight EPOCH: the full
    fingerprint of the model's parameters and buffers (storage pointer + version counter of each, ~140 us of host time for
    the 589 tensors of EGTR) is taken once per epoch, not per call.  What starts a new epoch: ``load_state_dict`` (a hook
    on the model), an explicit ``invalidate()``, and -- as the per-call O(1) check -- a change of the version counter or
    storage of any of a few SENTINEL tensors (the first and last parameter of the backbone, encoder, decoder and heads: an
    optimizer step, ``.to()`` / ``.half()`` / ``.cuda()`` or an in-place edit of the whole model moves all of them).  Every ``verify_every`` calls the full fingerprint is compared again as a backstop for edits that touch
    only non-sentinel tensors.  On a new epoch every graph is dropped (they all hold stale constants).  Edits through
    ``.data`` bypass the version counter -- call ``invalidate()`` after those.

    ``strict=True`` (what bench.py uses): a failed capture raises.  ``strict=False``: falls back to eager launches
    (``self.graphed = False``, reason in ``capture_error``) -- same kernels either way, about 2x slower at bs = 1.

    Every ``status_every`` calls the sticky status words of the one-launch decoder layers are polled without a
    synchronisation (``decoder_fused.poll_status``: asynchronous copy now, verdict at the next poll); a cluster barrier
    that timed out raises ``DecoderClusterError`` instead of handing out void decoder states."""

    def __init__(self, model, enabled=True, warmup=2, strict=False, max_graphs=16, verify_every=256, status_every=64,
                 capture_after=1, bucket=None):
        self.model = model
        self.enabled = enabled
        self.warmup = warmup
        self.strict = strict
        self.max_graphs = max(1, int(max_graphs))
        self.verify_every = max(1, int(verify_every))
        self.status_every = max(1, int(status_every))
        # a shape is captured when it is seen for the `capture_after`-th time and runs eagerly before that: a dataloader with
        # hundreds of distinct shapes (every long side between 600 and 1000) should not pay ~1.5 s of warm-up + capture for
        # a shape it meets once -- raise it (and `max_graphs`: sixteen graphs are ~6 GB of the 288) for such streams
        self.capture_after = max(1, int(capture_after))
        # bucket = k (opt-in): images are placed in the top-left corner of a zero canvas whose height and width are rounded up
        # to multiples of k, the rest masked out in pixel_mask -- exactly what the reference's collate does to the smaller
        # images of a BATCH (DetrFeatureExtractor.pad_and_create_pixel_mask) -- so that a dataset with hundreds of distinct
        # sizes needs a few dozen graphs (k = 32: <= 14 long sides for short side 600 / long side 600..1000, x 2
        # orientations).  Outputs are those of the padded forward (normalised boxes refer to the VALID region through the
        # valid ratios, as in batched inference), not bit-identical to the unpadded one.
        self.bucket = int(bucket) if bucket else None
        self._seen = collections.Counter()
        self.eager_calls = 0
        self._entries = collections.OrderedDict()   # key -> _GraphEntry, least recently used first
        self._tensors = None
        self._sentinels = None
        self._sentinel_key = None
        self._fingerprint_key = None
        self._epoch = 0
        self._calls = 0
        self.graphed = False
        self.captures = 0          # graphs captured so far (a shape that comes back after eviction counts again)
        self.evictions = 0
        self.capture_error = None
        self._hooks = []
        self._install_hooks()

    # ---- weight epochs -------------------------------------------------------------------------------------------
    def _install_hooks(self):
        """load_state_dict starts a new epoch at once (it also bumps every version counter, which the sentinels see);
        ``.to()`` / ``.cuda()`` / ``.half()`` replace every parameter's storage, which the sentinels see as well."""
        bump = self._bump
        try:
            self._hooks.append(self.model.register_load_state_dict_post_hook(lambda module, incompatible: bump()))
        except Exception:  # pragma: no cover - torch without the hook: the sentinels / verify pass still catch it
            pass

    def _bump(self):
        self._epoch += 1
        self._tensors = None
        self._sentinels = None

    def _all_tensors(self):
        if self._tensors is None:
            self._tensors = list(self.model.parameters()) + list(self.model.buffers())
        return self._tensors

    def _fingerprint(self):
        return [(t.data_ptr(), t._version) for t in self._all_tensors()]

    def _sentinel_fingerprint(self):
        if self._sentinels is None:
            picks = []
            for child in self.model.children():
                ps = list(child.parameters())
                if ps:
                    picks += [ps[0], ps[-1]]
                for grand in child.children():
                    gs = list(grand.parameters())
                    if gs:
                        picks += [gs[0], gs[-1]]
            own = list(self.model.parameters())
            picks += own[:1] + own[-1:]
            seen, uniq = set(), []
            for t in picks:
                if id(t) not in seen:
                    seen.add(id(t))
                    uniq.append(t)
            self._sentinels = uniq[:24]
        return tuple((t.data_ptr(), t._version) for t in self._sentinels)

    def _weights_changed(self):
        """O(1) per call; the full fingerprint only when an epoch was announced, a sentinel moved, or on the periodic verify."""
        full = self._fingerprint_key is None or self._calls % self.verify_every == 0
        epoch_now = self._epoch
        if self._sentinels is None or self._sentinel_fingerprint() != self._sentinel_key:
            full = True
        if getattr(self, "_seen_epoch", None) != epoch_now:
            full = True
        if not full:
            return False
        self._seen_epoch = epoch_now
        self._tensors = self._sentinels = None     # re-enumerate: a parameter OBJECT may have been replaced
        self._sentinel_key = self._sentinel_fingerprint()
        fp = self._fingerprint()
        if fp == self._fingerprint_key:
            return False
        changed = self._fingerprint_key is not None
        self._fingerprint_key = fp
        return changed

    def invalidate(self):
        """Forget every captured graph and every derived constant (after weights were edited through ``.data``)."""
        from . import ops
        ops.invalidate_derived(self.model)
        self._drop_all()
        self._bump()
        self._fingerprint_key = None

    def _drop_all(self):
        self._entries.clear()

    def close(self):
        """Release this object: take its hooks off the model and drop every captured graph."""
        for h in self._hooks:
            h.remove()
        self._hooks.clear()
        self._drop_all()

    # ---- capture / replay ----------------------------------------------------------------------------------------
    def _eager(self, pv, pm):
        return self.model(pixel_values=pv, pixel_mask=pm, output_attentions=False, output_attention_states=True,
                          output_hidden_states=True)

    @staticmethod
    def _key(pv, pm):
        return (tuple(pv.shape), pv.dtype, tuple(pm.shape), pm.dtype, pv.device)

    def _capture(self, pv, pm):
        static_in = (pv.clone(), pm.clone())
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(self.warmup):
                self._eager(*static_in)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with _collector_off(), torch.cuda.graph(g):
            static_out = self._eager(*static_in)
        self.captures += 1
        self.graphed = True
        return _GraphEntry(g, static_in, static_out, self._epoch)

    @property
    def cached_shapes(self):
        """(pixel shape, ...) keys of the graphs held now, least recently used first."""
        return [k[0] for k in self._entries]

    def prime(self, shapes, dtype=torch.float32, device=None):
        """Capture a graph for every (B, 3, H, W) in ``shapes`` ahead of time (zeros as pixels, all-ones masks) -- what an
        evaluation run does once for the resize buckets of its dataloader; returns the number of new captures."""
        device = device if device is not None else next(self.model.parameters()).device
        before = self.captures
        for shp in shapes:
            b, _, h, w = shp
            self(torch.zeros(*shp, dtype=dtype, device=device), torch.ones(b, h, w, dtype=torch.long, device=device))
        return self.captures - before

    def _to_bucket(self, pv, pm):
        k = self.bucket
        h, w = pv.shape[-2:]
        hb, wb = -(-h // k) * k, -(-w // k) * k
        if (hb, wb) == (h, w):
            return pv, pm
        cpv = pv.new_zeros(*pv.shape[:-2], hb, wb)
        cpv[..., :h, :w] = pv
        cpm = pm.new_zeros(*pm.shape[:-2], hb, wb)
        cpm[..., :h, :w] = pm
        return cpv, cpm

    def _poll_decoder_status(self, device):
        from . import decoder_fused
        decoder_fused.poll_status(device)

    @torch.no_grad()
    def __call__(self, pv, pm):
        if not self.enabled:
            return self._eager(pv, pm)
        if self.bucket:
            pv, pm = self._to_bucket(pv, pm)
        self._calls += 1
        if self._weights_changed():
            self._drop_all()      # every graph holds constants derived from the old weights
        key = self._key(pv, pm)
        entry = self._entries.get(key)
        if entry is None and self.capture_after > 1:
            self._seen[key] += 1
            if self._seen[key] < self.capture_after:
                self.eager_calls += 1
                return self._eager(pv, pm)
        if entry is None:
            try:
                entry = self._capture(pv, pm)
            except Exception as e:  # capture unsupported by some library call: run eagerly, same kernels
                if self.strict:
                    raise
                self.capture_error = repr(e)
                self.enabled = False
                self.graphed = False
                torch.cuda.synchronize()
                return self._eager(pv, pm)
            self._entries[key] = entry
            while len(self._entries) > self.max_graphs:
                self._entries.popitem(last=False)
                self.evictions += 1
        else:
            self._entries.move_to_end(key)
        entry.static_in[0].copy_(pv)
        entry.static_in[1].copy_(pm)
        entry.graph.replay()
        entry.replays += 1
        if self._calls % self.status_every == 0:
            self._poll_decoder_status(pv.device)
        return entry.static_out


def configure_optimizers(model, lr=2e-6, lr_backbone=2e-7, lr_initialized=2e-4, weight_decay=1e-4,
                         initialized_keys=()):
    """The reference's three AdamW parameter groups (train_egtr.py:426-467)."""
    diff = ["backbone", "reference_points", "sampling_offsets"]
    init = list(initialized_keys) if lr_initialized is not None else []
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    groups = [{"params": [p for n, p in named if not any(d in n for d in diff) and not any(d in n for d in init)]},
              {"params": [p for n, p in named if any(d in n for d in diff)], "lr": lr_backbone}]
    if init:
        groups.append({"params": [p for n, p in named if any(d in n for d in init)], "lr": lr_initialized})
    # same update rule as the reference's torch.optim.AdamW; on the GPU the single-kernel-per-group ("fused")
    # implementation replaces ~10 multi-tensor launches per group (the step is launch-bound: 42.5 M parameters)
    on_gpu = bool(named) and all(p.is_cuda for _, p in named)
    return torch.optim.AdamW(groups, lr=lr, weight_decay=weight_decay, fused=True if on_gpu else None)


def init_distributed():
    """One process per GPU; RCCL over xGMI when GPUs are present, gloo on CPU (tests).  Reads the torchrun env."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world <= 1 or dist.is_initialized():
        return world
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    if torch.cuda.is_available():
        lr = int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(lr)
        dist.init_process_group("nccl", device_id=torch.device("cuda", lr))
    else:
        dist.init_process_group("gloo")
    return world


class DataParallelTrainer:
    """Data-parallel train step with the reference's semantics (train_egtr.py:303-319, 770-779):
    identical replicas, per-rank micro-batches, gradient all-reduce (bucketed, overlapped with backward by DDP)
    once per optimizer step -- micro-steps before the accumulation boundary run under ``no_sync`` -- then
    clip-grad-norm 0.1 and AdamW.  ``num_boxes`` stays per-rank (model/egtr.py:976-980)."""

    def __init__(self, model, optimizer=None, accumulate=2, clip=0.1, bucket_cap_mb=25, graph=False, force_ddp=False,
                 grad_compression=None, deterministic=False, matmul_precision=None, relation_sampler=None,
                 relation_sampler_seed=None):
        """graph=True (single process, GPU, fixed image size): the static-shape part of the step -- backbone, encoder,
        decoder, detection + relation heads, forward AND backward -- is captured once into two HIP graphs
        (torch.cuda.make_graphed_callables over ``model.forward_tensors``) and replayed; the Hungarian matcher and the
        loss stay eager in between (they have data-dependent shapes).  Measured SLOWER than the eager step: the
        untraced eager step is GPU-bound with the host 25-40 ms ahead of the device, so a replay has no launch gaps to close,
        and it adds copies out of the graphs' static buffers (forward 15.1 vs 14.2 ms, backward 35.4 vs 29.9 ms).  Opt-in.

        ``grad_compression``: None (fp32 all-reduce, the reference's DDP), "bf16" or "fp16" -- DDP's communication hook that
        casts every gradient bucket to 16 bits for the all-reduce and back (torch's ``bf16_compress_hook`` / ``fp16_compress_hook``):
        half the bytes per link for the bandwidth-bound stress configuration (165 MB fp32 per step otherwise).  The
        averaged gradient is then rounded to 8 / 11 significant bits before clipping -- opt-in, not the parity configuration.

        ``deterministic=True``: every step runs under ``ops.deterministic()`` -- the library's order-free routes (fixed-point MSDA
        grad_value, indexed loss ties, gate means reduced in a fixed order): same inputs, device and build give the same bits
        from the library's own kernels -- and ``torch.backends.cudnn.deterministic`` is set, which REQUESTS deterministic MIOpen
        algorithms; MIOpen's compliance is requested, not promised, and vendor GEMMs / ATen operations without a deterministic
        form are outside the guarantee.  Works with ``graph=True``: the mode is part of the key of the captured
        step, so a step captured under one setting is never replayed under the other.

        ``matmul_precision``: None (follow ``ops.matmul_precision()``, i.e. EGTR_MATMUL_PRECISION or the last
        ``ops.set_matmul_precision``), "fp32" or "bf16": every step runs inside ``ops.matmul_precision_mode(..)``.  "bf16": the
        token-sized products of the encoder layers and of the decoder's value projections round each operand once to bf16
        (fp32 accumulation; weights, gradients and the optimizer stay fp32; no loss scaling) -- DESIGN.md 4.12b.  Part of the
        captured step's key like the deterministic mode, and it combines freely with it: the two touch different kernels.

        ``relation_sampler``: None (follow ``ops.relation_sampler()``), "python" or "device": every step runs inside
        ``ops.relation_sampler_mode(..)``.  It matters for a criterion with ``rel_sample_*_largest=False`` only: "device" draws the
        random candidate classes in the loss kernels (no host wait), "python" with the reference's
        ``random.sample``.  ``relation_sampler_seed``: the device sampler's seed (None: the current one, initially
        ``torch.initial_seed()``); the rank is added, so replicas draw independently.  The loss is eager in the graphed step
        too, so the sampler is no part of a captured step's key."""
        from . import ops
        self.relation_sampler = None if relation_sampler is None else ops._checked_relation_sampler(relation_sampler)
        rank = dist.get_rank() if dist.is_initialized() else 0
        if relation_sampler_seed is not None or (self.relation_sampler == "device" and rank):
            seed = ops.relation_sampler_state()[0] if relation_sampler_seed is None else int(relation_sampler_seed)
            ops.set_relation_sampler_state(seed + rank, 0)
        self.matmul_precision = None if matmul_precision is None else ops._checked_matmul_precision(matmul_precision)
        self.deterministic = bool(deterministic)
        if self.deterministic:
            torch.backends.cudnn.deterministic = True
        self.world = dist.get_world_size() if dist.is_initialized() else 1
        self.raw = model
        self.grad_compression = None
        self._graph_wanted = bool(graph) and self.world == 1
        self._graphed = None
        self._graph_key = None
        # force_ddp: wrap even in a one-rank process group, so that DDP's reducer (bucket hooks on the autograd Functions
        # that launch through the C ABI, gradient_as_bucket_view) can be exercised on a single-GPU box
        if self.world > 1 or (force_ddp and dist.is_initialized()):
            ids = [torch.cuda.current_device()] if next(model.parameters()).is_cuda else None
            self.model = torch.nn.parallel.DistributedDataParallel(
                model, device_ids=ids, find_unused_parameters=False, bucket_cap_mb=bucket_cap_mb,
                gradient_as_bucket_view=True)
            if grad_compression is not None:
                from torch.distributed.algorithms.ddp_comm_hooks import default_hooks
                hooks = {"bf16": default_hooks.bf16_compress_hook, "fp16": default_hooks.fp16_compress_hook}
                if grad_compression not in hooks:
                    raise ValueError(f"grad_compression must be None, 'bf16' or 'fp16', got {grad_compression!r}")
                self.model.register_comm_hook(state=None, hook=hooks[grad_compression])
                self.grad_compression = grad_compression
        else:
            self.model = model
        self.opt = optimizer if optimizer is not None else configure_optimizers(model)
        self.accumulate = accumulate
        self.clip = clip
        self._micro = 0

    def _graphed_body(self, pixel_values, pixel_mask):
        from . import ops
        key = (tuple(pixel_values.shape), pixel_values.dtype, tuple(pixel_mask.shape), pixel_mask.dtype, ops.is_deterministic(),
               ops.matmul_precision())
        if self._graphed is None or key != self._graph_key:
            raw = self.raw

            class _Body(torch.nn.Module):  # parameters are found through the wrapped model
                def __init__(self):
                    super().__init__()
                    self.m = raw

                def forward(self, pv, pm):
                    return self.m.forward_tensors(pv, pm)

            # gradients accumulated by earlier micro-steps of this window must survive the warm-up / capture backward
            # passes (a shape change can fall on any micro-step when accumulate > 1): stash, capture, restore
            params = [p for p in raw.parameters()]
            stash = [p.grad for p in params]
            for p in params:
                p.grad = None
            with _collector_off():
                self._graphed = torch.cuda.make_graphed_callables(
                    _Body(), (pixel_values.detach().clone(), pixel_mask.detach().clone()), num_warmup_iters=3)
            self._graph_key = key
            for p, g in zip(params, stash):  # drops what the warm-up / capture backward passes left behind
                p.grad = g
        return self._graphed(pixel_values, pixel_mask)

    def common_step(self, batch):
        pv, pm = batch["pixel_values"], batch["pixel_mask"]
        if self._graph_wanted and pv.is_cuda and self.raw.training:
            return self.raw.loss_from_tensors(self._graphed_body(pv, pm), batch["labels"])
        out = self.model(pixel_values=pv, pixel_mask=pm, labels=batch["labels"],
                         output_attentions=False, output_attention_states=True, output_hidden_states=True)
        return out.loss, out.loss_dict

    def _refused_flag(self):
        """0-dim float32 on the device: 1 if the device matcher refused a cost matrix (NaN / -inf entries, infeasible) in any
        forward since the last optimizer step, on any rank; None when no device matcher ran.  No host synchronisation."""
        from .deformable_detr import DeformableDetrHungarianMatcher
        statuses = DeformableDetrHungarianMatcher.take_step_statuses()
        if not statuses:
            return None
        # the worst solver status code of the window (0 = assigned, 1 = NaN / -inf entries, 2 = infeasible) ...
        worst = torch.cat([s.reshape(-1) for s in statuses]).max().to(torch.float32).reshape(())
        if self.world > 1:
            # replicas must skip together (4 bytes) -- and RAISE together, with the RIGHT message: the MAX of the status CODES
            # is queued for raise_if_invalid on every rank (a 0 / 1 flag made every remote refusal read "invalid numeric
            # entries"); otherwise only the refusing rank would stop at its next step and the others would block
            # in the next gradient all-reduce
            dist.all_reduce(worst, op=dist.ReduceOp.MAX)
            if worst.is_cuda:
                DeformableDetrHungarianMatcher.defer_status(worst)
        # ... and the 0 / 1 flag torch's GradScaler hands to the fused optimizers as `found_inf` (0-dim float32)
        return worst.ne(0).to(torch.float32).reshape(())

    def training_step(self, batch):
        """One micro-batch; returns (loss, loss_dict, stepped).

        A cost matrix the device matcher refuses (NaN / -inf: the reference raises scipy's ValueError inside the step,
        before backward) makes the loss and every gradient NaN.  The optimizer step of such a window is SKIPPED on the
        device (the fused AdamW's ``found_inf`` operand -- the mechanism of torch's GradScaler), so the weights and the
        optimizer state stay intact; the ValueError itself is raised by ``raise_if_invalid`` at the top of the next step
        (or by ``finalize()`` after the last one), without a host synchronisation inside the step that produced it.
        Optimizers without a device-side skip flag wait for the recorded status copy instead (one host wait per step)."""
        from .deformable_detr import DeformableDetrHungarianMatcher
        DeformableDetrHungarianMatcher.raise_if_invalid()
        self._micro += 1
        boundary = self._micro % self.accumulate == 0
        wrapped = self.model is not self.raw
        ctx = contextlib.nullcontext() if (boundary or not wrapped) else self.model.no_sync()
        from . import ops
        mode = ops.deterministic(True) if self.deterministic else contextlib.nullcontext()
        prec = ops.matmul_precision_mode(self.matmul_precision) if self.matmul_precision is not None else contextlib.nullcontext()
        sampler = (ops.relation_sampler_mode(self.relation_sampler) if self.relation_sampler is not None
                   else contextlib.nullcontext())
        with ctx, mode, prec, sampler:
            loss, loss_dict = self.common_step(batch)
            (loss / self.accumulate).backward()
        if boundary:
            refused = self._refused_flag()
            torch.nn.utils.clip_grad_norm_(self.raw.parameters(), self.clip)
            skip_on_device = refused is not None and all(g.get("fused") for g in self.opt.param_groups)
            if refused is not None and not skip_on_device:
                # no device-side skip in this optimizer: wait for the status copies and raise the matcher's ValueError now,
                # before the step (weights still intact); `refused` also covers the other ranks
                try:
                    DeformableDetrHungarianMatcher.raise_if_invalid()
                    if bool(refused.item()):
                        raise ValueError("matrix contains invalid numeric entries")
                except ValueError:
                    self.opt.zero_grad(set_to_none=True)
                    raise
            if skip_on_device:
                self.opt.found_inf = refused
            try:
                self.opt.step()
            finally:
                if skip_on_device:
                    del self.opt.found_inf
            self.opt.zero_grad(set_to_none=True)
        return loss.detach(), loss_dict, boundary

    def validation_step(self, batch):
        """One validation batch (train_egtr.py:333-336): the RAW model in evaluation mode under ``torch.no_grad()`` -- no DDP
        synchronisation, no graph capture -- through ``common_step``.  Returns (loss, loss_dict), detached, with
        ``loss_dict["loss"] = loss``.  In evaluation mode the criterion's relation loss is un-sampled (BCE over every element):
        on the device that is ops.RelationLossAllFunction's value-only launch, with no host synchronisation.  Every module's
        ``training`` flag is restored on the way out, after an exception too.

        The device matcher's per-step statuses of the validation forward are dropped, and the ones the current accumulation
        window had recorded are kept: nothing is stepped here, so a cost matrix refused in a validation batch must neither pile
        up over an epoch nor make the next training window skip its optimizer step.  The refusal itself is not lost: its
        ValueError is raised by ``raise_if_invalid`` at the top of the next ``training_step`` or by ``finalize()``, and the
        batch's loss terms are NaN."""
        from . import deformable_detr as dd
        window = dd.DeformableDetrHungarianMatcher.take_step_statuses()
        flags = [(m, m.training) for m in self.raw.modules()]   # per module: a submodule kept in eval mode stays there
        wrapped, graph_wanted = self.model, self._graph_wanted
        self.model, self._graph_wanted = self.raw, False
        self.raw.eval()
        try:
            with torch.no_grad():
                loss, loss_dict = self.common_step(batch)
            loss = loss.detach()
            loss_dict = {k: v.detach() for k, v in loss_dict.items()}
            loss_dict["loss"] = loss
            return loss, loss_dict
        finally:
            self.model, self._graph_wanted = wrapped, graph_wanted
            for m, flag in flags:
                m.training = flag
            dd.DeformableDetrHungarianMatcher.take_step_statuses()
            dd._STEP_MATCHER_STATUS.extend(window)

    @staticmethod
    def validation_epoch_end(outputs):
        """The reference's epoch summary (train_egtr.py:338-348): per key of the steps' loss dicts the mean over the steps, as
        ``{"validation_<key>": float}``.  ``outputs``: the ``validation_step`` results, (loss, loss_dict) pairs or the loss dicts
        alone.  The one host wait of a validation epoch: every mean is formed on the device, one copy brings them over."""
        dicts = [o[1] if isinstance(o, (tuple, list)) else o for o in outputs]
        if not dicts:
            return {}
        keys = list(dicts[0])
        means = torch.stack([torch.stack([torch.as_tensor(d[k]).detach().float() for d in dicts]).mean() for k in keys])
        return {f"validation_{k}": v for k, v in zip(keys, means.tolist())}

    def finalize(self):
        """After the last step of a run: raise what the device matcher refused in it (``training_step`` reports a refusal at
        the top of the NEXT step; there is none after the last one)."""
        from .deformable_detr import DeformableDetrHungarianMatcher
        DeformableDetrHungarianMatcher.raise_if_invalid()


def enable_gemm_tuning(results_file=None):
    """Let PyTorch's TunableOp pick, per GEMM shape, the fastest rocBLAS / hipBLASLt solution the first time the shape
    is seen (the MI355X analogue of the reference's ``torch.backends.cudnn.benchmark``-style autotuning).  The token
    sized encoder GEMMs (12 537 x 256 x {256, 384, 1024}) gain ~20 % over the libraries' default heuristics.  Call
    before the first forward; shapes must have been seen eagerly before a HIP-graph capture."""
    import os
    import tempfile
    try:
        import torch.cuda.tunable as tunable
    except Exception:  # pragma: no cover - very old torch
        return False
    tunable.enable(True)
    tunable.tuning_enable(True)
    if results_file is None:
        # one results file per PROCESS (= per rank): eight ranks tuning concurrently must not share a csv
        results_file = os.path.join(tempfile.gettempdir(),
                                    f"egtr_tunableop_r{os.environ.get('RANK', '0')}_{os.getpid()}.csv")
    tunable.set_filename(results_file, insert_device_ordinal=True)
    return True


def enable_conv_tuning():
    """MIOpen find mode (``torch.backends.cudnn.benchmark = True``): every convolution shape of the backbone gets the
    solver that measures fastest the first time it is seen, instead of the heuristic choice (ResNet-50 at 600x1000, fp32
    inference: 250 -> 261 images/s end to end).  Call before the first forward; shapes must have been seen eagerly
    before a HIP-graph capture.  No effect on the train step."""
    private_miopen_db()
    torch.backends.cudnn.benchmark = True
    return True


def private_miopen_db():
    """Multi-rank runs: give every rank its own MIOpen user database directory (find mode WRITES the tuned solvers
    there; eight ranks appending to one sqlite file race).  Must run before the first convolution; no-op for one rank
    or when the user already chose a path."""
    import tempfile
    if int(os.environ.get("WORLD_SIZE", "1")) > 1 and "MIOPEN_USER_DB_PATH" not in os.environ:
        d = os.path.join(tempfile.gettempdir(), f"egtr_miopen_r{os.environ.get('RANK', '0')}")
        os.makedirs(d, exist_ok=True)
        os.environ["MIOPEN_USER_DB_PATH"] = d
        os.environ.setdefault("MIOPEN_CUSTOM_CACHE_DIR", d)


@torch.no_grad()
def calculate_fps(model, batches, warmup=3, graphed=True, max_graphs=16, forward=None, capture_after=1):
    """evaluate_egtr.py:26-36 with warm-up and synchronisation (the reference's loop has neither).

    ``graphed=True`` (GPU): every batch goes through a ``GraphedForward`` -- one captured HIP graph per distinct image
    shape, LRU of ``max_graphs`` -- so a dataloader of differently sized images (evaluate_egtr.py:165-175: short side
    ``--min_size``, long side <= ``--max_size``) runs at graph-replay speed once each shape has been seen.  When ``batches``
    is a sequence its distinct shapes are captured BEFORE the clock starts (their two eager warm-up runs + capture are the
    analogue of the reference's cudnn autotuning on a new shape); for a plain iterator the first occurrence of a shape is
    inside the timed region.  ``forward``: an existing ``GraphedForward`` to reuse.  ``graphed=False``: eager launches.
    A real evaluation set has hundreds of distinct shapes: raise ``max_graphs`` (a 600x1000 graph holds < 0.5 GB of the 288 GB)
    and / or ``capture_after`` (eager until a shape comes back) accordingly."""
    import time
    model.eval()
    fwd = forward
    if fwd is None and graphed and torch.cuda.is_available():
        fwd = GraphedForward(model, enabled=True, strict=False, max_graphs=max_graphs, capture_after=capture_after)

    def run(batch):
        pv, pm = batch["pixel_values"].cuda(non_blocking=True), batch["pixel_mask"].cuda(non_blocking=True)
        if fwd is not None:
            return fwd(pv, pm)
        return model(pixel_values=pv, pixel_mask=pm, output_attentions=False, output_attention_states=True,
                     output_hidden_states=True)

    if fwd is not None and isinstance(batches, (list, tuple)):
        seen = set()
        for batch in batches:
            key = (tuple(batch["pixel_values"].shape), tuple(batch["pixel_mask"].shape))
            if key not in seen and len(seen) < fwd.max_graphs:
                seen.add(key)
                run(batch)
    n = 0
    t0 = None
    for i, batch in enumerate(batches):
        if i == warmup:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        run(batch)
        if i >= warmup:
            n += batch["pixel_values"].shape[0]
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0) if t0 is not None and n else float("nan")


@torch.no_grad()
def triplet_candidates(outputs, num_labels, orig_sizes, max_topk=100, mode="multiple"):
    """The evaluator inputs of the reference's ``evaluate_batch`` (train_egtr.py:54-175) computed where the model outputs
    live.  Per image: object scores / classes (softmax over the first ``num_labels`` logits), boxes rescaled to the original
    image size, and -- by ``mode`` --
      * "multiple" (train_egtr.py:85-106, multiple-predicate evaluator): the ``max_topk`` best (subject, object, predicate)
        triplets by ``pred_rel * pred_connectivity * score_s * score_o`` (self-pairs excluded): ``pred_rel_inds`` [k, 3],
        ``rel_scores`` [k];
      * "single" (train_egtr.py:120-139, single-predicate evaluator): the ``max_topk`` best (subject, object) PAIRS by
        ``max_p(pred_rel * pred_connectivity) * score_s * score_o``: ``pred_rel_inds`` [k, 2], ``rel_scores`` [k, R] (the
        pair's whole predicate row);
      * "oi" (train_egtr.py:154-174, Open Images evaluator): every pair, ``sbj_obj_inds`` [N*N, 2] (cartesian product in
        row-major order) and ``pred_scores`` [N*N, R].

    The reference copies ``pred_rel`` [N, N, R] (8 MB at N = 200) to the host and runs a full numpy argsort over its
    entries per image (lib/pytorch_misc.py:27-34); here it is one batched ``topk`` on the device and only ``max_topk`` rows
    leave it.  Ties between equal scores may be ordered differently from numpy's argsort (both orders are valid argsorts).
    ``orig_sizes``: [B, 2] (h, w).  Returns a list of dicts of tensors on the outputs' device with the reference's
    ``pred_entry`` keys (+ ``triplet_scores`` for the two top-k modes)."""
    if mode not in ("multiple", "single", "oi"):
        raise ValueError(f"mode must be 'multiple', 'single' or 'oi', got {mode!r}")
    logits, boxes = outputs["logits"], outputs["pred_boxes"]
    rel = torch.clamp(outputs["pred_rel"], 0.0, 1.0)
    if "pred_connectivity" in outputs and outputs["pred_connectivity"] is not None:
        rel = rel * torch.clamp(outputs["pred_connectivity"], 0.0, 1.0)
    B, N, _, R = rel.shape
    obj_scores, pred_classes = torch.max(logits.softmax(-1)[..., :num_labels], -1)         # [B, N]
    sizes = torch.as_tensor(orig_sizes, dtype=torch.float32, device=rel.device).reshape(B, 2)
    cx, cy, w, h = boxes.unbind(-1)
    xyxy = torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], -1)
    scale = torch.stack([sizes[:, 1], sizes[:, 0], sizes[:, 1], sizes[:, 0]], -1)            # (w, h, w, h)
    xyxy = xyxy * scale[:, None, :]
    common = [{"pred_boxes": xyxy[b], "pred_classes": pred_classes[b], "obj_scores": obj_scores[b]} for b in range(B)]
    if mode == "oi":
        ar = torch.arange(N, device=rel.device)
        pairs = torch.cartesian_prod(ar, ar)
        return [dict(c, sbj_obj_inds=pairs, pred_scores=rel[b].reshape(N * N, R)) for b, c in enumerate(common)]
    sub_ob = obj_scores[:, :, None] * obj_scores[:, None, :]
    sub_ob = sub_ob.masked_fill(torch.eye(N, dtype=torch.bool, device=rel.device)[None], 0.0)
    if mode == "single":
        scores = (rel.max(-1)[0] * sub_ob).reshape(B, -1)                                     # [B, N*N]
        k = min(max_topk, scores.shape[1])
        top, flat = torch.topk(scores, k, dim=1)
        s_idx = torch.div(flat, N, rounding_mode="floor")
        o_idx = flat % N
        rows = rel.reshape(B, N * N, R).gather(1, flat[:, :, None].expand(-1, -1, R))         # [B, k, R]
        return [dict(c, pred_rel_inds=torch.stack([s_idx[b], o_idx[b]], -1), rel_scores=rows[b], triplet_scores=top[b])
                for b, c in enumerate(common)]
    scores = (rel * sub_ob.unsqueeze(-1)).reshape(B, -1)
    k = min(max_topk, scores.shape[1])
    top, flat = torch.topk(scores, k, dim=1)                                                  # sorted descending
    s_idx = torch.div(flat, N * R, rounding_mode="floor")
    o_idx = torch.div(flat, R, rounding_mode="floor") % N
    p_idx = flat % R
    rel_scores = rel.reshape(B, -1).gather(1, flat)
    return [dict(c, pred_rel_inds=torch.stack([s_idx[b], o_idx[b], p_idx[b]], -1), rel_scores=rel_scores[b],
                 triplet_scores=top[b]) for b, c in enumerate(common)]


def _matched_queries(outputs, targets, matcher, num_labels):
    """GT object -> query: ``matcher`` (a ``DeformableDetrHungarianMatcher``) on the first ``num_labels`` logits, like every
    evaluator input.  One (pred_idx, tgt_idx) pair of index tensors per image."""
    return matcher({"logits": outputs["logits"][..., :num_labels], "pred_boxes": outputs["pred_boxes"]}, targets)[0]


def _matched_query_of(outputs, targets, matcher, num_labels, Gp):
    """``_matched_queries`` as int32 [B, Gp] on the outputs' device: the query of GT object g, -1 where the object is
    unmatched or padding.  Index writes only: nothing waits for the device."""
    device = outputs["logits"].device
    matched = _matched_queries(outputs, targets, matcher, num_labels)
    query_of = torch.full((len(matched), Gp), -1, dtype=torch.int32, device=device)
    for b, (pred_idx, tgt_idx) in enumerate(matched):
        query_of[b, tgt_idx.to(device).long()] = pred_idx.to(device).int()
    return query_of


@torch.no_grad()
def matched_pair_candidates(outputs, targets, matcher, num_labels):
    """The predicate-detection inputs (``evaluation.PredicateDetectionRecall``) of a model's outputs: "how good are the
    predicates once the objects are found".  Per image, ``matcher`` (a ``DeformableDetrHungarianMatcher``, run on the first
    ``num_labels`` logits like every evaluator input) maps GT objects to queries; ``pred_rel_inds`` [k, 2] is every ordered
    pair (s, o), s != o, of matched GT OBJECT indices in row-major order and ``rel_scores`` [k, R] the rows
    ``clamp(pred_rel) * clamp(pred_connectivity)`` at (query of s, query of o).  With at least as many queries as GT objects
    every GT object is matched and k = G (G - 1).  Returns a list of dicts of tensors on the outputs' device; nothing waits
    for the device (the matched counts are shapes)."""
    rel = torch.clamp(outputs["pred_rel"], 0.0, 1.0)
    if "pred_connectivity" in outputs and outputs["pred_connectivity"] is not None:
        rel = rel * torch.clamp(outputs["pred_connectivity"], 0.0, 1.0)
    device = rel.device
    matched = _matched_queries(outputs, targets, matcher, num_labels)
    out = []
    for b, (pred_idx, tgt_idx) in enumerate(matched):
        n = pred_idx.shape[0]
        k = torch.arange(n * max(n - 1, 0), device=device)          # static shape: nothing waits for the device
        s, o = k // max(n - 1, 1), k % max(n - 1, 1)
        o = o + (o >= s)                                            # row-major over (s, o), the diagonal left out
        order = torch.argsort(tgt_idx.to(device))                   # matched entries in GT-object order
        gt_of, q_of = tgt_idx.to(device)[order], pred_idx.to(device)[order]
        out.append({"pred_rel_inds": torch.stack([gt_of[s], gt_of[o]], -1), "rel_scores": rel[b, q_of[s], q_of[o]]})
    return out


def matched_topk_host(pred_rel, pred_conn, query_of, obj_score, K, mode):
    """The torch twin of ``ops.matched_topk`` (csrc/matched_topk.hip), same arguments, same definition, same outputs, on
    whatever device the tensors live (it reads ``query_of`` on the host).  Per image the domain is every (s, o, p) --
    (s, o) with ``mode`` 1 -- of GT-object indices with s != o and both objects matched (``0 <= query_of < N``);
    ``r = clamp(pred_rel[qs, qo, p]) [* clamp(pred_conn[qs, qo])]``, ``so = obj_score[s] * obj_score[o]``,
    ``score = r * so`` (mode 0) or ``max_p(r) * so`` (mode 1), each product rounded once in float32.  Order: descending
    score key (``evaluation.score_keys_host``: NaN last, -0 = +0), ties by ascending (s, o, p) -- a stable sort of the
    domain in row-major order.  Rows from ``count`` to ``K`` hold index Gp - 1 and score 0."""
    from .evaluation.vrd import score_keys_host
    B, N, _, R = pred_rel.shape
    Gp, K, dev = query_of.shape[1], int(K), pred_rel.device
    cols = 3 if mode == 0 else 2
    inds = torch.full((B, K, cols), Gp - 1, dtype=torch.int64, device=dev)
    rel_scores = torch.zeros((B, K) if mode == 0 else (B, K, R), dtype=torch.float32, device=dev)
    triplet_scores = torch.zeros(B, K, dtype=torch.float32, device=dev)
    count = torch.zeros(B, dtype=torch.int32, device=dev)
    q_host = query_of.cpu().long()
    for b in range(B):
        g = torch.nonzero((q_host[b] >= 0) & (q_host[b] < N)).flatten()          # matched GT objects, ascending
        M = g.numel()
        if M < 2:
            continue
        q, g = q_host[b][g].to(dev), g.to(dev)
        r = torch.clamp(pred_rel[b][q][:, q].float(), 0.0, 1.0)                    # [M, M, R]
        if pred_conn is not None:
            r = r * torch.clamp(pred_conn[b].reshape(N, N)[q][:, q].float(), 0.0, 1.0)[..., None]
        sc = obj_score[b][g].float()
        so = sc[:, None] * sc[None, :]
        off = ~torch.eye(M, dtype=torch.bool, device=dev)
        if mode == 0:
            score = (r * so[..., None])[off]                                       # [M (M - 1), R], row-major
            s_i, o_i = (x[off] for x in torch.meshgrid(g, g, indexing="ij"))
            flat_s, flat_o = s_i[:, None].expand(-1, R).reshape(-1), o_i[:, None].expand(-1, R).reshape(-1)
            flat_p = torch.arange(R, device=dev).expand(s_i.shape[0], R).reshape(-1)
            score, rvals = score.reshape(-1), r[off].reshape(-1)
        else:
            score = (r.max(-1)[0] * so)[off]                                       # [M (M - 1)]
            flat_s, flat_o = (x[off] for x in torch.meshgrid(g, g, indexing="ij"))
            rvals = r[off]                                                          # [M (M - 1), R]
        order = torch.sort(score_keys_host(score), descending=True, stable=True)[1][:K]
        n = order.numel()
        count[b] = n
        inds[b, :n, 0], inds[b, :n, 1] = flat_s[order], flat_o[order]
        if mode == 0:
            inds[b, :n, 2] = flat_p[order]
        rel_scores[b, :n] = rvals[order]
        triplet_scores[b, :n] = score[order]
    return inds, rel_scores, triplet_scores, count


def _pinned_to(t, device):
    """A host tensor on ``device`` without waiting for the stream (a pageable host -> device copy would)."""
    return t.pin_memory().to(device, non_blocking=True) if device.type == "cuda" else t


@torch.no_grad()
def matched_triplet_candidates(outputs, targets, matcher, num_labels, max_topk=100, mode="multiple", protocol="predcls"):
    """The candidate lists of the PredCls and SGCls protocols (lib/evaluation/sg_eval.py:99-106) for a one-stage model: the
    "given boxes" are the GT boxes, and the GT objects are the queries ``matcher`` assigns to them (as in
    ``matched_pair_candidates``).  Per image the ``max_topk`` best entries over the matched queries, scored as
    ``triplet_candidates`` scores them (train_egtr.py:57-69, 86, 122) with
      * "predcls": object scores 1 and the GT classes;
      * "sgcls": score and class of the matched query (softmax over the first ``num_labels`` logits);
    ``mode`` "multiple": (s, o, p) triplets, ``rel_scores`` [K]; "single": (s, o) pairs, ``rel_scores`` [K, R].  The order
    among equal scores is defined (ascending (s, o, p)); self pairs and unmatched objects are not in the list.

    Returns one dict per image with the keys ``SceneGraphRecall.update`` takes, indices in GT-OBJECT numbering, all of one
    shape: Gp = (largest G of the batch) + 1 objects -- ``pred_boxes[:G]`` are the GT boxes of ``evaluation.gt_entry``
    bit for bit, padding objects have a zero box and class -1, an unmatched GT object (G > N) has class -1 -- and
    ``max_topk`` candidate rows, the rows after the image's last entry pointing at object Gp - 1 at both ends: its class
    -1 equals no GT class, so such a row never matches and the recalls are those of the unpadded list.  Device tensors go
    to ``ops.matched_topk`` (csrc/matched_topk.hip), host tensors to ``matched_topk_host``; nothing waits for the
    device."""
    from .evaluation._common import gt_entry
    if mode not in ("multiple", "single"):
        raise ValueError(f"mode must be 'multiple' or 'single', got {mode!r}")
    if protocol not in ("predcls", "sgcls"):
        raise ValueError(f"protocol must be 'predcls' or 'sgcls', got {protocol!r}")
    rel = outputs["pred_rel"]
    conn = outputs["pred_connectivity"] if "pred_connectivity" in outputs else None
    device = rel.device
    B, N = rel.shape[0], rel.shape[1]
    gts = [gt_entry(t) for t in targets]
    Gp = max([g["gt_classes"].shape[0] for g in gts] + [0]) + 1
    boxes = torch.zeros(B, Gp, 4, dtype=torch.float32)
    gt_classes = torch.full((B, Gp), -1, dtype=torch.int64)
    for b, g in enumerate(gts):
        n = g["gt_classes"].shape[0]
        boxes[b, :n], gt_classes[b, :n] = g["gt_boxes"], g["gt_classes"]
    boxes, gt_classes = _pinned_to(boxes, device), _pinned_to(gt_classes, device)
    query_of = _matched_query_of(outputs, targets, matcher, num_labels, Gp)
    is_matched = query_of >= 0
    if protocol == "predcls":
        obj_scores = (gt_classes >= 0).float()
        classes = torch.where(is_matched, gt_classes, -1)
    else:
        q_scores, q_classes = torch.max(outputs["logits"].softmax(-1)[..., :num_labels], -1)          # [B, N]
        at = query_of.clamp(min=0).long()
        obj_scores = torch.where(is_matched, q_scores.float().gather(1, at), 0.0)
        classes = torch.where(is_matched, q_classes.gather(1, at), -1)
    args = (rel.float().contiguous(), None if conn is None else conn.float().contiguous(), query_of,
            obj_scores.contiguous(), max_topk, 0 if mode == "multiple" else 1)
    if device.type == "cpu":
        inds, rel_scores, triplet_scores, _ = matched_topk_host(*args)
    else:
        from . import ops
        with torch.cuda.device(device):
            inds, rel_scores, triplet_scores, _ = ops.matched_topk(*args)
    return [{"pred_boxes": boxes[b], "pred_classes": classes[b], "obj_scores": obj_scores[b], "pred_rel_inds": inds[b],
             "rel_scores": rel_scores[b], "triplet_scores": triplet_scores[b]} for b in range(B)]
