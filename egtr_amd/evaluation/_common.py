"""What the evaluators share: the reference's GT entry and bbox.pyx IoU, the first-rank matching on the host, and the
plumbing every device path needs -- the pinned staging ring, the ragged-GT upload in the relation layout, the lazily
placed accumulator, the argument checks and the record exchange of ``all_gather``."""
import collections

import torch

_MAX_CAND, _MAX_REL, _MAX_K = 1024, 256, 8


def rescale_bboxes(boxes, orig_size):
    """util/box_ops.py:87-91 for a target: normalised cxcywh -> xyxy, then x (w, h, w, h) in float32.
    ``orig_size`` is (h, w) like the targets' ``orig_size``."""
    h, w = orig_size[0], orig_size[1]
    cx, cy, bw, bh = boxes.unbind(-1)
    b = torch.stack([(cx - 0.5 * bw), (cy - 0.5 * bh), (cx + 0.5 * bw), (cy + 0.5 * bh)], dim=-1)
    return b * torch.tensor([w, h, w, h], dtype=torch.float32)


def gt_entry(target):
    """The reference's ``gt_entry`` of one target dict (train_egtr.py:69-80), on the host.  A target with ``rel_triplets``
    and no dense ``rel`` (egtr_amd.targets) gives its distinct rows in lexicographic order: what ``nonzero()`` returns on
    the dense tensor of the same triplets."""
    t = {k: (v.cpu() if torch.is_tensor(v) else torch.as_tensor(v)) for k, v in target.items()}
    if "rel" in t:
        rels = t["rel"].nonzero()
    else:
        rels = t["rel_triplets"].long().reshape(-1, 3)
        rels = torch.unique(rels, dim=0) if rels.shape[0] else rels
    return {"gt_relations": rels,
            "gt_boxes": rescale_bboxes(t["boxes"].float(), t["orig_size"]),
            "gt_classes": t["class_labels"].long()}


def _bbox_iou_pyx(gt, q):
    """bbox.pyx bbox_overlaps (:21-61) between paired rows of gt [..., 4] and q [..., 4] (float64), the same operation
    order as the Cython loop (every torch op rounds: no contraction)."""
    box_area = (q[..., 2] - q[..., 0] + 1) * (q[..., 3] - q[..., 1] + 1)
    iw = torch.minimum(gt[..., 2], q[..., 2]) - torch.maximum(gt[..., 0], q[..., 0]) + 1
    ih = torch.minimum(gt[..., 3], q[..., 3]) - torch.maximum(gt[..., 1], q[..., 1]) + 1
    ua = (gt[..., 2] - gt[..., 0] + 1) * (gt[..., 3] - gt[..., 1] + 1) + box_area - iw * ih
    iou = iw * ih / ua
    return torch.where((iw > 0) & (ih > 0), iou, torch.zeros((), dtype=torch.float64))


def numpy_argmax(rows):
    """numpy ``argmax(1)`` of a float tensor [K, R]: the lowest index among the maxima, the first NaN if any."""
    R = rows.shape[1]
    idx = torch.arange(R, device=rows.device).expand_as(rows)
    nan = rows.isnan()
    first_nan = torch.where(nan, idx, R).min(1).values
    top = rows.masked_fill(nan, float("-inf")).max(1, keepdim=True).values
    first_max = torch.where(rows == top, idx, R).min(1).values
    return torch.where(nan.any(1), first_nan, first_max.clamp(max=R - 1))


def first_ranks_host(pred_rels, pred_boxes, pred_classes, gt_rels, gt_boxes, gt_classes, iou_thresh=0.5):
    """First matching rank of each GT triplet (host, vectorised).  pred_rels [K, 3] (s, o, p) in rank order, pred_boxes
    [N, 4], pred_classes [N], gt_rels [T, 3], gt_boxes [G, 4], gt_classes [G].  Returns int64 [T], K where unmatched."""
    K, T = pred_rels.shape[0], gt_rels.shape[0]
    if K == 0 or T == 0:
        return torch.full((T,), K, dtype=torch.long)
    s, o, p = pred_rels[:, 0], pred_rels[:, 1], pred_rels[:, 2]
    gs, go, gp = gt_rels[:, 0], gt_rels[:, 1], gt_rels[:, 2]
    label = ((pred_classes[s][None, :] == gt_classes[gs][:, None]) & (pred_classes[o][None, :] == gt_classes[go][:, None])
             & (p[None, :] == gp[:, None]))                                                       # [T, K]
    pb, gb = pred_boxes.double(), gt_boxes.double()
    sub = _bbox_iou_pyx(gb[gs][:, None, :], pb[s][None, :, :]) >= iou_thresh
    obj = _bbox_iou_pyx(gb[go][:, None, :], pb[o][None, :, :]) >= iou_thresh
    match = label & sub & obj
    ranks = torch.arange(K).expand(T, K)
    return torch.where(match, ranks, K).min(1).values


def _tensor(x):
    return x if torch.is_tensor(x) else torch.as_tensor(x)


def seen_bits_host(counts):
    """The "occurs in training" bitset of a host count tensor (any shape, read row-major): int64 [ceil(n / 64)], bit
    (i & 63) of word i >> 6 set iff counts.flatten()[i] > 0 -- what egtr_rel_seen_bits_i64 writes (csrc/rel_stats.hip)."""
    seen = (counts.reshape(-1) > 0).long()
    words = (seen.numel() + 63) // 64
    seen = torch.cat([seen, seen.new_zeros(words * 64 - seen.numel())]).view(words, 64)
    weight = torch.ones(64, dtype=torch.int64) << torch.arange(64).clamp(max=62)
    weight[63] = -(1 << 63)     # bit 63 is the sign bit of the word
    return (seen * weight).sum(1)


# ---- argument checks ----------------------------------------------------------------------------------------------------
def check_ks(num_rel_labels, ks):
    """The ``num_rel_labels`` / ``ks`` checks of the relation evaluators; returns ``ks`` as a tuple of ints."""
    ks = tuple(int(k) for k in ks)
    if not 1 <= num_rel_labels <= _MAX_REL:
        raise ValueError(f"num_rel_labels must be in [1, {_MAX_REL}], got {num_rel_labels}")
    if not 1 <= len(ks) <= _MAX_K or any(k < 1 for k in ks) or any(b <= a for a, b in zip(ks, ks[1:])):
        raise ValueError(f"ks must be 1..{_MAX_K} ascending positive values, got {ks}")
    return ks


def check_gt_predicates(g, num_rel):
    """Every GT predicate of one ``gt_entry`` lies in [0, num_rel) (the kernels index per-predicate tables with it)."""
    if g["gt_relations"].numel() and int(g["gt_relations"][:, 2].max()) >= num_rel:
        raise ValueError(f"a GT predicate is outside [0, {num_rel})")


# ---- lazily placed accumulator ------------------------------------------------------------------------------------------
def placed(t, device, shape, dtype):
    """An accumulator that lives on the device of its first use: zeros of ``shape`` there while ``t`` is still None, ``t``
    itself afterwards -- inputs on another device are an error."""
    if t is None:
        return torch.zeros(shape, dtype=dtype, device=device)
    if t.device != device:
        raise ValueError(f"this evaluator accumulates on {t.device}, got inputs on {device}")
    return t


class FlatAccumulator:
    """The flat float64 ``acc`` [width] of the relation evaluators (None until the first use names a device)."""

    def _reset_acc(self, device):
        self.acc = None if device is None else torch.zeros(self.width, dtype=torch.float64, device=device)

    def _acc_on(self, device):
        self.acc = placed(self.acc, device, self.width, torch.float64)
        return self.acc

    def _host_acc(self):
        if self.acc is None:
            return torch.zeros(self.width, dtype=torch.float64)
        return self.acc.cpu()


# ---- host -> device staging of the ragged ground truth --------------------------------------------------------------------
class StagingRing:
    """[pinned buffer, event] slots of the host -> device GT copies of one evaluator."""

    def __init__(self):
        self.slots = []

    def slot(self, nbytes):
        """A pinned staging buffer no in-flight copy still reads: a slot whose event has completed is reused, otherwise
        a new slot is added (event.query() never waits)."""
        for slot in self.slots:
            if slot[0].numel() >= nbytes and slot[1].query():
                return slot
        slot = [torch.empty(max(nbytes, 4096), dtype=torch.uint8, pin_memory=True), torch.cuda.Event()]
        self.slots.append(slot)
        if len(self.slots) > 8:   # drop a finished slot so the ring stays small
            for i, s in enumerate(self.slots[:-1]):
                if s[1].query():
                    del self.slots[i]
                    break
        return slot


def copy_staged(slot, nbytes, device):
    """Start the copy of the first ``nbytes`` of a filled ring slot to a new device buffer and record the slot's event
    behind it; returns the device buffer (uint8 [nbytes]) without waiting."""
    buf, ev = slot
    dev = torch.empty(nbytes, dtype=torch.uint8, device=device)
    dev.copy_(buf[:nbytes], non_blocking=True)
    ev.record()
    return dev


# The relation layout, the byte contract with sgg_eval.hip and oi_eval.hip:
#   int64 [rel_off B+1 | box_off B+1 | rels 3T | classes G], then float32 boxes 4G
# box_off / rels / classes: the int64 indices where those sections start; f32_at: the byte offset of the boxes.
RelationLayout = collections.namedtuple("RelationLayout", "T G box_off rels classes f32_at nbytes")
# an uploaded buffer as the kernels take it, in their argument order (rels, boxes and classes None where T or G is 0)
RelationGT = collections.namedtuple("RelationGT", "rels rel_off T boxes classes box_off G")


def relation_layout(gts):
    """Sizes and section offsets of the relation layout for a batch of ``gt_entry`` dicts."""
    B = len(gts)
    T = sum(g["gt_relations"].shape[0] for g in gts)
    G = sum(g["gt_classes"].shape[0] for g in gts)
    n64 = 2 * (B + 1) + 3 * T + G
    return RelationLayout(T, G, B + 1, 2 * B + 2, 2 * B + 2 + 3 * T, 8 * n64, 8 * n64 + 16 * G)


def pack_relation_gt(gts, lay, buf):
    """Write the batch's ragged GT into the first ``lay.nbytes`` of the uint8 host buffer ``buf`` (pinned or not)."""
    i64 = buf[:lay.f32_at].view(torch.int64)
    f32 = buf[lay.f32_at:lay.nbytes].view(torch.float32)
    rels = [g["gt_relations"] for g in gts]
    i64[:lay.box_off] = torch.tensor([0] + [r.shape[0] for r in rels], dtype=torch.int64).cumsum(0)
    i64[lay.box_off:lay.rels] = torch.tensor([0] + [g["gt_classes"].shape[0] for g in gts], dtype=torch.int64).cumsum(0)
    if lay.T:
        i64[lay.rels:lay.classes] = torch.cat(rels).reshape(-1)
    if lay.G:
        i64[lay.classes:] = torch.cat([g["gt_classes"] for g in gts])
        f32.copy_(torch.cat([g["gt_boxes"] for g in gts]).reshape(-1))


def relation_views(dev, lay):
    """The typed views of a device buffer in the relation layout."""
    d64 = dev[:lay.f32_at].view(torch.int64)
    return RelationGT(d64[lay.rels:lay.classes] if lay.T else None, d64[:lay.box_off], lay.T,
                      dev[lay.f32_at:].view(torch.float32) if lay.G else None, d64[lay.classes:] if lay.G else None,
                      d64[lay.box_off:lay.rels], lay.G)


def upload_relation_gt(ring, gts, device):
    """Pack the batch's GT into a slot of ``ring`` and start its copy to ``device``: the device views, no wait."""
    lay = relation_layout(gts)
    slot = ring.slot(lay.nbytes)
    pack_relation_gt(gts, lay, slot[0])
    return relation_views(copy_staged(slot, lay.nbytes, device), lay)


# ---- record exchange between ranks ----------------------------------------------------------------------------------------
def backend_device(group):
    """The device a collective of ``group`` needs its tensors on."""
    import torch.distributed as dist
    return torch.device("cuda", torch.cuda.current_device()) if dist.get_backend(group) == "nccl" else torch.device("cpu")


def gather_records(rows, group):
    """``rows`` [r, n] (one dtype, on ``backend_device(group)``; n differs between ranks) of every rank of ``group``,
    concatenated along n in rank order: the counts are exchanged, every rank pads to the largest, gathers and trims."""
    import torch.distributed as dist
    world = dist.get_world_size(group)
    n = torch.tensor([rows.shape[1]], dtype=torch.int64, device=rows.device)
    sizes = [torch.zeros_like(n) for _ in range(world)]
    dist.all_gather(sizes, n, group=group)
    sizes = [int(x) for x in sizes]
    buf = torch.zeros(rows.shape[0], max(sizes + [1]), dtype=rows.dtype, device=rows.device)
    buf[:, :rows.shape[1]] = rows
    bufs = [torch.empty_like(buf) for _ in range(world)]
    dist.all_gather(bufs, buf, group=group)
    return torch.cat([b[:, :k] for b, k in zip(bufs, sizes)], 1)
