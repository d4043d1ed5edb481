"""Relation targets as triplet lists and bit-packed words.

The reference's dataset turns an image's relation triplets into a dense fp32 ``[num_queries, num_queries, 50]`` tensor on
the host (data/visual_genome.py:74-80): 8 MB per image at N = 200 for a few dozen ones.  A target dict may carry the triplets
themselves instead:

  ``"rel_triplets"``  int64 [K, 3] rows (subject, object, predicate); the predicate is zero-based after the ``no_relation``
                      category is removed (the values ``_get_rel_tensor`` indexes with).  K may be 0; a duplicated row means
                      the same as one occurrence (the reference's indexed assignment).

A dict that has ``"rel"`` is read as before, whatever else it carries.  Below the public interface the triplets become
``rel_bits``: int64 [B, N, N] read as unsigned, bit p of word [b, s, o] set iff (s, o, p) is a triplet of image b (a target
value is 0 or 1).  The loss kernels read the words (csrc/loss.hip, target format 1 of egtr_relation_loss_f32); ``unpack_relations`` gives the
dense tensor back to the routes that evaluate the reference's tensor composition.

A word holds 64 predicates.  A larger vocabulary (``MAX_REL_LABELS`` < ``num_rel_labels`` <= ``MAX_PACKED_REL_LABELS``, the
relation head's 256) takes WIDE words (``pack_relations_wide``): int64 [B, N, N, W] with W = ceil(R / 64), bit p & 63 of word
[b, s, o, p >> 6], bits at positions >= R zero; with W = 1 the memory is that of the [B, N, N] words.  The loss kernels read them
as target format 2 of the sampled and the un-sampled loss entry under either tie rule, so no dense target is built there
either (0.64 MB per image at N = 200, R = 100 where the dense tensor has 16 MB).  Beyond 256 predicates there are no words:
``dense_targets`` materialises the triplets as the dense tensor directly (``materialize_relations``) and the criterion takes the
dense target format, which is generic in R."""
import torch

from .kernels.heads import pack_relation_bits, pack_relation_bits_wide

__all__ = ["MAX_REL_LABELS", "MAX_PACKED_REL_LABELS", "relation_triplets", "has_dense", "pack_relations", "pack_relations_wide",
           "unpack_relations", "materialize_relations", "dense_targets"]

MAX_REL_LABELS = 64            # predicates in one word: the limit of ``pack_relations``
MAX_PACKED_REL_LABELS = 256    # predicates in the wide words: the limit of ``pack_relations_wide``
_INT64_MIN = -(1 << 63)


def relation_triplets(rel_list):
    """A ``rel.json`` entry (rows (subject, object, predicate) with ONE-based predicates, 0 = ``no_relation``) as the
    ``"rel_triplets"`` tensor: int64 [K, 3], zero-based predicates."""
    t = torch.as_tensor(rel_list, dtype=torch.int64).reshape(-1, 3).clone()
    t[:, 2] -= 1
    return t


def has_dense(targets):
    """Every target of the batch carries the dense ``"rel"`` tensor (which wins over ``"rel_triplets"``)."""
    return all("rel" in t for t in targets)


def _triplets_of(target):
    if "rel_triplets" not in target:
        raise KeyError('a target needs "rel" (dense fp32 [N, N, R]) or "rel_triplets" (int64 [K, 3])')
    t = target["rel_triplets"]
    if t.dim() != 2 or t.shape[1] != 3 or t.dtype != torch.int64:
        raise ValueError(f"rel_triplets must be int64 [K, 3], got {t.dtype} {tuple(t.shape)}")
    return t


def _check_host(t, b, N, R):
    if t.numel() == 0:
        return
    lo, hi = t.min(0).values.tolist(), t.max(0).values.tolist()
    if min(lo) < 0 or hi[0] >= N or hi[1] >= N or hi[2] >= R:
        raise ValueError(f"rel_triplets of image {b}: an index is outside [0, {N}) x [0, {N}) x [0, {R})")


def _bit(p):
    """1 << p as int64 for p in [0, 64): bit 63 is the sign bit (a shift by 63 would overflow)."""
    return torch.where(p == 63, torch.full_like(p, _INT64_MIN), torch.ones_like(p) << p.clamp(max=62))


def _gather(targets, N, R):
    """The batch's triplet tensors, their offsets and the total; host triplets checked (ValueError)."""
    trips = [_triplets_of(t) for t in targets]
    offs = [0]
    for t in trips:
        offs.append(offs[-1] + int(t.shape[0]))
    for b, t in enumerate(trips):
        if not t.is_cuda:
            _check_host(t, b, N, R)
    return trips, offs, offs[-1]


def _compose(trips, total, B, N, R, W, device):
    """The words as a tensor composition (the CPU route): flat int64 [B N N W]."""
    bits = torch.zeros(B * N * N * W, dtype=torch.int64, device=device)
    if total:
        t = torch.cat([x.to(device) for x in trips])
        img = torch.repeat_interleave(torch.arange(B, device=device),
                                      torch.tensor([x.shape[0] for x in trips], device=device))
        ok = ((t >= 0).all(1) & (t[:, 0] < N) & (t[:, 1] < N) & (t[:, 2] < R))   # (device rows moved here: the kernel's guard)
        rows = torch.unique(torch.cat([img[ok, None], t[ok]], 1), dim=0)         # distinct (b, s, o, p): a sum of bits is an OR
        if rows.numel():
            bits.index_add_(0, ((rows[:, 0] * N + rows[:, 1]) * N + rows[:, 2]) * W + (rows[:, 3] >> 6),
                            _bit(rows[:, 3] & 63))
    return bits


def _stage(trips, offs, total, B, device):
    """(triplets int64 [total, 3], offsets int32 [B + 1]) on ``device``: host triplets and their offsets in ONE pinned buffer,
    copied once; triplets that already live on a device are concatenated there."""
    if all(not t.is_cuda for t in trips):
        n_off = 2 * ((B + 4) // 4)   # int32 [B + 1] at the head of the int64 buffer, padded to 16 bytes
        host = torch.zeros(n_off + max(total, 1) * 3, dtype=torch.int64, pin_memory=True)
        host[:n_off].view(torch.int32)[:B + 1] = torch.tensor(offs, dtype=torch.int32)
        if total:
            torch.cat(trips, out=host[n_off:].view(total, 3))
        buf = host.to(device, non_blocking=True)
        return buf[n_off:], buf[:n_off].view(torch.int32)
    trip_d = (torch.cat([t.to(device) for t in trips]) if total
              else torch.zeros(1, 3, dtype=torch.int64, device=device)).contiguous()
    return trip_d, torch.tensor(offs, dtype=torch.int32).to(device, non_blocking=True)


def pack_relations(targets, num_queries, num_rel_labels, device):
    """``rel_bits`` int64 [B, N, N] on ``device`` from the targets' ``"rel_triplets"``.  Host triplets are checked on the host
    (ValueError for an index out of range), concatenated with their offsets in ONE pinned buffer and copied once; triplets
    that already live on a device are not read back -- the pack kernel drops a row with an index out of range.  On a GPU
    the words are built by egtr_pack_relations_u64 (one memset, one launch, no synchronisation), on the CPU by the tensor
    composition of the same words."""
    N, R = int(num_queries), int(num_rel_labels)
    if not 1 <= R <= MAX_REL_LABELS:
        raise ValueError(f"packed relation targets hold at most {MAX_REL_LABELS} predicates per pair, got {R}")
    device = torch.device(device)
    trips, offs, total = _gather(targets, N, R)
    B = len(trips)
    if device.type != "cuda":
        return _compose(trips, total, B, N, R, 1, device).view(B, N, N)
    trip_d, off_d = _stage(trips, offs, total, B, device)
    with torch.cuda.device(device):
        return pack_relation_bits(trip_d, off_d, B, total, N, R)


def pack_relations_wide(targets, num_queries, num_rel_labels, device):
    """Wide ``rel_bits`` int64 [B, N, N, W] with W = ceil(R / 64), for 1 <= R <= ``MAX_PACKED_REL_LABELS``: bit p & 63 of word
    [b, s, o, p >> 6] set iff (s, o, p) is a triplet of image b, bits at positions >= R zero.  Everything else is
    ``pack_relations``: host triplets checked (ValueError), one pinned copy, egtr_pack_relations_wide_u64 on a GPU, the tensor
    composition of the same words on the CPU.  With W = 1 the words are ``pack_relations(...)[..., None]``."""
    N, R = int(num_queries), int(num_rel_labels)
    if not 1 <= R <= MAX_PACKED_REL_LABELS:
        raise ValueError(f"wide packed relation targets hold 1 to {MAX_PACKED_REL_LABELS} predicates per pair, got {R}")
    W = (R + 63) // 64
    device = torch.device(device)
    trips, offs, total = _gather(targets, N, R)
    B = len(trips)
    if device.type != "cuda":
        return _compose(trips, total, B, N, R, W, device).view(B, N, N, W)
    trip_d, off_d = _stage(trips, offs, total, B, device)
    with torch.cuda.device(device):
        return pack_relation_bits_wide(trip_d, off_d, B, total, N, R)


def unpack_relations(rel_bits, b, num_rel_labels):
    """The dense fp32 [N, N, R] target of image ``b`` (what ``_get_rel_tensor`` builds), on the device of ``rel_bits``: the
    words [B, N, N] or the wide words [B, N, N, W]."""
    R = int(num_rel_labels)
    if rel_bits.dim() == 4:
        W = rel_bits.shape[3]
        if W != (R + 63) // 64:
            raise ValueError(f"wide rel_bits hold {W} words per pair, {R} predicates need {(R + 63) // 64}")
        shifts = torch.arange(64, dtype=torch.int64, device=rel_bits.device)
        dense = ((rel_bits[b].unsqueeze(-1) >> shifts) & 1).to(torch.float32)   # [N, N, W, 64]
        return dense.flatten(2)[..., :R].contiguous()
    shifts = torch.arange(R, dtype=torch.int64, device=rel_bits.device)
    return ((rel_bits[b].unsqueeze(-1) >> shifts) & 1).to(torch.float32)


def materialize_relations(target, b, num_queries, num_rel_labels, device):
    """The dense fp32 [N, N, R] target of ONE image (index ``b`` in its batch, for the message) from its ``"rel_triplets"``, any
    R: one zero fill, one indexed write, no synchronisation.  Host triplets are checked like ``pack_relations`` checks them
    (ValueError); a row that already lives on a device and has an index out of range is dropped, like the pack kernel's guard
    -- it is written to a spare element behind the tensor."""
    N, R = int(num_queries), int(num_rel_labels)
    t = _triplets_of(target)
    if not t.is_cuda:
        _check_host(t, b, N, R)
    flat = torch.zeros(N * N * R + 1, dtype=torch.float32, device=device)
    if t.shape[0]:
        t = t.to(device)
        ok = (t >= 0).all(1) & (t[:, 0] < N) & (t[:, 1] < N) & (t[:, 2] < R)
        flat.index_fill_(0, torch.where(ok, (t[:, 0] * N + t[:, 1]) * R + t[:, 2], N * N * R), 1.0)
    return flat[:N * N * R].view(N, N, R)


def dense_targets(targets, num_queries, num_rel_labels, device, rel_bits=None):
    """The targets with a dense ``"rel"`` each: a target that already has one is passed through, the others get theirs from
    the packed words (``rel_bits`` of the whole batch when the caller already packed it).  For the routes that evaluate the
    reference's tensor composition; N N R floats per image.  ``rel_bits`` may be the words [B, N, N] or the wide words
    [B, N, N, W].  More than ``MAX_REL_LABELS`` predicates and no words given: straight from the triplets
    (``materialize_relations``), the same values."""
    if has_dense(targets):
        return targets
    if rel_bits is None and int(num_rel_labels) > MAX_REL_LABELS:
        return [t if "rel" in t else dict(t, rel=materialize_relations(t, i, num_queries, num_rel_labels, device))
                for i, t in enumerate(targets)]
    if rel_bits is None:
        missing = [i for i, t in enumerate(targets) if "rel" not in t]
        rel_bits = pack_relations([targets[i] for i in missing], num_queries, num_rel_labels, device)
        where = {i: j for j, i in enumerate(missing)}
    else:
        where = {i: i for i in range(len(targets))}
    return [t if "rel" in t else dict(t, rel=unpack_relations(rel_bits, where[i], num_rel_labels))
            for i, t in enumerate(targets)]
