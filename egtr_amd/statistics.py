"""Training-set relation statistics: the ``fg_matrix`` the frequency bias and the logit adjustment are
built from, counted where the targets live.

The reference fills it with Python loops over its dataset classes (data/visual_genome.py:84-118 ``vg_get_statistics``,
data/open_image.py:161-185 ``oi_get_statistics``): ``fg_matrix[class[s], class[o], p] += 1`` for every relation row of every
training image, an int64 array [num_labels + 1, num_labels + 1, num_rel_labels] (the last row and column stay zero for
Visual Genome).  ``RelationStatistics`` accumulates the same array from target dicts as the collate produces them:

  ``class_labels``  [n], zero-based;
  ``rel_triplets``  int64 [K, 3] rows (subject index, object index, zero-based predicate) -- EVERY ROW AS GIVEN counts, a
                    duplicated row twice, as in both reference loops (the loss reads a duplicate as one occurrence,
                    ``egtr_amd.targets``; the statistics do not);
  ``rel``           dense [N, N, R] instead (it wins when both are present, as everywhere): one count per non-zero entry.

State on a GPU: one thread per row and a 64-bit integer atomic add (csrc/rel_stats.hip, ``egtr_rel_stats_i64``) -- integer
addition is order-free, so the counts are deterministic.  Host targets go through the evaluators' pinned ``StagingRing`` in
their relation layout (``evaluation/_common.py``; the box section carries zeros), device tensors are used where they are.
A row with an index, class or predicate out of range is NOT counted and raises a sticky status word, which ``update`` polls
without waiting and ``finalize()`` / ``fg_matrix()`` / ``seen_bits()`` turn into a ``ValueError``.  State on the CPU: the
same semantics in vectorised torch (``index_put_`` with ``accumulate=True``); a bad row raises at once and leaves the counts
as they were.
"""
import torch

from .evaluation._common import (RelationGT, StagingRing, backend_device, copy_staged, placed, seen_bits_host,
                                 upload_relation_gt)
from .kernels.statistics import rel_seen_bits, rel_stats_count

__all__ = ["RelationStatistics"]


def _rows_of(target):
    """(classes int64 [n], rows int64 [K, 3]) of one target dict, on the devices its tensors are on."""
    if "class_labels" not in target:
        raise KeyError('a target needs "class_labels"')
    classes = torch.as_tensor(target["class_labels"]).long().reshape(-1)
    if "rel" in target:
        rows = torch.as_tensor(target["rel"]).nonzero()
        if rows.shape[1] != 3:
            raise ValueError(f"rel must be [N, N, R], got {tuple(target['rel'].shape)}")
    elif "rel_triplets" in target:
        rows = torch.as_tensor(target["rel_triplets"])
        if rows.dim() != 2 or rows.shape[1] != 3 or rows.dtype != torch.int64:
            raise ValueError(f"rel_triplets must be int64 [K, 3], got {rows.dtype} {tuple(rows.shape)}")
    else:
        raise KeyError('a target needs "rel" (dense [N, N, R]) or "rel_triplets" (int64 [K, 3])')
    return classes, rows


class RelationStatistics:
    """``counts`` int64 [num_labels + 1, num_labels + 1, num_rel_labels]: the reference's ``fg_matrix``, accumulated by
    ``update(targets)``.  ``device``: where the counts live; None = where the tensors of the first ``update`` are (host
    targets: the CPU).  ``merge`` / ``all_reduce`` add instances; ``fg_matrix()`` is the host numpy array
    ``DetrForSceneGraphGeneration(config, fg_matrix=...)`` takes; ``seen_bits()`` the bitset of the zero-shot recall."""

    def __init__(self, num_labels, num_rel_labels, device=None):
        if num_labels < 1 or num_rel_labels < 1:
            raise ValueError(f"num_labels and num_rel_labels must be positive, got {num_labels}, {num_rel_labels}")
        self.num_labels, self.num_rel = int(num_labels), int(num_rel_labels)
        self.shape = (self.num_labels + 1, self.num_labels + 1, self.num_rel)
        self._ring = StagingRing()
        self.reset(device)

    # ---- state -----------------------------------------------------------------------------------------------------
    def reset(self, device=None):
        self.counts = None if device is None else torch.zeros(self.shape, dtype=torch.int64, device=device)
        self._status = None      # int32 [1] on the device of the counts (GPU state only)
        self._pending = None     # (pinned int32 host word, event) of the last asynchronous poll
        self._bad = False        # a finished poll saw the status word set
        self._host_word = None

    def _counts_on(self, device):
        self.counts = placed(self.counts, device, self.shape, torch.int64)
        if self.counts.is_cuda and self._status is None:
            self._status = torch.zeros(1, dtype=torch.int32, device=self.counts.device)
        return self.counts

    def merge(self, other):
        """Add another instance's counts (same num_labels / num_rel_labels) into this one."""
        if other.shape != self.shape:
            raise ValueError("merge needs statistics with the same num_labels and num_rel_labels")
        if other.counts is not None:
            self._counts_on(other.counts.device).add_(other.counts)
            if other._status is not None:
                self._status.bitwise_or_(other._status)
        self._bad |= other._bad
        return self

    def all_reduce(self, group=None):
        """Sum the counts over the ranks of ``group`` (one collective on the flat tensor).  No-op when torch.distributed
        is not initialised."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return self
        if self.counts is None:
            self._counts_on(backend_device(group))
        dist.all_reduce(self.counts.view(-1), op=dist.ReduceOp.SUM, group=group)
        return self

    # ---- update ----------------------------------------------------------------------------------------------------
    def update(self, targets):
        """Count the relation rows of a batch of target dicts.  With GPU state nothing is copied back and nothing waits
        (dense ``rel`` tensors that live on a device are the exception: ``nonzero()`` has to learn their row count)."""
        if not targets:
            return
        pairs = [_rows_of(t) for t in targets]
        if self.counts is not None:
            device = self.counts.device
        else:
            on_gpu = [x.device for cr in pairs for x in cr if x.is_cuda]
            device = on_gpu[0] if on_gpu else torch.device("cpu")
        if device.type == "cpu":
            self._update_host(pairs)
        else:
            self._update_device(pairs, device)

    def _update_host(self, pairs):
        counts = self._counts_on(torch.device("cpu"))
        C1, R = self.shape[0], self.shape[2]
        rows = torch.cat([r.cpu() for _, r in pairs])
        if rows.shape[0] == 0:
            return
        classes = torch.cat([c.cpu() for c, _ in pairs])
        n_rows = torch.tensor([r.shape[0] for _, r in pairs])
        n_obj = torch.tensor([c.shape[0] for c, _ in pairs])
        first = torch.repeat_interleave(n_obj.cumsum(0) - n_obj, n_rows)    # the row's image's first object
        limit = torch.repeat_interleave(n_obj, n_rows)
        s, o, p = rows.unbind(1)
        if not bool(((s >= 0) & (s < limit) & (o >= 0) & (o < limit) & (p >= 0) & (p < R)).all()):
            raise ValueError(f"a relation row has an object index outside its image or a predicate outside [0, {R})")
        cs, co = classes[first + s], classes[first + o]
        if not bool(((cs >= 0) & (cs < C1) & (co >= 0) & (co < C1)).all()):
            raise ValueError(f"a relation row refers to a class outside [0, {C1})")
        counts.view(-1).index_put_(((cs * C1 + co) * R + p,), torch.ones_like(p), accumulate=True)

    def _update_device(self, pairs, device):
        counts = self._counts_on(device)
        B = len(pairs)
        if all(not x.is_cuda for cr in pairs for x in cr):
            # the evaluators' ragged GT upload; its box section (16 bytes per object) carries zeros
            gts = [{"gt_relations": r, "gt_classes": c, "gt_boxes": torch.zeros(c.shape[0], 4)} for c, r in pairs]
            gt = upload_relation_gt(self._ring, gts, device)
        else:
            # tensors that already live on the device stay there: only the 2 (B + 1) offsets go through the ring
            offs = torch.tensor([[0] + [r.shape[0] for _, r in pairs], [0] + [c.shape[0] for c, _ in pairs]],
                                dtype=torch.int64).cumsum(1)
            T, G = int(offs[0, -1]), int(offs[1, -1])
            nbytes = 16 * (B + 1)
            slot = self._ring.slot(nbytes)
            slot[0][:nbytes].view(torch.int64).copy_(offs.reshape(-1))
            dev = copy_staged(slot, nbytes, device).view(torch.int64)
            rels = torch.cat([r.to(device, non_blocking=True) for _, r in pairs]).contiguous() if T else None
            classes = torch.cat([c.to(device, non_blocking=True) for c, _ in pairs]).contiguous() if G else None
            gt = RelationGT(rels, dev[:B + 1], T, None, classes, dev[B + 1:], G)
        with torch.cuda.device(device):
            rel_stats_count(gt, B, counts, self._status)
        self._poll()

    # ---- status ----------------------------------------------------------------------------------------------------
    def _poll(self):
        """Look at the status word without stalling the stream: the verdict of the previous asynchronous copy is read once
        its event has completed, then a new copy is queued."""
        if self._pending is not None:
            host, event = self._pending
            if not event.query():
                return
            self._bad |= bool(host[0])
            self._pending = None
        if self._status is not None and not self._bad:
            if self._host_word is None:   # one pinned word per instance: at most one copy is in flight
                self._host_word = torch.empty(1, dtype=torch.int32, pin_memory=True)
            host = self._host_word
            host.copy_(self._status, non_blocking=True)
            event = torch.cuda.Event()
            event.record(torch.cuda.current_stream(self._status.device))
            self._pending = (host, event)

    def finalize(self):
        """Wait for the updates and raise ``ValueError`` if a row was left out of the counts; returns self."""
        if self._status is not None and not self._bad:
            self._bad = bool(self._status.item())
            self._pending = None
        if self._bad:
            raise ValueError("RelationStatistics: a relation row had an object index outside its image, a class outside "
                             f"[0, {self.shape[0]}) or a predicate outside [0, {self.shape[2]}); it was not counted")
        return self

    # ---- results ---------------------------------------------------------------------------------------------------
    def fg_matrix(self):
        """The counts as a host numpy int64 array [num_labels + 1, num_labels + 1, num_rel_labels]: what
        ``vg_get_statistics`` / ``oi_get_statistics`` return for the same relation rows."""
        self.finalize()
        if self.counts is None:
            return torch.zeros(self.shape, dtype=torch.int64).numpy()
        return self.counts.cpu().numpy()

    def seen_bits(self):
        """int64 [ceil(C1 * C1 * R / 64)] where the counts live: bit (i & 63) of word i >> 6 is set iff the count at the
        row-major position i of (subject class, object class, predicate) is greater than zero."""
        self.finalize()
        if self.counts is None:
            return seen_bits_host(torch.zeros(self.shape, dtype=torch.int64))
        if self.counts.is_cuda:
            with torch.cuda.device(self.counts.device):
                return rel_seen_bits(self.counts)
        return seen_bits_host(self.counts)
