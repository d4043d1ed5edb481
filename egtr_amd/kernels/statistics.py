"""Bindings of the relation-statistics kernels (csrc/rel_stats.hip) and the zero-shot recall pass of the scene-graph
evaluator (csrc/sgg_eval.hip).  The callers (``egtr_amd.statistics``, ``egtr_amd.evaluation.sgg``) own the staging; these
take the device views of the relation layout (``evaluation._common.RelationGT``).  ``egtr_amd.ops`` re-exports every name
below."""
import ctypes

import torch

from .. import _lib
from .._lib import _chk

__all__ = ["rel_stats_count", "rel_seen_bits", "sgg_zero_shot"]


def rel_stats_count(gt, batch, counts, status):
    """egtr_rel_stats_i64: add the rows of the staged batch ``gt`` (its rels / rel_off / classes / box_off) to ``counts``
    int64 [C1, C1, R] in place; ``status`` int32 [1] gets bit 0 for a row that was not counted."""
    _chk(counts, "counts", torch.int64)
    _chk(status, "status", torch.int32)
    _lib.launch("egtr_rel_stats_i64", _lib.ptr(gt.rels), gt.rel_off.data_ptr(), int(gt.T), _lib.ptr(gt.classes),
                gt.box_off.data_ptr(), int(gt.G), int(batch), counts.shape[0], counts.shape[2], counts.data_ptr(),
                status.data_ptr())


def rel_seen_bits(counts):
    """egtr_rel_seen_bits_i64: int64 [ceil(n / 64)] words, bit (i & 63) of word i >> 6 set iff counts.flatten()[i] > 0."""
    _chk(counts, "counts", torch.int64)
    n = counts.numel()
    bits = torch.empty((n + 63) // 64, dtype=torch.int64, device=counts.device)
    _lib.launch("egtr_rel_seen_bits_i64", counts.data_ptr(), n, bits.data_ptr())
    return bits


def sgg_zero_shot(first_rank, gt, batch, num_cand, num_classes, num_rel, seen_bits, ks, acc):
    """egtr_sgg_zero_shot_f64 behind egtr_sgg_eval_f32 on the same stream: ``first_rank`` int32 as that launch wrote it
    for the staged ``gt``; returns the slab float64 [batch, len(ks) + 2] and adds its rows to ``acc`` in image order."""
    _chk(seen_bits, "seen_bits", torch.int64)
    if seen_bits.numel() < (num_classes * num_classes * num_rel + 63) // 64:
        raise ValueError("seen_bits is shorter than num_classes^2 * num_rel bits")
    slab = torch.empty(batch, len(ks) + 2, dtype=torch.float64, device=seen_bits.device)
    _lib.launch("egtr_sgg_zero_shot_f64", first_rank.data_ptr(), _lib.ptr(gt.rels), gt.rel_off.data_ptr(), int(gt.T),
                _lib.ptr(gt.classes), gt.box_off.data_ptr(), int(gt.G), int(batch), int(num_cand), int(num_classes),
                int(num_rel), seen_bits.data_ptr(), (ctypes.c_int * len(ks))(*ks), len(ks), slab.data_ptr(),
                _lib.ptr(acc))
    return slab
