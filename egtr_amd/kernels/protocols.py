"""Binding of the PredCls / SGCls candidate builder (csrc/matched_topk.hip).  The caller
(``egtr_amd.runtime.matched_triplet_candidates``) owns the matching and the dict format; this validates, allocates the
outputs and the workspace and launches one C entry on torch's current stream.  ``egtr_amd.ops`` re-exports every name
below."""
import torch

from .. import _lib
from .._lib import _chk

__all__ = ["matched_topk", "MATCHED_TOPK_MAX_K", "MATCHED_TOPK_MAX_REL"]

MATCHED_TOPK_MAX_K = 1024      # matched_topk.hip: kMaxK (the evaluators' _MAX_CAND)
MATCHED_TOPK_MAX_REL = 256     # matched_topk.hip: kMaxRel


def matched_topk(pred_rel, pred_conn, query_of, obj_score, K, mode):
    """egtr_matched_topk_f32: ``pred_rel`` float32 [B, N, N, R], ``pred_conn`` float32 [B, N, N] (or [B, N, N, 1]) or None,
    ``query_of`` int32 [B, Gp] (-1 = unmatched or padding), ``obj_score`` float32 [B, Gp], ``mode`` 0 (multiple predicates
    per pair) or 1 (one entry per pair).  Returns (inds int64 [B, K, 3 | 2], rel_scores float32 [B, K] | [B, K, R],
    triplet_scores float32 [B, K], count int32 [B]); the order and the padding rows are defined in include/egtr_hip.h."""
    _chk(pred_rel, "pred_rel", torch.float32)
    _chk(query_of, "query_of", torch.int32)
    _chk(obj_score, "obj_score", torch.float32)
    if pred_rel.dim() != 4 or pred_rel.shape[1] != pred_rel.shape[2]:
        raise ValueError(f"pred_rel must be [B, N, N, R], got {tuple(pred_rel.shape)}")
    B, N, _, R = pred_rel.shape
    if pred_conn is not None:
        _chk(pred_conn, "pred_connectivity", torch.float32)
        if pred_conn.numel() != B * N * N:
            raise ValueError(f"pred_connectivity must hold [B, N, N] values, got {tuple(pred_conn.shape)}")
    if query_of.dim() != 2 or query_of.shape[0] != B or query_of.shape != obj_score.shape:
        raise ValueError("query_of and obj_score must both be [B, Gp]")
    Gp, K, mode = query_of.shape[1], int(K), int(mode)
    if not 1 <= K <= MATCHED_TOPK_MAX_K or not 1 <= R <= MATCHED_TOPK_MAX_REL or N < 1 or Gp < 1 or mode not in (0, 1):
        raise ValueError(f"matched_topk: K in [1, {MATCHED_TOPK_MAX_K}], R in [1, {MATCHED_TOPK_MAX_REL}], N, Gp >= 1, "
                         f"mode 0 or 1; got K={K}, R={R}, N={N}, Gp={Gp}, mode={mode}")
    dev = pred_rel.device
    inds = torch.empty(B, K, 3 if mode == 0 else 2, dtype=torch.int64, device=dev)
    rel_scores = torch.empty((B, K) if mode == 0 else (B, K, R), dtype=torch.float32, device=dev)
    triplet_scores = torch.empty(B, K, dtype=torch.float32, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    nbytes = _lib.lib().egtr_matched_topk_workspace_bytes(B, Gp, K)
    workspace = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    _lib.launch("egtr_matched_topk_f32", pred_rel.data_ptr(), _lib.ptr(pred_conn), query_of.data_ptr(),
                obj_score.data_ptr(), B, N, R, Gp, K, mode, workspace.data_ptr(), inds.data_ptr(), rel_scores.data_ptr(),
                triplet_scores.data_ptr(), count.data_ptr())
    return inds, rel_scores, triplet_scores, count
