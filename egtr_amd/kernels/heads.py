"""Bindings of the relation-head forward kernels and their weight packers (csrc/rel_head*.hip), the device matcher
(csrc/matcher.hip), the target packing of the loss kernels and the relation loss on dense / bit-packed targets (csrc/loss.hip,
csrc/rel_targets.hip).  No routing decisions here -- ``egtr_amd.ops`` decides and
re-exports every name below -- but the entries' own size limits: which of the matcher's two entries serves a shape
(``hungarian_match_route``, the limits of csrc/matcher.hip; ``hungarian_match`` and ``DeformableDetrHungarianMatcher.prepare``
both ask it) and whether the large detection-loss entry serves a query count (``detection_loss_large_route``)."""
import torch

from .. import _lib
from .._lib import _chk
from .linear import _split3_bf16

__all__ = ["rel_head_split_weights", "rel_head_streams", "relation_head_split_bf16", "relation_head_train_forward",
           "REL_HEAD_MAX_REL", "REL_HEAD_NARROW_MAX_REL", "rel_head_streams_wide", "relation_head_split_bf16_wide", "hungarian_match",
           "hungarian_match_route", "HUNGARIAN_MAX_SIDE", "HUNGARIAN_LARGE_MAX_TARGETS", "HUNGARIAN_LARGE_MAX_QUERIES",
           "pack_detection_targets", "detection_loss_large_launch", "detection_loss_large_route", "DETECTION_LOSS_LARGE_ROWS",
           "DETECTION_LOSS_LARGE_MAX_QUERIES", "pack_relation_bits", "pack_relation_bits_wide", "relation_loss_launch",
           "relation_loss_all_launch", "relation_loss_policy_launch", "RELATION_POLICIES"]


def _rel_head_pieces(w, terms):
    """[pieces, ...] bf16: the three-way split (terms=6) or the one rounding to nearest even (terms=1) of an fp32 weight"""
    if terms not in (1, 6):
        raise ValueError(f"terms must be 6 (split-bf16, fp32 accuracy) or 1 (operands rounded to bf16), got {terms!r}")
    return _split3_bf16(w) if terms == 6 else w.detach().float().to(torch.bfloat16).unsqueeze(0)


def rel_head_split_weights(w2r, w3r, w2c, terms=6):
    """The MFMA operand streams of rel_head_fwd_x6 (layouts documented in csrc/rel_head.hip):
    w2x [8 nt][16 t][3 piece][64 lane][8] per MLP, w3x [8 nt][2 kb][OT][3 piece][64 lane][8] (relation MLP).
    ``terms=1``: the one-piece streams of the one-term training forward, the same order without the piece dimension --
    w2x [8 nt][16 t][64 lane][8], w3x [8 nt][2 kb][OT][64 lane][8], every element ``weight.to(torch.bfloat16)``."""
    pieces = _rel_head_pieces(w2r, terms).shape[0]

    def w2x(w2):
        p = _rel_head_pieces(w2, terms).view(pieces, 8, 32, 16, 2, 8)   # [piece, nt, pi, t, hf, e]
        p = p.permute(1, 3, 0, 4, 2, 5).contiguous()           # [nt, t, piece, hf, pi, e]; lane = 32 hf + pi
        return p if terms == 6 else p.squeeze(2)

    R = w3r.shape[0]
    OT = 1 if R <= 32 else 2
    w3p = torch.zeros(32 * OT, w3r.shape[1], dtype=torch.float32, device=w3r.device)
    w3p[:R] = w3r.detach().float()
    q = _rel_head_pieces(w3p, terms).view(pieces, OT, 32, w3r.shape[1])   # [piece, ot, pi, n]
    dev = w3r.device
    nt = torch.arange(8, device=dev).view(8, 1, 1, 1)
    kb = torch.arange(2, device=dev).view(1, 2, 1, 1)
    hf = torch.arange(2, device=dev).view(1, 1, 2, 1)
    e = torch.arange(8, device=dev).view(1, 1, 1, 8)
    nidx = 32 * nt + 16 * kb + (e & 3) + 8 * (e >> 2) + 4 * hf  # [nt, kb, hf, e]
    g = q[:, :, :, nidx]                                        # [piece, ot, pi, nt, kb, hf, e]
    w3x = g.permute(3, 4, 1, 0, 5, 2, 6).contiguous()           # [nt, kb, ot, piece, hf, pi, e]
    if terms == 1:
        w3x = w3x.squeeze(3)
    return w2x(w2r), w3x, w2x(w2c)


def rel_head_streams(w2r, w3r, w2c, terms=6):
    """``rel_head_split_weights`` as ONE launch (egtr_rel_head_streams_f32; ``terms=1``: egtr_rel_head_streams_bf16r_f32): the
    same three streams, bit for bit; what the training forward rebuilds after every optimizer step."""
    if terms not in (1, 6):
        raise ValueError(f"terms must be 6 (split-bf16, fp32 accuracy) or 1 (operands rounded to bf16), got {terms!r}")
    w2r_, w3r_, w2c_ = (_chk(t.detach().contiguous(), n, torch.float32)
                        for t, n in ((w2r, "w2r"), (w3r, "w3r"), (w2c, "w2c")))
    R = w3r_.shape[0]
    OT = 1 if R <= 32 else 2
    dev = w2r_.device
    pc = (3,) if terms == 6 else ()
    w2xr = torch.empty(8, 16, *pc, 2, 32, 8, dtype=torch.bfloat16, device=dev)
    w2xc = torch.empty(8, 16, *pc, 2, 32, 8, dtype=torch.bfloat16, device=dev)
    w3x = torch.empty(8, 2, OT, *pc, 2, 32, 8, dtype=torch.bfloat16, device=dev)
    _lib.launch("egtr_rel_head_streams_f32" if terms == 6 else "egtr_rel_head_streams_bf16r_f32", w2r_.data_ptr(),
                w2c_.data_ptr(), w3r_.data_ptr(), w2r_.shape[1], R, w2xr.data_ptr(), w2xc.data_ptr(), w3x.data_ptr())
    return w2xr, w3x, w2xc


def relation_head_train_forward(gate_q, gate_k, uq, uk, b1, w2r, b2r, w3r, b3r, w2c, b2c, w3c, b3c, triplet_dist, node_cls,
                                want_gate_mean, terms, streams=None):
    """Training forward of the relation head with layers 2 and 3 on the bf16 matrix cores: ``terms=6`` the six-term split
    product, fp32 to the last bit (egtr_rel_head_forward_bf16x6_save_f32); ``terms=1`` one product per element, activations and
    weights rounded once to bf16 (egtr_rel_head_forward_bf16r_save_f32).  Contiguous fp32 device tensors, hidden = 256,
    num_rel <= 64, 4 or 7 slots (the entries answer EGTR_E_UNSUPPORTED otherwise: a RuntimeError here).  The weight streams are
    rebuilt by one launch (``rel_head_streams``) unless ``streams`` = (w2x_rel, w3x_rel, w2x_conn) of the same ``terms`` is
    given.  Returns (rel [B, N, N, R], conn [B, N, N], gate_mean [T] or None, h1s, h2s [2, B N N, 256]: the fp32 post-ReLU
    activations of both layers and both MLPs).  No autograd, reads no switch."""
    tens = [_chk(t, n, torch.float32) for t, n in zip(
        (gate_q, gate_k, uq, uk, b1, w2r, b2r, w3r, b3r, w2c, b2c, w3c, b3c),
        ("gate_q", "gate_k", "uq", "uk", "b1", "w2r", "b2r", "w3r", "b3r", "w2c", "b2c", "w3c", "b3c"))]
    gq_, gk_, uq_, uk_, b1_, w2r_, b2r_, w3r_, b3r_, w2c_, b2c_, w3c_, b3c_ = tens
    B, N, T = gq_.shape
    Hd, R = w2r_.shape[1], w3r_.shape[0]
    dev = gq_.device
    w2xr, w3x, w2xc = rel_head_streams(w2r_, w3r_, w2c_, terms=terms) if streams is None else streams
    if streams is not None:
        pc = (3,) if terms == 6 else ()
        OT = 1 if R <= 32 else 2
        for t, n, shape in ((w2xr, "w2x_rel", (8, 16, *pc, 2, 32, 8)), (w2xc, "w2x_conn", (8, 16, *pc, 2, 32, 8)),
                            (w3x, "w3x_rel", (8, 2, OT, *pc, 2, 32, 8))):
            _chk(t, n, torch.bfloat16)
            if tuple(t.shape) != shape:
                raise RuntimeError(f"{n} must have shape {shape} for terms={terms}, got {tuple(t.shape)}")
    c1 = 0
    if triplet_dist is not None:
        _chk(triplet_dist, "triplet_dist", torch.float32)
        _chk(node_cls, "node_cls", torch.int64)
        c1 = triplet_dist.shape[0]
    rel = torch.empty(B, N, N, R, dtype=torch.float32, device=dev)
    conn = torch.empty(B, N, N, dtype=torch.float32, device=dev)
    gm = torch.zeros(T, dtype=torch.float32, device=dev) if want_gate_mean else None
    h1s = torch.empty(2, B * N * N, Hd, dtype=torch.float32, device=dev)
    h2s = torch.empty(2, B * N * N, Hd, dtype=torch.float32, device=dev)
    _lib.launch("egtr_rel_head_forward_bf16x6_save_f32" if terms == 6 else "egtr_rel_head_forward_bf16r_save_f32",
                gq_.data_ptr(), gk_.data_ptr(), uq_.data_ptr(), uk_.data_ptr(),
                b1_.data_ptr(), w2xr.data_ptr(), b2r_.data_ptr(), w3x.data_ptr(), b3r_.data_ptr(), w2xc.data_ptr(),
                b2c_.data_ptr(), w3c_.data_ptr(), b3c_.data_ptr(), _lib.ptr(triplet_dist),
                _lib.ptr(node_cls if triplet_dist is not None else None), B, N, T, Hd, R, c1, rel.data_ptr(),
                conn.data_ptr(), _lib.ptr(gm), h1s.data_ptr(), h2s.data_ptr())
    return rel, conn, gm, h1s, h2s


def relation_head_split_bf16(gate_q, gate_k, uq, uk, b1, w2x_rel, b2r, w3x_rel, b3r, w2x_conn, b2c, w3c, b3c,
                             num_rel, triplet_dist=None, node_cls=None, want_gate_mean=False, sigmoid=False):
    """Inference forward, fp32 in / fp32 out, layers 2 and 3 on the bf16 matrix cores from split operands
    (egtr_rel_head_forward_bf16x6_f32; ``w2x_*`` / ``w3x_rel`` from ``rel_head_split_weights``).  No autograd."""
    B, N, T = gate_q.shape
    dev = gate_q.device
    f32 = [_chk(t.detach().contiguous(), n, torch.float32)
           for t, n in ((gate_q, "gate_q"), (gate_k, "gate_k"), (uq, "uq"), (uk, "uk"), (b1, "b1"), (b2r, "b2r"),
                        (b3r, "b3r"), (b2c, "b2c"), (w3c, "w3c"), (b3c, "b3c"))]
    gq, gk, uq_, uk_, b1_, b2r_, b3r_, b2c_, w3c_, b3c_ = f32
    R = int(num_rel)
    OT = 1 if R <= 32 else 2
    for t, n, shape in ((w2x_rel, "w2x_rel", (8, 16, 3, 2, 32, 8)), (w2x_conn, "w2x_conn", (8, 16, 3, 2, 32, 8)),
                        (w3x_rel, "w3x_rel", (8, 2, OT, 3, 2, 32, 8))):
        _chk(t, n, torch.bfloat16)
        if tuple(t.shape) != shape:
            raise RuntimeError(f"{n} must have shape {shape}, got {tuple(t.shape)}")
    rel = torch.empty(B, N, N, R, dtype=torch.float32, device=dev)
    conn = torch.empty(B, N, N, dtype=torch.float32, device=dev)
    gm = torch.zeros(T, dtype=torch.float32, device=dev) if want_gate_mean else None
    td = None
    c1 = 0
    if triplet_dist is not None:
        td = _chk(triplet_dist.detach().contiguous(), "triplet_dist", torch.float32)
        _chk(node_cls, "node_cls", torch.int64)
        c1 = td.shape[0]
    _lib.launch("egtr_rel_head_forward_bf16x6_f32", gq.data_ptr(), gk.data_ptr(), uq_.data_ptr(), uk_.data_ptr(),
                b1_.data_ptr(), w2x_rel.data_ptr(), b2r_.data_ptr(), w3x_rel.data_ptr(), b3r_.data_ptr(), w2x_conn.data_ptr(),
                b2c_.data_ptr(), w3c_.data_ptr(), b3c_.data_ptr(), _lib.ptr(td), _lib.ptr(node_cls if td is not None else None),
                B, N, T, 256, R, c1, rel.data_ptr(), conn.data_ptr(), _lib.ptr(gm), 1 if sigmoid else 0)
    return rel, conn.unsqueeze(-1), gm


REL_HEAD_NARROW_MAX_REL = 64    # every entry but the wide ones
REL_HEAD_MAX_REL = 256          # egtr_rel_head_forward_wide_f32 / _wide_bf16x6_f32 (the evaluators' kEvalMaxRel)


def rel_head_streams_wide(w2r, w3r, w2c):
    """The operand streams of egtr_rel_head_forward_wide_bf16x6_f32 in one launch (egtr_rel_head_streams_wide_f32), num_rel <=
    256: w2x [8 nt][16 t][3 piece][2 hf][32 pi][8] per MLP as ``rel_head_streams``, and the relation output weights in the SAME
    order, w3x [OT][16 t][3 piece][2 hf][32 pi][8] = piece(W3)[32 ot + pi][16 t + 8 hf + e], OT = ceil(num_rel / 32), rows
    beyond num_rel zero."""
    w2r_, w3r_, w2c_ = (_chk(t.detach().contiguous(), n, torch.float32)
                        for t, n in ((w2r, "w2r"), (w3r, "w3r"), (w2c, "w2c")))
    R = w3r_.shape[0]
    dev = w2r_.device
    w2xr = torch.empty(8, 16, 3, 2, 32, 8, dtype=torch.bfloat16, device=dev)
    w2xc = torch.empty(8, 16, 3, 2, 32, 8, dtype=torch.bfloat16, device=dev)
    w3x = torch.empty((R + 31) // 32, 16, 3, 2, 32, 8, dtype=torch.bfloat16, device=dev)
    _lib.launch("egtr_rel_head_streams_wide_f32", w2r_.data_ptr(), w2c_.data_ptr(), w3r_.data_ptr(), w2r_.shape[1], R,
                w2xr.data_ptr(), w2xc.data_ptr(), w3x.data_ptr())
    return w2xr, w3x, w2xc


def relation_head_split_bf16_wide(gate_q, gate_k, uq, uk, b1, w2x_rel, b2r, w3x_rel, b3r, w2x_conn, b2c, w3c, b3c,
                                  num_rel, triplet_dist=None, node_cls=None, want_gate_mean=False, sigmoid=False):
    """``relation_head_split_bf16`` for up to 256 predicate classes (egtr_rel_head_forward_wide_bf16x6_f32; the streams from
    ``rel_head_streams_wide``).  No autograd."""
    B, N, T = gate_q.shape
    dev = gate_q.device
    f32 = [_chk(t.detach().contiguous(), n, torch.float32)
           for t, n in ((gate_q, "gate_q"), (gate_k, "gate_k"), (uq, "uq"), (uk, "uk"), (b1, "b1"), (b2r, "b2r"),
                        (b3r, "b3r"), (b2c, "b2c"), (w3c, "w3c"), (b3c, "b3c"))]
    gq, gk, uq_, uk_, b1_, b2r_, b3r_, b2c_, w3c_, b3c_ = f32
    R = int(num_rel)
    for t, n, shape in ((w2x_rel, "w2x_rel", (8, 16, 3, 2, 32, 8)), (w2x_conn, "w2x_conn", (8, 16, 3, 2, 32, 8)),
                        (w3x_rel, "w3x_rel", ((R + 31) // 32, 16, 3, 2, 32, 8))):
        _chk(t, n, torch.bfloat16)
        if tuple(t.shape) != shape:
            raise RuntimeError(f"{n} must have shape {shape}, got {tuple(t.shape)}")
    rel = torch.empty(B, N, N, R, dtype=torch.float32, device=dev)
    conn = torch.empty(B, N, N, dtype=torch.float32, device=dev)
    gm = torch.zeros(T, dtype=torch.float32, device=dev) if want_gate_mean else None
    td = None
    c1 = 0
    if triplet_dist is not None:
        td = _chk(triplet_dist.detach().contiguous(), "triplet_dist", torch.float32)
        _chk(node_cls, "node_cls", torch.int64)
        c1 = td.shape[0]
    _lib.launch("egtr_rel_head_forward_wide_bf16x6_f32", gq.data_ptr(), gk.data_ptr(), uq_.data_ptr(), uk_.data_ptr(),
                b1_.data_ptr(), w2x_rel.data_ptr(), b2r_.data_ptr(), w3x_rel.data_ptr(), b3r_.data_ptr(), w2x_conn.data_ptr(),
                b2c_.data_ptr(), w3c_.data_ptr(), b3c_.data_ptr(), _lib.ptr(td), _lib.ptr(node_cls if td is not None else None),
                B, N, T, 256, R, c1, rel.data_ptr(), conn.data_ptr(), _lib.ptr(gm), 1 if sigmoid else 0)
    return rel, conn.unsqueeze(-1), gm


HUNGARIAN_MAX_SIDE = 1024              # egtr_hungarian_match_f32: max(N, T)
HUNGARIAN_LARGE_MAX_TARGETS = 512      # egtr_hungarian_match_large_f32: T < N, T <= 512, N <= 65 536
HUNGARIAN_LARGE_MAX_QUERIES = 65536


def hungarian_match_route(num_query, max_targets):
    """Which entry serves ``num_query`` queries against at most ``max_targets`` targets per image (the limits of
    csrc/matcher.hip, one place for ``hungarian_match`` and ``DeformableDetrHungarianMatcher.prepare``): ``"small"``
    (egtr_hungarian_match_f32, everything up to 1024 a side), ``"large"`` (egtr_hungarian_match_large_f32, proposal-sized
    query sets) or ``None`` (neither: the caller keeps the host route)."""
    if max(num_query, max_targets) <= HUNGARIAN_MAX_SIDE:
        return "small"
    if max_targets < num_query <= HUNGARIAN_LARGE_MAX_QUERIES and max_targets <= HUNGARIAN_LARGE_MAX_TARGETS:
        return "large"
    return None


@torch.no_grad()
def hungarian_match(logits, pred_boxes, targets, class_cost, bbox_cost, giou_cost, cost_min=None,
                    inverse_sigmoid_smoothing=None, cost_in=None, want_cost=False, want_status=False, large=None):
    """DeformableDetrHungarianMatcher.forward on the device (egtr_hungarian_match_f32): cost matrix + linear sum
    assignment per image in one launch, nothing copied to the host (the reference's ``.cpu()`` at dd:2985 is a device
    synchronisation per step).  ``targets``: list of dicts with "class_labels" / "boxes" (device tensors); their COUNTS
    are host integers (tensor shapes), so output shapes are static.  ``cost_min`` / ``inverse_sigmoid_smoothing``: the two
    fp32 scalars of the adaptive-smoothing offset (dd:2992-2998) or None.  ``cost_in``: per-image [N, T_b] cost matrices
    to solve instead (tests).  Returns (pred_idx, tgt_idx, match_cost) flat device tensors + the per-image counts
    [+ cost blocks] [+ status]: entries of image b are sorted by query index, i.e. scipy's output order.
    ``large``: None routes by size (``hungarian_match_route``), True forces egtr_hungarian_match_large_f32 (any N > T;
    tests reach its edges at small sizes this way), False the one-wave entry.  Same tuple, same bits."""
    lib = _lib.lib()
    if cost_in is not None:
        B = len(cost_in)
        N = cost_in[0].shape[0]
        dev = cost_in[0].device
        sizes = [int(c.shape[1]) for c in cost_in]
        cin = torch.cat([_chk(c.contiguous(), "cost_in", torch.float32).reshape(-1) for c in cost_in]) \
            if sum(sizes) else torch.zeros(1, device=dev)
        K = 0
        lg = bx = ti = tb = None
    else:
        B, N, K = logits.shape
        dev = logits.device
        sizes = [int(t["boxes"].shape[0]) for t in targets]
        lg = _chk(logits.detach().contiguous(), "logits", torch.float32)
        bx = _chk(pred_boxes.detach().contiguous(), "pred_boxes", torch.float32)
        ti = torch.cat([t["class_labels"] for t in targets]).to(device=dev, dtype=torch.int64).contiguous()
        tb = torch.cat([t["boxes"] for t in targets]).to(device=dev, dtype=torch.float32).contiguous()
        cin = None
    n_out = [min(N, t) for t in sizes]
    offs = [0]
    for t in sizes:
        offs.append(offs[-1] + t)
    ooffs = [0]
    for t in n_out:
        ooffs.append(ooffs[-1] + t)
    meta = torch.tensor(offs + ooffs, dtype=torch.int32).to(dev, non_blocking=True)   # two small host -> device copies
    tot = max(ooffs[-1], 1)
    pred_idx = torch.empty(tot, dtype=torch.int64, device=dev)
    tgt_idx = torch.empty(tot, dtype=torch.int64, device=dev)
    mcost = torch.empty(tot, dtype=torch.float32, device=dev)
    cost_out = torch.empty(max(N * offs[-1], 1), dtype=torch.float32, device=dev) if want_cost else None
    status = torch.zeros(B, dtype=torch.int32, device=dev) if want_status else None
    smooth = 1 if cost_min is not None else 0
    max_t = max(sizes, default=0)
    if large is None:
        large = hungarian_match_route(N, max_t) == "large"
    common = (_lib.ptr(lg), _lib.ptr(bx), ti.data_ptr() if ti is not None and ti.numel() else None,
              tb.data_ptr() if tb is not None and tb.numel() else None, meta.data_ptr(), meta.data_ptr() + 4 * (B + 1),
              B, N, K, max_t, float(class_cost), float(bbox_cost), float(giou_cost), smooth,
              float(cost_min) if smooth else 0.0, float(inverse_sigmoid_smoothing) if smooth else 0.0,
              pred_idx.data_ptr(), tgt_idx.data_ptr(), mcost.data_ptr(), _lib.ptr(cost_out), _lib.ptr(cin),
              _lib.ptr(status))
    if large and max_t > 0:
        n_ws = lib.egtr_hungarian_match_large_workspace_bytes(B, N, max_t, offs[-1])
        if n_ws <= 0:
            raise _lib.EgtrHipError(f"egtr_hungarian_match_large_f32 serves T < N, T <= {HUNGARIAN_LARGE_MAX_TARGETS}, "
                                    f"N <= {HUNGARIAN_LARGE_MAX_QUERIES}; got N = {N}, T = {max_t}")
        workspace = torch.empty(n_ws, dtype=torch.uint8, device=dev)
        _lib.launch("egtr_hungarian_match_large_f32", *common, workspace.data_ptr(), n_ws)
    elif max_t > 0:
        n_scr = lib.egtr_hungarian_match_scratch_doubles(N, max_t, offs[-1])
        scratch = torch.empty(n_scr, dtype=torch.float64, device=dev) if n_scr > 0 else None
        _lib.launch("egtr_hungarian_match_f32", *common, _lib.ptr(scratch))
    out =[pred_idx[:ooffs[-1]], tgt_idx[:ooffs[-1]], mcost[:ooffs[-1]], n_out]
    if want_cost:
        out.append([cost_out[N * offs[i]: N * offs[i + 1]].view(N, sizes[i]) for i in range(B)])
    if want_status:
        out.append(status)
    return tuple(out)


def pack_detection_targets(targets, device):
    """Concatenated class labels / boxes of a batch + per-image offsets, built once per step and shared by the output
    sets (main + auxiliary) of ``detection_losses``."""
    sizes = [int(t["class_labels"].shape[0]) for t in targets]
    offs = [0]
    for n in sizes:
        offs.append(offs[-1] + n)
    if offs[-1]:
        labels = torch.cat([t["class_labels"] for t in targets]).to(device=device, dtype=torch.int64).contiguous()
        boxes = torch.cat([t["boxes"] for t in targets]).to(device=device, dtype=torch.float32).contiguous()
    else:   # keep the kernel's pointers valid
        labels = torch.zeros(1, dtype=torch.int64, device=device)
        boxes = torch.zeros(1, 4, dtype=torch.float32, device=device)
    toff = torch.tensor(offs, dtype=torch.int32).to(device, non_blocking=True)
    lengths = torch.tensor(sizes, dtype=torch.float32).to(device, non_blocking=True)
    return labels, boxes, toff, lengths


DETECTION_LOSS_LARGE_ROWS = 32             # loss.hip: kDetLargeRows, the query rows one workgroup owns
DETECTION_LOSS_LARGE_MAX_QUERIES = 65536   # loss.hip: kDetLargeMaxN (= HUNGARIAN_LARGE_MAX_QUERIES)


def detection_loss_large_route(num_query):
    """Whether an output set of ``num_query`` queries may take egtr_detection_loss_large_f32 (the entry's own bound; the
    criteria ask it at call time, so an A/B run can take the decision away)."""
    return 1 <= num_query <= DETECTION_LOSS_LARGE_MAX_QUERIES


def detection_loss_large_launch(logits, pred_boxes, pred_idx, tgt_idx, match_off, tgt_labels, tgt_boxes, tgt_off,
                                focal_alpha, num_boxes, want_grad=True):
    """egtr_detection_loss_large_f32 on an output set of up to 65 536 queries.  ``tgt_labels`` None: class-agnostic targets
    (every matched query's class is 0).  Returns (out [B, 4], grad_logits, grad_boxes_l1, grad_boxes_giou); with
    ``want_grad=False`` the value-only launch, the three gradients None and never allocated."""
    B, N, C = logits.shape
    lg = _chk(logits, "logits", torch.float32)
    bx = _chk(pred_boxes, "pred_boxes", torch.float32)
    n_ws = _lib.lib().egtr_detection_loss_large_workspace_bytes(B, N, C)
    if n_ws <= 0:
        raise _lib.EgtrHipError(f"egtr_detection_loss_large_f32 serves 1 <= N <= {DETECTION_LOSS_LARGE_MAX_QUERIES}, "
                                f"C >= 1, N * C < 2^31; got B = {B}, N = {N}, C = {C}")
    dev = lg.device
    workspace = torch.empty((n_ws + 7) // 8, dtype=torch.float64, device=dev)
    out = torch.empty(B, 4, dtype=torch.float32, device=dev)
    d_logits = torch.empty_like(lg) if want_grad else None
    d_l1 = torch.empty_like(bx) if want_grad else None
    d_giou = torch.empty_like(bx) if want_grad else None
    _lib.launch("egtr_detection_loss_large_f32", lg.data_ptr(), bx.data_ptr(), pred_idx.data_ptr(), tgt_idx.data_ptr(),
                match_off.data_ptr(), _lib.ptr(tgt_labels), tgt_boxes.data_ptr(), tgt_off.data_ptr(), B, N, C,
                float(focal_alpha), float(num_boxes), _lib.ptr(d_logits), _lib.ptr(d_l1), _lib.ptr(d_giou), out.data_ptr(),
                workspace.data_ptr())
    return out, d_logits, d_l1, d_giou


def pack_relation_bits(triplets, offsets, batch, total, num_query, num_rel):
    """egtr_pack_relations_u64: concatenated device triplets int64 [total, 3] + int32 offsets [batch + 1] -> the words
    int64 [batch, N, N] (bit p of word (s, o) set iff (s, o, p) is a triplet).  ``egtr_amd.targets.pack_relations`` is the
    public route (host checks, the single pinned copy)."""
    _chk(triplets, "triplets", torch.int64)
    _chk(offsets, "offsets", torch.int32)
    bits = torch.empty(batch, num_query, num_query, dtype=torch.int64, device=triplets.device)
    _lib.launch("egtr_pack_relations_u64", triplets.data_ptr(), offsets.data_ptr(), int(batch), int(total), int(num_query),
                int(num_rel), bits.data_ptr())
    return bits


def pack_relation_bits_wide(triplets, offsets, batch, total, num_query, num_rel):
    """egtr_pack_relations_wide_u64: the same operands -> the words int64 [batch, N, N, W], W = ceil(num_rel / 64), for up to
    256 predicates (bit p & 63 of word (s, o, p >> 6)).  ``egtr_amd.targets.pack_relations_wide`` is the public route."""
    _chk(triplets, "triplets", torch.int64)
    _chk(offsets, "offsets", torch.int32)
    bits = torch.empty(batch, num_query, num_query, (int(num_rel) + 63) // 64, dtype=torch.int64, device=triplets.device)
    _lib.launch("egtr_pack_relations_wide_u64", triplets.data_ptr(), offsets.data_ptr(), int(batch), int(total),
                int(num_query), int(num_rel), bits.data_ptr())
    return bits


def _target_format(target, packed, B, N, R):
    """The EGTR_REL_TARGET_* code of ``target``: 0 (pointer table), 1 (words [B, N, N]) or 2 (words [B, N, N, W],
    W = ceil(R / 64)) -- the rank of the words selects the form."""
    if not packed:
        return 0
    _chk(target, "rel_bits", torch.int64)
    if target.dim() == 4:
        if tuple(target.shape) != (B, N, N, (R + 63) // 64):
            raise RuntimeError(f"wide rel_bits must have shape {(B, N, N, (R + 63) // 64)}, got {tuple(target.shape)}")
        return 2
    if tuple(target.shape) != (B, N, N):
        raise RuntimeError(f"rel_bits must have shape {(B, N, N)}, got {tuple(target.shape)}")
    return 1


def relation_loss_launch(pred_rel, pred_conn, target, packed, pred_idx, tgt_idx, match_cost, out_off, nonmatching_cost,
                         sample_negatives, sample_nonmatching, deterministic=False):
    """``relation_loss_policy_launch`` with the ``sample_*`` largest logits of both classes: what the criterion trains with."""
    return relation_loss_policy_launch(pred_rel, pred_conn, target, packed, pred_idx, tgt_idx, match_cost, out_off,
                                       nonmatching_cost, ("largest", sample_negatives), ("largest", sample_nonmatching),
                                       deterministic=deterministic)


def relation_loss_all_launch(pred_rel, pred_conn, target, packed, pred_idx, tgt_idx, match_cost, out_off, nonmatching_cost,
                             want_grad=True):
    """egtr_relation_loss_all_f32: the un-sampled relation loss -- BCE over all N N R elements -- and the connectivity loss;
    ``target`` as in ``relation_loss_policy_launch``.  Returns (loss [2], grad_rel, grad_conn); ``want_grad=False`` is the
    value-only launch: no gradient buffer is allocated or written, both come back None."""
    B, N, _, R = pred_rel.shape
    dev = pred_rel.device
    fmt = _target_format(target, packed, B, N, R)
    loss = torch.empty(2, dtype=torch.float32, device=dev)
    grad_rel = torch.empty_like(pred_rel) if want_grad else None
    grad_conn = torch.empty_like(pred_conn) if want_grad else None
    ws = torch.empty(int(_lib.lib().egtr_relation_loss_all_workspace_bytes(B, N)), dtype=torch.uint8, device=dev)
    _lib.launch("egtr_relation_loss_all_f32", pred_rel.data_ptr(), pred_conn.data_ptr(), target.data_ptr(), fmt,
                pred_idx.data_ptr(), tgt_idx.data_ptr(), match_cost.data_ptr(), out_off.data_ptr(), B, N, R,
                float(nonmatching_cost), loss.data_ptr(), _lib.ptr(grad_rel), _lib.ptr(grad_conn), ws.data_ptr())
    return loss, grad_rel, grad_conn


RELATION_POLICIES = {"largest": 0, "random": 1, "all": 2}   # the policy codes of egtr_relation_loss_f32


def relation_loss_policy_launch(pred_rel, pred_conn, target, packed, pred_idx, tgt_idx, match_cost, out_off, nonmatching_cost,
                                negatives, nonmatching, seed=0, stream=0, deterministic=False):
    """egtr_relation_loss_f32: one sampling policy per candidate class.  ``target``: the device table of per-image pointers to
    dense fp32 targets or, with ``packed``, the words int64 [B, N, N] / [B, N, N, ceil(R / 64)].  ``negatives`` /
    ``nonmatching``: (policy, count) with policy "largest" | "random" | "all" (the count of "all" is ignored; None there).
    ``seed`` / ``stream``: the 64-bit words of a random class's keys, reduced modulo 2^64.  ``deterministic``: ties at the
    selection threshold of a "largest" class taken lowest flat index first.  Returns (loss [2], grad_rel, grad_conn)."""
    B, N, _, R = pred_rel.shape
    dev = pred_rel.device
    fmt = _target_format(target, packed, B, N, R)
    codes, counts = [], []
    for name, (policy, count) in (("negatives", negatives), ("nonmatching", nonmatching)):
        if policy not in RELATION_POLICIES:
            raise ValueError(f"{name}: policy must be one of {tuple(RELATION_POLICIES)}, got {policy!r}")
        if policy != "all" and (count is None or int(count) < 0):
            raise ValueError(f"{name}: a {policy!r} class takes a count >= 0, got {count!r}")
        codes.append(RELATION_POLICIES[policy])
        counts.append(0 if policy == "all" else int(count))

    def s64(v):   # any Python int -> the signed 64-bit value with the same low 64 bits
        v = int(v) & 0xFFFFFFFFFFFFFFFF
        return v - (1 << 64) if v >= (1 << 63) else v

    loss = torch.empty(2, dtype=torch.float32, device=dev)
    grad_rel = torch.empty_like(pred_rel)
    grad_conn = torch.empty_like(pred_conn)
    ws = torch.empty(int(_lib.lib().egtr_relation_loss_workspace_bytes(B, N)), dtype=torch.uint8, device=dev)
    _lib.launch("egtr_relation_loss_f32", pred_rel.data_ptr(), pred_conn.data_ptr(), target.data_ptr(), fmt,
                pred_idx.data_ptr(), tgt_idx.data_ptr(), match_cost.data_ptr(), out_off.data_ptr(), B, N, R,
                float(nonmatching_cost), counts[0], counts[1], loss.data_ptr(), grad_rel.data_ptr(), grad_conn.data_ptr(),
                ws.data_ptr(), codes[0], codes[1], s64(seed), s64(stream), 1 if deterministic else 0)
    return loss, grad_rel, grad_conn
