"""Shared test helpers: build the product model for a golden fixture."""
import json
import os

import numpy as np
import torch

import weights as W


def product_config(cfg_dict):
    from egtr_amd.deformable_detr import DeformableDetrConfig
    base_keys = ("num_queries", "encoder_layers", "decoder_layers", "dropout", "auxiliary_loss", "with_box_refine", "two_stage",
                 "two_stage_num_proposals")
    cfg = DeformableDetrConfig(**{k: cfg_dict[k] for k in base_keys if k in cfg_dict})
    for k, v in cfg_dict.items():
        if k not in base_keys:
            setattr(cfg, k, v)
    return cfg


def build_product_model(cfg_dict, shapes, seed, stub_backbone=True, device="cpu"):
    """Product DetrForSceneGraphGeneration with the fixture's seeded weights (and the fixtures' stub backbone)."""
    import egtr_amd.deformable_detr as pdd
    from egtr_amd.egtr import DetrForSceneGraphGeneration
    import _ref_import
    cfg = product_config(cfg_dict)
    fg = W.fg_matrix(cfg.num_labels, cfg.num_rel_labels, seed=0)
    orig = pdd.DeformableDetrTimmConvEncoder
    if stub_backbone:
        pdd.DeformableDetrTimmConvEncoder = _ref_import.make_stub_backbone_class()
    try:
        model = DetrForSceneGraphGeneration(cfg, fg_matrix=fg)
    finally:
        pdd.DeformableDetrTimmConvEncoder = orig
    sd = W.fill_state_dict(shapes, seed=seed, alias_heads=not cfg_dict.get("with_box_refine", False))
    sd["triplet_dist"], sd["rel_dist"] = W.freq_bias_tables(fg, cfg.freq_bias_eps)
    return model, cfg, sd


def small_inputs(g):
    rng = W.rng_inputs(int(g["input_seed"]))
    B, H, Wd = 2, int(g["H"]), int(g["W"])
    pv = torch.from_numpy(rng.standard_normal((B, 3, H, Wd))).float()
    pm = torch.ones(B, H, Wd, dtype=torch.long)
    vh, vw = [int(v) for v in g["valid1"]]
    pm[1, vh:, :] = 0
    pm[1, :, vw:] = 0
    pv[1] = pv[1] * pm[1][None].float()
    return pv, pm


def load_golden(golden_dir, name):
    return np.load(os.path.join(golden_dir, name), allow_pickle=False)


def product_heads(model, pv, pm):
    """Product forward returning the PRE-sigmoid relation / connectivity logits (egtr:402-416) next to the detection
    outputs: the north-star's 1e-3 bar is stated on logits, and saturated sigmoids would hide logit error."""
    with torch.no_grad():
        outputs = model.model(pv, pixel_mask=pm, output_attentions=False, output_hidden_states=True,
                              output_attention_states=True, return_dict=True)
        enc, last = outputs.encoder_last_hidden_state, outputs.last_hidden_state
        logits, boxes, _, _, rel, conn, _, _ = model._heads(outputs, want_gate_mean=False)
    return dict(logits=logits, pred_boxes=boxes, rel_logits=rel, conn_logits=conn, last_hidden=last, enc=enc,
                inter=outputs.intermediate_hidden_states, inter_ref=outputs.intermediate_reference_points)


def rel_mlp_from_logits(rel_logits, logits, triplet_dist):
    """rel_logits - frequency bias (egtr:405-413), the bias indexed by the SAME tensor's argmax classes: what the
    reference's ``rel_predictor`` hook captured before the bias was added."""
    node = logits.argmax(-1)
    bias = torch.stack([triplet_dist[n][:, n] for n in node])
    return rel_logits - bias


def padded_inputs(g, B, dtype=torch.float32):
    rng = W.rng_inputs(int(g["input_seed"]))
    H, Wd = int(g["H"]), int(g["W"])
    pv = torch.from_numpy(rng.standard_normal((B, 3, H, Wd))).float()
    pm = torch.ones(B, H, Wd, dtype=torch.long)
    vh, vw = [int(v) for v in g["valid1"]]
    pm[1, vh:, :] = 0
    pm[1, :, vw:] = 0
    pv[1] = pv[1] * pm[1][None].float()
    return pv.to(dtype), pm


def check_pred_entry(got, g, j, atol=1e-6, prefix="pred"):
    """``got``: one image's entry (numpy arrays) with the reference's pred_entry keys (+ optional triplet_scores);
    ``g``: tests/golden/postprocess.npz (outputs of the reference's own evaluate_batch, train_egtr.py:43-106).
    Rows are index-exact wherever the triplet score is unique; inside a group of exactly tied scores any order is a
    valid argsort (numpy's quicksort order is not a specification), so tie groups are compared as sets -- except the
    LAST group, which the top-k cut may truncate differently: there only membership in the full tie class counts."""
    want_inds, want_rel = g[f"{prefix}{j}_pred_rel_inds"], g[f"{prefix}{j}_rel_scores"]
    gi = np.asarray(got["pred_rel_inds"])
    assert gi.shape == want_inds.shape
    assert np.array_equal(np.asarray(got["pred_classes"]), g[f"{prefix}{j}_pred_classes"])
    assert np.abs(np.asarray(got["obj_scores"]) - g[f"{prefix}{j}_obj_scores"]).max() < atol
    assert np.abs(np.asarray(got["pred_boxes"]) - g[f"{prefix}{j}_pred_boxes"]).max() < 1e-3
    ts = np.asarray(got["triplet_scores"], dtype=np.float64)
    assert np.all(ts[:-1] >= ts[1:]), "triplets must come in descending score order"
    # group rows by (exactly) equal triplet score
    starts = [0] + [i for i in range(1, len(ts)) if ts[i] != ts[i - 1]] + [len(ts)]
    n_exact = 0
    for a, b in zip(starts[:-1], starts[1:]):
        last = b == len(ts)
        if b - a == 1 and not last:
            assert tuple(gi[a]) == tuple(want_inds[a]), (a, gi[a], want_inds[a])
            assert np.abs(np.asarray(got["rel_scores"][a], dtype=np.float64) - want_rel[a]).max() < atol
            n_exact += 1
        elif not last:
            assert set(map(tuple, gi[a:b])) == set(map(tuple, want_inds[a:b])), (a, b)
    return n_exact


def check_oi_entry(got, g, j, atol=1e-6):
    """One image's Open Images entry (numpy arrays, train_egtr.py:154-174) against postprocess_branches.npz."""
    ps, inds = np.asarray(got["pred_scores"]), np.asarray(got["sbj_obj_inds"])
    assert tuple(ps.shape) == tuple(g[f"oi{j}_pred_scores_shape"]) and inds.shape == (ps.shape[0], 2)
    assert np.abs(ps[::97] - g[f"oi{j}_pred_scores_strided"]).max() < atol
    assert abs(ps.astype(np.float64).sum() - float(g[f"oi{j}_pred_scores_sum"])) < 1e-6 * abs(float(g[f"oi{j}_pred_scores_sum"]))
    assert np.array_equal(inds[::97], g[f"oi{j}_sbj_obj_inds_strided"])
    assert int((inds.astype(np.int64) * np.array([1000003, 7])).sum()) == int(g[f"oi{j}_sbj_obj_inds_checksum"])
    assert np.array_equal(np.asarray(got["pred_classes"]), g[f"oi{j}_pred_classes"])
    assert np.abs(np.asarray(got["obj_scores"]) - g[f"oi{j}_obj_scores"]).max() < atol
    assert np.abs(np.asarray(got["pred_boxes"]) - g[f"oi{j}_pred_boxes"]).max() < 1e-3


def build_product_detector(cfg_dict, shapes, seed, device="cpu"):
    """Product DeformableDetrForObjectDetection with the det_small fixture's seeded weights (stub backbone)."""
    import egtr_amd.deformable_detr as pdd
    import _ref_import
    cfg = product_config(cfg_dict)
    orig = pdd.DeformableDetrTimmConvEncoder
    pdd.DeformableDetrTimmConvEncoder = _ref_import.make_stub_backbone_class()
    try:
        model = pdd.DeformableDetrForObjectDetection(cfg)
    finally:
        pdd.DeformableDetrTimmConvEncoder = orig
    sd = W.fill_state_dict(shapes, seed=seed, alias_heads=not cfg_dict.get("with_box_refine", False))
    return model, cfg, sd


def det_inputs(g, seed):
    rng = W.rng_inputs(seed + 1)
    B, H, Wd = 2, int(g["H"]), int(g["W"])
    pv = torch.from_numpy(rng.standard_normal((B, 3, H, Wd))).float()
    pm = torch.ones(B, H, Wd, dtype=torch.long)
    vh, vw = [int(v) for v in g["valid1"]]
    pm[1, vh:, :] = 0
    pm[1, :, vw:] = 0
    pv[1] = pv[1] * pm[1][None].float()
    return pv, pm


# ---- the split-bf16 ("x6") arithmetic restated on the host (egtr_amd/csrc/xs_format.h, x6_common.h) -------------------------
# A piece is an fp32 tensor whose low 16 bits are zero, i.e. a bf16 value.  bf16 shares fp32's exponent range, so its smallest
# step is 2^-133: three 8-bit pieces hold all 24 bits of an fp32 x exactly only while x's last bit is >= 2^-133, i.e.
# |x| >= 2^-110.  Below that (fp32 denormals included) the bits under 2^-133 are lost by any three-bf16 representation.
SIX_TERMS = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))      # (weight piece, activation piece), x6::mfma6's order
SMALL_TERMS = ((2, 0), (0, 2), (1, 1))                             # w_lo a_hi, w_hi a_lo, w_mid a_mid
# the small terms a paired operand family (``paired_operands``) resolves.  The third is exactly ZERO there -- "act": a_hi is equal
# and w_lo opposite within a pair, "wgt": w_hi equal and a_lo opposite -- so leaving it out changes nothing; the two families
# together cover all three.
RESOLVED_TERMS = {"act": ((0, 2), (1, 1)), "wgt": ((2, 0), (1, 1))}


def _f32_bits(x):
    return x.contiguous().view(torch.int32).to(torch.int64) & 0xffffffff


def _bits_f32(u):
    u = u & 0xffffffff
    return torch.where(u >= 2 ** 31, u - 2 ** 32, u).to(torch.int32).view(torch.float32)


def _trunc_bf16(x):
    return _bits_f32(_f32_bits(x) & 0xffff0000)


def _rne_bf16(x):
    u = _f32_bits(x)
    mag = u & 0x7fffffff
    r = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    r = torch.where(mag > 0x7f800000, torch.full_like(u, 0x7fc00000), torch.where(mag == 0x7f800000, u, r))
    return _bits_f32(r)


def split3_trunc(x):
    """xs::split3 of an activation: hi = the upper 16 bits of x, mid = the upper 16 bits of the exact residual x - hi, lo = the
    rest (x - hi) - mid as the bf16 that is stored (its upper 16 bits: the whole of it while |x| >= 2^-110).  A non-finite x
    keeps the inf / a quiet NaN in hi alone."""
    assert x.dtype == torch.float32
    u = _f32_bits(x)
    fin = (u & 0x7f800000) != 0x7f800000
    hi = _bits_f32(torch.where((u & 0x7fffffff) > 0x7f800000, torch.full_like(u, 0x7fc00000), u & 0xffff0000))
    r = torch.where(fin, x - hi, torch.zeros_like(x))            # exact: hi is x with its low bits cleared
    mid = _trunc_bf16(r)
    lo = _trunc_bf16(r - mid)                                      # r - mid: exact
    return hi, mid, lo


def split3_rne(w):
    """xs::split3_rne of a weight: every piece the bf16 nearest (ties to even) to what the pieces before it left over; the
    residuals are exact in fp32."""
    assert w.dtype == torch.float32
    fin = (_f32_bits(w) & 0x7f800000) != 0x7f800000
    hi = _rne_bf16(w)
    r1 = torch.where(fin, w - hi, torch.zeros_like(w))
    mid = _rne_bf16(r1)
    lo = _rne_bf16(r1 - mid)
    return hi, mid, lo


def term_sum(op, a_pieces, w_pieces, terms, cache=None):
    """sum over (wi, ai) in ``terms`` of op(a_pieces[ai], w_pieces[wi]) in fp64, ``op`` a LINEAR operator of each argument (a
    matrix product, a convolution).  ``cache``: a dict that keeps the single products between calls on the same pieces."""
    total = None
    for wi, ai in terms:
        if cache is not None and (wi, ai) in cache:
            t = cache[(wi, ai)]
        else:
            t = op(a_pieces[ai].double(), w_pieces[wi].double())
            if cache is not None:
                cache[(wi, ai)] = t
        total = t if total is None else total + t
    return total


def rel_fro(y, ref):
    return float((y.double() - ref).norm() / ref.norm())


def split_error_model(op, a, w, post=None, lost=SMALL_TERMS, a_split=None, w_split=None):
    """(ref, E_model, E_loss) of one case: the fp64 result of the intact fp32 operands, the relative Frobenius error of the
    six-term sum against it, and the smallest such error among the five-term sums that leave out one of ``lost`` in turn.
    ``post``: a map applied to every restatement before the errors are taken (the stem's ReLU + max-pool).  ``a_split`` /
    ``w_split``: the split of each operand; the default is what the forward kernels do, activation = truncation, weight = nearest
    even (the weight gradient splits both of its operands by truncation)."""
    post = post or (lambda t: t)
    ap, wp, cache = (a_split or split3_trunc)(a), (w_split or split3_rne)(w), {}
    ref = post(op(a.double(), w.double()))
    e_model = rel_fro(post(term_sum(op, ap, wp, SIX_TERMS, cache)), ref)
    e_loss = min(rel_fro(post(term_sum(op, ap, wp, [t for t in SIX_TERMS if t != out], cache)), ref) for out in lost)
    return ref, e_model, e_loss


def paired_operands(family, a_shape, w_shape, gen, nonneg=False):
    """(a, w) fp32 CPU tensors of the given shapes, the LAST dimension of both being the kernels' innermost K index (the
    channel), whose leading products cancel in adjacent k pairs (2i, 2i + 1), so that the result is carried by the small pieces
    alone.  w ~ N(0, 1 / fan-in).
    "act": w[..., 2i+1] = -w[..., 2i]; a[..., 2i+1] has the leading bf16 piece (by truncation, as activations are split) of
    a[..., 2i] and fresh random lower 16 bits: what remains is w (r - r'), carried by a_mid / a_lo.
    "wgt": a[..., 2i+1] = -a[..., 2i]; w[..., 2i+1] has the leading bf16 piece (to nearest even, as weights are split) of
    w[..., 2i] and a fresh residual within half a bf16 step of it: what remains is a (r - r'), carried by w_mid / w_lo."""
    assert a_shape[-1] == w_shape[-1] and a_shape[-1] % 2 == 0
    fan_in = 1
    for d in w_shape[1:]:
        fan_in *= d
    a = torch.randn(*a_shape, generator=gen)
    w = torch.randn(*w_shape, generator=gen) / fan_in ** 0.5
    if family == "act":
        w[..., 1::2] = -w[..., 0::2]
        low = torch.randint(0, 1 << 16, a[..., 0::2].shape, generator=gen)
        a[..., 1::2] = _bits_f32((_f32_bits(a[..., 0::2]) & 0xffff0000) | low)
        if nonneg:
            a = a.abs()
        assert torch.equal(split3_trunc(a[..., 1::2].contiguous())[0], split3_trunc(a[..., 0::2].contiguous())[0])
    elif family == "wgt":
        if nonneg:
            a = a.abs()
        a[..., 1::2] = a[..., 0::2] if nonneg else -a[..., 0::2]
        hi = split3_rne(w[..., 0::2].contiguous())[0]
        low = torch.randint(-0x7fff, 0x8000, hi.shape, generator=gen)
        w[..., 1::2] = _bits_f32(_f32_bits(hi) + low)             # bit arithmetic: fp32 steps, also across a binade
        assert torch.equal(split3_rne(w[..., 1::2].contiguous())[0], hi)
        if nonneg:
            w[..., 1::2] = -w[..., 1::2]
    else:
        raise ValueError(family)
    return a, w


def paired_operands_trunc(family, a_shape, w_shape, gen):
    """``paired_operands`` for a product whose operands are BOTH split by truncation (the weight gradient g^T x: ``a`` = g,
    ``w`` = x, the last dimension of both the reduction index m).  "act": as above, a shares the leading piece within a pair
    and w changes sign.  "wgt": the same construction with the roles exchanged -- w[..., 2i+1] has the leading piece BY
    TRUNCATION of w[..., 2i] and a[..., 2i+1] = -a[..., 2i].  RESOLVED_TERMS holds for both as it stands."""
    if family == "act":
        return paired_operands("act", a_shape, w_shape, gen)
    if family != "wgt":
        raise ValueError(family)
    w, a = paired_operands("act", w_shape, a_shape, gen)
    return a, w


def add_on_load(a):
    """(x, pos) with fl32(x + pos) == a bit for bit: x = a_hi + a_mid (16 significant bits: exact in fp32), pos = a - x, which
    is exact and equals a_lo wherever three bf16 hold a (|a| >= 2^-110; below that pos also keeps the bits a_lo cannot), the
    pieces by truncation.  For the entries that add position rows to an operand while loading it."""
    hi, mid, lo = split3_trunc(a)
    x = hi + mid
    pos = a - x
    full = a.abs() >= 2.0 ** -110
    assert torch.equal(x.double(), hi.double() + mid.double()) and torch.equal(pos.double(), a.double() - x.double())
    assert torch.equal(_f32_bits(pos[full]), _f32_bits(lo[full])) and torch.equal(_f32_bits(x + pos), _f32_bits(a + 0.0))
    return x, pos


def xs_decode(buf, rows, K):
    """The three pieces [rows, K] (fp32 tensors holding bf16 values) of an XS operand stream ``buf`` (flat uint8), from the
    layout description of xs_format.h: fragment (row // 32, k // 16, piece p) at byte ((rb * (K / 16) + ks) * 3 + p) * 1024,
    element (row % 32, k % 16) inside it at byte (kk // 8) * 512 + r * 16 + (kk % 8) * 2, little-endian bf16."""
    assert buf.dtype == torch.uint8 and K % 16 == 0 and buf.numel() == ((rows + 31) // 32) * (K // 16) * 3 * 1024
    half = buf.cpu().contiguous().view(torch.int16).to(torch.int64) & 0xffff
    row, k = torch.arange(rows).view(-1, 1), torch.arange(K).view(1, -1)
    rb, r, ks, kk = row // 32, row % 32, k // 16, k % 16
    pieces = []
    for p in range(3):
        byte = ((rb * (K // 16) + ks) * 3 + p) * 1024 + (kk // 8) * 512 + r * 16 + (kk % 8) * 2
        pieces.append(_bits_f32(half[byte // 2] << 16))
    return tuple(pieces)


# ---- decoder self-attention inputs whose scores are EXACT fp32 numbers (csrc/self_attn.hip; tests/test_gpu_self_attention.py) --------
# q and k are multiples of 1/8 in [-1, 1]: every product is a multiple of 1/64 of magnitude <= 1 and every partial sum of a
# 32-term score (plus a shift of up to 128) stays below 2^8 in steps of 2^-6, i.e. inside 24 bits: the score is the same fp32
# number whatever the summation order, so is s - max, and every value is exact in bf16 as well.  Component 0 of every head is
# q = 1, k = 0: writing c into k's component 0 shifts every score of that key by exactly c.
ATTN_HEAD_DIM = 32
ATTN_TILE = 16          # keys per register tile of the forward kernel
ATTN_DOMINANT = 128.0   # a dominant key's score exceeds every other by >= 128 - 2 * 11 > 104: exp(-104) is 0 in fp32


def attn_grid_inputs(seed, B, N, M):
    """(q, k, v, grad_out) fp32 CPU tensors [B, N, M * 32]: q, k on the 1/8 grid in [-1, 1] with component 0 of every head
    q = 1, k = 0; v and the upstream gradient standard normal."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randint(-8, 9, (B, N, M * ATTN_HEAD_DIM), generator=g).float() / 8
    k = torch.randint(-8, 9, (B, N, M * ATTN_HEAD_DIM), generator=g).float() / 8
    q[..., 0::ATTN_HEAD_DIM] = 1.0
    k[..., 0::ATTN_HEAD_DIM] = 0.0
    v = torch.randn(B, N, M * ATTN_HEAD_DIM, generator=g)
    go = torch.randn(B, N, M * ATTN_HEAD_DIM, generator=g)
    return q, k, v, go


def attn_shift(k, M, c):
    """A copy of ``k`` with component 0 of every head set to ``c``: every score moves by exactly c (q's component 0 is 1)."""
    assert k.shape[-1] == M * ATTN_HEAD_DIM
    k = k.clone()
    k[..., 0::ATTN_HEAD_DIM] = c
    return k


def attn_dominant_keys(k, B, N, M, rot=0):
    """(k', keys): a copy of ``k`` in which, for each (b, h), ONE key has component 0 = 128, and the [B, M] table of those keys.
    The key of (b, h) lies in tile t = (b * M + h + rot) mod ntile, at min(16 t + (5 t mod 16), N - 1): with B * M >= ntile every
    tile is dominant for some (b, h); smaller batches reach the other tiles through ``rot``."""
    assert k.shape == (B, N, M * ATTN_HEAD_DIM)
    ntile = (N + ATTN_TILE - 1) // ATTN_TILE
    k = k.clone()
    keys = torch.empty(B, M, dtype=torch.long)
    for b in range(B):
        for h in range(M):
            t = (b * M + h + rot) % ntile
            keys[b, h] = min(ATTN_TILE * t + (5 * t) % ATTN_TILE, N - 1)
            k[b, keys[b, h], h * ATTN_HEAD_DIM] = ATTN_DOMINANT
    return k, keys


def attn_heads(t, M):
    B, N, MD = t.shape
    return t.view(B, N, M, MD // M).transpose(1, 2)


def attn_scores(q, k, M):
    """[B, M, N, N] scores q k^T per head in the operands' dtype."""
    return attn_heads(q, M) @ attn_heads(k, M).transpose(-1, -2)


def attn_compose(q, k, v, M, drop_tile=None, skip_max=False):
    """softmax(q k^T) v per head as a plain torch composition in the operands' dtype and on their device: the yardstick of the
    kernel tests (fp32) and their reference (fp64).  Two deliberately WRONG variants show that an assertion has teeth:
    ``drop_tile=t`` leaves keys 16 t .. 16 t + 15 out (a register-tile slot that never receives its keys), ``skip_max`` takes
    exp(s) without subtracting the row maximum."""
    B, N, MD = q.shape
    s = attn_scores(q, k, M)
    if drop_tile is not None:
        s = s.clone()
        s[..., drop_tile * ATTN_TILE:(drop_tile + 1) * ATTN_TILE] = float("-inf")
    if skip_max:
        e = torch.exp(s)
        w = e / e.sum(-1, keepdim=True)
    else:
        w = torch.softmax(s, -1)
    return (w @ attn_heads(v, M)).transpose(1, 2).reshape(B, N, MD)


def attn_dominant_mismatches(out, v, keys, M):
    """The (b, h, tile) triples at which ``out[b, :, h]`` is not bit for bit ``v[b, keys[b, h], h]`` in every query row."""
    B = out.shape[0]
    bits = torch.int32 if out.dtype == torch.float32 else torch.int16
    kd = keys.to(v.device)
    want = torch.stack([attn_heads(v, M)[b, torch.arange(M, device=v.device), kd[b]] for b in range(B)])   # [B, M, D]
    same = (attn_heads(out, M).contiguous().view(bits) == want[:, :, None, :].contiguous().view(bits)).all(-1).all(-1).cpu()
    return [(b, h, int(keys[b, h]) // ATTN_TILE) for b in range(B) for h in range(M) if not bool(same[b, h])]
