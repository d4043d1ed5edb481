"""One decoder layer in TRAINING (self-attention with the retained scaled-q / k maps, deformable cross-attention on a value
projection that is handed in, FFN, three dropout + residual + LayerNorm steps) written out with torch tensor ops under autograd
on the CPU, in float64 (the reference) or float32 (the error yardstick), apart from the product's autograd node
(egtr_amd.ops.DecoderLayerTrainFunction) and from its kernels, as the node's docstring states the layer:

    q = s (x + pos) Wq^T + s bq,  k = (x + pos) Wk^T + bk,  v = x Wv^T + bv;   a = out_proj(softmax(q k^T) v)
    y1 = LN1(x + drop(a));   [off | logits] of (y1 + pos);   c = output_proj(MSDA(value, loc, softmax(logits)))
    y2 = LN2(y1 + drop(c));  y3 = LN3(y2 + drop(fc2(relu(fc1(y2)))))            returns (y3, q, k)

MSDA is ``oracle.msda.msda_forward_grid_sample`` (F.grid_sample), differentiated by autograd.  Nothing here calls a HIP kernel
or ``egtr_amd.ops``; the layer class is used for its parameters only.

The GPU test (tests/test_gpu_decoder_train_node.py) compares EVERY element of every output and gradient, so the inputs keep
away from the two kinks of the layer, where float32 and float64 may take different branches and a gradient differs at O(1): a
ReLU input near zero and a sample coordinate near a pixel boundary.  ``build`` picks, per case, the first seed at or after the
case's base seed whose float64 reference keeps every fc1 pre-activation at least DELTA_RELU from zero and every sample's pixel
coordinate at least DELTA_PX from an integer, and whose float32 composition has the same ReLU mask and the same bilinear cells;
the margins are 16 x the largest float32 deviation of those quantities, which tests/test_decoder_train_cases_cpu.py measures.
``DEFECTS``: deliberately wrong gradient wirings; the same CPU test shows that the cases resolve each.  Not a test module."""
import functools

import torch
import torch.nn.functional as F

from decoder_layer_restated import HEAD_DIM, HEADS, LEVELS, POINTS
from oracle import msda as OM

FACTOR = 4                      # the GPU test's bound: max(plain, FACTOR x the float32 composition's error), per tensor
MARGIN_FACTOR = 16              # margins = MARGIN_FACTOR x the largest float32 deviation over the cases
DELTA_RELU = 4e-5               # >= 16 x the measured deviation of an fc1 pre-activation (the CPU test asserts it)
DELTA_PX = 4e-5                 # >= 16 x the measured deviation of a pixel coordinate
MAX_SEEDS = 200
S = sum(h * w for h, w in LEVELS)
STATE_GRADS = ("grad_x", "grad_pos", "grad_ref", "grad_value")
FORWARD = ("y3", "q", "k")


def case(B, N, ffn, p, pos, base_seed):
    return dict(name=f"B{B}-N{N}-ffn{ffn}-p{p:g}-pos-{pos}", B=B, N=N, ffn=ffn, p=p, pos=pos, base_seed=base_seed)


# pos "expanded": one [N, 256] table, stride 0 over the batch (the model's query positions: the gradient is summed over the
# batch); "per_image": [B, N, 256] rows of their own
CASES = [
    case(2, 17, 64, 0.1, "expanded", 1000), case(2, 17, 64, 0.0, "per_image", 1200),
    case(1, 9, 1024, 0.1, "expanded", 2000), case(1, 9, 1024, 0.0, "per_image", 2200),
    case(3, 11, 128, 0.1, "expanded", 3000), case(3, 11, 128, 0.0, "expanded", 3200),
    case(3, 11, 128, 0.1, "per_image", 3400), case(3, 11, 128, 0.0, "per_image", 3600),
    case(1, 33, 64, 0.1, "per_image", 4000), case(1, 33, 64, 0.0, "expanded", 4200),
]


# ------------------------------------------------------------------------------------------------------------ layer and inputs
def make_layer(ffn, p, seed):
    """Built the way tests/test_gpu_train_fused.py::_decoder_layer builds it (perturbed offset / logit weights, LayerNorm
    weights in [0.5, 1.5]), on the CPU, in train mode."""
    from egtr_amd.deformable_detr import DeformableDetrConfig, DeformableDetrDecoderLayer
    torch.manual_seed(seed)
    layer = DeformableDetrDecoderLayer(DeformableDetrConfig(dropout=p, decoder_ffn_dim=ffn))
    with torch.no_grad():
        layer.encoder_attn.sampling_offsets.weight.normal_(0, 0.02)
        layer.encoder_attn.attention_weights.weight.normal_(0, 0.05)
        layer.encoder_attn.attention_weights.bias.normal_(0, 0.1)
        for ln in (layer.self_attn_layer_norm, layer.encoder_attn_layer_norm, layer.final_layer_norm):
            ln.weight.uniform_(0.5, 1.5)
            ln.bias.normal_(0, 0.1)
    return layer.train()


def make_inputs(c, seed):
    B, N, p = c["B"], c["N"], c["p"]
    g = torch.Generator().manual_seed(50_000 + seed)
    x = torch.randn(B, N, 256, generator=g)
    pos = torch.randn(N, 256, generator=g) * 0.5 if c["pos"] == "expanded" else torch.randn(B, N, 256, generator=g) * 0.5
    ref = torch.rand(B, N, 1, 2, generator=g)
    ratios = 0.7 + 0.3 * torch.rand(B, 1, 4, 2, generator=g)
    value = torch.randn(B, S, 256, generator=g)
    gy, gq, gk = (torch.randn(B, N, 256, generator=g) for _ in range(3))
    masks = (torch.rand(3, B * N, 256, generator=g) < 1.0 - p).to(torch.uint8) if p > 0 else None
    shapes = torch.tensor(LEVELS, dtype=torch.int64)
    lsi = torch.cat((shapes.new_zeros((1,)), shapes.prod(1).cumsum(0)[:-1]))
    return dict(x=x, pos=pos, ref=ref, ratios=ratios, value=value, gy=gy, gq=gq, gk=gk, masks=masks, shapes=shapes, lsi=lsi)


# -------------------------------------------------------------------------------------------------------------------- the layer
def _heads(t):
    B, N, _ = t.shape
    return t.view(B, N, HEADS, HEAD_DIM).transpose(1, 2)


def _value_only(shown, kept_gradient):
    """The value of ``shown`` with the gradient of ``kept_gradient`` (a backward that differs from its forward)."""
    return kept_gradient + (shown - kept_gradient).detach()


def compose(layer, inp, dtype, edit=None):
    """Forward and backward of the layer in ``dtype``: {"y3", "q", "k", "grad_x", "grad_pos", "grad_ref", "grad_value",
    "<parameter name>": its gradient (None for the layer's own value_proj), "pre": fc1's pre-activations, "px": the pixel
    coordinates of every sample [..., 2]}.  ``edit`` names one deliberate mistake of the BACKWARD (see DEFECTS); the forward
    values are the right ones under every edit."""
    def leaf(t):
        return t.detach().to(dtype).clone().requires_grad_(True)

    P = {n: leaf(q) for n, q in layer.named_parameters()}
    x = leaf(inp["x"])
    B, N, D = x.shape
    table = leaf(inp["pos"])
    pos = (table.unsqueeze(0).expand(B, N, D) if table.dim() == 2 else table) + 0       # [B, N, D], not a leaf
    pos.retain_grad()
    ref = leaf(inp["ref"])
    ref_in = ref * inp["ratios"].to(dtype)                                                # [B, N, 4, 2]
    ref_in.retain_grad()
    value = leaf(inp["value"])
    p = float(layer.dropout)
    scale = 1.0 / (1.0 - p) if p > 0 else 1.0
    masks = inp["masks"]
    s = float(layer.self_attn.scaling)

    def lin(v, name):
        return v @ P[name + ".weight"].t() + P[name + ".bias"]

    def drop(v, i):
        if masks is None:
            return v
        kept = v * masks[i].view(B, N, D).to(dtype) * scale
        if edit == f"dropout mask {i + 1} missing in the backward":
            return _value_only(kept, v * scale)
        return kept

    def norm(v, name, eps):
        return F.layer_norm(v, (D,), P[name + ".weight"], P[name + ".bias"], eps)

    def residual(v, i):
        return v.detach() if edit == f"residual gradient at LN{i} dropped" else v

    # ---- self-attention
    xp = x + pos
    q_lin = xp @ P["self_attn.q_proj.weight"].t()
    bq = P["self_attn.q_proj.bias"]
    if edit == "scaling missing from q's backward":
        q = _value_only((q_lin + bq) * s, q_lin + bq)
    elif edit == "scaling applied to q's bias gradient twice":
        q = q_lin * s + _value_only(bq * s, bq * s * s)
    else:
        q = (q_lin + bq) * s
    k = lin(xp, "self_attn.k_proj")
    v = lin(x, "self_attn.v_proj")
    att = torch.softmax(_heads(q) @ _heads(k).transpose(-1, -2), -1)
    a = lin((att @ _heads(v)).transpose(1, 2).reshape(B, N, D), "self_attn.out_proj")
    y1 = norm(residual(x, 1) + drop(a, 0), "self_attn_layer_norm", layer.self_attn_layer_norm.eps)
    # ---- deformable cross-attention on the value projection that is handed in
    z = y1 + (pos.detach() if edit == "position gradient missing the y1 + pos branch" else pos)
    off = lin(z, "encoder_attn.sampling_offsets").view(B, N, HEADS, 4, POINTS, 2)
    aw = torch.softmax(lin(z, "encoder_attn.attention_weights").view(B, N, HEADS, 4 * POINTS), -1).view(B, N, HEADS, 4, POINTS)
    shapes = inp["shapes"]
    wh = torch.stack([shapes[:, 1], shapes[:, 0]], -1).to(dtype)                          # (W_l, H_l)
    loc = ref_in[:, :, None, :, None, :] + off / wh[None, None, None, :, None, :]
    px = loc * wh[None, None, None, :, None, :] - 0.5                                     # pixel coordinates x W - 0.5, y H - 0.5
    cross = OM.msda_forward_grid_sample(value.view(B, S, HEADS, HEAD_DIM), shapes, loc, aw)
    c = lin(cross.view(B, N, D), "encoder_attn.output_proj")
    y2 = norm(residual(y1, 2) + drop(c, 1), "encoder_attn_layer_norm", layer.encoder_attn_layer_norm.eps)
    # ---- feed-forward block
    pre = lin(y2, "fc1")
    f = lin(torch.relu(pre), "fc2")
    y3 = norm(residual(y2, 3) + drop(f, 2), "final_layer_norm", layer.final_layer_norm.eps)
    gy, gq, gk = (inp[n].to(dtype) for n in ("gy", "gq", "gk"))
    if edit == "q-map upstream gradient dropped":
        gq = torch.zeros_like(gq)
    if edit == "k-map upstream gradient dropped":
        gk = torch.zeros_like(gk)
    torch.autograd.backward([y3, q, k], [gy, gq, gk])
    out = dict(y3=y3.detach(), q=q.detach(), k=k.detach(), grad_x=x.grad, grad_pos=table.grad, grad_ref=ref.grad,
               grad_value=value.grad, pre=pre.detach(), px=px.detach())
    for n in P:
        out[n] = P[n].grad
    if edit == "position gradient not summed over the batch":
        out["grad_pos"] = pos.grad[0]
    if edit == "reference-point gradient not summed over the levels":
        out["grad_ref"] = (ref_in.grad * inp["ratios"].to(dtype))[:, :, :1]
    if edit == "value gradient not summed over the heads":
        gv = value.grad.clone()
        gv[..., HEAD_DIM:] = 0                                                            # only head 0's samples arrive
        out["grad_value"] = gv
    for i, (ln, lin_name) in enumerate((("self_attn_layer_norm", "self_attn.out_proj"),
                                        ("encoder_attn_layer_norm", "encoder_attn.output_proj"), ("final_layer_norm", "fc2"))):
        if edit == f"d beta and d bias of LN{i + 1} swapped":
            out[ln + ".bias"], out[lin_name + ".bias"] = out[lin_name + ".bias"], out[ln + ".bias"]
    return out


def compared(out):
    """The names the GPU test compares: forward, state gradients, the 24 parameters with a gradient."""
    return list(FORWARD) + list(STATE_GRADS) + sorted(n for n, t in out.items() if "." in n and t is not None)


# ------------------------------------------------------------------------------------------------------------------ seed search
def kink_distances(r64):
    """(min |fc1 pre-activation|, min distance of a pixel coordinate from an integer) of a float64 result."""
    px = r64["px"]
    return float(r64["pre"].abs().min()), float((px - px.round()).abs().min())


def deviations(r32, r64):
    """max |float32 - float64| of the fc1 pre-activations and of the pixel coordinates."""
    return float((r32["pre"].double() - r64["pre"]).abs().max()), float((r32["px"].double() - r64["px"]).abs().max())


def same_branches(r32, r64):
    return (torch.equal(r32["pre"] > 0, r64["pre"] > 0)
            and torch.equal(torch.floor(r32["px"]).double(), torch.floor(r64["px"])))


@functools.lru_cache(maxsize=None)
def build(name):
    """(seed, layer, inputs, float64 result, float32 result) of the case: the first seed at or after its base seed that meets
    the conditions of the module docstring.  Computed once; nothing in it is written to afterwards."""
    c = next(c for c in CASES if c["name"] == name)
    for seed in range(c["base_seed"], c["base_seed"] + MAX_SEEDS):
        layer, inp = make_layer(c["ffn"], c["p"], seed), make_inputs(c, seed)
        r64 = compose(layer, inp, torch.float64)
        d_relu, d_px = kink_distances(r64)
        if d_relu < DELTA_RELU or d_px < DELTA_PX:
            continue
        r32 = compose(layer, inp, torch.float32)
        if same_branches(r32, r64):
            return seed, layer, inp, r64, r32
    raise AssertionError(f"{name}: no seed in [{c['base_seed']}, {c['base_seed'] + MAX_SEEDS}) keeps away from the kinks")


def errors(got, ref, names):
    """{name: max |got - ref|} over all elements."""
    return {n: float((got[n].double() - ref[n]).abs().max()) for n in names}


# ------------------------------------------------------------------------------------------------------------------ defects
def _always(c):
    return True


def _dropout(c):
    return c["p"] > 0


# (name, case -> whether the defect can show at that case)
DEFECTS = [
    ("position gradient missing the y1 + pos branch", _always),
    ("position gradient not summed over the batch", lambda c: c["pos"] == "expanded" and c["B"] >= 2),
    ("residual gradient at LN1 dropped", _always),
    ("residual gradient at LN2 dropped", _always),
    ("residual gradient at LN3 dropped", _always),
    ("q-map upstream gradient dropped", _always),
    ("k-map upstream gradient dropped", _always),
    ("scaling missing from q's backward", _always),
    ("scaling applied to q's bias gradient twice", _always),
    ("dropout mask 1 missing in the backward", _dropout),
    ("dropout mask 2 missing in the backward", _dropout),
    ("dropout mask 3 missing in the backward", _dropout),
    ("d beta and d bias of LN1 swapped", _always),
    ("d beta and d bias of LN2 swapped", _always),
    ("d beta and d bias of LN3 swapped", _always),
    ("reference-point gradient not summed over the levels", _always),
    ("value gradient not summed over the heads", _always),
]
