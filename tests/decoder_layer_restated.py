"""One decoder layer of the model (self-attention, deformable cross-attention, FFN, three LayerNorms, the next layer's scaled
q / k) written out from its definition with torch tensor ops on the CPU, in float64 (the reference) or float32 (the error
baseline), apart from the product's kernel (csrc/dec_layer.hip) and from the module's forward, so that the two check each other.
With it: seeded decoders whose every parameter matters (no zero bias, no constant column), the inputs of
``egtr_amd.decoder_fused.run`` for every path of the kernel, and ``DEFECTS`` -- deliberately wrong compositions that mimic what
the kernel could get wrong.  tests/test_decoder_layer_inputs_cpu.py shows that the inputs resolve every defect;
tests/test_gpu_decoder_layer.py compares the kernel.  Not a test module."""
import copy
import math

import numpy as np
import torch

import cpu_kernels
import weights as W

LEVELS = ((12, 16), (6, 8), (3, 4), (2, 2))                    # S = 256
LEVELS_34000 = ((160, 160), (80, 80), (40, 40), (20, 20))      # S = 34000: the padding mask is read from memory
LEVELS_32770 = ((156, 158), (78, 79), (39, 40), (20, 20))      # 1025 mask words: one past what the kernel keeps in LDS
LEVELS_32750 = ((156, 158), (78, 79), (39, 40), (19, 20))      # 1024 mask words: the last size held in LDS
HEADS, HEAD_DIM, POINTS = 8, 32, 4
OUTPUTS = ("states", "q", "k")                                 # what the GPU test compares, each [Ld, B, N, 256]
FACTOR = 4                                                     # the GPU test's bound: FACTOR x the float32 composition's error


def case(name, B, N, layers=2, levels=LEVELS, rows="per_image", ref="ratios", bias=True, mask=True, first_with_pos=False,
         score_scale=1.0, score_shift=0.0, logit_scale=1.0, seed=0):
    """rows: "expanded" (one image's rows, stride-0 over the batch, for states, positions and points), "per_image" (fresh
    rows for all three), "mixed" (states expanded, positions and points per image).  ref: "ratios" ([B, N, 2] points +
    valid ratios) or "premul" ([B, N, 4, 2], no ratios)."""
    return dict(name=name, B=B, N=N, layers=layers, levels=tuple(levels), rows=rows, ref=ref, bias=bias, mask=mask,
                first_with_pos=first_with_pos, score_scale=score_scale, score_shift=score_shift, logit_scale=logit_scale,
                seed=seed)


def _cases():
    out = []
    for n in (1, 7, 8, 9, 63, 64, 65, 256, 257, 320):             # row panels of 8, key tiles of 64, second tile per wave
        out.append(case(f"edges-B1-N{n}", 1, n, seed=n))
    for n in (1, 7, 8, 9, 63, 64, 65):
        out.append(case(f"edges-B2-N{n}", 2, n, seed=100 + n))
    for b, n in ((33, 1), (5, 57), (9, 33)):                       # > 32 clusters, every image ends in a partial panel
        out.append(case(f"loop-B{b}-N{n}", b, n, seed=200 + b))
    for rows in ("expanded", "per_image", "mixed"):
        for fwp in (False, True):
            out.append(case(f"rows-{rows}-{'with' if fwp else 'no'}-first-pos", 3, 20, rows=rows, first_with_pos=fwp, seed=300))
    for ref in ("ratios", "premul"):
        out.append(case(f"ref-{ref}", 2, 24, ref=ref, seed=400))
    for bias in (True, False):
        for mask in (True, False):
            out.append(case(f"value-{'bias' if bias else 'nobias'}-{'mask' if mask else 'nomask'}", 2, 24, bias=bias, mask=mask,
                            seed=500))
    out.append(case("mask-in-memory-S34000", 2, 16, levels=LEVELS_34000, seed=600))
    out.append(case("mask-in-memory-S32770", 2, 16, levels=LEVELS_32770, seed=601))
    out.append(case("mask-in-lds-S32750", 2, 16, levels=LEVELS_32750, seed=602))
    out.append(case("large-scores", 1, 300, score_scale=1.6, score_shift=56.0, logit_scale=12.0, seed=700))
    out.append(case("depth-6", 2, 40, layers=6, seed=800))
    return out


CASES = _cases()

# ------------------------------------------------------------------------------------------------------------------ model

_BASE = {}


def _base_decoder(num_layers):
    """The decoder of a model built the way tests/test_gpu_decoder_cluster.py::_model builds it (on the CPU), once per depth."""
    if num_layers not in _BASE:
        from egtr_amd.deformable_detr import DeformableDetrConfig
        from egtr_amd.egtr import DetrForSceneGraphGeneration
        cfg = DeformableDetrConfig(num_queries=8, encoder_layers=1, decoder_layers=num_layers, dropout=0.1,
                                   auxiliary_loss=False)
        for k, v in dict(num_labels=17, num_rel_labels=9, ce_loss_coefficient=2.0, rel_loss_coefficient=15.0,
                         connectivity_loss_coefficient=30.0, smoothing=1e-14, rel_sample_negatives=80,
                         rel_sample_nonmatching=80, rel_sample_negatives_largest=True, rel_sample_nonmatching_largest=True,
                         use_freq_bias=True, use_log_softmax=False, freq_bias_eps=1e-12, logit_adjustment=False,
                         logit_adj_tau=0.3).items():
            setattr(cfg, k, v)
        torch.manual_seed(0)
        _BASE[num_layers] = DetrForSceneGraphGeneration(cfg, fg_matrix=W.fg_matrix(17, 9)).eval().model.decoder
    return _BASE[num_layers]


def make_decoder(num_layers, seed, score_scale=1.0, score_shift=0.0, logit_scale=1.0, levels=LEVELS):
    """Every parameter of every layer from one PCG64 stream (names in sorted order) by the scale rules of
    tests/golden/weights.py::_scale_for: nothing is zero, nothing is constant along columns.  The LAST layer is reserved: its
    sampling-offset biases are all large and positive (half a level + 3 pixels + |r|), so that a row whose reference point
    is at 1.0 has all 128 samples outside every level there.  ``score_scale`` multiplies the q and k projection weights
    (scores grow with its square), ``score_shift`` is added to every score through channel 0 of each head's q and k biases,
    ``logit_scale`` multiplies the attention-logit weights."""
    dec = copy.deepcopy(_base_decoder(num_layers))
    rng = np.random.Generator(np.random.PCG64(seed))
    with torch.no_grad():
        for name, p in sorted(dec.named_parameters()):
            kind, s = W._scale_for(name, tuple(p.shape))
            r = torch.from_numpy(rng.standard_normal(tuple(p.shape)).astype(np.float32))
            p.copy_({"normal": s * r, "affine": 1 + s * r, "positive": 1 + s * r.abs()}[kind])
        for layer in dec.layers:
            sa = layer.self_attn
            sa.q_proj.weight.mul_(score_scale)
            sa.k_proj.weight.mul_(score_scale)
            if score_shift:
                t = math.sqrt(score_shift / sa.scaling)
                sa.q_proj.bias[::HEAD_DIM] += t
                sa.k_proj.bias[::HEAD_DIM] += t
            layer.encoder_attn.attention_weights.weight.mul_(logit_scale)
        so = dec.layers[-1].encoder_attn.sampling_offsets.bias      # [head, level, point, (x, y)]
        wh = torch.tensor([[w, h] for h, w in levels], dtype=torch.float32)
        so.copy_((0.5 * wh[None, :, None, :] + 3 + so.view(HEADS, 4, POINTS, 2).abs()).reshape(-1))
    return dec.eval()


def outside_rows(c):
    """(image, row) of the rows whose reference point is (1, 1): all their samples are outside in the last layer.  One per
    image; with a single query only image 0 has one (the other images keep a point of their own)."""
    if c["N"] == 1:
        return [(0, 0)]
    if c["rows"] == "expanded":
        return [(b, 2 % c["N"]) for b in range(c["B"])]
    return [(b, (5 * b + 2) % c["N"]) for b in range(c["B"])]


def make_inputs(c):
    """The arguments of ``decoder_fused.run`` after the decoder, as CPU tensors (``to_device`` moves them)."""
    B, N, Ld, levels = c["B"], c["N"], c["layers"], c["levels"]
    rng = np.random.Generator(np.random.PCG64(10_000 + c["seed"]))

    def normal(*shape):
        return torch.from_numpy(rng.standard_normal(shape, dtype=np.float32))

    def rows_of(per_image, width, draw):
        return draw(B, N, width) if per_image else draw(N, width).unsqueeze(0).expand(B, N, width)

    per_x = c["rows"] == "per_image"
    per_pos = c["rows"] in ("per_image", "mixed")
    hidden = rows_of(per_x, 256, normal)
    pos = rows_of(per_pos, 256, normal)
    pts = rows_of(per_pos, 2, lambda *s: torch.from_numpy(rng.random(s, dtype=np.float32))).clone()   # [B, N, 2] in [0, 1)
    for b in range(B if per_pos else 1):
        for i in range(5, N, 8):                                   # one row in eight: a coordinate exactly on the border
            pts[b, i, (i // 8) % 2] = float((i // 16) % 2)
    if N == 1:                                                     # a single query: the odd images' points sit on the right
        pts[1::2, 0, 0] = 1.0                                      # edge of what is valid, their samples straddle the padding
    for b, i in outside_rows(c):
        pts[b, i] = 1.0
    if not per_pos:
        pts = pts[:1].expand(B, N, 2)
    # image 0 is whole; the images after it are padded at the bottom and on the right of every level
    S = sum(h * w for h, w in levels)
    keep = torch.ones(B, S, dtype=torch.bool)
    ratios = torch.ones(B, 4, 2)
    starts = [0]
    for h, w in levels:
        starts.append(starts[-1] + h * w)
    for b in range(1, B):
        fy, fx = 0.55 + 0.45 * rng.random(), 0.55 + 0.45 * rng.random()
        for l, (h, w) in enumerate(levels):
            vh, vw = math.ceil(fy * h), math.ceil(fx * w)
            m = torch.zeros(h, w, dtype=torch.bool)
            m[:vh, :vw] = True
            keep[b, starts[l]:starts[l + 1]] = m.reshape(-1)
            ratios[b, l, 0], ratios[b, l, 1] = vw / w, vh / h
    if c["ref"] == "ratios":
        reference, valid_ratios = pts, ratios
    else:
        reference, valid_ratios = (pts[:, :, None, :] * ratios[:, None]).contiguous(), None
    first = None
    if c["first_with_pos"]:
        first = hidden + pos if (per_x or per_pos) else (hidden[0] + pos[0]).unsqueeze(0).expand(B, N, 256)
    return dict(hidden_states=hidden, position_embeddings=pos, reference_input=reference, values=normal(Ld, B, S, 256),
                value_bias=0.5 * normal(Ld, 256) if c["bias"] else None, keep_mask=keep if c["mask"] else None,
                spatial_shapes=torch.tensor(levels, dtype=torch.int64),
                level_start_index=torch.tensor(starts[:-1], dtype=torch.int64), first_with_pos=first,
                valid_ratios=valid_ratios)


def build(c):
    return (make_decoder(c["layers"], c["seed"], c["score_scale"], c["score_shift"], c["logit_scale"], c["levels"]),
            make_inputs(c))


def to_device(inputs, dev):
    """Stride-0 batch expansions stay expansions (of the moved rows)."""
    out = {}
    for k, t in inputs.items():
        if k.startswith("_"):
            continue
        if torch.is_tensor(t) and t.dim() == 3 and t.shape[0] > 1 and t.stride(0) == 0:
            out[k] = t[0].contiguous().to(dev).unsqueeze(0).expand(*t.shape)
        else:
            out[k] = t.to(dev) if torch.is_tensor(t) else t
    return out


# -------------------------------------------------------------------------------------------------------------- reference

def _layer_norm(v, ln, dtype):
    mean = v.mean(-1, keepdim=True)
    var = ((v - mean) ** 2).mean(-1, keepdim=True)
    return (v - mean) / torch.sqrt(var + ln.eps) * ln.weight.to(dtype) + ln.bias.to(dtype)


def _linear(v, lin, dtype, skip_k=None):
    w = lin.weight.to(dtype)
    if skip_k is not None:                                          # a K-slice of the product left out
        w = w.clone()
        w[:, skip_k] = 0
    return v @ w.t() + lin.bias.to(dtype)


def _heads(t):
    B, N, _ = t.shape
    return t.view(B, N, HEADS, HEAD_DIM).transpose(1, 2)


def _compose(decoder, inp, dtype, edit=None):
    """The layer stack; ``edit`` names one deliberate mistake (see DEFECTS) or is None."""
    x = inp["hidden_states"].to(dtype)
    pos = inp["position_embeddings"].to(dtype)
    B, N, _ = x.shape
    shapes, lsi = inp["spatial_shapes"], inp["level_start_index"]
    ref = inp["reference_input"].to(dtype)
    keep = inp["keep_mask"]
    if edit == "image 1 reads image 0's position rows":
        pos = torch.cat([pos[:1], pos[:1], pos[2:]])
    if edit == "image 1 reads image 0's reference rows":
        ref = torch.cat([ref[:1], ref[:1], ref[2:]])
    if edit == "image 1 reads image 0's padding mask":
        keep = torch.cat([keep[:1], keep[:1], keep[2:]])
    if edit == "padding mask ignored":
        keep = None
    if inp["valid_ratios"] is not None:
        ref = ref[:, :, None, :] * inp["valid_ratios"].to(dtype)[:, None]       # [B, N, 4, 2]
    wh = torch.stack([shapes[:, 1], shapes[:, 0]], -1).to(dtype)                 # (W_l, H_l)
    states, qs, ks, crosses = [], [], [], []
    for li, layer in enumerate(decoder.layers):
        sa, ca = layer.self_attn, layer.encoder_attn
        # ---- self-attention
        xp = x + pos
        q = _linear(xp, sa.q_proj, dtype)
        if not (edit == "q of the next layer unscaled" and li > 0):
            q = q * sa.scaling
        k = _linear(xp, sa.k_proj, dtype)
        v = _linear(xp if (edit == "v of the next layer from x + pos" and li > 0) else x, sa.v_proj, dtype)
        qs.append(q)
        ks.append(k)
        s = _heads(q) @ _heads(k).transpose(-1, -2)                              # [B, 8, N, N]
        if edit == "last key left out of the softmax":
            s[..., N - 1] = -math.inf
        if edit == "keys >= 256 left out":
            s[..., 256:] = -math.inf
        s = s - s.max(-1, keepdim=True).values
        p = torch.exp(s)
        p = p / p.sum(-1, keepdim=True)
        o = (p @ _heads(v)).transpose(1, 2).reshape(B, N, 256)
        y = _linear(o, sa.out_proj, dtype, slice(160, 192) if edit == "head 5 left out of out_proj" else None)
        x1 = _layer_norm(x + y, layer.self_attn_layer_norm, dtype)
        # ---- deformable cross-attention
        z = x1 + pos
        off = _linear(z, ca.sampling_offsets, dtype).view(B, N, HEADS, 4, POINTS, 2)
        if edit == "x and y offsets of one sample swapped":
            off = off.clone()
            off[:, :, 3, 0, 1] = off[:, :, 3, 0, 1].flip(-1)
        lg = _linear(z, ca.attention_weights, dtype).view(B, N, HEADS, 16)
        lg = lg - lg.max(-1, keepdim=True).values
        a = torch.exp(lg)
        a = (a / a.sum(-1, keepdim=True)).view(B, N, HEADS, 4, POINTS)
        loc = ref[:, :, None, :, None, :] + off / wh[None, None, None, :, None, :]
        if edit == "sampling points of two levels swapped":
            loc = loc[:, :, :, [0, 2, 1, 3]]
        vb = inp["value_bias"][li].to(dtype) if inp["value_bias"] is not None else None
        plain = keep is inp["keep_mask"] and edit != "value bias added unweighted"
        val = inp.setdefault("_values", {}).get((li, dtype)) if plain else None   # (the unedited values are prepared once)
        if val is None:
            val = inp["values"][li].to(dtype)
            if vb is not None and edit != "value bias added unweighted":
                val = val + vb
            if keep is not None:
                val = val * keep[..., None].to(dtype)
            if plain:
                inp["_values"][(li, dtype)] = val
        cross = cpu_kernels.OracleMSDA.ms_deform_attn_forward(val.view(B, -1, HEADS, HEAD_DIM), shapes, lsi, loc.contiguous(),
                                                              a.contiguous(), 64)
        if edit == "value bias added unweighted":
            cross = cross + vb
        crosses.append(cross)
        y = _linear(cross, ca.output_proj, dtype, slice(64, 96) if edit == "head 2 left out of output_proj" else None)
        x2 = _layer_norm(x1 + y, layer.encoder_attn_layer_norm, dtype)
        # ---- feed-forward
        hid = torch.relu(_linear(x2, layer.fc1, dtype, slice(188, 192) if edit == "a k group left out of fc1's second half"
                                 else None))
        y = _linear(hid, layer.fc2, dtype, slice(644, 648) if edit == "a k group left out of fc2" else None)
        x = _layer_norm(x2 + y, layer.final_layer_norm, dtype)
        states.append(x)
    return dict(states=torch.stack(states), q=torch.stack(qs), k=torch.stack(ks), cross_out=torch.stack(crosses))


def layer_f64(decoder, inputs, dtype=torch.float64):
    """states [Ld, B, N, 256], the scaled q and the k of every layer [Ld, B, N, 256], and ``cross_out`` [Ld, B, N, 256]: each
    layer's cross-attention output before ``output_proj``.  ``dtype=torch.float32``: the same composition as the error
    baseline."""
    with torch.no_grad():
        return _compose(decoder, inputs, dtype)


def errors(got, ref):
    """{(output, layer): max |got - ref|} over all elements."""
    return {(o, l): float((got[o][l].double() - ref[o][l]).abs().max()) for o in OUTPUTS for l in range(ref[o].shape[0])}


# ---------------------------------------------------------------------------------------------------------------- defects

def _dropped(attr):
    def run(decoder, inputs):
        dec = copy.deepcopy(decoder)
        with torch.no_grad():
            for li, layer in enumerate(dec.layers):
                if attr == "b_qkv_next":                            # the biases the kernel applies: layers after the first
                    if li > 0:
                        for lin in (layer.self_attn.q_proj, layer.self_attn.k_proj, layer.self_attn.v_proj):
                            lin.bias.zero_()
                else:
                    {"b_attn_out": layer.self_attn.out_proj, "b_cross_out": layer.encoder_attn.output_proj,
                     "b_fc1": layer.fc1, "b_fc2": layer.fc2}[attr].bias.zero_()
        return layer_f64(dec, inputs)
    return run


def _edited(name):
    def run(decoder, inputs):
        with torch.no_grad():
            return _compose(decoder, inputs, torch.float64, name)
    return run


def _always(c):
    return True


def _two_images(c):
    return c["B"] >= 2


# (name, (decoder, inputs) -> altered float64 result, case -> whether the defect can show at that case)
DEFECTS = [(f"{b} dropped", _dropped(b), _always) for b in ("b_attn_out", "b_cross_out", "b_fc1", "b_fc2")] + [
    ("b_qkv_next dropped", _dropped("b_qkv_next"), lambda c: c["layers"] >= 2)] + [
    (n, _edited(n), ok) for n, ok in (
        ("value bias added unweighted", lambda c: c["bias"]),
        ("head 5 left out of out_proj", _always),
        ("head 2 left out of output_proj", _always),
        ("a k group left out of fc2", _always),
        ("a k group left out of fc1's second half", _always),
        ("last key left out of the softmax", lambda c: c["N"] >= 2),
        ("keys >= 256 left out", lambda c: c["N"] > 256),
        ("x and y offsets of one sample swapped", _always),
        ("sampling points of two levels swapped", _always),
        ("padding mask ignored", lambda c: c["mask"] and c["B"] >= 2),
        ("image 1 reads image 0's position rows", lambda c: c["B"] >= 2 and c["rows"] != "expanded"),
        ("image 1 reads image 0's reference rows", lambda c: c["B"] >= 2 and c["rows"] != "expanded"),
        ("image 1 reads image 0's padding mask", lambda c: c["mask"] and c["B"] >= 2),
        ("q of the next layer unscaled", lambda c: c["layers"] >= 2),
        ("v of the next layer from x + pos", lambda c: c["layers"] >= 2))]
