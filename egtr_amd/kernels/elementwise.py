"""Bindings of the row-wise and geometry kernels (csrc/elementwise.hip, enc_train.hip and their kin):
LayerNorm and dropout + LayerNorm launches, position embeddings, the GroupNorm projections, box
decoding, row scaling and masking.  No routing decisions here -- ``egtr_amd.ops`` decides and re-exports every name
below."""
import torch

from .. import _lib
from .._lib import _chk
from .derived import cached_weights

__all__ = ["dropout_add_layernorm", "dropout_add_layernorm_backward", "add_layer_norm_into", "box_decode", "bias_mask_rows_",
           "add_layer_norm_pos", "scale_rows_multi", "sine_position_embedding", "input_proj_groupnorm_flatten",
           "input_proj_groupnorm_tokens", "input_proj_groupnorm_token_slabs", "level_geometry"]


def dropout_add_layernorm(x, residual, keep, scale, weight, bias, eps, flag=None):
    """LayerNorm(residual + keep * scale * x) over rows of 256 channels in one pass (egtr_dropout_add_layernorm_f32); ``keep``
    uint8 [rows, 256] or None; ``flag`` (int32 [1], optional) is OR-ed with 1 when an output element is non-finite."""
    rows = x.shape[0]
    y = torch.empty_like(x)
    _lib.launch("egtr_dropout_add_layernorm_f32", x.data_ptr(), residual.data_ptr(), _lib.ptr(keep), float(scale),
                weight.data_ptr(), bias.data_ptr(), y.data_ptr(), rows, 256, float(eps), _lib.ptr(flag))
    return y


def dropout_add_layernorm_backward(x, residual, keep, scale, weight, eps, grad_y, flag=None, y_out=None, clamp_value=0.0):
    """Backward of ``dropout_add_layernorm``: (grad_sum, grad_x (is grad_sum without dropout), [d gamma | d beta | d bias])."""
    lib = _lib.lib()
    rows = x.shape[0]
    gs = torch.empty_like(x)
    gx = torch.empty_like(x) if keep is not None else None
    ws = torch.empty(int(lib.egtr_dropout_add_layernorm_backward_workspace_floats(rows)), dtype=torch.float32, device=x.device)
    out = torch.empty(768, dtype=torch.float32, device=x.device)
    _lib.launch("egtr_dropout_add_layernorm_backward_f32", x.data_ptr(), residual.data_ptr(), _lib.ptr(keep), float(scale),
                weight.data_ptr(), grad_y.data_ptr(), _lib.ptr(flag),
                y_out.data_ptr() if (flag is not None and y_out is not None) else None, float(clamp_value), gs.data_ptr(),
                _lib.ptr(gx), ws.data_ptr(), out.data_ptr(), rows, 256, float(eps))
    return gs, (gx if gx is not None else gs), out


def add_layer_norm_into(x, residual, ln, out):
    """out = LayerNorm(x + residual) through the stand-alone kernel (egtr_add_layernorm_f32; inference, 256 channels)."""
    x2 = _chk(x.contiguous(), "x", torch.float32)
    r2 = _chk(residual.contiguous(), "residual", torch.float32)
    _chk(out, "out", torch.float32)
    if out.shape != x2.shape or x2.shape[-1] != 256:
        raise ValueError("add_layer_norm_into: out must have the shape of x, 256 channels")
    _lib.launch("egtr_add_layernorm_f32", x2.data_ptr(), r2.data_ptr(), ln.weight.data_ptr(), ln.bias.data_ptr(),
                out.data_ptr(), x2.numel() // 256, 256, float(ln.eps))
    return out


def box_decode(delta, init_reference, inter_references, eps=1e-5, logits_all=None):
    """sigmoid(delta + [inverse_sigmoid(reference_l), 0..]) for all decoder levels in one HIP launch (egr:286-305;
    reference_0 = init_reference, reference_l = inter_references[:, l-1]).  ``inter_references`` expanded from ONE tensor
    (stride 0 over the level axis: no box refinement) is not materialised.  With ``logits_all`` [B, Ld, N, C] the launch
    also returns argmax(logits_all[:, -1], -1) (the relation head's class lookup, egtr:405-413): (boxes, node_cls).
    Inference only."""
    B, Ld, N, four = delta.shape
    if four != 4:
        raise ValueError(f"delta must be [B, Ld, N, 4], got {tuple(delta.shape)}")
    d = _chk(delta.contiguous(), "delta", torch.float32)
    r0 = _chk(init_reference.contiguous(), "init_reference", torch.float32)
    RD = r0.shape[-1]
    # every level = the initial reference points, expanded over the level axis (the decoder without box refinement)
    same = (inter_references.dim() == 4 and Ld > 1 and inter_references.stride(1) == 0
            and inter_references.data_ptr() == init_reference.data_ptr()
            and inter_references.stride(0) == init_reference.stride(0)
            and tuple(inter_references.stride()[2:]) == tuple(init_reference.stride()[1:]))
    r1 = None if same else _chk(inter_references.contiguous(), "inter_references", torch.float32)
    if tuple(r0.shape) != (B, N, RD) or tuple(inter_references.shape) != (B, Ld, N, RD):
        raise ValueError(f"reference shapes {tuple(r0.shape)} / {tuple(inter_references.shape)} do not match delta "
                         f"{tuple(delta.shape)}")
    if RD not in (2, 4):
        raise ValueError(f"reference.shape[-1] should be 4 or 2, but got {RD}")
    out = torch.empty_like(d)
    lg, node, C = None, None, 0
    if logits_all is not None:
        lg = _chk(logits_all.contiguous(), "logits_all", torch.float32)
        C = lg.shape[-1]
        if tuple(lg.shape[:3]) != (B, Ld, N):
            raise ValueError("logits_all must be [B, Ld, N, C]")
        node = torch.empty(B, N, dtype=torch.int64, device=d.device)
    _lib.launch("egtr_box_decode_argmax_f32", d.data_ptr(), r0.data_ptr(), _lib.ptr(r1), B, Ld, N, RD, float(eps),
                out.data_ptr(), _lib.ptr(lg), C, _lib.ptr(node))
    return out if logits_all is None else (out, node)


def bias_mask_rows_(y, bias, keep):
    """In place: y[g, r, :] = keep[r] ? y[g, r, :] + bias[g, :] : 0  (y [G, R, C]; keep [R] bool or None)."""
    G, R, C = y.shape
    _chk(y, "y", torch.float32)
    b2 = _chk(bias.detach().contiguous(), "bias", torch.float32)
    k2 = None
    if keep is not None:
        k2 = keep.reshape(-1).contiguous()
        k2 = k2.view(torch.uint8) if k2.dtype == torch.bool else k2.to(torch.uint8)
        _chk(k2, "keep")
    _lib.launch("egtr_bias_mask_rows_f32", y.data_ptr(), b2.data_ptr(), _lib.ptr(k2), G, R, C)
    return y


def add_layer_norm_pos(x, residual, ln, pos, out=None):
    """(ln(residual + x), ln(residual + x) + pos) in one HIP launch; pos is [rows_p, 256] with rows % rows_p == 0
    (broadcast over the batch).  ``out``: optional contiguous destination of the first result (e.g. a slice of the
    decoder's stacked intermediate states).  Inference only."""
    if x.dtype == torch.bfloat16:
        # bf16 model (stress configuration): same launch shape, bf16 storage, fp32 statistics
        x2 = _chk(x.contiguous(), "x", torch.bfloat16)
        r2 = _chk(residual.contiguous(), "residual", torch.bfloat16)
        p2 = _chk(pos.contiguous(), "pos", torch.bfloat16)
        _chk(ln.weight, "ln.weight", torch.bfloat16)
        rows, prow = x2.numel() // 256, p2.numel() // 256
        if x2.shape[-1] != 256 or rows % prow != 0 or out is not None:
            raise ValueError("add_layer_norm_pos (bf16): d_model must be 256, pos must tile the rows, no `out`")
        y, yp = torch.empty_like(x2), torch.empty_like(x2)
        _lib.launch("egtr_add_layernorm_pos_bf16", x2.data_ptr(), r2.data_ptr(), ln.weight.data_ptr(), ln.bias.data_ptr(),
                    y.data_ptr(), rows, 256, float(ln.eps), p2.data_ptr(), prow, yp.data_ptr())
        return y, yp
    x2 = _chk(x.contiguous(), "x", torch.float32)
    r2 = _chk(residual.contiguous(), "residual", torch.float32)
    p2 = _chk(pos.contiguous(), "pos", torch.float32)
    rows = x2.numel() // 256
    prow = p2.numel() // 256
    if x2.shape[-1] != 256 or rows % prow != 0:
        raise ValueError("add_layer_norm_pos: d_model must be 256 and pos must tile the rows")
    y = torch.empty_like(x2) if out is None else _chk(out, "out", torch.float32)
    if y.shape != x2.shape:
        raise ValueError("add_layer_norm_pos: out must have the shape of x")
    yp = torch.empty_like(x2)
    _lib.launch("egtr_add_layernorm_pos_f32", x2.data_ptr(), r2.data_ptr(), ln.weight.data_ptr(), ln.bias.data_ptr(),
                y.data_ptr(), rows, 256, float(ln.eps), p2.data_ptr(), prow, yp.data_ptr())
    return y, yp


def scale_rows_multi(tensors, scales):
    """[t * s for t, s in zip(tensors, scales)] with s one value per row of t (shape [rows, 1, ...]), in one launch per 64
    tensors (egtr_scale_rows_multi_f32); tensors that do not qualify (not fp32 / columns not a multiple of 4) are multiplied by
    torch.  No autograd."""
    import ctypes
    out = [None] * len(tensors)
    todo = []
    for i, (t, s) in enumerate(zip(tensors, scales)):
        rows = t.shape[0]
        cols = t.numel() // rows if rows else 0
        if (t.is_cuda and t.dtype == torch.float32 and s.dtype == torch.float32 and s.numel() == rows and cols > 0
                and cols % 4 == 0):
            tc = t.contiguous()
            if tc.data_ptr() % 16 == 0:
                todo.append((i, tc, s.reshape(-1).contiguous(), rows, cols))
                continue
        out[i] = t * s
    for c0 in range(0, len(todo), 64):
        grp = todo[c0:c0 + 64]
        n = len(grp)
        res = [torch.empty_like(g[1]) for g in grp]
        PA, IA = ctypes.c_void_p * n, ctypes.c_int * n
        _lib.launch("egtr_scale_rows_multi_f32", n, PA(*[g[1].data_ptr() for g in grp]), PA(*[g[2].data_ptr() for g in grp]),
                    PA(*[r.data_ptr() for r in res]), IA(*[g[3] for g in grp]), IA(*[g[4] for g in grp]))
        for g, r in zip(grp, res):
            out[g[0]] = r
    return out


def sine_position_embedding(pixel_mask, embedding_dim, temperature, scale, eps=1e-6):
    """DeformableDetrSinePositionEmbedding(normalize=True) (dd:850-876) with the ~20 elementwise kernels after the two
    cumulative sums fused into one HIP kernel.  pixel_mask [B,H,W] bool/int -> [B, 2*embedding_dim, H, W] fp32."""
    y_embed = pixel_mask.cumsum(1, dtype=torch.float32).contiguous()
    x_embed = pixel_mask.cumsum(2, dtype=torch.float32).contiguous()
    dim_t = torch.arange(embedding_dim, dtype=torch.float32, device=pixel_mask.device)
    dim_t = temperature ** (2 * torch.div(dim_t, 2, rounding_mode="trunc") / embedding_dim)
    B, H, W_ = pixel_mask.shape
    out = torch.empty(B, 2 * embedding_dim, H, W_, dtype=torch.float32, device=pixel_mask.device)
    _lib.launch("egtr_sine_pos_embed_f32", y_embed.data_ptr(), x_embed.data_ptr(), dim_t.data_ptr(), out.data_ptr(), B, H, W_,
                embedding_dim, float(scale), float(eps))
    return out


def input_proj_groupnorm_flatten(conv_outputs, input_projs):
    """Conv bias + GroupNorm + flatten(2).transpose(1, 2) + cat over the levels (dd:2209-2262) in two HIP launches.
    ``conv_outputs[l]``: bias-free output [B,256,H_l,W_l] of ``input_projs[l][0]`` (fp32, or bf16 for a bf16 model: bf16
    activations in and out, fp32 statistics); ``input_projs[l]`` = Sequential(Conv2d, GroupNorm).  Returns [B, S, 256].
    Inference only."""
    import ctypes
    L = len(conv_outputs)
    B, C = conv_outputs[0].shape[:2]
    gn0 = input_projs[0][1]
    dt = conv_outputs[0].dtype
    if dt not in (torch.float32, torch.bfloat16):
        raise TypeError("input_proj_groupnorm_flatten: fp32 or bf16 convolution outputs")
    xs = [_chk(x.contiguous(), "conv output", dt) for x in conv_outputs]
    for proj in input_projs[:L]:
        conv, gn = proj[0], proj[1]
        if gn.num_groups != gn0.num_groups or gn.eps != gn0.eps or conv.bias is None:
            raise ValueError("input_proj_groupnorm_flatten: levels must share the GroupNorm configuration")
    srcs = [t for proj in input_projs[:L] for t in (proj[0].bias, proj[1].weight, proj[1].bias)]
    if dt == torch.float32:
        keep = [tuple(_chk(t.detach().contiguous(), "input_proj parameter", torch.float32) for t in srcs[3 * l:3 * l + 3])
                for l in range(L)]
    else:   # the kernel takes fp32 parameters: widened once per parameter version
        flat = cached_weights(input_projs, "gn_params_f32", srcs,
                              lambda: [t.detach().float().contiguous() for t in srcs])
        keep = [tuple(flat[3 * l:3 * l + 3]) for l in range(L)]
    hw = [int(v) for x in xs for v in x.shape[-2:]]
    S = sum(h * w for h, w in zip(hw[0::2], hw[1::2]))
    out = torch.empty(B, S, C, dtype=dt, device=xs[0].device)
    stats = torch.empty(L * B * gn0.num_groups * 2, dtype=torch.float32, device=xs[0].device)
    PA, IA = ctypes.c_void_p * L, ctypes.c_int * (2 * L)
    entry = "egtr_input_proj_groupnorm_flatten_f32" if dt == torch.float32 else "egtr_input_proj_groupnorm_flatten_bf16"
    _lib.launch(entry, L, PA(*[x.data_ptr() for x in xs]), PA(*[k[0].data_ptr() for k in keep]),
                PA(*[k[1].data_ptr() for k in keep]), PA(*[k[2].data_ptr() for k in keep]), IA(*hw), B, C, gn0.num_groups,
                float(gn0.eps), stats.data_ptr(), out.data_ptr())
    return out


def input_proj_groupnorm_tokens(token_outputs, input_projs):
    """The same for TOKEN-MAJOR projections [B, H_l*W_l, 256] (the channels-last backbone: the level's 1x1 convolution run as a
    plain GEMM, bias-free; bf16 or fp32): conv bias + GroupNorm(32) + concatenation in two launches, no transpose
    (egtr_input_proj_groupnorm_tokens_bf16 / _f32).  Returns [B, S, 256].  Inference only."""
    import ctypes
    lib = _lib.lib()
    L = len(token_outputs)
    B = token_outputs[0].shape[0]
    gn0 = input_projs[0][1]
    dt = token_outputs[0].dtype
    if dt not in (torch.bfloat16, torch.float32):
        raise TypeError("input_proj_groupnorm_tokens: bf16 or fp32 projections")
    xs = [_chk(x.contiguous(), "token-major projection", dt) for x in token_outputs]
    for proj, x in zip(input_projs[:L], xs):
        conv, gn = proj[0], proj[1]
        if gn.num_groups != 32 or gn.eps != gn0.eps or conv.bias is None or x.shape[-1] != 256 or x.shape[0] != B:
            raise ValueError("input_proj_groupnorm_tokens: 256 channels in 32 groups, one GroupNorm configuration")
    srcs = [t for proj in input_projs[:L] for t in (proj[0].bias, proj[1].weight, proj[1].bias)]
    flat = cached_weights(input_projs, "gn_params_f32", srcs, lambda: [t.detach().float().contiguous() for t in srcs])
    keep = [tuple(flat[3 * l:3 * l + 3]) for l in range(L)]
    toks = [int(x.shape[1]) for x in xs]
    S = sum(toks)
    out = torch.empty(B, S, 256, dtype=dt, device=xs[0].device)
    PA, IA = ctypes.c_void_p * L, ctypes.c_int * L
    stats = torch.empty(int(lib.egtr_input_proj_groupnorm_tokens_workspace_floats(L, IA(*toks), B)), dtype=torch.float32,
                        device=xs[0].device)
    entry = "egtr_input_proj_groupnorm_tokens_bf16" if dt == torch.bfloat16 else "egtr_input_proj_groupnorm_tokens_f32"
    _lib.launch(entry, L, PA(*[x.data_ptr() for x in xs]), PA(*[k[0].data_ptr() for k in keep]),
                PA(*[k[1].data_ptr() for k in keep]), PA(*[k[2].data_ptr() for k in keep]), IA(*toks), B, 256, 32,
                float(gn0.eps), stats.data_ptr(), out.data_ptr())
    return out


def input_proj_groupnorm_token_slabs(slabs, input_projs):
    """``input_proj_groupnorm_tokens`` on K-split partial products (egtr_input_proj_groupnorm_token_slabs_f32): ``slabs[l]`` is
    [S_l, B, H_l*W_l, 256] fp32 (``input_proj_x6``).  The statistics pass adds the slabs in order and leaves the sum in
    ``slabs[l][0]`` (the argument is MODIFIED); with S_l = 1 this is ``input_proj_groupnorm_tokens``.  Returns [B, S, 256]."""
    import ctypes
    lib = _lib.lib()
    L = len(slabs)
    B = slabs[0].shape[1]
    gn0 = input_projs[0][1]
    xs = [_chk(x, "slabs", torch.float32) for x in slabs]
    for proj, x in zip(input_projs[:L], xs):
        conv, gn = proj[0], proj[1]
        if gn.num_groups != 32 or gn.eps != gn0.eps or conv.bias is None or x.dim() != 4 or x.shape[-1] != 256 or x.shape[1] != B:
            raise ValueError("input_proj_groupnorm_token_slabs: [S, B, tokens, 256] slabs, 32 groups, one GroupNorm configuration")
    srcs = [t for proj in input_projs[:L] for t in (proj[0].bias, proj[1].weight, proj[1].bias)]
    flat = cached_weights(input_projs, "gn_params_f32", srcs, lambda: [t.detach().float().contiguous() for t in srcs])
    keep = [tuple(flat[3 * l:3 * l + 3]) for l in range(L)]
    toks = [int(x.shape[2]) for x in xs]
    out = torch.empty(B, sum(toks), 256, dtype=torch.float32, device=xs[0].device)
    PA, IA = ctypes.c_void_p * L, ctypes.c_int * L
    splits = IA(*[int(x.shape[0]) for x in xs])
    stats = torch.empty(int(lib.egtr_input_proj_groupnorm_token_slabs_workspace_floats(L, IA(*toks), splits, B)),
                        dtype=torch.float32, device=xs[0].device)
    _lib.launch("egtr_input_proj_groupnorm_token_slabs_f32", L, PA(*[x.data_ptr() for x in xs]), splits, PA(*[k[0].data_ptr() for k in keep]), PA(*[k[1].data_ptr() for k in keep]),
                PA(*[k[2].data_ptr() for k in keep]), IA(*toks), B, 256, 32, float(gn0.eps), stats.data_ptr(), out.data_ptr())
    return out


_DIM_T = {}


def level_geometry(pixel_mask, spatial_shapes_list, level_embed, embedding_dim, temperature, scale, eps=1e-6):
    """Everything DeformableDetrModel.forward derives from ``pixel_mask`` alone, in one HIP kernel
    (egtr_level_geometry_f32): returns (mask_flatten [B,S] bool, lvl_pos_embed_flatten [B,S,2E] incl. level_embed,
    valid_ratios [B,L,2], encoder reference_points [B,S,L,2], mask bits [B, ceil(S/32)] int32 -- the mask packed one bit per
    token, which the model hands to the fused MSDA kernels as ``mask_bits``).  A bf16 ``level_embed`` (bf16 model) gives bf16 position rows
    rounded like the reference's composition (egtr_level_geometry_bf16); everything else stays fp32.  Inference only (no
    autograd through level_embed)."""
    import ctypes
    dev = pixel_mask.device
    key = (embedding_dim, float(temperature), str(dev))
    dim_t = _DIM_T.get(key)
    if dim_t is None:  # a constant of the module configuration (dd:864-865)
        dim_t = torch.arange(embedding_dim, dtype=torch.float32, device=dev)
        dim_t = temperature ** (2 * torch.div(dim_t, 2, rounding_mode="trunc") / embedding_dim)
        _DIM_T[key] = dim_t
    if pixel_mask.dtype not in (torch.int64, torch.uint8, torch.bool):
        pixel_mask = (pixel_mask != 0).to(torch.uint8)
    pm = pixel_mask.contiguous()
    _chk(pm, "pixel_mask")
    pos_dtype = level_embed.dtype
    if pos_dtype == torch.bfloat16:
        le = level_embed.detach().float().contiguous()     # exact; [L, 2E]
    else:
        le = _chk(level_embed.detach().contiguous(), "level_embed", torch.float32)
    B, H, W_ = pm.shape
    L = len(spatial_shapes_list)
    S = sum(h * w for h, w in spatial_shapes_list)
    hw = (ctypes.c_int * (2 * L))(*[int(v) for hw_ in spatial_shapes_list for v in hw_])
    mask_u8 = torch.empty(B, S, dtype=torch.uint8, device=dev)
    bits = torch.empty(B, (S + 31) // 32, dtype=torch.int32, device=dev)
    pos = torch.empty(B, S, 2 * embedding_dim, dtype=pos_dtype, device=dev)
    vr = torch.empty(B, L, 2, dtype=torch.float32, device=dev)
    ref = torch.empty(B, S, L, 2, dtype=torch.float32, device=dev)
    entry = "egtr_level_geometry_bf16" if pos_dtype == torch.bfloat16 else "egtr_level_geometry_f32"
    _lib.launch(entry, pm.data_ptr(), pm.element_size(), dim_t.data_ptr(), le.data_ptr(), hw, L, B, H, W_, embedding_dim,
                float(scale), float(eps), mask_u8.data_ptr(), pos.data_ptr(), vr.data_ptr(), ref.data_ptr(), bits.data_ptr())
    # `bits`: one bit per token, consumed by the fused MSDA kernels (kept in LDS there) -- returned, and handed down by the
    # model as an explicit `mask_bits` argument (until round 5 it travelled as a Python attribute on the mask tensor)
    return mask_u8.view(torch.bool), pos, vr, ref, bits
