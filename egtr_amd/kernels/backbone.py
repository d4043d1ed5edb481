"""Bindings of the backbone kernels (the XS operand split, the stem, the 3x3 / strided 1x1 convolutions, the bottleneck tails, the
bias / activation passes): validate the tensors, allocate the outputs, launch one C entry.  No routing decisions here -- which
kernel serves a call is decided in ``egtr_amd.ops``, which re-exports every name below."""
import torch

from .. import _lib
from .._lib import _chk

__all__ = ["bias_relu_maxpool", "xs_bytes", "xs_split", "conv1x1_tail", "stem_weights", "stem_weights_bf16", "stem_fused_bf16",
           "stem_fused", "conv3x3_weights", "conv3x3", "conv1x1_strided", "conv_tail_pack_bf16", "conv1x1_tail_bf16",
           "bias_act_rows_", "bias_act_", "input_proj_x6_plan", "input_proj_x6_weights", "input_proj_x6"]


def bias_relu_maxpool(x, bias):
    """relu(max_pool2d(x, 3, 2, 1) + bias[c]) in one HIP pass (== max_pool2d(relu(x + bias[c]), 3, 2, 1) bit for bit): the
    ResNet stem epilogue.  fp32 NCHW, inference only."""
    N, C, H, W_ = x.shape
    x2 = _chk(x.contiguous(), "x", torch.float32)
    b2 = _chk(bias.contiguous(), "bias", torch.float32)
    y = torch.empty(N, C, (H - 1) // 2 + 1, (W_ - 1) // 2 + 1, dtype=torch.float32, device=x.device)
    _lib.launch("egtr_bias_relu_maxpool3x3s2_f32", x2.data_ptr(), b2.data_ptr(), y.data_ptr(), N, C, H, W_)
    return y


# ---- the XS operand format (csrc/xs_format.h, csrc/xs_split.hip): weights of the row-panel kernels ----------------------
def xs_bytes(rows, K):
    return int(_lib.lib().egtr_xs_bytes(int(rows), int(K)))


def xs_split(x, pos=None, weights=False, plain=True):
    """fp32 [rows, K] (unit inner stride) -> XS(x): the exact three-way bf16 split in 1 KiB MFMA-operand fragments
    (csrc/xs_format.h; egtr_xs_split_f32), a flat uint8 tensor.  ``pos`` [pos_rows, K]: also XS(x + pos[row % pos_rows]);
    returns (XS(x) or None when ``plain`` is False, XS(x + pos)).  ``weights``: pieces rounded to nearest even."""
    K = x.shape[-1]
    x2 = _lib.row_view(x, K)
    if not x2.is_cuda or x2.dtype != torch.float32:
        raise RuntimeError("xs_split: x must be a float32 CUDA/HIP tensor")
    rows = x2.shape[0]
    n = xs_bytes(rows, K)
    if n == 0:
        raise RuntimeError(f"xs_split: K = {K} must be a multiple of 16")
    out = torch.empty(n, dtype=torch.uint8, device=x.device) if plain else None
    out_pos, p2 = None, None
    if pos is not None:
        p2 = _chk(pos.reshape(-1, K).contiguous(), "pos", torch.float32)
        out_pos = torch.empty(n, dtype=torch.uint8, device=x.device)
    _lib.launch("egtr_xs_split_f32", x2.data_ptr(), x2.stride(0), _lib.ptr(p2), p2.shape[0] if p2 is not None else 0, rows, K,
                _lib.ptr(out), _lib.ptr(out_pos), 1 if weights else 0)
    return out if pos is None else (out, out_pos)


def conv1x1_tail(a, a_shift, w_xs, bias, shortcut, N, relu_in=True, relu_out=True, tile=(0, 0)):
    """relu(relu(a + a_shift) W^T + bias + shortcut) in ONE HIP launch (egtr_conv1x1_tail_x6_f32): the last 1x1 convolution of
    a ResNet bottleneck on channels-last fp32 rows together with the shift + ReLU in front of it and the shift + shortcut +
    ReLU behind it (reference: model/deformable_detr.py:735-760, the timm ResNet-50 backbone with frozen batch norm).
    ``a`` [M, K] raw 3x3-convolution output, ``w_xs`` = ``xs_split(W [N, K], weights=True)``, ``shortcut`` [M, N] or None.
    fp32-level accuracy (six-term split-bf16 products).  Inference only."""
    M, K = a.shape
    for name, t in (("a_shift", a_shift), ("bias", bias), ("shortcut", shortcut)):
        if t is not None and (not t.is_cuda or t.dtype != torch.float32 or t.stride(-1) != 1):
            raise RuntimeError(f"conv1x1_tail: {name} must be a float32 device tensor with unit inner stride")
    y = torch.empty(M, N, dtype=torch.float32, device=a.device)
    _lib.launch("egtr_conv1x1_tail_x6_f32", a.data_ptr(), a.stride(0), _lib.ptr(a_shift), 1 if relu_in else 0, w_xs.data_ptr(),
                _lib.ptr(bias), _lib.ptr(shortcut), shortcut.stride(0) if shortcut is not None else 0, 1 if relu_out else 0,
                y.data_ptr(), y.stride(0), M, K, N, int(tile[0]), int(tile[1]))
    return y


def stem_weights(w):
    """W [64, 3, 7, 7] fp32 (frozen BN scale folded in) -> the XS operand stream of the [64, 224] matrix the stem kernel walks:
    per kernel row 8 taps x 4 channels, the padded tap / channel zeros (csrc/stem_x6.hip)."""
    wm = torch.zeros(64, 7, 8, 4, dtype=torch.float32, device=w.device)
    wm[:, :, :7, :3] = w.detach().permute(0, 2, 3, 1)
    return xs_split(wm.reshape(64, 224), weights=True)


def stem_weights_bf16(w):
    """W [64, 3, 7, 7] bf16 (frozen BN scale folded in) -> the packed MFMA-operand stream of the bf16 stem kernel
    (csrc/stem_bf16.hip): per kernel row 8 taps x 4 channels, the padded tap / channel zeros."""
    wm = torch.zeros(64, 7, 8, 4, dtype=torch.bfloat16, device=w.device)
    wm[:, :, :7, :3] = w.detach().permute(0, 2, 3, 1)
    return conv_tail_pack_bf16(wm.reshape(64, 224).contiguous())


def stem_fused_bf16(x, w_packed, bias):
    """The bf16 twin of ``stem_fused`` (egtr_stem_conv7x7_pool_bf16): x [B, 3, H, W] NCHW bf16 -> channels-last bf16
    [B, 64, Hp, Wp]; ``bias`` fp32.  Inference only."""
    B, _, H, W = x.shape
    Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    Hp, Wp = (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1
    y = torch.empty((B, 64, Hp, Wp), dtype=torch.bfloat16, device=x.device, memory_format=torch.channels_last)
    _lib.launch("egtr_stem_conv7x7_pool_bf16", x.data_ptr(), w_packed.data_ptr(), bias.data_ptr(), y.data_ptr(), B, H, W)
    return y


def stem_fused(x, w_xs, bias):
    """maxpool3x3/2(relu(conv7x7/2(x) + bias)) of the ResNet stem in ONE HIP launch (egtr_stem_conv7x7_pool_x6_f32; reference:
    timm ResNet-50 conv1 -> bn1 -> act1 -> maxpool, model/deformable_detr.py:735-760).  x [B, 3, H, W] NCHW fp32 -> a
    channels-last [B, 64, Hp, Wp] tensor.  fp32-level accuracy (six-term split-bf16 products).  Inference only."""
    B, _, H, W = x.shape
    Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    Hp, Wp = (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1
    y = torch.empty((B, 64, Hp, Wp), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    _lib.launch("egtr_stem_conv7x7_pool_x6_f32", x.data_ptr(), w_xs.data_ptr(), bias.data_ptr(), y.data_ptr(), B, H, W)
    return y


def conv3x3_weights(w, stride=1, variant=0):
    """W [N, C, 3, 3] fp32 -> the XS operand stream of the [N, 9 C] matrix the kernel for (C, N, stride, variant) walks: channels
    in phases of CP (egtr_conv3x3_phase_channels), within a phase W[n][dy][dx][c'] (csrc/conv3x3_x6.hip)."""
    N, C = w.shape[:2]
    cp = int(_lib.lib().egtr_conv3x3_phase_channels(int(C), int(N), int(stride), int(variant)))
    if cp <= 0:
        raise RuntimeError(f"conv3x3_weights: C = {C}, N = {N}, stride {stride} is not served")
    wm = w.detach().reshape(N, C // cp, cp, 3, 3).permute(0, 1, 3, 4, 2).reshape(N, 9 * C).contiguous()
    return xs_split(wm, weights=True)


def conv3x3(x, w_xs, N, stride=1, variant=0, in_shift=None):
    """3x3 convolution, stride 1 or 2, padding 1, no bias, on a channels-last fp32 tensor in ONE HIP launch with fp32-level
    accuracy on the bf16 matrix cores (egtr_conv3x3_x6_f32; reference: the timm ResNet-50 bottleneck's conv2,
    model/deformable_detr.py:735-760).  ``w_xs`` from ``conv3x3_weights`` with the same stride / variant.  Returns a channels-last
    [B, N, Ho, Wo] tensor.  Inference only.
    ``in_shift`` ([C] fp32): the convolution of relu(x + in_shift[c]) instead -- the preceding bias-free conv1's folded-BN shift +
    ReLU applied while the input tile is loaded, the padding staying zero (egtr_conv3x3_x6_shift_f32)."""
    B, C, H, W = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    y = torch.empty((B, N, Ho, Wo), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    if in_shift is None:
        _lib.launch("egtr_conv3x3_x6_f32", x.data_ptr(), w_xs.data_ptr(), y.data_ptr(), B, H, W, C, N, int(stride), int(variant))
        return y
    if (not in_shift.is_cuda or in_shift.dtype != torch.float32 or in_shift.dim() != 1 or in_shift.shape[0] != C
            or not in_shift.is_contiguous()):
        raise RuntimeError(f"conv3x3: in_shift must be a contiguous float32 [{C}] device tensor")
    _lib.launch("egtr_conv3x3_x6_shift_f32", x.data_ptr(), in_shift.data_ptr(), w_xs.data_ptr(), y.data_ptr(), B, H, W, C, N,
                int(stride), int(variant))
    return y


def conv1x1_strided(x, w_xs, N, stride):
    """1x1 convolution with stride (no padding, no bias) on a channels-last fp32 tensor in ONE HIP launch
    (egtr_conv1x1_strided_x6_f32): a bottleneck's shortcut projection; ``w_xs`` = ``xs_split(W [N, C], weights=True)``.  Returns
    the rows [B Ho Wo, N].  fp32-level accuracy.  Inference only."""
    B, C, H, W = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    y = torch.empty(B * Ho * Wo, N, dtype=torch.float32, device=x.device)
    _lib.launch("egtr_conv1x1_strided_x6_f32", x.data_ptr(), w_xs.data_ptr(), y.data_ptr(), B, H, W, C, N, int(stride))
    return y


def conv_tail_pack_bf16(w):
    """W [N, K] bf16 -> the MFMA-operand stream of the bf16 bottleneck-tail kernel (egtr_conv1x1_tail_pack_weights_bf16)."""
    w = w.detach()
    if not w.is_cuda or w.dtype != torch.bfloat16 or w.dim() != 2 or w.stride(1) != 1:
        raise RuntimeError("conv_tail_pack_bf16: a 2-d bfloat16 device tensor with unit inner stride expected")
    N, K = w.shape
    out = torch.empty(N * K, dtype=torch.bfloat16, device=w.device)
    _lib.launch("egtr_conv1x1_tail_pack_weights_bf16", w.data_ptr(), w.stride(0), N, K, out.data_ptr())
    return out


def conv1x1_tail_bf16(a, a_shift, w_packed, bias, shortcut, N, relu_in=True, relu_out=True):
    """relu(bf16(relu(a + a_shift) W^T) + bias + shortcut) in ONE HIP launch (egtr_conv1x1_tail_bf16): the bf16 twin of
    ``conv1x1_tail`` with the rounding points of the pass / GEMM / pass composition it replaces.  ``a`` [M, K] and ``shortcut``
    [M, N] bf16, shifts fp32, ``w_packed`` from ``conv_tail_pack_bf16``.  Inference only."""
    M, K = a.shape
    for name, t, dt in (("a_shift", a_shift, torch.float32), ("bias", bias, torch.float32), ("shortcut", shortcut, torch.bfloat16)):
        if t is not None and (not t.is_cuda or t.dtype != dt or t.stride(-1) != 1):
            raise RuntimeError(f"conv1x1_tail_bf16: {name} must be a {dt} device tensor with unit inner stride")
    y = torch.empty(M, N, dtype=torch.bfloat16, device=a.device)
    _lib.launch("egtr_conv1x1_tail_bf16", a.data_ptr(), a.stride(0), _lib.ptr(a_shift), 1 if relu_in else 0,
                w_packed.data_ptr(), _lib.ptr(bias), _lib.ptr(shortcut), shortcut.stride(0) if shortcut is not None else 0,
                1 if relu_out else 0, y.data_ptr(), y.stride(0), M, K, N)
    return y


def bias_act_rows_(x2d, bias, residual=None, relu=True):
    """In-place y = act(x + bias[c] (+ residual)) on a channels-last activation given as its [rows, C] matrix (bf16 or fp32
    activations, fp32 bias: egtr_bias_act_nhwc_bf16 / _f32).  Inference only."""
    dt = x2d.dtype
    if dt not in (torch.bfloat16, torch.float32):
        raise TypeError("bias_act_rows_: bf16 or fp32 activations")
    _chk(x2d, "x", dt)
    _chk(bias, "bias", torch.float32)
    if residual is not None:
        _chk(residual, "residual", dt)
        if residual.shape != x2d.shape:
            raise ValueError("bias_act_rows_: residual must have the shape of x")
    rows, C = x2d.shape
    entry = "egtr_bias_act_nhwc_bf16" if dt == torch.bfloat16 else "egtr_bias_act_nhwc_f32"
    _lib.launch(entry, x2d.data_ptr(), bias.data_ptr(), _lib.ptr(residual), x2d.data_ptr(), rows, C, 1 if relu else 0)
    return x2d


def bias_act_(x, bias, residual=None, relu=True):
    """In-place y = act(x + bias[c] (+ residual)) on an NCHW activation (inference only, no autograd).  fp32, or bf16
    activations with an fp32 bias."""
    N, C, H, W_ = x.shape
    if x.dtype == torch.bfloat16:
        _chk(x, "x", torch.bfloat16)
        _chk(bias, "bias", torch.float32)
        if residual is not None:
            _chk(residual, "residual", torch.bfloat16)
        _lib.launch("egtr_bias_act_nchw_bf16", x.data_ptr(), bias.data_ptr(), _lib.ptr(residual), x.data_ptr(), N, C, H * W_,
                    1 if relu else 0)
        return x
    _chk(x, "x", torch.float32)
    _chk(bias, "bias", torch.float32)
    if residual is not None:
        _chk(residual, "residual", torch.float32)
    _lib.launch("egtr_bias_act_nchw_f32", x.data_ptr(), bias.data_ptr(), _lib.ptr(residual), x.data_ptr(), N, C, H * W_,
                1 if relu else 0)
    return x


# ---- the input projections of all levels as one grouped, K-split launch (csrc/input_proj_x6.hip) ---------------------------------
def input_proj_x6_plan(rows, K, tap_channels):
    """(splits S_l per level, workspace floats) for levels of ``rows[l]`` output rows and reduction length ``K[l]``;
    ``tap_channels[l]`` = C of a 3x3 / stride 2 level (K = 9 C), 0 of a plain one (egtr_input_proj_x6_workspace_floats: a function
    of the shapes alone, no device needed).  Raises for shapes the kernel does not serve."""
    import ctypes
    L = len(rows)
    IA = ctypes.c_int * L
    splits = IA()
    n = int(_lib.lib().egtr_input_proj_x6_workspace_floats(L, IA(*[int(v) for v in rows]), IA(*[int(v) for v in K]),
                                                           IA(*[int(v) for v in tap_channels]), splits))
    if n <= 0:
        raise RuntimeError(f"input_proj_x6_plan: rows {list(rows)}, K {list(K)}, tap channels {list(tap_channels)} are not served")
    return [int(v) for v in splits], n


def input_proj_x6_weights(w):
    """Conv2d weight [256, C, kh, kw] fp32 (1x1 or 3x3) -> the operand stream of the grouped kernel: the [256, kh kw C] matrix
    laid out [n][dy][dx][c], split round-to-nearest and tiled like ``gemm_split_tile`` ([N/128][K/32][3 pieces][128][32] bf16)."""
    w = w.detach()
    N = w.shape[0]
    wm = w.permute(0, 2, 3, 1).reshape(N, -1).contiguous()
    out = torch.empty(N // 128, wm.shape[1] // 32, 3, 128, 32, dtype=torch.bfloat16, device=w.device)
    _lib.launch("egtr_gemm_split_tile_weights_f32", wm.data_ptr(), wm.stride(0), 0, N, wm.shape[1], out.data_ptr(), 6)
    return out


def input_proj_x6(maps, w_tiled, strided3x3, splits=None, slabs=None):
    """The bias-free input projections of all levels in ONE launch (egtr_input_proj_x6_f32).  Level l multiplies ``maps[l]``
    (channels-last fp32 [B, C_l, H_l, W_l]) by ``w_tiled[l]`` (``input_proj_x6_weights``): a 1x1 convolution, or, where
    ``strided3x3[l]``, a 3x3 / stride 2 / padding 1 convolution (the extra level, of the last feature map).  Returns (slabs,
    splits, shapes): ``slabs[l]`` [S_l, B, H'_l W'_l, 256] fp32 partial products over the S_l ranges of K (their sum over dim
    0 is the projection), ``shapes[l]`` = (H'_l, W'_l) of the output.  ``splits``: the plan's own when None; ``slabs``: the caller's buffers of exactly those shapes.
    Inference only."""
    import ctypes
    L = len(maps)
    if not (L == len(w_tiled) == len(strided3x3)):
        raise ValueError("input_proj_x6: one weight and one kind per level")
    B = maps[0].shape[0]
    rows, Ks, tapc, geom, shapes = [], [], [], [], []
    for fm, conv in zip(maps, strided3x3):
        b, c, h, w = fm.shape
        if (not fm.is_cuda or fm.dtype != torch.float32 or b != B or not fm.is_contiguous(memory_format=torch.channels_last)
                or fm.data_ptr() % 16):
            raise RuntimeError("input_proj_x6: channels-last float32 device feature maps, 16-byte aligned")
        if conv:
            ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
            rows.append(b * ho * wo)
            Ks.append(9 * c)
            tapc.append(c)
            geom += [b, h, w, c]
            shapes.append((ho, wo))
        else:
            rows.append(b * h * w)
            Ks.append(c)
            tapc.append(0)
            geom += [0, 0, 0, 0]
            shapes.append((h, w))
    for l in range(L):
        if w_tiled[l].numel() != 3 * 256 * Ks[l] or w_tiled[l].dtype != torch.bfloat16:
            raise ValueError(f"input_proj_x6: weight stream {l} is not that of a [256, {Ks[l]}] matrix")
    plan, _ = input_proj_x6_plan(rows, Ks, tapc)
    splits = plan if splits is None else [int(v) for v in splits]
    want = [(splits[l], B, rows[l] // B, 256) for l in range(L)]
    if slabs is None:
        slabs = [torch.empty(w, dtype=torch.float32, device=maps[0].device) for w in want]
    elif [tuple(t.shape) for t in slabs] != want or any(t.dtype != torch.float32 or not t.is_contiguous() for t in slabs):
        raise ValueError(f"input_proj_x6: slabs must be contiguous float32 tensors of shapes {want}")
    PA, IA = ctypes.c_void_p * L, ctypes.c_int * L
    _lib.launch("egtr_input_proj_x6_f32", L, PA(*[x.data_ptr() for x in maps]), PA(*[w.data_ptr() for w in w_tiled]),
                PA(*[s.data_ptr() for s in slabs]), IA(*rows), IA(*Ks), (ctypes.c_int * (4 * L))(*geom), IA(*splits), 256)
    return slabs, splits, shapes
