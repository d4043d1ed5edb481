"""The routing and autograd layer over the HIP kernels of libegtr_hip.so, and the package's public op namespace.

What lives here: the route switches (``EGTR_*`` and the patchable module attributes), ``FALLBACKS`` / ``note_fallback`` / ``_gate``, the
``*_supported`` predicates, the dispatchers (``linear``, ``module_linear``, ``relation_head`` ...) and every ``autograd.Function``.
The thin bindings -- validate tensors, allocate outputs, launch one C entry -- live in ``egtr_amd.kernels`` and are re-exported
below, so ``ops.<name>`` stays the one spelling callers use.  Tests and tools rebind names ON THIS MODULE (the switches, ``_msda``,
``decoder_self_attention``, ``relation_head``, ``msda_forward_fused``, the backbone's convolution launches): every reader of such a
name resolves it in this module's namespace -- no kernels module reads a switch, calls one of those functions or imports ``ops``.

Every op enqueues on torch's current HIP stream through the C ABI (include/egtr_hip.h); none has a CPU or eager-PyTorch
fallback -- a missing library raises ``egtr_amd._lib.EgtrHipError``.
"""
import os

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib
from . import targets as rel_targets
from ._lib import _chk, _stream  # noqa: F401  (``_stream``: part of this namespace since the first round)
from .kernels.backbone import *  # noqa: F401,F403
from .kernels.derived import *  # noqa: F401,F403
from .kernels.elementwise import *  # noqa: F401,F403
from .kernels.elementwise import _DIM_T  # noqa: F401
from .kernels.heads import *  # noqa: F401,F403
from .kernels.linear import *  # noqa: F401,F403
from .kernels.linear import _c16, _skinny_bwd, _skinny_fwd, _split3_bf16, _wgrad_ex  # noqa: F401
from .kernels.protocols import *  # noqa: F401,F403
from .kernels.statistics import *  # noqa: F401,F403
from .kernels.vrd import *  # noqa: F401,F403
from .load_custom import load_hip_kernels

_MSDA = None


def _msda():
    global _MSDA
    if _MSDA is None:
        _MSDA = load_hip_kernels()
    return _MSDA


class MultiScaleDeformableAttentionFunction(Function):
    """Same contract as the reference's autograd Function (model/deformable_detr.py:402-455)."""

    @staticmethod
    def forward(context, value, value_spatial_shapes, value_level_start_index, sampling_locations,
                attention_weights, im2col_step):
        context.im2col_step = im2col_step
        if value.dtype == torch.bfloat16:  # bf16 values, fp32 sampling geometry (csrc: msda_fwd_q32_bf16)
            sampling_locations, attention_weights = sampling_locations.float(), attention_weights.float()
        output = _msda().ms_deform_attn_forward(value, value_spatial_shapes, value_level_start_index,
                                                sampling_locations, attention_weights, im2col_step)
        context.save_for_backward(value, value_spatial_shapes, value_level_start_index, sampling_locations,
                                  attention_weights)
        return output

    @staticmethod
    @once_differentiable
    def backward(context, grad_output):
        value, shapes, lsi, loc, attn = context.saved_tensors
        grad_value, grad_loc, grad_attn = _msda().ms_deform_attn_backward(
            value, shapes, lsi, loc, attn, grad_output.contiguous(), context.im2col_step)
        # bf16 values: loc / attn were promoted to fp32 in forward(); autograd casts their gradients back
        return grad_value, None, None, grad_loc, grad_attn, None


class MSDAGeometryFunction(Function):
    """(sampling_offsets [B, Lq, M*L*P*2], attention logits [B, Lq, M*L*P], reference_points [B, Lq, L, 2 | 4]) ->
    (sampling_locations [B, Lq, M, L, P, 2], attention_weights [B, Lq, M, L, P]) under autograd: softmax + location
    arithmetic of model/deformable_detr.py:1055-1073 in one pass per direction (csrc/msda_geom.hip).
    ``logits`` None: ``offsets`` is the output [B, Lq, 3*M*L*P] of ONE nn.Linear over the concatenated weights (offsets
    columns first); its gradient is then written as one buffer as well."""

    @staticmethod
    def forward(ctx, offsets, logits, reference_points, spatial_shapes, M, L, P):
        B, Lq = offsets.shape[:2]
        n_off = M * L * P * 2
        both = offsets.reshape(B * Lq, -1)
        both = both if both.stride(1) == 1 else both.contiguous()
        if logits is None:
            off, lg = both[:, :n_off], both[:, n_off:]
        else:
            off = both
            lg = logits.reshape(B * Lq, -1)
            lg = lg if lg.stride(1) == 1 else lg.contiguous()
        ref = _chk(reference_points.contiguous(), "reference_points", torch.float32)
        shp = _chk(spatial_shapes.contiguous(), "spatial_shapes", torch.int64)
        loc = torch.empty(B, Lq, M, L, P, 2, dtype=torch.float32, device=off.device)
        probs = torch.empty(B, Lq, M, L, P, dtype=torch.float32, device=off.device)
        _lib.launch("egtr_msda_geometry_forward_f32", off.data_ptr(), off.stride(0), lg.data_ptr(), lg.stride(0),
                    ref.data_ptr(), ref.shape[-1], shp.data_ptr(), loc.data_ptr(), probs.data_ptr(), B * Lq, M, L, P)
        ctx.save_for_backward(off, ref, shp, probs)
        ctx.dims = (M, L, P)
        ctx.shapes = (offsets.shape, logits.shape if logits is not None else None)
        return loc, probs

    @staticmethod
    @once_differentiable
    def backward(ctx, g_loc, g_probs):
        off, ref, shp, probs = ctx.saved_tensors
        M, L, P = ctx.dims
        rows = off.shape[0]
        n_off = M * L * P * 2
        g_loc = _chk(g_loc.contiguous(), "grad_locations", torch.float32)
        g_probs = _chk(g_probs.contiguous(), "grad_weights", torch.float32)
        g_off = torch.empty(ctx.shapes[0], dtype=torch.float32, device=off.device)
        if ctx.shapes[1] is None:
            g_lg, p_lg, ld_off, ld_lg = None, g_off.data_ptr() + 4 * n_off, g_off.shape[-1], g_off.shape[-1]
        else:
            g_lg = torch.empty(ctx.shapes[1], dtype=torch.float32, device=off.device)
            p_lg, ld_off, ld_lg = g_lg.data_ptr(), n_off, n_off // 2
        g_ref = torch.empty_like(ref) if ctx.needs_input_grad[2] else None
        _lib.launch("egtr_msda_geometry_backward_f32", g_loc.data_ptr(), g_probs.data_ptr(), probs.data_ptr(), off.data_ptr(),
                    off.stride(0), ref.data_ptr(), ref.shape[-1], shp.data_ptr(), g_off.data_ptr(), ld_off, p_lg, ld_lg,
                    _lib.ptr(g_ref), rows, M, L, P)
        return g_off, g_lg, g_ref, None, None, None, None


def msda_geometry_supported(offsets, logits, reference_points, M, L, P):
    """Shapes / dtypes served by MSDAGeometryFunction (else the ATen composition)."""
    def rows_ok(t):   # what egtr_msda_geometry_*_f32 asks of a row-strided operand: 16-byte base, row stride % 4 floats
        return t.data_ptr() % 16 == 0 and (t.stride(-1) != 1 or t.stride(-2) % 4 == 0)

    return (MSDA_GEOMETRY and offsets.is_cuda and offsets.dtype == torch.float32 and logits.dtype == torch.float32
            and reference_points.dtype == torch.float32 and L == 4 and P == 4 and M == 8
            and reference_points.shape[-1] in (2, 4) and offsets.dim() == 3 and logits.dim() == 3
            and reference_points.dim() == 4 and reference_points.shape[2] == L and M * L * P * 2 % 4 == 0
            and rows_ok(offsets) and rows_ok(logits))


MSDA_GEOMETRY = True   # module attribute (tests patch it for the switch-off twin); no environment switch since round 6


def msda_fused_supported(num_heads, channels, num_levels, num_points):
    """Shapes served by egtr_msda_forward_fused_f32 (the wave-per-query kernel)."""
    return num_heads == 8 and channels == 32 and num_levels * num_points == 16 and num_levels <= 4 \
        and num_points % 2 == 0


def msda_forward_fused(value, spatial_shapes, level_start_index, sampling_offsets, attn_logits, reference_points,
                       want_weights=False, keep_mask=None, value_bias=None, keep_bits=None):
    """MSDA forward with its softmax / sampling-location prologue fused in (no autograd: inference path).  With
    ``value_bias`` (fp32 only) ``value`` is the bias-free value projection and the kernel applies the bias.
    ``keep_bits``: the bit-packed copy of ``keep_mask`` (``level_geometry``'s fifth result), passed down explicitly."""
    from .load_custom import load_hip_kernels
    k = load_hip_kernels()
    if value.dtype == torch.bfloat16:
        if want_weights or value_bias is not None:
            raise NotImplementedError("the bf16 fused MSDA forward returns no attention weights and takes no value_bias")
        return k.ms_deform_attn_forward_fused_bf16(value, spatial_shapes, level_start_index, sampling_offsets,
                                                   attn_logits, reference_points, keep_mask, keep_bits=keep_bits), None
    return k.ms_deform_attn_forward_fused(value, spatial_shapes, level_start_index, sampling_offsets, attn_logits,
                                          reference_points, want_weights, keep_mask, value_bias=value_bias,
                                          keep_bits=keep_bits)


class DecoderSelfAttentionFunction(Function):
    """softmax(q k^T) v per head + the retained [B, M, N, D] maps of scaled q and k
    (replaces model/deformable_detr.py:1170-1253; q must already carry the D^-1/2 scaling of :1166)."""

    @staticmethod
    def forward(ctx, q, k, v, num_heads, want_maps):
        B, N, MD = q.shape
        D = MD // num_heads
        for t, n in ((q, "q"), (k, "k"), (v, "v")):
            _chk(t, n, torch.float32)
        out = torch.empty_like(q)
        need_bwd = q.requires_grad or k.requires_grad or v.requires_grad
        qh = torch.empty(B, num_heads, N, D, dtype=q.dtype, device=q.device) if want_maps else None
        kh = torch.empty_like(qh) if want_maps else None
        lse = torch.empty(B, num_heads, N, dtype=q.dtype, device=q.device) if need_bwd else None
        _lib.launch("egtr_self_attn_forward_f32", q.data_ptr(), k.data_ptr(), v.data_ptr(), B, N, num_heads, D, out.data_ptr(),
                    _lib.ptr(qh), _lib.ptr(kh), _lib.ptr(lse))
        ctx.num_heads = num_heads
        ctx.want_maps = want_maps
        if need_bwd:
            ctx.save_for_backward(q, k, v, out, lse)
        if want_maps:
            return out, qh, kh
        return out, None, None

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out, grad_qh, grad_kh):
        q, k, v, out, lse = ctx.saved_tensors
        B, N, MD = q.shape
        M = ctx.num_heads
        grad_out = grad_out.contiguous()
        gq, gk, gv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        _lib.launch("egtr_self_attn_backward_f32", q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr(),
                    grad_out.data_ptr(), B, N, M, MD // M, gq.data_ptr(), gk.data_ptr(), gv.data_ptr())
        # the retained maps are pure re-layouts of q and k: their gradients fold straight back
        if grad_qh is not None:
            gq = gq + grad_qh.transpose(1, 2).reshape(B, N, MD)
        if grad_kh is not None:
            gk = gk + grad_kh.transpose(1, 2).reshape(B, N, MD)
        return gq, gk, gv, None, None


SELF_ATTN_HEAD_DIM, SELF_ATTN_MAX_QUERIES = 32, 640   # what csrc/self_attn.hip serves (40 key tiles of 16 in registers)


def _self_attention_composed(q, k, v, num_heads, want_maps):
    """softmax(q k^T) v per head as batched GEMMs in the input dtype (the operation order of
    ``DeformableDetrMultiheadAttention._attention_with_map``), differentiable by ordinary autograd; the maps are views."""
    b, n, md = q.shape
    d = md // num_heads
    qh, kh, vh = (t.reshape(b, n, num_heads, d).transpose(1, 2) for t in (q, k, v))
    probs = torch.softmax(torch.matmul(qh, kh.transpose(2, 3)), dim=-1)
    out = torch.matmul(probs, vh).transpose(1, 2).reshape(b, n, md)
    return (out, qh, kh) if want_maps else (out, None, None)


def decoder_self_attention(q, k, v, num_heads, want_maps=True):
    # CPU tensors and other dtypes are not what the kernel exists for: they go on below exactly as before (and are refused there)
    if q.is_cuda and q.dtype in (torch.float32, torch.bfloat16):
        n, md = q.shape[1], q.shape[2]
        if not _gate("self_attention", True, md == SELF_ATTN_HEAD_DIM * num_heads and n <= SELF_ATTN_MAX_QUERIES,
                     lambda: f"{n} queries of head_dim {md / num_heads:g}: the kernel serves head_dim {SELF_ATTN_HEAD_DIM} and up to "
                             f"{SELF_ATTN_MAX_QUERIES} queries (batched GEMMs + softmax instead)"):
            return _self_attention_composed(q, k, v, num_heads, want_maps)
    if (q.dtype == torch.bfloat16 and q.is_cuda and k.dtype == v.dtype == torch.bfloat16 and q.shape[-1] == 32 * num_heads
            and q.shape[1] <= 640 and not (torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad))):
        # bf16 model at inference: the kernel reads and writes bf16 itself (fp32 arithmetic) -- no cast launches around it
        lib = _lib.lib()
        B, N, MD = q.shape
        q2, k2, v2 = (t if (t.is_contiguous() and t.data_ptr() % 16 == 0) else t.contiguous() for t in (q, k, v))
        out = torch.empty_like(q2)
        qh = torch.empty(B, num_heads, N, 32, dtype=q.dtype, device=q.device) if want_maps else None
        kh = torch.empty_like(qh) if want_maps else None
        _lib.launch("egtr_self_attn_forward_bf16", q2.data_ptr(), k2.data_ptr(), v2.data_ptr(), B, N, num_heads, 32,
                    out.data_ptr(), _lib.ptr(qh), _lib.ptr(kh))
        return out, qh, kh
    if q.dtype != torch.float32:  # fp16 models / bf16 under autograd: the kernel computes in fp32, results go back to the model dtype
        o, qm, km = DecoderSelfAttentionFunction.apply(q.float().contiguous(), k.float().contiguous(),
                                                       v.float().contiguous(), num_heads, want_maps)
        return o.to(q.dtype), (qm.to(q.dtype) if qm is not None else None), (km.to(q.dtype) if km is not None else None)
    return DecoderSelfAttentionFunction.apply(q.contiguous(), k.contiguous(), v.contiguous(), num_heads, want_maps)


SKINNY_BACKWARD_FUSED = True   # module attribute (tests patch it for the switch-off twin); no environment switch since round 6
# token-sized linears under autograd through TokenLinearFunction (split-bf16 forward / data / weight gradients); "0": plain autograd
TOKEN_LINEAR = os.environ.get("EGTR_TOKEN_LINEAR", "1") != "0"
SKINNY_MAX_ROWS = 4096  # above this the vendor GEMM (rocBLAS / hipBLASLt) fills the chip and is the right tool


class SkinnyLinearFunction(Function):
    """act((x W^T + b) * alpha) through egtr_linear_f32 (csrc/linear.hip).  Backward: egtr_linear_backward_f32 (data, weight
    and bias gradient in one launch) for N % 64 == 0, else vendor GEMMs + egtr_column_sum_f32."""

    @staticmethod
    def forward(ctx, x, weight, bias, alpha, relu):
        K = x.shape[-1]
        N = weight.shape[0]
        x2 = _chk(x.reshape(-1, K).contiguous(), "x", torch.float32)
        w = _chk(weight.contiguous(), "weight", torch.float32)
        b = _chk(bias.contiguous(), "bias", torch.float32) if bias is not None else None
        y = torch.empty(x2.shape[0], N, dtype=torch.float32, device=x.device)
        _lib.launch("egtr_linear_f32", x2.data_ptr(), w.data_ptr(), _lib.ptr(b), y.data_ptr(), x2.shape[0], K, N, float(alpha),
                    1 if relu else 0)
        ctx.alpha, ctx.relu, ctx.has_bias = float(alpha), bool(relu), bias is not None
        if x.requires_grad or weight.requires_grad or (bias is not None and bias.requires_grad):
            ctx.save_for_backward(x2, w, y if relu else None)
        return y.view(*x.shape[:-1], N)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        x2, w, y = ctx.saved_tensors
        g = grad_y.reshape(-1, grad_y.shape[-1])
        gb = None
        want_gb = ctx.has_bias and ctx.needs_input_grad[2]
        N, K = w.shape
        if SKINNY_BACKWARD_FUSED and N % 64 == 0 and K % 64 == 0 and g.dtype == torch.float32:
            # gx, gw, gb (+ ReLU mask and alpha) in one launch (egtr_linear_backward_f32)
            lib = _lib.lib()
            g = _chk(_c16(g), "grad", torch.float32)
            M = g.shape[0]
            gx = torch.empty(M, K, dtype=torch.float32, device=g.device) if ctx.needs_input_grad[0] else None
            gw = torch.empty(N, K, dtype=torch.float32, device=g.device) if ctx.needs_input_grad[1] else None
            gb = torch.empty(N, dtype=torch.float32, device=g.device) if want_gb else None
            if gx is not None or gw is not None or gb is not None:
                _lib.launch("egtr_linear_backward_f32", g.data_ptr(), y.data_ptr() if ctx.relu else None, x2.data_ptr(),
                            w.data_ptr(), ctx.alpha, _lib.ptr(gx), _lib.ptr(gw), _lib.ptr(gb), M, K, N)
            return (gx.view(*grad_y.shape[:-1], K) if gx is not None else None), gw, gb, None, None
        if ctx.relu and ctx.alpha == 1.0 and want_gb:
            g, gb = column_sum(g, relu_output=y)   # ReLU mask and bias gradient in one pass
        else:
            if ctx.relu:
                g = g * (y > 0).to(g.dtype)
            if ctx.alpha != 1.0:
                g = g * ctx.alpha
            if want_gb:
                gb = column_sum(g)
        gx = (g @ w).view(*grad_y.shape[:-1], w.shape[1]) if ctx.needs_input_grad[0] else None
        gw = g.t() @ x2 if ctx.needs_input_grad[1] else None
        return gx, gw, gb, None, None


def linear(x, weight, bias=None, alpha=1.0, relu=False):
    """nn.Linear (+ optional scale and ReLU).  Object-query-sized inputs on the GPU (rows <= SKINNY_MAX_ROWS,
    K % 64 == 0, fp32) run the hand-written skinny MFMA kernel (forward and backward); token-sized inputs (encoder,
    S ~ 12.5k rows per image) run the split-bf16 GEMM kernels -- in inference through ``module_linear`` /
    ``linear_split_bf16``, under autograd through ``TokenLinearFunction`` -- and the vendor GEMM where those do not apply
    (feature counts that are not multiples of 128 / 32, bf16 models).  (On CPU tensors -- host-logic tests -- F.linear.)"""
    rows = x.numel() // x.shape[-1]
    if x.is_cuda and x.dtype == torch.float32 and rows <= SKINNY_MAX_ROWS and x.shape[-1] % 64 == 0:
        return SkinnyLinearFunction.apply(x, weight, bias, alpha, relu)
    if (LINEAR_BF16 and x.is_cuda and x.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16
            and rows <= LINEAR_BF16_MAX_ROWS and x.shape[-1] % 16 == 0 and weight.shape[0] % 32 == 0
            and (bias is None or bias.dtype == torch.bfloat16)
            and not (torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad))):
        return linear_bf16(x, weight, bias, relu, alpha)
    if (relu and alpha == 1.0 and bias is not None and x.is_cuda and not torch.is_grad_enabled()
            and hasattr(torch, "_addmm_activation")):
        # token-sized GEMM with the ReLU in the hipBLASLt epilogue (saves one pass over the [S, 1024] activation)
        y = torch._addmm_activation(bias, x.reshape(-1, x.shape[-1]), weight.t(), use_gelu=False)
        return y.view(*x.shape[:-1], weight.shape[0])
    if (alpha == 1.0 and bias is not None and x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32
            and rows > SKINNY_MAX_ROWS and torch.is_grad_enabled() and TOKEN_LINEAR
            and (x.requires_grad or weight.requires_grad or bias.requires_grad)):
        return TokenLinearFunction.apply(x, weight, bias, relu)   # training, token-sized: bias gradient in one HIP pass
    y = torch.nn.functional.linear(x, weight, bias)
    if alpha != 1.0:
        y = y * alpha
    return torch.relu(y) if relu else y


# bf16 models: the encoder layer's feed-forward block + residual + LayerNorm (+ position rows) in one launch
# (csrc/ffn_bf16.hip).  "0": two vendor GEMMs + the LayerNorm launch.
FFN_BF16_FUSED = True   # module attribute (tests patch it for the switch-off twin); no environment switch since round 6


def ffn_bf16_supported(x, fc1, fc2, ln):
    return (FFN_BF16_FUSED and x.is_cuda and x.dtype == torch.bfloat16 and not torch.is_grad_enabled() and x.shape[-1] == 256
            and all(t.dtype == torch.bfloat16 for t in (fc1.weight, fc2.weight, ln.weight))
            and fc1.bias is not None and fc2.bias is not None and tuple(fc1.weight.shape)[1] == 256
            and tuple(fc2.weight.shape) == (256, fc1.weight.shape[0]) and fc1.weight.shape[0] % 32 == 0
            and fc1.weight.shape[0] <= 1024 and tuple(ln.weight.shape) == (256,))


# bf16 models, object-query-sized rows (the decoder of the stress configuration: 4800 rows): csrc/linear_bf16.hip instead of the
# vendor library, whose choice for these shapes takes 20 us per layer.  "0": F.linear.
LINEAR_BF16 = True   # module attribute (tests patch it for the switch-off twin); no environment switch since round 6
LINEAR_BF16_MAX_ROWS = 16384


class TokenLinearFunction(Function):
    """nn.Linear (+ ReLU) on token-sized inputs in TRAINING (reference: the encoder / cross-attention nn.Linear layers,
    model/deformable_detr.py:1049, 1053-1058, 1102, 1337-1343, under autograd).  Forward and data gradient g W run on the
    bf16 matrix cores through the exact three-way split (csrc/gemm_split.hip; W and W^T are re-tiled by one launch each,
    egtr_gemm_split_tile_weights_f32) where the shape allows (out features % 128, reduction % 32), else on the vendor
    GEMM; the weight gradient x^T g is the vendor GEMM autograd would call; the bias gradient -- a [rows, N] column sum
    per layer, with the ReLU mask applied on the way -- is egtr_column_sum_f32 (one pass instead of threshold_backward +
    a generic reduction).  EGTR_TOKEN_LINEAR=0 keeps plain autograd; EGTR_GEMM_SPLIT_BF16=0 keeps the vendor GEMMs."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu):
        x2 = x.reshape(-1, x.shape[-1])
        N, K = weight.shape
        ctx.split = GEMM_SPLIT_BF16 and x2.shape[0] >= GEMM_SPLIT_MIN_ROWS and weight.stride(1) == 1
        ctx.wt_t = None
        ctx.terms = terms = _gemm_terms()   # read once: the backward multiplies the way the forward did
        if ctx.split and N % 128 == 0 and K % 128 == 0 and ctx.needs_input_grad[0]:
            wt, ctx.wt_t = gemm_split_tile_pair(weight, terms=terms)   # W^T for the data gradient, same launch
            y = linear_split_bf16(x2, wt, bias, N, relu=relu, terms=terms)
        elif ctx.split and N % 128 == 0 and K % 32 == 0:
            y = linear_split_bf16(x2, gemm_split_tile(weight, terms=terms), bias, N, relu=relu, terms=terms)
        elif relu and hasattr(torch, "_addmm_activation"):
            y = torch._addmm_activation(bias, x2, weight.t(), use_gelu=False)
        else:
            y = torch.addmm(bias, x2, weight.t())
            if relu:
                y = torch.relu_(y)
        ctx.relu = bool(relu)
        ctx.save_for_backward(x2, weight, y if relu else None)
        ctx.in_shape = x.shape
        return y.view(*x.shape[:-1], weight.shape[0])

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        x2, weight, y = ctx.saved_tensors
        N = weight.shape[0]
        g = grad_y.reshape(-1, N)
        g = _chk(g if g.is_contiguous() else g.contiguous(), "grad", torch.float32)
        if ctx.relu:
            g, gb = column_sum(g, relu_output=y)
        else:
            gb = column_sum(g)
        gx = None
        if ctx.needs_input_grad[0]:
            K = weight.shape[1]
            if ctx.split and K % 128 == 0 and N % 32 == 0:   # g W = "linear" with W^T
                wt_t = ctx.wt_t if ctx.wt_t is not None else gemm_split_tile(weight, transposed=True, terms=ctx.terms)
                gx = linear_split_bf16(g, wt_t, None, K, terms=ctx.terms)
            else:
                gx = g.mm(weight)
            gx = gx.view(ctx.in_shape)
        gw = None
        if ctx.needs_input_grad[1]:
            K = weight.shape[1]
            if ctx.split and GEMM_SPLIT_WGRAD and N % 128 == 0 and K % 128 == 0 and x2.stride(1) == 1:
                gw = linear_split_bf16_wgrad(g, x2, terms=ctx.terms)
            else:
                # the product autograd forms for addmm (x^T g, viewed transposed): the same vendor kernel as the plain path
                gw = x2.t().mm(g).t()
        return gx, gw, gb if ctx.needs_input_grad[2] else None, None


# ---- training form of the encoder layer (round 4): ONE autograd Function per layer -------------------------------------------
# "0": the per-op composition of rounds 2 / 3 (TokenLinearFunction + F.dropout + AddLayerNormFunction + clamp_nonfinite_ ...)
ENCODER_TRAIN_FUSED = os.environ.get("EGTR_ENCODER_TRAIN_FUSED", "1") != "0"
# training forward of the relation head on the split-bf16 arithmetic (rel_head_fwd_x6 with the activation stores); 0: exact-f32 kernel
REL_HEAD_TRAIN_X6 = True   # module attribute (tests patch it for the switch-off twin); no environment switch since round 6


def _rows256(t):
    t2 = t.reshape(-1, t.shape[-1])
    if t2.stride(1) != 1 or t2.stride(0) != t2.shape[1] or t2.data_ptr() % 16:
        t2 = t2.contiguous()
        if t2.data_ptr() % 16:
            t2 = t2.clone()
    return t2


def _keep_bytes(keep_rows):
    """[..] bool / integer row mask (non-zero = valid token) -> the flat uint8 ``row_keep`` operand of the split GEMMs; None stays None."""
    if keep_rows is None:
        return None
    rk = keep_rows.reshape(-1).contiguous()
    return rk.view(torch.uint8) if rk.dtype == torch.bool else rk.to(torch.uint8)


class EncoderLayerTrainFunction(Function):
    """One Deformable-DETR encoder layer in TRAINING as a single autograd node (reference: DeformableDetrEncoderLayer.forward
    in train mode, model/deformable_detr.py:1283-1358, with DeformableDetrMultiscaleDeformableAttention.forward, :1026-1104):

        value = mask(value_proj(x));  [offsets | logits] = Linear_cat(x + pos)  (pos added while the GEMM loads its operand)
        (loc, attn) = softmax / sampling locations;  ctx = MSDA(value, loc, attn)
        y1 = LayerNorm1(x + dropout(output_proj(ctx)));  y2 = LayerNorm2(y1 + dropout(fc2(relu(fc1(y1)))))
        y2 = clamp(y2) iff y2 holds an inf / nan (flag on the device, no host synchronisation)

    Why one node: the per-op composition of rounds 2 / 3 spent, per layer and step, ~25 ATen launches on glue around the
    same kernels -- gradient accumulation adds where branches meet, dropout forward / backward passes, `x + pos`, masked_fill and
    its backward, isfinite / clamp passes, threshold_backward + bias-gradient column sums over the [rows, 1024] activation
    (profiles/r04_train_gaps.txt: 5.5 ms of ATen elementwise kernels per step).  Here those are epilogue options of the split-bf16
    GEMMs (egtr_linear_split_bf16_ex_f32: row mask, ReLU backward, branch accumulation, bias-gradient partials) and of the two
    dropout + residual + LayerNorm kernels (csrc/enc_train.hip).  Dropout masks are bytes drawn by one bernoulli_ per layer
    (``masks`` hands in fixed ones for tests).  Arithmetic per product: exactly TokenLinearFunction's (six-term bf16 split)."""

    @staticmethod
    def forward(ctx, x, pos, ref, keep_rows, shapes, lsi, p_drop, masks, ln_eps, so_w, so_b, aw_w, aw_b, vp_w, vp_b, op_w,
                op_b, ln1_w, ln1_b, fc1_w, fc1_b, fc2_w, fc2_b, ln2_w, ln2_b):
        B, S, D = x.shape
        M = B * S
        dev = x.device
        x2 = _rows256(x.detach())
        pos2 = _rows256(pos.detach())
        rk = _keep_bytes(keep_rows)
        bb = torch.cat([so_b.detach(), aw_b.detach()], 0)
        ctx.terms = terms = _gemm_terms()   # read once: the tiled weights saved for the backward are of this kind only
        # every weight of the layer (and its transpose, for the data gradients) into the GEMM's operand stream: one launch;
        # sampling_offsets | attention_weights as ONE [384, 256] weight without a materialised concatenation
        (wt_v, wtT_v), (wt_b, wtT_b), (wt_o, wtT_o), (wt_1, wtT_1), (wt_2, wtT_2) = gemm_split_tile_pairs(
            [vp_w, (so_w, aw_w), op_w, fc1_w, fc2_w], terms=terms)
        F1 = fc1_w.shape[0]
        nb = so_w.shape[0] + aw_w.shape[0]
        n_off = so_w.shape[0]
        # value projection (padded rows zeroed in the epilogue) + offsets / logits projection of x + pos: one launch
        value, both = linear_split_ex([dict(x=x2, wt=wt_v, N=D, b=vp_b.detach(), row_keep=rk),
                                       dict(x=x2, wt=wt_b, N=nb, b=bb, pos=pos2)], M, D, terms=terms)
        Mh, L, P_ = 8, shapes.shape[0], n_off // (8 * shapes.shape[0] * 2)
        refc = _chk(ref.detach().contiguous(), "reference_points", torch.float32)
        shp = _chk(shapes.contiguous(), "spatial_shapes", torch.int64)
        loc = torch.empty(B, S, Mh, L, P_, 2, dtype=torch.float32, device=dev)
        attn = torch.empty(B, S, Mh, L, P_, dtype=torch.float32, device=dev)
        off, lg = both[:, :n_off], both[:, n_off:]
        _lib.launch("egtr_msda_geometry_forward_f32", off.data_ptr(), off.stride(0), lg.data_ptr(), lg.stride(0),
                    refc.data_ptr(), refc.shape[-1], shp.data_ptr(), loc.data_ptr(), attn.data_ptr(), M, Mh, L, P_)
        value4 = value.view(B, S, Mh, D // Mh)
        att = _msda().ms_deform_attn_forward(value4, shp, lsi, loc, attn, 64).view(M, D)
        a = linear_split_ex([dict(x=att, wt=wt_o, N=D, b=op_b.detach())], M, D, terms=terms)[0]
        p = float(p_drop)
        scale = 1.0 / (1.0 - p) if p > 0.0 else 1.0
        m1 = m2 = None
        if masks is not None:
            m1, m2 = masks
        elif p > 0.0:
            mm = torch.empty(2, M, D, dtype=torch.uint8, device=dev).bernoulli_(1.0 - p)
            m1, m2 = mm[0], mm[1]
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        eps1, eps2 = float(ln_eps[0]), float(ln_eps[1])
        y1 = dropout_add_layernorm(a, x2, m1, scale, ln1_w.detach(), ln1_b.detach(), eps1)
        h = linear_split_ex([dict(x=y1, wt=wt_1, N=F1, b=fc1_b.detach(), relu=True)], M, D, terms=terms)[0]
        f = linear_split_ex([dict(x=h, wt=wt_2, N=D, b=fc2_b.detach())], M, F1, terms=terms)[0]
        y2 = dropout_add_layernorm(f, y1, m2, scale, ln2_w.detach(), ln2_b.detach(), eps2, flag=flag)
        cv = torch.finfo(torch.float32).max - 1000
        _lib.launch("egtr_clamp_if_flag_f32", y2.data_ptr(), None, y2.numel(), flag.data_ptr(), cv, 0)
        ctx.save_for_backward(x2, pos2, refc, shp, lsi, rk, value, both, loc, attn, att, a, m1, y1, h, f, m2, y2, flag,
                              wtT_v, wtT_b, wtT_o, wtT_1, wtT_2, ln1_w, ln2_w)
        ctx.dims = (B, S, D, F1, nb, n_off, Mh, L, P_, scale, cv, eps1, eps2)
        ctx.in_shape = x.shape
        ctx.pos_shape = pos.shape
        return y2.view(B, S, D)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_y2):
        (x2, pos2, refc, shp, lsi, rk, value, both, loc, attn, att, a, m1, y1, h, f, m2, y2, flag,
         wtT_v, wtT_b, wtT_o, wtT_1, wtT_2, ln1_w, ln2_w) = ctx.saved_tensors
        B, S, D, F1, nb, n_off, Mh, L, P_, scale, cv, eps1, eps2 = ctx.dims
        M = B * S
        dev = x2.device
        terms = ctx.terms
        g = _rows256(g_y2)
        # LayerNorm2 + dropout backward (+ the clamp's gradient mask when the forward raised its flag)
        gs2, gf, gbb2 = dropout_add_layernorm_backward(f, y1, m2, scale, ln2_w.detach(), eps2, g, flag, y2, cv)
        d_w2 = linear_split_bf16_wgrad(gf, h, terms=terms)
        colp = torch.empty((M + 31) // 32, F1, dtype=torch.float32, device=dev)
        g_h = linear_split_ex([dict(x=gf, wt=wtT_2, N=F1, relu_ref=h, colpart=colp)], M, D, terms=terms)[0]   # ReLU mask + bias partials
        d_b1 = column_sum(colp)
        d_w1 = linear_split_bf16_wgrad(g_h, y1, terms=terms)
        linear_split_ex([dict(x=g_h, wt=wtT_1, N=D, add1=gs2, out=gs2)], M, F1, terms=terms)   # gs2 <- d loss / d y1
        del g_h
        gs1, ga, gbb1 = dropout_add_layernorm_backward(a, x2, m1, scale, ln1_w.detach(), eps1, gs2)
        d_wo = linear_split_bf16_wgrad(ga, att, terms=terms)
        g_att = linear_split_ex([dict(x=ga, wt=wtT_o, N=D)], M, D, terms=terms)[0]
        g_value, g_loc, g_attn = _msda().ms_deform_attn_backward(value.view(B, S, Mh, D // Mh), shp, lsi, loc, attn,
                                                                 g_att.view(B, S, D), 64)
        g_both = torch.empty(M, nb, dtype=torch.float32, device=dev)
        off = both[:, :n_off]
        _lib.launch("egtr_msda_geometry_backward_f32", g_loc.data_ptr(), g_attn.data_ptr(), attn.data_ptr(), off.data_ptr(),
                    off.stride(0), refc.data_ptr(), refc.shape[-1], shp.data_ptr(), g_both.data_ptr(), nb,
                    g_both.data_ptr() + 4 * n_off, nb, None, M, Mh, L, P_)
        d_bb = column_sum(g_both)
        d_wb = _wgrad_ex(g_both, x2, x_pos=pos2, terms=terms)
        g_qin = linear_split_ex([dict(x=g_both, wt=wtT_b, N=D)], M, nb, terms=terms)[0]   # = d loss / d pos as well
        gv2 = g_value.view(M, D)
        d_bv = column_sum(gv2) if rk is None else weighted_column_sum(gv2, rk.to(torch.float32))
        d_wv = _wgrad_ex(gv2, x2, row_keep=rk, terms=terms)
        linear_split_ex([dict(x=gv2, wt=wtT_v, N=D, row_keep=rk, add1=gs1, add2=g_qin, out=gs1)], M, D, terms=terms)   # gs1 <- d loss / d x
        g_pos = g_qin.view(B, S, D)
        if tuple(ctx.pos_shape) != (B, S, D):
            g_pos = g_pos.sum_to_size(ctx.pos_shape)
        return (gs1.view(ctx.in_shape), g_pos, None, None, None, None, None, None, None,
                d_wb[:n_off], d_bb[:n_off], d_wb[n_off:], d_bb[n_off:], d_wv, d_bv, d_wo, gbb1[512:768],
                gbb1[0:256], gbb1[256:512], d_w1, d_b1, d_w2, gbb2[512:768], gbb2[0:256], gbb2[256:512])


class DecoderValueProjTrainFunction(Function):
    """The cross-attention value projections of ALL decoder layers in training as one autograd node (reference: value_proj +
    masked_fill of every DeformableDetrMultiscaleDeformableAttention of the decoder, model/deformable_detr.py:1048-1052):
    values_l = mask(enc W_l^T + b_l), l = 0 .. Ld - 1.  Forward: ONE grouped launch of the split-bf16 GEMM (the Ld products
    share the operand rows and the grid; padded rows zeroed in the epilogue).  Backward: d enc = sum_l mask (g_l W_l) as a
    chain of data-gradient products that accumulate into one buffer (no AccumulateGrad adds, no masked_fill backward), weight
    gradients with the row mask applied on load, bias gradients as mask-weighted column sums.  Returns Ld separate tensors
    (views of one stacked tensor would make autograd build a zero-filled [Ld, B, S, 256] gradient per layer)."""

    @staticmethod
    def forward(ctx, enc, keep_rows, *wb):
        nl = len(wb) // 2
        ws, bs = wb[:nl], wb[nl:]
        B, S, D = enc.shape
        M = B * S
        x2 = _rows256(enc.detach())
        rk = _keep_bytes(keep_rows)
        ctx.terms = terms = _gemm_terms()
        tiles = []
        for i0 in range(0, nl, 8):
            tiles += gemm_split_tile_pairs(list(ws[i0:i0 + 8]), terms=terms)
        outs = []
        for i0 in range(0, nl, 8):
            outs += linear_split_ex([dict(x=x2, wt=tiles[i][0], N=D, b=bs[i].detach(), row_keep=rk)
                                     for i in range(i0, min(nl, i0 + 8))], M, D, terms=terms)
        ctx.save_for_backward(x2, rk, *[t[1] for t in tiles])
        ctx.set_materialize_grads(False)   # an unused layer's values: None, not a zero tensor to multiply out
        ctx.nl = nl
        ctx.in_shape = enc.shape
        return tuple(o.view(B, S, D) for o in outs)

    @staticmethod
    @once_differentiable
    def backward(ctx, *gs):
        x2, rk = ctx.saved_tensors[:2]
        wtT = ctx.saved_tensors[2:]
        nl, terms = ctx.nl, ctx.terms
        M, D = x2.shape
        g_enc = None
        d_w, d_b = [], []
        rkf = rk.to(torch.float32) if rk is not None else None
        for i in range(nl):
            if gs[i] is None:
                d_w.append(None)
                d_b.append(None)
                continue
            g = _rows256(gs[i])
            d_b.append(column_sum(g) if rkf is None else weighted_column_sum(g, rkf))
            d_w.append(_wgrad_ex(g, x2, row_keep=rk, terms=terms))
            if g_enc is None:
                g_enc = linear_split_ex([dict(x=g, wt=wtT[i], N=D, row_keep=rk)], M, D, terms=terms)[0]
            else:
                linear_split_ex([dict(x=g, wt=wtT[i], N=D, row_keep=rk, add1=g_enc, out=g_enc)], M, D, terms=terms)
        return (g_enc.view(ctx.in_shape) if g_enc is not None else None, None, *d_w, *d_b)


def decoder_values_train_supported(enc, attention_mask, layers):
    eligible = (ENCODER_TRAIN_FUSED and GEMM_SPLIT_BF16 and torch.is_grad_enabled() and torch.is_tensor(enc) and enc.is_cuda
                and enc.dtype == torch.float32 and enc.dim() == 3 and enc.shape[0] * enc.shape[1] > SKINNY_MAX_ROWS)
    ok = (eligible and enc.shape[-1] == 256
          and all(tuple(l.encoder_attn.value_proj.weight.shape) == (256, 256) and l.encoder_attn.value_proj.bias is not None
                  and l.encoder_attn.value_proj.weight.dtype == torch.float32 for l in layers)
          and (attention_mask is None or tuple(attention_mask.shape) == tuple(enc.shape[:2])))
    return _gate("decoder_values_train", eligible, ok, lambda: f"encoder states {tuple(enc.shape)}: 256 channels, 256 -> 256 value "
                                                               "projections with biases served")


def decoder_values_train(enc, attention_mask, layers):
    """[value_proj_l(enc) with padded rows zeroed for l in layers] -- see DecoderValueProjTrainFunction."""
    return DecoderValueProjTrainFunction.apply(
        enc, attention_mask, *[l.encoder_attn.value_proj.weight for l in layers],
        *[l.encoder_attn.value_proj.bias for l in layers])


class DropoutAddLayerNormFunction(Function):
    """LayerNorm(residual + dropout(x)) over 256 channels as one pass per direction (csrc/enc_train.hip) -- the decoder layer's
    three "dropout, add, LayerNorm" steps in training (model/deformable_detr.py:1436-1438, 1455-1457, 1466-1468): instead of
    fused_dropout + add_layernorm forward and layer-norm backward + masked_scale backward.  The mask is a byte tensor drawn by
    bernoulli_ (``keep`` hands in a fixed one for tests)."""

    @staticmethod
    def forward(ctx, x, residual, weight, bias, eps, p, keep):
        x2, r2 = _rows256(x.detach()), _rows256(residual.detach())
        scale = 1.0
        if keep is None and p > 0.0:
            keep = torch.empty(x2.shape, dtype=torch.uint8, device=x2.device).bernoulli_(1.0 - p)
        if keep is not None:
            scale = 1.0 / (1.0 - p)
        y = dropout_add_layernorm(x2, r2, keep, scale, weight.detach(), bias.detach(), eps)
        ctx.save_for_backward(x2, r2, keep, weight)
        ctx.cfg = (float(eps), float(scale))
        return y.view(x.shape)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x2, r2, keep, weight = ctx.saved_tensors
        eps, scale = ctx.cfg
        gs, gx, gbb = dropout_add_layernorm_backward(x2, r2, keep, scale, weight.detach(), eps, _rows256(gy))
        return gx.view(gy.shape), gs.view(gy.shape), gbb[0:256], gbb[256:512], None, None, None


def dropout_add_layer_norm(x, residual, ln, p, training, keep=None):
    """ln(residual + dropout(x, p, training)); fp32 device tensors of 256 channels under autograd take the one-pass kernels."""
    if (ENCODER_TRAIN_FUSED and training and torch.is_grad_enabled() and x.is_cuda and x.dtype == torch.float32
            and x.shape[-1] == 256 and residual.shape == x.shape and 0.0 <= p < 1.0):
        return DropoutAddLayerNormFunction.apply(x, residual, ln.weight, ln.bias, ln.eps, float(p), keep)
    return add_layer_norm(torch.nn.functional.dropout(x, p=p, training=training), residual, ln)


def encoder_layer_train_supported(layer, x, pos, ref, attention_mask, output_attentions):
    """The fused training node serves the reference's training configuration: fp32 on the GPU, token-sized rows, d_model 256,
    8 heads x 4 levels x 4 points, 2-d reference points, ReLU FFN with a hidden width that tiles (multiple of 128),
    activation_dropout 0 (the reference default), no attention maps requested."""
    sa = layer.self_attn
    eligible = (ENCODER_TRAIN_FUSED and GEMM_SPLIT_BF16 and torch.is_grad_enabled() and layer.training and not output_attentions
                and torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 3
                and x.shape[0] * x.shape[1] > SKINNY_MAX_ROWS)
    ok = (eligible and x.shape[-1] == 256 and pos is not None and pos.dtype == torch.float32
          and tuple(pos.shape) == tuple(x.shape) and ref is not None and ref.dim() == 4 and ref.shape[-1] == 2
          and sa.n_heads == 8 and sa.n_levels == 4 and sa.n_points == 4 and ref.shape[2] == 4
          and layer.activation_fn is torch.nn.functional.relu and layer.activation_dropout == 0.0
          and layer.fc1.weight.shape[0] % 128 == 0 and tuple(layer.fc2.weight.shape) == (256, layer.fc1.weight.shape[0])
          and layer.fc1.weight.dtype == torch.float32 and 0.0 <= layer.dropout < 1.0
          and (attention_mask is None or tuple(attention_mask.shape) == tuple(x.shape[:2])))
    return _gate("encoder_layer_train", eligible, ok,
                 lambda: f"states {tuple(x.shape)}, {sa.n_heads} heads x {sa.n_levels} levels x {sa.n_points} points, fc1 "
                         f"{tuple(layer.fc1.weight.shape)}: the training node serves d_model 256, 8 x 4 x 4, ReLU, a hidden width "
                         "that is a multiple of 128, activation_dropout 0, 2-d reference points")


def encoder_layer_train(layer, x, attention_mask, pos, ref, spatial_shapes, level_start_index, masks=None):
    sa = layer.self_attn
    return EncoderLayerTrainFunction.apply(
        x, pos, ref, attention_mask, spatial_shapes, level_start_index, layer.dropout, masks,
        (layer.self_attn_layer_norm.eps, layer.final_layer_norm.eps), sa.sampling_offsets.weight, sa.sampling_offsets.bias, sa.attention_weights.weight, sa.attention_weights.bias,
        sa.value_proj.weight, sa.value_proj.bias, sa.output_proj.weight, sa.output_proj.bias,
        layer.self_attn_layer_norm.weight, layer.self_attn_layer_norm.bias, layer.fc1.weight, layer.fc1.bias,
        layer.fc2.weight, layer.fc2.bias, layer.final_layer_norm.weight, layer.final_layer_norm.bias)


# ---- decoder layer as ONE autograd node (training) ---------------------------------------------------------------------------
DECODER_TRAIN_FUSED = True   # module attribute, not an environment switch: tests patch it for the switch-off twin


class DecoderLayerTrainFunction(Function):
    """One Deformable-DETR decoder layer in TRAINING as a single autograd node (reference:
    DeformableDetrDecoderLayer.forward, model/deformable_detr.py:1390-1489; self-attention with the retained scaled-q / k maps
    :1107-1262; cross-attention :1026-1104 on the value projection handed in by ``DecoderValueProjTrainFunction``):

        q = s (x + pos) Wq^T + s bq,  k = (x + pos) Wk^T + bk,  v = x Wv^T + bv;   a = out_proj(softmax(q k^T) v)
        y1 = LN1(x + drop(a));   [off | logits] of (y1 + pos);   c = output_proj(MSDA(value, loc, softmax(logits)))
        y2 = LN2(y1 + drop(c));  y3 = LN3(y2 + drop(fc2(relu(fc1(y2)))))            returns (y3, q, k)

    The per-operation composition ran the same kernels as ~14 autograd nodes per layer; what autograd added around them -- per
    layer and step, on [B N, 256] tensors of 0.8 MB -- were the gradient-accumulation adds where branches meet (x feeds q / k, v
    and the residual; y1 feeds the offset / logit projections and the residual; y2 feeds fc1 and the residual; q and k also feed
    the relation head through the retained maps), ``x + pos`` / ``y1 + pos`` and their backward, and contiguous copies of views:
    ~18 launches of ~4 us each per layer (profiles/r06_train_ops_by_shape_before.txt: 55 add + 24 add_ + 14 copy_ + 12 mul
    launches of that shape per step).  Here every meeting point is the epilogue of the product that arrives last
    (egtr_linear_backward_acc_f32: up to two addends on grad_x; egtr_self_attn_backward_acc_f32: the maps' gradients on grad_q /
    grad_k); three ATen adds per layer remain (x + pos, y1 + pos, the two pos gradients).  Arithmetic: exactly the kernels of the
    composition (exact-f32 MFMA), so values agree to rounding of the changed summation order at the meeting points."""

    @staticmethod
    def forward(ctx, x, pos, ref, value, shapes, lsi, p_drop, masks, eps3, scaling, wq, bq, wk, bk, wv, bv, wo, bo, ln1w, ln1b,
                wso, bso, waw, baw, wop, bop, ln2w, ln2b, w1, b1, w2, b2, ln3w, ln3b):
        B, N, D = x.shape
        M = B * N
        dev = x.device
        x2 = _rows256(x.detach())
        pos3 = pos.detach()          # [B, N, D], usually a stride-0 batch expansion of the query table: added as it is (no copy)
        heads = 8
        d = [t.detach() for t in (wq, bq, wk, bk, wv, bv, wo, bo, ln1w, ln1b, wso, bso, waw, baw, wop, bop, ln2w, ln2b, w1, b1,
                                  w2, b2, ln3w, ln3b)]
        (wq_, bq_, wk_, bk_, wv_, bv_, wo_, bo_, g1, be1, wso_, bso_, waw_, baw_, wop_, bop_, g2, be2, w1_, b1_, w2_, b2_, g3,
         be3) = [t if t.is_contiguous() else t.contiguous() for t in d]
        p = float(p_drop)
        scale = 1.0 / (1.0 - p) if p > 0.0 else 1.0
        if masks is not None:
            m1, m2, m3 = masks[0], masks[1], masks[2]
        elif p > 0.0:
            mm = torch.empty(3, M, D, dtype=torch.uint8, device=dev).bernoulli_(1.0 - p)
            m1, m2, m3 = mm[0], mm[1], mm[2]
        else:
            m1 = m2 = m3 = None
        e1, e2, e3 = (float(v) for v in eps3)
        # ---- self-attention
        xp = _rows256(x2.view(B, N, D) + pos3)
        q = _skinny_fwd(xp, wq_, bq_, alpha=scaling)
        k = _skinny_fwd(xp, wk_, bk_)
        v = _skinny_fwd(x2, wv_, bv_)
        sa = torch.empty(M, D, dtype=torch.float32, device=dev)
        lse = torch.empty(B, heads, N, dtype=torch.float32, device=dev)
        _lib.launch("egtr_self_attn_forward_f32", q.data_ptr(), k.data_ptr(), v.data_ptr(), B, N, heads, D // heads,
                    sa.data_ptr(), None, None, lse.data_ptr())
        a = _skinny_fwd(sa, wo_, bo_)
        y1 = dropout_add_layernorm(a, x2, m1, scale, g1, be1, e1)
        # ---- cross-attention (MSDA over the encoder's value projection)
        y1p = _rows256(y1.view(B, N, D) + pos3)
        off = _skinny_fwd(y1p, wso_, bso_)
        lg = _skinny_fwd(y1p, waw_, baw_)
        L = shapes.shape[0]
        P_ = wso_.shape[0] // (heads * L * 2)
        refc = _chk(ref.detach().contiguous(), "reference_points", torch.float32)
        shp = _chk(shapes.contiguous(), "spatial_shapes", torch.int64)
        loc = torch.empty(B, N, heads, L, P_, 2, dtype=torch.float32, device=dev)
        attn = torch.empty(B, N, heads, L, P_, dtype=torch.float32, device=dev)
        _lib.launch("egtr_msda_geometry_forward_f32", off.data_ptr(), off.stride(0), lg.data_ptr(), lg.stride(0),
                    refc.data_ptr(), refc.shape[-1], shp.data_ptr(), loc.data_ptr(), attn.data_ptr(), M, heads, L, P_)
        val = value.detach()
        S = val.shape[1]
        val4 = (val if val.is_contiguous() else val.contiguous()).view(B, S, heads, D // heads)
        ca = _msda().ms_deform_attn_forward(val4, shp, lsi, loc, attn, 64).view(M, D)
        c = _skinny_fwd(ca, wop_, bop_)
        y2 = dropout_add_layernorm(c, y1, m2, scale, g2, be2, e2)
        # ---- feed-forward block
        h = _skinny_fwd(y2, w1_, b1_, relu=True)
        f = _skinny_fwd(h, w2_, b2_)
        y3 = dropout_add_layernorm(f, y2, m3, scale, g3, be3, e3)
        ctx.save_for_backward(x2, xp, q, k, v, sa, lse, a, m1, y1, y1p, off, refc, shp, lsi, loc, attn, val4, ca, c, m2, y2, h,
                              f, m3, wq_, wk_, wv_, wo_, g1, wso_, waw_, wop_, g2, w1_, w2_, g3)
        ctx.dims = (B, N, D, heads, L, P_, scale, e1, e2, e3, float(scaling))
        ctx.pos_shape = tuple(pos.shape)
        ctx.value_shape = tuple(value.shape)
        ctx.ref_needs_grad = bool(ref.requires_grad)
        return y3.view(B, N, D), q.view(B, N, D), k.view(B, N, D)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_y3, g_q_ext, g_k_ext):
        (x2, xp, q, k, v, sa, lse, a, m1, y1, y1p, off, refc, shp, lsi, loc, attn, val4, ca, c, m2, y2, h, f, m3, wq_, wk_, wv_,
         wo_, g1, wso_, waw_, wop_, g2, w1_, w2_, g3) = ctx.saved_tensors
        B, N, D, heads, L, P_, scale, e1, e2, e3, scaling = ctx.dims
        M = B * N
        dev = x2.device
        g3y = _rows256(g_y3)
        # ---- feed-forward block: LN3 <- fc2 <- ReLU <- fc1, the residual's gradient joins in fc1's data gradient
        gs3, gf, gbb3 = dropout_add_layernorm_backward(f, y2, m3, scale, g3, e3, g3y)
        g_h, d_w2, _ = _skinny_bwd(gf, h, w2_, want_gb=False)
        g_y2, d_w1, d_b1 = _skinny_bwd(g_h, y2, w1_, relu_out=h, add1=gs3)
        # ---- cross-attention
        gs2, gc, gbb2 = dropout_add_layernorm_backward(c, y1, m2, scale, g2, e2, g_y2)
        g_ca, d_wop, _ = _skinny_bwd(gc, ca, wop_, want_gb=False)
        g_value, g_loc, g_attn = _msda().ms_deform_attn_backward(val4, shp, lsi, loc, attn, g_ca.view(B, N, D), 64)
        g_off = torch.empty(M, off.shape[1], dtype=torch.float32, device=dev)
        g_lg = torch.empty(M, attn.numel() // M, dtype=torch.float32, device=dev)
        g_ref = torch.empty_like(refc) if ctx.ref_needs_grad else None
        _lib.launch("egtr_msda_geometry_backward_f32", g_loc.data_ptr(), g_attn.data_ptr(), attn.data_ptr(), off.data_ptr(),
                    off.stride(0), refc.data_ptr(), refc.shape[-1], shp.data_ptr(), g_off.data_ptr(), g_off.shape[1],
                    g_lg.data_ptr(), g_lg.shape[1], _lib.ptr(g_ref), M, heads, L, P_)
        t_so, d_wso, d_bso = _skinny_bwd(g_off, y1p, wso_)
        g_y1p, d_waw, d_baw = _skinny_bwd(g_lg, y1p, waw_, add1=t_so, out=t_so)          # d loss / d (y1 + pos)
        g_y1 = gs2.add_(g_y1p)
        # ---- self-attention
        gs1, ga, gbb1 = dropout_add_layernorm_backward(a, x2, m1, scale, g1, e1, g_y1)
        g_sa, d_wo, _ = _skinny_bwd(ga, sa, wo_, want_gb=False)
        gq, gk, gv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        gqe = _rows256(g_q_ext) if g_q_ext is not None else None
        gke = _rows256(g_k_ext) if g_k_ext is not None else None
        _lib.launch("egtr_self_attn_backward_acc_f32", q.data_ptr(), k.data_ptr(), v.data_ptr(), sa.data_ptr(), lse.data_ptr(),
                    g_sa.data_ptr(), B, N, heads, D // heads, gq.data_ptr(), gk.data_ptr(), gv.data_ptr(), _lib.ptr(gqe),
                    _lib.ptr(gke))
        u_q, d_wq, d_bq = _skinny_bwd(gq, xp, wq_, alpha=scaling)
        g_xp, d_wk, d_bk = _skinny_bwd(gk, xp, wk_, add1=u_q, out=u_q)                  # d loss / d (x + pos)
        g_x, d_wv, d_bv = _skinny_bwd(gv, x2, wv_, add1=g_xp, add2=gs1, out=gs1)
        g_pos = (g_y1p + g_xp).view(B, N, D)
        if ctx.pos_shape != (B, N, D):
            g_pos = g_pos.sum_to_size(ctx.pos_shape)
        g_val = g_value.view(ctx.value_shape)
        return (g_x.view(B, N, D), g_pos, g_ref, g_val, None, None, None, None, None, None,
                d_wq, d_bq, d_wk, d_bk, d_wv, d_bv, d_wo, gbb1[512:768], gbb1[0:256], gbb1[256:512],
                d_wso, d_bso, d_waw, d_baw, d_wop, gbb2[512:768], gbb2[0:256], gbb2[256:512],
                d_w1, d_b1, d_w2, gbb3[512:768], gbb3[0:256], gbb3[256:512])


def decoder_layer_train_supported(layer, x, pos, ref, value, attention_mask, output_attentions):
    """The decoder-layer training node serves the reference's training configuration: fp32 on the GPU, object-query rows,
    d_model 256, 8 heads, 4 levels x 4 points, 2-d reference points (no box refinement), ReLU FFN, no attention maps / masks /
    attention dropout, a precomputed (already masked) value projection."""
    sa, ca = layer.self_attn, layer.encoder_attn
    eligible = (DECODER_TRAIN_FUSED and ENCODER_TRAIN_FUSED and SKINNY_BACKWARD_FUSED and torch.is_grad_enabled()
                and layer.training and not output_attentions and attention_mask is None and torch.is_tensor(x) and x.is_cuda
                and x.dtype == torch.float32 and x.dim() == 3 and x.shape[0] * x.shape[1] <= SKINNY_MAX_ROWS
                and torch.is_tensor(value))
    ok = (eligible and x.shape[-1] == 256 and pos is not None and pos.dtype == torch.float32 and pos.shape[-1] == 256
          and ref is not None and ref.dim() == 4 and ref.shape[-1] == 2 and ref.shape[2] == 4
          and value.dim() == 3 and value.shape[-1] == 256 and value.dtype == torch.float32
          and sa.num_heads == 8 and sa.embed_dim == 256 and sa.dropout == 0.0 and sa.q_proj.bias is not None
          and ca.n_heads == 8 and ca.n_levels == 4 and ca.n_points == 4 and ca.d_model == 256
          and layer.activation_fn is torch.nn.functional.relu and layer.activation_dropout == 0.0
          and layer.fc1.weight.shape[0] % 64 == 0 and tuple(layer.fc2.weight.shape) == (256, layer.fc1.weight.shape[0])
          and x.shape[1] <= 640 and 0.0 <= layer.dropout < 1.0)
    return _gate("decoder_layer_train", eligible, ok,
                 lambda: f"states {tuple(x.shape)}: the training node serves d_model 256, 8 heads, 4 x 4 sampling points, ReLU, "
                         "2-d reference points, <= 640 queries, no attention dropout")


def decoder_layer_train(layer, x, pos, ref, value, spatial_shapes, level_start_index, masks=None):
    """(y3, scaled q, k) of one decoder layer through DecoderLayerTrainFunction."""
    sa, ca = layer.self_attn, layer.encoder_attn
    return DecoderLayerTrainFunction.apply(
        x, pos, ref, value, spatial_shapes, level_start_index, layer.dropout, masks,
        (layer.self_attn_layer_norm.eps, layer.encoder_attn_layer_norm.eps, layer.final_layer_norm.eps), float(sa.scaling),
        sa.q_proj.weight, sa.q_proj.bias, sa.k_proj.weight, sa.k_proj.bias, sa.v_proj.weight, sa.v_proj.bias,
        sa.out_proj.weight, sa.out_proj.bias, layer.self_attn_layer_norm.weight, layer.self_attn_layer_norm.bias,
        ca.sampling_offsets.weight, ca.sampling_offsets.bias, ca.attention_weights.weight, ca.attention_weights.bias,
        ca.output_proj.weight, ca.output_proj.bias, layer.encoder_attn_layer_norm.weight, layer.encoder_attn_layer_norm.bias,
        layer.fc1.weight, layer.fc1.bias, layer.fc2.weight, layer.fc2.bias, layer.final_layer_norm.weight,
        layer.final_layer_norm.bias)


# ---- the environment switches of the package (round 6: seven route switches, down from twenty-four) ----------------------------
# Each selects between two SHIPPED routes that both have a use; everything else that used to be switchable from the environment
# is either gone (the decoder's tagged hand-over, the double-buffered split GEMM: measured slower) or a plain module attribute
# that only the switch-off twin tests patch (the route it turns off is the generic composition that CPU tensors and unsupported
# shapes take anyway).  tests/test_gpu_model.py::test_full_size_with_every_kept_switch_off_at_once_vs_reference runs the
# combination of all of them.
#   EGTR_DECODER_CLUSTER=0      decoder_fused.ENABLED       decoder layer: one launch per layer  ->  per-operation launches
#   EGTR_GEMM_SPLIT_BF16=0      ops.GEMM_SPLIT_BF16         token-sized linears: split-bf16 matrix cores  ->  vendor fp32 GEMM; also the
#                                                           fp32 backbone's own split-bf16 kernels (stem, 3x3 convolutions, bottleneck
#                                                           tails: backbone.STEM_FUSED / CONV2_X6 / CONV3_FUSED / CONV1_X6)  ->  MIOpen /
#                                                           vendor GEMM + passes; and the grouped input projections
#                                                           (input_proj_x6_groupnorm)  ->  vendor GEMMs + MIOpen
#   EGTR_REL_HEAD_SPLIT_BF16=0  ops.REL_HEAD_SPLIT_BF16     relation head at inference: split-bf16  ->  exact-f32 MFMA kernel
#   EGTR_FFN_FUSED=0            ops.FFN_FUSED               encoder FFN / layer tail row-panel kernels  ->  separate launches
#   EGTR_BACKBONE_NHWC=0        backbone.NHWC_F32 / _BF16   inference backbone channels-last  ->  NCHW
#   EGTR_ENCODER_TRAIN_FUSED=0  ops.ENCODER_TRAIN_FUSED     training nodes (encoder / decoder layer, values, LayerNorm)  ->  per-op autograd
#   EGTR_TOKEN_LINEAR=0         ops.TOKEN_LINEAR            token-sized linears under autograd: TokenLinearFunction  ->  F.linear
#   EGTR_DETERMINISTIC=1        ops.DETERMINISTIC           (opt-IN) training: fp32 atomics / first-come tie tickets  ->  the order-free
#                                                           routes (fixed-point MSDA grad_value, indexed loss ties, gate means
#                                                           reduced in a fixed order); see set_deterministic() below
#   EGTR_MATMUL_PRECISION=bf16  ops.MATMUL_PRECISION        (opt-IN) training token GEMMs: six-term split-bf16, fp32 to the last bit  ->
#                                                           ONE product per element, operands rounded once to bf16 (nearest even),
#                                                           fp32 accumulation; see set_matmul_precision() below
#   (module attribute only)     ops.RELATION_LOSS_ALL       un-sampled relation loss (evaluation mode; both rel_sample_* None): one HIP
#                                                           pipeline over all elements  ->  the criterion's per-image tensor composition
# Not route switches: EGTR_HIP_LIBRARY (another build of the library), EGTR_STRICT_FAST_PATH (below), EGTR_TRUST_CHECKPOINT_PICKLE.
ENV_ROUTE_SWITCHES = ("EGTR_DECODER_CLUSTER", "EGTR_GEMM_SPLIT_BF16", "EGTR_REL_HEAD_SPLIT_BF16", "EGTR_FFN_FUSED",
                      "EGTR_BACKBONE_NHWC", "EGTR_ENCODER_TRAIN_FUSED", "EGTR_TOKEN_LINEAR", "EGTR_DETERMINISTIC",
                      "EGTR_MATMUL_PRECISION")

# ---- deterministic mode ------------------------------------------------------------------------------
# Opt-in: the same inputs on the same device with the same build give the same bits from the library's own kernels and this
# package's autograd Functions.  Three places on the training path depend on the order in which the hardware serves atomics; under
# the mode each takes an order-free route, consulted AT CALL TIME (a route switch, not a fall-off: nothing is counted in FALLBACKS):
#   MSDA backward, grad_value   fp32 atomics  ->  64-bit fixed point with integer atomics (egtr_msda_backward_det_*); float64 raises
#   relation loss, tied logits  tickets       ->  lowest flat index first (egtr_relation_loss_f32, deterministic = 1)
#   rel_gate_{t} logging        fp32 atomics  ->  a torch reduction (fixed order); the model output never depended on it
# Not covered: vendor kernels (MIOpen convolutions, rocBLAS GEMMs), ATen operations without a deterministic form, equality
# across batch sizes / devices / builds, or between this route and the default one.  torch's own global switch
# (torch.use_deterministic_algorithms) is honoured and never set from here.
DETERMINISTIC = os.environ.get("EGTR_DETERMINISTIC", "0") == "1"


def set_deterministic(flag):
    """Turn the library's deterministic routes on or off (process-wide; returns the previous setting)."""
    global DETERMINISTIC
    prev = DETERMINISTIC
    DETERMINISTIC = bool(flag)
    return prev


def is_deterministic():
    """True when the order-free routes are taken: ``ops.DETERMINISTIC`` or torch's global deterministic-algorithms switch."""
    return bool(DETERMINISTIC) or torch.are_deterministic_algorithms_enabled()


class deterministic:
    """``with ops.deterministic():`` -- the mode for a block (``flag=False``: off for a block); restores the previous setting."""

    def __init__(self, flag=True):
        self.flag = bool(flag)

    def __enter__(self):
        self.prev = set_deterministic(self.flag)
        return self

    def __exit__(self, *exc):
        set_deterministic(self.prev)
        return False


# ---- matmul precision of the training token GEMMs ----------------------------------------------------------
# Opt-in, the counterpart of torch.set_float32_matmul_precision("medium") / Lightning's precision="bf16" for this package's own
# kernels: under "bf16" the token-sized products of the autograd training routes -- TokenLinearFunction (forward, data gradient,
# weight gradient), every product of EncoderLayerTrainFunction and DecoderValueProjTrainFunction -- round each operand ONCE to
# bf16 (round to nearest even; `x + pos` is added in fp32 first) and issue one matrix instruction per k-step instead of six
# (csrc/gemm_split.hip, `terms` = 1 of its entries).  Accumulation, the tensors in memory, master weights, gradients and the
# optimizer stay fp32; bf16 has fp32's exponent range, so there is no loss scaling.  Consulted AT CALL TIME in a Function's
# forward and kept on its ctx for the backward (a route switch, not a fall-off: nothing is counted in FALLBACKS).
# RelationHeadFunction is covered where its split-bf16 training forward runs (4 or 7 slots, num_rel <= 64, hidden 256): layer 2
# of both MLPs (W2 h1) and layer 3 of the relation MLP (W3 h2) round their operands in the one-term form of rel_head_fwd_x6, and
# in the backward dh1 = dh2 W2 (with its ReLU mask and the b1 column sums: one `ex` launch per MLP) and dW2 = dh2^T h1 do.  NOT
# rounded there: layer 1, the connectivity output layer w3c h2, the layer-3 gradients G W3 and G^T h2 (K or N = num_rel); the
# saved h1 / h2 stay fp32.  Any other relation-head call keeps the exact-f32 kernel and backward under either mode.
# Not covered: every inference route (module_linear, ffn_fused, the grouped projections, the relation head, the backbone) keeps
# its bits -- a user who wants bf16 inference has the bf16 model; MSDA, LayerNorm, the losses and the matcher; shapes the split
# kernels do not serve still take the vendor GEMM in fp32.  torch's own float32_matmul_precision is neither read nor set.
_MATMUL_PRECISIONS = ("fp32", "bf16")


def _checked_matmul_precision(p):
    if p not in _MATMUL_PRECISIONS:
        raise ValueError(f"matmul precision must be one of {_MATMUL_PRECISIONS}, got {p!r}")
    return p


MATMUL_PRECISION = _checked_matmul_precision(os.environ.get("EGTR_MATMUL_PRECISION", "fp32"))


def set_matmul_precision(p):
    """"fp32" (the six-term split-bf16 products) or "bf16" (operands rounded once) for the training token GEMMs; process-wide,
    returns the previous setting."""
    global MATMUL_PRECISION
    prev = MATMUL_PRECISION
    MATMUL_PRECISION = _checked_matmul_precision(p)
    return prev


def matmul_precision():
    """The current setting: "fp32" or "bf16"."""
    return MATMUL_PRECISION


class matmul_precision_mode:
    """``with ops.matmul_precision_mode("bf16"):`` -- the setting for a block; restores the previous one, on an exception too."""

    def __init__(self, p):
        self.p = _checked_matmul_precision(p)

    def __enter__(self):
        self.prev = set_matmul_precision(self.p)
        return self

    def __exit__(self, *exc):
        set_matmul_precision(self.prev)
        return False


# ---- relation sampler: who draws a RANDOM candidate class of the relation loss ------------------------------
# The criterion's `rel_sample_*_largest=False` ablation takes a uniform random subset of a candidate class instead of its largest
# logits.  "python" (the default): the reference's composition -- nonzero() index lists and `random.sample` on the host; Python's
# `random` stream is consumed exactly as the reference consumes it.  "device" (opt-in): the subset is the k candidates with the
# largest keyed hash of their flat index (egtr_relation_loss_f32, policy 1): no host wait, and a function of (seed, stream) alone --
# the same distribution, other bits, and Python's `random` stream is left alone.  Every launch with a random class uses the
# current `stream` and advances it by one, so auxiliary output sets and successive steps draw independently; (seed, stream) is
# the whole state (relation_sampler_state / set_relation_sampler_state: checkpoint and resume).  No environment switch.
_RELATION_SAMPLERS = ("python", "device")
RELATION_SAMPLER = "python"
_RELATION_SAMPLER_SEED = None     # None: torch.initial_seed(), read when the first key is needed
_RELATION_SAMPLER_STREAM = 0


def _checked_relation_sampler(name):
    if name not in _RELATION_SAMPLERS:
        raise ValueError(f"relation sampler must be one of {_RELATION_SAMPLERS}, got {name!r}")
    return name


def set_relation_sampler(name, seed=None):
    """"python" (random.sample on the host, the reference's draws) or "device" (the keyed selection of the policy kernels) for a
    random candidate class of the relation loss; process-wide, returns the previous setting.  ``seed`` (any int) also restarts
    the stream at 0; ``seed=None`` keeps the current seed and stream (initially ``torch.initial_seed()``, stream 0)."""
    global RELATION_SAMPLER, _RELATION_SAMPLER_SEED, _RELATION_SAMPLER_STREAM
    prev = RELATION_SAMPLER
    RELATION_SAMPLER = _checked_relation_sampler(name)
    if seed is not None:
        _RELATION_SAMPLER_SEED, _RELATION_SAMPLER_STREAM = int(seed), 0
    return prev


def relation_sampler():
    """The current setting: "python" or "device"."""
    return RELATION_SAMPLER


def relation_sampler_state():
    """(seed, stream) of the device sampler: what the NEXT launch with a random class uses."""
    global _RELATION_SAMPLER_SEED
    if _RELATION_SAMPLER_SEED is None:
        _RELATION_SAMPLER_SEED = int(torch.initial_seed())
    return _RELATION_SAMPLER_SEED, _RELATION_SAMPLER_STREAM


def set_relation_sampler_state(seed, stream):
    """Resume: the next launch with a random class uses (seed, stream)."""
    global _RELATION_SAMPLER_SEED, _RELATION_SAMPLER_STREAM
    _RELATION_SAMPLER_SEED, _RELATION_SAMPLER_STREAM = int(seed), int(stream)


def _next_relation_stream():
    """(seed, stream) for one launch with a random class; the stream advances by one."""
    global _RELATION_SAMPLER_STREAM
    seed, stream = relation_sampler_state()
    _RELATION_SAMPLER_STREAM = stream + 1
    return seed, stream


class relation_sampler_mode:
    """``with ops.relation_sampler_mode("device", seed=5):`` -- the sampler for a block; restores the previous NAME on exit, on
    an exception too (the stream keeps counting: draws inside the block are not repeated after it)."""

    def __init__(self, name, seed=None):
        self.name, self.seed = _checked_relation_sampler(name), seed

    def __enter__(self):
        self.prev = set_relation_sampler(self.name, self.seed)
        return self

    def __exit__(self, *exc):
        set_relation_sampler(self.prev)
        return False


def _gemm_terms():
    """Products per element of a training token GEMM under the current setting (the ``terms`` of the kernels.linear bindings)."""
    return 1 if MATMUL_PRECISION == "bf16" else 6


# ---- leaving a HIP fast path is never silent ------------------------------------------------------------------------------
# Every route from a hand-written kernel to an ATen composition (unsupported shape, misaligned operand, a device that
# refuses the cluster kernel) is counted here and announced ONCE per reason; EGTR_STRICT_FAST_PATH=1 (bench.py sets it)
# turns the first one into an error, so a benchmark number can not come from a deoptimised path.
FALLBACKS = {}
STRICT_FAST_PATH = os.environ.get("EGTR_STRICT_FAST_PATH", "0") == "1"


class FastPathError(RuntimeError):
    pass


def note_fallback(name, why=""):
    n = FALLBACKS.get(name, 0)
    FALLBACKS[name] = n + 1
    if STRICT_FAST_PATH:
        raise FastPathError(f"left the HIP fast path '{name}': {why}")
    if n == 0:
        import warnings
        warnings.warn(f"egtr_amd: leaving the HIP fast path '{name}' ({why}); counted in egtr_amd.ops.FALLBACKS",
                      RuntimeWarning, stacklevel=3)


def _gate(name, eligible, ok, why):
    """A fast-path predicate's verdict, announced when it turns a call away that the path exists for (``eligible``: right
    device, dtype, mode and size class -- an explicit EGTR_* switch or a CPU / bf16 / tiny call is not a fall-off)."""
    if eligible and not ok:
        note_fallback(name, why() if callable(why) else why)
    return bool(ok)


def inference_fast_path(x):
    """True when the launch-count optimisations (grouped linears, LayerNorm + position output, batched value
    projections) apply: fp32 tensors on the GPU and no autograd graph being recorded."""
    return x.is_cuda and x.dtype == torch.float32 and not torch.is_grad_enabled()


# Decoder at inference: the residual-add + LayerNorm steps run as prologues of the skinny linears that consume them
# (kernels.linear.DeferredLayerNorm) instead of in launches of their own.  "0": stand-alone add_layernorm_256 launches.
DEFER_LAYERNORM = True   # module attribute (tests patch it for the switch-off twin); no environment switch since round 6

# Token-sized fp32 linears (encoder: S ~ 12.5k rows) on the bf16 matrix cores through exact three-way operand splits
# (csrc/gemm_split.hip): fp32-level accuracy at 2.67x less matrix time than the fp32 MFMA / vendor fp32 GEMM.
# Inference (module_linear) and training (TokenLinearFunction: forward, data and weight gradients);
# EGTR_GEMM_SPLIT_BF16=0 keeps the vendor fp32 GEMM.
GEMM_SPLIT_BF16 = os.environ.get("EGTR_GEMM_SPLIT_BF16", "1") != "0"
# encoder at inference: the offsets / weights projection adds the position embeddings while loading its operand instead of
# reading a materialised `hidden + pos` written by the previous layer's epilogue ("0": materialise)
LAZY_POS = True   # module attribute (tests patch it for the switch-off twin); no environment switch since round 6
GEMM_SPLIT_MIN_ROWS = 4096
GEMM_SPLIT_WGRAD = True   # module attribute (tests patch it for the switch-off twin); no environment switch since round 6


def gemm_split_supported(x, N, K):
    rows = x.numel() // x.shape[-1]
    eligible = (GEMM_SPLIT_BF16 and x.is_cuda and x.dtype == torch.float32 and not torch.is_grad_enabled()
                and rows >= GEMM_SPLIT_MIN_ROWS)
    return _gate("gemm_split", eligible, eligible and K % 32 == 0 and N % 128 == 0,
                 lambda: f"{rows} x {K} -> {N}: K must be a multiple of 32 and N of 128 (vendor GEMM instead)")


def input_proj_x6_supported(feature_maps, input_proj):
    """Shapes the grouped input-projection launch serves (csrc/input_proj_x6.hip): fp32 inference with the split-bf16 products
    on, channels-last fp32 feature maps whose channel counts are multiples of 32, at most four levels of Conv2d -> 256 channels:
    a 1x1 / stride 1 convolution per map and at most one extra level, 3x3 / stride 2 / padding 1 of the last map."""
    maps = list(feature_maps)
    L = len(input_proj)
    eligible = (GEMM_SPLIT_BF16 and len(maps) > 0 and not torch.is_grad_enabled()
                and all(fm.is_cuda and fm.dtype == torch.float32 for fm in maps)
                and all(p[0].weight.dtype == torch.float32 for p in input_proj))
    if not eligible:
        return False

    def conv_ok(c, k, s, p):
        return (tuple(c.kernel_size) == (k, k) and tuple(c.stride) == (s, s) and tuple(c.padding) == (p, p)
                and tuple(c.dilation) == (1, 1) and c.groups == 1 and c.out_channels == 256 and c.in_channels % 32 == 0)
    ok = (len(maps) <= L <= min(len(maps) + 1, 4)
          and all(fm.dim() == 4 and fm.is_contiguous(memory_format=torch.channels_last) and fm.data_ptr() % 16 == 0
                  and fm.shape[0] == maps[0].shape[0] for fm in maps)
          and all(conv_ok(input_proj[l][0], 1, 1, 0) and input_proj[l][0].in_channels == maps[l].shape[1]
                  for l in range(len(maps)))
          and (L == len(maps) or (conv_ok(input_proj[L - 1][0], 3, 2, 1)
                                  and input_proj[L - 1][0].in_channels == maps[-1].shape[1])))
    return _gate("input_proj_x6", True, ok,
                 lambda: f"maps {[tuple(fm.shape) for fm in maps]}: channels-last, channels a multiple of 32, 1x1 projections to "
                         "256 channels and at most one 3x3 / stride 2 extra level are served (vendor products instead)")


def input_proj_x6_groupnorm(feature_maps, input_proj):
    """Input projections + conv bias + GroupNorm(32) + concatenation of all levels in four launches: the grouped K-split product
    (``input_proj_x6``) and the token GroupNorm whose statistics pass sums the K ranges.  Returns ([B, S, 256], [(H_l, W_l)])."""
    L = len(input_proj)
    wts = [cached_weights(input_proj[l][0], "input_proj_x6_weights", [input_proj[l][0].weight],
                          lambda l=l: input_proj_x6_weights(input_proj[l][0].weight)) for l in range(L)]
    maps = list(feature_maps)
    extra = L - len(maps)
    slabs, _, shapes = input_proj_x6(maps + maps[-1:] * extra, wts, [False] * len(maps) + [True] * extra)
    return input_proj_groupnorm_token_slabs(slabs, input_proj), shapes


def conv1x1_tail_supported(a, N):
    """Shapes the bottleneck-tail kernel serves (csrc/conv_tail_x6.hip): fp32 pixel rows with unit inner stride, K = planes in
    {64, 128, 256, 512}, N a multiple of 64."""
    return (a.is_cuda and a.dtype == torch.float32 and a.dim() == 2 and a.stride(1) == 1 and a.stride(0) % 4 == 0
            and a.data_ptr() % 16 == 0 and a.shape[1] in (64, 128, 256, 512) and N % 64 == 0)


def stem_fused_bf16_supported(x, w):
    return (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 4 and x.shape[1] == 3 and x.is_contiguous()
            and tuple(w.shape) == (64, 3, 7, 7) and w.dtype == torch.bfloat16)


def stem_fused_supported(x, w):
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 3 and x.is_contiguous()
            and tuple(w.shape) == (64, 3, 7, 7))


def conv3x3_supported(x, N, stride=1, variant=0):
    """Shapes the split-bf16 3x3 convolution serves (csrc/conv3x3_x6.hip): channels-last fp32 [B, C, H, W] tensors (dense NHWC
    memory), padding 1, C == N in {64, 128, 256, 512} at stride 1 and {128, 256, 512} at stride 2."""
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last)
            and x.data_ptr() % 16 == 0
            and int(_lib.lib().egtr_conv3x3_phase_channels(int(x.shape[1]), int(N), int(stride), int(variant))) > 0)


def conv1x1_strided_supported(x, N, stride):
    """Shapes the strided 1x1 convolution serves (csrc/conv3x3_x6.hip, one tap): channels-last fp32 [B, C, H, W] with C in
    {256, 512, 1024}, N a multiple of 128, stride 1 or 2."""
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last)
            and x.data_ptr() % 16 == 0 and x.shape[1] in (256, 512, 1024) and N % 128 == 0 and stride in (1, 2))


def conv1x1_tail_bf16_supported(a, N):
    """Shapes the bf16 bottleneck-tail kernel serves (csrc/conv_tail_bf16.hip): bf16 pixel rows with unit inner stride, K = planes
    in {64, 128, 256, 512}, N a multiple of 256."""
    return (a.is_cuda and a.dtype == torch.bfloat16 and a.dim() == 2 and a.stride(1) == 1 and a.stride(0) % 8 == 0
            and a.data_ptr() % 16 == 0 and a.shape[1] in (64, 128, 256, 512) and N % 256 == 0)


FFN_FUSED = os.environ.get("EGTR_FFN_FUSED", "1") != "0"


def ffn_fused_supported(x, fc1, fc2, ln):
    """The encoder layer's feed-forward block as one launch (csrc/ffn_x6.hip): fp32 inference, token-sized row counts,
    d_model = 256, hidden width a multiple of 64."""
    rows = x.numel() // x.shape[-1]
    eligible = FFN_FUSED and GEMM_SPLIT_BF16 and inference_fast_path(x) and rows >= GEMM_SPLIT_MIN_ROWS
    ok = (eligible and x.shape[-1] == 256 and tuple(fc1.weight.shape)[1] == 256 and fc1.weight.shape[0] % 64 == 0
          and tuple(fc2.weight.shape) == (256, fc1.weight.shape[0]) and fc1.bias is not None and fc2.bias is not None
          and ln.weight.shape[0] == 256 and fc1.weight.dtype == torch.float32)
    return _gate("ffn_fused", eligible, ok,
                 lambda: f"d_model {x.shape[-1]}, fc1 {tuple(fc1.weight.shape)}: the row-panel kernel serves d_model 256, "
                         "a hidden width that is a multiple of 64, biases present")


# The whole tail of an encoder layer (output projection + LayerNorm + FFN block + LayerNorm) as ONE launch
# (egtr_encoder_tail_x6_f32); "0": projection + LayerNorm and the FFN block as two launches.
ENCODER_TAIL_FUSED = True   # module attribute (tests patch it for the switch-off twin); no environment switch since round 6


def encoder_tail_fused_supported(context, out_proj, ln1, fc1, fc2, ln2):
    return (ENCODER_TAIL_FUSED and proj_ln_fused_supported(context, out_proj, ln1)
            and ffn_fused_supported(context, fc1, fc2, ln2))


def proj_ln_fused_supported(x, lin, ln):
    rows = x.numel() // x.shape[-1]
    eligible = FFN_FUSED and GEMM_SPLIT_BF16 and inference_fast_path(x) and rows >= GEMM_SPLIT_MIN_ROWS
    ok = (eligible and x.shape[-1] == 256 and tuple(lin.weight.shape) == (256, 256) and lin.bias is not None
          and ln.weight.shape[0] == 256 and lin.weight.dtype == torch.float32)
    return _gate("proj_ln_fused", eligible, ok, lambda: f"projection {tuple(lin.weight.shape)}: the kernel serves 256 -> 256 with a bias")


def proj_multi_fused_supported(x):
    rows = x.numel() // x.shape[-1]
    eligible = FFN_FUSED and GEMM_SPLIT_BF16 and inference_fast_path(x) and rows >= GEMM_SPLIT_MIN_ROWS
    return _gate("proj_multi_fused", eligible, eligible and x.shape[-1] == 256, lambda: f"d_model {x.shape[-1]} (256 served)")


def module_linear(mod, x, alpha=1.0, relu=False):
    w = mod.weight
    if alpha == 1.0 and gemm_split_supported(x, w.shape[0], w.shape[1]):
        wt = cached_weights(mod, "gemm_split_bf16", [w], lambda: gemm_split_weights(w))
        return linear_split_bf16(x, wt, mod.bias, w.shape[0], relu)
    return linear(x, mod.weight, mod.bias, alpha, relu)


class BiasActFunction(Function):
    """y = relu(x + bias[c] (+ residual)) on an NCHW fp32 activation under autograd: one HIP pass forward
    (egtr_bias_act_nchw_f32), one mask pass backward (the masked gradient is the gradient of x AND of the residual)."""

    @staticmethod
    def forward(ctx, x, bias, residual):
        x = _chk(x.contiguous(), "x", torch.float32)
        _chk(bias, "bias", torch.float32)
        r = _chk(residual.contiguous(), "residual", torch.float32) if residual is not None else None
        N, C, H, W_ = x.shape
        y = torch.empty_like(x)
        _lib.launch("egtr_bias_act_nchw_f32", x.data_ptr(), bias.data_ptr(), _lib.ptr(r), y.data_ptr(), N, C, H * W_, 1)
        ctx.save_for_backward(y)
        ctx.has_residual = residual is not None
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        gm = torch.ops.aten.threshold_backward(g.contiguous(), y, 0.0)
        return gm, None, gm if ctx.has_residual else None


def bias_act(x, bias, residual=None):
    """relu(x + bias[c] (+ residual)) with autograd through x and residual (bias: a constant, e.g. a frozen-BN shift)."""
    return BiasActFunction.apply(x, bias, residual)


class LevelGeometryTrainFunction(Function):
    """``level_geometry`` under autograd: the position embeddings are sine(pixel_mask) + level_embed[level], so the only
    gradient is d level_embed[l] = sum over the tokens of level l (all images) of d pos -- four mask-weighted column sums over the
    [B * S, 256] gradient (egtr_weighted_column_sum_f32, ~13 us each) instead of autograd's cat-backward slices and generic
    `sum` reductions (161 us for the largest level).  Replaces, in training, the per-level mask interpolation, sine embedding,
    `+ level_embed`, cat, get_valid_ratio and get_reference_points compositions (model/deformable_detr.py:2195-2278, 1616-1648)
    by the two launches the inference path uses."""

    @staticmethod
    def forward(ctx, level_embed, pixel_mask, spatial_shapes_list, embedding_dim, temperature, scale):
        mask, pos, vr, ref, _ = level_geometry(pixel_mask, spatial_shapes_list, level_embed, embedding_dim, temperature, scale)
        ctx.shapes = (tuple(spatial_shapes_list), pos.shape[0])
        ctx.mark_non_differentiable(mask, vr, ref)
        return pos, mask, vr, ref

    @staticmethod
    @once_differentiable
    def backward(ctx, g_pos, g_mask, g_vr, g_ref):
        shapes, B = ctx.shapes
        g2 = _rows256(g_pos)
        return torch.stack([weighted_column_sum(g2, wl) for wl in _level_row_weights(shapes, B, g2.device)]), \
            None, None, None, None, None


# One-hot level membership of every token row ([B * S] floats per level): a constant of (level shapes, batch).  Multi-scale
# training meets a new shape combination in most batches, so the table is a small LRU (each entry is L x B*S floats on the
# device) and an entry is built ON the device from an arange -- no host tensor, no H2D copy, legal under stream capture.
_LEVEL_ROW_WEIGHTS = {}
_LEVEL_ROW_WEIGHTS_MAX = 4


def _level_row_weights(shapes, B, device):
    key = (shapes, B, str(device))
    w = _LEVEL_ROW_WEIGHTS.pop(key, None)
    if w is None:
        sizes = [h * w_ for h, w_ in shapes]
        S = sum(sizes)
        tok = torch.arange(B * S, device=device, dtype=torch.int32) % S      # token index within its image
        w, start = [], 0
        for n in sizes:   # (separate allocations: a row of one [L, B * S] tensor is 16-byte aligned only when B * S % 4 == 0)
            w.append(((tok >= start) & (tok < start + n)).to(torch.float32))
            start += n
        while len(_LEVEL_ROW_WEIGHTS) >= _LEVEL_ROW_WEIGHTS_MAX:
            _LEVEL_ROW_WEIGHTS.pop(next(iter(_LEVEL_ROW_WEIGHTS)))
    _LEVEL_ROW_WEIGHTS[key] = w   # (re-inserted last: most recently used)
    return w


def level_geometry_train(pixel_mask, spatial_shapes_list, level_embed, embedding_dim, temperature, scale):
    """(mask_flatten, lvl_pos_embed_flatten, valid_ratios, encoder reference points) with autograd through level_embed."""
    pos, mask, vr, ref = LevelGeometryTrainFunction.apply(level_embed, pixel_mask, list(spatial_shapes_list), embedding_dim,
                                                          temperature, scale)
    return mask, pos, vr, ref


class AddLayerNormFunction(Function):
    """LayerNorm(x + residual) over 256 channels in one pass (csrc/elementwise.hip).  Backward: one pass as well
    (egtr_add_layernorm_backward_f32: statistics recomputed from the saved inputs, gamma / beta gradients from
    per-workgroup partials in a fixed order)."""

    @staticmethod
    def forward(ctx, x, residual, weight, bias, eps):
        x2 = _chk(x.contiguous(), "x", torch.float32)
        r2 = _chk(residual.contiguous(), "residual", torch.float32)
        y = torch.empty_like(x2)
        _lib.launch("egtr_add_layernorm_f32", x2.data_ptr(), r2.data_ptr(), weight.data_ptr(), bias.data_ptr(), y.data_ptr(),
                    x2.numel() // x2.shape[-1], x2.shape[-1], float(eps))
        ctx.eps = eps
        ctx.save_for_backward(x2, r2, weight, bias)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        lib = _lib.lib()
        x, r, w, b = ctx.saved_tensors
        g = _chk(gy.contiguous(), "grad", torch.float32)
        rows = x.numel() // x.shape[-1]
        gs = torch.empty_like(x)
        ws = torch.empty(int(lib.egtr_add_layernorm_backward_workspace_floats(rows)), dtype=torch.float32, device=x.device)
        gwb = torch.empty(2, x.shape[-1], dtype=torch.float32, device=x.device)
        _lib.launch("egtr_add_layernorm_backward_f32", x.data_ptr(), r.data_ptr(), w.data_ptr(), g.data_ptr(), gs.data_ptr(),
                    ws.data_ptr(), gwb.data_ptr(), rows, x.shape[-1], float(ctx.eps))
        return gs, gs, gwb[0], gwb[1], None


def add_layer_norm(x, residual, ln):
    """ln(residual + x) for an nn.LayerNorm over d_model = 256."""
    if x.is_cuda and x.dtype == torch.float32 and x.shape[-1] == 256:
        return AddLayerNormFunction.apply(x, residual, ln.weight, ln.bias, ln.eps)
    if (x.is_cuda and x.dtype == torch.bfloat16 and x.shape[-1] == 256 and not torch.is_grad_enabled()
            and ln.weight.dtype == torch.bfloat16 and residual.dtype == torch.bfloat16):
        # bf16 inference (stress configuration): one pass, fp32 statistics
        lib = _lib.lib()
        x2 = _chk(x.contiguous(), "x", torch.bfloat16)
        r2 = _chk(residual.contiguous(), "residual", torch.bfloat16)
        y = torch.empty_like(x2)
        _lib.launch("egtr_add_layernorm_bf16", x2.data_ptr(), r2.data_ptr(), ln.weight.data_ptr(), ln.bias.data_ptr(),
                    y.data_ptr(), x2.numel() // 256, 256, float(ln.eps))
        return y
    return ln(residual + x)


class RelationHeadFunction(Function):
    """Fused pairwise gate + gated sum + relation / connectivity MLPs (replaces model/egtr.py:366-416)."""

    @staticmethod
    def forward(ctx, gate_q, gate_k, uq, uk, b1, w2r, b2r, w3r, b3r, w2c, b2c, w3c, b3c, triplet_dist, node_cls,
                want_gate_mean):
        B, N, T = gate_q.shape
        Hd = w2r.shape[1]
        R = w3r.shape[0]
        tens = [gate_q, gate_k, uq, uk, b1, w2r, b2r, w3r, b3r, w2c, b2c, w3c, b3c]
        names = ["gate_q", "gate_k", "uq", "uk", "b1", "w2r", "b2r", "w3r", "b3r", "w2c", "b2c", "w3c", "b3c"]
        tens = [_chk(t.contiguous(), n, torch.float32) for t, n in zip(tens, names)]
        need_grad = any(ctx.needs_input_grad[:13])
        ctx.terms = 6
        if REL_HEAD_TRAIN_X6 and need_grad and GEMM_SPLIT_BF16 and Hd == 256 and R <= 64 and T in (4, 7):
            # layers 2 and 3 on the bf16 matrix cores from split operands (the inference kernel with the two activation stores the
            # backward needs); the weight streams are rebuilt by one launch -- the weights change every step.  Matmul precision
            # "bf16": the one-term kernel on one-piece streams, read once -- the backward multiplies the way the forward did
            ctx.terms = _gemm_terms()
            rel, conn, gm, h1s, h2s = relation_head_train_forward(*tens, triplet_dist, node_cls, want_gate_mean, ctx.terms)
        else:   # exact f32 under either matmul precision (a route, not a fall-off), and so is its backward
            rel = torch.empty(B, N, N, R, dtype=torch.float32, device=gate_q.device)
            conn = torch.empty(B, N, N, dtype=torch.float32, device=gate_q.device)
            gm = torch.zeros(T, dtype=torch.float32, device=gate_q.device) if want_gate_mean else None
            if triplet_dist is not None:
                _chk(triplet_dist, "triplet_dist", torch.float32)
                _chk(node_cls, "node_cls", torch.int64)
                c1 = triplet_dist.shape[0]
            else:
                c1 = 0
            P_ = B * N * N
            h1s = torch.empty(2, P_, Hd, dtype=torch.float32, device=gate_q.device) if need_grad else None
            h2s = torch.empty(2, P_, Hd, dtype=torch.float32, device=gate_q.device) if need_grad else None
            # more than 64 predicate classes: the wide entry (layer 3 per output tile), the same arithmetic and the same saves
            _lib.launch("egtr_rel_head_forward_wide_f32" if R > REL_HEAD_NARROW_MAX_REL else "egtr_rel_head_forward_save_f32",
                        *[t.data_ptr() for t in tens], _lib.ptr(triplet_dist),
                        _lib.ptr(node_cls if triplet_dist is not None else None), B, N, T, Hd, R, c1, rel.data_ptr(),
                        conn.data_ptr(), _lib.ptr(gm), _lib.ptr(h1s), _lib.ptr(h2s))
        if need_grad:
            ctx.save_for_backward(*tens, h1s, h2s)
        return rel, conn.unsqueeze(-1), gm

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_rel, grad_conn, grad_gm):
        """MLP part: rocBLAS GEMMs on the [B*N*N, 256] activations the forward kernel saved (no recomputation; the
        ReLU masks are applied with threshold_backward).  Pairwise part (gradients of the per-query tables and of
        the gate logits): HIP, egtr_rel_head_backward_pairs_f32.  The frequency bias is an additive constant.
        A forward that took the one-term route (ctx.terms == 1, matmul precision "bf16"): the two layer-2 products of each MLP
        round their operands once to bf16 -- dh1 = (dh2 W2) * [h1 > 0] with the 32-row partial column sums of the b1 gradient is
        ONE egtr_linear_split_bf16_ex_f32 launch per MLP (instead of the vendor GEMM and a masked column-sum pass over its
        result), dW2 the one-term weight gradient; layer 3 (reduction or output of num_rel / 1) stays fp32."""
        (gate_q, gate_k, uq, uk, b1, w2r, b2r, w3r, b3r, w2c, b2c, w3c, b3c, h1s, h2s) = ctx.saved_tensors
        B, N, T = gate_q.shape
        Hd = w2r.shape[1]
        R = w3r.shape[0]
        P_ = B * N * N
        G = grad_rel.reshape(P_, R).contiguous()
        gc = grad_conn.reshape(P_, 1).contiguous()
        dh1 = torch.empty(2, P_, Hd, dtype=torch.float32, device=G.device)
        one_term = ctx.terms == 1 and Hd % 128 == 0
        if one_term:
            wgrad = ((lambda g, h: linear_split_bf16_wgrad(g, h, terms=1)) if GEMM_SPLIT_WGRAD else (lambda g, h: g.t() @ h))
            colp = torch.empty(2, (P_ + 31) // 32, Hd, dtype=torch.float32, device=G.device)

            def dgrad(g, w2, i):   # dh1[i] <- (g W2) * [h1s[i] > 0], colp[i] <- its column sums per 32 rows
                linear_split_ex([dict(x=g, wt=gemm_split_tile(w2, transposed=True, terms=1), N=Hd, relu_ref=h1s[i],
                                      colpart=colp[i], out=dh1[i])], P_, Hd, terms=1)
        else:
            wgrad = (linear_split_bf16_wgrad if GEMM_SPLIT_BF16 and GEMM_SPLIT_WGRAD and Hd % 128 == 0
                     else (lambda g, h: g.t() @ h))

            def dgrad(g, w2, i):
                torch.mm(g, w2, out=dh1[i])
        # relation MLP (ReLU masks and bias gradients: one pass each, egtr_column_sum_f32, the mask applied in place)
        dh2, db2r = column_sum(G @ w3r, relu_output=h2s[0], inplace=True)
        dw3r = G.t() @ h2s[0]
        db3r = G.sum(0)   # 50 columns: the generic reduction is faster (19 vs 30 us)
        dgrad(dh2, w2r, 0)
        dw2r = wgrad(dh2, h1s[0])
        # connectivity MLP (one output)
        dh2, db2c = column_sum(gc * w3c, relu_output=h2s[1], inplace=True)
        dw3c = weighted_column_sum(h2s[1], gc).view(1, -1)   # gc^T h2: one pass instead of a 220 us GEMV
        db3c = gc.sum(0)
        dgrad(dh2, w2c, 1)
        dw2c = wgrad(dh2, h1s[1])
        del dh2
        if one_term:   # the 32-row partial sums finished in a fixed order
            db1 = torch.cat([column_sum(colp[i]) for i in range(2)])
        else:
            db1 = torch.cat([column_sum(dh1[i], relu_output=h1s[i], inplace=True)[1] for i in range(2)])
        duq = torch.empty_like(uq)
        duk = torch.empty_like(uk)
        dgq = torch.empty_like(gate_q)
        dgk = torch.empty_like(gate_k)
        dz = torch.empty(P_ * T, dtype=torch.float32, device=G.device)
        _lib.launch("egtr_rel_head_backward_pairs_f32", dh1.data_ptr(), gate_q.data_ptr(), gate_k.data_ptr(), uq.data_ptr(),
                    uk.data_ptr(), B, N, T, Hd, duq.data_ptr(), duk.data_ptr(), dgq.data_ptr(), dgk.data_ptr(), dz.data_ptr())
        return (dgq, dgk, duq, duk, db1, dw2r, db2r, dw3r, db3r, dw2c, db2c, dw3c, db3c, None, None, None)


# bf16 model: layer 1 of the relation head (gated sum over the slots) on the matrix cores as well, tables pre-packed in
# operand order, W2 resident in LDS (csrc/rel_head_bf16.hip).  "0": the VALU layer 1 of rel_head_fwd_bf16w.
REL_HEAD_BF16_PACKED = True   # module attribute (tests patch it for the switch-off twin); no environment switch since round 6


def relation_head_bf16w(gate_q, gate_k, uq, uk, b1, w2r, b2r, w3r, b3r, w2c, b2c, w3c, b3c, triplet_dist=None,
                        node_cls=None, want_gate_mean=False):
    """Inference forward of a bf16 model: the matrix products on the bf16 matrix cores with the bf16 parameters as they are
    (egtr_rel_head_forward_bf16p: all three layers, per-query tables uq / uk rounded to bf16 -- a bf16 model produces them
    in bf16 -- and packed in operand order by egtr_rel_head_pack_tables_bf16; or, with ops.REL_HEAD_BF16_PACKED = False,
    egtr_rel_head_forward_bf16w with an fp32 VALU layer 1); gates, biases and the outputs are fp32.  No autograd."""
    B, N, T = gate_q.shape
    Hd = w2r.shape[1]
    R = w3r.shape[0]
    dev = gate_q.device
    if R > REL_HEAD_NARROW_MAX_REL:   # neither bf16 entry serves them: ``_relation_head`` routes such a model to the fp32 wide kernel
        raise ValueError(f"relation_head_bf16w serves at most {REL_HEAD_NARROW_MAX_REL} predicate classes, got {R}")
    packed = REL_HEAD_BF16_PACKED and T <= 10 and Hd == 256 and R <= 64
    tables = []
    for t, n in ((uq, "uq"), (uk, "uk")):
        t = t.detach()
        if packed and t.dtype == torch.bfloat16:
            tables.append(_chk(t.contiguous(), n, torch.bfloat16))
        else:
            tables.append(_chk(t.float().contiguous(), n, torch.float32))
    f32 = [_chk(t.detach().float().contiguous(), n, torch.float32)
           for t, n in ((gate_q, "gate_q"), (gate_k, "gate_k"), (b1, "b1"), (b2r, "b2r"),
                        (b3r, "b3r"), (b2c, "b2c"), (b3c, "b3c"))]
    gq, gk, b1_, b2r_, b3r_, b2c_, b3c_ = f32
    wts = [_chk(t.detach().contiguous(), n, torch.bfloat16)
           for t, n in ((w2r, "w2r"), (w3r, "w3r"), (w2c, "w2c"), (w3c, "w3c"))]
    w2r_, w3r_, w2c_, w3c_ = wts
    rel = torch.empty(B, N, N, R, dtype=torch.float32, device=dev)
    conn = torch.empty(B, N, N, dtype=torch.float32, device=dev)
    gm = torch.zeros(T, dtype=torch.float32, device=dev) if want_gate_mean else None
    td = None
    c1 = 0
    if triplet_dist is not None:
        td = _chk(triplet_dist.detach().float().contiguous(), "triplet_dist", torch.float32)
        _chk(node_cls, "node_cls", torch.int64)
        c1 = td.shape[0]
    if packed:
        if tuple(tables[0].shape) != (B, N, T, 2 * Hd) or tuple(tables[1].shape) != (B, N, T, 2 * Hd):
            raise ValueError("relation_head_bf16w: uq / uk must be [B, N, T, 512]")
        pk = []
        for t in tables:   # [B * N] rows of [mlp 2][tile 8][half 2][channel 32][8 slots] bf16 = 16 KiB
            out = torch.empty(B * N, 8192, dtype=torch.bfloat16, device=dev)
            _lib.launch("egtr_rel_head_pack_tables_bf16", t.data_ptr(), int(t.dtype == torch.bfloat16), B * N, T,
                        out.data_ptr())
            pk.append(out)
        _lib.launch("egtr_rel_head_forward_bf16p", gq.data_ptr(), gk.data_ptr(), pk[0].data_ptr(), pk[1].data_ptr(),
                    b1_.data_ptr(), w2r_.data_ptr(), b2r_.data_ptr(), w3r_.data_ptr(), b3r_.data_ptr(), w2c_.data_ptr(),
                    b2c_.data_ptr(), w3c_.data_ptr(), b3c_.data_ptr(), _lib.ptr(td),
                    _lib.ptr(node_cls if td is not None else None), B, N, T, Hd, R, c1, rel.data_ptr(), conn.data_ptr(),
                    _lib.ptr(gm))
        return rel, conn.unsqueeze(-1), gm
    uq_, uk_ = tables
    _lib.launch("egtr_rel_head_forward_bf16w", gq.data_ptr(), gk.data_ptr(), uq_.data_ptr(), uk_.data_ptr(), b1_.data_ptr(),
                w2r_.data_ptr(), b2r_.data_ptr(), w3r_.data_ptr(), b3r_.data_ptr(), w2c_.data_ptr(), b2c_.data_ptr(),
                w3c_.data_ptr(), b3c_.data_ptr(), _lib.ptr(td), _lib.ptr(node_cls if td is not None else None), B, N, T, Hd, R,
                c1, rel.data_ptr(), conn.data_ptr(), _lib.ptr(gm))
    return rel, conn.unsqueeze(-1), gm


# fp32 relation head on the bf16 matrix cores through three-way operand splits (csrc/rel_head.hip, rel_head_fwd_x6):
# fp32-level accuracy (tested against float64) at 2.67x less matrix time.  Inference only; set to False to run the
# exact-f32 MFMA kernel (v_mfma_f32_32x32x2_f32) everywhere.
REL_HEAD_SPLIT_BF16 = os.environ.get("EGTR_REL_HEAD_SPLIT_BF16", "1") != "0"


def relation_head(gate_q, gate_k, uq, uk, b1, w2r, b2r, w3r, b3r, w2c, b2c, w3c, b3c, triplet_dist=None,
                  node_cls=None, want_gate_mean=False, owner=None, sigmoid=False):
    """``owner`` (optional nn.Module): where the derived split-bf16 weight streams of the inference kernel are cached.
    ``sigmoid``: return sigmoid(logits) (the model outputs) instead of the logits -- in the inference kernel's epilogue."""
    if want_gate_mean and is_deterministic() and gate_q.is_cuda:
        # the kernels add the logged gate means with fp32 atomics: under the mode they get no gate_mean buffer and the means are
        # reduced by torch (fixed order); the model outputs do not depend on them
        rel, conn, _ = relation_head(gate_q, gate_k, uq, uk, b1, w2r, b2r, w3r, b3r, w2c, b2c, w3c, b3c, triplet_dist,
                                     node_cls, False, owner, sigmoid)
        with torch.no_grad():
            gq, gk = gate_q.detach().float(), gate_k.detach().float()
            gm = torch.sigmoid(gq[:, :, None, :] + gk[:, None, :, :]).mean(dim=(0, 1, 2))
        return rel, conn, gm
    if sigmoid:
        rel, conn, gm = _relation_head(gate_q, gate_k, uq, uk, b1, w2r, b2r, w3r, b3r, w2c, b2c, w3c, b3c, triplet_dist,
                                       node_cls, want_gate_mean, owner, True)
        return rel, conn, gm
    return _relation_head(gate_q, gate_k, uq, uk, b1, w2r, b2r, w3r, b3r, w2c, b2c, w3c, b3c, triplet_dist, node_cls,
                          want_gate_mean, owner, False)


def _relation_head(gate_q, gate_k, uq, uk, b1, w2r, b2r, w3r, b3r, w2c, b2c, w3c, b3c, triplet_dist, node_cls,
                   want_gate_mean, owner, sigmoid):
    if (REL_HEAD_SPLIT_BF16 and owner is not None and gate_q.dtype == torch.float32 and gate_q.is_cuda
            and w2r.shape == (256, 256) and w3r.shape[0] <= REL_HEAD_MAX_REL and gate_q.shape[-1] <= 9
            and not (torch.is_grad_enabled() and any(
                t.requires_grad for t in (gate_q, gate_k, uq, uk, b1, w2r, b2r, w3r, b3r, w2c, b2c, w3c, b3c)))):
        if w3r.shape[0] > REL_HEAD_NARROW_MAX_REL:   # 65 .. 256 predicate classes: the wide kernel, streams of their own
            w2xr, w3xr, w2xc = cached_weights(owner, "rel_head_split_bf16_wide", [w2r, w3r, w2c],
                                              lambda: rel_head_streams_wide(w2r, w3r, w2c))
            return relation_head_split_bf16_wide(gate_q, gate_k, uq, uk, b1, w2xr, b2r, w3xr, b3r, w2xc, b2c, w3c, b3c,
                                                 w3r.shape[0], triplet_dist, node_cls, want_gate_mean, sigmoid)
        w2xr, w3xr, w2xc = cached_weights(owner, "rel_head_split_bf16", [w2r, w3r, w2c],
                                          lambda: rel_head_split_weights(w2r, w3r, w2c))
        return relation_head_split_bf16(gate_q, gate_k, uq, uk, b1, w2xr, b2r, w3xr, b3r, w2xc, b2c, w3c, b3c,
                                        w3r.shape[0], triplet_dist, node_cls, want_gate_mean, sigmoid)
    if sigmoid:   # every other kernel returns logits
        rel, conn, gm = _relation_head(gate_q, gate_k, uq, uk, b1, w2r, b2r, w3r, b3r, w2c, b2c, w3c, b3c, triplet_dist,
                                       node_cls, want_gate_mean, None, False)
        return rel.sigmoid(), conn.sigmoid(), gm
    # (a bf16 model has no fast route above 64 predicate classes: egtr_rel_head_forward_bf16w / _bf16p refuse them, the call
    # falls through to the fp32 wide kernel on widened operands below)
    if gate_q.dtype == torch.bfloat16 and w3r.shape[0] <= REL_HEAD_NARROW_MAX_REL and not (
            torch.is_grad_enabled() and any(
            t.requires_grad for t in (gate_q, gate_k, uq, uk, b1, w2r, b2r, w3r, b3r, w2c, b2c, w3c, b3c))):
        rel, conn, gm = relation_head_bf16w(gate_q, gate_k, uq, uk, b1, w2r, b2r, w3r, b3r, w2c, b2c, w3c, b3c,
                                            triplet_dist, node_cls, want_gate_mean)
        return rel.to(torch.bfloat16), conn.to(torch.bfloat16), gm
    if gate_q.dtype != torch.float32:  # fp16 models / bf16 training: fp32 kernel, outputs cast back
        dt = gate_q.dtype
        f = [t.float() for t in (gate_q, gate_k, uq, uk, b1, w2r, b2r, w3r, b3r, w2c, b2c, w3c, b3c)]
        rel, conn, gm = RelationHeadFunction.apply(*f, triplet_dist.float() if triplet_dist is not None else None,
                                                   node_cls, want_gate_mean)
        return rel.to(dt), conn.to(dt), gm
    return RelationHeadFunction.apply(gate_q, gate_k, uq, uk, b1, w2r, b2r, w3r, b3r, w2c, b2c, w3c, b3c,
                                      triplet_dist, node_cls, want_gate_mean)


class RelationLossFunction(Function):
    """loss_rel / loss_connectivity of the SGG criterion (training mode) with their gradients from one pass over the logits
    (csrc/loss.hip, egtr_relation_loss_f32), one sampling policy per candidate class: ``negatives`` / ``nonmatching`` =
    (policy, count), policy "largest" | "random" | "all".  ``target``: the pointer table of the dense targets or, when
    ``packed``, the words [B, N, N] / the wide words [B, N, N, ceil(R / 64)].  ``seed`` / ``stream``: the words of a random
    class's keys.  Backward only scales the stored gradients."""

    @staticmethod
    def forward(ctx, pred_rel, pred_conn, target, pred_idx, tgt_idx, match_cost, out_off, nonmatching_cost, negatives,
                nonmatching, seed, stream, packed=False):
        pr = _chk(pred_rel.detach().contiguous(), "pred_rel", torch.float32)
        pc = _chk(pred_conn.detach().contiguous(), "pred_connectivity", torch.float32)
        loss, grad_rel, grad_conn = relation_loss_policy_launch(pr, pc, target, packed, pred_idx, tgt_idx, match_cost, out_off,
                                                                nonmatching_cost, negatives, nonmatching, seed, stream,
                                                                deterministic=is_deterministic())
        ctx.save_for_backward(grad_rel, grad_conn)
        return loss[0], loss[1]

    @staticmethod
    @once_differentiable
    def backward(ctx, g_rel, g_conn):
        grad_rel, grad_conn = ctx.saved_tensors
        return (grad_rel * g_rel, grad_conn * g_conn) + (None,) * 11


RELATION_LOSS_ALL = True   # module attribute (tests patch it for the switch-off twin); no environment switch


class RelationLossAllFunction(Function):
    """loss_rel / loss_connectivity of the SGG criterion WITHOUT sampling -- evaluation mode (validation_loss) and training with
    both ``rel_sample_*`` None: BCE over all N N R elements (csrc/loss.hip, egtr_relation_loss_all_f32; ``target`` / ``packed``
    as in RelationLossFunction).  ``want_grad``: None = when ``pred_rel`` or ``pred_conn`` requires grad; False is the
    value-only launch -- no gradient buffer exists.  Backward only scales the stored gradients."""

    @staticmethod
    def forward(ctx, pred_rel, pred_conn, target, pred_idx, tgt_idx, match_cost, out_off, nonmatching_cost, packed=False,
                want_grad=None):
        pr = _chk(pred_rel.detach().contiguous(), "pred_rel", torch.float32)
        pc = _chk(pred_conn.detach().contiguous(), "pred_connectivity", torch.float32)
        if want_grad is None:
            want_grad = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        loss, grad_rel, grad_conn = relation_loss_all_launch(pr, pc, target, packed, pred_idx, tgt_idx, match_cost, out_off,
                                                             nonmatching_cost, want_grad=bool(want_grad))
        ctx.has_grad = bool(want_grad)
        if ctx.has_grad:
            ctx.save_for_backward(grad_rel, grad_conn)
        return loss[0], loss[1]

    @staticmethod
    @once_differentiable
    def backward(ctx, g_rel, g_conn):
        if not ctx.has_grad:
            raise RuntimeError("RelationLossAllFunction ran its value-only launch (want_grad=False): there is no gradient")
        grad_rel, grad_conn = ctx.saved_tensors
        return grad_rel * g_rel, grad_conn * g_conn, None, None, None, None, None, None, None, None


class ClampNonFiniteFunction(Function):
    """dd:1346-1351 ("clamp the states iff any element is inf / nan") with the decision on the device: one reduction pass
    raises a flag, the in-place clamp and the gradient mask return at once while it is clear (csrc/elementwise.hip)."""

    @staticmethod
    def forward(ctx, x):
        _chk(x, "hidden_states", torch.float32)
        flag = torch.zeros(1, dtype=torch.int32, device=x.device)
        cv = torch.finfo(torch.float32).max - 1000
        _lib.launch("egtr_any_nonfinite_f32", x.data_ptr(), x.numel(), flag.data_ptr())
        _lib.launch("egtr_clamp_if_flag_f32", x.data_ptr(), None, x.numel(), flag.data_ptr(), cv, 0)
        ctx.mark_dirty(x)
        ctx.save_for_backward(x, flag)
        ctx.cv = cv
        return x

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, flag = ctx.saved_tensors
        # Autograd forbids mutating a grad_output (the same buffer may be another branch's gradient: AddLayerNorm's backward
        # hands ONE tensor to x and to the residual), so the mask is applied to a private copy: one extra pass over the
        # states per encoder layer (~0.3 % of a step) for a result that is correct on the steps that did clamp.
        g = g.clone(memory_format=torch.contiguous_format)
        _lib.launch("egtr_clamp_if_flag_f32", g.data_ptr(), x.data_ptr(), g.numel(), flag.data_ptr(), ctx.cv, 1)
        return g


def clamp_nonfinite_(x):
    """In place: x <- clamp(x, +-(finfo.max - 1000)) iff x holds an inf / nan (no host synchronisation).  fp32 contiguous
    device tensors; anything else takes the tensor composition of the same function."""
    if x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.data_ptr() % 16 == 0:
        return ClampNonFiniteFunction.apply(x)
    bad = torch.logical_not(torch.isfinite(x).all())
    cv = torch.finfo(x.dtype).max - 1000
    return torch.where(bad, torch.clamp(x, min=-cv, max=cv), x)


class DetectionLossFunction(Function):
    """loss_ce / loss_bbox / loss_giou (+ the cardinality counts) of one output set with their gradients from one launch
    (csrc/loss.hip, egtr_detection_loss_f32); backward only scales the stored gradients."""

    @staticmethod
    def forward(ctx, logits, boxes, pred_idx, tgt_idx, match_off, tgt_labels, tgt_boxes, tgt_off, focal_alpha,
                num_boxes):
        B, N, C = logits.shape
        lg = _chk(logits.detach().contiguous(), "logits", torch.float32)
        bx = _chk(boxes.detach().contiguous(), "pred_boxes", torch.float32)
        dev = lg.device
        out = torch.empty(B, 4, dtype=torch.float32, device=dev)
        d_logits = torch.empty_like(lg)
        d_l1 = torch.empty_like(bx)
        d_giou = torch.empty_like(bx)
        _lib.launch("egtr_detection_loss_f32", lg.data_ptr(), bx.data_ptr(), pred_idx.data_ptr(), tgt_idx.data_ptr(),
                    match_off.data_ptr(), tgt_labels.data_ptr(), tgt_boxes.data_ptr(), tgt_off.data_ptr(), B, N, C,
                    float(focal_alpha), float(num_boxes), d_logits.data_ptr(), d_l1.data_ptr(), d_giou.data_ptr(),
                    out.data_ptr())
        ctx.save_for_backward(d_logits, d_l1, d_giou)
        sums = out.sum(0)
        card = out[:, 3]
        ctx.mark_non_differentiable(card)
        return sums[0], sums[1], sums[2], card

    @staticmethod
    @once_differentiable
    def backward(ctx, g_ce, g_bbox, g_giou, g_card):
        d_logits, d_l1, d_giou = ctx.saved_tensors
        return (d_logits * g_ce, d_l1 * g_bbox + d_giou * g_giou, None, None, None, None, None, None, None, None)


def detection_losses(logits, pred_boxes, flat_match, packed_targets, focal_alpha, num_boxes):
    """{"loss_ce", "loss_bbox", "loss_giou", "cardinality_error"} of one output set (egtr:611-712) from one launch.
    ``flat_match``: (pred_idx, tgt_idx, n_out) as the device matcher packs them; ``packed_targets``:
    ``pack_detection_targets``."""
    pred_idx, tgt_idx, n_out = flat_match
    labels, boxes, toff, lengths = packed_targets
    offs = [0]
    for n in n_out:
        offs.append(offs[-1] + int(n))
    moff = torch.tensor(offs, dtype=torch.int32).to(logits.device, non_blocking=True)
    if pred_idx.numel() == 0:
        pred_idx = torch.zeros(1, dtype=torch.int64, device=logits.device)
        tgt_idx = torch.zeros(1, dtype=torch.int64, device=logits.device)
    ce, bbox, giou, card = DetectionLossFunction.apply(logits, pred_boxes, pred_idx, tgt_idx, moff, labels, boxes, toff,
                                                       focal_alpha, num_boxes)
    return {"loss_ce": ce, "loss_bbox": bbox, "loss_giou": giou,
            "cardinality_error": (card - lengths).abs().mean()}


class DetectionLossLargeFunction(Function):
    """``DetectionLossFunction`` for proposal-sized output sets (csrc/loss.hip, egtr_detection_loss_large_f32: up to 65 536
    queries).  ``tgt_labels`` None: class-agnostic targets."""

    @staticmethod
    def forward(ctx, logits, boxes, pred_idx, tgt_idx, match_off, tgt_labels, tgt_boxes, tgt_off, focal_alpha,
                num_boxes):
        out, d_logits, d_l1, d_giou = detection_loss_large_launch(
            logits.detach().contiguous(), boxes.detach().contiguous(), pred_idx, tgt_idx, match_off, tgt_labels, tgt_boxes,
            tgt_off, focal_alpha, num_boxes, want_grad=True)
        ctx.save_for_backward(d_logits, d_l1, d_giou)
        sums = out.sum(0)
        card = out[:, 3]
        ctx.mark_non_differentiable(card)
        return sums[0], sums[1], sums[2], card

    @staticmethod
    @once_differentiable
    def backward(ctx, g_ce, g_bbox, g_giou, g_card):
        d_logits, d_l1, d_giou = ctx.saved_tensors
        return (d_logits * g_ce, d_l1 * g_bbox + d_giou * g_giou, None, None, None, None, None, None, None, None)


def detection_losses_large(logits, pred_boxes, flat_match, packed_targets, focal_alpha, num_boxes, class_agnostic=False):
    """``detection_losses`` for an output set of up to 65 536 queries (the two-stage variant's per-token proposals): the
    same four terms from egtr_detection_loss_large_f32.  ``class_agnostic``: every target's class is 0, whatever labels
    ``packed_targets`` holds (the ``*_enc`` terms score the proposals against class-agnostic copies of the step's targets,
    so the step's own packed targets serve).  When no gradient can be asked for (grad mode off, or neither input requires
    one) the value-only launch runs and no gradient buffer is allocated."""
    pred_idx, tgt_idx, n_out = flat_match
    labels, boxes, toff, lengths = packed_targets
    offs = [0]
    for n in n_out:
        offs.append(offs[-1] + int(n))
    moff = torch.tensor(offs, dtype=torch.int32).to(logits.device, non_blocking=True)
    if pred_idx.numel() == 0:
        pred_idx = torch.zeros(1, dtype=torch.int64, device=logits.device)
        tgt_idx = torch.zeros(1, dtype=torch.int64, device=logits.device)
    if class_agnostic:
        labels = None
    if torch.is_grad_enabled() and (logits.requires_grad or pred_boxes.requires_grad):
        ce, bbox, giou, card = DetectionLossLargeFunction.apply(logits, pred_boxes, pred_idx, tgt_idx, moff, labels, boxes,
                                                                toff, focal_alpha, num_boxes)
    else:
        out, _, _, _ = detection_loss_large_launch(logits.detach().contiguous(), pred_boxes.detach().contiguous(), pred_idx,
                                                   tgt_idx, moff, labels, boxes, toff, focal_alpha, num_boxes,
                                                   want_grad=False)
        sums = out.sum(0)
        ce, bbox, giou, card = sums[0], sums[1], sums[2], out[:, 3]
    return {"loss_ce": ce, "loss_bbox": bbox, "loss_giou": giou,
            "cardinality_error": (card - lengths).abs().mean()}


def _relation_operands(pred_rel, targets, indices, matching_costs, rel_bits):
    """What the relation-loss entries read besides the logits: (target, packed, rels, pred_idx, tgt_idx, match_cost, out_off).
    ``target``: the pointer table of the dense targets (``rels`` keeps their contiguous forms alive until the launches are
    enqueued) or, for ``rel_triplets`` targets, the packed words."""
    dev = pred_rel.device
    packed = not rel_targets.has_dense(targets)
    if packed:
        if any("rel" in t for t in targets):
            raise ValueError('a batch mixes dense "rel" targets and "rel_triplets" targets: convert one kind '
                             "(egtr_amd.targets.dense_targets)")
        if rel_bits is None:   # up to 64 predicates one word per pair, up to 256 the wide words (their rank selects the entry)
            wide = rel_targets.MAX_REL_LABELS < pred_rel.shape[3] <= rel_targets.MAX_PACKED_REL_LABELS
            rel_bits = (rel_targets.pack_relations_wide if wide else rel_targets.pack_relations)(
                targets, pred_rel.shape[1], pred_rel.shape[3], dev)
        target = rel_bits
    else:
        rels = [_chk(t["rel"] if t["rel"].is_contiguous() else t["rel"].contiguous(), "target rel", torch.float32)
                for t in targets]
        target = torch.tensor([r.data_ptr() for r in rels], dtype=torch.int64).to(dev, non_blocking=True)
    offs = [0]
    for src, _ in indices:
        offs.append(offs[-1] + int(src.shape[0]))
    out_off = torch.tensor(offs, dtype=torch.int32).to(dev, non_blocking=True)
    pi = torch.cat([i[0] for i in indices]).to(device=dev, dtype=torch.int64)
    ti = torch.cat([i[1] for i in indices]).to(device=dev, dtype=torch.int64)
    mc = torch.cat(list(matching_costs)).to(device=dev, dtype=torch.float32)
    if pi.numel() == 0:   # keep the kernels' pointers valid
        pi = torch.zeros(1, dtype=torch.int64, device=dev)
        ti = torch.zeros(1, dtype=torch.int64, device=dev)
        mc = torch.zeros(1, dtype=torch.float32, device=dev)
    if not packed:
        return target, packed, rels, pi, ti, mc, out_off
    return target, packed, None, pi, ti, mc, out_off


def relation_losses(pred_rel, pred_conn, targets, indices, matching_costs, nonmatching_cost, sample_negatives,
                    sample_nonmatching, rel_bits=None):
    """(loss_rel, loss_connectivity) for device tensors, the ``sample_*`` largest logits of both candidate classes: see
    RelationLossFunction (the sampler state is neither read nor advanced).  ``indices`` / ``matching_costs``: the
    matcher's per-image device tensors; ``targets[b]["rel"]``: dense fp32 [N, N, R] on the device.  Targets that carry
    ``"rel_triplets"`` and no ``"rel"`` take a packed target format: ``rel_bits`` (``egtr_amd.targets.pack_relations``, or
    ``pack_relations_wide`` for 65 .. 256 predicates: 4-D words are the wide format) when the
    caller packed the batch already, else packed here -- no dense target exists on that route.
    ``sample_negatives`` and ``sample_nonmatching`` both None: the un-sampled loss over all elements
    (RelationLossAllFunction; value-only when nothing requires grad).  Exactly one None is not a kernel route (the criterion
    keeps that configuration on its tensor composition): ValueError."""
    if (sample_negatives is None) != (sample_nonmatching is None):
        raise ValueError("relation_losses takes both sample counts or neither: with exactly one of sample_negatives / "
                         "sample_nonmatching None the criterion's tensor route (_loss_relations_device) evaluates the loss")
    target, packed, rels, pi, ti, mc, out_off = _relation_operands(pred_rel, targets, indices, matching_costs, rel_bits)
    if sample_negatives is None:
        want_grad = torch.is_grad_enabled() and (pred_rel.requires_grad or pred_conn.requires_grad)
        out = RelationLossAllFunction.apply(pred_rel, pred_conn, target, pi, ti, mc, out_off, nonmatching_cost, packed,
                                            want_grad)
    else:
        out = RelationLossFunction.apply(pred_rel, pred_conn, target, pi, ti, mc, out_off, nonmatching_cost,
                                         ("largest", sample_negatives), ("largest", sample_nonmatching), 0, 0, packed)
    del rels   # (kept alive until the launches were enqueued; the caller's targets own the storage)
    return out


def relation_losses_sampled(pred_rel, pred_conn, targets, indices, matching_costs, nonmatching_cost, negatives, nonmatching,
                            rel_bits=None, seed=None, stream=None):
    """(loss_rel, loss_connectivity) with one sampling policy per candidate class (RelationLossFunction): ``negatives`` --
    the false candidates of the matched block -- and ``nonmatching`` -- the elements with an unmatched subject or object -- are
    (policy, count) with policy "largest" (the count n_true largest logits), "random" (a uniform subset of that size) or "all"
    (the whole class; count ignored).  The other arguments as in ``relation_losses``.  ``seed`` / ``stream``: the words of the
    random keys; None takes the sampler state (``relation_sampler_state``), and a launch with a random class then advances the
    stream by one -- whichever sampler is SET: calling this function is asking for the device's selection."""
    target, packed, rels, pi, ti, mc, out_off = _relation_operands(pred_rel, targets, indices, matching_costs, rel_bits)
    random_class = "random" in (negatives[0], nonmatching[0])
    if stream is None:   # the sampler's own stream: consumed by a launch that draws
        cur_seed, stream = _next_relation_stream() if random_class else relation_sampler_state()
    else:
        cur_seed = relation_sampler_state()[0]
    if seed is None:
        seed = cur_seed
    out = RelationLossFunction.apply(pred_rel, pred_conn, target, pi, ti, mc, out_off, nonmatching_cost,
                                     tuple(negatives), tuple(nonmatching), int(seed), int(stream), packed)
    del rels
    return out
